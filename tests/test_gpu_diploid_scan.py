"""GPU: impop_diploid_scan against the plain restatement of tests/plain_diploid.py — every integer and every double, bit for
bit.  What needs the trace line (IMPOP_TRACE=1 is read once per process) runs in one child process per module."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import dip_cases as dc
import plain_diploid as pd
from conftest import ROOT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


def scan(bm, case, **kw):
    return bm.diploid_scan(case.windows, case.pairs, case.min_run, want_individuals=True, **kw)


# ---- the known answer of the header -------------------------------------------------------------------------------------------------

def test_known_answer(ctx):
    bm = ctx.upload_dense(dc.known_matrix(), keep_hap_major=False)
    rec, ind = bm.diploid_scan([(0, 6, 0)], dc.KNOWN_PAIRS, 3, want_individuals=True)
    assert [tuple(int(x) for x in r)[:5] for r in ind[0]] == [(1, 1, 5, 1, 5), (2, 1, 3, 1, 3)]
    r = rec[0]
    assert (r["n_ind"], r["n_sites"], r["s_p"], r["het_sites"], r["het_total"], r["sum_p"]) == (2, 6, 4, 3, 3, 13)
    assert (r["roh_sites_total"], r["roh_runs_total"], r["longest_run"]) == (8, 2, 5)
    assert r["ho"] == 0.25 and r["he"] == 26.0 / 72.0 and r["f_is"] == 1.0 - 9.0 / 13.0 and r["f_roh"] == 8.0 / 12.0
    pd.assert_matches((rec, ind), pd.reference(dc.known_matrix(), dc.KNOWN_PAIRS, [(0, 6, 0)], 3), "known")
    bm.free()


# ---- geometry: tail granules of 1, 2, 3, 4 dwords and more than one full granule; default tiles and tiles of 2 and 5 blocks ----------

@pytest.mark.parametrize("n", (2, 33, 64, 65, 70, 130, 465))
def test_shapes_against_the_restatement(ctx, n, monkeypatch):
    for kind in ("spectrum", "founder"):
        case = dc.geometry_case(n, kind)
        bm = ctx.upload_dense(case.m01, keep_hap_major=False)
        for tile_blocks in (None, 5, 2) if kind == "founder" else (None, 1):
            if tile_blocks is None:
                monkeypatch.delenv("IMPOP_DIPLOID_TILE_BLOCKS", raising=False)
            else:  # a 2100-site window: 33 blocks, 7 tiles of 5 — every wave has a block, one of them two
                monkeypatch.setenv("IMPOP_DIPLOID_TILE_BLOCKS", str(tile_blocks))
            got = scan(bm, case)
            pd.assert_matches(got, case.want, (case.tag, tile_blocks))
            assert bm.diploid_scan(case.windows, case.pairs, case.min_run).tobytes() == got[0].tobytes()  # the records alone
        bm.free()


def test_one_individual(ctx):
    case = dc.geometry_case(70, "founder")
    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    for pair in ((1, 69), (69, 1), (40, 3)):
        got = bm.diploid_scan(case.windows, [pair], 30, want_individuals=True)
        pd.assert_matches(got, pd.reference(case.m01, [pair], case.windows, 30), pair)
    a = bm.diploid_scan(case.windows, [(1, 69)], 30, want_individuals=True)
    b = bm.diploid_scan(case.windows, [(69, 1)], 30, want_individuals=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()  # the order inside a pair changes nothing
    bm.free()


# ---- runs: first and last site, across a block edge, across a tile edge, over a whole tile; min_run at and above a run's length -------

@pytest.mark.parametrize("min_run", (1, dc.RUN_LONG, dc.RUN_LONG + 1))
def test_hand_made_runs(ctx, min_run, monkeypatch):
    case = dc.run_case(min_run)
    rows = case.want[1][0]
    assert rows["het"].tolist()[:2] == [0, len(dc.RUN_HETS)] and rows["longest_run"][0] == dc.RUN_WINDOW[1] - dc.RUN_WINDOW[0]
    if min_run > 1:
        assert rows["roh_runs"].tolist() == [1, 1 if min_run == dc.RUN_LONG else 0, 0]
    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    for tile_blocks in (dc.RUN_TILE_BLOCKS, 1, None):
        if tile_blocks is None:
            monkeypatch.delenv("IMPOP_DIPLOID_TILE_BLOCKS", raising=False)
        else:
            monkeypatch.setenv("IMPOP_DIPLOID_TILE_BLOCKS", str(tile_blocks))
        pd.assert_matches(scan(bm, case), case.want, (case.tag, tile_blocks))
    cm = bm.compact()
    pd.assert_matches(scan(cm, case), case.want, (case.tag, "compact"))
    cm.free()
    bm.free()


# ---- cross-checks against code from before this scan ---------------------------------------------------------------------------------

def test_het_is_the_gram_identity_and_sums_are_the_scan(ctx):
    case = dc.geometry_case(130, "founder")
    bm = ctx.upload_dense(case.m01, keep_hap_major=True)
    wins = [(5, 1061), (700, 2100)]
    rec, ind = bm.diploid_scan(wins, case.pairs, case.min_run, want_individuals=True)
    flags = np.zeros(130, np.uint8)
    flags[[h for p in case.pairs for h in p]] = 1
    old = bm.scan(wins, mask_p=flags)
    assert rec["sum_p"].tolist() == old["sum_p"].tolist() and rec["s_p"].tolist() == old["s_p"].tolist()
    for k, (b, e) in enumerate(wins):
        I = bm.pairwise_counts(b, e).astype(np.int64)
        want = [int(I[i, i] + I[j, j] - 2 * I[i, j]) for i, j in case.pairs]
        assert ind["het"][k].tolist() == want and ind["hom_alt"][k].tolist() == [int(I[i, j]) for i, j in case.pairs]
    bm.free()


# ---- the upper end of the range -------------------------------------------------------------------------------------------------------

def test_2048_individuals(ctx):
    rng = np.random.default_rng(11300)
    m01 = dc.founder_matrix(rng, 4096, 300, nf=5, p_switch=0.01, p_flip=0.004)
    perm = rng.permutation(4096)
    pairs = [(int(a), int(b)) for a, b in zip(perm[0::2], perm[1::2])]
    wins = [(0, 300), (17, 211), (190, 300)]
    want = pd.reference(m01, pairs, wins, 25)
    dc.assert_nontrivial(want[1], "n4096")
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    pd.assert_matches(bm.diploid_scan(wins, pairs, 25, want_individuals=True), want, "n4096")
    bm.free()


# ---- routes, chunks and the trace line, in a child process under IMPOP_TRACE=1 -------------------------------------------------------

def _route_case():
    return dc.geometry_case(465, "spectrum")


def _chunk_windows():
    return [(11 * k, 11 * k + 300) for k in range(100)]


def _child(out_path):
    import impop_amd
    from impop_amd import ImpopError
    ctx = impop_amd.Context(0)
    out = {}

    def call(tag, fn):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        out[tag], out[tag + "_ind"] = fn()
        sys.stderr.flush()

    case = _route_case()
    ups = {"default": {}, "norare": {"rare_split": False}, "dense": {"dense_scan": True}}
    for tag, ukw in ups.items():
        bm = ctx.upload_dense(case.m01, keep_hap_major=False, **ukw)
        call(tag, lambda: scan(bm, case))
        if tag == "default":
            cm = bm.compact()
            out["compact_sites"] = np.array([cm.n_site, bm.n_site])
            call("compact", lambda: scan(cm, case))
            cw = _chunk_windows()
            kw = dict(want_individuals=True)
            call("w100", lambda: bm.diploid_scan(cw, case.pairs, case.min_run, **kw))
            per_win = 80 + 32 + 24 * len(case.pairs) + 40 * len(case.pairs)
            call("chunked", lambda: bm.diploid_scan(cw, case.pairs, case.min_run, max_chunk_bytes=30 * per_win, **kw))
            call("chunked_compact", lambda: cm.diploid_scan(cw, case.pairs, case.min_run, max_chunk_bytes=30 * per_win, **kw))
            call("chunked_1", lambda: bm.diploid_scan(case.windows, case.pairs, case.min_run, max_chunk_bytes=1, **kw))
            cm.free()
        bm.free()
    bm = ctx.upload_dense(np.zeros((8, 200), np.uint8), keep_hap_major=False)
    sys.stderr.write("@@call over\n")
    sys.stderr.flush()
    try:
        bm.diploid_scan([(0, 200)], [(0, 1)] * 2049, 1)
        out["over"] = np.array([0])
    except ImpopError as exc:
        out["over"] = np.array([exc.code])
    bm.free()
    ctx.close()
    np.savez(out_path, **out)


_TRACE = re.compile(r"\[impop_diploid_scan\] (.*)$")


@pytest.fixture(scope="module")
def child():
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
        env.pop("IMPOP_DIPLOID_TILE_BLOCKS", None)
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_diploid_scan as t; t._child(sys.argv[1])", path],
                           capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        z = np.load(path)
        recs = {k: z[k] for k in z.files}
    trace, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@@call "):
            cur = line.split()[1]
            trace[cur] = []
        mt = _TRACE.search(line)
        if mt and cur:
            kv = dict(x.split("=") for x in mt.group(1).split())
            trace[cur].append({k: (v if k == "route" else int(v)) for k, v in kv.items()})
    return recs, trace


def test_uploads_and_compaction_give_identical_bytes(child):
    recs, trace = child
    case = _route_case()
    pd.assert_matches((recs["default"], recs["default_ind"]), case.want, "default")
    for tag in ("norare", "dense", "compact"):
        assert recs[tag].tobytes() == recs["default"].tobytes(), tag
        assert recs[tag + "_ind"].tobytes() == recs["default_ind"].tobytes(), tag
    assert recs["compact_sites"][0] < recs["compact_sites"][1]  # the compacted matrix really is shorter
    assert [trace[t][0]["route"] for t in ("default", "norare", "dense", "compact")] == ["dense", "dense", "dense", "compact"]
    for t in ("default", "compact"):
        assert len(trace[t]) == 1 and trace[t][0]["windows"] == len(case.windows) and trace[t][0]["individuals"] == len(case.pairs)
        assert trace[t][0]["chunks"] == 1 and trace[t][0]["launches"] == 2 and trace[t][0]["tiles"] >= 3
    assert trace["compact"][0]["bytes_streamed"] < trace["default"][0]["bytes_streamed"]


def test_chunking_never_changes_a_record(child):
    recs, trace = child
    case = _route_case()
    assert trace["w100"][0]["chunks"] == 1 and trace["w100"][0]["launches"] == 2
    for tag in ("chunked", "chunked_compact"):
        t = trace[tag][0]
        assert t["chunks"] >= 3 and t["launches"] == 2 * t["chunks"], t
        assert recs[tag].tobytes() == recs["w100"].tobytes() and recs[tag + "_ind"].tobytes() == recs["w100_ind"].tobytes(), tag
    n_empty = sum(1 for w in case.windows if w[0] == w[1])  # a chunk of one window without sites launches the window kernel alone
    t = trace["chunked_1"][0]
    assert t["chunks"] == len(case.windows) and t["launches"] == 2 * t["chunks"] - n_empty
    assert recs["chunked_1"].tobytes() == recs["default"].tobytes() and recs["chunked_1_ind"].tobytes() == recs["default_ind"].tobytes()
    cw = _chunk_windows()
    pick = [0, 1, 29, 30, 31, 59, 60, 99]
    want = pd.reference(case.m01, case.pairs, [cw[k] for k in pick], case.min_run)
    pd.assert_matches((recs["w100"][pick], recs["w100_ind"][pick]), want, "w100")


def test_limit_plus_one_is_refused_before_any_launch(child):
    recs, trace = child
    assert recs["over"].tolist() == [E_UNSUPPORTED] and trace["over"] == []


# ---- errors ---------------------------------------------------------------------------------------------------------------------------

def test_errors_and_empty_input(ctx):
    import ctypes as C

    import impop_amd
    from impop_amd import ImpopError, _lib
    case = dc.geometry_case(33, "founder")
    n, S = case.m01.shape
    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    bad = [([(10, 100)], [], 5), ([(10, 100)], [(0, 1)], 0), ([(10, 100)], [(0, n)], 5), ([(10, 100)], [(n + 7, 1)], 5),
           ([(10, 100)], [(4, 4)], 5), ([(10, 100)], [(0, 1), (2, 0)], 5), ([(10, 100)], [(0, 1), (1, 2)], 5),
           ([(100, 10)], [(0, 1)], 5), ([(10, S + 1)], [(0, 1)], 5)]
    for wins, pairs, min_run in bad:
        with pytest.raises(ImpopError) as ei:
            bm.diploid_scan(wins, pairs, min_run)
        assert ei.value.code == E_INVALID, (wins, pairs, min_run)
    with pytest.raises(ImpopError) as ei:
        bm.diploid_scan([(10, 100)], [(0, 1)] * 2049, 5)
    assert ei.value.code == E_UNSUPPORTED
    w = impop_amd.make_windows([(10, 100)])
    out = np.zeros(1, dtype=impop_amd.DIPLOID_DTYPE)
    pr = np.array([0, 1], dtype=np.uint32)
    prm = _lib.DiploidParams(C.sizeof(_lib.DiploidParams) - 4, 5, 0)  # a wrong struct_size
    rc = ctx._lib.impop_diploid_scan(ctx.handle, bm.handle, w.ctypes.data_as(C.POINTER(_lib.Window)), 1, pr.ctypes.data_as(C.POINTER(C.c_uint32)),
                                     1, C.byref(prm), out.ctypes.data_as(C.POINTER(_lib.DiploidStats)), None)
    assert rc == E_INVALID
    # afterwards the context is still usable
    pd.assert_matches(scan(bm, case), case.want, "after the errors")
    empty = bm.diploid_scan([], case.pairs, 5)
    assert empty.dtype == impop_amd.DIPLOID_DTYPE and len(empty) == 0
    rec, ind = bm.diploid_scan([], case.pairs, 5, want_individuals=True)
    assert len(rec) == 0 and ind.shape == (0, len(case.pairs)) and ind.dtype == impop_amd.DIPLOID_IND_DTYPE
    bm.free()


def test_timers_bracket_the_two_kernels(ctx):
    case = dc.geometry_case(64, "spectrum")
    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    wins = [w for w in case.windows if w[1] > w[0]]
    ctx.gram_timing(True)
    bm.diploid_scan(wins, case.pairs, case.min_run, max_chunk_bytes=1)
    ms, chunks = ctx.diploid_elapsed()
    ctx.gram_timing(False)
    assert chunks == len(wins) and len(ms) == 2 and all(t > 0.0 for t in ms)
    bm.free()


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def test_cli_tables_are_the_records(ctx, tmp_path):
    from impop_amd.matrixio import MatrixFile, save_matrix
    from impop_amd import pack_hap_major
    rng = np.random.default_rng(11700)
    n, W, origin = 24, 900, 5000
    m01 = dc.founder_matrix(rng, n, W)
    names = [f"S{i // 2:02d}#{i % 2 + 1}#chrT:0-1" for i in range(n - 1)] + ["CHM13#0#chrT:0-1"]  # S11 has one copy only
    mpath, bed, indp = str(tmp_path / "m.npz"), str(tmp_path / "w.bed"), str(tmp_path / "ind.tsv")
    save_matrix(mpath, MatrixFile(bits=pack_hap_major(m01), n_site=W, names=names, origin=origin, contig="chrT"))
    rows = [(0, 130), (100, 300), (250, 251), (300, 900), (0, 900)]
    open(bed, "w").write("".join(f"chrT\t{origin + b}\t{origin + e}\n" for b, e in rows))
    pairs = [(2 * i, 2 * i + 1) for i in range(11)]
    rec, ind = pd.reference(m01, pairs, rows, 40)
    dc.assert_nontrivial(ind, "cli")
    want = ["CHROM\tSTART\tEND\tN_IND\tSITES\tHET_SITES\tHO\tHE\tFIS\tROH_RUNS\tF_ROH\tLONGEST_RUN"]
    want_ind = ["CHROM\tSTART\tEND\tSAMPLE\tHET\tHOM_ALT\tLONGEST_RUN\tROH_RUNS\tROH_SITES"]
    fmt = lambda x: "NA" if np.isnan(x) else "%.8f" % x  # noqa: E731
    for k, (b, e) in enumerate(rows):
        r = rec[k]
        head = f"CHM13#0#chrT\t{origin + b}\t{origin + e}"
        want.append("\t".join([head, "11", str(e - b), str(int(r["het_sites"])), fmt(r["ho"]), fmt(r["he"]), fmt(r["f_is"]),
                               str(int(r["roh_runs_total"])), fmt(r["f_roh"]), str(int(r["longest_run"]))]))
        for i in range(11):
            q = ind[k, i]
            want_ind.append("\t".join([head, f"S{i:02d}"] + [str(int(q[f])) for f in ("het", "hom_alt", "longest_run", "roh_runs", "roh_sites")]))
    for extra in ([], ["--compact"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", mpath, "--bed", bed, "--format", "diploid",
                            "--roh-min-sites", "40", "--ind-table", indp] + extra, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout == "\n".join(want) + "\n"
        assert open(indp).read() == "\n".join(want_ind) + "\n"
        warn = [ln for ln in r.stderr.splitlines() if ln.startswith("Warning")]
        assert len(warn) == 1 and "S11#1#chrT:0-1" in warn[0] and "CHM13#0#chrT:0-1" in warn[0]
