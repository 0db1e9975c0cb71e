"""impop_haplotype_scan on an MI355X (run with -m gpu): the distinct haplotypes of every window and the statistics of their
frequencies, against the plain numpy reference of tests/hap_cases.py.  Integers and tables must be equal, doubles within 1e-12
relative.  Everything that needs IMPOP_TRACE=1 or IMPOP_HAPSCAN_KEY_BITS runs in two child processes, once per module."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import hap_cases as hc
from conftest import ROOT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = -1, -5
S = 3000


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


# ---- 1. shapes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (2, 31, 32, 33, 465, 513))
def test_shapes_against_numpy(ctx, n):
    rng = np.random.default_rng(9100 + n)
    m01 = hc.founder_matrix(rng, n, S)
    wins = hc.window_list(S)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    masks = [None, (rng.random(n) < 0.6).astype(np.uint8)]
    masks[1][0] = 1
    one = np.zeros(n, np.uint8)
    one[n // 2] = 1
    same = np.zeros(n, np.uint8)
    same[hc.twins(n)] = 1  # identical from TWIN_FROM on: one class in the windows behind it
    for flags in masks + [one, same]:
        got = bm.haplotype_scan(wins, mask_p=flags, want_members=True)
        ref = hc.reference(m01, flags, wins)
        hc.assert_matches(got, ref, (n, None if flags is None else int(flags.sum())))
        assert np.array_equal(bm.haplotype_scan(wins, mask_p=flags), got[0])  # the records alone
    rec = bm.haplotype_scan(wins)
    k = wins.index(hc.MONO)
    assert rec["n_distinct"][k] == 1 and rec["n_distinct"][wins.index((200, 200))] == 1 and rec["h1"][k] == 1.0
    if n >= 31:
        assert (rec["largest"] > 1).any() and (rec["n_distinct"] > 1).any()
    rec = bm.haplotype_scan(wins, mask_p=same)
    assert rec["n_distinct"][wins.index((hc.TWIN_FROM + 3, S - 5))] == 1
    bm.free()


# ---- 3. the existing engine: impop_cluster_scan at threshold 1.0 ------------------------------------------------------------------

def test_agrees_with_cluster_scan(ctx):
    rng = np.random.default_rng(9300)
    n = 465
    m01 = hc.founder_matrix(rng, n, S)
    wins = [w for w in hc.window_list(S) if w[1] > w[0]] + [(200, 200)]
    flags = (rng.random(n) < 0.7).astype(np.uint8)
    bm = ctx.upload_dense(m01, keep_hap_major=True)
    for f in (None, flags):
        rec, cl, sz = bm.haplotype_scan(wins, mask_p=f, want_members=True)
        crec, ccl, csz = bm.cluster_scan(wins, mask_p=f, threshold=1.0, kind="match", want_members=True)
        for a, b in (("n_members", "n_members"), ("n_distinct", "n_clusters"), ("largest", "largest"), ("n_singletons", "n_singletons"),
                     ("sum_sq", "sum_sq"), ("n_sites", "n_sites")):
            assert np.array_equal(rec[a], crec[b]), (a, f is None)
        assert np.array_equal(cl, ccl) and np.array_equal(sz, csz)
    bm.free()


# ---- 2., 4., 5., 6. under IMPOP_TRACE=1 in child processes ----------------------------------------------------------------------------

ROUTE_N = 465
COLL_NF = 64


def _route_inputs():
    rng = np.random.default_rng(9200)
    m01 = hc.founder_matrix(rng, ROUTE_N, S)
    weights = rng.integers(1, 9, size=S).astype(np.uint32)
    flags = (rng.random(ROUTE_N) < 0.8).astype(np.uint8)
    return m01, weights, flags, hc.window_list(S)


def _collision_inputs():
    rng = np.random.default_rng(9400)
    m01 = hc.founder_matrix(rng, ROUTE_N, S, nf=COLL_NF, p_site=0.12)
    wins = [(b, b + 700) for b in range(5, S - 700, 180)] + [(0, S)]
    return m01, wins


def _chunk_windows():
    return [(7 * k, 7 * k + 330) for k in range(300)]


def _flags(idx, n):
    f = np.zeros(n, np.uint8)
    f[np.asarray(idx, dtype=np.int64)] = 1
    return f


def _child(out_path, mode):
    import impop_amd
    from impop_amd import ImpopError
    ctx = impop_amd.Context(0)
    out = {}

    def call(tag, fn):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        r = fn()
        sys.stderr.flush()
        return r

    def keep(tag, res):
        out[tag], out[tag + "_cl"], out[tag + "_sz"] = res

    cm01, cwins = _collision_inputs()
    cbm = ctx.upload_dense(cm01, keep_hap_major=False)
    keep("coll", call("coll", lambda: cbm.haplotype_scan(cwins, want_members=True)))
    cbm.free()
    if mode == "full":
        m01, weights, flags, wins = _route_inputs()
        ups = {"indexed": {}, "norare": {"rare_split": False}, "dense": {"dense_scan": True}}
        for tag, kw in ups.items():
            bm = ctx.upload_dense(m01, keep_hap_major=False, **kw)
            keep(tag, call(tag, lambda: bm.haplotype_scan(wins, mask_p=flags, want_members=True)))
            if tag == "indexed":
                cm = bm.compact()
                keep("compact", call("compact", lambda: cm.haplotype_scan(wins, mask_p=flags, want_members=True)))
                cm.free()
                cw = _chunk_windows()
                out["w300"] = call("w300", lambda: bm.haplotype_scan(cw, mask_p=flags))
                out["w30"] = call("w30", lambda: bm.haplotype_scan(cw[:30], mask_p=flags))
                out["chunked"] = call("chunked", lambda: bm.haplotype_scan(cw, mask_p=flags, max_chunk_bytes=110 * 12 * int(flags.sum())))
                keep("chunked_t", call("chunked_t", lambda: bm.haplotype_scan(wins, mask_p=flags, want_members=True, max_chunk_bytes=1)))
            bm.free()
        bm = ctx.upload_dense(m01, keep_hap_major=False)
        bm.set_site_weights(weights)
        keep("weighted", call("weighted", lambda: bm.haplotype_scan(wins, mask_p=flags, want_members=True)))
        bm.free()
        big = ctx.upload_dense(np.zeros((4097, 200), np.uint8), keep_hap_major=False)
        try:
            call("over", lambda: big.haplotype_scan([(0, 200)]))
            out["over"] = np.array([0])
        except ImpopError as exc:
            out["over"] = np.array([exc.code])
        out["subset"] = call("subset", lambda: big.haplotype_scan([(0, 200)], mask_p=_flags(np.arange(1, 4097), 4097)))
        big.free()
    ctx.close()
    np.savez(out_path, **out)


_TRACE = re.compile(r"\[impop_haplotype_scan\] (.*)$")


def _run_child(mode, env_extra):
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]), **env_extra)
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_haplotype_scan as t; t._child(sys.argv[1], sys.argv[2])", path, mode],
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


@pytest.fixture(scope="module")
def child():
    return _run_child("full", {})


@pytest.fixture(scope="module")
def child_short_keys():
    return _run_child("coll", {"IMPOP_HAPSCAN_KEY_BITS": "4"})


def test_routes_give_identical_bytes(child):
    recs, trace = child
    m01, weights, flags, wins = _route_inputs()
    ref = hc.reference(m01, flags, wins)
    hc.assert_matches((recs["indexed"], recs["indexed_cl"], recs["indexed_sz"]), ref, "indexed")
    for tag in ("norare", "dense", "compact"):
        assert recs[tag].tobytes() == recs["indexed"].tobytes(), tag
        assert recs[tag + "_cl"].tobytes() == recs["indexed_cl"].tobytes() and recs[tag + "_sz"].tobytes() == recs["indexed_sz"].tobytes(), tag
    # site weights change W and nothing else
    hc.assert_matches((recs["weighted"], recs["weighted_cl"], recs["weighted_sz"]), hc.reference(m01, flags, wins, weights), "weighted")
    a, b = recs["weighted"].copy(), recs["indexed"].copy()
    a["n_sites"] = b["n_sites"] = 0
    assert a.tobytes() == b.tobytes()
    assert [trace[t][0]["route"] for t in ("indexed", "norare", "dense", "compact", "weighted")] == \
        ["indexed+rare", "indexed", "dense", "compact", "dense"]
    for t in ("indexed", "norare", "dense", "compact", "weighted"):
        assert len(trace[t]) == 1 and trace[t][0]["windows"] == len(wins) and trace[t][0]["collided_windows"] == 0
    assert max(trace["indexed"][0]["bytes_streamed"], trace["norare"][0]["bytes_streamed"]) < trace["dense"][0]["bytes_streamed"]


def test_collisions_take_the_exact_path(child, child_short_keys):
    recs, trace = child
    srecs, strace = child_short_keys
    m01, wins = _collision_inputs()
    ref = hc.reference(m01, None, wins)
    assert (ref[0]["n_distinct"] >= 40).all()
    hc.assert_matches((recs["coll"], recs["coll_cl"], recs["coll_sz"]), ref, "128 bits")
    assert trace["coll"][0]["collided_windows"] == 0
    assert strace["coll"][0]["collided_windows"] > 0  # 16 keys for 40 and more haplotypes
    for k in ("coll", "coll_cl", "coll_sz"):
        assert srecs[k].tobytes() == recs[k].tobytes(), k


def test_chunking_never_changes_a_record(child):
    recs, trace = child
    assert trace["w300"][0]["chunks"] == 1 and trace["chunked"][0]["chunks"] >= 3
    assert recs["chunked"].tobytes() == recs["w300"].tobytes()
    assert recs["w300"][:30].tobytes() == recs["w30"].tobytes()
    _, _, _, wins = _route_inputs()
    assert trace["chunked_t"][0]["chunks"] == len(wins)  # a budget of one byte: a chunk per window
    for k in ("", "_cl", "_sz"):
        assert recs["chunked_t" + k].tobytes() == recs["indexed" + k].tobytes()
    m01, _, flags, _ = _route_inputs()
    cw = _chunk_windows()
    pick = [0, 1, 29, 30, 109, 110, 111, 299]
    want = hc.reference(m01, flags, [cw[k] for k in pick])[0]
    for name in hc.INTEGERS:
        assert np.array_equal(recs["w300"][name][pick].astype(np.uint64), want[name]), name


def test_launches_do_not_depend_on_the_number_of_windows(child):
    _, trace = child
    (a,), (b,) = trace["w30"], trace["w300"]
    assert a["windows"] == 30 and b["windows"] == 300 and a["chunks"] == b["chunks"] == 1
    assert a["launches"] == b["launches"] and 1 <= a["launches"] <= 4
    assert trace["chunked"][0]["launches"] == a["launches"] * trace["chunked"][0]["chunks"]


# ---- 6. limits ----------------------------------------------------------------------------------------------------------------

def test_4096_members(ctx):
    from impop_amd import _lib
    assert _lib.HAPLOTYPE_MAX_N == 4096
    rng = np.random.default_rng(9600)
    n, W = 4096, 400
    m01 = hc.founder_matrix(rng, n, W, p_site=0.08, p_flip=2e-5)
    wins = [(0, W), (37, 165), (100, 101), (64, 64), (300, 400)]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    hc.assert_matches(bm.haplotype_scan(wins, want_members=True), hc.reference(m01, None, wins), "4096")
    dm = ctx.upload_dense(m01, keep_hap_major=False, dense_scan=True)
    assert dm.haplotype_scan(wins).tobytes() == bm.haplotype_scan(wins).tobytes()
    dm.free()
    bm.free()
    # every member a class of its own: the ranking and the tables at their largest
    ids = ((np.arange(n)[:, None] >> np.arange(12)[None, :]) & 1).astype(np.uint8)
    bm = ctx.upload_dense(ids, keep_hap_major=False)
    got = bm.haplotype_scan([(0, 12), (0, 11)], want_members=True)
    hc.assert_matches(got, hc.reference(ids, None, [(0, 12), (0, 11)]), "all distinct")
    assert got[0]["n_distinct"].tolist() == [4096, 2048]
    bm.free()


def test_limit_plus_one_is_refused_before_any_launch(child):
    recs, trace = child
    assert recs["over"].tolist() == [E_UNSUPPORTED] and trace["over"] == []
    assert len(trace["subset"]) == 1 and recs["subset"]["n_members"].tolist() == [4096] and recs["subset"]["n_distinct"].tolist() == [1]


def test_errors_and_empty_input(ctx):
    import impop_amd
    from impop_amd import ImpopError
    rng = np.random.default_rng(9700)
    n, W = 40, 300
    bm = ctx.upload_dense(hc.founder_matrix(rng, n, W), keep_hap_major=False)
    for wins, kw in (([(100, 10)], {}), ([(10, W + 1)], {}), ([(10, 100)], {"mask_p": np.zeros(n, np.uint8)})):
        with pytest.raises(ImpopError) as ei:
            bm.haplotype_scan(wins, **kw)
        assert ei.value.code == E_INVALID, (wins, kw)
    empty = bm.haplotype_scan([])
    assert empty.dtype == impop_amd.HAPLOTYPE_DTYPE and len(empty) == 0
    rec, cl, sz = bm.haplotype_scan([], want_members=True)
    assert len(rec) == 0 and cl.shape == (0, n) and sz.shape == (0, n)
    bm.free()


# ---- 7. the command line ------------------------------------------------------------------------------------------------------------

def test_cli_rows_are_the_records(ctx, tmp_path):
    from impop_amd.matrixio import MatrixFile, save_matrix
    from impop_amd import pack_hap_major
    rng = np.random.default_rng(9800)
    n, W, origin = 40, 900, 5000
    m01 = hc.founder_matrix(rng, n, W, nf=5, p_site=0.1, p_flip=0.002)
    names = [f"S{i:02d}#1#chrT:0-1" for i in range(n)]
    mpath, bed, sub = str(tmp_path / "m.npz"), str(tmp_path / "w.bed"), str(tmp_path / "u.txt")
    save_matrix(mpath, MatrixFile(bits=pack_hap_major(m01), n_site=W, names=names, origin=origin, contig="chrT"))
    rows = [(0, 130), (100, 300), (250, 251), (300, 900), (837, 900)]
    open(bed, "w").write("".join(f"chrT\t{origin + b}\t{origin + e}\n" for b, e in rows))
    keep = sorted(rng.choice(n, 31, replace=False).tolist())
    open(sub, "w").write("".join(names[i].partition("chrT")[0] + "\n" for i in keep))
    bm = ctx.upload_dense(m01, keep_hap_major=False)

    def table(recs):
        out = ["REGION\tLENGTH\tSAMPLES\tSITES\tHAPLOTYPES\tH1\tH12\tH2_H1\tHAP_DIVERSITY"]
        for (b, e), r in zip(rows, recs):
            out.append("\t".join([f"CHM13#0#chrT:{origin + b}-{origin + e}", str(e - b), str(int(r["n_members"])), str(int(r["n_sites"])),
                                  str(int(r["n_distinct"]))] + ["%.8f" % float(r[k]) for k in hc.DOUBLES]))
        return "\n".join(out) + "\n"

    def run(extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", mpath, "--bed", bed, "--format", "hapstats"]
                           + extra, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout

    full = bm.haplotype_scan(rows)
    hc.assert_matches(bm.haplotype_scan(rows, want_members=True), hc.reference(m01, None, rows), "cli")
    assert run([]) == table(full) and run(["--compact"]) == table(full)
    assert run(["-u", sub]) == table(bm.haplotype_scan(rows, mask_p=_flags(keep, n)))
    bm.free()
