"""GPU: impop_ibs_scan against the plain restatement of tests/plain_ibs.py — every integer and the double, bit for bit.  What needs
the trace line (IMPOP_TRACE=1 is read once per process) runs in one child process."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import dip_cases as dc
import ibs_cases as ic
import plain_ibs as pi
from conftest import ROOT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = -1, -5
ENVS = ("IMPOP_IBS_CHUNK_BLOCKS", "IMPOP_IBS_SEG_BLOCKS")


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


def set_blocks(monkeypatch, chunk, seg):
    for name, v in zip(ENVS, (chunk, seg)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))


def scan(bm, case, **kw):
    args = dict(min_sites=case.min_sites, site_begin=case.b, site_end=case.e, windows=case.windows)
    if case.mask is not None:
        args["mask_p"] = case.mask
    elif case.pairs != pi.all_pairs(range(case.m01.shape[0])):
        args["pairs"] = case.pairs
    args.update(kw)
    return bm.ibs_scan(**args)[:3]


def same_bytes(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- the known answer of the header -------------------------------------------------------------------------------------------------

def test_known_answer(ctx):
    bm = ctx.upload_dense(ic.known_matrix(), keep_hap_major=False)
    rec, seg, win, total = bm.ibs_scan(min_sites=ic.KNOWN_MIN_SITES, windows=ic.KNOWN_WINDOWS)
    assert [tuple(int(x) for x in r) for r in rec] == ic.KNOWN_PAIR_ROWS
    assert [tuple(int(x) for x in s) for s in seg] == ic.KNOWN_SEGMENTS and total == 6
    assert [(int(w["pair_sites"]), int(w["tracts"]), int(w["pairs_spanning"])) for w in win] == ic.KNOWN_WINDOW_ROWS
    assert win["share"].tolist() == [19.0 / 36.0, 1.0, 0.5] and win["n_sites"].tolist() == [6, 2, 3]
    pi.assert_matches((rec, seg, win), pi.reference(ic.known_matrix(), pi.all_pairs(range(4)), 0, 6, 2, ic.KNOWN_WINDOWS), "known")
    bm.free()


# ---- geometry: pair-tile edges, tail granules of 1..4 dwords, 32-row ballot groups; chunks and sub-segments of 1, 2, 5 blocks ---------

@pytest.mark.parametrize("n", (2, 33, 64, 65, 70, 130))
def test_shapes_against_the_restatement(ctx, n, monkeypatch):
    bm = ctx.upload_dense(ic.geometry_matrix(n), keep_hap_major=False)
    for min_sites in (1, 7, 65):
        case = ic.geometry_case(n, min_sites)
        settings = ((None, None), (1, 1), (2, 1), (5, 2), (None, 5)) if min_sites == 7 else ((None, None), (2, 1))
        for chunk, seg in settings:
            set_blocks(monkeypatch, chunk, seg)
            pi.assert_matches(scan(bm, case), case.want, (case.tag, chunk, seg))
    set_blocks(monkeypatch, None, None)
    # totals only: the same pair and window records, no list
    rec, seg, win, total = bm.ibs_scan(min_sites=case.min_sites, site_begin=case.b, site_end=case.e, windows=case.windows, want_segments=False)
    assert seg is None and total == len(case.want[1])
    pi.assert_same(rec, case.want[0], "totals")
    pi.assert_same(win, case.want[2], "totals")
    # no windows; the whole matrix as the range (site_end = 0)
    whole = pi.reference(case.m01, case.pairs, 0, ic.GEO_S, 7)
    pi.assert_matches(bm.ibs_scan(min_sites=7)[:3], whole, "whole")
    bm.free()


# ---- hand-made rows -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_sites", (1, ic.HAND_LONG, ic.HAND_LONG + 1))
def test_hand_made_rows(ctx, min_sites, monkeypatch):
    case = ic.hand_case(min_sites)
    b, e = ic.HAND_RANGE
    rec, seg, _ = case.want
    both = seg[seg["pair"] == 0]
    assert len(both) == 1 and tuple(both[0])[2:] == (b, e, 0, 3)          # identical rows: the range, open on both sides
    assert rec["longest"][1] == 0 and not (seg["pair"] == 1).any()       # different everywhere: nothing
    if min_sites > 1:
        assert rec["n_tracts"].tolist()[2:4] == ([1, 1] if min_sites == ic.HAND_LONG else [0, 0])
    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    for chunk, sg in ((ic.HAND_CHUNK_BLOCKS, ic.HAND_SEG_BLOCKS), (1, 1), (3, 2), (None, None)):
        set_blocks(monkeypatch, chunk, sg)
        pi.assert_matches(scan(bm, case), case.want, (case.tag, chunk, sg))
    cm = bm.compact()
    pi.assert_matches(scan(cm, case), case.want, (case.tag, "compact"))
    cm.free()
    bm.free()


# ---- uploads, weights, chunks and compaction never change a byte -----------------------------------------------------------------------

def test_invariance(ctx, monkeypatch):
    set_blocks(monkeypatch, None, None)
    rng = np.random.default_rng(20300)
    n, S = 70, 2100
    m01 = dc.founder_matrix(rng, n, S, nf=4)
    mono = rng.random(S) < 0.4  # monomorphic sites, all 0 or all 1: a compacted matrix really is shorter
    m01[:, mono] = (rng.random(int(mono.sum())) < 0.3).astype(np.uint8)[None, :]
    case = ic.Case("inv", m01, pi.all_pairs(range(n)), (5, 2093), 20, ic.window_list(5, 2093))
    base = None
    for ukw in ({"keep_hap_major": False}, {"keep_hap_major": True}, {"keep_hap_major": False, "dense_scan": True},
                {"keep_hap_major": False, "rare_split": False}):
        bm = ctx.upload_dense(m01, **ukw)
        got = scan(bm, case)
        if base is None:
            base = got
            pi.assert_matches(got, case.want, "inv")
            # several site chunks and several pair ranges of the segment staging
            small = scan(bm, case, max_chunk_bytes=2 * 5 * n * 8)
            assert same_bytes(small, base)
            cm = bm.compact()
            assert cm.n_site < bm.n_site
            assert same_bytes(scan(cm, case), base) and same_bytes(scan(cm, case, max_chunk_bytes=4096), base)
            cm.free()
            # weights: all ones changes nothing; others change n_sites alone, as the restatement says
            bm.set_site_weights(np.ones(S, dtype=np.uint32))
            assert same_bytes(scan(bm, case), base)
            wts = rng.integers(1, 5, size=S).astype(np.uint32)
            bm.set_site_weights(wts)
            got_w = scan(bm, case)
            assert same_bytes(got_w[:2], base[:2])
            pi.assert_same(got_w[2], pi.reference(m01, case.pairs, case.b, case.e, case.min_sites, case.windows, weights=wts)[2], "weighted")
            cw = bm.compact()
            assert same_bytes(scan(cw, case), got_w)
            cw.free()
        else:
            assert same_bytes(got, base), ukw
        bm.free()


# ---- the capacity protocol -------------------------------------------------------------------------------------------------------------

def test_capacity(ctx):
    import impop_amd
    from impop_amd import _lib
    case = ic.geometry_case(33, 7)
    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    total = len(case.want[1])
    w = impop_amd.make_windows(case.windows)
    prm = _lib.IbsParams(C.sizeof(_lib.IbsParams), case.min_sites, case.b, case.e, 0)
    for cap in (total - 1, 0, total, total + 5):
        rec = np.zeros(len(case.pairs), dtype=impop_amd.IBS_PAIR_DTYPE)
        win = np.zeros(len(w), dtype=impop_amd.IBS_WINDOW_DTYPE)
        seg = np.full(total + 5, 0xA5, dtype=np.uint8).repeat(32).view(impop_amd.IBS_SEGMENT_DTYPE)
        canary = seg.tobytes()
        n_seg = C.c_uint64(0)
        rc = ctx._lib.impop_ibs_scan(ctx.handle, bm.handle, None, None, 0, w.ctypes.data_as(C.POINTER(_lib.Window)), len(w), C.byref(prm),
                                     rec.ctypes.data_as(C.POINTER(_lib.IbsPair)), seg.ctypes.data_as(C.POINTER(_lib.IbsSegment)), cap,
                                     C.byref(n_seg), win.ctypes.data_as(C.POINTER(_lib.IbsWindow)))
        assert rc == 0 and n_seg.value == total
        pi.assert_same(rec, case.want[0], cap)
        pi.assert_same(win, case.want[2], cap)
        if cap < total:
            assert seg.tobytes() == canary  # untouched
        else:
            pi.assert_same(seg[:total], case.want[1], cap)
            assert seg[total:].tobytes() == canary[total * 32:]
    # the method: a caller-given capacity
    assert bm.ibs_scan(min_sites=7, site_begin=case.b, site_end=case.e, seg_capacity=total - 1)[1] is None
    pi.assert_same(bm.ibs_scan(min_sites=7, site_begin=case.b, site_end=case.e, seg_capacity=total)[1], case.want[1], "capacity")
    bm.free()


# ---- cross-checks against code from before this call ----------------------------------------------------------------------------------

def test_cross_checks(ctx):
    case = ic.geometry_case(70, 7)
    n = 70
    bm = ctx.upload_dense(case.m01, keep_hap_major=True)
    b, e = case.b, case.e
    rec = bm.ibs_scan(min_sites=7, site_begin=b, site_end=e, want_segments=False)[0]
    I = bm.pairwise_counts(b, e).astype(np.int64)
    assert rec["n_diff"].tolist() == [int(I[i, i] + I[j, j] - 2 * I[i, j]) for i, j in case.pairs]
    # disjoint pairs, one window = the range: the rows of impop_diploid_scan
    rng = np.random.default_rng(20400)
    perm = [int(x) for x in rng.permutation(n)]
    pairs = list(zip(perm[0::2], perm[1::2]))
    _, ind = bm.diploid_scan([(b, e)], pairs, 7, want_individuals=True)
    mine = bm.ibs_scan(pairs=pairs, min_sites=7, site_begin=b, site_end=e, want_segments=False)[0]
    assert mine["n_tracts"].tolist() == ind["roh_runs"][0].tolist() and mine["tract_sites"].tolist() == ind["roh_sites"][0].tolist()
    assert mine["longest"].tolist() == ind["longest_run"][0].tolist() and mine["n_diff"].tolist() == ind["het"][0].tolist()
    # pairs identical on a window: the classes of impop_haplotype_scan
    mask = np.zeros(n, np.uint8)
    mask[perm[:50]] = 1
    wins = [w for w in case.windows if w[1] - w[0] >= 7]
    hap = bm.haplotype_scan(wins, mask_p=mask)
    win = bm.ibs_scan(mask_p=mask, min_sites=7, site_begin=b, site_end=e, windows=wins, want_segments=False)[2]
    assert win["pairs_spanning"].tolist() == [int((int(h["sum_sq"]) - int(h["n_members"])) // 2) for h in hap]
    assert (win["pairs_spanning"] > 0).any()
    bm.free()


# ---- the list form ---------------------------------------------------------------------------------------------------------------------

def test_list_form(ctx, monkeypatch):
    case = ic.geometry_case(70, 7)
    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    b, e = case.b, case.e
    pairs = [(3, 69), (69, 3), (3, 69), (0, 69), (5, 6), (6, 5), (3, 4), (3, 40), (3, 65), (33, 3), (64, 31), (0, 1)]
    want = pi.reference(case.m01, pairs, b, e, 7, case.windows)
    for chunk, seg in ((None, None), (2, 1)):
        set_blocks(monkeypatch, chunk, seg)
        got = bm.ibs_scan(pairs=pairs, min_sites=7, site_begin=b, site_end=e, windows=case.windows)[:3]
        pi.assert_matches(got, want, ("list", chunk))
    set_blocks(monkeypatch, None, None)
    rec, seg = got[0], got[1]
    for f in ("n_diff", "longest", "n_tracts", "tract_sites"):  # (h2, h1): nothing but the two fields changes
        assert rec[f][0] == rec[f][1] == rec[f][2] and rec[f][4] == rec[f][5]
    a, c = seg[seg["pair"] == 4], seg[seg["pair"] == 5]
    assert len(a) and a["begin"].tolist() == c["begin"].tolist() and a["h1"].tolist() == c["h2"].tolist()
    # more than one tile of the list: 300 pairs, every haplotype in many
    rng = np.random.default_rng(20500)
    many = [(int(x), int(y)) for x, y in rng.integers(0, 70, size=(400, 2)) if x != y][:300]
    pi.assert_matches(bm.ibs_scan(pairs=many, min_sites=7, site_begin=b, site_end=e, windows=case.windows)[:3],
                      pi.reference(case.m01, many, b, e, 7, case.windows), "list300")
    # a mask subset against the same pairs given as a list
    members = sorted(int(x) for x in rng.permutation(70)[:23])
    mask = np.zeros(70, np.uint8)
    mask[members] = 1
    by_mask = bm.ibs_scan(mask_p=mask, min_sites=7, site_begin=b, site_end=e, windows=case.windows)[:3]
    by_list = bm.ibs_scan(pairs=pi.all_pairs(members), min_sites=7, site_begin=b, site_end=e, windows=case.windows)[:3]
    assert same_bytes(by_mask, by_list)
    pi.assert_matches(by_mask, pi.reference(case.m01, pi.all_pairs(members), b, e, 7, case.windows), "mask")
    bm.free()


# ---- the upper end of the range -------------------------------------------------------------------------------------------------------

def test_4096_haplotypes_all_pairs(ctx):
    rng = np.random.default_rng(20600)
    n, S, min_sites = 4096, 256, 60
    m01 = dc.founder_matrix(rng, n, S, nf=6, p_switch=0.01, p_flip=0.004)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    rec, seg, _, total = bm.ibs_scan(min_sites=min_sites)
    n_pairs = n * (n - 1) // 2
    assert n_pairs == 8386560 and len(rec) == n_pairs
    f = m01.astype(np.float32)
    G = (f @ f.T).astype(np.int64)  # exact: counts <= 256
    c = m01.sum(axis=1).astype(np.int64)
    iu, ju = np.triu_indices(n, 1)  # i-major
    assert np.array_equal(rec["n_diff"], (c[iu] + c[ju] - 2 * G[iu, ju]).astype(np.uint32))
    assert np.array_equal(rec["h1"], iu.astype(np.uint32)) and np.array_equal(rec["h2"], ju.astype(np.uint32))
    assert total == len(seg) == int(rec["n_tracts"].sum(dtype=np.int64)) > 0
    off = np.concatenate([[0], np.cumsum(rec["n_tracts"], dtype=np.int64)])
    assert np.array_equal(seg["pair"], np.repeat(np.arange(n_pairs, dtype=np.uint32), rec["n_tracts"]))
    pick = np.sort(rng.choice(n_pairs, size=2000, replace=False))
    want = pi.reference(m01, [(int(iu[p]), int(ju[p])) for p in pick], 0, S, min_sites)
    got_rec = rec[pick].copy()
    pi.assert_same(got_rec, want[0], "n4096 pairs")
    got_seg = np.concatenate([seg[off[p]:off[p + 1]] for p in pick])
    w_seg = want[1].copy()
    w_seg["pair"] = pick[w_seg["pair"]]
    pi.assert_same(got_seg, w_seg, "n4096 segments")
    assert (want[0]["n_tracts"] > 0).any() and (want[0]["n_tracts"] == 0).any()
    bm.free()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def test_refusals(ctx):
    import impop_amd
    from impop_amd import ImpopError, _lib
    case = ic.geometry_case(33, 7)
    n, S = case.m01.shape
    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    one = np.zeros(n, np.uint8)
    one[4] = 1
    bad = [dict(min_sites=0), dict(min_sites=5, site_begin=100, site_end=100), dict(min_sites=5, site_begin=200, site_end=100),
           dict(min_sites=5, site_end=S + 1), dict(min_sites=5, site_begin=S), dict(min_sites=5, pairs=[(4, 4)]),
           dict(min_sites=5, pairs=[(0, n)]), dict(min_sites=5, pairs=[(n + 7, 1)]), dict(min_sites=5, pairs=[(0, 1)], mask_p=np.ones(n, np.uint8)),
           dict(min_sites=5, mask_p=one), dict(min_sites=5, mask_p=np.zeros(n, np.uint8)),
           dict(min_sites=5, site_begin=10, site_end=500, windows=[(9, 100)]), dict(min_sites=5, site_begin=10, site_end=500, windows=[(400, 501)]),
           dict(min_sites=5, site_begin=10, site_end=500, windows=[(300, 200)])]
    for kw in bad:
        with pytest.raises(ImpopError) as ei:
            bm.ibs_scan(**kw)
        assert ei.value.code == E_INVALID, kw
    with pytest.raises(ImpopError) as ei:
        bm.ibs_scan(pairs=np.tile(np.array([[0, 1]], dtype=np.uint32), (_lib.IBS_MAX_PAIRS + 1, 1)), min_sites=5)
    assert ei.value.code == E_UNSUPPORTED
    # raw calls: a wrong struct_size; windows without win_out and the reverse
    w = impop_amd.make_windows([(10, 100)])
    rec = np.zeros(n * (n - 1) // 2, dtype=impop_amd.IBS_PAIR_DTYPE)
    win = np.zeros(1, dtype=impop_amd.IBS_WINDOW_DTYPE)
    n_seg = C.c_uint64(0)

    def raw(prm, windows, win_out):
        return ctx._lib.impop_ibs_scan(ctx.handle, bm.handle, None, None, 0, windows, 1 if windows is not None else 0, C.byref(prm),
                                       rec.ctypes.data_as(C.POINTER(_lib.IbsPair)), None, 0, C.byref(n_seg), win_out)

    good = _lib.IbsParams(C.sizeof(_lib.IbsParams), 5, 0, 0, 0)
    wp, wo = w.ctypes.data_as(C.POINTER(_lib.Window)), win.ctypes.data_as(C.POINTER(_lib.IbsWindow))
    assert raw(_lib.IbsParams(C.sizeof(_lib.IbsParams) - 4, 5, 0, 0, 0), wp, wo) == E_INVALID
    assert raw(good, wp, None) == E_INVALID and raw(good, None, wo) == E_INVALID
    assert raw(good, wp, wo) == 0
    # afterwards the context is still usable
    pi.assert_matches(scan(bm, case), case.want, "after the refusals")
    bm.free()
    big = ctx.upload_dense(np.zeros((_lib.IBS_MAX_N + 1, 64), np.uint8), keep_hap_major=False)
    with pytest.raises(ImpopError) as ei:
        big.ibs_scan(min_sites=5)
    assert ei.value.code == E_UNSUPPORTED
    big.free()


def test_timers_bracket_the_three_kernels(ctx, monkeypatch):
    set_blocks(monkeypatch, 5, 2)
    case = ic.geometry_case(64, 7)
    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    ctx.gram_timing(True)
    scan(bm, case, seg_capacity=len(case.want[1]))
    ms, chunks = ctx.ibs_elapsed()
    ctx.gram_timing(False)
    assert chunks == 2 * 7 and len(ms) == 3 and all(t > 0.0 for t in ms)  # 33 blocks in chunks of 5, two sweeps
    bm.free()


# ---- the trace line, in a child process under IMPOP_TRACE=1 ----------------------------------------------------------------------------

def _child(out_path):
    import impop_amd
    from impop_amd import ImpopError
    ctx = impop_amd.Context(0)
    out = {}
    case = ic.geometry_case(65, 7)

    def call(tag, fn):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        r = fn()
        out[tag + "_rec"], out[tag + "_seg"] = r[0], r[1] if r[1] is not None else np.zeros(0)
        sys.stderr.flush()

    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    kw = dict(min_sites=7, site_begin=case.b, site_end=case.e)
    call("totals", lambda: bm.ibs_scan(want_segments=False, **kw))
    call("fill", lambda: bm.ibs_scan(seg_capacity=len(case.want[1]), **kw))
    call("chunked", lambda: bm.ibs_scan(seg_capacity=len(case.want[1]), max_chunk_bytes=2 * 4 * 65 * 8, **kw))
    call("list", lambda: bm.ibs_scan(pairs=[(0, 1), (2, 64)], want_segments=False, **kw))
    cm = bm.compact()
    call("compact", lambda: cm.ibs_scan(want_segments=False, **kw))
    cm.free()
    sys.stderr.write("@@call refused\n")
    sys.stderr.flush()
    try:
        bm.ibs_scan(min_sites=0)
        out["refused"] = np.array([0])
    except ImpopError as exc:
        out["refused"] = np.array([exc.code])
    bm.free()
    ctx.close()
    np.savez(out_path, **out)


_TRACE = re.compile(r"\[impop_ibs_scan\] (.*)$")


def test_trace_line():
    case = ic.geometry_case(65, 7)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
        for name in ENVS:
            env.pop(name, None)
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_ibs_scan as t; t._child(sys.argv[1])", path],
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
    n_pairs, total = 65 * 64 // 2, len(case.want[1])
    for tag in ("totals", "fill", "chunked", "compact"):
        assert recs[tag + "_rec"].tobytes() == case.want[0].tobytes(), tag
    assert recs["fill_seg"].tobytes() == case.want[1].tobytes() == recs["chunked_seg"].tobytes()
    assert [len(trace[t]) for t in ("totals", "fill", "chunked", "list", "compact", "refused")] == [1, 1, 1, 1, 1, 0]
    assert recs["refused"].tolist() == [E_INVALID]
    t = trace["totals"][0]
    assert list(t) == ["route", "pairs", "site_chunks", "sub_segments", "launches", "tracts", "bytes_streamed"]
    assert t["route"] == "dense" and t["pairs"] == n_pairs and t["tracts"] == total and t["site_chunks"] == 1
    assert t["launches"] == 3 + 1 and t["sub_segments"] >= 1  # transpose, walk, combine; close
    f = trace["fill"][0]
    assert f["site_chunks"] == 2 and f["launches"] == 4 + 5 and f["bytes_streamed"] > t["bytes_streamed"]
    c = trace["chunked"][0]  # chunks of 4 blocks: 9 per sweep, and more than one pair range of the staging
    assert c["site_chunks"] >= 3 * 9 and c["tracts"] == total
    assert trace["list"][0]["pairs"] == 2 and trace["list"][0]["route"] == "dense"
    assert trace["compact"][0]["route"] == "compact" and trace["compact"][0]["bytes_streamed"] <= t["bytes_streamed"]


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def test_cli_tables_are_the_records(tmp_path):
    from impop_amd.matrixio import MatrixFile, save_matrix
    from impop_amd import pack_hap_major
    rng = np.random.default_rng(20700)
    n, W, origin = 24, 900, 5000
    m01 = dc.founder_matrix(rng, n, W)
    names = [f"S{i // 2:02d}#{i % 2 + 1}#chrT:0-1" for i in range(n - 1)] + ["CHM13#0#chrT:0-1"]  # S11 has one copy only
    mpath, bed, segp, pairp = str(tmp_path / "m.npz"), str(tmp_path / "w.bed"), str(tmp_path / "seg.tsv"), str(tmp_path / "pairs.tsv")
    save_matrix(mpath, MatrixFile(bits=pack_hap_major(m01), n_site=W, names=names, origin=origin, contig="chrT"))
    rows = [(0, 130), (100, 300), (250, 251), (300, 900), (0, 900)]
    open(bed, "w").write("".join(f"chrT\t{origin + b}\t{origin + e}\n" for b, e in rows))
    for mode, pairs in (("all", pi.all_pairs(range(n))), ("diploid", [(2 * i, 2 * i + 1) for i in range(11)])):
        rec, seg, win = pi.reference(m01, pairs, 0, W, 40, rows)
        ic.assert_nontrivial(rec, "cli")
        want = ["REGION\tLENGTH\tPAIRS\tTRACTS\tPAIRS_SPANNING\tPAIR_SITES\tSHARE"]
        for (b, e), w in zip(rows, win):
            want.append(f"CHM13#0#chrT:{origin + b}-{origin + e}\t{e - b}\t{len(pairs)}\t{int(w['tracts'])}\t{int(w['pairs_spanning'])}\t"
                        f"{int(w['pair_sites'])}\t{float(w['share']):.8f}")
        want_seg = ["seq1\tseq2\tstart\tend\tsites\topen"]
        for s in seg:
            fl = int(s["flags"])
            want_seg.append(f"{names[s['h1']]}\t{names[s['h2']]}\t{origin + int(s['begin'])}\t{origin + int(s['end'])}\t{int(s['end'] - s['begin'])}\t"
                            + (("L" if fl & 1 else "") + ("R" if fl & 2 else "") or "."))
        want_pairs = ["SEQ1\tSEQ2\tN_DIFF\tLONGEST\tTRACTS\tTRACT_SITES"]
        for q in rec:
            want_pairs.append(f"{names[q['h1']]}\t{names[q['h2']]}\t{int(q['n_diff'])}\t{int(q['longest'])}\t{int(q['n_tracts'])}\t{int(q['tract_sites'])}")
        for extra in ([], ["--compact"]):
            r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", mpath, "--bed", bed, "--format", "ibs",
                                "--ibs-min-sites", "40", "--ibs-pairs", mode, "--ibs-segments", segp, "--ibs-pair-table", pairp] + extra,
                               capture_output=True, text=True, cwd=ROOT, timeout=300)
            assert r.returncode == 0, r.stderr[-3000:]
            assert r.stdout == "\n".join(want) + "\n"
            assert open(segp).read() == "\n".join(want_seg) + "\n"
            assert open(pairp).read() == "\n".join(want_pairs) + "\n"
            warn = [ln for ln in r.stderr.splitlines() if ln.startswith("Warning")]
            assert len(warn) == (1 if mode == "diploid" else 0)
