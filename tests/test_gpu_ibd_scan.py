"""GPU: impop_ibd_scan against the plain restatement of tests/plain_ibd.py — every integer and the double, bit for bit.  What needs
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
import ibd_cases as bc
import ibs_cases as ic
import plain_ibd as pd
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
    """one call with room for exactly the segments the restatement has"""
    args = dict(case.kwargs(), seg_capacity=len(case.want[1]))
    args.update(kw)
    return bm.ibd_scan(**args)[:3]


def same_bytes(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- the known answers of the header ------------------------------------------------------------------------------------------------

def test_known_answers(ctx):
    m01 = bc.known_matrix()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    for rule, gmap, want in bc.KNOWN:
        kw = dict(rule)
        if gmap is not None:
            kw["map_pos"], kw["map_g"] = gmap
        rec, seg, win, total = bm.ibd_scan(windows=[(0, 40), (10, 13)], **kw)
        assert [tuple(int(s[f]) for f in ("begin", "end", "len", "n_tracts", "ibs_sites", "flags")) for s in seg] == want, rule
        assert total == len(want) == int(rec["n_segments"][0])
        pd.assert_matches((rec, seg, win), pd.reference(m01, [(0, 1)], 0, 40, gmap=gmap, windows=[(0, 40), (10, 13)], **rule), rule)
    bm.free()


# ---- geometry: pair-tile edges, more than one batch of tracts per pair, chunks and sub-segments of 1, 2, 5 blocks, pair ranges ---------

@pytest.mark.parametrize("n", (2, 33, 65, 130))
def test_shapes_against_the_restatement(ctx, n, monkeypatch):
    bm = ctx.upload_dense(ic.geometry_matrix(n), keep_hap_major=False)
    for with_map in (False, True):
        case = bc.geometry_case(n, with_map)
        for chunk, seg in ((None, None), (1, 1), (5, 2)):
            set_blocks(monkeypatch, chunk, seg)
            pd.assert_matches(scan(bm, case), case.want, (case.tag, chunk, seg))
        set_blocks(monkeypatch, None, None)
        # a staging of a third of the candidates: several pair ranges
        pd.assert_matches(scan(bm, case, max_chunk_bytes=64 * (int(case.want[0]["n_candidates"].sum()) // 3 + 1)), case.want, (case.tag, "small"))
    # totals only: the same pair and window records, no list; no windows
    rec, seg, win, total = bm.ibd_scan(**dict(case.kwargs(), want_segments=False))
    assert seg is None and total == len(case.want[1])
    pd.assert_same(rec, case.want[0], "totals")
    pd.assert_same(win, case.want[2], "totals")
    got = bm.ibd_scan(**dict(case.kwargs(), windows=None))  # a counting call, then a filling call
    assert got[2] is None
    pd.assert_same(got[1], case.want[1], "no windows")
    bm.free()


# ---- the hand-made pair: chains across a 64-tract batch and across chunk edges -----------------------------------------------------

@pytest.mark.parametrize("max_gap, min_seed, min_output", ((1, 15, 15), (0, 15, 15), (0, 3, 3), (1, 16, 3)))
def test_hand_made_pair(ctx, max_gap, min_seed, min_output, monkeypatch):
    case = bc.hand_case(max_gap, min_seed, min_output)
    seg = case.want[1]
    if (max_gap, min_seed) == (1, 15):
        assert len(seg) == 1 and tuple(int(x) for x in seg[0])[2:] == (69, 700, 631, 553, 79, 0, 3)  # one chain; its seed sits in the last batch
    elif (max_gap, min_seed) == (0, 15):
        assert [(int(s["begin"]), int(s["end"])) for s in seg] == [bc.HAND_SEED]  # none joined: the seed alone
    elif (max_gap, min_seed) == (0, 3):
        assert len(seg) == 79 and (seg["n_tracts"] == 1).all()
    else:
        assert len(seg) == 0 and int(case.want[0]["n_candidates"][0]) == 79  # no seed anywhere
    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    for chunk, sg in ((2, 1), (1, 1), (3, 2), (None, None)):
        set_blocks(monkeypatch, chunk, sg)
        pd.assert_matches(scan(bm, case), case.want, (case.tag, chunk, sg))
    cm = bm.compact()
    pd.assert_matches(scan(cm, case), case.want, (case.tag, "compact"))
    cm.free()
    bm.free()


# ---- with no map, no joining and equal thresholds the segments are impop_ibs_scan's tracts ------------------------------------------

def test_degenerates_to_ibs_scan(ctx):
    L = 7
    ibs = ic.geometry_case(65, L)
    bm = ctx.upload_dense(ibs.m01, keep_hap_major=False)
    rec, seg, win, total = bm.ibd_scan(min_seed=L, min_extend=L, min_output=L, max_gap=0, min_sites=L, site_begin=ibs.b, site_end=ibs.e,
                                       windows=ibs.windows)
    t_rec, t_seg, t_win, t_total = bm.ibs_scan(min_sites=L, site_begin=ibs.b, site_end=ibs.e, windows=ibs.windows)
    assert total == t_total == len(ibs.want[1]) > 0
    for f in ("h1", "h2", "begin", "end", "flags", "pair"):
        assert np.array_equal(seg[f], t_seg[f]), f
    assert np.array_equal(seg["len"], t_seg["end"] - t_seg["begin"]) and (seg["n_tracts"] == 1).all()
    assert np.array_equal(rec["n_segments"], t_rec["n_tracts"]) and np.array_equal(rec["n_candidates"], t_rec["n_tracts"])
    assert np.array_equal(rec["total_len"], t_rec["tract_sites"]) and np.array_equal(rec["ibs_sites"], t_rec["tract_sites"])
    assert win.tobytes() == t_win.tobytes()
    bm.free()


# ---- uploads, weights, chunks and compaction never change a byte --------------------------------------------------------------------

def test_invariance(ctx, monkeypatch):
    set_blocks(monkeypatch, None, None)
    rng = np.random.default_rng(21300)
    n, S = 70, 2100
    m01 = dc.founder_matrix(rng, n, S, nf=4)
    mono = rng.random(S) < 0.4  # monomorphic sites, all 0 or all 1: a compacted matrix really is shorter
    m01[:, mono] = (rng.random(int(mono.sum())) < 0.3).astype(np.uint8)[None, :]
    case = bc.Case("inv", m01, pi.all_pairs(range(n)), (5, 2093), dict(min_sites=10, min_extend=4000, min_seed=30000, min_output=60000, max_gap=3),
                   bc.GEO_MAP, ic.window_list(5, 2093))
    base = None
    for ukw in ({"keep_hap_major": False}, {"keep_hap_major": True}, {"keep_hap_major": False, "dense_scan": True},
                {"keep_hap_major": False, "rare_split": False}):
        bm = ctx.upload_dense(m01, **ukw)
        got = scan(bm, case)
        if base is None:
            base = got
            pd.assert_matches(got, case.want, "inv")
            assert same_bytes(scan(bm, case, max_chunk_bytes=2 * 5 * n * 8), base)
            cm = bm.compact()
            assert cm.n_site < bm.n_site
            assert same_bytes(scan(cm, case), base) and same_bytes(scan(cm, case, max_chunk_bytes=4096), base)
            cm.free()
            bm.set_site_weights(np.ones(S, dtype=np.uint32))
            assert same_bytes(scan(bm, case), base)
        else:
            assert same_bytes(got, base), ukw
        bm.free()


def test_list_form(ctx):
    case = bc.geometry_case(65, True)
    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    kw = case.kwargs()
    pairs = [(3, 64), (64, 3), (3, 64), (0, 64), (5, 6), (6, 5), (3, 4), (3, 40), (33, 3), (0, 1)]
    want = pd.reference(case.m01, pairs, case.b, case.e, gmap=case.gmap, windows=case.windows, **case.rule)
    rec, seg, win, _ = bm.ibd_scan(pairs=pairs, **kw)
    pd.assert_matches((rec, seg, win), want, "list")
    for f in ("n_segments", "n_candidates", "total_len", "total_extent", "longest_len", "ibs_sites"):  # (h2, h1): only the two fields change
        assert rec[f][0] == rec[f][1] == rec[f][2] and rec[f][4] == rec[f][5]
    a, c = seg[seg["pair"] == 4], seg[seg["pair"] == 5]
    assert len(a) and a["begin"].tolist() == c["begin"].tolist() and a["h1"].tolist() == c["h2"].tolist() and a["len"].tolist() == c["len"].tolist()
    rng = np.random.default_rng(21500)
    members = sorted(int(x) for x in rng.permutation(65)[:23])
    mask = np.zeros(65, np.uint8)
    mask[members] = 1
    by_mask = bm.ibd_scan(mask_p=mask, **kw)[:3]
    by_list = bm.ibd_scan(pairs=pi.all_pairs(members), **kw)[:3]
    assert same_bytes(by_mask, by_list)
    pd.assert_matches(by_mask, pd.reference(case.m01, pi.all_pairs(members), case.b, case.e, gmap=case.gmap, windows=case.windows, **case.rule), "mask")
    bm.free()


# ---- the capacity protocol -----------------------------------------------------------------------------------------------------------

def test_capacity(ctx):
    import impop_amd
    from impop_amd import _lib
    case = bc.geometry_case(33, False)
    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    total = len(case.want[1])
    w = impop_amd.make_windows(case.windows)
    r = case.rule
    prm = _lib.IbdParams(C.sizeof(_lib.IbdParams), r["min_sites"], case.b, case.e, r["min_seed"], r["min_extend"], r["min_output"], r["max_gap"],
                         None, None, 0, 0, 0)
    for cap in (total - 1, 0, total, total + 5):
        rec = np.zeros(len(case.pairs), dtype=impop_amd.IBD_PAIR_DTYPE)
        win = np.zeros(len(w), dtype=impop_amd.IBS_WINDOW_DTYPE)
        seg = np.full(total + 5, 0xA5, dtype=np.uint8).repeat(48).view(impop_amd.IBD_SEGMENT_DTYPE)
        canary = seg.tobytes()
        n_seg = C.c_uint64(0)
        rc = ctx._lib.impop_ibd_scan(ctx.handle, bm.handle, None, None, 0, w.ctypes.data_as(C.POINTER(_lib.Window)), len(w), C.byref(prm),
                                     rec.ctypes.data_as(C.POINTER(_lib.IbdPair)), seg.ctypes.data_as(C.POINTER(_lib.IbdSegment)), cap,
                                     C.byref(n_seg), win.ctypes.data_as(C.POINTER(_lib.IbsWindow)))
        assert rc == 0 and n_seg.value == total
        pd.assert_same(rec, case.want[0], cap)
        pd.assert_same(win, case.want[2], cap)
        if cap < total:
            assert seg.tobytes() == canary  # untouched
        else:
            pd.assert_same(seg[:total], case.want[1], cap)
            assert seg[total:].tobytes() == canary[total * 48:]
    kw = dict(case.kwargs(), windows=None)
    assert bm.ibd_scan(seg_capacity=total - 1, **kw)[1] is None
    pd.assert_same(bm.ibd_scan(seg_capacity=total, **kw)[1], case.want[1], "capacity")
    bm.free()


# ---- the upper end of the range, and the timers ------------------------------------------------------------------------------------------

def test_4096_haplotypes_all_pairs(ctx):
    rng = np.random.default_rng(21600)
    n, S = 4096, 256
    m01 = dc.founder_matrix(rng, n, S, nf=6, p_switch=0.01, p_flip=0.004)
    rule = dict(min_sites=8, min_extend=8, min_seed=40, min_output=70, max_gap=1)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    ctx.gram_timing(True)
    rec, seg, _, total = bm.ibd_scan(**rule)
    ms, chunks = ctx.ibd_elapsed()
    ctx.gram_timing(False)
    assert len(ms) == 4 and all(t > 0.0 for t in ms) and chunks >= 2  # transposes, walks, combine / close, chain
    n_pairs = n * (n - 1) // 2
    iu, ju = np.triu_indices(n, 1)  # i-major
    assert len(rec) == n_pairs and np.array_equal(rec["h1"], iu.astype(np.uint32)) and np.array_equal(rec["h2"], ju.astype(np.uint32))
    assert total == len(seg) == int(rec["n_segments"].sum(dtype=np.int64)) > 0
    assert np.array_equal(seg["pair"], np.repeat(np.arange(n_pairs, dtype=np.uint32), rec["n_segments"]))  # pair-major
    off = np.concatenate([[0], np.cumsum(rec["n_segments"], dtype=np.int64)])
    pick = np.sort(rng.choice(n_pairs, size=2000, replace=False))
    want = pd.reference(m01, [(int(iu[p]), int(ju[p])) for p in pick], 0, S, **rule)
    pd.assert_same(rec[pick].copy(), want[0], "n4096 pairs")
    w_seg = want[1].copy()
    w_seg["pair"] = pick[w_seg["pair"]]
    pd.assert_same(np.concatenate([seg[off[p]:off[p + 1]] for p in pick]), w_seg, "n4096 segments")
    assert (want[0]["n_segments"] > 0).any() and (want[0]["n_segments"] == 0).any() and (want[1]["n_tracts"] > 1).any()
    bm.free()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------

def test_refusals(ctx):
    import impop_amd
    from impop_amd import ImpopError, _lib
    case = bc.geometry_case(33, True)
    n, S = case.m01.shape
    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    one = np.zeros(n, np.uint8)
    one[4] = 1
    ok = dict(min_seed=20, min_extend=5, min_output=30, max_gap=2)
    bad = [dict(ok, min_sites=0), dict(ok, site_begin=100, site_end=100), dict(ok, site_begin=200, site_end=100), dict(ok, site_end=S + 1),
           dict(ok, site_begin=S), dict(ok, pairs=[(4, 4)]), dict(ok, pairs=[(0, n)]), dict(ok, pairs=[(0, 1)], mask_p=np.ones(n, np.uint8)),
           dict(ok, mask_p=one), dict(ok, mask_p=np.zeros(n, np.uint8)), dict(ok, site_begin=10, site_end=500, windows=[(9, 100)]),
           dict(ok, site_begin=10, site_end=500, windows=[(400, 501)]), dict(ok, site_begin=10, site_end=500, windows=[(300, 200)]),
           dict(ok, min_seed=4),                                              # min_seed < min_extend
           dict(ok, map_pos=[5], map_g=[7]),                                  # one breakpoint
           dict(ok, map_pos=[5, 5, 9], map_g=[1, 2, 3]),                      # pos repeats
           dict(ok, map_pos=[5, 4], map_g=[1, 2]),                            # pos descends
           dict(ok, map_pos=[5, 9], map_g=[2, 1]),                            # g decreases
           dict(ok, map_pos=[5, 5 + (1 << 32)], map_g=[1, 2]),                # a pos step of 2^32
           dict(ok, map_pos=[5, 9], map_g=[1, 1 + (1 << 32)])]                # a g step of 2^32
    for kw in bad:
        with pytest.raises(ImpopError) as ei:
            bm.ibd_scan(**kw)
        assert ei.value.code == E_INVALID, kw
    with pytest.raises(ImpopError) as ei:
        bm.ibd_scan(pairs=np.tile(np.array([[0, 1]], dtype=np.uint32), (_lib.IBS_MAX_PAIRS + 1, 1)), **ok)
    assert ei.value.code == E_UNSUPPORTED
    with pytest.raises(ImpopError) as ei:
        bm.ibd_scan(map_pos=np.arange(_lib.IBD_MAX_MAP + 1, dtype=np.uint64), map_g=np.zeros(_lib.IBD_MAX_MAP + 1, dtype=np.uint64), **ok)
    assert ei.value.code == E_UNSUPPORTED
    # the largest steps a map may have are taken
    bm.ibd_scan(map_pos=[5, 4 + (1 << 32)], map_g=[1, (1 << 32)], **ok)
    # raw calls: a wrong struct_size; windows without win_out and the reverse; one map pointer alone
    w = impop_amd.make_windows([(10, 100)])
    rec = np.zeros(n * (n - 1) // 2, dtype=impop_amd.IBD_PAIR_DTYPE)
    win = np.zeros(1, dtype=impop_amd.IBS_WINDOW_DTYPE)
    n_seg = C.c_uint64(0)
    mpos = np.array([0, 100], dtype=np.uint64)
    up = mpos.ctypes.data_as(C.POINTER(C.c_uint64))

    def raw(prm, windows, win_out):
        return ctx._lib.impop_ibd_scan(ctx.handle, bm.handle, None, None, 0, windows, 1 if windows is not None else 0, C.byref(prm),
                                       rec.ctypes.data_as(C.POINTER(_lib.IbdPair)), None, 0, C.byref(n_seg), win_out)

    def params(size=C.sizeof(_lib.IbdParams), pos=None, g=None, n_map=0):
        return _lib.IbdParams(size, 5, 0, 0, 20, 5, 30, 2, pos, g, n_map, 0, 0)

    wp, wo = w.ctypes.data_as(C.POINTER(_lib.Window)), win.ctypes.data_as(C.POINTER(_lib.IbsWindow))
    assert raw(params(size=C.sizeof(_lib.IbdParams) - 8), wp, wo) == E_INVALID
    assert raw(params(), wp, None) == E_INVALID and raw(params(), None, wo) == E_INVALID
    assert raw(params(pos=up, n_map=2), wp, wo) == E_INVALID and raw(params(pos=up, g=up, n_map=0), wp, wo) == E_INVALID
    assert raw(params(), wp, wo) == 0 and raw(params(pos=up, g=up, n_map=2), wp, wo) == 0
    # afterwards the context is still usable
    pd.assert_matches(scan(bm, case), case.want, "after the refusals")
    bm.free()
    big = ctx.upload_dense(np.zeros((_lib.IBS_MAX_N + 1, 64), np.uint8), keep_hap_major=False)
    with pytest.raises(ImpopError) as ei:
        big.ibd_scan(**ok)
    assert ei.value.code == E_UNSUPPORTED
    big.free()


# ---- the trace line, in a child process under IMPOP_TRACE=1 ------------------------------------------------------------------------------

def _child(out_path):
    import impop_amd
    from impop_amd import ImpopError
    ctx = impop_amd.Context(0)
    out = {}
    case = bc.geometry_case(65, True)
    kw = dict(case.kwargs(), windows=None)

    def call(tag, fn):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        r = fn()
        out[tag + "_rec"], out[tag + "_seg"] = r[0], r[1] if r[1] is not None else np.zeros(0)
        sys.stderr.flush()

    bm = ctx.upload_dense(case.m01, keep_hap_major=False)
    call("totals", lambda: bm.ibd_scan(want_segments=False, **kw))
    call("fill", lambda: bm.ibd_scan(seg_capacity=len(case.want[1]), **kw))
    call("chunked", lambda: bm.ibd_scan(seg_capacity=len(case.want[1]), max_chunk_bytes=2 * 4 * 65 * 8, **kw))
    call("nomap", lambda: bm.ibd_scan(pairs=[(0, 1), (2, 64)], want_segments=False, site_begin=case.b, site_end=case.e, **bc.GEO_RULE))
    cm = bm.compact()
    call("compact", lambda: cm.ibd_scan(want_segments=False, **kw))
    cm.free()
    sys.stderr.write("@@call refused\n")
    sys.stderr.flush()
    try:
        bm.ibd_scan(min_seed=1, min_extend=2, min_output=3)
        out["refused"] = np.array([0])
    except ImpopError as exc:
        out["refused"] = np.array([exc.code])
    bm.free()
    ctx.close()
    np.savez(out_path, **out)


_TRACE = re.compile(r"\[impop_ibd_scan\] (.*)$")


def test_trace_line():
    case = bc.geometry_case(65, True)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
        for name in ENVS:
            env.pop(name, None)
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_ibd_scan as t; t._child(sys.argv[1])", path],
                           capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        z = np.load(path)
        recs = {k: z[k] for k in z.files}
    assert "[impop_ibs_scan]" not in r.stderr  # the sweeps it borrows print nothing of their own
    trace, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@@call "):
            cur = line.split()[1]
            trace[cur] = []
        mt = _TRACE.search(line)
        if mt and cur:
            kv = dict(x.split("=") for x in mt.group(1).split())
            trace[cur].append({k: (v if k == "route" else int(v)) for k, v in kv.items()})
    n_pairs, total, cands = 65 * 64 // 2, len(case.want[1]), int(case.want[0]["n_candidates"].sum())
    for tag in ("totals", "fill", "chunked", "compact"):
        assert recs[tag + "_rec"].tobytes() == case.want[0].tobytes(), tag
    assert recs["fill_seg"].tobytes() == case.want[1].tobytes() == recs["chunked_seg"].tobytes()
    assert [len(trace[t]) for t in ("totals", "fill", "chunked", "nomap", "compact", "refused")] == [1, 1, 1, 1, 1, 0]
    assert recs["refused"].tolist() == [E_INVALID]
    t = trace["totals"][0]
    assert list(t) == ["route", "pairs", "pair_ranges", "candidates", "segments", "map_points", "launches", "bytes_streamed"]
    assert t["route"] == "dense" and t["pairs"] == n_pairs and t["segments"] == total and t["candidates"] == cands and t["pair_ranges"] == 1
    assert t["map_points"] == 8  # of the 10 breakpoints, those from the last at or left of 5 to the first at or right of 2093
    assert t["launches"] == 4 + 5 + 1  # count sweep; fill sweep; the chain kernel's count form
    f = trace["fill"][0]
    assert f["launches"] == t["launches"] + 1 and f["bytes_streamed"] > t["bytes_streamed"]  # and its fill form
    c = trace["chunked"][0]
    assert c["pair_ranges"] > 1 and c["segments"] == total and c["candidates"] == cands
    assert trace["nomap"][0]["pairs"] == 2 and trace["nomap"][0]["map_points"] == 0
    assert trace["compact"][0]["route"] == "compact" and trace["compact"][0]["bytes_streamed"] <= t["bytes_streamed"]


# ---- the command line ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ("all", "diploid"))
@pytest.mark.parametrize("with_map", (False, True))
def test_cli_tables_are_the_records(tmp_path, mode, with_map):
    from decimal import Decimal
    from impop_amd.matrixio import MatrixFile, save_matrix
    from impop_amd import ibd, pack_hap_major
    rng = np.random.default_rng(21700)
    n, W, origin = 24, 900, 5000
    m01 = dc.founder_matrix(rng, n, W)
    names = [f"S{i // 2:02d}#{i % 2 + 1}#chrT:0-1" for i in range(n - 1)] + ["CHM13#0#chrT:0-1"]  # S11 has one copy only
    mpath, bed, segp, pairp, mapp = (str(tmp_path / x) for x in ("m.npz", "w.bed", "seg.tsv", "pairs.tsv", "g.map"))
    save_matrix(mpath, MatrixFile(bits=pack_hap_major(m01), n_site=W, names=names, origin=origin, contig="chrT"))
    rows = [(0, 130), (100, 300), (250, 251), (300, 900), (0, 900)]
    open(bed, "w").write("".join(f"chrT\t{origin + b}\t{origin + e}\n" for b, e in rows))
    open(mapp, "w").write("chrT a 0.10 4900\nchrT b 0.3000004 5100\nchrU z 7 5150\nchrT c 0.3000004 5400\nchrT d 0.95 5890\nchrT e 1.0 7000\n")
    gmap = ibd.read_plink_map(mapp, "chrT", origin)
    assert gmap == ([0, 100, 400, 890, 2000], [200000, 300000, 300000, 950000, 1000000])
    site_rule = dict(min_sites=10, min_extend=10, min_seed=40, min_output=60, max_gap=3)
    cm_rule = dict(min_sites=10, min_extend=10000, min_seed=40000, min_output=80000, max_gap=3)
    site_opts = ["--ibd-min-seed", "40", "--ibd-min-extend", "10", "--ibd-min-output", "60"]
    cm_opts = ["--ibd-map", mapp, "--ibd-min-seed", "0.04", "--ibd-min-extend", "0.01", "--ibd-min-output", "0.08"]
    pairs = pi.all_pairs(range(n)) if mode == "all" else [(2 * i, 2 * i + 1) for i in range(11)]
    rule, gm, opts = (cm_rule, gmap, cm_opts) if with_map else (site_rule, None, site_opts)
    rec, seg, win = pd.reference(m01, pairs, 0, W, gmap=gm, windows=rows, **rule)
    assert len(seg) > 0 and (mode == "diploid" or (seg["n_tracts"] > 1).any())
    want = ["REGION\tLENGTH\tPAIRS\tSEGMENTS\tPAIRS_SPANNING\tPAIR_SITES\tSHARE"]
    for (b, e), w in zip(rows, win):
        want.append(f"CHM13#0#chrT:{origin + b}-{origin + e}\t{e - b}\t{len(pairs)}\t{int(w['tracts'])}\t{int(w['pairs_spanning'])}\t"
                    f"{int(w['pair_sites'])}\t{float(w['share']):.8f}")
    want_seg = ["seq1\tseq2\tstart\tend\tlen\ttracts\tibs_sites\topen" + ("\tcM" if gm else "")]
    for s in seg:
        fl = int(s["flags"])
        want_seg.append(f"{names[s['h1']]}\t{names[s['h2']]}\t{origin + int(s['begin'])}\t{origin + int(s['end'])}\t{int(s['len'])}\t"
                        f"{int(s['n_tracts'])}\t{int(s['ibs_sites'])}\t" + (("L" if fl & 1 else "") + ("R" if fl & 2 else "") or ".")
                        + (f"\t{Decimal(int(s['len'])) / 1000000:.6f}" if gm else ""))
    want_pairs = ["SEQ1\tSEQ2\tSEGMENTS\tCANDIDATES\tTOTAL_LEN\tTOTAL_EXTENT\tLONGEST_LEN\tIBS_SITES"]
    for q in rec:
        want_pairs.append("\t".join([names[q["h1"]], names[q["h2"]]] + [str(int(q[f])) for f in (
            "n_segments", "n_candidates", "total_len", "total_extent", "longest_len", "ibs_sites")]))
    for extra in ([], ["--compact"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_ibd.py"), "--matrix", mpath, "--bed", bed,
                            "--ibd-min-sites", "10", "--ibd-max-gap", "3", "--ibd-pairs", mode, "--ibd-segments", segp,
                            "--ibd-pair-table", pairp] + opts + extra, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout == "\n".join(want) + "\n"
        assert open(segp).read() == "\n".join(want_seg) + "\n"
        assert open(pairp).read() == "\n".join(want_pairs) + "\n"
