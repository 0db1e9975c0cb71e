"""GPU: impop_pairdist_scan — pairwise-distance distributions per window from the Gram pass — against the plain restatement
(tests/plain_pairdist.py: every integer, snn and gmin as bytes, both histogram tables), against the streaming scans of the same
windows, and against itself under every way of computing the same windows."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import pairdist_cases as pc
import plain_pairdist as pp
from conftest import ROOT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_N = 4096  # IMPOP_PAIRDIST_MAX_N


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def case(n):
    m01 = pc.matrix(n)
    return m01, pc.segment_distances(m01)


@functools.lru_cache(maxsize=None)
def reference(n, shape, K, hist):
    """the plain reference of a parity case, computed once: (per-window dicts, packed arrays)"""
    _, seg_H = case(n)
    wins = pc.window_lists()[shape]
    bins, width = (pc.BINS, pc.WIDTH) if hist else (0, 1)
    per = [pp.window(pc.window_distance(seg_H, w), w[1] - w[0], pc.panels(n, K), bins, width) for w in wins]
    return per, pp.pack(per, K, bins)


@pytest.fixture(scope="module")
def uploaded(ctx):
    """the case matrices on the device, one upload per n"""
    import impop_amd
    held = {}

    def get(n):
        if n not in held:
            m01 = case(n)[0]
            held[n] = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
        return held[n]
    yield get
    for bm in held.values():
        bm.free()


def blob(res):
    return b"".join(a.tobytes() for a in res if a is not None)


def assert_equal(got, want, what=""):
    """field by field for a readable failure, then byte for byte (snn and gmin included: NaN has one bit pattern)"""
    for g, w, kind in ((got[0], want[0], "panel"), (got[1], want[1], "pair")):
        assert g.shape == w.shape, (what, kind, g.shape, w.shape)
        for f in w.dtype.names:
            if w.dtype[f].kind != "f":
                bad = np.argwhere(g[f] != w[f])
                assert not len(bad), (what, kind, f, bad[:4].tolist(), g[f][tuple(bad[0])], w[f][tuple(bad[0])])
        assert g.tobytes() == w.tobytes(), (what, kind, "bytes of snn / gmin")
    for g, w, kind in ((got[2], want[2], "hist_within"), (got[3], want[3], "hist_between")):
        assert (g is None) == (w is None), (what, kind)
        if w is not None:
            assert g.shape == w.shape and g.dtype == np.uint32 and (g == w).all(), (what, kind, np.argwhere(g != w)[:4].tolist())


PARITY = [(n, shape, K, hist) for n in (31, 65, 465, 513, 1030) for shape in ("tiling", "sliding") for K in (1, 2, 3, 8)
          for hist in (False, True) if K < 8 or n >= 65]


@pytest.mark.parametrize("n,shape,K,hist", PARITY)
def test_exact_parity(uploaded, n, shape, K, hist):
    """Every integer of every record and both tables equal the restatement's; snn and gmin are compared as bytes.  The planted
    features are asserted on the reference first."""
    per, want = reference(n, shape, K, hist)
    feats = pc.planted_features(per, K)
    if not hist:
        feats.pop("overflow_bin")
    assert all(feats.values()), feats
    ties = pc.tie_counts(pc.window_distance(case(n)[1], pc.window_lists()[shape][0]), pc.panels(n, K))
    assert any(lo >= 2 for lo, _ in ties) and any(hi >= 2 for _, hi in ties)
    got = uploaded(n).pairdist_scan(pc.window_lists()[shape], pc.panels_flags(n, K), hist_bins=pc.BINS if hist else 0,
                                    hist_width=pc.WIDTH if hist else 1)
    assert_equal(got, want, (n, shape, K, hist))


def test_upper_end_of_the_member_range(ctx):
    """4096 members, the documented limit: K = 2, one 256-site window"""
    import impop_amd
    rng = np.random.default_rng(4096)
    n, S = MAX_N, 256
    m01 = rng.integers(0, 2, size=(n, S), dtype=np.uint8)
    m01[1000] = m01[3]       # a zero distance between the panels
    m01[2000] = 1 - m01[4]   # the full distance inside one (both in the even panel)
    X = m01.astype(np.float32)
    I = (X @ X.T).astype(np.int64)  # counts <= 256: exact in float32
    assert (np.diag(I) == m01.sum(axis=1)).all()
    pops = [list(range(0, n, 2)), list(range(1, n, 2))]
    want = pp.pack([pp.window(pp.hamming(I), S, pops)], 2, 0)
    assert int(want[0][0, 0]["max_h"]) == S and int(want[1][0, 0]["n_zero"]) >= 1
    bm = ctx.upload(impop_amd.pack_hap_major(m01), S, keep_hap_major=True)
    try:
        flags = [np.isin(np.arange(n), p).astype(np.uint8) for p in pops]
        assert_equal(bm.pairdist_scan([(0, S, S)], flags), want, "n = 4096")
    finally:
        bm.free()


@pytest.mark.parametrize("n", [65, 465])
@pytest.mark.parametrize("shape", ["tiling", "sliding"])
def test_cross_checks_against_the_streaming_scans(uploaded, n, shape):
    """sum_h of a panel is scan(mask_p = panel).sum_p, sum_h of a pair is scan(mask_a, mask_b).sum_ab, and a panel's n_zero is
    (sum_sq - n_members) / 2 of haplotype_scan(mask_p = panel): three kernels that share nothing with the Gram pass"""
    K = 3
    wins = pc.window_lists()[shape]
    flags = pc.panels_flags(n, K)
    bm = uploaded(n)
    panels, pairs, _, _ = bm.pairdist_scan(wins, flags)
    for k in range(K):
        assert (bm.scan(wins, mask_p=flags[k])["sum_p"] == panels[:, k]["sum_h"]).all()
        hs = bm.haplotype_scan(wins, mask_p=flags[k])
        assert ((hs["sum_sq"].astype(np.int64) - hs["n_members"]) // 2 == panels[:, k]["n_zero"].astype(np.int64)).all()
    p = 0
    for a in range(K):
        for b in range(a + 1, K):
            assert (bm.scan(wins, mask_a=flags[a], mask_b=flags[b])["sum_ab"] == pairs[:, p]["sum_h"]).all()
            p += 1


# ---- the same windows computed in every other way: byte-identical records and tables -----------------------------------------------

def _child(path, n, shape, K):
    import impop_amd
    ctx = impop_amd.Context(0)
    m01 = pc.matrix(n)
    bm = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
    got = bm.pairdist_scan(pc.window_lists()[shape], pc.panels_flags(n, K), hist_bins=pc.BINS, hist_width=pc.WIDTH)
    np.savez(path, panels=got[0], pairs=got[1], hw=got[2], hb=got[3])
    bm.free(); ctx.close()


def run_child(n, shape, K, env_extra):
    """-> (result, trace fields of the [impop_pairdist_scan] line)"""
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]), **env_extra)
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_pairdist_scan as t; t._child(sys.argv[1], %d, %r, %d)" % (n, shape, K), path],
                           capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = [l for l in r.stderr.splitlines() if l.startswith("[impop_pairdist_scan] pops=")]
        assert len(lines) == 1, r.stderr[-2000:]
        trace = dict(f.split("=") for f in lines[0].split()[1:])
        with np.load(path) as z:
            return (z["panels"].copy(), z["pairs"].copy(), z["hw"].copy(), z["hb"].copy()), trace


@pytest.mark.parametrize("n,K", [(465, 3), (513, 2)])
@pytest.mark.parametrize("shape", ["tiling", "sliding"])
def test_invariance_under_gram_chunk_and_histogram_switches(uploaded, n, K, shape):
    """int32 Gram counts, Gram chains of 1 and of 8 links, three windows per chunk (the chunk count read from the trace line),
    histograms tallied in global memory instead of LDS: the bytes of the default run (each switch is read by a fresh process)"""
    wins = pc.window_lists()[shape]
    base = uploaded(n).pairdist_scan(wins, pc.panels_flags(n, K), hist_bins=pc.BINS, hist_width=pc.WIDTH)
    assert_equal(base, reference(n, shape, K, True)[1])
    same, trace = run_child(n, shape, K, {})
    assert blob(same) == blob(base)
    assert trace["hist"] == "lds" and int(trace["chunks"]) == 1 and int(trace["windows"]) == len(wins)
    assert (int(trace["pops"]), int(trace["pairs"]), int(trace["hist_bins"])) == (K, K * (K - 1) // 2, pc.BINS)
    assert int(trace["members"]) == sum(len(p) for p in pc.panels(n, K))
    for env in ({"IMPOP_GRAM_U16": "0"}, {"IMPOP_GRAM_CHAIN": "1"}, {"IMPOP_GRAM_CHAIN": "8"}, {"IMPOP_PAIRWISE_CHUNK": "3"},
                {"IMPOP_PAIRDIST_LDS_BINS": "0"}):
        got, trace = run_child(n, shape, K, env)
        assert blob(got) == blob(base), env
        if "IMPOP_PAIRWISE_CHUNK" in env:
            assert int(trace["chunks"]) >= (len(wins) + 2) // 3 and int(trace["launches"]) == int(trace["chunks"])
        if "IMPOP_PAIRDIST_LDS_BINS" in env:
            assert trace["hist"] == "global"


def test_all_histogram_counters_too_many_for_lds(uploaded):
    """K = 8 with 1024 bins is 36 x 1024 counters: the global route without a switch; any K <= 8 and B <= 1024 works"""
    n, K = 65, 8
    wins = pc.window_lists()["tiling"][:3]
    _, seg_H = case(n)
    want = pp.pack([pp.window(pc.window_distance(seg_H, w), w[1] - w[0], pc.panels(n, K), 1024, 1) for w in wins], K, 1024)
    assert_equal(uploaded(n).pairdist_scan(wins, pc.panels_flags(n, K), hist_bins=1024, hist_width=1), want)


def test_invariance_compacted_alone_in_a_list_and_twice(ctx):
    """The matrix compacted to its variable sites (planted all-ones and all-zeros columns), a window alone against the same window
    in a list, and two calls on one input"""
    import impop_amd
    n, K = 465, 3
    m01 = pc.matrix(n).copy()
    m01[:, 5::17] = 1
    m01[:, 9::23] = 0
    flags = pc.panels_flags(n, K)
    full = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
    try:
        comp = full.compact()
        try:
            for shape, wins in pc.window_lists().items():
                a = full.pairdist_scan(wins, flags, hist_bins=pc.BINS, hist_width=pc.WIDTH)
                assert_equal(a, pp.scan(m01, wins, pc.panels(n, K), pc.BINS, pc.WIDTH), shape)
                assert blob(full.pairdist_scan(wins, flags, hist_bins=pc.BINS, hist_width=pc.WIDTH)) == blob(a)
                assert blob(comp.pairdist_scan(wins, flags, hist_bins=pc.BINS, hist_width=pc.WIDTH)) == blob(a), shape
                for k in (0, len(wins) // 2, len(wins) - 1):
                    one = full.pairdist_scan([wins[k]], flags, hist_bins=pc.BINS, hist_width=pc.WIDTH)
                    assert blob(one) == blob([x[k:k + 1] for x in a]), (shape, k)
        finally:
            comp.free()
    finally:
        full.free()


@pytest.mark.parametrize("heavy", [False, True])
def test_invariance_weighted_against_bp_expanded(ctx, heavy):
    """A node-level matrix with site weights gives what its bp-expanded matrix gives (every column repeated weight times).  With
    one weight >= 65536 the windows that hold it pass 2^16 sites: int32 counts."""
    import impop_amd
    from af_cases import planted_matrix
    rng = np.random.default_rng(99)
    n, cols, K = 120, 400, 3
    node = planted_matrix(n, 4, 4242)[:, :cols].copy()
    wt = rng.integers(1, 6, size=cols).astype(np.uint32)
    if heavy:
        wt[37] = 70000
        node[::2, 37] ^= 1
    expanded = np.repeat(node, wt, axis=1)
    edges = np.concatenate([[0], np.cumsum(wt.astype(np.int64))])
    node_wins = [(s, min(s + 50, cols), 0) for s in range(0, cols, 50)] + [(s, min(s + 100, cols), 0) for s in range(0, cols - 50, 50)]
    bp_wins = [(int(edges[a]), int(edges[b]), 0) for a, b, _ in node_wins]
    flags = pc.panels_flags(n, K, planted=False)
    bw = ctx.upload(impop_amd.pack_hap_major(node), cols, keep_hap_major=True)
    be = ctx.upload(impop_amd.pack_hap_major(expanded), expanded.shape[1], keep_hap_major=True)
    try:
        bw.set_site_weights(wt)
        width = 2000 if heavy else 3
        a = bw.pairdist_scan(node_wins, flags, hist_bins=pc.BINS, hist_width=width)
        assert blob(be.pairdist_scan(bp_wins, flags, hist_bins=pc.BINS, hist_width=width)) == blob(a)
        assert_equal(a, pp.scan(node, node_wins, pc.panels(n, K, planted=False), pc.BINS, width, weights=wt))
        if heavy:
            assert int(a[0]["n_sites"].max()) >= 65536 and int(a[0]["max_h"].max()) >= 70000
        comp = bw.compact()
        try:
            assert blob(comp.pairdist_scan(node_wins, flags, hist_bins=pc.BINS, hist_width=width)) == blob(a)
        finally:
            comp.free()
    finally:
        bw.free(); be.free()


# ---- limits and degenerate shapes ---------------------------------------------------------------------------------------------------

def raw_call(ctx, bm, wins, flags, bins=0, width=1, n_pop=None):
    """the C call with nothing checked on the Python side -> (return code, message)"""
    import ctypes as C
    import impop_amd
    from impop_amd import _lib
    w = impop_amd.make_windows(wins)
    K = len(flags) if n_pop is None else n_pop
    packed = np.concatenate([impop_amd.pack_mask(f, bm.n_hap) for f in flags]) if flags else np.zeros(1, np.uint64)
    pan = np.zeros((len(w), max(K, 1)), impop_amd.DIST_PANEL_DTYPE)
    pair = np.zeros((len(w), max(K * (K - 1) // 2, 1)), impop_amd.DIST_PAIR_DTYPE)
    hw = np.zeros((len(w), max(K, 1), max(bins, 1)), np.uint32)
    prm = _lib.PairdistParams(C.sizeof(_lib.PairdistParams), bins, width, 0)
    rc = ctx._lib.impop_pairdist_scan(ctx.handle, bm.handle, w.ctypes.data_as(C.POINTER(_lib.Window)), len(w),
                                      packed.ctypes.data_as(C.POINTER(C.c_uint64)), K, C.byref(prm),
                                      pan.ctypes.data_as(C.POINTER(_lib.DistPanel)), pair.ctypes.data_as(C.POINTER(_lib.DistPair)),
                                      hw.ctypes.data_as(C.POINTER(C.c_uint32)), None)
    return rc, ctx._lib.impop_last_error().decode()


def test_member_limit(ctx):
    """a union of 4097 members is refused with the limit in the message, before anything runs; 4096 is accepted"""
    from impop_amd import _lib
    n, S = MAX_N + 4, 64
    bm = ctx.synthetic(n, S, keep_hap_major=True)
    try:
        a = np.zeros(n, np.uint8); a[:2049] = 1
        b = np.zeros(n, np.uint8); b[2049:4097] = 1
        rc, msg = raw_call(ctx, bm, [(0, S, S)], [a, b])
        assert rc == _lib.E_UNSUPPORTED and "4097" in msg and "4096" in msg
        b[4096] = 0
        rc, msg = raw_call(ctx, bm, [(0, S, S)], [a, b])
        assert rc == 0, msg
    finally:
        bm.free()


def test_refusals_and_degenerate_shapes(ctx, uploaded):
    from impop_amd import _lib
    n, K = 65, 3
    bm = uploaded(n)
    wins = pc.window_lists()["tiling"]
    flags = pc.panels_flags(n, K)
    overlap = [flags[0], flags[1] | flags[0]]
    for what, args, needle in (("overlapping panels", dict(flags=overlap), "disjoint"),
                               ("an empty panel", dict(flags=[flags[0], np.zeros(n, np.uint8)]), "empty"),
                               ("n_pop 0", dict(flags=[], n_pop=0), "n_pop"),
                               ("n_pop 9", dict(flags=[np.eye(n, dtype=np.uint8)[i] for i in range(9)]), "n_pop"),
                               ("hist_bins 1025", dict(flags=flags, bins=1025), "hist_bins"),
                               ("hist_width 0", dict(flags=flags, bins=4, width=0), "hist_width")):
        rc, msg = raw_call(ctx, bm, wins, **args)
        assert rc == _lib.E_INVALID and needle in msg, (what, rc, msg)
    # a one-member panel: no pairs, sentinel indexes; its member still has neighbours in the other panel
    solo = [np.eye(n, dtype=np.uint8)[7], flags[1]]
    got = bm.pairdist_scan(wins, solo)
    assert_equal(got, pp.pack([pp.window(pc.window_distance(case(n)[1], w), w[1] - w[0], [[7], pc.panels(n, K)[1]]) for w in wins], 2, 0))
    r = got[0][0, 0]
    assert int(r["n_pairs"]) == 0 and (int(r["min_h"]), int(r["max_h"])) == (0, 0)
    assert [int(r[f]) for f in ("min_i", "min_j", "max_i", "max_j")] == [pp.NONE] * 4
    # an empty window between real ones, and an empty list
    some = [wins[0], (300, 300, 0), wins[2]]
    got = bm.pairdist_scan(some, flags, hist_bins=pc.BINS, hist_width=pc.WIDTH)
    assert_equal(got, pp.scan(case(n)[0], some, pc.panels(n, K), pc.BINS, pc.WIDTH), "empty window")
    assert int(got[0][1, 0]["n_sites"]) == 0 and int(got[1][1, 0]["n_zero"]) == int(got[1][1, 0]["n_pairs"]) and np.isnan(got[1][1, 0]["gmin"])
    none = bm.pairdist_scan([], flags, hist_bins=4)
    assert none[0].shape == (0, K) and none[1].shape == (0, 3) and none[2].shape == (0, K, 4)
    # the device error word: the call that sees it fails once and clears it
    good = bm.pairdist_scan(wins, flags)
    _lib.check(ctx._lib.impop_debug_raise_device_error(ctx.handle, 1))
    rc, msg = raw_call(ctx, bm, wins, flags)
    assert rc == _lib.E_INTERNAL, msg
    assert blob(bm.pairdist_scan(wins, flags)) == blob(good)


def test_sum_h2_admission_rule(ctx):
    """n = 40, K = 1 (780 pairs), one heavy column: weight 200 000 000 is refused (4e16 x 780 > 2^64) and the message names both
    numbers; weight 100 000 000 is accepted and exact"""
    import impop_amd
    from impop_amd import _lib
    rng = np.random.default_rng(40)
    n, S = 40, 64
    m01 = rng.integers(0, 2, size=(n, S), dtype=np.uint8)
    flags = [np.ones(n, np.uint8)]
    bm = ctx.upload(impop_amd.pack_hap_major(m01), S, keep_hap_major=True)
    try:
        wt = np.ones(S, np.uint32)
        wt[11] = 200_000_000
        bm.set_site_weights(wt)
        assert (int(wt.sum()) ** 2) * 780 > 2 ** 64 - 1
        rc, msg = raw_call(ctx, bm, [(0, S, 0)], flags)
        assert rc == _lib.E_UNSUPPORTED and str(int(wt.sum())) in msg and "780" in msg, msg
        wt[11] = 100_000_000
        bm.set_site_weights(wt)
        assert (int(wt.sum()) ** 2) * 780 <= 2 ** 64 - 1
        got = bm.pairdist_scan([(0, S, 0)], flags)
        want = pp.scan(m01, [(0, S, 0)], [list(range(n))], weights=wt)
        assert int(want[0][0, 0]["sum_h2"]) > 2 ** 61  # within a factor of eight of the top
        assert_equal(got, want)
    finally:
        bm.free()


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def test_cli_tables_are_the_records(ctx, tmp_path):
    """--format pairdist: the main table and the side tables are what impop_amd.pairdist formats from BitMatrix.pairdist_scan;
    --pairdist-outgroup adds RNDMIN; --compact changes nothing; --devices 2 is refused with exit code 2"""
    import impop_amd
    from impop_amd import pairdist as pd
    from impop_amd.matrixio import MatrixFile, save_matrix
    n, origin, K = 31, 5000, 3
    m01 = pc.matrix(n)
    S = m01.shape[1]
    names = [f"S{i:02d}#1#chrT:0-1" for i in range(n)]
    pops = pc.panels(n, K)
    mpath, bed = str(tmp_path / "m.npz"), str(tmp_path / "w.bed")
    save_matrix(mpath, MatrixFile(bits=impop_amd.pack_hap_major(m01), n_site=S, names=names, origin=origin, contig="chrT"))
    rows = [(0, 256), (128, 512), (768, 1152), (0, S)]
    open(bed, "w").write("".join(f"chrT\t{origin + b}\t{origin + e}\n" for b, e in rows))
    lists = []
    for k, p in enumerate(pops):
        lists.append(str(tmp_path / f"pop{k}.txt"))
        open(lists[-1], "w").write("".join(names[i].split("#")[0] + "\n" for i in p))  # sample names: prefixes of the sequences
    bm = ctx.upload(impop_amd.pack_hap_major(m01), S, keep_hap_major=True)
    try:
        got = bm.pairdist_scan([(b, e, e - b) for b, e in rows], pc.panels_flags(n, K), hist_bins=12, hist_width=4)
    finally:
        bm.free()
    assert_equal(got, pp.scan(m01, rows, pops, 12, 4))
    regions = [f"CHM13#0#chrT:{origin + b}-{origin + e}" for b, e in rows]  # -p / --region-prefix, as every table prints it
    labels = ["pop0", "pop1", "pop2"]
    text = lambda header, table: "\n".join(["\t".join(header)] + ["\t".join(r) for r in table]) + "\n"  # noqa: E731
    script = [sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", mpath, "--bed", bed, "--format", "pairdist", "--panel"] + lists
    panp, histp = str(tmp_path / "panels.tsv"), str(tmp_path / "hist.tsv")
    main, pan, hist = pd.tables(regions, [e - b for b, e in rows], labels, names, *got)
    assert len(main) == 4 * 3 and len(pan) == 4 * 3 and hist and any(r[11] == "NA" for r in main)  # the all-identical window: GMIN NA
    for extra in ([], ["--compact"]):
        r = subprocess.run(script + ["--pairdist-panels", panp, "--pairdist-hist", histp, "--pairdist-bins", "12", "--pairdist-bin-width", "4"] + extra,
                           capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout == text(pd.MAIN_COLUMNS, main)
        assert open(panp).read() == text(pd.PANEL_COLUMNS, pan)
        assert open(histp).read() == text(pd.HIST_COLUMNS, hist)
    main_og, pan_og, _ = pd.tables(regions, [e - b for b, e in rows], labels, names, got[0], got[1], outgroup=2)
    r = subprocess.run(script + ["--pairdist-outgroup", "3", "--pairdist-panels", panp], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == text(pd.MAIN_COLUMNS + ["RNDMIN"], main_og) and open(panp).read() == text(pd.PANEL_COLUMNS, pan_og)
    assert all(row[-1] == "NA" for row in main_og if "pop2" in row[2:4]) and any(row[-1] != "NA" for row in main_og)
    assert all(row[-1] == "NA" for row in pan_og)  # no histogram: no raggedness
    r = subprocess.run(script + ["--devices", "2"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 2 and "--devices" in r.stderr
