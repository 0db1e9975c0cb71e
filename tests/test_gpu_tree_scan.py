"""GPU: impop_tree_scan — exact single / complete / average linkage trees per window — against the plain restatement
(tests/plain_tree.py: a global search per step, Python integers for the rational comparisons), byte for byte, and against itself
under every way of computing the same windows."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import pairdist_cases as pc
import plain_pca as pl
import plain_tree as pt
import tree_cases as tc
from conftest import ROOT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KNOWN = np.array([[0, 0, 0, 0], [0, 0, 0, 1], [0, 1, 1, 1], [0, 0, 0, 1]], np.uint8)


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def uploaded(ctx):
    """the case matrices on the device, one upload per n"""
    import impop_amd
    held = {}

    def get(n):
        if n not in held:
            m01 = tc.matrix(n)
            held[n] = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
        return held[n]
    yield get
    for bm in held.values():
        bm.free()


def expected(refs, K):
    """the three arrays BitMatrix.tree_scan must return for the plain references of a window list"""
    import impop_amd
    m = refs[0]["n_members"]
    recs = np.zeros(len(refs), impop_amd.TREE_WINDOW_DTYPE)
    merges = np.zeros((len(refs), m - 1), impop_amd.TREE_MERGE_DTYPE)
    panels = np.zeros((len(refs), K), impop_amd.TREE_PANEL_DTYPE) if K else None
    for w, r in enumerate(refs):
        last = r["merges"][-1]
        recs[w] = (m, r["n_sites"], r["n_zero"], r["n_tied"], r["sum_h"], last[4], last[2], last[3], 0)
        for s, g in enumerate(r["merges"]):
            merges[w, s] = g
        for p in range(K):
            q = r["panels"][p]
            panels[w, p] = (q["n_members"], q["largest_clade"], q["mrca_size"], q["mrca_merge"])
    return recs, merges, panels


def same(got, want, what):
    for g, x, name in zip(got, want, ("windows", "merges", "panels")):
        assert (g is None) == (x is None), (what, name)
        if g is None:
            continue
        if g.tobytes() != x.tobytes():
            bad = np.argwhere(g != x)
            at = tuple(bad[0])
            raise AssertionError((what, name, "first difference at", at, g[at], x[at], "of", len(bad)))


def blob(res):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in res if a is not None)


# ---- 1. parity, bytes equal -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask", tc.MASKS)
@pytest.mark.parametrize("shape", ["tiling", "sliding"])
@pytest.mark.parametrize("n", tc.NS)
def test_parity(uploaded, n, shape, mask):
    wins = pc.window_lists()[shape]
    bm = uploaded(n)
    flags = tc.flags(n, mask)
    sum_p = bm.scan(wins, mask_p=flags)["sum_p"]
    distinct = bm.haplotype_scan(wins, mask_p=flags)["n_distinct"]
    one_panel = bm.pairdist_scan(wins, [np.ones(n, np.uint8) if flags is None else flags])[0][:, 0]
    for linkage in tc.LINKAGES:
        for K in tc.KS:
            refs = tc.references(n, shape, mask, linkage, K)
            pops = tc.pop_flags(n, mask, K)
            got = bm.tree_scan(wins, mask_p=flags, pops=pops, linkage=linkage)
            same(got, expected(refs, len(pops)), (n, shape, mask, linkage, K))
            recs, merges, _ = got
            assert (recs["sum_h"] == sum_p).all() and (recs["n_members"] - recs["n_zero_merges"] == distinct).all()
            if linkage == "complete":
                assert (recs["root_num"] == one_panel["max_h"]).all()
            if linkage == "single":
                assert (merges[:, 0]["num"] == one_panel["min_h"]).all()
            if K == 0:
                no_merges = bm.tree_scan(wins, mask_p=flags, linkage=linkage, want_merges=False)
                assert no_merges[1] is None and no_merges[2] is None and no_merges[0].tobytes() == recs.tobytes()


@functools.lru_cache(maxsize=None)
def big_references(n, linkage):
    m01 = tc.matrix(n)
    return [pt.window(pl.distances(m01, w[0], w[1]), w[1] - w[0], linkage) for w in pc.window_lists()["tiling"]]


@pytest.mark.parametrize("n", tc.BIG_NS)
def test_parity_at_every_switch_of_the_kernel(ctx, n):
    """either side of the lane stride (64) and of the workgroup widths (256 / 512 / 1024 threads), and the 465 and 513 of the other
    all-pairs tests: all members, the tiling list (one window has every value 0), the three linkages"""
    import impop_amd
    wins = pc.window_lists()["tiling"]
    m01 = tc.matrix(n)
    bm = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
    try:
        for linkage in tc.LINKAGES:
            refs = big_references(n, linkage)
            assert any(r["sum_h"] == 0 for r in refs) and any(r["n_tied"] for r in refs)
            same(bm.tree_scan(wins, linkage=linkage), expected(refs, 0), (n, linkage))
    finally:
        bm.free()


# ---- 2. the known answer ----------------------------------------------------------------------------------------------------------------

def test_known_answer(ctx):
    import impop_amd
    bm = ctx.upload(impop_amd.pack_hap_major(KNOWN), 4, keep_hap_major=True)
    try:
        pops = [np.array([1, 1, 0, 0], np.uint8), np.array([0, 0, 1, 1], np.uint8)]
        recs, merges, panels = bm.tree_scan([(0, 4, 4)], pops=pops, linkage="average")
        r = recs[0]
        assert [tuple(int(x) for x in g) for g in merges[0]] == [(1, 3, 1, 1, 0), (0, 1, 1, 2, 2), (0, 2, 3, 1, 7)]
        assert tuple(int(r[f]) for f in r.dtype.names) == (4, 4, 1, 0, 9, 7, 3, 1, 0)
        assert [tuple(int(x) for x in q) for q in panels[0]] == [(2, 1, 3, 1), (2, 1, 4, 2)]
        assert [tuple(int(x) for x in g) for g in bm.tree_scan([(0, 4, 4)], linkage="single")[1][0]] == [(1, 3, 1, 1, 0), (0, 1, 1, 2, 1), (0, 2, 3, 1, 2)]
        assert [tuple(int(x) for x in g) for g in bm.tree_scan([(0, 4, 4)], linkage="complete")[1][0]] == [(1, 3, 1, 1, 0), (0, 1, 1, 2, 1), (0, 2, 3, 1, 3)]
        # a window without sites: every value 0, the tie rule's order, all tied but the last
        recs, merges, _ = bm.tree_scan([(2, 2, 0)], linkage="average")
        assert [tuple(int(x) for x in g) for g in merges[0]] == [(0, 1, 1, 1, 0), (0, 2, 2, 1, 0), (0, 3, 3, 1, 0)]
        assert tuple(int(recs[0][f]) for f in recs.dtype.names) == (4, 0, 3, 2, 0, 0, 3, 1, 0)
    finally:
        bm.free()


# ---- 3. the same windows computed in every other way: identical bytes -------------------------------------------------------------------

def inv_matrix(n):
    m01 = tc.matrix(n).copy()
    m01[:, 5::17] = 1  # all-ones and all-zeros columns: compaction drops them
    m01[:, 9::23] = 0
    return m01


def _child(path, n, shape, linkage, compact):
    import impop_amd
    ctx = impop_amd.Context(0)
    m01 = inv_matrix(n)
    bm = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
    if compact:
        full, bm = bm, bm.compact()
        full.free()
    got = bm.tree_scan(pc.window_lists()[shape], pops=pc.panels_flags(n, 3), linkage=linkage)
    np.savez(path, recs=got[0], merges=got[1], panels=got[2])
    bm.free(); ctx.close()


def run_child(n, shape, linkage, env_extra, compact=False):
    """-> (result, trace fields of the [impop_tree_scan] line)"""
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]), **env_extra)
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_tree_scan as t; t._child(sys.argv[1], %d, %r, %r, %r)"
                            % (n, shape, linkage, compact), path], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = [l for l in r.stderr.splitlines() if l.startswith("[impop_tree_scan] route=")]
        assert len(lines) == 1, r.stderr[-2000:]
        trace = dict(f.split("=") for f in lines[0].split()[1:])
        with np.load(path) as z:
            return (z["recs"].copy(), z["merges"].copy(), z["panels"].copy()), trace


def test_same_windows_same_bytes(ctx):
    """three windows per chunk, int32 Gram counts, Gram chains of one and of eight links, 64-bit sums (each read by a fresh
    process), the compacted matrix, the window list reversed and a second call: the bytes of the default call.  The sliding list
    has segmented cells.  The trace line shows that several chunks and the compact route were really taken."""
    import impop_amd
    n, shape, linkage = 465, "sliding", "average"
    wins = pc.window_lists()[shape]
    m01 = inv_matrix(n)
    pops = pc.panels_flags(n, 3)
    bm = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
    try:
        base = bm.tree_scan(wins, pops=pops, linkage=linkage)
        assert blob(bm.tree_scan(wins, pops=pops, linkage=linkage)) == blob(base)
        rev = bm.tree_scan(wins[::-1], pops=pops, linkage=linkage)
        assert blob((rev[0][::-1], rev[1][::-1], rev[2][::-1])) == blob(base)
        comp = bm.compact()
        try:
            assert blob(comp.tree_scan(wins, pops=pops, linkage=linkage)) == blob(base)
        finally:
            comp.free()
    finally:
        bm.free()
    pos = pc.panels(n, 3)
    for w in (0, 7, len(wins) - 1):  # against the restatement too: a window either side of and inside the all-identical segments
        ref = pt.window(pl.distances(m01, wins[w][0], wins[w][1]), wins[w][1] - wins[w][0], linkage, pos)
        same([a[w:w + 1] for a in base], expected([ref], 3), ("inv", w))
    same_again, trace = run_child(n, shape, linkage, {})
    assert blob(same_again) == blob(base)
    assert trace["route"] == "dense" and int(trace["chunks"]) == 1 and int(trace["windows"]) == len(wins) and trace["linkage"] == linkage
    assert (int(trace["members"]), int(trace["pops"]), int(trace["launches"])) == (n, 3, 1)
    for env in ({"IMPOP_PAIRWISE_CHUNK": "3"}, {"IMPOP_GRAM_U16": "0"}, {"IMPOP_GRAM_CHAIN": "1"}, {"IMPOP_GRAM_CHAIN": "8"}, {"IMPOP_TREE_WIDE": "1"}):
        got, trace = run_child(n, shape, linkage, env)
        assert blob(got) == blob(base), env
        if "IMPOP_PAIRWISE_CHUNK" in env:
            assert int(trace["chunks"]) >= (len(wins) + 2) // 3 and int(trace["launches"]) == int(trace["chunks"])
    got, trace = run_child(n, shape, linkage, {"IMPOP_PAIRWISE_CHUNK": "3"}, compact=True)
    assert blob(got) == blob(base) and trace["route"] == "compact" and int(trace["chunks"]) > 1


# ---- 4. weights ---------------------------------------------------------------------------------------------------------------------------

def test_weighted_equals_bp_expanded(ctx):
    """a node-level matrix with site weights gives the bytes of its bp-expanded matrix, and both the restatement's"""
    import impop_amd
    from af_cases import planted_matrix
    rng = np.random.default_rng(99)
    n, cols = 120, 400
    node = planted_matrix(n, 4, 4242)[:, :cols].copy()
    wt = rng.integers(1, 6, size=cols).astype(np.uint32)
    expanded = np.repeat(node, wt, axis=1)
    edges = np.concatenate([[0], np.cumsum(wt.astype(np.int64))])
    node_wins = [(s, min(s + 50, cols), 0) for s in range(0, cols, 50)] + [(s, min(s + 100, cols), 0) for s in range(0, cols - 50, 50)]
    bp_wins = [(int(edges[a]), int(edges[b]), 0) for a, b, _ in node_wins]
    pos = pc.panels(n, 2, planted=False)
    pops = pc.panels_flags(n, 2, planted=False)
    bw = ctx.upload(impop_amd.pack_hap_major(node), cols, keep_hap_major=True)
    be = ctx.upload(impop_amd.pack_hap_major(expanded), expanded.shape[1], keep_hap_major=True)
    try:
        bw.set_site_weights(wt)
        for linkage in tc.LINKAGES:
            refs = [pt.window(pl.distances(node, a, b, weights=wt), int(edges[b] - edges[a]), linkage, pos) for a, b, _ in node_wins]
            a = bw.tree_scan(node_wins, pops=pops, linkage=linkage)
            b = be.tree_scan(bp_wins, pops=pops, linkage=linkage)
            same(a, expected(refs, 2), ("weighted", linkage))
            assert blob(a) == blob(b)
    finally:
        bw.free(); be.free()


# ---- 5. the 128-bit path ------------------------------------------------------------------------------------------------------------------

def test_the_128_bit_path(ctx):
    """1024 members in three groups on a weighted matrix with W = 2^31 - 1: the last merges compare values whose cross products pass
    2^64 (tree_cases.wide_preconditions), and the sums need 64 bits of storage"""
    import impop_amd
    m01, wt, win = tc.wide_case()
    assert tc.wide_preconditions() >= 2 ** 64
    ref = tc.wide_reference()
    assert max(g[4] for g in ref["merges"]) >= 2 ** 32
    bm = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
    try:
        bm.set_site_weights(wt)
        same(bm.tree_scan([win], linkage="average"), expected([ref], 0), "128-bit")
    finally:
        bm.free()


# ---- 6. the upper end of the member range -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def upper_end_case():
    """1024 haplotypes, one 256-site window: a sparse random background, 12 blocks of haplotypes that carry 16 sites of their own
    each, and a few copied rows (merges at 0)"""
    rng = np.random.default_rng(1024)
    n, S = 1024, 256
    m01 = (rng.random((n, S)) < 0.05).astype(np.uint8)
    sizes = [40, 50, 60, 70, 80, 90, 100, 110, 120, 96, 104, 104]
    at = 0
    for b, sz in enumerate(sizes):
        m01[at:at + sz, 16 * b:16 * (b + 1)] = 1
        at += sz
    m01[700] = m01[3]
    m01[1023] = m01[1022]
    return m01


@pytest.mark.parametrize("linkage", tc.LINKAGES)
def test_upper_end_of_the_member_range(ctx, linkage):
    import impop_amd
    m01 = upper_end_case()
    n, S = m01.shape
    ref = pt.window(pl.distances(m01, 0, S), S, linkage)
    bm = ctx.upload(impop_amd.pack_hap_major(m01), S, keep_hap_major=True)
    try:
        same(bm.tree_scan([(0, S, S)], linkage=linkage), expected([ref], 0), ("m = 1024", linkage))
    finally:
        bm.free()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------

def raw_call(ctx, bm, wins, mask=None, pops=(), linkage=2, struct_size=None, n_pop=None, panels_out=None):
    """the C call with nothing checked on the Python side -> (return code, message)"""
    import impop_amd
    from impop_amd import _lib
    w = impop_amd.make_windows(wins)
    n_p = bm.n_hap if mask is None else int(np.asarray(mask).sum())
    packed = None if mask is None else impop_amd.pack_mask(mask, bm.n_hap)
    K = len(pops) if n_pop is None else n_pop
    pm = np.concatenate([impop_amd.pack_mask(p, bm.n_hap) for p in pops]).astype(np.uint64) if len(pops) else np.zeros(256, np.uint64)
    out = np.zeros(max(len(w), 1), impop_amd.TREE_WINDOW_DTYPE)
    merges = np.zeros((max(len(w), 1), max(n_p, 2)), impop_amd.TREE_MERGE_DTYPE)
    pan = np.zeros((max(len(w), 1), 8), impop_amd.TREE_PANEL_DTYPE)
    want_panels = (K > 0) if panels_out is None else panels_out
    prm = _lib.TreeParams(C.sizeof(_lib.TreeParams) if struct_size is None else struct_size, linkage)
    u64p = C.POINTER(C.c_uint64)
    rc = ctx._lib.impop_tree_scan(ctx.handle, bm.handle, w.ctypes.data_as(C.POINTER(_lib.Window)), len(w),
                                  None if packed is None else packed.ctypes.data_as(u64p), pm.ctypes.data_as(u64p), K, C.byref(prm),
                                  out.ctypes.data_as(C.POINTER(_lib.TreeWindow)), merges.ctypes.data_as(C.POINTER(_lib.TreeMerge)),
                                  pan.ctypes.data_as(C.POINTER(_lib.TreePanel)) if want_panels else None)
    return rc, ctx._lib.impop_last_error().decode()


def test_refusals(ctx):
    """each with its code, and nothing launched: the Gram and tree timers of the context count no launch"""
    from impop_amd import _lib
    n, S = 1030, 64
    bm = ctx.synthetic(n, S, keep_hap_major=True)
    try:
        wins = [(0, S, S)]

        def flags(idx):
            f = np.zeros(n, np.uint8)
            f[list(idx)] = 1
            return f
        one, most, fits = flags([3]), flags(range(1025)), flags(range(1024))
        ctx.gram_timing(True)
        for what, args, code, needle in (
                ("|P| = 1", dict(mask=one), _lib.E_INVALID, "fewer than 2"),
                ("|P| = 1025", dict(mask=most), _lib.E_UNSUPPORTED, "1025"),
                ("linkage = 3", dict(mask=fits, linkage=3), _lib.E_INVALID, "linkage"),
                ("struct_size", dict(mask=fits, struct_size=16), _lib.E_INVALID, "struct_size"),
                ("n_pop = 9", dict(mask=fits, n_pop=9, panels_out=True), _lib.E_INVALID, "n_pop"),
                ("n_pop without out_panels", dict(mask=fits, pops=[flags([1, 2])], panels_out=False), _lib.E_INVALID, "out_panels"),
                ("out_panels without n_pop", dict(mask=fits, panels_out=True), _lib.E_INVALID, "out_panels"),
                ("overlapping panels", dict(mask=fits, pops=[flags([1, 2]), flags([2, 3])]), _lib.E_INVALID, "disjoint"),
                ("an empty panel", dict(mask=fits, pops=[flags([1, 2]), flags([])]), _lib.E_INVALID, "empty"),
                ("a panel member outside mask_p", dict(mask=fits, pops=[flags([1, 1027])]), _lib.E_INVALID, "outside mask_p")):
            rc, msg = raw_call(ctx, bm, wins, **args)
            assert rc == code and needle in msg, (what, rc, msg)
        assert ctx.gram_elapsed()[1] == 0 and ctx.tree_elapsed()[1] == 0
        rc, msg = raw_call(ctx, bm, [], mask=fits)
        assert rc == 0, msg
        assert ctx.gram_elapsed()[1] == 0
        rc, msg = raw_call(ctx, bm, wins, mask=fits)  # 1024 members are accepted
        assert rc == 0, msg
        t, chunks = ctx.tree_elapsed()
        assert chunks == 1 and t > 0 and ctx.gram_elapsed()[1] >= 1
        # the device error word: the call that sees it fails once and clears it
        _lib.check(ctx._lib.impop_debug_raise_device_error(ctx.handle, 1))
        rc, msg = raw_call(ctx, bm, wins, mask=fits)
        assert rc == _lib.E_INTERNAL, msg
        rc, msg = raw_call(ctx, bm, wins, mask=fits)
        assert rc == 0, msg
    finally:
        ctx.gram_timing(False)
        bm.free()


def _refusal_child():
    import impop_amd
    from impop_amd import _lib
    ctx = impop_amd.Context(0)
    bm = ctx.synthetic(1030, 64, keep_hap_major=True)
    f = np.zeros(1030, np.uint8); f[:1025] = 1
    assert raw_call(ctx, bm, [(0, 64, 64)], mask=f)[0] == _lib.E_UNSUPPORTED
    assert raw_call(ctx, bm, [(0, 64, 64)], linkage=7)[0] == _lib.E_INVALID
    print("refused", file=sys.stderr)
    f[1024] = 0
    assert raw_call(ctx, bm, [(0, 64, 64)], mask=f)[0] == 0
    bm.free(); ctx.close()


# ---- 7b / 8. the trace: nothing launched by a refused call; the line's fields ---------------------------------------------------------------

def test_trace_line_and_no_launch_when_refused():
    env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
    r = subprocess.run([sys.executable, "-c", "import test_gpu_tree_scan as t; t._refusal_child()"], capture_output=True, text=True, cwd=ROOT,
                       env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    before, after = r.stderr.split("refused\n")
    assert "[impop_gram]" not in before and "[impop_tree_scan]" not in before  # no launch, not even the front end entered
    assert "[impop_gram]" in after
    lines = [l for l in after.splitlines() if l.startswith("[impop_tree_scan] route=")]  # (the front end's timing laps carry the name too)
    assert len(lines) == 1
    assert re.fullmatch(r"\[impop_tree_scan\] route=(dense|compact) linkage=(single|complete|average) members=\d+ pops=\d+ windows=\d+ "
                        r"chunks=\d+ launches=\d+ rows_recomputed=\d+ tied_windows=\d+", lines[0]), lines[0]
    trace = dict(f.split("=") for f in lines[0].split()[1:])
    assert (trace["route"], trace["linkage"], int(trace["members"]), int(trace["pops"]), int(trace["windows"])) == ("dense", "average", 1024, 0, 1)
    assert int(trace["chunks"]) == 1 and int(trace["launches"]) == 1 and int(trace["rows_recomputed"]) >= 2 * 1023 * 1
    assert int(trace["tied_windows"]) in (0, 1)


# ---- 9. the command line --------------------------------------------------------------------------------------------------------------------

def test_cli_writes_the_four_outputs_for_two_matrices(ctx, tmp_path):
    """scripts/impop_tree.py on a BED over two matrices with two panels: the main table, the Newick lines, the merge and panel tables
    parse; the Newick leaves are the names; rf_prev is the plain restatement's; --compact changes nothing"""
    import impop_amd
    from impop_amd import tree
    from impop_amd.matrixio import MatrixFile, save_matrix
    n = 31
    m01 = tc.matrix(n)
    S = m01.shape[1]
    mats, bed_rows = [], []
    for c, (contig, origin) in enumerate((("chrA", 5000), ("chrB", 100))):
        names = [f"S{i:02d}#1#{contig}:0-1" for i in range(n)]
        path = str(tmp_path / f"{contig}.npz")
        mm = m01 if c == 0 else np.ascontiguousarray(m01[:, ::-1])
        save_matrix(path, MatrixFile(bits=impop_amd.pack_hap_major(mm), n_site=S, names=names, origin=origin, contig=contig))
        mats.append((path, contig, origin, names, mm))
        bed_rows += [(contig, origin + b, origin + e) for b, e in ((0, 256), (768, 1152), (0, S))]
    bed = str(tmp_path / "w.bed")
    open(bed, "w").write("".join(f"{c}\t{s}\t{e}\n" for c, s, e in bed_rows))
    pos = pc.panels(n, 2)
    panel_files = []
    for p, members in enumerate(pos):
        path = str(tmp_path / f"panel{p}.txt")
        open(path, "w").write("".join(f"S{i:02d}\n" for i in members))
        panel_files.append(path)
    out = {k: str(tmp_path / f"{k}.out") for k in ("nwk", "merges", "panels")}
    script = [sys.executable, os.path.join(ROOT, "scripts", "impop_tree.py"), "--bed", bed, "--matrix", mats[0][0], mats[1][0],
              "--panel"] + panel_files + ["--tree-linkage", "average", "--tree-newick", out["nwk"], "--tree-merges", out["merges"],
                                          "--tree-panels", out["panels"]]
    texts = []
    for extra in ([], ["--compact"]):
        r = subprocess.run(script + extra, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        texts.append((r.stdout,) + tuple(open(out[k]).read() for k in ("nwk", "merges", "panels")))
    assert texts[0] == texts[1]
    main, nwk, merges, panels = (t.splitlines() for t in texts[0])
    assert main[0].split("\t") == list(tree.MAIN_COLUMNS) and len(main) == 1 + len(bed_rows)
    assert merges[0].split("\t") == list(tree.MERGE_COLUMNS) and len(merges) == 1 + len(bed_rows) * (n - 1)
    assert panels[0].split("\t") == list(tree.PANEL_COLUMNS) and len(panels) == 1 + len(bed_rows) * 2
    assert len(nwk) == len(bed_rows)
    row = 0
    for path, contig, origin, names, mm in mats:
        prev = None
        for c, s, e in (r for r in bed_rows if r[0] == contig):
            ref = pt.window(pl.distances(mm, s - origin, e - origin), e - s, "average", pos)
            f = main[1 + row].split("\t")
            assert f[:3] == [c, str(s), str(e)] and [int(x) for x in f[3:7]] == [n, e - s, n - ref["n_zero"], ref["n_tied"]]
            assert float(f[7]) == pt.heights(ref["merges"], "average")[-1]
            assert f[8] == ("NA" if prev is None else str(pt.rf(prev["merges"], ref["merges"])))
            where, text = nwk[row].split("\t")[:-1], nwk[row].split("\t")[-1]
            assert where == [c, str(s), str(e)] and text == pt.newick(ref["merges"], names, "average")
            leaves = re.findall(r"[(,]('(?:[^']|'')*'|[^(),:;']+):", text)  # the names hold a colon: they are quoted
            assert sorted(x.strip("'") for x in leaves) == sorted(names) and all(x.startswith("'") for x in leaves)
            got = [tuple(int(x) for x in l.split("\t")[4:9]) for l in merges[1 + row * (n - 1): 1 + (row + 1) * (n - 1)]]
            assert got == ref["merges"]
            for p in range(2):
                q = panels[1 + row * 2 + p].split("\t")
                want = ref["panels"][p]
                assert [int(x) for x in q[4:7]] == [want["n_members"], want["largest_clade"], want["mrca_size"]]
                assert q[8] == ("1" if want["mrca_size"] == want["n_members"] else "0")
            prev = ref
            row += 1
