"""GPU: impop_pca_scan — the principal components of the haplotypes per window — certified against the plain restatement
(tests/plain_pca.py: the exact integers 2 m^2 B and numpy.linalg.eigh), with every bound derived from tol, the residual theorem of
symmetric matrices and the precision of the number format, and against itself under every way of computing the same windows."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import pairdist_cases as pc
import pca_cases as pcs
import plain_pca as pl
from conftest import ROOT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -52
TOL = pcs.TOL


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
            m01 = pcs.matrix(n)
            held[n] = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
        return held[n]
    yield get
    for bm in held.values():
        bm.free()


def in_regime(ref, k):
    """the preconditions of pca_cases on one reference window"""
    if ref["sum_h"] == 0:
        return True
    return pcs.regime_ratio(ref, k) <= 0.9 and not any(1e-13 * ref["trace"] < ref["lam"][j] < 1e-7 * ref["trace"]
                                                       for j in range(min(k, ref["n_members"])))


def certify(rec, vec, ref, k, tol=TOL, what=""):
    """the checks of one window against its exact spectrum; vec: [k, m]"""
    m = ref["n_members"]
    lam1 = float(ref["lam"][0])
    assert (int(rec["n_members"]), int(rec["n_sites"]), int(rec["sum_h"])) == (m, ref["n_sites"], ref["sum_h"]), what
    rank = int(rec["rank"])
    want_rank = pcs.rank_at(ref, k, tol)
    assert rank == want_rank, (what, rank, want_rank)
    assert int(rec["flags"]) == 0 and int(rec["reserved"]) == 0, (what, int(rec["flags"]), int(rec["iterations"]))
    assert (int(rec["iterations"]) == 0) == (ref["sum_h"] == 0), what
    assert np.isnan(rec["lambda"][k:]).all() and np.isnan(rec["resid"][rank:]).all(), what
    assert (rec["lambda"][rank:k] == 0.0).all() and (vec[rank:] == 0.0).all(), what
    bound = 2 * tol * lam1
    for j in range(rank):
        v, lam = vec[j], float(rec["lambda"][j])
        assert abs(lam - ref["lam"][j]) <= bound, (what, j, lam, ref["lam"][j], bound)
        res = float(np.linalg.norm(ref["B"] @ v - lam * v))
        assert res <= bound, (what, j, res, bound)
        assert float(rec["resid"][j]) <= tol * float(rec["lambda"][0]), (what, j)
        assert abs(v.sum()) <= 16 * m * EPS, (what, j, v.sum())
        assert pl.sign_ok(v), (what, j)
        if j:
            assert lam <= float(rec["lambda"][j - 1]), what
    if rank:
        V = vec[:rank]
        assert np.abs(V @ V.T - np.eye(rank)).max() <= 16 * m * EPS, (what, np.abs(V @ V.T - np.eye(rank)).max())
    if rank == k and k < m and ref["lam"][k - 1] - ref["lam"][k] >= 0.1 * lam1:  # Davis-Kahan: residual / gap
        U = ref["vec"][:, :k]
        sine = np.linalg.norm(vec[:k].T - U @ (U.T @ vec[:k].T), 2)
        assert sine <= 20 * tol, (what, sine)


# ---- 1. certified parity ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", pcs.KS)
@pytest.mark.parametrize("mask", pcs.MASKS)
@pytest.mark.parametrize("shape", ["tiling", "sliding"])
@pytest.mark.parametrize("n", pcs.NS)
def test_certified_parity(uploaded, n, shape, mask, k):
    wins = pc.window_lists()[shape]
    refs = pcs.references(n, shape, mask)
    assert all(in_regime(r, k) for r in refs) and any(r["sum_h"] == 0 for r in refs)
    bm = uploaded(n)
    recs, vecs, d2 = bm.pca_scan(wins, mask_p=pcs.flags(n, mask), k=k)
    assert d2 is None and vecs.shape == (len(wins), k, len(pcs.members(n, mask)))
    assert (bm.scan(wins, mask_p=pcs.flags(n, mask))["sum_p"] == recs["sum_h"]).all()
    for w, ref in enumerate(refs):
        certify(recs[w], vecs[w], ref, k, what=(n, shape, mask, k, w))
    if mask == "three" and k == 8:
        assert int(recs["rank"].max()) == 2
    no_vec = bm.pca_scan(wins, mask_p=pcs.flags(n, mask), k=k, want_vectors=False)
    assert no_vec[1] is None and no_vec[0].tobytes() == recs.tobytes()


# ---- 2. the known answer ---------------------------------------------------------------------------------------------------------

def test_known_answer(ctx):
    import impop_amd
    m01 = np.array([[0, 0, 0, 0], [0, 0, 0, 1], [0, 1, 1, 1], [0, 0, 0, 1]], np.uint8)
    bm = ctx.upload(impop_amd.pack_hap_major(m01), 4, keep_hap_major=True)
    try:
        recs, vecs, _ = bm.pca_scan([(0, 4, 4)], k=4)
    finally:
        bm.free()
    r = recs[0]
    assert (int(r["n_members"]), int(r["n_sites"]), int(r["sum_h"]), int(r["rank"]), int(r["flags"])) == (4, 4, 9, 2, 0)
    want = [(9 + 17 ** 0.5) / 8, (9 - 17 ** 0.5) / 8]
    assert all(abs(float(r["lambda"][j]) - want[j]) <= 2 * TOL * want[0] for j in range(2))
    assert (r["lambda"][2:4] == 0.0).all() and np.isnan(r["lambda"][4:]).all() and (vecs[0, 2:] == 0.0).all()
    assert np.abs(vecs[0, 0] - np.array([-0.472668, -0.184524, 0.841716, -0.184524])).max() < 1e-6
    certify(r, vecs[0], pl.window(pl.distances(m01, 0, 4), 4, 4), 4)


# ---- 3. the same windows computed in every other way: identical bytes -------------------------------------------------------------

def inv_matrix(n):
    m01 = pcs.matrix(n).copy()
    m01[:, 5::17] = 1  # all-ones and all-zeros columns: compaction drops them
    m01[:, 9::23] = 0
    return m01


def blob(res):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in res if a is not None)


def _child(path, n, shape, k, compact):
    import impop_amd
    ctx = impop_amd.Context(0)
    m01 = inv_matrix(n)
    bm = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
    if compact:
        full, bm = bm, bm.compact()
        full.free()
    got = bm.pca_scan(pc.window_lists()[shape], k=k, want_dist=True)
    np.savez(path, recs=got[0], vecs=got[1], d2=got[2])
    bm.free(); ctx.close()


def run_child(n, shape, k, env_extra, compact=False):
    """-> (result, trace fields of the [impop_pca_scan] line)"""
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]), **env_extra)
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_pca_scan as t; t._child(sys.argv[1], %d, %r, %d, %r)" % (n, shape, k, compact),
                            path], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = [l for l in r.stderr.splitlines() if l.startswith("[impop_pca_scan] route=")]
        assert len(lines) == 1, r.stderr[-2000:]
        trace = dict(f.split("=") for f in lines[0].split()[1:])
        with np.load(path) as z:
            return (z["recs"].copy(), z["vecs"].copy(), z["d2"].copy()), trace


@pytest.mark.parametrize("shape", ["tiling", "sliding"])
def test_same_windows_same_bytes(ctx, shape):
    """three windows per chunk, int32 Gram counts, a Gram chain of one link (each read by a fresh process), the compacted matrix, the
    window list reversed and a second call: the bytes of the default call, distances included.  The sliding list has segmented
    cells.  The trace line shows that several chunks and the compact route were really taken."""
    import impop_amd
    n, k = 465, 4
    wins = pc.window_lists()[shape]
    m01 = inv_matrix(n)
    refs = [pl.window(pl.distances(m01, win[0], win[1]), win[1] - win[0], k) for win in wins]
    assert all(in_regime(r, k) for r in refs)
    bm = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
    try:
        base = bm.pca_scan(wins, k=k, want_dist=True)
        assert blob(bm.pca_scan(wins, k=k, want_dist=True)) == blob(base)
        rev = bm.pca_scan(wins[::-1], k=k, want_dist=True)
        assert blob((rev[0][::-1], rev[1][::-1], rev[2][::-1, ::-1])) == blob(base)
        comp = bm.compact()
        try:
            assert blob(comp.pca_scan(wins, k=k, want_dist=True)) == blob(base)
        finally:
            comp.free()
    finally:
        bm.free()
    for w, ref in enumerate(refs):
        certify(base[0][w], base[1][w], ref, k, what=(shape, w))
    same, trace = run_child(n, shape, k, {})
    assert blob(same) == blob(base)
    assert trace["route"] == "dense" and int(trace["chunks"]) == 1 and int(trace["windows"]) == len(wins) and trace["dist"] == "on"
    assert (int(trace["members"]), int(trace["k"]), int(trace["unconverged"])) == (n, k, 0)
    assert int(trace["iterations_max"]) == int(base[0]["iterations"].max()) and int(trace["launches"]) == 2
    for env in ({"IMPOP_PAIRWISE_CHUNK": "3"}, {"IMPOP_GRAM_U16": "0"}, {"IMPOP_GRAM_CHAIN": "1"}):
        got, trace = run_child(n, shape, k, env)
        assert blob(got) == blob(base), env
        if "IMPOP_PAIRWISE_CHUNK" in env:
            assert int(trace["chunks"]) >= (len(wins) + 2) // 3 and int(trace["launches"]) == int(trace["chunks"]) + 1
    got, trace = run_child(n, shape, k, {"IMPOP_PAIRWISE_CHUNK": "3"}, compact=True)
    assert blob(got) == blob(base) and trace["route"] == "compact" and int(trace["chunks"]) > 1


# ---- 4. weights ---------------------------------------------------------------------------------------------------------------------

def test_weighted_equals_bp_expanded(ctx):
    """A node-level matrix with site weights gives what its bp-expanded matrix gives: integers exactly, eigenvalues within the
    bound of the parity test (both against the exact spectrum of the weighted distances)."""
    import impop_amd
    from af_cases import planted_matrix
    rng = np.random.default_rng(99)
    n, cols, k = 120, 400, 4
    node = planted_matrix(n, 4, 4242)[:, :cols].copy()
    wt = rng.integers(1, 6, size=cols).astype(np.uint32)
    expanded = np.repeat(node, wt, axis=1)
    edges = np.concatenate([[0], np.cumsum(wt.astype(np.int64))])
    node_wins = [(s, min(s + 50, cols), 0) for s in range(0, cols, 50)] + [(s, min(s + 100, cols), 0) for s in range(0, cols - 50, 50)]
    bp_wins = [(int(edges[a]), int(edges[b]), 0) for a, b, _ in node_wins]
    refs = [pl.window(pl.distances(node, a, b, weights=wt), int(edges[b] - edges[a]), k) for a, b, _ in node_wins]
    assert all(in_regime(r, k) for r in refs)
    bw = ctx.upload(impop_amd.pack_hap_major(node), cols, keep_hap_major=True)
    be = ctx.upload(impop_amd.pack_hap_major(expanded), expanded.shape[1], keep_hap_major=True)
    try:
        bw.set_site_weights(wt)
        a = bw.pca_scan(node_wins, k=k)
        b = be.pca_scan(bp_wins, k=k)
        for f in ("n_members", "n_sites", "rank", "flags", "sum_h"):
            assert (a[0][f] == b[0][f]).all(), f
        for w, ref in enumerate(refs):
            certify(a[0][w], a[1][w], ref, k, what=("weighted", w))
            certify(b[0][w], b[1][w], ref, k, what=("expanded", w))
        assert blob(a) == blob(b)  # the solver reads the same integers: the same bytes
    finally:
        bw.free(); be.free()


# ---- 5. the window-to-window distances ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 8])
def test_distance_matrix(uploaded, k):
    """against numpy from the RETURNED eigenvalues and vectors; symmetric, zero diagonal, NaN rows and columns exactly for the
    rank-0 windows; the same site range listed twice is at distance <= the bound"""
    n = 65
    wins = pc.window_lists()["tiling"] + pc.window_lists()["sliding"][:3] + [pc.window_lists()["tiling"][0]]
    recs, vecs, d2 = uploaded(n).pca_scan(wins, k=k, want_dist=True)
    assert (recs["flags"] == 0).all()
    dead = recs["rank"] == 0
    assert dead.any() and not dead.all()
    bound = 4 * k * k * n * EPS
    assert d2.shape == (len(wins), len(wins)) and np.isnan(d2[dead]).all() and np.isnan(d2[:, dead]).all()
    live = np.flatnonzero(~dead)
    assert not np.isnan(d2[np.ix_(live, live)]).any() and (d2[np.ix_(live, live)] >= 0).all()
    assert (d2[live, live] == 0.0).all() and (d2[np.ix_(live, live)] == d2[np.ix_(live, live)].T).all()
    for a in live:
        for b in live:
            if a != b:
                want = pl.dist2(recs[a]["lambda"], vecs[a], recs[b]["lambda"], vecs[b], k)
                assert abs(d2[a, b] - want) <= bound, (a, b, d2[a, b], want)
    assert d2[0, len(wins) - 1] <= bound
    assert d2[np.ix_(live, live)].max() > 0.01  # windows of different segments differ


# ---- 6. the upper end of the member range ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def upper_end_case():
    """1024 haplotypes, one 256-site window: a sparse random background, and 12 blocks of haplotypes of different sizes that carry
    16 sites of their own each"""
    rng = np.random.default_rng(1024)
    n, S = 1024, 256
    m01 = (rng.random((n, S)) < 0.05).astype(np.uint8)
    sizes = [40, 50, 60, 70, 80, 90, 100, 110, 120, 96, 104, 104]
    assert sum(sizes) == n
    at = 0
    for b, sz in enumerate(sizes):
        m01[at:at + sz, 16 * b:16 * (b + 1)] = 1
        at += sz
    return m01


def test_upper_end_of_the_member_range(ctx):
    import impop_amd
    m01 = upper_end_case()
    n, S, k = m01.shape[0], m01.shape[1], 8
    ref = pl.window(pl.distances(m01, 0, S), S, k)
    assert in_regime(ref, k) and pcs.rank_at(ref, k) == k
    bm = ctx.upload(impop_amd.pack_hap_major(m01), S, keep_hap_major=True)
    try:
        recs, vecs, _ = bm.pca_scan([(0, S, S)], k=k)
        assert int(bm.scan([(0, S, S)])["sum_p"][0]) == int(recs[0]["sum_h"])
    finally:
        bm.free()
    certify(recs[0], vecs[0], ref, k, what="m = 1024")


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------

def raw_call(ctx, bm, wins, mask=None, k=2, tol=1e-10, max_iter=500, vectors=True, dist=False, struct_size=None):
    """the C call with nothing checked on the Python side -> (return code, message)"""
    import ctypes as C
    import impop_amd
    from impop_amd import _lib
    w = impop_amd.make_windows(wins)
    n_p = bm.n_hap if mask is None else int(np.asarray(mask).sum())
    packed = None if mask is None else impop_amd.pack_mask(mask, bm.n_hap)
    out = np.zeros(max(len(w), 1), impop_amd.PCA_WINDOW_DTYPE)
    vec = np.zeros((max(len(w), 1), 8, max(n_p, 1)), np.float64)
    d2 = np.zeros((max(len(w), 1), max(len(w), 1)), np.float64)
    prm = _lib.PcaParams(C.sizeof(_lib.PcaParams) if struct_size is None else struct_size, k, tol, max_iter, 0)
    f64p = C.POINTER(C.c_double)
    rc = ctx._lib.impop_pca_scan(ctx.handle, bm.handle, w.ctypes.data_as(C.POINTER(_lib.Window)), len(w),
                                 None if packed is None else packed.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(prm),
                                 out.ctypes.data_as(C.POINTER(_lib.PcaWindow)), vec.ctypes.data_as(f64p) if vectors else None,
                                 d2.ctypes.data_as(f64p) if dist else None)
    return rc, ctx._lib.impop_last_error().decode()


def test_refusals(ctx):
    """each with its code, and nothing launched: the Gram and eigen timers of the context count no launch"""
    from impop_amd import _lib
    n, S = 1030, 64
    bm = ctx.synthetic(n, S, keep_hap_major=True)
    try:
        wins = [(0, S, S)]
        one = np.zeros(n, np.uint8); one[3] = 1
        most = np.zeros(n, np.uint8); most[:1025] = 1
        fits = np.zeros(n, np.uint8); fits[:1024] = 1
        ctx.gram_timing(True)
        for what, args, code, needle in (("|P| = 1", dict(mask=one), _lib.E_INVALID, "fewer than 2"),
                                         ("|P| = 1025", dict(mask=most), _lib.E_UNSUPPORTED, "1025"),
                                         ("k = 9", dict(mask=fits, k=9), _lib.E_INVALID, "k must be"),
                                         ("k = 0", dict(mask=fits, k=0), _lib.E_INVALID, "k must be"),
                                         ("tol = 0", dict(mask=fits, tol=0.0), _lib.E_INVALID, "tol"),
                                         ("tol = NaN", dict(mask=fits, tol=float("nan")), _lib.E_INVALID, "tol"),
                                         ("max_iter = 0", dict(mask=fits, max_iter=0), _lib.E_INVALID, "max_iter"),
                                         ("struct_size", dict(mask=fits, struct_size=16), _lib.E_INVALID, "struct_size"),
                                         ("out_dist2 without vectors", dict(mask=fits, vectors=False, dist=True), _lib.E_INVALID, "out_vectors")):
            rc, msg = raw_call(ctx, bm, wins, **args)
            assert rc == code and needle in msg, (what, rc, msg)
        assert ctx.gram_elapsed()[1] == 0 and ctx.pca_elapsed()[1] == 0
        rc, msg = raw_call(ctx, bm, [], mask=fits)
        assert rc == 0, msg
        assert ctx.gram_elapsed()[1] == 0
        rc, msg = raw_call(ctx, bm, wins, mask=fits)  # 1024 members are accepted
        assert rc == 0, msg
        t, chunks = ctx.pca_elapsed()
        assert chunks == 1 and t[0] > 0 and t[1] == 0 and ctx.gram_elapsed()[1] >= 1
        # the device error word: the call that sees it fails once and clears it
        _lib.check(ctx._lib.impop_debug_raise_device_error(ctx.handle, 1))
        rc, msg = raw_call(ctx, bm, wins, mask=fits)
        assert rc == _lib.E_INTERNAL, msg
        rc, msg = raw_call(ctx, bm, wins, mask=fits)
        assert rc == 0, msg
    finally:
        ctx.gram_timing(False)
        bm.free()


# ---- 8. max_iter ------------------------------------------------------------------------------------------------------------------------

def test_one_iteration_is_flagged_not_failed(uploaded):
    """max_iter = 1 on a structured window: flag bit 0, iterations = 1, the last iterate with residuals that are not understated;
    a window of rank 0 in the same call is not flagged"""
    n, k = 65, 2
    wins = pc.window_lists()["tiling"]
    refs = pcs.references(n, "tiling", "all")
    recs, vecs, _ = uploaded(n).pca_scan(wins, k=k, max_iter=1)
    for w, ref in enumerate(refs):
        r = recs[w]
        if ref["sum_h"] == 0:
            assert (int(r["flags"]), int(r["iterations"]), int(r["rank"])) == (0, 0, 0)
            continue
        assert int(r["flags"]) & 1 and int(r["iterations"]) == 1 and 1 <= int(r["rank"]) <= k
        for j in range(int(r["rank"])):
            v = vecs[w, j]
            assert abs(np.linalg.norm(v) - 1) <= 16 * n * EPS
            assert float(r["resid"][j]) >= np.linalg.norm(ref["B"] @ v - float(r["lambda"][j]) * v) / 2
        assert np.isnan(r["resid"][int(r["rank"]):]).all()
    full = uploaded(n).pca_scan(wins, k=k)[0]
    assert (full["flags"] == 0).all() and int(full["iterations"].max()) > 1


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def test_cli_writes_the_three_tables_for_two_matrices(ctx, tmp_path):
    """scripts/impop_pca.py on a BED over two matrices: the main and vector tables are what impop_amd.pca formats from
    BitMatrix.pca_scan; --pca-dist takes one matrix and writes the .npy with its region names; --compact changes nothing"""
    import impop_amd
    from impop_amd import pca
    from impop_amd.matrixio import MatrixFile, save_matrix
    n, k = 31, 3
    m01 = pcs.matrix(n)
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
    want_main, want_vec = [], []
    for path, contig, origin, names, mm in mats:
        rows = [(s - origin, e - origin) for c, s, e in bed_rows if c == contig]
        bm = ctx.upload(impop_amd.pack_hap_major(mm), S, keep_hap_major=True)
        try:
            recs, vecs, d2 = bm.pca_scan([(b, e, e - b) for b, e in rows], k=k, want_dist=True)
        finally:
            bm.free()
        regions = [f"CHM13#0#{contig}:{origin + b}-{origin + e}" for b, e in rows]
        a, b = pca.tables(regions, [e - b for b, e in rows], names, recs, vecs, k)
        want_main += a
        want_vec += b
        last = (regions, d2)
    text = lambda header, table: "\n".join(["\t".join(header)] + ["\t".join(r) for r in table]) + "\n"  # noqa: E731
    script = [sys.executable, os.path.join(ROOT, "scripts", "impop_pca.py"), "--bed", bed, "--pca-k", str(k)]
    vecp, distp = str(tmp_path / "vec.tsv"), str(tmp_path / "d.npy")
    for extra in ([], ["--compact"]):
        r = subprocess.run(script + ["--matrix", mats[0][0], mats[1][0], "--pca-vectors", vecp] + extra, capture_output=True, text=True,
                           cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout == text(pca.main_columns(k), want_main)
        assert open(vecp).read() == text(pca.vector_columns(k), want_vec)
    r = subprocess.run(script + ["--matrix", mats[1][0], "--pca-dist", distp], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and "no matrix holds chromosome chrA" in r.stderr, r.stderr[-3000:]
    assert r.stdout == text(pca.main_columns(k), want_main[3:])
    assert np.load(distp).tobytes() == last[1].tobytes() and open(distp + ".tsv").read().split() == last[0]
    r = subprocess.run(script + ["--matrix", mats[0][0], mats[1][0], "--pca-dist", distp], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 2 and "single --matrix" in r.stderr
