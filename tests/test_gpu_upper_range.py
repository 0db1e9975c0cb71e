"""Every kernel at the upper end of its documented haplotype range (run with -m gpu on an MI355X).

The rest of the suite lives at n = 31 .. 1030 and 4096.  Here each entry point is taken to the limit its code states, and
one step beyond it where that step must be refused by an argument check (never by a fault):

  impop_cluster_from_identity   n <= 12798 (IMPOP_CLUSTER_MAX_N); from n = 4095 the launch asks for more than 48 KiB of LDS
  impop_afs                     masks of up to 16383 haplotypes (48 .. 64 KiB of LDS from 12288), any number of windows
  impop_site_counts             any n
  impop_ehh                     more than 256 members (a second column of workgroups), wide rows
  impop_scan* / impop_scan_multi  n_hap <= 65535; the rare entries' 16-bit haplotype indices next to their 0xFFFF sentinel
  impop_pairwise_counts         n = 16384 / 16385, where the minor-allele polarity of the Gram operand switches off
  impop_pica2_pair_terms        directly, against pica2.py:125-145

The calls added since then are in tests/test_gpu_upper_range_scans.py (the wide matrices both files use come from
tests/wide_cases.py):

  impop_dstat_scan / impop_sfs_scan  n_hap <= 65535: Gf > 4, 56 .. 64 KiB of mask LDS, products next to 2^30, sums next to 2^62
  impop_sfs_scan's tables            a histogram that fills the 160 KiB of LDS exactly, one bin more, 65536 bins
  impop_haplotype_scan / impop_ld_scan / impop_diploid_scan / impop_ibs_scan / impop_ehh_scan
                                     their <= 4096 members (2048 individuals) scattered over a 65535-haplotype matrix

The references are tests/plain_refs.py (pinned to the goldens and the C oracle by tests/test_plain_refs.py); the doubles of a
scan record come from the oracle's site-count formulation under the tolerance policy of INTEGRATION.md 4 (conftest.stat_close).
Everything else is exact."""
import itertools
import math

import numpy as np
import pytest

import plain_refs as pr
from conftest import stat_close
from wide_cases import SCAN_S, _crafted_wide, _scan_windows, _special  # noqa: F401 (moved there unchanged)

pytestmark = pytest.mark.gpu

INT_KEYS = ("n_sites", "s_all", "s_p", "s_a", "s_b", "sum_p", "sum_a", "sum_b", "sum_ab")
DBL_KEYS = ("pi", "pi_site", "pi_a", "pi_b", "pi_xy", "dxy", "da", "fst", "tajima_d")
PAIR_KEYS = ("fst", "pi_a", "pi_b", "pi_xy", "dxy", "da")
KINDS = ({}, {"rare_split": False}, {"dense_scan": True})  # split index, unsplit index, no index


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    assert c.device_name().startswith("gfx950")
    yield c
    c.close()


def _flags(idx, n):
    f = np.zeros(n, np.uint8)
    f[np.asarray(idx, dtype=np.int64)] = 1
    return f


# ---- 1. af clustering ------------------------------------------------------------------------------------------------

AF_SIZES = (1, 2, 31, 32, 33, 64, 65, 255, 256, 257, 465, 1023, 4094, 4095, 4096, 12798)
AF_THR = 0.9


def _af_table(n, rng):
    """every value below the threshold, ~3 % NaN holes on both sides of the diagonal, no self rows"""
    t = np.full((n, n), 0.5)
    k = int(0.03 * n * n / 2)
    i, j = rng.integers(0, n, k), rng.integers(0, n, k)
    t[i, j] = np.nan
    t[j, i] = np.nan
    t[np.arange(n), np.arange(n)] = np.nan
    return t


def _link(t, i, j, v=0.95):
    t[i, j] = v
    t[j, i] = v


def _af_family(name, n, rng):
    t = _af_table(n, rng)
    perm = rng.permutation(n)
    if name == "singletons":
        pass
    elif name == "giant":  # a random tree under permuted labels plus as many extra edges
        if n > 1:
            child = np.arange(1, n)
            parent = (rng.random(n - 1) * child).astype(np.int64)
            _link(t, perm[child], perm[parent])
            _link(t, rng.integers(0, n, n), rng.integers(0, n, n), 0.97)
            t[np.arange(n), np.arange(n)] = np.nan
    elif name == "equal":  # clusters of 4 (and one remainder), labels permuted: the order among equals is by smallest member
        for a, b in itertools.combinations(range(4), 2):
            m = (n // 4) * 4
            _link(t, perm[a:m:4], perm[b:m:4])
        if n % 4 > 1:
            _link(t, perm[-1], perm[-2])
    elif name == "star":
        if n > 1:
            _link(t, perm[0], perm[1:])
    elif name in ("bridge_eq", "bridge_below"):  # two cliques and one edge at the threshold / one ulp below it
        h = n // 2
        for part in (perm[:h], perm[h:]):
            t[np.ix_(part, part)] = 0.95
        t[np.arange(n), np.arange(n)] = np.nan
        if h:
            _link(t, perm[0], perm[-1], AF_THR if name == "bridge_eq" else np.nextafter(AF_THR, 0.0))
    elif name == "path":  # the long-diameter case of label propagation
        if n > 1:
            _link(t, perm[:-1], perm[1:])
    elif name == "lower_only":  # the giant family with every pair present BELOW the diagonal only
        t = _af_family("giant", n, rng)
        t[np.triu_indices(n, 0)] = np.nan
    else:
        raise KeyError(name)
    return t


def _af_families(n):
    fams = ["singletons", "giant", "equal", "star", "bridge_eq", "bridge_below"]
    if n <= 2048:
        fams.append("path")  # one workgroup re-reads the whole adjacency per iteration: kept off the large sizes
    if n <= 4096:
        fams.append("lower_only")
    return fams


@pytest.mark.parametrize("n", AF_SIZES)
def test_af_cluster_up_to_the_lds_limit(ctx, oracle, n):
    """cluster_of, K and sizes equal ref_components exactly (and oracle.af_cluster where n <= 2048) on every graph family.
    4095 is the first size whose launch asks for more than 48 KiB of dynamic LDS, 12798 the largest accepted."""
    rng = np.random.default_rng(1000 + n)
    for fam in _af_families(n):
        t = _af_family(fam, n, rng)
        want_cl, want_K, want_sz = pr.ref_components(pr.adjacency(t, AF_THR))
        cl, K, sz = ctx.cluster_from_identity(t, AF_THR)
        assert K == want_K, (n, fam, K, want_K)
        assert sz.astype(np.int64).tolist() == want_sz.tolist(), (n, fam)
        assert (cl.astype(np.int64) == want_cl).all(), (n, fam)
        if n <= 2048:
            ocl, oK, osz = oracle.af_cluster(t, AF_THR)
            assert oK == K and (ocl == cl).all() and (osz == sz).all(), (n, fam)
        # what the family is for
        if fam == "singletons":
            assert K == n
        elif fam in ("giant", "star", "path", "bridge_eq", "lower_only"):
            assert K == 1 and int(sz[0]) == n, (n, fam, K)
        elif fam == "bridge_below" and n >= 2:
            assert K == 2 and sorted(sz.tolist()) == sorted([n // 2, n - n // 2]), (n, K)
        elif fam == "equal" and n >= 8:
            assert K >= n // 4 and int(sz[0]) == 4


def test_af_cluster_limit_is_refused_before_any_launch(ctx):
    """n = IMPOP_CLUSTER_MAX_N + 1 returns IMPOP_E_INVALID from the argument check (nothing is uploaded or launched), and the
    message names the real limit."""
    import impop_amd
    from impop_amd import _lib
    n = 12799
    t = np.full((n, n), 0.5)
    with pytest.raises(impop_amd.ImpopError) as ei:
        ctx.cluster_from_identity(t, AF_THR)
    assert "12798" in str(ei.value) and "12700" not in str(ei.value)
    assert ei.value.code == _lib.E_INVALID
    # the context is still good
    cl, K, sz = ctx.cluster_from_identity(np.array([[np.nan, 1.0], [np.nan, np.nan]]), AF_THR)
    assert K == 1 and cl.tolist() == [0, 0]


# ---- 2. AFS and site counts ----------------------------------------------------------------------------------------------

def _afs_matrix(rng, n, S):
    """all-zero, all-one and intermediate columns (the per-wave bins and the per-lane atomics of afs_kernel both fire)"""
    p = rng.beta(0.3, 1.5, size=S).astype(np.float32)
    m = (rng.random((n, S), dtype=np.float32) < p[None, :]).astype(np.uint8)
    kind = rng.random(S)
    m[:, kind < 0.3] = 0
    m[:, kind > 0.85] = 1
    return m


def _afs_windows(rng, S, n_short):
    long_ = [(0, S), (3, S - 5), (4097, 4097 + 4100), (700, 700), (64, 128), (63, 65), (1, 2), (S - 1, S), (S, S)]
    b = rng.integers(0, S - 70, n_short)
    short = [(int(x), int(x + l)) for x, l in zip(b, rng.integers(0, 70, n_short))]
    return long_, short


@pytest.mark.parametrize("n", (257, 465, 513, 1030, 4096, 16383))
def test_afs_and_site_counts_large_masks(ctx, n):
    """impop_afs == np.bincount of the column sums, impop_site_counts == the column sums.  Few long windows take several chunks per
    window and the atomic flush, many short ones a workgroup per window and the direct store; more than 255 haplotypes make the
    256-thread strides over the histogram take further trips.  At n = 16383 the masks of 12287, 12288 and 16383 haplotypes
    cross 48 KiB of LDS.  The short windows number 3000 up to n = 1030, 600 at n = 4096 and 250 at n = 16383 (their spectra
    would otherwise be 200 MB per call); every short window still has one chunk, hence a workgroup and a direct store of
    its own, whatever their number."""
    rng = np.random.default_rng(2000 + n)
    S = 64 * 160 + 7
    m = _afs_matrix(rng, n, S)
    bm = ctx.upload_dense(m, keep_hap_major=False)
    masks = [("all", None), ("60%", (rng.random(n) < 0.6).astype(np.uint8)), ("empty", np.zeros(n, np.uint8)), ("last", _flags([n - 1], n))]
    if n == 16383:
        masks += [("12287", _flags(np.arange(12287), n)), ("12288", _flags(np.arange(n - 12288, n), n))]
    long_, short = _afs_windows(rng, S, 3000 if n <= 1030 else 600 if n <= 4096 else 250)
    for name, mask in masks:
        cnt = pr.column_counts(m, mask)
        for wins in (long_, short):
            got = bm.afs([(a, b, 0) for a, b in wins], mask)
            want = pr.ref_afs(m, mask, wins, cnt)
            assert got.shape == want.shape, (n, name)
            bad = np.nonzero((got.astype(np.int64) != want).any(axis=1))[0]
            assert bad.size == 0, (n, name, len(wins), bad[:5].tolist())
        for s0, s1 in ((0, S), (5, 4099), (63, 65), (S - 70, S), (100, 100)):
            assert (bm.site_counts(s0, s1, mask).astype(np.int64) == pr.ref_site_counts(m, mask, s0, s1, cnt)).all(), (n, name, s0, s1)
    bm.free()


def test_afs_mask_of_16384_is_refused(ctx):
    import impop_amd
    n, S = 16385, 64
    m = np.zeros((n, S), np.uint8)
    m[::3, ::2] = 1
    bm = ctx.upload_dense(m, keep_hap_major=False)
    for mask in (_flags(np.arange(16384), n), None):
        with pytest.raises(impop_amd.ImpopError) as ei:
            bm.afs([(0, S, 0)], mask)
        assert "16383" in str(ei.value)
    mask = _flags(np.arange(2, 16385), n)  # 16383 haplotypes of a larger matrix are served
    assert (bm.afs([(0, S, 0)], mask).astype(np.int64) == pr.ref_afs(m, mask, [(0, S)])).all()
    bm.free()


def test_afs_more_windows_than_one_grid_holds(ctx):
    """70 000 windows in one call: windows ride on gridDim.y in batches of 65535"""
    rng = np.random.default_rng(2100)
    n, S, NW = 40, 3000, 70000
    m = _afs_matrix(rng, n, S)
    bm = ctx.upload_dense(m, keep_hap_major=False)
    b = rng.integers(0, S - 40, NW)
    wins = [(int(x), int(x + l)) for x, l in zip(b, rng.integers(1, 41, NW))]
    for mask in (None, (rng.random(n) < 0.6).astype(np.uint8)):
        got = bm.afs([(a, b_, 0) for a, b_ in wins], mask).astype(np.int64)
        want = pr.ref_afs(m, mask, wins)
        for w in (0, 65534, 65535, 65536, NW - 1):
            assert got[w].tolist() == want[w].tolist(), w
        assert (got == want).all()
    bm.free()


@pytest.mark.parametrize("n", (4096, 65535))
def test_site_counts_wide_rows(ctx, n):
    rng = np.random.default_rng(2200 + n)
    S = 64 * 8 + 11
    m = _afs_matrix(rng, n, S)
    m[[0, 31, 32, n - 2, n - 1], :] ^= (rng.random((5, S)) < 0.5).astype(np.uint8)
    bm = ctx.upload_dense(m, keep_hap_major=False)
    for mask in (None, (rng.random(n) < 0.6).astype(np.uint8), _flags([n - 1], n), _flags([0, n - 2], n)):
        for s0, s1 in ((0, S), (1, S - 1), (63, 130), (200, 201), (S - 11, S)):
            assert (bm.site_counts(s0, s1, mask).astype(np.int64) == pr.ref_site_counts(m, mask, s0, s1)).all(), (n, s0, s1)
    bm.free()


# ---- 3. EHH -----------------------------------------------------------------------------------------------------------------

EHH_W = (1, 63, 64, 65, 1024, 1025, 5000)


def _founders(rng, n, S, nf=7, pf=0.02, pp=0.0015):
    anc = rng.integers(0, 2, size=S, dtype=np.uint8)
    f = np.repeat(anc[None, :], nf, axis=0) ^ (rng.random((nf, S)) < pf).astype(np.uint8)
    return f[rng.integers(0, nf, size=n)] ^ (rng.random((n, S), dtype=np.float32) < pp).astype(np.uint8)


def _exactly(rng, n, k):
    return _flags(rng.choice(n, k, replace=False), n)


@pytest.mark.parametrize("n", (257, 465, 513, 1030, 4096))
def test_ehh_many_members(ctx, n):
    """exact list equality with the partition-refinement reference; 256 -> 257 members is gridDim.x 1 -> 2 of
    ehh_first_diff_kernel.  Every (members, direction, W) runs from an aligned and from an unaligned first site."""
    rng = np.random.default_rng(3000 + n)
    S = 5200
    m = _founders(rng, n, S)
    bm = ctx.upload_dense(m, keep_hap_major=False)
    members = [None, (rng.random(n) < 0.6).astype(np.uint8), _exactly(rng, n, 256), _exactly(rng, n, 257)]
    for mem in members:
        for rev in (False, True):
            for W in EHH_W:
                for s0 in (64, 37):
                    got = bm.ehh(s0, s0 + W, mem, rev).tolist()
                    assert got == pr.ref_ehh(m[:, s0:s0 + W], mem, rev), (n, None if mem is None else int(mem.sum()), rev, W, s0)
    bm.free()


def test_ehh_curves_that_never_or_at_once_reach_zero(ctx):
    """Two identical haplotypes keep one pair homozygous to the end (one pair of 513 haplotypes rounds to 0.000, so the curve
    is also taken over three members, where it ends at 0.333).  With 0/1 alleles at most two haplotypes can differ pairwise
    at one site, so "every pair differs at site 0" is the two-member case; its many-member analogue is a matrix whose rows
    are all distinct within the first ceil(log2 n) sites (the row index in binary), which takes the curve to 0 there."""
    rng = np.random.default_rng(3100)
    n, S = 513, 700
    m = (rng.random((n, S)) < 0.5).astype(np.uint8)
    m[400] = m[7]
    bm = ctx.upload_dense(m, keep_hap_major=False)
    for rev in (False, True):
        got = bm.ehh(3, 650, None, rev).tolist()
        assert got == pr.ref_ehh(m[:, 3:650], None, rev)
        mem = _flags([7, 400, 12], n)
        got = bm.ehh(3, 650, mem, rev).tolist()
        assert got == pr.ref_ehh(m[:, 3:650], mem, rev) and got[-1] == 0.333
    a, b = 7, int(np.nonzero(m[:, 70] != m[7, 70])[0][0])
    got = bm.ehh(70, 400, _flags([a, b], n)).tolist()
    assert got == [0.0] * 330 == pr.ref_ehh(m[:, 70:400], _flags([a, b], n))
    bm.free()
    m2 = ((np.arange(n)[:, None] >> np.arange(10)[None, :]) & 1).astype(np.uint8)
    m2 = np.concatenate([np.zeros((n, 5), np.uint8), m2, (rng.random((n, 100)) < 0.5).astype(np.uint8)], axis=1)
    bm = ctx.upload_dense(m2, keep_hap_major=False)
    got = bm.ehh(5, 115).tolist()
    assert got == pr.ref_ehh(m2[:, 5:115]) and got[9] == 0.0 and got[0] > 0.49
    got = bm.ehh(0, 115, None, True).tolist()
    assert got == pr.ref_ehh(m2, None, True)
    bm.free()


# ---- 4. scan and scan_multi above 4096 haplotypes ---------------------------------------------------------------------------------

def _masks_wide(n, seed, cfg):
    """P / A / B with the special haplotypes in P only, A only, B only, A and B (the overlap leaves both) or none; "last": A is
    exactly {n - 1}"""
    rng = np.random.default_rng(seed)
    P = (rng.random(n) < 0.6).astype(np.uint8)
    A = np.zeros(n, np.uint8); A[: n // 2] = 1
    B = np.zeros(n, np.uint8); B[n // 3:] = 1
    sp = _special(n)
    P[sp] = cfg == "P"
    A[sp] = cfg in ("A", "AB")
    B[sp] = cfg in ("B", "AB")
    if cfg == "last":
        A[:] = 0
        A[n - 1] = 1
        B[n - 1] = 0
    return P, A, B


def _check_records(oracle, recs, m, bits, wins, P, A, B, d_pi_mode, s_scope, where):
    n = m.shape[0]
    ints = pr.ref_scan_ints(m, P, A, B, wins)
    ov = A & B
    pk = oracle.pack_mask
    mP, mA, mB = pk(np.ones(n, np.uint8) if P is None else P), pk(A & ~ov), pk(B & ~ov)
    for wi, (w, r, want_i) in enumerate(zip(wins, recs, ints)):
        for k in INT_KEYS:
            assert int(r[k]) == want_i[k], (where, wi, w, k, int(r[k]), want_i[k])
        want = oracle.window_sitecount(bits, n, w[0], w[1], mP, mA, mB, w[2], d_pi_mode, s_scope)
        for k in DBL_KEYS:
            assert stat_close(k, float(r[k]), float(want[k]), float(want["dxy"])), (where, wi, w, k, float(r[k]), want[k])


def _truth(m):
    n = m.shape[0]
    c = m.sum(axis=0, dtype=np.int64)
    var = (c > 0) & (c < n)
    rare = var & (np.minimum(c, n - c) <= 3)
    return int(var.sum()), int(rare.sum()), int((var & ~rare).sum())


def _recover(value, pairs, W):
    """impop_scan_multi returns doubles only, so its integer sums are checked through them: for a window without seq_len
    value = sum / (pairs * W) in fp64, and every sum here is below 2^46, so rounding value * pairs * W to the nearest integer
    gives the sum back exactly.  (Windows with a seq_len are covered by the oracle's doubles alone.)  A population of one
    haplotype has pairs = 0: its within-sum is 0 by definition and the check reads 0 == 0; its between-sums are real."""
    return int(round(float(value) * pairs * W))


@pytest.mark.parametrize("n", (8191, 16385, 65535))
def test_scan_wide_matrices(ctx, oracle, n):
    """Above 4096 haplotypes: the three layouts return byte-identical records; every integer field of every window equals the
    column-sum reference; every double matches the oracle's site-count record.  At 65535 haplotype 65534 is one bit pattern
    away from the rare entries' 0xFFFF sentinel, and scan_multi with K = 8 asks for more than 48 KiB of LDS."""
    import impop_amd
    m = _crafted_wide(n, n)
    S = m.shape[1]
    bits = impop_amd.pack_hap_major(m)
    ms = [ctx.upload(bits, S, keep_hap_major=False, **kw) for kw in KINDS]
    kept, rare, common = _truth(m)
    info = {**ms[0].scan_index_info(), **ms[0].scan_split_info()}
    assert info["why"] == "" and (info["n_kept"], info["n_rare"], info["n_common"]) == (kept, rare, common), (n, info, kept, rare, common)
    assert info["rare_bytes"] == 8 * rare and rare > 60 and common > 30
    i1 = {**ms[1].scan_index_info(), **ms[1].scan_split_info()}
    assert i1["n_kept"] == kept and i1["n_rare"] == 0
    assert ms[2].scan_index_info()["n_kept"] == 0
    wins = _scan_windows(S)

    def three(fn, where):
        out = [np.asarray(fn(x)) for x in ms]
        for o in out[1:]:
            assert o.dtype == out[0].dtype and o.shape == out[0].shape and o.tobytes() == out[0].tobytes(), (n, where)
        return out[0]

    for cfg in ("P", "A", "B", "AB", "none", "last"):
        P, A, B = _masks_wide(n, n + 1, cfg)
        recs = three(lambda x: x.scan(wins, P, A, B), cfg)
        _check_records(oracle, recs, m, bits, wins, P, A, B, 0, 0, (n, cfg))
    P, A, B = _masks_wide(n, n + 2, "B")
    recs = three(lambda x: x.scan(wins, None, A, B), "P=None")
    _check_records(oracle, recs, m, bits, wins, None, A, B, 0, 0, (n, "P=None"))
    few = wins[:3] + wins[8:14]
    for d_pi_mode in (0, 1, 2):
        for s_scope in (0, 1):
            recs = three(lambda x: x.scan(few, P, A, B, d_pi_mode, s_scope), (d_pi_mode, s_scope))
            _check_records(oracle, recs, m, bits, few, P, A, B, d_pi_mode, s_scope, (n, "modes", d_pi_mode, s_scope))

    # K disjoint populations in one pass
    mw = [(300, 900, 0), (5, 300, 0), (2200, S - 3, 12345), (63, 65, 0), (900, 900, 0), (0, 60, 0)]
    ones = oracle.pack_mask(np.ones(n, np.uint8))
    for K in (2, 5, 8):
        owner = np.arange(n) % (K + 1)  # K = in no population
        rng = np.random.default_rng(n + K)
        owner = owner[rng.permutation(n)]
        owner[_special(n)] = [0, K - 1, K, 1 % K, K - 1]
        if K == 5:  # one population that is exactly {n - 1}
            owner[owner == 4] = K
            owner[n - 1] = 4
        pops = [(owner == k).astype(np.uint8) for k in range(K)]
        got = three(lambda x: x.scan_multi(mw, pops), ("multi", K))
        assert got.shape == (len(mw), K * (K - 1) // 2)
        within, between, nk = pr.ref_multi_ints(m, pops, [(a, b) for a, b, _ in mw])
        p = 0
        for k in range(K):
            for l in range(k + 1, K):
                pa, pb = nk[k] * (nk[k] - 1) / 2, nk[l] * (nk[l] - 1) / 2
                for wi, (s0, s1, sl) in enumerate(mw):
                    r = got[wi, p]
                    if sl == 0 and s1 > s0:
                        W = s1 - s0
                        assert _recover(r["pi_a"], pa, W) == int(within[wi, k]), (n, K, k, l, wi)
                        assert _recover(r["pi_b"], pb, W) == int(within[wi, l]), (n, K, k, l, wi)
                        assert _recover(r["dxy"], int(nk[k]) * int(nk[l]), W) == int(between[wi, p]), (n, K, k, l, wi)
                    want = oracle.window_sitecount(bits, n, s0, s1, ones, oracle.pack_mask(pops[k]), oracle.pack_mask(pops[l]), sl)
                    for key in PAIR_KEYS:
                        assert stat_close(key, float(r[key]), want[key], want["dxy"]), (n, K, k, l, wi, key, float(r[key]), want[key])
                p += 1
    for x in ms:
        x.free()


def test_scan_refuses_65536_haplotypes(ctx):
    import impop_amd
    n, S = 65536, 64
    m = np.zeros((n, S), np.uint8)
    m[[0, 31, n - 1], 3] = 1
    m[::2, 9] = 1
    bm = ctx.upload_dense(m, keep_hap_major=False)
    with pytest.raises(impop_amd.ImpopError) as ei:
        bm.scan([(0, S, 0)], None, _flags([0, 1], n), _flags([2, 3], n))
    assert "65535" in str(ei.value)
    with pytest.raises(impop_amd.ImpopError) as ei:
        bm.scan_multi([(0, S, 0)], [_flags([0, 1], n), _flags([2, 3], n)])
    assert "65535" in str(ei.value)
    info = bm.scan_split_info()
    assert info["n_rare"] == 0 and "n_hap > 65535" in info["why"]
    assert (bm.site_counts(0, S).astype(np.int64) == pr.ref_site_counts(m, None, 0, S)).all()  # what has no limit still serves it
    bm.free()


def test_scan_saturated_lane_accumulators(ctx, oracle):
    """n = 512, the top of the fixed-WPS kernel and of scan_multi's 32-bit path: every site has c = 256 with A = the carriers and
    B = the rest, so every per-site product is at its maximum 2^16; one window of 4096 * 64 sites scanned with tile_blocks =
    4096 gives a lane 1024 sites of one tile: 1024 * 2^16 = 2^26 per 32-bit accumulator, the documented worst case of the scan.
    impop_scan_multi takes no tile size: it runs the same matrix under its default tiling (at most 4096 blocks, the bound of
    its 32-bit path), so its sums are pinned at whatever tile the library chooses, not at a forced one.  Pins the margin
    against later tile-size changes."""
    import impop_amd
    n, S = 512, 4096 * 64
    m = np.zeros((n, S), np.uint8)
    m[:256] = 1
    A, B = _flags(np.arange(256), n), _flags(np.arange(256, 512), n)
    bits = impop_amd.pack_hap_major(m)
    bm = ctx.upload(bits, S, keep_hap_major=False)
    wins = [(0, S, 0), (0, S, S), (64, S - 64, 0)]
    recs = bm.scan(wins, None, A, B, tile_blocks=4096)
    assert int(recs[0]["sum_p"]) == S << 16 == int(recs[0]["sum_ab"]) and int(recs[0]["s_all"]) == S and int(recs[0]["sum_a"]) == 0
    _check_records(oracle, recs, m, bits, wins, None, A, B, 0, 0, "saturated")
    recs = bm.scan(wins, B, B, A)
    _check_records(oracle, recs, m, bits, wins, B, B, A, 0, 0, "saturated default tiles")
    got = bm.scan_multi(wins, [A, B])
    within, between, nk = pr.ref_multi_ints(m, [A, B], [(a, b) for a, b, _ in wins])
    for wi, (s0, s1, sl) in enumerate(wins):
        if sl == 0:
            assert _recover(got[wi, 0]["dxy"], 256 * 256, s1 - s0) == int(between[wi, 0]) == (s1 - s0) << 16
            assert _recover(got[wi, 0]["pi_a"], 256 * 255 / 2, s1 - s0) == int(within[wi, 0]) == 0
        want = oracle.window_sitecount(bits, n, s0, s1, oracle.pack_mask(np.ones(n, np.uint8)), oracle.pack_mask(A), oracle.pack_mask(B), sl)
        for key in PAIR_KEYS:
            assert stat_close(key, float(got[wi, 0][key]), want[key], want["dxy"]), (wi, key)
    # mixed populations: both orders of the between-population product are non-zero at every site
    A2, B2 = _flags(np.arange(128, 384), n), _flags(np.r_[0:128, 384:512], n)
    got = bm.scan_multi(wins, [A2, B2])
    within, between, nk = pr.ref_multi_ints(m, [A2, B2], [(a, b) for a, b, _ in wins])
    assert _recover(got[0, 0]["dxy"], 256 * 256, S) == int(between[0, 0]) == S * 2 * 128 * 128
    assert _recover(got[0, 0]["pi_a"], 256 * 255 / 2, S) == int(within[0, 0]) == S * 128 * 128
    bm.free()


# ---- 5. Gram at the polarity boundary ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (16384, 16385))
def test_pairwise_counts_at_the_polarity_boundary(ctx, oracle, n):
    """n = 16384 is the last size whose Gram operand is stored by minor allele (16384 % 96 != 0: the phi row is there), 16385 the
    first without.  Mostly-ones columns make sure sites really are flipped.  The n x n counts must be symmetric, carry the
    per-haplotype counts on the diagonal, and equal an int64 product of the unpacked bits on 64 rows: the first and last row,
    the rows on both sides of the first and the last 96-row tile edge, and random ones."""
    rng = np.random.default_rng(5000 + n)
    S, s0, s1 = 2100, 37, 2085
    p = np.where(rng.random(S) < 0.5, rng.beta(0.3, 3.0, S), 1 - rng.beta(0.3, 3.0, S)).astype(np.float32)
    m = (rng.random((n, S), dtype=np.float32) < p[None, :]).astype(np.uint8)
    m[:, rng.random(S) < 0.05] = 1
    m[[0, 95, 96, n - 2, n - 1], :] ^= (rng.random((5, S)) < 0.3).astype(np.uint8)
    bm = ctx.upload_dense(m, keep_hap_major=True)
    I = bm.pairwise_counts(s0, s1)
    w = m[:, s0:s1].astype(np.int64)
    assert (np.diagonal(I).astype(np.int64) == w.sum(axis=1)).all()
    last_edge = (n - 1) // 96 * 96
    rows = sorted({0, 95, 96, last_edge - 1, last_edge, n - 1} | set(rng.choice(n, 64, replace=False).tolist()[:58]))
    rows = rows[:64] if len(rows) > 64 else rows
    assert {0, 95, 96, last_edge - 1, last_edge, n - 1} <= set(rows) and len(rows) <= 64
    want = w[rows] @ w.T
    assert (I[rows].astype(np.int64) == want).all()
    del want, w
    for lo in range(0, n, 2048):  # symmetry, a band of rows at a time
        assert (I[lo:lo + 2048] == I[:, lo:lo + 2048].T).all(), lo
    del I
    if n == 16384:
        # the windowed all-pairs statistics on top of the same operand (S and Tajima's D switched off): at threshold 1 every
        # haplotype is its own group, so pi and the Fst fields are those of the streaming scan
        P = _flags(np.r_[rng.choice(n - 1, 2999, replace=False), n - 1], n)
        A = _flags(np.arange(0, 1500), n)
        B = _flags(np.arange(n - 1500, n), n)
        wins = [(0, 300, 300), (37, 700, 0), (1024, 2085, 5000)]
        got = bm.pairwise_scan(wins, P, A, B, threshold=1.0, s_scope=2)
        ref = bm.scan(wins, P, A, B)
        # the streaming scan is the go-between, so it is pinned first: integers to the column sums, doubles to the oracle
        _check_records(oracle, ref, m, oracle.pack_hap_major(m), wins, P, A, B, 0, 0, "scan at 16384")
        for wi in range(len(wins)):
            assert int(got[wi]["n_sites"]) == wins[wi][1] - wins[wi][0] and int(got[wi]["n_groups"]) <= 3000
            for k in ("pi", "pi_site", "pi_a", "pi_b", "pi_xy", "dxy", "da", "fst"):
                assert stat_close(k, float(got[wi][k]), float(ref[wi][k]), float(ref[wi]["dxy"])), (wi, k, float(got[wi][k]), float(ref[wi][k]))
            assert math.isnan(float(got[wi]["tajima_d"])) and int(got[wi]["s_all"]) == 0
    bm.free()


# ---- 6. impop_pica2_pair_terms ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (1023, 4096))
def test_pica2_pair_terms(ctx, n):
    """sims is a rounded copy of the table: bit-exact.  values is (1 - sim) * f_g * f_h in the reference's operation order
    (pica2.py:137-139), which the kernel follows, and fp64 division and multiplication are correctly rounded on both sides
    (the library is built without contraction): bit-exact as well."""
    import impop_amd
    rng = np.random.default_rng(6000 + n)
    t = 0.97 + 0.03 * rng.random((n, n))
    t = np.minimum(t, t.T)
    hole = rng.random((n, n)) < 0.015
    t[hole | hole.T] = np.nan
    for G in (2, 3, 257, 1000):
        rep = np.sort(rng.choice(n, G, replace=False)).astype(np.uint32)
        if G == 3:
            rep = rep[[2, 0, 1]]  # not in index order: the pair is still keyed (smaller, larger)
        t[rep[0], rep[1]] = t[rep[1], rep[0]] = np.nan  # a representative pair without data
        size = rng.integers(1, 9, G).astype(np.uint32)  # sums to something other than n
        size[0] += int(size.sum()) == n
        assert int(size.sum()) != n
        for rd in (None, 4, 5):
            sims, vals = ctx.pica2_pair_terms(t, rd, rep, size)
            ws, wv = pr.ref_pair_terms(t, rd, rep, size)
            assert np.isnan(sims[0]) and np.isnan(vals[0])
            assert sims.tobytes() == ws.tobytes() or (np.isnan(sims) == np.isnan(ws)).all() and (sims[~np.isnan(ws)] == ws[~np.isnan(ws)]).all(), (n, G, rd)
            ok = ~np.isnan(wv)
            assert (np.isnan(vals) == ~ok).all()
            worst = np.max(np.abs(vals[ok] - wv[ok]) / np.maximum(np.abs(wv[ok]), 1e-300)) if ok.any() else 0.0  # G = 2: the one pair is absent
            print(f"pair_terms n={n} G={G} round={rd}: worst relative difference of values {worst:.3e}")
            assert (vals[ok] == wv[ok]).all(), (n, G, rd, worst)
    # as the header says: an out-of-range representative is an error, fewer than two groups is nothing to do
    with pytest.raises(impop_amd.ImpopError):
        ctx.pica2_pair_terms(t, None, np.array([0, n], np.uint32), np.array([1, 1], np.uint32))
    for G in (0, 1):
        sims, vals = ctx.pica2_pair_terms(t, None, np.arange(G, dtype=np.uint32), np.ones(G, np.uint32))
        assert len(sims) == 0 and len(vals) == 0
