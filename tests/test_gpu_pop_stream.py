"""GPU: the streaming pass that impop_scan_multi and impop_dstat_scan share (csrc/pop_stream.h), both calls on the same matrices
at the haplotype counts where the pass changes path: a tail only, no tail, the top of the two-blocks-in-flight loop (and of
scan_multi's 32-bit accumulators), the first count beyond it, batches of four granules and one, two full batches with a tail.
The sites are those of dstat_cases.draw_sites, thinned: draw_sites leaves half of them variable and the variable-site index is
built only where at most a quarter vary, so six in ten columns are made monomorphic again and every matrix has its index and its
rare stream (asserted; 33 haplotypes have the index alone).  Every device value is an exact integer: the references are the plain
restatements of plain_dstat.py and plain_refs.py, and nothing is compared with a tolerance."""
import functools

import numpy as np
import pytest

import dstat_cases as dc
import plain_dstat as pd
import plain_refs as pr

pytestmark = pytest.mark.gpu

N_SITE = 4200
# n -> (G, r, Gf): granules per site, dwords of the last one, full granules (internal.h, sb64.h)
SHAPES = {33: (1, 2, 0), 128: (1, 4, 1), 465: (4, 3, 3), 512: (4, 4, 4), 513: (5, 1, 4), 641: (6, 1, 5), 1100: (9, 3, 8)}
# dstat_cases.GEOMETRY_WINDOWS with its long windows scaled from 2100 to 4200 sites, one window of a single block, and one of
# 12 blocks: three per wave, an odd number for the loop that takes two at a time
WINDOWS = [(0, 64), (1, 65), (63, 129), (0, N_SITE), (1400, 2800), (N_SITE - 64, N_SITE), (5, 6), (128, 192), (256, 1024)]
MULTI_K = (2, 5, 8)
ROUTES = ({}, {"rare_split": False}, {"dense_scan": True})  # indexed+rare, indexed, dense; the compacted matrix comes from the first
PAIR_KEYS = ("fst", "pi_a", "pi_b", "pi_xy", "dxy", "da")


def geometry(n):
    wps = (n + 31) // 32
    G = (wps + 3) // 4
    r = wps - 4 * (G - 1)
    return G, r, G if r == 4 else G - 1


def flags(members, n):
    f = np.zeros(n, dtype=np.uint8)
    f[list(members)] = 1
    return f


def multi_pops(n, K):
    """K disjoint cuts of a permutation, one haplotype in no population"""
    perm = np.random.default_rng(1400 + 10 * n + K).permutation(n)
    cuts = np.linspace(0, n - 1, K + 1).astype(int)
    return [flags(perm[cuts[k]:cuts[k + 1]], n) for k in range(K)]


def multi_records(m01, pops, windows):
    """impop_pair_stats of every window and pair from the exact sums of plain_refs.ref_multi_ints, in the operation order of
    hudson_fst (csrc/scan.hip) for windows without a seq_len: the same IEEE doubles, so the records are compared bit for bit."""
    within, between, nk = pr.ref_multi_ints(m01, pops, windows)
    K = len(pops)
    out = np.zeros((len(windows), K * (K - 1) // 2), dtype=[(k, "<f8") for k in PAIR_KEYS])
    for wi, (s0, s1) in enumerate(windows):
        W, p = float(s1 - s0), 0
        for k in range(K):
            for l in range(k + 1, K):
                nA, nB = float(nk[k]), float(nk[l])
                pi_a = float(within[wi, k]) / (nA * (nA - 1.0) / 2.0 * W) if nk[k] >= 2 else 0.0
                pi_b = float(within[wi, l]) / (nB * (nB - 1.0) / 2.0 * W) if nk[l] >= 2 else 0.0
                dxy = float(between[wi, p]) / (nA * nB * W)
                pi_xy = 0.5 * (pi_a + pi_b)
                out[wi, p] = ((dxy - pi_xy) / dxy if dxy > 0 else 0.0, pi_a, pi_b, pi_xy, dxy, dxy - pi_xy)
                p += 1
    return out, within, between, nk


def recover(value, pairs, W):
    """the integer sum behind value = sum / (pairs * W): every sum here is below 2^46 (test_gpu_upper_range._recover), so
    rounding value * pairs * W to the nearest integer gives it back exactly"""
    return int(round(float(value) * pairs * W))


@functools.lru_cache(maxsize=None)
def case(n):
    """the matrix, dstat's four populations, weights for the weighted twin: computed once, never modified"""
    rng = np.random.default_rng(14000 + n)
    m01 = dc.draw_sites(rng, n, N_SITE)
    mono = rng.random(N_SITE) < 0.6
    m01[:, mono] = rng.integers(0, 2, int(mono.sum()), dtype=np.uint8)[None, :]
    c = m01.sum(axis=0, dtype=np.int64)
    assert 4 * int(((c > 0) & (c < n)).sum()) <= N_SITE  # few enough variable sites for the index (IMPOP_INDEX_MAX_KEPT_INV)
    pops = dc.cut_pops(rng, n)
    w = rng.integers(1, 4, N_SITE).astype(np.uint32)
    m01.setflags(write=False)
    w.setflags(write=False)
    return m01, pops, w


def dstat_want(n, polarize, weights=None):
    m01, pops, _ = case(n)
    want = pd.reference(m01, pops, dc.GEOMETRY_QUARTETS, WINDOWS, polarize, weights=weights)
    dc.assert_not_hollow(want)
    return want


def multi_want(n, K):
    m01, _, _ = case(n)
    want, within, between, nk = multi_records(m01, multi_pops(n, K), WINDOWS)
    live = (between > 0).any(axis=1)  # not hollow: some non-zero dxy in at least two thirds of the windows
    assert 3 * int(live.sum()) >= 2 * live.size, (n, K, int(live.sum()))
    return want, within, between, nk


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=sorted(SHAPES))
def mats(ctx, request):
    """one shape: the matrix on its three routes, compacted, weighted, and the bp-expanded twin of the weighted one"""
    n = request.param
    assert geometry(n) == SHAPES[n]
    m01, _, w = case(n)
    ms = [ctx.upload_dense(m01, keep_hap_major=False, **kw) for kw in ROUTES]
    index, split = ms[0].scan_index_info(), ms[0].scan_split_info()
    assert index["why"] == "" and index["n_kept"] > 0, index
    if n > 64:  # up to 64 haplotypes a row is no wider than a rare entry: an index without the split
        assert split["why"] == "" and split["n_rare"] > 0 and split["n_common"] > 0, split
    ms.append(ms[0].compact())
    weighted = ctx.upload_dense(m01, keep_hap_major=False)
    weighted.set_site_weights(w)
    expanded = ctx.upload_dense(np.repeat(m01, w, axis=1), keep_hap_major=False)
    yield n, ms, weighted, expanded
    for x in ms + [weighted, expanded]:
        x.free()


def expanded_windows(w):
    start = np.concatenate([[0], np.cumsum(w.astype(np.int64))])
    return [(int(start[b]), int(start[e])) for b, e in WINDOWS]


@pytest.mark.parametrize("polarize", (False, True))
def test_dstat_scan(mats, polarize):
    n, ms, weighted, expanded = mats
    _, pops, w = case(n)
    mk = [flags(p, n) for p in pops]
    want = dstat_want(n, polarize)
    got = [x.dstat_scan(WINDOWS, mk, dc.GEOMETRY_QUARTETS, polarize=polarize) for x in ms]
    pd.assert_matches(got[0], want, (n, polarize))
    for tag, g in zip(("indexed", "dense", "compact"), got[1:]):
        assert g.tobytes() == got[0].tobytes(), (n, polarize, tag)
    # weights: the sums of the bp-expanded matrix, the two counters those of the columns
    gw = weighted.dstat_scan(WINDOWS, mk, dc.GEOMETRY_QUARTETS, polarize=polarize)
    pd.assert_matches(gw, dstat_want(n, polarize, w), (n, polarize, "weighted"))
    gx = expanded.dstat_scan(expanded_windows(w), mk, dc.GEOMETRY_QUARTETS, polarize=polarize)
    pd.assert_matches(gw, gx, (n, polarize, "expanded"), skip=("n_informative", "n_skipped"))


@pytest.mark.parametrize("K", MULTI_K)
def test_scan_multi(mats, K):
    n, ms, weighted, expanded = mats
    _, _, w = case(n)
    pops = multi_pops(n, K)
    want, within, between, nk = multi_want(n, K)
    wins = [(a, b, 0) for a, b in WINDOWS]
    got = [np.asarray(x.scan_multi(wins, pops)) for x in ms]
    assert got[0].shape == want.shape
    p = 0
    for k in range(K):
        for l in range(k + 1, K):
            pa, pb = int(nk[k] * (nk[k] - 1) // 2), int(nk[l] * (nk[l] - 1) // 2)
            for wi, (s0, s1) in enumerate(WINDOWS):
                r = got[0][wi, p]
                assert recover(r["pi_a"], pa, s1 - s0) == int(within[wi, k]), (n, K, k, l, wi)
                assert recover(r["pi_b"], pb, s1 - s0) == int(within[wi, l]), (n, K, k, l, wi)
                assert recover(r["dxy"], int(nk[k]) * int(nk[l]), s1 - s0) == int(between[wi, p]), (n, K, k, l, wi)
            p += 1
    for key in PAIR_KEYS:
        assert pd.bits_equal(got[0][key], want[key]).all(), (n, K, key)
    for tag, g in zip(("indexed", "dense", "compact"), got[1:]):
        assert g.tobytes() == got[0].tobytes(), (n, K, tag)
    # weights: exactly the records of the bp-expanded matrix (the same integer sums over the same W)
    gw = np.asarray(weighted.scan_multi(wins, pops))
    gx = np.asarray(expanded.scan_multi([(a, b, 0) for a, b in expanded_windows(w)], pops))
    assert gw.tobytes() == gx.tobytes(), (n, K, "expanded")
    wsum = np.concatenate([[0], np.cumsum(w.astype(np.int64))])
    cols = [np.asarray(case(n)[0])[f.astype(bool)].sum(axis=0, dtype=np.int64) for f in pops]
    for wi, (s0, s1) in enumerate(WINDOWS):  # ... and those are the weighted sums of the restatement
        W = int(wsum[s1] - wsum[s0])
        c0, c1 = cols[0][s0:s1], cols[1][s0:s1]
        cross = int((w[s0:s1].astype(np.int64) * (c0 * (int(nk[1]) - c1) + c1 * (int(nk[0]) - c0))).sum())
        assert recover(gw[wi, 0]["dxy"], int(nk[0]) * int(nk[1]), W) == cross, (n, K, wi)
