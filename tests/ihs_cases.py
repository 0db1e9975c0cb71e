"""Shared cases of the impop_ihs_scan tests: founder mosaics with recombination points and about 1 % mutations, which give real
long matches, and stretches of sites that are monomorphic; each with the survival tables of the plain restatement
(tests/plain_ihs.py) computed once.  The geometry cases are chosen so that the restatement's own output exercises the cutoff, the
range edge and the limits (assert_coverage)."""
import functools

import numpy as np

import plain_ihs as pi

# the header's known answer
KNOWN_ROWS = ["1011010", "1011000", "0011010", "0100110", "0101110", "1101100"]
KNOWN_PARAMS = dict(min_mac=3, cutoff_milli=300)
KNOWN_LIMITS = dict(max_bp=2, max_sites=1)
KNOWN_SITES = [0, 1, 2, 4]
KNOWN_HEAD = [((3, 3), (0, 3))] * 4   # n, c1
KNOWN_FLAGS = [85, 119, 221, 187]
KNOWN_I2 = [[[0, 6], [0, 10]], [[4, 22], [4, 12]], [[10, 6], [10, 16]], [[22, 4], [8, 4]]]  # ihh2 = sl2: unit spacing
KNOWN_LIMIT_FLAGS = [43605, 43605, 64005, 21930]
KNOWN_LIMIT_IHH2 = [[[0, 6], [0, 6]], [[4, 12], [4, 10]], [[10, 6], [10, 12]], [[12, 4], [6, 4]]]
KNOWN_LIMIT_SL2 = [[[0, 4], [0, 4]], [[4, 6], [4, 6]], [[6, 4], [6, 6]], [[6, 4], [4, 4]]]


def known_matrix():
    return np.array([[int(c) for c in r] for r in KNOWN_ROWS], dtype=np.uint8)


def mosaic(rng, n, S, nf=6, p_switch=0.02, p_mut=0.01, p_mono=0.35):
    """n rows over S sites: each row copies one of nf random founders and switches founder with probability p_switch per site
    (a recombination point); about p_mut of the entries are flipped; p_mono of the sites are made monomorphic (all 0 or all 1),
    in stretches"""
    founders = (rng.random((nf, S)) < 0.5).astype(np.uint8)
    m01 = np.empty((n, S), dtype=np.uint8)
    for i in range(n):
        switch = rng.random(S) < p_switch
        switch[0] = True
        src = rng.integers(0, nf, size=S)
        who = src[np.maximum.accumulate(np.where(switch, np.arange(S), 0))]
        m01[i] = founders[who, np.arange(S)]
    m01 ^= (rng.random((n, S)) < p_mut).astype(np.uint8)
    s = 0
    while s < S:  # stretches of 1..12 sites, monomorphic with probability p_mono
        ln = int(rng.integers(1, 13))
        if rng.random() < p_mono:
            m01[:, s:s + ln] = int(rng.random() < 0.3)
        s += ln
    return m01


GEO_S, GEO_RANGE, GEO_CORES = 330, (7, 323), (9, 320)   # 6 blocks; every edge off the 64-site boundaries
GEO_N = (2, 33, 64, 65, 70, 130)
# (min_mac, cutoff_milli, (max_bp, max_sites)): every value the scan's paths depend on at least once
GEO_PARAMS = [(1, 50, (0, 0)), (2, 250, (37, 5)), (5, 1000, (1000, 0)), (1, 0, (37, 5)), (2, 50, (1000, 0)), (1, 50, (37, 5)), (5, 250, (0, 0))]
GEO_CHUNKS = (1, 2, 5, None)


@functools.lru_cache(maxsize=None)
def geometry_matrix(n):
    rng = np.random.default_rng(21000 + n)
    m01 = mosaic(rng, n, GEO_S, nf=5 if n > 4 else 2, p_switch=0.015, p_mut=0.01)
    m01.setflags(write=False)
    return m01


def geometry_pops(n, K):
    if K == 1:
        return [None]
    a = np.zeros(n, bool)
    a[np.random.default_rng(21500 + n).permutation(n)[:max(n // 2, 1)]] = True
    return [a, ~a]


@functools.lru_cache(maxsize=None)
def geometry_tables(n, K):
    return pi.survivors(geometry_matrix(n), GEO_RANGE[0], GEO_RANGE[1], geometry_pops(n, K))


@functools.lru_cache(maxsize=None)
def geometry_want(n, K, min_mac, cutoff, limits):
    r = pi.records(geometry_tables(n, K), GEO_CORES[0], GEO_CORES[1], min_mac=min_mac, cutoff_milli=cutoff, max_bp=limits[0],
                   max_sites=limits[1])
    r.setflags(write=False)  # shared among tests: computed once, never changed
    return r


def bp_shares(rec):
    """of the (core, class, half) base-pair integrals of classes with a pair: the shares with neither bit, with EDGE, with LIMIT"""
    tot = free = edge = limit = 0
    for r in rec:
        for g in range(2):
            if r["n"][g] < 2:
                continue
            for h in range(2):
                tot += 1
                e = bool(int(r["flags"]) & pi.flag_bit(False, 0, g, h))
                l = bool(int(r["flags"]) & pi.flag_bit(True, 0, g, h))
                edge, limit, free = edge + e, limit + l, free + (not e and not l)
    tot = max(tot, 1)
    return free / tot, edge / tot, limit / tot


def assert_coverage(n, K):
    """a run where every integral hits the range edge would hide the cutoff and limit paths"""
    free, edge, _ = bp_shares(geometry_want(n, K, 1, 50, (0, 0)))
    assert free >= 0.25 and edge >= 0.05, (n, K, free, edge)
    _, _, limit = bp_shares(geometry_want(n, K, 1, 50, (37, 5)))
    assert limit >= 0.05, (n, K, limit)
