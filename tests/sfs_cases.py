"""Inputs of the impop_sfs_scan tests: the header's known answer with its literal results, the geometry generator with its planted
fixed differences and outgroup ties, population cuts, and the condition that keeps a case from being hollow."""
import numpy as np

import dstat_cases as dc

# the header's case: A = {0..4}, B = {5..9}, O = {10, 11}; the carriers of a population are its lowest-numbered members
KNOWN_COUNTS = [(1, 0, 0), (2, 1, 0), (5, 0, 0), (0, 4, 0), (1, 1, 1), (3, 5, 2), (0, 0, 0), (5, 5, 2), (0, 0, 1), (4, 2, 0), (0, 5, 2)]
KNOWN_POPS = [[0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 11]]
KNOWN_PAIRS = [(0, 1)]
KNOWN_WINDOW = (0, 11)
INT_FIELDS = ("seg", "eta1", "eta_n1", "sum_het", "sum_c", "sum_c2")
PAIR_FIELDS = ("private_a", "private_b", "shared", "fixed_a", "fixed_b", "n_union")
# outgroup (None or 2) -> per population (seg, eta1, eta_n1, sum_het, sum_c, sum_c2)
KNOWN_INTS = {
    None: [(5, 2, 1, 24, 11, 31), (4, 2, 1, 18, 8, 22), (2, 2, 2, 2, 2, 2)],
    2: [(4, 1, 1, 20, 9, 25), (3, 1, 1, 14, 7, 21), (0, 0, 0, 0, 0, 0)],
}
KNOWN_SKIPPED = {None: 0, 2: 2}
KNOWN_PAIR = {None: (2, 1, 3, 1, 1, 8), 2: (2, 1, 2, 2, 0, 7)}
KNOWN_CELLS = {  # (c_A, c_B) -> sites
    None: {(0, 4): 1, (0, 5): 1, (1, 0): 1, (1, 1): 1, (2, 1): 1, (3, 5): 1, (4, 2): 1, (5, 0): 1},
    2: {(0, 4): 1, (1, 0): 1, (2, 0): 1, (2, 1): 1, (4, 2): 1, (5, 0): 2},
}
# (outgroup, population, field) -> the header's digits, good to 1e-8
KNOWN_DIGITS = {
    (None, 0, "theta_pi"): 2.4, (None, 0, "theta_h"): 3.1, (None, 0, "theta_l"): 2.75, (None, 0, "faywu_h"): -0.7,
    (None, 1, "theta_w"): 1.92, (None, 1, "theta_pi"): 1.8, (None, 1, "tajima_d"): -0.41017465,
    (None, 1, "faywu_h_norm"): -0.34892049, (None, 1, "zeng_e"): 0.13767880,
    (2, 0, "tajima_d"): 0.27344977, (2, 0, "faywu_h"): -0.5, (2, 0, "faywu_h_norm"): -0.43615061, (2, 0, "zeng_e"): 0.56792505,
}

GEOMETRY_N = (12, 33, 64, 65, 70, 130, 465)
GEOMETRY_SITES = dc.GEOMETRY_SITES
GEOMETRY_WINDOWS = dc.GEOMETRY_WINDOWS
GEOMETRY_PAIRS = [(0, 1), (1, 0), (0, 2)]
GEOMETRY_OUTGROUP = 3
PLANT_RANGE = (700, 1400)
PLANTED = 8  # sites of each planted kind


def known_matrix():
    m = np.zeros((12, len(KNOWN_COUNTS)), dtype=np.uint8)
    for s, counts in enumerate(KNOWN_COUNTS):
        for k, c in enumerate(counts):
            lo = KNOWN_POPS[k][0]
            m[lo:lo + c, s] = 1
    return m


def cut_pops(rng, n):
    """from a permutation: n//4, n//3, the rest, and an EVEN outgroup of 2 max(1, n//16) (an odd one never ties); one haplotype is
    left out.  -> [P0, P1, P2, O]"""
    perm = [int(x) for x in rng.permutation(n)]
    a, b, o = n // 4, n // 3, 2 * max(1, n // 16)
    return [sorted(perm[:a]), sorted(perm[a:a + b]), sorted(perm[a + b:n - 1 - o]), sorted(perm[n - 1 - o:n - 1])]


def plant(rng, m, pops, lo, hi):
    """inside sites [lo, hi): PLANTED sites fixed in population 0 and absent in 1, PLANTED the other way round (the outgroup all 0:
    neither flipped nor a tie), and PLANTED outgroup ties.  Random sites never give a fixed difference at n >= 33."""
    sites = [int(s) for s in rng.choice(np.arange(lo, hi), size=3 * PLANTED, replace=False)]
    p0, p1, og = pops[0], pops[1], pops[3]
    for i, s in enumerate(sites):
        if i < 2 * PLANTED:
            m[p0, s] = 1 if i < PLANTED else 0
            m[p1, s] = 0 if i < PLANTED else 1
            m[og, s] = 0
        else:
            m[og, s] = 0
            m[og[:len(og) // 2], s] = 1
    return sites


def geometry_case(n):
    rng = np.random.default_rng(12000 + n)
    m = dc.draw_sites(rng, n, GEOMETRY_SITES)
    pops = cut_pops(rng, n)
    plant(rng, m, pops, *PLANT_RANGE)
    return m, pops


def crafted_case(n):
    """dstat_cases.crafted (rare-only, common-only, monomorphic and mixed stretches: every route has work) with this module's
    populations and plants in its mixed stretch"""
    m, wins = dc.crafted(n)
    rng = np.random.default_rng(177 + n)
    pops = cut_pops(rng, n)
    plant(rng, m, pops, 3000, 4000)
    return m, wins, pops


def eight_pops(rng, n):
    """eight disjoint populations (one haplotype left out) and all 28 pairs of them, the last population the outgroup"""
    perm = [int(x) for x in rng.permutation(n)]
    cuts = np.linspace(0, n - 1, 9).astype(int)
    pops = [sorted(perm[cuts[i]:cuts[i + 1]]) for i in range(8)]
    if len(pops[7]) % 2:  # an even outgroup
        pops[7] = pops[7][:-1]
    pairs = [(a, b) for a in range(8) for b in range(a + 1, 8)]
    return pops, pairs


def assert_known(result, outgroup):
    """the header's literal integers, cells and digits in a (stats, pair records, sfs, jsfs) result for the known case"""
    stats, prec, sfs, jsfs = result
    assert stats.shape == (1, 3) and prec.shape == (1, 1)
    for k in range(3):
        r = stats[0, k]
        assert tuple(int(r[f]) for f in INT_FIELDS) == KNOWN_INTS[outgroup][k], (outgroup, k)
        assert int(r["n_sites"]) == 11 and int(r["n_skipped"]) == KNOWN_SKIPPED[outgroup] and int(r["flags"]) == 0
    assert tuple(int(prec[0, 0][f]) for f in PAIR_FIELDS) == KNOWN_PAIR[outgroup]
    assert int(prec[0, 0]["n_skipped"]) == KNOWN_SKIPPED[outgroup] and int(prec[0, 0]["flags"]) == 0
    for (og, k, f), v in KNOWN_DIGITS.items():
        if og == outgroup:
            assert abs(float(stats[0, k][f]) - v) < 1e-8, (og, k, f, float(stats[0, k][f]))
    if jsfs is not None:
        t = jsfs[0][0]
        assert t.shape == (6, 6)
        assert {(int(a), int(b)): int(t[a, b]) for a, b in np.argwhere(t > 0)} == KNOWN_CELLS[outgroup]
    if sfs is not None:
        for k in range(3):
            assert sfs[k].shape == (1, len(KNOWN_POPS[k]) + 1) and int(sfs[k][0].sum()) == KNOWN_INTS[outgroup][k][0]
            assert int(sfs[k][0, 0]) == 0 and int(sfs[k][0, -1]) == 0
            assert int(sfs[k][0, 1]) == KNOWN_INTS[outgroup][k][1]  # eta1 is bin 1


def assert_not_hollow(ref, outgroup, flipped=0):
    """ref = plain_sfs.reference's result for the case, flipped = the sites the outgroup flipped.  At least two thirds of the
    (window, non-outgroup population) records with seg >= 2; every pair class non-zero in some record; when polarised some site
    skipped and some flipped; at least two thirds of the windows with >= 2 distinct non-zero joint cells in every pair's table."""
    stats, prec, _, jsfs = ref
    cols = [k for k in range(stats.shape[1]) if k != outgroup]
    seg = stats["seg"][:, cols]
    assert 3 * int((seg >= 2).sum()) >= 2 * seg.size, (int((seg >= 2).sum()), seg.size)
    for f in PAIR_FIELDS[:5]:
        assert prec[f].max() > 0, f
    if outgroup is not None:
        assert stats["n_skipped"].max() > 0 and flipped > 0
    for t in jsfs:
        cells = (t.reshape(t.shape[0], -1) > 0).sum(axis=1)
        assert 3 * int((cells >= 2).sum()) >= 2 * len(cells), cells.tolist()
