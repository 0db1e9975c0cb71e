"""The inputs of the impop_permtest_scan GPU tests (tests/test_gpu_permtest_scan.py), small and fixed.  What the tests rely on —
that the planted windows beat every labelling, that the exchangeable ones tie with every labelling, that the tie case passes 16,
that the multi-plane cases pass 255 / 65535 — is asserted on the plain restatement, on the CPU, by tests/test_permtest_cases_host.py.
"""
import numpy as np

SEED = 20261020
N = 140          # haplotypes of the shape cases
S = 96           # their sites
WINS3 = [(0, 40, 40), (40, 41, 1), (17, 96, 79)]  # three short windows: (site_begin, site_end, seq_len)


def matrix(n=N, s=S, seed=SEED):
    rng = np.random.default_rng(seed)
    freq = rng.random(s) ** 2
    m = (rng.random((n, s)) < freq[None, :]).astype(np.uint8)
    m[n // 2:, ::7] ^= 1  # some structure between the halves
    return m


def panels(sizes, n=N, seed=SEED):
    """disjoint panels of the given sizes, their members scattered over 0 .. n - 1 (so the merged order interleaves them)"""
    order = np.random.default_rng(seed + 1).permutation(n)
    out, at = [], 0
    for k in sizes:
        out.append(sorted(int(x) for x in order[at:at + k]))
        at += k
    return out


def flags(pops, n):
    out = []
    for p in pops:
        f = np.zeros(n, np.uint8)
        f[list(p)] = 1
        out.append(f)
    return out


# (panel sizes, n): the shapes that can break the tiling; K = 3 leaves haplotypes in no panel, K = 8 at n = 65
SHAPES = {"5_6": ((5, 6), N), "37_29": ((37, 29), N), "70_61": ((70, 61), N), "1_9": ((1, 9), N), "k3": ((20, 13, 31), N),
          "k8_n65": ((9, 8, 8, 8, 8, 8, 8, 8), 65)}
N_PERMS = (1, 17, 100)


def plane_case():
    """-> (m01 [24 x 400], windows): W = 0, W = 1 and 255 < W <= 65535 with a distance above 255"""
    m = matrix(24, 400, SEED + 2)
    m[:12, 60:400] = 0
    m[12:, 60:400] = 1  # 340 fixed differences between the halves
    m[::3, 100:130] ^= 1
    return m, [(5, 5, 0), (7, 8, 1), (0, 400, 400)]


def weighted_case():
    """-> (node matrix [24 x 40], weights, node windows, bp-expanded matrix, bp windows): one weight of 70000 inside a 40-site window"""
    rng = np.random.default_rng(SEED + 3)
    node = matrix(24, 40, SEED + 4)
    wt = rng.integers(1, 5, size=40).astype(np.uint32)
    wt[11] = 70000
    node[::2, 11] ^= 1
    edges = np.concatenate([[0], np.cumsum(wt.astype(np.int64))])
    node_wins = [(0, 40, 0), (0, 11, 0), (5, 30, 0)]
    bp_wins = [(int(edges[a]), int(edges[b]), 0) for a, b, _ in node_wins]
    return node, wt, node_wins, np.repeat(node, wt, axis=1), bp_wins


def tie_case():
    """-> (m01 [40 x 64], pops): 18 identical haplotypes inside panel 0 (tied_i = 17 for each) and duplicates across the panels"""
    m = matrix(40, 64, SEED + 5)
    pops = [list(range(0, 22)), list(range(22, 40))]
    m[0:18] = m[0]
    m[30] = m[20]   # a duplicate across the panels
    m[31] = m[20]
    return m, pops


def planted_case():
    """-> (m01 [24 x 80], pops, windows): windows 0 and 2 planted (50 fixed differences between the panels, private variation inside),
    window 1 exchangeable (all members identical)"""
    n = 24
    m = np.zeros((n, 240), np.uint8)
    for base in (0, 160):
        m[12:, base:base + 50] = 1
        for i in range(n):
            m[i, base + 50 + i] = 1  # a private site each: within-panel distances of 2
    pops = [list(range(0, 12)), list(range(12, 24))]
    return m, pops, [(0, 80, 80), (80, 160, 80), (160, 240, 80)]


def upper_case():
    """-> (m01 [1024 x 200], pops 512 + 512 interleaved, two windows)"""
    m = matrix(1024, 200, SEED + 6)
    return m, panels((512, 512), 1024, SEED + 7), [(0, 120, 120), (90, 200, 110)]
