"""Inputs of the principal-component tests (tests/test_gpu_pca_scan.py), kept apart so that the CPU suite can check that they mean
something (tests/test_pca_cases_host.py) without a GPU.

The matrices and window lists are pairdist_cases', unmodified: planted segments, copied rows (repeated structure), and three
segments in which every haplotype is the same (windows of rank 0).  The masks: all members, every third haplotype, the pair
{0, 2} (m = 2: one non-zero eigenvalue, H_02 / 2) and three members (m = 3: rank <= 2 < k for k = 8).

preconditions(n, shape, mask) asserts, from the plain restatement alone, what the certified bounds of the GPU tests rest on:
  * the guaranteed regime of the header, lambda_{k+9} <= 0.9 lambda_j for every non-zero lambda_j, j <= k, for every k in KS;
  * no exact eigenvalue among the first k in (1e-13 trace, 1e-7 trace), where the zero rule could go either way.
"""
import functools

import numpy as np

import pairdist_cases as pc
import plain_pca as pl

NS = (31, 65, 465, 513)
KS = (1, 2, 4, 8)
MASKS = ("all", "third", "pair", "three")
TOL = 1e-10


def members(n, mask):
    return {"all": list(range(n)), "third": list(range(0, n, 3)), "pair": [0, 2], "three": [0, 2, 5]}[mask]


def flags(n, mask):
    """None for all members, else the 0/1 array BitMatrix.pca_scan takes"""
    if mask == "all":
        return None
    f = np.zeros(n, np.uint8)
    f[members(n, mask)] = 1
    return f


@functools.lru_cache(maxsize=None)
def matrix(n):
    return pc.matrix(n)


@functools.lru_cache(maxsize=None)
def references(n, shape, mask):
    """per window of the list: plain_pca.window at k = 8 (the spectrum is whole; rank is recounted per k by rank_at)"""
    m01 = matrix(n)
    return [pl.window(pl.distances(m01, w[0], w[1], members(n, mask)), w[1] - w[0], 8, TOL) for w in pc.window_lists()[shape]]


def rank_at(ref, k, tol=TOL):
    r = 0
    while r < min(k, ref["n_members"]) and ref["lam"][r] > tol * ref["trace"]:
        r += 1
    return r


def regime_ratio(ref, k):
    """the largest lambda_{k+9} / lambda_j over the non-zero lambda_j, j <= k (0.0 when lambda_{k+9} does not exist or is zero)"""
    lam, m = ref["lam"], ref["n_members"]
    tail = max(float(lam[k + 8]), 0.0) if k + 8 < m else 0.0
    worst = 0.0
    for j in range(min(k, m)):
        if lam[j] > 1e-13 * ref["trace"]:
            worst = max(worst, tail / float(lam[j]))
    return worst


def preconditions(n, shape, mask):
    """-> (worst regime ratio, ranks of the windows at k = 8); asserts the two conditions of the module text"""
    worst, ranks = 0.0, []
    for ref in references(n, shape, mask):
        ranks.append(rank_at(ref, 8))
        if ref["sum_h"] == 0:
            continue
        for k in KS:
            ratio = regime_ratio(ref, k)
            assert ratio <= 0.9, (n, shape, mask, k, ratio)
            worst = max(worst, ratio)
            for j in range(min(k, ref["n_members"])):
                assert not (1e-13 * ref["trace"] < ref["lam"][j] < 1e-7 * ref["trace"]), (n, shape, mask, k, j, ref["lam"][j], ref["trace"])
    return worst, ranks
