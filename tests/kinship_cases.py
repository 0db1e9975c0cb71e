"""Inputs of the kinship tests (tests/test_gpu_kinship_scan.py), kept apart so that the CPU suite can check that they mean something
(tests/test_kinship_host.py) without a GPU.

matrix(N): af_cases.planted_matrix (16 segments of 128 sites) over 2 N + 1 haplotypes; pairs(N): the individuals' copies drawn from a
fixed permutation, so they are non-adjacent, in either order, and one haplotype stays unpaired.  Planted on top:
  * individual 1 is a duplicate of individual 0 (both copies): ibs0 = 0, KING-robust 0.5 wherever het > 0;
  * N >= 3: individual 2 is a child of individual 0: it carries 0's first copy whole, so ibs0 = 0 between them;
  * N >= 5: individual 4 is homozygous throughout segments 6, 7 and 8: min(het) = 0 for its pairs in the windows inside them.
"""
import numpy as np

from af_cases import SEG, planted_matrix

N_SEG = 16
KIN = (884, 10000)  # the 3rd-degree cut point of KING as a fraction


def n_hap(N):
    return 2 * N + 1


def pairs(N):
    return np.random.default_rng(7000 + N).permutation(n_hap(N))[: 2 * N].reshape(N, 2).astype(np.uint32)


def matrix(N):
    m = planted_matrix(max(n_hap(N), 9), N_SEG, 9300 + N)[: n_hap(N)].copy()  # the generator's chains need nine rows
    pr = pairs(N)
    m[pr[1, 0]] = m[pr[0, 0]]
    m[pr[1, 1]] = m[pr[0, 1]]
    if N >= 3:
        m[pr[2, 1]] = m[pr[0, 0]]
    if N >= 5:
        m[pr[4, 1], 6 * SEG: 9 * SEG] = m[pr[4, 0], 6 * SEG: 9 * SEG]
    return m


def window_lists():
    """the lists of the pairdist cases: tiling, 8 windows of two segments; sliding, three-segment windows stepping by one; each with
    an empty window and a one-site window added.  (begin, end, seq_len)"""
    tiling = [(2 * k * SEG, (2 * k + 2) * SEG, 2 * SEG) for k in range(N_SEG // 2)]
    sliding = [(k * SEG, (k + 3) * SEG, 3 * SEG) for k in range(N_SEG - 2)]
    extra = [(300, 300, 0), (777, 778, 1)]
    return {"tiling": tiling[:3] + extra + tiling[3:], "sliding": sliding[:5] + extra + sliding[5:]}


def watch(N):
    """the planted pairs first, one of them with i > j"""
    w = [(1, 0)]
    if N >= 3:
        w += [(0, 2), (1, 2)]
    if N >= 5:
        w += [(4, 3), (N - 1, N - 2)]
    return w
