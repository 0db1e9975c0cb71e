"""Inputs of the pairwise-distance-distribution tests (tests/test_gpu_pairdist_scan.py), kept apart so that the CPU suite can check
that they mean something (tests/test_pairdist_host.py) without a GPU.

matrix(n): af_cases.planted_matrix (16 segments of 128 sites) with features planted on top; panels(n, K): K disjoint panels that
interleave along the haplotype axis and leave every (K + 1)-th haplotype in no panel, with the planted rows placed by hand:
  * rows 0, 12 (panel 0) and 1 (panel 1) are one haplotype everywhere: between-panel n_zero > 0, nearest-neighbour ties across panels;
  * row 24 (panel 0) is a copy of row 5 (panel 1), which nothing else equals: its only nearest neighbour is in the other panel;
  * row 2 (last panel) is the complement of row 0 in segments 0 and 1: the maximum of the windows there is attained by (0, 2) and
    (12, 2) (and the minimum 0 by the copies), so the tie-break decides;
  * in segments 6, 7 and 8 every haplotype equals row 0: the windows inside them have H = 0 throughout (gmin NaN, all neighbours tied).
"""
import numpy as np

from af_cases import SEG, planted_matrix

N_SEG = 16
BINS, WIDTH = 16, 3  # the histogram of the parity tests: distances of 45 and more overflow into the last bin


def matrix(n, seed=None):
    m = planted_matrix(n, N_SEG, 9100 + n if seed is None else seed)
    m[12] = m[0]
    m[1] = m[0]
    m[24] = m[5]
    m[2, : 2 * SEG] = 1 - m[0, : 2 * SEG]
    m[:, 6 * SEG: 9 * SEG] = m[0, 6 * SEG: 9 * SEG]
    return m


def panels(n, K, planted=True):
    """-> K ascending index lists; planted False: the interleaved panels alone (for matrices without the planted rows)"""
    where = {i: i % (K + 1) for i in range(n)}
    if planted:
        where.update({0: 0, 12: 0, 24: 0, 2: K - 1})
        if K > 1:
            where.update({1: 1, 5: 1})
    return [[i for i in range(n) if where[i] == k] for k in range(K)]


def panels_flags(n, K, planted=True):
    """the same panels as 0/1 flag arrays, the form BitMatrix.pairdist_scan takes"""
    out = []
    for p in panels(n, K, planted):
        f = np.zeros(n, np.uint8)
        f[p] = 1
        out.append(f)
    return out


def window_lists():
    """tiling: 8 windows of two segments; sliding: three-segment windows stepping by one.  (begin, end, seq_len)"""
    tiling = [(2 * k * SEG, (2 * k + 2) * SEG, 2 * SEG) for k in range(N_SEG // 2)]
    sliding = [(k * SEG, (k + 3) * SEG, 3 * SEG) for k in range(N_SEG - 2)]
    return {"tiling": tiling, "sliding": sliding}


def segment_distances(m01):
    """H of every 128-site segment (int64): a window's distances are the sum of its segments'"""
    from plain_pairdist import gram, hamming
    return [hamming(gram(m01, s * SEG, (s + 1) * SEG)) for s in range(N_SEG)]


def window_distance(seg_H, win):
    return sum(seg_H[s] for s in range(win[0] // SEG, win[1] // SEG))


def planted_features(per_window, K):
    """what the planted rows must show in the plain reference's result [(panels, pairs, hw, hb) per window]; K >= 2 for the
    between-panel ones.  -> dict of booleans"""
    f = {}
    f["all_identical_window"] = any(all(r["sum_h"] == 0 for r in pa) and all(r["sum_h"] == 0 for r in pr) for pa, pr, _, _ in per_window)
    recs = [(r, h) for pa, pr, hw, hb in per_window for r, h in list(zip(pa, hw)) + list(zip(pr, hb))]
    f["overflow_bin"] = any(h is not None and h[-1] > 0 and r["max_h"] >= BINS * WIDTH for r, h in recs)
    if K > 1:
        f["between_zero"] = any(r["n_zero"] > 0 for _, pr, _, _ in per_window for r in pr)
        f["nan_gmin"] = any(r["gmin"] != r["gmin"] for _, pr, _, _ in per_window for r in pr)
        f["nn_other_a"] = any(r["nn_other_a"] > 0 and r["sum_h"] > 0 for _, pr, _, _ in per_window for r in pr)
    return f


def tie_counts(H, pops):
    """-> [(pairs attaining the minimum, pairs attaining the maximum)] per record of a window: panels, then pairs of panels"""
    out = []
    hs = [H[np.ix_(p, p)][np.triu_indices(len(p), 1)] for p in pops]
    hs += [H[np.ix_(pops[k], pops[l])].ravel() for k in range(len(pops)) for l in range(k + 1, len(pops))]
    for h in hs:
        out.append((int((h == h.min()).sum()), int((h == h.max()).sum())) if len(h) else (0, 0))
    return out
