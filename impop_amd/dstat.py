"""Host-side companions of BitMatrix.dstat_scan: the genome-wide value of a ratio statistic with its block-jackknife error.

Pure numpy / Python on the host: the per-window integers come from the device (impop_dstat_scan), the few hundred blocks of a
jackknife are not work for a GPU.
"""
from __future__ import annotations

import math

import numpy as np

from .distributed import shard_range

NAN = float("nan")


def block_jackknife(num, den, n_blocks: int):
    """Delete-one block jackknife of theta = sum(num) / sum(den) over windows -> (theta, SE, Z, B).

    The windows, in order, are cut into n_blocks consecutive groups by impop_shard_range's rule (the first len % n_blocks
    groups hold one window more); N_j, D_j are a group's sums.  theta_(-j) = (sum N - N_j) / (sum D - D_j),
    SE = sqrt((B - 1) / B * sum_j (theta_(-j) - mean theta_(-j))^2), Z = theta / SE.  Groups with D_j = 0 are kept; with fewer
    than two groups of non-zero denominator SE = Z = NaN.  num / den: Python ints (object arrays, exact) or float64, as passed
    — for D: num = abba - baba, den = abba + baba; for f_d: its numerator and denominator in frequencies."""
    num, den = np.asarray(num), np.asarray(den)
    if num.shape != den.shape or num.ndim != 1:
        raise ValueError("num and den must be two 1-D arrays of one length")
    B = int(n_blocks)
    if B < 1:
        raise ValueError("n_blocks must be at least 1")
    zero = 0 if num.dtype == object and den.dtype == object else 0.0
    Nj, Dj = [], []
    for j in range(B):
        lo, hi = shard_range(len(num), B, j)
        Nj.append(sum(num[lo:hi].tolist(), zero))
        Dj.append(sum(den[lo:hi].tolist(), zero))
    N, D = sum(Nj, zero), sum(Dj, zero)
    theta = N / D if D != 0 else NAN
    if sum(1 for d in Dj if d != 0) < 2:
        return theta, NAN, NAN, B
    loo = [(N - n) / (D - d) if D - d != 0 else NAN for n, d in zip(Nj, Dj)]
    mean = sum(loo) / B
    se = math.sqrt((B - 1) / B * sum((t - mean) ** 2 for t in loo))
    return theta, se, (theta / se if se != 0 else NAN), B


def d_jackknife(recs, n_blocks: int):
    """block_jackknife of Patterson's D over one quartet's records (a column of dstat_scan's array), exact integer sums"""
    abba = np.array([int(x) for x in recs["abba"]], dtype=object)
    baba = np.array([int(x) for x in recs["baba"]], dtype=object)
    return block_jackknife(abba - baba, abba + baba, n_blocks)


def fd_jackknife(recs, sizes, n_blocks: int):
    """block_jackknife of Martin's f_d over one quartet's records; sizes = (n1, n2, n3, nO).  Numerator and denominator per
    window are the record's own expressions (include/impop_hip.h), in float64."""
    n1, n2, n3, nO = (int(x) for x in sizes)
    num = (recs["abba"] - recs["baba"]).astype(np.float64) / float(n1 * n2 * n3 * nO)
    den = recs["fd_den_p2"].astype(np.float64) / float(n1 * n2 * n2 * nO) + recs["fd_den_p3"].astype(np.float64) / float(n1 * n3 * n3 * nO)
    return block_jackknife(num, den, n_blocks)
