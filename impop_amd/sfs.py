"""Host-side companions of BitMatrix.sfs_scan: the neutrality statistics of a spectrum's integers, folding, and the sums of per-window
tables over blocks of windows.

Pure numpy / Python on the host: the per-window integers and tables come from the device (impop_sfs_scan); the doubles are formed
by the library's one host routine (impop_sfs_neutrality), so that a genome-wide record made from summed integers is computed
exactly as a window's is.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .distributed import shard_range

NEUTRALITY_FIELDS = ("theta_w", "theta_pi", "theta_h", "theta_l", "tajima_d", "faywu_h", "faywu_h_norm", "zeng_e")


def neutrality(n: int, seg: int, sum_het: int, sum_c: int, sum_c2: int) -> dict:
    """The eight doubles of an SFS_DTYPE record from its integers (n = the population's size), as impop_sfs_scan forms them:
    -> {theta_w, theta_pi, theta_h, theta_l, tajima_d, faywu_h, faywu_h_norm, zeng_e}.  Needs the built library, no device."""
    out = (C.c_double * 8)()
    _lib.check(_lib.load().impop_sfs_neutrality(int(n), int(seg), int(sum_het), int(sum_c), int(sum_c2), out))
    return dict(zip(NEUTRALITY_FIELDS, (float(x) for x in out)))


def fold(spectrum) -> np.ndarray:
    """Folds a 1-D spectrum over n sequences (n + 1 bins along the last axis, bin c = sites with c derived alleles) into
    n // 2 + 1 bins of the minor-allele count: bin j = spectrum[j] + spectrum[n - j], the middle bin of an even n once."""
    s = np.asarray(spectrum)
    n = s.shape[-1] - 1
    if n < 0:
        raise ValueError("a spectrum has at least one bin")
    half = n // 2
    out = s[..., :half + 1].copy()
    mirror = s[..., ::-1][..., :half + 1]
    out += mirror
    if n % 2 == 0:
        out[..., half] = s[..., half]
    return out


def block_sums(tables, n_blocks: int) -> np.ndarray:
    """Sums per-window tables (windows along axis 0) over n_blocks consecutive groups of windows, cut by impop_shard_range's rule
    (the first len % n_blocks groups hold one window more) as dstat.block_jackknife cuts its blocks -> [n_blocks, ...] uint64."""
    t = np.asarray(tables)
    B = int(n_blocks)
    if B < 1:
        raise ValueError("n_blocks must be at least 1")
    out = np.zeros((B,) + t.shape[1:], dtype=np.uint64)
    for j in range(B):
        lo, hi = shard_range(t.shape[0], B, j)
        out[j] = t[lo:hi].sum(axis=0, dtype=np.uint64)
    return out
