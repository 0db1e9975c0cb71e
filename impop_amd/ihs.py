"""Host side of impop_ihs_scan: the record layout, the doubles formed from a record's exact integers, and the genome-wide
standardisation that turns them into scores.  All of it is plain numpy on the records BitMatrix.ihs_scan returns."""
from __future__ import annotations

import numpy as np

IHS_DTYPE = np.dtype([("site", "<u8"), ("n", "<u4", (2,)), ("c1", "<u4", (2,)), ("flags", "<u4"), ("reserved", "<u4"),
                      ("ihh2", "<u8", (2, 2)), ("sl2", "<u8", (2, 2))])
assert IHS_DTYPE.itemsize == 96
IHS_SCAN_MAX_N = 4096
EDGE_BITS, LIMIT_BITS = 0x00FF, 0xFF00
# a measure's EDGE bits: bit 4 measure + 2 class + half
EDGE_OF_MEASURE = (0x000F, 0x00F0)


def ihs_values(rec, k: int = 1) -> dict:
    """The doubles of records `rec` (IHS_DTYPE), k = the number of populations of the scan.  In this order: C_g = n_g (n_g - 1) / 2;
    iHH_g = (ihh2[g][0] + ihh2[g][1]) / (2 C_g), SL_g likewise; score = ln(iHH_1 / iHH_0) and ln(SL_1 / SL_0).  k = 1: the scores are
    iHS and nSL (allele 1 against allele 0), k = 2: XP-EHH and XP-nSL with population A against B, ln(iHH_A / iHH_B).  NaN where a
    term is 0 or a class has fewer than 2 members.  -> {"ihh": [n, 2], "sl": [n, 2], "ihs" | "xpehh": [n], "nsl" | "xpnsl": [n],
    "freq1": [n]} (freq1: the allele-1 frequency among all members)."""
    if k not in (1, 2):
        raise ValueError("k must be 1 or 2")
    rec = np.asarray(rec, dtype=IHS_DTYPE)
    n = rec["n"].astype(np.float64)
    C = n * (n - 1.0) / 2.0
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for name, field in (("ihh", "ihh2"), ("sl", "sl2")):
            tot = rec[field][:, :, 0].astype(np.float64) + rec[field][:, :, 1].astype(np.float64)
            v = tot / (2.0 * C)
            v[(rec["n"] < 2) | (tot == 0)] = np.nan
            out[name] = v
        num, den = (1, 0) if k == 1 else (0, 1)
        for score, name in ((("ihs", "xpehh")[k - 1], "ihh"), (("nsl", "xpnsl")[k - 1], "sl")):
            out[score] = np.log(out[name][:, num] / out[name][:, den])
        tot_n = rec["n"].sum(axis=1).astype(np.float64)
        out["freq1"] = rec["c1"].sum(axis=1).astype(np.float64) / tot_n
    return out


def standardize(score, flags, measure: int, freq1=None, bins: int = 50):
    """(score - mean) / sd (ddof = 1) over the cores that carry no EDGE bit of `measure` (0 = base pairs, 1 = sites) and whose score
    is finite.  With freq1 given (iHS, nSL): within each of `bins` equal bins of the allele-1 frequency on [0, 1); without (the XP
    scores): over all cores at once.  Every core gets a value from its bin's mean and sd, cores with an EDGE bit included; a bin
    with fewer than 2 contributing cores gives NaN."""
    score = np.asarray(score, dtype=np.float64)
    flags = np.asarray(flags)
    use = ((flags & EDGE_OF_MEASURE[measure]) == 0) & np.isfinite(score)
    if freq1 is None:
        which = np.zeros(len(score), dtype=np.int64)
        bins = 1
    else:
        if bins < 1:
            raise ValueError("bins must be at least 1")
        which = np.minimum((np.asarray(freq1, dtype=np.float64) * bins).astype(np.int64), bins - 1)
    out = np.full(len(score), np.nan)
    for b in range(bins):
        sel = which == b
        vals = score[sel & use]
        if len(vals) < 2:
            continue
        sd = vals.std(ddof=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[sel] = (score[sel] - vals.mean()) / sd
    return out
