"""Values derived on the host from the integers of Genotypes.kinship_scan (impop_kinship_scan), and the rows
scripts/impop_scan.py --format kinship writes from them.  Pure functions of the records: no device is touched here.

A joint genotype table is nine integers t[3 a + b]: the sites where individual i has genotype a and individual j genotype b
(0 hom-ref, 1 het, 2 hom-alt)."""
from __future__ import annotations

import math

NA = "NA"
WINDOW_COLUMNS = ["REGION", "LENGTH", "INDIVIDUALS", "PAIRS", "HET_HET", "IBS0", "IBS2", "RELATED", "UNDEFINED"]
PAIR_COLUMNS = ["IND_A", "IND_B", "SITES", "HET_A", "HET_B", "HET_HET", "IBS0", "IBS1", "IBS2", "KING_WITHIN", "KING_ROBUST", "IBS_DIST",
                "IBS0_FRAC", "DEGREE"]
WATCH_COLUMNS = ["REGION", "IND_A", "IND_B", "HET_A", "HET_B", "HET_HET", "IBS0", "KING_WITHIN", "KING_ROBUST"]
# the usual KING cut points on the robust estimator: (lower bound, label)
DEGREE_CUTS = [(0.354, "duplicate/MZ"), (0.177, "1st"), (0.0884, "2nd"), (0.0442, "3rd")]
KIN_DEN = 10000  # the CLI's threshold as num / KIN_DEN


def pair_order(N):
    """the pair order of scan_multi: (0,1),(0,2),..,(1,2),.."""
    return [(a, b) for a in range(N) for b in range(a + 1, N)]


def pair_index(N, i, j) -> int:
    return i * (2 * N - i - 1) // 2 + (j - i - 1)


def cells(t):
    """-> (n, het_i, het_j, het_het, ibs0, ibs1, ibs2) of a table"""
    t = [int(x) for x in t]
    return (sum(t), t[3] + t[4] + t[5], t[1] + t[4] + t[7], t[4], t[2] + t[6], t[1] + t[3] + t[5] + t[7], t[0] + t[4] + t[8])


def king_within(het_i, het_j, het_het, ibs0) -> float:
    """(het_het - 2 ibs0) / (het_i + het_j): one integer numerator, one integer denominator, one division"""
    den = int(het_i) + int(het_j)
    return (int(het_het) - 2 * int(ibs0)) / den if den else math.nan


def king_robust(het_i, het_j, het_het, ibs0) -> float:
    """(2 (het_het - 2 ibs0) + 2 m - het_i - het_j) / (4 m) with m = min(het_i, het_j): integers, then one division"""
    a, b = int(het_i), int(het_j)
    m = min(a, b)
    return (2 * (int(het_het) - 2 * int(ibs0)) + 2 * m - a - b) / (4 * m) if m else math.nan


def ibs_dist(ibs1, ibs2, n) -> float:
    """(ibs2 + 0.5 * ibs1) / n"""
    return (int(ibs2) + 0.5 * int(ibs1)) / int(n) if int(n) else math.nan


def ibs0_frac(ibs0, n) -> float:
    return int(ibs0) / int(n) if int(n) else math.nan


def degree(kr: float) -> str:
    if kr != kr:
        return NA
    for cut, label in DEGREE_CUTS:
        if kr > cut:
            return label
    return "unrelated"


def threshold_fraction(threshold: float):
    """a kinship threshold as (num, den) with den = KIN_DEN"""
    num = int(round(float(threshold) * KIN_DEN))
    if not 0 <= num <= KIN_DEN:
        raise ValueError("the kinship threshold must lie in 0 .. 1")
    return num, KIN_DEN


def fmt(x) -> str:
    if isinstance(x, float):
        return NA if x != x else repr(x)
    return str(x)


def window_row(region, length, rec):
    return [fmt(x) for x in (region, length, int(rec["n_ind"]), int(rec["n_pairs"]), int(rec["het_het"]), int(rec["ibs0"]), int(rec["ibs2"]),
                             int(rec["n_related"]), int(rec["n_undefined"]))]


def pair_row(name_a, name_b, t):
    n, a, b, hh, i0, i1, i2 = cells(t)
    kr = king_robust(a, b, hh, i0)
    return [fmt(x) for x in (name_a, name_b, n, a, b, hh, i0, i1, i2, king_within(a, b, hh, i0), kr, ibs_dist(i1, i2, n), ibs0_frac(i0, n),
                             degree(kr))]


def watch_row(region, name_a, name_b, rec):
    a, b, hh, i0 = int(rec["het_i"]), int(rec["het_j"]), int(rec["het_het"]), int(rec["ibs0"])
    return [fmt(x) for x in (region, name_a, name_b, a, b, hh, i0, king_within(a, b, hh, i0), king_robust(a, b, hh, i0))]


def tables(regions, lengths, ind_names, windows, pair_totals=None, watch=None, watch_rows=None):
    """-> (window rows, pair rows, watch rows), headers excluded.  pair_totals: [N(N-1)/2, 9] integers (any host sum of
    kinship_scan's pair tables); watch: [(i, j)] with watch_rows [n_windows, n_watch]."""
    N = len(ind_names)
    main = [window_row(region, lengths[w], windows[w]) for w, region in enumerate(regions)]
    pairs = []
    if pair_totals is not None:
        for p, (a, b) in enumerate(pair_order(N)):
            pairs.append(pair_row(ind_names[a], ind_names[b], pair_totals[p]))
    wat = []
    if watch:
        for w, region in enumerate(regions):
            for q, (a, b) in enumerate(watch):
                wat.append(watch_row(region, ind_names[a], ind_names[b], watch_rows[w][q]))
    return main, pairs, wat
