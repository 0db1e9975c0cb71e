"""Values derived on the host from the integers of BitMatrix.pairdist_scan (impop_pairdist_scan), and the rows
scripts/impop_scan.py --format pairdist writes from them.  Pure functions of the records: no device is touched here."""
from __future__ import annotations

import math

NA = "NA"
MAIN_COLUMNS = ["REGION", "LENGTH", "POP_A", "POP_B", "PAIRS", "DXY", "DMIN", "DMIN_SEQ_A", "DMIN_SEQ_B", "DMAX", "IDENTICAL", "GMIN",
                "SNN", "NN_SAME_A", "NN_SAME_B", "NN_OTHER_A", "NN_OTHER_B"]
PANEL_COLUMNS = ["REGION", "POP", "HAPLOTYPES", "PAIRS", "MEAN", "VARIANCE", "MIN", "MAX", "IDENTICAL", "RAGGEDNESS"]
HIST_COLUMNS = ["REGION", "KIND", "POP", "BIN", "COUNT"]


def pair_order(K):
    """the pair order of scan_multi: (0,1),(0,2),..,(1,2),.."""
    return [(a, b) for a in range(K) for b in range(a + 1, K)]


def mean_h(rec) -> float:
    """mean distance of a record's pairs (NaN without pairs)"""
    n = int(rec["n_pairs"])
    return int(rec["sum_h"]) / n if n else math.nan


def variance_h(rec) -> float:
    """population variance of the distances, from the exact integers: (n sum_h2 - sum_h^2) / n^2"""
    n, s, s2 = int(rec["n_pairs"]), int(rec["sum_h"]), int(rec["sum_h2"])
    return (n * s2 - s * s) / (n * n) if n else math.nan


def raggedness(hist) -> float:
    """Harpending's raggedness r = sum_{i=1}^{B} (x_i - x_{i-1})^2 of a histogram's relative frequencies x_0 .. x_{B-1}, x_B = 0
    (NaN for an empty histogram).  With bins wider than one distance, or an overflowing last bin, it is the raggedness of the
    binned distribution."""
    total = sum(int(c) for c in hist)
    if not total:
        return math.nan
    x = [int(c) / total for c in hist] + [0.0]
    return sum((x[i] - x[i - 1]) ** 2 for i in range(1, len(x)))


def dmin_per_site(rec, length) -> float:
    return int(rec["min_h"]) / length if length else math.nan


def rnd_min(pair_kl, pair_ko, pair_lo) -> float:
    """RND_min = min_h(k, l) / ((mean H(k, O) + mean H(l, O)) / 2) for an outgroup panel O (NaN when the denominator is 0)"""
    den = (mean_h(pair_ko) + mean_h(pair_lo)) / 2
    return int(pair_kl["min_h"]) / den if den else math.nan


def fmt(x) -> str:
    if isinstance(x, float):
        return NA if x != x else repr(x)
    return str(x)


def main_row(region, length, names, a, b, rec, seq_names, rndmin=None):
    """one row of the main table: pair (a, b) of a window; rndmin: a float to append (with --pairdist-outgroup), or None"""
    has = int(rec["n_pairs"]) > 0
    row = [region, length, names[a], names[b], int(rec["n_pairs"]), mean_h(rec) / length if length else math.nan, int(rec["min_h"]),
           seq_names[int(rec["min_i"])] if has else NA, seq_names[int(rec["min_j"])] if has else NA, int(rec["max_h"]), int(rec["n_zero"]),
           float(rec["gmin"]), float(rec["snn"]), int(rec["nn_same_a"]), int(rec["nn_same_b"]), int(rec["nn_other_a"]),
           int(rec["nn_other_b"])]
    if rndmin is not None:
        row.append(float(rndmin))
    return [fmt(x) for x in row]


def panel_row(region, name, rec, hist=None):
    return [fmt(x) for x in (region, name, int(rec["n_members"]), int(rec["n_pairs"]), mean_h(rec), variance_h(rec), int(rec["min_h"]),
                             int(rec["max_h"]), int(rec["n_zero"]), raggedness(hist) if hist is not None else NA)]


def hist_rows(region, kind, label, hist):
    """long form, non-zero bins only"""
    return [[region, kind, label, str(b), str(int(c))] for b, c in enumerate(hist) if int(c)]


def outgroup_pair_index(K, k, o):
    a, b = (k, o) if k < o else (o, k)
    return pair_order(K).index((a, b))


def tables(regions, lengths, names, seq_names, panels, pairs, hist_within=None, hist_between=None, outgroup=None):
    """-> (main rows, panel rows, histogram rows) of a scan's result, headers excluded.  outgroup: index of the panel O; pairs
    that contain O get NA for RNDMIN."""
    K = len(names)
    order = pair_order(K)
    main, pan, hist = [], [], []
    for w, region in enumerate(regions):
        for p, (a, b) in enumerate(order):
            r = None
            if outgroup is not None:
                r = math.nan if outgroup in (a, b) else rnd_min(pairs[w, p], pairs[w, outgroup_pair_index(K, a, outgroup)],
                                                                pairs[w, outgroup_pair_index(K, b, outgroup)])
            main.append(main_row(region, lengths[w], names, a, b, pairs[w, p], seq_names, r))
            if hist_between is not None:
                hist += hist_rows(region, "between", f"{names[a]}:{names[b]}", hist_between[w, p])
        for k in range(K):
            pan.append(panel_row(region, names[k], panels[w, k], hist_within[w, k] if hist_within is not None else None))
            if hist_within is not None:
                hist += hist_rows(region, "within", names[k], hist_within[w, k])
    return main, pan, hist
