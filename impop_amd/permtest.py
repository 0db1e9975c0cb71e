"""The rows scripts/impop_scan.py --format permtest writes from the records of BitMatrix.permtest_scan (impop_permtest_scan).
Pure functions of the records: no device is touched here.  Long form: one row per window and pair of panels; the observed values
are per site where they have a unit (DXY / LENGTH), the counts and p-values as the call returned them."""
from __future__ import annotations

import math

from .pairdist import fmt, pair_order

MAIN_COLUMNS = ["REGION", "LENGTH", "POP_A", "POP_B", "N_A", "N_B", "N_PERM", "FST", "PHI_ST", "DXY", "SNN", "GE_FST", "GE_PHI", "GE_DXY",
                "GE_SNN", "P_FST", "P_PHI", "P_DXY", "P_SNN"]
NULL_COLUMNS = ["REGION", "POP_A", "POP_B", "PERM", "WA", "WB", "AB", "NN"]


def main_row(region, length, names, a, b, rec):
    row = [region, length, names[a], names[b], int(rec["n_a"]), int(rec["n_b"]), int(rec["n_perm"]), float(rec["fst"]), float(rec["phi_st"]),
           float(rec["dxy"]) / length if length else math.nan, float(rec["snn"]), int(rec["ge_fst"]), int(rec["ge_phi"]), int(rec["ge_dxy"]),
           int(rec["ge_snn"]), float(rec["p_fst"]), float(rec["p_phi"]), float(rec["p_dxy"]), float(rec["p_snn"])]
    return [fmt(x) for x in row]


def null_rows(region, names, a, b, rec, null):
    """the null distribution of one window and pair: a row per labelling, AB = tot - WA - WB with tot = wa + wb + ab of the record"""
    tot = int(rec["wa"]) + int(rec["wb"]) + int(rec["ab"])
    return [[region, names[a], names[b], str(r), str(int(e["wa"])), str(int(e["wb"])), str(tot - int(e["wa"]) - int(e["wb"])), str(int(e["nn"]))]
            for r, e in enumerate(null)]


def tables(regions, lengths, names, pairs, null=None):
    """-> (main rows, null rows) of a scan's result, headers excluded; null rows only with a null table"""
    order = pair_order(len(names))
    main, nul = [], []
    for w, region in enumerate(regions):
        for p, (a, b) in enumerate(order):
            main.append(main_row(region, lengths[w], names, a, b, pairs[w, p]))
            if null is not None:
                nul += null_rows(region, names, a, b, pairs[w, p], null[w, p])
    return main, nul
