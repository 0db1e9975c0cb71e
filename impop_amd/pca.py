"""Values derived on the host from the records of BitMatrix.pca_scan (impop_pca_scan), and the rows scripts/impop_pca.py writes
from them.  Pure functions of the records: no device is touched here."""
from __future__ import annotations

import math

NA = "NA"
FLAG_UNCONVERGED = 1


def main_columns(k):
    return (["REGION", "LENGTH", "SAMPLES", "SITES", "RANK", "TOTAL_VAR"] + [f"LAMBDA{j + 1}" for j in range(k)]
            + [f"PVE{j + 1}" for j in range(k)] + ["ITERATIONS", "FLAGS"])


def vector_columns(k):
    return ["REGION", "SEQUENCE"] + [f"PC{j + 1}" for j in range(k)]


def total_var(rec) -> float:
    """trace(B) = sum_h / m"""
    return int(rec["sum_h"]) / int(rec["n_members"])


def pve(rec, j) -> float:
    """proportion of variance explained by pair j: lambda_j m / sum_h (NaN without variance)"""
    s = int(rec["sum_h"])
    return float(rec["lambda"][j]) * int(rec["n_members"]) / s if s else math.nan


def flag_text(rec) -> str:
    if int(rec["flags"]) & FLAG_UNCONVERGED:
        return "unconverged"
    return "rank0" if int(rec["rank"]) == 0 else "ok"


def fmt(x) -> str:
    if isinstance(x, float):
        return NA if x != x else repr(x)
    return str(x)


def main_row(region, length, rec, k):
    """one row of the main table.  Without variance (rank 0) the eigenvalues are 0.0 and the proportions NA."""
    row = [region, int(length), int(rec["n_members"]), int(rec["n_sites"]), int(rec["rank"]), total_var(rec)]
    row += [float(rec["lambda"][j]) for j in range(k)]
    row += [pve(rec, j) for j in range(k)]
    row += [int(rec["iterations"]), flag_text(rec)]
    return [fmt(x) for x in row]


def vector_rows(region, seq_names, rec, vectors, k):
    """long form: one row per member; the components of the pairs beyond the window's rank are NA"""
    rank = int(rec["rank"])
    return [[region, name] + [fmt(float(vectors[j][i])) if j < rank else NA for j in range(k)] for i, name in enumerate(seq_names)]


def tables(regions, lengths, seq_names, records, vectors, k):
    """-> (main rows, vector rows or None) of a scan's result, headers excluded; seq_names: the members in ascending index"""
    main = [main_row(r, lengths[w], records[w], k) for w, r in enumerate(regions)]
    vec = None
    if vectors is not None:
        vec = []
        for w, r in enumerate(regions):
            vec += vector_rows(r, seq_names, records[w], vectors[w], k)
    return main, vec
