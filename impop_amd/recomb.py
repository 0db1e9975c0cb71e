"""Host tables of BitMatrix.recomb_scan (impop_recomb_scan): the R_min breakpoint intervals and the maximal four-gamete blocks of a
window, derived from its site_table row and its used_sites row, and the rows of scripts/impop_recomb.py's tables.

Sites are indexed 0..n_used-1 in position order; `left1` of site j is 1 + the nearest site on its left that shows four gametes
with it (0: none).  Definitions: include/impop_hip.h, impop_recomb_scan."""
from __future__ import annotations

import math

import numpy as np

MAIN_COLUMNS = ("REGION", "LENGTH", "SAMPLES", "SITES", "QUALIFYING", "USED", "RMIN", "FGT_PAIRS", "FGT_FRACTION", "FGT_ADJACENT", "BLOCKS",
                "LONGEST_BLOCK_SITES", "LONGEST_BLOCK_START", "LONGEST_BLOCK_END", "WALL_B", "WALL_Q")
INTERVAL_COLUMNS = ("REGION", "INTERVAL", "LEFT_SITE", "RIGHT_SITE", "LEFT_POS", "RIGHT_POS")
BLOCK_COLUMNS = ("REGION", "BLOCK", "FIRST_SITE", "LAST_SITE", "SITES", "START", "END")


def intervals(left1, n_used: int):
    """the open intervals (left1_j - 1, j) Hudson & Kaplan's greedy takes, as site indices: each holds at least one recombination
    event, intervals that share an end point are disjoint; len() is the record's rmin"""
    cut, out = 0, []
    for j in range(int(n_used)):
        l = int(left1[j])
        if l >= 1 and l - 1 >= cut:
            out.append((l - 1, j))
            cut = j
    return out


def blocks(left1, n_used: int):
    """the maximal runs of pairwise compatible sites as (first, last) site indices; len() is the record's n_blocks"""
    m = int(n_used)
    if m == 0:
        return []
    run = np.maximum.accumulate(np.asarray(left1[:m], dtype=np.int64))
    return [(int(run[j]), j) for j in range(m) if j == m - 1 or run[j + 1] > run[j]]


def fmt(x) -> str:
    x = float(x)
    return "NA" if math.isnan(x) else "%.8f" % x


def main_row(region: str, length: int, rec, bp):
    """one row of the main table; bp maps an original site coordinate to a position"""
    m = int(rec["n_used"])
    return [region, str(length), str(int(rec["n_members"])), str(int(rec["n_sites"])), str(int(rec["n_qualifying"])), str(m),
            str(int(rec["rmin"])), str(int(rec["n_incompatible"])), fmt(rec["four_gamete_fraction"]), str(int(rec["n_incompatible_adjacent"])),
            str(int(rec["n_blocks"])), str(int(rec["longest_block_sites"])),
            str(bp(int(rec["longest_block_begin"]))) if m else "NA", str(bp(int(rec["longest_block_end"]))) if m else "NA",
            fmt(rec["wall_b"]), fmt(rec["wall_q"])]


def interval_rows(region: str, rec, site_row, used_row, bp):
    return [[region, str(k), str(a), str(b), str(bp(int(used_row[a]))), str(bp(int(used_row[b])))]
            for k, (a, b) in enumerate(intervals(site_row["left1"], rec["n_used"]))]


def block_rows(region: str, rec, site_row, used_row, bp):
    return [[region, str(k), str(a), str(b), str(b - a + 1), str(bp(int(used_row[a]))), str(bp(int(used_row[b])))]
            for k, (a, b) in enumerate(blocks(site_row["left1"], rec["n_used"]))]
