"""Host tables of BitMatrix.ldband_scan (impop_ldband_scan): the rows of scripts/impop_ldband.py's main, decay and site tables, and
the kept sites of the greedy LD pruning for feeding other tools.

r2 sums arrive as fixed-point integers (1.0 = 2^30); the decay bins hold the band pairs by coordinate distance; the site table is
one flat array, window w's rows at [site_off[w], site_off[w] + n_qualifying[w]).  The pruning is greedy in position order with the
earlier site staying: no parity with PLINK's --indep-pairwise is claimed.  Definitions: include/impop_hip.h, impop_ldband_scan."""
from __future__ import annotations

import math

import numpy as np

FX_ONE = 1 << 30
MAIN_COLUMNS = ("REGION", "LENGTH", "SAMPLES", "SITES", "QUALIFYING", "PAIRS", "MEAN_R2", "STRONG", "PERFECT", "KEPT")
DECAY_COLUMNS = ("REGION", "BIN", "DIST_FROM", "DIST_TO", "PAIRS", "MEAN_R2", "STRONG_FRACTION")
SITE_COLUMNS = ("REGION", "POS", "CARRIERS", "PARTNERS", "LD_SCORE", "KEPT")


def fmt(x) -> str:
    x = float(x)
    return "NA" if math.isnan(x) else "%.8f" % x


def mean_r2(sum_r2_fx: int, pairs: int) -> float:
    """the record's mean_r2, operation by operation"""
    return float(int(sum_r2_fx)) / (float(int(pairs)) * 1073741824.0) if int(pairs) else float("nan")


def site_rows_of(rec, table):
    """the rows of one window's record in the flat site table"""
    a = int(rec["site_off"])
    return table[a:a + int(rec["n_qualifying"])]


def main_row(region: str, length: int, rec):
    return [region, str(length), str(int(rec["n_members"])), str(int(rec["n_sites"])), str(int(rec["n_qualifying"])), str(int(rec["n_pairs"])),
            fmt(rec["mean_r2"]), str(int(rec["n_strong"])), str(int(rec["n_perfect"])), str(int(rec["n_kept"]))]


def decay_rows(region: str, bins, bin_width: int):
    """one row per decay bin of a window: distances DIST_FROM..DIST_TO inclusive, the last bin open-ended (DIST_TO NA)"""
    out, last = [], len(bins) - 1
    for b in range(len(bins)):
        pairs = int(bins["pairs"][b])
        out.append([region, str(b), str(b * int(bin_width)), "NA" if b == last else str((b + 1) * int(bin_width) - 1), str(pairs),
                    fmt(mean_r2(bins["sum_r2_fx"][b], pairs)), fmt(float(int(bins["n_strong"][b])) / float(pairs) if pairs else float("nan"))])
    return out


def site_rows(region: str, rows, bp):
    """one row per qualifying site of a window; bp maps an original site coordinate to a position"""
    return [[region, str(bp(int(r["coord"]))), str(int(r["carriers"])), str(int(r["n_partners"])), "%.8f" % (float(int(r["ld_score_fx"])) / FX_ONE),
             str(int(r["kept"]))] for r in rows]


def kept_positions(rows, bp=int):
    """the coordinates (through bp) of the sites the pruning keeps, in position order"""
    rows = np.asarray(rows)
    return [bp(int(c)) for c in rows["coord"][rows["kept"] == 1]]
