"""Host side of scripts/impop_paint.py: the switch costs of a genetic map, and the tables made from the records of
BitMatrix.paint_scan (impop_paint_scan) — the segment list, the chunk-count and chunk-length matrices with names, and the long-form
local-ancestry table.  Host arithmetic only; the records themselves are integers from the device."""
from __future__ import annotations

import math

import numpy as np

MAX_COST = 1 << 20  # IMPOP_PAINT_MAX_COST
NO_PANEL = 255      # IMPOP_PAINT_NO_PANEL
NO_PANEL_LABEL = "none"

SEGMENT_COLUMNS = ["recipient", "donor", "start", "end", "sites", "mismatches"]
RECIPIENT_COLUMNS = ["RECIPIENT", "DONORS", "SEGMENTS", "COST", "MISMATCHES", "DISTINCT_DONORS", "LONGEST_SITES", "LONGEST_DONOR"]
ANCESTRY_COLUMNS = ["REGION", "RECIPIENT", "PANEL", "SITES", "SHARE"]
MAIN_COLUMNS = ["REGION", "LENGTH", "RECIPIENTS", "SWITCHES", "MISMATCHES", "CELLS"]


def switch_costs_from_map(positions, map_pos, map_cm, rho: float, scale: float) -> np.ndarray:
    """Per-site switch costs c_s (uint32, entry 0 = 0 and ignored) for stored sites at `positions` (ascending coordinates) from a
    genetic map (map_pos ascending coordinates, map_cm centimorgans, interpolated linearly and held constant outside the map).
    With d_s the map distance in Morgans between sites s-1 and s and p = 1 - exp(-rho * d_s), the probability of a switch,
        c_s = min(2^20, max(0, floor(scale * ln((1 - p) / p) + 0.5))),   and d_s = 0 gives 2^20.
    ln((1 - p) / p) = -ln p - (-ln(1 - p)) is the cost of switching MINUS the cost of staying: the Li-Stephens stay term is folded
    into the switch cost, which is all impop_paint_scan's recursion has room for; where a switch is likelier than a stay (p > 1/2)
    the cost is 0.  Host doubles only; the device sees the integers."""
    pos = np.asarray(positions, dtype=np.float64)
    cm = np.interp(pos, np.asarray(map_pos, dtype=np.float64), np.asarray(map_cm, dtype=np.float64))
    out = np.zeros(len(pos), dtype=np.uint32)
    for s in range(1, len(pos)):
        d = (cm[s] - cm[s - 1]) / 100.0
        if not d > 0.0:
            out[s] = MAX_COST
            continue
        p = 1.0 - math.exp(-float(rho) * d)
        if p <= 0.0:  # rho d below half an ulp of 1: the cost is past the cap anyway
            out[s] = MAX_COST
            continue
        v = math.floor(float(scale) * math.log((1.0 - p) / p) + 0.5) if p < 1.0 else 0
        out[s] = min(MAX_COST, max(0, int(v)))
    return out


def segment_rows(names, segs, site_bp):
    """impop_paint_segment records -> rows; site_bp(site) = the position of a site in bp; end is exclusive"""
    return [[names[int(q["h"])], names[int(q["donor"])], str(site_bp(int(q["begin"]))), str(site_bp(int(q["end"]) - 1) + 1),
             str(int(q["n_sites"])), str(int(q["n_mismatch"]))] for q in segs]


def recipient_rows(names, recs):
    return [[names[int(q["h"])], str(int(q["n_donors"])), str(int(q["n_segments"])), str(int(q["cost"])), str(int(q["n_mismatch"])),
             str(int(q["distinct_donors"])), str(int(q["longest_sites"])), names[int(q["longest_donor"])]] for q in recs]


def chunk_matrix(names, recs, table, donors=None):
    """one of the two [n_rec, n_hap] matrices as (header, rows): a row per recipient, a column per donor haplotype (donors: 0/1
    flags over the haplotypes, None = every haplotype) — the layout of ChromoPainter's chunkcounts / chunklengths files, with
    lengths in sites"""
    cols = [h for h in range(len(names)) if donors is None or donors[h]]
    header = ["RECIPIENT"] + [names[h] for h in cols]
    return header, [[names[int(q["h"])]] + [str(int(table[r, h])) for h in cols] for r, q in enumerate(recs)]


def ancestry_rows(regions, names, recs, anc, panel_labels):
    """anc [n_windows, n_rec, n_panels + 1] -> the long form: REGION RECIPIENT PANEL SITES SHARE (share of the recipient's sites of
    the window, six decimals; NA for a window without sites)"""
    labels = list(panel_labels) + [NO_PANEL_LABEL]
    out = []
    for w, reg in enumerate(regions):
        for r, q in enumerate(recs):
            tot = int(anc[w, r].sum())
            for p, lab in enumerate(labels):
                v = int(anc[w, r, p])
                out.append([str(reg), names[int(q["h"])], lab, str(v), "NA" if tot == 0 else f"{v / tot:.6f}"])
    return out


def main_rows(regions, lengths, n_rec, win):
    """one row per BED row from the impop_paint_window records; n_rec: the recipients behind each row"""
    return [[str(reg), str(L), str(int(k)), str(int(r["n_switches"])), str(int(r["n_mismatch"])), str(int(r["cells"]))]
            for reg, L, k, r in zip(regions, lengths, n_rec, win)]
