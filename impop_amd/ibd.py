"""Host side of scripts/impop_ibd.py: the reader of a PLINK .map as the genetic map of impop_ibd_scan, and the writers of its
three tables from the records of BitMatrix.ibd_scan."""
from __future__ import annotations

from decimal import ROUND_HALF_EVEN, Decimal, InvalidOperation

UNIT = 10 ** 6  # map units per centimorgan: micro-centimorgans

MAIN_COLUMNS = ["REGION", "LENGTH", "PAIRS", "SEGMENTS", "PAIRS_SPANNING", "PAIR_SITES", "SHARE"]
SEGMENT_COLUMNS = ["seq1", "seq2", "start", "end", "len", "tracts", "ibs_sites", "open"]
PAIR_COLUMNS = ["SEQ1", "SEQ2", "SEGMENTS", "CANDIDATES", "TOTAL_LEN", "TOTAL_EXTENT", "LONGEST_LEN", "IBS_SITES"]


def centimorgans(text) -> int:
    """a decimal number of centimorgans -> integer micro-centimorgans, rounded half to even"""
    try:
        v = (Decimal(str(text)) * UNIT).quantize(Decimal(1), rounding=ROUND_HALF_EVEN)
    except InvalidOperation:
        raise ValueError(f"'{text}' is not a number of centimorgans")
    if v < 0:
        raise ValueError(f"{text} centimorgans: a map position cannot be negative")
    return int(v)


def chrom_matches(chrom: str, contig: str) -> bool:
    """a .map row's chromosome against the matrix's contig: equal, or equal once a PanSN prefix and a leading 'chr' are dropped"""
    def bare(c):
        c = c.rsplit("#", 1)[-1]
        return c[3:] if c.startswith("chr") else c
    return chrom == contig or bare(chrom) == bare(contig)


def read_plink_map(path, contig: str, origin: int):
    """A PLINK .map (4 whitespace columns: chrom, id, cM, bp) -> (pos, g): site coordinates (bp - origin) and micro-centimorgans of
    the rows of `contig` (contig '': every row).  Rows of other chromosomes are dropped; bp must ascend strictly.  Rows left of the
    matrix's first site cannot be site coordinates: the last of them and the first row at or right of the origin give one
    breakpoint at site 0 (g interpolated as G itself interpolates, rounding down), the others are dropped."""
    rows = []
    with open(path) as f:
        for line_no, line in enumerate(f, 1):
            p = line.split()
            if not p or p[0].startswith("#"):
                continue
            if len(p) != 4:
                raise ValueError(f"{path}:{line_no}: a .map row has 4 columns (chrom id cM bp), this one has {len(p)}")
            if contig and not chrom_matches(p[0], contig):
                continue
            try:
                bp = int(p[3])
            except ValueError:
                raise ValueError(f"{path}:{line_no}: bp '{p[3]}' is not an integer")
            try:
                g = centimorgans(p[2])
            except ValueError as exc:
                raise ValueError(f"{path}:{line_no}: {exc}")
            if rows and bp <= rows[-1][0]:
                raise ValueError(f"{path}:{line_no}: bp {bp} does not ascend (the row before has {rows[-1][0]})")
            rows.append((bp, g))
    left = [r for r in rows if r[0] < origin]
    kept = [(bp - origin, g) for bp, g in rows if bp >= origin]
    if left and kept and kept[0][0] > 0:
        (bp0, g0), (x1, g1) = left[-1], kept[0]
        x0 = bp0 - origin  # negative
        kept.insert(0, (0, g0 + (0 - x0) * (g1 - g0) // (x1 - x0)))
    elif left and not kept:
        kept = [(0, left[-1][1]), (1, left[-1][1])]  # the whole map lies left of the matrix: G is its last value
    return [x for x, _ in kept], [g for _, g in kept]


def open_flag(flags: int) -> str:
    return ("L" if flags & 1 else "") + ("R" if flags & 2 else "") or "."


def main_rows(regions, lengths, n_pairs, win):
    """one row per BED row from the impop_ibs_window records of the segments"""
    out = []
    for reg, L, npair, r in zip(regions, lengths, n_pairs, win):
        share = float(r["share"])
        out.append([str(reg), str(L), str(int(npair)), str(int(r["tracts"])), str(int(r["pairs_spanning"])), str(int(r["pair_sites"])),
                    "NA" if share != share else f"{share:.8f}"])
    return out


def segment_rows(names, segs, site_bp, with_cm: bool):
    """impop_ibd_segment records; site_bp(site) = the position of a site in bp; with_cm: len is in micro-centimorgans, add a cM column"""
    out = []
    for q in segs:
        b, e, ln = int(q["begin"]), int(q["end"]), int(q["len"])
        row = [names[int(q["h1"])], names[int(q["h2"])], str(site_bp(b)), str(site_bp(e - 1) + 1), str(ln), str(int(q["n_tracts"])),
               str(int(q["ibs_sites"])), open_flag(int(q["flags"]))]
        if with_cm:
            row.append(f"{Decimal(ln) / UNIT:.6f}")
        out.append(row)
    return out


def pair_rows(names, recs):
    return [[names[int(q["h1"])], names[int(q["h2"])]] + [str(int(q[f])) for f in ("n_segments", "n_candidates", "total_len", "total_extent",
                                                                                "longest_len", "ibs_sites")] for q in recs]
