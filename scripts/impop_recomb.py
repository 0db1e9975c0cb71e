#!/usr/bin/env python3
"""Recombination per BED row from bit matrices: the four-gamete test, Hudson & Kaplan's R_min with its breakpoint intervals,
four-gamete blocks and Wall's B and Q — BitMatrix.recomb_scan (impop_recomb_scan) behind the tables of impop_amd/recomb.py.

    impop_recomb.py --matrix M [M ...] --bed BED [-u subset.txt] [--recomb-min-maf F] [--recomb-max-sites N]
                    [--recomb-intervals iv.tsv] [--recomb-blocks blocks.tsv] [--compact] [-o OUT] [--device N]

Main table, one row per BED row:  REGION LENGTH SAMPLES SITES QUALIFYING USED RMIN FGT_PAIRS FGT_FRACTION FGT_ADJACENT BLOCKS
LONGEST_BLOCK_SITES LONGEST_BLOCK_START LONGEST_BLOCK_END WALL_B WALL_Q  (REGION = chrom:start-end; QUALIFYING = sites whose minor
allele is carried by at least ceil(F n) of the n sequences, at least 2 without --recomb-min-maf; USED = those left after thinning
to --recomb-max-sites, default 4096; FGT_PAIRS = pairs of used sites that show all four gametes; doubles as %.8f, NA where
undefined; positions are origin + site, as --format ld prints OMEGA_POS).  A thinned row's RMIN is still a lower bound.
--recomb-intervals FILE: one row per interval of R_min (each holds at least one recombination event).  --recomb-blocks FILE: one
row per maximal run of pairwise compatible sites.  BED rows are matched to matrices by chromosome; one process, one GPU.
"""
import argparse
import math
import os
import sys

import _bootstrap  # noqa: F401
import impop_amd
from impop_amd import _lib, recomb
from impop_scan import fail, flags_for, load_matrix, read_bed, site_bp


def parser():
    ap = argparse.ArgumentParser(description="per-window four-gamete test, Hudson-Kaplan R_min, blocks, Wall's B and Q (impop_recomb_scan)")
    ap.add_argument("--matrix", nargs="+", required=True)
    ap.add_argument("--bed", required=True)
    ap.add_argument("-u", "--subset", help="sequences to analyse (default: all)")
    ap.add_argument("--recomb-min-maf", type=float, default=None, metavar="F", help="minor-allele frequency a site needs (default: count 2)")
    ap.add_argument("--recomb-max-sites", type=int, default=None, metavar="N", help=f"2..{_lib.RECOMB_MAX_SITES}, default 4096")
    ap.add_argument("--recomb-intervals", metavar="FILE", help="the breakpoint intervals of R_min")
    ap.add_argument("--recomb-blocks", metavar="FILE", help="the maximal four-gamete blocks")
    ap.add_argument("--compact", action="store_true", help="scan from the matrix compacted to its variable sites: identical output")
    ap.add_argument("-o", "--output")
    ap.add_argument("--device", type=int, default=None, help="default: LOCAL_RANK, else 0")
    return ap


def refusal(args):
    """what is refused before any file is opened -> message or None"""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "impop_recomb.py runs in one process (WORLD_SIZE > 1: start it without torch.distributed.run)"
    if args.recomb_min_maf is not None and not 0.0 <= args.recomb_min_maf <= 0.5:
        return "--recomb-min-maf must lie in 0..0.5"
    if args.recomb_max_sites is not None and not 2 <= args.recomb_max_sites <= _lib.RECOMB_MAX_SITES:
        return f"--recomb-max-sites must lie in 2..{_lib.RECOMB_MAX_SITES}"
    return None


def min_mac(min_maf, n_members):
    """--recomb-min-maf F among n_members sequences as the min_mac of impop_recomb_scan; without it a minor count of 2"""
    return 2 if min_maf is None else max(1, int(math.ceil(min_maf * n_members)))


def main(argv=None):
    args = parser().parse_args(argv)
    why = refusal(args)
    if why:
        fail(why)
    bed = read_bed(args.bed)
    mats = {}
    for p in args.matrix:
        mf = load_matrix(p)
        key = mf.contig or ""
        if key in mats:
            fail(f"two matrices for contig '{mf.contig}' ({p})")
        mats[key] = mf
    if "" in mats and len(mats) > 1:
        fail("several --matrix files need a contig name each (matrixio `contig`)")
    rows, per_mat = [], {}
    for chrom, s, e in bed:
        key = "" if "" in mats else chrom
        if key not in mats:
            print(f"Warning: Skipping region {chrom}:{s}-{e}: no matrix holds chromosome {chrom}", file=sys.stderr)
            continue
        per_mat.setdefault(key, []).append(len(rows))
        rows.append((chrom, s, e))
    max_sites = args.recomb_max_sites or 4096
    want_tables = bool(args.recomb_intervals or args.recomb_blocks)
    main_rows, interval_rows, block_rows = ([None] * len(rows) for _ in range(3))
    ctx = impop_amd.Context(args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", "0")))
    try:
        for key, idx in per_mat.items():
            mf = mats[key]
            mask = flags_for(args.subset, mf.names) if args.subset else None
            n_members = mf.n_hap if mask is None else int(mask.sum())
            if n_members == 0:
                fail("-u selects no sequence of the matrix")
            if n_members > _lib.RECOMB_MAX_N:
                fail(f"{n_members} sequences, more than the {_lib.RECOMB_MAX_N} a recombination scan takes: narrow them with -u")
            wins = [mf.site_range(rows[i][1], rows[i][2]) + (rows[i][2] - rows[i][1],) for i in idx]
            bm = ctx.upload(mf.bits, mf.n_site, keep_hap_major=False)
            try:
                if mf.site_weight is not None:
                    bm.set_site_weights(mf.site_weight)
                if args.compact:
                    full, bm = bm, bm.compact()
                    full.free()
                got = bm.recomb_scan(wins, mask_p=mask, min_mac=min_mac(args.recomb_min_maf, n_members), max_sites=max_sites,
                                     want_sites=want_tables, want_site_table=want_tables)
            finally:
                bm.free()
            recs, used, table = got if want_tables else (got, None, None)
            bp = site_bp(mf)
            for at, i in enumerate(idx):
                chrom, s, e = rows[i]
                region = f"{chrom}:{s}-{e}"
                main_rows[i] = recomb.main_row(region, e - s, recs[at], bp)
                interval_rows[i] = recomb.interval_rows(region, recs[at], table[at], used[at], bp) if args.recomb_intervals else []
                block_rows[i] = recomb.block_rows(region, recs[at], table[at], used[at], bp) if args.recomb_blocks else []
    finally:
        ctx.close()
    out = open(args.output, "w") if args.output else sys.stdout
    print("\t".join(recomb.MAIN_COLUMNS), file=out)
    for r in main_rows:
        print("\t".join(r), file=out)
    if args.output:
        out.close()
    for path, columns, blocks in ((args.recomb_intervals, recomb.INTERVAL_COLUMNS, interval_rows),
                                  (args.recomb_blocks, recomb.BLOCK_COLUMNS, block_rows)):
        if path:
            with open(path, "w") as f:
                print("\t".join(columns), file=f)
                for block in blocks:
                    for r in block:
                        print("\t".join(r), file=f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
