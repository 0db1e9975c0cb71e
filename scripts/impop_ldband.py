#!/usr/bin/env python3
"""Banded LD per BED row from bit matrices: the LD decay curve, per-site LD scores and a greedy LD pruning in one pass —
BitMatrix.ldband_scan (impop_ldband_scan) behind the tables of impop_amd/ldband.py.

    impop_ldband.py --matrix M [M ...] --bed BED [-u subset.txt] [--ldband-min-maf F] [--ldband-sites B] [--ldband-max-dist D]
                    [--ldband-bin-width w --ldband-bins N] [--ldband-r2 0.2] [--ldband-decay decay.tsv]
                    [--ldband-site-table sites.tsv] [--ldband-prune-in keep.txt] [--compact] [-o OUT] [--device N]

Main table, one row per BED row:  REGION LENGTH SAMPLES SITES QUALIFYING PAIRS MEAN_R2 STRONG PERFECT KEPT  (REGION =
chrom:start-end; QUALIFYING = sites whose minor allele is carried by at least ceil(F n) of the n sequences, at least 2 without
--ldband-min-maf, none of them thinned away; PAIRS = pairs of qualifying sites at most --ldband-sites sites, default 256, and at
most --ldband-max-dist coordinate units apart, default no limit; STRONG = pairs with r2 above --ldband-r2, a decimal with at most 4
places, default 0.2; KEPT = sites a greedy pruning at that r2 keeps; doubles as %.8f, NA where undefined).
--ldband-decay FILE: REGION BIN DIST_FROM DIST_TO PAIRS MEAN_R2 STRONG_FRACTION, --ldband-bins rows (default 100) of
--ldband-bin-width (default 1000) per BED row, the last bin open-ended.  --ldband-site-table FILE: REGION POS CARRIERS PARTNERS
LD_SCORE KEPT per qualifying site, LD_SCORE = the sum of r2 over its partners on both sides.  --ldband-prune-in FILE: chrom and
position of the kept sites, each once.  The pruning is greedy in position order, the earlier site stays: no parity with PLINK's
--indep-pairwise is claimed.  BED rows are matched to matrices by chromosome; one process, one GPU.
"""
import argparse
import math
import os
import re
import sys

import _bootstrap  # noqa: F401
import impop_amd
from impop_amd import _lib, ldband
from impop_scan import fail, flags_for, load_matrix, read_bed, site_bp

R2_SCALE = 10000


def parser():
    ap = argparse.ArgumentParser(description="per-window LD decay, LD scores and LD pruning from one banded pair pass (impop_ldband_scan)")
    ap.add_argument("--matrix", nargs="+", required=True)
    ap.add_argument("--bed", required=True)
    ap.add_argument("-u", "--subset", help="sequences to analyse (default: all)")
    ap.add_argument("--ldband-min-maf", type=float, default=None, metavar="F", help="minor-allele frequency a site needs (default: count 2)")
    ap.add_argument("--ldband-sites", type=int, default=256, metavar="B", help=f"partners on either side, 1..{_lib.LDBAND_MAX_BAND}")
    ap.add_argument("--ldband-max-dist", type=int, default=0, metavar="D", help="largest coordinate distance of a pair (default 0: no limit)")
    ap.add_argument("--ldband-bin-width", type=int, default=1000, metavar="w")
    ap.add_argument("--ldband-bins", type=int, default=100, metavar="N", help=f"1..{_lib.LDBAND_MAX_BINS}")
    ap.add_argument("--ldband-r2", default="0.2", metavar="R2", help="threshold of a strong pair and of the pruning, at most 4 decimal places")
    ap.add_argument("--ldband-decay", metavar="FILE", help="the decay curve")
    ap.add_argument("--ldband-site-table", metavar="FILE", help="LD score and pruning verdict per qualifying site")
    ap.add_argument("--ldband-prune-in", metavar="FILE", help="chrom and position of the sites the pruning keeps")
    ap.add_argument("--compact", action="store_true", help="scan from the matrix compacted to its variable sites: identical output")
    ap.add_argument("-o", "--output")
    ap.add_argument("--device", type=int, default=None, help="default: LOCAL_RANK, else 0")
    return ap


def threshold(text):
    """--ldband-r2 as (thr_num, 10000), or None where it is not a decimal in 0..1 with at most 4 places"""
    mt = re.fullmatch(r"(\d+)(?:\.(\d{0,4}))?", text.strip())
    if not mt:
        return None
    num = int(mt.group(1)) * R2_SCALE + int((mt.group(2) or "").ljust(4, "0") or "0")
    return (num, R2_SCALE) if num <= R2_SCALE else None


def refusal(args):
    """what is refused before any file is opened -> message or None"""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "impop_ldband.py runs in one process (WORLD_SIZE > 1: start it without torch.distributed.run)"
    if args.ldband_min_maf is not None and not 0.0 <= args.ldband_min_maf <= 0.5:
        return "--ldband-min-maf must lie in 0..0.5"
    if not 1 <= args.ldband_sites <= _lib.LDBAND_MAX_BAND:
        return f"--ldband-sites must lie in 1..{_lib.LDBAND_MAX_BAND}"
    if args.ldband_max_dist < 0:
        return "--ldband-max-dist must not be negative"
    if args.ldband_bin_width < 1:
        return "--ldband-bin-width must be at least 1"
    if not 1 <= args.ldband_bins <= _lib.LDBAND_MAX_BINS:
        return f"--ldband-bins must lie in 1..{_lib.LDBAND_MAX_BINS}"
    if threshold(args.ldband_r2) is None:
        return "--ldband-r2 must be a decimal in 0..1 with at most 4 places"
    return None


def min_mac(min_maf, n_members):
    """--ldband-min-maf F among n_members sequences as the min_mac of impop_ldband_scan; without it a minor count of 2"""
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
    want_sites = bool(args.ldband_site_table or args.ldband_prune_in)
    main_rows, decay_rows, site_rows = ([None] * len(rows) for _ in range(3))
    kept = {}  # chrom -> positions, over all its BED rows
    ctx = impop_amd.Context(args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", "0")))
    try:
        for key, idx in per_mat.items():
            mf = mats[key]
            mask = flags_for(args.subset, mf.names) if args.subset else None
            n_members = mf.n_hap if mask is None else int(mask.sum())
            if n_members == 0:
                fail("-u selects no sequence of the matrix")
            if n_members > _lib.LDBAND_MAX_N:
                fail(f"{n_members} sequences, more than the {_lib.LDBAND_MAX_N} a banded LD scan takes: narrow them with -u")
            wins = [mf.site_range(rows[i][1], rows[i][2]) + (rows[i][2] - rows[i][1],) for i in idx]
            bm = ctx.upload(mf.bits, mf.n_site, keep_hap_major=False)
            try:
                if mf.site_weight is not None:
                    bm.set_site_weights(mf.site_weight)
                if args.compact:
                    full, bm = bm, bm.compact()
                    full.free()
                got = bm.ldband_scan(wins, mask_p=mask, min_mac=min_mac(args.ldband_min_maf, n_members), band_sites=args.ldband_sites,
                                     max_dist=args.ldband_max_dist, bin_width=args.ldband_bin_width, n_bins=args.ldband_bins,
                                     threshold=threshold(args.ldband_r2), want_bins=True, want_sites=want_sites)
            finally:
                bm.free()
            recs, bins, table = got if want_sites else got + (None,)
            bp = site_bp(mf)
            for at, i in enumerate(idx):
                chrom, s, e = rows[i]
                region = f"{chrom}:{s}-{e}"
                main_rows[i] = ldband.main_row(region, e - s, recs[at])
                decay_rows[i] = ldband.decay_rows(region, bins[at], args.ldband_bin_width) if args.ldband_decay else []
                mine = ldband.site_rows_of(recs[at], table) if want_sites else []
                site_rows[i] = ldband.site_rows(region, mine, bp) if args.ldband_site_table else []
                if args.ldband_prune_in:
                    kept.setdefault(chrom, set()).update(ldband.kept_positions(mine, bp))
    finally:
        ctx.close()
    out = open(args.output, "w") if args.output else sys.stdout
    print("\t".join(ldband.MAIN_COLUMNS), file=out)
    for r in main_rows:
        print("\t".join(r), file=out)
    if args.output:
        out.close()
    for path, columns, blocks in ((args.ldband_decay, ldband.DECAY_COLUMNS, decay_rows), (args.ldband_site_table, ldband.SITE_COLUMNS, site_rows)):
        if path:
            with open(path, "w") as f:
                print("\t".join(columns), file=f)
                for block in blocks:
                    for r in block:
                        print("\t".join(r), file=f)
    if args.ldband_prune_in:
        with open(args.ldband_prune_in, "w") as f:
            for chrom in sorted(kept):
                for p in sorted(kept[chrom]):
                    print(f"{chrom}\t{p}", file=f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
