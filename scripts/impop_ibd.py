#!/usr/bin/env python3
"""IBD segments per pair of sequences from bit matrices: BitMatrix.ibd_scan (impop_ibd_scan) behind the tables of impop_amd/ibd.py.

    impop_ibd.py --matrix M [M ...] --bed BED [-u subset.txt] [--ibd-pairs all|diploid] [--ibd-map plink.map]
                 [--ibd-min-seed 2.0 --ibd-min-extend 1.0 --ibd-min-output 2.0] [--ibd-max-gap 1000] [--ibd-min-sites 100]
                 [--ibd-segments seg.tsv] [--ibd-pair-table pairs.tsv] [--region-prefix P] [--compact] [-o OUT] [--device N]

A pair's exact identity-by-state tracts of at least --ibd-min-sites sites and --ibd-min-extend length are joined across gaps of at
most --ibd-max-gap sites; a chain is an IBD segment when it holds a tract of at least --ibd-min-seed and is --ibd-min-output long
(the seed-and-extend rule of include/impop_hip.h; --ibd-min-sites is the cost lever: every tract at least that long is staged on
the device).  With --ibd-map (a PLINK .map: chrom id cM bp) the three lengths are centimorgans with the defaults shown; without
one they are sites and all three must be given.  Pairs: every pair of the sequences of -u (default: all), or with --ibd-pairs
diploid the two haplotypes of every sample.  The scan covers each matrix's whole site range; the BED rows are its windows.
Main table, one row per BED row:  REGION LENGTH PAIRS SEGMENTS PAIRS_SPANNING PAIR_SITES SHARE.  --ibd-segments: seq1 seq2 start
end (bp, end exclusive) len (an integer: sites, or micro-centimorgans with a map) tracts ibs_sites open (L, R, LR or .) and, with a
map, cM with six decimals.  --ibd-pair-table: SEQ1 SEQ2 SEGMENTS CANDIDATES TOTAL_LEN TOTAL_EXTENT LONGEST_LEN IBS_SITES.
BED rows are matched to matrices by chromosome, as impop_scan.py does; one process, one GPU.
"""
import argparse
import os
import sys

import numpy as np

import _bootstrap  # noqa: F401
import impop_amd
from impop_amd import ibd
from impop_scan import fail, flags_for, load_matrix, pair_samples, read_bed, site_bp

CM_DEFAULTS = {"ibd_min_seed": "2.0", "ibd_min_extend": "1.0", "ibd_min_output": "2.0"}


def parser():
    ap = argparse.ArgumentParser(description="IBD segments from IBS tracts, gaps and a genetic map (impop_ibd_scan)")
    ap.add_argument("--matrix", nargs="+", required=True)
    ap.add_argument("--bed", required=True)
    ap.add_argument("-u", "--subset", metavar="LIST", help="the sequences to pair (default: all)")
    ap.add_argument("-p", "--region-prefix", default="CHM13#0#")
    ap.add_argument("--ibd-pairs", choices=["all", "diploid"], default="all")
    ap.add_argument("--ibd-map", metavar="FILE", help="PLINK .map (chrom id cM bp): lengths in centimorgans")
    ap.add_argument("--ibd-min-seed", metavar="X", help="cM with a map (default 2.0), else sites")
    ap.add_argument("--ibd-min-extend", metavar="X", help="cM with a map (default 1.0), else sites")
    ap.add_argument("--ibd-min-output", metavar="X", help="cM with a map (default 2.0), else sites")
    ap.add_argument("--ibd-max-gap", type=int, default=1000, metavar="N", help="sites between two joined tracts, at most")
    ap.add_argument("--ibd-min-sites", type=int, default=100, metavar="N", help="sites a tract needs to count at all")
    ap.add_argument("--ibd-segments", metavar="PATH")
    ap.add_argument("--ibd-pair-table", metavar="PATH")
    ap.add_argument("--compact", action="store_true", help="scan from the matrix compacted to its variable sites: identical output")
    ap.add_argument("-o", "--output")
    ap.add_argument("--device", type=int, default=None, help="default: LOCAL_RANK, else 0")
    return ap


def thresholds(args):
    """-> ((min_seed, min_extend, min_output) in map units or sites, None) or (None, the refusal)"""
    vals = []
    for key in ("ibd_min_seed", "ibd_min_extend", "ibd_min_output"):
        opt, text = "--" + key.replace("_", "-"), getattr(args, key)
        if args.ibd_map:
            try:
                vals.append(ibd.centimorgans(CM_DEFAULTS[key] if text is None else text))
            except ValueError as exc:
                return None, f"{opt}: {exc}"
        else:
            if text is None:
                return None, "without --ibd-map the lengths are sites: give --ibd-min-seed, --ibd-min-extend and --ibd-min-output"
            try:
                vals.append(int(text))
            except ValueError:
                return None, f"{opt}: without --ibd-map '{text}' must be a whole number of sites"
            if vals[-1] < 0:
                return None, f"{opt} takes 0 or more"
    if vals[0] < vals[1]:
        return None, "--ibd-min-seed is below --ibd-min-extend"
    return tuple(vals), None


def refusal(args):
    """what is refused before any file is opened -> message or None"""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "impop_ibd.py runs in one process (WORLD_SIZE > 1: start it without torch.distributed.run)"
    if args.ibd_min_sites < 1:
        return "--ibd-min-sites takes 1 or more"
    if args.ibd_max_gap < 0:
        return "--ibd-max-gap takes 0 or more"
    return thresholds(args)[1]


def main(argv=None):
    args = parser().parse_args(argv)
    why = refusal(args)
    if why:
        fail(why)
    (min_seed, min_extend, min_output), _ = thresholds(args)
    bed = read_bed(args.bed)

    def full_name(chrom):
        return chrom if chrom.startswith(args.region_prefix) else args.region_prefix + chrom
    mats = {}
    for p in args.matrix:
        mf = load_matrix(p)
        key = full_name(mf.contig) if mf.contig else ""
        if key in mats:
            fail(f"two matrices for contig '{mf.contig}' ({p})")
        mats[key] = mf
    if "" in mats and len(mats) > 1:
        fail("several --matrix files need a contig name each (matrixio `contig`)")
    rows, per_mat = [], {}
    for chrom, s, e in bed:
        region = f"{full_name(chrom)}:{s}-{e}"
        key = "" if "" in mats else full_name(chrom)
        if key not in mats:
            print(f"Warning: Skipping region {region}: no matrix holds chromosome {chrom}", file=sys.stderr)
            continue
        per_mat.setdefault(key, []).append(len(rows))
        rows.append((region, key, s, e))
    win = np.zeros(len(rows), dtype=impop_amd.IBS_WINDOW_DTYPE)
    n_pairs = np.zeros(len(rows), dtype=np.int64)
    seg_rows, pair_rows = [], []
    ctx = impop_amd.Context(args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", "0")))
    try:
        for key, idx in per_mat.items():
            mf = mats[key]
            kw = dict(min_seed=min_seed, min_extend=min_extend, min_output=min_output, max_gap=args.ibd_max_gap, min_sites=args.ibd_min_sites,
                      windows=[mf.site_range(rows[i][2], rows[i][3]) for i in idx], want_segments=bool(args.ibd_segments))
            if args.ibd_map:
                if mf.site_pos is not None:
                    fail("--ibd-map needs a matrix whose sites are consecutive bp (matrixio `origin`), not one with site_pos")
                try:
                    kw["map_pos"], kw["map_g"] = ibd.read_plink_map(args.ibd_map, mf.contig, mf.origin)
                except ValueError as exc:
                    fail(f"--ibd-map: {exc}")
                if len(kw["map_pos"]) < 2:
                    fail(f"--ibd-map: {len(kw['map_pos'])} rows for contig '{mf.contig}': a map needs two")
            mask_p = None if not args.subset else flags_for(args.subset, mf.names)
            if args.ibd_pairs == "diploid":
                kw["pairs"], _ = pair_samples("ibd", mf.names, mask_p, 1)
            else:
                n_matched = mf.n_hap if mask_p is None else int(mask_p.sum())
                if n_matched < 2:
                    fail(f"{n_matched} sequences make no pair")
                kw["mask_p"] = mask_p
            bm = ctx.upload(mf.bits, mf.n_site, keep_hap_major=False)
            try:
                if mf.site_weight is not None:
                    bm.set_site_weights(mf.site_weight)
                if args.compact:
                    full, bm = bm, bm.compact()
                    full.free()
                try:
                    prec, segs, win[idx], _ = bm.ibd_scan(**kw)
                except impop_amd.ImpopError as exc:
                    fail(exc.message)
            finally:
                bm.free()
            n_pairs[idx] = len(prec)
            if args.ibd_segments:
                seg_rows.extend(ibd.segment_rows(mf.names, segs, site_bp(mf), bool(args.ibd_map)))
            if args.ibd_pair_table:
                pair_rows.extend(ibd.pair_rows(mf.names, prec))
    finally:
        ctx.close()

    def table(fh, columns, body):
        print("\t".join(columns), file=fh)
        for r in body:
            print("\t".join(r), file=fh)
    out = open(args.output, "w") if args.output else sys.stdout
    table(out, ibd.MAIN_COLUMNS, ibd.main_rows([r[0] for r in rows], [r[3] - r[2] for r in rows], n_pairs, win))
    if args.output:
        out.close()
    if args.ibd_segments:
        with open(args.ibd_segments, "w") as fh:
            table(fh, ibd.SEGMENT_COLUMNS + (["cM"] if args.ibd_map else []), seg_rows)
    if args.ibd_pair_table:
        with open(args.ibd_pair_table, "w") as fh:
            table(fh, ibd.PAIR_COLUMNS, pair_rows)
    return 0


if __name__ == "__main__":
    sys.exit(main())
