#!/usr/bin/env python3
"""Principal components per BED row ("local PCA") from bit matrices: BitMatrix.pca_scan (impop_pca_scan) behind the tables of
impop_amd/pca.py.

    impop_pca.py --matrix M [M ...] --bed BED [-u subset.txt] [--region-prefix P] [--pca-k 2] [--pca-tol 1e-10]
                 [--pca-max-iter 500] [--pca-vectors FILE] [--pca-dist FILE] [--compact] [-o OUT] [--device N]

Main table, one row per BED row:  REGION LENGTH SAMPLES SITES RANK TOTAL_VAR LAMBDA1..k PVE1..k ITERATIONS FLAGS
(TOTAL_VAR = sum_h / m = trace of the double-centred distance matrix; PVEj = LAMBDAj / TOTAL_VAR; NA where undefined; FLAGS =
ok, rank0 or unconverged).  --pca-vectors FILE: long form REGION SEQUENCE PC1..PCk, one row per sequence of -u (all without).
--pca-dist FILE: lostruct's window-to-window distance matrix as FILE (.npy, rows x rows float64, NaN for rank0 / unconverged rows)
with the region names, one per line, in FILE + ".tsv"; it is one call per matrix, so it takes exactly one --matrix.
BED rows are matched to matrices by chromosome, as impop_scan.py does; one process, one GPU.
"""
import argparse
import os
import sys

import numpy as np

import _bootstrap  # noqa: F401
import impop_amd
from impop_amd import _lib, pca
from impop_scan import fail, flags_for, load_matrix, read_bed, site_bp  # noqa: F401  (site_bp: the bp of a site, for callers)


def parser():
    ap = argparse.ArgumentParser(description="per-window principal components of the haplotypes (impop_pca_scan)")
    ap.add_argument("--matrix", nargs="+", required=True)
    ap.add_argument("--bed", required=True)
    ap.add_argument("-u", "--subset", help="sequences to analyse (default: all)")
    ap.add_argument("-p", "--region-prefix", default="CHM13#0#")
    ap.add_argument("--pca-k", type=int, default=2, metavar="K", help="eigenpairs per window, 1..8")
    ap.add_argument("--pca-tol", type=float, default=1e-10, metavar="TOL", help="relative residual bound, 1e-13..1e-2")
    ap.add_argument("--pca-max-iter", type=int, default=500, metavar="N", help="1..100000")
    ap.add_argument("--pca-vectors", metavar="FILE", help="long-form table of the eigenvectors")
    ap.add_argument("--pca-dist", metavar="FILE", help=".npy of the window-to-window distances, region names in FILE.tsv")
    ap.add_argument("--compact", action="store_true", help="scan from the matrix compacted to its variable sites: identical output")
    ap.add_argument("-o", "--output")
    ap.add_argument("--device", type=int, default=None, help="default: LOCAL_RANK, else 0")
    return ap


def refusal(args):
    """what is refused before any file is opened -> message or None"""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "impop_pca.py runs in one process (WORLD_SIZE > 1: start it without torch.distributed.run)"
    if not 1 <= args.pca_k <= _lib.PCA_MAX_K:
        return f"--pca-k must be 1..{_lib.PCA_MAX_K}"
    if not 1e-13 <= args.pca_tol <= 1e-2:
        return "--pca-tol must be in [1e-13, 1e-2]"
    if not 1 <= args.pca_max_iter <= 100000:
        return "--pca-max-iter must be 1..100000"
    if args.pca_dist and len(args.matrix) > 1:
        return "--pca-dist is one distance matrix over the windows of ONE matrix: give a single --matrix"
    return None


def main(argv=None):
    args = parser().parse_args(argv)
    why = refusal(args)
    if why:
        fail(why)
    bed = read_bed(args.bed)
    if args.pca_dist and len(bed) > _lib.PCA_MAX_DIST_WINDOWS:
        fail(f"--pca-dist: {len(bed)} BED rows, more than the {_lib.PCA_MAX_DIST_WINDOWS} a distance matrix takes")

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
    k = args.pca_k
    main_rows = [None] * len(rows)
    vec_rows = [None] * len(rows)
    dist = None
    ctx = impop_amd.Context(args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", "0")))
    try:
        for key, idx in per_mat.items():
            mf = mats[key]
            mask = flags_for(args.subset, mf.names) if args.subset else None
            members = [n for i, n in enumerate(mf.names) if mask is None or mask[i]]
            if len(members) < 2:
                fail("-u selects fewer than two sequences of the matrix")
            if len(members) > _lib.PCA_MAX_N:
                fail(f"{len(members)} sequences, more than the {_lib.PCA_MAX_N} a principal-component scan takes: narrow them with -u")
            wins = [mf.site_range(rows[i][2], rows[i][3]) + (rows[i][3] - rows[i][2],) for i in idx]
            bm = ctx.upload(mf.bits, mf.n_site, keep_hap_major=True)
            try:
                if mf.site_weight is not None:
                    bm.set_site_weights(mf.site_weight)
                if args.compact:
                    full, bm = bm, bm.compact()
                    full.free()
                recs, vecs, d2 = bm.pca_scan(wins, mask_p=mask, k=k, tol=args.pca_tol, max_iter=args.pca_max_iter,
                                             want_vectors=bool(args.pca_vectors or args.pca_dist), want_dist=bool(args.pca_dist))
            finally:
                bm.free()
            regions = [rows[i][0] for i in idx]
            m_rows, v_rows = pca.tables(regions, [rows[i][3] - rows[i][2] for i in idx], members, recs, vecs if args.pca_vectors else None, k)
            for n, i in enumerate(idx):
                main_rows[i] = m_rows[n]
                if v_rows is not None:
                    vec_rows[i] = v_rows[n * len(members):(n + 1) * len(members)]
            if d2 is not None:
                dist = (d2, regions)
    finally:
        ctx.close()
    out = open(args.output, "w") if args.output else sys.stdout
    print("\t".join(pca.main_columns(k)), file=out)
    for r in main_rows:
        print("\t".join(r), file=out)
    if args.output:
        out.close()
    if args.pca_vectors:
        with open(args.pca_vectors, "w") as f:
            print("\t".join(pca.vector_columns(k)), file=f)
            for block in vec_rows:
                for r in block:
                    print("\t".join(r), file=f)
    if args.pca_dist:
        d2, regions = dist if dist is not None else (np.zeros((0, 0)), [])
        with open(args.pca_dist, "wb") as f:  # the name as given: numpy.save would append .npy to a path without it
            np.save(f, d2)
        with open(args.pca_dist + ".tsv", "w") as f:
            for r in regions:
                print(r, file=f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
