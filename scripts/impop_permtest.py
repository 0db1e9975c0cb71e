#!/usr/bin/env python3
"""Permutation p-values for Hudson's Fst, AMOVA Phi_ST, Dxy and Hudson's S_nn per BED row and pair of population lists, from bit
matrices: BitMatrix.permtest_scan (impop_permtest_scan) behind the tables of impop_amd/permtest.py.

    impop_permtest.py --matrix M [M ...] --bed BED --panel a.txt b.txt [more.txt] [--perm-n 1000] [--perm-seed 1]
                      [--perm-null null.tsv] [--region-prefix P] [--compact] [-o OUT] [--device N]

--panel takes 2 to 8 disjoint lists of sequence names, at most 1024 sequences in all.  --perm-n labellings (default 1000, at most
16384) of seed --perm-seed (default 1) reassign the sequences of a pair of lists to its two lists; the same labellings serve every
BED row, so the p-values of neighbouring rows share their null draws.
Main table, one row per BED row and pair of lists:  REGION LENGTH POP_A POP_B N_A N_B N_PERM FST (Hudson) PHI_ST (AMOVA) DXY (per
site) SNN GE_FST GE_PHI GE_DXY GE_SNN (the labellings at least as differentiated as the observed one, compared in integers) P_FST
P_PHI P_DXY P_SNN (= (1 + GE) / (N_PERM + 1)); doubles printed with repr, NA where undefined.  --perm-null FILE: every labelling's
integers in long form, REGION POP_A POP_B PERM WA WB AB NN (rows x pairs x N_PERM at most 2^22 per matrix).
BED rows are matched to matrices by chromosome, as impop_scan.py does; one process, one GPU.
"""
import argparse
import os
import sys

import _bootstrap  # noqa: F401
import impop_amd
from impop_amd import _lib, permtest
from impop_scan import fail, flags_for, load_matrix, read_bed


def parser():
    ap = argparse.ArgumentParser(description="permutation p-values for Fst, Phi_ST, Dxy and S_nn per window (impop_permtest_scan)")
    ap.add_argument("--matrix", nargs="+", required=True)
    ap.add_argument("--bed", required=True)
    ap.add_argument("--panel", nargs="+", metavar="LIST", help="2 to 8 disjoint lists of sequence names")
    ap.add_argument("-p", "--region-prefix", default="CHM13#0#")
    ap.add_argument("--perm-n", type=int, default=1000, metavar="R", help="labellings per pair of lists, 1..16384")
    ap.add_argument("--perm-seed", type=int, default=1, metavar="S", help="seed of the labellings, 0..2^64 - 1")
    ap.add_argument("--perm-null", metavar="FILE", help="long-form table of every labelling's WA WB AB NN")
    ap.add_argument("--compact", action="store_true", help="scan from the matrix compacted to its variable sites: identical output")
    ap.add_argument("-o", "--output")
    ap.add_argument("--device", type=int, default=None, help="default: LOCAL_RANK, else 0")
    return ap


def refusal(args):
    """what is refused before any file is opened -> message or None"""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "impop_permtest.py runs in one process (WORLD_SIZE > 1: start it without torch.distributed.run)"
    if not args.panel or not 2 <= len(args.panel) <= 8:
        return "--panel takes a.txt b.txt [more.txt]: 2 to 8 population lists"
    if not 1 <= args.perm_n <= _lib.PERMTEST_MAX_PERM:
        return f"--perm-n must be 1..{_lib.PERMTEST_MAX_PERM}"
    if not 0 <= args.perm_seed < 1 << 64:
        return "--perm-seed must be 0..2^64 - 1"
    return None


def main(argv=None):
    args = parser().parse_args(argv)
    why = refusal(args)
    if why:
        fail(why)
    bed = read_bed(args.bed)
    labels = [os.path.splitext(os.path.basename(p))[0] for p in args.panel]
    NP = len(labels) * (len(labels) - 1) // 2

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
    main_rows = [None] * len(rows)
    null_rows = [None] * len(rows)
    ctx = impop_amd.Context(args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", "0")))
    try:
        for key, idx in per_mat.items():
            mf = mats[key]
            pops = [flags_for(f, mf.names) for f in args.panel]
            for k, f in enumerate(pops):
                if not f.any():
                    fail(f"--panel {args.panel[k]}: none of its sequences is in the matrix")
                for l in range(k):
                    if (f & pops[l]).any():
                        fail(f"--panel {args.panel[l]} and {args.panel[k]} share sequences: the lists must be disjoint")
            if sum(int(f.sum()) for f in pops) > _lib.PERMTEST_MAX_N:
                fail(f"the lists hold {sum(int(f.sum()) for f in pops)} sequences, more than the {_lib.PERMTEST_MAX_N} a permutation test takes")
            if args.perm_null and len(idx) * NP * args.perm_n > _lib.PERMTEST_MAX_NULL:
                fail(f"--perm-null: {len(idx)} BED rows x {NP} pairs x {args.perm_n} labellings, more than the {_lib.PERMTEST_MAX_NULL} entries "
                     "a null table takes")
            wins = [mf.site_range(rows[i][2], rows[i][3]) + (rows[i][3] - rows[i][2],) for i in idx]
            bm = ctx.upload(mf.bits, mf.n_site, keep_hap_major=True)
            try:
                if mf.site_weight is not None:
                    bm.set_site_weights(mf.site_weight)
                if args.compact:
                    full, bm = bm, bm.compact()
                    full.free()
                pairs, null = bm.permtest_scan(wins, pops, n_perm=args.perm_n, seed=args.perm_seed, null=bool(args.perm_null))
            finally:
                bm.free()
            m_rows, n_rows = permtest.tables([rows[i][0] for i in idx], [rows[i][3] - rows[i][2] for i in idx], labels, pairs, null)
            for n, i in enumerate(idx):
                main_rows[i] = m_rows[n * NP:(n + 1) * NP]
                null_rows[i] = n_rows[n * NP * args.perm_n:(n + 1) * NP * args.perm_n]
    finally:
        ctx.close()
    out = open(args.output, "w") if args.output else sys.stdout
    print("\t".join(permtest.MAIN_COLUMNS), file=out)
    for block in main_rows:
        for r in block:
            print("\t".join(r), file=out)
    if args.output:
        out.close()
    if args.perm_null:
        with open(args.perm_null, "w") as f:
            print("\t".join(permtest.NULL_COLUMNS), file=f)
            for block in null_rows:
                for r in block:
                    print("\t".join(r), file=f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
