#!/usr/bin/env python3
"""Exact linkage trees per BED row ("local trees") from bit matrices: BitMatrix.tree_scan (impop_tree_scan) behind the tables of
impop_amd/tree.py.

    impop_tree.py --matrix M [M ...] --bed BED [-u subset.txt] [--panel a.txt b.txt ...] [--tree-linkage single|complete|average]
                  [--tree-newick trees.nwk] [--tree-merges merges.tsv] [--tree-panels panels.tsv] [--compact] [-o OUT] [--device N]

Main table, one row per BED row:  chrom start end n_members n_sites distinct tied_merges root_height rf_prev
(distinct = n_members - n_zero_merges, the distinct haplotypes of the window; tied_merges: steps at which the tie rule chose;
root_height: half the value of the last merge; rf_prev: the Robinson-Foulds distance to the previous row of the same matrix, NA
for its first).  --tree-newick FILE: chrom start end and the tree in Newick, one line per row, the leaves named by the sequences
of -u (all without).  --tree-merges FILE: long form, one row per merge.  --tree-panels FILE (needs --panel): one row per (BED row,
panel) with the largest clade inside the panel, its most recent common ancestor and whether the panel is monophyletic.
BED rows are matched to matrices by chromosome, as impop_scan.py does; one process, one GPU.
"""
import argparse
import os
import sys

import _bootstrap  # noqa: F401
import impop_amd
from impop_amd import _lib, tree
from impop_scan import fail, flags_for, load_matrix, panel_labels, read_bed


def parser():
    ap = argparse.ArgumentParser(description="per-window single / complete / average linkage trees of the haplotypes (impop_tree_scan)")
    ap.add_argument("--matrix", nargs="+", required=True)
    ap.add_argument("--bed", required=True)
    ap.add_argument("-u", "--subset", help="sequences to analyse (default: all)")
    ap.add_argument("--panel", nargs="+", default=[], metavar="LIST", help="up to 8 disjoint lists of sequences inside -u")
    ap.add_argument("--tree-linkage", choices=tree.LINKAGES, default="average")
    ap.add_argument("--tree-newick", metavar="FILE", help="the trees in Newick, one line per BED row")
    ap.add_argument("--tree-merges", metavar="FILE", help="long-form table of the merges")
    ap.add_argument("--tree-panels", metavar="FILE", help="clade statistics per (BED row, panel); needs --panel")
    ap.add_argument("--compact", action="store_true", help="scan from the matrix compacted to its variable sites: identical output")
    ap.add_argument("-o", "--output")
    ap.add_argument("--device", type=int, default=None, help="default: LOCAL_RANK, else 0")
    return ap


def refusal(args):
    """what is refused before any file is opened -> message or None"""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "impop_tree.py runs in one process (WORLD_SIZE > 1: start it without torch.distributed.run)"
    if len(args.panel) > 8:
        return "--panel takes at most 8 lists"
    if args.tree_panels and not args.panel:
        return "--tree-panels needs --panel"
    return None


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
    labels = panel_labels(args)
    main_rows, merge_rows, panel_rows, newick = ([None] * len(rows) for _ in range(4))
    ctx = impop_amd.Context(args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", "0")))
    try:
        for key, idx in per_mat.items():
            mf = mats[key]
            mask = flags_for(args.subset, mf.names) if args.subset else None
            members = [n for i, n in enumerate(mf.names) if mask is None or mask[i]]
            if len(members) < 2:
                fail("-u selects fewer than two sequences of the matrix")
            if len(members) > _lib.TREE_MAX_N:
                fail(f"{len(members)} sequences, more than the {_lib.TREE_MAX_N} a tree scan takes: narrow them with -u")
            pops = [flags_for(f, mf.names) for f in args.panel]
            for f, flags in zip(args.panel, pops):
                if not flags.any():
                    fail(f"--panel {f} matches no sequence of the matrix")
                if mask is not None and (flags & (1 - mask)).any():
                    fail(f"--panel {f} names sequences outside -u")
            wins = [mf.site_range(rows[i][1], rows[i][2]) + (rows[i][2] - rows[i][1],) for i in idx]
            bm = ctx.upload(mf.bits, mf.n_site, keep_hap_major=True)
            try:
                if mf.site_weight is not None:
                    bm.set_site_weights(mf.site_weight)
                if args.compact:
                    full, bm = bm, bm.compact()
                    full.free()
                recs, merges, panels = bm.tree_scan(wins, mask_p=mask, pops=pops, linkage=args.tree_linkage)
            finally:
                bm.free()
            m, g, p, n = tree.tables([rows[i] for i in idx], members, recs, merges, panels, labels, args.tree_linkage,
                                     want_merges=bool(args.tree_merges))
            per = len(members) - 1
            for at, i in enumerate(idx):
                main_rows[i], newick[i] = m[at], "\t".join([str(x) for x in rows[i]] + [n[at]])
                merge_rows[i] = g[at * per:(at + 1) * per] if args.tree_merges else []
                panel_rows[i] = p[at * len(labels):(at + 1) * len(labels)]
    finally:
        ctx.close()
    out = open(args.output, "w") if args.output else sys.stdout
    print("\t".join(tree.MAIN_COLUMNS), file=out)
    for r in main_rows:
        print("\t".join(r), file=out)
    if args.output:
        out.close()
    if args.tree_newick:
        with open(args.tree_newick, "w") as f:
            for line in newick:
                print(line, file=f)
    for path, columns, blocks in ((args.tree_merges, tree.MERGE_COLUMNS, merge_rows), (args.tree_panels, tree.PANEL_COLUMNS, panel_rows)):
        if path:
            with open(path, "w") as f:
                print("\t".join(columns), file=f)
                for block in blocks:
                    for r in block:
                        print("\t".join(r), file=f)
    return 0


if __name__ == "__main__":
    sys.exit(main())
