#!/usr/bin/env python3
"""Chromosome painting from bit matrices: BitMatrix.paint_scan (impop_paint_scan) behind the tables of impop_amd/paint.py.

    impop_paint.py --matrix M [M ...] --bed BED [-u recipients.txt] [--paint-donors donors.txt] [--panel a.txt b.txt ...]
                   [--paint-by-sample] [--paint-mismatch MU] [--paint-switch C | --paint-map plink.map --paint-rho R --paint-scale S]
                   [--paint-segments seg.tsv] [--paint-recipients rec.tsv] [--paint-chunkcounts cc.tsv] [--paint-chunklengths cl.tsv]
                   [--paint-ancestry anc.tsv] [--region-prefix P] [--compact] [-o OUT] [--device N]

Every sequence of -u (default: all) is painted as a Viterbi mosaic of the sequences of --paint-donors (default: all) other than
itself and, with --paint-by-sample, other than the second haplotype of its own sample (sample#1#..., sample#2#...).  The model is
the integer Li-Stephens recursion of include/impop_hip.h: --paint-mismatch per differing site (default 1), --paint-switch per change
of donor (default 1), or with --paint-map (a PLINK .map: chrom id cM bp) the per-site costs of
impop_amd.paint.switch_costs_from_map with --paint-rho (default 1.0) and --paint-scale (default 1.0).  It is the Viterbi path, not
the posterior painting, and no parity with ChromoPainter's output is claimed.  The scan covers each matrix's whole site range; the
BED rows are its windows.
Main table, one row per BED row:  REGION LENGTH RECIPIENTS SWITCHES MISMATCHES CELLS.  --paint-segments: recipient donor start end
(bp, end exclusive) sites mismatches.  --paint-recipients: RECIPIENT DONORS SEGMENTS COST MISMATCHES DISTINCT_DONORS LONGEST_SITES
LONGEST_DONOR.  --paint-chunkcounts / --paint-chunklengths: a row per recipient, a column per donor (lengths in sites).
--paint-ancestry (needs --panel): REGION RECIPIENT PANEL SITES SHARE, the panels by their lists' base names, then `none`.
BED rows are matched to matrices by chromosome, as impop_scan.py does; one process, one GPU.
"""
import argparse
import os
import sys

import numpy as np

import _bootstrap  # noqa: F401
import impop_amd
from impop_amd import ibd, paint
from impop_scan import fail, flags_for, load_matrix, panel_labels, read_bed, site_bp


def parser():
    ap = argparse.ArgumentParser(description="Li-Stephens Viterbi haplotype mosaics (impop_paint_scan)")
    ap.add_argument("--matrix", nargs="+", required=True)
    ap.add_argument("--bed", required=True)
    ap.add_argument("-u", "--subset", metavar="LIST", help="the recipients (default: all)")
    ap.add_argument("-p", "--region-prefix", default="CHM13#0#")
    ap.add_argument("--paint-donors", metavar="LIST", help="the donors (default: all)")
    ap.add_argument("--panel", nargs="+", default=[], metavar="LIST", help="up to 8 disjoint lists: the donors' panels")
    ap.add_argument("--paint-by-sample", action="store_true", help="a haplotype never copies from its own sample")
    ap.add_argument("--paint-mismatch", type=int, default=1, metavar="MU")
    ap.add_argument("--paint-switch", type=int, default=None, metavar="C")
    ap.add_argument("--paint-map", metavar="FILE", help="PLINK .map (chrom id cM bp): per-site switch costs")
    ap.add_argument("--paint-rho", type=float, default=1.0, metavar="R")
    ap.add_argument("--paint-scale", type=float, default=1.0, metavar="S")
    ap.add_argument("--paint-segments", metavar="PATH")
    ap.add_argument("--paint-recipients", metavar="PATH")
    ap.add_argument("--paint-chunkcounts", metavar="PATH")
    ap.add_argument("--paint-chunklengths", metavar="PATH")
    ap.add_argument("--paint-ancestry", metavar="PATH")
    ap.add_argument("--compact", action="store_true", help="paint the matrix compacted to its variable sites (a different, shorter model)")
    ap.add_argument("-o", "--output")
    ap.add_argument("--device", type=int, default=None, help="default: LOCAL_RANK, else 0")
    return ap


def refusal(args):
    """what is refused before any file is opened -> message or None"""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "impop_paint.py runs in one process (WORLD_SIZE > 1: start it without torch.distributed.run)"
    if not 1 <= args.paint_mismatch <= 65535:
        return "--paint-mismatch takes 1 .. 65535"
    if args.paint_map and args.paint_switch is not None:
        return "--paint-switch and --paint-map exclude each other"
    if args.paint_switch is not None and not 0 <= args.paint_switch <= paint.MAX_COST:
        return f"--paint-switch takes 0 .. {paint.MAX_COST}"
    if not args.paint_rho > 0.0 or not args.paint_scale >= 0.0:
        return "--paint-rho takes a positive number, --paint-scale a non-negative one"
    if len(args.panel) > 8:
        return "--panel takes at most 8 lists"
    if args.paint_ancestry and not args.panel:
        return "--paint-ancestry needs --panel"
    return None


def sample_groups(names):
    """group[h]: the two haplotypes of a sample share one, everyone else is alone"""
    from impop_amd.popnames import pair_haplotypes
    group = np.arange(len(names), dtype=np.uint32)
    for a, b in pair_haplotypes(list(names))[0]:
        group[b] = group[a]
    return group


def main(argv=None):
    args = parser().parse_args(argv)
    why = refusal(args)
    if why:
        fail(why)
    bed = read_bed(args.bed)
    labels = panel_labels(args)

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
    win = np.zeros(len(rows), dtype=impop_amd.PAINT_WINDOW_DTYPE)
    n_rec = np.zeros(len(rows), dtype=np.int64)
    seg_rows, rec_rows, cc_tabs, cl_tabs, anc_rows = [], [], [], [], []
    ctx = impop_amd.Context(args.device if args.device is not None else int(os.environ.get("LOCAL_RANK", "0")))
    try:
        for key, idx in per_mat.items():
            mf = mats[key]
            rflags = np.ones(mf.n_hap, np.uint8) if not args.subset else flags_for(args.subset, mf.names)
            dflags = np.ones(mf.n_hap, np.uint8) if not args.paint_donors else flags_for(args.paint_donors, mf.names)
            recipients = np.nonzero(rflags)[0].astype(np.uint32)
            if not len(recipients):
                fail("-u selects no sequence of the matrix")
            panel = np.full(mf.n_hap, paint.NO_PANEL, dtype=np.uint8)
            for k, f in enumerate(args.panel):
                pf = flags_for(f, mf.names).astype(bool)
                if (panel[pf] != paint.NO_PANEL).any():
                    fail(f"--panel: {labels[k]} shares a sequence with a list before it")
                panel[pf] = k
            kw = dict(donors=dflags, mismatch_cost=args.paint_mismatch, switch_cost=1 if args.paint_switch is None else args.paint_switch,
                      group=sample_groups(mf.names) if args.paint_by_sample else None, panel=panel if args.panel else None,
                      n_panels=len(args.panel), windows=[mf.site_range(rows[i][2], rows[i][3]) for i in idx],
                      want_segments=bool(args.paint_segments), want_ancestry=bool(args.paint_ancestry))
            bm = ctx.upload(mf.bits, mf.n_site, keep_hap_major=False)
            try:
                if args.compact:
                    full, bm = bm, bm.compact()
                    full.free()
                if args.paint_map:
                    if mf.site_pos is not None:
                        fail("--paint-map needs a matrix whose sites are consecutive bp (matrixio `origin`), not one with site_pos")
                    try:
                        mpos, mg = ibd.read_plink_map(args.paint_map, mf.contig, mf.origin)
                    except ValueError as exc:
                        fail(f"--paint-map: {exc}")
                    if len(mpos) < 2:
                        fail(f"--paint-map: {len(mpos)} rows for contig '{mf.contig}': a map needs two")
                    stored = bm.positions() if args.compact else np.arange(mf.n_site)
                    kw["site_switch_cost"] = paint.switch_costs_from_map(stored, mpos, np.asarray(mg, dtype=np.float64) / ibd.UNIT,
                                                                         args.paint_rho, args.paint_scale)
                try:
                    got = bm.paint_scan(recipients, **kw)
                except impop_amd.ImpopError as exc:
                    fail(exc.message)
            finally:
                bm.free()
            win[idx] = got["windows"]
            n_rec[idx] = len(recipients)
            recs = got["recipients"]
            if args.paint_segments:
                seg_rows.extend(paint.segment_rows(mf.names, got["segments"], site_bp(mf)))
            if args.paint_recipients:
                rec_rows.extend(paint.recipient_rows(mf.names, recs))
            if args.paint_chunkcounts:
                cc_tabs.append(paint.chunk_matrix(mf.names, recs, got["chunk_counts"], dflags))
            if args.paint_chunklengths:
                cl_tabs.append(paint.chunk_matrix(mf.names, recs, got["chunk_sites"], dflags))
            if args.paint_ancestry:
                anc_rows.extend(paint.ancestry_rows([rows[i][0] for i in idx], mf.names, recs, got["anc"], labels))
    finally:
        ctx.close()

    def table(fh, columns, body):
        print("\t".join(columns), file=fh)
        for r in body:
            print("\t".join(r), file=fh)
    out = open(args.output, "w") if args.output else sys.stdout
    table(out, paint.MAIN_COLUMNS, paint.main_rows([r[0] for r in rows], [r[3] - r[2] for r in rows], n_rec, win))
    if args.output:
        out.close()
    for path, columns, body in ((args.paint_segments, paint.SEGMENT_COLUMNS, seg_rows), (args.paint_recipients, paint.RECIPIENT_COLUMNS, rec_rows),
                                (args.paint_ancestry, paint.ANCESTRY_COLUMNS, anc_rows)):
        if path:
            with open(path, "w") as fh:
                table(fh, columns, body)
    for path, tabs in ((args.paint_chunkcounts, cc_tabs), (args.paint_chunklengths, cl_tabs)):
        if path:
            with open(path, "w") as fh:  # one block per matrix: its donors are its columns
                for header, body in tabs:
                    table(fh, header, body)
    return 0


if __name__ == "__main__":
    sys.exit(main())
