#!/usr/bin/env python3
"""Batch window driver: replaces the per-window `while read chr start end` loops of
run_pica2_impg.sh:126-190, run_h-fst.sh:155-190, run_tajd.sh:103-196 and run_fst_impg.sh:160-221 with GPU passes
over resident presence matrices, and prints the same TSV tables (headers run_pica2_impg.sh:119,122 /
run_h-fst.sh:148 / run_tajd.sh:101 / run_fst_impg.sh:158) so plot_*_trend.R work unchanged.

    impop_scan.py --matrix chr2.npz --bed windows.bed --format tajd -l samples.txt            # -t 0.999 -r 5 like run_tajd.sh
    impop_scan.py --matrix chr1.npz --bed windows.bed --format hfst -A afr.txt -B eas.txt [-r 5]
    impop_scan.py --matrix chr2.npz --bed windows.bed --format pica2 -t 0.999 -r 5 [-u subset.txt]
    impop_scan.py --matrix chr1.npz chr2.npz ... --bed genome.bed --format all ...            # one matrix per chromosome
    impop_scan.py --matrix chr2.npz --bed windows.bed --format all --panel afr.txt amr.txt eas.txt eur.txt sas.txt   # both panel drivers
    impop_scan.py --sim-list windows.tsv --format pica2 -t 0.999 -r 5                         # one `.sim` table per window
    impop_scan.py --matrix chr2.npz --bed windows.bed --format af [-t 1.0] [-u subset.txt] [--af-clusters c.tsv] [--af-details d.tsv]
    impop_scan.py --matrix chr2.npz --bed windows.bed --format ehh [--ehh-core-offset N | --ehh-cores pos.txt] [--ehh-flanks two-sided]
    impop_scan.py --matrix chr2.npz --bed windows.bed --format hapstats [-u subset.txt] [--compact]   # K, H1, H12, H2/H1 per window
    impop_scan.py --matrix chr2.npz --bed windows.bed --format ld [-u subset.txt] [--ld-min-maf F] [--ld-max-sites M]   # ZnS, |D'|, omega
    impop_scan.py --matrix chr2.npz --bed windows.bed --format diploid [-u subset.txt] [--roh-min-sites N] [--ind-table PATH]   # Ho, He, F_IS, ROH
    impop_scan.py --matrix chr2.npz --bed cores.bed --format ihs [-u subset.txt] [--ihs-min-maf F] [--ihs-cutoff F] [--ihs-max-extend BP] [--ihs-max-extend-sites N] [--ihs-bins B] [--ihs-keep-edge] [--compact]   # iHS / nSL per site
    impop_scan.py --matrix chr2.npz --bed cores.bed --format xpehh --panel a.txt b.txt [--ihs-...] [--compact]   # XP-EHH / XP-nSL per site
    impop_scan.py --matrix chr2.npz --bed windows.bed --format ibs [-u subset.txt] [--ibs-min-sites N] [--ibs-pairs all|diploid] [--ibs-segments PATH] [--ibs-pair-table PATH]   # IBS tracts / ROH segments
    impop_scan.py --matrix chr2.npz --bed windows.bed --format kinship [-u subset.txt] [--kin-threshold 0.0884] [--kin-pairs pairs.tsv] [--kin-watch sampleA,sampleB ...] [--kin-watch-table watch.tsv] [--compact]   # joint genotype tables, KING kinship per pair of samples
    impop_scan.py --matrix chr2.npz --bed windows.bed --format pairdist --panel a.txt b.txt [more.txt] [--pairdist-outgroup K] [--pairdist-panels panels.tsv] [--pairdist-hist hist.tsv --pairdist-bins B --pairdist-bin-width w] [--compact]   # d_min, G_min, S_nn, mismatch distributions
    impop_scan.py --matrix chr2.npz --bed windows.bed --format sfs --panel A.txt [B.txt ...] [--sfs-outgroup i] [--sfs-pair i,j]...   # spectra, neutrality tests
    impop_scan.py --matrix chr2.npz --bed windows.bed --format dstat --panel P1.txt P2.txt P3.txt O.txt [more.txt] [--quartet 1,2,3,4]...   # ABBA-BABA D, f4, f_d

--sim-list FILE (instead of --matrix / --bed): TSV rows `chrom  start  end  sim_path  [S]`, one `impg similarity` table per
window (a relative sim_path is taken from the list's directory).  Formats pica2, hfst, tajd, all; the tables of a chunk share
two kernel launches (impop_stats_from_identity_batch) while the next chunk is parsed on the host threads.  tajd / all need the
S column (segregating sites, run_tajd.sh:129-150) and -l.  A window whose table fails (missing file, invalid similarity value,
a population without sequences) is skipped with the reference driver's stderr lines; no per-window log files are written.

What -t / -r mean, per format (the THRESHOLD / R_VALUE columns always print what was computed):
  tajd    pica2's threshold / rounding behind the PI column and Tajima's D.  Defaults 0.999 and 5 — run_tajd.sh:9-10.
  pica2   pica2.py -t / -r (run_pica2_impg.sh requires both; here the default is 1.0 / no rounding).
  fst3pi  the three pica2 runs of run_fst_impg.sh:73 (same defaults as pica2).
  hfst    -r is h-fst.py -r (run_h-fst.sh:76-78); -t only with --fst-method grouped (hud.py -t, default 0.999).
  all     -t / -r as for tajd (same defaults) for the pica2 and tajd tables; the h-fst table rounds with --fst-round-digits.
  af      af.py --threshold (default 1.0, af.py:73); -r rounds the identity like pica2 -r first (af.py itself does not round).
  `-r none` switches rounding off where a default would apply.

--format af (scripts/af.py per window, impop_cluster_scan): haplotype clusters = connected components of {identity >= -t} among
the sequences of -u (default: all).  Main table REGION LENGTH THRESHOLD HAPLOTYPES CLUSTERS LARGEST SINGLETONS HOMOZYGOSITY
(homozygosity = sum of squared cluster frequencies, "%.6f" like af.py:60); --af-clusters FILE gets af.py's summary rows and
--af-details FILE its per-sample rows, each behind a REGION column.  One process, one GPU; not with --sim-list.  Sequence names
are cut at the first ':' as af.py cuts them and must then be distinct (af.py would merge two rows of one name into one sample).

--format ehh (scripts/wip/ehhgfa.py's scan, impop_ehh_scan): every BED row is a window with one core site, --ehh-core-offset N
(0-based site offset into the window; default its midpoint (end - begin) // 2) or --ehh-cores FILE (one bp position per BED row,
blank / # lines skipped; the first site at or right of it is the core).  One row per allele present at the core among the sequences
of -u (default: all): REGION LENGTH CORE ALLELE REF_ALT N_HAPLOTYPES AREA IHH_LEFT IHH_RIGHT.  CORE is the core site's bp position,
REF_ALT compares the allele with that of --ehh-ref NAME (default: the matrix's first sequence), IHH_LEFT / IHH_RIGHT are the integrals
of the two halves' EHH curves in sites and AREA their sum, all three exact thousandths printed as integer.milli ("12.276").
--ehh-flanks reference (default) takes both halves from the sites right of the core like ehhgfa.py:56-61, two-sided the left half
from the sites left of it.  One process, one GPU; not with --sim-list, -A / -B / --panel / -l, --compact, --devices N, -t / -r.

--format hapstats (impop_haplotype_scan): the haplotype-frequency statistics of every BED row among the sequences of -u (default:
all) - two sequences are the same haplotype when they agree at every site of the window.  One table REGION LENGTH SAMPLES SITES
HAPLOTYPES H1 H12 H2_H1 HAP_DIVERSITY (SAMPLES = sequences compared, SITES = the window's sites or summed weights, HAPLOTYPES = distinct
ones, H1 = haplotype homozygosity, H12 / H2_H1 after Garud et al., the doubles "%.8f").  Streams the scan index, needs no all-pairs
operand; --compact allowed.  One process, one GPU; not with --sim-list, -A / -B / --panel / -l, --devices N, -t / -r.

--format ld (impop_ld_scan): linkage disequilibrium between the sites of every BED row among the sequences of -u (default: all).
A site qualifies when its minor allele is carried by at least max(1, ceil(F * SAMPLES)) of them (--ld-min-maf F, default 0.05); more
than --ld-max-sites M qualifying sites (default 512, 4..1024) are thinned evenly to M.  One table REGION LENGTH SAMPLES SITES
QUALIFYING USED ZNS MEAN_DPRIME PERFECT COMPLETE OMEGA_MAX OMEGA_POS (ZNS = Kelly's mean r2 over the used pairs, PERFECT / COMPLETE =
pairs with r2 = 1 / |D'| = 1, OMEGA_MAX = the Kim-Nielsen omega at its best split and OMEGA_POS the position of the first used site
right of that split, NA when fewer than 4 sites are used; the doubles "%.8f").  Needs no all-pairs operand; --compact allowed.  One
process, one GPU; not with --sim-list, -A / -B / --panel / -l, --devices N, -t / -r.

--format diploid (impop_diploid_scan): the individual level.  The sequences of -u (default: all) are paired by their PanSN fields,
`sample#1#...` with `sample#2#...`; sequences of samples that are not exactly one of each are named in one warning and left out.
One table CHROM START END N_IND SITES HET_SITES HO HE FIS ROH_RUNS F_ROH LONGEST_RUN (HO = heterozygous sites per individual and
site, HE = 2 sum p q n / (n - 1) per site among the 2 N_IND copies, FIS = 1 - HO / HE, runs of homozygosity = stretches of at least
--roh-min-sites N sites (default 50) without a heterozygous site, F_ROH = the share of sites inside them; NA where undefined);
--ind-table PATH adds one row per window and sample: CHROM START END SAMPLE HET HOM_ALT LONGEST_RUN ROH_RUNS ROH_SITES.  --compact
allowed.  One process, one GPU; not with --sim-list, -A / -B / --panel / -l, --devices N, -t / -r.

--format ihs / xpehh (impop_ihs_scan): per-site integrated haplotype homozygosity from a device PBWT.  The site range is the whole
matrix of each BED row's contig; the row selects the cores (the sites of the row that vary among the sequences and whose minor-allele
frequency is at least --ihs-min-maf, default 0.05).  ihs: the sequences of -u (default: all), classes by allele, one row per core
CHROM SITE N0 N1 FREQ1 IHH0 IHH1 IHS IHS_STD SL0 SL1 NSL NSL_STD FLAGS; xpehh: the two lists of --panel, classes by population,
CHROM SITE NA NB FREQ1_A FREQ1_B IHH_A IHH_B XPEHH XPEHH_STD SL_A SL_B XPNSL XPNSL_STD FLAGS.  The EHH curve is integrated until it
falls below --ihs-cutoff (default 0.05), at most --ihs-max-extend site coordinates (default 1000000; 0 = no limit) for IHH and
--ihs-max-extend-sites varying sites (default 100; 0 = no limit) for SL.  The *_STD columns are standardised over all rows of the run:
iHS and nSL within --ihs-bins (default 50) bins of FREQ1, the XP scores over all cores.  Cores whose integral ran into the end of the
matrix (an EDGE bit in FLAGS) are left out unless --ihs-keep-edge is given.  Allele 1 against allele 0 is the caller's polarity.

--format ibs (impop_ibs_scan): pairwise identity-by-state tracts over the whole matrix of each BED row's contig, every pair of the
sequences of -u (default: all; --ibs-pairs all) or the two haplotypes of every sample (--ibs-pairs diploid: the PanSN pairing of
--format diploid, so the tracts are the runs of homozygosity as segments).  A tract is a maximal stretch of sites without a
difference between the two rows; tracts of at least --ibs-min-sites N sites (default 50) are reported.  One table REGION LENGTH
PAIRS TRACTS PAIRS_SPANNING PAIR_SITES SHARE, one row per BED row (TRACTS = reported tracts that meet the row's sites,
PAIRS_SPANNING = those that contain all of them, PAIR_SITES = sites of the row inside reported tracts summed over the pairs, SHARE =
PAIR_SITES / (PAIRS x the row's sites), "%.8f", NA for a row without sites); all BED rows of one matrix go into one call.
--ibs-segments PATH writes the segment list as TSV `seq1 seq2 start end sites open` (start / end in bp, end exclusive; open = L, R,
LR or . : the tract is cut by the matrix's first / last site, not by a difference), --ibs-pair-table PATH one row per pair: SEQ1
SEQ2 N_DIFF LONGEST TRACTS TRACT_SITES.  --compact allowed.  One process, one GPU; not with --sim-list, -A / -B / --panel / -l,
--devices N, -t / -r.

--format dstat (impop_dstat_scan): introgression statistics per BED row and quartet (P1, P2, P3, O) of the --panel lists (4..8 of
them).  --quartet i,j,k,o names a quartet by 1-based positions in --panel and may be repeated; with exactly four lists the default is
1,2,3,4.  The four populations of a quartet must not share a sequence.  One table CHROM START END P1 P2 P3 O N_SITES N_INFORMATIVE
N_SKIPPED ABBA BABA D F4 F_D, one row per window and quartet (P1..O = the lists' base names; ABBA / BABA = the summed site patterns in
frequencies; D = (ABBA - BABA) / (ABBA + BABA); F4 = mean (p1 - p2)(p3 - pO) summed over sites; F_D after Martin et al. 2015; the
doubles "%.8f", nan where undefined).  --dstat-polarize takes the outgroup's major allele as ancestral per site (N_SKIPPED = sites where
the outgroup is split evenly).  --dstat-blocks N with --dstat-summary PATH writes per quartet the value over all rows with its
block-jackknife error: P1 P2 P3 O D D_SE D_Z F_D F_D_SE BLOCKS ABBA BABA.  Streams the scan index; --compact allowed.  One process, one
GPU; not with --sim-list, -A / -B / -l / -u, --devices N, -t / -r.

--format kinship (impop_kinship_scan): a pair of individuals.  The sequences of -u (default: all) are paired into samples as --format
diploid pairs them; per BED row REGION LENGTH INDIVIDUALS PAIRS HET_HET IBS0 IBS2 RELATED UNDEFINED, the sums over all pairs of samples and
the pairs whose KING-robust kinship in the row is at least --kin-threshold (UNDEFINED: a sample without a heterozygous site).  --kin-pairs
PATH writes, per pair, the joint genotype counts summed over all rows and all --matrix files (integer sums on the host) with KING_WITHIN,
KING_ROBUST, IBS_DIST, IBS0_FRAC and the DEGREE label of the usual cut points 0.354 / 0.177 / 0.0884 / 0.0442.  --kin-watch A,B with
--kin-watch-table PATH follows pairs row by row.
--format pairdist (impop_pairdist_scan): the distribution of the pairwise distances H per BED row, from one Gram pass for all --panel
lists (1..8, disjoint).  Main table, one row per BED row and pair of lists: REGION LENGTH POP_A POP_B PAIRS DXY (mean H / LENGTH) DMIN
DMIN_SEQ_A DMIN_SEQ_B (the closest pair of sequences) DMAX IDENTICAL (pairs with H = 0) GMIN SNN NN_SAME_A NN_SAME_B NN_OTHER_A
NN_OTHER_B; --pairdist-outgroup K (1-based list) adds RNDMIN = DMIN / ((mean H(A,O) + mean H(B,O)) / 2), NA for the pairs that hold O.
--pairdist-panels PATH writes per row and list REGION POP HAPLOTYPES PAIRS MEAN VARIANCE MIN MAX IDENTICAL RAGGEDNESS (Harpending's, of
the histogram when one was asked for, else NA).  --pairdist-hist PATH with --pairdist-bins B (1..1024) and --pairdist-bin-width w
writes the histograms in long form, non-zero bins only: REGION KIND (within | between) POP (list, or listA:listB) BIN COUNT; the last
bin collects the overflow.  Doubles are printed with repr, NA where undefined.  --compact allowed.  One process, one GPU; not with
--sim-list, -A / -B / -l / -u, --devices N, -t / -r.

--format sfs (impop_sfs_scan): what is read from the site-frequency spectrum, per BED row and population of the --panel lists (1..8
of them).  One table CHROM START END POP N N_SITES S ETA1 ETA_N1 N_SKIPPED THETA_W THETA_PI THETA_H THETA_L TAJIMA_D FAYWU_H
FAYWU_H_NORM ZENG_E, one row per window and population (POP = the list's base name, N = its sequences in the matrix; the doubles
"%.8f", nan where undefined).  --sfs-outgroup i takes the major allele of list i (1-based) as ancestral per site; without it allele 1
counts as derived, which THETA_H, THETA_L, FAYWU_H, FAYWU_H_NORM and ZENG_E rely on.  --sfs-pair i,j (repeatable, lists that share no
sequence) with --sfs-pairs-out PATH writes per window and pair CHROM START END POP_A POP_B PRIVATE_A PRIVATE_B SHARED FIXED_A FIXED_B
N_UNION.  --sfs-spectra PATH.npz writes sfs_<label> and (per pair) jsfs_<a>_<b>, summed over the rows of each of --sfs-blocks N
consecutive groups of BED rows (default 1: the genome-wide spectra); the rows are scanned in batches, so the per-row tables never all
sit in host memory.  Streams the scan index; --compact allowed.  One process, one GPU; not with --sim-list, -A / -B / -l / -u,
--devices N, -t / -r.

--panel A.txt B.txt ... (2..8 disjoint lists; run_tajd_panels.sh / run_h_fst_panels.sh).  --format hfst: one h-fst table per pair,
headed `# A-vs-B`; --format tajd: one tajd table per panel, headed `# A`, SAMPLES = the list's line count, -t 0.999 -r 5 and S
over all rows like run_tajd.sh; --format all: the pair tables, then the panel tables (h-fst rounds with --fst-round-digits).  The
panels and pairs of a window share ONE Gram pass (impop_pairwise_scan_panel); only unrounded `match` h-fst tables alone keep the
streaming K-population scan (impop_scan_multi).  One process, one GPU; not with --fst-method grouped, -l, --devices N, --sim-list.

A threshold >= 1 without rounding on the `match` identity is the streaming site-count scan (every haplotype its own
group: exact integer identities); anything else runs the all-pairs path (impop_pairwise_scan).
BED rows are matched to matrices by chromosome (run_pica2_impg.sh:139-151 builds REGION from each row's own chromosome):
a row whose chromosome no matrix holds is skipped with a warning.
"""
import argparse
import contextlib
import math
import os
import sys
from types import SimpleNamespace

import numpy as np

import _bootstrap  # noqa: F401
import impop_amd
from impop_amd.drivers import bed_row_ok
from impop_amd.matrixio import load_matrix
from impop_amd.popnames import expand_population, read_subset_file


def read_bed(path, fmt="tajd"):
    """BED rows -> [(chrom, start, end)].  Comment / empty rows are skipped silently, unusable rows with the warning the
    reference driver of that table prints on stderr (impop_amd.drivers.bed_row_ok)."""
    rows = []
    with open(path) as f:
        for line_no, line in enumerate(f, 1):
            p = line.rstrip("\n").split("\t")
            if not p or not p[0] or p[0].startswith("#"):
                continue
            chrom = p[0]
            start, end = (p[1] if len(p) > 1 else ""), (p[2] if len(p) > 2 else "")
            if not bed_row_ok(chrom, start, end, line_no, fmt):
                continue
            rows.append((chrom, int(start), int(end)))
    return rows


def awk_line_count(list_file):
    """SAMPLE_COUNT of run_tajd.sh:83: `awk 'NF && $1 !~ /^#/' list | wc -l` — lines with at least one field whose
    first field does not start with '#'; a name listed twice counts twice."""
    n = 0
    with open(list_file) as f:
        for line in f:
            fields = line.split()
            if fields and not fields[0].startswith("#"):
                n += 1
    return n


def flags_for(list_file, names):
    raw = read_subset_file(list_file)
    members, missing = expand_population(raw, set(names))
    if missing:
        print(f"Warning: {len(missing)} identifiers from {os.path.basename(list_file)} did not match any sequences", file=sys.stderr)
    return np.array([1 if n in members else 0 for n in names], dtype=np.uint8)


def round_arg(v):
    if v.lower() in ("none", "off", ""):
        return "none"
    r = int(v)
    if r < 0:
        raise argparse.ArgumentTypeError("round digits must be >= 0 (or `none`)")
    return r


def threshold_arg(v):
    """-t keeps the user's TEXT next to the number: the bash drivers print "${THRESHOLD}" as typed (run_pica2_impg.sh:185-187,
    run_fst_impg.sh:220), so `-t 0.9990` must come back as 0.9990 in the THRESHOLD column"""
    x = float(v)
    if not (x == x):
        raise argparse.ArgumentTypeError("threshold must be a number")
    return (x, v)


class Runner:
    """One matrix on the device(s) + the three ways a row set can be scanned: one device, one process driving several
    contexts (--devices N, impop_*_sharded) or one rank of a torch.distributed job (records all-gathered once per scan)."""

    def __init__(self, args, mf, windows, need_pairs, rank, world, local_rank):
        self.args, self.mf, self.rank, self.world, self.local_rank = args, mf, rank, world, local_rank
        self.all_wins = impop_amd.make_windows(windows)
        self.n_total = len(self.all_wins)
        self.ctx = impop_amd.Context(args.device)
        self.bm, self.slabs, self.ctxs, self.begins = None, [], [], []
        self.local_wins = self.all_wins
        if args.devices > 1:
            from impop_amd import engine
            import ctypes as C
            n_dev = C.c_int(0)
            impop_amd._lib.load().impop_device_count(C.byref(n_dev))
            for k in range(args.devices):
                first, cnt, s0, s1 = engine.shard_windows_c(self.all_wins, args.devices, k)
                w0, w1 = s0 // 64, max((s1 + 63) // 64, s0 // 64 + 1)
                ck = impop_amd.Context(k if n_dev.value >= args.devices else 0)
                n_slab = max(min(mf.n_site, 64 * w1) - 64 * w0, 0)
                sk = ck.upload(np.ascontiguousarray(mf.bits[:, w0:w1]), n_slab, keep_hap_major=need_pairs)
                if mf.site_weight is not None:
                    sk.set_site_weights(mf.site_weight[64 * w0: 64 * w0 + n_slab])
                self.ctxs.append(ck); self.slabs.append(sk); self.begins.append(64 * w0)
        elif world > 1:
            from impop_amd.distributed import shard_windows
            loc, s0, s1, _ = shard_windows(self.all_wins, world, rank)
            w0, w1 = s0 // 64, (s1 + 63) // 64  # slab = whole 64-bit words of the hap-major rows
            slab = np.ascontiguousarray(mf.bits[:, w0:w1]) if len(loc) else np.zeros((mf.n_hap, 1), np.uint64)
            shift = s0 - 64 * w0
            loc = loc.copy()
            loc["site_begin"] += np.uint64(shift)
            loc["site_end"] += np.uint64(shift)
            n_slab = max(min(mf.n_site, 64 * w1) - 64 * w0, 0)
            self.bm = self.ctx.upload(slab, n_slab, keep_hap_major=need_pairs)
            if mf.site_weight is not None:
                self.bm.set_site_weights(mf.site_weight[64 * w0: 64 * w0 + n_slab])
            self.local_wins = loc
        else:
            self.bm = self.ctx.upload(mf.bits, mf.n_site, keep_hap_major=need_pairs)
            if mf.site_weight is not None:
                self.bm.set_site_weights(mf.site_weight)
        if args.compact:
            full = self.bm
            self.bm = full.compact()
            full.free()

    def _gather(self, res):
        if self.world > 1:
            from impop_amd.distributed import gather_records
            import torch
            dev = torch.device("cuda", self.local_rank) if self.args.backend == "nccl" else None
            res = gather_records(res, self.n_total, self.world, self.rank, dev)
        return res

    def stream(self, mask_p, mask_a, mask_b):
        """the streaming site-count scan: pica2 at threshold >= 1 unrounded, h-fst unrounded, S, D (STATS records)"""
        if self.slabs:
            from impop_amd import engine
            return engine.scan_sharded(self.slabs, self.begins, self.all_wins, mask_p, mask_a, mask_b)
        return self._gather(self.bm.scan(self.local_wins, mask_p, mask_a, mask_b))

    def pairs(self, mask_p, mask_a, mask_b, threshold, round_digits, want_s, fst_method="direct"):
        """the all-pairs path: thresholded / rounded pica2, rounded or grouped Fst (PAIRWISE records).  want_s False skips
        the S / D part (s_scope 2)."""
        kw = dict(kind=self.args.identity, threshold=threshold, round_digits=round_digits, s_scope=0 if want_s else 2,
                  fst_method=fst_method)
        if self.slabs:
            from impop_amd import engine
            return engine.pairwise_scan_sharded(self.slabs, self.begins, self.all_wins, mask_p, mask_a, mask_b, **kw)
        return self._gather(self.bm.pairwise_scan(self.local_wins, mask_p, mask_a, mask_b, **kw))

    def panel(self, pops):
        pr = self.bm.scan_multi(self.local_wins, pops)
        if self.world > 1:  # one all-gather of [window, pair] records, a window's pairs travelling as one item
            from impop_amd.distributed import gather_records
            import torch
            n_pairs = pr.shape[1]
            item = np.dtype((np.void, n_pairs * pr.dtype.itemsize))
            flat = np.ascontiguousarray(pr).reshape(-1).view(item) if len(pr) else np.zeros(0, dtype=item)
            dev = torch.device("cuda", self.local_rank) if self.args.backend == "nccl" else None
            full = gather_records(flat, self.n_total, self.world, self.rank, dev)
            pr = full.view(pr.dtype).reshape(self.n_total, n_pairs)
        return pr

    def panel_allpairs(self, pops, threshold, round_digits, want_s, want_pairs):
        """K panels and their pairs from one Gram pass per window (impop_pairwise_scan_panel): thresholded / rounded pica2 and
        Tajima's D per panel, rounded or `dice` h-fst per pair -> (panels, pairs, windows).  One process, one GPU."""
        return self.bm.pairwise_scan_panel(self.local_wins, pops, kind=self.args.identity, threshold=threshold, round_digits=round_digits,
                                           s_scope=0 if want_s else 2, want_pairs=want_pairs)

    def hapstats(self, mask_p):
        """haplotype-frequency statistics per window (impop_haplotype_scan; HAPLOTYPE records).  One process, one GPU."""
        return self.bm.haplotype_scan(self.local_wins, mask_p=mask_p)

    def ld(self, mask_p, min_mac, max_sites):
        """linkage disequilibrium per window (impop_ld_scan) -> (LD records, used_sites).  One process, one GPU."""
        return self.bm.ld_scan(self.local_wins, mask_p=mask_p, min_mac=min_mac, max_sites=max_sites, want_sites=True)

    def diploid(self, pairs, min_run, want_individuals):
        """the individual level per window (impop_diploid_scan) -> DIPLOID records, or (records, rows).  One process, one GPU."""
        return self.bm.diploid_scan(self.local_wins, pairs, min_run, want_individuals=want_individuals)

    def dstat(self, pops, quartets, polarize):
        """ABBA-BABA D, f4 and f_d per window and quartet (impop_dstat_scan; DSTAT records [windows, quartets]).  One process, one GPU."""
        return self.bm.dstat_scan(self.local_wins, pops, quartets, polarize=polarize)

    def sfs(self, pops, pairs, outgroup, tables, w0, w1):
        """spectrum summaries, pair classes and (tables) spectra of the rows [w0, w1) (impop_sfs_scan) -> (SFS records [rows, pops],
        SFS_PAIR records [rows, pairs], sfs or None, jsfs or None).  One process, one GPU."""
        return self.bm.sfs_scan(self.local_wins[w0:w1], pops, pairs, outgroup=outgroup, tables=tables)

    def close(self):
        for sk, ck in zip(self.slabs, self.ctxs):
            sk.free(); ck.close()
        if self.bm is not None:
            self.bm.free()
        self.ctx.close()


def write_tables(out, args, fmt, regions, L_col, col, s_all, samples_col, thr_txt, r_txt, panel_tables=None, panel_labels=None, fst_skip=(),
                 panel_taj=None):
    """the TSV tables of the reference's drivers (headers run_pica2_impg.sh:119,122 / run_h-fst.sh:148 / run_tajd.sh:101 /
    run_fst_impg.sh:158) from per-row columns; shared by the matrix path and --sim-list"""
    if args.panel:  # one table per pair (run_h_fst_panels.sh), then one per panel (run_tajd_panels.sh); nothing else
        p = 0
        K = len(args.panel)
        for k in range(K if panel_tables is not None else 0):
            for l in range(k + 1, K):
                print(f"# {panel_labels[k]}-vs-{panel_labels[l]}", file=out)
                print("REGION\tLENGTH\tFST\tPI_A\tPI_B\tPI_XY\tDXY\tDA", file=out)
                for i, reg in enumerate(regions):
                    r = panel_tables[i, p]
                    print(f"{reg}\t{L_col[i]}\t{float(r['fst']):.8f}\t{float(r['pi_a']):.8f}\t{float(r['pi_b']):.8f}\t"
                          f"{float(r['pi_xy']):.8f}\t{float(r['dxy']):.8f}\t{float(r['da']):.8f}", file=out)
                p += 1
        for k in range(K if panel_taj is not None else 0):
            print(f"# {panel_labels[k]}", file=out)
            print("REGION\tLENGTH\tSAMPLES\tSEGREGATING_SITES\tPI\tTAJIMAS_D", file=out)  # run_tajd.sh:101
            for i, reg in enumerate(regions):
                D = float(panel_taj["tajima_d"][i, k])
                taj = "NA" if D != D else repr(D)  # run_tajd.sh:192-194
                print(f"{reg}\t{L_col[i]}\t{panel_taj['samples'][k]}\t{int(panel_taj['s_all'][i])}\t{panel_taj['pi_site'][i, k]:.8f}\t{taj}", file=out)
        return
    if fmt in ("pica2", "all"):
        if args.subset:
            print("REGION\tSUBSET\tLENGTH\tTHRESHOLD\tR_VALUE\tPICA_OUTPUT", file=out)
        else:
            print("REGION\tLENGTH\tTHRESHOLD\tR_VALUE\tPICA_OUTPUT", file=out)
        for i, reg in enumerate(regions):
            cell = f"{col['pi_site'][i]:.8f} (sequence length: {L_col[i]})"  # pica2.py:226
            if args.subset:
                print(f"{reg}\t{os.path.basename(args.subset)}\t{L_col[i]}\t{thr_txt}\t{r_txt}\t{cell}", file=out)
            else:
                print(f"{reg}\t{L_col[i]}\t{thr_txt}\t{r_txt}\t{cell}", file=out)
    if fmt in ("hfst", "all") and args.pop_a and args.pop_b and not args.panel:
        print("REGION\tLENGTH\tFST\tPI_A\tPI_B\tPI_XY\tDXY\tDA", file=out)
        for i, reg in enumerate(regions):
            if i in fst_skip:  # --sim-list: a window whose table holds no member of one population
                continue
            print(f"{reg}\t{L_col[i]}\t{col['fst'][i]:.8f}\t{col['pi_a'][i]:.8f}\t{col['pi_b'][i]:.8f}\t"
                  f"{col['pi_xy'][i]:.8f}\t{col['dxy'][i]:.8f}\t{col['da'][i]:.8f}", file=out)
    if fmt == "fst3pi":
        from impop_amd.drivers import fst_3pi_fields
        print("REGION\tLENGTH\tTHRESHOLD\tR_VALUE\tPI_A\tPI_B\tPI_C\tPI_AB_AVG\tFST", file=out)  # run_fst_impg.sh:158
        for i, reg in enumerate(regions):
            ta, tb, tc, avg, fst = fst_3pi_fields(float(col["pi3_a"][i]), float(col["pi3_b"][i]), float(col["pi3_c"][i]))
            print(f"{reg}\t{L_col[i]}\t{thr_txt}\t{r_txt}\t{ta}\t{tb}\t{tc}\t{avg}\t{fst}", file=out)
    if fmt in ("tajd", "all"):
        print("REGION\tLENGTH\tSAMPLES\tSEGREGATING_SITES\tPI\tTAJIMAS_D", file=out)
        for i, reg in enumerate(regions):
            D = float(col["tajima_d"][i])
            taj = "NA" if D != D else repr(D)  # run_tajd.sh:192-194
            print(f"{reg}\t{L_col[i]}\t{samples_col}\t{int(s_all[i])}\t{col['pi_site'][i]:.8f}\t{taj}", file=out)


AF_HEADER = "REGION\tLENGTH\tTHRESHOLD\tHAPLOTYPES\tCLUSTERS\tLARGEST\tSINGLETONS\tHOMOZYGOSITY"
EHH_HEADER = "REGION\tLENGTH\tCORE\tALLELE\tREF_ALT\tN_HAPLOTYPES\tAREA\tIHH_LEFT\tIHH_RIGHT"
HAP_HEADER = "REGION\tLENGTH\tSAMPLES\tSITES\tHAPLOTYPES\tH1\tH12\tH2_H1\tHAP_DIVERSITY"
LD_HEADER = "REGION\tLENGTH\tSAMPLES\tSITES\tQUALIFYING\tUSED\tZNS\tMEAN_DPRIME\tPERFECT\tCOMPLETE\tOMEGA_MAX\tOMEGA_POS"
DIPLOID_HEADER = "CHROM\tSTART\tEND\tN_IND\tSITES\tHET_SITES\tHO\tHE\tFIS\tROH_RUNS\tF_ROH\tLONGEST_RUN"
DIPLOID_IND_HEADER = "CHROM\tSTART\tEND\tSAMPLE\tHET\tHOM_ALT\tLONGEST_RUN\tROH_RUNS\tROH_SITES"


IBS_HEADER = "REGION\tLENGTH\tPAIRS\tTRACTS\tPAIRS_SPANNING\tPAIR_SITES\tSHARE"
IBS_SEGMENT_HEADER = "seq1\tseq2\tstart\tend\tsites\topen"
IBS_PAIR_HEADER = "SEQ1\tSEQ2\tN_DIFF\tLONGEST\tTRACTS\tTRACT_SITES"


def write_ibs_table(out, regions, L_col, n_pairs, recs):
    """the table of --format ibs from impop_ibs_window records (one per region); n_pairs: the pairs of each region's matrix"""
    print(IBS_HEADER, file=out)
    for reg, L, npair, r in zip(regions, L_col, n_pairs, recs):
        print(f"{reg}\t{L}\t{int(npair)}\t{int(r['tracts'])}\t{int(r['pairs_spanning'])}\t{int(r['pair_sites'])}\t{_na(r['share'])}", file=out)


def write_ibs_segments(out, names, segs, site_bp, header=True):
    """--ibs-segments: impop_ibs_segment records as TSV; site_bp(site) = the position of a site in bp"""
    if header:
        print(IBS_SEGMENT_HEADER, file=out)
    for q in segs:
        b, e, fl = int(q["begin"]), int(q["end"]), int(q["flags"])
        print(f"{names[int(q['h1'])]}\t{names[int(q['h2'])]}\t{site_bp(b)}\t{site_bp(e - 1) + 1}\t{e - b}\t"
              f"{('L' if fl & 1 else '') + ('R' if fl & 2 else '') or '.'}", file=out)


def write_ibs_pairs(out, names, recs, header=True):
    """--ibs-pair-table: impop_ibs_pair records, one row per pair"""
    if header:
        print(IBS_PAIR_HEADER, file=out)
    for q in recs:
        print(f"{names[int(q['h1'])]}\t{names[int(q['h2'])]}\t{int(q['n_diff'])}\t{int(q['longest'])}\t{int(q['n_tracts'])}\t"
              f"{int(q['tract_sites'])}", file=out)


DSTAT_HEADER = "CHROM\tSTART\tEND\tP1\tP2\tP3\tO\tN_SITES\tN_INFORMATIVE\tN_SKIPPED\tABBA\tBABA\tD\tF4\tF_D"
DSTAT_SUMMARY_HEADER = "P1\tP2\tP3\tO\tD\tD_SE\tD_Z\tF_D\tF_D_SE\tBLOCKS\tABBA\tBABA"


def parse_quartets(specs, n_panel):
    """--quartet i,j,k,o (1-based positions in --panel, repeatable) -> [(P1, P2, P3, O)] 0-based; none given: 1,2,3,4 when the
    panel has exactly four lists.  ValueError with the message otherwise."""
    if not specs:
        if n_panel != 4:
            raise ValueError(f"--panel holds {n_panel} lists: say which four make a quartet with --quartet i,j,k,o (repeatable)")
        return [(0, 1, 2, 3)]
    out = []
    for spec in specs:
        parts = spec.split(",")
        if len(parts) != 4 or not all(x.strip().isdigit() for x in parts):
            raise ValueError(f"--quartet {spec}: four 1-based positions in --panel, as in 1,2,3,4")
        q = tuple(int(x) - 1 for x in parts)
        for k in q:
            if not 0 <= k < n_panel:
                raise ValueError(f"--quartet {spec}: position {k + 1} is outside the {n_panel} lists of --panel")
        if len(set(q)) != 4:
            raise ValueError(f"--quartet {spec}: a population is named twice")
        out.append(q)
    if len(out) > 64:
        raise ValueError("--quartet: at most 64 quartets per run")
    return out


SFS_HEADER = ("CHROM\tSTART\tEND\tPOP\tN\tN_SITES\tS\tETA1\tETA_N1\tN_SKIPPED\tTHETA_W\tTHETA_PI\tTHETA_H\tTHETA_L\tTAJIMA_D\tFAYWU_H\t"
              "FAYWU_H_NORM\tZENG_E")
SFS_PAIRS_HEADER = "CHROM\tSTART\tEND\tPOP_A\tPOP_B\tPRIVATE_A\tPRIVATE_B\tSHARED\tFIXED_A\tFIXED_B\tN_UNION"
SFS_DOUBLES = ("theta_w", "theta_pi", "theta_h", "theta_l", "tajima_d", "faywu_h", "faywu_h_norm", "zeng_e")
SFS_BATCH_ROWS = 1024  # BED rows per impop_sfs_scan call of --sfs-spectra: their tables are summed into the blocks, then dropped


def parse_sfs_pairs(specs, n_panel):
    """--sfs-pair i,j (1-based positions in --panel, repeatable) -> [(a, b)] 0-based"""
    out = []
    for spec in specs or []:
        try:
            pair = tuple(int(x) - 1 for x in spec.split(","))
        except ValueError:
            pair = ()
        if len(pair) != 2:
            raise ValueError(f"--sfs-pair {spec}: two 1-based positions in --panel, as in 1,2")
        for k in pair:
            if not 0 <= k < n_panel:
                raise ValueError(f"--sfs-pair {spec}: position {k + 1} is outside the {n_panel} lists of --panel")
        if pair[0] == pair[1]:
            raise ValueError(f"--sfs-pair {spec}: a population is named twice")
        out.append(pair)
    if len(out) > 28:
        raise ValueError("--sfs-pair: at most 28 pairs per run")
    return out


IHS_HEADER = "CHROM\tSITE\tN0\tN1\tFREQ1\tIHH0\tIHH1\tIHS\tIHS_STD\tSL0\tSL1\tNSL\tNSL_STD\tFLAGS"
XPEHH_HEADER = "CHROM\tSITE\tNA\tNB\tFREQ1_A\tFREQ1_B\tIHH_A\tIHH_B\tXPEHH\tXPEHH_STD\tSL_A\tSL_B\tXPNSL\tXPNSL_STD\tFLAGS"


def write_ihs_table(out, K, chroms, bps, rec, bins, keep_edge):
    """the table of --format ihs (K = 1) / xpehh (K = 2) from impop_ihs_core records of all rows of the run: the doubles, the scores
    standardised over all of them, one row per core; cores with an EDGE bit are left out unless keep_edge"""
    from impop_amd import ihs as ih
    v = ih.ihs_values(rec, K)
    first, second = ("ihs", "nsl") if K == 1 else ("xpehh", "xpnsl")
    freq = v["freq1"] if K == 1 else None
    std = [ih.standardize(v[first], rec["flags"], 0, freq, bins), ih.standardize(v[second], rec["flags"], 1, freq, bins)]
    num = lambda x: "NA" if x != x else f"{x:.8f}"  # noqa: E731
    print(IHS_HEADER if K == 1 else XPEHH_HEADER, file=out)
    for i, r in enumerate(rec):
        if (int(r["flags"]) & ih.EDGE_BITS) and not keep_edge:
            continue
        n0, n1 = int(r["n"][0]), int(r["n"][1])
        fr = num(v["freq1"][i]) if K == 1 else f"{int(r['c1'][0]) / n0:.8f}\t{int(r['c1'][1]) / n1:.8f}"
        print(f"{chroms[i]}\t{bps[i]}\t{n0}\t{n1}\t{fr}\t{num(v['ihh'][i, 0])}\t{num(v['ihh'][i, 1])}\t{num(v[first][i])}\t{num(std[0][i])}\t"
              f"{num(v['sl'][i, 0])}\t{num(v['sl'][i, 1])}\t{num(v[second][i])}\t{num(std[1][i])}\t{int(r['flags'])}", file=out)


def sfs_row(region, label, n, r):
    """one row of the --format sfs table: region, the population's list name and size, the record"""
    chrom, start, end = split_region(region)
    return (f"{chrom}\t{start}\t{end}\t{label}\t{int(n)}\t{int(r['n_sites'])}\t{int(r['seg'])}\t{int(r['eta1'])}\t{int(r['eta_n1'])}\t"
            f"{int(r['n_skipped'])}\t" + "\t".join(f"{float(r[f]):.8f}" for f in SFS_DOUBLES))


def sfs_pair_row(region, label_a, label_b, r):
    """one row of --sfs-pairs-out: region, the pair's list names, the six counters"""
    chrom, start, end = split_region(region)
    return f"{chrom}\t{start}\t{end}\t{label_a}\t{label_b}\t" + "\t".join(
        str(int(r[f])) for f in ("private_a", "private_b", "shared", "fixed_a", "fixed_b", "n_union"))


def write_sfs_table(out, regions, labels, sizes_rows, recs):
    """the table of --format sfs: one row per region and population from impop_sfs_stats records [regions, populations]"""
    print(SFS_HEADER, file=out)
    for reg, sizes, per_k in zip(regions, sizes_rows, recs):
        for label, n, r in zip(labels, sizes, per_k):
            print(sfs_row(reg, label, n, r), file=out)


def write_sfs_pairs(out, regions, labels, pairs, recs):
    print(SFS_PAIRS_HEADER, file=out)
    for reg, per_p in zip(regions, recs):
        for (a, b), r in zip(pairs, per_p):
            print(sfs_pair_row(reg, labels[a], labels[b], r), file=out)


def dstat_row(region, labels, quartet, sizes, r):
    """one row of the --format dstat table: region, the quartet's list names, the record; ABBA / BABA as frequencies"""
    chrom, start, end = split_region(region)
    n1, n2, n3, nO = (int(sizes[k]) for k in quartet)
    norm = float(n1 * n2 * n3 * nO)
    return (f"{chrom}\t{start}\t{end}\t" + "\t".join(labels[k] for k in quartet) + f"\t{int(r['n_sites'])}\t{int(r['n_informative'])}\t"
            f"{int(r['n_skipped'])}\t{float(int(r['abba'])) / norm:.8f}\t{float(int(r['baba'])) / norm:.8f}\t{float(r['d']):.8f}\t"
            f"{float(r['f4']):.8f}\t{float(r['fd']):.8f}")


def write_dstat_table(out, regions, labels, quartets, sizes_rows, recs):
    """the table of --format dstat: one row per region and quartet from impop_dstat_stats records [regions, quartets];
    sizes_rows[i] = the populations' sizes in the matrix of region i"""
    print(DSTAT_HEADER, file=out)
    for reg, sizes, per_q in zip(regions, sizes_rows, recs):
        for q, r in zip(quartets, per_q):
            print(dstat_row(reg, labels, q, sizes, r), file=out)


def write_dstat_summary(out, labels, quartets, sizes_rows, recs, n_blocks):
    """--dstat-summary: per quartet the genome-wide D and f_d over all regions with their block-jackknife errors
    (impop_amd.dstat.block_jackknife over n_blocks consecutive groups of regions)"""
    from impop_amd.dstat import block_jackknife
    print(DSTAT_SUMMARY_HEADER, file=out)
    for qi, q in enumerate(quartets):
        norms = [[int(sz[k]) for k in q] for sz in sizes_rows]
        abba = np.array([int(x) for x in recs["abba"][:, qi]], dtype=object)
        baba = np.array([int(x) for x in recs["baba"][:, qi]], dtype=object)
        prod = np.array([float(a * b * c * d) for a, b, c, d in norms])
        if len({tuple(x) for x in norms}) > 1:  # matrices with different population sizes: frequencies, not counts
            abba, baba = abba.astype(np.float64) / prod, baba.astype(np.float64) / prod
        d, d_se, d_z, B = block_jackknife(abba - baba, abba + baba, n_blocks)
        fd_num = (recs["abba"][:, qi] - recs["baba"][:, qi]).astype(np.float64) / prod
        fd_den = recs["fd_den_p2"][:, qi].astype(np.float64) / np.array([float(a * b * b * d) for a, b, c, d in norms]) \
            + recs["fd_den_p3"][:, qi].astype(np.float64) / np.array([float(a * c * c * d) for a, b, c, d in norms])
        fd, fd_se, _, _ = block_jackknife(fd_num, fd_den, n_blocks)
        s_abba = float(np.sum(recs["abba"][:, qi].astype(np.float64) / prod)) if len(prod) else 0.0
        s_baba = float(np.sum(recs["baba"][:, qi].astype(np.float64) / prod)) if len(prod) else 0.0
        print("\t".join(labels[k] for k in q) + f"\t{float(d):.8f}\t{float(d_se):.8f}\t{float(d_z):.8f}\t{float(fd):.8f}\t{float(fd_se):.8f}\t{B}\t"
              f"{s_abba:.8f}\t{s_baba:.8f}", file=out)


def _na(x, digits=8):
    x = float(x)
    return "NA" if x != x else f"{x:.{digits}f}"


def split_region(region):
    """'CHM13#0#chr2:100-200' -> ('CHM13#0#chr2', '100', '200')"""
    chrom, _, span = region.rpartition(":")
    start, _, end = span.partition("-")
    return chrom, start, end


def write_diploid_table(out, regions, recs):
    """the table of --format diploid from impop_diploid_stats records (one per region)"""
    print(DIPLOID_HEADER, file=out)
    for reg, r in zip(regions, recs):
        chrom, start, end = split_region(reg)
        print(f"{chrom}\t{start}\t{end}\t{int(r['n_ind'])}\t{int(r['n_sites'])}\t{int(r['het_sites'])}\t{_na(r['ho'])}\t{_na(r['he'])}\t"
              f"{_na(r['f_is'])}\t{int(r['roh_runs_total'])}\t{_na(r['f_roh'])}\t{int(r['longest_run'])}", file=out)


def write_diploid_ind_table(out, regions, samples, rows, header=True):
    """--ind-table: one row per region and sample from impop_diploid_ind rows ([regions, samples])"""
    if header:
        print(DIPLOID_IND_HEADER, file=out)
    for reg, per_sample in zip(regions, rows):
        chrom, start, end = split_region(reg)
        for name, q in zip(samples, per_sample):
            print(f"{chrom}\t{start}\t{end}\t{name}\t{int(q['het'])}\t{int(q['hom_alt'])}\t{int(q['longest_run'])}\t{int(q['roh_runs'])}\t"
                  f"{int(q['roh_sites'])}", file=out)


def ld_min_mac(min_maf, n_members):
    """--ld-min-maf F among n_members sequences as the min_mac of impop_ld_scan"""
    return max(1, int(math.ceil(min_maf * n_members)))


def write_ld_table(out, regions, L_col, recs, omega_pos):
    """the table of --format ld from impop_ld_stats records (one per region); omega_pos: the position of used site omega_split, or None"""
    print(LD_HEADER, file=out)
    for reg, L, r, pos in zip(regions, L_col, recs, omega_pos):
        print(f"{reg}\t{L}\t{int(r['n_members'])}\t{int(r['n_sites'])}\t{int(r['n_qualifying'])}\t{int(r['n_used'])}\t{float(r['zns']):.8f}\t"
              f"{float(r['mean_dprime']):.8f}\t{int(r['n_perfect'])}\t{int(r['n_complete'])}\t{float(r['omega_max']):.8f}\t"
              f"{'NA' if pos is None else pos}", file=out)


def write_hap_table(out, regions, L_col, recs):
    """the table of --format hapstats from impop_haplotype_stats records (one per region)"""
    print(HAP_HEADER, file=out)
    for reg, L, r in zip(regions, L_col, recs):
        print(f"{reg}\t{L}\t{int(r['n_members'])}\t{int(r['n_sites'])}\t{int(r['n_distinct'])}\t{float(r['h1']):.8f}\t{float(r['h12']):.8f}\t"
              f"{float(r['h2_h1']):.8f}\t{float(r['hap_diversity']):.8f}", file=out)


def milli_text(k):
    """exact thousandths as text: 12276 -> '12.276'"""
    k = int(k)
    return f"{k // 1000}.{k % 1000:03d}"


def ehh_rows(region, length, core_bp, rec):
    """the rows of --format ehh for one impop_ehh_stats record: one per allele present"""
    out = []
    for al in (0, 1):
        n = int(rec["n_members"][al])
        if n:
            left, right = int(rec["area_milli"][al][0]), int(rec["area_milli"][al][1])
            out.append(f"{region}\t{length}\t{core_bp}\t{al}\t{'REF' if al == int(rec['ref_allele']) else 'ALT'}\t{n}\t"
                       f"{milli_text(left + right)}\t{milli_text(left)}\t{milli_text(right)}")
    return out


def read_core_positions(path):
    with open(path) as f:
        return [int(line.split()[0]) for line in f if line.strip() and not line.lstrip().startswith("#")]


def write_af_table(out, regions, L_col, thr_txt, recs):
    """the main table of --format af from impop_cluster_stats records (one per region)"""
    print(AF_HEADER, file=out)
    for reg, L, r in zip(regions, L_col, recs):
        n, sq = int(r["n_members"]), int(r["sum_sq"])
        hom = sq / (n * n) if n else 0.0
        print(f"{reg}\t{L}\t{thr_txt}\t{n}\t{int(r['n_clusters'])}\t{int(r['largest'])}\t{int(r['n_singletons'])}\t{hom:.6f}", file=out)


def write_af_clusters(handle, regions, clusters_per_region, header=True):
    """REGION + the rows of af.write_summary (af.py:56-60: cluster_id, count, "%.6f" frequency; csv-module line endings)"""
    import csv
    from impop_amd.af import build_summary
    w = csv.writer(handle, delimiter="\t")
    if header:
        w.writerow(("REGION", "cluster_id", "count", "frequency"))
    for reg, clusters in zip(regions, clusters_per_region):
        w.writerows([(reg, cid, size, f"{freq:.6f}") for cid, size, freq, _ in build_summary(clusters)])


def write_af_details(handle, regions, clusters_per_region, threshold, header=True):
    """REGION + the rows of af.write_details (af.py:62-68: sample_id, cluster_id, threshold)"""
    import csv
    from impop_amd.af import build_summary
    w = csv.writer(handle, delimiter="\t")
    if header:
        w.writerow(("REGION", "sample_id", "cluster_id", "threshold"))
    for reg, clusters in zip(regions, clusters_per_region):
        w.writerows([(reg, sample, cid, threshold) for cid, _, _, members in build_summary(clusters) for sample in members])


def sim_list_refusal(args):
    """what --sim-list does not combine with (one line each, exit 2, before any device is opened)"""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        return "--sim-list is a one-process, one-GPU driver: not under torch.distributed.run"
    if args.devices > 1:
        return "--sim-list runs on one GPU: not with --devices N"
    if args.panel:
        return "--sim-list has no --panel (the K-population scan streams a presence matrix)"
    if args.compact:
        return "--sim-list has no --compact (there is no presence matrix to compact)"
    if args.fst_method == "grouped":
        return "--sim-list computes the direct h-fst table: not with --fst-method grouped"
    if args.format == "fst3pi":
        return "--sim-list formats are pica2, hfst, tajd and all"
    if args.format == "hfst" and not (args.pop_a and args.pop_b):
        return "--format hfst needs -A and -B"
    if args.format in ("tajd", "all") and not args.sample_list:
        return "--sim-list --format tajd / all needs -l samples.txt (SAMPLE_COUNT, run_tajd.sh:83)"
    if args.sequence_length is not None and (args.format != "pica2" or args.sequence_length <= 0):
        return "--sequence-length (a positive integer) belongs to --format pica2 (run_pica2_impg.sh -l)"
    return None


def scan_sim_list(args, fmt, pica_t, pica_r, fst_r, thr_txt, r_txt):
    """--sim-list: every window's own `.sim` table through impop_stats_from_identity_batch (impop_amd.simbatch)"""
    from impop_amd import simbatch
    rows = simbatch.read_sim_list(args.sim_list, fmt)
    want_pica, want_fst, want_d = fmt in ("pica2", "tajd", "all"), fmt in ("hfst", "all") and bool(args.pop_a and args.pop_b), \
        fmt in ("tajd", "all")
    if want_d:
        for row in rows:
            try:
                ok = row.S is not None and float(row.S) >= 0
            except ValueError:
                ok = False
            if not ok:
                fail(f"--format {fmt} with --sim-list needs a non-negative S column (row {row.chrom}:{row.start}-{row.end})")
    sample_count = None
    if args.sample_list:
        sample_count = awk_line_count(args.sample_list)  # run_tajd.sh:83
        if want_d and sample_count < 2:
            fail(f"Need at least two samples to compute Tajima's D (found {sample_count})", 1)  # :84-87
    pops, no_fst = None, set()
    NO_POP = "Error: No valid sequences found in one or both populations"
    if want_fst:
        pops = [simbatch.PopulationFlags(read_subset_file(f)) for f in (args.pop_a, args.pop_b)]

    def full_name(chrom):
        return chrom if chrom.startswith(args.region_prefix) else args.region_prefix + chrom

    def length_of(row):
        return args.sequence_length if args.sequence_length is not None else row.end - row.start

    def make_problem(row, tab):
        pr = {"ident": tab.dense, "seq_len": length_of(row)}
        if want_pica:
            pr["seed_rank"] = simbatch.seed_rank(tab)
        if want_fst:
            (fa, miss_a), (fb, miss_b) = pops[0](tab.names), pops[1](tab.names)
            for tag, miss in (("A", miss_a), ("B", miss_b)):  # per window, as the per-window script prints them
                if miss:
                    print(f"Warning: {miss} identifiers from population {tag} did not match any sequences", file=sys.stderr)
            both = int((fa & fb).sum())
            if both:
                print(f"Warning: {both} sequences appear in both populations", file=sys.stderr)  # h-fst.py:181-185
            if not fa.any() or not fb.any():  # h-fst.py:319-321
                if fmt == "hfst":
                    return simbatch.SimFailure(NO_POP)
                no_fst.add((row.chrom, row.start, row.end))  # --format all: only the h-fst table loses the window
            else:
                pr["in_a"], pr["in_b"] = fa, fb
        if want_d:
            pr["tajima_n"], pr["tajima_S"] = sample_count, float(row.S)
        return pr

    ctx = impop_amd.Context(args.device)
    flavor = "hfst" if fmt == "hfst" else "pica2"
    results = simbatch.run_pipeline(ctx, rows, flavor, make_problem, pica_t, pica_r, fst_r, n_threads=args.sim_threads)
    ctx.close()
    kept = []
    for row, res in zip(rows, results):
        region = f"{full_name(row.chrom)}:{row.start}-{row.end}"
        if res[0] == "ok":
            kept.append((region, row, res[1]))
            continue
        # the reference drivers' stderr lines: run_pica2_impg.sh:174-176, run_h-fst.sh:83-84, run_tajd.sh:166-167
        if fmt == "hfst":
            print(res[1], file=sys.stderr)
            print(f"Error: FST calculation failed for region {region}", file=sys.stderr)
        elif fmt == "pica2":
            print(f"Error: pica2.py failed for region {region}", file=sys.stderr)
            print(res[1], file=sys.stderr)
        else:
            print(f"Warning: pica2.py failed for region {region}", file=sys.stderr)
    n_rows = len(kept)
    col = {k: np.full(n_rows, np.nan) for k in ("pi_site", "tajima_d", "fst", "pi_a", "pi_b", "pi_xy", "dxy", "da")}
    s_all = np.zeros(n_rows, dtype=np.int64)
    L_col = np.array([length_of(row) for _, row, _ in kept], dtype=np.int64)
    for i, (_, row, rec) in enumerate(kept):
        col["pi_site"][i], col["tajima_d"][i] = rec["pi_site"], rec["tajima_d"]
        for j, k in enumerate(("fst", "pi_a", "pi_b", "pi_xy", "dxy", "da")):
            col[k][i] = rec["fst"][j]
        if want_d:
            s_all[i] = int(float(row.S))
    out = open(args.output, "w") if args.output else sys.stdout
    fst_skip = set()
    for i, (region, row, _) in enumerate(kept):
        if (row.chrom, row.start, row.end) in no_fst:  # run_h-fst.sh:83-84, behind h-fst.py's own line
            print(NO_POP, file=sys.stderr)
            print(f"Error: FST calculation failed for region {region}", file=sys.stderr)
            fst_skip.add(i)
    write_tables(out, args, fmt, [k[0] for k in kept], L_col, col, s_all, sample_count if sample_count is not None else 0, thr_txt, r_txt,
                 fst_skip=fst_skip)
    if args.output:
        out.close()


def fail(message, code=2):
    print(f"Error: {message}", file=sys.stderr)
    sys.exit(code)


def panel_labels(args):
    """the --panel lists' base names, as the tables print them"""
    return [os.path.splitext(os.path.basename(f))[0] for f in args.panel]


def site_bp(mf):
    """site index -> position in bp on the matrix's contig"""
    return (lambda c: int(mf.site_pos[c])) if mf.site_pos is not None else (lambda c: int(mf.origin + c))


def pair_samples(fmt, names, mask_p, min_samples):
    """the sequences of mask_p (None: all) paired into samples by their PanSN fields -> (pairs, sample names); the sequences left
    out are named in one warning, fewer than min_samples (1 or 2) paired samples end the run"""
    from impop_amd.popnames import pair_haplotypes
    chosen = None if mask_p is None else [nm for nm, f in zip(names, mask_p) if f]
    pairs, samples, unpaired = pair_haplotypes(list(names), chosen)
    if unpaired:
        print(f"Warning: --format {fmt}: {len(unpaired)} sequences are not one of a sample's two haplotypes and are left out: "
              + " ".join(unpaired), file=sys.stderr)
    if len(pairs) < min_samples:
        few = "no sample with both of its haplotypes" if min_samples == 1 else "fewer than two samples with both of their haplotypes"
        fail(f"--format {fmt}: {few} (sample#1#..., sample#2#...) among the sequences")
    return pairs, samples


def check_lists(fmt, labels, pops, groups, disjoint):
    """what a --panel scan would refuse, with the lists' names.  groups: [(lists that must select a sequence, pairs of lists that
    must not share one)], checked group by group; disjoint: the format's words behind `share a sequence; `"""
    for need, pairs in groups:
        for k in need:
            if not pops[k].any():
                fail(f"--format {fmt}: {labels[k]} selects no sequence of the matrix")
        for a, b in pairs:
            if (pops[a] & pops[b]).any():
                fail(f"--format {fmt}: {labels[a]} and {labels[b]} share a sequence; {disjoint}")


def pica_params(args):
    """-> (threshold, round digits) behind the pica2-derived columns and the THRESHOLD / R_VALUE texts"""
    if args.format in ("tajd", "all"):  # run_tajd.sh:9-10
        pica_t = 0.999 if args.threshold is None else args.threshold
        pica_r = 5 if args.round_digits is None else (None if args.round_digits == "none" else args.round_digits)
    else:
        pica_t = 1.0 if args.threshold is None else args.threshold
        pica_r = None if args.round_digits in (None, "none") else args.round_digits
    thr_txt = args.threshold_text if args.threshold_text is not None else repr(float(pica_t))  # as typed, like "${THRESHOLD}" in the drivers
    return pica_t, pica_r, thr_txt, "" if pica_r is None else str(pica_r)


class Job:
    """The front end of every matrix-path format: the matrices keyed by contig, the usable BED rows with their region text and the
    rows grouped per matrix (BED rows are matched to matrices by chromosome), and the one way through a matrix: windows -> Runner
    -> scan -> close."""

    def __init__(self, args, rank=0, world=1, local_rank=0):
        self.args, self.rank, self.world, self.local_rank = args, rank, world, local_rank

        def full_name(chrom):
            return chrom if chrom.startswith(args.region_prefix) else args.region_prefix + chrom
        self.mats = {}
        for p in args.matrix:
            mf = load_matrix(p)
            key = full_name(mf.contig) if mf.contig else ""
            if key in self.mats:
                fail(f"two matrices for contig '{mf.contig}' ({p})")
            self.mats[key] = mf
        if "" in self.mats and len(self.mats) > 1:
            fail("several --matrix files need a contig name each (matrixio `contig`)")
        bed = read_bed(args.bed, args.format)
        self.ehh_cores = read_core_positions(args.ehh_cores) if args.ehh_cores else None  # one per usable BED row: see row_bed
        if self.ehh_cores is not None and len(self.ehh_cores) != len(bed):
            fail(f"--ehh-cores holds {len(self.ehh_cores)} positions for {len(bed)} BED rows")
        # rows[i] = (region, key of its matrix, start, end); row_bed[i] = index of row i among the usable BED rows
        self.rows, self.per_mat, self.row_bed = [], {}, []
        for bed_no, (chrom, s, e) in enumerate(bed):
            region = f"{full_name(chrom)}:{s}-{e}"
            key = "" if "" in self.mats else full_name(chrom)
            if key not in self.mats:
                print(f"Warning: Skipping region {region}: no matrix holds chromosome {chrom}", file=sys.stderr)
                continue
            self.per_mat.setdefault(key, []).append(len(self.rows))
            self.rows.append((region, key, s, e))
            self.row_bed.append(bed_no)
        self.n_rows = len(self.rows)
        self.regions = [r[0] for r in self.rows]
        self.L_col = np.array([e - s for _, _, s, e in self.rows], dtype=np.int64)  # LENGTH = end - start (run_pica2_impg.sh:133)

    def matrices(self):
        """per matrix, in the order of each matrix's first BED row: (key, matrix, the indices of its rows, their windows)"""
        for key, idx in self.per_mat.items():
            mf = self.mats[key]
            yield key, mf, np.array(idx), [mf.site_range(self.rows[i][2], self.rows[i][3]) + (int(self.L_col[i]),) for i in idx]

    @contextlib.contextmanager
    def upload(self, mf, wins, need_pairs):
        """the matrix on the device(s) with its windows; closed on every way out"""
        run = Runner(self.args, mf, wins, need_pairs, self.rank, self.world, self.local_rank)
        try:
            yield run
        finally:
            run.close()

    def subset_mask(self, mf):
        return flags_for(self.args.subset, mf.names) if self.args.subset else None

    def open_output(self):
        return (open(self.args.output, "w") if self.args.output else sys.stdout) if self.rank == 0 else open(os.devnull, "w")

    def close_output(self, out):
        if self.args.output or self.rank != 0:
            out.close()


def print_rows(handle, table):
    if handle:
        for row in table:
            print("\t".join(row), file=handle)


def scan_af(args, job):
    """--format af: the main table to --output / stdout, --af-clusters / --af-details to their paths"""
    from impop_amd.af import _sample_of, clusters_from_ranks
    pica_t, pica_r, thr_txt, _ = pica_params(args)
    want_members = bool(args.af_clusters or args.af_details)
    out = job.open_output()
    recs = np.zeros(job.n_rows, dtype=impop_amd.CLUSTER_DTYPE)
    clusters = [None] * job.n_rows
    for _, mf, idx, wins in job.matrices():
        mask_p = job.subset_mask(mf)
        members = [_sample_of(mf.names[i]) for i in (range(mf.n_hap) if mask_p is None else np.flatnonzero(mask_p))]
        if len(set(members)) != len(members):
            # af.py names its nodes by the cut name, so two sequences of one name would be ONE sample there, while the
            # records count sequences: the main table and the side tables of one run would disagree
            dup = sorted({m for m in members if members.count(m) > 1})[0]
            fail(f"--format af needs distinct sequence names before the first ':' ('{dup}' names several rows of the matrix)")
        with job.upload(mf, wins, True) as run:
            res = run.bm.cluster_scan(run.local_wins, mask_p=mask_p, kind=args.identity, threshold=pica_t, round_digits=pica_r,
                                      want_members=want_members)
        if want_members:
            recs[idx] = res[0]
            for i, row in zip(idx, res[1]):
                clusters[i] = clusters_from_ranks(row, members)
        else:
            recs[idx] = res
    write_af_table(out, job.regions, job.L_col, thr_txt, recs)
    if args.af_clusters:
        with open(args.af_clusters, "w", newline="") as fh:
            write_af_clusters(fh, job.regions, clusters)
    if args.af_details:
        with open(args.af_details, "w", newline="") as fh:
            write_af_details(fh, job.regions, clusters, float(pica_t))
    job.close_output(out)


def scan_ehh(args, job):
    """--format ehh: one core per BED row; cores and the reference sequence are checked before the matrix goes up"""
    out = job.open_output()
    lines = [None] * job.n_rows
    for _, mf, idx, wins in job.matrices():
        cores = []
        for i, (b, en, _) in zip(idx, wins):
            if job.ehh_cores is not None:
                c = mf.site_range(job.ehh_cores[job.row_bed[i]], job.ehh_cores[job.row_bed[i]])[0]
            else:
                c = b + ((en - b) // 2 if args.ehh_core_offset is None else args.ehh_core_offset)
            if not b <= c < en:
                fail(f"--format ehh: the core of {job.regions[i]} (site {c}) is outside the window's sites [{b}, {en})")
            cores.append(c)
        ref_hap = 0
        if args.ehh_ref is not None:
            if args.ehh_ref not in mf.names:
                fail(f"--ehh-ref {args.ehh_ref} is not a sequence of the matrix")
            ref_hap = list(mf.names).index(args.ehh_ref)
        with job.upload(mf, wins, False) as run:
            recs = run.bm.ehh_scan([(b, en) for b, en, _ in wins], cores, mask=job.subset_mask(mf), ref_hap=ref_hap,
                                   flanks=args.ehh_flanks or "reference")
        bp = site_bp(mf)
        for i, c, r in zip(idx, cores, recs):
            lines[i] = ehh_rows(job.regions[i], int(job.L_col[i]), bp(c), r)
    print(EHH_HEADER, file=out)
    for rows in lines:
        for line in rows:
            print(line, file=out)
    job.close_output(out)


def scan_hapstats(args, job):
    """--format hapstats: one row per BED row"""
    out = job.open_output()
    recs = np.zeros(job.n_rows, dtype=impop_amd.HAPLOTYPE_DTYPE)
    for _, mf, idx, wins in job.matrices():
        mask_p = job.subset_mask(mf)
        if mask_p is not None and not mask_p.any():
            fail("--format hapstats: -u selects no sequence of the matrix")
        with job.upload(mf, wins, False) as run:
            recs[idx] = run.hapstats(mask_p)
    write_hap_table(out, job.regions, job.L_col, recs)
    job.close_output(out)


def scan_ld(args, job):
    """--format ld: one row per BED row; OMEGA_POS is the position of the first used site right of the best split"""
    out = job.open_output()
    recs = np.zeros(job.n_rows, dtype=impop_amd.LD_DTYPE)
    omega_pos = [None] * job.n_rows
    for _, mf, idx, wins in job.matrices():
        mask_p = job.subset_mask(mf)
        if mask_p is not None and not mask_p.any():
            fail("--format ld: -u selects no sequence of the matrix")
        n_matched = mf.n_hap if mask_p is None else int(mask_p.sum())
        with job.upload(mf, wins, False) as run:
            got, used = run.ld(mask_p, ld_min_mac(0.05 if args.ld_min_maf is None else args.ld_min_maf, n_matched), args.ld_max_sites or 512)
        recs[idx] = got
        bp = site_bp(mf)
        for i, r, u in zip(idx, got, used):
            if r["omega_split"]:
                omega_pos[i] = bp(int(u[int(r["omega_split"])]))
    write_ld_table(out, job.regions, job.L_col, recs, omega_pos)
    job.close_output(out)


def scan_diploid(args, job):
    """--format diploid: one row per BED row, --ind-table one per row and sample"""
    out = job.open_output()
    recs = np.zeros(job.n_rows, dtype=impop_amd.DIPLOID_DTYPE)
    ind = [None] * job.n_rows  # per row: (sample names, impop_diploid_ind rows)
    min_run = 50 if args.roh_min_sites is None else args.roh_min_sites
    for _, mf, idx, wins in job.matrices():
        pairs, samples = pair_samples("diploid", mf.names, job.subset_mask(mf), 1)
        with job.upload(mf, wins, False) as run:
            if args.ind_table:
                recs[idx], ind_rows = run.diploid(pairs, min_run, True)
                for i, q in zip(idx, ind_rows):
                    ind[i] = (samples, q)
            else:
                recs[idx] = run.diploid(pairs, min_run, False)
    write_diploid_table(out, job.regions, recs)
    if args.ind_table:
        with open(args.ind_table, "w") as fh:
            print(DIPLOID_IND_HEADER, file=fh)
            for reg, entry in zip(job.regions, ind):
                write_diploid_ind_table(fh, [reg], entry[0], [entry[1]], header=False)
    job.close_output(out)


def scan_ibs(args, job):
    """--format ibs: all BED rows of a matrix in one call over its whole site range; the segment list and the pair table are
    written matrix by matrix"""
    out = job.open_output()
    seg_fh = open(args.ibs_segments, "w") if args.ibs_segments else None
    pair_fh = open(args.ibs_pair_table, "w") if args.ibs_pair_table else None
    if seg_fh:
        print(IBS_SEGMENT_HEADER, file=seg_fh)
    if pair_fh:
        print(IBS_PAIR_HEADER, file=pair_fh)
    recs = np.zeros(job.n_rows, dtype=impop_amd.IBS_WINDOW_DTYPE)
    n_pairs = np.zeros(job.n_rows, dtype=np.int64)
    for _, mf, idx, wins in job.matrices():
        mask_p = job.subset_mask(mf)
        kw = dict(min_sites=50 if args.ibs_min_sites is None else args.ibs_min_sites, windows=[(b, en) for b, en, _ in wins],
                  want_segments=seg_fh is not None)
        if (args.ibs_pairs or "all") == "diploid":
            kw["pairs"], _ = pair_samples("ibs", mf.names, mask_p, 1)
        else:
            n_matched = mf.n_hap if mask_p is None else int(mask_p.sum())
            if n_matched < 2:
                fail(f"--format ibs: {n_matched} sequences make no pair")
            kw["mask_p"] = mask_p
        with job.upload(mf, wins, False) as run:
            prec, segs, recs[idx], _ = run.bm.ibs_scan(**kw)
        n_pairs[idx] = len(prec)
        if seg_fh:
            write_ibs_segments(seg_fh, mf.names, segs, site_bp(mf), header=False)
        if pair_fh:
            write_ibs_pairs(pair_fh, mf.names, prec, header=False)
    write_ibs_table(out, job.regions, job.L_col, n_pairs, recs)
    for fh in (seg_fh, pair_fh):
        if fh:
            fh.close()
    job.close_output(out)


def scan_dstat(args, job):
    """--format dstat: one row per BED row and quartet, --dstat-summary the block jackknife over all rows"""
    quartets = parse_quartets(args.quartet, len(args.panel))
    labels = panel_labels(args)
    out = job.open_output()
    recs = np.zeros((job.n_rows, len(quartets)), dtype=impop_amd.DSTAT_DTYPE)
    sizes_rows = [None] * job.n_rows  # per row: the populations' sizes in its matrix
    for _, mf, idx, wins in job.matrices():
        pops = [flags_for(f, mf.names) for f in args.panel]
        check_lists("dstat", labels, pops, [(q, [(a, b) for i, a in enumerate(q) for b in q[i + 1:]]) for q in quartets],
                    "the four populations of a quartet must be disjoint")
        with job.upload(mf, wins, False) as run:
            recs[idx] = run.dstat(pops, quartets, bool(args.dstat_polarize))
        for i in idx:
            sizes_rows[i] = [int(p.sum()) for p in pops]
    write_dstat_table(out, job.regions, labels, quartets, sizes_rows, recs)
    if args.dstat_summary:
        with open(args.dstat_summary, "w") as fh:
            write_dstat_summary(fh, labels, quartets, sizes_rows, recs, args.dstat_blocks)
    job.close_output(out)


def scan_sfs(args, job):
    """--format sfs: one row per BED row and population, --sfs-pairs-out one per row and pair, --sfs-spectra the spectra summed
    over --sfs-blocks consecutive groups of rows (scanned in batches of SFS_BATCH_ROWS rows)"""
    from impop_amd.distributed import shard_range
    pairs = parse_sfs_pairs(args.sfs_pair, len(args.panel))
    labels = panel_labels(args)
    out = job.open_output()
    recs = np.zeros((job.n_rows, len(args.panel)), dtype=impop_amd.SFS_DTYPE)
    pair_recs = np.zeros((job.n_rows, len(pairs)), dtype=impop_amd.SFS_PAIR_DTYPE)
    sizes_rows = [None] * job.n_rows
    n_blocks = args.sfs_blocks or 1
    blocks, block_of = None, np.zeros(job.n_rows, dtype=np.int64)  # --sfs-spectra: name -> [blocks, bins...] sums; the block of every row
    for j in range(n_blocks):
        lo, hi = shard_range(job.n_rows, n_blocks, j)
        block_of[lo:hi] = j
    tables = (("sfs",) + (("jsfs",) if pairs else ())) if args.sfs_spectra else ()
    for key, mf, idx, wins in job.matrices():
        pops = [flags_for(f, mf.names) for f in args.panel]
        check_lists("sfs", labels, pops, [(range(len(pops)), pairs)], "the two populations of a pair must be disjoint")
        outgroup = None if args.sfs_outgroup is None else args.sfs_outgroup - 1
        batch = SFS_BATCH_ROWS if tables else max(len(idx), 1)
        with job.upload(mf, wins, False) as run:
            for w0 in range(0, len(idx), batch):
                part = idx[w0:w0 + batch]
                recs[part], pr, sfs, jsfs = run.sfs(pops, pairs, outgroup, tables, w0, w0 + len(part))
                if pairs:
                    pair_recs[part] = pr
                if tables:
                    named = [(f"sfs_{labels[k]}", t) for k, t in enumerate(sfs)]
                    named += [(f"jsfs_{labels[a]}_{labels[b]}", t) for (a, b), t in zip(pairs, jsfs or [])]
                    if blocks is None:
                        blocks = {nm: np.zeros((n_blocks,) + t.shape[1:], dtype=np.uint64) for nm, t in named}
                    for nm, t in named:
                        if blocks[nm].shape[1:] != t.shape[1:]:
                            fail(f"--sfs-spectra: {nm} has another shape in the matrix of {key or 'the run'} (the lists select another "
                                 "number of its sequences); write the spectra per matrix")
                        np.add.at(blocks[nm], block_of[part], t.astype(np.uint64))
        for i in idx:
            sizes_rows[i] = [int(p.sum()) for p in pops]
    write_sfs_table(out, job.regions, labels, sizes_rows, recs)
    if args.sfs_pairs_out:
        with open(args.sfs_pairs_out, "w") as fh:
            write_sfs_pairs(fh, job.regions, labels, pairs, pair_recs)
    if args.sfs_spectra:
        np.savez(args.sfs_spectra, **(blocks or {}))
    job.close_output(out)


def scan_pairdist(args, job):
    """--format pairdist: the main table to --output / stdout, the side tables to their paths; the rows are written matrix by matrix"""
    from impop_amd import pairdist as pd
    labels = panel_labels(args)
    og = None if args.pairdist_outgroup is None else args.pairdist_outgroup - 1
    out = job.open_output()
    pan_fh = open(args.pairdist_panels, "w") if args.pairdist_panels else None
    hist_fh = open(args.pairdist_hist, "w") if args.pairdist_hist else None
    print("\t".join(pd.MAIN_COLUMNS + (["RNDMIN"] if og is not None else [])), file=out)
    print_rows(pan_fh, [pd.PANEL_COLUMNS])
    print_rows(hist_fh, [pd.HIST_COLUMNS])
    for _, mf, idx, wins in job.matrices():
        pops = [flags_for(f, mf.names) for f in args.panel]
        check_lists("pairdist", labels, pops, [((k,), [(l, k) for l in range(k)]) for k in range(len(pops))], "the lists must be disjoint")
        with job.upload(mf, wins, True) as run:
            panels, pairs, hw, hb = run.bm.pairdist_scan(run.local_wins, pops, hist_bins=args.pairdist_bins or 0, hist_width=args.pairdist_bin_width or 1)
        main, pan, hist = pd.tables([job.regions[i] for i in idx], [int(job.L_col[i]) for i in idx], labels, list(mf.names), panels, pairs,
                                    hw, hb, outgroup=og)
        for fh, table in ((out, main), (pan_fh, pan), (hist_fh, hist)):
            print_rows(fh, table)
    for fh in (pan_fh, hist_fh):
        if fh:
            fh.close()
    job.close_output(out)


def scan_kinship(args, job):
    """--format kinship: one row per BED row to --output / stdout, the per-pair totals and the watch rows to their paths; the rows
    are written matrix by matrix"""
    from impop_amd import kinship as kin
    frac = kin.threshold_fraction(0.0884 if args.kin_threshold is None else args.kin_threshold)
    out = job.open_output()
    watch_fh = open(args.kin_watch_table, "w") if args.kin_watch_table else None
    print("\t".join(kin.WINDOW_COLUMNS), file=out)
    print_rows(watch_fh, [kin.WATCH_COLUMNS])
    samples, totals = None, None
    for key, mf, idx, wins in job.matrices():
        if mf.site_weight is not None:
            fail("--format kinship: the matrix has site weights; a genotype is read per column")
        pairs, smp = pair_samples("kinship", mf.names, job.subset_mask(mf), 2)
        if samples is not None and list(smp) != samples:
            fail(f"--format kinship: the matrix of {key} pairs other samples than the one before it; the per-pair totals need one set of samples")
        samples = list(smp)
        watch = []
        for spec in args.kin_watch or []:
            a, b = spec.split(",")
            if a not in samples or b not in samples:
                fail(f"--kin-watch {spec}: {a if a not in samples else b} is not one of the paired samples")
            watch.append((samples.index(a), samples.index(b)))
        with job.upload(mf, wins, False) as run:
            g = run.bm.genotypes(pairs)
            try:
                recs, ptot, wrows = g.kinship_scan(run.local_wins, kin=frac, watch=watch or None, want_pairs=args.kin_pairs is not None)
            finally:
                g.free()
        if ptot is not None:  # integer sums on the host, over all rows and all matrices
            t = [[int(x) for x in rec] for rec in ptot["t"]]
            totals = t if totals is None else [[a + b for a, b in zip(ra, rb)] for ra, rb in zip(totals, t)]
        main, _, wat = kin.tables([job.regions[i] for i in idx], [int(job.L_col[i]) for i in idx], samples, recs, None, watch, wrows)
        print_rows(out, main)
        print_rows(watch_fh, wat)
    if args.kin_pairs:
        with open(args.kin_pairs, "w") as fh:
            print_rows(fh, [kin.PAIR_COLUMNS])
            if totals is not None:
                print_rows(fh, kin.tables([], [], samples, [], totals)[1])
    if watch_fh:
        watch_fh.close()
    job.close_output(out)


def scan_ihs(args, job):
    """--format ihs / xpehh: one impop_ihs_scan per BED row over its contig's whole matrix, the row's sites as cores; the scores are
    standardised over all rows of the run (grouped by matrix) and the table goes to --output / stdout"""
    from impop_amd import ihs as ih
    K = 2 if args.format == "xpehh" else 1
    maf = 0.05 if args.ihs_min_maf is None else args.ihs_min_maf
    cutoff_milli = int(round(1000 * (0.05 if args.ihs_cutoff is None else args.ihs_cutoff)))
    max_bp = 1000000 if args.ihs_max_extend is None else args.ihs_max_extend
    max_sites = 100 if args.ihs_max_extend_sites is None else args.ihs_max_extend_sites
    chroms, bps, recs = [], [], []
    for _, mf, idx, wins in job.matrices():
        if K == 2:
            pops = [flags_for(f, mf.names) for f in args.panel]
            if (pops[0] & pops[1]).any():
                fail("--format xpehh: the two lists of --panel share a sequence; they must be disjoint")
            if min(int(p.sum()) for p in pops) < 2:
                fail("--format xpehh: each list of --panel needs at least two sequences of the matrix")
            n_members = int(pops[0].sum() + pops[1].sum())
        else:
            pops = [job.subset_mask(mf), None]
            n_members = mf.n_hap if pops[0] is None else int(pops[0].sum())
            if n_members < 2:
                fail(f"--format ihs: {n_members} sequences make no pair")
        bp = site_bp(mf)
        with job.upload(mf, wins, False) as run:
            for i, (b, en, _) in zip(idx, wins):
                if en <= b:
                    continue
                rec, _ = run.bm.ihs_scan(mask_a=pops[0], mask_b=pops[1], core_begin=b, core_end=en, min_mac=max(1, math.ceil(maf * n_members)),
                                         cutoff_milli=cutoff_milli, max_extend_bp=max_bp, max_extend_sites=max_sites)
                recs.append(rec)
                chroms += [split_region(job.regions[i])[0]] * len(rec)
                bps += [bp(int(c)) for c in rec["site"]]
    out = job.open_output()
    write_ihs_table(out, K, chroms, bps, np.concatenate(recs) if recs else np.zeros(0, dtype=ih.IHS_DTYPE),
                    50 if args.ihs_bins is None else args.ihs_bins, args.ihs_keep_edge)
    job.close_output(out)


def classic_plan(args, rank, world, local_rank):
    """pica2 / hfst / tajd / fst3pi / all: the checks between the refusals and the first file read, in their order, the process group
    of a torch.distributed launch, and what is computed: (threshold, round digits) behind the pica2-derived columns, the round digits
    of the h-fst table, which tables need the all-pairs path"""
    fmt = args.format
    # --panel on the all-pairs path (impop_pairwise_scan_panel) is the one-process form: refused before any rank waits for another
    panel_allpairs = bool(args.panel) and (fmt in ("tajd", "all") or args.round_digits not in (None, "none") or args.identity != "match")
    if panel_allpairs and world > 1:
        fail("--panel with --format tajd / all, -r N or --identity dice runs on one GPU (impop_pairwise_scan_panel has no sharded "
             "form): not under torch.distributed.run")
    if args.panel and args.fst_method == "grouped":
        fail("--panel has no --fst-method grouped (the panel calls are the direct method; use -A / -B per pair)")
    if args.panel and fmt in ("tajd", "all") and args.sample_list:
        fail("--panel with --format tajd / all takes every panel's list as its sample list: not with -l")
    if args.panel and not 2 <= len(args.panel) <= 8:
        fail("--panel takes 2 to 8 population lists")
    if world > 1:
        import torch
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)
    if args.devices > 1 and (world > 1 or args.panel or args.compact):
        fail("--devices N is the one-process form: not under torch.distributed.run, not with --panel / --compact")
    p = SimpleNamespace(grouped_fst=fmt == "hfst" and args.fst_method == "grouped")
    p.pica_t, p.pica_r, p.thr_txt, p.r_txt = pica_params(args)
    if fmt == "hfst":
        p.fst_r = None if args.round_digits in (None, "none") else args.round_digits
        if args.threshold is not None and not p.grouped_fst:
            fail("--format hfst takes -t only with --fst-method grouped (h-fst.py has no threshold)")
    else:
        p.fst_r = None if args.fst_round_digits in (None, "none") else args.fst_round_digits
    if args.fst_round_digits is not None and fmt != "all":
        fail("--fst-round-digits belongs to --format all (use -r with --format hfst)")
    p.grouped_t = 0.999 if args.threshold is None else args.threshold  # hud.py -t
    p.pica_pairs = not (p.pica_t >= 1.0 and p.pica_r is None and args.identity == "match")
    p.fst_pairs = p.grouped_fst or p.fst_r is not None or args.identity != "match"
    p.want_pica = fmt in ("pica2", "tajd", "all", "fst3pi")
    p.want_fst = fmt in ("hfst", "all") and not args.panel
    if args.panel and fmt not in ("hfst", "tajd", "all"):
        fail("--panel belongs to --format hfst (every pair), tajd (every panel), all (both) or dstat (quartets)")
    # --panel: the pair tables come from the streaming K-population scan (impop_scan_multi) when h-fst is unrounded on `match`,
    # else - like every per-panel tajd table - from impop_pairwise_scan_panel: one Gram pass per window for all panels and pairs
    p.panel_fst = bool(args.panel) and fmt in ("hfst", "all")
    p.panel_tajd = bool(args.panel) and fmt in ("tajd", "all")
    p.need_pairs = (p.panel_tajd or (p.panel_fst and p.fst_pairs)) if args.panel else \
        (p.want_pica and p.pica_pairs) or (p.want_fst and p.fst_pairs)
    return p


def classic_panel(args, job, run, idx, pops, t):
    """--panel on hfst / tajd / all for the rows idx of one matrix: the pair records into t.panel_tables, the panel records into
    t.panel_taj"""
    p = job.plan
    pr = pan = pw = None
    if p.panel_fst and not p.fst_pairs:
        pr = run.panel(pops)
    one_call = p.panel_fst and p.fst_pairs and p.panel_tajd and p.pica_r == p.fst_r
    if p.panel_tajd:
        pan, pr2, pw = run.panel_allpairs(pops, p.pica_t, p.pica_r, True, one_call)
        if one_call:
            pr = pr2
    if p.panel_fst and pr is None:  # (h-fst.py has no threshold: it only groups pica2)
        _, pr, _ = run.panel_allpairs(pops, p.pica_t, p.fst_r, False, True)
    if pr is not None:
        if t.panel_tables is None:
            t.panel_tables = np.zeros((job.n_rows, pr.shape[1]), dtype=pr.dtype)
        t.panel_tables[idx] = pr
    if pan is not None:
        K = len(pops)
        if t.panel_taj is None:
            t.panel_taj = {"pi_site": np.full((job.n_rows, K), np.nan), "tajima_d": np.full((job.n_rows, K), np.nan),
                           "s_all": np.zeros(job.n_rows, dtype=np.int64), "samples": [awk_line_count(f) for f in args.panel]}
        t.panel_taj["pi_site"][idx] = pan["pi_site"]
        t.panel_taj["s_all"][idx] = pw["s_all"]
        D = pan["tajima_d"].copy()
        for k in range(K):
            cnt_k, matched = t.panel_taj["samples"][k], int(pops[k].sum())
            if cnt_k < 2:
                fail(f"Need at least two samples to compute Tajima's D (found {cnt_k})", 1)  # run_tajd.sh:84-87
            if cnt_k != matched and len(idx):  # run_tajd.sh:180: n = the list's LINE count (see the -l case in classic_pair)
                print(f"Warning: sample list {t.panel_labels[k]} has {cnt_k} lines but selects {matched} haplotypes; Tajima's D uses "
                      f"n = {cnt_k} like run_tajd.sh", file=sys.stderr)
                pi_txt = np.array([float(f"{float(x):.8f}") for x in pan["pi_site"][:, k]])
                D[:, k] = run.ctx.tajimas_d(np.full(len(idx), cnt_k, dtype=np.int64), pw["s_all"].astype(np.float64), pi_txt)
        t.panel_taj["tajima_d"][idx] = D


def classic_fst3pi(job, run, idx, mask_a, mask_b, t):
    """run_fst_impg.sh:73: pica2.py -t T -r R on the lists A, B and A u B, for the rows idx of one matrix"""
    p = job.plan
    if p.pica_pairs:
        for name, sel in (("pi3_a", mask_a), ("pi3_b", mask_b), ("pi3_c", mask_a | mask_b)):
            t.col[name][idx] = run.pairs(sel, None, None, p.pica_t, p.pica_r, False)["pi_site"]
    else:
        from impop_amd.drivers import pi_union_site
        res = run.stream(None, mask_a, mask_b)
        nA, nB = int(mask_a.sum()), int(mask_b.sum())
        t.col["pi3_a"][idx], t.col["pi3_b"][idx] = res["pi_a"], res["pi_b"]
        t.col["pi3_c"][idx] = [pi_union_site(r, nA, nB, int(L)) for r, L in zip(res, job.L_col[idx])]


def classic_pair(args, job, run, idx, mask_p, mask_a, mask_b, n_hap, n_matched, t):
    """the pica2 / h-fst / tajd columns of the rows idx of one matrix: one call where both tables round alike"""
    p, fmt = job.plan, args.format
    want_s = fmt in ("tajd", "all")
    one_call = p.want_pica and p.want_fst and p.pica_pairs and p.fst_pairs and p.pica_r == p.fst_r and not p.grouped_fst
    pica_rec = fst_rec = None
    if p.want_pica:
        pica_rec = run.pairs(mask_p, mask_a if one_call else None, mask_b if one_call else None, p.pica_t, p.pica_r, want_s) \
            if p.pica_pairs else run.stream(mask_p, mask_a, mask_b)
        if one_call or (p.want_fst and not p.pica_pairs and not p.fst_pairs):
            fst_rec = pica_rec
    if p.want_fst and fst_rec is None and mask_a is not None:
        fst_rec = run.pairs(None, mask_a, mask_b, p.grouped_t, p.fst_r, False, args.fst_method if p.grouped_fst else "direct") \
            if p.fst_pairs else run.stream(None, mask_a, mask_b)
    if pica_rec is not None:
        t.col["pi_site"][idx] = pica_rec["pi_site"]
        if want_s:
            t.s_all[idx] = pica_rec["s_all"]
            D = pica_rec["tajima_d"]
            t.samples_col = t.sample_count if t.sample_count is not None else n_hap
            if t.sample_count is not None and t.sample_count != n_matched and len(idx):
                # run_tajd.sh:180 hands tj_d.py `-n SAMPLE_COUNT`, the list's LINE count, whatever the number of
                # haplotypes those lines select (a bare sample name selects two, an unknown name none, a repeated
                # line counts twice).  The scan evaluated D with n = matched haplotypes: redo D (on the GPU,
                # impop_tajimas_d) with the reference's n, pi through the same "%.8f" text (run_tajd.sh:174) and S.
                print(f"Warning: sample list has {t.sample_count} lines but selects {n_matched} haplotypes; Tajima's D uses "
                      f"n = {t.sample_count} like run_tajd.sh", file=sys.stderr)
                pi_txt = np.array([float(f"{float(x):.8f}") for x in pica_rec["pi_site"]])
                D = run.ctx.tajimas_d(np.full(len(idx), t.sample_count, dtype=np.int64), pica_rec["s_all"].astype(np.float64), pi_txt)
            t.col["tajima_d"][idx] = D
    if fst_rec is not None:
        for k in ("fst", "pi_a", "pi_b", "pi_xy", "dxy", "da"):
            t.col[k][idx] = fst_rec[k]


def scan_classic(args, job):
    """--format pica2 / hfst / tajd / fst3pi / all, with -A / -B, -l, -u or --panel, on one device, --devices N or one rank of a
    torch.distributed job: the tables of the reference's drivers (write_tables)"""
    p, fmt = job.plan, args.format
    if args.sequence_length is not None:
        if fmt != "pica2" or args.sequence_length <= 0:
            fail("--sequence-length (a positive integer) belongs to --format pica2 (run_pica2_impg.sh -l)")
        job.L_col[:] = args.sequence_length  # EFFECTIVE_LENGTH, run_pica2_impg.sh:153-157
    out = job.open_output()
    t = SimpleNamespace(s_all=np.zeros(job.n_rows, dtype=np.int64), panel_tables=None, panel_taj=None, samples_col=0, sample_count=None,
                        panel_labels=panel_labels(args) if args.panel else None)
    t.col = {k: np.full(job.n_rows, np.nan) for k in ("pi_site", "tajima_d", "fst", "pi_a", "pi_b", "pi_xy", "dxy", "da", "pi3_a", "pi3_b", "pi3_c")}
    if args.sample_list:
        t.sample_count = awk_line_count(args.sample_list)  # run_tajd.sh:83
        if fmt in ("tajd", "all") and t.sample_count < 2:
            fail(f"Need at least two samples to compute Tajima's D (found {t.sample_count})", 1)  # :84-87
    for _, mf, idx, wins in job.matrices():
        with job.upload(mf, wins, p.need_pairs) as run:
            mask_p = mask_a = mask_b = None
            if args.sample_list:
                mask_p = flags_for(args.sample_list, mf.names)
            if args.subset:
                mask_p = flags_for(args.subset, mf.names)
            n_matched = mf.n_hap if mask_p is None else int(mask_p.sum())
            if args.pop_a and args.pop_b:
                mask_a, mask_b = flags_for(args.pop_a, mf.names), flags_for(args.pop_b, mf.names)
                if not mask_a.any() or not mask_b.any():
                    fail("No valid sequences found in one or both populations", 1)  # h-fst.py:319-321
            if args.panel:
                classic_panel(args, job, run, idx, [flags_for(f, mf.names) for f in args.panel], t)
            elif fmt == "fst3pi":
                if mask_a is None:
                    fail("--format fst3pi needs -A and -B")
                if (mask_a & mask_b).any():
                    fail("--format fst3pi needs disjoint populations")
                classic_fst3pi(job, run, idx, mask_a, mask_b, t)
            else:
                classic_pair(args, job, run, idx, mask_p, mask_a, mask_b, mf.n_hap, n_matched, t)
    write_tables(out, args, fmt, job.regions, job.L_col, t.col, t.s_all, t.samples_col, p.thr_txt, p.r_txt, t.panel_tables, t.panel_labels,
                 panel_taj=t.panel_taj)
    job.close_output(out)


# ---- what each format does not combine with: one table, walked in its order by refusal() ------------------------------------------

def _excludes(sentence, *options):
    """the sentence saying whose sequences a format works on, and the options that sentence excludes"""
    return lambda a: f"--format {a.format} {sentence}" if any(getattr(a, o) for o in options) else None


def _takes_panel(lo, hi, lists):
    return lambda a: None if a.panel and lo <= len(a.panel) <= hi else f"--format {a.format} takes --panel {lists}"


def _has_no_threshold(why):
    """the formats that count sites: -t / -r / --fst-round-digits mean nothing to them"""
    return lambda a: f"--format {a.format} {why}" if (a.threshold is not None or a.round_digits is not None
                                                       or a.fst_round_digits is not None) else None


def _when(fmt, check):
    return lambda a: check(a) if a.format == fmt else None


def _no_identity(a):
    if a.threshold is not None or a.round_digits is not None or a.identity != "match":
        return "-t / -r / --identity belong to other formats"


def _no_fst(a):
    if a.fst_method != "direct" or a.fst_round_digits is not None or a.sequence_length is not None:
        return "--fst-method / --fst-round-digits / --sequence-length belong to other formats"


_OF_SUBSET = ("panel", "pop_a", "pop_b", "sample_list")   # what a format of the sequences of -u excludes: -A / -B / --panel / -l
_OF_PANEL = ("pop_a", "pop_b", "sample_list", "subset")   # what a format of the --panel populations excludes: -A / -B / -l / -u


def _ehh_values(a):
    if a.ehh_core_offset is not None and a.ehh_cores:
        return "give --ehh-core-offset or --ehh-cores, not both"
    if a.ehh_core_offset is not None and a.ehh_core_offset < 0:
        return "--ehh-core-offset is a 0-based offset into the window (>= 0)"


def _ld_values(a):
    if a.ld_min_maf is not None and not 0.0 <= a.ld_min_maf <= 0.5:
        return "--ld-min-maf is a minor-allele frequency (0 .. 0.5)"
    if a.ld_max_sites is not None and not 4 <= a.ld_max_sites <= 1024:
        return "--ld-max-sites takes 4 .. 1024"


def _diploid_values(a):
    if a.roh_min_sites is not None and a.roh_min_sites < 1:
        return "--roh-min-sites takes 1 or more"


def _ibs_values(a):
    if a.ibs_min_sites is not None and a.ibs_min_sites < 1:
        return "--ibs-min-sites takes 1 or more"


def _dstat_values(a):
    if (a.dstat_blocks is None) != (a.dstat_summary is None):
        return "--dstat-blocks N and --dstat-summary PATH go together"
    if a.dstat_blocks is not None and a.dstat_blocks < 1:
        return "--dstat-blocks takes 1 or more"
    try:
        parse_quartets(a.quartet, len(a.panel))
    except ValueError as e:
        return str(e)


def _sfs_values(a):
    if a.sfs_outgroup is not None and not 1 <= a.sfs_outgroup <= len(a.panel):
        return f"--sfs-outgroup {a.sfs_outgroup}: position is outside the {len(a.panel)} lists of --panel"
    if a.sfs_blocks is not None and a.sfs_spectra is None:
        return "--sfs-blocks N belongs to --sfs-spectra PATH.npz"
    if a.sfs_blocks is not None and a.sfs_blocks < 1:
        return "--sfs-blocks takes 1 or more"
    try:
        parse_sfs_pairs(a.sfs_pair, len(a.panel))
    except ValueError as e:
        return str(e)
    if a.sfs_pairs_out is not None and not a.sfs_pair:
        return "--sfs-pairs-out PATH needs at least one --sfs-pair i,j"
    if a.sfs_pair and a.sfs_pairs_out is None and a.sfs_spectra is None:
        return "--sfs-pair i,j goes with --sfs-pairs-out PATH or --sfs-spectra PATH.npz"


def _pairdist_values(a):
    if a.pairdist_outgroup is not None and not (len(a.panel) >= 3 and 1 <= a.pairdist_outgroup <= len(a.panel)):
        return f"--pairdist-outgroup {a.pairdist_outgroup}: a 1-based position among at least three lists of --panel"
    if (a.pairdist_bins is not None or a.pairdist_bin_width is not None) and a.pairdist_hist is None:
        return "--pairdist-bins / --pairdist-bin-width belong to --pairdist-hist PATH"
    if a.pairdist_hist is not None and a.pairdist_bins is None:
        return "--pairdist-hist PATH needs --pairdist-bins B"
    if a.pairdist_bins is not None and not 1 <= a.pairdist_bins <= 1024:
        return "--pairdist-bins takes 1 to 1024"
    if a.pairdist_bin_width is not None and a.pairdist_bin_width < 1:
        return "--pairdist-bin-width takes 1 or more"


def _kinship_values(a):
    if a.kin_threshold is not None and not 0.0 <= a.kin_threshold <= 1.0:
        return "--kin-threshold takes a kinship in 0 .. 1"
    if bool(a.kin_watch) != (a.kin_watch_table is not None):
        return "--kin-watch sampleA,sampleB and --kin-watch-table PATH go together"
    for spec in a.kin_watch or []:
        parts = spec.split(",")
        if len(parts) != 2 or not all(parts) or parts[0] == parts[1]:
            return f"--kin-watch {spec}: two different sample names, as in sampleA,sampleB"
    if len(a.kin_watch or []) > 1024:
        return "--kin-watch: at most 1024 pairs per run"


def _ihs_values(a):
    if a.ihs_min_maf is not None and not 0.0 < a.ihs_min_maf <= 0.5:
        return "--ihs-min-maf takes a frequency above 0, at most 0.5"
    if a.ihs_cutoff is not None and not 0.0 <= a.ihs_cutoff <= 1.0:
        return "--ihs-cutoff takes 0 to 1"
    if (a.ihs_max_extend is not None and a.ihs_max_extend < 0) or (a.ihs_max_extend_sites is not None and a.ihs_max_extend_sites < 0):
        return "--ihs-max-extend / --ihs-max-extend-sites take 0 (no limit) or more"
    if a.ihs_bins is not None and a.ihs_bins < 1:
        return "--ihs-bins takes 1 or more"


class Format:
    """One entry of FORMATS.  formats: the --format names it serves; scan(args, job): what runs them; own(args): whether one of its own
    options was given, stray: the line that answers them under another format; checks: for a one-process, one-GPU format, what
    follows the three sentences every such format shares (refusal()), in the order they are tried: each args -> a line or None."""

    def __init__(self, formats, scan, own=None, stray=None, checks=None):
        self.formats, self.scan, self.own, self.stray, self.checks = formats, scan, own, stray, checks
        self.one_gpu = checks is not None


FORMATS = (
    Format(("af",), scan_af, lambda a: a.af_clusters or a.af_details, "--af-clusters / --af-details belong to --format af",
           (_excludes("clusters the sequences of -u (default: all): not with -A / -B / --panel / -l", *_OF_SUBSET), _no_fst)),
    Format(("ehh",), scan_ehh,
           lambda a: a.ehh_core_offset is not None or a.ehh_cores or a.ehh_flanks is not None or a.ehh_ref is not None,
           "--ehh-core-offset / --ehh-cores / --ehh-flanks / --ehh-ref belong to --format ehh",
           (_excludes("scans the sequences of -u (default: all) on the full matrix: not with -A / -B / --panel / -l / --compact",
                      *_OF_SUBSET, "compact"), _ehh_values, _no_identity, _no_fst)),
    Format(("hapstats",), scan_hapstats, None, None,
           (_excludes("compares the sequences of -u (default: all): not with -A / -B / --panel / -l", *_OF_SUBSET), _no_identity, _no_fst)),
    Format(("ld",), scan_ld, lambda a: a.ld_min_maf is not None or a.ld_max_sites is not None,
           "--ld-min-maf / --ld-max-sites belong to --format ld",
           (_excludes("compares the sites among the sequences of -u (default: all): not with -A / -B / --panel / -l", *_OF_SUBSET),
            _no_identity, _no_fst, _ld_values)),
    Format(("diploid",), scan_diploid, lambda a: a.roh_min_sites is not None or a.ind_table is not None,
           "--roh-min-sites / --ind-table belong to --format diploid",
           (_excludes("pairs the sequences of -u (default: all): not with -A / -B / --panel / -l", *_OF_SUBSET), _no_identity, _no_fst,
            _diploid_values)),
    Format(("ibs",), scan_ibs,
           lambda a: a.ibs_min_sites is not None or a.ibs_pairs is not None or a.ibs_segments is not None or a.ibs_pair_table is not None,
           "--ibs-min-sites / --ibs-pairs / --ibs-segments / --ibs-pair-table belong to --format ibs",
           (_excludes("pairs the sequences of -u (default: all): not with -A / -B / --panel / -l", *_OF_SUBSET), _no_identity, _no_fst,
            _ibs_values)),
    Format(("dstat",), scan_dstat,
           lambda a: a.quartet or a.dstat_polarize or a.dstat_blocks is not None or a.dstat_summary is not None,
           "--quartet / --dstat-polarize / --dstat-blocks / --dstat-summary belong to --format dstat",
           (_takes_panel(4, 8, "P1.txt P2.txt P3.txt O.txt [more lists]: 4 to 8 population lists"),
            _excludes("compares the populations of --panel: not with -A / -B / -l / -u", *_OF_PANEL), _no_identity, _no_fst, _dstat_values)),
    Format(("sfs",), scan_sfs,
           lambda a: (a.sfs_outgroup is not None or a.sfs_pair or a.sfs_pairs_out is not None or a.sfs_spectra is not None
                      or a.sfs_blocks is not None),
           "--sfs-outgroup / --sfs-pair / --sfs-pairs-out / --sfs-spectra / --sfs-blocks belong to --format sfs",
           (_takes_panel(1, 8, "A.txt [B.txt ...]: 1 to 8 population lists"),
            _excludes("reads the spectra of the populations of --panel: not with -A / -B / -l / -u", *_OF_PANEL), _no_identity, _no_fst,
            _sfs_values)),
    Format(("pairdist",), scan_pairdist,
           lambda a: (a.pairdist_outgroup is not None or a.pairdist_panels is not None or a.pairdist_hist is not None
                      or a.pairdist_bins is not None or a.pairdist_bin_width is not None),
           "--pairdist-outgroup / --pairdist-panels / --pairdist-hist / --pairdist-bins / --pairdist-bin-width belong to --format pairdist",
           (_takes_panel(1, 8, "a.txt b.txt [more.txt]: 1 to 8 population lists"),
            _excludes("reads the distances of the populations of --panel: not with -A / -B / -l / -u", *_OF_PANEL),
            _has_no_threshold("counts differing sites: it has no -t / -r"), _pairdist_values)),
    Format(("kinship",), scan_kinship,
           lambda a: a.kin_threshold is not None or a.kin_pairs is not None or bool(a.kin_watch) or a.kin_watch_table is not None,
           "--kin-threshold / --kin-pairs / --kin-watch / --kin-watch-table belong to --format kinship",
           (_excludes("pairs the sequences of -u (default: all): not with -A / -B / --panel / -l", *_OF_SUBSET),
            _has_no_threshold("counts genotypes: it has no -t / -r (the kinship threshold is --kin-threshold)"), _kinship_values)),
    Format(("ihs", "xpehh"), scan_ihs,
           lambda a: (a.ihs_min_maf is not None or a.ihs_cutoff is not None or a.ihs_max_extend is not None
                      or a.ihs_max_extend_sites is not None or a.ihs_bins is not None or a.ihs_keep_edge),
           "--ihs-min-maf / --ihs-cutoff / --ihs-max-extend / --ihs-max-extend-sites / --ihs-bins / --ihs-keep-edge belong to "
           "--format ihs and --format xpehh",
           (_has_no_threshold("integrates haplotype homozygosity: it has no -t / -r"),
            _when("ihs", _excludes("scans the sequences of -u (default: all): not with -A / -B / --panel / -l", *_OF_SUBSET)),
            _when("xpehh", _takes_panel(2, 2, "a.txt b.txt: two population lists")),
            _when("xpehh", _excludes("compares the two populations of --panel: not with -A / -B / -l / -u", *_OF_PANEL)), _ihs_values)),
    Format(("pica2", "hfst", "tajd", "fst3pi", "all"), scan_classic),  # their checks: classic_plan(), sim_list_refusal()
)


def refusal(args):
    """What the command line does not combine with: one line (exit 2, before any file is read or device opened), or None.  The table
    is walked in its order: the entry of --format runs its checks, every entry before and after it answers for its own options."""
    f = f"--format {args.format}"
    for entry in FORMATS:
        if args.format not in entry.formats:
            if entry.own is not None and entry.own(args):
                return entry.stray
        elif entry.one_gpu:
            if args.sim_list:
                return f"{f} scans a presence matrix (--matrix / --bed): not with --sim-list"
            if int(os.environ.get("WORLD_SIZE", "1")) > 1:
                return f"{f} is a one-process, one-GPU scan: not under torch.distributed.run"
            if args.devices > 1:
                return f"{f} runs on one GPU: not with --devices N"
            for check in entry.checks:
                message = check(args)
                if message:
                    return message
    return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--matrix", nargs="+", help=".npz presence matrices (impop_amd.matrixio), one per chromosome")
    ap.add_argument("--bed", "-b")
    ap.add_argument("--sim-list", metavar="FILE", help="instead of --matrix / --bed: TSV `chrom start end sim_path [S]`, one .sim "
                    "identity table per window (formats pica2, hfst, tajd, all)")
    ap.add_argument("--sim-threads", type=int, default=0, metavar="N", help="--sim-list: host threads that parse tables "
                    "(default: OMP_NUM_THREADS, else 16)")
    ap.add_argument("--format", choices=["pica2", "hfst", "tajd", "fst3pi", "af", "ehh", "hapstats", "ld", "diploid", "ibs", "dstat", "sfs", "pairdist", "kinship", "ihs", "xpehh", "all"], default="all",
                    help="fst3pi = the 3 x pi table of run_fst_impg.sh (needs -A and -B, disjoint); af = haplotype clusters per window "
                         "(scripts/af.py; not part of `all`); ehh = integrated EHH per core site (ehhgfa.py; not part of `all`); "
                         "hapstats = haplotype-frequency statistics per window (K, H1, H12, H2/H1, diversity; not part of `all`); "
                         "ld = linkage disequilibrium per window (ZnS, mean |D'|, Kim-Nielsen omega; not part of `all`); "
                         "diploid = heterozygosity, F_IS and runs of homozygosity per window and individual (not part of `all`); "
                         "ibs = pairwise identity-by-state tracts / ROH segments over each row's whole matrix (not part of `all`); "
                         "dstat = Patterson's D (ABBA-BABA), f4 and f_d per window and quartet of --panel populations (not part of `all`); "
                         "sfs = spectrum summaries and neutrality tests per window and --panel population, pair classes and spectra "
                         "(not part of `all`); ihs = iHS and nSL per site from a device PBWT, xpehh = XP-EHH and XP-nSL per site between the "
                         "two --panel populations, cores = the varying sites of each row (neither is part of `all`)")
    ap.add_argument("--af-clusters", metavar="FILE", help="af: long table REGION cluster_id count frequency (af.py's summary per window)")
    ap.add_argument("--af-details", metavar="FILE", help="af: long table REGION sample_id cluster_id threshold (af.py --details per window)")
    ap.add_argument("--ehh-core-offset", type=int, default=None, metavar="N", help="ehh: 0-based site offset of the core into each window "
                    "(default: the window's midpoint)")
    ap.add_argument("--ehh-cores", metavar="FILE", help="ehh: one core position (bp) per BED row instead of an offset")
    ap.add_argument("--ehh-flanks", choices=["reference", "two-sided"], default=None, help="ehh: reference (default) = both halves from "
                    "the sites right of the core (ehhgfa.py:56-61); two-sided = the left half from the sites left of it")
    ap.add_argument("--ehh-ref", metavar="NAME", default=None, help="ehh: the sequence whose core allele is REF (default: the first)")
    ap.add_argument("--ld-min-maf", type=float, default=None, metavar="F", help="ld: a site takes part when its minor allele is carried by "
                    "at least max(1, ceil(F * SAMPLES)) sequences (default 0.05)")
    ap.add_argument("--ld-max-sites", type=int, default=None, metavar="M", help="ld: more qualifying sites than M are thinned evenly to M "
                    "(default 512; 4..1024)")
    ap.add_argument("--roh-min-sites", type=int, default=None, metavar="N", help="diploid: a stretch without a heterozygous site counts as a "
                    "run of homozygosity when it is at least N sites long (default 50)")
    ap.add_argument("--ind-table", metavar="PATH", help="diploid: also write one row per window and sample to PATH")
    ap.add_argument("--ihs-min-maf", type=float, default=None, metavar="F", help="ihs / xpehh: cores have a minor-allele frequency of at least F (default 0.05)")
    ap.add_argument("--ihs-cutoff", type=float, default=None, metavar="F", help="ihs / xpehh: integrate until EHH falls below F (default 0.05)")
    ap.add_argument("--ihs-max-extend", type=int, default=None, metavar="BP", help="ihs / xpehh: integrate IHH at most this far from the core, in site "
                    "coordinates (default 1000000; 0 = no limit)")
    ap.add_argument("--ihs-max-extend-sites", type=int, default=None, metavar="N", help="ihs / xpehh: integrate SL over at most N varying sites "
                    "(default 100; 0 = no limit)")
    ap.add_argument("--ihs-bins", type=int, default=None, metavar="B", help="ihs: frequency bins of the standardisation (default 50)")
    ap.add_argument("--ihs-keep-edge", action="store_true", help="ihs / xpehh: keep the cores whose integral ran into the end of the matrix")
    ap.add_argument("--ibs-min-sites", type=int, default=None, metavar="N", help="ibs: a stretch without a difference between two "
                    "sequences is reported when it is at least N sites long (default 50)")
    ap.add_argument("--ibs-pairs", choices=["all", "diploid"], default=None, help="ibs: all = every pair of the sequences of -u (default); "
                    "diploid = the two haplotypes of every sample, paired as --format diploid pairs them")
    ap.add_argument("--ibs-segments", metavar="PATH", help="ibs: write the segment list to PATH (TSV seq1 seq2 start end sites open)")
    ap.add_argument("--ibs-pair-table", metavar="PATH", help="ibs: write one row per pair to PATH (SEQ1 SEQ2 N_DIFF LONGEST TRACTS TRACT_SITES)")
    ap.add_argument("--quartet", action="append", default=None, metavar="i,j,k,o", help="dstat: the populations P1,P2,P3,O of a quartet as "
                    "1-based positions in --panel; repeatable (default with exactly four lists: 1,2,3,4)")
    ap.add_argument("--dstat-polarize", action="store_true", help="dstat: per site and quartet the outgroup's major allele is ancestral "
                    "(a site where the outgroup is split evenly is skipped)")
    ap.add_argument("--dstat-blocks", type=int, default=None, metavar="N", help="dstat: with --dstat-summary, the number of consecutive "
                    "groups of BED rows of the block jackknife")
    ap.add_argument("--dstat-summary", metavar="PATH", help="dstat: one row per quartet to PATH: D, its jackknife SE and Z, f_d and its "
                    "SE, the block count, the summed ABBA / BABA")
    ap.add_argument("--sfs-outgroup", type=int, default=None, metavar="i", help="sfs: the major allele of --panel list i (1-based) is "
                    "ancestral per site (a site where it is split evenly is skipped); default: allele 1 counts as derived")
    ap.add_argument("--sfs-pair", action="append", default=None, metavar="i,j", help="sfs: a pair of --panel lists (1-based, no shared "
                    "sequence) for --sfs-pairs-out and the joint spectra of --sfs-spectra; repeatable")
    ap.add_argument("--sfs-pairs-out", metavar="PATH", help="sfs: one row per window and --sfs-pair to PATH: private, shared and fixed sites")
    ap.add_argument("--sfs-spectra", metavar="PATH.npz", help="sfs: the 1-D spectrum of every list (sfs_<label>) and the joint spectrum of "
                    "every --sfs-pair (jsfs_<a>_<b>), summed over the BED rows of each of --sfs-blocks groups")
    ap.add_argument("--sfs-blocks", type=int, default=None, metavar="N", help="sfs: with --sfs-spectra, the number of consecutive groups "
                    "of BED rows the spectra are summed over (default 1)")
    ap.add_argument("-A", "--pop-a"); ap.add_argument("-B", "--pop-b")
    ap.add_argument("--pairdist-outgroup", type=int, default=None, metavar="K", help="pairdist: --panel list K (1-based) is the outgroup O: adds "
                    "RNDMIN = DMIN / ((mean H(A,O) + mean H(B,O)) / 2) to the main table")
    ap.add_argument("--pairdist-panels", metavar="PATH", help="pairdist: one row per window and --panel list to PATH: the mismatch "
                    "distribution's mean, variance, extremes and raggedness")
    ap.add_argument("--pairdist-hist", metavar="PATH", help="pairdist: the distance histograms within every list and between every pair to "
                    "PATH, long form, non-zero bins only; needs --pairdist-bins")
    ap.add_argument("--pairdist-bins", type=int, default=None, metavar="B", help="pairdist: bins per histogram (1..1024); the last collects the overflow")
    ap.add_argument("--kin-threshold", type=float, default=None, metavar="PHI", help="kinship: a pair counts as RELATED in a window when its "
                    "KING-robust kinship is at least PHI (default 0.0884, the 2nd / 3rd degree cut; compared exactly as round(PHI * 10000) / 10000)")
    ap.add_argument("--kin-pairs", metavar="PATH", help="kinship: the joint genotype counts of every pair of samples summed over all BED rows "
                    "and all --matrix files to PATH, with KING within-family and robust kinship, the IBS distance and the degree label")
    ap.add_argument("--kin-watch", action="append", default=None, metavar="A,B", help="kinship: also follow the pair of samples A,B row by "
                    "row (repeatable, at most 1024); needs --kin-watch-table")
    ap.add_argument("--kin-watch-table", metavar="PATH", help="kinship: one row per BED row and --kin-watch pair to PATH")
    ap.add_argument("--pairdist-bin-width", type=int, default=None, metavar="w", help="pairdist: distances per bin (default 1)")
    ap.add_argument("--panel", nargs="+", metavar="POP.txt", help="K = 2..8 disjoint population lists.  hfst: every pair (replaces "
                    "run_h_fst_panels.sh), one table per pair headed `# POP_A-vs-POP_B` - unrounded `match` in ONE streaming pass, with "
                    "-r N or --identity dice from one Gram pass per window (impop_pairwise_scan_panel).  tajd: every panel (replaces "
                    "run_tajd_panels.sh: -t 0.999 -r 5, S over all rows), one table per panel headed `# POP`, SAMPLES = the list's "
                    "line count.  all: both.  One process, one GPU; not with --fst-method grouped, -l, --devices N, --sim-list")
    ap.add_argument("-l", "--sample-list", help="tajd: sample list (run_tajd.sh -l); n = its line count")
    ap.add_argument("-u", "--subset", help="pica2: --subset-sequence-list")
    ap.add_argument("--sequence-length", type=int, default=None, metavar="L",
                    help="pica2: run_pica2_impg.sh -l — the length handed to pica2 AND printed in the LENGTH column, instead of end - start")
    ap.add_argument("-t", "--threshold", type=threshold_arg, default=None, help="see the table above")
    ap.add_argument("-r", "--round-digits", type=round_arg, default=None, help="an integer, or `none`; see the table above")
    ap.add_argument("--fst-round-digits", type=round_arg, default=None, help="--format all: h-fst.py -r for the h-fst table")
    ap.add_argument("-p", "--region-prefix", default="CHM13#0#")
    ap.add_argument("-o", "--output")
    ap.add_argument("--identity", choices=["match", "dice"], default="match")
    ap.add_argument("--fst-method", choices=["direct", "grouped"], default="direct",
                    help="hfst: grouped = scripts/hudson/hud.py -m grouped at -t (default 0.999), per window on the all-pairs path")
    ap.add_argument("--compact", action="store_true", help="scan from the matrix compacted to its variable sites "
                    "(impop_matrix_compact): identical output, far fewer bytes (and, on the all-pairs path, multiply-adds) per pass")
    ap.add_argument("--device", type=int, default=None, help="default: LOCAL_RANK, else 0")
    ap.add_argument("--devices", type=int, default=1, metavar="N",
                    help="ONE process driving N GPUs through the C ABI (impop_scan_sharded; impop_pairwise_scan_sharded for the "
                         "all-pairs formats): the BED rows are cut into N contiguous ranges, each device holds the slab of sites its "
                         "rows touch, every device works before the first result is fetched; no torch, no launcher.  With fewer "
                         "than N devices the contexts share device 0.  Not with --panel or --compact")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend when launched with WORLD_SIZE > 1 "
                    "(nccl = RCCL over xGMI; gloo for rehearsals)")
    args = ap.parse_args()
    if args.sim_list and (args.matrix or args.bed):
        ap.error("--sim-list replaces --matrix / --bed: give one or the other")
    if not args.sim_list and not (args.matrix and args.bed):
        ap.error("give --matrix and --bed, or --sim-list")
    message = refusal(args)
    if message:
        fail(message)
    fmt = args.format
    entry = next(e for e in FORMATS if fmt in e.formats)
    if args.sim_list:
        message = sim_list_refusal(args)
        if message:
            fail(message)
    args.threshold_text = None
    if args.threshold is not None:
        args.threshold, args.threshold_text = args.threshold
    # Multi-GPU: `python -m torch.distributed.run --nproc-per-node N scripts/impop_scan.py ...` — the BED rows
    # are sharded over ranks, each rank uploads only the slab its windows touch, scans it, and ONE
    # all-gather of the fixed-size records per scan brings everything to rank 0, which prints.
    rank, world, local_rank = 0, 1, 0
    if fmt not in ("pairdist", "kinship", "ihs", "xpehh"):  # these four never read the launcher's variables: device 0 unless --device
        rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
        local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    plan = None if entry.one_gpu else classic_plan(args, rank, world, local_rank)
    if args.device is None:
        args.device = local_rank if (world == 1 or args.backend == "nccl") else 0
    if plan is not None and args.sim_list:
        return scan_sim_list(args, fmt, plan.pica_t, plan.pica_r, plan.fst_r, plan.thr_txt, plan.r_txt)
    job = Job(args, rank, world, local_rank)
    job.plan = plan
    entry.scan(args, job)
    if world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
