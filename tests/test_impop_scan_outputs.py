"""No GPU: whole runs of scripts/impop_scan.py with a stand-in for its Runner.  tests/golden/impop_scan_outputs.json holds, for a
list of command lines over two small matrices (chr3, chr8) and a BED that alternates between them, what the driver wrote when the
fixture was recorded: stdout, stderr, every side file, the exit code and the list of calls the stand-in received (constructions with
need_pairs / compact, every device call with its arguments).  The test replays all of it byte for byte, which pins the number of
uploads, the order of the device calls, the row order of every table and the order of the warnings.  Of a run that ends early
(exit code not 0) the list keeps the device calls only, neither the constructions nor close(): a check may move in front of the
upload it follows today, and a matrix that went up may be closed on the way out, but no check moves behind a device call.  The
fixture is frozen: a refactor of the driver never re-records it.  A text of more than 4000 characters (--help, a long segment list) is held as its sha256.
`python tests/test_impop_scan_outputs.py --write [SCRIPT]` records it anew, from SCRIPT if one is given (a change of behaviour)."""
import contextlib
import hashlib
import importlib.util
import io
import json
import os
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):  # also when run as a script to record
    if _p not in sys.path:
        sys.path.insert(0, _p)
SCAN = os.path.join(ROOT, "scripts", "impop_scan.py")
FIXTURE = os.path.join(ROOT, "tests", "golden", "impop_scan_outputs.json")


def load_cli(script=SCAN):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("impop_scan_cli_outputs", script)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    return mod


# ---- the stand-in ---------------------------------------------------------------------------------------------------------------------

def plain(x):
    """arguments of a call as plain lists"""
    if x is None or isinstance(x, (bool, str)):
        return x
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float(x)
    if isinstance(x, np.ndarray) and x.dtype.names:
        return [[plain(r[f]) for f in x.dtype.names] for r in x.reshape(-1)]
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, dict):
        return {k: plain(v) for k, v in sorted(x.items())}
    return [plain(v) for v in x]


def members(mask):
    return None if mask is None else np.flatnonzero(np.asarray(mask)).tolist()


def seeded(dtype, shape, tag):
    """records of a dtype that depend on nothing but the call's name and shape: small integers, doubles with a few nan"""
    rng = np.random.default_rng(zlib.crc32(f"{tag}{shape}".encode()))
    out = np.zeros(shape, dtype=dtype)
    for name in dtype.names:
        sub = out[name]
        if sub.dtype.kind == "f":
            v = rng.random(sub.shape) * 2 - 0.5
            v[rng.random(sub.shape) < 0.1] = np.nan
            sub[...] = v
        else:
            sub[...] = rng.integers(1, 40, size=sub.shape)
    return out


class StandIn:
    """stands in for impop_scan.Runner: records every call, answers from the plain restatements under tests/ where one exists and
    with seeded records of the right dtype elsewhere"""
    calls = []

    def __init__(self, args, mf, windows, need_pairs, rank, world, local_rank):
        self.mf = mf
        self.m01 = np.unpackbits(np.ascontiguousarray(mf.bits).view(np.uint8), axis=1, bitorder="little")[:, :mf.n_site]
        self.local_wins = [tuple(int(x) for x in w) for w in windows]
        self.n = len(self.local_wins)
        self.bm, self.ctx = _Matrix(self), _Context()
        StandIn.calls.append(["Runner", mf.contig, self.local_wins, bool(need_pairs), bool(args.compact), rank, world, local_rank])

    def _note(self, name, *a):
        StandIn.calls.append([name] + [plain(x) for x in a])

    def stream(self, mask_p, mask_a, mask_b):
        import impop_amd
        self._note("stream", members(mask_p), members(mask_a), members(mask_b))
        return seeded(impop_amd.STATS_DTYPE, self.n, "stream")

    def pairs(self, mask_p, mask_a, mask_b, threshold, round_digits, want_s, fst_method="direct"):
        import impop_amd
        self._note("pairs", members(mask_p), members(mask_a), members(mask_b), threshold, round_digits, want_s, fst_method)
        return seeded(impop_amd.PAIRWISE_DTYPE, self.n, "pairs")

    def panel(self, pops):
        import impop_amd
        self._note("panel", [members(p) for p in pops])
        K = len(pops)
        return seeded(impop_amd.PAIR_DTYPE, (self.n, K * (K - 1) // 2), "panel")

    def panel_allpairs(self, pops, threshold, round_digits, want_s, want_pairs):
        import impop_amd
        self._note("panel_allpairs", [members(p) for p in pops], threshold, round_digits, want_s, want_pairs)
        K = len(pops)
        return (seeded(impop_amd.PANEL_DTYPE, (self.n, K), "pa_panels"),
                seeded(impop_amd.PAIR_DTYPE, (self.n, K * (K - 1) // 2 if want_pairs else 0), "pa_pairs"),
                seeded(impop_amd.PANEL_WINDOW_DTYPE, self.n, "pa_windows"))

    def hapstats(self, mask_p):
        import impop_amd
        self._note("hapstats", members(mask_p))
        return seeded(impop_amd.HAPLOTYPE_DTYPE, self.n, "hapstats")

    def ld(self, mask_p, min_mac, max_sites):
        import impop_amd
        self._note("ld", members(mask_p), min_mac, max_sites)
        rec = seeded(impop_amd.LD_DTYPE, self.n, "ld")
        rec["omega_split"] %= 4  # 0 = no split: OMEGA_POS NA
        used = np.array([[b + min(j, max(e - b - 1, 0)) for j in range(max_sites)] for b, e, _ in self.local_wins],
                        dtype=np.uint64).reshape(self.n, max_sites)
        return rec, used

    def diploid(self, pairs, min_run, want_individuals):
        import plain_diploid
        self._note("diploid", pairs, min_run, want_individuals)
        rec, ind = plain_diploid.reference(self.m01, pairs, self.local_wins, min_run)
        return (rec, ind) if want_individuals else rec

    def dstat(self, pops, quartets, polarize):
        import plain_dstat
        self._note("dstat", [members(p) for p in pops], quartets, polarize)
        return plain_dstat.reference(self.m01, [members(p) for p in pops], quartets, [w[:2] for w in self.local_wins], polarize)

    def sfs(self, pops, pairs, outgroup, tables, w0, w1):
        import plain_sfs
        self._note("sfs", [members(p) for p in pops], pairs, outgroup, tables, w0, w1)
        st, pr, sfs, jsfs = plain_sfs.reference(self.m01, [members(p) for p in pops], pairs, [w[:2] for w in self.local_wins[w0:w1]], outgroup)
        return st, pr, sfs if "sfs" in tables else None, jsfs if "jsfs" in tables else None

    def close(self):
        self._note("close")


class _Context:
    def tajimas_d(self, n, S, pi):
        StandIn.calls.append(["tajimas_d", plain(n), plain(S), plain(pi)])
        return np.asarray(S, dtype=np.float64) * 0.001 - np.asarray(pi, dtype=np.float64) + np.asarray(n, dtype=np.float64)


class _Genotypes:
    def __init__(self, run, pairs):
        self.run, self.pairs = run, pairs

    def kinship_scan(self, windows, kin=(884, 10000), watch=None, want_pairs=True):
        import plain_kinship
        self.run._note("kinship_scan", windows, kin, watch, want_pairs)
        out, tot, wat = plain_kinship.scan(self.run.m01, self.pairs, [w[:2] for w in windows], tuple(kin), watch or ())
        return out, tot if want_pairs else None, wat if watch else None

    def free(self):
        self.run._note("genotypes.free")


class _Matrix:
    def __init__(self, run):
        self.run = run

    def cluster_scan(self, windows, mask_p=None, kind="match", threshold=1.0, round_digits=None, want_members=True):
        import impop_amd
        run = self.run
        run._note("cluster_scan", windows, members(mask_p), kind, threshold, round_digits, want_members)
        rec = seeded(impop_amd.CLUSTER_DTYPE, run.n, "cluster")
        n_mem = run.m01.shape[0] if mask_p is None else int(np.asarray(mask_p).sum())
        ranks = np.array([[(i + w) % 3 for i in range(n_mem)] for w in range(run.n)], dtype=np.uint32).reshape(run.n, n_mem)
        return (rec, ranks) if want_members else rec

    def ehh_scan(self, windows, cores, mask=None, ref_hap=0, flanks="reference"):
        import impop_amd
        self.run._note("ehh_scan", windows, cores, members(mask), ref_hap, flanks)
        rec = seeded(impop_amd.EHH_DTYPE, self.run.n, "ehh")
        rec["ref_allele"] %= 2
        rec["n_members"][::2, 0] = 0  # an allele nobody carries prints no row
        return rec

    def ibs_scan(self, pairs=None, mask_p=None, min_sites=1, windows=None, want_segments=True):
        import plain_ibs
        run = self.run
        run._note("ibs_scan", pairs, members(mask_p), min_sites, windows, want_segments)
        prs = [tuple(p) for p in pairs] if pairs is not None else plain_ibs.all_pairs(plain_ibs.members_of(mask_p, run.m01.shape[0]))
        rec, seg, win = plain_ibs.reference(run.m01, prs, 0, run.m01.shape[1], min_sites, windows=windows)
        return rec, seg if want_segments else seg[:0], win, None

    def pairdist_scan(self, windows, pops, hist_bins=0, hist_width=1):
        import plain_pairdist
        self.run._note("pairdist_scan", windows, [members(p) for p in pops], hist_bins, hist_width)
        return plain_pairdist.scan(self.run.m01, [w[:2] for w in windows], [members(p) for p in pops], hist_bins, hist_width)

    def genotypes(self, pairs):
        self.run._note("genotypes", pairs)
        return _Genotypes(self.run, pairs)

    def ihs_scan(self, mask_a=None, mask_b=None, core_begin=None, core_end=None, min_mac=1, cutoff_milli=50, max_extend_bp=0,
                 max_extend_sites=0):
        import plain_ihs
        run = self.run
        run._note("ihs_scan", members(mask_a), members(mask_b), core_begin, core_end, min_mac, cutoff_milli, max_extend_bp, max_extend_sites)
        pops = [mask_a] if mask_b is None else [mask_a, mask_b]
        rec = plain_ihs.reference(run.m01, 0, run.m01.shape[1], core_begin, core_end, pops, min_mac=min_mac, cutoff_milli=cutoff_milli,
                                  max_bp=max_extend_bp, max_sites=max_extend_sites)
        return rec, None


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------

def write_inputs(d):
    """two matrices of 16 haplotypes on chr3 / chr8 (the shape of test_batch_driver_rows_go_to_their_chromosome), a BED that alternates
    between them with a row nobody holds, a malformed row and a prefixed row, and the population lists"""
    from impop_amd import matrixio
    rng = np.random.default_rng(77)
    n = 16
    for chrom, W, origin in (("chr3", 300, 500), ("chr8", 200, 0)):
        anc = (rng.random(W) < 0.3).astype(np.uint8)
        fam = np.repeat(anc[None], 4, axis=0) ^ (rng.random((4, W)) < 0.08).astype(np.uint8)
        m = fam[rng.integers(0, 4, size=n)] ^ (rng.random((n, W)) < 0.02).astype(np.uint8)
        m[1] = m[0]
        names = [f"S{i // 2:03d}#{i % 2 + 1}#{chrom}:{origin}-{origin + W}" for i in range(n)]
        matrixio.save_matrix(os.path.join(d, f"{chrom}.npz"), matrixio.from_dense(m, names, origin=origin, contig=f"CHM13#0#{chrom}"))
        if chrom == "chr8":
            matrixio.save_matrix(os.path.join(d, "anon.npz"), matrixio.from_dense(m, names, origin=origin, contig=""))
            matrixio.save_matrix(os.path.join(d, "weighted.npz"), matrixio.from_dense(m, names, origin=origin, contig="CHM13#0#chr8",
                                                                                      site_weight=np.full(W, 2, dtype=np.uint32)))
    files = {
        "g.bed": "# comment\nchr8\t10\t90\nchr3\t600\t700\nchrX\t5\t50\nchr3\tx\ty\nCHM13#0#chr8\t90\t200\tname\nchr3\t700\t800\n",
        "A.txt": "S000\nS001_hap1_hprc_r2\nS002#2\n", "B.txt": "S005\nS006\nS007_mat\n", "C.txt": "S003\nS004#1\n", "D.txt": "S004#2\n",
        "all.txt": "".join(f"S{i:03d}\n" for i in range(6)), "sub.txt": "".join(f"S{i:03d}\n" for i in range(1, 7)),
        "odd.txt": "S000\nS001#1\nS003\n", "one.txt": "S000#1\n", "solo.txt": "S000\n", "none.txt": "ZZZ\n", "mix.txt": "S000\nS006#1\n",
        "c.bed": "chr8\t10\t30\nchr3\t600\t620\nchrX\t5\t50\nchr8\t90\t110\n", "few.txt": "S001\nS002\n",
        "cores.txt": "# bp per BED row\n50\n650\n20\n150\n750\n", "cores_short.txt": "50\n650\n",
    }
    for name, text in files.items():
        with open(os.path.join(d, name), "w") as f:
            f.write(text)


M2 = ["--matrix", "chr3.npz", "chr8.npz", "--bed", "g.bed"]
M8 = ["--matrix", "chr8.npz", "--bed", "g.bed"]
MC = ["--matrix", "chr3.npz", "chr8.npz", "--bed", "c.bed"]  # short rows, for the formats that print a row per site or per pair
AB = ["-A", "A.txt", "-B", "B.txt"]
P2, P3, P4 = ["--panel", "A.txt", "B.txt"], ["--panel", "A.txt", "B.txt", "C.txt"], ["--panel", "A.txt", "B.txt", "C.txt", "D.txt"]
IHS_OPTS = ["--ihs-min-maf", "0.1", "--ihs-cutoff", "0.1", "--ihs-max-extend", "100", "--ihs-max-extend-sites", "10", "--ihs-bins", "4",
            "--ihs-keep-edge", "--compact"]


def invocations():
    """(name, argv behind the script's name)"""
    def f(fmt, *extra, mats=M2):
        return mats + ["--format", fmt] + [x for e in extra for x in (e if isinstance(e, list) else [e])]
    runs = [
        ("pica2", f("pica2")), ("pica2_rich", f("pica2", "-u", "sub.txt", "-t", "0.9990", "-r", "4", "--compact")),
        ("pica2_length", f("pica2", "--sequence-length", "777", "-o", "out.tsv")),
        ("hfst", f("hfst", AB)), ("hfst_rich", f("hfst", AB, "-r", "5", "--compact")), ("hfst_grouped", f("hfst", AB, "--fst-method", "grouped", "-t", "0.99")),
        ("hfst_panel", f("hfst", P3)), ("hfst_panel_r", f("hfst", P3, "-r", "5")), ("hfst_none", f("hfst")),
        ("tajd", f("tajd")), ("tajd_rich", f("tajd", "-l", "all.txt", "--compact")), ("tajd_panel", f("tajd", P3)),
        ("tajd_anon", f("tajd", mats=["--matrix", "anon.npz", "--bed", "g.bed"])),
        ("fst3pi", f("fst3pi", AB)), ("fst3pi_rich", f("fst3pi", AB, "-t", "0.99", "-r", "5")),
        ("all", f("all", AB, "-l", "all.txt")), ("all_rich", f("all", AB, "-l", "all.txt", "--fst-round-digits", "5", "--compact")),
        ("all_same_r", f("all", AB, "-r", "5", "--fst-round-digits", "5")), ("all_bare", f("all")), ("all_panel", f("all", P3)),
        ("all_panel_r", f("all", P3, "--fst-round-digits", "3", "-t", "0.99")),
        ("af", f("af")), ("af_rich", f("af", "-u", "sub.txt", "-t", "0.99", "-r", "3", "--af-clusters", "c.tsv", "--af-details", "d.tsv", "--compact")),
        ("ehh", f("ehh")), ("ehh_cores", f("ehh", "-u", "sub.txt", "--ehh-cores", "cores.txt", "--ehh-flanks", "two-sided")),
        ("ehh_offset_ref", f("ehh", "--ehh-core-offset", "5", "--ehh-ref", "S002#1#chr8:0-200", mats=M8)),
        ("hapstats", f("hapstats")), ("hapstats_rich", f("hapstats", "-u", "sub.txt", "--compact")),
        ("ld", f("ld")), ("ld_rich", f("ld", "-u", "sub.txt", "--ld-min-maf", "0.1", "--ld-max-sites", "16", "--compact", "-o", "out.tsv")),
        ("diploid", f("diploid")), ("diploid_rich", f("diploid", "-u", "odd.txt", "--roh-min-sites", "5", "--ind-table", "ind.tsv", "--compact")),
        ("ibs", f("ibs")), ("ibs_rich", f("ibs", "-u", "few.txt", "--ibs-min-sites", "5", "--ibs-segments", "seg.tsv", "--ibs-pair-table", "pt.tsv",
                                          "--compact", mats=MC)),
        ("ibs_diploid", f("ibs", "--ibs-pairs", "diploid", "-u", "odd.txt", "--ibs-min-sites", "5", "--ibs-segments", "seg.tsv")),
        ("dstat", f("dstat", P4)), ("dstat_rich", f("dstat", P4, "--quartet", "1,2,3,4", "--quartet", "2,1,3,4", "--dstat-polarize", "--dstat-summary",
                                                     "sum.tsv", "--dstat-blocks", "2", "--compact")),
        ("sfs", f("sfs", P2)), ("sfs_rich", f("sfs", P3, "--sfs-outgroup", "3", "--sfs-pair", "1,2", "--sfs-pairs-out", "sp.tsv", "--sfs-spectra",
                                               "sp.npz", "--sfs-blocks", "2", "--compact")),
        ("pairdist", f("pairdist", P2)), ("pairdist_rich", f("pairdist", P3, "--pairdist-outgroup", "3", "--pairdist-panels", "pp.tsv",
                                                            "--pairdist-hist", "ph.tsv", "--pairdist-bins", "8", "--pairdist-bin-width", "2",
                                                            "--compact", "-o", "out.tsv")),
        ("kinship", f("kinship")), ("kinship_rich", f("kinship", "-u", "sub.txt", "--kin-threshold", "0.05", "--kin-pairs", "kp.tsv", "--kin-watch",
                                                       "S001,S002", "--kin-watch", "S003,S001", "--kin-watch-table", "kw.tsv", "--compact")),
        ("ihs", f("ihs", mats=MC)), ("ihs_rich", f("ihs", "-u", "sub.txt", IHS_OPTS, "-o", "out.tsv", mats=MC)),
        ("xpehh", f("xpehh", P2, mats=MC)), ("xpehh_rich", f("xpehh", P2, IHS_OPTS, mats=MC)),
        # ---- the exits that depend on the data
        ("x_sfs_none", f("sfs", "--panel", "A.txt", "none.txt")),
        ("x_sfs_share", f("sfs", "--panel", "A.txt", "mix.txt", "--sfs-pair", "1,2", "--sfs-pairs-out", "sp.tsv")),
        ("x_dstat_none", f("dstat", "--panel", "A.txt", "B.txt", "none.txt", "D.txt")),
        ("x_dstat_share", f("dstat", "--panel", "A.txt", "mix.txt", "C.txt", "D.txt")),
        ("x_pairdist_none", f("pairdist", "--panel", "A.txt", "none.txt")), ("x_pairdist_share", f("pairdist", "--panel", "A.txt", "mix.txt")),
        ("x_xpehh_share", f("xpehh", "--panel", "A.txt", "mix.txt")), ("x_xpehh_few", f("xpehh", "--panel", "one.txt", "B.txt")),
        ("x_ihs_one", f("ihs", "-u", "one.txt")), ("x_hapstats_none", f("hapstats", "-u", "none.txt")), ("x_ld_none", f("ld", "-u", "none.txt")),
        ("x_diploid_unpaired", f("diploid", "-u", "one.txt")), ("x_ibs_unpaired", f("ibs", "--ibs-pairs", "diploid", "-u", "one.txt")),
        ("x_ibs_one", f("ibs", "-u", "one.txt")), ("x_kinship_few", f("kinship", "-u", "solo.txt")),
        ("x_kinship_watch", f("kinship", "--kin-watch", "S001,NOPE", "--kin-watch-table", "kw.tsv")),
        ("x_kinship_weights", f("kinship", mats=["--matrix", "weighted.npz", "--bed", "g.bed"])),
        ("x_ehh_ref", f("ehh", "--ehh-ref", "NOPE")), ("x_ehh_core", f("ehh", "--ehh-core-offset", "5000")),
        ("x_ehh_cores_short", f("ehh", "--ehh-cores", "cores_short.txt")),
        ("x_hfst_none", f("hfst", "-A", "A.txt", "-B", "none.txt")), ("x_fst3pi_bare", f("fst3pi")),
        ("x_fst3pi_share", f("fst3pi", "-A", "A.txt", "-B", "mix.txt")), ("x_tajd_one", f("tajd", "-l", "one.txt")),
        ("x_tajd_panel_one", f("tajd", "--panel", "A.txt", "one.txt")),
    ]
    for fmt, extra in (("tajd", []), ("pairdist", P2), ("kinship", []), ("ihs", [])):  # the front end's own exits, per way in
        runs.append((f"x_{fmt}_two_matrices", f(fmt, extra, mats=["--matrix", "chr8.npz", "chr8.npz", "--bed", "g.bed"])))
        runs.append((f"x_{fmt}_no_contig", f(fmt, extra, mats=["--matrix", "anon.npz", "chr3.npz", "--bed", "g.bed"])))
    return runs


INPUTS = ("chr3.npz", "chr8.npz", "anon.npz", "weighted.npz", "g.bed", "A.txt", "B.txt", "C.txt", "D.txt", "all.txt", "sub.txt", "odd.txt", "one.txt",
          "solo.txt", "none.txt", "mix.txt", "cores.txt", "cores_short.txt", "c.bed", "few.txt")


def pin(text):
    """a long text as its digest: compared byte for byte all the same"""
    return text if len(text) <= 4000 else f"sha256 {hashlib.sha256(text.encode()).hexdigest()} of {len(text)} characters"


def side_files(d):
    out = {}
    for name in sorted(os.listdir(d)):
        if name in INPUTS:
            continue
        path = os.path.join(d, name)
        if name.endswith(".npz"):
            with np.load(path) as z:
                out[name] = {k: [str(z[k].dtype), list(z[k].shape), int(z[k].sum())] for k in sorted(z.files)}
        else:
            with open(path, newline="") as f:
                out[name] = pin(f.read())
        os.remove(path)
    return out


def run_one(cli, d, argv):
    """one run of main() inside directory d -> what it wrote"""
    StandIn.calls = []
    cli.Runner = StandIn
    out, err = io.StringIO(), io.StringIO()
    keep = (sys.argv, os.getcwd(), os.environ.get("COLUMNS"))
    sys.argv = ["impop_scan.py"] + argv
    os.environ["COLUMNS"] = "100"
    os.chdir(d)
    try:
        with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
            try:
                cli.main()
                code = 0
            except SystemExit as e:
                code = e.code
    finally:
        sys.argv = keep[0]
        os.chdir(keep[1])
        if keep[2] is None:
            os.environ.pop("COLUMNS", None)
        else:
            os.environ["COLUMNS"] = keep[2]
    calls = json.loads(json.dumps(StandIn.calls))
    if code != 0:  # see the module's docstring: of a run that ends early only the device calls are pinned
        calls = [c for c in calls if c[0] not in ("Runner", "close")]
    return {"code": code, "stdout": pin(out.getvalue()), "stderr": err.getvalue(), "files": side_files(d), "calls": calls}


def record_all(d, script=SCAN):
    write_inputs(d)
    cli = load_cli(script)
    runs = {name: run_one(cli, d, argv) for name, argv in invocations()}
    runs["help"] = run_one(cli, d, ["--help"])
    return runs


@pytest.fixture(scope="module")
def replayed(tmp_path_factory):
    return record_all(str(tmp_path_factory.mktemp("scan_outputs")))


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_holds_every_invocation(recorded):
    assert os.path.getsize(FIXTURE) < 1024 * 1024
    assert list(recorded) == [name for name, _ in invocations()] + ["help"]
    for name, run in recorded.items():  # the runs that are meant to end early do, the others do not
        assert (run["code"] != 0) == name.startswith("x_"), (name, run["code"], run["stderr"][-300:])
    uploads = {name: sum(c[0] == "Runner" for c in run["calls"]) for name, run in recorded.items()}
    assert uploads["ld"] == uploads["kinship"] == uploads["all_panel"] == 2 and uploads["help"] == 0


@pytest.mark.parametrize("part", ("code", "stderr", "stdout", "files", "calls"))
def test_driver_writes_what_was_recorded(replayed, recorded, part):
    wrong = [name for name in recorded if replayed[name][part] != recorded[name][part]]
    if wrong:
        got, want = replayed[wrong[0]][part], recorded[wrong[0]][part]
        if isinstance(want, str):
            g, w = got.splitlines(), want.splitlines()
            k = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
            got, want = g[k:k + 2], w[k:k + 2]
        pytest.fail(f"{part} differs in {wrong}; the first: got {str(got)[:600]} want {str(want)[:600]}")


if __name__ == "__main__":
    import tempfile
    if sys.argv[1:2] != ["--write"] or len(sys.argv) > 3:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        runs = record_all(tmp, *sys.argv[2:])
    with open(FIXTURE, "w") as fh:
        json.dump(runs, fh, separators=(",", ":"))
        fh.write("\n")
    print(f"{len(runs)} runs, {os.path.getsize(FIXTURE)} bytes")
    for name, run in runs.items():
        print(f"{name:24s} code {run['code']}  calls {len(run['calls'])}  {run['stderr'].strip().splitlines()[-1][:110] if run['stderr'].strip() else ''}")
