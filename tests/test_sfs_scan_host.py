"""No GPU: the host side of impop_sfs_scan — the header's known answer against the plain restatement, the ABI declaration and its
binding, the record layouts on both sides, the library's host arithmetic (impop_sfs_neutrality) against the restatement bit for
bit, the NaN rules, the host companions, csrc/sfs_math.h's part cutter and table offsets under ASan + UBSan
(tests/fuzz/sfs_host.cc), and what scripts/impop_scan.py refuses, prints and writes for --format sfs."""
import ctypes as C
import importlib.util
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import plain_sfs as ps
import sfs_cases as sc
from conftest import ROOT

SCAN = os.path.join(ROOT, "scripts", "impop_scan.py")
FIELDS = ["n_sites", "seg", "eta1", "eta_n1", "n_skipped", "flags", "sum_het", "sum_c", "sum_c2", "theta_w", "theta_pi", "theta_h", "theta_l",
          "tajima_d", "faywu_h", "faywu_h_norm", "zeng_e"]
OFFSETS = [0, 4, 8, 12, 16, 20, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96, 104]
PAIR_FIELDS = ["private_a", "private_b", "shared", "fixed_a", "fixed_b", "n_union", "n_skipped", "flags"]
PARAM_FIELDS = ["struct_size", "outgroup", "tile_blocks", "tables", "max_chunk_bytes"]


def load_cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("impop_scan_cli_sfs", SCAN)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    return mod


def known_reference(outgroup):
    return ps.reference(sc.known_matrix(), sc.KNOWN_POPS, sc.KNOWN_PAIRS, [sc.KNOWN_WINDOW], outgroup)


# ---- the definitions ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("outgroup", (None, 2))
def test_known_answer_of_the_header(outgroup):
    sc.assert_known(known_reference(outgroup), outgroup)
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    assert "(1,0,0) (2,1,0) (5,0,0) (0,4,0) (1,1,1) (3,5,2) (0,0,0) (5,5,2) (0,0,1) (4,2,0) (0,5,2)" in header  # the case is in the header
    assert "A 5 2 1 24 11 31, B 4 2 1 18 8 22" in header and "A 4 1 1 20 9 25" in header and "B 3 1 1 14 7 21" in header
    assert "private_a 2, private_b 1, shared 3, fixed_a 1, fixed_b 1, n_union 8" in header
    assert "private_a 2, private_b 1, shared 2, fixed_a 2, fixed_b 0, n_union 7" in header
    for digits in ("-0.41017465", "-0.34892049", "0.13767880", "0.27344977", "-0.43615061", "0.56792505"):
        assert digits in header


def test_restatement_details():
    # a tie adds to n_skipped and to nothing else; a monomorphic site is never a tie; weights multiply the sums, not the counters
    m = sc.known_matrix()
    a = ps.reference(m, sc.KNOWN_POPS, sc.KNOWN_PAIRS, [sc.KNOWN_WINDOW], 2)
    ties = [s for s, c in enumerate(sc.KNOWN_COUNTS) if 2 * c[2] == 2]
    assert ties == [4, 8] and int(a[0][0, 0]["n_skipped"]) == 2
    no_ties = ps.reference(np.delete(m, ties, axis=1), sc.KNOWN_POPS, sc.KNOWN_PAIRS, [(0, 9)], 2)
    for f in sc.INT_FIELDS:
        assert (no_ties[0][f] == a[0][f]).all()
    assert (no_ties[3][0] == a[3][0]).all()
    b = ps.reference(m, sc.KNOWN_POPS, sc.KNOWN_PAIRS, [sc.KNOWN_WINDOW], 2, weights=[3] * 11)
    for f in ("sum_het", "sum_c", "sum_c2"):
        assert (b[0][f] == 3 * a[0][f]).all()
    for f in ("seg", "eta1", "eta_n1", "n_skipped"):
        assert (b[0][f] == a[0][f]).all()
    assert (b[0]["n_sites"] == 33).all() and (b[2][0] == a[2][0]).all() and (b[3][0] == a[3][0]).all()
    ps.assert_records(b[1], a[1])
    # sum_het = n sum_c - sum_c2, and the pair's n_union is its table's total
    for st, n in zip(a[0][0], (5, 5, 2)):
        assert int(st["sum_het"]) == n * int(st["sum_c"]) - int(st["sum_c2"])
    assert int(a[3][0].sum()) == int(a[1][0, 0]["n_union"])


def test_generators_are_not_hollow():
    for n in (12, 70):
        m, pops = sc.geometry_case(n)
        o = 2 * max(1, n // 16)
        assert [len(p) for p in pops] == [n // 4, n // 3, n - 1 - n // 4 - n // 3 - o, o] and o % 2 == 0
        assert len({h for p in pops for h in p}) == n - 1
        for og in (None, sc.GEOMETRY_OUTGROUP):
            ref = ps.reference(m, pops, sc.GEOMETRY_PAIRS, sc.GEOMETRY_WINDOWS, og)
            sc.assert_not_hollow(ref, og, sum(ps.polarized_counts(m, pops, og)[2]))
    hollow = (np.zeros((2, 2), dtype=ps.STATS_DTYPE), np.zeros((2, 1), dtype=ps.PAIR_DTYPE), [], [np.zeros((2, 3, 3), np.uint32)])
    with pytest.raises(AssertionError):
        sc.assert_not_hollow(hollow, None)
    # populations of 2 and 3 make some variances exactly zero: NaN ratios next to finite thetas
    m, pops = sc.geometry_case(12)
    st = ps.reference(m, pops, [], [(0, 2100)], None)[0][0]
    assert [len(p) for p in pops[:3]] == [3, 4, 2]
    assert math.isnan(st[2]["tajima_d"]) and math.isnan(st[2]["faywu_h_norm"]) and st[2]["seg"] > 0 and st[2]["theta_w"] > 0
    assert math.isnan(st[0]["tajima_d"]) or math.isnan(st[0]["zeng_e"]) or math.isnan(st[0]["faywu_h_norm"])
    assert not math.isnan(st[1]["tajima_d"])


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------

def test_abi_declares_sfs_scan():
    import impop_amd
    from impop_amd import _lib
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    assert re.search(r"#define IMPOP_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    assert int(re.search(r"#define IMPOP_SFS_PAIR_GROUP (\d+)u\b", header).group(1)) == _lib.SFS_PAIR_GROUP
    assert int(re.search(r"#define IMPOP_SFS_MAX_PAIRS (\d+)u\b", header).group(1)) == _lib.SFS_MAX_PAIRS == 28
    assert int(re.search(r"#define IMPOP_SFS_TABLE_1D (\d+)u\b", header).group(1)) == _lib.SFS_TABLE_1D == 1
    assert int(re.search(r"#define IMPOP_SFS_TABLE_JOINT (\d+)u\b", header).group(1)) == _lib.SFS_TABLE_JOINT == 2
    for fn, n_args in (("impop_sfs_scan", 13), ("impop_sfs_neutrality", 6), ("impop_ctx_sfs_elapsed", 3)):
        assert re.search(r"^int %s\(" % fn, header, re.M) and len(_lib.SIGNATURES[fn][1]) == n_args
    assert re.search(r"typedef struct impop_sfs_stats \{\s*/\* 112 bytes", header)
    assert re.search(r"typedef struct impop_sfs_pair \{\s*/\* 32 bytes", header)
    assert re.search(r"typedef struct impop_sfs_params \{\s*/\* 24 bytes", header)
    assert C.sizeof(_lib.SfsStats) == 112 and C.sizeof(_lib.SfsPair) == 32 and C.sizeof(_lib.SfsParams) == 24
    assert impop_amd.SFS_DTYPE.itemsize == 112 and impop_amd.SFS_PAIR_DTYPE.itemsize == 32
    assert ps.STATS_DTYPE == impop_amd.SFS_DTYPE and ps.PAIR_DTYPE == impop_amd.SFS_PAIR_DTYPE
    assert [n for n, _ in _lib.SfsStats._fields_] == FIELDS == list(impop_amd.SFS_DTYPE.names)
    for name, off in zip(FIELDS, OFFSETS):  # the header's layout: 6 x uint32, 3 x uint64, 8 x double
        assert getattr(_lib.SfsStats, name).offset == off == impop_amd.SFS_DTYPE.fields[name][1]
    assert [n for n, _ in _lib.SfsPair._fields_] == PAIR_FIELDS == list(impop_amd.SFS_PAIR_DTYPE.names)
    for i, name in enumerate(PAIR_FIELDS):
        assert getattr(_lib.SfsPair, name).offset == 4 * i == impop_amd.SFS_PAIR_DTYPE.fields[name][1]
    assert [getattr(_lib.SfsParams, n).offset for n in PARAM_FIELDS] == [0, 4, 8, 12, 16]
    for struct, want in (("impop_sfs_stats", FIELDS), ("impop_sfs_pair", PAIR_FIELDS), ("impop_sfs_params", PARAM_FIELDS)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert declared == want
    assert hasattr(impop_amd.BitMatrix, "sfs_scan") and hasattr(impop_amd.Context, "sfs_elapsed")


def test_library_exports_the_symbols():
    from impop_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "libimpop_hip.so is not built"
    lib = C.CDLL(_lib.SO_PATH)
    assert hasattr(lib, "impop_sfs_scan") and hasattr(lib, "impop_sfs_neutrality") and hasattr(lib, "impop_ctx_sfs_elapsed")
    assert lib.impop_version() == 4


# ---- the host arithmetic: the library's one routine against the restatement, bit for bit ------------------------------------------------

def _library_doubles(n, seg, sum_het, sum_c, sum_c2):
    from impop_amd import _lib
    out = (C.c_double * 8)()
    assert _lib.load().impop_sfs_neutrality(n, seg, sum_het, sum_c, sum_c2, out) == 0
    return [float(x) for x in out]


def _integers_for(n, S, rng):
    """S segregating sites of n sequences: plausible sums (n = 1 cannot segregate: the sums are then arbitrary)"""
    c = [int(x) for x in rng.integers(1, max(n, 2), S)]
    return sum(x * (n - x) for x in c) if n > 1 else 0, sum(c), sum(x * x for x in c)


@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 58, 465, 65535))
def test_neutrality_equals_the_restatement_bit_for_bit(n):
    rng = np.random.default_rng(50 + n)
    for S in (0, 1, 2, 2543):
        for _ in range(3):
            het, sc_, sc2 = _integers_for(n, S, rng)
            got, want = _library_doubles(n, S, het, sc_, sc2), ps.doubles(n, S, het, sc_, sc2)
            assert ps.bits_equal(got, want).all(), (n, S, got, want)


def test_neutrality_of_the_known_case():
    from impop_amd import sfs
    for og in (None, 2):
        st = known_reference(og)[0][0]
        for k, n in enumerate((5, 5, 2)):
            ints = tuple(int(st[k][f]) for f in ("seg", "sum_het", "sum_c", "sum_c2"))
            got = _library_doubles(n, *ints)
            assert ps.bits_equal(got, [st[k][f] for f in ps.DOUBLE_FIELDS]).all(), (og, k)
            d = sfs.neutrality(n, *ints)
            assert list(d) == list(ps.DOUBLE_FIELDS) and ps.bits_equal(list(d.values()), got).all()
            for (o, kk, f), v in sc.KNOWN_DIGITS.items():
                if o == og and kk == k:
                    assert abs(d[f] - v) < 1e-8


def test_nan_rules():
    nan = math.isnan
    assert all(nan(x) for x in _library_doubles(1, 0, 0, 0, 0)) and all(nan(x) for x in _library_doubles(0, 3, 1, 1, 1))
    assert all(nan(x) for x in ps.doubles(1, 0, 0, 0, 0))
    # S == 0: the thetas and Fay & Wu's H are 0, the three ratios NaN
    tw, tp, th, tl, d, h, hn, e = _library_doubles(58, 0, 0, 0, 0)
    assert (tw, tp, th, tl, h) == (0.0, 0.0, 0.0, 0.0, 0.0) and nan(d) and nan(hn) and nan(e)
    # n = 2: every variance is exactly 0 (one site, c = 1)
    tw, tp, th, tl, d, h, hn, e = _library_doubles(2, 1, 1, 1, 1)
    assert (tw, tp, th, tl, h) == (1.0, 1.0, 1.0, 1.0, 0.0) and nan(d) and nan(hn) and nan(e)
    # n = 3, S = 1: Tajima's variance is e1 S + e2 S (S - 1) with e1 = 0 exactly
    got = _library_doubles(3, 1, 2, 1, 1)
    assert nan(got[4]) and ps.bits_equal(got, ps.doubles(3, 1, 2, 1, 1)).all()
    # a healthy case has none
    assert not any(nan(x) for x in _library_doubles(58, 100, 40000, 1500, 30000))
    from impop_amd import _lib
    assert _lib.load().impop_sfs_neutrality(5, 1, 4, 1, 1, None) == -1


# ---- the host companions ----------------------------------------------------------------------------------------------------------------

def test_fold_and_block_sums():
    from impop_amd import sfs
    assert sfs.fold([0, 5, 3, 2, 0]).tolist() == [0, 7, 3]        # n = 4: the middle bin once
    assert sfs.fold([0, 5, 3, 2, 1, 0]).tolist() == [0, 6, 5]     # n = 5
    assert sfs.fold(np.array([[0, 1, 0], [0, 4, 0]])).tolist() == [[0, 1], [0, 4]]
    rng = np.random.default_rng(7)
    for n_windows, B in ((7, 1), (7, 3), (8, 8), (64, 5), (2, 4)):
        t = rng.integers(0, 2**32, (n_windows, 3, 4), dtype=np.uint64).astype(np.uint32)
        got = sfs.block_sums(t, B)
        base, extra = divmod(n_windows, B)
        lo = 0
        for j in range(B):  # impop_shard_range: the first n % B blocks hold one more
            hi = lo + base + (1 if j < extra else 0)
            want = np.zeros((3, 4), dtype=object)
            for w in range(lo, hi):
                want = want + t[w].astype(object)
            assert (got[j].astype(object) == want).all()
            lo = hi
        assert got.dtype == np.uint64 and got.shape == (B, 3, 4) and lo == n_windows
    with pytest.raises(ValueError):
        sfs.block_sums(t, 0)


# ---- csrc/sfs_math.h under the sanitizers ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sfs_host_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("sfs_host") / "sfs_host")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "sfs_host.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-4000:])
    return r.stdout.strip()


# (part_tiles, tile ranges of the windows): the driver's line, items as window:tiles
PART_CASES = {
    "equal_shares": (4, [(0, 9)], "items=3 sizes=0:3,0:3,0:3"),                     # 9 tiles under 4: ceil(9 / 4) = 3 parts of 3
    "short_tail": (4, [(0, 10)], "items=3 sizes=0:4,0:4,0:2"),                      # 3 parts of ceil(10 / 3) = 4, the last 2
    "windows_without_tiles": (4, [(5, 5), (3, 8), (0, 0), (7, 8)], "items=3 sizes=1:3,1:2,3:1"),
    "one_tile_parts": (1, [(2, 5)], "items=3 sizes=0:1,0:1,0:1"),
    "overlap": (2, [(0, 3), (1, 4)], "items=4 sizes=0:2,0:1,1:2,1:1"),             # overlapping windows share tiles, not items
}


@pytest.mark.parametrize("case", sorted(PART_CASES))
def test_part_cutter(sfs_host_exe, case):
    """The driver checks the cut itself (every tile of every window in exactly one part, parts within their bound, equal shares)
    and exits non-zero on a breach; here: it ran clean under the sanitizers and cut where the case's arithmetic says."""
    part_tiles, wins, line = PART_CASES[case]
    assert _run(sfs_host_exe, "parts", part_tiles, *[x for w in wins for x in w]) == line


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_parts_and_offsets_on_random_lists(sfs_host_exe, seed):
    assert _run(sfs_host_exe, "random", seed, 300) == "random ok lists=300"


# ---- the driver -----------------------------------------------------------------------------------------------------------------------

def test_pair_parsing():
    cli = load_cli()
    assert cli.parse_sfs_pairs(None, 3) == [] and cli.parse_sfs_pairs(["2,1", "1,3"], 3) == [(1, 0), (0, 2)]
    for specs, n_panel, needle in ((["1,4"], 3, "position 4 is outside the 3 lists"), (["2,2"], 3, "named twice"),
                                   (["0,1"], 3, "position 0 is outside"), (["1,2,3"], 3, "two 1-based positions"),
                                   (["a,b"], 3, "two 1-based positions"), (["1,2"] * 29, 3, "at most 28 pairs")):
        with pytest.raises(ValueError) as ei:
            cli.parse_sfs_pairs(specs, n_panel)
        assert needle in str(ei.value)


@pytest.mark.parametrize("extra,needle", [
    ([], "1 to 8 population lists"),
    (["--panel"] + list("abcdefghi"), "1 to 8 population lists"),
    (["--panel", "a", "b", "--sfs-pair", "1,3", "--sfs-pairs-out", "p.tsv"], "position 3 is outside the 2 lists of --panel"),
    (["--panel", "a", "b", "--sfs-pair", "1,1", "--sfs-pairs-out", "p.tsv"], "a population is named twice"),
    (["--panel", "a", "b", "--sfs-outgroup", "3"], "--sfs-outgroup 3: position is outside the 2 lists"),
    (["--panel", "a", "b", "--sfs-outgroup", "0"], "--sfs-outgroup 0: position is outside"),
    (["--panel", "a", "b", "--sfs-pairs-out", "p.tsv"], "needs at least one --sfs-pair"),
    (["--panel", "a", "b", "--sfs-pair", "1,2"], "goes with --sfs-pairs-out PATH or --sfs-spectra"),
    (["--panel", "a", "--sfs-blocks", "2"], "--sfs-blocks N belongs to --sfs-spectra"),
    (["--panel", "a", "--sfs-spectra", "s.npz", "--sfs-blocks", "0"], "--sfs-blocks takes 1 or more"),
    (["--panel", "a", "b", "--devices", "2"], "not with --devices N"),
    (["--panel", "a", "b", "-u", "s.txt"], "not with -A / -B / -l / -u"),
    (["--panel", "a", "b", "-r", "5"], "-t / -r / --identity belong to other formats"),
])
def test_driver_refuses_next_to_sfs(extra, needle):
    r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "sfs"] + extra,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and needle in r.stderr, (r.returncode, r.stderr[-500:])
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("Error: "), r.stderr[-500:]


@pytest.mark.parametrize("stray", (["--sfs-outgroup", "1"], ["--sfs-pair", "1,2"], ["--sfs-pairs-out", "p"], ["--sfs-spectra", "s.npz"],
                                   ["--sfs-blocks", "2"]))
def test_stray_sfs_options_are_refused(stray):
    r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "ld"] + stray,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "belong to --format sfs" in r.stderr


def test_row_formatter_prints_the_known_answer():
    cli = load_cli()
    stats, prec, _, _ = known_reference(None)
    row = cli.sfs_row("CHM13#0#chr9:1000-1011", "eur", 5, stats[0, 1]).split("\t")
    assert row[:10] == ["CHM13#0#chr9", "1000", "1011", "eur", "5", "11", "4", "2", "1", "0"]
    assert row[10:] == ["1.92000000", "1.80000000", "2.20000000", "2.00000000", "-0.41017465", "-0.40000000", "-0.34892049", "0.13767880"]
    row = cli.sfs_row("c:1-2", "o", 1, _nan_record()).split("\t")
    assert row[10:] == ["nan"] * 8
    assert cli.sfs_pair_row("CHM13#0#chr9:1000-1011", "afr", "eur", prec[0, 0]) == "CHM13#0#chr9\t1000\t1011\tafr\teur\t2\t1\t3\t1\t1\t8"
    assert cli.SFS_HEADER.split("\t") == ["CHROM", "START", "END", "POP", "N", "N_SITES", "S", "ETA1", "ETA_N1", "N_SKIPPED", "THETA_W",
                                         "THETA_PI", "THETA_H", "THETA_L", "TAJIMA_D", "FAYWU_H", "FAYWU_H_NORM", "ZENG_E"]
    assert cli.SFS_PAIRS_HEADER.split("\t")[3:] == ["POP_A", "POP_B", "PRIVATE_A", "PRIVATE_B", "SHARED", "FIXED_A", "FIXED_B", "N_UNION"]


def _nan_record():
    r = np.zeros(1, dtype=ps.STATS_DTYPE)
    for f in ps.DOUBLE_FIELDS:
        r[f] = float("nan")
    return r[0]


class _Recorder:
    """stands in for impop_scan.Runner: records the calls, answers with the restatement"""
    calls = []

    def __init__(self, args, mf, windows, need_pairs, rank, world, local_rank):
        self.windows = windows
        _Recorder.calls.append(("init", need_pairs, bool(args.compact)))

    def sfs(self, pops, pairs, outgroup, tables, w0, w1):
        members = [np.flatnonzero(p).tolist() for p in pops]
        _Recorder.calls.append(("sfs", members, list(pairs), outgroup, tuple(tables), w0, w1))
        st, pr, sfs, jsfs = ps.reference(sc.known_matrix(), members, pairs, [w[:2] for w in self.windows[w0:w1]], outgroup)
        return st, pr, sfs if "sfs" in tables else None, jsfs if "jsfs" in tables else None

    def close(self):
        pass


def test_driver_prints_the_sfs_tables(tmp_path, capsys):
    import contextlib
    import io

    from impop_amd import matrixio
    names = [f"S{i}#1#chr9:1000-1011" for i in range(12)]
    matrixio.save_matrix(str(tmp_path / "m.npz"), matrixio.from_dense(sc.known_matrix(), names, origin=1000, contig="CHM13#0#chr9"))
    bed_rows = [(1000, 1011), (1000, 1004), (1004, 1011), (1002, 1009), (1010, 1011)]
    (tmp_path / "w.bed").write_text("".join(f"chr9\t{a}\t{b}\n" for a, b in bed_rows))
    for k, label in enumerate(("afr", "eur", "chimp")):
        (tmp_path / f"{label}.txt").write_text("".join(f"S{h}#1\n" for h in sc.KNOWN_POPS[k]))
    (tmp_path / "mix.txt").write_text("S0#1\nS5#1\n")
    cli = load_cli()
    cli.Runner = _Recorder

    def run(extra):
        _Recorder.calls = []
        out, old = io.StringIO(), sys.argv
        sys.argv = [SCAN, "--matrix", str(tmp_path / "m.npz"), "--bed", str(tmp_path / "w.bed"), "--format", "sfs"] + extra
        try:
            with contextlib.redirect_stdout(out):
                cli.main()
        finally:
            sys.argv = old
        return out.getvalue().splitlines(), list(_Recorder.calls), capsys.readouterr().err

    panel = ["--panel"] + [str(tmp_path / f"{x}.txt") for x in ("afr", "eur", "chimp")]
    lines, calls, _ = run(panel)
    assert calls == [("init", False, False), ("sfs", sc.KNOWN_POPS, [], None, (), 0, 5)]
    assert lines[0] == cli.SFS_HEADER and len(lines) == 1 + 5 * 3
    assert lines[2] == ("CHM13#0#chr9\t1000\t1011\teur\t5\t11\t4\t2\t1\t0\t1.92000000\t1.80000000\t2.20000000\t2.00000000\t-0.41017465\t"
                        "-0.40000000\t-0.34892049\t0.13767880")
    assert [ln.split("\t")[3] for ln in lines[1:4]] == ["afr", "eur", "chimp"]  # window-major, a row per population
    # one population is a panel too
    lines, calls, _ = run(panel[:2])
    assert calls[1] == ("sfs", sc.KNOWN_POPS[:1], [], None, (), 0, 5) and len(lines) == 6
    # pairs, the outgroup (1-based on the command line), --compact, the spectra in blocks, scanned in batches of rows
    cli.SFS_BATCH_ROWS = 2
    pairs_out, spectra = tmp_path / "pairs.tsv", tmp_path / "s.npz"
    lines, calls, _ = run(panel + ["--sfs-pair", "1,2", "--sfs-pair", "2,1", "--sfs-outgroup", "3", "--compact", "--sfs-pairs-out",
                                   str(pairs_out), "--sfs-spectra", str(spectra), "--sfs-blocks", "2"])
    assert calls[0] == ("init", False, True)
    assert [c[3:] for c in calls[1:]] == [(2, ("sfs", "jsfs"), 0, 2), (2, ("sfs", "jsfs"), 2, 4), (2, ("sfs", "jsfs"), 4, 5)]
    assert all(c[2] == [(0, 1), (1, 0)] for c in calls[1:])
    assert lines[1].split("\t")[9] == "2" and lines[1].split("\t")[6] == "4"  # the first row with the outgroup: 2 ties, S = 4
    rows = pairs_out.read_text().splitlines()
    assert rows[0] == cli.SFS_PAIRS_HEADER and len(rows) == 1 + 5 * 2
    assert rows[1] == "CHM13#0#chr9\t1000\t1011\tafr\teur\t2\t1\t2\t2\t0\t7" and rows[2].split("\t")[3:7] == ["eur", "afr", "1", "2"]
    # the block sums against a literal loop over the rows' own tables: blocks of 3 and 2 rows (impop_shard_range)
    wins = [(a - 1000, b - 1000) for a, b in bed_rows]
    _, _, sfs, jsfs = ps.reference(sc.known_matrix(), sc.KNOWN_POPS, [(0, 1), (1, 0)], wins, 2)
    z = np.load(spectra)
    assert sorted(z.files) == ["jsfs_afr_eur", "jsfs_eur_afr", "sfs_afr", "sfs_chimp", "sfs_eur"]
    for name, t in (("sfs_afr", sfs[0]), ("sfs_eur", sfs[1]), ("sfs_chimp", sfs[2]), ("jsfs_afr_eur", jsfs[0]), ("jsfs_eur_afr", jsfs[1])):
        want = np.zeros((2,) + t.shape[1:], dtype=np.uint64)
        for row in range(5):
            want[0 if row < 3 else 1] += t[row]
        assert z[name].dtype == np.uint64 and (z[name] == want).all(), name
    assert int(z["jsfs_afr_eur"][0].sum()) > 0 and (z["jsfs_afr_eur"] == z["jsfs_eur_afr"].transpose(0, 2, 1)).all()
    # one block by default: the genome-wide spectra
    lines, calls, _ = run(panel + ["--sfs-spectra", str(spectra)])
    z = np.load(spectra)
    assert sorted(z.files) == ["sfs_afr", "sfs_chimp", "sfs_eur"] and z["sfs_afr"].shape == (1, 6)
    assert (z["sfs_afr"][0] == ps.reference(sc.known_matrix(), sc.KNOWN_POPS, [], wins, None)[2][0].sum(axis=0)).all()
    assert all(c[4] == ("sfs",) for c in calls[1:])
    # the populations of a pair that share a sequence: an error exit naming the lists
    with pytest.raises(SystemExit) as ei:
        run(["--panel", str(tmp_path / "afr.txt"), str(tmp_path / "mix.txt"), "--sfs-pair", "1,2", "--sfs-pairs-out", str(pairs_out)])
    assert ei.value.code == 2 and "afr and mix share a sequence" in capsys.readouterr().err
