"""No GPU: the host side of impop_dstat_scan — the header's known answer against the plain restatement, the ABI declaration and its
binding, the record layout on both sides, the block jackknife against a literal delete-one loop, and what scripts/impop_scan.py
refuses and prints for --format dstat."""
import ctypes as C
import importlib.util
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dstat_cases as dc
import plain_dstat as pd
from conftest import ROOT

SCAN = os.path.join(ROOT, "scripts", "impop_scan.py")
FIELDS = ["n_sites", "n_informative", "n_skipped", "flags", "abba", "baba", "f4_num", "fd_den_p2", "fd_den_p3", "d", "f4", "fd"]
OFFSETS = [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 72]


def load_cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("impop_scan_cli_dstat", SCAN)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    return mod


# ---- the definitions ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("polarize", (False, True))
def test_known_answer_of_the_header(polarize):
    rec = pd.reference(dc.known_matrix(), dc.KNOWN_POPS, dc.KNOWN_QUARTETS, [(0, 6)], polarize)
    for qi, q in enumerate(dc.KNOWN_QUARTETS):
        r = rec[0, qi]
        got = tuple(int(r[f]) for f in ("abba", "baba", "f4_num", "fd_den_p2", "fd_den_p3", "n_informative", "n_skipped"))
        assert got == dc.KNOWN_INTS[q] and int(r["n_sites"]) == 6 and int(r["flags"]) == 0
        assert (float(r["d"]), float(r["f4"]), float(r["fd"])) == dc.KNOWN_DOUBLES[q]
    assert float(rec[0, 0]["d"]) == 3.0 / 11.0 and float(rec[0, 0]["fd"]) == 0.3 and float(rec[0, 1]["fd"]) == -0.6
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    assert "(0,2,2,0) (2,0,2,0) (1,2,1,0) (0,1,2,0) (1,1,0,0) (2,2,2,2)" in header  # the case is stated in the header
    assert "abba 28, baba 16, f4_num -12, fd_den_p2 24, fd_den_p3 16, n_informative 4, n_skipped 0" in header
    assert "abba 16, baba 28, f4_num 12, fd_den_p2 12, fd_den_p3 8" in header


def test_restatement_details():
    # a polarisation tie is skipped and counted; a flipped site equals its mirror image; a donor tie goes to P2
    assert pd.site_terms((1, 1, 1, 1), (2, 2, 2, 2), True) == (0, 0, 0, 0, 0, 1)
    assert pd.site_terms((2, 0, 0, 2), (2, 2, 2, 2), True) == pd.site_terms((0, 2, 2, 0), (2, 2, 2, 2), False)
    t = pd.site_terms((0, 1, 2, 0), (2, 2, 4, 2), False)  # c2 n3 == c3 n2
    assert t[3] != 0 and t[4] == 0
    d, f4, fd = pd.doubles(0, 0, 0, 0, 0, (1, 2, 3, 4))
    assert math.isnan(d) and f4 == 0.0 and math.isnan(fd)
    # weights multiply the sums, not the site counters
    m = dc.known_matrix()
    a = pd.reference(m, dc.KNOWN_POPS, dc.KNOWN_QUARTETS, [(0, 6)], False)
    b = pd.reference(m, dc.KNOWN_POPS, dc.KNOWN_QUARTETS, [(0, 6)], False, weights=[3] * 6)
    assert (b["abba"] == 3 * a["abba"]).all() and (b["f4_num"] == 3 * a["f4_num"]).all() and (b["n_sites"] == 18).all()
    assert (b["n_informative"] == a["n_informative"]).all() and pd.bits_equal(b["d"], a["d"]).all()


def test_generators_are_not_hollow():
    for n in (8, 70):
        m, pops = dc.geometry_case(n)
        assert [len(p) for p in pops] == [n // 5, n // 4, n // 3, n - 1 - n // 5 - n // 4 - n // 3]
        assert len({h for p in pops for h in p}) == n - 1
        dc.assert_not_hollow(pd.reference(m, pops, dc.GEOMETRY_QUARTETS, dc.GEOMETRY_WINDOWS, False))
    with pytest.raises(AssertionError):
        dc.assert_not_hollow(np.zeros((2, 2), dtype=pd.STATS_DTYPE))


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------

def test_abi_declares_dstat_scan():
    import impop_amd
    from impop_amd import _lib
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    assert re.search(r"#define IMPOP_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    assert int(re.search(r"#define IMPOP_DSTAT_GROUP (\d+)u\b", header).group(1)) == _lib.DSTAT_GROUP
    assert int(re.search(r"#define IMPOP_DSTAT_MAX_QUARTETS (\d+)u\b", header).group(1)) == _lib.DSTAT_MAX_QUARTETS == 64
    for fn, n_args in (("impop_dstat_scan", 10), ("impop_ctx_dstat_elapsed", 3)):
        assert re.search(r"\bint %s\(" % fn, header) and len(_lib.SIGNATURES[fn][1]) == n_args
    assert re.search(r"typedef struct impop_dstat_stats \{\s*/\* 80 bytes", header)
    assert C.sizeof(_lib.DstatStats) == 80 and C.sizeof(_lib.DstatParams) == 16 and impop_amd.DSTAT_DTYPE.itemsize == 80
    assert pd.STATS_DTYPE == impop_amd.DSTAT_DTYPE
    assert [n for n, _ in _lib.DstatStats._fields_] == FIELDS == list(impop_amd.DSTAT_DTYPE.names)
    for name, off in zip(FIELDS, OFFSETS):  # the header's layout: 4 x uint32, 5 x int64, 3 x double
        assert getattr(_lib.DstatStats, name).offset == off == impop_amd.DSTAT_DTYPE.fields[name][1]
    assert [getattr(_lib.DstatParams, n).offset for n in ("struct_size", "polarize", "tile_blocks", "reserved")] == [0, 4, 8, 12]
    for struct, want in (("impop_dstat_stats", FIELDS), ("impop_dstat_params", ["struct_size", "polarize", "tile_blocks", "reserved"])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert declared == want
    assert hasattr(impop_amd.BitMatrix, "dstat_scan") and hasattr(impop_amd.Context, "dstat_elapsed")


def test_library_exports_both_symbols():
    from impop_amd import _lib
    assert os.path.exists(_lib.SO_PATH), "libimpop_hip.so is not built"
    lib = C.CDLL(_lib.SO_PATH)
    assert hasattr(lib, "impop_dstat_scan") and hasattr(lib, "impop_ctx_dstat_elapsed")
    assert lib.impop_version() == 4


# ---- the block jackknife --------------------------------------------------------------------------------------------------------------

def _literal_jackknife(num, den, B):
    n = len(num)
    base, extra = divmod(n, B)
    blocks, lo = [], 0
    for j in range(B):  # impop_shard_range: the first n % B blocks hold one more
        hi = lo + base + (1 if j < extra else 0)
        blocks.append((lo, hi))
        lo = hi
    N, D = sum(num), sum(den)
    theta = N / D
    if B == 1:  # deleting the one block leaves nothing
        return theta, float("nan"), float("nan")
    loo = []
    for lo, hi in blocks:
        loo.append((N - sum(num[lo:hi])) / (D - sum(den[lo:hi])))
    mean = sum(loo) / B
    se = math.sqrt((B - 1) / B * sum((t - mean) ** 2 for t in loo))
    return theta, se, theta / se if se else float("nan")


@pytest.mark.parametrize("n_windows", (7, 8, 64))
@pytest.mark.parametrize("n_blocks", (1, 3, 8))
def test_block_jackknife_is_the_delete_one_loop(n_windows, n_blocks):
    from impop_amd.dstat import block_jackknife
    rng = np.random.default_rng(100 * n_windows + n_blocks)
    abba = [int(x) for x in rng.integers(0, 10**12, n_windows)]
    baba = [int(x) for x in rng.integers(0, 10**12, n_windows)]
    if n_windows == 8:
        abba[2] = baba[2] = 0  # a window without an informative site stays in its block
    num = [a - b for a, b in zip(abba, baba)]
    den = [a + b for a, b in zip(abba, baba)]
    for as_float in (False, True):
        a = np.array(num, dtype=np.float64 if as_float else object)
        b = np.array(den, dtype=np.float64 if as_float else object)
        theta, se, z, B = block_jackknife(a, b, n_blocks)
        want = _literal_jackknife([float(x) for x in num] if as_float else num, [float(x) for x in den] if as_float else den, n_blocks)
        assert B == n_blocks
        if n_blocks == 1:  # one block: no delete-one value
            assert theta == want[0] and math.isnan(se) and math.isnan(z)
        else:
            assert (theta, se, z) == want


def test_block_jackknife_needs_two_blocks_with_a_denominator():
    from impop_amd.dstat import block_jackknife
    theta, se, z, B = block_jackknife(np.array([3.0, 0.0, 0.0, 0.0]), np.array([4.0, 0.0, 0.0, 0.0]), 4)
    assert theta == 0.75 and math.isnan(se) and math.isnan(z) and B == 4
    theta, se, z, B = block_jackknife(np.array([0, 0], dtype=object), np.array([0, 0], dtype=object), 2)
    assert math.isnan(theta) and math.isnan(se) and math.isnan(z)
    # blocks with a zero denominator are kept: B stays 4 in the variance
    num, den = np.array([3.0, 0.0, 1.0, 0.0]), np.array([4.0, 0.0, 5.0, 0.0])
    theta, se, z, B = block_jackknife(num, den, 4)
    loo = [(4.0 - 3.0) / (9.0 - 4.0), 4.0 / 9.0, (4.0 - 1.0) / (9.0 - 5.0), 4.0 / 9.0]
    mean = sum(loo) / 4
    assert B == 4 and se == math.sqrt(3 / 4 * sum((t - mean) ** 2 for t in loo)) and z == theta / se
    with pytest.raises(ValueError):
        block_jackknife(num, den, 0)


# ---- the driver -----------------------------------------------------------------------------------------------------------------------

def test_quartet_parsing():
    cli = load_cli()
    assert cli.parse_quartets(None, 4) == [(0, 1, 2, 3)]
    assert cli.parse_quartets(["2,1,3,4", "1,2,3,5"], 5) == [(1, 0, 2, 3), (0, 1, 2, 4)]
    for specs, n_panel, needle in ((["1,2,3,5"], 4, "position 5 is outside the 4 lists"), (["1,2,2,4"], 4, "named twice"),
                                   (["0,1,2,3"], 4, "position 0 is outside"), (["1,2,3"], 4, "four 1-based positions"),
                                   (["a,b,c,d"], 4, "four 1-based positions"), (None, 5, "say which four")):
        with pytest.raises(ValueError) as ei:
            cli.parse_quartets(specs, n_panel)
        assert needle in str(ei.value)


@pytest.mark.parametrize("extra,needle", [
    (["--panel", "a", "b", "c", "d", "--quartet", "1,2,3,5"], "position 5 is outside the 4 lists of --panel"),
    (["--panel", "a", "b", "c", "d", "e", "--quartet", "1,2,2,5"], "a population is named twice"),
    (["--panel", "a", "b", "c"], "4 to 8 population lists"),
    ([], "4 to 8 population lists"),
    (["--panel", "a", "b", "c", "d", "--devices", "2"], "not with --devices N"),
    (["--panel", "a", "b", "c", "d", "-u", "s.txt"], "not with -A / -B / -l / -u"),
    (["--panel", "a", "b", "c", "d", "--dstat-blocks", "5"], "go together"),
    (["--panel", "a", "b", "c", "d", "-r", "5"], "-t / -r / --identity belong to other formats"),
])
def test_driver_refuses_next_to_dstat(extra, needle):
    r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "dstat"] + extra,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and needle in r.stderr, (r.returncode, r.stderr[-500:])
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("Error: "), r.stderr[-500:]


def test_stray_dstat_options_are_refused():
    r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "ld", "--quartet", "1,2,3,4"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "belong to --format dstat" in r.stderr


def test_row_formatter_prints_the_known_answer():
    cli = load_cli()
    rec = pd.reference(dc.known_matrix(), dc.KNOWN_POPS, dc.KNOWN_QUARTETS, [(0, 6)], False)
    labels = ["afr", "eur", "eas", "chimp"]
    row = cli.dstat_row("CHM13#0#chr9:1000-1006", labels, (0, 1, 2, 3), [2, 2, 2, 2], rec[0, 0])
    assert row == "CHM13#0#chr9\t1000\t1006\tafr\teur\teas\tchimp\t6\t4\t0\t1.75000000\t1.00000000\t0.27272727\t-0.75000000\t0.30000000"
    row = cli.dstat_row("CHM13#0#chr9:1000-1006", labels, (1, 0, 2, 3), [2, 2, 2, 2], rec[0, 1])
    assert row.split("\t")[3:7] == ["eur", "afr", "eas", "chimp"] and row.split("\t")[-3:] == ["-0.27272727", "0.75000000", "-0.60000000"]
    empty = np.zeros(1, dtype=pd.STATS_DTYPE)[0]
    empty["d"] = empty["fd"] = float("nan")
    assert cli.dstat_row("c:1-2", labels, (0, 1, 2, 3), [2, 2, 2, 2], empty).split("\t")[-3:] == ["nan", "0.00000000", "nan"]
    assert cli.DSTAT_HEADER.split("\t") == ["CHROM", "START", "END", "P1", "P2", "P3", "O", "N_SITES", "N_INFORMATIVE", "N_SKIPPED", "ABBA",
                                            "BABA", "D", "F4", "F_D"]


class _Recorder:
    """stands in for impop_scan.Runner: records the calls, answers with the restatement"""
    calls = []

    def __init__(self, args, mf, windows, need_pairs, rank, world, local_rank):
        self.windows = windows
        _Recorder.calls.append(("init", need_pairs, bool(args.compact)))

    def dstat(self, pops, quartets, polarize):
        _Recorder.calls.append(("dstat", [np.flatnonzero(p).tolist() for p in pops], list(quartets), polarize))
        return pd.reference(dc.known_matrix(), [np.flatnonzero(p).tolist() for p in pops], quartets, [w[:2] for w in self.windows], polarize)

    def close(self):
        pass


def test_driver_prints_the_dstat_tables(tmp_path, capsys):
    import contextlib
    import io

    from impop_amd import matrixio
    names = [f"S{i}#1#chr9:1000-1006" for i in range(8)]
    matrixio.save_matrix(str(tmp_path / "m.npz"), matrixio.from_dense(dc.known_matrix(), names, origin=1000, contig="CHM13#0#chr9"))
    (tmp_path / "w.bed").write_text("chr9\t1000\t1006\nchr9\t1000\t1003\n")
    for k, label in enumerate(("afr", "eur", "eas", "chimp")):
        (tmp_path / f"{label}.txt").write_text("".join(f"S{h}#1\n" for h in dc.KNOWN_POPS[k]))
    (tmp_path / "mix.txt").write_text("S0#1\nS2#1\n")
    cli = load_cli()
    cli.Runner = _Recorder

    def run(extra):
        _Recorder.calls = []
        out, old = io.StringIO(), sys.argv
        sys.argv = [SCAN, "--matrix", str(tmp_path / "m.npz"), "--bed", str(tmp_path / "w.bed"), "--format", "dstat"] + extra
        try:
            with contextlib.redirect_stdout(out):
                cli.main()
        finally:
            sys.argv = old
        return out.getvalue().splitlines(), list(_Recorder.calls), capsys.readouterr().err

    panel = ["--panel"] + [str(tmp_path / f"{x}.txt") for x in ("afr", "eur", "eas", "chimp")]
    lines, calls, _ = run(panel)
    assert calls == [("init", False, False), ("dstat", dc.KNOWN_POPS, [(0, 1, 2, 3)], False)]
    assert lines[0] == cli.DSTAT_HEADER and len(lines) == 3
    assert lines[1] == "CHM13#0#chr9\t1000\t1006\tafr\teur\teas\tchimp\t6\t4\t0\t1.75000000\t1.00000000\t0.27272727\t-0.75000000\t0.30000000"
    summary = tmp_path / "sum.tsv"
    lines, calls, _ = run(panel + ["--quartet", "1,2,3,4", "--quartet", "2,1,3,4", "--dstat-polarize", "--compact", "--dstat-blocks", "2",
                                   "--dstat-summary", str(summary)])
    assert calls == [("init", False, True), ("dstat", dc.KNOWN_POPS, [(0, 1, 2, 3), (1, 0, 2, 3)], True)] and len(lines) == 5
    assert [ln.split("\t")[3:5] for ln in lines[1:]] == [["afr", "eur"], ["eur", "afr"]] * 2  # window-major, a row per quartet
    rows = summary.read_text().splitlines()
    assert rows[0] == cli.DSTAT_SUMMARY_HEADER and len(rows) == 3 and rows[1].split("\t")[:4] == ["afr", "eur", "eas", "chimp"]
    assert rows[1].split("\t")[9] == "2" and rows[2].split("\t")[4].startswith("-")
    # populations of a quartet that share a sequence: an error exit naming the lists
    with pytest.raises(SystemExit) as ei:
        run(["--panel"] + [str(tmp_path / f"{x}.txt") for x in ("afr", "mix", "eas", "chimp")])
    assert ei.value.code == 2 and "afr and mix share a sequence" in capsys.readouterr().err
