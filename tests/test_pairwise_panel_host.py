"""No GPU: the host side of impop_pairwise_scan_panel — the ABI declaration and its binding, the record sizes, what
scripts/impop_scan.py refuses next to --panel, and which call each --panel form of the driver takes (a recording stand-in for
the Runner: no device is opened)."""
import contextlib
import importlib.util
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

SCAN = os.path.join(ROOT, "scripts", "impop_scan.py")


def load_cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("impop_scan_cli_panel", SCAN)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    return mod


def test_abi_declares_pairwise_scan_panel():
    import ctypes as C
    import impop_amd
    from impop_amd import _lib
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    assert re.search(r"#define IMPOP_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    assert re.search(r"\bint impop_pairwise_scan_panel\(", header) and "impop_pairwise_scan_panel" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["impop_pairwise_scan_panel"][1]) == 10
    assert C.sizeof(_lib.PanelStats) == 48 and C.sizeof(_lib.PanelWindow) == 8
    assert impop_amd.PANEL_DTYPE.itemsize == 48 and impop_amd.PANEL_WINDOW_DTYPE.itemsize == 8
    assert [n for n, _ in _lib.PanelStats._fields_] == list(impop_amd.PANEL_DTYPE.names)
    assert [n for n, _ in _lib.PanelWindow._fields_] == list(impop_amd.PANEL_WINDOW_DTYPE.names)
    for name, ct in _lib.PanelStats._fields_:  # same offsets on both sides
        assert getattr(_lib.PanelStats, name).offset == impop_amd.PANEL_DTYPE.fields[name][1]
    if os.path.exists(_lib.SO_PATH):
        assert hasattr(C.CDLL(_lib.SO_PATH), "impop_pairwise_scan_panel")


@pytest.mark.parametrize("extra,env,needle", [
    (["--format", "tajd", "--devices", "2"], {}, "--devices N"),
    (["--format", "hfst", "-r", "5", "--fst-method", "grouped"], {}, "--fst-method grouped"),
    (["--format", "tajd", "-l", "s.txt"], {}, "not with -l"),
    (["--format", "pica2"], {}, "--panel belongs to --format hfst"),
    (["--format", "hfst", "-r", "5"], {"WORLD_SIZE": "2", "RANK": "0"}, "not under torch.distributed.run"),
    (["--format", "all"], {"WORLD_SIZE": "2", "RANK": "1"}, "not under torch.distributed.run"),
])
def test_driver_refuses_next_to_panel(extra, env, needle):
    r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--panel", "A.txt", "B.txt", "--backend", "gloo"] + extra,
                       capture_output=True, text=True, env=dict(os.environ, **env), timeout=120)
    assert r.returncode == 2 and needle in r.stderr, (r.returncode, r.stderr[-500:])


def test_driver_refuses_sim_list_and_bad_panel_counts():
    r = subprocess.run([sys.executable, SCAN, "--sim-list", "none.tsv", "--format", "tajd", "--panel", "A.txt", "B.txt"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--sim-list has no --panel" in r.stderr, r.stderr[-500:]
    r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "tajd", "--panel", "A.txt"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "2 to 8 population lists" in r.stderr, r.stderr[-500:]


class _Recorder:
    """stands in for impop_scan.Runner: records the calls, returns records that name their source"""
    calls = []

    def __init__(self, args, mf, windows, need_pairs, rank, world, local_rank):
        self.n = len(windows)
        self.need_pairs = need_pairs
        _Recorder.calls.append(("init", need_pairs))

    def panel(self, pops):
        import impop_amd
        _Recorder.calls.append(("scan_multi", len(pops)))
        K = len(pops)
        out = np.zeros((self.n, K * (K - 1) // 2), dtype=impop_amd.PAIR_DTYPE)
        out["fst"] = 0.125
        return out

    def panel_allpairs(self, pops, threshold, round_digits, want_s, want_pairs):
        import impop_amd
        _Recorder.calls.append(("panel", len(pops), threshold, round_digits, want_s, want_pairs))
        K = len(pops)
        pan = np.zeros((self.n, K), dtype=impop_amd.PANEL_DTYPE)
        pan["pi_site"] = 0.00123456789
        pan["tajima_d"] = np.arange(K)[None, :] - 1.5
        pan["tajima_d"][0, 0] = np.nan
        pairs = np.zeros((self.n, K * (K - 1) // 2 if want_pairs else 0), dtype=impop_amd.PAIR_DTYPE)
        if want_pairs:
            pairs["fst"] = 0.25
        win = np.zeros(self.n, dtype=impop_amd.PANEL_WINDOW_DTYPE)
        win["s_all"] = 7
        return pan, pairs, win

    def close(self):
        pass


@pytest.fixture()
def fixture_files(tmp_path):
    from impop_amd import matrixio
    rng = np.random.default_rng(5)
    n, W = 12, 600
    m = (rng.random((n, W)) < 0.3).astype(np.uint8)
    names = [f"S{i // 2:03d}#{i % 2 + 1}#chr9:{1000}-{1000 + W}" for i in range(n)]
    matrixio.save_matrix(str(tmp_path / "m.npz"), matrixio.from_dense(m, names, origin=1000, contig="CHM13#0#chr9"))
    (tmp_path / "w.bed").write_text("chr9\t1000\t1300\nchr9\t1300\t1600\n")
    (tmp_path / "A.txt").write_text("S000#1\nS000#2\nS001#1\n")
    (tmp_path / "B.txt").write_text("S002#1\nS002#2\n")
    (tmp_path / "C.txt").write_text("S003#1\nS004#1\nS004#2\nS005#2\n")
    return tmp_path


def _run_cli(cli, tmp, extra):
    _Recorder.calls = []
    cli.Runner = _Recorder
    argv = [SCAN, "--matrix", str(tmp / "m.npz"), "--bed", str(tmp / "w.bed"), "--panel"] + [str(tmp / f) for f in ("A.txt", "B.txt", "C.txt")] + extra
    out, old = io.StringIO(), sys.argv
    sys.argv = argv
    try:
        with contextlib.redirect_stdout(out):
            cli.main()
    finally:
        sys.argv = old
    return out.getvalue().splitlines(), list(_Recorder.calls)


def test_driver_routes_of_panel(fixture_files):
    cli = load_cli()
    # unrounded `match` h-fst alone: the streaming K-population scan, as before — no hap-major operand, no all-pairs call
    lines, calls = _run_cli(cli, fixture_files, ["--format", "hfst"])
    assert calls == [("init", False), ("scan_multi", 3)]
    assert lines[0] == "# A-vs-B" and lines[1] == "REGION\tLENGTH\tFST\tPI_A\tPI_B\tPI_XY\tDXY\tDA" and len(lines) == 3 * 4
    assert lines[2].startswith("CHM13#0#chr9:1000-1300\t300\t0.12500000\t")
    # -r N, or dice: the panel call, pairs only, no S
    lines, calls = _run_cli(cli, fixture_files, ["--format", "hfst", "-r", "5"])
    assert calls == [("init", True), ("panel", 3, 1.0, 5, False, True)]
    assert [ln for ln in lines if ln.startswith("#")] == ["# A-vs-B", "# A-vs-C", "# B-vs-C"] and lines[2].split("\t")[2] == "0.25000000"
    lines, calls = _run_cli(cli, fixture_files, ["--format", "hfst", "--identity", "dice"])
    assert calls == [("init", True), ("panel", 3, 1.0, None, False, True)]
    # tajd: the defaults of run_tajd.sh, panels only, S over all rows
    lines, calls = _run_cli(cli, fixture_files, ["--format", "tajd"])
    assert calls == [("init", True), ("panel", 3, 0.999, 5, True, False)]
    assert [ln for ln in lines if ln.startswith("#")] == ["# A", "# B", "# C"] and len(lines) == 3 * 4
    assert lines[1] == "REGION\tLENGTH\tSAMPLES\tSEGREGATING_SITES\tPI\tTAJIMAS_D"
    assert lines[2] == "CHM13#0#chr9:1000-1300\t300\t3\t7\t0.00123457\tNA" and lines[3] == "CHM13#0#chr9:1300-1600\t300\t3\t7\t0.00123457\t-1.5"
    assert lines[6] == "CHM13#0#chr9:1000-1300\t300\t2\t7\t0.00123457\t-0.5" and lines[10].split("\t")[2] == "4"
    # all: both; one call when the two tables round alike, the streaming pairs next to the panel call when h-fst is unrounded
    lines, calls = _run_cli(cli, fixture_files, ["--format", "all", "--fst-round-digits", "5"])
    assert calls == [("init", True), ("panel", 3, 0.999, 5, True, True)]
    assert [ln for ln in lines if ln.startswith("#")] == ["# A-vs-B", "# A-vs-C", "# B-vs-C", "# A", "# B", "# C"]
    lines, calls = _run_cli(cli, fixture_files, ["--format", "all"])
    assert calls == [("init", True), ("scan_multi", 3), ("panel", 3, 0.999, 5, True, False)]
    lines, calls = _run_cli(cli, fixture_files, ["--format", "all", "--fst-round-digits", "3", "-t", "0.99"])
    assert calls == [("init", True), ("panel", 3, 0.99, 5, True, False), ("panel", 3, 0.99, 3, False, True)]
