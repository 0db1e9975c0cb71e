"""No GPU: the host side of impop_haplotype_scan — the ABI declaration and its binding, the record layout on both sides, what
scripts/impop_scan.py refuses next to --format hapstats, the table it prints (a recording stand-in for the Runner: no device is
opened), and the plain reference of tests/hap_cases.py on a case small enough to check by hand."""
import contextlib
import importlib.util
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hap_cases as hc
from conftest import ROOT

SCAN = os.path.join(ROOT, "scripts", "impop_scan.py")


def load_cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("impop_scan_cli_hapstats", SCAN)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    return mod


def test_abi_declares_haplotype_scan():
    import ctypes as C
    import impop_amd
    from impop_amd import _lib
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    assert re.search(r"#define IMPOP_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    assert re.search(r"#define IMPOP_HAPLOTYPE_MAX_N 4096u\b", header) and _lib.HAPLOTYPE_MAX_N == 4096
    assert re.search(r"\bint impop_haplotype_scan\(", header) and "impop_haplotype_scan" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["impop_haplotype_scan"][1]) == 9
    assert C.sizeof(_lib.HaplotypeStats) == 64 and C.sizeof(_lib.HaplotypeParams) == 16
    assert impop_amd.HAPLOTYPE_DTYPE.itemsize == 64
    fields = ["n_members", "n_distinct", "largest", "second", "n_singletons", "n_sites", "sum_sq", "h1", "h12", "h2_h1", "hap_diversity"]
    assert [n for n, _ in _lib.HaplotypeStats._fields_] == fields == list(impop_amd.HAPLOTYPE_DTYPE.names)
    for name, _ in _lib.HaplotypeStats._fields_:  # same offsets on both sides
        assert getattr(_lib.HaplotypeStats, name).offset == impop_amd.HAPLOTYPE_DTYPE.fields[name][1]
    assert _lib.HaplotypeStats.sum_sq.offset == 24 and _lib.HaplotypeStats.h1.offset == 32
    # the struct of the header, member by member in the same order
    body = re.search(r"typedef struct impop_haplotype_stats \{(.*?)\} impop_haplotype_stats;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert declared == fields
    assert hasattr(impop_amd.BitMatrix, "haplotype_scan")
    if os.path.exists(_lib.SO_PATH):
        assert hasattr(C.CDLL(_lib.SO_PATH), "impop_haplotype_scan")


@pytest.mark.parametrize("extra,env,needle", [
    (["--devices", "2"], {}, "not with --devices N"),
    (["-A", "a.txt", "-B", "b.txt"], {}, "not with -A / -B / --panel / -l"),
    (["--panel", "a.txt", "b.txt"], {}, "not with -A / -B / --panel / -l"),
    (["-l", "s.txt"], {}, "not with -A / -B / --panel / -l"),
    ([], {"WORLD_SIZE": "2", "RANK": "0"}, "not under torch.distributed.run"),
    ([], {"WORLD_SIZE": "2", "RANK": "1"}, "not under torch.distributed.run"),
])
def test_driver_refuses_next_to_hapstats(extra, env, needle):
    r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "hapstats", "--backend", "gloo"] + extra,
                       capture_output=True, text=True, env=dict(os.environ, **env), timeout=120)
    assert r.returncode == 2 and needle in r.stderr, (r.returncode, r.stderr[-500:])
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("Error: --format hapstats"), r.stderr[-500:]


def test_driver_refuses_sim_list():
    r = subprocess.run([sys.executable, SCAN, "--sim-list", "none.tsv", "--format", "hapstats"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stderr.strip() == "Error: --format hapstats scans a presence matrix (--matrix / --bed): not with --sim-list"


def test_other_formats_keep_their_messages():
    r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "af", "--devices", "2"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stderr.strip() == "Error: --format af runs on one GPU: not with --devices N"
    r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "ehh", "--compact"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--format ehh scans the sequences of -u" in r.stderr


class _Recorder:
    """stands in for impop_scan.Runner: records the calls, returns records that name their source"""
    calls = []

    def __init__(self, args, mf, windows, need_pairs, rank, world, local_rank):
        self.n = len(windows)
        _Recorder.calls.append(("init", need_pairs, bool(args.compact)))

    def hapstats(self, mask_p):
        import impop_amd
        _Recorder.calls.append(("hapstats", None if mask_p is None else int(np.asarray(mask_p).sum())))
        out = np.zeros(self.n, dtype=impop_amd.HAPLOTYPE_DTYPE)
        out["n_members"], out["n_sites"] = 12, [300, 299]
        out["n_distinct"] = [5, 1]
        out["h1"], out["h12"], out["h2_h1"], out["hap_diversity"] = [0.25, 1.0], [0.3888888888888, 1.0], [0.123456789, 0.0], [0.8181818181818, 0.0]
        return out

    def close(self):
        pass


def test_driver_prints_the_hapstats_table(tmp_path):
    from impop_amd import matrixio
    rng = np.random.default_rng(5)
    n, W = 12, 600
    m = (rng.random((n, W)) < 0.3).astype(np.uint8)
    names = [f"S{i // 2:03d}#{i % 2 + 1}#chr9:{1000}-{1000 + W}" for i in range(n)]
    matrixio.save_matrix(str(tmp_path / "m.npz"), matrixio.from_dense(m, names, origin=1000, contig="CHM13#0#chr9"))
    (tmp_path / "w.bed").write_text("chr9\t1000\t1300\nchr9\t1300\t1600\n")
    (tmp_path / "u.txt").write_text("S000#1\nS000#2\nS001#1\n")
    cli = load_cli()
    cli.Runner = _Recorder

    def run(extra):
        _Recorder.calls = []
        out, old = io.StringIO(), sys.argv
        sys.argv = [SCAN, "--matrix", str(tmp_path / "m.npz"), "--bed", str(tmp_path / "w.bed"), "--format", "hapstats"] + extra
        try:
            with contextlib.redirect_stdout(out):
                cli.main()
        finally:
            sys.argv = old
        return out.getvalue().splitlines(), list(_Recorder.calls)

    lines, calls = run([])
    assert calls == [("init", False, False), ("hapstats", None)]  # no all-pairs operand is asked for
    assert lines == ["REGION\tLENGTH\tSAMPLES\tSITES\tHAPLOTYPES\tH1\tH12\tH2_H1\tHAP_DIVERSITY",
                     "CHM13#0#chr9:1000-1300\t300\t12\t300\t5\t0.25000000\t0.38888889\t0.12345679\t0.81818182",
                     "CHM13#0#chr9:1300-1600\t300\t12\t299\t1\t1.00000000\t1.00000000\t0.00000000\t0.00000000"]
    lines, calls = run(["-u", str(tmp_path / "u.txt"), "--compact"])
    assert calls == [("init", False, True), ("hapstats", 3)] and len(lines) == 3


def test_reference_on_a_hand_case():
    m01 = np.array([[0, 1, 0, 1],
                    [0, 1, 0, 0],
                    [0, 1, 0, 1],
                    [1, 1, 0, 0],
                    [0, 1, 0, 0],
                    [0, 1, 0, 1]], dtype=np.uint8)
    rec, cl, sz = hc.reference(m01, None, [(0, 4), (1, 3), (2, 2), (3, 4)])
    assert cl.tolist() == [[0, 1, 0, 2, 1, 0], [0] * 6, [0] * 6, [0, 1, 0, 1, 1, 0]]  # equal sizes: the smaller first member first
    assert sz.tolist() == [[3, 2, 1, 0, 0, 0], [6, 0, 0, 0, 0, 0], [6, 0, 0, 0, 0, 0], [3, 3, 0, 0, 0, 0]]
    assert rec["n_distinct"].tolist() == [3, 1, 1, 2] and rec["second"].tolist() == [2, 0, 0, 3] and rec["n_singletons"].tolist() == [1, 0, 0, 0]
    assert rec["sum_sq"].tolist() == [14, 36, 36, 18] and rec["n_sites"].tolist() == [4, 2, 0, 1]
    assert rec["h1"][0] == 14 / 36 and rec["h12"][0] == 14 / 36 + 2.0 * (3 / 6) * (2 / 6) and rec["hap_diversity"][1] == 0.0
    assert abs(rec["h2_h1"][0] - (14 - 9) / 14) < 1e-15 and rec["hap_diversity"][3] == (1.0 - 0.5) * 6 / 5
    rec, cl, sz = hc.reference(m01, [1, 0, 0, 1, 0, 0], [(0, 4)], weights=[5, 1, 2, 3])
    assert cl.tolist() == [[0, 1]] and sz.tolist() == [[1, 1]] and rec["n_sites"].tolist() == [11] and rec["second"].tolist() == [1]
