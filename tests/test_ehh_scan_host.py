"""No GPU: the host side of the windowed EHH scan — the window list of ehhgfa.main against the reference's own output
(tests/golden/ehh.json["cli"]), the ABI declaration and record layout, and what `impop_scan.py --format ehh` refuses before
any device is opened."""
import ctypes as C
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

SCAN = os.path.join(ROOT, "scripts", "impop_scan.py")


def _n_col(case):
    return len(case["matrix_text"].splitlines()[0].split())


def test_window_list_matches_the_reference_rows():
    """every rc-0 case: the (name, colstart, colend) the reference printed are the list's, in order; the last window of a
    matrix that is no multiple of -w keeps its nominal colend and is cut at the matrix end"""
    from impop_amd.ehh import window_list
    cases = [c for c in load_golden("ehh.json")["cli"] if c["rc"] == 0]
    assert len(cases) >= 3
    cut = 0
    for c in cases:
        wl = window_list(_n_col(c), c["w"], c["p"])
        printed = []
        for line in c["out"].splitlines():
            name, cs, ce = (int(x) for x in line.split()[:3])
            if (name, cs, ce) not in printed:
                printed.append((name, cs, ce))
        assert [(w[0], w[1], w[2]) for w in wl] == printed
        for name, cs, ce, hi, core in wl:
            assert hi == min(ce, _n_col(c)) and core == cs + c["p"] - 1 and cs <= core < hi
            cut += hi < ce
    assert cut >= 1  # the golden cases hold a cut last window


def test_window_list_raises_the_reference_errors():
    from impop_amd.ehh import window_list
    bad = [c for c in load_golden("ehh.json")["cli"] if c["rc"] != 0]
    assert len(bad) == 1 and bad[0]["stderr_last"].startswith("IndexError: ")
    c = bad[0]
    with pytest.raises(IndexError) as ei:  # the test SNP is the window's last column: the right flank is empty
        window_list(_n_col(c), c["w"], c["p"])
    assert "IndexError: " + str(ei.value) == c["stderr_last"]
    with pytest.raises(IndexError) as ei:  # 25 columns, -w 10, -p 8: the third window has 5 columns
        window_list(25, 10, 8)
    assert str(ei.value) == "index 7 is out of bounds for axis 1 with size 5"
    with pytest.raises(ValueError):
        window_list(25, 10, 0)
    assert window_list(0, 10, 3) == []


def test_abi_declares_ehh_scan():
    from impop_amd import _lib
    import impop_amd
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    assert re.search(r"#define IMPOP_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    for sym in ("impop_ehh_scan", "impop_ctx_ehh_elapsed"):
        assert re.search(r"^int %s\(" % sym, header, flags=re.M) and sym in _lib.SIGNATURES
    assert "64 bytes" in header[header.index("typedef struct impop_ehh_stats"):][:80]
    assert C.sizeof(_lib.EhhStats) == 64 and C.sizeof(_lib.EhhWindow) == 24 and C.sizeof(_lib.EhhParams) == 24
    assert impop_amd.EHH_DTYPE.itemsize == 64
    assert [n for n, _ in _lib.EhhStats._fields_] == list(impop_amd.EHH_DTYPE.names)
    for name, _ in _lib.EhhStats._fields_:
        assert getattr(_lib.EhhStats, name).offset == impop_amd.EHH_DTYPE.fields[name][1]
    assert impop_amd.EHH_DTYPE["area_milli"].shape == (2, 2) and impop_amd.EHH_DTYPE["area_milli"].base == np.dtype("<i8")
    limit = int(re.search(r"#define IMPOP_EHH_SCAN_MAX_N (\d+)u", header).group(1))
    assert limit >= 4096 and limit == _lib.EHH_SCAN_MAX_N
    if os.path.exists(_lib.SO_PATH):
        lib = C.CDLL(_lib.SO_PATH)
        assert hasattr(lib, "impop_ehh_scan") and hasattr(lib, "impop_ctx_ehh_elapsed")


@pytest.mark.parametrize("extra,env,text", [
    (["--sim-list", "x.tsv"], {}, "not with --sim-list"),
    (["--matrix", "m.npz", "--bed", "w.bed", "--devices", "2"], {}, "not with --devices"),
    (["--matrix", "m.npz", "--bed", "w.bed"], {"WORLD_SIZE": "2"}, "not under torch.distributed.run"),
    (["--matrix", "m.npz", "--bed", "w.bed", "-A", "a.txt", "-B", "b.txt"], {}, "not with -A"),
    (["--matrix", "m.npz", "--bed", "w.bed", "--panel", "a.txt", "b.txt"], {}, "not with -A"),
    (["--matrix", "m.npz", "--bed", "w.bed", "-l", "s.txt"], {}, "not with -A"),
    (["--matrix", "m.npz", "--bed", "w.bed", "--compact"], {}, "--compact"),
    (["--matrix", "m.npz", "--bed", "w.bed", "--ehh-core-offset", "3", "--ehh-cores", "c.txt"], {}, "not both"),
    (["--matrix", "m.npz", "--bed", "w.bed", "--ehh-core-offset", "-1"], {}, ">= 0"),
    (["--matrix", "m.npz", "--bed", "w.bed", "-t", "0.9"], {}, "belong to other formats"),
])
def test_ehh_refusals_exit_before_any_device(extra, env, text):
    r = subprocess.run([sys.executable, SCAN, "--format", "ehh"] + extra, env=dict(os.environ, **env), capture_output=True, text=True)
    assert r.returncode == 2 and r.stdout == "" and text in r.stderr, r.stderr


def test_ehh_flags_need_format_ehh():
    for flag in (["--ehh-core-offset", "3"], ["--ehh-cores", "c.txt"], ["--ehh-flanks", "two-sided"], ["--ehh-ref", "x"]):
        r = subprocess.run([sys.executable, SCAN, "--format", "pica2", "--matrix", "m.npz", "--bed", "w.bed"] + flag,
                           capture_output=True, text=True)
        assert r.returncode == 2 and "belong to --format ehh" in r.stderr, (flag, r.stderr)


def test_ehh_rows_follow_the_documented_rule():
    """exact thousandths as integer.milli, one row per allele present, REF / ALT against ref_allele"""
    import impop_amd
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("impop_scan_cli_ehh", SCAN)
        cli = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(cli)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    assert [cli.milli_text(k) for k in (0, 7, 1000, 12276, 12000000)] == ["0.000", "0.007", "1.000", "12.276", "12000.000"]
    rec = np.zeros(2, dtype=impop_amd.EHH_DTYPE)
    rec[0]["n_members"], rec[0]["ref_allele"], rec[0]["area_milli"] = (39, 1), 1, ((8753, 9000), (6000000, 6000000))
    rec[1]["n_members"], rec[1]["ref_allele"], rec[1]["area_milli"] = (0, 40), 1, ((0, 0), (4000, 276))
    assert cli.ehh_rows("R:0-20", 20, 107, rec[0]) == ["R:0-20\t20\t107\t0\tALT\t39\t17.753\t8.753\t9.000",
                                                      "R:0-20\t20\t107\t1\tREF\t1\t12000.000\t6000.000\t6000.000"]
    assert cli.ehh_rows("R:20-40", 20, 127, rec[1]) == ["R:20-40\t20\t127\t1\tREF\t40\t4.276\t4.000\t0.276"]
