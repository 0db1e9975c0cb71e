"""No GPU: csrc/ihs_math.h — the arithmetic impop_ihs_scan shares between host and device (the cutoff comparison, a break's
nearest-greater spans and its share of an integral, reach and flag rules, the chunk cutter, the warm-up start) — through the
stand-alone driver tests/fuzz/ihs_math.cc, built with ASan + UBSan.  The driver runs a serial PBWT from a random chunk's warm-up
start, forms the integrals the way the walk kernel does and compares them with pair-by-pair counting from the rows."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def ihs_math_exe(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ihs_math") / "ihs_math")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "ihs_math.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("seed", (1, 20261020, 977))
def test_walk_arithmetic_equals_pair_counting(ihs_math_exe, seed):
    r = subprocess.run([ihs_math_exe, str(seed), "150"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 150", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_header_is_plain_cxx():
    """no HIP types: the device and the host run the same code"""
    src = open(os.path.join(ROOT, "impop_amd", "csrc", "ihs_math.h")).read()
    assert "hip/hip_runtime.h" not in src and "IHS_HD" in src
    for name in ("ihs_cut_ok", "ihs_span_left", "ihs_span_right", "ihs_break_term", "ihs_far", "ihs_flag", "ihs_chunks", "ihs_warm_start"):
        assert name in src, name
    kernel = open(os.path.join(ROOT, "impop_amd", "csrc", "ihs.hip")).read()
    for name in ("ihs_cut_ok", "ihs_span_left", "ihs_span_right", "ihs_break_term", "ihs_alive_term", "ihs_far", "ihs_flag", "ihs_chunks",
                 "ihs_warm_start"):
        assert name + "(" in kernel, name  # the kernel calls them: it has no arithmetic of its own to drift
