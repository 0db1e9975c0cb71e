"""No GPU: csrc/kin_math.h — the joint genotype table from the planes' Gram entries, the exact threshold comparison and the pair
index of impop_kinship_scan — through the stand-alone driver tests/fuzz/kin_math.cc, built with ASan + UBSan.  The driver draws
random small genotype sets and compares the table with direct counting of the genotype pairs (also with the constant of a
compacted window) and the threshold test with an exact rational comparison in 128-bit integers."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def kin_math_exe(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("kin_math") / "kin_math")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "kin_math.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("seed", (1, 20261020, 977))
def test_tables_and_thresholds_equal_direct_counting(kin_math_exe, seed):
    r = subprocess.run([kin_math_exe, str(seed), "300"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 300", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_header_is_plain_cxx():
    """no HIP types: the device and the host run the same code"""
    src = open(os.path.join(ROOT, "impop_amd", "csrc", "kin_math.h")).read()
    assert "hip/hip_runtime.h" not in src and "DIP_HD" in src
    for name in ("kin_table", "kin_het_het", "kin_ibs0", "kin_ibs2", "kin_related", "kin_pair_index"):
        assert name in src, name
    hip = open(os.path.join(ROOT, "impop_amd", "csrc", "kinship.hip")).read()
    for name in ("kin_table", "kin_het_het", "kin_ibs0", "kin_ibs2", "kin_related", "kin_pair_index"):
        assert name in hip, name  # the kernels run the header's code, not a copy of it
