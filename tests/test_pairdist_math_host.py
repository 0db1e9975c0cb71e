"""No GPU: csrc/pairdist_math.h — the key order, the (min, ties, same) merge, the S_nn summation, gmin and the sum_h2 admission rule
of impop_pairdist_scan — through the stand-alone driver tests/fuzz/pairdist_math.cc, built with ASan + UBSan.  The driver cuts
random small distance matrices into random tiles, merges them in random order and compares records, nearest-neighbour counts, the
bits of snn and the admission rule at its boundary with a direct scan."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def pairdist_math_exe(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pairdist_math") / "pairdist_math")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "pairdist_math.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("seed", (1, 20261019, 977))
def test_tiled_merges_equal_the_direct_scan(pairdist_math_exe, seed):
    r = subprocess.run([pairdist_math_exe, str(seed), "1000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 1000", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_header_is_plain_cxx():
    """no HIP types: the device and the host run the same code"""
    src = open(os.path.join(ROOT, "impop_amd", "csrc", "pairdist_math.h")).read()
    assert "hip/hip_runtime.h" not in src and "DIP_HD" in src
    for name in ("pd_min_key", "pd_max_key", "pd_nn_merge", "pd_nn_pair", "pd_snn_term", "pd_gmin", "pd_sum_h2_admitted"):
        assert name in src, name
    hip = open(os.path.join(ROOT, "impop_amd", "csrc", "pairdist.hip")).read()
    for name in ("pd_acc_add", "pd_nn_merge", "pd_nn_pair", "pd_snn_term", "pd_snn_finish", "pd_gmin", "pd_fields", "pd_bin"):
        assert name in hip, name  # the kernel runs the header's code, not a copy of it
