"""No GPU: csrc/dip_runs.h — the run-length summary of impop_diploid_scan and its associative combine — through the stand-alone
driver tests/fuzz/dip_runs.cc, built with ASan + UBSan.  The driver cuts random heterozygous-site sets into random tiles and
"waves", folds them in order and compares with a direct scan of the definition for min_run in {1, 2, 7, 64, 65}."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def dip_runs_exe(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("dip_runs") / "dip_runs")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "dip_runs.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("seed", (1, 20260101, 977))
def test_fold_in_any_cutting_equals_the_direct_scan(dip_runs_exe, seed):
    r = subprocess.run([dip_runs_exe, str(seed), "1500"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 1500", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_header_is_plain_cxx():
    """no HIP types: the device and the host run the same code"""
    src = open(os.path.join(ROOT, "impop_amd", "csrc", "dip_runs.h")).read()
    assert "hip/hip_runtime.h" not in src and "__host__ __device__" in src and "dip_combine" in src and "dip_close" in src
