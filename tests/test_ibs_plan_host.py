"""No GPU: csrc/ibs_plan.h — the host logic of impop_ibs_scan (pair tiles, the chunk / sub-segment cutter, segment offsets, the
window-edge accumulation) together with dip_runs.h's combine — through the stand-alone driver tests/fuzz/ibs_plan.cc, built with
ASan + UBSan.  The driver cuts random difference sets into random chunks and sub-segments, folds them in order as the device does
and compares tract counts, slots, offsets and window sums with a direct scan of the definition, min_sites in {1, 2, 7, 64, 65}."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def ibs_plan_exe(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ibs_plan") / "ibs_plan")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "ibs_plan.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("seed", (1, 20261019, 977))
def test_chunked_sweeps_equal_the_direct_scan(ibs_plan_exe, seed):
    r = subprocess.run([ibs_plan_exe, str(seed), "1000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 1000", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_header_is_plain_cxx():
    """no HIP types: the device and the host run the same code"""
    src = open(os.path.join(ROOT, "impop_amd", "csrc", "ibs_plan.h")).read()
    assert "hip/hip_runtime.h" not in src and "DIP_HD" in src and "ibs_add_tract" in src and "ibs_cut" in src
