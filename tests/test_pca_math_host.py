"""No GPU: csrc/pca_math.h — the block iteration of impop_pca_scan, its orthonormalisation, the round-robin Jacobi, the zero,
convergence and sign rules and the window distance — through the stand-alone driver tests/fuzz/pca_math.cc, built with ASan +
UBSan.  The driver runs the whole iteration (pca_solve_serial) on the double-centred distance matrices of random small 0/1
matrices and compares eigenvalues, residuals, orthonormality and signs with a brute-force Jacobi of the full matrix."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def pca_math_exe(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pca_math") / "pca_math")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "pca_math.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("seed", (1, 20261020, 977))
def test_iteration_equals_the_brute_force_spectrum(pca_math_exe, seed):
    r = subprocess.run([pca_math_exe, str(seed), "150"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 150", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_header_is_plain_cxx():
    """no HIP types: the device and the host run the same code, and the kernel calls it rather than copies of it"""
    src = open(os.path.join(ROOT, "impop_amd", "csrc", "pca_math.h")).read()
    assert "hip/hip_runtime.h" not in src and "DIP_HD" in src and "__global__" not in src and "threadIdx" not in src
    shared = ("pca_start", "pca_hv_add", "pca_bv_row", "pca_centre_row", "pca_gs_partials", "pca_gs_subtract", "pca_gs_scale",
              "pca_dot_partials", "pca_rotate_row", "pca_resid_partials", "pca_jacobi_threshold", "pca_jacobi_round_angles",
              "pca_jacobi_elem", "pca_jacobi_qelem", "pca_sort_desc", "pca_trace", "pca_rank", "pca_converged", "pca_sign_pivot",
              "pca_dist2")
    for name in shared:
        assert re.search(r"PCA_FN \w+ %s\(" % name, src), name
    hip = open(os.path.join(ROOT, "impop_amd", "csrc", "pca.hip")).read()
    assert '#include "pca_math.h"' in hip
    for name in shared:
        assert name + "(" in hip, name  # the kernel runs the header's code ...
        assert not re.search(r"\b(?:double|void|bool|int|uint32_t)\s+%s\s*\(" % name, hip), name  # ... and defines none of it again
    for arithmetic in ("sqrt(th * th", "0x9E3779B97F4A7C15"):  # the rotation angle and the start hash live in the header alone
        assert arithmetic in src and arithmetic not in hip
