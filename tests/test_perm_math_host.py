"""No GPU: csrc/perm_math.h — the labelling generator, the four integer comparisons, the S_nn term, the algebra from a quadratic form
to (wa, wb) and the serial statement of a whole window — through the stand-alone driver tests/fuzz/perm_math.cc, built with ASan +
UBSan and run as a program.  The driver compares perm_window_serial on random small H with the definition restated over sets of
positions, and drives the 128-bit comparisons at the refusal bound against a schoolbook product."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def perm_math_exe(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("perm_math") / "perm_math")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "perm_math.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("seed", (1, 20261020, 977))
def test_serial_statement_equals_the_definition_over_sets(perm_math_exe, seed):
    r = subprocess.run([perm_math_exe, str(seed), "300"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 300", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_header_is_plain_cxx_and_the_kernels_call_it():
    src = open(os.path.join(ROOT, "impop_amd", "csrc", "perm_math.h")).read()
    assert "hip/hip_runtime.h" not in src and "DIP_HD" in src and "__global__" not in src and "threadIdx" not in src
    hip = open(os.path.join(ROOT, "impop_amd", "csrc", "permtest.hip")).read()
    assert '#include "perm_math.h"' in hip
    for name in ("perm_ge_fst", "perm_ge_phi", "perm_ge_dxy", "perm_ge_snn", "perm_nn_term", "perm_wa_wb"):
        assert name + "(" in src and name + "(" in hip, name
    assert "__int128" in src and "__int128" not in hip and "2952069120" in src and "2952069120" not in hip
