"""No GPU: csrc/ldband_math.h — the fixed-point r2, the strong test, the decay bin and the sliding kept window of impop_ldband_scan —
through the stand-alone driver tests/fuzz/ldband_math.cc, built with ASan + UBSan.  The driver compares the kept window (as an
array of 1..16 words, and word by word as the prune kernel drives it across lanes) with the definition of the greedy pruning for
band in {1, 63, 64, 65, 300, 1024} and q = 0, 1, 2, ..., and the strong test with 128-bit arithmetic at the n = 4096 extremes."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "impop_amd", "csrc")


@pytest.fixture(scope="module")
def ldband_math_exe(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ldband_math") / "ldband_math")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + CSRC, "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "ldband_math.cc"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("seed", (1, 20261021, 977))
def test_kept_window_and_strong_test_equal_brute_force(ldband_math_exe, seed):
    r = subprocess.run([ldband_math_exe, str(seed), "120"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 120", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_header_is_plain_cxx():
    """no HIP types: the device and the host run the same code, and the kernels call it rather than copies of it"""
    src = open(os.path.join(CSRC, "ldband_math.h")).read()
    assert "hip/hip_runtime.h" not in src and "DIP_HD" in src and "__global__" not in src and "threadIdx" not in src
    shared = ("ldband_fx", "ldband_strong", "ldband_perfect", "ldband_bin", "ldband_word_hit", "ldband_word_carry", "ldband_word_shift",
              "ldband_words")
    for name in shared + ("ldband_kept_step",):
        assert re.search(r"LDBAND_FN \w+ %s\(" % name, src), name
    hip = open(os.path.join(CSRC, "ldband.hip")).read()
    assert '#include "ldband_math.h"' in hip and '#include "ld_select.h"' in hip and "ld_select_kernel" in hip
    for name in shared:
        assert name + "(" in hip, name  # the kernels run the header's code ...
        assert not re.search(r"\b(?:bool|int|void|uint32_t|uint64_t)\s+%s\s*\(" % name, hip), name  # ... and define none of it
    # the scaling, the threshold products and the shift live in the header alone
    for arithmetic in ("(r2 * 1073741824.0)", "(uint64_t)thr_den >", "(k_word << 1)", "d / bin_width"):
        assert arithmetic in src and arithmetic not in hip, arithmetic


def test_the_constants_are_the_public_ones():
    src = open(os.path.join(CSRC, "ldband_math.h")).read()
    pub = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    for name, value in (("MAX_N", 4096), ("MAX_BAND", 1024), ("MAX_BINS", 4096)):
        assert re.search(r"#define IMPOP_LDBAND_%s\s+%du" % (name, value), pub), name
        assert re.search(r"LDBAND_%s = %d;" % (name, value), src), name
    assert re.search(r"#define IMPOP_LDBAND_FX_ONE\s+1073741824u", pub) and "LDBAND_FX_ONE = 1u << 30" in src
    from impop_amd import _lib
    assert (_lib.LDBAND_MAX_N, _lib.LDBAND_MAX_BAND, _lib.LDBAND_MAX_BINS, _lib.LDBAND_FX_ONE) == (4096, 1024, 4096, 1 << 30)
