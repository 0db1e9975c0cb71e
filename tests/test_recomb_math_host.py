"""No GPU: csrc/recomb_math.h — the greedy R_min, the running maximum with its blocks and Wall's counts of impop_recomb_scan —
through the stand-alone driver tests/fuzz/recomb_math.cc, built with ASan + UBSan.  The driver runs the header's one-pass scheme on
random per-site arrays (m = 0, 1, 2 included) and compares every counter with brute force: a DP maximum of disjoint intervals and
an O(m^2) search for the maximal compatible runs."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def recomb_math_exe(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("recomb_math") / "recomb_math")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "recomb_math.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("seed", (1, 20261021, 977))
def test_one_pass_scheme_equals_brute_force(recomb_math_exe, seed):
    r = subprocess.run([recomb_math_exe, str(seed), "2000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 2000", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_header_is_plain_cxx():
    """no HIP types: the device and the host run the same code, and the kernel calls it rather than copies of it"""
    src = open(os.path.join(ROOT, "impop_amd", "csrc", "recomb_math.h")).read()
    assert "hip/hip_runtime.h" not in src and "DIP_HD" in src and "__global__" not in src and "threadIdx" not in src
    shared = ("recomb_start", "recomb_step", "recomb_end", "recomb_seen_words")
    for name in shared:
        assert re.search(r"RECOMB_FN \w+ %s\(" % name, src), name
    hip = open(os.path.join(ROOT, "impop_amd", "csrc", "recomb.hip")).read()
    assert '#include "recomb_math.h"' in hip and '#include "ld_select.h"' in hip
    for name in shared:
        assert name + "(" in hip, name  # the kernel runs the header's code ...
        assert not re.search(r"\b(?:bool|int|void|uint32_t|uint64_t|RecombState)\s+%s\s*\(" % name, hip), name  # ... and defines none of it
    for arithmetic in ("left1 - 1u >= s.cut", "left1 > s.M"):  # the greedy and the running maximum live in the header alone
        assert arithmetic in src and arithmetic not in hip


def test_one_ranking_rule_for_both_scans():
    """the thinning rule floor(k q / m) is written once, in ld_select.h, and both scans launch that kernel"""
    csrc = os.path.join(ROOT, "impop_amd", "csrc")
    rule = "(rank * m + q - 1) / q"
    assert rule in open(os.path.join(csrc, "ld_select.h")).read()
    for f in ("ldscan.hip", "recomb.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert rule not in text and "ld_gather_kernel" in text and "ld_select_kernel" in text and '#include "ld_select.h"' in text
