"""No GPU: csrc/tree_math.h — the exact value comparison with its tie rule, the Lance-Williams updates, the cached-neighbour rule
and the panel bookkeeping of impop_tree_scan — through the stand-alone driver tests/fuzz/tree_math.cc, built with ASan + UBSan.
The driver runs the whole clustering (tree_solve_serial: the kernel's scheme) on random small integer matrices with many ties and
compares every merge, counter and panel record with a brute-force global search, and the comparison with unsigned __int128."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def tree_math_exe(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("tree_math") / "tree_math")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "tree_math.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("seed", (1, 20261021, 977))
def test_cached_scheme_equals_the_global_search(tree_math_exe, seed):
    r = subprocess.run([tree_math_exe, str(seed), "300"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 300", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_header_is_plain_cxx():
    """no HIP types: the device and the host run the same code, and the kernel calls it rather than copies of it"""
    src = open(os.path.join(ROOT, "impop_amd", "csrc", "tree_math.h")).read()
    assert "hip/hip_runtime.h" not in src and "DIP_HD" in src and "__global__" not in src and "threadIdx" not in src
    shared = ("tree_key", "tree_key_less", "tree_best_of_row", "tree_best_combine", "tree_lance_williams", "tree_cache_survives",
              "tree_panel_start", "tree_panel_merge", "tree_count_merge")
    for name in shared + ("tree_mul_64x64", "tree_cmp_value", "tree_is_tied"):
        assert re.search(r"TREE_FN \w+ %s\(" % name, src), name
    hip = open(os.path.join(ROOT, "impop_amd", "csrc", "tree.hip")).read()
    assert '#include "tree_math.h"' in hip
    for name in shared:
        assert name + "(" in hip, name  # the kernel runs the header's code ...
    for name in shared + ("tree_mul_64x64", "tree_cmp_value", "tree_is_tied"):  # ... and defines none of it again
        assert not re.search(r"\b(?:bool|int|void|uint32_t|uint64_t|TreeKey|TreeBest|TreePanel|TreeU128)\s+%s\s*\(" % name, hip), name
    for arithmetic in ("p11 + (p01 >> 32)", "x.a != y.a ? x.a < y.a"):  # the wide multiply and the tie rule live in the header alone
        assert arithmetic in src and arithmetic not in hip
    assert "__int128" not in src  # one definition for host and device
