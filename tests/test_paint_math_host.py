"""No GPU: csrc/paint_math.h — the one-site state update, the packed (value, slot) word, the renormalisation, the backtrack over the
per-site records and the window overlap of impop_paint_scan — through the stand-alone driver tests/fuzz/paint_math.cc, built with
ASan + UBSan.  The driver runs the device's origin-pointer form beside the literal stay-bit recursion of the header on random small
inputs (c_s = 0, mu = c, all-equal rows, duplicated donors, 1 and 1024 donors) and at the 2^20 / 65535 limits over more than 2^16
sites."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "impop_amd", "csrc")


@pytest.fixture(scope="module")
def paint_math_exe(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("paint_math") / "paint_math")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + CSRC, "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "paint_math.cc"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("seed", (1, 20261021, 977))
def test_origin_pointer_form_equals_the_stay_bit_definition(paint_math_exe, seed):
    r = subprocess.run([paint_math_exe, str(seed), "96"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 96", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_header_is_plain_cxx():
    """no HIP types: the device and the host run the same code, and the kernels call it rather than copies of it"""
    src = open(os.path.join(CSRC, "paint_math.h")).read()
    assert "hip/hip_runtime.h" not in src and "DIP_HD" in src and "__global__" not in src and "threadIdx" not in src
    shared = ("paint_site_update", "paint_pack", "paint_pack_value", "paint_pack_slot", "paint_renorm", "paint_backtrack", "paint_overlap")
    for name in shared:
        assert re.search(r"PAINT_FN \w+ %s\(" % name, src), name
    hip = open(os.path.join(CSRC, "paint.hip")).read()
    assert '#include "paint_math.h"' in hip and '#include "ibs_transpose.h"' in hip and "ibs_transpose_kernel" in hip
    for name in shared:
        assert name + "(" in hip, name  # the kernels run the header's code ...
        assert not re.search(r"\b(?:bool|int|void|uint32_t|uint64_t)\s+%s\s*\(" % name, hip), name  # ... and define none of it
    # the stay rule, the packing and the renormalisation live in the header alone
    for arithmetic in ("R <= c", "(R << PAINT_SLOT_BITS)", "R -= site_min", "r.org < end"):
        assert arithmetic in src and arithmetic not in hip, arithmetic
    # the transpose is shared, not copied: ibs.hip includes it and defines no kernel of that name
    ibs = open(os.path.join(CSRC, "ibs.hip")).read()
    assert '#include "ibs_transpose.h"' in ibs and "void ibs_transpose_kernel" not in ibs
    # no workgroup barrier, no LDS and no atomic in the forward kernel
    fwd = hip[hip.index("void paint_forward_kernel"):hip.index("void paint_backtrack_kernel")]
    assert "__syncthreads" not in fwd and "atomic" not in fwd and "__shared__" not in fwd and "wave_min_u32_dpp" in fwd


def test_the_constants_are_the_public_ones():
    src = open(os.path.join(CSRC, "paint_math.h")).read()
    pub = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    for name, value in (("MAX_DONORS", 1024), ("MAX_RECIPIENTS", 4096), ("MAX_PANELS", 8), ("MAX_COST", 1048576)):
        assert re.search(r"#define IMPOP_PAINT_%s\s+%du" % (name, value), pub), name
        assert re.search(r"PAINT_%s = %d;" % (name, value), src), name
    assert re.search(r"#define IMPOP_PAINT_NO_PANEL\s+255u", pub)
    assert "DEV_ERR_PAINT = 8192u" in open(os.path.join(CSRC, "internal.h")).read()
    from impop_amd import _lib
    assert (_lib.PAINT_MAX_DONORS, _lib.PAINT_MAX_RECIPIENTS, _lib.PAINT_MAX_PANELS, _lib.PAINT_MAX_COST, _lib.PAINT_NO_PANEL) == \
        (1024, 4096, 8, 1 << 20, 255)
    assert "impop_paint_scan" in _lib.SIGNATURES and "impop_ctx_paint_elapsed" in _lib.SIGNATURES


def test_the_abi_version_is_still_4():
    from impop_amd import _lib
    pub = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    assert _lib.ABI_VERSION == 4 and re.search(r"#define IMPOP_ABI_VERSION\s+4\b", pub)
