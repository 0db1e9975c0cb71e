"""csrc/win_chunks.h on the host (plain C++, no HIP, no GPU): the member set and the chunk planner of the chunked window calls,
checked by tests/fuzz/win_chunks.cc against its own brute-force model under ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def win_chunks_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("win_chunks") / "win_chunks")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "win_chunks.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-4000:])
    return r.stdout.strip()


_BIG = 1 << 40
_TILING = [(2 * i, 2 * i + 2) for i in range(6)]        # 6 windows of 2 tiles each, nothing shared
_SLIDING = [(i, i + 2) for i in range(7)]               # 50 % overlap: every tile but the ends in two windows
_NESTED = [(0, 8), (0, 8), (2, 5), (3, 4), (0, 8)]      # identical and nested
_WITH_EMPTY = [(0, 3), (0, 0), (3, 5), (5, 5), (4, 8), (0, 0)]  # windows without tiles between others
# name: (budget, cap, n_tiles, (per_tile, per_win, per_item), windows, the driver's line).  Costs of 100 / 10 / 1 bytes.
PLAN_CASES = {
    "tiling": (450, 0, 12, (100, 10, 1), _TILING, "chunks=3 sizes=2,2,2"),          # a window: 212 bytes, two: 424
    "sliding": (450, 0, 8, (100, 10, 1), _SLIDING, "chunks=3 sizes=3,3,1"),         # 212, then 112 per further window: 436 for three
    "nested_and_identical": (850, 0, 8, (100, 10, 1), _NESTED, "chunks=2 sizes=3,2"),  # 818 + 18 + 13 = 849, the fourth adds 11
    "windows_without_tiles": (550, 0, 8, (100, 10, 1), _WITH_EMPTY, "chunks=2 sizes=4,2"),
    "single_window": (_BIG, 0, 4, (100, 10, 1), [(1, 4)], "chunks=1 sizes=1"),
    "single_window_over_budget": (1, 0, 4, (100, 10, 1), [(1, 4)], "chunks=1 sizes=1"),
    "budget_1": (1, 0, 8, (100, 10, 1), _SLIDING, "chunks=7 sizes=1,1,1,1,1,1,1"),
    "budget_fits_everything": (_BIG, 0, 8, (100, 10, 1), _SLIDING, "chunks=1 sizes=7"),
    "cap_3_unlimited_budget": (_BIG, 3, 8, (100, 10, 1), _SLIDING, "chunks=3 sizes=3,3,1"),
    "cap_3_tiling_of_8": (_BIG, 3, 16, (100, 10, 1), [(2 * i, 2 * i + 2) for i in range(8)], "chunks=3 sizes=3,3,2"),
}


@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_tiled_plan(win_chunks_exe, case):
    """The driver checks every property of the plan itself (tests/fuzz/win_chunks.cc lists them) and exits non-zero on a breach;
    here: it ran clean under the sanitizers and cut where the case's arithmetic says."""
    budget, cap, n_tiles, costs, windows, line = PLAN_CASES[case]
    assert _run(win_chunks_exe, "plan", budget, cap, n_tiles, *costs, *[x for w in windows for x in w]) == line


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_tiled_plan_random_lists(win_chunks_exe, seed):
    assert _run(win_chunks_exe, "random", seed, 200) == "random ok lists=200"


def test_member_set(win_chunks_exe):
    """n_hap in {1, 31, 32, 33, 64, 65, 465} x {null mask, empty, first only, last only, random}, the mask's spare bits set."""
    assert _run(win_chunks_exe, "members") == "members ok cases=35"
