"""csrc/tile_cut.h on the host (plain C++, no HIP, no GPU): the cutter that decides which bytes every streaming kernel reads, and
the default tile size, checked by tests/fuzz/tile_cut.cc against its own brute-force model under ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def tile_cut_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("tile_cut") / "tile_cut")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "tile_cut.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-4000:])
    return r.stdout.strip()


def _sites(*ranges):
    """windows of a route without a split: (site_begin, site_end) -> the six numbers of a window, r = g = 0"""
    return [(a, 0, 0, b, 0, 0) for a, b in ranges]


# name: (tile_blocks, wps, packed, windows as (c0, r0, g0, c1, r1, g1), the driver's line).  A tile is printed as the blocks it
# touches, or blocks+entries+singletons where it has rare sites.  row_bytes = 256 wps, budget = tile_blocks row_bytes.
CUT_CASES = {
    # three windows of 8 blocks side by side, 4 blocks a tile: each is ceil(8 / 4) = 2 parts of 4
    "tiling": (4, 15, 0, _sites((0, 512), (512, 1024), (1024, 1536)), "tiles=6 sizes=4,4,4,4,4,4"),
    # 512-site windows every 256 sites: four segments of 256 sites = 4 blocks, each tiled once though two windows hold the inner ones
    "sliding_50_percent": (4, 15, 0, _sites((0, 512), (256, 768), (512, 1024)), "tiles=4 sizes=4,4,4,4"),
    # segments [0,128) 2 blocks, [128,192) [192,256) [256,320) 1 block each, [320,1024) 11 blocks = ceil(11 / 4) = 3 parts of
    # ceil(11 / 3) = 4, 4 and the remaining 3
    "nested_and_identical": (4, 15, 0, _sites((0, 1024), (0, 1024), (128, 320), (192, 256)), "tiles=7 sizes=2,1,1,1,4,4,3"),
    # empty windows, one at another's edge and one where no window is, cut nothing
    "empty_windows_between": (4, 15, 0, _sites((0, 256), (256, 256), (300, 300), (512, 640)), "tiles=2 sizes=4,2"),
    # the example of the cutter's own comment: 781 blocks under a 512-block limit are 2 parts of ceil(781 / 2) = 391 and 390
    "one_window_over_budget": (512, 1, 0, _sites((0, 781 * 64)), "tiles=2 sizes=391,390"),
    # sites [32, 200) touch blocks 0..3: four parts of one block, [32,64) [64,128) [128,192) [192,200)
    "tile_blocks_1": (1, 3, 0, _sites((32, 200)), "tiles=4 sizes=1,1,1,1"),
    # split route, no rows: 100 entries = 800 B against 768 B are 2 parts of 50
    "rare_sites_only": (1, 3, 0, [(5, 0, 0, 5, 100, 0)], "tiles=2 sizes=0+50+0,0+50+0"),
    # packed, wps 1, budget 256 B: 2 blocks (512 B) + 3 multis + 70 singletons (584 B) = 1096 B are 5 parts; per = ceil(2 / 5) = 1
    # block, per_r = ceil(73 / 5) = 15 rare sites: offsets 0, 15, 30, 45, 60, 73.  The first `off` rare sites hold
    # floor(3 off / 73) = 0, 0, 1, 1, 2, 3 of the multis and singletons for the rest
    "packed_singletons_do_not_divide": (1, 1, 1, [(0, 0, 0, 128, 3, 70)], "tiles=5 sizes=1+0+15,1+1+14,0+0+15,0+1+14,0+1+12"),
    # the same segment as the split route sees it (73 entries): the parts hold as many rare sites, 15 15 15 15 13
    "packed_segment_as_split": (1, 1, 0, [(0, 0, 0, 128, 73, 0)], "tiles=5 sizes=1+15+0,1+15+0,0+15+0,0+15+0,0+13+0"),
}


@pytest.mark.parametrize("case", sorted(CUT_CASES))
def test_cut(tile_cut_exe, case):
    """The driver checks every property of the cut itself (tests/fuzz/tile_cut.cc lists them) and exits non-zero on a breach;
    here: it ran clean under the sanitizers and cut where the case's arithmetic says."""
    tile_blocks, wps, packed, windows, line = CUT_CASES[case]
    assert _run(tile_cut_exe, "cut", tile_blocks, wps, packed, *[x for w in windows for x in w]) == line


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_cut_random_lists(tile_cut_exe, seed):
    assert _run(tile_cut_exe, "random", seed, 200) == "random ok lists=200"


# max(min(32, by_bytes), min(by_bytes, by_parallelism)) with by_bytes = max(32, 1024 // wps) (wps > 16: max(4, 1024 // wps))
# and by_parallelism = blocks // (16 n_cu), n_cu <= 0 counting as 256.  (wps, blocks, n_cu): tile_blocks
RULE_CASES = {
    (15, 0, 256): 32,                  # by_bytes 68, by_parallelism 0: the floor, min(32, 68)
    (15, 50 * 4096, 256): 50,          # by_parallelism 50, between the floor and by_bytes
    (15, 50 * 4096 + 4095, 256): 50,   # ... rounded down
    (15, 100 * 4096, 256): 68,         # by_parallelism 100: capped by by_bytes
    (15, 50 * 4096, 0): 50,            # no CU count: 256
    (15, 40 * 16 * 304, 304): 40,
    (1, 2000 * 4096, 256): 1024,       # by_bytes 1024
    (16, 0, 256): 32,                  # by_bytes 64, the last narrow width
    (16, 1000 * 4096, 256): 64,
    (17, 10 * 4096, 256): 32,          # wide: by_bytes max(4, 60) = 60, floor 32 above by_parallelism 10
    (17, 1000 * 4096, 256): 60,
    (40, 0, 256): 25,                  # by_bytes 25 is below 32: the floor is by_bytes itself
    (40, 1000 * 4096, 256): 25,
    (512, 1000 * 4096, 256): 4,        # by_bytes max(4, 2): one block per wave
}


def test_default_tile_rule(tile_cut_exe):
    got = {k: _run(tile_cut_exe, "rule", *k) for k in RULE_CASES}
    assert got == {k: f"tile_blocks={v}" for k, v in RULE_CASES.items()}
