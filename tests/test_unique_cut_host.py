"""The unique-row route of csrc/tile_cut.h on the host (plain C++, no HIP, no GPU): which of a tile's rows the fixed-WPS scan kernel
reads as rows (head, tail) and which as representatives of the distinct-row stream (its whole blocks), the bytes that takes and
the bound its 32-bit lane sums rest on, checked by tests/fuzz/unique_cut.cc against its own row-by-row model under ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def unique_cut_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("unique_cut") / "unique_cut")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "unique_cut.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-4000:])
    return r.stdout.strip()


# 5 blocks of rows, the last of 13: 64 * 4 + 13 = 269 rows holding 64, 1, 10, 2, 13 representatives: ubase = 0, 64, 65, 75, 77, 90.
# A block of rows or of the stream is 256 wps bytes; a block of the stream carries 64 weight bytes.  wps = 15: 3840 and 3904.
N_ROWS, REPS = 269, "64,1,10,2,13"
# name: (tile_blocks, wps, windows as (c0, c1), the driver's line).  A tile is head+mid[u0-u1)+tail.
CUT_CASES = {
    # [5, 200): head 59 rows of block 0, whole blocks 1 and 2 = representatives [64, 75) in block 1 of the stream, tail 8 rows
    "head_mid_tail": (32, 15, [(5, 200)], "tiles=1 split=59+2[64-75)+8 bytes=%d" % (2 * 3840 + 3904)),
    # inside one block: no whole block, the rows as they are
    "inside_one_block": (32, 15, [(70, 120)], "tiles=1 split=50+0+0 bytes=3840"),
    # exactly one block never takes the stream: a block of it and its weights are more than the block of rows
    "one_whole_block": (32, 15, [(64, 128)], "tiles=1 split=64+0+0 bytes=3840"),
    # exactly blocks 1 and 2: 11 representatives, [64, 75), in block 1 of the stream alone
    "two_whole_blocks": (32, 15, [(64, 192)], "tiles=1 split=0+2[64-75)+0 bytes=3904"),
    # blocks 0 and 1: [0, 65) touches two blocks of the stream, 2 * 3904 bytes against 2 * 3840 of rows: the rows
    "range_across_stream_blocks": (32, 15, [(0, 128)], "tiles=1 split=128+0+0 bytes=%d" % (2 * 3840)),
    # the whole matrix: the final partial block is a tail, never a whole block
    "whole_matrix": (32, 15, [(0, 269)], "tiles=1 split=0+4[0-77)+13 bytes=%d" % (3840 + 2 * 3904)),
    # tile_blocks 1: every tile is one block
    "tile_blocks_1": (1, 15, [(5, 200)], "tiles=4 split=59+0+0,64+0+0,64+0+0,8+0+0 bytes=%d" % (4 * 3840)),
    # tile_blocks 2 over [0, 269): 5 blocks in 3 parts of 2, 2, 1; the cut falls between whole blocks
    "tile_blocks_2": (2, 15, [(0, 269)], "tiles=3 split=128+0+0,0+2[65-77)+0,13+0+0 bytes=%d" % (2 * 3840 + 3904 + 3840)),
    # nested windows: segments [0,31) [31,64) [64,128) [128,269): one block cut in two has no whole block
    "nested": (32, 3, [(0, 269), (31, 128), (64, 128)], "tiles=4 split=31+0+0,33+0+0,64+0+0,0+2[65-77)+13 bytes=%d" % (3 * 768 + 832 + 768)),
    "empty": (32, 3, [(9, 9), (269, 269)], "tiles=0 split= bytes=0"),
}


@pytest.mark.parametrize("case", sorted(CUT_CASES))
def test_unique_cut(unique_cut_exe, case):
    """The driver checks every property of the split itself (tests/fuzz/unique_cut.cc lists them) and exits non-zero on a breach;
    here: it ran clean under the sanitizers and split where the case's arithmetic says."""
    tile_blocks, wps, windows, line = CUT_CASES[case]
    assert _run(unique_cut_exe, "cut", tile_blocks, wps, N_ROWS, REPS, *[x for w in windows for x in w]) == line


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_unique_cut_random_lists(unique_cut_exe, seed):
    assert _run(unique_cut_exe, "random", seed, 160) == "random ok lists=160"


def test_lane_sum_bound(unique_cut_exe):
    """tile_blocks up to 4096 at wps 16: with the cap on a tile's whole blocks (UNIQ_MID_MAX = 2040) the worst lane of the weighted
    sums reaches 511 x 64 x 2^16 + 2^16 + 2^24, below 2^32"""
    assert _run(unique_cut_exe, "bound") == "bound ok worst=%d" % (511 * 64 * 65536 + 65536 + (1 << 24))
