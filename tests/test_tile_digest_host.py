"""csrc/tile_digest.h on the host (plain C++, no HIP, no GPU): what a tile of a plan's digest may hold — the bound on a lane's 32-bit
sums and the caps it gives — when a plan takes the digest, and the layout's arithmetic, checked by tests/fuzz/tile_digest.cc under
ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("tile_digest") / "tile_digest")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "tile_digest.cc"),
                        "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-4000:])
    return r.stdout.strip()


def test_worst_lane_stays_under_the_bound(exe):
    """every size the caps admit, wps 1 .. 16.  The worst lane seen is at least the caps' own at n = 512: 32 768 common rows of
    c (n - c) = 2^16 in one lane (2^31) and 65 535 singletons of 511 each through the histogram"""
    out = _run(exe, "bound")
    assert out.startswith("bound ok sizes="), out
    worst = int(out.rpartition("worst=")[2])
    assert 2**31 + 65535 * 511 <= worst < 2**32, out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_layout_and_rule_random(exe, seed):
    assert _run(exe, "random", seed, 3000) == "random ok n=3000"


# (candidates, common rows, singletons, entries): DIGEST_ROWS_MAX = 512 candidates, 512 x 64 = 32 768 common rows (a candidate
# stands for at most 64), DIGEST_SINGLES_MAX = 65 535 (a uint16 count), WAVE_RARE_WORDS_MAX = 2^18 entries
FITS_CASES = {
    (0, 0, 0, 0): 1,
    (130, 400, 2216, 46): 1,          # a headline tile: head + representatives + tail, 2 216 singletons, 46 entries
    (512, 512, 0, 0): 1,
    (513, 513, 0, 0): 0,
    (512, 32768, 65535, 2**18): 1,    # every cap at once
    (512, 32769, 0, 0): 0,
    (1, 1, 65536, 0): 0,
    (1, 1, 0, 2**18 + 1): 0,
}
# (site_begin, site_end, uniq_begin, uniq_end): head + representatives + tail, or every row where the tile has no range
CANDIDATE_CASES = {
    (0, 0, 0, 0): 0,
    (5, 200, 0, 0): 195,
    (5, 300, 64, 130): 59 + 66 + 44,      # head [5, 64), 66 representatives for blocks 1 .. 3, tail [256, 300)
    (64, 320, 0, 63): 63,                 # neither head nor tail
    (64, 330, 127, 129): 2 + 10,
}
# (single_begin, single_end, wps): a histogram is 64 wps bytes; the range reads the 8-byte words it touches
HIST_CASES = {
    (0, 0, 15): 0,
    (0, 2216, 15): 1,       # 554 words = 4 432 bytes against 960
    (0, 480, 15): 1,        # 120 words = 960 bytes: no shorter than the histogram
    (0, 476, 15): 0,        # 119 words
    (3, 479, 15): 1,        # 476 singletons again, across 120 words
    (0, 20, 5): 0,
    (10, 10, 1): 0,
}
# (override, reusable, wave_tiles, all_fit, bytes with the digest, bytes without)
CHOICE_CASES = {
    (-1, 1, 1, 1, 100, 100): 1,
    (-1, 1, 1, 1, 101, 100): 0,       # the byte rule
    (-1, 0, 1, 1, 50, 100): 0,        # a one-shot plan
    (-1, 1, 0, 1, 50, 100): 0,        # not the one-wave body
    (-1, 1, 1, 0, 50, 100): 0,        # a tile above the caps
    (0, 1, 1, 1, 50, 100): 0,
    (1, 0, 1, 1, 500, 100): 1,        # forced: one-shot calls included, byte rule ignored
    (1, 1, 0, 1, 50, 100): 0,
    (1, 1, 1, 0, 50, 100): 0,
}


def test_fixed_cases(exe):
    assert {k: _run(exe, "fits", *k) for k in FITS_CASES} == {k: f"fits={v}" for k, v in FITS_CASES.items()}
    assert {k: _run(exe, "candidates", *k) for k in CANDIDATE_CASES} == {k: f"candidates={v}" for k, v in CANDIDATE_CASES.items()}
    assert {k: _run(exe, "hist", *k) for k in HIST_CASES} == {k: f"hist={v}" for k, v in HIST_CASES.items()}
    assert {k: _run(exe, "choice", *k) for k in CHOICE_CASES} == {k: f"digest={v}" for k, v in CHOICE_CASES.items()}
