"""csrc/tile_cut.h on the host (plain C++, no HIP, no GPU): when a plan runs the one-wave-per-tile body of the fixed-WPS kernel —
the bound on a lane's 32-bit sums, the cap it gives and the default rule — checked by tests/fuzz/wave_tiles.cc under ASan + UBSan."""
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
    out = str(tmp_path_factory.mktemp("wave_tiles") / "wave_tiles")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "wave_tiles.cc"),
                        "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-4000:])
    return r.stdout.strip()


def test_worst_lane_stays_under_the_bound(exe):
    """every size the cap admits, wps 1 .. 16.  The worst lane seen is at least the cap itself at n = 512, all its rare words
    singletons: 512 blocks x 64 x 2^16 = 2^31 for the rows and ceil(2^18 / 64) = 4096 words of 4 x 511 (a carrier in P, nP = 512)"""
    out = _run(exe, "bound")
    assert out.startswith("bound ok sizes="), out
    worst = int(out.rpartition("worst=")[2])
    assert 2**31 + 4096 * 4 * 511 <= worst < 2**32, out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_rule_random(exe, seed):
    assert _run(exe, "random", seed, 20000) == "random ok n=20000"


# (n_tiles, largest tile's blocks read, largest tile's rare words, n_cu): the rule.  Thresholds of tile_cut.h: at least
# WAVE_RULE_TILES_PER_CU = 8 tiles per CU (n_cu <= 0 counts as 256), at most WAVE_RULE_BLOCKS = 6 blocks and
# WAVE_RULE_RARE_WORDS = 1536 rare words, under the cap of WAVE_BLOCKS_MAX = 512 blocks and WAVE_RARE_WORDS_MAX = 2^18 rare words
RULE_CASES = {
    (4854, 5, 700, 256): 1,        # the headline plan: 4 854 >= 2 048 tiles of at most 5 blocks, 46 entries + 550 singleton words
    (2048, 5, 700, 256): 1,        # exactly 8 n_cu
    (2047, 5, 700, 256): 0,        # one short: four-wave workgroups reach more SIMDs
    (2047, 5, 700, 0): 0,          # no CU count: 256
    (2048, 5, 700, 0): 1,
    (2432, 5, 700, 304): 1,        # 8 x 304
    (2431, 5, 700, 304): 0,
    (4854, 6, 1536, 256): 1,       # both thresholds, reached
    (4854, 7, 700, 256): 0,        # 150 kb windows as one tile: level with four waves, which then stay
    (4854, 5, 1537, 256): 0,
    (100000, 513, 0, 256): 0,      # above the cap
    (100000, 0, 2**18 + 1, 256): 0,
    (0, 0, 0, 256): 0,             # no tile
}
# (override, ...): 0 never, 1 whenever the cap allows, -1 the rule
CHOICE_CASES = {
    (0, 4854, 4, 600, 256): 0,
    (1, 1, 4, 600, 256): 1,            # forced: one tile will do
    (1, 1, 512, 2**18, 256): 1,        # at the cap
    (1, 4854, 513, 600, 256): 0,       # above it, whatever the override says
    (1, 4854, 4, 2**18 + 1, 256): 0,
    (-1, 4854, 4, 600, 256): 1,
    (-1, 4854, 16, 600, 256): 0,       # the rule refuses what the override would take
    (1, 4854, 16, 600, 256): 1,
    (-1, 1, 4, 600, 256): 0,
}


def test_rule(exe):
    got = {k: _run(exe, "rule", *k) for k in RULE_CASES}
    assert got == {k: f"wave_tiles={v}" for k, v in RULE_CASES.items()}


def test_choice(exe):
    got = {k: _run(exe, "choice", *k) for k in CHOICE_CASES}
    assert got == {k: f"wave_tiles={v}" for k, v in CHOICE_CASES.items()}


# (site_begin, site_end, rare_begin, rare_end, single_begin, single_end, uniq_begin, uniq_end): blocks read, rare words
TILE_CASES = {
    (0, 0, 0, 0, 0, 0, 0, 0): (0, 0),
    (5, 200, 0, 0, 0, 0, 0, 0): (4, 0),               # no range of the stream: blocks 0 .. 3 of the rows
    (5, 300, 10, 56, 0, 0, 64, 130): (4, 46),         # head and tail block; representatives [64, 130) touch blocks 1 and 2 of the stream
    (64, 320, 0, 0, 0, 0, 0, 63): (1, 0),             # no head, no tail, one block of the stream
    (64, 330, 0, 0, 3, 2203, 127, 129): (3, 551),     # a tail; [127, 129) touches two blocks; singletons [3, 2203) are words [0, 551)
    (0, 0, 7, 8, 4, 5, 0, 0): (0, 2),                 # one entry, one singleton
}


def test_tile_sizes(exe):
    got = {k: _run(exe, "tile", *k) for k in TILE_CASES}
    assert got == {k: f"blocks={v[0]} rare_words={v[1]}" for k, v in TILE_CASES.items()}
