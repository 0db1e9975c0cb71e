"""csrc/panel_set.h on the host (plain C++, no HIP, no GPU): the K disjoint panels of impop_pairdist_scan, impop_permtest_scan and
impop_pairwise_scan_panel — classes, positions, offsets, the merged list and observed labelling of every pair, and the two refusals —
checked by tests/fuzz/panel_set.cc against its own brute-force model under ASan + UBSan."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def panel_set_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("panel_set") / "panel_set")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "panel_set.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_panel_sets_against_the_model(panel_set_exe, seed):
    """n_hap in {1, 2, 63, 64, 65, 130} x K in 1 .. 8, 20 random disjoint sets each where K panels exist (35 of the 48 shapes); per
    set one overlap and one emptied population (64 per round), and per shape the null masks (48) and, where K > n_hap, an empty
    population (13).  The driver checks every property itself (tests/fuzz/panel_set.cc lists them) and exits non-zero on a breach."""
    r = subprocess.run([panel_set_exe, str(seed), "20"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr[-4000:])
    assert r.stdout.strip() == "panel_set ok sets=700 refusals=1341"
