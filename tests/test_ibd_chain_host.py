"""No GPU: csrc/ibd_chain.h — the genetic map and the chain step of impop_ibd_scan — through the stand-alone driver
tests/fuzz/ibd_chain.cc, built with ASan + UBSan; the plain restatement (tests/plain_ibd.py) against the header's known answers;
the shared cases' conditions; the ABI's declarations; the .map reader, the table writers and the command line's refusals."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ibd_cases as bc
import plain_ibd as pd
from conftest import ROOT

SCRIPT = os.path.join(ROOT, "scripts", "impop_ibd.py")


@pytest.fixture(scope="module")
def ibd_chain_exe(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ibd_chain") / "ibd_chain")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++", os.path.join(ROOT, "tests", "fuzz", "ibd_chain.cc"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


@pytest.mark.parametrize("seed", (1, 20261020, 977))
def test_batched_chains_equal_the_direct_evaluation(ibd_chain_exe, seed):
    r = subprocess.run([ibd_chain_exe, str(seed), "1500"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok 1500", (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_the_header_is_plain_cxx():
    """no HIP types: the device and the host run the same code"""
    src = open(os.path.join(ROOT, "impop_amd", "csrc", "ibd_chain.h")).read()
    assert "hip/hip_runtime.h" not in src and "__global__" not in src and "__shfl" not in src and "threadIdx" not in src
    assert "DIP_HD" in src and "ibd_map_eval" in src and "ibd_chain_lanes" in src and "ibd_chain_batch" in src
    dev = open(os.path.join(ROOT, "impop_amd", "csrc", "ibd.hip")).read()
    assert '#include "ibd_chain.h"' in dev and "ibd_map_eval(" in dev and "ibd_chain_lanes(" in dev


def test_known_answers_of_the_header():
    m01 = bc.known_matrix()
    assert pd.tracts_of(m01[0], m01[1], 0, 40) == [(0, 10), (11, 12), (13, 30), (31, 40)]
    gm = (bc.KNOWN_MAP[0], bc.KNOWN_MAP[1])
    assert [pd.G(gm, x) for x in (13, 30, 31, 0, 40, 45)] == [65, 110, 111, 0, 120, 120]
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    assert "G(13) = 65, G(30) = 110, G(31) = 111" in header and "[0,10), [11,12), [13,30), [31,40)" in header
    for rule, gmap, want in bc.KNOWN:
        rec, seg, _ = pd.reference(m01, [(0, 1)], 0, 40, gmap=gmap, **rule)
        assert [tuple(int(s[f]) for f in ("begin", "end", "len", "n_tracts", "ibs_sites", "flags")) for s in seg] == want, rule
        assert int(rec["n_segments"][0]) == len(want)


def test_cases_meet_their_conditions():
    for with_map in (False, True):
        c = bc.geometry_case(33, with_map)  # Case() asserts the five conditions
        assert c.stats["no_seed"] > 0 and c.stats["too_short"] > 0 and int(c.want[0]["n_candidates"].max()) > 64
    one = bc.hand_case(1)
    seg = one.want[1]
    assert len(seg) == 1 and (int(seg["begin"][0]), int(seg["end"][0]), int(seg["n_tracts"][0])) == (69, 700, 79)
    none = bc.hand_case(0).want[1]
    assert [(int(s["begin"]), int(s["end"]), int(s["n_tracts"])) for s in none] == [bc.HAND_SEED + (1,)]
    assert len(bc.hand_case(0, 3, 3).want[1]) == 79


def test_abi_declares_ibd_scan():
    from impop_amd import _lib
    import impop_amd
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    for name in ("impop_ibd_scan", "impop_ctx_ibd_elapsed"):
        assert name in _lib.SIGNATURES and f"int {name}(" in header
    assert _lib.ABI_VERSION == 4  # additive only
    assert C.sizeof(_lib.IbdParams) == 88 and C.sizeof(_lib.IbdPair) == 48 and C.sizeof(_lib.IbdSegment) == 48
    assert impop_amd.IBD_PAIR_DTYPE == pd.PAIR and impop_amd.IBD_SEGMENT_DTYPE == pd.SEGMENT
    for dt, st in ((impop_amd.IBD_PAIR_DTYPE, _lib.IbdPair), (impop_amd.IBD_SEGMENT_DTYPE, _lib.IbdSegment)):
        assert [(n, dt.fields[n][1]) for n in dt.names] == [(n, getattr(st, n).offset) for n, _ in st._fields_]
    assert "ibd.hip" in open(os.path.join(ROOT, "impop_amd", "build.py")).read()


def test_plink_map_reader(tmp_path):
    from impop_amd import ibd
    assert [ibd.centimorgans(x) for x in ("0", "1.0000005", "1.0000015", "2.5", "0.0000004")] == [0, 1000000, 1000002, 2500000, 0]
    p = tmp_path / "a.map"
    p.write_text("chr1 a 0.5 900\nchr2 x 9 950\nchr1 b 1.5 1100\n1\tc\t1.5\t1200\nCHM13#0#chr1 d 3.25 5000\n")
    pos, g = ibd.read_plink_map(str(p), "chr1", 1000)
    assert pos == [0, 100, 200, 4000] and g == [1000000, 1500000, 1500000, 3250000]  # site 0: halfway between 900 and 1100
    pos, g = ibd.read_plink_map(str(p), "chr1", 100)
    assert pos == [800, 1000, 1100, 4900] and g == [500000, 1500000, 1500000, 3250000]
    assert ibd.read_plink_map(str(p), "chr2", 0) == ([950], [9000000])
    for bad in ("chr1 a 0.5 900\nchr1 b 0.6 900\n", "chr1 a 0.5 900\nchr1 b 0.6 800\n", "chr1 a 0.5\n", "chr1 a x 5\n", "chr1 a -1 5\n"):
        p.write_text(bad)
        with pytest.raises(ValueError):
            ibd.read_plink_map(str(p), "chr1", 0)


def test_writers_on_hand_made_records():
    from impop_amd import ibd
    seg = np.zeros(2, dtype=pd.SEGMENT)
    seg[0] = (0, 1, 5, 30, 2500001, 20, 2, 0, 1)
    seg[1] = (1, 2, 40, 50, 10, 10, 1, 1, 2)
    names = ["a", "b", "c"]
    assert ibd.segment_rows(names, seg, lambda s: 1000 + s, True) == [["a", "b", "1005", "1030", "2500001", "2", "20", "L", "2.500001"],
                                                                        ["b", "c", "1040", "1050", "10", "1", "10", "R", "0.000010"]]
    assert ibd.segment_rows(names, seg[1:], lambda s: s, False) == [["b", "c", "40", "50", "10", "1", "10", "R"]]
    rec = np.zeros(1, dtype=pd.PAIR)
    rec[0] = (0, 2, 3, 9, 100, 90, 60, 80)
    assert ibd.pair_rows(names, rec) == [["a", "c", "3", "9", "100", "90", "60", "80"]]
    win = np.zeros(2, dtype=pd.WINDOW)
    win[0] = (12, 3, 1, 10, 0, 0.4)
    win[1] = (0, 0, 0, 0, 0, np.nan)
    assert ibd.main_rows(["r1", "r2"], [10, 0], [3, 3], win) == [["r1", "10", "3", "3", "1", "12", "0.40000000"], ["r2", "0", "3", "0", "0", "0", "NA"]]


@pytest.mark.parametrize("extra, needle", [
    ([], "without --ibd-map the lengths are sites"),
    (["--ibd-min-seed", "5", "--ibd-min-extend", "2"], "without --ibd-map the lengths are sites"),
    (["--ibd-min-seed", "5", "--ibd-min-extend", "9", "--ibd-min-output", "5"], "below --ibd-min-extend"),
    (["--ibd-min-seed", "1.5", "--ibd-min-extend", "1", "--ibd-min-output", "5"], "whole number of sites"),
    (["--ibd-map", "none.map", "--ibd-min-seed", "x"], "not a number of centimorgans"),
    (["--ibd-map", "none.map", "--ibd-min-sites", "0"], "--ibd-min-sites takes 1 or more"),
])
def test_script_refuses_before_it_opens_a_file(extra, needle):
    r = subprocess.run([sys.executable, SCRIPT, "--matrix", "none.npz", "--bed", "none.bed"] + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and needle in r.stderr, r.stderr[-2000:]
