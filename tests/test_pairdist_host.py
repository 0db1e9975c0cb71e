"""No GPU: the host side of impop_pairdist_scan — the plain restatement against a brute-force loop over sites, pairs and members,
the known answer of the header, the planted features of the GPU tests' inputs, the ABI declaration and its binding, the record
layouts on both sides, and impop_amd/pairdist.py's derived values and row formatting against hand-computed ones."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import pairdist_cases as pc
import plain_pairdist as pp
from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
PANEL_FIELDS = ["n_members", "n_sites", "n_pairs", "sum_h", "sum_h2", "n_zero", "min_h", "max_h", "min_i", "min_j", "max_i", "max_j"]
PAIR_FIELDS = ["n_pairs", "sum_h", "sum_h2", "n_zero", "min_h", "max_h", "min_i", "min_j", "max_i", "max_j", "nn_same_a", "nn_same_b",
               "nn_other_a", "nn_other_b", "snn", "gmin", "reserved"]


def same_records(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in y:
            if isinstance(y[k], float):
                assert np.float64(x[k]).tobytes() == np.float64(y[k]).tobytes(), (k, x[k], y[k])
            else:
                assert int(x[k]) == int(y[k]), (k, x[k], y[k])


@pytest.mark.parametrize("seed", range(12))
def test_restatement_equals_the_brute_force_loops(seed):
    rng = np.random.default_rng(seed)
    n, S = int(rng.integers(2, 13)), int(rng.integers(1, 40))
    m01 = rng.integers(0, 2, size=(n, S), dtype=np.uint8)
    for i in range(1, n):  # copies and near-copies: zero distances and ties
        if rng.random() < 0.4:
            m01[i] = m01[int(rng.integers(0, i))]
            if rng.random() < 0.5:
                m01[i, int(rng.integers(0, S))] ^= 1
    w = rng.integers(1, 5, size=S) if seed % 2 else np.ones(S, np.int64)
    K = int(rng.integers(1, min(n, 4) + 1))
    cls = rng.integers(0, K + 1, size=n)
    cls[:K] = np.arange(K)  # no panel empty
    pops = [[int(i) for i in np.flatnonzero(cls == k)] for k in range(K)]
    bins, width = (0, 1) if seed % 3 == 0 else (int(rng.integers(1, 7)), int(rng.integers(1, 4)))
    got = pp.window(pp.hamming(pp.gram(m01, 0, S, w)), int(w.sum()), pops, bins, width)
    want = pp.brute_window(m01.tolist(), [int(x) for x in w], pops, bins, width)
    same_records(got[0], want[0])
    same_records(got[1], want[1])
    if bins:
        assert [h.tolist() for h in got[2]] == want[2] and [h.tolist() for h in got[3]] == want[3]


def test_known_answer_of_the_header():
    m01 = np.array([[0, 0, 0, 0], [0, 0, 0, 1], [0, 1, 1, 1], [0, 0, 0, 1]], np.uint8)
    H = pp.hamming(pp.gram(m01, 0, 4))
    assert [int(H[i, j]) for i in range(4) for j in range(i + 1, 4)] == [1, 3, 1, 2, 0, 2]
    pa, pr, _, _ = pp.window(H, 4, [[0, 1], [2, 3]])
    assert [(r["n_pairs"], r["sum_h"], r["sum_h2"], r["n_zero"], r["min_h"], r["max_h"], r["min_i"], r["min_j"]) for r in pa] == \
        [(1, 1, 1, 0, 1, 1, 0, 1), (1, 2, 4, 0, 2, 2, 2, 3)]
    r = pr[0]
    assert (r["n_pairs"], r["sum_h"], r["sum_h2"], r["n_zero"]) == (4, 6, 14, 1)
    assert (r["min_h"], r["min_i"], r["min_j"], r["max_h"], r["max_i"], r["max_j"]) == (0, 1, 3, 3, 0, 2)
    assert (r["nn_same_a"], r["nn_same_b"], r["nn_other_a"], r["nn_other_b"]) == (0, 0, 1, 1) and r["snn"] == 0.25 and r["gmin"] == 0.0
    body = HEADER[HEADER.index("#define IMPOP_PAIRDIST_MAX_N"):HEADER.index("typedef struct impop_pairdist_params")]
    body = " ".join(body.replace("*", " ").split())
    for text in ("haplotypes 0000, 0001, 0111, 0001", "H01 = 1, H02 = 3, H03 = 1, H12 = 2, H13 = 0, H23 = 2", "n_pairs 4, sum_h 6, sum_h2 14, n_zero 1",
                 "min_h 0 at (1,3), max_h 3 at (0,2)", "(1,2), (0,1), (1,2), (0,1)", "snn = 0.25", "gmin = 0.0"):
        assert text in body, text


@pytest.mark.parametrize("n,K", [(31, 1), (31, 3), (65, 2), (65, 8)])
def test_planted_inputs_show_their_features(n, K):
    m01 = pc.matrix(n)
    pops = pc.panels(n, K)
    assert all(pops) and sum(len(p) for p in pops) < n and len(set(sum(pops, []))) == sum(len(p) for p in pops)
    seg_H = pc.segment_distances(m01)
    lists = pc.window_lists()
    assert len(lists["tiling"]) == 8 and all(w[1] - w[0] == 3 * pc.SEG for w in lists["sliding"])
    for wins in lists.values():
        Hs = [pc.window_distance(seg_H, w) for w in wins]
        assert (Hs[1] == pp.hamming(pp.gram(m01, wins[1][0], wins[1][1]))).all()
        per = [pp.window(H, w[1] - w[0], pops, pc.BINS, pc.WIDTH) for H, w in zip(Hs, wins)]
        assert all(pc.planted_features(per, K).values()), pc.planted_features(per, K)
        ties = pc.tie_counts(Hs[0], pops)  # the first window: the complemented row and the copies
        assert any(lo >= 2 for lo, _ in ties) and any(hi >= 2 for _, hi in ties), ties


def test_abi_declares_pairdist_scan():
    import impop_amd
    from impop_amd import _lib
    assert re.search(r"#define IMPOP_ABI_VERSION 4\b", HEADER) and _lib.ABI_VERSION == 4
    assert re.search(r"#define IMPOP_PAIRDIST_MAX_N\s+4096u\b", HEADER) and _lib.PAIRDIST_MAX_N == 4096
    assert re.search(r"#define IMPOP_PAIRDIST_MAX_BINS\s+1024u\b", HEADER) and _lib.PAIRDIST_MAX_BINS == 1024
    for fn, n_args in (("impop_pairdist_scan", 11), ("impop_ctx_pairdist_elapsed", 3)):
        assert re.search(r"^int %s\(" % fn, HEADER, re.M) and len(_lib.SIGNATURES[fn][1]) == n_args
        decl = re.search(r"^int %s\((.*?)\);" % fn, HEADER, re.M | re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == n_args
    sides = ((_lib.DistPanel, impop_amd.DIST_PANEL_DTYPE, pp.PANEL_DTYPE, PANEL_FIELDS, "impop_dist_panel", 64),
             (_lib.DistPair, impop_amd.DIST_PAIR_DTYPE, pp.PAIR_DTYPE, PAIR_FIELDS, "impop_dist_pair", 96))
    for struct, dtype, plain, fields, cname, size in sides:
        assert C.sizeof(struct) == size == dtype.itemsize and dtype == plain
        assert [n for n, _ in struct._fields_] == fields == list(dtype.names)
        for name, _ in struct._fields_:  # same offsets on both sides
            assert getattr(struct, name).offset == dtype.fields[name][1]
        assert re.search(r"typedef struct %s \{\s*/\* %d bytes" % (cname, size), HEADER)
    assert _lib.DistPanel.n_pairs.offset == 8 and _lib.DistPanel.min_h.offset == 40 and _lib.DistPanel.max_j.offset == 60
    assert _lib.DistPair.min_h.offset == 32 and _lib.DistPair.nn_same_a.offset == 56 and _lib.DistPair.snn.offset == 72
    assert _lib.DistPair.gmin.offset == 80 and _lib.DistPair.reserved.offset == 88
    assert C.sizeof(_lib.PairdistParams) == 16
    for struct, want in (("impop_dist_panel", PANEL_FIELDS), ("impop_dist_pair", PAIR_FIELDS),
                         ("impop_pairdist_params", ["struct_size", "hist_bins", "hist_width", "reserved"])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert declared == want
    assert [n for n, _ in _lib.PairdistParams._fields_] == ["struct_size", "hist_bins", "hist_width", "reserved"]
    assert hasattr(impop_amd.BitMatrix, "pairdist_scan") and hasattr(impop_amd.Context, "pairdist_elapsed")


def test_derived_values():
    from impop_amd import pairdist as pd
    rec = dict(n_pairs=4, sum_h=6, sum_h2=14, n_zero=1, min_h=0, max_h=3)
    assert pd.mean_h(rec) == 1.5 and pd.variance_h(rec) == (4 * 14 - 36) / 16 == 1.25
    assert math.isnan(pd.mean_h(dict(n_pairs=0, sum_h=0, sum_h2=0))) and math.isnan(pd.variance_h(dict(n_pairs=0, sum_h=0, sum_h2=0)))
    # frequencies 1/4, 1/2, 1/4, then 0: (1/4)^2 + (1/4)^2 + (1/4)^2
    assert pd.raggedness([1, 2, 1]) == 3 / 16 and pd.raggedness([4]) == 1.0 and math.isnan(pd.raggedness([0, 0]))
    assert pd.dmin_per_site(dict(min_h=5), 100) == 0.05
    ko, lo = dict(n_pairs=2, sum_h=20, sum_h2=0), dict(n_pairs=4, sum_h=120, sum_h2=0)  # means 10 and 30
    assert pd.rnd_min(dict(min_h=5), ko, lo) == 5 / 20
    assert math.isnan(pd.rnd_min(dict(min_h=0), dict(n_pairs=1, sum_h=0, sum_h2=0), dict(n_pairs=1, sum_h=0, sum_h2=0)))
    assert pd.pair_order(3) == [(0, 1), (0, 2), (1, 2)] and pd.outgroup_pair_index(3, 1, 2) == 2 and pd.outgroup_pair_index(3, 2, 0) == 1


def test_cli_rows():
    from impop_amd import pairdist as pd
    m01 = np.array([[0, 0, 0, 0], [0, 0, 0, 1], [0, 1, 1, 1], [0, 0, 0, 1]], np.uint8)
    panels, pairs, hw, hb = pp.scan(m01, [(0, 4, 4)], [[0, 1], [2, 3]], bins=3, width=1)
    seq = ["s0", "s1", "s2", "s3"]
    main, pan, hist = pd.tables(["chr:0-4"], [4], ["A", "B"], seq, panels, pairs, hw, hb)
    assert main == [["chr:0-4", "4", "A", "B", "4", "0.375", "0", "s1", "s3", "3", "1", "0.0", "0.25", "0", "0", "1", "1"]]
    assert len(main[0]) == len(pd.MAIN_COLUMNS)
    assert pan == [["chr:0-4", "A", "2", "1", "1.0", "0.0", "1", "1", "0", repr(pd.raggedness([0, 1, 0]))],
                   ["chr:0-4", "B", "2", "1", "2.0", "0.0", "2", "2", "0", repr(pd.raggedness([0, 0, 1]))]]
    assert len(pan[0]) == len(pd.PANEL_COLUMNS)
    assert hist == [["chr:0-4", "between", "A:B", "0", "1"], ["chr:0-4", "between", "A:B", "1", "1"], ["chr:0-4", "between", "A:B", "2", "2"],
                    ["chr:0-4", "within", "A", "1", "1"], ["chr:0-4", "within", "B", "2", "1"]]
    # without histograms RAGGEDNESS is NA; a one-member panel has no pairs: NA for its mean; NaN gmin prints NA
    one = np.zeros((1, 2), pp.PANEL_DTYPE)
    one[0, 0]["n_members"] = 1
    one[0, 0]["min_i"] = one[0, 0]["min_j"] = pp.NONE
    assert pd.panel_row("r", "A", one[0, 0]) == ["r", "A", "1", "0", "NA", "NA", "0", "0", "0", "NA"]
    same = pp.scan(np.zeros((2, 3), np.uint8), [(0, 3, 3)], [[0], [1]])
    assert pd.main_row("r", 3, ["A", "B"], 0, 1, same[1][0, 0], ["x", "y"])[11] == "NA"
    # an outgroup adds RNDMIN: NA for the pairs that hold it.  min H(A, B) = H01 = H03 = 1, mean H(A, O) = H02 = 3, mean H(B, O) = (2 + 2) / 2
    p3 = pp.scan(m01, [(0, 4, 4)], [[0], [1, 3], [2]])
    main3, _, _ = pd.tables(["r"], [4], ["A", "B", "O"], seq, p3[0], p3[1], outgroup=2)
    assert [r[-1] for r in main3] == [repr(1 / ((3 + 2) / 2)), "NA", "NA"] and len(main3[0]) == len(pd.MAIN_COLUMNS) + 1


@pytest.mark.parametrize("extra,env,needle", [
    (["--devices", "2"], {}, "--devices"),
    ([], {"WORLD_SIZE": "2"}, "torch.distributed.run"),
    (["--pairdist-hist", "h.tsv"], {}, "--pairdist-bins"),
    (["--pairdist-outgroup", "2"], {}, "at least three lists"),
    (["-t", "0.99"], {}, "-t / -r"),
])
def test_cli_refusals_need_no_device(extra, env, needle):
    """what --format pairdist does not combine with: one line on stderr and exit code 2, before any file or device is opened"""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", "none.npz", "--bed", "none.bed", "--format",
                        "pairdist", "--panel", "a.txt", "b.txt"] + extra, capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, **env), timeout=120)
    assert r.returncode == 2 and needle in r.stderr and r.stdout == "", (r.returncode, r.stderr)
