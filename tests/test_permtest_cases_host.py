"""No GPU: the inputs of the impop_permtest_scan GPU tests (tests/permtest_cases.py) have the properties those tests rely on, under
the plain restatement: the planted windows beat every labelling in all four tests, the exchangeable window ties with every one, the
tie case passes 16 ties, every multi-plane case passes 255 or 65535."""
import numpy as np

import permtest_cases as pc
import plain_permtest as pt

SEED = 12345  # the GPU tests' seed


def labels_of(n_perm):
    return lambda p, m, m_k: pt.labels(SEED, p, m, m_k, n_perm)


def test_planted_windows_beat_and_exchangeable_windows_tie_with_every_labelling():
    m01, pops, wins = pc.planted_case()
    n_perm = 100
    per = [pt.window(pt.hamming(pt.gram(m01, w[0], w[1])), w[1] - w[0], pops, labels_of(n_perm))[0][0] for w in wins]
    for w, ge in ((0, 0), (1, n_perm), (2, 0)):
        assert [per[w]["ge_" + t] for t in ("fst", "phi", "dxy", "snn")] == [ge] * 4, (w, per[w])
    assert per[1]["wa"] + per[1]["wb"] + per[1]["ab"] == 0 and per[0]["fst"] > 0.9 and per[0]["snn"] == 1.0


def test_tie_case_passes_sixteen_ties():
    m01, pops = pc.tie_case()
    rec = pt.window(pt.hamming(pt.gram(m01, 0, 64)), 64, pops, labels_of(2))[0][0]
    assert rec["tied_max"] == 17 and pt.SCALE % rec["tied_max"] != 0
    H = pt.hamming(pt.gram(m01, 0, 64))
    assert H[20, 30] == 0 and H[20, 31] == 0 and 20 in pops[0] and 30 in pops[1]  # duplicates across the panels


def test_multi_plane_cases_pass_a_byte_and_two():
    m01, wins = pc.plane_case()
    pops = [list(range(0, 24, 2)), list(range(1, 24, 2))]
    h = [pt.window(pt.hamming(pt.gram(m01, w[0], w[1])), w[1] - w[0], pops, labels_of(1))[0][0]["h_max"] for w in wins]
    assert h[0] == 0 and h[1] <= 1 and 255 < h[2] <= 65535
    node, wt, node_wins, expanded, bp_wins = pc.weighted_case()
    assert expanded.shape[1] == int(wt.sum()) and int(wt[0:40].sum()) > 65535
    rec = pt.window(pt.hamming(pt.gram(node, 0, 40, wt)), int(wt.sum()), [list(range(0, 11)), list(range(11, 24))], labels_of(1))[0][0]
    assert rec["h_max"] > 65535
    assert (pt.hamming(pt.gram(node, 0, 40, wt)) == pt.hamming(pt.gram(expanded, bp_wins[0][0], bp_wins[0][1]))).all()


def test_shapes_are_what_their_names_say():
    for name, (sizes, n) in pc.SHAPES.items():
        pops = pc.panels(sizes, n)
        flat = [i for p in pops for i in p]
        assert [len(p) for p in pops] == list(sizes) and len(set(flat)) == len(flat) and max(flat) < n, name
    assert sum(pc.SHAPES["k3"][0]) < pc.N and sum(pc.SHAPES["k8_n65"][0]) == 65 and sum(pc.SHAPES["37_29"][0]) > 64
    assert sum(pc.SHAPES["70_61"][0]) > 128
    m01, pops, wins = pc.upper_case()
    assert m01.shape == (1024, 200) and [len(p) for p in pops] == [512, 512] and len(wins) == 2
