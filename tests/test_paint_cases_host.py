"""No GPU: the plain restatement of impop_paint_scan (tests/paint_cases.py) against the header's known answers and against the
exhaustive enumeration of every path, and switch_costs_from_map at hand-computed values."""
import itertools
import math

import numpy as np
import pytest

import paint_cases as pc
from impop_amd.paint import MAX_COST, switch_costs_from_map


@pytest.mark.parametrize("mu,c", sorted(pc.KNOWN))
def test_known_answers(mu, c):
    cost, n_mismatch, segments = pc.KNOWN[(mu, c)]
    got = pc.reference(pc.known_matrix(), [0], donors=[0, 1, 1, 1], mu=mu, c=c)
    r = got["recipients"][0]
    assert (int(r["cost"]), int(r["n_mismatch"]), int(r["n_donors"]), int(r["n_segments"])) == (cost, n_mismatch, 3, len(segments))
    assert [(int(s["donor"]), int(s["begin"]), int(s["end"])) for s in got["segments"]] == segments
    assert int(got["segments"]["n_sites"].sum()) == 12 and int(got["segments"]["n_mismatch"].sum()) == n_mismatch
    assert got["chunk_counts"][0].tolist() == [0] + [sum(1 for d, _, _ in segments if d == h) for h in (1, 2, 3)]
    assert got["chunk_sites"][0].tolist() == [0] + [sum(e - b for d, b, e in segments if d == h) for h in (1, 2, 3)]


def test_exhaustive_paths():
    """all K^L paths for K <= 3, L <= 7: the restatement's cost is the minimum and its path attains it"""
    rng = np.random.default_rng(20261021)
    for trial in range(120):
        K, L = int(rng.integers(1, 4)), int(rng.integers(1, 8))
        x = (rng.random(L) < 0.5).astype(np.uint8)
        D = (rng.random((K, L)) < 0.5).astype(np.uint8)
        if trial % 4 == 0 and K > 1:
            D[1] = D[0]  # a duplicated donor: ties
        mu = int(rng.integers(1, 4))
        cs = rng.integers(0, 4, size=L) if trial % 3 else np.full(L, mu)
        cost, d = pc.viterbi(x, D, mu, cs)
        best = min(pc.path_cost(x, D, mu, cs, p) for p in itertools.product(range(K), repeat=L))
        assert cost == best == pc.path_cost(x, D, mu, cs, d), (trial, cost, best)


def test_all_identical_rows():
    m01 = np.tile((np.arange(40) % 3 == 0).astype(np.uint8), (6, 1))
    got = pc.reference(m01, [2, 0], donors=[1, 0, 1, 1, 0, 1], mu=3, c=2, b=4, e=33)
    assert got["recipients"]["cost"].tolist() == [0, 0] and got["n_segments"] == 2
    assert [(int(s["h"]), int(s["donor"]), int(s["begin"]), int(s["end"]), int(s["n_sites"])) for s in got["segments"]] == \
        [(2, 0, 4, 33, 29), (0, 2, 4, 33, 29)]  # the lowest admissible donor; a haplotype never copies from itself


def test_groups_and_windows_add_up():
    rng = np.random.default_rng(5)
    m01 = pc.mosaic_matrix(rng, 8, 90)
    group = np.arange(8) // 2
    panel = np.array([0, 0, 1, 1, 255, 255, 2, 2])
    wins = pc.partition_windows(10, 85)
    got = pc.reference(m01, [0, 3, 5], mu=2, c=3, group=group, panel=panel, n_panels=3, b=10, e=85, windows=wins)
    for s in got["segments"]:
        assert group[s["donor"]] != group[s["h"]]
    assert int(got["windows"]["cells"].sum()) == 3 * 75
    assert int(got["windows"]["n_switches"].sum()) == int((got["recipients"]["n_segments"] - 1).sum())
    assert (got["anc"].sum(axis=1)[:, :3] == got["windows"]["copied"][:, :3]).all()
    assert (got["anc"].sum(axis=1)[:, 3] == got["windows"]["copied"][:, 8]).all()
    assert (got["windows"]["copied"].sum(axis=1) == got["windows"]["cells"]).all()


def test_switch_costs_from_map():
    # sites 1000 bp apart on a map of 1 cM per 1 Mb: d = 1e-5 Morgans; rho = 100: p = 1 - exp(-1e-3)
    pos = [0, 1000, 2000, 2000, 1002000]
    c = switch_costs_from_map(pos, [0, 2000000], [0.0, 2.0], rho=100.0, scale=10.0)
    p = 1.0 - math.exp(-100.0 * 1e-5)
    assert 0.00099 < p < 0.001
    want = math.floor(10.0 * math.log((1.0 - p) / p) + 0.5)
    assert want == 69  # 10 ln(999.5) = 69.07
    assert c.dtype == np.uint32 and c.tolist()[:4] == [0, want, want, MAX_COST]  # entry 0 is ignored; d = 0 gives 2^20
    # 1 Mb = 1e-2 Morgans: p = 1 - e^-1 = 0.632 > 1/2: a switch is likelier than a stay, the cost is 0
    assert c[4] == 0
    # the cap: a tiny distance
    assert switch_costs_from_map([0, 1], [0, 10 ** 9], [0.0, 1.0], rho=1.0, scale=1e6)[1] == MAX_COST
    # scale 1, p = 1/4: ln 3 = 1.0986 -> 1
    d = -math.log(0.75)
    assert switch_costs_from_map([0, 1], [0, 1], [0.0, 100.0 * d], rho=1.0, scale=1.0)[1] == 1
