"""No GPU: the plain restatement of impop_ldband_scan (tests/ldband_cases.py) against the header's known answer, the identities its
outputs must satisfy, an O(q B) brute force of the pruning rule, the scalar pair arithmetic of ld_cases.pair_scalar, and the
invariance under flipped alleles — so that the GPU tests compare the kernels with something that was itself checked."""
import numpy as np
import pytest

import hap_cases as hc
import ld_cases as lc
import ldband_cases as bc


def test_known_answer():
    m01 = np.ascontiguousarray(bc.KNOWN_ROWS.T)
    p = bc.KNOWN_PARAMS
    rec, bins, tab = bc.reference(m01, None, [(0, 5)], p["min_mac"], p["band_sites"], p["max_dist"], p["bin_width"], p["n_bins"],
                                  p["threshold"])
    K = bc.KNOWN
    for k in ("n_pairs", "sum_r2_fx", "n_perfect", "n_strong", "n_kept"):
        assert int(rec[k][0]) == K[k], k
    assert (int(rec["n_members"][0]), int(rec["n_sites"][0]), int(rec["n_qualifying"][0]), int(rec["site_off"][0])) == (4, 5, 5, 0)
    assert tab["kept"].tolist() == K["kept"] and tab["ld_score_fx"].tolist() == K["ld_score_fx"]
    assert tab["n_partners"].tolist() == K["n_partners"] and tab["carriers"].tolist() == K["carriers"]
    assert tab["n_strong"].tolist() == K["n_strong_site"] and tab["coord"].tolist() == [0, 1, 2, 3, 4]
    assert [(int(bins["pairs"][0, b]), int(bins["sum_r2_fx"][0, b]), int(bins["n_strong"][0, b])) for b in range(3)] == K["bins"]
    assert rec["mean_r2"][0] == 4652881236.0 / (10.0 * 1073741824.0)
    # the header's own cross-checks, and fx of 4/12
    assert sum(K["ld_score_fx"]) == 2 * K["sum_r2_fx"] and sum(b[1] for b in K["bins"]) == K["sum_r2_fx"]
    assert int((4.0 / 12.0) * 1073741824.0) == 357913941 and 3 * bc.FX_ONE + 4 * 357913941 == K["sum_r2_fx"]


CASES = [dict(min_mac=1, band_sites=64, max_dist=0), dict(min_mac=2, band_sites=300, max_dist=0), dict(min_mac=2, band_sites=7, max_dist=150),
         dict(min_mac=24, band_sites=1024, max_dist=0)]


@pytest.fixture(scope="module")
def planted():
    m01 = bc.planted_matrix(np.random.default_rng(31000 + 33), 33, p_flip=1e-3)
    flags = (np.random.default_rng(5).random(33) < 0.7).astype(np.uint8)
    flags[:3] = 1
    return m01, flags


@pytest.mark.parametrize("case", range(len(CASES)))
def test_identities(planted, case):
    m01, flags = planted
    wins = bc.window_list()
    for f in (None, flags):
        rec, bins, tab = bc.reference(m01, f, wins, bin_width=50, n_bins=16, threshold=(1, 5), **CASES[case])
        assert np.array_equal(bins["pairs"].sum(axis=1), rec["n_pairs"])
        assert np.array_equal(bins["sum_r2_fx"].sum(axis=1), rec["sum_r2_fx"])
        assert np.array_equal(bins["n_strong"].sum(axis=1), rec["n_strong"])
        assert (rec["n_perfect"] <= rec["n_strong"]).all() and (rec["n_kept"] <= rec["n_qualifying"]).all()
        assert np.array_equal(np.cumsum(rec["n_qualifying"]) - rec["n_qualifying"], rec["site_off"])
        for i in range(len(wins)):
            a, z = int(rec["site_off"][i]), int(rec["site_off"][i] + rec["n_qualifying"][i])
            assert int(tab["ld_score_fx"][a:z].sum(dtype=np.uint64)) == 2 * int(rec["sum_r2_fx"][i])
            assert int(tab["n_partners"][a:z].sum(dtype=np.uint64)) == 2 * int(rec["n_pairs"][i])
            assert int(tab["n_strong"][a:z].sum(dtype=np.uint64)) == 2 * int(rec["n_strong"][i])
            assert int(tab["kept"][a:z].sum()) == int(rec["n_kept"][i]) and (z == a or tab["kept"][a] == 1)
            assert (np.diff(tab["coord"][a:z].astype(np.int64)) > 0).all()
        assert np.isnan(rec["mean_r2"][rec["n_pairs"] == 0]).all() and (rec["mean_r2"][rec["n_pairs"] > 0] <= 1.0).all()
        # among 33 haplotypes no minor allele has 24 carriers: that case is the one where nothing qualifies anywhere
        assert (rec["n_pairs"] == 0).any() and (rec["n_pairs"] > 0).any() == (CASES[case]["min_mac"] <= 16)


def test_the_planted_window_is_not_trivial():
    """window (1000, 1051) holds the five planted columns: q = 5, 10 pairs, three of them perfect; 6 strong at 1/5; 2 kept"""
    for n in (33, 465):
        m01 = bc.planted_matrix(np.random.default_rng(31000 + n), n, p_flip=1e-3)
        lc.check_planted(m01)
        rec, _, tab = bc.reference(m01, None, [(1000, 1051)], 1, 64, 0, 50, 16, (1, 5))
        assert (int(rec["n_qualifying"][0]), int(rec["n_pairs"][0]), int(rec["n_perfect"][0])) == (5, 10, 3)
        assert int(rec["n_strong"][0]) == 6 and int(rec["n_kept"][0]) == 2 and tab["kept"].tolist() == [1, 0, 0, 0, 1]


def brute_kept(strong_band):
    """kept_j = 1 iff no i < j is kept and strong with j inside the band"""
    q = len(strong_band)
    kept = []
    for j in range(q):
        kept.append(0 if any(kept[i] and strong_band[i, j] for i in range(j)) else 1)
    return kept


@pytest.mark.parametrize("band_sites,max_dist", [(1, 0), (3, 0), (64, 0), (65, 40), (300, 0), (1024, 0)])
def test_pruning_equals_brute_force(band_sites, max_dist):
    rng = np.random.default_rng(31100 + band_sites)
    n = 40
    m01 = hc.founder_matrix(rng, n, 500, nf=4, p_site=0.7, p_flip=2e-3)
    qs = bc.qualifying(m01, None, 2)
    assert len(qs) > 200
    rows = m01[:, qs].T
    _, band, strong, _, _ = bc.window_tables(rows, qs, n, band_sites, max_dist, 50, 16, (1, 5))
    sb = band & strong
    kept = bc.prune(sb, band_sites)
    assert kept == brute_kept(sb) and 0 < sum(kept) < len(qs)
    _, _, tab = bc.reference(m01, None, [(0, 500)], 2, band_sites, max_dist, 50, 16, (1, 5))
    assert tab["kept"].tolist() == kept


def test_fx_is_pair_scalar_scaled_and_truncated():
    rng = np.random.default_rng(31200)
    n = 61
    m01 = hc.founder_matrix(rng, n, 300, nf=5, p_site=0.6, p_flip=5e-3)
    flags = (rng.random(n) < 0.8).astype(np.uint8)
    P = bc.members(m01, flags)
    qs = bc.qualifying(m01, flags, 1)
    rows = m01[P][:, qs].T
    fx, band, strong, perfect, bins = bc.window_tables(rows, qs, len(P), 9, 0, 7, 5, (3, 10))
    seen = 0
    for j, k in zip(*np.nonzero(band)):
        num, den, r2, _, _ = lc.pair_scalar(rows[j], rows[k], len(P))
        assert int(fx[j, k]) == int(r2 * 1073741824.0) and 0 <= int(fx[j, k]) <= bc.FX_ONE
        assert bool(strong[j, k]) == (num * num * 10 > 3 * den) and bool(perfect[j, k]) == (num * num == den)
        assert int(bins[j, k]) == min((int(qs[k]) - int(qs[j])) // 7, 4)
        seen += 1
    assert seen > 500 and strong[band].any() and not strong[band].all()


def test_flipping_alleles_changes_nothing(planted):
    m01, flags = planted
    rng = np.random.default_rng(31300)
    flipped = m01.copy()
    cols = rng.random(m01.shape[1]) < 0.4
    flipped[:, cols] ^= 1
    wins = bc.window_list()
    a = bc.reference(m01, flags, wins, 2, 20, 0, 50, 16, (1, 5))
    b = bc.reference(flipped, flags, wins, 2, 20, 0, 50, 16, (1, 5))
    for k in bc.INTEGERS:
        assert np.array_equal(a[0][k], b[0][k]), k
    assert lc.bits(a[0]["mean_r2"]).tolist() == lc.bits(b[0]["mean_r2"]).tolist()
    for k in bc.BIN_FIELDS:
        assert np.array_equal(a[1][k], b[1][k]), k
    for k in bc.SITE_FIELDS:
        if k != "carriers":  # the one column that names an allele
            assert np.array_equal(a[2][k], b[2][k]), k
    assert not np.array_equal(a[2]["carriers"], b[2]["carriers"])


def test_positions_change_bins_and_max_dist_membership():
    rng = np.random.default_rng(31400)
    n, W = 30, 400
    m01 = hc.founder_matrix(rng, n, W, nf=4, p_site=0.6, p_flip=2e-3)
    pos = np.cumsum(rng.integers(1, 40, size=W)).astype(np.uint64)
    plain = bc.reference(m01, None, [(0, W)], 2, 12, 60, 25, 8, (1, 5))
    spread = bc.reference(m01, None, [(0, W)], 2, 12, 60, 25, 8, (1, 5), pos=pos)
    assert spread[0]["n_pairs"][0] < plain[0]["n_pairs"][0] and not np.array_equal(spread[1]["pairs"], plain[1]["pairs"])
    assert np.array_equal(spread[2]["coord"], pos[bc.qualifying(m01, None, 2)])
