"""CPU only: the inputs of tests/wide_cases.py are not hollow.  For every case the plain restatement (plain_dstat / plain_sfs) is
computed and asked for what the GPU tests of test_gpu_upper_range_scans.py rely on: informative records, both signs, outgroup
ties, every pair class, the products next to 2^30, the largest c^2, and in Python integers the largest weight sum each
call's overflow rule admits and the first it refuses."""
import numpy as np
import pytest

import dstat_cases as dc
import plain_dstat as pd
import plain_sfs as ps
import sfs_cases as sc
import wide_cases as wc

CASES = [(n, 4) for n in wc.WIDE_N] + [(65535, 8)]
OG = wc.WIDE_OUTGROUP


def rare_window_informative(ref, windows):
    """at least two thirds of the records of the rare-only window carry an ABBA or a BABA site"""
    row = ref[windows.index(wc.RARE_WINDOW)]
    inf = (row["abba"] + row["baba"]) > 0
    assert 3 * int(inf.sum()) >= 2 * inf.size, (int(inf.sum()), inf.size)


def several_members(ref, pops, outgroup):
    """an sfs reference without the one-haplotype populations (0 < c < 1 never holds: they cannot segregate), the outgroup's
    index moved along; their pairs go with them"""
    keep = [k for k, p in enumerate(pops) if len(p) > 1]
    return keep, (None if outgroup is None else keep.index(outgroup))


@pytest.mark.parametrize("n,K", CASES)
def test_wide_pop_case_dstat(n, K):
    m, pops, wins = wc.wide_pop_case(n, K, n + K)
    counts = wc.pop_counts(m, pops)
    quartets = wc.wide_quartets(K)
    assert len(quartets) > 3  # IMPOP_DSTAT_GROUP
    skipped = 0
    for polarize in (False, True):
        ref = pd.reference(None, pops, quartets, wins, polarize, counts=counts)
        dc.assert_not_hollow(ref)
        rare_window_informative(ref, wins)
        skipped += int(ref["n_skipped"].max()) if polarize else 0
        assert polarize or not ref["n_skipped"].any()
    assert skipped > 0
    # the members the tests are about: every special haplotype in some population, {n - 1} alone at K >= 5
    union = set(h for p in pops for h in p)
    assert set(wc._special(n)) <= union and (K < 5 or pops[4] == [n - 1])
    # admission: the largest W the rule admits and the first it refuses, far beyond this matrix
    for q in quartets:
        nq = [len(pops[k]) for k in q]
        t = nq[0] * nq[3] * max(nq[1], nq[2]) ** 2
        W = wc.dstat_w_limit(nq)
        assert t * (W - 1) < 2 ** 62 <= t * W and W - 1 > m.shape[1]


def test_carriers_outside_the_populations_are_hollow():
    """what the case guards against: rare sites whose carriers are in no population leave the rare-only window without a site"""
    n, K = 8191, 4
    m, pops, wins = wc.wide_pop_case(n, K, n + K, carriers="outside")
    ref = pd.reference(None, pops, wc.wide_quartets(K), wins, False, counts=wc.pop_counts(m, pops))
    with pytest.raises(AssertionError):
        rare_window_informative(ref, wins)
    st = ps.reference(None, pops, [], [wc.RARE_WINDOW], None, counts=wc.pop_counts(m, pops))[0]
    assert not st["seg"].any()


@pytest.mark.parametrize("n,K", CASES)
def test_wide_pop_case_sfs(n, K):
    m, pops, wins = wc.wide_pop_case(n, K, n + K)
    counts = wc.pop_counts(m, pops)
    pairs = wc.wide_pairs(K)
    assert len(pairs) > 4 and len(pops[OG]) % 2 == 0  # IMPOP_SFS_PAIR_GROUP; an even outgroup
    for og in (None, OG):
        ref = ps.reference(None, pops, pairs, wins, og, counts=counts)
        keep, og_kept = several_members(ref, pops, og)
        kp = [i for i, (a, b) in enumerate(pairs) if a in keep and b in keep]
        sub = (ref[0][:, keep], ref[1][:, kp], None, [ref[3][i] for i in kp])
        sc.assert_not_hollow(sub, og_kept, sum(ps.polarized_counts(None, pops, og, counts)[2]))
        for f in sc.PAIR_FIELDS[:5]:
            assert ref[1][f].max() > 0, f
        if og is not None:
            assert ref[0]["n_skipped"].max() > 0
        st = ref[0][wins.index(wc.RARE_WINDOW)]
        assert (st["seg"][[k for k in keep if k != og]] >= 2).all()  # the rare entries count for every population
    for p in pops:
        W = wc.sfs_w_limit(len(p))
        assert len(p) ** 2 * (W - 1) < 2 ** 62 <= len(p) ** 2 * W and W - 1 > m.shape[1]


def test_extreme_quartet_case():
    m, pops, quartets, wins = wc.extreme_quartet_case()
    sizes = [len(p) for p in pops]
    assert sizes == [32766, 32766, 2, 1] and not set(pops[0]) & set(pops[1])
    counts = wc.pop_counts(m, pops)
    pr = wc.extreme_products(counts, sizes, quartets)
    for k in ("c1n2", "c2n1", "r1c2", "c2n3", "c3n2"):
        assert 2 ** 29 < pr[k].max() < 2 ** 30, k
    assert pr["x"].max() > 2 ** 29 and pr["x"].min() < -2 ** 29
    assert all(0 < pr["donor_p2"][q].sum() < m.shape[1] for q in range(len(quartets)))
    assert pr["fixed12"][0].sum() >= 2
    for polarize in (False, True):
        ref = pd.reference(None, pops, quartets, wins, polarize, counts=counts)
        dc.assert_not_hollow(ref)
        assert (ref["fd_den_p2"] != 0).any() and (ref["fd_den_p3"] != 0).any()
        assert np.abs(ref["f4_num"]).max() > 2 ** 31 and ref["abba"].max() > 2 ** 31  # beyond what 32 bits hold
    for q in quartets:
        nq = [sizes[k] for k in q]
        W = wc.dstat_w_limit(nq)
        assert nq[0] * nq[3] * max(nq[1], nq[2]) ** 2 * (W - 1) < 2 ** 62 and W > 100 * m.shape[1]


def test_big_sfs_case():
    n = 65535
    m, pops, pairs, wins = wc.big_sfs_case(n)
    cap = wc.sfs_lds_bins(1, n)
    assert [len(p) for p in pops[:3]] == [n, cap - 1, cap] and cap == (163840 - 8192) // 4
    assert len(pops[0]) + 1 > cap  # ALL: 65536 bins, never in LDS
    for a, b in pairs:
        assert not set(pops[a]) & set(pops[b]), (a, b)
    counts = wc.pop_counts(m, pops)
    for og in (None, 5):
        ref = ps.reference(None, pops, pairs, wins, og, counts=counts)
        st = ref[0]
        assert (st["seg"][0, :5] >= 2).all()
        for f in sc.PAIR_FIELDS[:5]:
            assert ref[1][f].max() > 0, (og, f)
        assert st["eta1"][0, 0] > 0 and st["eta_n1"][0, 0] > 0  # both hot bins of the widest spectrum
        assert ref[2][0][0, 1] > 0 and ref[2][0][0, n - 1] > 0 and ref[2][0][0, n // 2 - 2:n // 2 + 3].sum() > 0
    c_all = counts[0]
    assert int(c_all[c_all < n].max()) == n - 1 and int((c_all[(c_all > 0) & (c_all < n)] ** 2).max()) == 65534 ** 2 < 2 ** 32
    assert (c_all == 1).any()
    W = wc.sfs_w_limit(n)
    assert n * n * (W - 1) < 2 ** 62 <= n * n * W


def test_joint_cap_pops():
    pops, at, over = wc.joint_cap_pops(8191, np.random.default_rng(5))
    assert [len(p) for p in pops] == [127, 315, 316]
    assert 128 * 316 == wc.sfs_lds_bins(2, 8191) == (163840 - 2048) // 4
    assert not set(pops[0]) & set(pops[2])


@pytest.mark.parametrize("nm", (130, 465))
def test_scatter(nm):
    import hap_cases as hc
    n_wide = 65535
    mm = hc.founder_matrix(np.random.default_rng(nm), nm, 1200, p_site=0.08, p_flip=1e-4)
    wide, pos = wc.scatter(mm, n_wide, 31 + nm)
    assert wide.shape == (n_wide, 1200) and (np.diff(pos) > 0).all() and set(wc._special(n_wide)) <= set(pos.tolist())
    changed = (wide[pos] != mm).any(axis=0)
    assert 0 < changed.sum() <= 1200 // 4 and not changed[mm.min(axis=0) != mm.max(axis=0)].any()  # planted on member-monomorphic sites only
    rows = np.ones(n_wide, bool)
    rows[pos] = False
    packed = np.ascontiguousarray(np.packbits(wide[rows], axis=1))
    assert len(np.unique(packed.view([("", packed.dtype)] * packed.shape[1]))) > wc.N_DECOYS  # decoy rows with private variants
    # rare entries that list one member alongside non-members, and entries that list the carriers of allele 0
    c = wide.sum(axis=0, dtype=np.int64)
    minor = np.minimum(c, n_wide - c)
    rare = np.flatnonzero((minor >= 1) & (minor <= 3))
    mixed = zeros = 0
    for s in rare:
        carriers = np.flatnonzero(wide[:, s] == (1 if c[s] <= 3 else 0))
        in_m = np.isin(carriers, pos).sum()
        mixed += 0 < in_m < len(carriers)
        zeros += c[s] > 3
    assert mixed >= 5 and zeros >= 3
