"""Inputs of the upper-range tests (test_gpu_upper_range.py, test_gpu_upper_range_scans.py), importable without a GPU: wide
matrices whose rare entries name the haplotypes next to the 0xFFFF sentinel, K populations scattered over them, quartets whose
32-bit products come close to 2^30, populations at the LDS cap of the sfs table pass, and a small member set scattered over a
65535-row matrix.  tests/test_wide_cases_host.py keeps each of them from being hollow."""
import itertools

import numpy as np

# ---- the wide scan matrix of test_gpu_upper_range.py (moved here unchanged: the same seeds give the same matrices) --------------

SCAN_S = 64 * 40 + 13


def _special(n):
    return [0, 31, 32, n - 2, n - 1]


def _crafted_wide(n, seed):
    """0/1 [n, SCAN_S] like _crafted of test_gpu_scan_rare.py: a rare-only, a common-only and a monomorphic stretch, then a mix.
    Rare columns have 1 .. 4 carriers of either allele among haplotypes 0, 31, 32, n - 2, n - 1 (every subset, so n - 1 sits
    in every slot of an entry and alone in one; 4 carriers is a common site); every such column appears at least once."""
    rng = np.random.default_rng(seed)
    S = SCAN_S
    cols = []
    for k in (1, 2, 3, 4):
        for car in itertools.combinations(_special(n), k):
            for pol in (0, 1):
                c = np.zeros(n, np.uint8)
                c[list(car)] = 1
                cols.append(c ^ pol)
    cols = np.array(cols).T  # [n, 60]
    m = np.repeat((rng.random(S) < 0.5)[None, :].astype(np.uint8), n, axis=0)
    m[:, :cols.shape[1]] = cols

    def put_rare(lo, hi, p):
        idx = np.nonzero(rng.random(hi - lo) < p)[0] + lo
        m[:, idx] = cols[:, rng.integers(0, cols.shape[1], len(idx))]

    def put_common(lo, hi, p):
        idx = np.nonzero(rng.random(hi - lo) < p)[0] + lo
        m[:, idx] = (rng.random((n, len(idx)), dtype=np.float32) < 0.3).astype(np.uint8)

    put_rare(60, 400, 0.3)
    put_common(400, 800, 0.1)
    put_rare(1000, S, 0.08)
    put_common(1000, S, 0.04)
    for s in np.nonzero(rng.random(S - 1000) < 0.04)[0] + 1000:  # private sites of either polarity at random haplotypes
        m[:, s] = 0
        m[rng.integers(0, n), s] = 1
        if rng.random() < 0.5:
            m[:, s] ^= 1
    return m


def _scan_windows(S):
    w = [(0, 400, 0), (400, 800, 0), (800, 1000, 0), (0, S, S), (390, 410, 0), (999, 1001, 0), (5, 5, 0), (63, 65, 0), (S - 13, S, 0),
         (1800, S, 12345), (0, 60, 0), (0, 1, 7)]
    w += [(a, min(a + 150, S), 150) for a in range(1000, 1750, 150)]  # a tiling of the mixed stretch
    return w


# ---- shared ---------------------------------------------------------------------------------------------------------------------

WIDE_N = (8191, 16385, 65535)
INDEX_MAX_KEPT_INV = 4  # a matrix gets its variable-site index when at most 1/4 of its sites vary (internal.h)
RARE_WINDOW = (0, 400)  # the rare-only stretch of _crafted_wide and of wide_pop_case


def pop_counts(m, pops):
    """the populations' column sums [K][n_site], int64, without a whole-matrix cast (the counts= argument of plain_dstat / plain_sfs)"""
    return [m[np.asarray(list(p), dtype=np.int64)].sum(axis=0, dtype=np.int64) for p in pops]


def flags_of(members, n):
    f = np.zeros(n, np.uint8)
    f[np.asarray(list(members), dtype=np.int64)] = 1
    return f


def varying_fraction(m):
    c = m.sum(axis=0, dtype=np.int64)
    return float(((c > 0) & (c < m.shape[0])).mean())


def dstat_w_limit(n):
    """n = (n1, n2, n3, nO) -> the first W impop_dstat_scan refuses: the smallest W with n1 nO max(n2, n3)^2 W >= 2^62"""
    t = n[0] * n[3] * max(n[1], n[2]) ** 2
    return -(-(1 << 62) // t)


def sfs_w_limit(nk):
    """the first W impop_sfs_scan refuses for a population of nk haplotypes: the smallest W with nk^2 W >= 2^62"""
    return -(-(1 << 62) // (nk * nk))


# ---- K moderate populations scattered over a wide matrix --------------------------------------------------------------------------

POP_SIZES = (200, 317, 263, 151, 1, 229, 350, 181)  # all different; 200 and 350 even (an odd outgroup never ties); [4]: {n - 1}
WIDE_OUTGROUP = 0  # the even population the tests polarise by
PLANTED = 6        # sites of each planted kind


def wide_quartets(K):
    """more than IMPOP_DSTAT_GROUP quartets; the even population 0 is the outgroup of most, population 3 (odd) of one, and at
    K = 8 the one-haplotype population {n - 1} of two"""
    q = [(1, 2, 3, 0), (2, 1, 3, 0), (3, 1, 2, 0), (0, 1, 2, 3)]
    if K >= 8:
        q += [(5, 6, 7, 0), (6, 5, 7, 0), (1, 5, 2, 4), (7, 3, 6, 4), (2, 7, 5, 0), (1, 2, 3, 0)]
    return q


def wide_pairs(K):
    """all pairs of the K populations (more than IMPOP_SFS_PAIR_GROUP)"""
    return [(a, b) for a in range(K) for b in range(a + 1, K)]


def wide_pops(n, K, rng):
    """K disjoint populations of POP_SIZES[:K] members, scattered over 0 .. n - 1; haplotype 0 is in population 0, 31 in 1, 32 in
    2, n - 2 in 3, and n - 1 in 3 (K < 5) or alone in 4"""
    assert 4 <= K <= 8
    sp = _special(n)
    home = {sp[0]: 0, sp[1]: 1, sp[2]: 2, sp[3]: 3, sp[4]: 3 if K < 5 else 4}
    rest = rng.permutation(np.setdiff1d(np.arange(n), sp))
    pops, at = [], 0
    for k in range(K):
        mine = [h for h, p in home.items() if p == k]
        take = POP_SIZES[k] - len(mine)
        pops.append(sorted(mine + [int(x) for x in rest[at:at + take]]))
        at += take
    assert [len(p) for p in pops] == list(POP_SIZES[:K]) and len(set(len(p) for p in pops)) == K
    assert any(len(p) % 2 == 0 for p in pops) and (K < 5 or pops[4] == [n - 1])
    for p in pops[:4]:  # over the whole index range
        assert p[0] < n // 8 and p[-1] > n - n // 8
    return pops


def wide_pop_case(n, K, seed, carriers="pops"):
    """-> (m01 [n, SCAN_S], pops, windows).  The site mix of _crafted_wide (a rare-only, a common-only and a monomorphic stretch,
    then a mix; rare sites of both polarities), but the 1 .. 3 carriers of a rare site are drawn from the union of the
    populations (every subset of 1 .. 3 of the special haplotypes among them), so that the rare entries count for the populations.
    carriers="outside" draws them from the haplotypes in no population instead: the hollow case test_wide_cases_host.py must
    refuse.  In the mixed and the common stretch: PLANTED sites fixed in population 1 and absent in 2, PLANTED the other way
    round, and 2 PLANTED sites at which the even population 0 is split in half (outgroup ties).
    windows = _scan_windows without its seq_len column."""
    assert n in WIDE_N and carriers in ("pops", "outside")
    rng = np.random.default_rng(seed)
    S = SCAN_S
    pops = wide_pops(n, K, rng)
    union = np.array(sorted(h for p in pops for h in p), dtype=np.int64)
    src = union if carriers == "pops" else np.setdiff1d(np.arange(n), union)
    cols = []
    if carriers == "pops":
        for k in (1, 2, 3):
            for car in itertools.combinations(_special(n), k):
                for pol in (0, 1):
                    c = np.zeros(n, np.uint8)
                    c[list(car)] = 1
                    cols.append(c ^ pol)
    n_fixed = len(cols)
    for i in range(300):
        c = np.zeros(n, np.uint8)
        c[rng.choice(src, size=1 + i % 3, replace=False)] = 1
        cols.append(c ^ (i // 3 % 2))
    cols = np.array(cols).T
    m = np.repeat((rng.random(S) < 0.5)[None, :].astype(np.uint8), n, axis=0)
    m[:, :60] = cols[:, :60]

    def put_rare(lo, hi, p):
        idx = np.nonzero(rng.random(hi - lo) < p)[0] + lo
        m[:, idx] = cols[:, rng.integers(0, cols.shape[1], len(idx))]

    def put_common(lo, hi, p):
        idx = np.nonzero(rng.random(hi - lo) < p)[0] + lo
        m[:, idx] = (rng.random((n, len(idx)), dtype=np.float32) < 0.3).astype(np.uint8)

    put_rare(60, 400, 0.3)
    put_common(400, 800, 0.1)
    put_rare(1000, S, 0.08)
    put_common(1000, S, 0.04)
    for s in np.nonzero(rng.random(S - 1000) < 0.04)[0] + 1000:  # private sites of either polarity
        m[:, s] = 0
        m[rng.choice(src), s] = 1
        if rng.random() < 0.5:
            m[:, s] ^= 1
    # common sites inside the short windows (390, 410) and (S - 13, S), which would otherwise often hold none
    for s in (403, 406, S - 9, S - 4):
        m[:, s] = (rng.random(n, dtype=np.float32) < 0.3).astype(np.uint8)
    # plants: on a common background, so every population segregates around them
    p0, p1, p2 = (np.asarray(pops[k], dtype=np.int64) for k in (0, 1, 2))
    sites = np.concatenate([rng.choice(np.arange(410, 790), size=PLANTED, replace=False),
                            rng.choice(np.arange(1010, S - 20), size=3 * PLANTED, replace=False)])
    for i, s in enumerate(int(x) for x in sites):
        m[:, s] = (rng.random(n, dtype=np.float32) < 0.3).astype(np.uint8)
        kind = i % 4
        if kind == 0:
            m[p1, s], m[p2, s], m[p0, s] = 1, 0, 0
        elif kind == 1:
            m[p1, s], m[p2, s], m[p0, s] = 0, 1, 0
        else:  # a tie in population 0: one half carries 1
            m[p0, s] = 0
            m[rng.choice(p0, size=len(p0) // 2, replace=False), s] = 1
    if carriers == "pops":
        assert n_fixed == 50
    assert INDEX_MAX_KEPT_INV * varying_fraction(m) <= 1.0
    return m, pops, [(a, b) for a, b, _ in _scan_windows(S)]


# ---- quartets whose 32-bit products come close to 2^30 ----------------------------------------------------------------------------

EXTREME_QUARTETS = [(0, 1, 2, 3), (1, 0, 2, 3), (2, 0, 1, 3)]  # (A, B, C, O), (B, A, C, O), (C, A, B, O)
EXTREME_S = 400
PRODUCT_FLOOR = 1 << 29


def extreme_products(counts, sizes, quartets):
    """per site and quartet the 32-bit quantities of dstat_site (unpolarised), as int64 arrays [n_quartets, n_site] by name"""
    out = {k: [] for k in ("c1n2", "c2n1", "r1c2", "c2n3", "c3n2", "x", "donor_p2", "fixed12")}
    for q in quartets:
        (c1, c2, c3, _), (n1, n2, n3, _) = [np.asarray(counts[k], dtype=np.int64) for k in q], [sizes[k] for k in q]
        out["c1n2"].append(c1 * n2)
        out["c2n1"].append(c2 * n1)
        out["r1c2"].append((n1 - c1) * c2)
        out["c2n3"].append(c2 * n3)
        out["c3n2"].append(c3 * n2)
        out["x"].append(c1 * n2 - c2 * n1)
        out["donor_p2"].append((c2 * n3 >= c3 * n2).astype(np.int64))
        out["fixed12"].append((((c1 == n1) & (c2 == 0)) | ((c1 == 0) & (c2 == n2))).astype(np.int64))
    return {k: np.array(v) for k, v in out.items()}


def extreme_quartet_case(n=65535):
    """-> (m01 [n, EXTREME_S], pops [A, B, C, O], EXTREME_QUARTETS, windows).  A = the even and B = the odd haplotypes below
    n - 3 (32766 each at n = 65535: n_A n_B = 2^30 - 131068, the largest product of two sizes a quartet can have), C = {n - 3, n - 2},
    O = {n - 1}.  A quarter of the sites vary (the matrix gets its index): every combination of c_A, c_B in {0, 1, half, n - 1, n},
    with c_C and c_O going through their six combinations, then random counts.  The carriers are random members."""
    rng = np.random.default_rng(77000 + n)
    half = (n - 3) // 2
    A, B = list(range(0, 2 * half, 2)), list(range(1, 2 * half, 2))
    pops = [A, B, [n - 3, n - 2], [n - 1]]
    sizes = [len(p) for p in pops]
    levels = (0, 1, half // 2 + 1, half - 1, half)
    want = []
    for rep in (0, 1):
        for i, (ca, cb) in enumerate(itertools.product(levels, levels)):
            k = (i + 3 * rep) % 6
            want.append((ca, cb, k % 3, k // 3))
    for _ in range(EXTREME_S // INDEX_MAX_KEPT_INV - len(want)):
        want.append((int(rng.integers(0, half + 1)), int(rng.integers(0, half + 1)), int(rng.integers(0, 3)), int(rng.integers(0, 2))))
    assert len(want) == EXTREME_S // INDEX_MAX_KEPT_INV
    m = np.repeat((rng.random(EXTREME_S) < 0.5)[None, :].astype(np.uint8), n, axis=0)
    where = np.sort(rng.choice(EXTREME_S, size=len(want), replace=False))
    for s, cs in zip((int(x) for x in where), want):
        m[:, s] = 0
        for p, c in zip(pops, cs):
            m[rng.choice(np.asarray(p), size=c, replace=False), s] = 1
    counts = pop_counts(m, pops)
    pr = extreme_products(counts, sizes, EXTREME_QUARTETS)
    for k in ("c1n2", "c2n1", "r1c2", "c2n3", "c3n2"):
        assert PRODUCT_FLOOR < pr[k].max() < 2 * PRODUCT_FLOOR, (k, int(pr[k].max()))
    assert pr["x"].max() > PRODUCT_FLOOR and pr["x"].min() < -PRODUCT_FLOOR
    for q in range(len(EXTREME_QUARTETS)):
        assert 0 < pr["donor_p2"][q].sum() < EXTREME_S
    assert pr["fixed12"][0].sum() >= 2
    for q in EXTREME_QUARTETS:  # the bound admits windows far longer than the matrix
        assert dstat_w_limit([sizes[k] for k in q]) > 100 * EXTREME_S
    assert INDEX_MAX_KEPT_INV * varying_fraction(m) <= 1.0
    return m, pops, EXTREME_QUARTETS, [(0, EXTREME_S), (3, 201), (199, 397), (64, 128)]


# ---- populations at the LDS cap of the sfs table pass -----------------------------------------------------------------------------

SFS_LDS_BYTES = 160 * 1024  # sfs.hip: a workgroup's LDS


def sfs_lds_bins(kj, n_hap):
    """sfs_lds_bins of sfs.hip restated: the bins a table job's histogram may have next to its kj masks in LDS, a mask being the
    matrix's dword columns padded to whole granules of four: (SFS_LDS_BYTES - kj * wps4 * 4) / 4"""
    wps = (n_hap + 31) // 32
    wps4 = (wps + 3) // 4 * 4
    return (SFS_LDS_BYTES - kj * wps4 * 4) // 4


BIG_SFS_S = 400
BIG_SFS_PAIRS = [(3, 4), (3, 5), (4, 5), (1, 5), (5, 2)]  # disjoint populations only
BIG_SFS_WINDOWS = [(0, BIG_SFS_S), (0, 200), (137, 333), (64, 128)]


def big_sfs_case(n=65535):
    """-> (m01 [n, BIG_SFS_S], pops [ALL, BIG, BIG1, a, b, o], BIG_SFS_PAIRS, BIG_SFS_WINDOWS).  BIG has one haplotype fewer than
    a one-population table job has bins in LDS (its spectrum of n + 1 bins fills the cap exactly), BIG1 = BIG and one more (one
    bin over); a, b small and disjoint from each other and from BIG1; o = {n - 1}.  A quarter of the sites vary: singletons (ALL
    has c = 1) and their mirror images (c = n - 1) at haplotypes that include 0, 31, 32, n - 2 and n - 1, sites near c = n / 2,
    and sites of other frequencies."""
    rng = np.random.default_rng(88000 + n)
    cap = sfs_lds_bins(1, n)
    n_big = cap - 1
    assert n_big + 40 + 57 + 2 <= n
    order = rng.permutation(n - 1)  # n - 1 is the outgroup's
    big = sorted(int(x) for x in order[:n_big])
    big1 = sorted(int(x) for x in order[:n_big + 1])
    a = sorted(int(x) for x in order[n_big + 1:n_big + 41])
    b = sorted(int(x) for x in order[n_big + 41:n_big + 98])
    pops = [list(range(n)), big, big1, a, b, [n - 1]]
    assert len(big) + 1 == cap and len(big1) == cap and set(big) < set(big1)
    m = np.repeat((rng.random(BIG_SFS_S) < 0.5)[None, :].astype(np.uint8), n, axis=0)
    where = np.sort(rng.choice(BIG_SFS_S, size=BIG_SFS_S // INDEX_MAX_KEPT_INV, replace=False))
    lone = _special(n) + a[:3] + b[:3] + [int(x) for x in rng.integers(0, n, 9)]
    for i, s in enumerate(int(x) for x in where):
        if i < 2 * len(lone):  # one carrier of 1, then one carrier of 0
            m[:, s] = i % 2
            m[lone[i // 2], s] = 1 - i % 2
        elif i < 2 * len(lone) + 10:
            c = n // 2 + (i % 5) - 2
            m[:, s] = 0
            m[rng.choice(n, size=c, replace=False), s] = 1
        else:
            m[:, s] = (rng.random(n, dtype=np.float32) < rng.choice([0.01, 0.1, 0.3, 0.7, 0.95])).astype(np.uint8)
    # a and b: fixed differences at two of the random sites each way
    for i, s in enumerate(int(x) for x in where[-4:]):
        m[a, s], m[b, s] = i % 2, 1 - i % 2
    assert INDEX_MAX_KEPT_INV * varying_fraction(m) <= 1.0
    return m, pops, BIG_SFS_PAIRS, BIG_SFS_WINDOWS


def joint_cap_pops(n, rng):
    """-> (pops [p127, q315, q316], at-cap pair (0, 1), over-cap pair (0, 2)) for a two-population joint job (kj = 2, no outgroup)
    on an n-haplotype matrix: (|p| + 1) (|q315| + 1) is exactly sfs_lds_bins(2, n), one more member in q is over it"""
    cap = sfs_lds_bins(2, n)
    na1 = 128
    assert cap % na1 == 0
    nb1 = cap // na1
    order = rng.permutation(n)
    p = sorted(int(x) for x in order[:na1 - 1])
    q = [int(x) for x in order[na1 - 1:na1 - 1 + nb1]]
    pops = [p, sorted(q[:-1]), sorted(q)]
    assert (len(pops[0]) + 1) * (len(pops[1]) + 1) == cap and (len(pops[0]) + 1) * (len(pops[2]) + 1) > cap
    return pops, (0, 1), (0, 2)


# ---- a member set scattered over a wide matrix ---------------------------------------------------------------------------------------

N_DECOYS = 6
RUN = 40  # consecutive member rows that cross a multiple of 32


def scatter_positions(nm, n_wide, rng):
    """nm ascending row numbers in 0 .. n_wide - 1: 0, 31, 32, n_wide - 2, n_wide - 1, a run of RUN consecutive rows that crosses
    a multiple of 32, the rest random"""
    assert nm >= RUN + 8 and n_wide >= 64 * nm
    start = 32 * int(rng.integers(4, n_wide // 32 - 4)) - 13
    fixed = set(_special(n_wide)) | set(range(start, start + RUN))
    rest = rng.permutation(np.setdiff1d(np.arange(n_wide), np.array(sorted(fixed))))[:nm - len(fixed)]
    pos = np.array(sorted(fixed | set(int(x) for x in rest)), dtype=np.int64)
    assert len(pos) == nm and (start // 32) != ((start + RUN - 1) // 32)
    per_column = np.bincount(pos // 32, minlength=(n_wide + 31) // 32)
    assert (per_column == 1).sum() >= 10 and (per_column == 0).sum() > 0  # dword columns with exactly one member, and skipped ones
    return pos


def scatter(member_matrix, n_wide, seed):
    """-> (wide [n_wide, S], members ascending): wide[members[i]] is member_matrix[i] (plus the private variants below), every
    other row a copy of one of N_DECOYS decoy haplotypes.  A decoy is random at the sites that vary among the members and the
    complement of the members at some of the sites where they agree, so it differs from every member at many sites and a kernel
    that reads a wrong row cannot agree by accident.  On member-monomorphic sites further rare variants are planted: carried by
    1 .. 3 decoy rows only, and by one member together with 1 .. 2 decoy rows; half of these sites are stored with 1 as the
    major allele (all rows complemented where the members carried 0), so their entries list the carriers of allele 0.  At most a quarter of all sites vary among all rows (asserted), so the wide matrix gets its
    variable-site index and its rare split."""
    mm = np.ascontiguousarray(member_matrix, dtype=np.uint8)
    nm, S = mm.shape
    rng = np.random.default_rng(seed)
    pos = scatter_positions(nm, n_wide, rng)
    c = mm.sum(axis=0, dtype=np.int64)
    var = (c > 0) & (c < nm)
    mono = np.flatnonzero(~var)
    budget = S // INDEX_MAX_KEPT_INV - int(var.sum())
    assert budget >= 30, ("the members vary at too many sites to leave room for decoy sites", int(var.sum()), S)
    extra = rng.choice(mono, size=budget, replace=False)
    n_diff = budget // 3
    diff_sites, rare_sites = extra[:n_diff], extra[n_diff:]
    decoys = np.repeat(mm[:1], N_DECOYS, axis=0)
    decoys[:, var] = rng.integers(0, 2, size=(N_DECOYS, int(var.sum())), dtype=np.uint8)
    for s in diff_sites:  # some decoys carry the allele no member has (never none and never all: rows outside the members differ)
        k = rng.permutation(N_DECOYS)[:int(rng.integers(1, N_DECOYS))]
        decoys[k, s] ^= 1
    owner = rng.integers(0, N_DECOYS, size=n_wide)
    wide = decoys[owner]
    wide[pos] = mm
    is_decoy = np.ones(n_wide, bool)
    is_decoy[pos] = False
    decoy_rows = np.flatnonzero(is_decoy)
    mixed = zeros_listed = 0
    for i, s in enumerate(int(x) for x in rare_sites):
        k = 1 + i % 3
        if i % 2:  # one member among the carriers
            wide[pos[int(rng.integers(0, nm))], s] ^= 1
            k = max(k - 1, 1)
            mixed += 1
        wide[rng.choice(decoy_rows, size=k, replace=False), s] ^= 1
        if i // 2 % 2 and mm[0, s] == 0:  # the whole site in the other polarity: the same differences between any two rows
            wide[:, s] ^= 1
        zeros_listed += int(wide[:, s].sum(dtype=np.int64)) > n_wide // 2
    dist = (decoys[:, None, :] != wide[pos][None, :, :]).sum(axis=2)
    assert dist.min() >= 20, int(dist.min())
    assert mixed >= 5 and zeros_listed >= 3 and len(rare_sites) - zeros_listed >= 3, (mixed, zeros_listed)
    assert INDEX_MAX_KEPT_INV * varying_fraction(wide) <= 1.0
    return wide, pos
