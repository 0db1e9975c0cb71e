"""Inputs of the impop_dstat_scan tests: the header's known answer, the geometry generator, a crafted matrix with rare-only,
common-only, monomorphic and mixed stretches, population cuts and quartet lists."""
import numpy as np

# the header's case: P1 = {0,1}, P2 = {2,3}, P3 = {4,5}, O = {6,7}; the carriers of a population are its lowest-numbered haplotypes
KNOWN_COUNTS = [(0, 2, 2, 0), (2, 0, 2, 0), (1, 2, 1, 0), (0, 1, 2, 0), (1, 1, 0, 0), (2, 2, 2, 2)]
KNOWN_POPS = [[0, 1], [2, 3], [4, 5], [6, 7]]
KNOWN_QUARTETS = [(0, 1, 2, 3), (1, 0, 2, 3)]
KNOWN_INTS = {  # quartet -> abba, baba, f4_num, fd_den_p2, fd_den_p3, n_informative, n_skipped
    (0, 1, 2, 3): (28, 16, -12, 24, 16, 4, 0),
    (1, 0, 2, 3): (16, 28, 12, 12, 8, 4, 0),
}
KNOWN_DOUBLES = {(0, 1, 2, 3): (12.0 / 44.0, -0.75, 0.3), (1, 0, 2, 3): (-12.0 / 44.0, 0.75, -0.6)}

GEOMETRY_N = (8, 33, 64, 65, 70, 130, 465)
GEOMETRY_SITES = 2100
GEOMETRY_QUARTETS = [(0, 1, 2, 3), (1, 0, 2, 3), (2, 3, 0, 1)]
GEOMETRY_WINDOWS = [(0, 64), (1, 65), (63, 129), (0, 2100), (700, 1400), (2036, 2100), (5, 6)]


def known_matrix():
    m = np.zeros((8, len(KNOWN_COUNTS)), dtype=np.uint8)
    for s, counts in enumerate(KNOWN_COUNTS):
        for k, c in enumerate(counts):
            m[2 * k:2 * k + c, s] = 1
    return m


def draw_sites(rng, n, n_site):
    """half monomorphic in either allele, one fifth with 1..3 carriers of either polarity, the rest Bernoulli(f), f uniform per site"""
    m = np.zeros((n, n_site), dtype=np.uint8)
    kind = rng.random(n_site)
    for s in range(n_site):
        if kind[s] < 0.5:
            m[:, s] = rng.integers(0, 2)
        elif kind[s] < 0.7:
            k = int(rng.integers(1, 4))
            col = np.zeros(n, dtype=np.uint8)
            col[rng.choice(n, size=min(k, n), replace=False)] = 1
            m[:, s] = col if rng.integers(0, 2) else 1 - col
        else:
            m[:, s] = rng.random(n) < rng.random()
    return m


def cut_pops(rng, n):
    """four disjoint populations of unequal sizes from a permutation: n//5, n//4, n//3 and the rest but one haplotype"""
    perm = [int(x) for x in rng.permutation(n)]
    a, b, c = n // 5, n // 4, n // 3
    return [sorted(perm[:a]), sorted(perm[a:a + b]), sorted(perm[a + b:a + b + c]), sorted(perm[a + b + c:n - 1])]


def geometry_case(n):
    rng = np.random.default_rng(9000 + n)
    return draw_sites(rng, n, GEOMETRY_SITES), cut_pops(rng, n)


def crafted(n, seed=3):
    """stretches of 1000 sites on a monomorphic background of either allele (three quarters of all sites stay monomorphic, so the
    matrix gets its variable-site index): rare only, common only, monomorphic, mixed, rare with the 0-allele listed, common only"""
    rng = np.random.default_rng(seed + n)
    L, kinds = 1000, ("rare", "common", "mono", "mixed", "rare0", "common")
    S = L * len(kinds)
    m = np.repeat((rng.random(S) < 0.5)[None, :].astype(np.uint8), n, axis=0)

    def put_rare(lo, p, flip):
        for s in np.nonzero(rng.random(L) < p)[0] + lo:
            col = np.zeros(n, dtype=np.uint8)
            col[rng.choice(n, size=int(rng.integers(1, 4)), replace=False)] = 1
            m[:, s] = 1 - col if flip else col

    def put_common(lo, p):
        idx = np.nonzero(rng.random(L) < p)[0] + lo
        m[:, idx] = (rng.random((n, len(idx))) < rng.uniform(0.15, 0.85, size=len(idx))).astype(np.uint8)

    for k, kind in enumerate(kinds):
        if kind in ("rare", "rare0"):
            put_rare(k * L, 0.25, kind == "rare0")
        elif kind == "common":
            put_common(k * L, 0.2)
        elif kind == "mixed":
            put_rare(k * L, 0.1, False)
            put_rare(k * L, 0.05, True)
            put_common(k * L, 0.1)
    # windows that start and end inside each stretch, and some across stretches
    wins = [(k * L + 37, k * L + 901) for k in range(len(kinds))] + [(0, S), (750, 2250), (1990, 4010), (3999, 5001), (1433, 1434)]
    return m, wins


def six_pops(rng, n):
    """six disjoint populations (one haplotype left out) and 15 quartets over them: a repeated quartet, two that share three"""
    perm = [int(x) for x in rng.permutation(n)]
    cuts = np.linspace(0, n - 1, 7).astype(int)
    pops = [sorted(perm[cuts[i]:cuts[i + 1]]) for i in range(6)]
    quartets = [(0, 1, 2, 3), (0, 1, 2, 4), (0, 1, 2, 3), (1, 0, 2, 5), (2, 3, 4, 5), (5, 4, 3, 2), (0, 2, 4, 5), (1, 3, 5, 0),
                (3, 1, 0, 2), (4, 5, 0, 1), (2, 0, 1, 5), (3, 4, 5, 0), (1, 2, 3, 4), (5, 0, 3, 1), (4, 2, 1, 3)]
    return pops, quartets


def assert_not_hollow(ref):
    """at least two thirds of the records informative, both signs of abba - baba"""
    inf = (ref["abba"] + ref["baba"]) > 0
    diff = ref["abba"] - ref["baba"]
    assert 3 * int(inf.sum()) >= 2 * inf.size, (int(inf.sum()), inf.size)
    assert (diff > 0).any() and (diff < 0).any()
