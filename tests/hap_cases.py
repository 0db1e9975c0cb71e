"""Shared by the haplotype-scan tests: matrices, window lists, the plain numpy reference and the comparison rules.

Reference: np.unique(m01[P][:, b:e], axis=0, return_inverse=True) gives the classes of a window, ordering them by
(-size, smallest member) the tables, and the formulas of include/impop_hip.h (impop_haplotype_scan) the doubles.  Integers and tables
must be equal; doubles within 1e-12 relative (few-flop epilogues)."""
import numpy as np

REL_TOL = 1e-12
DOUBLES = ("h1", "h12", "h2_h1", "hap_diversity")
INTEGERS = ("n_members", "n_distinct", "largest", "second", "n_singletons", "n_sites", "sum_sq")
MONO = (1000, 1100)  # founder_matrix keeps these sites monomorphic
TWIN_FROM = 1500     # ... and from here on the rows of twins() equal row 0


def twins(n):
    return sorted({0, n // 2, n - 1})


def founder_matrix(rng, n, S, nf=8, p_site=0.1, p_flip=2e-4):
    """nf founders that differ at about p_site of the sites (the others are monomorphic, all 0 or all 1), every haplotype a copy
    of one founder with sparse private flips: classes of size > 1, and few enough variable sites that the scan index is built"""
    anc = rng.integers(0, 2, size=S, dtype=np.uint8)
    f = np.repeat(anc[None, :], nf, axis=0)
    var = rng.random(S) < p_site
    f[:, var] = rng.integers(0, 2, size=(nf, int(var.sum())), dtype=np.uint8)
    m = f[rng.integers(0, nf, size=n)] ^ (rng.random((n, S), dtype=np.float32) < p_flip).astype(np.uint8)
    if S > MONO[1]:
        m[:, MONO[0]:MONO[1]] = anc[None, MONO[0]:MONO[1]]
    if S > TWIN_FROM:
        for r in twins(n):
            m[r, TWIN_FROM:] = m[0, TWIN_FROM:]
    return np.ascontiguousarray(m)


def window_list(S):
    """windows that start and end inside a 64-site block, a one-site window, an empty one, monomorphic sites only, the whole matrix,
    its last site, and two sliding lists whose windows overlap by half (the 10 kb / 5 kb shape)"""
    w = [(37, 517), (64, 128), (100, 101), (200, 200), MONO, (0, S), (S - 1, S), (TWIN_FROM + 3, S - 5), (63, 65), (0, 0), (S, S)]
    w += [(b, min(b + 640, S)) for b in range(0, S - 320, 320)]
    w += [(b, min(b + 500, S)) for b in range(13, S - 250, 250)]
    return [(int(b), int(e)) for b, e in w]


def reference(m01, flags, windows, weights=None):
    """-> (records as a dict of arrays, class_of [n_windows, |P|], sizes [n_windows, |P|])"""
    n = m01.shape[0]
    P = np.arange(n) if flags is None else np.flatnonzero(np.asarray(flags))
    nP = len(P)
    rows = m01[P]
    rec = {k: np.zeros(len(windows), dtype=np.float64 if k in DOUBLES else np.uint64) for k in INTEGERS + DOUBLES}
    class_of = np.zeros((len(windows), nP), dtype=np.uint32)
    sizes = np.zeros((len(windows), nP), dtype=np.uint32)
    for i, (b, e) in enumerate(windows):
        if e > b:
            _, inv = np.unique(rows[:, b:e], axis=0, return_inverse=True)
            inv = np.asarray(inv).ravel()
        else:
            inv = np.zeros(nP, dtype=np.int64)
        counts = np.bincount(inv)
        first = np.full(len(counts), nP, dtype=np.int64)
        np.minimum.at(first, inv, np.arange(nP))
        order = np.lexsort((first, -counts))  # by (-size, smallest member)
        rank = np.empty(len(counts), dtype=np.int64)
        rank[order] = np.arange(len(counts))
        class_of[i] = rank[inv]
        sz = counts[order]
        sizes[i, :len(sz)] = sz
        largest, second = int(sz[0]), int(sz[1]) if len(sz) > 1 else 0
        sum_sq = int((sz.astype(np.int64) ** 2).sum())
        nn = float(nP)
        h1 = float(sum_sq) / (nn * nn)
        rec["n_members"][i], rec["n_distinct"][i], rec["largest"][i], rec["second"][i] = nP, len(sz), largest, second
        rec["n_singletons"][i], rec["sum_sq"][i] = int((sz == 1).sum()), sum_sq
        rec["n_sites"][i] = (e - b) if weights is None else int(np.asarray(weights[b:e], dtype=np.int64).sum())
        rec["h1"][i] = h1
        rec["h12"][i] = h1 + 2.0 * (float(largest) / nn) * (float(second) / nn)
        rec["h2_h1"][i] = (h1 - (float(largest) / nn) * (float(largest) / nn)) / h1
        rec["hap_diversity"][i] = 0.0 if nP < 2 else (1.0 - h1) * nn / (nn - 1.0)
    return rec, class_of, sizes


def assert_matches(got, ref, where=""):
    """got = (records, class_of, sizes) of BitMatrix.haplotype_scan(want_members=True), ref = reference(...)"""
    rec, cl, sz = got
    want, wcl, wsz = ref
    assert len(rec) == len(wcl), where
    for k in INTEGERS:
        assert np.array_equal(rec[k].astype(np.uint64), want[k]), (where, k, rec[k][:8], want[k][:8])
    assert np.array_equal(cl, wcl), (where, "class_of")
    assert np.array_equal(sz, wsz), (where, "sizes")
    for k in DOUBLES:
        err = np.abs(rec[k] - want[k])
        assert (err <= REL_TOL * np.abs(want[k])).all(), (where, k, float(err.max()))
