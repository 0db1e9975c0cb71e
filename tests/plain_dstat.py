"""A plain restatement of impop_dstat_scan's definitions (include/impop_hip.h) from a hap-major 0/1 array: a loop over sites with
Python integers, the doubles formed by the expressions in the record's comments.  It uses no code of the library, so that the
device's integers and the host's doubles can be compared with it bit for bit."""
import numpy as np

STATS_DTYPE = np.dtype([("n_sites", "<u4"), ("n_informative", "<u4"), ("n_skipped", "<u4"), ("flags", "<u4"), ("abba", "<i8"), ("baba", "<i8"),
                        ("f4_num", "<i8"), ("fd_den_p2", "<i8"), ("fd_den_p3", "<i8"), ("d", "<f8"), ("f4", "<f8"), ("fd", "<f8")])
INT_FIELDS = [n for n in STATS_DTYPE.names if STATS_DTYPE[n].kind != "f"]
NAN = float("nan")


def site_terms(c, n, polarize):
    """(abba, baba, f4, fd_p2, fd_p3, skipped) of one site, unweighted: c = (c1, c2, c3, cO), n = (n1, n2, n3, nO)"""
    c1, c2, c3, cO = c
    n1, n2, n3, nO = n
    if polarize:
        if 2 * cO == nO:
            return 0, 0, 0, 0, 0, 1
        if 2 * cO > nO:
            c1, c2, c3, cO = n1 - c1, n2 - c2, n3 - c3, nO - cO
    abba = (n1 - c1) * c2 * c3 * (nO - cO)
    baba = c1 * (n2 - c2) * c3 * (nO - cO)
    f4 = (c1 * n2 - c2 * n1) * (c3 * nO - cO * n3)
    if c2 * n3 >= c3 * n2:
        return abba, baba, f4, (c2 * n1 - c1 * n2) * c2 * (nO - cO), 0, 0
    return abba, baba, f4, 0, (c3 * n1 - c1 * n3) * c3 * (nO - cO), 0


def doubles(abba, baba, f4_num, fd_den_p2, fd_den_p3, n):
    """d, f4, fd in the header's operation order"""
    n1, n2, n3, nO = n
    d = float(abba - baba) / float(abba + baba) if abba + baba else NAN
    f4 = float(f4_num) / float(n1 * n2 * n3 * nO)
    den = float(fd_den_p2) / float(n1 * n2 * n2 * nO) + float(fd_den_p3) / float(n1 * n3 * n3 * nO)
    fd = (float(abba - baba) / float(n1 * n2 * n3 * nO)) / den if den != 0.0 else NAN
    return d, f4, fd


def reference(m01, pops, quartets, windows, polarize=False, weights=None, counts=None):
    """-> records [n_windows, n_quartets]; pops = lists of haplotype indices, quartets = rows (P1, P2, P3, O) of indices into pops,
    windows = (site_begin, site_end) rows, weights = one integer per site or None.  counts = the populations' column sums
    [K][n_site] where the caller has them already (a wide matrix is then not cast to int64 as a whole; m01 is not read)"""
    if counts is None:
        m = np.asarray(m01).astype(np.int64)
        counts = [m[list(p)].sum(axis=0) for p in pops]
    counts = [[int(x) for x in c] for c in counts]  # per population, per site
    n_site = len(counts[0])
    sizes = [len(p) for p in pops]
    wt = [1] * n_site if weights is None else [int(x) for x in weights]
    out = np.zeros((len(windows), len(quartets)), dtype=STATS_DTYPE)
    for qi, q in enumerate(quartets):
        q = [int(x) for x in q]
        n = tuple(sizes[k] for k in q)
        terms = [site_terms(tuple(counts[k][s] for k in q), n, polarize) for s in range(n_site)]
        for wi, w in enumerate(windows):
            b, e = int(w[0]), int(w[1])
            tot = [0, 0, 0, 0, 0]
            inf = skip = W = 0
            for s in range(b, e):
                t = terms[s]
                for f in range(5):
                    tot[f] += wt[s] * t[f]
                inf += t[0] + t[1] > 0
                skip += t[5]
                W += wt[s]
            out[wi, qi] = (W, inf, skip, 0) + tuple(tot) + doubles(*tot, n)
    return out


def bits_equal(a, b):
    """element-wise: the same bits, or NaN against NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def assert_matches(got, want, tag="", skip=()):
    """every integer equal, every double equal bit for bit (NaN matches NaN)"""
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    for name in STATS_DTYPE.names:
        if name in skip:
            continue
        a, b = np.asarray(got[name]), np.asarray(want[name])
        same = bits_equal(a, b) if STATS_DTYPE[name].kind == "f" else a == b
        assert same.all(), (tag, name, np.argwhere(~same)[:4].tolist(), a[~same][:4], b[~same][:4])
