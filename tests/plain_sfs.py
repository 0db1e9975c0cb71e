"""A plain restatement of impop_sfs_scan's definitions (include/impop_hip.h) from a hap-major 0/1 array: a loop over sites with
Python integers, the doubles formed by the expressions in the header's comment, in its operator order.  It uses no code of the
library, so that the device's integers, the tables and the host's doubles can be compared with it bit for bit."""
import math

import numpy as np

STATS_DTYPE = np.dtype([("n_sites", "<u4"), ("seg", "<u4"), ("eta1", "<u4"), ("eta_n1", "<u4"), ("n_skipped", "<u4"), ("flags", "<u4"),
                        ("sum_het", "<u8"), ("sum_c", "<u8"), ("sum_c2", "<u8"), ("theta_w", "<f8"), ("theta_pi", "<f8"), ("theta_h", "<f8"),
                        ("theta_l", "<f8"), ("tajima_d", "<f8"), ("faywu_h", "<f8"), ("faywu_h_norm", "<f8"), ("zeng_e", "<f8")])
PAIR_DTYPE = np.dtype([("private_a", "<u4"), ("private_b", "<u4"), ("shared", "<u4"), ("fixed_a", "<u4"), ("fixed_b", "<u4"),
                       ("n_union", "<u4"), ("n_skipped", "<u4"), ("flags", "<u4")])
DOUBLE_FIELDS = ("theta_w", "theta_pi", "theta_h", "theta_l", "tajima_d", "faywu_h", "faywu_h_norm", "zeng_e")
NAN = float("nan")


def tajima_constants(n):
    """a1, a2, e1, e2 of tj_d.py:41-60 for n >= 2"""
    a1 = 0.0
    for i in range(1, n):
        a1 += 1.0 / float(i)
    a2 = 0.0
    for i in range(1, n):
        a2 += 1.0 / (float(i) * float(i))
    dn = float(n)
    b1 = (dn + 1.0) / (3.0 * (dn - 1.0))
    b2 = 2.0 * (dn * dn + dn + 3.0) / (9.0 * dn * (dn - 1.0))
    c1 = b1 - (1.0 / a1)
    c2 = b2 - ((dn + 2.0) / (a1 * dn)) + (a2 / (a1 * a1))
    e1 = c1 / a1
    e2 = c2 / (a1 * a1 + a2)
    return a1, a2, e1, e2


_CONSTANTS = {}


def doubles(n, seg, sum_het, sum_c, sum_c2):
    """theta_w, theta_pi, theta_h, theta_l, tajima_d, faywu_h, faywu_h_norm, zeng_e in the header's operation order"""
    n = int(n)
    if n < 2:
        return (NAN,) * 8
    if n not in _CONSTANTS:
        _CONSTANTS[n] = tajima_constants(n)
    a1, a2, e1, e2 = _CONSTANTS[n]
    dn, S = float(n), float(int(seg))

    def ratio(num, var):
        return num / math.sqrt(var) if S > 0.0 and var > 0.0 and math.isfinite(var) else NAN

    P = dn * (dn - 1.0) / 2.0
    theta_w = S / a1
    theta_pi = float(int(sum_het)) / P
    theta_h = float(int(sum_c2)) / P
    theta_l = float(int(sum_c)) / (dn - 1.0)
    var_d = e1 * S + e2 * S * (S - 1.0)
    tajima_d = ratio(theta_pi - theta_w, var_d)
    T2 = S * (S - 1.0) / (a1 * a1 + a2)
    b = a2 + 1.0 / (dn * dn)
    faywu_h = theta_pi - theta_h
    var_h = (dn - 2.0) / (6.0 * (dn - 1.0)) * theta_w + \
        (18.0 * dn * dn * (3.0 * dn + 2.0) * b - (88.0 * dn * dn * dn + 9.0 * dn * dn - 13.0 * dn + 6.0)) / \
        (9.0 * dn * (dn - 1.0) * (dn - 1.0)) * T2
    faywu_h_norm = ratio(theta_pi - theta_l, var_h)
    var_e = (dn / (2.0 * (dn - 1.0)) - 1.0 / a1) * theta_w + \
        (a2 / (a1 * a1) + 2.0 * (dn / (dn - 1.0)) * (dn / (dn - 1.0)) * a2 -
         2.0 * (dn * a2 - dn + 1.0) / ((dn - 1.0) * a1) - (3.0 * dn + 1.0) / (dn - 1.0)) * T2
    zeng_e = ratio(theta_l - theta_w, var_e)
    return theta_w, theta_pi, theta_h, theta_l, tajima_d, faywu_h, faywu_h_norm, zeng_e


def polarized_counts(m01, pops, outgroup, counts=None):
    """-> (counts [K][n_site] as the outgroup polarises them, tie [n_site], flipped [n_site]).  counts = the populations' column
    sums as stored, [K][n_site], where the caller has them already (a wide matrix is then not cast to int64 as a whole; m01 is
    not read)"""
    if counts is None:
        m = np.asarray(m01).astype(np.int64)
        counts = [m[list(p)].sum(axis=0) for p in pops]
    counts = [[int(x) for x in c] for c in counts]
    n_site = len(counts[0])
    sizes = [len(p) for p in pops]
    tie, flipped = [False] * n_site, [False] * n_site
    if outgroup is not None:
        for s in range(n_site):
            cO, nO = counts[outgroup][s], sizes[outgroup]
            if 2 * cO == nO:
                tie[s] = True
            elif 2 * cO > nO:
                flipped[s] = True
                for k in range(len(pops)):
                    counts[k][s] = sizes[k] - counts[k][s]
    return counts, tie, flipped


def reference(m01, pops, pairs, windows, outgroup=None, weights=None, counts=None):
    """-> (stats [n_windows, K], pair records [n_windows, P], sfs: K arrays [n_windows, n_k + 1], jsfs: P arrays
    [n_windows, n_a + 1, n_b + 1]); pops = lists of haplotype indices, pairs = rows (a, b) of indices into pops, windows =
    (site_begin, site_end) rows, outgroup = an index into pops or None, weights = one integer per site or None, counts as
    in polarized_counts"""
    counts, tie, _ = polarized_counts(m01, pops, outgroup, counts)
    n_site = len(counts[0])
    sizes = [len(p) for p in pops]
    K, P, W = len(pops), len(pairs), len(windows)
    wt = [1] * n_site if weights is None else [int(x) for x in weights]
    stats = np.zeros((W, K), dtype=STATS_DTYPE)
    prec = np.zeros((W, P), dtype=PAIR_DTYPE)
    sfs = [np.zeros((W, sizes[k] + 1), dtype=np.uint32) for k in range(K)]
    jsfs = [np.zeros((W, sizes[a] + 1, sizes[b] + 1), dtype=np.uint32) for a, b in pairs]
    for wi, w in enumerate(windows):
        b, e = int(w[0]), int(w[1])
        n_sites = sum(wt[b:e])
        skipped = sum(1 for s in range(b, e) if tie[s])
        for k in range(K):
            n = sizes[k]
            seg = eta1 = eta_n1 = het = sc = sc2 = 0
            for s in range(b, e):
                c = counts[k][s]
                if tie[s] or not 0 < c < n:
                    continue
                seg += 1
                eta1 += c == 1
                eta_n1 += c == n - 1
                het += wt[s] * c * (n - c)
                sc += wt[s] * c
                sc2 += wt[s] * c * c
                sfs[k][wi, c] += 1
            stats[wi, k] = (n_sites, seg, eta1, eta_n1, skipped, 0, het, sc, sc2) + doubles(n, seg, het, sc, sc2)
        for pi, (a, bb) in enumerate(pairs):
            nA, nB = sizes[a], sizes[bb]
            cls = [0, 0, 0, 0, 0]
            for s in range(b, e):
                if tie[s]:
                    continue
                cA, cB = counts[a][s], counts[bb][s]
                sA, sB = 0 < cA < nA, 0 < cB < nB
                hit = [sA and not sB, sB and not sA, sA and sB, cA == nA and cB == 0, cA == 0 and cB == nB]
                assert sum(hit) <= 1
                for f in range(5):
                    cls[f] += hit[f]
                if any(hit):
                    jsfs[pi][wi, cA, cB] += 1
            prec[wi, pi] = tuple(cls) + (sum(cls), skipped, 0)
    return stats, prec, sfs, jsfs


def bits_equal(a, b):
    """element-wise: the same bits, or NaN against NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def assert_records(got, want, tag="", skip=()):
    """every integer equal, every double equal bit for bit (NaN matches NaN); for either record type"""
    assert got.shape == want.shape and got.dtype.names == want.dtype.names, (tag, got.shape, want.shape)
    for name in want.dtype.names:
        if name in skip:
            continue
        a, b = np.asarray(got[name]), np.asarray(want[name])
        same = bits_equal(a, b) if want.dtype[name].kind == "f" else a == b
        assert same.all(), (tag, name, np.argwhere(~same)[:4].tolist(), a[~same][:4], b[~same][:4])


def assert_matches(got, want, tag="", skip=()):
    """got / want = (stats, pair records, sfs or None, jsfs or None): records as assert_records, every table bin equal"""
    assert_records(got[0], want[0], (tag, "stats"), skip)
    assert_records(got[1], want[1], (tag, "pairs"), skip)
    for which, name in ((2, "sfs"), (3, "jsfs")):
        if got[which] is None:
            continue
        assert len(got[which]) == len(want[which]), (tag, name)
        for i, (a, b) in enumerate(zip(got[which], want[which])):
            assert a.shape == b.shape and a.dtype == np.uint32, (tag, name, i, a.shape, b.shape)
            assert (a == b).all(), (tag, name, i, np.argwhere(a != b)[:4].tolist())
