"""Shared by the LD-scan tests: matrices, window lists, the plain restatement of impop_ld_scan and the comparison rule.

The restatement follows include/impop_hip.h (impop_ld_scan) operation by operation: site selection and the pair arithmetic in
integers, one IEEE division per r2 and per |D'|, and every sum in the stated order (strictly sequential: Python loops and
np.add.accumulate, never np.sum or sum(), which add in another order).  pair_scalar is the pair arithmetic in Python integers and
floats; pair_tables is the same on int64 / float64 arrays (each element one correctly rounded operation of the same exact operands)
and tests/test_ld_scan_host.py holds the two to each other bit for bit.  Integers and used_sites must be equal and doubles equal
bit for bit: a difference is a bug, not noise."""
import numpy as np

import hap_cases as hc

INTEGERS = ("n_members", "n_sites", "n_qualifying", "n_used", "n_perfect", "n_complete", "omega_split")
DOUBLES = ("sum_r2", "sum_dprime", "zns", "mean_dprime", "omega_max")
S = 3000
PLANT = (1010, 1020, 1030, 1040, 1050)  # columns planted in hap_cases.MONO, otherwise monomorphic
# q = 0..5 qualifying sites (omega is undefined below 4), then what is left of the stretch: monomorphic sites only
PLANT_WINDOWS = [(1000, 1005), (1000, 1011), (1000, 1021), (1000, 1031), (1000, 1041), (1000, 1051), (1060, 1100)]


def planted_matrix(rng, n, n_site=S, **kw):
    """hap_cases.founder_matrix with five columns planted in its monomorphic stretch: a random column x, a copy of x (r2 = 1),
    the complement of x (r2 = 1 with num < 0), a column carried only by carriers of x (three gametes: |D'| = 1, r2 < 1) and an
    independent one"""
    m = hc.founder_matrix(rng, n, n_site, **kw)
    x = (rng.random(n) < 0.5).astype(np.uint8)
    x[0], x[1] = 1, 0
    sub = x & (rng.random(n) < 0.6).astype(np.uint8)
    sub[0] = 1
    if n > 2:
        x[2], sub[2] = 1, 0
    m[:, PLANT[0]], m[:, PLANT[1]], m[:, PLANT[2]], m[:, PLANT[3]] = x, x, 1 - x, sub
    m[:, PLANT[4]] = (rng.random(n) < 0.5).astype(np.uint8)
    return np.ascontiguousarray(m)


def window_list(n_site=S):
    """starts and ends inside a 64-site block, a one-site window, empty windows, monomorphic sites only, the whole matrix, the
    planted q = 0..5 windows, and two sliding lists whose windows overlap by half"""
    w = [(37, 517), (64, 128), (100, 101), PLANT[:1] + (PLANT[0] + 1,), (200, 200), (0, n_site), (n_site - 1, n_site), (63, 65), (0, 0),
         (n_site, n_site)] + PLANT_WINDOWS
    w += [(b, min(b + 640, n_site)) for b in range(0, n_site - 320, 320)]
    w += [(b, min(b + 500, n_site)) for b in range(13, n_site - 250, 250)]
    return [(int(b), int(e)) for b, e in w]


def members(m01, flags):
    return np.arange(m01.shape[0]) if flags is None else np.flatnonzero(np.asarray(flags))


def qualifying(m01, flags, min_mac):
    """positions of the sites with min(c, |P| - c) >= min_mac, ascending"""
    P = members(m01, flags)
    c = m01[P].sum(axis=0, dtype=np.int64)
    return np.flatnonzero(np.minimum(c, len(P) - c) >= min_mac)


def thinning_ranks(q, max_sites):
    m = min(q, max_sites)
    return [(k * q) // m for k in range(m)]


def pair_scalar(row_s, row_t, n):
    """-> (num, den, r2, dmax or None, dprime) of two sites' 0/1 rows over P, in Python integers and floats"""
    cs, ct = int(sum(int(v) for v in row_s)), int(sum(int(v) for v in row_t))
    n11 = int(sum(int(a) & int(b) for a, b in zip(row_s, row_t)))
    num = n * n11 - cs * ct
    den = cs * (n - cs) * ct * (n - ct)
    r2 = float(num * num) / float(den)
    if num > 0:
        dmax = min(cs * (n - ct), (n - cs) * ct)
    elif num < 0:
        dmax = min(cs * ct, (n - cs) * (n - ct))
    else:
        return num, den, r2, None, 0.0
    return num, den, r2, dmax, float(abs(num)) / float(dmax)


def pair_tables(rows, n):
    """rows [m, |P|] 0/1 -> num, den, dmax (int64 [m, m]; dmax of num == 0 entries is not meaningful), r2, dprime (float64 [m, m])"""
    r = rows.astype(np.int64)
    c = r.sum(axis=1)
    f = rows.astype(np.float64)
    n11 = (f @ f.T).astype(np.int64)  # counts far below 2^53: exact in float64, and the product runs in BLAS
    num = n * n11 - np.outer(c, c)
    v = c * (n - c)
    den = np.outer(v, v)
    r2 = (num * num).astype(np.float64) / den.astype(np.float64)
    dmax = np.where(num > 0, np.minimum(np.outer(c, n - c), np.outer(n - c, c)), np.minimum(np.outer(c, c), np.outer(n - c, n - c)))
    dprime = np.where(num != 0, np.abs(num).astype(np.float64) / dmax.astype(np.float64), 0.0)
    return num, den, dmax, r2, dprime


def site_sums(r2, dprime):
    """-> a, b, dp (lists of floats): a_j = sum_{i<j} r2(i,j) and dp_j likewise, i ascending from 0.0; b_j = sum_{k>j} r2(j,k), k ascending"""
    m = len(r2)
    if m == 0:
        return [], [], []
    up = np.triu(r2, 1)  # zeros elsewhere: x + 0.0 == x exactly, so they do not disturb the order
    a = np.add.accumulate(up, axis=0)[-1]
    b = np.add.accumulate(up, axis=1)[:, -1]
    dp = np.add.accumulate(np.triu(dprime, 1), axis=0)[-1]
    return [float(x) for x in a], [float(x) for x in b], [float(x) for x in dp]


def prefix_suffix(a, b):
    """-> L[0..m], R[0..m]: L(l) = sum_{j<l} a_j, j ascending; R(l) = sum_{j>=l} b_j accumulated from j = m-1 downwards"""
    m = len(a)
    L, R = [0.0] * (m + 1), [0.0] * (m + 1)
    for j in range(m):
        L[j + 1] = L[j] + a[j]
    for j in range(m - 1, -1, -1):
        R[j] = R[j + 1] + b[j]
    return L, R


def omega(L, R, m):
    """-> (omega_max, omega_split): 0.0, 0 when no split is defined"""
    sum_r2 = L[m]
    best, split = 0.0, 0
    for l in range(2, m - 1):
        cross = (sum_r2 - L[l]) - R[l]
        if not cross > 0.0:
            continue
        w = ((L[l] + R[l]) / float(l * (l - 1) // 2 + (m - l) * (m - l - 1) // 2)) / (cross / float(l * (m - l)))
        if split == 0 or w > best:
            best, split = w, l
    return best, split


def reference(m01, flags, windows, min_mac=1, max_sites=512, weights=None):
    """-> (records as a dict of arrays, used_sites [n_windows, max_sites] uint64)"""
    P = members(m01, flags)
    n = len(P)
    rowsP = m01[P]
    qual = qualifying(m01, flags, min_mac)
    rec = {k: np.zeros(len(windows), dtype=np.float64 if k in DOUBLES else np.uint64) for k in INTEGERS + DOUBLES}
    used = np.zeros((len(windows), max_sites), dtype=np.uint64)
    for i, (b, e) in enumerate(windows):
        qs = qual[np.searchsorted(qual, b):np.searchsorted(qual, e)]
        q = len(qs)
        sites = [int(qs[r]) for r in thinning_ranks(q, max_sites)]
        m = len(sites)
        used[i, :m] = sites
        num, den, dmax, r2, dprime = pair_tables(rowsP[:, sites].T, n)
        iu = np.triu_indices(m, 1)
        a, bb, dp = site_sums(r2, dprime)
        L, R = prefix_suffix(a, bb)
        sum_dp = 0.0
        for x in dp:
            sum_dp = sum_dp + x
        pairs = m * (m - 1) // 2
        rec["n_members"][i], rec["n_qualifying"][i], rec["n_used"][i] = n, q, m
        rec["n_sites"][i] = (e - b) if weights is None else int(np.asarray(weights[b:e], dtype=np.int64).sum())
        rec["n_perfect"][i] = int((num[iu] * num[iu] == den[iu]).sum())
        rec["n_complete"][i] = int(((num[iu] != 0) & (np.abs(num[iu]) == dmax[iu])).sum())
        rec["sum_r2"][i], rec["sum_dprime"][i] = L[m], sum_dp
        rec["zns"][i] = 0.0 if m < 2 else L[m] / float(pairs)
        rec["mean_dprime"][i] = 0.0 if m < 2 else sum_dp / float(pairs)
        rec["omega_max"][i], rec["omega_split"][i] = omega(L, R, m)
    return rec, used


def windows_with_q(qual, q, start=3):
    """a window holding exactly q of the qualifying positions `qual`, beginning start positions in"""
    return (int(qual[start]), int(qual[start + q - 1]) + 1)


def bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def assert_matches(got, ref, where=""):
    """got = (records, used_sites) of BitMatrix.ld_scan(want_sites=True), ref = reference(...)"""
    rec, used = got
    want, wused = ref
    assert len(rec) == len(wused), where
    for k in INTEGERS:
        assert np.array_equal(rec[k].astype(np.uint64), want[k]), (where, k, rec[k][:12], want[k][:12])
    assert np.array_equal(used, wused), (where, "used_sites")
    for k in DOUBLES:
        same = bits(rec[k]) == bits(want[k])
        assert same.all(), (where, k, int(np.flatnonzero(~same)[0]), rec[k][~same][:4], want[k][~same][:4])


# the planted columns, checked where they are defined: the reference counts a perfect pair with num > 0, one with num < 0 and
# complete pairs that are not perfect
def check_planted(m01, flags=None):
    n = len(members(m01, flags))
    rows = m01[members(m01, flags)][:, list(PLANT)].T
    num, den, dmax, r2, dprime = pair_tables(rows, n)
    assert num[0, 1] > 0 and num[0, 1] ** 2 == den[0, 1] and r2[0, 1] == 1.0
    assert num[0, 2] < 0 and num[0, 2] ** 2 == den[0, 2] and r2[0, 2] == 1.0 and dprime[0, 2] == 1.0
    assert num[0, 3] != 0 and abs(num[0, 3]) == dmax[0, 3] and num[0, 3] ** 2 != den[0, 3] and dprime[0, 3] == 1.0 and r2[0, 3] < 1.0
    rec, _ = reference(m01, flags, [PLANT_WINDOWS[5]], 1, 512)
    assert rec["n_used"][0] == 5 and rec["n_perfect"][0] >= 3 and rec["n_complete"][0] > rec["n_perfect"][0]
