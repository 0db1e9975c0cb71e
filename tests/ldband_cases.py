"""Shared by the banded-LD tests: the plain restatement of impop_ldband_scan, the header's known answer and the comparison rule.

The restatement follows include/impop_hip.h (impop_ldband_scan) operation by operation, each from the full q x q tables of a window
and never by the kernel's running scheme: num, den and the one IEEE division of ld_cases.pair_tables, fx by one exact scaling and
one truncation, the band as a mask over index and coordinate differences, strong and perfect in integers, the bins by integer
division, the pruning by the sliding register K exactly as the header words it (a Python integer).  Everything the device writes is
an integer and mean_r2 is one host operation on exact values, so integers and tables must be equal and mean_r2 equal bit for bit
(NaN as NaN): a difference is a bug, not noise."""
import numpy as np

import ld_cases as lc
from ld_cases import members, pair_tables, planted_matrix, qualifying, window_list  # noqa: F401  (the tests take them from here)
from recomb_cases import KNOWN_ROWS  # noqa: F401

FX_ONE = 1 << 30
INTEGERS = ("n_members", "n_sites", "n_qualifying", "n_kept", "n_pairs", "sum_r2_fx", "n_strong", "n_perfect", "site_off")
BIN_FIELDS = ("pairs", "sum_r2_fx", "n_strong")
SITE_FIELDS = ("coord", "ld_score_fx", "carriers", "n_partners", "n_strong", "kept")

# the header's known answer: recomb_cases.KNOWN_ROWS, one window [0, 5)
KNOWN_PARAMS = dict(min_mac=1, band_sites=4, max_dist=0, bin_width=2, n_bins=3, threshold=(1, 2))
KNOWN = {"n_pairs": 10, "sum_r2_fx": 4652881236, "n_perfect": 3, "n_strong": 3, "n_kept": 3, "kept": [1, 1, 0, 0, 1],
         "ld_score_fx": [2505397589, 357913941, 2505397589, 2505397589, 1431655764], "n_partners": [4, 4, 4, 4, 4],
         "carriers": [2, 2, 2, 2, 1], "n_strong_site": [2, 0, 2, 2, 0],
         "bins": [(4, 1431655765, 1), (5, 2863311530, 2), (1, 357913941, 0)]}


def window_tables(rows, coords, n, band_sites, max_dist, bin_width, n_bins, threshold):
    """rows [q, |P|] 0/1 of a window's qualifying sites, coords [q] -> the q x q tables (upper triangle meaningful): fx (uint64),
    band, strong, perfect (bool), bin (int64)"""
    q = len(rows)
    num, den, _, r2, _ = pair_tables(rows, n)
    fx = (r2 * 1073741824.0).astype(np.uint64)  # a power-of-two scaling is exact; the cast truncates
    idx = np.arange(q, dtype=np.int64)
    gap = idx[None, :] - idx[:, None]
    c = np.asarray(coords, dtype=np.uint64).astype(np.int64)
    dist = c[None, :] - c[:, None]
    band = (gap >= 1) & (gap <= band_sites)
    if max_dist:
        band &= dist <= max_dist
    sq, d = (num * num).astype(np.uint64), den.astype(np.uint64)
    strong = sq * np.uint64(threshold[1]) > np.uint64(threshold[0]) * d
    perfect = sq == d
    bins = np.minimum(np.where(band, dist, 0) // int(bin_width), n_bins - 1)
    return fx, band, strong, perfect, bins


def prune(strong_band, band_sites):
    """the header's sliding window: strong_band[i, j] for i < j -> kept (list of 0/1)"""
    q = len(strong_band)
    K, full, kept = 0, (1 << band_sites) - 1, []
    for j in range(q):
        mask = 0
        for o in range(1, min(j, band_sites) + 1):
            if strong_band[j - o, j]:
                mask |= 1 << (o - 1)
        k = 1 if (mask & K) == 0 else 0
        K = ((K << 1) | k) & full
        kept.append(k)
    return kept


def reference(m01, flags, windows, min_mac=2, band_sites=256, max_dist=0, bin_width=1000, n_bins=100, threshold=(1, 5), pos=None,
              weights=None):
    """-> (records as a dict of arrays, bins as a dict of [n_windows, n_bins] uint64, the flat site table as a dict of arrays).
    pos: the coordinate of every column (default: its index), as a compacted matrix reports it"""
    P = members(m01, flags)
    n = len(P)
    rowsP = m01[P]
    qual = qualifying(m01, flags, min_mac)
    rec = {k: np.zeros(len(windows), dtype=np.uint64) for k in INTEGERS}
    rec["mean_r2"] = np.zeros(len(windows), dtype=np.float64)
    bins = {k: np.zeros((len(windows), n_bins), dtype=np.uint64) for k in BIN_FIELDS}
    table = {k: [] for k in SITE_FIELDS}
    off = 0
    for i, (b, e) in enumerate(windows):
        qs = qual[np.searchsorted(qual, b):np.searchsorted(qual, e)]
        q = len(qs)
        coords = np.asarray(qs if pos is None else np.asarray(pos)[qs], dtype=np.uint64)
        rows = rowsP[:, qs].T
        fx, band, strong, perfect, bn = window_tables(rows, coords, n, band_sites, max_dist, bin_width, n_bins, threshold)
        fxb = np.where(band, fx, np.uint64(0))
        sb = band & strong
        n_pairs, total = int(band.sum()), int(fxb.sum(dtype=np.uint64))
        for k, v in (("pairs", band.astype(np.uint64)), ("sum_r2_fx", fxb), ("n_strong", sb.astype(np.uint64))):
            np.add.at(bins[k][i], bn[band], v[band])
        kept = prune(sb, band_sites)
        both, both_band, both_strong = fxb + fxb.T, band | band.T, sb | sb.T
        table["coord"] += [int(x) for x in coords]
        table["ld_score_fx"] += [int(x) for x in both.sum(axis=1, dtype=np.uint64)] if q else []
        table["carriers"] += [int(x) for x in rows.sum(axis=1, dtype=np.int64)] if q else []
        table["n_partners"] += [int(x) for x in both_band.sum(axis=1)] if q else []
        table["n_strong"] += [int(x) for x in both_strong.sum(axis=1)] if q else []
        table["kept"] += kept
        rec["n_members"][i], rec["n_qualifying"][i], rec["n_kept"][i], rec["site_off"][i] = n, q, sum(kept), off
        rec["n_sites"][i] = (e - b) if weights is None else int(np.asarray(weights[b:e], dtype=np.int64).sum())
        rec["n_pairs"][i], rec["sum_r2_fx"][i], rec["n_strong"][i] = n_pairs, total, int(sb.sum())
        rec["n_perfect"][i] = int((band & perfect).sum())
        rec["mean_r2"][i] = float(total) / (float(n_pairs) * 1073741824.0) if n_pairs else float("nan")
        off += q
    dt = {"coord": np.uint64, "ld_score_fx": np.uint64}
    return rec, bins, {k: np.asarray(v, dtype=dt.get(k, np.uint32)) for k, v in table.items()}


def assert_matches(got, ref, where=""):
    """got = (records, bins, site table) of BitMatrix.ldband_scan(want_bins=True, want_sites=True), ref = reference(...)"""
    rec, bins, table = got
    want, wbins, wtable = ref
    assert len(rec) == len(want["n_pairs"]), where
    for k in INTEGERS:
        assert np.array_equal(rec[k].astype(np.uint64), want[k]), (where, k, rec[k][:12], want[k][:12])
    same = lc.bits(rec["mean_r2"]) == lc.bits(want["mean_r2"])
    assert same.all(), (where, "mean_r2", int(np.flatnonzero(~same)[0]), rec["mean_r2"][~same][:4], want["mean_r2"][~same][:4])
    assert bins.shape == wbins["pairs"].shape, (where, bins.shape)
    for k in BIN_FIELDS:
        assert np.array_equal(bins[k], wbins[k]), (where, "bins", k)
    assert len(table) == len(wtable["coord"]) == int(want["n_qualifying"].sum()), (where, "n_site_rows", len(table))
    for k in SITE_FIELDS:
        assert np.array_equal(table[k], wtable[k]), (where, "site table", k)
