#!/usr/bin/env python3
"""impop_ldband_scan at 465 haplotypes, from one process and one run, min_mac 2, band 256, threshold 1/5, decay bins on:

  compact_50kb   --windows (4096) x 50 kb windows of the synthetic founder chromosome, compacted to its variable sites
  dense_50kb     --dense-windows (256; 0: skip) x 50 kb windows of the 12.8 M-site slab whose founders differ at 0.9 % of the
                 sites: thousands of qualifying sites per window, the pair kernel's own load
  dense_whole    the same slab as ONE window: a chromosome-arm window, no thinning

Per point: the median of 5 timed calls after one warm-up call of BitMatrix.ldband_scan(want_bins=True); from HIP events
(impop_ctx_gram_timing) the time of its five kernel groups (select, counting pass included / rank + gather / pairs / prune /
reduce) in one call; q and the band pairs; for the pair kernel band pairs per second and pairs x wps x 4 B/s, the row bytes a
pair's popcounts read (the kernel evaluates every pair from both of its sites, so it does twice that work).  Next to it the same
figure of recomb_pairs_kernel computed from profiles/r29_recomb_scan.json (site_pairs_per_s x wps x 4): a yardstick, not a gate.
  numpy_ms_per_window  the plain numpy restatement (all pairs of a window by one matrix product, the band as a mask, the pruning
                 as a loop over sites) on --numpy-windows (2) windows of dense_50kb, rows downloaded from the device; its
                 integers must equal the device's.  numpy_ratio = that mean x the windows of the point / the call's ms.
One JSON line on stdout; --out FILE also writes it there (the recorded run: profiles/r30_ldband_scan.json).  --windows N and
--dense-windows N scale the points down for a rehearsal."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import impop_amd  # noqa: E402

N_HAP, SEED, MIN_MAC, BAND, THR = 465, 1, 2, 256, (1, 5)
WPS = (N_HAP + 31) // 32
DENSE_P_FOUNDER = 0.009
BINS = {"compact_50kb": (1000, 100), "dense_50kb": (100, 100), "dense_whole": (100, 100)}  # bin_width, n_bins


def passes(fn, warmup=1, steps=5):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def numpy_window(m01, coords, bin_width, n_bins):
    """the restatement of one window from its [n, W] 0/1 matrix -> (q, n_pairs, sum_r2_fx, n_strong, n_perfect, n_kept)"""
    n = m01.shape[0]
    c_all = m01.sum(axis=0, dtype=np.int64)
    qual = np.flatnonzero(np.minimum(c_all, n - c_all) >= MIN_MAC)
    q = len(qual)
    f = m01[:, qual].T.astype(np.float32)  # counts <= 465: exact in float32
    c = c_all[qual]
    n11 = (f @ f.T).astype(np.int64)
    num = n * n11 - np.outer(c, c)
    v = c * (n - c)
    den = np.outer(v, v)
    fx = ((num * num).astype(np.float64) / den.astype(np.float64) * 1073741824.0).astype(np.uint64)
    idx = np.arange(q)
    gap = idx[None, :] - idx[:, None]
    band = (gap >= 1) & (gap <= BAND)
    strong = band & ((num * num) * THR[1] > THR[0] * den)
    pos = coords[qual]
    bins = np.bincount(np.minimum((pos[None, :] - pos[:, None])[band] // bin_width, n_bins - 1), minlength=n_bins)
    kept = np.zeros(q, dtype=bool)
    for j in range(q):
        lo = max(0, j - BAND)
        kept[j] = not (kept[lo:j] & strong[lo:j, j]).any()
    assert int(bins.sum()) == int(band.sum())
    return q, int(band.sum()), int(fx[band].sum(dtype=np.uint64)), int(strong.sum()), int((band & (num * num == den)).sum()), int(kept.sum())


def numpy_reference(bm, wins, rec, bin_width, n_bins, k):
    if k <= 0:
        return None, 0, True
    pick = sorted({int(i) for i in np.linspace(0, len(wins) - 1, k)})
    ts, same = [], True
    for i in pick:
        b, e = int(wins[i][0]), int(wins[i][1])
        bits = bm.download(b, e)
        m01 = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :e - b]
        t0 = time.perf_counter()
        got = numpy_window(m01, np.arange(b, e, dtype=np.int64), bin_width, n_bins)
        ts.append(time.perf_counter() - t0)
        r = rec[i]
        same &= got == tuple(int(r[f]) for f in ("n_qualifying", "n_pairs", "sum_r2_fx", "n_strong", "n_perfect", "n_kept"))
    return statistics.mean(ts) * 1e3, len(pick), bool(same)


def point(ctx, bm, name, wl, numpy_windows):
    wins = impop_amd.make_windows(wl)
    bin_width, n_bins = BINS[name]
    kw = dict(min_mac=MIN_MAC, band_sites=BAND, threshold=THR, bin_width=bin_width, n_bins=n_bins, want_bins=True)
    rec, bins = bm.ldband_scan(wins, **kw)
    t = passes(lambda: bm.ldband_scan(wins, **kw))
    ctx.gram_timing(True)
    bm.ldband_scan(wins, **kw)
    ker, chunks = ctx.ldband_elapsed()
    ctx.gram_timing(False)
    np_ms, np_n, np_same = numpy_reference(bm, wl, rec, bin_width, n_bins, numpy_windows)
    q, pairs = int(rec["n_qualifying"].sum()), int(rec["n_pairs"].sum())
    pps = pairs / (ker[2] * 1e-3) if ker[2] > 0 else None
    total_fx, total_pairs = int(rec["sum_r2_fx"].sum()), max(pairs, 1)
    return {"windows": len(wins), "band": BAND, "bin_width": bin_width, "n_bins": n_bins, "ldband_scan_ms": round(t * 1e3, 3),
            "kernel_ms": {k: round(v, 3) for k, v in zip(("select", "rank_gather", "pairs", "prune", "reduce"), ker)},
            "kernels_ms": round(sum(ker), 3), "chunks": int(chunks), "qualifying": q, "max_qualifying": int(rec["n_qualifying"].max()),
            "band_pairs": pairs, "band_pairs_per_s": None if pps is None else round(pps, 1),
            "pair_row_TBps": None if pps is None else round(pps * WPS * 4 / 1e12, 3),
            "strong_pairs": int(rec["n_strong"].sum()), "kept_sites": int(rec["n_kept"].sum()),
            "mean_r2": round(total_fx / (total_pairs * 1073741824.0), 6), "bins_filled": int((bins["pairs"].sum(axis=0) > 0).sum()),
            "numpy_ms_per_window": None if np_ms is None else round(np_ms, 3), "numpy_windows": np_n, "numpy_equal": np_same,
            "numpy_ratio": None if np_ms is None else round(np_ms * len(wins) / (t * 1e3), 1)}


def recomb_yardstick():
    try:
        r = json.loads(open(os.path.join(ROOT, "profiles", "r29_recomb_scan.json")).readline())
        return {k: round(r[k]["site_pairs_per_s"] * WPS * 4 / 1e12, 3) for k in ("tiling_50kb", "dense_50kb") if k in r}
    except (OSError, ValueError, KeyError):
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--dense-windows", type=int, default=256)
    ap.add_argument("--numpy-windows", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = impop_amd.Context(0)
    res = {"bench": "ldband_scan", "device": ctx.device_name(), "n_hap": N_HAP, "wps": WPS, "min_mac": MIN_MAC, "threshold": list(THR),
           "passes": "median of 5 after 1 warm-up", "dense_p_founder": DENSE_P_FOUNDER,
           "recomb_pairs_kernel_row_TBps": recomb_yardstick()}
    full = ctx.synthetic(N_HAP, 50000 * a.windows, seed=SEED, keep_hap_major=False)
    bm = full.compact()
    full.free()
    res["compact_50kb"] = point(ctx, bm, "compact_50kb", [(k * 50000, (k + 1) * 50000, 50000) for k in range(a.windows)], 0)
    bm.free()
    if a.dense_windows > 0:
        bm = ctx.synthetic(N_HAP, 50000 * a.dense_windows, seed=SEED, p_founder=DENSE_P_FOUNDER, keep_hap_major=False)
        res["dense_50kb"] = point(ctx, bm, "dense_50kb", [(k * 50000, (k + 1) * 50000, 50000) for k in range(a.dense_windows)], a.numpy_windows)
        res["dense_whole"] = point(ctx, bm, "dense_whole", [(0, 50000 * a.dense_windows, 50000 * a.dense_windows)], 0)
        bm.free()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
