#!/usr/bin/env python3
"""impop_pairdist_scan at 465 haplotypes on the synthetic bench chromosome, from one process and one run:

  tiling_50kb       --windows (default 4096) windows of 50 kb, one Gram matrix each
  sliding_10kb_5kb  the 10 kb windows stepping by 5 kb over the same span (elementary segments shared between neighbours)

Per window list, K = 2 panels (140 / 100 haplotypes) and K = 5 (140 / 88 / 100 / 60 / 72), each without histograms and with 256 bins
of width 4: the whole call (median of 5 after 3 warm-up), the Gram time and the distribution kernel's time from HIP events
(impop_ctx_gram_timing: impop_ctx_gram_elapsed, impop_ctx_pairdist_elapsed), and the kernel's share of the call.
Baseline, in the same process on the same matrix: the only route there was before this call — one impop_pairwise_counts per window
(the full Gram matrix copied to the host) plus the numpy statement of the same records (tests/plain_pairdist.window, no
histograms), timed on --baseline-windows windows of the list and scaled per window; its records are compared with the call's.
No counter run is made here: which of the strided column reads, the LDS atomics of the histograms and the wave reductions bounds the
distribution kernel is NOT attributed.
One JSON line on stdout; --out FILE also writes it there (the recorded run: profiles/r21_pairdist_scan.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import impop_amd  # noqa: E402
import plain_pairdist as pp  # noqa: E402

N_HAP, SEED, SIZES = 465, 1, (140, 88, 100, 60, 72)
BINS, WIDTH = 256, 4


def passes(fn, warmup=3, steps=5):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), max(ts) - min(ts)


def windows_of(name, nw):
    if name == "tiling_50kb":
        return [(k * 50000, (k + 1) * 50000, 50000) for k in range(nw)]
    return [(5000 * k, 5000 * k + 10000, 10000) for k in range(max(nw * 10239 // 4096, 1))]


def panels(K):
    perm = np.random.default_rng(SEED).permutation(N_HAP)
    sizes = SIZES if K == 5 else (140, 100)
    pops, o = [], 0
    for s in sizes:
        f = np.zeros(N_HAP, np.uint8)
        f[perm[o: o + s]] = 1
        o += s
        pops.append(f)
    return pops


def point(ctx, bm, wins, pops, bins):
    kw = dict(hist_bins=bins, hist_width=WIDTH if bins else 1)
    t, spread = passes(lambda: bm.pairdist_scan(wins, pops, **kw))
    ctx.gram_timing(True)
    bm.pairdist_scan(wins, pops, **kw)
    gram_ms, launches = ctx.gram_elapsed()
    epi_ms, chunks = ctx.pairdist_elapsed()
    ctx.gram_timing(False)
    return {"call_ms": round(t * 1e3, 3), "spread_ms": round(spread * 1e3, 3), "us_per_window": round(t / len(wins) * 1e6, 3),
            "gram_kernel_ms": round(gram_ms, 3), "gram_launches": int(launches), "pairdist_kernel_ms": round(epi_ms, 3), "chunks": int(chunks),
            "pairdist_share_of_call": round(epi_ms / (t * 1e3), 3)}


def baseline(bm, wins, pops, n_sub, call_ms):
    idx = [np.flatnonzero(p).tolist() for p in pops]
    sub = [wins[int(k)] for k in np.linspace(0, len(wins) - 1, n_sub).astype(int)]

    def loop():
        return [pp.window(pp.hamming(bm.pairwise_counts(w[0], w[1]).astype(np.int64)), w[1] - w[0], idx) for w in sub]

    per = loop()
    t0 = time.perf_counter()
    loop()
    t = time.perf_counter() - t0
    want = pp.pack(per, len(pops), 0)
    got = bm.pairdist_scan(sub, pops)
    same = bool(got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes())
    per_window_ms = t * 1e3 / len(sub)
    return {"windows_timed": len(sub), "ms_per_window": round(per_window_ms, 3), "scaled_ms": round(per_window_ms * len(wins), 1),
            "records_equal": same, "ratio_to_pairdist_scan": round(per_window_ms * len(wins) / call_ms, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--baseline-windows", type=int, default=24)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = impop_amd.Context(0)
    res = {"bench": "pairdist_scan", "device": ctx.device_name(), "n_hap": N_HAP, "hist": f"{BINS} bins of width {WIDTH}",
           "passes": "median of 5 after 3 warm-up; spread = max - min",
           "not_measured": "no counter run: the split of the distribution kernel between strided column reads out of L2, LDS histogram atomics "
                           "and wave reductions is unattributed"}
    bm = ctx.synthetic(N_HAP, 50000 * a.windows, seed=SEED, keep_hap_major=True)
    for name in ("tiling_50kb", "sliding_10kb_5kb"):
        wins = windows_of(name, a.windows)
        r = {"windows": len(wins)}
        for K in (2, 5):
            pops = panels(K)
            r[f"K{K}"] = point(ctx, bm, wins, pops, 0)
            r[f"K{K}_hist"] = point(ctx, bm, wins, pops, BINS)
            r[f"K{K}_counts_loop"] = baseline(bm, wins, pops, a.baseline_windows, r[f"K{K}"]["call_ms"])
        res[name] = r
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
