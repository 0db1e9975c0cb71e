#!/usr/bin/env python3
"""impop_permtest_scan on the synthetic bench chromosome (465 haplotypes), from one process and one run, on --windows (default 4096)
tiling windows of 50 kb:

  two panels    haplotypes 0-139 / 140-239 at n_perm = 100 and 1000, on the full matrix; n_perm = 1000 again on the matrix compacted
                to its variable sites
  five panels   93 haplotypes each (10 pairs) at n_perm = 1000, on the full matrix

Per point: the whole call (median of 3 after 1 warm-up), the Gram time (impop_ctx_gram_elapsed), the preparation and the labelling
kernel (impop_ctx_permtest_elapsed), and the labelling kernel's int8 MAC rate — m_pad^2 x 64 columns x planes per task — as a
fraction of the i8 peak, taken as twice the ~2.5 PF dense BF16 figure: 2.5e15 MAC/s.
Yardstick, in the same process on the same matrix, windows and panels: impop_pairdist_scan, and the ratio of the two calls.
No counter run is made here: how the labelling kernel's time splits between the matrix cores, the plane loads out of L2 and the
S_nn popcounts in the VALU is NOT attributed.
One JSON line on stdout; --out FILE also writes it there (the recorded run: profiles/r24_permtest_scan.json)."""
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

N_HAP, SEED = 465, 1
I8_PEAK_MAC_PER_S = 2.5e15


def passes(fn, warmup=1, steps=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), max(ts) - min(ts)


def panel(lo, hi):
    f = np.zeros(N_HAP, np.uint8)
    f[lo:hi] = 1
    return f


def point(ctx, bm, wins, pops, n_perm, planes):
    t, spread = passes(lambda: bm.permtest_scan(wins, pops, n_perm=n_perm, seed=SEED))
    ctx.gram_timing(True)
    bm.permtest_scan(wins, pops, n_perm=n_perm, seed=SEED)
    gram_ms, _ = ctx.gram_elapsed()
    (prep_ms, label_ms), chunks = ctx.permtest_elapsed()
    ctx.gram_timing(False)
    sizes = [int(p.sum()) for p in pops]
    tasks_per_pair = (n_perm + 62) // 63
    macs = 0
    for a in range(len(sizes)):
        for b in range(a + 1, len(sizes)):
            m_pad = (sizes[a] + sizes[b] + 63) // 64 * 64
            macs += m_pad * m_pad * 64 * planes * tasks_per_pair
    macs *= len(wins)
    rate = macs / (label_ms * 1e-3) if label_ms > 0 else 0.0
    yt, _ = passes(lambda: bm.pairdist_scan(wins, pops))
    ctx.gram_timing(True)
    bm.pairdist_scan(wins, pops)
    pd_ms, _ = ctx.pairdist_elapsed()
    ctx.gram_timing(False)
    return {"panels": sizes, "n_perm": n_perm, "planes": planes, "call_ms": round(t * 1e3, 3), "spread_ms": round(spread * 1e3, 3),
            "gram_kernel_ms": round(gram_ms, 3), "prep_kernel_ms": round(prep_ms, 3), "label_kernel_ms": round(label_ms, 3), "chunks": int(chunks),
            "label_int8_macs": int(macs), "label_mac_per_s": round(rate, 1), "label_fraction_of_i8_peak": round(rate / I8_PEAK_MAC_PER_S, 5),
            "pairdist_call_ms": round(yt * 1e3, 3), "pairdist_kernel_ms": round(pd_ms, 3), "ratio_permtest_to_pairdist": round(t / yt, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = impop_amd.Context(0)
    res = {"bench": "permtest_scan", "device": ctx.device_name(), "n_hap": N_HAP, "windows": a.windows, "window_bp": 50000,
           "i8_peak_mac_per_s": I8_PEAK_MAC_PER_S, "passes": "median of 3 after 1 warm-up; spread = max - min",
           "not_measured": "no counter run: the split of the labelling kernel between the matrix cores, the plane loads and the S_nn popcounts "
                           "is unattributed"}
    wins = [(k * 50000, (k + 1) * 50000, 50000) for k in range(a.windows)]
    two = [panel(0, 140), panel(140, 240)]
    five = [panel(93 * k, 93 * (k + 1)) for k in range(5)]
    full = ctx.synthetic(N_HAP, 50000 * a.windows, seed=SEED, keep_hap_major=True)
    res["two_panels_100"] = point(ctx, full, wins, two, 100, 2)
    res["two_panels_1000"] = point(ctx, full, wins, two, 1000, 2)
    res["five_panels_1000"] = point(ctx, full, wins, five, 1000, 2)
    comp = full.compact()
    kept = np.bincount((comp.positions() // 50000).astype(np.int64), minlength=a.windows)  # kept sites per window decide the planes
    w_max = int(kept.max())
    res["two_panels_1000_compacted"] = point(ctx, comp, wins, two, 1000, 1 if w_max < 256 else 2 if w_max < 65536 else 3)
    res["two_panels_1000_compacted"]["n_site"] = int(comp.n_site)
    res["two_panels_1000_compacted"]["widest_kept_window"] = w_max
    comp.free()
    full.free()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
