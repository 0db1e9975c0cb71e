#!/usr/bin/env python3
"""impop_pca_scan at 465 haplotypes on the synthetic bench chromosome, from one process and one run: --windows (default 4096)
windows of 50 kb, on the full and on the compacted matrix, at k = 2 and k = 8.

Per point: the whole call (median of 5 after 3 warm-up), the Gram time and the eigen kernel's time from HIP events
(impop_ctx_gram_timing: impop_ctx_gram_elapsed, impop_ctx_pca_elapsed), mean and max iterations, unconverged windows; and once per
k the call with the window distances (the distance kernel over windows x windows).
Baseline, in the same process on the same matrix: what there was before this call for the same answer — one impop_pairwise_counts
per window (the full Gram matrix copied to the host), the double centring and numpy.linalg.eigh on the host — timed on
--baseline-windows windows and stated per window; its k largest eigenvalues are compared with the call's.
No counter run is made here: what bounds the eigen kernel (fp64 VALU, the L2 reads of the distance matrix, the barriers of the
reductions and of the Jacobi rounds) is NOT attributed.
One JSON line on stdout; --out FILE also writes it there (the recorded run: profiles/r26_pca_scan.json)."""
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
import plain_pca as pl  # noqa: E402
from plain_pairdist import hamming  # noqa: E402

N_HAP, SEED = 465, 1


def passes(fn, warmup=3, steps=5):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), max(ts) - min(ts)


def point(ctx, bm, wins, k, dist):
    kw = dict(k=k, want_vectors=True, want_dist=dist)
    t, spread = passes(lambda: bm.pca_scan(wins, **kw), *((1, 3) if dist else (3, 5)))
    ctx.gram_timing(True)
    recs = bm.pca_scan(wins, **kw)[0]
    gram_ms, launches = ctx.gram_elapsed()
    (eigen_ms, dist_ms), chunks = ctx.pca_elapsed()
    ctx.gram_timing(False)
    live = recs["iterations"][recs["iterations"] > 0]
    return {"call_ms": round(t * 1e3, 3), "spread_ms": round(spread * 1e3, 3), "us_per_window": round(t / len(wins) * 1e6, 3),
            "gram_kernel_ms": round(gram_ms, 3), "gram_launches": int(launches), "eigen_kernel_ms": round(eigen_ms, 3),
            "distance_kernel_ms": round(dist_ms, 3), "chunks": int(chunks), "eigen_share_of_call": round(eigen_ms / (t * 1e3), 3),
            "iterations_mean": round(float(live.mean()), 2) if len(live) else 0.0, "iterations_max": int(recs["iterations"].max()),
            "unconverged": int((recs["flags"] & 1).sum()), "rank0": int((recs["rank"] == 0).sum())}


def baseline(bm, wins, k, n_sub, call_ms):
    sub = [wins[int(i)] for i in np.linspace(0, len(wins) - 1, n_sub).astype(int)]

    def loop():
        return [pl.spectrum(hamming(bm.pairwise_counts(w[0], w[1]).astype(np.int64)))[0][:k] for w in sub]

    want = loop()
    t0 = time.perf_counter()
    loop()
    t = time.perf_counter() - t0
    got = bm.pca_scan(sub, k=k)[0]
    worst = max(float(np.abs(got[i]["lambda"][:k] - want[i]).max() / max(want[i][0], 1e-300)) for i in range(len(sub)))
    per_window_ms = t * 1e3 / len(sub)
    return {"windows_timed": len(sub), "ms_per_window": round(per_window_ms, 3), "scaled_ms": round(per_window_ms * len(wins), 1),
            "worst_relative_eigenvalue_difference": worst, "ratio_to_pca_scan": round(per_window_ms * len(wins) / call_ms, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--baseline-windows", type=int, default=64)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = impop_amd.Context(0)
    res = {"bench": "pca_scan", "device": ctx.device_name(), "n_hap": N_HAP, "windows": a.windows, "tol": 1e-10, "max_iter": 500,
           "passes": "median of 5 after 3 warm-up (with distances: of 3 after 1); spread = max - min",
           "eigen_kernel": "fp64 VALU block subspace iteration, 16 columns; no f64-MFMA form was built, so none is compared",
           "not_measured": "no counter run: the split of the eigen kernel between fp64 VALU, L2 reads of the distance matrix and barriers is "
                           "unattributed"}
    full = ctx.synthetic(N_HAP, 50000 * a.windows, seed=SEED, keep_hap_major=True)
    wins = [(i * 50000, (i + 1) * 50000, 50000) for i in range(a.windows)]
    comp = full.compact()
    for name, bm in (("dense", full), ("compact", comp)):
        r = {}
        for k in (2, 8):
            r[f"k{k}"] = point(ctx, bm, wins, k, False)
            if name == "dense":
                r[f"k{k}_with_distances"] = point(ctx, bm, wins, k, True)
                r[f"k{k}_counts_eigh_loop"] = baseline(bm, wins, k, a.baseline_windows, r[f"k{k}"]["call_ms"])
        res[name] = r
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
