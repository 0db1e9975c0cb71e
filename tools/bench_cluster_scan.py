#!/usr/bin/env python3
"""impop_cluster_scan next to impop_pairwise_scan(s_scope=2) on the same windows, from one process and one run:

  tiling    the bench.py all-pairs shape: 4096 x 50 kb windows, 465 haplotypes, `match`, t = 0.999
  sliding   10 kb windows every 5 kb over the same matrix (windows are sums of 5 kb segments)
  chained   the generator of tools/bench_pairwise_groups.py (32 founders whose pairwise distances straddle the threshold: pica2
            finds hundreds of groups there) — under af's transitive closure the founders chain into ONE cluster per window: the
            all-linked extreme
  many      hundreds of clusters per window: t = 1.0 without rounding (af.py's default: clusters = distinct haplotypes) on 8
            founders with about one private difference per haplotype and 50 kb window.  The point is REFUSED (exit 1, no
            JSON) unless the mean number of clusters per window is at least 100, and window 0's cluster sizes are checked on
            the host against the distinct rows of the downloaded window.

Per point: windows/s of both calls and of the call with its member tables (each 3 warm-up, best of 5 timed calls: the clock
settles under FP4 load), the
clustering kernel's own time from HIP events next to the Gram kernel's (impop_ctx_gram_timing), clusters per window.
One JSON line on stdout; --out FILE also writes it there.  --windows N scales every point down for a rehearsal."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import impop_amd  # noqa: E402


def timed(fn, warmup=3, steps=5):
    for _ in range(warmup):
        fn()
    best = 1e30
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        best = min(best, time.perf_counter() - t0)
    return best


def point(ctx, bm, wins, thr, digits, min_clusters=0):
    kw = dict(kind="match", threshold=thr, round_digits=digits)
    t_cl = timed(lambda: bm.cluster_scan(wins, want_members=False, **kw))
    t_clm = timed(lambda: bm.cluster_scan(wins, want_members=True, **kw))
    t_pw = timed(lambda: bm.pairwise_scan(wins, s_scope=2, **kw))
    ctx.gram_timing(True)
    rec = bm.cluster_scan(wins, want_members=False, **kw)
    gram_ms, _ = ctx.gram_elapsed()
    clus_ms, chunks = ctx.cluster_elapsed()
    ctx.gram_timing(False)
    K = rec["n_clusters"]
    if min_clusters and float(K.mean()) < min_clusters:
        sys.exit(f"refused: {float(K.mean()):.1f} clusters per window on average, the point asks for at least {min_clusters}")
    return {"windows": len(wins), "cluster_scan_windows_per_s": round(len(wins) / t_cl, 1),
            "cluster_scan_with_members_windows_per_s": round(len(wins) / t_clm, 1),
            "pairwise_scan_s_scope2_windows_per_s": round(len(wins) / t_pw, 1), "cluster_scan_ms": round(t_cl * 1e3, 3),
            "pairwise_scan_ms": round(t_pw * 1e3, 3), "gram_kernel_ms": round(gram_ms, 3), "cluster_kernel_ms": round(clus_ms, 3),
            "chunks": int(chunks), "clusters_per_window_mean": round(float(K.mean()), 2), "clusters_per_window_max": int(K.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--out")
    a = ap.parse_args()
    n, W, NW = 465, 50000, a.windows
    ctx = impop_amd.Context(0)
    res = {"bench": "cluster_scan", "device": ctx.device_name(), "n_hap": n, "threshold": 0.999, "round_digits": 5}
    bm = ctx.synthetic(n, W * NW, seed=1, keep_hap_major=True)
    res["tiling_50kb"] = point(ctx, bm, impop_amd.fixed_windows(W * NW, W), 0.999, 5)
    span = W * NW // 4
    sliding = [(s, s + 10000, 10000) for s in range(0, span - 10000 + 1, 5000)]
    res["sliding_10kb_5kb"] = point(ctx, bm, sliding, 0.999, 5)
    bm.free()
    NG = max(NW // 2, 1)
    bm = ctx.synthetic(n, W * NG, seed=7, n_founder=32, p_founder=2e-4, keep_hap_major=True)
    res["chained_50kb"] = point(ctx, bm, impop_amd.fixed_windows(W * NG, W), 0.999, 5)
    bm.free()
    bm = ctx.synthetic(n, W * NG, seed=11, n_founder=8, p_founder=1e-3, p_private_word=6e-4, keep_hap_major=True)
    wins = impop_amd.fixed_windows(W * NG, W)
    res["many_50kb_t1"] = point(ctx, bm, wins, 1.0, None, min_clusters=100)
    # window 0 on the host: at t = 1.0 the clusters are the distinct rows of the window
    rows = impop_amd.unpack_hap_major(bm.download(0, W), W)
    _, counts = np.unique(rows, axis=0, return_counts=True)
    _, _, sz = bm.cluster_scan(wins[:1], kind="match", threshold=1.0)
    got = sz[0][sz[0] > 0]
    assert sorted(got.tolist(), reverse=True) == sorted(counts.tolist(), reverse=True), "window 0: cluster sizes differ from the distinct rows"
    res["many_50kb_t1"]["window0_clusters_checked_on_host"] = int(len(counts))
    bm.free()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
