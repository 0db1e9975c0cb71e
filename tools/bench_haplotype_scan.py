#!/usr/bin/env python3
"""impop_haplotype_scan next to impop_cluster_scan(threshold = 1.0), the only other way to a window's haplotype spectrum, from one
process and one run:

  tiling_50kb        4096 x 50 kb windows of one synthetic founder matrix of 465 haplotypes
  sliding_10kb_5kb   10239 x 10 kb windows every 5 kb from the start of the same matrix (overlapping windows share tiles)
  one_window_chunks  the first --chunk-windows (256; 0: skip) windows of tiling_50kb with max_chunk_bytes=1: a chunk per window,
                     so the host's per-chunk path (metadata up, launches, records down, one synchronisation) is what is timed

Per point, on the same windows: the median of 5 timed calls after one warm-up call of BitMatrix.haplotype_scan and of
BitMatrix.cluster_scan(threshold=1.0, kind="match", want_members=False); from HIP events (impop_ctx_gram_timing) the time of the
haplotype scan's three kernel groups (fingerprint / grouping / verification) and of the cluster scan's Gram and clustering
kernels in one call each; and from the IMPOP_TRACE=1 line of one haplotype call, taken from a child process (the switch is read
once per process), the bytes its fingerprint kernel streams — over that kernel's time, against the 6.8 TB/s read ceiling of
profiles/r01_hbm_read_ceiling.txt.  The integers of the two calls' records are compared before anything is timed.
One JSON line on stdout; --out FILE also writes it there.  --windows N scales the points down for a rehearsal."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import impop_amd  # noqa: E402

N_HAP, SEED = 465, 1
CLUSTER_KW = dict(threshold=1.0, kind="match", want_members=False)
POINTS = ("tiling_50kb", "sliding_10kb_5kb")


def passes(fn, warmup=1, steps=5):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def windows_of(name, nw):
    if name == "tiling_50kb":
        return [(k * 50000, (k + 1) * 50000, 50000) for k in range(nw)]
    return [(5000 * k, 5000 * k + 10000, 10000) for k in range(max(nw * 10239 // 4096, 1))]


def point(ctx, bm, name, nw):
    wins = impop_amd.make_windows(windows_of(name, nw))
    hap, clu = bm.haplotype_scan(wins), bm.cluster_scan(wins, **CLUSTER_KW)
    for a, b in (("n_members", "n_members"), ("n_distinct", "n_clusters"), ("largest", "largest"), ("n_singletons", "n_singletons"),
                 ("sum_sq", "sum_sq"), ("n_sites", "n_sites")):
        assert np.array_equal(hap[a], clu[b]), (name, a)
    t_hap = passes(lambda: bm.haplotype_scan(wins))
    t_clu = passes(lambda: bm.cluster_scan(wins, **CLUSTER_KW))
    ctx.gram_timing(True)
    bm.haplotype_scan(wins)
    ker, chunks = ctx.haplotype_elapsed()
    ctx.gram_timing(False)
    ctx.gram_timing(True)
    bm.cluster_scan(wins, **CLUSTER_KW)
    gram_ms, _ = ctx.gram_elapsed()
    clus_ms, _ = ctx.cluster_elapsed()
    ctx.gram_timing(False)
    return {"windows": len(wins), "haplotype_scan_ms": round(t_hap * 1e3, 3), "cluster_scan_ms": round(t_clu * 1e3, 3),
            "cluster_over_haplotype": round(t_clu / t_hap, 2), "haplotype_windows_per_s": round(len(wins) / t_hap, 1),
            "cluster_windows_per_s": round(len(wins) / t_clu, 1),
            "haplotype_kernel_ms": {"fingerprint": round(ker[0], 3), "classify": round(ker[1], 3), "verify_and_exact": round(ker[2], 3)},
            "haplotype_kernels_ms": round(sum(ker), 3), "chunks": int(chunks),
            "cluster_kernel_ms": {"gram": round(gram_ms, 3), "clustering": round(clus_ms, 3)},
            "mean_distinct_haplotypes": round(float(hap["n_distinct"].mean()), 2)}


def chunk_point(ctx, bm, nw, k):
    """a chunk per window: the median of 5 calls after one warm-up, and the chunks the timers counted in one call"""
    wins = impop_amd.make_windows(windows_of("tiling_50kb", min(k, nw)))
    t = passes(lambda: bm.haplotype_scan(wins, max_chunk_bytes=1))
    ctx.gram_timing(True)
    bm.haplotype_scan(wins, max_chunk_bytes=1)
    _, chunks = ctx.haplotype_elapsed()
    ctx.gram_timing(False)
    return {"windows": min(k, nw), "max_chunk_bytes": 1, "ms": round(t * 1e3, 3), "chunks": int(chunks)}


def trace_child(nw):
    ctx = impop_amd.Context(0)
    bm = ctx.synthetic(N_HAP, 50000 * nw, seed=SEED, keep_hap_major=False)
    for name in POINTS:
        sys.stderr.write(f"@@point {name}\n")
        sys.stderr.flush()
        bm.haplotype_scan(windows_of(name, nw))
        sys.stderr.write("@@end\n")
        sys.stderr.flush()
    bm.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--chunk-windows", type=int, default=256)
    ap.add_argument("--out")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(a.windows)
    ctx = impop_amd.Context(0)
    res = {"bench": "haplotype_scan", "device": ctx.device_name(), "n_hap": N_HAP, "passes": "median of 5 after 1 warm-up",
           "hbm_read_ceiling_TBps": 6.8}
    bm = ctx.synthetic(N_HAP, 50000 * a.windows, seed=SEED, keep_hap_major=True)
    for name in POINTS:
        res[name] = point(ctx, bm, name, a.windows)
    if a.chunk_windows > 0:
        res["one_window_chunks"] = chunk_point(ctx, bm, a.windows, a.chunk_windows)
    bm.free()
    ctx.close()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child", "--windows", str(a.windows)],
                       env=dict(os.environ, IMPOP_TRACE="1"), capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit("the trace run failed:\n" + r.stderr[-2000:])
    cur = None
    for line in r.stderr.splitlines():
        if line.startswith("@@point "):
            cur = line.split()[1]
        elif line.startswith("@@end"):
            cur = None
        elif line.startswith("[impop_haplotype_scan]") and cur:
            res[cur]["trace"] = line
            streamed = int(re.search(r"bytes_streamed=(\d+)", line).group(1))
            fp_ms = res[cur]["haplotype_kernel_ms"]["fingerprint"]
            res[cur]["bytes_streamed"] = streamed
            res[cur]["fingerprint_TBps"] = round(streamed / (fp_ms * 1e-3) / 1e12, 3) if fp_ms > 0 else None
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
