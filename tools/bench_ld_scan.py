#!/usr/bin/env python3
"""impop_ld_scan at 465 haplotypes, from one process and one run:

  tiling_50kb        4096 x 50 kb windows of one synthetic founder matrix
  sliding_10kb_5kb   10239 x 10 kb windows every 5 kb from the start of the same matrix
  one_window_chunks  the first --chunk-windows (256; 0: skip) windows of tiling_50kb with max_chunk_bytes=1: a chunk per window,
                     so the host's per-chunk path (metadata up, launches, records down, one synchronisation) is what is timed

Per point: the median of 5 timed calls after one warm-up call of BitMatrix.ld_scan (min_mac = ceil(0.05 x 465) = 24, max_sites
512, the command line's defaults); from HIP events (impop_ctx_gram_timing) the time of its three kernel groups (select / gather /
pairs) in one call; the mean qualifying and used sites per window and the site pairs evaluated per second; and from the
IMPOP_TRACE=1 line of one call, taken from a child process (the switch is read once per process), the bytes the select kernel
streams — over that kernel's time, against the 6.8 TB/s read ceiling of profiles/r01_hbm_read_ceiling.txt.  Nothing comparable
exists to set it against, so no ratio is formed.
One JSON line on stdout; --out FILE also writes it there (the recorded run: profiles/r10_ld_scan.json).  --windows N scales the
points down for a rehearsal."""
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
LD_KW = dict(min_mac=24, max_sites=512)
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
    rec = bm.ld_scan(wins, **LD_KW)
    t = passes(lambda: bm.ld_scan(wins, **LD_KW))
    ctx.gram_timing(True)
    bm.ld_scan(wins, **LD_KW)
    ker, chunks = ctx.ld_elapsed()
    ctx.gram_timing(False)
    used = rec["n_used"].astype(np.int64)
    pairs = int((used * (used - 1) // 2).sum())
    return {"windows": len(wins), "ld_scan_ms": round(t * 1e3, 3), "windows_per_s": round(len(wins) / t, 1),
            "kernel_ms": {"select": round(ker[0], 3), "gather": round(ker[1], 3), "pairs": round(ker[2], 3)},
            "kernels_ms": round(sum(ker), 3), "chunks": int(chunks),
            "mean_qualifying": round(float(rec["n_qualifying"].mean()), 2), "mean_used": round(float(used.mean()), 2),
            "site_pairs": pairs, "site_pairs_per_s": round(pairs / (ker[2] * 1e-3), 1) if ker[2] > 0 else None,
            "mean_zns": round(float(rec["zns"].mean()), 6)}


def chunk_point(ctx, bm, nw, k):
    """a chunk per window: the median of 5 calls after one warm-up, and the chunks the timers counted in one call"""
    wins = impop_amd.make_windows(windows_of("tiling_50kb", min(k, nw)))
    t = passes(lambda: bm.ld_scan(wins, max_chunk_bytes=1, **LD_KW))
    ctx.gram_timing(True)
    bm.ld_scan(wins, max_chunk_bytes=1, **LD_KW)
    _, chunks = ctx.ld_elapsed()
    ctx.gram_timing(False)
    return {"windows": min(k, nw), "max_chunk_bytes": 1, "ms": round(t * 1e3, 3), "chunks": int(chunks)}


def trace_child(nw):
    ctx = impop_amd.Context(0)
    bm = ctx.synthetic(N_HAP, 50000 * nw, seed=SEED, keep_hap_major=False)
    for name in POINTS:
        sys.stderr.write(f"@@point {name}\n")
        sys.stderr.flush()
        bm.ld_scan(windows_of(name, nw), **LD_KW)
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
    res = {"bench": "ld_scan", "device": ctx.device_name(), "n_hap": N_HAP, "passes": "median of 5 after 1 warm-up",
           "hbm_read_ceiling_TBps": 6.8, **LD_KW}
    bm = ctx.synthetic(N_HAP, 50000 * a.windows, seed=SEED, keep_hap_major=False)
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
        elif line.startswith("[impop_ld_scan]") and cur:
            res[cur]["trace"] = line
            streamed = int(re.search(r"bytes_streamed=(\d+)", line).group(1))
            sel_ms = res[cur]["kernel_ms"]["select"]
            res[cur]["bytes_streamed"] = streamed
            res[cur]["select_TBps"] = round(streamed / (sel_ms * 1e-3) / 1e12, 3) if sel_ms > 0 else None
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
