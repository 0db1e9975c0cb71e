#!/usr/bin/env python3
"""impop_diploid_scan at 465 haplotypes (232 pairs: haplotypes 2 i and 2 i + 1; one haplotype in no pair), from one process and
one run:

  tiling_50kb        4096 x 50 kb windows of one synthetic founder matrix
  sliding_10kb_5kb   10239 x 10 kb windows every 5 kb from the start of the same matrix
  one_window_chunks  the first --chunk-windows (256; 0: skip) windows of tiling_50kb with max_chunk_bytes=1: a chunk per window,
                     so the host's per-chunk path (metadata up, launches, records down, one synchronisation) is what is timed

Per point: the median of 5 timed calls after one warm-up call of BitMatrix.diploid_scan (min_run 50, the command line's default,
records only); from HIP events (impop_ctx_gram_timing) the time of its two kernels (tile / window) in one call; the mean
heterozygosity and F_ROH; and from the IMPOP_TRACE=1 line of one call, taken from a child process (the switch is read once per
process), the bytes the tile kernel streams — over that kernel's time, against the 6.8 TB/s read ceiling of
profiles/r01_hbm_read_ceiling.txt.
Next to it, in the same process, the route to the same `het` values that existed before: one impop_pairwise_counts per window
(het_i = a_h1 + a_h2 - 2 I_h1h2) on the first 64 windows of the tiling, from a 64-window cut of the same synthetic chromosome that
keeps its hap-major operand; its rows are compared with impop_diploid_scan's, and the ratio of the two times per window is formed.
One JSON line on stdout; --out FILE also writes it there (the recorded run: profiles/r11_diploid_scan.json).  --windows N scales
the points down for a rehearsal."""
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

N_HAP, SEED, MIN_RUN, LOOP_WINDOWS = 465, 1, 50, 64
PAIRS = [(2 * i, 2 * i + 1) for i in range(N_HAP // 2)]
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
    rec = bm.diploid_scan(wins, PAIRS, MIN_RUN)
    t = passes(lambda: bm.diploid_scan(wins, PAIRS, MIN_RUN))
    ctx.gram_timing(True)
    bm.diploid_scan(wins, PAIRS, MIN_RUN)
    ker, chunks = ctx.diploid_elapsed()
    ctx.gram_timing(False)
    total = sum(ker)
    return {"windows": len(wins), "diploid_scan_ms": round(t * 1e3, 3), "ms_per_4096_windows": round(t * 1e3 * 4096 / len(wins), 3),
            "windows_per_s": round(len(wins) / t, 1), "kernel_ms": {"tile": round(ker[0], 3), "window": round(ker[1], 3)},
            "kernel_share": {"tile": round(ker[0] / total, 4), "window": round(ker[1] / total, 4)} if total > 0 else None,
            "kernels_ms": round(total, 3), "chunks": int(chunks), "mean_ho": float(rec["ho"].mean()), "mean_he": float(rec["he"].mean()),
            "mean_f_roh": round(float(rec["f_roh"].mean()), 6), "mean_het_sites": round(float(rec["het_sites"].mean()), 2)}


def gram_loop(ctx, nw, dip_ms_per_window):
    """today's route to het: one Gram per window"""
    k = min(LOOP_WINDOWS, nw)
    wins = windows_of("tiling_50kb", k)
    bm = ctx.synthetic(N_HAP, 50000 * k, seed=SEED, keep_hap_major=True)
    h1 = np.array([p[0] for p in PAIRS])
    h2 = np.array([p[1] for p in PAIRS])

    def loop():
        out = np.zeros((k, len(PAIRS)), dtype=np.int64)
        for j, (b, e, _) in enumerate(wins):
            I = bm.pairwise_counts(b, e).astype(np.int64)
            out[j] = I[h1, h1] + I[h2, h2] - 2 * I[h1, h2]
        return out

    het = loop()
    t = passes(loop)
    _, ind = bm.diploid_scan(wins, PAIRS, MIN_RUN, want_individuals=True)
    same = bool(np.array_equal(ind["het"].astype(np.int64), het))
    bm.free()
    ms_per_window = t * 1e3 / k
    return {"windows": k, "pairwise_counts_loop_ms": round(t * 1e3, 3), "ms_per_window": round(ms_per_window, 4),
            "ms_per_4096_windows": round(ms_per_window * 4096, 1), "het_equal": same,
            "ratio_to_diploid_scan": round(ms_per_window / dip_ms_per_window, 1) if dip_ms_per_window > 0 else None}


def chunk_point(ctx, bm, nw, k):
    """a chunk per window: the median of 5 calls after one warm-up, and the chunks the timers counted in one call"""
    wins = impop_amd.make_windows(windows_of("tiling_50kb", min(k, nw)))
    t = passes(lambda: bm.diploid_scan(wins, PAIRS, MIN_RUN, max_chunk_bytes=1))
    ctx.gram_timing(True)
    bm.diploid_scan(wins, PAIRS, MIN_RUN, max_chunk_bytes=1)
    _, chunks = ctx.diploid_elapsed()
    ctx.gram_timing(False)
    return {"windows": min(k, nw), "max_chunk_bytes": 1, "ms": round(t * 1e3, 3), "chunks": int(chunks)}


def trace_child(nw):
    ctx = impop_amd.Context(0)
    bm = ctx.synthetic(N_HAP, 50000 * nw, seed=SEED, keep_hap_major=False)
    for name in POINTS:
        sys.stderr.write(f"@@point {name}\n")
        sys.stderr.flush()
        bm.diploid_scan(windows_of(name, nw), PAIRS, MIN_RUN)
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
    res = {"bench": "diploid_scan", "device": ctx.device_name(), "n_hap": N_HAP, "n_ind": len(PAIRS), "min_run": MIN_RUN,
           "passes": "median of 5 after 1 warm-up", "hbm_read_ceiling_TBps": 6.8}
    bm = ctx.synthetic(N_HAP, 50000 * a.windows, seed=SEED, keep_hap_major=False)
    for name in POINTS:
        res[name] = point(ctx, bm, name, a.windows)
    if a.chunk_windows > 0:
        res["one_window_chunks"] = chunk_point(ctx, bm, a.windows, a.chunk_windows)
    bm.free()
    res["gram_loop_50kb"] = gram_loop(ctx, a.windows, res["tiling_50kb"]["diploid_scan_ms"] / res["tiling_50kb"]["windows"])
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
        elif line.startswith("[impop_diploid_scan]") and cur:
            res[cur]["trace"] = line
            streamed = int(re.search(r"bytes_streamed=(\d+)", line).group(1))
            tile_ms = res[cur]["kernel_ms"]["tile"]
            res[cur]["bytes_streamed"] = streamed
            res[cur]["tile_TBps"] = round(streamed / (tile_ms * 1e-3) / 1e12, 3) if tile_ms > 0 else None
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
