#!/usr/bin/env python3
"""impop_ehh_scan next to the per-window path on the same windows, from one process and one run:

  tiling_50kb        256 x 50 kb windows of one synthetic founder matrix of 465 haplotypes, the core in the middle of each
  sliding_10kb_5kb   as many 10 kb windows every 5 kb from the start of the same matrix (overlapping windows), central cores
  one_window_chunks  the first --chunk-windows (256; 0: skip) windows of tiling_50kb with max_chunk_bytes=1: a chunk per window,
                     so the host's per-chunk path (metadata up, launches, records down, one synchronisation) is what is timed

Per point, on the same windows and cores (flanks = reference, ehhgfa.py:56-61):
  scan   one BitMatrix.ehh_scan call
  loop   four BitMatrix.ehh calls per window (allele 0 / 1 x backwards / forwards over the right flank) with the member
         masks of every window prepared beforehand — what ehh.scan_windows costs per window without its host work
each the median of 5 passes after one warm-up pass, plus the scan's kernel time from HIP events (impop_ctx_ehh_elapsed) and
its IMPOP_TRACE=1 line, taken from a child process (the switch is read once per process).  The records of the scan are checked
against the loop's vectors (sum of rint(1000 * EHH)) on every window before anything is timed.
One JSON line on stdout; --out FILE also writes it there.  --windows N scales the points down for a rehearsal."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import impop_amd  # noqa: E402

N_HAP, SEED = 465, 1


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
        wins = [(k * 50000, (k + 1) * 50000) for k in range(nw)]
    else:
        wins = [(s, s + 10000) for s in range(0, nw * 5000, 5000)]
    return wins, [b + (e - b) // 2 for b, e in wins]


def matrix(ctx, nw):
    return ctx.synthetic(N_HAP, 50000 * nw, seed=SEED)


def point(ctx, bm, name, nw):
    wins, cores = windows_of(name, nw)
    masks = []
    for c in cores:  # the core column of every window, as member flags per allele
        col = impop_amd.unpack_hap_major(bm.download(c, c + 1), 1)[:, 0]
        masks.append([(col == a).astype(np.uint8) for a in (0, 1)])

    def loop():
        out = []
        for (b, e), c, mk in zip(wins, cores, masks):
            out.append([[bm.ehh(c + 1, e, mk[a], reverse=(h == 0)) for h in (0, 1)] for a in (0, 1)])
        return out

    rec = bm.ehh_scan(wins, cores)
    for r, vecs, mk in zip(rec, loop(), masks):
        for a in (0, 1):
            for h in (0, 1):
                want = int(np.rint(1000.0 * vecs[a][h]).astype(np.int64).sum()) if mk[a].any() else 0
                assert int(r["area_milli"][a][h]) == want, "the scan and the per-window kernel disagree"
    t_scan = passes(lambda: bm.ehh_scan(wins, cores))
    t_loop = passes(loop)
    ctx.gram_timing(True)
    bm.ehh_scan(wins, cores)
    kernel_ms, chunks = ctx.ehh_elapsed()
    ctx.gram_timing(False)
    minor = np.minimum(rec["n_members"][:, 0], rec["n_members"][:, 1])
    return {"windows": len(wins), "scan_ms": round(t_scan * 1e3, 3), "loop_ms": round(t_loop * 1e3, 3),
            "speedup": round(t_loop / t_scan, 1), "scan_windows_per_s": round(len(wins) / t_scan, 1),
            "loop_windows_per_s": round(len(wins) / t_loop, 1), "scan_kernel_ms": round(kernel_ms, 3), "chunks": int(chunks),
            "windows_with_both_alleles": int((minor > 0).sum()), "minor_allele_members_mean": round(float(minor.mean()), 1)}


def chunk_point(ctx, bm, nw, k):
    """a chunk per window: the median of 5 calls after one warm-up, and the chunks the timers counted in one call"""
    wins, cores = windows_of("tiling_50kb", min(k, nw))
    t = passes(lambda: bm.ehh_scan(wins, cores, max_chunk_bytes=1))
    ctx.gram_timing(True)
    bm.ehh_scan(wins, cores, max_chunk_bytes=1)
    _, chunks = ctx.ehh_elapsed()
    ctx.gram_timing(False)
    return {"windows": min(k, nw), "max_chunk_bytes": 1, "ms": round(t * 1e3, 3), "chunks": int(chunks)}


def trace_child(nw):
    ctx = impop_amd.Context(0)
    bm = matrix(ctx, nw)
    for name in ("tiling_50kb", "sliding_10kb_5kb"):
        sys.stderr.write(f"@@point {name}\n")
        sys.stderr.flush()
        bm.ehh_scan(*windows_of(name, nw))
    bm.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--chunk-windows", type=int, default=256)
    ap.add_argument("--out")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(a.windows)
    ctx = impop_amd.Context(0)
    res = {"bench": "ehh_scan", "device": ctx.device_name(), "n_hap": N_HAP, "flanks": "reference", "passes": "median of 5 after 1 warm-up"}
    bm = matrix(ctx, a.windows)
    for name in ("tiling_50kb", "sliding_10kb_5kb"):
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
        elif line.startswith("[impop_ehh_scan]") and cur:
            res[cur].setdefault("trace", []).append(line)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
