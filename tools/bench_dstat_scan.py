#!/usr/bin/env python3
"""impop_dstat_scan on the synthetic 465-haplotype bench matrix, 4096 x 50 kb windows, from one process and one run:

  (a) dstat_scan, one quartet of four populations (116 haplotypes each, one haplotype in none)
  (b) impop_scan_multi for the same four populations on the same windows: the same index bytes streamed, first and second
      moments only, so (a) / (b) is what the wider per-site arithmetic costs
  (c) the route there was before: four impop_site_counts calls plus the numpy evaluation of the same five integers, on the
      first 256 windows in chunks of 64 (the full range would hold 3.3 GB of counts on the host), scaled to 4096 windows; its
      integers are compared with (a)'s
  and dstat_scan with 3 quartets of the four populations and 15 quartets of five (93 haplotypes each): one and five launch groups.

Per point the median of 10 timed calls after 2 warm-up calls (wall clock around the call), for dstat_scan also the summed time of
its streaming launches from HIP events (impop_ctx_gram_timing) in one call and, from the IMPOP_TRACE=1 line of a child process, the
bytes those launches stream.  impop_scan_multi has no event bracket, so (a) / (b) is formed from the wall times of the two calls.
One JSON line on stdout; --out FILE also writes it there (the recorded run: profiles/r13_dstat_scan.json).  --windows N scales the
points down for a rehearsal; --commit HASH is recorded with the numbers."""
import argparse
import itertools
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

N_HAP, SEED, WINDOW, LOOP_WINDOWS, LOOP_CHUNK = 465, 20251031, 50000, 256, 64


def flags(lo, hi):
    f = np.zeros(N_HAP, dtype=np.uint8)
    f[lo:hi] = 1
    return f


POPS4 = [flags(116 * k, 116 * (k + 1)) for k in range(4)]
POPS5 = [flags(93 * k, 93 * (k + 1)) for k in range(5)]
Q1 = [(0, 1, 2, 3)]
Q3 = [(0, 1, 2, 3), (1, 0, 2, 3), (2, 3, 0, 1)]
Q15 = [q for s in itertools.combinations(range(5), 4) for q in ((s[0], s[1], s[2], s[3]), (s[0], s[2], s[1], s[3]), (s[1], s[2], s[0], s[3]))]
POINTS = {"q1_k4": (POPS4, Q1), "q3_k4": (POPS4, Q3), "q15_k5": (POPS5, Q15)}


def passes(fn, warmup=2, steps=10):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def windows_of(nw):
    return impop_amd.make_windows([(k * WINDOW, (k + 1) * WINDOW, WINDOW) for k in range(nw)])


def dstat_point(ctx, bm, wins, pops, quartets):
    rec = bm.dstat_scan(wins, pops, quartets)
    t = passes(lambda: bm.dstat_scan(wins, pops, quartets))
    ctx.gram_timing(True)
    bm.dstat_scan(wins, pops, quartets)
    ker, launches = ctx.dstat_elapsed()
    ctx.gram_timing(False)
    inf = (rec["abba"] + rec["baba"]) > 0
    return {"windows": len(wins), "populations": len(pops), "quartets": len(quartets), "dstat_scan_ms": round(t * 1e3, 3),
            "windows_per_s": round(len(wins) / t, 1), "streaming_ms": round(ker, 3), "streaming_launches": int(launches),
            "informative_records": int(inf.sum()), "mean_d": float(np.nanmean(rec["d"])) if inf.any() else None}, rec


def site_counts_route(bm, nw, rec):
    """four impop_site_counts calls per chunk and the five integers per window in numpy"""
    k = min(LOOP_WINDOWS, nw)
    n = [int(p.sum()) for p in POPS4]

    def loop():
        out = np.zeros((k, 5), dtype=np.int64)
        for w0 in range(0, k, LOOP_CHUNK):
            w1 = min(k, w0 + LOOP_CHUNK)
            c1, c2, c3, cO = (bm.site_counts(w0 * WINDOW, w1 * WINDOW, p).astype(np.int64).reshape(w1 - w0, WINDOW) for p in POPS4)
            rO = n[3] - cO
            p2 = c2 * n[2] >= c3 * n[1]
            out[w0:w1, 0] = ((n[0] - c1) * c2 * c3 * rO).sum(axis=1)
            out[w0:w1, 1] = (c1 * (n[1] - c2) * c3 * rO).sum(axis=1)
            out[w0:w1, 2] = ((c1 * n[1] - c2 * n[0]) * (c3 * n[3] - cO * n[2])).sum(axis=1)
            out[w0:w1, 3] = np.where(p2, (c2 * n[0] - c1 * n[1]) * c2 * rO, 0).sum(axis=1)
            out[w0:w1, 4] = np.where(p2, 0, (c3 * n[0] - c1 * n[2]) * c3 * rO).sum(axis=1)
        return out

    got = loop()
    t = passes(loop)
    same = all(np.array_equal(got[:, j], rec[name][:k, 0]) for j, name in enumerate(("abba", "baba", "f4_num", "fd_den_p2", "fd_den_p3")))
    return {"windows": k, "ms": round(t * 1e3, 3), "ms_per_4096_windows": round(t * 1e3 * 4096 / k, 1), "integers_equal": bool(same)}


def trace_child(nw):
    ctx = impop_amd.Context(0)
    bm = ctx.synthetic(N_HAP, WINDOW * nw, seed=SEED, keep_hap_major=False)
    wins = windows_of(nw)
    for name, (pops, quartets) in POINTS.items():
        sys.stderr.write(f"@@point {name}\n")
        sys.stderr.flush()
        bm.dstat_scan(wins, pops, quartets)
        sys.stderr.write("@@end\n")
        sys.stderr.flush()
    bm.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--out")
    ap.add_argument("--commit", default="")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(a.windows)
    ctx = impop_amd.Context(0)
    res = {"bench": "dstat_scan", "commit": a.commit, "device": ctx.device_name(), "n_hap": N_HAP, "window_sites": WINDOW,
           "group_size": impop_amd._lib.DSTAT_GROUP, "passes": "median of 10 after 2 warm-up", "hbm_read_ceiling_TBps": 6.8}
    bm = ctx.synthetic(N_HAP, WINDOW * a.windows, seed=SEED, keep_hap_major=False)
    wins = windows_of(a.windows)
    recs = {}
    for name, (pops, quartets) in POINTS.items():
        res[name], recs[name] = dstat_point(ctx, bm, wins, pops, quartets)
    t_multi = passes(lambda: bm.scan_multi(wins, POPS4))
    res["scan_multi_k4"] = {"windows": len(wins), "scan_multi_ms": round(t_multi * 1e3, 3)}
    res["site_counts_route"] = site_counts_route(bm, a.windows, recs["q1_k4"])
    bm.free()
    ctx.close()
    a_ms = res["q1_k4"]["dstat_scan_ms"]
    res["a_ms"] = a_ms
    res["a_over_b"] = round(a_ms / res["scan_multi_k4"]["scan_multi_ms"], 3)
    res["c_over_a"] = round(res["site_counts_route"]["ms_per_4096_windows"] * len(wins) / 4096 / a_ms, 1)
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
        elif line.startswith("[impop_dstat_scan]") and cur:
            res[cur]["trace"] = line
            streamed = int(re.search(r"bytes_streamed=(\d+)", line).group(1))
            ms, launches = res[cur]["streaming_ms"], res[cur]["streaming_launches"]
            res[cur]["bytes_streamed_per_launch"] = streamed
            res[cur]["streaming_TBps"] = round(streamed * launches / (ms * 1e-3) / 1e12, 3) if ms > 0 else None
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
