#!/usr/bin/env python3
"""impop_sfs_scan on the synthetic 465-haplotype bench matrix, 4096 x 50 kb windows, the five populations tools/bench_multi.py uses
at K = 5 (93 haplotypes each), from one process and one run:

  (a) the summary pass alone (no pair, no table) against impop_scan_multi for the same populations on the same windows: the same
      index bytes streamed, so (a) / (b) is what the spectrum's per-site arithmetic costs over the first two moments; and the
      summary pass with one pair and with all ten pairs (one and three launch groups)
  (b) the 1-D table pass on the DENSE matrix (uploaded without the scan index) against one impop_afs call per population on that
      same matrix, the 1-D table pass on the default (indexed) route, and the joint table of one pair on the default route (no
      earlier path to compare with)

Per point the median of 10 timed calls after 2 warm-up calls (wall clock around the call, which ends in a synchronise), and the
summed time of the summary / table launches from HIP events (impop_ctx_gram_timing) in one more call; from the IMPOP_TRACE=1 line
of a child process the bytes the two passes stream.  impop_scan_multi and impop_afs have no event bracket, so the ratios are
formed from wall times.  One JSON line on stdout; --out FILE also writes it there (the recorded run:
profiles/r19_sfs_scan.json).  --windows N scales the points down for a rehearsal; --commit HASH is recorded with the numbers."""
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

N_HAP, SEED, WINDOW, K = 465, 20251031, 50000, 5


def flags(lo, hi):
    f = np.zeros(N_HAP, dtype=np.uint8)
    f[lo:hi] = 1
    return f


POPS = [flags((N_HAP // K) * k, (N_HAP // K) * (k + 1)) for k in range(K)]
PAIRS10 = [(a, b) for a in range(K) for b in range(a + 1, K)]
# name -> (dense matrix, pairs, tables)
POINTS = {
    "summary": (False, [], ()),
    "summary_1pair": (False, PAIRS10[:1], ()),
    "summary_10pairs": (False, PAIRS10, ()),
    "sfs_dense": (True, [], ("sfs",)),
    "sfs_indexed": (False, [], ("sfs",)),
    "jsfs_1pair_indexed": (False, PAIRS10[:1], ("jsfs",)),
}


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


def sfs_point(ctx, bm, wins, pairs, tables):
    call = lambda: bm.sfs_scan(wins, POPS, pairs, tables=tables)  # noqa: E731
    st, pr, sfs, jsfs = call()
    t = passes(call)
    ctx.gram_timing(True)
    call()
    ker, launches = ctx.sfs_elapsed()
    ctx.gram_timing(False)
    out = {"windows": len(wins), "pairs": len(pairs), "tables": list(tables), "sfs_scan_ms": round(t * 1e3, 3),
           "windows_per_s": round(len(wins) / t, 1), "summary_kernel_ms": round(ker[0], 3), "summary_launches": int(launches),
           "table_kernel_ms": round(ker[1], 3), "mean_seg": float(st["seg"].mean()), "mean_tajima_d": float(np.nanmean(st["tajima_d"]))}
    if sfs is not None:
        out["sfs_sites"] = int(sum(int(t_.sum()) for t_ in sfs))
    if jsfs is not None:
        out["jsfs_sites"] = int(sum(int(t_.sum()) for t_ in jsfs))
    return out, (st, pr, sfs, jsfs)


def trace_child(nw):
    ctx = impop_amd.Context(0)
    wins = windows_of(nw)
    for dense in (False, True):
        bm = ctx.synthetic(N_HAP, WINDOW * nw, seed=SEED, keep_hap_major=False, dense_scan=dense)
        for name, (d, pairs, tables) in POINTS.items():
            if d != dense:
                continue
            sys.stderr.write(f"@@point {name}\n")
            sys.stderr.flush()
            bm.sfs_scan(wins, POPS, pairs, tables=tables)
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
    res = {"bench": "sfs_scan", "commit": a.commit, "device": ctx.device_name(), "n_hap": N_HAP, "window_sites": WINDOW, "populations": K,
           "pair_group": impop_amd._lib.SFS_PAIR_GROUP, "passes": "median of 10 after 2 warm-up", "hbm_read_ceiling_TBps": 6.8}
    wins = windows_of(a.windows)
    keep = {}
    for dense in (False, True):
        bm = ctx.synthetic(N_HAP, WINDOW * a.windows, seed=SEED, keep_hap_major=False, dense_scan=dense)
        for name, (d, pairs, tables) in POINTS.items():
            if d == dense:
                res[name], keep[name] = sfs_point(ctx, bm, wins, pairs, tables)
        if not dense:
            t_multi = passes(lambda: bm.scan_multi(wins, POPS))
            res["scan_multi_k5"] = {"windows": len(wins), "scan_multi_ms": round(t_multi * 1e3, 3)}
        else:  # one impop_afs call per population on the same dense matrix; its bins 1 .. n - 1 are the spectrum's
            afs = [bm.afs(wins, p) for p in POPS]
            t_afs = passes(lambda: [bm.afs(wins, p) for p in POPS])
            same = all(np.array_equal(x[:, 1:-1], y[:, 1:-1]) for x, y in zip(afs, keep["sfs_dense"][2]))
            res["afs_per_population_dense"] = {"windows": len(wins), "calls": K, "ms": round(t_afs * 1e3, 3), "bins_equal": bool(same)}
        bm.free()
    ctx.close()
    res["tables_equal_dense_vs_indexed"] = bool(all(np.array_equal(x, y) for x, y in zip(keep["sfs_dense"][2], keep["sfs_indexed"][2])))
    res["records_equal_dense_vs_indexed"] = bool(keep["sfs_dense"][0].tobytes() == keep["sfs_indexed"][0].tobytes())
    res["a_over_b"] = round(res["summary"]["sfs_scan_ms"] / res["scan_multi_k5"]["scan_multi_ms"], 3)
    res["afs_over_sfs_dense"] = round(res["afs_per_population_dense"]["ms"] / res["sfs_dense"]["sfs_scan_ms"], 3)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child", "--windows", str(a.windows)],
                       env=dict(os.environ, IMPOP_TRACE="1"), capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit("the trace run failed:\n" + r.stderr[-2000:])
    cur = None
    for line in r.stderr.splitlines():
        if line.startswith("@@point "):
            cur = line.split()[1]
        elif line.startswith("@@end"):
            cur = None
        elif line.startswith("[impop_sfs_scan]") and cur:
            p = res[cur]
            p["trace"] = line
            streamed = int(re.search(r" bytes_streamed=(\d+)", line).group(1))
            table = int(re.search(r"table_bytes_streamed=(\d+)", line).group(1))
            if p["summary_kernel_ms"] > 0:
                p["summary_TBps"] = round(streamed * p["summary_launches"] / (p["summary_kernel_ms"] * 1e-3) / 1e12, 3)
            if p["table_kernel_ms"] > 0:
                p["table_TBps"] = round(table / (p["table_kernel_ms"] * 1e-3) / 1e12, 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
