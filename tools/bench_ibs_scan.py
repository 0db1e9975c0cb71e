#!/usr/bin/env python3
"""impop_ibs_scan at 465 haplotypes, from one process and one run, on two matrices cut from the synthetic bench chromosome:

  compact   the first --sites sites (default: all 242.7 M), compacted to their variable sites (coordinates through d_pos)
  dense     the first --dense-sites sites (default 12.8 M) as they are

Per matrix, the range = the whole matrix, and four points: all 107 880 pairs and the 232 diploid pairs (haplotypes 2 i and
2 i + 1), each with totals only (pair records, no list) and with the segment list (one call with room for it).  min_sites starts at
--min-sites and doubles until the all-pairs list holds at most --max-segments records; the value and the list lengths are recorded.
Per point: the median of 10 timed calls after 2 warm-up calls and their spread (max - min), the three kernel times of one call
from HIP events (impop_ctx_gram_timing: transpose / walk / combine + close), and from the IMPOP_TRACE=1 line of a child process
(the switch is read once per process) the bytes streamed.
Baseline, in the same process on the same matrices: what the library could do for the totals before this call — 465 rounds of
impop_diploid_scan with one window = the range, round-robin disjoint pairs (every pair of the 465 once); its rows of one round are
compared with impop_ibs_scan's.  Median of --loop-steps timed loops after one warm-up loop.
No counter run is made here: which of LDS, VALU or the stream bounds the walk kernel is NOT measured.
One JSON line on stdout; --out FILE also writes it there (the recorded run: profiles/r20_ibs_scan.json)."""
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

N_HAP, SEED = 465, 20251031
DIPLOID = [(2 * i, 2 * i + 1) for i in range(N_HAP // 2)]


def passes(fn, warmup=2, steps=10):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), max(ts) - min(ts)


def round_robin(n):
    """n odd: n rounds of (n - 1) / 2 disjoint pairs that cover every pair once (the circle method; one haplotype sits out)"""
    return [[((r + k) % n, (r - k) % n) for k in range(1, (n - 1) // 2 + 1)] for r in range(n)]


def matrices(ctx, sites, dense_sites):
    full = ctx.synthetic(N_HAP, sites, seed=SEED, keep_hap_major=False)
    cm = full.compact()
    full.free()
    return {"compact": cm, "dense": ctx.synthetic(N_HAP, dense_sites, seed=SEED, keep_hap_major=False)}


def point(ctx, bm, pairs, min_sites, want_list):
    kw = dict(pairs=pairs, min_sites=min_sites)
    rec, _, _, total = bm.ibs_scan(want_segments=False, **kw)
    if want_list:
        kw["seg_capacity"] = total
    else:
        kw["want_segments"] = False
    t, spread = passes(lambda: bm.ibs_scan(**kw))
    ctx.gram_timing(True)
    bm.ibs_scan(**kw)
    ker, chunks = ctx.ibs_elapsed()
    ctx.gram_timing(False)
    return {"pairs": len(rec), "segments": int(total), "ms": round(t * 1e3, 3), "spread_ms": round(spread * 1e3, 3),
            "kernel_ms": {"transpose": round(ker[0], 3), "walk": round(ker[1], 3), "combine_close": round(ker[2], 3)},
            "site_chunks": int(chunks), "mean_n_diff": round(float(rec["n_diff"].mean()), 2), "mean_longest": round(float(rec["longest"].mean()), 2)}


def baseline(bm, min_sites, rounds, steps, ibs_ms):
    span = getattr(bm, "compacted_from_sites", None) or bm.n_site
    win = [(0, int(span))]

    def loop():
        return [bm.diploid_scan(win, pr, min_sites, want_individuals=True)[1][0] for pr in rounds]

    rows = loop()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        loop()
        ts.append(time.perf_counter() - t0)
    t = statistics.median(ts)
    mine = bm.ibs_scan(pairs=rounds[7], min_sites=min_sites, want_segments=False)[0]
    same = bool(np.array_equal(mine["n_tracts"], rows[7]["roh_runs"]) and np.array_equal(mine["tract_sites"], rows[7]["roh_sites"])
                and np.array_equal(mine["longest"], rows[7]["longest_run"]) and np.array_equal(mine["n_diff"], rows[7]["het"]))
    return {"rounds": len(rounds), "pairs_per_round": len(rounds[0]), "loop_ms": round(t * 1e3, 3), "spread_ms": round((max(ts) - min(ts)) * 1e3, 3),
            "steps": steps, "rows_equal": same, "ratio_to_ibs_scan_totals": round(t * 1e3 / ibs_ms, 2) if ibs_ms > 0 else None}


def trace_child(a):
    ctx = impop_amd.Context(0)
    for name, bm in matrices(ctx, a.sites, a.dense_sites).items():
        for tag, pairs in (("all", None), ("diploid", DIPLOID)):
            for mode in ("totals", "list"):
                sys.stderr.write(f"@@point {name}.{tag}_{mode}\n")
                sys.stderr.flush()
                total = bm.ibs_scan(pairs=pairs, min_sites=a.min_sites, want_segments=False)[3] if mode == "list" else 0
                sys.stderr.write("@@go\n")
                sys.stderr.flush()
                bm.ibs_scan(pairs=pairs, min_sites=a.min_sites, **({"seg_capacity": total} if mode == "list" else {"want_segments": False}))
                sys.stderr.write("@@end\n")
                sys.stderr.flush()
        bm.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=50000 * 4854, help="sites of the chromosome that is compacted (default: the bench chromosome)")
    ap.add_argument("--dense-sites", type=int, default=50000 * 256, help="sites of the dense slab")
    ap.add_argument("--min-sites", type=int, default=64)
    ap.add_argument("--max-segments", type=int, default=12_000_000)
    ap.add_argument("--loop-steps", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(a)
    ctx = impop_amd.Context(0)
    res = {"bench": "ibs_scan", "device": ctx.device_name(), "n_hap": N_HAP, "passes": "median of 10 after 2 warm-up; spread = max - min",
           "not_measured": "no counter run: which of LDS, VALU or the stream bounds the walk kernel is unmeasured"}
    mats = matrices(ctx, a.sites, a.dense_sites)
    min_sites = a.min_sites
    while mats["compact"].ibs_scan(min_sites=min_sites, want_segments=False)[3] > a.max_segments:
        min_sites *= 2
    res["min_sites"] = min_sites
    rounds = round_robin(N_HAP)
    for name, bm in mats.items():
        r = {"sites": int(bm.n_site), "range_sites": int(getattr(bm, "compacted_from_sites", None) or bm.n_site)}
        for tag, pairs in (("all", None), ("diploid", DIPLOID)):
            for mode in ("totals", "list"):
                r[f"{tag}_{mode}"] = point(ctx, bm, pairs, min_sites, mode == "list")
        r["diploid_scan_loop"] = baseline(bm, min_sites, rounds, a.loop_steps, r["all_totals"]["ms"])
        res[name] = r
        bm.free()
    ctx.close()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child", "--sites", str(a.sites), "--dense-sites", str(a.dense_sites),
                        "--min-sites", str(min_sites)], env=dict(os.environ, IMPOP_TRACE="1"), capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit("the trace run failed:\n" + r.stderr[-2000:])
    cur, go = None, False
    for line in r.stderr.splitlines():
        if line.startswith("@@point "):
            cur, go = line.split()[1].split("."), False
        elif line.startswith("@@go"):
            go = True
        elif line.startswith("@@end"):
            cur = None
        elif line.startswith("[impop_ibs_scan]") and cur and go:
            p = res[cur[0]][cur[1]]
            p["trace"] = line
            p["bytes_streamed"] = int(re.search(r"bytes_streamed=(\d+)", line).group(1))
            walk = p["kernel_ms"]["walk"]
            p["streamed_TBps_over_kernels"] = round(p["bytes_streamed"] / (sum(p["kernel_ms"].values()) * 1e-3) / 1e12, 3) if walk > 0 else None
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
