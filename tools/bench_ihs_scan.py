#!/usr/bin/env python3
"""impop_ihs_scan on the compacted synthetic bench chromosome (bench.py's: 465 haplotypes, 4854 x 50 kb, seed 20251031), every
site with a minor-allele frequency of at least 5 % as a core, default limits (cutoff 0.05, 1 Mb, 100 sites):

  count        the call with no room for records: classification, prefix and the count alone
  scan         the call with room: the same plus tables, the PBWT walk and the records down; cores per second from this
  kernels      HIP-event time of [classification + prefix + tables, walk] in one scan call (impop_ctx_ihs_elapsed)
  ehh_scan     (--sample 0: skipped) a sample of --sample (4096) of the same cores, evenly spaced, through impop_ehh_scan TWO_SIDED on the full matrix
               with windows of core +- 1 Mb (it has no cutoff and refuses compacted matrices), and its cores per second
  trace        the IMPOP_TRACE=1 line of one scan call, from a child process (the switch is read once per process)

scan and count are the median of --steps (3) calls after one warm-up call; ehh_scan is one call after one warm-up call on a
tenth of the sample.  The sample's records are compared where the two definitions meet: the class sizes at the core.
One JSON line on stdout; --out FILE also writes it there.  --windows N scales the chromosome down for a rehearsal.
Nothing here is attributed by a counter run: the figures are wall-clock and event times."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import impop_amd  # noqa: E402

N_HAP, SEED, WINDOW = 465, 20251031, 50000
PARAMS = dict(min_mac=math.ceil(0.05 * N_HAP), cutoff_milli=50, max_extend_bp=1000000, max_extend_sites=100)


def timed(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def trace_child(n_windows):
    ctx = impop_amd.Context(0)
    bm = ctx.synthetic(N_HAP, WINDOW * n_windows, seed=SEED)
    cm = bm.compact()
    bm.free()
    _, total = cm.ihs_scan(**PARAMS)
    cm.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4854)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--out")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(a.windows)
    ctx = impop_amd.Context(0)
    n_site = WINDOW * a.windows
    bm = ctx.synthetic(N_HAP, n_site, seed=SEED)
    cm = bm.compact()
    res = {"bench": "ihs_scan", "device": ctx.device_name(), "n_hap": N_HAP, "sites": n_site, "kept_sites": int(cm.n_site), "params": PARAMS,
           "chunk_blocks_env": os.environ.get("IMPOP_IHS_CHUNK_BLOCKS"), "passes": f"median of {a.steps} after 1 warm-up"}
    _, total = cm.ihs_scan(capacity=0, **PARAMS)
    res["cores"] = total
    t_count = timed(lambda: cm.ihs_scan(capacity=0, **PARAMS), 0, a.steps)
    rec = [None]

    def scan():
        rec[0] = cm.ihs_scan(capacity=total, **PARAMS)[0]

    t_scan = timed(scan, 1, a.steps)
    ctx.gram_timing(True)
    scan()
    kernel_ms, _ = ctx.ihs_elapsed()
    ctx.gram_timing(False)
    rec = rec[0]
    res.update({"count_ms": round(t_count * 1e3, 3), "scan_ms": round(t_scan * 1e3, 3), "cores_per_s": round(total / t_scan, 1),
                "classify_kernel_ms": round(kernel_ms[0], 3), "walk_kernel_ms": round(kernel_ms[1], 3),
                "edge_share": round(float(((rec["flags"] & 0xFF) != 0).mean()), 4), "limit_share": round(float(((rec["flags"] & 0xFF00) != 0).mean()), 4)})
    cm.free()
    if a.sample > 0:  # the same cores through impop_ehh_scan, two-sided, windows of core +- 1 Mb
        pick = rec[np.linspace(0, total - 1, min(a.sample, total)).astype(np.int64)]
        cores = pick["site"].astype(np.int64)
        wins = np.stack([np.maximum(cores - PARAMS["max_extend_bp"], 0), np.minimum(cores + PARAMS["max_extend_bp"] + 1, n_site)], axis=1)
        bm.ehh_scan(wins[::10], cores[::10], flanks="two-sided")
        t0 = time.perf_counter()
        erec = bm.ehh_scan(wins, cores, flanks="two-sided")
        t_ehh = time.perf_counter() - t0
        assert np.array_equal(erec["n_members"], pick["n"]), "the two scans disagree on the class sizes at the cores"
        res["ehh_scan"] = {"cores": len(cores), "ms": round(t_ehh * 1e3, 3), "cores_per_s": round(len(cores) / t_ehh, 1)}
        res["cores_per_s_ratio"] = round((total / t_scan) / (len(cores) / t_ehh), 1)
    bm.free()
    ctx.close()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child", "--windows", str(a.windows)],
                       env=dict(os.environ, IMPOP_TRACE="1"), capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit("the trace run failed:\n" + r.stderr[-2000:])
    res["trace"] = [ln for ln in r.stderr.splitlines() if ln.startswith("[impop_ihs_scan]")]
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
