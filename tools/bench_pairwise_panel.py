#!/usr/bin/env python3
"""impop_pairwise_scan_panel next to the loop of impop_pairwise_scan calls it replaces, from one process and one run:

  tiling_50kb        4096 x 50 kb windows of one synthetic founder matrix of 465 haplotypes
  sliding_10kb_5kb   10239 x 10 kb windows every 5 kb from the start of the same matrix (overlapping windows: shared segment matrices)

Five disjoint panels of 140 / 88 / 100 / 60 / 72 haplotypes (5 in none), `match`, -t 0.999 -r 5 (run_tajd_panels.sh,
run_h_fst_panels.sh).  Per point, on the same windows:
  panel  one BitMatrix.pairwise_scan_panel call (s_scope 0)
  loop   five pairwise_scan(mask_p = panel, s_scope 0) + ten pairwise_scan(mask_a, mask_b, s_scope 2): the per-panel and
         per-pair runs of the two panel drivers — fifteen Gram passes where the panel call makes one
each the median of 5 timed calls after 3 warm-up calls, plus, from HIP events (impop_ctx_gram_timing), the Gram-kernel time of
one call of each leg and the time of the panel call's Fst kernel, and the IMPOP_TRACE=1 lines of one panel call, taken from a
child process (the switch is read once per process).  The panel call's records are checked against the loop's before anything
is timed: panels byte for byte, pairs to 1e-9 relative (floors of INTEGRATION.md §4 for Fst / Da).
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

N_HAP, SEED, SIZES = 465, 1, (140, 88, 100, 60, 72)
KW = dict(kind="match", threshold=0.999, round_digits=5)


def passes(fn, warmup=3, steps=5):
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
    return [(5000 * k, 5000 * k + 10000, 10000) for k in range(max(nw * 10239 // 4096, 1))]  # 10239 at the default: two chunks


def panels():
    perm = np.random.default_rng(SEED).permutation(N_HAP)
    pops, o = [], 0
    for s in SIZES:
        f = np.zeros(N_HAP, np.uint8)
        f[perm[o: o + s]] = 1
        o += s
        pops.append(f)
    return pops


def loop(bm, wins, pops):
    one = [bm.pairwise_scan(wins, p, None, None, s_scope=0, **KW) for p in pops]
    two = [bm.pairwise_scan(wins, None, pops[k], pops[l], s_scope=2, **KW) for k in range(len(pops)) for l in range(k + 1, len(pops))]
    return one, two


def close(key, a, b, dxy):
    floor = 1e-12 if key == "fst" else 1e-12 * np.abs(dxy) if key == "da" else 0.0
    return bool((np.abs(a - b) <= np.maximum(1e-9 * np.maximum(np.abs(a), np.abs(b)), floor)).all())


def point(ctx, bm, name, nw):
    wins, pops = windows_of(name, nw), panels()
    pan, pairs, _ = bm.pairwise_scan_panel(wins, pops, **KW)
    one, two = loop(bm, wins, pops)
    for k, r in enumerate(one):
        for key in ("pi", "pi_site", "tajima_d", "n_groups"):
            assert pan[:, k][key].tobytes() == r[key].tobytes(), ("panel", k, key)
    for p, r in enumerate(two):
        for key in ("fst", "pi_a", "pi_b", "pi_xy", "dxy", "da"):
            assert close(key, pairs[:, p][key], r[key], r["dxy"]), ("pair", p, key)
    t_panel = passes(lambda: bm.pairwise_scan_panel(wins, pops, **KW))
    t_loop = passes(lambda: loop(bm, wins, pops))
    ctx.gram_timing(True)
    bm.pairwise_scan_panel(wins, pops, **KW)
    gram_panel, launches = ctx.gram_elapsed()
    fst_ms, chunks = ctx.cluster_elapsed()
    ctx.gram_timing(False)
    ctx.gram_timing(True)
    loop(bm, wins, pops)
    gram_loop, launches_loop = ctx.gram_elapsed()
    ctx.gram_timing(False)
    return {"windows": len(wins), "panel_ms": round(t_panel * 1e3, 3), "loop_ms": round(t_loop * 1e3, 3), "loop_over_panel": round(t_loop / t_panel, 2),
            "panel_windows_per_s": round(len(wins) / t_panel, 1), "gram_kernel_ms_panel": round(gram_panel, 3), "gram_launches_panel": int(launches),
            "gram_kernel_ms_loop": round(gram_loop, 3), "gram_launches_loop": int(launches_loop), "gram_loop_over_panel": round(gram_loop / gram_panel, 2),
            "panel_fst_kernel_ms": round(fst_ms, 3), "chunks": int(chunks),
            "panel_fst_kernel_ms_per_4096_windows": round(fst_ms * 4096 / len(wins), 3)}


def trace_child(nw):
    ctx = impop_amd.Context(0)
    bm = ctx.synthetic(N_HAP, 50000 * nw, seed=SEED, keep_hap_major=True)
    pops = panels()
    for name in ("tiling_50kb", "sliding_10kb_5kb"):
        wins = windows_of(name, nw)
        bm.pairwise_scan_panel(wins, pops, **KW)  # (the first call builds the site bitmap)
        sys.stderr.write(f"@@point {name}\n")
        sys.stderr.flush()
        bm.pairwise_scan_panel(wins, pops, **KW)
        sys.stderr.write("@@end\n")
        sys.stderr.flush()
    bm.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--out")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(a.windows)
    ctx = impop_amd.Context(0)
    res = {"bench": "pairwise_panel", "device": ctx.device_name(), "n_hap": N_HAP, "panels": list(SIZES), "params": "match -t 0.999 -r 5",
           "passes": "median of 5 after 3 warm-up"}
    bm = ctx.synthetic(N_HAP, 50000 * a.windows, seed=SEED, keep_hap_major=True)
    for name in ("tiling_50kb", "sliding_10kb_5kb"):
        res[name] = point(ctx, bm, name, a.windows)
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
        elif line.startswith("[impop_") and cur:
            res[cur].setdefault("trace", []).append(line)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
