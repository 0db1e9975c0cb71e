#!/usr/bin/env python3
"""impop_recomb_scan at 465 haplotypes, from one process and one run, min_mac 2:

  tiling_50kb        4096 x 50 kb windows of one synthetic founder matrix, no thinning (max_sites 4096)
  sliding_10kb_5kb   10239 x 10 kb windows every 5 kb from the start of the same matrix
  skewed             sliding_10kb_5kb with --arms (4) whole-chromosome-arm windows among them, max_sites 16384: a few windows
                     thinned to 16384 sites next to thousands that hold a few dozen
  dense_50kb         --dense-windows (256; 0: skip) x 50 kb windows of a second matrix whose founders differ at 0.9 % of the sites:
                     thousands of non-singleton sites per window, the pair kernel's own load

Per point: the median of 5 timed calls after one warm-up call of BitMatrix.recomb_scan; from HIP events (impop_ctx_gram_timing)
the time of its four kernel groups (select / gather / pairs / finish) in one call; the mean qualifying and used sites per window,
the site pairs tested per second of the pair kernel; from the IMPOP_TRACE=1 line of one call, taken from a child process (the
switch is read once per process), pair_tiles and the bytes the select kernel streams.  Two references per point, neither a target:
  ld_scan_ms         impop_ld_scan on the same windows at min_mac 2, max_sites 1024 (median of 5 after a warm-up), as a scale;
  numpy_ms_per_window  the plain numpy restatement (all pairs by one matrix product, then the per-site and per-window integers)
                     on --numpy-windows (3) windows spread over the list, rows downloaded from the device; its records must equal
                     the device's.  numpy_ms = that mean x the windows of the point, an extrapolation.
One JSON line on stdout; --out FILE also writes it there (the recorded run: profiles/r29_recomb_scan.json).  --windows N scales
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

N_HAP, SEED, MIN_MAC = 465, 1, 2
POINTS = ("tiling_50kb", "sliding_10kb_5kb", "skewed")
DENSE_P_FOUNDER = 0.009


def passes(fn, warmup=1, steps=5):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def windows_of(name, nw, arms=4):
    if name in ("tiling_50kb", "dense_50kb"):
        return [(k * 50000, (k + 1) * 50000, 50000) for k in range(nw)]
    w = [(5000 * k, 5000 * k + 10000, 10000) for k in range(max(nw * 10239 // 4096, 1))]
    if name == "skewed":
        n_site = 50000 * nw
        step = max(len(w) // (arms + 1), 1)
        for a in range(arms):  # arm windows: halves of the chromosome, shifted, spread through the list
            b = (a * n_site) // (2 * arms)
            w.insert((a + 1) * step, (b, b + n_site // 2, n_site // 2))
    return w


def max_sites_of(name):
    return 16384 if name == "skewed" else 4096


def numpy_window(m01, min_mac, max_sites):
    """the restatement of one window from its [n, W] 0/1 matrix -> (n_qualifying, n_used, rmin, n_incompatible, n_blocks, B', A)"""
    n = m01.shape[0]
    c_all = m01.sum(axis=0, dtype=np.int64)
    qual = np.flatnonzero(np.minimum(c_all, n - c_all) >= min_mac)
    q = len(qual)
    m = min(q, max_sites)
    sites = qual[[(k * q) // m for k in range(m)]] if m else qual[:0]
    f = m01[:, sites].T.astype(np.float32)  # counts <= 465: exact in float32
    c = c_all[sites]
    n11 = (f @ f.T).astype(np.int64)
    n10, n01 = c[:, None] - n11, c[None, :] - n11
    n00 = n - c[:, None] - c[None, :] + n11
    inc = np.triu((n11 > 0) & (n10 > 0) & (n01 > 0) & (n00 > 0), 1)
    cong = np.triu(((n10 == 0) & (n01 == 0)) | ((n11 == 0) & (n00 == 0)))
    idx = np.arange(m)
    left1 = np.where(inc.any(axis=0), (inc * (idx[:, None] + 1)).max(axis=0), 0) if m else idx
    rep = cong.argmax(axis=0) if m else idx
    cut = rmin = 0
    for j in range(m):
        if left1[j] >= 1 and left1[j] - 1 >= cut:
            rmin, cut = rmin + 1, j
    run = np.maximum.accumulate(left1) if m else left1
    n_blocks = int((run[1:] > run[:-1]).sum()) + (1 if m else 0)
    same = rep[1:] == rep[:-1]
    in_pair = np.zeros(m, bool)
    in_pair[1:] |= same
    in_pair[:-1] |= same
    return q, m, rmin, int(inc.sum()), n_blocks, int(same.sum()), len(set(rep[in_pair].tolist()))


def numpy_reference(bm, wins, rec, max_sites, k):
    """-> (mean ms per window of the restatement over k windows spread over the list, windows compared, all equal)"""
    if k <= 0:
        return None, 0, True
    short = [i for i, w in enumerate(wins) if w[1] - w[0] <= 100000]  # an arm window's rows are not brought to the host
    pick = sorted({short[int(i)] for i in np.linspace(0, len(short) - 1, k)})
    ts, same = [], True
    for i in pick:
        b, e = int(wins[i][0]), int(wins[i][1])
        bits = bm.download(b, e)
        m01 = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :e - b]
        t0 = time.perf_counter()
        got = numpy_window(m01, MIN_MAC, max_sites)
        ts.append(time.perf_counter() - t0)
        r = rec[i]
        same &= got == (int(r["n_qualifying"]), int(r["n_used"]), int(r["rmin"]), int(r["n_incompatible"]), int(r["n_blocks"]),
                        int(r["n_congruent_adjacent"]), int(r["n_congruent_partitions"]))
    return statistics.mean(ts) * 1e3, len(pick), bool(same)


def point(ctx, bm, name, nw, arms, numpy_windows):
    wl = windows_of(name, nw, arms)
    wins = impop_amd.make_windows(wl)
    kw = dict(min_mac=MIN_MAC, max_sites=max_sites_of(name))
    rec = bm.recomb_scan(wins, **kw)
    t = passes(lambda: bm.recomb_scan(wins, **kw))
    ctx.gram_timing(True)
    bm.recomb_scan(wins, **kw)
    ker, chunks = ctx.recomb_elapsed()
    ctx.gram_timing(False)
    t_ld = passes(lambda: bm.ld_scan(wins, min_mac=MIN_MAC, max_sites=1024))
    np_ms, np_n, np_same = numpy_reference(bm, wl, rec, kw["max_sites"], numpy_windows)
    used = rec["n_used"].astype(np.int64)
    pairs = int((used * (used - 1) // 2).sum())
    return {"windows": len(wins), "max_sites": kw["max_sites"], "recomb_scan_ms": round(t * 1e3, 3), "windows_per_s": round(len(wins) / t, 1),
            "kernel_ms": {"select": round(ker[0], 3), "gather": round(ker[1], 3), "pairs": round(ker[2], 3), "finish": round(ker[3], 3)},
            "kernels_ms": round(sum(ker), 3), "chunks": int(chunks),
            "mean_qualifying": round(float(rec["n_qualifying"].mean()), 2), "mean_used": round(float(used.mean()), 2),
            "max_used": int(used.max()), "site_pairs": pairs,
            "site_pairs_per_s": round(pairs / (ker[2] * 1e-3), 1) if ker[2] > 0 else None,
            "mean_rmin": round(float(rec["rmin"].mean()), 3), "incompatible_pairs": int(rec["n_incompatible"].sum()),
            "ld_scan_ms": round(t_ld * 1e3, 3), "numpy_ms_per_window": None if np_ms is None else round(np_ms, 3),
            "numpy_windows": np_n, "numpy_equal": np_same, "numpy_ms": None if np_ms is None else round(np_ms * len(wins), 1)}


def matrices(ctx, a):
    """(points, matrix) in turn, each matrix freed before the next is made"""
    yield POINTS, lambda: ctx.synthetic(N_HAP, 50000 * a.windows, seed=SEED, keep_hap_major=False), a.windows
    if a.dense_windows > 0:
        yield ("dense_50kb",), lambda: ctx.synthetic(N_HAP, 50000 * a.dense_windows, seed=SEED, p_founder=DENSE_P_FOUNDER,
                                                     keep_hap_major=False), a.dense_windows


def trace_child(a):
    ctx = impop_amd.Context(0)
    for names, make, nw in matrices(ctx, a):
        bm = make()
        for name in names:
            sys.stderr.write(f"@@point {name}\n")
            sys.stderr.flush()
            bm.recomb_scan(windows_of(name, nw, a.arms), min_mac=MIN_MAC, max_sites=max_sites_of(name))
            sys.stderr.write("@@end\n")
            sys.stderr.flush()
        bm.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--dense-windows", type=int, default=256)
    ap.add_argument("--arms", type=int, default=4)
    ap.add_argument("--numpy-windows", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trace_child:
        return trace_child(a)
    ctx = impop_amd.Context(0)
    res = {"bench": "recomb_scan", "device": ctx.device_name(), "n_hap": N_HAP, "min_mac": MIN_MAC, "passes": "median of 5 after 1 warm-up",
           "hbm_read_ceiling_TBps": 6.8, "dense_p_founder": DENSE_P_FOUNDER}
    for names, make, nw in matrices(ctx, a):
        bm = make()
        for name in names:
            res[name] = point(ctx, bm, name, nw, a.arms, a.numpy_windows)
        bm.free()
    ctx.close()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child", "--windows", str(a.windows), "--dense-windows",
                        str(a.dense_windows), "--arms", str(a.arms)], env=dict(os.environ, IMPOP_TRACE="1"), capture_output=True, text=True,
                       timeout=900)
    if r.returncode != 0:
        sys.exit("the trace run failed:\n" + r.stderr[-2000:])
    cur = None
    for line in r.stderr.splitlines():
        if line.startswith("@@point "):
            cur = line.split()[1]
        elif line.startswith("@@end"):
            cur = None
        elif line.startswith("[impop_recomb_scan]") and cur:
            res[cur]["trace"] = line
            streamed = int(re.search(r"bytes_streamed=(\d+)", line).group(1))
            sel_ms = res[cur]["kernel_ms"]["select"]
            res[cur]["bytes_streamed"] = streamed
            res[cur]["pair_tiles"] = int(re.search(r"pair_tiles=(\d+)", line).group(1))
            res[cur]["select_TBps"] = round(streamed / (sel_ms * 1e-3) / 1e12, 3) if sel_ms > 0 else None
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
