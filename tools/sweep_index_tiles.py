"""Tile size of INDEXED scan plans: the headline workload (465 haplotypes, 4854 x 50 kb windows) on the variable-site index,
plans with several tile_blocks side by side, interleaved rounds, HIP-event kernel time of the streaming kernel
(impop_scan_plan_timing) and the end-to-end launch (streaming kernel + finalize) per setting.

    python tools/sweep_index_tiles.py [--rounds 7] [--launches 50] [--tiles 0,8,16,24,32,48,64,96,128]

Prints one JSON line per setting: median kernel ms, bytes streamed, GB/s of those bytes, median launch ms."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--tiles", default="0,8,16,24,32,48,64,96,128")
    ap.add_argument("--n-hap", type=int, default=465)
    ap.add_argument("--window", type=int, default=50000)
    ap.add_argument("--n-windows", type=int, default=4854)
    a = ap.parse_args()
    import impop_amd
    ctx = impop_amd.Context(0)
    n, W, NW = a.n_hap, a.window, a.n_windows
    t0 = time.perf_counter()
    bm = ctx.synthetic(n, W * NW, seed=20251031)
    ctx.synchronize()
    info = bm.scan_index_info()
    print(json.dumps({"matrix_s": time.perf_counter() - t0, **info}), flush=True)
    wins = impop_amd.fixed_windows(W * NW, W)
    in_a = np.zeros(n, np.uint8); in_a[:140] = 1
    in_b = np.zeros(n, np.uint8); in_b[140:240] = 1
    tiles = [int(t) for t in a.tiles.split(",")]
    plans = {t: bm.plan(wins, None, in_a, in_b, tile_blocks=t) for t in tiles}
    ref = None
    for t, p in plans.items():
        p.launch()
        r = p.fetch().tobytes()
        ref = r if ref is None else ref
        assert r == ref, f"tile_blocks={t}: records differ"
    kern = {t: [] for t in tiles}
    full = {t: [] for t in tiles}
    for _ in range(a.rounds):
        for t, p in plans.items():
            p.timing(True)
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.launches):
                p.launch()
            ctx.synchronize()
            full[t].append((time.perf_counter() - t0) / a.launches * 1e3)
            ms, k = p.elapsed()
            kern[t].append(ms / k)
            p.timing(False)
    for t, p in plans.items():
        km = float(np.median(kern[t]))
        print(json.dumps({"tile_blocks": t, "n_tiles": p.n_tiles, "bytes_streamed": p.bytes_streamed, "kernel_ms": km,
                          "kernel_ms_min": float(np.min(kern[t])), "kernel_ms_max": float(np.max(kern[t])),
                          "GBps": p.bytes_streamed / (km / 1e3) / 1e9, "launch_ms": float(np.median(full[t]))}), flush=True)
    for p in plans.values():
        p.destroy()
    bm.free()
    ctx.close()


if __name__ == "__main__":
    main()
