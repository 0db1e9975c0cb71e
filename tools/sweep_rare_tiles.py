"""Tiles of the SPLIT scan index (rare-site entries + common-site rows): the headline workload (465 haplotypes, 4854 x 50 kb
windows) on a split matrix and on its unsplit twin (IMPOP_KEEP_NO_RARE_SPLIT), plans with several tile_blocks side by side,
interleaved rounds, HIP-event kernel time of the streaming kernel (impop_scan_plan_timing) and the end-to-end launch per
setting.  --cold also times single launches each behind a 512 MiB write to another buffer, so that the rare entries and rows
(about 0.2 GB, under the 256 MiB Infinity Cache) cannot be served from the cache the previous launch left behind.

    python tools/sweep_rare_tiles.py [--rounds 7] [--launches 50] [--tiles 0,8,16,32,49,64,96,128] [--cold 20]

The lines of profiles/r05_rare_tile_sweep.jsonl marked "separate" came from a variant build that put a segment's entries and
rows into separate tiles instead of one workgroup reading a share of both; it was slower (0.0512-0.0520 ms) and was removed
(commit 7af4fd5 still has its build switch).  Prints one JSON line per setting."""
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
    ap.add_argument("--tiles", default="0,8,16,32,49,64,96,128")
    ap.add_argument("--cold", type=int, default=0, help="single launches behind a 512 MiB write, per setting (0: skip)")
    ap.add_argument("--n-hap", type=int, default=465)
    ap.add_argument("--window", type=int, default=50000)
    ap.add_argument("--n-windows", type=int, default=4854)
    a = ap.parse_args()
    import impop_amd
    ctx = impop_amd.Context(0)
    n, W, NW = a.n_hap, a.window, a.n_windows
    mats = {}
    for name, split in (("split", True), ("nosplit", False)):
        ctx.synchronize()
        t0 = time.perf_counter()
        mats[name] = ctx.synthetic(n, W * NW, seed=20251031, rare_split=split)
        ctx.synchronize()
        print(json.dumps({"matrix": name, "create_s": time.perf_counter() - t0, **mats[name].scan_index_info(),
                          **{("split_" + k): v for k, v in mats[name].scan_split_info().items()}}), flush=True)
    wins = impop_amd.fixed_windows(W * NW, W)
    in_a = np.zeros(n, np.uint8); in_a[:140] = 1
    in_b = np.zeros(n, np.uint8); in_b[140:240] = 1
    tiles = [int(t) for t in a.tiles.split(",")]
    plans = {("split", t): mats["split"].plan(wins, None, in_a, in_b, tile_blocks=t) for t in tiles}
    plans[("nosplit", 0)] = mats["nosplit"].plan(wins, None, in_a, in_b)
    ref = None
    for key, p in plans.items():
        p.launch()
        r = p.fetch().tobytes()
        ref = r if ref is None else ref
        assert r == ref, f"{key}: records differ"
    kern = {k: [] for k in plans}
    full = {k: [] for k in plans}
    for _ in range(a.rounds):
        for key, p in plans.items():
            p.timing(True)
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.launches):
                p.launch()
            ctx.synchronize()
            full[key].append((time.perf_counter() - t0) / a.launches * 1e3)
            ms, k = p.elapsed()
            kern[key].append(ms / k)
            p.timing(False)
    cold = {k: [] for k in plans}
    if a.cold:
        import torch
        flush = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
        for i in range(a.cold):
            for key, p in plans.items():
                flush.fill_(i & 255)
                torch.cuda.synchronize()  # the write is done (and the cache full of it) before the launch
                p.timing(True)
                p.launch()
                ms, k = p.elapsed()
                cold[key].append(ms / k)
                p.timing(False)
    for key, p in plans.items():
        km = float(np.median(kern[key]))
        out = {"matrix": key[0], "tile_blocks": key[1], "n_tiles": p.n_tiles, "bytes_streamed": p.bytes_streamed, "kernel_ms": km,
               "kernel_ms_min": float(np.min(kern[key])), "kernel_ms_max": float(np.max(kern[key])),
               "GBps": p.bytes_streamed / (km / 1e3) / 1e9, "launch_ms": float(np.median(full[key]))}
        if cold[key]:
            cm = float(np.median(cold[key]))
            out.update({"cold_kernel_ms": cm, "cold_GBps": p.bytes_streamed / (cm / 1e3) / 1e9})
        print(json.dumps(out), flush=True)
    for p in plans.values():
        p.destroy()
    for m in mats.values():
        m.free()
    ctx.close()


if __name__ == "__main__":
    main()
