"""Where one wave per tile stops paying (tile_cut.h, wave_tile_rule): the headline matrix (465 haplotypes, 4854 x 50 kb sites,
synthetic) scanned in disjoint windows of several lengths and numbers, every plan made twice — IMPOP_SCAN_WAVE_TILES=0, four
waves per tile, and =1, one wave per tile wherever the 32-bit lane sums allow — interleaved rounds, HIP-event time of the
streaming kernel (impop_scan_plan_timing) and the wall time of launch + synchronise per setting.  A window count that the
matrix is too short for at that length is capped at what fits and printed as it ran.

    python tools/sweep_wave_tiles.py [--rounds 5] [--launches 50] [--lengths 5,10,25,50,100,200,400] [--counts 256,1024,4854]
                                     [--sites N] [--tile-blocks B]     (a longer matrix and larger tiles: long windows in number)

Prints one JSON line per (length, count): kernel microseconds per launch of both arms (median and min .. max over the rounds),
the plan's bytes per tile, and whether forced 1 wins by more than the forced-0 arm's
own spread — the criterion the thresholds of the rule were set by."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ENV = "IMPOP_SCAN_WAVE_TILES"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--lengths", default="5,10,25,50,100,200,400", help="window lengths in kb")
    ap.add_argument("--counts", default="256,1024,4854")
    ap.add_argument("--n-hap", type=int, default=465)
    ap.add_argument("--sites", type=int, default=4854 * 50000)
    ap.add_argument("--tile-blocks", type=int, default=0, help="0: the default tile; else the plans' tile_blocks (larger tiles)")
    a = ap.parse_args()
    import impop_amd
    os.environ["IMPOP_SCAN_DIGEST"] = "0"  # the two bodies on the streams: a kept plan on one wave would otherwise take a tile digest
    ctx = impop_amd.Context(0)
    n = a.n_hap
    bm = ctx.synthetic(n, a.sites, seed=20251031)
    ctx.synchronize()
    in_a = np.zeros(n, np.uint8); in_a[: min(140, n)] = 1
    in_b = np.zeros(n, np.uint8); in_b[min(140, n): min(240, n)] = 1
    for kb in (int(x) for x in a.lengths.split(",")):
        W = kb * 1000
        for want in (int(x) for x in a.counts.split(",")):
            nw = min(want, a.sites // W)
            windows = impop_amd.fixed_windows(a.sites, W)[:nw]
            plans = {}
            for arm in ("0", "1"):
                os.environ[ENV] = arm
                plans[arm] = bm.plan(windows, None, in_a, in_b, tile_blocks=a.tile_blocks)
            del os.environ[ENV]
            ref = None
            for arm, pl in plans.items():  # warm up, and the two bodies must agree
                pl.launch()
                r = pl.fetch().tobytes()
                assert ref is None or r == ref, (kb, nw, "records differ between the arms")
                ref = r
            us = {arm: [] for arm in plans}
            wall = {arm: [] for arm in plans}
            for _ in range(a.rounds):
                for arm, pl in plans.items():
                    pl.timing(True)
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.launches):
                        pl.launch()
                    ctx.synchronize()
                    wall[arm].append((time.perf_counter() - t0) / a.launches * 1e6)
                    ms, k = pl.elapsed()
                    pl.timing(False)
                    us[arm].append(ms / max(k, 1) * 1e3)
            med = {arm: float(np.median(v)) for arm, v in us.items()}
            spread0 = max(us["0"]) - min(us["0"])
            out = {"window_kb": kb, "windows": nw, "tile_blocks": a.tile_blocks, "tiles": plans["0"].n_tiles, "bytes_streamed": plans["0"].bytes_streamed,
                   "bytes_per_tile": plans["0"].bytes_streamed / max(plans["0"].n_tiles, 1),
                   "kernel_us_four_waves": {"median": med["0"], "min": min(us["0"]), "max": max(us["0"])},
                   "kernel_us_one_wave": {"median": med["1"], "min": min(us["1"]), "max": max(us["1"])},
                   "wall_us_four_waves": float(np.median(wall["0"])), "wall_us_one_wave": float(np.median(wall["1"])),
                   "one_wave_gain_us": med["0"] - med["1"], "four_wave_spread_us": spread0,
                   "one_wave_wins": bool(med["0"] - med["1"] > spread0 and max(us["1"]) < min(us["0"]))}
            print(json.dumps(out), flush=True)
            for pl in plans.values():
                pl.destroy()
    bm.free()
    ctx.close()


if __name__ == "__main__":
    main()
