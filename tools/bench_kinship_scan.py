#!/usr/bin/env python3
"""impop_genotypes_create + impop_kinship_scan with 232 individuals (464 of the 465 haplotypes) on the synthetic bench chromosome,
from one process and one run, on --windows (default 4096) tiling windows of 50 kb, for the full matrix and for the matrix
compacted to its variable sites:

  plane build   impop_genotypes_create: the kernel's time from HIP events (impop_ctx_kinship_elapsed[0]) and the GB/s of the bytes
                it reads (the source's site-major rows) plus the bytes it writes (the 2N-row operand's cells); the whole call too
  kinship scan  the whole call (median of 5 after 3 warm-up) with the per-pair totals and 16 watched pairs, the Gram time
                (impop_ctx_gram_elapsed) and the epilogue kernels' time (impop_ctx_kinship_elapsed[1]) with its share of the call;
                and the call without the per-pair totals (the window kernel alone)

Yardstick, in the same process on the same matrix: impop_pairdist_scan on the same windows with the 464 paired haplotypes as one
panel — the same Gram size (480 padded rows) — and the ratio of the two calls.
No counter run is made here: how the epilogue's time splits between the strided column reads of the A x H entries, the row reads
and the reductions is NOT attributed.
One JSON line on stdout; --out FILE also writes it there (the recorded run: profiles/r23_kinship_scan.json)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import impop_amd  # noqa: E402

N_HAP, N_IND, SEED, N_WATCH = 465, 232, 1, 16
KIN = (884, 10000)


def passes(fn, warmup=3, steps=5):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), max(ts) - min(ts)


def pairs_of():
    return np.random.default_rng(SEED).permutation(N_HAP)[: 2 * N_IND].reshape(N_IND, 2).astype(np.uint32)


def build_point(ctx, bm, pairs):
    """-> (the planes, figures of the plane build)"""
    bm.genotypes(pairs).free()  # warm-up: the kernel's code object, the scratch
    ctx.gram_timing(True)
    t0 = time.perf_counter()
    g = bm.genotypes(pairs)
    call = time.perf_counter() - t0
    (build_ms, _), _ = ctx.kinship_elapsed()
    ctx.gram_timing(False)
    n_block = (bm.n_site + 63) // 64
    read = n_block * 64 * bm.bytes_per_site
    written = ((2 * N_IND + 31) // 32) * n_block * 256
    return g, {"kernel_ms": round(build_ms, 3), "call_ms": round(call * 1e3, 3), "bytes_read": int(read), "bytes_written": int(written),
               "gb_per_s": round((read + written) / (build_ms * 1e-3) / 1e9, 1) if build_ms > 0 else None, "plane_bytes": int(g.device_bytes)}


def scan_point(ctx, g, wins, watch):
    t, spread = passes(lambda: g.kinship_scan(wins, kin=KIN, watch=watch, want_pairs=True))
    ctx.gram_timing(True)
    g.kinship_scan(wins, kin=KIN, watch=watch, want_pairs=True)
    gram_ms, launches = ctx.gram_elapsed()
    (_, epi_ms), chunks = ctx.kinship_elapsed()
    ctx.gram_timing(False)
    lean, _ = passes(lambda: g.kinship_scan(wins, kin=KIN, watch=None, want_pairs=False))
    ctx.gram_timing(True)
    g.kinship_scan(wins, kin=KIN, watch=None, want_pairs=False)
    (_, lean_epi_ms), _ = ctx.kinship_elapsed()
    ctx.gram_timing(False)
    return {"call_ms": round(t * 1e3, 3), "spread_ms": round(spread * 1e3, 3), "us_per_window": round(t / len(wins) * 1e6, 3),
            "gram_kernel_ms": round(gram_ms, 3), "gram_launches": int(launches), "epilogue_ms": round(epi_ms, 3), "chunks": int(chunks),
            "epilogue_share_of_call": round(epi_ms / (t * 1e3), 3), "windows_only_call_ms": round(lean * 1e3, 3),
            "windows_only_epilogue_ms": round(lean_epi_ms, 3)}


def yardstick(ctx, bm, wins, pairs):
    panel = np.zeros(N_HAP, np.uint8)
    panel[pairs.ravel()] = 1
    t, spread = passes(lambda: bm.pairdist_scan(wins, [panel]))
    ctx.gram_timing(True)
    bm.pairdist_scan(wins, [panel])
    gram_ms, _ = ctx.gram_elapsed()
    epi_ms, _ = ctx.pairdist_elapsed()
    ctx.gram_timing(False)
    return {"call_ms": round(t * 1e3, 3), "spread_ms": round(spread * 1e3, 3), "gram_kernel_ms": round(gram_ms, 3),
            "pairdist_kernel_ms": round(epi_ms, 3), "members": int(panel.sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = impop_amd.Context(0)
    res = {"bench": "kinship_scan", "device": ctx.device_name(), "n_hap": N_HAP, "individuals": N_IND, "windows": a.windows, "window_bp": 50000,
           "watch": N_WATCH, "passes": "median of 5 after 3 warm-up; spread = max - min; the plane build is one timed call after one warm-up",
           "not_measured": "no counter run: the split of the epilogue between the strided column reads, the row reads and the reductions is "
                           "unattributed"}
    pairs = pairs_of()
    watch = [(k, N_IND - 1 - k) for k in range(N_WATCH)]
    wins = [(k * 50000, (k + 1) * 50000, 50000) for k in range(a.windows)]
    full = ctx.synthetic(N_HAP, 50000 * a.windows, seed=SEED, keep_hap_major=True)
    for name in ("full", "compacted"):
        bm = full if name == "full" else full.compact()
        g, build = build_point(ctx, bm, pairs)
        r = {"n_site": int(bm.n_site), "plane_build": build, "kinship_scan": scan_point(ctx, g, wins, watch),
             "pairdist_scan_one_panel": yardstick(ctx, bm, wins, pairs)}
        r["ratio_kinship_to_pairdist"] = round(r["kinship_scan"]["call_ms"] / r["pairdist_scan_one_panel"]["call_ms"], 3)
        g.free()
        if bm is not full:
            bm.free()
        res[name] = r
    full.free()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
