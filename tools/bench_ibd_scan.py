#!/usr/bin/env python3
"""impop_ibd_scan at 465 haplotypes, all 107 880 pairs, from one process and one run, on the two matrices of tools/bench_ibs_scan.py
(the synthetic bench chromosome compacted to its variable sites, and its first 12.8 M sites as they are).

Per matrix the range = the whole matrix.  min_sites starts at --min-sites and doubles until impop_ibs_scan's all-pairs list holds
at most --max-segments records (the rule of bench_ibs_scan.py); the rule is max_gap = min_sites / 4, min_extend = the length of
min_sites sites at the map's mean rate, min_seed = min_output = 3 x that.  Two points: with a genetic map (one breakpoint per
--map-step sites, rates drawn per interval, every tenth interval at rate zero: too long for the kernel's LDS staging on the full
chromosome) and without one (lengths in sites).
Per point: the median of --steps timed calls after one warm-up call and their spread (max - min) for one call with room for the
segment list, the four kernel times of one call from HIP events (impop_ctx_gram_timing: transpose / walk / combine + close /
chain), candidates and segments.
Baseline, in the same process on the same matrix: impop_ibs_scan with its segment list at the same min_sites (one call with room
for it), and the stitching of that list on the host in numpy (map lookup with searchsorted, candidate and break flags, reduceat);
its segments are compared with the call's.  ratio_to_ibs_scan = ibd call / ibs call; speedup_over_ibs_plus_host = (ibs call + host
stitching) / ibd call.
No counter run is made here: what bounds the chain kernel is NOT measured.
One JSON line on stdout; --out FILE also writes it there (the recorded run: profiles/r26_ibd_scan.json)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import impop_amd  # noqa: E402
from bench_ibs_scan import N_HAP, matrices  # noqa: E402


def passes(fn, steps):
    fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), max(ts) - min(ts)


def make_map(span, step, seed=20261020):
    """breakpoints every `step` coordinates over [0, span]; micro-units per coordinate drawn per interval, every tenth zero"""
    rng = np.random.default_rng(seed)
    pos = np.arange(0, span + step, step, dtype=np.uint64)
    rate = rng.integers(0, 3, size=len(pos) - 1).astype(np.uint64)  # mean 1 unit per coordinate
    rate[::10] = 0
    g = np.concatenate([[0], np.cumsum(rate * np.uint64(step), dtype=np.uint64)]).astype(np.uint64)
    return pos, g


def G_of(gmap, x):
    if gmap is None:
        return x.astype(np.uint64)
    pos, g = gmap
    k = np.clip(np.searchsorted(pos, x, side="right") - 1, 0, len(pos) - 2)
    xc = np.clip(x, pos[0], pos[-1]).astype(np.uint64)
    return g[k] + (xc - pos[k]) * (g[k + 1] - g[k]) // (pos[k + 1] - pos[k])


def host_stitch(seg, gmap, rule):
    """the definition over impop_ibs_scan's list (tracts of extent >= min_sites, pair-major, ascending) -> (begin, end, len, pair)"""
    s, t, pair = seg["begin"], seg["end"], seg["pair"]
    gs, gt = G_of(gmap, s), G_of(gmap, t)
    cand = (gt - gs) >= rule["min_extend"]
    s, t, pair, gs, gt = s[cand], t[cand], pair[cand], gs[cand], gt[cand]
    if len(s) == 0:
        return s, t, gs, pair
    seed = (gt - gs) >= rule["min_seed"]
    brk = np.ones(len(s), dtype=bool)
    brk[1:] = (pair[1:] != pair[:-1]) | (s[1:] - t[:-1] > rule["max_gap"])
    head = np.flatnonzero(brk)
    last = np.concatenate([head[1:], [len(s)]]) - 1
    has_seed = np.add.reduceat(seed.astype(np.int64), head) > 0
    ln = gt[last] - gs[head]
    keep = has_seed & (ln >= rule["min_output"])
    return s[head][keep], t[last][keep], ln[keep], pair[head][keep]


def point(ctx, bm, min_sites, gmap, steps):
    span = int(getattr(bm, "compacted_from_sites", None) or bm.n_site)
    unit = min_sites if gmap is None else int(int(gmap[1][-1]) * min_sites // span)
    rule = dict(min_extend=unit, min_seed=3 * unit, min_output=3 * unit, max_gap=min_sites // 4)
    kw = dict(rule, min_sites=min_sites)
    if gmap is not None:
        kw["map_pos"], kw["map_g"] = gmap
    rec, _, _, total = bm.ibd_scan(want_segments=False, **kw)
    t, spread = passes(lambda: bm.ibd_scan(seg_capacity=total, **kw), steps)
    ctx.gram_timing(True)
    _, seg, _, _ = bm.ibd_scan(seg_capacity=total, **kw)
    ker, chunks = ctx.ibd_elapsed()
    ctx.gram_timing(False)
    n_tracts = bm.ibs_scan(min_sites=min_sites, want_segments=False)[3]
    t_ibs, spread_ibs = passes(lambda: bm.ibs_scan(min_sites=min_sites, seg_capacity=n_tracts), steps)
    tracts = bm.ibs_scan(min_sites=min_sites, seg_capacity=n_tracts)[1]
    ts = []
    for _ in range(max(steps // 2, 1)):
        t0 = time.perf_counter()
        hb, he, hl, hp = host_stitch(tracts, gmap, rule)
        ts.append(time.perf_counter() - t0)
    t_host = statistics.median(ts)
    same = bool(len(hb) == len(seg) and np.array_equal(hb, seg["begin"]) and np.array_equal(he, seg["end"]) and np.array_equal(hl, seg["len"])
                and np.array_equal(hp, seg["pair"]))
    return {"pairs": len(rec), "rule": dict(kw, map_pos=None, map_g=None) if gmap is not None else kw,
            "map_points": 0 if gmap is None else len(gmap[0]), "staged_tracts": int(n_tracts), "candidates": int(rec["n_candidates"].sum(dtype=np.int64)),
            "segments": int(total), "ms": round(t * 1e3, 3), "spread_ms": round(spread * 1e3, 3),
            "kernel_ms": {"transpose": round(ker[0], 3), "walk": round(ker[1], 3), "combine_close": round(ker[2], 3), "chain": round(ker[3], 3)},
            "site_chunks": int(chunks), "ibs_scan_list_ms": round(t_ibs * 1e3, 3), "ibs_scan_spread_ms": round(spread_ibs * 1e3, 3),
            "host_stitch_ms": round(t_host * 1e3, 3), "host_segments_equal": same, "ratio_to_ibs_scan": round(t / t_ibs, 3),
            "speedup_over_ibs_plus_host": round((t_ibs + t_host) / t, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=50000 * 4854, help="sites of the chromosome that is compacted (default: the bench chromosome)")
    ap.add_argument("--dense-sites", type=int, default=50000 * 256, help="sites of the dense slab")
    ap.add_argument("--min-sites", type=int, default=64)
    ap.add_argument("--max-segments", type=int, default=12_000_000)
    ap.add_argument("--map-step", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = impop_amd.Context(0)
    res = {"bench": "ibd_scan", "device": ctx.device_name(), "n_hap": N_HAP, "passes": f"median of {a.steps} after 1 warm-up; spread = max - min",
           "not_measured": "no counter run: what bounds the chain kernel is unattributed"}
    mats = matrices(ctx, a.sites, a.dense_sites)
    min_sites = a.min_sites
    while mats["compact"].ibs_scan(min_sites=min_sites, want_segments=False)[3] > a.max_segments:
        min_sites *= 2
    res["min_sites"] = min_sites
    for name, bm in mats.items():
        span = int(getattr(bm, "compacted_from_sites", None) or bm.n_site)
        res[name] = {"sites": int(bm.n_site), "range_sites": span, "map": point(ctx, bm, min_sites, make_map(span, a.map_step), a.steps),
                     "no_map": point(ctx, bm, min_sites, None, a.steps)}
        bm.free()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
