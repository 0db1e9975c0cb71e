#!/usr/bin/env python3
"""impop_paint_scan from one process and one run, mismatch cost 2, switch cost 12, no segment list:

  compact_all    465 haplotypes all against all (every haplotype a recipient, the other 464 its donors) on the synthetic founder
                 chromosome of --windows (4096) x 50 kb, compacted to its variable sites
  dense_all      the same on the --dense-sites (12.8 M) dense slab whose founders differ at 0.9 % of the sites
  donors_1024    --wide-recipients (64) recipients against 1024 donors (the limit: 16 states a lane) over --wide-sites (1 M) dense sites

Per point: the median of --steps (3) timed calls after one warm-up call of BitMatrix.paint_scan(want_segments=False) with
max_chunk_bytes = --budget-gib (the default budget of 1 GiB would cut a 12.8 M-site call into ranges of 5 recipients: the per-site
records are 8 bytes x sites x recipients); from HIP events (impop_ctx_gram_timing) the time of its four kernel groups (transpose /
forward / backtrack + emit + mismatch + records / windows) in one call; donor-site updates per second = sum over recipients of
donors x sites / the forward kernel's time; the recipient ranges and site chunks from the trace line's counters recomputed here.
  numpy          the same recursion (the literal stay-bit form, vectorised over the donors, a Python loop over the sites) for
                 --numpy-recipients (2) recipients over the first --numpy-sites (20000) sites of the dense slab, rows downloaded from
                 the device; cost, n_segments and n_mismatch must equal the device's on that range.  numpy_updates_per_s is the
                 comparison figure.
One JSON line on stdout; --out FILE also writes it there (the recorded run: profiles/r31_paint_scan.json).  Every figure in it is
measured in that run; what bounds the forward kernel is NOT attributed: no counter run was made."""
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

N_HAP, SEED, MU, C_SWITCH = 465, 1, 2, 12
DENSE_P_FOUNDER = 0.009


def passes(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def numpy_paint(x, D, mu, c):
    """the literal recursion with the stay bits -> (cost, n_segments, n_mismatch)"""
    K, L = D.shape
    mm = (D != x[None, :]).astype(np.int64) * mu
    stay = np.zeros((L, K), dtype=bool)
    A = np.zeros(L, dtype=np.int64)
    V = mm[:, 0].copy()
    A[0] = int(np.argmin(V))
    for s in range(1, L):
        sw = int(V.min()) + c
        stay[s] = V <= sw
        V = mm[:, s] + np.minimum(V, sw)
        A[s] = int(np.argmin(V))
    d = np.zeros(L, dtype=np.int64)
    d[L - 1] = A[L - 1]
    for s in range(L - 1, 0, -1):
        d[s - 1] = d[s] if stay[s, d[s]] else A[s - 1]
    return int(V.min()), 1 + int((d[1:] != d[:-1]).sum()), int((mm[d, np.arange(L)] != 0).sum())


def point(ctx, bm, recipients, donors, budget, steps, sites):
    kw = dict(donors=donors, mismatch_cost=MU, switch_cost=C_SWITCH, want_segments=False, want_chunks=True, max_chunk_bytes=budget)
    got = bm.paint_scan(recipients, **kw)
    t = passes(lambda: bm.paint_scan(recipients, **kw), 0, steps)
    ctx.gram_timing(True)
    bm.paint_scan(recipients, **kw)
    ker, chunks = ctx.paint_elapsed()
    ctx.gram_timing(False)
    rec = got["recipients"]
    updates = int(rec["n_donors"].astype(np.int64).sum()) * sites
    range_len = min(len(recipients), max(1, (budget // 2) // (sites * 8)))
    return {"recipients": len(recipients), "donors_max": int(rec["n_donors"].max()), "sites": sites, "paint_scan_ms": round(t * 1e3, 3),
            "kernel_ms": {k: round(v, 3) for k, v in zip(("transpose", "forward", "backtrack_emit", "windows"), ker)},
            "forward_chunks": int(chunks), "recipient_ranges": -(-len(recipients) // range_len), "donor_site_updates": updates,
            "donor_site_updates_per_s": round(updates / (ker[1] * 1e-3), 1) if ker[1] > 0 else None,
            "ns_per_site_per_recipient_wave": round(ker[1] * 1e6 / (sites * -(-len(recipients) // range_len)), 3) if ker[1] > 0 else None,
            "segments": got["n_segments"], "mismatches": int(rec["n_mismatch"].astype(np.int64).sum()),
            "cost_sum": int(rec["cost"].astype(np.uint64).sum()), "measured": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--dense-sites", type=int, default=12800000)
    ap.add_argument("--wide-sites", type=int, default=1000000)
    ap.add_argument("--wide-recipients", type=int, default=64)
    ap.add_argument("--numpy-sites", type=int, default=20000)
    ap.add_argument("--numpy-recipients", type=int, default=2)
    ap.add_argument("--budget-gib", type=float, default=128.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    budget = int(a.budget_gib * (1 << 30))
    ctx = impop_amd.Context(0)
    res = {"bench": "paint_scan", "device": ctx.device_name(), "n_hap": N_HAP, "mismatch_cost": MU, "switch_cost": C_SWITCH,
           "passes": f"median of {a.steps} after 1 warm-up", "max_chunk_bytes": budget, "dense_p_founder": DENSE_P_FOUNDER,
           "forward_kernel_bound": "unattributed: no counter run was made"}
    everyone = np.arange(N_HAP, dtype=np.uint32)
    if a.windows > 0:
        full = ctx.synthetic(N_HAP, 50000 * a.windows, seed=SEED, keep_hap_major=False)
        bm = full.compact()
        full.free()
        res["compact_all"] = point(ctx, bm, everyone, None, budget, a.steps, bm.n_site)
        bm.free()
    if a.dense_sites > 0:
        bm = ctx.synthetic(N_HAP, a.dense_sites, seed=SEED, p_founder=DENSE_P_FOUNDER, keep_hap_major=False)
        res["dense_all"] = point(ctx, bm, everyone, None, budget, a.steps, a.dense_sites)
        if a.numpy_recipients > 0:
            L = min(a.numpy_sites, a.dense_sites)
            bits = bm.download(0, L)
            m01 = np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little")[:, :L]
            pick = [int(x) for x in np.linspace(0, N_HAP - 1, a.numpy_recipients)]
            dev = bm.paint_scan(pick, mismatch_cost=MU, switch_cost=C_SWITCH, site_end=L, want_segments=False)["recipients"]
            same, t0 = True, time.perf_counter()
            for k, h in enumerate(pick):
                others = [j for j in range(N_HAP) if j != h]
                same &= numpy_paint(m01[h], m01[others], MU, C_SWITCH) == (int(dev["cost"][k]), int(dev["n_segments"][k]), int(dev["n_mismatch"][k]))
            dt = time.perf_counter() - t0
            res["numpy"] = {"recipients": len(pick), "sites": L, "seconds": round(dt, 3), "equal": bool(same),
                            "numpy_updates_per_s": round(len(pick) * (N_HAP - 1) * L / dt, 1), "measured": True}
        bm.free()
    if a.wide_sites > 0:
        bm = ctx.synthetic(1025, a.wide_sites, seed=SEED, p_founder=DENSE_P_FOUNDER, keep_hap_major=False)
        donors = np.ones(1025, np.uint8)
        donors[0] = 0  # 1024 donors; recipient 0 sees them all, the others 1023
        rc = np.array(sorted({0} | {int(x) for x in np.linspace(1, 1024, a.wide_recipients - 1)}), dtype=np.uint32)
        res["donors_1024"] = point(ctx, bm, rc, donors, budget, a.steps, a.wide_sites)
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
