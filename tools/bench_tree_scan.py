#!/usr/bin/env python3
"""impop_tree_scan at 465 haplotypes on the synthetic bench chromosome, from one process and one run: --windows (default 4096)
windows of 50 kb, on the full and on the compacted matrix, for the three linkages, without panels and with five.

Per point: the whole call (median of 5 after 3 warm-up), the Gram time and the tree kernel's time from HIP events
(impop_ctx_gram_timing: impop_ctx_gram_elapsed, impop_ctx_tree_elapsed), rows_recomputed per merge from the call's IMPOP_TRACE line,
windows with tied merges.
Against what: impop_pairdist_scan (one panel) and impop_pca_scan (k = 2) on the same windows — the same Gram pass, so the ratio
isolates the epilogue; and a host baseline for the same answer: one impop_pairwise_counts per window (the full Gram matrix copied to
the host) plus scipy.cluster.hierarchy.linkage where scipy is installed, else tests/plain_tree.py, timed on --baseline-windows
windows and stated per window.  scipy's floating-point trees are not compared merge for merge (its tie rule is its own); the
sorted single-linkage heights are.
No counter run is made here: whether the tree kernel is bound by the barriers of its m - 1 dependent steps or by the rescanned rows
out of memory is NOT attributed; one experiment bears on it: the same points under IMPOP_TREE_WIDE=1 (64-bit sums: twice the bytes of
every row read and of the scratch, the same steps and barriers; --skip-baselines runs the tree points alone).
One JSON line on stdout; --out FILE also writes it there (the recorded run: profiles/r28_tree_scan.json)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["IMPOP_TRACE"] = "1"  # read once per process by the library: the bench parses the [impop_tree_scan] line
import numpy as np  # noqa: E402

import impop_amd  # noqa: E402
import plain_tree as pt  # noqa: E402
from plain_pairdist import hamming  # noqa: E402

N_HAP, SEED, LINKAGES = 465, 1, ("single", "complete", "average")


class quiet_stderr:
    """file descriptor 2 into a temporary file for the time of a block; .text afterwards"""

    def __enter__(self):
        sys.stderr.flush()
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def passes(fn, warmup=3, steps=5):
    with quiet_stderr():
        for _ in range(warmup):
            fn()
        ts = []
        for _ in range(steps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
    return statistics.median(ts), max(ts) - min(ts)


def point(ctx, bm, wins, linkage, pops):
    kw = dict(linkage=linkage, pops=pops, want_merges=True)
    t, spread = passes(lambda: bm.tree_scan(wins, **kw))
    ctx.gram_timing(True)
    with quiet_stderr() as err:
        recs = bm.tree_scan(wins, **kw)[0]
    gram_ms, launches = ctx.gram_elapsed()
    tree_ms, chunks = ctx.tree_elapsed()
    ctx.gram_timing(False)
    line = [l for l in err.text.splitlines() if l.startswith("[impop_tree_scan] route=")][-1]
    trace = dict(f.split("=") for f in line.split()[1:])
    return {"call_ms": round(t * 1e3, 3), "spread_ms": round(spread * 1e3, 3), "us_per_window": round(t / len(wins) * 1e6, 3),
            "gram_kernel_ms": round(gram_ms, 3), "gram_launches": int(launches), "tree_kernel_ms": round(tree_ms, 3), "chunks": int(chunks),
            "tree_share_of_call": round(tree_ms / (t * 1e3), 3),
            "rows_recomputed_per_merge": round(int(trace["rows_recomputed"]) / (len(wins) * (N_HAP - 1)), 3),
            "tied_windows": int(trace["tied_windows"]), "distinct_mean": round(float((recs["n_members"] - recs["n_zero_merges"]).mean()), 1)}


def same_gram_pass(ctx, bm, wins):
    """the two neighbours on the same windows"""
    out = {}
    for name, fn in (("pairdist_scan", lambda: bm.pairdist_scan(wins, [np.ones(N_HAP, np.uint8)])),
                     ("pca_scan_k2", lambda: bm.pca_scan(wins, k=2, want_vectors=False))):
        t, spread = passes(fn)
        ctx.gram_timing(True)
        with quiet_stderr():
            fn()
        gram_ms, _ = ctx.gram_elapsed()
        ctx.gram_timing(False)
        out[name] = {"call_ms": round(t * 1e3, 3), "spread_ms": round(spread * 1e3, 3), "gram_kernel_ms": round(gram_ms, 3)}
    return out


def baseline(bm, wins, linkage, n_sub, call_ms):
    sub = [wins[int(i)] for i in np.linspace(0, len(wins) - 1, n_sub).astype(int)]
    try:
        from scipy.cluster.hierarchy import linkage as scipy_linkage
        from scipy.spatial.distance import squareform
        how = "scipy.cluster.hierarchy.linkage"

        def solve(H):
            return scipy_linkage(squareform(H.astype(np.float64), checks=False), linkage)
    except ImportError:
        how = "tests/plain_tree.py"

        def solve(H):
            return pt.tree(H, linkage)

    def loop():
        with quiet_stderr():
            return [solve(hamming(bm.pairwise_counts(w[0], w[1]).astype(np.int64))) for w in sub]

    want = loop()
    t0 = time.perf_counter()
    loop()
    t = time.perf_counter() - t0
    res = {"how": how, "windows_timed": len(sub), "ms_per_window": round(t * 1e3 / len(sub), 3),
           "scaled_ms": round(t * 1e3 / len(sub) * len(wins), 1), "ratio_to_tree_scan": round(t * 1e3 / len(sub) * len(wins) / call_ms, 1)}
    if linkage == "single" and how.startswith("scipy"):
        with quiet_stderr():
            got = bm.tree_scan(sub, linkage="single")[1]
        res["single_heights_equal_scipy"] = all(sorted(int(x) for x in got[i]["num"]) == sorted(int(x) for x in want[i][:, 2])
                                                for i in range(len(sub)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--baseline-windows", type=int, default=16)
    ap.add_argument("--skip-baselines", action="store_true", help="the tree points alone (the run under IMPOP_TREE_WIDE=1)")
    ap.add_argument("--out")
    a = ap.parse_args()
    ctx = impop_amd.Context(0)
    res = {"bench": "tree_scan", "device": ctx.device_name(), "n_hap": N_HAP, "windows": a.windows,
           "passes": "median of 5 after 3 warm-up; spread = max - min",
           "sums": "uint64 forced (IMPOP_TREE_WIDE=1)" if os.environ.get("IMPOP_TREE_WIDE") == "1" else "uint32 where they fit",
           "not_measured": "no counter run: the split of the tree kernel between the barriers of its dependent steps, the rescanned rows and "
                           "the strided column stores is unattributed beyond what the run with 64-bit sums shows"}
    full = ctx.synthetic(N_HAP, 50000 * a.windows, seed=SEED, keep_hap_major=True)
    wins = [(i * 50000, (i + 1) * 50000, 50000) for i in range(a.windows)]
    five = []
    for p in range(5):
        f = np.zeros(N_HAP, np.uint8)
        f[p::6] = 1
        five.append(f)
    comp = full.compact()
    for name, bm in (("dense", full), ("compact", comp)):
        r = {}
        for linkage in LINKAGES:
            r[linkage] = point(ctx, bm, wins, linkage, None)
            r[linkage + "_five_panels"] = point(ctx, bm, wins, linkage, five)
            if name == "dense" and not a.skip_baselines:
                r[linkage + "_host_baseline"] = baseline(bm, wins, linkage, a.baseline_windows, r[linkage]["call_ms"])
        if not a.skip_baselines:
            r.update(same_gram_pass(ctx, bm, wins))
        res[name] = r
    comp.free()
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
