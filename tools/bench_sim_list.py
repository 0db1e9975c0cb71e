#!/usr/bin/env python3
"""Throughput of the `.sim` list path: K tables of 465 names are written once, then tables/s of
  (a) the batch driver path in-process (impop_amd.simbatch.run_pipeline), split into host parse and GPU call;
  (b) the per-file drop-in CLIs (scripts/pica2.py) of another checkout, --cli-tree DIR (a built worktree of the parent
      commit), one process after another on a sample of the same files;
  (c) the reference-style chain of oracle/ref_style.py on the same tables with 16 processes (as oracle/ref_style_mp.py runs it).
(c) is ref_style.window_chain on up to 32 of the tables held in memory, without population flags and without reading the
files: a shortcut that favours the baseline.  (a) runs with IMPOP_TRACE=1 (the library's phase events; stderr to a file).
(b) and (c) are the comparison points.  One warm-up pass of (a) is discarded; the median of --repeats passes is reported.
Run on the GPU box with at most 16 CPUs in use:   python tools/bench_sim_list.py --tables 256 --out profiles/r06_sim_list.json"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_tables(d, k, n=465, seed=1):
    rng = np.random.default_rng(seed)
    names = [f"HG{i // 2:05d}#{i % 2 + 1}#CM0{i:05d}.1:1000-51000" for i in range(n)]
    paths, sims = [], []
    for t in range(k):
        sim = 0.998 + 0.002 * rng.random((n, n))
        sim = np.minimum(sim, sim.T)
        p = os.path.join(d, f"w{t:04d}.sim")
        with open(p, "w") as f:
            f.write("group.a\tgroup.b\tgroup.a.length\tgroup.b.length\tintersection\testimated.identity\n")
            for i in range(n):
                f.write("".join(f"{names[i]}\t{names[j]}\t50000\t50000\t49900\t{float(sim[i, j])!r}\n" for j in range(n)))
        paths.append(p)
        sims.append(sim)
    return names, paths, sims


_G = {}


def _ref_one(k):
    from oracle import ref_style
    n = len(_G["names"])
    z = np.zeros(n, np.uint8)
    return ref_style.window_chain(_G["names"], _G["sims"][k % len(_G["sims"])], z, z, 50000, 100)["pi_site"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tables", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cli-tree", help="checkout whose scripts/pica2.py is timed per file (built; e.g. the parent commit)")
    ap.add_argument("--cli-sample", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()
    os.environ["IMPOP_TRACE"] = "1"  # read once by the library: the per-chunk phase times come from its trace lines
    import re
    import impop_amd
    from impop_amd import simbatch
    res = {"command": " ".join(sys.argv), "cpus": "16 (OMP_NUM_THREADS / --threads; never the machine's core count)", "tables": a.tables}
    with tempfile.TemporaryDirectory() as d:
        names, paths, sims = write_tables(d, a.tables)
        rows = [simbatch.SimRow("chr1", 50000 * t, 50000 * t + 50000, p, "100") for t, p in enumerate(paths)]
        # (c) first: the pool forks, which must happen before this process opens the GPU
        import multiprocessing as mp
        _G.update(names=names, sims=sims[: min(a.tables, 32)])
        with mp.get_context("fork").Pool(16) as pool:
            pool.map(_ref_one, range(16))  # warm-up (imports)
            jobs = max(32, len(_G["sims"]))
            t0 = time.perf_counter()
            pool.map(_ref_one, range(jobs), chunksize=1)
            dt = time.perf_counter() - t0
        res["c_ref_style_mp16"] = {"tables_per_s": jobs / dt, "jobs": jobs, "processes": 16,
                                   "note": "oracle/ref_style.py window_chain on the dense tables, as oracle/ref_style_mp.py runs it; file reading not included"}
        ctx = impop_amd.Context(0)
        make = lambda row, tab: {"ident": tab.dense, "seq_len": 50000, "seed_rank": simbatch.seed_rank(tab)}  # noqa: E731
        walls, phases = [], []
        trace_path = os.path.join(d, "trace.txt")
        for rep in range(a.repeats + 1):
            tm = {}
            sys.stderr.flush()
            saved, fd = os.dup(2), os.open(trace_path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC)
            os.dup2(fd, 2)  # the library's trace lines of this pass
            try:
                t0 = time.perf_counter()
                out = simbatch.run_pipeline(ctx, rows, "pica2", make, 0.999, 5, None, n_threads=a.threads, timings=tm)
                w = time.perf_counter() - t0
            finally:
                os.dup2(saved, 2); os.close(saved); os.close(fd)
            for key in ("stage_us", "up_us", "kernels_us", "down_us"):
                tm[key[:-3] + "_s"] = sum(int(v) for v in re.findall(key + r"=(\d+)", open(trace_path).read())) * 1e-6
            assert all(r[0] == "ok" for r in out)
            if rep:
                walls.append(w); phases.append(tm)
        ctx.close()
        med = statistics.median(walls)
        res["a_batch"] = {"tables_per_s": a.tables / med, "wall_s_median": med, "wall_s_all": walls,
                          "parse_s_median": statistics.median(p["parse_s"] for p in phases),
                          "gpu_call_s_median": statistics.median(p["gpu_call_s"] for p in phases),
                          "stage_s_median": statistics.median(p["stage_s"] for p in phases),
                          "upload_s_median": statistics.median(p["up_s"] for p in phases),
                          "kernels_s_median": statistics.median(p["kernels_s"] for p in phases),
                          "download_s_median": statistics.median(p["down_s"] for p in phases),
                          "note": "parse of chunk c+1 overlaps the GPU call of chunk c; gpu_call = Python marshalling + stage (host copy into page-locked memory) + upload + kernels + download"}
        if a.cli_tree:
            ts = []
            for p in paths[: a.cli_sample]:
                t0 = time.perf_counter()
                r = subprocess.run([sys.executable, os.path.join(a.cli_tree, "scripts", "pica2.py"), p, "-t", "0.999", "-r", "5", "-l", "50000",
                                    "-d", d], capture_output=True, text=True)
                assert r.returncode == 0, r.stderr
                ts.append(time.perf_counter() - t0)
            res["b_cli_per_file"] = {"tables_per_s": 1.0 / statistics.median(ts), "s_per_file_median": statistics.median(ts), "files": len(ts)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
