#!/usr/bin/env python3
"""Generate tests/golden/af_windows.json by running the REAL reference's scripts/af.py (pangenome/impop) on the `.sim` rows of
windows of small seeded bit matrices.  The reference is imported by file path at generation time (like oracle/gen_golden.py);
nothing of it is copied: the fixture holds inputs (bit matrices, PanSN names, windows, thresholds, the .sim rows with their
identities written with repr) and the reference's outputs (af.cluster's lists, write_summary's rows).

Usage: python3 tools/gen_af_golden.py [--ref /root/reference] [--out tests/golden/af_windows.json]
"""
from __future__ import annotations

import argparse
import base64
import importlib.util
import io
import json
import os
import sys
import tempfile

import numpy as np

sys.dont_write_bytecode = True


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def pack_rows(m01):
    n, W = m01.shape
    words = (W + 63) // 64
    pad = np.zeros((n, words * 64), dtype=np.uint8)
    pad[:, :W] = m01
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint64).reshape(n, words)


def make_case(seed, n, n_site, shuffle_names):
    rng = np.random.default_rng(seed)
    founders = rng.integers(0, 2, size=(3, n_site), dtype=np.uint8)
    m = np.zeros((n, n_site), np.uint8)
    for i in range(n):
        m[i] = founders[i % 3]
        if i % 4 == 1:    # one site per 100 away from its founder: chains at thresholds below 1
            m[i, rng.integers(0, 100) + 100 * np.arange(n_site // 100)] ^= 1
        elif i % 4 == 3:  # far from everything
            m[i, rng.choice(n_site, size=n_site // 8, replace=False)] ^= 1
    samples = [f"HG{(i // 2):03d}#{(i % 2) + 1}#chrT" for i in range(n)]
    if shuffle_names:
        samples = [samples[k] for k in rng.permutation(n)]
    return m, [f"{s}:0-{n_site}" for s in samples]


def sim_rows(m, names, b, e):
    """the rows `impg similarity` lists for the window: every unordered pair (diagonal included) once, `match` identity"""
    W = e - b
    rows = []
    for i in range(len(names)):
        for j in range(i, len(names)):
            H = int((m[i, b:e] != m[j, b:e]).sum())
            rows.append((names[i], names[j], repr((W - H) / W if W else 1.0)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "af_windows.json"))
    args = ap.parse_args()
    af = load("ref_af", os.path.join(args.ref, "scripts", "af.py"))
    cases = []
    for seed, n, n_site, shuffle in ((11, 12, 600, False), (12, 14, 500, True)):
        m, names = make_case(seed, n, n_site, shuffle)
        windows = []
        plan = [(0, 200, 1.0), (200, 400, 1.0), (100, 500, 1.0), (0, n_site, 1.0), (0, 200, 0.995), (100, 300, 0.995), (0, n_site, 0.99),
                (150, 450, 0.9)]
        for b, e, thr in plan:
            rows = sim_rows(m, names, b, e)
            with tempfile.TemporaryDirectory() as td:
                path = os.path.join(td, "loc.sim")
                with open(path, "w") as f:
                    f.write("group.a\tgroup.b\testimated.identity\n")
                    f.writelines(f"{a}\t{c}\t{v}\n" for a, c, v in rows)
                ref_rows, ref_samples = af.load_pairs(path)
            clusters = af.cluster(ref_rows, ref_samples, thr)
            summary = af.build_summary(clusters)
            buf = io.StringIO(newline="")
            af.write_summary(summary, buf)
            lines = buf.getvalue().split("\r\n")
            assert lines[0] == "cluster_id\tcount\tfrequency" and lines[-1] == ""
            windows.append({"begin": b, "end": e, "threshold": thr, "sim": [list(r) for r in rows], "clusters": clusters,
                            "summary_rows": lines[1:-1]})
        cases.append({"n": n, "n_site": n_site, "names": names, "bits_u64_b64": base64.b64encode(pack_rows(m).tobytes()).decode(),
                      "windows": windows})
    with open(args.out, "w") as f:
        json.dump({"generator": "tools/gen_af_golden.py", "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
