"""Inputs and call sequences of tests/test_gpu_pairwise_panel.py that also run in the child processes it starts (another
IMPOP_PAIRWISE_CHUNK / IMPOP_GRAM_U16, or IMPOP_TRACE=1: all read once per process).  Seeded: parent and child build the same
matrices, so their records can be compared byte for byte.

    python tests/panel_cases.py front OUT.npz     the inherited-front-end cases, every record of every case
    python tests/panel_cases.py trace OUT.npz     the calls whose [impop_gram] / route lines the parent reads, between @@ markers
"""
import sys

import numpy as np

KW = dict(kind="match", threshold=0.999, round_digits=5)


def founders(rng, n, W, nf=8, pf=0.004, pp=0.0008):
    anc = rng.integers(0, 2, size=W, dtype=np.uint8)
    f = np.repeat(anc[None, :], nf, axis=0) ^ (rng.random((nf, W)) < pf).astype(np.uint8)
    m = f[rng.integers(0, nf, size=n)].copy()
    m ^= (rng.random((n, W)) < pp).astype(np.uint8)
    return m


def panels(rng, n, sizes):
    """disjoint membership flags of the given sizes under a random permutation of the haplotypes"""
    perm = rng.permutation(n)
    pops, o = [], 0
    for s in sizes:
        f = np.zeros(n, np.uint8)
        f[perm[o: o + s]] = 1
        o += s
        pops.append(f)
    return pops


def blob(res):
    """the three arrays of one call (or of several calls, window-wise concatenated) as one byte string"""
    if isinstance(res, list):
        res = tuple(np.concatenate(x) for x in zip(*res))
    return np.frombuffer(b"".join(np.ascontiguousarray(a).tobytes() for a in res), dtype=np.uint8)


def reference_inputs():
    """the five reference panels (run_tajd_panels.sh / run_h_fst_panels.sh sizes) on 465 haplotypes: class boundaries inside 64-wide
    words, 5 haplotypes in no panel; a full, an unaligned, an empty and a one-site window without seq_len"""
    rng = np.random.default_rng(77)
    n, W = 465, 4000
    m = founders(rng, n, W)
    pops = panels(rng, n, [140, 88, 100, 60, 72])
    wins = [(0, W, W), (100, 1777, 50000), (2000, 2000, 5), (3999, 4000, 0)]
    return m, pops, wins


def front_cases(ctx):
    """name -> bytes of every record: sliding windows (shared segments), tilings, windows of >= 65536 sites (int32 counts),
    compacted and weighted matrices.  The equalities between the cases are asserted by the test; a child process under another
    chunk size or count width must return the same bytes for every case."""
    rng = np.random.default_rng(2024)
    n, W = 70, 70000
    m = founders(rng, n, W)
    pops = panels(rng, n, [30, 17, 20])
    out = {}
    bm = ctx.upload_dense(m, keep_hap_major=True)
    sliding = [(k * 5000, k * 5000 + 10000, 10000) for k in range(8)]  # 10 kb windows every 5 kb
    tiling = [(k * 3000 + 7, k * 3000 + 2900, 3000) for k in range(12)] + [(100, 100, 5)]
    big = [(0, W, W), (1234, 67000, 0)]
    out["sliding"] = blob(bm.pairwise_scan_panel(sliding, pops, **KW))
    out["sliding_each"] = blob([bm.pairwise_scan_panel([w], pops, **KW) for w in sliding])
    out["tiling"] = blob(bm.pairwise_scan_panel(tiling, pops, **KW))
    out["tiling_again"] = blob(bm.pairwise_scan_panel(tiling, pops, **KW))
    out["tiling_scope1"] = blob(bm.pairwise_scan_panel(tiling, pops, s_scope=1, **KW))
    out["big"] = blob(bm.pairwise_scan_panel(big, pops, **KW))
    out["big_again"] = blob(bm.pairwise_scan_panel(big, pops, **KW))
    bc = bm.compact()
    out["compact_sliding"] = blob(bc.pairwise_scan_panel(sliding, pops, **KW))
    out["compact_tiling"] = blob(bc.pairwise_scan_panel(tiling, pops, **KW))
    bc.free()
    bm.free()
    # node-level matrix with node lengths as site weights against its bp-expanded form (S counts columns on the one and base
    # pairs on the other: compared without S, s_scope 2)
    Wn = 3000
    wt = rng.integers(1, 40, size=Wn).astype(np.uint32)
    pre = np.concatenate([[0], np.cumsum(wt)]).astype(np.int64)
    node_wins = [(k * 250 + 3, k * 250 + 240, int(pre[k * 250 + 240] - pre[k * 250 + 3])) for k in range(12)]
    bp_wins = [(int(pre[a]), int(pre[b]), L) for a, b, L in node_wins]
    bw = ctx.upload_dense(m[:, :Wn], keep_hap_major=True)
    bw.set_site_weights(wt)
    out["weighted"] = blob(bw.pairwise_scan_panel(node_wins, pops, s_scope=2, **KW))
    out["weighted_S"] = blob(bw.pairwise_scan_panel(node_wins, pops, **KW))
    bwc = bw.compact()
    out["weighted_compact_S"] = blob(bwc.pairwise_scan_panel(node_wins, pops, **KW))
    bwc.free()
    bw.free()
    be = ctx.upload_dense(np.repeat(m[:, :Wn], wt, axis=1), keep_hap_major=True)
    out["expanded"] = blob(be.pairwise_scan_panel(bp_wins, pops, s_scope=2, **KW))
    be.free()
    return out


def trace_calls(ctx):
    """the calls whose trace lines the parent reads; results that the parent (or this process) compares"""
    out = {}
    m, pops, _ = reference_inputs()
    bm = ctx.upload_dense(m, keep_hap_major=True)
    wins = [(k * 300 + k % 7, k * 300 + 300 - (k % 5) * 37, 300) for k in range(12)]
    sys.stderr.write("@@pairwise\n"); sys.stderr.flush()
    bm.pairwise_scan(wins, None, pops[0], pops[1], s_scope=2, **KW)
    sys.stderr.write("@@panel\n"); sys.stderr.flush()
    out["reference12"] = blob(bm.pairwise_scan_panel(wins, pops, **KW))
    sys.stderr.write("@@dice\n"); sys.stderr.flush()
    dice = bm.pairwise_scan_panel(wins[:3], pops, kind="dice", threshold=0.999, round_digits=5)
    sys.stderr.write("@@end\n"); sys.stderr.flush()
    out["dice"] = blob(dice)
    p = 0
    for k in range(5):  # the general route IS launch_hfst per pair on the same counts: the Fst fields are pairwise_scan's, byte for byte
        for l in range(k + 1, 5):
            two = bm.pairwise_scan(wins[:3], None, pops[k], pops[l], kind="dice", threshold=0.999, round_digits=5, s_scope=2)
            for key in ("fst", "pi_a", "pi_b", "pi_xy", "dxy", "da"):
                assert dice[1][:, p][key].tobytes() == two[key].tobytes(), ("dice", k, l, key)
            p += 1
    bm.free()
    rng = np.random.default_rng(513)
    n, W = 513, 2000
    m = founders(rng, n, W)
    pops = panels(rng, n, [200, 13, 300])
    bm = ctx.upload_dense(m, keep_hap_major=True)
    wins = [(0, W, W), (100, 1777, 50000), (2000, 2000, 5)]
    sys.stderr.write("@@n513\n"); sys.stderr.flush()
    res = bm.pairwise_scan_panel(wins, pops, **KW)
    sys.stderr.write("@@end513\n"); sys.stderr.flush()
    out["n513"] = blob(res)
    p = 0
    for k in range(3):
        one = bm.pairwise_scan(wins, pops[k], None, None, **KW)
        for key in ("pi", "pi_site", "tajima_d", "n_groups"):
            assert res[0][:, k][key].tobytes() == one[key].tobytes(), ("n513 panel", k, key)
        for l in range(k + 1, 3):
            two = bm.pairwise_scan(wins, None, pops[k], pops[l], s_scope=2, **KW)
            for key in ("fst", "pi_a", "pi_b", "pi_xy", "dxy", "da"):
                assert res[1][:, p][key].tobytes() == two[key].tobytes(), ("n513", k, l, key)
            p += 1
    bm.free()
    return out


if __name__ == "__main__":
    import impop_amd
    c = impop_amd.Context(0)
    np.savez(sys.argv[2], **(front_cases(c) if sys.argv[1] == "front" else trace_calls(c)))
    c.close()
