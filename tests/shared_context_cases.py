"""Inputs of the tests of scan plans that share one context (test_gpu_scan_shared_context.py, and on the host
test_scan_shared_context_host.py): the matrices, subset masks, window lists and the CPU oracle's records.  A helper module.

Every plan reads Tajima's constants for ITS nP; a plan that finalizes with another plan's constants gets tajima_d wrong and
nothing else.  So the inputs are chosen for D: n_hap = 465 haplotypes, every site common (carrier frequency 0.15 .. 0.85, so
every site segregates in all rows and in every subset of 40), windows with a sequence length, subsets P of 465 (None), 40, 2
and 1 haplotypes.  A plan of the three finalize variants each: 64 windows of 50 sites ("w64": at most two 64-site blocks a
window, so at most two tiles, one thread per window), one window of 3 990 sites at tile_blocks 1 ("mid": more than 48 tiles, 64
threads per window) and one of 132 008 sites at tile_blocks 1 ("big": more than 2 048 tiles, 256 threads per window)."""
import functools
from typing import NamedTuple

import numpy as np

N = 465
S_SMALL = 4173
S_BIG = 64 * 2062 + 45  # 2 063 blocks of 64 sites, the last one partial
SEED_SMALL, SEED_BIG, SEED_NODES = 20261, 20262, 20263
SIZES = (465, 40, 2, 1)
PAIRS = ((40, 465), (465, 40), (2, 40))  # (plan A's |P|, plan B's |P|)
K_NODES = 900

INT_KEYS = ("n_sites", "s_all", "s_p", "s_a", "s_b", "sum_p", "sum_a", "sum_b", "sum_ab")
DBL_KEYS = ("pi", "pi_site", "pi_a", "pi_b", "pi_xy", "dxy", "da", "fst", "tajima_d")

WINDOWS = {
    "w64": [(7 + 61 * i, 7 + 61 * i + 50, (50, 1, 50000, 777)[i % 4]) for i in range(64)],
    "mid": [(5, 3995, 3990)],
    "big": [(3, S_BIG - 2, 50000)],
    "pw": [(0, 700, 700), (650, 2000, 50000), (2100, 2164, 64)],  # the all-pairs calls between the plan launches
    "nodes": [(0, K_NODES, 0), (3, 500, 12345), (K_NODES // 2, K_NODES // 2 + 1, 7), (K_NODES - 64, K_NODES, 99)]
             + [(40 * i + 3, 40 * i + 90, 1000 + i) for i in range(20)],
}


class Spec(NamedTuple):
    """one plan: the matrix it scans, its window list, |P|, the wiring of D, the tiling, and whether it takes a tile digest"""
    kind: str          # "small" | "big" | "crafted" | "weighted"
    windows: str       # a key of WINDOWS, or "crafted"
    psize: int
    d_pi_mode: int = 0
    s_scope: int = 0
    tile_blocks: int = 0
    digest: bool = False


def _common_sites(S, seed):
    rng = np.random.default_rng(seed)
    f = rng.uniform(0.15, 0.85, S)
    m = np.empty((N, S), np.uint8)
    for s0 in range(0, S, 8192):  # in slices: the big matrix as one array of random floats would be a quarter of a gigabyte
        s1 = min(s0 + 8192, S)
        m[:, s0:s1] = rng.random((N, s1 - s0), dtype=np.float32) < f[None, s0:s1]
    return m


@functools.lru_cache(maxsize=None)
def matrix(kind):
    """the 0/1 matrix [N, sites] that upload_dense takes"""
    if kind == "small":
        return _common_sites(S_SMALL, SEED_SMALL)
    if kind == "big":
        return _common_sites(S_BIG, SEED_BIG)
    if kind == "crafted":  # a matrix whose plans take a tile digest: the crafted one of test_gpu_scan_joint_issue
        import test_gpu_scan_joint_issue as J
        return J._crafted(N, 2700 + N)
    assert kind == "weighted"
    return nodes()[0]


@functools.lru_cache(maxsize=None)
def nodes():
    """the weighted matrix: one column per node with a weight; three in ten nodes carried by every haplotype, one in ten by
    none, which compaction drops -> (nodes [N, K_NODES], weights)"""
    rng = np.random.default_rng(SEED_NODES)
    m = (rng.random((N, K_NODES)) < rng.uniform(0.15, 0.85, K_NODES)[None, :]).astype(np.uint8)
    u = rng.random(K_NODES)
    m[:, u < 0.3] = 1
    m[:, u > 0.9] = 0
    return m, rng.integers(1, 40, size=K_NODES).astype(np.uint32)


def windows(spec):
    if spec.windows == "crafted":
        import test_gpu_scan_joint_issue as J
        return J.LISTS[3]
    return WINDOWS[spec.windows]


def mask_p(size):
    """the subset of `size` haplotypes as 0/1 flags; None for all of them"""
    if size == N:
        return None
    P = np.zeros(N, np.uint8)
    P[np.random.default_rng(1000 + size).choice(N, size, replace=False)] = 1
    return P


def masks_ab():
    A = np.zeros(N, np.uint8); A[:140] = 1
    B = np.zeros(N, np.uint8); B[140:240] = 1
    return A, B


def panels():
    """three disjoint panels of three sizes for impop_pairwise_scan_panel"""
    out, o = [], 0
    for s in (30, 77, 140):
        f = np.zeros(N, np.uint8); f[o: o + s] = 1; o += s
        out.append(f)
    return out


@functools.lru_cache(maxsize=None)
def _packed(kind):
    from oracle import oracle
    if kind == "weighted":
        m, w = nodes()
        return oracle.pack_hap_major(np.repeat(m, w, axis=1))
    return oracle.pack_hap_major(matrix(kind))


@functools.lru_cache(maxsize=None)
def want(spec):
    """the CPU oracle's record of every window of the plan -> list of dicts"""
    from oracle import oracle
    bits = _packed(spec.kind)
    P = mask_p(spec.psize)
    A, B = masks_ab()
    mp = oracle.pack_mask(np.ones(N, np.uint8) if P is None else P)
    ma, mb = oracle.pack_mask(A), oracle.pack_mask(B)
    out = []
    if spec.kind != "weighted":
        for s0, s1, sl in windows(spec):
            out.append(oracle.window_sitecount(bits, N, s0, s1, mp, ma, mb, sl, spec.d_pi_mode, spec.s_scope))
        return out
    # a weighted column is its weight in identical base pairs: the sums, n_sites and every pi of the expanded matrix, but the
    # segregating-site counts count NODES, and Tajima's D follows from that S (test_weighted_sites_equal_bp_expanded_matrix)
    m, w = nodes()
    cum = np.concatenate(([0], np.cumsum(w))).astype(np.int64)
    rows = {"all": np.ones(N, bool), "p": np.ones(N, bool) if P is None else P.astype(bool), "a": A.astype(bool), "b": B.astype(bool)}
    for a, b, sl in windows(spec):
        r = oracle.window_sitecount(bits, N, int(cum[a]), int(cum[b]), mp, ma, mb, sl, spec.d_pi_mode, spec.s_scope)
        for key, sel in rows.items():
            c, k = m[sel, a:b].sum(axis=0), int(sel.sum())
            r["s_" + key] = int(((c > 0) & (c < k)).sum())
        S = float(r["s_all"] if spec.s_scope == 0 else r["s_p"])
        W = float(cum[b] - cum[a])
        pin = oracle.py_round(r["pi_site"], 8) if spec.d_pi_mode == 0 else r["pi_site"] if spec.d_pi_mode == 1 else r["pi"] * W
        r["tajima_d"] = oracle.tajimas_d(spec.psize, S, pin)[0] if spec.psize >= 2 and pin == pin else float("nan")
        out.append(r)
    return out


def d_with_n(spec, n_consts):
    """Tajima's D of every window of the plan, through the oracle, from the window's own S and pi but the constants of
    n_consts haplotypes: what a finalize kernel that read another plan's constants would write (n_consts = spec.psize: the
    right value).  Like the plans, a subset of fewer than two haplotypes stands for n = 2 in the constants."""
    from oracle import oracle
    assert spec.kind != "weighted" and spec.d_pi_mode == 0
    out = []
    for (s0, s1, sl), r in zip(windows(spec), want(spec)):
        S = float(r["s_all"] if spec.s_scope == 0 else r["s_p"])
        pin = oracle.py_round(r["pi_site"], 8)
        out.append(oracle.tajimas_d(max(n_consts, 2), S, pin)[0] if spec.psize >= 2 and pin == pin else float("nan"))
    return out
