"""Inputs of the windowed-clustering tests (tests/test_gpu_cluster_scan.py), kept apart so that the CPU suite can check that
they mean something (tests/test_cluster_scan_host.py) without a GPU.

planted_matrix: a 0/1 matrix [n, n_seg * SEG] whose windows (one or two segments of SEG sites) cluster non-trivially at
THRESHOLD under both identity kinds:
  * chains: member k of a chain differs from member k + 1 at ONE site per active segment and from member k + 2 at two, so over a
    two-segment window neighbours are 2 sites apart (linked) and next-but-one neighbours 4 (not linked): a component that is
    no clique, where af's transitive closure and pica2's seed-only grouping part ways.  A chain is inactive in every third
    segment (its members scatter there), so the windows differ;
  * copies: every fourth other haplotype is an exact copy of one of six founders (cliques of nearly equal size: ties);
  * the rest carry their founder plus private flips in every segment (singletons)."""
import numpy as np

SEG = 128
THRESHOLD = 0.988  # a window of 256 sites: 3 differences link under `match` (253/256 = 0.98828), 4 do not (0.98438)


def planted_matrix(n, n_seg, seed):
    rng = np.random.default_rng(seed)
    S = n_seg * SEG
    m = np.zeros((n, S), np.uint8)
    founders = rng.integers(0, 2, size=(6, S), dtype=np.uint8)
    chain_len = [5, 5, 4, 3] if n >= 64 else [4, 4]
    row = 0
    for c, L in enumerate(chain_len):
        base = rng.integers(0, 2, size=S, dtype=np.uint8)
        cur = base.copy()
        for k in range(L):
            if k:
                for s in range(n_seg):
                    active = (s + c) % 3 != 0
                    sites = rng.choice(SEG, size=1 if active else 12, replace=False) + s * SEG
                    cur[sites] ^= 1
            m[row] = cur
            row += 1
    for i in range(row, n):
        h = founders[i % 6].copy()
        if i % 4 != 0:
            for s in range(n_seg):
                h[rng.choice(SEG, size=8, replace=False) + s * SEG] ^= 1
        m[i] = h
    return m


def window_lists(n_seg):
    """tiling: two segments each, disjoint; sliding: two segments each, 50 % overlap.  (begin, end, seq_len)"""
    tiling = [(2 * k * SEG, (2 * k + 2) * SEG, 2 * SEG) for k in range(n_seg // 2)]
    sliding = [(k * SEG, (k + 2) * SEG, 2 * SEG) for k in range(n_seg - 1)]
    return {"tiling": tiling, "sliding": sliding}


def subset_flags(n):
    f = np.array([1 if (i < 20 or i % 3 != 2) else 0 for i in range(n)], np.uint8)
    return f


def round_table(t, digits):
    """CPython round(x, digits) of every entry (what pica2 -r sees), through the table's distinct values"""
    if digits is None:
        return t
    u, inv = np.unique(t, return_inverse=True)
    return np.array([round(float(x), digits) for x in u])[inv].reshape(t.shape)


def window_identity(oracle, bits, n, s0, s1, kind, digits, members=None):
    """the identity table of a window as the reference pipeline would hand it to af.py: oracle counts -> oracle identity ->
    rounding; restricted to `members` (indices) when given"""
    I = oracle.pairwise_counts(bits, n, s0, s1)
    t = round_table(oracle.identity(I, s1 - s0, {"match": 0, "dice": 1}[kind]), digits)
    if members is not None:
        t = t[np.ix_(members, members)]
    return t


def seed_only_groups(adj):
    """pica2-style grouping of a symmetric boolean relation: seeds in index order, a seed takes its free neighbours only.
    -> group index per element (to tell a transitive component from a seed's neighbourhood)"""
    n = adj.shape[0]
    g = np.full(n, -1)
    k = 0
    for i in range(n):
        if g[i] >= 0:
            continue
        g[i] = k
        g[(g < 0) & adj[i]] = k
        k += 1
    return g
