"""A plain numpy restatement of impop_kinship_scan, straight from the 0/1 matrix: genotypes g = m[h1] + m[h2], the joint genotype
table of a pair by counting the sites with (g_i, g_j) = (a, b).  No heterozygous / homozygous bit planes, no Gram entries.  The
counting is nine 0/1 indicator products per window (float32 sums of ones below 2^24: exact)."""
import numpy as np

KIN_WINDOW_DTYPE = np.dtype([("n_ind", "<u4"), ("n_sites", "<u4"), ("n_pairs", "<u8"), ("het_het", "<u8"), ("ibs0", "<u8"), ("ibs2", "<u8"),
                             ("n_related", "<u4"), ("n_undefined", "<u4")])
KIN_PAIR_DTYPE = np.dtype([("t", "<u8", (9,))])
KIN_WATCH_DTYPE = np.dtype([("het_het", "<u4"), ("ibs0", "<u4"), ("het_i", "<u4"), ("het_j", "<u4")])


def genotypes(m01, pairs):
    """[N, sites] of 0 / 1 / 2"""
    pr = np.asarray(pairs).reshape(-1, 2)
    return m01[pr[:, 0]].astype(np.int8) + m01[pr[:, 1]].astype(np.int8)


def pair_order(N):
    return [(a, b) for a in range(N) for b in range(a + 1, N)]


def window_tables(g, b, e):
    """-> [N, N, 9] int64: cell 3 a + b of (i, j) = #{s in [b, e) : g_i(s) = a and g_j(s) = b}"""
    assert e - b < 2 ** 24
    ind = [(g[:, b:e] == a).astype(np.float32) for a in range(3)]
    N = g.shape[0]
    T = np.zeros((N, N, 9), np.int64)
    for a in range(3):
        for c in range(3):
            T[:, :, 3 * a + c] = np.rint(ind[a] @ ind[c].T).astype(np.int64)
    return T


def het_of(g, b, e):
    return (g[:, b:e] == 1).sum(axis=1).astype(np.int64)


def related(het_i, het_j, het_het, ibs0, num, den):
    """KING-robust >= num / den, in integers; m = 0 is never related"""
    m = np.minimum(het_i, het_j)
    return (m > 0) & (den * (2 * (het_het - 2 * ibs0) + 2 * m - het_i - het_j) >= 4 * m * num)


def scan(m01, pairs, wins, kin=(884, 10000), watch=()):
    """-> (windows KIN_WINDOW_DTYPE [n_windows], pair totals KIN_PAIR_DTYPE [N(N-1)/2], watch rows KIN_WATCH_DTYPE [n_windows, n_watch])"""
    g = genotypes(m01, pairs)
    N = g.shape[0]
    iu = np.triu_indices(N, 1)  # row-major: the pair order (0,1),(0,2),..,(1,2),..
    out = np.zeros(len(wins), KIN_WINDOW_DTYPE)
    tot = np.zeros((N * (N - 1) // 2, 9), np.int64)
    wat = np.zeros((len(wins), len(watch)), KIN_WATCH_DTYPE)
    for w, win in enumerate(wins):
        b, e = int(win[0]), int(win[1])
        T = window_tables(g, b, e)
        het = het_of(g, b, e)
        t = T[iu]
        hh, i0, i2 = t[:, 4], t[:, 2] + t[:, 6], t[:, 0] + t[:, 4] + t[:, 8]
        a, c = het[iu[0]], het[iu[1]]
        out[w] = (N, e - b, len(t), hh.sum(), i0.sum(), i2.sum(), related(a, c, hh, i0, kin[0], kin[1]).sum(), (np.minimum(a, c) == 0).sum())
        tot += t
        for q, (i, j) in enumerate(watch):
            wat[w, q] = (T[i, j, 4], T[i, j, 2] + T[i, j, 6], het[i], het[j])
    pairs_out = np.zeros(len(tot), KIN_PAIR_DTYPE)
    pairs_out["t"] = tot
    return out, pairs_out, wat


def planes(m01, pairs):
    """the XOR and AND planes impop_genotypes_download returns, as 0/1 rows: [2N, sites], H then A"""
    pr = np.asarray(pairs).reshape(-1, 2)
    return np.concatenate([m01[pr[:, 0]] ^ m01[pr[:, 1]], m01[pr[:, 0]] & m01[pr[:, 1]]])
