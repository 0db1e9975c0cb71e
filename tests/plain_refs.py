"""Plain host references (numpy / pure Python, exact) for the upper-range GPU tests.

Every function here is written as a different algorithm from both the HIP kernel it checks and the C oracle
(oracle/impop_oracle.c), so that one misreading cannot sit in all three:

  ref_components   quick-find union-find over both orientations of the table (kernel: min-label propagation with
                   pointer jumping; oracle: parent-pointer union-find)
  ref_ehh          partition refinement, site by site (kernel: first differing site of every pair; oracle: pair loop)
  ref_afs / ref_site_counts / ref_scan_ints / ref_multi_ints
                   int64 column sums of the unpacked 0/1 matrix (kernels: popcounts over the SB64 layout and the
                   rare-entry stream)
  ref_pair_terms   a Python loop in the operation order of pica2.py:125-145

tests/test_plain_refs.py pins each of them to the goldens and the oracle on small shapes; no GPU is needed there."""
import numpy as np


# ---- af.cluster -------------------------------------------------------------------------------------------------------

def ref_components(adj_bool):
    """Connected components of a dense boolean relation, either orientation of a pair linking it.
    -> (cluster_of [n], K, sizes [K]), clusters ordered by (-size, smallest member) (af.py:43: equal sizes compare their
    sorted member lists, and disjoint sorted lists compare by their first entry)."""
    a = np.asarray(adj_bool, dtype=bool)
    n = a.shape[0]
    if n == 0:
        return np.zeros(0, np.int64), 0, np.zeros(0, np.int64)
    assert a.shape == (n, n)
    sym = a | a.T
    lab = np.arange(n, dtype=np.int64)  # quick-find: lab[i] = smallest member of i's set so far
    for i in range(n):
        nb = np.flatnonzero(sym[i])
        if nb.size == 0:
            continue
        li = lab[i]
        ls = lab[nb]
        if not (ls != li).any():
            continue
        merge = np.unique(np.append(ls, li))
        keep = merge[0]
        lab[np.isin(lab, merge[1:])] = keep
    size = np.bincount(lab, minlength=n)
    roots = np.flatnonzero(size)
    order = sorted(roots.tolist(), key=lambda r: (-int(size[r]), r))
    rank = np.full(n, -1, dtype=np.int64)
    rank[order] = np.arange(len(order))
    return rank[lab], len(order), size[order].astype(np.int64)


def adjacency(ident, threshold):
    """{identity >= threshold} of a dense table with NaN holes (non-strict, af.py:38)"""
    t = np.asarray(ident, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ~np.isnan(t) & (t >= threshold)


# ---- EHH --------------------------------------------------------------------------------------------------------------

def ref_ehh(m01, members=None, reverse=False):
    """calc_EHH (ehhgfa.py:6-21) of the rows flagged in `members` (n flags; None = all) of the 0/1 window m01 [n, W], by
    partition refinement: a group id per member, every group split by the column's bit; pairs(i) = sum C(size, 2).
    -> list of W floats; fewer than two members -> [500.0] * W."""
    m = np.asarray(m01)
    if members is not None:
        m = m[_rows(members, m.shape[0], True)]
    k, W = m.shape
    if k < 2:
        return [500.0] * W
    if reverse:
        m = m[:, ::-1]
    denom = k * (k - 1) / 2
    gid = np.zeros(k, dtype=np.int64)
    out = []
    pairs = k * (k - 1) // 2
    for i in range(W):
        if pairs:
            key = 2 * gid + (m[:, i] != 0)
            present = np.bincount(key, minlength=2 * k) > 0
            gid = (np.cumsum(present) - 1)[key]
            sz = np.bincount(gid).astype(np.int64)
            pairs = int((sz * (sz - 1) // 2).sum())
        out.append(round(pairs / denom, 3))
    return out


# ---- per-site counts, spectra, scan sums ------------------------------------------------------------------------------------

def _rows(flags, n, none_is_all):
    if flags is None:
        return np.ones(n, bool) if none_is_all else np.zeros(n, bool)
    f = np.asarray(flags).astype(bool).ravel()
    assert f.size == n
    return f


def column_counts(m01, rows=None):
    """int64 carriers per column among the rows flagged in `rows` (None = all)"""
    m = np.asarray(m01)
    if rows is None:
        return m.sum(axis=0, dtype=np.int64)
    f = _rows(rows, m.shape[0], True)
    if not f.any():
        return np.zeros(m.shape[1], np.int64)
    return m[f].sum(axis=0, dtype=np.int64)


def ref_site_counts(m01, rows, site_begin, site_end, counts=None):
    """counts: column_counts(m01, rows) computed earlier, to spare the pass over a large matrix"""
    return (column_counts(m01, rows) if counts is None else counts)[site_begin:site_end]


def ref_afs(m01, rows, windows, counts=None):
    """out[w, c] = #sites of window w with c carriers among `rows` (None = all); counts as in ref_site_counts"""
    m = np.asarray(m01)
    c = column_counts(m, rows) if counts is None else counts
    nP = m.shape[0] if rows is None else int(_rows(rows, m.shape[0], True).sum())
    out = np.zeros((len(windows), nP + 1), dtype=np.int64)
    for k, w in enumerate(windows):
        out[k] = np.bincount(c[int(w[0]):int(w[1])], minlength=nP + 1)
    return out


SCAN_INT_KEYS = ("n_sites", "s_all", "s_p", "s_a", "s_b", "sum_p", "sum_a", "sum_b", "sum_ab")


def ref_scan_ints(m01, P, A, B, windows):
    """The integer fields of impop_window_stats for every window: P None = all haplotypes, A / B None = empty; haplotypes in
    both A and B leave both (h-fst.py:181-185).  -> list of dicts (Python ints)."""
    m = np.asarray(m01)
    n = m.shape[0]
    fP, fA, fB = _rows(P, n, True), _rows(A, n, False), _rows(B, n, False)
    both = fA & fB
    fA, fB = fA & ~both, fB & ~both
    nP, nA, nB = int(fP.sum()), int(fA.sum()), int(fB.sum())
    c = column_counts(m, None)
    cP, cA, cB = column_counts(m, fP), column_counts(m, fA), column_counts(m, fB)
    seg = lambda cc, nn: ((cc > 0) & (cc < nn)).astype(np.int64)
    cols = {"s_all": seg(c, n), "s_p": seg(cP, nP), "s_a": seg(cA, nA), "s_b": seg(cB, nB),
            "sum_p": cP * (nP - cP), "sum_a": cA * (nA - cA), "sum_b": cB * (nB - cB),
            "sum_ab": cA * (nB - cB) + cB * (nA - cA)}
    pre = {k: np.concatenate([[0], np.cumsum(v, dtype=np.int64)]) for k, v in cols.items()}
    out = []
    for w in windows:
        s0, s1 = int(w[0]), int(w[1])
        r = {"n_sites": s1 - s0}
        for k in cols:
            r[k] = int(pre[k][s1] - pre[k][s0]) if s1 > s0 else 0
        out.append(r)
    return out


def ref_multi_ints(m01, pops, windows):
    """Per window the K sums  sum_s c_k (n_k - c_k)  and, for the pairs k < l in row-major order, the K(K-1)/2 sums
    sum_s c_k (n_l - c_l) + c_l (n_k - c_k)  that impop_scan_multi accumulates.  -> (within [n_win, K], between [n_win, NP],
    pop sizes [K]) as int64."""
    m = np.asarray(m01)
    n = m.shape[0]
    fl = [_rows(p, n, False) for p in pops]
    K = len(fl)
    nk = [int(f.sum()) for f in fl]
    ck = [column_counts(m, f) for f in fl]
    cols = [ck[k] * (nk[k] - ck[k]) for k in range(K)]
    for k in range(K):
        for l in range(k + 1, K):
            cols.append(ck[k] * (nk[l] - ck[l]) + ck[l] * (nk[k] - ck[k]))
    pre = [np.concatenate([[0], np.cumsum(v, dtype=np.int64)]) for v in cols]
    tot = np.array([[int(p[max(int(w[1]), int(w[0]))] - p[int(w[0])]) for p in pre] for w in windows], dtype=np.int64).reshape(len(windows), len(cols))
    return tot[:, :K], tot[:, K:], np.array(nk, dtype=np.int64)


# ---- pica2 Step 2 -----------------------------------------------------------------------------------------------------

def ref_pair_terms(ident, round_digits, rep, group_size):
    """pica2.py:125-145 for given groups: for g < h in row-major order sim = round(ident[rep_g, rep_h], r) (NaN stays NaN, r None
    or < 0 = no rounding) and (1 - sim) * f_g * f_h with f = size / sum(size), in the reference's operation order
    (freq_i = len / total; pair_value = (1 - similarity) * freq_i * freq_j).  The pair is read as the reference keys it,
    (smaller index, larger index) (pica2.py:86).  -> (sims, values) float64 arrays."""
    t = np.asarray(ident, dtype=np.float64)
    rep = [int(r) for r in rep]
    size = [int(s) for s in group_size]
    total = sum(size)
    G = len(rep)
    sims, vals = [], []
    for g in range(G):
        fg = size[g] / total
        for h in range(g + 1, G):
            a, b = (rep[g], rep[h]) if rep[g] <= rep[h] else (rep[h], rep[g])
            s = float(t[a, b])
            if round_digits is not None and round_digits >= 0 and s == s:
                s = round(s, round_digits)
            fh = size[h] / total
            sims.append(s)
            vals.append((1 - s) * fg * fh)
    return np.array(sims, dtype=np.float64), np.array(vals, dtype=np.float64)
