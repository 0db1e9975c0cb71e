"""A plain numpy / Python restatement of impop_pairdist_scan, written from the prose of include/impop_hip.h and from nothing
else: I = X diag(w) X^T in int64, H_ij = a_i + a_j - 2 I_ij, Python integers for sum_h2, a plain loop over the members for the
nearest neighbours, and the one double sum as a left-to-right loop from 0.0.

    gram(m01, s0, s1, weights)            -> I (int64)
    hamming(I)                            -> H (int64)
    window(H, n_sites, pops, bins, width) -> (panel records, pair records, hist_within, hist_between) as Python dicts / lists
    scan(...)                             -> the same packed into the structured arrays the call returns (bytes comparable)
    brute_window(rows, w, pops, bins, width): the definition once more as loops over sites and pairs (n <= 12), to check the above
"""
import numpy as np

NONE = 0xFFFFFFFF
PANEL_DTYPE = np.dtype([("n_members", "<u4"), ("n_sites", "<u4"), ("n_pairs", "<u8"), ("sum_h", "<u8"), ("sum_h2", "<u8"), ("n_zero", "<u8"),
                        ("min_h", "<u4"), ("max_h", "<u4"), ("min_i", "<u4"), ("min_j", "<u4"), ("max_i", "<u4"), ("max_j", "<u4")])
PAIR_DTYPE = np.dtype([("n_pairs", "<u8"), ("sum_h", "<u8"), ("sum_h2", "<u8"), ("n_zero", "<u8"), ("min_h", "<u4"), ("max_h", "<u4"),
                       ("min_i", "<u4"), ("min_j", "<u4"), ("max_i", "<u4"), ("max_j", "<u4"), ("nn_same_a", "<u4"), ("nn_same_b", "<u4"),
                       ("nn_other_a", "<u4"), ("nn_other_b", "<u4"), ("snn", "<f8"), ("gmin", "<f8"), ("reserved", "<u8")])
DIST_FIELDS = ("n_pairs", "sum_h", "sum_h2", "n_zero", "min_h", "max_h", "min_i", "min_j", "max_i", "max_j")


def gram(m01, s0, s1, weights=None):
    X = np.asarray(m01)[:, s0:s1].astype(np.int64)
    w = np.ones(s1 - s0, np.int64) if weights is None else np.asarray(weights, np.int64)[s0:s1]
    return (X * w) @ X.T


def hamming(I):
    a = np.diag(I)
    return a[:, None] + a[None, :] - 2 * I


def _distance_fields(h, ii, jj):
    """h: the distances of a record's pairs in (i, j) order, ii / jj: their haplotype indexes"""
    n = len(h)
    if n == 0:
        return dict(n_pairs=0, sum_h=0, sum_h2=0, n_zero=0, min_h=0, max_h=0, min_i=NONE, min_j=NONE, max_i=NONE, max_j=NONE)
    vals, cnt = np.unique(h, return_counts=True)
    lo, hi = int(np.argmin(h)), int(np.argmax(h))  # the first of the ties in (i, j) order
    return dict(n_pairs=n, sum_h=sum(int(v) * int(c) for v, c in zip(vals, cnt)), sum_h2=sum(int(v) * int(v) * int(c) for v, c in zip(vals, cnt)),
                n_zero=int((h == 0).sum()), min_h=int(h[lo]), max_h=int(h[hi]), min_i=int(ii[lo]), min_j=int(jj[lo]), max_i=int(ii[hi]),
                max_j=int(jj[hi]))


def _hist(h, bins, width):
    if not bins:
        return None
    return np.bincount(np.minimum(h // width, bins - 1), minlength=bins).astype(np.uint32)


def nearest(H, pops):
    """per member of any panel: {panel: (min H, ties)} against every panel, itself excluded"""
    out = {}
    for p in pops:
        for i in p:
            t = {}
            for c, q in enumerate(pops):
                others = q[q != i]
                if len(others):
                    row = H[i, others]
                    d = int(row.min())
                    t[c] = (d, int((row == d).sum()))
            out[int(i)] = t
    return out


def window(H, n_sites, pops, bins=0, width=1):
    pops = [np.asarray(sorted(int(x) for x in p), np.int64) for p in pops]
    K = len(pops)
    panels, pairs, hw, hb = [], [], [], []
    for p in pops:
        a, b = np.triu_indices(len(p), 1)
        h = H[p[a], p[b]]
        r = _distance_fields(h, p[a], p[b])
        r.update(n_members=len(p), n_sites=int(n_sites))
        panels.append(r)
        hw.append(_hist(h, bins, width))
    nn = nearest(H, pops) if K > 1 else None
    for k in range(K):
        for l in range(k + 1, K):
            pk, pl = pops[k], pops[l]
            h = H[np.ix_(pk, pl)].ravel()
            r = _distance_fields(h, np.repeat(pk, len(pl)), np.tile(pl, len(pk)))
            hb.append(_hist(h, bins, width))
            terms = []
            counts = dict(nn_same_a=0, nn_same_b=0, nn_other_a=0, nn_other_b=0)
            in_k = set(pk.tolist())
            for i in sorted([int(x) for x in pk] + [int(x) for x in pl]):
                own, other, side = (k, l, "a") if i in in_k else (l, k, "b")
                cand = [nn[i][c] for c in (own, other) if c in nn[i]]
                d = min(c[0] for c in cand)
                tied = sum(c[1] for c in cand if c[0] == d)
                same = nn[i][own][1] if own in nn[i] and nn[i][own][0] == d else 0
                terms.append(float(same) / float(tied))
                counts["nn_same_" + side] += same == tied
                counts["nn_other_" + side] += same == 0
            s = 0.0
            for t in terms:  # left to right, from 0.0
                s += t
            r.update(counts)
            r["snn"] = s / float(len(pk) + len(pl))
            r["gmin"] = float(r["min_h"]) / (float(r["sum_h"]) / float(r["n_pairs"])) if r["sum_h"] else float("nan")
            r["reserved"] = 0
            pairs.append(r)
    return panels, pairs, hw, hb


def pack(per_window, K, bins):
    """[(panels, pairs, hw, hb) per window] -> the four arrays of BitMatrix.pairdist_scan"""
    n_w, NP = len(per_window), K * (K - 1) // 2
    panels = np.zeros((n_w, K), PANEL_DTYPE)
    pairs = np.zeros((n_w, NP), PAIR_DTYPE)
    hw = np.zeros((n_w, K, bins), np.uint32) if bins else None
    hb = np.zeros((n_w, NP, bins), np.uint32) if bins else None
    for w, (pa, pr, a, b) in enumerate(per_window):
        for k, r in enumerate(pa):
            for f in PANEL_DTYPE.names:
                panels[w, k][f] = r[f]
            if bins:
                hw[w, k] = a[k]
        for k, r in enumerate(pr):
            for f in PAIR_DTYPE.names:
                pairs[w, k][f] = r[f]
            if bins:
                hb[w, k] = b[k]
    return panels, pairs, hw, hb


def scan(m01, wins, pops, bins=0, width=1, weights=None, H_of=None):
    """H_of (optional): window -> H, where the caller has the distances already"""
    per = []
    for win in wins:
        s0, s1 = int(win[0]), int(win[1])
        H = H_of(win) if H_of else hamming(gram(m01, s0, s1, weights))
        W = (s1 - s0) if weights is None else int(np.asarray(weights, np.int64)[s0:s1].sum())
        per.append(window(H, W, pops, bins, width))
    return pack(per, len(pops), bins)


def brute_window(rows, w, pops, bins=0, width=1):
    """The header's definitions as loops over sites, pairs and members; rows: lists of 0/1, w: weights.  -> like window()"""
    def H(i, j):
        return sum(w[s] for s in range(len(w)) if rows[i][s] != rows[j][s])
    def fields(prs):
        r = dict(n_pairs=len(prs), sum_h=0, sum_h2=0, n_zero=0, min_h=0, max_h=0, min_i=NONE, min_j=NONE, max_i=NONE, max_j=NONE)
        hist = [0] * bins
        for n, (i, j) in enumerate(prs):
            h = H(i, j)
            r["sum_h"] += h; r["sum_h2"] += h * h; r["n_zero"] += h == 0
            if n == 0 or h < r["min_h"]:
                r["min_h"], r["min_i"], r["min_j"] = h, i, j
            if n == 0 or h > r["max_h"]:
                r["max_h"], r["max_i"], r["max_j"] = h, i, j
            if bins:
                hist[min(h // width, bins - 1)] += 1
        return r, hist
    pops = [sorted(p) for p in pops]
    panels, pairs, hw, hb = [], [], [], []
    for p in pops:
        r, hist = fields([(i, j) for i in p for j in p if i < j])
        r.update(n_members=len(p), n_sites=sum(w))
        panels.append(r); hw.append(hist)
    for k in range(len(pops)):
        for l in range(k + 1, len(pops)):
            r, hist = fields([(i, j) for i in pops[k] for j in pops[l]])
            both = sorted(pops[k] + pops[l])
            s = 0.0
            r.update(nn_same_a=0, nn_same_b=0, nn_other_a=0, nn_other_b=0)
            for i in both:
                d = min(H(i, j) for j in both if j != i)
                tied = [j for j in both if j != i and H(i, j) == d]
                mine = pops[k] if i in pops[k] else pops[l]
                same = sum(1 for j in tied if j in mine)
                side = "a" if i in pops[k] else "b"
                r["nn_same_" + side] += same == len(tied)
                r["nn_other_" + side] += same == 0
                s += float(same) / float(len(tied))
            r["snn"] = s / float(len(both))
            r["gmin"] = float(r["min_h"]) / (float(r["sum_h"]) / float(r["n_pairs"])) if r["sum_h"] else float("nan")
            r["reserved"] = 0
            pairs.append(r); hb.append(hist)
    return panels, pairs, hw, hb
