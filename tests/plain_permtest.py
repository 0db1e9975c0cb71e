"""A plain numpy / Python restatement of impop_permtest_scan, written from the prose of include/impop_hip.h and from nothing else.
H comes from plain_pairdist.gram / hamming; the labellings are GIVEN masks (one Python integer per labelling, bit i = position i);
every sum is an exact integer (int64 partial sums of at most 2^19 distances <= 2^31, then Python integers) and every comparison is
made on Python integers; the doubles follow the header's order of operations.  It also restates the header's generator.

    labelling(seed, p, m, m_a, r)          -> the mask of labelling r as a Python integer
    labels(seed, p, m, m_a, n_perm)        -> [n_perm masks]
    words(masks, m)                        -> [n, ceil(m / 64)] uint64, the layout of impop_permtest_labels
    pair(H, U, m_k, label_masks)           -> dict of the record's fields, and the null rows [(wa, wb, nn)]
    window(H, n_sites, pops, labels_of)    -> [(record, null) per pair k < l]; labels_of(p, m, m_k) -> masks
    scan(m01, wins, pops, labels_of, weights=None, want_null=True) -> the arrays BitMatrix.permtest_scan returns
"""
import numpy as np

from plain_pairdist import gram, hamming

SCALE = 2952069120
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
PAIR_DTYPE = np.dtype([("n_a", "<u4"), ("n_b", "<u4"), ("n_sites", "<u4"), ("n_perm", "<u4"), ("wa", "<u8"), ("wb", "<u8"), ("ab", "<u8"),
                       ("nn", "<u8"), ("ge_fst", "<u4"), ("ge_phi", "<u4"), ("ge_dxy", "<u4"), ("ge_snn", "<u4"), ("fst", "<f8"),
                       ("phi_st", "<f8"), ("dxy", "<f8"), ("snn", "<f8"), ("p_fst", "<f8"), ("p_phi", "<f8"), ("p_dxy", "<f8"), ("p_snn", "<f8")])
NULL_DTYPE = np.dtype([("wa", "<u8"), ("wb", "<u8"), ("nn", "<u8")])


def sm(x):
    z = (x + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def labelling(seed, p, m, m_a, r):
    k3 = sm(sm(sm(seed & M64) ^ p) ^ r)
    a = list(range(m))
    mask = 0
    for t in range(m_a):
        u = sm((k3 + t * GOLDEN) & M64)
        j = t + ((u * (m - t)) >> 64)
        a[t], a[j] = a[j], a[t]
        mask |= 1 << a[t]
    return mask


def labels(seed, p, m, m_a, n_perm):
    return [labelling(seed, p, m, m_a, r) for r in range(n_perm)]


def words(masks, m):
    mw = (m + 63) // 64
    return np.array([[(z >> (64 * t)) & M64 for t in range(mw)] for z in masks], dtype=np.uint64).reshape(len(masks), mw)


def from_words(arr):
    return [sum(int(v) << (64 * t) for t, v in enumerate(row)) for row in arr]


def q_of(m):
    return max(m * (m - 1) // 2, 1)


def ge_fst(wa, wb, o, m_k, m_l):
    x, x0 = wa * q_of(m_l) + wb * q_of(m_k), o["wa"] * q_of(m_l) + o["wb"] * q_of(m_k)
    return x * (o["tot"] - o["wa"] - o["wb"]) <= x0 * (o["tot"] - wa - wb)


def ge_phi(wa, wb, o, m_k, m_l):
    return wa * m_l + wb * m_k <= o["wa"] * m_l + o["wb"] * m_k


def ge_dxy(wa, wb, o):
    return o["tot"] - wa - wb >= o["tot"] - o["wa"] - o["wb"]


def ge_snn(nn, o):
    return nn >= o["nn"]


def doubles(o, m_k, m_l):
    """fst, phi_st, dxy in the header's order of operations"""
    wa, wb, tot = o["wa"], o["wb"], o["tot"]
    ab, m = tot - wa - wb, m_k + m_l
    dxy = float(ab) / (float(m_k) * float(m_l))
    pi_a = float(wa) / float(q_of(m_k)) if m_k >= 2 else 0.0
    pi_b = float(wb) / float(q_of(m_l)) if m_l >= 2 else 0.0
    pi_xy = (pi_a + pi_b) / 2.0
    fst = (dxy - pi_xy) / dxy if dxy > 0.0 else 0.0
    phi = float("nan")
    if m > 2:
        ssd_w = float(wa) / float(m_k) + float(wb) / float(m_l)
        ssd_a = float(tot) / float(m) - ssd_w
        ms_w = ssd_w / float(m - 2)
        n0 = 2.0 * float(m_k) * float(m_l) / float(m)
        s2a = (ssd_a - ms_w) / n0
        den = s2a + ms_w
        if den != 0.0:
            phi = s2a / den
    return fst, phi, dxy


def pair(Hu, z0, m_k, label_masks, n_sites=0):
    """Hu: the m x m distances of U (ascending haplotype index), z0 / label_masks: Python integer masks"""
    Hu = np.asarray(Hu, np.int64)
    m = len(Hu)
    m_l = m - m_k
    off = Hu + np.eye(m, dtype=np.int64) * (1 << 40)  # the diagonal never is a nearest neighbour
    d = off.min(axis=1)
    T = off == d[:, None]
    tied = T.sum(axis=1)
    term = [SCALE // int(t) for t in tied]
    tot = int(np.triu(Hu, 1).sum())

    def integers(z):
        bits = np.array([(z >> i) & 1 for i in range(m)], dtype=bool)
        wa = int(np.triu(Hu[np.ix_(bits, bits)], 1).sum())
        wb = int(np.triu(Hu[np.ix_(~bits, ~bits)], 1).sum())
        same = (T & (bits[:, None] == bits[None, :])).sum(axis=1)
        return wa, wb, sum(int(s) * t for s, t in zip(same, term)), same

    wa0, wb0, nn0, same0 = integers(z0)
    o = dict(wa=wa0, wb=wb0, nn=nn0, tot=tot)
    ge = [0, 0, 0, 0]
    null = []
    for z in label_masks:
        assert bin(z).count("1") == m_k and z >> m == 0
        wa, wb, nn, _ = integers(z)
        null.append((wa, wb, nn))
        ge[0] += ge_fst(wa, wb, o, m_k, m_l)
        ge[1] += ge_phi(wa, wb, o, m_k, m_l)
        ge[2] += ge_dxy(wa, wb, o)
        ge[3] += ge_snn(nn, o)
    s = 0.0
    for i in range(m):  # left to right, from 0.0
        s += float(int(same0[i])) / float(int(tied[i]))
    fst, phi, dxy = doubles(o, m_k, m_l)
    n_perm = len(label_masks)
    p = [(1.0 + float(g)) / (float(n_perm) + 1.0) for g in ge]
    rec = dict(n_a=m_k, n_b=m_l, n_sites=int(n_sites), n_perm=n_perm, wa=wa0, wb=wb0, ab=tot - wa0 - wb0, nn=nn0, ge_fst=ge[0], ge_phi=ge[1],
               ge_dxy=ge[2], ge_snn=ge[3], fst=fst, phi_st=phi, dxy=dxy, snn=s / float(m), p_fst=p[0], p_phi=p[1], p_dxy=p[2], p_snn=p[3],
               tied_max=int(tied.max()), h_max=int(Hu.max()))
    return rec, null


def window(H, n_sites, pops, labels_of):
    pops = [sorted(int(x) for x in p) for p in pops]
    out = []
    p = 0
    for k in range(len(pops)):
        for l in range(k + 1, len(pops)):
            U = sorted(pops[k] + pops[l])
            in_k = set(pops[k])
            z0 = sum(1 << i for i, h in enumerate(U) if h in in_k)
            out.append(pair(np.asarray(H)[np.ix_(U, U)], z0, len(pops[k]), labels_of(p, len(U), len(pops[k])), n_sites))
            p += 1
    return out


def pack(per_window, n_perm, want_null=True):
    n_w, NP = len(per_window), len(per_window[0]) if per_window else 0
    pairs = np.zeros((n_w, NP), PAIR_DTYPE)
    null = np.zeros((n_w, NP, n_perm), NULL_DTYPE) if want_null else None
    for w, per in enumerate(per_window):
        for k, (r, nl) in enumerate(per):
            for f in PAIR_DTYPE.names:
                pairs[w, k][f] = r[f]
            if want_null:
                for j, (a, b, c) in enumerate(nl):
                    null[w, k, j] = (a, b, c)
    return pairs, null


def scan(m01, wins, pops, labels_of, n_perm, weights=None, want_null=True):
    per = []
    for win in wins:
        s0, s1 = int(win[0]), int(win[1])
        H = hamming(gram(m01, s0, s1, weights))
        W = (s1 - s0) if weights is None else int(np.asarray(weights, np.int64)[s0:s1].sum())
        per.append(window(H, W, pops, labels_of))
    return pack(per, n_perm, want_null)
