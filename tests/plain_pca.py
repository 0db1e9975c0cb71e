"""A plain numpy / Python restatement of impop_pca_scan, written from the prose of include/impop_hip.h and from nothing else:
I = X diag(w) X^T in int64, H_ij = a_i + a_j - 2 I_ij, the exact integer matrix 2 m^2 B = m (r_i + r_j) - m^2 H_ij - t, and
numpy.linalg.eigh of it.  The tested library is never the standard.

    distances(m01, s0, s1, members, weights) -> H over the members (int64)
    centred(H)                                -> (2 m^2 B as int64, r, t)
    spectrum(H)                               -> (eigenvalues descending, eigenvectors as columns, B as float64)
    window(H, n_sites, k, tol)                -> dict of what a record must hold, from the exact spectrum
    dist2(lam_a, vec_a, lam_b, vec_b, k)      -> lostruct's distance from RETURNED eigenvalues and vectors
"""
import numpy as np

from plain_pairdist import gram, hamming


def distances(m01, s0, s1, members=None, weights=None):
    H = hamming(gram(m01, s0, s1, weights))
    if members is None:
        return H
    p = np.asarray(sorted(int(x) for x in members), np.int64)
    return H[np.ix_(p, p)]


def centred(H):
    """-> (2 m^2 B, r, t) in exact int64 arithmetic (checked against Python integers on the way)"""
    H = np.asarray(H, np.int64)
    m = H.shape[0]
    r = H.sum(axis=1)
    t = int(r.sum())
    B2 = m * (r[:, None] + r[None, :]) - m * m * H - t
    big = m * (int(r.max()) * 2) + m * m * int(H.max()) + t  # the largest magnitude any term reaches
    assert big < 2 ** 62
    return B2, r, t


def spectrum(H):
    B2, _, _ = centred(H)
    m = H.shape[0]
    assert int(np.abs(B2).max()) < 2 ** 53  # exact as float64
    lam, vec = np.linalg.eigh(B2.astype(np.float64))
    lam, vec = lam[::-1] / (2.0 * m * m), vec[:, ::-1]
    return lam, vec, B2.astype(np.float64) / (2.0 * m * m)


def window(H, n_sites, k, tol=1e-10):
    m = H.shape[0]
    _, _, t = centred(H)
    lam, vec, B = spectrum(H)
    trace = t / 2 / m
    rank = 0
    while rank < min(k, m) and lam[rank] > tol * trace:
        rank += 1
    return dict(n_members=m, n_sites=int(n_sites), sum_h=t // 2, trace=trace, rank=rank, lam=lam, vec=vec, B=B)


def sign_ok(v):
    """the component of largest magnitude is positive, the lowest index on exact ties"""
    a = np.abs(v)
    return v[int(np.argmax(a))] > 0  # argmax returns the first of the ties


def dist2(lam_a, vec_a, lam_b, vec_b, k):
    """vec_*: [k, m]"""
    a = np.asarray(lam_a[:k], np.float64) / np.sum(lam_a[:k])
    b = np.asarray(lam_b[:k], np.float64) / np.sum(lam_b[:k])
    d = (a * a).sum() + (b * b).sum() - 2.0 * float(a @ ((np.asarray(vec_a) @ np.asarray(vec_b).T) ** 2) @ b)
    return max(d, 0.0)
