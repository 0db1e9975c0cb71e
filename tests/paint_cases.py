"""The plain restatement of impop_paint_scan (include/impop_hip.h) and the case generators of its tests.  numpy, no GPU.

The restatement is the LITERAL recursion of the header: the full table of V_j(s), the stay bits stay_j(s) for every state and site,
and the backtrack that reads them.  It is deliberately not the origin-pointer form the device uses (csrc/paint_math.h).  It also
forms the segments, the per-recipient records, the two chunk matrices, the window records and anc."""
from collections import namedtuple

import numpy as np

RECIPIENT_DTYPE = np.dtype([("h", "<u4"), ("n_donors", "<u4"), ("n_segments", "<u4"), ("n_mismatch", "<u4"), ("distinct_donors", "<u4"),
                            ("longest_sites", "<u4"), ("longest_donor", "<u4"), ("reserved", "<u4"), ("cost", "<u8")])
SEGMENT_DTYPE = np.dtype([("h", "<u4"), ("donor", "<u4"), ("begin", "<u8"), ("end", "<u8"), ("n_sites", "<u4"), ("n_mismatch", "<u4"),
                          ("recipient", "<u4"), ("reserved", "<u4")])
WINDOW_DTYPE = np.dtype([("n_switches", "<u8"), ("n_mismatch", "<u8"), ("cells", "<u8"), ("copied", "<u8", (9,))])
NO_PANEL = 255

KNOWN_ROWS = ("000000000100", "000000111111", "111111000000", "111111111011")
# (mu, c) -> (cost, n_mismatch, [(donor, begin, end)])
KNOWN = {(1, 2): (3, 1, [(1, 0, 6), (2, 6, 12)]),
         (3, 1): (3, 0, [(1, 0, 6), (2, 6, 9), (1, 9, 10), (2, 10, 12)]),
         (1, 5): (5, 5, [(1, 0, 12)])}


def known_matrix():
    return np.array([[int(ch) for ch in row] for row in KNOWN_ROWS], dtype=np.uint8)


def admissible(n_hap, donors, group, h):
    """the admissible donors of recipient h, ascending"""
    dm = np.ones(n_hap, bool) if donors is None else np.asarray(donors).astype(bool)
    g = np.arange(n_hap) if group is None else np.asarray(group)
    return [j for j in range(n_hap) if dm[j] and g[j] != g[h]]


def viterbi(x, D, mu, cs):
    """x: the recipient's row [L]; D: the donors' rows [K, L]; cs[s] = c_s (cs[0] unused) -> (cost, path d[s] as an index into D).
    The literal recursion: V, M, A, the stay bits of every state and site, the backtrack over them."""
    K, L = D.shape
    mm = (D != x[None, :]).astype(np.int64) * int(mu)
    V = np.zeros((L, K), dtype=np.int64)
    stay = np.zeros((L, K), dtype=bool)
    M = np.zeros(L, dtype=np.int64)
    A = np.zeros(L, dtype=np.int64)
    V[0] = mm[:, 0]
    M[0] = V[0].min()
    A[0] = int(np.argmin(V[0]))  # the first of equals: the lowest admissible j
    for s in range(1, L):
        sw = M[s - 1] + int(cs[s])
        stay[s] = V[s - 1] <= sw
        V[s] = mm[:, s] + np.minimum(V[s - 1], sw)
        M[s] = V[s].min()
        A[s] = int(np.argmin(V[s]))
    d = np.zeros(L, dtype=np.int64)
    d[L - 1] = A[L - 1]
    for s in range(L - 1, 0, -1):
        d[s - 1] = d[s] if stay[s, d[s]] else A[s - 1]
    return int(M[L - 1]), d


def path_cost(x, D, mu, cs, d):
    """the cost of ANY path d under the model"""
    L = len(x)
    total = sum(int(mu) for s in range(L) if D[d[s], s] != x[s])
    return total + sum(int(cs[s]) for s in range(1, L) if d[s] != d[s - 1])


def reference(m01, recipients, donors=None, mu=1, c=1, site_cost=None, group=None, panel=None, n_panels=0, b=0, e=None, windows=None,
              coords=None):
    """-> dict(recipients, segments, n_segments, chunk_counts, chunk_sites, windows, anc) as BitMatrix.paint_scan returns them.
    m01 holds the STORED sites; coords (None: the identity) their original coordinates, for a compacted matrix; [b, e) is in
    original coordinates and site_cost has one entry per stored site of the range."""
    m01 = np.asarray(m01, dtype=np.uint8)
    n_hap, S = m01.shape
    coords = np.arange(S, dtype=np.int64) if coords is None else np.asarray(coords, dtype=np.int64)
    e = (int(coords[-1]) + 1 if len(coords) else 0) if e is None else int(e)
    sel = np.nonzero((coords >= b) & (coords < e))[0]
    L = len(sel)
    assert L > 0
    co = coords[sel]
    X = m01[:, sel]
    cs = np.full(L, int(c), dtype=np.int64) if site_cost is None else np.asarray(site_cost, dtype=np.int64)
    assert len(cs) == L
    pan = np.full(n_hap, NO_PANEL, dtype=np.int64) if panel is None else np.asarray(panel, dtype=np.int64)
    rec = np.zeros(len(recipients), dtype=RECIPIENT_DTYPE)
    segs = []
    cc = np.zeros((len(recipients), n_hap), dtype=np.uint32)
    cl = np.zeros((len(recipients), n_hap), dtype=np.uint64)
    paths, miss = [], []
    for r, h in enumerate(recipients):
        adm = admissible(n_hap, donors, group, h)
        assert adm, "no admissible donor"
        cost, d = viterbi(X[h], X[adm], mu, cs)
        dh = np.array(adm, dtype=np.int64)[d]  # donor haplotype per site
        paths.append(dh)
        miss.append(X[dh, np.arange(L)] != X[h])
        cuts = [0] + [s for s in range(1, L) if dh[s] != dh[s - 1]] + [L]
        mine = []
        for s0, s1 in zip(cuts[:-1], cuts[1:]):
            mine.append((h, int(dh[s0]), b if s0 == 0 else int(co[s0]), e if s1 == L else int(co[s1]), s1 - s0, int(miss[-1][s0:s1].sum()), r, 0))
            cc[r, dh[s0]] += 1
            cl[r, dh[s0]] += s1 - s0
        longest = max(range(len(mine)), key=lambda k: (mine[k][4], -k))
        rec[r] = (h, len(adm), len(mine), int(miss[-1].sum()), int((cc[r] > 0).sum()), mine[longest][4], mine[longest][1], 0, cost)
        segs.extend(mine)
    out = dict(recipients=rec, segments=np.array(segs, dtype=SEGMENT_DTYPE), n_segments=len(segs), chunk_counts=cc, chunk_sites=cl,
               windows=None, anc=None)
    if windows is not None:
        win = np.zeros(len(windows), dtype=WINDOW_DTYPE)
        anc = np.zeros((len(windows), len(recipients), n_panels + 1), dtype=np.uint32)
        for w, (wb, we) in enumerate(windows):
            inside = (co >= wb) & (co < we)
            for r in range(len(recipients)):
                dh = paths[r]
                sw = np.zeros(L, bool)
                sw[1:] = dh[1:] != dh[:-1]
                win["n_switches"][w] += int((sw & inside).sum())
                win["n_mismatch"][w] += int((miss[r] & inside).sum())
                win["cells"][w] += int(inside.sum())
                for s in np.nonzero(inside)[0]:
                    p = int(pan[dh[s]])
                    win["copied"][w][8 if p == NO_PANEL else p] += 1
                    anc[w, r, n_panels if p == NO_PANEL else p] += 1
        out["windows"], out["anc"] = win, anc
    return out


KEYS = ("recipients", "segments", "chunk_counts", "chunk_sites", "windows", "anc")


def assert_equal(got, want, tag=""):
    assert got["n_segments"] == want["n_segments"], (tag, "n_segments", got["n_segments"], want["n_segments"])
    for k in KEYS:
        g, w = got[k], want[k]
        if w is None or g is None:
            assert g is None and w is None, (tag, k)
            continue
        if g.tobytes() != w.tobytes():
            bad = np.nonzero(np.atleast_1d(g != w))[0][:5] if g.shape == w.shape else None
            raise AssertionError((tag, k, g.shape, w.shape, bad, None if bad is None or not len(bad) else (g[bad[0]], w[bad[0]])))


def same_bytes(a, b):
    return a["n_segments"] == b["n_segments"] and all((a[k] is None and b[k] is None) or a[k].tobytes() == b[k].tobytes() for k in KEYS)


# ---- generators ---------------------------------------------------------------------------------------------------------------------

def mosaic_matrix(rng, n, S, nf=5, p_switch=0.02, p_mut=0.01):
    """n haplotypes, each a mosaic of nf founders with a few private differences: paths with real switches and mismatches"""
    founders = (rng.random((nf, S)) < 0.35).astype(np.uint8)
    m = np.zeros((n, S), dtype=np.uint8)
    for i in range(n):
        f = int(rng.integers(nf))
        jumps = rng.random(S) < p_switch
        src = np.zeros(S, dtype=np.int64)
        for s in range(S):
            if jumps[s]:
                f = int(rng.integers(nf))
            src[s] = f
        m[i] = founders[src, np.arange(S)]
    m ^= (rng.random((n, S)) < p_mut).astype(np.uint8)
    return m


Case = namedtuple("Case", "tag m01 kw want")


def make_case(tag, m01, **kw):
    return Case(tag, m01, kw, reference(m01, **kw))


def window_list(b, e):
    """irregular, overlapping, one empty, one outside the range, one that sticks out on both sides"""
    L = e - b
    return [(b, e), (b + L // 5, b + L // 2), (b + L // 3, b + L // 3 + 1), (b + L // 2 - 3, e - 1), (b + 7, b + 7), (e + 10, e + 50),
            (max(b - 5, 0), e + 5), (b + 1, b + 2)]


def partition_windows(b, e, k=5):
    cuts = [b + (e - b) * i // k for i in range(k + 1)]
    return list(zip(cuts[:-1], cuts[1:]))
