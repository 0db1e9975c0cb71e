"""The definitions of impop_ihs_scan (include/impop_hip.h) restated with plain loops: no PBWT, no divergence array.  Per pair of
rows it takes the run of identity around each stepped site, counts per core, class and half how many pairs reach j steps, and
integrates that survival curve as the definitions say.

    tables = survivors(m01, b, e, pops)            the survival counts, independent of every parameter
    records(tables, core_b, core_e, min_mac, ...)  the records (IHS_DTYPE), byte for byte what the device writes

weighted_survivors() is the same for a matrix given as a few distinct rows with multiplicities (the 4096-member case, where
pairs x sites is out of reach); tests cross-check it against survivors() on small matrices."""
import numpy as np

IHS_DTYPE = np.dtype([("site", "<u8"), ("n", "<u4", (2,)), ("c1", "<u4", (2,)), ("flags", "<u4"), ("reserved", "<u4"),
                      ("ihh2", "<u8", (2, 2)), ("sl2", "<u8", (2, 2))])
assert IHS_DTYPE.itemsize == 96
EDGE_BITS, LIMIT_BITS = 0x00FF, 0xFF00


def flag_bit(limit, measure, cls, half):
    return 1 << ((8 if limit else 0) + 4 * measure + 2 * cls + half)


class Tables:
    """pos[x]: coordinate of stepped ordinal x; cP[x]: carriers in P; surv[h][x, g, j]: pairs of class g at x identical over the j
    further stepped sites of half h (j = 0: at x alone); n[x, g], c1[x, g]: class sizes and allele-1 carriers"""
    def __init__(self, pos, cP, n, c1, surv):
        self.pos, self.cP, self.n, self.c1, self.surv = pos, cP, n, c1, surv


def _pops(m01, pops):
    nh = m01.shape[0]
    masks = [np.ones(nh, bool) if p is None else np.asarray(p).astype(bool) for p in pops]
    assert len(masks) in (1, 2)
    if len(masks) == 2:
        assert not (masks[0] & masks[1]).any()
    return masks


def _runs(agree):
    """per stepped site x: the number of consecutive sites of agreement that end at x (towards lower x) and that begin at x"""
    S = len(agree)
    idx = np.arange(S)
    last_dis = np.maximum.accumulate(np.where(agree, -1, idx))
    left = idx - last_dis
    next_dis = np.minimum.accumulate(np.where(agree, S, idx)[::-1])[::-1]
    right = next_dis - idx
    return left, right  # 0 where the pair differs at x


def _finish(hist):
    """hist[x, g, run] -> surv[x, g, j] = pairs with run >= j + 1"""
    return np.cumsum(hist[:, :, ::-1], axis=2)[:, :, ::-1][:, :, 1:]


def survivors(m01, b, e, pops):
    m01 = np.asarray(m01)
    masks = _pops(m01, pops)
    P = masks[0] if len(masks) == 1 else masks[0] | masks[1]
    members = np.flatnonzero(P)
    X = m01[members][:, b:e].astype(np.uint8)
    cP = X.sum(axis=0).astype(np.int64)
    stepped = np.flatnonzero((cP > 0) & (cP < len(members)))
    Xs, S = X[:, stepped], len(stepped)
    hist = [np.zeros((S, 2, S + 2), np.int64) for _ in range(2)]
    label = None if len(masks) == 1 else masks[1][members].astype(np.int64)  # 0 = A, 1 = B
    ar = np.arange(S)
    for i in range(len(members)):
        for j in range(i + 1, len(members)):
            if label is not None and label[i] != label[j]:
                continue
            agree = Xs[i] == Xs[j]
            left, right = _runs(agree)
            cls = Xs[i].astype(np.int64) if label is None else np.full(S, label[i])
            np.add.at(hist[0], (ar, cls, left), 1)
            np.add.at(hist[1], (ar, cls, right), 1)
    if label is None:
        n = np.stack([len(members) - cP[stepped], cP[stepped]], axis=1)
        c1 = np.stack([np.zeros(S, np.int64), cP[stepped]], axis=1)
    else:
        n = np.tile(np.array([(label == 0).sum(), (label == 1).sum()]), (S, 1))
        c1 = np.stack([Xs[label == 0].sum(axis=0), Xs[label == 1].sum(axis=0)], axis=1).astype(np.int64)
    return Tables(b + stepped, cP[stepped], n, c1, [_finish(h) for h in hist])


def weighted_survivors(rows, mult, b, e):
    """rows[r, sites]: distinct rows; mult: one list (K = 1) or two (K = 2, per population) of multiplicities per row"""
    rows = np.asarray(rows)
    mult = [np.asarray(mm, dtype=np.int64) for mm in mult]
    tot = mult[0] if len(mult) == 1 else mult[0] + mult[1]
    X = rows[:, b:e].astype(np.int64)
    cP = (X * tot[:, None]).sum(axis=0)
    stepped = np.flatnonzero((cP > 0) & (cP < tot.sum()))
    Xs, S = X[:, stepped], len(stepped)
    hist = [np.zeros((S, 2, S + 2), np.int64) for _ in range(2)]
    ar = np.arange(S)
    for i in range(len(rows)):
        for j in range(i, len(rows)):
            agree = Xs[i] == Xs[j]
            left, right = _runs(agree)
            for g, mm in enumerate(mult):
                w = mm[i] * (mm[i] - 1) // 2 if i == j else mm[i] * mm[j]
                if w == 0:
                    continue
                cls = Xs[i] if len(mult) == 1 else np.full(S, g)
                np.add.at(hist[0], (ar, cls, left), w)
                np.add.at(hist[1], (ar, cls, right), w)
    if len(mult) == 1:
        c = cP[stepped]
        n = np.stack([tot.sum() - c, c], axis=1)
        c1 = np.stack([np.zeros(S, np.int64), c], axis=1)
    else:
        n = np.tile(np.array([mult[0].sum(), mult[1].sum()]), (S, 1))
        c1 = np.stack([(Xs * mm[:, None]).sum(axis=0) for mm in mult], axis=1)
    return Tables(b + stepped, cP[stepped], n, c1, [_finish(h) for h in hist])


def integral(surv, dist, C, cutoff_milli, J_range, J_u):
    """one (class, half, measure): surv[j] and dist[j] (distance of x_j from the core) for j = 0 .. J_range -> (I2, flag kind)
    with kind 0 = none, 1 = EDGE, 2 = LIMIT"""
    if 1000 * int(surv[0]) < cutoff_milli * C:
        return 0, 0
    jstar = 0
    for j in range(1, J_u + 1):  # surv never increases with j: the first failure ends the search
        if 1000 * int(surv[j]) < cutoff_milli * C:
            break
        jstar = j
    I2 = 0
    for j in range(jstar):
        I2 += (int(surv[j]) + int(surv[j + 1])) * abs(int(dist[j + 1]) - int(dist[j]))
    kind = 0 if jstar != J_u else 1 if J_u == J_range else 2
    return I2, kind


def records(t, core_b, core_e, min_mac=1, cutoff_milli=50, max_bp=0, max_sites=0):
    S = len(t.pos)
    nP = int(t.n[0].sum()) if S else 0
    out = []
    for x in range(S):
        p = int(t.pos[x])
        c = int(t.cP[x])
        if not (core_b <= p < core_e) or min(c, nP - c) < min_mac:
            continue
        r = np.zeros((), IHS_DTYPE)
        r["site"], r["n"], r["c1"] = p, t.n[x], t.c1[x]
        flags = 0
        for g in range(2):
            ng = int(t.n[x, g])
            if ng < 2:
                continue
            C = ng * (ng - 1) // 2
            for h in range(2):
                J_range = x if h == 0 else S - 1 - x
                xs = np.arange(x, -1, -1) if h == 0 else np.arange(x, S)   # x_0 = the core, x_1, ... x_J_range
                surv = t.surv[h][x, g, :J_range + 1]
                for measure in range(2):
                    if measure == 0:
                        dist = np.abs(t.pos[xs].astype(np.int64) - p)
                        lim = max_bp
                    else:
                        dist = np.arange(J_range + 1)
                        lim = max_sites
                    J_u = J_range
                    if lim:
                        J_u = int(np.flatnonzero(dist <= lim).max())
                    I2, kind = integral(surv, dist, C, cutoff_milli, J_range, J_u)
                    r["sl2" if measure else "ihh2"][g, h] = I2
                    if kind:
                        flags |= flag_bit(kind == 2, measure, g, h)
        r["flags"] = flags
        out.append(r)
    return np.array(out, dtype=IHS_DTYPE) if out else np.zeros(0, IHS_DTYPE)


def reference(m01, b, e, core_b, core_e, pops, **params):
    return records(survivors(m01, b, e, pops), core_b, core_e, **params)


def assert_same(got, want, tag=""):
    assert got.dtype == want.dtype and len(got) == len(want), (tag, len(got), len(want))
    if got.tobytes() == want.tobytes():
        return
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.tobytes() == w.tobytes(), f"{tag}: record {i}\n got  {g}\n want {w}"
