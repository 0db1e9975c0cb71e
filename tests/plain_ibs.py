"""A plain numpy / Python restatement of impop_ibs_scan's definition (include/impop_hip.h), written from the prose: per pair the
sites of the range where the two rows differ, the tracts between them, the reported ones as segments, and per window the sums
over the reported tracts taken one tract at a time.  Nothing here knows about chunks, summaries or window edges."""
import numpy as np

PAIR = np.dtype([("h1", "<u4"), ("h2", "<u4"), ("n_diff", "<u4"), ("longest", "<u4"), ("n_tracts", "<u4"), ("reserved", "<u4"),
                 ("tract_sites", "<u8")])
SEGMENT = np.dtype([("h1", "<u4"), ("h2", "<u4"), ("begin", "<u8"), ("end", "<u8"), ("pair", "<u4"), ("flags", "<u4")])
WINDOW = np.dtype([("pair_sites", "<u8"), ("tracts", "<u4"), ("pairs_spanning", "<u4"), ("n_sites", "<u4"), ("reserved", "<u4"),
                   ("share", "<f8")])
OPEN_LEFT, OPEN_RIGHT = 1, 2


def all_pairs(members):
    """pairs i < j of the members in ascending order, i-major"""
    mem = sorted(int(h) for h in members)
    return [(mem[i], mem[j]) for i in range(len(mem)) for j in range(i + 1, len(mem))]


def members_of(mask, n):
    return list(range(n)) if mask is None else [int(i) for i in np.flatnonzero(np.asarray(mask))]


def tracts_of(row1, row2, b, e):
    """-> (n_diff, [(begin, end)]: every tract of the pair in [b, e), of any length >= 1, ascending)"""
    d = np.flatnonzero(row1[b:e] != row2[b:e]).astype(np.int64) + b
    begins = np.concatenate([[b], d + 1])
    ends = np.concatenate([d, [e]])
    keep = ends > begins  # tracts of length 0 are not tracts
    return len(d), list(zip(begins[keep].tolist(), ends[keep].tolist()))


def reference(m01, pairs, b, e, min_sites, windows=None, weights=None):
    """m01: the FULL 0/1 matrix [haplotype, site] (a compacted matrix drops monomorphic sites only: no pair differs there);
    pairs: [(h1, h2)] in pair order.  -> (pair records, segments, window records or None)"""
    m01 = np.asarray(m01)
    rec = np.zeros(len(pairs), dtype=PAIR)
    parts = []
    for k, (h1, h2) in enumerate(pairs):
        n_diff, tr = tracts_of(m01[h1], m01[h2], b, e)
        rep = [(s, t) for s, t in tr if t - s >= min_sites]
        rec[k] = (h1, h2, n_diff, max([t - s for s, t in tr], default=0), len(rep), 0, sum(t - s for s, t in rep))
        part = np.zeros(len(rep), dtype=SEGMENT)
        for i, (s, t) in enumerate(rep):
            part[i] = (h1, h2, s, t, k, (OPEN_LEFT if s == b else 0) | (OPEN_RIGHT if t == e else 0))
        parts.append(part)
    seg = np.concatenate(parts) if parts else np.zeros(0, dtype=SEGMENT)
    if windows is None:
        return rec, seg, None
    win = np.zeros(len(windows), dtype=WINDOW)
    s_all, t_all = seg["begin"].astype(np.int64), seg["end"].astype(np.int64)
    for i, w in enumerate(windows):
        wb, we = int(w[0]), int(w[1])
        W = we - wb if weights is None else int(np.asarray(weights, dtype=np.int64)[wb:we].sum())
        if we <= wb:
            win[i] = (0, 0, 0, W, 0, np.nan)
            continue
        inter = np.clip(np.minimum(t_all, we) - np.maximum(s_all, wb), 0, None)
        pair_sites = int(inter.sum())
        meets = int(((s_all < we) & (t_all > wb)).sum())
        spans = int(((s_all <= wb) & (t_all >= we)).sum())
        win[i] = (pair_sites, meets, spans, W, 0, float(pair_sites) / (float(len(pairs)) * float(we - wb)))
    return rec, seg, win


def assert_same(got, want, tag=""):
    """every integer and the double, bit for bit (NaN against NaN)"""
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, got.shape, want.shape)
    for f in want.dtype.names:
        g, w = got[f], want[f]
        if w.dtype.kind == "f":
            assert (np.isnan(g) == np.isnan(w)).all(), (tag, f)
            ok = ~np.isnan(w)
            assert g[ok].tobytes() == w[ok].tobytes(), (tag, f, g[ok][:8], w[ok][:8])
        else:
            bad = np.flatnonzero(g != w)
            assert bad.size == 0, (tag, f, bad[:8], g[bad[:8]], w[bad[:8]])


def assert_matches(got, want, tag=""):
    """got / want: (pair records, segments, window records or None)"""
    assert_same(got[0], want[0], (tag, "pairs"))
    assert_same(got[1], want[1], (tag, "segments"))
    if want[2] is None:
        assert got[2] is None, tag
    else:
        assert_same(got[2], want[2], (tag, "windows"))
