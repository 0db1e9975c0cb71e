"""A plain Python restatement of impop_ibd_scan's definition (include/impop_hip.h), written from the prose and in Python integers:
per pair a direct scan of the two rows gives the tracts, then candidates, chains and segments follow one tract at a time; the
window sums are taken per window over the whole segment list.  Nothing here knows about batches, masks, staging or window edges."""
import bisect

import numpy as np

PAIR = np.dtype([("h1", "<u4"), ("h2", "<u4"), ("n_segments", "<u4"), ("n_candidates", "<u4"), ("total_len", "<u8"),
                 ("total_extent", "<u8"), ("longest_len", "<u8"), ("ibs_sites", "<u8")])
SEGMENT = np.dtype([("h1", "<u4"), ("h2", "<u4"), ("begin", "<u8"), ("end", "<u8"), ("len", "<u8"), ("ibs_sites", "<u4"),
                    ("n_tracts", "<u4"), ("pair", "<u4"), ("flags", "<u4")])
WINDOW = np.dtype([("pair_sites", "<u8"), ("tracts", "<u4"), ("pairs_spanning", "<u4"), ("n_sites", "<u4"), ("reserved", "<u4"),
                   ("share", "<f8")])
OPEN_LEFT, OPEN_RIGHT = 1, 2


def G(gmap, x):
    """gmap: None or (pos, g), two lists of Python integers"""
    if gmap is None:
        return int(x)
    pos, g = gmap
    x = int(x)
    if x <= pos[0]:
        return g[0]
    if x >= pos[-1]:
        return g[-1]
    k = bisect.bisect_right(pos, x) - 1  # pos[k] <= x < pos[k + 1]
    return g[k] + (x - pos[k]) * (g[k + 1] - g[k]) // (pos[k + 1] - pos[k])


def tracts_of(row1, row2, b, e):
    """every tract of the pair in [b, e), of any length >= 1, ascending: a direct scan of the differing sites"""
    out, start = [], b
    for p in np.flatnonzero(row1[b:e] != row2[b:e]).tolist():
        p += b
        if p > start:
            out.append((start, p))
        start = p + 1
    if e > start:
        out.append((start, e))
    return out


def chains_of(tracts, gmap, min_sites, min_extend, min_seed, max_gap):
    """-> (candidates, [chain]) with chain = (the candidates' list, has a seed)"""
    lengths = [(s, t, G(gmap, t) - G(gmap, s)) for s, t in tracts if t - s >= min_sites]
    cands = [(s, t) for s, t, ln in lengths if ln >= min_extend]
    chains = []
    for s, t, ln in lengths:
        if ln < min_extend:
            continue
        seed = ln >= min_seed
        if chains and s - chains[-1][0][-1][1] <= max_gap:
            chains[-1][0].append((s, t))
            chains[-1][1] = chains[-1][1] or seed
        else:
            chains.append([[(s, t)], seed])
    return cands, chains


def reference(m01, pairs, b, e, min_sites, min_extend, min_seed, min_output, max_gap, gmap=None, windows=None, weights=None, stats=None):
    """m01: the FULL 0/1 matrix [haplotype, site]; pairs: [(h1, h2)] in pair order; gmap: None or (pos, g).
    -> (pair records, segments, window records or None).  stats (a dict, optional) counts the chains dropped and why."""
    m01 = np.asarray(m01)
    if gmap is not None:
        gmap = ([int(x) for x in gmap[0]], [int(x) for x in gmap[1]])
    rec = np.zeros(len(pairs), dtype=PAIR)
    rows = []
    no_seed = too_short = 0
    for k, (h1, h2) in enumerate(pairs):
        cands, chains = chains_of(tracts_of(m01[h1], m01[h2], b, e), gmap, min_sites, min_extend, min_seed, max_gap)
        mine = []
        for members, seed in chains:
            s, t = members[0][0], members[-1][1]
            ln = G(gmap, t) - G(gmap, s)
            if not seed:
                no_seed += 1
            elif ln < min_output:
                too_short += 1
            else:
                mine.append((h1, h2, s, t, ln, sum(y - x for x, y in members), len(members), k,
                             (OPEN_LEFT if s == b else 0) | (OPEN_RIGHT if t == e else 0)))
        rec[k] = (h1, h2, len(mine), len(cands), sum(r[4] for r in mine), sum(r[3] - r[2] for r in mine), max([r[4] for r in mine], default=0),
                  sum(r[5] for r in mine))
        rows.extend(mine)
    seg = np.array(rows, dtype=SEGMENT) if rows else np.zeros(0, dtype=SEGMENT)
    if stats is not None:
        stats.update(no_seed=no_seed, too_short=too_short)
    if windows is None:
        return rec, seg, None
    win = np.zeros(len(windows), dtype=WINDOW)
    for i, w in enumerate(windows):
        wb, we = int(w[0]), int(w[1])
        W = we - wb if weights is None else int(np.asarray(weights, dtype=np.int64)[wb:we].sum())
        if we <= wb:
            win[i] = (0, 0, 0, W, 0, np.nan)
            continue
        pair_sites = meets = spans = 0
        for r in rows:  # brute force: one segment at a time
            s, t = r[2], r[3]
            pair_sites += max(min(t, we) - max(s, wb), 0)
            meets += 1 if s < we and t > wb else 0
            spans += 1 if s <= wb and t >= we else 0
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
