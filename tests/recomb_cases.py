"""Shared by the recombination-scan tests: matrices, the plain restatement of impop_recomb_scan, a literal restatement of Hudson &
Kaplan's deletion procedure, and the comparison rule.

The restatement follows include/impop_hip.h (impop_recomb_scan) definition by definition, each from the full m x m tables of
incompatible and congruent pairs and never by the kernel's running scheme: left1 / n_left / rep per site, the greedy R_min with its
intervals, the blocks from the running maximum, Wall's counts from sets.  Everything the device writes is an integer and the three
doubles are one IEEE division of exact values each, so integers and tables must be equal and doubles equal bit for bit (NaN as
NaN): a difference is a bug, not noise."""
import numpy as np

import hap_cases as hc
import ld_cases as lc

INTEGERS = ("n_members", "n_sites", "n_qualifying", "n_used", "rmin", "n_incompatible_adjacent", "n_blocks", "longest_block_sites",
            "n_congruent_adjacent", "n_congruent_partitions", "n_partitions", "n_incompatible", "longest_block_begin", "longest_block_end")
DOUBLES = ("four_gamete_fraction", "wall_b", "wall_q")
SITE_FIELDS = ("left1", "n_left", "rep", "carriers")
TILE = 256  # sites of one tile of the pair kernel (the trace's pair_tiles)

# the header's known answer: five sites as rows over (h0, h1, h2, h3)
KNOWN_ROWS = np.array([[1, 1, 0, 0], [1, 0, 1, 0], [1, 1, 0, 0], [0, 0, 1, 1], [1, 0, 0, 0]], dtype=np.uint8)
KNOWN = {"left1": [0, 1, 2, 2, 0], "n_left": [0, 1, 1, 1, 0], "rep": [0, 1, 0, 0, 4], "n_incompatible": 3, "n_incompatible_adjacent": 2,
         "rmin": 2, "intervals": [(0, 1), (1, 2)], "n_blocks": 3, "longest_block_sites": 3, "longest": (2, 4), "n_congruent_adjacent": 1,
         "n_congruent_partitions": 1, "n_partitions": 3, "wall_b": 0.25, "wall_q": 0.4}


# ---- matrices -----------------------------------------------------------------------------------------------------------------------

def tree_matrix(rng, n, k):
    """k mutations dropped on the branches of one random coalescent tree of n leaves -> [n, k] 0/1: a perfect phylogeny, no pair
    of its columns shows four gametes.  Half of the columns are stored with flipped polarity."""
    live = [np.eye(n, dtype=np.uint8)[i] for i in range(n)]
    branches = list(live)
    while len(live) > 1:
        a, b = sorted(rng.choice(len(live), 2, replace=False).tolist())
        node = live[a] | live[b]
        live = [x for t, x in enumerate(live) if t not in (a, b)] + [node]
        if len(live) > 1:
            branches.append(node)  # the root's set is everyone: no mutation shows there
    cols = np.stack([branches[t] for t in rng.integers(0, len(branches), size=k)], axis=1)
    flip = rng.random(k) < 0.5
    cols[:, flip] ^= 1
    return np.ascontiguousarray(cols)


def mosaic(rng, n, seg_lens):
    """independent trees side by side: recombination can only show between segments, rmin <= len(seg_lens) - 1"""
    return np.ascontiguousarray(np.concatenate([tree_matrix(rng, n, k) for k in seg_lens], axis=1))


MOSAIC_SEGS = (40, 25)  # fits hap_cases.MONO's hundred sites with monomorphic sites left on either side
MOSAIC_AT = hc.MONO[0] + 10


def planted_matrix(rng, n, n_site=lc.S, **kw):
    """hap_cases.founder_matrix (many violations) with a mosaic of two trees planted in its monomorphic stretch"""
    m = hc.founder_matrix(rng, n, n_site, **kw)
    mo = mosaic(rng, n, MOSAIC_SEGS)
    m[:, MOSAIC_AT:MOSAIC_AT + mo.shape[1]] = mo
    return np.ascontiguousarray(m)


def window_list():
    """ld_cases.window_list() and the planted mosaic: whole, its first tree alone, across the seam"""
    return lc.window_list() + [(MOSAIC_AT, MOSAIC_AT + sum(MOSAIC_SEGS)), (MOSAIC_AT, MOSAIC_AT + MOSAIC_SEGS[0]),
                               (MOSAIC_AT + 20, MOSAIC_AT + 55)]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------

def pair_relations(rows, n):
    """rows [m, |P|] 0/1 -> incompatible, congruent (bool [m, m]), carriers (int64 [m])"""
    f = rows.astype(np.float64)
    c = rows.astype(np.int64).sum(axis=1)
    n11 = (f @ f.T).astype(np.int64)  # counts far below 2^53: exact
    n10 = c[:, None] - n11
    n01 = c[None, :] - n11
    n00 = n - c[:, None] - c[None, :] + n11
    inc = (n11 > 0) & (n10 > 0) & (n01 > 0) & (n00 > 0)
    cong = ((n10 == 0) & (n01 == 0)) | ((n11 == 0) & (n00 == 0))
    return inc, cong, c


def site_rows(inc, cong):
    """-> left1, n_left, rep (lists) from the pair tables"""
    m = len(inc)
    left1, n_left, rep = [], [], []
    for j in range(m):
        at = np.flatnonzero(inc[:j, j])
        left1.append(int(at[-1]) + 1 if len(at) else 0)
        n_left.append(len(at))
        rep.append(int(np.flatnonzero(cong[:j + 1, j])[0]))
    return left1, n_left, rep


def rmin_intervals(left1):
    """the greedy of the header -> [(left1_j - 1, j)] of the chosen sites"""
    cut, out = 0, []
    for j, l in enumerate(left1):
        if l >= 1 and l - 1 >= cut:
            out.append((l - 1, j))
            cut = j
    return out


def maximal_blocks(left1):
    """-> [(first, last)] of the maximal pairwise-compatible runs, by the running maximum M"""
    m = len(left1)
    M = np.maximum.accumulate(np.asarray(left1, dtype=np.int64)) if m else []
    return [(int(M[j]), j) for j in range(m) if j == m - 1 or M[j + 1] > M[j]]


def window_values(left1, n_left, rep):
    """the per-window integers from the per-site rows (site indices, not coordinates)"""
    m = len(left1)
    blocks = maximal_blocks(left1)
    M = np.maximum.accumulate(np.asarray(left1, dtype=np.int64)) if m else np.zeros(0, np.int64)
    lens = [j - int(M[j]) + 1 for j in range(m)]
    best = max(lens) if m else 0
    jb = lens.index(best) if m else 0
    in_pair = [j for j in range(m) if (j >= 1 and rep[j] == rep[j - 1]) or (j + 1 < m and rep[j + 1] == rep[j])]
    return {"rmin": len(rmin_intervals(left1)), "n_incompatible": int(sum(n_left)),
            "n_incompatible_adjacent": sum(1 for j in range(1, m) if left1[j] == j), "n_blocks": len(blocks),
            "longest_block_sites": best, "longest": (int(M[jb]), jb) if m else (0, 0),
            "n_congruent_adjacent": sum(1 for j in range(1, m) if rep[j] == rep[j - 1]),
            "n_congruent_partitions": len({rep[j] for j in in_pair}), "n_partitions": sum(1 for j in range(m) if rep[j] == j)}


def doubles(m, n_incompatible, b_prime, a):
    pairs = m * (m - 1) // 2
    return (float(n_incompatible) / float(pairs) if pairs else float("nan"), float(b_prime) / float(m - 1) if m > 1 else float("nan"),
            float(b_prime + a) / float(m) if m else float("nan"))


def hudson_kaplan(inc):
    """Hudson & Kaplan 1985, literally: list the intervals (i, j), i < j, of all incompatible pairs; delete every interval that
    contains another one; then, from the left, keep an interval and delete those that overlap it (a shared end point is no
    overlap).  -> R_min, the number of intervals left"""
    m = len(inc)
    iv = [(i, j) for i in range(m) for j in range(i + 1, m) if inc[i, j]]
    keep = [a for a in iv if not any(b != a and a[0] <= b[0] and b[1] <= a[1] for b in iv)]
    keep.sort()
    out = []
    while keep:
        i, j = keep[0]
        out.append((i, j))
        keep = [b for b in keep[1:] if not i < b[0] < j]  # no interval contains another: the later ones begin right of i
    return len(out)


def reference(m01, flags, windows, min_mac=2, max_sites=4096, weights=None):
    """-> (records as a dict of arrays, used_sites [n_windows, max_sites] uint64, site_table as a dict of [n_windows, max_sites])"""
    P = lc.members(m01, flags)
    n = len(P)
    rowsP = m01[P]
    qual = lc.qualifying(m01, flags, min_mac)
    rec = {k: np.zeros(len(windows), dtype=np.float64 if k in DOUBLES else np.uint64) for k in INTEGERS + DOUBLES}
    used = np.zeros((len(windows), max_sites), dtype=np.uint64)
    table = {k: np.zeros((len(windows), max_sites), dtype=np.uint32) for k in SITE_FIELDS}
    for i, (b, e) in enumerate(windows):
        qs = qual[np.searchsorted(qual, b):np.searchsorted(qual, e)]
        q = len(qs)
        sites = [int(qs[r]) for r in lc.thinning_ranks(q, max_sites)]
        m = len(sites)
        used[i, :m] = sites
        inc, cong, c = pair_relations(rowsP[:, sites].T, n)
        left1, n_left, rep = site_rows(inc, cong)
        table["left1"][i, :m], table["n_left"][i, :m], table["rep"][i, :m], table["carriers"][i, :m] = left1, n_left, rep, c
        v = window_values(left1, n_left, rep)
        rec["n_members"][i], rec["n_qualifying"][i], rec["n_used"][i] = n, q, m
        rec["n_sites"][i] = (e - b) if weights is None else int(np.asarray(weights[b:e], dtype=np.int64).sum())
        for k in ("rmin", "n_incompatible", "n_incompatible_adjacent", "n_blocks", "longest_block_sites", "n_congruent_adjacent",
                  "n_congruent_partitions", "n_partitions"):
            rec[k][i] = v[k]
        if m:
            rec["longest_block_begin"][i], rec["longest_block_end"][i] = sites[v["longest"][0]], sites[v["longest"][1]]
        rec["four_gamete_fraction"][i], rec["wall_b"][i], rec["wall_q"][i] = doubles(m, v["n_incompatible"], v["n_congruent_adjacent"],
                                                                                  v["n_congruent_partitions"])
    return rec, used, table


def pair_tiles(rec):
    return int(((rec["n_used"].astype(np.int64) + TILE - 1) // TILE).sum())


def assert_matches(got, ref, where=""):
    """got = (records, used_sites, site_table) of BitMatrix.recomb_scan(want_sites=True, want_site_table=True), ref = reference(...)"""
    rec, used, table = got
    want, wused, wtable = ref
    assert len(rec) == len(wused), where
    for k in INTEGERS:
        assert np.array_equal(rec[k].astype(np.uint64), want[k]), (where, k, rec[k][:12], want[k][:12])
    assert np.array_equal(used, wused), (where, "used_sites")
    for k in SITE_FIELDS:
        assert np.array_equal(table[k], wtable[k]), (where, "site_table", k)
    for k in DOUBLES:
        same = lc.bits(rec[k]) == lc.bits(want[k])
        assert same.all(), (where, k, int(np.flatnonzero(~same)[0]), rec[k][~same][:4], want[k][~same][:4])
    assert (rec["reserved"] == 0).all(), where
