"""Inputs of the linkage-tree tests (tests/test_gpu_tree_scan.py), kept apart so that the CPU suite can check that they mean
something (tests/test_tree_host.py) without a GPU.

The matrices, window lists and panels are pairdist_cases', the masks pca_cases', unmodified: planted segments, copied rows (merges
at value 0, ties), and three segments in which every haplotype is the same (windows with every value 0: the scheme's worst case).
Panels are given to the call as member POSITIONS of the mask; a panel that the mask leaves empty is dropped (the call refuses empty
panels), so the masks `pair` and `three` see fewer panels than K.

wide_case(): the 128-bit case.  1024 haplotypes in three groups of 512, 255 and 257 over 64 columns: three heavy columns of weight
g each, on which the groups read 000, 110 and 011 — every between-group distance is 2 g — and 61 columns of weight 1 with random
bits (a little sparser in the first two groups), W = 3 g + 61 = 2^31 - 1.  The last three clusters are the groups; their values
S / D are within 1e-9 of one another while their denominators 512 x 255, 512 x 257 and 255 x 257 differ, and the smallest is the
first pair's: deciding it against the second takes products of about 2^30.4 x 2^17 x 2^17 > 2^64.

preconditions() asserts, from the plain restatement alone, what the GPU tests rest on (see its text).
"""
import functools

import numpy as np

import pairdist_cases as pc
import pca_cases as pcs
import plain_pca as pl
import plain_tree as pt

NS = (31, 65)
# 465 and 513 as in the other all-pairs tests; and either side of every switch of the kernel as built: the rows a lane strides
# (multiples of 64) and the workgroup widths (256 threads up to 256 members, 512 up to 512, 1024 beyond)
BIG_NS = (63, 64, 65, 255, 256, 257, 465, 511, 512, 513)
MASKS = pcs.MASKS
LINKAGES = pt.LINKAGES
KS = (0, 2, 3)

members = pcs.members
flags = pcs.flags


@functools.lru_cache(maxsize=None)
def matrix(n):
    return pc.matrix(n)


def pops(n, mask, K):
    """-> the panels of pairdist_cases inside the mask, as lists of haplotype indexes; empty ones dropped"""
    inside = set(members(n, mask))
    return [q for q in ([i for i in p if i in inside] for p in (pc.panels(n, K) if K else [])) if q]


def pop_flags(n, mask, K):
    out = []
    for p in pops(n, mask, K):
        f = np.zeros(n, np.uint8)
        f[p] = 1
        out.append(f)
    return out


def pop_positions(n, mask, K):
    where = {h: i for i, h in enumerate(members(n, mask))}
    return [[where[h] for h in p] for p in pops(n, mask, K)]


@functools.lru_cache(maxsize=None)
def references(n, shape, mask, linkage, K):
    """per window of the list: plain_tree.window"""
    m01 = matrix(n)
    pos = pop_positions(n, mask, K)
    return [pt.window(pl.distances(m01, w[0], w[1], members(n, mask)), w[1] - w[0], linkage, pos) for w in pc.window_lists()[shape]]


# ---- the 128-bit case

WIDE_G = (2 ** 31 - 1 - 61) // 3
WIDE_SIZES = (512, 255, 257)


@functools.lru_cache(maxsize=None)
def wide_case():
    """-> (0/1 matrix [1024, 64], weights uint32 [64], the window (begin, end, seq_len) in columns)"""
    rng = np.random.default_rng(128)
    n, cols = sum(WIDE_SIZES), 64
    a, b = WIDE_SIZES[0], WIDE_SIZES[0] + WIDE_SIZES[1]
    density = np.where(np.arange(n) < b, 0.45, 0.5)[:, None]  # the first two groups a little sparser: theirs is the smallest value
    m01 = (rng.random((n, cols)) < density).astype(np.uint8)
    m01[:a, :3] = (0, 0, 0)
    m01[a:b, :3] = (1, 1, 0)
    m01[b:, :3] = (0, 1, 1)
    wt = np.ones(cols, np.uint32)
    wt[:3] = WIDE_G
    assert int(wt.sum()) == 2 ** 31 - 1
    return m01, wt, (0, cols, 0)


@functools.lru_cache(maxsize=None)
def wide_reference():
    m01, wt, win = wide_case()
    return pt.window(pl.distances(m01, win[0], win[1], weights=wt), int(wt.sum()), "average")


def preconditions():
    """Over the parity cases there are: windows with n_tied_merges > 0 and windows with none; a window with all values 0; a panel
    that is monophyletic in some window and not in another; a merge record set where largest_clade < mrca_size; non-decreasing
    values everywhere.  -> dict of what was seen"""
    seen = dict(tied=0, untied=0, all_zero=0, mono=set(), not_mono=set(), clade_below_mrca=0)
    for n in NS:
        for shape in ("tiling", "sliding"):
            for mask in MASKS:
                for linkage in LINKAGES:
                    for K in KS:
                        for ref in references(n, shape, mask, linkage, K):
                            m = ref["n_members"]
                            assert len(ref["merges"]) == m - 1
                            seen["tied" if ref["n_tied"] else "untied"] += 1
                            if ref["sum_h"] == 0:
                                seen["all_zero"] += 1
                                assert ref["n_zero"] == m - 1 and ref["n_tied"] == m - 2
                                assert [g[:2] for g in ref["merges"]] == [(0, k) for k in range(1, m)]
                            for p, q in enumerate(ref["panels"]):
                                key = (n, mask, K, p)
                                (seen["mono"] if q["mrca_size"] == q["n_members"] else seen["not_mono"]).add(key)
                                seen["clade_below_mrca"] += q["largest_clade"] < q["mrca_size"]
                                assert 1 <= q["largest_clade"] <= q["n_members"] <= q["mrca_size"] <= m
    assert seen["tied"] and seen["untied"] and seen["all_zero"] and seen["clade_below_mrca"], seen
    assert seen["mono"] & seen["not_mono"], "no panel is monophyletic in one window and not in another"
    return seen


def wide_preconditions():
    """the restatement itself compares, in the 128-bit case, values whose cross products pass 2^64"""
    ref = wide_reference()
    assert ref["max_product"] >= 2 ** 64, ref["max_product"]
    assert ref["n_members"] == 1024 and ref["n_sites"] == 2 ** 31 - 1
    return ref["max_product"]
