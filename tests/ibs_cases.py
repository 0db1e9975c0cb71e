"""Shared cases of the impop_ibs_scan tests: matrices, pair lists, ranges and window lists, each with the records of the plain
restatement (tests/plain_ibs.py) computed once.  A case is only handed out when its tracts are non-trivial: at least one pair
with a reported tract, one without, and a pair with more than one."""
import functools

import numpy as np

import dip_cases as dc
import plain_ibs as pi

KNOWN_ROWS = dc.KNOWN_ROWS  # the header's known answer: h0 = 100010, h1 = 000010, h2 = 110000, h3 = 100001
KNOWN_MIN_SITES = 2
KNOWN_WINDOWS = [(0, 6), (2, 4), (3, 6)]
KNOWN_PAIR_ROWS = [(0, 1, 1, 5, 1, 0, 5), (0, 2, 2, 2, 1, 0, 2), (0, 3, 2, 4, 1, 0, 4), (1, 2, 3, 2, 1, 0, 2), (1, 3, 3, 3, 1, 0, 3),
                   (2, 3, 2, 3, 1, 0, 3)]
KNOWN_SEGMENTS = [(0, 1, 1, 6, 0, pi.OPEN_RIGHT), (0, 2, 2, 4, 1, 0), (0, 3, 0, 4, 2, pi.OPEN_LEFT), (1, 2, 2, 4, 3, 0), (1, 3, 1, 4, 4, 0),
                  (2, 3, 2, 5, 5, 0)]
KNOWN_WINDOW_ROWS = [(19, 6, 0), (12, 6, 6), (9, 6, 1)]


def known_matrix():
    return dc.known_matrix()


def assert_nontrivial(rec, tag=""):
    assert (rec["n_tracts"] > 0).any() and (rec["n_tracts"] == 0).any() and (rec["n_tracts"] > 1).any(), f"case {tag}: trivial tracts"


def window_list(b, e):
    """inside [b, e): edges off the 64-site boundaries, one site, an empty window, nested and overlapping windows in non-sorted
    order, a repeated window, the whole range, windows that share an edge"""
    mid = (b + e) // 2
    w = [(mid - 90, e - 37), (b, b + 56), (b + 65, b + 66), (b, e), (e - 1, e), (e - 300, e), (b, mid + 11), (130, 131), (64, 128),
         (mid - 90, mid + 200), (mid, mid + 7), (b + 1, e - 1), (129, 640), (200, 200), (129, 640), (640, 700), (mid + 7, mid + 40)]
    return [tuple(int(x) for x in t) for t in w]


class Case:
    def __init__(self, tag, m01, pairs, rng_be, min_sites, windows, mask=None, nontrivial=True):
        self.tag, self.m01, self.pairs, self.min_sites, self.windows, self.mask = tag, m01, pairs, min_sites, windows, mask
        self.b, self.e = rng_be
        self.want = pi.reference(m01, pairs, self.b, self.e, min_sites, windows)
        for a in self.want:
            if a is not None:
                a.setflags(write=False)  # shared among tests: computed once, never changed
        if nontrivial:
            assert_nontrivial(self.want[0], tag)


GEO_S, GEO_RANGE = 2100, (5, 2093)  # 33 blocks; both edges off the 64-site boundaries


@functools.lru_cache(maxsize=None)
def geometry_matrix(n):
    rng = np.random.default_rng(20000 + n)
    m01 = dc.founder_matrix(rng, n, GEO_S, nf=3 if n > 4 else 2, p_switch=0.004, p_flip=0.002, p_site=0.08)
    if n >= 4:
        m01[n - 1] = 1 - m01[0]  # a pair that differs at every site
    m01.setflags(write=False)
    return m01


@functools.lru_cache(maxsize=None)
def geometry_case(n, min_sites):
    """all pairs of n haplotypes over [5, 2093) of 2100 sites"""
    m01 = geometry_matrix(n)
    return Case(f"geo{n}/{min_sites}", m01, pi.all_pairs(range(n)), GEO_RANGE, min_sites, window_list(*GEO_RANGE), nontrivial=n > 2)


# ---- hand-made rows: 704 sites, the range [69, 700), chunks of 2 blocks and sub-segments of 1 --------------------------------------

HAND_S, HAND_RANGE, HAND_CHUNK_BLOCKS, HAND_SEG_BLOCKS = 704, (69, 700), 2, 1
# the chunks then begin at 64, 192, 320, 448, 576 and every block is a sub-segment.  Rows 4 and 5 differ at:
HAND_DIFFS = [69, 127, 128, 191, 192, 255, 256, 260, 660, 699]
# 69 / 699: the first and the last site of the range; 127 / 128: bits 63 and 0 across a word edge; 191 / 192: across a chunk edge;
# 255 / 256: across a sub-segment edge inside a chunk; 260 -> 660 spans the whole chunks [320, 448) and [448, 576): 399 sites
HAND_LONG = 399
HAND_PAIRS = [(0, 1), (2, 3), (4, 5), (5, 4), (0, 4)]


@functools.lru_cache(maxsize=None)
def hand_case(min_sites):
    rng = np.random.default_rng(20900)
    m01 = np.zeros((6, HAND_S), dtype=np.uint8)
    m01[0] = m01[1] = rng.random(HAND_S) < 0.4  # identical rows: one tract = the range, open on both sides
    m01[2] = rng.random(HAND_S) < 0.5
    m01[3] = 1 - m01[2]                          # different at every site: no tract, longest 0
    m01[4] = m01[5] = rng.random(HAND_S) < 0.4
    m01[5, HAND_DIFFS] ^= 1
    c = Case(f"hand{min_sites}", m01, HAND_PAIRS, HAND_RANGE, min_sites, [HAND_RANGE, (261, 660), (260, 660), (300, 400), (69, 70)],
             nontrivial=False)
    rec, seg, _ = c.want
    b, e = HAND_RANGE
    assert tuple(rec[0])[2:] == (0, e - b, 1 if e - b >= min_sites else 0, 0, e - b if e - b >= min_sites else 0)
    assert tuple(rec[1])[2:] == (e - b, 0, 0, 0, 0)
    assert rec[2]["n_diff"] == len(HAND_DIFFS) and rec[2]["longest"] == HAND_LONG
    return c
