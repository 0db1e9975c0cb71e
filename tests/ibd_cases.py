"""Shared cases of the impop_ibd_scan tests: matrices, pair lists, ranges, rules, maps and window lists, each with the records of
the plain restatement (tests/plain_ibd.py) computed once.  A case is only handed out when, checked here on the CPU, it holds a pair
with no segment, a pair with more than one, a segment of more than one tract, a chain dropped for lacking a seed and a chain
dropped by min_output."""
import functools

import numpy as np

import ibs_cases as ic
import plain_ibd as pd
import plain_ibs as pi

# ---- the known answers of the header ---------------------------------------------------------------------------------------------
KNOWN_DIFFS = [10, 12, 30]
KNOWN_RANGE = (0, 40)
KNOWN_MAP = ([0, 20, 40], [0, 100, 120])
# (rule, map, the segments as (begin, end, len, n_tracts, ibs_sites, flags))
KNOWN = [
    (dict(min_sites=2, min_extend=5, min_seed=12, min_output=20, max_gap=3), None, [(0, 40, 40, 3, 36, pd.OPEN_LEFT | pd.OPEN_RIGHT)]),
    (dict(min_sites=2, min_extend=5, min_seed=12, min_output=20, max_gap=2), None, [(13, 40, 27, 2, 26, pd.OPEN_RIGHT)]),
    (dict(min_sites=2, min_extend=5, min_seed=12, min_output=30, max_gap=2), None, []),
    (dict(min_sites=2, min_extend=10, min_seed=40, min_output=50, max_gap=3), KNOWN_MAP, [(0, 30, 110, 2, 27, pd.OPEN_LEFT)]),
]


def known_matrix():
    m01 = np.zeros((2, 40), dtype=np.uint8)
    m01[1, KNOWN_DIFFS] = 1
    return m01


def assert_nontrivial(want, stats, tag=""):
    rec, seg, _ = want
    assert (rec["n_segments"] == 0).any() and (rec["n_segments"] > 1).any() and (seg["n_tracts"] > 1).any(), f"case {tag}: trivial segments"
    assert stats["no_seed"] > 0 and stats["too_short"] > 0, f"case {tag}: no chain dropped for its seed / its length"


class Case:
    def __init__(self, tag, m01, pairs, rng_be, rule, gmap, windows, mask=None, nontrivial=True):
        self.tag, self.m01, self.pairs, self.rule, self.gmap, self.windows, self.mask = tag, m01, pairs, dict(rule), gmap, windows, mask
        self.b, self.e = rng_be
        self.stats = {}
        self.want = pd.reference(m01, pairs, self.b, self.e, gmap=gmap, windows=windows, stats=self.stats, **rule)
        for a in self.want:
            if a is not None:
                a.setflags(write=False)  # shared among tests: computed once, never changed
        if nontrivial:
            assert_nontrivial(self.want, self.stats, tag)

    def kwargs(self):
        """the arguments of BitMatrix.ibd_scan"""
        kw = dict(self.rule, site_begin=self.b, site_end=self.e, windows=self.windows)
        if self.gmap is not None:
            kw["map_pos"], kw["map_g"] = self.gmap
        if self.mask is not None:
            kw["mask_p"] = self.mask
        elif self.pairs != pi.all_pairs(range(self.m01.shape[0])):
            kw["pairs"] = self.pairs
        return kw


# ---- geometry: all pairs of n haplotypes over [5, 2093) of 2100 sites ------------------------------------------------------------
# breakpoints left of the range, right of it and right of the matrix, two one site apart, a zero-rate interval [700, 900)
GEO_MAP = ([0, 3, 150, 151, 700, 900, 1500, 2000, 2095, 2600], [1000, 1000, 90000, 97000, 400000, 400000, 1300000, 1420000, 1500000, 1500007])
GEO_RULE = dict(min_sites=4, min_extend=6, min_seed=25, min_output=60, max_gap=2)             # sites
GEO_RULE_MAP = dict(min_sites=4, min_extend=3000, min_seed=15000, min_output=40000, max_gap=2)  # units of GEO_MAP


@functools.lru_cache(maxsize=None)
def geometry_case(n, with_map):
    m01 = ic.geometry_matrix(n)
    return Case(f"geo{n}/{'map' if with_map else 'sites'}", m01, pi.all_pairs(range(n)), ic.GEO_RANGE, GEO_RULE_MAP if with_map else GEO_RULE,
                GEO_MAP if with_map else None, ic.window_list(*ic.GEO_RANGE), nontrivial=n > 2)


# ---- the hand-made pair: 704 sites, the range [69, 700), a difference every 8 sites ---------------------------------------------
# tracts [69,72), [73,80), ..., [697,700): 79 of them, more than one 64-tract batch, every gap one site.  No difference at 680: the
# tract [673,688), 15 sites, is the only one of its length and the 77th of the pair: a seed in the last batch only.
HAND_S, HAND_RANGE = 704, (69, 700)
HAND_DIFFS = [p for p in range(72, 700, 8) if p != 680]
HAND_SEED = (673, 688)


@functools.lru_cache(maxsize=None)
def hand_case(max_gap, min_seed=15, min_output=15):
    rng = np.random.default_rng(21900)
    m01 = np.zeros((2, HAND_S), dtype=np.uint8)
    m01[0] = m01[1] = rng.random(HAND_S) < 0.4
    m01[1, HAND_DIFFS] ^= 1
    c = Case(f"hand/gap{max_gap}", m01, [(0, 1)], HAND_RANGE, dict(min_sites=3, min_extend=3, min_seed=min_seed, min_output=min_output, max_gap=max_gap),
             None, [HAND_RANGE, (100, 600), (673, 688), (672, 688)], nontrivial=False)
    assert int(c.want[0]["n_candidates"][0]) == len(HAND_DIFFS) + 1 > 64
    return c
