"""Shared cases of the impop_diploid_scan tests: matrices, pairings and window lists, each with the records of the plain
restatement (tests/plain_diploid.py) computed once.  A case is only handed out when its run-of-homozygosity fields are non-trivial:
at least one individual with roh_runs > 0 and one with roh_runs == 0."""
import functools

import numpy as np

import plain_diploid as pd

KNOWN_ROWS = ["100010", "000010", "110000", "100001"]  # the header's known answer: haplotype rows over 6 sites
KNOWN_PAIRS = [(0, 1), (2, 3)]


def known_matrix():
    return np.array([[int(ch) for ch in row] for row in KNOWN_ROWS], dtype=np.uint8)


def spectrum_matrix(rng, n, S, p_mono=0.35):
    """independent sites; a share p_mono of them monomorphic (all 0 or all 1), so that a compacted matrix really is shorter, the
    rest with allele frequencies from rare to common"""
    f = rng.choice([0.002, 0.01, 0.05, 0.2, 0.5, 0.9], size=S)
    m = (rng.random((n, S)) < f[None, :]).astype(np.uint8)
    mono = rng.random(S) < p_mono
    m[:, mono] = (rng.random(int(mono.sum())) < 0.3).astype(np.uint8)[None, :]
    return m


def founder_matrix(rng, n, S, nf=4, p_switch=0.004, p_flip=0.0015, p_site=0.3):
    """every haplotype a mosaic of nf founders with long segments and a few private flips: the two copies of an individual are
    often identical over hundreds of sites, so runs of homozygosity are long"""
    founders = (rng.random((nf, S)) < p_site).astype(np.uint8)
    m = np.zeros((n, S), dtype=np.uint8)
    for h in range(n):
        switch = rng.random(S) < p_switch
        src = (rng.integers(0, nf) + np.cumsum(switch * rng.integers(1, nf, size=S))) % nf
        m[h] = founders[src, np.arange(S)]
    m ^= (rng.random((n, S)) < p_flip).astype(np.uint8)
    return m


def pairing(rng, n, leave_out=0.15):
    """pairs over a shuffled part of the haplotypes: members of a pair lie in different dword columns wherever there is more than
    one column ((1, 69) when n >= 70), about half the pairs have h1 > h2, about leave_out of the haplotypes are in no pair"""
    idx = list(range(n))
    pairs = []
    if n >= 70:
        pairs.append((1, 69))
        idx.remove(1)
        idx.remove(69)
    idx = [int(i) for i in rng.permutation(idx)]
    keep = len(idx) if n <= 4 else max(2, int(len(idx) * (1.0 - leave_out)))
    keep -= keep % 2
    for a, b in zip(idx[0:keep:2], idx[1:keep:2]):
        pairs.append((a, b))
    return pairs


def window_list(S):
    """edges off the 64-site boundaries, a window inside one block, one site, the end of the matrix, overlapping and nested
    windows in non-sorted order, the whole matrix (more than four blocks per wave of a default tile never fit in S <= 3000 sites:
    the tests shorten the tile instead, IMPOP_DIPLOID_TILE_BLOCKS), one with a seq_len"""
    w = [(S // 2 - 90, S - 37), (3, 61), (70, 71), (0, S), (S - 1, S), (S - 300, S), (5, S // 2 + 11), (130, 131), (64, 128),
         (S // 2 - 90, S // 2 + 200), (S // 2, S // 2 + 7, 1000), (1, S - 1), (129, 640), (200, 200)]
    return [tuple(int(x) for x in t) for t in w]


def assert_nontrivial(ind, tag=""):
    assert (ind["roh_runs"] > 0).any() and (ind["roh_runs"] == 0).any(), f"case {tag}: the ROH fields are trivial"


class Case:
    def __init__(self, tag, m01, pairs, windows, min_run):
        self.tag, self.m01, self.pairs, self.windows, self.min_run = tag, m01, pairs, windows, min_run
        self.want = pd.reference(m01, pairs, windows, min_run)
        for a in self.want:
            a.setflags(write=False)  # shared among tests: computed once, never changed
        assert_nontrivial(self.want[1], tag)


@functools.lru_cache(maxsize=None)
def geometry_case(n, kind):
    """n_hap = n on 1500 (spectrum) or 2100 (founder) sites"""
    rng = np.random.default_rng(11000 + n + (0 if kind == "spectrum" else 500))
    if kind == "spectrum":
        S, min_run = 1500, 12
        m01 = spectrum_matrix(rng, n, S)
    else:
        S, min_run = 2100, 90
        m01 = founder_matrix(rng, n, S)
    pairs = pairing(rng, n)
    if kind == "founder" and len(pairs) > 1:  # one individual that is heterozygous everywhere: no run at all, roh_runs == 0
        m01[pairs[-1][1]] = 1 - m01[pairs[-1][0]]
    return Case(f"{kind}{n}", m01, pairs, window_list(S), min_run)


# ---- hand-made runs: 704 sites, tiles of 2 blocks (IMPOP_DIPLOID_TILE_BLOCKS=2), the window [69, 600) --------------------------------

RUN_S, RUN_WINDOW, RUN_TILE_BLOCKS = 704, (69, 600), 2
# the window's tiles then end at 192, 320, 448, 576.  Individual 1 is heterozygous at:
RUN_HETS = [69, 120, 140, 180, 200, 460, 599]
# 69 / 599: the first and the last site of the window; 120 -> 140 crosses the block edge 128; 180 -> 200 the tile edge 192;
# 200 -> 460 spans the whole tile [320, 448) and is 259 sites long
RUN_LONG = 259


@functools.lru_cache(maxsize=None)
def run_case(min_run):
    rng = np.random.default_rng(11900)
    m01 = np.zeros((6, RUN_S), dtype=np.uint8)
    m01[0] = m01[1] = rng.random(RUN_S) < 0.4          # individual 0: no heterozygous site, one run of W
    m01[2] = m01[3] = rng.random(RUN_S) < 0.4
    m01[3, RUN_HETS] ^= 1                              # individual 1: exactly RUN_HETS
    m01[4] = rng.random(RUN_S) < 0.5
    m01[5] = m01[4] ^ (np.arange(RUN_S) % 3 != 2)      # individual 2: runs of one site only
    c = Case(f"runs{min_run}", m01, [(0, 1), (3, 2), (4, 5)], [RUN_WINDOW, (0, RUN_S), (69, 70), (599, 600), (140, 461)], min_run)
    row = c.want[1][0, 1]
    assert row["het"] == len(RUN_HETS) and row["longest_run"] == RUN_LONG
    return c
