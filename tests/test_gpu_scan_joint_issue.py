"""The unique-row route's kernel at the edges of its streams (run with -m gpu on an MI355X): entry counts around the batch of
the entry loop, singleton ranges around a batch of SU = 4 words per thread (a word that no lane of a wave holds is skipped by a
ballot, so every start and end alignment and ranges of one word matter), tiles of 0 .. 21 blocks of rows, heads, tails and ranges
of the distinct-row stream that begin and end at every lane that bounds a cache line, and the tile reduction's wave sums in the
VALU.  The records must stay, byte for byte, those of the same bits uploaded without the distinct-row stream and without any
index, and match the CPU oracle.

The crafted matrix (31 000 sites, 7 600 of them variable so that it keeps its index):
  G   4120 singletons side by side from site 0: a window [x, x + c) of them is the range [x, x + c) of the singleton stream, read
      as the 8-byte words [x / 4, ceil((x + c) / 4)).  Ranges of 1023, 1024 and 1025 words (256 SU - 1, 256 SU, 256 SU + 1) and
      of one word, with every start alignment x % 4 and every end alignment (x + c) % 4.
  M   520 sites of minor count 2 or 3 side by side: a window of k of them holds k entries.  k = 0, 1, 2, 255, 256, 257 (one entry a
      thread, more or less) and 515; a window that ends G and begins M holds both streams.
  R   43 blocks of 64 common rows, row j at site R0 + 4 j + 1 and a window edge "at row j" at site R0 + 4 j; 250 rare sites at
      sites R0 + 4 j + 3.  Blocks 0 .. 17 repeat few rows (F_REPS distinct ones each, either polarity), so that the stream's
      prefix before blocks 1, 2, 3, 4 is 64, 65, 127, 128 and before block 13 is 257: ranges of the stream that begin and end at
      0, 1, 63 and 64 within a block of it.  Blocks 18 .. 42 are 64 distinct rows each: a tile there reads its rows, and its
      blocks number 0 .. 21: none, fewer than the four waves, and past a whole turn of eight, four or two blocks in flight a wave.
At the default tiling and n = 465 or 512 every window of a list is one tile (asserted); at n = 65 the budget of a tile is 24 KB:
the windows over R are single tiles (asserted) and the large singleton ranges are cut, as they are with tile_blocks 1 and 2."""
import numpy as np
import pytest

from conftest import stat_close

pytestmark = pytest.mark.gpu

INT_KEYS = ("n_sites", "s_all", "s_p", "s_a", "s_b", "sum_p", "sum_a", "sum_b", "sum_ab")
DBL_KEYS = ("pi", "pi_site", "pi_a", "pi_b", "pi_xy", "dxy", "da", "fst", "tajima_d")
S = 31000
NG, NM = 4120, 520
G0, M0, R0 = 0, NG, NG + NM + 20
F_REPS = (64, 1, 62, 1, 16, 16, 16, 16, 16, 16, 16, 16, 1, 1, 32, 32, 1, 1)
NF, NU = len(F_REPS), 25
NC = 64 * (NF + NU)
EDGES = (0, 1, 3, 4, 5, 7, 8, 9, 31, 63, 64)  # the 4-lane and 8-lane line boundaries of a 16-byte-per-lane load, and the ends


def _row_site(j):
    return R0 + 4 * j


def _rows(a, b, seq_len=None):
    """a window over the common rows [a, b) and the rare sites between them"""
    return (_row_site(a), _row_site(b), b - a if seq_len is None else seq_len)


# (first whole block, one past the last) of windows in F: the ranges of the stream [64, 128) [64, 127) [65, 128) [127, 160)
# [224, 257) and, through the 32-a-block part, [257, 322); the window begins in the block before and ends in the block after
F_MIDS = ((1, 4), (1, 3), (2, 4), (3, 6), (10, 13), (13, 16))


def _window_lists():
    lists = []
    singles = ((0, 4089), (1, 4093), (2, 4097), (3, 1), (1, 2), (0, 4), (2, 3), (3, 4), (1, 1023), (0, 1024), (2, 1027))
    entries = (255, 256, 257, 515, 1, 0, 2, 256, 255, 257, 515)
    for i in range(11):
        e0, e1 = EDGES[i], EDGES[(3 * i + 2) % 11]
        g0, g1 = F_MIDS[i % len(F_MIDS)]
        x, c = singles[i]
        k = entries[i]
        wl = [(G0 + x, G0 + x + c, c)]                                  # singletons only
        if i % 2:
            wl.append((M0 + 3, M0 + 3 + k, 7))                          # entries only
        else:
            wl.append((G0 + NG - 5 - i, M0 + k, 50))                    # the end of G and the beginning of M: both streams, no row
        wl.append(_rows(64 * (g0 - 1) + e0, 64 * g1 + e1))              # head | representatives | tail, every edge
        u0 = 64 * NF                                                    # the distinct blocks: about i and exactly 21 - i items
        wl.append(_rows(u0 + 64 + e0 % 64, u0 + 64 + 64 * i + e1 % 64, 1000))
        b = u0 + 64 * (i + 3)
        wl.append(_rows(b + e1 % 64, b + 64 * (21 - i) - (63 - e0 % 64)))
        wl.append(_rows(64 * 7 + min(e0, 60), 64 * 7 + min(e0, 60) + 1 + i))  # one partial block only
        wl.append((S - 40, S - 40, 0))                                  # empty
        lists.append([w for w in wl if w[0] <= w[1]])
    # no head (the window begins on a block), no tail, neither; no representative (one whole block never takes the stream)
    lists.append([_rows(64, 64 * 4 + 9), _rows(64 * 5 + 31, 64 * 9), _rows(64 * 10, 64 * 13), _rows(64 * 14 + 5, 64 * 15 + 64 + 3),
                  (0, S, S)])
    return lists


LISTS = _window_lists()


def _masks(n, cfg):
    rng = np.random.default_rng(700 + n)
    P = (rng.random(n) < 0.6).astype(np.uint8)
    A = np.zeros(n, np.uint8); A[: n // 3] = 1
    B = np.zeros(n, np.uint8); B[n // 2 + 2:] = 1
    if cfg == "overlap":  # haplotypes in A and B: the plan takes them out of both
        A[: n // 2] = 1
        B[n // 4: n // 2] = 1
    return (None if cfg == "noP" else P), A, B


CFGS = ("P", "noP", "overlap")


def _crafted(n, seed):
    rng = np.random.default_rng(seed)
    m = np.zeros((n, S), np.uint8)

    def rare(site, k):
        col = np.zeros(n, np.uint8)
        col[rng.choice(n, k, replace=False)] = 1
        m[:, site] = col ^ rng.integers(0, 2)

    def row():
        r = np.zeros(n, np.uint8)
        r[rng.choice(n, rng.integers(4, n - 3), replace=False)] = 1
        return r

    for s in range(NG):
        rare(G0 + s, 1)
    for s in range(NM):
        rare(M0 + s, int(rng.integers(2, 4)))
    j = 0
    for reps in F_REPS + (64,) * NU:
        pool = [row() for _ in range(reps)]
        for q in range(64):
            x = pool[q % reps]
            m[:, _row_site(j) + 1] = (1 - x) if (reps < 64 and rng.random() < 0.5) else x
            j += 1
    for jj in rng.choice(NC, 250, replace=False):
        rare(_row_site(int(jj)) + 3, int(rng.integers(1, 4)))
    c = m.sum(axis=0, dtype=np.int64)
    assert int(((c > 0) & (c < n)).sum()) * 4 < S  # else the matrix gets no index
    assert int((np.minimum(c, n - c) > 3).sum()) == NC
    return m


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    assert c.device_name().startswith("gfx950")
    yield c
    c.close()


@pytest.fixture(scope="module", params=(65, 465, 512))
def mats(ctx, request):
    n = request.param
    bits = _crafted(n, 2400 + n)
    uniq = ctx.upload_dense(bits, keep_hap_major=False)
    plain = ctx.upload_dense(bits, keep_hap_major=False, unique_rows=False)
    dense = ctx.upload_dense(bits, keep_hap_major=False, dense_scan=True)
    want = {(cfg, i): dense.scan(wl, *_masks(n, cfg)) for cfg in CFGS for i, wl in enumerate(LISTS)}  # once, shared, unchanged
    yield n, bits, uniq, plain, want
    for m in (uniq, plain, dense):
        m.free()


def test_matrix_has_the_streams(mats):
    n, bits, uniq, plain, want = mats
    info = uniq.scan_unique_info()
    assert info["n_common"] == NC and info["n_unique"] == sum(F_REPS) + 64 * NU and info["why"] == "", info
    assert uniq.scan_single_info()["n_single"] >= NG
    assert plain.scan_unique_info()["n_unique"] == 0


@pytest.mark.parametrize("cfg", CFGS)
def test_records_equal_plain_and_dense(mats, cfg):
    n, bits, uniq, plain, want = mats
    P, A, B = _masks(n, cfg)
    for i, wl in enumerate(LISTS):
        ref = want[(cfg, i)].tobytes()
        for tb in (0, 1, 2):
            assert uniq.scan(wl, P, A, B, tile_blocks=tb).tobytes() == ref, (n, cfg, i, tb)
            assert plain.scan(wl, P, A, B, tile_blocks=tb).tobytes() == ref, (n, cfg, i, tb)


def test_crafted_windows_are_single_tiles(mats):
    """default tiling: a list's windows are disjoint, so its tiles are its non-empty windows, one each — the entry counts,
    singleton ranges and item totals of the docstring are those of single tiles.  n = 65 (a tile's budget is 32 blocks of 768
    bytes, which the large singleton ranges exceed): the windows over R, the ones with up to 21 blocks."""
    n, bits, uniq, plain, want = mats
    P, A, B = _masks(n, "P")
    for i, wl in enumerate(LISTS[:11]):
        if n < 465:
            wl = [w for w in wl if w[0] >= R0]
        pl = uniq.plan(wl, P, A, B)
        tiles = pl.n_tiles
        pl.destroy()
        assert tiles == sum(1 for w in wl if w[1] > w[0]), (n, i, tiles)


def test_stream_ranges_are_where_the_docstring_says(mats):
    """a window of F alone is one tile: its bytes are its head's and its tail's block of rows, the blocks of the stream that the
    representatives of its whole blocks touch — from the prefix sums of F_REPS — each with 64 weight bytes, 8 bytes per entry and
    the 8-byte words its singletons touch"""
    n, bits, uniq, plain, want = mats
    wps = (n + 31) // 32
    c = bits.sum(axis=0, dtype=np.int64)
    mac = np.minimum(c, n - c)
    n_single, n_multi, n_common = (np.concatenate([[0], np.cumsum(k)]) for k in (mac == 1, (mac == 2) | (mac == 3), mac > 3))
    pre = np.concatenate([[0], np.cumsum(F_REPS)])
    assert [int(pre[g]) for g in (1, 2, 3, 4, 13)] == [64, 65, 127, 128, 257]
    P, A, B = _masks(n, "P")
    for i in range(11):
        g0, g1 = F_MIDS[i % len(F_MIDS)]
        w = _rows(64 * (g0 - 1) + EDGES[i], 64 * g1 + EDGES[(3 * i + 2) % 11])
        cb, ce = int(n_common[w[0]]), int(n_common[w[1]])
        m0, m1 = (cb + 63) // 64, ce // 64
        u0, u1 = int(pre[m0]), int(pre[m1])
        s0, s1 = int(n_single[w[0]]), int(n_single[w[1]])
        stream = ((u1 + 63) // 64 - u0 // 64) * (256 * wps + 64)
        assert m1 - m0 >= 2 and stream < (m1 - m0) * 256 * wps, (n, i, (m0, m1), (u0, u1))  # the tile takes the stream
        rows = ((cb % 64 != 0) + (ce % 64 != 0)) * 256 * wps + stream
        rare = 8 * int(n_multi[w[1]] - n_multi[w[0]]) + (8 * ((s1 + 3) // 4 - s0 // 4) if s1 > s0 else 0)
        pl = uniq.plan([w], P, A, B)
        got = (pl.n_tiles, pl.bytes_streamed)
        pl.destroy()
        assert got == (1, rows + rare), (n, i, w, (m0, m1), (u0, u1), got, rows, rare)


def test_oracle_sample(mats, oracle):
    from impop_amd.engine import pack_hap_major
    n, bits, uniq, plain, want = mats
    for cfg in ("P", "overlap"):
        P, A, B = _masks(n, cfg)
        ov = A & B
        mp = oracle.pack_mask(np.ones(n, np.uint8) if P is None else P)
        ma, mb = oracle.pack_mask(A & ~ov), oracle.pack_mask(B & ~ov)
        for i in (0, 3, 7, 11):
            wl, got = LISTS[i], uniq.scan(LISTS[i], P, A, B)
            for w in range(len(wl)):
                s0, s1, sl = wl[w]
                if s1 - s0 > 12000:
                    continue
                ref = oracle.window_sitecount(pack_hap_major(bits[:, s0:s1]), n, 0, s1 - s0, mp, ma, mb, sl, 0, 0)
                for k in INT_KEYS:
                    assert int(got[w][k]) == int(ref[k]), (n, cfg, i, w, k, int(got[w][k]), int(ref[k]))
                for k in DBL_KEYS:
                    assert stat_close(k, float(got[w][k]), float(ref[k]), float(ref["dxy"])), (n, cfg, i, w, k, float(got[w][k]), ref[k])


def test_set_masks_between_launches(mats):
    """the masks are kernel arguments: one plan, two launches, the records follow the masks"""
    n, bits, uniq, plain, want = mats
    P, A, B = _masks(n, "P")
    P2, A2, B2 = _masks(n, "overlap")
    for tb in (0, 2):
        pl = uniq.plan(LISTS[0], P, A, B, tile_blocks=tb)
        try:
            pl.launch()
            r1 = pl.fetch()
            pl.set_masks(P2, A2, B2)
            pl.launch()
            r2 = pl.fetch()
        finally:
            pl.destroy()
        assert r1.tobytes() == want[("P", 0)].tobytes(), (n, tb)
        assert r2.tobytes() == want[("overlap", 0)].tobytes(), (n, tb)
