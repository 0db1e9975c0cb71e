"""The rare-entry decoder of the fixed-WPS scan kernel (run with -m gpu on an MI355X).

For n <= 512 the kernel looks the listed haplotypes of an entry up in a per-workgroup LDS table of population codes and folds
the entries of a tile through their moments (sum m, sum m^2, sum mA mB); which allele the listed haplotypes carry drops out of
the arithmetic.  The records must stay those of the dense stream, byte for byte, and match the CPU oracle.

Shapes: n = 65 and 70 (the smallest split, WPS 3), 257 (the table's second pass over the haplotypes starts at 256), 465
(WPS 15) and 512 (WPS 16: the highest haplotype index, 511, next to the table's entry for unused slots).  The matrices are
crafted: rare columns with 1..3 listed haplotypes of either polarity, haplotypes 0, 31, 32, 255, 256 and n - 1 among them;
windows holding exactly 1 / 255 / 256 / 257 entries (one below, at and above one entry per thread), one with more entries than
two passes of the unrolled loop, a rows-only one, one without a variable site and an empty one.  Masks put the special
haplotypes in P only, A only, B only, in A and B (the overlap leaves both) or nowhere; populations of 0, 1, 2 and 3 haplotypes
make the segregating-site tests 0 < m < nA bite."""
import numpy as np
import pytest

from conftest import stat_close

pytestmark = pytest.mark.gpu

INT_KEYS = ("n_sites", "s_all", "s_p", "s_a", "s_b", "sum_p", "sum_a", "sum_b", "sum_ab")
DBL_KEYS = ("pi", "pi_site", "pi_a", "pi_b", "pi_xy", "dxy", "da", "fst", "tajima_d")
S = 64 * 300 + 13
N_BIG = 3300  # more than 256 threads x 4 entries x 3: full batches of the unrolled loop, then its one-at-a-time tail
WINDOWS = [
    (0, 4000, 4000),        # entries only, N_BIG of them
    (4000, 6000, 0),        # rows only (seq_len 0: pi_site and Tajima's D are NaN)
    (6000, 7000, 1000),     # no variable site
    (6500, 6500, 0),        # empty
    (7000, 7010, 10),       # 1 entry
    (7100, 7400, 0),        # 255 entries
    (7400, 7700, 300),      # 256 entries
    (7700, 8000, 77777),    # 257 entries
    (8000, 10000, 12345),   # mix
    (10001, 10063, 62),
    (10063, S, S - 10063),
    (0, S, S),              # everything again, over several tiles
    (3990, 7405, 0),        # overlapping the others
]


def _special(n):
    return sorted({0, 31, 32, min(255, n - 1), min(256, n - 1), n - 1})


def _crafted(n, seed):
    """0/1 [n, S] with exact counts of rare (1..3 listed haplotypes, either polarity) and common (4 <= c <= n - 4) columns per
    stretch; everything else monomorphic 0 or 1.  Fewer than S / 4 sites vary, so the matrix gets its scan index."""
    rng = np.random.default_rng(seed)
    m = np.repeat((rng.random(S) < 0.5)[None, :].astype(np.uint8), n, axis=0)
    sp = _special(n)

    def rare(lo, hi, count, taken=()):
        free = np.setdiff1d(np.arange(lo, hi), np.asarray(taken, dtype=np.int64))
        idx = np.sort(rng.choice(free, count, replace=False))
        for s in idx:
            k = int(rng.integers(1, 4))
            pool = sp if rng.random() < 0.6 else np.arange(n)
            col = np.zeros(n, np.uint8)
            col[rng.choice(pool, k, replace=False)] = 1
            m[:, s] = col ^ rng.integers(0, 2)
        return idx

    def common(lo, hi, count, taken=()):
        free = np.setdiff1d(np.arange(lo, hi), np.asarray(taken, dtype=np.int64))
        for s in rng.choice(free, count, replace=False):
            col = np.zeros(n, np.uint8)
            col[rng.choice(n, rng.integers(4, n - 3), replace=False)] = 1
            m[:, s] = col

    rare(0, 4000, N_BIG)
    common(4000, 6000, 300)
    rare(7000, 7010, 1)
    rare(7100, 7400, 255)
    rare(7400, 7700, 256)
    rare(7700, 8000, 257)
    for lo, hi, nr, nc in ((8000, 10000, 100, 60), (10000, S, 140, 80)):
        common(lo, hi, nc, taken=rare(lo, hi, nr))
    c = m.sum(axis=0, dtype=np.int64)
    assert int(((c > 0) & (c < n)).sum()) * 4 < S
    return m


def _masks(n, cfg):
    """cfg P / A / B / AB / none: where the special haplotypes go; tiny: populations of 1 and 3 haplotypes, P of 2"""
    rng = np.random.default_rng(1000 + n)
    sp = _special(n)
    if cfg == "tiny":
        P = np.zeros(n, np.uint8); P[[0, 31]] = 1
        A = np.zeros(n, np.uint8); A[32] = 1
        B = np.zeros(n, np.uint8); B[[0, 31, n - 1]] = 1
        return P, A, B
    P = (rng.random(n) < 0.6).astype(np.uint8)
    A = np.zeros(n, np.uint8); A[: n // 2] = 1
    B = np.zeros(n, np.uint8); B[n // 3:] = 1
    P[sp] = cfg == "P"
    A[sp] = cfg in ("A", "AB")
    B[sp] = cfg in ("B", "AB")
    return (None if cfg == "none" else P), A, B


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    assert c.device_name().startswith("gfx950")
    yield c
    c.close()


@pytest.fixture(scope="module", params=(65, 70, 257, 465, 512))
def mats(ctx, request):
    n = request.param
    bits = _crafted(n, 9000 + n)
    split = ctx.upload_dense(bits, keep_hap_major=False)
    dense = ctx.upload_dense(bits, keep_hap_major=False, dense_scan=True)
    info = split.scan_split_info()
    c = bits.sum(axis=0, dtype=np.int64)
    assert info["n_rare"] == int(((c > 0) & (c < n) & (np.minimum(c, n - c) <= 3)).sum()) > N_BIG, info
    yield n, bits, split, dense
    split.free()
    dense.free()


@pytest.mark.parametrize("cfg", ("P", "A", "B", "AB", "none", "tiny"))
def test_split_equals_dense_and_oracle(mats, oracle, cfg):
    from impop_amd.engine import pack_hap_major
    n, bits, split, dense = mats
    P, A, B = _masks(n, cfg)
    got = split.scan(WINDOWS, P, A, B)
    assert got.tobytes() == dense.scan(WINDOWS, P, A, B).tobytes(), (n, cfg)
    # one tile per window and several (tile_blocks = 1: the long windows' entries are cut over many workgroups)
    assert split.scan(WINDOWS, P, A, B, tile_blocks=1).tobytes() == got.tobytes(), (n, cfg)
    ov = A & B
    mp = oracle.pack_mask(np.ones(n, np.uint8) if P is None else P)
    ma, mb = oracle.pack_mask(A & ~ov), oracle.pack_mask(B & ~ov)
    for i, (s0, s1, sl) in enumerate(WINDOWS[:11]):
        want = oracle.window_sitecount(pack_hap_major(bits[:, s0:s1]), n, 0, s1 - s0, mp, ma, mb, sl, 0, 0)
        for k in INT_KEYS:
            assert int(got[i][k]) == int(want[k]), (n, cfg, i, k, int(got[i][k]), int(want[k]))
        for k in DBL_KEYS:
            assert stat_close(k, float(got[i][k]), float(want[k]), float(want["dxy"])), (n, cfg, i, k, float(got[i][k]), want[k])


@pytest.mark.parametrize("s_scope", (0, 1))
def test_s_scope_and_pi_mode(mats, s_scope):
    n, bits, split, dense = mats
    P, A, B = _masks(n, "AB")
    for d_pi_mode in (1, 2):
        assert split.scan(WINDOWS, P, A, B, d_pi_mode, s_scope).tobytes() == dense.scan(WINDOWS, P, A, B, d_pi_mode, s_scope).tobytes()
