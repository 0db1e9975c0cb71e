"""The one-wave-per-tile body of the fixed-WPS kernel (scan_tiles_kernel_wave; run with -m gpu on an MI355X): wave w of workgroup g
owns tile 4 g + w, so what matters is the number of tiles mod 4 (idle waves in the last workgroup), tiles without rare sites next
to tiles with them (the table is filled for all), the entry loop and the singleton loop at 64 threads (RU = 4, SU = 5: more than
256 entries or 320 words run them twice), and the 32-bit lane sums, which hold four times as much of a tile as with four waves.
IMPOP_SCAN_WAVE_TILES=1 forces that body where the cap allows (tile_cut.h, wave_tile_fits), =0 forbids it; the records must be,
byte for byte, those of the forced four-wave route, of the same bits without the distinct-row stream, and of the dense matrix.

The matrix is the crafted one of test_gpu_scan_joint_issue (its docstring maps the regions G, M and R): its eleven window lists
hold every alignment of a singleton range, entry counts around 256 and 515, heads, tails and ranges of the stream at every edge,
and tile_blocks 1 and 2 cut them into many small tiles.  On top:
  COUNTS   lists of 1, 2, 3, 4, 5, 7 and 9 disjoint one-tile windows (asserted): every remainder mod 4, alone and behind full
           workgroups; a singleton-only tile of 1290 singletons from alignment 1 (323 words: two batches), an entry-only tile of 300
           entries (two turns of the unrolled loop), row-only tiles, one partial block, no head, no tail
  OVER     overlapping windows: tiles are elementary segments and windows span several
The cap (a child process, which also reads the trace lines): n = 512, every row with c = 256, the largest c (n - c); a tile of
WAVE_BLOCKS_MAX = 512 blocks of distinct rows runs on one wave and a tile of 513 blocks does not, whatever the override says."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import test_gpu_scan_joint_issue as J

pytestmark = pytest.mark.gpu

ENV = "IMPOP_SCAN_WAVE_TILES"
WAVE_BLOCKS_MAX = 512  # tile_cut.h


class _force:
    """the override is read where a plan is made"""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.old = os.environ.get(ENV)
        os.environ[ENV] = self.v

    def __exit__(self, *a):
        if self.old is None:
            del os.environ[ENV]
        else:
            os.environ[ENV] = self.old


def _scan(mat, force, wl, P, A, B, tb=0):
    with _force(force):
        return mat.scan(wl, P, A, B, tile_blocks=tb)


POOL = [
    (J.G0 + 1, J.G0 + 1 + 1290, 1290),          # singletons only, words [0, 323): two batches of 64 x 5
    J._rows(64 * 18 + 5, 64 * 22 + 9),          # distinct rows: five blocks, both edges partial
    (J.M0 + 3, J.M0 + 3 + 300, 7),              # 300 entries only
    J._rows(3, 64 * 4 + 9),                     # head | representatives | tail
    (J.G0 + 1400, J.G0 + 1402, 2),              # two singletons in one word
    J._rows(64 * 7 + 5, 64 * 7 + 9),            # one partial block, no whole block
    J._rows(64 * 10, 64 * 13),                  # neither head nor tail
    (J.G0 + 2002, J.G0 + 2002 + 1283, 1283),    # alignment 2, ends at alignment 1
    J._rows(64 * 30 + 31, 64 * 41),             # head only, ten whole blocks of distinct rows
]
COUNTS = {k: POOL[:k] for k in (1, 2, 3, 4, 5, 7, 9)}
OVER = [J._rows(10, 700), J._rows(300, 1500), J._rows(64 * 18, 64 * 30), (0, 3000, 3000), (2000, 4500, 2500),
        (J.M0 - 50, J._row_site(200), 1), (0, J.S, J.S), (J.M0 + 100, J.M0 + 100, 0)]
EXTRA = list(COUNTS.values()) + [OVER]


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
    bits = J._crafted(n, 2500 + n)
    uniq = ctx.upload_dense(bits, keep_hap_major=False)
    plain = ctx.upload_dense(bits, keep_hap_major=False, unique_rows=False)
    dense = ctx.upload_dense(bits, keep_hap_major=False, dense_scan=True)
    lists = J.LISTS + EXTRA
    want = {(cfg, i): dense.scan(wl, *J._masks(n, cfg)) for cfg in J.CFGS for i, wl in enumerate(lists)}  # once, shared, unchanged
    yield n, uniq, plain, lists, want
    for m in (uniq, plain, dense):
        m.free()


def test_matrix_has_the_stream(mats):
    n, uniq, plain, lists, want = mats
    assert uniq.scan_unique_info()["n_unique"] == sum(J.F_REPS) + 64 * J.NU and plain.scan_unique_info()["n_unique"] == 0


@pytest.mark.parametrize("cfg", J.CFGS)
def test_one_wave_records_equal_four_wave_plain_and_dense(mats, cfg):
    n, uniq, plain, lists, want = mats
    P, A, B = J._masks(n, cfg)
    for i, wl in enumerate(lists):
        ref = want[(cfg, i)].tobytes()
        for tb in (0, 1, 2):
            assert _scan(uniq, "1", wl, P, A, B, tb).tobytes() == ref, (n, cfg, i, tb, "one wave")
            assert _scan(uniq, "0", wl, P, A, B, tb).tobytes() == ref, (n, cfg, i, tb, "four waves")
            assert _scan(plain, "1", wl, P, A, B, tb).tobytes() == ref, (n, cfg, i, tb, "plain")


def test_tile_counts(mats):
    """a COUNTS list of k windows is k tiles: k mod 4 waves of the last workgroup have a tile.  n = 65: a tile's budget is 24 KB,
    which every window of the pool stays under as well"""
    n, uniq, plain, lists, want = mats
    P, A, B = J._masks(n, "P")
    for k, wl in COUNTS.items():
        with _force("1"):
            pl = uniq.plan(wl, P, A, B)
        tiles = pl.n_tiles
        pl.destroy()
        assert tiles == k, (n, k, tiles)


def test_set_masks_between_launches(mats):
    """the masks are kernel arguments and the table is filled from them at every launch"""
    n, uniq, plain, lists, want = mats
    P, A, B = J._masks(n, "P")
    P2, A2, B2 = J._masks(n, "overlap")
    for i in (0, len(J.LISTS) + 6):  # a list of the crafted eleven, the nine tiles of COUNTS
        for tb in (0, 2):
            with _force("1"):
                pl = uniq.plan(lists[i], P, A, B, tile_blocks=tb)
            try:
                pl.launch()
                r1 = pl.fetch()
                pl.set_masks(P2, A2, B2)
                pl.launch()
                r2 = pl.fetch()
            finally:
                pl.destroy()
            assert r1.tobytes() == want[("P", i)].tobytes(), (n, i, tb)
            assert r2.tobytes() == want[("overlap", i)].tobytes(), (n, i, tb)


# ---- the trace line and the cap, in a child process (IMPOP_TRACE is read once per process) ----
N_CAP = 512
CAP_DISTINCT, CAP_REPEATS = WAVE_BLOCKS_MAX + 1, 200  # blocks of 64 distinct rows, then blocks of one row 64 times: the matrix
# keeps the stream while its representatives are at most 3/4 of its common rows — (513 x 64 + 200) / (713 x 64) = 0.72
S_CAP = 4 * 64 * (CAP_DISTINCT + CAP_REPEATS) + 200  # the common rows side by side from site 0; few enough to keep the index
_SCAN = re.compile(r"\[impop_scan\] (.*)$")


def _cap_bits():
    rng = np.random.default_rng(77)
    rows = 64 * CAP_DISTINCT
    half = np.zeros((rows, N_CAP), np.uint8)
    half[:, : N_CAP // 2] = 1
    bits = np.zeros((N_CAP, S_CAP), np.uint8)
    bits[:, :rows] = rng.permuted(half, axis=1).T  # c = 256 in every row: c (n - c) = 2^16
    bits[: N_CAP // 2, rows: rows + 64 * CAP_REPEATS] = 1
    return bits


def _child():
    import impop_amd
    ctx = impop_amd.Context(0)

    def mark(tag):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()

    n = 465
    bits = J._crafted(n, 2500 + n)
    uniq = ctx.upload_dense(bits, keep_hap_major=False)
    P, A, B = J._masks(n, "P")
    for force in ("1", "0", None):
        for k, wl in COUNTS.items():
            mark(f"counts_{k}_{force}")
            if force is None:
                uniq.plan(wl, P, A, B).destroy()
            else:
                with _force(force):
                    uniq.plan(wl, P, A, B).destroy()
    mark("other")  # whatever traces from here on is not a line of the plans above
    uniq.free()
    bits = _cap_bits()
    P = (np.arange(N_CAP) % 3 != 0).astype(np.uint8)
    A = (np.arange(N_CAP) < N_CAP // 2).astype(np.uint8)
    B = 1 - A
    mats = {"uniq": ctx.upload_dense(bits, keep_hap_major=False), "plain": ctx.upload_dense(bits, keep_hap_major=False, unique_rows=False),
            "dense": ctx.upload_dense(bits, keep_hap_major=False, dense_scan=True)}
    for tag, blocks in (("at_cap", WAVE_BLOCKS_MAX), ("above_cap", WAVE_BLOCKS_MAX + 1)):
        wl = [(0, 64 * blocks, 64 * blocks)]
        for mask_p in (None, P):
            want = mats["dense"].scan(wl, mask_p, A, B).tobytes()
            mark(f"{tag}_one")
            with _force("1"):
                pl = mats["uniq"].plan(wl, mask_p, A, B, tile_blocks=4096)
            tiles = pl.n_tiles
            pl.launch()
            one = pl.fetch().tobytes()
            pl.destroy()
            mark("other")
            same = one == want and _scan(mats["uniq"], "0", wl, mask_p, A, B, 4096).tobytes() == want and \
                mats["plain"].scan(wl, mask_p, A, B, tile_blocks=4096).tobytes() == want
            sys.stderr.write(f"@@same {tag} {int(mask_p is not None)} {tiles} {int(same)}\n")
    for m in mats.values():
        m.free()
    ctx.close()


@pytest.fixture(scope="module")
def child():
    env = dict(os.environ, IMPOP_TRACE="1")
    env.pop(ENV, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    traces, same, cur = {}, [], None
    for line in r.stderr.splitlines():
        if line.startswith("@@call "):
            cur = line[7:]
        elif line.startswith("@@same "):
            same.append(line.split()[1:])
        else:
            mt = _SCAN.search(line)
            if mt and cur is not None:
                head = mt.group(1).partition(" why=")[0]
                traces.setdefault(cur, []).append(dict(kv.split("=", 1) for kv in head.split()))
    return traces, same


def test_trace_reports_the_body(child):
    """forced on: one wave per tile; forced off: never; neither: the rule, which refuses a plan of fewer than 8 tiles per CU"""
    traces, same = child
    for k in COUNTS:
        for force, flag in (("1", "1"), ("0", "0"), (None, "0")):
            got = traces[f"counts_{k}_{force}"]
            assert len(got) == 1, (k, force, got)
            t = got[0]
            assert t["wave_tiles"] == flag and int(t["tiles"]) == k and int(t["unique_rows"]) > 0, (k, force, t)


def test_tile_at_the_cap_and_plan_above_it(child):
    """512 blocks of rows at c (n - c) = 2^16 each put 2^25 into a lane's sum_p, 64 x 2^25 into the tile's; 513 blocks are above the
    cap and the plan reports wave_tiles=0 under IMPOP_SCAN_WAVE_TILES=1"""
    traces, same = child
    assert same == [["at_cap", "0", "1", "1"], ["at_cap", "1", "1", "1"], ["above_cap", "0", "1", "1"], ["above_cap", "1", "1", "1"]], same
    assert [t["wave_tiles"] for t in traces["at_cap_one"]] == ["1", "1"], traces["at_cap_one"]
    assert [t["wave_tiles"] for t in traces["above_cap_one"]] == ["0", "0"], traces["above_cap_one"]


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        sys.path.insert(0, ROOT)
        _child()
