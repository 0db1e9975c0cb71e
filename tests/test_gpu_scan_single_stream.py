"""The singleton stream of the split scan index (run with -m gpu on an MI355X).

A split index of 65..512 haplotypes keeps its rare sites once more as two packed streams: one uint16 per singleton site (the
index of its one minor-allele carrier) and the 8-byte entries of the MAC 2-3 sites alone.  Plans of the fixed-WPS scan kernel
read those (the packed route), 2 bytes per singleton instead of 8; every other call keeps reading the complete 8-byte entries.
The records must stay, byte for byte, those of the same matrix made without the stream (IMPOP_KEEP_NO_SINGLE_STREAM) and
without any index (IMPOP_KEEP_DENSE_SCAN), and match the CPU oracle.

Shapes: n = 65 and 70 (WPS 3, the smallest split), 257, 465 (WPS 15) and 512 (WPS 16, haplotype 511 next to the table's entry
for padding).  The crafted matrix has a stretch where every site is a singleton (64 per block; there a site's index is its
place in the stream, so window edges put the range at every offset mod 4 at both ends), one with MAC 2-3 and common sites but
no singleton, a monomorphic one, and a mix whose singletons sit at haplotypes 0, n - 1, in no population or anywhere, in both
polarities.  tile_blocks 1 and 4 cut the singleton run into many tiles (96 rare sites per tile at n = 65).  A second crafted
matrix, 70 haplotypes by 64 * 2048 + 13 sites, puts all three site classes on both sides of the 1024-block chunk boundaries of
the index's block prefix."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, stat_close

pytestmark = pytest.mark.gpu

INT_KEYS = ("n_sites", "s_all", "s_p", "s_a", "s_b", "sum_p", "sum_a", "sum_b", "sum_ab")
DBL_KEYS = ("pi", "pi_site", "pi_a", "pi_b", "pi_xy", "dxy", "da", "fst", "tajima_d")
S = 64 * 100 + 13
R1, R2, R3 = 640, 1280, 1920  # ends of the singleton-only, the no-singleton and the monomorphic stretch
WINDOWS = (
    [(a, b, b - a) for a in (4, 5, 6, 7) for b in (100, 101, 102, 103)]   # every offset mod 4 at both ends; nested, overlapping
    + [(5, 6, 1), (639, 640, 0), (700, 701, 1), (1300, 1301, 1)]           # one site: a singleton, the run's last, other, monomorphic
    + [(9, 9, 0), (S, S, 0), (1300, 1900, 600)]                            # empty, empty at the end, no variable site
    + [(0, S, S), (0, 3000, 3000), (500, 2500, 0), (1000, 2000, 77777), (R1 - 3, R1 + 3, 6), (0, R1, R1), (R1, R2, 0)]
    + [(s, min(s + 500, S), 500) for s in range(R3, S, 500)]
    + [(S - 13, S, 13), (63, 65, 2), (1, 2, 1)]
)
ORACLE_WINDOWS = (0, 5, 10, 15, 16, 17, 18, 23, 24, 28, 29, 30, len(WINDOWS) - 3)


def _special(n):
    """haplotype 0, haplotype n - 1 and two that _masks keeps out of every population"""
    return [0, n - 1, n // 2, n // 2 + 1]


def _crafted(n, seed):
    rng = np.random.default_rng(seed)
    m = np.repeat((rng.random(S) < 0.5)[None, :].astype(np.uint8), n, axis=0)  # monomorphic 0 or 1
    sp = _special(n)

    def singleton(s):
        h = sp[rng.integers(0, len(sp))] if rng.random() < 0.5 else rng.integers(0, n)
        col = np.zeros(n, np.uint8)
        col[h] = 1
        m[:, s] = col ^ rng.integers(0, 2)  # c = 1 or c = n - 1

    def multi(s):
        col = np.zeros(n, np.uint8)
        pool = sp if rng.random() < 0.5 else np.arange(n)
        col[rng.choice(pool, rng.integers(2, 4), replace=False)] = 1
        m[:, s] = col ^ rng.integers(0, 2)

    def common(s):
        col = np.zeros(n, np.uint8)
        col[rng.choice(n, rng.integers(4, n - 3), replace=False)] = 1
        m[:, s] = col

    for s in range(0, R1):
        singleton(s)
    for s in rng.choice(np.arange(R1, R2), 150, replace=False):
        multi(s) if rng.random() < 0.6 else common(s)
    free = np.setdiff1d(np.arange(R3, S), np.arange(2560, 2688))  # two blocks of the mix without a singleton
    pick = rng.choice(free, 560, replace=False)
    for s in pick[:330]:
        singleton(s)
    for s in pick[330:450]:
        multi(s)
    for s in pick[450:]:
        common(s)
    for s in rng.choice(np.arange(2560, 2688), 20, replace=False):
        multi(s)
    c = m.sum(axis=0, dtype=np.int64)
    assert int(((c > 0) & (c < n)).sum()) * 4 < S  # else the matrix gets no index
    return m


def _masks(n, cfg):
    """-> P (or None), A, B as 0/1 vectors.  The special haplotypes n // 2 and n // 2 + 1 are in no population."""
    rng = np.random.default_rng(500 + n)
    P = (rng.random(n) < 0.6).astype(np.uint8)
    A = np.zeros(n, np.uint8); A[: n // 3] = 1
    B = np.zeros(n, np.uint8); B[n // 2 + 2:] = 1
    if cfg == "overlap":    # haplotypes in A and B: the plan takes them out of both
        A[: n // 2] = 1
        B[n // 4: n // 2] = 1
    elif cfg == "A1":       # A of one haplotype: no site segregates in A
        A[:] = 0
        A[0] = 1
    elif cfg == "emptyB":
        B[:] = 0
    P[_special(n)[2:]] = 0
    return (None if cfg == "noP" else P), A, B


CFGS = ("P", "noP", "overlap", "A1", "emptyB")


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
    bits = _crafted(n, 7000 + n)
    packed = ctx.upload_dense(bits, keep_hap_major=False)
    plain = ctx.upload_dense(bits, keep_hap_major=False, single_stream=False)
    dense = ctx.upload_dense(bits, keep_hap_major=False, dense_scan=True)
    yield n, bits, packed, plain, dense
    for m in (packed, plain, dense):
        m.free()


def _check_oracle(oracle, bits, n, got, P, A, B, which, tag):
    from impop_amd.engine import pack_hap_major
    ov = A & B
    mp = oracle.pack_mask(np.ones(n, np.uint8) if P is None else P)
    ma, mb = oracle.pack_mask(A & ~ov), oracle.pack_mask(B & ~ov)
    for i in which:
        s0, s1, sl = WINDOWS[i]
        want = oracle.window_sitecount(pack_hap_major(bits[:, s0:s1]), n, 0, s1 - s0, mp, ma, mb, sl, 0, 0)
        for k in INT_KEYS:
            assert int(got[i][k]) == int(want[k]), (tag, i, k, int(got[i][k]), int(want[k]))
        for k in DBL_KEYS:
            assert stat_close(k, float(got[i][k]), float(want[k]), float(want["dxy"])), (tag, i, k, float(got[i][k]), want[k])


@pytest.mark.parametrize("cfg", CFGS)
def test_packed_equals_plain_dense_and_oracle(mats, oracle, cfg):
    n, bits, packed, plain, dense = mats
    P, A, B = _masks(n, cfg)
    got = packed.scan(WINDOWS, P, A, B)
    assert got.tobytes() == plain.scan(WINDOWS, P, A, B).tobytes(), (n, cfg)
    assert got.tobytes() == dense.scan(WINDOWS, P, A, B).tobytes(), (n, cfg)
    for tb in (1, 4):  # segments cut into several tiles inside the singleton run
        assert packed.scan(WINDOWS, P, A, B, tile_blocks=tb).tobytes() == got.tobytes(), (n, cfg, tb)
    _check_oracle(oracle, bits, n, got, P, A, B, ORACLE_WINDOWS, (n, cfg))


def test_pi_mode_and_s_scope(mats):
    n, bits, packed, plain, dense = mats
    P, A, B = _masks(n, "overlap")
    for d_pi_mode, s_scope in ((1, 1), (2, 0)):
        assert packed.scan(WINDOWS, P, A, B, d_pi_mode, s_scope).tobytes() == dense.scan(WINDOWS, P, A, B, d_pi_mode, s_scope).tobytes()


def test_set_masks_between_launches(mats):
    n, bits, packed, plain, dense = mats
    P, A, B = _masks(n, "P")
    pl = packed.plan(WINDOWS, P, A, B, tile_blocks=4)
    pl.launch()
    r1 = pl.fetch()
    P2, A2, B2 = _masks(n, "A1")
    pl.set_masks(P2, A2, B2)
    pl.launch()
    r2 = pl.fetch()
    pl.destroy()
    assert r1.tobytes() == dense.scan(WINDOWS, P, A, B).tobytes(), n
    assert r2.tobytes() == dense.scan(WINDOWS, P2, A2, B2).tobytes(), n


def test_info_tiles_and_bytes(mats):
    n, bits, packed, plain, dense = mats
    c = bits.sum(axis=0, dtype=np.int64)
    mac = np.minimum(c, n - c)
    n_single, n_multi = int((mac == 1).sum()), int(((mac == 2) | (mac == 3)).sum())
    info = packed.scan_single_info()
    assert (info["n_single"], info["n_multi"], info["why"]) == (n_single, n_multi, ""), info
    n_block = (S + 63) // 64
    assert info["stream_bytes"] == 16 * (n_block + 1) + (2 * n_single + 7) // 8 * 8 + 8 + 8 * n_multi, info
    split = packed.scan_split_info()  # what it reported before: every rare site at 8 bytes
    assert split["n_rare"] == n_single + n_multi and split["rare_bytes"] == 8 * split["n_rare"], split
    assert plain.scan_split_info() == split
    off = plain.scan_single_info()
    assert off["n_single"] == 0 and off["stream_bytes"] == 0 and off["why"].startswith("opted out"), off
    assert packed.scan_index_info()["index_bytes"] == plain.scan_index_info()["index_bytes"] + info["stream_bytes"]
    assert dense.scan_single_info()["why"] != ""
    P, A, B = _masks(n, "P")
    for tb in (0, 1, 4):
        a, b = packed.plan(WINDOWS, P, A, B, tile_blocks=tb), plain.plan(WINDOWS, P, A, B, tile_blocks=tb)
        assert a.n_tiles == b.n_tiles, (n, tb, a.n_tiles, b.n_tiles)
        assert a.bytes_streamed < b.bytes_streamed, (n, tb, a.bytes_streamed, b.bytes_streamed)
        a.destroy()
        b.destroy()
    # one window over the singleton run: 640 singletons as 160 words instead of 640 entries
    a, b = packed.plan([(0, R1, 0)], P, A, B), plain.plan([(0, R1, 0)], P, A, B)
    assert (a.n_tiles, a.bytes_streamed, b.bytes_streamed) == (b.n_tiles, 2 * R1, 8 * R1), (a.bytes_streamed, b.bytes_streamed)
    a.destroy()
    b.destroy()


def test_other_calls_read_the_entries(mats):
    """impop_scan_multi and impop_dstat_scan keep their route: identical records with and without the stream"""
    n, bits, packed, plain, dense = mats
    pops = [(np.arange(n) % 4) == k for k in range(4)]
    assert packed.scan_multi(WINDOWS, pops).tobytes() == plain.scan_multi(WINDOWS, pops).tobytes(), n
    quartets = [(0, 1, 2, 3), (1, 0, 3, 2)]
    assert packed.dstat_scan(WINDOWS, pops, quartets).tobytes() == plain.dstat_scan(WINDOWS, pops, quartets).tobytes(), n


# ---- all three site classes across the chunks of the index's block prefix (1024 blocks each) ----
LONG_N, LONG_S = 70, 64 * 2048 + 13           # 2049 blocks + the entry past the last: three chunks, about 1.1 MB
LONG_B1, LONG_B2 = 64 * 1024, 64 * 2048       # the first sites of the second and of the third chunk
LONG_WINDOWS = [
    (LONG_B1 - 5, LONG_B1 + 7, 12), (LONG_B2 - 3, LONG_B2 + 2, 5),              # a few sites either side of a chunk boundary
    (LONG_B1 - 300, LONG_B1, 300), (LONG_B1, LONG_B1 + 300, 300),               # ending and starting exactly on one
    (LONG_S - 500, LONG_S, 500), (LONG_B2, LONG_S, 13), (0, LONG_S, LONG_S),    # ending at n_site; the whole matrix
    (0, LONG_B1, 0), (LONG_B1 - 64, LONG_B2 + 13, 1), (LONG_B2 - 1, LONG_B2, 1),
]


def _crafted_long():
    """monomorphic but for 4000 singleton, 2000 MAC 2-3 and 2000 common sites anywhere, and 40 sites either side of both chunk
    boundaries that take the three classes in turn"""
    n, rng = LONG_N, np.random.default_rng(1717)
    m = np.repeat((rng.random(LONG_S) < 0.5)[None, :].astype(np.uint8), n, axis=0)
    near = np.concatenate([np.arange(b - 40, min(b + 40, LONG_S)) for b in (LONG_B1, LONG_B2)])
    far = rng.choice(np.setdiff1d(np.arange(LONG_S), near), 8000, replace=False)
    kind = np.concatenate([np.arange(len(near)) % 3, np.repeat([0, 1, 2], [4000, 2000, 2000])])
    for s, k in zip(np.concatenate([near, far]), kind):
        col = np.zeros(n, np.uint8)
        col[rng.choice(n, 1 if k == 0 else rng.integers(2, 4) if k == 1 else rng.integers(4, n - 3), replace=False)] = 1
        m[:, s] = col ^ (rng.integers(0, 2) if k < 2 else 0)
    return m


@pytest.fixture(scope="module")
def long_mats(ctx):
    bits = _crafted_long()
    ms = [ctx.upload_dense(bits, keep_hap_major=False, **kw) for kw in ({}, dict(single_stream=False), dict(dense_scan=True))]
    yield bits, ms
    for m in ms:
        m.free()


def test_classes_across_prefix_chunks(long_mats):
    """the per-block ranks of the kept, the common and the singleton sites all run over three chunks of the block prefix: the
    counts are numpy's, and windows on, at and across the chunk boundaries give the records of the dense stream"""
    bits, (packed, plain, dense) = long_mats
    n = LONG_N
    c = bits.sum(axis=0, dtype=np.int64)
    mac = np.minimum(c, n - c)
    n_kept, n_single, n_multi = int((mac > 0).sum()), int((mac == 1).sum()), int(((mac == 2) | (mac == 3)).sum())
    for b in (LONG_B1, LONG_B2):  # every class on both sides of both boundaries
        for side in (mac[b - 40:b], mac[b:b + 13]):
            assert (side == 1).any() and ((side == 2) | (side == 3)).any() and (side > 3).any()
    for m in (packed, plain):
        idx, split = m.scan_index_info(), m.scan_split_info()
        assert (idx["n_kept"], idx["why"]) == (n_kept, ""), idx
        assert (split["n_rare"], split["n_common"], split["why"]) == (n_single + n_multi, n_kept - n_single - n_multi, ""), split
    single = packed.scan_single_info()
    assert (single["n_single"], single["n_multi"], single["why"]) == (n_single, n_multi, ""), single
    assert plain.scan_single_info()["n_single"] == 0 and dense.scan_index_info()["n_kept"] == 0
    P, A, B = _masks(n, "P")
    for tb in (0, 4):
        want = dense.scan(LONG_WINDOWS, P, A, B, tile_blocks=tb)
        for m in (packed, plain):
            got = m.scan(LONG_WINDOWS, P, A, B, tile_blocks=tb)
            for k in INT_KEYS + DBL_KEYS:
                assert got[k].tobytes() == want[k].tobytes(), (tb, k, got[k], want[k])
    assert int(want["s_all"][6]) == n_kept  # the whole matrix


def _hip_runtime():
    """the HIP runtime the library is bound to (the one copy in this process), for the stream-capture calls"""
    import ctypes as C
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(paths) == 1, paths
    return C.CDLL(paths.pop())


def test_graph_replay():
    """a packed plan captured into a graph: the masks and the singleton ranges are kernel arguments of the captured launch"""
    import ctypes as C

    import impop_amd
    n = 465
    bits = _crafted(n, 7000 + n)
    P, A, B = _masks(n, "overlap")
    _, A2, B2 = _masks(n, "A1")
    probe = impop_amd.Context(0)  # loads the library, and with it the runtime
    hip = _hip_runtime()
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0  # hipStreamNonBlocking
    c = impop_amd.Context(0, stream=stream.value)
    bm = c.upload_dense(bits, keep_hap_major=False)
    dense = c.upload_dense(bits, keep_hap_major=False, dense_scan=True)
    assert bm.scan_single_info()["n_single"] > 0
    want1, want2 = dense.scan(WINDOWS, P, A, B), dense.scan(WINDOWS, P, A2, B2)
    assert want1.tobytes() != want2.tobytes()
    pl = bm.plan(WINDOWS, P, A, B, tile_blocks=4)
    pl.launch()
    assert pl.fetch().tobytes() == want1.tobytes()
    pl.set_masks(P, A2, B2)  # same P: the context's Tajima constants stay as they are, the capture holds the two kernels only
    c.synchronize()
    assert hip.hipStreamBeginCapture(stream, 0) == 0  # hipStreamCaptureModeGlobal
    pl.launch()
    assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0
    assert hip.hipGraphInstantiate(C.byref(gexec), graph, None, None, C.c_size_t(0)) == 0
    assert pl.fetch().tobytes() == want1.tobytes()  # captured, not run
    for _ in range(2):
        assert hip.hipGraphLaunch(gexec, stream) == 0
    assert pl.fetch().tobytes() == want2.tobytes()
    assert hip.hipGraphExecDestroy(gexec) == 0 and hip.hipGraphDestroy(graph) == 0
    pl.destroy()
    bm.free()
    dense.free()
    c.close()
    probe.close()
    assert hip.hipStreamDestroy(stream) == 0


@pytest.mark.parametrize("kind", ("n64", "n600", "weighted", "nosplit"))
def test_routes_without_the_stream(ctx, kind):
    """no singleton stream, with a reason, and the records of the dense stream"""
    n = {"n64": 64, "n600": 600}.get(kind, 465)
    bits = _crafted(n, 7100 + n)
    bm = ctx.upload_dense(bits, keep_hap_major=False, rare_split=kind != "nosplit")
    dense = ctx.upload_dense(bits, keep_hap_major=False, dense_scan=True)
    if kind == "weighted":
        w = np.random.default_rng(3).integers(1, 50, S).astype(np.uint32)
        bm.set_site_weights(w)
        dense.set_site_weights(w)
    info = bm.scan_single_info()
    assert (info["n_single"], info["n_multi"], info["stream_bytes"]) == (0, 0, 0) and info["why"] != "", (kind, info)
    P, A, B = _masks(n, "P")
    assert bm.scan(WINDOWS, P, A, B).tobytes() == dense.scan(WINDOWS, P, A, B).tobytes(), kind
    bm.free()
    dense.free()


_SCAN = re.compile(r"\[impop_scan\] (.*)$")


def _trace_child():
    import impop_amd
    ctx = impop_amd.Context(0)
    n = 465
    bits = _crafted(n, 7000 + n)
    P, A, B = _masks(n, "P")
    for tag, kw in (("packed", {}), ("plain", dict(single_stream=False))):
        bm = ctx.upload_dense(bits, keep_hap_major=False, **kw)
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        pl = bm.plan(WINDOWS[23:25], P, A, B)  # the whole matrix and its first 3000 sites
        sys.stderr.write(f"@@plan {tag} {pl.n_tiles} {pl.bytes_streamed}\n")
        sys.stderr.write("@@call multi\n")
        sys.stderr.flush()
        bm.scan_multi(WINDOWS[23:25], [(np.arange(n) % 2) == k for k in range(2)])
        pl.destroy()
        bm.free()
    ctx.close()


def test_trace_fields():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child"], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, IMPOP_TRACE="1"), timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    traces, plans, cur = {}, {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@@call "):
            cur = line[7:]
        elif line.startswith("@@plan "):
            _, tag, tiles, nbytes = line.split()
            plans[tag] = (int(tiles), int(nbytes))
        else:
            mt = _SCAN.search(line)
            if mt and cur is not None:
                head = mt.group(1).partition(" why=")[0]
                traces.setdefault(cur, []).append({k: v for k, v in (kv.split("=", 1) for kv in head.split())})
    n = 465
    c = _crafted(n, 7000 + n).sum(axis=0, dtype=np.int64)
    mac = np.minimum(c, n - c)
    n_single, n_rare = int((mac == 1).sum()), int(((mac >= 1) & (mac <= 3)).sum())
    covered = n_rare  # the two windows cover every site (the second lies inside the first: one segment each way)
    packed, plain = traces["packed"][0], traces["plain"][0]
    for t in (packed, plain):
        assert t["split"] == "on" and int(t["rare_sites"]) == n_rare and int(t["rare_bytes"]) == 8 * covered, t
        assert "single_sites" in t and "rare_streamed" in t, t
    assert int(packed["single_sites"]) == n_single and int(plain["single_sites"]) == 0
    assert int(plain["rare_streamed"]) == int(plain["rare_bytes"])
    assert int(packed["rare_streamed"]) < 8 * (n_rare - n_single) + 2 * n_single + 16 * int(packed["tiles"])
    assert int(packed["tiles"]) == int(plain["tiles"]) == plans["packed"][0] == plans["plain"][0]
    assert int(packed["bytes_streamed"]) == plans["packed"][1] < plans["plain"][1] == int(plain["bytes_streamed"])
    assert int(plain["bytes_streamed"]) - int(packed["bytes_streamed"]) == int(plain["rare_streamed"]) - int(packed["rare_streamed"])
    for t in traces["multi"]:  # impop_scan_multi never takes the packed route
        assert int(t["single_sites"]) == 0 and int(t["rare_streamed"]) == int(t["rare_bytes"]) == 8 * covered, t


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--trace-child":
        sys.path.insert(0, ROOT)
        _trace_child()
