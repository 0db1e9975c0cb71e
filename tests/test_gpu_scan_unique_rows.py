"""The distinct-row stream of the split scan index (run with -m gpu on an MI355X).

A split index of 65..512 haplotypes keeps, per 64-row block of its common rows, the distinct rows once with a one-byte weight:
rows that are equal or each other's complement within the n real haplotypes are one representative.  Plans of the fixed-WPS scan
kernel read a tile's whole blocks from that stream and only the partial blocks at window edges as rows.  The records must stay,
byte for byte, those of the same matrix made without the stream (IMPOP_KEEP_NO_UNIQUE_ROWS) and without any index
(IMPOP_KEEP_DENSE_SCAN), and match the CPU oracle.

Shapes: n = 65 (WPS 3), 465 (WPS 15, 15 padding bits in the last dword) and 512 (WPS 16, none).  The crafted matrix has 64 * 100 +
13 sites; its 64 * 12 + 13 common rows stand at sites 8 j + 3, so a window edge at such a site is an edge at common row j, and the
blocks of common rows are: 0 one row 64 times; 1 a row and its complement, alternating (one representative); 2 64 distinct rows;
3 rows that differ from another in haplotype 0 or n - 1 alone, as they are and complemented (64 representatives: none may fold);
4 carriers inside A only; 5 inside B only; 6 in no population; 7 across both, some complemented; 8 .. 11 draws from a pool of 20
patterns in either polarity; 12 the final 13 rows.  Singletons and MAC 2-3 sites stand between them (sites 8 j + 6)."""
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
NC = 64 * 12 + 13  # common rows


def _site(j):
    """the matrix site a window edge at common row j stands at"""
    return 8 * j + 3 if j < NC else S


def _cw(a, b, seq_len=None):
    """a window over the common rows [a, b)"""
    return (_site(a), _site(b), b - a if seq_len is None else seq_len)


EDGES = (0, 1, 31, 63, 64)  # every position of a block
WINDOWS = (
    [_cw(64 + a, 64 * 6 + b) for a in EDGES for b in EDGES]                     # nested and overlapping: one segment, many windows
    + [_cw(64 * 3 + 5, 64 * 3 + 50), _cw(64 * 2, 64 * 3), _cw(0, 64 * 2)]       # inside one block; exactly one; exactly two
    + [(0, S, S), (9, 9, 0), (S, S, 0), (_site(70), _site(70), 0)]              # everything; empty ones
    + [_cw(a, min(a + 300, NC), 777) for a in range(0, NC, 150)]                # sliding, half overlapping, into the final 13 rows
    + [_cw(64 * 11 + 7, NC), _cw(64 * 12, NC), (1, 2, 1), (0, _site(64 * 4), 0)]
    + [_cw(64 * 7, 64 * 12), _cw(64 * 8 + 63, 64 * 9 + 1, 0)]
)
# The whole list cuts the rows at every edge of every window, which leaves few segments with two whole blocks; the stream is
# read where a tile has at least two.  So the lists are also scanned on their own: the nested ones share the segment [128, 384)
# (four whole blocks), the sliding ones have segments of 150 rows.
LISTS = {"all": WINDOWS, "nested": WINDOWS[:25], "one_each": WINDOWS[25:32], "sliding": WINDOWS[32:38], "rest": WINDOWS[38:]}
ORACLE_WINDOWS = (0, 6, 12, 18, 24, 25, 26, 27, 28, 32, 34, len(WINDOWS) - 6, len(WINDOWS) - 2, len(WINDOWS) - 1)


def _pops(n):
    """the haplotype sets of _masks: A, B and the haplotypes in neither"""
    return np.arange(0, n // 3), np.arange(n // 2 + 2, n), np.arange(n // 3, n // 2 + 2)


def _masks(n, cfg):
    """-> P (or None), A, B as 0/1 vectors: the five configurations of the singleton-stream test"""
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
    P[[n // 2, n // 2 + 1]] = 0
    return (None if cfg == "noP" else P), A, B


CFGS = ("P", "noP", "overlap", "A1", "emptyB")


def _crafted(n, seed, folding=True):
    """folding=False: every common row random, so no block repeats a row and the stream does not pay"""
    rng = np.random.default_rng(seed)
    m = np.repeat((rng.random(S) < 0.5)[None, :].astype(np.uint8), n, axis=0)  # monomorphic 0 or 1
    in_a, in_b, in_none = _pops(n)

    def row(pool=None, lo=4, hi=None):
        """a common row: its carriers drawn from pool, min(c, n - c) > 3"""
        pool = np.arange(n) if pool is None else pool
        hi = min(len(pool), n - 4) if hi is None else hi
        r = np.zeros(n, np.uint8)
        r[rng.choice(pool, rng.integers(lo, hi + 1), replace=False)] = 1
        return r

    def flip(r):
        return (1 - r).astype(np.uint8)

    rows = []
    if not folding:
        rows = [row() for _ in range(NC)]
    else:
        r0 = row()
        rows += [r0] * 64                                                  # 0
        r1 = row()
        rows += [r1 if j % 2 == 0 else flip(r1) for j in range(64)]       # 1
        rows += [row() for _ in range(64)]                                 # 2
        for _ in range(16):                                                # 3
            y = row(np.arange(1, n - 1), 5, n - 7)  # haplotypes 0 and n - 1 carry 0; every variant stays common
            y0, y1, y01 = y.copy(), y.copy(), y.copy()
            y0[0] = y01[0] = 1
            y1[n - 1] = y01[n - 1] = 1
            rows += [y, y0, flip(y01), y1]  # flip(y01) is one haplotype from the complement of y0 and from that of y1
        rows += [x for x in [row(in_a) for _ in range(8)] for _ in range(8)]        # 4
        rows += [x for x in [row(in_b) for _ in range(4)] for _ in range(16)]       # 5
        rows += [x for x in [row(in_none) for _ in range(2)] for _ in range(32)]    # 6
        across = [row(np.concatenate([in_a[:6], in_b[:6]]), 4, 12) for _ in range(16)]
        rows += [across[j % 16] if j % 3 else flip(across[j % 16]) for j in range(64)]  # 7
        pool = [row() for _ in range(20)]
        for j in range(64 * 4 + 13):                                       # 8 .. 11 and the final 13
            x = pool[rng.integers(0, 20)]
            rows.append(flip(x) if rng.random() < 0.5 else x)
    assert len(rows) == NC
    for j, r in enumerate(rows):
        c = int(r.sum())
        assert min(c, n - c) > 3, (j, c)
        m[:, _site(j)] = r
    for j in rng.choice(NC, 300, replace=False):  # rare sites between the rows: singletons, MAC 2 and 3, either polarity
        col = np.zeros(n, np.uint8)
        col[rng.choice(n, rng.integers(1, 4), replace=False)] = 1
        m[:, 8 * j + 6] = col ^ rng.integers(0, 2)
    c = m.sum(axis=0, dtype=np.int64)
    kept = (c > 0) & (c < n)
    assert int(kept.sum()) * 4 < S  # else the matrix gets no index
    assert int((np.minimum(c, n - c) > 3).sum()) == NC
    return m


def _representatives(bits, n):
    """numpy: the distinct rows of every block of 64 common rows, a row and its complement counting once"""
    c = bits.sum(axis=0, dtype=np.int64)
    rows = bits[:, np.minimum(c, n - c) > 3].T.copy()      # common rows in site order
    rows[rows[:, 0] == 1] ^= 1                             # canonical: haplotype 0 carries 0
    return [len(np.unique(rows[b:b + 64], axis=0)) for b in range(0, len(rows), 64)], len(rows)


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
    bits = _crafted(n, 9000 + n)
    uniq = ctx.upload_dense(bits, keep_hap_major=False)
    plain = ctx.upload_dense(bits, keep_hap_major=False, unique_rows=False)
    dense = ctx.upload_dense(bits, keep_hap_major=False, dense_scan=True)
    yield n, bits, uniq, plain, dense
    for m in (uniq, plain, dense):
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


def test_blocks_are_what_the_docstring_says(mats):
    n, bits, uniq, plain, dense = mats
    per_block, n_common = _representatives(bits, n)
    assert n_common == NC and len(per_block) == 13
    assert per_block[:8] == [1, 1, 64, 64, 8, 4, 2, 16] and all(p <= 20 for p in per_block[8:]), per_block
    assert sum(per_block) * 4 <= 3 * NC  # the stream pays


@pytest.mark.parametrize("cfg", CFGS)
def test_unique_equals_plain_dense_and_oracle(mats, oracle, cfg):
    n, bits, uniq, plain, dense = mats
    P, A, B = _masks(n, cfg)
    for name, wl in LISTS.items():
        want = dense.scan(wl, P, A, B)
        for tb in (0, 1, 2):  # 2: the cuts fall between whole blocks; 1: every tile is one block, which reads its rows
            got = uniq.scan(wl, P, A, B, tile_blocks=tb)
            assert got.tobytes() == want.tobytes(), (n, cfg, name, tb)
            assert plain.scan(wl, P, A, B, tile_blocks=tb).tobytes() == want.tobytes(), (n, cfg, name, tb)
        if name == "all":
            _check_oracle(oracle, bits, n, want, P, A, B, ORACLE_WINDOWS, (n, cfg))


def test_set_masks_between_launches(mats):
    """the stream does not depend on the masks: the records follow them (the nested list: tiles that read the stream)"""
    n, bits, uniq, plain, dense = mats
    wl = LISTS["nested"]
    P, A, B = _masks(n, "P")
    P2, A2, B2 = _masks(n, "A1")
    for tb in (0, 2):
        pl = uniq.plan(wl, P, A, B, tile_blocks=tb)
        try:
            pl.launch()
            r1 = pl.fetch()
            pl.set_masks(P2, A2, B2)
            pl.launch()
            r2 = pl.fetch()
        finally:
            pl.destroy()
        assert r1.tobytes() == dense.scan(wl, P, A, B).tobytes(), (n, tb)
        assert r2.tobytes() == dense.scan(wl, P2, A2, B2).tobytes(), (n, tb)


def test_info_tiles_and_bytes(mats):
    n, bits, uniq, plain, dense = mats
    per_block, n_common = _representatives(bits, n)
    n_unique = sum(per_block)
    assert n_common == NC
    info = uniq.scan_unique_info()
    assert (info["n_unique"], info["n_common"], info["why"]) == (n_unique, NC, ""), info
    wps, nvb, nub = (n + 31) // 32, (NC + 63) // 64, (n_unique + 63) // 64
    # the per-block mask and prefix; the rows, whole blocks and one of slack; the weights, whole blocks and 64 bytes
    assert info["stream_bytes"] == 16 * (nvb + 1) + (nub + 1) * 256 * wps + 256 + 64 * nub + 64, info
    off = plain.scan_unique_info()
    assert off["n_unique"] == 0 and off["stream_bytes"] == 0 and off["why"].startswith("opted out"), off
    assert uniq.scan_index_info()["index_bytes"] == plain.scan_index_info()["index_bytes"] + info["stream_bytes"]
    assert dense.scan_unique_info()["why"] != "" and dense.scan_unique_info()["n_unique"] == 0
    assert uniq.scan_single_info() == plain.scan_single_info() and uniq.scan_split_info() == plain.scan_split_info()
    P, A, B = _masks(n, "P")

    def plans(wl, tb):
        a, b = uniq.plan(wl, P, A, B, tile_blocks=tb), plain.plan(wl, P, A, B, tile_blocks=tb)
        got = (a.n_tiles, a.bytes_streamed, b.n_tiles, b.bytes_streamed)
        a.destroy()
        b.destroy()
        return got

    for name, wl in LISTS.items():
        for tb in (0, 1, 2):
            ta, ba, tb_, bb = plans(wl, tb)
            assert ta == tb_ and ba <= bb, (n, name, tb, ta, tb_, ba, bb)
            if tb == 1:  # one block a tile: a block of the stream and its weights are never fewer bytes than the block of rows
                assert ba == bb, (n, name, tb, ba, bb)
            elif name in ("nested", "sliding"):
                # nested, 0: [128, 384) is blocks 2 .. 5, 140 representatives in three blocks of the stream against four of rows;
                # 2: its second half, blocks 4 and 5, is 12 representatives in one.  sliding: [0, 150) holds blocks 0 and 1
                assert ba < bb, (n, name, tb, ba, bb)
    # blocks 0 and 1 alone, no rare site counted apart: two representatives in one block of the stream against two blocks of rows
    ta, ba, tb_, bb = plans([_cw(0, 128)], 0)
    assert ta == tb_ == 1 and bb - ba == 2 * 256 * wps - (256 * wps + 64), (ba, bb)


def test_stream_is_independent_of_the_singleton_stream(ctx):
    """with IMPOP_KEEP_NO_SINGLE_STREAM the matrix keeps its distinct-row stream, and the records"""
    n = 465
    bits = _crafted(n, 9000 + n)
    both = ctx.upload_dense(bits, keep_hap_major=False)
    nosingle = ctx.upload_dense(bits, keep_hap_major=False, single_stream=False)
    assert nosingle.scan_unique_info() == both.scan_unique_info() and nosingle.scan_single_info()["n_single"] == 0
    P, A, B = _masks(n, "overlap")
    for tb in (0, 2):
        assert nosingle.scan(LISTS["nested"], P, A, B, tile_blocks=tb).tobytes() == both.scan(LISTS["nested"], P, A, B).tobytes()
    both.free()
    nosingle.free()


@pytest.mark.parametrize("n", (65, 465))
def test_gate_random_rows_keep_no_stream(ctx, n):
    """common rows that never repeat: no stream, a reason, the index of the matrix made without it, the same records"""
    bits = _crafted(n, 9100 + n, folding=False)
    per_block, n_common = _representatives(bits, n)
    assert sum(per_block) * 4 > n_common * 3
    bm = ctx.upload_dense(bits, keep_hap_major=False)
    twin = ctx.upload_dense(bits, keep_hap_major=False, unique_rows=False)
    info = bm.scan_unique_info()
    assert (info["n_unique"], info["n_common"], info["stream_bytes"]) == (0, 0, 0) and "above 3/4" in info["why"], info
    assert bm.scan_index_info() == twin.scan_index_info()
    P, A, B = _masks(n, "P")
    a, b = bm.plan(WINDOWS, P, A, B), twin.plan(WINDOWS, P, A, B)
    same = (a.n_tiles, a.bytes_streamed) == (b.n_tiles, b.bytes_streamed)
    a.destroy()
    b.destroy()
    assert same
    assert bm.scan(WINDOWS, P, A, B).tobytes() == twin.scan(WINDOWS, P, A, B).tobytes()
    bm.free()
    twin.free()


@pytest.mark.parametrize("kind", ("n64", "n600", "weighted", "nosplit"))
def test_routes_without_the_stream(ctx, kind):
    """no distinct-row stream, with a reason, and the records of the dense stream"""
    n = {"n64": 64, "n600": 600}.get(kind, 465)
    bits = _crafted(n, 9200 + n)
    bm = ctx.upload_dense(bits, keep_hap_major=False, rare_split=kind != "nosplit")
    dense = ctx.upload_dense(bits, keep_hap_major=False, dense_scan=True)
    if kind == "weighted":
        w = np.random.default_rng(3).integers(1, 50, S).astype(np.uint32)
        bm.set_site_weights(w)
        dense.set_site_weights(w)
    info = bm.scan_unique_info()
    assert (info["n_unique"], info["n_common"], info["stream_bytes"]) == (0, 0, 0) and info["why"] != "", (kind, info)
    P, A, B = _masks(n, "P")
    assert bm.scan(WINDOWS, P, A, B).tobytes() == dense.scan(WINDOWS, P, A, B).tobytes(), kind
    bm.free()
    dense.free()


def _hip_runtime():
    """the HIP runtime the library is bound to (the one copy in this process), for the stream-capture calls"""
    import ctypes as C
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(paths) == 1, paths
    return C.CDLL(paths.pop())


def test_graph_replay():
    """a plan on the unique-row route captured into a graph: the masks and the ranges of the stream are kernel arguments of
    the captured launch; the replay's records are a direct launch's"""
    import ctypes as C

    import impop_amd
    n = 465
    bits = _crafted(n, 9000 + n)
    P, A, B = _masks(n, "overlap")
    _, A2, B2 = _masks(n, "A1")
    probe = impop_amd.Context(0)  # loads the library, and with it the runtime
    hip = _hip_runtime()
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0  # hipStreamNonBlocking
    c = impop_amd.Context(0, stream=stream.value)
    bm = c.upload_dense(bits, keep_hap_major=False)
    assert bm.scan_unique_info()["n_unique"] > 0
    pl = bm.plan(LISTS["nested"], P, A, B, tile_blocks=2)  # tiles that read the stream
    pl.launch()
    direct1 = pl.fetch()
    pl.set_masks(P, A2, B2)  # a plan owns its Tajima constants: a capture holds the two kernels only, whatever P (test_gpu_scan_shared_context.py)
    pl.launch()
    direct2 = pl.fetch()
    assert direct1.tobytes() != direct2.tobytes()
    pl.set_masks(P, A, B)
    pl.launch()
    assert pl.fetch().tobytes() == direct1.tobytes()
    pl.set_masks(P, A2, B2)
    c.synchronize()
    assert hip.hipStreamBeginCapture(stream, 0) == 0  # hipStreamCaptureModeGlobal
    pl.launch()
    assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0
    assert hip.hipGraphInstantiate(C.byref(gexec), graph, None, None, C.c_size_t(0)) == 0
    assert pl.fetch().tobytes() == direct1.tobytes()  # captured, not run
    for _ in range(2):
        assert hip.hipGraphLaunch(gexec, stream) == 0
    assert pl.fetch().tobytes() == direct2.tobytes()
    assert hip.hipGraphExecDestroy(gexec) == 0 and hip.hipGraphDestroy(graph) == 0
    pl.destroy()
    bm.free()
    c.close()
    probe.close()
    assert hip.hipStreamDestroy(stream) == 0


_SCAN = re.compile(r"\[impop_scan\] (.*)$")


def _trace_child():
    import impop_amd
    ctx = impop_amd.Context(0)
    n = 465
    bits = _crafted(n, 9000 + n)
    P, A, B = _masks(n, "P")
    dense = ctx.upload_dense(bits, keep_hap_major=False, dense_scan=True)
    want = dense.scan(WINDOWS, P, A, B).tobytes()
    for tag, kw in (("uniq", {}), ("plain", dict(unique_rows=False))):
        bm = ctx.upload_dense(bits, keep_hap_major=False, **kw)
        sys.stderr.write("@@call other\n")  # the scan below traces too: not a line of the calls under test
        sys.stderr.flush()
        info = bm.scan_unique_info()
        sys.stderr.write(f"@@info {tag} {info['n_unique']} {info['why'].replace(' ', '_') or '-'}\n")
        sys.stderr.write(f"@@same {tag} {int(bm.scan(WINDOWS, P, A, B).tobytes() == want)}\n")
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        pl = bm.plan([(0, S, S)], P, A, B)  # the whole matrix: one tile
        sys.stderr.write(f"@@plan {tag} {pl.n_tiles} {pl.bytes_streamed}\n")
        sys.stderr.write(f"@@call multi_{tag}\n")
        sys.stderr.flush()
        bm.scan_multi([(0, S, S)], [(np.arange(n) % 2) == k for k in range(2)])
        pl.destroy()
        bm.free()
    dense.free()
    ctx.close()


def _run_child(env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--trace-child"], capture_output=True, text=True, cwd=ROOT,
                       env=dict(os.environ, IMPOP_TRACE="1", **env), timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    traces, plans, infos, same, cur = {}, {}, {}, {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@@call "):
            cur = line[7:]
        elif line.startswith("@@plan "):
            _, tag, tiles, nbytes = line.split()
            plans[tag] = (int(tiles), int(nbytes))
        elif line.startswith("@@info "):
            _, tag, n_unique, why = line.split()
            infos[tag] = (int(n_unique), why)
        elif line.startswith("@@same "):
            same[line.split()[1]] = line.split()[2]
        else:
            mt = _SCAN.search(line)
            if mt and cur is not None:
                head = mt.group(1).partition(" why=")[0]
                traces.setdefault(cur, []).append({k: v for k, v in (kv.split("=", 1) for kv in head.split())})
    return traces, plans, infos, same


def test_trace_fields():
    traces, plans, infos, same = _run_child({})
    n = 465
    per_block, _ = _representatives(_crafted(n, 9000 + n), n)
    n_unique = sum(per_block)
    assert infos["uniq"] == (n_unique, "-") and infos["plain"][0] == 0 and same == {"uniq": "1", "plain": "1"}
    uniq, plain = traces["uniq"][0], traces["plain"][0]
    assert int(uniq["unique_rows"]) == n_unique and int(plain["unique_rows"]) == 0
    assert int(uniq["tiles"]) == int(plain["tiles"]) == plans["uniq"][0] == plans["plain"][0] == 1
    assert int(uniq["bytes_streamed"]) == plans["uniq"][1] < plans["plain"][1] == int(plain["bytes_streamed"])
    assert int(uniq["rare_streamed"]) == int(plain["rare_streamed"]) and int(uniq["rows_streamed"]) < int(plain["rows_streamed"])
    for t in (uniq, plain):
        assert int(t["bytes_streamed"]) == int(t["rows_streamed"]) + int(t["rare_streamed"]), t
    # 13 blocks of rows; or the representatives of the 12 whole blocks, from the start of the stream, and the final 13 rows as a tail
    wps, ub = 15, (sum(per_block[:12]) + 63) // 64
    assert int(plain["rows_streamed"]) == 13 * 256 * wps and int(uniq["rows_streamed"]) == (1 + ub) * 256 * wps + 64 * ub
    for tag in ("multi_uniq", "multi_plain"):  # impop_scan_multi reads the rows
        for t in traces[tag]:
            assert int(t["unique_rows"]) == 0 and int(t["rows_streamed"]) == int(plain["rows_streamed"]), t


def test_environment_opt_out():
    """IMPOP_NO_UNIQUE_ROWS=1, read in native code: no matrix of the process keeps the stream; the records stay"""
    traces, plans, infos, same = _run_child({"IMPOP_NO_UNIQUE_ROWS": "1"})
    assert infos["uniq"][0] == 0 and infos["uniq"][1].startswith("opted_out_(IMPOP_NO_UNIQUE_ROWS"), infos
    assert same == {"uniq": "1", "plain": "1"} and plans["uniq"] == plans["plain"]
    assert int(traces["uniq"][0]["unique_rows"]) == 0


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--trace-child":
        sys.path.insert(0, ROOT)
        _trace_child()
