"""The tile digest of a scan plan (csrc/tile_digest.h; scan_tiles_kernel_digest and digest_build_kernel in scan.hip; run with -m gpu
on an MI355X).  A plan on the one-wave body works out once, per tile, the distinct common rows under complement with a uint16 weight
each and, per haplotype, how many of the tile's singleton sites it carries; launches read that in place of rows and singleton
stream.  IMPOP_SCAN_WAVE_TILES=1 IMPOP_SCAN_DIGEST=1 reach it on small plans, IMPOP_SCAN_DIGEST=0 forbids it.  Records must be,
byte for byte, those of the same plan without a digest and of the dense matrix: after set_masks, and from a captured graph, too.

Two matrices.  The crafted one of test_gpu_scan_joint_issue with its eleven window lists and mask configurations, at n = 65, 465,
512 (WPS 3 / 15 / 16: a last granule of 3 / 3 / 4 dwords) and n = 150 (WPS 5: a last granule of 1 dword), tile_blocks 0, 1, 2.
And one of its own at n = 150 (not a multiple of 32: the complement is taken within the real haplotypes), whose regions are
  G   singleton sites side by side from site 0 (site s is singleton s of the stream): 3000 on haplotype n - 1 in alternating
      polarity, 400 on haplotype 0, 400 on haplotype 7 (in no population of MASKS), 20 on random carriers (a range of six words is
      shorter than a histogram of 320 bytes: the tile keeps its range), 600 on random carriers
  M   120 sites of minor count 2 or 3
  R   common rows, row j at site R0 + 4 j + 1, a window edge "at row j" at site R0 + 4 j.  Groups of rows in which every pattern
      occurs twice, the second time complemented: 1 pattern 300 times (weight above 255), 1 pattern 10 times, and 63, 64, 65, 128,
      129 patterns; a run of one pattern 640 times keeps the matrix's distinct-row stream worth having.
A window over a group is one tile (asserted) whose representatives number the group's patterns; digest_info is checked against
that count, the histogram rule and the layout's arithmetic, bytes_streamed against what a launch reads."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import test_gpu_scan_joint_issue as J

pytestmark = pytest.mark.gpu

WAVE, DIGEST = "IMPOP_SCAN_WAVE_TILES", "IMPOP_SCAN_DIGEST"
DIGEST_ROWS_MAX = 512  # tile_digest.h


class _env:
    """the overrides are read where a plan is made"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _on():
    return _env(**{WAVE: "1", DIGEST: "1"})


def _off():
    return _env(**{WAVE: "1", DIGEST: "0"})


def _plan_records(mat, env, wl, P, A, B, tb=0):
    """plan() + launch() + fetch() -> (records, digest_info, n_tiles, bytes_streamed)"""
    with env:
        pl = mat.plan(wl, P, A, B, tile_blocks=tb)
    try:
        pl.launch()
        return pl.fetch(), pl.digest_info(), pl.n_tiles, pl.bytes_streamed
    finally:
        pl.destroy()


def _hip_runtime():
    """the HIP runtime the library is bound to (the one copy in this process), for the stream-capture calls"""
    import ctypes as C
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(paths) == 1, paths
    return C.CDLL(paths.pop())


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    assert c.device_name().startswith("gfx950")
    yield c
    c.close()


# ---- the crafted matrix of test_gpu_scan_joint_issue ----
@pytest.fixture(scope="module", params=(65, 150, 465, 512))
def mats(ctx, request):
    n = request.param
    bits = J._crafted(n, 2700 + n)
    uniq = ctx.upload_dense(bits, keep_hap_major=False)
    dense = ctx.upload_dense(bits, keep_hap_major=False, dense_scan=True)
    assert uniq.scan_unique_info()["n_unique"] > 0 and uniq.scan_single_info()["n_single"] > 0
    want = {(cfg, i): dense.scan(wl, *J._masks(n, cfg)) for cfg in J.CFGS for i, wl in enumerate(J.LISTS)}  # once, shared, unchanged
    yield n, uniq, want
    uniq.free()
    dense.free()


@pytest.mark.parametrize("cfg", J.CFGS)
def test_digest_records_equal_plain_and_dense(mats, cfg):
    n, uniq, want = mats
    P, A, B = J._masks(n, cfg)
    taken = 0
    for i, wl in enumerate(J.LISTS):
        ref = want[(cfg, i)].tobytes()
        for tb in (0, 1, 2):
            got, info, tiles, _ = _plan_records(uniq, _on(), wl, P, A, B, tb)
            assert got.tobytes() == ref, (n, cfg, i, tb, "digest", info)
            assert info["on"] == (info["why"] == ""), info
            taken += info["on"]
            got0, info0, tiles0, _ = _plan_records(uniq, _off(), wl, P, A, B, tb)
            assert got0.tobytes() == ref, (n, cfg, i, tb, "no digest")
            assert not info0["on"] and info0["why"] == "IMPOP_SCAN_DIGEST=0" and info0["digest_bytes"] == 0 and tiles0 == tiles, info0
    # at tile_blocks 1 and 2 every tile of the eleven crafted lists is under the caps (a tile of the default tiling may hold 21
    # blocks of distinct rows, and the last list the whole matrix as one window)
    assert taken >= 2 * 11, (n, cfg, taken)


def test_set_masks_between_launches(mats):
    """the masks are kernel arguments and the digest holds nothing of them"""
    n, uniq, want = mats
    P, A, B = J._masks(n, "P")
    P2, A2, B2 = J._masks(n, "overlap")
    for i in (0, 5):
        for tb in (1, 2):
            with _on():
                pl = uniq.plan(J.LISTS[i], P, A, B, tile_blocks=tb)
            try:
                assert pl.digest_info()["on"]
                pl.launch()
                r1 = pl.fetch()
                pl.set_masks(P2, A2, B2)
                pl.launch()
                r2 = pl.fetch()
                pl.set_masks(None, A, B)
                pl.launch()
                r3 = pl.fetch()
            finally:
                pl.destroy()
            assert r1.tobytes() == want[("P", i)].tobytes(), (n, i, tb)
            assert r2.tobytes() == want[("overlap", i)].tobytes(), (n, i, tb)
            assert r3.tobytes() == want[("noP", i)].tobytes(), (n, i, tb)


def test_graph_replay():
    """a digest plan captured into a graph: nothing but the two kernels, the masks arguments of the captured launch"""
    import ctypes as C

    import impop_amd
    n = 465
    bits = J._crafted(n, 2700 + n)
    P, A, B = J._masks(n, "overlap")
    _, A2, B2 = J._masks(n, "P")
    wl = J.LISTS[3]
    probe = impop_amd.Context(0)  # loads the library, and with it the runtime
    hip = _hip_runtime()
    stream, graph, gexec = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0  # hipStreamNonBlocking
    c = impop_amd.Context(0, stream=stream.value)
    bm = c.upload_dense(bits, keep_hap_major=False)
    dense = c.upload_dense(bits, keep_hap_major=False, dense_scan=True)
    want1, want2 = dense.scan(wl, P, A, B), dense.scan(wl, P, A2, B2)
    assert want1.tobytes() != want2.tobytes()
    with _on():
        pl = bm.plan(wl, P, A, B, tile_blocks=2)
    assert pl.digest_info()["on"]
    pl.launch()
    assert pl.fetch().tobytes() == want1.tobytes()
    pl.set_masks(P, A2, B2)  # a plan owns its Tajima constants: a capture holds the two kernels only, whatever P (test_gpu_scan_shared_context.py)
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


# ---- a matrix of its own ----
N2, WPS2 = 150, 5
SEGS = (("last", 3000), ("zero", 400), ("nopop", 400), ("few", 20), ("mix", 600))  # G, in this order from site 0
NM2 = 120
GROUPS = ((1, 300), (1, 10), (63, 126), (64, 128), (65, 130), (128, 256), (129, 258), (1, 640))  # (patterns, rows)
NG2 = sum(c for _, c in SEGS)
M02 = NG2
R02 = NG2 + NM2 + 20
NR2 = sum(r for _, r in GROUPS)
S2 = 4 * (NG2 + NM2 + NR2) + 2000
NOPOP = 7


def _seg(name):
    s = 0
    for k, c in SEGS:
        if k == name:
            return s, s + c
        s += c
    raise KeyError(name)


def _group(i):
    a = sum(r for _, r in GROUPS[:i])
    return a, a + GROUPS[i][1]


def _rows2(a, b):
    return (R02 + 4 * a, R02 + 4 * b, b - a)


def _own():
    """-> (bits [n, S2], rows [NR2, n]: the common rows in order)"""
    rng = np.random.default_rng(2027)
    n = N2
    m = np.zeros((n, S2), np.uint8)

    def single(site, h, flip):
        col = np.zeros(n, np.uint8)
        col[h] = 1
        m[:, site] = col ^ flip

    s = 0
    for name, c in SEGS:
        for q in range(c):
            h = {"last": n - 1, "zero": 0, "nopop": NOPOP}.get(name)
            single(s, int(rng.integers(0, n)) if h is None else h, q & 1)
            s += 1
    for q in range(NM2):
        col = np.zeros(n, np.uint8)
        col[rng.choice(n, int(rng.integers(2, 4)), replace=False)] = 1
        m[:, M02 + q] = col ^ (q & 1)
    rows = np.zeros((NR2, n), np.uint8)
    j = 0
    seen = set()
    for pats, count in GROUPS:
        pool = []
        while len(pool) < pats:
            r = np.zeros(n, np.uint8)
            r[rng.choice(n, int(rng.integers(4, n - 3)), replace=False)] = 1
            key = (r ^ r[0]).tobytes()
            if key not in seen:  # distinct under complement over the whole matrix
                seen.add(key)
                pool.append(r)
        for q in range(count):
            x = pool[q % pats]
            rows[j] = (1 - x) if (q // pats) & 1 else x
            m[:, R02 + 4 * j + 1] = rows[j]
            j += 1
    c = m.sum(axis=0, dtype=np.int64)
    assert int(((c > 0) & (c < n)).sum()) * 4 < S2 and int((np.minimum(c, n - c) > 3).sum()) == NR2
    return m, rows


def _distinct(rows, a, b):
    sub = rows[a:b]
    return len(np.unique(sub ^ sub[:, :1], axis=0)) if b > a else 0


def _single_words(a, b):
    return (b + 3) // 4 - a // 4 if b > a else 0


# one-tile windows (asserted): the order puts every kind among the first nine
POOL2 = [
    _seg("last"),                       # 0 representatives; every singleton on haplotype n - 1
    _rows2(*_group(0)),                 # one pattern 300 times
    _seg("few"),                        # keeps its range ...
    _seg("mix"),                        # ... next to a histogram
    _rows2(*_group(2)),                 # 63
    _rows2(*_group(3)),                 # 64
    _rows2(*_group(4)),                 # 65
    _rows2(*_group(5)),                 # 128
    _rows2(*_group(6)),                 # 129
    _seg("zero"),
    _seg("nopop"),
    (M02, M02 + NM2),                   # entries only
    _rows2(*_group(1)),                 # one pattern ten times
]
POOL2 = [(w[0], w[1], w[1] - w[0]) for w in POOL2]
COUNTS2 = {k: POOL2[:k] for k in (1, 2, 3, 4, 5, 9, len(POOL2))}
OVER2 = [(0, 3500, 3500), (2900, 3810, 910), (3790, 4500, 710), _rows2(5, 700), _rows2(250, 900), _rows2(600, 1300),
         (M02 - 30, R02 + 4 * 50, 1), (0, S2, S2)]


def _masks2(cfg):
    n = N2
    P = np.ones(n, np.uint8); P[[NOPOP, 20, 21]] = 0
    A = np.zeros(n, np.uint8); A[10:60] = 1
    B = np.zeros(n, np.uint8); B[80:] = 1
    if cfg == "overlap":
        A[10:100] = 1
        B[60:] = 1
    return (None if cfg == "noP" else P), A, B


@pytest.fixture(scope="module")
def own(ctx):
    bits, rows = _own()
    uniq = ctx.upload_dense(bits, keep_hap_major=False)
    dense = ctx.upload_dense(bits, keep_hap_major=False, dense_scan=True)
    assert uniq.scan_unique_info()["n_unique"] > 0 and uniq.scan_single_info()["n_single"] == NG2
    lists = list(COUNTS2.values()) + [OVER2]
    want = {(cfg, i): dense.scan(wl, *_masks2(cfg)) for cfg in J.CFGS for i, wl in enumerate(lists)}
    yield uniq, rows, lists, want
    uniq.free()
    dense.free()


@pytest.mark.parametrize("cfg", J.CFGS)
def test_own_matrix_records(own, cfg):
    uniq, rows, lists, want = own
    P, A, B = _masks2(cfg)
    for i, wl in enumerate(lists):
        ref = want[(cfg, i)].tobytes()
        got, info, tiles, _ = _plan_records(uniq, _on(), wl, P, A, B)
        assert info["on"], (i, info)
        assert got.tobytes() == ref, (cfg, i, "digest")
        got0, info0, _, _ = _plan_records(uniq, _off(), wl, P, A, B)
        assert got0.tobytes() == ref and not info0["on"], (cfg, i, "no digest")
    # overlapping windows without the one above the caps: tiles are elementary segments
    wl = OVER2[:-1]
    got, info, tiles, _ = _plan_records(uniq, _on(), wl, P, A, B)
    assert info["on"] and tiles > len(wl), (info, tiles)
    assert got.tobytes() == want[(cfg, len(lists) - 1)][:-1].tobytes()


def test_digest_info_is_the_model(own):
    """representatives per tile add up to the distinct rows under complement of every window; a tile has a histogram unless its
    range of the singleton stream is fewer bytes than 64 wps; the digest's bytes are the layout's, bytes_streamed what a launch reads"""
    uniq, rows, lists, want = own
    P, A, B = _masks2("P")
    for k, wl in COUNTS2.items():
        _, info, tiles, streamed = _plan_records(uniq, _on(), wl, P, A, B)
        assert tiles == k and info["on"], (k, tiles, info)
        reps, padded, hists, kept, entries = 0, 0, 0, 0, 0
        for (a, b, _) in wl:
            if a >= R02:
                d = _distinct(rows, (a - R02) // 4, (b - R02) // 4)
                reps += d
                padded += (d + 3) // 4 * 4
            elif a >= M02:
                entries += b - a
            else:
                words = _single_words(a, b)
                if words * 8 >= 64 * WPS2:
                    hists += 1
                else:
                    kept += words * 8
        model = {"on": True, "n_rows": reps, "n_hist_tiles": hists, "digest_bytes": padded * (4 * WPS2 + 2) + hists * 64 * WPS2, "why": ""}
        assert info == model, (k, info, model)
        assert streamed == model["digest_bytes"] + kept + 8 * entries, (k, streamed, model, kept, entries)
    pats = {i: _distinct(rows, *_group(i)) for i in range(len(GROUPS))}
    assert [pats[i] for i in range(len(GROUPS))] == [p for p, _ in GROUPS]  # the model counts what the matrix was made of


# ---- the trace line, the rule and the cap, in a child process (IMPOP_TRACE is read once per process) ----
_SCAN = re.compile(r"\[impop_scan\] (.*)$")
U0 = 64 * J.NF  # the first of the crafted matrix's 1600 distinct rows


def _child():
    import impop_amd
    ctx = impop_amd.Context(0)

    def mark(tag):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()

    n = 465
    bits = J._crafted(n, 2700 + n)
    uniq = ctx.upload_dense(bits, keep_hap_major=False)
    dense = ctx.upload_dense(bits, keep_hap_major=False, dense_scan=True)
    P, A, B = J._masks(n, "P")
    wl = J.LISTS[3]
    mark("other")
    want = dense.scan(wl, P, A, B).tobytes()

    def plan(tag, wl, tb=2, **env):
        mark(tag)
        with _env(**env):
            pl = uniq.plan(wl, P, A, B, tile_blocks=tb)
        info = pl.digest_info()
        sys.stderr.write(f"@@plan {tag} {pl.n_tiles} {pl.bytes_streamed} {int(info['on'])} {info['digest_bytes']}\n")
        pl.launch()
        got = pl.fetch().tobytes()
        pl.destroy()
        mark("other")
        return got

    same = plan("both", wl, **{WAVE: "1", DIGEST: "1"}) == want
    same = plan("forbidden", wl, **{WAVE: "1", DIGEST: "0"}) == want and same
    same = plan("rule", wl, **{WAVE: "1", DIGEST: None}) == want and same      # the default rule on a plan its maker keeps
    same = plan("four_waves", wl, **{WAVE: "0", DIGEST: "1"}) == want and same  # not the one-wave body
    mark("one_shot")
    with _env(**{WAVE: "1", DIGEST: None}):
        same = uniq.scan(wl, P, A, B, tile_blocks=2).tobytes() == want and same
    mark("one_shot_forced")
    with _env(**{WAVE: "1", DIGEST: "1"}):
        same = uniq.scan(wl, P, A, B, tile_blocks=2).tobytes() == want and same
    mark("other")
    sys.stderr.write(f"@@same lists {int(same)}\n")
    for tag, count in (("at_cap", DIGEST_ROWS_MAX), ("above_cap", DIGEST_ROWS_MAX + 1)):
        cap = [J._rows(U0, U0 + count)]
        ref = dense.scan(cap, P, A, B).tobytes()
        got = plan(tag, cap, 0, **{WAVE: "1", DIGEST: "1"})  # the default tiling: one tile
        sys.stderr.write(f"@@same {tag} {int(got == ref)}\n")
    uniq.free()
    dense.free()
    ctx.close()


@pytest.fixture(scope="module")
def child():
    env = dict(os.environ, IMPOP_TRACE="1")
    env.pop(WAVE, None)
    env.pop(DIGEST, None)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    traces, plans, same, cur = {}, {}, {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@@call "):
            cur = line[7:]
        elif line.startswith("@@plan "):
            f = line.split()
            plans[f[1]] = [int(x) for x in f[2:]]
        elif line.startswith("@@same "):
            same[line.split()[1]] = line.split()[2]
        else:
            mt = _SCAN.search(line)
            if mt and cur is not None:
                head = mt.group(1).partition(" why=")[0]
                traces.setdefault(cur, []).append(dict(kv.split("=", 1) for kv in head.split()))
    return traces, plans, same


def test_trace_reports_the_digest(child):
    """digest=1 under the two overrides and by the rule on a kept plan; digest=0 where it is forbidden, on four waves and for the
    one-shot scan; one line per plan, whose byte counts add up and are the plan's own"""
    traces, plans, same = child
    assert same["lists"] == "1"
    for tag, flag in (("both", "1"), ("forbidden", "0"), ("four_waves", "0"), ("one_shot", "0"), ("one_shot_forced", "1"), ("at_cap", "1"),
                      ("above_cap", "0")):
        got = traces[tag]
        assert len(got) == 1, (tag, got)
        t = got[0]
        assert t["digest"] == flag, (tag, t)
        assert list(t)[-2:] == ["wave_tiles", "digest"], t
        assert int(t["bytes_streamed"]) == int(t["rows_streamed"]) + int(t["rare_streamed"]), t
        if tag in plans:
            tiles, streamed, on, dbytes = plans[tag]
            assert (tiles, streamed, on) == (int(t["tiles"]), int(t["bytes_streamed"]), int(flag)), (tag, plans[tag], t)
            assert (dbytes > 0) == (flag == "1")
    assert traces["four_waves"][0]["wave_tiles"] == "0" and traces["both"][0]["wave_tiles"] == "1"
    # the rule: a kept plan on the one-wave body takes the digest exactly where a launch then reads no more than without
    t, plain = traces["rule"][0], traces["forbidden"][0]
    assert len(traces["rule"]) == 1 and t["digest"] == str(int(int(traces["both"][0]["bytes_streamed"]) <= int(plain["bytes_streamed"]))), (t, plain)
    assert int(t["bytes_streamed"]) <= int(plain["bytes_streamed"])
    assert traces["both"][0]["tiles"] == plain["tiles"]


def test_tile_above_the_cap(child):
    """512 candidate rows are a digest tile, 513 are not under both overrides; the records are right either way"""
    traces, plans, same = child
    assert same["at_cap"] == "1" and same["above_cap"] == "1"
    assert plans["at_cap"][0] == 1 and plans["above_cap"][0] == 1  # one tile each
    assert traces["above_cap"][0]["wave_tiles"] == "1"


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--child":
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        _child()
