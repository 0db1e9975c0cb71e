"""GPU: impop_dstat_scan against the plain restatement of tests/plain_dstat.py — every integer and all three doubles, bit for bit,
NaN matching NaN.  What needs the trace line (IMPOP_TRACE=1 is read once per process) runs in one child process per module."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import dstat_cases as dc
import plain_dstat as pd
from conftest import ROOT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


def flags(members, n):
    f = np.zeros(n, dtype=np.uint8)
    f[list(members)] = 1
    return f


def masks(pops, n):
    return [flags(p, n) for p in pops]


# ---- the known answer of the header -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("polarize", (False, True))
def test_known_answer(ctx, polarize):
    bm = ctx.upload_dense(dc.known_matrix(), keep_hap_major=False)
    rec = bm.dstat_scan([(0, 6)], masks(dc.KNOWN_POPS, 8), dc.KNOWN_QUARTETS, polarize=polarize)
    assert rec.shape == (1, 2)
    for qi, q in enumerate(dc.KNOWN_QUARTETS):
        r = rec[0, qi]
        got = tuple(int(r[f]) for f in ("abba", "baba", "f4_num", "fd_den_p2", "fd_den_p3", "n_informative", "n_skipped"))
        assert got == dc.KNOWN_INTS[q] and int(r["n_sites"]) == 6 and int(r["flags"]) == 0
        assert (float(r["d"]), float(r["f4"]), float(r["fd"])) == dc.KNOWN_DOUBLES[q]
    pd.assert_matches(rec, pd.reference(dc.known_matrix(), dc.KNOWN_POPS, dc.KNOWN_QUARTETS, [(0, 6)], polarize), "known")
    bm.free()


# ---- geometry: tails of 1..4 dwords, more than one full granule, 64-bit products at 465; default tiles and tiles of 1, 2, 5 blocks ------

@pytest.mark.parametrize("n", dc.GEOMETRY_N)
def test_shapes_against_the_restatement(ctx, n, monkeypatch):
    m01, pops = dc.geometry_case(n)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    for polarize in (False, True):
        want = pd.reference(m01, pops, dc.GEOMETRY_QUARTETS, dc.GEOMETRY_WINDOWS, polarize)
        dc.assert_not_hollow(want)
        for tile_blocks in (None, 1, 2, 5):
            if tile_blocks is None:
                monkeypatch.delenv("IMPOP_DSTAT_TILE_BLOCKS", raising=False)
            else:
                monkeypatch.setenv("IMPOP_DSTAT_TILE_BLOCKS", str(tile_blocks))
            got = bm.dstat_scan(dc.GEOMETRY_WINDOWS, masks(pops, n), dc.GEOMETRY_QUARTETS, polarize=polarize)
            pd.assert_matches(got, want, (n, polarize, tile_blocks))
    bm.free()


# ---- weights: the records of the bp-expanded matrix, the counters those of the columns ----------------------------------------------

def test_weights_are_the_expanded_matrix(ctx):
    n, S = 33, 300
    rng = np.random.default_rng(33300)
    m01 = dc.draw_sites(rng, n, S)
    pops = dc.cut_pops(rng, n)
    w = rng.integers(1, 10, S).astype(np.uint32)
    w[137] = 70000
    wins = [(0, S), (5, 137), (130, 140), (137, 138), (138, 300)]
    start = np.concatenate([[0], np.cumsum(w.astype(np.int64))])
    wins_x = [(int(start[b]), int(start[e])) for b, e in wins]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    bm.set_site_weights(w)
    bx = ctx.upload_dense(np.repeat(m01, w, axis=1), keep_hap_major=False)
    for polarize in (False, True):
        want = pd.reference(m01, pops, dc.GEOMETRY_QUARTETS, wins, polarize, weights=w)
        dc.assert_not_hollow(want)
        got = bm.dstat_scan(wins, masks(pops, n), dc.GEOMETRY_QUARTETS, polarize=polarize)
        pd.assert_matches(got, want, ("weighted", polarize))  # n_informative and n_skipped count columns
        exp = bx.dstat_scan(wins_x, masks(pops, n), dc.GEOMETRY_QUARTETS, polarize=polarize)
        pd.assert_matches(got, exp, ("expanded", polarize), skip=("n_informative", "n_skipped"))
        assert (exp["n_informative"] >= got["n_informative"]).all()
    bx.free()
    bm.free()


# ---- overlap and order --------------------------------------------------------------------------------------------------------------

def test_permuting_the_windows_permutes_the_records(ctx, monkeypatch):
    n = 70
    m01, pops = dc.geometry_case(n)
    wins = [(0, 2100), (10, 300), (250, 900), (250, 900), (299, 300), (64, 128), (1000, 2099), (63, 1985), (1999, 2100), (640, 641)]
    want = pd.reference(m01, pops, dc.GEOMETRY_QUARTETS, wins, True)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    monkeypatch.setenv("IMPOP_DSTAT_TILE_BLOCKS", "3")
    got = bm.dstat_scan(wins, masks(pops, n), dc.GEOMETRY_QUARTETS, polarize=True)
    pd.assert_matches(got, want, "overlap")
    assert got[2].tobytes() == got[3].tobytes()
    perm = np.random.default_rng(5).permutation(len(wins))
    shuffled = bm.dstat_scan([wins[i] for i in perm], masks(pops, n), dc.GEOMETRY_QUARTETS, polarize=True)
    assert shuffled.tobytes() == got[perm].tobytes()
    bm.free()


# ---- routes, quartet groups and the trace line, in a child process under IMPOP_TRACE=1 ----------------------------------------------

ROUTE_N = (70, 465)
ROUTES = ("default", "norare", "dense", "compact")


def _route_case(n):
    m01, wins = dc.crafted(n)
    pops = dc.cut_pops(np.random.default_rng(77 + n), n)
    return m01, wins, pops


def _group_case():
    n = 130
    m01, _ = dc.geometry_case(n)
    pops, quartets = dc.six_pops(np.random.default_rng(606), n)
    return m01, pops, quartets, [(0, 2100), (100, 163), (700, 1400)]


def _child(out_path):
    import impop_amd
    from impop_amd import ImpopError
    ctx = impop_amd.Context(0)
    out = {}

    def call(tag, fn):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        out[tag] = fn()
        sys.stderr.flush()

    for n in ROUTE_N:
        m01, wins, pops = _route_case(n)
        mk = masks(pops, n)
        for tag, ukw in (("default", {}), ("norare", {"rare_split": False}), ("dense", {"dense_scan": True})):
            bm = ctx.upload_dense(m01, keep_hap_major=False, **ukw)
            for pol in (0, 1):
                call(f"{tag}/{n}/{pol}", lambda: bm.dstat_scan(wins, mk, dc.GEOMETRY_QUARTETS, polarize=bool(pol)))
            if tag == "default":  # tiles of one block: the rows and the rare entries of a window in many tiles
                call(f"default_t1/{n}", lambda: bm.dstat_scan(wins, mk, dc.GEOMETRY_QUARTETS, polarize=True, tile_blocks=1))
                cm = bm.compact()
                for pol in (0, 1):
                    call(f"compact/{n}/{pol}", lambda: cm.dstat_scan(wins, mk, dc.GEOMETRY_QUARTETS, polarize=bool(pol)))
                cm.free()
            bm.free()
    m01, pops, quartets, wins = _group_case()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    call("group15", lambda: bm.dstat_scan(wins, masks(pops, 130), quartets, polarize=True))
    call("group1", lambda: bm.dstat_scan(wins, masks(pops, 130), quartets[:1], polarize=True))
    bm.free()
    # the overflow bound depends on sizes and weights alone: refused before any launch
    n = 4096
    bm = ctx.upload_dense(np.ones((n, 1), np.uint8), keep_hap_major=False)
    bm.set_site_weights(np.array([2 ** 31], dtype=np.uint32))
    sys.stderr.write("@@call overflow\n")
    sys.stderr.flush()
    try:
        bm.dstat_scan([(0, 1)], masks([range(k * 1024, (k + 1) * 1024) for k in range(4)], n), [(0, 1, 2, 3)])
        out["overflow"] = np.array([0])
    except ImpopError as exc:
        out["overflow"] = np.array([exc.code])
        out["overflow_msg"] = np.array([str(exc)])
    bm.free()
    ctx.close()
    np.savez(out_path, **out)


_TRACE = re.compile(r"\[impop_dstat_scan\] (.*)$")


@pytest.fixture(scope="module")
def child():
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
        env.pop("IMPOP_DSTAT_TILE_BLOCKS", None)
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_dstat_scan as t; t._child(sys.argv[1])", path],
                           capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        z = np.load(path)
        recs = {k: z[k] for k in z.files}
    trace, other, cur = {}, {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@@call "):
            cur = line.split()[1]
            trace[cur], other[cur] = [], []
            continue
        mt = _TRACE.search(line)
        if mt and cur:
            kv = dict(x.split("=") for x in mt.group(1).split())
            trace[cur].append({k: (v if k == "route" else int(v)) for k, v in kv.items()})
        elif cur and line.startswith("[impop"):
            other[cur].append(line)
    return recs, trace, other


@pytest.mark.parametrize("n", ROUTE_N)
def test_routes_give_identical_bytes(child, n):
    recs, trace, _ = child
    m01, wins, pops = _route_case(n)
    for pol in (0, 1):
        want = pd.reference(m01, pops, dc.GEOMETRY_QUARTETS, wins, bool(pol))
        dc.assert_not_hollow(want)
        pd.assert_matches(recs[f"default/{n}/{pol}"], want, ("default", n, pol))
        for tag in ROUTES[1:]:
            assert recs[f"{tag}/{n}/{pol}"].tobytes() == recs[f"default/{n}/{pol}"].tobytes(), (tag, n, pol)
    assert recs[f"default_t1/{n}"].tobytes() == recs[f"default/{n}/1"].tobytes()
    assert trace[f"default_t1/{n}"][0]["tiles"] > trace[f"default/{n}/1"][0]["tiles"]
    lines = [trace[f"{t}/{n}/0"] for t in ROUTES]
    assert all(len(x) == 1 for x in lines)
    assert [x[0]["route"] for x in lines] == ["indexed+rare", "indexed", "dense", "compact"]
    for x in lines:
        assert x[0]["windows"] == len(wins) and x[0]["quartets"] == 3 and x[0]["launches"] == 2 and x[0]["tiles"] >= 1
    split, plain, dense, compact = (x[0]["bytes_streamed"] for x in lines)
    assert split < dense and plain < dense and compact < dense


def test_quartet_groups(child):
    from impop_amd import _lib
    recs, trace, _ = child
    m01, pops, quartets, wins = _group_case()
    assert len(quartets) == 15 and len(set(quartets)) == 14  # one quartet is listed twice
    assert any(len(set(a) & set(b)) == 3 for a in quartets for b in quartets)  # two quartets share three populations
    want = pd.reference(m01, pops, quartets, wins, True)
    dc.assert_not_hollow(want)
    pd.assert_matches(recs["group15"], want, "group15")
    twice = [i for i, q in enumerate(quartets) if q == quartets[0]]
    assert recs["group15"][:, twice[0]].tobytes() == recs["group15"][:, twice[1]].tobytes()
    assert recs["group1"].tobytes() == np.ascontiguousarray(recs["group15"][:, :1]).tobytes()
    one, all15 = trace["group1"][0], trace["group15"][0]
    n_groups = -(-15 // _lib.DSTAT_GROUP)
    assert n_groups > 1 and one["launches"] == 2 and all15["launches"] == n_groups * one["launches"]
    assert all15["quartets"] == 15 and all15["tiles"] == one["tiles"] and all15["bytes_streamed"] == one["bytes_streamed"]


def test_overflow_bound_refuses_before_any_launch(child):
    recs, trace, other = child
    assert recs["overflow"].tolist() == [E_UNSUPPORTED]
    msg = str(recs["overflow_msg"][0])
    assert "quartet 0" in msg and "window 0" in msg and "2^62" in msg
    assert trace["overflow"] == [] and other["overflow"] == []  # neither the route nor the scan was reached


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals(ctx):
    import impop_amd
    from impop_amd import ImpopError, _lib
    n = 33
    m01, pops = dc.geometry_case(n)
    S = m01.shape[1]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    mk = masks(pops, n)
    extra = flags(pops[0][:2] + pops[1][:1], n)  # overlaps populations 0 and 1, disjoint from 2 and 3
    q = [(0, 1, 2, 3)]
    bad = [
        ([(0, 100)], mk[:3], [(0, 1, 2, 2)], "n_pop must be 4..8"),
        ([(0, 100)], mk + mk + [mk[0]], q, "n_pop must be 4..8"),
        ([(0, 100)], mk[:3] + [flags([], n)], q, "is empty"),
        ([(0, 100)], mk, [(0, 1, 2, 4)], "population index 4"),
        ([(0, 100)], mk, [(0, 1, 2, 2)], "share a haplotype"),
        ([(0, 100)], mk + [extra], [(0, 1, 4, 3)], "share a haplotype"),
        ([(0, S + 1)], mk, q, "bad site range"),
        ([(100, 10)], mk, q, "bad site range"),
    ]
    for wins, mm, quartets, needle in bad:
        with pytest.raises(ImpopError) as ei:
            bm.dstat_scan(wins, mm, quartets)
        assert ei.value.code == E_INVALID and needle in str(ei.value), (needle, str(ei.value))
    # populations that never share a quartet may overlap
    got = bm.dstat_scan(dc.GEOMETRY_WINDOWS, mk + [extra], q)
    pd.assert_matches(got, pd.reference(m01, pops, q, dc.GEOMETRY_WINDOWS, False), "overlapping populations outside the quartet")
    w = impop_amd.make_windows([(0, 100)])
    out = np.zeros(1, dtype=impop_amd.DSTAT_DTYPE)
    packed = np.concatenate([impop_amd.pack_mask(f, n) for f in mk])
    qa = np.array([0, 1, 2, 3], dtype=np.uint32)
    prm = _lib.DstatParams(C.sizeof(_lib.DstatParams) - 4, 0, 0, 0)  # a wrong struct_size
    rc = ctx._lib.impop_dstat_scan(ctx.handle, bm.handle, w.ctypes.data_as(C.POINTER(_lib.Window)), 1, packed.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   4, qa.ctypes.data_as(C.POINTER(C.c_uint32)), 1, C.byref(prm), out.ctypes.data_as(C.POINTER(_lib.DstatStats)))
    assert rc == E_INVALID
    empty = bm.dstat_scan([], mk, q)
    assert empty.shape == (0, 1) and empty.dtype == impop_amd.DSTAT_DTYPE
    bm.free()


def test_refuses_65536_haplotypes(ctx):
    from impop_amd import ImpopError
    n, S = 65536, 64
    m = np.zeros((n, S), np.uint8)
    m[::2, 9] = 1
    bm = ctx.upload_dense(m, keep_hap_major=False)
    with pytest.raises(ImpopError) as ei:
        bm.dstat_scan([(0, S)], masks([[0, 1], [2, 3], [4, 5], [6, 7]], n), [(0, 1, 2, 3)])
    assert ei.value.code == E_INVALID and "65535" in str(ei.value)
    bm.free()


# ---- timing ---------------------------------------------------------------------------------------------------------------------------

def test_timer_brackets_the_streaming_launches(ctx):
    m01, pops, quartets, wins = _group_case()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    ctx.gram_timing(True)
    bm.dstat_scan(wins, masks(pops, 130), quartets)
    ms, launches = ctx.dstat_elapsed()
    ctx.gram_timing(False)
    from impop_amd import _lib
    assert ms > 0.0 and launches == -(-len(quartets) // _lib.DSTAT_GROUP)
    bm.free()


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def test_cli_prints_the_known_answer(tmp_path):
    from impop_amd import matrixio
    names = [f"S{i}#1#chr9:1000-1006" for i in range(8)]
    matrixio.save_matrix(str(tmp_path / "m.npz"), matrixio.from_dense(dc.known_matrix(), names, origin=1000, contig="CHM13#0#chr9"))
    (tmp_path / "w.bed").write_text("chr9\t1000\t1006\n")
    for k, label in enumerate(("p1", "p2", "p3", "o")):
        (tmp_path / f"{label}.txt").write_text("".join(f"S{h}#1\n" for h in dc.KNOWN_POPS[k]))
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", str(tmp_path / "m.npz"), "--bed", str(tmp_path / "w.bed"),
           "--format", "dstat", "--panel"] + [str(tmp_path / f"{x}.txt") for x in ("p1", "p2", "p3", "o")]
    for extra in ([], ["--compact", "--dstat-polarize"]):
        r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert len(lines) == 2 and lines[0].startswith("CHROM\tSTART\tEND\tP1\tP2\tP3\tO")
        assert lines[1] == "CHM13#0#chr9\t1000\t1006\tp1\tp2\tp3\to\t6\t4\t0\t1.75000000\t1.00000000\t0.27272727\t-0.75000000\t0.30000000"
