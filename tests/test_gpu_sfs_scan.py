"""GPU: impop_sfs_scan against the plain restatement of tests/plain_sfs.py — every integer, all eight doubles and every table bin,
bit for bit, NaN matching NaN.  What needs the trace line (IMPOP_TRACE=1 is read once per process) runs in one child process per
module."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import dstat_cases as dc
import plain_sfs as ps
import sfs_cases as sc
from conftest import ROOT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = -1, -5
BOTH = ("sfs", "jsfs")


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


def flipped(m01, pops, outgroup):
    return sum(ps.polarized_counts(m01, pops, outgroup)[2])


def same_bytes(a, b):
    """two sfs_scan results: the same bytes in the records and in every table"""
    if a[0].tobytes() != b[0].tobytes() or a[1].tobytes() != b[1].tobytes():
        return False
    for x, y in ((a[2], b[2]), (a[3], b[3])):
        if (x is None) != (y is None) or (x is not None and any(p.shape != q.shape or (p != q).any() for p, q in zip(x, y))):
            return False
    return True


# ---- the known answer of the header -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("outgroup", (None, 2))
def test_known_answer(ctx, outgroup):
    bm = ctx.upload_dense(sc.known_matrix(), keep_hap_major=False)
    got = bm.sfs_scan([sc.KNOWN_WINDOW], masks(sc.KNOWN_POPS, 12), sc.KNOWN_PAIRS, outgroup=outgroup, tables=BOTH)
    sc.assert_known(got, outgroup)
    ps.assert_matches(got, ps.reference(sc.known_matrix(), sc.KNOWN_POPS, sc.KNOWN_PAIRS, [sc.KNOWN_WINDOW], outgroup), "known")
    bm.free()


# ---- geometry: tails of 1..4 dwords, more than one full granule, the 73 KB joint table at 465; default tiles and tiles of 1, 2, 5 blocks

_GEOMETRY = {}


def geometry_reference(n, outgroup):
    """the case and its restatement, computed once per module"""
    if (n, outgroup) not in _GEOMETRY:
        m01, pops = sc.geometry_case(n)
        want = ps.reference(m01, pops, sc.GEOMETRY_PAIRS, sc.GEOMETRY_WINDOWS, outgroup)
        sc.assert_not_hollow(want, outgroup, flipped(m01, pops, outgroup))
        _GEOMETRY[(n, outgroup)] = (m01, pops, want)
    return _GEOMETRY[(n, outgroup)]


@pytest.mark.parametrize("n", sc.GEOMETRY_N)
def test_shapes_against_the_restatement(ctx, n, monkeypatch):
    m01, pops, _ = geometry_reference(n, None)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    for outgroup in (None, sc.GEOMETRY_OUTGROUP):
        want = geometry_reference(n, outgroup)[2]
        for tile_blocks in (None, 1, 2, 5):
            if tile_blocks is None:
                monkeypatch.delenv("IMPOP_SFS_TILE_BLOCKS", raising=False)
            else:
                monkeypatch.setenv("IMPOP_SFS_TILE_BLOCKS", str(tile_blocks))
            got = bm.sfs_scan(sc.GEOMETRY_WINDOWS, masks(pops, n), sc.GEOMETRY_PAIRS, outgroup=outgroup, tables=BOTH)
            ps.assert_matches(got, want, (n, outgroup, tile_blocks))
    if n == 465:  # the joint table the LDS form has to hold next to three masks
        assert (len(pops[0]) + 1) * (len(pops[1]) + 1) * 4 > 72000
    if n == 12:  # populations of 2 and 3: variances that are exactly zero
        st = geometry_reference(12, None)[2][0]
        assert np.isnan(st["tajima_d"][:, 2]).all() and (st["seg"][:, 2] > 0).any()
    bm.free()


def test_tables_do_not_depend_on_the_other_populations(ctx):
    n = 70
    m01, pops, want = geometry_reference(n, None)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    # K = 1 without pairs; the same population among others gives the same record and spectrum
    st, pr, sfs, jsfs = bm.sfs_scan(sc.GEOMETRY_WINDOWS, masks(pops[1:2], n), tables=("sfs",))
    assert st.shape == (7, 1) and pr.shape == (7, 0) and jsfs is None and len(sfs) == 1
    assert st[:, 0].tobytes() == np.ascontiguousarray(want[0][:, 1]).tobytes() and (sfs[0] == want[2][1]).all()
    # no tables asked: none come back, the records are the same
    st2, pr2, none1, none2 = bm.sfs_scan(sc.GEOMETRY_WINDOWS, masks(pops, n), sc.GEOMETRY_PAIRS)
    assert none1 is None and none2 is None
    ps.assert_matches((st2, pr2, None, None), want, "no tables")
    # the mirrored pair is the transposed table with a and b swapped
    got = bm.sfs_scan(sc.GEOMETRY_WINDOWS, masks(pops, n), sc.GEOMETRY_PAIRS, tables=("jsfs",))
    assert got[2] is None and (got[3][0] == got[3][1].transpose(0, 2, 1)).all()
    assert (got[1]["private_a"][:, 0] == got[1]["private_b"][:, 1]).all() and (got[1]["fixed_a"][:, 0] == got[1]["fixed_b"][:, 1]).all()
    bm.free()


# ---- cross-checks against existing entry points ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", (33, 465))
def test_agrees_with_impop_scan_and_impop_afs(ctx, n):
    m01, pops, _ = geometry_reference(n, None)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    mk = masks(pops, n)
    odd = [k for k, p in enumerate(pops) if len(p) % 2 == 1][0]  # an odd outgroup never ties: the folded quantities stay what they are
    for outgroup in (None, odd):
        st, _, sfs, _ = bm.sfs_scan(sc.GEOMETRY_WINDOWS, mk, outgroup=outgroup, tables=("sfs",))
        if outgroup is not None:
            assert (st["n_skipped"] == 0).all() and flipped(m01, pops, outgroup) > 0
        for k in range(len(pops)):
            rec = bm.scan(sc.GEOMETRY_WINDOWS, mask_p=mk[k], d_pi_mode=2, s_scope=1)
            assert (st["seg"][:, k] == rec["s_p"]).all() and (st["sum_het"][:, k] == rec["sum_p"]).all(), (n, outgroup, k)
            assert (st["n_sites"][:, k] == rec["n_sites"]).all()
            a, b = st["tajima_d"][:, k], rec["tajima_d"]
            assert (np.isnan(a) == np.isnan(b)).all(), (n, outgroup, k, a, b)
            ok = ~np.isnan(a)
            assert (np.abs(a[ok] - b[ok]) <= 1e-9 * np.abs(b[ok])).all(), (n, outgroup, k, a, b)
            if outgroup is None:  # impop_afs counts the stored allele, bins 0 and n included
                afs = bm.afs(sc.GEOMETRY_WINDOWS, mk[k])
                assert afs.shape == sfs[k].shape and (afs[:, 1:-1] == sfs[k][:, 1:-1]).all()
                assert (sfs[k][:, 0] == 0).all() and (sfs[k][:, -1] == 0).all()
    bm.free()


# ---- weights: the sums of the bp-expanded matrix, the counters and the tables those of the columns -----------------------------------

def test_weights_are_the_expanded_matrix(ctx):
    n, S = 33, 300
    rng = np.random.default_rng(33300)
    m01 = dc.draw_sites(rng, n, S)
    pops = sc.cut_pops(rng, n)
    sc.plant(rng, m01, pops, 100, 250)
    w = rng.integers(1, 10, S).astype(np.uint32)
    w[137] = 70000
    wins = [(0, S), (5, 137), (130, 140), (137, 138), (138, 300)]
    start = np.concatenate([[0], np.cumsum(w.astype(np.int64))])
    wins_x = [(int(start[b]), int(start[e])) for b, e in wins]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    bm.set_site_weights(w)
    bx = ctx.upload_dense(np.repeat(m01, w, axis=1), keep_hap_major=False)
    for outgroup in (None, sc.GEOMETRY_OUTGROUP):
        want = ps.reference(m01, pops, sc.GEOMETRY_PAIRS, wins, outgroup, weights=w)
        got = bm.sfs_scan(wins, masks(pops, n), sc.GEOMETRY_PAIRS, outgroup=outgroup, tables=BOTH)
        ps.assert_matches(got, want, ("weighted", outgroup))  # counters and tables count columns
        exp = bx.sfs_scan(wins_x, masks(pops, n), sc.GEOMETRY_PAIRS, outgroup=outgroup)
        for f in ("n_sites", "sum_het", "sum_c", "sum_c2", "theta_pi", "theta_h", "theta_l", "faywu_h"):
            assert ps.bits_equal(got[0][f], exp[0][f]).all() if got[0].dtype[f].kind == "f" else (got[0][f] == exp[0][f]).all(), f
        assert (exp[0]["seg"] >= got[0]["seg"]).all() and (exp[0]["seg"] > got[0]["seg"]).any()
    bx.free()
    bm.free()


# ---- overlap and order --------------------------------------------------------------------------------------------------------------

def test_permuting_the_windows_permutes_the_records_and_tables(ctx, monkeypatch):
    n = 70
    m01, pops, _ = geometry_reference(n, None)
    wins = [(0, 2100), (10, 300), (250, 900), (250, 900), (299, 300), (64, 128), (1000, 2099), (63, 1985), (1999, 2100), (640, 641)]
    og = sc.GEOMETRY_OUTGROUP
    want = ps.reference(m01, pops, sc.GEOMETRY_PAIRS, wins, og)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    monkeypatch.setenv("IMPOP_SFS_TILE_BLOCKS", "3")
    got = bm.sfs_scan(wins, masks(pops, n), sc.GEOMETRY_PAIRS, outgroup=og, tables=BOTH)
    ps.assert_matches(got, want, "overlap")
    assert got[0][2].tobytes() == got[0][3].tobytes() and (got[3][0][2] == got[3][0][3]).all()
    perm = np.random.default_rng(5).permutation(len(wins))
    shuffled = bm.sfs_scan([wins[i] for i in perm], masks(pops, n), sc.GEOMETRY_PAIRS, outgroup=og, tables=BOTH)
    assert same_bytes(shuffled, (got[0][perm], got[1][perm], [t[perm] for t in got[2]], [t[perm] for t in got[3]]))
    # chunking never changes a byte: a budget of one window's tables, then of three
    row_bytes = 4 * (sum(len(p) + 1 for p in pops) + sum((len(pops[a]) + 1) * (len(pops[b]) + 1) for a, b in sc.GEOMETRY_PAIRS))
    for budget in (1, 3 * row_bytes + 200):
        chunked = bm.sfs_scan(wins, masks(pops, n), sc.GEOMETRY_PAIRS, outgroup=og, tables=BOTH, max_chunk_bytes=budget)
        assert same_bytes(chunked, got), budget
    bm.free()


# ---- routes, pair groups, the two table forms, chunks and the trace line, in a child process under IMPOP_TRACE=1 ---------------------

ROUTE_N = (70, 465)
ROUTES = ("default", "norare", "dense", "compact")
OG = sc.GEOMETRY_OUTGROUP


def _group_case():
    n = 130
    m01, _ = sc.geometry_case(n)
    pops, pairs = sc.eight_pops(np.random.default_rng(808), n)
    return m01, pops, pairs, [(0, 2100), (100, 163), (700, 1400)]


def _pack(res):
    """an sfs_scan result as arrays for np.savez"""
    out = {"stats": res[0], "pairs": res[1]}
    for name, tabs in (("sfs", res[2]), ("jsfs", res[3])):
        for i, t in enumerate(tabs or []):
            out[f"{name}{i}"] = t
    return out


def _unpack(recs, tag):
    def tabs(name):
        keys = sorted((k for k in recs if re.fullmatch(rf"{re.escape(tag)}:{name}\d+", k)), key=lambda k: int(k.rsplit(name, 1)[1]))
        return [recs[k] for k in keys] or None
    return recs[f"{tag}:stats"], recs[f"{tag}:pairs"], tabs("sfs"), tabs("jsfs")


def _child(out_path):
    import impop_amd
    from impop_amd import ImpopError
    ctx = impop_amd.Context(0)
    out = {}

    def call(tag, fn):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        for k, v in _pack(fn()).items():
            out[f"{tag}:{k}"] = v
        sys.stderr.flush()

    for n in ROUTE_N:
        m01, wins, pops = sc.crafted_case(n)
        mk = masks(pops, n)
        for tag, ukw in (("default", {}), ("norare", {"rare_split": False}), ("dense", {"dense_scan": True})):
            bm = ctx.upload_dense(m01, keep_hap_major=False, **ukw)
            for og in (None, OG):
                call(f"{tag}/{n}/{og}", lambda: bm.sfs_scan(wins, mk, sc.GEOMETRY_PAIRS, outgroup=og, tables=BOTH))
            if tag == "default":  # tiles of one block: the rows and the rare entries of a window in many tiles and parts
                call(f"default_t1/{n}", lambda: bm.sfs_scan(wins, mk, sc.GEOMETRY_PAIRS, outgroup=OG, tables=BOTH, tile_blocks=1))
                call(f"default_chunks/{n}", lambda: bm.sfs_scan(wins, mk, sc.GEOMETRY_PAIRS, outgroup=OG, tables=BOTH, max_chunk_bytes=1))
                for bins in ("0", "200"):  # every job, then only the joint jobs, tally straight into global memory
                    os.environ["IMPOP_SFS_LDS_BINS"] = bins
                    call(f"default_bins{bins}/{n}", lambda: bm.sfs_scan(wins, mk, sc.GEOMETRY_PAIRS, outgroup=OG, tables=BOTH, tile_blocks=2))
                del os.environ["IMPOP_SFS_LDS_BINS"]
                cm = bm.compact()
                for og in (None, OG):
                    call(f"compact/{n}/{og}", lambda: cm.sfs_scan(wins, mk, sc.GEOMETRY_PAIRS, outgroup=og, tables=BOTH))
                cm.free()
            bm.free()
    m01, pops, pairs, wins = _group_case()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    call("group28", lambda: bm.sfs_scan(wins, masks(pops, 130), pairs, outgroup=7, tables=BOTH))
    call("group1", lambda: bm.sfs_scan(wins, masks(pops, 130), pairs[:1], outgroup=7, tables=BOTH))
    call("group0", lambda: bm.sfs_scan(wins, masks(pops, 130), [], outgroup=7))
    bm.free()
    # the overflow bound depends on sizes and weights alone: refused before any launch
    n = 65535
    bm = ctx.upload_dense(np.ones((n, 1), np.uint8), keep_hap_major=False)
    bm.set_site_weights(np.array([2 ** 31], dtype=np.uint32))
    sys.stderr.write("@@call overflow\n")
    sys.stderr.flush()
    try:
        bm.sfs_scan([(0, 1)], masks([range(0, 10), range(10, n)], n), [(0, 1)])
        out["overflow"] = np.array([0])
    except ImpopError as exc:
        out["overflow"] = np.array([exc.code])
        out["overflow_msg"] = np.array([str(exc)])
    bm.free()
    ctx.close()
    np.savez(out_path, **out)


_TRACE = re.compile(r"\[impop_sfs_scan\] (.*)$")


@pytest.fixture(scope="module")
def child():
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
        env.pop("IMPOP_SFS_TILE_BLOCKS", None)
        env.pop("IMPOP_SFS_LDS_BINS", None)
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_sfs_scan as t; t._child(sys.argv[1])", path],
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
    from impop_amd import _lib
    recs, trace, _ = child
    m01, wins, pops = sc.crafted_case(n)
    for og in (None, OG):
        want = ps.reference(m01, pops, sc.GEOMETRY_PAIRS, wins, og)
        sc.assert_not_hollow(want, og, flipped(m01, pops, og))
        base = _unpack(recs, f"default/{n}/{og}")
        ps.assert_matches(base, want, ("default", n, og))
        for tag in ROUTES[1:]:
            assert same_bytes(_unpack(recs, f"{tag}/{n}/{og}"), base), (tag, n, og)
    base = _unpack(recs, f"default/{n}/{OG}")
    for tag in ("default_t1", "default_chunks", "default_bins0", "default_bins200"):
        assert same_bytes(_unpack(recs, f"{tag}/{n}"), base), (tag, n)
    lines = [trace[f"{t}/{n}/None"] for t in ROUTES]
    assert all(len(x) == 1 for x in lines)
    assert [x[0]["route"] for x in lines] == ["indexed+rare", "indexed", "dense", "compact"]
    n_jobs = 4 + len(sc.GEOMETRY_PAIRS)
    for x in lines:
        x = x[0]
        assert x["windows"] == len(wins) and x["pops"] == 4 and x["pairs"] == 3 and x["tiles"] >= 1 and x["chunks"] == 1
        assert x["table_jobs"] == n_jobs == x["lds_jobs"] and x["table_items"] >= len(wins) - 2  # a window without a variable site has no tile
        assert x["launches"] == 2 + n_jobs  # one pair group: a streaming and a finalize launch, then a launch per table
        assert x["table_bytes_streamed"] >= n_jobs * x["bytes_streamed"]  # overlapping windows re-read the tiles they share
    split, plain, dense, compact = (x[0]["bytes_streamed"] for x in lines)
    assert split < dense and plain < dense and compact < dense
    one, t1 = trace[f"default/{n}/{OG}"][0], trace[f"default_t1/{n}"][0]
    assert t1["tiles"] > one["tiles"] and t1["table_items"] > one["table_items"]
    chunks = trace[f"default_chunks/{n}"][0]
    assert chunks["chunks"] == len(wins) and (chunks["launches"] - 2) % n_jobs == 0  # a launch per job and chunk that has an item
    assert len(wins) - 2 <= (chunks["launches"] - 2) // n_jobs <= len(wins)
    assert chunks["table_items"] == one["table_items"] and chunks["table_bytes_streamed"] == one["table_bytes_streamed"]
    assert trace[f"default_bins0/{n}"][0]["lds_jobs"] == 0
    small = sum(1 for p in pops if len(p) + 1 <= 200)  # IMPOP_SFS_LDS_BINS=200: the spectra stay in LDS, the joint tables go global
    assert trace[f"default_bins200/{n}"][0]["lds_jobs"] == small and 0 < small < n_jobs
    assert _lib.SFS_PAIR_GROUP >= 3


def test_pair_groups(child):
    from impop_amd import _lib
    recs, trace, _ = child
    m01, pops, pairs, wins = _group_case()
    assert len(pairs) == 28 == _lib.SFS_MAX_PAIRS and len(pops) == 8 and len(pops[7]) % 2 == 0
    want = ps.reference(m01, pops, pairs, wins, 7)
    g28, g1, g0 = (_unpack(recs, t) for t in ("group28", "group1", "group0"))
    ps.assert_matches(g28, want, "group28")
    assert (want[0]["seg"][:, :7] >= 2).all() and want[0]["n_skipped"].max() > 0 and all(t.sum() > 0 for t in want[3])
    assert g1[0].tobytes() == g28[0].tobytes() == g0[0].tobytes()  # the populations' records do not depend on the pair list
    assert g1[1].tobytes() == np.ascontiguousarray(g28[1][:, :1]).tobytes() and (g1[3][0] == g28[3][0]).all()
    assert g0[1].shape == (3, 0) and g0[2] is None
    one, all28, none = trace["group1"][0], trace["group28"][0], trace["group0"][0]
    n_groups = -(-28 // _lib.SFS_PAIR_GROUP)
    assert n_groups > 1 and none["launches"] == 2 and none["table_jobs"] == 0 and none["chunks"] == 0
    assert one["launches"] == 2 + 8 + 1 and all28["launches"] == 2 * n_groups + 8 + 28
    assert all28["pairs"] == 28 and all28["tiles"] == one["tiles"] and all28["bytes_streamed"] == one["bytes_streamed"]


def test_overflow_bound_refuses_before_any_launch(child):
    recs, trace, other = child
    assert recs["overflow"].tolist() == [E_UNSUPPORTED]
    msg = str(recs["overflow_msg"][0])
    assert "population 1" in msg and "window 0" in msg and "2^62" in msg
    assert trace["overflow"] == [] and other["overflow"] == []  # neither the route nor the scan was reached


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals(ctx):
    import impop_amd
    from impop_amd import ImpopError, _lib
    n = 33
    m01, pops, want = geometry_reference(n, None)
    S = m01.shape[1]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    mk = masks(pops, n)
    extra = flags(pops[0][:2] + pops[1][:1], n)  # overlaps populations 0 and 1, disjoint from 2 and 3
    W = [(0, 100)]
    bad = [
        (W, [], (), {}, "n_pop must be 1..8"),
        (W, mk + mk + [mk[0]], (), {}, "n_pop must be 1..8"),
        (W, mk[:3] + [flags([], n)], (), {}, "is empty"),
        (W, mk, [(0, 4)], {}, "population index 4"),
        (W, mk, [(2, 2)], {}, "both populations are 2"),
        (W, mk + [extra], [(4, 0)], {}, "share a haplotype"),
        (W, mk, [(0, 1)] * 29, {}, "n_pairs must be 0..28"),
        (W, mk, (), {"outgroup": 4}, "outgroup 4 outside"),
        (W, mk, (), {"tables": ("jsfs",)}, "need at least one pair"),
        ([(0, S + 1)], mk, (), {}, "bad site range"),
        ([(100, 10)], mk, (), {}, "bad site range"),
    ]
    for wins, mm, pairs, kw, needle in bad:
        with pytest.raises(ImpopError) as ei:
            bm.sfs_scan(wins, mm, pairs, **kw)
        assert ei.value.code == E_INVALID and needle in str(ei.value), (needle, str(ei.value))
    # populations that share no pair may overlap
    got = bm.sfs_scan(sc.GEOMETRY_WINDOWS, mk + [extra], sc.GEOMETRY_PAIRS + [(4, 2)], tables=BOTH)
    assert got[0][:, :4].tobytes() == want[0].tobytes() and (got[1][:, :3] == want[1]).all()
    ps.assert_matches(got, ps.reference(m01, pops + [sorted(pops[0][:2] + pops[1][:1])], sc.GEOMETRY_PAIRS + [(4, 2)], sc.GEOMETRY_WINDOWS), "overlap")
    # the raw call: a wrong struct_size, a requested table without its pointer
    w = impop_amd.make_windows(W)
    out = np.zeros(4, dtype=impop_amd.SFS_DTYPE)
    packed = np.concatenate([impop_amd.pack_mask(f, n) for f in mk])

    def raw(prm):
        return ctx._lib.impop_sfs_scan(ctx.handle, bm.handle, w.ctypes.data_as(C.POINTER(_lib.Window)), 1, packed.ctypes.data_as(C.POINTER(C.c_uint64)),
                                       4, None, 0, C.byref(prm), out.ctypes.data_as(C.POINTER(_lib.SfsStats)), None, None, None)

    assert raw(_lib.SfsParams(C.sizeof(_lib.SfsParams) - 4, -1, 0, 0, 0)) == E_INVALID
    assert raw(_lib.SfsParams(C.sizeof(_lib.SfsParams), -1, 0, _lib.SFS_TABLE_1D, 0)) == E_INVALID
    assert "sfs_out is NULL" in ctx._lib.impop_last_error().decode()
    assert raw(_lib.SfsParams(C.sizeof(_lib.SfsParams), -1, 0, 0, 0)) == 0
    assert out.tobytes() == bm.sfs_scan(W, mk)[0].tobytes()
    empty = bm.sfs_scan([], mk, sc.GEOMETRY_PAIRS, tables=BOTH)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 3) and empty[0].dtype == impop_amd.SFS_DTYPE and empty[3][0].shape[0] == 0
    bm.free()


def test_refuses_65536_haplotypes(ctx):
    from impop_amd import ImpopError
    n, S = 65536, 64
    m = np.zeros((n, S), np.uint8)
    m[::2, 9] = 1
    bm = ctx.upload_dense(m, keep_hap_major=False)
    with pytest.raises(ImpopError) as ei:
        bm.sfs_scan([(0, S)], masks([[0, 1], [2, 3]], n), [(0, 1)])
    assert ei.value.code == E_INVALID and "65535" in str(ei.value)
    bm.free()


# ---- timing ---------------------------------------------------------------------------------------------------------------------------

def test_timer_brackets_the_streaming_launches(ctx):
    from impop_amd import _lib
    m01, pops, pairs, wins = _group_case()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    ctx.gram_timing(True)
    bm.sfs_scan(wins, masks(pops, 130), pairs)
    ms, launches = ctx.sfs_elapsed()
    assert ms[0] > 0.0 and ms[1] == 0.0 and launches == -(-len(pairs) // _lib.SFS_PAIR_GROUP)
    bm.sfs_scan(wins, masks(pops, 130), pairs[:1], tables=BOTH)
    ms2, launches2 = ctx.sfs_elapsed()
    ctx.gram_timing(False)
    assert ms2[0] > ms[0] and ms2[1] > 0.0 and launches2 == launches + 1
    bm.free()


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def test_cli_prints_the_known_answer(tmp_path):
    from impop_amd import matrixio
    names = [f"S{i}#1#chr9:1000-1011" for i in range(12)]
    matrixio.save_matrix(str(tmp_path / "m.npz"), matrixio.from_dense(sc.known_matrix(), names, origin=1000, contig="CHM13#0#chr9"))
    (tmp_path / "w.bed").write_text("chr9\t1000\t1011\n")
    for k, label in enumerate(("a", "b", "o")):
        (tmp_path / f"{label}.txt").write_text("".join(f"S{h}#1\n" for h in sc.KNOWN_POPS[k]))
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", str(tmp_path / "m.npz"), "--bed", str(tmp_path / "w.bed"),
           "--format", "sfs", "--panel"] + [str(tmp_path / f"{x}.txt") for x in ("a", "b", "o")]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 4 and lines[0].startswith("CHROM\tSTART\tEND\tPOP\tN\tN_SITES\tS\tETA1")
    assert lines[2] == ("CHM13#0#chr9\t1000\t1011\tb\t5\t11\t4\t2\t1\t0\t1.92000000\t1.80000000\t2.20000000\t2.00000000\t-0.41017465\t-0.40000000\t"
                        "-0.34892049\t0.13767880")
    extra = ["--compact", "--sfs-outgroup", "3", "--sfs-pair", "1,2", "--sfs-pairs-out", str(tmp_path / "p.tsv"), "--sfs-spectra", str(tmp_path / "s.npz")]
    r = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[1].split("\t")[3:10] == ["a", "5", "11", "4", "1", "1", "2"] and lines[1].split("\t")[14] == "0.27344977"
    assert (tmp_path / "p.tsv").read_text().splitlines()[1] == "CHM13#0#chr9\t1000\t1011\ta\tb\t2\t1\t2\t2\t0\t7"
    z = np.load(tmp_path / "s.npz")
    assert sorted(z.files) == ["jsfs_a_b", "sfs_a", "sfs_b", "sfs_o"] and z["jsfs_a_b"].shape == (1, 6, 6)
    assert {(int(a), int(b)): int(z["jsfs_a_b"][0, a, b]) for a, b in np.argwhere(z["jsfs_a_b"][0] > 0)} == sc.KNOWN_CELLS[2]
