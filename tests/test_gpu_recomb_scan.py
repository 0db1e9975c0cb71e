"""impop_recomb_scan on an MI355X (run with -m gpu): the four-gamete test, Hudson & Kaplan's R_min, four-gamete blocks and Wall's B
and Q of every window against the plain restatement of tests/recomb_cases.py.  Records, used_sites and the site table must be
equal, the doubles bit for bit.  What needs the trace line (IMPOP_TRACE=1 is read once per process) runs in one child process."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import hap_cases as hc
import ld_cases as lc
import recomb_cases as rc
from conftest import ROOT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = -1, -5
S = lc.S
FULL = dict(want_sites=True, want_site_table=True)


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


def test_known_answer(ctx):
    bm = ctx.upload_dense(np.ascontiguousarray(rc.KNOWN_ROWS.T), keep_hap_major=False)
    rec, used, tab = bm.recomb_scan([(0, 5)], min_mac=1, **FULL)
    K = rc.KNOWN
    assert used.shape == tab.shape == (1, 4096) and used[0, :5].tolist() == [0, 1, 2, 3, 4] and not used[0, 5:].any()
    for k in ("left1", "n_left", "rep"):
        assert tab[k][0, :5].tolist() == K[k], k
        assert not tab[k][0, 5:].any()
    assert tab["carriers"][0, :5].tolist() == [2, 2, 2, 2, 1]
    r = rec[0]
    for k in ("n_incompatible", "n_incompatible_adjacent", "rmin", "n_blocks", "longest_block_sites", "n_congruent_adjacent",
              "n_congruent_partitions", "n_partitions"):
        assert int(r[k]) == K[k], k
    assert (int(r["n_members"]), int(r["n_sites"]), int(r["n_qualifying"]), int(r["n_used"])) == (4, 5, 5, 5)
    assert (int(r["longest_block_begin"]), int(r["longest_block_end"])) == K["longest"]
    assert float(r["wall_b"]) == 0.25 and float(r["wall_q"]) == 0.4 and float(r["four_gamete_fraction"]) == 3.0 / 10.0
    from impop_amd import recomb
    assert recomb.intervals(tab["left1"][0], 5) == K["intervals"] and recomb.blocks(tab["left1"][0], 5) == [(0, 0), (1, 1), (2, 4)]
    rc.assert_matches((rec, used, tab), rc.reference(np.ascontiguousarray(rc.KNOWN_ROWS.T), None, [(0, 5)], 1), "known")
    bm.free()


# ---- shapes: 2 dwords (rows of 4 in registers), 15 (16); min_mac 1 lets singletons in, which can never show four gametes ---------

@pytest.mark.parametrize("n", (33, 64, 465))
def test_shapes_against_the_restatement(ctx, n):
    rng = np.random.default_rng(30100 + n)
    m01 = rc.planted_matrix(rng, n, p_flip=1e-3)
    wins = rc.window_list()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    sub = (rng.random(n) < 0.6).astype(np.uint8)
    sub[:3] = 1
    for flags in (None, sub):
        for min_mac in (1, 2, 24):
            got = bm.recomb_scan(wins, mask_p=flags, min_mac=min_mac, **FULL)
            ref = rc.reference(m01, flags, wins, min_mac)
            rc.assert_matches(got, ref, (n, flags is None, min_mac))
            assert bm.recomb_scan(wins, mask_p=flags, min_mac=min_mac).tobytes() == got[0].tobytes()  # the records alone (NaN included)
            if flags is None and min_mac == 2 and n >= 64:
                k = wins.index((0, S))
                assert ref[0]["rmin"][k] > 20 and ref[0]["n_blocks"][k] > 20 and ref[0]["n_partitions"][k] < ref[0]["n_used"][k]
                k = len(wins) - 3  # the planted mosaic of two trees
                assert ref[0]["n_used"][k] > 10 and ref[0]["rmin"][k] <= 1
    bm.free()


@pytest.mark.parametrize("n", (200, 1000))
def test_rows_of_8_and_32_dwords_in_registers(ctx, n):
    rng = np.random.default_rng(30150 + n)
    W = 700
    m01 = hc.founder_matrix(rng, n, W, p_site=0.5, p_flip=1e-3)
    wins = [(0, W), (37, 333), (300, 301), (650, W)]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    ref = rc.reference(m01, None, wins, 2)
    assert ref[0]["n_used"][0] > 256 and ref[0]["rmin"][0] > 0
    rc.assert_matches(bm.recomb_scan(wins, **FULL), ref, n)
    bm.free()


# ---- tile and workgroup edges: a tile holds 256 sites, a wave 64; 1025 and 2049 are past what the LD scan can hold -----------------

EDGE_Q = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1025, 2049)


def test_tile_and_workgroup_edges(ctx):
    rng = np.random.default_rng(30200)
    n = 465
    m01 = hc.founder_matrix(rng, n, S, p_site=0.85, p_flip=2e-4)
    qual = lc.qualifying(m01, None, 2)
    assert len(qual) > 2049 + 10
    wins = [lc.windows_with_q(qual, q) for q in EDGE_Q]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    got = bm.recomb_scan(wins, **FULL)
    ref = rc.reference(m01, None, wins, 2)
    assert ref[0]["n_used"].tolist() == list(EDGE_Q) and ref[0]["rmin"][-1] > 100
    rc.assert_matches(got, ref, "edges")
    bm.free()


@pytest.mark.parametrize("max_sites", (8, 64))
def test_thinning_at_and_beyond_max_sites(ctx, max_sites):
    rng = np.random.default_rng(30300 + max_sites)
    n = 465
    m01 = hc.founder_matrix(rng, n, S, p_site=0.3)
    qual = lc.qualifying(m01, None, 2)
    assert len(qual) > 6 * max_sites + 10
    wins = [lc.windows_with_q(qual, q) for q in (max_sites - 1, max_sites, max_sites + 1, 2 * max_sites + 1, 6 * max_sites + 5)] + [(0, S)]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    got = bm.recomb_scan(wins, max_sites=max_sites, **FULL)
    ref = rc.reference(m01, None, wins, 2, max_sites)
    assert ref[0]["n_qualifying"][:5].tolist() == [max_sites - 1, max_sites, max_sites + 1, 2 * max_sites + 1, 6 * max_sites + 5]
    assert ref[0]["n_used"].tolist() == [max_sites - 1] + [max_sites] * 5
    rc.assert_matches(got, ref, max_sites)
    assert got[1].shape == got[2].shape == (len(wins), max_sites)
    # thinning keeps R_min a lower bound: never above the unthinned window's
    full = bm.recomb_scan(wins)
    assert (got[0]["rmin"] <= full["rmin"]).all()
    bm.free()


def test_windows_of_more_than_256_blocks(ctx):
    """the gather ranks a window's sites from per-thread runs of 64-site blocks: one block per thread up to 16384 sites, longer
    runs beyond (here 3 and 2 blocks, with a last thread that has fewer) — for this scan and for the LD scan that shares the kernel"""
    rng = np.random.default_rng(30350)
    n, W = 33, 40000
    m01 = hc.founder_matrix(rng, n, W, p_site=0.04, p_flip=2e-4)
    wins = [(0, W), (1000, 33000), (17, 16500), (20000, 20001)]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    ref = rc.reference(m01, None, wins, 2)
    assert ref[0]["n_used"][0] > 1200 and ref[0]["rmin"][0] > 100
    rc.assert_matches(bm.recomb_scan(wins, **FULL), ref, "long")
    rc.assert_matches(bm.recomb_scan(wins, max_sites=300, **FULL), rc.reference(m01, None, wins, 2, 300), "long, thinned")
    lc.assert_matches(bm.ld_scan(wins, min_mac=2, max_sites=64, want_sites=True), lc.reference(m01, None, wins, 2, 64), "long, ld")
    bm.free()


def test_perfect_phylogeny_and_mosaic(ctx):
    rng = np.random.default_rng(30400)
    n = 465
    t01 = rc.tree_matrix(rng, n, 700)
    bm = ctx.upload_dense(t01, keep_hap_major=False)
    wins = [(0, 700), (100, 400)]
    got = bm.recomb_scan(wins, min_mac=1, **FULL)
    rc.assert_matches(got, rc.reference(t01, None, wins, 1), "tree")
    rec = got[0]
    assert (rec["n_used"] > 200).all() and not rec["n_incompatible"].any() and not rec["rmin"].any() and not rec["n_incompatible_adjacent"].any()
    assert rec["n_blocks"].tolist() == [1, 1] and rec["longest_block_sites"].tolist() == rec["n_used"].tolist()
    assert not got[2]["left1"].any() and (rec["four_gamete_fraction"] == 0.0).all()
    bm.free()
    segs = (40, 70, 25, 130)
    for nn in (33, n):
        mo = rc.mosaic(rng, nn, segs)
        bm = ctx.upload_dense(mo, keep_hap_major=False)
        got = bm.recomb_scan([(0, sum(segs))], min_mac=1, **FULL)
        rc.assert_matches(got, rc.reference(mo, None, [(0, sum(segs))], 1), ("mosaic", nn))
        assert 0 < int(got[0]["rmin"][0]) <= len(segs) - 1
        bm.free()


def test_4096_members(ctx):
    from impop_amd import _lib
    assert _lib.RECOMB_MAX_N == 4096 and _lib.RECOMB_MAX_SITES == 16384
    rng = np.random.default_rng(30500)
    n, W = 4096, 400
    m01 = hc.founder_matrix(rng, n, W, p_site=0.3, p_flip=2e-4)
    wins = [(0, W), (37, 165), (100, 101), (64, 64), (300, 400)]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    for min_mac, max_sites in ((4, 4096), (1, 300)):  # rows of 128 dwords are read from the scratch; (1, 300) holds over a tile
        got = bm.recomb_scan(wins, min_mac=min_mac, max_sites=max_sites, **FULL)
        ref = rc.reference(m01, None, wins, min_mac, max_sites)
        assert ref[0]["n_used"][0] >= 64 and ref[0]["rmin"][0] > 0
        rc.assert_matches(got, ref, ("4096", min_mac))
    assert ref[0]["n_used"][0] > 256
    bm.free()


# ---- skew: one long window among many short ones ------------------------------------------------------------------------------------

def _skew_inputs():
    rng = np.random.default_rng(30600)
    m01 = hc.founder_matrix(rng, 465, S, p_site=0.85, p_flip=2e-4)
    qual = lc.qualifying(m01, None, 2)
    big = lc.windows_with_q(qual, 2049)
    small = [(13 * k, 13 * k + 9) for k in range(200)]
    return m01, small[:77] + [big] + small[77:], [big] + small


def test_one_long_window_among_short_ones(ctx):
    m01, mixed, first = _skew_inputs()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    ref_mixed = rc.reference(m01, None, mixed, 2, 2100)
    assert ref_mixed[0]["n_used"][77] == 2049 and np.delete(ref_mixed[0]["n_used"], 77).max() < 10
    got = bm.recomb_scan(mixed, max_sites=2100, **FULL)
    rc.assert_matches(got, ref_mixed, "mixed")
    order = [77] + list(range(77)) + list(range(78, 201))
    got_first = bm.recomb_scan(first, max_sites=2100, **FULL)
    for a, b in zip(got_first, got):
        assert a.tobytes() == b[order].tobytes()
    bm.free()


def test_stale_scratch_never_reaches_a_result(ctx):
    import impop_amd
    m01, mixed, _ = _skew_inputs()
    small = [(1400, 1440), (5, 5), (2000, 2100)]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    bm.recomb_scan(mixed, min_mac=1, max_sites=2100, **FULL)  # leaves rows, lists and tables of 2049 sites in the scratch
    after = bm.recomb_scan(small, max_sites=2100, **FULL)
    bm.free()
    fresh_ctx = impop_amd.Context(0)
    fm = fresh_ctx.upload_dense(m01, keep_hap_major=False)
    fresh = fm.recomb_scan(small, max_sites=2100, **FULL)
    fm.free()
    fresh_ctx.close()
    for a, b in zip(after, fresh):
        assert a.tobytes() == b.tobytes()
    rec, used, tab = after
    for i, m in enumerate(rec["n_used"].tolist()):
        assert not used[i, m:].any() and not tab[i, m:].view(np.uint32).any()
    rc.assert_matches(after, rc.reference(m01, None, small, 2, 2100), "after")


# ---- invariance, under IMPOP_TRACE=1 in a child process -----------------------------------------------------------------------------

ROUTE_N = 465


def _route_inputs():
    rng = np.random.default_rng(30700)
    m01 = rc.planted_matrix(rng, ROUTE_N)
    weights = rng.integers(1, 9, size=S).astype(np.uint32)
    flags = (rng.random(ROUTE_N) < 0.8).astype(np.uint8)
    return m01, weights, flags, rc.window_list()


def _chunk_windows():
    return [(7 * k, 7 * k + 330) for k in range(120)]


def _child(out_path):
    import impop_amd
    from impop_amd import ImpopError
    ctx = impop_amd.Context(0)
    out = {}

    def call(tag, fn):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        r = fn()
        sys.stderr.flush()
        return r

    def keep(tag, res):
        out[tag], out[tag + "_sites"], out[tag + "_table"] = res

    m01, weights, flags, wins = _route_inputs()
    kw = dict(mask_p=flags, min_mac=2, max_sites=64, **FULL)
    ups = {"default": {}, "norare": {"rare_split": False}, "dense": {"dense_scan": True}}
    for tag, ukw in ups.items():
        bm = ctx.upload_dense(m01, keep_hap_major=False, **ukw)
        keep(tag, call(tag, lambda: bm.recomb_scan(wins, **kw)))
        if tag == "default":
            cm = bm.compact()
            keep("compact", call("compact", lambda: cm.recomb_scan(wins, **kw)))
            cm.free()
            perm = np.random.default_rng(1).permutation(len(wins))
            out["perm"] = perm
            keep("permuted", call("permuted", lambda: bm.recomb_scan([wins[k] for k in perm], **kw)))
            cw = _chunk_windows()
            keep("w120", call("w120", lambda: bm.recomb_scan(cw, **kw)))
            keep("w30", call("w30", lambda: bm.recomb_scan(cw[:30], **kw)))
            keep("chunked", call("chunked", lambda: bm.recomb_scan(cw, max_chunk_bytes=40 * 64 * (4 * 15 + 36), **kw)))
            keep("chunked_1", call("chunked_1", lambda: bm.recomb_scan(wins, max_chunk_bytes=1, **kw)))
        bm.free()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    bm.set_site_weights(weights)
    keep("weighted", call("weighted", lambda: bm.recomb_scan(wins, **kw)))
    bm.free()
    s01, mixed, _ = _skew_inputs()
    bm = ctx.upload_dense(s01, keep_hap_major=False)
    out["skew"] = call("skew", lambda: bm.recomb_scan(mixed, max_sites=2100))
    bm.free()
    big = ctx.upload_dense(np.zeros((4097, 200), np.uint8), keep_hap_major=False)
    try:
        call("over", lambda: big.recomb_scan([(0, 200)]))
        out["over"] = np.array([0])
    except ImpopError as exc:
        out["over"] = np.array([exc.code])
    f = np.ones(4097, np.uint8)
    f[0] = 0
    out["subset4096"] = call("subset4096", lambda: big.recomb_scan([(0, 200)], mask_p=f))
    big.free()
    ctx.close()
    np.savez(out_path, **out)


_TRACE = re.compile(r"\[impop_recomb_scan\] (.*)$")


@pytest.fixture(scope="module")
def child():
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_recomb_scan as t; t._child(sys.argv[1])", path],
                           capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        z = np.load(path)
        recs = {k: z[k] for k in z.files}
    trace, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@@call "):
            cur = line.split()[1]
            trace[cur] = []
        mt = _TRACE.search(line)
        if mt and cur:
            kv = dict(x.split("=") for x in mt.group(1).split())
            trace[cur].append({k: (v if k == "route" else int(v)) for k, v in kv.items()})
    return recs, trace


def _triple(recs, tag):
    return recs[tag], recs[tag + "_sites"], recs[tag + "_table"]


def _same(recs, a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(_triple(recs, a), _triple(recs, b)))


def test_uploads_and_compaction_give_identical_bytes(child):
    recs, trace = child
    m01, weights, flags, wins = _route_inputs()
    ref = rc.reference(m01, flags, wins, 2, 64)
    rc.assert_matches(_triple(recs, "default"), ref, "default")
    for tag in ("norare", "dense", "compact"):
        assert _same(recs, tag, "default"), tag
    # site weights change W and nothing else
    rc.assert_matches(_triple(recs, "weighted"), rc.reference(m01, flags, wins, 2, 64, weights), "weighted")
    a, b = recs["weighted"].copy(), recs["default"].copy()
    a["n_sites"] = b["n_sites"] = 0
    assert a.tobytes() == b.tobytes() and recs["weighted_sites"].tobytes() == recs["default_sites"].tobytes()
    assert recs["weighted_table"].tobytes() == recs["default_table"].tobytes()
    assert (recs["weighted"]["n_sites"] != recs["default"]["n_sites"]).any()
    assert [trace[t][0]["route"] for t in ("default", "norare", "dense", "compact", "weighted")] == ["dense", "dense", "dense", "compact", "dense"]
    for t in ("default", "compact"):
        assert len(trace[t]) == 1 and trace[t][0]["windows"] == len(wins)
        assert trace[t][0]["qualifying"] == int(ref[0]["n_qualifying"].sum()) and trace[t][0]["used"] == int(ref[0]["n_used"].sum())
        assert trace[t][0]["pair_tiles"] == rc.pair_tiles(ref[0])
    assert trace["compact"][0]["bytes_streamed"] < trace["default"][0]["bytes_streamed"]


def test_window_order_does_not_change_a_record(child):
    recs, _ = child
    perm = recs["perm"]
    for a, b in zip(_triple(recs, "permuted"), _triple(recs, "default")):
        assert a.tobytes() == b[perm].tobytes()


def test_chunking_never_changes_a_record(child):
    recs, trace = child
    assert trace["w120"][0]["chunks"] == 1 and trace["chunked"][0]["chunks"] >= 3
    assert _same(recs, "chunked", "w120")
    assert recs["w120"][:30].tobytes() == recs["w30"].tobytes() and recs["w120_table"][:30].tobytes() == recs["w30_table"].tobytes()
    _, _, _, wins = _route_inputs()
    assert trace["chunked_1"][0]["chunks"] == len(wins)  # a budget of one byte: a chunk per window
    assert _same(recs, "chunked_1", "default")
    m01, _, flags, _ = _route_inputs()
    cw = _chunk_windows()
    pick = [0, 1, 29, 30, 39, 40, 41, 119]
    want = rc.reference(m01, flags, [cw[k] for k in pick], 2, 64)
    rc.assert_matches(tuple(x[pick] for x in _triple(recs, "w120")), want, "w120")


def test_launches_do_not_depend_on_the_number_of_windows(child):
    _, trace = child
    (a,), (b,) = trace["w30"], trace["w120"]
    assert a["windows"] == 30 and b["windows"] == 120 and a["chunks"] == b["chunks"] == 1
    assert a["launches"] == b["launches"] and 3 <= a["launches"] <= 5
    assert trace["chunked"][0]["launches"] == a["launches"] * trace["chunked"][0]["chunks"]


def test_pair_tiles_of_a_skewed_list_are_the_windows_own(child):
    recs, trace = child
    rec = recs["skew"]
    assert rec["n_used"][77] == 2049 and trace["skew"][0]["chunks"] == 1
    tiles = (rec["n_used"].astype(np.int64) + rc.TILE - 1) // rc.TILE
    assert tiles[77] == 9 and trace["skew"][0]["pair_tiles"] == int(tiles.sum()) < 9 + 200 + 1


def test_limit_plus_one_is_refused_before_any_launch(child):
    recs, trace = child
    assert recs["over"].tolist() == [E_UNSUPPORTED] and trace["over"] == []
    assert len(trace["subset4096"]) == 1 and recs["subset4096"]["n_members"].tolist() == [4096]
    assert recs["subset4096"]["n_qualifying"].tolist() == [0] and recs["subset4096"]["n_sites"].tolist() == [200]
    assert recs["subset4096"]["n_blocks"].tolist() == [0] and np.isnan(recs["subset4096"]["wall_q"]).all()


# ---- errors -------------------------------------------------------------------------------------------------------------------------

def test_errors_and_empty_input(ctx):
    import impop_amd
    from impop_amd import ImpopError
    rng = np.random.default_rng(30800)
    n, W = 40, 300
    m01 = hc.founder_matrix(rng, n, W, p_flip=2e-3)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    cases = [([(10, 100)], {"mask_p": np.zeros(n, np.uint8)}), ([(10, 100)], {"min_mac": 0}), ([(10, 100)], {"max_sites": 1}),
             ([(10, 100)], {"max_sites": 16385}), ([(100, 10)], {}), ([(10, W + 1)], {})]
    for wins, kw in cases:
        with pytest.raises(ImpopError) as ei:
            bm.recomb_scan(wins, **kw)
        assert ei.value.code == E_INVALID, (wins, kw)
    assert len(bm.recomb_scan([(10, 100)], max_sites=2)) == 1 and len(bm.recomb_scan([(10, 100)], max_sites=16384)) == 1
    got = bm.recomb_scan([(10, 100)], max_sites=0, **FULL)  # 0 = 4096
    assert got[1].shape == (1, 4096)
    rc.assert_matches(got, rc.reference(m01, None, [(10, 100)], 2, 4096), "0 = 4096")
    empty = bm.recomb_scan([])
    assert empty.dtype == impop_amd.RECOMB_DTYPE and len(empty) == 0
    rec, sites, tab = bm.recomb_scan([], **FULL)
    assert len(rec) == 0 and sites.shape == (0, 4096) and tab.shape == (0, 4096) and tab.dtype == impop_amd.RECOMB_SITE_DTYPE
    bm.free()


def test_timers_bracket_the_four_kernel_groups(ctx):
    rng = np.random.default_rng(30900)
    m01 = rc.planted_matrix(rng, 64)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    ctx.gram_timing(True)
    bm.recomb_scan(lc.window_list(), max_chunk_bytes=1)
    ms, chunks = ctx.recomb_elapsed()
    ctx.gram_timing(False)
    assert chunks == len(lc.window_list()) and len(ms) == 4 and all(t > 0.0 for t in ms)
    bm.free()


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def test_cli_tables_are_the_restatement(ctx, tmp_path):
    from impop_amd.matrixio import MatrixFile, save_matrix
    from impop_amd import pack_hap_major
    rng = np.random.default_rng(31000)
    n, W, origin = 40, 900, 5000
    m01 = hc.founder_matrix(rng, n, W, nf=5, p_site=0.2, p_flip=0.002)
    names = [f"S{i:02d}#1#chrT:0-1" for i in range(n)]
    mpath, bed, sub = str(tmp_path / "m.npz"), str(tmp_path / "w.bed"), str(tmp_path / "u.txt")
    save_matrix(mpath, MatrixFile(bits=pack_hap_major(m01), n_site=W, names=names, origin=origin, contig="chrT"))
    rows = [(0, 130), (100, 300), (250, 251), (300, 900), (837, 900), (0, 900)]
    open(bed, "w").write("".join(f"chrT\t{origin + b}\t{origin + e}\n" for b, e in rows))
    keep = sorted(rng.choice(n, 31, replace=False).tolist())
    open(sub, "w").write("".join(names[i].partition("chrT")[0] + "\n" for i in keep))
    flags = np.zeros(n, np.uint8)
    flags[keep] = 1

    def fmt(x):
        return "NA" if np.isnan(x) else "%.8f" % x

    def tables(ref, members):
        rec, used, tab = ref
        main = ["REGION\tLENGTH\tSAMPLES\tSITES\tQUALIFYING\tUSED\tRMIN\tFGT_PAIRS\tFGT_FRACTION\tFGT_ADJACENT\tBLOCKS\tLONGEST_BLOCK_SITES\t"
                "LONGEST_BLOCK_START\tLONGEST_BLOCK_END\tWALL_B\tWALL_Q"]
        iv, bl = ["REGION\tINTERVAL\tLEFT_SITE\tRIGHT_SITE\tLEFT_POS\tRIGHT_POS"], ["REGION\tBLOCK\tFIRST_SITE\tLAST_SITE\tSITES\tSTART\tEND"]
        for i, (b, e) in enumerate(rows):
            reg, m = f"chrT:{origin + b}-{origin + e}", int(rec["n_used"][i])
            main.append("\t".join([reg, str(e - b), str(members), str(e - b), str(int(rec["n_qualifying"][i])), str(m), str(int(rec["rmin"][i])),
                                   str(int(rec["n_incompatible"][i])), fmt(rec["four_gamete_fraction"][i]),
                                   str(int(rec["n_incompatible_adjacent"][i])), str(int(rec["n_blocks"][i])),
                                   str(int(rec["longest_block_sites"][i])),
                                   str(origin + int(rec["longest_block_begin"][i])) if m else "NA",
                                   str(origin + int(rec["longest_block_end"][i])) if m else "NA", fmt(rec["wall_b"][i]), fmt(rec["wall_q"][i])]))
            left1 = tab["left1"][i, :m].tolist()
            for k, (a, z) in enumerate(rc.rmin_intervals(left1)):
                iv.append("\t".join([reg, str(k), str(a), str(z), str(origin + int(used[i, a])), str(origin + int(used[i, z]))]))
            for k, (a, z) in enumerate(rc.maximal_blocks(left1)):
                bl.append("\t".join([reg, str(k), str(a), str(z), str(z - a + 1), str(origin + int(used[i, a])), str(origin + int(used[i, z]))]))
        return tuple("\n".join(t) + "\n" for t in (main, iv, bl))

    def run(extra):
        ivp, blp = str(tmp_path / "iv.tsv"), str(tmp_path / "bl.tsv")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_recomb.py"), "--matrix", mpath, "--bed", bed,
                            "--recomb-intervals", ivp, "--recomb-blocks", blp] + extra, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout, open(ivp).read(), open(blp).read()

    want = tables(rc.reference(m01, None, rows, 2, 4096), n)
    assert "NA" in want[0] and len(want[1].splitlines()) > 3 and len(want[2].splitlines()) > 8
    assert run([]) == want and run(["--compact"]) == want
    mac = max(1, int(np.ceil(0.1 * 31)))
    assert run(["-u", sub, "--recomb-min-maf", "0.1", "--recomb-max-sites", "16"]) == tables(rc.reference(m01, flags, rows, mac, 16), 31)
