"""impop_ldband_scan on an MI355X (run with -m gpu): the banded r2 pass with its decay bins, LD scores and greedy pruning of every
window against the plain restatement of tests/ldband_cases.py.  Records (the NaN bytes of mean_r2 included), bins, the flat site
table and n_site_rows must be equal bit for bit.  What needs the trace line (IMPOP_TRACE=1 is read once per process) runs in one
child process."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import hap_cases as hc
import ld_cases as lc
import ldband_cases as bc
from conftest import ROOT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = -1, -5
S = lc.S
FULL = dict(want_bins=True, want_sites=True)
COMMON = dict(bin_width=50, n_bins=16, threshold=(1, 5))
CASES = ((1, 64, 0), (2, 300, 0), (2, 7, 150), (24, 1024, 0))  # min_mac, band_sites, max_dist


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


def scan(bm, wins, flags, case, **kw):
    return bm.ldband_scan(wins, mask_p=flags, min_mac=case[0], band_sites=case[1], max_dist=case[2], **{**COMMON, **FULL, **kw})


def ref_of(m01, flags, wins, case, **kw):
    return bc.reference(m01, flags, wins, case[0], case[1], case[2], **{**COMMON, **kw})


def test_known_answer(ctx):
    m01 = np.ascontiguousarray(bc.KNOWN_ROWS.T)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    rec, bins, tab = bm.ldband_scan([(0, 5)], **bc.KNOWN_PARAMS, **FULL)
    K = bc.KNOWN
    r = rec[0]
    for k in ("n_pairs", "sum_r2_fx", "n_perfect", "n_strong", "n_kept"):
        assert int(r[k]) == K[k], k
    assert (int(r["n_members"]), int(r["n_sites"]), int(r["n_qualifying"]), int(r["site_off"])) == (4, 5, 5, 0)
    assert float(r["mean_r2"]) == 4652881236.0 / (10.0 * 1073741824.0)
    assert tab["coord"].tolist() == [0, 1, 2, 3, 4] and tab["kept"].tolist() == K["kept"] and tab["ld_score_fx"].tolist() == K["ld_score_fx"]
    assert tab["n_partners"].tolist() == K["n_partners"] and tab["carriers"].tolist() == K["carriers"]
    assert tab["n_strong"].tolist() == K["n_strong_site"]
    assert [tuple(int(x) for x in bins[0, b]) for b in range(3)] == K["bins"]
    p = bc.KNOWN_PARAMS
    bc.assert_matches((rec, bins, tab), bc.reference(m01, None, [(0, 5)], p["min_mac"], p["band_sites"], p["max_dist"], p["bin_width"],
                                                     p["n_bins"], p["threshold"]), "known")
    from impop_amd import ldband
    assert ldband.kept_positions(tab) == [0, 1, 4]
    bm.free()


# ---- shapes: 2 dwords (rows of 4 in registers) and 15 (16); empty, one-site, monomorphic-only and overlapping windows ---------------

@pytest.mark.parametrize("n", (33, 465))
def test_shapes_against_the_restatement(ctx, n):
    m01 = bc.planted_matrix(np.random.default_rng(31000 + n), n, p_flip=1e-3)
    wins = bc.window_list()
    rng = np.random.default_rng(31050 + n)
    sub = (rng.random(n) < 0.6).astype(np.uint8)
    sub[:3] = 1
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    whole, planted = wins.index((0, S)), wins.index((1000, 1051))
    for flags in (None, sub):
        for case in CASES:
            got = scan(bm, wins, flags, case)
            ref = ref_of(m01, flags, wins, case)
            bc.assert_matches(got, ref, (n, flags is None, case))
            plain = bm.ldband_scan(wins, mask_p=flags, min_mac=case[0], band_sites=case[1], max_dist=case[2], **COMMON)
            assert plain.tobytes() == got[0].tobytes()  # the records alone (NaN included)
            if flags is not None:
                continue
            rec = ref[0]
            if case[0] <= 2:  # the five planted columns, all inside every band
                assert (int(rec["n_qualifying"][planted]), int(rec["n_pairs"][planted])) == (5, 10)
                assert (int(rec["n_strong"][planted]), int(rec["n_perfect"][planted]), int(rec["n_kept"][planted])) == (6, 3, 2)
            if n == 465:  # no path is dead: the figures of the whole matrix
                q, pairs, strong, kept = (int(rec[k][whole]) for k in ("n_qualifying", "n_pairs", "n_strong", "n_kept"))
                if case == (2, 300, 0):
                    assert (q, pairs, strong, kept) == (526, 112650, 9428, 180) and (ref[1]["pairs"][whole] > 0).all()
                if case == (1, 64, 0):
                    assert (q, kept) == (1285, 948)
                if case == (24, 1024, 0):
                    assert (q, kept) == (295, 11)
                if case == (2, 7, 150):
                    assert pairs == 7 * q - 28 and strong > 0 and kept > q // 2  # a band of 7: most sites stay
    bm.free()


# ---- row widths: 8 and 32 dwords in registers, the generic path, the documented maximum; band 65 = two kept words --------------------

@pytest.mark.parametrize("n", (200, 1000, 2100, 4096))
def test_row_widths(ctx, n):
    from impop_amd import _lib
    assert _lib.LDBAND_MAX_N == 4096
    rng = np.random.default_rng(31150 + n)
    W = 700
    m01 = hc.founder_matrix(rng, n, W, p_site=0.5, p_flip=1e-3)
    wins = [(0, W), (37, 333), (300, 301), (650, W)]
    case = (2, 65, 0)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    ref = ref_of(m01, None, wins, case)
    assert ref[0]["n_qualifying"][0] > 256 and ref[0]["n_strong"][0] > 0 and 0 < ref[0]["n_kept"][0] < ref[0]["n_qualifying"][0]
    bc.assert_matches(scan(bm, wins, None, case), ref, n)
    bm.free()


# ---- agreement with shipped code -----------------------------------------------------------------------------------------------------

def test_a_band_over_the_whole_window_is_the_ld_scan(ctx):
    n = 465
    m01 = bc.planted_matrix(np.random.default_rng(31000 + n), n, p_flip=1e-3)
    wins = [w for w in bc.window_list() if w[1] - w[0] <= 640]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    rec, _, tab = scan(bm, wins, None, (2, 1024, 0))
    ld, used = bm.ld_scan(wins, min_mac=2, max_sites=1024, want_sites=True)
    q = rec["n_qualifying"].astype(np.int64)
    assert q.max() > 100 and q.max() <= 1024 and (q == 0).any()
    assert np.array_equal(rec["n_pairs"].astype(np.int64), q * (q - 1) // 2)
    assert np.array_equal(ld["n_used"], rec["n_qualifying"]) and np.array_equal(ld["n_perfect"].astype(np.uint64), rec["n_perfect"])
    assert rec["n_perfect"].sum() >= 3
    for i in range(len(wins)):
        a = int(rec["site_off"][i])
        assert np.array_equal(used[i, :q[i]], tab["coord"][a:a + q[i]]), i
    bm.free()


# ---- positions with irregular gaps: the same columns scattered over a longer matrix ----------------------------------------------------

def _scattered():
    rng = np.random.default_rng(31200)
    n, W = 40, 400
    m01 = hc.founder_matrix(rng, n, W, nf=4, p_site=0.6, p_flip=2e-3)
    pos = np.cumsum(rng.integers(1, 40, size=W)).astype(np.int64)
    wide = np.zeros((n, int(pos[-1]) + 1), dtype=np.uint8)
    wide[:, pos] = m01
    return m01, pos, np.ascontiguousarray(wide)


def test_irregular_positions_move_bins_and_max_dist_membership(ctx):
    m01, pos, wide = _scattered()
    W = m01.shape[1]
    case, kw = (2, 12, 60), dict(bin_width=25, n_bins=8)
    narrow_ref = ref_of(m01, None, [(0, W)], case, **kw)
    spread_ref = ref_of(m01, None, [(0, W)], case, pos=pos, **kw)
    assert spread_ref[0]["n_pairs"][0] < narrow_ref[0]["n_pairs"][0] and not np.array_equal(spread_ref[1]["pairs"], narrow_ref[1]["pairs"])
    spread_ref[0]["n_sites"][0] = wide.shape[1]
    bm = ctx.upload_dense(wide, keep_hap_major=False)
    got = scan(bm, [(0, wide.shape[1])], None, case, **kw)
    bc.assert_matches(got, spread_ref, "scattered")
    cm = bm.compact()
    again = scan(cm, [(0, wide.shape[1])], None, case, **kw)
    for a, b in zip(got, again):
        assert a.tobytes() == b.tobytes()
    cm.free()
    bm.free()
    nm = ctx.upload_dense(m01, keep_hap_major=False)
    bc.assert_matches(scan(nm, [(0, W)], None, case, **kw), narrow_ref, "narrow")
    nm.free()


def test_flipping_alleles_changes_nothing_but_carriers(ctx):
    n = 465
    m01 = bc.planted_matrix(np.random.default_rng(31000 + n), n, p_flip=1e-3)
    flipped = m01.copy()
    flipped[:, np.random.default_rng(31300).random(S) < 0.4] ^= 1
    wins = bc.window_list()[:12]
    a_bm, b_bm = ctx.upload_dense(m01, keep_hap_major=False), ctx.upload_dense(np.ascontiguousarray(flipped), keep_hap_major=False)
    a, b = scan(a_bm, wins, None, (2, 70, 0)), scan(b_bm, wins, None, (2, 70, 0))
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for k in bc.SITE_FIELDS:
        assert np.array_equal(a[2][k], b[2][k]) == (k != "carriers"), k
    a_bm.free()
    b_bm.free()


# ---- capacity and refusals -----------------------------------------------------------------------------------------------------------

def _raw(bm, wins, table, capacity, want_bins=True, **kw):
    """the C call itself -> (rc, records, bins, n_site_rows)"""
    import impop_amd
    from impop_amd._lib import LdbandBin, LdbandParams, LdbandSite, LdbandStats, Window
    from impop_amd.engine import make_windows
    p = dict(min_mac=2, band_sites=20, n_bins=16, thr_num=1, thr_den=5, bin_width=50, max_dist=0, max_chunk_bytes=0)
    p.update(kw)
    w = make_windows(wins)
    prm = LdbandParams(C.sizeof(LdbandParams), p["min_mac"], p["band_sites"], p["n_bins"], p["thr_num"], p["thr_den"], p["bin_width"],
                       p["max_dist"], p["max_chunk_bytes"])
    rec = np.zeros(len(w), dtype=impop_amd.LDBAND_DTYPE)
    bins = np.zeros((len(w), p["n_bins"]), dtype=impop_amd.LDBAND_BIN_DTYPE)
    rows = C.c_uint64(0xDEAD)
    rc = bm.ctx._lib.impop_ldband_scan(bm.ctx.handle, bm.handle, w.ctypes.data_as(C.POINTER(Window)), len(w), None, C.byref(prm),
                                       rec.ctypes.data_as(C.POINTER(LdbandStats)), bins.ctypes.data_as(C.POINTER(LdbandBin)) if want_bins else None,
                                       table.ctypes.data_as(C.POINTER(LdbandSite)) if table is not None else None, capacity, C.byref(rows))
    return rc, rec, bins, rows.value


def test_a_null_or_short_site_table_is_left_alone(ctx):
    import impop_amd
    rng = np.random.default_rng(31400)
    n, W = 64, 600
    m01 = hc.founder_matrix(rng, n, W, p_site=0.5, p_flip=2e-3)
    wins = [(0, 300), (100, 101), (250, 600), (5, 5)]
    ref = bc.reference(m01, None, wins, 2, 20, 0, 50, 16, (1, 5))
    total = int(ref[0]["n_qualifying"].sum())
    assert total > 300
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    rc, rec, bins, rows = _raw(bm, wins, None, 0)
    assert rc == 0 and rows == total
    bc.assert_matches((rec, bins, _fill(bm, wins, total)), ref, "null table, then one that fits")  # records and bins of the NULL call
    short_tab = np.frombuffer(bytearray(b"\xab" * (32 * total)), dtype=impop_amd.LDBAND_SITE_DTYPE)
    rc2, rec2, bins2, rows2 = _raw(bm, wins, short_tab, total - 1)
    assert rc2 == 0 and rows2 == total and rec2.tobytes() == rec.tobytes() and bins2.tobytes() == bins.tobytes()
    assert short_tab.tobytes() == b"\xab" * (32 * total)  # untouched
    rc3, rec3, _, rows3 = _raw(bm, wins, None, 0, want_bins=False)
    assert rc3 == 0 and rows3 == total and rec3.tobytes() == rec.tobytes()
    rc4, _, _, rows4 = _raw(bm, [], None, 0)
    assert rc4 == 0 and rows4 == 0
    bm.free()


def _fill(bm, wins, total):
    import impop_amd
    tab = np.zeros(total, dtype=impop_amd.LDBAND_SITE_DTYPE)
    rc, _, _, rows = _raw(bm, wins, tab, total)
    assert rc == 0 and rows == total
    return tab


def test_errors_and_empty_input(ctx):
    import impop_amd
    from impop_amd import ImpopError
    rng = np.random.default_rng(31500)
    n, W = 40, 300
    m01 = hc.founder_matrix(rng, n, W, p_flip=2e-3)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    ok = [(10, 100)]
    cases = [(ok, {"mask_p": np.zeros(n, np.uint8)}), (ok, {"min_mac": 0}), (ok, {"band_sites": 0}), (ok, {"band_sites": 1025}),
             (ok, {"n_bins": 0}), (ok, {"n_bins": 4097}), (ok, {"bin_width": 0}), (ok, {"threshold": (1, 0)}), (ok, {"threshold": (1, 65536)}),
             (ok, {"threshold": (6, 5)}), ([(100, 10)], {}), ([(10, W + 1)], {})]
    for wins, kw in cases:
        with pytest.raises(ImpopError) as ei:
            bm.ldband_scan(wins, **kw)
        assert ei.value.code == E_INVALID, (wins, kw)
    from impop_amd._lib import LdbandParams
    rc, _, _, rows = _raw(bm, ok, None, 0)
    assert rc == 0
    w = impop_amd.make_windows(ok)
    bad = LdbandParams(C.sizeof(LdbandParams) - 8, 2, 20, 16, 1, 5, 50, 0, 0)
    rec = np.zeros(1, dtype=impop_amd.LDBAND_DTYPE)
    from impop_amd._lib import LdbandStats, Window
    assert bm.ctx._lib.impop_ldband_scan(bm.ctx.handle, bm.handle, w.ctypes.data_as(C.POINTER(Window)), 1, None, C.byref(bad),
                                         rec.ctypes.data_as(C.POINTER(LdbandStats)), None, None, 0, None) == E_INVALID
    # the limits themselves are taken
    for kw in ({"band_sites": 1}, {"band_sites": 1024}, {"n_bins": 1}, {"n_bins": 4096}, {"threshold": (0, 1)}, {"threshold": (65535, 65535)}):
        got = bm.ldband_scan([(0, W)], want_bins=True, want_sites=True, **kw)
        p = dict(band_sites=256, n_bins=100, threshold=(1, 5))
        p.update(kw)
        bc.assert_matches(got, bc.reference(m01, None, [(0, W)], 2, p["band_sites"], 0, 1000, p["n_bins"], p["threshold"]), kw)
    assert not bm.ldband_scan([(0, W)], threshold=(65535, 65535))["n_strong"].any()
    empty = bm.ldband_scan([])
    assert empty.dtype == impop_amd.LDBAND_DTYPE and len(empty) == 0
    rec, bins, tab = bm.ldband_scan([], **FULL)
    assert len(rec) == 0 and bins.shape == (0, 100) and tab.shape == (0,) and tab.dtype == impop_amd.LDBAND_SITE_DTYPE
    bm.free()


def test_a_window_over_the_budget_is_refused_before_anything_is_written(ctx):
    from impop_amd import ImpopError
    rng = np.random.default_rng(31600)
    n, W = 40, 600
    m01 = hc.founder_matrix(rng, n, W, p_site=0.6, p_flip=2e-3)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    wins = [(0, 10), (0, W)]
    q = bc.reference(m01, None, wins, 2, 20, 0, 50, 16, (1, 5))[0]["n_qualifying"]
    slot = 4 * 2 + 8 * 1 + 32  # a row of 2 dwords, one word of strong mask, a site row
    assert int(q[0]) * slot <= 4096 < int(q[1]) * slot
    rc, rec, bins, rows = _raw(bm, wins, None, 0, max_chunk_bytes=4096)
    assert rc == E_UNSUPPORTED and rows == 0xDEAD and not rec.view(np.uint8).any() and not bins.view(np.uint8).any()
    with pytest.raises(ImpopError) as ei:
        bm.ldband_scan(wins, band_sites=20, max_chunk_bytes=4096)
    assert ei.value.code == E_UNSUPPORTED and str(int(q[1])) in str(ei.value) and "4096" in str(ei.value)
    rc, rec, _, rows = _raw(bm, wins[:1], None, 0, max_chunk_bytes=4096)
    assert rc == 0 and rows == int(q[0])
    bm.free()


def test_timers_bracket_the_five_kernel_groups(ctx):
    m01 = bc.planted_matrix(np.random.default_rng(31700), 64)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    wins = [(0, 640), (320, 960), (1000, 1051)]
    ctx.gram_timing(True)
    bm.ldband_scan(wins)
    bm.ldband_scan(wins[:1])
    ms, chunks = ctx.ldband_elapsed()
    ctx.gram_timing(False)
    assert chunks == 2 and len(ms) == 5 and all(t > 0.0 for t in ms)
    bm.free()


# ---- invariance, under IMPOP_TRACE=1 in a child process -----------------------------------------------------------------------------

ROUTE_N = 465
ROUTE_CASE = (2, 70, 400)


def _route_inputs():
    rng = np.random.default_rng(31800)
    m01 = bc.planted_matrix(rng, ROUTE_N)
    weights = rng.integers(1, 9, size=S).astype(np.uint32)
    flags = (rng.random(ROUTE_N) < 0.8).astype(np.uint8)
    return m01, weights, flags, bc.window_list()


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
        out[tag], out[tag + "_bins"], out[tag + "_table"] = res

    m01, weights, flags, wins = _route_inputs()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    keep("default", call("default", lambda: scan(bm, wins, flags, ROUTE_CASE)))
    os.environ["IMPOP_LDBAND_LDS_BINS"] = "0"
    keep("global", call("global", lambda: scan(bm, wins, flags, ROUTE_CASE)))
    os.environ["IMPOP_LDBAND_LDS_BINS"] = "15"  # one fewer than the 16 bins asked for
    keep("global15", call("global15", lambda: scan(bm, wins, flags, ROUTE_CASE)))
    os.environ["IMPOP_LDBAND_LDS_BINS"] = "16"
    keep("lds16", call("lds16", lambda: scan(bm, wins, flags, ROUTE_CASE)))
    del os.environ["IMPOP_LDBAND_LDS_BINS"]
    out["nobins"] = call("nobins", lambda: bm.ldband_scan(wins, mask_p=flags, min_mac=2, band_sites=70, max_dist=400, **COMMON))
    cm = bm.compact()
    keep("compact", call("compact", lambda: scan(cm, wins, flags, ROUTE_CASE)))
    cm.free()
    perm = np.random.default_rng(1).permutation(len(wins))
    out["perm"] = perm
    keep("permuted", call("permuted", lambda: scan(bm, [wins[k] for k in perm], flags, ROUTE_CASE)))
    cw = _chunk_windows()
    keep("w120", call("w120", lambda: scan(bm, cw, flags, ROUTE_CASE)))
    keep("w30", call("w30", lambda: scan(bm, cw[:30], flags, ROUTE_CASE)))
    keep("chunked", call("chunked", lambda: scan(bm, cw, flags, ROUTE_CASE, max_chunk_bytes=100000)))
    keep("chunked_w", call("chunked_w", lambda: scan(bm, wins, flags, ROUTE_CASE, max_chunk_bytes=50000)))
    bm.free()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    bm.set_site_weights(weights)
    keep("weighted", call("weighted", lambda: scan(bm, wins, flags, ROUTE_CASE)))
    bm.free()
    big = ctx.upload_dense(np.zeros((4097, 200), np.uint8), keep_hap_major=False)
    try:
        call("over", lambda: big.ldband_scan([(0, 200)]))
        out["over"] = np.array([0])
    except ImpopError as exc:
        out["over"] = np.array([exc.code])
    f = np.ones(4097, np.uint8)
    f[0] = 0
    out["subset4096"] = call("subset4096", lambda: big.ldband_scan([(0, 200)], mask_p=f))
    big.free()
    ctx.close()
    np.savez(out_path, **out)


_TRACE = re.compile(r"\[impop_ldband_scan\] (.*)$")


@pytest.fixture(scope="module")
def child():
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
        env.pop("IMPOP_LDBAND_LDS_BINS", None)
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_ldband_scan as t; t._child(sys.argv[1])", path],
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
            trace[cur].append({k: (v if k in ("route", "bins") else int(v)) for k, v in kv.items()})
    return recs, trace


def _triple(recs, tag):
    return recs[tag], recs[tag + "_bins"], recs[tag + "_table"]


def _same(recs, a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(_triple(recs, a), _triple(recs, b)))


def test_trace_line_and_the_two_homes_of_the_decay_counters(child):
    recs, trace = child
    m01, weights, flags, wins = _route_inputs()
    ref = ref_of(m01, flags, wins, ROUTE_CASE)
    bc.assert_matches(_triple(recs, "default"), ref, "default")
    assert (ref[1]["pairs"].sum(axis=0) > 0).sum() >= 8 and ref[0]["n_strong"].sum() > 0
    for tag, home in (("default", "lds"), ("global", "global"), ("global15", "global"), ("lds16", "lds"), ("nobins", "off"), ("compact", "lds")):
        assert len(trace[tag]) == (1 if tag == "nobins" else 2), tag  # a site table costs a sizing call and a filling one
        t = trace[tag][-1]
        assert tag == "nobins" or t == trace[tag][0], tag
        assert set(t) == {"route", "windows", "chunks", "launches", "qualifying", "pairs", "band", "bins", "bytes_streamed"}, t
        assert t["bins"] == home and t["band"] == 70 and t["windows"] == len(wins), (tag, t)
        assert t["pairs"] == int(ref[0]["n_pairs"].sum()) and t["qualifying"] == int(ref[0]["n_qualifying"].sum()), (tag, t)
    for tag in ("global", "global15", "lds16", "compact"):
        assert _same(recs, tag, "default"), tag
    assert recs["nobins"].tobytes() == recs["default"].tobytes()
    assert [trace[t][0]["route"] for t in ("default", "compact", "weighted")] == ["dense", "compact", "dense"]
    assert trace["compact"][0]["bytes_streamed"] < trace["default"][0]["bytes_streamed"]
    # site weights change W and nothing else
    bc.assert_matches(_triple(recs, "weighted"), ref_of(m01, flags, wins, ROUTE_CASE, weights=weights), "weighted")
    assert recs["weighted_table"].tobytes() == recs["default_table"].tobytes() and recs["weighted_bins"].tobytes() == recs["default_bins"].tobytes()


def test_window_order_does_not_change_a_window(child):
    recs, _ = child
    perm = recs["perm"]
    a, b = recs["permuted"].copy(), recs["default"][perm].copy()
    a["site_off"] = b["site_off"] = 0  # the one field that names a window's place in the call
    assert a.tobytes() == b.tobytes() and recs["permuted_bins"].tobytes() == recs["default_bins"][perm].tobytes()
    d, p = recs["default"], recs["permuted"]
    for at, k in enumerate(perm):
        x = recs["permuted_table"][int(p["site_off"][at]):int(p["site_off"][at] + p["n_qualifying"][at])]
        y = recs["default_table"][int(d["site_off"][k]):int(d["site_off"][k] + d["n_qualifying"][k])]
        assert x.tobytes() == y.tobytes(), k


def test_chunking_never_changes_a_byte(child):
    recs, trace = child
    assert trace["w120"][0]["chunks"] == 1 and trace["chunked"][0]["chunks"] >= 3 and trace["chunked_w"][0]["chunks"] >= 3
    assert _same(recs, "chunked", "w120") and _same(recs, "chunked_w", "default")
    n30 = int(recs["w30"]["n_qualifying"].sum())
    assert recs["w120"][:30].tobytes() == recs["w30"].tobytes() and recs["w120_table"][:n30].tobytes() == recs["w30_table"].tobytes()
    a, b = trace["w30"][0], trace["w120"][0]
    assert a["launches"] == b["launches"] == 8  # the counting pass's two and the six of the one chunk, however many windows
    assert trace["chunked"][0]["launches"] == 2 + 6 * trace["chunked"][0]["chunks"]


def test_limit_plus_one_is_refused_before_any_launch(child):
    recs, trace = child
    assert recs["over"].tolist() == [E_UNSUPPORTED] and trace["over"] == []
    r = recs["subset4096"]
    assert len(trace["subset4096"]) == 1 and r["n_members"].tolist() == [4096] and r["n_qualifying"].tolist() == [0]
    assert r["n_sites"].tolist() == [200] and r["n_pairs"].tolist() == [0] and np.isnan(r["mean_r2"]).all()


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def test_cli_tables_are_the_restatement(ctx, tmp_path):
    from impop_amd.matrixio import MatrixFile, save_matrix
    from impop_amd import pack_hap_major
    rng = np.random.default_rng(31900)
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

    def tables(ref, members, bin_width, n_bins):
        rec, bins, tab = ref
        main = ["REGION\tLENGTH\tSAMPLES\tSITES\tQUALIFYING\tPAIRS\tMEAN_R2\tSTRONG\tPERFECT\tKEPT"]
        decay, sites = ["REGION\tBIN\tDIST_FROM\tDIST_TO\tPAIRS\tMEAN_R2\tSTRONG_FRACTION"], ["REGION\tPOS\tCARRIERS\tPARTNERS\tLD_SCORE\tKEPT"]
        kept = set()
        for i, (b, e) in enumerate(rows):
            reg = f"chrT:{origin + b}-{origin + e}"
            main.append("\t".join([reg, str(e - b), str(members), str(e - b)] + [str(int(rec[k][i])) for k in ("n_qualifying", "n_pairs")] +
                                  [fmt(rec["mean_r2"][i])] + [str(int(rec[k][i])) for k in ("n_strong", "n_perfect", "n_kept")]))
            for k in range(n_bins):
                pairs, fx, strong = (int(bins[f][i, k]) for f in bc.BIN_FIELDS)
                decay.append("\t".join([reg, str(k), str(k * bin_width), "NA" if k == n_bins - 1 else str((k + 1) * bin_width - 1), str(pairs),
                                        fmt(float(fx) / (float(pairs) * 1073741824.0) if pairs else float("nan")),
                                        fmt(float(strong) / float(pairs) if pairs else float("nan"))]))
            a = int(rec["site_off"][i])
            for j in range(a, a + int(rec["n_qualifying"][i])):
                sites.append("\t".join([reg, str(origin + int(tab["coord"][j])), str(int(tab["carriers"][j])), str(int(tab["n_partners"][j])),
                                        "%.8f" % (float(int(tab["ld_score_fx"][j])) / 1073741824.0), str(int(tab["kept"][j]))]))
                if tab["kept"][j]:
                    kept.add(origin + int(tab["coord"][j]))
        return tuple("\n".join(t) + "\n" for t in (main, decay, sites, [f"chrT\t{p}" for p in sorted(kept)]))

    def run(extra):
        dp, sp, kp = str(tmp_path / "decay.tsv"), str(tmp_path / "sites.tsv"), str(tmp_path / "keep.txt")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_ldband.py"), "--matrix", mpath, "--bed", bed,
                            "--ldband-decay", dp, "--ldband-site-table", sp, "--ldband-prune-in", kp] + extra,
                           capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout, open(dp).read(), open(sp).read(), open(kp).read()

    want = tables(bc.reference(m01, None, rows, 2, 256, 0, 1000, 100, (2000, 10000)), n, 1000, 100)
    assert "NA" in want[0] and len(want[2].splitlines()) > 100 and 3 < len(want[3].splitlines()) < len(want[2].splitlines())
    assert run([]) == want and run(["--compact"]) == want
    mac = max(1, int(np.ceil(0.1 * 31)))
    opts = ["-u", sub, "--ldband-min-maf", "0.1", "--ldband-sites", "9", "--ldband-max-dist", "40", "--ldband-bin-width", "7", "--ldband-bins", "5",
            "--ldband-r2", "0.3125"]
    assert run(opts) == tables(bc.reference(m01, flags, rows, mac, 9, 40, 7, 5, (3125, 10000)), 31, 7, 5)
    # refused before any file is opened
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_ldband.py"), "--matrix", "/nonexistent", "--bed", "/nonexistent",
                        "--ldband-r2", "0.12345"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and "--ldband-r2" in r.stderr
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_ldband.py"), "--matrix", "/nonexistent", "--bed", "/nonexistent"],
                       capture_output=True, text=True, cwd=ROOT, timeout=120, env=dict(os.environ, WORLD_SIZE="2"))
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr
