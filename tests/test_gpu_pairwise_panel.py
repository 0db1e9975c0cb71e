"""GPU: impop_pairwise_scan_panel — K panels and their K(K-1)/2 pairs from one Gram pass per window.

Expected values never come from the call under test: panels are compared, byte for byte, with impop_pairwise_scan(mask_p = the
panel) (the same pica2 kernel and the same finalize arithmetic) and with the oracle's pica2 on the panel's sub-matrix; pairs with
oracle.hfst and with impop_pairwise_scan(mask_a, mask_b) under the tolerance policy of INTEGRATION.md §4 (stat_close): the panel
kernel sums the same terms in another order than the two-class kernel.  Where the call takes the general route (n > 512, dice)
the pairs are launch_hfst's own and must equal pairwise_scan's byte for byte.

s_p is defined for s_scope 1 only (the header: one streaming pass per panel; s_scope 0 takes S = s_all from the site bitmap and
runs no such pass), so the reference-panel test compares pi / pi_site / n_groups / tajima_d at s_scope 0 AND all five fields,
s_p included, at s_scope 1 — each against pairwise_scan at the same s_scope."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import panel_cases
from conftest import ROOT, rel_close, stat_close
from panel_cases import KW, blob, founders, panels, reference_inputs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FST_KEYS = ("fst", "pi_a", "pi_b", "pi_xy", "dxy", "da")


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    assert c.device_name().startswith("gfx950")
    yield c
    c.close()


def _sim(oracle, bits, n, a, b, kind=0):
    return oracle.identity(oracle.pairwise_counts(bits, n, a, b), b - a, kind) if b > a else np.ones((n, n))


def check_call(bm, oracle, m, pops, wins, kind="match", thr=0.999, rd=5, s_scope=0):
    """one panel call against pairwise_scan per panel / per pair and against the oracle; returns its three arrays"""
    n, K = m.shape[0], len(pops)
    kw = dict(kind=kind, threshold=thr, round_digits=rd)
    bits = oracle.pack_hap_major(m)
    pan, pairs, pw = bm.pairwise_scan_panel(wins, pops, s_scope=s_scope, **kw)
    assert pan.shape == (len(wins), K) and pairs.shape == (len(wins), K * (K - 1) // 2) and pw.shape == (len(wins),)
    sims = [_sim(oracle, bits, n, a, b, 1 if kind == "dice" else 0) for a, b, _ in wins]
    for wi, (a, b, _) in enumerate(wins):
        c = m[:, a:b].sum(0)
        assert int(pw[wi]["n_sites"]) == b - a and int(pw[wi]["s_all"]) == (int(((c > 0) & (c < n)).sum()) if s_scope != 2 else 0), wi
    for k in range(K):
        one = bm.pairwise_scan(wins, pops[k], None, None, s_scope=s_scope, **kw)
        for key in ("pi", "pi_site", "tajima_d", "n_groups") + (("s_p",) if s_scope == 1 else ()):
            assert pan[:, k][key].tobytes() == one[key].tobytes(), (k, key, pan[:, k][key], one[key])
        assert (pan[:, k]["n_members"] == int(pops[k].sum())).all() and (pan[:, k]["reserved"] == 0).all()
        sel = np.nonzero(pops[k])[0]
        for wi, (a, b, L) in enumerate(wins):
            pi, ps, _, G = oracle.pica2(sims[wi][np.ix_(sel, sel)], thr, L if L else None, rd)
            assert int(pan[wi, k]["n_groups"]) == G, (k, wi)
            assert rel_close(float(pan[wi, k]["pi"]), pi, 1e-9, 0.0) and rel_close(float(pan[wi, k]["pi_site"]), ps, 1e-9, 0.0), (k, wi)
            if s_scope != 2 and len(sel) >= 2 and L:
                S = float(pan[wi, k]["s_p"]) if s_scope == 1 else float(pw[wi]["s_all"])
                D, _ = oracle.tajimas_d(len(sel), S, oracle.py_round(float(pan[wi, k]["pi_site"]), 8))
                assert float(pan[wi, k]["tajima_d"]) == D or (D != D and np.isnan(pan[wi, k]["tajima_d"])), (k, wi, D)
    p = 0
    for k in range(K):
        for l in range(k + 1, K):
            two = bm.pairwise_scan(wins, None, pops[k], pops[l], s_scope=2, **kw)
            for wi, (a, b, L) in enumerate(wins):
                h, _ = oracle.hfst(sims[wi], pops[k], pops[l], L if L else None, rd)
                for key in FST_KEYS:
                    got = float(pairs[wi, p][key])
                    assert stat_close(key, got, h[key], h["dxy"]), ("oracle", k, l, wi, key, got, h[key])
                    assert stat_close(key, got, float(two[wi][key]), float(two[wi]["dxy"])), ("pairwise_scan", k, l, wi, key, got)
            p += 1
    return pan, pairs, pw


def test_reference_panels(ctx, oracle):
    m, pops, wins = reference_inputs()
    assert sum(int(f.sum()) for f in pops) == 460 and m.shape == (465, 4000)
    bm = ctx.upload_dense(m, keep_hap_major=True)
    a = check_call(bm, oracle, m, pops, wins, s_scope=0)
    b = check_call(bm, oracle, m, pops, wins, s_scope=1)
    assert blob(a[1]).tobytes() == blob(b[1]).tobytes()  # the pairs do not depend on s_scope
    again = bm.pairwise_scan_panel(wins, pops, **KW)
    assert blob(a).tobytes() == blob(again).tobytes()
    # the empty window: identity 1 everywhere, one group per panel
    assert (a[0][2]["pi"] == 0).all() and (a[0][2]["n_groups"] == 1).all()
    bm.free()


@pytest.mark.parametrize("n,sizes,seed", [(150, [70, 61], 1), (300, [40, 33, 50, 21, 37, 45, 30, 36], 2), (40, [11, 9, 13], 3),
                                          (512, [64, 64, 1, 383], 4)],
                         ids=["K2", "K8", "word0", "aligned+single"])
def test_class_bookkeeping_edges(ctx, oracle, n, sizes, seed):
    rng = np.random.default_rng(seed)
    W = 1500
    m = founders(rng, n, W, pf=0.01, pp=0.002)
    if n == 512:  # word-aligned class boundaries: the panels are ranges of the haplotype order, not a permutation
        pops, o = [], 0
        for s in sizes:
            f = np.zeros(n, np.uint8); f[o: o + s] = 1; o += s
            pops.append(f)
    else:
        pops = panels(rng, n, sizes)
    wins = [(0, W, W), (37, 1111, 0), (700, 700, 9)]
    bm = ctx.upload_dense(m, keep_hap_major=True)
    pan, pairs, _ = check_call(bm, oracle, m, pops, wins, thr=0.995, rd=4)
    if n == 512:  # the one-member panel: no pair inside it
        assert (pan[:, 2]["pi"] == 0).all() and (pan[:, 2]["n_groups"] == 1).all() and np.isnan(pan[:, 2]["tajima_d"]).all()
        assert (pairs[:, 1]["pi_b"] == 0).all() and (pairs[:, 3]["pi_b"] == 0).all() and (pairs[:, 5]["pi_a"] == 0).all()
        bits = oracle.pack_hap_major(m)
        _, cnt = oracle.hfst(_sim(oracle, bits, n, 0, W), pops[0], pops[2], W, 4)
        assert int(cnt[2]) == 0 and int(cnt[4]) == 64  # within-pair count 0, 64 x 1 pairs between
    bm.free()


def test_s_scope_1_takes_the_streaming_scan(ctx, oracle):
    rng = np.random.default_rng(8)
    n, W = 130, 3000
    m = founders(rng, n, W, pf=0.01, pp=0.003)
    pops = panels(rng, n, [50, 30, 44])
    wins = [(0, W, W), (5, 2999, 2994), (64, 128, 64), (10, 10, 3)]
    bm = ctx.upload_dense(m, keep_hap_major=True)
    pan, _, pw = check_call(bm, oracle, m, pops, wins, s_scope=1)
    for k in range(3):
        s = bm.scan(wins, pops[k], None, None)
        assert (pan[:, k]["s_p"] == s["s_p"]).all() and (pw["s_all"] == s["s_all"]).all()
        assert (pan[:, k]["s_p"] <= pw["s_all"]).all()
    p2, _, w2 = bm.pairwise_scan_panel(wins, pops, s_scope=2, **KW)
    assert np.isnan(p2["tajima_d"]).all() and (p2["s_p"] == 0).all() and (w2["s_all"] == 0).all()
    assert p2["pi"].tobytes() == pan["pi"].tobytes()
    no_pairs = bm.pairwise_scan_panel(wins, pops, want_pairs=False, **KW)
    assert no_pairs[1].shape == (4, 0) and no_pairs[0]["pi"].tobytes() == pan["pi"].tobytes()
    bm.free()


def test_errors(ctx):
    import impop_amd
    from impop_amd import _lib
    import ctypes as C
    rng = np.random.default_rng(1)
    n, W = 80, 500
    m = founders(rng, n, W)
    pops = panels(rng, n, [20, 25, 30])
    bm = ctx.upload_dense(m, keep_hap_major=True)
    wins = [(0, W, W), (10, 200, 190)]

    def code(p, **kw):
        with pytest.raises(impop_amd.ImpopError) as e:
            bm.pairwise_scan_panel(wins, p, **dict(KW, **kw))
        return e.value.code
    both = pops[0] | pops[1]
    assert code([pops[0], both]) == _lib.E_INVALID                        # overlapping panels
    assert code([pops[0], np.zeros(n, np.uint8)]) == _lib.E_INVALID       # an empty panel
    assert code([pops[0]]) == _lib.E_INVALID                              # K = 1
    nine = panels(rng, n, [8] * 9)
    assert code(nine) == _lib.E_INVALID                                   # K = 9
    packed = np.concatenate([impop_amd.pack_mask(p, n) for p in pops]).astype(np.uint64)
    w = impop_amd.make_windows(wins)
    prm = _lib.PairwiseParams(C.sizeof(_lib.PairwiseParams), 0, 0.999, 5, 0, 0, 1)  # fst_method 1
    pan = np.zeros((2, 3), dtype=impop_amd.PANEL_DTYPE)
    rc = ctx._lib.impop_pairwise_scan_panel(ctx.handle, bm.handle, w.ctypes.data_as(C.POINTER(_lib.Window)), 2,
                                            packed.ctypes.data_as(C.POINTER(C.c_uint64)), 3, C.byref(prm),
                                            pan.ctypes.data_as(C.POINTER(_lib.PanelStats)), None, None)
    assert rc == _lib.E_UNSUPPORTED and b"fst_method" in ctx._lib.impop_last_error()
    # the device error word: the call that sees it fails once, the next one works
    good = bm.pairwise_scan_panel(wins, pops, **KW)
    _lib.check(ctx._lib.impop_debug_raise_device_error(ctx.handle, 1))
    assert code(pops) == _lib.E_INTERNAL
    after = bm.pairwise_scan_panel(wins, pops, **KW)
    assert blob(good).tobytes() == blob(after).tobytes()
    bm.free()


def _child(mode, path, **extra):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, HERE]), **extra)
    r = subprocess.run([sys.executable, os.path.join(HERE, "panel_cases.py"), mode, path], capture_output=True, text=True, env=env, cwd=ROOT,
                       timeout=300)
    assert r.returncode == 0, (mode, extra, r.stderr[-3000:])
    return r.stderr, dict(np.load(path))


def test_one_gram_and_routes(ctx):
    """IMPOP_TRACE=1 is read once per process: the calls run in a child (tests/panel_cases.py trace_calls, which also holds the
    general route's pairs against pairwise_scan byte for byte); the parent reads the lines between the markers."""
    with tempfile.TemporaryDirectory() as td:
        err, got = _child("trace", os.path.join(td, "t.npz"), IMPOP_TRACE="1")

    def part(a, b):
        return err.split(f"@@{a}\n", 1)[1].split(f"@@{b}\n", 1)[0].splitlines()
    gram = lambda lines: [ln for ln in lines if ln.startswith("[impop_gram]")]  # noqa: E731
    route = lambda lines: [ln for ln in lines if ln.startswith("[impop_pairwise_scan_panel] pops=")]  # noqa: E731
    one, pan = part("pairwise", "panel"), part("panel", "dice")
    assert len(gram(one)) >= 1 and gram(pan) == gram(one), (gram(one), gram(pan))  # as many Gram launches, and the same ones
    assert route(pan) == ["[impop_pairwise_scan_panel] pops=5 pairs=10 route=small"] and not route(one)
    assert route(part("dice", "end")) == ["[impop_pairwise_scan_panel] pops=5 pairs=10 route=general"]
    assert route(part("n513", "end513")) == ["[impop_pairwise_scan_panel] pops=3 pairs=3 route=general"]
    # the trace changes no record
    m, pops, _ = reference_inputs()
    bm = ctx.upload_dense(m, keep_hap_major=True)
    wins = [(k * 300 + k % 7, k * 300 + 300 - (k % 5) * 37, 300) for k in range(12)]
    assert blob(bm.pairwise_scan_panel(wins, pops, **KW)).tobytes() == got["reference12"].tobytes()
    bm.free()


@pytest.fixture(scope="module")
def front(ctx):
    return panel_cases.front_cases(ctx)


def test_inherited_front_end(front):
    same = lambda a, b: front[a].tobytes() == front[b].tobytes()  # noqa: E731
    assert same("sliding", "sliding_each")          # shared segments (the SEG instantiations) == every window on its own
    assert same("tiling", "tiling_again") and same("big", "big_again")  # two calls, identical bytes
    assert same("compact_sliding", "sliding") and same("compact_tiling", "tiling")
    assert same("weighted", "expanded")             # node lengths as weights == the bp-expanded matrix
    assert same("weighted_compact_S", "weighted_S")
    assert not same("tiling", "tiling_scope1")      # (s_p and D differ: the cases are not trivially alike)


@pytest.mark.parametrize("env", [{"IMPOP_PAIRWISE_CHUNK": "3"}, {"IMPOP_GRAM_U16": "0"}], ids=["chunks-of-3", "int32-counts"])
def test_front_end_switches_change_no_record(front, env):
    """several chunks per call (the switch test_pairwise_scan_in_several_chunks' siblings use), and int32 counts where uint16 would fit"""
    with tempfile.TemporaryDirectory() as td:
        _, got = _child("front", os.path.join(td, "f.npz"), **env)
    assert sorted(got) == sorted(front)
    for name in front:
        assert got[name].tobytes() == front[name].tobytes(), (env, name)


def test_big_window_against_pairwise_scan(ctx, oracle):
    """a window of >= 65536 sites: 32-bit counts in the small kernels"""
    rng = np.random.default_rng(65)
    n, W = 24, 66000
    m = founders(rng, n, W, pf=0.002, pp=0.0004)
    pops = panels(rng, n, [9, 7, 6])
    bm = ctx.upload_dense(m, keep_hap_major=True)
    check_call(bm, oracle, m, pops, [(0, W, W), (300, 65900, 0)])
    bm.free()


def test_driver_panel_tables(tmp_path):
    from impop_amd import matrixio
    rng = np.random.default_rng(12)
    n, W = 24, 5000
    m = founders(rng, n, W, nf=4, pf=0.01, pp=0.002)
    names = [f"S{i // 2:03d}#{i % 2 + 1}#chr9:{1000}-{1000 + W}" for i in range(n)]
    matrixio.save_matrix(str(tmp_path / "m.npz"), matrixio.from_dense(m, names, origin=1000, contig="CHM13#0#chr9"))
    (tmp_path / "w.bed").write_text("chr9\t1000\t3000\nchr9\t3000\t6000\nCHM13#0#chr9\t2000\t2500\tname\n")
    (tmp_path / "A.txt").write_text("S000\nS001_hap1_hprc_r2\nS002#2\nS003\n")   # 4 lines, 6 haplotypes: D uses n = 4
    (tmp_path / "B.txt").write_text("S005#1\nS005#2\nS006#1\nS006#2\nS007#1\n")
    (tmp_path / "C.txt").write_text("S008#1\nS009#2\nS010#1\nS010#2\nS011#1\nS011#2\n")
    scan = os.path.join(ROOT, "scripts", "impop_scan.py")
    base = [sys.executable, scan, "--matrix", str(tmp_path / "m.npz"), "--bed", str(tmp_path / "w.bed")]
    lists = [str(tmp_path / f"{x}.txt") for x in "ABC"]

    def run(*extra):
        r = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout.strip().split("\n"), r.stderr
    got, err = run("--format", "tajd", "--panel", *lists)
    assert "sample list A has 4 lines but selects 6 haplotypes" in err
    want = []
    for x, f in zip("ABC", lists):
        want += [f"# {x}"] + run("--format", "tajd", "-l", f)[0]
    assert got == want
    got, _ = run("--format", "hfst", "-r", "5", "--panel", *lists)
    want = []
    for i in range(3):
        for j in range(i + 1, 3):
            want += [f"# {'ABC'[i]}-vs-{'ABC'[j]}"] + run("--format", "hfst", "-r", "5", "-A", lists[i], "-B", lists[j])[0]
    assert got == want
