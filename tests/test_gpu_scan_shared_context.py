"""Scan plans that share one context, launched eagerly and replayed from captured graphs (run with -m gpu on an MI355X).

Every plan finalizes with Tajima's constants for ITS |P|.  A plan owns them, so any number of plans and graphs may share a
context: whatever was created, launched, captured or called on the context in between, a launch and a replay of a plan write
that plan's records.  A captured launch is the plan's two kernels, the tile scan and the finalize: two graph nodes, always.

Reference, for every launch and replay checked here: the records are byte-identical to BitMatrix.scan(...) with the same
arguments on a fresh Context, and each one is compared with the CPU oracle as test_gpu_parity.py does (integers exact, doubles
to its REL = 1e-9 with its NaN rule; on the crafted and the weighted matrix Fst and Da with the floors of the tolerance policy,
conftest.stat_close, as the tests of those matrices do).  The oracle is the judge.  The inputs are those of
shared_context_cases.py, which test_scan_shared_context_host.py shows to tell the constants of the subset sizes apart.

A test goes through its whole call sequence and reports every mismatch and node count at the end, so that one run shows all
of what a build gets wrong."""
import os

import numpy as np
import pytest

import hip_capture
import shared_context_cases as sc
from conftest import rel_close, stat_close
from shared_context_cases import Spec
from test_gpu_parity import REL

pytestmark = pytest.mark.gpu

RECORD = 128  # bytes of one impop_window_stats


def _upload(ctx, kind):
    """-> (the matrix plans are made on, everything to free)"""
    if kind == "weighted":  # set_site_weights + compact: plans run scan_tiles_anyn_kernel with the weights
        m, w = sc.nodes()
        bn = ctx.upload_dense(m, keep_hap_major=False)
        bn.set_site_weights(w)
        cm = bn.compact()
        assert cm.n_site < sc.K_NODES
        return cm, [cm, bn]
    bm = ctx.upload_dense(sc.matrix(kind), keep_hap_major=kind == "small")  # the all-pairs calls need the haplotype-major copy
    return bm, [bm]


def _scan_args(spec):
    A, B = sc.masks_ab()
    return (sc.windows(spec), sc.mask_p(spec.psize), A, B), dict(d_pi_mode=spec.d_pi_mode, s_scope=spec.s_scope, tile_blocks=spec.tile_blocks)


_REF = {}


def _ref(spec):
    """BitMatrix.scan with the plan's arguments on a fresh Context: once, shared, unchanged; compared with the oracle here"""
    key = spec._replace(digest=False)  # scan() is a one-shot plan, which takes no digest
    if key not in _REF:
        import impop_amd
        c = impop_amd.Context(0)
        bm, owned = _upload(c, spec.kind)
        args, kw = _scan_args(spec)
        got = bm.scan(*args, **kw)
        for m in owned:
            m.free()
        c.close()
        bad = _against_oracle(got, spec)
        assert not bad, bad[:4]
        _REF[key] = got
    return _REF[key]


def _against_oracle(got, spec):
    """-> the fields that miss the oracle's, as (window, field, got, want)"""
    bad = []
    policy = spec.kind in ("crafted", "weighted")
    for i, want in enumerate(sc.want(spec)):
        for k in sc.INT_KEYS:
            if int(got[i][k]) != int(want[k]):
                bad.append((i, k, int(got[i][k]), int(want[k])))
        for k in sc.DBL_KEYS:
            g, w = float(got[i][k]), float(want[k])
            ok = stat_close(k, g, w, float(want["dxy"]), REL) if policy else rel_close(g, w, REL, 1e-300)
            if not ok:
                bad.append((i, k, g, w))
    return bad


class _Out:
    """a torch device buffer a plan launches into: zeroed before a launch, read after a synchronisation"""

    def __init__(self, shared, plan):
        import torch
        self.shared, self.n = shared, plan.n_windows
        self.t = torch.zeros(max(self.n, 1) * RECORD, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def zero(self):
        import torch
        self.shared.sync()
        self.t.zero_()
        torch.cuda.synchronize()

    def read(self):
        from impop_amd.engine import STATS_DTYPE
        self.shared.sync()
        return np.frombuffer(self.t.cpu().numpy().tobytes(), dtype=STATS_DTYPE)[: self.n]


class Shared:
    """one context on a capture stream; the matrices, plans, buffers and graphs of a test all live on it"""

    def __init__(self):
        import impop_amd
        self.cs = hip_capture.CaptureStream()
        self.ctx = impop_amd.Context(0, stream=self.cs.handle)
        self.mats, self.owned, self.plans, self.graphs, self.problems = {}, [], [], [], []

    def sync(self):
        self.ctx.synchronize()

    def matrix(self, kind):
        if kind not in self.mats:
            self.mats[kind], owned = _upload(self.ctx, kind)
            self.owned += owned
        return self.mats[kind]

    def plan(self, spec):
        args, kw = _scan_args(spec)
        bm = self.matrix(spec.kind)
        env = {"IMPOP_SCAN_WAVE_TILES": "1", "IMPOP_SCAN_DIGEST": "1"} if spec.digest else {}
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)  # read where the plan is made
        try:
            pl = bm.plan(*args, **kw)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        self.plans.append(pl)
        assert bool(pl.digest_info()["on"]) == spec.digest, (spec, pl.digest_info())
        # the finalize variant the list is for, through the tile count of the single-window plans
        if spec.windows == "w64":
            assert pl.n_tiles <= 2 * 64, pl.n_tiles
        elif spec.windows == "mid":
            assert 48 < pl.n_tiles <= 2048, pl.n_tiles
        elif spec.windows == "big":
            assert pl.n_tiles > 2048, pl.n_tiles
        return pl

    def out(self, plan):
        return _Out(self, plan)

    def capture(self, plan, out, tag):
        g = self.cs.capture(lambda: plan.launch(out.ptr))
        self.graphs.append(g)
        if g.n_nodes != 2:
            self.problems.append((tag, "graph nodes", g.n_nodes, 2))
        return g

    def check(self, got, spec, tag):
        """got against the fresh context's records, byte for byte, and against the oracle's"""
        ref = _ref(spec)
        if got.tobytes() != ref.tobytes():
            i = next(i for i in range(len(ref)) if got[i].tobytes() != ref[i].tobytes())
            self.problems.append((tag, "not the fresh context's bytes", "window", i, "tajima_d got", float(got[i]["tajima_d"]),
                                  "want", float(ref[i]["tajima_d"])))
        bad = _against_oracle(got, spec)
        if bad:
            self.problems.append((tag, "oracle", len(bad), "fields; first", bad[0]))

    def launch_checked(self, plan, out, spec, tag):
        out.zero()
        plan.launch(out.ptr)
        self.check(out.read(), spec, tag)

    def replay_checked(self, graph, out, spec, tag):
        out.zero()
        graph.replay()
        self.check(out.read(), spec, tag)

    def verdict(self):
        assert not self.problems, "\n".join(str(p) for p in self.problems)

    def close(self):
        self.sync()
        for g in self.graphs:
            g.destroy()
        for pl in self.plans:
            pl.destroy()
        for m in self.owned:
            m.free()
        self.ctx.close()
        self.cs.destroy()


@pytest.fixture
def shared():
    s = Shared()
    assert s.ctx.device_name().startswith("gfx950")
    yield s
    s.close()


@pytest.fixture(scope="module", autouse=True)
def _drop_the_matrices():
    yield
    _REF.clear()
    for f in (sc.matrix, sc.nodes, sc._packed, sc.want):
        f.cache_clear()


def _pair_specs(pair):
    return Spec("small", "w64", pair[0]), Spec("small", "w64", pair[1])


def _pairwise_d(bm, psize):
    """tajima_d of impop_pairwise_scan on the small window list, subset of psize, S over all rows"""
    A, B = sc.masks_ab()
    return bm.pairwise_scan(sc.WINDOWS["pw"], sc.mask_p(psize), A, B, threshold=0.99, round_digits=4, s_scope=0)["tajima_d"].copy()


_PAIRWISE_REF = {}


def _pairwise_ref(psize):
    """the same call on a fresh context"""
    if psize not in _PAIRWISE_REF:
        import impop_amd
        c = impop_amd.Context(0)
        bm, owned = _upload(c, "small")
        _PAIRWISE_REF[psize] = _pairwise_d(bm, psize)
        for m in owned:
            m.free()
        c.close()
    return _PAIRWISE_REF[psize]


@pytest.mark.parametrize("pair", sc.PAIRS)
def test_eager_alternate(shared, pair):
    """A, B, A, B launched back to back with no host synchronisation in between: the stream orders everything a launch needs"""
    sa, sb = _pair_specs(pair)
    A, B = shared.plan(sa), shared.plan(sb)
    seq = ((A, sa), (B, sb), (A, sa), (B, sb))
    outs = [shared.out(pl) for pl, _ in seq]
    shared.sync()
    for (pl, _), o in zip(seq, outs):
        pl.launch(o.ptr)
    shared.sync()
    for k, ((_, spec), o) in enumerate(zip(seq, outs)):
        shared.check(o.read(), spec, ("launch", k))
    shared.verdict()


def _replay_after_other_plan(shared, sa, sb):
    A = shared.plan(sa)
    oa = shared.out(A)
    shared.launch_checked(A, oa, sa, "A eager")
    ga = shared.capture(A, oa, "capture A")
    B = shared.plan(sb)
    ob = shared.out(B)
    shared.launch_checked(B, ob, sb, "B eager")
    for k in range(2):
        shared.replay_checked(ga, oa, sa, ("replay A", k))
    return A, oa, ga, B, ob


@pytest.mark.parametrize("pair", sc.PAIRS)
def test_replay_after_other_plan(shared, pair):
    """A captured; B created and launched on the same context; A's replays write A's records"""
    _replay_after_other_plan(shared, *_pair_specs(pair))
    shared.verdict()


def _both_captured(shared, sa, sb):
    A = shared.plan(sa)
    oa = shared.out(A)
    ga = shared.capture(A, oa, "capture A")
    B = shared.plan(sb)
    ob = shared.out(B)
    gb = shared.capture(B, ob, "capture B")
    for k, which in enumerate("ABABBA"):
        g, o, spec = (ga, oa, sa) if which == "A" else (gb, ob, sb)
        shared.replay_checked(g, o, spec, ("replay", k, which))


@pytest.mark.parametrize("pair", sc.PAIRS)
def test_both_captured(shared, pair):
    """A and B each in a graph of its own, replayed A, B, A, B, B, A: every replay writes its plan's records"""
    _both_captured(shared, *_pair_specs(pair))
    shared.verdict()


@pytest.mark.parametrize("pair", sc.PAIRS)
def test_captured_not_yet_replayed(shared, pair):
    """a capture runs nothing: an eager all-pairs call with A's |P| issued between A's capture and its first replay gets the
    D of a fresh context, and the replay A's records"""
    sa, sb = _pair_specs(pair)
    A, B = shared.plan(sa), shared.plan(sb)
    oa, ob = shared.out(A), shared.out(B)
    shared.launch_checked(B, ob, sb, "B eager")
    ga = shared.capture(A, oa, "capture A")
    got, want = _pairwise_d(shared.matrix("small"), pair[0]), _pairwise_ref(pair[0])
    if got.tobytes() != want.tobytes():
        shared.problems.append(("pairwise_scan tajima_d", got.tolist(), want.tolist()))
    shared.replay_checked(ga, oa, sa, "replay A")
    shared.verdict()


@pytest.mark.parametrize("pair", sc.PAIRS)
def test_all_pairs_in_between(shared, pair):
    """impop_pairwise_scan and impop_pairwise_scan_panel keep the context's own constants for their subsets and panels; a
    plan's graph replayed after them writes the plan's records"""
    sa, _ = _pair_specs(pair)
    A = shared.plan(sa)
    oa = shared.out(A)
    ga = shared.capture(A, oa, "capture A")
    bm = shared.matrix("small")
    got, want = _pairwise_d(bm, pair[1]), _pairwise_ref(pair[1])
    if got.tobytes() != want.tobytes():
        shared.problems.append(("pairwise_scan tajima_d", got.tolist(), want.tolist()))
    bm.pairwise_scan_panel(sc.WINDOWS["pw"], sc.panels(), threshold=0.99, round_digits=4, want_pairs=False)  # three sizes, one slot
    shared.replay_checked(ga, oa, sa, "replay A")
    shared.verdict()


@pytest.mark.parametrize("pair", sc.PAIRS)
def test_set_masks_changes_nP(shared, pair):
    """set_masks to another |P| refills the plan's constants: eager launches follow it, with another plan launched in between,
    and so does a NEW capture (a graph taken before the call keeps the old subset sizes: capture again)"""
    sy = Spec("small", "w64", pair[1])
    X, Y = shared.plan(Spec("small", "w64", 40)), shared.plan(sy)
    ox, oy = shared.out(X), shared.out(Y)
    A, B = sc.masks_ab()
    for size in (40, 2, 465):
        X.set_masks(sc.mask_p(size), A, B)
        shared.launch_checked(X, ox, Spec("small", "w64", size), ("X eager", size))
        shared.launch_checked(Y, oy, sy, ("Y eager after", size))
    if pair[0] == 465:  # X stands at 465: away and back, nP changes twice
        X.set_masks(sc.mask_p(40), A, B)
    X.set_masks(sc.mask_p(pair[0]), A, B)
    gx = shared.capture(X, ox, "capture X")
    shared.launch_checked(Y, oy, sy, "Y eager after the capture")
    for k in range(2):
        shared.replay_checked(gx, ox, Spec("small", "w64", pair[0]), ("replay X", k))
    shared.verdict()


# The three finalize variants, the wiring (1, 1), a plan with a tile digest, a plan on a weighted compacted matrix, and
# |P| = 1 on either side: plan A of each row against plan B, through both capture scenarios.
VARIANTS = {
    "tpw64": (Spec("small", "mid", 40, tile_blocks=1), Spec("small", "mid", 465, tile_blocks=1)),
    "tpw256": (Spec("big", "big", 40, tile_blocks=1), Spec("big", "big", 465, tile_blocks=1)),
    "tpw256_2": (Spec("big", "big", 465, tile_blocks=1), Spec("small", "w64", 2)),
    "mode11": (Spec("small", "w64", 40, d_pi_mode=1, s_scope=1), Spec("small", "w64", 465)),
    "digest": (Spec("crafted", "crafted", 40, tile_blocks=2, digest=True), Spec("small", "w64", 465)),
    "weighted": (Spec("weighted", "nodes", 40), Spec("small", "w64", 2)),
    "one_then_40": (Spec("small", "w64", 1), Spec("small", "w64", 40)),
    "40_then_one": (Spec("small", "w64", 40), Spec("small", "w64", 1)),
}


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variants_replay_after_other_plan(shared, name):
    _replay_after_other_plan(shared, *VARIANTS[name])
    shared.verdict()


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_variants_both_captured(shared, name):
    _both_captured(shared, *VARIANTS[name])
    shared.verdict()


def test_a_subset_of_one_has_no_d(shared):
    spec = Spec("small", "w64", 1)
    pl = shared.plan(spec)
    o = shared.out(pl)
    shared.launch_checked(pl, o, spec, "eager")
    assert np.isnan(o.read()["tajima_d"]).all()
    shared.verdict()


def test_graph_shape_after_everything_else_ran(shared):
    """one captured launch is the tile kernel and the finalize, two nodes, on a context whose other plans of other sizes and
    all-pairs calls have all run before the capture"""
    specs = [Spec("small", "w64", s) for s in (40, 465, 2, 1)] + [VARIANTS["tpw64"][0], VARIANTS["weighted"][0], VARIANTS["digest"][0]]
    plans = [(shared.plan(s), s) for s in specs]
    outs = [shared.out(pl) for pl, _ in plans]
    for (pl, s), o in zip(plans, outs):
        shared.launch_checked(pl, o, s, ("eager", s))
    _pairwise_d(shared.matrix("small"), 77)
    for (pl, s), o in zip(reversed(plans), reversed(outs)):
        g = shared.capture(pl, o, ("capture", s))
        assert g.n_nodes == 2, (s, g.n_nodes)
        shared.replay_checked(g, o, s, ("replay", s))
    shared.verdict()
