"""The all-pairs path at production batch sizes (run with -m gpu on an MI355X).

A Gram launch with enough (cell, tile-pair) tasks runs without a K-split, and only then with uint16 counts packed two to a dword
and with chained tickets (one wave takes several windows and prefetches the next one's first pairs); chunking by bytes, device
window mapping and the multi-chunk compaction scan also start only at scale.  Every scenario here
  * asserts from the IMPOP_TRACE=1 lines of its launches that it reached the configuration it is about (never by re-deriving
    the launch heuristic in Python: a copy would let the test drift back into testing nothing when the heuristic is retuned),
  * compares sampled windows (chain and chunk edges among them) with the exact oracle,
  * and requires byte-identical records from a process with uint16 counts and chains switched off.
The calls run in child processes (the env switches are read once per process); the parent rebuilds the same inputs from the
same seeds for the oracle."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT, rel_close, stat_close

pytestmark = pytest.mark.gpu

REL = 1e-9
HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN = {"IMPOP_GRAM_U16": "0", "IMPOP_GRAM_CHAIN": "1"}  # int32 counts, one window per ticket
SWITCHES = ("IMPOP_GRAM_U16", "IMPOP_GRAM_CHAIN", "IMPOP_NO_POLARITY", "IMPOP_EPILOGUE_SMALL", "IMPOP_EPILOGUE_FAST")


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    assert c.device_name().startswith("gfx950")
    yield c
    c.close()


# ---- child processes ----------------------------------------------------------------------------------------------

def _worker(name, out_path):
    """Child side: run scenario `name`'s calls, each behind a marker line on stderr, and save every call's records."""
    import impop_amd
    ctx = impop_amd.Context(0)
    recs = {}

    def call(tag, fn):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        recs[tag] = fn()

    SCENARIOS[name](ctx, call)
    np.savez(out_path, **{f"r{i}": r for i, r in enumerate(recs.values())}, tags=np.array(json.dumps(list(recs))))
    ctx.close()


_GRAM = re.compile(r"\[impop_gram\] (.*)$")


def _launch(name, extra=None, timeout=600):
    """-> (records by call tag, trace by call tag: {"gram": [launch dicts], "chunks": number of chunk-done lines})."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(PYTHONPATH=os.pathsep.join([ROOT, HERE]), IMPOP_TRACE="1", **(extra or {}))
    code = "import sys, test_gpu_batch_regimes as t; t._worker(sys.argv[1], sys.argv[2])"
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "recs.npz")
        r = subprocess.run([sys.executable, "-c", code, name, path], capture_output=True, text=True, env=env, cwd=ROOT,
                           timeout=timeout)
        assert r.returncode == 0, (name, extra, r.stderr[-3000:])
        z = np.load(path)
        tags = json.loads(str(z["tags"]))
        recs = {t: z[f"r{i}"] for i, t in enumerate(tags)}
    trace, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@@call "):
            cur = line[7:]
            trace[cur] = {"gram": [], "chunks": 0}
        elif cur is not None and (m := _GRAM.search(line)):
            trace[cur]["gram"].append({k: int(v) for k, v in (kv.split("=") for kv in m.group(1).split())})
        elif cur is not None and "[impop_pairwise_scan] chunk done" in line:
            trace[cur]["chunks"] += 1
    assert set(trace) == set(recs), (set(trace), set(recs))
    return recs, trace


def _same_records(a, b, what):
    assert a.keys() == b.keys(), what
    for t in a:
        assert a[t].tobytes() == b[t].tobytes(), (what, t)


def _regime(launches, what, ksplit=1, u16=1, chain_min=2, chain=None):
    """Every Gram launch of a call ran in the intended configuration."""
    assert launches, what
    for g in launches:
        assert g["ksplit"] == ksplit and g["u16"] == u16, (what, g)
        assert (g["chain"] == chain) if chain is not None else (g["chain"] >= chain_min), (what, g)


# ---- the oracle ---------------------------------------------------------------------------------------------------

def _check(oracle, I, W, rec, call, inA, inB, L, what, sel=None):
    """One window's record against oracle identity -> pica2 (of the members `sel`, indices; None: of everybody) / h-fst (or
    hud.py's grouped Fst) from its exact counts I.  (tests/test_gpu_irregular_overlap.py uses it too.)"""
    kind, thr, rd, fm = call["kind"], call["thr"], call["rd"], call.get("fm", "direct")
    sim = oracle.identity(I, W, {"match": 0, "dice": 1}[kind])
    pi, ps, _, G = oracle.pica2(sim if sel is None else sim[np.ix_(sel, sel)], thr, L if L else None, rd)
    assert int(rec["n_groups"]) == G, what + (int(rec["n_groups"]), G)
    for k, v in (("pi", pi), ("pi_site", ps)):
        got = float(rec[k])
        assert (got != got and v != v) or rel_close(got, v, REL, 0.0), what + (k, got, v)
    if fm == "grouped":
        h, _ = oracle.hud_grouped(sim, inA, inB, thr, L if L else None, rd)
    else:
        h, _ = oracle.hfst(sim, inA, inB, L if L else None, rd)
    for k, v in h.items():
        assert stat_close(k, float(rec[k]), v, h["dxy"], REL), what + (k, float(rec[k]), v)


def _scan(bm, call, wins):
    return bm.pairwise_scan(wins, None, call["inA"], call["inB"], kind=call["kind"], threshold=call["thr"],
                            round_digits=call["rd"], fst_method=call["fm"], s_scope=call.get("s_scope", 2))


def _pops(n, seed):
    rng = np.random.default_rng(seed)
    inA = (rng.random(n) < 0.35).astype(np.uint8)
    inB = ((rng.random(n) < 0.45) & (inA == 0)).astype(np.uint8)
    return inA, inB


# ---- (a) chained tickets with uint16 counts --------------------------------------------------------------------------

SPECIAL = (1, 63, 64, 65, 127, 128, 129, 383, 384, 385)  # next links of 1 to 3 pairs; pair counts not a multiple of 3


def _chain_windows(n_win, seed):
    """A BED-like tiling of short windows (<= 8192 sites): the special sizes at unaligned and odd-cell starts, 8192-site
    windows with an empty window behind them, random lengths and seq_lens."""
    rng = np.random.default_rng(seed)
    wins, s = [], 0
    for k in range(n_win):
        mode = k % 16
        if mode < 10:
            L = SPECIAL[mode]
            if k % 3 == 0:
                s += int(rng.integers(1, 64))           # unaligned start
            elif k % 3 == 1:
                s = (s + 63) // 64 * 64
                s += 64 if (s // 64) % 2 == 0 else 0    # odd-cell start
        elif mode == 10:
            L = 8192
        elif mode == 11:
            L = 0                                       # empty, between two long ones
        elif mode == 12:
            L = 8192 - int(rng.integers(0, 100))
        else:
            L = int(rng.integers(1, 2000))
        seq = (0, L, 50000)[k % 3]
        wins.append((s, s + L, seq))
        s += L + int(rng.integers(0, 3))
    return wins, s + 64


def _sliding(n_win, size, step, start=5):
    return [(start + k * step, start + k * step + size, size) for k in range(n_win)]


# n -> (tiling windows, sliding windows or 0): enough cells for ksplit = 1 and chains of 2-8 at the default chain choice
CHAIN_SHAPES = {97: (6500, 0), 192: (6500, 0), 200: (3000, 3000), 465: (2200, 2200)}
CHAIN_CALLS = ({"kind": "match", "thr": 0.999, "rd": 4, "fm": "direct"}, {"kind": "dice", "thr": 0.9995, "rd": None, "fm": "grouped"})


def _chain_inputs(n):
    n_tile, n_slide = CHAIN_SHAPES[n]
    tiling, W = _chain_windows(n_tile, seed=n)
    lists = {"tile": tiling}
    if n_slide:
        lists["slide"] = _sliding(n_slide, 600, 300)
        W = max(W, lists["slide"][-1][1] + 64)
    if n == 465:  # descending, under 5 % overlap: not a tiling, no shared segments, cells unsorted (no prefetch across links)
        desc = [(a, b + (64 if k % 50 == 0 and 0 < b - a < 8000 else 0), L) for k, (a, b, L) in enumerate(tiling[:2000])][::-1]
        lists["desc"] = [(a, min(b, W), L) for a, b, L in desc]
    return W, lists


def _weighted_inputs(heavy):
    """n = 200 on the fused-plane path: weights from planes 0, 3 and 6 only (gaps between the used planes); the heaviest
    window weighs `heavy` (65535: uint16 counts, 65536: int32)."""
    n, nw = 200, 3000
    rng = np.random.default_rng(606)
    wins, s = [], 0
    for k in range(nw):
        L = 1000 if k == 1234 else int(rng.integers(20, 800))
        wins.append((s, s + L, 0))
        s += L
    W = s
    w = rng.choice(np.array([1, 8, 9, 64, 65, 72, 73], np.uint32), size=W, p=[.3, .2, .1, .1, .1, .1, .1]).astype(np.uint32)
    a, b, _ = wins[1234]
    w[a:b] = 65                       # 65 000, then + 8 on (heavy - 65000) // 8 sites and + 7 on one more
    extra = heavy - 65000
    w[a:a + extra // 8] = 73
    if extra % 8:
        assert extra % 8 == 7
        w[a + extra // 8] = 72
    cum = np.concatenate(([0], np.cumsum(w.astype(np.int64))))
    assert cum[b] - cum[a] == heavy and max(cum[e] - cum[s0] for s0, e, _ in wins) == heavy
    wins = [(s0, e, int(cum[e] - cum[s0])) for s0, e, _ in wins]
    return n, W, wins, w


def _sc_chains(ctx, call):
    for n in CHAIN_SHAPES:
        W, lists = _chain_inputs(n)
        bm = ctx.synthetic(n, W, seed=n + 1, keep_hap_major=True)
        inA, inB = _pops(n, n)
        for lname, wins in lists.items():
            for ci, c in enumerate(CHAIN_CALLS):
                if lname != "tile" and ci:
                    continue
                c = dict(c, inA=inA, inB=inB)
                call(f"{n}/{lname}/{ci}", lambda: _scan(bm, c, wins))
        bm.free()
    for heavy in (65535, 65536):
        n, W, wins, w = _weighted_inputs(heavy)
        bm = ctx.synthetic(n, W, seed=607, keep_hap_major=True)
        bm.set_site_weights(w)
        inA, inB = _pops(n, 608)
        for ci, c in enumerate(CHAIN_CALLS):
            c = dict(c, inA=inA, inB=inB)
            call(f"weighted/{heavy}/{ci}", lambda: _scan(bm, c, wins))
        bm.free()


def _sc_forced_chain(ctx, call):
    """n = 95 (one 96-row tile, the phi row is the last padding row): one task per window, so even the 8192 cells of a full
    chunk give the default chain choice one link — the chain length is forced by the parent (IMPOP_GRAM_CHAIN)."""
    n = 95
    wins, W = _chain_windows(8192, seed=95)
    bm = ctx.synthetic(n, W, seed=96, keep_hap_major=True)
    inA, inB = _pops(n, 95)
    for ci, c in enumerate(CHAIN_CALLS):
        c = dict(c, inA=inA, inB=inB)
        call(f"95/tile/{ci}", lambda: _scan(bm, c, wins))
    bm.free()


def _chain_samples(n_win, rng, k=6):
    """first and last windows (first links of every queue, partial last chains) and a few in between"""
    mid = rng.choice(np.arange(16, n_win - 16), size=k, replace=False).tolist()
    return sorted(set(list(range(0, 10)) + list(range(n_win - 10, n_win)) + mid))


def _oracle_windows(oracle, ctx, n, W, seed, recs, tagged, weights=None):
    """tagged: [(tag, call, windows, sample indices)] on the synthetic matrix (n, W, seed)"""
    bm = ctx.synthetic(n, W, seed=seed, keep_hap_major=False)
    cum = None if weights is None else np.concatenate(([0], np.cumsum(weights.astype(np.int64))))
    try:
        for tag, c, wins, sample in tagged:
            for k in sample:
                a, b, L = wins[k]
                if b == a:
                    I, Ww = np.zeros((n, n), np.int64), 0
                elif weights is None:
                    I, Ww = oracle.pairwise_counts(bm.download(a, b), n, 0, b - a), b - a
                else:
                    import impop_amd
                    m = impop_amd.unpack_hap_major(bm.download(a, b), b - a).astype(np.int64)
                    I, Ww = (m * weights[a:b].astype(np.int64)) @ m.T, int(cum[b] - cum[a])
                _check(oracle, I, Ww, recs[tag][k], c, c["inA"], c["inB"], L, (tag, k, (a, b, L)))
    finally:
        bm.free()


def test_chained_tickets_with_uint16_counts(ctx, oracle):
    """n = 97 / 192 (no phi row) / 200 / 465 at the default chain choice: tilings of 1..8192-site windows (the special sizes,
    unaligned and odd-cell starts, empty windows between long ones, partial last chains), sliding windows (shared segments
    inside chains), a descending non-tiling list (prefetch refused) and a weighted matrix on the fused-plane path (planes 0, 3,
    6; heaviest window 65 535: uint16, 65 536: int32); `match` / direct Fst and `dice` / grouped Fst."""
    recs, trace = _launch("chains")
    for tag, t in trace.items():
        u16 = 0 if tag.startswith("weighted/65536") else 1
        _regime(t["gram"], tag, u16=u16)
        if tag.startswith("weighted"):
            assert all(g["fused_planes"] == 1 for g in t["gram"]), (tag, t["gram"])
    plain, ptrace = _launch("chains", PLAIN)
    for tag, t in ptrace.items():
        _regime(t["gram"], tag, u16=0, chain=1)
    _same_records(recs, plain, "u16 + chains vs int32, one window per ticket")
    rng = np.random.default_rng(5)
    for n in CHAIN_SHAPES:
        W, lists = _chain_inputs(n)
        inA, inB = _pops(n, n)
        tagged = []
        for lname, wins in lists.items():
            for ci, c in enumerate(CHAIN_CALLS):
                if lname != "tile" and ci:
                    continue
                s = _chain_samples(len(wins), rng, 4 if n == 465 else 6)
                if lname == "tile":
                    s = sorted(set(s) | {10, 11, 12, 13})  # an 8192-site window, the empty one behind it, the one after
                tagged.append((f"{n}/{lname}/{ci}", dict(c, inA=inA, inB=inB), wins, s))
        _oracle_windows(oracle, ctx, n, W, n + 1, recs, tagged)
    for heavy in (65535, 65536):
        n, W, wins, w = _weighted_inputs(heavy)
        inA, inB = _pops(n, 608)
        tagged = [(f"weighted/{heavy}/{ci}", dict(c, inA=inA, inB=inB), wins, sorted(set(_chain_samples(len(wins), rng, 4)) | {1234}))
                  for ci, c in enumerate(CHAIN_CALLS)]
        _oracle_windows(oracle, ctx, n, W, 607, recs, tagged, weights=w)


def test_forced_chains_on_single_tile_windows(ctx, oracle):
    """n = 95 (one tile, phi row as its last padding row), 8192 windows in one launch: chains of 3 (partial last chains in
    every queue) and of 8 — byte-identical to each other, to int32 counts without chains and to the operand stored as given."""
    recs, trace = _launch("forced_chain", {"IMPOP_GRAM_CHAIN": "3"})
    for tag, t in trace.items():
        _regime(t["gram"], tag, chain=3)
    for extra, chain, u16 in (({"IMPOP_GRAM_CHAIN": "8"}, 8, 1), (PLAIN, 1, 0), ({"IMPOP_GRAM_CHAIN": "3", "IMPOP_NO_POLARITY": "1"}, 3, 1)):
        other, otrace = _launch("forced_chain", extra)
        for tag, t in otrace.items():
            _regime(t["gram"], (extra, tag), u16=u16, chain=chain)
        _same_records(recs, other, extra)
    wins, W = _chain_windows(8192, seed=95)
    inA, inB = _pops(95, 95)
    rng = np.random.default_rng(95)
    tagged = [(f"95/tile/{ci}", dict(c, inA=inA, inB=inB), wins, sorted(set(_chain_samples(len(wins), rng)) | {10, 11, 12}))
              for ci, c in enumerate(CHAIN_CALLS)]
    _oracle_windows(oracle, ctx, 95, W, 96, recs, tagged)


# ---- (b) uint16 counts in the upper half of their range ------------------------------------------------------------

LONG = (65535, 40000, 32768, 50001)  # the first one noise-free


def _high_u16_inputs(n):
    """Rows are a founder F (30 %) or its complement (70 %) with noise: every site is stored complemented where F = 0, so the
    F rows store (nearly) all ones and their stored counts reach the window length.  Packed directly.  Layout: the long windows,
    a 65 536-site window, then short windows enough for ksplit = 1.  -> (bits, W, windows without / with the 65 536 one)"""
    rng = np.random.default_rng(n)
    n_short = 8192 // {465: 15, 700: 36}[n] + 60
    starts, s = [], 0
    for L in LONG + (65536,):
        s += int(rng.integers(0, 40))
        starts.append((s, s + L))
        s += L
    short = []
    for k in range(n_short):
        s += int(rng.integers(0, 9))
        L = int(rng.integers(1, 200))
        short.append((s, s + L, (0, L)[k % 2]))
        s += L
    W = s
    nw = (W + 63) // 64
    F = rng.integers(0, 2**63, size=nw, dtype=np.uint64) ^ (rng.integers(0, 2, size=nw, dtype=np.uint64) << np.uint64(63))
    is_f = rng.random(n) < 0.3
    bits = np.where(is_f[:, None], F[None, :], ~F[None, :])
    cnt = int(0.002 * n * W)
    rows, cols = rng.integers(0, n, size=cnt), rng.integers(0, W, size=cnt)
    a0, b0 = starts[0]
    keep = (cols < a0) | (cols >= b0)
    np.bitwise_xor.at(bits, (rows[keep], cols[keep] // 64), np.uint64(1) << (cols[keep] % 64).astype(np.uint64))
    if W % 64:
        bits[:, -1] &= np.uint64((1 << (W % 64)) - 1)
    longw = [(a, b, (b - a) * (1 + k % 2)) for k, (a, b) in enumerate(starts)]
    return bits, W, longw[:4] + short, longw + short


HIGH_CALLS = ({"kind": "match", "thr": 0.999, "rd": 5, "fm": "direct"}, {"kind": "dice", "thr": 0.9999, "rd": None, "fm": "direct"})


def _sc_high_u16(ctx, call):
    for n in (465, 700):
        bits, W, wins, wins16 = _high_u16_inputs(n)
        bm = ctx.upload(bits, W, keep_hap_major=True)
        inA, inB = _pops(n, n + 7)
        for ci, c in enumerate(HIGH_CALLS):
            c = dict(c, inA=inA, inB=inB)
            call(f"{n}/below/{ci}", lambda: _scan(bm, c, wins))
            call(f"{n}/at65536/{ci}", lambda: _scan(bm, c, wins16))
        bm.free()


def test_uint16_counts_in_the_upper_half_of_their_range(ctx, oracle):
    """Windows of 32 768 .. 65 535 sites whose stored (minor-allele) counts reach 2^15 and beyond — 65 535 exactly in a noise-free
    window — among enough short windows for ksplit = 1 and uint16 counts: `match` and `dice` (the uint16 unflip), n = 465
    (stats_small.hip) and n = 700 (general kernels).  With a 65 536-site window in the call: int32 counts, equally exact."""
    import impop_amd
    for n in (465, 700):  # precondition, in numpy: the stored polarity really has counts >= 2^15, and 65 535 in the first window
        bits, W, wins, _ = _high_u16_inputs(n)
        top = 0
        for k, (a, b, _) in enumerate(wins[:4]):
            m = impop_amd.unpack_hap_major(bits[:, a // 64:(b + 63) // 64], b - a // 64 * 64)[:, a % 64:]
            c = m.sum(axis=0, dtype=np.int64)
            stored = m ^ (2 * c > n).astype(np.uint8)[None, :]
            a_row = stored.sum(axis=1, dtype=np.int64)    # the diagonal of the stored Gram: its largest entries
            top = max(top, int(a_row.max()))
            if k == 0:
                assert int(a_row.max()) == 65535 == b - a
        assert top >= 32768
    recs, trace = _launch("high_u16")
    for tag, t in trace.items():
        _regime(t["gram"], tag, u16=0 if "/at65536/" in tag else 1, chain=1)
    plain, ptrace = _launch("high_u16", PLAIN)
    for tag, t in ptrace.items():
        _regime(t["gram"], tag, u16=0, chain=1)
    _same_records(recs, plain, "u16 vs int32")
    for n in (465, 700):
        bits, W, wins, wins16 = _high_u16_inputs(n)
        inA, inB = _pops(n, n + 7)
        for ci, c in enumerate(HIGH_CALLS):
            c = dict(c, inA=inA, inB=inB)
            for what, ww, sample in (("below", wins, (0, 1, 2, 3, 4, len(wins) - 1)), ("at65536", wins16, (0, 4, 5))):
                for k in sample:
                    a, b, L = ww[k]
                    I = oracle.pairwise_counts(bits, n, a, b)
                    _check(oracle, I, b - a, recs[f"{n}/{what}/{ci}"][k], c, inA, inB, L, (n, what, ci, k))


# ---- (c) chunking by bytes at a large leading dimension ---------------------------------------------------------------

BIG_N = 2000


def _big_ld_lists():
    rng = np.random.default_rng(2000)
    disjoint, s = [], 0
    for k in range(700):
        L = int(rng.integers(1, 400))
        disjoint.append((s, s + L, (0, L)[k % 2]))
        s += L + int(rng.integers(0, 5))
    sliding = _sliding(700, 400, 200, start=3)
    W = max(s, sliding[-1][1]) + 64
    return W, {"disjoint": disjoint, "sliding": sliding}


BIG_CALL = {"kind": "match", "thr": 0.999, "rd": 4, "fm": "direct"}


def _big_ld_inputs():
    """Packed directly: the first half of the haplotypes descends from four founders, the second half from four others, so
    the two halves (the populations) are apart and Fst is not a near-cancellation (random populations at n = 2000 leave
    Da = Dxy - pi_xy at the rounding level of their sums, below what the tolerance policy can compare)."""
    W, lists = _big_ld_lists()
    rng = np.random.default_rng(2002)
    nw = (W + 63) // 64
    f = rng.integers(0, 2**63, size=(8, nw), dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, size=(8, nw), dtype=np.uint64)
    who = np.where(np.arange(BIG_N) < BIG_N // 2, rng.integers(0, 4, size=BIG_N), rng.integers(4, 8, size=BIG_N))
    bits = f[who].copy()
    cnt = int(0.002 * BIG_N * W)
    rows, cols = rng.integers(0, BIG_N, size=cnt), rng.integers(0, W, size=cnt)
    np.bitwise_xor.at(bits, (rows, cols // 64), np.uint64(1) << (cols % 64).astype(np.uint64))
    if W % 64:
        bits[:, -1] &= np.uint64((1 << (W % 64)) - 1)
    inA = (np.arange(BIG_N) < BIG_N // 2).astype(np.uint8)
    return bits, W, lists, inA, (1 - inA).astype(np.uint8)


def _sc_big_ld(ctx, call):
    bits, W, lists, inA, inB = _big_ld_inputs()
    bm = ctx.upload(bits, W, keep_hap_major=True)
    c = dict(BIG_CALL, inA=inA, inB=inB)
    for name, wins in lists.items():
        call(f"{name}/whole", lambda: _scan(bm, c, wins))
        h = len(wins) // 2
        call(f"{name}/halves", lambda: np.concatenate([_scan(bm, c, wins[:h]), _scan(bm, c, wins[h:])]))
    bm.free()


def test_chunking_by_bytes_at_a_large_leading_dimension(ctx, oracle):
    """n = 2000 (ld = 2016: 16 MB per Gram matrix, so a chunk holds a few hundred): ~700 short disjoint / sliding windows run
    in two or more chunks, each with ksplit = 1, uint16 counts and chains; the whole call equals the same windows asked for in
    two halves, byte for byte, and the windows on either side of each cut match the oracle."""
    recs, trace = _launch("big_ld")
    plain, _ = _launch("big_ld", PLAIN)
    _same_records(recs, plain, "u16 + chains vs int32, one window per ticket")
    bits, W, lists, inA, inB = _big_ld_inputs()
    c = dict(BIG_CALL, inA=inA, inB=inB)
    for name, wins in lists.items():
        t = trace[f"{name}/whole"]
        assert t["chunks"] >= 2 and len(t["gram"]) == t["chunks"], (name, t)
        _regime(t["gram"], name)
        assert recs[f"{name}/whole"].tobytes() == recs[f"{name}/halves"].tobytes(), name
        sample, done = {0, len(wins) - 1}, 0
        for g in t["gram"][:-1]:  # cut after about `cells` windows (sliding: a chunk's windows cover one cell more)
            done += g["cells"]
            sample |= {k for k in range(done - 2, done + 2) if 0 <= k < len(wins)}
        for k in sorted(sample):
            a, b, L = wins[k]
            I = oracle.pairwise_counts(bits, BIG_N, a, b)
            _check(oracle, I, b - a, recs[f"{name}/whole"][k], c, inA, inB, L, (name, k))


# ---- (d) compaction and window mapping at scale -----------------------------------------------------------------------

CN, CW = 200, 300000  # five chunks of 1024 blocks (65 536 sites) in the compaction's prefix scan


def _compact_inputs():
    """Packed 8192 sites at a time: 45 % all-zero, 45 % all-one and 10 % variable columns; sites [65536, 131072) without a
    variable site, [196608, 262144) all variable.  -> (bits, kept positions, packed kept columns)"""
    from oracle import oracle as orc
    rng = np.random.default_rng(300)
    f = (rng.random((6, 8192)) < 0.5).astype(np.uint8)
    words, kept_cols, var = [], [], []
    for s in range(0, CW, 8192):
        L = min(8192, CW - s)
        kind = rng.choice(3, size=L, p=[0.45, 0.45, 0.10])
        if 65536 <= s < 131072:
            kind = rng.choice(2, size=L)
        elif 196608 <= s < 262144:
            kind[:] = 2
        m = np.zeros((CN, L), np.uint8)
        m[:, kind == 1] = 1
        v = np.nonzero(kind == 2)[0]
        m[:, v] = f[rng.integers(0, 6, size=CN)][:, v % 8192] ^ (rng.random((CN, v.size)) < 0.01)
        m[0, v] = 1
        m[1, v] = 0  # every "variable" column really is
        words.append(orc.pack_hap_major(m))
        kept_cols.append(m[:, v])
        var.append(s + v)
    var = np.concatenate(var).astype(np.uint64)
    return np.concatenate(words, axis=1), var, orc.pack_hap_major(np.concatenate(kept_cols, axis=1))


def _compact_windows(pos):
    rng = np.random.default_rng(301)
    P = pos.astype(np.int64)
    e = {0, CW, int(P[0]) - 1, int(P[0]), int(P[-1]), int(P[-1]) + 1}
    for k in range(0, P.size, 4096):
        e |= {int(P[k]) - 1, int(P[k]), int(P[k]) + 1}
    for j in range(1, 5):
        e |= {65536 * j - 1, 65536 * j, 65536 * j + 1}
    e |= set(P[rng.choice(P.size, 400, replace=False)].tolist())
    e |= set(rng.integers(0, CW, size=1400).tolist())
    e = sorted(x for x in e if 0 <= x <= CW)
    return [(a, b, (b - a, 0, 7777)[k % 3]) for k, (a, b) in enumerate(zip(e[:-1], e[1:]))]


COMPACT_CALL = {"kind": "dice", "thr": 0.999, "rd": 5, "fm": "direct", "s_scope": 0}


def _sc_compact(ctx, call):
    bits, pos, _ = _compact_inputs()
    wins = _compact_windows(pos)
    full = ctx.upload(bits, CW, keep_hap_major=True)
    cm = full.compact()
    inA, inB = _pops(CN, 302)
    c = dict(COMPACT_CALL, inA=inA, inB=inB)
    call("compact/all", lambda: _scan(cm, c, wins))
    call("compact/slices", lambda: np.concatenate([_scan(cm, c, wins[k:k + 255]) for k in range(0, len(wins), 255)]))
    call("full/all", lambda: _scan(full, c, wins))
    cm.free()
    full.free()


def test_compaction_and_window_mapping_at_scale(ctx, oracle):
    """n = 200, 300 000 sites (five prefix-scan chunks, a chunk without and one with only variable sites, > 4096 kept sites):
    n_site, positions() and download() exactly against numpy; window edges before the first / after the last kept site, on
    kept positions, on pos[k * 4096] and +-1, on the chunk boundaries and at the end.  pairwise_scan of >= 256 windows (edges
    mapped on the device; ksplit = 1) equals the same windows in slices of <= 255 (mapped on the host) and the full matrix's
    records; scan and scan_multi (host mapping through the coarse level) equal the full matrix's."""
    bits, pos, kept = _compact_inputs()
    assert pos.size > 4096
    wins = _compact_windows(pos)
    assert len(wins) >= 256
    full = ctx.upload(bits, CW, keep_hap_major=False)
    cm = full.compact()
    try:
        assert cm.n_site == pos.size and cm.n_hap == CN
        assert (cm.positions() == pos).all()
        assert (cm.download() == kept).all()
        inA, inB = _pops(CN, 302)
        assert cm.scan(wins, None, inA, inB).tobytes() == full.scan(wins, None, inA, inB).tobytes()
        pops = [(np.arange(CN) % 3 == k).astype(np.uint8) for k in range(3)]
        assert cm.scan_multi(wins, pops).tobytes() == full.scan_multi(wins, pops).tobytes()
    finally:
        cm.free()
        full.free()
    recs, trace = _launch("compact")
    plain, _ = _launch("compact", PLAIN)
    _same_records(recs, plain, "u16 vs int32")
    g = trace["compact/all"]["gram"]
    assert len(g) == 1 and g[0]["ksplit"] == 1 and g[0]["u16"] == 1, g
    assert recs["compact/all"].tobytes() == recs["compact/slices"].tobytes()
    assert recs["compact/all"].tobytes() == recs["full/all"].tobytes()
    c = dict(COMPACT_CALL, inA=inA, inB=inB)
    for k in (0, 1, 2, len(wins) // 2, len(wins) - 2, len(wins) - 1):
        a, b, L = wins[k]
        _check(oracle, oracle.pairwise_counts(bits, CN, a, b), b - a, recs["compact/all"][k], c, inA, inB, L, ("compact", k))


# ---- (e) several chunks of overlapping windows --------------------------------------------------------------------------

SLIDE_N, SLIDE_W = 40, 320
SLIDE_CALLS = ({"kind": "match", "thr": 0.97, "rd": 4}, {"kind": "dice", "thr": 0.95, "rd": None})


def _slide_inputs():
    """Windows of 64 sites at step 16 (every site but the edges in four windows: shared segments) and an empty window among
    them; a subset P and disjoint A / B."""
    wins = _sliding((SLIDE_W - 64) // 16 + 1, 64, 16, start=0)
    wins.insert(7, (100, 100, 0))
    rng = np.random.default_rng(41)
    inP = (rng.random(SLIDE_N) < 0.8).astype(np.uint8)
    inA, inB = _pops(SLIDE_N, 42)
    return wins, inP, inA, inB


def _sc_slide(ctx, call):
    wins, inP, inA, inB = _slide_inputs()
    bm = ctx.synthetic(SLIDE_N, SLIDE_W, seed=43, keep_hap_major=True)
    for ci, c in enumerate(SLIDE_CALLS):
        call(f"slide/{ci}", lambda: bm.pairwise_scan(wins, inP, inA, inB, kind=c["kind"], threshold=c["thr"], round_digits=c["rd"], s_scope=1))
    bm.free()


def test_overlapping_windows_in_chunks_of_three(ctx, oracle):
    """impop_pairwise_scan on sliding windows (elementary segments shared by neighbours, an empty window, subset P, A / B) with
    IMPOP_PAIRWISE_CHUNK=3: several chunks, neighbouring chunks contract their shared segments again — the records of the one-chunk
    call byte for byte, and both the oracle's."""
    recs, trace = _launch("slide")
    chunked, ctrace = _launch("slide", {"IMPOP_PAIRWISE_CHUNK": "3"})
    wins, inP, inA, inB = _slide_inputs()
    assert all(not (a & b) for a, b in zip(inA, inB)) and inA.any() and inB.any() and 1 < inP.sum() < SLIDE_N
    for tag in recs:
        assert trace[tag]["chunks"] == 1 and ctrace[tag]["chunks"] == (len(wins) + 2) // 3, (tag, trace[tag], ctrace[tag])
    _same_records(recs, chunked, "one chunk vs chunks of three windows")
    bm = ctx.synthetic(SLIDE_N, SLIDE_W, seed=43, keep_hap_major=False)
    sel = np.nonzero(inP)[0]
    try:
        for ci, c in enumerate(SLIDE_CALLS):
            for got in (recs, chunked):
                for k, (a, b, L) in enumerate(wins):
                    I = oracle.pairwise_counts(bm.download(a, b), SLIDE_N, 0, b - a) if b > a else np.zeros((SLIDE_N, SLIDE_N), np.int64)
                    _check(oracle, I, b - a, got[f"slide/{ci}"][k], c, inA, inB, L, (ci, k, (a, b, L)), sel=sel)
    finally:
        bm.free()


SCENARIOS = {"chains": _sc_chains, "forced_chain": _sc_forced_chain, "high_u16": _sc_high_u16, "big_ld": _sc_big_ld,
             "compact": _sc_compact, "slide": _sc_slide}
