"""The rare/common split of the variable-site scan index (run with -m gpu on an MI355X).

A kept site with min(c, n - c) <= 3 is stored as one 8-byte entry listing its minor-allele carriers; the other kept sites stay
SB64 rows.  Every scenario here scans the same windows on three matrices made from the same bits: the split index (default),
the unsplit index (IMPOP_KEEP_NO_RARE_SPLIT) and no index (IMPOP_KEEP_DENSE_SCAN).  Records must be byte-identical, sampled
windows must match the exact oracle, and the IMPOP_TRACE=1 lines must show the route and the split.  The calls run in one
child process (IMPOP_TRACE is read once per process); each call is announced by a marker line on stderr."""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import ROOT, stat_close

pytestmark = pytest.mark.gpu

KINDS = ("split", "nosplit", "dense")
INT_KEYS = ("n_sites", "s_all", "s_p", "s_a", "s_b", "sum_p", "sum_a", "sum_b", "sum_ab")
DBL_KEYS = ("pi", "pi_site", "pi_a", "pi_b", "pi_xy", "dxy", "da", "fst", "tajima_d")
SYN_N, SYN_S = 465, 64 * 3000 + 5  # synthetic matrix whose split counts are checked against tests/synth_ref.py


# ---- child side ---------------------------------------------------------------------------------------------------

def _crafted(n, seed):
    """0/1 [n, S]: rare-only, common-only and monomorphic stretches, then a mix.  Rare columns have 1..4 carriers of either
    allele at haplotypes 0, 31, 32, n - 1 (MAC 4 is common), plus private sites at random haplotypes."""
    rng = np.random.default_rng(seed)
    S = 64 * 300 + 13
    sets = [[0], [31], [32], [n - 1], [0, 31], [32, n - 1], [0, 31, 32], [31, 32, n - 1], [0, 31, 32, n - 1], [1, 2, 3, 4]]
    rare_cols = []
    for car in sets:
        for pol in (0, 1):
            col = np.zeros(n, np.uint8)
            col[car] = 1
            rare_cols.append(col ^ pol)
    rare_cols = np.array(rare_cols).T
    m = np.repeat((rng.random(S) < 0.5)[None, :].astype(np.uint8), n, axis=0)  # monomorphic 0 or 1

    def put_rare(lo, hi, p):
        idx = np.nonzero(rng.random(hi - lo) < p)[0] + lo
        m[:, idx] = rare_cols[:, rng.integers(0, rare_cols.shape[1], len(idx))]

    def put_common(lo, hi, p):
        idx = np.nonzero(rng.random(hi - lo) < p)[0] + lo
        m[:, idx] = (rng.random((n, len(idx))) < 0.3).astype(np.uint8)

    put_rare(0, 4000, 0.3)
    put_common(4000, 8000, 0.1)
    put_rare(10000, S, 0.1)
    put_common(10000, S, 0.05)
    idx = np.nonzero(rng.random(S - 10000) < 0.05)[0] + 10000  # private sites of either polarity at random haplotypes
    for s in idx:
        h = rng.integers(0, n)
        m[:, s] = 0
        m[h, s] = 1
        if rng.random() < 0.5:
            m[:, s] ^= 1
    return m


def _masks(n, seed, cfg):
    """P / A / B with haplotypes 0, 31, 32, n - 1 in P only, A only, B only, A and B (the overlap leaves both), or none"""
    rng = np.random.default_rng(seed)
    P = (rng.random(n) < 0.6).astype(np.uint8)
    A = np.zeros(n, np.uint8); A[: n // 2] = 1
    B = np.zeros(n, np.uint8); B[n // 3:] = 1
    sp = [0, 31, 32, n - 1]
    P[sp] = cfg == "P"
    A[sp] = cfg in ("A", "AB")
    B[sp] = cfg in ("B", "AB")
    return P, A, B


def _run_child(out_path):
    import impop_amd
    from impop_amd import engine
    ctx = impop_amd.Context(0)
    recs, oracle_items, infos = {}, [], {}

    def call(tag, fn):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        recs[tag] = np.asarray(fn())
        sys.stderr.flush()

    def oracle_window(tag, bm, wi, w, P, A, B):
        s0, s1, sl = int(w[0]), int(w[1]), int(w[2]) if len(w) > 2 else 0
        ov = A & B
        oracle_items.append({"tag": tag, "wi": wi, "n": bm.n_hap, "s0": s0, "s1": s1, "seq_len": sl,
                             "P": None if P is None else P.tolist(), "A": (A & ~ov).tolist(), "B": (B & ~ov).tolist()})
        recs[f"bits:{len(oracle_items) - 1}"] = bm.download(s0, s1)

    def three(make):
        return {"split": make(dict()), "nosplit": make(dict(rare_split=False)), "dense": make(dict(dense_scan=True))}

    def each(tag, ms, fn):
        for k in KINDS:
            call(f"{tag}|{k}", lambda k=k: fn(ms[k]))

    # crafted matrices: n = 100, 465, 512 (fixed-WPS kernel) and 600 (the any-n kernel)
    for n in (100, 465, 512, 600):
        bits = _crafted(n, n)
        S = bits.shape[1]
        ms = three(lambda kw: ctx.upload_dense(bits, keep_hap_major=False, **kw))
        infos[f"c{n}"] = {k: {**ms[k].scan_index_info(), **ms[k].scan_split_info()} for k in KINDS}
        infos[f"c{n}_truth"] = _truth(bits)
        wins = [(0, 4000, 0), (4000, 8000, 0), (8000, 10000, 0), (0, S, S), (3990, 4010, 0), (9999, 10001, 0), (5, 5, 0),
                (63, 65, 0), (S - 13, S, 0), (10000, S, 12345)]
        fixed = impop_amd.fixed_windows(S, 3000)
        slide = impop_amd.fixed_windows(S, 5000, 1700)
        for cfg in ("P", "A", "B", "AB", "none"):
            P, A, B = _masks(n, n + 1, cfg)
            each(f"c{n}_{cfg}_edges", ms, lambda m: m.scan(wins, P, A, B))
            if cfg in ("A", "AB"):
                oracle_window(f"c{n}_{cfg}_edges|split", ms["split"], 0, wins[0], P, A, B)
                oracle_window(f"c{n}_{cfg}_edges|split", ms["split"], 9, wins[9], P, A, B)
        P, A, B = _masks(n, n + 2, "B")
        each(f"c{n}_fixed", ms, lambda m: m.scan(fixed, None, A, B))
        each(f"c{n}_sliding", ms, lambda m: m.scan(slide, P, A, B, 2, 1))
        oracle_window(f"c{n}_fixed|split", ms["split"], 2, (int(fixed[2]["site_begin"]), int(fixed[2]["site_end"]),
                                                             int(fixed[2]["seq_len"])), None, A, B)
        pops = [np.arange(n) % 2 == 0, np.arange(n) % 2 == 1]
        each(f"c{n}_multi2", ms, lambda m: m.scan_multi(slide, pops))
        pops8 = [(np.arange(n) % 8) == k for k in range(8)]
        pops8[0][[0, 31]] = False
        each(f"c{n}_multi8", ms, lambda m: m.scan_multi(fixed, pops8))

        def set_after(m, P=P, A=A, B=B):
            pl = m.plan(fixed, None, A, B)
            pl.launch()
            r1 = pl.fetch()
            P2, A2, B2 = _masks(n, n + 3, "AB")
            pl.set_masks(P2, A2, B2)
            pl.launch()
            r2 = pl.fetch()
            pl.destroy()
            return np.concatenate([r1, r2])
        each(f"c{n}_set_masks", ms, set_after)
        P2, A2, B2 = _masks(n, n + 3, "AB")
        each(f"c{n}_fresh", ms, lambda m: m.scan(fixed, P2, A2, B2))
        for m in ms.values():
            m.free()

    # n <= 64: rows are no wider than an entry, the index stays unsplit
    bits = _crafted(40, 40)
    ms = three(lambda kw: ctx.upload_dense(bits, keep_hap_major=False, **kw))
    infos["c40"] = {k: {**ms[k].scan_index_info(), **ms[k].scan_split_info()} for k in KINDS}
    P, A, B = _masks(40, 41, "A")
    each("c40", ms, lambda m: m.scan(impop_amd.fixed_windows(bits.shape[1], 2000), P, A, B))
    for m in ms.values():
        m.free()

    # synthetic matrix: split counts against tests/synth_ref.py (in the parent), one chromosome-long window (many tiles)
    ms = three(lambda kw: ctx.synthetic(SYN_N, SYN_S, seed=21, **kw))
    infos["syn"] = {k: {**ms[k].scan_index_info(), **ms[k].scan_split_info()} for k in KINDS}
    P, A, B = _masks(SYN_N, 5, "P")
    whole = [(0, SYN_S, 0)]
    each("syn_whole", ms, lambda m: m.scan(whole, P, A, B))
    each("syn_whole_t4", ms, lambda m: m.scan(whole, P, A, B, tile_blocks=4))
    sys.stderr.write("@@call none\n")  # not compared call by call
    sys.stderr.flush()
    pl = ms["split"].plan(whole, P, A, B, tile_blocks=4)
    infos["syn_tiles_t4"] = pl.n_tiles
    pl.destroy()
    each("syn_windows", ms, lambda m: m.scan(impop_amd.fixed_windows(SYN_S, 50000, 20000), None, A, B))
    oracle_window("syn_whole|split", ms["split"], 0, (0, SYN_S), P, A, B)
    for m in ms.values():
        m.free()

    # impop_scan_sharded: two split slabs on two contexts against one whole matrix of each kind
    S4 = 64 * 1500 + 29
    w4 = impop_amd.fixed_windows(S4, 6000, 2000)
    P, A, B = _masks(SYN_N, 6, "B")
    ms = three(lambda kw: ctx.synthetic(SYN_N, S4, seed=14, **kw))
    each("sharded_whole", ms, lambda m: m.scan(w4, P, A, B))
    ctx2 = impop_amd.Context(0)
    slabs, begins = [], []
    for k, c in enumerate((ctx, ctx2)):
        _, _, b0, b1 = engine.shard_windows_c(w4, 2, k)
        slabs.append(c.synthetic(SYN_N, b1 - b0, seed=14, site_begin=b0))
        begins.append(b0)
    call("sharded|split", lambda: engine.scan_sharded(slabs, begins, w4, P, A, B))
    for s_ in slabs:
        s_.free()
    for m in ms.values():
        m.free()
    ctx2.close()

    # graph capture of a split plan
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c3 = impop_amd.Context(0, stream=s.cuda_stream)
        NW, Wn = 200, 50000
        wins = impop_amd.fixed_windows(NW * Wn, Wn)
        P, A, B = _masks(SYN_N, 7, "none")
        sys.stderr.write("@@call graph|split\n")
        big = c3.synthetic(SYN_N, NW * Wn, seed=15)
        pl = big.plan(wins, P, A, B)
        sys.stderr.write("@@call none\n")
        pl.launch()
        recs["graph_eager|split"] = pl.fetch()
        g_out = torch.zeros(NW * 128, dtype=torch.uint8, device="cuda")
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            pl.launch(g_out.data_ptr())
        infos["graph_zero_after_capture"] = int(g_out.sum()) == 0
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        recs["graph_replay|split"] = g_out.cpu().numpy()
        del g
        pl.destroy()
        big.free()
        c3.close()
    np.savez(out_path, **{f"r{i}": r for i, r in enumerate(recs.values())}, tags=np.array(json.dumps(list(recs))),
             oracle=np.array(json.dumps(oracle_items)), infos=np.array(json.dumps(infos)))
    ctx.close()


def _truth(bits):
    n = bits.shape[0]
    c = bits.sum(axis=0, dtype=np.int64)
    var = (c > 0) & (c < n)
    rare = var & (np.minimum(c, n - c) <= 3)
    return {"n_kept": int(var.sum()), "n_rare": int(rare.sum()), "n_common": int((var & ~rare).sum())}


# ---- parent side --------------------------------------------------------------------------------------------------

_SCAN = re.compile(r"\[impop_scan\] (.*)$")


@pytest.fixture(scope="module")
def run():
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], capture_output=True, text=True, cwd=ROOT,
                           env=env, timeout=900)
        assert r.returncode == 0, r.stderr[-4000:]
        z = np.load(out)
        tags = json.loads(str(z["tags"]))
        recs = {t: z[f"r{i}"] for i, t in enumerate(tags)}
        oracle_items = json.loads(str(z["oracle"]))
        infos = json.loads(str(z["infos"]))
    traces, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@@call "):
            cur = line[7:]
            continue
        mt = _SCAN.search(line)
        if mt and cur is not None:
            head, _, why = mt.group(1).partition(" why=")
            d = dict(kv.split("=", 1) for kv in head.split())
            d["why"] = why
            traces.setdefault(cur, []).append(d)
    return recs, traces, oracle_items, infos


def _bases(recs):
    return sorted({t.split("|")[0] for t in recs if t.endswith("|split") and t.split("|")[0] + "|dense" in recs})


def test_three_layouts_byte_identical(run):
    recs, _, _, _ = run
    bases = _bases(recs)
    assert len(bases) >= 49
    for base in bases:
        a = recs[base + "|split"]
        assert len(a) > 0, base
        for k in ("nosplit", "dense"):
            b = recs[base + "|" + k]
            assert a.dtype == b.dtype and a.shape == b.shape, (base, k)
            assert a.tobytes() == b.tobytes(), (base, k)
    assert recs["sharded|split"].tobytes() == recs["sharded_whole|dense"].tobytes()
    for n in (100, 465, 512, 600):  # set_masks after create: the second launch equals a fresh scan with those masks
        nf = len(recs[f"c{n}_fresh|split"])
        assert recs[f"c{n}_set_masks|split"][nf:].tobytes() == recs[f"c{n}_fresh|split"].tobytes(), n


def test_graph_capture(run):
    recs, _, _, infos = run
    assert infos["graph_zero_after_capture"] is True
    assert recs["graph_replay|split"].tobytes() == recs["graph_eager|split"].tobytes()


def test_split_info_and_counts(run):
    _, _, _, infos = run
    for n in (100, 465, 512, 600):
        t, i = infos[f"c{n}_truth"], infos[f"c{n}"]
        assert i["split"]["n_kept"] == t["n_kept"] == i["nosplit"]["n_kept"], n
        assert (i["split"]["n_rare"], i["split"]["n_common"]) == (t["n_rare"], t["n_common"]), (n, i["split"], t)
        assert i["split"]["rare_bytes"] == 8 * t["n_rare"] and i["split"]["why"] == "", n
        assert i["nosplit"]["n_rare"] == 0 and i["nosplit"]["why"].startswith("opted out"), n
        assert i["dense"]["n_kept"] == 0 and i["dense"]["n_rare"] == 0 and i["dense"]["why"] != "", n
    c40 = infos["c40"]["split"]
    assert c40["n_kept"] > 0 and c40["index_bytes"] > 0 and c40["n_rare"] == 0 and "64" in c40["why"]
    # the synthetic generator, restated in numpy
    from synth_ref import synth_matrix
    t = _truth(synth_matrix(SYN_N, 0, SYN_S, seed=21))
    i = infos["syn"]
    assert i["split"]["n_kept"] == t["n_kept"] and i["split"]["n_rare"] == t["n_rare"] and i["split"]["n_common"] == t["n_common"]
    assert t["n_rare"] > t["n_common"] > 0
    assert 0 < i["split"]["index_bytes"] < i["nosplit"]["index_bytes"]
    assert infos["syn_tiles_t4"] > 8


def test_routes_from_trace(run):
    recs, traces, _, infos = run
    for base in _bases(recs):
        for k in KINDS:
            lines = traces.get(f"{base}|{k}")
            assert lines, (base, k)
            for d in lines:
                assert d["route"] == ("dense" if k == "dense" else "indexed"), (base, k, d)
                assert "rare_sites" in d and "rare_bytes" in d and "split" in d, d
                if k == "dense":
                    assert d["why"].startswith("opted out") and d["split"].startswith("off:") and d["rare_bytes"] == "0", (base, d)
                elif k == "split" and not base.startswith("c40"):
                    assert d["why"] == "" and d["split"] == "on" and int(d["rare_sites"]) > 0, (base, d)
                else:
                    assert d["why"] == "" and d["split"].startswith("off:") and d["rare_bytes"] == "0", (base, d)
    assert traces["c40|split"][0]["split"].startswith("off:n_hap_<=_64")
    assert all(d["split"] == "on" for d in traces["sharded|split"])
    # kept_sites counts every variable site; the split plan reads fewer bytes than the unsplit one
    a, b = traces["syn_whole|split"][0], traces["syn_whole|nosplit"][0]
    assert a["kept_sites"] == b["kept_sites"] == str(infos["syn"]["split"]["n_kept"])
    assert int(a["rare_bytes"]) == 8 * infos["syn"]["split"]["n_rare"]
    assert 0 < int(a["bytes_streamed"]) * 2 < int(b["bytes_streamed"])
    assert traces["graph|split"][0]["split"] == "on"


def test_sampled_windows_against_oracle(run, oracle):
    recs, _, items, _ = run
    assert len(items) >= 16
    for i, it in enumerate(items):
        n = it["n"]
        bits = recs[f"bits:{i}"]
        flags = lambda v: np.ones(n, np.uint8) if v is None else np.asarray(v, np.uint8)
        want = oracle.window_sitecount(bits, n, 0, it["s1"] - it["s0"], oracle.pack_mask(flags(it["P"])), oracle.pack_mask(flags(it["A"])),
                                       oracle.pack_mask(flags(it["B"])), it["seq_len"], 0, 0)
        got = recs[it["tag"]][it["wi"]]
        for k in INT_KEYS:
            assert int(got[k]) == int(want[k]), (it["tag"], it["wi"], k, int(got[k]), int(want[k]))
        for k in DBL_KEYS:
            assert stat_close(k, float(got[k]), float(want[k]), float(want["dxy"])), (it["tag"], it["wi"], k, float(got[k]), want[k])


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    sys.path.insert(0, ROOT)
    _run_child(sys.argv[2])
