"""The variable-site scan index (run with -m gpu on an MI355X).

Every matrix made by upload / synthetic carries an index of the sites that vary among all haplotypes, and scan plans of an
unweighted matrix stream those sites only.  Each scenario here scans the same windows on an indexed matrix and on the same
matrix made with the opt-out flag (IMPOP_KEEP_DENSE_SCAN), requires byte-identical records, asserts each plan's route from its
IMPOP_TRACE=1 line, and checks sampled windows against the exact oracle.  The calls run in one child process (IMPOP_TRACE is
read once per process); each call is announced by a marker line on stderr so its trace lines can be told apart."""
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

HERE = os.path.dirname(os.path.abspath(__file__))
INT_KEYS = ("n_sites", "s_all", "s_p", "s_a", "s_b", "sum_p", "sum_a", "sum_b", "sum_ab")
DBL_KEYS = ("pi", "pi_site", "pi_a", "pi_b", "pi_xy", "dxy", "da", "fst", "tajima_d")


# ---- child side ---------------------------------------------------------------------------------------------------

def _masks(n, seed):
    rng = np.random.default_rng(seed)
    P = (rng.random(n) < 0.6).astype(np.uint8)
    A = np.zeros(n, np.uint8); A[: n // 2] = 1
    B = np.zeros(n, np.uint8); B[n // 3:] = 1  # overlaps A: the overlap leaves both
    return P, A, B


def _pair(ctx, call, tag, make, fn):
    """the same calls on the indexed matrix and on its dense (opt-out) twin"""
    idx, den = make(False), make(True)
    call(f"{tag}|indexed", lambda: fn(idx))
    call(f"{tag}|dense", lambda: fn(den))
    return idx, den


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

    def oracle_window(tag, bm, wi, w, P, A, B, mode=0, scope=0):
        s0, s1, sl = int(w["site_begin"]), int(w["site_end"]), int(w["seq_len"])
        ov = A & B
        oracle_items.append({"tag": tag, "wi": wi, "n": bm.n_hap, "s0": s0, "s1": s1, "seq_len": sl, "mode": mode, "scope": scope,
                             "P": None if P is None else P.tolist(), "A": (A & ~ov).tolist(), "B": (B & ~ov).tolist()})
        recs[f"bits:{len(oracle_items) - 1}"] = bm.download(s0, s1)

    # n = 465 (WPS 15): fixed windows (the last one clipped at n_site, n_site not a multiple of 64), sliding overlapping windows,
    # subset P, overlapping A / B, every d_pi_mode x s_scope, and set_masks after create
    n, S = 465, 64 * 2000 + 37
    P, A, B = _masks(n, 1)
    fixed = impop_amd.fixed_windows(S, 5000)
    slide = impop_amd.fixed_windows(S, 7000, 2500)
    mk = lambda d: ctx.synthetic(n, S, seed=11, dense_scan=d)
    idx, den = mk(False), mk(True)
    infos["n465"] = idx.scan_index_info()
    infos["n465_dense"] = den.scan_index_info()
    for mode in (0, 1, 2):
        for scope in (0, 1):
            for name, m in (("indexed", idx), ("dense", den)):
                call(f"n465_fixed_{mode}{scope}|{name}", lambda m=m: m.scan(fixed, P, A, B, mode, scope))
    for name, m in (("indexed", idx), ("dense", den)):
        call(f"n465_sliding|{name}", lambda m=m: m.scan(slide, None, A, B))

        def set_after(m=m):
            pl = m.plan(fixed, None, A, B)
            pl.launch()
            r1 = pl.fetch()
            pl.set_masks(P, B, A)
            pl.launch()
            r2 = pl.fetch()
            pl.destroy()
            return np.concatenate([r1, r2])
        call(f"n465_set_masks|{name}", set_after)
        call(f"n465_swapped|{name}", lambda m=m: m.scan(fixed, P, B, A))
    oracle_window("n465_fixed_00|indexed", idx, 3, fixed[3], P, A, B)
    oracle_window("n465_fixed_21|indexed", idx, len(fixed) - 1, fixed[-1], P, A, B, 2, 1)
    oracle_window("n465_sliding|indexed", idx, 5, slide[5], None, A, B)

    # window edges: empty, single-site, mid-block, at site 0 and at n_site
    edges = impop_amd.make_windows([(0, 0, 0), (0, 1, 0), (S - 1, S, 0), (63, 65, 0), (64, 128, 0), (5, 5, 0), (0, S, S), (100, 101, 7),
                                    (77, S, 0), (128, 1000, 1000), (S - 64, S, 0), (S // 2, S // 2 + 37, 0), (S - 37, S, 0), (0, 64, 0)])
    for name, m in (("indexed", idx), ("dense", den)):
        call(f"n465_edges|{name}", lambda m=m: m.scan(edges, P, A, B))
    oracle_window("n465_edges|indexed", idx, 3, edges[3], P, A, B)
    oracle_window("n465_edges|indexed", idx, 12, edges[12], P, A, B)

    # scan_multi (K = 3 disjoint populations)
    pops = [np.arange(n) < 150, (np.arange(n) >= 150) & (np.arange(n) < 300), np.arange(n) >= 300]
    for name, m in (("indexed", idx), ("dense", den)):
        call(f"n465_multi|{name}", lambda m=m: m.scan_multi(slide, pops))

    # impop_matrix_free is refused while an indexed plan lives
    sys.stderr.write("@@call none\n")  # the plans below are not compared call by call
    sys.stderr.flush()
    pl = idx.plan(fixed, None, A, B)
    try:
        idx.free()
        infos["free_refused"] = False
    except impop_amd.ImpopError:
        infos["free_refused"] = True
    pl.destroy()
    infos["n465_bytes_idx"] = idx.plan(fixed, None, A, B).bytes_streamed
    infos["n465_bytes_den"] = den.plan(fixed, None, A, B).bytes_streamed
    import gc
    gc.collect()

    # weighted matrix: weights are indexed by matrix site, so its plans stream the dense layout
    wts = np.random.default_rng(5).integers(1, 200, S).astype(np.uint32)
    for name, m in (("indexed", idx), ("dense", den)):
        m.set_site_weights(wts)
        call(f"weighted|{name}", lambda m=m: m.scan(slide, P, A, B))
        m.set_site_weights(None)
    call("after_weights|indexed", lambda: idx.scan(fixed, P, A, B))
    idx.free(); den.free()

    # n <= 32 (one dword per site) and n > 512 (the any-n kernel)
    for n2, S2, tag in ((20, 64 * 500 + 3, "n20"), (600, 64 * 400 + 7, "n600")):
        P2, A2, B2 = _masks(n2, 2)
        w2 = impop_amd.fixed_windows(S2, 3000, 1000)
        i2, d2 = _pair(ctx, call, tag, lambda d: ctx.synthetic(n2, S2, seed=12, dense_scan=d), lambda m: m.scan(w2, P2, A2, B2))
        infos[tag] = i2.scan_index_info()
        oracle_window(f"{tag}|indexed", i2, 4, w2[4], P2, A2, B2)
        i2.free(); d2.free()

    # a slab that starts at global site 12345
    S3 = 64 * 700 + 11
    w3 = impop_amd.fixed_windows(S3, 4000)
    i3, d3 = _pair(ctx, call, "slab", lambda d: ctx.synthetic(n, S3, seed=13, site_begin=12345, dense_scan=d),
                   lambda m: m.scan(w3, None, A, B))
    oracle_window("slab|indexed", i3, 2, w3[2], None, A, B)
    i3.free(); d3.free()

    # impop_scan_sharded over two contexts: slabs with site_begin != 0, against one whole indexed matrix and its dense twin
    S4 = 64 * 1500 + 29
    w4 = impop_amd.fixed_windows(S4, 6000, 2000)
    whole_i, whole_d = _pair(ctx, call, "sharded_whole", lambda d: ctx.synthetic(n, S4, seed=14, dense_scan=d),
                             lambda m: m.scan(w4, P, A, B))
    ctx2 = impop_amd.Context(0)
    slabs, begins = [], []
    for k, c in enumerate((ctx, ctx2)):
        _, _, b0, b1 = engine.shard_windows_c(w4, 2, k)
        slabs.append(c.synthetic(n, b1 - b0, seed=14, site_begin=b0))
        begins.append(b0)
    call("sharded|indexed", lambda: engine.scan_sharded(slabs, begins, w4, P, A, B))
    for s_ in slabs:
        s_.free()
    whole_i.free(); whole_d.free()
    ctx2.close()

    # uploads: a zero-segregating stretch, an all-monomorphic matrix (index of 0 sites), and one above the 1/4 threshold
    rng = np.random.default_rng(7)
    n5, S5 = 40, 64 * 80 + 21
    m01 = np.repeat((rng.random(S5) < 0.5)[None, :], n5, axis=0).astype(np.uint8)  # monomorphic columns, 0 or 1
    var = rng.random(S5) < 0.08
    var[2000:3000] = False
    m01[:, var] = (rng.random((n5, int(var.sum()))) < 0.3).astype(np.uint8)
    w5 = impop_amd.make_windows([(2000, 3000, 0), (0, S5, 0), (1990, 2010, 0), (2999, 3001, 0), (S5 - 21, S5, 0)]
                                + [(s, min(s + 700, S5), 0) for s in range(0, S5, 500)])
    P5, A5, B5 = _masks(n5, 3)
    i5, d5 = _pair(ctx, call, "upload_zero_seg", lambda d: ctx.upload_dense(m01, keep_hap_major=False, dense_scan=d),
                   lambda m: m.scan(w5, P5, A5, B5))
    infos["upload"] = i5.scan_index_info()
    oracle_window("upload_zero_seg|indexed", i5, 0, w5[0], P5, A5, B5)
    oracle_window("upload_zero_seg|indexed", i5, 3, w5[3], P5, A5, B5)
    i5.free(); d5.free()
    mono = np.repeat((rng.random(S5) < 0.5)[None, :], n5, axis=0).astype(np.uint8)
    i6, d6 = _pair(ctx, call, "upload_monomorphic", lambda d: ctx.upload_dense(mono, keep_hap_major=False, dense_scan=d),
                   lambda m: m.scan(w5, P5, A5, B5))
    infos["monomorphic"] = i6.scan_index_info()
    i6.free(); d6.free()
    dense01 = (rng.random((n5, 5000)) < 0.5).astype(np.uint8)
    i7 = ctx.upload_dense(dense01, keep_hap_major=True)
    infos["above"] = i7.scan_index_info()
    call("upload_above|dense", lambda: i7.scan([(0, 5000), (17, 4000)], None, A5, B5))
    i7.free()

    # graph capture of an indexed plan, and stream ordering: a consumer enqueued right behind a scan of about a millisecond
    # on the same stream (a dense plan: the indexed one is ~15x shorter) must see the finished records
    import torch
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        c3 = impop_amd.Context(0, stream=s.cuda_stream)
        NW, Wn = 2000, 50000
        wins = impop_amd.fixed_windows(NW * Wn, Wn)
        big_i = c3.synthetic(n, NW * Wn, seed=15)
        big_d = c3.synthetic(n, NW * Wn, seed=15, dense_scan=True)
        sys.stderr.write("@@call stream|indexed\n")
        pi_ = big_i.plan(wins, None, A, B)
        sys.stderr.write("@@call stream|dense\n")
        pd_ = big_d.plan(wins, None, A, B)
        sys.stderr.write("@@call none\n")
        out = torch.zeros(NW * 128, dtype=torch.uint8, device="cuda")
        s.synchronize()
        copies = []
        for _ in range(3):
            out.zero_()
            pd_.launch(out.data_ptr())
            copies.append(out.clone())  # same stream, no host sync: ordered behind the scan
        s.synchronize()
        recs["stream_copies|dense"] = np.stack([c.cpu().numpy() for c in copies])
        pi_.launch()
        recs["stream|indexed"] = pi_.fetch()
        pd_.launch()
        recs["stream|dense"] = pd_.fetch()
        g_out = torch.zeros(NW * 128, dtype=torch.uint8, device="cuda")
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            pi_.launch(g_out.data_ptr())
        infos["graph_zero_after_capture"] = int(g_out.sum()) == 0
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        recs["graph|indexed"] = g_out.cpu().numpy()
        del g
        pi_.destroy(); pd_.destroy(); big_i.free(); big_d.free()
        c3.close()
    np.savez(out_path, **{f"r{i}": r for i, r in enumerate(recs.values())}, tags=np.array(json.dumps(list(recs))),
             oracle=np.array(json.dumps(oracle_items)), infos=np.array(json.dumps(infos)))
    ctx.close()


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


def _pairs(recs):
    return sorted(t.split("|")[0] for t in recs if t.endswith("|indexed") and t.split("|")[0] + "|dense" in recs)


def test_indexed_records_equal_dense(run):
    recs, traces, _, _ = run
    pairs = _pairs(recs)
    assert len(pairs) >= 18
    for base in pairs:
        a, b = recs[base + "|indexed"], recs[base + "|dense"]
        assert a.dtype == b.dtype and a.shape == b.shape and len(a) > 0, base
        assert a.tobytes() == b.tobytes(), base
    # two indexed slabs on two contexts == one whole matrix, indexed or dense
    assert recs["sharded|indexed"].tobytes() == recs["sharded_whole|dense"].tobytes()
    # set_masks after create: the second launch equals a fresh scan with those masks; weights set and removed change nothing
    nf = len(recs["n465_swapped|indexed"])
    assert recs["n465_set_masks|indexed"][nf:].tobytes() == recs["n465_swapped|indexed"].tobytes()
    assert recs["after_weights|indexed"].tobytes() == recs["n465_fixed_00|indexed"].tobytes()


def test_routes_from_trace(run):
    recs, traces, _, infos = run
    for tag, lines in traces.items():
        if tag == "none":
            continue
        base, kind = tag.split("|")
        want = "dense" if kind == "dense" or base in ("weighted", "upload_above") else "indexed"
        assert lines, tag
        for d in lines:
            assert d["route"] == want, (tag, d)
            if base == "upload_above":
                assert "above 1/4" in d["why"], (tag, d)
            elif kind == "dense":
                assert d["why"].startswith("opted out"), (tag, d)
            elif base == "weighted":
                assert d["why"] == "site weights", (tag, d)
            else:
                assert d["why"] == "", (tag, d)
    # every scenario that should reach a plan did
    for base in _pairs(recs):
        assert traces.get(base + "|indexed"), base
    assert traces["sharded|indexed"] and all(d["route"] == "indexed" for d in traces["sharded|indexed"])
    assert traces["after_weights|indexed"][0]["route"] == "indexed"  # weights removed: indexed again
    # bytes streamed: what the indexed plan reads, far below the dense stream of the same windows
    assert 0 < infos["n465_bytes_idx"] * 4 < infos["n465_bytes_den"]
    si = traces["stream|indexed"][0]
    sd = traces["stream|dense"][0]
    assert 0 < int(si["kept_sites"]) * 8 < int(sd["kept_sites"]) and si["tiles"] != "0"
    assert int(si["bytes_streamed"]) * 8 < int(sd["bytes_streamed"])


def test_index_info(run):
    _, _, _, infos = run
    for k in ("n465", "n20", "n600", "upload"):
        i = infos[k]
        assert i["index_bytes"] > 0 and i["n_kept"] > 0 and i["why"] == "", (k, i)
    assert infos["n465_dense"] == {"n_kept": 0, "index_bytes": 0, "why": infos["n465_dense"]["why"]}
    assert infos["n465_dense"]["why"].startswith("opted out")
    assert infos["monomorphic"]["n_kept"] == 0 and infos["monomorphic"]["index_bytes"] > 0
    assert infos["above"]["index_bytes"] == 0 and "above 1/4" in infos["above"]["why"]
    assert infos["free_refused"] is True


def test_zero_segregating_and_monomorphic_windows(run):
    recs, _, _, _ = run
    r = recs["upload_zero_seg|indexed"]
    assert int(r[0]["n_sites"]) == 1000 and int(r[0]["s_all"]) == 0 and int(r[0]["sum_p"]) == 0
    m = recs["upload_monomorphic|indexed"]
    assert (m["s_all"] == 0).all() and (m["sum_ab"] == 0).all() and (m["n_sites"] > 0).all()


def test_stream_order_and_graph_capture(run):
    recs, _, _, infos = run
    want = recs["stream|dense"].tobytes()
    assert recs["stream|indexed"].tobytes() == want
    for c in recs["stream_copies|dense"]:
        assert c.tobytes() == want
    assert infos["graph_zero_after_capture"] is True
    assert recs["graph|indexed"].tobytes() == want


def test_sampled_windows_against_oracle(run, oracle):
    recs, _, items, _ = run
    assert len(items) >= 10
    for i, it in enumerate(items):
        n = it["n"]
        bits = recs[f"bits:{i}"]
        flags = lambda v: np.ones(n, np.uint8) if v is None else np.asarray(v, np.uint8)
        want = oracle.window_sitecount(bits, n, 0, it["s1"] - it["s0"], oracle.pack_mask(flags(it["P"])), oracle.pack_mask(flags(it["A"])),
                                       oracle.pack_mask(flags(it["B"])), it["seq_len"], it["mode"], it["scope"])
        got = recs[it["tag"]][it["wi"]]
        for k in INT_KEYS:
            assert int(got[k]) == int(want[k]), (it["tag"], it["wi"], k, int(got[k]), int(want[k]))
        for k in DBL_KEYS:
            assert stat_close(k, float(got[k]), float(want[k]), float(want["dxy"])), (it["tag"], it["wi"], k, float(got[k]), want[k])


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    sys.path.insert(0, ROOT)
    _run_child(sys.argv[2])
