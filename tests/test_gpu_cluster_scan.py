"""GPU: impop_cluster_scan — af.py's clustering per window straight from the bit matrix — against the C oracle
(oracle.af_cluster on oracle identities), the plain reference (plain_refs.ref_components), the reference's own output
(tests/golden/af_windows.json) and itself under every way of computing the same windows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from af_cases import (SEG, THRESHOLD, planted_matrix, seed_only_groups, subset_flags, window_identity, window_lists)
from conftest import GOLDEN, ROOT, golden_bits
from plain_refs import adjacency, ref_components

pytestmark = pytest.mark.gpu

N_SEG = 16
CLUSTER_MAX_N = 12798  # IMPOP_CLUSTER_MAX_N


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


def expected(oracle, bits, n, win, kind, digits, thr, members=None):
    """-> (cluster_of, K, sizes, adjacency) of one window from the oracle; the plain reference must agree with it"""
    t = window_identity(oracle, bits, n, win[0], win[1], kind, digits, members)
    adj = adjacency(t, thr)
    cl, K, sz = oracle.af_cluster(t, thr)
    cl2, K2, sz2 = ref_components(adj)
    assert K == K2 and (cl.astype(np.int64) == cl2).all() and (sz.astype(np.int64) == sz2).all()
    return cl.astype(np.int64), K, sz.astype(np.int64), adj


def check_window(rec, cl_row, sz_row, want, W):
    cl, K, sz, _ = want
    m = len(cl)
    assert int(rec["n_members"]) == m and int(rec["n_clusters"]) == K and int(rec["n_sites"]) == W
    assert (cl_row.astype(np.int64) == cl).all()
    assert (sz_row[:K].astype(np.int64) == sz).all() and not sz_row[K:].any()
    assert int(rec["largest"]) == (int(sz[0]) if K else 0)
    assert int(rec["n_singletons"]) == int((sz == 1).sum())
    assert int(rec["sum_sq"]) == int((sz * sz).sum())


@pytest.mark.parametrize("n", [31, 465, 513, 1030])
@pytest.mark.parametrize("kind", ["match", "dice"])
@pytest.mark.parametrize("digits", [None, 5])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("shape", ["tiling", "sliding"])
def test_exact_parity(ctx, oracle, n, kind, digits, masked, shape):
    """Every window's cluster_of, n_clusters, sizes, largest, n_singletons and sum_sq equal the oracle's and the plain
    reference's.  n <= 512 with `match` runs the window-shape kernel, everything else the general one; the sliding list sums
    elementary segments.  The planted inputs are checked on the oracle's result first: some window is clustered non-trivially,
    has a component that is no clique, and has two clusters of one size."""
    m01 = planted_matrix(n, N_SEG, 7000 + n)
    bits = oracle.pack_hap_major(m01)
    wins = window_lists(N_SEG)[shape]
    assert len(wins) >= 8
    flags = subset_flags(n) if masked else None
    members = np.flatnonzero(flags) if masked else None
    want = [expected(oracle, bits, n, w, kind, digits, THRESHOLD, members) for w in wins]
    nP = len(want[0][0])
    assert any(1 < K < nP for _, K, _, _ in want)
    assert any(len(set(sz.tolist())) < len(sz) for _, _, sz, _ in want)
    def has_open_component(cl, adj):
        a = adj | adj.T
        same = cl[:, None] == cl[None, :]
        return bool((same & ~a & ~np.eye(len(cl), dtype=bool)).any()) and len(set(seed_only_groups(a).tolist())) != len(set(cl.tolist()))
    assert any(has_open_component(cl, adj) for cl, _, _, adj in want)
    bm = ctx.upload(bits, m01.shape[1], keep_hap_major=True)
    try:
        rec, cl, sz = bm.cluster_scan(wins, mask_p=flags, kind=kind, threshold=THRESHOLD, round_digits=digits)
        assert cl.shape == (len(wins), nP) and sz.shape == (len(wins), nP)
        for k, w in enumerate(wins):
            check_window(rec[k], cl[k], sz[k], want[k], w[1] - w[0])
        only = bm.cluster_scan(wins, mask_p=flags, kind=kind, threshold=THRESHOLD, round_digits=digits, want_members=False)
        assert only.tobytes() == rec.tobytes()
    finally:
        bm.free()


@pytest.mark.parametrize("W,thr,digits", [(1000, 0.999, None), (997, 0.999, 5)])
def test_non_strict_compare(ctx, oracle, W, thr, digits):
    """af.py:38 links at identity >= threshold.  W = 1000: a pair one site apart has identity 999/1000 == 0.999 exactly.
    W = 997 with -r 5: 996/997 = 0.998996... rounds to 0.999 exactly.  Either way `>=` and `>` cluster the input differently
    (checked on the oracle first), and the GPU gives the `>=` answer — from both kernel forms."""
    rng = np.random.default_rng(W)
    n = 40
    m01 = np.zeros((n, W + 30), np.uint8)
    base = rng.integers(0, 2, size=W + 30, dtype=np.uint8)
    for i in range(n):
        m01[i] = base
        if i >= 8:
            m01[i, rng.choice(W, size=40, replace=False)] ^= 1
    for i in range(1, 8):  # a chain: i differs from i - 1 at exactly one site of the window
        m01[i] = m01[i - 1]
        m01[i, 10 * i] ^= 1
    bits = oracle.pack_hap_major(m01)
    t = window_identity(oracle, bits, n, 0, W, "match", digits)
    assert t[0, 1] == thr
    with np.errstate(invalid="ignore"):
        strict = ref_components(t > thr)
    loose = ref_components(adjacency(t, thr))
    assert strict[1] != loose[1]
    cl_o, K_o, sz_o = oracle.af_cluster(t, thr)
    assert K_o == loose[1] and (cl_o == loose[0]).all()
    bm = ctx.upload(bits, m01.shape[1], keep_hap_major=True)
    try:
        rec, cl, sz = bm.cluster_scan([(0, W, W)], kind="match", threshold=thr, round_digits=digits)
        check_window(rec[0], cl[0], sz[0], (loose[0], loose[1], loose[2], None), W)
    finally:
        bm.free()
    got = run_variant(dict(n=n, seed=W, special="nonstrict", W=W, thr=thr, digits=digits), {"IMPOP_EPILOGUE_SMALL": "0"})
    assert (got["cl"][0].astype(np.int64) == loose[0]).all() and int(got["rec"][0]["n_clusters"]) == loose[1]


# ---- the same windows computed in every other way: byte-identical records and tables -----------------------------------

VARIANT = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import impop_amd
from af_cases import planted_matrix, window_lists, THRESHOLD
from oracle import oracle as orc
spec = json.loads(sys.argv[2])
ctx = impop_amd.Context(0)
if spec.get("special") == "nonstrict":
    W, n = spec["W"], spec["n"]
    rng = np.random.default_rng(W)
    m01 = np.zeros((n, W + 30), np.uint8)
    base = rng.integers(0, 2, size=W + 30, dtype=np.uint8)
    for i in range(n):
        m01[i] = base
        if i >= 8:
            m01[i, rng.choice(W, size=40, replace=False)] ^= 1
    for i in range(1, 8):
        m01[i] = m01[i - 1]
        m01[i, 10 * i] ^= 1
    wins, thr, digits = [(0, W, W)], spec["thr"], spec["digits"]
else:
    m01 = planted_matrix(spec["n"], 16, spec["seed"])
    wins, thr, digits = window_lists(16)[spec["shape"]], THRESHOLD, spec.get("digits")
bm = ctx.upload(orc.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
rec, cl, sz = bm.cluster_scan(wins, kind=spec.get("kind", "match"), threshold=thr, round_digits=digits)
np.savez(sys.argv[3], rec=rec, cl=cl, sz=sz)
bm.free(); ctx.close()
'''


def run_variant(spec, env_extra):
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "r.npz")
        env = dict(os.environ, **env_extra)
        r = subprocess.run([sys.executable, "-c", VARIANT, ROOT, json.dumps(spec), out], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        with np.load(out) as z:
            return {k: z[k].copy() for k in z.files}


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("rec", "cl", "sz"))


@pytest.mark.parametrize("n,kind", [(465, "match"), (513, "match"), (465, "dice")])
@pytest.mark.parametrize("shape", ["tiling", "sliding"])
def test_invariance_under_gram_and_chunk_switches(ctx, oracle, n, kind, shape):
    """uint16 counts off, the Gram chains forced to 1 and to 8 links, three windows per chunk, the window-shape kernel off:
    the records and tables of the default run, byte for byte (each switch is read once per process: a child each)."""
    spec = dict(n=n, seed=7000 + n, shape=shape, kind=kind)
    m01 = planted_matrix(n, N_SEG, 7000 + n)
    bm = ctx.upload(oracle.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
    try:
        rec, cl, sz = bm.cluster_scan(window_lists(N_SEG)[shape], kind=kind, threshold=THRESHOLD)
    finally:
        bm.free()
    base = dict(rec=rec, cl=cl, sz=sz)
    for env in ({"IMPOP_GRAM_U16": "0"}, {"IMPOP_GRAM_CHAIN": "1"}, {"IMPOP_GRAM_CHAIN": "8"}, {"IMPOP_PAIRWISE_CHUNK": "3"},
                {"IMPOP_EPILOGUE_SMALL": "0"}):
        assert same(base, run_variant(spec, env)), env


@pytest.mark.parametrize("kind", ["match", "dice"])
def test_invariance_compacted_alone_and_in_a_list(ctx, oracle, kind):
    """The matrix compacted to its variable sites (all-ones sites come back as the per-window constant) and a window scanned
    alone give what the full matrix and the list give."""
    n = 465
    m01 = planted_matrix(n, N_SEG, 7000 + n)
    m01[:, 5::17] = 1   # monomorphic columns: all haplotypes carry them ...
    m01[:, 9::23] = 0   # ... or none does
    bits = oracle.pack_hap_major(m01)
    full = ctx.upload(bits, m01.shape[1], keep_hap_major=True)
    try:
        for shape, wins in window_lists(N_SEG).items():
            a = full.cluster_scan(wins, kind=kind, threshold=THRESHOLD, round_digits=5)
            comp = full.compact()
            try:
                b = comp.cluster_scan(wins, kind=kind, threshold=THRESHOLD, round_digits=5)
            finally:
                comp.free()
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), shape
            for k in (0, len(wins) // 2, len(wins) - 1):
                c = full.cluster_scan([wins[k]], kind=kind, threshold=THRESHOLD, round_digits=5)
                assert c[0].tobytes() == a[0][k:k + 1].tobytes() and (c[1][0] == a[1][k]).all() and (c[2][0] == a[2][k]).all()
            want = expected(oracle, bits, n, wins[1], kind, 5, THRESHOLD)
            check_window(a[0][1], a[1][1], a[2][1], want, wins[1][1] - wins[1][0])
    finally:
        full.free()


@pytest.mark.parametrize("heavy", [False, True])
def test_invariance_weighted_against_bp_expanded(ctx, oracle, heavy):
    """A node-level matrix with site weights clusters like its bp-expanded matrix (every column repeated weight times).  With
    one weight >= 65536 the windows that hold it pass 2^16 sites: int32 counts."""
    rng = np.random.default_rng(99)
    n, cols = 120, 400
    node = planted_matrix(n, 4, 4242)[:, :cols]
    wt = rng.integers(1, 6, size=cols).astype(np.uint32)
    if heavy:
        wt[37] = 70000
        node[:, 37] = 1      # a long anchor every haplotype carries (as real graphs have them)
        node[::2, 300] ^= 1
    expanded = np.repeat(node, wt, axis=1)
    edges = np.concatenate([[0], np.cumsum(wt.astype(np.int64))])
    node_wins = [(s, min(s + 50, cols), 0) for s in range(0, cols, 50)] + [(s, min(s + 100, cols), 0) for s in range(0, cols - 50, 50)]
    bp_wins = [(int(edges[a]), int(edges[b]), 0) for a, b, _ in node_wins]
    thr = 0.97
    bw = ctx.upload(oracle.pack_hap_major(node), cols, keep_hap_major=True)
    be = ctx.upload(oracle.pack_hap_major(expanded), expanded.shape[1], keep_hap_major=True)
    try:
        bw.set_site_weights(wt)
        for kind in ("match", "dice"):
            a = bw.cluster_scan(node_wins, kind=kind, threshold=thr)
            b = be.cluster_scan(bp_wins, kind=kind, threshold=thr)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), kind
            assert any(1 < int(r["n_clusters"]) < n for r in a[0])
            if heavy:
                assert int(a[0]["n_sites"].max()) >= 65536
        comp = bw.compact()
        try:
            c = comp.cluster_scan(node_wins, kind="match", threshold=thr)
        finally:
            comp.free()
        a = bw.cluster_scan(node_wins, kind="match", threshold=thr)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, c))
    finally:
        bw.free(); be.free()


# ---- against the real reference -------------------------------------------------------------------------------------------

def test_reference_af_clusters_and_driver_rows(ctx, tmp_path):
    """tests/golden/af_windows.json holds what the reference's af.cluster + build_summary + write_summary make of each window's
    .sim rows.  impop_amd.af.cluster_windows returns the same lists, and `impop_scan.py --format af --af-clusters` the same rows
    behind its REGION column, byte for byte."""
    from impop_amd import af
    import impop_amd
    from impop_amd import matrixio
    with open(os.path.join(GOLDEN, "af_windows.json")) as f:
        gold = json.load(f)
    assert any(c["names"] != sorted(c["names"]) for c in gold["cases"])
    assert any(w["threshold"] == 1.0 for c in gold["cases"] for w in c["windows"])
    for ci, case in enumerate(gold["cases"]):
        bits = golden_bits(case)
        bm = ctx.upload(bits, case["n_site"], keep_hap_major=True)
        try:
            by_thr = {}
            for w in case["windows"]:
                by_thr.setdefault(w["threshold"], []).append(w)
            for thr, ws in by_thr.items():
                got = af.cluster_windows(bm, [(w["begin"], w["end"], w["end"] - w["begin"]) for w in ws], case["names"], thr)
                for w, g in zip(ws, got):
                    assert g == w["clusters"], (ci, w["begin"], thr)
        finally:
            bm.free()
        # the driver on the same matrix
        npz, bed = str(tmp_path / f"m{ci}.npz"), str(tmp_path / f"w{ci}.bed")
        matrixio.save_matrix(npz, matrixio.from_dense(impop_amd.unpack_hap_major(bits, case["n_site"]), case["names"], origin=0,
                                                       contig="REF#0#chrT"))
        for thr, ws in by_thr.items():
            with open(bed, "w") as f:
                for w in ws:
                    f.write(f"chrT\t{w['begin']}\t{w['end']}\n")
            side = str(tmp_path / "clusters.tsv")
            r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", npz, "--bed", bed, "--format", "af",
                                "-t", repr(thr), "--af-clusters", side, "-p", "REF#0#"], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            with open(side, newline="") as f:
                text = f.read()
            want = "REGION\tcluster_id\tcount\tfrequency\r\n"
            for w in ws:
                reg = f"REF#0#chrT:{w['begin']}-{w['end']}"
                want += "".join(f"{reg}\t{line}\r\n" for line in w["summary_rows"])
            assert text == want
            lines = r.stdout.splitlines()
            assert lines[0] == "REGION\tLENGTH\tTHRESHOLD\tHAPLOTYPES\tCLUSTERS\tLARGEST\tSINGLETONS\tHOMOZYGOSITY"
            for w, line in zip(ws, lines[1:]):
                sizes = [len(c) for c in w["clusters"]]
                tot = sum(sizes)
                hom = sum(s * s for s in sizes) / (tot * tot)
                assert line == (f"REF#0#chrT:{w['begin']}-{w['end']}\t{w['end'] - w['begin']}\t{thr!r}\t{tot}\t{len(sizes)}\t{max(sizes)}\t"
                                f"{sizes.count(1)}\t{hom:.6f}")


# ---- limits and degenerate shapes -----------------------------------------------------------------------------------------

def test_limit_is_refused_before_any_launch(ctx):
    import impop_amd
    n = CLUSTER_MAX_N + 1
    bm = ctx.upload(np.zeros((n, 1), np.uint64), 64, keep_hap_major=True)
    try:
        with pytest.raises(impop_amd.ImpopError) as e:
            bm.cluster_scan([(0, 64, 64)])
        assert e.value.code == -1 and str(CLUSTER_MAX_N) in e.value.message
        flags = np.ones(n, np.uint8); flags[-1] = 0   # one member fewer: accepted
        rec = bm.cluster_scan([(0, 64, 64)], mask_p=flags, want_members=False)
        assert int(rec[0]["n_members"]) == CLUSTER_MAX_N and int(rec[0]["n_clusters"]) == 1 and int(rec[0]["largest"]) == CLUSTER_MAX_N
    finally:
        bm.free()


@pytest.mark.parametrize("kind", ["match", "dice"])
def test_degenerate_shapes(ctx, oracle, kind):
    """|P| = 0, |P| = 1, a window without sites and an empty window list each return a defined result."""
    n = 50
    m01 = planted_matrix(n, 2, 5)
    bm = ctx.upload(oracle.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
    try:
        rec, cl, sz = bm.cluster_scan([], kind=kind)
        assert len(rec) == 0 and cl.shape == (0, n)
        rec, cl, sz = bm.cluster_scan([(0, 200, 200), (7, 7, 0)], mask_p=np.zeros(n, np.uint8), kind=kind)
        assert cl.shape == (2, 0) and all(int(r["n_members"]) == 0 and int(r["n_clusters"]) == 0 and int(r["sum_sq"]) == 0 for r in rec)
        one = np.zeros(n, np.uint8); one[17] = 1
        rec, cl, sz = bm.cluster_scan([(0, 200, 200)], mask_p=one, kind=kind)
        assert (int(rec[0]["n_clusters"]), int(rec[0]["largest"]), int(rec[0]["n_singletons"]), int(rec[0]["sum_sq"])) == (1, 1, 1, 1)
        assert cl.tolist() == [[0]] and sz.tolist() == [[1]]
        # an empty window: identity 1.0 for every pair — one cluster of everybody; next to a real window in the same call
        rec, cl, sz = bm.cluster_scan([(30, 30, 0), (0, 256, 256), (256, 256, 0)], kind=kind, threshold=THRESHOLD)
        for k in (0, 2):
            assert int(rec[k]["n_sites"]) == 0 and int(rec[k]["n_clusters"]) == 1 and int(rec[k]["largest"]) == n
            assert int(rec[k]["sum_sq"]) == n * n and not cl[k].any() and sz[k].tolist() == [n] + [0] * (n - 1)
        want = expected(oracle, oracle.pack_hap_major(m01), n, (0, 256), kind, None, THRESHOLD)
        check_window(rec[1], cl[1], sz[1], want, 256)
    finally:
        bm.free()


def test_config5_shape_through_the_general_form(ctx, oracle):
    """One window of 4096 haplotypes (more than the window-shape kernel holds; over 48 KiB of dynamic LDS in the general one)."""
    n = 4096
    m01 = planted_matrix(n, 2, 4096)
    bits = oracle.pack_hap_major(m01)
    bm = ctx.upload(bits, m01.shape[1], keep_hap_major=True)
    try:
        rec, cl, sz = bm.cluster_scan([(0, 2 * SEG, 2 * SEG)], threshold=THRESHOLD)
    finally:
        bm.free()
    t = window_identity(oracle, bits, n, 0, 2 * SEG, "match", None)
    cl_w, K_w, sz_w = ref_components(adjacency(t, THRESHOLD))
    assert 1 < K_w < n
    check_window(rec[0], cl[0], sz[0], (cl_w, K_w, sz_w, None), 2 * SEG)


def test_device_error_word_fails_the_call(ctx, oracle):
    """The call checks the device error word like impop_pairwise_scan: a raised bit fails it (IMPOP_E_INTERNAL) and is cleared."""
    import ctypes as C
    import impop_amd
    m01 = planted_matrix(40, 2, 3)
    bm = ctx.upload(oracle.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
    try:
        impop_amd.engine.check(ctx._lib.impop_debug_raise_device_error(ctx.handle, C.c_uint32(2)))
        with pytest.raises(impop_amd.ImpopError) as e:
            bm.cluster_scan([(0, 256, 256)])
        assert e.value.code == -6
        rec = bm.cluster_scan([(0, 256, 256)], want_members=False)
        assert int(rec[0]["n_members"]) == 40
    finally:
        bm.free()


def test_driver_subset_compact_dice_details(ctx, tmp_path):
    """`impop_scan.py --format af -u subset --compact --identity dice --af-details`: the main table and both side tables are
    what impop_amd.af.cluster_windows returns for the same members, identity and threshold on the uncompacted matrix."""
    import importlib.util
    import impop_amd
    from impop_amd import af, matrixio
    with open(os.path.join(GOLDEN, "af_windows.json")) as f:
        case = json.load(f)["cases"][1]   # names out of index order
    bits, names, S = golden_bits(case), case["names"], case["n_site"]
    npz, bed, sub = str(tmp_path / "m.npz"), str(tmp_path / "w.bed"), str(tmp_path / "subset.txt")
    matrixio.save_matrix(npz, matrixio.from_dense(impop_amd.unpack_hap_major(bits, S), names, origin=0, contig="REF#0#chrT"))
    wins = [(0, 200), (100, 300), (150, 450), (0, S)]
    with open(bed, "w") as f:
        f.writelines(f"chrT\t{b}\t{e}\n" for b, e in wins)
    with open(sub, "w") as f:
        f.write("HG000\nHG001#1\nHG002\nHG003\nHG004#2\nHG005\nHG006\n")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("impop_scan_cli_af_gpu", os.path.join(ROOT, "scripts", "impop_scan.py"))
        cli = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(cli)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    mask = cli.flags_for(sub, names)
    assert 2 < int(mask.sum()) < len(names)
    thr = 0.98
    bm = ctx.upload(bits, S, keep_hap_major=True)
    try:
        want = af.cluster_windows(bm, [(b, e, e - b) for b, e in wins], names, thr, mask_p=mask, kind="dice")
    finally:
        bm.free()
    assert any(1 < len(c) < int(mask.sum()) for c in want)
    clusters, details = str(tmp_path / "c.tsv"), str(tmp_path / "d.tsv")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", npz, "--bed", bed, "--format", "af", "-t", "0.98",
                        "-u", sub, "--compact", "--identity", "dice", "--af-clusters", clusters, "--af-details", details, "-p", "REF#0#"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    regions = [f"REF#0#chrT:{b}-{e}" for b, e in wins]
    want_c, want_d = "REGION\tcluster_id\tcount\tfrequency\r\n", "REGION\tsample_id\tcluster_id\tthreshold\r\n"
    lines = r.stdout.splitlines()
    assert len(lines) == 1 + len(wins)
    for reg, (b, e), cl, line in zip(regions, wins, want, lines[1:]):
        summary = af.build_summary(cl)
        want_c += "".join(f"{reg}\t{cid}\t{size}\t{freq:.6f}\r\n" for cid, size, freq, _ in summary)
        want_d += "".join(f"{reg}\t{s}\t{cid}\t{thr}\r\n" for cid, _, _, members in summary for s in members)
        sizes = [len(c) for c in cl]
        tot = sum(sizes)
        assert tot == int(mask.sum())
        assert line == f"{reg}\t{e - b}\t0.98\t{tot}\t{len(sizes)}\t{max(sizes)}\t{sizes.count(1)}\t{sum(s * s for s in sizes) / (tot * tot):.6f}"
    assert open(clusters, newline="").read() == want_c
    assert open(details, newline="").read() == want_d


def test_driver_refuses_rows_that_share_a_cut_name(tmp_path):
    import impop_amd
    from impop_amd import matrixio
    m = np.zeros((4, 128), np.uint8)
    names = ["A#1#chrT:0-64", "A#1#chrT:64-128", "B#1#chrT:0-128", "B#2#chrT:0-128"]
    npz, bed = str(tmp_path / "m.npz"), str(tmp_path / "w.bed")
    matrixio.save_matrix(npz, matrixio.from_dense(m, names, origin=0, contig="REF#0#chrT"))
    with open(bed, "w") as f:
        f.write("chrT\t0\t100\n")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", npz, "--bed", bed, "--format", "af", "-p", "REF#0#"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "distinct sequence names" in r.stderr and r.stdout == ""
