"""GPU: impop_genotypes_* and impop_kinship_scan — joint genotype tables and KING kinship per pair of individuals from the Gram
pass over the genotype planes — against the plain restatement (tests/plain_kinship.py, byte for byte), against impop_diploid_scan
and impop_pairwise_counts on the same windows, and against itself under every way of computing the same windows."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import kinship_cases as kc
import plain_kinship as pk
from conftest import ROOT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_N, MAX_WATCH = 2048, 1024  # IMPOP_KINSHIP_MAX_N, IMPOP_KINSHIP_MAX_WATCH


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def reference(N, shape):
    """the plain reference of a parity case, computed once"""
    return pk.scan(kc.matrix(N), kc.pairs(N), kc.window_lists()[shape], kc.KIN, kc.watch(N))


@pytest.fixture(scope="module")
def planes_of(ctx):
    """the case matrices' genotype planes on the device, one build per N; the source matrix is freed at once"""
    import impop_amd
    held = {}

    def get(N):
        if N not in held:
            m01 = kc.matrix(N)
            bm = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=False)
            held[N] = bm.genotypes(kc.pairs(N))
            bm.free()
        return held[N]
    yield get
    for g in held.values():
        g.free()


def blob(res):
    return b"".join(a.tobytes() for a in res if a is not None)


def assert_equal(got, want, what=""):
    """field by field for a readable failure, then byte for byte"""
    for g, w, kind in zip(got, want, ("window", "pair", "watch")):
        if g is None:
            continue
        assert g.shape == w.shape, (what, kind, g.shape, w.shape)
        for f in w.dtype.names:
            bad = np.argwhere(g[f] != w[f])
            assert not len(bad), (what, kind, f, bad[:4].tolist(), g[f][tuple(bad[0])], w[f][tuple(bad[0])])
        assert g.tobytes() == w.tobytes(), (what, kind)


def unpack(words, n_site):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")[:, :n_site]


# ---- the planes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [2, 3, 16, 17, 48, 49])
def test_planes_are_xor_and_and(ctx, N):
    """download() equals numpy XOR / AND: n_site no multiple of 64, ranges that start and end inside a block, pairs that are
    non-adjacent and in either order, one haplotype unpaired (N = 3: the seventh)"""
    import impop_amd
    S = 1000 + N  # never a multiple of 64
    m01 = kc.matrix(N)[:, :S].copy()
    pr = kc.pairs(N)
    assert (pr[:, 0] > pr[:, 1]).any() and (np.abs(pr[:, 0].astype(int) - pr[:, 1].astype(int)) > 1).any() and m01.shape[0] == 2 * N + 1
    want = pk.planes(m01, pr)
    bm = ctx.upload(impop_amd.pack_hap_major(m01), S, keep_hap_major=False)
    try:
        g = bm.genotypes(pr)
    finally:
        bm.free()  # the handle owns its memory
    try:
        assert (g.n_ind, g.n_site) == (N, S) and g.device_bytes > 0
        assert (unpack(g.download(), S) == want).all()
        for b, e in ((0, 64), (1, 63), (63, 65), (100, 100 + 129), (S - 70, S), (S - 1, S), (64, 640)):
            got = g.download(b, e)
            assert got.shape == (2 * N, max((e - b + 63) // 64, 1))
            assert (unpack(got, e - b) == want[:, b:e]).all(), (b, e)
            assert blob([got]) == blob([impop_amd.pack_hap_major(want[:, b:e])]), (b, e)  # the bits past the range are zero
        swapped = None
        bm = ctx.upload(impop_amd.pack_hap_major(m01), S, keep_hap_major=True)
        try:
            swapped = bm.genotypes(pr[:, ::-1])
            assert blob([swapped.download()]) == blob([g.download()])
        finally:
            bm.free()
            if swapped is not None:
                swapped.free()
    finally:
        g.free()


# ---- parity ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["tiling", "sliding"])
@pytest.mark.parametrize("N", [2, 3, 48, 49, 232])
def test_exact_parity(planes_of, N, shape):
    """Every integer of every record equals the restatement's, with and without the pair totals and the watch rows.  The planted
    features are asserted on the reference first."""
    from impop_amd import kinship as kin
    wins, watch = kc.window_lists()[shape], kc.watch(N)
    want = reference(N, shape)
    ww, wp, wt = want
    assert any(int(w["n_sites"]) == 0 for w in ww) and any(int(w["n_sites"]) == 1 for w in ww)
    dup = wp["t"][kin.pair_index(N, 0, 1)].astype(np.int64)
    n, a, b, hh, i0, _, _ = kin.cells(dup)
    assert i0 == 0 and a == b == hh > 0 and kin.king_robust(a, b, hh, i0) == 0.5
    if N >= 3:
        _, a, b, hh, i0, _, _ = kin.cells(wp["t"][kin.pair_index(N, 0, 2)])
        assert i0 == 0 and hh > 0 and (a != hh or b != hh)  # parent and child, not a duplicate
    if N >= 5:
        assert any(int(w["n_undefined"]) > 0 and int(w["n_sites"]) > 1 for w in ww)
        assert any(0 < int(w["n_related"]) < int(w["n_pairs"]) for w in ww)
        assert (wt[:, 3]["het_i"] == 0).any()  # the homozygous stretch of individual 4, seen through a watched pair
    g = planes_of(N)
    got = g.kinship_scan(wins, kin=kc.KIN, watch=watch)
    assert_equal(got, want, (N, shape))
    assert blob(g.kinship_scan(wins, kin=kc.KIN, watch=watch)) == blob(got)  # identical bytes from call to call
    lean = g.kinship_scan(wins, kin=kc.KIN, watch=None, want_pairs=False)
    assert lean[1] is None and lean[2] is None and blob(lean[:1]) == blob(got[:1])
    assert blob(g.kinship_scan(wins, kin=kc.KIN, watch=watch, want_pairs=False)[2:]) == blob(got[2:])
    for num in (0, kc.KIN[1]):  # the ends of the threshold's range
        assert_equal(g.kinship_scan(wins, kin=(num, kc.KIN[1]), want_pairs=False)[:1],
                     pk.scan(kc.matrix(N), kc.pairs(N), wins, (num, kc.KIN[1]))[:1], (N, shape, num))


def test_int32_gram_counts(ctx):
    """one window of 70 000 sites: the counts pass 2^16"""
    import impop_amd
    rng = np.random.default_rng(70000)
    N, S = 4, 70000
    m01 = rng.integers(0, 2, size=(9, S), dtype=np.uint8)
    m01[:, ::3] = 1  # alt_i and AA above 2^16 / 4
    pr = kc.pairs(N)
    wins = [(0, S, S), (5, 66000, 0)]
    want = pk.scan(m01, pr, wins, kc.KIN, [(0, 3)])
    assert int(want[1]["t"].max()) > 20000 and int(want[0]["n_sites"][0]) == S
    bm = ctx.upload(impop_amd.pack_hap_major(m01), S, keep_hap_major=False)
    try:
        g = bm.genotypes(pr)
        try:
            assert_equal(g.kinship_scan(wins, kin=kc.KIN, watch=[(0, 3)]), want)
        finally:
            g.free()
    finally:
        bm.free()


def test_upper_end_of_the_individual_range(ctx):
    """2048 individuals, the documented limit, over one 256-site window"""
    import impop_amd
    rng = np.random.default_rng(2048)
    N, S = MAX_N, 256
    m01 = rng.integers(0, 2, size=(2 * N, S), dtype=np.uint8)
    pr = np.arange(2 * N, dtype=np.uint32).reshape(N, 2)
    m01[pr[2000]] = m01[pr[7]]  # a duplicate far from its original
    want = pk.scan(m01, pr, [(0, S, S)], kc.KIN, [(2000, 7), (2047, 0)])
    assert int(want[0]["n_related"][0]) >= 1 and int(want[2][0, 0]["ibs0"]) == 0
    bm = ctx.upload(impop_amd.pack_hap_major(m01), S, keep_hap_major=False)
    try:
        g = bm.genotypes(pr)
        try:
            assert_equal(g.kinship_scan([(0, S, S)], kin=kc.KIN, watch=[(2000, 7), (2047, 0)]), want, "N = 2048")
        finally:
            g.free()
    finally:
        bm.free()


# ---- the same windows computed in every other way: byte-identical records ------------------------------------------------------------

def _child(path, N, shape):
    import impop_amd
    ctx = impop_amd.Context(0)
    m01 = kc.matrix(N)
    bm = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=False)
    g = bm.genotypes(kc.pairs(N))
    got = g.kinship_scan(kc.window_lists()[shape], kin=kc.KIN, watch=kc.watch(N))
    np.savez(path, w=got[0], p=got[1], t=got[2])
    g.free(); bm.free(); ctx.close()


def run_child(N, shape, env_extra):
    """-> (result, trace fields of the [impop_kinship_scan] line)"""
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]), **env_extra)
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_kinship_scan as t; t._child(sys.argv[1], %d, %r)" % (N, shape), path],
                           capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = [l for l in r.stderr.splitlines() if l.startswith("[impop_kinship_scan] route=")]
        assert len(lines) == 1, r.stderr[-2000:]
        trace = dict(f.split("=") for f in lines[0].split()[1:])
        with np.load(path) as z:
            return (z["w"].copy(), z["p"].copy(), z["t"].copy()), trace


@pytest.mark.parametrize("shape", ["tiling", "sliding"])
def test_invariance_under_gram_and_chunk_switches(planes_of, shape):
    """one and three windows per chunk (the chunk count read from the trace line), int32 Gram counts, Gram chains of 1 and of 8
    links: the bytes of the default run (each switch is read by a fresh process); and the trace line's fields"""
    N = 49
    wins = kc.window_lists()[shape]
    base = planes_of(N).kinship_scan(wins, kin=kc.KIN, watch=kc.watch(N))
    assert_equal(base, reference(N, shape))
    same, trace = run_child(N, shape, {})
    assert blob(same) == blob(base)
    assert set(trace) == {"route", "individuals", "rows", "windows", "chunks", "launches", "watch", "plane_bytes"}
    assert trace["route"] == "dense" and int(trace["individuals"]) == N and int(trace["rows"]) == 192 and int(trace["windows"]) == len(wins)
    # the window kernel, and the totals kernel with its reduce pass (a chunk of several windows is cut into slices)
    assert int(trace["chunks"]) == 1 and int(trace["launches"]) == 3 and int(trace["watch"]) == len(kc.watch(N))
    assert int(trace["plane_bytes"]) == planes_of(N).device_bytes
    for env in ({"IMPOP_PAIRWISE_CHUNK": "1"}, {"IMPOP_PAIRWISE_CHUNK": "3"}, {"IMPOP_GRAM_U16": "0"}, {"IMPOP_GRAM_CHAIN": "1"},
                {"IMPOP_GRAM_CHAIN": "8"}):
        got, trace = run_child(N, shape, env)
        assert blob(got) == blob(base), env
        if "IMPOP_PAIRWISE_CHUNK" in env:
            k = int(env["IMPOP_PAIRWISE_CHUNK"])
            assert int(trace["chunks"]) >= (len(wins) + k - 1) // k
            assert int(trace["launches"]) == 2 * int(trace["chunks"]) if k == 1 else 2 * int(trace["chunks"]) <= int(trace["launches"]) <= 3 * int(trace["chunks"])


def test_invariance_compacted_source_and_swapped_copies(ctx):
    """planes built from the compacted source (planted all-ones and all-zeros columns) and planes built with h1 and h2 swapped give
    the bytes of the planes of the full matrix, which are the restatement's"""
    import impop_amd
    N = 49
    m01 = kc.matrix(N).copy()
    m01[:, 5::17] = 1
    m01[:, 9::23] = 0
    pr, watch = kc.pairs(N), kc.watch(N)
    full = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
    try:
        comp = full.compact()
        assert comp.n_site < full.n_site
        gf, gc, gs = full.genotypes(pr), comp.genotypes(pr), full.genotypes(pr[:, ::-1])
        comp.free()
        try:
            assert gc.n_site == comp.n_site and gf.n_site == full.n_site
            for shape, wins in kc.window_lists().items():
                a = gf.kinship_scan(wins, kin=kc.KIN, watch=watch)
                assert_equal(a, pk.scan(m01, pr, wins, kc.KIN, watch), shape)
                assert blob(gc.kinship_scan(wins, kin=kc.KIN, watch=watch)) == blob(a), shape
                assert blob(gs.kinship_scan(wins, kin=kc.KIN, watch=watch)) == blob(a), shape
        finally:
            gf.free(); gc.free(); gs.free()
    finally:
        full.free()


# ---- cross-checks against existing calls ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["tiling", "sliding"])
def test_cross_checks_against_diploid_scan_and_pairwise_counts(ctx, shape):
    """het_i of a watched pair and the margins of a one-window table equal impop_diploid_scan's het / hom_alt; the table's squared
    genotype distance equals the four haplotype Hamming distances minus the two het counts, from impop_pairwise_counts"""
    import impop_amd
    N = 17
    m01, pr = kc.matrix(N), kc.pairs(N)
    wins = [w for w in kc.window_lists()[shape] if w[1] > w[0]]
    watch = [(i, (i + 1) % N) for i in range(N)]
    bm = ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)
    try:
        g = bm.genotypes(pr)
        try:
            _, ind = bm.diploid_scan(wins, pr, min_run=1, want_individuals=True)
            _, _, wat = g.kinship_scan(wins, kin=kc.KIN, watch=watch, want_pairs=False)
            assert (wat["het_i"] == ind["het"]).all() and (wat["het_j"] == np.roll(ind["het"], -1, axis=1)).all()
            order = pk.pair_order(N)
            d2 = np.array([(a - b) ** 2 for a in range(3) for b in range(3)], np.int64)
            for k, w in enumerate(wins[:4]):
                _, tot, _ = g.kinship_scan([w], kin=kc.KIN)
                t = tot["t"].astype(np.int64)
                I = bm.pairwise_counts(w[0], w[1]).astype(np.int64)
                H = np.diag(I)[:, None] + np.diag(I)[None, :] - 2 * I
                for p, (i, j) in enumerate(order):
                    assert t[p, 3:6].sum() == ind[k, i]["het"] and t[p, 6:9].sum() == ind[k, i]["hom_alt"]
                    assert t[p, 1::3].sum() == ind[k, j]["het"] and t[p, 2::3].sum() == ind[k, j]["hom_alt"]
                    four = H[pr[i, 0], pr[j, 0]] + H[pr[i, 0], pr[j, 1]] + H[pr[i, 1], pr[j, 0]] + H[pr[i, 1], pr[j, 1]]
                    assert (d2 * t[p]).sum() == four - int(ind[k, i]["het"]) - int(ind[k, j]["het"]), (k, i, j)
        finally:
            g.free()
    finally:
        bm.free()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def raw_create(ctx, bm, pairs):
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.uint32).reshape(-1, 2))
    out = C.c_void_p()
    rc = ctx._lib.impop_genotypes_create(ctx.handle, bm.handle, pr.ctypes.data_as(C.POINTER(C.c_uint32)), len(pr), C.byref(out))
    msg = ctx._lib.impop_last_error().decode()
    if rc == 0:
        ctx._lib.impop_genotypes_free(ctx.handle, out)
    return rc, msg


def raw_scan(ctx, g, wins, kin=kc.KIN, watch=(), n_watch=None, struct_size=None):
    import impop_amd
    from impop_amd import _lib
    w = impop_amd.make_windows(wins)
    wa = np.ascontiguousarray(np.asarray(list(watch) or [(0, 0)], dtype=np.uint32).reshape(-1, 2))
    nw = len(watch) if n_watch is None else n_watch
    out = np.zeros(max(len(w), 1), impop_amd.KIN_WINDOW_DTYPE)
    rows = np.zeros((max(len(w), 1), max(nw, 1)), impop_amd.KIN_WATCH_DTYPE)
    prm = _lib.KinshipParams(C.sizeof(_lib.KinshipParams) if struct_size is None else struct_size, kin[0], kin[1], 0)
    rc = ctx._lib.impop_kinship_scan(ctx.handle, g.handle, w.ctypes.data_as(C.POINTER(_lib.Window)), len(w), C.byref(prm),
                                     wa.ctypes.data_as(C.POINTER(C.c_uint32)), nw, out.ctypes.data_as(C.POINTER(_lib.KinWindow)), None,
                                     rows.ctypes.data_as(C.POINTER(_lib.KinWatch)))
    return rc, ctx._lib.impop_last_error().decode()


def test_refusals(ctx, planes_of):
    import impop_amd
    from impop_amd import _lib
    n, S = 2 * MAX_N + 4, 64
    bm = ctx.synthetic(n, S, keep_hap_major=False)
    try:
        for what, pairs, code, needle in (("an index outside the matrix", [(0, 1), (2, n)], _lib.E_INVALID, "outside"),
                                          ("both copies one haplotype", [(0, 1), (3, 3)], _lib.E_INVALID, "both copies"),
                                          ("a haplotype in two pairs", [(0, 1), (2, 1)], _lib.E_INVALID, "two pairs"),
                                          ("one individual", [(0, 1)], _lib.E_INVALID, "two individuals"),
                                          ("2049 individuals", np.arange(2 * MAX_N + 2).reshape(-1, 2), _lib.E_UNSUPPORTED, "2049")):
            rc, msg = raw_create(ctx, bm, pairs)
            assert rc == code and needle in msg and "impop_genotypes_create" in msg, (what, rc, msg)
        wt = np.ones(S, np.uint32)
        bm.set_site_weights(wt)
        rc, msg = raw_create(ctx, bm, [(0, 1), (2, 3)])
        assert rc == _lib.E_UNSUPPORTED and "weights" in msg and "impop_genotypes_create" in msg
        bm.set_site_weights(None)
        rc, msg = raw_create(ctx, bm, [(0, 1), (2, 3)])
        assert rc == 0, msg
    finally:
        bm.free()
    N = 17
    g = planes_of(N)
    wins = kc.window_lists()["tiling"]
    for what, args, needle in (("a watched pair i == j", dict(watch=[(0, 1), (5, 5)]), "twice"),
                               ("a watched individual outside", dict(watch=[(0, N)]), "outside"),
                               ("too many watched pairs", dict(watch=[(0, 1)], n_watch=MAX_WATCH + 1), "1025"),
                               ("kin_den 0", dict(kin=(0, 0)), "kin_den"),
                               ("kin_den above 2^20", dict(kin=(1, (1 << 20) + 1)), "kin_den"),
                               ("kin_num above kin_den", dict(kin=(11, 10)), "kin_num"),
                               ("a window outside the planes", dict(wins=[(0, 5000, 0)]), "site range"),
                               ("a wrong struct_size", dict(struct_size=12), "struct_size")):
        a = dict(wins=wins)
        a.update(args)
        rc, msg = raw_scan(ctx, g, **a)
        assert rc == _lib.E_INVALID and needle in msg and ("impop_kinship" in msg), (what, rc, msg)
    assert raw_scan(ctx, g, [])[0] == 0  # n_windows == 0
    none = g.kinship_scan([], kin=kc.KIN, watch=[(0, 1)])
    assert none[0].shape == (0,) and none[2].shape == (0, 1) and not none[1]["t"].any()
    # the device error word: the call that sees it fails once and clears it
    good = g.kinship_scan(wins, kin=kc.KIN)
    _lib.check(ctx._lib.impop_debug_raise_device_error(ctx.handle, 256))
    rc, msg = raw_scan(ctx, g, wins)
    assert rc == _lib.E_INTERNAL and "impop_kinship_scan" in msg and "joint genotype table" in msg, msg
    assert blob(g.kinship_scan(wins, kin=kc.KIN)) == blob(good)
    # timers: the plane build and the epilogue
    ctx.gram_timing(True)
    try:
        g.kinship_scan(wins, kin=kc.KIN)
        ms, chunks = ctx.kinship_elapsed()
        assert chunks == 1 and ms[0] == 0.0 and ms[1] > 0.0 and ctx.gram_elapsed()[1] == 1
    finally:
        ctx.gram_timing(False)


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def test_cli_tables_are_the_records(tmp_path):
    """--format kinship: the main table, --kin-pairs and --kin-watch-table are what impop_amd.kinship formats from the restatement's
    records; -u restricts the samples; --compact changes nothing"""
    import impop_amd
    from impop_amd import kinship as kin
    from impop_amd.matrixio import MatrixFile, save_matrix
    N, origin = 17, 5000
    m01 = kc.matrix(N)
    S = m01.shape[1]
    names = [f"S{i // 2:02d}#{i % 2 + 1}#chrT:0-1" for i in range(2 * N)] + ["CHM13#0#chrT:0-1"]
    samples = [f"S{i:02d}" for i in range(N)]
    pr = np.arange(2 * N).reshape(N, 2)
    mpath, bed, sub = str(tmp_path / "m.npz"), str(tmp_path / "w.bed"), str(tmp_path / "sub.txt")
    save_matrix(mpath, MatrixFile(bits=impop_amd.pack_hap_major(m01), n_site=S, names=names, origin=origin, contig="chrT"))
    rows = [(0, 256), (128, 512), (768, 1152), (0, S)]
    open(bed, "w").write("".join(f"chrT\t{origin + b}\t{origin + e}\n" for b, e in rows))
    open(sub, "w").write("".join(s + "\n" for s in samples[:5]))
    regions = [f"CHM13#0#chrT:{origin + b}-{origin + e}" for b, e in rows]
    text = lambda header, table: "\n".join(["\t".join(header)] + ["\t".join(r) for r in table]) + "\n"  # noqa: E731
    script = [sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", mpath, "--bed", bed, "--format", "kinship"]
    pairp, watp = str(tmp_path / "pairs.tsv"), str(tmp_path / "watch.tsv")
    watch = [(3, 0), (1, 2)]
    ww, wp, wt = pk.scan(m01, pr, [(b, e, e - b) for b, e in rows], kin.threshold_fraction(0.2), watch)
    main, pairs, wat = kin.tables(regions, [e - b for b, e in rows], samples, ww, wp["t"], watch, wt)
    assert len(main) == 4 and len(pairs) == N * (N - 1) // 2 and len(wat) == 8 and any(r[-1] == "unrelated" for r in pairs)
    for extra in ([], ["--compact"]):
        r = subprocess.run(script + ["--kin-threshold", "0.2", "--kin-pairs", pairp, "--kin-watch", "S03,S00", "--kin-watch", "S01,S02",
                                     "--kin-watch-table", watp] + extra, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "1 sequences are not one of a sample's two haplotypes" in r.stderr
        assert r.stdout == text(kin.WINDOW_COLUMNS, main)
        assert open(pairp).read() == text(kin.PAIR_COLUMNS, pairs)
        assert open(watp).read() == text(kin.WATCH_COLUMNS, wat)
    ww5, _, _ = pk.scan(m01, pr[:5], [(b, e, e - b) for b, e in rows], kin.threshold_fraction(0.0884))
    r = subprocess.run(script + ["-u", sub], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == text(kin.WINDOW_COLUMNS, kin.tables(regions, [e - b for b, e in rows], samples[:5], ww5)[0])
