"""GPU: impop_permtest_scan — permutation p-values for Fst, Phi_ST, Dxy and S_nn per window and pair of panels — byte for byte
against the plain restatement (tests/plain_permtest.py) fed with impop_permtest_labels' masks, the null table included wherever it
is allowed; against impop_pairdist_scan on the same call; and against itself under every way of computing the same windows."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import permtest_cases as pc
import plain_permtest as pt
from conftest import ROOT

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 12345


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


def labels_of(seed, n_perm):
    """the restatement's labellings come from the library's generator (itself checked against the restatement's on the host)"""
    import impop_amd

    @functools.lru_cache(maxsize=None)
    def get(p, m, m_k):
        return pt.from_words(impop_amd.permtest_labels(seed, p, m, m_k, n_perm))
    return get


def upload(ctx, m01):
    import impop_amd
    return ctx.upload(impop_amd.pack_hap_major(m01), m01.shape[1], keep_hap_major=True)


def blob(res):
    return b"".join(a.tobytes() for a in res if a is not None)


def assert_equal(got, want, what=""):
    """field by field for a readable failure, then byte for byte (the doubles included: NaN has one bit pattern)"""
    g, w = got[0], want[0]
    assert g.shape == w.shape, (what, g.shape, w.shape)
    for f in w.dtype.names:
        if w.dtype[f].kind != "f":
            bad = np.argwhere(g[f] != w[f])
            assert not len(bad), (what, f, bad[:4].tolist(), g[f][tuple(bad[0])], w[f][tuple(bad[0])])
    assert g.tobytes() == w.tobytes(), (what, "bytes of the doubles")
    assert (got[1] is None) == (want[1] is None), what
    if want[1] is not None:
        assert got[1].shape == want[1].shape and got[1].tobytes() == want[1].tobytes(), (what, "null table")


def check_case(ctx, m01, wins, pops, n_perm, weights=None, seed=SEED, what=""):
    bm = upload(ctx, m01)
    try:
        if weights is not None:
            bm.set_site_weights(weights)
        got = bm.permtest_scan(wins, pc.flags(pops, m01.shape[0]), n_perm=n_perm, seed=seed, null=True)
    finally:
        bm.free()
    want = pt.scan(m01, wins, pops, labels_of(seed, n_perm), n_perm, weights=weights)
    assert_equal(got, want, what)
    return got


# ---- shapes that can break the tiling ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", sorted(pc.SHAPES))
def test_shapes(ctx, shape):
    """panel sizes below a tile, across 64 and 128 members, a one-member panel, K = 3 with haplotypes in no panel, K = 8 at n = 65"""
    sizes, n = pc.SHAPES[shape]
    check_case(ctx, pc.matrix(n), pc.WINS3, pc.panels(sizes, n), 17, what=shape)


@pytest.mark.parametrize("n_perm", pc.N_PERMS)
def test_column_counts(ctx, n_perm):
    """n_perm = 1, 17, 100: the columns are no multiple of 16, 32 or 64, and 100 takes two labelling tasks per pair"""
    check_case(ctx, pc.matrix(), pc.WINS3, pc.panels((37, 29)), n_perm, what=n_perm)


# ---- byte planes ------------------------------------------------------------------------------------------------------------------

def test_byte_planes_unweighted(ctx):
    """W = 0, W = 1 and 255 < W <= 65535 in one call: two planes"""
    m01, wins = pc.plane_case()
    got = check_case(ctx, m01, wins, [list(range(0, 24, 2)), list(range(1, 24, 2))], 17)
    assert [int(x) for x in got[0]["n_sites"][:, 0]] == [0, 1, 400] and int(got[0]["ab"][0, 0]) == 0


def test_byte_planes_weighted_and_bp_expanded(ctx):
    """W > 65535 through site weights on a 40-site window (three planes); the weighted matrix gives the bytes of its bp-expanded one"""
    node, wt, node_wins, expanded, bp_wins = pc.weighted_case()
    pops = [list(range(0, 11)), list(range(11, 24))]
    a = check_case(ctx, node, node_wins, pops, 17, weights=wt)
    assert int(a[0]["n_sites"].max()) > 65535
    be = upload(ctx, expanded)
    try:
        b = be.permtest_scan(bp_wins, pc.flags(pops, 24), n_perm=17, seed=SEED, null=True)
    finally:
        be.free()
    assert blob(a) == blob(b)


def test_compacted_matrix_with_fewer_planes_gives_the_same_bytes(ctx):
    """a 400-site window whose last 300 sites every haplotype carries: two planes on the full matrix, one on the compacted one"""
    m01 = pc.matrix(24, 400, pc.SEED + 8).copy()
    m01[:, 100:400] = 1
    pops = [list(range(0, 11)), list(range(11, 24))]
    wins = [(0, 400, 400), (50, 300, 250)]
    a = check_case(ctx, m01, wins, pops, 17)
    full = upload(ctx, m01)
    try:
        comp = full.compact()
        try:
            assert comp.n_site <= 100
            assert blob(comp.permtest_scan(wins, pc.flags(pops, 24), n_perm=17, seed=SEED, null=True)) == blob(a)
        finally:
            comp.free()
    finally:
        full.free()


# ---- ties, planted and exchangeable windows -------------------------------------------------------------------------------------------

def test_ties(ctx):
    m01, pops = pc.tie_case()
    check_case(ctx, m01, [(0, 64, 64), (0, 20, 20)], pops, 100)


def test_planted_and_exchangeable_windows(ctx):
    """p = 1 / (n_perm + 1) exactly on the planted windows, p = 1 exactly on the exchangeable one"""
    m01, pops, wins = pc.planted_case()
    n_perm = 100
    got = check_case(ctx, m01, wins, pops, n_perm)[0]
    for w, ge, p in ((0, 0, 1.0 / (n_perm + 1.0)), (1, n_perm, 1.0), (2, 0, 1.0 / (n_perm + 1.0))):
        for t in ("fst", "phi", "dxy", "snn"):
            assert int(got["ge_" + t][w, 0]) == ge and float(got["p_" + t][w, 0]) == p, (w, t)


# ---- the upper end -------------------------------------------------------------------------------------------------------------------

def test_upper_end_of_the_member_range(ctx):
    """1024 members (512 + 512) x 200 sites, 2 windows, n_perm = 32; one member more is refused before anything runs"""
    from impop_amd import _lib
    m01, pops, wins = pc.upper_case()
    check_case(ctx, m01, wins, pops, 32)
    big = np.zeros((1026, 64), np.uint8)
    bm = upload(ctx, big)
    try:
        rc, msg = raw_call(ctx, bm, [(0, 64, 64)], pc.flags([list(range(0, 513)), list(range(513, 1025))], 1026), 4)
        assert rc == _lib.E_UNSUPPORTED and "1025" in msg and "1024" in msg, (rc, msg)
    finally:
        bm.free()


# ---- the same windows computed in every other way: one blob ----------------------------------------------------------------------------

INV = dict(sizes=(70, 61), n_perm=100)


def _child(path):
    import impop_amd
    ctx = impop_amd.Context(0)
    bm = upload(ctx, pc.matrix())
    got = bm.permtest_scan(pc.WINS3, pc.flags(pc.panels(INV["sizes"]), pc.N), n_perm=INV["n_perm"], seed=SEED, null=True)
    with open(path, "wb") as f:
        f.write(blob(got))
    bm.free(); ctx.close()


def run_child(tmp_path, env_extra):
    """-> (blob, trace fields of the [impop_permtest_scan] line)"""
    path = str(tmp_path / "r.bin")
    env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]), **env_extra)
    r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_permtest_scan as t; t._child(sys.argv[1])", path],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stderr.splitlines() if l.startswith("[impop_permtest_scan] route=")]
    assert len(lines) == 1, r.stderr[-2000:]
    with open(path, "rb") as f:
        return f.read(), dict(f.split("=") for f in lines[0].split()[1:])


@functools.lru_cache(maxsize=None)
def invariance_reference():
    return pt.scan(pc.matrix(), pc.WINS3, pc.panels(INV["sizes"]), labels_of(SEED, INV["n_perm"]), INV["n_perm"])


@pytest.mark.parametrize("env", [{}, {"IMPOP_PAIRWISE_CHUNK": "1"}, {"IMPOP_GRAM_U16": "0"}, {"IMPOP_GRAM_CHAIN": "1"}],
                         ids=["default", "chunk1", "int32", "chain1"])
def test_invariance_under_the_switches(tmp_path, env):
    """every switch is read by a fresh process; the bytes are the restatement's, and the trace line tells the call's shape"""
    got, trace = run_child(tmp_path, env)
    assert got == blob(invariance_reference()), env
    assert trace["route"] == "dense" and trace["null"] == "on" and int(trace["planes"]) == 1
    assert (int(trace["pops"]), int(trace["pairs"]), int(trace["members"]), int(trace["perms"]), int(trace["windows"])) == (2, 1, 131, 100, 3)
    assert int(trace["chunks"]) == (3 if "IMPOP_PAIRWISE_CHUNK" in env else 1) and int(trace["launches"]) == 2 * int(trace["chunks"])


def test_invariance_compacted_permuted_and_twice(ctx):
    m01 = pc.matrix().copy()
    m01[:, 5::17] = 1
    m01[:, 9::23] = 0
    pops = pc.panels((37, 29))
    fl = pc.flags(pops, pc.N)
    full = upload(ctx, m01)
    try:
        a = full.permtest_scan(pc.WINS3, fl, n_perm=17, seed=SEED, null=True)
        assert_equal(a, pt.scan(m01, pc.WINS3, pops, labels_of(SEED, 17), 17))
        assert blob(full.permtest_scan(pc.WINS3, fl, n_perm=17, seed=SEED, null=True)) == blob(a)
        order = [2, 0, 1]
        b = full.permtest_scan([pc.WINS3[i] for i in order], fl, n_perm=17, seed=SEED, null=True)
        back = np.argsort(order)
        assert blob([b[0][back], b[1][back]]) == blob(a)
        comp = full.compact()
        try:
            assert blob(comp.permtest_scan(pc.WINS3, fl, n_perm=17, seed=SEED, null=True)) == blob(a)
        finally:
            comp.free()
        assert blob(full.permtest_scan(pc.WINS3, fl, n_perm=17, seed=SEED, null=False)) == a[0].tobytes()
    finally:
        full.free()


# ---- cross-checks ---------------------------------------------------------------------------------------------------------------------

def test_against_pairdist_scan_and_the_prefix_property(ctx):
    pops = pc.panels((20, 13, 31))
    fl = pc.flags(pops, pc.N)
    bm = upload(ctx, pc.matrix())
    try:
        long, long_null = bm.permtest_scan(pc.WINS3, fl, n_perm=200, seed=SEED, null=True)
        short, short_null = bm.permtest_scan(pc.WINS3, fl, n_perm=100, seed=SEED, null=True)
        panels, pairs, _, _ = bm.pairdist_scan(pc.WINS3, fl)
        other = bm.permtest_scan(pc.WINS3, fl, n_perm=100, seed=SEED + 1, null=True)[1]
    finally:
        bm.free()
    assert short_null.tobytes() == long_null[:, :, :100].tobytes() and other.tobytes() != short_null.tobytes()
    for f in ("wa", "wb", "ab", "nn", "fst", "phi_st", "dxy", "snn"):
        assert short[f].tobytes() == long[f].tobytes(), f
    assert long["snn"].tobytes() == pairs["snn"].tobytes() and (long["ab"] == pairs["sum_h"]).all()
    p = 0
    for k in range(3):
        for l in range(k + 1, 3):
            assert (long["wa"][:, p] == panels["sum_h"][:, k]).all() and (long["wb"][:, p] == panels["sum_h"][:, l]).all()
            p += 1


def raw_call(ctx, bm, wins, fl, n_perm, n_pop=None, struct_size=None, null=False):
    """the C call with nothing checked on the Python side -> (return code, message)"""
    import impop_amd
    from impop_amd import _lib
    w = impop_amd.make_windows(wins)
    K = len(fl) if n_pop is None else n_pop
    packed = np.concatenate([impop_amd.pack_mask(f, bm.n_hap) for f in fl]) if fl else np.zeros(1, np.uint64)
    out = np.zeros((max(len(w), 1), 64), impop_amd.PERM_PAIR_DTYPE)
    nul = np.zeros(1, impop_amd.PERM_NULL_DTYPE)  # only ever passed where the call must refuse before it writes
    prm = _lib.PermtestParams(C.sizeof(_lib.PermtestParams) if struct_size is None else struct_size, n_perm, SEED)
    rc = ctx._lib.impop_permtest_scan(ctx.handle, bm.handle, w.ctypes.data_as(C.POINTER(_lib.Window)), len(w),
                                      packed.ctypes.data_as(C.POINTER(C.c_uint64)), K, C.byref(prm),
                                      out.ctypes.data_as(C.POINTER(_lib.PermPair)), nul.ctypes.data_as(C.POINTER(_lib.PermNull)) if null else None)
    return rc, ctx._lib.impop_last_error().decode()


def test_refusals(ctx):
    from impop_amd import _lib
    n = 65
    bm = upload(ctx, pc.matrix(n))
    try:
        fl = pc.flags(pc.panels((9, 8, 8), n), n)
        eye = np.eye(n, dtype=np.uint8)
        for what, args, needle in (("struct_size", dict(fl=fl, n_perm=4, struct_size=8), "struct_size"),
                                   ("n_pop 1", dict(fl=fl[:1], n_perm=4), "n_pop"),
                                   ("n_pop 9", dict(fl=[eye[i] for i in range(9)], n_perm=4), "n_pop"),
                                   ("n_perm 0", dict(fl=fl, n_perm=0), "n_perm"),
                                   ("n_perm 16385", dict(fl=fl, n_perm=16385), "n_perm"),
                                   ("overlapping panels", dict(fl=[fl[0], fl[1] | fl[0]], n_perm=4), "disjoint"),
                                   ("an empty panel", dict(fl=[fl[0], np.zeros(n, np.uint8)], n_perm=4), "empty")):
            rc, msg = raw_call(ctx, bm, pc.WINS3, **args)
            assert rc == _lib.E_INVALID and needle in msg, (what, rc, msg)
        # the null-table bound: 87 windows x 3 pairs x 16384 labellings pass 2^22 entries
        many = [(0, 4, 4)] * 29
        rc, msg = raw_call(ctx, bm, many, fl, 16384 * 3, null=True)
        assert rc == _lib.E_INVALID, (rc, msg)  # n_perm itself comes first
        rc, msg = raw_call(ctx, bm, many * 3, fl, 16384, null=True)
        assert rc == _lib.E_UNSUPPORTED and "2^22" in msg, (rc, msg)
        # nothing to do
        rc, msg = raw_call(ctx, bm, [], fl, 4)
        assert rc == 0, msg
        # the device error word: the call that sees it fails once and clears it
        good = bm.permtest_scan(pc.WINS3, fl, n_perm=4, seed=SEED)
        _lib.check(ctx._lib.impop_debug_raise_device_error(ctx.handle, 512))
        rc, msg = raw_call(ctx, bm, pc.WINS3, fl, 4)
        assert rc == _lib.E_INTERNAL and "permutation test" in msg, (rc, msg)
        assert bm.permtest_scan(pc.WINS3, fl, n_perm=4, seed=SEED)[0].tobytes() == good[0].tobytes()
    finally:
        bm.free()


def test_the_fst_admission_rule(ctx):
    """W_max * P_max^2 > 2^62 is refused with both numbers in the message: a 513-member panel has q = 131328 and admits W up to
    2^62 / q^2 = 267386880; site weights put a window just above and just below"""
    from impop_amd import _lib
    q = 513 * 512 // 2
    w_ok = (1 << 62) // (q * q)
    m01 = np.zeros((1024, 8), np.uint8)
    m01[::2, 0] = 1
    bm = upload(ctx, m01)
    try:
        fl = pc.flags([list(range(0, 513)), list(range(513, 1024))], 1024)
        wt = np.ones(8, np.uint32)
        wt[0] = w_ok - 7
        bm.set_site_weights(wt)
        rc, msg = raw_call(ctx, bm, [(0, 8, 0)], fl, 2)
        assert rc == 0, msg
        wt[0] = w_ok - 6
        bm.set_site_weights(wt)
        rc, msg = raw_call(ctx, bm, [(0, 8, 0)], fl, 2)
        assert rc == _lib.E_UNSUPPORTED and str(w_ok + 1) in msg and str(q) in msg, (rc, msg)
    finally:
        bm.free()


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def test_cli_writes_the_two_tables_for_two_matrices(ctx, tmp_path):
    """scripts/impop_permtest.py on a BED over two matrices: the main and null tables are what impop_amd.permtest formats from
    BitMatrix.permtest_scan; --compact changes nothing"""
    import impop_amd
    from impop_amd import permtest as pm
    from impop_amd.matrixio import MatrixFile, save_matrix
    n, n_perm = 65, 17
    m01 = pc.matrix(n)
    S = m01.shape[1]
    pops = pc.panels((9, 8, 8), n)
    mats, bed_rows, lists = [], [], []
    for k, p in enumerate(pops):
        lists.append(str(tmp_path / f"pop{k}.txt"))
        open(lists[-1], "w").write("".join(f"S{i:02d}\n" for i in p))
    for c, (contig, origin) in enumerate((("chrA", 5000), ("chrB", 100))):
        names = [f"S{i:02d}#1#{contig}:0-1" for i in range(n)]
        path = str(tmp_path / f"{contig}.npz")
        mm = m01 if c == 0 else np.ascontiguousarray(m01[:, ::-1])
        save_matrix(path, MatrixFile(bits=impop_amd.pack_hap_major(mm), n_site=S, names=names, origin=origin, contig=contig))
        mats.append((path, contig, origin, mm))
        bed_rows += [(contig, origin + b, origin + e) for b, e, _ in pc.WINS3]
    bed = str(tmp_path / "w.bed")
    open(bed, "w").write("".join(f"{c}\t{s}\t{e}\n" for c, s, e in bed_rows))
    want_main, want_null = [], []
    for path, contig, origin, mm in mats:
        bm = upload(ctx, mm)
        try:
            pairs, null = bm.permtest_scan(pc.WINS3, pc.flags(pops, n), n_perm=n_perm, seed=7, null=True)
        finally:
            bm.free()
        regions = [f"CHM13#0#{contig}:{origin + b}-{origin + e}" for b, e, _ in pc.WINS3]
        a, b = pm.tables(regions, [e - b for b, e, _ in pc.WINS3], ["pop0", "pop1", "pop2"], pairs, null)
        want_main += a
        want_null += b
    text = lambda header, table: "\n".join(["\t".join(header)] + ["\t".join(r) for r in table]) + "\n"  # noqa: E731
    nullp = str(tmp_path / "null.tsv")
    script = [sys.executable, os.path.join(ROOT, "scripts", "impop_permtest.py"), "--bed", bed, "--panel"] + lists + [
        "--perm-n", str(n_perm), "--perm-seed", "7", "--matrix", mats[0][0], mats[1][0], "--perm-null", nullp]
    for extra in ([], ["--compact"]):
        r = subprocess.run(script + extra, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        assert r.stdout == text(pm.MAIN_COLUMNS, want_main)
        assert open(nullp).read() == text(pm.NULL_COLUMNS, want_null)
