"""GPU: impop_ihs_scan against the plain restatement of tests/plain_ihs.py — every record byte for byte.  What needs the trace
line (IMPOP_TRACE=1 is read once per process) runs in one child process."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import ihs_cases as ic
import plain_ihs as pi
from conftest import ROOT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = -1, -5
ENV = "IMPOP_IHS_CHUNK_BLOCKS"


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


def set_chunk(monkeypatch, blocks):
    if blocks is None:
        monkeypatch.delenv(ENV, raising=False)
    else:
        monkeypatch.setenv(ENV, str(blocks))


def scan(bm, pops, site=(0, None), cores=(None, None), min_mac=1, cutoff=50, limits=(0, 0)):
    rec, total = bm.ihs_scan(mask_a=pops[0], mask_b=pops[1] if len(pops) == 2 else None, site_begin=site[0], site_end=site[1],
                             core_begin=cores[0], core_end=cores[1], min_mac=min_mac, cutoff_milli=cutoff, max_extend_bp=limits[0],
                             max_extend_sites=limits[1])
    assert total == len(rec)
    return rec


# ---- the known answer of the header -------------------------------------------------------------------------------------------------

def test_known_answer(ctx):
    bm = ctx.upload_dense(ic.known_matrix(), keep_hap_major=False)
    rec = scan(bm, [None], min_mac=ic.KNOWN_PARAMS["min_mac"], cutoff=ic.KNOWN_PARAMS["cutoff_milli"])
    assert rec["site"].tolist() == ic.KNOWN_SITES and rec["flags"].tolist() == ic.KNOWN_FLAGS
    assert [(tuple(r["n"]), tuple(r["c1"])) for r in rec] == ic.KNOWN_HEAD
    assert rec["ihh2"].tolist() == ic.KNOWN_I2 and rec["sl2"].tolist() == ic.KNOWN_I2 and not rec["reserved"].any()
    lim = scan(bm, [None], min_mac=3, cutoff=300, limits=(ic.KNOWN_LIMITS["max_bp"], ic.KNOWN_LIMITS["max_sites"]))
    assert lim["flags"].tolist() == ic.KNOWN_LIMIT_FLAGS and lim["ihh2"].tolist() == ic.KNOWN_LIMIT_IHH2
    assert lim["sl2"].tolist() == ic.KNOWN_LIMIT_SL2
    pi.assert_same(rec, pi.reference(ic.known_matrix(), 0, 7, 0, 7, [None], **ic.KNOWN_PARAMS), "known")
    bm.free()


# ---- geometry: tail granules of 1..4 dwords, 32-row ballot groups; chunks of 1, 2, 5 blocks and the default ----------------------------

@pytest.mark.parametrize("n", ic.GEO_N)
def test_shapes_against_the_restatement(ctx, n, monkeypatch):
    bm = ctx.upload_dense(ic.geometry_matrix(n), keep_hap_major=False)
    for K in (1, 2) if n >= 4 else (1,):  # two populations need two members each
        if n >= 33:
            ic.assert_coverage(n, K)
        pops = ic.geometry_pops(n, K)
        for min_mac, cutoff, limits in ic.GEO_PARAMS:
            want = ic.geometry_want(n, K, min_mac, cutoff, limits)
            for chunk in ic.GEO_CHUNKS:
                set_chunk(monkeypatch, chunk)
                got = scan(bm, pops, ic.GEO_RANGE, ic.GEO_CORES, min_mac, cutoff, limits)
                pi.assert_same(got, want, (n, K, min_mac, cutoff, limits, chunk))
    bm.free()


# ---- ranges -----------------------------------------------------------------------------------------------------------------------------

def test_ranges(ctx, monkeypatch):
    n = 70
    m01 = ic.geometry_matrix(n).copy()
    m01[:, 0] = m01[:, ic.GEO_S - 1] = np.arange(n) % 2   # the matrix's first and last site are cores
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    S = ic.GEO_S
    cases = [((0, None), (None, None)), ((0, S), (0, 1)), ((0, S), (S - 1, S)), ((65, 200), (70, 190)), ((64, 128), (64, 128)),
             ((63, 129), (100, 100)), ((1, S - 1), (130, 131)), ((5, 300), (5, 300))]
    for chunk in (None, 1, 2):
        set_chunk(monkeypatch, chunk)
        for site, cores in cases:
            for K, limits in ((1, (0, 0)), (2, (37, 5)), (1, (37, 5))):
                pops = ic.geometry_pops(n, K)
                b, e = site[0], S if site[1] is None else site[1]
                kb = b if cores[0] is None else cores[0]
                ke = e if cores[1] is None else cores[1]
                if ke == 0:
                    continue
                want = pi.reference(m01, b, e, kb, ke, pops, min_mac=2, cutoff_milli=50, max_bp=limits[0], max_sites=limits[1])
                pi.assert_same(scan(bm, pops, site, cores, 2, 50, limits), want, (site, cores, K, limits, chunk))
    whole = scan(bm, [None], min_mac=2)
    assert whole["site"][0] == 0 and whole["site"][-1] == S - 1
    # a core range with no core: [100, 100), and one over sites that are monomorphic
    mono = m01.copy()
    mono[:, 150:170] = 1
    bm2 = ctx.upload_dense(mono, keep_hap_major=False)
    rec, total = bm2.ihs_scan(core_begin=150, core_end=170)
    assert total == 0 and len(rec) == 0
    rec, total = bm2.ihs_scan(core_begin=100, core_end=100)
    assert total == 0 and len(rec) == 0
    bm2.free()
    bm.free()


# ---- uploads, weights, compaction and the order of the haplotypes never change a byte -------------------------------------------------

def test_equivalent_matrices(ctx, monkeypatch):
    set_chunk(monkeypatch, None)
    n = 65
    m01 = ic.geometry_matrix(n)
    rng = np.random.default_rng(21700)
    for K in (1, 2):
        pops = ic.geometry_pops(n, K)
        args = (ic.GEO_RANGE, ic.GEO_CORES, 2, 50, (37, 5))
        want = ic.geometry_want(n, K, 2, 50, (37, 5))
        for ukw in ({"keep_hap_major": False}, {"keep_hap_major": True}):
            bm = ctx.upload_dense(m01, **ukw)
            pi.assert_same(scan(bm, pops, *args), want, ukw)
            if not ukw["keep_hap_major"]:
                cm = bm.compact()
                assert cm.n_site < bm.n_site
                for chunk in (None, 1):
                    set_chunk(monkeypatch, chunk)
                    pi.assert_same(scan(cm, pops, *args), want, ("compact", chunk))
                set_chunk(monkeypatch, None)
                cm.free()
                bm.set_site_weights(rng.integers(1, 5, size=ic.GEO_S).astype(np.uint32))
                pi.assert_same(scan(bm, pops, *args), want, "weighted")
                cw = bm.compact()
                pi.assert_same(scan(cw, pops, *args), want, "weighted, compact")
                cw.free()
            bm.free()
        perm = rng.permutation(n)
        bm = ctx.upload_dense(m01[perm], keep_hap_major=False)
        ppops = [None if p is None else p[perm] for p in pops]
        pi.assert_same(scan(bm, ppops, *args), want, "permuted")
        bm.free()
    # a subset as the one population: the other rows play no part
    sub = np.zeros(n, bool)
    sub[rng.permutation(n)[:41]] = True
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    want = pi.reference(m01, *ic.GEO_RANGE, *ic.GEO_CORES, [sub], min_mac=2)
    pi.assert_same(scan(bm, [sub], ic.GEO_RANGE, ic.GEO_CORES, 2), want, "subset")
    only = ctx.upload_dense(m01[sub], keep_hap_major=False)
    pi.assert_same(scan(only, [None], ic.GEO_RANGE, ic.GEO_CORES, 2), want, "subset alone")
    only.free()
    bm.free()


# ---- degenerate inputs ------------------------------------------------------------------------------------------------------------------

def test_degenerate_inputs(ctx, monkeypatch):
    set_chunk(monkeypatch, None)
    rng = np.random.default_rng(21800)
    # no stepped site: every site monomorphic in P (the other rows vary)
    m01 = (rng.random((10, 200)) < 0.5).astype(np.uint8)
    P = np.zeros(10, bool)
    P[:6] = True
    m01[:6] = m01[0]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    rec, total = bm.ihs_scan(mask_a=P)
    assert total == 0 and len(rec) == 0
    bm.free()
    # a class of one member (min_mac = 1): its integrals are 0 and carry no flag
    m01 = ic.mosaic(rng, 20, 150, nf=3)
    m01[:, 70] = 0
    m01[7, 70] = 1
    want = pi.reference(m01, 0, 150, 0, 150, [None])
    one = want[want["site"] == 70][0]
    assert one["n"].tolist() == [19, 1] and not one["ihh2"][1].any() and not (int(one["flags"]) & 0xCCCC) and one["ihh2"][0].all()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    pi.assert_same(scan(bm, [None]), want, "singleton class")
    bm.free()
    # all haplotypes pairwise different at the core's neighbours: sites 0..2 and 4..6 spell the row's index, site 3 is the core
    idx = np.arange(8)
    code = np.stack([(idx >> k) & 1 for k in range(3)], axis=1).astype(np.uint8)
    m01 = np.concatenate([code, (idx[:, None] % 2).astype(np.uint8), code], axis=1)
    want = pi.reference(m01, 0, 7, 3, 4, [None], cutoff_milli=0)
    assert len(want) == 1 and want["flags"][0] == 0xFF and want["sl2"][0].tolist() == [[10, 22], [10, 22]]  # C = 6, surv 6, 2, 1, 0 / 6, 6, 2, 1
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    pi.assert_same(scan(bm, [None], cores=(3, 4), cutoff=0), want, "all different")
    bm.free()
    # two populations with the same rows
    half = ic.mosaic(rng, 17, 200, nf=3)
    m01 = np.concatenate([half, half])
    a = np.arange(34) < 17
    want = pi.reference(m01, 0, 200, 0, 200, [a, ~a], min_mac=2)
    assert len(want) and (want["ihh2"][:, 0] == want["ihh2"][:, 1]).all() and (want["c1"][:, 0] == want["c1"][:, 1]).all()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    pi.assert_same(scan(bm, [a, ~a], min_mac=2), want, "identical populations")
    bm.free()


# ---- the upper end of the range ---------------------------------------------------------------------------------------------------------

def test_4096_members(ctx, monkeypatch):
    from impop_amd import ImpopError
    rng = np.random.default_rng(21900)
    nh, S, n = 4100, 130, 4096
    distinct = ic.mosaic(rng, 12, S, nf=3, p_switch=0.03, p_mut=0.02, p_mono=0.2)
    which = rng.integers(0, 12, size=nh)
    m01 = distinct[which]
    P = np.ones(nh, bool)
    P[rng.permutation(nh)[:4]] = False
    assert P.sum() == n
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    mult = np.bincount(which[P], minlength=12)
    want = pi.records(pi.weighted_survivors(distinct, [mult], 3, 127), 3, 127, min_mac=5, cutoff_milli=50, max_bp=40, max_sites=10)
    assert len(want) > 40 and (want["flags"] & 0xFF00).any() and ((want["flags"] & 0xFF) == 0).any()
    for chunk in (None, 1):
        set_chunk(monkeypatch, chunk)
        pi.assert_same(scan(bm, [P], (3, 127), (None, None), 5, 50, (40, 10)), want, ("n4096", chunk))
    set_chunk(monkeypatch, None)
    A = P & (rng.random(nh) < 0.4)
    B = P & ~A
    mults = [np.bincount(which[A], minlength=12), np.bincount(which[B], minlength=12)]
    want2 = pi.records(pi.weighted_survivors(distinct, mults, 3, 127), 3, 127, min_mac=5, cutoff_milli=250)
    pi.assert_same(scan(bm, [A, B], (3, 127), (None, None), 5, 250), want2, "n4096 K2")
    with pytest.raises(ImpopError) as ei:
        more = P.copy()
        more[np.flatnonzero(~P)[0]] = True
        bm.ihs_scan(mask_a=more)
    assert ei.value.code == E_UNSUPPORTED
    bm.free()


# ---- the capacity protocol -------------------------------------------------------------------------------------------------------------

def test_capacity(ctx):
    import impop_amd
    from impop_amd import _lib
    n = 33
    want = ic.geometry_want(n, 1, 2, 250, (37, 5))
    total = len(want)
    bm = ctx.upload_dense(ic.geometry_matrix(n), keep_hap_major=False)
    prm = _lib.IhsParams(C.sizeof(_lib.IhsParams), 2, 250, 0, 37, 5)
    for cap in (0, total - 1, total, total + 3):
        rec = np.full(total + 3, 0xA5, dtype=np.uint8).repeat(96).view(impop_amd.IHS_DTYPE)
        canary = rec.tobytes()
        cnt = C.c_uint64(0)
        rc = ctx._lib.impop_ihs_scan(ctx.handle, bm.handle, ic.GEO_RANGE[0], ic.GEO_RANGE[1], ic.GEO_CORES[0], ic.GEO_CORES[1], None, None,
                                     C.byref(prm), rec.ctypes.data_as(C.POINTER(_lib.IhsCore)), cap, C.byref(cnt))
        assert rc == 0 and cnt.value == total
        if cap < total:
            assert rec.tobytes() == canary  # untouched
        else:
            pi.assert_same(rec[:total], want, cap)
            assert rec[total:].tobytes() == canary[total * 96:]
    kw = dict(site_begin=ic.GEO_RANGE[0], site_end=ic.GEO_RANGE[1], core_begin=ic.GEO_CORES[0], core_end=ic.GEO_CORES[1], min_mac=2,
              cutoff_milli=250, max_extend_bp=37, max_extend_sites=5)
    assert bm.ihs_scan(capacity=total - 1, **kw) == (None, total)
    pi.assert_same(bm.ihs_scan(capacity=total, **kw)[0], want, "capacity")
    bm.free()


def test_timers_bracket_the_kernels(ctx, monkeypatch):
    set_chunk(monkeypatch, 2)
    bm = ctx.upload_dense(ic.geometry_matrix(64), keep_hap_major=False)
    ctx.gram_timing(True)
    bm.ihs_scan(capacity=1000, max_extend_bp=37, max_extend_sites=5)
    ms, walks = ctx.ihs_elapsed()
    ctx.gram_timing(False)
    assert walks == 1 and len(ms) == 2 and all(t > 0.0 for t in ms)
    bm.free()


# ---- refusals and the trace line, in a child process under IMPOP_TRACE=1 ---------------------------------------------------------------

def _refusals(n):
    a = np.arange(n) < n // 2
    one = np.zeros(n, bool)
    one[3] = True
    overlap = ~a
    overlap[0] = True
    S = ic.GEO_S
    return [dict(min_mac=0), dict(cutoff_milli=1001), dict(site_begin=100, site_end=100), dict(site_begin=200, site_end=100),
            dict(site_end=S + 1), dict(site_begin=S), dict(site_begin=10, site_end=200, core_begin=9, core_end=100),
            dict(site_begin=10, site_end=200, core_begin=100, core_end=201), dict(site_begin=10, site_end=200, core_begin=150, core_end=100),
            dict(mask_a=a, mask_b=overlap), dict(mask_a=a, mask_b=one), dict(mask_a=one, mask_b=a), dict(mask_a=one),
            dict(mask_a=np.zeros(n, bool)), dict(mask_b=a)]


def _child(out_path):
    import impop_amd
    from impop_amd import ImpopError, _lib
    ctx = impop_amd.Context(0)
    out = {}
    n = 65
    m01 = ic.geometry_matrix(n)
    kw = dict(site_begin=ic.GEO_RANGE[0], site_end=ic.GEO_RANGE[1], core_begin=ic.GEO_CORES[0], core_end=ic.GEO_CORES[1], min_mac=2,
              cutoff_milli=50, max_extend_bp=37, max_extend_sites=5)

    def call(tag, fn):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        out[tag] = fn()[0]
        sys.stderr.flush()

    bm = ctx.upload_dense(m01, keep_hap_major=False)
    call("default", lambda: bm.ihs_scan(capacity=1000, **kw))
    os.environ[ENV] = "1"
    call("chunked", lambda: bm.ihs_scan(capacity=1000, **kw))
    del os.environ[ENV]
    pops = ic.geometry_pops(n, 2)
    call("two", lambda: bm.ihs_scan(mask_a=pops[0], mask_b=pops[1], capacity=1000, **kw))
    cm = bm.compact()
    call("compact", lambda: cm.ihs_scan(capacity=1000, **kw))
    cm.free()
    sys.stderr.write("@@call refused\n")
    sys.stderr.flush()
    codes = []
    for bad in _refusals(n):
        try:
            bm.ihs_scan(**bad)
            codes.append(0)
        except ImpopError as exc:
            codes.append(exc.code)
    cnt = C.c_uint64(0)
    codes.append(ctx._lib.impop_ihs_scan(ctx.handle, bm.handle, 0, 0, 0, 0, None, None,
                                         C.byref(_lib.IhsParams(C.sizeof(_lib.IhsParams) - 4, 1, 50, 0, 0, 0)), None, 0, C.byref(cnt)))
    out["refused"] = np.array(codes)
    sys.stderr.flush()
    call("after", lambda: bm.ihs_scan(capacity=1000, **kw))
    bm.free()
    ctx.close()
    np.savez(out_path, **out)


_TRACE = re.compile(r"\[impop_ihs_scan\] (.*)$")


def test_refusals_and_trace_line():
    n = 65
    want = ic.geometry_want(n, 1, 2, 50, (37, 5))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
        env.pop(ENV, None)
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_ihs_scan as t; t._child(sys.argv[1])", path],
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
    for tag in ("default", "chunked", "compact", "after"):
        assert recs[tag].tobytes() == want.tobytes(), tag
    assert recs["two"].tobytes() == ic.geometry_want(n, 2, 2, 50, (37, 5)).tobytes()
    assert [len(trace[t]) for t in ("default", "chunked", "two", "compact", "refused", "after")] == [1, 1, 1, 1, 0, 1]
    assert recs["refused"].tolist() == [E_INVALID] * (len(_refusals(n)) + 1)
    t = trace["default"][0]
    assert list(t) == ["route", "pops", "members", "stepped", "cores", "chunks", "warmup_steps", "launches", "bytes_streamed"]
    assert t["route"] == "dense" and t["pops"] == 1 and t["members"] == n and t["cores"] == len(want) and t["launches"] == 4
    assert t["stepped"] == len(ic.geometry_tables(n, 1).pos) and t["chunks"] >= 1
    c = trace["chunked"][0]  # [7, 323): 6 blocks, one chunk each, every chunk but the outer ones warms up in both directions
    assert c["chunks"] == 6 and c["warmup_steps"] > t["warmup_steps"] and c["bytes_streamed"] > t["bytes_streamed"]
    assert trace["two"][0]["pops"] == 2 and trace["two"][0]["cores"] == len(ic.geometry_want(n, 2, 2, 50, (37, 5)))
    k = trace["compact"][0]
    assert k["route"] == "compact" and k["cores"] == len(want) and k["stepped"] == t["stepped"] and k["bytes_streamed"] <= t["bytes_streamed"]


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def test_cli_tables_are_the_records(tmp_path):
    import importlib.util
    import io
    import math
    from impop_amd.matrixio import MatrixFile, save_matrix
    from impop_amd import pack_hap_major
    scan_py = os.path.join(ROOT, "scripts", "impop_scan.py")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("impop_scan_cli_ihs_gpu", scan_py)
        cli = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(cli)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    n, origin = 33, 5000
    m01 = ic.geometry_matrix(n)
    names = [f"S{i:02d}#1#chrT:0-1" for i in range(n)]
    mpath, bed = str(tmp_path / "m.npz"), str(tmp_path / "w.bed")
    save_matrix(mpath, MatrixFile(bits=pack_hap_major(m01), n_site=ic.GEO_S, names=names, origin=origin, contig="chrT"))
    rows = [(10, 100), (200, 300)]
    open(bed, "w").write("".join(f"chrT\t{origin + b}\t{origin + e}\n" for b, e in rows))
    a = np.arange(n) < 15
    for name, mask in (("a.txt", a), ("b.txt", ~a), ("sub.txt", np.arange(n) % 3 != 0)):
        open(str(tmp_path / name), "w").write("".join(nm.partition("chrT")[0] + "\n" for nm, f in zip(names, mask) if f))  # S07#1# : a PanSN prefix
    opts = ["--ihs-min-maf", "0.1", "--ihs-cutoff", "0.25", "--ihs-max-extend", "37", "--ihs-max-extend-sites", "5", "--ihs-bins", "4"]
    for fmt, sel, pops, keep in (("ihs", [], [None], False), ("ihs", ["-u", str(tmp_path / "sub.txt")], [np.arange(n) % 3 != 0], True),
                                 ("xpehh", ["--panel", str(tmp_path / "a.txt"), str(tmp_path / "b.txt")], [a, ~a], False)):
        members = n if pops[0] is None else int(sum(int(p.sum()) for p in pops))
        t = pi.survivors(m01, 0, ic.GEO_S, pops)
        rec = np.concatenate([pi.records(t, b, e, min_mac=math.ceil(0.1 * members), cutoff_milli=250, max_bp=37, max_sites=5) for b, e in rows])
        want = io.StringIO()  # CHROM carries the region prefix, as every table's REGION does
        cli.write_ihs_table(want, len(pops), ["CHM13#0#chrT"] * len(rec), [origin + int(s) for s in rec["site"]], rec, 4, keep)
        assert len(want.getvalue().splitlines()) > 20
        for extra in ([], ["--compact"]):
            r = subprocess.run([sys.executable, scan_py, "--matrix", mpath, "--bed", bed, "--format", fmt] + sel + opts + extra
                               + (["--ihs-keep-edge"] if keep else []), capture_output=True, text=True, cwd=ROOT, timeout=300)
            assert r.returncode == 0, r.stderr[-3000:]
            assert r.stdout == want.getvalue(), (fmt, extra)
