"""GPU: impop_paint_scan against the plain restatement of tests/paint_cases.py — every integer of every output, bit for bit.  What
needs the trace line (IMPOP_TRACE=1 is read once per process) runs in one child process."""
import ctypes as C
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import paint_cases as pc
from conftest import ROOT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED, E_INTERNAL = -1, -5, -6
ENV = "IMPOP_PAINT_CHUNK_BLOCKS"
RENAME = {"mu": "mismatch_cost", "c": "switch_cost", "site_cost": "site_switch_cost", "b": "site_begin", "e": "site_end"}


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


def scan(bm, kw, **extra):
    args = {RENAME.get(k, k): v for k, v in kw.items() if k != "coords"}
    args.update(extra)
    return bm.paint_scan(args.pop("recipients"), **args)


def some_recipients(n, k=6):
    return sorted({0, n - 1} | {int(x) for x in np.linspace(0, n - 1, k)})


def test_error_codes_are_the_librarys():
    from impop_amd import _lib
    assert (_lib.E_INVALID, _lib.E_UNSUPPORTED, _lib.E_INTERNAL) == (E_INVALID, E_UNSUPPORTED, E_INTERNAL)


# ---- the header's known answers ---------------------------------------------------------------------------------------------------------

def test_known_answers(ctx):
    bm = ctx.upload_dense(pc.known_matrix(), keep_hap_major=False)
    for (mu, c), (cost, n_mismatch, segments) in pc.KNOWN.items():
        kw = dict(recipients=[0], donors=[0, 1, 1, 1], mu=mu, c=c)
        got = scan(bm, kw)
        r = got["recipients"][0]
        assert (int(r["cost"]), int(r["n_mismatch"]), int(r["n_donors"])) == (cost, n_mismatch, 3)
        assert [(int(s["donor"]), int(s["begin"]), int(s["end"])) for s in got["segments"]] == segments
        pc.assert_equal(got, pc.reference(pc.known_matrix(), **kw), ("known", mu, c))
    bm.free()
    # every donor identical to the recipient: one segment from the lowest admissible donor, cost 0
    same = np.tile((np.arange(150) % 3 == 0).astype(np.uint8), (5, 1))
    bm = ctx.upload_dense(same, keep_hap_major=False)
    got = bm.paint_scan([3, 0], mismatch_cost=3, switch_cost=2)
    assert got["recipients"]["cost"].tolist() == [0, 0] and got["segments"]["donor"].tolist() == [0, 1]
    assert got["segments"]["n_sites"].tolist() == [150, 150] and got["n_segments"] == 2
    bm.free()


# ---- donor counts: one state per lane, the state-slot edges, the limit ------------------------------------------------------------------

@pytest.mark.parametrize("n_don,S", ((1, 200), (2, 230), (63, 300), (64, 300), (65, 300), (129, 330), (465, 260), (1024, 200)))
def test_donor_counts(ctx, n_don, S):
    rng = np.random.default_rng(1000 + n_don)
    n = n_don + 1  # every recipient sees all the others
    m01 = pc.mosaic_matrix(rng, n, S, nf=6)
    panel = (np.arange(n) % 3).astype(np.uint8)
    panel[::7] = pc.NO_PANEL
    kw = dict(recipients=some_recipients(n, 4), mu=2, c=5, b=3, e=S - 2, windows=pc.window_list(3, S - 2), panel=panel, n_panels=3)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    want = pc.reference(m01, **kw)
    assert int(want["recipients"]["n_donors"].max()) == n_don
    if n_don > 2:
        assert want["n_segments"] > len(kw["recipients"]) and int(want["recipients"]["n_mismatch"].sum()) > 0  # real mosaics
    pc.assert_equal(scan(bm, kw), want, ("donors", n_don))
    bm.free()


# ---- unaligned ranges ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", (1, 2, 63, 64, 65, 130))
def test_unaligned_ranges(ctx, L):
    rng = np.random.default_rng(2000 + L)
    n, S = 20, 37 + 130 + 40
    m01 = pc.mosaic_matrix(rng, n, S, p_switch=0.08, p_mut=0.05)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    for b in (37, 64, 0):
        kw = dict(recipients=some_recipients(n, 5), mu=1, c=2, b=b, e=b + L, windows=[(b, b + L), (b, b + 1), (b + L - 1, b + L + 9)])
        pc.assert_equal(scan(bm, kw), pc.reference(m01, **kw), ("range", b, L))
    bm.free()


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------

def test_ties(ctx):
    rng = np.random.default_rng(3000)
    n, S = 70, 400
    m01 = pc.mosaic_matrix(rng, n, S, nf=3, p_mut=0.03)
    m01[10:20] = m01[40:50]  # duplicated donor rows
    m01[5] = m01[66]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    rc = some_recipients(n, 8) + [5, 12, 45]
    zeros = rng.integers(0, 4, size=S).astype(np.uint32)
    zeros[rng.random(S) < 0.3] = 0
    for tag, kw in (("mu=c=1", dict(mu=1, c=1)), ("c=0", dict(mu=1, c=0)), ("per-site zeros", dict(mu=2, site_cost=zeros)),
                    ("limits", dict(mu=65535, c=1 << 20)),
                    ("per-site limits", dict(mu=65535, site_cost=np.where(rng.random(S) < 0.5, 1 << 20, 0).astype(np.uint32)))):
        kw = dict(kw, recipients=sorted(set(rc)), windows=pc.partition_windows(0, S))
        want = pc.reference(m01, **kw)
        pc.assert_equal(scan(bm, kw), want, tag)
    bm.free()


# ---- groups -------------------------------------------------------------------------------------------------------------------------------

def test_groups(ctx):
    from impop_amd import ImpopError
    rng = np.random.default_rng(4000)
    n, S = 24, 300
    m01 = pc.mosaic_matrix(rng, n, S, nf=4)
    m01[1::2] = m01[0::2] ^ (rng.random((n // 2, S)) < 0.002)  # the other haplotype of one's own sample is the best donor by far
    group = (np.arange(n) // 2).astype(np.uint32)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    kw = dict(recipients=list(range(n)), mu=2, c=4, group=group)
    got = scan(bm, kw)
    pc.assert_equal(got, pc.reference(m01, **kw), "groups")
    assert (group[got["segments"]["donor"]] != group[got["segments"]["h"]]).all()
    assert (got["recipients"]["n_donors"] == n - 2).all()
    free = scan(bm, dict(recipients=list(range(n)), mu=2, c=4))
    assert (free["recipients"]["cost"] < got["recipients"]["cost"]).any()  # without groups the own sample is copied
    # a recipient whose only donors are in its own group
    only = np.zeros(n, np.uint8)
    only[[6, 7]] = 1
    with pytest.raises(ImpopError) as ei:
        bm.paint_scan([6], donors=only, group=group)
    assert ei.value.code == E_INVALID
    assert bm.paint_scan([5], donors=only, group=group)["recipients"]["n_donors"].tolist() == [2]
    bm.free()


# ---- compacted matrix ------------------------------------------------------------------------------------------------------------------------

def test_compacted_matrix(ctx):
    rng = np.random.default_rng(5000)
    n, S = 40, 900
    m01 = pc.mosaic_matrix(rng, n, S)
    mono = rng.random(S) < 0.5
    m01[:, mono] = (rng.random(int(mono.sum())) < 0.3).astype(np.uint8)[None, :]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    cm = bm.compact()
    keep = cm.positions().astype(np.int64)
    assert 0 < len(keep) < S
    b, e = 101, 850
    L = int(((keep >= b) & (keep < e)).sum())
    cost = rng.integers(0, 6, size=L).astype(np.uint32)
    for tag, extra in (("constant", dict(c=3)), ("per-site", dict(site_cost=cost))):
        kw = dict(recipients=some_recipients(n), mu=2, b=b, e=e, windows=pc.window_list(b, e), **extra)
        got = scan(cm, kw)
        pc.assert_equal(got, pc.reference(m01[:, keep], coords=keep, **kw), ("compact", tag))
        seg = got["segments"]
        for r in range(len(kw["recipients"])):  # original coordinates; a recipient's segments tile [b, e)
            mine = seg[seg["recipient"] == r]
            assert mine["begin"][0] == b and mine["end"][-1] == e and (mine["begin"][1:] == mine["end"][:-1]).all()
            assert np.isin(mine["begin"][1:], keep).all() and int(mine["n_sites"].sum()) == L
    cm.free()
    bm.free()


# ---- windows ------------------------------------------------------------------------------------------------------------------------------

def test_windows(ctx):
    rng = np.random.default_rng(6000)
    n, S = 50, 500
    m01 = pc.mosaic_matrix(rng, n, S)
    panel = (np.arange(n) % 8).astype(np.uint8)
    panel[3::9] = pc.NO_PANEL
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    b, e = 20, 470
    rc = some_recipients(n, 7)
    kw = dict(recipients=rc, mu=3, c=4, b=b, e=e, panel=panel, n_panels=8, windows=pc.window_list(b, e))
    got = scan(bm, kw)
    pc.assert_equal(got, pc.reference(m01, **kw), "windows")
    w, anc = got["windows"], got["anc"]
    assert w["cells"][4] == 0 and w["cells"][5] == 0 and not anc[4].any() and not anc[5].any()  # the empty one, the one outside
    assert (anc.sum(axis=1)[:, :8] == w["copied"][:, :8]).all() and (anc.sum(axis=1)[:, 8] == w["copied"][:, 8]).all()
    part = dict(kw, windows=pc.partition_windows(b, e, 7))
    got = scan(bm, part)
    pc.assert_equal(got, pc.reference(m01, **part), "partition")
    assert int(got["windows"]["cells"].sum()) == len(rc) * (e - b)
    assert int(got["windows"]["n_switches"].sum()) == int((got["recipients"]["n_segments"] - 1).sum())
    assert int(got["windows"]["n_mismatch"].sum()) == int(got["recipients"]["n_mismatch"].sum())
    # window records without anc, anc without panels
    plain = scan(bm, dict(recipients=rc, mu=3, c=4, b=b, e=e, windows=pc.window_list(b, e)))
    assert plain["anc"].shape == (8, len(rc), 1) and (plain["anc"][:, :, 0].sum(axis=1) == plain["windows"]["cells"]).all()
    bm.free()


# ---- the capacity protocol ------------------------------------------------------------------------------------------------------------------

def test_segment_capacity(ctx):
    rng = np.random.default_rng(7000)
    n, S = 30, 400
    m01 = pc.mosaic_matrix(rng, n, S)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    kw = dict(recipients=list(range(n)), mu=2, c=3)
    want = pc.reference(m01, **kw)
    total = want["n_segments"]
    assert total > n
    exact = scan(bm, kw, seg_capacity=total)
    pc.assert_equal(exact, want, "exact capacity")
    short = scan(bm, kw, seg_capacity=total - 1)
    assert short["segments"] is None and short["n_segments"] == total
    for k in ("recipients", "chunk_counts", "chunk_sites"):
        assert short[k].tobytes() == want[k].tobytes(), k
    none = scan(bm, kw, want_segments=False)
    assert none["segments"] is None and none["n_segments"] == total
    # raw: one short leaves the caller's buffer untouched, several recipient ranges included
    from impop_amd import _lib, PAINT_SEGMENT_DTYPE
    buf = np.full(total, 0xAB, dtype=np.uint8).repeat(PAINT_SEGMENT_DTYPE.itemsize).view(PAINT_SEGMENT_DTYPE)
    rcp = np.arange(n, dtype=np.uint32)
    n_seg = C.c_uint64(0)
    prm = _lib.PaintParams(C.sizeof(_lib.PaintParams), 2, 3, 0, 0, 0, None, 0, None, None, 4 * S * 8 * 2)
    rc = ctx._lib.impop_paint_scan(ctx.handle, bm.handle, None, rcp.ctypes.data_as(C.POINTER(C.c_uint32)), n, None, 0, C.byref(prm), None,
                                   buf.ctypes.data_as(C.POINTER(_lib.PaintSegment)), total - 1, C.byref(n_seg), None, None, None, None)
    assert rc == 0 and n_seg.value == total and (buf.view(np.uint8) == 0xAB).all()
    bm.free()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------

def refusal_cases(n, S):
    """(kwargs of BitMatrix.paint_scan with `recipients`, the code)"""
    one = np.zeros(n, np.uint8)
    one[4] = 1
    bad_cost = np.ones(S, np.uint32)
    bad_cost[S // 2] = (1 << 20) + 1
    pan = np.zeros(n, np.uint8)
    pan[3] = 2
    return [
        (dict(recipients=[0], site_begin=100, site_end=100), E_INVALID), (dict(recipients=[0], site_begin=200, site_end=100), E_INVALID),
        (dict(recipients=[0], site_end=S + 1), E_INVALID), (dict(recipients=[0], site_begin=S), E_INVALID),
        (dict(recipients=[]), E_INVALID), (dict(recipients=[n]), E_INVALID), (dict(recipients=[1, 2, 1]), E_INVALID),
        (dict(recipients=[4], donors=one), E_INVALID), (dict(recipients=[0], donors=np.zeros(n, np.uint8)), E_INVALID),
        (dict(recipients=[0], mismatch_cost=0), E_INVALID), (dict(recipients=[0], mismatch_cost=65536), E_INVALID),
        (dict(recipients=[0], switch_cost=(1 << 20) + 1), E_INVALID), (dict(recipients=[0], site_switch_cost=bad_cost), E_INVALID),
        (dict(recipients=[0], site_switch_cost=np.ones(S - 1, np.uint32)), E_INVALID),
        (dict(recipients=[0], site_begin=10, site_end=S - 10, site_switch_cost=np.ones(S, np.uint32)), E_INVALID),
        (dict(recipients=[0], panel=pan, n_panels=2), E_INVALID), (dict(recipients=[0], n_panels=2), E_INVALID),
        (dict(recipients=[0], windows=[(50, 40)]), E_INVALID),
        (dict(recipients=[0], panel=np.zeros(n, np.uint8), n_panels=9), E_UNSUPPORTED),
    ]


def raw_refusals(ctx, bm, good=True):
    """a wrong struct_size; win_out without windows; good: and the same call in order -> the codes"""
    import impop_amd
    from impop_amd import _lib
    rcp = np.zeros(1, dtype=np.uint32)
    n_seg = C.c_uint64(0)
    win = np.zeros(1, dtype=impop_amd.PAINT_WINDOW_DTYPE)

    def raw(size, win_out):
        prm = _lib.PaintParams(size, 1, 1, 0, 0, 0, None, 0, None, None, 0)
        return ctx._lib.impop_paint_scan(ctx.handle, bm.handle, None, rcp.ctypes.data_as(C.POINTER(C.c_uint32)), 1, None, 0, C.byref(prm),
                                         None, None, 0, C.byref(n_seg), None, None, win_out, None)
    codes = [raw(C.sizeof(_lib.PaintParams) - 8, None), raw(C.sizeof(_lib.PaintParams), win.ctypes.data_as(C.POINTER(_lib.PaintWindow)))]
    return codes + [raw(C.sizeof(_lib.PaintParams), None)] if good else codes


def test_refusals(ctx):
    from impop_amd import ImpopError, _lib
    rng = np.random.default_rng(8000)
    n, S = 12, 260
    m01 = pc.mosaic_matrix(rng, n, S)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    for kw, code in refusal_cases(n, S):
        kw = dict(kw)
        with pytest.raises(ImpopError) as ei:
            bm.paint_scan(kw.pop("recipients"), **kw)
        assert ei.value.code == code, kw
    assert raw_refusals(ctx, bm) == [E_INVALID, E_INVALID, 0]
    kw = dict(recipients=[0, 5], mu=2, c=3)
    pc.assert_equal(scan(bm, kw), pc.reference(m01, **kw), "after the refusals")  # the context is still usable
    bm.free()
    # over the limits: 1025 admissible donors; 4097 recipients
    big = ctx.upload_dense(np.zeros((_lib.PAINT_MAX_RECIPIENTS + 1, 64), np.uint8), keep_hap_major=False)
    donors = np.zeros(big.n_hap, np.uint8)
    donors[:_lib.PAINT_MAX_DONORS + 2] = 1
    for kw in (dict(recipients=[1], donors=donors), dict(recipients=[2000], donors=donors[::-1].copy() | donors),
               dict(recipients=np.arange(big.n_hap), donors=donors)):
        with pytest.raises(ImpopError) as ei:
            big.paint_scan(kw.pop("recipients"), **kw)
        assert ei.value.code == E_UNSUPPORTED
    donors[0] = 0
    assert big.paint_scan([1], donors=donors)["recipients"]["n_donors"].tolist() == [_lib.PAINT_MAX_DONORS]  # the limit itself
    big.free()


# ---- stale memory, the error bit, the timers ---------------------------------------------------------------------------------------------

def test_two_calls_on_one_context_are_independent(ctx):
    rng = np.random.default_rng(9000)
    big = pc.mosaic_matrix(rng, 90, 700)
    small = pc.mosaic_matrix(rng, 9, 130)
    bm1, bm2 = ctx.upload_dense(big, keep_hap_major=False), ctx.upload_dense(small, keep_hap_major=False)
    kw1 = dict(recipients=some_recipients(90, 12), mu=2, c=3, windows=pc.window_list(0, 700))
    kw2 = dict(recipients=[8, 0, 4], mu=1, c=1, b=5, e=120, windows=pc.window_list(5, 120))
    want1, want2 = pc.reference(big, **kw1), pc.reference(small, **kw2)
    for _ in range(2):
        pc.assert_equal(scan(bm1, kw1), want1, "large")
        pc.assert_equal(scan(bm2, kw2), want2, "small after large")
    bm1.free()
    bm2.free()


def test_error_bit_surfaces(ctx):
    from impop_amd import ImpopError, _lib
    m01 = pc.mosaic_matrix(np.random.default_rng(9100), 8, 100)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    assert ctx._lib.impop_debug_raise_device_error(ctx.handle, 8192) == 0
    with pytest.raises(ImpopError) as ei:
        bm.paint_scan([0])
    assert ei.value.code == E_INTERNAL and "painting" in ei.value.message
    kw = dict(recipients=[0, 7], mu=1, c=2)
    pc.assert_equal(scan(bm, kw), pc.reference(m01, **kw), "after the error")  # the word was cleared
    bm.free()


def test_timers_bracket_the_four_kernels(ctx, monkeypatch):
    monkeypatch.setenv(ENV, "2")
    m01 = pc.mosaic_matrix(np.random.default_rng(9200), 20, 700)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    ctx.gram_timing(True)
    bm.paint_scan([0, 3, 9], windows=[(0, 700)])
    ms, chunks = ctx.paint_elapsed()
    ctx.gram_timing(False)
    assert chunks == 6 and len(ms) == 4 and all(t > 0.0 for t in ms)  # 11 blocks in chunks of 2
    bm.free()


# ---- chunk independence, recipient ranges and the silent refusals: the trace line, in a child process under IMPOP_TRACE=1 ----------------

CHILD_N, CHILD_S, CHILD_B, CHILD_E = 30, 760, 29, 729  # a 700-site range: 12 blocks, unaligned at both ends


def child_case():
    m01 = pc.mosaic_matrix(np.random.default_rng(9300), CHILD_N, CHILD_S)
    panel = (np.arange(CHILD_N) % 2).astype(np.uint8)
    kw = dict(recipients=list(range(0, CHILD_N, 2)), mu=2, c=3, b=CHILD_B, e=CHILD_E, windows=pc.window_list(CHILD_B, CHILD_E), panel=panel,
              n_panels=2)
    return m01, kw


def _child(out_path):
    import impop_amd
    from impop_amd import ImpopError
    ctx = impop_amd.Context(0)
    out = {}
    m01, kw = child_case()
    bm = ctx.upload_dense(m01, keep_hap_major=False)

    def call(tag, m, env=None, **extra):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        if env is None:
            os.environ.pop(ENV, None)
        else:
            os.environ[ENV] = str(env)
        got = scan(m, kw, **extra)
        for k in pc.KEYS:
            out[f"{tag}_{k}"] = got[k]
        sys.stderr.flush()

    call("default", bm)
    call("chunk1", bm, env=1)
    call("chunk3", bm, env=3)
    call("ranges", bm, max_chunk_bytes=2 * 4 * 700 * 8)  # records of 4 recipients: 15 recipients in 4 ranges
    call("both", bm, env=5, max_chunk_bytes=2 * 7 * 700 * 8)
    cm = bm.compact()
    call("compact", cm)
    cm.free()
    os.environ.pop(ENV, None)
    sys.stderr.write("@@call refused\n")
    sys.stderr.flush()
    codes = []
    for rkw, _ in refusal_cases(CHILD_N, CHILD_S):
        rkw = dict(rkw)
        try:
            bm.paint_scan(rkw.pop("recipients"), **rkw)
            codes.append(0)
        except ImpopError as exc:
            codes.append(exc.code)
    codes += raw_refusals(ctx, bm, good=False)
    out["refused"] = np.array(codes)
    sys.stderr.flush()
    bm.free()
    ctx.close()
    np.savez(out_path, **out)


_TRACE = re.compile(r"\[impop_paint_scan\] (.*)$")


def test_chunks_ranges_and_the_trace_line():
    m01, kw = child_case()
    want = pc.reference(m01, **kw)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
        env.pop(ENV, None)
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_paint_scan as t; t._child(sys.argv[1])", path],
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
    for tag in ("default", "chunk1", "chunk3", "ranges", "both"):
        for k in pc.KEYS:
            assert recs[f"{tag}_{k}"].tobytes() == want[k].tobytes(), (tag, k)
    assert [len(trace[t]) for t in ("default", "chunk1", "chunk3", "ranges", "both", "compact", "refused")] == [1, 1, 1, 1, 1, 1, 0]
    want_codes = [code for _, code in refusal_cases(CHILD_N, CHILD_S)] + [E_INVALID, E_INVALID]
    assert recs["refused"].tolist() == want_codes  # every refusal, and nothing was launched: no trace line
    t = trace["default"][0]
    assert list(t) == ["route", "recipients", "donors", "sites", "site_chunks", "recipient_ranges", "segments", "launches", "bytes_streamed"]
    assert (t["route"], t["recipients"], t["donors"], t["sites"]) == ("dense", 15, CHILD_N, 700)
    assert (t["site_chunks"], t["recipient_ranges"], t["segments"]) == (1, 1, want["n_segments"])
    assert t["launches"] == 1 + 1 + 2 + 2 + 1  # transpose; forward; count, emit; mismatch, windows; records
    blocks = (CHILD_E + 63) // 64 - CHILD_B // 64
    assert blocks == 12
    # several site chunks: every range transposes them for the forward pass and again for the mismatch and window kernels
    assert trace["chunk1"][0]["site_chunks"] == 2 * 12 and trace["chunk3"][0]["site_chunks"] == 2 * 4
    assert trace["ranges"][0]["recipient_ranges"] == 4 and trace["ranges"][0]["site_chunks"] == 1
    assert trace["both"][0]["recipient_ranges"] == 3 and trace["both"][0]["site_chunks"] == 3 * 2 * 3
    assert all(trace[k][0]["segments"] == want["n_segments"] for k in ("chunk1", "chunk3", "ranges", "both"))
    assert trace["compact"][0]["route"] == "compact" and trace["compact"][0]["sites"] <= 700


# ---- the command line -----------------------------------------------------------------------------------------------------------------

def test_cli_tables_are_the_records(tmp_path):
    from impop_amd import pack_hap_major, paint
    from impop_amd.matrixio import MatrixFile, save_matrix
    rng = np.random.default_rng(9400)
    n, W, origin = 14, 500, 7000
    m01 = pc.mosaic_matrix(rng, n, W, nf=4)
    names = [f"S{i // 2:02d}#{i % 2 + 1}#chrT:0-1" for i in range(n - 1)] + ["CHM13#0#chrT:0-1"]
    mpath, bed = str(tmp_path / "m.npz"), str(tmp_path / "w.bed")
    save_matrix(mpath, MatrixFile(bits=pack_hap_major(m01), n_site=W, names=names, origin=origin, contig="chrT"))
    rows = [(0, 130), (100, 300), (250, 251), (300, 500), (0, 500)]
    open(bed, "w").write("".join(f"chrT\t{origin + b}\t{origin + e}\n" for b, e in rows))
    lists = {"rec": names[0:6], "don": names[2:], "east": names[2:7], "west": names[7:11]}
    for k, v in lists.items():
        open(str(tmp_path / f"{k}.txt"), "w").write("".join(x[:x.index("chrT")] + "\n" for x in v))  # PanSN prefixes: S00#1#
    group = np.arange(n)
    for i in range(0, n - 2, 2):
        group[i + 1] = group[i]  # S06 has one copy only: alone, as CHM13 is
    donors = np.array([nm in lists["don"] for nm in names], dtype=np.uint8)
    panel = np.array([0 if nm in lists["east"] else 1 if nm in lists["west"] else pc.NO_PANEL for nm in names])
    want = pc.reference(m01, list(range(6)), donors=donors, mu=2, c=3, group=group, panel=panel, n_panels=2, windows=rows)
    regions = [f"CHM13#0#chrT:{origin + b}-{origin + e}" for b, e in rows]

    def text(columns, body):
        return "\n".join("\t".join(r) for r in [columns] + body) + "\n"
    out = {k: str(tmp_path / f"{k}.tsv") for k in ("seg", "rec", "cc", "cl", "anc")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_paint.py"), "--matrix", mpath, "--bed", bed, "-u", str(tmp_path / "rec.txt"),
                        "--paint-donors", str(tmp_path / "don.txt"), "--panel", str(tmp_path / "east.txt"), str(tmp_path / "west.txt"),
                        "--paint-by-sample", "--paint-mismatch", "2", "--paint-switch", "3", "--paint-segments", out["seg"],
                        "--paint-recipients", out["rec"], "--paint-chunkcounts", out["cc"], "--paint-chunklengths", out["cl"],
                        "--paint-ancestry", out["anc"]], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == text(paint.MAIN_COLUMNS, paint.main_rows(regions, [e - b for b, e in rows], [6] * len(rows), want["windows"]))
    assert open(out["seg"]).read() == text(paint.SEGMENT_COLUMNS, paint.segment_rows(names, want["segments"], lambda c: origin + c))
    assert open(out["rec"]).read() == text(paint.RECIPIENT_COLUMNS, paint.recipient_rows(names, want["recipients"]))
    assert open(out["cc"]).read() == text(*paint.chunk_matrix(names, want["recipients"], want["chunk_counts"], donors))
    assert open(out["cl"]).read() == text(*paint.chunk_matrix(names, want["recipients"], want["chunk_sites"], donors))
    assert open(out["anc"]).read() == text(paint.ANCESTRY_COLUMNS, paint.ancestry_rows(regions, names, want["recipients"], want["anc"], ["east", "west"]))
    # a spot check that does not go through impop_amd/paint.py: the first segment row and a chunk-count header
    first = want["segments"][0]
    assert open(out["seg"]).read().splitlines()[1] == f"{names[0]}\t{names[int(first['donor'])]}\t{origin}\t{origin + int(first['end'])}\t" \
                                                       f"{int(first['n_sites'])}\t{int(first['n_mismatch'])}"
    assert open(out["cc"]).read().splitlines()[0].split("\t") == ["RECIPIENT"] + lists["don"]
    # the per-site costs of a map: the cost array the scan gets is switch_costs_from_map's
    mp = str(tmp_path / "t.map")
    open(mp, "w").write(f"chrT\ta\t0.0\t{origin}\nchrT\tb\t0.002\t{origin + 250}\nchrT\tc\t0.5\t{origin + W}\n")
    cost = paint.switch_costs_from_map(np.arange(W), [0, 250, W], [0.0, 0.002, 0.5], rho=50.0, scale=2.0)
    assert 0 < cost[300] < cost[100] < paint.MAX_COST
    want = pc.reference(m01, list(range(6)), donors=donors, mu=2, site_cost=cost, windows=rows)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_paint.py"), "--matrix", mpath, "--bed", bed, "-u", str(tmp_path / "rec.txt"),
                        "--paint-donors", str(tmp_path / "don.txt"), "--paint-mismatch", "2", "--paint-map", mp, "--paint-rho", "50",
                        "--paint-scale", "2", "--paint-segments", out["seg"]], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout == text(paint.MAIN_COLUMNS, paint.main_rows(regions, [e - b for b, e in rows], [6] * len(rows), want["windows"]))
    assert open(out["seg"]).read() == text(paint.SEGMENT_COLUMNS, paint.segment_rows(names, want["segments"], lambda c: origin + c))
