"""impop_ehh_scan on an MI355X (run with -m gpu): integrated EHH per core site for a batch of windows.

The expected records come from the reference's own output (tests/golden/ehh.json) and from the plain partition-refinement
reference tests/plain_refs.ref_ehh: area_milli[a][h] = sum(round(1000 * EHH[i])) over the half's sites, an integer, so
every comparison of thousandths is exact.  The one tolerance, |area - float(reference text)| <= 1e-12, is the issue's: the
reference's np.cumsum is a left-to-right fp64 sum of W <= 40 values below 1000 (2 W 2^-52 area < 1e-12 for every golden row)."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import plain_refs as pr
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


def _flags(idx, n):
    f = np.zeros(n, np.uint8)
    f[np.asarray(idx, dtype=np.int64)] = 1
    return f


def _founders(rng, n, S, nf=7, pf=0.02, pp=0.0015):
    """few haplotype classes, long runs without a split (the generator of test_gpu_upper_range)"""
    anc = rng.integers(0, 2, size=S, dtype=np.uint8)
    f = np.repeat(anc[None, :], nf, axis=0) ^ (rng.random((nf, S)) < pf).astype(np.uint8)
    return f[rng.integers(0, nf, size=n)] ^ (rng.random((n, S), dtype=np.float32) < pp).astype(np.uint8)


def _bernoulli(rng, n, S):
    """many splits inside one 64-site word: the curve is at 0 within about log2 n sites"""
    return (rng.random((n, S)) < 0.5).astype(np.uint8)


def _milli(values):
    return sum(round(v * 1000) for v in values)


def expected(m01, flags, b, e, c, flanks, ref_hap, cache):
    """one record from the plain reference: ([n0, n1], ref_allele, [[a0h0, a0h1], [a1h0, a1h1]])"""
    n = m01.shape[0]
    in_p = np.ones(n, bool) if flags is None else np.asarray(flags).astype(bool)
    col = m01[:, c] != 0
    members, milli = [0, 0], [[0, 0], [0, 0]]
    for a in (0, 1):
        mem = in_p & (col == bool(a))
        members[a] = int(mem.sum())
        for h in (0, 1):
            right = h == 1 or flanks == "reference"
            lo, hi = (c + 1, e) if right else (b, c)
            if members[a] == 0 or hi <= lo:
                continue  # nobody, or an empty flank: 0
            key = (mem.tobytes(), lo, hi, h == 0)
            if key not in cache:
                cache[key] = _milli(pr.ref_ehh(m01[:, lo:hi], mem.astype(np.uint8), reverse=(h == 0)))
            milli[a][h] = cache[key]
    return members, int(col[ref_hap]), milli


def check_records(rec, m01, flags, windows, cores, flanks, ref_hap, cache, tag):
    assert len(rec) == len(windows)
    for r, (b, e), c in zip(rec, windows, cores):
        members, ref, milli = expected(m01, flags, b, e, c, flanks, ref_hap, cache)
        where = (tag, flanks, b, e, c)
        assert r["n_members"].tolist() == members, where
        assert int(r["ref_allele"]) == ref and int(r["reserved"]) == 0, where
        assert r["area_milli"].tolist() == milli, where
        assert r["area"].tolist() == [(milli[a][0] + milli[a][1]) / 1000.0 for a in (0, 1)], where


# ---- 1. the reference's own output ------------------------------------------------------------------------------------------

def _golden_matrix(case):
    whole = np.array([[float(x) for x in line.split()] for line in case["matrix_text"].splitlines()])
    return (whole != 0).astype(np.uint8)  # ehhgfa.py:50


def test_reference_goldens(ctx):
    from impop_amd import ehh
    cases = load_golden("ehh.json")["cli"]
    n_rows = single = 0
    for c in cases:
        m01 = _golden_matrix(c)
        bm = ctx.upload_dense(m01, keep_hap_major=False)
        if c["rc"] == 0:
            rows = ehh.scan_matrix(bm, c["w"], c["p"], c["refpos"])
            want = [line.split() for line in c["out"].splitlines()]
            assert len(rows) == len(want)
            for (name, cs, ce, al, label, milli, area), w in zip(rows, want):
                print(name, cs, ce, al, label, milli, area, "reference:", w[5])
                assert [name, cs, ce] == [int(x) for x in w[:3]] and float(al) == float(w[3]) and label == w[4]
                assert milli == round(float(w[5]) * 1000)
                assert abs(area - float(w[5])) <= 1e-12
                n_rows += 1
                single += w[5] == "12000" and milli == 12_000_000
        else:  # the test SNP is the window's last column: scan_matrix raises the reference's error, the scan itself returns 0
            with pytest.raises(IndexError) as ei:
                ehh.scan_matrix(bm, c["w"], c["p"], c["refpos"])
            assert "IndexError: " + str(ei.value) == c["stderr_last"]
            n_col = m01.shape[1]
            wins = [(s, min(s + c["w"], n_col)) for s in range(0, n_col, c["w"])]
            cores = [s + c["p"] - 1 for s, _ in wins]
            rec = bm.ehh_scan(wins, cores, ref_hap=c["refpos"] - 1)
            assert not rec["area_milli"].any() and not rec["area"].any()
            assert (rec["n_members"].sum(axis=1) == m01.shape[0]).all()
        bm.free()
    assert n_rows == 10 and single == 1


# ---- 2. exactness against the plain reference ----------------------------------------------------------------------------------

WIDTHS = (1, 2, 63, 64, 65, 129, 1025)
STARTS = (64, 37)


def _window_cores():
    """every (W, start) with its first, last and an interior site as core; the windows of 65 and 129 sites also with the first
    bit 0 and the first bit 63 of a 64-site word inside them"""
    wins, cores = [], []
    for W in WIDTHS:
        for s0 in STARTS:
            cs = {s0, s0 + W - 1, s0 + W // 2}
            if W in (65, 129):
                cs |= {next(c for c in range(s0, s0 + W) if c % 64 == 0), next(c for c in range(s0, s0 + W) if c % 64 == 63)}
            for c in sorted(cs):
                wins.append((s0, s0 + W))
                cores.append(c)
    return wins, cores


@pytest.mark.parametrize("kind", ("founders", "bernoulli"))
@pytest.mark.parametrize("n", (2, 63, 64, 65, 257, 465, 1030))
def test_exact_against_plain_reference(ctx, n, kind):
    rng = np.random.default_rng(4100 + n + (1000 if kind == "bernoulli" else 0))
    S = 64 + 1025 + 40
    m01 = _founders(rng, n, S) if kind == "founders" else _bernoulli(rng, n, S)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    wins, cores = _window_cores()
    ref_hap = n // 2
    cache = {}
    for flags in (None, (rng.random(n) < 0.6).astype(np.uint8)):
        for flanks in ("reference", "two-sided"):
            rec = bm.ehh_scan(wins, cores, mask=flags, ref_hap=ref_hap, flanks=flanks)  # all (W, start, core) in one call
            check_records(rec, m01, flags, wins, cores, flanks, ref_hap, cache, (n, kind, flags is not None))
    # a mask that leaves allele 1 of the core with 0, 1 and 2 members (the site of the window with the most even split)
    b, e = 37, 37 + 129
    c = b + 1 + int(np.argmin(np.abs(m01[:, b + 1:e - 1].sum(axis=0) * 2 - n)))
    ones, zeros = np.flatnonzero(m01[:, c] == 1), np.flatnonzero(m01[:, c] == 0)
    for k in (0, 1, 2):
        if len(ones) < k or len(zeros) == 0:
            continue
        flags = _flags(np.concatenate([zeros, ones[:k]]), n)
        for flanks in ("reference", "two-sided"):
            rec = bm.ehh_scan([(b, e)], [c], mask=flags, ref_hap=int(zeros[0]), flanks=flanks)
            assert rec["n_members"].tolist() == [[len(zeros), k]]
            check_records(rec, m01, flags, [(b, e)], [c], flanks, int(zeros[0]), cache, (n, kind, "few", k))
            want = [0, 500000 * (e - c - 1) if flanks == "reference" else 500000 * (c - b), None][k]
            assert want is None or int(rec["area_milli"][0][1][0]) == want
    bm.free()


# ---- 3. curves that never break ------------------------------------------------------------------------------------------

def test_curves_that_never_break(ctx):
    """two identical haplotypes keep one pair homozygous to the end of both flanks: among 513 members (the pair rounds to
    0.000) and among three (0.333 to the end)"""
    rng = np.random.default_rng(4300)
    n, S = 513, 700
    m01 = _bernoulli(rng, n, S)
    m01[400] = m01[7]
    core = 350
    third = int(next(i for i in range(n) if i not in (7, 400) and m01[i, core] == m01[7, core]))
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    cache = {}
    a = int(m01[7, core])
    for flags in (None, _flags([7, 400, third], n)):
        for flanks in ("reference", "two-sided"):
            rec = bm.ehh_scan([(0, S), (3, 650)], [core, core], mask=flags, ref_hap=7, flanks=flanks)
            check_records(rec, m01, flags, [(0, S), (3, 650)], [core, core], flanks, 7, cache, "never")
            if flags is not None:  # 0.333 at every site once the third member has left: far above what a broken pair leaves
                assert rec["n_members"][0].tolist()[a] == 3 and int(rec["area_milli"][0][a][1]) >= 333 * (S - core - 1)
    bm.free()


# ---- 4. the upper end of the documented range ------------------------------------------------------------------------------

def test_4096_members(ctx):
    from impop_amd import _lib
    assert _lib.EHH_SCAN_MAX_N == 4096
    rng = np.random.default_rng(4400)
    n, S = 4096, 1200
    m01 = _founders(rng, n, S)
    m01[:, 600] = rng.integers(0, 2, size=n)  # a core that splits the panel in two large halves
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    wins = [(64, 64 + 1025), (37, 37 + 129), (100, 165), (590, 654), (0, 63), (600, 601)]
    cores = [600, 100, 164, 600, 0, 600]
    cache = {}
    rec = bm.ehh_scan(wins, cores, ref_hap=4095, flanks="two-sided")
    check_records(rec, m01, None, wins, cores, "two-sided", 4095, cache, "4096")
    rec = bm.ehh_scan(wins[:2], cores[:2], ref_hap=0, flanks="reference")
    check_records(rec, m01, None, wins[:2], cores[:2], "reference", 0, cache, "4096")
    assert rec["n_members"][0].sum() == 4096 and rec["n_members"][0].min() > 1500
    bm.free()


# ---- 5. agreement with impop_ehh ----------------------------------------------------------------------------------------------

def test_agrees_with_per_window_kernel(ctx):
    rng = np.random.default_rng(4500)
    n, S, W = 465, 5000 * 8 + 100, 5000
    m01 = _founders(rng, n, S, pf=0.004, pp=0.0004)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    wins = [(37 + k * W, 37 + (k + 1) * W) for k in range(8)]
    # cores where both alleles are common (the most even split of a stretch of each window), at varied offsets
    cores = []
    for k, (b, e) in enumerate(wins):
        lo = b + 1 + 590 * k
        cores.append(lo + int(np.argmin(np.abs(m01[:, lo:lo + 500].sum(axis=0) * 2 - n))))
    for flanks in ("reference", "two-sided"):
        rec = bm.ehh_scan(wins, cores, flanks=flanks)
        for r, (b, e), c in zip(rec, wins, cores):
            for a in (0, 1):
                mem = (m01[:, c] == a).astype(np.uint8)
                assert int(r["n_members"][a]) == int(mem.sum())
                for h in (0, 1):
                    lo, hi = (c + 1, e) if (h == 1 or flanks == "reference") else (b, c)
                    vec = bm.ehh(lo, hi, mem, reverse=(h == 0))
                    want = int(np.rint(1000.0 * vec).astype(np.int64).sum()) if mem.sum() else 0
                    assert int(r["area_milli"][a][h]) == want, (flanks, b, e, c, a, h)
    bm.free()


# ---- 6. batch invariants (and 4. the limit + 1) in a child process under IMPOP_TRACE=1 ------------------------------------------

BATCH_N, BATCH_S = 465, 7 * 300 + 200


def _batch_inputs():
    rng = np.random.default_rng(4600)
    m01 = _founders(rng, BATCH_N, BATCH_S, pf=0.03, pp=0.003)
    wins = [(7 * k, 7 * k + 130) for k in range(300)]
    cores = [b + (k * 37) % 130 for k, (b, _) in enumerate(wins)]
    flags = (rng.random(BATCH_N) < 0.6).astype(np.uint8)
    return m01, wins, cores, flags


CAP_N, CAP_S, CAP_PERIOD, CAP_WINDOWS = 8, 512, 200, 65536  # one window more than a launch's blockIdx.y holds


def _cap_inputs():
    """65536 three-site windows, the core in the middle, the list repeating with period 200"""
    m01 = _bernoulli(np.random.default_rng(4650), CAP_N, CAP_S)
    begins = (np.arange(CAP_WINDOWS) % CAP_PERIOD) * 5 % (CAP_S - 3)
    return m01, np.stack([begins, begins + 3], axis=1), begins + 1


def _child(out_path):
    import signal

    import impop_amd
    from impop_amd import ImpopError
    m01, wins, cores, flags = _batch_inputs()
    ctx = impop_amd.Context(0)
    bm = ctx.upload_dense(m01, keep_hap_major=False)

    def call(tag, fn):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        return fn()

    out = {}
    out["w300"] = call("w300", lambda: bm.ehh_scan(wins, cores, mask=flags, flanks="two-sided"))
    out["w30"] = call("w30", lambda: bm.ehh_scan(wins[:30], cores[:30], mask=flags, flanks="two-sided"))
    per_window = 3 * int(flags.sum()) * 8  # a 130-site window touches 3 or 4 blocks of 64 sites
    out["chunked"] = call("chunked", lambda: bm.ehh_scan(wins, cores, mask=flags, flanks="two-sided", max_chunk_bytes=90 * per_window))
    bm.free()
    cap_m01, cap_wins, cap_cores = _cap_inputs()
    small = ctx.upload_dense(cap_m01, keep_hap_major=False)
    signal.alarm(120)  # this step's own limit (some 260000 tiny workgroups: seconds); the default action ends the process
    out["cap"] = call("cap", lambda: small.ehh_scan(cap_wins, cap_cores, flanks="two-sided"))
    signal.alarm(0)
    small.free()
    big = ctx.upload_dense(np.zeros((4097, 200), np.uint8), keep_hap_major=False)
    try:
        call("over", lambda: big.ehh_scan([(0, 200)], [100]))
        out["over"] = np.array([0])
    except ImpopError as exc:
        out["over"] = np.array([exc.code])
    served = call("subset", lambda: big.ehh_scan([(0, 200)], [100], mask=_flags(np.arange(1, 4097), 4097)))  # 4096 of 4097 are served
    out["subset"] = served
    big.free()
    ctx.close()
    np.savez(out_path, **out)


_TRACE = re.compile(r"\[impop_ehh_scan\] (.*)$")


@pytest.fixture(scope="module")
def child():
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_ehh_scan as t; t._child(sys.argv[1])", path],
                           capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
        assert r.returncode != -14, "the child's 65536-window step (cap) ran into its own 120 s limit (SIGALRM): a hang\n" + r.stderr[-2000:]
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
            trace[cur].append({k: int(v) for k, v in (kv.split("=") for kv in mt.group(1).split())})
    return recs, trace


def test_chunking_never_changes_a_record(ctx, child):
    recs, trace = child
    assert len(trace["w300"]) == 1 and len(trace["chunked"]) >= 3
    assert sum(t["windows"] for t in trace["chunked"]) == 300 and [t["chunk"] for t in trace["chunked"]] == list(range(len(trace["chunked"])))
    assert recs["w300"].tobytes() == recs["chunked"].tobytes()
    assert recs["w300"][:30].tobytes() == recs["w30"].tobytes()
    m01, wins, cores, flags = _batch_inputs()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    cache = {}
    for k in (0, 1, 29, 30, 89, 90, 91, 150, 298, 299):  # chunk edges of the forced chunking among them
        one = bm.ehh_scan([wins[k]], [cores[k]], mask=flags, flanks="two-sided")
        assert one.tobytes() == recs["w300"][k:k + 1].tobytes(), k
        check_records(one, m01, flags, [wins[k]], [cores[k]], "two-sided", 0, cache, "batch")
    bm.free()


def test_launches_do_not_depend_on_the_number_of_windows(child):
    _, trace = child
    (a,), (b,) = trace["w30"], trace["w300"]
    assert a["windows"] == 30 and b["windows"] == 300 and a["problems"] == 120 and b["problems"] == 1200
    assert a["launches"] == b["launches"] and 1 <= a["launches"] <= 3
    assert b["scratch_bytes"] > a["scratch_bytes"] > 0
    for t in trace["chunked"]:
        assert t["launches"] == a["launches"]


def test_window_cap_of_one_launch_cuts_a_second_chunk(child):
    """65536 windows, far below the byte budget: the 65535 windows that blockIdx.y holds, then one; the records do not notice"""
    recs, trace = child
    assert [(t["chunk"], t["windows"]) for t in trace["cap"]] == [(0, 65535), (1, 1)]
    rec = recs["cap"]
    m01, wins, cores = _cap_inputs()
    check_records(rec[:CAP_PERIOD], m01, None, wins[:CAP_PERIOD].tolist(), cores[:CAP_PERIOD].tolist(), "two-sided", 0, {}, "cap")
    assert len(rec) == CAP_WINDOWS and rec[np.arange(CAP_WINDOWS) % CAP_PERIOD].tobytes() == rec.tobytes()


def test_limit_plus_one_is_refused_before_any_launch(child):
    recs, trace = child
    assert recs["over"].tolist() == [E_UNSUPPORTED] and trace["over"] == []
    assert len(trace["subset"]) == 1 and recs["subset"]["n_members"].tolist() == [[4096, 0]]


# ---- 7. errors ----------------------------------------------------------------------------------------------------------

def test_errors(ctx):
    import impop_amd
    from impop_amd import ImpopError
    rng = np.random.default_rng(4700)
    n, S = 40, 300
    m01 = _founders(rng, n, S)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    for wins, cores, kw, code in (([(10, 100)], [100], {}, E_INVALID),       # the core is site_end
                                  ([(10, 100)], [9], {}, E_INVALID),         # the core is left of the window
                                  ([(100, 10)], [50], {}, E_INVALID),        # a bad range
                                  ([(10, S + 1)], [50], {}, E_INVALID),      # past the matrix
                                  ([(10, 100)], [50], {"ref_hap": n}, E_INVALID)):
        with pytest.raises(ImpopError) as ei:
            bm.ehh_scan(wins, cores, **kw)
        assert ei.value.code == code, (wins, cores, kw)
    empty = bm.ehh_scan(np.zeros((0, 2), np.int64), [])
    assert empty.dtype == impop_amd.EHH_DTYPE and len(empty) == 0
    ok = bm.ehh_scan([(10, 100)], [99], ref_hap=n - 1)
    assert ok["n_members"].sum() == n
    cm = bm.compact()
    with pytest.raises(ImpopError) as ei:
        cm.ehh_scan([(10, 100)], [50])
    assert ei.value.code == E_UNSUPPORTED
    cm.free()
    bm.free()


# ---- 8. the command line ----------------------------------------------------------------------------------------------------

def test_cli_rows_are_the_records(ctx, tmp_path):
    from impop_amd.matrixio import MatrixFile, save_matrix
    from impop_amd import pack_hap_major
    rng = np.random.default_rng(4800)
    n, S, origin = 40, 900, 5000
    m01 = _founders(rng, n, S, nf=5, pf=0.05, pp=0.01)
    names = [f"S{i:02d}#1#chrT:0-1" for i in range(n)]
    mpath, bed, sub = str(tmp_path / "m.npz"), str(tmp_path / "w.bed"), str(tmp_path / "u.txt")
    save_matrix(mpath, MatrixFile(bits=pack_hap_major(m01), n_site=S, names=names, origin=origin, contig="chrT"))
    rows = [(0, 130), (100, 300), (250, 251), (300, 900), (837, 900)]
    open(bed, "w").write("".join(f"chrT\t{origin + b}\t{origin + e}\n" for b, e in rows))
    keep = sorted(rng.choice(n, 31, replace=False).tolist())
    open(sub, "w").write("".join(names[i].partition("chrT")[0] + "\n" for i in keep))  # PanSN prefixes "S07#1#"
    flags = _flags(keep, n)
    bm = ctx.upload_dense(m01, keep_hap_major=False)

    def table(recs, cores):
        out = ["REGION\tLENGTH\tCORE\tALLELE\tREF_ALT\tN_HAPLOTYPES\tAREA\tIHH_LEFT\tIHH_RIGHT"]
        for (b, e), c, r in zip(rows, cores, recs):
            for a in (0, 1):
                if r["n_members"][a]:
                    lr = [int(x) for x in r["area_milli"][a]]
                    txt = [f"{k // 1000}.{k % 1000:03d}" for k in (lr[0] + lr[1], lr[0], lr[1])]
                    out.append("\t".join([f"CHM13#0#chrT:{origin + b}-{origin + e}", str(e - b), str(origin + c), str(a),
                                          "REF" if a == int(r["ref_allele"]) else "ALT", str(int(r["n_members"][a]))] + txt))
        return "\n".join(out) + "\n"

    def run(extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", mpath, "--bed", bed, "--format", "ehh"]
                           + extra, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout

    mid = [b + (e - b) // 2 for b, e in rows]
    assert run([]) == table(bm.ehh_scan(rows, mid), mid)
    ref = keep[3]
    got = run(["-u", sub, "--ehh-flanks", "two-sided", "--ehh-ref", names[ref], "--ehh-core-offset", "0"])
    first = [b for b, _ in rows]
    assert got == table(bm.ehh_scan(rows, first, mask=flags, ref_hap=ref, flanks="two-sided"), first)
    cores = [17, 299, 250, 512, 899]
    cpath = str(tmp_path / "cores.txt")
    open(cpath, "w").write("# bp\n" + "".join(f"{origin + c}\n" for c in cores))
    assert run(["--ehh-cores", cpath]) == table(bm.ehh_scan(rows, cores), cores)
    assert len(run([]).splitlines()) >= 1 + len(rows)
    bm.free()
