"""impop_ld_scan on an MI355X (run with -m gpu): ZnS, mean |D'|, the perfect / complete pair counts and the Kim-Nielsen omega of
every window against the plain restatement of tests/ld_cases.py.  Integers and used_sites must be equal, doubles equal bit for
bit.  What needs the trace line (IMPOP_TRACE=1 is read once per process) runs in one child process per module."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import hap_cases as hc
import ld_cases as lc
from conftest import ROOT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
E_INVALID, E_UNSUPPORTED = -1, -5
S = lc.S


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


# ---- shapes: one- and two-dword edges, 15 dwords with a 3-dword tail; min_mac 1 and 4 straddle the rare-site limit ---------------

@pytest.mark.parametrize("n", (33, 64, 465))
def test_shapes_against_the_restatement(ctx, n):
    rng = np.random.default_rng(10100 + n)
    m01 = lc.planted_matrix(rng, n, p_flip=1e-3)
    lc.check_planted(m01)
    wins = lc.window_list()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    sub = (rng.random(n) < 0.6).astype(np.uint8)
    sub[:3] = 1
    for flags in (None, sub):
        for min_mac in (1, 4, 24):
            got = bm.ld_scan(wins, mask_p=flags, min_mac=min_mac, want_sites=True)
            lc.assert_matches(got, lc.reference(m01, flags, wins, min_mac, 512), (n, flags is None, min_mac))
            assert np.array_equal(bm.ld_scan(wins, mask_p=flags, min_mac=min_mac), got[0])  # the records alone
    rec = bm.ld_scan(wins)
    k0 = wins.index(lc.PLANT_WINDOWS[0])
    assert rec["n_qualifying"][k0:k0 + 7].tolist() == [0, 1, 2, 3, 4, 5, 0]
    assert rec["omega_split"][k0:k0 + 4].tolist() == [0, 0, 0, 0] and (rec["omega_max"][k0:k0 + 4] == 0.0).all()
    assert rec["n_perfect"][k0 + 5] >= 3 and rec["n_complete"][k0 + 5] > rec["n_perfect"][k0 + 5]
    assert rec["n_sites"][wins.index((200, 200))] == 0 and rec["n_used"][wins.index((0, S))] > 100
    assert (rec["omega_split"] > 0).any()
    bm.free()


def test_subset_in_which_variable_sites_are_monomorphic(ctx):
    rng = np.random.default_rng(10200)
    n = 465
    m01 = lc.planted_matrix(rng, n)
    x = m01[:, lc.PLANT[0]]
    flags = x.copy()  # the carriers of the planted column: it, its copy and its complement are monomorphic among them
    wins = lc.PLANT_WINDOWS + [(0, S), (900, 1300)]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    got = bm.ld_scan(wins, mask_p=flags, want_sites=True)
    ref = lc.reference(m01, flags, wins, 1, 512)
    lc.assert_matches(got, ref, "subset")
    assert got[0]["n_qualifying"][:6].tolist() == [0, 0, 0, 0, 1, 2]
    assert lc.reference(m01, None, wins, 1, 512)[0]["n_qualifying"][:6].tolist() == [0, 1, 2, 3, 4, 5]
    bm.free()


# ---- selection edges ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_sites", (8, 64))
def test_thinning_at_and_beyond_max_sites(ctx, max_sites):
    rng = np.random.default_rng(10300 + max_sites)
    n = 465
    m01 = lc.planted_matrix(rng, n, p_site=0.3)
    qual = lc.qualifying(m01, None, 2)
    assert len(qual) > 6 * max_sites + 10
    wins = [lc.windows_with_q(qual, q) for q in (max_sites - 1, max_sites, max_sites + 1, 2 * max_sites + 1, 6 * max_sites + 5)] + [(0, S)]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    got = bm.ld_scan(wins, min_mac=2, max_sites=max_sites, want_sites=True)
    ref = lc.reference(m01, None, wins, 2, max_sites)
    assert ref[0]["n_qualifying"][:5].tolist() == [max_sites - 1, max_sites, max_sites + 1, 2 * max_sites + 1, 6 * max_sites + 5]
    assert ref[0]["n_used"].tolist() == [max_sites - 1] + [max_sites] * 5
    lc.assert_matches(got, ref, max_sites)
    assert got[1].shape == (len(wins), max_sites)
    bm.free()


def test_1024_sites_are_more_than_a_workgroup_has_lanes(ctx):
    rng = np.random.default_rng(10400)
    n = 465
    m01 = lc.planted_matrix(rng, n, p_site=0.55)
    qual = lc.qualifying(m01, None, 1)
    assert len(qual) > 1300
    wins = [(0, S), lc.windows_with_q(qual, 1024), lc.windows_with_q(qual, 1025), lc.windows_with_q(qual, 700)]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    got = bm.ld_scan(wins, max_sites=1024, want_sites=True)
    ref = lc.reference(m01, None, wins, 1, 1024)
    assert ref[0]["n_used"].tolist() == [1024, 1024, 1024, 700]
    lc.assert_matches(got, ref, "1024")
    bm.free()


def test_4096_members(ctx):
    from impop_amd import _lib
    assert _lib.LD_MAX_N == 4096 and _lib.LD_MAX_SITES == 1024
    rng = np.random.default_rng(10500)
    n, W = 4096, 400
    m01 = hc.founder_matrix(rng, n, W, p_site=0.3, p_flip=2e-4)
    wins = [(0, W), (37, 165), (100, 101), (64, 64), (300, 400)]
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    for max_sites in (64, 512):  # rows staged in LDS, rows read from the scratch
        got = bm.ld_scan(wins, min_mac=4, max_sites=max_sites, want_sites=True)
        ref = lc.reference(m01, None, wins, 4, max_sites)
        assert ref[0]["n_used"][0] >= 64
        lc.assert_matches(got, ref, ("4096", max_sites))
    bm.free()


# ---- invariance, under IMPOP_TRACE=1 in a child process -----------------------------------------------------------------------------

ROUTE_N = 465


def _route_inputs():
    rng = np.random.default_rng(10600)
    m01 = lc.planted_matrix(rng, ROUTE_N)
    weights = rng.integers(1, 9, size=S).astype(np.uint32)
    flags = (rng.random(ROUTE_N) < 0.8).astype(np.uint8)
    return m01, weights, flags, lc.window_list()


def _chunk_windows():
    return [(7 * k, 7 * k + 330) for k in range(120)]


def _child(out_path):
    import impop_amd
    from impop_amd import ImpopError
    ctx = impop_amd.Context(0)
    out = {}

    def call(tag, fn):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        r = fn()
        sys.stderr.flush()
        return r

    def keep(tag, res):
        out[tag], out[tag + "_sites"] = res

    m01, weights, flags, wins = _route_inputs()
    kw = dict(mask_p=flags, min_mac=2, max_sites=64, want_sites=True)
    ups = {"default": {}, "norare": {"rare_split": False}, "dense": {"dense_scan": True}}
    for tag, ukw in ups.items():
        bm = ctx.upload_dense(m01, keep_hap_major=False, **ukw)
        keep(tag, call(tag, lambda: bm.ld_scan(wins, **kw)))
        if tag == "default":
            cm = bm.compact()
            keep("compact", call("compact", lambda: cm.ld_scan(wins, **kw)))
            cm.free()
            perm = np.random.default_rng(1).permutation(len(wins))
            out["perm"] = perm
            keep("permuted", call("permuted", lambda: bm.ld_scan([wins[k] for k in perm], **kw)))
            cw = _chunk_windows()
            keep("w120", call("w120", lambda: bm.ld_scan(cw, **kw)))
            keep("w30", call("w30", lambda: bm.ld_scan(cw[:30], **kw)))
            keep("chunked", call("chunked", lambda: bm.ld_scan(cw, max_chunk_bytes=40 * 64 * (4 * 15 + 12), **kw)))
            keep("chunked_1", call("chunked_1", lambda: bm.ld_scan(wins, max_chunk_bytes=1, **kw)))
        bm.free()
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    bm.set_site_weights(weights)
    keep("weighted", call("weighted", lambda: bm.ld_scan(wins, **kw)))
    bm.free()
    big = ctx.upload_dense(np.zeros((4097, 200), np.uint8), keep_hap_major=False)
    try:
        call("over", lambda: big.ld_scan([(0, 200)]))
        out["over"] = np.array([0])
    except ImpopError as exc:
        out["over"] = np.array([exc.code])
    f = np.ones(4097, np.uint8)
    f[0] = 0
    out["subset4096"] = call("subset4096", lambda: big.ld_scan([(0, 200)], mask_p=f))
    big.free()
    ctx.close()
    np.savez(out_path, **out)


_TRACE = re.compile(r"\[impop_ld_scan\] (.*)$")


@pytest.fixture(scope="module")
def child():
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_ld_scan as t; t._child(sys.argv[1])", path],
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
    return recs, trace


def test_uploads_and_compaction_give_identical_bytes(child):
    recs, trace = child
    m01, weights, flags, wins = _route_inputs()
    ref = lc.reference(m01, flags, wins, 2, 64)
    lc.assert_matches((recs["default"], recs["default_sites"]), ref, "default")
    for tag in ("norare", "dense", "compact"):
        assert recs[tag].tobytes() == recs["default"].tobytes(), tag
        assert recs[tag + "_sites"].tobytes() == recs["default_sites"].tobytes(), tag
    # site weights change W and nothing else
    lc.assert_matches((recs["weighted"], recs["weighted_sites"]), lc.reference(m01, flags, wins, 2, 64, weights), "weighted")
    a, b = recs["weighted"].copy(), recs["default"].copy()
    a["n_sites"] = b["n_sites"] = 0
    assert a.tobytes() == b.tobytes() and recs["weighted_sites"].tobytes() == recs["default_sites"].tobytes()
    assert (recs["weighted"]["n_sites"] != recs["default"]["n_sites"]).any()
    assert [trace[t][0]["route"] for t in ("default", "norare", "dense", "compact", "weighted")] == ["dense", "dense", "dense", "compact", "dense"]
    for t in ("default", "compact"):
        assert len(trace[t]) == 1 and trace[t][0]["windows"] == len(wins)
        assert trace[t][0]["qualifying"] == int(ref[0]["n_qualifying"].sum()) and trace[t][0]["used"] == int(ref[0]["n_used"].sum())
    assert trace["compact"][0]["bytes_streamed"] < trace["default"][0]["bytes_streamed"]


def test_window_order_does_not_change_a_record(child):
    recs, _ = child
    perm = recs["perm"]
    assert recs["permuted"].tobytes() == recs["default"][perm].tobytes()
    assert recs["permuted_sites"].tobytes() == recs["default_sites"][perm].tobytes()


def test_chunking_never_changes_a_record(child):
    recs, trace = child
    assert trace["w120"][0]["chunks"] == 1 and trace["chunked"][0]["chunks"] >= 3
    assert recs["chunked"].tobytes() == recs["w120"].tobytes() and recs["chunked_sites"].tobytes() == recs["w120_sites"].tobytes()
    assert recs["w120"][:30].tobytes() == recs["w30"].tobytes()
    _, _, _, wins = _route_inputs()
    assert trace["chunked_1"][0]["chunks"] == len(wins)  # a budget of one byte: a chunk per window
    assert recs["chunked_1"].tobytes() == recs["default"].tobytes() and recs["chunked_1_sites"].tobytes() == recs["default_sites"].tobytes()
    m01, _, flags, _ = _route_inputs()
    cw = _chunk_windows()
    pick = [0, 1, 29, 30, 39, 40, 41, 119]
    want = lc.reference(m01, flags, [cw[k] for k in pick], 2, 64)
    lc.assert_matches((recs["w120"][pick], recs["w120_sites"][pick]), want, "w120")


def test_launches_do_not_depend_on_the_number_of_windows(child):
    _, trace = child
    (a,), (b,) = trace["w30"], trace["w120"]
    assert a["windows"] == 30 and b["windows"] == 120 and a["chunks"] == b["chunks"] == 1
    assert a["launches"] == b["launches"] and 3 <= a["launches"] <= 4
    assert trace["chunked"][0]["launches"] == a["launches"] * trace["chunked"][0]["chunks"]


def test_limit_plus_one_is_refused_before_any_launch(child):
    recs, trace = child
    assert recs["over"].tolist() == [E_UNSUPPORTED] and trace["over"] == []
    assert len(trace["subset4096"]) == 1 and recs["subset4096"]["n_members"].tolist() == [4096]
    assert recs["subset4096"]["n_qualifying"].tolist() == [0] and recs["subset4096"]["n_sites"].tolist() == [200]


# ---- errors -------------------------------------------------------------------------------------------------------------------------

def test_errors_and_empty_input(ctx):
    import impop_amd
    from impop_amd import ImpopError
    rng = np.random.default_rng(10700)
    n, W = 40, 300
    m01 = hc.founder_matrix(rng, n, W, p_flip=2e-3)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    cases = [([(10, 100)], {"mask_p": np.zeros(n, np.uint8)}), ([(10, 100)], {"min_mac": 0}), ([(10, 100)], {"max_sites": 3}),
             ([(10, 100)], {"max_sites": 1025}), ([(100, 10)], {}), ([(10, W + 1)], {})]
    for wins, kw in cases:
        with pytest.raises(ImpopError) as ei:
            bm.ld_scan(wins, **kw)
        assert ei.value.code == E_INVALID, (wins, kw)
    assert len(bm.ld_scan([(10, 100)], max_sites=4)) == 1 and len(bm.ld_scan([(10, 100)], max_sites=1024)) == 1
    rec, sites = bm.ld_scan([(10, 100)], max_sites=0, want_sites=True)  # 0 = 512
    assert sites.shape == (1, 512)
    lc.assert_matches((rec, sites), lc.reference(m01, None, [(10, 100)], 1, 512), "0 = 512")
    empty = bm.ld_scan([])
    assert empty.dtype == impop_amd.LD_DTYPE and len(empty) == 0
    rec, sites = bm.ld_scan([], want_sites=True)
    assert len(rec) == 0 and sites.shape == (0, 512)
    bm.free()


def test_timers_bracket_the_three_kernel_groups(ctx):
    rng = np.random.default_rng(10800)
    m01 = lc.planted_matrix(rng, 64)
    bm = ctx.upload_dense(m01, keep_hap_major=False)
    ctx.gram_timing(True)
    bm.ld_scan(lc.window_list(), max_chunk_bytes=1)
    ms, chunks = ctx.ld_elapsed()
    ctx.gram_timing(False)
    assert chunks == len(lc.window_list()) and len(ms) == 3 and all(t > 0.0 for t in ms)
    bm.free()


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def test_cli_rows_are_the_records(ctx, tmp_path):
    from impop_amd.matrixio import MatrixFile, save_matrix
    from impop_amd import pack_hap_major
    rng = np.random.default_rng(10900)
    n, W, origin = 40, 900, 5000
    m01 = hc.founder_matrix(rng, n, W, nf=5, p_site=0.2, p_flip=0.002)
    names = [f"S{i:02d}#1#chrT:0-1" for i in range(n)]
    mpath, bed, sub = str(tmp_path / "m.npz"), str(tmp_path / "w.bed"), str(tmp_path / "u.txt")
    save_matrix(mpath, MatrixFile(bits=pack_hap_major(m01), n_site=W, names=names, origin=origin, contig="chrT"))
    rows = [(0, 130), (100, 300), (250, 251), (300, 900), (837, 900), (0, 900)]
    open(bed, "w").write("".join(f"chrT\t{origin + b}\t{origin + e}\n" for b, e in rows))
    keep = sorted(rng.choice(n, 31, replace=False).tolist())
    open(sub, "w").write("".join(names[i].partition("chrT")[0] + "\n" for i in keep))
    flags = np.zeros(n, np.uint8)
    flags[keep] = 1

    def table(ref, members):
        rec, used = ref
        out = ["REGION\tLENGTH\tSAMPLES\tSITES\tQUALIFYING\tUSED\tZNS\tMEAN_DPRIME\tPERFECT\tCOMPLETE\tOMEGA_MAX\tOMEGA_POS"]
        for i, (b, e) in enumerate(rows):
            split = int(rec["omega_split"][i])
            out.append("\t".join([f"CHM13#0#chrT:{origin + b}-{origin + e}", str(e - b), str(members), str(e - b), str(int(rec["n_qualifying"][i])),
                                  str(int(rec["n_used"][i])), "%.8f" % rec["zns"][i], "%.8f" % rec["mean_dprime"][i], str(int(rec["n_perfect"][i])),
                                  str(int(rec["n_complete"][i])), "%.8f" % rec["omega_max"][i],
                                  str(origin + int(used[i, split])) if split else "NA"]))
        return "\n".join(out) + "\n"

    def run(extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", mpath, "--bed", bed, "--format", "ld"]
                           + extra, capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        return r.stdout

    mac = lambda f, k: max(1, int(np.ceil(f * k)))  # noqa: E731
    want = table(lc.reference(m01, None, rows, mac(0.05, n), 512), n)
    assert "NA" in want and any(ln.split("\t")[-1] not in ("NA", "OMEGA_POS") for ln in want.splitlines())
    assert run([]) == want and run(["--compact"]) == want
    assert run(["-u", sub, "--ld-min-maf", "0.1", "--ld-max-sites", "16"]) == table(lc.reference(m01, flags, rows, mac(0.1, 31), 16), 31)
