"""No GPU: the host side of impop_ld_scan — the ABI declaration and its binding, the record layout on both sides, the plain
restatement of tests/ld_cases.py against independent formulas (np.corrcoef, block sums of the r2 matrix, the textbook omega), the
thinning ranks, and what scripts/impop_scan.py refuses and prints for --format ld (a recording stand-in for the Runner: no device
is opened)."""
import contextlib
import ctypes as C
import importlib.util
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ld_cases as lc
from conftest import ROOT

SCAN = os.path.join(ROOT, "scripts", "impop_scan.py")
FIELDS = ["n_members", "n_sites", "n_qualifying", "n_used", "n_perfect", "n_complete", "omega_split", "reserved",
          "sum_r2", "sum_dprime", "zns", "mean_dprime", "omega_max"]


def load_cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("impop_scan_cli_ld", SCAN)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    return mod


def test_abi_declares_ld_scan():
    import impop_amd
    from impop_amd import _lib
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    assert re.search(r"#define IMPOP_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    assert re.search(r"#define IMPOP_LD_MAX_N\s+4096u\b", header) and _lib.LD_MAX_N == 4096
    assert re.search(r"#define IMPOP_LD_MAX_SITES\s+1024u\b", header) and _lib.LD_MAX_SITES == 1024
    for fn, n_args in (("impop_ld_scan", 8), ("impop_ctx_ld_elapsed", 3)):
        assert re.search(r"\bint %s\(" % fn, header) and len(_lib.SIGNATURES[fn][1]) == n_args
    assert C.sizeof(_lib.LdStats) == 72 and C.sizeof(_lib.LdParams) == 24 and impop_amd.LD_DTYPE.itemsize == 72
    assert [n for n, _ in _lib.LdStats._fields_] == FIELDS == list(impop_amd.LD_DTYPE.names)
    for name, _ in _lib.LdStats._fields_:  # same offsets on both sides
        assert getattr(_lib.LdStats, name).offset == impop_amd.LD_DTYPE.fields[name][1]
    assert _lib.LdStats.sum_r2.offset == 32 and _lib.LdParams.max_chunk_bytes.offset == 16
    for struct, want in (("impop_ld_stats", FIELDS), ("impop_ld_params", ["struct_size", "min_mac", "max_sites", "reserved", "max_chunk_bytes"])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert declared == want
    assert [n for n, _ in _lib.LdParams._fields_] == ["struct_size", "min_mac", "max_sites", "reserved", "max_chunk_bytes"]
    assert hasattr(impop_amd.BitMatrix, "ld_scan") and hasattr(impop_amd.Context, "ld_elapsed")
    if os.path.exists(_lib.SO_PATH):
        lib = C.CDLL(_lib.SO_PATH)
        assert hasattr(lib, "impop_ld_scan") and hasattr(lib, "impop_ctx_ld_elapsed")
        assert lib.impop_version() == 4


# ---- the restatement against independent formulas ------------------------------------------------------------------------------------

def _small(seed, n, S):
    rng = np.random.default_rng(seed)
    return lc.planted_matrix(rng, n, S, nf=6, p_site=0.4, p_flip=5e-3)


def _tables(m01, flags, sites):
    P = lc.members(m01, flags)
    return lc.pair_tables(m01[P][:, sites].T, len(P)), m01[P][:, sites].T


@pytest.mark.parametrize("seed,n,flagged", [(1, 12, False), (2, 33, True), (3, 70, False)])
def test_pair_arithmetic(seed, n, flagged):
    m01 = _small(seed, n, 1200)
    flags = None
    if flagged:
        flags = (np.random.default_rng(seed).random(n) < 0.7).astype(np.uint8)
        flags[:4] = 1
    sites = [int(s) for s in lc.qualifying(m01, flags, 1)[:40]]
    (num, den, dmax, r2, dprime), rows = _tables(m01, flags, sites)
    nP = rows.shape[1]
    # the array form against Python integers and floats, bit for bit
    for i in range(len(sites)):
        for j in range(len(sites)):
            s_num, s_den, s_r2, s_dmax, s_dp = lc.pair_scalar(rows[i], rows[j], nP)
            assert (s_num, s_den) == (int(num[i, j]), int(den[i, j]))
            assert lc.bits(s_r2) == lc.bits(r2[i, j]) and lc.bits(s_dp) == lc.bits(dprime[i, j])
            assert s_dmax is None or s_dmax == int(dmax[i, j])
    # r2 is the squared correlation of the two columns (1e-9 relative)
    want = np.corrcoef(rows.astype(np.float64)) ** 2
    assert np.allclose(r2, want, rtol=1e-9, atol=1e-12)
    assert ((dprime >= 0.0) & (dprime <= 1.0)).all() and np.array_equal(r2, r2.T) and np.array_equal(dprime, dprime.T)
    # flipping a site's alleles changes neither statistic
    flipped = rows.copy()
    flipped[::2] ^= 1
    _, _, _, r2f, dpf = lc.pair_tables(flipped, nP)
    assert np.array_equal(lc.bits(r2f), lc.bits(r2)) and np.array_equal(lc.bits(dpf), lc.bits(dprime))


def test_sums_prefix_suffix_and_omega():
    m01 = _small(5, 40, 1200)
    sites = [int(s) for s in lc.qualifying(m01, None, 2)[:30]]
    (num, den, dmax, r2, dprime), rows = _tables(m01, None, sites)
    m = len(sites)
    a, b, dp = lc.site_sums(r2, dprime)
    L, R = lc.prefix_suffix(a, b)
    up = np.triu(r2, 1)
    # the stated order, spelled out with Python floats
    for j in (0, 1, 7, m - 1):
        acc = 0.0
        for i in range(j):
            acc = acc + float(r2[i, j])
        assert lc.bits(acc) == lc.bits(a[j])
        acc = 0.0
        for k in range(j + 1, m):
            acc = acc + float(r2[j, k])
        assert lc.bits(acc) == lc.bits(b[j])
    best = (0.0, 0)
    for l in range(m + 1):
        left, right, cross = up[:l, :l].sum(), up[l:, l:].sum(), up[:l, l:].sum()
        assert abs(L[l] - left) <= 1e-9 * max(left, 1e-300) and abs(R[l] - right) <= 1e-9 * max(right, 1e-300)
        assert abs(((L[m] - L[l]) - R[l]) - cross) <= 1e-9 * max(cross, 1.0)
        if 2 <= l <= m - 2 and cross > 0:
            w = ((left + right) / (l * (l - 1) / 2 + (m - l) * (m - l - 1) / 2)) / (cross / (l * (m - l)))  # Kim & Nielsen 2004
            if w > best[0]:
                best = (w, l)
    om, split = lc.omega(L, R, m)
    assert split == best[1] and abs(om - best[0]) <= 1e-9 * best[0] and split >= 2
    # the record of the window that holds exactly these sites carries the same sums
    rec, used = lc.reference(m01, None, [(sites[0], sites[-1] + 1)], 2, 512)
    assert used[0, :m].tolist() == sites and rec["n_used"][0] == m and rec["omega_split"][0] == split
    assert lc.bits(rec["sum_r2"][0]) == lc.bits(L[m]) and lc.bits(rec["omega_max"][0]) == lc.bits(om)
    # fewer than 4 sites: no split
    assert lc.omega(*lc.prefix_suffix([0.0, 0.5, 1.0], [1.0, 0.5, 0.0]), 3) == (0.0, 0)


def test_reference_records_on_a_hand_case():
    #                 s0 s1 s2 s3 s4
    m01 = np.array([[1, 1, 0, 1, 0],
                    [1, 1, 0, 1, 0],
                    [1, 1, 0, 0, 0],
                    [0, 0, 1, 0, 0],
                    [0, 0, 1, 0, 1],
                    [0, 0, 1, 0, 0]], dtype=np.uint8)
    rec, used = lc.reference(m01, None, [(0, 5), (0, 4), (0, 0), (4, 5)], 1, 4)
    assert rec["n_qualifying"].tolist() == [5, 4, 0, 1] and rec["n_used"].tolist() == [4, 4, 0, 1]
    assert used.tolist() == [[0, 1, 2, 3], [0, 1, 2, 3], [0, 0, 0, 0], [4, 0, 0, 0]]  # ranks floor(k 5 / 4) = 0, 1, 2, 3
    # s0 = s1 = complement of s2: three perfect pairs; s3 is carried only by carriers of s0: complete, not perfect
    assert rec["n_perfect"].tolist() == [3, 3, 0, 0] and rec["n_complete"].tolist() == [6, 6, 0, 0]
    r2_03 = float((6 * 2 - 3 * 2) ** 2) / float(3 * 3 * 2 * 4)
    assert rec["sum_r2"][0] == ((1.0 + (1.0 + 1.0)) + ((r2_03 + r2_03) + r2_03)) and rec["zns"][0] == rec["sum_r2"][0] / 6.0
    assert rec["sum_dprime"][0] == 6.0 and rec["mean_dprime"][0] == 1.0
    # m = 4: the one split l = 2: within = r2(0,1) + r2(2,3), between = the other four
    assert rec["omega_split"].tolist() == [2, 2, 0, 0]
    assert abs(rec["omega_max"][0] - ((1.0 + r2_03) / 2.0) / ((2.0 + 2 * r2_03) / 4.0)) < 1e-15
    assert rec["zns"][2:].tolist() == [0.0, 0.0] and rec["omega_max"][2:].tolist() == [0.0, 0.0]
    rec, _ = lc.reference(m01, [1, 1, 1, 0, 1, 1], [(0, 5)], 2, 4, weights=[5, 1, 2, 3, 7])
    assert rec["n_members"].tolist() == [5] and rec["n_sites"].tolist() == [18] and rec["n_qualifying"].tolist() == [4]  # s4: one carrier


@pytest.mark.parametrize("max_sites", (4, 8, 64, 512, 1024))
def test_thinning_ranks(max_sites):
    for q in (0, 1, 3, max_sites - 1, max_sites, max_sites + 1, 2 * max_sites - 1, 2 * max_sites + 1, 7 * max_sites + 3, 2 ** 32 - 1):
        r = lc.thinning_ranks(q, max_sites)
        assert len(r) == min(q, max_sites)
        if r:
            assert r[0] == 0 and r[-1] < q and all(x < y for x, y in zip(r, r[1:]))
        if q <= max_sites:
            assert r == list(range(q))


def test_planted_columns_are_counted():
    for seed, n in ((1, 33), (2, 64), (3, 465)):
        lc.check_planted(lc.planted_matrix(np.random.default_rng(seed), n))


# ---- the driver ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra,env,needle", [
    (["--devices", "2"], {}, "not with --devices N"),
    (["-A", "a.txt", "-B", "b.txt"], {}, "not with -A / -B / --panel / -l"),
    (["--panel", "a.txt", "b.txt"], {}, "not with -A / -B / --panel / -l"),
    (["-l", "s.txt"], {}, "not with -A / -B / --panel / -l"),
    ([], {"WORLD_SIZE": "2", "RANK": "0"}, "not under torch.distributed.run"),
    ([], {"WORLD_SIZE": "2", "RANK": "1"}, "not under torch.distributed.run"),
    (["-t", "0.9"], {}, "-t / -r / --identity belong to other formats"),
    (["--ld-max-sites", "3"], {}, "--ld-max-sites takes 4 .. 1024"),
    (["--ld-min-maf", "0.7"], {}, "--ld-min-maf is a minor-allele frequency"),
])
def test_driver_refuses_next_to_ld(extra, env, needle):
    r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "ld", "--backend", "gloo"] + extra,
                       capture_output=True, text=True, env=dict(os.environ, **env), timeout=120)
    assert r.returncode == 2 and needle in r.stderr, (r.returncode, r.stderr[-500:])
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("Error: "), r.stderr[-500:]


def test_driver_refuses_sim_list_and_stray_options():
    r = subprocess.run([sys.executable, SCAN, "--sim-list", "none.tsv", "--format", "ld"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stderr.strip() == "Error: --format ld scans a presence matrix (--matrix / --bed): not with --sim-list"
    r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "hapstats", "--ld-max-sites", "64"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stderr.strip() == "Error: --ld-min-maf / --ld-max-sites belong to --format ld"


class _Recorder:
    """stands in for impop_scan.Runner: records the calls, returns records that name their source"""
    calls = []

    def __init__(self, args, mf, windows, need_pairs, rank, world, local_rank):
        self.n = len(windows)
        _Recorder.calls.append(("init", need_pairs, bool(args.compact)))

    def ld(self, mask_p, min_mac, max_sites):
        import impop_amd
        _Recorder.calls.append(("ld", None if mask_p is None else int(np.asarray(mask_p).sum()), min_mac, max_sites))
        out = np.zeros(self.n, dtype=impop_amd.LD_DTYPE)
        out["n_members"], out["n_sites"] = 12, [300, 299]
        out["n_qualifying"], out["n_used"] = [700, 3], [max_sites, 3]
        out["n_perfect"], out["n_complete"] = [2, 0], [41, 1]
        out["zns"], out["mean_dprime"], out["omega_max"], out["omega_split"] = [0.123456789, 0.5], [0.75, 1.0], [3.14159265358, 0.0], [2, 0]
        used = np.zeros((self.n, max_sites), dtype=np.uint64)
        used[0, :4] = [5, 17, 123, 200]
        return out, used

    def close(self):
        pass


def test_driver_prints_the_ld_table(tmp_path):
    from impop_amd import matrixio
    rng = np.random.default_rng(5)
    n, W = 12, 600
    m = (rng.random((n, W)) < 0.3).astype(np.uint8)
    names = [f"S{i // 2:03d}#{i % 2 + 1}#chr9:{1000}-{1000 + W}" for i in range(n)]
    matrixio.save_matrix(str(tmp_path / "m.npz"), matrixio.from_dense(m, names, origin=1000, contig="CHM13#0#chr9"))
    (tmp_path / "w.bed").write_text("chr9\t1000\t1300\nchr9\t1300\t1600\n")
    (tmp_path / "u.txt").write_text("S000#1\nS000#2\nS001#1\n")
    cli = load_cli()
    cli.Runner = _Recorder

    def run(extra):
        _Recorder.calls = []
        out, old = io.StringIO(), sys.argv
        sys.argv = [SCAN, "--matrix", str(tmp_path / "m.npz"), "--bed", str(tmp_path / "w.bed"), "--format", "ld"] + extra
        try:
            with contextlib.redirect_stdout(out):
                cli.main()
        finally:
            sys.argv = old
        return out.getvalue().splitlines(), list(_Recorder.calls)

    lines, calls = run([])
    assert calls == [("init", False, False), ("ld", None, 1, 512)]  # ceil(0.05 * 12) = 1; no all-pairs operand is asked for
    assert lines == ["REGION\tLENGTH\tSAMPLES\tSITES\tQUALIFYING\tUSED\tZNS\tMEAN_DPRIME\tPERFECT\tCOMPLETE\tOMEGA_MAX\tOMEGA_POS",
                     "CHM13#0#chr9:1000-1300\t300\t12\t300\t700\t512\t0.12345679\t0.75000000\t2\t41\t3.14159265\t1123",
                     "CHM13#0#chr9:1300-1600\t300\t12\t299\t3\t3\t0.50000000\t1.00000000\t0\t1\t0.00000000\tNA"]
    lines, calls = run(["-u", str(tmp_path / "u.txt"), "--compact", "--ld-min-maf", "0.4", "--ld-max-sites", "64"])
    assert calls == [("init", False, True), ("ld", 3, 2, 64)] and len(lines) == 3  # ceil(0.4 * 3) = 2
    assert cli.ld_min_mac(0.05, 465) == 24 and cli.ld_min_mac(0.0, 465) == 1 and cli.ld_min_mac(0.5, 33) == 17
