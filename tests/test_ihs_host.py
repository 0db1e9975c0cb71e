"""No GPU: the host side of impop_ihs_scan — the known answer of the header from the plain restatement, the weighted restatement
against the plain one, ihs_values and standardize against numpy, the ABI declaration and its binding, and what
scripts/impop_scan.py refuses and writes for --format ihs / xpehh (hand-made records: no device is opened)."""
import ctypes as C
import importlib.util
import io
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ihs_cases as ic
import plain_ihs as pi
from conftest import ROOT

SCAN = os.path.join(ROOT, "scripts", "impop_scan.py")
CORE_FIELDS = ["site", "n", "c1", "flags", "reserved", "ihh2", "sl2"]
PARAM_FIELDS = ["struct_size", "min_mac", "cutoff_milli", "reserved", "max_extend_bp", "max_extend_sites"]


def load_cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("impop_scan_cli_ihs", SCAN)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    return mod


# ---- the definitions ------------------------------------------------------------------------------------------------------------------

def test_known_answer_of_the_header():
    m01 = ic.known_matrix()
    rec = pi.reference(m01, 0, 7, 0, 7, [None], **ic.KNOWN_PARAMS)
    assert rec["site"].tolist() == ic.KNOWN_SITES and rec["flags"].tolist() == ic.KNOWN_FLAGS
    assert [(tuple(r["n"]), tuple(r["c1"])) for r in rec] == ic.KNOWN_HEAD
    assert rec["ihh2"].tolist() == ic.KNOWN_I2 == rec["sl2"].tolist()
    lim = pi.reference(m01, 0, 7, 0, 7, [None], **ic.KNOWN_PARAMS, **ic.KNOWN_LIMITS)
    assert lim["flags"].tolist() == ic.KNOWN_LIMIT_FLAGS and lim["ihh2"].tolist() == ic.KNOWN_LIMIT_IHH2 and lim["sl2"].tolist() == ic.KNOWN_LIMIT_SL2
    # one value by hand: core 1, class 0 = h0, h1, h2, towards higher sites: all three pairs agree at sites 1..4, one at site 5;
    # 1000 * 1 >= 300 * 3, so the integral runs to the edge: 3 * (3 + 3) + (3 + 1) = 22, EDGE
    assert rec["ihh2"][1][0][1] == 22 and rec["flags"][1] & pi.flag_bit(False, 0, 0, 1)
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    body = header[header.index("#define IMPOP_IHS_SCAN_MAX_N"):header.index("typedef struct impop_ihs_params")]
    flat = re.sub(r"\s+", "", body.replace("*", ""))
    for row in ic.KNOWN_ROWS:  # the case is stated in the header
        assert row in body
    for site, fl, i2 in zip(ic.KNOWN_SITES, ic.KNOWN_FLAGS, ic.KNOWN_I2):
        assert f"{site}:(3,3)(0,3){fl}{i2}".replace(" ", "") in flat, site
    for vals in (ic.KNOWN_LIMIT_FLAGS, ic.KNOWN_LIMIT_IHH2, ic.KNOWN_LIMIT_SL2):
        assert ",".join(str(x) for x in vals).replace(" ", "") in flat


@pytest.mark.parametrize("seed", range(4))
def test_weighted_restatement_equals_the_plain_one(seed):
    rng = np.random.default_rng(21110 + seed)
    r, S = int(rng.integers(4, 8)), int(rng.integers(30, 70))
    distinct = ic.mosaic(rng, r, S, nf=3, p_mut=0.05)
    which = rng.integers(0, r, size=int(rng.integers(8, 41)))
    m01 = distinct[which]
    n = len(which)
    kw = dict(min_mac=1 + seed % 2, cutoff_milli=(50, 250, 0, 1000)[seed], max_bp=(0, 9, 30, 0)[seed], max_sites=(0, 4, 0, 3)[seed])
    plain = pi.reference(m01, 1, S - 1, 2, S - 2, [None], **kw)
    mult = np.bincount(which, minlength=r)
    pi.assert_same(pi.records(pi.weighted_survivors(distinct, [mult], 1, S - 1), 2, S - 2, **kw), plain, "K1")
    a = rng.random(n) < 0.5
    a[:2], a[2:4] = True, False
    plain2 = pi.reference(m01, 1, S - 1, 2, S - 2, [a, ~a], **kw)
    mults = [np.bincount(which[a], minlength=r), np.bincount(which[~a], minlength=r)]
    pi.assert_same(pi.records(pi.weighted_survivors(distinct, mults, 1, S - 1), 2, S - 2, **kw), plain2, "K2")
    assert len(plain) and len(plain2)


def test_cases_exercise_the_cutoff_the_edge_and_the_limits():
    for n in ic.GEO_N[1:]:
        for K in (1, 2):
            ic.assert_coverage(n, K)
    assert {p[0] for p in ic.GEO_PARAMS} == {1, 2, 5} and {p[1] for p in ic.GEO_PARAMS} == {0, 50, 250, 1000}
    assert {p[2] for p in ic.GEO_PARAMS} == {(0, 0), (37, 5), (1000, 0)} and set(ic.GEO_CHUNKS) == {1, 2, 5, None}


# ---- the doubles and the standardisation ---------------------------------------------------------------------------------------------

def hand_records():
    from impop_amd.ihs import IHS_DTYPE
    rec = np.zeros(7, dtype=IHS_DTYPE)
    #            site  n        c1      flags   ihh2                      sl2
    rows = [(10, (5, 4), (0, 4), 0, ((30, 50), (12, 24)), ((10, 10), (6, 6))),
            (11, (6, 3), (0, 3), 0x01, ((60, 30), (6, 3)), ((20, 10), (3, 3))),       # EDGE, base pairs, class 0, half 0
            (12, (8, 1), (0, 1), 0, ((28, 28), (0, 0)), ((14, 14), (0, 0))),          # a class of one
            (13, (5, 4), (0, 4), 0x0100, ((40, 40), (0, 0)), ((10, 30), (12, 0))),    # LIMIT; iHH_1 = 0
            (14, (5, 4), (0, 4), 0x10, ((30, 10), (6, 6)), ((10, 10), (6, 12))),      # EDGE, sites
            (15, (5, 4), (0, 4), 0, ((30, 70), (12, 12)), ((10, 30), (6, 6))),
            (16, (4, 5), (0, 5), 0, ((30, 70), (12, 12)), ((10, 30), (6, 6)))]
    for i, (site, n, c1, fl, ihh2, sl2) in enumerate(rows):
        rec[i] = (site, n, c1, fl, 0, ihh2, sl2)
    return rec


def test_ihs_values_against_plain_arithmetic():
    from impop_amd.ihs import ihs_values
    rec = hand_records()
    for k, names in ((1, ("ihs", "nsl")), (2, ("xpehh", "xpnsl"))):
        v = ihs_values(rec, k)
        for i, r in enumerate(rec):
            for field, out, score in (("ihh2", "ihh", names[0]), ("sl2", "sl", names[1])):
                want = []
                for g in range(2):
                    ng = int(r["n"][g])
                    tot = int(r[field][g][0]) + int(r[field][g][1])
                    want.append(float("nan") if ng < 2 or tot == 0 else tot / (2.0 * (ng * (ng - 1) // 2)))
                for g in range(2):
                    assert (math.isnan(want[g]) and math.isnan(v[out][i, g])) or v[out][i, g] == want[g], (k, i, field, g)
                num, den = (want[1], want[0]) if k == 1 else (want[0], want[1])
                s = float("nan") if math.isnan(num) or math.isnan(den) else math.log(num / den)
                assert (math.isnan(s) and math.isnan(v[score][i])) or v[score][i] == s, (k, i, score)
            assert v["freq1"][i] == int(r["c1"].sum()) / int(r["n"].sum())
    v = ihs_values(rec, 1)
    assert v["ihh"][0].tolist() == [4.0, 3.0] and v["ihs"][0] == math.log(3.0 / 4.0)
    assert np.isnan(v["ihs"][2]) and np.isnan(v["ihs"][3]) and not np.isnan(v["nsl"][3])   # a class of one; a zero term
    with pytest.raises(ValueError):
        ihs_values(rec, 3)


def test_standardize_against_numpy():
    from impop_amd.ihs import standardize
    rng = np.random.default_rng(21200)
    n = 400
    score = rng.normal(size=n)
    score[rng.random(n) < 0.05] = np.nan
    freq = rng.random(n) * 0.999
    flags = np.where(rng.random(n) < 0.2, rng.integers(1, 1 << 16, size=n), 0).astype(np.uint32)
    for measure, edge in ((0, 0x000F), (1, 0x00F0)):
        got = standardize(score, flags, measure, freq, bins=20)
        for b in range(20):
            sel = (np.floor(freq * 20).astype(int) == b)
            use = sel & ((flags & edge) == 0) & ~np.isnan(score)
            if use.sum() < 2:
                assert np.isnan(got[sel]).all()
                continue
            want = (score[sel] - score[use].mean()) / score[use].std(ddof=1)
            assert np.allclose(got[sel], want, rtol=1e-12, atol=0, equal_nan=True)
        allc = standardize(score, flags, measure)  # the XP scores: every core at once
        use = ((flags & edge) == 0) & ~np.isnan(score)
        assert np.allclose(allc, (score - score[use].mean()) / score[use].std(ddof=1), rtol=1e-12, atol=0, equal_nan=True)
    # the two-core bin: a mean and a sample standard deviation exist, so both cores get +-1/sqrt(2); one core alone gives NaN; a core
    # with an EDGE bit takes no part in the mean but is scored
    s = np.array([1.0, 3.0, 5.0, 9.0, 2.0])
    f = np.array([0.11, 0.12, 0.55, 0.13, 0.95])
    fl = np.array([0, 0, 0, 0x01, 0], dtype=np.uint32)
    got = standardize(s, fl, 0, f, bins=10)
    assert np.allclose(got[:2], [-1 / math.sqrt(2), 1 / math.sqrt(2)]) and np.isnan(got[2]) and np.isnan(got[4])
    assert math.isclose(got[3], (9.0 - 2.0) / math.sqrt(2.0))
    assert np.isnan(standardize(s, fl, 1, f, bins=10)[2]) and not np.isnan(standardize(s, fl, 1, f, bins=10)[3])
    assert np.isnan(standardize(s[:1], fl[:1], 0)).all()
    with pytest.raises(ValueError):
        standardize(s, fl, 0, f, bins=0)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------

def test_abi_declares_ihs_scan():
    import impop_amd
    from impop_amd import _lib, ihs
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    assert re.search(r"#define IMPOP_IHS_SCAN_MAX_N\s+4096u\b", header) and _lib.IHS_SCAN_MAX_N == 4096 == ihs.IHS_SCAN_MAX_N
    assert re.search(r"#define IMPOP_IHS_EDGE_BITS\s+0x00FFu", header) and re.search(r"#define IMPOP_IHS_LIMIT_BITS\s+0xFF00u", header)
    assert (ihs.EDGE_BITS, ihs.LIMIT_BITS) == (pi.EDGE_BITS, pi.LIMIT_BITS) == (0x00FF, 0xFF00)
    for fn, n_args in (("impop_ihs_scan", 12), ("impop_ctx_ihs_elapsed", 3)):
        assert re.search(r"^int %s\(" % fn, header, re.M) and len(_lib.SIGNATURES[fn][1]) == n_args
    assert C.sizeof(_lib.IhsCore) == 96 == impop_amd.IHS_DTYPE.itemsize and impop_amd.IHS_DTYPE == pi.IHS_DTYPE == ihs.IHS_DTYPE
    assert [n for n, _ in _lib.IhsCore._fields_] == CORE_FIELDS == list(impop_amd.IHS_DTYPE.names)
    for name, _ in _lib.IhsCore._fields_:  # same offsets on both sides
        assert getattr(_lib.IhsCore, name).offset == impop_amd.IHS_DTYPE.fields[name][1]
    assert _lib.IhsCore.ihh2.offset == 32 and _lib.IhsCore.sl2.offset == 64
    assert C.sizeof(_lib.IhsParams) == 32 and [n for n, _ in _lib.IhsParams._fields_] == PARAM_FIELDS
    assert re.search(r"typedef struct impop_ihs_core \{\s*/\* 96 bytes", header) and re.search(r"typedef struct impop_ihs_params \{\s*/\* 32 bytes", header)
    for struct, want in (("impop_ihs_core", CORE_FIELDS), ("impop_ihs_params", PARAM_FIELDS)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [re.sub(r"\[.*", "", n.strip()) for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert declared == want
    assert hasattr(impop_amd.BitMatrix, "ihs_scan") and hasattr(impop_amd.Context, "ihs_elapsed")
    if os.path.exists(_lib.SO_PATH):
        lib = C.CDLL(_lib.SO_PATH)
        assert hasattr(lib, "impop_ihs_scan") and hasattr(lib, "impop_ctx_ihs_elapsed")


# ---- the driver -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt,extra,env,needle", [
    ("ihs", ["--devices", "2"], {}, "not with --devices N"),
    ("ihs", ["-A", "a.txt", "-B", "b.txt"], {}, "not with -A / -B / --panel / -l"),
    ("ihs", ["--panel", "a.txt", "b.txt"], {}, "not with -A / -B / --panel / -l"),
    ("ihs", [], {"WORLD_SIZE": "2", "RANK": "0"}, "not under torch.distributed.run"),
    ("ihs", ["-t", "0.9"], {}, "it has no -t / -r"),
    ("ihs", ["--ihs-min-maf", "0.6"], {}, "--ihs-min-maf takes a frequency above 0, at most 0.5"),
    ("ihs", ["--ihs-min-maf", "0"], {}, "--ihs-min-maf takes a frequency above 0, at most 0.5"),
    ("ihs", ["--ihs-cutoff", "1.5"], {}, "--ihs-cutoff takes 0 to 1"),
    ("ihs", ["--ihs-max-extend", "-1"], {}, "take 0 (no limit) or more"),
    ("ihs", ["--ihs-max-extend-sites", "-1"], {}, "take 0 (no limit) or more"),
    ("ihs", ["--ihs-bins", "0"], {}, "--ihs-bins takes 1 or more"),
    ("xpehh", [], {}, "--format xpehh takes --panel a.txt b.txt: two population lists"),
    ("xpehh", ["--panel", "a.txt"], {}, "two population lists"),
    ("xpehh", ["--panel", "a.txt", "b.txt", "c.txt"], {}, "two population lists"),
    ("xpehh", ["--panel", "a.txt", "b.txt", "-u", "s.txt"], {}, "not with -A / -B / -l / -u"),
    ("xpehh", ["--panel", "a.txt", "b.txt", "--devices", "2"], {}, "not with --devices N"),
])
def test_driver_refuses_next_to_ihs(fmt, extra, env, needle):
    r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", fmt, "--backend", "gloo"] + extra,
                       capture_output=True, text=True, env=dict(os.environ, **env), timeout=120)
    assert r.returncode == 2 and needle in r.stderr, (r.returncode, r.stderr[-500:])
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("Error: "), r.stderr[-500:]


def test_driver_refuses_sim_list_and_stray_options():
    r = subprocess.run([sys.executable, SCAN, "--sim-list", "none.tsv", "--format", "ihs"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stderr.strip() == "Error: --format ihs scans a presence matrix (--matrix / --bed): not with --sim-list"
    for stray in (["--ihs-min-maf", "0.1"], ["--ihs-cutoff", "0.1"], ["--ihs-max-extend", "5"], ["--ihs-max-extend-sites", "5"], ["--ihs-bins", "5"],
                  ["--ihs-keep-edge"]):
        r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "ld"] + stray,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and r.stderr.strip().endswith("belong to --format ihs and --format xpehh"), r.stderr


def test_table_writer_on_hand_made_records():
    from impop_amd.ihs import ihs_values, standardize
    cli = load_cli()
    rec = hand_records()
    chroms, bps = ["c"] * len(rec), [1000 + 2 * int(s) for s in rec["site"]]
    out = io.StringIO()
    cli.write_ihs_table(out, 1, chroms, bps, rec, 1, False)
    lines = out.getvalue().splitlines()
    assert lines[0] == "CHROM\tSITE\tN0\tN1\tFREQ1\tIHH0\tIHH1\tIHS\tIHS_STD\tSL0\tSL1\tNSL\tNSL_STD\tFLAGS" == cli.IHS_HEADER
    assert [ln.split("\t")[1] for ln in lines[1:]] == ["1020", "1024", "1026", "1030", "1032"]  # the two cores with an EDGE bit are left out
    v = ihs_values(rec, 1)
    z = standardize(v["ihs"], rec["flags"], 0, v["freq1"], 1)
    assert lines[1] == (f"c\t1020\t5\t4\t{4 / 9:.8f}\t4.00000000\t3.00000000\t{math.log(0.75):.8f}\t{z[0]:.8f}\t1.00000000\t1.00000000\t0.00000000\t"
                        f"{standardize(v['nsl'], rec['flags'], 1, v['freq1'], 1)[0]:.8f}\t0")
    assert lines[2].split("\t")[6:9] == ["NA", "NA", "NA"] and lines[3].split("\t")[-1] == "256"
    out = io.StringIO()
    cli.write_ihs_table(out, 1, chroms, bps, rec, 1, True)
    assert len(out.getvalue().splitlines()) == 1 + len(rec)
    out = io.StringIO()
    cli.write_ihs_table(out, 2, chroms, bps, rec, 50, False)
    lines = out.getvalue().splitlines()
    assert lines[0] == "CHROM\tSITE\tNA\tNB\tFREQ1_A\tFREQ1_B\tIHH_A\tIHH_B\tXPEHH\tXPEHH_STD\tSL_A\tSL_B\tXPNSL\tXPNSL_STD\tFLAGS" == cli.XPEHH_HEADER
    assert lines[1].split("\t")[:9] == ["c", "1020", "5", "4", "0.00000000", "1.00000000", "4.00000000", "3.00000000", f"{math.log(4 / 3):.8f}"]
    out = io.StringIO()
    cli.write_ihs_table(out, 1, [], [], rec[:0], 50, False)
    assert out.getvalue() == cli.IHS_HEADER + "\n"
