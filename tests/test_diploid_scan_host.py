"""No GPU: the host side of impop_diploid_scan — the known answer of the header against the plain restatement, the ABI declaration
and its binding, the record layouts on both sides, pair_haplotypes on PanSN names, and what scripts/impop_scan.py refuses and
prints for --format diploid (a recording stand-in for the Runner: no device is opened)."""
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

import dip_cases as dc
import plain_diploid as pd
from conftest import ROOT

SCAN = os.path.join(ROOT, "scripts", "impop_scan.py")
STATS_FIELDS = ["n_ind", "n_sites", "s_p", "het_sites", "het_total", "sum_p", "roh_sites_total", "roh_runs_total", "longest_run",
                "ho", "he", "f_is", "f_roh"]
IND_FIELDS = ["het", "hom_alt", "longest_run", "roh_runs", "roh_sites", "reserved"]


def load_cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("impop_scan_cli_diploid", SCAN)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    return mod


# ---- the definitions ------------------------------------------------------------------------------------------------------------------

def test_known_answer_of_the_header():
    rec, ind = pd.reference(dc.known_matrix(), dc.KNOWN_PAIRS, [(0, 6, 0)], 3)
    assert [tuple(int(x) for x in r) for r in ind[0]] == [(1, 1, 5, 1, 5, 0), (2, 1, 3, 1, 3, 0)]
    r = rec[0]
    assert [int(r[f]) for f in STATS_FIELDS[:9]] == [2, 6, 4, 3, 3, 13, 8, 2, 5]
    assert r["ho"] == 0.25 and r["he"] == 26.0 / 72.0 and r["f_is"] == 1.0 - 9.0 / 13.0 and r["f_roh"] == 8.0 / 12.0
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    for row in dc.KNOWN_ROWS:  # the case is stated in the header
        assert row in header
    assert "ho 0.25, he 26/72, f_is 1 - 9/13, f_roh 8/12" in header


def test_runs_and_doubles_of_the_restatement():
    assert pd.runs_of([], 10, 20) == [10] and pd.runs_of([], 5, 5) == []
    assert pd.runs_of([10, 19], 10, 20) == [8] and pd.runs_of([12, 13, 17], 10, 20) == [2, 3, 2]
    ho, he, f_is, f_roh = pd.doubles(3, 0, 0, 0, 0, 0)
    assert all(np.isnan(x) for x in (ho, he, f_is, f_roh))
    ho, he, f_is, f_roh = pd.doubles(2, 6, 12, 3, 13, 8)  # seq_len takes the place of W in ho and he only
    assert ho == 3.0 / 24.0 and he == 26.0 / (12.0 * 12.0) and f_is == 1.0 - 9.0 / 13.0 and f_roh == 8.0 / 12.0
    # a window of one site; an individual without a heterozygous site has one run of W
    m = np.array([[1, 0, 1], [1, 1, 1]], dtype=np.uint8)
    rec, ind = pd.reference(m, [(0, 1)], [(1, 2), (0, 3), (0, 1)], 1)
    assert ind["het"].ravel().tolist() == [1, 1, 0] and ind["roh_runs"].ravel().tolist() == [0, 2, 1]
    assert ind["longest_run"].ravel().tolist() == [0, 1, 1] and ind["hom_alt"].ravel().tolist() == [0, 2, 1]
    assert np.isnan(rec["f_is"][2]) and rec["f_is"][0] == 1.0 - 1.0 / 1.0


def test_cases_are_not_trivial():
    for n in (2, 33, 465):
        for kind in ("spectrum", "founder"):
            case = dc.geometry_case(n, kind)
            assert len(case.pairs) >= 1 and len({h for p in case.pairs for h in p}) == 2 * len(case.pairs)
            mono = (case.m01.sum(axis=0) == 0) | (case.m01.sum(axis=0) == n)
            assert kind != "spectrum" or n == 2 or mono.sum() > 100  # a compacted matrix really is shorter
    assert (1, 69) in dc.geometry_case(70, "founder").pairs and any(a > b for a, b in dc.geometry_case(70, "founder").pairs)
    assert len(dc.geometry_case(465, "founder").pairs) < 232  # some haplotypes are in no pair
    with pytest.raises(AssertionError):
        dc.assert_nontrivial(np.zeros((1, 3), dtype=pd.IND_DTYPE))


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------

def test_abi_declares_diploid_scan():
    import impop_amd
    from impop_amd import _lib
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    assert re.search(r"#define IMPOP_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    assert re.search(r"#define IMPOP_DIPLOID_MAX_N\s+2048u\b", header) and _lib.DIPLOID_MAX_N == 2048
    for fn, n_args in (("impop_diploid_scan", 9), ("impop_ctx_diploid_elapsed", 3)):
        assert re.search(r"\bint %s\(" % fn, header) and len(_lib.SIGNATURES[fn][1]) == n_args
    assert re.search(r"typedef struct impop_diploid_stats \{\s*/\* 80 bytes", header)
    assert re.search(r"typedef struct impop_diploid_ind \{\s*/\* 24 bytes", header)
    assert C.sizeof(_lib.DiploidStats) == 80 and C.sizeof(_lib.DiploidInd) == 24 and C.sizeof(_lib.DiploidParams) == 16
    assert impop_amd.DIPLOID_DTYPE.itemsize == 80 and impop_amd.DIPLOID_IND_DTYPE.itemsize == 24
    assert pd.STATS_DTYPE == impop_amd.DIPLOID_DTYPE and pd.IND_DTYPE == impop_amd.DIPLOID_IND_DTYPE
    assert [n for n, _ in _lib.DiploidStats._fields_] == STATS_FIELDS == list(impop_amd.DIPLOID_DTYPE.names)
    assert [n for n, _ in _lib.DiploidInd._fields_] == IND_FIELDS == list(impop_amd.DIPLOID_IND_DTYPE.names)
    for struct, dtype in ((_lib.DiploidStats, impop_amd.DIPLOID_DTYPE), (_lib.DiploidInd, impop_amd.DIPLOID_IND_DTYPE)):
        for name, _ in struct._fields_:  # same offsets on both sides
            assert getattr(struct, name).offset == dtype.fields[name][1]
    assert _lib.DiploidStats.ho.offset == 48 and _lib.DiploidParams.max_chunk_bytes.offset == 8
    for struct, want in (("impop_diploid_stats", STATS_FIELDS), ("impop_diploid_ind", IND_FIELDS),
                         ("impop_diploid_params", ["struct_size", "min_run", "max_chunk_bytes"])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert declared == want
    assert hasattr(impop_amd.BitMatrix, "diploid_scan") and hasattr(impop_amd.Context, "diploid_elapsed")
    if os.path.exists(_lib.SO_PATH):
        lib = C.CDLL(_lib.SO_PATH)
        assert hasattr(lib, "impop_diploid_scan") and hasattr(lib, "impop_ctx_diploid_elapsed")
        assert lib.impop_version() == 4


# ---- pairing --------------------------------------------------------------------------------------------------------------------------

def test_pair_haplotypes():
    from impop_amd.popnames import pair_haplotypes
    names = ["HG01#2#chr1:100-200", "CHM13#0#chr1", "HG01#1#chr1:100-200", "HG02#1#chr1", "T3#1#a", "T3#2#a", "T3#3#a", "HG03#1#c:5-9",
             "HG03#2#c:5-9", "plain"]
    pairs, samples, unpaired = pair_haplotypes(names)
    assert pairs == [(2, 0), (7, 8)] and samples == ["HG01", "HG03"]  # (index of #1#, index of #2#), whatever their order in the matrix
    assert unpaired == ["CHM13#0#chr1", "HG02#1#chr1", "T3#1#a", "T3#2#a", "T3#3#a", "plain"]
    # a subset: only its names take part; half a person inside the subset is unpaired, names outside it are not mentioned
    pairs, samples, unpaired = pair_haplotypes(names, subset=["HG03#1#c:5-9", "HG03#2#c:5-9", "HG01#1#chr1:100-200", "nobody#1#x"])
    assert pairs == [(7, 8)] and samples == ["HG03"] and unpaired == ["HG01#1#chr1:100-200"]
    assert pair_haplotypes([]) == ([], [], [])
    assert pair_haplotypes(["A#1#x", "A#1#y"]) == ([], [], ["A#1#x", "A#1#y"])  # two sequences of one haplotype are no pair
    # a ':' inside the suffix does not reach the fields
    assert pair_haplotypes(["A#1#x:1-2#9", "A#2#x:1-2"])[0] == [(0, 1)]


# ---- the driver -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra,env,needle", [
    (["--devices", "2"], {}, "not with --devices N"),
    (["-A", "a.txt", "-B", "b.txt"], {}, "not with -A / -B / --panel / -l"),
    (["--panel", "a.txt", "b.txt"], {}, "not with -A / -B / --panel / -l"),
    (["-l", "s.txt"], {}, "not with -A / -B / --panel / -l"),
    ([], {"WORLD_SIZE": "2", "RANK": "0"}, "not under torch.distributed.run"),
    ([], {"WORLD_SIZE": "2", "RANK": "1"}, "not under torch.distributed.run"),
    (["-t", "0.9"], {}, "-t / -r / --identity belong to other formats"),
    (["--roh-min-sites", "0"], {}, "--roh-min-sites takes 1 or more"),
])
def test_driver_refuses_next_to_diploid(extra, env, needle):
    r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "diploid", "--backend", "gloo"] + extra,
                       capture_output=True, text=True, env=dict(os.environ, **env), timeout=120)
    assert r.returncode == 2 and needle in r.stderr, (r.returncode, r.stderr[-500:])
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("Error: "), r.stderr[-500:]


def test_driver_refuses_sim_list_and_stray_options():
    r = subprocess.run([sys.executable, SCAN, "--sim-list", "none.tsv", "--format", "diploid"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stderr.strip() == "Error: --format diploid scans a presence matrix (--matrix / --bed): not with --sim-list"
    for stray in (["--roh-min-sites", "64"], ["--ind-table", "x.tsv"]):
        r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "ld"] + stray,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and r.stderr.strip() == "Error: --roh-min-sites / --ind-table belong to --format diploid"


class _Recorder:
    """stands in for impop_scan.Runner: records the calls, returns records that name their source"""
    calls = []

    def __init__(self, args, mf, windows, need_pairs, rank, world, local_rank):
        self.n = len(windows)
        _Recorder.calls.append(("init", need_pairs, bool(args.compact)))

    def diploid(self, pairs, min_run, want_individuals):
        import impop_amd
        _Recorder.calls.append(("diploid", [tuple(p) for p in pairs], min_run, want_individuals))
        out = np.zeros(self.n, dtype=impop_amd.DIPLOID_DTYPE)
        out["n_ind"], out["n_sites"], out["het_sites"] = len(pairs), [300, 299], [41, 0]
        out["ho"], out["he"], out["f_is"] = [0.0123456789, 0.0], [0.02, 0.0], [0.382716057, float("nan")]
        out["roh_runs_total"], out["f_roh"], out["longest_run"] = [7, 3], [0.5, 1.0], [120, 299]
        if not want_individuals:
            return out
        ind = np.zeros((self.n, len(pairs)), dtype=impop_amd.DIPLOID_IND_DTYPE)
        ind["het"] = np.arange(self.n * len(pairs)).reshape(self.n, -1)
        ind["hom_alt"], ind["longest_run"], ind["roh_runs"], ind["roh_sites"] = 9, 120, 2, 200
        return out, ind

    def close(self):
        pass


def test_driver_prints_the_diploid_tables(tmp_path, capsys):
    from impop_amd import matrixio
    rng = np.random.default_rng(5)
    n, W = 12, 600
    m = (rng.random((n, W)) < 0.3).astype(np.uint8)
    names = [f"S{i // 2:03d}#{i % 2 + 1}#chr9:{1000}-{1000 + W}" for i in range(n - 1)] + ["CHM13#0#chr9"]  # S005 has one copy only
    matrixio.save_matrix(str(tmp_path / "m.npz"), matrixio.from_dense(m, names, origin=1000, contig="CHM13#0#chr9"))
    (tmp_path / "w.bed").write_text("chr9\t1000\t1300\nchr9\t1300\t1600\n")
    (tmp_path / "u.txt").write_text("S000#1\nS000#2\nS001\nS002#1\n")
    (tmp_path / "none.txt").write_text("S002#1\nCHM13#0\n")
    cli = load_cli()
    cli.Runner = _Recorder

    def run(extra):
        _Recorder.calls = []
        out, old = io.StringIO(), sys.argv
        sys.argv = [SCAN, "--matrix", str(tmp_path / "m.npz"), "--bed", str(tmp_path / "w.bed"), "--format", "diploid"] + extra
        try:
            with contextlib.redirect_stdout(out):
                cli.main()
        finally:
            sys.argv = old
        return out.getvalue().splitlines(), list(_Recorder.calls), capsys.readouterr().err

    lines, calls, err = run([])
    assert calls == [("init", False, False), ("diploid", [(0, 1), (2, 3), (4, 5), (6, 7), (8, 9)], 50, False)]  # no all-pairs operand
    assert lines == ["CHROM\tSTART\tEND\tN_IND\tSITES\tHET_SITES\tHO\tHE\tFIS\tROH_RUNS\tF_ROH\tLONGEST_RUN",
                     "CHM13#0#chr9\t1000\t1300\t5\t300\t41\t0.01234568\t0.02000000\t0.38271606\t7\t0.50000000\t120",
                     "CHM13#0#chr9\t1300\t1600\t5\t299\t0\t0.00000000\t0.00000000\tNA\t3\t1.00000000\t299"]
    warn = [ln for ln in err.splitlines() if ln.startswith("Warning")]  # the unpaired haplotypes, in ONE warning
    assert len(warn) == 1 and "S005#1#chr9:1000-1600" in warn[0] and "CHM13#0#chr9" in warn[0] and "2 sequences" in warn[0]
    ind_path = tmp_path / "ind.tsv"
    lines, calls, err = run(["-u", str(tmp_path / "u.txt"), "--compact", "--roh-min-sites", "7", "--ind-table", str(ind_path)])
    assert calls == [("init", False, True), ("diploid", [(0, 1), (2, 3)], 7, True)] and len(lines) == 3
    assert "S002#1#chr9:1000-1600" in err and "S005" not in err
    assert ind_path.read_text().splitlines() == [
        "CHROM\tSTART\tEND\tSAMPLE\tHET\tHOM_ALT\tLONGEST_RUN\tROH_RUNS\tROH_SITES",
        "CHM13#0#chr9\t1000\t1300\tS000\t0\t9\t120\t2\t200", "CHM13#0#chr9\t1000\t1300\tS001\t1\t9\t120\t2\t200",
        "CHM13#0#chr9\t1300\t1600\tS000\t2\t9\t120\t2\t200", "CHM13#0#chr9\t1300\t1600\tS001\t3\t9\t120\t2\t200"]
    # fewer than one pair: an error exit
    with pytest.raises(SystemExit) as ei:
        run(["-u", str(tmp_path / "none.txt")])
    assert ei.value.code == 2 and "no sample with both of its haplotypes" in capsys.readouterr().err
