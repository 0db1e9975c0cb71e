"""No GPU: the host side of impop_pca_scan — the ABI declaration and its binding, the record layouts on both sides, the plain
restatement on the known answer of the header, impop_amd/pca.py's derived values and row formatting on hand-made records, and
what scripts/impop_pca.py refuses before it opens a file."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

import plain_pca as pl
from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
WINDOW_FIELDS = ["n_members", "n_sites", "rank", "iterations", "flags", "reserved", "sum_h", "lambda", "resid"]
KNOWN = np.array([[0, 0, 0, 0], [0, 0, 0, 1], [0, 1, 1, 1], [0, 0, 0, 1]], np.uint8)


def test_abi_declares_pca_scan():
    import impop_amd
    from impop_amd import _lib
    assert re.search(r"#define IMPOP_ABI_VERSION 4\b", HEADER) and _lib.ABI_VERSION == 4
    assert re.search(r"#define IMPOP_PCA_MAX_N\s+1024u\b", HEADER) and _lib.PCA_MAX_N == 1024
    assert re.search(r"#define IMPOP_PCA_MAX_K\s+8u\b", HEADER) and _lib.PCA_MAX_K == 8
    for fn, n_args in (("impop_pca_scan", 9), ("impop_ctx_pca_elapsed", 3)):
        assert re.search(r"^int %s\(" % fn, HEADER, re.M) and len(_lib.SIGNATURES[fn][1]) == n_args
        decl = re.search(r"^int %s\((.*?)\);" % fn, HEADER, re.M | re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == n_args
    assert C.sizeof(_lib.PcaParams) == 24 and C.sizeof(_lib.PcaWindow) == 160 == impop_amd.PCA_WINDOW_DTYPE.itemsize
    assert re.search(r"typedef struct impop_pca_params \{\s*/\* 24 bytes", HEADER)
    assert re.search(r"typedef struct impop_pca_window \{\s*/\* 160 bytes", HEADER)
    assert [n for n, _ in _lib.PcaWindow._fields_] == WINDOW_FIELDS == list(impop_amd.PCA_WINDOW_DTYPE.names)
    for name, _ in _lib.PcaWindow._fields_:  # same offsets on both sides
        assert getattr(_lib.PcaWindow, name).offset == impop_amd.PCA_WINDOW_DTYPE.fields[name][1]
    assert _lib.PcaWindow.sum_h.offset == 24 and getattr(_lib.PcaWindow, "lambda").offset == 32 and _lib.PcaWindow.resid.offset == 96
    assert [n for n, _ in _lib.PcaParams._fields_] == ["struct_size", "k", "tol", "max_iter", "reserved"]
    assert _lib.PcaParams.tol.offset == 8 and _lib.PcaParams.max_iter.offset == 16
    for struct, want in (("impop_pca_params", ["struct_size", "k", "tol", "max_iter", "reserved"]), ("impop_pca_window", WINDOW_FIELDS)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [re.sub(r"\[\d+\]", "", n).strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert declared == want
    assert hasattr(impop_amd.BitMatrix, "pca_scan") and hasattr(impop_amd.Context, "pca_elapsed")
    lib = _lib.load()
    assert hasattr(lib, "impop_pca_scan") and hasattr(lib, "impop_ctx_pca_elapsed")
    # what the header must state about the call
    doc = " ".join(HEADER[HEADER.index("#define IMPOP_PCA_MAX_N"):HEADER.index("typedef struct impop_pca_params")].replace("*", " ").split())
    for text in ("lambda_{k+9} <= 0.9 lambda_j", "2 m^2 B_ij = m (r_i + r_j) - m^2 H_ij - t", "lowest index on exact ties",
                 "[impop_pca_scan] route=<dense|compact> members= k= windows= chunks= launches= iterations_max= unconverged= dist=<off|on>",
                 "out_dist2 without out_vectors", "16384 windows", "r = (5, 3, 7, 3), t = 18, sum_h = 9, trace = 2.25"):
        assert text in doc, text


def test_known_answer_of_the_header():
    H = pl.distances(KNOWN, 0, 4)
    assert [int(H[i, j]) for i in range(4) for j in range(i + 1, 4)] == [1, 3, 1, 2, 0, 2]
    B2, r, t = pl.centred(H)
    assert r.tolist() == [5, 3, 7, 3] and t == 18
    assert B2.tolist() == [[22, -2, -18, -2], [-2, 6, -10, 6], [-18, -10, 38, -10], [-2, 6, -10, 6]]  # 32 B: 2 m^2 = 32
    assert (B2.sum(axis=1) == 0).all()  # B 1 = 0, exactly
    ref = pl.window(H, 4, 2)
    assert ref["sum_h"] == 9 and ref["trace"] == 2.25 and ref["rank"] == 2
    want = [(9 + math.sqrt(17)) / 8, (9 - math.sqrt(17)) / 8]
    assert all(abs(ref["lam"][j] - want[j]) <= 1e-15 * want[j] for j in range(2))
    assert np.abs(ref["lam"][2:]).max() <= 1e-15
    assert abs(ref["lam"][:2].sum() - ref["trace"]) <= 4e-16 * ref["trace"]
    v = ref["vec"][:, 0] * (1 if pl.sign_ok(ref["vec"][:, 0]) else -1)
    assert np.abs(v - np.array([-0.472668, -0.184524, 0.841716, -0.184524])).max() < 1e-6
    # and a brute-force check of the matrix itself: B = -1/2 J H J
    J = np.eye(4) - 0.25
    assert np.abs(-0.5 * J @ H @ J - B2 / 32.0).max() < 1e-15


def record(**kw):
    import impop_amd
    r = np.zeros(1, impop_amd.PCA_WINDOW_DTYPE)[0]
    r["lambda"][:] = np.nan
    r["resid"][:] = np.nan
    for k, v in kw.items():
        if k in ("lambda", "resid"):
            r[k][:len(v)] = v
        else:
            r[k] = v
    return r


def test_tables_from_hand_made_records():
    from impop_amd import pca
    assert pca.main_columns(2) == ["REGION", "LENGTH", "SAMPLES", "SITES", "RANK", "TOTAL_VAR", "LAMBDA1", "LAMBDA2", "PVE1", "PVE2",
                                   "ITERATIONS", "FLAGS"]
    assert pca.vector_columns(3) == ["REGION", "SEQUENCE", "PC1", "PC2", "PC3"]
    ok = record(n_members=4, n_sites=4, rank=2, iterations=3, sum_h=9, **{"lambda": [1.5, 0.75], "resid": [1e-12, 1e-12]})
    assert pca.total_var(ok) == 2.25 and pca.pve(ok, 0) == 1.5 * 4 / 9 and pca.flag_text(ok) == "ok"
    assert pca.main_row("chr:0-4", 4, ok, 2) == ["chr:0-4", "4", "4", "4", "2", "2.25", "1.5", "0.75", repr(1.5 * 4 / 9), repr(0.75 * 4 / 9),
                                                "3", "ok"]
    flat = record(n_members=3, n_sites=10, rank=0, iterations=0, sum_h=0, **{"lambda": [0.0, 0.0]})
    assert pca.flag_text(flat) == "rank0" and math.isnan(pca.pve(flat, 0))
    assert pca.main_row("r", 10, flat, 2) == ["r", "10", "3", "10", "0", "0.0", "0.0", "0.0", "NA", "NA", "0", "rank0"]
    slow = record(n_members=4, n_sites=4, rank=1, iterations=500, flags=1, sum_h=9, **{"lambda": [1.5, 0.0], "resid": [0.1]})
    assert pca.flag_text(slow) == "unconverged" and pca.main_row("r", 4, slow, 2)[-2:] == ["500", "unconverged"]
    vec = np.array([[[0.5, -0.5, 0.5, -0.5], [0.0, 0.0, 0.0, 0.0]]])
    main, rows = pca.tables(["r"], [4], ["a", "b", "c", "d"], np.array([slow]), vec, 2)
    assert main == [pca.main_row("r", 4, slow, 2)]
    assert rows == [["r", "a", "0.5", "NA"], ["r", "b", "-0.5", "NA"], ["r", "c", "0.5", "NA"], ["r", "d", "-0.5", "NA"]]
    assert pca.tables(["r"], [4], ["a"], np.array([ok]), None, 2)[1] is None


@pytest.fixture()
def cli(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "scripts"))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    import impop_pca
    return impop_pca


@pytest.mark.parametrize("extra,env,needle", [
    (["--pca-k", "0"], {}, "--pca-k"),
    (["--pca-k", "9"], {}, "--pca-k"),
    (["--pca-tol", "0"], {}, "--pca-tol"),
    (["--pca-tol", "0.1"], {}, "--pca-tol"),
    (["--pca-max-iter", "0"], {}, "--pca-max-iter"),
    (["--pca-max-iter", "100001"], {}, "--pca-max-iter"),
    (["--pca-dist", "d.npy", "--matrix", "a.npz", "b.npz"], {}, "single --matrix"),
    ([], {"WORLD_SIZE": "2"}, "one process"),
])
def test_cli_refusals_read_no_file(cli, monkeypatch, capsys, extra, env, needle):
    """one line on stderr and exit code 2, in process, before any file or device is opened (the named files do not exist)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(cli, "load_matrix", lambda *a: pytest.fail("a matrix was opened"))
    monkeypatch.setattr(cli, "read_bed", lambda *a: pytest.fail("the BED was opened"))
    with pytest.raises(SystemExit) as e:
        cli.main(["--matrix", "none.npz", "--bed", "none.bed"] + extra)
    err = capsys.readouterr()
    assert e.value.code == 2 and needle in err.err and err.out == "", err.err


def test_cli_refuses_a_distance_matrix_of_too_many_rows(cli, monkeypatch, capsys):
    """--pca-dist with more than 16384 usable BED rows: refused once the BED is read, before any matrix is loaded"""
    monkeypatch.setattr(cli, "read_bed", lambda *a: [("chr1", i, i + 1) for i in range(16385)])
    monkeypatch.setattr(cli, "load_matrix", lambda *a: pytest.fail("a matrix was opened"))
    with pytest.raises(SystemExit) as e:
        cli.main(["--matrix", "none.npz", "--bed", "none.bed", "--pca-dist", "d.npy"])
    assert e.value.code == 2 and "16385" in capsys.readouterr().err
