"""No GPU: the host side of impop_permtest_scan — impop_permtest_labels against the restatement's generator bit for bit, the known
answer of the header through the serial statement of csrc/perm_math.h and through the restatement, the comparison rules on the
degenerate cases, the ABI declarations and record layouts on both sides, the table writer and what scripts/impop_permtest.py refuses before it opens a file."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import plain_permtest as pt
from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
KNOWN_H = np.array([[0, 1, 3, 1], [1, 0, 2, 0], [3, 2, 0, 2], [1, 0, 2, 0]])
SIX = [0b0011, 0b0101, 0b1001, 0b0110, 0b1010, 0b1100]
SIX_WA_WB = [(1, 2), (3, 0), (1, 2), (2, 1), (0, 3), (2, 1)]


@pytest.mark.parametrize("m", [2, 11, 64, 65, 131, 1024])
def test_labels_equal_the_restated_generator(m):
    import impop_amd
    for m_a in sorted({1, m - 1, max(m // 2, 1)}):
        got = impop_amd.permtest_labels(99, 5, m, m_a, 12)
        assert got.shape == (12, (m + 63) // 64) and got.dtype == np.uint64
        assert (got == pt.words(pt.labels(99, 5, m, m_a, 12), m)).all(), (m, m_a)
        for z in pt.from_words(got):
            assert bin(z).count("1") == m_a and z >> m == 0
        assert (impop_amd.permtest_labels(99, 5, m, m_a, 5) == got[:5]).all()  # the prefix property
        if m > 2:
            assert not (impop_amd.permtest_labels(100, 5, m, m_a, 12) == got).all()
            assert not (impop_amd.permtest_labels(99, 6, m, m_a, 12) == got).all()


def test_labels_refuses_bad_shapes():
    import impop_amd
    for m, m_a, n in ((1, 1, 1), (4, 0, 1), (4, 4, 1), (1025, 3, 1), (8, 3, 16385)):
        with pytest.raises(impop_amd.ImpopError):
            impop_amd.permtest_labels(1, 0, m, m_a, n)


def test_labellings_are_uniform_enough():
    """every 2-subset of 4 positions turns up about equally often among 6000 labellings"""
    import impop_amd
    counts = np.bincount(impop_amd.permtest_labels(3, 0, 4, 2, 6000)[:, 0].astype(np.int64), minlength=16)
    assert sorted(np.flatnonzero(counts).tolist()) == sorted(SIX) and counts[SIX].min() > 900 and counts[SIX].max() < 1100


@pytest.fixture(scope="module")
def known_lines(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("perm_known") / "perm_math")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "impop_amd", "csrc"), "-x", "c++",
                        os.path.join(ROOT, "tests", "fuzz", "perm_math.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, "known"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return r.stdout.splitlines()


def test_known_answer_through_the_serial_statement(known_lines):
    assert known_lines[0] == "obs 1 2 %d 9" % pt.SCALE and known_lines[1] == "st 1/2 0/1 1/2 0/1"
    null = [tuple(int(x) for x in l.split()[1:]) for l in known_lines[2:8]]
    assert [n[:2] for n in null] == SIX_WA_WB and all(9 - a - b == 6 for a, b, _ in null)
    assert known_lines[8] == "ge 6 6 6 6" and known_lines[9] == "doubles 0 0 1.5 0.25"
    # ab(z) = 0 with x(z) > 0 is not counted; tot = 0 counts every labelling, in every test; 17 ties floor
    assert known_lines[10] == "degenerate 0 1 1 1 %d" % (pt.SCALE // 17)


def test_known_answer_and_degenerate_rules_through_the_restatement(known_lines):
    rec, null = pt.window(KNOWN_H, 4, [[0, 1], [2, 3]], lambda p, m, m_k: SIX)[0]
    assert (rec["wa"], rec["wb"], rec["ab"], rec["nn"], rec["snn"]) == (1, 2, 6, pt.SCALE, 0.25)
    assert [n[:2] for n in null] == SIX_WA_WB
    assert [tuple(int(x) for x in l.split()[1:]) for l in known_lines[2:8]] == null
    assert (rec["ge_fst"], rec["ge_phi"], rec["ge_dxy"], rec["ge_snn"]) == (6, 6, 6, 6) and rec["p_fst"] == 1.0
    assert (rec["fst"], rec["phi_st"], rec["dxy"]) == (0.0, 0.0, 1.5)
    o = dict(wa=1, wb=2, nn=0, tot=9)
    assert not pt.ge_fst(4, 5, o, 2, 2) and pt.ge_fst(4, 5, dict(wa=4, wb=5, nn=0, tot=9), 2, 2)
    zero = dict(wa=0, wb=0, nn=0, tot=0)
    assert pt.ge_fst(0, 0, zero, 2, 2) and pt.ge_phi(0, 0, zero, 2, 2) and pt.ge_dxy(0, 0, zero) and pt.ge_snn(0, zero)
    assert pt.SCALE == 720720 * 4096 and all(pt.SCALE % t == 0 for t in range(1, 17)) and pt.SCALE % 17
    # one-member panels: pi = 0.0, phi_st NaN at m = 2; Dxy = 0 gives fst 0.0
    f, phi, d = pt.doubles(dict(wa=0, wb=0, tot=5), 1, 1)
    assert (f, d) == (1.0, 5.0) and phi != phi
    assert pt.doubles(dict(wa=3, wb=3, tot=6), 3, 3)[0] == 0.0


def test_abi_declares_permtest_scan():
    import impop_amd
    from impop_amd import _lib
    assert re.search(r"#define IMPOP_PERMTEST_MAX_N\s+1024u", HEADER) and _lib.PERMTEST_MAX_N == 1024
    assert re.search(r"#define IMPOP_PERMTEST_MAX_PERM\s+16384u", HEADER) and _lib.PERMTEST_MAX_PERM == 16384
    assert str(_lib.PERMTEST_SCALE) in HEADER and _lib.PERMTEST_SCALE == pt.SCALE
    for fn, n_args in (("impop_permtest_scan", 9), ("impop_permtest_labels", 6), ("impop_ctx_permtest_elapsed", 3)):
        assert re.search(r"^int %s\(" % fn, HEADER, re.M) and len(_lib.SIGNATURES[fn][1]) == n_args, fn
        decl = re.search(r"^int %s\((.*?)\);" % fn, HEADER, re.M | re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == n_args, fn
    for struct, dtype, plain, cname, size in ((_lib.PermPair, impop_amd.PERM_PAIR_DTYPE, pt.PAIR_DTYPE, "impop_perm_pair", 128),
                                              (_lib.PermNull, impop_amd.PERM_NULL_DTYPE, pt.NULL_DTYPE, "impop_perm_null", 24)):
        assert C.sizeof(struct) == size == dtype.itemsize and dtype == plain
        assert [n for n, _ in struct._fields_] == list(dtype.names)
        for name, _ in struct._fields_:
            assert getattr(struct, name).offset == dtype.fields[name][1]
        assert re.search(r"typedef struct %s \{\s*/\* %d bytes" % (cname, size), HEADER)
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), HEADER, re.S).group(1), flags=re.S)
        declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert declared == list(dtype.names)
    assert C.sizeof(_lib.PermtestParams) == 16 and [n for n, _ in _lib.PermtestParams._fields_] == ["struct_size", "n_perm", "seed"]
    assert re.search(r"typedef struct impop_permtest_params \{\s*/\* 16 bytes", HEADER)
    assert hasattr(impop_amd.BitMatrix, "permtest_scan") and hasattr(impop_amd.Context, "permtest_elapsed")
    lib = _lib.load()
    assert all(hasattr(lib, f) for f in ("impop_permtest_scan", "impop_permtest_labels", "impop_ctx_permtest_elapsed"))
    doc = " ".join(HEADER[HEADER.index("#define IMPOP_PERMTEST_MAX_N"):HEADER.index("typedef struct impop_permtest_params")].replace("*", " ").split())
    for needle in ("[impop_permtest_scan] route=<dense|compact> pops= pairs= members= perms= planes= windows= chunks= launches= null=<off|on>",
                   "SHARE THEIR NULL DRAWS", "0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "Known answer"):
        assert needle in doc, needle


def test_table_writer_on_the_known_answer():
    from impop_amd import permtest as pm
    per = [pt.window(KNOWN_H, 4, [[0, 1], [2, 3]], lambda p, m, m_k: SIX)]
    pairs, null = pt.pack(per, 6)
    main, nul = pm.tables(["chr:0-4"], [4], ["A", "B"], pairs, null)
    assert main == [["chr:0-4", "4", "A", "B", "2", "2", "6", "0.0", "0.0", "0.375", "0.25", "6", "6", "6", "6", "1.0", "1.0", "1.0", "1.0"]]
    assert len(main[0]) == len(pm.MAIN_COLUMNS) and len(nul) == 6 and len(nul[0]) == len(pm.NULL_COLUMNS)
    assert nul[1] == ["chr:0-4", "A", "B", "1", "3", "0", "6", str(2 * pt.SCALE)]
    assert pm.tables(["chr:0-4"], [4], ["A", "B"], pairs)[1] == []
    pairs["phi_st"][0, 0] = np.nan
    assert pm.tables(["r"], [0], ["A", "B"], pairs)[0][0][8:10] == ["NA", "NA"]


@pytest.mark.parametrize("extra,env,needle", [
    (["--panel", "a.txt", "b.txt"], {"WORLD_SIZE": "2"}, "torch.distributed.run"),
    (["--panel", "a.txt"], {}, "2 to 8 population lists"),
    ([], {}, "2 to 8 population lists"),
    (["--panel"] + ["p.txt"] * 9, {}, "2 to 8 population lists"),
    (["--panel", "a.txt", "b.txt", "--perm-n", "0"], {}, "1..16384"),
    (["--panel", "a.txt", "b.txt", "--perm-n", "16385"], {}, "1..16384"),
    (["--panel", "a.txt", "b.txt", "--perm-seed", "-1"], {}, "--perm-seed"),
    (["--panel", "a.txt", "b.txt", "-t", "0.99"], {}, "unrecognized arguments"),
    (["--panel", "a.txt", "b.txt", "-r", "5"], {}, "unrecognized arguments"),
])
def test_cli_refusals_need_no_device(extra, env, needle):
    """scripts/impop_permtest.py: one line on stderr and exit code 2, before any file or device is opened; the driver has no
    identity threshold and no rounding, so -t / -r are no options of it"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_permtest.py"), "--matrix", "none.npz", "--bed", "none.bed"] + extra,
                       capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, **env), timeout=120)
    assert r.returncode == 2 and needle in r.stderr and r.stdout == "", (r.returncode, r.stderr)
