"""No GPU: the host side of impop_kinship_scan — the plain restatement against a brute-force loop over sites and pairs, the known
answer of the header through the restatement and through impop_amd/kinship.py, the planted features of the GPU tests' inputs, the
ABI declaration and its binding, the record layouts on both sides, and the CLI's tables on a stubbed result."""
import ctypes as C
import math
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import kinship_cases as kc
import plain_kinship as pk
from conftest import ROOT

HEADER = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
WINDOW_FIELDS = ["n_ind", "n_sites", "n_pairs", "het_het", "ibs0", "ibs2", "n_related", "n_undefined"]
KNOWN = np.array([[1, 0, 0, 0, 1, 0], [0, 0, 0, 0, 1, 0], [1, 1, 0, 0, 0, 0], [1, 0, 0, 0, 0, 1]], np.uint8)


@pytest.mark.parametrize("seed", range(10))
def test_restatement_equals_the_brute_force_loops(seed):
    rng = np.random.default_rng(seed)
    N, S = int(rng.integers(2, 7)), int(rng.integers(1, 50))
    m01 = rng.integers(0, 2, size=(2 * N + 1, S), dtype=np.uint8)
    if seed % 2:
        m01[1] = m01[0]
    pr = rng.permutation(2 * N + 1)[: 2 * N].reshape(N, 2)
    wins = [(0, S, 0), (S // 2, S, 0), (S // 3, S // 3, 0)]
    num, den = int(rng.integers(0, 11)), 10
    watch = [(N - 1, 0)]
    ww, wp, wt = pk.scan(m01, pr, wins, (num, den), watch)
    tot = {}
    for w, (b, e, _) in enumerate(wins):
        hh_sum = i0_sum = i2_sum = rel = und = 0
        for p, (i, j) in enumerate(pk.pair_order(N)):
            t = [0] * 9
            for s in range(b, e):
                t[3 * (int(m01[pr[i, 0], s]) + int(m01[pr[i, 1], s])) + int(m01[pr[j, 0], s]) + int(m01[pr[j, 1], s])] += 1
            a, c = t[3] + t[4] + t[5], t[1] + t[4] + t[7]
            hh, i0 = t[4], t[2] + t[6]
            hh_sum += hh; i0_sum += i0; i2_sum += t[0] + t[4] + t[8]
            m = min(a, c)
            und += m == 0
            rel += m > 0 and Fraction(2 * (hh - 2 * i0) + 2 * m - a - c, 4 * m) >= Fraction(num, den)
            tot[p] = [x + y for x, y in zip(tot.get(p, [0] * 9), t)]
            if (i, j) == (0, N - 1):
                assert tuple(int(x) for x in wt[w, 0]) == (hh, i0, c, a)  # the watched pair is (N - 1, 0): het_i is N - 1's
        assert tuple(int(x) for x in ww[w]) == (N, e - b, N * (N - 1) // 2, hh_sum, i0_sum, i2_sum, rel, und)
    assert [[int(x) for x in r] for r in wp["t"]] == [tot[p] for p in range(len(tot))]


def test_known_answer_of_the_header():
    from impop_amd import kinship as kin
    g = pk.genotypes(KNOWN, [(0, 1), (2, 3)])
    assert g.tolist() == [[1, 0, 0, 0, 2, 0], [2, 1, 0, 0, 0, 1]]
    ww, wp, wt = pk.scan(KNOWN, [(0, 1), (2, 3)], [(0, 6, 0)], (0, 1), [(0, 1)])
    t = [int(x) for x in wp["t"][0]]
    assert t == [2, 2, 0, 0, 0, 1, 1, 0, 0]  # t00 = 2, t01 = 2, t12 = 1, t20 = 1
    assert tuple(int(x) for x in ww[0]) == (2, 6, 1, 0, 1, 2, 0, 0) and tuple(int(x) for x in wt[0, 0]) == (0, 1, 1, 2)
    n, a, b, hh, i0, i1, i2 = kin.cells(t)
    assert (n, a, b, hh, i0, i1, i2) == (6, 1, 2, 0, 1, 3, 2)
    assert kin.king_within(a, b, hh, i0) == -2 / 3 and kin.king_robust(a, b, hh, i0) == -5 / 4
    assert kin.ibs_dist(i1, i2, n) == 3.5 / 6 and kin.ibs0_frac(i0, n) == 1 / 6
    body = HEADER[HEADER.index("#define IMPOP_KINSHIP_MAX_N"):HEADER.index("typedef struct impop_genotypes")]
    body = " ".join(body.replace("*", " ").split())
    for text in ("h0 = 100010, h1 = 000010, h2 = 110000, h3 = 100001", "g_0 = 1,0,0,0,2,0 and g_1 = 2,1,0,0,0,1",
                 "t00 = 2, t01 = 2, t12 = 1, t20 = 1", "het = (1, 2), het_het = 0, ibs0 = 1, ibs2 = 2", "= -2/3", "KING-robust = -5/4",
                 "overlapping windows count as often as they occur", "IMPOP_PAIRWISE_CHUNK",
                 "[impop_kinship_scan] route=<dense|compact> individuals= rows= windows= chunks= launches= watch= plane_bytes="):
        assert text in body, text


def test_derived_values():
    from impop_amd import kinship as kin
    nan = math.isnan
    assert nan(kin.king_within(0, 0, 0, 0)) and nan(kin.king_robust(0, 5, 0, 0)) and nan(kin.ibs_dist(0, 0, 0)) and nan(kin.ibs0_frac(0, 0))
    assert kin.king_robust(10, 10, 10, 0) == 0.5 and kin.king_within(10, 10, 10, 0) == 0.5
    assert [kin.degree(x) for x in (0.5, 0.355, 0.354, 0.25, 0.1, 0.05, 0.0442, 0.0, -1.0, math.nan)] == \
        ["duplicate/MZ", "duplicate/MZ", "1st", "1st", "2nd", "3rd", "unrelated", "unrelated", "unrelated", "NA"]
    assert kin.threshold_fraction(0.0884) == (884, 10000) and kin.threshold_fraction(0) == (0, 10000) and kin.threshold_fraction(1) == (10000, 10000)
    with pytest.raises(ValueError):
        kin.threshold_fraction(1.5)
    assert kin.pair_order(3) == [(0, 1), (0, 2), (1, 2)] and [kin.pair_index(4, i, j) for i, j in kin.pair_order(4)] == list(range(6))


@pytest.mark.parametrize("N", [2, 3, 17, 49])
def test_planted_inputs_show_their_features(N):
    from impop_amd import kinship as kin
    m01, pr = kc.matrix(N), kc.pairs(N)
    assert m01.shape == (2 * N + 1, kc.N_SEG * kc.SEG) and len(set(pr.ravel().tolist())) == 2 * N
    assert (pr[:, 0] > pr[:, 1]).any() and (np.abs(pr[:, 0].astype(int) - pr[:, 1].astype(int)) > 1).any()
    for shape, wins in kc.window_lists().items():
        assert sum(1 for w in wins if w[1] == w[0]) == 1 and sum(1 for w in wins if w[1] - w[0] == 1) == 1
        ww, wp, wt = pk.scan(m01, pr, wins, kc.KIN, kc.watch(N))
        _, a, b, hh, i0, _, _ = kin.cells(wp["t"][0])
        assert i0 == 0 and a == b == hh > 0 and kin.king_robust(a, b, hh, i0) == 0.5 and kin.degree(0.5) == "duplicate/MZ"
        if N >= 3:
            _, a, b, hh, i0, _, _ = kin.cells(wp["t"][1])
            assert i0 == 0 and hh > 0 and kin.king_robust(a, b, hh, i0) < 0.5
        if N >= 5:
            assert any(int(w["n_undefined"]) > 0 and int(w["n_sites"]) > 1 for w in ww)
            assert any(0 < int(w["n_related"]) < int(w["n_pairs"]) for w in ww)
    # the planes of the restatement's helper are what the device builds: XOR and AND
    pl = pk.planes(m01, pr)
    g = pk.genotypes(m01, pr)
    assert ((pl[:N] == 1) == (g == 1)).all() and ((pl[N:] == 1) == (g == 2)).all()


def test_abi_declares_kinship_scan():
    import impop_amd
    from impop_amd import _lib
    assert re.search(r"#define IMPOP_ABI_VERSION 4\b", HEADER) and _lib.ABI_VERSION == 4
    assert re.search(r"#define IMPOP_KINSHIP_MAX_N\s+2048u", HEADER) and _lib.KINSHIP_MAX_N == 2048
    assert re.search(r"#define IMPOP_KINSHIP_MAX_WATCH\s+1024u", HEADER) and _lib.KINSHIP_MAX_WATCH == 1024
    for fn, n_args in (("impop_genotypes_create", 5), ("impop_genotypes_info", 4), ("impop_genotypes_download", 6), ("impop_genotypes_free", 2),
                       ("impop_kinship_scan", 10), ("impop_ctx_kinship_elapsed", 3)):
        assert re.search(r"^int %s\(" % fn, HEADER, re.M) and len(_lib.SIGNATURES[fn][1]) == n_args, fn
        decl = re.search(r"^int %s\((.*?)\);" % fn, HEADER, re.M | re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", decl, flags=re.S).split(",")) == n_args, fn
    sides = ((_lib.KinWindow, impop_amd.KIN_WINDOW_DTYPE, pk.KIN_WINDOW_DTYPE, WINDOW_FIELDS, "impop_kin_window", 48),
             (_lib.KinPair, impop_amd.KIN_PAIR_DTYPE, pk.KIN_PAIR_DTYPE, ["t"], "impop_kin_pair", 72),
             (_lib.KinWatch, impop_amd.KIN_WATCH_DTYPE, pk.KIN_WATCH_DTYPE, ["het_het", "ibs0", "het_i", "het_j"], "impop_kin_watch", 16))
    for struct, dtype, plain, fields, cname, size in sides:
        assert C.sizeof(struct) == size == dtype.itemsize and dtype == plain
        assert [n for n, _ in struct._fields_] == fields == list(dtype.names)
        for name, _ in struct._fields_:  # same offsets on both sides
            assert getattr(struct, name).offset == dtype.fields[name][1]
        assert re.search(r"typedef struct %s \{\s*/\* %d bytes" % (cname, size), HEADER)
    assert _lib.KinWindow.n_pairs.offset == 8 and _lib.KinWindow.het_het.offset == 16 and _lib.KinWindow.n_related.offset == 40
    assert _lib.KinWindow.n_undefined.offset == 44 and _lib.KinWatch.het_j.offset == 12
    assert C.sizeof(_lib.KinshipParams) == 16 and [n for n, _ in _lib.KinshipParams._fields_] == ["struct_size", "kin_num", "kin_den", "reserved"]
    for struct, want in (("impop_kin_window", WINDOW_FIELDS), ("impop_kin_watch", ["het_het", "ibs0", "het_i", "het_j"]),
                         ("impop_kinship_params", ["struct_size", "kin_num", "kin_den", "reserved"])):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), HEADER, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert declared == want
    assert hasattr(impop_amd.BitMatrix, "genotypes") and hasattr(impop_amd.Context, "kinship_elapsed")
    assert all(hasattr(impop_amd.Genotypes, f) for f in ("kinship_scan", "download", "free"))


def test_cli_tables_on_a_stubbed_result():
    from impop_amd import kinship as kin
    ww, wp, wt = pk.scan(KNOWN, [(0, 1), (2, 3)], [(0, 6, 0), (0, 6, 0)], (0, 1), [(1, 0)])
    main, pairs, wat = kin.tables(["chr:0-6", "chr:0-6"], [6, 6], ["A", "B"], ww, wp["t"], [(1, 0)], wt)
    assert main == [["chr:0-6", "6", "2", "1", "0", "1", "2", "0", "0"]] * 2 and len(main[0]) == len(kin.WINDOW_COLUMNS)
    # the totals of two identical windows: every count doubled, the ratios unchanged
    assert pairs == [["A", "B", "12", "2", "4", "0", "2", "6", "4", repr(-2 / 3), repr(-5 / 4), repr(7.0 / 12), repr(2 / 12), "unrelated"]]
    assert len(pairs[0]) == len(kin.PAIR_COLUMNS)
    assert wat == [["chr:0-6", "B", "A", "2", "1", "0", "1", repr(-2 / 3), repr(-5 / 4)]] * 2 and len(wat[0]) == len(kin.WATCH_COLUMNS)
    # a pair without a heterozygous site: NA for both estimators and for the degree
    zero = np.zeros(9, np.int64)
    zero[0] = 5
    assert kin.pair_row("A", "B", zero)[9:] == ["NA", "NA", "1.0", "0.0", "NA"]


@pytest.mark.parametrize("extra,env,needle", [
    (["--devices", "2"], {}, "--devices"),
    ([], {"WORLD_SIZE": "2"}, "torch.distributed.run"),
    (["--panel", "a.txt"], {}, "--panel"),
    (["-t", "0.99"], {}, "--kin-threshold"),
    (["--kin-threshold", "1.5"], {}, "0 .. 1"),
    (["--kin-watch", "A,B"], {}, "go together"),
    (["--kin-watch", "A,A", "--kin-watch-table", "w.tsv"], {}, "two different sample names"),
])
def test_cli_refusals_need_no_device(extra, env, needle):
    """what --format kinship does not combine with: one line on stderr and exit code 2, before any file or device is opened"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", "none.npz", "--bed", "none.bed", "--format",
                        "kinship"] + extra, capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, **env), timeout=120)
    assert r.returncode == 2 and needle in r.stderr and r.stdout == "", (r.returncode, r.stderr)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "impop_scan.py"), "--matrix", "none.npz", "--bed", "none.bed", "--format",
                        "diploid", "--kin-pairs", "p.tsv"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and "belong to --format kinship" in r.stderr
