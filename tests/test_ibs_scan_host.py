"""No GPU: the host side of impop_ibs_scan — the known answer of the header against the plain restatement, the restatement against
a brute-force per-site loop, the ABI declaration and its binding, the record layouts on both sides, and what scripts/impop_scan.py
refuses and writes for --format ibs (hand-made records: no device is opened)."""
import ctypes as C
import importlib.util
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ibs_cases as ic
import plain_ibs as pi
from conftest import ROOT

SCAN = os.path.join(ROOT, "scripts", "impop_scan.py")
PAIR_FIELDS = ["h1", "h2", "n_diff", "longest", "n_tracts", "reserved", "tract_sites"]
SEGMENT_FIELDS = ["h1", "h2", "begin", "end", "pair", "flags"]
WINDOW_FIELDS = ["pair_sites", "tracts", "pairs_spanning", "n_sites", "reserved", "share"]
PARAM_FIELDS = ["struct_size", "min_sites", "site_begin", "site_end", "max_chunk_bytes"]


def load_cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("impop_scan_cli_ibs", SCAN)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    return mod


# ---- the definitions ------------------------------------------------------------------------------------------------------------------

def test_known_answer_of_the_header():
    m01 = ic.known_matrix()
    rec, seg, win = pi.reference(m01, pi.all_pairs(range(4)), 0, 6, ic.KNOWN_MIN_SITES, ic.KNOWN_WINDOWS)
    assert [tuple(int(x) for x in r) for r in rec] == ic.KNOWN_PAIR_ROWS
    assert [tuple(int(x) for x in s) for s in seg] == ic.KNOWN_SEGMENTS
    assert len(seg) == 6 and int(rec["tract_sites"].sum()) == 19
    assert [(int(w["pair_sites"]), int(w["tracts"]), int(w["pairs_spanning"])) for w in win] == ic.KNOWN_WINDOW_ROWS
    assert win["n_sites"].tolist() == [6, 2, 3] and win["share"].tolist() == [19.0 / 36.0, 12.0 / 12.0, 9.0 / 18.0]
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    body = header[header.index("#define IMPOP_IBS_MAX_N"):header.index("typedef struct impop_ibs_params")]
    for row in ic.KNOWN_ROWS:  # the case is stated in the header
        assert row in body
    for text in ("[1,6) OPEN_RIGHT", "[0,4) OPEN_LEFT", "Six segments, 19 tract sites", "(19, 6, 0)", "(12, 6, 6)", "(9, 6, 1)"):
        assert text in body, text


def brute_force(m01, pairs, b, e, min_sites, windows):
    """one site at a time: a counter of the sites since the last difference"""
    rows, segs = [], []
    for k, (h1, h2) in enumerate(pairs):
        n_diff = longest = n_tracts = sites = 0
        run_begin = b
        for s in range(b, e + 1):
            if s == e or m01[h1, s] != m01[h2, s]:
                length = s - run_begin
                longest = max(longest, length)
                if length >= min_sites and length > 0:
                    n_tracts += 1
                    sites += length
                    segs.append((k, run_begin, s))
                if s < e:
                    n_diff += 1
                run_begin = s + 1
        rows.append((n_diff, longest, n_tracts, sites))
    wins = []
    for wb, we in windows:
        covered = meets = spans = 0
        for _, s, t in segs:
            n_in = sum(1 for x in range(wb, we) if s <= x < t)
            covered += n_in
            meets += n_in > 0
            spans += we > wb and n_in == we - wb
        wins.append((covered, meets, spans))
    return rows, segs, wins


@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_a_per_site_loop(seed):
    rng = np.random.default_rng(20100 + seed)
    n, S = int(rng.integers(2, 7)), int(rng.integers(1, 90))
    m01 = (rng.random((n, S)) < rng.choice([0.05, 0.3, 0.5])).astype(np.uint8)
    if seed % 2:
        m01[1] = m01[0]
    b = int(rng.integers(0, S))
    e = int(rng.integers(b + 1, S + 1))
    pairs = pi.all_pairs(range(n)) if seed % 3 else [(1, 0), (0, 1), (n - 1, 0), (0, 1)]
    windows = [(b, e), (b, b)] + [tuple(sorted(int(x) for x in rng.integers(b, e + 1, size=2))) for _ in range(5)]
    for min_sites in (1, 2, 7):
        rec, seg, win = pi.reference(m01, pairs, b, e, min_sites, windows)
        rows, segs, wins = brute_force(m01, pairs, b, e, min_sites, windows)
        assert [(int(r["n_diff"]), int(r["longest"]), int(r["n_tracts"]), int(r["tract_sites"])) for r in rec] == rows
        assert [(int(s["pair"]), int(s["begin"]), int(s["end"])) for s in seg] == segs
        assert [(int(w["pair_sites"]), int(w["tracts"]), int(w["pairs_spanning"])) for w in win] == wins
        assert all((s["flags"] & 1 != 0) == (s["begin"] == b) and (s["flags"] & 2 != 0) == (s["end"] == e) for s in seg)
        assert np.isnan(win["share"][1]) and (rec["h1"].tolist(), rec["h2"].tolist()) == tuple(map(list, zip(*pairs)))


def test_pairs_spanning_counts_the_pairs_identical_on_the_window():
    case = ic.geometry_case(33, 7)
    members = list(range(33))
    for (wb, we), w in zip(case.windows, case.want[2]):
        if we - wb < case.min_sites:
            continue
        same = sum(1 for i, j in pi.all_pairs(members) if (case.m01[i, wb:we] == case.m01[j, wb:we]).all())
        assert int(w["pairs_spanning"]) == same, (wb, we)
    assert any(w["pairs_spanning"] > 0 for w in case.want[2]) and any(w["pairs_spanning"] == 0 for w in case.want[2])


def test_cases_are_not_trivial():
    for n in (33, 130):
        for min_sites in (1, 7, 65):
            c = ic.geometry_case(n, min_sites)
            assert len(c.pairs) == n * (n - 1) // 2 and len(c.want[1]) == int(c.want[0]["n_tracts"].sum()) > 0
            assert (c.want[0]["longest"] == 0).any()  # a pair that differs everywhere
            assert (c.want[1]["flags"] == 0).any() and (c.want[1]["flags"] & 1).any() and (c.want[1]["flags"] & 2).any()
    h = ic.hand_case(ic.HAND_LONG)
    assert h.want[0]["n_tracts"].tolist() == [1, 0, 1, 1, h.want[0]["n_tracts"][4]]
    assert ic.hand_case(ic.HAND_LONG + 1).want[0]["n_tracts"].tolist()[:4] == [1, 0, 0, 0]
    with pytest.raises(AssertionError):
        ic.assert_nontrivial(np.zeros(3, dtype=pi.PAIR))


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------

def test_abi_declares_ibs_scan():
    import impop_amd
    from impop_amd import _lib
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    assert re.search(r"#define IMPOP_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    assert re.search(r"#define IMPOP_IBS_MAX_N\s+4096u\b", header) and _lib.IBS_MAX_N == 4096
    assert re.search(r"#define IMPOP_IBS_MAX_PAIRS\s+8388608u\b", header) and _lib.IBS_MAX_PAIRS == 8388608 >= 4096 * 4095 // 2
    assert re.search(r"#define IMPOP_IBS_OPEN_LEFT\s+1u\b", header) and re.search(r"#define IMPOP_IBS_OPEN_RIGHT\s+2u\b", header)
    assert (_lib.IBS_OPEN_LEFT, _lib.IBS_OPEN_RIGHT) == (pi.OPEN_LEFT, pi.OPEN_RIGHT) == (1, 2)
    for fn, n_args in (("impop_ibs_scan", 13), ("impop_ctx_ibs_elapsed", 3)):
        assert re.search(r"^int %s\(" % fn, header, re.M) and len(_lib.SIGNATURES[fn][1]) == n_args
    sides = ((_lib.IbsPair, impop_amd.IBS_PAIR_DTYPE, pi.PAIR, PAIR_FIELDS, "impop_ibs_pair"),
             (_lib.IbsSegment, impop_amd.IBS_SEGMENT_DTYPE, pi.SEGMENT, SEGMENT_FIELDS, "impop_ibs_segment"),
             (_lib.IbsWindow, impop_amd.IBS_WINDOW_DTYPE, pi.WINDOW, WINDOW_FIELDS, "impop_ibs_window"))
    for struct, dtype, plain, fields, cname in sides:
        assert C.sizeof(struct) == 32 == dtype.itemsize and dtype == plain
        assert [n for n, _ in struct._fields_] == fields == list(dtype.names)
        for name, _ in struct._fields_:  # same offsets on both sides
            assert getattr(struct, name).offset == dtype.fields[name][1]
        assert re.search(r"typedef struct %s \{\s*/\* 32 bytes" % cname, header)
    assert C.sizeof(_lib.IbsParams) == 32 and [n for n, _ in _lib.IbsParams._fields_] == PARAM_FIELDS
    assert _lib.IbsParams.max_chunk_bytes.offset == 24 and _lib.IbsPair.tract_sites.offset == 24 and _lib.IbsWindow.share.offset == 24
    for struct, want in (("impop_ibs_pair", PAIR_FIELDS), ("impop_ibs_segment", SEGMENT_FIELDS), ("impop_ibs_window", WINDOW_FIELDS),
                         ("impop_ibs_params", PARAM_FIELDS)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
        assert declared == want
    assert hasattr(impop_amd.BitMatrix, "ibs_scan") and hasattr(impop_amd.Context, "ibs_elapsed")
    if os.path.exists(_lib.SO_PATH):
        lib = C.CDLL(_lib.SO_PATH)
        assert hasattr(lib, "impop_ibs_scan") and hasattr(lib, "impop_ctx_ibs_elapsed")
        assert lib.impop_version() == 4


# ---- the driver -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra,env,needle", [
    (["--devices", "2"], {}, "not with --devices N"),
    (["-A", "a.txt", "-B", "b.txt"], {}, "not with -A / -B / --panel / -l"),
    (["--panel", "a.txt", "b.txt"], {}, "not with -A / -B / --panel / -l"),
    ([], {"WORLD_SIZE": "2", "RANK": "0"}, "not under torch.distributed.run"),
    ([], {"WORLD_SIZE": "2", "RANK": "1"}, "not under torch.distributed.run"),
    (["-t", "0.9"], {}, "-t / -r / --identity belong to other formats"),
    (["--ibs-min-sites", "0"], {}, "--ibs-min-sites takes 1 or more"),
])
def test_driver_refuses_next_to_ibs(extra, env, needle):
    r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "ibs", "--backend", "gloo"] + extra,
                       capture_output=True, text=True, env=dict(os.environ, **env), timeout=120)
    assert r.returncode == 2 and needle in r.stderr, (r.returncode, r.stderr[-500:])
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("Error: "), r.stderr[-500:]


def test_driver_refuses_sim_list_and_stray_options():
    r = subprocess.run([sys.executable, SCAN, "--sim-list", "none.tsv", "--format", "ibs"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and r.stderr.strip() == "Error: --format ibs scans a presence matrix (--matrix / --bed): not with --sim-list"
    for stray in (["--ibs-min-sites", "64"], ["--ibs-segments", "x.tsv"], ["--ibs-pairs", "diploid"], ["--ibs-pair-table", "x.tsv"]):
        r = subprocess.run([sys.executable, SCAN, "--matrix", "none.npz", "--bed", "none.bed", "--format", "ld"] + stray,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and r.stderr.strip() == "Error: --ibs-min-sites / --ibs-pairs / --ibs-segments / --ibs-pair-table belong to --format ibs"


def test_writers_on_hand_made_records():
    cli = load_cli()
    names = ["A#1#c", "A#2#c", "B#1#c"]
    win = np.zeros(2, dtype=pi.WINDOW)
    win[0] = (1234, 5, 2, 300, 0, 1234.0 / (3.0 * 300.0))
    win[1] = (0, 0, 0, 0, 0, np.nan)
    out = io.StringIO()
    cli.write_ibs_table(out, ["c:1000-1300", "c:1300-1300"], [300, 0], [3, 3], win)
    assert out.getvalue().splitlines() == ["REGION\tLENGTH\tPAIRS\tTRACTS\tPAIRS_SPANNING\tPAIR_SITES\tSHARE",
                                           "c:1000-1300\t300\t3\t5\t2\t1234\t1.37111111", "c:1300-1300\t0\t3\t0\t0\t0\tNA"]
    seg = np.array([(0, 1, 0, 40, 0, 1), (0, 2, 10, 600, 1, 2), (2, 1, 0, 600, 2, 3), (1, 2, 5, 9, 2, 0)], dtype=pi.SEGMENT)
    out = io.StringIO()
    cli.write_ibs_segments(out, names, seg, lambda c: 1000 + 2 * c)  # every site two bp apart
    assert out.getvalue().splitlines() == ["seq1\tseq2\tstart\tend\tsites\topen", "A#1#c\tA#2#c\t1000\t1079\t40\tL", "A#1#c\tB#1#c\t1020\t2199\t590\tR",
                                           "B#1#c\tA#2#c\t1000\t2199\t600\tLR", "A#2#c\tB#1#c\t1010\t1017\t4\t."]
    rec = np.array([(0, 1, 7, 40, 1, 0, 40), (2, 1, 0, 600, 1, 0, 600)], dtype=pi.PAIR)
    out = io.StringIO()
    cli.write_ibs_pairs(out, names, rec)
    assert out.getvalue().splitlines() == ["SEQ1\tSEQ2\tN_DIFF\tLONGEST\tTRACTS\tTRACT_SITES", "A#1#c\tA#2#c\t7\t40\t1\t40", "B#1#c\tA#2#c\t0\t600\t1\t600"]
