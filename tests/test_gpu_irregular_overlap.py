"""GPU: the windowed all-pairs calls (impop_pairwise_scan, impop_pairwise_scan_panel, impop_cluster_scan) on an irregular window
list — unsorted, with duplicate, nested, empty and one-site windows and a disjoint one behind a gap (tests/overlap_cases.py).

The planner (csrc/pair_plan.h) cuts such a list into 18 elementary segments, and the statistics kernels form a window's Gram
counts as the sum of 0, 1, 2, 3, 5, 7, 9 or 14 consecutive matrices, in an order that is not the caller's.  Regular sliding lists
(every other test of the segmented route) give 2 or 4 segments per window and the identity order.  Here, for 40 / 130 / 300 / 513
haplotypes, plain and compacted, and for a weighted matrix against its bp-expanded form:

  * every window of every call against the C oracle on the dense uncompacted matrix (pica2 / h-fst / hud.py grouped Fst through
    test_gpu_batch_regimes._check, af clustering through test_gpu_cluster_scan.expected / check_window; integer fields equal,
    floating fields under conftest.stat_close / rel_close at 1e-9: INTEGRATION.md §4), the panel call also field by field
    against pairwise_scan of the same list, as test_gpu_pairwise_panel.check_call does;
  * the list call against the same call made one window at a time (one-matrix kernels), byte for byte;
  * the duplicates, the compacted matrix on windows without a kept site, the one-site window on an all-ones column;
  * from the IMPOP_TRACE=1 lines: 18 cells for 12 windows in one chunk, 4 (6) chunks under IMPOP_PAIRWISE_CHUNK=3 (2);
  * IMPOP_PAIRWISE_CHUNK=3 / 2 and IMPOP_GRAM_U16=0 change no byte; IMPOP_EPILOGUE_SMALL=0 (the general kernels' segment loops
    at every n) changes no integer and stays within the oracle's tolerance.

(A Gram launch of 18 cells splits its site axis, and a split launch writes int32 counts: at these sizes every run here has
int32 counts, so IMPOP_GRAM_U16=0 only pins that down.  The uint16 instantiations of the segment loops need thousands of cells
per launch; they are reached by the regular slides of test_gpu_batch_regimes alone.)

All GPU work runs in child processes (the switches are read once per process), one after another; this process computes the
oracle's side once (fixture `ref`)."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import overlap_cases as oc
from conftest import ROOT, stat_close
from overlap_cases import parts
from test_gpu_batch_regimes import SWITCHES, _check
from test_gpu_cluster_scan import check_window, expected

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FST_KEYS = ("fst", "pi_a", "pi_b", "pi_xy", "dxy", "da")
EMPTY, ALL_ONES, ALL_ZEROS, DUPLICATES = 4, 3, 8, (1, 5)  # indices into the window list
_GRAM = re.compile(r"\[impop_gram\] (.*)$")
_CHUNK = re.compile(r"\[impop_(?:pairwise_scan|pairwise_scan_panel|cluster_scan)\] chunk done")


def _child(extra, each=False):
    """-> (arrays by name, trace by call tag: {"gram": [launch dicts], "chunks": chunk-done lines}) of one child process"""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES + ("IMPOP_PAIRWISE_CHUNK",)}
    env.update(PYTHONPATH=os.pathsep.join([ROOT, HERE]), IMPOP_TRACE="1", **extra)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        r = subprocess.run([sys.executable, os.path.join(HERE, "overlap_cases.py"), path] + (["each"] if each else []),
                           capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
        assert r.returncode == 0, (extra, r.stderr[-3000:])
        with np.load(path) as z:
            got = {k: z[k].copy() for k in z.files}
    trace, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@@call "):
            cur = line[7:]
            trace[cur] = {"gram": [], "chunks": 0}
        elif cur is not None and (m := _GRAM.search(line)):
            trace[cur]["gram"].append({k: int(v) for k, v in (kv.split("=") for kv in m.group(1).split())})
        elif cur is not None and _CHUNK.search(line):
            trace[cur]["chunks"] += 1
    return got, trace


@pytest.fixture(scope="module")
def default_run():
    return _child({}, each=True)


def _list_tags():
    return [f"{mt}.{name}" for mt, (n, _, _) in oc.matrices().items() for name in oc.call_names(n)]


def _is_each(name):
    return name.split("#")[0].endswith(".each")


def _array_names():
    """what a child without `each` saves: one array per pairwise_scan call, three per panel or cluster call"""
    one = lambda tag: ".ps_" in tag or ".pp" in tag  # noqa: E731
    return sorted(x for tag in _list_tags() for x in ([tag] if one(tag) else [f"{tag}#{i}" for i in range(3)]))


# ---- the oracle's side, computed once ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ref(oracle):
    """per matrix tag: the dense uncompacted matrix the records must describe (the weighted one bp-expanded), its windows, and the
    exact counts of every window; `clusters` caches the expected clusterings"""
    dense = {f"n{n}": (oc.matrix(n), oc.WINDOWS) for n in oc.SHAPES}
    node, wt, _, bp_wins = oc.weighted_inputs()
    dense[f"w{oc.WEIGHTED_N}"] = (np.repeat(node, wt, axis=1), bp_wins)
    out = {"clusters": {}}
    for key, (m, wins) in dense.items():
        bits = oracle.pack_hap_major(m)
        out[key] = {"m": m, "bits": bits, "wins": wins, "n": m.shape[0],
                    "I": [oracle.pairwise_counts(bits, m.shape[0], a, b) for a, b, _ in wins]}
    return out


def _seg_sites(m, rows, a, b):
    c = m[rows.astype(bool), a:b].sum(0)
    return int(((c > 0) & (c < int(rows.sum()))).sum())


def _check_pairwise(oracle, R, rec, call, inP, inA, inB, s_scope, what):
    """every window of one pairwise_scan call: pica2 of P and the Fst of A / B through _check; n_sites, S and Tajima's D"""
    n, sel = R["n"], np.flatnonzero(inP)
    assert rec.shape == (len(R["wins"]),)
    for k, (a, b, L) in enumerate(R["wins"]):
        r, w = rec[k], what + (k, (a, b, L))
        _check(oracle, R["I"][k], b - a, r, call, inA, inB, L, w, sel=sel)
        assert int(r["n_sites"]) == b - a and int(r["reserved"]) == 0, w
        if s_scope == 1:
            assert int(r["s_all"]) == _seg_sites(R["m"], np.ones(n, np.uint8), a, b) and int(r["s_p"]) == _seg_sites(R["m"], inP, a, b), w
            if len(sel) >= 2 and L:
                D, _ = oracle.tajimas_d(len(sel), float(r["s_p"]), oracle.py_round(float(r["pi_site"]), 8))
                assert float(r["tajima_d"]) == D or (D != D and np.isnan(r["tajima_d"])), w + (float(r["tajima_d"]), D)
            else:
                assert np.isnan(r["tajima_d"]), w
        else:
            assert int(r["s_all"]) == 0 and int(r["s_p"]) == 0 and np.isnan(r["tajima_d"]), w


def _check_panel(oracle, R, got, tag, pops, s_scope):
    """the panel call: per panel the fields of pairwise_scan(mask_p = the panel), byte for byte; per pair those of
    pairwise_scan(mask_a, mask_b) and the oracle's h-fst under stat_close; the pairwise_scan records themselves against the oracle"""
    c, n, K = oc.PANEL_CALL, R["n"], len(pops)
    pan, pairs, pw = parts(got, f"{tag}.panel")
    assert pan.shape == (len(R["wins"]), K) and pairs.shape == (len(R["wins"]), K * (K - 1) // 2) and pw.shape == (len(R["wins"]),)
    for k, (a, b, _) in enumerate(R["wins"]):
        want_s = _seg_sites(R["m"], np.ones(n, np.uint8), a, b) if s_scope == 1 else 0
        assert int(pw[k]["n_sites"]) == b - a and int(pw[k]["s_all"]) == want_s, (tag, k)
    for j, (x, y) in enumerate(oc.PANEL_PAIRS):
        two = got[f"{tag}.pp{j}"]
        _check_pairwise(oracle, R, two, c, pops[j], pops[x], pops[y], s_scope, (tag, f"pp{j}"))
        for key in ("pi", "pi_site", "tajima_d", "n_groups") + (("s_p",) if s_scope == 1 else ()):
            assert pan[:, j][key].tobytes() == two[key].tobytes(), (tag, j, key, pan[:, j][key], two[key])
        assert (pan[:, j]["n_members"] == int(pops[j].sum())).all() and (pan[:, j]["reserved"] == 0).all()
        for k, (a, b, L) in enumerate(R["wins"]):
            h, _ = oracle.hfst(oracle.identity(R["I"][k], b - a, 0), pops[x], pops[y], L if L else None, c["rd"])
            for key in FST_KEYS:
                v = float(pairs[k, j][key])
                assert stat_close(key, v, h[key], h["dxy"]), (tag, "oracle", j, k, key, v, h[key])
                assert stat_close(key, v, float(two[k][key]), float(two[k]["dxy"])), (tag, "pairwise_scan", j, k, key, v)


def _check_clusters(oracle, ref, R, key, got, tag, name, inP):
    c = oc.CL_CALLS[name]
    rec, cl, sz = parts(got, f"{tag}.cl_{name}")
    members = np.flatnonzero(inP)
    assert cl.shape == (len(R["wins"]), len(members)) and sz.shape == cl.shape
    want = ref["clusters"].get((key, name))
    if want is None:
        want = [expected(oracle, R["bits"], R["n"], w, c["kind"], c["rd"], c["thr"], members) for w in R["wins"]]
        assert any(1 < K < len(members) for _, K, _, _ in want), (key, name)  # the threshold clusters some window non-trivially
        ref["clusters"][(key, name)] = want
    for k, (a, b, _) in enumerate(R["wins"]):
        check_window(rec[k], cl[k], sz[k], want[k], b - a)


def _check_against_oracle(oracle, ref, got):
    for tag, (n, _, s_scope) in oc.matrices().items():
        key = tag.split(".")[0]
        R = ref[key]
        inP, inA, inB = oc.masks(n)
        for name, c in oc.PS_CALLS.items():
            _check_pairwise(oracle, R, got[f"{tag}.ps_{name}"], c, inP, inA, inB, s_scope, (tag, name))
        for name in oc.CL_CALLS:
            _check_clusters(oracle, ref, R, key, got, tag, name, inP)
        if n in oc.PANEL_SIZES:
            _check_panel(oracle, R, got, tag, oc.panel_flags(n), s_scope)


# ---- the tests ---------------------------------------------------------------------------------------------------------------

def test_every_window_against_the_oracle(default_run, oracle, ref):
    got, _ = default_run
    assert sorted(k for k in got if not _is_each(k)) == _array_names()
    _check_against_oracle(oracle, ref, got)


def test_list_equals_one_window_at_a_time(default_run):
    """A one-window list is a tiling: the one-matrix kernels.  The sums over segments are integer sums, so the records and tables
    of the list call are theirs byte for byte."""
    got, _ = default_run
    for tag in _list_tags():
        if ".pp" in tag:
            continue
        for i, (a, b) in enumerate(zip(parts(got, tag), parts(got, tag + ".each"))):
            assert a.shape == b.shape and a.dtype == b.dtype, (tag, i)
            for k in range(len(a)):
                assert a[k].tobytes() == b[k].tobytes(), (tag, i, k, oc.SEG_COUNTS[k], a[k], b[k])


def test_duplicates_and_windows_without_a_kept_site(default_run):
    got, _ = default_run
    for tag in _list_tags():
        for i, a in enumerate(parts(got, tag)):
            assert a[DUPLICATES[0]].tobytes() == a[DUPLICATES[1]].tobytes(), (tag, i)
    for tag, (n, _, _) in oc.matrices().items():
        # the one-site window on the all-ones column: every identity is 1
        for name in oc.PS_CALLS:
            r = got[f"{tag}.ps_{name}"][ALL_ONES]
            assert float(r["pi"]) == 0.0 and int(r["n_groups"]) == 1, (tag, name, r)
        for name in oc.CL_CALLS:
            assert int(parts(got, f"{tag}.cl_{name}")[0][ALL_ONES]["n_clusters"]) == 1, (tag, name)
        if n in oc.PANEL_SIZES:
            pan = parts(got, f"{tag}.panel")[0][ALL_ONES]
            assert (pan["pi"] == 0).all() and (pan["n_groups"] == 1).all(), (tag, pan)
        # a compacted matrix keeps neither column 410 nor column 150: no Gram matrix for a window of one site — the plain
        # matrix's records, byte for byte
        plain = {"compact": tag.replace(".compact", ".plain"), "node_compact": tag.replace(".node_compact", ".node")}.get(tag.split(".")[1])
        if plain:
            for name in oc.call_names(n):
                for i, (a, b) in enumerate(zip(parts(got, f"{tag}.{name}"), parts(got, f"{plain}.{name}"))):
                    for k in (ALL_ONES, ALL_ZEROS, EMPTY):
                        assert a[k].tobytes() == b[k].tobytes(), (tag, name, i, k, a[k], b[k])


def test_the_segmented_route_was_taken(default_run):
    """the [impop_gram] line of every call on an uncompacted matrix: one launch of 18 cells for the 12 windows, one chunk"""
    _, trace = default_run
    for tag in _list_tags():
        t = trace[tag]
        assert t["chunks"] == 1, (tag, t)
        if ".compact" not in tag and ".node_compact" not in tag:
            assert [g["cells"] for g in t["gram"]] == [oc.N_CELLS], (tag, t)
        else:  # fewer cuts survive the compaction, but the windows still share cells
            assert len(t["gram"]) == 1 and 0 < t["gram"][0]["cells"] <= oc.N_CELLS, (tag, t)


@pytest.mark.parametrize("env,chunks", [({"IMPOP_PAIRWISE_CHUNK": "3"}, 4), ({"IMPOP_PAIRWISE_CHUNK": "2"}, 6), ({"IMPOP_GRAM_U16": "0"}, 1)],
                         ids=["chunks-of-3", "chunks-of-2", "int32-counts"])
def test_switches_change_no_byte(default_run, env, chunks):
    """chunks that cut the list (first_of() subtracts a non-zero c_lo, neighbouring chunks contract shared cells again) and
    int32 counts where uint16 would do"""
    base, _ = default_run
    got, trace = _child(env)
    assert sorted(got) == _array_names()
    for name in got:
        assert got[name].tobytes() == base[name].tobytes(), (env, name)
    for tag in _list_tags():
        t = trace[tag]
        assert t["chunks"] == chunks, (env, tag, t)
        if "IMPOP_GRAM_U16" in env:
            assert all(g["u16"] == 0 for g in t["gram"]), (tag, t)
        elif ".compact" not in tag and ".node_compact" not in tag:  # every chunk holds a window with sites; shared cells twice
            assert len(t["gram"]) == chunks and sum(g["cells"] for g in t["gram"]) > oc.N_CELLS, (env, tag, t)


def test_general_kernels_sum_segments(default_run, oracle, ref):
    """IMPOP_EPILOGUE_SMALL=0: n = 40 / 130 / 300 through gram_at and the segment loops of the general kernels.  They sum in
    another order than the window-shape kernels: integer fields and tables equal, floating fields within the oracle's tolerance."""
    base, _ = default_run
    got, _ = _child({"IMPOP_EPILOGUE_SMALL": "0"})
    assert sorted(got) == _array_names()
    for name, a in got.items():
        b = base[name]
        if a.dtype.names is None:
            assert a.tobytes() == b.tobytes(), name
            continue
        for f in a.dtype.names:
            if a.dtype[f].kind in "iu":
                assert a[f].tobytes() == b[f].tobytes(), (name, f)
    _check_against_oracle(oracle, ref, got)
