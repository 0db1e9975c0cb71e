"""No GPU: the host side of the windowed clustering — ABI declaration, the `--format af` writers and refusals of
scripts/impop_scan.py on hand-built records, the mirror's re-ordering of clusters against the reference's lists
(tests/golden/af_windows.json), the regeneration of that file, and that the planted GPU-test inputs mean something."""
import importlib.util
import io
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from af_cases import THRESHOLD, planted_matrix, seed_only_groups, subset_flags, window_identity, window_lists
from conftest import GOLDEN, ROOT
from plain_refs import adjacency, ref_components

SCAN = os.path.join(ROOT, "scripts", "impop_scan.py")


def load_cli():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        spec = importlib.util.spec_from_file_location("impop_scan_cli_af", SCAN)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(os.path.join(ROOT, "scripts"))
    return mod


def test_abi_declares_cluster_scan():
    import ctypes as C
    from impop_amd import _lib
    header = open(os.path.join(ROOT, "include", "impop_hip.h")).read()
    assert re.search(r"#define IMPOP_ABI_VERSION 4\b", header) and _lib.ABI_VERSION == 4
    assert re.search(r"\bint impop_cluster_scan\(", header) and "impop_cluster_scan" in _lib.SIGNATURES
    assert C.sizeof(_lib.ClusterStats) == 32
    import impop_amd
    assert impop_amd.CLUSTER_DTYPE.itemsize == 32
    assert [n for n, _ in _lib.ClusterStats._fields_] == list(impop_amd.CLUSTER_DTYPE.names)
    if os.path.exists(_lib.SO_PATH):
        assert hasattr(C.CDLL(_lib.SO_PATH), "impop_cluster_scan")


def test_af_writers_on_hand_built_records():
    import impop_amd
    cli = load_cli()
    recs = np.zeros(3, dtype=impop_amd.CLUSTER_DTYPE)
    recs[0] = (6, 3, 3, 1, 9 + 4 + 1, 100, 0)
    recs[1] = (5, 5, 1, 5, 5, 50, 0)
    recs[2] = (0, 0, 0, 0, 0, 10, 0)
    out = io.StringIO()
    cli.write_af_table(out, ["R:0-100", "R:100-150", "R:150-160"], [100, 50, 10], "0.9990", recs)
    assert out.getvalue().splitlines() == [
        "REGION\tLENGTH\tTHRESHOLD\tHAPLOTYPES\tCLUSTERS\tLARGEST\tSINGLETONS\tHOMOZYGOSITY",
        "R:0-100\t100\t0.9990\t6\t3\t3\t1\t0.388889",
        "R:100-150\t50\t0.9990\t5\t5\t1\t5\t0.200000",
        "R:150-160\t10\t0.9990\t0\t0\t0\t0\t0.000000"]
    clusters = [[["a", "b", "c"], ["d", "e"], ["f"]], [["x"]]]
    buf = io.StringIO(newline="")
    cli.write_af_clusters(buf, ["R:0-100", "R:100-150"], clusters)
    assert buf.getvalue() == ("REGION\tcluster_id\tcount\tfrequency\r\nR:0-100\tc1\t3\t0.500000\r\nR:0-100\tc2\t2\t0.333333\r\n"
                              "R:0-100\tc3\t1\t0.166667\r\nR:100-150\tc1\t1\t1.000000\r\n")
    buf = io.StringIO(newline="")
    cli.write_af_details(buf, ["R:0-100"], clusters[:1], 0.999)
    assert buf.getvalue() == ("REGION\tsample_id\tcluster_id\tthreshold\r\nR:0-100\ta\tc1\t0.999\r\nR:0-100\tb\tc1\t0.999\r\n"
                              "R:0-100\tc\tc1\t0.999\r\nR:0-100\td\tc2\t0.999\r\nR:0-100\te\tc2\t0.999\r\nR:0-100\tf\tc3\t0.999\r\n")


@pytest.mark.parametrize("extra,env,text", [
    (["--sim-list", "x.tsv"], {}, "not with --sim-list"),
    (["--matrix", "m.npz", "--bed", "w.bed", "--devices", "2"], {}, "not with --devices"),
    (["--matrix", "m.npz", "--bed", "w.bed"], {"WORLD_SIZE": "2"}, "not under torch.distributed.run"),
    (["--matrix", "m.npz", "--bed", "w.bed", "-A", "a.txt", "-B", "b.txt"], {}, "not with -A"),
])
def test_af_refusals_exit_before_any_device(extra, env, text):
    r = subprocess.run([sys.executable, SCAN, "--format", "af"] + extra, env=dict(os.environ, **env), capture_output=True, text=True)
    assert r.returncode == 2 and r.stdout == "" and text in r.stderr, r.stderr


def test_af_side_tables_need_format_af():
    r = subprocess.run([sys.executable, SCAN, "--format", "pica2", "--matrix", "m.npz", "--bed", "w.bed", "--af-clusters", "c.tsv"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "belong to --format af" in r.stderr


def test_mirror_reorders_clusters_like_the_reference():
    """cluster ranks by (-size, smallest index) — what the kernel returns — turned into the reference's lists, whose equal-size
    clusters are ordered by their sorted names; names differ from index order in one golden case"""
    from impop_amd.af import _sample_of, clusters_from_ranks
    with open(os.path.join(GOLDEN, "af_windows.json")) as f:
        gold = json.load(f)
    moved = 0
    for case in gold["cases"]:
        names = case["names"]
        ix = {nm: i for i, nm in enumerate(names)}
        for w in case["windows"]:
            t = np.full((case["n"], case["n"]), np.nan)
            for a, b, v in w["sim"]:
                t[ix[a], ix[b]] = t[ix[b], ix[a]] = float(v)
            cl, K, _ = ref_components(adjacency(t, w["threshold"]))
            samples = [_sample_of(nm) for nm in names]
            got = clusters_from_ranks(cl, samples)
            assert got == w["clusters"]
            by_index = [sorted(samples[i] for i in np.flatnonzero(cl == k)) for k in range(K)]
            moved += by_index != got
    assert moved  # the tie rule by names was exercised


def test_mirror_merges_members_that_share_a_sample_name():
    from impop_amd.af import clusters_from_ranks
    assert clusters_from_ranks([0, 1, 1, 2], ["s1", "s1", "s2", "s3"]) == [["s1", "s2"], ["s3"]]


def test_golden_regenerates_byte_identically(tmp_path):
    ref = os.environ.get("IMPOP_REFERENCE", "/root/reference")
    if not os.path.exists(os.path.join(ref, "scripts", "af.py")):
        pytest.skip("the reference checkout is not on this machine")
    out = str(tmp_path / "af_windows.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_af_golden.py"), "--ref", ref, "--out", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "af_windows.json"), "rb").read()


@pytest.mark.parametrize("n", [31, 465])
@pytest.mark.parametrize("kind", ["match", "dice"])
@pytest.mark.parametrize("masked", [False, True])
def test_planted_inputs_mean_something(oracle, n, kind, masked):
    """what tests/test_gpu_cluster_scan.py asserts of its inputs before it looks at the GPU, here without one"""
    m01 = planted_matrix(n, 16, 7000 + n)
    bits = oracle.pack_hap_major(m01)
    members = np.flatnonzero(subset_flags(n)) if masked else None
    for shape, wins in window_lists(16).items():
        nontrivial = open_comp = tie = False
        for w in wins:
            t = window_identity(oracle, bits, n, w[0], w[1], kind, None, members)
            a = adjacency(t, THRESHOLD)
            cl, K, sz = ref_components(a)
            nontrivial |= 1 < K < len(cl)
            tie |= len(set(sz.tolist())) < len(sz)
            same = cl[:, None] == cl[None, :]
            open_comp |= bool((same & ~(a | a.T)).any()) and len(set(seed_only_groups(a | a.T).tolist())) != K
        assert nontrivial and open_comp and tie, (shape, nontrivial, open_comp, tie)
