"""No GPU: the plain restatement of impop_recomb_scan (tests/recomb_cases.py) against Hudson & Kaplan's deletion procedure stated
literally, the header's known answer, the perfect-phylogeny generator, the host tables of impop_amd/recomb.py, and what
scripts/impop_recomb.py refuses before it opens a file."""
import os
import subprocess
import sys

import numpy as np
import pytest

import recomb_cases as rc
from conftest import ROOT

SCRIPT = os.path.join(ROOT, "scripts", "impop_recomb.py")


def _random_small(rng):
    n, m = int(rng.integers(4, 12)), int(rng.integers(0, 14))
    return (rng.random((m, n)) < rng.choice([0.2, 0.5])).astype(np.uint8), n


def test_greedy_rmin_is_the_deletion_procedure_on_300_matrices():
    rng = np.random.default_rng(32100)
    positive = 0
    for _ in range(300):
        rows, n = _random_small(rng)
        inc, cong, _ = rc.pair_relations(rows, n)
        left1, n_left, rep = rc.site_rows(inc, cong)
        got = len(rc.rmin_intervals(left1))
        assert got == rc.hudson_kaplan(inc), (rows.tolist(), left1)
        positive += got > 0
        # every chosen interval is an incompatible pair, and they are disjoint
        iv = rc.rmin_intervals(left1)
        assert all(inc[a, b] for a, b in iv) and all(iv[k][1] <= iv[k + 1][0] for k in range(len(iv) - 1))
        assert sum(n_left) == int(np.triu(inc, 1).sum())
    assert positive > 100


def test_known_answer():
    K = rc.KNOWN
    inc, cong, c = rc.pair_relations(rc.KNOWN_ROWS, 4)
    left1, n_left, rep = rc.site_rows(inc, cong)
    assert (left1, n_left, rep) == (K["left1"], K["n_left"], K["rep"]) and c.tolist() == [2, 2, 2, 2, 1]
    v = rc.window_values(left1, n_left, rep)
    for k in ("n_incompatible", "n_incompatible_adjacent", "rmin", "n_blocks", "longest_block_sites", "longest", "n_congruent_adjacent",
              "n_congruent_partitions", "n_partitions"):
        assert v[k] == K[k], k
    assert rc.rmin_intervals(left1) == K["intervals"] and rc.hudson_kaplan(inc) == 2
    fgt, b, q = rc.doubles(5, v["n_incompatible"], v["n_congruent_adjacent"], v["n_congruent_partitions"])
    assert (fgt, b, q) == (0.3, K["wall_b"], K["wall_q"])
    assert all(np.isnan(x) for x in rc.doubles(0, 0, 0, 0)) and np.isnan(rc.doubles(1, 0, 0, 0)[1]) and rc.doubles(1, 0, 0, 0)[2] == 0.0
    rec, used, table = rc.reference(np.ascontiguousarray(rc.KNOWN_ROWS.T), None, [(0, 5), (1, 4), (2, 2)], 1)
    assert rec["rmin"].tolist() == [2, 1, 0] and rec["n_blocks"].tolist() == [3, 2, 0] and used[1, :4].tolist() == [1, 2, 3, 0]
    assert (rec["longest_block_begin"][0], rec["longest_block_end"][0]) == (2, 4)


@pytest.mark.parametrize("n", (5, 33, 200))
def test_a_tree_shows_no_recombination(n):
    rng = np.random.default_rng(32200 + n)
    t01 = rc.tree_matrix(rng, n, 150)
    rec, _, table = rc.reference(t01, None, [(0, 150)], 1)
    assert rec["n_used"][0] > 20 and rec["n_incompatible"][0] == 0 and rec["rmin"][0] == 0 and rec["n_blocks"][0] == 1
    assert not table["left1"].any() and rec["longest_block_sites"][0] == rec["n_used"][0]
    segs = (40, 70, 25, 130)
    mo = rc.mosaic(rng, n, segs)
    r2 = rc.reference(mo, None, [(0, sum(segs))], 1)[0]
    assert r2["rmin"][0] <= len(segs) - 1 and (n < 33 or r2["rmin"][0] > 0)


def test_host_tables_are_the_restatement():
    from impop_amd import recomb
    rng = np.random.default_rng(32300)
    for _ in range(60):
        rows, n = _random_small(rng)
        inc, cong, _ = rc.pair_relations(rows, n)
        left1, n_left, rep = rc.site_rows(inc, cong)
        m = len(left1)
        padded = np.array(left1 + [7, 7, 7], dtype=np.uint32)  # entries past n_used are never read
        assert recomb.intervals(padded, m) == rc.rmin_intervals(left1)
        got = recomb.blocks(padded, m)
        assert got == rc.maximal_blocks(left1)
        # the blocks by search: maximal runs of pairwise compatible sites
        ok = lambda a, b: not inc[a:b + 1, a:b + 1].any()  # noqa: E731
        runs = [(a, b) for b in range(m) for a in range(b + 1) if ok(a, b) and not (a > 0 and ok(a - 1, b)) and not (b + 1 < m and ok(a, b + 1))]
        assert sorted(got) == sorted(runs)
    assert recomb.fmt(float("nan")) == "NA" and recomb.fmt(0.25) == "0.25000000"
    rec = {"n_used": 5, "n_members": 4, "n_sites": 5, "n_qualifying": 5, "rmin": 2, "n_incompatible": 3, "four_gamete_fraction": 0.3,
           "n_incompatible_adjacent": 2, "n_blocks": 3, "longest_block_sites": 3, "longest_block_begin": 2, "longest_block_end": 4,
           "wall_b": 0.25, "wall_q": 0.4}
    assert recomb.main_row("c:100-105", 5, rec, lambda s: 100 + s) == ["c:100-105", "5", "4", "5", "5", "5", "2", "3", "0.30000000", "2", "3",
                                                                       "3", "102", "104", "0.25000000", "0.40000000"]
    assert len(recomb.MAIN_COLUMNS) == 16


@pytest.mark.parametrize("extra, env, needle", [
    ([], {"WORLD_SIZE": "2"}, "one process"),
    (["--recomb-min-maf", "0.6"], {}, "--recomb-min-maf"),
    (["--recomb-max-sites", "1"], {}, "--recomb-max-sites"),
    (["--recomb-max-sites", "16385"], {}, "--recomb-max-sites"),
])
def test_cli_refusals(extra, env, needle, tmp_path):
    r = subprocess.run([sys.executable, SCRIPT, "--matrix", str(tmp_path / "none.npz"), "--bed", str(tmp_path / "none.bed")] + extra,
                       capture_output=True, text=True, cwd=ROOT, env=dict(os.environ, **env), timeout=120)
    assert r.returncode != 0 and needle in r.stderr and "Traceback" not in r.stderr, r.stderr[-2000:]
