"""GPU: scripts/impop_scan.py on two matrices at once puts every record on the row of its own region.  Two matrices of 16
haplotypes (chr3: 2000 sites, chr8: 1500), a BED of four rows that alternate between them plus one row of a chromosome nobody holds;
per format three runs: both matrices, the first alone, the second alone.  `ld` prints in BED order, `kinship` grouped by matrix in
the order of each matrix's first BED row; every row of the joint run equals the same region's row of its single-matrix run."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SCAN = os.path.join(ROOT, "scripts", "impop_scan.py")
BED_ROWS = [("chr8", 100, 900), ("chr3", 1000, 2000), ("chrX", 5, 50), ("chr8", 900, 1500), ("chr3", 2000, 2500)]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from impop_amd import matrixio
    d = tmp_path_factory.mktemp("two_matrices")
    rng = np.random.default_rng(2024)
    n = 16
    for chrom, W, origin in (("chr3", 2000, 500), ("chr8", 1500, 0)):
        anc = (rng.random(W) < 0.3).astype(np.uint8)
        fam = np.repeat(anc[None], 4, axis=0) ^ (rng.random((4, W)) < 0.05).astype(np.uint8)
        m = fam[rng.integers(0, 4, size=n)] ^ (rng.random((n, W)) < 0.02).astype(np.uint8)
        names = [f"S{i // 2:03d}#{i % 2 + 1}#{chrom}:{origin}-{origin + W}" for i in range(n)]
        matrixio.save_matrix(str(d / f"{chrom}.npz"), matrixio.from_dense(m, names, origin=origin, contig=f"CHM13#0#{chrom}"))
    (d / "g.bed").write_text("".join(f"{c}\t{s}\t{e}\n" for c, s, e in BED_ROWS))
    return d


def run(inputs, fmt, matrices):
    r = subprocess.run([sys.executable, SCAN, "--matrix"] + [str(inputs / f"{m}.npz") for m in matrices] + ["--bed", str(inputs / "g.bed"),
                       "--format", fmt], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    return lines[0], lines[1:], r.stderr


def region(chrom, s, e):
    return f"CHM13#0#{chrom}:{s}-{e}"


@pytest.mark.parametrize("fmt,order", [
    ("ld", [0, 1, 3, 4]),        # BED order
    ("kinship", [0, 3, 1, 4]),   # grouped by matrix, chr8 first: its first row comes first in the BED
])
def test_joint_run_equals_the_single_matrix_runs(inputs, fmt, order):
    header, rows, err = run(inputs, fmt, ["chr3", "chr8"])
    assert err.count("no matrix holds chromosome") == 1 and "Skipping region CHM13#0#chrX:5-50" in err
    assert [r.split("\t")[0] for r in rows] == [region(*BED_ROWS[k]) for k in order]
    single = {}
    for chrom in ("chr3", "chr8"):
        h1, rows1, err1 = run(inputs, fmt, [chrom])
        assert h1 == header and err1.count("no matrix holds chromosome") == 3
        assert [r.split("\t")[0] for r in rows1] == [region(*b) for b in BED_ROWS if b[0] == chrom]
        single.update({r.split("\t")[0]: r for r in rows1})
    assert len(single) == 4
    for r in rows:
        assert r == single[r.split("\t")[0]]
    assert len({r.split("\t", 2)[2] for r in rows}) == 4  # four regions, four different records: a mixed-up row would show
