"""No GPU: the inputs of the principal-component tests (tests/pca_cases.py) meet, by the plain restatement alone, the conditions the
certified bounds of tests/test_gpu_pca_scan.py rest on."""
import pytest

import pca_cases as pcs


@pytest.mark.parametrize("n", pcs.NS)
def test_inputs_meet_the_preconditions(n):
    """the guaranteed regime for every (window, mask, k), no eigenvalue where the zero rule could go either way; a window of rank 0
    in every list; rank < k for k = 8 at m = 3; one non-zero eigenvalue at m = 2"""
    worst = 0.0
    for shape in ("tiling", "sliding"):
        for mask in pcs.MASKS:
            ratio, ranks = pcs.preconditions(n, shape, mask)
            worst = max(worst, ratio)
            assert 0 in ranks, (shape, mask, ranks)
            if mask == "three":
                assert max(ranks) == 2
            if mask == "pair":
                assert set(ranks) == {0, 1}
                refs = pcs.references(n, shape, mask)
                assert all(abs(r["lam"][0] - r["sum_h"] / 2) <= 1e-12 * r["sum_h"] for r in refs)  # lambda_1 = H_02 / 2
            if mask == "all" and n >= 65:
                assert max(ranks) == 8
    assert 0.0 < worst <= 0.9
