"""The inputs of test_gpu_scan_shared_context.py can tell one plan's Tajima constants from another's: a condition on the
inputs, checked on the host with the CPU oracle alone.

For every pair of subset sizes the GPU scenarios run, and every window of their lists, D is worked out from the window's own S
and pi with the constants of the plan's own n and with those of the other plan's n.  At least half of the windows must have a
finite D, and there the two must differ by more than 1e-6 relative: three orders above the 1e-9 the GPU tests compare to.

n = 2 is the one size with no finite D at all: b1 = b2 = 1 and a1 = a2 = 1 give c1 = c2 = 0 exactly, so e1 = e2 = 0, the
denominator is 0 and tj_d.py returns nan for every S and pi.  For the plan of the pair (2, 40) whose |P| is 2 the condition is
therefore the NaN rule instead: its right D is NaN in every window, and with the other plan's constants at least half of the
windows (in fact all) must come out finite, which the comparison of the GPU tests refuses just as it refuses a wrong number.
The other plan of that pair, |P| = 40, is held to the condition as written: with the constants of n = 2 its finite D turn NaN."""
import math

import pytest

import shared_context_cases as sc

SENSITIVITY = 1e-6


def _differ(x, y):
    """told apart by the comparison of the GPU tests with three orders to spare: one of them NaN, or 1e-6 relative apart"""
    if math.isnan(x) or math.isnan(y):
        return math.isnan(x) != math.isnan(y)
    return abs(x - y) > SENSITIVITY * max(abs(x), abs(y))


@pytest.mark.parametrize("name,tile_blocks", (("w64", 0), ("mid", 1), ("big", 1)))
@pytest.mark.parametrize("pair", sc.PAIRS)
def test_windows_tell_the_constants_apart(oracle, pair, name, tile_blocks):
    kind = "big" if name == "big" else "small"
    for own, other in (pair, pair[::-1]):
        spec = sc.Spec(kind, name, own, tile_blocks=tile_blocks)
        right, wrong = sc.d_with_n(spec, own), sc.d_with_n(spec, other)
        want = [r["tajima_d"] for r in sc.want(spec)]
        assert all((math.isnan(a) and math.isnan(b)) or a == b for a, b in zip(right, want)), (pair, own, right[:3], want[:3])
        n_win = len(right)
        if own == 2:
            assert all(math.isnan(d) for d in right), (pair, own, right[:3])
            assert 2 * sum(math.isfinite(d) for d in wrong) >= n_win, (pair, own, wrong[:3])
            continue
        finite = [i for i in range(n_win) if math.isfinite(right[i])]
        assert 2 * len(finite) >= n_win, (pair, own, name, len(finite), n_win)
        for i in finite:
            assert _differ(right[i], wrong[i]), (pair, own, name, i, right[i], wrong[i])


def test_a_subset_of_one_has_no_d_and_takes_the_constants_of_two(oracle):
    """|P| = 1: D is NaN whatever the constants; a plan of 40 that read that plan's constants (those of n = 2) would lose
    its finite D"""
    one = sc.Spec("small", "w64", 1)
    assert all(math.isnan(r["tajima_d"]) for r in sc.want(one))
    forty = sc.Spec("small", "w64", 40)
    right, wrong = sc.d_with_n(forty, 40), sc.d_with_n(forty, 1)
    assert all(math.isfinite(d) for d in right) and all(math.isnan(d) for d in wrong)


def test_shapes_reach_the_three_finalize_variants():
    """what the docstring of the cases says of the lists: at most two blocks a window; more than 48 and more than 2 048 blocks"""
    assert len(sc.WINDOWS["w64"]) == 64
    for s0, s1, _ in sc.WINDOWS["w64"]:
        assert s1 - s0 == 50 and (s1 - 1) // 64 - s0 // 64 <= 1 and s1 <= sc.S_SMALL
    (s0, s1, _), = sc.WINDOWS["mid"]
    assert 48 < (s1 - s0) // 64 and (s1 - s0 + 63) // 64 + 1 <= 2048 and s1 <= sc.S_SMALL
    (s0, s1, _), = sc.WINDOWS["big"]
    assert (s1 - s0) // 64 > 2048 and s1 <= sc.S_BIG
    assert all(s1 <= sc.S_SMALL for _, s1, _ in sc.WINDOWS["pw"]) and all(s1 <= sc.K_NODES for _, s1, _ in sc.WINDOWS["nodes"])
