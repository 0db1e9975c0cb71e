"""The event-pair timers of the batched calls on an MI355X (run with -m gpu): impop_ctx_gram_timing with its three
read-outs (gram / cluster / ehh) and impop_scan_plan_timing.  bench.py and tools/bench_*.py rely on these values.

Matrix: 65 haplotypes (wps = 3, split index on, rows padded to 96) x 4096 sites, hap-major copy kept.  Every figure is
printed before it is asserted."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu
N_HAP, N_SITE = 65, 4096
WINDOWS = [(0, 1024), (1024, 2048), (2048, 3072)]       # disjoint, 1024 sites each
CORES = [(b + e) // 2 for b, e in WINDOWS]              # central cores


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def bm(ctx):
    m = ctx.synthetic(N_HAP, N_SITE, seed=7, keep_hap_major=True)
    yield m
    m.free()


def _one_window_bytes(windows, cores, n_members):
    """|P| x blocks x 8 of the widest window: what impop_ehh_scan transposes for it with the reference flanks (core, end)"""
    blocks = [((e + 63) >> 6) - ((c + 1) >> 6) for (_, e), c in zip(windows, cores)]
    return n_members * max(blocks) * 8, blocks


def test_counts_and_reset(ctx, bm):
    ctx.gram_timing(True)
    bm.pairwise_scan(WINDOWS)
    t, k = ctx.gram_elapsed()
    print("gram after pairwise_scan:", t, k)
    assert t > 0 and k == 1
    assert ctx.cluster_elapsed() == (0.0, 0) and ctx.ehh_elapsed() == (0.0, 0)

    bm.cluster_scan(WINDOWS)
    tg, kg = ctx.gram_elapsed()
    tc, kc = ctx.cluster_elapsed()
    print("after cluster_scan: gram", tg, kg, "cluster", tc, kc)
    assert kg == 2 and tg > t and kc == 1 and tc > 0
    assert ctx.ehh_elapsed() == (0.0, 0)

    bm.ehh_scan(WINDOWS, CORES)
    te, ke = ctx.ehh_elapsed()
    print("after ehh_scan: ehh", te, ke)
    assert ke == 1 and te > 0
    assert ctx.gram_elapsed()[1] == 2 and ctx.cluster_elapsed()[1] == 1

    ctx.gram_timing(True)  # switching on again starts from zero
    assert ctx.gram_elapsed() == (0.0, 0) and ctx.cluster_elapsed() == (0.0, 0) and ctx.ehh_elapsed() == (0.0, 0)

    ctx.gram_timing(False)
    bm.pairwise_scan(WINDOWS)
    bm.cluster_scan(WINDOWS)
    bm.ehh_scan(WINDOWS, CORES)
    assert ctx.gram_elapsed() == (0.0, 0) and ctx.cluster_elapsed() == (0.0, 0) and ctx.ehh_elapsed() == (0.0, 0)


def test_ehh_chunks_grow_and_reuse_the_pool(ctx, bm):
    budget, blocks = _one_window_bytes(WINDOWS, CORES, N_HAP)
    assert len(set(blocks)) == 1  # equal windows: the budget holds exactly one of them, never two
    ctx.gram_timing(True)
    bm.ehh_scan(WINDOWS, CORES, max_chunk_bytes=budget)
    t1, k1 = ctx.ehh_elapsed()
    bm.ehh_scan(WINDOWS, CORES, max_chunk_bytes=budget)
    t2, k2 = ctx.ehh_elapsed()
    print("ehh chunks:", t1, k1, t2, k2)
    assert k1 == 3 and k2 == 6 and 0 < t1 < t2
    ctx.gram_timing(False)


def test_ehh_sum_is_the_sum_of_its_chunks(ctx, bm):
    """Three equal chunks sum to about three single-chunk calls, which is the upper bound itself; so the bound's right side is
    the largest of several single-chunk calls and its left side the smallest of several three-chunk calls.  Summing the wrong
    pairs (all six of two calls, the first start to the last stop with the host's synchronisations between, one pair
    only) still falls outside."""
    budget, _ = _one_window_bytes(WINDOWS, CORES, N_HAP)
    bm.ehh_scan(WINDOWS, CORES, max_chunk_bytes=budget)  # warm
    singles = []
    for _ in range(3):
        for w, c in zip(WINDOWS, CORES):
            ctx.gram_timing(True)
            bm.ehh_scan([w], [c], max_chunk_bytes=budget)
            t, k = ctx.ehh_elapsed()
            assert k == 1
            singles.append(t)
    totals = []
    for _ in range(3):
        ctx.gram_timing(True)
        bm.ehh_scan(WINDOWS, CORES, max_chunk_bytes=budget)
        t, k = ctx.ehh_elapsed()
        assert k == 3
        totals.append(t)
    ctx.gram_timing(False)
    largest, total = max(singles), min(totals)
    print("single-chunk ms:", singles, "three-chunk ms:", totals)
    assert largest <= total <= 3 * largest


def test_plan_timer(ctx, bm):
    p = bm.plan(WINDOWS)
    try:
        assert p.n_tiles > 0
        p.timing(True)
        p.launch()
        p.launch()
        t, k = p.elapsed()
        print("plan:", t, k)
        assert k == 2 and t > 0
        p.timing(True)
        assert p.elapsed() == (0.0, 0)
        p.timing(False)
        p.launch()
        assert p.elapsed() == (0.0, 0)
    finally:
        p.destroy()
    z = bm.plan([(0, 0), (77, 77)])  # windows of zero length: no tile, nothing to time
    try:
        assert z.n_tiles == 0
        z.timing(True)
        z.launch()
        z.launch()
        assert z.elapsed() == (0.0, 0)
    finally:
        z.destroy()


def test_a_timer_that_is_off_creates_no_event():
    """impop_debug_timer_pool_sizes: the event pools (gram, cluster, ehh, plan) of a fresh context stay empty without timing"""
    import impop_amd
    c = impop_amd.Context(0)
    try:
        m = c.synthetic(N_HAP, N_SITE, seed=7, keep_hap_major=True)
        p = m.plan(WINDOWS)
        m.pairwise_scan(WINDOWS)
        m.cluster_scan(WINDOWS)
        m.ehh_scan(WINDOWS, CORES)
        p.launch()
        p.fetch()
        sizes = (C.c_uint64 * 4)()
        impop_amd.engine.check(c._lib.impop_debug_timer_pool_sizes(c.handle, p._h, sizes))
        assert list(sizes) == [0, 0, 0, 0]
        c.gram_timing(True)
        p.timing(True)
        m.pairwise_scan(WINDOWS)
        m.cluster_scan(WINDOWS)
        m.ehh_scan(WINDOWS, CORES)
        p.launch()
        impop_amd.engine.check(c._lib.impop_debug_timer_pool_sizes(c.handle, p._h, sizes))
        assert list(sizes) == [2, 1, 1, 1]
        p.destroy()
        m.free()
    finally:
        c.close()
