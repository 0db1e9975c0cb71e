"""The scans added after test_gpu_upper_range.py, at the upper end of their haplotype range (run with -m gpu on an MI355X).

  impop_dstat_scan, impop_sfs_scan     n_hap = 8191, 16385, 65535 with K populations scattered over the matrix: the general granule
                                       loop of pop_stream_tile (Gf > 4) in the sfs kernels, more than 48 KiB of mask LDS at K = 8,
                                       rare entries that name haplotypes 65533 and 65534, products of two counts next to 2^30,
                                       c^2 = 65534^2, sums next to the 2^62 admission bound
  impop_sfs_scan's table pass          exactly 160 KiB of dynamic LDS, the first job one bin over, a spectrum of 65536 bins
  impop_haplotype_scan, impop_ld_scan, impop_diploid_scan, impop_ibs_scan, impop_ehh_scan
                                       130 / 465 members scattered over a 65535-haplotype matrix (wps = 2048): the same bytes as
                                       the members' rows uploaded alone

The inputs are tests/wide_cases.py (kept from being hollow by tests/test_wide_cases_host.py), the references the plain restatements
each call's own test file uses.  Every value is an exact integer or a double formed on the host from exact integers in a fixed
order: every comparison is exact."""
import functools
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import dip_cases as dipc
import hap_cases as hc
import ibs_cases as ic
import ld_cases as lc
import plain_diploid as pdip
import plain_dstat as pd
import plain_ibs as pi
import plain_sfs as ps
import wide_cases as wc
from conftest import ROOT
from test_gpu_upper_range import KINDS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
E_UNSUPPORTED = -5
BOTH = ("sfs", "jsfs")
OG = wc.WIDE_OUTGROUP
N_WIDE = 65535


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    assert c.device_name().startswith("gfx950")
    yield c
    c.close()


def masks(pops, n):
    return [wc.flags_of(p, n) for p in pops]


def same_bytes(a, b):
    """two sfs_scan results: the same bytes in the records and in every table"""
    if a[0].tobytes() != b[0].tobytes() or a[1].tobytes() != b[1].tobytes():
        return False
    for x, y in ((a[2], b[2]), (a[3], b[3])):
        if (x is None) != (y is None) or (x is not None and any(p.shape != q.shape or (p != q).any() for p, q in zip(x, y))):
            return False
    return True


# ---- a., b.  K populations scattered over a wide matrix ----------------------------------------------------------------------------

def site_weights(S):
    return (np.arange(S) % 3 + 1).astype(np.uint32)


class WidePops:
    """one wide_pop_case on the device: the three uploads of KINDS, compact() of the first, and a weighted twin"""

    def __init__(self, ctx, n, K):
        import impop_amd
        self.n, self.K = n, K
        self.m, self.pops, self.wins = wc.wide_pop_case(n, K, n + K)
        self.counts = wc.pop_counts(self.m, self.pops)
        self.masks = masks(self.pops, n)
        S = self.m.shape[1]
        bits = impop_amd.pack_hap_major(self.m)
        self.ups = [ctx.upload(bits, S, keep_hap_major=False, **kw) for kw in KINDS]
        self.ups.append(self.ups[0].compact())
        self.weights = site_weights(S)
        self.weighted = ctx.upload(bits, S, keep_hap_major=False)
        self.weighted.set_site_weights(self.weights)
        info = {**self.ups[0].scan_index_info(), **self.ups[0].scan_split_info()}
        assert info["why"] == "" and info["n_rare"] > 100 and info["n_common"] > 100, info
        assert self.ups[1].scan_split_info()["n_rare"] == 0 and self.ups[2].scan_index_info()["n_kept"] == 0
        self.wps4 = ((n + 31) // 32 + 3) // 4 * 4

    @functools.lru_cache(maxsize=None)
    def dstat_ref(self, polarize, weighted):
        return pd.reference(None, self.pops, wc.wide_quartets(self.K), self.wins, polarize, self.weights if weighted else None, self.counts)

    @functools.lru_cache(maxsize=None)
    def sfs_ref(self, pairs, og, weighted):
        return ps.reference(None, self.pops, list(pairs), self.wins, og, self.weights if weighted else None, self.counts)

    def free(self):
        for x in self.ups + [self.weighted]:
            x.free()


@pytest.fixture(scope="module")
def wide(ctx):
    made = {}

    def get(n, K):
        if (n, K) not in made:
            made[(n, K)] = WidePops(ctx, n, K)
        return made[(n, K)]

    yield get
    for w in made.values():
        w.free()


def pop_counts_of(n):
    return (4, 8) if n == N_WIDE else (4,)


@pytest.mark.parametrize("n", wc.WIDE_N)
def test_dstat_wide(wide, n):
    """pop_stream_tile's general granule loop under dstat_tiles_kernel at n > 512 on every route, rare entries listing 0, 31, 32,
    n - 2 and n - 1 against K masks in LDS, and at K = 8 and n = 65535 64 KiB of mask LDS (the opt-in above 48 KiB)"""
    from impop_amd import _lib
    for K in pop_counts_of(n):
        w = wide(n, K)
        quartets = wc.wide_quartets(K)
        assert len(quartets) > _lib.DSTAT_GROUP
        if K == 8:
            assert K * w.wps4 * 4 > 48 * 1024
        for polarize in (False, True):
            outs = [u.dstat_scan(w.wins, w.masks, quartets, polarize=polarize) for u in w.ups]
            for o in outs[1:]:
                assert o.tobytes() == outs[0].tobytes(), (n, K, polarize)
            pd.assert_matches(outs[0], w.dstat_ref(polarize, False), (n, K, polarize))
            got = w.weighted.dstat_scan(w.wins, w.masks, quartets, polarize=polarize)
            pd.assert_matches(got, w.dstat_ref(polarize, True), (n, K, polarize, "weighted"))


@pytest.mark.parametrize("n", wc.WIDE_N)
def test_sfs_wide(wide, n):
    """Gf > 4 in sfs_tiles_kernel and in sfs_table_kernel (the spectra and the joint tables, LDS form), the rare entries next to
    the sentinel, more than 48 KiB of mask LDS at K = 8, pairs beyond one group; tiles of one block and chunks of one window"""
    from impop_amd import _lib
    for K in pop_counts_of(n):
        w = wide(n, K)
        pairs = tuple(wc.wide_pairs(K))
        assert len(pairs) > _lib.SFS_PAIR_GROUP
        # K = 8: all 28 pairs as records; the tables of five pairs of the moderate populations and of the one-haplotype one
        tab_pairs = pairs if K == 4 else ((1, 3), (3, 7), (5, 7), (1, 5), (7, 4))
        if K == 8:
            assert K * w.wps4 * 4 > 48 * 1024
        for og in (None, OG):
            if K == 8:
                outs = [u.sfs_scan(w.wins, w.masks, pairs, outgroup=og) for u in w.ups]
                for o in outs[1:]:
                    assert same_bytes(o, outs[0]), (n, K, og)
                ps.assert_matches(outs[0], w.sfs_ref(pairs, og, False), (n, K, og, "records"))
            outs = [u.sfs_scan(w.wins, w.masks, tab_pairs, outgroup=og, tables=BOTH) for u in (w.ups if K == 4 else w.ups[:1])]
            for o in outs[1:]:
                assert same_bytes(o, outs[0]), (n, K, og)
            ps.assert_matches(outs[0], w.sfs_ref(tab_pairs, og, False), (n, K, og))
            got = w.weighted.sfs_scan(w.wins, w.masks, tab_pairs, outgroup=og, tables=BOTH)
            ps.assert_matches(got, w.sfs_ref(tab_pairs, og, True), (n, K, og, "weighted"))
        for kw in ({"tile_blocks": 1}, {"max_chunk_bytes": 1}):
            assert same_bytes(w.ups[0].sfs_scan(w.wins, w.masks, tab_pairs, outgroup=OG, tables=BOTH, **kw), outs[0]), (n, K, kw)


# ---- c.  32-bit products next to 2^30 ----------------------------------------------------------------------------------------------

def test_dstat_extreme_products(ctx):
    """populations of 32766, 32766, 2 and 1: c1 n2, c2 n1, (n1 - c1) c2, c2 n3 and c3 n2 above 2^29, x of both signs above 2^29 in
    magnitude, both donors of Martin's denominator (wide_cases.extreme_quartet_case asserts it)"""
    m, pops, quartets, wins = wc.extreme_quartet_case()
    n = m.shape[0]
    counts = wc.pop_counts(m, pops)
    mk = masks(pops, n)
    ups = [ctx.upload_dense(m, keep_hap_major=False, **kw) for kw in ({"dense_scan": True}, {})]
    assert ups[0].scan_index_info()["n_kept"] == 0 and ups[1].scan_index_info()["why"] == "" and ups[1].scan_split_info()["n_rare"] > 0
    for polarize in (False, True):
        want = pd.reference(None, pops, quartets, wins, polarize, counts=counts)
        for u, tag in zip(ups, ("dense", "indexed")):
            pd.assert_matches(u.dstat_scan(wins, mk, quartets, polarize=polarize), want, (tag, polarize))
    for u in ups:
        u.free()


# ---- d.  admitted just below the overflow bound --------------------------------------------------------------------------------------

def _refused(fn):
    from impop_amd import ImpopError
    with pytest.raises(ImpopError) as ei:
        fn()
    assert ei.value.code == E_UNSUPPORTED and "2^62" in str(ei.value)


def test_admitted_just_below_the_overflow_bound_dstat(ctx):
    """four populations of about 16000 haplotypes: the rule n1 nO max(n2, n3)^2 W < 2^62 admits W = 70 and refuses 71.  Nearly all
    of the weight lies on a column with c = (0, n2, n3, 0), so abba = (W - 2) n1 n2 n3 nO is within a factor of four of 2^62."""
    n = N_WIDE
    sizes = (16001, 16000, 15999, 16002)
    edges = np.concatenate([[0], np.cumsum(sizes)])
    order = np.random.default_rng(62).permutation(n)
    pops = [sorted(int(x) for x in order[edges[k]:edges[k + 1]]) for k in range(4)]
    W = wc.dstat_w_limit(sizes) - 1
    t = sizes[0] * sizes[3] * max(sizes[1], sizes[2]) ** 2
    assert t * W < 2 ** 62 <= t * (W + 1) and W > 8
    m = np.zeros((n, 3), np.uint8)
    m[pops[1], 0] = m[pops[2], 0] = 1          # ABBA at its largest
    m[pops[0], 1] = m[pops[2], 1] = 1          # BABA at its largest
    m[:, 2] = np.random.default_rng(63).random(n) < 0.5
    wt = np.array([W - 2, 1, 1], dtype=np.uint32)
    mk = masks(pops, n)
    bm = ctx.upload_dense(m, keep_hap_major=False)
    bm.set_site_weights(wt)
    for polarize in (False, True):
        want = pd.reference(None, pops, [(0, 1, 2, 3)], [(0, 3)], polarize, wt, wc.pop_counts(m, pops))
        assert 4 * int(want["abba"][0, 0]) > 2 ** 62 > int(want["abba"][0, 0])
        assert int(want["abba"][0, 0]) >= (W - 2) * sizes[0] * sizes[1] * sizes[2] * sizes[3]
        pd.assert_matches(bm.dstat_scan([(0, 3)], mk, [(0, 1, 2, 3)], polarize=polarize), want, ("admitted", polarize))
    wt[0] += 1
    bm.set_site_weights(wt)
    _refused(lambda: bm.dstat_scan([(0, 3)], mk, [(0, 1, 2, 3)]))
    bm.free()


def test_admitted_just_below_the_overflow_bound_sfs(ctx):
    """all 65535 haplotypes as one population: n^2 W < 2^62 admits W = 1073774592 and refuses one more.  Nearly all of the weight lies
    on a column with c = 65534, so sum_c2 = (W - 2) 65534^2 + ... is within a factor of four of 2^62."""
    n = N_WIDE
    W = wc.sfs_w_limit(n) - 1
    assert n * n * W < 2 ** 62 <= n * n * (W + 1) and W < 2 ** 32
    rng = np.random.default_rng(64)
    m = np.ones((n, 3), np.uint8)
    m[40000, 0] = 0
    m[:, 1] = 0
    m[n - 2, 1] = 1
    m[:, 2] = rng.random(n) < 0.5
    pops = [list(range(n)), sorted(int(x) for x in rng.permutation(n)[:500])]
    wt = np.array([W - 2, 1, 1], dtype=np.uint32)
    mk = masks(pops, n)
    bm = ctx.upload_dense(m, keep_hap_major=False)
    bm.set_site_weights(wt)
    want = ps.reference(None, pops, [], [(0, 3)], None, wt, wc.pop_counts(m, pops))
    assert 4 * int(want[0]["sum_c2"][0, 0]) > 2 ** 62 > int(want[0]["sum_c2"][0, 0]) >= (W - 2) * 65534 ** 2
    got = bm.sfs_scan([(0, 3)], mk)
    ps.assert_matches(got, want, "admitted")
    assert int(got[0]["n_sites"][0, 0]) == W
    wt[0] += 1
    bm.set_site_weights(wt)
    _refused(lambda: bm.sfs_scan([(0, 3)], mk))
    bm.free()


# ---- e.  the table pass at its natural LDS cap, in a child process under IMPOP_TRACE=1 ------------------------------------------------

JOINT_N = 8191


def _joint_case():
    m, _, wins = wc.wide_pop_case(JOINT_N, 4, JOINT_N + 4)
    pops, at, over = wc.joint_cap_pops(JOINT_N, np.random.default_rng(JOINT_N))
    return m, pops, at, over, wins


def _child(out_path):
    import impop_amd
    ctx = impop_amd.Context(0)
    out = {}

    def call(tag, fn):
        sys.stderr.write(f"@@call {tag}\n")
        sys.stderr.flush()
        st, _, sfs, jsfs = fn()
        out[f"{tag}:stats"] = st
        for i, t in enumerate((sfs or []) + (jsfs or [])):
            out[f"{tag}:t{i}"] = t
        sys.stderr.flush()

    m, pops, _, wins = wc.big_sfs_case()
    bm = ctx.upload_dense(m, keep_hap_major=False)
    call("big", lambda: bm.sfs_scan(wins, masks(pops, m.shape[0]), tables=("sfs",)))
    bm.free()
    m, pops, at, over, wins = _joint_case()
    bm = ctx.upload_dense(m, keep_hap_major=False)
    mk = masks(pops, JOINT_N)
    call("joint_at", lambda: bm.sfs_scan(wins, [mk[at[0]], mk[at[1]]], [(0, 1)], tables=("jsfs",)))
    call("joint_over", lambda: bm.sfs_scan(wins, [mk[over[0]], mk[over[1]]], [(0, 1)], tables=("jsfs",)))
    bm.free()
    ctx.close()
    np.savez(out_path, **out)


_TRACE = re.compile(r"\[impop_sfs_scan\] (.*)$")


def test_sfs_tables_at_the_natural_lds_cap():
    """BIG's spectrum has exactly the bins the LDS holds next to one mask of 2048 dwords (a launch with 163840 bytes of dynamic
    LDS), BIG1's one more (the global form), ALL's 65536; then a joint table of 128 x 316 bins next to two masks of 256 dwords,
    and one of 128 x 317.  IMPOP_SFS_LDS_BINS is not set: the sizes alone choose the form."""
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "r.npz")
        env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, HERE]))
        for k in ("IMPOP_SFS_LDS_BINS", "IMPOP_SFS_TILE_BLOCKS"):
            env.pop(k, None)
        r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_upper_range_scans as t; t._child(sys.argv[1])", path],
                           capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-4000:]
        z = np.load(path)
        recs = {k: z[k] for k in z.files}
    trace, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@@call "):
            cur = line.split()[1]
            trace[cur] = []
            continue
        mt = _TRACE.search(line)
        if mt and cur:
            kv = dict(x.split("=") for x in mt.group(1).split())
            trace[cur].append({k: (v if k == "route" else int(v)) for k, v in kv.items()})
    # one population per job: BIG at the cap, BIG1 and ALL over it, the three small ones far below
    m, pops, _, wins = wc.big_sfs_case()
    cap = wc.sfs_lds_bins(1, m.shape[0])
    assert [len(p) + 1 for p in pops[:3]] == [m.shape[0] + 1, cap, cap + 1] and 8192 + 4 * cap == wc.SFS_LDS_BYTES
    (line,) = trace["big"]
    print("big:", line)
    assert line["table_jobs"] == 6 and line["lds_jobs"] == sum(len(p) + 1 <= cap for p in pops) == 4
    want = ps.reference(None, pops, [], wins, None, counts=wc.pop_counts(m, pops))
    ps.assert_records(recs["big:stats"], want[0], "big")
    for k in range(len(pops)):
        assert recs[f"big:t{k}"].shape == want[2][k].shape and (recs[f"big:t{k}"] == want[2][k]).all(), k
    assert want[2][1][0].sum() > 20 and want[2][0][0, 1] > 0 and want[2][0][0, m.shape[0] - 1] > 0
    # a joint job of two populations
    m, pops, at, over, wins = _joint_case()
    cap2 = wc.sfs_lds_bins(2, JOINT_N)
    counts = wc.pop_counts(m, pops)
    for tag, pr, lds in (("joint_at", at, 1), ("joint_over", over, 0)):
        two = [pops[pr[0]], pops[pr[1]]]
        bins = (len(two[0]) + 1) * (len(two[1]) + 1)
        assert (bins == cap2) == bool(lds) and bins - cap2 in (0, len(two[0]) + 1)
        (line,) = trace[tag]
        print(tag + ":", line)
        assert line["table_jobs"] == 1 and line["lds_jobs"] == lds, (tag, line)
        want = ps.reference(None, two, [(0, 1)], wins, None, counts=[counts[pr[0]], counts[pr[1]]])
        ps.assert_records(recs[f"{tag}:stats"], want[0], tag)
        assert recs[f"{tag}:t0"].shape == want[3][0].shape and (recs[f"{tag}:t0"] == want[3][0]).all(), tag
        assert (want[3][0][3] > 0).sum() > 50  # the whole matrix: many distinct joint cells


# ---- f.  a small member set scattered over a 65535-haplotype matrix -------------------------------------------------------------------

MEMBER_COUNTS = (130, 465)
SCATTER_S = 1200
CALLS = ("haplotype_scan", "ld_scan", "diploid_scan", "ibs_scan_all_pairs", "ibs_scan_list", "ehh_scan")
EHH_WINDOWS = [(64, 664), (37, 166), (100, 165), (590, 654), (0, 63), (600, 601), (200, 1190)]
EHH_CORES = [300, 100, 164, 600, 0, 600, 700]


def member_matrix(call, nm):
    """each call's own small generator, with few enough variable sites that the wide matrix still gets its index"""
    rng = np.random.default_rng(70000 + nm + 7 * CALLS.index(call))
    if call == "haplotype_scan":
        return hc.founder_matrix(rng, nm, SCATTER_S, p_site=0.08, p_flip=1e-4)
    if call == "ld_scan":
        return lc.planted_matrix(rng, nm, SCATTER_S, p_site=0.08, p_flip=1e-4)
    if call == "diploid_scan":
        return dipc.founder_matrix(rng, nm, SCATTER_S, nf=4, p_switch=0.004, p_flip=1e-4, p_site=0.035)
    if call.startswith("ibs_scan"):
        m = dipc.founder_matrix(rng, nm, SCATTER_S, nf=3, p_switch=0.004, p_flip=1e-4, p_site=0.035)
        m[nm - 1] = m[0]
        m[nm - 1, ::40] ^= 1  # a pair without a tract of 60 sites
        return m
    import test_gpu_ehh_scan as tes
    m = tes._founders(rng, nm, SCATTER_S, pp=1e-4)
    m[:, 600] = rng.integers(0, 2, size=nm)  # a core that splits the members in two large halves
    return m


def scan_windows():
    S = SCATTER_S
    w = [(37, 517), (64, 128), (100, 101), (200, 200), hc.MONO, (0, S), (S - 1, S), (63, 65), (0, 0), (S, S)]
    return w + [(b, min(b + 640, S)) for b in range(0, S - 320, 320)]


class Scattered:
    def __init__(self, ctx, call, nm):
        import impop_amd
        self.wide, self.pos = wc.scatter(member_matrix(call, nm), N_WIDE, 100 * nm + CALLS.index(call))
        self.alone_m = np.ascontiguousarray(self.wide[self.pos])
        self.flags = wc.flags_of(self.pos, N_WIDE)
        bits = impop_amd.pack_hap_major(self.wide)
        self.ups = [ctx.upload(bits, SCATTER_S, keep_hap_major=False, **kw) for kw in KINDS]
        self.alone = ctx.upload_dense(self.alone_m, keep_hap_major=False)
        info = {**self.ups[0].scan_index_info(), **self.ups[0].scan_split_info()}
        assert info["why"] == "" and 0 < info["n_kept"] <= SCATTER_S // 4 and info["n_rare"] >= 20 and info["n_common"] >= 20, info
        assert self.ups[1].scan_index_info()["n_kept"] == info["n_kept"] and self.ups[1].scan_split_info()["n_rare"] == 0
        assert self.ups[2].scan_index_info()["n_kept"] == 0

    def free(self):
        for x in self.ups + [self.alone]:
            x.free()


def flat(res):
    """a call's result as a list of arrays"""
    return [a for a in (res if isinstance(res, tuple) else (res,)) if isinstance(a, np.ndarray)]


def assert_same_bytes(a, b, where):
    a, b = flat(a), flat(b)
    assert len(a) == len(b), where
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (where, i)


def mapped(res, pos, fields=("h1", "h2")):
    """the records of an ibs_scan on the members' own matrix with their haplotype indices as the wide matrix numbers them (the
    other calls' records carry no haplotype index: ehh_scan's ref_hap is an argument, haplotype_scan's h1 a statistic)"""
    out = []
    for a in flat(res):
        a = a.copy()
        for f in fields:
            if a.dtype.names and f in a.dtype.names:
                a[f] = pos[a[f]]
        out.append(a)
    return tuple(out)


@pytest.mark.parametrize("call", CALLS)
def test_members_scattered_over_a_wide_matrix(ctx, call):
    """hap_block_words, hap_rare_members and ibs_transpose_kernel find the members through ppos / pmask over wps = 2048 dword
    columns (n_pad = 65536), most of them skipped and some with one member; rare entries list one member next to decoys"""
    for nm in MEMBER_COUNTS:
        sc = Scattered(ctx, call, nm)
        try:
            _scattered(sc, call, nm)
        finally:
            sc.free()


def _scattered(sc, call, nm):
    pos, loc = sc.pos, sc.alone_m
    if call == "haplotype_scan":
        wins = scan_windows()
        run = lambda u, **kw: u.haplotype_scan(wins, mask_p=sc.flags, want_members=True, **kw)
        alone = sc.alone.haplotype_scan(wins, want_members=True)
        check = lambda got: hc.assert_matches(got, hc.reference(loc, None, wins), (call, nm))
    elif call == "ld_scan":
        lc.check_planted(member_matrix(call, nm))  # before scatter plants rare variants in the stretch around them
        wins = scan_windows() + lc.PLANT_WINDOWS
        run = lambda u, **kw: u.ld_scan(wins, mask_p=sc.flags, min_mac=2, max_sites=256, want_sites=True, **kw)
        alone = sc.alone.ld_scan(wins, min_mac=2, max_sites=256, want_sites=True)
        check = lambda got: lc.assert_matches(got, lc.reference(loc, None, wins, 2, 256), (call, nm))
    elif call == "diploid_scan":
        N, min_run = nm // 2, 40
        assert N in (65, 232)
        local = [(i, i + N) if i % 2 == 0 else (i + N, i) for i in range(N)]  # the two copies far apart in the wide matrix
        pairs = [(int(pos[a]), int(pos[b])) for a, b in local]
        assert min(abs(a - b) for a, b in pairs) > 4096
        wins = dipc.window_list(SCATTER_S)
        run = lambda u, **kw: u.diploid_scan(wins, pairs, min_run, want_individuals=True, **kw)
        alone = sc.alone.diploid_scan(wins, local, min_run, want_individuals=True)
        want = pdip.reference(loc, local, wins, min_run)
        dipc.assert_nontrivial(want[1], (call, nm))
        check = lambda got: pdip.assert_matches(got, want, (call, nm))
    elif call.startswith("ibs_scan"):
        b, e, min_sites = 5, SCATTER_S - 7, 60
        wins = ic.window_list(b, e)
        if call == "ibs_scan_all_pairs":
            local = pi.all_pairs(range(nm))
            kw0 = dict(mask_p=sc.flags)
            alone = sc.alone.ibs_scan(min_sites=min_sites, site_begin=b, site_end=e, windows=wins)[:3]
        else:
            rng = np.random.default_rng(nm)
            local = [(0, nm - 1), (nm - 1, 0), (0, nm - 1), (3, 4)] + [(int(x), int(y)) for x, y in rng.integers(0, nm, size=(700, 2)) if x != y]
            kw0 = dict(pairs=[(int(pos[a]), int(pos[c])) for a, c in local])
            alone = sc.alone.ibs_scan(pairs=local, min_sites=min_sites, site_begin=b, site_end=e, windows=wins)[:3]
        run = lambda u, **kw: u.ibs_scan(min_sites=min_sites, site_begin=b, site_end=e, windows=wins, **kw0, **kw)[:3]
        if len(local) <= 10000:
            want = mapped(pi.reference(loc, local, b, e, min_sites, wins), pos)
            ic.assert_nontrivial(want[0], (call, nm))
            check = lambda got: pi.assert_matches(got, want, (call, nm))
        else:
            # 107880 pairs: the restatement's pair loop would take seven seconds, so it is run on 3000 of them, drawn at random
            # (like test_gpu_ibs_scan.test_4096_haplotypes_all_pairs); every pair, segment and window record is still held to the
            # members' own upload below, byte for byte
            pick = np.sort(np.random.default_rng(nm).choice(len(local), size=3000, replace=False))
            pick[0], pick[-1] = 0, len(local) - 1
            want = mapped(pi.reference(loc, [local[p] for p in pick], b, e, min_sites), pos)
            ic.assert_nontrivial(want[0], (call, nm))

            def check(got):
                rec, seg, _ = got
                assert len(rec) == len(local) and len(seg) == int(rec["n_tracts"].sum(dtype=np.int64))
                off = np.concatenate([[0], np.cumsum(rec["n_tracts"], dtype=np.int64)])
                pi.assert_same(rec[pick].copy(), want[0], (call, nm, "pairs"))
                w_seg = want[1].copy()
                w_seg["pair"] = pick[w_seg["pair"]]
                pi.assert_same(np.concatenate([seg[off[p]:off[p + 1]] for p in pick]), w_seg, (call, nm, "segments"))
    else:
        import test_gpu_ehh_scan as tes
        ref_local = nm // 2
        cache = {}

        def run(u, **kw):
            return tuple(u.ehh_scan(EHH_WINDOWS, EHH_CORES, mask=sc.flags, ref_hap=int(pos[ref_local]), flanks=f, **kw) for f in ("reference", "two-sided"))

        alone = tuple(sc.alone.ehh_scan(EHH_WINDOWS, EHH_CORES, ref_hap=ref_local, flanks=f) for f in ("reference", "two-sided"))

        def check(got):
            for rec, f in zip(got, ("reference", "two-sided")):
                tes.check_records(rec, loc, None, EHH_WINDOWS, EHH_CORES, f, ref_local, cache, (call, nm))
            assert got[0]["n_members"][3].min() > nm // 4
    outs = [run(u) for u in sc.ups]
    check(outs[0])
    for o in outs[1:]:
        assert_same_bytes(o, outs[0], (call, nm, "routes"))
    assert_same_bytes(outs[0], mapped(alone, pos) if call.startswith("ibs_scan") else alone, (call, nm, "alone"))
    # chunks of one window; impop_ibs_scan sweeps the whole range once per budget of segments, so a budget of one byte would be a
    # sweep per tract: it gets five blocks of words, as in test_gpu_ibs_scan.py (four site chunks, hundreds of pair ranges)
    budget = 2 * 5 * nm * 8 if call.startswith("ibs_scan") else 1
    assert_same_bytes(run(sc.ups[0], max_chunk_bytes=budget), outs[0], (call, nm, "chunked"))
