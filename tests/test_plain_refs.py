"""tests/plain_refs.py against what already pins the semantics: the reference goldens and the C oracle, on a few hundred small
random shapes, all exact.  No GPU: this is what makes the plain references fit to judge the kernels at sizes the oracle
cannot reach (tests/test_gpu_upper_range.py)."""
import math

import numpy as np

import plain_refs as pr
from conftest import fh, golden_bits, load_golden


def _dense_from_rows(rows, names):
    ix = {s: i for i, s in enumerate(names)}
    sim = np.full((len(names), len(names)), np.nan)
    for a, b, v in rows:
        sim[ix[a], ix[b]] = sim[ix[b], ix[a]] = v
    return sim


def _clusters(cl, K, names):
    return [sorted(names[i] for i in range(len(names)) if cl[i] == k) for k in range(K)]


def _unpack(bits, W):
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8), axis=1, bitorder="little")[:, :W]


def test_components_reference_goldens(oracle):
    g = load_golden("six_seq.json")
    rows = [(a, b, fh(v)) for a, b, v in g["rows"]]
    names = sorted({r[0] for r in rows} | {r[1] for r in rows})
    sim = _dense_from_rows(rows, names)
    np.fill_diagonal(sim, np.nan)
    assert g["af"]
    for c in g["af"]:
        cl, K, sz = pr.ref_components(pr.adjacency(sim, fh(c["threshold"])))
        assert _clusters(cl, K, names) == c["clusters"]
        assert sz.tolist() == [len(x) for x in c["clusters"]]
        # one orientation of every pair is enough, whichever it is
        for tri in (np.triu, np.tril):
            one = np.where(tri(np.ones_like(sim, dtype=bool), 0), sim, np.nan)
            cl1, K1, _ = pr.ref_components(pr.adjacency(one, fh(c["threshold"])))
            assert _clusters(cl1, K1, names) == c["clusters"]
            ocl, oK, _ = oracle.af_cluster(one, fh(c["threshold"]))
            assert _clusters(ocl, oK, names) == c["clusters"]
    b = load_golden("bitmatrix.json")
    seen = 0
    for m in b["matrices"]:
        n, W = m["n"], m["W"]
        I = oracle.pairwise_counts(golden_bits(m), n, 0, W)
        trunc = [s.split(":", 1)[0] for s in m["names"]]
        for kind, kid in (("match", 0), ("dice", 1)):
            sim = oracle.identity(I, W, kid)
            for c in m["kinds"][kind]["af"]:
                cl, K, _ = pr.ref_components(pr.adjacency(sim, fh(c["threshold"])))
                assert _clusters(cl, K, trunc) == c["clusters"]
                seen += 1
    assert seen > 0


def test_components_random_against_oracle(oracle):
    rng = np.random.default_rng(11)
    for trial in range(300):
        n = int(rng.integers(1, 81))
        t = np.round(rng.random((n, n)), 2)
        t = np.minimum(t, t.T) if trial % 3 else t  # every third table is asymmetric: either orientation links
        t[rng.random((n, n)) < 0.2] = np.nan
        thr = float(rng.choice([0.5, 0.8, 0.9, 0.97, 0.99, 1.01]))
        if trial % 5 == 0:  # equal-sized clusters under permuted labels: the tie-break by smallest member
            k = max(n // 4, 1)
            lab = rng.permutation(n) % k
            t = np.where(lab[:, None] == lab[None, :], 1.0, 0.0)
            thr = 1.0
        cl, K, sz = pr.ref_components(pr.adjacency(t, thr))
        ocl, oK, osz = oracle.af_cluster(t, thr)
        assert K == oK and cl.tolist() == ocl.tolist() and sz.tolist() == osz.tolist(), (trial, n, thr)
        assert sz.sum() == n and (np.diff(sz) <= 0).all()


def test_ehh_reference_goldens():
    g = load_golden("ehh.json")
    assert g["calc"]
    for c in g["calc"]:
        m01 = np.array([[int(ch) for ch in r] for r in c["rows"]], dtype=np.uint8)
        assert pr.ref_ehh(m01) == [fh(v) for v in c["fwd"]]
        assert pr.ref_ehh(m01, None, True) == [fh(v) for v in c["rev"]]


def test_ehh_random_against_oracle(oracle):
    rng = np.random.default_rng(12)
    for trial in range(200):
        n, W = int(rng.integers(1, 81)), int(rng.integers(1, 301))
        nf = int(rng.integers(1, 6))
        founders = (rng.random((nf, W)) < 0.3).astype(np.uint8)
        m01 = founders[rng.integers(0, nf, n)] ^ (rng.random((n, W)) < 0.01).astype(np.uint8)
        bits = oracle.pack_hap_major(m01)
        s0 = int(rng.integers(0, W))
        s1 = int(rng.integers(s0 + 1, W + 1))
        mem = None if trial % 3 == 0 else (rng.random(n) < (0.6 if trial % 3 == 1 else 0.05)).astype(np.uint8)
        for rev in (False, True):
            want = oracle.ehh(bits, n, s0, s1, mem, rev).tolist()
            assert pr.ref_ehh(m01[:, s0:s1], mem, rev) == want, (trial, n, W, s0, s1, rev)


def test_counts_and_afs_reference_golden(tmp_path):
    from impop_amd import extract
    g = load_golden("afs_table.json")
    p = tmp_path / "paths.tsv"
    p.write_text(g["table_text"])
    mf = extract.from_paths_table(str(p), native=False)
    n, W = mf.n_hap, mf.n_site
    m01 = _unpack(mf.bits, W)
    c = pr.ref_site_counts(m01, None, 0, W)
    for k, col in enumerate(g["columns"]):
        assert (int(c[k]) if col["value"] == 1 else n - int(c[k])) == col["count"], col
    want = np.zeros(n + 1, dtype=np.int64)
    for v in g["counts_d"].get("1", []):
        want[v] += 1
    for v in g["counts_d"].get("0", []):
        want[n - v] += 1
    assert pr.ref_afs(m01, None, [(0, W)])[0].tolist() == want.tolist()


def test_scan_ints_afs_and_multi_random_against_oracle(oracle):
    rng = np.random.default_rng(13)
    for trial in range(150):
        n, W = int(rng.integers(2, 81)), int(rng.integers(1, 301))
        m01 = (rng.random((n, W)) < rng.beta(0.3, 1.0, size=W)[None, :]).astype(np.uint8)
        m01[:, rng.random(W) < 0.2] = 0
        m01[:, rng.random(W) < 0.1] = 1
        bits = oracle.pack_hap_major(m01)
        P = None if trial % 2 else (rng.random(n) < 0.6).astype(np.uint8)
        A = (rng.random(n) < 0.5).astype(np.uint8)
        B = (rng.random(n) < 0.5).astype(np.uint8)  # overlaps A: the overlap leaves both
        wins = [(0, W)]
        for _ in range(3):
            s0 = int(rng.integers(0, W + 1))
            wins.append((s0, int(rng.integers(s0, W + 1))))
        got = pr.ref_scan_ints(m01, P, A, B, wins)
        ov = A & B
        fP = np.ones(n, np.uint8) if P is None else P
        for (s0, s1), r in zip(wins, got):
            for fn in (oracle.window_allpairs, oracle.window_sitecount):
                want = fn(bits, n, s0, s1, oracle.pack_mask(fP), oracle.pack_mask(A & ~ov), oracle.pack_mask(B & ~ov), 0)
                for k in pr.SCAN_INT_KEYS:
                    assert r[k] == int(want[k]), (trial, fn.__name__, k, s0, s1)
        # spectrum and per-site counts: the site scan of one column says whether it segregates; c itself from the pair counts
        I = oracle.pairwise_counts(bits, n, 0, W)
        assert int(np.trace(I)) == int(pr.column_counts(m01).sum())
        sub = fP.astype(bool)
        afs = pr.ref_afs(m01, P, wins)
        for (s0, s1), row in zip(wins, afs):
            assert row.sum() == s1 - s0 and len(row) == int(sub.sum()) + 1
            assert (row * np.arange(len(row))).sum() == int(m01[sub][:, s0:s1].sum())
            for cc in (0, len(row) - 1):
                want = sum(1 for s in range(s0, s1) if int(m01[sub, s].sum()) == cc)
                assert row[cc] == want or len(row) == 1
        assert pr.ref_site_counts(m01, P, wins[1][0], wins[1][1]).tolist() == [int(m01[sub, s].sum()) for s in range(*wins[1])]
        # K disjoint populations: every pair's sums are the two-population record's sum_a / sum_b / sum_ab
        K = int(rng.integers(2, 6))
        owner = rng.integers(0, K + 1, n)  # K = unassigned
        pops = [(owner == k).astype(np.uint8) for k in range(K)]
        within, between, nk = pr.ref_multi_ints(m01, pops, wins)
        assert nk.tolist() == [int(p.sum()) for p in pops]
        p = 0
        for k in range(K):
            for l in range(k + 1, K):
                for wi, (s0, s1) in enumerate(wins):
                    want = oracle.window_sitecount(bits, n, s0, s1, oracle.pack_mask(np.ones(n, np.uint8)), oracle.pack_mask(pops[k]),
                                                   oracle.pack_mask(pops[l]), 0)
                    assert (int(within[wi, k]), int(within[wi, l]), int(between[wi, p])) == \
                        (int(want["sum_a"]), int(want["sum_b"]), int(want["sum_ab"])), (trial, k, l, wi)
                p += 1


def test_pair_terms_against_pica2(oracle):
    """Every element its own group (threshold above every value): pica2.py:154's pi is n/(n-1) * sum(2 * pair_value) over the pairs
    with data, which the oracle's restatement of the whole analysis returns.  The summation order differs, hence 1e-12."""
    rng = np.random.default_rng(14)
    for trial in range(60):
        n = int(rng.integers(2, 41))
        t = 0.9 + 0.1 * rng.random((n, n))
        t = np.minimum(t, t.T)
        hole = rng.random((n, n)) < 0.1
        t[hole | hole.T] = np.nan
        rd = [None, 4, 5][trial % 3]
        sims, vals = pr.ref_pair_terms(t, rd, np.arange(n), np.ones(n, np.uint32))
        assert len(sims) == n * (n - 1) // 2
        iu = np.triu_indices(n, 1)
        want_s = [float(v) if rd is None or v != v else round(float(v), rd) for v in t[iu]]
        assert all((a == b) or (a != a and b != b) for a, b in zip(sims.tolist(), want_s))
        ok = ~np.isnan(vals)
        pi, _, _, G = oracle.pica2(t, 1.0, None, rd)
        want = n / (n - 1) * math.fsum(2 * v for v in vals[ok]) if ok.any() else 0.0
        assert G == n and abs(pi - want) <= 1e-12 * max(abs(want), 1e-300), (trial, pi, want)
    # weights: sizes that do not sum to n, representatives in any order, the (smaller, larger) key
    t = np.array([[np.nan, 0.5, 0.25], [0.75, np.nan, np.nan], [0.125, 0.0625, np.nan]])
    sims, vals = pr.ref_pair_terms(t, None, [2, 0, 1], [3, 5, 2])
    assert sims[0] == 0.25 and sims[1] != sims[1] and sims[2] == 0.5 and vals[1] != vals[1]
    assert vals[0] == (1 - 0.25) * (3 / 10) * (5 / 10) and vals[2] == (1 - 0.5) * (5 / 10) * (2 / 10)
