"""GPU: ragged batches of `.sim` identity tables — impop_stats_from_identity_batch against the reference-captured goldens, the
single-problem entry points and the oracle; chunking; and `impop_scan.py --sim-list` against the per-file drop-in CLIs (which
tests/test_cli_dropin.py pins to the reference)."""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import ROOT, fh, load_golden, rel_close, stat_close

pytestmark = pytest.mark.gpu
SCRIPTS = os.path.join(ROOT, "scripts")
REL = 1e-9
FST_KEYS = ("fst", "pi_a", "pi_b", "pi_xy", "dxy", "da")


@pytest.fixture(scope="module")
def ctx():
    import impop_amd
    c = impop_amd.Context(0)
    yield c
    c.close()


def same_float(a, b):
    return (a != a and b != b) or a == b


def check_against_single(ctx, pr, rec, grp, thr, rd, frd, tag):
    """every field of a batch record against impop_pi_from_identity / impop_fst_from_identity on the same table"""
    sim = pr["ident"]
    pi, ps, g1, G, (sum2, npairs) = ctx.pi_from_identity(sim, thr, rd, pr.get("seq_len"), seed_rank=pr.get("seed_rank"), detail=True)
    assert int(rec["status"]) == 0 and int(rec["n_groups"]) == G and int(rec["n_pairs_with_data"]) == npairs, tag
    assert rel_close(float(rec["pi"]), pi, REL) and rel_close(float(rec["pi_site"]), ps, REL), (tag, float(rec["pi"]), pi)
    assert rel_close(float(rec["sum_2pairs"]), sum2, REL), tag
    assert grp is None or (grp == g1).all(), tag
    if pr.get("in_a") is not None:
        out, cnt = ctx.fst_from_identity(sim, pr["in_a"], pr["in_b"], pr.get("seq_len"), frd)
        assert (rec["fst_counts"] == cnt).all(), (tag, rec["fst_counts"], cnt)
        for k, key in enumerate(FST_KEYS):
            assert stat_close(key, float(rec["fst"][k]), float(out[k]), float(out[4])), (tag, key, float(rec["fst"][k]), float(out[k]))
    else:
        assert np.isnan(rec["fst"]).all() and not rec["fst_counts"].any(), tag
    if pr.get("tajima_n") is None:
        assert np.isnan(rec["tajima_d"]), tag


# ---- 1. goldens in one ragged call ------------------------------------------------------------------------------------------
def golden_tables(tmp_path):
    """name -> dict(sim, names, pica=[(thr, round, L, want pi, want pi_site or text)], hfst=[(round, L, a flags, b flags, want)])"""
    from impop_amd import simfile
    from impop_amd.popnames import expand_population
    T = {}
    g = load_golden("cli_pansn.json")
    p = tmp_path / "win8.sim"
    p.write_text(g["sim_text"])
    names, dense, _ = simfile.read_dense(str(p), "pica2")
    opt = lambda argv, f, conv: conv(argv[argv.index(f) + 1]) if f in argv else None  # noqa: E731
    pops = {"popA.txt": g["popA"], "popB.txt": g["popB"]}
    flags = {}
    for k, text in pops.items():
        mem, _ = expand_population({ln.strip() for ln in text.splitlines() if ln.strip() and ln[0] != "#"}, set(names))
        flags[k] = np.array([1 if n in mem else 0 for n in names], np.uint8)
    T["win8"] = dict(sim=dense, names=names,
                     pica=[(opt(c["argv"], "-t", float), opt(c["argv"], "-r", int), opt(c["argv"], "-l", int), None, c["stdout"].split()[0])
                           for c in g["pica2"]],
                     hfst=[(opt(c["argv"], "-r", int), opt(c["argv"], "-l", int), flags[opt(c["argv"], "-a", str)],
                            flags[opt(c["argv"], "-b", str)], c["stdout"].strip().split("\t")) for c in g["hfst"]])
    g = load_golden("six_seq.json")
    rows = [(a, b, fh(v)) for a, b, v in g["rows"]]
    names = sorted({r[0] for r in rows} | {r[1] for r in rows})
    sim = simfile.densify({((a, b) if a <= b else (b, a)): v for a, b, v in rows}, names)
    fa = np.array([1 if "popA" in s else 0 for s in names], np.uint8)
    fb = np.array([1 if "popB" in s else 0 for s in names], np.uint8)
    T["six_seq"] = dict(sim=sim, names=names, pica=[(fh(c["threshold"]), c["round"], c["L"], fh(c["pi"]), fh(c["pi_site"])) for c in g["pica2"]],
                        hfst=[(c["round"], c["L"], fa, fb, {k: fh(v) for k, v in c["out"].items()}) for c in g["hfst"]])
    rg = load_golden("ragged.json")
    names = rg["names"]
    full = np.array([[fh(v) for v in row] for row in rg["sim"]])
    d = {(names[i], names[j]): float(full[i, j]) for i in range(len(names)) for j in range(i, len(names))}
    for a, b in rg["dropped"]:
        d.pop((a, b), None)
    T["ragged"] = dict(sim=simfile.densify(d, names), names=names,
                       pica=[(fh(c["threshold"]), c["round"], c["L"], fh(c["pi"]), fh(c["pi_site"])) for c in rg["pica2"]],
                       hfst=[(None, c["L"], np.array([1 if n in c["a"] else 0 for n in names], np.uint8),
                              np.array([1 if n in c["b"] else 0 for n in names], np.uint8), {k: fh(v) for k, v in c["out"].items()})
                             for c in rg["hfst"]])
    T["empty"] = dict(sim=np.zeros((0, 0)), names=[], pica=[(1.0, None, 100, fh(rg["degenerate"]["empty"][0]), fh(rg["degenerate"]["empty"][1]))], hfst=[])
    T["single"] = dict(sim=np.ones((1, 1)), names=["x"], pica=[(1.0, None, 100, fh(rg["degenerate"]["single"][0]), fh(rg["degenerate"]["single"][1]))], hfst=[])
    return T


def test_goldens_in_one_ragged_call(ctx, tmp_path):
    T = golden_tables(tmp_path)
    seeded = load_golden("pica2_seeded.json")["tables"]
    assert [t["n"] for t in seeded] == [5, 12, 31, 36, 36]
    seeded_sim = {t["name"]: np.array([[fh(v) for v in row] for row in t["sim"]]) for t in seeded}
    pica_cfgs = {(thr, rd) for t in T.values() for thr, rd, *_ in t["pica"]}
    pica_cfgs |= {(fh(c["threshold"]), c["round"]) for t in seeded for c in t["runs"][0]["pica2"]}
    fst_rounds = sorted({rd for t in T.values() for rd, *_ in t["hfst"]}, key=lambda r: -1 if r is None else r)
    n_seeds = max(len(t["runs"]) for t in seeded)
    assert n_seeds == 40
    compared, hfst_seen = {}, set()
    for thr, rd in sorted(pica_cfgs, key=lambda c: (c[0], -1 if c[1] is None else c[1])):
        seeded_cfg = any(fh(c["threshold"]) == thr and c["round"] == rd for t in seeded for c in t["runs"][0]["pica2"])
        for si in range(n_seeds if seeded_cfg else 1):
            frd = fst_rounds[si % len(fst_rounds)]
            problems, checks = [], []
            for t in seeded:  # that hash seed's order as seed_rank; Tajima's D from the captured S
                run = t["runs"][si % len(t["runs"])]
                at = {nm: i for i, nm in enumerate(t["names"])}
                rank = np.zeros(t["n"], np.uint32)
                for k, nm in enumerate(run["order"]):
                    rank[at[nm]] = k
                case = [c for c in run["pica2"] if fh(c["threshold"]) == thr and c["round"] == rd]
                pr = dict(ident=seeded_sim[t["name"]], seq_len=t["L"], seed_rank=rank, in_a=np.array(t["in_a"], np.uint8),
                          in_b=np.array(t["in_b"], np.uint8))
                if case:
                    pr.update(tajima_n=t["n"], tajima_S=float(case[0]["S"]))
                problems.append(pr)
                checks.append((t["name"], "seeded", case[0] if case else None))
            for name, t in T.items():  # every golden case of this configuration as a problem of its own (its own L)
                pcs = [c for c in t["pica"] if (c[0], c[1]) == (thr, rd)]
                hcs = [(k, c) for k, c in enumerate(t["hfst"]) if c[0] == frd]
                for pc in pcs:
                    problems.append(dict(ident=t["sim"], seq_len=pc[2]))
                    checks.append((name, pc, None))
                for k, hc in hcs:
                    problems.append(dict(ident=t["sim"], seq_len=hc[1], in_a=hc[2], in_b=hc[3]))
                    checks.append((name, None, (k, hc)))
                if not pcs and not hcs:  # the table still takes part in every call
                    problems.append(dict(ident=t["sim"], seq_len=77))
                    checks.append((name, None, None))
            # the tables mixed with each other, not sorted by kind or size
            perm = np.random.default_rng(si).permutation(len(problems))
            problems, checks = [problems[i] for i in perm], [checks[i] for i in perm]
            recs, groups = ctx.stats_from_identity_batch(problems, thr, rd, frd)
            for pr, rec, grp, (name, pc, hc) in zip(problems, recs, groups, checks):
                tag = (name, thr, rd, frd, si)
                check_against_single(ctx, pr, rec, grp, thr, rd, frd, tag)
                if pc == "seeded":
                    c = hc
                    if c is None:
                        continue
                    assert int(rec["n_groups"]) == c["n_groups"], tag
                    assert rel_close(float(rec["pi"]), fh(c["pi"]), REL) and rel_close(float(rec["pi_site"]), fh(c["pi_site"]), REL), tag
                    assert f"{float(rec['pi_site']):.8f}" == c["pi_text"], tag
                    got, want = float(rec["tajima_d"]), fh(c["D"])
                    assert (got != got and want != want) or rel_close(got, want, REL), (tag, got, want)
                    compared[name] = compared.get(name, 0) + 1
                    continue
                if pc:
                    if pc[3] is None:  # captured CLI text
                        assert f"{float(rec['pi_site']):.8f}" == pc[4], (tag, float(rec["pi_site"]), pc[4])
                    else:
                        assert rel_close(float(rec["pi"]), pc[3], REL) and rel_close(float(rec["pi_site"]), pc[4], REL), tag
                    compared[name] = compared.get(name, 0) + 1
                if hc:
                    k_case, hc = hc
                    want = hc[4]
                    if isinstance(want, list):
                        assert [f"{float(v):.8f}" for v in rec["fst"]] == want, (tag, rec["fst"], want)
                    else:
                        for k, key in enumerate(FST_KEYS):
                            assert stat_close(key, float(rec["fst"][k]), want[key], want["dxy"]), (tag, key, float(rec["fst"][k]), want[key])
                    hfst_seen.add((name, k_case))
    want_names = {t["name"] for t in seeded} | set(T)
    assert set(compared) == want_names, (set(compared) ^ want_names)  # no table left out of the comparison
    # ... and no golden h-fst case (rounding, L, populations) of any table
    assert hfst_seen == {(name, k) for name, t in T.items() for k in range(len(t["hfst"]))}, hfst_seen
    assert len(hfst_seen) >= 7
    # every captured (hash seed, threshold, rounding) of every seeded table was required at least once
    assert all(compared[t["name"]] >= sum(len(run["pica2"]) for run in t["runs"]) for t in seeded), compared
    assert compared["chain5"] >= 80


# ---- 2. / 3. random ragged batch ----------------------------------------------------------------------------------------------
def random_batch(seed=11):
    rng = np.random.default_rng(seed)
    sizes = [465] * 5 + [1, 2, 3, 2, 3, 1] + [int(x) for x in rng.integers(2, 521, size=61)]
    rng.shuffle(sizes)
    problems = []
    for t, n in enumerate(sizes):
        sim = 0.9982 + 0.0016 * rng.random((n, n))  # around the 0.999 threshold: rounding and grouping matter
        sim = np.minimum(sim, sim.T)
        np.fill_diagonal(sim, 1.0)
        holes = rng.random((n, n)) < (0.03 if t % 3 == 0 else 0.0)
        sim[holes | holes.T] = np.nan
        pr = dict(ident=sim, seq_len=int(rng.integers(1000, 60000)) if t % 7 else 0)
        if t % 2 == 0:
            pr["seed_rank"] = rng.permutation(n).astype(np.uint32)
        if t % 4 != 3:
            fa = (rng.random(n) < 0.45).astype(np.uint8)
            fb = (rng.random(n) < 0.45).astype(np.uint8)  # overlapping A / B
            if t % 10 == 1:
                fb[:] = 0  # an empty population
            pr["in_a"], pr["in_b"] = fa, fb
        if t % 5 == 0:
            pr["tajima_n"], pr["tajima_S"] = max(n, 2), float(rng.integers(0, 400))
        problems.append(pr)
    return problems


def many_group_tables(seed=23):
    """Tables whose group count lies in 65 .. n — the wave-per-row form of the group-pair sum — up to the supported maximum
    n = 1023: every element its own group (all identities below the threshold; real 465-haplotype tables at -t 0.999 look like
    this), with and without NaN holes and a seed order, and clustered tables with 70 .. 400 groups.  -> [(problem, G or None)]"""
    rng = np.random.default_rng(seed)
    out = []
    for n, clusters, holes, ordered in ((465, 0, False, False), (465, 0, True, True), (1023, 0, False, False), (1023, 0, True, True),
                                        (300, 70, False, True), (465, 100, True, False), (1023, 400, False, True), (1023, 65, True, False)):
        sim = 0.90 + 0.0985 * rng.random((n, n))  # < 0.9985: below the 0.999 threshold, rounded to 5 digits or not
        if clusters:
            cl = np.concatenate([np.arange(clusters), rng.integers(0, clusters, size=n - clusters)])
            rng.shuffle(cl)
            same = cl[:, None] == cl[None, :]
            sim[same] = 0.9992 + 0.0007 * rng.random(int(same.sum()))  # every pair inside a cluster is above it
        sim = np.minimum(sim, sim.T)
        np.fill_diagonal(sim, 1.0)
        if holes:
            h = (rng.random((n, n)) < 0.03) & ~(cl[:, None] == cl[None, :] if clusters else np.eye(n, dtype=bool))
            sim[h | h.T] = np.nan  # pairs across groups only: the group count stays what the construction says
        pr = dict(ident=sim, seq_len=int(rng.integers(1000, 60000)))
        if ordered:
            pr["seed_rank"] = rng.permutation(n).astype(np.uint32)
        pr["in_a"], pr["in_b"] = (rng.random(n) < 0.5).astype(np.uint8), (rng.random(n) < 0.5).astype(np.uint8)
        pr["tajima_n"], pr["tajima_S"] = n, float(rng.integers(1, 400))
        out.append((pr, clusters or n))
    return out


def test_random_ragged_batch_equals_single_problem_entry_points(ctx, oracle):
    from impop_amd import _lib
    problems = random_batch()
    ns = [p["ident"].shape[0] for p in problems]
    assert len(problems) >= 64 and ns.count(465) >= 5 and sum(n <= 3 for n in ns) >= 6 and max(ns) <= 520
    many = many_group_tables()
    many_at = {}
    for k, (pr, G) in enumerate(many):  # spread through the batch
        at = 5 + 9 * k
        problems.insert(at, pr)
        many_at[at] = G
    ns = [p["ident"].shape[0] for p in problems]
    assert all(problems[at] is many[k][0] for k, at in enumerate(sorted(many_at)))
    big = dict(ident=np.full((1030, 1030), 0.5), seq_len=10)
    mid = len(problems) // 2
    for rd in (5, None):
        recs, groups = ctx.stats_from_identity_batch(problems, 0.999, rd, rd)
        for t, (pr, rec, grp) in enumerate(zip(problems, recs, groups)):
            check_against_single(ctx, pr, rec, grp, 0.999, rd, rd, (t, ns[t], rd))
            if pr.get("tajima_n") is not None:
                ps = float(rec["pi_site"])
                want = float(ctx.tajimas_d(pr["tajima_n"], pr["tajima_S"], float(f"{ps:.8f}"))[0]) if ps == ps else float("nan")
                assert same_float(float(rec["tajima_d"]), want), (t, float(rec["tajima_d"]), want)
        for at, G in many_at.items():  # the many-group tables really have the group counts they were built for
            assert int(recs[at]["n_groups"]) == G and 65 <= G <= ns[at], (at, ns[at], int(recs[at]["n_groups"]), G)
        assert {ns[at] for at, G in many_at.items() if G == ns[at]} == {465, 1023}
        for t in list(range(0, len(problems), 9))[:8] + sorted(many_at):  # a sample, and every many-group table, against the CPU oracle
            pr, rec = problems[t], recs[t]
            pi, ps, ogrp, oG = oracle.pica2(pr["ident"], 0.999, pr["seq_len"], rd, seed_rank=pr.get("seed_rank"))
            assert oG == int(rec["n_groups"]) and (ogrp == groups[t]).all(), t
            assert rel_close(float(rec["pi"]), pi, REL, 1e-300) and rel_close(float(rec["pi_site"]), ps, REL, 1e-300), t
            if pr.get("in_a") is not None:
                h, _ = oracle.hfst(pr["ident"], pr["in_a"], pr["in_b"], pr["seq_len"], rd)
                for k, key in enumerate(FST_KEYS):
                    assert stat_close(key, float(rec["fst"][k]), h[key], h["dxy"]), (t, key)
        # a table too large for the batch in the middle: its own status, the neighbours' records untouched
        recs2, groups2 = ctx.stats_from_identity_batch(problems[:mid] + [big] + problems[mid:], 0.999, rd, rd)
        assert int(recs2[mid]["status"]) == _lib.E_UNSUPPORTED and len(groups2[mid]) == 1030
        assert np.delete(recs2, mid).tobytes() == recs.tobytes()
        assert all((a == b).all() for a, b in zip(groups2[:mid] + groups2[mid + 1:], groups))


def _chunk_child():
    """child process under IMPOP_TRACE=1 (read once per process): one chunk vs many, and launches per chunk"""
    import impop_amd
    c = impop_amd.Context(0)
    problems = random_batch()
    print("MARK one", file=sys.stderr, flush=True)
    one, g1 = c.stats_from_identity_batch(problems, 0.999, 5, 5, max_chunk_bytes=1 << 30)
    print("MARK many", file=sys.stderr, flush=True)
    many, g2 = c.stats_from_identity_batch(problems, 0.999, 5, 5, max_chunk_bytes=3 << 20)
    assert one.tobytes() == many.tobytes() and all((a == b).all() for a, b in zip(g1, g2))
    small = [p for p in problems if p["ident"].shape[0] <= 120]
    print("MARK four", file=sys.stderr, flush=True)
    c.stats_from_identity_batch(small[:4], 0.999, 5, 5)
    print("MARK forty", file=sys.stderr, flush=True)
    c.stats_from_identity_batch((small * 3)[:40], 0.999, 5, 5)
    print("MARK end", file=sys.stderr, flush=True)
    c.close()
    print("child ok")


def test_chunking_is_invisible():
    env = dict(os.environ, IMPOP_TRACE="1", PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run([sys.executable, "-c", "import test_gpu_sim_batch as t; t._chunk_child()"], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stderr[-3000:]
    sect, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("MARK "):
            cur = line.split()[1]
            sect[cur] = []
        elif line.startswith("[impop_sim_batch]") and cur:
            sect[cur].append({k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", line)})
    assert len(sect["one"]) == 1 and sect["one"][0]["tables"] == 72 and 465 <= sect["one"][0]["max_n"] <= 520
    assert len(sect["many"]) >= 4 and sum(c["tables"] for c in sect["many"]) == 72
    assert [c["chunk"] for c in sect["many"]] == list(range(len(sect["many"])))
    assert all(c["bytes_up"] <= (3 << 20) + 4096 or c["tables"] == 1 for c in sect["many"])  # + alignment of the side tables
    assert len(sect["four"]) == 1 and len(sect["forty"]) == 1
    assert sect["four"][0]["tables"] == 4 and sect["forty"][0]["tables"] == 40
    assert sect["four"][0]["launches"] == sect["forty"][0]["launches"] <= 4
    assert {c["launches"] for s in sect.values() for c in s} == {sect["four"][0]["launches"]}


# ---- 4. / 5. the driver ---------------------------------------------------------------------------------------------------------
def run_py(script, argv, hashseed, cwd):
    r = subprocess.run([sys.executable, os.path.join(SCRIPTS, script)] + argv, capture_output=True, text=True, cwd=cwd,
                       env=dict(os.environ, PYTHONHASHSEED=str(hashseed)))
    r.stderr = "".join(l for l in r.stderr.splitlines(True) if "amdgpu.ids" not in l)  # libdrm's notice at device open
    return r


def write_sim(path, names, sim):
    n = len(names)
    with open(path, "w") as f:
        f.write("group.a\tgroup.b\tgroup.a.length\tgroup.b.length\tintersection\testimated.identity\n")
        for i in range(n):
            f.write("".join(f"{names[i]}\t{names[j]}\t50000\t50000\t49900\t{float(sim[i, j])!r}\n" for j in range(n)))


def data_rows(stdout, header_start="REGION"):
    lines = stdout.splitlines()
    assert lines and lines[0].startswith(header_start), stdout[:300]
    return [l.split("\t") for l in lines[1:]]


def test_driver_equals_the_drop_in_clis(tmp_path):
    td = str(tmp_path)
    rng = np.random.default_rng(3)
    big = [f"HG{i // 2:05d}#{i % 2 + 1}#CM0{i:05d}.1:1000-51000" for i in range(465)]  # as tests/test_sim_ingest.py
    pool = big[:120]
    rows, files = [], []
    for w in range(64):
        if w % 8 == 3:
            names = big
        else:
            k = int(rng.integers(20, 121))
            keep = set(rng.choice(120, size=k, replace=False).tolist()) | {0, 1, 2, 60, 61, 62}  # both populations present
            names = [pool[i] for i in sorted(keep)]
        n = len(names)
        sim = 0.9986 + 0.0009 * rng.random((n, n))  # near the 0.999 threshold
        sim = np.minimum(sim, sim.T)
        np.fill_diagonal(sim, 1.0)
        p = os.path.join(td, f"w{w:02d}.sim")
        write_sim(p, names, sim)
        files.append(p)
        s, e = 10000 * w, 10000 * w + int(rng.integers(5000, 50000))
        rows.append(("chr7", s, e, f"w{w:02d}.sim", int(rng.integers(0, 300))))
    assert sum(1 for w in range(64) if w % 8 == 3) == 8
    with open(os.path.join(td, "windows.tsv"), "w") as f:
        f.write("# chrom start end sim S\n")
        for r in rows:
            f.write("\t".join(str(x) for x in r) + "\n")
    open(os.path.join(td, "popA.txt"), "w").write("".join(f"HG{i:05d}\n" for i in range(0, 25)))
    open(os.path.join(td, "popB.txt"), "w").write("".join(f"HG{i:05d}_hap1_hprc_r2_v1.0.1\n" for i in range(20, 70)) + "NOPE\n")
    open(os.path.join(td, "samples.txt"), "w").write("".join(f"HG{i:05d}\n" for i in range(40)) + "# c\n\n")
    n_samples = 40
    os.mkdir(os.path.join(td, "logs"))
    for seed in (0, 7):
        def per_file(k):
            chrom, s, e, _, S = rows[k]
            L = e - s
            a = run_py("pica2.py", [files[k], "-t", "0.999", "-r", "5", "-l", str(L), "-d", os.path.join(td, "logs")], seed, td)
            b = run_py("h-fst.py", [files[k], "-a", os.path.join(td, "popA.txt"), "-b", os.path.join(td, "popB.txt"), "-l", str(L),
                                    "-d", os.path.join(td, "logs")], seed, td)
            assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
            pi_text = a.stdout.split()[0]
            c = run_py("tj_d.py", ["-n", str(n_samples), "-p", pi_text, "-S", str(S)], seed, td)
            assert c.returncode == 0, c.stderr
            return a.stdout.strip(), b.stdout.strip().split("\t"), pi_text, c.stdout.split()[2]
        with ThreadPoolExecutor(max_workers=8) as ex:  # at most 8 child processes hold the GPU at a time
            want = list(ex.map(per_file, range(64)))
        lst = os.path.join(td, "windows.tsv")
        r = run_py("impop_scan.py", ["--sim-list", lst, "--format", "pica2", "-t", "0.999", "-r", "5"], seed, td)
        assert r.returncode == 0, r.stderr
        got = data_rows(r.stdout)
        assert len(got) == 64
        for k, g in enumerate(got):
            chrom, s, e, _, S = rows[k]
            assert g[:4] == [f"CHM13#0#chr7:{s}-{e}", str(e - s), "0.999", "5"] and g[4] == want[k][0], (seed, k, g, want[k][0])
        r = run_py("impop_scan.py", ["--sim-list", lst, "--format", "hfst", "-A", os.path.join(td, "popA.txt"), "-B",
                                     os.path.join(td, "popB.txt")], seed, td)
        assert r.returncode == 0, r.stderr
        got = data_rows(r.stdout)
        assert len(got) == 64
        for k, g in enumerate(got):
            assert g[2:] == want[k][1], (seed, k, g, want[k][1])
        r = run_py("impop_scan.py", ["--sim-list", lst, "--format", "tajd", "-l", os.path.join(td, "samples.txt")], seed, td)
        assert r.returncode == 0, r.stderr
        got = data_rows(r.stdout)
        assert len(got) == 64
        for k, g in enumerate(got):
            taj = "NA" if want[k][3].lower() == "nan" else want[k][3]
            assert g[2:] == [str(n_samples), str(rows[k][4]), want[k][2], taj], (seed, k, g, want[k])
    assert len({w[0] for w in want}) > 8  # the windows really differ


def test_driver_sends_a_table_too_large_for_the_batch_through_the_single_problem_entry_points(tmp_path):
    """1030 names: IMPOP_E_UNSUPPORTED in the batch record; the pipeline then calls impop_pi_from_identity / impop_fst_from_identity /
    impop_tajimas_d for that window, and its rows equal the per-file CLIs' like its small neighbours' do."""
    td = str(tmp_path)
    rng = np.random.default_rng(5)
    big = [f"HG{i // 2:05d}#{i % 2 + 1}#CM0{i:05d}.1:1000-51000" for i in range(1030)]
    files, rows = [], []
    for w, names in enumerate((big[:40], big, big[:90])):
        n = len(names)
        sim = 0.9986 + 0.0009 * rng.random((n, n))
        sim = np.minimum(sim, sim.T)
        np.fill_diagonal(sim, 1.0)
        files.append(os.path.join(td, f"w{w}.sim"))
        write_sim(files[-1], names, sim)
        rows.append(("chr3", 1000 * w, 1000 * w + 20000 + w, f"w{w}.sim", 40 + w))
    lst = os.path.join(td, "windows.tsv")
    with open(lst, "w") as f:
        for r in rows:
            f.write("\t".join(str(x) for x in r) + "\n")
    A, B, S = (os.path.join(td, x) for x in ("popA.txt", "popB.txt", "samples.txt"))
    open(A, "w").write("".join(f"HG{i:05d}\n" for i in range(0, 12)))
    open(B, "w").write("".join(f"HG{i:05d}\n" for i in range(10, 300)))
    open(S, "w").write("".join(f"HG{i:05d}\n" for i in range(30)))
    os.mkdir(os.path.join(td, "logs"))
    want = []
    for k, (chrom, s, e, _, Sk) in enumerate(rows):
        L = e - s
        a = run_py("pica2.py", [files[k], "-t", "0.999", "-r", "5", "-l", str(L), "-d", os.path.join(td, "logs")], 0, td)
        b = run_py("h-fst.py", [files[k], "-a", A, "-b", B, "-l", str(L), "-d", os.path.join(td, "logs")], 0, td)
        assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
        c = run_py("tj_d.py", ["-n", "30", "-p", a.stdout.split()[0], "-S", str(Sk)], 0, td)
        assert c.returncode == 0, c.stderr
        want.append((a.stdout.strip(), b.stdout.strip().split("\t"), a.stdout.split()[0], c.stdout.split()[2]))
    r = run_py("impop_scan.py", ["--sim-list", lst, "--format", "all", "-A", A, "-B", B, "-l", S], 0, td)
    assert r.returncode == 0, r.stderr
    tables, cur = {}, None
    for line in r.stdout.splitlines():
        f = line.split("\t")
        if f[0] == "REGION":
            cur = tuple(f)
            tables[cur] = []
        else:
            tables[cur].append(f)
    pica, hfst, tajd = (next(v for k, v in tables.items() if key in k) for key in ("PICA_OUTPUT", "FST", "TAJIMAS_D"))
    assert len(pica) == len(hfst) == len(tajd) == 3
    for k in range(3):
        taj = "NA" if want[k][3].lower() == "nan" else want[k][3]
        assert pica[k][4] == want[k][0] and hfst[k][2:] == want[k][1] and tajd[k][2:] == ["30", str(rows[k][4]), want[k][2], taj], (k, pica[k], hfst[k], tajd[k], want[k])


def test_driver_on_seeded_tables_equals_captured_cli_stdout(tmp_path):
    g = load_golden("pica2_seeded.json")
    td = str(tmp_path)
    for t in g["tables"]:
        open(os.path.join(td, t["name"] + ".sim"), "w").write(t["sim_text"])
    n_checked, outcomes = 0, {}
    for si in range(10):
        seed = g["tables"][0]["runs"][si]["hashseed"]
        assert all(t["runs"][si]["hashseed"] == seed for t in g["tables"])
        by_cfg = {}  # the tables were captured at thresholds of their own: one list per (-t, -r), holding the tables captured with it
        for t in g["tables"]:
            for c in t["runs"][si]["cli"]:
                assert c["rc"] == 0 and c["l"] == t["L"]
                by_cfg.setdefault((c["t"], c["r"]), []).append((t, c))
        for (tt, rr), members in by_cfg.items():
            lst = os.path.join(td, "list.tsv")
            with open(lst, "w") as f:
                for t, _ in members:
                    f.write(f"chrS\t0\t{t['L']}\t{t['name']}.sim\n")
            r = run_py("impop_scan.py", ["--sim-list", lst, "--format", "pica2", "-t", str(tt)] + (["-r", str(rr)] if rr is not None else []),
                       seed, td)
            assert r.returncode == 0, r.stderr
            got = data_rows(r.stdout)
            assert len(got) == len(members)
            for (t, c), row in zip(members, got):
                assert row[:3] == [f"CHM13#0#chrS:0-{t['L']}", str(t["L"]), str(tt)]
                assert row[4] == c["stdout"].strip(), (t["name"], seed, tt, rr, row, c["stdout"])
                outcomes.setdefault((t["name"], tt, rr), set()).add(c["stdout"])
                n_checked += 1
    assert n_checked >= 80 and max(len(v) for v in outcomes.values()) >= 2


def test_failed_windows_are_skipped_with_the_drivers_lines(tmp_path):
    td = str(tmp_path)
    names = [f"HG{i // 2:05d}#{i % 2 + 1}#c:0-9" for i in range(8)]
    rng = np.random.default_rng(9)
    sim = 0.99 + 0.01 * rng.random((8, 8))
    sim = np.minimum(sim, sim.T)
    write_sim(os.path.join(td, "good1.sim"), names, sim)
    write_sim(os.path.join(td, "good2.sim"), names[:6], sim[:6, :6])
    write_sim(os.path.join(td, "onlyA.sim"), names[:2], sim[:2, :2])  # no member of population B
    open(os.path.join(td, "bad.sim"), "w").write("group.a\tgroup.b\testimated.identity\nx\ty\t0.5\nx\tz\tzzz\n")
    open(os.path.join(td, "popA.txt"), "w").write("HG00000\n")
    open(os.path.join(td, "popB.txt"), "w").write("HG00001\nHG00002\n")
    open(os.path.join(td, "samples.txt"), "w").write("HG00000\nHG00001\nHG00002\n")

    def write_list(name, sims):
        with open(os.path.join(td, name), "w") as f:
            for k, s in enumerate(sims):
                f.write(f"chr1\t{1000 * k}\t{1000 * k + 1000}\t{s}\t{5 + k}\n")
        return os.path.join(td, name)
    full = write_list("full.tsv", ["good1.sim", "missing.sim", "bad.sim", "onlyA.sim", "good2.sim"])
    reg = lambda k: f"CHM13#0#chr1:{1000 * k}-{1000 * k + 1000}"  # noqa: E731
    miss = os.path.join(td, "missing.sim")
    A, B = os.path.join(td, "popA.txt"), os.path.join(td, "popB.txt")
    cases = {
        "pica2": (["-t", "0.999", "-r", "5"], [0, 3, 4],
                  [f"Error: pica2.py failed for region {reg(1)}", f"Error: File not found {miss}",
                   f"Error: pica2.py failed for region {reg(2)}", "Error: Invalid similarity value on line 3: zzz"]),
        "tajd": (["-l", os.path.join(td, "samples.txt")], [0, 3, 4],
                 [f"Warning: pica2.py failed for region {reg(1)}", f"Warning: pica2.py failed for region {reg(2)}"]),
        # h-fst.py skips the unparsable value with a warning (h-fst.py:107-109); what is left of bad.sim has no population member
        "hfst": (["-A", A, "-B", B], [0, 4],
                 [f"Error: File not found: {miss}", f"Error: FST calculation failed for region {reg(1)}",
                  "Error: No valid sequences found in one or both populations", f"Error: FST calculation failed for region {reg(2)}",
                  "Error: No valid sequences found in one or both populations", f"Error: FST calculation failed for region {reg(3)}"]),
    }
    for fmt, (extra, survivors, want_err) in cases.items():
        r = run_py("impop_scan.py", ["--sim-list", full, "--format", fmt] + extra, 0, td)
        assert r.returncode == 0, (fmt, r.stderr)
        err = [l for l in r.stderr.splitlines() if l.startswith(("Error", "Warning: pica2"))]
        assert err == want_err, (fmt, r.stderr)
        got = data_rows(r.stdout)
        assert [g[0] for g in got] == [reg(k) for k in survivors], (fmt, r.stdout)
        # the other rows are what a list of the good tables alone prints
        sims = ["good1.sim", "missing.sim", "bad.sim", "onlyA.sim", "good2.sim"]
        with open(os.path.join(td, "ok.tsv"), "w") as f:
            for k in survivors:
                f.write(f"chr1\t{1000 * k}\t{1000 * k + 1000}\t{sims[k]}\t{5 + k}\n")
        r2 = run_py("impop_scan.py", ["--sim-list", os.path.join(td, "ok.tsv"), "--format", fmt] + extra, 0, td)
        assert r2.returncode == 0 and r2.stdout == r.stdout, (fmt, r2.stdout, r.stdout)
        assert not [l for l in r2.stderr.splitlines() if l.startswith("Error")], r2.stderr


# ---- 6. device error word -----------------------------------------------------------------------------------------------------
def test_device_error_word_fails_one_batch_call(ctx):
    import ctypes as C

    import impop_amd
    from impop_amd import _lib
    problems = random_batch()[:6]
    want, _ = ctx.stats_from_identity_batch(problems, 0.999, 5, 5)
    _lib.check(_lib.load().impop_debug_raise_device_error(ctx.handle, C.c_uint32(1)))
    with pytest.raises(impop_amd.ImpopError) as e:
        ctx.stats_from_identity_batch(problems, 0.999, 5, 5)
    assert e.value.code == _lib.E_INTERNAL
    got, _ = ctx.stats_from_identity_batch(problems, 0.999, 5, 5)  # reported once, then cleared
    assert got.tobytes() == want.tobytes()
