"""CPU: the host side of the `.sim` batch — impop_sim_parse_many against per-file impop_sim_parse, the list reader, the
argument errors of `impop_scan.py --sim-list` (raised before any device is opened) and the "%.8f" -> Tajima wiring of the
batch records as host arithmetic."""
import ctypes as C
import math
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, fh, load_golden

SCAN = os.path.join(ROOT, "scripts", "impop_scan.py")
HDR = "group.a\tgroup.b\testimated.identity\n"


def snapshot(lib, h):
    """everything the accessors tell about one parsed table"""
    from impop_amd import _lib
    n, rows, nb, bad_line, n_bad = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_int64(), C.c_uint64()
    _lib.check(lib.impop_sim_info(h, C.byref(n), C.byref(rows), C.byref(nb), C.byref(bad_line), C.byref(n_bad)))
    buf = C.create_string_buffer(max(nb.value, 1))
    _lib.check(lib.impop_sim_names(h, buf))
    dense = np.empty((n.value, n.value))
    _lib.check(lib.impop_sim_dense(h, dense.ctypes.data_as(C.POINTER(C.c_double))))
    seen = np.zeros(max(n.value, 1), dtype=np.uint32)
    _lib.check(lib.impop_sim_first_seen(h, seen.ctypes.data_as(C.POINTER(C.c_uint32))))
    txt = C.create_string_buffer(256)
    _lib.check(lib.impop_sim_bad_text(h, txt, len(txt)))
    return (buf.raw[: nb.value], dense.tobytes(), rows.value, seen[: n.value].tobytes(), bad_line.value, txt.value, n_bad.value)


def mixed_files(tmp_path):
    files = []

    def put(name, text):
        p = tmp_path / name
        p.write_bytes(text.encode())
        files.append(str(p))
    put("win8.sim", load_golden("cli_pansn.json")["sim_text"])
    for t in load_golden("pica2_seeded.json")["tables"]:
        put(t["name"] + ".sim", t["sim_text"])
    # the random table recipe of tests/test_sim_ingest.py: duplicates, self pairs, extra columns, CRLF, exponents, blank lines
    for seed in (5, 6, 7):
        rnd = random.Random(seed)
        nm = [f"S{i:03d}#{h}#chr{rnd.randint(1, 3)}:{rnd.randint(0, 9)}-{rnd.randint(10, 99)}" for i in range(10 * seed) for h in (1, 2)]
        lines = ["x\tgroup.b\tjunk\testimated.identity\tgroup.a"]
        for _ in range(1500):
            a, b = rnd.choice(nm), rnd.choice(nm)
            v = rnd.choice([repr(rnd.random()), "1", "0.99950", "1e-3", "9.99E-01", " 0.5 ", "+.5", "5.", "1E+0", "nan", "inf", "-Infinity"])
            lines.append(f"q\t{b}\tzz\t{v}\t{a}\textra\tmore")
            if rnd.random() < 0.02:
                lines.append("")
        put(f"rand{seed}.sim", "\r\n".join(lines) + "\r\n")
    put("declined.sim", HDR + 'a\t"b"\t0.5\n')          # csv quoting: left to the Python reader
    put("badvalue.sim", HDR + "a\tb\t0.5\nx\ty\tzzz\nc\td\t0.25\n")
    put("empty.sim", "")
    files.append(str(tmp_path / "missing.sim"))
    return files


@pytest.mark.parametrize("flavor", [0, 1])
def test_parse_many_equals_per_file_parse(tmp_path, flavor):
    from impop_amd import _lib
    lib = _lib.load()
    files = mixed_files(tmp_path)
    want = []
    for f in files:
        h = C.c_void_p()
        rc = lib.impop_sim_parse(os.fsencode(f), flavor, C.byref(h))
        assert (rc == 0) == bool(h.value)
        want.append((rc, snapshot(lib, h) if rc == 0 else None))
        if rc == 0:
            lib.impop_sim_free(h)
    assert {rc for rc, _ in want} == {0, _lib.E_UNSUPPORTED, _lib.E_INVALID}
    assert any(s is not None and (s[4] >= 0 or s[6] > 0) for _, s in want)  # the bad value is in the set
    k = len(files)
    paths = (C.c_char_p * k)(*[os.fsencode(f) for f in files])
    for n_threads in (1, 3, 16):
        handles, rcs = (C.c_void_p * k)(), (C.c_int32 * k)()
        _lib.check(lib.impop_sim_parse_many(paths, k, flavor, n_threads, handles, rcs))
        for i in range(k):
            assert rcs[i] == want[i][0], (files[i], n_threads)
            assert bool(handles[i]) == (rcs[i] == 0)
            if rcs[i] == 0:
                h = C.c_void_p(handles[i])
                assert snapshot(lib, h) == want[i][1], (files[i], n_threads)
                lib.impop_sim_free(h)
    # the Python ingest over the same files: tables, the reference's failure texts, the declined file via the Python reader
    from impop_amd import simbatch
    res = simbatch.ingest(files, "pica2" if flavor == 0 else "hfst", n_threads=3)
    by = {os.path.basename(f): r for f, r in zip(files, res)}
    assert isinstance(by["win8.sim"], simbatch.SimTable) and len(by["win8.sim"].names) == 8
    # each reader's own spelling (pica2.py:55-57, h-fst.py:116-118)
    assert by["missing.sim"] == simbatch.SimFailure(f"Error: File not found{'' if flavor == 0 else ':'} {files[-1]}")
    assert isinstance(by["declined.sim"], simbatch.SimTable) and by["declined.sim"].names == ["a", "b"]
    if flavor == 0:
        assert by["badvalue.sim"] == simbatch.SimFailure("Error: Invalid similarity value on line 3: zzz")
        assert by["empty.sim"] == simbatch.SimFailure(f"Error: File {files[-2]} is empty or missing a header")
    else:
        assert by["badvalue.sim"].names == ["a", "b", "c", "d"]  # h-fst skips the bad value with a warning
    t = by["chain5.sim"]
    assert sorted(t.elements) == t.names and t.dense.shape == (5, 5)


@pytest.mark.parametrize("sanitizer", ["address,undefined", "thread"])
def test_parse_many_under_host_sanitizers(tmp_path, sanitizer):
    """The recipe of tests/test_parser_fuzz.py for the library's only threaded code: csrc/simparse.hip compiled AS C++ with a host
    sanitizer next to tests/fuzz/parse_many_threads.cc, over the mixed file set (clean, declined, bad value, empty, missing) with
    1, 3 and 16 threads: every result equals impop_sim_parse's, and the sanitizer reports nothing."""
    import shutil
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    csrc = os.path.join(ROOT, "impop_amd", "csrc")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=" + sanitizer, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + csrc]
    if "undefined" in sanitizer:
        flags.append("-fno-sanitize-recover=undefined")
    exe = str(tmp_path / "parse_many_threads")
    r = subprocess.run([gxx] + flags + ["-x", "c++", os.path.join(csrc, "simparse.hip"), os.path.join(ROOT, "tests", "fuzz", "parse_many_threads.cc"),
                        "-o", exe, "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    d = tmp_path / "files"
    d.mkdir()
    files = mixed_files(d)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1", TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "parse_many ok" in r.stdout and "ERROR" not in r.stderr and "WARNING: ThreadSanitizer" not in r.stderr \
        and "runtime error" not in r.stderr, r.stderr[-4000:]
    nums = [int(x) for x in re.findall(r"(\d+)", r.stdout.strip().splitlines()[-1])]
    assert nums[0] >= 24 * 4 * len(files) and nums[1] > 0 and nums[2] > 0, r.stdout


def test_parse_many_thread_default_and_bad_arguments(tmp_path, monkeypatch):
    from impop_amd import _lib
    lib = _lib.load()
    p = tmp_path / "a.sim"
    p.write_text(HDR + "a\tb\t0.5\n")
    paths = (C.c_char_p * 2)(os.fsencode(str(p)), None)
    handles, rcs = (C.c_void_p * 2)(), (C.c_int32 * 2)()
    monkeypatch.setenv("OMP_NUM_THREADS", "2")
    assert lib.impop_sim_parse_many(paths, 2, 0, 0, handles, rcs) == 0
    assert rcs[0] == 0 and rcs[1] == _lib.E_INVALID and handles[0] and not handles[1]
    lib.impop_sim_free(C.c_void_p(handles[0]))
    assert lib.impop_sim_parse_many(paths, 2, 0, -1, handles, rcs) == _lib.E_INVALID
    assert lib.impop_sim_parse_many(None, 2, 0, 1, handles, rcs) == _lib.E_INVALID
    assert lib.impop_sim_parse_many(None, 0, 0, 1, None, None) == 0


def test_list_reader(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import impop_scan
    finally:
        sys.path.pop(0)
    from impop_amd import simbatch
    sub = tmp_path / "lists"
    sub.mkdir()
    bed_rows = ["chr1\t0\t1000", "# a comment", "", "chr1\t1000\t2000", "chr2\tx\t5", "chr2\t9\t9", "chr2\t10\t3", "chr3\t5", "chr3\t7\t70"]
    extra = ["\tw/a.sim", "", "", "\t/abs/b.sim\t17", "\tc.sim", "\td.sim\t3", "\te.sim", "", "\tf.sim\t"]
    (sub / "w.bed").write_text("\n".join(bed_rows) + "\n")
    (sub / "w.tsv").write_text("\n".join(b + (x if b and not b.startswith("#") else "") for b, x in zip(bed_rows, extra)) + "\n")
    for fmt in ("pica2", "hfst", "tajd", "all"):
        capsys.readouterr()
        bed = impop_scan.read_bed(str(sub / "w.bed"), fmt)
        bed_err = capsys.readouterr().err
        rows = simbatch.read_sim_list(str(sub / "w.tsv"), fmt)
        assert capsys.readouterr().err == bed_err and bed_err.count("Warning:") >= 3
        assert [(r.chrom, r.start, r.end) for r in rows] == bed
        assert rows[0].sim_path == str(sub / "w" / "a.sim") and rows[0].S is None   # relative to the list's directory
        assert rows[1].sim_path == "/abs/b.sim" and rows[1].S == "17"
        assert rows[-1].sim_path == str(sub / "f.sim") and rows[-1].S is None       # an empty S cell is no S
    (sub / "short.tsv").write_text("chr1\t0\t10\n")
    with pytest.raises(ValueError):
        simbatch.read_sim_list(str(sub / "short.tsv"), "pica2")


def test_population_flags_are_cached_per_name_tuple():
    from impop_amd import simbatch
    g = load_golden("popnames.json")
    pf = simbatch.PopulationFlags(g["raw"])
    names = sorted(g["sequences"])
    flags, n_missing = pf(names)
    assert [n for n, f in zip(names, flags) if f] == g["expanded"] and n_missing == len(g["missing"])
    assert pf(list(names))[0] is flags                    # same names: the cached array
    sub = names[: len(names) // 2]
    f2, _ = pf(sub)
    assert [n for n, f in zip(sub, f2) if f] == [n for n in g["expanded"] if n in set(sub)]


def scan(argv, env=None, cwd=None):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.update(env or {})
    return subprocess.run([sys.executable, SCAN] + argv, capture_output=True, text=True, env=e, cwd=cwd)


def test_sim_list_argument_errors_exit_2_before_any_device(tmp_path):
    lst = tmp_path / "w.tsv"
    lst.write_text("chr1\t0\t100\ta.sim\n")
    (tmp_path / "s.txt").write_text("HG1\nHG2\n")
    L, S = str(lst), str(tmp_path / "s.txt")
    cases = [
        (["--sim-list", L, "--matrix", "m.npz", "--bed", "w.bed"], "--sim-list replaces --matrix / --bed", None),
        (["--format", "pica2"], "give --matrix and --bed, or --sim-list", None),
        (["--sim-list", L, "--format", "pica2", "--devices", "2"], "not with --devices", None),
        (["--sim-list", L, "--format", "hfst", "-A", "a", "-B", "b", "--panel", "a", "b"], "--panel", None),
        (["--sim-list", L, "--format", "pica2", "--compact"], "--compact", None),
        (["--sim-list", L, "--format", "hfst", "-A", "a", "-B", "b", "--fst-method", "grouped"], "--fst-method grouped", None),
        (["--sim-list", L, "--format", "pica2"], "torch.distributed.run", {"WORLD_SIZE": "2", "RANK": "0"}),
        (["--sim-list", L, "--format", "fst3pi"], "pica2, hfst, tajd and all", None),
        (["--sim-list", L, "--format", "hfst"], "needs -A and -B", None),
        (["--sim-list", L, "--format", "tajd"], "needs -l", None),
        (["--sim-list", L, "--format", "tajd", "-l", S], "needs a non-negative S column", None),  # the list has no S
        (["--sim-list", L, "--format", "hfst", "-A", "a", "-B", "b", "-t", "0.9"], "takes -t only with", None),
    ]
    for argv, text, env in cases:
        r = scan(argv, env)
        assert r.returncode == 2, (argv, r.returncode, r.stderr)
        assert text in r.stderr and r.stdout == "", (argv, r.stderr)
        assert len([l for l in r.stderr.splitlines() if l.startswith("Error:")]) <= 1
        assert "no HIP device" not in r.stderr and "Traceback" not in r.stderr, r.stderr


def test_tajima_wiring_from_pi_text_against_goldens(oracle):
    """A record's tajima_d = tj_d.py's D at pi = float("%.8f" % pi_site) (run_tajd.sh:174-180): the same host arithmetic the
    kernel runs, against the oracle (pinned bit-exact to tests/golden/tajima.json by test_oracle_golden) at the text value,
    and against the golden D itself where the golden pi already is its own 8-decimal text."""
    from impop_amd import simbatch
    g = load_golden("tajima.json")
    exact = 0
    for c in g["cases"]:
        n, S, pi = c["n"], fh(c["S"]), fh(c["pi"])
        for x in (pi, pi / 3.0, pi * 1e-3, 0.5e-8, 1.5e-8, 2.5e-8, 0.123456785, 0.0):
            got = simbatch.tajimas_d_from_pi_site(n, S, x)
            want, _ = oracle.tajimas_d(n, S, float(f"{x:.8f}"))
            assert (math.isnan(got) and math.isnan(want)) or got == want, (n, S, x, got, want)
        if float(f"{pi:.8f}") == pi:
            got, want = simbatch.tajimas_d_from_pi_site(n, S, pi), fh(c["D"])
            assert (math.isnan(got) and math.isnan(want)) or got == want
            exact += 1
    assert exact >= 1
    for e in g["errors"]:  # what tj_d.py refuses is "no D" in a record
        assert math.isnan(simbatch.tajimas_d_from_pi_site(e["n"], e["S"], e["pi"]))
    assert math.isnan(simbatch.tajimas_d_from_pi_site(10, 5.0, float("nan")))
