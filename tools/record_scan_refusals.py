#!/usr/bin/env python3
"""What scripts/impop_scan.py refuses before it reads a file, as a grid of command lines run in process (no GPU, no subprocess).

    python tools/record_scan_refusals.py                       # replay tests/golden/impop_scan_refusals.json against the script
    python tools/record_scan_refusals.py --literals OLD.py     # also list the `return "..."` lines of OLD.py's *_refusal functions
                                                               # that no case of the grid produces
    python tools/record_scan_refusals.py --write               # record the fixture anew (a change of behaviour, never a refactor)

The script is loaded by path as the host tests load it; its load_matrix, read_bed and scan_sim_list are replaced by functions that
raise a sentinel, so a command line that gets that far has passed every refusal.  A case is (format, option fragment, variant):
the fragment alone, with --devices 2, with --sim-list in place of --matrix / --bed, or (one-GPU formats only) with WORLD_SIZE=2.
tests/test_impop_scan_refusals.py replays the fixture with run_case() below."""
import argparse
import ast
import contextlib
import hashlib
import importlib.util
import io
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCAN = os.path.join(ROOT, "scripts", "impop_scan.py")
FIXTURE = os.path.join(ROOT, "tests", "golden", "impop_scan_refusals.json")

FORMATS = ["pica2", "hfst", "tajd", "fst3pi", "af", "ehh", "hapstats", "ld", "diploid", "ibs", "dstat", "sfs", "pairdist", "kinship", "ihs",
           "xpehh", "all"]
CLASSIC = ("pica2", "hfst", "tajd", "fst3pi", "all")  # accept WORLD_SIZE > 1 and would go on to torch.distributed: never run with it
VARIANTS = ["alone", "devices", "simlist", "world"]
PASSED = "passed"

# option -> (a valid sample, out-of-range samples); everything the parser has but --matrix / --bed / --format / --sim-list / --output /
# --device / --backend / --region-prefix
OPTIONS = [
    (["--sim-threads", "4"], []),
    (["--af-clusters", "c.tsv"], []), (["--af-details", "d.tsv"], []),
    (["--ehh-core-offset", "3"], [["--ehh-core-offset", "-1"]]), (["--ehh-cores", "p.txt"], []), (["--ehh-flanks", "two-sided"], []),
    (["--ehh-ref", "X"], []),
    (["--ld-min-maf", "0.1"], [["--ld-min-maf", "0.7"], ["--ld-min-maf", "-0.1"]]),
    (["--ld-max-sites", "64"], [["--ld-max-sites", "2"], ["--ld-max-sites", "2000"]]),
    (["--roh-min-sites", "10"], [["--roh-min-sites", "0"]]), (["--ind-table", "i.tsv"], []),
    (["--ihs-min-maf", "0.1"], [["--ihs-min-maf", "0"], ["--ihs-min-maf", "0.6"]]),
    (["--ihs-cutoff", "0.1"], [["--ihs-cutoff", "1.5"], ["--ihs-cutoff", "-0.1"]]),
    (["--ihs-max-extend", "1000"], [["--ihs-max-extend", "-1"]]), (["--ihs-max-extend-sites", "10"], [["--ihs-max-extend-sites", "-1"]]),
    (["--ihs-bins", "10"], [["--ihs-bins", "0"]]), (["--ihs-keep-edge"], []),
    (["--ibs-min-sites", "10"], [["--ibs-min-sites", "0"]]), (["--ibs-pairs", "diploid"], []), (["--ibs-segments", "s.tsv"], []),
    (["--ibs-pair-table", "p.tsv"], []),
    (["--quartet", "1,2,3,4"], [["--quartet", "1,2,3"], ["--quartet", "1,2,3,9"], ["--quartet", "1,2,2,4"]]),
    (["--dstat-polarize"], []), (["--dstat-blocks", "2"], [["--dstat-blocks", "0"]]), (["--dstat-summary", "s.tsv"], []),
    (["--sfs-outgroup", "1"], [["--sfs-outgroup", "0"], ["--sfs-outgroup", "9"]]),
    (["--sfs-pair", "1,2"], [["--sfs-pair", "1,1"], ["--sfs-pair", "1,9"], ["--sfs-pair", "x"]]),
    (["--sfs-pairs-out", "p.tsv"], []), (["--sfs-spectra", "s.npz"], []), (["--sfs-blocks", "2"], [["--sfs-blocks", "0"]]),
    (["-A", "a.txt"], []), (["-B", "b.txt"], []), (["-A", "a.txt", "-B", "b.txt"], []),
    (["--pairdist-outgroup", "1"], [["--pairdist-outgroup", "0"], ["--pairdist-outgroup", "9"]]),
    (["--pairdist-panels", "p.tsv"], []), (["--pairdist-hist", "h.tsv"], []),
    (["--pairdist-bins", "8"], [["--pairdist-bins", "0"], ["--pairdist-bins", "2000"]]),
    (["--pairdist-bin-width", "2"], [["--pairdist-bin-width", "0"]]),
    (["--kin-threshold", "0.1"], [["--kin-threshold", "1.5"]]), (["--kin-pairs", "k.tsv"], []),
    (["--kin-watch", "A,B"], [["--kin-watch", "A,A"], ["--kin-watch", "A"]]), (["--kin-watch-table", "w.tsv"], []),
    (["--panel", "a.txt", "b.txt"], [["--panel", "a.txt"], ["--panel"] + [f"p{k}.txt" for k in range(9)]]),
    (["-l", "s.txt"], []), (["-u", "u.txt"], []),
    (["--sequence-length", "100"], [["--sequence-length", "0"]]),
    (["-t", "0.99"], [["-t", "nan"]]), (["-r", "5"], [["-r", "-1"], ["-r", "none"]]), (["--fst-round-digits", "5"], []),
    (["--identity", "dice"], []), (["--fst-method", "grouped"], []), (["--compact"], []), (["--devices", "2"], [["--devices", "0"]]),
]
PANEL4 = ["--panel", "a.txt", "b.txt", "c.txt", "d.txt"]
PANEL3 = ["--panel", "a.txt", "b.txt", "c.txt"]
PANEL2 = ["--panel", "a.txt", "b.txt"]
# a context the whole option list is run again behind: the formats whose checks need their --panel first
CONTEXTS = {"dstat": [PANEL4], "sfs": [PANEL2], "pairdist": [PANEL3], "xpehh": [PANEL2], "hfst": [PANEL2], "tajd": [PANEL2], "all": [PANEL2]}
# command lines that reach what one option at a time does not
EXTRA = {
    "ehh": [["--ehh-core-offset", "3", "--ehh-cores", "p.txt"]],
    "dstat": [PANEL4 + ["--dstat-blocks", "2", "--dstat-summary", "s.tsv"], PANEL4 + ["--dstat-blocks", "0", "--dstat-summary", "s.tsv"],
              PANEL4 + ["--panel"] + [f"p{k}.txt" for k in range(5)], ["--panel"] + [f"p{k}.txt" for k in range(5)],
              PANEL4 + [x for k in range(65) for x in ("--quartet", "1,2,3,4")]],
    "sfs": [PANEL2 + ["--sfs-spectra", "s.npz", "--sfs-blocks", "2"], PANEL2 + ["--sfs-spectra", "s.npz", "--sfs-blocks", "0"],
            PANEL2 + ["--sfs-pair", "1,2", "--sfs-pairs-out", "p.tsv"], PANEL2 + ["--sfs-pair", "1,2", "--sfs-spectra", "s.npz"],
            PANEL2 + ["--sfs-spectra", "s.npz"] + [x for k in range(29) for x in ("--sfs-pair", "1,2")]],
    "pairdist": [PANEL3 + ["--pairdist-hist", "h.tsv", "--pairdist-bins", "8"], PANEL3 + ["--pairdist-hist", "h.tsv", "--pairdist-bins", "0"],
                 PANEL3 + ["--pairdist-hist", "h.tsv", "--pairdist-bins", "2000"], PANEL2 + ["--pairdist-outgroup", "1"],
                 PANEL3 + ["--pairdist-hist", "h.tsv", "--pairdist-bins", "8", "--pairdist-bin-width", "0"],
                 PANEL3 + ["--pairdist-hist", "h.tsv", "--pairdist-bins", "8", "--pairdist-bin-width", "2"]],
    "kinship": [["--kin-watch", "A,B", "--kin-watch-table", "w.tsv"], ["--kin-watch", "A,A", "--kin-watch-table", "w.tsv"],
                ["--kin-watch", "A,", "--kin-watch-table", "w.tsv"],
                ["--kin-watch-table", "w.tsv"] + [x for k in range(1025) for x in ("--kin-watch", "A,B")]],
    "xpehh": [PANEL3],
    "hfst": [["-A", "a.txt", "-B", "b.txt", "-t", "0.99"], ["-A", "a.txt", "-B", "b.txt", "-t", "0.99", "--fst-method", "grouped"],
             PANEL2 + ["-r", "5"], PANEL2 + ["--identity", "dice"]],
    "tajd": [["-l", "s.txt", "--sequence-length", "100"]],
    "all": [["-l", "s.txt", "-A", "a.txt", "-B", "b.txt", "--fst-round-digits", "5"]],
    "pica2": [["--sequence-length", "100", "-u", "u.txt"]],
    "fst3pi": [["-A", "a.txt", "-B", "b.txt", "-t", "0.99", "-r", "5"]],
}
# one own flag per format: the (active format, other format) pairs run the other's flag with --devices 2
OWN_FLAG = {"af": ["--af-clusters", "c.tsv"], "ehh": ["--ehh-ref", "X"], "ld": ["--ld-max-sites", "64"], "diploid": ["--roh-min-sites", "3"],
            "ibs": ["--ibs-min-sites", "10"], "dstat": ["--dstat-polarize"], "sfs": ["--sfs-outgroup", "1"],
            "pairdist": ["--pairdist-bins", "8"], "kinship": ["--kin-threshold", "0.1"], "ihs": ["--ihs-bins", "10"],
            "xpehh": ["--ihs-keep-edge"], "pica2": ["--sequence-length", "100"], "hfst": ["--fst-method", "grouped"],
            "tajd": ["-l", "s.txt"], "fst3pi": ["-A", "a.txt", "-B", "b.txt"], "all": ["--fst-round-digits", "5"], "hapstats": ["--compact"]}


# refusal lines no command line of the grid reaches, with the reason
UNREACHED = [{"message": "--sim-list is a one-process, one-GPU driver: not under torch.distributed.run",
              "reason": "needs WORLD_SIZE > 1 with pica2 / hfst / tajd / all, which the grid never runs: past the refusals those go on to "
                        "torch.distributed"}]


class Passed(Exception):
    """raised by the stand-ins for load_matrix / read_bed / scan_sim_list: every refusal has passed"""


def load_cli(path=SCAN, name="impop_scan_cli_refusals"):
    scripts = os.path.join(ROOT, "scripts")
    sys.path.insert(0, scripts)
    try:
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        sys.path.remove(scripts)

    def passed(*a, **k):
        raise Passed()
    mod.load_matrix = mod.read_bed = mod.scan_sim_list = passed
    return mod


def argv_of(fmt, fragment, variant):
    files = ["--sim-list", "s.tsv"] if variant == "simlist" else ["--matrix", "m.npz", "--bed", "w.bed"]
    return ["impop_scan.py", "--format", fmt] + files + list(fragment) + (["--devices", "2"] if variant == "devices" else [])


def run_case(cli, fmt, fragment, variant):
    """-> (exit code or PASSED, stderr text)"""
    if variant == "world" and fmt in CLASSIC:
        raise ValueError(f"--format {fmt} accepts WORLD_SIZE > 1: not part of the grid")
    keep = {k: os.environ.get(k) for k in ("WORLD_SIZE", "COLUMNS")}
    old_argv, err = sys.argv, io.StringIO()
    os.environ["COLUMNS"] = "100"
    os.environ.pop("WORLD_SIZE", None)
    if variant == "world":
        os.environ["WORLD_SIZE"] = "2"
    sys.argv = argv_of(fmt, fragment, variant)
    try:
        with contextlib.redirect_stderr(err), contextlib.redirect_stdout(io.StringIO()):
            try:
                cli.main()
                code = 0
            except Passed:
                code = PASSED
            except SystemExit as e:
                code = e.code
    finally:
        sys.argv = old_argv
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return code, err.getvalue()


def grid():
    """-> (fragments, [(format index, fragment index, variant index)])"""
    fragments, index, cases = [], {}, []

    def frag(f):
        key = tuple(f)
        if key not in index:
            index[key] = len(fragments)
            fragments.append(list(f))
        return index[key]

    singles = [[]] + [f for valid, bad in OPTIONS for f in [valid] + bad]
    for fi, fmt in enumerate(FORMATS):
        todo = list(singles)
        for ctx in CONTEXTS.get(fmt, []):
            todo += [ctx + f for f in singles if f[:1] != ["--panel"]]
        todo += EXTRA.get(fmt, [])
        for f in todo:
            for vi, variant in enumerate(VARIANTS):
                if variant == "world" and fmt in CLASSIC:
                    continue
                cases.append((fi, frag(f), vi))
    for fi, fmt in enumerate(FORMATS):
        for other in FORMATS:
            if other != fmt:
                cases.append((fi, frag(OWN_FLAG[other]), VARIANTS.index("devices")))
    return fragments, sorted(set(cases))


def grid_digest(fragments, cases):
    """what ties a fixture to the grid it was recorded on"""
    return hashlib.sha256(json.dumps([FORMATS, VARIANTS, fragments, cases]).encode()).hexdigest()


def record(cli):
    """-> the fixture: the distinct outcomes [exit code or PASSED, stderr text] and, per case in the order of grid(), its outcome"""
    fragments, cases = grid()
    outcomes, index, results = [], {}, []
    for fi, gi, vi in cases:
        got = run_case(cli, FORMATS[fi], fragments[gi], VARIANTS[vi])
        if got not in index:
            index[got] = len(outcomes)
            outcomes.append(list(got))
        results.append(index[got])
    return {"grid_sha256": grid_digest(fragments, cases), "outcomes": outcomes, "results": results, "unreached": UNREACHED}


def refusal_literals(path):
    """the `return "..."` / `return f"..."` lines of the *_refusal functions of a script -> [(line, regex)]"""
    out = []

    def strings(node):
        if isinstance(node, ast.Constant) and isinstance(node.value, str):
            yield re.escape(node.value)
        elif isinstance(node, ast.JoinedStr):
            yield "".join(re.escape(v.value) if isinstance(v, ast.Constant) else ".*" for v in node.values)
        elif isinstance(node, ast.IfExp):
            yield from strings(node.body)
            yield from strings(node.orelse)
        elif isinstance(node, ast.BinOp):  # adjacent literals joined with +
            left, right = list(strings(node.left)), list(strings(node.right))
            if left and right:
                yield left[0] + right[0]

    for fn in ast.walk(ast.parse(open(path).read())):
        if isinstance(fn, ast.FunctionDef) and fn.name.endswith("_refusal"):
            for node in ast.walk(fn):
                if isinstance(node, ast.Return) and node.value is not None:
                    for rx in strings(node.value):
                        out.append((node.lineno, rx))
    return out


def unreached(path, messages):
    seen = [m[len("Error: "):].rstrip("\n") for m in messages if m.startswith("Error: ")]
    return [(line, rx) for line, rx in refusal_literals(path) if not any(re.fullmatch(rx, m, re.S) for m in seen)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--script", default=SCAN)
    ap.add_argument("--literals", metavar="OLD.py", help="a script with *_refusal functions: list their return lines no case produces")
    ap.add_argument("--write", action="store_true", help="write the fixture instead of comparing with it")
    args = ap.parse_args()
    got = record(load_cli(args.script))
    print(f"{len(got['results'])} cases, {len(got['outcomes'])} distinct outcomes")
    if args.literals:
        missing = unreached(args.literals, [text for _, text in got["outcomes"]])
        for line, rx in missing:
            print(f"unreached: line {line}: {rx}")
        print(f"{len(missing)} refusal lines unreached")
    if args.write:
        with open(FIXTURE, "w") as f:
            json.dump(got, f, separators=(",", ":"))
            f.write("\n")
        print(f"wrote {FIXTURE} ({os.path.getsize(FIXTURE)} bytes)")
        return 0
    same = os.path.exists(FIXTURE) and json.load(open(FIXTURE)) == got
    print("the script answers as recorded" if same else "the script does NOT answer as recorded")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
