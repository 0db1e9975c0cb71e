"""No GPU: what scripts/impop_scan.py refuses before it reads a file.  tools/record_scan_refusals.py builds a grid of command lines
(every format x every option, valid and out of range, alone / with --devices 2 / with --sim-list / under WORLD_SIZE=2, and every
ordered pair of formats) and runs a case in process; tests/golden/impop_scan_refusals.json holds, per case in the grid's order, the
exit code and the stderr text the driver gave when the fixture was recorded.  The fixture is frozen: a refactor of the driver
never re-records it."""
import importlib.util
import json
import os

import pytest

from conftest import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "impop_scan_refusals.json")


@pytest.fixture(scope="module")
def recorder():
    spec = importlib.util.spec_from_file_location("record_scan_refusals", os.path.join(ROOT, "tools", "record_scan_refusals.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_is_the_grid(recorder, fixture):
    assert os.path.getsize(FIXTURE) < 200 * 1024
    fragments, cases = recorder.grid()
    assert fixture["grid_sha256"] == recorder.grid_digest(fragments, cases) and len(fixture["results"]) == len(cases)
    assert len(fixture["unreached"]) <= 10 and all(u["message"] and u["reason"] for u in fixture["unreached"])
    world, devices = recorder.VARIANTS.index("world"), recorder.VARIANTS.index("devices")
    for fi, _, vi in cases:  # the formats that accept a multi-process launch never run with WORLD_SIZE=2
        assert not (vi == world and recorder.FORMATS[fi] in recorder.CLASSIC)
    with_devices = {(fi, tuple(fragments[gi])) for fi, gi, vi in cases if vi == devices}
    for fi, fmt in enumerate(recorder.FORMATS):  # every ordered pair of formats: the other's own flag with --devices 2
        for other in recorder.FORMATS:
            assert other == fmt or (fi, tuple(recorder.OWN_FLAG[other])) in with_devices


def test_driver_refuses_as_recorded(recorder, fixture):
    cli = recorder.load_cli()
    env = dict(os.environ)
    fragments, cases = recorder.grid()
    wrong = []
    for (fi, gi, vi), k in zip(cases, fixture["results"]):
        fmt, fragment, variant = recorder.FORMATS[fi], fragments[gi], recorder.VARIANTS[vi]
        got, want = recorder.run_case(cli, fmt, fragment, variant), tuple(fixture["outcomes"][k])
        if got != want:
            wrong.append((fmt, variant, " ".join(fragment)[:200], (got[0], got[1][-300:]), (want[0], want[1][-300:])))
    assert dict(os.environ) == env
    assert not wrong, f"{len(wrong)} of {len(cases)} cases differ; the first: {wrong[0]}"
