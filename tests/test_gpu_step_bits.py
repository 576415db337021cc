"""GPU: the bits of the main solver's loops (FusedSolver on every schedule, BatchSolver) against tests/golden/step_bits.json.

What this pins is this library's arithmetic under this compiler on gfx950: per case and run, a SHA-256 of the iterate and of the
solution after 40 iterations with a launch cut inside (25 in one launch, then 15 in launches of 5), the status, cri / tau / kappa bit
for bit and the schedule in use.  The cases are the smallest shapes that reach every kernel that carries the step's arithmetic
(totsu_amd/csrc/thip_step.h): the reference, fused and carried schedules with compensated and plain state, the block-per-cone
projection, the one-launch, merged, one-thread-per-row and three-launch m-tails of the one-pass schedule with the folded
termination test, the tiled sparse copy, rows of PSD blocks, the tau -> 0 ending of the verdict, and BatchSolver.  No tolerance: a
refactor of the kernels must leave every field as it is.

The record is made by tests/golden/make_step_bits_fixture.py, which this test calls case by case.  To re-record deliberately -- on a
commit whose arithmetic is meant to change, or after a toolchain bump -- run that script on an MI355X and commit its output, saying so
in the commit."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_step_bits_fixture", os.path.join(GOLDEN, "make_step_bits_fixture.py"))
FX = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FX)


@pytest.fixture(scope="module")
def T():
    import totsu_amd
    from totsu_amd import _lib
    _lib.init()
    return totsu_amd


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "step_bits.json")) as f:
        return json.load(f)["cases"]


def test_the_fixture_holds_every_case_on_its_schedule(recorded):
    assert sorted(recorded) == sorted(FX.CASE_IDS)
    for cid, _, runs in FX.CASES:
        for label, schedule, _ in runs:
            if schedule is not None:             # (no fall-back from "sweep": the record is of the kernels the case is there for)
                assert recorded[cid]["runs"][label]["schedule"] == schedule, (cid, label)
    assert [r["status"][2] for r in recorded["F1"]["runs"].values()] == [1, 1]      # both verdicts are of the tau -> 0 kind


@pytest.mark.parametrize("case", FX.CASE_IDS)
def test_bits(T, recorded, case):
    want, got = recorded[case], FX.record(T, case)
    assert got["inputs"] == want["inputs"], "%s: inputs differ (a generator changed, not a kernel)" % case
    assert sorted(got["runs"]) == sorted(want["runs"]), case
    diff = ["%s %s %s: %r, recorded %r" % (case, r, k, got["runs"][r].get(k), want["runs"][r].get(k))
            for r in sorted(want["runs"]) for k in sorted(set(got["runs"][r]) | set(want["runs"][r]))
            if got["runs"][r].get(k) != want["runs"][r].get(k)]
    assert not diff, "\n".join(diff)
