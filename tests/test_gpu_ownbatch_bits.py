"""GPU: the bits of the three own-A batch families (SmallBatchSolver, MidBatchSolver, SdpBatchSolver) against
tests/golden/ownbatch_bits.json.

What this pins is this library's arithmetic under this compiler on gfx950: per case and problem, a SHA-256 of the iterate, the
preconditioner and the solution after 40 iterations with launch cuts inside (25 in one launch, then 15 in launches of 5), the
status and cri / tau / kappa bit for bit.  The cases reach every path of the shared init and iteration bodies: every workgroup size
a family has, block cones and rowabs, "plain" state arithmetic, replace (the init kernel on one slot), the 16-byte and the 4-byte
load of a streamed A, the tau -> 0 ending of status_eval, PSD orders on both sides of 32, and an SDP batch without a PSD segment.
No tolerance: a refactor of the kernels or of the host machinery must leave every field as it is.

The record is made by tests/golden/make_ownbatch_bits_fixture.py, which this test calls case by case.  To re-record deliberately --
on a commit whose arithmetic is meant to change, or after a toolchain bump -- run that script on an MI355X and commit its output,
saying so in the commit."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_ownbatch_bits_fixture", os.path.join(GOLDEN, "make_ownbatch_bits_fixture.py"))
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
    with open(os.path.join(GOLDEN, "ownbatch_bits.json")) as f:
        return json.load(f)["cases"]


def test_the_fixture_holds_every_case(recorded):
    assert sorted(recorded) == sorted(FX.CASE_IDS)


@pytest.mark.parametrize("case", FX.CASE_IDS)
def test_bits(T, recorded, case):
    want, got = recorded[case], FX.record(T, case)
    assert got["inputs"] == want["inputs"], "%s: inputs differ (a generator changed, not a kernel)" % case
    assert len(got["problems"]) == len(want["problems"]), case
    diff = ["%s problem %d %s: %r, recorded %r" % (case, i, k, g[k], w[k])
            for i, (g, w) in enumerate(zip(got["problems"], want["problems"])) for k in sorted(set(g) | set(w)) if g.get(k) != w.get(k)]
    assert not diff, "\n".join(diff)
