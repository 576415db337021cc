"""CPU test of tests/state_numpy.py, the numpy restatement of the solver loop with optional Kahan terms: on the SOCP of the GPU
floor tests (tests/test_gpu_state_arith.py, instance A) the dual criterion after 15 000 iterations stagnates in plain f32,
goes more than ten times lower with the compensated iterate and lower again in f64.  The bounds are the ones the GPU tests
put on the device's two state arithmetics: this test pins the emulation they lean on.  The last case records what that floor can
and cannot see: with a term on u alone it is as low as with all five (9.3e-8), so the floor tests bind u's term and no other."""
import pytest

import numpy as np

from state_numpy import criteria_after, socp_dense

ITERS = 15_000


@pytest.fixture(scope="module")
def instance_a():
    return socp_dense(200, [99] * 6, seed=1)


@pytest.mark.parametrize("dtype,kahan,lo,hi", [(np.float32, False, 2e-6, 2e-5), (np.float32, True, 0.0, 5e-7),
                                               (np.float64, False, 0.0, 1e-7), (np.float32, ("u",), 0.0, 5e-7)],
                         ids=["f32-plain", "f32-kahan", "f64", "f32-kahan-on-u-only"])
def test_dual_floor_of_the_emulated_loop(instance_a, dtype, kahan, lo, hi):
    A, b, c, seg, babs = instance_a
    cri = criteria_after(A, b, c, seg, ITERS, dtype, kahan, b_rowabs=babs)
    print("emulated loop, %s %s: cri = (%.3e, %.3e, %.3e)" % (np.dtype(dtype).name, ("kahan %s" % (kahan,) if kahan else "plain"), *cri))
    assert lo < cri[1] < hi, cri
