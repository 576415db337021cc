"""The problems of the warm-start tests (tests/test_warm_start_cpu.py, tests/test_gpu_warm_start.py) that numpy alone builds, and the
oracle's runs of them at the iterations a start is taken from and compared at (computed once per session and never changed).  A
plain module, like tests/ownbatch_cases.py, whose helpers it uses."""
import numpy as np

import oracle as O
from ownbatch_cases import F, _D, _edge, _oracle
from problems import benchmark_lp, random_socp
from sparse_cases import masked, problem_of
from state_numpy import socp_dense
from tau_zero_problems import svec

ZERO, RPOS, SOC, ROT, PSD = 0, 1, 2, 3, 4
K_START, J_RUN = (0, 9), (1, 10)                      # a start is the snapshot after iteration k; j iterations are run from it
SNAPS = [0, 1, 9, 10, 19]                             # every k and every k + j
SOCP_CONES = [5, 1, 0, 17, 70, 3]                     # 102 x 12, tests/ownbatch_cases.py's "socp"


# what the project's oracle tests hold an iterate to, relative to the reference iterate's max norm, at the iterates they check
# (tests/ownbatch_cases.py TOLS / SDP_TOLS, tests/test_gpu_solver.py): (iterate, tolerance)
_ANCHORS = {False: ((0, 2e-5), (1, 2e-5), (9, 1e-4), (99, 2e-3)), True: ((0, 5e-5), (1, 5e-5), (9, 3e-4), (49, 3e-3))}


def iterate_tol(it, psd=False):
    """the tolerance of iterate `it`: the existing tests' at an iterate they check, and between two of those the geometric
    interpolation of the two -- the f32 error of the loop grows with the iteration count, and a bound that grows by a constant
    factor per iteration is the tighter of the two simple ways to join two checked points (at iterate 10: 1.03e-4 where the linear
    join gives 1.21e-4).  Nothing here comes from what the start kernels were measured to give (about 2e-6)"""
    pts = _ANCHORS[bool(psd)]
    assert pts[0][0] <= it <= pts[-1][0], it
    for (i0, t0), (i1, t1) in zip(pts, pts[1:]):
        if i0 <= it <= i1:
            return t0 * (t1 / t0) ** ((it - i0) / (i1 - i0))


def sdp_numpy(n, k, seed):
    """a strictly primal- and dual-feasible SDP with one PSD cone of order k, tri(k) x n, in the stacked form: the slack is
    -(sum_j x_j F_j + F_n), packed as ProbSDP.dense() packs it (tests/tau_zero_problems.py::f5 without its contradiction)"""
    rng = np.random.default_rng(31337 + 100 * k + seed)
    x0 = rng.standard_normal(n)
    Fs = []
    for _ in range(n):
        B = rng.standard_normal((k, k)) / np.sqrt(n)
        Fs.append((B + B.T) / 2)
    Fn = -np.eye(k) - sum(x * Fm for x, Fm in zip(x0, Fs))
    B = rng.standard_normal((k, k))
    Y = B @ B.T / k + 0.1 * np.eye(k)
    c = np.array([-np.trace(Fm @ Y) for Fm in Fs])
    return _D(np.stack([svec(Fm) for Fm in Fs], axis=1), -svec(Fn), c, [PSD], [k * (k + 1) // 2])


def socp_numpy(seed):
    """tests/ownbatch_cases.py's 102 x 12 SOCP as numpy stacks it (tests/state_numpy.py::socp_dense), with the pieces its oracle takes"""
    A, b, c, seg, babs = socp_dense(12, SOCP_CONES, seed)
    d = _D(A, b, c, [t for t, _ in seg], [l for _, l in seg])
    d.vec_b_rowabs = babs
    assert (d.m, d.n) == (102, 12)
    return d, random_socp(12, SOCP_CONES, seed=seed)


def sparse40x30(seed):
    """a 40 x 30 LP at about 10 % density with an empty column (28), an empty row (38), a full row (13) and a column of exactly 33
    entries (5) -- one more than the sparse pass's SPB_LONG = 32, so that column is summed by a wave; no row of 30 columns can be"""
    rng = np.random.default_rng(4040 + seed)
    A = masked(40, 30, 0.10, rng)
    col = np.zeros(40, F)
    rows = rng.choice([r for r in range(40) if r != 38], size=33, replace=False)
    col[rows] = (rng.standard_normal(33) / np.sqrt(3.0)).astype(F)
    A[:, 5] = col
    A[13, 5] = A[13, 5] if A[13, 5] != 0 else F(0.25)
    A[38, :] = 0
    assert int((A[:, 5] != 0).sum()) in (33, 34) and not A[:, 28].any() and not A[38].any()
    return problem_of(A, [RPOS], [40], rng)


_RUNS = {}


def oracle_run(key, d, socp=None):
    """the oracle's snapshots and trace of problem d at SNAPS (computed once per key)"""
    if key not in _RUNS:
        ro = _oracle(d, SNAPS, socp=socp)
        assert ro.status == O.EXCESS_ITER and len(ro.trace) > max(SNAPS)
        _RUNS[key] = ro
    return _RUNS[key]


def snap_xy(ro, d, it):
    """(x, y) of the oracle's snapshot after iteration `it`"""
    N = d.n + 2 * d.m + 1
    s = ro.snaps[SNAPS.index(it)]
    return s[:N], s[N:]


def cpu_problems():
    """[(key, dense problem, SOCP pieces or None)]: what the restatement is validated on"""
    out = [("edge80x40_%d" % s, _edge(80, 40, s), None) for s in range(2)]
    d, pieces = socp_numpy(0)
    out.append(("socp102x12", d, pieces))
    out.append(("sdp45x6", sdp_numpy(6, 9, 0), None))
    return out


def bench20(seed):
    """problems.benchmark_lp(20): 40 x 20 over the nonnegative cone"""
    c, G, h = benchmark_lp(20, seed=seed)
    return _D(G, h, c, [RPOS], [40])


# the inputs of "ends at once" (a solve to 1e-5 restarted at 1e-3 stops within two iterations): per family, the candidates -- problems
# the loop brings to 1e-5 within some ten thousand iterations; the CPU test keeps those for which the restatement stops with state OK
# at iteration index <= 1, and asserts that it kept them all
def ends_at_once_candidates():
    return {
        "small": [bench20(0), bench20(1)],
        "mid": [socp_numpy(s)[0] for s in range(2)],
        "sdp": [sdp_numpy(6, 9, s) for s in range(2)],
        "ragged": [_edge(1, 1, 0), bench20(0), socp_numpy(0)[0], sdp_numpy(6, 9, 0), _edge(20, 10, 0)],
        "sparse": [sparse40x30(s) for s in (0, 3)],
        "raggedsparse": [sparse40x30(0), bench20(1), sparse40x30(3)],
    }
