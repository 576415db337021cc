"""CPU: the f64 restatement of the loop that takes a start (tests/warm_numpy.py) against the oracle -- from the zero start, from the
oracle's own snapshots, and under a positive scaling of the start -- and the precondition of the GPU test "ends at once" on its
inputs.  The oracle has no start-iterate input; it returns snapshots, and a start at its iterate after iteration k followed by j
iterations must give its snapshot at k + j."""
import numpy as np
import pytest

import warm_numpy as W
from warm_cases import J_RUN, K_START, SNAPS, cpu_problems, ends_at_once_candidates, oracle_run, snap_xy

TOL = 1e-9            # of the snapshot's max norm: f64 against f64, the same projections


def _err(got, want):
    return max(np.abs(got[0] - want[0]).max() / max(np.abs(want[0]).max(), 1e-6), np.abs(got[1] - want[1]).max() / max(np.abs(want[1]).max(), 1e-6))


@pytest.fixture(scope="module")
def cases():
    return [(key, d, W.Problem.of_dense(d), oracle_run(key, d, socp=pieces)) for key, d, pieces in cpu_problems()]


def test_zero_start_reproduces_the_oracle(cases):
    for key, d, p, ro in cases:
        r = W.run(p, max(SNAPS) + 1, snap_iters=(0, 1, 9, 19))
        pc = ro.precond
        N = d.n + 2 * d.m + 1
        assert np.allclose(np.concatenate([p.Tx, p.Ty, p.Ts, [p.t_tau]]), pc[:N], rtol=1e-12, atol=0), key
        assert np.allclose(np.concatenate([p.Tx, p.Sv, [p.s_kappa]]), pc[N:], rtol=1e-12, atol=0), key
        for it in (0, 1, 9, 19):
            e = _err(r.snaps[it], snap_xy(ro, d, it))
            print("%s zero start, iterate %d: err %.2e" % (key, it, e))
            assert e <= TOL, (key, it, e)
        tr = ro.trace[19]
        assert r.kind == tr[1] and np.allclose(r.cri, tr[2:], rtol=1e-7, atol=1e-12), (key, r.cri, tr)


def test_start_at_a_snapshot_reproduces_the_later_snapshot(cases):
    for key, d, p, ro in cases:
        for k in K_START:
            for j in J_RUN:
                r = W.run(p, j, start=snap_xy(ro, d, k), snap_iters=(j - 1,))
                e = _err(r.snaps[j - 1], snap_xy(ro, d, k + j))
                print("%s start at %d, %d iterations: err %.2e" % (key, k, j, e))
                assert e <= TOL, (key, k, j, e)
                assert r.iters == j - 1 and r.state == W.RUNNING
                tr = ro.trace[k + j]
                assert r.kind == tr[1] and np.allclose(r.cri, tr[2:], rtol=1e-7, atol=1e-12), (key, k, j)


def test_homogeneity(cases):
    # the iteration is positively homogeneous: a start scaled by 1 / tau gives iterates scaled by 1 / tau, and the same criteria --
    # which licenses raw_iterate and any other positive scaling of a start
    for key, d, p, ro in cases:
        x, y = snap_xy(ro, d, 9)
        s = 1.0 / x[-1]
        a = W.run(p, 10, start=(x, y))
        b = W.run(p, 10, start=(s * x, s * y))
        for g, w in ((b.x, s * a.x), (b.y, s * a.y)):
            assert np.abs(g - w).max() <= 1e-12 * np.abs(w).max(), key
        assert np.allclose(a.cri, b.cri, rtol=1e-9, atol=1e-15), key


def test_ends_at_once_precondition():
    # the inputs of tests/test_gpu_warm_start.py::test_ends_at_once: solved to 1e-5, restarted from that iterate at 1e-3, the
    # restatement stops with state OK at iteration index <= 1
    for fam, ds in ends_at_once_candidates().items():
        for q, d in enumerate(ds):
            p = W.Problem.of_dense(d)
            first = W.run(p, 200000, eps_acc=1e-5, eps_inf=1e-5)
            assert first.state == W.OK, (fam, q, first.state, first.iters)
            again = W.run(p, 100, start=(first.x, first.y), eps_acc=1e-3, eps_inf=1e-3)
            print("%s %d (%d x %d): %d iterations to 1e-5, then stops at index %d" % (fam, q, d.m, d.n, first.iters + 1, again.iters))
            assert again.state == W.OK and again.iters <= 1, (fam, q, again.state, again.iters)
            sol = W.solution(first, d.n, d.m)
            assert np.abs(W.solution(again, d.n, d.m) - sol).max() <= 1e-3 * max(1.0, np.abs(sol).max()), (fam, q)
            # the device may stop up to two iterations later (iters <= 2): the answer must not be travelling while the criteria hold,
            # as that of a box LP with a nearly free coordinate does -- 3e-3 per iteration at the first iterate under 1e-5
            more = W.run(p, 3, start=(first.x, first.y), snap_iters=(0, 1, 2))
            for it in range(3):
                moved = np.abs(more.snaps[it][0][:d.n] / more.snaps[it][0][-1] - sol).max()
                assert moved <= 0.5e-3 * max(1.0, np.abs(sol).max()), (fam, q, it, moved)


# ---- the warm slot policy on a stub (the pattern of tests/test_batch_stream_cpu.py) ---------------------------------------------

class _Res:
    def __init__(self, state, iters):
        self.state, self.iters = state, iters


class _WarmStub:
    """slots whose occupants stop after scripted iteration counts, problem (b, c) = ([k], [count, final state]); raw_iterate(i) is a
    token that names the slot's occupant.  Records every replace with the start it was given"""

    def __init__(self, problems):
        self.n_inst = len(problems)
        self.prob, self.need, self.end = [int(b[0]) for b, _ in problems], [int(c[0]) for _, c in problems], [int(c[1]) for _, c in problems]
        self.iters = [0] * self.n_inst
        self.replaced = []                               # (slot, new problem, start or None)
        self.raw_reads = []

    def _running(self, i):
        return self.iters[i] < self.need[i]

    def run_until_any(self, max_steps=-1, poll_every=16):
        was = [self._running(i) for i in range(self.n_inst)]
        while any(self._running(i) for i in range(self.n_inst)) and not any(w and not self._running(i) for i, w in enumerate(was)):
            for i in range(self.n_inst):
                if self._running(i):
                    self.iters[i] = min(self.iters[i] + poll_every, self.need[i])
        return [_Res(-1 if self._running(i) else self.end[i], self.iters[i]) for i in range(self.n_inst)]

    def solution(self, i):
        assert not self._running(i)
        return np.array([self.prob[i]], np.float32), np.array([self.iters[i]], np.float32)

    def raw_iterate(self, i):
        assert not self._running(i)
        self.raw_reads.append((i, self.prob[i]))
        return ("x of", i, self.prob[i]), ("y of", i, self.prob[i])

    def replace(self, i, b, c, start=None):
        assert not self._running(i)
        self.replaced.append((i, int(b[0]), start))
        self.prob[i], self.need[i], self.end[i], self.iters[i] = int(b[0]), int(c[0]), int(c[1]), 0


def _stub_problems(counts, ends):
    return [(np.array([k], np.float32), np.array([c, e], np.float32)) for k, (c, e) in enumerate(zip(counts, ends))]


@pytest.mark.parametrize("slots", [1, 3, 8])
def test_warm_slot_policy(slots):
    from totsu_amd.batch import stream_slots
    counts = [70, 200, 30, 90, 16, 17, 300, 8, 8, 120, 45]
    ends = [0, 3, 0, 0, 2, 0, 1, 0, 0, 3, 0]             # OK, ExcessIter, Infeasible, Unbounded among them
    probs = _stub_problems(counts, ends)
    s = min(slots, len(probs))
    runs = {}
    for warm in (False, True):
        stub, pulled = _WarmStub(probs[:s]), []

        def gen():
            for p in probs[s:]:
                pulled.append(int(p[0][0]))
                yield p
        got = list(stream_slots(stub, gen(), 8, warm=warm))
        runs[warm] = (stub, got, pulled)
        assert sorted(k for k, _, _, _ in got) == list(range(len(counts)))
        for k, r, x, y in got:
            assert int(x[0]) == k and r.state == ends[k] and r.iters == counts[k]
    cold, warm = runs[False], runs[True]
    # order of results, what was pulled when, and which slot took which problem are those of the cold policy
    assert [k for k, _, _, _ in cold[1]] == [k for k, _, _, _ in warm[1]] and cold[2] == warm[2]
    assert [(i, k) for i, k, _ in cold[0].replaced] == [(i, k) for i, k, _ in warm[0].replaced]
    assert all(st is None for _, _, st in cold[0].replaced) and cold[0].raw_reads == []
    # the slot's own last raw iterate is handed over exactly when the occupant ended OK
    prev = {i: i for i in range(s)}                      # the occupant of each slot before a replace
    for i, k, st in warm[0].replaced:
        if ends[prev[i]] == 0:
            assert st == (("x of", i, prev[i]), ("y of", i, prev[i])), (i, k, st)
        else:
            assert st is None, (i, k, st)
        prev[i] = k
    assert len(warm[0].raw_reads) == sum(1 for _, _, st in warm[0].replaced if st is not None)


def test_warm_is_lazy():
    from totsu_amd.batch import stream_slots
    probs = _stub_problems([40, 8, 80, 16, 24], [0, 0, 0, 0, 0])
    stub, pulled = _WarmStub(probs[:2]), []

    def gen():
        for p in probs[2:]:
            pulled.append(int(p[0][0]))
            yield p
    it = stream_slots(stub, gen(), 8, warm=True)
    k, r, x, y = next(it)
    assert k == 1 and pulled == [2] and stub.replaced == [(1, 2, (("x of", 1, 1), ("y of", 1, 1)))]


def test_wrong_lengths_are_refused_before_anything_is_uploaded():
    # the checks of set_iterate / replace(start=) that need no device: on objects that were never given a handle
    from totsu_amd.fused import _start_arrays
    from totsu_amd.ownbatch import OwnBatchSolver
    x, y = np.zeros(3 + 2 * 5 + 1, np.float32), np.zeros(3 + 5 + 1, np.float32)
    assert _start_arrays(3, 5, x, y)[0].dtype == np.float32
    for bx, by in ((x[:-1], y), (x, y[:-1]), (np.zeros(0), y)):
        with pytest.raises(ValueError):
            _start_arrays(3, 5, bx, by)
    sb = OwnBatchSolver.__new__(OwnBatchSolver)
    sb.n, sb.m, sb.n_prob, sb.h = 3, 5, 4, None
    for args in (([x[:-1]], [y], 0), ([x], [y, y], 0), ([], [], 0), ([x, x], [y, y], 3), ([x], [y], -1), ([x], [y], 4)):
        with pytest.raises(ValueError):
            sb.set_iterates(args[0], args[1], first=args[2])
    with pytest.raises(ValueError):
        sb.set_iterate(4, x, y)
    with pytest.raises(ValueError):
        sb.replace(0, np.zeros(15), np.zeros(5), np.zeros(3), start=(x, y[:-1]))
