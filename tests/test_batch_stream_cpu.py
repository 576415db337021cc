"""CPU: what streaming problems through the slots of a batch (totsu_amd.solve_many, BatchSolver.stream / replace, regroup=True) rests
on and that needs no GPU -- the regroup rule (thip_batch_live_grouping) and the slot-filling policy against a stub batch."""
import numpy as np
import pytest

from totsu_amd import _lib


@pytest.mark.parametrize("max_group", [8, 4, 2])
def test_live_groups_for_every_batch_size_and_mask(max_group):
    from totsu_amd.batch import group_sizes, live_groups
    rng = np.random.default_rng(max_group)
    for B in range(1, 65):
        masks = [np.ones(B, bool), np.zeros(B, bool)] + [rng.random(B) < p for p in (0.1, 0.5, 0.9)]
        for live in masks:
            g = live_groups(list(live), max_group)
            want = [int(i) for i in np.flatnonzero(live)]
            # members: exactly the live indices, ascending, in launch order
            assert [i for grp in g for i in grp] == want, (B, live, g)
            # full groups first, the rest last; ceil(live / max_group) launches per pass
            L = len(want)
            assert [len(grp) for grp in g] == [max_group] * (L // max_group) + ([L % max_group] if L % max_group else []), (B, g)
            assert len(g) == -(-L // max_group)
        assert [len(grp) for grp in live_groups([1] * B, max_group)] == group_sizes(B, max_group)
        assert live_groups([0] * B, max_group) == []
    # the case of the issue: 11 instances, the live count falling to 9, 5, 2
    live = [1] * 11
    for dead, want in (((5, 9), [8, 1]), ((1, 0, 2, 3), [5]), ((4, 6, 7), [2])):
        for i in dead:
            live[i] = 0
        assert [len(grp) for grp in live_groups(live, 8)] == want


def test_live_groups_refuses_bad_arguments():
    import ctypes as C
    from totsu_amd._lib import lib
    from totsu_amd.batch import live_groups
    for live, g in (([], 8), ([1] * 65, 8), ([1] * 4, 3), ([1] * 4, 16), ([1] * 4, 0)):
        with pytest.raises(_lib.ThipError) as e:
            live_groups(live, g)
        assert e.value.code == _lib.E_INVALID
    one, n = (C.c_int * 4)(1, 1, 1, 1), C.c_int()
    for args in ((4, 8, None, C.byref(n), None, None), (4, 8, one, None, None, None)):      # null live flags, null group count
        with pytest.raises(_lib.ThipError) as e:
            lib.thip_batch_live_grouping(*args)
        assert e.value.code == _lib.E_INVALID
    lib.thip_batch_live_grouping(4, 8, one, C.byref(n), None, None)                          # sizes and members are optional
    assert n.value == 1


class _Res:
    def __init__(self, state, iters):
        self.state, self.iters = state, iters


class _StubBatch:
    """n_inst slots whose occupants stop after scripted iteration counts: problem (b, c) = ([k], [count]) stops after `count`
    iterations.  run_until_any advances every running slot in steps of poll_every and returns at the first poll at which a slot that
    was running has stopped.  Records what the policy did to it."""

    def __init__(self, problems):
        self.n_inst = len(problems)
        self.prob = [int(b[0]) for b, _ in problems]
        self.need = [int(c[0]) for _, c in problems]
        self.iters = [0] * self.n_inst
        self.placed = list(self.prob)                    # every problem ever put into a slot
        self.log = []                                    # ("run", stopped slots at return) / ("replace", slot)
        self.max_in_flight = self.n_inst

    def _running(self, i):
        return self.iters[i] < self.need[i]

    def run_until_any(self, max_steps=-1, poll_every=16):
        assert max_steps < 0
        was = [self._running(i) for i in range(self.n_inst)]
        while any(self._running(i) for i in range(self.n_inst)) and not any(w and not self._running(i) for i, w in enumerate(was)):
            for i in range(self.n_inst):
                if self._running(i):
                    self.iters[i] = min(self.iters[i] + poll_every, self.need[i])
        self.log.append(("run", [i for i in range(self.n_inst) if not self._running(i)]))
        return [self.status(i) for i in range(self.n_inst)]

    def status(self, i):
        return _Res(_lib.ST_RUNNING if self._running(i) else _lib.ST_OK, self.iters[i])

    def solution(self, i):
        assert not self._running(i)
        return np.array([self.prob[i]], np.float32), np.array([self.iters[i]], np.float32)

    def replace(self, i, b, c):
        assert not self._running(i)                      # the policy only ever refills a slot whose problem has stopped
        self.prob[i], self.need[i], self.iters[i] = int(b[0]), int(c[0]), 0
        self.placed.append(int(b[0]))
        self.log.append(("replace", i))


def _problems(counts):
    return [(np.array([k], np.float32), np.array([c], np.float32)) for k, c in enumerate(counts)]


def _drive(counts, slots, poll_every=8, lazy=False):
    from totsu_amd.batch import stream_slots
    probs = _problems(counts)
    s = min(slots, len(probs))
    stub = _StubBatch(probs[:s])
    rest = probs[s:]
    pulled = []

    def gen():
        for p in rest:
            pulled.append(int(p[0][0]))
            yield p

    got = list(stream_slots(stub, gen() if lazy else rest, poll_every))
    return stub, got, pulled


@pytest.mark.parametrize("counts,slots", [
    ([70, 200, 30, 90, 16, 17, 300, 8, 8, 120, 45], 4),      # more problems than slots, several stopping at the same poll
    ([50, 20, 90], 8),                                     # fewer problems than slots
    ([33], 4),                                             # exactly one problem
    ([10, 20, 30, 40, 50, 60, 70, 80], 8),                 # as many as slots
    (list(range(1, 41)), 3),
])
def test_slot_filling_policy(counts, slots):
    stub, got, _ = _drive(counts, slots)
    n = len(counts)
    # every problem is placed exactly once, and comes back exactly once with its own result
    assert sorted(stub.placed) == list(range(n))
    assert sorted(k for k, _, _, _ in got) == list(range(n))
    for k, r, x, y in got:
        assert int(x[0]) == k and r.state == _lib.ST_OK and r.iters == counts[k] == int(y[0])
    # never more in flight than there are slots
    assert stub.n_inst == min(slots, n)
    # a stopped slot is refilled at the very next return while problems remain: between a run that found slots stopped and the next
    # run, those slots are replaced -- as many of them as there are problems left
    left = n - stub.n_inst
    seen = set()                                           # slots read out and left empty (nothing to refill them with)
    for q, ev in enumerate(stub.log):
        if ev[0] != "run":
            continue
        stopped = [i for i in ev[1] if i not in seen]
        refills = []
        for nxt in stub.log[q + 1:]:
            if nxt[0] == "run":
                break
            refills.append(nxt[1])
        take = min(left, len(stopped))
        assert refills == stopped[:take], (q, ev, refills)
        left -= take
        seen.update(stopped[take:])
    assert left == 0
    # in input order once sorted by k: what solve_many does
    out = [None] * n
    for k, r, x, y in got:
        out[k] = r.iters
    assert out == counts


def test_slot_filling_takes_a_lazy_iterator_no_further_than_needed():
    counts = [40, 8, 80, 16, 24, 8, 8]
    stub, got, pulled = _drive(counts, 2, lazy=True)
    assert sorted(k for k, _, _, _ in got) == list(range(7))
    assert pulled == [2, 3, 4, 5, 6]
    # a problem is pulled from the iterator only when a slot is free for it: stop consuming after the first result
    from totsu_amd.batch import stream_slots
    probs = _problems(counts)
    stub = _StubBatch(probs[:2])
    pulled = []

    def gen():
        for p in probs[2:]:
            pulled.append(int(p[0][0]))
            yield p

    it = stream_slots(stub, gen(), 8)
    k, r, x, y = next(it)
    assert k == 1 and pulled == [2]                        # slot 1 (8 iterations) stopped first and took problem 2


def test_solve_many_refuses_without_touching_a_device():
    from types import SimpleNamespace
    from totsu_amd import solve_many
    d = SimpleNamespace(n=2, m=4, mat_a=np.zeros(8, np.float32), seg_type=[_lib.CONE_RPOS], seg_len=[4])
    b, c = np.ones(4, np.float32), np.ones(2, np.float32)
    for kw in (dict(vecs_b=[b], vecs_c=[c], slots=0), dict(vecs_b=[b], vecs_c=[c], slots=65), dict(vecs_b=[], vecs_c=[]),
               dict(vecs_b=[b, b], vecs_c=[c])):
        with pytest.raises(ValueError):
            solve_many(d, **kw)
