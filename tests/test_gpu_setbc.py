"""GPU: set_bc and solutions / statuses of the six own-A batch families (thip_<family>_set_bc, thip_<family>_solutions).  A range of
problems takes a new (b, c) and keeps its A on the device; the definition everything is held to is the route that existed before:
replace(i, the same A, b, c, rowabs) on every slot -- bit for bit in the preconditioner, the iterate and the status block, at once
and after further iterations, at every workgroup size a family can run, under both state arithmetics -- and, with the iterate kept,
replace(..., start=iterate(i)).  The f64 oracle on (A, b', c') guards against both routes being wrong together; its tolerance is
tests/warm_cases.py::iterate_tol, what the families' own oracle tests hold an iterate to.  solutions() is solution(i) and status(i)
of every problem of a range, bit for bit."""
import numpy as np
import pytest

from ownbatch_cases import F, T, _dense_of, _term_problem  # noqa: F401  (T: the fixture)
from setbc_cases import FAMILIES, RAGGED, Fam, full, param, perturbed, rowsums, same, with_bc
from warm_cases import PSD, iterate_tol, snap_xy

pytestmark = pytest.mark.gpu

RUNNING, OK, EXCESS = -1, 0, 3


@pytest.fixture(scope="module")
def fams(T):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Fam(T, name)
        return made[name]
    return get


def _new(ds):
    return [perturbed(d, i) for i, d in enumerate(ds)]


def _walk(X, Y, P, tag, steps=(1, 10, 50), poll=64):
    """X and Y hold the same state now and after 1, 10 and 50 further iterations"""
    for i in range(P):
        same(full(X, i), full(Y, i), tag + ("at once", i))
    done = 0
    for j in steps:
        X.run(j - done, poll_every=poll)
        Y.run(j - done, poll_every=poll)
        done = j
        for i in range(P):
            same(full(X, i), full(Y, i), tag + (j, i))
            assert X.status(i).iters == j, tag


# ---- 1. fresh, bitwise --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arith", ["plain", "compensated"])
@pytest.mark.parametrize("name", FAMILIES)
def test_fresh_bitwise(T, fams, name, arith):
    fam = fams(name)
    p = param(T, arith)
    for label, ds, _, kws in fam.sets:
        new = _new(ds)
        for kw in kws:
            for forced in fam.forced:
                for poll in (1, 7):
                    X, Y = fam.make(ds, p, forced, **kw), fam.make(ds, p, forced, **kw)
                    try:
                        X.run(10, poll_every=poll)
                        fam.set_bc(X, new)
                        assert X.info()["live"] == len(ds)
                        for i, d in enumerate(new):
                            fam.replace(Y, i, d)
                        for i in range(len(ds)):
                            st = X.status(i)
                            assert (st.state, st.iters, st.kind, st.tau, st.kappa) == (RUNNING, 0, 0, 1.0, 0.0)
                        _walk(X, Y, len(ds), (name, arith, label, str(kw), forced, poll), poll=poll)
                    finally:
                        X.destroy()
                        Y.destroy()


# ---- 2. keep, bitwise, on running problems ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arith", ["plain", "compensated"])
@pytest.mark.parametrize("name", FAMILIES)
def test_keep_bitwise_on_running_problems(T, fams, name, arith):
    fam = fams(name)
    p = param(T, arith)
    for label, ds, _, kws in fam.sets:
        new = _new(ds)
        for kw in kws:
            for forced in fam.forced:
                for poll in (1, 7):
                    X, Y = fam.make(ds, p, forced, **kw), fam.make(ds, p, forced, **kw)
                    try:
                        X.run(10, poll_every=poll)
                        Y.run(10, poll_every=poll)
                        its = [X.iterate(i) for i in range(len(ds))]
                        fam.set_bc(X, new, keep=True)
                        for i, d in enumerate(new):
                            fam.replace(Y, i, d, start=Y.iterate(i))
                        for i in range(len(ds)):                 # the iterate is the one that lay in the arena
                            x, y = X.iterate(i)
                            assert np.array_equal(x, its[i][0]) and np.array_equal(y, its[i][1])
                            st = X.status(i)
                            assert (st.state, st.iters, st.kind, tuple(st.cri)) == (RUNNING, 0, 0, (0.0, 0.0, 0.0))
                        _walk(X, Y, len(ds), (name, arith, label, str(kw), forced, poll), poll=poll)
                    finally:
                        X.destroy()
                        Y.destroy()


# ---- 3. the oracle ------------------------------------------------------------------------------------------------------------------

def _rel(got, want):
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-6)


@pytest.mark.parametrize("name", FAMILIES)
def test_fresh_against_the_oracle(T, fams, name):
    fam = fams(name)
    p = param(T)
    for label, ds, _, kws in fam.sets:
        new = [with_bc(d, d.vec_b, d.vec_c, rowabs=None) for d in _new(ds)]        # (|b'|: the dense oracle's row sums)
        ros = [fam.oracle(label, q, d, None) for q, d in enumerate(new)]
        for kw in kws:
            X = fam.make(ds, p, **kw)
            try:
                X.run(10, poll_every=64)
                fam.set_bc(X, new)
                done = 0
                for it in (0, 1, 9):
                    X.run(it + 1 - done, poll_every=64)
                    done = it + 1
                    for i, (ro, d) in enumerate(zip(ros, new)):
                        x, y = X.iterate(i)
                        rx, ry = snap_xy(ro, d, it)
                        tol = iterate_tol(it, PSD in d.seg_type)
                        ex, ey = _rel(x, rx), _rel(y, ry)
                        print("setbc %s %s %s problem %d iterate %d: err x %.2e y %.2e (tol %.2e)" % (name, label, kw, i, it, ex, ey, tol))
                        assert ex <= tol and ey <= tol, (name, label, i, it, ex, ey)
            finally:
                X.destroy()


# ---- 4. row sums --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["none", "explicit", "mixed"])
@pytest.mark.parametrize("name", FAMILIES)
def test_row_sums(T, fams, name, case):
    fam = fams(name)
    p = param(T)
    label, ds, _, kws = fam.sets[0]
    held = [with_bc(d, d.vec_b, d.vec_c, rowabs=rowsums(d, i)) for i, d in enumerate(ds)]
    new = _new(held)
    for i, d in enumerate(new):
        has = {"none": False, "explicit": True, "mixed": i % 2 == 0}[case]
        new[i] = with_bc(d, d.vec_b, d.vec_c, rowabs=rowsums(d, 10 + i) if has else None)
    for kw in kws:
        X, Y = fam.make(held, p, **kw), fam.make(held, p, **kw)
        try:
            X.run(3, poll_every=3)
            fam.set_bc(X, new)
            for i, d in enumerate(new):
                fam.replace(Y, i, d)
            _walk(X, Y, len(ds), (name, case, str(kw)), steps=(1, 10))
        finally:
            X.destroy()
            Y.destroy()


# ---- 5. a sub-range -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_a_sub_range(T, fams, name):
    fam = fams(name)
    P, first, count = 300, 7, 5
    for kw0 in fam.sets[0][3]:
        cyc, kw = fam.cycled(0, P, kw0)
        new = [perturbed(cyc[first + k], k) for k in range(count)]
        p = param(T)
        X, Y, Z = (fam.make(cyc, p, **kw) for _ in range(3))
        try:
            for sb in (X, Y, Z):
                sb.run(10, poll_every=64)
            fam.set_bc(X, new, first=first)
            for k, d in enumerate(new):
                fam.replace(Y, first + k, d)
            assert X.info()["live"] == P
            for sb in (X, Y, Z):
                sb.run(10, poll_every=64)
            for i in range(P):
                same(full(X, i), full(Y if first <= i < first + count else Z, i), (name, str(kw0), i))
                assert X.status(i).iters == (10 if first <= i < first + count else 20)
        finally:
            for sb in (X, Y, Z):
                sb.destroy()
        # every problem had stopped: the range alone is live again, and the others stay where they stopped
        p = param(T, max_iter=8)
        X, Z = fam.make(cyc, p, **kw), fam.make(cyc, p, **kw)
        try:
            for sb in (X, Z):
                res = sb.run(-1, poll_every=64)
                assert [r.state for r in res] == [EXCESS] * P and sb.info()["live"] == 0
            before = X.info()
            fam.set_bc(X, new, first=first)
            assert X.info()["live"] == count
            assert [r.state for r in X.statuses()] == [RUNNING if first <= i < first + count else EXCESS for i in range(P)]
            X.run(3, poll_every=3)
            after = X.info()
            assert after["live"] == count and after["launches"] - before["launches"] == (2 if name in RAGGED else 1)
            assert after["workgroups"] - before["workgroups"] == count
            res = X.run(-1, poll_every=64)
            assert X.info()["live"] == 0 and [(r.state, r.iters) for r in res] == [(EXCESS, 7)] * P
            for i in range(P):
                if not first <= i < first + count:
                    same(full(X, i), full(Z, i), (name, "stopped", i))
        finally:
            X.destroy()
            Z.destroy()


# ---- 6. a stopped slot runs again ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_a_stopped_slot_runs_again(T, fams, name):
    from tau_zero_problems import _lp_layout
    from tau_zero_problems import family as tz_family
    from totsu_amd import _lib
    fam = fams(name)
    label, ds, _, kws = fam.sets[0]
    f1 = _dense_of(tz_family("F1"))                              # the infeasible LP, 128 x 64: its iteration ends through tau = 0
    f1.vec_b_rowabs = None
    feasible = with_bc(f1, _lp_layout(64, 126, 1)[4], f1.vec_c)  # the same A with the b its construction started from
    kw1 = {"nnz_caps": [0, 0]} if name == "raggedsparse" else {}
    cases = [("excess", ds, _new(ds), param(T, max_iter=5), kw, _lib.ST_EXCESS_ITER, 0) for kw in kws] + \
            [("tau zero", [f1, f1], [feasible, feasible], param(T, eps_acc=1e-5, eps_inf=1e-5, max_iter=5000),
              dict(kw1, **{k: v for k, v in kw.items() if k != "nnz_caps"}), _lib.ST_INFEASIBLE, 1) for kw in kws]
    for what, held, new, p, kw, state, kind in cases:
        X, Y, W = (fam.make(held, p, **kw) for _ in range(3))
        try:
            for sb in (X, Y, W):
                res = sb.run(-1, poll_every=64)
                assert [r.state for r in res] == [state] * len(held) and res[0].kind == kind, (what, [(r.state, r.kind, r.iters) for r in res])
            raws = [W.raw_iterate(i) for i in range(len(held))]
            assert all((x[-1] <= 1e-12) == (kind == 1) for x, _ in raws)
            fam.set_bc(W, new, keep=True)                        # kept: the arena's iterate, running at iteration 0, and it stops again
            for i in range(len(held)):
                st = W.status(i)
                assert (st.state, st.iters, st.kind, tuple(st.cri)) == (RUNNING, 0, 0, (0.0, 0.0, 0.0)), (what, i)
                x, y = W.iterate(i)
                assert x[-1] == raws[i][0][-1] and y[-1] == raws[i][1][-1]
                nm = held[i].n + held[i].m                       # (the raw iterate is the arena's to one rounding: x_s, u, v exactly)
                assert np.array_equal(x[nm:], raws[i][0][nm:]) and np.array_equal(y, raws[i][1])
                assert np.allclose(x[:nm], raws[i][0][:nm], rtol=3e-7, atol=0)
            assert W.info()["live"] == len(held)
            res = W.run(-1, poll_every=64)
            assert all(r.state != RUNNING for r in res) and W.info()["live"] == 0, what
            fam.set_bc(X, new)                                   # fresh: the replace route, bit for bit
            for i, d in enumerate(new):
                fam.replace(Y, i, d)
            _walk(X, Y, len(held), (name, what, str(kw)), steps=(1, 4))
        finally:
            for sb in (X, Y, W):
                sb.destroy()


# ---- 7. then replace, then set_bc again ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_then_replace_then_set_bc_again(T, fams, name):
    fam = fams(name)
    p = param(T)
    label, ds, _, kws = fam.sets[0]
    P = len(ds)
    one, two, three = _new(ds), [perturbed(d, 20 + i) for i, d in enumerate(ds)], [perturbed(d, 40 + i) for i, d in enumerate(ds)]
    for kw in kws:
        X, Y = fam.make(ds, p, **kw), fam.make(ds, p, **kw)
        try:
            def step(data, by_set_bc):
                for i, d in enumerate(data):
                    fam.replace(Y, i, d)
                if by_set_bc:
                    fam.set_bc(X, data)
                else:
                    for i, d in enumerate(data):
                        fam.replace(X, i, d)
                _walk(X, Y, P, (name, str(kw)), steps=(1, 5))
            dev0 = X.info()["device_bytes"]
            step(one, True)
            dev1 = X.info()["device_bytes"]
            store = sum(2 * d.m + d.n for d in ds) * 4
            assert dev1 - dev0 >= store + sum(2 * d.m + d.n + 1 for d in ds) * 4, (dev0, dev1)      # the store and the staging buffer
            step(two, False)                                     # the slots point at caller memory again
            assert X.info()["device_bytes"] == dev1
            step(three, True)
            assert X.info()["device_bytes"] == dev1
            fam.set_bc(X, one[P - 1:], first=P - 1)                   # (a smaller call fits the staging buffer that is there)
            assert X.info()["device_bytes"] == dev1
        finally:
            X.destroy()
            Y.destroy()


# ---- 8. solutions() -----------------------------------------------------------------------------------------------------------------

def _check_solutions(sb, P, tag):
    want = [sb.solution(i) for i in range(P)]
    stat = [sb.status(i) for i in range(P)]
    for first, count in ((0, None), (P // 3, max(1, P // 4)), (P - 1, 1)):
        got = sb.solutions(first, count)
        sts = sb.statuses(first, count)
        n = P - first if count is None else count
        assert len(got) == len(sts) == n
        for k in range(n):
            i = first + k
            assert np.array_equal(got[k][0], want[i][0]) and np.array_equal(got[k][1], want[i][1]), (tag, first, i)
            a, b = sts[k], stat[i]
            assert (a.state, a.iters, a.kind, a.cri, a.tau, a.kappa, a.norm_b, a.norm_c) == \
                (b.state, b.iters, b.kind, b.cri, b.tau, b.kappa, b.norm_b, b.norm_c), (tag, first, i)
    return stat


@pytest.mark.parametrize("name", FAMILIES)
def test_solutions(T, fams, name):
    fam = fams(name)
    if name in RAGGED:                                           # the set as it is: stopped by max_iter, some restarted and running
        label, ds, _, kws = fam.sets[0]
        for kw in kws:
            sb = fam.make(ds, param(T, max_iter=12), **kw)
            try:
                sb.run(-1, poll_every=64)
                fam.set_bc(sb, ds[1:3], first=1)
                sb.run(3, poll_every=3)
                stat = _check_solutions(sb, len(ds), (name, str(kw)))
                assert sorted({s.state for s in stat}) == [RUNNING, EXCESS]
            finally:
                sb.destroy()
        return
    # one shape, P = 300: the infeasible (tau -> 0), the feasible and the unbounded box in turn, solved; then some restarted and
    # stopped by max_iter, and some of those restarted again and running
    P = 300
    ds = [_term_problem(i) for i in range(P)]
    for kw in fam.sets[0][3]:
        sb = fam.make(ds, param(T, eps_acc=1e-5, eps_inf=1e-5, max_iter=100000), **kw)
        try:
            res = sb.run(-1, poll_every=64)
            assert sorted({r.state for r in res}) == [0, 1, 2]
            fam.set_bc(sb, ds[:30])
            sb.set_param(param(T, eps_acc=1e-5, eps_inf=1e-5, max_iter=5))
            sb.run(-1, poll_every=5)
            fam.set_bc(sb, ds[:9])
            sb.run(2, poll_every=2)
            stat = _check_solutions(sb, P, (name, str(kw)))
            assert [s.state for s in stat[:9]] == [RUNNING] * 9 and [s.state for s in stat[9:30]] == [EXCESS] * 21
            assert {s.state for s in stat[30:]} == {0, 1, 2} and any(s.kind == 1 and s.tau == 0.0 for s in stat[30:])
        finally:
            sb.destroy()


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_refusals(T, fams, name, monkeypatch):
    from totsu_amd import _lib
    fam = fams(name)
    label, ds, _, kws = fam.sets[0]
    new = _new(ds)
    P = len(ds)
    for kw in kws:
        sb = fam.make(ds, param(T), **kw)
        try:
            sb.run(2, poll_every=2)
            info = sb.info()
            dev, dev_all = info["device_bytes"], info["device_bytes_all"]
            want = [full(sb, i) for i in range(P)]
            b, c = [d.vec_b for d in new], [d.vec_c for d in new]

            def unchanged():
                now = sb.info()
                assert (now["device_bytes"], now["device_bytes_all"], now["live"]) == (dev, dev_all, P)
                for i in range(P):
                    same(full(sb, i), want[i])

            def bad(match, *a, **k):
                with pytest.raises(ValueError, match=match):
                    sb.set_bc(*a, **k)
                unchanged()
            last = P - 1
            bad("problem %d" % last, b[:last] + [np.append(b[last], F(1))], c)             # wrong lengths, naming the problem
            bad("problem 0", b, [c[0][:-1]] + c[1:]) if c[0].size > 1 else None
            bad("problem %d" % last, b, c, [None] * last + [np.zeros(b[last].size + 1, F)])
            bad("no problems", b, c, first=1)                                               # a range past the end
            bad("no problems", b[:1], c[:1], first=P)
            bad("no problems", b[:1], c[:1], first=-1)
            bad("at least one", [], [])                                                     # count = 0
            bad("one pair per problem", b, c[:-1]) if P > 1 else None
            for a in ((P, 1), (0, P + 1), (-1, 1), (0, 0)):
                with pytest.raises(ValueError):
                    sb.solutions(*a)
                with pytest.raises(ValueError):
                    sb.statuses(*a)
            fn = getattr(_lib.load(), sb._prefix + "set_bc")
            sol = getattr(_lib.load(), sb._prefix + "solutions")
            fb, fc = np.concatenate(b), np.concatenate(c)
            pb, pc = fb.ctypes.data, fc.ctypes.data
            for args in ((sb.h, P, 1), (sb.h, 0, 0), (sb.h, 0, -1), (sb.h, -1, 1), (sb.h, 0, P + 1), (None, 0, 1)):
                assert fn(args[0], args[1], args[2], pb, pc, None, None, 0) == _lib.E_INVALID, args
                assert sol(args[0], args[1], args[2], None, None, None) == _lib.E_INVALID, args
            assert fn(sb.h, 0, 1, None, pc, None, None, 0) == _lib.E_INVALID
            assert fn(sb.h, 0, 1, pb, None, None, None, 1) == _lib.E_INVALID
            unchanged()
            # a handle that was created and not initialised: the family's own constructor with its init call left out
            with monkeypatch.context() as mp:
                mp.setattr(_lib.lib, sb._prefix + "init", lambda h: 0, raising=False)
                raw = fam.make(ds, param(T), **kw)
            try:
                assert fn(raw.h, 0, 1, pb, pc, None, None, 0) == _lib.E_INVALID
                assert sol(raw.h, 0, 1, None, None, None) == _lib.E_INVALID
                with pytest.raises(ValueError):
                    fam.set_bc(raw, new)
            finally:
                raw.destroy()
            unchanged()
            sb.run(2, poll_every=2)                              # and the batch still runs, and takes a set_bc
            assert [sb.status(i).iters for i in range(P)] == [4] * P
            fam.set_bc(sb, new)
            assert [s.iters for s in sb.statuses()] == [0] * P and sb.info()["device_bytes"] > dev
        finally:
            sb.destroy()
