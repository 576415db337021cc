"""GPU: many small problems, each with its OWN A, iterated on chip (totsu_amd.SmallBatchSolver / thip_smallbatch_*): every problem's
iterates against the f64 oracle, edge shapes, independent termination, isolation from the neighbours, steps and limits, replace,
the refusals.  Every oracle state a test relies on is asserted first (confirmed on the CPU).  The families, the oracle runs and the
helpers are those of tests/ownbatch_cases.py."""
import numpy as np
import pytest

import oracle as O
from ownbatch_cases import F, ITERS, TOLS, T, _D, _edge, _lp_arrays, _oracle, _term_problem, check_against_oracle  # noqa: F401
from ownbatch_cases import family as _family

pytestmark = pytest.mark.gpu


def _check(T, label, ds, ros, iters, tols, **kw):
    check_against_oracle(T, T.SmallBatchSolver, label, ds, ros, iters, tols, **kw)


# ---- 1. iterates against the oracle, every problem with its own A -----------------------------------------------------------

@pytest.mark.parametrize("name", ["lp20", "lp40", "socp", "qp"])
def test_iterates_own_a(T, name):
    ds, ros = _family(T, name)
    _check(T, name, ds, ros, ITERS, TOLS)


@pytest.mark.parametrize("threads", [64, 256, 1024])
@pytest.mark.parametrize("name", ["lp20", "socp"])
def test_iterates_every_workgroup_size(T, name, threads):
    ds, ros = _family(T, name)
    _check(T, "%s/%d threads" % (name, threads), ds, ros, ITERS, TOLS, force_threads=threads)


def test_iterates_plain_state(T):
    ds, ros = _family(T, "lp40")
    _check(T, "lp40/plain", ds, ros, ITERS, TOLS, state_arith="plain")


# ---- 2. edge shapes ----------------------------------------------------------------------------------------------------------

EDGE_SHAPES = [(1, 1), (2, 1), (3, 2), (65, 33), (129, 190), (192, 128), (1024, 24), (24, 1024)]


@pytest.mark.parametrize("m,n", EDGE_SHAPES)
def test_edge_shapes(T, m, n):
    """one row, one column, m * n odd (an A that is not 16-byte aligned from the second problem on), more rows / columns than a
    workgroup's slices cover at once, the area limit, the longest rows and the longest columns"""
    ds = [_edge(m, n, s) for s in range(3)]
    ros = [_oracle(d, ITERS[:3]) for d in ds]
    _check(T, "edge %dx%d" % (m, n), ds, ros, ITERS[:3], TOLS[:3])


@pytest.mark.parametrize("m,n", [(1, 1), (2, 1), (3, 2), (24, 1024)])
def test_edge_shapes_converge(T, m, n):
    ds = [_edge(m, n, s) for s in range(3)]
    ros = [O.solve_matop_cones(O.param(max_iter=100000, eps_acc=1e-4), d.vec_c, d.mat_a, d.vec_b, d.seg_type, d.seg_len) for d in ds]
    for ro in ros:
        assert ro.status == O.OK and ro.iters <= 339
    p = T.SolverParam()
    p.max_iter, p.eps_acc = 100000, 1e-4
    sb = T.SmallBatchSolver.from_dense(ds, p)
    res = sb.run(-1, poll_every=32)
    for i, d in enumerate(ds):
        assert res[i].state == ros[i].status, (i, res[i].state)
        x, y = sb.solution(i)
        fs = T.FusedSolver(d.n, d.m, d.mat_a, d.vec_b, d.vec_c, d.seg_type, d.seg_len, p, "carried")
        xf, yf = fs.solve()
        fs.destroy()
        print("edge %dx%d problem %d: %d iterations (oracle %d), |x - x_carried| %.2e |y - y_carried| %.2e"
              % (m, n, i, res[i].iters, ros[i].iters, np.abs(x - xf).max(), np.abs(y - yf).max()))
        assert np.allclose(x, xf, atol=1e-3) and np.allclose(y, yf, atol=1e-3)
    sb.destroy()


# ---- 3. independent termination ------------------------------------------------------------------------------------------------

def test_independent_termination(T):
    from totsu_amd import _lib
    P = 18
    ds = [_term_problem(i) for i in range(P)]
    ros = [O.solve_matop_cones(O.param(max_iter=100000, eps_acc=1e-5, eps_inf=1e-5), d.vec_c, d.mat_a, d.vec_b, d.seg_type, d.seg_len,
                               trace_cap=400) for d in ds]
    want = [O.INFEASIBLE, O.OK, O.UNBOUNDED]
    for i, ro in enumerate(ros):                       # (the oracle: 54-73, 112-187 and 31-38 iterations)
        assert ro.status == want[i % 3] and ro.iters < 399, (i, ro.status_name, ro.iters)
    p = T.SolverParam()
    p.max_iter, p.eps_acc, p.eps_inf = 100000, 1e-5, 1e-5
    sb = T.SmallBatchSolver.from_dense(ds, p)
    early, wg, live = {}, [0], [P]
    while True:
        res = sb.run_until_any(8, poll_every=8)        # 8 iterations at a time, back as soon as something has stopped
        info = sb.info()
        wg.append(info["workgroups"])
        live.append(info["live"])
        assert wg[-1] - wg[-2] == live[-2]             # one workgroup per problem that was running: they fall with the live set
        for i, r in enumerate(res):
            if r.state != _lib.ST_RUNNING and i not in early:
                early[i] = (r.state, r.iters, r.kind) + sb.iterate(i)
        if all(r.state != _lib.ST_RUNNING for r in res):
            break
        assert len(wg) < 200
    assert live[0] == P and live[-1] == 0 and len(set(live)) >= 3 and live == sorted(live, reverse=True)
    iters = [r.iters for r in res]
    print("independent termination: iterations", iters, "oracle", [ro.iters for ro in ros])
    for i, ro in enumerate(ros):
        assert res[i].state == ro.status, (i, res[i].state, ro.status_name)
        assert res[i].kind == ro.trace[-1][1], (i, res[i].kind)
        st, it, kind, x, y = early[i]                  # what the problem held when it was first seen stopped
        x2, y2 = sb.iterate(i)
        assert (st, it, kind) == (res[i].state, res[i].iters, res[i].kind)
        assert np.array_equal(x, x2) and np.array_equal(y, y2)
    assert len(set(iters)) >= 3                        # they stopped at their own times
    sols = sb.solve()                                  # nothing runs any more: the list of solutions / errors
    for i, s_ in enumerate(sols):
        if i % 3 == 1:
            assert isinstance(s_, tuple) and np.allclose(s_[0], ros[i].x, atol=1e-3)
        else:
            assert isinstance(s_, T.SolverError)
    sb.destroy()


# ---- 4. isolation and reproducibility ------------------------------------------------------------------------------------------

def test_isolation_and_reproducibility(T):
    from totsu_amd import _lib
    P = 300                                            # more workgroups than the device has CUs
    seeds = list(range(P))
    seeds[P - 1] = 0                                   # the same LP at index 0 and at index 299
    a, b, c = _lp_arrays(seeds)
    p = T.SolverParam()
    p.max_iter, p.eps_acc = 1500, 1e-3                 # (the oracle needs 400 .. 8000 iterations at 1e-3: both endings occur)
    seg = ([_lib.CONE_RPOS], [40])

    def run(aa, bb, cc, idx):
        sb = T.SmallBatchSolver(20, 40, aa, bb, cc, seg[0], seg[1], p)
        sb.run(100, poll_every=50)
        mid = [sb.iterate(i) for i in idx]
        assert all(sb.status(i).iters == 100 for i in idx)
        res = sb.run(-1, poll_every=100)
        out = [(mid[k], (res[i].state, res[i].iters), sb.solution(i)) for k, i in enumerate(idx)]
        states = [r.state for r in res]
        sb.destroy()
        return out, states, [r.iters for r in res]

    alone, _, _ = run(a[:1], b[:1], c[:1], [0])
    first, states, iters = run(a, b, c, [0, P - 1])
    second, _, _ = run(a, b, c, [0, P - 1])
    assert _lib.ST_OK in states and _lib.ST_EXCESS_ITER in states and len(set(iters)) > 20      # the neighbours stop at their own times
    ref = alone[0]
    for got in first + second:
        assert got[1] == ref[1], (got[1], ref[1])
        for u, v in zip(got[0] + got[2], ref[0] + ref[2]):
            assert np.array_equal(u, v)


# ---- 5. steps and limits -------------------------------------------------------------------------------------------------------

def test_steps_and_limits(T):
    from totsu_amd import _lib
    ds, _ = _family(T, "lp20")
    p = T.SolverParam()
    p.eps_acc = 1e-30
    sb = T.SmallBatchSolver.from_dense(ds, p)
    res = sb.run(7, poll_every=4)
    assert all(r.state == _lib.ST_RUNNING and r.iters == 7 for r in res)
    info = sb.info()
    assert info["launches"] == 2 and info["workgroups"] == 2 * len(ds)
    sb.destroy()
    ro = O.solve_matop_cones(O.param(max_iter=50, eps_acc=1e-30), ds[0].vec_c, ds[0].mat_a, ds[0].vec_b, ds[0].seg_type, ds[0].seg_len)
    assert ro.status == O.EXCESS_ITER and ro.iters == 49
    p.max_iter = 50
    sb = T.SmallBatchSolver.from_dense(ds, p)
    res = sb.run(-1, poll_every=16)
    assert all(r.state == _lib.ST_EXCESS_ITER and r.iters + 1 == 50 for r in res)      # the index of the 50th iteration, as the oracle's
    before = [sb.iterate(i) for i in range(len(ds))]
    launches = sb.info()["launches"]
    res = sb.run(10, poll_every=4)                     # a later run moves nothing (and launches nothing)
    assert all(r.state == _lib.ST_EXCESS_ITER and r.iters == 49 for r in res)
    assert sb.info()["launches"] == launches
    for i, (x, y) in enumerate(before):
        x2, y2 = sb.iterate(i)
        assert np.array_equal(x, x2) and np.array_equal(y, y2)
    sb.destroy()


# ---- 6. replace ----------------------------------------------------------------------------------------------------------------

def test_replace(T):
    from totsu_amd import _lib
    ds, _ = _family(T, "lp20")
    p = T.SolverParam()
    p.eps_acc = 1e-30

    def snaps(sb, i, pre=0):
        out = [sb.precond(i)]
        done = 0
        for it in (0, 1, 9):
            sb.run(it + 1 - done, poll_every=64)
            done = it + 1
            out.append(sb.iterate(i) + (sb.status(i).iters - pre,))
        return out

    fresh = T.SmallBatchSolver.from_dense([ds[4]], p)
    want_new = snaps(fresh, 0)
    fresh.destroy()
    untouched = T.SmallBatchSolver.from_dense(ds[:4], p)
    untouched.run(5 + 10, poll_every=64)
    want_others = [untouched.iterate(i) for i in range(4)]
    untouched.destroy()

    sb = T.SmallBatchSolver.from_dense(ds[:4], p)
    sb.run(5, poll_every=64)
    sb.replace(1, ds[4].mat_a, ds[4].vec_b, ds[4].vec_c)
    st = sb.status(1)
    assert st.state == _lib.ST_RUNNING and st.iters == 0 and sb.info()["live"] == 4
    got = snaps(sb, 1)                                 # the other slots advance by the same 10 iterations
    for g, w in zip(got, want_new):
        assert len(g) == len(w)
        for u, v in zip(g, w):
            assert np.array_equal(u, v)
    for i in (0, 2, 3):
        x, y = sb.iterate(i)
        assert np.array_equal(x, want_others[i][0]) and np.array_equal(y, want_others[i][1])
    sb.destroy()

    # a stopped slot can be replaced
    p2 = T.SolverParam()
    p2.eps_acc, p2.max_iter = 1e-30, 6
    sb = T.SmallBatchSolver.from_dense(ds[:4], p2)
    res = sb.run(-1, poll_every=4)
    assert all(r.state == _lib.ST_EXCESS_ITER for r in res) and sb.info()["live"] == 0
    sb.set_param(p)
    sb.replace(1, ds[4].mat_a, ds[4].vec_b, ds[4].vec_c)
    assert sb.info()["live"] == 1
    got = snaps(sb, 1)
    for g, w in zip(got, want_new):
        for u, v in zip(g, w):
            assert np.array_equal(u, v)
    assert [sb.status(i).state for i in range(4)] == [_lib.ST_EXCESS_ITER, _lib.ST_RUNNING, _lib.ST_EXCESS_ITER, _lib.ST_EXCESS_ITER]
    sb.destroy()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_leave_nothing_allocated(T):
    import ctypes as C
    from totsu_amd import _lib
    from totsu_amd._lib import lib
    S = T.SmallBatchSolver
    z = lambda *s: np.zeros(s, F)
    ds, _ = _family(T, "lp20")
    soc, _ = _family(T, "socp")
    bad = [lambda: S(3, 6, z(2, 18), z(2, 6), z(2, 3), [_lib.CONE_PSD], [6]),
           lambda: S(1, 24577, z(1, 24577), z(1, 24577), z(1, 1), [1], [24577]),
           lambda: S(24, 1025, z(1, 24 * 1025), z(1, 1025), z(1, 24), [1], [1025]),
           lambda: S(3, 6, z(2, 18), z(2, 6), z(2, 3), [1], [5]),
           lambda: S(3, 6, z(0, 18), z(0, 6), z(0, 3), [1], [6]),
           lambda: S(3, 6, z(2, 17), z(2, 6), z(2, 3), [1], [6]),
           lambda: S(3, 6, z(2, 18), z(2, 6), z(3, 3), [1], [6])]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    lp40, _ = _family(T, "lp40")
    with pytest.raises(ValueError):
        S.from_dense([ds[0], lp40[0]])
    d2 = _D(np.zeros((40, 20)), np.zeros(40), np.zeros(20), [1, 0], [39, 1])
    with pytest.raises(ValueError):
        S.from_dense([ds[0], d2])
    # the C ABI itself, over device arrays that exist: THIP_E_INVALID, *out stays NULL
    da, db, dc = (T.DeviceBuffer.from_host(z(64)) for _ in range(3))
    par = _lib.Param(-1, 1e-6, 1e-6, 1e-12, 0, 0, 0)

    def create(n, m, P, st, sl):
        st, sl = np.asarray(st, np.int32), np.asarray(sl, np.int64)
        h = C.c_void_p()
        with pytest.raises(_lib.ThipError) as e:
            lib.thip_smallbatch_create(n, m, P, da.ptr, db.ptr, dc.ptr, None, st.size, st.ctypes.data_as(C.POINTER(C.c_int32)),
                                       sl.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(par), C.byref(h))
        assert e.value.code == _lib.E_INVALID and not h.value

    create(3, 6, 2, [_lib.CONE_PSD], [6])
    create(1, 24577, 1, [1], [24577])
    create(24, 1025, 1, [1], [1025])
    create(3, 6, 2, [1], [5])
    create(3, 6, 0, [1], [6])
    create(3, 6, 1048577, [1], [6])
    for d in (da, db, dc):
        d.free()
    # no refusal left device memory behind: a later object is all the library holds
    sb = S.from_dense(ds)
    info = sb.info()
    assert info["device_bytes"] > info["arena_bytes"] > 0 and info["device_bytes_all"] == info["device_bytes"]
    sb2 = S.from_dense(soc)
    assert sb2.info()["device_bytes_all"] == info["device_bytes"] + sb2.info()["device_bytes"]
    sb2.destroy()
    assert sb.info()["device_bytes_all"] == info["device_bytes"]
    sb.destroy()
