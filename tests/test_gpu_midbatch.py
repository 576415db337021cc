"""GPU: many mid-size problems, each with its OWN A streamed from memory (totsu_amd.MidBatchSolver / thip_midbatch_*): every problem's
iterates against the f64 oracle, edge shapes around every tiling constant of the kernel, independent termination, isolation from the
neighbours and from the launch boundaries (bitwise), steps and limits, replace, the tau -> 0 branch, the refusals.  Every oracle
state a test relies on is asserted first.  The families, the oracle runs and the helpers are those of
tests/ownbatch_cases.py (computed once per session).

The kernel's tiling constants (thip_midbatch.hip):
    ROWS   = 256   rows per wave step (a lane holds 4 consecutive rows)
    CK     = 8     columns per chunk (loaded at once by a unit)
    WAVES  = 4, 16 waves of a workgroup (256 or 1024 threads); R = ceil(m / ROWS) row tiles against WAVES decides how a wave
                   walks the units (R < WAVES: column slices; R > WAVES: several row tiles per wave -- reachable with 4 waves only,
                   since 16 row tiles do not fit LDS)
    CB     = max(8, (2048 / R) & ~7)  columns per batch of the cross-wave sum of A^T y (2048 at R = 1, 1024 at R = 2)"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import tau_zero_problems as Z
from ownbatch_cases import (F, ITERS, TOLS, T, _D, _compare_snap, _dense_of, _edge, _lp_arrays, _oracle, _term_problem,  # noqa: F401
                            _View, check_against_oracle)
from ownbatch_cases import family as _family

pytestmark = pytest.mark.gpu

ROWS, CK, WAVES = 256, 8, (4, 16)


def _check(T, label, ds, ros, iters, tols, **kw):
    info = check_against_oracle(T, T.MidBatchSolver, label, ds, ros, iters, tols, **kw)
    n, m = ds[0].n, ds[0].m
    assert info["a_bytes_per_iter"] == 8 * m * n
    assert info["load_bytes"] == (16 if m % 4 == 0 else 4)
    return info


# ---- 1. iterates against the oracle, every problem with its own A -----------------------------------------------------------

@pytest.mark.parametrize("name", ["lp80", "lp260", "socp60", "qp", "lp20", "socp"])
def test_iterates_own_a(T, name):
    ds, ros = _family(T, name)
    info = _check(T, name, ds, ros, ITERS, TOLS)
    assert info["threads"] == (1024 if ds[0].m * ds[0].n > 8192 else 256)


@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("name", ["lp20", "lp80", "socp60"])
def test_iterates_every_workgroup_size(T, name, threads):
    ds, ros = _family(T, name)
    _check(T, "%s/%d threads" % (name, threads), ds, ros, ITERS, TOLS, force_threads=threads)


@pytest.mark.parametrize("name", ["lp80", "socp60"])
def test_iterates_plain_state(T, name):
    ds, ros = _family(T, name)
    _check(T, name + "/plain", ds, ros, ITERS, TOLS, state_arith="plain")


# ---- 2. edge shapes ----------------------------------------------------------------------------------------------------------

EDGE_SHAPES = [(1, 1, 0), (1, 300, 0), (300, 1, 0),
               (65, 33, 0), (66, 5, 0), (67, 9, 0),                       # m = 4k + 1, 4k + 2, 4k + 3; 65 * 33 is odd
               (ROWS - 1, 12, 0), (ROWS, 12, 0), (ROWS + 1, 12, 0),       # rows per wave step
               (40, CK - 1, 0), (40, CK, 0), (40, CK + 1, 0),             # columns per chunk
               (3 * ROWS, 10, 256), (4 * ROWS, 10, 256), (4 * ROWS + 1, 10, 256),      # row tiles: WAVES - 1, WAVES, WAVES + 1 (4 waves)
               (8, 2047, 0), (8, 2048, 0), (8, 2049, 0), (260, 1025, 0)]  # columns per batch at R = 1 (2048) and R = 2 (1024)


@pytest.mark.parametrize("m,n,threads", EDGE_SHAPES)
def test_edge_shapes(T, m, n, threads):
    """iterates 0 and 1 against the oracle at C - 1, C, C + 1 of every tiling constant, one row, one column, the 4-byte path"""
    ds = [_edge(m, n, s) for s in range(2)]
    ros = [_oracle(d, ITERS[:2]) for d in ds]
    kw = {"force_threads": threads} if threads else {}
    _check(T, "edge %dx%d" % (m, n), ds, ros, ITERS[:2], TOLS[:2], **kw)


def test_floor_edge_shape(T):
    """2000 x 1000: 34 000 floats of vectors, 8 MB of A per problem"""
    d = _edge(2000, 1000, 0)
    _check(T, "edge 2000x1000", [d], [_oracle(d, ITERS[:2])], ITERS[:2], TOLS[:2])


def test_unaligned_a_takes_the_4_byte_path_with_the_same_bits(T):
    """m % 4 == 0 with every A one float off a 16-byte boundary: info() reports the 4-byte path, the iterates are those of the
    aligned batch bit for bit (the same lanes hold the same entries on both paths)"""
    ds, _ = _family(T, "lp80")
    p = T.SolverParam()
    p.eps_acc = 1e-30
    a = np.stack([d.mat_a for d in ds])
    b, c = np.stack([d.vec_b for d in ds]), np.stack([d.vec_c for d in ds])
    seg = (ds[0].seg_type, ds[0].seg_len)

    def run(mats):
        sb = T.MidBatchSolver(80, 160, mats, b, c, seg[0], seg[1], p)
        info = sb.info()
        sb.run(10, poll_every=4)
        out = [sb.iterate(i) + sb.precond(i) for i in range(len(ds))]
        sb.destroy()
        return info, out

    i16, want = run(a)
    base = T.DeviceBuffer.from_host(np.concatenate([np.zeros(1, F), a.ravel()]))
    assert base.ptr % 16 == 0
    i4, got = run(_View(T, base, 1, a.size))
    base.free()
    assert (i16["load_bytes"], i4["load_bytes"]) == (16, 4)
    for g, w in zip(got, want):
        for u, v in zip(g, w):
            assert np.array_equal(u, v)


# ---- 3. independent termination ------------------------------------------------------------------------------------------------

def test_independent_termination(T):
    from totsu_amd import _lib
    P = 18
    ds = [_term_problem(i) for i in range(P)]
    ros = [O.solve_matop_cones(O.param(max_iter=100000, eps_acc=1e-5, eps_inf=1e-5), d.vec_c, d.mat_a, d.vec_b, d.seg_type, d.seg_len,
                               trace_cap=400) for d in ds]
    want = [O.INFEASIBLE, O.OK, O.UNBOUNDED]
    for i, ro in enumerate(ros):
        assert ro.status == want[i % 3] and ro.iters < 399, (i, ro.status_name, ro.iters)
    p = T.SolverParam()
    p.max_iter, p.eps_acc, p.eps_inf = 100000, 1e-5, 1e-5
    sb = T.MidBatchSolver.from_dense(ds, p)
    early, wg, live = {}, [0], [P]
    while True:
        res = sb.run_until_any(8, poll_every=8)        # 8 iterations at a time, back as soon as something has stopped
        info = sb.info()
        wg.append(info["workgroups"])
        live.append(info["live"])
        assert wg[-1] - wg[-2] == live[-2]             # one workgroup per problem that was running, ONE launch: back at the first poll
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
    sols = sb.solve()
    for i, s_ in enumerate(sols):
        if i % 3 == 1:
            assert isinstance(s_, tuple) and np.allclose(s_[0], ros[i].x, atol=1e-3)
        else:
            assert isinstance(s_, T.SolverError)
    sb.destroy()


def test_easy_and_hard_lps_stop_on_their_own(T):
    """feasible LPs of 160 x 80 that need 2069 .. 4897 iterations at eps_acc = 1e-3 in the oracle (each at least 12 % more than the
    one before), in one batch: they stop in the oracle's order, each is found at the first poll after its stop, and what a stopped
    problem holds no longer changes while the others run on"""
    from totsu_amd import _lib
    ds, _ = _family(T, "lp80")
    ros = [O.solve_matop_cones(O.param(max_iter=40000, eps_acc=1e-3), d.vec_c, d.mat_a, d.vec_b, d.seg_type, d.seg_len) for d in ds]
    want = sorted(ro.iters for ro in ros)
    assert all(ro.status == O.OK for ro in ros) and all(b >= 1.12 * a for a, b in zip(want, want[1:])), want
    p = T.SolverParam()
    p.max_iter, p.eps_acc = 40000, 1e-3
    POLL = 100
    sb = T.MidBatchSolver.from_dense(ds, p)
    early, calls = {}, 0
    while len(early) < len(ds):
        res = sb.run_until_any(-1, poll_every=POLL)
        calls += 1
        launches = sb.info()["launches"]
        new = [i for i, r in enumerate(res) if r.state != _lib.ST_RUNNING and i not in early]
        assert new, "run_until_any came back without a new stop"
        for i in new:
            assert (launches - 1) * POLL < res[i].iters + 1 <= launches * POLL, (i, res[i].iters, launches)      # the first poll after
            early[i] = (res[i].state, res[i].iters) + sb.iterate(i)
        assert calls <= len(ds)
    print("easy and hard: iterations", [r.iters for r in res], "oracle", [ro.iters for ro in ros], "calls", calls)
    assert all(r.state == _lib.ST_OK for r in res) and sb.info()["live"] == 0
    assert np.array_equal(np.argsort([r.iters for r in res]), np.argsort([ro.iters for ro in ros]))
    for i, r in enumerate(res):
        x, y = sb.iterate(i)
        assert early[i][:2] == (r.state, r.iters) and np.array_equal(early[i][2], x) and np.array_equal(early[i][3], y)
        xs, _ = sb.solution(i)
        assert np.allclose(xs, ros[i].x, atol=2e-2 * max(1.0, np.abs(ros[i].x).max()))
    sb.destroy()


# ---- 4. isolation and reproducibility ------------------------------------------------------------------------------------------

def test_isolation_and_reproducibility(T):
    from totsu_amd import _lib
    P = 300                                            # more workgroups than the device has CUs
    seeds = list(range(P))
    seeds[P - 1] = 0                                   # the same LP at index 0 and at index 299
    a, b, c = _lp_arrays(seeds)
    p = T.SolverParam()
    p.max_iter, p.eps_acc = 1500, 1e-3
    seg = ([_lib.CONE_RPOS], [40])

    def run(aa, bb, cc, idx):
        sb = T.MidBatchSolver(20, 40, aa, bb, cc, seg[0], seg[1], p)
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


@pytest.mark.parametrize("name", ["lp260", "socp60"])
def test_launch_cuts_change_nothing(T, name):
    """100 iterations as 100 launches of 1, as 7 + 93 and as one launch: the same bits (the carried pair lives in the arena)"""
    ds, _ = _family(T, name)
    p = T.SolverParam()
    p.eps_acc = 1e-30

    def run(cuts):
        sb = T.MidBatchSolver.from_dense(ds, p)
        for steps, poll in cuts:
            sb.run(steps, poll_every=poll)
        assert all(sb.status(i).iters == 100 for i in range(len(ds)))
        out = [sb.iterate(i) + (tuple(sb.status(i).cri),) for i in range(len(ds))]
        launches = sb.info()["launches"]
        sb.destroy()
        return out, launches

    one, l1 = run([(100, 100)])
    single, l100 = run([(100, 1)])
    split, l2 = run([(7, 7), (93, 93)])
    assert (l1, l100, l2) == (1, 100, 2)
    for other in (single, split):
        for g, w in zip(other, one):
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and g[2] == w[2]


# ---- 5. steps and limits -------------------------------------------------------------------------------------------------------

def test_steps_and_limits(T):
    from totsu_amd import _lib
    ds, _ = _family(T, "lp80")
    p = T.SolverParam()
    p.eps_acc = 1e-30
    sb = T.MidBatchSolver.from_dense(ds, p)
    res = sb.run(7, poll_every=4)
    assert all(r.state == _lib.ST_RUNNING and r.iters == 7 for r in res)
    info = sb.info()
    assert info["launches"] == 2 and info["workgroups"] == 2 * len(ds)
    sb.destroy()
    ro = O.solve_matop_cones(O.param(max_iter=50, eps_acc=1e-30), ds[0].vec_c, ds[0].mat_a, ds[0].vec_b, ds[0].seg_type, ds[0].seg_len)
    assert ro.status == O.EXCESS_ITER and ro.iters == 49
    p.max_iter = 50
    sb = T.MidBatchSolver.from_dense(ds, p)
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
    ds, _ = _family(T, "lp80")
    p = T.SolverParam()
    p.eps_acc = 1e-30

    def snaps(sb, i):
        st = sb.status(i)
        out = [sb.precond(i) + ((st.state, st.iters, st.tau, st.kappa, st.norm_b, st.norm_c),)]
        done = 0
        for it in (0, 1, 9):
            sb.run(it + 1 - done, poll_every=64)
            done = it + 1
            st = sb.status(i)
            out.append(sb.iterate(i) + ((st.state, st.iters, st.kind, tuple(st.cri)),))
        return out

    def same(got, want):
        for g, w in zip(got, want):
            assert len(g) == len(w) == 3
            assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and g[2] == w[2], (g[2], w[2])

    fresh = T.MidBatchSolver.from_dense([ds[4]], p)
    want_new = snaps(fresh, 0)
    fresh.destroy()
    untouched = T.MidBatchSolver.from_dense(ds[:4], p)
    untouched.run(5 + 10, poll_every=64)
    want_others = [untouched.iterate(i) for i in range(4)]
    untouched.destroy()

    sb = T.MidBatchSolver.from_dense(ds[:4], p)
    sb.run(5, poll_every=64)
    sb.replace(1, ds[4].mat_a, ds[4].vec_b, ds[4].vec_c)
    st = sb.status(1)
    assert st.state == _lib.ST_RUNNING and st.iters == 0 and sb.info()["live"] == 4
    same(snaps(sb, 1), want_new)                       # the other slots advance by the same 10 iterations
    for i in (0, 2, 3):
        x, y = sb.iterate(i)
        assert np.array_equal(x, want_others[i][0]) and np.array_equal(y, want_others[i][1])
    sb.destroy()

    # a stopped slot can be replaced
    p2 = T.SolverParam()
    p2.eps_acc, p2.max_iter = 1e-30, 6
    sb = T.MidBatchSolver.from_dense(ds[:4], p2)
    res = sb.run(-1, poll_every=4)
    assert all(r.state == _lib.ST_EXCESS_ITER for r in res) and sb.info()["live"] == 0
    sb.set_param(p)
    sb.replace(1, ds[4].mat_a, ds[4].vec_b, ds[4].vec_c)
    assert sb.info()["live"] == 1
    same(snaps(sb, 1), want_new)
    assert [sb.status(i).state for i in range(4)] == [_lib.ST_EXCESS_ITER, _lib.ST_RUNNING, _lib.ST_EXCESS_ITER, _lib.ST_EXCESS_ITER]
    sb.destroy()


# ---- 7. the tau -> 0 branch ----------------------------------------------------------------------------------------------------

def _tau_zero_batch(name):
    fams, pls = Z.family(name), Z.plan(name)
    return (fams, pls) if name == "F6" else ([fams], [pls])


@pytest.mark.parametrize("name", ["F1", "F2", "F3", "F4", "F6"])
def test_iterates_and_criteria_through_tau_zero(T, name):
    fams, pls = _tau_zero_batch(name)
    for fam, pl in zip(fams, pls):
        before, ones, after = Z.counts(pl)
        if fam.verdict != Z.OK:
            assert before >= 1 and ones >= 3 and (after >= 1 or not fam.flips_back), (fam.name, before, ones, after)
    p = T.SolverParam()
    p.eps_acc = p.eps_inf = 1e-30
    sb = T.MidBatchSolver.from_dense([_dense_of(f) for f in fams], p)
    done = 0
    for it in sorted(set(i for pl in pls for i in pl.chosen)):
        sb.run(it + 1 - done, poll_every=64)
        done = it + 1
        for q, (fam, pl) in enumerate(zip(fams, pls)):
            if it in pl.chosen:
                x, y = sb.iterate(q)
                _compare_snap("midbatch/%s" % fam.name, fam, pl, it, x, y, sb.status(q))
    assert all(sb.status(q).state == -1 for q in range(len(fams)))
    if name == "F6":                                   # the slots are in different regimes at the end of the window
        assert [sb.status(q).kind for q in range(3)] == [0, 1, 1] == [pl.kinds[-1] for pl in pls]
    sb.destroy()


@pytest.mark.parametrize("name", ["F1", "F2", "F3", "F4", "F6"])
def test_verdicts(T, name):
    fams, pls = _tau_zero_batch(name)
    for fam, pl in zip(fams, pls):
        assert pl.status == fam.verdict and pl.iters <= Z.MAX_VERDICT_ITER
    if name == "F6":
        assert [pl.status for pl in pls] == [Z.OK, Z.INFEASIBLE, Z.UNBOUNDED]
    p = T.SolverParam()
    p.max_iter, p.eps_acc, p.eps_inf = 100_000, Z.EPS, Z.EPS
    sb = T.MidBatchSolver.from_dense([_dense_of(f) for f in fams], p)
    res = sb.run(-1, poll_every=25)
    n, m = fams[0].n, fams[0].m
    for q, (fam, pl, r) in enumerate(zip(fams, pls, res)):
        margin = max(3, pl.iters // 50)
        print("tau_zero verdict midbatch/%-14s state %d at %d (oracle %d at %d, margin %d) kind %d cri %s"
              % (fam.name, r.state, r.iters, pl.status, pl.iters, margin, r.kind, tuple("%.3e" % c for c in r.cri)))
        assert r.state == pl.status, (fam.name, r.state, pl.status)
        assert abs(r.iters - pl.iters) <= margin, (fam.name, r.iters, pl.iters)
        (x, y), sol = sb.iterate(q), sb.solution(q)
        if pl.status == Z.OK:
            assert r.kind == 0 and r.tau > 0 and np.allclose(sol[0], pl.x, atol=2e-3 * max(1.0, np.abs(pl.x).max()))
        else:                                          # a kind-1 ending is not scaled: the answer is the iterate's x_x, x_y bit for bit
            assert r.kind == 1 and r.tau == 0.0 and x[n + 2 * m] == 0.0, (fam.name, r.kind, r.tau)
            assert r.cri[0 if pl.status == Z.UNBOUNDED else 1] <= Z.EPS, (fam.name, r.cri)
            assert np.array_equal(sol[0], x[:n]) and np.array_equal(sol[1], x[n:n + m]), fam.name
    sb.destroy()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------

def test_refusals_leave_nothing_allocated(T):
    from totsu_amd import _lib
    from totsu_amd._lib import lib
    S = T.MidBatchSolver
    z = lambda *s: np.zeros(s, F)
    ds, _ = _family(T, "lp80")
    keep = S.from_dense(ds)                            # something alive, so that device_bytes_all can be read before and after
    before = keep.info()["device_bytes_all"]
    assert before == keep.info()["device_bytes"] > keep.info()["arena_bytes"] > 0
    bad = [lambda: S(3, 6, z(2, 18), z(2, 6), z(2, 3), [_lib.CONE_PSD], [6]),
           lambda: S(2, 4097, z(1, 2 * 4097), z(1, 4097), z(1, 2), [1], [4097]),
           lambda: S(4097, 2, z(1, 2 * 4097), z(1, 2), z(1, 4097), [1], [2]),
           lambda: S(1000, 2020, z(1, 1), z(1, 2020), z(1, 1000), [1], [2020]),
           lambda: S(3, 6, z(2, 18), z(2, 6), z(2, 3), [1], [5]),
           lambda: S(3, 6, z(0, 18), z(0, 6), z(0, 3), [1], [6]),
           lambda: S(3, 6, z(2, 17), z(2, 6), z(2, 3), [1], [6]),
           lambda: S(3, 6, z(2, 18), z(2, 6), z(3, 3), [1], [6])]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    lp20, _ = _family(T, "lp20")
    with pytest.raises(ValueError):
        S.from_dense([ds[0], lp20[0]])
    with pytest.raises(ValueError):
        S.from_dense([ds[0], _D(np.zeros((160, 80)), np.zeros(160), np.zeros(80), [1, 0], [159, 1])])
    # the C ABI itself, over device arrays that exist: THIP_E_INVALID, thip_last_error set, *out stays NULL
    da, db, dc = (T.DeviceBuffer.from_host(z(64)) for _ in range(3))
    par = _lib.Param(-1, 1e-6, 1e-6, 1e-12, 0, 0, 0)

    def create(n, m, P, st, sl, null_seg=False):
        st, sl = np.asarray(st, np.int32), np.asarray(sl, np.int64)
        h = C.c_void_p()
        with pytest.raises(_lib.ThipError) as e:
            lib.thip_midbatch_create(n, m, P, da.ptr, db.ptr, dc.ptr, None, st.size,
                                     None if null_seg else st.ctypes.data_as(C.POINTER(C.c_int32)),
                                     sl.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(par), C.byref(h))
        assert e.value.code == _lib.E_INVALID and not h.value and _lib.load().thip_last_error()
        assert keep.info()["device_bytes_all"] == before

    create(3, 6, 2, [_lib.CONE_PSD], [6])
    create(3, 8, 2, [1, _lib.CONE_PSD], [2, 6])
    create(2, 4097, 1, [1], [4097])
    create(4097, 2, 1, [1], [2])
    create(1000, 2020, 1, [1], [2020])                 # a map beyond LDS
    create(3, 6, 2, [1], [5])
    create(3, 6, 2, [1], [7])
    create(3, 6, 2, [9], [6])                          # an unknown segment
    create(3, 6, 2, [1], [6], null_seg=True)           # a null one
    create(3, 6, 0, [1], [6])
    create(3, 6, 1048577, [1], [6])
    for d in (da, db, dc):
        d.free()
    # no refusal left device memory behind: a later object is all the library holds beside the first
    soc, _ = _family(T, "socp")
    sb2 = S.from_dense(soc)
    assert sb2.info()["device_bytes_all"] == before + sb2.info()["device_bytes"]
    sb2.destroy()
    assert keep.info()["device_bytes_all"] == before
    keep.destroy()


def test_own_a_batch_returns_the_batch_the_shape_needs(T):
    lp20, _ = _family(T, "lp20")
    lp260, _ = _family(T, "lp260")
    small, mid = T.own_a_batch(lp20), T.own_a_batch(lp260[:2])
    assert type(small) is T.SmallBatchSolver and type(mid) is T.MidBatchSolver
    assert all(r.iters == 3 for r in small.run(3)) and all(r.iters == 3 for r in mid.run(3))
    small.destroy()
    mid.destroy()
