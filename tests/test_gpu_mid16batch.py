"""GPU: the mid batch over a library-owned 16-bit copy of every problem's A (totsu_amd.Mid16BatchSolver / thip_mid16batch_*).

The contract under test: with W the widened matrix of the stored form (tests/mid16_cases.py), a Mid16BatchSolver is BIT FOR BIT a
MidBatchSolver over W in f32 -- the twin.  So: the stored form against its numpy restatement, word for word; the twin at every
workgroup size, in both state arithmetics, on the edge shapes of the f32 family and after every call of the family; the f64 oracle
run on W at the project's tolerances; that the rounding is applied and the memory halved; that a 16-bit batch's end iterate starts
an f32 batch on the exact matrix; the refusals.  Both stored forms unless said."""
import ctypes as C

import numpy as np
import pytest

import mid16_cases as M
import oracle as O
import tau_zero_problems as Z
from ownbatch_cases import F, ITERS, TOLS, T, _dense_of, _edge, _lp_arrays, _oracle, _term_problem, check_against_oracle  # noqa: F401
from ownbatch_cases import family as _family

pytestmark = pytest.mark.gpu

KINDS = M.KINDS


def _param(T, **kw):
    p = T.SolverParam()
    p.eps_acc = 1e-30
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _pair(T, ds, kind, p=None, **kw):
    sb = T.Mid16BatchSolver.from_dense(ds, p, a_dtype=kind, **kw)
    return sb, M.twin_of(T, sb, ds, p, **kw)


def _both(fn, *solvers):
    for s in solvers:
        fn(s)


# ---- 1. the stored form ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n", M.STORED_SHAPES)
def test_stored_form_is_the_numpy_restatement(T, m, n, kind):
    from totsu_amd import mid16batch as MM
    mats = [M.planted(m, n, seed) for seed in range(2)]
    rng = np.random.default_rng(m + n)
    b, c = rng.standard_normal((2, m)).astype(F), rng.standard_normal((2, n)).astype(F)
    sb = T.Mid16BatchSolver(n, m, np.stack(mats), b, c, [1], [m], _param(T), a_dtype=kind)
    try:
        for i, a in enumerate(mats):
            words, inv = sb.stored_a(i)
            want_w, want_inv = M.stored(a, m, n, kind)
            assert words.shape == (n, M.ld16(m)) and words.dtype == np.uint16
            assert np.array_equal(words, want_w), (i, np.argwhere(words != want_w)[:4])
            assert not words[:, m:].any()                          # the pad rows
            if kind == "f16":
                assert np.array_equal(inv, want_inv), (i, inv, want_inv)
                if n >= 5:                                         # the planted columns did what they were planted for
                    assert inv[1] == 1.0 and inv[2] == F(2.0 ** 114) and inv[3] == F(2.0 ** -113) and inv[4] == F(2.0 ** -13)
                    sub = words[4, 1:m].view(np.float16)
                    assert m < 8 or (np.count_nonzero((sub != 0) & (np.abs(sub) < 2.0 ** -14)) >= 4)
            else:
                assert inv is None
            assert np.array_equal(sb.widened(i), M.widen(want_w, want_inv, m))
            got = words.nbytes + (0 if inv is None else inv.nbytes)
            assert MM.store_bytes(n, m, kind) == (got + 15) // 16 * 16 == M.store_bytes(n, m, kind)
        assert sb.info()["a_store_bytes"] == 2 * M.store_bytes(n, m, kind)
    finally:
        sb.destroy()


# ---- 2. the twin ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("arith", ["compensated", "plain"])
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("name", ["lp80", "lp260", "socp60", "qp"])
def test_twin(T, name, threads, arith, kind):
    ds, _ = _family(T, name)
    p = _param(T, state_arith=arith)
    sb, tw = _pair(T, ds, kind, p, force_threads=threads)
    try:
        assert sb.info()["threads"] == tw.info()["threads"] == threads
        M.assert_same(sb, tw, len(ds), "init")
        done = 0
        for it in (1, 2, 10, 50):
            _both(lambda s: s.run(it - done, poll_every=64), sb, tw)
            done = it
            assert sb.status(0).iters == it
            M.assert_same(sb, tw, len(ds), "%s/%d/%s/%s after %d" % (name, threads, arith, kind, it))
    finally:
        sb.destroy()
        tw.destroy()


# ---- 3. edge shapes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n,threads", M.EDGE_SHAPES)
def test_edge_shapes_against_the_twin(T, m, n, threads, kind):
    ds = [_edge(m, n, s) for s in range(2)]
    kw = {"force_threads": threads} if threads else {}
    sb, tw = _pair(T, ds, kind, _param(T), **kw)
    try:
        assert sb.info()["load_bytes"] == 8
        for it in (1, 2):
            _both(lambda s: s.run(1, poll_every=1), sb, tw)
            M.assert_same(sb, tw, 2, "edge %dx%d after %d" % (m, n, it))
    finally:
        sb.destroy()
        tw.destroy()


@pytest.mark.parametrize("kind", KINDS)
def test_floor_edge_shape_against_the_twin(T, kind):
    """2000 x 1000, one problem: the shape rule is the mid batch's, and the largest shape of its tests still fits"""
    d = _edge(2000, 1000, 0)
    sb, tw = _pair(T, [d], kind, _param(T))
    try:
        for it in (1, 2):
            _both(lambda s: s.run(1, poll_every=1), sb, tw)
            M.assert_same(sb, tw, 1, "2000x1000 after %d" % it)
        assert sb.info()["a_store_bytes"] == M.store_bytes(1000, 2000, kind)
    finally:
        sb.destroy()
        tw.destroy()


# ---- 4. the oracle on W --------------------------------------------------------------------------------------------------------------

def _oracle_on_w(T, name, kind):
    """the f64 oracle's runs on the widened matrices (the numpy restatement's, which test 1 holds the device to)"""
    ds, _ = _family(T, name)
    out_d, out_r = [], []
    for i, d in enumerate(ds):
        w = M.widened_of(d.mat_a, d.m, d.n, kind)
        wd = M.WDense(d, w)
        if name == "socp60":                           # the SOCP oracle on the pieces of W: rows of cone i are [-c_i^T ; -G_i]
            from problems import random_socp
            f, Gs, hs, cs, dd = random_socp(60, [5, 1, 0, 17, 140, 250, 3], seed=i)
            wm = w.reshape(d.n, d.m).T.astype(np.float64)
            o, Gw, cw = 0, [], []
            for G in Gs:
                cw.append(-wm[o])
                Gw.append(-wm[o + 1:o + 1 + G.shape[0]])
                o += 1 + G.shape[0]
            assert o == d.m
            out_r.append(_oracle(wd, ITERS, socp=(f, Gw, hs, cw, dd)))
        else:
            out_r.append(_oracle(wd, ITERS))
        out_d.append(wd)
    for ro in out_r:
        assert ro.status == O.EXCESS_ITER and len(ro.trace) > max(ITERS)
    return ds, out_r


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["lp80", "socp60"])
def test_iterates_against_the_oracle_on_w(T, name, kind):
    ds, ros = _oracle_on_w(T, name, kind)
    info = check_against_oracle(T, T.Mid16BatchSolver, "%s/%s" % (name, kind), ds, ros, ITERS, TOLS, a_dtype=kind)
    assert info["a_dtype"] == kind


# ---- 5. rounding and memory ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_the_rounding_is_applied_and_the_memory_halved(T, kind):
    ds, _ = _family(T, "lp80")
    n, m, P = ds[0].n, ds[0].m, len(ds)
    p = _param(T)
    sb = T.Mid16BatchSolver.from_dense(ds, p, a_dtype=kind)
    f32 = T.MidBatchSolver.from_dense(ds, p)
    try:
        i16, i32 = sb.info(), f32.info()
        per = 2 * M.ld16(m) * n + (4 * n if kind == "f16" else 0)
        assert (i16["a_dtype"], i16["load_bytes"], i16["a_bytes_per_iter"]) == (kind, 8, 2 * per)
        assert i16["a_store_bytes"] == P * M.store_bytes(n, m, kind)
        # what the handle holds beyond an f32 handle of the same problems is the store, to the byte; the f32 stack is not kept
        assert i16["device_bytes"] - i32["device_bytes"] == i16["a_store_bytes"]
        assert i16["a_store_bytes"] <= (P * 4 * m * n) // 2 + P * (4 * n + 16)
        assert sb.mats_a is None
        _both(lambda s: s.run(10, poll_every=10), sb, f32)
        for i in range(P):
            assert not np.array_equal(sb.iterate(i)[0], f32.iterate(i)[0])
    finally:
        sb.destroy()
        f32.destroy()


# ---- 6. the family's methods, each against the twin after the same calls ------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_launch_cuts_change_nothing(T, kind):
    ds, _ = _family(T, "socp60")
    p = _param(T)
    sb, tw = _pair(T, ds, kind, p)
    tw.run(64, poll_every=64)
    want = [M.state_of(tw, i) for i in range(len(ds))]
    tw.destroy()
    sb.destroy()
    for poll in (1, 7, 64):
        sb = T.Mid16BatchSolver.from_dense(ds, p, a_dtype=kind)
        sb.run(64, poll_every=poll)
        assert sb.info()["launches"] == -(-64 // poll)
        for i in range(len(ds)):
            g = M.state_of(sb, i)
            assert all(np.array_equal(g[k], want[i][k]) for k in range(4)) and g[4] == want[i][4], (poll, i)
        sb.destroy()


@pytest.mark.parametrize("kind", KINDS)
def test_index_and_neighbours_change_nothing(T, kind):
    from totsu_amd import _lib
    P = 300
    a, b, c = _lp_arrays([i % 7 for i in range(P)])
    p = _param(T, max_iter=1500, eps_acc=1e-3)
    sb = T.Mid16BatchSolver(20, 40, a, b, c, [_lib.CONE_RPOS], [40], p, a_dtype=kind)
    w = np.stack([sb.widened(i) for i in range(7)])
    tw = T.MidBatchSolver(20, 40, w[[i % 7 for i in range(P)]], b, c, [_lib.CONE_RPOS], [40], p)
    try:
        _both(lambda s: s.run(100, poll_every=50), sb, tw)
        for i in (0, 1, 7, 150, 299):
            g, t = M.state_of(sb, i), M.state_of(sb, i % 7)
            assert all(np.array_equal(g[k], t[k]) for k in range(4)) and g[4] == t[4], i
        M.assert_same(sb, tw, 7, "P = 300 after 100")
        r16, r32 = sb.run(-1, poll_every=100), tw.run(-1, poll_every=100)
        assert [(r.state, r.iters) for r in r16] == [(r.state, r.iters) for r in r32]
        for (x, y), (xt, yt) in zip(sb.solutions(), tw.solutions()):
            assert np.array_equal(x, xt) and np.array_equal(y, yt)
    finally:
        sb.destroy()
        tw.destroy()


@pytest.mark.parametrize("kind", KINDS)
def test_independent_termination(T, kind):
    from totsu_amd import _lib
    ds = [_term_problem(i) for i in range(18)]
    p = _param(T, max_iter=100000, eps_acc=1e-5, eps_inf=1e-5)
    sb, tw = _pair(T, ds, kind, p)
    try:
        r16, r32 = sb.run(-1, poll_every=8), tw.run(-1, poll_every=8)
        assert all(r.state != _lib.ST_RUNNING for r in r16) and len(set(r.state for r in r16)) == 3
        assert len(set(r.iters for r in r16)) >= 3
        assert [(r.state, r.iters, r.kind) for r in r16] == [(r.state, r.iters, r.kind) for r in r32]
        M.assert_same(sb, tw, len(ds), "termination")
    finally:
        sb.destroy()
        tw.destroy()


@pytest.mark.parametrize("kind", KINDS)
def test_replace(T, kind):
    ds, _ = _family(T, "lp80")
    p = _param(T)
    sb, tw = _pair(T, ds[:4], kind, p)
    fresh = T.Mid16BatchSolver.from_dense([ds[4]], p, a_dtype=kind)
    try:
        _both(lambda s: s.run(5, poll_every=5), sb, tw)
        held = sb.info()["device_bytes"]
        sb.replace(1, ds[4].mat_a, ds[4].vec_b, ds[4].vec_c)
        assert sb.info()["device_bytes"] == held                     # converted into the slot's block: nothing allocated
        assert np.array_equal(sb.widened(1), M.widened_of(ds[4].mat_a, ds[4].m, ds[4].n, kind))
        tw.replace(1, sb.widened(1), ds[4].vec_b, ds[4].vec_c)
        M.assert_same(sb, tw, 4, "replace")
        _both(lambda s: s.run(10, poll_every=4), sb, tw, fresh)
        M.assert_same(sb, tw, 4, "replace + 10")
        g, w = M.state_of(sb, 1), M.state_of(fresh, 0)              # and a fresh batch of the new problem alone
        assert all(np.array_equal(g[k], w[k]) for k in range(4)) and g[4] == w[4]
    finally:
        sb.destroy()
        tw.destroy()
        fresh.destroy()


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_set_bc(T, kind, keep):
    ds, _ = _family(T, "socp60")
    sb, tw = _pair(T, ds, kind, _param(T))
    try:
        _both(lambda s: s.run(6, poll_every=6), sb, tw)
        nb = [ds[(i + 1) % len(ds)].vec_b for i in range(len(ds))]
        nc = [ds[(i + 1) % len(ds)].vec_c * F(1.25) for i in range(len(ds))]
        nr = [ds[(i + 1) % len(ds)].vec_b_rowabs for i in range(len(ds))]
        _both(lambda s: s.set_bc(nb, nc, nr, keep_iterate=keep), sb, tw)
        M.assert_same(sb, tw, len(ds), "set_bc")
        db, dc, dr = (T.DeviceBuffer.from_host(np.concatenate(v)) for v in (nb, nc, nr))
        _both(lambda s: s.run(9, poll_every=4), sb, tw)
        M.assert_same(sb, tw, len(ds), "set_bc + 9")
        _both(lambda s: s.set_bc_dev(db, dc, dr, keep_iterate=keep), sb, tw)
        _both(lambda s: s.run(3, poll_every=3), sb, tw)
        M.assert_same(sb, tw, len(ds), "set_bc_dev + 3")
        for d in (db, dc, dr):
            d.free()
    finally:
        sb.destroy()
        tw.destroy()


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("route", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_set_a(T, kind, route, keep):
    """new values of A for slots 1 and 2: against the twin handed the widened new A, and (fresh) against replace"""
    ds, _ = _family(T, "lp80")
    p = _param(T)
    sb, tw = _pair(T, ds[:4], kind, p)
    rp = T.Mid16BatchSolver.from_dense(ds[:4], p, a_dtype=kind)
    try:
        _both(lambda s: s.run(5, poll_every=5), sb, tw, rp)
        new = [ds[4].mat_a, ds[0].mat_a * F(1.5)]
        held = sb.info()["device_bytes"]
        if route == "host":
            sb.set_a(new, first=1, keep_iterate=keep)
        else:
            dv = T.DeviceBuffer.from_host(np.concatenate(new))
            sb.set_a_dev(dv, first=1, count=2, keep_iterate=keep)
            assert sb.info()["device_bytes"] == held                 # (the host route allocates its stage; this one nothing)
            dv.free()
        wn = [M.widened_of(a, ds[0].m, ds[0].n, kind) for a in new]
        assert np.array_equal(sb.widened(1), wn[0]) and np.array_equal(sb.widened(2), wn[1])
        assert np.array_equal(sb.widened(0), M.widened_of(ds[0].mat_a, ds[0].m, ds[0].n, kind))      # the neighbours' blocks stay
        tw.set_a(wn, first=1, keep_iterate=keep)
        M.assert_same(sb, tw, 4, "set_a")
        if not keep:
            for k in (0, 1):
                rp.replace(1 + k, new[k], ds[1 + k].vec_b, ds[1 + k].vec_c)
        _both(lambda s: s.run(8, poll_every=3), sb, tw, rp)
        M.assert_same(sb, tw, 4, "set_a + 8")
        if not keep:
            for i in (1, 2):
                g, w = M.state_of(sb, i), M.state_of(rp, i)
                assert all(np.array_equal(g[k], w[k]) for k in range(4)) and g[4] == w[4], i
    finally:
        sb.destroy()
        tw.destroy()
        rp.destroy()


@pytest.mark.parametrize("kind", KINDS)
def test_set_iterates_and_solutions(T, kind):
    ds, _ = _family(T, "socp60")
    p = _param(T, eps_acc=1e-3, max_iter=400)
    sb, tw = _pair(T, ds, kind, p)
    try:
        _both(lambda s: s.run(20, poll_every=20), sb, tw)
        xs, ys = zip(*[sb.raw_iterate((i + 1) % len(ds)) for i in range(len(ds))])
        _both(lambda s: s.set_iterates(xs, ys), sb, tw)
        M.assert_same(sb, tw, len(ds), "set_iterates")
        _both(lambda s: s.run(7, poll_every=7), sb, tw)
        M.assert_same(sb, tw, len(ds), "set_iterates + 7")
        dx, dy = T.DeviceBuffer.from_host(np.concatenate(xs)), T.DeviceBuffer.from_host(np.concatenate(ys))
        _both(lambda s: s.set_iterates_dev(dx, dy), sb, tw)
        _both(lambda s: s.run(-1, poll_every=50), sb, tw)
        M.assert_same(sb, tw, len(ds), "set_iterates_dev + run")
        dx.free()
        dy.free()
        s16, s32 = sb.solutions(), tw.solutions()
        for i, ((x, y), (xt, yt)) in enumerate(zip(s16, s32)):
            assert np.array_equal(x, xt) and np.array_equal(y, yt)
            x1, y1 = sb.solution(i)
            assert np.array_equal(x, x1) and np.array_equal(y, y1)
        assert [(r.state, r.iters) for r in sb.statuses()] == [(r.state, r.iters) for r in tw.statuses()]
        gx, gy, gs = sb.solutions_dev()
        assert np.array_equal(gx.to_host(), np.concatenate([x for x, _ in s16]))
        assert np.array_equal(gy.to_host(), np.concatenate([y for _, y in s16]))
        assert list(gs.to_host().view(np.int32)) == [r.state for r in sb.statuses()]
        for d in (gx, gy, gs):
            d.free()
    finally:
        sb.destroy()
        tw.destroy()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["F1", "F2", "F3", "F4", "F6"])
def test_tau_zero_families_end_as_the_twin(T, name, kind):
    fams = Z.family(name)
    fams = fams if name == "F6" else [fams]
    ds = [_dense_of(f) for f in fams]
    p = _param(T, max_iter=100_000, eps_acc=Z.EPS, eps_inf=Z.EPS)
    sb, tw = _pair(T, ds, kind, p)
    try:
        r16, r32 = sb.run(-1, poll_every=25), tw.run(-1, poll_every=25)
        print("tau_zero mid16/%s/%s: %s" % (name, kind, [(r.state, r.iters, r.kind) for r in r16]))
        assert all(r.state != -1 for r in r16)
        assert [(r.state, r.iters, r.kind, r.tau) for r in r16] == [(r.state, r.iters, r.kind, r.tau) for r in r32]
        M.assert_same(sb, tw, len(ds), "tau zero")
    finally:
        sb.destroy()
        tw.destroy()


# ---- 7. the mixed route --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_a_16_bit_batch_warm_starts_the_exact_one(T, kind):
    from totsu_amd import _lib
    ds, _ = _family(T, "lp80")
    p = _param(T, max_iter=40000, eps_acc=1e-3)
    cold = T.MidBatchSolver.from_dense(ds, p)
    r_cold = cold.run(-1, poll_every=100)
    assert all(r.state == _lib.ST_OK for r in r_cold)                 # these inputs end OK in f32, cold
    sb = T.Mid16BatchSolver.from_dense(ds, p, a_dtype=kind)
    try:
        r16 = sb.run(-1, poll_every=100)
        xs, ys = zip(*[sb.raw_iterate(i) for i in range(len(ds))])
        cold.reinit()
        cold.set_iterates(xs, ys)
        r_warm = cold.run(-1, poll_every=100)
        print("mixed route %s: cold f32 %s; 16-bit %s then f32 %s" % (kind, [r.iters + 1 for r in r_cold], [r.iters + 1 for r in r16],
                                                                      [r.iters + 1 for r in r_warm]))
        assert all(r.state == _lib.ST_OK for r in r_warm)             # by the f32 batch's own stopping test, on the exact matrix
    finally:
        sb.destroy()
        cold.destroy()


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_nothing_allocated(T):
    from totsu_amd import _lib
    from totsu_amd._lib import lib
    S = T.Mid16BatchSolver
    z = lambda *s: np.zeros(s, F)
    ds, _ = _family(T, "lp80")
    keep = S.from_dense(ds)
    before = keep.info()["device_bytes_all"]
    assert before == keep.info()["device_bytes"] > keep.info()["a_store_bytes"] > 0 and keep.info()["a_dtype"] == "f16"
    bad = [lambda: S(3, 6, z(2, 18), z(2, 6), z(2, 3), [_lib.CONE_PSD], [6]),
           lambda: S(3, 6, z(2, 18), z(2, 6), z(2, 3), [1], [6], a_dtype="f32"),
           lambda: S(3, 6, z(2, 18), z(2, 6), z(2, 3), [1], [6], a_dtype="f8"),
           lambda: S(2, 4097, z(1, 2 * 4097), z(1, 4097), z(1, 2), [1], [4097]),
           lambda: S(1000, 2020, z(1, 1), z(1, 2020), z(1, 1000), [1], [2020]),
           lambda: S(3, 6, z(2, 17), z(2, 6), z(2, 3), [1], [6]),
           lambda: S(3, 6, z(2, 18), z(2, 6), z(3, 3), [1], [6]),
           lambda: keep.set_a_dev(None),
           lambda: keep.set_a([z(5)], first=0),
           lambda: keep.replace(0, z(5), ds[0].vec_b, ds[0].vec_c)]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    with pytest.raises(ValueError, match="PSD"):
        S(3, 6, z(2, 18), z(2, 6), z(2, 3), [_lib.CONE_PSD], [6])
    with pytest.raises(ValueError, match="MidBatchSolver"):
        S(3, 6, z(2, 18), z(2, 6), z(2, 3), [1], [6], a_dtype="f32")
    assert keep.info()["device_bytes_all"] == before
    # the C ABI itself
    da, db, dc = (T.DeviceBuffer.from_host(z(64)) for _ in range(3))
    par = _lib.Param(-1, 1e-6, 1e-6, 1e-12, 0, 0, 0)

    def create(n, m, P, st, sl, kind, match):
        st, sl = np.asarray(st, np.int32), np.asarray(sl, np.int64)
        h = C.c_void_p()
        with pytest.raises(_lib.ThipError, match=match) as e:
            lib.thip_mid16batch_create_kind(n, m, P, da.ptr, db.ptr, dc.ptr, None, st.size, st.ctypes.data_as(C.POINTER(C.c_int32)),
                                            sl.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(par), kind, C.byref(h))
        assert e.value.code == _lib.E_INVALID and not h.value
        assert keep.info()["device_bytes_all"] == before

    create(3, 6, 2, [_lib.CONE_PSD], [6], M.A_F16, "mid16 batch takes no PSD")
    create(3, 8, 2, [1, _lib.CONE_PSD], [2, 6], M.A_BF16, "mid16 batch takes no PSD")
    create(3, 6, 2, [1], [6], 0, "thip_midbatch")
    create(3, 6, 2, [1], [6], 3, "unknown stored form")
    create(2, 4097, 1, [1], [4097], M.A_F16, "4096")
    create(1000, 2020, 1, [1], [2020], M.A_F16, "LDS")
    create(3, 6, 2, [1], [5], M.A_F16, "cover")
    create(3, 6, 0, [1], [6], M.A_F16, "mid16 batch holds")
    with pytest.raises(_lib.ThipError, match="no f32 A lies in place"):
        lib.thip_mid16batch_set_a_dev(keep.h, 0, 1, None, 0)
    assert keep.info()["device_bytes_all"] == before
    for d in (da, db, dc):
        d.free()
    keep.run(3)
    assert all(keep.status(i).iters == 3 for i in range(len(ds)))     # and the batch is as it was: running
    sb2 = S.from_dense(ds[:2], a_dtype="bf16")
    assert sb2.info()["device_bytes_all"] == before + sb2.info()["device_bytes"]
    sb2.destroy()
    assert keep.info()["device_bytes_all"] == before
    keep.destroy()


def test_no_chooser_returns_the_family(T):
    lp260, _ = _family(T, "lp260")
    mid = T.own_a_batch(lp260[:2])
    assert type(mid) is T.MidBatchSolver
    mid.destroy()
