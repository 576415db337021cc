"""GPU: start iterates of the single solver and of the shared-A batch (thip_solver_set_iterate, thip_batch_set_iterate; set_iterate /
raw_iterate / replace(start=) / stream(warm=) / solve_many(warm=) in Python).  The schedules without carried products continue bit
for bit from their own iterate; every schedule started at the oracle's snapshot after iteration k reaches the oracle's snapshot at
k + j, at what the solver's own oracle tests hold an iterate to (tests/test_gpu_solver.py, tests/test_gpu_sweep.py: 2e-5 at iterates
0 and 1, 1e-4 at 9, 2e-3 at 99) and between those iterates their geometric interpolation (tests/warm_cases.py::iterate_tol); a started slot of a batch touches no other slot; a warm path gives the cold path's answers.
Everything runs with gemv_autotune=False, so that two solvers of one problem run one tiling."""
import copy

import numpy as np
import pytest

import oracle as O
import warm_numpy as W
from ownbatch_cases import F, T, _D, _edge  # noqa: F401  (T: the fixture)
from problems import benchmark_lp
from warm_cases import J_RUN, K_START, SNAPS, iterate_tol, oracle_run, snap_xy, socp_numpy, sparse40x30

pytestmark = pytest.mark.gpu


def _tol(it):
    return iterate_tol(it)


def _param(T, arith=None, **kw):
    p = T.SolverParam()
    p.eps_acc = 1e-30
    if arith:
        p.state_arith = arith
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _rel(got, want):
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-6)


_MADE = {}


def problem(name):
    """(dense problem, SOCP pieces or None): lp80x40, lp2504x1252 (the shape the one-pass kernel takes), socp102x12, sp40x30"""
    if name not in _MADE:
        if name == "lp80x40":
            _MADE[name] = (_edge(80, 40, 0), None)
        elif name == "lp2504x1252":
            c, G, h = benchmark_lp(1252, seed=0)
            _MADE[name] = (_D(G, h, c, [1], [2504]), None)
        elif name == "socp102x12":
            _MADE[name] = socp_numpy(0)
        else:
            assert name == "sp40x30", name
            _MADE[name] = (sparse40x30(0), None)
    return _MADE[name]


def _matrix(d, form):
    if form == "dense":
        return d.mat_a
    import scipy.sparse as sp
    return sp.csr_matrix(np.asarray(d.mat_a, F).reshape(d.n, d.m).T)


def make(T, d, p, schedule, form="dense", **kw):
    """form: dense, tiled (the tiled sparse copy) or csr2 (the two CSR copies)"""
    return T.FusedSolver(d.n, d.m, _matrix(d, form), d.vec_b, d.vec_c, d.seg_type, d.seg_len, p, schedule, vec_b_rowabs=d.vec_b_rowabs,
                         gemv_autotune=False, sweep_min_bytes=0, sparse_two_copies=form == "csr2", **kw)


def _state(fs):
    st = fs.status()
    return fs.iterate() + ((st.state, st.iters, st.kind, tuple(st.cri)),)


# ---- 8. bitwise continuation: the schedules that carry no products ----------------------------------------------------------------

@pytest.mark.parametrize("schedule", ["reference", "fused"])
@pytest.mark.parametrize("name,form", [("lp80x40", "dense"), ("socp102x12", "dense"), ("lp2504x1252", "dense"), ("sp40x30", "tiled"),
                                       ("sp40x30", "csr2")])
def test_bitwise_continuation(T, name, form, schedule):
    d, _ = problem(name)
    p = _param(T, "plain")
    for hand, poll in ((10, 64), (1, 1), (10, 7)):
        R, S = make(T, d, p, schedule, form), make(T, d, p, schedule, form)
        try:
            R.run(hand, poll_every=poll)
            S.set_iterate(*R.iterate())
            st = S.status()
            assert st.state == -1 and st.iters == 0 and tuple(st.cri) == (0.0, 0.0, 0.0)
            S.run(10, poll_every=poll)
            R.run(10, poll_every=poll)
            r, s = _state(R), _state(S)
            assert np.array_equal(r[0], s[0]) and np.array_equal(r[1], s[1]), (name, form, schedule, hand, poll)
            assert r[2][0] == s[2][0] == -1 and r[2][2:] == s[2][2:] and s[2][1] == 10 and r[2][1] == hand + 10, (r[2], s[2])
        finally:
            R.destroy()
            S.destroy()


# ---- 9. oracle parity: every schedule, every stored form ----------------------------------------------------------------------------

CASES = [(n, "dense", s) for n in ("lp80x40", "socp102x12") for s in ("reference", "fused", "carried")] + \
        [("lp2504x1252", "dense", s) for s in ("fused", "carried", "sweep")] + \
        [("sp40x30", f, s) for f in ("tiled", "csr2") for s in ("fused", "carried")] + [("sp40x30", "tiled", "sweep")]


def _parity(T, label, d, ro, build, want_schedule):
    worst = 0.0
    for k in K_START:
        for j in J_RUN:
            fs = build()
            try:
                assert fs.schedule_in_use() == want_schedule, (label, fs.schedule_in_use())
                x0, y0 = snap_xy(ro, d, k)
                fs.set_iterate(x0.astype(F), y0.astype(F))
                fs.run(j, poll_every=64)
                assert fs.schedule_in_use() == want_schedule
                x, y = fs.iterate()
                rx, ry = snap_xy(ro, d, k + j)
                tol = _tol(k + j)
                ex, ey = _rel(x, rx), _rel(y, ry)
                worst = max(worst, ex, ey)
                print("warm solver %s start %d + %d: err x %.2e y %.2e (tol %.2e)" % (label, k, j, ex, ey, tol))
                assert ex <= tol and ey <= tol, (label, k, j, ex, ey)
                st, tr = fs.status(), ro.trace[k + j]
                assert st.state == -1 and st.iters == j and st.kind == tr[1], (label, k, j, st.iters, st.kind)
                assert np.allclose(st.cri, tr[2:], rtol=max(50 * tol, 1e-3), atol=1e-5), (label, k, j, st.cri, tr)
            finally:
                fs.destroy()
    print("warm solver %s worst error %.2e" % (label, worst))


@pytest.mark.parametrize("name,form,schedule", CASES)
def test_oracle_parity(T, name, form, schedule):
    d, pieces = problem(name)
    ro = oracle_run("solver/" + name, d, socp=pieces)
    _parity(T, "%s %s %s" % (name, form, schedule), d, ro, lambda: make(T, d, _param(T), schedule, form), schedule)


def test_oracle_parity_f16_storage(T):
    # the stored matrix is another (rounded) matrix: the oracle runs on the dequantised one (tests/test_gpu_bf16.py)
    from test_gpu_bf16 import f16_quantize
    d, _ = problem("lp80x40")
    dr = copy.copy(d)
    A = np.asarray(d.mat_a, F).reshape((d.n, d.m)).T
    dr.mat_a = np.asfortranarray(f16_quantize(A)[2]).ravel(order="F")
    ro = O.solve_matop_cones(O.param(max_iter=max(SNAPS) + 2, eps_acc=1e-30), dr.vec_c, dr.mat_a, dr.vec_b, dr.seg_type, dr.seg_len,
                             snap_iters=SNAPS, trace_cap=max(SNAPS) + 3, use_ql=True)
    _parity(T, "lp80x40 f16 carried", d, ro, lambda: make(T, d, _param(T), "carried", a_storage="f16"), "carried")


# ---- 10. the shared-A batch ---------------------------------------------------------------------------------------------------------

def _box(n=40, B=8):
    rng = np.random.default_rng(2024)
    A = np.vstack([np.eye(n), -np.eye(n)]).astype(F)
    d = _D(A, np.ones(2 * n), np.ones(n), [1], [2 * n])
    bs = [rng.uniform(0.5, 1.5, 2 * n).astype(F) for _ in range(B + 1)]
    cs = [rng.standard_normal(n).astype(F) for _ in range(B + 1)]
    return d, bs, cs


def test_batch_replace_with_start_leaves_the_other_slots_alone(T):
    d, bs, cs = _box()
    B, i = 8, 3
    p = _param(T, "plain")
    mk = lambda vb, vc: T.BatchSolver.from_dense(d, vb, vc, p, gemv_autotune=False)        # noqa: E731
    warm, cold = mk(bs[:B], cs[:B]), mk(bs[:B], cs[:B])
    held_b, held_c = list(bs[:B]), list(cs[:B])
    held_b[i], held_c[i] = bs[B], cs[B]
    fresh = mk(held_b, held_c)
    try:
        for b in (warm, cold):
            b.run(10, poll_every=5)
        x, y = warm.iterate(i)
        warm.replace(i, bs[B], cs[B], start=(x, y))
        cold.replace(i, bs[B], cs[B])
        fresh.set_iterate(i, x, y)
        assert warm.counters()["replaced"] == cold.counters()["replaced"] == 1 and warm.status(i).iters == 0
        new = copy.copy(d)
        new.vec_b, new.vec_c = bs[B], cs[B]
        ref = W.run(W.Problem.of_dense(new), 10, start=(x, y), snap_iters=(0, 9))
        done = 0
        for j in (1, 10):
            for b in (warm, cold, fresh):
                b.run(j - done, poll_every=5)
            done = j
            for q in range(B):
                if q != i:                                           # bit for bit what they are without the start
                    assert all(np.array_equal(a, c) for a, c in zip(warm.iterate(q), cold.iterate(q))), (j, q)
                    assert warm.status(q).iters == 10 + j
            gx, gy = warm.iterate(i)
            assert all(np.array_equal(a, c) for a, c in zip((gx, gy), fresh.iterate(i))), j
            st, sf = warm.status(i), fresh.status(i)
            assert (st.state, st.iters, st.kind, tuple(st.cri)) == (sf.state, sf.iters, sf.kind, tuple(sf.cri)) and st.iters == j
            ex, ey = _rel(gx, ref.snaps[j - 1][0]), _rel(gy, ref.snaps[j - 1][1])
            print("warm batch replace(start) + %d: err x %.2e y %.2e (tol %.0e)" % (j, ex, ey, _tol(j - 1)))
            assert ex <= _tol(j - 1) and ey <= _tol(j - 1), (j, ex, ey)
    finally:
        for b in (warm, cold, fresh):
            b.destroy()


def test_solve_many_warm_gives_the_cold_answers(T):
    # a path of 12 LPs, 80 x 40 over a shared A: c_k = c + lambda_k d, every c_k < 0 as benchmark_lp's c is (bounded)
    c, G, h = benchmark_lp(40, seed=0)
    d = _D(G, h, c, [1], [80])
    w = np.random.default_rng(5).uniform(0, 1, 40)
    cs = [(c * (1 + 0.03 * k * w)).astype(F) for k in range(12)]
    bs = [d.vec_b] * 12
    p = _param(T, eps_acc=1e-5, eps_inf=1e-5, max_iter=400000)
    cold = T.solve_many(d, bs, cs, slots=8, param=p, poll_every=64, gemv_autotune=False)
    warm = T.solve_many(d, bs, cs, slots=8, param=p, poll_every=64, warm=True, gemv_autotune=False)
    assert len(cold) == len(warm) == 12 and cold.counters["replaced"] == warm.counters["replaced"] == 4
    for k in range(12):
        (rc, xc, _), (rw, xw, _) = cold[k], warm[k]
        assert rc.state == rw.state == 0, (k, rc.state, rw.state)
        err = np.abs(xw - xc).max() / max(1.0, np.abs(xc).max())
        print("warm path problem %2d: %6d iterations cold, %6d warm, answers differ by %.2e" % (k, rc.iters + 1, rw.iters + 1, err))
        assert err <= 2e-3, (k, err)
        ck = cs[k].astype(np.float64)                                # its own result: no other problem's answer does better under c_k
        for other in range(12):                                      # (neighbours of the path may share their vertex: equality is fine)
            assert ck @ xw <= ck @ cold[other][1] + 2e-3 * max(1.0, abs(ck @ xw)), (k, other)
    print("warm path: %d instance-iterations cold, %d warm" % (cold.counters["instance_iterations"], warm.counters["instance_iterations"]))


# ---- 11. refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(T, monkeypatch):
    from totsu_amd import _lib
    d, _ = problem("lp80x40")
    p = _param(T)
    fs = make(T, d, p, "carried")
    bt = T.BatchSolver.from_dense(d, [d.vec_b] * 2, [d.vec_c] * 2, p, gemv_autotune=False)
    try:
        fs.run(2, poll_every=2)
        bt.run(2, poll_every=2)
        x, y = fs.iterate()
        want = _state(fs)
        want_b = bt.iterate(1)

        def bad(xx, yy):
            with pytest.raises(ValueError):
                fs.set_iterate(xx, yy)
            with pytest.raises(ValueError):
                bt.set_iterate(1, xx, yy)
            with pytest.raises(ValueError):
                bt.replace(1, d.vec_b, d.vec_c, start=(xx, yy)) if xx.size != x.size or yy.size != y.size else bt.set_iterate(1, xx, yy)
            g = _state(fs)
            assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]) and g[2] == want[2]
            assert all(np.array_equal(a, b) for a, b in zip(bt.iterate(1), want_b))
        bad(x[:-1], y)
        bad(x, np.concatenate([y, y[:1]]))
        for v in (-1.0, np.nan, np.inf):
            z = x.copy()
            z[-1] = v
            bad(z, y)
        for v in (1.0, np.nan, -np.inf):
            z = y.copy()
            z[-1] = v
            bad(x, z)
        for i in (-1, 2):
            with pytest.raises(ValueError):
                bt.set_iterate(i, x, y)
        L = _lib.load()
        px, py = x.ctypes.data, y.ctypes.data
        for args in ((None, px, py), (fs.h, None, py), (fs.h, px, None)):
            assert L.thip_solver_set_iterate(*args) == _lib.E_INVALID
        for args in ((None, 0, px, py), (bt.h, 2, px, py), (bt.h, -1, px, py), (bt.h, 0, None, py), (bt.h, 0, px, None)):
            assert L.thip_batch_set_iterate(*args) == _lib.E_INVALID
        for bx, by in ((-1.0, None), (None, 1.0)):                   # the library's own word on tau and kappa (Python checks them first)
            zx, zy = x.copy(), y.copy()
            if bx is not None:
                zx[-1] = bx
            if by is not None:
                zy[-1] = by
            assert L.thip_solver_set_iterate(fs.h, zx.ctypes.data, zy.ctypes.data) == _lib.E_INVALID
            assert L.thip_batch_set_iterate(bt.h, 1, zx.ctypes.data, zy.ctypes.data) == _lib.E_INVALID
        # handles that were created and not initialised: the classes' own constructors with the init call left out
        with monkeypatch.context() as mp:
            mp.setattr(_lib.lib, "thip_solver_init", lambda h: 0, raising=False)
            mp.setattr(_lib.lib, "thip_batch_init", lambda h: 0, raising=False)
            raw_s = make(T, d, p, "carried")
            raw_b = T.BatchSolver.from_dense(d, [d.vec_b] * 2, [d.vec_c] * 2, p, gemv_autotune=False)
        try:
            assert L.thip_solver_set_iterate(raw_s.h, px, py) == _lib.E_INVALID
            assert L.thip_batch_set_iterate(raw_b.h, 0, px, py) == _lib.E_INVALID
            with pytest.raises(ValueError):
                raw_s.set_iterate(x, y)
            with pytest.raises(ValueError):
                raw_b.set_iterate(0, x, y)
        finally:
            raw_s.destroy()
            raw_b.destroy()
        g = _state(fs)
        assert np.array_equal(g[0], want[0]) and np.array_equal(g[1], want[1]) and g[2] == want[2]
        fs.run(2, poll_every=2)                                      # and both still run
        bt.run(2, poll_every=2)
        assert fs.status().iters == 4 and [bt.status(i).iters for i in range(2)] == [4, 4]
        # a bare set_iterate retires the slot's iterations into the counter, as a replace does
        assert bt.counters()["instance_iterations"] == 8
        bt.set_iterate(1, *bt.iterate(1))
        assert bt.status(1).iters == 0 and bt.counters()["instance_iterations"] == 8
        bt.run(3, poll_every=3)
        assert bt.counters()["instance_iterations"] == 8 + 6 and bt.counters()["replaced"] == 0
    finally:
        fs.destroy()
        bt.destroy()
    # a solver with an all-reduce callback (a world of one rank: the sum is the buffer itself), and one with a column shard set
    hook = lambda ctx, buf, count, stream: 0        # noqa: E731
    ar = make(T, d, p, "carried", allreduce=hook)
    big, _ = problem("lp2504x1252")
    xb, yb = np.zeros(big.n + 2 * big.m + 1, F), np.zeros(big.n + big.m + 1, F)
    xb[-1] = 1.0
    cs = make(T, big, p, "sweep", allreduce=hook, col_shard=True)
    try:
        ar.run(1, poll_every=1)
        with pytest.raises(ValueError):
            ar.set_iterate(x, y)
        assert ar.status().iters == 1
        with pytest.raises(ValueError):
            cs.set_iterate(xb, yb)
    finally:
        ar.destroy()
        cs.destroy()
