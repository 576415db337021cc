"""GPU: a batch of problems that share A (totsu_amd.BatchSolver / thip_batch_*): the multi-vector dual GEMV alone against f64
numpy, every instance's iterates against the f64 oracle, independent termination, a batch of one against FusedSolver, A held once,
the refusals."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from problems import benchmark_lp, random_sdp, random_socp

pytestmark = pytest.mark.gpu

TOLS = [2e-5, 2e-5, 1e-4, 2e-3]      # iterates 0, 1, 9, 99 relative to the iterate's max norm (tests/test_gpu_solver.py)


@pytest.fixture(scope="module")
def T():
    import totsu_amd
    from totsu_amd import _lib
    _lib.init()
    return totsu_amd


def _mb(T, typ):
    return T.MatBuild(T.F32HIP, typ)


# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------

def _ptrs(bufs):
    return (C.c_void_p * len(bufs))(*[b.ptr for b in bufs])


_KERNEL_INPUTS = {}


def _kernel_inputs(m, n):
    """A, eight vector pairs scaled by 10^U(-3, 3) per instance, and their f64 products with the componentwise bound -- made once per shape"""
    if (m, n) not in _KERNEL_INPUTS:
        rng = np.random.default_rng(1000 * m + n)
        a = rng.standard_normal((m, n)).astype(np.float32)
        xn = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32) for _ in range(8)]
        xt = [(rng.standard_normal(m) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32) for _ in range(8)]
        a64, aa = a.astype(np.float64), np.abs(a.astype(np.float64))
        ref = [(a64 @ xn[i].astype(np.float64), a64.T @ xt[i].astype(np.float64), 1e-5 * (aa @ np.abs(xn[i].astype(np.float64))),
                1e-5 * (aa.T @ np.abs(xt[i].astype(np.float64)))) for i in range(8)]
        _KERNEL_INPUTS[(m, n)] = (a, xn, xt, ref)
    return _KERNEL_INPUTS[(m, n)]


@pytest.mark.parametrize("nv,nj", [(2, 1), (3, 1), (4, 1), (5, 1), (8, 1), (2, 2), (3, 2), (4, 2)])
@pytest.mark.parametrize("m,n", [(80, 40), (1028, 7), (2504, 300), (4096 + 4, 513)])
def test_multi_vector_kernel_against_numpy(T, m, n, nv, nj):
    """m % 16 != 0 (the padded copy), a partial last row tile, several column chunks, fewer columns than a chunk; nv = 3 and 5 leave
    slots of the NV = 4 / 8 instance unused; one instance has its stop flag set; nj = 2: the two-row-group tiling of NV = 2 and 4"""
    from totsu_amd import _lib
    from totsu_amd._lib import lib
    a, xn, xt, ref = _kernel_inputs(m, n)
    D = T.DeviceBuffer
    da = D.from_host(np.asfortranarray(a).ravel(order="F"))
    dxn, dxt = [D.from_host(v) for v in xn[:nv]], [D.from_host(v) for v in xt[:nv]]
    stopped = nv // 2                                    # this slot's stop flag is set
    flags = (C.c_int * nv)(*[1 if i == stopped else 0 for i in range(nv)])
    outs = []
    for _ in range(2):                                   # two launches on the same inputs
        on = [D.from_host(np.full(m, 7.0, np.float32)) for _ in range(nv)]
        ot = [D.from_host(np.full(n, 7.0, np.float32)) for _ in range(nv)]
        ms = C.c_float()
        lib.thip_test_gemv_multi(m, n, da.ptr, nv, _ptrs(dxn), _ptrs(dxt), _ptrs(on), _ptrs(ot), flags, nj, 0, 1, C.byref(ms))
        outs.append(([b.to_host() for b in on], [b.to_host() for b in ot]))
        for b in on + ot:
            b.free()
    for i in range(nv):
        gn, gt = outs[0][0][i], outs[0][1][i]
        if i == stopped:                                 # no work that changes its state
            assert (gn == 7.0).all() and (gt == 7.0).all()
            continue
        rn, rt, bn, bt = ref[i]
        en, et = np.abs(gn - rn), np.abs(gt - rt)
        print("m=%d n=%d nv=%d nj=%d slot %d: max err / bound N %.3f T %.3f" % (m, n, nv, nj, i, (en / np.maximum(bn, 1e-300)).max(),
                                                                              (et / np.maximum(bt, 1e-300)).max()))
        assert (en <= bn).all(), (i, (en / np.maximum(bn, 1e-300)).max())
        assert (et <= bt).all(), (i, (et / np.maximum(bt, 1e-300)).max())
        assert np.array_equal(gn, outs[1][0][i]) and np.array_equal(gt, outs[1][1][i])      # bitwise reproducible
    for b in [da] + dxn + dxt:
        b.free()


# ---- 2. / 3. iterates of every instance against the f64 oracle ----------------------------------------------------------------

def _instances(dense, B, kind):
    """b_i, c_i of instance i drawn from seed i: the LP generator's own distributions (c = -U(0, 1), h = [0; U(0, 1)]); for the
    cone programs a 1 % perturbation of the template's b (its strictly feasible point stays one) and a 10 % one of its c"""
    b0, c0 = np.asarray(dense.vec_b, np.float32), np.asarray(dense.vec_c, np.float32)
    bs, cs = [], []
    for i in range(B):
        rng = np.random.default_rng(i)
        if kind == "lp":
            n = dense.n
            cs.append((-rng.uniform(0, 1, n)).astype(np.float32))
            bs.append(np.concatenate([np.zeros(n), rng.uniform(0, 1, n)]).astype(np.float32))
        else:
            cs.append((c0 + 0.1 * np.abs(c0).max() * rng.standard_normal(c0.size)).astype(np.float32))
            bs.append((b0 + 0.01 * np.abs(b0).max() * rng.standard_normal(b0.size)).astype(np.float32))
    return bs, cs


def _oracle_snaps(dense, b, c, iters):
    par = O.param(max_iter=max(iters) + 2, eps_acc=1e-30)
    return O.solve_matop_cones(par, c, dense.mat_a, b, dense.seg_type, dense.seg_len, snap_iters=iters, trace_cap=max(iters) + 3,
                               use_ql=True)


def _check_batch_iterates(T, dense, bs, cs, iters, tols, check_precond=True, **kw):
    """_check_iterates of tests/test_gpu_solver.py for every instance of a batch"""
    B = len(bs)
    ros = [_oracle_snaps(dense, bs[i], cs[i], iters) for i in range(B)]
    p = T.SolverParam()
    p.eps_acc = 1e-30
    bt = T.BatchSolver.from_dense(dense, bs, cs, p, **kw)
    N = dense.n + 2 * dense.m + 1
    if check_precond:
        for i in range(B):
            t, s = bt.precond(i)
            assert np.allclose(t, ros[i].precond[:N], rtol=2e-5, atol=0), (i, np.abs(t / ros[i].precond[:N] - 1).max())
            assert np.allclose(s, ros[i].precond[N:], rtol=2e-5, atol=0), (i, np.abs(s / ros[i].precond[N:] - 1).max())
    done = 0
    for q, (it, tol) in enumerate(zip(iters, tols)):
        bt.run(it + 1 - done, poll_every=64)
        done = it + 1
        for i in range(B):
            x, y = bt.iterate(i)
            rx, ry = ros[i].snaps[q][:N], ros[i].snaps[q][N:]
            sx, sy = max(np.abs(rx).max(), 1e-6), max(np.abs(ry).max(), 1e-6)
            print("instance %d iterate %d: err x %.2e y %.2e (tol %.0e)" % (i, it, np.abs(x - rx).max() / sx, np.abs(y - ry).max() / sy, tol))
            assert np.abs(x - rx).max() <= tol * sx, (i, it, np.abs(x - rx).max() / sx)
            assert np.abs(y - ry).max() <= tol * sy, (i, it, np.abs(y - ry).max() / sy)
            st = bt.status(i)
            assert st.iters == it + 1 or st.iters == it
            tr = ros[i].trace[it]
            assert np.allclose(st.cri, tr[2:], rtol=max(50 * tol, 1e-3), atol=1e-5), (i, it, st.cri, tr)
    return bt


def _lp_dense(T, sz, seed=1):
    c, G, h = benchmark_lp(sz, seed=seed)
    lp = T.ProbLP(_mb(T, T.MatType.General(sz, 1)).set_array(c.reshape(-1, 1)), _mb(T, T.MatType.General(2 * sz, sz)).set_array(G),
                  _mb(T, T.MatType.General(2 * sz, 1)).set_array(h.reshape(-1, 1)), _mb(T, T.MatType.General(0, sz)),
                  _mb(T, T.MatType.General(0, 1)))
    return lp.dense()


def _socp_dense(T):
    n, cones = 30, [5, 1, 0, 17, 99, 3]
    f, Gs, hs, cs, d = random_socp(n, cones, seed=2)
    socp = T.ProbSOCP(_mb(T, T.MatType.General(n, 1)).set_array(f.reshape(-1, 1)),
                      [_mb(T, T.MatType.General(G.shape[0], n)).set_array(G) for G in Gs],
                      [_mb(T, T.MatType.General(len(h_), 1)).set_array(h_.reshape(-1, 1)) for h_ in hs],
                      [_mb(T, T.MatType.General(n, 1)).set_array(c_.reshape(-1, 1)) for c_ in cs], d,
                      _mb(T, T.MatType.General(0, n)), _mb(T, T.MatType.General(0, 1)))
    return socp.dense()


def test_batch_iterates_lp(T):
    dense = _lp_dense(T, 40)
    bs, cs = _instances(dense, 3, "lp")
    _check_batch_iterates(T, dense, bs, cs, [0, 1, 9, 99], TOLS).destroy()


def test_batch_iterates_socp(T):
    dense = _socp_dense(T)
    bs, cs = _instances(dense, 3, "cone")
    _check_batch_iterates(T, dense, bs, cs, [0, 1, 9, 99], TOLS).destroy()


def test_batch_iterates_lp_multi_chunk(T):
    """m = 2504 (the padded copy, three row tiles, many column chunks), B = 5 on the NV = 8 instance, inside the loop"""
    dense = _lp_dense(T, 1252)
    bs, cs = _instances(dense, 5, "lp")
    _check_batch_iterates(T, dense, bs, cs, [0, 1, 9], TOLS[:3]).destroy()


def test_batch_iterates_sdp(T):
    n, k = 6, 24
    c, syms = random_sdp(n, k, seed=3)
    sdp = T.ProbSDP(_mb(T, T.MatType.General(n, 1)).set_array(c.reshape(-1, 1)),
                    [_mb(T, T.MatType.SymPack(k)).set_array(s) for s in syms],
                    _mb(T, T.MatType.General(0, n)), _mb(T, T.MatType.General(0, 1)), 1e-12)
    dense = sdp.dense()
    bs, cs = _instances(dense, 2, "cone")
    _check_batch_iterates(T, dense, bs, cs, [0, 1, 9], TOLS[:3]).destroy()


# ---- 4. independent termination --------------------------------------------------------------------------------------------

def test_instances_terminate_independently(T):
    """A = [I; -I] (x <= b[:2], -x <= b[2:]) over the nonnegative cone: a feasible box, x <= -1 and x >= 1 (infeasible), a second
    feasible box with another c.  Each instance ends in the oracle's state; one that stopped earlier stays frozen."""
    from totsu_amd import _lib
    a = np.vstack([np.eye(2), -np.eye(2)]).astype(np.float32)
    bs = [np.array([1, 1, 1, 1], np.float32), np.array([-1, -1, -1, -1], np.float32), np.array([2, 3, 1, 0.5], np.float32)]
    cs = [np.array([1, 1], np.float32), np.array([1, 1], np.float32), np.array([-1, 2], np.float32)]
    want_x = [np.array([-1., -1.]), None, np.array([2., -0.5])]
    ros = [O.solve_matop_cones(O.param(max_iter=100000, eps_acc=1e-5), cs[i], a, bs[i], [O.CONE_RPOS], [4]) for i in range(3)]
    assert [r.status for r in ros] == [O.OK, O.INFEASIBLE, O.OK]              # confirmed on the CPU first
    for i in (0, 2):
        assert np.allclose(ros[i].x, want_x[i], atol=1e-3)
    p = T.SolverParam()
    p.max_iter, p.eps_acc = 100_000, 1e-5
    bt = T.BatchSolver(2, 4, np.asfortranarray(a).ravel(order="F"), bs, cs, [_lib.CONE_RPOS], [4], p)
    frozen, first = {}, None
    for _ in range(100000 // 8):
        res = bt.run(8, poll_every=8)
        for i, r in enumerate(res):
            if r.state != _lib.ST_RUNNING and i not in frozen:
                frozen[i] = (r.iters, bt.iterate(i))
                first = i if first is None else first
        if len(frozen) == 3:
            break
    assert len(frozen) == 3
    states = {O.OK: _lib.ST_OK, O.INFEASIBLE: _lib.ST_INFEASIBLE}
    iters = [frozen[i][0] for i in range(3)]
    assert len(set(iters)) > 1, iters                      # they did stop at different iterations
    for i in range(3):
        st = bt.status(i)
        assert st.state == states[ros[i].status], (i, st.state)
        print("instance %d: state %d after %d iterations (oracle %d)" % (i, st.state, st.iters, ros[i].iters))
        # frozen since it stopped: the same iteration count and bitwise the same iterate after the others have finished
        x, y = bt.iterate(i)
        assert st.iters == frozen[i][0]
        assert np.array_equal(x, frozen[i][1][0]) and np.array_equal(y, frozen[i][1][1]), i
        if want_x[i] is not None:
            xs, _ = bt.solution(i)
            assert np.allclose(xs, want_x[i], atol=1e-3), (i, xs)
    sol = bt.solve()
    assert isinstance(sol[1], T.SolverError) and sol[1].kind == T.SolverError.Infeasible
    bt.destroy()


# ---- 5. a batch of one and an arbitrary B -----------------------------------------------------------------------------------

def test_batch_of_one_is_the_carried_solver(T):
    dense = _lp_dense(T, 40)
    bs, cs = _instances(dense, 1, "lp")
    iters = [0, 1, 9]
    p = T.SolverParam()
    p.eps_acc = 1e-30
    fs = T.FusedSolver(dense.n, dense.m, dense.mat_a, bs[0], cs[0], dense.seg_type, dense.seg_len, p, "carried")
    bt = T.BatchSolver.from_dense(dense, bs, cs, p)
    assert bt.info()["group_sizes"] == [1]
    done = 0
    for it, tol in zip(iters, TOLS):
        fs.run(it + 1 - done, poll_every=64)
        bt.run(it + 1 - done, poll_every=64)
        done = it + 1
        (fx, fy), (bx, by) = fs.iterate(), bt.iterate(0)
        assert np.abs(bx - fx).max() <= tol * max(np.abs(fx).max(), 1e-6) and np.abs(by - fy).max() <= tol * max(np.abs(fy).max(), 1e-6)
    fs.destroy()
    bt.destroy()
    # the same final state
    p = T.SolverParam()
    p.max_iter, p.eps_acc = 100_000, 1e-4
    fs = T.FusedSolver(dense.n, dense.m, dense.mat_a, bs[0], cs[0], dense.seg_type, dense.seg_len, p, "carried")
    bt = T.BatchSolver.from_dense(dense, bs, cs, p)
    fr, br = fs.run(), bt.run()[0]
    assert (br.state, br.kind) == (fr.state, fr.kind) and abs(br.iters - fr.iters) <= 2, (br.state, br.iters, fr.state, fr.iters)
    (fx, fy), (bx, by) = fs.solution(), bt.solution(0)
    assert np.allclose(bx, fx, atol=1e-3) and np.allclose(by, fy, atol=1e-3)
    fs.destroy()
    bt.destroy()


def test_batch_of_eleven_two_groups(T):
    """B = 11: a group of 8 (NV = 8) and a group of 3 (NV = 4 with a slot unused); every instance's iterate 9 against the oracle,
    and two runs of the same batch with the autotune off are bitwise identical"""
    dense = _lp_dense(T, 40)
    bs, cs = _instances(dense, 11, "lp")
    bt = _check_batch_iterates(T, dense, bs, cs, [9], [TOLS[2]], check_precond=False, gemv_autotune=False)
    assert bt.info()["group_sizes"] == [8, 3] and bt.info()["passes_per_iteration"] == 4
    first = [bt.iterate(i) for i in range(11)]
    bt.reinit()
    bt.run(10, poll_every=64)
    for i in range(11):
        x, y = bt.iterate(i)
        assert np.array_equal(x, first[i][0]) and np.array_equal(y, first[i][1]), i
    bt.destroy()


# ---- 6. A is held once -------------------------------------------------------------------------------------------------------

def test_a_is_held_once(T):
    dense = _lp_dense(T, 1252)                             # m = 2504: needs the padded copy
    bs, cs = _instances(dense, 4, "lp")
    bt = T.BatchSolver.from_dense(dense, bs, cs)
    info = bt.info()
    bytes_a = 4 * dense.m * dense.n
    assert info["a_copies"] == 1 and bytes_a <= info["a_bytes"] <= 4 * (dense.m + 15) * dense.n
    assert info["device_bytes"] < 1.5 * bytes_a + info["arena_bytes"], info
    assert info["groups"] == 1 and info["passes_per_iteration"] == 2 and info["bytes_per_pass"] == bytes_a
    bt.destroy()
    d40 = _lp_dense(T, 40)                                  # m = 80: the caller's array as it is, no copy
    bs, cs = _instances(d40, 2, "lp")
    bt = T.BatchSolver.from_dense(d40, bs, cs)
    assert bt.info()["a_copies"] == 0 and bt.info()["a_bytes"] == 0
    bt.destroy()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------

def test_refusals(T):
    import scipy.sparse as sp
    from totsu_amd import _lib
    from totsu_amd._lib import lib
    dense = _lp_dense(T, 40)
    bs, cs = _instances(dense, 3, "lp")
    bad = (ValueError, _lib.ThipError)

    def refused(fn):
        with pytest.raises(bad) as e:
            fn()
        assert not isinstance(e.value, _lib.ThipError) or e.value.code == _lib.E_INVALID

    refused(lambda: T.BatchSolver.from_dense(dense, [], []))                                     # n_inst = 0
    refused(lambda: T.BatchSolver.from_dense(dense, [bs[0]] * 65, [cs[0]] * 65))                 # n_inst = 65
    refused(lambda: T.BatchSolver.from_dense(dense, bs, cs, a_storage="bf16"))                   # 16-bit storage
    refused(lambda: T.BatchSolver.from_dense(dense, bs, cs, a_storage="f16"))
    refused(lambda: T.BatchSolver.from_dense(dense, bs, cs[:2]))                                 # mismatched lengths
    refused(lambda: T.BatchSolver.from_dense(dense, bs, [cs[0], cs[1], cs[2][:-1]]))
    refused(lambda: T.BatchSolver.from_dense(dense, [bs[0], bs[1][:-1], bs[2]], cs))
    a = np.asarray(dense.mat_a, np.float32).reshape((dense.n, dense.m)).T
    refused(lambda: T.BatchSolver(dense.n, dense.m, sp.csc_matrix(a), bs, cs, dense.seg_type, dense.seg_len))       # a sparse matrix
    refused(lambda: T.BatchSolver(dense.n, dense.m, T.Bf16Matrix.from_f32(dense.mat_a, dense.m, dense.n), bs, cs, dense.seg_type,
                                  dense.seg_len))
    # and the C ABI itself
    D = T.DeviceBuffer
    da, db, dc = D.from_host(dense.mat_a), D.from_host(bs[0]), D.from_host(cs[0])
    st, sl = np.ascontiguousarray(dense.seg_type, np.int32), np.ascontiguousarray(dense.seg_len, np.int64)
    par = _lib.Param(-1, 1e-6, 1e-6, 1e-12, 0, 0, 0)

    def create(n_inst, mat, pb, pc):
        prob = _lib.Problem(dense.n, dense.m, mat, None, None, None, len(st), st.ctypes.data_as(C.POINTER(C.c_int32)),
                            sl.ctypes.data_as(C.POINTER(C.c_int64)))
        h = C.c_void_p()
        lib.thip_batch_create(C.byref(prob), n_inst, pb, pc, C.byref(par), C.byref(h))
        return h

    one_b, one_c = (C.c_void_p * 65)(*[db.ptr] * 65), (C.c_void_p * 65)(*[dc.ptr] * 65)
    for n_inst, mat, pb, pc in ((0, da.ptr, one_b, one_c), (65, da.ptr, one_b, one_c), (2, None, one_b, one_c),
                                (2, da.ptr, None, one_c), (2, da.ptr, one_b, (C.c_void_p * 2)(dc.ptr, None))):
        with pytest.raises(_lib.ThipError) as e:
            create(n_inst, mat, pb, pc)
        assert e.value.code == _lib.E_INVALID
    h = create(2, da.ptr, one_b, one_c)
    for kind in (1, 2):
        with pytest.raises(_lib.ThipError) as e:
            lib.thip_batch_set_a_storage(h, kind)
        assert e.value.code == _lib.E_INVALID
    lib.thip_batch_set_a_storage(h, 0)
    with pytest.raises(_lib.ThipError) as e:
        lib.thip_batch_set_max_group(h, 3)
    assert e.value.code == _lib.E_INVALID
    with pytest.raises(_lib.ThipError) as e:
        lib.thip_batch_run(h, 1, 1, None)                    # not initialised
    assert e.value.code == _lib.E_INVALID
    lib.thip_batch_destroy(h)
    for b in (da, db, dc):
        b.free()
