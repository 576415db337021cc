"""GPU: problems streamed through the slots of a batch (thip_batch_replace / _set_regroup / _run_until_any / _counters;
BatchSolver.replace, regroup=True, stream, totsu_amd.solve_many): a replaced slot is a fresh init bit for bit, the launches follow
the live set and change nothing else, the stream returns every problem's own result.

The box family: A = [I; -I] (4 x 2) over the nonnegative cone.  Every row of A has one nonzero and every column two, so each product
entry is one product or a sum of two terms -- the same float in every summation order and on every kernel instance.  On this family
results are therefore compared with np.array_equal across any grouping."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as O
from problems import benchmark_lp, random_socp

pytestmark = pytest.mark.gpu

TOLS = [2e-5, 2e-5, 1e-4, 2e-3]      # iterates 0, 1, 9, 99 relative to the iterate's max norm (tests/test_gpu_solver.py)
BOX_A = np.vstack([np.eye(2), -np.eye(2)]).astype(np.float32)


@pytest.fixture(scope="module")
def T():
    import totsu_amd
    from totsu_amd import _lib
    _lib.init()
    return totsu_amd


def _mb(T, typ):
    return T.MatBuild(T.F32HIP, typ)


def _instances(dense, B, kind):
    """b_i, c_i of instance i drawn from seed i, as tests/test_gpu_batch.py draws them: the LP generator's own distributions
    (c = -U(0, 1), h = [0; U(0, 1)]); for the cone programs a 1 % perturbation of the template's b and a 10 % one of its c"""
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


# ---- the box family ----------------------------------------------------------------------------------------------------------

def fam(i):
    rng = np.random.default_rng(100 + i)
    c = rng.standard_normal(2)
    c = np.where(np.abs(c) < 0.2, 0.2 * np.sign(c) + (c == 0), c)
    b = -rng.uniform(0.5, 2.0, 4) if i % 4 == 1 else rng.uniform(0.5, 3.0, 4)
    return b.astype(np.float32), c.astype(np.float32)      # feasible: x*_j = -b[2+j] if c_j > 0 else b[j]


def _xstar(b, c):
    return np.array([-b[2 + j] if c[j] > 0 else b[j] for j in range(2)], np.float64)


_BOX_ORACLE = {}


def _box_oracle(i):
    """the f64 oracle on fam(i) at eps_acc = 1e-5: the statuses are confirmed on the CPU before the device is asked"""
    if i not in _BOX_ORACLE:
        b, c = fam(i)
        r = O.solve_matop_cones(O.param(max_iter=100000, eps_acc=1e-5), c, BOX_A, b, [O.CONE_RPOS], [4])
        assert r.status == (O.INFEASIBLE if i % 4 == 1 else O.OK), (i, r.status)
        if i % 4 != 1:
            assert np.abs(r.x - _xstar(b, c)).max() <= 1e-3, (i, r.x)
        _BOX_ORACLE[i] = r
    return _BOX_ORACLE[i]


def _box_param(T):
    p = T.SolverParam()
    p.max_iter, p.eps_acc = 100_000, 1e-5
    return p


def _box_dense():
    from totsu_amd import _lib
    return SimpleNamespace(n=2, m=4, mat_a=np.asfortranarray(BOX_A).ravel(order="F"), seg_type=[_lib.CONE_RPOS], seg_len=[4])


def _box_batch(T, idx, **kw):
    bs, cs = zip(*[fam(i) for i in idx])
    return T.BatchSolver.from_dense(_box_dense(), list(bs), list(cs), _box_param(T), gemv_autotune=False, **kw)


def _want_state(i):
    from totsu_amd import _lib
    return {O.OK: _lib.ST_OK, O.INFEASIBLE: _lib.ST_INFEASIBLE}[_box_oracle(i).status]


@pytest.fixture(scope="module")
def fixed24(T):
    """fam(0 .. 23) in ONE fixed batch (groups of 8 fixed by index, no replace, no regroup): (state, iters, x, y) per problem"""
    for i in range(24):
        _box_oracle(i)
    bt = _box_batch(T, range(24))
    res = bt.run(-1, poll_every=8)
    out = [(r.state, r.iters) + bt.solution(i) for i, r in enumerate(res)]
    bt.destroy()
    for i, (state, iters, x, y) in enumerate(out):
        assert state == _want_state(i), (i, state)
    print("fixed batch of 24: iters", [o[1] for o in out], "oracle", [_box_oracle(i).iters for i in range(24)])
    return out


# ---- 1. replace is a fresh init, bit for bit -----------------------------------------------------------------------------------

def _oracle_snaps(dense, b, c, iters):
    par = O.param(max_iter=max(iters) + 2, eps_acc=1e-30)
    return O.solve_matop_cones(par, c, dense.mat_a, b, dense.seg_type, dense.seg_len, snap_iters=iters, trace_cap=max(iters) + 3,
                               use_ql=True)


def _same_slot(pa, i, pb, j, what):
    for name, (ga, gb) in (("iterate", (pa.iterate(i), pb.iterate(j))), ("precond", (pa.precond(i), pb.precond(j)))):
        assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1], gb[1]), (what, name, i, j)
    assert pa.status(i).iters == pb.status(j).iters, (what, i, j)


@pytest.mark.parametrize("shape,B,k", [("lp40", 3, 20), ("lp1252", 5, 10), ("socp", 3, 20)])
def test_replace_is_a_fresh_init(T, shape, B, k):
    """P = [p0, p1, p2, ..] runs k iterations, takes p_new into slot 1, runs k more; Q = [p0, p_new, p2, ..] runs k; R = P without the
    replace runs 2 k.  Slot 1 of P is slot 1 of Q and the other slots of P are R's, bitwise: iterate, preconditioner, iteration count.
    lp40 (NV = 4 with a spare slot) also against the f64 oracle for p_new; lp1252: m = 2504, padded copy, several tiles and chunks,
    NV = 8; socp: the block cones' group minima."""
    dense = _lp_dense(T, 40) if shape == "lp40" else _lp_dense(T, 1252) if shape == "lp1252" else _socp_dense(T)
    bs, cs = _instances(dense, B + 1, "lp" if shape.startswith("lp") else "cone")
    nb, nc = bs[B], cs[B]                                    # p_new: the draw after the batch's own
    bs, cs = bs[:B], cs[:B]
    p = T.SolverParam()
    p.eps_acc = 1e-30
    da = T.DeviceBuffer.from_host(dense.mat_a)               # one upload of A for the three batches
    mk = lambda vb, vc: T.BatchSolver(dense.n, dense.m, da, vb, vc, dense.seg_type, dense.seg_len, p, gemv_autotune=False)
    P, R = mk(bs, cs), mk(bs, cs)
    Q = mk([bs[0], nb] + bs[2:], [cs[0], nc] + cs[2:])
    P.run(k, poll_every=64)
    P.replace(1, nb, nc)
    assert P.status(1).iters == 0 and P.counters()["replaced"] == 1
    _same_slot(P, 1, Q, 1, "after replace: the start iterate and the preconditioner")
    N = dense.n + 2 * dense.m + 1
    oracle_iters = [0, 1, 9, 99] if shape == "lp40" else []
    ro = _oracle_snaps(dense, nb, nc, oracle_iters) if oracle_iters else None

    def against_oracle(q):
        x, y = P.iterate(1)
        rx, ry = ro.snaps[q][:N], ro.snaps[q][N:]
        sx, sy = max(np.abs(rx).max(), 1e-6), max(np.abs(ry).max(), 1e-6)
        print("replaced slot, iterate %d: err x %.2e y %.2e (tol %.0e)" % (oracle_iters[q], np.abs(x - rx).max() / sx,
                                                                          np.abs(y - ry).max() / sy, TOLS[q]))
        assert np.abs(x - rx).max() <= TOLS[q] * sx and np.abs(y - ry).max() <= TOLS[q] * sy, (q, oracle_iters[q])

    done = 0
    for q, it in enumerate(oracle_iters[:3]):                # iterates 0, 1, 9 of p_new lie inside the k iterations
        P.run(it + 1 - done, poll_every=64)
        done = it + 1
        against_oracle(q)
    P.run(k - done, poll_every=64)
    Q.run(k, poll_every=64)
    R.run(2 * k, poll_every=64)
    assert P.status(1).iters == k and Q.status(1).iters == k
    _same_slot(P, 1, Q, 1, "k iterations after the replace")
    for i in [0] + list(range(2, B)):
        assert R.status(i).iters == 2 * k
        _same_slot(P, i, R, i, "a slot beside the replaced one")
    if oracle_iters:
        P.run(100 - k, poll_every=64)
        against_oracle(3)
    assert P.counters()["instance_iterations"] == sum(P.status(i).iters for i in range(B)) + k      # + the retired occupant's
    for bt in (P, Q, R):
        bt.destroy()
    da.free()


# ---- 2. replacing a stopped slot -----------------------------------------------------------------------------------------------

def _run_out(bt, on_poll=None):
    """run(8, poll_every=8) until every instance has stopped; the last statuses"""
    from totsu_amd import _lib
    for _ in range(100_000 // 8):
        res = bt.run(8, poll_every=8)
        if on_poll:
            on_poll(res)
        if all(r.state != _lib.ST_RUNNING for r in res):
            return res
    raise AssertionError("still running after 100 000 iterations")


def test_replace_a_stopped_slot(T, fixed24):
    from totsu_amd import _lib
    for i in range(4):
        _box_oracle(i)
    ref = _box_batch(T, range(3))                            # never replaced
    ref_res = _run_out(ref)
    ref_sol = [ref.solution(i) for i in range(3)]
    bt = _box_batch(T, range(3))
    for _ in range(100_000 // 8):
        res = bt.run(8, poll_every=8)
        if res[1].state != _lib.ST_RUNNING:
            break
    assert res[1].state == _lib.ST_INFEASIBLE
    stopped_at = res[1].iters
    bt.replace(1, *fam(3))
    assert bt.status(1).state == _lib.ST_RUNNING and bt.status(1).iters == 0
    res = _run_out(bt)
    b3, c3 = fam(3)
    x1, y1 = bt.solution(1)
    print("slot 1: fam(1) INFEASIBLE after %d, then fam(3): state %d after %d iterations (oracle %d)"
          % (stopped_at, res[1].state, res[1].iters, _box_oracle(3).iters))
    assert res[1].state == _lib.ST_OK and np.abs(x1 - _xstar(b3, c3)).max() <= 1e-3, (res[1].state, x1)
    # its iterations count from 0: what fam(3) takes in a batch it was in from the start, and the same floats
    assert res[1].iters == fixed24[3][1]
    assert np.array_equal(x1, fixed24[3][2]) and np.array_equal(y1, fixed24[3][3])
    for i in (0, 2):
        assert (res[i].state, res[i].iters) == (ref_res[i].state, ref_res[i].iters), i
        x, y = bt.solution(i)
        assert np.array_equal(x, ref_sol[i][0]) and np.array_equal(y, ref_sol[i][1]), i
    c = bt.counters()
    assert c["replaced"] == 1 and c["instance_iterations"] == stopped_at + sum(r.iters for r in res)
    bt.destroy()
    ref.destroy()


# ---- 3. regrouping follows the live set, and changes nothing else ------------------------------------------------------------------

@pytest.mark.parametrize("max_group", [8, 4])
def test_regroup_follows_the_live_set(T, max_group):
    from totsu_amd import _lib
    from totsu_amd.batch import group_sizes, kernel_instance, live_groups
    B = 11
    for i in range(B):
        _box_oracle(i)
    fixed = []
    for size in group_sizes(B, max_group):
        fixed.append(list(range(sum(len(g) for g in fixed), sum(len(g) for g in fixed) + size)))
    finals = {}
    for regroup in (False, True):
        bt = _box_batch(T, range(B), max_group=max_group, regroup=regroup)
        live = [True] * B
        want = {1: 0, 2: 0, 4: 0, 8: 0}
        frozen, live_counts = {}, []
        assert bt.counters()["launches"] == want and bt.counters()["live"] == B
        for _ in range(100_000 // 8):
            if not any(live):
                break
            # what this call must issue, from the statuses held: two passes x 8 iterations per group
            groups = live_groups(live, max_group) if regroup else [g for g in fixed if any(live[i] for i in g)]
            for g in groups:
                want[kernel_instance(len(g))] += 2 * 8
            live_counts.append(sum(live))
            res = bt.run(8, poll_every=8)
            live = [r.state == _lib.ST_RUNNING for r in res]
            c = bt.counters()
            assert c["launches"] == want and c["passes"] == sum(want.values()) and c["live"] == sum(live), (regroup, c, want)
            assert c["groups_now"] == len(live_groups(live, max_group) if regroup else [g for g in fixed if any(live[i] for i in g)])
            for i, r in enumerate(res):
                if not live[i] and i not in frozen:
                    frozen[i] = (r.iters, bt.iterate(i))
        assert not any(live)
        for i in range(B):
            st = bt.status(i)
            assert st.state == _want_state(i), (i, st.state)
            x, y = bt.iterate(i)                             # a stopped instance's iterate does not change afterwards
            assert st.iters == frozen[i][0] and np.array_equal(x, frozen[i][1][0]) and np.array_equal(y, frozen[i][1][1]), i
        print("max_group %d regroup %s: live per call %s, launches %s, passes %d" % (max_group, regroup, live_counts, want, sum(want.values())))
        finals[regroup] = ([bt.status(i).iters for i in range(B)], [bt.solution(i) for i in range(B)], dict(want), live_counts)
        bt.destroy()
    off, on = finals[False], finals[True]
    assert on[0] == off[0], (on[0], off[0])
    for i in range(B):
        assert np.array_equal(on[1][i][0], off[1][i][0]) and np.array_equal(on[1][i][1], off[1][i][1]), i
    assert sum(on[2].values()) < sum(off[2].values())
    if max_group == 8:
        assert 9 in on[3] and on[2][1] > 0                   # live = 9: a group of 8 and the single-vector kernel


# ---- 4. the stream -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_group", [2, 4, 8])
def test_solve_many_box_family(T, fixed24, max_group):
    from totsu_amd import _lib
    probs = [fam(i) for i in range(24)]
    out = T.solve_many(_box_dense(), [b for b, _ in probs], [c for _, c in probs], slots=4, param=_box_param(T), poll_every=8,
                       max_group=max_group, gemv_autotune=False)
    assert len(out) == 24
    for i, (r, x, y) in enumerate(out):                      # input order: problem i's own result at position i
        assert r.state == (_lib.ST_INFEASIBLE if i % 4 == 1 else _lib.ST_OK), (i, r.state)
        if i % 4 != 1:
            assert np.abs(x - _xstar(*probs[i])).max() <= 1e-3, (i, x)
        # bitwise what the same problem gives in one fixed batch of all 24: nothing of a slot's previous occupant is left
        assert r.iters == fixed24[i][1], (i, r.iters, fixed24[i][1])
        assert np.array_equal(x, fixed24[i][2]) and np.array_equal(y, fixed24[i][3]), i
    assert out.counters["replaced"] == 20
    assert out.counters["instance_iterations"] == sum(r.iters for r, _, _ in out)
    assert out.counters["live"] == 0
    print("max_group %d: %s" % (max_group, out.counters))


def test_solve_many_generic_lp(T):
    """a generic A: each streamed problem against its own FusedSolver(.., "carried").  Iteration counts are printed, not asserted:
    the kernel instance that serves a problem changes with the live set."""
    dense = _lp_dense(T, 40)
    bs, cs = _instances(dense, 10, "lp")
    p = T.SolverParam()
    p.max_iter, p.eps_acc = 100_000, 1e-4
    out = T.solve_many(dense, bs, cs, slots=3, param=p)
    assert len(out) == 10 and out.counters["replaced"] == 7
    da = T.DeviceBuffer.from_host(dense.mat_a)
    for i, (r, x, y) in enumerate(out):
        fs = T.FusedSolver(dense.n, dense.m, da, bs[i], cs[i], dense.seg_type, dense.seg_len, p, "carried")
        fr = fs.run()
        fx, fy = fs.solution()
        fs.destroy()
        print("problem %d: state %d after %d iterations (FusedSolver carried: %d)" % (i, r.state, r.iters, fr.iters))
        assert (r.state, r.kind) == (fr.state, fr.kind), (i, r.state, fr.state)
        assert np.allclose(x, fx, atol=1e-3) and np.allclose(y, fy, atol=1e-3), i
    da.free()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------

def test_stream_refusals(T):
    from totsu_amd import _lib
    from totsu_amd._lib import lib
    dense = _lp_dense(T, 40)
    bs, cs = _instances(dense, 4, "lp")
    bad = (ValueError, _lib.ThipError)

    def refused(fn):
        with pytest.raises(bad) as e:
            fn()
        assert not isinstance(e.value, _lib.ThipError) or e.value.code == _lib.E_INVALID

    p = T.SolverParam()
    p.eps_acc = 1e-30
    bt = T.BatchSolver.from_dense(dense, bs[:3], cs[:3], p, gemv_autotune=False)
    ref = T.BatchSolver.from_dense(dense, bs[:3], cs[:3], p, gemv_autotune=False)
    bt.run(3, poll_every=3)
    refused(lambda: bt.replace(3, bs[3], cs[3]))                                   # no such slot
    refused(lambda: bt.replace(-1, bs[3], cs[3]))
    refused(lambda: bt.replace(1, None, cs[3]))                                    # null vectors
    refused(lambda: bt.replace(1, bs[3], None))
    refused(lambda: bt.replace(1, bs[3][:-1], cs[3]))                              # wrong lengths
    refused(lambda: bt.replace(1, bs[3], np.concatenate([cs[3], cs[3]])))
    refused(lambda: bt.replace(1, T.DeviceBuffer(dense.m - 1), cs[3]))
    D = T.DeviceBuffer
    db, dc = D.from_host(bs[3]), D.from_host(cs[3])
    for args in ((bt.h, 3, db.ptr, dc.ptr), (bt.h, -1, db.ptr, dc.ptr), (bt.h, 1, None, dc.ptr), (bt.h, 1, db.ptr, None),
                 (None, 1, db.ptr, dc.ptr)):
        with pytest.raises(_lib.ThipError) as e:
            lib.thip_batch_replace(*args)
        assert e.value.code == _lib.E_INVALID
    with pytest.raises(_lib.ThipError) as e:
        lib.thip_batch_set_regroup(bt.h, 1)                                        # after init
    assert e.value.code == _lib.E_INVALID
    with pytest.raises(_lib.ThipError) as e:
        lib.thip_batch_counters(bt.h, None)
    assert e.value.code == _lib.E_INVALID
    # after the refused calls the batch still runs, and is what it would have been without them
    bt.run(4, poll_every=4)
    ref.run(7, poll_every=7)
    assert bt.counters()["replaced"] == 0
    for i in range(3):
        assert bt.status(i).iters == 7
        (x, y), (rx, ry) = bt.iterate(i), ref.iterate(i)
        assert np.array_equal(x, rx) and np.array_equal(y, ry), i
    bt.destroy()
    ref.destroy()
    # a batch that is not initialised
    da = D.from_host(dense.mat_a)
    st, sl = np.ascontiguousarray(dense.seg_type, np.int32), np.ascontiguousarray(dense.seg_len, np.int64)
    par = _lib.Param(-1, 1e-6, 1e-6, 1e-12, 0, 0, 0)
    prob = _lib.Problem(dense.n, dense.m, da.ptr, None, None, None, len(st), st.ctypes.data_as(C.POINTER(C.c_int32)),
                        sl.ctypes.data_as(C.POINTER(C.c_int64)))
    h = C.c_void_p()
    lib.thip_batch_create(C.byref(prob), 2, (C.c_void_p * 2)(db.ptr, db.ptr), (C.c_void_p * 2)(dc.ptr, dc.ptr), C.byref(par), C.byref(h))
    for call in (lambda: lib.thip_batch_replace(h, 0, db.ptr, dc.ptr), lambda: lib.thip_batch_run_until_any(h, 1, 1, None)):
        with pytest.raises(_lib.ThipError) as e:
            call()
        assert e.value.code == _lib.E_INVALID
    lib.thip_batch_set_regroup(h, 1)                                               # before init: taken
    lib.thip_batch_init(h)
    stt = (_lib.Status * 2)()
    lib.thip_batch_run_until_any(h, 2, 1, stt)
    assert [s.iter for s in stt] == [2, 2]
    lib.thip_batch_destroy(h)
    for b in (da, db, dc):
        b.free()
    # solve_many
    refused(lambda: T.solve_many(dense, bs, cs, slots=0))
    refused(lambda: T.solve_many(dense, bs, cs, slots=65))
    refused(lambda: T.solve_many(dense, [], []))
