"""GPU: sparse problems of different shapes, cone layouts and patterns in ONE batch (totsu_amd.RaggedSparseBatchSolver /
thip_raggedsparse_*).  The yardstick is bitwise: a problem of the batch must hold -- preconditioner, iterates, status -- what a
SparseBatchSolver holds that was given this problem alone at the same workgroup size: at every workgroup size, for both state
arithmetics, whatever its index, its neighbours, its class's live list, the launch cuts, and whether its blob is resident.
SparseBatchSolver is itself tested against the f64 oracle on these constructions (tests/test_gpu_sparsebatch.py); the same batch is
held to the oracle here too, each problem at its family's iterates and tolerances.  Then the exact products against the dense
ragged batch, independent termination with the launch counters of both classes, the tau -> 0 verdicts, replace and the refusals.

The set is tests/raggedsparse_cases.py's; the uniform family's runs are computed once per (workgroup size, state arithmetic)."""
import ctypes as C

import numpy as np
import pytest

import raggedsparse_cases as RC
import tau_zero_problems as Z
from ownbatch_cases import F, T, _D, _dense_of, _same, _snap, _term_problem  # noqa: F401
from sparse_cases import RPOS, csc_of, identity_problem, masked, problem_of, sparse_problem

pytestmark = pytest.mark.gpu

STEPS = (1, 2, 10, 50)                       # the iteration counts of the bitwise comparisons
_REFS = {}


def _param(T, arith=None, **kw):
    p = T.SolverParam()
    p.eps_acc = 1e-30
    if arith:
        p.state_arith = arith
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _nnz(d):
    return int(csc_of(d)[0][-1])


def _alone(T, d, p, force=None, **kw):
    """the uniform family holding d alone"""
    if force is not None:
        kw["force_threads"] = force
    return T.SparseBatchSolver.from_dense([d], p, **kw)


def _full(sb, i):
    return _snap(sb, i) + sb.precond(i)


def _same_full(g, w, what=None):
    assert g[2] == w[2], (what, g[2], w[2])
    for u, v in zip(g[:2] + g[3:], w[:2] + w[3:]):
        assert u.shape == v.shape and np.array_equal(u, v), what


def _walk(sb, idx, steps=STEPS, poll=64):
    """{iteration count: [what problem i holds then, for i in idx]}"""
    out, done = {}, 0
    for s in steps:
        sb.run(s - done, poll_every=poll)
        done = s
        out[s] = [_full(sb, i) for i in idx]
    return out


def _ref(T, force=None, arith=None):
    """per problem of the set: {iteration count: what a SparseBatchSolver holds for it alone}; computed once"""
    key = (force, arith)
    if key not in _REFS:
        out = []
        for d in RC.problems(T):
            sb = _alone(T, d, _param(T, arith), force)
            out.append({s: v[0] for s, v in _walk(sb, [0]).items()})
            sb.destroy()
        _REFS[key] = out
    return _REFS[key]


def _kw(force=None, resident=None):
    kw = {}
    if force is not None:
        kw["force_threads"] = force
    if resident is not None:
        kw["force_resident"] = resident
    return kw


# ---- 1. bit for bit the uniform family, problem by problem -----------------------------------------------------------------------

def test_the_shapes_the_cpu_tests_plan_are_the_real_ones(T):
    for d, s in zip(RC.problems(T), RC.shapes()):
        assert (d.n, d.m, list(d.seg_type), list(d.seg_len), _nnz(d)) == (s.n, s.m, s.seg_type, s.seg_len, s.nnz)


@pytest.mark.parametrize("arith", [None, "plain"])
@pytest.mark.parametrize("force", [None, 256, 1024])
def test_every_problem_has_the_uniform_family_s_bits(T, force, arith):
    from totsu_amd import raggedsparse as RS
    from totsu_amd import sparsebatch as SB
    ds, want = RC.problems(T), _ref(T, force, arith)
    nnz = [_nnz(d) for d in ds]
    plan = RC.restate(ds, nnz, None, force)
    sp = [RS.SparseProblem.of_dense(d) for d in ds]
    RC.check_plan(RS.plan(sp, **_kw(force)), plan)
    rs = T.RaggedSparseBatchSolver.from_dense(ds, _param(T, arith), **_kw(force))
    try:
        assert rs.shapes == [(d.n, d.m) for d in ds] and rs.nnz_caps == nnz
        info = rs.info()
        for got, w in zip(info["classes"], plan["info"]["classes"]):
            assert (got["n_prob"], got["threads"], got["lds_bytes"], got["n_resident"]) == (w["n_prob"], w["threads"], w["lds_bytes"],
                                                                                           w["n_resident"])
        if force is None:
            assert [c["n_prob"] for c in info["classes"]] == [17, 2]
        assert info["n_resident"] == sum(plan["resident"]) == len(ds) - 3
        assert info["blob_bytes"] == sum(SB.capacity_bytes(d.n, d.m, k) for d, k in zip(ds, nnz))
        assert info["arena_bytes"] == 4 * sum(6 * d.n + 10 * d.m for d in ds)
        # (1 x 1 and 1 x 300 share the one-row table, 300 x 1 and 300 x 200 the table of 300 nonnegative rows)
        assert info["n_layouts"] == plan["info"]["n_layouts"] == len(ds) - 2
        assert info["n_prob"] == info["live"] == len(ds) and info["nnz_total"] == sum(nnz)
        assert info["a_bytes_per_iter"] > 0 and info["max_psd_order"] == 33 and info["n_psd"] == 12
        for s, got in _walk(rs, range(len(ds))).items():
            for j, g in enumerate(got):
                assert g[2][1] == s
                _same_full(g, want[j][s], (RC.SET[j], s, force, arith))
    finally:
        rs.destroy()


# ---- 2. independence: index, neighbours, the class's live list, the launch cuts ----------------------------------------------------

@pytest.mark.parametrize("how,poll", [("permuted", 7), ("cycled", 64), ("as is", 1)])
def test_a_problem_does_not_depend_on_the_batch_around_it(T, how, poll):
    ds, want = RC.problems(T), _ref(T)
    if how == "permuted":
        order = [int(j) for j in np.random.default_rng(5).permutation(len(ds))]
    elif how == "cycled":
        order = [q % len(ds) for q in range(300)]                 # more workgroups than the device has CUs
    else:
        order = list(range(len(ds)))
    rs = T.RaggedSparseBatchSolver.from_dense([ds[j] for j in order], _param(T))
    try:
        rs.run(STEPS[-1], poll_every=poll)
        cuts = -(-STEPS[-1] // poll)
        info = rs.info()
        assert [c["launches"] for c in info["classes"]] == [cuts, cuts] and info["launches"] == 2 * cuts
        assert info["workgroups"] == cuts * len(order) and info["n_layouts"] == len(ds) - 2
        for q, j in enumerate(order):
            _same_full(_full(rs, q), want[j][STEPS[-1]], (how, q, RC.SET[j]))
    finally:
        rs.destroy()


# ---- 3. residency changes no bit ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("resident", [0, 1])
def test_residency_changes_no_bit(T, resident):
    ds, want = RC.problems(T), _ref(T)
    rs = T.RaggedSparseBatchSolver.from_dense(ds, _param(T), force_resident=resident)
    try:
        info = rs.info()
        assert info["n_resident"] == (len(ds) - 3 if resident else 0)
        nnz = [_nnz(d) for d in ds]
        plan = RC.restate(ds, nnz, None, None, resident)
        assert [c["lds_bytes"] for c in info["classes"]] == [c["lds_bytes"] for c in plan["info"]["classes"]]
        if not resident:                                          # every class shrinks to its members' vectors, every blob is streamed
            assert info["classes"][0]["lds_bytes"] == max(RC.vector_bytes(d) for d, c in zip(ds, plan["cls"]) if c == 0)
            assert info["a_bytes_per_iter"] >= 8 * sum(4 * k + d.m + d.n + 4 for d, k in zip(ds, nnz))
        got = _walk(rs, range(len(ds)))
        for s in STEPS:
            for j, g in enumerate(got[s]):
                _same_full(g, want[j][s], (RC.SET[j], s, resident))
    finally:
        rs.destroy()


# ---- 4. against the f64 oracle ----------------------------------------------------------------------------------------------------

def test_the_set_against_the_oracle(T):
    """the comparison of ownbatch_cases.check_against_oracle, each problem with its own lengths, iterates and tolerances"""
    runs = [r for r in (RC.oracle_run(T, j) for j in range(len(RC.SET))) if r is not None]
    assert len(runs) == len(RC.SET) - 1
    rs = T.RaggedSparseBatchSolver.from_dense([r[0] for r in runs], _param(T))
    try:
        for i, (d, ro, _, _) in enumerate(runs):
            N = d.n + 2 * d.m + 1
            t, s = rs.precond(i)
            assert t.size == N and s.size == d.n + d.m + 1
            et, es = np.abs(t / ro.precond[:N] - 1).max(), np.abs(s / ro.precond[N:] - 1).max()
            print("ragged sparse problem %d preconditioner: rel err tau %.2e sigma %.2e" % (i, et, es))
            assert np.allclose(t, ro.precond[:N], rtol=2e-5, atol=0), (i, et)
            assert np.allclose(s, ro.precond[N:], rtol=2e-5, atol=0), (i, es)
        done = 0
        for it in sorted(set(v for r in runs for v in r[2])):
            rs.run(it + 1 - done, poll_every=64)
            done = it + 1
            for i, (d, ro, iters, tols) in enumerate(runs):
                if it not in iters:
                    continue
                q = list(iters).index(it)
                tol = tols[q]
                N = d.n + 2 * d.m + 1
                x, y = rs.iterate(i)
                rx, ry = ro.snaps[q][:N], ro.snaps[q][N:]
                sx, sy = max(np.abs(rx).max(), 1e-6), max(np.abs(ry).max(), 1e-6)
                ex, ey = np.abs(x - rx).max() / sx, np.abs(y - ry).max() / sy
                print("ragged sparse problem %d (%d x %d) iterate %d: err x %.2e y %.2e (tol %.0e)" % (i, d.m, d.n, it, ex, ey, tol))
                assert ex <= tol and ey <= tol, (i, it, ex, ey)
                st = rs.status(i)
                assert st.state == -1 and st.iters == it + 1
                tr = ro.trace[it]
                assert st.kind == tr[1]
                assert np.allclose(st.cri, tr[2:], rtol=max(50 * tol, 1e-3), atol=1e-5), (i, it, st.cri, tr)
    finally:
        rs.destroy()


# ---- 5. exact products: the dense ragged batch's bits -------------------------------------------------------------------------------

def test_identity_rows_give_the_dense_ragged_batch_s_bits(T):
    """A = [I; -I] at n = 17, 40, 64 in one batch: every product of either pass is exact and every sum is at most one rounding of two
    exact terms plus zeros, so the sparse pass and the dense pass give the same h and g, and the shared iteration the same iterates
    (both batches run these three at 256 threads)"""
    ds = [identity_problem(k, n) for k, n in enumerate((17, 40, 64))]
    assert all(_nnz(d) == 2 * d.n and d.m * d.n <= 8192 for d in ds)
    p = _param(T)
    sp, dn = T.RaggedSparseBatchSolver.from_dense(ds, p), T.RaggedBatchSolver.from_dense(ds, p)
    try:
        assert [c["n_prob"] for c in sp.info()["classes"]] == [c["n_prob"] for c in dn.info()["classes"]] == [3, 0]
        a, b = _walk(sp, range(3), steps=(1, 10, 50)), _walk(dn, range(3), steps=(1, 10, 50))
        for s in a:
            for i in range(3):
                _same_full(a[s][i], b[s][i], (s, i))
    finally:
        sp.destroy()
        dn.destroy()


# ---- 6. independent termination ---------------------------------------------------------------------------------------------------

def test_independent_termination_and_the_launch_counters(T):
    from totsu_amd import _lib
    from totsu_amd import raggedsparse as RS
    POLL = 8
    ds = [_term_problem(i) for i in range(6)] + [RC.host_problem(j) for j in (0, 5, 9, 12, 13)] + [_term_problem(i) for i in range(6, 9)]
    nnz = [_nnz(d) for d in ds]
    plan = RS.plan([RS.SparseProblem.of_dense(d) for d in ds])
    cls = plan["cls"]
    assert cls == [0] * 7 + [1] + [0] * 6                              # lp1000x700 alone in the 1024-thread class
    for c in (0, 1):                                                   # the live order is by entry count, ties by index
        assert plan["order"][c] == sorted((q for q in range(len(ds)) if cls[q] == c), key=lambda q: (-nnz[q], q))
    assert plan["order"][0][:2] == [6, 10]
    p = _param(T, eps_acc=1e-5, eps_inf=1e-5, max_iter=600)
    want = []
    for d in ds:
        sb = _alone(T, d, p)
        r = sb.run(-1, poll_every=POLL)[0]
        want.append((r.state, r.iters, r.kind, tuple(r.cri)) + sb.solution(0) + sb.iterate(0))
        sb.destroy()
    assert {w[0] for w in want[:6]} == {_lib.ST_OK, _lib.ST_INFEASIBLE, _lib.ST_UNBOUNDED} and len(set(w[1] for w in want)) >= 4, [w[:2] for w in want]
    rs = T.RaggedSparseBatchSolver.from_dense(ds, p)
    try:
        live = [cls.count(k) for k in (0, 1)]
        launches, groups, calls, stopped, seen = [0, 0], [0, 0], 0, set(), {}
        while sum(live):
            res = rs.run_until_any(-1, poll_every=POLL)
            calls += 1
            info = rs.info()
            now = [c["live"] for c in info["classes"]]
            polls = [c["launches"] - l for c, l in zip(info["classes"], launches)]
            # one launch per class with a live member per poll, as many workgroups as it had live members; a class without one: none
            running = [k for k in (0, 1) if live[k]]
            assert len(set(polls[k] for k in running)) == 1 and polls[running[0]] >= 1, (polls, live)
            for k in (0, 1):
                assert polls[k] == (polls[running[0]] if live[k] else 0), (k, polls, live)
                assert info["classes"][k]["workgroups"] - groups[k] == polls[k] * live[k]
            new = {i for i, r in enumerate(res) if r.state != _lib.ST_RUNNING} - stopped
            assert new and sum(now) == sum(live) - len(new), (new, now, live)
            for i in new:
                seen[i] = _full(rs, i)
            for i in stopped:                                          # a stopped slot's bits do not move
                _same_full(_full(rs, i), seen[i], i)
            stopped |= new
            launches, groups, live = [c["launches"] for c in info["classes"]], [c["workgroups"] for c in info["classes"]], now
            assert info["live"] == sum(now) and calls <= len(ds)
        assert info["launches"] == sum(launches) and info["workgroups"] == sum(groups) and calls >= 4
        print("ragged sparse termination: iterations", [r.iters for r in res], "launches per class", launches)
        for i, w in enumerate(want):
            st = rs.status(i)
            assert (st.state, st.iters, st.kind, tuple(st.cri)) == w[:4], (i, st.iters, w[1])
            for u, v in zip(rs.solution(i) + rs.iterate(i), w[4:]):
                assert u.shape == v.shape and np.array_equal(u, v), i
    finally:
        rs.destroy()


# ---- 7. tau -> 0: each member's own verdict -----------------------------------------------------------------------------------------

def test_verdicts_among_feasible_problems_of_other_shapes(T):
    fams = [Z.family("F1"), Z.family("F2"), Z.family("F3"), Z.family("F4"), Z.family("F5")] + Z.family("F6")
    feas = [RC.host_problem(0), RC.problems(T)[14], RC.host_problem(3), RC.host_problem(9)]      # lp40x30, part22, mixed145x40, 1 x 1
    ds, verdict = [], []
    for k, f in enumerate(fams):                                   # F, feasible, F, feasible, ...
        ds.append(_dense_of(f))
        verdict.append(f.verdict)
        if k < len(feas):
            ds.append(feas[k])
            verdict.append(None)
    assert {Z.INFEASIBLE, Z.UNBOUNDED} <= set(verdict)
    p = _param(T, max_iter=3 * Z.MAX_VERDICT_ITER, eps_acc=Z.EPS, eps_inf=Z.EPS)
    rs = T.RaggedSparseBatchSolver.from_dense(ds, p)
    try:
        res = rs.run(-1, poll_every=25)
        for i, (d, v) in enumerate(zip(ds, verdict)):
            sb = _alone(T, d, p)
            w = sb.run(-1, poll_every=25)[0]
            print("ragged sparse tau_zero problem %d (%d x %d): state %d at %d kind %d (alone: %d at %d)"
                  % (i, d.m, d.n, res[i].state, res[i].iters, res[i].kind, w.state, w.iters))
            if v is not None:
                assert w.state == v, (i, w.state, v)               # (the uniform family's verdict is the family's)
            assert (res[i].state, res[i].iters, res[i].kind, res[i].cri, res[i].tau) == (w.state, w.iters, w.kind, w.cri, w.tau), i
            if v in (Z.INFEASIBLE, Z.UNBOUNDED):
                assert res[i].kind == 1 and res[i].tau == 0.0
            for u, z in zip(rs.iterate(i) + rs.solution(i), sb.iterate(0) + sb.solution(0)):
                assert np.array_equal(u, z), i
            sb.destroy()
    finally:
        rs.destroy()


# ---- 8. replace -------------------------------------------------------------------------------------------------------------------

def test_replace_is_a_fresh_init_of_that_slot_alone(T):
    from totsu_amd import _lib
    from totsu_amd._lib import lib
    held = [RC.host_problem(3), sparse_problem("lp40x30", 1), RC.problems(T)[14], RC.host_problem(0)]
    cap = _nnz(held[1])
    rng = np.random.default_rng(77)
    fewer = problem_of(masked(40, 30, 0.04, rng), [RPOS], [40], rng)                  # another pattern, fewer entries
    A = np.zeros(1200)
    A[rng.choice(1200, cap, replace=False)] = rng.standard_normal(cap)
    exact = problem_of(A.reshape(40, 30), [RPOS], [40], rng)                          # exactly cap entries
    A[np.nonzero(A == 0)[0][0]] = 1.0
    over = problem_of(A.reshape(40, 30), [RPOS], [40], rng)                           # one entry too many
    assert 0 < _nnz(fewer) < cap == _nnz(exact) == _nnz(over) - 1
    p = _param(T)

    def fresh(d, steps):
        """what a fresh batch of d alone holds at init and after each of steps"""
        sb = T.RaggedSparseBatchSolver.from_dense([d], p)
        out = [_full(sb, 0)] + [v[0] for v in _walk(sb, [0], steps=steps).values()]
        sb.destroy()
        return out

    def others(total):
        sb = T.RaggedSparseBatchSolver.from_dense(held, p)
        sb.run(total, poll_every=64)
        out = [_full(sb, i) for i in range(4)]
        sb.destroy()
        return out

    rs = T.RaggedSparseBatchSolver.from_dense(held, p)
    try:
        assert rs.nnz_caps[1] == cap
        rs.run(5, poll_every=4)
        done = 5
        for new in (fewer, exact):
            want = fresh(new, (1, 2, 10))
            rs.replace(1, csc_of(new), new.vec_b, new.vec_c)
            st, info = rs.status(1), rs.info()
            assert (st.state, st.iters) == (_lib.ST_RUNNING, 0) and info["live"] == 4
            assert info["nnz_total"] == sum(_nnz(d) for d in held) - cap + _nnz(new)
            _same_full(_full(rs, 1), want[0], "fresh")
            for k, got in enumerate(_walk(rs, [1], steps=(1, 2, 10)).values()):
                _same_full(got[0], want[k + 1], k)
            done += 10
            untouched = others(done)
            for i in (0, 2, 3):                                        # the neighbours went on as if nothing had happened
                _same_full(_full(rs, i), untouched[i], i)
        # refusals: one entry too many, arrays of another length -- the slot is left as it was
        before = _full(rs, 1)
        with pytest.raises(ValueError, match="%d entries where nnz_cap is %d" % (cap + 1, cap)):
            rs.replace(1, csc_of(over), over.vec_b, over.vec_c)
        cp, ri, va = csc_of(over)
        with pytest.raises(_lib.ThipError, match="%d entries where nnz_cap is %d" % (cap + 1, cap)) as e:      # and the library itself
            db, dc = T.DeviceBuffer.from_host(over.vec_b), T.DeviceBuffer.from_host(over.vec_c)
            try:
                lib.thip_raggedsparse_replace(rs.h, 1, cp.ctypes.data_as(C.POINTER(C.c_int64)), ri.ctypes.data_as(C.POINTER(C.c_int32)),
                                              va.ctypes.data_as(C.POINTER(C.c_float)), db.ptr, dc.ptr, None)
            finally:
                db.free()
                dc.free()
        assert e.value.code == _lib.E_INVALID
        other = held[0]
        for args in ((csc_of(other), exact.vec_b, exact.vec_c), (csc_of(exact), exact.vec_b[:-1], exact.vec_c),
                     (csc_of(exact), exact.vec_b, other.vec_c)):
            with pytest.raises(ValueError):
                rs.replace(1, *args)
        with pytest.raises(ValueError):
            rs.replace(4, csc_of(exact), exact.vec_b, exact.vec_c)
        _same_full(_full(rs, 1), before, "refused")
        assert rs.info()["live"] == 4
        rs.run(5, poll_every=64)                                       # ... and runs on as the problem it held
        want = fresh(exact, (15,))
        _same_full(_full(rs, 1), want[1], "after the refusals")
    finally:
        rs.destroy()


# ---- 9. refusals leave nothing allocated --------------------------------------------------------------------------------------------

def test_refusals_leave_nothing_allocated(T):
    from totsu_amd import raggedsparse as RS
    S = T.RaggedSparseBatchSolver
    host = [RC.host_problem(j) for j in (0, 3, 7, 9)]
    keep = S.from_dense(host[:3])
    info = keep.info()
    before = info["device_bytes_all"]
    assert before == info["device_bytes"] > info["arena_bytes"] + info["blob_bytes"] > 0

    def sp():
        return [RS.SparseProblem.of_dense(d) for d in host]

    z = np.zeros
    bad = RS.SparseProblem(3, 2145, (z(4, np.int64), [], []), z(2145, F), z(3, F), [4], [2145])          # order 65
    with pytest.raises(ValueError, match="problem 2: .*above 64"):
        S(sp()[:2] + [bad] + sp()[2:])
    ps = sp()
    cp, ri, va = (np.array(v) for v in ps[1].mat)
    assert cp[1] >= 2
    ri[[0, 1]] = ri[[1, 0]]                                                             # an unsorted column
    ps[1].mat = (cp, ri, va)
    with pytest.raises(ValueError, match="problem 1: the row indices of a column are not strictly ascending"):
        S(ps)
    ps = sp()
    cp, ri, va = (np.array(v) for v in ps[2].mat)
    va[5] = np.inf
    ps[2].mat = (cp, ri, va)
    with pytest.raises(ValueError, match="problem 2: a value of A is not finite"):
        S(ps)
    with pytest.raises(ValueError, match="nnz_caps holds 3 entries where 4 problems"):
        S(sp(), nnz_caps=[0, 0, 0])
    with pytest.raises(ValueError, match="problem 3: .*nnz_cap 2 exceeds m n = 1"):
        S(sp(), nnz_caps=[0, 0, 0, 2])
    with pytest.raises(ValueError, match="256 or 1024"):
        S(sp(), force_threads=512)
    with pytest.raises(ValueError):
        S([])
    assert keep.info()["device_bytes_all"] == before                   # every refusal came before the first allocation, or freed it
    rs2 = S(sp())
    assert rs2.info()["device_bytes_all"] == before + rs2.info()["device_bytes"]
    assert all(r.iters == 3 for r in rs2.run(3))
    rs2.destroy()
    assert keep.info()["device_bytes_all"] == before
    keep.destroy()


def test_scipy_matrices_are_the_triples(T):
    sps = pytest.importorskip("scipy.sparse")
    from totsu_amd import raggedsparse as RS
    host = [RC.host_problem(j) for j in (0, 3, 8, 12)]
    p = _param(T)

    def run(mats):
        rs = T.RaggedSparseBatchSolver([RS.SparseProblem(d.n, d.m, mt, d.vec_b, d.vec_c, d.seg_type, d.seg_len) for d, mt in zip(host, mats)], p)
        rs.run(10, poll_every=4)
        out = [_full(rs, i) for i in range(len(host))]
        rs.destroy()
        return out

    want = run([csc_of(d) for d in host])
    mats = [sps.coo_matrix(np.asarray(d.mat_a).reshape(d.n, d.m).T) for d in host]
    for g, w in zip(run(mats), want):
        _same_full(g, w)
