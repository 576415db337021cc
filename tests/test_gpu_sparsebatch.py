"""GPU: many problems of one shape, each with its OWN SPARSE A held as packed entries (totsu_amd.SparseBatchSolver /
thip_sparsebatch_*): every problem's iterates against the f64 oracle on sparse, PSD and fully dense families, both workgroup sizes
and state arithmetics, rows and columns of every length around the kernel's constants, resident against streamed (bitwise),
independence of index, neighbours, launch cuts and offsets (bitwise), the dense families as anchor, independent termination and the
tau -> 0 branch, replace, the refusals and info().  Every oracle state a test relies on is asserted first (tests/sparse_cases.py and
tests/ownbatch_cases.py assert theirs when they build a family).

The kernel's constants (thip_sparsebatch.hip):
    SPB_LONG = 32   a row or column of more entries is summed by one wave (64 lanes, entries l, l + 64, ..), a shorter one by one lane
    threads  = 256 when max(m, n) <= 1024 and nnz_cap <= 8192, else 1024"""
import numpy as np
import pytest

import oracle as O
import tau_zero_problems as Z
from ownbatch_cases import (ITERS, SDP_ITERS, SDP_TOLS, TOLS, F, T, _compare_snap, _dense_of, _snap, _same, _term_problem,  # noqa: F401
                            check_against_oracle)
from ownbatch_cases import family as _family
from sparse_cases import SHAPES, SPB_LONG, blob_of, csc_of, sparse_family

pytestmark = pytest.mark.gpu

STREAMED_BY_RULE = {"lp1000x700", "lp2000x1000"}       # the slot's capacity does not fit beside the vectors (asserted against fits)


def _param(T, **kw):
    p = T.SolverParam()
    p.eps_acc = 1e-30
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _check(T, label, ds, ros, iters, tols, **kw):
    from totsu_amd import sparsebatch
    info = check_against_oracle(T, T.SparseBatchSolver, label, ds, ros, iters, tols, **kw)
    d = ds[0]
    nnz = [int(csc_of(x)[0][-1]) for x in ds]
    cap = kw.get("nnz_cap") or max(nnz)
    lds, thr, res = sparsebatch.fits(d.n, d.m, d.seg_type, d.seg_len, cap)
    assert (info["nnz_cap"], info["nnz_total"], info["blob_bytes"]) == (cap, sum(nnz), sparsebatch.capacity_bytes(d.n, d.m, cap))
    if "force_resident" not in kw:
        assert info["resident"] == res and info["lds_bytes"] == lds
    if "force_threads" not in kw:
        assert info["threads"] == thr == (256 if max(d.m, d.n) <= 1024 and cap <= 8192 else 1024)
    used = [blob_of(x.n, x.m, *csc_of(x)).size for x in ds]
    assert info["a_bytes_per_iter"] == (0 if info["resident"] else 2 * 4 * (sum(used) // len(ds)))
    return info


# ---- 1. iterates against the oracle ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lp40x30", "lp257x129", "lp300x200", "mixed145x40", "mixed700x300", "lp1000x700", "lp2000x1000", "zero"])
def test_iterates_sparse(T, name):
    ds, ros, iters = sparse_family(name)
    tols = [TOLS[ITERS.index(i)] for i in iters]
    info = _check(T, name, ds, ros, iters, tols)
    assert info["resident"] == (0 if name in STREAMED_BY_RULE else 1)


@pytest.mark.parametrize("name", ["part48", "part23", "mixed", "sdp9"])
def test_iterates_psd(T, name):
    ds, ros = _family(T, name)
    info = _check(T, name, ds, ros, SDP_ITERS, SDP_TOLS)
    # (mixed: 812 x 5, every entry present, and the 49 920-byte tail of its order-33 cone: 71 512 bytes of blob do not fit beside them)
    assert info["resident"] == (0 if name == "mixed" else 1) and info["n_psd"] >= 1
    if name == "part48":
        assert (ds[0].m, ds[0].n, info["nnz_cap"], info["max_psd_order"], info["psd_lds_bytes"]) == (560, 528, 560, 32, 0)
    if name == "mixed":
        assert info["max_psd_order"] == 33 and info["psd_lds_bytes"] == 49920


@pytest.mark.parametrize("name", ["lp20", "socp", "qp"])
def test_iterates_dense_families(T, name):
    """every row of these is long or nearly full: the wave-per-row path on most of the matrix"""
    ds, ros = _family(T, name)
    info = _check(T, name, ds, ros, ITERS, TOLS)
    assert info["resident"] == 1


# ---- 2. both workgroup sizes, both state arithmetics ----------------------------------------------------------------------------

@pytest.mark.parametrize("arith", [None, "plain"])
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("name", ["lp40x30", "mixed145x40", "part23"])
def test_every_workgroup_size_and_state_arithmetic(T, name, threads, arith):
    if name in SHAPES:
        (ds, ros, iters), tols = sparse_family(name), TOLS
    else:
        (ds, ros), iters, tols = _family(T, name), SDP_ITERS, SDP_TOLS
    _check(T, "%s/%d/%s" % (name, threads, arith or "compensated"), ds, ros, iters, tols, force_threads=threads, state_arith=arith)


# ---- 3. rows and columns of every length ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("name", ["rows", "cols"])
def test_row_and_column_lengths(T, name, threads):
    """0, 1, SPB_LONG - 1, SPB_LONG, SPB_LONG + 1, 63, 64, 65, 128, 129 and 140 entries in a row (rows) or a column (cols)"""
    ds, ros, iters = sparse_family(name)
    A = np.asarray(ds[0].mat_a).reshape(ds[0].n, ds[0].m).T
    lens = (A != 0).sum(axis=1 if name == "rows" else 0)[:11]
    assert list(lens) == [0, 1, SPB_LONG - 1, SPB_LONG, SPB_LONG + 1, 63, 64, 65, 128, 129, 140]
    _check(T, "%s/%d" % (name, threads), ds, ros, iters, TOLS[:3], force_threads=threads)


@pytest.mark.parametrize("name", ["tiny1x1", "tiny1x300", "tiny300x1"])
def test_one_entry_one_row_one_column(T, name):
    ds, ros, iters = sparse_family(name)
    _check(T, name, ds, ros, iters, TOLS[:3])


# ---- 4. resident and streamed ---------------------------------------------------------------------------------------------------

def _bits(T, ds, cuts, **kw):
    """iterate, preconditioner and status of every problem after each cut of (steps, poll_every)"""
    sb = T.SparseBatchSolver.from_dense(ds, _param(T), **kw)
    out = []
    for steps, poll in cuts:
        sb.run(steps, poll_every=poll)
        out.append([_snap(sb, i) + sb.precond(i) for i in range(len(ds))])
    info = sb.info()
    sb.destroy()
    return out, info


def _same_bits(got, want):
    for g_cut, w_cut in zip(got, want):
        for g, w in zip(g_cut, w_cut):
            _same(g, w)
            assert np.array_equal(g[3], w[3]) and np.array_equal(g[4], w[4])


@pytest.mark.parametrize("name", ["lp300x200", "mixed145x40", "rows", "part23", "part48"])
def test_streamed_gives_the_resident_bits(T, name):
    ds = sparse_family(name)[0] if name in SHAPES or name == "rows" else _family(T, name)[0]
    cuts = [(1, 64), (9, 64), (40, 64)]                               # after 1, 10 and 50 iterations
    res, i1 = _bits(T, ds, cuts)
    stm, i0 = _bits(T, ds, cuts, force_resident=0)
    assert (i1["resident"], i0["resident"]) == (1, 0) and i1["a_bytes_per_iter"] == 0 < i0["a_bytes_per_iter"]
    assert i0["lds_bytes"] == i1["lds_bytes"] - i1["blob_bytes"]
    _same_bits(stm, res)


def test_a_capacity_beyond_lds_is_streamed_by_rule(T):
    ds, ros, iters = sparse_family("lp2000x1000")
    info = _check(T, "lp2000x1000/nnz_cap 40000", ds, ros, iters, TOLS[:2], nnz_cap=40000)
    assert (info["resident"], info["nnz_cap"], info["threads"]) == (0, 40000, 1024)
    with pytest.raises(ValueError, match="cannot be resident"):
        T.SparseBatchSolver.from_dense(ds, _param(T), nnz_cap=40000, force_resident=1)
    # and a larger capacity than the entries need moves no bit
    small = sparse_family("lp40x30")[0]
    cuts = [(10, 64)]
    res, i1 = _bits(T, small, cuts)
    big, i0 = _bits(T, small, cuts, nnz_cap=1200)
    assert i1["resident"] == 1 and i0["resident"] == 1 and i0["blob_bytes"] > i1["blob_bytes"]
    _same_bits(big, res)


# ---- 5. bitwise independence ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lp40x30", "mixed145x40"])
def test_a_problem_does_not_depend_on_index_neighbours_cuts_or_offsets(T, name):
    ds = sparse_family(name)[0]
    P = 300                                                            # more workgroups than the device has CUs
    cyc = [ds[i % len(ds)] for i in range(P)]
    cyc[P - 1] = ds[0]                                                 # the same problem at index 0 and at index 299
    p = _param(T)

    def run(problems, idx, poll):
        sb = T.SparseBatchSolver.from_dense(problems, p)
        sb.run(64, poll_every=poll)
        out = [_snap(sb, i) + sb.precond(i) for i in idx]
        launches = sb.info()["launches"]
        sb.destroy()
        return out, launches

    (alone,), l1 = run([ds[0]], [0], 64)
    assert l1 == 1 and alone[2][1] == 64
    for poll, launches in ((64, 1), (7, 10), (1, 64)):
        got, l = run(cyc, [0, P - 1], poll)
        assert l == launches
        for g in got:
            _same(g, alone)
            assert np.array_equal(g[3], alone[3]) and np.array_equal(g[4], alone[4])
    # behind another problem: its entries lie at another offset of the concatenated arrays
    (g,), _ = run([ds[1], ds[0]], [1], 64)
    _same(g, alone)


# ---- 6. the dense families as anchor --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("threads", [256, 1024])
def test_identity_rows_give_the_mid_batch_s_bits(T, threads):
    """A = [I; -I]: every product of either family's pass is exact and every sum is at most one rounding of two exact terms plus
    zeros, so the sparse pass and the dense pass give the same h and g, and the shared iteration the same iterates"""
    ds = sparse_family("identity")[0]
    assert all((d.m, d.n) == (80, 40) and int(csc_of(d)[0][-1]) == 80 for d in ds)
    p = _param(T)
    sp = T.SparseBatchSolver.from_dense(ds, p, force_threads=threads)
    md = T.MidBatchSolver.from_dense(ds, p, force_threads=threads)
    for i in range(len(ds)):
        for u, v in zip(sp.precond(i), md.precond(i)):
            assert np.array_equal(u, v)
    done = 0
    for it in (1, 10, 50):
        sp.run(it - done, poll_every=64)
        md.run(it - done, poll_every=64)
        done = it
        for i in range(len(ds)):
            g, w = _snap(sp, i), _snap(md, i)
            worst = max(np.abs(g[0] - w[0]).max(), np.abs(g[1] - w[1]).max())
            print("identity/%d problem %d after %d iterations: max difference %.3e" % (threads, i, it, worst))
            _same(g, w)
    sp.destroy()
    md.destroy()


@pytest.mark.parametrize("name", ["lp300x200", "part48"])
def test_agreement_with_the_dense_family(T, name):
    if name in SHAPES:
        (ds, _, _), dense, iters, tols = sparse_family(name), T.MidBatchSolver, ITERS, TOLS
    else:
        (ds, _), dense, iters, tols = _family(T, name), T.SdpBatchSolver, SDP_ITERS, SDP_TOLS
    p = _param(T)
    sp, dn = T.SparseBatchSolver.from_dense(ds, p), dense.from_dense(ds, p)
    done = 0
    for it, tol in zip(iters, tols):
        sp.run(it + 1 - done, poll_every=64)
        dn.run(it + 1 - done, poll_every=64)
        done = it + 1
        for i in range(len(ds)):
            for g, w in zip(sp.iterate(i), dn.iterate(i)):
                s = max(np.abs(w).max(), 1e-6)
                err = np.abs(g - w).max() / s
                print("%s problem %d iterate %d: sparse against dense %.2e (tol %.0e)" % (name, i, it, err, tol))
                assert err <= tol
    sp.destroy()
    dn.destroy()


# ---- 7. independent termination, the tau -> 0 branch ----------------------------------------------------------------------------

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
    sb = T.SparseBatchSolver.from_dense(ds, p)
    assert sb.info()["nnz_cap"] == 4 and sb.info()["nnz_total"] == sum(4 if i % 3 < 2 else 2 for i in range(P))
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


def _tau_zero_batch(name):
    from totsu_amd import sparsebatch
    fams, pls = Z.family(name), Z.plan(name)
    fams, pls = (fams, pls) if name == "F6" else ([fams], [pls])
    d = _dense_of(fams[0])
    sparsebatch.fits(d.n, d.m, d.seg_type, d.seg_len)                 # (F5, 588 x 64 with orders 6 and 33: taken)
    return fams, pls


@pytest.mark.parametrize("name", ["F1", "F2", "F3", "F4", "F5", "F6"])
def test_iterates_and_criteria_through_tau_zero(T, name):
    fams, pls = _tau_zero_batch(name)
    for fam, pl in zip(fams, pls):
        before, ones, after = Z.counts(pl)
        if fam.verdict != Z.OK:
            assert before >= 1 and ones >= 3 and (after >= 1 or not fam.flips_back), (fam.name, before, ones, after)
    p = T.SolverParam()
    p.eps_acc = p.eps_inf = 1e-30
    sb = T.SparseBatchSolver.from_dense([_dense_of(f) for f in fams], p)
    done = 0
    for it in sorted(set(i for pl in pls for i in pl.chosen)):
        sb.run(it + 1 - done, poll_every=64)
        done = it + 1
        for q, (fam, pl) in enumerate(zip(fams, pls)):
            if it in pl.chosen:
                x, y = sb.iterate(q)
                _compare_snap("sparsebatch/%s" % fam.name, fam, pl, it, x, y, sb.status(q))
    assert all(sb.status(q).state == -1 for q in range(len(fams)))
    if name == "F6":                                   # the slots are in different regimes at the end of the window
        assert [sb.status(q).kind for q in range(3)] == [0, 1, 1] == [pl.kinds[-1] for pl in pls]
    sb.destroy()


@pytest.mark.parametrize("name", ["F1", "F2", "F3", "F4", "F5", "F6"])
def test_verdicts_through_tau_zero(T, name):
    fams, pls = _tau_zero_batch(name)
    for fam, pl in zip(fams, pls):
        assert pl.status == fam.verdict and pl.iters <= Z.MAX_VERDICT_ITER
    p = T.SolverParam()
    p.max_iter, p.eps_acc, p.eps_inf = 100_000, Z.EPS, Z.EPS
    sb = T.SparseBatchSolver.from_dense([_dense_of(f) for f in fams], p)
    res = sb.run(-1, poll_every=25)
    n, m = fams[0].n, fams[0].m
    for q, (fam, pl, r) in enumerate(zip(fams, pls, res)):
        margin = max(3, pl.iters // 50)
        print("tau_zero verdict sparsebatch/%-14s state %d at %d (oracle %d at %d, margin %d) kind %d cri %s"
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


# ---- 8. replace -----------------------------------------------------------------------------------------------------------------

def test_replace(T):
    """a slot given a problem with ANOTHER pattern (and fewer or as many entries as nnz_cap) is a fresh batch's slot bit for bit"""
    from totsu_amd import _lib
    from sparse_cases import sparse_problem
    ds = sparse_family("lp40x30")[0]
    new = sparse_problem("lp40x30", 17)
    nnz = [int(csc_of(d)[0][-1]) for d in ds[:3]]
    nnz_new = int(csc_of(new)[0][-1])
    cap = max(nnz + [nnz_new])
    assert not np.array_equal(csc_of(new)[1][:20], csc_of(ds[1])[1][:20])      # another pattern
    p = _param(T)

    def snaps(sb, i):
        st = sb.status(i)
        out = [sb.precond(i) + ((st.state, st.iters, st.tau, st.kappa, st.norm_b, st.norm_c),)]
        done = 0
        for it in (0, 1, 9):
            sb.run(it + 1 - done, poll_every=64)
            done = it + 1
            out.append(_snap(sb, i))
        return out

    def same(got, want):
        for g, w in zip(got, want):
            assert len(g) == len(w) == 3
            _same(g, w)

    fresh = T.SparseBatchSolver.from_dense([new], p)
    want_new = snaps(fresh, 0)
    fresh.destroy()
    untouched = T.SparseBatchSolver.from_dense(ds[:3], p)
    untouched.run(5 + 10, poll_every=64)
    want_others = [untouched.iterate(i) for i in range(3)]
    untouched.destroy()

    sb = T.SparseBatchSolver.from_dense(ds[:3], p, nnz_cap=cap)
    sb.run(5, poll_every=64)
    sb.replace(1, csc_of(new), new.vec_b, new.vec_c)
    st = sb.status(1)
    info = sb.info()
    assert st.state == _lib.ST_RUNNING and st.iters == 0 and info["live"] == 3
    assert info["nnz_total"] == nnz[0] + nnz_new + nnz[2] and info["nnz_cap"] == cap
    same(snaps(sb, 1), want_new)                       # the other slots advance by the same 10 iterations
    for i in (0, 2):
        x, y = sb.iterate(i)
        assert np.array_equal(x, want_others[i][0]) and np.array_equal(y, want_others[i][1])
    # more entries than the slot can take: both numbers are named, nothing moves
    full = np.ones((40, 30), F)
    from ownbatch_cases import _D
    too_big = csc_of(_D(full, np.zeros(40), np.zeros(30), [1], [40]))
    before = _snap(sb, 1)
    with pytest.raises(ValueError, match="1200 entries where nnz_cap is %d" % cap):
        sb.replace(1, too_big, new.vec_b, new.vec_c)
    _same(_snap(sb, 1), before)
    sb.destroy()

    # a stopped slot can be replaced
    sb = T.SparseBatchSolver.from_dense(ds[:3], _param(T, max_iter=6), nnz_cap=cap)
    res = sb.run(-1, poll_every=4)
    assert all(r.state == _lib.ST_EXCESS_ITER for r in res) and sb.info()["live"] == 0
    sb.set_param(p)
    sb.replace(1, csc_of(new), new.vec_b, new.vec_c)
    assert sb.info()["live"] == 1
    same(snaps(sb, 1), want_new)
    assert [sb.status(i).state for i in range(3)] == [_lib.ST_EXCESS_ITER, _lib.ST_RUNNING, _lib.ST_EXCESS_ITER]
    sb.destroy()


def test_scipy_matrices_are_the_triples(T):
    sp = pytest.importorskip("scipy.sparse")
    ds = sparse_family("lp40x30")[0]
    p = _param(T)
    b, c = np.stack([d.vec_b for d in ds]), np.stack([d.vec_c for d in ds])

    def run(mats):
        sb = T.SparseBatchSolver(30, 40, mats, b, c, [1], [40], p)
        sb.run(10, poll_every=4)
        out = [_snap(sb, i) for i in range(len(ds))]
        sb.destroy()
        return out

    want = run([csc_of(d) for d in ds])
    mats = [sp.coo_matrix(np.asarray(d.mat_a).reshape(30, 40).T) for d in ds]
    for g, w in zip(run(mats), want):
        _same(g, w)


# ---- 9. refusals and info -------------------------------------------------------------------------------------------------------

def test_refusals_leave_nothing_allocated(T):
    from totsu_amd import _lib
    S = T.SparseBatchSolver
    ds = sparse_family("lp40x30")[0]
    d = ds[0]
    b, c = np.stack([x.vec_b for x in ds]), np.stack([x.vec_c for x in ds])
    good = [csc_of(x) for x in ds]
    keep = S(30, 40, good, b, c, [1], [40])
    all0 = keep.info()["device_bytes_all"]
    assert all0 == keep.info()["device_bytes"] > 0

    def bad(k, cp=None, ri=None, va=None):
        t = [np.array(v) for v in good[k]]
        for i, v in enumerate((cp, ri, va)):
            if v is not None:
                t[i] = v(t[i])
        out = list(good)
        out[k] = tuple(t)
        return out

    def set_at(i, v):
        def f(a):
            a = a.copy()
            a[i] = v
            return a
        return f

    cases = [("problem 1: the column pointers are not monotone from 0", bad(1, cp=set_at(0, 1))),
             ("problem 2: the column pointers are not monotone from 0", bad(2, cp=set_at(5, 0))),
             ("problem 0: a row index is out of range", bad(0, ri=set_at(3, 40))),
             ("problem 0: the row indices of a column are not strictly ascending", bad(0, ri=lambda a: np.concatenate([a[1:2], a[1:]]))),
             ("problem 1: a value of A is not finite", bad(1, va=set_at(7, np.nan))),
             ("problem 2: a value of A is not finite", bad(2, va=set_at(0, -np.inf)))]
    assert good[0][0][1] >= 2                                           # (the first column holds two entries: duplicating the second row index breaks the order)
    for words, mats in cases:
        with pytest.raises(ValueError, match=words):
            S(30, 40, mats, b, c, [1], [40])
    with pytest.raises(ValueError, match="problem 0 holds %d entries where nnz_cap is 10" % int(good[0][0][-1])):
        S(30, 40, good, b, c, [1], [40], nnz_cap=10)
    with pytest.raises(ValueError, match="nnz_cap 1201 exceeds m n = 1200"):
        S(30, 40, good, b, c, [1], [40], nnz_cap=1201)
    with pytest.raises(ValueError, match="order above 64"):
        S(5, 2145, [(np.zeros(6, np.int64), [], [])], np.zeros((1, 2145), F), np.zeros((1, 5), F), [_lib.CONE_PSD], [2145])
    with pytest.raises(ValueError, match="do not cover m rows"):
        S(30, 40, good, b, c, [1], [39])
    with pytest.raises(ValueError, match="vecs_b"):
        S(30, 40, good, b[:2], c, [1], [40])
    with pytest.raises(ValueError, match="256 or 1024"):
        S(30, 40, good, b, c, [1], [40], force_threads=512)
    assert keep.info()["device_bytes_all"] == all0                     # every refusal came before the first allocation, or freed it
    keep.destroy()


def test_info_matches_the_cpu_packing(T):
    from totsu_amd import sparsebatch
    ds, _ = _family(T, "part48")
    P = 64
    cyc = [ds[i % len(ds)] for i in range(P)]
    d = ds[0]
    n, m = d.n, d.m
    sp = T.SparseBatchSolver.from_dense(cyc, _param(T))
    dn = T.SdpBatchSolver.from_dense(cyc, _param(T))
    i_sp, i_dn = sp.info(), dn.info()
    sp.destroy()
    dn.destroy()
    nnz = [int(csc_of(x)[0][-1]) for x in cyc]
    assert nnz == [560] * P
    blob = sparsebatch.capacity_bytes(n, m, 560)
    assert blob == 16 * 560 + 4 * (2 * (m + n) + 4) == 17680
    assert (i_sp["nnz_cap"], i_sp["nnz_total"], i_sp["blob_bytes"], i_sp["resident"]) == (560, 560 * P, blob, 1)
    stride = 4 * (6 * n + 10 * m)
    # the arena, the status blocks, the slots, the live list, the class bytes, the cone table -- and the blobs
    common = P * (stride + 64 + 32 + 4) + ((m + 3) & ~3) + 4 * 3
    assert i_dn["device_bytes"] == common and i_sp["device_bytes"] == common + P * blob
    assert i_sp["arena_bytes"] == i_dn["arena_bytes"] == P * stride
    # what the two routes hold of A on the device: the blobs against the dense arrays the SDP batch streams (its info counts the
    # handle's own allocations, the caller's A is beside them)
    a_sparse, a_dense = P * blob, P * 4 * m * n
    print("part48 x %d: A on the device %d bytes sparse, %d bytes dense (1 / %.1f); whole handles with A: %d against %d (1 / %.1f)"
          % (P, a_sparse, a_dense, a_dense / a_sparse, i_sp["device_bytes"], i_dn["device_bytes"] + a_dense,
             (i_dn["device_bytes"] + a_dense) / i_sp["device_bytes"]))
    assert i_sp["device_bytes"] - common == a_sparse and 50 * a_sparse < a_dense
