"""GPU: many small SDPs, each with its OWN A, the PSD cones projected on chip by the problem's workgroup (totsu_amd.SdpBatchSolver /
thip_sdpbatch_*): the projection alone against the f64 oracle, every problem's iterates against the oracle, isolation from the
neighbours, the launch boundaries and the alignment of A (bitwise), the mid batch's bits on layouts without PSD cones, independent
termination, the tau -> 0 branch, the refusals.  Every oracle state a test relies on is asserted first.  The families, the
oracle runs and the helpers are those of tests/ownbatch_cases.py.

The kernel's constants (thip_sdpbatch.hip): operands of extent 32 (one wave) up to order 32 and 64 (four waves) above; K walked in
chunks of 4 MFMA steps, ceil(k / 8) of them; workgroups of 256 or 1024 threads."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import tau_zero_problems as Z
from ownbatch_cases import SDP_ITERS as ITERS
from ownbatch_cases import SDP_TOLS as TOLS
from ownbatch_cases import (F, T, _compare_snap, _dense_of, _same, _sdp_dense, _snap, _View, check_against_oracle,  # noqa: F401
                            tri)
from ownbatch_cases import family as _family

pytestmark = pytest.mark.gpu

LARGEST = 57                                                   # the largest order a layout can hold (tests/test_sdpbatch_cpu.py)


# ---- 1. the projection alone ---------------------------------------------------------------------------------------------------

def _packed(s):
    k = s.shape[0]
    return np.array([s[r, c] * (np.sqrt(2.0) if r != c else 1.0) for c in range(k) for r in range(c + 1)], dtype=F)


def _rand_sym(k, seed, rank_def=False):
    """tests/test_gpu_eig.py: a full-rank matrix, or a few large eigenvalues of both signs and many exact zeros"""
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((k, k))
    s = (b + b.T) / 2
    if rank_def and k > 3:
        q, _ = np.linalg.qr(b)
        w = np.zeros(k)
        w[: k // 4] = rng.uniform(0.5, 2.0, k // 4)
        w[k // 4: k // 2] = -rng.uniform(0.5, 2.0, k // 2 - k // 4)
        s = (q * w) @ q.T
    return s


def _project(T, k, xs, rxs=None):
    """thip_test_sdpbatch_project on the packed matrices xs (count x k (k + 1) / 2) in ONE launch -> the projections[, the rx]"""
    from totsu_amd._lib import lib
    xs = np.ascontiguousarray(xs, dtype=F).reshape(-1, tri(k))
    dx = T.DeviceBuffer.from_host(xs)
    dr = None if rxs is None else T.DeviceBuffer.from_host(np.ascontiguousarray(rxs, dtype=F))
    lib.thip_test_sdpbatch_project(k, xs.shape[0], dx.ptr, None if dr is None else dr.ptr)
    out = dx.to_host().reshape(xs.shape)
    dx.free()
    if dr is None:
        return out
    r = dr.to_host().reshape(xs.shape)
    dr.free()
    return out, r


@pytest.mark.parametrize("k,rank_def", [(k, r) for k in [1, 2, 3, 31, 32, 33, 47, 48, LARGEST, 64] for r in (False, True)])
def test_psd_projection(T, k, rank_def):
    x = _packed(_rand_sym(k, k + 17 * rank_def, rank_def))
    ref = O.proj(O.CONE_PSD, x.astype(np.float64), use_ql=True)
    rx0 = np.random.default_rng(k).standard_normal(x.size).astype(F)
    got, rx = _project(T, k, x, rx0)
    got = got[0]
    err = np.abs(got - ref).max() / np.linalg.norm(x)
    again = _project(T, k, got)[0]
    err2 = np.abs(again - got).max() / np.linalg.norm(x)
    print("sdpbatch projection k = %2d %s: err %.2e, idempotence %.2e (tol 2e-5)" % (k, "rank-deficient" if rank_def else "full rank", err, err2))
    assert err <= 2e-5, err
    assert err2 <= 2e-5, err2
    assert np.array_equal(rx[0], rx0 - F(2.0) * got)               # the reflection that rides in the pack


@pytest.mark.parametrize("k", [1, 2, 4, 6, 12, 32, 40, 64])
def test_psd_projection_at_every_scale_and_on_special_matrices(T, k):
    """the cases and tolerances of tests/test_gpu_eig.py::test_psd_projection_at_every_scale_and_on_special_matrices"""
    rng = np.random.default_rng(k)
    b = rng.standard_normal((k, k))
    s = (b + b.T) / 2
    v = rng.standard_normal((k, 1))
    e0 = np.zeros((k, k))
    e0[0, 0] = 1.0
    cases = [("random", s, 2e-5), ("1e-18", s * 1e-18, 2e-5), ("1e-25", s * 1e-25, 2e-5), ("1e15", s * 1e15, 2e-5),
             ("subnormal 1e-40", s * 1e-40, 1e-3), ("subnormal 3e-44", s * 3e-44, 0.2),
             ("zero", np.zeros((k, k)), 0.0), ("identity", np.eye(k), 2e-5), ("-identity", -np.eye(k), 2e-5),
             ("rank one", v @ v.T, 2e-5), ("-rank one", -(v @ v.T), 2e-5), ("diagonal", np.diag(rng.standard_normal(k)), 2e-5),
             ("e0 e0^T", e0, 2e-5)]
    xs = np.stack([_packed(mat) for _, mat, _ in cases])
    gots = _project(T, k, xs)                                      # (one launch: a workgroup each)
    for (tag, mat, tol), x, got in zip(cases, xs, gots):
        ev, z = np.linalg.eigh(mat.astype(np.float64))
        ref = _packed((z * np.maximum(ev, 0)) @ z.T).astype(np.float64)
        assert np.all(np.isfinite(got)), tag
        assert np.abs(got - ref).max() <= tol * np.linalg.norm(x.astype(np.float64)), (tag, np.abs(got - ref).max())


@pytest.mark.parametrize("k", [12, 40])
def test_a_batch_of_projections_is_each_one_alone(T, k):
    xs = np.stack([_packed(_rand_sym(k, 1000 + i, i % 2 == 1)) for i in range(70)])
    rx0 = np.random.default_rng(k).standard_normal(xs.shape).astype(F)
    got, rx = _project(T, k, xs, rx0)
    for i in range(70):
        g1, r1 = _project(T, k, xs[i], rx0[i])
        assert np.array_equal(g1[0], got[i]) and np.array_equal(r1[0], rx[i]), i


# ---- 2. iterates against the oracle, every problem with its own A --------------------------------------------------------------

def _check(T, label, ds, ros, **kw):
    info = check_against_oracle(T, T.SdpBatchSolver, label, ds, ros, ITERS, TOLS, **kw)
    assert info["a_bytes_per_iter"] == 8 * ds[0].m * ds[0].n
    return info


@pytest.mark.parametrize("name", ["sdp9", "sdp24", "sdp33", "sdp48", "part23", "part44", "mixed"])
def test_iterates_own_a(T, name):
    ds, ros = _family(T, name)
    info = _check(T, name, ds, ros)
    assert info["threads"] == (1024 if ds[0].m * ds[0].n > 8192 else 256)
    if name == "part44":
        assert (ds[0].n, ds[0].m) == (136, 152)


@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("name", ["sdp9", "sdp33", "mixed"])
def test_iterates_every_workgroup_size(T, name, threads):
    ds, ros = _family(T, name)
    _check(T, "%s/%d threads" % (name, threads), ds, ros, force_threads=threads)


@pytest.mark.parametrize("name", ["sdp24", "sdp48", "mixed"])
def test_iterates_plain_state(T, name):
    ds, ros = _family(T, name)
    _check(T, name + "/plain", ds, ros, state_arith="plain")


# ---- 3. bitwise properties -----------------------------------------------------------------------------------------------------

def test_a_problem_does_not_depend_on_its_index_or_its_neighbours(T):
    ds = [_sdp_dense(T, 6, 9, seed) for seed in range(39)]
    ds.append(ds[0])                                               # the same SDP at index 0 and at index 39
    p = T.SolverParam()
    p.eps_acc = 1e-30

    def run(dd, idx):
        sb = T.SdpBatchSolver.from_dense(dd, p)
        sb.run(60, poll_every=25)
        out = [_snap(sb, i) for i in idx]
        sb.destroy()
        return out

    alone = run(ds[:1], [0])[0]
    assert alone[2][1] == 60
    for got in run(ds, [0, 39]):
        _same(got, alone)


@pytest.mark.parametrize("name", ["sdp33", "mixed"])
def test_launch_cuts_change_nothing(T, name):
    ds, _ = _family(T, name)
    p = T.SolverParam()
    p.eps_acc = 1e-30

    def run(steps, poll):
        sb = T.SdpBatchSolver.from_dense(ds, p)
        sb.run(steps, poll_every=poll)
        out = [_snap(sb, i) for i in range(len(ds))]
        launches = sb.info()["launches"]
        sb.destroy()
        return out, launches

    one, l1 = run(50, 50)
    single, l50 = run(50, 1)
    assert (l1, l50) == (1, 50) and all(o[2][1] == 50 for o in one)
    for g, w in zip(single, one):
        _same(g, w)


def test_a_replaced_slot_is_a_fresh_init(T):
    from totsu_amd import _lib
    ds, _ = _family(T, "sdp33")
    p = T.SolverParam()
    p.eps_acc = 1e-30

    def snaps(sb, i):
        st = sb.status(i)
        out = [sb.precond(i) + ((st.state, st.iters, st.tau, st.kappa, st.norm_b, st.norm_c),)]
        done = 0
        for it in (0, 1, 9):
            sb.run(it + 1 - done, poll_every=64)
            done = it + 1
            out.append(_snap(sb, i))
        return out

    fresh = T.SdpBatchSolver.from_dense([ds[2]], p)
    want = snaps(fresh, 0)
    fresh.destroy()
    sb = T.SdpBatchSolver.from_dense(ds[:2], p)
    sb.run(5, poll_every=64)
    sb.replace(1, ds[2].mat_a, ds[2].vec_b, ds[2].vec_c)
    st = sb.status(1)
    assert st.state == _lib.ST_RUNNING and st.iters == 0 and sb.info()["live"] == 2
    for g, w in zip(snaps(sb, 1), want):
        _same(g, w)
    assert sb.status(0).iters == 15
    sb.destroy()


def test_unaligned_a_takes_the_4_byte_path_with_the_same_bits(T):
    ds, _ = _family(T, "sdp24")                                    # m = 300: a multiple of 4, every A 16-byte aligned
    p = T.SolverParam()
    p.eps_acc = 1e-30
    a = np.stack([d.mat_a for d in ds])
    b, c = np.stack([d.vec_b for d in ds]), np.stack([d.vec_c for d in ds])

    def run(mats):
        sb = T.SdpBatchSolver(6, 300, mats, b, c, ds[0].seg_type, ds[0].seg_len, p)
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


# ---- 4. no PSD cone: the shared code is shared ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lp80", "socp60"])
def test_without_psd_cones_the_bits_are_the_mid_batch_s(T, name):
    ds, _ = _family(T, name)
    p = T.SolverParam()
    p.eps_acc = 1e-30
    out = []
    for cls in (T.MidBatchSolver, T.SdpBatchSolver):
        sb = cls.from_dense(ds, p)
        sb.run(100, poll_every=32)
        out.append([_snap(sb, i) + sb.precond(i) for i in range(len(ds))])
        info = sb.info()
        sb.destroy()
    assert (info["max_psd_order"], info["n_psd"], info["psd_lds_bytes"]) == (0, 0, 0)
    for g, w in zip(*out):
        assert g[2] == w[2] and g[2][1] == 100
        for u, v in zip(g[:2] + g[3:], w[:2] + w[3:]):
            assert np.array_equal(u, v)


# ---- 5. independent termination ------------------------------------------------------------------------------------------------

def test_independent_termination(T):
    from totsu_amd import _lib
    ds = [_sdp_dense(T, 6, 9, seed) for seed in range(6)]
    ros = [O.solve_matop_cones(O.param(max_iter=100000, eps_acc=1e-4), d.vec_c, d.mat_a, d.vec_b, d.seg_type, d.seg_len, use_ql=True)
           for d in ds]
    assert all(ro.status == O.OK for ro in ros), [ro.status_name for ro in ros]
    assert [ro.iters for ro in ros[:3]] == [373, 503, 667], [ro.iters for ro in ros]
    assert len(set(ro.iters for ro in ros)) >= 3
    p = T.SolverParam()
    p.max_iter, p.eps_acc = 100000, 1e-4
    sb = T.SdpBatchSolver.from_dense(ds, p)
    early, live = {}, [len(ds)]
    while True:
        res = sb.run_until_any(-1, poll_every=16)
        live.append(sb.info()["live"])
        for i, r in enumerate(res):
            if r.state != _lib.ST_RUNNING and i not in early:
                early[i] = (r.state, r.iters, r.kind) + sb.iterate(i)
        if all(r.state != _lib.ST_RUNNING for r in res):
            break
        assert len(live) <= len(ds) + 1
    print("independent termination: iterations", [r.iters for r in res], "oracle", [ro.iters for ro in ros])
    assert live[0] == len(ds) and live[-1] == 0 and len(set(live)) >= 3 and live == sorted(live, reverse=True)
    for i, ro in enumerate(ros):
        assert res[i].state == ro.status == _lib.ST_OK, (i, res[i].state)
        assert abs(res[i].iters - ro.iters) <= max(3, ro.iters // 50), (i, res[i].iters, ro.iters)
        st, it, kind, x, y = early[i]                              # what the problem held when it was first seen stopped
        x2, y2 = sb.iterate(i)
        assert (st, it, kind) == (res[i].state, res[i].iters, res[i].kind)
        assert np.array_equal(x, x2) and np.array_equal(y, y2)
    for i, s_ in enumerate(sb.solve()):
        assert isinstance(s_, tuple)
        assert np.abs(s_[0] - ros[i].x).max() <= 2e-3 * max(1.0, np.abs(ros[i].x).max()), i
    sb.destroy()


# ---- 6. the tau -> 0 branch: family F5 (588 x 64, orders 6 and 33, infeasible) --------------------------------------------------

def test_iterates_and_criteria_through_tau_zero(T):
    fam, pl = Z.family("F5"), Z.plan("F5")
    assert fam.psd and (fam.m, fam.n) == (588, 64) and fam.tol(0) == Z.TOLS_PSD[0]
    before, ones, after = Z.counts(pl)
    assert before >= 1 and ones >= 3 and (after >= 1 or not fam.flips_back), (before, ones, after)
    p = T.SolverParam()
    p.eps_acc = p.eps_inf = 1e-30
    sb = T.SdpBatchSolver.from_dense([_dense_of(fam)], p)
    assert sb.info()["max_psd_order"] == 33 and sb.info()["psd_lds_bytes"] == 49920
    done = 0
    for it in pl.chosen:
        sb.run(it + 1 - done, poll_every=64)
        done = it + 1
        x, y = sb.iterate(0)
        _compare_snap("sdpbatch/F5", fam, pl, it, x, y, sb.status(0))
    assert sb.status(0).state == -1
    sb.destroy()


def test_verdict_through_tau_zero(T):
    fam, pl = Z.family("F5"), Z.plan("F5")
    assert pl.status == fam.verdict == Z.INFEASIBLE and pl.iters <= Z.MAX_VERDICT_ITER
    p = T.SolverParam()
    p.max_iter, p.eps_acc, p.eps_inf = 100_000, Z.EPS, Z.EPS
    sb = T.SdpBatchSolver.from_dense([_dense_of(fam)], p)
    r = sb.run(-1, poll_every=25)[0]
    n, m = fam.n, fam.m
    margin = max(3, pl.iters // 50)
    print("tau_zero verdict sdpbatch/F5 state %d at %d (oracle %d at %d, margin %d) kind %d cri %s"
          % (r.state, r.iters, pl.status, pl.iters, margin, r.kind, tuple("%.3e" % c for c in r.cri)))
    assert r.state == pl.status, (r.state, pl.status)
    assert abs(r.iters - pl.iters) <= margin, (r.iters, pl.iters)
    (x, y), sol = sb.iterate(0), sb.solution(0)
    assert r.kind == 1 and r.tau == 0.0 and x[n + 2 * m] == 0.0, (r.kind, r.tau)
    assert r.cri[1] <= Z.EPS, r.cri
    assert np.array_equal(sol[0], x[:n]) and np.array_equal(sol[1], x[n:n + m])
    sb.destroy()


# ---- 7. refusals, info, conic_batch --------------------------------------------------------------------------------------------

def test_refusals_leave_nothing_allocated(T):
    from totsu_amd import _lib
    from totsu_amd._lib import lib
    S = T.SdpBatchSolver
    PSD = _lib.CONE_PSD
    z = lambda *s: np.zeros(s, F)
    ds, _ = _family(T, "sdp33")
    keep = S.from_dense(ds)                            # something alive, so that device_bytes_all can be read before and after
    info = keep.info()
    before = info["device_bytes_all"]
    assert before == info["device_bytes"] > info["arena_bytes"] > 0
    assert (info["max_psd_order"], info["n_psd"], info["psd_lds_bytes"]) == (33, 1, 49920)
    assert info["lds_bytes"] == 4 * (6208 + 8 * 6 + 13 * 561) + 564 + 49920 and info["n_prob"] == 3 and info["live"] == 3
    bad = [lambda: S(3, 7, z(2, 21), z(2, 7), z(2, 3), [PSD], [7]),
           lambda: S(3, 2145, z(1, 3 * 2145), z(1, 2145), z(1, 3), [PSD], [2145]),
           lambda: S(2, 4097, z(1, 2 * 4097), z(1, 4097), z(1, 2), [1], [4097]),
           lambda: S(4097, 2, z(1, 2 * 4097), z(1, 2), z(1, 4097), [1], [2]),
           lambda: S(837, 1176, z(1, 1), z(1, 1176), z(1, 837), [PSD], [1176]),
           lambda: S(3, 6, z(2, 18), z(2, 6), z(2, 3), [PSD], [3]),
           lambda: S(3, 6, z(0, 18), z(0, 6), z(0, 3), [PSD], [6]),
           lambda: S(3, 6, z(2, 17), z(2, 6), z(2, 3), [PSD], [6]),
           lambda: S(3, 6, z(2, 18), z(2, 6), z(3, 3), [PSD], [6])]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    sdp9, _ = _family(T, "sdp9")
    with pytest.raises(ValueError):
        S.from_dense([ds[0], sdp9[0]])
    # the C ABI itself, over device arrays that exist: THIP_E_INVALID, thip_last_error set, *out stays NULL
    da, db, dc = (T.DeviceBuffer.from_host(z(64)) for _ in range(3))
    par = _lib.Param(-1, 1e-6, 1e-6, 1e-12, 0, 0, 0)

    def create(n, m, P, st, sl, null_seg=False):
        st, sl = np.asarray(st, np.int32), np.asarray(sl, np.int64)
        h = C.c_void_p()
        with pytest.raises(_lib.ThipError) as e:
            lib.thip_sdpbatch_create(n, m, P, da.ptr, db.ptr, dc.ptr, None, st.size,
                                     None if null_seg else st.ctypes.data_as(C.POINTER(C.c_int32)),
                                     sl.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(par), C.byref(h))
        assert e.value.code == _lib.E_INVALID and not h.value and _lib.load().thip_last_error()
        assert keep.info()["device_bytes_all"] == before

    create(3, 7, 2, [PSD], [7])                        # not triangular
    create(3, 8, 2, [1, PSD], [4, 4])
    create(3, 2145, 1, [PSD], [2145])                  # order 65
    create(2, 4097, 1, [1], [4097])
    create(4097, 2, 1, [1], [2])
    create(837, 1176, 1, [PSD], [1176])                # a map beyond LDS
    create(3, 6, 2, [PSD], [3])
    create(3, 6, 2, [PSD, 1], [6, 1])
    create(3, 6, 2, [9], [6])                          # an unknown segment
    create(3, 6, 2, [PSD], [6], null_seg=True)         # a null one
    create(3, 6, 0, [PSD], [6])
    create(3, 6, 1048577, [PSD], [6])
    for d in (da, db, dc):
        d.free()
    with pytest.raises(_lib.ThipError):                # the projection hook's own bounds
        lib.thip_test_sdpbatch_project(65, 1, keep.mats_a.ptr, None)
    with pytest.raises(_lib.ThipError):
        lib.thip_test_sdpbatch_project(0, 1, keep.mats_a.ptr, None)
    # no refusal left device memory behind: a later object is all the library holds beside the first
    sb2 = S.from_dense(sdp9)
    assert sb2.info()["device_bytes_all"] == before + sb2.info()["device_bytes"]
    assert (sb2.info()["max_psd_order"], sb2.info()["psd_lds_bytes"]) == (9, 0)
    sb2.destroy()
    assert keep.info()["device_bytes_all"] == before
    keep.destroy()


def test_conic_batch_returns_the_batch_the_layout_needs(T):
    lp20, _ = _family(T, "lp20")
    lp260, _ = _family(T, "lp260")
    sdp9, _ = _family(T, "sdp9")
    small, mid, sdp = T.conic_batch(lp20), T.conic_batch(lp260[:2]), T.conic_batch(sdp9)
    assert (type(small), type(mid), type(sdp)) == (T.SmallBatchSolver, T.MidBatchSolver, T.SdpBatchSolver)
    for sb in (small, mid, sdp):
        assert all(r.iters == 3 for r in sb.run(3))
        sb.destroy()
    with pytest.raises(ValueError, match="FusedSolver"):
        T.own_a_batch(sdp9)
