"""GPU tests of the tau -> 0 branch of the iteration (criteria_inf, solver.rs:614-656) on every kernel that carries it.

While tau > eps_zero the criteria are criteria_conv's; once tau has been clamped to 0 they are p = x_s + A x_x, d = A^T x_y,
cri_unbdd / cri_infeas (inf where the denominator is not positive), the verdicts Unbounded / Infeasible, and an ending that is NOT
scaled by 1 / tau.  That branch is written eight times in device code (post_k, ycrit_k, status_eval, sw_xm_k, sw_cone_k, sw_vm_k,
sweep_k, sp_col_k), next to the clamps tau <- max(tau, 0) (xupdate_k, status_eval's tau_next, sw_tau_k) and kappa <- min(kappa, 0)
(ycrit_k, sweep_k, sp_col_k), finalize_k's rule not to scale a kind-1 ending and thip_solver_resume's refusal of one.  The problems
are the seeded families of tests/tau_zero_problems.py (random unsymmetric A, no two rows alike, block cones included), validated
on the CPU oracle by tests/test_tau_zero_families_cpu.py, which also explains which iterations are DECISIVE (the f32 loop and the
f64 oracle are provably on the same side of eps_zero there).  Every leg first asserts the path that ran: schedule, stored form,
passes, and for the one-pass legs the m-tail form the library reports (1 merged, 2 a wave per cone, 3 three launches, + 4 one
thread per row).

Measured on an MI355X (the test prints every figure before it asserts).

Oracle, eps_acc = eps_inf = 1e-5: verdict iteration, and the iterations below 100 at which the kind of the criteria flips:
    F1 Infeasible at 1212, flips [3]          F2 Unbounded at 481, flips [5]         F3 Infeasible at 805, flips [4, 8, 16]
    F4 Unbounded at 378, flips [6, 8, 33]     F5 Infeasible at 1344, flips [4]       (F3 on the bf16 matrix: 806; on the f16 one: 805)
    F6: OK at 1383, no flip; Infeasible at 552, flips [5]; Unbounded at 481, flips [5]
Every leg, the batch's three slots and the trait-level Solver reached the oracle's verdict AT the oracle's iteration (difference 0
in all 33 runs; the margin asserted is max(3, iters // 50)).

Largest relative deviation of the iterate (x or y, of the largest entry) at each chosen snap; z: tau is 0 there, *: not decisive.
The ladder allows 2e-5 / 1e-4 / 2e-3 (5e-5 / 3e-4 / 3e-3 with PSD blocks); nothing measured is above 8e-7:
    reference/F1         0:4.7e-08 1:1.2e-07 2:2.0e-07 3z:1.9e-07 9z:2.0e-07 49z:1.6e-07 99z:1.9e-07
    reference/F2         0:7.3e-08 1:1.3e-07 4:1.1e-07 5z:9.4e-08 9z:2.4e-07 49z:9.7e-08 99z:7.8e-08
    reference/F3         0:6.9e-08 1:1.1e-07 3:1.1e-07 4z:9.8e-08 7z:7.7e-08 8:8.8e-08 9:9.5e-08 15:1.2e-07* 16z:9.5e-08* 49z:1.5e-07 99z:1.5e-07
    reference/F4         0:3.1e-08 1:6.0e-08 5:5.9e-08 6z:8.9e-08 7z:1.8e-07 8:1.6e-07 9:1.3e-07 32:2.5e-07* 33z:1.7e-07 49z:1.6e-07 99z:1.1e-07
    reference/F5         0:4.1e-08 1:1.1e-07 3:2.1e-07 4z:2.0e-07 9z:4.9e-07 49z:3.7e-07 99z:7.6e-07
    fused/F1             0:4.7e-08 1:1.2e-07 2:2.0e-07 3z:1.9e-07 9z:2.0e-07 49z:1.6e-07 99z:1.9e-07
    fused/F2             0:7.3e-08 1:1.3e-07 4:1.1e-07 5z:9.4e-08 9z:2.4e-07 49z:9.7e-08 99z:7.8e-08
    fused/F3             0:6.9e-08 1:1.1e-07 3:1.1e-07 4z:9.8e-08 7z:7.7e-08 8:8.8e-08 9:9.5e-08 15:1.2e-07* 16z:9.5e-08* 49z:1.5e-07 99z:1.5e-07
    fused/F4             0:3.1e-08 1:6.0e-08 5:5.9e-08 6z:8.9e-08 7z:1.8e-07 8:1.6e-07 9:1.3e-07 32:2.5e-07* 33z:1.7e-07 49z:1.6e-07 99z:1.1e-07
    fused/F5             0:4.1e-08 1:1.1e-07 3:2.1e-07 4z:2.0e-07 9z:4.9e-07 49z:3.7e-07 99z:7.6e-07
    carried/F1           0:4.7e-08 1:1.2e-07 2:2.0e-07 3z:1.9e-07 9z:2.0e-07 49z:1.6e-07 99z:1.9e-07
    carried/F2           0:7.3e-08 1:1.3e-07 4:1.1e-07 5z:9.4e-08 9z:2.9e-07 49z:1.3e-07 99z:7.5e-08
    carried/F3           0:6.9e-08 1:1.1e-07 3:1.1e-07 4z:7.7e-08 7z:7.7e-08 8:8.8e-08 9:9.5e-08 15:7.8e-08* 16z:9.5e-08* 49z:4.7e-08 99z:3.0e-08
    carried/F4           0:3.1e-08 1:6.0e-08 5:5.9e-08 6z:8.9e-08 7z:2.2e-07 8:1.6e-07 9:1.3e-07 32:5.5e-07* 33z:4.1e-07 49z:1.7e-07 99z:1.7e-07
    carried/F5           0:4.1e-08 1:1.1e-07 3:2.3e-07 4z:2.3e-07 9z:6.4e-07 49z:4.3e-07 99z:3.7e-07
    carried-bf16/F3      0:6.9e-08 1:2.6e-08 3:9.5e-08 4z:5.4e-08 7z:4.9e-08 8:7.4e-08 9:9.0e-08 15:1.0e-07* 16z:9.0e-08* 49z:1.0e-07 99z:3.8e-08
    carried-f16/F3       0:6.9e-08 1:4.4e-08 3:6.5e-08 4z:9.0e-08 7z:9.2e-08 8:1.1e-07 9:1.6e-07 15:7.4e-08* 16z:6.3e-08* 49z:6.3e-08 99z:6.3e-08
    carried-csr/F1       0:4.7e-08 1:1.2e-07 2:2.1e-07 3z:1.9e-07 9z:2.0e-07 49z:1.8e-07 99z:2.2e-07
    carried-csr/F3       0:6.9e-08 1:1.1e-07 3:1.1e-07 4z:7.7e-08 7z:7.7e-08 8:8.8e-08 9:9.5e-08 15:5.6e-08* 16z:9.5e-08* 49z:3.7e-08 99z:1.7e-08
    sweep/F1             0:4.7e-08 1:1.2e-07 2:2.0e-07 3z:1.9e-07 9z:2.1e-07 49z:1.6e-07 99z:2.2e-07
    sweep/F3             0:6.9e-08 1:1.1e-07 3:1.1e-07 4z:7.7e-08 7z:7.7e-08 8:7.4e-08 9:7.0e-08 15:1.2e-07* 16z:9.5e-08* 49z:1.5e-07 99z:1.5e-07
    sweep/F4             0:3.1e-08 1:6.0e-08 5:5.7e-08 6z:1.0e-07 7z:2.3e-07 8:1.2e-07 9:1.7e-07 32:2.1e-07* 33z:1.7e-07 49z:1.6e-07 99z:1.3e-07
    sweep/F5             0:4.1e-08 1:1.1e-07 3:1.6e-07 4z:2.1e-07 9z:5.4e-07 49z:3.7e-07 99z:5.2e-07
    sweep-nofold/F3      0:6.9e-08 1:1.1e-07 3:1.1e-07 4z:7.7e-08 7z:7.7e-08 8:7.4e-08 9:7.0e-08 15:1.2e-07* 16z:9.5e-08* 49z:1.5e-07 99z:1.5e-07
    sweep-bf16/F3        0:6.9e-08 1:2.6e-08 3:1.1e-07 4z:5.4e-08 7z:7.6e-08 8:7.4e-08 9:1.1e-07 15:1.0e-07* 16z:9.0e-08* 49z:8.0e-08 99z:4.9e-08
    sweep-f16/F3         0:6.9e-08 1:4.4e-08 3:6.5e-08 4z:9.0e-08 7z:9.0e-08 8:5.8e-08 9:4.4e-08 15:7.5e-08* 16z:9.3e-08* 49z:4.7e-08 99z:4.3e-08
    sweep-tiled/F3       0:6.9e-08 1:1.1e-07 3:9.3e-08 4z:7.7e-08 7z:7.7e-08 8:5.9e-08 9:7.0e-08 15:1.2e-07* 16z:9.5e-08* 49z:1.5e-07 99z:1.5e-07
    sweep-tiled/F4       0:2.6e-08 1:6.0e-08 5:1.3e-07 6z:2.7e-07 7z:3.1e-07 8:1.3e-07 9:1.1e-07 32:3.7e-07* 33z:2.3e-07 49z:8.6e-08 99z:1.3e-07
    batch/F6-ok          0:6.8e-08 1:8.6e-08 9:1.6e-07 49:1.4e-07 99:1.2e-07
    batch/F6-infeasible  0:3.3e-08 1:3.3e-08 4:5.7e-08 5z:8.1e-08 9z:1.9e-07 49z:1.5e-07 99z:1.1e-07
    batch/F6-unbounded   0:7.3e-08 1:1.3e-07 4:1.1e-07 5z:9.4e-08 9z:2.4e-07 49z:9.8e-08 99z:8.6e-08

Scratch builds with one arithmetic change in the tau = 0 arm of one site (none committed; NOTEBOOK.md, section 15.1), cases of
this file failing out of 64:
    post_k    p = xs - s    27: test 1 on every reference / fused / carried leg and the batch, the verdict test on F2, F4 and the batch
    sw_cone_k p = ns - hx    5: test 1 on the five form-2 legs (sweep, -nofold, -bf16, -f16, -tiled on F3)
    sweep_k   d = g3 + c    13: test 1 and the verdict test on the dense sweep legs of F1, F3, F5; ExcessIter on sweep-F3
    sp_col_k  d = g3 + c     2: test 1 and the verdict test on sweep-tiled-F3
Each fails only legs that run the changed site.  The earlier suite (the 326 cases of the files that run the solver loops) is not
blind to a wrong p: on the post_k build 5 of its cases fail (the unbounded LP of tests/lp.rs ends ExcessIter on reference / fused /
carried and in test_sweep_infeasible_and_unbounded_certificates, and test_schedules_agree_at_the_full_socp_size, whose n = 50 000
instance has tau = 0 at the iteration it compares), on the sw_cone_k build 1 (that last test: one cross-schedule comparison of cri,
cri_infeas = inf there, so d is not seen).  It was not run on the sweep_k and sp_col_k builds.
Cost (--durations): 64 cases in 5.6 s; the slowest call 0.35 s (the trait-level Solver on F1)."""
import numpy as np
import pytest

import tau_zero_problems as Z
from test_gpu_bf16 import bf16_round, f16_quantize

pytestmark = pytest.mark.gpu

PASSES = {"reference": 6, "fused": 3, "carried": 2, "sweep": 1}

# leg: (schedule, a_storage, form of A, families, the m-tail form per family)
#   form of A: "dense", "csr" (two CSR copies: finished products, nT < 0 in post_k), "tiled" (the tiled sparse copy: sp_col_k)
LEGS = {
    "reference":    ("reference", "f32", "dense", ("F1", "F2", "F3", "F4", "F5"), {}),      # post_k, ycrit_k, status_k, xupdate_k's clamp
    "fused":        ("fused", "f32", "dense", ("F1", "F2", "F3", "F4", "F5"), {}),
    "carried":      ("carried", "f32", "dense", ("F1", "F2", "F3", "F4", "F5"), {}),
    "carried-bf16": ("carried", "bf16", "dense", ("F3",), {}),                              # the same on the 16-bit GEMV
    "carried-f16":  ("carried", "f16", "dense", ("F3",), {}),
    "carried-csr":  ("carried", "f32", "csr", ("F1", "F3"), {}),
    "sweep":        ("sweep", "f32", "dense", ("F1", "F3", "F4", "F5"), {"F1": 1, "F3": 2, "F4": 3, "F5": 3}),   # sweep_k, sw_xm_k, sw_cone_k,
                                                                                            # sw_vm_k, folded status_eval, sw_tau_k
    # status_k with tau_next as its own launch, asked for through inject_sweep_fault(5).  The library reports nothing from which a
    # test could tell that the termination test was NOT folded (tests/test_gpu_sweep.py has the same gap): if the hook did nothing,
    # this leg would pass as a copy of sweep/F3
    "sweep-nofold": ("sweep", "f32", "dense", ("F3",), {"F3": 2}),
    "sweep-bf16":   ("sweep", "bf16", "dense", ("F3",), {"F3": 2}),                         # sweep_k<bf16>
    "sweep-f16":    ("sweep", "f16", "dense", ("F3",), {"F3": 2}),                          # sweep_k<f16>
    "sweep-tiled":  ("sweep", "f32", "tiled", ("F3", "F4"), {"F3": 2, "F4": 7}),            # sp_col_k, sw_xm_k<FLAT>
}
CASES = [(leg, fam) for leg, v in LEGS.items() for fam in v[3]]
EXCESS_CASES = [("fused", "F1"), ("carried", "F5"), ("sweep", "F3"), ("sweep-tiled", "F4")]


@pytest.fixture(scope="module")
def T():
    import totsu_amd
    from totsu_amd import _lib
    _lib.init()
    return totsu_amd


def _dense(fam):
    from totsu_amd.problem import _Dense
    return _Dense(*fam.args())


_PLANS = {}


def _plan(fam_name, a_storage):
    """the oracle's plan on the matrix the leg streams: the family's own, or its 16-bit rounding (computed once, shared)"""
    if a_storage == "f32":
        return Z.plan(fam_name)
    key = (fam_name, a_storage)
    if key not in _PLANS:
        fam = Z.family(fam_name)
        if a_storage == "bf16":
            mat = bf16_round(fam.mat_a).astype(np.float64)
        else:
            mat = np.asfortranarray(f16_quantize(fam.A)[2]).ravel(order="F")
        _PLANS[key] = Z.oracle_plan(fam, mat_a=mat)
    return _PLANS[key]


def _solver(T, leg, fam, param):
    schedule, a_storage, form, _, _ = LEGS[leg]
    if form == "csr":
        import scipy.sparse as sp
        fs = T.FusedSolver(fam.n, fam.m, sp.csr_matrix(fam.A), fam.vec_b, fam.vec_c, fam.seg_type, fam.seg_len, param, schedule,
                           sparse_two_copies=True, gemv_autotune=False)
    else:
        kw = {"a_layout": "tiled"} if form == "tiled" else {}
        fs = T.FusedSolver.from_dense(_dense(fam), param, schedule, a_storage=a_storage, sweep_min_bytes=0, gemv_autotune=False, **kw)
    if leg == "sweep-nofold":
        fs.inject_sweep_fault(5)
    return fs


def _assert_path(fs, leg, fam):
    schedule, a_storage, form, _, _ = LEGS[leg]
    assert fs.schedule_in_use() == schedule, (leg, fam.name, fs.schedule_in_use())
    assert fs.a_storage == a_storage
    passes, bpp = fs.passes()
    if form == "dense":
        assert passes == PASSES[schedule] and bpp == fam.m * fam.n * (4 if a_storage == "f32" else 2), (leg, fam.name, passes, bpp)
        assert fs.a_layout == "dense" and fs._spt is None and fs._csr is None
    elif form == "csr":
        assert fs._csr is not None and fs._spt is None and passes == 2 and bpp == 16 * int(np.count_nonzero(fam.A)), (leg, fam.name, passes, bpp)
    else:
        info = fs.sptile_info()
        assert fs.a_layout == "tiled" and passes == 2 and info["nnz"] == int(np.count_nonzero(fam.A)), (leg, fam.name, passes, info)
        if LEGS[leg][4][fam.name] == 7:
            assert info["slices_n"] <= 4, info           # the one-thread-per-row form of sw_xm_k


def _assert_mtail(fs, leg, fam):
    assert fs.kahan_terms()[1] == LEGS[leg][4].get(fam.name, 0), (leg, fam.name, fs.kahan_terms()[1])
    if LEGS[leg][0] == "sweep":
        assert fs.sweep_faults()["faults"] == 0


def _compare_snap(tag, fam, pl, it, x, y, st):
    """the iterate after iteration `it` against the oracle's; at a decisive snap also kind, criteria and tau == 0"""
    N = pl.N
    tol = fam.tol(it)
    rx, ry = pl.snaps[it][:N], pl.snaps[it][N:]
    sx, sy = max(np.abs(rx).max(), 1e-6), max(np.abs(ry).max(), 1e-6)
    ex, ey = np.abs(x - rx).max() / sx, np.abs(y - ry).max() / sy
    print("tau_zero %-22s it %2d kind %d %s err x %.2e y %.2e (tol %.0e) tau %.3e cri %s"
          % (tag, it, pl.kinds[it], "decisive" if pl.decisive[it] else "--------", ex, ey, tol, x[N - 1], tuple("%.3e" % c for c in st.cri)))
    assert ex <= tol and ey <= tol, (tag, it, ex, ey, tol)
    assert st.iters == it + 1 or st.iters == it, (tag, it, st.iters)
    if not pl.decisive[it]:
        return
    assert st.kind == pl.kinds[it], (tag, it, st.kind, pl.kinds[it])
    ncri = 3 if pl.kinds[it] == 0 else 2
    want, got = np.array(pl.cri[it][:ncri]), np.array(st.cri[:ncri])
    assert np.array_equal(np.isinf(want), np.isinf(got)), (tag, it, got, want)
    assert np.allclose(got, want, rtol=max(50 * tol, 1e-3), atol=1e-5), (tag, it, got, want)
    assert (x[N - 1] == 0.0) == (rx[N - 1] == 0.0), (tag, it, x[N - 1], rx[N - 1])
    if pl.kinds[it] == 1:
        assert x[N - 1] == 0.0 and y[-1] <= 0.0


@pytest.mark.parametrize("leg,fam_name", CASES)
def test_iterates_and_criteria_through_tau_zero(T, leg, fam_name):
    fam, pl = Z.family(fam_name), _plan(fam_name, LEGS[leg][1])
    before, ones, after = Z.counts(pl)                    # (the rounded matrices of the 16-bit legs have plans of their own)
    assert before >= 1 and ones >= 3 and (after >= 1 or not fam.flips_back), (leg, fam_name, before, ones, after)
    p = T.SolverParam()
    p.eps_acc = p.eps_inf = 1e-30
    fs = _solver(T, leg, fam, p)
    _assert_path(fs, leg, fam)
    done = 0
    for it in pl.chosen:
        fs.run(it + 1 - done, poll_every=64)
        done = it + 1
        x, y = fs.iterate()
        _compare_snap("%s/%s" % (leg, fam_name), fam, pl, it, x, y, fs.status())
    _assert_mtail(fs, leg, fam)
    assert fs.status().state == -1
    fs.destroy()


def test_batch_iterates_and_criteria_through_tau_zero(T):
    """three slots over one A in three regimes at once (bounded, infeasible, unbounded): the per-instance tails after
    dual_gemv_multi_k"""
    fams, pls = Z.family("F6"), Z.plan("F6")
    p = T.SolverParam()
    p.eps_acc = p.eps_inf = 1e-30
    bt = T.BatchSolver.from_dense(_dense(fams[0]), [f.vec_b for f in fams], [f.vec_c for f in fams], p, gemv_autotune=False)
    assert bt.info()["group_sizes"] == [3]
    done = 0
    for it in sorted(set(i for pl in pls for i in pl.chosen)):
        bt.run(it + 1 - done, poll_every=64)
        done = it + 1
        for q, (fam, pl) in enumerate(zip(fams, pls)):
            if it in pl.chosen:
                x, y = bt.iterate(q)
                _compare_snap("batch/%s" % fam.name, fam, pl, it, x, y, bt.status(q))
    # the slots are in different regimes at the end of the window
    assert [bt.status(q).kind for q in range(3)] == [0, 1, 1] == [pl.kinds[-1] for pl in pls]
    bt.destroy()


def _verdict_param(T):
    p = T.SolverParam()
    p.max_iter, p.eps_acc, p.eps_inf = 100_000, Z.EPS, Z.EPS
    return p


def _assert_unscaled_ending(tag, r, sol, iterate, fam, want_state, want_iters):
    x, y = iterate
    n, m = fam.n, fam.m
    margin = max(3, want_iters // 50)
    print("tau_zero verdict %-22s state %d at %d (oracle %d at %d, margin %d) kind %d cri %s"
          % (tag, r.state, r.iters, want_state, want_iters, margin, r.kind, tuple("%.3e" % c for c in r.cri)))
    assert r.state == want_state, (tag, r.state, want_state)
    assert abs(r.iters - want_iters) <= margin, (tag, r.iters, want_iters)
    assert r.kind == 1 and r.tau == 0.0 and x[n + 2 * m] == 0.0, (tag, r.kind, r.tau)
    assert r.cri[0 if want_state == Z.UNBOUNDED else 1] <= Z.EPS, (tag, r.cri)
    # finalize_k does not scale a kind-1 ending: the answer is the iterate's x_x, x_y bit for bit
    assert np.array_equal(sol[0], x[:n]) and np.array_equal(sol[1], x[n:n + m]), tag
    assert np.abs(sol[1]).max() > 0 or np.abs(sol[0]).max() > 0


@pytest.mark.parametrize("leg,fam_name", CASES)
def test_verdict_and_unscaled_ending(T, leg, fam_name):
    fam, pl = Z.family(fam_name), _plan(fam_name, LEGS[leg][1])
    assert pl.status == fam.verdict and pl.iters <= Z.MAX_VERDICT_ITER
    fs = _solver(T, leg, fam, _verdict_param(T))
    _assert_path(fs, leg, fam)
    r = fs.run(-1, poll_every=25)
    _assert_mtail(fs, leg, fam)
    _assert_unscaled_ending("%s/%s" % (leg, fam_name), r, fs.solution(), fs.iterate(), fam, pl.status, pl.iters)
    fs.destroy()


def test_batch_verdicts_and_endings(T):
    """the three slots end OK, Infeasible and Unbounded, each at its own iteration; the OK slot IS scaled by 1 / tau"""
    fams, pls = Z.family("F6"), Z.plan("F6")
    assert [pl.status for pl in pls] == [Z.OK, Z.INFEASIBLE, Z.UNBOUNDED]
    bt = T.BatchSolver.from_dense(_dense(fams[0]), [f.vec_b for f in fams], [f.vec_c for f in fams], _verdict_param(T),
                                  gemv_autotune=False)
    res = bt.run(-1, poll_every=25)
    n, m = fams[0].n, fams[0].m
    for q in (1, 2):
        _assert_unscaled_ending("batch/%s" % fams[q].name, res[q], bt.solution(q), bt.iterate(q), fams[q], pls[q].status, pls[q].iters)
    r, (x, y), (xs, ys) = res[0], bt.iterate(0), bt.solution(0)
    print("tau_zero verdict %-22s state %d at %d (oracle %d at %d) kind %d tau %.4f" % ("batch/F6-ok", r.state, r.iters, pls[0].status,
                                                                                     pls[0].iters, r.kind, r.tau))
    assert r.state == Z.OK and r.kind == 0 and abs(r.iters - pls[0].iters) <= max(3, pls[0].iters // 50)
    tau = x[n + 2 * m]
    assert r.tau == tau and 0.0 < tau < 1.0
    # finalize_k scales x_x, x_y in place by 1 / tau: the answer is the oracle's (which is scaled), not tau times it
    assert np.array_equal(xs, x[:n]) and np.array_equal(ys, x[n:n + m])
    ex, ey = np.abs(xs - pls[0].x).max() / np.abs(pls[0].x).max(), np.abs(ys - pls[0].y).max() / np.abs(pls[0].y).max()
    print("tau_zero verdict %-22s answer against the oracle's: x %.2e y %.2e (unscaled it would be off by %.2f)" % ("batch/F6-ok", ex, ey, 1 - tau))
    assert ex <= 1e-2 and ey <= 1e-2 and 1 - tau > 0.5, (ex, ey, tau)
    assert len({res[q].iters for q in range(3)}) == 3
    bt.destroy()


@pytest.mark.parametrize("fam_name", ["F1", "F3"])
def test_trait_level_solver_verdict(T, fam_name):
    """the ninth restatement: the Python trait-level Solver over the HIP backend (one L call per reference call)"""
    from totsu_amd.problem import _ConeList
    fam, pl = Z.family(fam_name), Z.plan(fam_name)
    L = T.F32HIP
    op_c = T.MatOp(L, T.MatType.General(fam.n, 1), fam.vec_c.copy())
    op_a = T.MatOp(L, T.MatType.General(fam.m, fam.n), fam.mat_a.copy())
    op_b = T.MatOp(L, T.MatType.General(fam.m, 1), fam.vec_b.copy())
    cones = {Z.CONE_ZERO: T.ConeZero, Z.CONE_RPOS: T.ConeRPos, Z.CONE_SOC: T.ConeSOC}
    cone = _ConeList([(cones[t](L), l) for t, l in zip(fam.seg_type, fam.seg_len)])
    s = T.Solver(L)
    s.fused = None
    s.param.max_iter, s.param.eps_acc, s.param.eps_inf = 100_000, Z.EPS, Z.EPS
    s.trace = []
    work = np.zeros(T.Solver.query_worklen(op_a.size()), dtype=np.float32)
    with pytest.raises(T.SolverError) as e:
        s.solve((op_c, op_a, op_b, cone, work))
    print("tau_zero verdict %-22s state %d at %d (oracle %d at %d)" % ("trait/" + fam_name, e.value.kind, s.iters, pl.status, pl.iters))
    assert e.value.kind == pl.status == fam.verdict
    assert abs(s.iters - pl.iters) <= max(3, pl.iters // 50), (s.iters, pl.iters)
    assert s.trace[-1][1] == 1
    for o in (op_c, op_a, op_b):
        o.drop()


@pytest.mark.parametrize("leg,fam_name", EXCESS_CASES)
def test_excess_iter_while_tau_is_zero(T, leg, fam_name):
    from totsu_amd._lib import E_INVALID, ThipError
    fam, pl = Z.family(fam_name), _plan(fam_name, LEGS[leg][1])
    # a decisive kind-1 snap; the latest one up to 49, so that tau has been 0 for a while (past every early flip back) and the
    # case still runs only 50 iterations twice
    i0 = max(i for i in pl.chosen if pl.decisive[i] and pl.kinds[i] == 1 and i <= 49)
    n, m, N = fam.n, fam.m, pl.N
    p = T.SolverParam()
    p.max_iter, p.eps_acc, p.eps_inf = i0 + 1, 1e-30, 1e-30
    fs = _solver(T, leg, fam, p)
    _assert_path(fs, leg, fam)
    runs = []
    for again in (False, True):
        if again:
            fs.reinit()
            assert fs.status().state == -1 and fs.status().iters == 0
        r = fs.run(-1, poll_every=16)
        x, y = fs.iterate()
        xs, ys = fs.solution()
        assert r.state == Z.EXCESS_ITER and r.kind == 1 and r.iters == i0, (leg, fam_name, r.state, r.kind, r.iters, i0)
        _compare_snap("excess %s/%s" % (leg, fam_name), fam, pl, i0, x, y, r)
        assert np.array_equal(xs, x[:n]) and np.array_equal(ys, x[n:n + m])          # unscaled, bit for bit
        with pytest.raises(ThipError) as e:
            fs.resume()
        assert e.value.code == E_INVALID
        assert fs.status().state == Z.EXCESS_ITER and fs.status().iters == i0         # the refusal changes nothing
        runs.append((x, y, xs, ys))
    _assert_mtail(fs, leg, fam)
    for a, b in zip(*runs):
        assert np.array_equal(a, b), (leg, fam_name)
    fs.destroy()
