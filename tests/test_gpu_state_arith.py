"""GPU tests of the iterate's state arithmetic (thip_param.state_arith) on every kernel that carries it.

THIP_STATE_COMPENSATED (the default) keeps a Kahan term per entry of x_x, x_y, x_s, u and v.  A term is ~1e-8 of its entry:
the iterate-parity tests (2e-5 .. 2e-3 of the largest entry) and the bitwise-reproducibility tests pass with a term of the wrong
sign, one that is never read back, or one the compiler folded away.  The compensated add is written five times over (comp_add in
xupdate_k / ycrit_k; the same in sw_xm_k / sw_vm_k; cadd in sw_cone_k; sw_comp_add in sweep_k, three element types; open-coded in
sp_col_k).  Two tests, each on every path, each asserting the path that ran (schedule, stored form, passes and bytes, plan, and
the m-tail form the library reports through thip_test_solver_kahan):

1. test_compensated_state_lowers_the_f32_floor: WHERE THE ITERATE STAGNATES.  In plain f32 an update below half an ulp of its entry
   is lost and the dual criterion of the SOCPs below freezes at ~6e-6; with the terms it goes to ~1e-7.  tests/state_numpy.py
   restates the reference's loop in numpy f32 with and without the terms (tests/test_state_numpy_cpu.py pins it): dual criterion,
   plain / Kahan / f64,
       A = random_socp(200, [99] * 6, seed=1), 15 000 iterations:     6.23e-6 / 1.29e-7 / 3.5e-9   (matrix rounded to bf16:
                                                                      6.27e-6 / 8.9e-8, quantised as thip_to_f16: 6.26e-6 / 2.1e-7)
       B = random_socp(200, [99] * 5 + [129], seed=1), 20 000:        7.31e-6 / 1.20e-7 / 4.9e-10
   so: plain in (2e-6, 2e-5), compensated < 5e-7 and at most a tenth of plain (emulated ratio 27 - 70).
   WHAT THIS BINDS IS u's TERM ONLY.  The same emulation with the terms of single vectors removed (A, 15 000): only u kept 9.3e-8,
   x_x and u kept 9.7e-8, all but v 9.0e-8, all but x_s 1.2e-7, all but x_y 8.6e-8 -- as good as all five -- while u's term alone
   reversed gives 1.9e-6.  The floor is the stagnation of u; the primal criterion and the gap do not separate either (6e-8 in
   every variant, also evaluated in f64).  So every leg of this test checks the u update of its schedule (ycrit_k, sweep_k,
   sp_col_k), and the terms of x_y, x_s, v (the m-tail kernels) and of x_x are invisible to it.

2. test_compensated_update_of_the_running_solver_bit_for_bit: the terms of the m-vectors, read from the running solver.  After
   300 iterations the iterate, the preconditioner and the Kahan terms are read back, ONE more iteration runs, and they are read
   again.  x_s <- x_s + T_s o v has an increment the host knows exactly (a product of two f32 it has read), and its term is formed
   before the cone projection, so the new term of x_s must equal numpy's Fast2Sum
       y = f32(inc - k) ; t = f32(x_s + y) ; k' = f32(f32(t - x_s) - y)
   BIT FOR BIT (inc rounded on its own, or contracted into an fma with the subtraction: either, for the whole vector).  A term
   read with the wrong sign, not read, not written, or written from re-associated arithmetic fails it; x_y and v go through the
   same comp_add / cadd in the same kernel, but their increments hold f32 dot products the host cannot reproduce, so for v, u
   and x_x (no projection between the add and the store) the test checks what can be checked from outside: the stored term is
   the exact rounding error of the stored sum, k' = f32(f32(t - x) - y) and t = f32(x + y) for y = (t - x) - k'.  x_y's term
   (formed before a projection, from a dot product) is bound only through the function it shares with x_s.
   The u and x_x adds of sweep_k are checked bit for bit at kernel level (tests/test_gpu_sweep.py, tests/test_gpu_bf16.py).

Measured on an MI355X, dual criterion plain / compensated (test 1 prints all three criteria of every run):
    reference                      A, 15 000  6.33e-6 / 1.68e-7
    fused                          A, 15 000  6.33e-6 / 1.68e-7
    carried                        A, 15 000  6.27e-6 / 5.7e-8
    carried, a_storage="f16"       A, 15 000  6.26e-6 / 5.9e-8
    sweep (cone-wave m-tail)       A, 15 000  6.24e-6 / 6.8e-8
    sweep (three-launch m-tail)    B, 20 000  7.32e-6 / 3.70e-7
    sweep, bf16                    A, 15 000  6.27e-6 / 6.5e-8
    sweep, f16                     A, 15 000  6.26e-6 / 7.2e-8
    sweep, tiled sparse copy       A, 15 000  6.29e-6 / 5.9e-8
    sweep, tiled sparse copy       B, 20 000  7.38e-6 / 6.3e-8
Two legs on the tiled copy: on A the tiled copy's m-tail is sw_cone_k again (the library's rule does not look at the operator),
so B on the tiled copy is the case that reaches sw_xm_k<FLAT>.

Three scratch builds with one sign reversed (y = inc + k), every earlier test of the selection tried passing on all three: in
sw_cone_k's cadd test 1 passes on all ten legs and test 2 fails on the four cone-wave legs; in sw_comp_add test 1 fails on the four
dense sweep legs and the kernel-level bitwise tests fail; in comp_add test 1 fails on reference / fused / carried / carried-f16 and
test 2 on those and on both three-launch legs (NOTEBOOK.md, section 12.3).

Not here: the merged LP m-tail sw_xm_k<MERGE> in test 1 (no LP tried separates the two arithmetics within 300 000 iterations), and a
column-sharded leg (NOTEBOOK.md, section 12)."""
import numpy as np
import pytest

from state_numpy import socp_dense
from test_gpu_solver import _mb

pytestmark = pytest.mark.gpu

INSTANCES = {"A": (200, [99] * 6, 1),                  # every row in a cone of 100 rows: the one-launch cone-wave m-tail (sw_cone_k)
             "B": (200, [99] * 5 + [129], 1)}          # one cone of 130 rows: sw_xm_k + soc_k + sw_vm_k by the library's own rule

# id: (instance, iterations, schedule, a_storage, sparse) and the restatements of the compensated add the case runs
CASES = {
    "reference":          ("A", 15_000, "reference", "f32", False),      # comp_add in xupdate_k / ycrit_k
    "fused":              ("A", 15_000, "fused", "f32", False),          # the same, 3 passes
    "carried":            ("A", 15_000, "carried", "f32", False),        # the same, 2 passes
    "carried-f16":        ("A", 15_000, "carried", "f16", False),        # the same on the 16-bit GEMV
    "sweep-cone-wave":    ("A", 15_000, "sweep", "f32", False),          # sw_comp_add (sweep_k f32) + cadd (sw_cone_k)
    "sweep-three-launch": ("B", 20_000, "sweep", "f32", False),          # sw_comp_add + comp_add in sw_xm_k / sw_vm_k
    "sweep-bf16":         ("A", 15_000, "sweep", "bf16", False),         # sw_comp_add in sweep_k<bf16> + cadd
    "sweep-f16":          ("A", 15_000, "sweep", "f16", False),          # sw_comp_add in sweep_k<f16> + cadd
    "sweep-tiled":        ("A", 15_000, "sweep", "f32", True),           # sp_col_k's open-coded add + cadd
    "sweep-tiled-rows":   ("B", 20_000, "sweep", "f32", True),           # sp_col_k + comp_add in sw_xm_k<FLAT> / sw_vm_k
}

PASSES = {"reference": 6, "fused": 3, "carried": 2, "sweep": 1}


@pytest.fixture(scope="module")
def T():
    import totsu_amd
    from totsu_amd import _lib
    _lib.init()
    return totsu_amd


@pytest.fixture(scope="module")
def dense_of(T):
    """instance name -> the stacked dense description of ProbSOCP (built once, never changed)"""
    made, probs = {}, []

    def get(name):
        if name not in made:
            from problems import random_socp
            n, cones, seed = INSTANCES[name]
            f, Gs, hs, cs, d = random_socp(n, cones, seed=seed)
            socp = T.ProbSOCP(_mb(T, T.MatType.General(n, 1)).set_array(f.reshape(-1, 1)),
                              [_mb(T, T.MatType.General(G.shape[0], n)).set_array(G) for G in Gs],
                              [_mb(T, T.MatType.General(len(h_), 1)).set_array(h_.reshape(-1, 1)) for h_ in hs],
                              [_mb(T, T.MatType.General(n, 1)).set_array(c_.reshape(-1, 1)) for c_ in cs], d,
                              _mb(T, T.MatType.General(0, n)), _mb(T, T.MatType.General(0, 1)))
            dn = socp.dense()
            # the instance the emulation of tests/state_numpy.py runs is this one
            A, b, c, seg, babs = socp_dense(n, cones, seed)
            assert np.array_equal(np.asarray(dn.mat_a).reshape((dn.m, dn.n), order="F"), A)
            assert np.array_equal(dn.vec_b, b) and np.array_equal(dn.vec_c, c) and np.array_equal(dn.vec_b_rowabs, babs)
            assert [l for l in dn.seg_len if l] == [l for _, l in seg]
            made[name] = dn
            probs.append(socp)
        return made[name]
    yield get
    for q in probs:
        q.drop()


def _solver(T, dn, param, schedule, a_storage, sparse):
    if not sparse:
        # (the plan autotune off: the geometry, hence the order of the sums and the figure read after N iterations, is the same in every run)
        return T.FusedSolver.from_dense(dn, param, schedule, a_storage=a_storage, sweep_min_bytes=0, gemv_autotune=False)
    import scipy.sparse as sp
    A = sp.csc_matrix(np.asarray(dn.mat_a).reshape((dn.m, dn.n), order="F"))
    return T.FusedSolver(dn.n, dn.m, A, np.asarray(dn.vec_b, np.float32), np.asarray(dn.vec_c, np.float32), dn.seg_type, dn.seg_len,
                         param, schedule, vec_b_rowabs=dn.vec_b_rowabs)


def _assert_path(fs, dn, name, schedule, a_storage, sparse):
    """the case runs the kernels its name says: the schedule, the stored form, the passes over A and their bytes, the plan"""
    assert fs.schedule_in_use() == schedule, (name, fs.schedule_in_use())
    assert fs.a_storage == a_storage
    passes, bpp = fs.passes()
    if sparse:
        info = fs._spt.info()
        assert passes == 2 and bpp >= 8 * dn.m * dn.n and info["nnz"] == dn.m * dn.n, (name, passes, bpp, info)
        if name == "sweep-tiled-rows":
            # at most four slices per row block: the three-launch m-tail takes the one-thread-per-row form of sw_xm_k
            assert info["slices_n"] <= 4, info
    else:
        assert passes == PASSES[schedule] and bpp == dn.m * dn.n * (4 if a_storage == "f32" else 2), (name, passes, bpp)
    if schedule == "sweep":
        if not sparse:
            pl = fs.sweep_plan()
            assert pl["workgroups_per_column_group"] in (1, 2, 4, 8, 16, 32) and pl["columns_per_panel"] in (1, 2, 4), pl


# the m-tail form the library reports after a one-pass step (thip_test_solver_kahan): 2 a wave per cone, 3 three launches, + 4 one
# thread per row; 0: no one-pass step ran
MTAIL = {"sweep-cone-wave": 2, "sweep-bf16": 2, "sweep-f16": 2, "sweep-tiled": 2, "sweep-three-launch": 3, "sweep-tiled-rows": 7}


def _assert_mtail(fs, name):
    assert fs.kahan_terms()[1] == MTAIL.get(name, 0), (name, fs.kahan_terms()[1])


@pytest.mark.parametrize("name", list(CASES))
def test_compensated_state_lowers_the_f32_floor(T, dense_of, name):
    inst, iters, schedule, a_storage, sparse = CASES[name]
    dn = dense_of(inst)
    p = T.SolverParam()
    p.eps_acc = 0.0
    floors = {}
    for arith in ("plain", "compensated"):
        p.state_arith = arith
        fs = _solver(T, dn, p, schedule, a_storage, sparse)
        _assert_path(fs, dn, name, schedule, a_storage, sparse)
        r = fs.run(iters, poll_every=64)
        assert r.iters == iters and fs.schedule_in_use() == schedule, (name, arith, r.iters)
        if schedule == "sweep":
            assert fs.sweep_faults()["faults"] == 0
        _assert_mtail(fs, name)
        fs.destroy()
        print("state_arith floor %-18s %-11s cri = (%.3e, %.3e, %.3e)" % (name, arith, *r.cri))
        assert r.cri[0] < 1e-6 and r.cri[2] < 1e-6, (name, arith, r.cri)
        floors[arith] = r.cri[1]
    assert 2e-6 < floors["plain"] < 2e-5, (name, floors)
    assert floors["compensated"] < 5e-7, (name, floors)
    assert floors["compensated"] <= floors["plain"] / 10, (name, floors)


def _fast2sum(x, y):
    t = x + y
    return t, (t - x) - y


@pytest.mark.parametrize("name", list(CASES))
def test_compensated_update_of_the_running_solver_bit_for_bit(T, dense_of, name):
    inst, _, schedule, a_storage, sparse = CASES[name]
    dn = dense_of(inst)
    n, m = dn.n, dn.m
    p = T.SolverParam()
    p.eps_acc = 0.0
    fs = _solver(T, dn, p, schedule, a_storage, sparse)
    _assert_path(fs, dn, name, schedule, a_storage, sparse)
    fs.run(300, poll_every=300)
    (x0, y0), (k0, _) = fs.iterate(), fs.kahan_terms()
    Ts = fs.precond()[0][n + m:n + 2 * m]
    fs.run(1, poll_every=1)
    (x1, y1), (k1, form) = fs.iterate(), fs.kahan_terms()
    assert fs.status().iters == 301 and form == MTAIL.get(name, 0), (name, form)
    fs.destroy()
    xs0, v0 = x0[n + m:n + 2 * m], y0[n:n + m]
    assert all(a.dtype == np.float32 for a in (xs0, v0, Ts, k0["xs"]))
    # x_s: the increment is T_s o v, known exactly; the term is formed before the projection
    assert (k0["xs"] != 0).mean() > 0.5 and (v0 != 0).mean() > 0.9, name            # mid-solve: the terms are in use
    y_two = (Ts * v0) - k0["xs"]                                                   # product rounded, then the subtraction
    y_fma = (Ts.astype(np.float64) * v0.astype(np.float64) - k0["xs"].astype(np.float64)).astype(np.float32)      # one rounding
    want = [_fast2sum(xs0, y)[1] for y in (y_two, y_fma)]
    wrong_sign = _fast2sum(xs0, (Ts * v0) + k0["xs"])[1]
    assert (wrong_sign != want[0]).mean() > 0.3, name                              # the data tells the two signs apart
    miss = min(int((k1["xs"] != w).sum()) for w in want)
    print("state_arith x_s term %-18s entries differing from Fast2Sum: %d of %d (reversed sign would differ in %d)"
          % (name, miss, m, int((wrong_sign != want[0]).sum())))
    assert miss == 0, (name, miss)
    # v, u, x_x: no projection between the add and the store, so the stored term is the exact error of the stored sum
    for vec, old, new in (("v", v0, y1[n:n + m]), ("u", y0[:n], y1[:n]), ("xx", x0[:n], x1[:n])):
        kn = k1[vec]
        y = ((new.astype(np.float64) - old.astype(np.float64)) - kn.astype(np.float64)).astype(np.float32)
        ok = np.abs(old) >= np.abs(y)                                              # where Fast2Sum is error-free
        t, k = _fast2sum(old, y)
        assert ok.mean() > 0.9 and (kn != 0).mean() > 0.5, (name, vec, ok.mean())
        assert np.array_equal(t[ok], new[ok]) and np.array_equal(k[ok], kn[ok]), (name, vec, int((k[ok] != kn[ok]).sum()))
