"""GPU: every loop that projects on second-order and rotated second-order cones, on the layouts of tests/cone_layouts.py, iterate
by iterate against the f64 oracle.  The projection exists three times on the device -- soc_k (a wave or a block per cone; with the
second vector and rx <- rx - 2 x inside the loops), its copy in the one-launch m-tail of the one-pass schedule, and sb_soc of the
own-A batches -- around host code that turns seg_type / seg_len into tables.  tests/test_cone_layouts_cpu.py holds the condition
that makes these comparisons mean something: at the compared iterates the oracle itself takes all three branches of
cone_soc.rs:49-61 on every (cone type, length) of every layout, on the tau > 0 branch.  Iterates and tolerances are the project's
(tests/ownbatch_cases.py): 0, 1, 9, 99 at 2e-5, 2e-5, 1e-4, 2e-3, and with PSD blocks 0, 1, 9, 49 at 5e-5, 5e-5, 3e-4, 3e-3."""
import numpy as np
import pytest

import cone_layouts as CL
from ownbatch_cases import T, check_against_oracle  # noqa: F401  (T: the module fixture)

pytestmark = pytest.mark.gpu

ALL = list(CL.LAYOUTS)
SWEEP = ["mid", "short_soc", "short_soc_rot", "long", "psd_big"]


def _param(T):
    p = T.SolverParam()
    p.eps_acc = 1e-30
    return p


def _compare(label, i, it, tol, x, y, st, ro, q, N, iters_ok):
    """one iterate against the oracle's snapshot q, relative to the snapshot's max norm; status, kind and criteria there.  Returns
    the larger of the two errors"""
    rx, ry = ro.snaps[q][:N], ro.snaps[q][N:]
    sx, sy = max(np.abs(rx).max(), 1e-6), max(np.abs(ry).max(), 1e-6)
    ex, ey = np.abs(x - rx).max() / sx, np.abs(y - ry).max() / sy
    print("%s problem %d iterate %d: err x %.2e y %.2e (tol %.0e)" % (label, i, it, ex, ey, tol))
    assert ex <= tol and np.abs(x - rx).max() <= tol * sx, (label, i, it, ex)
    assert ey <= tol and np.abs(y - ry).max() <= tol * sy, (label, i, it, ey)
    assert st.state == -1 and st.iters in iters_ok, (label, i, it, st.state, st.iters)
    tr = ro.trace[it]
    assert st.kind == tr[1] == 0
    assert np.allclose(st.cri, tr[2:], rtol=max(50 * tol, 1e-3), atol=1e-5), (label, i, it, st.cri, tr)
    return max(ex, ey)


def _check_precond(label, i, t, s, ro, N):
    et, es = np.abs(t / ro.precond[:N] - 1).max(), np.abs(s / ro.precond[N:] - 1).max()
    print("%s problem %d preconditioner: rel err tau %.2e sigma %.2e" % (label, i, et, es))
    assert np.allclose(t, ro.precond[:N], rtol=2e-5, atol=0), (label, i, et)
    assert np.allclose(s, ro.precond[N:], rtol=2e-5, atol=0), (label, i, es)


def _check_fused(T, name, schedule, want_schedule=None, others=(), **kw):
    """one FusedSolver on the layout's first seed against its oracle; `others`: solvers advanced beside it, returned with it"""
    seed = CL.LAYOUTS[name]["seeds"][0]
    d, ro = CL.oracle(name, seed, 0, T=T)
    iters, tols = CL.iters_tols(name)
    label = "%s %s%s" % (name, schedule, " tiled" if kw.get("a_layout") == "tiled" else "")
    fs = T.FusedSolver.from_dense(d, _param(T), schedule, **kw)
    try:
        assert fs.schedule_in_use() == (want_schedule or schedule), (label, fs.schedule_in_use())
        if fs.schedule_in_use() == "sweep":
            assert fs.passes()[0] == (2 if kw.get("a_layout") == "tiled" else 1)      # (the tiled copy: one product launch each way)
        N = d.n + 2 * d.m + 1
        _check_precond(label, 0, *fs.precond(), ro, N)
        worst, done = [], 0
        for q, (it, tol) in enumerate(zip(iters, tols)):
            for f in (fs,) + tuple(others):
                f.run(it + 1 - done, poll_every=64)
            done = it + 1
            x, y = fs.iterate()
            worst.append(_compare(label, 0, it, tol, x, y, fs.status(), ro, q, N, (it + 1,)))
            for f in others:
                for u_, v_ in zip((x, y), f.iterate()):
                    assert np.abs(u_ - v_).max() <= 2e-6 * max(np.abs(v_).max(), 1e-6), (label, it)
                assert np.allclose(fs.status().cri, f.status().cri, rtol=1e-4, atol=1e-7)
        print("%s worst iterate errors at %s: %s" % (label, iters, " ".join("%.2e" % w for w in worst)))
        return fs.sptile_info(), fs.a_layout, np.count_nonzero(np.asarray(d.mat_a))
    finally:
        fs.destroy()
        for f in others:
            f.destroy()


@pytest.mark.parametrize("schedule", ["reference", "fused", "carried"])
@pytest.mark.parametrize("name", ALL)
def test_fused_solver_against_oracle(T, name, schedule):
    """reference: the stand-alone primitives; fused / carried: soc_batched2 with x_s beside x_y and rx <- rx - 2 x folded in (a block
    per cone on `long`), the PSD groups by order and the one-by-one orders above psd_small_max() on psd_big"""
    _check_fused(T, name, schedule, gemv_autotune=False)


@pytest.mark.parametrize("name", SWEEP)
def test_sweep_against_oracle(T, name):
    """the one-pass schedule at n >= 96 (sweep_min_bytes=0: whenever the kernel takes the shape): the three-launch m-tail with
    soc_batched2 and the rotated tables on mid / short_soc_rot / long / psd_big, the one-launch m-tail (a wave per cone) on short_soc"""
    _check_fused(T, name, "sweep", sweep_min_bytes=0, gemv_autotune=False)


def test_short_soc_one_launch_m_tail_is_its_three_launch_form(T):
    """short_soc again, beside a second solver held to the three-launch form (test hook): the iterates agree to round-off at every
    compared iterate, as tests/test_gpu_sweep.py::test_cone_wave_m_kernel_is_the_three_launch_form asks of its layout"""
    d, _ = CL.oracle("short_soc", CL.LAYOUTS["short_soc"]["seeds"][0], 0, T=T)
    b = T.FusedSolver.from_dense(d, _param(T), "sweep", sweep_min_bytes=0, gemv_autotune=False)
    b.inject_sweep_fault(3)                    # three launches
    _check_fused(T, "short_soc", "sweep", others=(b,), sweep_min_bytes=0, gemv_autotune=False)


@pytest.mark.parametrize("schedule", ["carried", "sweep"])
def test_tiled_copy_against_oracle(T, schedule):
    """mid with A held as the tiled sparse copy built on the device from the dense matrix"""
    info, layout, nnz = _check_fused(T, "mid", schedule, a_layout="tiled", gemv_autotune=False)
    assert layout == "tiled" and info is not None and info["nnz"] == nnz


@pytest.mark.parametrize("name", ["small", "long"])
def test_batch_solver_three_instances_over_one_a(T, name):
    """BatchSolver: the three instances of the layout's first seed (their own x0, s0, y0, so their own b and c) over one A, each
    against its own oracle"""
    seed = CL.LAYOUTS[name]["seeds"][0]
    runs = [CL.oracle(name, seed, inst, T=T) for inst in CL.LAYOUTS[name]["instances"]]
    assert len(runs) == 3
    d0 = runs[0][0]
    assert all(np.array_equal(d.mat_a, d0.mat_a) and not np.array_equal(d.vec_b, d0.vec_b) for d, _ in runs[1:])
    iters, tols = CL.iters_tols(name)
    label = "%s batch" % name
    bt = T.BatchSolver.from_dense(d0, [d.vec_b for d, _ in runs], [d.vec_c for d, _ in runs], _param(T), gemv_autotune=False)
    try:
        N = d0.n + 2 * d0.m + 1
        for i, (_, ro) in enumerate(runs):
            _check_precond(label, i, *bt.precond(i), ro, N)
        worst, done = [0.0] * len(iters), 0
        for q, (it, tol) in enumerate(zip(iters, tols)):
            bt.run(it + 1 - done, poll_every=64)
            done = it + 1
            for i, (_, ro) in enumerate(runs):
                x, y = bt.iterate(i)
                worst[q] = max(worst[q], _compare(label, i, it, tol, x, y, bt.status(i), ro, q, N, (it, it + 1)))
        print("%s worst iterate errors at %s: %s" % (label, iters, " ".join("%.2e" % w for w in worst)))
    finally:
        bt.destroy()


FAMILY = {"small": ("SmallBatchSolver", (64, 256, 1024)), "mid": ("MidBatchSolver", (256, 1024)), "psd": ("SdpBatchSolver", (256, 1024))}


def _own_a(T, name):
    runs = [CL.oracle(name, seed, 0, T=T) for seed in CL.LAYOUTS[name]["seeds"]]
    assert len(runs) == 4
    return [d for d, _ in runs], [ro for _, ro in runs]


def _check_conic_batch(T, name, label, **kw):
    """conic_batch's own choice (asserted), then the family's comparison with the oracle (check_against_oracle)"""
    ds, ros = _own_a(T, name)

    class ViaConicBatch:
        @staticmethod
        def from_dense(denses, param, **kw_):
            sb = T.conic_batch(denses, param, **kw_)
            if type(sb) is not getattr(T, FAMILY[name][0]):
                sb.destroy()
                raise AssertionError("%s went to %s" % (name, type(sb).__name__))
            return sb

    iters, tols = CL.iters_tols(name)
    return check_against_oracle(T, ViaConicBatch, label, ds, ros, iters, tols, **kw)


@pytest.mark.parametrize("name,threads", [(n, t) for n in FAMILY for t in FAMILY[n][1]])
def test_conic_batch_at_every_workgroup_size(T, name, threads):
    """four problems per layout, each with its own A, through sb_soc at every workgroup size the family's test hook takes"""
    info = _check_conic_batch(T, name, "%s own-A %d threads" % (name, threads), force_threads=threads)
    assert info["threads"] == threads


@pytest.mark.parametrize("name", list(FAMILY))
def test_conic_batch_plain_state_arithmetic(T, name):
    """once with plain f32 iterate updates, at the family's own workgroup size"""
    _check_conic_batch(T, name, "%s own-A plain" % name, state_arith="plain")
