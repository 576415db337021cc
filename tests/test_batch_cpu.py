"""CPU: what a batch of problems that share A (totsu_amd.BatchSolver, thip_batch_*) rests on and that needs no GPU -- how B
instances are grouped into multi-vector launches, and that instances iterated in lockstep over one operator do not interact."""
import numpy as np
import pytest

import oracle as O
from problems import benchmark_lp


@pytest.mark.parametrize("max_group", [8, 4, 2])
def test_grouping_for_every_batch_size(max_group):
    from totsu_amd.batch import group_sizes, kernel_instance
    for B in range(1, 65):
        g = group_sizes(B, max_group)
        # full groups first, the rest last; ceil(B / max_group) launches per pass
        assert g == [max_group] * (B // max_group) + ([B % max_group] if B % max_group else []), (B, g)
        assert len(g) == -(-B // max_group) and sum(g) == B
        # every group runs on the smallest kernel instance that holds it
        for members in g:
            inst = kernel_instance(members)
            assert inst in (1, 2, 4, 8) and inst >= members and (inst == 1 or inst // 2 < members)
    assert group_sizes(11) == [8, 3] and [kernel_instance(v) for v in group_sizes(11)] == [8, 4]
    assert group_sizes(1) == [1] and kernel_instance(1) == 1


def test_grouping_refuses_bad_arguments():
    from totsu_amd import _lib
    from totsu_amd.batch import group_sizes
    for B, g in ((0, 8), (65, 8), (4, 3), (4, 16)):
        with pytest.raises(_lib.ThipError) as e:
            group_sizes(B, g)
        assert e.value.code == _lib.E_INVALID


def _lockstep_lp(A, bs, cs, iters, eps_zero=1e-12):
    """The iteration on k instances at once, in f64: state vectors are the COLUMNS of n x k / m x k arrays, and every product with A
    is ONE matrix-matrix product for all instances (the carried schedule's two per iteration: stage X multiplies (u, v), stage C the
    new (x_x, x_y), and K rx follows by linearity from the carried products).  Nonnegative cone.  Returns {iteration: (x, y)} per
    instance in the layout of the oracle's snapshots."""
    m, n = A.shape
    k = len(bs)
    Bm, Cm = np.stack(bs, axis=1).astype(np.float64), np.stack(cs, axis=1).astype(np.float64)
    colabs, rowabs = np.abs(A).sum(axis=0)[:, None], np.abs(A).sum(axis=1)[:, None]          # once for all instances
    t_tau = np.abs(Cm).sum(axis=0) + np.abs(Bm).sum(axis=0)
    rec = lambda v: 1.0 / np.maximum(v, eps_zero)
    Tx, Ty, Ts, Tt = rec(colabs + np.abs(Cm)), rec(rowabs + np.abs(Bm)), rec(np.ones((m, k))), rec(t_tau)
    Su, Sv, Sk = Tx.copy(), rec(rowabs + np.abs(Bm) + 1.0), Tt.copy()
    xx, xy, xs, tau = np.zeros((n, k)), np.zeros((m, k)), np.zeros((m, k)), np.ones(k)
    u, v, kappa = np.zeros((n, k)), np.zeros((m, k)), np.zeros(k)
    gP, hP = A.T @ xy, A @ xx                       # the carried products of the start iterate
    out = [{} for _ in range(k)]
    for it in range(max(iters) + 1):
        g1, h1 = A.T @ v, A @ u                     # stage X: one read of A for all instances
        xx0, xy0, xs0, tau0 = xx, xy, xs, tau
        xx = xx + Tx * (g1 + Cm * kappa)
        xy = np.maximum(xy + Ty * (-h1 + Bm * kappa), 0.0)
        xs = np.maximum(xs + Ts * v, 0.0)
        tau = np.maximum(tau + Tt * (-(Cm * u).sum(axis=0) - (Bm * v).sum(axis=0)), 0.0)
        rxx, rxy, rxs, rtau = xx0 - 2 * xx, xy0 - 2 * xy, xs0 - 2 * xs, tau0 - 2 * tau
        g3, h3 = A.T @ xy, A @ xx                   # stage C: one read of A for all instances
        u = u + Su * (-(gP - 2 * g3) - Cm * rtau)   # A^T rx_y = A^T x_y_k - 2 A^T x_y_{k+1}
        v = v + Sv * ((hP - 2 * h3) + rxs - Bm * rtau)
        kappa = np.minimum(kappa + Sk * ((Cm * rxx).sum(axis=0) + (Bm * rxy).sum(axis=0)), 0.0)
        gP, hP = g3, h3
        if it in iters:
            for j in range(k):
                out[j][it] = (np.concatenate([xx[:, j], xy[:, j], xs[:, j], [tau[j]]]), np.concatenate([u[:, j], v[:, j], [kappa[j]]]))
    return out


def test_lockstep_instances_do_not_interact():
    """two instances iterated in lockstep over one A equal two independent f64 oracle solves to 1e-12 of the iterate's size"""
    _, G, _ = benchmark_lp(24, seed=1)
    A = G.astype(np.float64)
    m, n = A.shape
    bs, cs = [], []
    for i in range(2):
        rng = np.random.default_rng(i)
        cs.append(-rng.uniform(0, 1, n))
        bs.append(np.concatenate([np.zeros(n), rng.uniform(0, 1, n)]))
    iters = [0, 1, 9, 49]
    got = _lockstep_lp(A, bs, cs, iters)
    N = n + 2 * m + 1
    for j in range(2):
        ro = O.solve_matop_cones(O.param(max_iter=max(iters) + 2, eps_acc=1e-30), cs[j], A, bs[j], [O.CONE_RPOS], [m],
                                 snap_iters=iters, trace_cap=max(iters) + 3)
        for q, it in enumerate(iters):
            x, y = got[j][it]
            rx, ry = ro.snaps[q][:N], ro.snaps[q][N:]
            assert np.abs(x - rx).max() <= 1e-12 * max(np.abs(rx).max(), 1.0), (j, it, np.abs(x - rx).max())
            assert np.abs(y - ry).max() <= 1e-12 * max(np.abs(ry).max(), 1.0), (j, it, np.abs(y - ry).max())
    # and an instance alone gives bitwise what it gives beside another one: column j of a product does not depend on the others
    alone = _lockstep_lp(A, bs[:1], cs[:1], iters)
    for it in iters:
        assert np.abs(alone[0][it][0] - got[0][it][0]).max() <= 1e-13 and np.abs(alone[0][it][1] - got[0][it][1]).max() <= 1e-13
