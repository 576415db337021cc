"""numpy restatement, in f64, of the solver loop (solver.rs:460-612, as tests/state_numpy.py restates it) that takes a START: the
iterate (x, y) = ((x_x, x_y, x_s, tau), (u, v, kappa)) the loop begins from instead of x = 0, y = 0, tau = 1.  All five cones (the
projections are the oracle's own, oracle.proj), the preconditioner with product_group, and the termination test of solver.rs:381-451
(as thip_step.h's step_verdict states it).  It is validated on the CPU against the oracle's snapshots from the zero start and from
a snapshot (tests/test_warm_start_cpu.py), and is then the reference of the GPU tests for a start on a changed (b, c), for which the
oracle -- which has no start-iterate input -- offers nothing.  Test infrastructure (host logic), not a fallback of the product."""
import numpy as np

import oracle as O

ZERO, RPOS, SOC, ROT, PSD = 0, 1, 2, 3, 4
RUNNING, OK, UNBOUNDED, INFEASIBLE, EXCESS_ITER = -1, 0, 1, 2, 3      # THIP_ST_* (totsu_amd/_lib.py)


def _project(z, seg_type, seg_len, dual, eps_zero):
    off = 0
    for t, l in zip(seg_type, seg_len):
        if l:
            z[off:off + l] = O.proj(int(t), z[off:off + l], dual_cone=dual, eps_zero=eps_zero, use_ql=True)
        off += l
    assert off == z.size


class Problem:
    """(A, b, c, cone layout) with its norms and preconditioner (calc_norms, calc_precond: solver.rs:460-524)"""

    def __init__(self, A, b, c, seg_type, seg_len, b_rowabs=None, eps_zero=1e-12):
        f = np.float64
        self.A, self.b, self.c = np.asarray(A, f), np.asarray(b, f).ravel(), np.asarray(c, f).ravel()
        self.m, self.n = self.A.shape
        self.seg_type, self.seg_len, self.eps_zero = [int(t) for t in seg_type], [int(l) for l in seg_len], eps_zero
        m = self.m
        babs = np.abs(self.b) if b_rowabs is None else np.asarray(b_rowabs, f).ravel()

        def inv(t):
            return 1.0 / np.maximum(t, eps_zero)
        rowabs, colabs = np.abs(self.A).sum(axis=1), np.abs(self.A).sum(axis=0)
        self.Tx = inv(colabs + np.abs(self.c))                      # (sigma of u is tau of x_x)
        self.Ty, self.Ts, self.Sv = inv(rowabs + babs), inv(np.ones(m)), inv(rowabs + babs + 1.0)
        self.t_tau = self.s_kappa = 1.0 / max(np.abs(self.c).sum() + np.abs(self.b).sum(), eps_zero)
        off = 0
        for t, l in zip(self.seg_type, self.seg_len):               # product_group (solver.rs:509-523)
            if t >= SOC and l:
                self.Ty[off:off + l] = self.Ty[off:off + l].min()
                self.Ts[off:off + l] = self.Ts[off:off + l].min()
            off += l
        assert off == m
        self.norm_b, self.norm_c = np.linalg.norm(self.b), np.linalg.norm(self.c)

    @classmethod
    def of_dense(cls, d, **kw):
        """of a Prob*.dense()-like problem (mat_a column-major)"""
        A = np.asarray(d.mat_a, np.float64).reshape(d.n, d.m).T
        return cls(A, d.vec_b, d.vec_c, d.seg_type, d.seg_len, b_rowabs=getattr(d, "vec_b_rowabs", None), **kw)

    def zero_start(self):
        x, y = np.zeros(self.n + 2 * self.m + 1), np.zeros(self.n + self.m + 1)
        x[-1] = 1.0
        return x, y


class Run:
    """what run() returns: state, iters (the index of the last iteration executed), kind, cri, the final (x, y) and snaps
    {iteration index: (x, y)}"""


def run(p, steps, start=None, snap_iters=(), eps_acc=1e-30, eps_inf=1e-30, max_iter=None):
    """up to `steps` iterations of problem p from `start` (None: the zero start).  Iteration indices count from 0 at the start, as
    the device's do after set_iterate"""
    n, m, A, b, c, ez = p.n, p.m, p.A, p.b, p.c, p.eps_zero
    x, y = p.zero_start() if start is None else (np.asarray(start[0], np.float64).copy(), np.asarray(start[1], np.float64).copy())
    assert x.size == n + 2 * m + 1 and y.size == n + m + 1
    xx, xy, xs, tau = x[:n].copy(), x[n:n + m].copy(), x[n + m:n + 2 * m].copy(), x[-1]
    u, v, kappa = y[:n].copy(), y[n:n + m].copy(), y[-1]
    out = Run()
    out.state, out.iters, out.kind, out.cri, out.snaps = RUNNING, 0, 0, (0.0, 0.0, 0.0), {}
    for it in range(steps):
        ox, oy, os_, ot = xx, xy.copy(), xs.copy(), tau
        # x <- proj(x - T o K^T y)                                 (solver.rs:538-555)
        xx = xx + p.Tx * (A.T @ v + c * kappa)
        xy = xy + p.Ty * (b * kappa - A @ u)
        xs = xs + p.Ts * v
        tau = max(tau + p.t_tau * (-(c @ u) - (b @ v)), 0.0)
        _project(xy, p.seg_type, p.seg_len, True, ez)
        _project(xs, p.seg_type, p.seg_len, False, ez)
        rx, ry, rs, rt = ox - 2 * xx, oy - 2 * xy, os_ - 2 * xs, ot - 2 * tau
        # y <- y + S o K (x_k - 2 x_{k+1})                          (solver.rs:556-570)
        u = u + p.Tx * (-(A.T @ ry) - c * rt)
        v = v + p.Sv * (A @ rx + rs - b * rt)
        kappa = min(kappa + p.s_kappa * (c @ rx + b @ ry), 0.0)
        out.iters = it
        if it in snap_iters:
            out.snaps[it] = (np.concatenate([xx, xy, xs, [tau]]), np.concatenate([u, v, [kappa]]))
        excess = max_iter is not None and it + 1 >= max_iter
        if tau > ez:                                               # criteria_conv (solver.rs:573-612)
            pr, du = xs / tau - b + (A @ xx) / tau, c + (A.T @ xy) / tau
            gx, gy = (c @ xx) / tau, (b @ xy) / tau
            out.kind = 0
            out.cri = (np.linalg.norm(pr) / (1 + p.norm_b), np.linalg.norm(du) / (1 + p.norm_c), abs(gx + gy) / (1 + abs(gx) + abs(gy)))
            if max(out.cri) <= eps_acc:
                out.state = OK
            elif excess:
                out.state = EXCESS_ITER
        else:                                                      # criteria_inf (solver.rs:614-655)
            npr, ndu = np.linalg.norm(xs + A @ xx), np.linalg.norm(A.T @ xy)
            mcx, mby = -(c @ xx), -(b @ xy)
            out.kind = 1
            out.cri = (npr * p.norm_c / mcx if mcx > ez else np.inf, ndu * p.norm_b / mby if mby > ez else np.inf, 0.0)
            if out.cri[0] <= eps_inf:
                out.state = UNBOUNDED
            elif out.cri[1] <= eps_inf:
                out.state = INFEASIBLE
            elif excess:
                out.state = EXCESS_ITER
        if out.state != RUNNING:
            break
    out.x, out.y = np.concatenate([xx, xy, xs, [tau]]), np.concatenate([u, v, [kappa]])
    return out


def solution(r, n, m):
    """what solution() reads of a finished run: x_x / tau"""
    return r.x[:n] / r.x[-1]
