"""numpy restatement of the solver loop (solver.rs:460-612: calc_norms, calc_precond with product_group, the x / y updates
and criteria_conv) in a chosen floating-point type, with optional Kahan terms on the five iterate vectors x_x, x_y, x_s, u, v
in the arithmetic of comp_add (totsu_amd/csrc/thip_solver_kernels.inc): what thip_param.state_arith switches on the device.
It tells where the plain f32 iterate stagnates and where the compensated one does, so that the GPU tests of the state
arithmetic (tests/test_gpu_state_arith.py) have bounds that do not come from the kernels under test.  Test infrastructure
(host logic), not a fallback of the product."""
import numpy as np

from problems import random_socp

CONE_ZERO, CONE_RPOS, CONE_SOC = 0, 1, 2


def socp_dense(n, cones, seed):
    """problems.random_socp stacked as ProbSOCP.dense() stacks it (socp.rs:88-93): rows of cone i are [-c_i^T ; -G_i],
    b = [d_i ; h_i], and the row sums of the preconditioner take the signed d_i (socp.rs:271).
    Returns (A (m x n), b, c, [(cone type, rows)], b_rowabs)."""
    f, Gs, hs, cs, d = random_socp(n, cones, seed=seed)
    rows, b, babs, seg = [], [], [], []
    for G, h, c, di in zip(Gs, hs, cs, d):
        rows += [-c.reshape(1, -1), -G]
        b += [[di], h]
        babs += [[di], np.abs(h)]
        seg.append((CONE_SOC, 1 + G.shape[0]))
    return (np.vstack(rows).astype(np.float32), np.concatenate(b).astype(np.float32), f.astype(np.float32), seg,
            np.concatenate(babs).astype(np.float32))


def _project(z, seg, dual, dt):
    off = 0
    for ty, ln in seg:
        s = z[off:off + ln]
        if ty == CONE_ZERO:
            if not dual:
                s[:] = 0
        elif ty == CONE_RPOS:
            np.maximum(s, 0, out=s)
        elif ln:                                                   # cone_soc.rs:38-65
            t, nrm = s[0], dt(np.linalg.norm(s[1:].astype(np.float64)))
            if nrm <= -t:
                s[:] = 0
            elif nrm > t:
                s[1:] *= (dt(1) + t / nrm) / dt(2)
                s[0] = (nrm + t) / dt(2)
        off += ln


def criteria_after(A, b, c, seg, iters, dtype=np.float32, kahan=False, b_rowabs=None, eps_zero=1e-12, iterate=False):
    """`iters` iterations from x = 0, tau = 1 in `dtype`; returns criteria_conv's triple (primal, dual, gap) of the last
    iterate (None while tau <= eps_zero).  seg: [(cone type, rows)] over the m rows; kahan: a compensation term per entry
    of x_x, x_y, x_s, u, v, updated as  y = inc - k ; t = x + y ; k = (t - x) - y  (tau and kappa stay plain, as on the device);
    a collection of names out of "xx", "xy", "xs", "u", "v" keeps the terms of those vectors only (what a kernel that lost
    the others would compute).  iterate=True: returns (criteria, dict of the iterate's vectors and tau, kappa) instead."""
    dt = np.dtype(dtype).type
    A, b, c = (np.asarray(a).astype(dt) for a in (A, b, c))
    m, n = A.shape
    babs = np.abs(b) if b_rowabs is None else np.asarray(b_rowabs).astype(dt)

    def inv(t):
        return (dt(1) / np.maximum(t, dt(eps_zero))).astype(dt)
    rowabs, colabs = np.abs(A).sum(axis=1).astype(dt), np.abs(A).sum(axis=0).astype(dt)
    Tx = Su = inv(colabs + np.abs(c))
    Ty, Ts, Sv = inv(rowabs + babs), np.ones(m, dt), inv(rowabs + babs + dt(1))
    t_tau = s_kappa = dt(1) / max(dt(np.abs(c).sum() + babs.sum()), dt(eps_zero))
    off = 0
    for ty, ln in seg:                                             # product_group (solver.rs:509-523)
        if ty >= CONE_SOC and ln:
            Ty[off:off + ln] = Ty[off:off + ln].min()
            Ts[off:off + ln] = Ts[off:off + ln].min()
        off += ln
    assert off == m
    norm_b, norm_c = np.linalg.norm(b.astype(np.float64)), np.linalg.norm(c.astype(np.float64))
    xx, xy, xs, u, v = (np.zeros(k, dt) for k in (n, m, m, n, m))
    tau, kappa = dt(1), dt(0)
    K = {name: np.zeros(k, dt) for name, k in dict(xx=n, xy=m, xs=m, u=n, v=m).items()}
    comp = set(K) if kahan is True else set(kahan or ())
    assert comp <= set(K)

    def add(name, x, inc):
        inc = inc.astype(dt)
        if name not in comp:
            return (x + inc).astype(dt)
        y = (inc - K[name]).astype(dt)
        t = (x + y).astype(dt)
        K[name] = ((t - x).astype(dt) - y).astype(dt)
        return t
    cri = None
    for _ in range(iters):
        ox, oy, os_, ot = xx, xy.copy(), xs.copy(), tau
        # x <- proj(x - T o K^T y)                                 (solver.rs:538-555)
        xx = add("xx", xx, Tx * (A.T @ v + c * kappa))
        xy = add("xy", xy, Ty * (b * kappa - A @ u))
        xs = add("xs", xs, Ts * v)
        tau = max(dt(tau + t_tau * (-(c @ u) - (b @ v))), dt(0))
        _project(xy, seg, True, dt)
        _project(xs, seg, False, dt)
        rx, ry, rs, rt = ox - 2 * xx, oy - 2 * xy, os_ - 2 * xs, ot - 2 * tau
        # y <- y + S o K (x_k - 2 x_{k+1})                          (solver.rs:556-570)
        u = add("u", u, Su * (-(A.T @ ry) - c * rt))
        v = add("v", v, Sv * (A @ rx + rs - b * rt))
        kappa = min(dt(kappa + s_kappa * (c @ rx + b @ ry)), dt(0))
        if tau > eps_zero:                                         # criteria_conv (solver.rs:573-612)
            p = xs / tau - b + (A @ xx) / tau
            d = c + (A.T @ xy) / tau
            gx, gy = float(c @ xx) / float(tau), float(b @ xy) / float(tau)
            cri = (np.linalg.norm(p.astype(np.float64)) / (1 + norm_b), np.linalg.norm(d.astype(np.float64)) / (1 + norm_c),
                   abs(gx + gy) / (1 + abs(gx) + abs(gy)))
    if iterate:
        return cri, dict(xx=xx, xy=xy, xs=xs, u=u, v=v, tau=tau, kappa=kappa)
    return cri
