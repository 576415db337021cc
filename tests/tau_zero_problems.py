"""Seeded infeasible / unbounded problems that drive the iteration through tau = 0 (criteria_inf, solver.rs:614-656), and the
selection of the iterations at which a test may compare the f32 device loop with the f64 oracle there.

Every family is returned as the fields totsu_amd.problem._Dense takes (Family.args()): n, m, column-major A, b, c, seg_type,
seg_len, in the stacked form  A x + s = b, s in K,  minimise c.x  (rows of a second-order cone: [-c_i^T ; -G_i], b = [d_i ; h_i];
of a PSD block: the packed upper triangle by columns, off-diagonal entries times sqrt(2), as ProbSDP.dense() lays it out).
A, b, c are f32 values; m % 4 == 0 and n >= 64 (the one-pass kernel takes the shape); A is random and unsymmetric.

numpy only; the oracle is imported where a function runs it."""
import contextlib
import types

import numpy as np

CONE_ZERO, CONE_RPOS, CONE_SOC, CONE_ROTSOC, CONE_PSD = 0, 1, 2, 3, 4
OK, UNBOUNDED, INFEASIBLE, EXCESS_ITER = 0, 1, 2, 3

MAX_VERDICT_ITER = 1500                       # every family reaches its verdict in the oracle within this many iterations
EPS = 1e-5                                    # eps_acc = eps_inf of the verdict runs
N_SNAP = 100                                  # snapshots 0 .. 99: where the project has iterate tolerances
BASE_SNAPS = (0, 1, 9, 49, 99)
TOLS_LP_SOCP = (2e-5, 1e-4, 2e-3)             # _check_iterates' ladder: up to iteration 1, up to 9, up to 99
TOLS_PSD = (5e-5, 3e-4, 3e-3)

# the width of each contradiction / the length of each unbounded objective (chosen on the oracle: tests/test_tau_zero_families_cpu.py)
F1_GAP, F2_SCALE, F3_GAP, F4_SCALE, F5_GAP, F6_GAP = 60.0, 10.0, 12.0, 4.0, 60.0, 20.0
F3_K, F3_FSCALE = 3.0, 3.0
LP_BIAS, SOC_BIAS, PSD_BIAS = 0.3, 2.0, 1.0
N_DUAL = 6                                     # rows with a positive multiplier in the bounded objective c = -A^T y0


class Family:
    def __init__(self, name, n, A, b, c, seg_type, seg_len, verdict, flips_back=False):
        A = np.asarray(A, np.float32)
        self.name, self.n, self.m = name, int(n), int(A.shape[0])
        assert A.shape == (self.m, self.n) and self.m % 4 == 0 and self.n >= 64 and sum(seg_len) == self.m
        self.A = A                                                      # (m, n), f32
        self.mat_a = np.asfortranarray(A).ravel(order="F")              # column-major, as _Dense holds it
        self.vec_b, self.vec_c = np.asarray(b, np.float32), np.asarray(c, np.float32)
        assert self.vec_b.shape == (self.m,) and self.vec_c.shape == (self.n,)
        self.seg_type, self.seg_len = [int(t) for t in seg_type], [int(l) for l in seg_len]
        self.verdict, self.flips_back = verdict, flips_back
        self.psd = CONE_PSD in self.seg_type

    def args(self):
        """positional arguments of totsu_amd.problem._Dense"""
        return self.n, self.m, self.mat_a, self.vec_b, self.vec_c, self.seg_type, self.seg_len

    def with_bc(self, name, b, c, verdict):
        return Family(name, self.n, self.A, b, c, self.seg_type, self.seg_len, verdict)

    def tol(self, it):
        t = TOLS_PSD if self.psd else TOLS_LP_SOCP
        return t[0] if it <= 1 else t[1] if it <= 9 else t[2]


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


# ---- LP over the layout [one zero-cone row a ; nonnegative rows G ; one more nonnegative row 2 a] ------------------------------

def _lp_layout(n, n_g, seed):
    rng = np.random.default_rng(seed)
    a = _f32(rng.standard_normal(n) / np.sqrt(n))
    w = rng.standard_normal(n)
    G = _f32(rng.standard_normal((n_g, n)) / np.sqrt(n) + LP_BIAS * np.outer(rng.uniform(0.5, 1.5, n_g), w / np.linalg.norm(w)))
    x0 = rng.standard_normal(n)
    slack = rng.uniform(0.1, 1.1, n_g + 1)
    last = 2.0 * a                                    # exact in f32; not equal to row 0, but in the same direction
    A = np.vstack([a, G, last])
    b_feas = np.concatenate([[a @ x0], G @ x0 + slack[:n_g], [last @ x0 + slack[n_g]]])
    y0 = np.zeros(n_g + 2)                            # in the dual cone (free, then >= 0), a few rows only
    y0[0] = rng.standard_normal()
    y0[rng.choice(np.arange(1, n_g + 1), N_DUAL, replace=False)] = rng.uniform(0.5, 1.5, N_DUAL)
    c_bounded = -(A.T @ y0)                            # A^T y0 + c = 0: dual feasible, so a feasible b gives a bounded problem
    return a, G, x0, A, b_feas, c_bounded


def _lp_infeasible_b(A, b_feas, x0, gap):
    """the last row asks  2 a.x <= 2 a.x0 - gap  while row 0 holds a.x = a.x0"""
    b = b_feas.copy()
    b[-1] = A[-1] @ x0 - gap
    return b


def _lp_unbounded_c(a, G, scale):
    """c = -scale r / |r| for the least-squares r with a.r = 0, G r = -1: x + t r stays feasible, c.r < 0"""
    M = np.vstack([a, G])
    r = np.linalg.lstsq(M, np.concatenate([[0.0], -np.ones(G.shape[0])]), rcond=None)[0]
    assert np.abs(M @ r - np.concatenate([[0.0], -np.ones(G.shape[0])])).max() < 1e-9
    return -scale * r / np.linalg.norm(r)


def f1(seed=1, gap=F1_GAP):
    """infeasible LP, 128 x 64: the sweep's merged m-tail (sw_xm_k<MERGE>)"""
    a, G, x0, A, b_feas, c = _lp_layout(64, 126, seed)
    return Family("F1", 64, A, _lp_infeasible_b(A, b_feas, x0, gap), c, [CONE_ZERO, CONE_RPOS], [1, 127], INFEASIBLE)


def f2(seed=2, scale=F2_SCALE):
    """unbounded LP, 64 x 64, over F1's layout"""
    a, G, x0, A, b_feas, _ = _lp_layout(64, 62, seed)
    return Family("F2", 64, A, b_feas, _lp_unbounded_c(a, G, scale), [CONE_ZERO, CONE_RPOS], [1, 63], UNBOUNDED)


def f6(seed=2, gap=F6_GAP, scale=F2_SCALE):
    """F2's matrix with three (b, c): bounded and feasible, infeasible (F1's contradictory last row), unbounded (F2's c)"""
    a, G, x0, A, b_feas, c_bounded = _lp_layout(64, 62, seed)
    base = Family("F6-ok", 64, A, b_feas, c_bounded, [CONE_ZERO, CONE_RPOS], [1, 63], OK)
    return [base, base.with_bc("F6-infeasible", _lp_infeasible_b(A, b_feas, x0, gap), c_bounded, INFEASIBLE),
            base.with_bc("F6-unbounded", b_feas, _lp_unbounded_c(a, G, scale), UNBOUNDED)]


# ---- second-order cones, built as problems.random_socp builds them ------------------------------------------------------------

def _soc_blocks(rng, n, cones, x0, bias=0.0, h_scale=1.0, margin=1.0):
    """rows [-c_i^T ; -G_i], b = [d_i ; h_i] of cones strictly feasible at x0 (by margin U(0.1, 1.1)), and the pairs (G_i, c_i);
    bias: the length of a direction common to every c_i (the feasible set is then unbounded along it)"""
    rows, bs, parts = [], [], []
    w = rng.standard_normal(n)
    w /= np.linalg.norm(w)
    for ni in cones:
        G = _f32(rng.standard_normal((ni, n)) / np.sqrt(n))
        h = _f32(h_scale * rng.standard_normal(ni))
        c = _f32(rng.standard_normal(n) / np.sqrt(n) + bias * rng.uniform(0.5, 1.5) * w)
        d = np.linalg.norm(G @ x0 + h) - c @ x0 + margin * rng.uniform(0.1, 1.1)
        rows += [-c.reshape(1, n), -G]
        bs += [[d], h]
        parts.append((G, c))
    return rows, bs, parts


def f3(seed=13, gap=F3_GAP, k=F3_K, fscale=F3_FSCALE, x_scale=0.015, margin=0.5, bias=SOC_BIAS):
    """infeasible SOCP, 256 x 96, every row in a plain second-order cone of at most 129 rows (the sweep's m-tail is sw_cone_k):
    the slack of the first cone (64 rows) is (-gap ; k x[:63]), never in the cone; then strictly feasible cones of 100, 20, 8, 64
    rows.  The objective is dual feasible for those four (as random_socp's) and long enough to pull tau to zero early, before the
    contradiction does for good; b is small next to the gap, so that t_tau b.v moves tau by a decisive amount."""
    n = 96
    rng = np.random.default_rng(seed)
    x0 = x_scale * rng.standard_normal(n)
    first = np.zeros((64, n))
    first[1:, :63] = -k * np.eye(63)                                    # s = b - A x = (-gap ; k x[:63])
    b_first = np.zeros(64)
    b_first[0] = -gap
    rows, bs, parts = _soc_blocks(rng, n, (99, 19, 7, 63), x0, bias, x_scale, margin)
    f = np.zeros(n)
    for G, c in parts:
        t = rng.uniform(0.5, 1.5)
        v = rng.standard_normal(G.shape[0])
        v *= 0.9 * t * rng.uniform(0, 1) / np.linalg.norm(v)
        f += t * c + G.T @ v
    return Family("F3", n, np.vstack([first] + rows), np.concatenate([b_first] + [np.ravel(v) for v in bs]), fscale * f,
                  [CONE_SOC] * 5, [64, 100, 20, 8, 64], INFEASIBLE, flips_back=True)


def f4(seed=4, scale=F4_SCALE):
    """unbounded SOCP, 160 x 200: a cone of 132 rows (more than 129: the three-launch m-tail), one of 20, 8 nonnegative rows;
    c = -scale r / |r| with G_i r = 0, c_i.r = 1 and P r = -1 on the nonnegative rows P"""
    n = 200
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal(n)
    rows, bs, parts = _soc_blocks(rng, n, [131, 19], x0)
    P = _f32(rng.standard_normal((8, n)) / np.sqrt(n))
    hp = P @ x0 + rng.uniform(0.1, 1.1, 8)
    M = np.vstack([parts[0][0], parts[1][0], parts[0][1], parts[1][1], P])
    rhs = np.concatenate([np.zeros(150), np.ones(2), -np.ones(8)])
    r = np.linalg.lstsq(M, rhs, rcond=None)[0]
    assert np.abs(M @ r - rhs).max() < 1e-9
    return Family("F4", n, np.vstack(rows + [P]), np.concatenate([np.ravel(v) for v in bs] + [hp]), -scale * r / np.linalg.norm(r),
                  [CONE_SOC, CONE_SOC, CONE_RPOS], [132, 20, 8], UNBOUNDED, flips_back=True)


# ---- PSD blocks -----------------------------------------------------------------------------------------------------------------

def svec(S):
    """symmetric matrix -> packed upper triangle by columns, off-diagonal entries times sqrt(2) (what ProbSDP.dense() holds)"""
    k = S.shape[0]
    return np.array([S[r, c] * (1.0 if r == c else np.sqrt(2.0)) for c in range(k) for r in range(c + 1)])


def f5(seed=5, gap=F5_GAP, n=64, bias=PSD_BIAS):
    """infeasible SDP, 588 x 64: PSD blocks of order 6 and 33 and 6 nonnegative rows; the slack of block i is
    -(sum_j x_j F_ij + F_in), and entry (0, 0) of the first is pinned at -gap (every F_0j has a zero there, F_0n has +gap)"""
    rng = np.random.default_rng(seed)
    x0 = rng.standard_normal(n)
    w = rng.standard_normal(n)
    w /= np.linalg.norm(w)
    cols, bs, c = [], [], np.zeros(n)
    for q, k in enumerate((6, 33)):
        Fs = []
        for j in range(n):
            B = rng.standard_normal((k, k)) / np.sqrt(n)
            Fs.append((B + B.T) / 2 + bias * w[j] * np.eye(k))
        if q == 0:
            for F in Fs:
                F[0, 0] = 0.0
        Fn = -np.eye(k) - sum(x * F for x, F in zip(x0, Fs))            # x0 strictly feasible for the block ...
        if q == 0:
            Fn[0, 0] = gap                                              # ... but for this entry
        B = rng.standard_normal((k, k))
        Y = B @ B.T / k + 0.1 * np.eye(k)
        c += np.array([-np.trace(F @ Y) for F in Fs])                   # dual feasible, as problems.random_sdp
        cols.append(np.stack([svec(F) for F in Fs], axis=1))
        bs.append(-svec(Fn))
    P = rng.standard_normal((6, n)) / np.sqrt(n)
    cols.append(P)
    bs.append(P @ x0 + rng.uniform(0.1, 1.1, 6))
    return Family("F5", n, np.vstack(cols), np.concatenate(bs), c / 2, [CONE_PSD, CONE_PSD, CONE_RPOS], [21, 561, 6], INFEASIBLE)


FAMILIES = {"F1": f1, "F2": f2, "F3": f3, "F4": f4, "F5": f5}
_MADE = {}


def family(name):
    """the family (built once and never changed); "F6" is the list of its three instances"""
    if name not in _MADE:
        _MADE[name] = f6() if name == "F6" else FAMILIES[name]()
    return _MADE[name]


# ---- the oracle's runs, and the snaps a comparison may use ---------------------------------------------------------------------

@contextlib.contextmanager
def _oracle():
    """the oracle with at most 8 threads (small problems: a handful beats every core of a big host); the setting is put back"""
    import oracle as O
    before = O.num_threads()
    if before > 8:
        O.set_num_threads(8)
    try:
        yield O
    finally:
        if before > 8:
            O.set_num_threads(before)


def oracle_verdict(fam, mat_a=None):
    with _oracle() as O:
        ro = O.solve_matop_cones(O.param(max_iter=100_000, eps_acc=EPS, eps_inf=EPS), fam.vec_c,
                                 fam.mat_a if mat_a is None else mat_a, fam.vec_b, fam.seg_type, fam.seg_len, use_ql=True)
    return ro.status, ro.iters, ro.x, ro.y


def oracle_plan(fam, mat_a=None, verdict=True):
    """the oracle's first N_SNAP iterations of one family as a namespace: snaps[i] (the iterate after iteration i), kinds[i],
    cri[i], tau[i], pre[i] (tau at iteration i before the clamp max(., 0)), decisive[i], flips, the chosen snaps, and the verdict
    run (status, iters, and the answer x, y it returns).  mat_a: another (rounded) column-major matrix in place of the family's"""
    n, m = fam.n, fam.m
    N = n + 2 * m + 1
    with _oracle() as O:
        ro = O.solve_matop_cones(O.param(max_iter=N_SNAP + 2, eps_acc=1e-30, eps_inf=1e-30), fam.vec_c,
                                 fam.mat_a if mat_a is None else mat_a, fam.vec_b, fam.seg_type, fam.seg_len,
                                 snap_iters=list(range(N_SNAP)), trace_cap=N_SNAP + 3, use_ql=True)
    assert len(ro.trace) >= N_SNAP and [t[0] for t in ro.trace[:N_SNAP]] == list(range(N_SNAP))
    pl = types.SimpleNamespace()
    pl.snaps, pl.precond, pl.N = ro.snaps, ro.precond, N
    pl.kinds = [t[1] for t in ro.trace[:N_SNAP]]
    pl.cri = [t[2:] for t in ro.trace[:N_SNAP]]
    pl.tau = ro.snaps[:, N - 1].copy()
    c, b = fam.vec_c.astype(np.float64), fam.vec_b.astype(np.float64)
    t_tau = ro.precond[N - 1]
    pl.pre = np.empty(N_SNAP)
    pl.pre[0] = 1.0                                                     # init_vecs: tau = 1, y = 0
    for k in range(N_SNAP - 1):
        y = ro.snaps[k][N:]
        pl.pre[k + 1] = pl.tau[k] + t_tau * (-(c @ y[:n]) - (b @ y[n:n + m]))
    pl.decisive = [bool(abs(pl.pre[i]) >= 10 * fam.tol(i) * (np.abs(ro.snaps[i][:N]).max() + np.abs(ro.snaps[i][N:]).max()))
                   for i in range(N_SNAP)]
    pl.flips = [i for i in range(1, N_SNAP) if pl.kinds[i] != pl.kinds[i - 1]]
    chosen = set(BASE_SNAPS)
    for f in pl.flips:
        chosen |= {f - 1, f}
    pl.chosen = sorted(chosen)
    pl.status, pl.iters, pl.x, pl.y = oracle_verdict(fam, mat_a) if verdict else (None, None, None, None)
    return pl


_PLANS = {}


def plan(name):
    """the plan of a family by name ("F6": the list of three), computed once and shared"""
    if name not in _PLANS:
        fam = family(name)
        _PLANS[name] = [oracle_plan(f) for f in fam] if name == "F6" else oracle_plan(fam)
    return _PLANS[name]


def counts(pl):
    """(decisive chosen snaps of kind 0 before the first of kind 1, of kind 1, of kind 0 after one of kind 1)"""
    first1 = pl.kinds.index(1) if 1 in pl.kinds else N_SNAP
    dec = [i for i in pl.chosen if pl.decisive[i]]
    return (sum(1 for i in dec if pl.kinds[i] == 0 and i < first1), sum(1 for i in dec if pl.kinds[i] == 1),
            sum(1 for i in dec if pl.kinds[i] == 0 and i > first1))
