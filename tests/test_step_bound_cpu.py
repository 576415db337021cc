"""CPU: the one-step bound of tests/step_bound.py before any kernel is held to it.  A plain f32 numpy evaluation of the step with
sequential sums passes check() on every input and start and uses at most a quarter of the bound; six planted errors in that f32
step are each rejected, and the first three of them are errors the suite's former check of one iteration from a snapshot
(tests/warm_cases.py::iterate_tol(1) = 2e-5 of the iterate's max norm) lets through -- the first two at every start, the third
(a whole row's dot product, which does not shrink with the row's scale) at one of twelve seeds and starts, all twelve recorded;
the starts hold what they are there for: every branch of the block-cone projection on layout_small_s, and tau == 0."""
import numpy as np
import pytest

import cone_layouts as CL
import step_bound as SB
from step_bound import EPS, F, PSD, ROT, RPOS, SOC, ZERO

QUARTER = 0.25


# ---- the step in f32 ------------------------------------------------------------------------------------------------------------

def _seq(M, axis):
    """sums along an axis in f32, one term after the other"""
    M = np.asarray(M, F)
    if M.shape[axis] == 0:
        return np.zeros(np.delete(M.shape, axis), F)
    return np.cumsum(M, axis=axis, dtype=F).take(-1, axis=axis)


def _dot(a, b):
    return _seq(a * b, 0)


def _soc32(z):
    if z.size == 0:
        return z
    t, nrm = z[0], np.sqrt(_seq(z[1:] * z[1:], 0))
    if nrm <= -t:
        return np.zeros_like(z)
    if nrm <= t:
        return z
    out = z.copy()
    out[1:] *= (F(1) + t / nrm) / F(2)
    out[0] = (nrm + t) / F(2)
    return out


def _rot32(z):
    if z.size == 1:
        return np.maximum(z, F(0))
    s2 = np.sqrt(F(2))
    w = z.copy()
    w[0], w[1] = (z[0] + z[1]) / s2, (z[0] - z[1]) / s2
    w = _soc32(w)
    r, s = w[0], w[1]
    w[0], w[1] = (r + s) / s2, (r - s) / s2
    return w


def _psd32(z):
    k = int(round((np.sqrt(8 * z.size + 1) - 1) / 2))
    cols, rows = np.nonzero(np.tri(k, dtype=bool))               # (c, r) with r <= c, by columns: the packing of svec
    scale = np.where(rows == cols, F(1), np.sqrt(F(2))).astype(F)
    S = np.zeros((k, k), F)
    S[rows, cols] = z / scale
    S[cols, rows] = z / scale
    w, Z = np.linalg.eigh(S)
    P = ((Z * np.maximum(w, F(0))) @ Z.T).astype(F)
    return (P[rows, cols] * scale).astype(F)


def _project32(z, seg_type, seg_len, dual):
    off = 0
    for t, l in zip(seg_type, seg_len):
        s = slice(off, off + l)
        if t == ZERO:
            if not dual:
                z[s] = 0
        elif t == RPOS:
            z[s] = np.maximum(z[s], F(0))
        elif l:
            z[s] = {SOC: _soc32, ROT: _rot32, PSD: _psd32}[t](z[s].copy())
        off += l


class P32:
    """the problem and its preconditioner in f32 (tests/state_numpy.py's, with sequential sums)"""

    def __init__(self, d, eps_zero=1e-12):
        self.A = np.asarray(d.mat_a, F).reshape(d.n, d.m).T.copy()
        self.b, self.c = np.asarray(d.vec_b, F), np.asarray(d.vec_c, F)
        self.m, self.n, self.seg_type, self.seg_len, self.ez = d.m, d.n, d.seg_type, d.seg_len, eps_zero
        babs = np.abs(self.b) if d.vec_b_rowabs is None else np.asarray(d.vec_b_rowabs, F)

        def inv(t):
            return (F(1) / np.maximum(t, F(eps_zero))).astype(F)
        rowabs, colabs = _seq(np.abs(self.A), 1), _seq(np.abs(self.A), 0)
        self.Tx = inv(colabs + np.abs(self.c))
        self.Ty, self.Ts, self.Sv = inv(rowabs + babs), np.ones(d.m, F), inv(rowabs + babs + F(1))
        self.t_tau = F(1) / max(F(_seq(np.abs(self.c), 0) + _seq(np.abs(self.b), 0)), F(eps_zero))
        off = 0
        for t, l in zip(self.seg_type, self.seg_len):
            if t >= SOC and l:
                self.Ty[off:off + l] = self.Ty[off:off + l].min()
                self.Ts[off:off + l] = self.Ts[off:off + l].min()
            off += l
        self.norm_b, self.norm_c = np.sqrt(_dot(self.b, self.b)), np.sqrt(_dot(self.c, self.c))


def f32_step(q, x32, y32, plant=None, arg=None):
    """one iteration in f32; plant: one of the planted errors below -> (x, y, kind, cri)"""
    n, m, A, b, c = q.n, q.m, q.A, q.b, q.c
    x32, y32 = np.asarray(x32, F), np.asarray(y32, F)
    xx, xy, xs, tau = x32[:n].copy(), x32[n:n + m].copy(), x32[n + m:n + 2 * m].copy(), x32[-1]
    u, v, kappa = y32[:n].copy(), y32[n:n + m].copy(), y32[-1]
    ox, oy, os_, ot = xx, xy.copy(), xs.copy(), tau
    terms = A * v[:, None]
    if plant == "drop_ATv":                                    # one row's term left out of A^T v
        terms[arg[0], arg[1]] = 0
    Au = _seq(A * u[None, :], 1)
    if plant == "drop_last_row_Au":                            # the remainder row of an odd m
        Au[m - 1] = 0
    xx = xx + q.Tx * (_seq(terms, 0) + c * kappa)
    xy = xy + q.Ty * (b * kappa - Au)
    xs = xs + q.Ts * v
    tau = tau + q.t_tau * (-_dot(c, u) - _dot(b, v))
    if plant != "no_tau_clamp":
        tau = max(tau, F(0))
    raw = {"xy": xy.copy(), "xs": xs.copy()}
    _project32(xy, q.seg_type, q.seg_len, True)
    _project32(xs, q.seg_type, q.seg_len, False)
    if plant == "soc_tail_unscaled":                           # one tail entry of a block that is scaled to the boundary
        which, row = arg
        (xy if which == "xy" else xs)[row] = raw[which][row]
    two = F(2)
    rx, ry, rs, rt = ox - two * xx, oy - two * xy, os_ - two * xs, ot - two * tau
    u = u + q.Tx * (-_seq(A * ry[:, None], 0) - c * rt)
    v = v + q.Sv * (_seq(A * rx[None, :], 1) + rs - b * rt)
    if plant == "kappa_reads_x_next":                          # x_{k+1} instead of x_k - 2 x_{k+1}
        kappa = min(kappa + q.t_tau * (_dot(c, xx) + _dot(b, xy)), F(0))
    else:
        kappa = min(kappa + q.t_tau * (_dot(c, rx) + _dot(b, ry)), F(0))
    with np.errstate(all="ignore"):
        if tau > q.ez:
            pr, du = xs / tau - b + _seq(A * xx[None, :], 1) / tau, c + _seq(A * xy[:, None], 0) / tau
            gx, gy = _dot(c, xx) / tau, _dot(b, xy) / tau
            kind, cri = 0, (np.sqrt(_dot(pr, pr)) / (1 + q.norm_b), np.sqrt(_dot(du, du)) / (1 + q.norm_c), abs(gx + gy) / (1 + abs(gx) + abs(gy)))
        else:
            pr, du = xs + _seq(A * xx[None, :], 1), _seq(A * xy[:, None], 0)
            mcx, mby = -_dot(c, xx), -_dot(b, xy)
            kind = 1
            cri = (np.sqrt(_dot(pr, pr)) * q.norm_c / mcx if mcx > q.ez else np.inf,
                   np.sqrt(_dot(du, du)) * q.norm_b / mby if mby > q.ez else np.inf, 0.0)
    return (np.concatenate([xx, xy, xs, [tau]]).astype(F), np.concatenate([u, v, [kappa]]).astype(F), kind, tuple(float(t) for t in cri))


# ---- the f32 step passes, with room ---------------------------------------------------------------------------------------------

_P32 = {}


def _q(name):
    if name not in _P32:
        _P32[name] = P32(SB.problem(name))
    return _P32[name]


def _all_starts():
    out = [(name, "k=%d" % k, None) for name in SB.NAMES for k in SB.ks_of(name)]
    return out + [(name, label, None) for name in SB.TAU_ZERO for label in ("before", "zero", "back")]


def _start(name, label):
    if label.startswith("k="):
        return SB.start(name, int(label[2:]))
    found = [s for lb, _, s in SB.tau_zero_starts(name) if lb == label]
    return found[0] if found else None


@pytest.mark.parametrize("name", SB.NAMES + SB.TAU_ZERO)
def test_f32_step_uses_a_quarter_of_the_bound(name):
    labels = [lb for nm, lb, _ in _all_starts() if nm == name]
    d, worst = SB.problem(name), 0.0
    for label in labels:
        st = _start(name, label)
        if st is None:                                         # (tau does not return within the window: F1, F2, F6)
            assert label == "back" and name not in ("F3", "F4")
            continue
        x, y, kind, cri = f32_step(_q(name), *st)
        ratios = SB.check(d, st, x, y, kind, cri)
        print("one step in f32, %s %s: %s" % (name, label, SB.fmt(ratios)))
        w = max(max(ratios[k] for k in ("x_x", "x_y", "x_s", "tau")), max(ratios[k] for k in ("u", "v", "kappa")) / SB.Y_FACTOR)
        worst = max(worst, w)
    print("one step in f32, %s: worst share of the bound %.4f" % (name, worst))
    assert worst <= QUARTER, (name, worst)


def test_tau_zero_occurs_among_the_starts():
    zeros = [(name, label) for name, label, _ in _all_starts() if _start(name, label) is not None and _start(name, label)[0][-1] == 0.0]
    print("starts with tau == 0: %s" % zeros)
    assert len([z for z in zeros if z[1] == "zero"]) == len(SB.TAU_ZERO)
    for name in ("F3", "F4"):                                  # tau returns, and is positive again at `back`
        assert _start(name, "back")[0][-1] > 0.0
    # and the step from `before` clamps: the reference's tau after it is exactly 0
    for name in SB.TAU_ZERO:
        assert SB.reference_step(SB.problem(name), *_start(name, "before"))[0][-1] == 0.0, name


def test_every_projection_branch_on_the_layout():
    seen = {"y": set(), "s": set()}
    for k in SB.KS:
        st = _start("layout_small_s", "k=%d" % k)
        rx = SB.reference_step(SB.problem("layout_small_s"), *st)[0]
        here = {}
        for _, kind, l, which, br in CL.branches("small", rx):
            if l > 1:
                here.setdefault(which, set()).add(br)
                seen[which].add(br)
        print("layout_small_s after the step from k = %d: branches of x_y %s, of x_s %s" % (k, sorted(here["y"]), sorted(here["s"])))
        assert here["y"] | here["s"] >= {"zero", "inside", "boundary"}, (k, here)
    assert "outside" not in seen["y"] | seen["s"]


# ---- planted errors -----------------------------------------------------------------------------------------------------------------

def _judge(tag, d, st, x, y, kind=None, cri=None):
    ratios, fails = SB.violations(d, st, x, y, kind, cri)
    old = SB.old_check_passes(d, st, x, y)
    print("planted %-28s new check: %s (%s); the former 2e-5 of the max norm: %s" % (tag, "REJECTED" if fails else "passed", SB.fmt(ratios), "passed" if old else "rejected"))
    return bool(fails), old


def _smallest_B(d, st):
    Bx, _ = SB.bounds(d, *st)
    assert all(t < SOC for t in d.seg_type)                    # every component of x is held componentwise
    cand = np.where(Bx > 0, Bx, np.inf)
    i = int(np.argmin(cand))
    return i, Bx[i]


@pytest.mark.parametrize("k", SB.KS)
def test_planted_small_component(k):
    name = "lp80x40s"
    d, st = SB.problem(name), _start(name, "k=%d" % k)
    x, y, kind, cri = f32_step(_q(name), *st)
    i, B = _smallest_B(d, st)
    x = x.copy()
    x[i] = F(np.float64(x[i]) + 1e-4 * B)
    rx = SB.reference_step(d, *st)[0]
    print("planted 1e-4 B in x[%d]: B = %.3e, %.1e of the iterate's max norm" % (i, B, 1e-4 * B / np.abs(rx).max()))
    rejected, old = _judge("1e-4 B_i, smallest B_i, k=%d" % k, d, st, x, y, kind, cri)
    assert rejected and old


@pytest.mark.parametrize("k", SB.KS)
def test_planted_dropped_row_of_ATv(k):
    name = "lp80x40s"
    d, st = SB.problem(name), _start(name, "k=%d" % k)
    p = SB.f64_problem(d)
    v = np.abs(SB.parts(p, *st)[5])
    Bx, _ = SB.bounds(d, *st)
    term = p.Tx[None, :] * np.abs(p.A) * v[:, None]            # what row i adds to component j of x_x
    # the smallest term that the bound must still see: above EPS B_j by the quarter the f32 evaluation itself may use
    need = (1 + QUARTER) * EPS * Bx[None, :d.n]
    cand = np.where(term > need, term, np.inf)
    i, j = np.unravel_index(int(np.argmin(cand)), cand.shape)
    assert np.isfinite(cand[i, j])
    print("planted dropped term: row %d of column %d, %.2f EPS B_j" % (i, j, term[i, j] / (EPS * Bx[j])))
    x, y, kind, cri = f32_step(_q(name), *st, plant="drop_ATv", arg=(i, j))
    rejected, old = _judge("row left out of A^T v, k=%d" % k, d, st, x, y, kind, cri)
    assert rejected and old


def test_planted_dropped_last_row_of_an_odd_m():
    # what this error is next to the iterate's max norm depends on the scales the last row and the columns drew: the former check sees
    # it on most seeds.  Every seed and start must be rejected by the bound; the seeds and starts the former check lets through are
    # recorded, and there is at least one
    name, passed_old = "lp157x157s", []
    for seed in range(4):
        d, q = SB.problem(name, seed), P32(SB.problem(name, seed))
        assert d.m % 2 == 1
        for k in SB.KS:
            st = SB.start(name, k, seed)
            x, y, kind, cri = f32_step(q, *st, plant="drop_last_row_Au")
            rejected, old = _judge("last row left out of A u, seed %d k=%d" % (seed, k), d, st, x, y, kind, cri)
            assert rejected, (seed, k)
            if old:
                passed_old.append((seed, k))
    print("planted last row left out of A u: the former check passes (seed, k) = %s" % passed_old)
    assert passed_old


def _scaled_block(name):
    """(start label, 'xy' / 'xs', first row, rows) of the longest second-order block where a step's projection scales it to the
    boundary, at the start where it is scaled the most (alpha the furthest from 1)"""
    d = SB.problem(name)
    p = SB.f64_problem(d)
    l = max(l_ for t, l_ in zip(d.seg_type, d.seg_len) if t == SOC)
    q = [i for i, (t, l_) in enumerate(zip(d.seg_type, d.seg_len)) if t == SOC and l_ == l][0]
    off = int(np.sum(d.seg_len[:q]))
    best = None
    for k in SB.KS:
        xx, xy, xs, tau, u, v, kappa = SB.parts(p, *_start(name, "k=%d" % k))
        for which, z in (("xy", xy + p.Ty * (p.b * kappa - p.A @ u)), ("xs", xs + p.Ts * v)):
            t, nrm = z[off], np.linalg.norm(z[off + 1:off + l])
            if nrm > abs(t):                                   # cone_soc.rs:49-61: the third branch
                alpha = (1 + t / nrm) / 2
                if best is None or 1 - alpha > best[0]:
                    best = (1 - alpha, "k=%d" % k, which, off, l, z)
    assert best is not None, name
    return best[1:]


def test_planted_unscaled_tail_entry():
    name = "socp102x12s"
    label, which, off, l, z = _scaled_block(name)
    d, st = SB.problem(name), _start(name, label)
    row = off + 1 + int(np.argmax(np.abs(z[off + 1:off + l])))
    x, y, kind, cri = f32_step(_q(name), *st, plant="soc_tail_unscaled", arg=(which, row))
    rejected, _ = _judge("unscaled tail entry (%s row %d, %s)" % (which, row, label), d, st, x, y, kind, cri)
    assert rejected


@pytest.mark.parametrize("name", SB.TAU_ZERO)
def test_planted_tau_not_clamped(name):
    d, st = SB.problem(name), _start(name, "before")
    x, y, kind, cri = f32_step(_q(name), *st, plant="no_tau_clamp")
    assert x[-1] < 0
    rejected, _ = _judge("tau not clamped, %s" % name, d, st, x, y, kind, cri)
    assert rejected


@pytest.mark.parametrize("name,k", [("lp80x40s", 9), ("socp102x12s", 9), ("socp102x12s", 99)])
def test_planted_kappa_reads_x_next(name, k):
    # (not from k = 99 on of lp80x40s: there c.x + b.y has cancelled to 1.2 and 1.5 EPS B_kappa, and kappa moves by less than the
    # Y_FACTOR EPS B_kappa it is held to -- no bound made of absolute values sees an error in a sum that has cancelled that far)
    d, st = SB.problem(name), _start(name, "k=%d" % k)
    x, y, kind, cri = f32_step(_q(name), *st, plant="kappa_reads_x_next")
    rejected, _ = _judge("kappa from x_{k+1}, %s k=%d" % (name, k), d, st, x, y, kind, cri)
    assert rejected


@pytest.mark.parametrize("k", [99, 999])
def test_planted_kappa_reads_x_next_where_the_sum_has_cancelled(k):
    """the blind spot, pinned: on lp80x40s from k = 99 on the plant moves kappa by more than EPS B_kappa and less than the
    Y_FACTOR EPS B_kappa it is held to, so neither check sees it.  If this fails, the blind spot has moved"""
    name = "lp80x40s"
    d, st = SB.problem(name), _start(name, "k=%d" % k)
    x, y, kind, cri = f32_step(_q(name), *st, plant="kappa_reads_x_next")
    ratios, fails = SB.violations(d, st, x, y, kind, cri)
    rejected, old = _judge("kappa from x_{k+1}, %s k=%d" % (name, k), d, st, x, y, kind, cri)
    assert not rejected and old and not fails
    assert 1.0 < ratios["kappa"] <= SB.Y_FACTOR, ratios["kappa"]
