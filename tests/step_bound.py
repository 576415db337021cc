"""One iteration of the solver loop held to a componentwise f32 bound that does not grow with the iteration count, the inputs that
make it bite, and the starts deep in a solve.  A plain module, like tests/warm_cases.py: numpy and the oracle, no device
(tests/test_step_bound_cpu.py validates it on the CPU; tests/test_gpu_one_step.py uses it on every loop).

The bound.  One iteration from the start (x, y) = ((x_x, x_y, x_s, tau), (u, v, kappa)), held in f32, is computed in f64 by
tests/warm_numpy.py (reference_step).  Every component i of the result is a sum of terms; B_i is the sum of their absolute values
(bounds), and a correct f32 evaluation differs from the f64 one by a small multiple of u B_i, u = 2^-24, whatever the iteration
count and however small component i is next to the iterate's max norm.  check() asserts, with EPS = 1e-5:

    |d_i| <= EPS B_i                        x_x, tau, rows of the zero and nonnegative cones (the clamp is 1-Lipschitz per component)
    ||d_blk||_2 <= EPS ||B_blk||_2 + T_CONE max|reference blk|
                                            a second-order, rotated or PSD block (the projection is non-expansive, so this holds
                                            across a change of branch)
    |d_i| <= Y_FACTOR EPS B_i               u, v, kappa: the second half's own rounding costs EPS B and it reads x_k - 2 x_{k+1},
                                            which carries at most 2 EPS B of the first half's error
    kind == the reference's                 unless the reference tau lies within EPS B_tau of eps_zero
    criteria: rtol 1e-3, atol 1e-5          what every oracle comparison of the suite holds them to

The three constants and their sources -- none is fitted to what a kernel returns:
    EPS = 1e-5      the componentwise constant the project holds its products to (1e-5 |A||x| in tests/test_gpu_batch.py and
                    tests/test_gpu_gemv_tilings.py): 168 u, against the 2 u a plain f32 evaluation needs
    Y_FACTOR = 3    1 + 2, as derived above
    T_CONE = 2e-5   the projection tolerance of the primitive tests: tests/test_gpu_primitives.py for the second-order and the
                    rotated cone, test_psd_projection of tests/test_gpu_sdpbatch.py / tests/test_gpu_eig.py for the PSD cone

B, from absolute values only (T_x, T_y, T_s, S_v, t_tau, s_kappa: the preconditioner):
    B_xx = |x_x| + T_x (|A|^T |v| + |c| |kappa|)        B_xy = |x_y| + T_y (|b| |kappa| + |A| |u|)
    B_xs = |x_s| + T_s |v|                              B_tau = |tau| + t_tau (|c|.|u| + |b|.|v|)
and with |r| <= |x_k| + 2 B for r = x_k - 2 x_{k+1}:
    B_u = |u| + T_x (|A|^T (|x_y| + 2 B_xy) + |c| (|tau| + 2 B_tau))
    B_v = |v| + S_v (|A| (|x_x| + 2 B_xx) + (|x_s| + 2 B_xs) + |b| (|tau| + 2 B_tau))
    B_kappa = |kappa| + s_kappa (|c|.(|x_x| + 2 B_xx) + |b|.(|x_y| + 2 B_xy))

The inputs (problem(name, seed)).  The `s` variants are scaled in f64 before the rounding to f32: rows by 10^U(-3, 3) -- a block
cone gets one factor for the whole cone, so that a point of the cone stays in it -- and columns by 10^U(-3, 3); b = A x0 + s0 and
c = -A^T y0 are then rebuilt from the scaled A as tests/ownbatch_cases.py::_edge builds them, s0 strictly inside the cone and y0
strictly inside its dual (the layout of tests/cone_layouts.py keeps its own complementary x0, s0, y0, which send its block cones
through all three branches of the projection).  A matrix stored in 16 bits is another matrix: the problem handed to
reference_step and bounds is the widened one (with_matrix).

The starts (start(name, k, seed)): the f64 restatement's own iterate after k = 9, 99, 999 iterations from the zero start, rounded
to f32; and of the tau -> 0 families F1-F4, F6 of tests/tau_zero_problems.py (tau_zero_starts) the iterate just before tau first
clamps to 0, the first iterate with tau == 0, and for F3 and F4 the first iterate after tau returns.  Every f64 run is computed once
per session and never changed."""
import copy
import zlib

import numpy as np

import warm_numpy as W
from ownbatch_cases import F, _D

ZERO, RPOS, SOC, ROT, PSD = 0, 1, 2, 3, 4
EPS, Y_FACTOR = 1e-5, 3.0
T_CONE = {SOC: 2e-5, ROT: 2e-5, PSD: 2e-5}
CRI_RTOL, CRI_ATOL = 1e-3, 1e-5
KS = (9, 99, 999)
NAMES = ("lp80x40s", "lp157x157s", "lp2504x1252s", "socp102x12s", "layout_small_s", "sdp45x6", "sdp561x6", "sp40x30s")
TAU_ZERO = ("F1", "F2", "F3", "F4", "F6-infeasible", "F6-unbounded")       # (F6-ok never clamps: tests/test_gpu_tau_zero.py)
TAU_ZERO_WINDOW = 100


def ks_of(name):
    """the k's of an input's starts (lp2504x1252s: 9 and 99 only, to keep the CPU time down)"""
    return KS[:2] if name.startswith("lp2504x1252") else KS


# ---- the inputs ---------------------------------------------------------------------------------------------------------------

def _rng(name, seed, what):
    return np.random.default_rng([zlib.crc32(name.encode()), int(seed), int(what)])


def scaled(name, seed, A, seg_type, seg_len, point=None):
    """the `s` variant of (A, cones): R A C with R = diag(10^U(-3, 3)), one factor per block cone, C = diag(10^U(-3, 3)), in f64;
    b = A' x0 + s0, c = -A'^T y0 from point = (x0, s0, y0), or a point drawn as tests/sparse_cases.py::problem_of draws it"""
    from sparse_cases import interior
    A = np.asarray(A, np.float64)
    m, n = A.shape
    rng = _rng(name, seed, 0)
    rows, off = np.empty(m), 0
    for t, l in zip(seg_type, seg_len):
        rows[off:off + l] = 10.0 ** rng.uniform(-3, 3) if t >= SOC else 10.0 ** rng.uniform(-3, 3, l)
        off += l
    assert off == m
    cols = 10.0 ** rng.uniform(-3, 3, n)
    A = rows[:, None] * A * cols[None, :]
    if point is None:
        point = rng.standard_normal(n), interior(rng, seg_type, seg_len, False), interior(rng, seg_type, seg_len, True)
    x0, s0, y0 = point
    A32 = A.astype(F)
    A64 = A32.astype(np.float64)
    return _D(A32, A64 @ x0 + s0, -A64.T @ y0, seg_type, seg_len)


def _matrix_of(d):
    return np.asarray(d.mat_a, np.float64).reshape(d.n, d.m).T


_MADE = {}


def problem(name, seed=0):
    """the dense problem (the fields of Prob*.dense()) of an input by name: lp<m>x<n>s (the scaled _edge(m, n, seed); m = 2504 the
    scaled benchmark_lp(1252)), socp102x12s, layout_small_s, sdp45x6, sdp561x6 (unscaled, tests/warm_cases.py::sdp_numpy),
    sp40x30s, sp257x129s, spmixed145x40s (tests/sparse_cases.py), and the tau -> 0 families by their names"""
    key = (name, seed)
    if key in _MADE:
        return _MADE[key]
    from warm_cases import sdp_numpy, socp_numpy, sparse40x30
    if name in ("F1", "F2", "F3", "F4") or name.startswith("F6-"):
        import tau_zero_problems as Z
        fam = Z.family(name) if not name.startswith("F6-") else [f for f in Z.family("F6") if f.name == name][0]
        d = _D(fam.A, fam.vec_b, fam.vec_c, fam.seg_type, fam.seg_len)
    elif name == "lp2504x1252s":
        from problems import benchmark_lp
        _, G, _ = benchmark_lp(1252, seed=seed)
        d = scaled(name, seed, G, [RPOS], [2504])
    elif name.startswith("lp"):
        m, n = (int(v) for v in name[2:-1].split("x"))
        assert name.endswith("s")
        rng = np.random.default_rng(1000 * m + n + 7919 * seed)                    # _edge's own A, x0, s0, y0
        A = (rng.standard_normal((m, n)) / np.sqrt(n)).astype(F)
        point = rng.standard_normal(n), rng.uniform(0.1, 1.1, m), rng.uniform(0.1, 1.1, m)
        d = scaled(name, seed, A, [RPOS], [m], point)
    elif name == "socp102x12s":
        b = socp_numpy(seed)[0]
        d = scaled(name, seed, _matrix_of(b), b.seg_type, b.seg_len)
    elif name == "layout_small_s":
        import cone_layouts as CL
        b = CL.build("small", CL.LAYOUTS["small"]["seeds"][seed])
        d = scaled(name, seed, _matrix_of(b), b.seg_type, b.seg_len, (b.x0, b.s0, b.y0))
    elif name in ("sdp45x6", "sdp561x6"):
        d = sdp_numpy(6, 9 if name == "sdp45x6" else 33, seed)
    elif name == "sp40x30s":
        b = sparse40x30(seed)
        d = scaled(name, seed, _matrix_of(b), b.seg_type, b.seg_len)
    else:
        from sparse_cases import sparse_problem
        assert name in ("sp257x129s", "spmixed145x40s"), name
        b = sparse_problem({"sp257x129s": "lp257x129", "spmixed145x40s": "mixed145x40"}[name], seed)
        d = scaled(name, seed, _matrix_of(b), b.seg_type, b.seg_len)
    d.name, d.seed = name, seed
    _MADE[key] = d
    return d


def with_matrix(d, mat_a):
    """d over another column-major matrix (the widened form of a matrix stored in 16 bits)"""
    e = copy.copy(d)
    e._f64 = None
    e.mat_a = np.ascontiguousarray(mat_a, dtype=F).ravel()
    assert e.mat_a.size == d.m * d.n
    return e


def f64_problem(d):
    """the warm_numpy.Problem of a dense problem, kept on the object itself (it lives as long as the problem does)"""
    if getattr(d, "_f64", None) is None:
        d._f64 = W.Problem.of_dense(d)
    return d._f64


# ---- the problem sets of the own-A families -------------------------------------------------------------------------------------------

OWN_A_FAMILIES = ("small", "mid", "mid16-bf16", "mid16-f16", "sdp", "ragged", "sparse", "raggedsparse")


def _set(name, seeds):
    return [(name, s) for s in seeds]


def own_a_sets(family):
    """[(label, [(input, seed)], [keywords], resident)] of an own-A family: the sets of tests/test_gpu_warm_start.py::Fam with the
    scaled variants in place of the _edge problems, layout_small_s where the family takes block cones, sdp561x6 for sdp and ragged.
    A set has three members (sdp561x6: the same problem three times), so that every k is among its starts.  resident: for the
    sparse families, per keyword set, which members hold their entries in LDS (tests/test_sparsebatch_cpu.py and
    tests/test_raggedsparse_cpu.py hold the rule; here it is what the case names); None elsewhere"""
    one = [{"a_dtype": family[6:]}] if family.startswith("mid16") else [{}]
    layout = ("layout_small_s", _set("layout_small_s", range(3)), one, None)
    if family == "small":
        return [("lp80x40s", _set("lp80x40s", range(3)), one, None), ("lp1x1s", _set("lp1x1s", range(3)), one, None),
                ("socp102x12s", _set("socp102x12s", range(3)), one, None), layout]
    if family.startswith("mid"):
        return [("lp160x96s", _set("lp160x96s", range(3)), one, None), ("lp157x157s", _set("lp157x157s", range(3)), one, None), layout]
    if family == "sdp":
        return [("sdp45x6", _set("sdp45x6", range(3)), one, None), ("sdp561x6", [("sdp561x6", 0)] * 3, one, None), layout]
    if family == "ragged":
        return [("seven", [("lp1x1s", 0), ("sdp561x6", 0), ("lp80x40s", 0), ("lp160x96s", 0), ("lp157x157s", 0), ("sdp45x6", 0),
                           ("layout_small_s", 0)], one, None)]
    if family == "sparse":           # 198 entries lie in LDS beside the vectors; the 22 800 of the layout's full A do not
        return [("sp40x30s", _set("sp40x30s", range(3)), [{}, {"force_resident": 0}], [[1, 1, 1], [0, 0, 0]]),
                layout[:3] + ([[0, 0, 0]],)]
    assert family == "raggedsparse", family
    # sp257x129s in a slot of m n entries cannot reside (streamed); the others reside; nor can the layout's full A
    return [("four", [("sp40x30s", 0), ("sp257x129s", 0), ("spmixed145x40s", 0), ("lp80x40s", 0)], [{"nnz_caps": [0, 257 * 129, 0, 3200]}],
             [[1, 0, 1, 1]]), layout[:3] + ([[0, 0, 0]],)]


# ---- the starts ---------------------------------------------------------------------------------------------------------------

_RUNS = {}


def _f32(xy):
    return xy[0].astype(F), xy[1].astype(F)


def start(name, k, seed=0):
    """the f64 restatement's iterate after iteration k of problem(name, seed) from the zero start, rounded to f32"""
    key = (name, seed)
    if key not in _RUNS:
        ks = ks_of(name)
        _RUNS[key] = W.run(f64_problem(problem(name, seed)), max(ks) + 1, snap_iters=ks).snaps
    return _f32(_RUNS[key][k])


_TZ = {}


def tau_zero_starts(name):
    """[(label, iteration index, (x, y) in f32)] of a tau -> 0 family: `before` the iterate just before tau first clamps to 0,
    `zero` the first iterate with tau == 0, and where tau returns within the window `back`, the first iterate after that"""
    if name not in _TZ:
        r = W.run(f64_problem(problem(name)), TAU_ZERO_WINDOW, snap_iters=range(TAU_ZERO_WINDOW))
        tau = [r.snaps[i][0][-1] for i in range(TAU_ZERO_WINDOW)]
        first = next(i for i, t in enumerate(tau) if t == 0.0)
        assert first >= 1 and tau[first - 1] > 0.0
        out = [("before", first - 1, _f32(r.snaps[first - 1])), ("zero", first, _f32(r.snaps[first]))]
        back = next((i for i in range(first + 1, TAU_ZERO_WINDOW) if tau[i] > 0.0), None)
        if back is not None:
            out.append(("back", back, _f32(r.snaps[back])))
        _TZ[name] = out
    return _TZ[name]


# ---- the reference and the bound --------------------------------------------------------------------------------------------------

def parts(p, x, y):
    """(x_x, x_y, x_s, tau, u, v, kappa) of an iterate, in f64"""
    n, m = p.n, p.m
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    assert x.size == n + 2 * m + 1 and y.size == n + m + 1, (x.size, y.size, n, m)
    return x[:n], x[n:n + m], x[n + m:n + 2 * m], x[-1], y[:n], y[n:n + m], y[-1]


def reference_step(problem, x32, y32):
    """(x, y, kind, criteria) of one iteration in f64 from the f32 start, through warm_numpy.run(p, 1, start=...)"""
    p = problem if isinstance(problem, W.Problem) else f64_problem(problem)
    r = W.run(p, 1, start=(np.asarray(x32, np.float64), np.asarray(y32, np.float64)))
    return r.x, r.y, r.kind, tuple(r.cri)


def bounds(problem, x32, y32):
    """(B_x, B_y): per component of x = (x_x, x_y, x_s, tau) and y = (u, v, kappa) the sum of the absolute values of its terms"""
    p = problem if isinstance(problem, W.Problem) else f64_problem(problem)
    xx, xy, xs, tau, u, v, kappa = (np.abs(a) for a in parts(p, x32, y32))
    A, b, c = np.abs(p.A), np.abs(p.b), np.abs(p.c)
    Bxx = xx + p.Tx * (A.T @ v + c * kappa)
    Bxy = xy + p.Ty * (b * kappa + A @ u)
    Bxs = xs + p.Ts * v
    Bt = tau + p.t_tau * (c @ u + b @ v)
    rx, ry, rs, rt = xx + 2 * Bxx, xy + 2 * Bxy, xs + 2 * Bxs, tau + 2 * Bt
    Bu = u + p.Tx * (A.T @ ry + c * rt)
    Bv = v + p.Sv * (A @ rx + rs + b * rt)
    Bk = kappa + p.s_kappa * (c @ rx + b @ ry)
    return np.concatenate([Bxx, Bxy, Bxs, [Bt]]), np.concatenate([Bu, Bv, [Bk]])


def _ratio(delta, allowed):
    """max delta / allowed, 0 where delta is 0 (a component with no terms has B = 0 and must be exact)"""
    delta, allowed = np.atleast_1d(delta), np.atleast_1d(allowed)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(delta == 0.0, 0.0, delta / allowed)
    return float(r.max()) if r.size else 0.0


def violations(problem, start, got_x, got_y, kind=None, cri=None):
    """(ratios, failures): ratios = the worst |d| / (EPS B) per vector (a block cone enters x_y / x_s with ||d||_2 over its own
    allowance; u, v, kappa may reach Y_FACTOR), failures = one line per assertion of check() that does not hold"""
    p = problem if isinstance(problem, W.Problem) else f64_problem(problem)
    n, m = p.n, p.m
    rx, ry, rkind, rcri = reference_step(p, *start)
    Bx, By = bounds(p, *start)
    gx, gy = np.asarray(got_x, np.float64), np.asarray(got_y, np.float64)
    assert gx.shape == rx.shape and gy.shape == ry.shape, (gx.shape, gy.shape)
    fails, ratios = [], {}
    if not (np.isfinite(gx).all() and np.isfinite(gy).all()):
        return {"nonfinite": np.inf}, ["the iterate is not finite"]
    dx, dy = np.abs(gx - rx), np.abs(gy - ry)
    ratios["x_x"] = _ratio(dx[:n], EPS * Bx[:n])
    ratios["tau"] = _ratio(dx[-1], EPS * Bx[-1])
    for nm, base in (("x_y", n), ("x_s", n + m)):
        worst, off = 0.0, 0
        for t, l in zip(p.seg_type, p.seg_len):
            s = slice(base + off, base + off + l)
            if l and t < SOC:
                r = _ratio(dx[s], EPS * Bx[s])
                if r > 1.0:
                    i = int(np.argmax(np.where(dx[s] == 0, 0, dx[s] / np.maximum(EPS * Bx[s], 1e-300))))
                    fails.append("%s row %d (cone %d): |d| = %.3e > EPS B = %.3e" % (nm, off + i, t, dx[s][i], EPS * Bx[s][i]))
            elif l:
                allow = EPS * np.linalg.norm(Bx[s]) + T_CONE[t] * np.abs(rx[s]).max()
                r = _ratio(np.linalg.norm(dx[s]), allow)
                if r > 1.0:
                    fails.append("%s block at row %d (cone %d, %d rows): ||d|| = %.3e > %.3e" % (nm, off, t, l, np.linalg.norm(dx[s]), allow))
            else:
                r = 0.0
            worst = max(worst, r)
            off += l
        ratios[nm] = worst
    for nm, s in (("x_x", slice(0, n)), ("tau", slice(n + 2 * m, n + 2 * m + 1))):
        if ratios[nm] > 1.0:
            i = int(np.argmax(np.where(dx[s] == 0, 0, dx[s] / np.maximum(EPS * Bx[s], 1e-300))))
            fails.append("%s[%d]: |d| = %.3e > EPS B = %.3e" % (nm, i, dx[s][i], EPS * Bx[s][i]))
    for nm, s in (("u", slice(0, n)), ("v", slice(n, n + m)), ("kappa", slice(n + m, n + m + 1))):
        ratios[nm] = _ratio(dy[s], EPS * By[s])
        if ratios[nm] > Y_FACTOR:
            i = int(np.argmax(np.where(dy[s] == 0, 0, dy[s] / np.maximum(EPS * By[s], 1e-300))))
            fails.append("%s[%d]: |d| = %.3e > %g EPS B = %.3e" % (nm, i, dy[s][i], Y_FACTOR, Y_FACTOR * EPS * By[s][i]))
    decided = abs(rx[-1] - p.eps_zero) > EPS * Bx[-1]
    if kind is not None:
        if decided and kind != rkind:
            fails.append("kind %d, the reference's %d (tau %.3e)" % (kind, rkind, rx[-1]))
        if cri is not None and kind == rkind:
            k = 3 if rkind == 0 else 2
            want, have = np.array(rcri[:k], np.float64), np.array(cri[:k], np.float64)
            if not np.array_equal(np.isinf(want), np.isinf(have)) or not np.allclose(have, want, rtol=CRI_RTOL, atol=CRI_ATOL):
                fails.append("criteria %s, the reference's %s" % (tuple(have), tuple(want)))
    return ratios, fails


def check(problem, start, got_x, got_y, kind=None, cri=None):
    """asserts the bound of the module docstring on (got_x, got_y), the result of one iteration from `start` (and, where given, on
    the kind and the criteria the loop reports); returns the worst ratio |d| / (EPS B) per vector"""
    ratios, fails = violations(problem, start, got_x, got_y, kind, cri)
    assert not fails, "; ".join(fails)
    return ratios


def fmt(ratios):
    return " ".join("%s %.3f" % kv for kv in ratios.items())


def old_check_passes(problem, start, got_x, got_y):
    """what the suite held one iteration from a snapshot to before (tests/warm_cases.py::iterate_tol(1) of the iterate's max norm)"""
    from warm_cases import iterate_tol
    p = problem if isinstance(problem, W.Problem) else f64_problem(problem)
    rx, ry, _, _ = reference_step(p, *start)
    tol = iterate_tol(1, PSD in p.seg_type)
    ex = np.abs(np.asarray(got_x, np.float64) - rx).max() / max(np.abs(rx).max(), 1e-6)
    ey = np.abs(np.asarray(got_y, np.float64) - ry).max() / max(np.abs(ry).max(), 1e-6)
    return bool(ex <= tol and ey <= tol)
