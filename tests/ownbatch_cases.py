"""What the GPU tests of the three own-A batch families share (tests/test_gpu_smallbatch.py, tests/test_gpu_midbatch.py,
tests/test_gpu_sdpbatch.py): the problem families with their oracle runs (computed once per session and never changed), the
comparison of a batch against the f64 oracle, and the small helpers of the bitwise tests.  A plain module, like tests/problems.py."""
import numpy as np
import pytest

import oracle as O
from problems import benchmark_lp, partitioning_sdp, random_sdp, random_socp, svm_qp

F = np.float32
ITERS = [0, 1, 9, 99]
TOLS = [2e-5, 2e-5, 1e-4, 2e-3]      # iterates 0, 1, 9, 99 relative to the iterate's max norm (tests/test_gpu_solver.py)
SDP_ITERS, SDP_TOLS = [0, 1, 9, 49], [5e-5, 5e-5, 3e-4, 3e-3]      # tests/test_gpu_solver.py::test_iterates_sdp
MIXED_ORDERS = [3, 6, 6, 12, 6, 33, 12, 1]


@pytest.fixture(scope="module")
def T():
    import totsu_amd
    from totsu_amd import _lib
    _lib.init()
    return totsu_amd


def tri(k):
    return k * (k + 1) // 2


def _mb(T, typ):
    return T.MatBuild(T.F32HIP, typ)


class _D:
    """the fields of Prob*.dense() for problems built from arrays"""

    def __init__(self, a, b, c, seg_type, seg_len):
        a = np.asarray(a, F)
        self.m, self.n = a.shape
        self.mat_a, self.vec_b, self.vec_c = np.asfortranarray(a).ravel(order="F"), np.asarray(b, F), np.asarray(c, F)
        self.seg_type, self.seg_len, self.vec_b_rowabs = list(seg_type), list(seg_len), None


def _oracle(d, iters, socp=None):
    """the oracle's snapshots, trace and preconditioner of one problem.  socp: the ProbSOCP pieces -- its op_b adds scl_d, not
    |scl_d|, to the row sums (what dense().vec_b_rowabs carries), so the SOCP oracle is the SOCP one"""
    par = O.param(max_iter=max(iters) + 2, eps_acc=1e-30)
    if socp is not None:
        f, Gs, hs, cs, dd = socp
        return O.solve_socp(par, f, Gs, hs, cs, dd, np.zeros((0, f.size)), [], trace_cap=max(iters) + 3, snap_iters=iters)
    return O.solve_matop_cones(par, d.vec_c, d.mat_a, d.vec_b, d.seg_type, d.seg_len, snap_iters=iters, trace_cap=max(iters) + 3,
                               use_ql=True)


def _edge(m, n, seed):
    """a primal- and dual-feasible LP over the nonnegative cone: b = A x0 + s0, c = -A^T y0, s0, y0 ~ U(0.1, 1.1)"""
    rng = np.random.default_rng(1000 * m + n + 7919 * seed)
    A = (rng.standard_normal((m, n)) / np.sqrt(n)).astype(F)
    x0, s0, y0 = rng.standard_normal(n), rng.uniform(0.1, 1.1, m), rng.uniform(0.1, 1.1, m)
    return _D(A, A.astype(np.float64) @ x0 + s0, -A.astype(np.float64).T @ y0, [1], [m])


def _term_problem(i):
    """three kinds over A = [D; -D], D = diag(U(0.5, 1.5)), two unknowns: 0 an infeasible box (b = -1), 1 a feasible box (b = 1),
    2 the upper bounds alone (the rows of -D are zero) with c = (1, 1): unbounded"""
    rng = np.random.default_rng(100 + i)
    D = np.diag(rng.uniform(0.5, 1.5, 2))
    k = i % 3
    A = np.vstack([D, -D if k < 2 else 0.0 * D])
    return _D(A, -np.ones(4) if k == 0 else np.ones(4), np.ones(2), [1], [4])


def _lp_arrays(seeds):
    a, b, c = [], [], []
    for s in seeds:
        cc, G, h = benchmark_lp(20, seed=s)
        a.append(np.asfortranarray(G).ravel(order="F"))
        b.append(h)
        c.append(cc)
    return np.stack(a), np.stack(b), np.stack(c)


# ---- the families ------------------------------------------------------------------------------------------------------------

def _socp_dense(T, n, cones, seed):
    """(the dense problem, the ProbSOCP pieces the oracle needs)"""
    f, Gs, hs, cs, d = random_socp(n, cones, seed=seed)
    socp = T.ProbSOCP(_mb(T, T.MatType.General(n, 1)).set_array(f.reshape(-1, 1)),
                      [_mb(T, T.MatType.General(G.shape[0], n)).set_array(G) for G in Gs],
                      [_mb(T, T.MatType.General(len(h_), 1)).set_array(h_.reshape(-1, 1)) for h_ in hs],
                      [_mb(T, T.MatType.General(n, 1)).set_array(c_.reshape(-1, 1)) for c_ in cs], d,
                      _mb(T, T.MatType.General(0, n)), _mb(T, T.MatType.General(0, 1)))
    return socp.dense(), (f, Gs, hs, cs, d)


def _sdp_dense(T, n, k, seed):
    c, syms = random_sdp(n, k, seed=seed)
    sdp = T.ProbSDP(_mb(T, T.MatType.General(n, 1)).set_array(c.reshape(-1, 1)),
                    [_mb(T, T.MatType.SymPack(k)).set_array(s) for s in syms],
                    _mb(T, T.MatType.General(0, n)), _mb(T, T.MatType.General(0, 1)), 1e-12)
    d = sdp.dense()
    sdp.drop()
    return d


def _part_dense(T, grid, seed):
    w, syms_f, mat_a, vec_b = partitioning_sdp(*grid, seed=seed)
    l, n = grid[0] * grid[1], w.size
    sdp = T.ProbSDP(_mb(T, T.MatType.General(n, 1)).set_array(w.reshape(-1, 1)),
                    [_mb(T, T.MatType.SymPack(l)).set_array(s_) for s_ in syms_f],
                    _mb(T, T.MatType.General(l, n)).set_array(mat_a), _mb(T, T.MatType.General(l, 1)).set_array(vec_b.reshape(-1, 1)),
                    1e-12)
    d = sdp.dense()
    sdp.drop()
    assert d.seg_type == [O.CONE_PSD, O.CONE_ZERO] and d.seg_len == [n, l]
    return d


def _psd_block(T, n, k, seed):
    """the rows of one PSD cone of order k of a stacked problem in n unknowns: (its k (k + 1) / 2 rows of A, of b, its share of c),
    those of _sdp_dense(T, n, k, seed).  What _mixed_dense and tests/cone_layouts.py build their PSD segments from"""
    d = _sdp_dense(T, n, k, seed)
    sk = tri(k)
    return np.asarray(d.mat_a, dtype=F).reshape((n, d.m)).T[:sk], np.asarray(d.vec_b, dtype=F)[:sk], np.asarray(d.vec_c, dtype=F)


def _mixed_dense(T, seed):
    """in the manner of tests/test_gpu_solver.py::test_iterates_many_psd_cones: 3 nonnegative rows in front (no PSD block starts on a
    multiple of 4), PSD cones of eight orders, then a second-order cone of 17 rows and a rotated one of 5"""
    from totsu_amd import _lib
    n = 5
    rng = np.random.default_rng(99 + seed)
    blocks = [rng.standard_normal((3, n)).astype(F)]
    bs, st, sl = [np.abs(rng.standard_normal(3)).astype(F) + 1.0], [_lib.CONE_RPOS], [3]
    c0 = np.zeros(n, F)
    for q, k in enumerate(MIXED_ORDERS):
        rows, b, c = _psd_block(T, n, k, 10 + q + 100 * seed)
        blocks.append(rows)
        bs.append(b)
        st.append(_lib.CONE_PSD)
        sl.append(tri(k))
        c0 = c0 + c
    for t, rows in ((_lib.CONE_SOC, 17), (_lib.CONE_ROTSOC, 5)):   # s = b - A x with large leading entries: inside the cone at x = 0
        blocks.append((rng.standard_normal((rows, n)) / 4).astype(F))
        b = (rng.standard_normal(rows) / 4).astype(F)
        b[0] = 3.0
        if t == _lib.CONE_ROTSOC:
            b[1] = 3.0
        bs.append(b)
        st.append(t)
        sl.append(rows)
    a = np.vstack(blocks)
    beg = np.cumsum([0] + sl)[:-1]
    assert all(b_ % 4 != 0 for b_, t in zip(beg, st) if t == _lib.CONE_PSD)
    return _D(a, np.concatenate(bs), c0 / len(MIXED_ORDERS), st, sl)


_FAMILIES = {}


def family(T, name):
    """(list of dense problems, list of oracle results): computed once, shared by every test of every file that uses the family.
    lp20 / lp40 (ProbLP), lp80 / lp260 (arrays), socp, socp60, qp: the oracle at ITERS; sdp<k>, part<rows><columns>, mixed: the oracle
    at SDP_ITERS"""
    if name in _FAMILIES:
        return _FAMILIES[name]
    ds, ros, iters = [], [], ITERS
    if name in ("lp20", "lp40"):
        sz = int(name[2:])
        for i in range(5):
            c, G, h = benchmark_lp(sz, seed=i)
            lp = T.ProbLP(_mb(T, T.MatType.General(sz, 1)).set_array(c.reshape(-1, 1)), _mb(T, T.MatType.General(2 * sz, sz)).set_array(G),
                          _mb(T, T.MatType.General(2 * sz, 1)).set_array(h.reshape(-1, 1)), _mb(T, T.MatType.General(0, sz)),
                          _mb(T, T.MatType.General(0, 1)))
            ds.append(lp.dense())
            ros.append(_oracle(ds[-1], ITERS))
    elif name in ("lp80", "lp260"):
        sz = int(name[2:])
        for i in range(5):
            c, G, h = benchmark_lp(sz, seed=i)
            ds.append(_D(G, h, c, [1], [2 * sz]))
            ros.append(_oracle(ds[-1], ITERS))
    elif name in ("socp", "socp60"):
        n, cones, count, shape = (12, [5, 1, 0, 17, 70, 3], 4, (102, 12)) if name == "socp" else \
            (60, [5, 1, 0, 17, 140, 250, 3], 3, (423, 60))
        for i in range(count):
            d, pieces = _socp_dense(T, n, cones, i)
            ds.append(d)
            assert (d.m, d.n) == shape and d.vec_b_rowabs is not None and (name == "socp" or d.m * d.n > 24576)
            ros.append(_oracle(d, ITERS, socp=pieces))
    elif name == "qp":
        l = 12
        for i in range(3):
            q = svm_qp(l, seed=i)
            qp = T.ProbQP(_mb(T, T.MatType.SymPack(l)).set_by_fn(lambda r, c: q["sym_p"][r, c]),
                          _mb(T, T.MatType.General(l, 1)).set_array(q["vec_q"].reshape(-1, 1)),
                          _mb(T, T.MatType.General(l, l)).set_array(q["mat_g"]),
                          _mb(T, T.MatType.General(l, 1)).set_array(q["vec_h"].reshape(-1, 1)),
                          _mb(T, T.MatType.General(1, l)).set_array(q["mat_a"]),
                          _mb(T, T.MatType.General(1, 1)).set_array(q["vec_b"].reshape(-1, 1)), 1e-12)
            ds.append(qp.dense())
            assert (ds[-1].m, ds[-1].n) == (27, 13) and ds[-1].seg_type == [3, 1, 0]
            ros.append(_oracle(ds[-1], ITERS))          # (on the dense A itself: its P^(1/2) is the device's f32 one)
    else:
        iters = SDP_ITERS
        if name.startswith("sdp"):
            ds = [_sdp_dense(T, 6, int(name[3:]), seed) for seed in range(3)]
        elif name.startswith("part"):
            ds = [_part_dense(T, (int(name[4]), int(name[5])), seed) for seed in range(2)]
        else:
            assert name == "mixed", name
            ds = [_mixed_dense(T, seed) for seed in range(2)]
        ros = [_oracle(d, SDP_ITERS) for d in ds]
    for ro in ros:
        assert ro.status == O.EXCESS_ITER and len(ro.trace) > max(iters)
    _FAMILIES[name] = (ds, ros)
    return _FAMILIES[name]


# ---- a batch against the oracle ------------------------------------------------------------------------------------------------

def check_against_oracle(T, cls, label, ds, ros, iters, tols, state_arith=None, **kw):
    """a batch of class cls over the problems ds: every problem's preconditioner (rtol 2e-5), its iterate after each of iters against
    the oracle's snapshot (tols, relative to the snapshot's max norm), its status, kind and criteria there, and the workgroup size
    and LDS bound of info().  Returns info() for what the family adds to it"""
    p = T.SolverParam()
    p.eps_acc = 1e-30
    if state_arith:
        p.state_arith = state_arith
    sb = cls.from_dense(ds, p, **kw)
    try:
        n, m = ds[0].n, ds[0].m
        N = n + 2 * m + 1
        worst = [0.0] * len(iters)
        for i, ro in enumerate(ros):
            t, s = sb.precond(i)
            et, es = np.abs(t / ro.precond[:N] - 1).max(), np.abs(s / ro.precond[N:] - 1).max()
            print("%s problem %d preconditioner: rel err tau %.2e sigma %.2e" % (label, i, et, es))
            assert np.allclose(t, ro.precond[:N], rtol=2e-5, atol=0), (i, et)
            assert np.allclose(s, ro.precond[N:], rtol=2e-5, atol=0), (i, es)
        done = 0
        for q, (it, tol) in enumerate(zip(iters, tols)):
            sb.run(it + 1 - done, poll_every=64)
            done = it + 1
            for i, ro in enumerate(ros):
                x, y = sb.iterate(i)
                rx, ry = ro.snaps[q][:N], ro.snaps[q][N:]
                sx, sy = max(np.abs(rx).max(), 1e-6), max(np.abs(ry).max(), 1e-6)
                ex, ey = np.abs(x - rx).max() / sx, np.abs(y - ry).max() / sy
                worst[q] = max(worst[q], ex, ey)
                print("%s problem %d iterate %d: err x %.2e y %.2e (tol %.0e)" % (label, i, it, ex, ey, tol))
                assert ex <= tol and np.abs(x - rx).max() <= tol * sx, (i, it, ex)
                assert ey <= tol and np.abs(y - ry).max() <= tol * sy, (i, it, ey)
                st = sb.status(i)
                assert st.state == -1 and st.iters == it + 1
                tr = ro.trace[it]
                assert st.kind == tr[1]
                assert np.allclose(st.cri, tr[2:], rtol=max(50 * tol, 1e-3), atol=1e-5), (i, it, st.cri, tr)
        print("%s worst iterate errors at %s: %s" % (label, iters, " ".join("%.2e" % w for w in worst)))
        info = sb.info()
        assert info["threads"] == (kw.get("force_threads") or info["threads"]) and info["lds_bytes"] <= 163840
        return info
    finally:
        sb.destroy()


# ---- helpers of the bitwise and the tau -> 0 tests ---------------------------------------------------------------------------------

def _View(T, base, offset, n):
    """a DeviceBuffer that is a window into a buffer someone else owns"""
    class V(T.DeviceBuffer):
        def __init__(self):                    # (no allocation)
            self.n, self.ptr = n, base.ptr + 4 * offset

        def free(self):
            self.ptr = None
    return V()


def _snap(sb, i):
    st = sb.status(i)
    return sb.iterate(i) + ((st.state, st.iters, st.kind, tuple(st.cri)),)


def _same(g, w):
    assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and g[2] == w[2], (g[2], w[2])


def _dense_of(fam):
    from totsu_amd.problem import _Dense
    return _Dense(*fam.args())


def _compare_snap(tag, fam, pl, it, x, y, st):
    """the iterate after iteration `it` against the oracle's; at a decisive snap also kind, criteria and tau == 0
    (tests/test_gpu_tau_zero.py)"""
    N = pl.N
    tol = fam.tol(it)
    rx, ry = pl.snaps[it][:N], pl.snaps[it][N:]
    sx, sy = max(np.abs(rx).max(), 1e-6), max(np.abs(ry).max(), 1e-6)
    ex, ey = np.abs(x - rx).max() / sx, np.abs(y - ry).max() / sy
    print("tau_zero %-22s it %2d kind %d %s err x %.2e y %.2e (tol %.0e) tau %.3e cri %s"
          % (tag, it, pl.kinds[it], "decisive" if pl.decisive[it] else "--------", ex, ey, tol, x[N - 1], tuple("%.3e" % c for c in st.cri)))
    assert ex <= tol and ey <= tol, (tag, it, ex, ey, tol)
    assert st.iters == it + 1, (tag, it, st.iters)
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
