"""GPU: start iterates of the six own-A batch families (thip_<family>_set_iterates; set_iterate / set_iterates / raw_iterate /
replace(start=) of the Python classes).  A problem handed its own iterate continues bit for bit (which pins the carried pair
A x_x, A^T x_y of the streamed families); a problem started at the oracle's snapshot after iteration k reaches the oracle's
snapshot at k + j; a start on a changed (b, c) follows the f64 restatement (tests/warm_numpy.py, validated on the CPU by
tests/test_warm_start_cpu.py); a solve restarted from its own answer ends at once; a start touches no other problem; a stopped
slot runs again; every refusal leaves the batch as it was.

Tolerances (tests/warm_cases.py::iterate_tol) are what the families' own oracle tests hold an iterate to at the iterates they check
(tests/ownbatch_cases.py TOLS / SDP_TOLS: 2e-5 at 0 and 1, 1e-4 at 9, 2e-3 at 99; with a PSD cone 5e-5, 3e-4, 3e-3 at 49), and between
two of those the geometric interpolation of the two -- 1.03e-4 at iterate 10 and 1.39e-4 at 19, with a PSD cone 3.18e-4 and 5.33e-4 --
relative to the reference iterate's max norm."""
import copy

import numpy as np
import pytest

import warm_numpy as W
from ownbatch_cases import F, T, _dense_of, _edge, _same, _snap  # noqa: F401  (T: the fixture)
from sparse_cases import csc_of, sparse_problem
from warm_cases import J_RUN, K_START, PSD, ends_at_once_candidates, iterate_tol, oracle_run, sdp_numpy, snap_xy, socp_numpy, sparse40x30

pytestmark = pytest.mark.gpu

FAMILIES = ["small", "mid", "sdp", "ragged", "sparse", "raggedsparse"]


def _tol(d, it):
    return iterate_tol(it, PSD in d.seg_type)


def _param(T, arith=None, **kw):
    p = T.SolverParam()
    p.eps_acc = 1e-30
    if arith:
        p.state_arith = arith
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class Fam:
    """a family: its class, the workgroup sizes its test hook forces, its problem sets [(label, problems, SOCP pieces per problem or
    None, [extra keywords])], and how it is made and refilled"""

    def __init__(self, T, name):
        self.name = name
        self.cls = {"small": T.SmallBatchSolver, "mid": T.MidBatchSolver, "sdp": T.SdpBatchSolver, "ragged": T.RaggedBatchSolver,
                    "sparse": T.SparseBatchSolver, "raggedsparse": T.RaggedSparseBatchSolver}[name]
        self.forced = (64, 256, 1024) if name == "small" else (256, 1024)
        self.sparse = name in ("sparse", "raggedsparse")
        one = [{}]
        if name == "small":
            socp = [socp_numpy(s) for s in range(2)]
            self.sets = [("lp80x40", [_edge(80, 40, s) for s in range(3)], None, one), ("lp1x1", [_edge(1, 1, s) for s in range(2)], None, one),
                         ("socp102x12", [d for d, _ in socp], [p for _, p in socp], one)]
        elif name == "mid":
            self.sets = [("lp160x96", [_edge(160, 96, s) for s in range(2)], None, one),       # aligned: 16-byte loads
                         ("lp157x157", [_edge(157, 157, s) for s in range(2)], None, one)]     # m odd: the 4-byte path
        elif name == "sdp":
            self.sets = [("sdp45x6", [sdp_numpy(6, 9, s) for s in range(2)], None, one),
                         ("sdp561x6", [sdp_numpy(6, 33, 0)], None, one)]                        # order 33: the larger LDS map
        elif name == "ragged":                                                                  # both thread classes, 1 x 1 among them
            self.sets = [("five", [_edge(1, 1, 0), _edge(80, 40, 0), _edge(160, 96, 0), _edge(157, 157, 0), sdp_numpy(6, 9, 0)], None, one)]
        elif name == "sparse":
            self.sets = [("sp40x30", [sparse40x30(s) for s in range(3)], None, [{}, {"force_resident": 0}])]
        else:       # lp257x129 in a slot of m n entries cannot reside (streamed, the 1024-thread class); the others reside
            ds = [sparse40x30(0), sparse_problem("lp257x129", 0), sparse_problem("mixed145x40", 0), _edge(80, 40, 0)]
            self.sets = [("four", ds, None, [{"nnz_caps": [0, 257 * 129, 0, 3200]}])]

    def make(self, ds, p, forced=None, **kw):
        return self.cls.from_dense(ds, p, force_threads=forced, **kw)

    def replace(self, sb, i, d, start=None):
        sb.replace(i, csc_of(d) if self.sparse else d.mat_a, d.vec_b, d.vec_c, d.vec_b_rowabs, start=start)

    def oracle(self, label, q, d, pieces):
        return oracle_run("%s/%s/%d" % (self.name, label, q), d, socp=None if pieces is None else pieces[q])


@pytest.fixture(scope="module")
def fams(T):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Fam(T, name)
        return made[name]
    return get


def _with_bc(d, b, c):
    e = copy.copy(d)
    e.vec_b, e.vec_c = np.asarray(b, F), np.asarray(c, F)
    return e


def _perturbed(d, seed):
    rng = np.random.default_rng(77 + seed)
    return _with_bc(d, d.vec_b * (1 + 0.01 * rng.standard_normal(d.m)), d.vec_c * (1 + 0.01 * rng.standard_normal(d.n)))


def _rel(got, want):
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-6)


# ---- 1. bitwise continuation ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_bitwise_continuation(T, fams, name):
    fam = fams(name)
    p = _param(T, "plain")
    for label, ds, _, kws in fam.sets:
        for kw in kws:
            for forced in fam.forced:
                for hand, poll in ((10, 1), (10, 7), (10, 64), (1, 1), (1, 7), (1, 64)):
                    R, S = fam.make(ds, p, forced, **kw), fam.make(ds, p, forced, **kw)
                    try:
                        R.run(hand, poll_every=poll)
                        its = [R.iterate(i) for i in range(len(ds))]
                        S.set_iterates([x for x, _ in its], [y for _, y in its])
                        assert S.info()["live"] == len(ds)
                        S.run(10, poll_every=poll)
                        R.run(10, poll_every=poll)
                        for i in range(len(ds)):
                            r, s = _snap(R, i), _snap(S, i)
                            tag = (name, label, kw, forced, hand, poll, i)
                            assert np.array_equal(r[0], s[0]) and np.array_equal(r[1], s[1]), tag
                            assert r[2][0] == s[2][0] == -1 and r[2][2:] == s[2][2:], (tag, r[2], s[2])
                            assert s[2][1] == 10 and r[2][1] == hand + 10, tag
                    finally:
                        R.destroy()
                        S.destroy()


# ---- 2. oracle parity ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arith", ["plain", "compensated"])
@pytest.mark.parametrize("name", FAMILIES)
def test_oracle_parity(T, fams, name, arith):
    fam = fams(name)
    p = _param(T, arith)
    worst = {}
    for label, ds, pieces, kws in fam.sets:
        ros = [fam.oracle(label, q, d, pieces) for q, d in enumerate(ds)]
        for kw, k, j in [(kw, k, j) for kw in kws for k in K_START for j in J_RUN]:
            sb = fam.make(ds, p, **kw)
            try:
                starts = [snap_xy(ro, d, k) for ro, d in zip(ros, ds)]
                sb.set_iterates([x.astype(F) for x, _ in starts], [y.astype(F) for _, y in starts])
                sb.run(j, poll_every=64)
                for i, (ro, d) in enumerate(zip(ros, ds)):
                    x, y = sb.iterate(i)
                    rx, ry = snap_xy(ro, d, k + j)
                    tol = _tol(d, k + j)
                    ex, ey = _rel(x, rx), _rel(y, ry)
                    wk = (k, j) + tuple(kw.get(f) for f in ("force_resident",) if f in kw)
                    worst[wk] = max(worst.get(wk, 0.0), ex, ey)
                    print("warm %s %s %s %s problem %d start %d + %d: err x %.2e y %.2e (tol %.2e)" % (name, arith, label, kw, i, k, j, ex, ey, tol))
                    assert ex <= tol and ey <= tol, (name, label, i, k, j, ex, ey)
                    st = sb.status(i)
                    tr = ro.trace[k + j]
                    assert st.state == -1 and st.iters == j and st.kind == tr[1], (name, label, i, k, j, st.iters, st.kind)
                    assert np.allclose(st.cri, tr[2:], rtol=max(50 * tol, 1e-3), atol=1e-5), (name, label, i, k, j, st.cri, tr)
            finally:
                sb.destroy()
    print("warm %s %s worst errors by (start, iterations): %s" % (name, arith, " ".join("%s %.2e" % kv for kv in sorted(worst.items()))))


# ---- 3. another (b, c) --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_replace_with_start_on_another_b_c(T, fams, name):
    fam = fams(name)
    p = _param(T, "plain")
    for label, ds, _, kws in fam.sets:
        for kw in kws:
            i = len(ds) - 1
            new = _perturbed(ds[i], i)
            held = ds[:i] + [new]
            A, B = fam.make(ds, p, **kw), fam.make(held, p, **kw)
            try:
                A.run(10, poll_every=64)
                x, y = A.iterate(i)                                  # (running: the raw iterate)
                fam.replace(A, i, new, start=(x, y))
                B.set_iterate(i, x, y)
                for a, b in zip(A.precond(i), B.precond(i)):
                    assert np.array_equal(a, b), (name, label)
                ref = W.run(W.Problem.of_dense(new), 10, start=(x, y), snap_iters=(0, 9))
                done = 0
                for j in (1, 10):
                    A.run(j - done, poll_every=64)
                    B.run(j - done, poll_every=64)
                    done = j
                    _same(_snap(A, i), _snap(B, i))
                    gx, gy = A.iterate(i)
                    tol = _tol(new, j - 1)                           # j iterations from the same f32 start: the ladder at iterate j - 1
                    ex, ey = _rel(gx, ref.snaps[j - 1][0]), _rel(gy, ref.snaps[j - 1][1])
                    print("warm %s %s %s replace(start) + %d: err x %.2e y %.2e (tol %.2e)" % (name, label, kw, j, ex, ey, tol))
                    assert ex <= tol and ey <= tol, (name, label, j, ex, ey)
                    assert A.status(i).iters == j
            finally:
                A.destroy()
                B.destroy()


# ---- 4. ends at once ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_ends_at_once(T, fams, name):
    fam = fams(name)
    ds = ends_at_once_candidates()[name]
    for kw in ([{"nnz_caps": [0] * len(ds)}] if name == "raggedsparse" else fam.sets[0][3]):      # (sparse: resident and streamed)
        _ends_at_once(T, fam, name, ds, kw)


def _ends_at_once(T, fam, name, ds, kw):
    sb = fam.make(ds, _param(T, eps_acc=1e-5, eps_inf=1e-5, max_iter=400000), **kw)
    try:
        first = sb.run(-1, poll_every=256)
        assert [r.state for r in first] == [0] * len(ds), [(r.state, r.iters) for r in first]
        sols = [sb.solution(i)[0] for i in range(len(ds))]
        raws = [sb.raw_iterate(i) for i in range(len(ds))]
        for i, (x, y) in enumerate(raws):                        # raw_iterate undoes the read-out's 1 / tau, to one rounding
            sx, _ = sb.iterate(i)
            nm = ds[i].n + ds[i].m
            assert x[-1] == sx[-1] and np.array_equal(x[nm:], sx[nm:])
            assert np.allclose(x[:nm], sx[:nm] * x[-1], rtol=3e-7, atol=0)
        sb.set_param(_param(T, eps_acc=1e-3, eps_inf=1e-3, max_iter=400000))
        for i, d in enumerate(ds):
            fam.replace(sb, i, d, start=raws[i])
            assert all(np.array_equal(a, b) for a, b in zip(sb.iterate(i), raws[i])) and sb.status(i).state == -1
        for i, r in enumerate(sb.run(-1, poll_every=1)):
            x = sb.solution(i)[0]
            print("warm %s %s ends at once: problem %d (%d x %d) %d iterations first, then state %d at index %d"
                  % (name, kw, i, ds[i].m, ds[i].n, first[i].iters + 1, r.state, r.iters))
            assert r.state == 0 and r.iters <= 2, (name, i, r.state, r.iters)
            assert np.abs(x - sols[i]).max() <= 1e-3 * max(1.0, np.abs(sols[i]).max()), (name, i)
    finally:
        sb.destroy()


# ---- 5. independence ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arith", ["plain", "compensated"])
@pytest.mark.parametrize("name", FAMILIES)
def test_independence(T, fams, name, arith):
    fam = fams(name)
    label, ds, _, kws = fam.sets[0]
    P, at = 300, (0, 150, 299)
    cyc = [ds[i % len(ds)] for i in range(P)]
    for i in at:
        cyc[i] = ds[0]
    p = _param(T, arith)
    for kw in kws:
        kw = dict(kw)
        if "nnz_caps" in kw:
            kw["nnz_caps"] = [kw["nnz_caps"][0 if i in at else i % len(ds)] for i in range(P)]
        _independence(fam, cyc, p, kw, P, at, arith)


def _independence(fam, cyc, p, kw, P, at, arith):
    ref, one, bulk, singles, src = (fam.make(cyc, p, **kw) for _ in range(5))
    try:
        src.run(3, poll_every=64)
        its = [src.iterate(i) for i in range(P)]
        x0, y0 = its[0]
        ref.run(10, poll_every=64)
        for i in at:
            one.set_iterates([x0], [y0], first=i)
        one.run(10, poll_every=64)
        started = [_snap(one, i) for i in at]
        for s in started[1:]:
            _same(s, started[0])
        assert started[0][2][1] == 10
        for i in range(P):
            if i not in at:
                _same(_snap(one, i), _snap(ref, i))
        bulk.set_iterates([x for x, _ in its], [y for _, y in its])
        for i in range(P):
            singles.set_iterate(i, *its[i])
        bulk.run(10, poll_every=64)
        singles.run(10, poll_every=64)
        for i in range(P):
            _same(_snap(bulk, i), _snap(singles, i))
        if arith == "plain":                                     # (and both continue src, whose Kahan terms a plain run does not have)
            src.run(10, poll_every=64)
            for i in range(P):
                b, s = _snap(bulk, i), _snap(src, i)
                assert np.array_equal(b[0], s[0]) and np.array_equal(b[1], s[1]) and b[2][1] + 3 == s[2][1]
    finally:
        for sb in (ref, one, bulk, singles, src):
            sb.destroy()


# ---- 6. a stopped slot --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_a_stopped_slot_runs_again(T, fams, name):
    from tau_zero_problems import family as tz_family
    from totsu_amd import _lib
    fam = fams(name)
    label, ds, _, kws = fam.sets[0]
    f1 = _dense_of(tz_family("F1"))                              # the infeasible LP, 128 x 64: its iteration ends through tau = 0
    f1.vec_b_rowabs = None
    kw1 = {"nnz_caps": [0, 0]} if name == "raggedsparse" else {}
    cases = [("excess", ds, _param(T, max_iter=5), kw, _lib.ST_EXCESS_ITER, 0) for kw in kws] + \
            [("tau zero", [f1, f1], _param(T, eps_acc=1e-5, eps_inf=1e-5, max_iter=5000), dict(kw1, **{k: v for k, v in kw.items() if k != "nnz_caps"}),
              _lib.ST_INFEASIBLE, 1) for kw in kws]
    for what, held, p, kw, state, kind in cases:
        sb, fresh = fam.make(held, p, **kw), fam.make(held, p, **kw)
        try:
            res = sb.run(-1, poll_every=64)
            assert [r.state for r in res] == [state] * len(held) and res[0].kind == kind, (what, [(r.state, r.kind, r.iters) for r in res])
            assert sb.info()["live"] == 0
            i = len(held) - 1
            x, y = sb.raw_iterate(i)
            assert (x[-1] <= 1e-12) == (kind == 1)
            before = sb.info()
            sb.set_iterate(i, x, y)
            st = sb.status(i)
            assert st.state == -1 and st.iters == 0 and st.kind == 0 and tuple(st.cri) == (0.0, 0.0, 0.0), (what, st.state, st.iters)
            assert sb.info()["live"] == 1
            fresh.set_iterate(i, x, y)
            sb.run(3, poll_every=3)
            after = sb.info()
            assert after["launches"] == before["launches"] + 1 and after["workgroups"] == before["workgroups"] + 1, what
            fresh.run(3, poll_every=3)
            _same(_snap(sb, i), _snap(fresh, i))
            assert sb.status(i).iters >= 1 or sb.status(i).state != -1
            for q in range(len(held) - 1):                       # the other slots stay stopped where they were
                assert sb.status(q).state == state and sb.status(q).iters == res[q].iters
        finally:
            sb.destroy()
            fresh.destroy()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_refusals(T, fams, name, monkeypatch):
    from totsu_amd import _lib
    fam = fams(name)
    label, ds, _, kws = fam.sets[0]
    for kw in kws:
        _refusals(T, fam, name, ds, kw, monkeypatch)


def _refusals(T, fam, name, ds, kw, monkeypatch):
    from totsu_amd import _lib
    sb = fam.make(ds, _param(T), **kw)
    try:
        sb.run(2, poll_every=2)
        P, dev = len(ds), sb.info()["device_bytes"]
        x, y = sb.iterate(0)
        want = _snap(sb, 0)

        def bad(xx, yy, first=0, count=None):
            with pytest.raises(ValueError):
                if count is None:
                    sb.set_iterate(first, xx, yy)
                else:
                    sb.set_iterates([xx] * count, [yy] * count, first=first)
            assert sb.info()["device_bytes"] == dev
            _same(_snap(sb, 0), want)
        bad(x[:-1], y)                                           # wrong lengths
        bad(x, np.concatenate([y, y[:1]]))
        for k, v in ((-1, -1.0), (-1, np.nan), (-1, np.inf)):    # tau
            z = x.copy()
            z[k] = v
            bad(z, y)
        for v in (1.0, np.nan, -np.inf):                         # kappa
            z = y.copy()
            z[-1] = v
            bad(x, z)
        bad(x, y, first=P)                                       # ranges outside the batch
        bad(x, y, first=-1)
        if P > 1 and name not in ("ragged", "raggedsparse"):
            bad(x, y, first=P - 1, count=2)
        fn = getattr(_lib.load(), sb._prefix + "set_iterates")
        px, py = x.ctypes.data, y.ctypes.data
        for args in ((sb.h, P, 1, px, py), (sb.h, 0, 0, px, py), (sb.h, 0, -1, px, py), (sb.h, -1, 1, px, py), (sb.h, 0, P + 1, px, py),
                     (sb.h, 0, 1, None, py), (sb.h, 0, 1, px, None), (None, 0, 1, px, py)):
            assert fn(*args) == _lib.E_INVALID, args
        z = x.copy()                                             # the library's own word on tau and kappa (Python checks them first)
        z[-1] = -1.0
        assert fn(sb.h, 0, 1, z.ctypes.data, py) == _lib.E_INVALID
        z = y.copy()
        z[-1] = 1.0
        assert fn(sb.h, 0, 1, px, z.ctypes.data) == _lib.E_INVALID
        # a handle that was created and not initialised: the family's own constructor with its init call left out
        with monkeypatch.context() as mp:
            mp.setattr(_lib.lib, sb._prefix + "init", lambda h: 0, raising=False)
            raw = fam.make(ds, _param(T), **kw)
        try:
            assert fn(raw.h, 0, 1, px, py) == _lib.E_INVALID
            with pytest.raises(ValueError):
                raw.set_iterate(0, x, y)
        finally:
            raw.destroy()
        assert sb.info()["device_bytes"] == dev
        _same(_snap(sb, 0), want)
        sb.run(2, poll_every=2)                                  # and the batch still runs
        assert [sb.status(i).iters for i in range(P)] == [4] * P
        sb.set_iterate(0, x, y)                                  # a start that is taken allocates its staging buffer, once
        grown = sb.info()["device_bytes"] - dev
        assert 4 * (x.size + y.size) <= grown <= 4 * (x.size + y.size) + 16 and sb.status(0).iters == 0, grown
        sb.set_iterate(0, x, y)
        assert sb.info()["device_bytes"] == dev + grown
    finally:
        sb.destroy()
