"""GPU: the wide batch over a library-owned 16-bit copy of every problem's A (totsu_amd.Wide16BatchSolver / thip_wide16batch_*).

The contract under test: with W the widened matrix of the stored form (tests/mid16_cases.py), a Wide16BatchSolver is BIT FOR BIT a
WideBatchSolver over W in f32 -- the twin: the whole arena block (6 n + 11 m floats), the status blocks, solutions(), the
preconditioner.  So:
    1. the stored form against its numpy restatement, word for word;
    2. the twin on the family layouts of tests/ownbatch_cases.py (PSD orders below and above 32, rotated cones, a mixed layout), and on
       the layouts the mid batch takes also a Mid16BatchSolver;
    3. the twin beyond the old rules and on every edge shape of the tiling;
    4. the f64 oracle run on W at the project's tolerances, the f32 twin first;
    5. 4096 x 4096;
    6. bitwise independence of index, neighbours and launch cuts;
    7. every round call against the twin after the same call with the widened new matrix;
    8. stop conditions in lockstep with the twin;
    9. refusals and info();
   10. the mixed route into an f32 batch over the exact matrices.
Both stored forms unless said.  Every reference is computed once and never changed."""
import ctypes as C

import numpy as np
import pytest

import mid16_cases as M
import oracle as O
import tau_zero_problems as Z
import wide16_cases as W
from ownbatch_cases import F, ITERS, TOLS, T, _dense_of, _edge, _oracle, _sdp_dense, _term_problem, check_against_oracle, tri  # noqa: F401
from ownbatch_cases import family as _family

pytestmark = pytest.mark.gpu

KINDS = M.KINDS
# (workgroup size, state arithmetic): not the full 2 x 2 -- the seams are tested in full by the wide and the mid16 suites
PARAMS = [(256, "compensated"), (1024, "plain")]


def _destroy(*solvers):
    for s in solvers:
        s.destroy()


# ---- 1. the stored form ------------------------------------------------------------------------------------------------------------

def _stored_cases(T):
    out = [(m, n, [1], [m]) for m, n in M.STORED_SHAPES] + [(2521, 1, [1], [2521])]
    d = _family(T, "sdp9")[0][0]
    return out + [(d.m, d.n, list(d.seg_type), list(d.seg_len))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", range(len(M.STORED_SHAPES) + 2))
def test_stored_form_is_the_numpy_restatement(T, case, kind):
    from totsu_amd import wide16batch as WW
    m, n, st, sl = _stored_cases(T)[case]
    mats = [M.planted(m, n, seed) for seed in range(2)]
    rng = np.random.default_rng(m + n)
    b, c = rng.standard_normal((2, m)).astype(F), rng.standard_normal((2, n)).astype(F)
    sb = T.Wide16BatchSolver(n, m, np.stack(mats), b, c, st, sl, W.param(T), a_dtype=kind)
    try:
        for i, a in enumerate(mats):
            words, inv = sb.stored_a(i)
            want_w, want_inv = M.stored(a, m, n, kind)
            assert words.shape == (n, M.ld16(m)) and words.dtype == np.uint16
            assert np.array_equal(words, want_w), (i, np.argwhere(words != want_w)[:4])
            assert not words[:, m:].any()                          # the pad rows
            if kind == "f16":
                assert np.array_equal(inv, want_inv), (i, inv, want_inv)
            else:
                assert inv is None
            assert np.array_equal(sb.widened(i), M.widen(want_w, want_inv, m))
            got = words.nbytes + (0 if inv is None else inv.nbytes)
            assert WW.store_bytes(n, m, kind) == (got + 15) // 16 * 16 == M.store_bytes(n, m, kind)
        assert sb.info()["a_store_bytes"] == 2 * M.store_bytes(n, m, kind)
        assert sb.mats_a is None                                   # the f32 upload is gone
    finally:
        sb.destroy()


# ---- 2. the twin on the family layouts -----------------------------------------------------------------------------------------------

LAYOUTS = ["lp20", "lp80", "lp260", "socp60", "qp", "sdp9", "sdp33", "sdp48", "part23", "mixed"]
WALK = (0, 1, 2, 10, 50)


def _walk(T, sb):
    out, done = [W.state(T, sb)], 0
    for it in WALK[1:]:
        sb.run(it - done, poll_every=64)
        done = it
        out.append(W.state(T, sb))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("threads,arith", PARAMS)
@pytest.mark.parametrize("name", LAYOUTS)
def test_twin_on_family_layouts(T, name, threads, arith, kind):
    ds, _ = _family(T, name)
    n, m = ds[0].n, ds[0].m
    p = W.param(T, state_arith=arith)
    sb, tw = W.pair(T, ds, kind, p, force_threads=threads)
    mid = None
    try:
        assert sb.info()["threads"] == tw.info()["threads"] == threads
        got, want = _walk(T, sb), _walk(T, tw)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g[0].shape == (len(ds), 6 * n + 11 * m)
            W.same_state(g, w, (name, threads, arith, kind, "after %d iterations" % WALK[k]))
        assert all(s.iters == 50 for s in sb.statuses())
        if 4 not in list(ds[0].seg_type):              # no PSD cone and a shape the mid batch takes: a Mid16BatchSolver's bits too
            mid = T.Mid16BatchSolver.from_dense(ds, p, a_dtype=kind, force_threads=threads)
            for k, w in enumerate(_walk(T, mid)):
                W.same_state(got[k], w, (name, threads, arith, kind, "mid16 after %d iterations" % WALK[k]), floats=6 * n + 10 * m)
    finally:
        _destroy(sb, tw, *([mid] if mid is not None else []))


# ---- 3. the twin beyond the old rules ------------------------------------------------------------------------------------------------

BEYOND = ["lp2521x1", "lp2x4096", "lp4096x3", "lp2020x40", "socp2600", "mixed64", "sdp48n837"]


def _twin_after(T, ds, kind, iters, p=None, **kw):
    sb, tw = W.pair(T, ds, kind, p or W.param(T), **kw)
    try:
        assert sb.info()["load_bytes"] == 8
        done = 0
        for it in iters:
            W.both(lambda s: s.run(it - done, poll_every=64), sb, tw)
            done = it
            assert all(s.iters == it for s in sb.statuses())
            W.same_state(W.state(T, sb), W.state(T, tw), "after %d" % it)
        return sb.info()
    finally:
        _destroy(sb, tw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", BEYOND)
def test_twin_beyond_the_old_rules(T, name, kind):
    ds, max_k = W.wide_case(T, name)
    n, m = ds[0].n, ds[0].m
    assert len(ds) == 2
    assert (W.old_rule(n, m, max_k) > W.LDS) == (name in ("lp4096x3", "socp2600", "mixed64", "sdp48n837")), name
    info = _twin_after(T, ds, kind, (0, 1, 10))
    assert info["lds_bytes"] == info["lds_bytes_per_problem"] == W.rule(n, m, max_k) <= W.LDS and info["max_psd_order"] == max_k
    assert info["threads"] == (1024 if m * n > 8192 else 256)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n,threads", M.EDGE_SHAPES)
def test_twin_on_the_edge_shapes_of_the_tiling(T, m, n, threads, kind):
    """every tiling constant of the pass at C - 1, C, C + 1"""
    ds = [_edge(m, n, s) for s in range(2)]
    _twin_after(T, ds, kind, (0, 1, 10), **({"force_threads": threads} if threads else {}))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("arith", ["compensated", "plain"])
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("name", ["lp2020x40", "socp2600", "mixed64"])
def test_twin_beyond_every_workgroup_size_and_arithmetic(T, name, threads, arith, kind):
    ds, _ = W.wide_case(T, name)
    info = _twin_after(T, ds, kind, (0, 1, 10), W.param(T, state_arith=arith), force_threads=threads)
    assert info["threads"] == threads


# ---- 4. the oracle on W --------------------------------------------------------------------------------------------------------------

_ON_W = {}


def _oracle_on_w(T, name, kind):
    """(the problems, the problems with the widened matrices of the numpy restatement -- which test 1 holds the device to --, the f64
    oracle's runs on those), computed once"""
    if (name, kind) not in _ON_W:
        ds, _ = W.wide_case(T, name)
        wds = [M.WDense(d, M.widened_of(d.mat_a, d.m, d.n, kind)) for d in ds]
        ros = [_oracle(wd, ITERS) for wd in wds]
        for ro in ros:
            assert ro.status == O.EXCESS_ITER and len(ro.trace) > max(ITERS)
        _ON_W[(name, kind)] = (ds, wds, ros)
    return _ON_W[(name, kind)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["lp2020x40", "mixed64"])
def test_iterates_against_the_oracle_on_w(T, name, kind):
    ds, wds, ros = _oracle_on_w(T, name, kind)
    # the precondition: the f32 twin on W passes the same call (if it does not, the case is wrong, not the tolerance)
    check_against_oracle(T, T.WideBatchSolver, "%s/%s/f32 twin" % (name, kind), wds, ros, ITERS, TOLS)
    info = check_against_oracle(T, T.Wide16BatchSolver, "%s/%s" % (name, kind), ds, ros, ITERS, TOLS, a_dtype=kind)
    assert info["a_dtype"] == kind


# ---- 5. the largest shape ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_largest_shape(T, kind):
    """4096 x 4096, one problem, iterates 0 and 1, bitwise against the twin (which the wide suite holds to the oracle)"""
    from totsu_amd import wide16batch as WW
    d = _edge(4096, 4096, 0)
    sb, tw = W.pair(T, [d], kind, W.param(T))
    try:
        info = sb.info()
        assert info["lds_bytes"] == 127232 and info["threads"] == 1024
        assert info["a_store_bytes"] == WW.store_bytes(4096, 4096, kind) == M.store_bytes(4096, 4096, kind)
        for it in (0, 1):
            W.both(lambda s: s.run(1, poll_every=1), sb, tw)
            W.same_state(W.state(T, sb), W.state(T, tw), "4096 x 4096, iterate %d" % it)
    finally:
        _destroy(sb, tw)


# ---- 6. independence -----------------------------------------------------------------------------------------------------------------

SMALL_BEYOND = (2640, 2)          # 8 n + 13 m = 34 336 floats and the class bytes: beyond the mid batch's map


@pytest.mark.parametrize("kind", KINDS)
def test_index_and_neighbours_change_nothing(T, kind):
    """P = 300 problems (more workgroups than CUs) cycled from 3: every copy holds the bits of its original, at any index, and the
    originals hold the twin's"""
    from totsu_amd import _lib
    m, n = SMALL_BEYOND
    assert W.old_rule(n, m) > W.LDS
    P = 300
    ds = [_edge(m, n, s) for s in range(3)]
    pick = [i % 3 for i in range(P)]
    a = np.stack([ds[k].mat_a for k in pick])
    b, c = np.stack([ds[k].vec_b for k in pick]), np.stack([ds[k].vec_c for k in pick])
    p = W.param(T)
    sb = T.Wide16BatchSolver(n, m, a, b, c, [_lib.CONE_RPOS], [m], p, a_dtype=kind)
    tw = T.WideBatchSolver.from_dense(W.widened_problems(sb, ds), p)
    try:
        W.both(lambda s: s.run(50, poll_every=25), sb, tw)
        got, want = W.state(T, sb), W.state(T, tw)
        for i in range(P):
            k = i % 3
            assert np.array_equal(got[0][i].view(np.uint32), want[0][k].view(np.uint32)), i
            assert repr(got[1][i]) == repr(want[1][k]), i
            for u, v in zip(got[2][i] + got[3][i], want[2][k] + want[3][k]):
                assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), i
    finally:
        _destroy(sb, tw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["lp2020x40", "mixed64"])
def test_launch_cuts_change_nothing(T, name, kind):
    """50 iterations as launches of 1, of 7, of 64, and as runs of 1 + 9 + 40: the bits of one run of 50"""
    ds, _ = W.wide_case(T, name)
    p = W.param(T)

    def run(cuts, poll):
        sb = T.Wide16BatchSolver.from_dense(ds, p, a_dtype=kind)
        try:
            for steps in cuts:
                sb.run(steps, poll_every=poll)
            assert all(s.iters == 50 for s in sb.statuses())
            return W.state(T, sb), sb.info()["launches"]
        finally:
            sb.destroy()

    want, l64 = run([50], 64)
    assert l64 == 1
    for poll, launches in ((1, 50), (7, 8)):
        got, l = run([50], poll)
        assert l == launches
        W.same_state(got, want, "%s/%s poll %d" % (name, kind, poll))
    got, l = run([1, 9, 40], 64)
    assert l == 3
    W.same_state(got, want, "%s/%s cut 1 + 9 + 40" % (name, kind))


# ---- 7. the round calls --------------------------------------------------------------------------------------------------------------

def _round_problems():
    m, n = SMALL_BEYOND
    return [_edge(m, n, 40 + s) for s in range(6)]


def _check_round(T, sb, tw, what, steps=9):
    W.same_state(W.state(T, sb), W.state(T, tw), what)
    W.both(lambda s: s.run(steps, poll_every=4), sb, tw)
    W.same_state(W.state(T, sb), W.state(T, tw), what + " + %d" % steps)


@pytest.mark.parametrize("kind", KINDS)
def test_replace_host_and_device(T, kind):
    ds = _round_problems()
    m, n = SMALL_BEYOND
    sb, tw = W.pair(T, ds[:3], kind, W.param(T))
    try:
        W.both(lambda s: s.run(5, poll_every=5), sb, tw)
        held = sb.info()["device_bytes"]
        sb.replace(1, ds[3].mat_a, ds[3].vec_b, ds[3].vec_c)
        assert sb.info()["device_bytes"] == held                     # converted into the slot's block: nothing allocated
        assert np.array_equal(sb.widened(1), M.widened_of(ds[3].mat_a, m, n, kind))
        assert np.array_equal(sb.widened(0), M.widened_of(ds[0].mat_a, m, n, kind))      # the neighbours' blocks stay
        tw.replace(1, sb.widened(1), ds[3].vec_b, ds[3].vec_c)
        assert sb.status(1).iters == 0 and sb.status(0).iters == 5
        _check_round(T, sb, tw, "replace from the host")
        da = T.DeviceBuffer.from_host(ds[4].mat_a)
        sb.replace(2, da, ds[4].vec_b, ds[4].vec_c)
        tw.replace(2, M.widened_of(ds[4].mat_a, m, n, kind), ds[4].vec_b, ds[4].vec_c)
        _check_round(T, sb, tw, "replace from a DeviceBuffer")
        da.free()
    finally:
        _destroy(sb, tw)


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("route", ["host", "dev"])
@pytest.mark.parametrize("kind", KINDS)
def test_set_a(T, kind, route, keep):
    """new values of A for slots 1 and 2: the twin handed the widened new A"""
    ds = _round_problems()
    m, n = SMALL_BEYOND
    sb, tw = W.pair(T, ds[:4], kind, W.param(T))
    try:
        W.both(lambda s: s.run(5, poll_every=5), sb, tw)
        new = [ds[4].mat_a, ds[0].mat_a * F(1.5)]
        if route == "host":
            sb.set_a(new, first=1, keep_iterate=keep)
        else:
            held = sb.info()["device_bytes"]
            dv = T.DeviceBuffer.from_host(np.concatenate(new))
            sb.set_a_dev(dv, first=1, count=2, keep_iterate=keep)
            assert sb.info()["device_bytes"] == held
            dv.free()
            with pytest.raises(ValueError, match="no f32 A lies in place"):
                sb.set_a_dev(None)
        wn = [M.widened_of(a, m, n, kind) for a in new]
        assert np.array_equal(sb.widened(1), wn[0]) and np.array_equal(sb.widened(2), wn[1])
        assert np.array_equal(sb.widened(0), M.widened_of(ds[0].mat_a, m, n, kind))
        tw.set_a(wn, first=1, keep_iterate=keep)
        assert [s.iters for s in sb.statuses()] == [5, 0, 0, 5]
        _check_round(T, sb, tw, "set_a %s keep %s" % (route, keep))
    finally:
        _destroy(sb, tw)


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_set_bc(T, kind, keep):
    ds = _round_problems()
    sb, tw = W.pair(T, ds[:3], kind, W.param(T))
    try:
        W.both(lambda s: s.run(6, poll_every=6), sb, tw)
        nb, nc = [d.vec_b for d in ds[3:]], [d.vec_c * F(1.25) for d in ds[3:]]
        W.both(lambda s: s.set_bc(nb, nc, keep_iterate=keep), sb, tw)
        assert all(s.iters == 0 for s in sb.statuses())
        _check_round(T, sb, tw, "set_bc keep %s" % keep)
        db, dc = T.DeviceBuffer.from_host(np.concatenate(nb[::-1])), T.DeviceBuffer.from_host(np.concatenate(nc[::-1]))
        W.both(lambda s: s.set_bc_dev(db, dc, keep_iterate=keep), sb, tw)
        _check_round(T, sb, tw, "set_bc_dev keep %s" % keep, steps=3)
        for d in (db, dc):
            d.free()
    finally:
        _destroy(sb, tw)


@pytest.mark.parametrize("kind", KINDS)
def test_set_iterates_and_solutions(T, kind):
    ds = _round_problems()[:3]
    sb, tw = W.pair(T, ds, kind, W.param(T))
    try:
        W.both(lambda s: s.run(20, poll_every=20), sb, tw)
        xs, ys = zip(*[sb.raw_iterate((i + 1) % 3) for i in range(3)])
        W.both(lambda s: s.set_iterates(xs, ys), sb, tw)
        assert all(s.iters == 0 for s in sb.statuses())
        _check_round(T, sb, tw, "set_iterates", steps=7)
        dx, dy = T.DeviceBuffer.from_host(np.concatenate(xs)), T.DeviceBuffer.from_host(np.concatenate(ys))
        W.both(lambda s: s.set_iterates_dev(dx, dy), sb, tw)
        _check_round(T, sb, tw, "set_iterates_dev", steps=7)
        dx.free()
        dy.free()
        sols = sb.solutions()
        for i, (x, y) in enumerate(sols):
            x1, y1 = sb.solution(i)
            assert np.array_equal(x, x1) and np.array_equal(y, y1)
        gx, gy, gs = sb.solutions_dev()
        assert np.array_equal(gx.to_host(), np.concatenate([x for x, _ in sols]))
        assert np.array_equal(gy.to_host(), np.concatenate([y for _, y in sols]))
        assert list(gs.to_host().view(np.int32)) == [r.state for r in sb.statuses()]
        for d in (gx, gy, gs):
            d.free()
    finally:
        _destroy(sb, tw)


# ---- 8. stop conditions --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_independent_termination_in_lockstep_with_the_twin(T, kind):
    from totsu_amd import _lib
    P = 18
    ds = [_term_problem(i) for i in range(P)]
    p = W.param(T, max_iter=100000, eps_acc=1e-5, eps_inf=1e-5)
    sb, tw = W.pair(T, ds, kind, p)
    try:
        live = [P]
        while True:
            res = sb.run_until_any(8, poll_every=8)
            tw.run_until_any(8, poll_every=8)
            live.append(sb.info()["live"])
            W.same_state(W.state(T, sb), W.state(T, tw), "a problem that stops inside a launch leaves the twin's state")
            if all(r.state != _lib.ST_RUNNING for r in res):
                break
            assert len(live) < 200
        assert live[-1] == 0 and len(set(live)) >= 3 and live == sorted(live, reverse=True)
        assert len(set(r.state for r in res)) == 3 and len(set(r.iters for r in res)) >= 3
    finally:
        _destroy(sb, tw)


_PADDED = {}


@pytest.mark.parametrize("name,kind", [("F1", "bf16"), ("F5", "f16")])
def test_tau_zero_families_end_as_the_twin(T, name, kind):
    """the tau -> 0 families padded to m = 2600: the verdict, the criteria and the iteration count of the twin"""
    if name not in _PADDED:
        _PADDED[name] = W.padded(Z.family(name))
    fam = _PADDED[name]
    assert fam.m == W.PAD_M
    ds = [_dense_of(fam)]
    p = W.param(T, max_iter=100_000, eps_acc=Z.EPS, eps_inf=Z.EPS)
    sb, tw = W.pair(T, ds, kind, p)
    try:
        r16, r32 = sb.run(-1, poll_every=25), tw.run(-1, poll_every=25)
        print("tau_zero wide16/%s/%s: %s" % (name, kind, [(r.state, r.iters, r.kind, r.cri) for r in r16]))
        assert all(r.state != -1 for r in r16)
        assert [(r.state, r.iters, r.kind, r.tau, tuple(r.cri)) for r in r16] == [(r.state, r.iters, r.kind, r.tau, tuple(r.cri)) for r in r32]
        W.same_state(W.state(T, sb), W.state(T, tw), "tau zero %s" % name)
    finally:
        _destroy(sb, tw)


# ---- 9. refusals and info ------------------------------------------------------------------------------------------------------------

def test_refusals_leave_nothing_allocated(T):
    from totsu_amd import _lib
    from totsu_amd._lib import lib
    S = T.Wide16BatchSolver
    z = lambda *s: np.zeros(s, F)
    ds, _ = _family(T, "lp80")
    keep = S.from_dense(ds)
    before = keep.info()["device_bytes_all"]
    assert before == keep.info()["device_bytes"] > keep.info()["a_store_bytes"] > 0 and keep.info()["a_dtype"] == "f16"
    t33 = tri(33)
    shape_refusals = [((2, 4097, [1], [4097]), "1 <= m <= 4096"), ((4097, 2, [1], [2]), "1 <= n <= 4096"),
                      ((2987, 4096, [_lib.CONE_PSD, 1], [t33, 4096 - t33]), "do not fit the LDS"),
                      ((3, 7, [_lib.CONE_PSD], [7]), "triangular"), ((3, tri(65), [_lib.CONE_PSD], [tri(65)]), "above 64")]
    for (n, m, st, sl), word in shape_refusals:                     # wb_check's refusals, in wb_check's words
        with pytest.raises(ValueError, match=word):
            S(n, m, z(1, 1), z(1, m), z(1, n), st, sl)
        with pytest.raises(ValueError, match=word):
            T.WideBatchSolver(n, m, z(1, 1), z(1, m), z(1, n), st, sl)
    bad = [lambda: S(3, 6, z(2, 18), z(2, 6), z(2, 3), [1], [6], a_dtype="f8"),
           lambda: S(3, 6, z(2, 18), z(2, 6), z(2, 3), [1], [5]),
           lambda: S(3, 6, z(2, 17), z(2, 6), z(2, 3), [1], [6]),
           lambda: S(3, 6, z(2, 18), z(2, 6), z(3, 3), [1], [6]),
           lambda: keep.set_a_dev(None),
           lambda: keep.set_a([z(5)], first=0),
           lambda: keep.replace(0, z(5), ds[0].vec_b, ds[0].vec_c)]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    with pytest.raises(ValueError, match="f32 A is WideBatchSolver"):
        S(3, 6, z(2, 18), z(2, 6), z(2, 3), [1], [6], a_dtype="f32")
    with pytest.raises(ValueError, match="Wide16BatchSolver holds a 16-bit copy"):
        keep.set_a_dev(None)
    assert keep.info()["device_bytes_all"] == before
    # the C ABI itself
    da, db, dc = (T.DeviceBuffer.from_host(z(64)) for _ in range(3))
    par = _lib.Param(-1, 1e-6, 1e-6, 1e-12, 0, 0, 0)

    def create(n, m, P, st, sl, kind, match):
        st, sl = np.asarray(st, np.int32), np.asarray(sl, np.int64)
        h = C.c_void_p()
        with pytest.raises(_lib.ThipError, match=match) as e:
            lib.thip_wide16batch_create_kind(n, m, P, da.ptr, db.ptr, dc.ptr, None, st.size, st.ctypes.data_as(C.POINTER(C.c_int32)),
                                             sl.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(par), kind, C.byref(h))
        assert e.value.code == _lib.E_INVALID and not h.value
        assert keep.info()["device_bytes_all"] == before

    for (n, m, st, sl), word in shape_refusals:
        create(n, m, 1, st, sl, M.A_F16, word)
    create(3, 6, 2, [1], [6], 0, "thip_widebatch")
    create(3, 6, 2, [1], [6], 3, "unknown stored form")
    create(3, 6, 2, [1], [5], M.A_BF16, "cover")
    create(3, 6, 0, [1], [6], M.A_F16, "wide16 batch holds")
    create(3, 6, 1048577, [1], [6], M.A_F16, "wide16 batch holds")
    with pytest.raises(_lib.ThipError, match="no f32 A lies in place"):
        lib.thip_wide16batch_set_a_dev(keep.h, 0, 1, None, 0)
    assert keep.info()["device_bytes_all"] == before
    for d in (da, db, dc):
        d.free()
    keep.run(3)
    assert all(keep.status(i).iters == 3 for i in range(len(ds)))     # and the batch is as it was: running
    sb2 = S.from_dense(ds[:2], a_dtype="bf16")
    assert sb2.info()["device_bytes_all"] == before + sb2.info()["device_bytes"]
    sb2.destroy()
    assert keep.info()["device_bytes_all"] == before
    keep.destroy()


@pytest.mark.parametrize("kind", KINDS)
def test_info_reports_the_rule_and_the_store(T, kind):
    """an order-64 cone: the operands behind the class bytes are part of what info() and fits report; the handle holds the store and
    no f32 copy of A"""
    from totsu_amd import wide16batch as WW
    ds, max_k = W.wide_case(T, "mixed64")
    n, m, P = ds[0].n, ds[0].m, len(ds)
    p = W.param(T)
    sb = T.Wide16BatchSolver.from_dense(ds, p, a_dtype=kind)
    f32 = T.WideBatchSolver.from_dense(ds, p)
    try:
        i16, i32 = sb.info(), f32.info()
        assert (i16["max_psd_order"], i16["n_psd"], i16["psd_lds_bytes"]) == (64, 2, 49920)
        assert i16["lds_bytes"] == i16["lds_bytes_per_problem"] == W.rule(n, m, 64) == WW.fits(n, m, ds[0].seg_type, ds[0].seg_len)[0]
        assert i16["lds_bytes"] == i32["lds_bytes"] and i16["threads"] == i32["threads"]
        assert i16["arena_bytes_per_problem"] == 4 * (6 * n + 11 * m) and i16["arena_bytes"] == P * 4 * (6 * n + 11 * m) == i32["arena_bytes"]
        per = 2 * M.ld16(m) * n + (4 * n if kind == "f16" else 0)
        assert (i16["a_dtype"], i16["load_bytes"], i16["a_bytes_per_iter"]) == (kind, 8, 2 * per)
        assert i16["a_store_bytes"] == P * M.store_bytes(n, m, kind)
        # what the handle holds beyond an f32 handle of the same problems is the store, to the byte; the f32 stack is not kept
        assert i16["device_bytes"] - i32["device_bytes"] == i16["a_store_bytes"]
        assert sb.mats_a is None
    finally:
        _destroy(sb, f32)


# ---- 10. the mixed route -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_mixed_route_into_the_exact_batch(T, kind):
    """20 iterations in 16 bits, the raw iterate into an f32 batch over the EXACT matrices, 20 more: bit for bit the same f32 batch
    handed the twin's raw iterate"""
    ds, _ = _family(T, "lp260")
    p = W.param(T)
    sb, tw = W.pair(T, ds, kind, p)
    exact = [T.WideBatchSolver.from_dense(ds, p) for _ in range(2)]
    try:
        W.both(lambda s: s.run(20, poll_every=20), sb, tw)
        for src, dst in zip((sb, tw), exact):
            xs, ys = zip(*[src.raw_iterate(i) for i in range(len(ds))])
            dst.set_iterates(xs, ys)
            dst.run(20, poll_every=20)
        assert all(s.iters == 20 for s in exact[0].statuses())
        W.same_state(W.state(T, exact[0]), W.state(T, exact[1]), "mixed route %s" % kind)
    finally:
        _destroy(sb, tw, *exact)
