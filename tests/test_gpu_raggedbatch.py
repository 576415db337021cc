"""GPU: problems of different shapes and cone layouts in ONE batch (totsu_amd.RaggedBatchSolver / thip_raggedbatch_*).  A problem of
a ragged batch must hold, bit for bit, what a MidBatchSolver -- an SdpBatchSolver when its layout has a PSD segment -- holds that
was given this problem alone: at every workgroup size, for both state arithmetics, whatever its index, its neighbours, its class's
live list, the alignment of its A and the launch cuts.  The same batch against the f64 oracle at the project's iterates and
tolerances, every cone layout of tests/cone_layouts.py the shape rule takes in one batch, independent termination with the launch
counters of both classes, the tau -> 0 verdicts, the largest LDS map, replace, the refusals.

The problems and their oracle runs are those of tests/ownbatch_cases.py and tests/cone_layouts.py; the uniform family's runs are
computed once per (workgroup size, state arithmetic) and shared.

The set (m x n): lp40[0] 80 x 40 (256 threads), lp80[0] 160 x 80 (1024), 128 x 64 (m n = 8192: 256) and 3 x 2731 (m n = 8193 =
3 * 2731: 1024 -- with 2731 ROWS the vectors alone exceed the LDS of a CU and the shape rule refuses the problem, so the far side
of the thread rule is reached with 2731 columns), socp60[0] 423 x 60 (m odd: 4-byte loads; row sums), socp[0] 102 x 12, a 102 x 12
nonnegative LP (the same shape, another layout), qp[0] 27 x 13, sdp9[0] 45 x 6, mixed[0] 812 x 5 (eight PSD cones of orders 1 .. 33
behind three nonnegative rows: the operand tail behind the class bytes), 1 x 1.  The 588 x 64 problem with orders 6 and 33 is
family F5 of tests/tau_zero_problems.py: it sits in the batch of test 7."""
import copy
import ctypes as C

import numpy as np
import pytest

import cone_layouts as CL
import tau_zero_problems as Z
from ownbatch_cases import (F, ITERS, SDP_ITERS, SDP_TOLS, TOLS, T, _dense_of, _edge, _oracle, _same, _snap, _View)  # noqa: F401
from ownbatch_cases import family as _family

pytestmark = pytest.mark.gpu

PSD = 4
STEPS = (1, 2, 10, 50)                       # the iteration counts of the bitwise comparisons
SET = [("lp40", 0), ("lp80", 0), ("edge", (128, 64)), ("edge", (3, 2731)), ("socp60", 0), ("socp", 0), ("edge", (102, 12)), ("qp", 0),
       ("sdp9", 0), ("mixed", 0), ("edge", (1, 1))]
_EDGE_RUNS, _REFS = {}, {}


def _problem(T, j):
    """(the dense problem, its oracle run, the iterates and tolerances the project compares its kind at)"""
    name, k = SET[j]
    if name == "edge":                        # tests/test_gpu_midbatch.py::test_edge_shapes: iterates 0 and 1
        if k not in _EDGE_RUNS:
            d = _edge(k[0], k[1], 0)
            _EDGE_RUNS[k] = (d, _oracle(d, ITERS[:2]))
        return _EDGE_RUNS[k] + (ITERS[:2], TOLS[:2])
    ds, ros = _family(T, name)
    sdp = PSD in ds[k].seg_type
    return ds[k], ros[k], SDP_ITERS if sdp else ITERS, SDP_TOLS if sdp else TOLS


def _set(T):
    return [_problem(T, j)[0] for j in range(len(SET))]


def _param(T, arith=None, **kw):
    p = T.SolverParam()
    p.eps_acc = 1e-30
    if arith:
        p.state_arith = arith
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _alone(T, d, p, force=None):
    """the uniform family holding d alone"""
    cls = T.SdpBatchSolver if PSD in d.seg_type else T.MidBatchSolver
    kw = {} if force is None else {"force_threads": force}
    return cls.from_dense([d], p, **kw)


def _full(sb, i):
    return _snap(sb, i) + sb.precond(i)


def _same_full(g, w, what=None):
    assert g[2] == w[2], (what, g[2], w[2])
    for u, v in zip(g[:2] + g[3:], w[:2] + w[3:]):
        assert u.shape == v.shape and np.array_equal(u, v), what


def _walk(sb, idx, steps=STEPS, poll=64):
    """{iteration count: [what problem i holds then, for i in idx]}"""
    out, done = {}, 0
    for s in steps:
        sb.run(s - done, poll_every=poll)
        done = s
        out[s] = [_full(sb, i) for i in idx]
    return out


def _ref(T, force=None, arith=None):
    """per problem of the set: {iteration count: what the uniform family holds for it alone}; computed once"""
    key = (force, arith)
    if key not in _REFS:
        out = []
        for d in _set(T):
            sb = _alone(T, d, _param(T, arith), force)
            out.append({s: v[0] for s, v in _walk(sb, [0]).items()})
            sb.destroy()
        _REFS[key] = out
    return _REFS[key]


# ---- 1. bit for bit the uniform family, problem by problem -----------------------------------------------------------------------

@pytest.mark.parametrize("arith", [None, "plain"])
@pytest.mark.parametrize("force", [None, 256, 1024])
def test_every_problem_has_the_uniform_family_s_bits(T, force, arith):
    ds, want = _set(T), _ref(T, force, arith)
    rb = T.RaggedBatchSolver.from_dense(ds, _param(T, arith), **({} if force is None else {"force_threads": force}))
    try:
        assert rb.shapes == [(d.n, d.m) for d in ds]
        info = rb.info()
        want_cls = [int((force or (256 if d.m * d.n <= 8192 else 1024)) == 1024) for d in ds]
        assert [c["n_prob"] for c in info["classes"]] == [want_cls.count(0), want_cls.count(1)]
        assert [c["threads"] for c in info["classes"]] == [256, 1024]
        if force is None:
            assert want_cls == [0, 1, 0, 1, 1, 0, 0, 0, 0, 0, 0]
        assert info["n_layouts"] == len(ds) and info["n_prob"] == info["live"] == len(ds)      # all distinct
        assert info["n_load16"] == sum(d.m % 4 == 0 for d in ds) == 4                # every A lies at a multiple of 4 floats
        assert info["a_bytes_per_iter"] == sum(8 * d.m * d.n for d in ds)
        assert info["arena_bytes"] == 4 * sum(6 * d.n + 10 * d.m for d in ds)
        for s, got in _walk(rb, range(len(ds))).items():
            for j, g in enumerate(got):
                assert g[2][1] == s
                _same_full(g, want[j][s], (SET[j], s, force, arith))
    finally:
        rb.destroy()


# ---- 2. independence: index, neighbours, the class's live list, the launch cuts ----------------------------------------------------

@pytest.mark.parametrize("how,poll", [("permuted", 7), ("cycled", 64), ("as is", 1)])
def test_a_problem_does_not_depend_on_the_batch_around_it(T, how, poll):
    ds, want = _set(T), _ref(T)
    if how == "permuted":
        order = [int(j) for j in np.random.default_rng(5).permutation(len(ds))]
    elif how == "cycled":
        order = [q % len(ds) for q in range(300)]                 # more workgroups than the device has CUs
    else:
        order = list(range(len(ds)))
    rb = T.RaggedBatchSolver.from_dense([ds[j] for j in order], _param(T))
    try:
        rb.run(STEPS[-1], poll_every=poll)
        cuts = -(-STEPS[-1] // poll)
        info = rb.info()
        assert [c["launches"] for c in info["classes"]] == [cuts, cuts] and info["launches"] == 2 * cuts
        assert info["workgroups"] == cuts * len(order)
        if how == "cycled":
            assert info["n_layouts"] == len(ds)
        for q, j in enumerate(order):
            _same_full(_full(rb, q), want[j][STEPS[-1]], (how, q, SET[j]))
    finally:
        rb.destroy()


# ---- 3. the alignment of A --------------------------------------------------------------------------------------------------------

def test_a_at_every_offset_mod_4_gives_the_same_bits(T):
    ds, want = _set(T), _ref(T)
    d = ds[1]                                                      # lp80[0]: m = 160
    size = d.m * d.n
    at = [k * (size + 4) + k for k in range(4)]                    # float offsets 0, 1, 2, 3 mod 4
    host = np.zeros(at[-1] + size, F)
    for a in at:
        host[a:a + size] = d.mat_a
    base = T.DeviceBuffer.from_host(host)
    assert base.ptr % 16 == 0
    probs = []
    for a in at:
        q = copy.copy(d)
        q.mat_a = _View(T, base, a, size)
        probs.append(q)
    rb = T.RaggedBatchSolver(probs + [ds[4]], _param(T))           # and socp60[0]: m odd
    try:
        assert rb.info()["n_load16"] == 1
        rb.run(STEPS[-1], poll_every=16)
        for q in range(4):
            _same_full(_full(rb, q), want[1][STEPS[-1]], q)
        _same_full(_full(rb, 4), want[4][STEPS[-1]], "socp60")
    finally:
        rb.destroy()
        base.free()


# ---- 4. against the f64 oracle ----------------------------------------------------------------------------------------------------

def _against_oracle(rb, label, runs):
    """runs: per problem (dense, oracle run, iterates, tolerances).  The comparison of ownbatch_cases.check_against_oracle, each
    problem with its own lengths, iterates and tolerances"""
    for i, (d, ro, _, _) in enumerate(runs):
        N = d.n + 2 * d.m + 1
        t, s = rb.precond(i)
        assert t.size == N and s.size == d.n + d.m + 1
        et, es = np.abs(t / ro.precond[:N] - 1).max(), np.abs(s / ro.precond[N:] - 1).max()
        print("%s problem %d preconditioner: rel err tau %.2e sigma %.2e" % (label, i, et, es))
        assert np.allclose(t, ro.precond[:N], rtol=2e-5, atol=0), (i, et)
        assert np.allclose(s, ro.precond[N:], rtol=2e-5, atol=0), (i, es)
    done = 0
    for it in sorted(set(v for r in runs for v in r[2])):
        rb.run(it + 1 - done, poll_every=64)
        done = it + 1
        for i, (d, ro, iters, tols) in enumerate(runs):
            if it not in iters:
                continue
            q = list(iters).index(it)
            tol = tols[q]
            N = d.n + 2 * d.m + 1
            x, y = rb.iterate(i)
            rx, ry = ro.snaps[q][:N], ro.snaps[q][N:]
            sx, sy = max(np.abs(rx).max(), 1e-6), max(np.abs(ry).max(), 1e-6)
            ex, ey = np.abs(x - rx).max() / sx, np.abs(y - ry).max() / sy
            print("%s problem %d (%d x %d) iterate %d: err x %.2e y %.2e (tol %.0e)" % (label, i, d.m, d.n, it, ex, ey, tol))
            assert ex <= tol and ey <= tol, (i, it, ex, ey)
            st = rb.status(i)
            assert st.state == -1 and st.iters == it + 1
            tr = ro.trace[it]
            assert st.kind == tr[1]
            assert np.allclose(st.cri, tr[2:], rtol=max(50 * tol, 1e-3), atol=1e-5), (i, it, st.cri, tr)


def test_the_mixed_batch_against_the_oracle(T):
    runs = [_problem(T, j) for j in range(len(SET))]
    rb = T.RaggedBatchSolver.from_dense([r[0] for r in runs], _param(T))
    try:
        _against_oracle(rb, "ragged", runs)
    finally:
        rb.destroy()


# ---- 5. every cone layout the shape rule takes, side by side ------------------------------------------------------------------------

def test_cone_layouts_in_one_batch(T):
    """the layouts of tests/cone_layouts.py with all their seeds in ONE batch: ragged and short layouts beside each other, with
    different n_cones, zero included.  `long` (9107 rows) and `psd_big` (an order of 65) are beyond what one workgroup holds: the
    rule refuses them, here as in the SDP batch, and names them by index"""
    from totsu_amd import raggedbatch as RB
    taken, runs = [], []
    for name in CL.LAYOUTS:
        st, sl, _ = CL.segments(name)
        try:
            T.sdpbatch.fits(CL.LAYOUTS[name]["n"], sum(sl), st, sl)
        except ValueError:
            continue
        taken.append(name)
        iters, tols = CL.iters_tols(name)
        for seed in CL.LAYOUTS[name]["seeds"]:
            d, ro = CL.oracle(name, seed, 0, T=T)
            runs.append((d, ro, iters, tols))
    assert taken == ["small", "mid", "short_soc", "short_soc_rot", "psd"] and len(runs) == 14
    for name in ("long", "psd_big"):
        st, sl, _ = CL.segments(name)
        with pytest.raises(ValueError, match="problem 2:") as e:
            RB.fits([runs[0][0], runs[5][0], type("S", (), dict(n=CL.LAYOUTS[name]["n"], m=sum(sl), seg_type=st, seg_len=sl))()])
        assert e.value.problem == 2
    rb = T.RaggedBatchSolver.from_dense([r[0] for r in runs], _param(T))
    try:
        assert rb.info()["n_layouts"] == len(taken)
        _against_oracle(rb, "ragged layouts", runs)
    finally:
        rb.destroy()


# ---- 6. independent termination ---------------------------------------------------------------------------------------------------

def test_independent_termination_and_the_launch_counters(T):
    from totsu_amd import _lib
    POLL = 16
    ds = [_family(T, "lp40")[0][0], _family(T, "lp80")[0][0], _family(T, "qp")[0][0], _family(T, "lp80")[0][1], _family(T, "sdp9")[0][0],
          _family(T, "socp")[0][0], _family(T, "lp40")[0][1]]
    cls = [int(d.m * d.n > 8192) for d in ds]
    assert cls == [0, 1, 0, 1, 0, 0, 0]
    p = _param(T, eps_acc=1e-3, max_iter=100000)
    want = []
    for d in ds:
        sb = _alone(T, d, p)
        r = sb.run(-1, poll_every=POLL)[0]
        want.append((r.state, r.iters, r.kind, tuple(r.cri)) + sb.solution(0) + sb.iterate(0))
        sb.destroy()
    assert all(w[0] == _lib.ST_OK for w in want) and len(set(w[1] for w in want)) >= 4, [w[:2] for w in want]
    rb = T.RaggedBatchSolver.from_dense(ds, p)
    try:
        live = [sum(1 for c in cls if c == k) for k in (0, 1)]
        launches, groups, dead_at, calls, stopped = [0, 0], [0, 0], {}, 0, set()
        while sum(live):
            res = rb.run_until_any(-1, poll_every=POLL)
            calls += 1
            info = rb.info()
            now = [c["live"] for c in info["classes"]]
            polls = [c["launches"] - l for c, l in zip(info["classes"], launches)]
            # one launch per class with a live member per poll, workgroups equal to the live count; a class without one: none
            running = [k for k in (0, 1) if live[k]]
            assert len(set(polls[k] for k in running)) == 1 and polls[running[0]] >= 1, (polls, live)
            for k in (0, 1):
                assert polls[k] == (polls[running[0]] if live[k] else 0), (k, polls, live)
                assert info["classes"][k]["workgroups"] - groups[k] == polls[k] * live[k]
                if live[k] == 0:
                    assert info["classes"][k]["launches"] == dead_at[k]
                elif now[k] == 0:
                    dead_at[k] = info["classes"][k]["launches"]
            # back at the first stop: something that was running has stopped, and it stopped within the last launch
            new = {i for i, r in enumerate(res) if r.state != _lib.ST_RUNNING} - stopped
            assert new and sum(now) == sum(live) - len(new), (new, now, live)
            for i in new:
                total = info["classes"][cls[i]]["launches"]
                assert (total - 1) * POLL <= res[i].iters <= total * POLL, (i, res[i].iters, total)
            stopped |= new
            launches, groups, live = [c["launches"] for c in info["classes"]], [c["workgroups"] for c in info["classes"]], now
            assert info["live"] == sum(now) and calls <= len(ds)
        assert len(dead_at) == 2 and dead_at[0] != dead_at[1]                 # one class went on alone after the other had stopped
        assert info["launches"] == sum(launches) and info["workgroups"] == sum(groups)
        print("ragged termination: iterations", [r.iters for r in res], "launches per class", launches)
        for i, w in enumerate(want):
            st = rb.status(i)
            assert (st.state, st.iters, st.kind, tuple(st.cri)) == w[:4], (i, st.iters, w[1])
            for u, v in zip(rb.solution(i) + rb.iterate(i), w[4:]):
                assert u.shape == v.shape and np.array_equal(u, v), i
        for i, s_ in enumerate(rb.solve()):
            assert isinstance(s_, tuple) and s_[0].size == ds[i].n and s_[1].size == ds[i].m
    finally:
        rb.destroy()


# ---- 7. tau -> 0: each member's own verdict -----------------------------------------------------------------------------------------

def test_verdicts_among_feasible_problems_of_other_shapes(T):
    fams = [Z.family("F1"), Z.family("F2"), Z.family("F3"), Z.family("F4"), Z.family("F5")] + Z.family("F6")[1:]
    assert all(f.verdict in (Z.INFEASIBLE, Z.UNBOUNDED) for f in fams) and {f.verdict for f in fams} == {Z.INFEASIBLE, Z.UNBOUNDED}
    feas = [_family(T, "lp40")[0][0], _family(T, "sdp9")[0][0], _family(T, "socp")[0][0], _family(T, "qp")[0][0]]
    ds, verdict = [], []
    for k, f in enumerate(fams):                                   # F, feasible, F, feasible, ...
        ds.append(_dense_of(f))
        verdict.append(f.verdict)
        if k < len(feas):
            ds.append(feas[k])
            verdict.append(Z.OK)
    p = _param(T, max_iter=100000, eps_acc=Z.EPS, eps_inf=Z.EPS)
    rb = T.RaggedBatchSolver.from_dense(ds, p)
    try:
        res = rb.run(-1, poll_every=25)
        for i, (d, v) in enumerate(zip(ds, verdict)):
            sb = _alone(T, d, p)
            w = sb.run(-1, poll_every=25)[0]
            print("ragged tau_zero problem %d (%d x %d): state %d at %d kind %d (alone: %d at %d)" % (i, d.m, d.n, res[i].state, res[i].iters,
                                                                                                   res[i].kind, w.state, w.iters))
            assert w.state == v, (i, w.state, v)                   # (the uniform family's verdict is the family's)
            assert (res[i].state, res[i].iters, res[i].kind, res[i].cri, res[i].tau) == (w.state, w.iters, w.kind, w.cri, w.tau), i
            if v != Z.OK:
                assert res[i].kind == 1 and res[i].tau == 0.0
            for u, z in zip(rb.iterate(i) + rb.solution(i), sb.iterate(0) + sb.solution(0)):
                assert np.array_equal(u, z), i
            sb.destroy()
    finally:
        rb.destroy()


# ---- 8. the largest map beside the smallest ---------------------------------------------------------------------------------------

def test_largest_map_beside_the_smallest(T):
    big, one = _edge(2000, 1000, 0), _problem(T, len(SET) - 1)[0]
    assert (one.m, one.n) == (1, 1)
    p = _param(T)
    rb = T.RaggedBatchSolver.from_dense([big, one], p, force_threads=1024)
    try:
        info = rb.info()
        assert info["classes"][1]["lds_bytes"] == 162832 and info["classes"][1]["n_prob"] == 2 and info["classes"][0]["n_prob"] == 0
        got = _walk(rb, [0, 1], steps=(1, 2))
        for i, d in enumerate((big, one)):
            sb = _alone(T, d, p, 1024)
            for s, w in _walk(sb, [0], steps=(1, 2)).items():
                _same_full(got[s][i], w[0], (i, s))
            sb.destroy()
        assert rb.info()["classes"][0]["launches"] == 0 and rb.info()["classes"][1]["launches"] == 2
    finally:
        rb.destroy()


# ---- 9. replace and reinit --------------------------------------------------------------------------------------------------------

def test_replace_is_a_fresh_init_of_that_slot_alone(T):
    from totsu_amd import _lib
    lp40, lp80, sdp9, socp = (_family(T, k)[0] for k in ("lp40", "lp80", "sdp9", "socp"))
    p = _param(T, max_iter=40)
    held = [lp40[0], lp80[0], sdp9[0], socp[0]]

    def alone(d, steps):
        sb = _alone(T, d, p)
        sb.run(steps, poll_every=64)
        out = _full(sb, 0)
        sb.destroy()
        return out

    def data(d):
        return (d.mat_a, d.vec_b, d.vec_c) + ((d.vec_b_rowabs,) if d.vec_b_rowabs is not None else ())

    rb = T.RaggedBatchSolver.from_dense(held, p)
    try:
        rb.run(10, poll_every=4)
        rb.replace(1, *data(lp80[1]))                               # a running slot
        held[1] = lp80[1]
        st = rb.status(1)
        assert (st.state, st.iters) == (_lib.ST_RUNNING, 0) and rb.info()["live"] == 4
        _same_full(_full(rb, 1), alone(lp80[1], 0), "fresh")
        rb.run(5, poll_every=64)
        for i, steps in enumerate((15, 5, 15, 15)):
            _same_full(_full(rb, i), alone(held[i], steps), (i, steps))
        rb.run(-1, poll_every=64)
        assert [rb.status(i).state for i in range(4)] == [_lib.ST_EXCESS_ITER] * 4 and rb.info()["live"] == 0
        end = [_full(rb, i) for i in range(4)]
        rb.replace(2, *data(sdp9[1]))                               # stopped slots: one without, one with row sums
        rb.replace(3, *data(socp[1]))
        held[2], held[3] = sdp9[1], socp[1]
        assert socp[1].vec_b_rowabs is not None
        info = rb.info()
        assert info["live"] == 2 and [c["live"] for c in info["classes"]] == [2, 0]
        rb.run(7, poll_every=3)
        for i in (2, 3):
            _same_full(_full(rb, i), alone(held[i], 7), i)
        for i in (0, 1):                                            # no other slot's bits move
            _same_full(_full(rb, i), end[i], i)
            _same_full(end[i], alone(held[i], 100), i)
        with pytest.raises(ValueError):                             # arrays of another length: the slot keeps its shape
            rb.replace(0, lp80[0].mat_a, lp80[0].vec_b, lp80[0].vec_c)
        with pytest.raises(ValueError):
            rb.replace(0, lp40[0].mat_a, lp40[0].vec_b[:-1], lp40[0].vec_c)
        with pytest.raises(ValueError):
            rb.replace(4, *data(lp40[0]))
        rb.reinit()                                                 # every slot again, on the data it holds now
        assert rb.info()["live"] == 4 and rb.info()["launches"] == 0
        rb.run(3, poll_every=64)
        for i in range(4):
            _same_full(_full(rb, i), alone(held[i], 3), i)
    finally:
        rb.destroy()


# ---- 10. refusals: nothing allocated ----------------------------------------------------------------------------------------------

def test_refusals_leave_nothing_allocated(T):
    from totsu_amd import _lib
    from totsu_amd._lib import lib
    S = T.RaggedBatchSolver
    ds = _set(T)
    keep = S.from_dense(ds[:3])                        # something alive, so that device_bytes_all can be read before and after
    info = keep.info()
    before = info["device_bytes_all"]
    assert before == info["device_bytes"] > info["arena_bytes"] > 0
    z = lambda *s: np.zeros(s, F)

    def shape(n, m, st, sl):
        d = copy.copy(ds[0])
        d.n, d.m, d.seg_type, d.seg_len = n, m, st, sl
        d.mat_a, d.vec_b, d.vec_c, d.vec_b_rowabs = z(m * n), z(m), z(n), None
        return d

    refused = [shape(3, 2145, [PSD], [2145]),          # order 65
               shape(3, 7, [PSD], [7]),                # not triangular
               shape(2, 4097, [1], [4097]),            # 4097 rows
               shape(837, 1176, [PSD], [1176]),        # a map beyond LDS
               shape(3, 6, [PSD], [3])]                # segments that do not cover m
    for bad in refused:
        with pytest.raises(ValueError, match="problem 2:"):
            S.from_dense(ds[:2] + [bad] + ds[2:4])
    with pytest.raises(ValueError):                    # no problem at all
        S.from_dense([])
    for kind in ("mat_a", "vec_b", "vec_c"):           # arrays of the wrong length
        bad = copy.copy(ds[1])
        setattr(bad, kind, np.asarray(getattr(bad, kind))[:-1])
        with pytest.raises(ValueError, match="problem 1: %s" % kind):
            S.from_dense([ds[0], bad])
    bad = copy.copy(ds[4])
    bad.vec_b_rowabs = np.asarray(bad.vec_b_rowabs)[:-1]
    with pytest.raises(ValueError, match="problem 0: vec_b_rowabs"):
        S.from_dense([bad])
    # a device array that lies no whole number of floats from the others of its kind
    base = T.DeviceBuffer.from_host(z(2 * ds[0].m * ds[0].n + 8))

    class Skew(T.DeviceBuffer):
        def __init__(self, nbytes):
            self.n, self.ptr = ds[0].m * ds[0].n, base.ptr + nbytes

        def free(self):
            self.ptr = None
    a0, a1 = copy.copy(ds[0]), copy.copy(ds[0])
    a0.mat_a, a1.mat_a = Skew(0), Skew(4 * ds[0].m * ds[0].n + 2)
    with pytest.raises(ValueError, match="misaligned float offset"):
        S([a0, a1])
    assert keep.info()["device_bytes_all"] == before
    # the C ABI itself: THIP_E_INVALID, thip_last_error set, *out stays NULL, nothing allocated
    par = _lib.Param(-1, 1e-6, 1e-6, 1e-12, 0, 0, 0)
    db = T.DeviceBuffer.from_host(z(64))

    def create(n, m, st, sl, a_ptr=None, at=(0, 0), n_prob=None, null=None):
        P = len(n)
        arr = lambda v, t: np.asarray(v, t)
        n_, m_, ns = arr(n, np.uintp), arr(m, np.uintp), arr([len(s) for s in st], np.uintp)
        st_, sl_ = arr([t for s in st for t in s], np.int32), arr([t for s in sl for t in s], np.int64)
        at_ = arr((list(at) + [0] * P)[:P], np.int64)
        zero = np.zeros(P, np.int64)
        ps, p64 = C.POINTER(C.c_size_t), C.POINTER(C.c_int64)
        h = C.c_void_p()
        with pytest.raises(_lib.ThipError) as e:
            lib.thip_raggedbatch_create(P if n_prob is None else n_prob, n_.ctypes.data_as(ps), m_.ctypes.data_as(ps),
                                        db.ptr if a_ptr is None else a_ptr, None if null == "at_a" else at_.ctypes.data_as(p64), db.ptr,
                                        zero.ctypes.data_as(p64), db.ptr, zero.ctypes.data_as(p64), None, None,
                                        ns.ctypes.data_as(ps), st_.ctypes.data_as(C.POINTER(C.c_int32)), sl_.ctypes.data_as(p64),
                                        None if null == "par" else C.byref(par), C.byref(h))
        assert e.value.code == _lib.E_INVALID and not h.value and _lib.load().thip_last_error()
        assert keep.info()["device_bytes_all"] == before
        return str(e.value)

    ok = ([3, 2], [6, 4], [[PSD], [1]], [[6], [4]])
    assert "problem 1:" in create([3, 3], [6, 2145], [[PSD], [PSD]], [[6], [2145]])
    assert "problem 0:" in create([3, 3], [7, 6], [[PSD], [PSD]], [[7], [6]])
    assert "problem 1:" in create([3, 2], [6, 4097], [[PSD], [1]], [[6], [4097]])
    assert "problem 1:" in create([3, 837], [6, 1176], [[PSD], [PSD]], [[6], [1176]])
    assert "problem 1:" in create([3, 3], [6, 6], [[PSD], [PSD]], [[6], [3]])
    assert "problem 0:" in create([3, 3], [6, 6], [[9], [PSD]], [[6], [6]])
    create(*ok, n_prob=0)
    create(*ok, n_prob=1048577)
    create(*ok, a_ptr=db.ptr + 2)                      # a base that is no float address
    create(*ok, at=(0, -3))                            # an offset before the array
    create(*ok, null="at_a")
    create(*ok, null="par")
    db.free()
    base.free()
    with pytest.raises(_lib.ThipError) as e:           # force_threads after init
        lib.thip_test_raggedbatch_force_threads(keep.h, 256)
    assert e.value.code == _lib.E_INVALID
    with pytest.raises(ValueError):
        keep.replace(0, ds[1].mat_a, ds[1].vec_b, ds[1].vec_c)
    with pytest.raises(ValueError):
        keep.iterate(3)
    # no refusal left device memory behind: a later object is all the library holds beside the first
    rb2 = T.ragged_batch(ds[3:6])
    assert isinstance(rb2, S) and rb2.info()["device_bytes_all"] == before + rb2.info()["device_bytes"]
    assert all(r.iters == 3 for r in rb2.run(3))
    rb2.destroy()
    assert keep.info()["device_bytes_all"] == before
    keep.destroy()
