"""GPU: the wide batch (totsu_amd.WideBatchSolver / thip_widebatch_*) -- the SDP batch's iteration with all but the pass vectors left
in the problem's arena block, so that every shape to 4096 x 4096 and every PSD order to 64 is taken.
    1. bit for bit the mid / SDP batch on every family layout of tests/ownbatch_cases.py those take: arena, status blocks,
       solutions(), at both workgroup sizes, both state arithmetics and on the 4-byte load path;
    2. beyond the old rules, against the f64 oracle: iterates 0 / 1 / 9 / 99 and criteria at TOLS (check_against_oracle, unchanged);
    3. bitwise independence of index, neighbours, alignment of A and launch cuts;
    4. stop conditions: independent termination, the tau -> 0 families padded beyond the mid batch's rule;
    5. the round calls and their _dev twins; solutions against solution(i);
    6. refusals leave nothing allocated; info() reports the LDS bytes the rule predicts.
Every oracle state a test relies on is asserted first; references are computed once per session and never changed."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import tau_zero_problems as Z
from ownbatch_cases import (F, ITERS, TOLS, T, _D, _compare_snap, _dense_of, _edge, _mixed_dense, _oracle, _psd_block, _sdp_dense,  # noqa: F401
                            _socp_dense, _term_problem, _View, check_against_oracle, tri)
from ownbatch_cases import family as _family

pytestmark = pytest.mark.gpu

LDS = 163840


def rule(n, m, max_k=0):
    """the wide batch's LDS map (README.md, tests/test_widebatch_cpu.py)"""
    return 4 * (6208 + 3 * n + 3 * m) + ((m + 3) & ~3) + (49920 if max_k > 32 else 0)


def old_rule(n, m, max_k=0):
    """the mid / SDP batch's"""
    return 4 * (6208 + 8 * n + 13 * m) + ((m + 3) & ~3) + (49920 if max_k > 32 else 0)


def _param(T, **kw):
    p = T.SolverParam()
    p.eps_acc = 1e-30
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _arena(T, sb):
    """the whole arena of a batch as it lies on the device, one row per problem"""
    from totsu_amd._lib import lib
    addr, size = (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    lib.thip_test_ownbatch_addresses(sb.h, addr, size)
    assert addr[0] and size[0] == sb.info()["arena_bytes"]
    a = _View(T, type("B", (), {"ptr": addr[0]})(), 0, size[0] // 4).to_host()
    return a.reshape(sb.n_prob, -1)


def _blocks(sb):
    return [(s.state, s.iters, s.kind, s.cri, s.tau, s.kappa, s.norm_b, s.norm_c) for s in sb.statuses()]


def _state(T, sb):
    """everything a test compares bit for bit: the mid batch's part of every arena block, the status blocks, solutions()"""
    n, m = sb.n, sb.m
    return _arena(T, sb)[:, :6 * n + 10 * m].copy(), _blocks(sb), sb.solutions()


def _same_state(got, want, what):
    assert got[0].shape == want[0].shape and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (what, "arena")
    assert repr(got[1]) == repr(want[1]), (what, got[1], want[1])
    for (gx, gy), (wx, wy) in zip(got[2], want[2]):
        assert np.array_equal(gx.view(np.uint32), wx.view(np.uint32)) and np.array_equal(gy.view(np.uint32), wy.view(np.uint32)), what


# ---- 1. bit for bit on the shapes the mid or the SDP batch also takes ---------------------------------------------------------------

SHARED = ["lp20", "lp40", "lp80", "lp260", "socp", "socp60", "qp", "sdp9", "sdp24", "sdp33", "sdp48", "part23", "part44", "mixed"]


def _other(T, ds):
    return T.SdpBatchSolver if 4 in list(ds[0].seg_type) else T.MidBatchSolver


def _walk(T, cls, ds, p, **kw):
    sb = cls.from_dense(ds, p, **kw)
    out, done = [_state(T, sb)], 0
    for it in (1, 2, 10, 50):
        sb.run(it - done, poll_every=64)
        done = it
        out.append(_state(T, sb))
    info = sb.info()
    sb.destroy()
    return out, info


@pytest.mark.parametrize("arith", ["compensated", "plain"])
@pytest.mark.parametrize("threads", [256, 1024])
@pytest.mark.parametrize("name", SHARED)
def test_bit_for_bit_on_shared_shapes(T, name, threads, arith):
    ds, _ = _family(T, name)
    p = _param(T, state_arith=arith)
    want, wi = _walk(T, _other(T, ds), ds, p, force_threads=threads)
    got, gi = _walk(T, T.WideBatchSolver, ds, p, force_threads=threads)
    for k, (g, w) in enumerate(zip(got, want)):
        _same_state(g, w, (name, threads, arith, "after %s iterations" % (0, 1, 2, 10, 50)[k]))
    n, m = ds[0].n, ds[0].m
    assert gi["threads"] == wi["threads"] == threads and gi["load_bytes"] == wi["load_bytes"]
    assert gi["arena_bytes_per_problem"] == 4 * (6 * n + 11 * m) and gi["arena_bytes"] == len(ds) * 4 * (6 * n + 11 * m)
    assert gi["lds_bytes"] == gi["lds_bytes_per_problem"] == rule(n, m, gi["max_psd_order"]) < wi["lds_bytes"]


@pytest.mark.parametrize("name", ["lp80", "sdp24"])
def test_bit_for_bit_on_the_4_byte_load_path(T, name):
    """m % 4 == 0 with every A one float off a 16-byte boundary: both batches report the 4-byte path and hold the same bits -- which
    are those of the aligned run"""
    ds, _ = _family(T, name)
    p = _param(T)
    n, m = ds[0].n, ds[0].m
    assert m % 4 == 0
    a = np.stack([np.asarray(d.mat_a, F).ravel() for d in ds])
    b, c = np.stack([np.asarray(d.vec_b, F) for d in ds]), np.stack([np.asarray(d.vec_c, F) for d in ds])
    base = T.DeviceBuffer.from_host(np.concatenate([np.zeros(1, F), a.ravel()]))
    assert base.ptr % 16 == 0

    def run(cls, mats):
        sb = cls(n, m, mats, b, c, ds[0].seg_type, ds[0].seg_len, p)
        lb = sb.info()["load_bytes"]
        sb.run(10, poll_every=4)
        out = _state(T, sb)
        sb.destroy()
        return lb, out

    l4w, wide4 = run(T.WideBatchSolver, _View(T, base, 1, a.size))
    l4o, other4 = run(_other(T, ds), _View(T, base, 1, a.size))
    l16, wide16 = run(T.WideBatchSolver, a)
    base.free()
    assert (l4w, l4o, l16) == (4, 4, 16)
    _same_state(wide4, other4, name + " unaligned")
    _same_state(wide4, wide16, name + " unaligned against aligned")


# ---- 2. beyond the old rules, against the f64 oracle -----------------------------------------------------------------------------

def _check(T, label, ds, ros, iters, tols, max_k=0, **kw):
    n, m = ds[0].n, ds[0].m
    info = check_against_oracle(T, T.WideBatchSolver, label, ds, ros, iters, tols, **kw)
    assert info["lds_bytes"] == info["lds_bytes_per_problem"] == rule(n, m, max_k) <= LDS
    assert info["a_bytes_per_iter"] == 8 * m * n and info["max_psd_order"] == max_k
    assert info["load_bytes"] == (16 if m % 4 == 0 else 4)
    return info


_WIDE = {}


def _wide_case(T, name):
    """(problems, oracle runs at ITERS, largest PSD order), computed once"""
    if name in _WIDE:
        return _WIDE[name]
    from totsu_amd import _lib
    max_k, socp = 0, None
    if name.startswith("lp"):
        m, n = (int(v) for v in name[2:].split("x"))
        ds = [_edge(m, n, s) for s in range(2)]
    elif name == "socp2600":
        ds, socp = [], []
        for s in range(2):
            d, pieces = _socp_dense(T, 60, [5, 1, 0, 17, 1200, 1367, 3], s)
            assert (d.m, d.n) == (2600, 60)
            ds.append(d)
            socp.append(pieces)
    elif name == "mixed64":
        # 3 nonnegative rows, an order-64 and an order-5 PSD cone, a second-order cone of 9 rows and a rotated one of 5: n = 2
        n, max_k, ds = 2, 64, []
        for s in range(2):
            rng = np.random.default_rng(640 + s)
            blocks, bs, st, sl = [rng.standard_normal((3, n)).astype(F)], [np.abs(rng.standard_normal(3)).astype(F) + 1.0], [_lib.CONE_RPOS], [3]
            c0 = np.zeros(n, F)
            for q, k in enumerate((64, 5)):
                rows, b, c = _psd_block(T, n, k, 70 + q + 10 * s)
                blocks.append(rows)
                bs.append(b)
                st.append(_lib.CONE_PSD)
                sl.append(tri(k))
                c0 = c0 + c
            for t, rows in ((_lib.CONE_SOC, 9), (_lib.CONE_ROTSOC, 5)):
                blocks.append((rng.standard_normal((rows, n)) / 4).astype(F))
                b = (rng.standard_normal(rows) / 4).astype(F)
                b[0] = 3.0
                if t == _lib.CONE_ROTSOC:
                    b[1] = 3.0
                bs.append(b)
                st.append(t)
                sl.append(rows)
            ds.append(_D(np.vstack(blocks), np.concatenate(bs), c0 / 2, st, sl))
    else:
        assert name == "sdp48n837", name
        max_k, ds = 48, [_sdp_dense(T, 837, 48, 0)]
    ros = [_oracle(d, ITERS, socp=None if socp is None else socp[i]) for i, d in enumerate(ds)]
    for ro in ros:
        assert ro.status == O.EXCESS_ITER and len(ro.trace) > max(ITERS)
    _WIDE[name] = (ds, ros, max_k)
    return _WIDE[name]


# LPs 2521 x 1 (m n odd: the second slot's A is off a 16-byte boundary), 2 x 4096 and 4096 x 3, 2020 x 40, 1300 x 2100; an SOCP with
# m = 2600; a mixed layout with an order-64 PSD cone at n = 2; order 48 at n = 837
BEYOND = ["lp2521x1", "lp2x4096", "lp4096x3", "lp2020x40", "lp1300x2100", "socp2600", "mixed64", "sdp48n837"]


@pytest.mark.parametrize("name", BEYOND)
def test_iterates_beyond_the_old_rules(T, name):
    """iterates 0, 1, 9, 99, the criteria and the preconditioner against the f64 oracle at TOLS.  (2521 x 1, 2 x 4096 and 1300 x 2100
    lie beyond 8 n + 13 m <= 32 768 but inside the mid batch's map, which has 3072 floats to spare; 2020 x 40 is the mid batch's too:
    m = 2020 at a small n.  The others are refused by every batch before this one.)"""
    ds, ros, max_k = _wide_case(T, name)
    assert (old_rule(ds[0].n, ds[0].m, max_k) > LDS) == (name in ("lp4096x3", "socp2600", "mixed64", "sdp48n837")), name
    info = _check(T, name, ds, ros, ITERS, TOLS, max_k=max_k)
    assert info["threads"] == (1024 if ds[0].m * ds[0].n > 8192 else 256)


@pytest.mark.parametrize("threads,arith", [(256, "compensated"), (1024, "plain")])
@pytest.mark.parametrize("name", ["lp2020x40", "socp2600", "mixed64"])
def test_iterates_beyond_every_workgroup_size_and_arithmetic(T, name, threads, arith):
    ds, ros, max_k = _wide_case(T, name)
    _check(T, "%s/%d/%s" % (name, threads, arith), ds, ros, ITERS, TOLS, max_k=max_k, force_threads=threads, state_arith=arith)


def test_largest_shape(T):
    """4096 x 4096: 127 232 bytes of LDS, 64 MB of A; iterates 0 and 1 (as test_gpu_midbatch.py::test_floor_edge_shape)"""
    d = _edge(4096, 4096, 0)
    info = _check(T, "edge 4096x4096", [d], [_oracle(d, ITERS[:2])], ITERS[:2], TOLS[:2])
    assert info["lds_bytes"] == 127232 and info["threads"] == 1024


# ---- 3. bitwise independence -----------------------------------------------------------------------------------------------------

SMALL_BEYOND = (2640, 2)          # 8 n + 13 m = 34 336 floats and the class bytes: beyond the mid batch's map


def test_isolation_and_reproducibility(T):
    """P = 300 problems of 2640 x 2 (more workgroups than CUs), the same LP at index 0 and at index 299: its iterates are those of
    the LP alone, run after run"""
    from totsu_amd import _lib
    m, n = SMALL_BEYOND
    assert old_rule(n, m) > LDS
    P = 300
    ds = [_edge(m, n, s) for s in range(24)]
    pick = [0] + [1 + (i % 23) for i in range(P - 2)] + [0]
    a = np.stack([ds[k].mat_a for k in pick])
    b, c = np.stack([ds[k].vec_b for k in pick]), np.stack([ds[k].vec_c for k in pick])
    p = _param(T, max_iter=260, eps_acc=1e-3)

    def run(aa, bb, cc, idx):
        sb = T.WideBatchSolver(n, m, aa, bb, cc, [_lib.CONE_RPOS], [m], p)
        sb.run(100, poll_every=50)
        mid = [sb.iterate(i) for i in idx]
        assert all(sb.status(i).iters == 100 for i in idx)
        res = sb.run(-1, poll_every=100)
        st = _blocks(sb)
        out = [(mid[k], st[i], sb.solution(i)) for k, i in enumerate(idx)]
        sb.destroy()
        return out, [r.state for r in res]

    alone, _ = run(a[:1], b[:1], c[:1], [0])
    first, states = run(a, b, c, [0, P - 1])
    second, _ = run(a, b, c, [0, P - 1])
    assert all(s != _lib.ST_RUNNING for s in states)
    ref = alone[0]
    for got in first + second:
        assert repr(got[1]) == repr(ref[1]), (got[1], ref[1])
        for u, v in zip(got[0] + got[2], ref[0] + ref[2]):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


def test_alignment_of_a_changes_nothing(T):
    from totsu_amd import _lib
    m, n = SMALL_BEYOND
    ds = [_edge(m, n, s) for s in range(3)]
    a = np.stack([d.mat_a for d in ds])
    b, c = np.stack([d.vec_b for d in ds]), np.stack([d.vec_c for d in ds])
    p = _param(T)
    base = T.DeviceBuffer.from_host(np.concatenate([np.zeros(1, F), a.ravel()]))

    def run(mats):
        sb = T.WideBatchSolver(n, m, mats, b, c, [_lib.CONE_RPOS], [m], p)
        lb = sb.info()["load_bytes"]
        sb.run(30, poll_every=7)
        out = _state(T, sb)
        sb.destroy()
        return lb, out

    l16, want = run(a)
    l4, got = run(_View(T, base, 1, a.size))
    base.free()
    assert (l16, l4) == (16, 4)
    _same_state(got, want, "unaligned A")


@pytest.mark.parametrize("name", ["lp2020x40", "mixed64"])
def test_launch_cuts_change_nothing(T, name):
    """100 iterations as launches of 1, of 7 and of 64: the same bits (all but x_x u x_y v is updated where it lies)"""
    ds, _, _ = _wide_case(T, name)
    p = _param(T)

    def run(poll):
        sb = T.WideBatchSolver.from_dense(ds, p)
        sb.run(100, poll_every=poll)
        assert all(s.iters == 100 for s in sb.statuses())
        out, launches = _state(T, sb), sb.info()["launches"]
        sb.destroy()
        return out, launches

    (one, l1), (seven, l7), (big, l64) = run(1), run(7), run(64)
    assert (l1, l7, l64) == (100, 15, 2)
    _same_state(one, big, name + " poll 1")
    _same_state(seven, big, name + " poll 7")


# ---- 4. stop conditions ----------------------------------------------------------------------------------------------------------

def test_independent_termination(T):
    from totsu_amd import _lib
    P = 18
    ds = [_term_problem(i) for i in range(P)]
    ros = [O.solve_matop_cones(O.param(max_iter=100000, eps_acc=1e-5, eps_inf=1e-5), d.vec_c, d.mat_a, d.vec_b, d.seg_type, d.seg_len,
                               trace_cap=400) for d in ds]
    want = [O.INFEASIBLE, O.OK, O.UNBOUNDED]
    for i, ro in enumerate(ros):
        assert ro.status == want[i % 3] and ro.iters < 399, (i, ro.status_name, ro.iters)
    p = _param(T, max_iter=100000, eps_acc=1e-5, eps_inf=1e-5)
    sb = T.WideBatchSolver.from_dense(ds, p)
    mid = T.MidBatchSolver.from_dense(ds, p)
    early, live = {}, [P]
    while True:
        res = sb.run_until_any(8, poll_every=8)
        mid.run_until_any(8, poll_every=8)
        live.append(sb.info()["live"])
        _same_state(_state(T, sb), _state(T, mid), "a problem that stops inside a launch leaves the mid batch's state")
        for i, r in enumerate(res):
            if r.state != _lib.ST_RUNNING and i not in early:
                early[i] = (r.state, r.iters, r.kind) + sb.iterate(i)
        if all(r.state != _lib.ST_RUNNING for r in res):
            break
        assert len(live) < 200
    assert live[-1] == 0 and len(set(live)) >= 3 and live == sorted(live, reverse=True)
    for i, ro in enumerate(ros):
        assert res[i].state == ro.status and res[i].kind == ro.trace[-1][1], (i, res[i].state, ro.status_name)
        st, it, kind, x, y = early[i]
        x2, y2 = sb.iterate(i)
        assert (st, it, kind) == (res[i].state, res[i].iters, res[i].kind) and np.array_equal(x, x2) and np.array_equal(y, y2)
    assert len(set(r.iters for r in res)) >= 3
    sb.destroy()
    mid.destroy()


PAD_M = 2600                       # rows of every padded family: 13 m alone is 33 800 floats


def _padded(fam):
    """the family with inert rows appended -- a zero cone of zero rows, b = 0 -- up to PAD_M rows: the same problem, beyond the mid
    batch's rule (and, for F5, the SDP batch's)"""
    extra = PAD_M - fam.m
    assert extra > 0 and old_rule(fam.n, PAD_M, 33 if fam.psd else 0) > LDS
    A = np.vstack([fam.A, np.zeros((extra, fam.n), F)])
    return Z.Family(fam.name + "/padded", fam.n, A, np.concatenate([fam.vec_b, np.zeros(extra, F)]), fam.vec_c,
                    fam.seg_type + [Z.CONE_ZERO], fam.seg_len + [extra], fam.verdict, fam.flips_back)


_PADDED = {}


def _tau_zero_batch(name):
    if name not in _PADDED:
        fams = Z.family(name)
        fams = [_padded(f) for f in (fams if name == "F6" else [fams])]
        _PADDED[name] = (fams, [Z.oracle_plan(f) for f in fams])
    return _PADDED[name]


TAU_ZERO = ["F1", "F2", "F3", "F4", "F5", "F6"]


@pytest.mark.parametrize("name", TAU_ZERO)
def test_iterates_and_criteria_through_tau_zero(T, name):
    fams, pls = _tau_zero_batch(name)
    for fam, pl in zip(fams, pls):
        before, ones, after = Z.counts(pl)
        if fam.verdict != Z.OK:
            assert before >= 1 and ones >= 3 and (after >= 1 or not fam.flips_back), (fam.name, before, ones, after)
    sb = T.WideBatchSolver.from_dense([_dense_of(f) for f in fams], _param(T, eps_inf=1e-30))
    done = 0
    for it in sorted(set(i for pl in pls for i in pl.chosen)):
        sb.run(it + 1 - done, poll_every=64)
        done = it + 1
        for q, (fam, pl) in enumerate(zip(fams, pls)):
            if it in pl.chosen:
                x, y = sb.iterate(q)
                _compare_snap("widebatch/%s" % fam.name, fam, pl, it, x, y, sb.status(q))
    assert all(sb.status(q).state == -1 for q in range(len(fams)))
    if name == "F6":
        assert [sb.status(q).kind for q in range(3)] == [0, 1, 1] == [pl.kinds[-1] for pl in pls]
    sb.destroy()


@pytest.mark.parametrize("name", TAU_ZERO)
def test_verdicts(T, name):
    fams, pls = _tau_zero_batch(name)
    for fam, pl in zip(fams, pls):
        assert pl.status == fam.verdict and pl.iters <= Z.MAX_VERDICT_ITER
    sb = T.WideBatchSolver.from_dense([_dense_of(f) for f in fams], _param(T, max_iter=100_000, eps_acc=Z.EPS, eps_inf=Z.EPS))
    res = sb.run(-1, poll_every=25)
    n, m = fams[0].n, fams[0].m
    for q, (fam, pl, r) in enumerate(zip(fams, pls, res)):
        margin = max(3, pl.iters // 50)
        print("tau_zero verdict widebatch/%-20s state %d at %d (oracle %d at %d, margin %d) kind %d cri %s"
              % (fam.name, r.state, r.iters, pl.status, pl.iters, margin, r.kind, tuple("%.3e" % c for c in r.cri)))
        assert r.state == pl.status, (fam.name, r.state, pl.status)
        assert abs(r.iters - pl.iters) <= margin, (fam.name, r.iters, pl.iters)
        (x, y), sol = sb.iterate(q), sb.solution(q)
        if pl.status == Z.OK:
            assert r.kind == 0 and r.tau > 0 and np.allclose(sol[0], pl.x, atol=2e-3 * max(1.0, np.abs(pl.x).max()))
        else:
            assert r.kind == 1 and r.tau == 0.0 and x[n + 2 * m] == 0.0, (fam.name, r.kind, r.tau)
            assert r.cri[0 if pl.status == Z.UNBOUNDED else 1] <= Z.EPS, (fam.name, r.cri)
            assert np.array_equal(sol[0], x[:n]) and np.array_equal(sol[1], x[n:n + m]), fam.name
    sb.destroy()


# ---- 5. the round calls ----------------------------------------------------------------------------------------------------------

def _round_problems(T):
    m, n = SMALL_BEYOND
    return [_edge(m, n, 40 + s) for s in range(6)]


def _after(T, sb, steps=9):
    sb.run(steps, poll_every=4)
    return _state(T, sb)


@pytest.mark.parametrize("threads", [256, 1024])
def test_round_calls_host_and_device_twins(T, threads):
    """on 2640 x 2, beyond the mid batch's rule: replace is a fresh init of the slot; a run handed its own iterate continues bit for
    bit; set_bc / set_a without keep are replace; every _dev call leaves what its host twin leaves; solutions is solution(i)"""
    from totsu_amd import _lib
    ds = _round_problems(T)
    old, new = ds[:3], ds[3:]
    m, n = SMALL_BEYOND
    p = _param(T)
    mk = lambda probs: T.WideBatchSolver.from_dense(probs, p, force_threads=threads)

    # replace: slot 1 takes new[0] and is what a fresh batch holds; the other slots run on
    fresh = mk([new[0]])
    want_new = _after(T, fresh)
    fresh.destroy()
    sb = mk(old)
    sb.run(5, poll_every=64)
    sb.replace(1, new[0].mat_a, new[0].vec_b, new[0].vec_c)
    assert sb.status(1).state == _lib.ST_RUNNING and sb.status(1).iters == 0
    got = _after(T, sb)
    assert np.array_equal(got[0][1].view(np.uint32), want_new[0][0].view(np.uint32)) and repr(got[1][1]) == repr(want_new[1][0])
    untouched = mk(old)
    want_old = _after(T, untouched, 5 + 9)
    untouched.destroy()
    for i in (0, 2):
        assert np.array_equal(got[0][i].view(np.uint32), want_old[0][i].view(np.uint32)) and repr(got[1][i]) == repr(want_old[1][i])
    sols = sb.solutions()
    for i in range(3):
        x, y = sb.solution(i)
        assert np.array_equal(sols[i][0], x) and np.array_equal(sols[i][1], y)
    part = sb.solutions(first=1, count=2)
    assert np.array_equal(part[0][0], sols[1][0]) and np.array_equal(part[1][1], sols[2][1])
    sb.destroy()

    # set_iterates: plain arithmetic carries no compensation terms, so a run that is handed its own iterate continues bit for bit
    pp = _param(T, state_arith="plain")
    ref = T.WideBatchSolver.from_dense(old, pp, force_threads=threads)
    ref.run(6, poll_every=6)
    its = [ref.iterate(i) for i in range(3)]
    ref.run(9, poll_every=4)
    want = [ref.iterate(i) for i in range(3)]
    ref.destroy()
    outs = []
    for dev in (False, True):
        sb = T.WideBatchSolver.from_dense(old, pp, force_threads=threads)
        if dev:
            dx = T.DeviceBuffer.from_host(np.concatenate([x for x, _ in its]))
            dy = T.DeviceBuffer.from_host(np.concatenate([y for _, y in its]))
            sb.set_iterates_dev(dx, dy)
        else:
            sb.set_iterates([x for x, _ in its], [y for _, y in its])
        assert all(s.iters == 0 and s.state == _lib.ST_RUNNING for s in sb.statuses())
        outs.append(_after(T, sb))
        for i in range(3):
            x, y = sb.iterate(i)
            assert np.array_equal(x, want[i][0]) and np.array_equal(y, want[i][1])
        sb.destroy()
        if dev:
            dx.free()
            dy.free()
    _same_state(outs[1], outs[0], "set_iterates_dev against set_iterates")

    # set_bc and set_a, keep or not: the _dev twin leaves the host call's bits; without keep they are replace
    nb, nc = [d.vec_b for d in new], [d.vec_c for d in new]
    na = [d.mat_a for d in new]
    for keep in (False, True):
        outs = []
        for dev in (False, True):
            sb = mk(old)
            sb.run(5, poll_every=5)
            if dev:
                db, dc = T.DeviceBuffer.from_host(np.concatenate(nb)), T.DeviceBuffer.from_host(np.concatenate(nc))
                sb.set_bc_dev(db, dc, keep_iterate=keep)
            else:
                sb.set_bc(nb, nc, keep_iterate=keep)
            mid_state = _state(T, sb)
            if dev:
                da = T.DeviceBuffer.from_host(np.concatenate(na))
                sb.set_a_dev(da, keep_iterate=keep)
            else:
                sb.set_a(na, keep_iterate=keep)
            assert all(s.iters == 0 and s.state == _lib.ST_RUNNING for s in sb.statuses())
            outs.append((mid_state, _state(T, sb), _after(T, sb)))
            sb.destroy()
            if dev:
                for d in (db, dc, da):
                    d.free()
        for g, w in zip(outs[1], outs[0]):
            _same_state(g, w, "the _dev round against the host round, keep = %s" % keep)
        if not keep:                                   # new A, new b, new c and a fresh init: the batch of the new problems
            sb = mk(new)
            _same_state(outs[0][1], _state(T, sb), "set_bc + set_a against a fresh batch")
            _same_state(outs[0][2], _after(T, sb), "set_bc + set_a against a fresh batch, 9 iterations on")
            sb.destroy()

    # solutions_dev: solutions() and the state words, left on the device
    sb = mk(old)
    sb.run(7, poll_every=7)
    x, y, st = sb.solutions_dev()
    sols = sb.solutions()
    assert np.array_equal(x.to_host(), np.concatenate([s[0] for s in sols])) and np.array_equal(y.to_host(), np.concatenate([s[1] for s in sols]))
    assert list(st.to_host().view(np.int32)) == [s.state for s in sb.statuses()]
    for d in (x, y, st):
        d.free()
    sb.destroy()


# ---- 6. refusals, info -----------------------------------------------------------------------------------------------------------

def test_refusals_leave_nothing_allocated(T):
    from totsu_amd import _lib
    from totsu_amd._lib import lib
    S = T.WideBatchSolver
    z = lambda *s: np.zeros(s, F)
    ds, _ = _family(T, "lp80")
    keep = S.from_dense(ds)
    info = keep.info()
    before = info["device_bytes_all"]
    assert before == info["device_bytes"] > info["arena_bytes"] == len(ds) * info["arena_bytes_per_problem"] > 0
    assert info["lds_bytes"] == info["lds_bytes_per_problem"] == rule(80, 160) and info["psd_lds_bytes"] == 0
    t33 = tri(33)
    bad = [lambda: S(2, 4097, z(1, 2 * 4097), z(1, 4097), z(1, 2), [1], [4097]),
           lambda: S(4097, 2, z(1, 2 * 4097), z(1, 2), z(1, 4097), [1], [2]),
           lambda: S(2987, 4096, z(1, 2987 * 4096), z(1, 4096), z(1, 2987), [_lib.CONE_PSD, 1], [t33, 4096 - t33]),
           lambda: S(3, 7, z(1, 21), z(1, 7), z(1, 3), [_lib.CONE_PSD], [7]),
           lambda: S(3, tri(65), z(1, 3 * tri(65)), z(1, tri(65)), z(1, 3), [_lib.CONE_PSD], [tri(65)]),
           lambda: S(3, 6, z(2, 18), z(2, 6), z(2, 3), [1], [5]),
           lambda: S(3, 6, z(0, 18), z(0, 6), z(0, 3), [1], [6]),
           lambda: S(3, 6, z(2, 17), z(2, 6), z(2, 3), [1], [6])]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    da, db, dc = (T.DeviceBuffer.from_host(z(64)) for _ in range(3))
    par = _lib.Param(-1, 1e-6, 1e-6, 1e-12, 0, 0, 0)
    msgs = []

    def create(n, m, P, st, sl):
        st, sl = np.asarray(st, np.int32), np.asarray(sl, np.int64)
        h = C.c_void_p()
        with pytest.raises(_lib.ThipError) as e:
            lib.thip_widebatch_create(n, m, P, da.ptr, db.ptr, dc.ptr, None, st.size, st.ctypes.data_as(C.POINTER(C.c_int32)),
                                      sl.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(par), C.byref(h))
        assert e.value.code == _lib.E_INVALID and not h.value
        msgs.append((_lib.load().thip_last_error() or b"").decode())
        assert keep.info()["device_bytes_all"] == before

    create(2, 4097, 1, [1], [4097])
    create(4097, 2, 1, [1], [2])
    create(2987, 4096, 1, [_lib.CONE_PSD, 1], [t33, 4096 - t33])
    create(3, 7, 1, [_lib.CONE_PSD], [7])
    create(3, tri(65), 1, [_lib.CONE_PSD], [tri(65)])
    assert all(msgs) and len(set(msgs)) == 5, msgs
    create(3, 6, 2, [1], [5])
    create(3, 6, 0, [1], [6])
    create(3, 6, 1048577, [1], [6])
    for d in (da, db, dc):
        d.free()
    soc, _ = _family(T, "socp")
    sb2 = S.from_dense(soc)
    assert sb2.info()["device_bytes_all"] == before + sb2.info()["device_bytes"]
    sb2.destroy()
    assert keep.info()["device_bytes_all"] == before
    keep.destroy()


def test_info_reports_the_rule(T):
    """an order-64 cone: the operands behind the class bytes are part of what info() and fits report"""
    from totsu_amd import widebatch as WB
    ds, _, max_k = _wide_case(T, "mixed64")
    n, m = ds[0].n, ds[0].m
    sb = T.WideBatchSolver.from_dense(ds)
    info = sb.info()
    sb.destroy()
    assert (info["max_psd_order"], info["n_psd"], info["psd_lds_bytes"]) == (64, 2, 49920)
    assert info["lds_bytes"] == info["lds_bytes_per_problem"] == rule(n, m, 64) == WB.fits(n, m, ds[0].seg_type, ds[0].seg_len)[0]
    assert info["arena_bytes_per_problem"] == 4 * (6 * n + 11 * m)
