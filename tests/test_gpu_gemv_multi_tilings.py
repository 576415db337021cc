"""GPU: every tiling a batch can run the multi-vector dual GEMV under (dual_gemv_multi_k, thip_gemv_multi.hip: the instances NV = 2, 4,
8, one or two row groups per lane, 16 .. 256 columns per chunk), pinned and run alone through thip_test_dual_gemv_multi at the smallest
shapes where it can go wrong, and the dispatch around it: the candidates pinned on a batch, the autotune at its threshold, and the
mapping from the size of a live group to the stored plan.

Each kernel case first asserts from the plan record that the tiling it was written for RAN.  Two references, both independent of the
kernel.  Exact: integers (A in -4 .. 4, vectors in -8 .. 8; every partial sum an integer below 2^24), so the result must EQUAL the
int64 product under every plan -- a dropped, doubled or misplaced row or column shows.  Rounding: standard-normal A, vectors scaled
by 10^U(-3, 3) per slot, against the f64 product inside a bound that follows from the order of summation alone (the second stage sums
in f64): per element (K + 3) 2^-24 (|A||x|), K = the columns per chunk for A x (a lane's sequential FMAs over its chunk) and 8 nj + 8
for A^T y (a lane's FMAs, the six butterfly levels, the two adds across the waves).  The hook fills every slot's scratch with NaNs
beforehand and keeps a guard tail behind it, so a sum that is consumed but was never written, and a store past the scratch, show too;
the outputs are longer than the products, so a store past a result shows as well."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from gemv_multi_plans import (BLK, CANDIDATES, FIELDS, FORMS, ITERS, PAIRS, PIN_SHAPE, TOLS, TUNE_SHAPE, VW, blocks_for, lp_data, plan,
                              restated_plan)

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
SLACK = 16                          # floats of every output behind the product: they must stay as given
U = 2.0 ** -24


@pytest.fixture(scope="module")
def T():
    import totsu_amd
    from totsu_amd import _lib
    _lib.init()
    return totsu_amd


def _up(v, a):
    return (v + a - 1) // a * a


# ---- the kernel alone -----------------------------------------------------------------------------------------------------------

_INPUTS = {}


def _inputs(ref, m, n):
    """host data of one shape, made once: A (m x n), eight vector pairs, and per slot the f64 products with their magnitudes
    (A x, A^T y, |A||x|, |A|^T|y|); a test that runs fewer columns takes the leading ones (column-major: a prefix of the array)"""
    key = (ref, m, n)
    if key not in _INPUTS:
        rng = np.random.default_rng(7919 * m + 31 * n + (ref == "exact"))
        if ref == "exact":
            a = rng.integers(-4, 5, (m, n)).astype(np.float32)
            xn = [rng.integers(-8, 9, n).astype(np.float32) for _ in range(8)]
            xt = [rng.integers(-8, 9, m).astype(np.float32) for _ in range(8)]
        else:
            a = rng.standard_normal((m, n)).astype(np.float32)
            xn = [(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32) for _ in range(8)]
            xt = [(rng.standard_normal(m) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32) for _ in range(8)]
        _INPUTS[key] = (a, xn, xt)
    return _INPUTS[key]


class Case:
    """one matrix and eight vector pairs on the device, outputs with SLACK floats behind them"""

    def __init__(self, T, ref, m, nmax):
        self.T, self.ref, self.m, self.nmax = T, ref, m, nmax
        a, xn, xt = _inputs(ref, m, nmax)
        self.a64, self.abs64 = a.astype(np.float64), np.abs(a.astype(np.float64))
        self.xn, self.xt = xn, xt
        D = T.DeviceBuffer
        # (a tile of NaNs behind the matrix, as the hook keeps behind its padded copy: a load that strays past the last column stays
        # inside the allocation and shows in the result)
        self.da = D.from_host(np.concatenate([np.asfortranarray(a).ravel(order="F"), np.full(2 * BLK * VW, np.nan, np.float32)]))
        self.dxn, self.dxt = [D.from_host(v) for v in xn], [D.from_host(v) for v in xt]
        self.on, self.ot = [D(m + SLACK) for _ in range(8)], [D(nmax + SLACK) for _ in range(8)]
        self.sn, self.st = np.full(m + SLACK, SENTINEL, np.float32), np.full(nmax + SLACK, SENTINEL, np.float32)
        self.extra = []

    def device(self, v):
        d = self.T.DeviceBuffer.from_host(v)
        self.extra.append(d)
        return d

    def want(self, i, n):
        x, y = self.xn[i][:n].astype(np.float64), self.xt[i].astype(np.float64)
        a, aa = self.a64[:, :n], self.abs64[:, :n]
        return a @ x, a.T @ y, aa @ np.abs(x), aa.T @ np.abs(y)

    def run(self, n, nv, nj, tb, stopped=None, dxn=None, dxt=None, mat=None):
        """one launch over the leading n columns into sentinel-filled outputs: (plan record as a dict, out_n[nv], out_t[nv])"""
        from totsu_amd import _lib
        lib = _lib.lib
        for i in range(nv):
            lib.thip_h2d(self.on[i].ptr, self.sn.ctypes.data, self.sn.size)
            lib.thip_h2d(self.ot[i].ptr, self.st.ctypes.data, self.st.size)
        dxn, dxt = dxn or self.dxn, dxt or self.dxt
        arr = lambda bufs: (C.c_void_p * max(len(bufs), 1))(*[b if b is None or isinstance(b, int) else b.ptr for b in bufs])
        flags = None if stopped is None else (C.c_int32 * max(nv, 1))(*[1 if s else 0 for s in stopped[:nv]])
        t = _lib.GemvMultiTest(self.m, n, self.da.ptr if mat is None else mat, nv, nj, tb, 0, arr(dxn[:nv]), arr(dxt[:nv]),
                               arr(self.on[:nv]), arr(self.ot[:nv]), flags)
        rec = _lib.GemvPlanRec()
        lib.thip_test_dual_gemv_multi(C.byref(t), C.byref(rec))
        return {k: getattr(rec, k) for k in FIELDS}, [b.to_host() for b in self.on[:nv]], [b.to_host() for b in self.ot[:nv]]

    def free(self):
        for b in [self.da] + self.dxn + self.dxt + self.on + self.ot + self.extra:
            b.free()


def _check(case, n, inst, nj, tb, worst, nv=None, want_cpc=None):
    """all slots live under the hint (nj, tb): the plan that ran is the planner's, and every slot's two products are right"""
    m = case.m
    nv = inst if nv is None else nv
    rec, gn, gt = case.run(n, nv, nj, tb)
    where = (case.ref, m, n, nv, nj, tb, rec)
    assert rec == plan(m, n, inst, nj, tb)[0] == restated_plan(m, n, inst, nj, tb), where
    assert rec["nj"] == (nj if inst < 8 else 1) and rec["ku"] == 8 // rec["nj"], where
    if want_cpc is not None:
        assert rec["cols_per_chunk"] == want_cpc, where
    kn, kt = rec["cols_per_chunk"] + 3, 8 * rec["nj"] + 8 + 3
    for i in range(nv):
        rn, rt, bn, bt = case.want(i, n)
        assert (gn[i][m:] == SENTINEL).all() and (gt[i][n:] == SENTINEL).all(), (where, i)      # nothing behind a product is written
        for out, r, b, k, side in ((gn[i][:m], rn, bn, kn, "N"), (gt[i][:n], rt, bt, kt, "T")):
            if case.ref == "exact":
                assert np.array_equal(out.astype(np.float64), r), (where, i, side, np.flatnonzero(out != r)[:8])
            else:
                err = np.abs(out - r)
                assert np.isfinite(out).all(), (where, i, side)
                ratio, old = float((err / (k * U * b)).max()), float((err / (1e-5 * b)).max())
                worst[side] = tuple(max(a, b) for a, b in zip(worst.get(side, (0.0, 0.0)), (ratio, old)))
                assert ratio <= 1.0, (where, i, side, ratio)
    return rec


def _report(label, worst):
    print("%s: largest error / derived bound (and / the 1e-5 |A||x| bound)  %s"
          % (label, "  ".join("%s %.3f (%.4f)" % (k, r[0], r[1]) for k, r in sorted(worst.items()))))


def _row_cases(nj):
    t = BLK * VW * nj
    return [1, 2, 3, 4, 5, 7, t - 4, t - 1, t, t + 1, t + 4] + list(range(t + 1020, t + 1025)) + [2 * t + 1, 2 * t + 16]


@pytest.mark.parametrize("inst,nj", FORMS)
def test_rows_at_16_columns_per_chunk(T, inst, nj):
    """n = 40 (three chunks of 16, the last of 8), every m % 4 with the padded copy (m % 16 != 0) and without it, one partial tile
    only, exactly full tiles, one row / one vector into the next tile, under nj = 2 a second row group that is absent (T + 1020 ..
    T + 1024 rows: the fallback offset taken by every lane of group 1), partial and full; a 16-row last tile with no padded copy"""
    worst, n = {}, 40
    for m in _row_cases(nj):
        for ref in ("exact", "rounding"):
            case = Case(T, ref, m, n)
            rec = _check(case, n, inst, nj, 0, worst, want_cpc=16)
            assert (rec["tiles"], rec["chunks"], rec["m_load"]) == (-(-m // (BLK * VW * nj)), 3, _up(m, 4))
            case.free()
    _report("rows NV=%d nj=%d" % (inst, nj), worst)


CPCS = [16, 24, 56, 128, 256]


def _column_cases(m, inst, nj, cpc):
    """{n: target_blocks} of the column counts that exercise a chunk width: the issue's list -- n = 1, KU - 1, KU, KU + 1 (one short
    chunk), cpc - 1, cpc, cpc + 1, cpc + KU - 1, 3 cpc + KU + 1 -- as far as ANY grid target makes the planner choose this width for
    them (it rounds ceil(n / chunks) up to 8, so few columns never meet a wide chunk, and a last chunk of w columns behind full ones
    of width cpc needs at least (cpc - w) / 8 chunks), and for the last-chunk widths 1, KU - 1, KU + 1 the fewest chunks that do"""
    ku = 8 // nj
    ns = [1, ku - 1, ku, ku + 1, cpc - 1, cpc, cpc + 1, cpc + ku - 1, 3 * cpc + ku + 1]
    for w in (1, ku - 1, ku + 1):
        ns.append(next(k * cpc + w for k in range(1, 64) if blocks_for(m, k * cpc + w, inst, nj, cpc)))
    out = {}
    for n in sorted(set(ns)):
        tb = blocks_for(m, n, inst, nj, cpc)
        if tb:
            out[n] = tb
    return out


@pytest.mark.parametrize("m", [8, 1028])
@pytest.mark.parametrize("inst,nj", FORMS)
def test_columns_at_every_chunk_width(T, inst, nj, m):
    """the unrolled steps of KU columns and the one-column tail inside and behind them, a last chunk of one column behind long ones,
    a chunk that fills the LDS rows to their last float (256 columns), on one partial row tile and on a full one plus four rows"""
    ku = 8 // nj
    cases = {cpc: _column_cases(m, inst, nj, cpc) for cpc in CPCS}
    # what the planner lets a launch come to: the short single chunks at the least width only; at every width a single chunk one
    # column short and full, and several chunks with a last one of 1, KU - 1 and KU + 1 columns
    assert {1, ku - 1, ku, ku + 1} <= set(cases[16])
    for cpc in CPCS:
        last = {(n - 1) % cpc + 1 for n in cases[cpc] if n > cpc}
        assert {cpc - 1, cpc} <= set(cases[cpc]) and {1, ku - 1, ku + 1} <= last, (cpc, cases[cpc])
    assert {257, 256 + ku - 1, 3 * 256 + ku + 1} <= set(cases[256])
    nmax = max(max(c) for c in cases.values())
    worst = {}
    for ref in ("exact", "rounding"):
        case = Case(T, ref, m, nmax)
        for cpc in CPCS:
            for n, tb in cases[cpc].items():
                rec = _check(case, n, inst, nj, tb, worst, want_cpc=cpc)
                assert rec["chunks"] == -(-n // cpc)
        case.free()
    _report("columns NV=%d nj=%d m=%d" % (inst, nj, m), worst)


@pytest.mark.parametrize("inst,cand", PAIRS)
def test_every_candidate_as_given(T, inst, cand):
    """the 17 (instance, candidate) pairs the autotune can pick, with the grid target as the library lists it: at 4 x 300 000 and
    6 x 300 000 (the padded copy), where the seven candidates are seven different plans, and at 2052 x 600 (three tiles under
    nj = 1, two under nj = 2, the last one partial)"""
    nj, tb = CANDIDATES[cand]
    want = {(1, 8192): 40, (1, 4096): 80, (1, 2048): 152, (2, 8192): 40, (2, 4096): 80, (2, 2048): 152, (2, 1024): 256}
    worst = {}
    for m, n in ((4, 300_000), (6, 300_000), (2052, 600)):
        for ref in ("exact", "rounding"):
            case = Case(T, ref, m, n)
            rec = _check(case, n, inst, nj, tb, worst, want_cpc=want[(nj if inst < 8 else 1, tb)] if n == 300_000 else None)
            if m == 2052:
                assert rec["tiles"] == (3 if rec["nj"] == 1 else 2)
            case.free()
    _report("candidate %s on NV=%d" % (CANDIDATES[cand], inst), worst)


def _poison(v, k):
    v = v.copy()
    v[k % v.size::3] = [np.nan, np.inf, -np.inf][k % 3]
    return v


@pytest.mark.parametrize("nv", range(2, 9))
def test_slots(T, nv):
    """each single slot stopped, all but one stopped, all stopped (the kernel returns at entry): a stopped slot's outputs stay as
    given, and the live slots' results are bitwise those of the launch with every slot live -- whether the others are live, stopped,
    or stopped and holding NaN and Inf -- and bitwise reproducible.  nv = 3 and 5 .. 7 leave slots of the NV = 4 / 8 table unused."""
    m, n = 1030, 40                       # the padded copy, a partial second tile (one tile under nj = 2), three chunks
    inst = 2 if nv <= 2 else 4 if nv <= 4 else 8
    case = Case(T, "rounding", m, n)
    bad_n = [case.device(_poison(case.xn[i], i)) for i in range(nv)]
    bad_t = [case.device(_poison(case.xt[i], i + 1)) for i in range(nv)]
    patterns = [[j == i for j in range(nv)] for i in range(nv)] + [[j != i for j in range(nv)] for i in range(nv)] + [[True] * nv]
    worst = {}
    for nj in ((1, 2) if inst < 8 else (1,)):
        _check(case, n, inst, nj, 0, worst, nv=nv)                        # every slot live: right, and the yardstick below
        rec0, base_n, base_t = case.run(n, nv, nj, 0, stopped=[False] * nv)
        for stopped in patterns:
            for poisoned in (False, True):
                dxn = [bad_n[i] if (poisoned and stopped[i]) else case.dxn[i] for i in range(nv)]
                dxt = [bad_t[i] if (poisoned and stopped[i]) else case.dxt[i] for i in range(nv)]
                got = [case.run(n, nv, nj, 0, stopped=stopped, dxn=dxn, dxt=dxt) for _ in range(2)]
                where = (nv, nj, stopped, poisoned)
                assert got[0][0] == rec0, where                           # (the plan is reported also when the kernel returned at entry)
                for i in range(nv):
                    for a, b, base in ((got[0][1][i], got[1][1][i], base_n[i]), (got[0][2][i], got[1][2][i], base_t[i])):
                        assert np.array_equal(a, b), (where, i)
                        if stopped[i]:
                            assert (a == SENTINEL).all(), (where, i)
                        else:
                            assert np.array_equal(a, base), (where, i)
    case.free()


def test_bad_arguments_launch_nothing(T):
    from totsu_amd import _lib
    m, n = 40, 24
    case = Case(T, "exact", m, n)

    def refused(n_=n, nv=2, nj=0, tb=0, m_=None, **kw):
        keep = case.m
        case.m = m if m_ is None else m_
        try:
            with pytest.raises(_lib.ThipError) as e:
                case.run(n_, nv, nj, tb, **kw)
        finally:
            case.m = keep
        assert e.value.code == _lib.E_INVALID, e.value
        for i in range(8):
            assert (case.on[i].to_host() == SENTINEL).all() and (case.ot[i].to_host() == SENTINEL).all()

    case.run(n, 8, 0, 0, stopped=[True] * 8)                             # (leaves all sixteen outputs sentinel-filled)
    refused(nv=1)
    refused(nv=0)
    nine = case.dxn + [case.dxn[0]]
    case.on.append(case.on[0]); case.ot.append(case.ot[0])
    refused(nv=9, dxn=nine, dxt=case.dxt + [case.dxt[0]])
    case.on.pop(); case.ot.pop()
    refused(n_=0)
    refused(m_=0)
    refused(nj=-1)
    refused(tb=-1)
    refused(nv=3, dxn=[case.dxn[0], None, case.dxn[2]])                  # a null vector
    refused(nv=3, dxt=[case.dxt[0], case.dxt[1], None])
    refused(mat=case.da.ptr + 4)                                         # no 16-byte loads from there
    rec, gn, gt = case.run(n, 2, 0, 0)                                   # and the same arguments, valid, do launch
    assert rec["chunks"] == 2 and np.array_equal(gn[0][:m].astype(np.float64), case.want(0, n)[0])
    case.free()


# ---- solver level: the plans a batch stores, and what its launches ran under ----------------------------------------------------

_LP = {}


def _lp(m, n, cols=None):
    """the data, A column-major (its leading `cols` columns: a prefix), and the f64 oracle's run per instance, made when first asked for"""
    cols = n if cols is None else cols
    if (m, n) not in _LP:
        _LP[(m, n)] = lp_data(m, n) + ({},)
    a, bs, cs, ros = _LP[(m, n)]
    flat = np.asfortranarray(a[:, :cols]).ravel(order="F")

    def oracle(i):
        if (cols, i) not in ros:
            ros[(cols, i)] = O.solve_matop_cones(O.param(max_iter=max(ITERS) + 2, eps_acc=1e-30), cs[i][:cols], flat, bs[i], [O.CONE_RPOS],
                                                 [m], snap_iters=ITERS, trace_cap=max(ITERS) + 3, use_ql=True)
        return ros[(cols, i)]
    return flat, bs, [c[:cols] for c in cs], oracle


def _batch(T, m, n, B, cols=None, **kw):
    from totsu_amd import _lib
    flat, bs, cs, oracle = _lp(m, n, cols)
    p = T.SolverParam()
    p.eps_acc = 1e-30
    bt = T.BatchSolver(n if cols is None else cols, m, flat, bs[:B], cs[:B], [_lib.CONE_RPOS], [m], p, **kw)
    return bt, oracle


def _follow_oracle(bt, oracle, B, label):
    """_check_batch_iterates of tests/test_gpu_batch.py on a batch that exists already: the preconditioner, the iterates and the
    criteria of every instance"""
    N = bt.n + 2 * bt.m + 1
    for i in range(B):
        t, s = bt.precond(i)
        ro = oracle(i)
        assert np.allclose(t, ro.precond[:N], rtol=2e-5, atol=0), (i, np.abs(t / ro.precond[:N] - 1).max())
        assert np.allclose(s, ro.precond[N:], rtol=2e-5, atol=0), (i, np.abs(s / ro.precond[N:] - 1).max())
    done = 0
    for q, (it, tol) in enumerate(zip(ITERS, TOLS)):
        bt.run(it + 1 - done, poll_every=64)
        done = it + 1
        worst = 0.0
        for i in range(B):
            ro = oracle(i)
            x, y = bt.iterate(i)
            rx, ry = ro.snaps[q][:N], ro.snaps[q][N:]
            ex, ey = np.abs(x - rx).max() / max(np.abs(rx).max(), 1e-6), np.abs(y - ry).max() / max(np.abs(ry).max(), 1e-6)
            worst = max(worst, ex, ey)
            assert ex <= tol and ey <= tol, (label, i, it, ex, ey)
            st = bt.status(i)
            assert st.iters in (it, it + 1)
            assert np.allclose(st.cri, ro.trace[it][2:], rtol=max(50 * tol, 1e-3), atol=1e-5), (label, i, it, st.cri, ro.trace[it])
        print("%s iterate %d: largest err %.2e (tol %.0e)" % (label, it, worst, tol))


def _stored(bt):
    return {nv: (p["rows_groups_per_lane"], p["target_workgroups"]) for nv, p in bt.info()["plans"].items()}


@pytest.mark.parametrize("inst,cand,B", [(i, k, i) for i, k in PAIRS] + [(4, k, 3) for k in range(7)] + [(8, k, 5) for k in range(3)])
def test_every_candidate_pinned_carries_a_batch(T, inst, cand, B):
    m, n = PIN_SHAPE
    bt, oracle = _batch(T, m, n, B)
    assert _stored(bt) == {2: (0, 0), 4: (0, 0), 8: (0, 0)}              # below the autotune's threshold: untuned until pinned
    assert bt.last_multi_plan(inst)["chunks"] > 0                        # (init's own pass ran the shape heuristic)
    bt.pin_multi_plan(inst, cand)
    assert _stored(bt) == {nv: (CANDIDATES[cand] if nv == inst else (0, 0)) for nv in (2, 4, 8)}
    _follow_oracle(bt, oracle, B, "NV=%d B=%d %s" % (inst, B, CANDIDATES[cand]))
    want = plan(m, n, inst, *CANDIDATES[cand])[0]
    got = bt.last_multi_plan(inst)
    assert {k: got[k] for k in FIELDS} == want and got["chunks2"] == 0, (got, want)
    for other in {2, 4, 8} - {inst}:
        assert not any(bt.last_multi_plan(other).values())               # no launch of another instance
    bt.destroy()


def test_pin_refusals(T):
    from totsu_amd import _lib
    bt, _ = _batch(T, 8, 40, 3)
    for inst, cand in ((8, 3), (8, 6), (4, 7), (4, -2), (2, 99), (3, 0), (1, 0), (16, 0), (0, 0)):
        with pytest.raises(_lib.ThipError) as e:
            bt.pin_multi_plan(inst, cand)
        assert e.value.code == _lib.E_INVALID, (inst, cand)
    with pytest.raises(_lib.ThipError) as e:
        bt.last_multi_plan(3)
    assert e.value.code == _lib.E_INVALID
    assert _stored(bt) == {2: (0, 0), 4: (0, 0), 8: (0, 0)}
    bt.pin_multi_plan(4, 5)
    assert _stored(bt)[4] == CANDIDATES[5]
    bt.pin_multi_plan(4, -1)                                             # back to untuned
    assert _stored(bt) == {2: (0, 0), 4: (0, 0), 8: (0, 0)}
    bt.destroy()


def _is_candidate(p, inst):
    return p in CANDIDATES and (inst < 8 or p[0] == 1)


def test_the_autotune_at_its_threshold(T):
    """4096 x 1024 is m n = 2^22 exactly: the autotune times the candidates of the instances the batch can come to launch -- the
    groups' own under fixed groups, NV = 2 .. max_group under regroup -- keeps its picks over a second init and drops them when it is
    switched off; one column fewer and nothing is timed.  No assertion on which candidate wins, nor on time."""
    from totsu_amd._lib import lib
    m, n = TUNE_SHAPE
    none = {2: (0, 0), 4: (0, 0), 8: (0, 0)}
    # B = 8 in fixed groups: one group on NV = 8
    bt, oracle = _batch(T, m, n, 8)
    got = _stored(bt)
    assert _is_candidate(got[8], 8) and got[2] == got[4] == (0, 0), got
    info = bt.info()["plans"]
    bt.reinit()                                                          # tuned already: the picks (and their times) stay
    assert bt.info()["plans"] == info
    _follow_oracle(bt, oracle, 8, "tuned, fixed groups %s" % (got[8],))
    last = bt.last_multi_plan(8)
    assert {k: last[k] for k in FIELDS} == plan(m, n, 8, *got[8])[0], last
    lib.thip_batch_set_gemv_autotune(bt.h, 0)
    assert _stored(bt) == none
    bt.destroy()
    # regroup: every instance the live set can come to be served by
    bt, oracle = _batch(T, m, n, 8, regroup=True, max_group=8)
    got = _stored(bt)
    assert all(_is_candidate(got[nv], nv) for nv in (2, 4, 8)), got
    _follow_oracle(bt, oracle, 8, "tuned, regroup %s" % (got,))
    last = bt.last_multi_plan(8)
    assert {k: last[k] for k in FIELDS} == plan(m, n, 8, *got[8])[0], last
    bt.destroy()
    bt, oracle = _batch(T, m, n, 8, regroup=True, max_group=4)
    got = _stored(bt)
    assert _is_candidate(got[2], 2) and _is_candidate(got[4], 4) and got[8] == (0, 0), got
    bt.destroy()
    # switched off beforehand: nothing is timed
    bt, _ = _batch(T, m, n, 8, regroup=True, gemv_autotune=False)
    assert _stored(bt) == none
    bt.destroy()
    # one column below the threshold: nothing is timed either
    for kw in ({}, {"regroup": True}):
        bt, _ = _batch(T, m, n, 8, cols=n - 1, **kw)
        assert _stored(bt) == none, kw
        bt.destroy()


def test_group_size_to_plan_slot(T):
    """B = 8 small LPs that converge after different numbers of iterations, regroup: the live set shrinks through the sizes served by
    NV = 8, 4, 2 and the single-vector kernel.  With a different candidate pinned on each instance, the launches of every batch of
    iterations ran the kernel instance of the live count under the plan pinned for IT, the launch counters say the same, and every
    instance ends where its own carried solver ends."""
    from totsu_amd import _lib
    from totsu_amd.batch import kernel_instance, live_groups
    a = np.vstack([np.eye(2), -np.eye(2)]).astype(np.float32)            # x <= b[:2], -x <= b[2:]: boxes, as in tests/test_gpu_batch.py
    rng = np.random.default_rng(11)
    bs = [np.concatenate([rng.uniform(0.5, 3, 2), rng.uniform(0.5, 3, 2)]).astype(np.float32) * 4.0 ** (i % 4 - 1) for i in range(8)]
    cs = [(rng.choice([-1, 1], 2) * rng.uniform(0.5, 2, 2)).astype(np.float32) for i in range(8)]
    p = T.SolverParam()
    p.max_iter, p.eps_acc = 100_000, 1e-5
    flat = np.asfortranarray(a).ravel(order="F")
    bt = T.BatchSolver(2, 4, flat, bs, cs, [_lib.CONE_RPOS], [4], p, regroup=True)
    pins = {8: 1, 4: 4, 2: 3}                                            # (1, 4096) on NV = 8, (2, 4096) on NV = 4, (2, 8192) on NV = 2
    for inst, cand in pins.items():
        bt.pin_multi_plan(inst, cand)
    assert _stored(bt) == {inst: CANDIDATES[cand] for inst, cand in pins.items()}
    live = [True] * 8
    seen, every = set(), 8
    want_launches = {1: 0, 2: 0, 4: 0, 8: 0}
    for _ in range(100_000 // every):
        groups = live_groups(live)
        assert len(groups) <= 1                                          # at most eight live: one launch per pass
        res = bt.run(every, poll_every=every)
        if groups:
            inst = kernel_instance(len(groups[0]))
            seen.add(inst)
            want_launches[inst] += 2 * every
            if inst > 1:
                last = bt.last_multi_plan(inst)
                want = plan(4, 2, inst, *CANDIDATES[pins[inst]])[0]
                assert {k: last[k] for k in FIELDS} == want and last["nj"] == CANDIDATES[pins[inst]][0], (inst, last, want)
        ctr = bt.counters()
        assert ctr["launches"] == want_launches, (ctr, want_launches, live)
        live = [r.state == _lib.ST_RUNNING for r in res]
        assert ctr["live"] == sum(live)
        if not any(live):
            break
    assert not any(live)
    assert seen == {1, 2, 4, 8}, seen                                    # the live set did pass through every kernel instance
    for i in range(8):
        fs = T.FusedSolver(2, 4, flat, bs[i], cs[i], [_lib.CONE_RPOS], [4], p, "carried")
        fr, br = fs.run(), bt.status(i)
        assert (br.state, br.kind) == (fr.state, fr.kind) and br.state == _lib.ST_OK and abs(br.iters - fr.iters) <= 2, (i, br.iters, fr.iters)
        (fx, fy), (bx, by) = fs.solution(), bt.solution(i)
        assert np.allclose(bx, fx, atol=1e-3) and np.allclose(by, fy, atol=1e-3), (i, bx, fx)
        fs.destroy()
    bt.destroy()
