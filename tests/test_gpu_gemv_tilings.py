"""GPU: every instance of the single-vector dual GEMV (dual_gemv_k, thip_gemv.hip) the plan autotune can pick, pinned and run alone
through thip_test_dual_gemv at the smallest shapes where it can go wrong, against f64 numpy of the same operation.

Each case first asserts from the plan record that the instance it was written for RAN (rows per load, row groups per lane, the grid,
the form of the partial last row tile).  Two references: integers (every partial sum an integer below 2^24, so the result must EQUAL
the integer product in any order of summation: a dropped, doubled or misplaced row or column shows) and standard-normal data against
the f64 product of the matrix as stored, componentwise inside 1e-5 |A||x| (the bound tests/test_gpu_batch.py applies to the same
arithmetic).  The hook fills its partial-sum scratch with NaNs beforehand, so a sum that is consumed but was never written shows too.
Solver level: the nine candidates pinned one by one (thip_test_solver_pin_gemv_plan) carry a solve to iterate 9 against the oracle."""
import ctypes as C
import types

import numpy as np
import pytest

import oracle as O
from gemv_plans import BLK, CANDIDATES, MAXCW
from problems import random_socp

pytestmark = pytest.mark.gpu

KIND = {"f32": 0, "bf16": 1, "f16": 2}
VW = {"f32": 4, "bf16": 8, "f16": 8}
KU = {1: 8, 2: 4, 4: 2}
NAN16 = {"bf16": 0x7fc0, "f16": 0x7e00}
SENTINEL = 7.0
NARROW = [1, 7, 9, 17, 100]         # columns: the remainder loops of KU = 8, 4, 2 and several chunks
PRODUCTS = [("N", 1, 0, 0), ("T", 0, 1, 0), ("NT", 1, 1, 0), ("ABS", 1, 1, 1)]


@pytest.fixture(scope="module")
def T():
    import totsu_amd
    from totsu_amd import _lib
    _lib.init()
    return totsu_amd


def _up(v, a):
    return (v + a - 1) // a * a


def _candidate_blocks(nj):
    return next(tb for j, tb in CANDIDATES if j == nj)


def _want_chunks(m, n, cols, tiles, tb):
    """(chunk rows, columns per chunk) of a launch over `cols` columns -- the planner's rule for matrices below 64 MB: the grid
    target (2048 workgroups unless hinted) spread over the row tiles, at least 16 and at most MAXCW columns per chunk, a multiple of 8"""
    assert m * n * 4 < 64e6 and m * n * 4 / 2e5 <= 2048
    per = max(1, (tb or 2048) // tiles)
    cpc = min(MAXCW, _up(max(16, -(-cols // per)), 8))
    return -(-cols // cpc), cpc


class Stored:
    """one matrix as it lies in device memory, twice: `Z` with pitch roundup(m, 16) and zeros below row m, `X` with a pitch > m and
    NaNs below row m; `dec` = the f64 matrix the stored entries decode to"""

    def __init__(self, T, kind, a, unaligned=False):
        from totsu_amd._lib import lib
        m, n = a.shape
        self.kind, self.m, self.n, self.bufs = kind, m, n, []
        self.inv = None
        if unaligned:
            # the VW = 1 fallback: f32, base pointer one float off 16 bytes, a tight odd pitch, NaN in the pad row if there is one
            assert kind == "f32"
            ld = m if m % 2 else m + 1
            h = np.full((n, ld), np.nan, np.float32)
            h[:, :m] = a.T
            buf = T.DeviceBuffer.from_host(np.concatenate([np.zeros(1, np.float32), h.ravel()]))
            self.bufs.append(buf)
            self.X = self.Z = (buf.ptr + 4, ld)
            self.dec = a.astype(np.float64)
            return
        ldz = _up(m, 16)
        ldx = ldz if ldz > m else m + 16
        if kind == "f32":
            hz = np.zeros((n, ldz), np.float32)
            hz[:, :m] = a.T
            hx = np.full((n, ldx), np.nan, np.float32)
            hx[:, :m] = a.T
            bz, bx = T.DeviceBuffer.from_host(hz), T.DeviceBuffer.from_host(hx)
            self.dec = a.astype(np.float64)
        else:
            # the library's own conversion (bit-exactness: tests/test_gpu_bf16.py), read back and decoded
            src = T.DeviceBuffer.from_host(np.ascontiguousarray(a.T))
            bz = T.DeviceBuffer((ldz * n + 1) // 2 + 4, zero=True)
            if kind == "bf16":
                lib.thip_to_bf16(m, n, src.ptr, bz.ptr, ldz)
            else:
                self.inv = T.DeviceBuffer(n)
                self.bufs.append(self.inv)
                lib.thip_to_f16(m, n, src.ptr, bz.ptr, ldz, self.inv.ptr)
            bits = bz.to_host().view(np.uint16)[:ldz * n].reshape((n, ldz))
            assert not bits[:, m:].any()                    # the library's zeros below row m
            src.free()
            if kind == "bf16":
                self.dec = (bits[:, :m].astype(np.uint32) << 16).view(np.float32).astype(np.float64).T
            else:
                inv = self.inv.to_host().astype(np.float64)
                assert np.all(np.log2(inv) % 1 == 0)         # powers of two: the scaling is exact
                self.dec = (bits[:, :m].view(np.float16).astype(np.float64) * inv[:, None]).T
            hx = np.full((n, ldx), NAN16[kind], np.uint16)
            hx[:, :m] = bits[:, :m]
            raw = np.zeros(((ldx * n + 1) // 2 + 4) * 2, np.uint16)
            raw[:ldx * n] = hx.ravel()
            bx = T.DeviceBuffer.from_host(raw.view(np.float32))
        self.bufs += [bz, bx]
        self.Z, self.X = (bz.ptr, ldz), (bx.ptr, ldx)

    def free(self):
        for b in self.bufs:
            b.free()


class Vectors:
    def __init__(self, T, m, n, xn, xt):
        self.xn, self.xt = T.DeviceBuffer.from_host(xn), T.DeviceBuffer.from_host(xt)
        self.on, self.ot = T.DeviceBuffer(m), T.DeviceBuffer(n)
        self.sn, self.st = np.full(m, SENTINEL, np.float32), np.full(n, SENTINEL, np.float32)

    def free(self):
        for b in (self.xn, self.xt, self.on, self.ot):
            b.free()


def _call(st, where, pad_zero, v, do_n, do_t, abs_mode, nj, tb, col_split=0, stopped=0):
    """one thip_test_dual_gemv call into sentinel-filled outputs: (plan record, out_n, out_t)"""
    from totsu_amd import _lib
    lib = _lib.lib
    lib.thip_h2d(v.on.ptr, v.sn.ctypes.data, v.sn.size)
    lib.thip_h2d(v.ot.ptr, v.st.ctypes.data, v.st.size)
    ptr, lda = where
    t = _lib.GemvTest(st.m, st.n, lda, ptr, None if st.inv is None else st.inv.ptr, KIND[st.kind], pad_zero,
                      v.xn.ptr, v.xt.ptr, v.on.ptr, v.ot.ptr, do_n, do_t, abs_mode, nj, tb, stopped, col_split)
    rec = _lib.GemvPlanRec()
    lib.thip_test_dual_gemv(C.byref(t), C.byref(rec))
    return rec, v.on.to_host(), v.ot.to_host()


def _inputs(ref, m, n, seed):
    rng = np.random.default_rng(seed)
    if ref == "exact":
        a = rng.integers(-4, 5, (m, n)).astype(np.float32)
        xn, xt = rng.integers(-8, 9, n).astype(np.float32), rng.integers(-8, 9, m).astype(np.float32)
    else:
        a = rng.standard_normal((m, n)).astype(np.float32)
        xn = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32)
        xt = (rng.standard_normal(m) * 10.0 ** rng.uniform(-3, 3)).astype(np.float32)
    return a, xn, xt


def _references(dec, xn, xt):
    """per product: (A x, A^T y, their componentwise magnitudes |A||x|, |A|^T|y|) in f64; ABS: the row and column sums of |A|"""
    x, y, aa = xn.astype(np.float64), xt.astype(np.float64), np.abs(dec)
    plain = (dec @ x, dec.T @ y, aa @ np.abs(x), aa.T @ np.abs(y))
    ab = (aa.sum(axis=1), aa.sum(axis=0), aa.sum(axis=1), aa.sum(axis=0))
    return {"N": plain, "T": plain, "NT": plain, "ABS": ab}


def _forms(kind, m, unaligned=False):
    """(name, which copy, pad_zero, rows the partial last tile may load whole) of the tile forms this m can take"""
    if unaligned:
        return [("guarded", "X", 0, 0)]
    vw = VW[kind]
    own = m if m % vw == 0 else 0
    forms = [("a", "Z", 1, _up(m, vw))]                   # the library's zero-padded copy: unguarded
    if m % vw:
        forms.append(("b", "Z", 0, 0))                    # the same bytes without the promise: guarded
    forms.append(("c", "X", 0, own))                      # NaNs below row m: guarded, or unguarded up to m exactly
    return forms


def _check_products(T, kind, m, n, hints, refs, worst, want_plan, col_splits=(0,), unaligned=False):
    """all products in all tile forms on one shape, under each (nj, target_blocks) of `hints` and each column split"""
    for ref in refs:
        a, xn, xt = _inputs(ref, m, n, 7919 * m + 31 * n + (ref == "exact"))
        st = Stored(T, kind, a, unaligned)
        v = Vectors(T, m, n, xn, xt)
        want = _references(st.dec, xn, xt)
        for nj, tb in hints:
            for cs in col_splits:
                first = None
                for form, copy, pad_zero, m_load in _forms(kind, m, unaligned):
                    got = {}
                    for name, do_n, do_t, abs_mode in PRODUCTS:
                        rec, gn, gt = _call(st, getattr(st, copy), pad_zero, v, do_n, do_t, abs_mode, nj, tb, cs)
                        where = (kind, m, n, nj, tb, cs, ref, form, name)
                        want_plan(rec, m_load, n, tb, cs, where)
                        rn, rt, bn, bt = want[name]
                        for out, r, b, on, side in ((gn, rn, bn, do_n, "N"), (gt, rt, bt, do_t, "T")):
                            if not on:
                                assert (out == SENTINEL).all(), where           # a product not asked for is not written
                            elif ref == "exact":
                                assert np.array_equal(out.astype(np.float64), r), (where, side, np.flatnonzero(out != r)[:8])
                            else:
                                ratio = float((np.abs(out - r) / (1e-5 * b)).max())
                                key = (name, side)
                                worst[key] = max(worst.get(key, 0.0), ratio)
                                assert ratio <= 1.0, (where, side, ratio)
                        got[name] = (gn, gt)
                    rec, gn, gt = _call(st, getattr(st, copy), pad_zero, v, 1, 1, 0, nj, tb, cs, stopped=1)
                    assert (gn == SENTINEL).all() and (gt == SENTINEL).all(), (kind, m, n, nj, tb, cs, form, "stopped")
                    if first is None:
                        first = got
                        if ref == "rounding":                                 # bitwise reproducible
                            _, gn, gt = _call(st, getattr(st, copy), pad_zero, v, 1, 1, 0, nj, tb, cs)
                            assert np.array_equal(gn, got["NT"][0]) and np.array_equal(gt, got["NT"][1]), (kind, m, n, nj, tb, cs)
                    else:
                        # same plan, same order of every sum: nothing below row m may reach a result, whatever lies there
                        for name in got:
                            assert np.array_equal(got[name][0], first[name][0]) and np.array_equal(got[name][1], first[name][1]), \
                                (kind, m, n, nj, tb, cs, ref, form, name)
        v.free()
        st.free()


def _report(label, worst):
    print("%s: largest error / bound  %s" % (label, "  ".join("%s.%s %.3f" % (k[0], k[1], r) for k, r in sorted(worst.items()))))


# (the last one beyond the six classes of a tile's edges: the partial tile ends inside the LAST row group of a lane, odd -- the only
# class in which the row groups 1 .. nj - 1 of a partial tile are all in use and the last one is cut)
ROW_CLASSES = ["VW", "T-VW", "T", "T+VW", "T+1", "2.5T+1", "2T-cut"]


def _rows(kind, nj, row_class):
    vw = VW[kind]
    t = BLK * vw * nj
    return {"VW": vw, "T-VW": t - vw, "T": t, "T+VW": t + vw, "T+1": t + 1, "2.5T+1": 2 * t + t // 2 + 1,
            "2T-cut": t + (nj - 1) * BLK * vw + 100 * vw + 1}[row_class]


@pytest.mark.parametrize("row_class", ROW_CLASSES)
@pytest.mark.parametrize("nj", [1, 2, 4])
@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_vector_instances(T, kind, nj, row_class):
    """the 3 x 3 instances (element type x row groups per lane) on one partial tile only / the last full lane group missing / exactly
    full / one vector into a second tile / one row into it / an odd m with several tiles / a second tile cut inside its last row
    group, in every tile form that m can take"""
    vw = VW[kind]
    tile = BLK * vw * nj
    m = _rows(kind, nj, row_class)
    tiles = -(-m // tile)
    ran = set()

    def want_plan(rec, m_load, n, tb, cs, where):
        chunks, cpc = _want_chunks(m, n, n, tiles, tb)
        got = (rec.vw, rec.nj, rec.ku, rec.tiles, rec.chunks, rec.cols_per_chunk, rec.m_load)
        assert got == (vw, nj, KU[nj], tiles, chunks, cpc, m_load), (where, got)
        ran.add((where[7], rec.m_load > 0))

    worst = {}
    hints = [(nj, 0), (nj, _candidate_blocks(nj))]
    for n in NARROW:
        _check_products(T, kind, m, n, hints + ([(nj, 1)] if n >= 17 else []), ("exact", "rounding"), worst, want_plan)
    # one chunk at the most columns a chunk may hold, and one column past it
    if row_class in ("VW", "T+1"):
        for n in (MAXCW, MAXCW + 1):
            _check_products(T, kind, m, n, [(nj, 1)], ("exact", "rounding") if row_class == "VW" else ("exact",), worst, want_plan)
    # the forms this m was written for did run
    if m % vw:
        assert ran == {("a", True), ("b", False), ("c", False)}, ran
    else:
        assert ran == {("a", True), ("c", True)}, ran
    _report("%s nj=%d m=%d" % (kind, nj, m), worst)


@pytest.mark.parametrize("m", [255, 256, 257, 4095, 4096, 5121])
def test_unaligned_fallback(T, m):
    """VW = 1 (a base pointer off 16 bytes, an odd pitch): one row group per lane below 4096 rows, four from there on, on both sides
    of a tile; the hint's row groups are not for this path"""
    nj = 4 if m >= 4096 else 1
    tiles = -(-m // (BLK * nj))

    def want_plan(rec, m_load, n, tb, cs, where):
        chunks, cpc = _want_chunks(m, n, n, tiles, tb)
        got = (rec.vw, rec.nj, rec.ku, rec.tiles, rec.chunks, rec.cols_per_chunk, rec.m_load)
        assert got == (1, nj, 4 if nj == 4 else 8, tiles, chunks, cpc, 0), (where, got)

    worst = {}
    for n in NARROW:
        _check_products(T, "f32", m, n, [(0, 0), (2, 4096)] + ([(0, 1)] if n >= 17 else []), ("exact", "rounding"), worst, want_plan,
                        unaligned=True)
    if m in (257, 4096):
        for n in (MAXCW, MAXCW + 1):
            _check_products(T, "f32", m, n, [(0, 1)], ("exact", "rounding"), worst, want_plan, unaligned=True)
    _report("f32 unaligned m=%d" % m, worst)


@pytest.mark.parametrize("nj", [1, 2, 4])
@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_column_ranges(T, kind, nj):
    """the column-range form as the solver's column-split pipeline issues it: two launches over [0, c) and [c, n) filling consecutive
    chunk rows, one full and one partial row tile"""
    vw = VW[kind]
    tile = BLK * vw * nj
    m = tile + 1
    tiles = 2

    def want_plan(rec, m_load, n, tb, cs, where):
        (r1, c1), (r2, c2) = _want_chunks(m, n, cs, tiles, tb), _want_chunks(m, n, n - cs, tiles, tb)
        got = (rec.vw, rec.nj, rec.ku, rec.tiles, rec.chunks, rec.cols_per_chunk, rec.chunks2, rec.cols_per_chunk2, rec.m_load)
        assert got == (vw, nj, KU[nj], tiles, r1, c1, r2, c2, m_load), (where, got)

    worst = {}
    # split after 8 columns, at the solver's split column, and 8 columns before the end (104) or at the last multiple of 8 that
    # leaves at least 8 (100: the hook, like the pipeline, splits at multiples of 8 only)
    for n in (24, 100, 104):
        splits = sorted({8, (n // 2) // 8 * 8, (n - 8) // 8 * 8})
        _check_products(T, kind, m, n, [(nj, 0), (nj, _candidate_blocks(nj)), (nj, 1)], ("exact", "rounding"), worst, want_plan,
                        col_splits=splits)
    _report("%s nj=%d m=%d column ranges" % (kind, nj, m), worst)


def test_split_form_fits_the_scratch_where_a_half_drops_under_64_mb(T):
    """24 621 x 958 is 94 MB and its column halves are 47 MB each: below 64 MB the least chunk width halves, so the two half-launches
    fill 61 chunk rows where one launch fills 30 -- 496 floats more than twice the scratch of one launch held before the scratch was
    sized from the split form too (the pipeline then stopped with THIP_E_WORK).  Integers: the result must be exact."""
    m, n = 24_621, 958
    rng = np.random.default_rng(5)
    a = rng.integers(-4, 5, (n, m), dtype=np.int8)                   # column-major
    xn, xt = rng.integers(-8, 9, n).astype(np.float32), rng.integers(-8, 9, m).astype(np.float32)
    ld = _up(m, 16)
    h = np.zeros((n, ld), np.float32)
    h[:, :m] = a
    st = types.SimpleNamespace(kind="f32", m=m, n=n, inv=None)
    buf = T.DeviceBuffer.from_host(h)
    v = Vectors(T, m, n, xn, xt)
    split = (n // 2) // 8 * 8
    rec, gn, gt = _call(st, (buf.ptr, ld), 1, v, 1, 1, 0, 0, 0, split)
    assert (rec.vw, rec.nj, rec.tiles, rec.chunks, rec.chunks2, rec.cols_per_chunk, rec.cols_per_chunk2) == (4, 1, 25, 30, 31, 16, 16)
    assert rec.m_load == _up(m, 4)
    # every partial sum is an integer below 2^24: f32 BLAS is exact in any order
    assert np.array_equal(gn, h[:, :m].T @ xn) and np.array_equal(gt, h[:, :m] @ xt)
    v.free()
    buf.free()


def test_bad_arguments_launch_nothing(T):
    from totsu_amd import _lib
    m, n = 40, 24
    a, xn, xt = _inputs("exact", m, n, 1)
    st16 = Stored(T, "f16", a)
    st = Stored(T, "f32", a)
    v = Vectors(T, m, n, xn, xt)

    def refused(stored, where, **kw):
        args = dict(pad_zero=0, v=v, do_n=1, do_t=1, abs_mode=0, nj=0, tb=0)
        args.update(kw)
        with pytest.raises(_lib.ThipError) as e:
            _call(stored, where, **args)
        assert e.value.code == _lib.E_INVALID, e.value
        assert (v.on.to_host() == SENTINEL).all() and (v.ot.to_host() == SENTINEL).all()

    refused(st, (st.Z[0], m - 1))                                    # lda < m
    refused(st, st.Z, do_n=0, do_t=0)                                # no product
    refused(st, st.Z, nj=-1)
    for cs in (4, 12, n, n + 8):                                     # not a multiple of 8, or no column left for the second launch
        refused(st, st.Z, col_split=cs)
    inv, st16.inv = st16.inv, None
    refused(st16, st16.Z)                                            # f16 without its scales
    st16.inv = inv
    xn_buf, v.xn = v.xn, type("Null", (), {"ptr": None})()
    refused(st, st.Z)                                                # a null vector the N product needs
    rec, gn, gt = _call(st, st.Z, 0, v, 0, 1, 0, 0, 0)               # ... which the T product alone does not
    assert np.array_equal(gt.astype(np.float64), st.dec.T @ xt.astype(np.float64)) and (gn == SENTINEL).all()
    rec, gn, gt = _call(st, st.Z, 0, v, 1, 1, 1, 0, 0)               # ... nor do the |A| sums
    assert np.array_equal(gn.astype(np.float64), np.abs(st.dec).sum(axis=1))
    v.xn = xn_buf
    v.free()
    st.free()
    st16.free()


# ---- solver level: each candidate pinned carries a solve ------------------------------------------------------------------------

SOCP_N, SOCP_CONES = 37, [5, 1, 0, 17, 99, 3, 500, 1400, 2067]      # m = sum (n_i + 1) = 4101: odd (the padded copy), two row
ITERS, TOLS = [0, 1, 9], [2e-5, 2e-5, 1e-4]                          # tiles at nj = 4 and five at nj = 1
_CACHE = {}


def _mb(T, typ):
    return T.MatBuild(T.F32HIP, typ)


def _dense(T):
    if "dense" not in _CACHE:
        f, Gs, hs, cs, d = random_socp(SOCP_N, SOCP_CONES, seed=3)
        # the row sums of b carry d_i, not |d_i|, as the reference's SOCP operator does: only with every d_i > 0 (this seed) is the
        # oracle's preconditioner of the stacked problem like for like
        assert min(d) > 0
        socp = T.ProbSOCP(_mb(T, T.MatType.General(SOCP_N, 1)).set_array(f.reshape(-1, 1)),
                          [_mb(T, T.MatType.General(G.shape[0], SOCP_N)).set_array(G) for G in Gs],
                          [_mb(T, T.MatType.General(len(h_), 1)).set_array(h_.reshape(-1, 1)) for h_ in hs],
                          [_mb(T, T.MatType.General(SOCP_N, 1)).set_array(c_.reshape(-1, 1)) for c_ in cs], d,
                          _mb(T, T.MatType.General(0, SOCP_N)), _mb(T, T.MatType.General(0, 1)))
        _CACHE["dense"] = socp.dense()
        assert (_CACHE["dense"].m, _CACHE["dense"].n) == (4101, SOCP_N)
    return _CACHE["dense"]


def _oracle(T, storage):
    """the f64 oracle's preconditioner and iterates on the matrix as stored (computed once per stored form)"""
    if storage not in _CACHE:
        import copy
        from test_gpu_bf16 import bf16_round, f16_quantize
        d = copy.copy(_dense(T))
        if storage == "bf16":
            d.mat_a = bf16_round(np.asarray(d.mat_a, np.float32))
        elif storage == "f16":
            A = np.asarray(d.mat_a, np.float32).reshape((d.n, d.m)).T
            d.mat_a = np.asfortranarray(f16_quantize(A)[2]).ravel(order="F")
        _CACHE[storage] = O.solve_matop_cones(O.param(max_iter=max(ITERS) + 2, eps_acc=1e-30), d.vec_c, d.mat_a, d.vec_b, d.seg_type,
                                              d.seg_len, snap_iters=ITERS, trace_cap=max(ITERS) + 3, use_ql=True)
    return _CACHE[storage]


def _pinned(T, schedule, cand, **kw):
    p = T.SolverParam()
    p.eps_acc = 1e-30
    fs = T.FusedSolver.from_dense(_dense(T), p, schedule, **kw)
    assert fs.gemv_plan()["rows_groups_per_lane"] == 0               # below the autotune's threshold: the heuristic until pinned
    fs.pin_gemv_plan(cand)
    plan = fs.gemv_plan()
    assert (plan["rows_groups_per_lane"], plan["target_workgroups"]) == CANDIDATES[cand], (cand, plan)
    return fs


def _follow_oracle(T, fs, ro, label, check_precond=True):
    d = _dense(T)
    N = d.n + 2 * d.m + 1
    if check_precond:
        t, s = fs.precond()
        assert np.allclose(t, ro.precond[:N], rtol=2e-5, atol=0), np.abs(t / ro.precond[:N] - 1).max()
        assert np.allclose(s, ro.precond[N:], rtol=2e-5, atol=0), np.abs(s / ro.precond[N:] - 1).max()
    done = 0
    for q, (it, tol) in enumerate(zip(ITERS, TOLS)):
        fs.run(it + 1 - done, poll_every=64)
        done = it + 1
        x, y = fs.iterate()
        rx, ry = ro.snaps[q][:N], ro.snaps[q][N:]
        ex, ey = np.abs(x - rx).max() / max(np.abs(rx).max(), 1e-6), np.abs(y - ry).max() / max(np.abs(ry).max(), 1e-6)
        print("%s iterate %d: err x %.2e y %.2e (tol %.0e)" % (label, it, ex, ey, tol))
        assert ex <= tol and ey <= tol, (label, it, ex, ey)
        assert fs.status().iters in (it, it + 1)


@pytest.mark.parametrize("cand", range(len(CANDIDATES)))
@pytest.mark.parametrize("schedule", ["fused", "carried"])
def test_every_candidate_carries_a_solve(T, schedule, cand):
    fs = _pinned(T, schedule, cand)
    _follow_oracle(T, fs, _oracle(T, "f32"), "%s %s" % (schedule, CANDIDATES[cand]))
    assert (fs.gemv_plan()["rows_groups_per_lane"], fs.gemv_plan()["target_workgroups"]) == CANDIDATES[cand]
    fs.destroy()


@pytest.mark.parametrize("cand", [0, 3, 8])
def test_candidates_under_the_reference_schedule(T, cand):
    # one product per launch: A^T y alone, then A x alone, each into its half of the scratch
    fs = _pinned(T, "reference", cand)
    _follow_oracle(T, fs, _oracle(T, "f32"), "reference %s" % (CANDIDATES[cand],))
    fs.destroy()


@pytest.mark.parametrize("cand", [1, 3, 7])
def test_candidates_in_the_column_split_pipeline(T, cand):
    # overlap 2 (pipelined) against overlap 3 (its in-order form) with a stand-in all-reduce on one rank: bitwise equal, and
    # the iterates are the oracle's
    out = []
    for overlap in (3, 2):
        fs = _pinned(T, "carried", cand, allreduce=("spin", 0), overlap=overlap)
        info = fs.overlap_info()
        assert info == {"mode": overlap, "launches_per_pass": 2, "split_col": 16}, info
        assert (fs.gemv_plan()["rows_groups_per_lane"], fs.gemv_plan()["target_workgroups"]) == CANDIDATES[cand]
        if overlap == 3:
            _follow_oracle(T, fs, _oracle(T, "f32"), "split %s" % (CANDIDATES[cand],))
        else:
            for steps in np.diff([-1] + ITERS):                      # (the same batches: the pipeline drains where the host looks)
                fs.run(int(steps), poll_every=64)
        out.append(fs.iterate())
        assert (fs.gemv_plan()["rows_groups_per_lane"], fs.gemv_plan()["target_workgroups"]) == CANDIDATES[cand]
        fs.destroy()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("cand", [3, 6])                             # one nj = 2 and one nj = 4 candidate
@pytest.mark.parametrize("storage", ["bf16", "f16"])
def test_candidates_on_16_bit_storage(T, storage, cand):
    fs = _pinned(T, "carried", cand, a_storage=storage)
    assert fs.passes()[1] == SOCP_N * 4101 * 2
    # (the preconditioner is that of the stored matrix as well: its |A| sums stream the 16-bit copy)
    _follow_oracle(T, fs, _oracle(T, storage), "%s %s" % (storage, CANDIDATES[cand]))
    fs.destroy()
