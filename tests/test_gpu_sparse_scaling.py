"""GPU: the tiled sparse products (thip_sptile.hip) on BADLY SCALED matrices -- rows or columns that are small as a whole.  The LDS
accumulators are fixed-point words; with one scale per product an out element whose own (|A||x|)_i lies decades below
amax * xmax lost its low bits (and abs-mode sums of small rows came out 0).  The scale is per out element now;
these tests hold every code path of sp_tile_k to the suite's elementwise bound |out - ref| <= 1e-5 (|A||x|) + 1e-30 against an
f64 numpy product of the same f32-rounded matrix and vector, D1 R D2 with fixed seeds (tests/sptile_numpy.py).  The two-copy CSR
route sums in plain f32: it is the control that shows the bound is fair."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import sptile_numpy as S
from problems import l1reg_lp
from test_gpu_sparse import _iterates_vs_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import totsu_amd
    from totsu_amd import _lib
    _lib.init()
    return totsu_amd


def _sl(L, a):
    return L.Sl.new_mut(np.ascontiguousarray(a, dtype=np.float32))


# every case on every code path of sp_tile_k (the layouts of sptile_numpy.LAYOUTS), case D also on its own half-dense shape;
# for each the N product with scaled rows and the T product with scaled columns
_PRODUCTS = [(case, layout, trans, two)
             for layout in ("single", "staged", "lite", "full", "tall") for case in "ABCDF"
             for trans in (False, True) for two in (False, True)] + \
            [("D", "wide50", trans, two) for trans in (False, True) for two in (False, True)]


def _worst(err, scale):
    nz = scale > 0
    return float((err[nz] / scale[nz]).max()) if nz.any() else 0.0


def _id(case, layout, trans, two):
    return "%s-%s-%s-%s" % (case, layout, "T" if trans else "N", "csr" if two else "tiled")


@pytest.mark.parametrize("case,layout,trans,two_copies", _PRODUCTS, ids=[_id(*p) for p in _PRODUCTS])
def test_products_and_abs_sums_under_diagonal_scaling(T, case, layout, trans, two_copies):
    from totsu_amd.sparse import SparseMatOp
    L = T.F32HIP
    a, v = S.scaled_case(case, layout, trans)
    m, n = a.shape
    rng = np.random.default_rng(7)
    w = rng.standard_normal(n if trans else m).astype(np.float32)      # the other side's vector: plain N(0, 1)
    x, y = (w, v) if trans else (v, w)
    op = SparseMatOp(L, a, two_copies=two_copies)
    if not two_copies and layout == "full":
        assert op.t.info()["dense_tiles"] == 2
    ax, aty = _sl(L, np.zeros(m)), _sl(L, np.zeros(n))
    op.op(1.0, _sl(L, x), 0.0, ax)
    op.trans_op(1.0, _sl(L, y), 0.0, aty)
    ax, aty = ax.get_ref().copy(), aty.get_ref().copy()
    ref_n, sc_n = S.reference(a, x, False)
    ref_t, sc_t = S.reference(a, y, True)
    e_n, e_t = np.abs(ax - ref_n), np.abs(aty - ref_t)
    # adjointness <A x, y> == <x, A^T y>
    lhs = float(ax.astype(np.float64) @ y.astype(np.float64))
    rhs = float(x.astype(np.float64) @ aty.astype(np.float64))
    adj_scale = float(sc_n @ np.abs(y.astype(np.float64)))
    st, ss = _sl(L, np.zeros(n)), _sl(L, np.zeros(m))
    op.absadd_cols(st)
    op.absadd_rows(ss)
    st, ss = st.get_ref().copy(), ss.get_ref().copy()
    op.drop()
    a64 = abs(a.astype(np.float64))
    cols, rows = np.asarray(a64.sum(axis=0)).ravel(), np.asarray(a64.sum(axis=1)).ravel()
    print("scaling %s %-6s %s %s: op %.2e trans_op %.2e adjoint %.2e abs rows %.2e (%d zero) abs cols %.2e (%d zero)"
          % (case, layout, "T" if trans else "N", "csr" if two_copies else "tiled", _worst(e_n, sc_n), _worst(e_t, sc_t),
             abs(lhs - rhs) / max(adj_scale, 1e-300), _worst(np.abs(ss - rows), rows), int(((ss == 0) & (rows > 0)).sum()),
             _worst(np.abs(st - cols), cols), int(((st == 0) & (cols > 0)).sum())))
    assert np.all(e_n <= 1e-5 * sc_n + 1e-30)
    assert np.all(e_t <= 1e-5 * sc_t + 1e-30)
    assert abs(lhs - rhs) <= 1e-5 * adj_scale + 1e-30
    assert np.allclose(ss, rows, rtol=1e-5, atol=0.0) and np.allclose(st, cols, rtol=1e-5, atol=0.0)
    assert np.all(ss[rows > 0] > 0) and np.all(st[cols > 0] > 0)


@pytest.mark.parametrize("layout,trans", [("single", False), ("single", True), ("staged", True), ("full", False)])
def test_error_beyond_the_in_vector_window_is_bounded_as_documented(T, layout, trans):
    # the stated limit: a 1e6 spike in the in-vector over rows / columns of 10^+-6.  An out element that misses the spike may lose
    # bits, but no more than include/totsu_f32hip.h promises beside thip_sptile_mv:
    #     err_i <= 1e-5 (|A||x|)_i + 2^-G amax_i max|x|,   G = 50 - 2 head_bits,  head_bits = ceil(log2(longest row / column)) + 1
    from totsu_amd.sparse import SparseMatOp
    L = T.F32HIP
    a, v = S.scaled_case("spike", layout, trans)
    op = SparseMatOp(L, a)
    out = _sl(L, np.zeros(a.shape[1] if trans else a.shape[0]))
    (op.trans_op if trans else op.op)(1.0, _sl(L, v), 0.0, out)
    out = out.get_ref().copy()
    op.drop()
    ref, scale = S.reference(a, v, trans)
    model = S.SpTileModel(a)
    bound = model.guarantee(v, trans)
    err = np.abs(out - ref)
    print("spike %s %s: worst err / (|A||x|) %.2e, worst err / documented bound %.2e, G = %d"
          % (layout, "T" if trans else "N", _worst(err, scale), _worst(err, bound), model.window_bits(trans)))
    assert np.all(err <= bound + 1e-30)


def _scaled_lp(which, seed):
    """l1reg_lp(1500) with the rows of G and h (which == "rows") or the columns of G and c multiplied by 10^uniform(-3, 3)"""
    c, G, h = l1reg_lp(1500, seed=3)
    rng = np.random.default_rng(seed)
    if which == "rows":
        d = 10.0 ** rng.uniform(-3, 3, h.size)
        G, h = G * d[:, None], h * d
    else:
        d = 10.0 ** rng.uniform(-3, 3, c.size)
        G, c = G * d[None, :], c * d
    A = sp.csc_matrix(G.astype(np.float32))
    A.sort_indices()
    return A, h.astype(np.float32), c.astype(np.float32)


# Tolerances of the iterates 0, 1, 2, 9 (relative to the largest entry of the oracle's iterate): the existing ones of
# test_sparse_lp_workload_iterates_vs_oracle, unless the CONTROL -- the same problem on the two CSR copies, independent kernels with
# plain f32 sums -- exceeds one: then twice the control's measured error.  The tiled route gets the control's tolerances.
_LP_TOLS = {
    "rows": [3e-5, 6e-5, 1e-4, 3e-4],
    "cols": [3e-5, 6e-5, 1e-4, 3e-4],
}


@pytest.mark.parametrize("schedule,two_copies", [("carried", True), ("sweep", False), ("carried", False)],
                         ids=["carried-csr", "sweep-tiled", "carried-tiled"])
@pytest.mark.parametrize("which", ["rows", "cols"])
def test_badly_scaled_sparse_lp_iterates_and_preconditioner_vs_oracle(T, which, schedule, two_copies):
    # through the two-right-hand-side route of the loop and sp_col_k's block maxima (sweep), and the one-right-hand-side products of
    # the carried schedule; the preconditioner is made of the abs-mode row and column sums
    A, b, c = _scaled_lp(which, seed=17)
    got, want = _iterates_vs_oracle(T, A, b, c, [1], [b.size], [0, 1, 2, 9], _LP_TOLS[which], schedule,
                                    sparse_two_copies=two_copies, report="scaled lp %s %s %s" % (which, schedule, "csr" if two_copies else "tiled"))
    n, m = c.size, b.size
    N = n + 2 * m + 1
    for name, g, r in (("tau", got[0], want[:N]), ("sigma", got[1], want[N:])):
        rel = np.abs(g - r) / np.abs(r)
        print("scaled lp %s %s %s: preconditioner %s worst relative error %.2e" % (which, schedule, "csr" if two_copies else "tiled", name, rel.max()))
        assert np.all(np.isfinite(g)) and np.allclose(g, r, rtol=1e-5, atol=0.0)


def test_create_refuses_missing_column_pointers(T):
    # n_col > 0 needs its n_col + 1 column pointers even without entries
    from totsu_amd._lib import ThipError, E_INVALID, lib
    h = C.c_void_p()
    with pytest.raises(ThipError) as ei:
        lib.thip_sptile_create(5, 3, 0, None, None, None, C.byref(h))
    assert ei.value.code == E_INVALID and not h.value
    # (with them, a matrix without entries is fine)
    cp = np.zeros(4, np.int64)
    lib.thip_sptile_create(5, 3, 0, cp.ctypes.data, None, None, C.byref(h))
    lib.thip_sptile_destroy(h)


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_create_refuses_a_non_finite_stored_value(T, bad):
    # the integer accumulators cannot carry it: it would come out as a finite number
    from totsu_amd._lib import ThipError, E_INVALID, lib
    cp = np.array([0, 1, 3], np.int64)
    ri = np.array([0, 1, 2], np.int32)
    va = np.array([1.0, bad, 2.0], np.float32)
    h = C.c_void_p()
    with pytest.raises(ThipError) as ei:
        lib.thip_sptile_create(3, 2, 3, cp.ctypes.data, ri.ctypes.data, va.ctypes.data, C.byref(h))
    assert ei.value.code == E_INVALID and not h.value


def test_sptile_leaves_the_callers_csc_matrix_alone(T):
    # tocsc() of a CSC matrix is the matrix itself: sorting its indices in place would reorder the caller's arrays
    from totsu_amd.sparse import SpTile
    L = T.F32HIP
    rng = np.random.default_rng(5)
    a = sp.random(500, 300, density=0.05, format="csc", random_state=rng, dtype=np.float32)
    for j in range(300):                                # rows DESCENDING inside every column
        s = slice(a.indptr[j], a.indptr[j + 1])
        a.indices[s], a.data[s] = a.indices[s][::-1].copy(), a.data[s][::-1].copy()
    a.has_sorted_indices = False
    ind, dat, ptr = a.indices.copy(), a.data.copy(), a.indptr.copy()
    t = SpTile(a)
    assert np.array_equal(a.indices, ind) and np.array_equal(a.data, dat) and np.array_equal(a.indptr, ptr)
    assert not a.has_sorted_indices
    x = rng.standard_normal(300).astype(np.float32)
    y = _sl(L, np.zeros(500))
    t.mv(False, 1.0, _sl(L, x), 0.0, y)
    t.free()
    ref, scale = S.reference(a.tocsr(), x)
    assert np.all(np.abs(y.get_ref() - ref) <= 1e-5 * scale + 1e-30)
