"""GPU: the tiled sparse copy built ON THE DEVICE from dense column-major panels (thip_sptile_builder_*, thip_sptile_from_dense,
SpTile.from_dense / SpTile.Builder, FusedSolver(a_layout=...)).  Route H is SpTile(scipy.sparse.csc_matrix(dense)) -- the host
assembly of thip_sptile_create --, route D the device build; the contract is IDENTITY: thip_test_sptile_equal compares every part of
the two objects (directory, items, exponent codes, indices, values bit for bit), so the products and the solver's iterates are
bitwise those of the host route.  H, the dense array and its device copy are made once per matrix and shared."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import sptile_numpy as S

pytestmark = pytest.mark.gpu

PARTS = ["equal", "dimensions / nnz", "nnz_pad / nidx / ndense / max_visit", "headN / headT", "slN / slT / item counts", "tiles",
         "order", "itemsN / itemsT", "rexp / cexp", "idx", "vals"]


@pytest.fixture(scope="module")
def T():
    import totsu_amd
    from totsu_amd import _lib
    _lib.init()
    return totsu_amd


def _first_difference(a, b):
    from totsu_amd._lib import lib
    d = C.c_int(-1)
    lib.thip_test_sptile_equal(a.h, b.h, C.byref(d))
    return PARTS[d.value]


def _flat(d):
    return np.asfortranarray(d, dtype=np.float32).ravel(order="F")


def _dense_of(name):
    if name == "with_full_tiles":
        return S.with_full_tiles(np.random.default_rng(5))
    if name == "diag4097":
        d = np.zeros((4097, 4097), np.float32)
        d[np.arange(4097), np.arange(4097)] = np.arange(1, 4098, dtype=np.float32)
        return d
    if name == "one":
        return np.array([[3.5]], np.float32)
    if name == "quads":                 # 5 x 3, column non-zero counts 1, 2, 3: the padding of a tile to whole quads
        d = np.zeros((5, 3), np.float32)
        d[2, 0] = 1.0
        d[[0, 4], 1] = [2.0, -3.0]
        d[[1, 2, 3], 2] = [4.0, 5.0, -6.0]
        return d
    if name == "zeros100":
        return np.zeros((100, 100), np.float32)
    if name == "norows":
        return np.zeros((0, 5), np.float32)
    if name == "nocols":
        return np.zeros((7, 0), np.float32)
    return S._pattern(name).toarray().astype(np.float32)       # a LAYOUTS shape with its random pattern


_CACHE = {}


def _case(name):
    """(dense f32 array, H, DeviceBuffer of the column-major matrix): made once, never changed"""
    if name not in _CACHE:
        from totsu_amd.fused import DeviceBuffer
        from totsu_amd.sparse import SpTile
        d = _dense_of(name)
        _CACHE[name] = (d, SpTile(sp.csc_matrix(d)), DeviceBuffer.from_host(_flat(d)) if d.size else DeviceBuffer(1))
    return _CACHE[name]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for d, h, buf in _CACHE.values():
        h.free()
        buf.free()
    _CACHE.clear()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. identity
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["with_full_tiles", "single", "staged", "lite", "tall", "wide50", "diag4097", "one", "quads",
                                  "zeros100", "norows", "nocols"])
def test_device_build_is_the_host_build(T, name):
    from totsu_amd.sparse import SpTile
    d, H, buf = _case(name)
    D = SpTile.from_dense(buf, d.shape[0], d.shape[1])
    assert _first_difference(H, D) == "equal"
    assert D.info() == H.info()
    assert D.info()["nnz"] == np.count_nonzero(d)
    D.free()
    # the one-call form of the C ABI (no nnz comes back from it: the Python class goes through the builder)
    from totsu_amd._lib import lib
    h = C.c_void_p()
    lib.thip_sptile_from_dense(d.shape[0], d.shape[1], buf.ptr, d.shape[0], C.byref(h))
    D2 = SpTile.__new__(SpTile)
    D2.shape, D2.nnz, D2.h = d.shape, H.nnz, h
    assert _first_difference(H, D2) == "equal"
    D2.free()


def test_full_tile_matrix_has_the_layout_the_host_route_gives_it(T):
    # (what `with_full_tiles` is for: the device route finds the same tiles without indices)
    _, H, _ = _case("with_full_tiles")
    assert H.info()["dense_tiles"] == 2


def test_signed_zeros_are_dropped_and_subnormals_kept(T):
    from totsu_amd.sparse import SpTile
    rng = np.random.default_rng(11)
    d = rng.standard_normal((300, 40)).astype(np.float32)
    d[rng.uniform(size=d.shape) < 0.5] = 0.0
    d[rng.uniform(size=d.shape) < 0.1] = -0.0
    sub = rng.uniform(size=d.shape) < 0.1
    d[sub] = np.array([1, 0x80000001, 0x007fffff, 0x80400000], np.uint32).view(np.float32)[rng.integers(4, size=int(sub.sum()))]
    d[:, 7] = np.float32(1e-42)                                 # a column of subnormals only: the smallest exponent code
    bits = d.view(np.uint32) & np.uint32(0x7fffffff)
    stored = bits != 0
    assert (d.view(np.uint32) == 0x80000000).any() and ((bits != 0) & (bits < 0x00800000)).any()
    # the CSC form with the zeros dropped BY THEIR BITS (no float comparison, whatever the host's denormal mode)
    cols, rows = np.nonzero(stored.T)
    colptr = np.concatenate([[0], np.cumsum(stored.sum(axis=0))]).astype(np.int64)
    H = SpTile.from_csc_arrays(300, 40, colptr, rows.astype(np.int32), np.ascontiguousarray(d.T[stored.T], dtype=np.float32))
    D = SpTile.from_dense(_flat(d), 300, 40)
    assert D.info()["nnz"] == int(stored.sum())
    assert _first_difference(H, D) == "equal" and D.info() == H.info()
    H.free()
    D.free()


# ---------------------------------------------------------------------------------------------------------------------------
# 2. panels: any widths, any order, any leading dimension
# ---------------------------------------------------------------------------------------------------------------------------
def _build(shape, count_panels, fill_panels, ptr, ld):
    """panels: (c0, ncols) in the order they are fed; the matrix at device address ptr with leading dimension ld"""
    from totsu_amd.sparse import SpTile
    b = SpTile.Builder(*shape)
    for c0, nc in count_panels:
        b.count(c0, nc, ptr + 4 * c0 * ld, ld)
    b.plan()
    for c0, nc in fill_panels:
        b.fill(c0, nc, ptr + 4 * c0 * ld, ld)
    return b.finish()


def _split(n, widths):
    """panels of the given widths, repeated until the n columns are covered"""
    out, c0, k = [], 0, 0
    while c0 < n:
        w = min(widths[k % len(widths)], n - c0)
        out.append((c0, w))
        c0 += w
        k += 1
    return out


@pytest.mark.parametrize("feed", ["4000+106", "1+4095+10", "reverse", "different-splits"])
@pytest.mark.parametrize("name", ["with_full_tiles", "staged"])
def test_panel_widths_and_order_do_not_matter(T, name, feed):
    d, H, buf = _case(name)
    m, n = d.shape
    if feed == "4000+106":              # crosses the 4096 boundary
        cp = fp = _split(n, [4000, 106])
    elif feed == "1+4095+10":
        cp = fp = _split(n, [1, 4095, 10])
    elif feed == "reverse":
        cp = fp = _split(n, [1500])[::-1]
    else:
        cp, fp = _split(n, [777, 2048]), _split(n, [4096, 33])[::-1]
    D = _build((m, n), cp, fp, buf.ptr, m)
    assert _first_difference(H, D) == "equal" and D.info() == H.info()
    D.free()


@pytest.mark.parametrize("name,c0", [("with_full_tiles", 3806), ("staged", 3950)])
def test_panels_of_one_column(T, name, c0):
    # on a 300-column slice that crosses the 4096 boundary of its matrix (the slice is a matrix of its own)
    from totsu_amd.sparse import SpTile
    d, _, buf = _case(name)
    m = d.shape[0]
    H = SpTile(sp.csc_matrix(d[:, c0:c0 + 300]))
    one = [(j, 1) for j in range(300)]
    D = _build((m, 300), one, one, buf.ptr + 4 * c0 * m, m)
    assert _first_difference(H, D) == "equal" and D.info() == H.info()
    H.free()
    D.free()


@pytest.mark.parametrize("name", ["with_full_tiles", "staged"])
def test_padded_leading_dimension_with_nan_in_the_pad_rows(T, name):
    # ld = n_row + 5 (no 16-byte alignment of the columns either): rows n_row .. ld - 1 are never read as data
    from totsu_amd.fused import DeviceBuffer
    from totsu_amd.sparse import SpTile
    d, H, _ = _case(name)
    m, n = d.shape
    padded = np.full((n, m + 5), np.nan, np.float32)
    padded[:, :m] = d.T
    buf = DeviceBuffer.from_host(padded.ravel())
    D = SpTile.from_dense(buf, m, n, ld=m + 5)
    buf.free()
    assert _first_difference(H, D) == "equal" and D.info() == H.info()
    D.free()


@pytest.mark.parametrize("name", ["with_full_tiles", "staged"])
def test_host_array_streamed_through_a_staging_buffer(T, name):
    from totsu_amd.sparse import SpTile
    d, H, buf = _case(name)
    m, n = d.shape
    Dd = SpTile.from_dense(buf, m, n)
    Dh = SpTile.from_dense(d, m, n, panel_cols=7)          # 2-D host array, read column by column, 7 columns per panel
    assert _first_difference(Dd, Dh) == "equal" and _first_difference(H, Dh) == "equal"
    assert Dh.info() == Dd.info() == H.info()
    Dd.free()
    Dh.free()


def test_flat_host_array_with_the_default_panel(T):
    from totsu_amd.sparse import SpTile
    d, H, _ = _case("single")
    D = SpTile.from_dense(_flat(d), *d.shape)
    assert _first_difference(H, D) == "equal"
    D.free()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. products
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["with_full_tiles", "staged"])
def test_products_are_bitwise_those_of_the_host_route(T, name):
    from totsu_amd.sparse import SpTile
    L = T.F32HIP
    d, H, buf = _case(name)
    m, n = d.shape
    D = SpTile.from_dense(buf, m, n)
    rng = np.random.default_rng(3)
    for trans in (False, True):
        x = L.Sl.new_mut(rng.standard_normal(m if trans else n).astype(np.float32))
        for abs_mode in (0, 1):
            out = []
            for mat in (H, D):
                y = L.Sl.new_mut(np.zeros(n if trans else m, np.float32))
                mat.mv(trans, 1.0, x, 0.0, y, abs_mode=abs_mode)
                out.append(y.get_ref().copy())
                y.drop()
            assert np.abs(out[0]).max() > 0
            assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32)), (trans, abs_mode)
        x.drop()
    D.free()


# ---------------------------------------------------------------------------------------------------------------------------
# 4. errors: THIP_E_INVALID, nothing launched / nothing written out of range
# ---------------------------------------------------------------------------------------------------------------------------
def _invalid(f, *a):
    from totsu_amd import _lib
    with pytest.raises(_lib.ThipError) as e:
        f(*a)
    assert e.value.code == _lib.E_INVALID


def test_builder_errors(T):
    from totsu_amd.fused import DeviceBuffer
    from totsu_amd.sparse import SpTile
    rng = np.random.default_rng(1)
    m, n = 50, 8
    d = rng.standard_normal((m, n)).astype(np.float32)
    d[rng.uniform(size=d.shape) < 0.6] = 0.0
    d[:, 3] = 0.0
    d[[4, 9], 3] = [1.0, 2.0]
    buf = DeviceBuffer.from_host(_flat(d))
    # a NaN / an Inf entry: reported at plan
    for v in (np.nan, np.inf, -np.inf):
        bad = d.copy()
        bad[17, 5] = v
        bbuf = DeviceBuffer.from_host(_flat(bad))
        b = SpTile.Builder(m, n)
        b.count(0, n, bbuf)
        _invalid(b.plan)
        b.destroy()
        bbuf.free()
    # a column counted twice; plan with a column missing; fill before plan; a panel past n_col; ld < n_row
    b = SpTile.Builder(m, n)
    b.count(0, 5, buf)
    _invalid(b.count, 4, 2, buf.ptr + 4 * 4 * m)
    _invalid(b.plan)
    _invalid(b.fill, 0, 5, buf)
    _invalid(b.count, 5, 4, buf.ptr + 4 * 5 * m)
    _invalid(b.count, 9, 1, buf.ptr)
    _invalid(b.count, 5, 3, buf.ptr + 4 * 5 * m, m - 1)
    _invalid(b.count, 5, 3, None)
    b.count(5, 3, buf.ptr + 4 * 5 * m)          # (the refused calls marked nothing: the columns are still free)
    b.plan()
    # a column filled twice; finish with a column unfilled
    b.fill(0, 5, buf)
    _invalid(b.fill, 2, 1, buf.ptr + 4 * 2 * m)
    h = C.c_void_p()
    from totsu_amd._lib import lib
    _invalid(lib.thip_sptile_builder_finish, b.h, C.byref(h))
    b.fill(5, 3, buf.ptr + 4 * 5 * m)
    D = b.finish()
    H = SpTile(sp.csc_matrix(d))
    assert _first_difference(H, D) == "equal"
    D.free()
    # a fill panel with MORE non-zeros in one column than were counted (column 3: 2 counted, 50 given), and one with fewer: a device
    # flag, reported at finish
    for fewer in (False, True):
        other = d.copy()
        other[:, 3] = 0.0 if fewer else 7.0
        obuf = DeviceBuffer.from_host(_flat(other))
        b = SpTile.Builder(m, n)
        b.count(0, n, buf)
        b.plan()
        b.fill(0, n, obuf)
        _invalid(lib.thip_sptile_builder_finish, b.h, C.byref(h))
        b.destroy()
        obuf.free()
    # the device is as it was: a build and a product after all of the above
    D = SpTile.from_dense(buf, m, n)
    assert _first_difference(H, D) == "equal"
    L = T.F32HIP
    x, y = L.Sl.new_mut(np.ones(n, np.float32)), L.Sl.new_mut(np.zeros(m, np.float32))
    D.mv(False, 1.0, x, 0.0, y)
    assert np.allclose(y.get_ref(), d.sum(axis=1), rtol=1e-5, atol=1e-5)
    for o in (x, y):
        o.drop()
    for o in (D, H, buf):
        o.free()


def test_overcounted_fill_stays_inside_its_segment(T):
    # the in-kernel bound over two row blocks: column 2 arrives in pass 2 with EVERY row set (5000 entries where ~1500 were counted).
    # The fill writes the counted number of entries and no more -- the store is sized by the counts, so anything else would be an
    # out-of-range write --, finish refuses the object, and the device serves the next build as before
    from totsu_amd._lib import lib
    from totsu_amd.fused import DeviceBuffer
    from totsu_amd.sparse import SpTile
    rng = np.random.default_rng(2)
    m, n = 5000, 6                      # two row blocks
    d = rng.standard_normal((m, n)).astype(np.float32)
    d[rng.uniform(size=d.shape) < 0.7] = 0.0
    more = d.copy()
    more[:, 2] = 1.0                    # every row of column 2 non-zero in pass 2
    buf, mbuf = DeviceBuffer.from_host(_flat(d)), DeviceBuffer.from_host(_flat(more))
    b = SpTile.Builder(m, n)
    b.count(0, n, buf)
    b.plan()
    b.fill(2, 1, mbuf.ptr + 4 * 2 * m)
    for j in (0, 1, 3, 4, 5):
        b.fill(j, 1, buf.ptr + 4 * j * m)
    h = C.c_void_p()
    _invalid(lib.thip_sptile_builder_finish, b.h, C.byref(h))
    b.destroy()
    D, H = SpTile.from_dense(buf, m, n), SpTile(sp.csc_matrix(d))
    assert _first_difference(H, D) == "equal"
    for o in (D, H, buf, mbuf):
        o.free()


# ---------------------------------------------------------------------------------------------------------------------------
# 5. the solver: Prob*.dense() -> FusedSolver.from_dense(..., a_layout="tiled"), no scipy object in the call
# ---------------------------------------------------------------------------------------------------------------------------
def _mb(T, typ):
    return T.MatBuild(T.F32HIP, typ)


def _prob(T, which):
    from problems import l1reg_lp, partitioning_sdp, toruscompl_socp
    col = lambda v: np.asarray(v, np.float32).reshape(-1, 1)
    if which == "lp":
        c, G, h = l1reg_lp(l=20, seed=1)
        n, m = c.size, h.size
        return T.ProbLP(_mb(T, T.MatType.General(n, 1)).set_array(col(c)), _mb(T, T.MatType.General(m, n)).set_array(G),
                        _mb(T, T.MatType.General(m, 1)).set_array(col(h)), _mb(T, T.MatType.General(0, n)),
                        _mb(T, T.MatType.General(0, 1)))
    if which == "sdp":
        w, syms_f, mat_a, vec_b = partitioning_sdp(6, 5, seed=2)
        l, n = 30, w.size
        return T.ProbSDP(_mb(T, T.MatType.General(n, 1)).set_array(col(w)),
                         [_mb(T, T.MatType.SymPack(l)).set_array(s_) for s_ in syms_f],
                         _mb(T, T.MatType.General(l, n)).set_array(mat_a), _mb(T, T.MatType.General(l, 1)).set_array(col(vec_b)), 1e-12)
    q = toruscompl_socp(9, 7, 0.2)
    n = q["vec_f"].size
    return T.ProbSOCP(_mb(T, T.MatType.General(n, 1)).set_array(col(q["vec_f"])),
                      [_mb(T, T.MatType.General(G.shape[0], n)).set_array(G) for G in q["mats_g"]],
                      [_mb(T, T.MatType.General(len(h_), 1)).set_array(col(h_)) for h_ in q["vecs_h"]],
                      [_mb(T, T.MatType.General(n, 1)).set_array(col(c_)) for c_ in q["vecs_c"]], list(q["scls_d"]),
                      _mb(T, T.MatType.General(q["vec_b"].size, n)).set_array(q["mat_a"]),
                      _mb(T, T.MatType.General(q["vec_b"].size, 1)).set_array(col(q["vec_b"])))


def _scipy_route(T, d, param, schedule):
    A = np.asarray(d.mat_a, np.float32).reshape((d.m, d.n), order="F")
    return A, T.FusedSolver(d.n, d.m, sp.csc_matrix(A), d.vec_b, d.vec_c, d.seg_type, d.seg_len, param, schedule, d.vec_b_rowabs)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("schedule", ["sweep", "fused"])
@pytest.mark.parametrize("which", ["lp", "sdp", "socp"])
def test_solver_on_the_device_built_copy_is_bitwise_the_scipy_route(T, which, schedule):
    prob = _prob(T, which)
    d = prob.dense()
    p = T.SolverParam()
    p.eps_acc = 0.0
    fd = T.FusedSolver.from_dense(d, p, schedule=schedule, a_layout="tiled")
    A, fh = _scipy_route(T, d, p, schedule)
    assert fd.a_layout == "tiled" and fd.sptile_info()["nnz"] == np.count_nonzero(A)
    assert fd.sptile_info() == fh.sptile_info()
    assert fd.schedule_in_use() == fh.schedule_in_use() == schedule
    rd, rh = fd.run(50, poll_every=64), fh.run(50, poll_every=64)
    assert rd.iters == rh.iters == 50
    for a, b in zip(fd.iterate(), fh.iterate()):
        assert np.array_equal(_bits(a), _bits(b))
    assert np.array_equal(_bits(rd.cri), _bits(rh.cri))
    fd.destroy()
    fh.destroy()
    prob.drop()


def test_converged_lp_stops_at_the_same_iteration(T):
    prob = _prob(T, "lp")
    d = prob.dense()
    p = T.SolverParam()
    p.eps_acc = 1e-3
    fd = T.FusedSolver.from_dense(d, p, schedule="sweep", a_layout="tiled")
    _, fh = _scipy_route(T, d, p, "sweep")
    xd, _ = fd.solve()
    xh, _ = fh.solve()
    assert fd.status().iters == fh.status().iters > 0
    assert np.array_equal(_bits(xd), _bits(xh))
    fd.destroy()
    fh.destroy()
    prob.drop()


# ---------------------------------------------------------------------------------------------------------------------------
# 6. a_layout="auto"
# ---------------------------------------------------------------------------------------------------------------------------
def test_auto_takes_the_tiled_copy_of_a_mostly_zero_matrix(T):
    prob = _prob(T, "sdp")
    d = prob.dense()
    fs = T.FusedSolver.from_dense(d, T.SolverParam(), schedule="sweep", a_layout="auto")
    assert fs.a_layout == "tiled" and fs.sptile_info()["nnz"] == np.count_nonzero(np.asarray(d.mat_a))
    fs.destroy()
    prob.drop()


def test_auto_keeps_a_random_dense_matrix_dense(T):
    from problems import benchmark_lp
    c, G, h = benchmark_lp(96, seed=4)
    n, m = c.size, h.size
    p = T.SolverParam()
    p.eps_acc = 0.0
    sol = [T.FusedSolver(n, m, _flat(G), h, c, [1], [m], p, gemv_autotune=False, **kw) for kw in ({"a_layout": "auto"}, {})]
    assert sol[0].a_layout == sol[1].a_layout == "dense" and sol[0].sptile_info() is None
    for _ in range(10):
        for s in sol:
            s.run(1)
        for a, b in zip(sol[0].iterate(), sol[1].iterate()):
            assert np.array_equal(_bits(a), _bits(b))
    for s in sol:
        s.destroy()
