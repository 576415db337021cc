"""CPU: the shape rules of the on-chip small batch (thip_smallbatch_fits needs no device) and the Python-side checks of
SmallBatchSolver.from_dense."""
import ctypes as C

import numpy as np
import pytest

from totsu_amd import _lib
from totsu_amd import smallbatch as SB
from totsu_amd.problem import _Dense

RPOS = [_lib.CONE_RPOS]


def _fits_rc(n, m, seg_type, seg_len):
    """the raw return code, lds_bytes, threads"""
    lib = _lib.load()
    st = np.ascontiguousarray(seg_type, dtype=np.int32)
    sl = np.ascontiguousarray(seg_len, dtype=np.int64)
    lds, thr = C.c_size_t(0), C.c_int(0)
    rc = lib.thip_smallbatch_fits(n, m, st.size, st.ctypes.data_as(C.POINTER(C.c_int32)), sl.ctypes.data_as(C.POINTER(C.c_int64)),
                                  C.byref(lds), C.byref(thr))
    return rc, lds.value, thr.value


def test_fits_accepts_the_whole_boundary():
    worst = (0, 0, 0)
    for m in range(1, 1025):
        n = min(1024, 24576 // m)
        rc, lds, thr = _fits_rc(n, m, RPOS, [m])
        assert rc == 0, (m, n, rc)
        assert 0 < lds <= 163840, (m, n, lds)
        assert thr in (64, 256, 1024), (m, n, thr)
        worst = max(worst, (lds, m, n))
    print("largest workgroup: %d bytes of LDS at m = %d, n = %d" % worst)


def test_fits_python_wrapper_and_thread_choice():
    lds, thr = SB.fits(40, 80, [_lib.CONE_RPOS, _lib.CONE_ZERO], [80, 0])
    assert thr == 256 and lds <= 163840
    assert SB.fits(1, 1, RPOS, [1])[1] == 64
    assert SB.fits(128, 192, RPOS, [192])[1] == 1024
    # mixed cones, a segment of no rows, a cone of one row
    assert SB.fits(12, 102, [2, 2, 2, 2, 2, 2, 0], [6, 2, 1, 18, 71, 4, 0])[0] > 0


@pytest.mark.parametrize("n,m,seg_type,seg_len", [
    (24, 1025, RPOS, [1025]),                    # m beyond 1024
    (1025, 24, RPOS, [24]),                      # n beyond 1024
    (1, 24577, RPOS, [24577]),
    (24577, 1, RPOS, [1]),
    (128, 193, RPOS, [193]),                     # m * n = 24 704: the first m beyond the area limit at n = 128
    (1, 1, RPOS + RPOS, [1, 1]),                     # segments that sum to more than m
    (3, 7, RPOS, [6]),                           # ... to less
    (0, 4, RPOS, [4]),
    (4, 0, RPOS, [0]),
    (3, 6, [_lib.CONE_PSD], [6]),                # a PSD layout
    (3, 8, [_lib.CONE_RPOS, _lib.CONE_PSD], [2, 6]),
    (3, 6, [7], [6]),                            # no such cone
    (3, 6, RPOS, [-6]),
])
def test_fits_refuses(n, m, seg_type, seg_len):
    rc, _, _ = _fits_rc(n, m, seg_type, seg_len)
    assert rc == _lib.E_INVALID
    assert _lib.load().thip_last_error()
    with pytest.raises(ValueError):
        SB.fits(n, m, seg_type, seg_len)


def test_area_limit_is_exact():
    assert _fits_rc(128, 192, RPOS, [192])[0] == 0                     # 24 576
    assert _fits_rc(1, 24576, RPOS, [24576])[0] == _lib.E_INVALID      # the area fits, m does not
    assert _fits_rc(24, 1024, RPOS, [1024])[0] == 0
    assert _fits_rc(3, 8192, RPOS, [8192])[0] == _lib.E_INVALID
    assert _fits_rc(157, 157, RPOS, [157])[0] == _lib.E_INVALID        # 24 649 = 24 576 + 73
    assert _fits_rc(156, 157, RPOS, [157])[0] == 0


def _dense(n, m, seg_type, seg_len, rowabs=False, seed=0):
    rng = np.random.default_rng(seed)
    f = np.float32
    b = rng.standard_normal(m).astype(f)
    return _Dense(n, m, rng.standard_normal(m * n).astype(f), b, rng.standard_normal(n).astype(f), seg_type, seg_len,
                  np.abs(b) if rowabs else None)


def test_from_dense_checks_need_no_device():
    S = SB.SmallBatchSolver
    ok = [_dense(3, 5, [1, 0], [4, 1], seed=k) for k in range(3)]
    assert S.check_same_layout(ok) == ok
    with pytest.raises(ValueError):
        S.from_dense([])
    with pytest.raises(ValueError):                                   # another shape
        S.from_dense(ok + [_dense(3, 6, [1, 0], [5, 1])])
    with pytest.raises(ValueError):
        S.from_dense(ok + [_dense(4, 5, [1, 0], [4, 1])])
    with pytest.raises(ValueError):                                   # the same rows in other segments
        S.from_dense(ok + [_dense(3, 5, [1, 0], [3, 2])])
    with pytest.raises(ValueError):                                   # the same segments of other cones
        S.from_dense(ok + [_dense(3, 5, [1, 2], [4, 1])])
    with pytest.raises(ValueError):                                   # one carries vec_b_rowabs, the others do not
        S.from_dense(ok + [_dense(3, 5, [1, 0], [4, 1], rowabs=True)])
    bad = _dense(3, 5, [1, 0], [4, 1])
    bad.mat_a = bad.mat_a[:-1]
    with pytest.raises(ValueError):
        S.from_dense(ok + [bad])


def test_constructor_refusals_come_before_the_device():
    """every refusal of the shape, the layout and the array lengths is raised before thip_init is needed"""
    S = SB.SmallBatchSolver
    f = np.float32
    z = lambda *s: np.zeros(s, f)
    with pytest.raises(ValueError):
        S(3, 6, z(2, 18), z(2, 6), z(2, 3), [_lib.CONE_PSD], [6])
    with pytest.raises(ValueError):
        S(1, 24577, z(1, 24577), z(1, 24577), z(1, 1), RPOS, [24577])
    with pytest.raises(ValueError):
        S(24, 1025, z(1, 24 * 1025), z(1, 1025), z(1, 24), RPOS, [1025])
    with pytest.raises(ValueError):
        S(3, 6, z(2, 18), z(2, 6), z(2, 3), RPOS, [5])
    with pytest.raises(ValueError):                                   # P = 0
        S(3, 6, z(0, 18), z(0, 6), z(0, 3), RPOS, [6])
    with pytest.raises(ValueError):                                   # arrays of the wrong length
        S(3, 6, z(2, 17), z(2, 6), z(2, 3), RPOS, [6])
    with pytest.raises(ValueError):
        S(3, 6, z(2, 18), z(2, 6), z(3, 3), RPOS, [6])
    with pytest.raises(ValueError):
        S(3, 6, z(2, 18), z(2, 6), z(2, 3), RPOS, [6], vecs_b_rowabs=z(1, 6))
