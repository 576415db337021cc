"""CPU: the shape rules of the streamed mid-size batch (thip_midbatch_fits needs no device), the Python-side checks of
MidBatchSolver and the choice own_a_batch makes between the small and the mid batch."""
import ctypes as C

import numpy as np
import pytest

from totsu_amd import _lib
from totsu_amd import midbatch as MB
from totsu_amd import smallbatch as SB
from totsu_amd.problem import _Dense

RPOS = [_lib.CONE_RPOS]
LDS = 163840
FIXED = 64 + 4096 + 2048          # floats of LDS beside the vectors: the block sums, the row-sum and the column-sum scratch


def _fits_rc(n, m, seg_type, seg_len):
    """the raw return code, lds_bytes, threads"""
    lib = _lib.load()
    st = np.ascontiguousarray(seg_type, dtype=np.int32)
    sl = np.ascontiguousarray(seg_len, dtype=np.int64)
    lds, thr = C.c_size_t(0), C.c_int(0)
    rc = lib.thip_midbatch_fits(n, m, st.size, st.ctypes.data_as(C.POINTER(C.c_int32)), sl.ctypes.data_as(C.POINTER(C.c_int64)),
                                C.byref(lds), C.byref(thr))
    return rc, lds.value, thr.value


def test_fits_accepts_the_whole_floor_boundary():
    """every m in 1 .. 2520 with the largest n of 8 n + 13 m <= 32 768 (capped at 4096)"""
    worst = (0, 0, 0)
    for m in range(1, 2521):
        n = min(4096, (32768 - 13 * m) // 8)
        assert n >= 1
        rc, lds, thr = _fits_rc(n, m, RPOS, [m])
        assert rc == 0, (m, n, rc)
        assert 0 < lds <= LDS, (m, n, lds)
        assert lds == 4 * (FIXED + 8 * n + 13 * m) + ((m + 3) & ~3), (m, n, lds)
        assert thr in (256, 1024), (m, n, thr)
        worst = max(worst, (lds, m, n))
    print("largest workgroup on the floor's edge: %d bytes of LDS at m = %d, n = %d" % worst)


def test_fits_python_wrapper_and_thread_choice():
    lds, thr = MB.fits(260, 520, RPOS, [520])
    assert thr == 1024 and lds == 4 * (FIXED + 8 * 260 + 13 * 520) + 520
    assert MB.fits(1, 1, RPOS, [1])[1] == 256                      # small shapes are taken: the edge tests run them
    assert MB.fits(40, 80, [_lib.CONE_RPOS, _lib.CONE_ZERO], [80, 0])[1] == 256
    assert MB.fits(128, 65, RPOS, [65])[1] == 1024                 # 8320 > 8192 entries
    assert MB.fits(60, 400, [2, 2, 2, 2, 3, 0], [200, 130, 2, 1, 60, 7])[0] > 0


@pytest.mark.parametrize("n,m,seg_type,seg_len", [
    (8, 4097, RPOS, [4097]),                     # m beyond 4096
    (4097, 8, RPOS, [8]),                        # n beyond 4096
    (1000, 2020, RPOS, [2020]),                  # the first m whose map exceeds LDS at n = 1000
    (1, 1, RPOS + RPOS, [1, 1]),                 # segments that sum to more than m
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
        MB.fits(n, m, seg_type, seg_len)


def test_lds_limit_is_exact():
    """4 (6208 + 8 n + 13 m) + roundup4(m) <= 163 840.  At n = 1000: 56 832 + 52 m + roundup4(m) -- m = 2019 gives exactly
    163 840, m = 2020 gives 163 892"""
    assert 4 * (FIXED + 8000 + 13 * 2019) + 2020 == LDS
    rc, lds, _ = _fits_rc(1000, 2019, RPOS, [2019])
    assert rc == 0 and lds == LDS
    assert _fits_rc(1000, 2020, RPOS, [2020])[0] == _lib.E_INVALID
    assert _fits_rc(1000, 2000, RPOS, [2000])[0] == 0                  # beyond the floor (34 000 floats of vectors), still taken
    assert _fits_rc(4096, 100, RPOS, [100])[0] == 0                    # 161 204 bytes
    assert _fits_rc(4096, 200, RPOS, [200])[0] == _lib.E_INVALID       # 166 504 bytes
    assert _fits_rc(1, 2520, RPOS, [2520])[0] == 0
    assert _fits_rc(1, 3100, RPOS, [3100])[0] == _lib.E_INVALID


def _dense(n, m, seg_type, seg_len, rowabs=False, seed=0):
    rng = np.random.default_rng(seed)
    f = np.float32
    b = rng.standard_normal(m).astype(f)
    return _Dense(n, m, rng.standard_normal(m * n).astype(f), b, rng.standard_normal(n).astype(f), seg_type, seg_len,
                  np.abs(b) if rowabs else None)


def test_from_dense_checks_need_no_device():
    S = MB.MidBatchSolver
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
    with pytest.raises(ValueError):
        MB.own_a_batch([])
    with pytest.raises(ValueError):
        MB.own_a_batch(ok + [_dense(3, 6, [1, 0], [5, 1])])


def test_constructor_refusals_come_before_the_device():
    """every refusal of the shape, the layout and the array lengths is raised before thip_init is needed"""
    S = MB.MidBatchSolver
    f = np.float32
    z = lambda *s: np.zeros(s, f)
    with pytest.raises(ValueError):
        S(3, 6, z(2, 18), z(2, 6), z(2, 3), [_lib.CONE_PSD], [6])
    with pytest.raises(ValueError):
        S(2, 4097, z(1, 2 * 4097), z(1, 4097), z(1, 2), RPOS, [4097])
    with pytest.raises(ValueError):
        S(4097, 2, z(1, 2 * 4097), z(1, 2), z(1, 4097), RPOS, [2])
    with pytest.raises(ValueError):                                   # the map exceeds LDS
        S(1000, 2020, z(1, 1), z(1, 2020), z(1, 1000), RPOS, [2020])
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


@pytest.mark.parametrize("m,n,want", [(156, 157, "small"), (157, 157, "mid"), (80, 40, "small"), (2000, 1000, "mid")])
def test_own_a_batch_choice(m, n, want):
    assert MB.choose(n, m, RPOS, [m]) == want
    assert want == ("small" if m * n <= 24576 and max(m, n) <= 1024 else "mid")
    # the choice is the two rules and nothing else
    small_ok = True
    try:
        SB.fits(n, m, RPOS, [m])
    except ValueError:
        small_ok = False
    assert small_ok == (want == "small")
    MB.fits(n, m, RPOS, [m])                                          # the mid batch takes every one of these shapes


def test_own_a_batch_refuses_by_naming_fused_solver():
    with pytest.raises(ValueError, match="FusedSolver"):
        MB.choose(8, 4097, RPOS, [4097])
    with pytest.raises(ValueError, match="FusedSolver"):
        MB.own_a_batch([_dense(8, 4097, RPOS, [4097])])
    with pytest.raises(ValueError, match="FusedSolver"):             # PSD: neither batch
        MB.own_a_batch([_dense(3, 6, [_lib.CONE_PSD], [6])])
    import totsu_amd
    assert totsu_amd.own_a_batch is MB.own_a_batch and totsu_amd.MidBatchSolver is MB.MidBatchSolver
