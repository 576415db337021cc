"""CPU: the shape rule of the wide batch (thip_widebatch_fits needs no device) against its restatement, the shapes the family exists
for, its refusals -- each in its own words --, what the mid and the SDP batch answer on the same shapes (what they answered before:
their own restated rules), the Python-side checks of WideBatchSolver, and that no chooser returns the class."""
import ctypes as C

import numpy as np
import pytest

from totsu_amd import _lib
from totsu_amd import midbatch as MB
from totsu_amd import sdpbatch as SP
from totsu_amd import widebatch as WB
from totsu_amd.problem import _Dense

ZERO, RPOS, SOC, ROTSOC, PSD = _lib.CONE_ZERO, _lib.CONE_RPOS, _lib.CONE_SOC, _lib.CONE_ROTSOC, _lib.CONE_PSD
LDS = 163840
FIXED = 64 + 4096 + 2048          # floats of LDS beside the vectors: the block sums, the row-sum and the column-sum scratch
TAIL = 3 * 64 * 65 * 4            # bytes of the three operands that do not overlay the pass scratch (orders above 32)


def tri(k):
    return k * (k + 1) // 2


def rule(n, m, max_k):
    """README.md / DESIGN.md 4.2, restated: the pass vectors (x_x u x_y v, g h), the class bytes, and 49 920 bytes when the largest
    PSD order exceeds 32"""
    return 4 * (FIXED + 3 * n + 3 * m) + ((m + 3) & ~3) + (TAIL if max_k > 32 else 0)


def old_rule(n, m, max_k):
    """the mid batch's map (every vector in LDS), and the SDP batch's tail"""
    return 4 * (FIXED + 8 * n + 13 * m) + ((m + 3) & ~3) + (TAIL if max_k > 32 else 0)


def _fits_rc(name, n, m, seg_type, seg_len):
    """the raw return code, lds_bytes, threads, message of thip_<name>_fits"""
    lib = _lib.load()
    st = np.ascontiguousarray(seg_type, dtype=np.int32)
    sl = np.ascontiguousarray(seg_len, dtype=np.int64)
    lds, thr = C.c_size_t(0), C.c_int(0)
    rc = getattr(lib, "thip_%s_fits" % name)(n, m, st.size, st.ctypes.data_as(C.POINTER(C.c_int32)),
                                             sl.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(lds), C.byref(thr))
    return rc, lds.value, thr.value, (lib.thip_last_error() or b"").decode() if rc else ""


def wide(n, m, seg_type, seg_len):
    return _fits_rc("widebatch", n, m, seg_type, seg_len)


def test_rule_restated_over_a_grid():
    """thip_widebatch_fits is the restated rule: every m, n of a grid to 4096 with no PSD cone (always accepted), and with one PSD cone
    of every order 1 .. 64 in front of nonnegative rows (accepted exactly when the rule holds)"""
    dims = (1, 2, 3, 5, 64, 255, 256, 257, 1000, 2020, 2986, 2987, 4095, 4096)
    for m in dims:
        for n in dims:
            rc, lds, thr, _ = wide(n, m, [RPOS], [m])
            assert rc == 0 and lds == rule(n, m, 0) <= LDS, (m, n, rc, lds)
            assert thr == (256 if n * m <= 8192 else 1024)
    assert rule(4096, 4096, 0) == 127232
    for k in range(1, 65):
        for m in sorted(set((tri(k), tri(k) + 5, 2600, 4096))):
            if m < tri(k):
                continue
            st, sl = ([PSD], [m]) if m == tri(k) else ([PSD, RPOS], [tri(k), m - tri(k)])
            for n in (1, 48, 837, 2986, 2987, 4096):
                rc, lds, _, _ = wide(n, m, st, sl)
                want = rule(n, m, k)
                assert (rc == 0) == (want <= LDS), (k, m, n, rc, want)
                if rc == 0:
                    assert lds == want, (k, m, n, lds, want)
                if k > 32:
                    assert (want <= LDS) == (12 * (n + m) + ((m + 3) & ~3) <= 89088)
    # several cones: the largest order decides
    m = tri(3) + tri(33) + tri(6)
    assert wide(5, m, [PSD] * 3, [tri(3), tri(33), tri(6)])[1] == rule(5, m, 33)
    m = tri(3) + tri(32) + tri(6)
    assert wide(5, m, [PSD] * 3, [tri(3), tri(32), tri(6)])[1] == rule(5, m, 32)
    # all five cones in one layout
    rc, lds, _, _ = wide(7, 3 + 4 + 9 + 5 + tri(40), [ZERO, RPOS, SOC, ROTSOC, PSD], [3, 4, 9, 5, tri(40)])
    assert rc == 0 and lds == rule(7, 21 + tri(40), 40)


# (m, n, seg_type, seg_len, largest order, does the mid / SDP batch take it)
ACCEPTED = [(2020, 1000, [RPOS], [2020], 0),                  # the first m the mid batch refuses at n = 1000
            (2521, 1, [RPOS], [2521], 0),                     # the smallest shapes beyond 8 n + 13 m <= 32 768
            (2, 4096, [RPOS], [2], 0),
            (4096, 4096, [RPOS], [4096], 0),
            (tri(64), 4096, [PSD], [tri(64)], 64),            # an order-64 cone alone takes every n
            (tri(48), 837, [PSD], [tri(48)], 48)]             # the first n the SDP batch refuses at order 48


@pytest.mark.parametrize("m,n,seg_type,seg_len,max_k", ACCEPTED)
def test_shapes_beyond_the_old_rules_are_accepted(m, n, seg_type, seg_len, max_k):
    rc, lds, thr, msg = wide(n, m, seg_type, seg_len)
    assert rc == 0 and lds == rule(n, m, max_k) <= LDS, msg
    assert WB.fits(n, m, seg_type, seg_len) == (lds, thr) and WB.lds_rule(n, m, max_k) == lds
    # beyond the rule of thumb 8 n + 13 m <= 32 768 (with a tail: beyond the SDP batch's map); the batches before this one answer by
    # their own maps, in the words they had (2521 x 1 and 2 x 4096 lie in the 3072 floats between the rule of thumb and the map)
    assert 8 * n + 13 * m > 32768 or max_k > 32
    refused = old_rule(n, m, max_k) > LDS
    assert refused == ((m, n) not in ((2521, 1), (2, 4096)))
    for name in ("sdpbatch",) + (("midbatch",) if max_k == 0 else ()):
        rc, old_lds, _, msg = _fits_rc(name, n, m, seg_type, seg_len)
        if refused:
            assert rc == _lib.E_INVALID and "do not fit the LDS" in msg
        else:
            assert rc == 0 and old_lds == old_rule(n, m, max_k)


def test_the_edges_the_old_rules_name():
    assert _fits_rc("midbatch", 1000, 2000, [RPOS], [2000])[0] == 0 and _fits_rc("midbatch", 1000, 2020, [RPOS], [2020])[0] != 0
    assert 8 * 1 + 13 * 2520 <= 32768 < 8 * 1 + 13 * 2521 and 32768 < 8 * 4096 + 13 * 2
    assert _fits_rc("sdpbatch", 836, tri(48), [PSD], [tri(48)])[0] == 0
    for k in range(58, 65):                                    # legal orders whose vectors alone did not fit: all taken here
        assert _fits_rc("sdpbatch", 1, tri(k), [PSD], [tri(k)])[0] == _lib.E_INVALID
        assert wide(1, tri(k), [PSD], [tri(k)])[0] == 0 and wide(4096, tri(k), [PSD], [tri(k)])[0] == 0


REFUSED = [(8, 4097, [RPOS], [4097], "m <= 4096"),                                    # m = 4097
           (4097, 8, [RPOS], [8], "n <= 4096"),                                       # n = 4097
           (2987, 4096, [PSD, RPOS], [tri(33), 4096 - tri(33)], "do not fit the LDS"),  # the map: an order above 32 at m = 4096
           (3, 7, [PSD], [7], "triangular"),                                          # a PSD length of 7
           (3, tri(65), [PSD], [tri(65)], "above 64")]                                # order 65


@pytest.mark.parametrize("n,m,seg_type,seg_len,word", REFUSED)
def test_fits_refuses(n, m, seg_type, seg_len, word):
    rc, _, _, msg = wide(n, m, seg_type, seg_len)
    assert rc == _lib.E_INVALID and word in msg, msg
    with pytest.raises(ValueError):
        WB.fits(n, m, seg_type, seg_len)


def test_each_refusal_has_its_own_message():
    msgs = [wide(*r[:4])[3] for r in REFUSED]
    assert all(msgs) and len(set(msgs)) == len(REFUSED), msgs


def test_the_map_limit_is_exact_at_m_4096():
    """m = 4096 holding an order-33 cone: n = 2986 is the last one taken (12 (n + m) + m <= 89 088)"""
    st, sl = [PSD, RPOS], [tri(33), 4096 - tri(33)]
    rc, lds, _, _ = wide(2986, 4096, st, sl)
    assert rc == 0 and lds == rule(2986, 4096, 33) == LDS - 8
    assert wide(2987, 4096, st, sl)[0] == _lib.E_INVALID
    assert wide(2986, 4096, [PSD, RPOS], [tri(32), 4096 - tri(32)])[1] == rule(2986, 4096, 32)      # order 32: no tail
    assert wide(4096, 4096, [PSD, RPOS], [tri(32), 4096 - tri(32)])[0] == 0


@pytest.mark.parametrize("n,m,seg_type,seg_len", [(3, 6, [PSD], [3]), (3, 6, [PSD, PSD], [6, 1]), (3, 6, [7], [6]), (3, 6, [PSD], [-6]),
                                                  (0, 6, [PSD], [6]), (3, 0, [], [])])
def test_other_refusals(n, m, seg_type, seg_len):
    assert wide(n, m, seg_type, seg_len)[0] == _lib.E_INVALID


def test_mid_and_sdp_rules_answer_what_they_answered():
    """thip_midbatch_fits and thip_sdpbatch_fits on this file's shapes and a grid: their own restated rule, untouched"""
    shapes = [(n, m, st, sl, k) for m, n, st, sl, k in ACCEPTED] + [(n, m, st, sl, 0) for n, m, st, sl, _ in REFUSED[:2]]
    for m in (1, 160, 520, 1000, 2000, 2019, 2020, 2520, 2521, 4096):
        for n in (1, 80, 1000, 1001, 4095, 4096):
            shapes.append((n, m, [RPOS], [m], 0))
    for k in (9, 32, 33, 48, 57, 58, 64):
        for n in (1, 46, 47, 836, 837):
            shapes.append((n, tri(k) + 3, [RPOS, PSD], [3, tri(k)], k))
    for n, m, st, sl, k in shapes:
        ok = 1 <= m <= 4096 and 1 <= n <= 4096 and old_rule(n, m, k) <= LDS
        rc, lds, thr, _ = _fits_rc("sdpbatch", n, m, st, sl)
        assert (rc == 0) == ok, ("sdp", n, m, k)
        if ok:
            assert lds == old_rule(n, m, k) and thr == (256 if n * m <= 8192 else 1024)
        if k == 0:
            rc, lds, _, _ = _fits_rc("midbatch", n, m, st, sl)
            assert (rc == 0) == ok and (not ok or lds == old_rule(n, m, 0)), ("mid", n, m)
        else:
            assert _fits_rc("midbatch", n, m, st, sl)[0] == _lib.E_INVALID


def _dense(n, m, seg_type, seg_len):
    return _Dense(n, m, np.zeros(m * n, np.float32), np.zeros(m, np.float32), np.zeros(n, np.float32), list(seg_type), list(seg_len))


def test_no_chooser_returns_the_wide_batch():
    """own_a_batch, conic_batch and ragged_batch still refuse what they refused (the refusals come before any device call)"""
    import totsu_amd as T
    d = _dense(1000, 2020, [RPOS], [2020])
    for choose in (T.own_a_batch, T.conic_batch, T.ragged_batch):
        with pytest.raises(ValueError):
            choose([d])
    with pytest.raises(ValueError):
        MB.choose(1000, 2020, [RPOS], [2020])
    assert T.WideBatchSolver._prefix == "thip_widebatch_" and issubclass(T.WideBatchSolver, T.SdpBatchSolver)


def test_python_side_refusals_need_no_device():
    import totsu_amd as T
    z = lambda *s: np.zeros(s, np.float32)
    S = T.WideBatchSolver
    bad = [lambda: S(2, 4097, z(1, 2 * 4097), z(1, 4097), z(1, 2), [1], [4097]),
           lambda: S(4097, 2, z(1, 2 * 4097), z(1, 2), z(1, 4097), [1], [2]),
           lambda: S(3, 7, z(1, 21), z(1, 7), z(1, 3), [PSD], [7]),
           lambda: S(3, 6, z(2, 18), z(2, 6), z(2, 3), [1], [5]),
           lambda: S(3, 6, z(0, 18), z(0, 6), z(0, 3), [1], [6]),
           lambda: S(3, 6, z(2, 17), z(2, 6), z(2, 3), [1], [6]),
           lambda: S(3, 6, z(2, 18), z(2, 6), z(3, 3), [1], [6])]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    with pytest.raises(ValueError):
        S.from_dense([])
    with pytest.raises(ValueError):
        S.from_dense([_dense(3, 6, [1], [6]), _dense(3, 7, [1], [7])])


def test_info_record_extends_the_sdp_batch_record():
    names = [f for f, _ in _lib.WideBatchInfo._fields_]
    assert names[:len(_lib.SdpBatchInfo._fields_)] == [f for f, _ in _lib.SdpBatchInfo._fields_]
    assert names[-2:] == ["lds_bytes_per_problem", "arena_bytes_per_problem"]
    assert C.sizeof(_lib.WideBatchInfo) == C.sizeof(_lib.SdpBatchInfo) + 16
