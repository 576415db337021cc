"""CPU: the shape rules of the SDP batch (thip_sdpbatch_fits needs no device), the Python-side checks of SdpBatchSolver and the
choice conic_batch makes between the small, the mid and the SDP batch."""
import ctypes as C

import numpy as np
import pytest

from totsu_amd import _lib
from totsu_amd import midbatch as MB
from totsu_amd import sdpbatch as SP
from totsu_amd import smallbatch as SB
from totsu_amd.problem import _Dense

RPOS, PSD, ZERO = _lib.CONE_RPOS, _lib.CONE_PSD, _lib.CONE_ZERO
LDS = 163840
FIXED = 64 + 4096 + 2048          # floats of LDS beside the vectors: the block sums, the row-sum and the column-sum scratch
TAIL = 3 * 64 * 65 * 4            # bytes of the three operands that do not overlay the pass scratch (orders above 32)


def tri(k):
    return k * (k + 1) // 2


def rule(n, m, max_k):
    """DESIGN.md 4.2, restated: the mid batch's map, and 49 920 bytes when the largest PSD order exceeds 32"""
    return 4 * (FIXED + 8 * n + 13 * m) + ((m + 3) & ~3) + (TAIL if max_k > 32 else 0)


def _fits_rc(n, m, seg_type, seg_len):
    """the raw return code, lds_bytes, threads, message"""
    lib = _lib.load()
    st = np.ascontiguousarray(seg_type, dtype=np.int32)
    sl = np.ascontiguousarray(seg_len, dtype=np.int64)
    lds, thr = C.c_size_t(0), C.c_int(0)
    rc = lib.thip_sdpbatch_fits(n, m, st.size, st.ctypes.data_as(C.POINTER(C.c_int32)), sl.ctypes.data_as(C.POINTER(C.c_int64)),
                                C.byref(lds), C.byref(thr))
    return rc, lds.value, thr.value, (lib.thip_last_error() or b"").decode() if rc else ""


# the layouts the family exists for: (m, n, seg_type, seg_len, largest order)
REQUIRED = [(45, 6, [PSD], [45], 9),
            (300, 6, [PSD], [300], 24),
            (588, 64, [PSD, PSD, RPOS], [21, 561, 6], 33),               # family F5 of tests/tau_zero_problems.py
            (560, 528, [PSD, ZERO], [528, 32], 32),                      # the 4 x 8 partitioning_sdp
            (1176, 48, [PSD], [1176], 48)]


def test_rule_restated():
    """lds_bytes is the restated rule over a sweep of (n, k), one cone of order k and 5 nonnegative rows"""
    for k in range(1, 65):
        for n in (1, 6, 48, 200, 836, 837, 2000, 4096):
            m = tri(k) + 5
            rc, lds, thr, _ = _fits_rc(n, m, [RPOS, PSD], [5, tri(k)])
            want = rule(n, m, k)
            assert (rc == 0) == (want <= LDS), (n, k, rc, want)
            if rc == 0:
                assert lds == want, (n, k, lds, want)
                assert thr == (256 if n * m <= 8192 else 1024)
    # several cones: the largest order decides
    assert _fits_rc(5, tri(3) + tri(33) + tri(6), [PSD] * 3, [tri(3), tri(33), tri(6)])[1] == rule(5, tri(3) + tri(33) + tri(6), 33)
    assert _fits_rc(5, tri(3) + tri(32) + tri(6), [PSD] * 3, [tri(3), tri(32), tri(6)])[1] == rule(5, tri(3) + tri(32) + tri(6), 32)


@pytest.mark.parametrize("m,n,seg_type,seg_len,max_k", REQUIRED)
def test_required_layouts_are_accepted(m, n, seg_type, seg_len, max_k):
    rc, lds, thr, _ = _fits_rc(n, m, seg_type, seg_len)
    assert rc == 0 and lds == rule(n, m, max_k) <= LDS
    assert SP.fits(n, m, seg_type, seg_len) == (lds, thr)


def test_largest_order_and_no_psd():
    """what the one rule leaves between order 48 and the kernel's cap of 64: 53 m + 32 n <= 89 088 takes orders up to 57"""
    assert _fits_rc(46, tri(57), [PSD], [tri(57)])[0] == 0                      # order 57: 1653 rows, n <= 46
    assert _fits_rc(47, tri(57), [PSD], [tri(57)])[0] == _lib.E_INVALID
    for k in range(58, 65):                                                     # a legal order whose vectors alone are too many
        rc, _, _, msg = _fits_rc(1, tri(k), [PSD], [tri(k)])
        assert rc == _lib.E_INVALID and "LDS" in msg, (k, msg)
    # without a PSD segment the map is the mid batch's
    for n, m, st, sl in ((260, 520, [RPOS], [520]), (60, 400, [2, 2, 2, 2, 3, 0], [200, 130, 2, 1, 60, 7]), (1000, 2019, [RPOS], [2019])):
        assert SP.fits(n, m, st, sl) == MB.fits(n, m, st, sl)


@pytest.mark.parametrize("n,m,seg_type,seg_len,word", [
    (3, 2, [PSD], [2], "triangular"),                    # PSD lengths that are no k (k + 1) / 2
    (3, 4, [PSD], [4], "triangular"),
    (3, 7, [PSD], [7], "triangular"),
    (3, 9, [RPOS, PSD], [2, 7], "triangular"),
    (3, 4, [RPOS, PSD], [4, 0], "triangular"),           # k >= 1
    (3, 2145, [PSD], [2145], "above 64"),                # order 65
    (8, 4097, [RPOS], [4097], "4096"),                   # m beyond 4096
    (4097, 8, [RPOS], [8], "4096"),                      # n beyond 4096
    (3, 6, [PSD], [3], "cover"),                         # segments that sum to less than m
    (3, 6, [PSD, PSD], [6, 1], "cover"),                 # ... to more
    (3, 6, [7], [6], "bad cone segment"),                # no such cone
    (3, 6, [PSD], [-6], "bad cone segment"),
    (0, 6, [PSD], [6], "4096"),
])
def test_fits_refuses(n, m, seg_type, seg_len, word):
    rc, _, _, msg = _fits_rc(n, m, seg_type, seg_len)
    assert rc == _lib.E_INVALID and word in msg, msg
    with pytest.raises(ValueError):
        SP.fits(n, m, seg_type, seg_len)


def test_each_refusal_has_its_own_message():
    msgs = [_fits_rc(3, 7, [PSD], [7])[3], _fits_rc(3, 2145, [PSD], [2145])[3], _fits_rc(837, 1176, [PSD], [1176])[3]]
    assert all(msgs) and len(set(msgs)) == 3, msgs


def test_lds_limit_is_exact_at_order_48():
    """one cone of order 48 (1176 rows): 4 (6208 + 8 n + 15 288) + 1176 + 49 920 <= 163 840 holds up to n = 836"""
    assert rule(836, 1176, 48) <= LDS < rule(837, 1176, 48)
    rc, lds, _, _ = _fits_rc(836, 1176, [PSD], [1176])
    assert rc == 0 and lds == rule(836, 1176, 48) == 163832
    rc, _, _, msg = _fits_rc(837, 1176, [PSD], [1176])
    assert rc == _lib.E_INVALID and "LDS" in msg


def test_thread_choice_is_the_mid_batch_s():
    for m, n, st, sl, _ in REQUIRED:
        assert SP.fits(n, m, st, sl)[1] == MB.fits(n, m, [RPOS], [m])[1] == (256 if n * m <= 8192 else 1024)
    assert SP.fits(6, tri(52), [PSD], [tri(52)])[1] == 1024 and SP.fits(5, tri(52), [PSD], [tri(52)])[1] == 256      # 8268 > 8192 >= 6890
    assert SP.fits(6, 45, [PSD], [45])[1] == 256 and SP.fits(48, 1176, [PSD], [1176])[1] == 1024


def _dense(n, m, seg_type, seg_len, seed=0):
    rng = np.random.default_rng(seed)
    f = np.float32
    return _Dense(n, m, rng.standard_normal(m * n).astype(f), rng.standard_normal(m).astype(f), rng.standard_normal(n).astype(f),
                  seg_type, seg_len, None)


class _Chosen(Exception):
    pass


def test_conic_batch_choice(monkeypatch):
    """small, mid, SDP in that order, by the three rules alone (from_dense is caught before it needs a device)"""
    def spy(cls, denses, param=None, **kw):
        raise _Chosen(cls.__name__)
    monkeypatch.setattr(SB.SmallBatchSolver, "from_dense", classmethod(spy))
    for d, want in ((_dense(20, 40, [RPOS], [40]), "SmallBatchSolver"), (_dense(157, 157, [RPOS], [157]), "MidBatchSolver"),
                    (_dense(6, 45, [PSD], [45]), "SdpBatchSolver"), (_dense(64, 588, [PSD, PSD, RPOS], [21, 561, 6]), "SdpBatchSolver")):
        with pytest.raises(_Chosen, match="^%s$" % want):
            SP.conic_batch([d, d])
    with pytest.raises(ValueError, match="FusedSolver"):
        SP.conic_batch([_dense(8, 4097, [RPOS], [4097])])
    with pytest.raises(ValueError, match="FusedSolver"):
        SP.conic_batch([_dense(3, 2145, [PSD], [2145])])
    with pytest.raises(ValueError):
        SP.conic_batch([])
    with pytest.raises(ValueError):                                   # another layout
        SP.conic_batch([_dense(6, 45, [PSD], [45]), _dense(6, 45, [RPOS], [45])])
    import totsu_amd
    assert totsu_amd.conic_batch is SP.conic_batch and totsu_amd.SdpBatchSolver is SP.SdpBatchSolver
    assert issubclass(SP.SdpBatchSolver, MB.MidBatchSolver)


def test_constructor_refusals_come_before_the_device():
    """every refusal of the shape, the layout and the array lengths is raised before thip_init is needed"""
    S = SP.SdpBatchSolver
    f = np.float32
    z = lambda *s: np.zeros(s, f)
    with pytest.raises(ValueError):
        S(3, 7, z(2, 21), z(2, 7), z(2, 3), [PSD], [7])
    with pytest.raises(ValueError):
        S(3, 2145, z(1, 3 * 2145), z(1, 2145), z(1, 3), [PSD], [2145])
    with pytest.raises(ValueError):
        S(2, 4097, z(1, 2 * 4097), z(1, 4097), z(1, 2), [RPOS], [4097])
    with pytest.raises(ValueError):
        S(4097, 2, z(1, 2 * 4097), z(1, 2), z(1, 4097), [RPOS], [2])
    with pytest.raises(ValueError):                                   # the map exceeds LDS
        S(837, 1176, z(1, 1), z(1, 1176), z(1, 837), [PSD], [1176])
    with pytest.raises(ValueError):
        S(3, 6, z(2, 18), z(2, 6), z(2, 3), [PSD], [3])
    with pytest.raises(ValueError):                                   # P = 0
        S(3, 6, z(0, 18), z(0, 6), z(0, 3), [PSD], [6])
    with pytest.raises(ValueError):                                   # arrays of the wrong length
        S(3, 6, z(2, 17), z(2, 6), z(2, 3), [PSD], [6])
    with pytest.raises(ValueError):
        S(3, 6, z(2, 18), z(2, 6), z(3, 3), [PSD], [6])
    with pytest.raises(ValueError):
        S(3, 6, z(2, 18), z(2, 6), z(2, 3), [PSD], [6], vecs_b_rowabs=z(1, 6))


def test_the_old_chooser_is_unchanged():
    with pytest.raises(ValueError, match="FusedSolver"):             # own_a_batch and choose still know two batches and no PSD
        MB.own_a_batch([_dense(6, 45, [PSD], [45])])
    with pytest.raises(ValueError, match="FusedSolver"):
        MB.choose(6, 45, [PSD], [45])
    for fits in (SB.fits, MB.fits):
        with pytest.raises(ValueError, match="takes no PSD segment"):
            fits(6, 45, [PSD], [45])
