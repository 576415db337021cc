"""CPU: what the mid batch over a 16-bit A decides without a device -- its shape rule (the mid batch's, unchanged), the size of a
problem's block of the store -- and the numpy restatements of the two roundings (tests/mid16_cases.py) that the GPU tests hold the
device to: bf16 against the bit formula on every upper-half pattern and every tie, f16 against numpy's float16, the scale rule
against frexp; the new symbols in the headers and the library; the Python-side refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mid16_cases as M
from totsu_amd import _lib
from totsu_amd import mid16batch as MM
from totsu_amd import midbatch as MB

F = np.float32
RPOS = [_lib.CONE_RPOS]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fits_rc(name, n, m, seg_type, seg_len):
    lib = _lib.load()
    st = np.ascontiguousarray(seg_type, dtype=np.int32)
    sl = np.ascontiguousarray(seg_len, dtype=np.int64)
    lds, thr = C.c_size_t(0), C.c_int(0)
    rc = getattr(lib, name)(n, m, st.size, st.ctypes.data_as(C.POINTER(C.c_int32)), sl.ctypes.data_as(C.POINTER(C.c_int64)),
                            C.byref(lds), C.byref(thr))
    return rc, lds.value, thr.value


BOUNDARY = [(1000, 2019), (1000, 2020), (1000, 2000), (4096, 100), (4096, 200), (1, 2520), (1, 3100), (8, 4097), (4097, 8), (0, 4),
            (4, 0), (1, 1), (260, 520), (128, 65), (40, 80)]


def test_fits_is_the_mid_batch_rule():
    """on the boundary shapes of tests/test_midbatch_cpu.py, and along the floor's edge"""
    shapes = BOUNDARY + [(min(4096, (32768 - 13 * m) // 8), m) for m in range(1, 2521, 37)]
    taken = 0
    for n, m in shapes:
        want = _fits_rc("thip_midbatch_fits", n, m, RPOS, [m])
        got = _fits_rc("thip_mid16batch_fits", n, m, RPOS, [m])
        assert got == want, (n, m, got, want)
        taken += got[0] == 0
    assert 0 < taken < len(shapes)
    assert MM.fits(1000, 2000, RPOS, [2000]) == MB.fits(1000, 2000, RPOS, [2000])      # 2000 x 1000 still fits
    for st, sl in (([1, 1], [1, 1]), ([7], [6]), (RPOS, [-6]), (RPOS, [5])):
        assert _fits_rc("thip_mid16batch_fits", 3, 6, st, sl)[0] == _lib.E_INVALID


def test_a_psd_segment_is_refused_in_the_family_s_words():
    with pytest.raises(ValueError, match="mid16 batch takes no PSD"):
        MM.fits(3, 6, [_lib.CONE_PSD], [6])
    with pytest.raises(ValueError, match="mid16 batch takes no PSD"):
        MM.fits(3, 8, [_lib.CONE_RPOS, _lib.CONE_PSD], [2, 6])


def test_store_bytes_is_the_formula():
    rng = np.random.default_rng(5)
    shapes = [(1, 1), (1, 4096), (4096, 1), (1000, 2000), (5, 66), (9, 67), (33, 65)]
    shapes += [(int(n), int(m)) for n, m in zip(rng.integers(1, 4097, 300), rng.integers(1, 4097, 300))]
    for n, m in shapes:
        ld = (m + 3) // 4 * 4
        for kind, scales in (("bf16", 0), ("f16", 4 * n)):
            want = (2 * ld * n + scales + 15) // 16 * 16
            assert MM.store_bytes(n, m, kind) == want == M.store_bytes(n, m, kind), (n, m, kind)
            assert want % 16 == 0 and want <= 2 * m * n + 6 * n + scales + 15
    out = C.c_size_t()
    for kind in (0, 3, -1):
        with pytest.raises(_lib.ThipError):
            _lib.lib.thip_mid16batch_store_bytes(4, 4, kind, C.byref(out))
    with pytest.raises(ValueError, match="MidBatchSolver"):
        MM.store_bytes(4, 4, "f32")


def _bf16_by_value(a):
    """round to nearest even to the upper 16 bits, from the VALUES: the two neighbours and the distance to each, in f64"""
    b = a.view(np.uint32)
    with np.errstate(invalid="ignore"):                                # (the nan patterns are masked out by the caller)
        lo = (b & 0xffff0000).view(F).astype(np.float64)
        hi = ((b & 0xffff0000) + 0x10000).view(F).astype(np.float64)
        v = a.astype(np.float64)
        up = (np.abs(hi - v) < np.abs(v - lo)) | ((np.abs(hi - v) == np.abs(v - lo)) & (((b >> 16) & 1) == 1))
    return np.where(up, (b >> 16) + 1, b >> 16).astype(np.uint16)


def test_bf16_restatement_against_the_bit_formula():
    """every pattern of the upper half with the lower half 0, 1, 0x7fff, 0x8000 (the tie), 0x8001, 0xffff"""
    hi = np.arange(65536, dtype=np.uint32) << 16
    for low in (0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff):
        b = hi | np.uint32(low)
        got = M.bf16_words(b.view(F))
        special = (b & 0x7f800000) == 0x7f800000
        b64 = b.astype(np.uint64)
        formula = np.where(special, (b64 >> 16) | np.uint64(0x40 if low else 0), (b64 + 0x7fff + ((b64 >> 16) & 1)) >> 16).astype(np.uint16)
        assert np.array_equal(got, formula), hex(low)
        fin = ~special & (((b + 0x10000) & 0x7f800000) != 0x7f800000)      # (a carry into the exponent of inf is the formula's alone)
        assert np.array_equal(got[fin], _bf16_by_value(b.view(F))[fin]), hex(low)
    # ties go to even in both directions
    t = np.array([0x3f808000, 0x3f818000, 0xbf808000, 0xbf818000], dtype=np.uint32).view(F)
    assert list(M.bf16_words(t)) == [0x3f80, 0x3f82, 0xbf80, 0xbf82]
    assert list(M.bf16_words(np.array([-0.0, 0.0], F))) == [0x8000, 0]


def test_f16_restatement_against_numpy_and_frexp():
    rng = np.random.default_rng(11)
    cols = (rng.standard_normal((64, 50)) * np.exp(rng.uniform(-60, 60, (64, 1)))).astype(F)
    cols[3] = 0.0
    cols[4, 0], cols[5, :] = 3e38, cols[5, :] * 0 + F(1e-30)
    inv = M.f16_inv_scale(cols)
    mx = np.abs(cols).max(axis=1)
    for c in range(64):
        if mx[c] == 0:
            assert inv[c] == 1.0
            continue
        f, e = np.frexp(mx[c])
        assert 0.5 <= f < 1 and inv[c] == np.ldexp(F(1), int(e) - 14)
        assert 2.0 ** 13 <= mx[c] / inv[c] < 2.0 ** 14                 # the largest entry lands in [2^13, 2^14): no f16 overflow
    words = M.f16_words(cols, inv)
    want = (cols.astype(np.float64) / inv.astype(np.float64)[:, None]).astype(np.float16)      # (the quotient is exact: a power of two)
    assert np.array_equal(words, want.view(np.uint16))
    assert np.isfinite(words.view(np.float16)).all()
    # subnormal words and their ties, as planted for the GPU test
    a = M.planted(65, 33).reshape(33, 65)
    w, s = M.stored(a.ravel(), 65, 33, "f16")
    sub = w[4, 1:8].view(np.float16).astype(np.float64) / 2.0 ** -24
    assert s[4] == F(2.0 ** -13) and list(sub) == [128.0, 2.0, 2.0, 2.0, -1.0, 0.0, 0.0]
    assert w.shape == (33, 68) and not w[:, 65:].any()
    # W: one f32 multiply of the widened word
    W = M.widen(w, s, 65).reshape(33, 65)
    assert np.array_equal(W, w[:, :65].view(np.float16).astype(F) * s[:, None]) and abs(W[2, 0] / 3e38 - 1) < 2.0 ** -10
    wb, sb_ = M.stored(a.ravel(), 65, 33, "bf16")
    assert sb_ is None and np.array_equal(M.widen(wb, None, 65).view(np.uint32), wb[:, :65].astype(np.uint32).ravel() << 16)


NAMES = ["fits", "store_bytes", "create", "create_kind", "set_param", "init", "run", "run_until_any", "status", "solution", "iterate",
         "precond", "replace", "set_iterates", "set_bc", "solutions", "set_a", "set_bc_dev", "set_a_dev", "set_iterates_dev",
         "solutions_dev", "stored", "info", "destroy"]


def test_symbols_in_the_headers_and_the_library():
    lib = C.CDLL(_lib.SO_PATH)
    hdr = open(os.path.join(ROOT, "include", "totsu_f32hip.h")).read()
    for name in NAMES:
        sym = "thip_mid16batch_" + name
        assert getattr(lib, sym) is not None
        assert re.search(r"\bint %s\(" % sym, hdr), sym
    assert getattr(lib, "thip_test_mid16batch_force_threads") is not None
    assert "thip_test_mid16batch_force_threads" in open(os.path.join(ROOT, "include", "totsu_f32hip_test.h")).read()
    assert "thip_mid16batch_info_t" in hdr and "a_store_bytes" in hdr
    assert C.sizeof(_lib.Mid16BatchInfo) == C.sizeof(_lib.MidBatchInfo) + 8


def test_python_refusals_come_before_the_device():
    import totsu_amd
    S = MM.Mid16BatchSolver
    assert totsu_amd.Mid16BatchSolver is S and issubclass(S, MB.MidBatchSolver)
    z = lambda *s: np.zeros(s, F)
    with pytest.raises(ValueError, match="MidBatchSolver"):
        S(3, 6, z(2, 18), z(2, 6), z(2, 3), RPOS, [6], a_dtype="f32")
    with pytest.raises(ValueError):
        S(3, 6, z(2, 18), z(2, 6), z(2, 3), RPOS, [6], a_dtype="fp8")
    with pytest.raises(ValueError, match="PSD"):
        S(3, 6, z(2, 18), z(2, 6), z(2, 3), [_lib.CONE_PSD], [6])
    with pytest.raises(ValueError):
        S(1000, 2020, z(1, 1), z(1, 2020), z(1, 1000), RPOS, [2020])
    with pytest.raises(ValueError):
        S(3, 6, z(2, 17), z(2, 6), z(2, 3), RPOS, [6])
    # no chooser knows the family
    assert all(cls is not S for cls, _ in MB.FAMILIES)
