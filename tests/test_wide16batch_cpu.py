"""CPU: what the wide batch over a 16-bit A decides without a device -- its shape rule (the wide batch's, unchanged, PSD cones
included), the size of a problem's block of the store (the mid16 batch's), the refusals of a stored form and of a shape through the
library, the new symbols and the info record, the one mixin both 16-bit classes share, and that no chooser returns the class."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mid16_cases as M
from totsu_amd import _lib
from totsu_amd import mid16batch as MM
from totsu_amd import wide16batch as WW
from totsu_amd import widebatch as WB
from totsu_amd.problem import _Dense

ZERO, RPOS, SOC, ROTSOC, PSD = _lib.CONE_ZERO, _lib.CONE_RPOS, _lib.CONE_SOC, _lib.CONE_ROTSOC, _lib.CONE_PSD
F = np.float32
LDS = 163840
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tri(k):
    return k * (k + 1) // 2


def _fits_rc(name, n, m, seg_type, seg_len):
    """the raw return code, lds_bytes, threads, message of thip_<name>_fits"""
    lib = _lib.load()
    st = np.ascontiguousarray(seg_type, dtype=np.int32)
    sl = np.ascontiguousarray(seg_len, dtype=np.int64)
    lds, thr = C.c_size_t(0), C.c_int(0)
    rc = getattr(lib, "thip_%s_fits" % name)(n, m, st.size, st.ctypes.data_as(C.POINTER(C.c_int32)),
                                             sl.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(lds), C.byref(thr))
    return rc, lds.value, thr.value, (lib.thip_last_error() or b"").decode() if rc else ""


# the named shapes of tests/test_widebatch_cpu.py: (n, m, seg_type, seg_len), accepted and refused
NAMED = [(1000, 2020, [RPOS], [2020]), (1, 2521, [RPOS], [2521]), (4096, 2, [RPOS], [2]), (4096, 4096, [RPOS], [4096]),
         (4096, tri(64), [PSD], [tri(64)]), (837, tri(48), [PSD], [tri(48)]),
         (8, 4097, [RPOS], [4097]), (4097, 8, [RPOS], [8]), (2987, 4096, [PSD, RPOS], [tri(33), 4096 - tri(33)]),
         (2986, 4096, [PSD, RPOS], [tri(33), 4096 - tri(33)]), (3, 7, [PSD], [7]), (3, tri(65), [PSD], [tri(65)]),
         (3, 6, [PSD], [3]), (3, 6, [PSD, PSD], [6, 1]), (3, 6, [7], [6]), (3, 6, [PSD], [-6]), (0, 6, [PSD], [6]), (3, 0, [], []),
         (7, 21 + tri(40), [ZERO, RPOS, SOC, ROTSOC, PSD], [3, 4, 9, 5, tri(40)]),
         (5, tri(3) + tri(33) + tri(6), [PSD] * 3, [tri(3), tri(33), tri(6)])]
REFUSED = [(8, 4097, [RPOS], [4097], "m <= 4096"), (4097, 8, [RPOS], [8], "n <= 4096"),
           (2987, 4096, [PSD, RPOS], [tri(33), 4096 - tri(33)], "do not fit the LDS"), (3, 7, [PSD], [7], "triangular"),
           (3, tri(65), [PSD], [tri(65)], "above 64")]


def test_fits_is_the_wide_batch_rule():
    """return code, LDS bytes, threads and the words of a refusal: thip_widebatch_fits', on every named shape and on 200 random
    draws with one PSD cone of a random order in front of nonnegative rows"""
    rng = np.random.default_rng(16)
    shapes = list(NAMED)
    for _ in range(200):
        k = int(rng.integers(0, 70))
        m = int(rng.integers(max(tri(k), 1), 4200))
        n = int(rng.integers(1, 4200))
        if k == 0:
            shapes.append((n, m, [RPOS], [m]))
        else:
            shapes.append((n, m, [PSD, RPOS], [tri(k), m - tri(k)]))
    taken = 0
    for n, m, st, sl in shapes:
        want = _fits_rc("widebatch", n, m, st, sl)
        got = _fits_rc("wide16batch", n, m, st, sl)
        assert got == want, (n, m, st, sl, got, want)
        taken += got[0] == 0
        if got[0] == 0:
            assert WW.fits(n, m, st, sl) == WB.fits(n, m, st, sl) == got[1:3]
        else:
            with pytest.raises(ValueError):
                WW.fits(n, m, st, sl)
    assert 20 < taken < len(shapes) - 20
    assert _fits_rc("wide16batch", 4096, 4096, [RPOS], [4096])[1] == 127232


@pytest.mark.parametrize("n,m,seg_type,seg_len,word", REFUSED)
def test_shape_refusals_are_in_the_rule_s_words(n, m, seg_type, seg_len, word):
    rc, _, _, msg = _fits_rc("wide16batch", n, m, seg_type, seg_len)
    assert rc == _lib.E_INVALID and word in msg, msg
    with pytest.raises(ValueError, match=word):
        WW.fits(n, m, seg_type, seg_len)
    import totsu_amd as T
    z = lambda *s: np.zeros(s, F)
    with pytest.raises(ValueError, match=word):                    # before anything is uploaded: no device is needed
        T.Wide16BatchSolver(n, m, z(1, 1), z(1, m), z(1, n), seg_type, seg_len)


def test_store_bytes_is_the_mid16_formula():
    rng = np.random.default_rng(5)
    shapes = [(1, 1), (1, 4096), (4096, 1), (4096, 4096), (1000, 2020), (5, 66), (9, 67), (33, 65)]
    shapes += [(int(n), int(m)) for n, m in zip(rng.integers(1, 4097, 300), rng.integers(1, 4097, 300))]
    for n, m in shapes:
        for kind in M.KINDS:
            assert WW.store_bytes(n, m, kind) == M.store_bytes(n, m, kind) == MM.store_bytes(n, m, kind), (n, m, kind)
    assert WW.store_bytes(4096, 4096, "bf16") == 2 * 4096 * 4096 and WW.store_bytes(4096, 4096, "f16") == 2 * 4096 * 4096 + 4 * 4096


def test_stored_form_refusals_through_the_library():
    out = C.c_size_t()
    with pytest.raises(_lib.ThipError, match="thip_widebatch"):
        _lib.lib.thip_wide16batch_store_bytes(4, 4, 0, C.byref(out))
    for kind in (3, -1):
        with pytest.raises(_lib.ThipError, match="unknown stored form"):
            _lib.lib.thip_wide16batch_store_bytes(4, 4, kind, C.byref(out))
    with pytest.raises(ValueError, match="f32 A is WideBatchSolver"):
        WW.store_bytes(4, 4, "f32")
    with pytest.raises(ValueError, match="bf16"):
        WW.store_bytes(4, 4, "fp8")
    # create_kind refuses the stored form before it asks for a device
    par = _lib.Param(-1, 1e-6, 1e-6, 1e-12, 0, 0, 0)
    st, sl, h = np.array([1], np.int32), np.array([6], np.int64), C.c_void_p()
    for kind, word in ((0, "thip_widebatch"), (3, "unknown stored form")):
        with pytest.raises(_lib.ThipError, match=word) as e:
            _lib.lib.thip_wide16batch_create_kind(3, 6, 2, None, None, None, None, 1, st.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  sl.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(par), kind, C.byref(h))
        assert e.value.code == _lib.E_INVALID and not h.value


NAMES = ["fits", "store_bytes", "create", "create_kind", "set_param", "init", "run", "run_until_any", "status", "solution", "iterate",
         "precond", "replace", "set_iterates", "set_bc", "solutions", "set_a", "set_bc_dev", "set_a_dev", "set_iterates_dev",
         "solutions_dev", "stored", "info", "destroy"]


def test_symbols_in_the_headers_and_the_library():
    lib = C.CDLL(_lib.SO_PATH)
    hdr = open(os.path.join(ROOT, "include", "totsu_f32hip.h")).read()
    for name in NAMES:
        sym = "thip_wide16batch_" + name
        assert getattr(lib, sym) is not None
        assert re.search(r"\bint %s\(" % sym, hdr), sym
    assert getattr(lib, "thip_test_wide16batch_force_threads") is not None
    assert "thip_test_wide16batch_force_threads" in open(os.path.join(ROOT, "include", "totsu_f32hip_test.h")).read()


def test_info_record_is_the_wide_record_and_the_store_s_fields():
    names = [f for f, _ in _lib.Wide16BatchInfo._fields_]
    wide = [f for f, _ in _lib.WideBatchInfo._fields_]
    assert [f if f != "a_dtype" else "reserved" for f in names[:len(wide)]] == wide          # a_dtype takes the reserved word
    assert names[len(wide):] == ["a_store_bytes"] and set(f for f, _ in _lib.Mid16BatchInfo._fields_) <= set(names)
    assert C.sizeof(_lib.Wide16BatchInfo) == C.sizeof(_lib.WideBatchInfo) + 8
    for f, _ in _lib.WideBatchInfo._fields_:
        if f != "reserved":
            assert getattr(_lib.Wide16BatchInfo, f).offset == getattr(_lib.WideBatchInfo, f).offset, f


def test_the_class_is_exported_and_shares_one_mixin():
    import totsu_amd as T
    from totsu_amd.store16 import Store16
    S = WW.Wide16BatchSolver
    assert T.Wide16BatchSolver is S and "Wide16BatchSolver" in T.__all__
    assert issubclass(S, T.WideBatchSolver) and issubclass(S, Store16) and issubclass(T.Mid16BatchSolver, Store16)
    assert S._prefix == "thip_wide16batch_"
    for name in ("_create", "replace", "set_a_dev", "stored_a", "widened", "info"):      # one text, not two
        assert getattr(S, name) is getattr(T.Mid16BatchSolver, name) is getattr(Store16, name), name


def _dense(n, m, seg_type, seg_len):
    return _Dense(n, m, np.zeros(m * n, F), np.zeros(m, F), np.zeros(n, F), list(seg_type), list(seg_len))


def test_python_refusals_come_before_the_device():
    import totsu_amd as T
    S = T.Wide16BatchSolver
    z = lambda *s: np.zeros(s, F)
    with pytest.raises(ValueError, match="f32 A is WideBatchSolver"):
        S(3, 6, z(2, 18), z(2, 6), z(2, 3), [RPOS], [6], a_dtype="f32")
    with pytest.raises(ValueError, match="bf16"):
        S(3, 6, z(2, 18), z(2, 6), z(2, 3), [RPOS], [6], a_dtype="fp8")
    with pytest.raises(ValueError, match="MidBatchSolver"):         # and the mid16 batch still answers in its own words
        T.Mid16BatchSolver(3, 6, z(2, 18), z(2, 6), z(2, 3), [RPOS], [6], a_dtype="f32")
    for f in (lambda: S(3, 6, z(2, 18), z(2, 6), z(2, 3), [RPOS], [5]),
              lambda: S(3, 6, z(0, 18), z(0, 6), z(0, 3), [RPOS], [6]),
              lambda: S(3, 6, z(2, 17), z(2, 6), z(2, 3), [RPOS], [6]),
              lambda: S(3, 6, z(2, 18), z(2, 6), z(3, 3), [RPOS], [6]),
              lambda: S.from_dense([]),
              lambda: S.from_dense([_dense(3, 6, [1], [6]), _dense(3, 7, [1], [7])])):
        with pytest.raises(ValueError):
            f()


def test_no_chooser_returns_the_class():
    import totsu_amd as T
    from totsu_amd import midbatch as MB
    d = _dense(1000, 2020, [RPOS], [2020])
    for choose in (T.own_a_batch, T.conic_batch, T.ragged_batch):
        with pytest.raises(ValueError):
            choose([d])
    assert all(cls is not T.Wide16BatchSolver for cls, _ in MB.FAMILIES)
