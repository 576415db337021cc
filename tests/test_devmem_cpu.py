"""CPU: what the round calls on device memory need of the host (totsu_amd/devmem.py, the hooks of totsu_amd/csrc/thip_ownbatch.h that
need no device): as_device on hand-built __cuda_array_interface__ objects and its refusals, the offset tables of the packed arrays
against a numpy restatement, the overlap predicate, the 24 symbols, and DeviceBuffer.__cuda_array_interface__ on a stub pointer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("smallbatch", "midbatch", "sdpbatch", "raggedbatch", "sparsebatch", "raggedsparse")
CALLS = {"set_bc_dev": 8, "set_a_dev": 5, "set_iterates_dev": 5, "solutions_dev": 6}
HOOKS = {"thip_test_ownbatch_addresses": 3, "thip_test_ownbatch_last_transfer": 3, "thip_test_ownbatch_overlap": 4,
         "thip_test_ownbatch_offsets": 4, "thip_test_ownbatch_copy_chunk": 0}


class Cai:
    """an object that speaks __cuda_array_interface__ and owns nothing"""

    def __init__(self, shape, typestr="<f4", ptr=0x7F0000001000, readonly=False, strides=None):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, readonly), "version": 2, "strides": strides}


def _stub_buffer(n, ptr):
    from totsu_amd import DeviceBuffer
    b = DeviceBuffer.__new__(DeviceBuffer)                        # (no allocation; the pointer is taken back before the object dies)
    b.n, b.ptr = n, ptr
    return b


# ---- as_device ----------------------------------------------------------------------------------------------------------------------

def test_as_device_accepts():
    from totsu_amd.devmem import as_device
    assert as_device(Cai((12,)), "v") == (0x7F0000001000, 12)
    assert as_device(Cai((3, 4)), "v") == (0x7F0000001000, 12)                                  # packed rows
    assert as_device(Cai((3, 4), strides=(16, 4)), "v") == (0x7F0000001000, 12)                 # .. said out loud
    assert as_device(Cai((1, 4), strides=(999, 4)), "v")[1] == 4                                # an axis of one may say anything
    assert as_device(Cai((5,), readonly=True), "v")[1] == 5                                     # an input may be read-only
    assert as_device(Cai((5,), typestr="<i4"), "state", out=True, typestr="<i4")[1] == 5
    assert as_device(Cai((0,), ptr=0), "v") == (0, 0)
    b = _stub_buffer(7, 0x1000)
    try:
        assert as_device(b, "v") == (0x1000, 7) and as_device(b, "s", out=True, typestr="<i4") == (0x1000, 7)
    finally:
        b.ptr = None


def test_as_device_refuses():
    import torch
    from totsu_amd.devmem import as_device
    for obj, out, match in ((Cai((4,), typestr="<f8"), False, r"vals: dtype '<f8' where float32"),
                            (Cai((4,), typestr="<i4"), False, r"vals: dtype"),
                            (Cai((4,)), False, None),
                            (Cai((3, 4), strides=(32, 4)), False, r"vals: the array is not contiguous"),
                            (Cai((3, 4), strides=(4, 12)), False, r"vals: the array is not contiguous"),
                            (Cai((4,), strides=(8,)), False, r"vals: the array is not contiguous"),
                            (Cai((4,), readonly=True), True, r"vals: a read-only array where an output"),
                            (Cai((4,), ptr=0), False, r"vals: a null address"),
                            (np.zeros(4, np.float32), False, r"vals: an array on the host"),
                            (torch.zeros(4), False, r"vals: a tensor on the host"),
                            ([1.0, 2.0], False, r"vals: a DeviceBuffer, a torch tensor on the GPU or"),
                            (None, False, r"vals: ")):
        if match is None:
            assert as_device(obj, "vals", out=out)[1] == 4
            continue
        with pytest.raises(ValueError, match=match):
            as_device(obj, "vals", out=out)
    freed = _stub_buffer(3, None)
    with pytest.raises(ValueError, match="vals: the DeviceBuffer has been freed"):
        as_device(freed, "vals")


def test_device_buffer_speaks_the_interface():
    b = _stub_buffer(5, 0x2000)
    try:
        cai = b.__cuda_array_interface__
        assert cai["shape"] == (5,) and cai["typestr"] == "<f4" and cai["data"] == (0x2000, False)
        assert cai["version"] in (2, 3) and cai.get("strides") is None
        assert set(cai) >= {"shape", "typestr", "data", "version"}
        from totsu_amd.devmem import as_device
        assert as_device(Cai(cai["shape"], cai["typestr"], *cai["data"]), "v") == (0x2000, 5)
        b.ptr = None
        with pytest.raises(AttributeError):
            b.__cuda_array_interface__
    finally:
        b.ptr = None


# ---- the offset tables --------------------------------------------------------------------------------------------------------------

def _offsets(shapes):
    from totsu_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        pytest.skip("the library is not built")
    lib = _lib.load()
    cnt = len(shapes)
    n = (C.c_size_t * max(cnt, 1))(*[s[0] for s in shapes])
    m = (C.c_size_t * max(cnt, 1))(*[s[1] for s in shapes])
    out = np.zeros((5, cnt + 1), dtype=np.int64)
    assert lib.thip_test_ownbatch_offsets(cnt, n, m, out.ctypes.data_as(C.POINTER(C.c_int64))) == 0
    return out


def _restated(shapes):
    n, m = np.array([s[0] for s in shapes], np.int64), np.array([s[1] for s in shapes], np.int64)
    lens = [n, m, n + 2 * m + 1, n + m + 1, m * n]
    return np.stack([np.concatenate([[0], np.cumsum(v)]) for v in lens])


def test_offset_tables_of_the_ragged_set():
    from setbc_cases import Fam

    class Stub:
        SmallBatchSolver = MidBatchSolver = SdpBatchSolver = RaggedBatchSolver = SparseBatchSolver = RaggedSparseBatchSolver = None
    from totsu_amd import devmem
    for name in ("ragged", "raggedsparse"):
        ds = Fam(Stub, name).sets[0][1]
        shapes = [(d.n, d.m) for d in ds]
        got = _offsets(shapes)
        assert np.array_equal(got, _restated(shapes)), name
        for q in range(5):                                       # and the Python side's one rule gives the same
            assert np.array_equal(got[q], devmem.offsets([devmem.part_lengths(*s)[q] for s in shapes])), (name, q)


def test_offset_tables_of_random_shapes():
    rng = np.random.default_rng(4242)
    for _ in range(300):
        cnt = int(rng.integers(1, 40))
        shapes = [(int(rng.integers(1, 4097)), int(rng.integers(1, 4097))) for _ in range(cnt)]
        assert np.array_equal(_offsets(shapes), _restated(shapes))
    assert np.array_equal(_offsets([]), np.zeros((5, 1), np.int64))


# ---- the overlap predicate ----------------------------------------------------------------------------------------------------------

def test_overlap_predicate():
    from totsu_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        pytest.skip("the library is not built")
    ov = _lib.load().thip_test_ownbatch_overlap
    a = 0x7F0000000000
    assert ov(a, 64, a + 128, 64) == 0 and ov(a + 128, 64, a, 64) == 0          # disjoint
    assert ov(a, 64, a + 64, 64) == 0 and ov(a + 64, 64, a, 64) == 0            # touching
    assert ov(a, 64, a + 63, 64) == 1 and ov(a + 63, 4, a, 64) == 1             # one byte shared
    assert ov(a, 256, a + 64, 16) == 1 and ov(a + 64, 16, a, 256) == 1          # nested
    assert ov(a, 64, a, 64) == 1                                                # the exact in-place range
    assert ov(a, 0, a, 64) == 0 and ov(a, 64, a + 8, 0) == 0                    # an empty range shares nothing
    assert ov(2 ** 64 - 64, 64, 0, 64) == 0                                     # the last bytes of the address space


# ---- the symbols --------------------------------------------------------------------------------------------------------------------

def _declared(header):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(thip_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S))


def _arity(args):
    args = args.strip()
    return 0 if args in ("void", "") else args.count(",") + 1


def test_the_headers_declare_the_24_symbols():
    api, hooks = _declared("totsu_f32hip.h"), _declared("totsu_f32hip_test.h")
    for n in NAMES:
        for call, arity in CALLS.items():
            name = "thip_%s_%s" % (n, call)
            assert name in api and _arity(api[name]) == arity, name
    for name, arity in HOOKS.items():
        assert name in hooks and name not in api and _arity(hooks[name]) == arity, name


def test_the_library_and_the_binding_have_the_24_symbols():
    from totsu_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        pytest.skip("the library is not built")
    lib = _lib.load()
    names = ["thip_%s_%s" % (n, call) for n in NAMES for call in CALLS]
    assert len(names) == 24
    for name in names + list(HOOKS):
        assert name in _lib.PROTOTYPES, name
        assert getattr(lib, name) is not None, name
        want = CALLS.get(name.split("_", 2)[2], HOOKS.get(name))
        assert len(_lib.PROTOTYPES[name][1]) == want, name
    from totsu_amd.ownbatch import OwnBatchSolver
    for method in ("set_bc_dev", "set_a_dev", "set_iterates_dev", "solutions_dev"):
        assert callable(getattr(OwnBatchSolver, method))
