"""`Mid16BatchSolver`: the mid batch (`MidBatchSolver`: many mid-size conic programs of one shape and cone layout, each with its OWN
dense A streamed by one workgroup per problem) over a LIBRARY-OWNED 16-BIT COPY of every problem's A (thip_mid16batch_* in
include/totsu_f32hip.h): half the bytes of A per pass, half the memory, and one load path for every m (the store pads the leading
dimension).  The shapes, the cones, the methods and the ValueErrors are `MidBatchSolver`'s.

a_dtype, fixed at construction: "bf16" -- the f32 rounded to nearest even to its upper 16 bits -- or "f16" -- one power-of-two scale
per column, inv_s[c] = 2^(e - 14) with e the exponent frexp gives the column's largest |a| (1 for a column of zeros), and the word
f16(a / inv_s[c]).  The problem solved is the one with the ROUNDED matrix W (`widened(i)`): W(r, c) the bf16 word shifted left 16
bits, or float32(h(r, c)) * inv_s[c].  The batch is bit for bit a `MidBatchSolver` over W.  Its end iterate (`raw_iterate`) is a
start (`set_iterates`) for a `MidBatchSolver` over the exact matrix -- the batch form of the single solver's mixed route.

The f32 matrices are converted on the device at construction, by `replace`, `set_a` and `set_a_dev(values)`, and are not kept:
`set_a_dev(None)`, the in-place form, is refused.  No chooser returns this class: rounding the caller's matrix is never an automatic
choice."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .fused import A_STORAGE, DeviceBuffer
from .midbatch import MidBatchSolver


def fits(n, m, seg_type, seg_len):
    """the shape rules alone (thip_mid16batch_fits, which is the mid batch's; needs no GPU): (lds_bytes, threads), or ValueError"""
    from .ownbatch import _fits
    return _fits("thip_mid16batch_", n, m, seg_type, seg_len)


def _kind(a_dtype):
    if a_dtype == "f32":
        raise ValueError('a Mid16BatchSolver stores A in 16 bits (a_dtype "bf16" or "f16"): f32 A is MidBatchSolver')
    if a_dtype not in ("bf16", "f16"):
        raise ValueError('a_dtype is "bf16" or "f16", not %r' % (a_dtype,))
    return A_STORAGE[a_dtype]


def store_bytes(n, m, a_dtype="f16"):
    """the bytes of one problem's block of the store (thip_mid16batch_store_bytes; needs no GPU)"""
    out = C.c_size_t()
    lib.thip_mid16batch_store_bytes(int(n), int(m), _kind(a_dtype), C.byref(out))
    return out.value


class Mid16BatchSolver(MidBatchSolver):
    """OwnBatchSolver on thip_mid16batch_*.  info() reports a_dtype ("bf16" / "f16"), load_bytes (8), a_bytes_per_iter (bytes of the
    store read per problem-iteration) and a_store_bytes."""
    _prefix, _force_hook, _what, _Info = "thip_mid16batch_", "thip_test_mid16batch_force_threads", "mid16", _lib.Mid16BatchInfo

    def __init__(self, n, m, mats_a, vecs_b, vecs_c, seg_type, seg_len, param=None, a_dtype="f16", **kw):
        self.h = None
        self.a_dtype, self._a_kind = a_dtype, _kind(a_dtype)
        super().__init__(n, m, mats_a, vecs_b, vecs_c, seg_type, seg_len, param, **kw)

    @classmethod
    def from_dense(cls, denses, param=None, a_dtype="f16", **kw):
        return super().from_dense(denses, param, a_dtype=a_dtype, **kw)

    def _create(self, *args):
        lib.thip_mid16batch_create_kind(*args[:-1], self._a_kind, args[-1])
        # the library holds its own copy: the upload of the f32 stack goes (a DeviceBuffer of the caller's stays the caller's)
        if self.mats_a in self._owned:
            self._owned.remove(self.mats_a)
            self.mats_a.free()
        self.mats_a = None

    def replace(self, i, mat_a, vec_b, vec_c, vec_b_rowabs=None, start=None):
        """OwnBatchSolver.replace; the f32 mat_a is converted into the slot's block, and an upload of it is freed at once"""
        if mat_a is None or isinstance(mat_a, DeviceBuffer):
            return super().replace(i, mat_a, vec_b, vec_c, vec_b_rowabs, start)
        if np.asarray(mat_a).size != self.m * self.n:
            raise ValueError("mat_a: %d entries where %d are needed" % (np.asarray(mat_a).size, self.m * self.n))
        da = DeviceBuffer.from_host(mat_a)
        try:
            super().replace(i, da, vec_b, vec_c, vec_b_rowabs, start)
        finally:
            lib.thip_sync()
            da.free()

    def set_a_dev(self, values=None, first=0, count=None, keep_iterate=False):
        """OwnBatchSolver.set_a_dev with `values` (m n f32 per problem, converted from where they lie); values=None is refused:
        the batch keeps no f32 A that could have been rewritten in place"""
        if values is None:
            raise ValueError("set_a_dev: a Mid16BatchSolver holds a 16-bit copy of every A and no f32 A lies in place to be read again: "
                             "hand the values in")
        return super().set_a_dev(values, first, count, keep_iterate)

    def info(self):
        o = super().info()
        o["a_dtype"] = {v: k for k, v in A_STORAGE.items()}[o["a_dtype"]]
        return o

    def stored_a(self, i):
        """problem i's block as it lies in the store: (words, inv_scale) -- words (n, ld16) uint16, one row per COLUMN of A, ld16 =
        roundup4(m), the pad rows included; inv_scale (n,) float32, or None for bf16"""
        if not 0 <= int(i) < self.n_prob:
            raise ValueError("stored_a: no problem %r in a batch of %d" % (i, self.n_prob))
        ld16 = (self.m + 3) & ~3
        words = np.empty((self.n, ld16), dtype=np.uint16)
        inv = np.empty(self.n, dtype=np.float32) if self.a_dtype == "f16" else None
        lib.thip_mid16batch_stored(self.h, int(i), words.ctypes.data, None if inv is None else inv.ctypes.data)
        return words, inv

    def widened(self, i):
        """the matrix problem i is solved with, W, as float32 (m n, column-major -- what mat_a is), built on the host from stored_a(i)"""
        words, inv = self.stored_a(i)
        words = words[:, :self.m]
        if inv is None:
            w = (words.astype(np.uint32) << 16).view(np.float32)
        else:
            w = words.view(np.float16).astype(np.float32) * inv[:, None]
        return np.ascontiguousarray(w, dtype=np.float32).ravel()
