"""What the own-A batch solvers over a LIBRARY-OWNED 16-BIT COPY of every problem's A add to their f32 family (`Mid16BatchSolver`
to `MidBatchSolver`, `Wide16BatchSolver` to `WideBatchSolver`): one mixin, `Store16`, placed in front of the f32 class.

a_dtype, fixed at construction: "bf16" -- the f32 rounded to nearest even to its upper 16 bits -- or "f16" -- one power-of-two scale
per column, inv_s[c] = 2^(e - 14) with e the exponent frexp gives the column's largest |a| (1 for a column of zeros), and the word
f16(a / inv_s[c]).  The problem solved is the one with the ROUNDED matrix W (`widened(i)`): W(r, c) the bf16 word shifted left 16
bits, or float32(h(r, c)) * inv_s[c].

The f32 matrices are converted on the device at construction, by `replace`, `set_a` and `set_a_dev(values)`, and are not kept:
`set_a_dev(None)`, the in-place form, is refused."""
import ctypes as C

import numpy as np

from ._lib import lib
from .fused import A_STORAGE, DeviceBuffer


def kind_of(a_dtype, name16, name32):
    """the library's word for a_dtype; ValueError for "f32" (that is the class name32) and for anything unknown"""
    if a_dtype == "f32":
        raise ValueError('a %s stores A in 16 bits (a_dtype "bf16" or "f16"): f32 A is %s' % (name16, name32))
    if a_dtype not in ("bf16", "f16"):
        raise ValueError('a_dtype is "bf16" or "f16", not %r' % (a_dtype,))
    return A_STORAGE[a_dtype]


def store_bytes_of(prefix, n, m, kind):
    """the bytes of one problem's block of the store (thip_NAME_store_bytes; needs no GPU)"""
    out = C.c_size_t()
    getattr(lib, prefix + "store_bytes")(int(n), int(m), kind, C.byref(out))
    return out.value


class Store16:
    """the additions: a_dtype, a create that carries it and frees the f32 upload, replace / set_a_dev on a store, stored_a, widened,
    info() with the dtype's name.  _name16 / _name32: the class's own name and its f32 family's, for the ValueErrors"""
    _name16 = _name32 = None

    def __init__(self, n, m, mats_a, vecs_b, vecs_c, seg_type, seg_len, param=None, a_dtype="f16", **kw):
        self.h = None
        self.a_dtype, self._a_kind = a_dtype, kind_of(a_dtype, self._name16, self._name32)
        super().__init__(n, m, mats_a, vecs_b, vecs_c, seg_type, seg_len, param, **kw)

    @classmethod
    def from_dense(cls, denses, param=None, a_dtype="f16", **kw):
        return super().from_dense(denses, param, a_dtype=a_dtype, **kw)

    def _create(self, *args):
        self._c("create_kind")(*args[:-1], self._a_kind, args[-1])
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
            raise ValueError("set_a_dev: a %s holds a 16-bit copy of every A and no f32 A lies in place to be read again: "
                             "hand the values in" % self._name16)
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
        self._c("stored")(self.h, int(i), words.ctypes.data, None if inv is None else inv.ctypes.data)
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
