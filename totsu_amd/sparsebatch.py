"""`SparseBatchSolver`: many conic programs of one shape n, m and one cone layout, each with its OWN SPARSE A with its own pattern
(thip_sparsebatch_* in include/totsu_f32hip.h; totsu_amd/csrc/thip_sparsebatch.hip).  The iteration is the SDP batch's -- one
workgroup per problem, every vector in LDS, all five cones with PSD orders <= 64 projected on chip, poll_every whole iterations per
launch -- but A is held as its entries: the library packs each problem's CSC arrays on the host into a blob that holds the entries
in column order and in row order, and a pass walks them.  When the blob fits the LDS left beside the vectors it is copied there
once per launch (resident); otherwise the batch is taken all the same and the entries are read from memory (streamed), with the same
bits.  The host machinery and the methods are `OwnBatchSolver`'s (totsu_amd/ownbatch.py).

Taken: what `sdpbatch.fits` takes, at any number of entries.  Every slot reserves room for nnz_cap entries (the largest count among
the problems given, or more if the caller says so), so `replace` can hand a slot another pattern.  Refused (ValueError): column
pointers that are not monotone from 0, a row index out of range or not strictly ascending inside its column, a value that is not
finite, more entries than nnz_cap, nnz_cap > m n, and every refusal of the SDP batch's rule.  Explicit zeros are kept as entries.

There is no automatic choice between this family and the dense ones: `conic_batch`, `own_a_batch` and `ragged_batch` are unchanged."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .fused import DeviceBuffer, _c_param
from .ownbatch import OwnBatchSolver
from .solver import SolverParam

_P32, _P64, _PF = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_float)


def _value_errors(fn, *a):
    try:
        return fn(*a)
    except _lib.ThipError as e:
        if e.code == _lib.E_INVALID:
            raise ValueError(str(e)) from None
        raise


def fits(n, m, seg_type, seg_len, nnz_cap=0):
    """the rule alone (thip_sparsebatch_fits; needs no GPU): (lds_bytes, threads, resident) of one workgroup of a batch whose slots
    take nnz_cap entries, or ValueError"""
    st = np.ascontiguousarray(seg_type, dtype=np.int32)
    sl = np.ascontiguousarray(seg_len, dtype=np.int64)
    if st.size != sl.size:
        raise ValueError("seg_type and seg_len differ in length: %d vs %d" % (st.size, sl.size))
    if int(n) < 0 or int(m) < 0 or int(nnz_cap) < 0:
        raise ValueError("negative shape (n = %r, m = %r, nnz_cap = %r)" % (n, m, nnz_cap))
    lds, thr, res = C.c_size_t(), C.c_int(), C.c_int()
    _value_errors(lib.thip_sparsebatch_fits, int(n), int(m), int(nnz_cap), st.size, st.ctypes.data_as(_P32), sl.ctypes.data_as(_P64),
                  C.byref(lds), C.byref(thr), C.byref(res))
    return lds.value, thr.value, res.value


def capacity_bytes(n, m, nnz_cap):
    """what every slot of a batch reserves for its blob"""
    return (16 * int(nnz_cap) + 4 * (2 * (int(m) + int(n)) + 4) + 15) & ~15


def csc_of(mat, n, m):
    """(colptr int64, rowidx int32, values float32) of one problem's A: a (colptr, rowidx, values) triple, taken as it is, or a
    scipy.sparse matrix of shape (m, n), converted into a copy (duplicates summed, indices sorted; the caller's object is never
    touched)"""
    if not isinstance(mat, (tuple, list)):
        try:
            import scipy.sparse as sp
        except ImportError:
            sp = None
        if sp is None or not sp.issparse(mat):
            raise ValueError("a matrix is a (colptr, rowidx, values) triple or a scipy.sparse matrix, not %s" % type(mat).__name__)
        if mat.shape != (m, n):
            raise ValueError("a matrix of shape %r where %d x %d is needed" % (mat.shape, m, n))
        c = sp.csc_matrix(mat, copy=True)
        c.sum_duplicates()
        c.sort_indices()
        mat = (c.indptr, c.indices, c.data)
    if len(mat) != 3:
        raise ValueError("a matrix is a (colptr, rowidx, values) triple")
    cp = np.ascontiguousarray(mat[0], dtype=np.int64).ravel()
    ri = np.ascontiguousarray(mat[1], dtype=np.int32).ravel()
    va = np.ascontiguousarray(mat[2], dtype=np.float32).ravel()
    if cp.size != n + 1:
        raise ValueError("colptr holds %d entries where n + 1 = %d are needed" % (cp.size, n + 1))
    if ri.size != va.size:
        raise ValueError("rowidx and values differ in length: %d vs %d" % (ri.size, va.size))
    if cp[-1] > va.size:
        raise ValueError("colptr ends at %d where %d entries are given" % (cp[-1], va.size))
    return cp, ri, va


def csc_of_dense(mat_a, n, m):
    """the entries != 0 of a dense column-major A (m * n floats) as a CSC triple"""
    a = np.asarray(mat_a, dtype=np.float32).reshape(n, m)          # a[j, i] = A[i, j]
    cols, rows = np.nonzero(a)
    cp = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=cp[1:])
    return cp, rows.astype(np.int32), a[cols, rows]


def pack(n, m, mat, nnz_cap=0):
    """the blob the library stores for one problem (thip_test_sparsebatch_pack; needs no GPU): (the used words as a uint32 array,
    the row length above which a row is summed by a wave); ValueError for every refusal of the stored form"""
    n, m = int(n), int(m)
    cp, ri, va = csc_of(mat, n, m)
    used, long_len = C.c_size_t(), C.c_int()
    args = (n, m, cp.ctypes.data_as(_P64), ri.ctypes.data_as(_P32), va.ctypes.data_as(_PF), int(nnz_cap))
    _value_errors(lib.thip_test_sparsebatch_pack, *args, None, 0, C.byref(used), C.byref(long_len))
    out = np.zeros(used.value, dtype=np.uint32)
    _value_errors(lib.thip_test_sparsebatch_pack, *args, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(used),
                  C.byref(long_len))
    return out, long_len.value


def pattern_values(pattern, item, n, m, i):
    """what set_a of a sparse family makes of one problem's item (needs no handle): a plain array of values is returned as it is;
    a (colptr, rowidx, values) triple or a scipy.sparse matrix must have exactly `pattern` = (colptr, rowidx), slot i's present
    one, and gives its values.  ValueError otherwise: another pattern is replace's"""
    triple = isinstance(item, (tuple, list)) and len(item) == 3 and np.ndim(item[0]) == 1
    if not triple and (isinstance(item, (tuple, list, np.ndarray)) or np.isscalar(item)):
        return item
    cp, ri, va = csc_of(item, n, m)
    nnz = int(cp[-1])
    if not (np.array_equal(cp, pattern[0]) and np.array_equal(ri[:nnz], pattern[1])):
        raise ValueError("problem %d: the matrix has another pattern than the slot holds (%d entries against %d); set_a keeps the "
                         "pattern -- use replace for another one" % (i, nnz, int(pattern[0][-1])))
    return va[:nnz]


def _pattern_of(triple):
    cp, ri, _ = triple
    return cp.copy(), ri[:int(cp[-1])].copy()


class SparseSetA:
    """set_a's sparse side, shared by SparseBatchSolver and RaggedSparseBatchSolver: `_patterns[i]`, slot i's (colptr, rowidx) as
    of construction or its last replace, kept on the host for the comparison"""

    def _a_size(self, i):
        return int(self._patterns[int(i)][0][-1])

    def _a_values(self, i, item):
        n, m = self._nm(i)
        return pattern_values(self._patterns[int(i)], item, n, m, int(i))

    def blob(self, i):
        """TEST HOOK: slot i's blob as it lies on the device, a uint32 array of the words it uses"""
        fn = getattr(lib, "thip_test_%s_blob" % self._prefix[len("thip_"):-1])
        used = C.c_size_t()
        _value_errors(fn, self.h, int(i), None, 0, C.byref(used))
        out = np.zeros(used.value, dtype=np.uint32)
        _value_errors(fn, self.h, int(i), out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size, C.byref(used))
        return out


class SparseBatchSolver(SparseSetA, OwnBatchSolver):
    """run / run_until_any / status / solution / iterate / precond / set_iterate(s) / set_bc / set_a / solutions / the _dev round calls / reinit / set_param /
    info / solve / destroy of OwnBatchSolver, on thip_sparsebatch_*.  force_threads (256, 1024) and force_resident (0: read the entries from memory, 1: from LDS) are test
    hooks.  info() adds nnz_cap, nnz_total, blob_bytes, resident and the PSD fields of the SDP batch; a_bytes_per_iter is 0 when
    resident."""
    _prefix, _force_hook, _what, _Info = "thip_sparsebatch_", "thip_test_sparsebatch_force_threads", "sparse", _lib.SparseBatchInfo

    def __init__(self, n, m, mats, vecs_b, vecs_c, seg_type, seg_len, param=None, vecs_b_rowabs=None, nnz_cap=None, force_threads=None,
                 force_resident=None):
        """mats: one (colptr, rowidx, values) triple or scipy.sparse matrix per problem (host); vecs_b: (P, m); vecs_c: (P, n);
        vecs_b_rowabs: (P, m) or None (|b|) -- host arrays (uploaded) or DeviceBuffers.  nnz_cap: the entries a slot can take
        (None: the largest count given)"""
        self.h = None
        self._owned = []
        self._slot_owned = {}
        self.n, self.m = int(n), int(m)
        fits(self.n, self.m, seg_type, seg_len)             # every shape refusal, before anything is converted or uploaded
        mats = list(mats)
        self.n_prob = len(mats)
        if not 1 <= self.n_prob <= _lib.SMALLBATCH_MAX_PROB:
            raise ValueError("a sparse batch holds 1 .. %d problems, not %d" % (_lib.SMALLBATCH_MAX_PROB, self.n_prob))
        for name, arr, per in (("vecs_b", vecs_b, self.m), ("vecs_c", vecs_c, self.n), ("vecs_b_rowabs", vecs_b_rowabs, self.m)):
            if arr is None and name == "vecs_b_rowabs":
                continue
            got = arr.n if isinstance(arr, DeviceBuffer) else np.asarray(arr).size
            want = self.n_prob * per
            if (got < want) if isinstance(arr, DeviceBuffer) else (got != want):
                raise ValueError("%s: %d entries where %d problems x %d = %d are needed" % (name, got, self.n_prob, per, want))
        triples = [csc_of(mt, self.n, self.m) for mt in mats]
        self._patterns = [_pattern_of(t) for t in triples]
        counts = [int(t[0][-1]) for t in triples]
        cap = 0 if nnz_cap is None else int(nnz_cap)
        if nnz_cap is not None:
            if cap > self.m * self.n:
                raise ValueError("nnz_cap %d exceeds m n = %d" % (cap, self.m * self.n))
            for k, c in enumerate(counts):
                if c > cap:
                    raise ValueError("problem %d holds %d entries where nnz_cap is %d" % (k, c, cap))
        self.nnz_cap = cap if nnz_cap is not None else max(counts)
        colptr = np.concatenate([t[0] for t in triples])
        start = np.zeros(self.n_prob, dtype=np.int64)
        np.cumsum([t[1].size for t in triples[:-1]], out=start[1:])
        rowidx = np.ascontiguousarray(np.concatenate([t[1] for t in triples]), dtype=np.int32)
        values = np.ascontiguousarray(np.concatenate([t[2] for t in triples]), dtype=np.float32)
        self.param = param or SolverParam()
        self._st = np.ascontiguousarray(seg_type, dtype=np.int32)
        self._sl = np.ascontiguousarray(seg_len, dtype=np.int64)
        _lib.ensure_init()
        try:
            self.vecs_b, self.vecs_c = self._dev(vecs_b), self._dev(vecs_c)
            self.vecs_b_rowabs = None if vecs_b_rowabs is None else self._dev(vecs_b_rowabs)
            par = _c_param(self.param)
            h = C.c_void_p()
            _value_errors(lib.thip_sparsebatch_create, self.n, self.m, self.n_prob, colptr.ctypes.data_as(_P64),
                          start.ctypes.data_as(_P64), rowidx.ctypes.data_as(_P32), values.ctypes.data_as(_PF), self.vecs_b.ptr,
                          self.vecs_c.ptr, None if self.vecs_b_rowabs is None else self.vecs_b_rowabs.ptr, cap, len(self._st),
                          self._st.ctypes.data_as(_P32), self._sl.ctypes.data_as(_P64), C.byref(par), C.byref(h))
            self.h = h
            if force_threads is not None:
                _value_errors(lib.thip_test_sparsebatch_force_threads, self.h, int(force_threads))
            if force_resident is not None:
                _value_errors(lib.thip_test_sparsebatch_force_resident, self.h, int(force_resident))
            lib.thip_sparsebatch_init(self.h)
        except Exception:
            self.destroy()
            raise

    @classmethod
    def from_dense(cls, denses, param=None, **kw):
        """one problem per Prob*.dense() of the list, its A as the entries != 0; ValueError when their shapes or cone layouts differ"""
        denses = cls.check_same_layout(denses)
        d0 = denses[0]
        f = np.float32
        mats = [csc_of_dense(d.mat_a, d0.n, d0.m) for d in denses]
        b = np.stack([np.asarray(d.vec_b, f).ravel() for d in denses]).reshape(len(denses), d0.m)
        c = np.stack([np.asarray(d.vec_c, f).ravel() for d in denses]).reshape(len(denses), d0.n)
        r = None if d0.vec_b_rowabs is None else np.stack([np.asarray(d.vec_b_rowabs, f).ravel() for d in denses])
        return cls(d0.n, d0.m, mats, b, c, d0.seg_type, d0.seg_len, param, vecs_b_rowabs=r, **kw)

    def replace(self, i, mat, vec_b, vec_c, vec_b_rowabs=None, start=None):
        """slot i -- running or stopped -- takes the problem (mat, vec_b, vec_c[, vec_b_rowabs]) as a fresh init, mat of any pattern
        with at most nnz_cap entries; no other slot is touched.  start: None, or the (x, y) the new problem starts from (replace,
        then set_iterate)"""
        if not 0 <= int(i) < self.n_prob:
            raise ValueError("replace: no slot %r in a batch of %d" % (i, self.n_prob))
        start = self._start_of(i, start)
        cp, ri, va = csc_of(mat, self.n, self.m)
        if int(cp[-1]) > self.nnz_cap:
            raise ValueError("replace: the problem holds %d entries where nnz_cap is %d" % (int(cp[-1]), self.nnz_cap))
        for name, v, want in (("vec_b", vec_b, self.m), ("vec_c", vec_c, self.n), ("vec_b_rowabs", vec_b_rowabs, self.m)):
            if v is None:
                if name == "vec_b_rowabs":
                    continue
                raise ValueError("replace: %s is needed" % name)
            got = v.n if isinstance(v, DeviceBuffer) else np.asarray(v).size
            if (got < want) if isinstance(v, DeviceBuffer) else (got != want):
                raise ValueError("%s: %d entries where %d are needed" % (name, got, want))
        i, own = int(i), []
        try:
            db, dc = self._dev(vec_b, own), self._dev(vec_c, own)
            dr = None if vec_b_rowabs is None else self._dev(vec_b_rowabs, own)
            _value_errors(lib.thip_sparsebatch_replace, self.h, i, cp.ctypes.data_as(_P64), ri.ctypes.data_as(_P32),
                          va.ctypes.data_as(_PF), db.ptr, dc.ptr, None if dr is None else dr.ptr)
        except Exception:
            for d in own:
                d.free()
            raise
        self._patterns[i] = _pattern_of((cp, ri, va))
        old, self._slot_owned[i] = self._slot_owned.get(i, []), own
        for d in old:
            d.free()
        self._started(i, start)
