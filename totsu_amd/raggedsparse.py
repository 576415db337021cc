"""`RaggedSparseBatchSolver`: many conic programs in ONE batch, each with its OWN SPARSE A with its own pattern, its own shape
n_p, m_p and its own cone layout -- one relaxation per graph on graphs of different size, banded MPC horizons of different length,
l1-regularised fits on folds of different size (thip_raggedsparse_* in include/totsu_f32hip.h;
totsu_amd/csrc/thip_raggedsparse.hip).  Where `RaggedBatchSolver` (different shapes, dense A) and `SparseBatchSolver` (one shape,
sparse A) meet: one workgroup per running problem looks its problem up in a table and walks that problem's packed entries.  A
problem's preconditioner, iterates and status are, bit for bit, those of a `SparseBatchSolver` that holds it alone.

The plan (`plan`, needs no GPU).  Slot p reserves room for cap_p entries -- the problem's own count unless `nnz_caps` gives more --
so `replace` can hand it another pattern.  The workgroup size is the sparse batch's rule on (n_p, m_p, cap_p), which splits the
problems into a 256-thread and a 1024-thread class; every poll makes one launch per class that still has a running problem, the
problems with the most entries first.  A problem whose blob fits the LDS left beside its own vectors is resident (copied there
once per launch), the others are read from memory: per problem, in one launch.  `info()` reports all of it.

Taken: whatever `sdpbatch.fits` takes, problem by problem, with cap_p <= m_p n_p.  Refused (ValueError, naming the problem): such a
problem, every refusal of the stored form (`sparsebatch`), no problem at all, arrays or `nnz_caps` of the wrong length; `replace`
with more than cap_i entries or arrays of another length.

Not here: a `replace` that changes a slot's shape, and any automatic choice between this family and the others -- `conic_batch`,
`own_a_batch` and `ragged_batch` are unchanged.  Which route when: see `RaggedSparseBatchSolver`."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .fused import DeviceBuffer, _c_param
from .raggedbatch import RaggedBatchSolver, _info_dict, _ptrs, _shape_arrays
from .solver import SolverParam
from .sparsebatch import _P32, _P64, _PF, SparseSetA, _pattern_of, _value_errors, csc_of, csc_of_dense

_KINDS = ("vec_b", "vec_c", "vec_b_rowabs")
_PSZ, _PI = C.POINTER(C.c_size_t), C.POINTER(C.c_int)


class SparseProblem:
    """the fields a RaggedSparseBatchSolver reads of a problem: n, m, mat (a (colptr, rowidx, values) triple or a scipy.sparse
    matrix of shape (m, n)), vec_b (m), vec_c (n), seg_type, seg_len and vec_b_rowabs (m, or None: |b|)"""

    def __init__(self, n, m, mat, vec_b, vec_c, seg_type, seg_len, vec_b_rowabs=None):
        self.n, self.m, self.mat, self.vec_b, self.vec_c = int(n), int(m), mat, vec_b, vec_c
        self.seg_type, self.seg_len, self.vec_b_rowabs = list(seg_type), list(seg_len), vec_b_rowabs

    @classmethod
    def of_dense(cls, d):
        """a Prob*.dense() with its A taken as the entries != 0"""
        return cls(d.n, d.m, csc_of_dense(d.mat_a, d.n, d.m), d.vec_b, d.vec_c, d.seg_type, d.seg_len, getattr(d, "vec_b_rowabs", None))


def _triples(problems):
    """every problem's A as a (colptr, rowidx, values) triple (sparsebatch.csc_of: the caller's object is never touched)"""
    out = []
    for k, d in enumerate(problems):
        try:
            out.append(csc_of(d.mat, int(d.n), int(d.m)))
        except ValueError as e:
            raise ValueError("problem %d: %s" % (k, e)) from None
    return out


def _caps(n_prob, nnz_caps):
    """the capacities as the C API takes them (0: the problem's own count)"""
    if nnz_caps is None:
        return np.zeros(n_prob, dtype=np.uintp)
    caps = [0 if c is None else int(c) for c in nnz_caps]
    if len(caps) != n_prob:
        raise ValueError("nnz_caps holds %d entries where %d problems are given" % (len(caps), n_prob))
    for k, c in enumerate(caps):
        if c < 0:
            raise ValueError("problem %d: a negative nnz_cap (%d)" % (k, c))
    return np.array(caps, dtype=np.uintp)


def _plan(problems, nnz, nnz_caps, force_threads, force_resident):
    problems, n, m, ns, st, sl = _shape_arrays(problems)
    P = len(problems)
    caps = _caps(P, nnz_caps)
    nnz = np.array(nnz, dtype=np.uintp)
    cls, order, lay, lds_at, res = (np.zeros(P, dtype=np.int32) for _ in range(5))
    at, blob_at = np.zeros(P, dtype=np.int64), np.zeros(P, dtype=np.int64)
    o = _lib.RaggedSparseInfo()
    sp = _ptrs(n, m, ns, st, sl)
    _value_errors(lib.thip_test_raggedsparse_plan, sp[0], sp[1], sp[2], nnz.ctypes.data_as(_PSZ), caps.ctypes.data_as(_PSZ), sp[3], sp[4],
                  sp[5], int(force_threads or 0), -1 if force_resident is None else int(force_resident), cls.ctypes.data_as(_PI),
                  order.ctypes.data_as(_PI), lay.ctypes.data_as(_PI), at.ctypes.data_as(_P64), blob_at.ctypes.data_as(_P64),
                  lds_at.ctypes.data_as(_PI), res.ctypes.data_as(_PI), C.byref(o))
    n0 = int((cls == 0).sum())
    return {"cls": cls.tolist(), "order": [order[:n0].tolist(), order[n0:].tolist()], "layout": lay.tolist(), "arena_at": at.tolist(),
            "blob_at": blob_at.tolist(), "lds_at": lds_at.tolist(), "resident": res.tolist(), "info": _info_dict(o)}


def _nnz_of(problems):
    """the entry counts: from `mat`, or -- for a problem given by its shape alone -- its `nnz` (0 when it has none)"""
    have = [k for k, d in enumerate(problems) if getattr(d, "mat", None) is not None]
    out = [int(getattr(d, "nnz", 0)) for d in problems]
    for k in have:
        try:
            out[k] = int(csc_of(problems[k].mat, int(problems[k].n), int(problems[k].m))[0][-1])
        except ValueError as e:
            raise ValueError("problem %d: %s" % (k, e)) from None
    return out


def fits(problems, nnz_caps=None):
    """the rules alone (thip_raggedsparse_fits; needs no GPU): [(lds_bytes, threads, resident)] of one workgroup per problem, for
    slots of nnz_caps entries (None: each problem's own count), or a ValueError that names the first problem refused (its index is
    the exception's `problem`)"""
    problems, n, m, ns, st, sl = _shape_arrays(problems)
    P = len(problems)
    caps = _caps(P, nnz_caps)
    if not caps.all():
        caps = np.where(caps == 0, np.array(_nnz_of(problems), dtype=np.uintp), caps).astype(np.uintp)
    lds = np.zeros(P, dtype=np.uintp)
    thr, res = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
    bad = C.c_int(-1)
    sp = _ptrs(n, m, ns, st, sl)
    try:
        lib.thip_raggedsparse_fits(sp[0], sp[1], sp[2], caps.ctypes.data_as(_PSZ), sp[3], sp[4], sp[5], C.byref(bad),
                                   lds.ctypes.data_as(_PSZ), thr.ctypes.data_as(_PI), res.ctypes.data_as(_PI))
    except _lib.ThipError as e:
        if e.code == _lib.E_INVALID:
            err = ValueError(str(e))
            err.problem = bad.value
            raise err from None
        raise
    return [(int(a), int(b), int(c)) for a, b, c in zip(lds, thr, res)]


def plan(problems, nnz_caps=None, force_threads=None, force_resident=None):
    """the plan a RaggedSparseBatchSolver of these problems makes (thip_test_raggedsparse_plan; needs no GPU): a dict of `cls` (per
    problem: 0 the 256-thread class, 1 the 1024-thread class), `order` (per class, its members in the order of its live list),
    `layout` (per problem, the index of its cone table), `arena_at` (floats), `blob_at` (bytes), `lds_at` (floats: where the resident
    copy lies), `resident` (per problem) and `info` (the no-device part of info())"""
    problems = list(problems)
    return _plan(problems, _nnz_of(problems), nnz_caps, force_threads, force_resident)


class RaggedSparseBatchSolver(SparseSetA, RaggedBatchSolver):
    """run / run_until_any / status / solution / iterate / raw_iterate / set_iterate(s) / set_bc / set_a / solutions / the _dev round calls / precond / replace /
    reinit / set_param / info / solve / destroy of OwnBatchSolver, on thip_raggedsparse_*, with every length the problem's own.  `shapes`: [(n_p, m_p)]; `nnz_caps`: the entries
    each slot can take.  force_threads (256, 1024: every problem in that one class) and force_resident (0: nobody resident, 1:
    everybody who fits) are test hooks.

    Which route when.  For sparse problems of different shapes the two earlier routes are one `SparseBatchSolver` per distinct
    (n, m, layout) in turn, or `ragged_batch` on the densified matrices.  Measured (profiles/raggedsparse_rate.txt, one MI355X,
    problem-iterations/s, this class against bucketing / against the densified ragged batch, at P = 256 and P = 1024):
    partitioning_sdp on 16 grids from (2, 2) to (4, 8) 11.5x / 2.62x and 3.66x / 1.22x; sparse LPs with every shape unique
    (n = 32 .. 512, m = 2 n) at 1 % density 125x / 8.1x and 246x / 6.9x, at 5 % 59x / 1.62x and 141x / 1.67x -- neither earlier
    route wins on any of them; the margin over the dense route shrinks with the density, as the sparse batch's does.  ONE shape
    (partitioning_sdp(4, 8)) against `SparseBatchSolver` itself: 1.002 and 1.001, where two runs of either class differ by 0.2 %:
    the descriptor and the forced live list cost nothing that this measurement can see.  Problems whose A is mostly entries
    still belong to `ragged_batch`: an entry costs 16 bytes against 4."""
    _prefix, _force_hook, _what = "thip_raggedsparse_", "thip_test_raggedsparse_force_threads", "ragged sparse"

    def __init__(self, problems, param=None, nnz_caps=None, force_threads=None, force_resident=None):
        """problems: objects with n, m, mat (a (colptr, rowidx, values) triple or a scipy.sparse matrix, host), vec_b (m), vec_c (n),
        seg_type, seg_len and optionally vec_b_rowabs (m, or None: |b|) -- the vectors host arrays (packed and uploaded) or
        DeviceBuffers (read in place).  nnz_caps: per problem the entries its slot can take (None: its own count)"""
        self.h = None
        self._owned = []
        self._slot_owned = {}
        problems = list(problems)
        self.n_prob = len(problems)
        if not 1 <= self.n_prob <= _lib.SMALLBATCH_MAX_PROB:
            raise ValueError("a ragged sparse batch holds 1 .. %d problems, not %d" % (_lib.SMALLBATCH_MAX_PROB, self.n_prob))
        caps = _caps(self.n_prob, nnz_caps)
        _shape_arrays(problems)
        for k, d in enumerate(problems):
            self._check_vectors("problem %d: " % k, d.n, d.m, d.vec_b, d.vec_c, getattr(d, "vec_b_rowabs", None))
        triples = _triples(problems)
        self._patterns = [_pattern_of(t) for t in triples]
        counts = [int(t[0][-1]) for t in triples]
        _plan(problems, counts, caps, force_threads, force_resident)       # every refusal of the rule, before anything is uploaded
        self.shapes = [(int(d.n), int(d.m)) for d in problems]
        self.nnz_caps = [int(c) if c else k for c, k in zip(caps, counts)]
        colptr = np.concatenate([t[0] for t in triples])
        start = np.zeros(self.n_prob, dtype=np.int64)
        np.cumsum([t[1].size for t in triples[:-1]], out=start[1:])
        rowidx = np.ascontiguousarray(np.concatenate([t[1] for t in triples]), dtype=np.int32)
        values = np.ascontiguousarray(np.concatenate([t[2] for t in triples]), dtype=np.float32)
        self.param = param or SolverParam()
        _lib.ensure_init()
        try:
            base, ats = self._upload(problems, _KINDS)
            _, n, m, ns, st, sl = _shape_arrays(problems)
            par = _c_param(self.param)
            h = C.c_void_p()
            sp = _ptrs(n, m, ns, st, sl)

            def at(kind):
                return None if ats[kind] is None else ats[kind].ctypes.data_as(_P64)
            _value_errors(lib.thip_raggedsparse_create, sp[0], sp[1], sp[2], colptr.ctypes.data_as(_P64), start.ctypes.data_as(_P64),
                          rowidx.ctypes.data_as(_P32), values.ctypes.data_as(_PF), caps.ctypes.data_as(_PSZ), base["vec_b"], at("vec_b"),
                          base["vec_c"], at("vec_c"), base["vec_b_rowabs"], at("vec_b_rowabs"), sp[3], sp[4], sp[5], C.byref(par),
                          C.byref(h))
            self.h = h
            self._data = problems           # (DeviceBuffers the caller handed in stay alive with the solver)
            if force_threads is not None:
                _value_errors(lib.thip_test_raggedsparse_force_threads, self.h, int(force_threads))
            if force_resident is not None:
                _value_errors(lib.thip_test_raggedsparse_force_resident, self.h, int(force_resident))
            lib.thip_raggedsparse_init(self.h)
        except Exception:
            self.destroy()
            raise

    @staticmethod
    def _check_vectors(what, n, m, vec_b, vec_c, vec_b_rowabs):
        for name, v, want in (("vec_b", vec_b, int(m)), ("vec_c", vec_c, int(n)), ("vec_b_rowabs", vec_b_rowabs, int(m))):
            if v is None:
                if name == "vec_b_rowabs":
                    continue
                raise ValueError("%s%s is needed" % (what, name))
            got = v.n if isinstance(v, DeviceBuffer) else np.asarray(v).size
            if (got < want) if isinstance(v, DeviceBuffer) else (got != want):
                raise ValueError("%s%s: %d entries where %d are needed" % (what, name, got, want))

    @classmethod
    def from_dense(cls, denses, param=None, **kw):
        """one problem per Prob*.dense() of the list -- any mix of ProbLP / SOCP / SDP / QP / QCQP --, its A taken as the entries != 0"""
        return cls([SparseProblem.of_dense(d) for d in denses], param, **kw)

    def replace(self, i, mat, vec_b, vec_c, vec_b_rowabs=None, start=None):
        """slot i -- running or stopped -- takes another problem of ITS shape and cone layout, mat of any pattern with at most
        nnz_caps[i] entries, as a fresh init; no other slot is touched, and a refusal leaves the slot as it was.  start: None, or the
        (x, y) the new problem starts from (replace, then set_iterate)"""
        if not 0 <= int(i) < self.n_prob:
            raise ValueError("replace: no slot %r in a batch of %d" % (i, self.n_prob))
        start = self._start_of(i, start)
        i, own = int(i), []
        n, m = self.shapes[i]
        try:
            cp, ri, va = csc_of(mat, n, m)
        except ValueError as e:
            raise ValueError("replace: %s" % e) from None
        if int(cp[-1]) > self.nnz_caps[i]:
            raise ValueError("replace: the problem holds %d entries where nnz_cap is %d" % (int(cp[-1]), self.nnz_caps[i]))
        self._check_vectors("replace: ", n, m, vec_b, vec_c, vec_b_rowabs)
        try:
            db, dc = self._dev(vec_b, own), self._dev(vec_c, own)
            dr = None if vec_b_rowabs is None else self._dev(vec_b_rowabs, own)
            _value_errors(lib.thip_raggedsparse_replace, self.h, i, cp.ctypes.data_as(_P64), ri.ctypes.data_as(_P32), va.ctypes.data_as(_PF),
                          db.ptr, dc.ptr, None if dr is None else dr.ptr)
        except Exception:
            for d in own:
                d.free()
            raise
        self._patterns[i] = _pattern_of((cp, ri, va))
        old, self._slot_owned[i] = self._slot_owned.get(i, []), own
        for d in old:
            d.free()
        self._started(i, start)

    def info(self):
        o = _lib.RaggedSparseInfo()
        lib.thip_raggedsparse_info(self.h, C.byref(o))
        return _info_dict(o)
