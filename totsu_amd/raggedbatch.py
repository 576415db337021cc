"""`RaggedBatchSolver`: many conic programs in ONE batch, each with its OWN dense f32 A, its own shape n_p, m_p and its own cone
layout -- one relaxation per graph, one SVM per fold, one program per agent, MPC horizons of different length
(thip_raggedbatch_* in include/totsu_f32hip.h).  The kernel is the SDP batch's iteration on a problem the workgroup looks up in a
table: one workgroup per running problem, every vector in LDS, A streamed twice per iteration, PSD cones of order k <= 64 projected
on chip.  A problem's iterates are, bit for bit, those of a `MidBatchSolver` / `SdpBatchSolver` that holds it alone.

A launch has one workgroup size and one LDS size, so the problems are split by shape into a 256-thread class (m_p n_p <= 8192) and
a 1024-thread class, each with the largest LDS map of its members; every poll makes one launch per class that still has a running
problem, the longest problems (m_p n_p) first.  Problems take 6 n_p + 10 m_p floats of state each, packed; identical layouts share
one cone table.  `info()` reports all of it.

Taken: whatever `sdpbatch.fits` takes, problem by problem (`fits` here names the first problem refused).  Refused (ValueError): such
a problem, no problem at all, arrays of the wrong length, a device array at an offset that is no whole number of floats from the
others of its kind, `replace` with arrays of another length.

`ragged_batch(denses)` is the chooser's name.  Which route when: problems that share n, m and the cone layout go to `conic_batch`,
which can keep a small A in LDS (SmallBatchSolver) and launches without descriptors; problems whose shapes or layouts differ go to
`ragged_batch` instead of one `conic_batch` per distinct (n, m, layout)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .fused import DeviceBuffer, _c_param
from .ownbatch import OwnBatchSolver
from .solver import SolverParam

_KINDS = ("mat_a", "vec_b", "vec_c", "vec_b_rowabs")


def _shape_arrays(problems):
    """the arrays of thip_raggedbatch_fits for a list of Prob*.dense()-like problems (n, m, seg_type, seg_len)"""
    problems = list(problems)
    for k, d in enumerate(problems):
        if len(d.seg_type) != len(d.seg_len):
            raise ValueError("problem %d: seg_type and seg_len differ in length: %d vs %d" % (k, len(d.seg_type), len(d.seg_len)))
        if int(d.n) < 0 or int(d.m) < 0:
            raise ValueError("problem %d: negative shape (n = %r, m = %r)" % (k, d.n, d.m))
    n = np.array([int(d.n) for d in problems], dtype=np.uintp)
    m = np.array([int(d.m) for d in problems], dtype=np.uintp)
    ns = np.array([len(d.seg_type) for d in problems], dtype=np.uintp)
    st = np.array([int(t) for d in problems for t in d.seg_type], dtype=np.int32)
    sl = np.array([int(t) for d in problems for t in d.seg_len], dtype=np.int64)
    return problems, n, m, ns, st, sl


def _ptrs(n, m, ns, st, sl):
    ps = C.POINTER(C.c_size_t)
    return (len(n), n.ctypes.data_as(ps), m.ctypes.data_as(ps), ns.ctypes.data_as(ps), st.ctypes.data_as(C.POINTER(C.c_int32)),
            sl.ctypes.data_as(C.POINTER(C.c_int64)))


def fits(problems):
    """the shape rules alone (thip_raggedbatch_fits; needs no GPU): [(lds_bytes, threads)] of one workgroup per problem, or a
    ValueError that names the first problem refused (its index is the exception's `problem`)"""
    problems, n, m, ns, st, sl = _shape_arrays(problems)
    lds = np.zeros(len(problems), dtype=np.uintp)
    thr = np.zeros(len(problems), dtype=np.int32)
    bad = C.c_int(-1)
    try:
        lib.thip_raggedbatch_fits(*_ptrs(n, m, ns, st, sl), C.byref(bad), lds.ctypes.data_as(C.POINTER(C.c_size_t)),
                                  thr.ctypes.data_as(C.POINTER(C.c_int)))
    except _lib.ThipError as e:
        if e.code == _lib.E_INVALID:
            err = ValueError(str(e))
            err.problem = bad.value
            raise err from None
        raise
    return [(int(a), int(b)) for a, b in zip(lds, thr)]


def plan(problems, force_threads=None):
    """the launch plan a RaggedBatchSolver of these problems makes (thip_test_raggedbatch_plan; needs no GPU): a dict of `cls`
    (per problem: 0 the 256-thread class, 1 the 1024-thread class), `order` (per class, its members in the order of its live
    list), `layout` (per problem, the index of its cone table), `arena_at` (per problem, in floats) and `info` (the no-device part
    of info())"""
    problems, n, m, ns, st, sl = _shape_arrays(problems)
    P = len(problems)
    cls, order, lay = (np.zeros(P, dtype=np.int32) for _ in range(3))
    at = np.zeros(P, dtype=np.int64)
    o = _lib.RaggedBatchInfo()
    pi = C.POINTER(C.c_int)
    try:
        lib.thip_test_raggedbatch_plan(*_ptrs(n, m, ns, st, sl), int(force_threads or 0), cls.ctypes.data_as(pi), order.ctypes.data_as(pi),
                                       lay.ctypes.data_as(pi), at.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(o))
    except _lib.ThipError as e:
        if e.code == _lib.E_INVALID:
            raise ValueError(str(e)) from None
        raise
    n0 = int((cls == 0).sum())
    return {"cls": cls.tolist(), "order": [order[:n0].tolist(), order[n0:].tolist()], "layout": lay.tolist(), "arena_at": at.tolist(),
            "info": _info_dict(o)}


def _info_dict(o):
    d = {k: getattr(o, k) for k, _ in o._fields_ if k != "cls"}
    d["classes"] = [{k: getattr(c, k) for k, _ in c._fields_} for c in o.cls]
    return d


def pack(problems, kinds=_KINDS):
    """where from_dense puts the host arrays of each kind (needs no GPU): {kind: (one float32 array, [offset in floats per problem;
    -1: the problem has none])}.  Every array starts at a multiple of 4 floats, so an A whose m_p is a multiple of 4 is read with
    16-byte loads.  Problems whose array of a kind is already a DeviceBuffer get offset None there"""
    out = {}
    for kind in kinds:
        parts, at, o = [], [], 0
        for d in problems:
            v = getattr(d, kind, None)
            if v is None:
                at.append(-1)
            elif isinstance(v, DeviceBuffer):
                at.append(None)
            else:
                v = np.asarray(v, dtype=np.float32).ravel()
                at.append(o)
                parts.append((o, v))
                o += (v.size + 3) & ~3
        buf = np.zeros(o, dtype=np.float32)
        for a, v in parts:
            buf[a:a + v.size] = v
        out[kind] = (buf, at)
    return out


class RaggedBatchSolver(OwnBatchSolver):
    """run / run_until_any / status / solution / iterate / raw_iterate / set_iterate(s) / set_bc / set_a / solutions / the _dev round calls / statuses / precond /
    replace / reinit / set_param / info / solve / destroy of OwnBatchSolver, on thip_raggedbatch_*, with every length the problem's own.  `shapes`: [(n_p, m_p)].  force_threads: test hook
    (256, 1024: every problem in that one class)."""
    _prefix, _force_hook, _what = "thip_raggedbatch_", "thip_test_raggedbatch_force_threads", "ragged"

    def __init__(self, problems, param=None, force_threads=None):
        """problems: Prob*.dense()-like objects -- n, m, mat_a (m * n, column-major), vec_b (m), vec_c (n), seg_type, seg_len and
        vec_b_rowabs (m, or None: |b|); each array a host array (packed and uploaded) or a DeviceBuffer holding it (read in place)"""
        self.h = None
        self._owned = []
        self._slot_owned = {}
        problems = list(problems)
        self.n_prob = len(problems)
        if not 1 <= self.n_prob <= _lib.SMALLBATCH_MAX_PROB:
            raise ValueError("a ragged batch holds 1 .. %d problems, not %d" % (_lib.SMALLBATCH_MAX_PROB, self.n_prob))
        for k, d in enumerate(problems):
            self._check_lengths("problem %d: " % k, d.n, d.m, d.mat_a, d.vec_b, d.vec_c, getattr(d, "vec_b_rowabs", None))
        fits(problems)                      # every shape refusal, before anything is uploaded
        self.shapes = [(int(d.n), int(d.m)) for d in problems]
        self.param = param or SolverParam()
        _lib.ensure_init()
        try:
            base, ats = self._upload(problems, _KINDS)
            _, n, m, ns, st, sl = _shape_arrays(problems)
            par = _c_param(self.param)
            h = C.c_void_p()
            p64 = C.POINTER(C.c_int64)
            sp = _ptrs(n, m, ns, st, sl)

            def at(kind):
                return None if ats[kind] is None else ats[kind].ctypes.data_as(p64)
            lib.thip_raggedbatch_create(sp[0], sp[1], sp[2], base["mat_a"], at("mat_a"), base["vec_b"], at("vec_b"), base["vec_c"],
                                        at("vec_c"), base["vec_b_rowabs"], at("vec_b_rowabs"), sp[3], sp[4], sp[5], C.byref(par),
                                        C.byref(h))
            self.h = h
            self._data = problems           # (DeviceBuffers the caller handed in stay alive with the solver)
            if force_threads is not None:
                lib.thip_test_raggedbatch_force_threads(self.h, int(force_threads))
            lib.thip_raggedbatch_init(self.h)
        except _lib.ThipError as e:
            self.destroy()
            if e.code == _lib.E_INVALID:
                raise ValueError(str(e)) from None
            raise
        except Exception:
            self.destroy()
            raise

    def _upload(self, problems, kinds):
        """the host arrays of each kind packed and uploaded (the object owns them): ({kind: the lowest device address of the kind, or
        None}, {kind: the problems' offsets from it in floats as an int64 array (-1: the problem has none), or None})"""
        packed = pack(problems, kinds)
        base, ats = {}, {}
        for kind in kinds:
            buf, at = packed[kind]
            dev = self._dev(buf) if buf.size else None
            ptrs = [None if a == -1 else getattr(d, kind).ptr if a is None else dev.ptr + 4 * a for d, a in zip(problems, at)]
            have = [p for p in ptrs if p is not None]
            if not have:
                base[kind], ats[kind] = None, None
                continue
            base[kind] = min(have)
            for k, p in enumerate(ptrs):
                if p is not None and (p - base[kind]) % 4:
                    raise ValueError("problem %d: %s lies at a misaligned float offset (%d bytes from the others of its kind)"
                                     % (k, kind, p - base[kind]))
            ats[kind] = np.array([-1 if p is None else (p - base[kind]) // 4 for p in ptrs], dtype=np.int64)
        return base, ats

    @staticmethod
    def _check_lengths(what, n, m, mat_a, vec_b, vec_c, vec_b_rowabs):
        n, m = int(n), int(m)
        for name, v, want in (("mat_a", mat_a, m * n), ("vec_b", vec_b, m), ("vec_c", vec_c, n), ("vec_b_rowabs", vec_b_rowabs, m)):
            if v is None:
                if name == "vec_b_rowabs":
                    continue
                raise ValueError("%s%s is needed" % (what, name))
            got = v.n if isinstance(v, DeviceBuffer) else np.asarray(v).size
            if (got < want) if isinstance(v, DeviceBuffer) else (got != want):
                raise ValueError("%s%s: %d entries where %d are needed" % (what, name, got, want))

    @classmethod
    def from_dense(cls, denses, param=None, **kw):
        """one problem per Prob*.dense() of the list -- any mix of ProbLP / SOCP / SDP / QP / QCQP, with and without vec_b_rowabs"""
        return cls(list(denses), param, **kw)

    def replace(self, i, mat_a, vec_b, vec_c, vec_b_rowabs=None, start=None):
        """slot i -- running or stopped -- takes new data of ITS shape and cone layout as a fresh init; no other slot is touched.
        start: None, or the (x, y) the new problem starts from (replace, then set_iterate)"""
        if not 0 <= int(i) < self.n_prob:
            raise ValueError("replace: no slot %r in a batch of %d" % (i, self.n_prob))
        i, own = int(i), []
        n, m = self.shapes[i]
        self._check_lengths("replace: ", n, m, mat_a, vec_b, vec_c, vec_b_rowabs)
        start = self._start_of(i, start)
        try:
            da, db, dc = self._dev(mat_a, own), self._dev(vec_b, own), self._dev(vec_c, own)
            dr = None if vec_b_rowabs is None else self._dev(vec_b_rowabs, own)
            lib.thip_raggedbatch_replace(self.h, i, da.ptr, db.ptr, dc.ptr, None if dr is None else dr.ptr)
        except Exception:
            for d in own:
                d.free()
            raise
        old, self._slot_owned[i] = self._slot_owned.get(i, []), own
        for d in old:
            d.free()
        self._started(i, start)

    def _lengths(self, i):
        n, m = self._shape(i)
        return n + 2 * m + 1, n + m + 1

    def _nm(self, i):
        """(set_bc, solutions: every length is the problem's own)"""
        return self.shapes[int(i)]

    def _pair(self, name, i, nx, ny):
        x = np.empty(nx, dtype=np.float32)
        y = np.empty(ny, dtype=np.float32)
        self._c(name)(self.h, int(i), x.ctypes.data, y.ctypes.data)
        return x, y

    def _shape(self, i):
        if not 0 <= int(i) < self.n_prob:
            raise ValueError("no problem %r in a batch of %d" % (i, self.n_prob))
        return self.shapes[int(i)]

    def solution(self, i):
        n, m = self._shape(i)
        return self._pair("solution", i, n, m)

    def iterate(self, i):
        n, m = self._shape(i)
        return self._pair("iterate", i, n + 2 * m + 1, n + m + 1)

    def precond(self, i):
        n, m = self._shape(i)
        return self._pair("precond", i, n + 2 * m + 1, n + m + 1)

    def info(self):
        o = _lib.RaggedBatchInfo()
        lib.thip_raggedbatch_info(self.h, C.byref(o))
        return _info_dict(o)

    def destroy(self):
        OwnBatchSolver.destroy(self)
        self._data = None


def ragged_batch(denses, param=None, **kw):
    """the batch solver for a list of Prob*.dense() whose shapes or cone layouts DIFFER and that each have their own A: a
    RaggedBatchSolver over all of them -- one handle, one launch per workgroup-size class and poll -- where the only earlier route
    was one conic_batch per distinct (n, m, layout).  Problems that share n, m and the layout belong to conic_batch: it can keep a
    small A in LDS, which no ragged batch does, and its kernels are launched with the shape instead of looking it up.
    Measured (profiles/raggedbatch_rate.txt, one MI355X, problem-iterations/s against bucketing by (n, m, layout) with one
    conic_batch per bucket in turn, at P = 256 / 1024): every shape unique (LPs, n = 32 .. 512) 63x / 190x; four shapes x P / 4
    (LP 80 x 40, LP 256 x 128, SOCP 423 x 60, SDP 45 x 6) 1.21x / 1.05x -- bucketing wins on neither, but with a handful of buckets
    the gain is small, and a class lasts as long as its slowest member; ONE shape (LP 256 x 128) against MidBatchSolver itself
    0.95x: the descriptor and the forced live list cost 5 % where two runs of one class differ by 0.1 %."""
    return RaggedBatchSolver.from_dense(denses, param, **kw)
