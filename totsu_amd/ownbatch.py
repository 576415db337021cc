"""What the own-A batch solvers share -- `SmallBatchSolver` (A in LDS), `MidBatchSolver` (A streamed) and `SdpBatchSolver` (A
streamed, PSD cones projected on chip): many conic programs of one shape n, m and one cone layout, each with its OWN dense f32 A,
one workgroup per problem, a launch advancing every running problem by poll_every iterations (the generic C API of
totsu_amd/csrc/thip_ownbatch.h).  `OwnBatchSolver` is the whole host side; a family is a subclass that names its prefix of the C
API, its test hook, its word for the ValueErrors and its info record.  `_fits` is the shape rule of a family by prefix,
`first_that_takes` the chooser over an ordered list of families."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .fused import DeviceBuffer, FusedResult, _c_param, _checked, _raw, _start_scalars
from .solver import SolverError, SolverParam


def _fits(prefix, n, m, seg_type, seg_len):
    st = np.ascontiguousarray(seg_type, dtype=np.int32)
    sl = np.ascontiguousarray(seg_len, dtype=np.int64)
    if st.size != sl.size:
        raise ValueError("seg_type and seg_len differ in length: %d vs %d" % (st.size, sl.size))
    if int(n) < 0 or int(m) < 0:
        raise ValueError("negative shape (n = %r, m = %r)" % (n, m))
    lds, thr = C.c_size_t(), C.c_int()
    try:
        getattr(lib, prefix + "fits")(int(n), int(m), st.size, st.ctypes.data_as(C.POINTER(C.c_int32)), sl.ctypes.data_as(C.POINTER(C.c_int64)),
                                      C.byref(lds), C.byref(thr))
    except _lib.ThipError as e:
        if e.code == _lib.E_INVALID:
            raise ValueError(str(e)) from None
        raise
    return lds.value, thr.value


def first_that_takes(families, n, m, seg_type, seg_len, refusal):
    """the first class of the ordered list of (class, rule) whose rule -- a `fits` -- takes the shape and the cone layout (needs no
    GPU); ValueError(refusal % (m, n, the last rule's words)) when none does"""
    for cls, rule in families:
        try:
            rule(n, m, seg_type, seg_len)
        except ValueError as e:
            last = e
            continue
        return cls
    raise ValueError(refusal % (m, n, last)) from None


class OwnBatchSolver:
    # what a family of own-A batches differs in (the subclasses set these)
    _prefix = _force_hook = _what = _Info = None

    def _c(self, name):
        return getattr(lib, self._prefix + name)

    def __init__(self, n, m, mats_a, vecs_b, vecs_c, seg_type, seg_len, param=None, vecs_b_rowabs=None, force_threads=None):
        """mats_a: (P, m * n) -- every A column-major; vecs_b: (P, m); vecs_c: (P, n); vecs_b_rowabs: (P, m) or None (|b|) -- host
        arrays (uploaded) or DeviceBuffers holding the same, problem after problem.  force_threads: the family's test hook."""
        self.h = None
        self._owned = []
        self._slot_owned = {}
        self.n, self.m = int(n), int(m)
        _fits(self._prefix, self.n, self.m, seg_type, seg_len)      # every shape refusal, before anything is uploaded
        self.n_prob = self._count(vecs_b, self.m, "vecs_b")
        if not 1 <= self.n_prob <= _lib.SMALLBATCH_MAX_PROB:
            raise ValueError("a %s batch holds 1 .. %d problems, not %d" % (self._what, _lib.SMALLBATCH_MAX_PROB, self.n_prob))
        for name, arr, per in (("mats_a", mats_a, self.m * self.n), ("vecs_b", vecs_b, self.m), ("vecs_c", vecs_c, self.n),
                               ("vecs_b_rowabs", vecs_b_rowabs, self.m)):
            if arr is None and name == "vecs_b_rowabs":
                continue
            got = arr.n if isinstance(arr, DeviceBuffer) else np.asarray(arr).size
            want = self.n_prob * per
            if (got < want) if isinstance(arr, DeviceBuffer) else (got != want):
                raise ValueError("%s: %d entries where %d problems x %d = %d are needed" % (name, got, self.n_prob, per, want))
        self.param = param or SolverParam()
        self._st = np.ascontiguousarray(seg_type, dtype=np.int32)
        self._sl = np.ascontiguousarray(seg_len, dtype=np.int64)
        _lib.ensure_init()
        try:
            self.mats_a, self.vecs_b, self.vecs_c = self._dev(mats_a), self._dev(vecs_b), self._dev(vecs_c)
            self.vecs_b_rowabs = None if vecs_b_rowabs is None else self._dev(vecs_b_rowabs)
            par = _c_param(self.param)
            h = C.c_void_p()
            self._c("create")(self.n, self.m, self.n_prob, self.mats_a.ptr, self.vecs_b.ptr, self.vecs_c.ptr,
                              None if self.vecs_b_rowabs is None else self.vecs_b_rowabs.ptr, len(self._st),
                              self._st.ctypes.data_as(C.POINTER(C.c_int32)), self._sl.ctypes.data_as(C.POINTER(C.c_int64)),
                              C.byref(par), C.byref(h))
            self.h = h
            if force_threads is not None:
                getattr(lib, self._force_hook)(self.h, int(force_threads))
            self._c("init")(self.h)
        except Exception:
            self.destroy()
            raise

    @staticmethod
    def _count(vecs_b, m, name):
        if isinstance(vecs_b, DeviceBuffer):
            return vecs_b.n // max(m, 1)
        a = np.asarray(vecs_b)
        if a.ndim == 2:
            return a.shape[0]
        return a.size // max(m, 1)

    @staticmethod
    def check_same_layout(denses):
        """ValueError unless every Prob*.dense() of the list has the first one's n, m and cone layout (needs no GPU)"""
        denses = list(denses)
        if not denses:
            raise ValueError("from_dense needs at least one problem")
        d0 = denses[0]
        lay0 = (list(map(int, d0.seg_type)), list(map(int, d0.seg_len)))
        for k, d in enumerate(denses):
            if (d.n, d.m) != (d0.n, d0.m):
                raise ValueError("problem %d is %d x %d where problem 0 is %d x %d" % (k, d.m, d.n, d0.m, d0.n))
            if (list(map(int, d.seg_type)), list(map(int, d.seg_len))) != lay0:
                raise ValueError("problem %d has another cone layout than problem 0" % k)
            if (d.vec_b_rowabs is None) != (d0.vec_b_rowabs is None):
                raise ValueError("problem %d and problem 0 differ in whether they carry vec_b_rowabs" % k)
            if np.asarray(d.mat_a).size != d0.n * d0.m:
                raise ValueError("problem %d: mat_a holds %d entries where m * n = %d are needed" % (k, np.asarray(d.mat_a).size, d0.n * d0.m))
        return denses

    @classmethod
    def from_dense(cls, denses, param=None, **kw):
        """one problem per Prob*.dense() of the list; ValueError when their shapes or cone layouts differ"""
        denses = cls.check_same_layout(denses)
        d0 = denses[0]
        f = np.float32
        a = np.stack([np.asarray(d.mat_a, f).ravel() for d in denses])
        b = np.stack([np.asarray(d.vec_b, f).ravel() for d in denses]).reshape(len(denses), d0.m)
        c = np.stack([np.asarray(d.vec_c, f).ravel() for d in denses]).reshape(len(denses), d0.n)
        r = None if d0.vec_b_rowabs is None else np.stack([np.asarray(d.vec_b_rowabs, f).ravel() for d in denses])
        return cls(d0.n, d0.m, a, b, c, d0.seg_type, d0.seg_len, param, vecs_b_rowabs=r, **kw)

    def _dev(self, a, owned=None):
        if isinstance(a, DeviceBuffer):
            return a
        d = DeviceBuffer.from_host(a)
        (self._owned if owned is None else owned).append(d)
        return d

    def replace(self, i, mat_a, vec_b, vec_c, vec_b_rowabs=None, start=None):
        """slot i -- running or stopped -- takes the problem (mat_a, vec_b, vec_c[, vec_b_rowabs]) as a fresh init; no other slot
        is touched.  What the object had uploaded for the slot's previous replacement is freed after the call.  start: None, or the
        (x, y) the new problem starts from (replace, then set_iterate)."""
        if not 0 <= int(i) < self.n_prob:
            raise ValueError("replace: no slot %r in a batch of %d" % (i, self.n_prob))
        start = self._start_of(i, start)
        for name, v, want in (("mat_a", mat_a, self.m * self.n), ("vec_b", vec_b, self.m), ("vec_c", vec_c, self.n),
                              ("vec_b_rowabs", vec_b_rowabs, self.m)):
            if v is None:
                if name == "vec_b_rowabs":
                    continue
                raise ValueError("replace: %s is needed" % name)
            got = v.n if isinstance(v, DeviceBuffer) else np.asarray(v).size
            if (got < want) if isinstance(v, DeviceBuffer) else (got != want):
                raise ValueError("%s: %d entries where %d are needed" % (name, got, want))
        i, own = int(i), []
        try:
            da, db, dc = self._dev(mat_a, own), self._dev(vec_b, own), self._dev(vec_c, own)
            dr = None if vec_b_rowabs is None else self._dev(vec_b_rowabs, own)
            self._c("replace")(self.h, i, da.ptr, db.ptr, dc.ptr, None if dr is None else dr.ptr)
        except Exception:
            for d in own:
                d.free()
            raise
        old, self._slot_owned[i] = self._slot_owned.get(i, []), own
        for d in old:
            d.free()
        self._started(i, start)

    def _lengths(self, i):
        """the lengths of problem i's x and y as iterate(i) returns them"""
        return self.n + 2 * self.m + 1, self.n + self.m + 1

    def _start_of(self, i, start):
        """replace's start argument, checked before anything is uploaded: None, or (x, y) as float32 arrays"""
        if start is None:
            return None
        x, y = start
        return self._iterates(int(i), [x], [y])

    def _started(self, i, start):
        if start is not None:
            self._set_checked(int(i), 1, *start)

    def _iterates(self, first, xs, ys):
        """(the xs one after another, the ys likewise) for the problems from `first` on, every length, tau and kappa checked
        (ValueError) -- before replace(start=) touches the slot"""
        xs, ys = list(xs), list(ys)
        if len(xs) != len(ys) or not xs:
            raise ValueError("set_iterates: %d x where there are %d y (one pair per problem, at least one)" % (len(xs), len(ys)))
        if not 0 <= int(first) <= int(first) + len(xs) <= self.n_prob:
            raise ValueError("set_iterates: no problems %r .. %r in a batch of %d" % (first, int(first) + len(xs) - 1, self.n_prob))
        out_x, out_y = [], []
        for k, (x, y) in enumerate(zip(xs, ys)):
            x, y = np.ascontiguousarray(x, dtype=np.float32).ravel(), np.ascontiguousarray(y, dtype=np.float32).ravel()
            nx, ny = self._lengths(int(first) + k)
            if x.size != nx or y.size != ny:
                raise ValueError("problem %d: a start holds x of %d and y of %d entries (x_x x_y x_s tau | u v kappa), not %d and %d"
                                 % (int(first) + k, nx, ny, x.size, y.size))
            _start_scalars(x, y, "problem %d: " % (int(first) + k))
            out_x.append(x)
            out_y.append(y)
        return np.concatenate(out_x), np.concatenate(out_y)

    def _set_checked(self, first, count, x, y):
        _checked(self._c("set_iterates"), self.h, int(first), int(count), x.ctypes.data, y.ctypes.data)

    def set_iterates(self, xs, ys, first=0):
        """problems first, first + 1, .. start from the iterates (xs[k], ys[k]) -- each what iterate() returns for a running problem
        or raw_iterate() for any, in the problem's own lengths -- instead of x = 0, y = 0, tau = 1: iteration 0, running, the
        compensation terms zero; the problem's data, norms and preconditioner stay.  One upload and one launch (one per
        workgroup-size class in a ragged batch) for all of them.  ValueError: a wrong length (before anything is uploaded), a tau
        that is negative or not finite, a kappa that is positive or not finite."""
        xs = list(xs)
        x, y = self._iterates(first, xs, ys)
        self._set_checked(first, len(xs), x, y)

    def set_iterate(self, i, x, y):
        """set_iterates for problem i alone"""
        if not 0 <= int(i) < self.n_prob:
            raise ValueError("set_iterate: no problem %r in a batch of %d" % (i, self.n_prob))
        self.set_iterates([x], [y], first=int(i))

    def raw_iterate(self, i):
        """iterate(i) with the read-out's final scaling undone: a problem that stopped with kind 0 in state OK / ExcessIter has its
        x_x and x_y returned divided by tau, and this multiplies them by tau again (exact to one rounding); for a running problem
        it is iterate(i) itself.  It is what set_iterate / replace(start=) expect from a finished solve.  The iteration is
        positively homogeneous, so any positive multiple of the whole (x, y) is an equally valid start."""
        return _raw(self.iterate(i), self.status(i))

    def reinit(self):
        """the family's init again: a fresh solve of every problem"""
        self._c("init")(self.h)

    def set_param(self, param):
        self.param = param
        par = _c_param(param)
        self._c("set_param")(self.h, C.byref(par))

    def _run(self, fn, max_steps, poll_every):
        st = (_lib.Status * self.n_prob)()
        fn(self.h, int(max_steps), int(poll_every), st)
        return [FusedResult(s) for s in st]

    def run(self, max_steps=-1, poll_every=16):
        """every running problem advances by up to max_steps iterations; returns the list of the problems' FusedResult"""
        return self._run(self._c("run"), max_steps, poll_every)

    def run_until_any(self, max_steps=-1, poll_every=16):
        """run(), but back at the first poll that finds stopped a problem that was running when the call began"""
        return self._run(self._c("run_until_any"), max_steps, poll_every)

    def status(self, i):
        st = _lib.Status()
        self._c("status")(self.h, int(i), C.byref(st))
        return FusedResult(st)

    def solution(self, i):
        x = np.empty(self.n, dtype=np.float32)
        y = np.empty(self.m, dtype=np.float32)
        self._c("solution")(self.h, int(i), x.ctypes.data, y.ctypes.data)
        return x, y

    def iterate(self, i):
        x = np.empty(self.n + 2 * self.m + 1, dtype=np.float32)
        y = np.empty(self.n + self.m + 1, dtype=np.float32)
        self._c("iterate")(self.h, int(i), x.ctypes.data, y.ctypes.data)
        return x, y

    def precond(self, i):
        t = np.empty(self.n + 2 * self.m + 1, dtype=np.float32)
        s = np.empty(self.n + self.m + 1, dtype=np.float32)
        self._c("precond")(self.h, int(i), t.ctypes.data, s.ctypes.data)
        return t, s

    def info(self):
        o = self._Info()
        self._c("info")(self.h, C.byref(o))
        return {k: getattr(o, k) for k, _ in self._Info._fields_ if k != "reserved"}

    def solve(self, poll_every=16):
        """Solver::solve semantics per problem: the list of (x, y), or a SolverError for a problem that did not converge"""
        out = []
        for i, r in enumerate(self.run(-1, poll_every)):
            out.append(self.solution(i) if r.state == _lib.ST_OK else SolverError(r.state))
        return out

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def destroy(self):
        if getattr(self, "h", None) is not None:
            self._c("destroy")(self.h)
            self.h = None
        for d in getattr(self, "_owned", []) + [d for own in getattr(self, "_slot_owned", {}).values() for d in own]:
            d.free()
        self._owned, self._slot_owned = [], {}
