"""What the own-A batch solvers share -- `SmallBatchSolver` (A in LDS), `MidBatchSolver` (A streamed) and `SdpBatchSolver` (A
streamed, PSD cones projected on chip): many conic programs of one shape n, m and one cone layout, each with its OWN dense f32 A,
one workgroup per problem, a launch advancing every running problem by poll_every iterations (the generic C API of
totsu_amd/csrc/thip_ownbatch.h).  `OwnBatchSolver` is the whole host side; a family is a subclass that names its prefix of the C
API, its test hook, its word for the ValueErrors and its info record.  `_fits` is the shape rule of a family by prefix,
`first_that_takes` the chooser over an ordered list of families."""
import ctypes as C

import numpy as np

from . import _lib, devmem
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


def pack_bc(n_prob, shape_of, vecs_b, vecs_c, vecs_b_rowabs=None, first=0):
    """the arrays thip_NAME_set_bc takes (needs no handle and no GPU): (count, b, c, rowabs or None, has or None) for the problems
    first, first + 1, .. of a batch of n_prob whose problem i has the shape shape_of(i) = (n_i, m_i).  b: every vecs_b[k] one after
    another as float32, c likewise; rowabs: m floats for every problem (zeros where vecs_b_rowabs[k] is None), or None when
    vecs_b_rowabs is None or every entry of it is; has: one byte per problem, 1 where the problem has row sums, or None when all or
    none have.  ValueError: no problem, lists of different lengths, a range outside the batch, a vector of the wrong length (the
    message names the problem)"""
    vecs_b, vecs_c = list(vecs_b), list(vecs_c)
    count, first = len(vecs_b), int(first)
    if count < 1 or len(vecs_c) != count:
        raise ValueError("set_bc: %d b where there are %d c (one pair per problem, at least one)" % (count, len(vecs_c)))
    rows = [None] * count if vecs_b_rowabs is None else list(vecs_b_rowabs)
    if len(rows) != count:
        raise ValueError("set_bc: %d vecs_b_rowabs where there are %d b (one entry per problem, None: |b|)" % (len(rows), count))
    if not 0 <= first <= first + count <= int(n_prob):
        raise ValueError("set_bc: no problems %r .. %r in a batch of %d" % (first, first + count - 1, n_prob))
    bs, cs, rs, has = [], [], [], np.zeros(count, dtype=np.uint8)
    for k, (b, c, r) in enumerate(zip(vecs_b, vecs_c, rows)):
        n, m = shape_of(first + k)
        b, c = np.ascontiguousarray(b, dtype=np.float32).ravel(), np.ascontiguousarray(c, dtype=np.float32).ravel()
        if b.size != m or c.size != n:
            raise ValueError("problem %d: b holds %d and c %d entries where m = %d and n = %d are needed" % (first + k, b.size, c.size, m, n))
        if r is None:
            r = np.zeros(m, dtype=np.float32)
        else:
            r = np.ascontiguousarray(r, dtype=np.float32).ravel()
            if r.size != m:
                raise ValueError("problem %d: vec_b_rowabs holds %d entries where m = %d are needed" % (first + k, r.size, m))
            has[k] = 1
        bs.append(b)
        cs.append(c)
        rs.append(r)
    b, c = np.concatenate(bs), np.concatenate(cs)
    if not has.any():
        return count, b, c, None, None
    return count, b, c, np.concatenate(rs), None if has.all() else has


def pack_a(n_prob, size_of, mats_a, first=0, values_of=None):
    """the arrays thip_NAME_set_a takes (needs no handle and no GPU): (count, values, counts) for the problems first, first + 1, ..
    of a batch of n_prob whose problem i takes size_of(i) values -- m_i n_i of a dense A (column-major), the entries of a sparse
    problem's present pattern (CSC order).  mats_a: one host array per problem, or a 2-D array of one row per problem.  values:
    every problem's values one after another as float32; counts: how many each brings, int64.  values_of(i, item): what a family
    makes of an item that is no plain array (a sparse family's triple or scipy matrix, whose pattern it compares).  ValueError,
    all before anything is uploaded: no problem, a range outside the batch, a wrong length (the message names the problem), a
    value that is not finite"""
    first = int(first)
    whole = mats_a if isinstance(mats_a, np.ndarray) and mats_a.ndim == 2 and mats_a.dtype != object else None
    mats_a = list(mats_a)
    count = len(mats_a)
    if count < 1:
        raise ValueError("set_a: no problem (one array of values per problem, at least one)")
    if not 0 <= first <= first + count <= int(n_prob):
        raise ValueError("set_a: no problems %r .. %r in a batch of %d" % (first, first + count - 1, n_prob))
    if whole is not None and all(int(size_of(first + k)) == whole.shape[1] for k in range(count)):
        with np.errstate(over="ignore"):    # one row per problem, every length right: one conversion and one check for all
            v = np.ascontiguousarray(whole, dtype=np.float32)
        if np.isfinite(v).all():
            return count, v.ravel(), np.full(count, whole.shape[1], dtype=np.int64)
    out = []
    for k, a in enumerate(mats_a):
        if values_of is not None:
            a = values_of(first + k, a)
        with np.errstate(over="ignore"):        # (a value too large for float32 becomes inf and is refused below)
            a = np.ascontiguousarray(a, dtype=np.float32).ravel()
        want = int(size_of(first + k))
        if a.size != want:
            raise ValueError("problem %d: %d values of A where %d are needed%s"
                             % (first + k, a.size, want, "" if values_of is None else " (the slot's entry count; another pattern is replace's)"))
        if not np.isfinite(a).all():
            raise ValueError("problem %d: a value of A is not finite" % (first + k))
        out.append(a)
    counts = np.array([a.size for a in out], dtype=np.int64)
    return count, np.ascontiguousarray(np.concatenate(out), dtype=np.float32), counts


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
            self._create(self.n, self.m, self.n_prob, self.mats_a.ptr, self.vecs_b.ptr, self.vecs_c.ptr,
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

    def _create(self, *args):
        """the family's create call on the arguments of thip_NAME_create (a family whose create takes more overrides this)"""
        self._c("create")(*args)

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

    def _nm(self, i):
        """problem i's own (n, m)"""
        return self.n, self.m

    def set_bc(self, vecs_b, vecs_c, vecs_b_rowabs=None, first=0, keep_iterate=False):
        """problems first, first + 1, .. take the new vecs_b[k], vecs_c[k] (lists or 2-D arrays of host vectors, each in the problem's
        own m / n) and KEEP their A, which stays on the device: one upload, one launch (one per workgroup-size class in a ragged
        batch) and one read of the status blocks for all of them.  vecs_b_rowabs: None, or a list whose entries may each be None
        (|b| of the new b).  keep_iterate=False: each problem ends exactly as replace(i, its present A, b, c, rowabs) leaves it --
        a fresh init, iteration 0, running.  keep_iterate=True: the preconditioner and norms of the new data, and the iterate as it
        lies on the device kept (x_x x_y x_s tau | u v kappa, no read-out scaling; the compensation terms zero): iteration 0 and
        running again, whether the problem was running or had stopped -- a warm start of every problem of the range without
        reading an iterate out.  The first call allocates the batch's own store of b, c and row sums on the device (info()'s
        device_bytes).  ValueError: a wrong length (before anything is uploaded; the message names the problem), a range outside
        the batch."""
        count, b, c, r, has = pack_bc(self.n_prob, self._nm, vecs_b, vecs_c, vecs_b_rowabs, first)
        _checked(self._c("set_bc"), self.h, int(first), count, b.ctypes.data, c.ctypes.data, None if r is None else r.ctypes.data,
                 None if has is None else has.ctypes.data, 1 if keep_iterate else 0)

    def _a_size(self, i):
        """how many values problem i's A holds: m n here, the present pattern's entries in a sparse family"""
        n, m = self._nm(i)
        return n * m

    _a_values = None        # (a sparse family: what it makes of a triple or a scipy matrix)

    def set_a(self, mats_a, first=0, keep_iterate=False):
        """problems first, first + 1, .. take NEW VALUES of A and keep their shape, cone layout, b, c and row sums: one call, one
        launch (one per workgroup-size class in a ragged batch) and one read of the status blocks for all of them.  mats_a: one
        host array per problem -- the problem's own m n floats, column-major, as replace takes them (a 2-D array of one row per
        problem where the shapes are uniform); in a sparse family the values in the CSC order of the slot's present pattern, or a
        (colptr, rowidx, values) triple or scipy.sparse matrix of exactly that pattern.  A dense A is OVERWRITTEN IN PLACE on the
        device, in the memory the slot reads it from (the batch's own upload, or the DeviceBuffer the caller handed in); nothing
        is allocated.  keep_iterate=False: each problem ends exactly as replace(i, new A, its present b, c, rowabs) leaves it.
        keep_iterate=True: the preconditioner and norms of the new data and the iterate as it lies on the device kept (the
        compensation terms zero; what a streamed family carries formed again): iteration 0 and running again, whether the problem
        was running or had stopped; followed by set_bc(.., keep_iterate=True) it is a round that moves A, b and c.  b, c and the
        row sums are the slot's present ones (after a set_bc: those).  ValueError, before anything is uploaded or touched: a wrong
        length (the message names the problem), a value that is not finite, a range outside the batch, another pattern (that is
        replace's)."""
        count, v, counts = pack_a(self.n_prob, self._a_size, mats_a, first, self._a_values)
        _checked(self._c("set_a"), self.h, int(first), count, v.ctypes.data, counts.ctypes.data, 1 if keep_iterate else 0)

    def _range(self, first, count):
        first = int(first)
        count = self.n_prob - first if count is None else int(count)
        if not (0 <= first and 1 <= count and first + count <= self.n_prob):
            raise ValueError("no problems %r .. %r in a batch of %d" % (first, first + count - 1, self.n_prob))
        return first, count

    def solutions(self, first=0, count=None):
        """[solution(i) for the problems first .. first + count - 1] (count None: to the end), bit for bit, in one read-out: a
        kernel gathers every x and y of the range into one buffer, which comes down in one copy beside the status blocks"""
        first, count = self._range(first, count)
        shapes = [self._nm(first + k) for k in range(count)]
        x = np.empty(sum(n for n, _ in shapes), dtype=np.float32)
        y = np.empty(sum(m for _, m in shapes), dtype=np.float32)
        _checked(self._c("solutions"), self.h, first, count, x.ctypes.data, y.ctypes.data, None)
        out, ox, oy = [], 0, 0
        for n, m in shapes:
            out.append((x[ox:ox + n].copy(), y[oy:oy + m].copy()))
            ox, oy = ox + n, oy + m
        return out

    def statuses(self, first=0, count=None):
        """[status(i) for the problems first .. first + count - 1] (count None: to the end) from one copy of their status blocks"""
        first, count = self._range(first, count)
        st = (_lib.Status * count)()
        _checked(self._c("solutions"), self.h, first, count, None, None, st)
        return [FusedResult(s) for s in st]

    # ---- the round calls on device memory: the four above for a caller whose round lives on the GPU ------------------------------

    def _dev_arg(self, obj, what, want, torch_seen, out=False, typestr="<f4"):
        """the address of the device array `obj`, which holds at least `want` elements (ValueError before the call says what was needed)"""
        ptr, got = devmem.as_device(obj, what, out=out, typestr=typestr)
        if got < want:
            raise ValueError("%s: %d entries where %d are needed (the problems' parts one after another, each in its own length)"
                             % (what, got, want))
        if devmem.is_torch(obj):
            torch_seen.append(obj)
        return ptr

    @staticmethod
    def _torch_ordered(torch_seen):
        """a torch tensor's producer ran on torch's current stream and the library runs on its own: that stream first"""
        if torch_seen:
            import torch
            torch.cuda.current_stream(torch_seen[0].device).synchronize()

    def _sums(self, first, count):
        """the lengths of the range's packed arrays: (c / solution x, b / solution y, iterate x, iterate y) summed over its problems"""
        sn = sm = sx = sy = 0
        for k in range(count):
            n, m = self._nm(first + k)
            nx, ny = self._lengths(first + k)
            sn, sm, sx, sy = sn + n, sm + m, sx + nx, sy + ny
        return sn, sm, sx, sy

    def set_bc_dev(self, b, c, b_rowabs=None, first=0, count=None, keep_iterate=False):
        """set_bc with the new data taken from DEVICE memory -- a DeviceBuffer, a torch tensor on the GPU, anything with
        __cuda_array_interface__: float32, the problems' b one after another (each its own m), c likewise (n), b_rowabs m per
        problem or None.  The range is left bit for bit as set_bc leaves it when handed the same floats; nothing but a table of a
        few dozen bytes per problem goes up.  ValueError: as set_bc, and an array that is too short, of another dtype, not
        contiguous, on the host, or overlapping memory the batch owns."""
        first, count = self._range(first, count)
        sn, sm, _, _ = self._sums(first, count)
        seen = []
        pb, pc = self._dev_arg(b, "set_bc_dev: b", sm, seen), self._dev_arg(c, "set_bc_dev: c", sn, seen)
        pr = None if b_rowabs is None else self._dev_arg(b_rowabs, "set_bc_dev: b_rowabs", sm, seen)
        self._torch_ordered(seen)
        _checked(self._c("set_bc_dev"), self.h, first, count, pb, pc, pr, None, 1 if keep_iterate else 0)

    def set_a_dev(self, values=None, first=0, count=None, keep_iterate=False):
        """set_a with the new values taken from DEVICE memory: the problems' values one after another -- m n floats each,
        column-major, in a dense family (copied device to device into the memory the slots read, in place); the entries in the CSC
        order of each slot's present pattern in a sparse one (read where they lie).  values=None, a dense family only: the caller
        has ALREADY rewritten A in the buffer the batch was built over, nothing is copied and the batch initialises again from
        what lies there -- the zero-copy form; a `values` that overlaps that buffer is refused (write None).  Bit for bit what
        set_a does with the same floats.  ValueError, the batch unchanged: a value that is not finite (found by a kernel before
        anything is touched; the message names the problem), an array that is too short, of another dtype, not contiguous, on the
        host, or overlapping memory the batch owns."""
        first, count = self._range(first, count)
        seen = []
        pv = None
        if values is not None:
            pv = self._dev_arg(values, "set_a_dev: values", sum(int(self._a_size(first + k)) for k in range(count)), seen)
        self._torch_ordered(seen)
        _checked(self._c("set_a_dev"), self.h, first, count, pv, 1 if keep_iterate else 0)

    def set_iterates_dev(self, x, y, first=0, count=None):
        """set_iterates with the iterates taken from DEVICE memory: x the problems' (x_x x_y x_s tau) one after another, y their
        (u v kappa), in the lengths iterate() returns.  Bit for bit what set_iterates does with the same floats.  ValueError, the
        batch unchanged: a tau that is negative or not finite, a kappa that is positive or not finite (found by a kernel; the
        message names the problem), and what set_bc_dev refuses of an array."""
        first, count = self._range(first, count)
        _, _, sx, sy = self._sums(first, count)
        seen = []
        px, py = self._dev_arg(x, "set_iterates_dev: x", sx, seen), self._dev_arg(y, "set_iterates_dev: y", sy, seen)
        self._torch_ordered(seen)
        _checked(self._c("set_iterates_dev"), self.h, first, count, px, py)

    def solutions_dev(self, first=0, count=None, out_x=None, out_y=None, out_state=None, sync=True):
        """solutions() left ON THE DEVICE: (x, y, state) -- the problems' x one after another (each its own n), their y (m), and one
        int32 state code per problem -- bit for bit what solutions() and statuses() return, the final 1/tau scaling applied by the
        kernel.  out_x / out_y / out_state: where to write (float32, float32, int32 device arrays, or a DeviceBuffer for any; long
        enough), else freshly allocated DeviceBuffers (the state's 4-byte words are int32: to_host().view(numpy.int32)).  Nothing
        comes to the host.  sync=True waits for the library's stream before returning; sync=False returns after the launch, and
        the caller orders its readers behind that stream."""
        first, count = self._range(first, count)
        sn, sm, _, _ = self._sums(first, count)
        seen = []
        x = DeviceBuffer(sn) if out_x is None else out_x
        y = DeviceBuffer(sm) if out_y is None else out_y
        st = DeviceBuffer(count) if out_state is None else out_state
        px = self._dev_arg(x, "solutions_dev: out_x", sn, seen, out=True)
        py = self._dev_arg(y, "solutions_dev: out_y", sm, seen, out=True)
        ps = self._dev_arg(st, "solutions_dev: out_state", count, seen, out=True, typestr="<i4")
        self._torch_ordered(seen)
        _checked(self._c("solutions_dev"), self.h, first, count, px, py, ps)
        if sync:
            lib.thip_sync()
        return x, y, st

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
