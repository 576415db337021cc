"""`BatchSolver`: B problems over the SAME dense f32 A (their own b_i, c_i; one cone layout) iterated in lockstep on the device
(thip_batch_* in include/totsu_f32hip.h) -- a regularisation path, a parameter sweep, a set of scenarios.  One multi-vector launch
forms the products of up to eight instances from one read of A, so an iteration of the batch costs 2 * ceil(B / 8) passes over A
instead of 2 B; everything else is the ordinary fused loop (2-pass carried schedule) on each instance's own state.

The instances are SLOTS: `replace` hands a slot -- running or stopped -- the next problem as a fresh init, `regroup=True` makes the
launches follow the live set (ceil(live / max_group) per pass), and `stream` / `solve_many` push any number of (b, c) through the
slots of one batch, refilling a slot as soon as its problem has stopped."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .fused import Bf16Matrix, DeviceBuffer, FusedResult, _c_param, _checked, _raw, _start_arrays
from .solver import SolverError, SolverParam


def group_sizes(n_inst, max_group=_lib.BATCH_GROUP_DEFAULT):
    """instances per multi-vector launch of one pass (thip_batch_grouping; needs no GPU)"""
    g, mem = C.c_int(), (C.c_int * _lib.BATCH_MAX)()
    lib.thip_batch_grouping(int(n_inst), int(max_group), C.byref(g), mem)
    return [mem[i] for i in range(g.value)]


def live_groups(live, max_group=_lib.BATCH_GROUP_DEFAULT):
    """the regroup rule (thip_batch_live_grouping; needs no GPU): `live` holds one flag per instance; returns the launches of one
    pass as lists of instance indices -- the live ones in ascending order, full groups first and the rest last"""
    live = [1 if v else 0 for v in live]
    n = len(live)
    g, sizes, mem = C.c_int(), (C.c_int * _lib.BATCH_MAX)(), (C.c_int * _lib.BATCH_MAX)()
    lib.thip_batch_live_grouping(n, int(max_group), (C.c_int * max(n, 1))(*live), C.byref(g), sizes, mem)
    out, at = [], 0
    for k in range(g.value):
        out.append([mem[at + j] for j in range(sizes[k])])
        at += sizes[k]
    return out


def stream_slots(batch, problems, poll_every=16, warm=False):
    """The slot-filling policy, over any object with n_inst / run_until_any / replace / solution (a BatchSolver, or a
    stub of one; warm=True also asks it for raw_iterate and replace(start=)).  warm=True: a refilled slot starts from the raw
    iterate its previous occupant ended with when that occupant ended OK, and afresh otherwise -- the choice for a path or a sweep,
    where the next problem is the last one slightly changed; order, laziness and results per problem are those of warm=False.
    The batch's slots hold
    problems 0 .. n_inst - 1 when this starts; the (b, c) of the iterable `problems` -- lazy or unbounded -- are numbered on from
    n_inst.  Whenever run_until_any returns, every slot found stopped is read out and handed the next problem at once; yields
    (k, result, x, y) per finished problem k, in the order they finish.  Ends when the iterable is dry and every slot has stopped."""
    it = iter(problems)
    occupant = list(range(batch.n_inst))           # the problem in each slot; None: read out, and nothing left to put there
    nxt = batch.n_inst
    while any(k is not None for k in occupant):
        res = batch.run_until_any(-1, poll_every)
        done = []
        for i, k in enumerate(occupant):
            r = res[i]
            if k is None or r.state == _lib.ST_RUNNING:
                continue
            x, y = batch.solution(i)
            done.append((k, r, x, y))
            occupant[i] = None
            if it is not None:
                try:
                    vec_b, vec_c = next(it)
                except StopIteration:
                    it = None
                else:
                    if warm and r.state == _lib.ST_OK:
                        batch.replace(i, vec_b, vec_c, start=batch.raw_iterate(i))
                    else:
                        batch.replace(i, vec_b, vec_c)
                    occupant[i], nxt = nxt, nxt + 1
        for d in done:
            yield d


class ManyResults(list):
    """solve_many's return value: (FusedResult, x, y) per problem in input order; .counters / .info: the batch's, at the end"""
    counters = None
    info = None


def solve_many(dense, vecs_b, vecs_c, slots=8, param=None, poll_every=16, warm=False, **kw):
    """Any number (>= 1) of problems (vecs_b[k], vecs_c[k]) over the A and cones of `dense` (Prob*.dense(); its own b / c are not
    used), streamed through one BatchSolver of min(slots, len) slots (slots <= 64) with regroup=True.  Returns the list of
    (FusedResult, x, y) IN INPUT ORDER (a ManyResults).  warm=True: a refilled slot starts from the iterate its previous occupant
    ended with (stream_slots) -- for problems given in an order in which neighbours are alike.  **kw: BatchSolver's (max_group,
    gemv_autotune)."""
    vecs_b, vecs_c = list(vecs_b), list(vecs_c)
    if len(vecs_b) != len(vecs_c):
        raise ValueError("vecs_b and vecs_c differ in length: %d vs %d" % (len(vecs_b), len(vecs_c)))
    if len(vecs_b) < 1:
        raise ValueError("solve_many needs at least one problem")
    if not 1 <= int(slots) <= _lib.BATCH_MAX:
        raise ValueError("slots is 1 .. %d, not %r" % (_lib.BATCH_MAX, slots))
    s = min(int(slots), len(vecs_b))
    kw["regroup"] = True
    bt = BatchSolver.from_dense(dense, vecs_b[:s], vecs_c[:s], param, **kw)
    try:
        out = ManyResults([None] * len(vecs_b))
        for k, r, x, y in bt.stream(zip(vecs_b[s:], vecs_c[s:]), poll_every, warm=warm):
            out[k] = (r, x, y)
        out.counters, out.info = bt.counters(), bt.info()
    finally:
        bt.destroy()
    return out


def kernel_instance(members):
    """the kernel a group of `members` instances runs on: 1 = the single-vector dual GEMV, else NV = 2, 4 or 8"""
    return 1 if members <= 1 else 2 if members <= 2 else 4 if members <= 4 else 8


class BatchSolver:
    def __init__(self, n, m, mat_a, vecs_b, vecs_c, seg_type, seg_len, param=None, vec_b_rowabs=None, a_storage="f32",
                 gemv_autotune=None, max_group=None, regroup=False):
        """mat_a: DeviceBuffer or host array (column-major m x n, dense f32).  vecs_b / vecs_c: one array (or DeviceBuffer) per
        instance.  Refused (ValueError): a sparse or 16-bit A, an a_storage other than "f32", lists of different lengths, vectors
        of the wrong length, no instance or more than 64.  regroup=True: the launches follow the live set (thip_batch_set_regroup)."""
        self.h = None
        self._owned = []
        self._slot_owned = []
        if hasattr(mat_a, "tocsr") or isinstance(mat_a, Bf16Matrix) or type(mat_a).__name__ == "SpTile":
            raise ValueError("BatchSolver streams a dense f32 A: sparse and 16-bit matrices are not taken")
        if a_storage != "f32":
            raise ValueError("BatchSolver streams A in f32 only (a_storage=%r)" % (a_storage,))
        if len(vecs_b) != len(vecs_c):
            raise ValueError("vecs_b and vecs_c differ in length: %d vs %d" % (len(vecs_b), len(vecs_c)))
        if not 1 <= len(vecs_b) <= _lib.BATCH_MAX:
            raise ValueError("a batch holds 1 .. %d instances, not %d" % (_lib.BATCH_MAX, len(vecs_b)))
        self.n, self.m, self.n_inst = int(n), int(m), len(vecs_b)
        for name, vs, want in (("vecs_b", vecs_b, self.m), ("vecs_c", vecs_c, self.n)):
            for v in vs:
                self._check_len(name, v, want)
        if not isinstance(mat_a, DeviceBuffer) and np.asarray(mat_a).size != self.n * self.m:
            raise ValueError("mat_a: %d entries where m * n = %d are needed" % (np.asarray(mat_a).size, self.n * self.m))
        _lib.ensure_init()
        self.mat_a = self._dev(mat_a)
        self.vecs_b, self.vecs_c = [], []
        for vb, vc in zip(vecs_b, vecs_c):
            own = []                                # what the batch uploaded for this slot: freed when the slot is replaced
            self.vecs_b.append(self._dev(vb, own))
            self.vecs_c.append(self._dev(vc, own))
            self._slot_owned.append(own)
        self.vec_b_rowabs = None if vec_b_rowabs is None else self._dev(vec_b_rowabs)
        self.param = param or SolverParam()
        self._st = np.ascontiguousarray(seg_type, dtype=np.int32)
        self._sl = np.ascontiguousarray(seg_len, dtype=np.int64)
        prob = _lib.Problem(self.n, self.m, self.mat_a.ptr, None, None, None if self.vec_b_rowabs is None else self.vec_b_rowabs.ptr,
                            len(self._st), self._st.ctypes.data_as(C.POINTER(C.c_int32)), self._sl.ctypes.data_as(C.POINTER(C.c_int64)))
        pb = (C.c_void_p * self.n_inst)(*[v.ptr for v in self.vecs_b])
        pc = (C.c_void_p * self.n_inst)(*[v.ptr for v in self.vecs_c])
        par = _c_param(self.param)
        h = C.c_void_p()
        lib.thip_batch_create(C.byref(prob), self.n_inst, pb, pc, C.byref(par), C.byref(h))
        self.h = h
        if gemv_autotune is not None:
            lib.thip_batch_set_gemv_autotune(self.h, 1 if gemv_autotune else 0)     # False: bit-reproducible across runs
        if max_group is not None:
            lib.thip_batch_set_max_group(self.h, int(max_group))
        if regroup:
            lib.thip_batch_set_regroup(self.h, 1)
        lib.thip_batch_init(self.h)

    @staticmethod
    def from_dense(d, vecs_b, vecs_c, param=None, **kw):
        """the stacked description of Prob*.dense() for A and the cones; its own vec_b / vec_c are not used"""
        return BatchSolver(d.n, d.m, d.mat_a, vecs_b, vecs_c, d.seg_type, d.seg_len, param, **kw)

    @staticmethod
    def _check_len(name, v, want):
        got = v.n if isinstance(v, DeviceBuffer) else np.asarray(v).size
        if (got < want) if isinstance(v, DeviceBuffer) else (got != want):
            raise ValueError("%s: a vector of %d entries where %d are needed" % (name, got, want))

    def _dev(self, a, owned=None):
        if isinstance(a, DeviceBuffer):
            return a
        d = DeviceBuffer.from_host(a)
        (self._owned if owned is None else owned).append(d)
        return d

    def replace(self, i, vec_b, vec_c, start=None):
        """slot i -- running or stopped -- takes the problem (vec_b, vec_c) (host arrays or DeviceBuffers) as a fresh init; no
        other instance is touched.  What the batch had uploaded for the slot's previous problem is freed after the call.
        start: None, or the (x, y) the new problem starts from (replace, then set_iterate)."""
        if vec_b is None or vec_c is None:
            raise ValueError("replace: vec_b and vec_c are needed")
        if not 0 <= int(i) < self.n_inst:
            raise ValueError("replace: no slot %r in a batch of %d" % (i, self.n_inst))
        self._check_len("vec_b", vec_b, self.m)
        self._check_len("vec_c", vec_c, self.n)
        if start is not None:
            start = _start_arrays(self.n, self.m, *start)
        i, own = int(i), []
        try:
            db, dc = self._dev(vec_b, own), self._dev(vec_c, own)
            lib.thip_batch_replace(self.h, i, db.ptr, dc.ptr)
        except Exception:
            for d in own:
                d.free()
            raise
        old, self._slot_owned[i] = self._slot_owned[i], own
        self.vecs_b[i], self.vecs_c[i] = db, dc
        for d in old:
            d.free()
        if start is not None:
            _checked(lib.thip_batch_set_iterate, self.h, i, start[0].ctypes.data, start[1].ctypes.data)

    def set_iterate(self, i, x, y):
        """slot i goes on from the iterate (x, y) -- what iterate(i) returns for a running instance, or raw_iterate(i) for any --
        instead of x = 0, y = 0, tau = 1: iteration 0, running, the compensation terms zero; b, c, the norms and the
        preconditioner stay.  Costs one single-vector pass over A (the slot's carried products).  ValueError: a wrong length
        (before anything is uploaded), a tau that is negative or not finite, a kappa that is positive or not finite."""
        if not 0 <= int(i) < self.n_inst:
            raise ValueError("set_iterate: no slot %r in a batch of %d" % (i, self.n_inst))
        x, y = _start_arrays(self.n, self.m, x, y)
        _checked(lib.thip_batch_set_iterate, self.h, int(i), x.ctypes.data, y.ctypes.data)

    def raw_iterate(self, i):
        """iterate(i) with the read-out's final scaling undone (FusedSolver.raw_iterate): what set_iterate expects from a finished solve"""
        return _raw(self.iterate(i), self.status(i))

    def reinit(self):
        """thip_batch_init again: a fresh solve of every instance"""
        lib.thip_batch_init(self.h)

    def set_param(self, param):
        self.param = param
        par = _c_param(param)
        lib.thip_batch_set_param(self.h, C.byref(par))

    def run(self, max_steps=-1, poll_every=16):
        """every running instance advances by up to max_steps iterations; returns the list of the instances' FusedResult"""
        st = (_lib.Status * self.n_inst)()
        lib.thip_batch_run(self.h, int(max_steps), int(poll_every), st)
        return [FusedResult(s) for s in st]

    def run_until_any(self, max_steps=-1, poll_every=16):
        """run(), but back at the first poll that finds stopped an instance that was running when the call began"""
        st = (_lib.Status * self.n_inst)()
        lib.thip_batch_run_until_any(self.h, int(max_steps), int(poll_every), st)
        return [FusedResult(s) for s in st]

    def stream(self, problems, poll_every=16, warm=False):
        """generator: the batch's own problems (k = 0 .. n_inst - 1) and then those of the iterable `problems` of (b, c) (k counts
        on), each slot refilled as soon as its problem has stopped; yields (k, FusedResult, x, y) as they finish (stream_slots).
        warm=True: a refilled slot starts from the iterate its previous occupant ended with"""
        return stream_slots(self, problems, poll_every, warm=warm)

    def counters(self):
        """what run / run_until_any have issued since the last init: launches by kernel instance {1, 2, 4, 8}, passes over A,
        instance_iterations (retired occupants included), replaced, live and groups_now as of the last poll"""
        o = _lib.BatchCounters()
        lib.thip_batch_counters(self.h, C.byref(o))
        d = {k: getattr(o, k) for k in ("passes", "instance_iterations", "replaced", "live", "groups_now")}
        d["launches"] = {nv: o.launches[q] for q, nv in enumerate((1, 2, 4, 8))}
        return d

    def status(self, i):
        st = _lib.Status()
        lib.thip_batch_status(self.h, int(i), C.byref(st))
        return FusedResult(st)

    def solution(self, i):
        x = np.empty(self.n, dtype=np.float32)
        y = np.empty(self.m, dtype=np.float32)
        lib.thip_batch_solution(self.h, int(i), x.ctypes.data, y.ctypes.data)
        return x, y

    def iterate(self, i):
        x = np.empty(self.n + 2 * self.m + 1, dtype=np.float32)
        y = np.empty(self.n + self.m + 1, dtype=np.float32)
        lib.thip_batch_iterate(self.h, int(i), x.ctypes.data, y.ctypes.data)
        return x, y

    def precond(self, i):
        t = np.empty(self.n + 2 * self.m + 1, dtype=np.float32)
        s = np.empty(self.n + self.m + 1, dtype=np.float32)
        lib.thip_batch_precond(self.h, int(i), t.ctypes.data, s.ctypes.data)
        return t, s

    def info(self):
        o = _lib.BatchInfo()
        lib.thip_batch_info(self.h, C.byref(o))
        d = {k: getattr(o, k) for k in ("n_inst", "max_group", "groups", "passes_per_iteration", "a_copies", "a_bytes",
                                        "bytes_per_pass", "arena_bytes", "device_bytes")}
        d["group_sizes"] = group_sizes(self.n_inst, o.max_group)
        d["plans"] = {nv: {"rows_groups_per_lane": o.plan_nj[q], "target_workgroups": o.plan_blocks[q], "autotune_ms": o.plan_ms[q]}
                      for q, nv in ((1, 2), (2, 4), (3, 8))}
        return d

    def pin_multi_plan(self, instance, candidate_index):
        """TEST HOOK (thip_test_batch_pin_multi_plan): the tiling of the multi-vector kernel instance NV = 2, 4 or 8 pinned to a
        candidate of its autotune (-1: untuned again); after init, before the first run"""
        lib.thip_test_batch_pin_multi_plan(self.h, int(instance), int(candidate_index))

    def last_multi_plan(self, instance):
        """TEST HOOK (thip_test_batch_last_multi_plan): the plan record of the latest launch of that kernel instance, as a dict
        (all zeros: not launched yet)"""
        rec = _lib.GemvPlanRec()
        lib.thip_test_batch_last_multi_plan(self.h, int(instance), C.byref(rec))
        return {k: getattr(rec, k) for k, _ in rec._fields_}

    def solve(self, poll_every=16):
        """Solver::solve semantics per instance: the list of (x, y), or a SolverError for an instance that did not converge"""
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
            lib.thip_batch_destroy(self.h)
            self.h = None
        for d in getattr(self, "_owned", []) + [d for own in getattr(self, "_slot_owned", []) for d in own]:
            d.free()
        self._owned, self._slot_owned = [], []
