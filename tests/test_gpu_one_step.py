"""GPU: ONE iteration of every solver loop -- the single solver's four schedules over every stored form of A, the shared-A batch,
the own-A families (the mid batch also over both 16-bit copies of A) at every workgroup size their test hooks force -- from starts deep in a solve, held to the componentwise
f32 bound of tests/step_bound.py (validated on the CPU by tests/test_step_bound_cpu.py): set_iterate, run(1, poll_every=1),
iterate, check.  The bound does not grow with the iteration count and is relative to each component's own terms, not to the
iterate's max norm; the inputs have rows and columns scaled over 10^+-3, and the starts are the f64 iterates after 9, 99 and 999
iterations and the iterates around tau's first clamp to 0 of the tau -> 0 families.  Every case first asserts the path that ran
and prints the worst ratio |d| / (EPS B) per vector (allowed: 1 for x, 3 for y)."""
import numpy as np
import pytest

import step_bound as SB
import test_gpu_tau_zero as TZ
from mid16_cases import widened_of
from ownbatch_cases import F, T  # noqa: F401  (T: the fixture)

pytestmark = pytest.mark.gpu

ARITH = ["plain", "compensated"]
PASSES = {"reference": 6, "fused": 3, "carried": 2, "sweep": 1}      # over a dense A (the reference schedule: two single GEMVs per stage)
STAGES = {"reference": 3, "fused": 3, "carried": 2, "sweep": 1}


def _param(T, arith):
    p = T.SolverParam()
    p.eps_acc = p.eps_inf = 1e-30
    p.state_arith = arith
    return p


def _worst(into, ratios):
    for k, v in ratios.items():
        into[k] = max(into.get(k, 0.0), v)


# ---- the single solver ------------------------------------------------------------------------------------------------------------

DENSE = ["lp80x40s", "socp102x12s", "layout_small_s", "sdp45x6"]
SOLVER_CASES = [(n, "dense", "f32", s) for n in DENSE for s in ("reference", "fused", "carried")] + \
               [("lp2504x1252s", "dense", "f32", s) for s in ("fused", "carried", "sweep")] + \
               [("lp2504x1252s", "dense", a, "sweep") for a in ("bf16", "f16")] + \
               [("sp40x30s", f, "f32", s) for f in ("tiled", "csr2") for s in ("fused", "carried")] + [("sp40x30s", "tiled", "f32", "sweep")]


def _up(v, k):
    return (v + k - 1) // k * k


_WIDE = {}


def _widened(T, d, kind):
    """d over the matrix its 16-bit stored form decodes to: the library's own conversion, read back and decoded, as
    tests/test_gpu_gemv_tilings.py::Stored does (bit-exactness of the conversion: tests/test_gpu_bf16.py)"""
    key = (d.name, d.seed, kind)
    if key not in _WIDE:
        from totsu_amd._lib import lib
        m, n = d.m, d.n
        ld = _up(m, 16)
        src = T.DeviceBuffer.from_host(np.ascontiguousarray(d.mat_a, dtype=F))
        dst = T.DeviceBuffer((ld * n + 1) // 2 + 4, zero=True)
        inv = None
        if kind == "bf16":
            lib.thip_to_bf16(m, n, src.ptr, dst.ptr, ld)
        else:
            inv = T.DeviceBuffer(n)
            lib.thip_to_f16(m, n, src.ptr, dst.ptr, ld, inv.ptr)
        bits = dst.to_host().view(np.uint16)[:ld * n].reshape((n, ld))
        assert not bits[:, m:].any()
        if kind == "bf16":
            dec = (bits[:, :m].astype(np.uint32) << 16).view(np.float32)
        else:
            s = inv.to_host()
            assert np.all(np.log2(s.astype(np.float64)) % 1 == 0)          # powers of two: the scaling is exact
            dec = (bits[:, :m].view(np.float16).astype(np.float64) * s.astype(np.float64)[:, None]).astype(F)
            inv.free()
        src.free()
        dst.free()
        _WIDE[key] = SB.with_matrix(d, dec)
    return _WIDE[key]


def _make_solver(T, d, p, schedule, form, a_storage):
    mat = d.mat_a
    if form != "dense":
        import scipy.sparse as sp
        mat = sp.csr_matrix(np.asarray(d.mat_a, F).reshape(d.n, d.m).T)
    return T.FusedSolver(d.n, d.m, mat, d.vec_b, d.vec_c, d.seg_type, d.seg_len, p, schedule, vec_b_rowabs=d.vec_b_rowabs,
                         gemv_autotune=False, sweep_min_bytes=0, sparse_two_copies=form == "csr2", a_storage=a_storage)


def _assert_solver_path(fs, d, schedule, form, a_storage):
    assert fs.schedule_in_use() == schedule, (schedule, fs.schedule_in_use())
    assert fs.a_storage == a_storage
    passes, bpp = fs.passes()
    nnz = int(np.count_nonzero(np.asarray(d.mat_a)))
    if form == "dense":
        assert fs.a_layout == "dense" and fs._spt is None and fs._csr is None
        assert passes == PASSES[schedule] and bpp == d.m * d.n * (4 if a_storage == "f32" else 2), (passes, bpp)
    elif form == "csr2":                                       # a stage reads the two CSR copies once: 2 nnz (value, index) pairs
        assert fs._csr is not None and fs._spt is None
        assert passes == STAGES[schedule] and bpp == 16 * nnz, (passes, bpp)
    else:                                                      # of the tiled copy every product is one pass over the stored entries
        assert fs._spt is not None and fs._csr is None and fs.a_layout == "tiled" and fs.sptile_info()["nnz"] == nnz, fs.sptile_info()
        assert passes == 2 * STAGES[schedule], (schedule, passes)
    return "%s, %s A in %s, %d passes of %d bytes" % (fs.schedule_in_use(), form, a_storage, passes, bpp)


def _one_step(fs, ref, st):
    """set_iterate, one iteration, iterate -> check against the problem `ref`"""
    fs.set_iterate(*st)
    fs.run(1, poll_every=1)
    x, y = fs.iterate()
    s = fs.status()
    assert s.state == -1 and s.iters == 1, (s.state, s.iters)
    return SB.check(ref, st, x, y, s.kind, tuple(s.cri))


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("name,form,a_storage,schedule", SOLVER_CASES)
def test_solver_one_step(T, name, form, a_storage, schedule, arith):
    d = SB.problem(name)
    ref = d if a_storage == "f32" else _widened(T, d, a_storage)
    fs = _make_solver(T, d, _param(T, arith), schedule, form, a_storage)
    try:
        path = _assert_solver_path(fs, d, schedule, form, a_storage)
        worst = {}
        for k in SB.ks_of(name):
            ratios = _one_step(fs, ref, SB.start(name, k))
            assert fs.schedule_in_use() == schedule
            print("one step solver %s %s k=%d: %s" % (name, arith, k, SB.fmt(ratios)))
            _worst(worst, ratios)
        print("one step solver %s %s [%s] worst: %s" % (name, arith, path, SB.fmt(worst)))
    finally:
        fs.destroy()


# ---- the tau -> 0 starts on every leg tests/test_gpu_tau_zero.py selects -------------------------------------------------------------

TZ_CASES = [(leg, fam) for leg, fam in TZ.CASES if fam in SB.TAU_ZERO]


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("leg,fam_name", TZ_CASES)
def test_solver_one_step_around_tau_zero(T, leg, fam_name, arith):
    fam = TZ.Z.family(fam_name)
    d = SB.problem(fam_name)
    a_storage = TZ.LEGS[leg][1]
    ref = d if a_storage == "f32" else _widened(T, d, a_storage)
    fs = TZ._solver(T, leg, fam, _param(T, arith))
    try:
        TZ._assert_path(fs, leg, fam)
        worst = {}
        for label, it, st in SB.tau_zero_starts(fam_name):
            ratios = _one_step(fs, ref, st)
            x, _ = fs.iterate()
            print("one step solver %s/%s %s from `%s` (iterate %d, tau %.3e -> %.3e): %s" % (leg, fam_name, arith, label, it, st[0][-1], x[-1], SB.fmt(ratios)))
            _worst(worst, ratios)
        TZ._assert_mtail(fs, leg, fam)
        print("one step solver %s/%s %s worst: %s" % (leg, fam_name, arith, SB.fmt(worst)))
    finally:
        fs.destroy()


# ---- the shared-A batch -----------------------------------------------------------------------------------------------------------

def _batch_step(bt, i, ref, st):
    x, y = bt.iterate(i)
    s = bt.status(i)
    assert s.state == -1 and s.iters == 1, (i, s.state, s.iters)
    return SB.check(ref, st, x, y, s.kind, tuple(s.cri)), (x, y)


@pytest.mark.parametrize("arith", ARITH)
def test_batch_one_step(T, arith):
    name = "lp80x40s"
    d = SB.problem(name)
    bt = T.BatchSolver.from_dense(d, [d.vec_b] * 3, [d.vec_c] * 3, _param(T, arith), gemv_autotune=False)
    try:
        assert bt.info()["group_sizes"] == [3] and bt.info()["n_inst"] == 3
        starts = [SB.start(name, k) for k in SB.KS]                  # every slot its own start
        for i, st in enumerate(starts):
            bt.set_iterate(i, *st)
        bt.run(1, poll_every=1)
        worst, first = {}, []
        for i, st in enumerate(starts):
            ratios, got = _batch_step(bt, i, d, st)
            print("one step batch %s slot %d k=%d: %s" % (arith, i, SB.KS[i], SB.fmt(ratios)))
            _worst(worst, ratios)
            first.append(got)
        # slot 1 is set again, to another start: its neighbours' results do not move
        again = [starts[0], starts[2], starts[2]]
        for i, st in enumerate(again):
            bt.set_iterate(i, *st)
        bt.run(1, poll_every=1)
        for i, st in enumerate(again):
            ratios, got = _batch_step(bt, i, d, st)
            _worst(worst, ratios)
            if i != 1:
                assert np.array_equal(got[0], first[i][0]) and np.array_equal(got[1], first[i][1]), i
        print("one step batch %s [3 slots in one group] worst: %s" % (arith, SB.fmt(worst)))
    finally:
        bt.destroy()


@pytest.mark.parametrize("arith", ARITH)
def test_batch_one_step_around_tau_zero(T, arith):
    """F6's three slots over one A, the bounded one at its iterate 9, the other two around their first clamp"""
    fams = TZ.Z.family("F6")
    ds = [SB.problem(f.name) for f in fams]
    bt = T.BatchSolver.from_dense(TZ._dense(fams[0]), [f.vec_b for f in fams], [f.vec_c for f in fams], _param(T, arith), gemv_autotune=False)
    try:
        assert bt.info()["group_sizes"] == [3]
        worst = {}
        for q, label in enumerate(("before", "zero")):
            starts = [SB.start("F6-ok", 9)] + [SB.tau_zero_starts(f.name)[q][2] for f in fams[1:]]
            for i, st in enumerate(starts):
                bt.set_iterate(i, *st)
            bt.run(1, poll_every=1)
            for i, st in enumerate(starts):
                ratios, (x, _) = _batch_step(bt, i, ds[i], st)
                print("one step batch/%s %s from `%s` (tau -> %.3e): %s" % (fams[i].name, arith, label if i else "k=9", x[-1], SB.fmt(ratios)))
                _worst(worst, ratios)
        print("one step batch/F6 %s worst: %s" % (arith, SB.fmt(worst)))
    finally:
        bt.destroy()


# ---- the own-A families -------------------------------------------------------------------------------------------------------------

class Fam:
    """a family: its class, the workgroup sizes its test hook forces, its problem sets (tests/step_bound.py::own_a_sets), and what
    info() must say of the path a case names"""

    def __init__(self, T, name):
        self.name = name
        self.a_dtype = name[6:] if name.startswith("mid16") else None
        self.cls = {"small": T.SmallBatchSolver, "mid": T.MidBatchSolver, "mid16-bf16": T.Mid16BatchSolver, "mid16-f16": T.Mid16BatchSolver,
                    "sdp": T.SdpBatchSolver, "ragged": T.RaggedBatchSolver, "sparse": T.SparseBatchSolver,
                    "raggedsparse": T.RaggedSparseBatchSolver}[name]
        self.forced = (64, 256, 1024) if name == "small" else (256, 1024)
        self.sets = SB.own_a_sets(name)

    def path(self, sb, ds, forced, kw, resident):
        """asserts from info() (and, for which slot of a ragged sparse batch is streamed, from the plan the batch was made by) that
        the named path ran: the class, the forced workgroup size, the stored 16-bit type, who holds its entries in LDS"""
        info, count = sb.info(), len(ds)
        assert type(sb) is self.cls and info["n_prob"] == count == info["live"], (info["n_prob"], info["live"], count)
        said = []
        if "classes" in info:                                  # the ragged families: every problem in the forced class
            assert [c["threads"] for c in info["classes"]] == [256, 1024], info["classes"]
            assert [c["n_prob"] for c in info["classes"]] == ([count, 0] if forced == 256 else [0, count]), (forced, info["classes"])
            assert [c["live"] for c in info["classes"]] == [c["n_prob"] for c in info["classes"]]
        else:
            assert info["threads"] == forced, (info["threads"], forced)
        said.append("%d threads" % forced)
        if self.a_dtype:
            assert info["a_dtype"] == self.a_dtype
            said.append("A in %s" % info["a_dtype"])
        if self.name == "sparse":                              # one flag for the batch: everybody resident, or nobody
            assert info["resident"] == resident[0] and len(set(resident)) == 1, (info["resident"], resident)
            assert info["nnz_total"] == sum(int(np.count_nonzero(d.mat_a)) for d in ds)
            said.append("resident" if info["resident"] else "streamed")
        if self.name == "raggedsparse":
            from totsu_amd import raggedsparse as RS
            plan = RS.plan([RS.SparseProblem.of_dense(d) for d in ds], force_threads=forced, **kw)
            assert list(plan["resident"]) == resident and list(plan["cls"]) == [int(forced == 1024)] * count, (plan["resident"], plan["cls"])
            assert info["n_resident"] == sum(resident), (info["n_resident"], resident)
            assert [c["n_resident"] for c in info["classes"]] == ([sum(resident), 0] if forced == 256 else [0, sum(resident)])
            assert info["nnz_total"] == sum(int(np.count_nonzero(d.mat_a)) for d in ds)
            said.append("resident %s" % resident)
        return "%s, %s" % (self.cls.__name__, ", ".join(said))


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("name", SB.OWN_A_FAMILIES)
def test_own_a_one_step(T, name, arith):
    fam = Fam(T, name)
    p = _param(T, arith)
    for label, members, kws, residents in fam.sets:
        ds = [SB.problem(nm, seed) for nm, seed in members]
        # the problems of one batch start at different k's, so that a mix-up between slots shows
        ks = [SB.ks_of(nm)[i % len(SB.ks_of(nm))] for i, (nm, _) in enumerate(members)]
        starts = [SB.start(nm, k, seed) for (nm, seed), k in zip(members, ks)]
        refs = ds if fam.a_dtype is None else [SB.with_matrix(d, widened_of(d.mat_a, d.m, d.n, fam.a_dtype)) for d in ds]
        for q, kw in enumerate(kws):
            worst, paths = {}, []
            for forced in fam.forced:
                sb = fam.cls.from_dense(ds, p, force_threads=forced, **kw)
                try:
                    paths.append(fam.path(sb, ds, forced, kw, None if residents is None else residents[q]))
                    if fam.a_dtype is not None:
                        assert all(np.array_equal(sb.widened(i), r.mat_a) for i, r in enumerate(refs))
                    sb.set_iterates([x for x, _ in starts], [y for _, y in starts])
                    sb.run(1, poll_every=1)
                    for i, (ref, st) in enumerate(zip(refs, starts)):
                        x, y = sb.iterate(i)
                        s = sb.status(i)
                        assert s.state == -1 and s.iters == 1, (name, label, i, s.state, s.iters)
                        ratios = SB.check(ref, st, x, y, s.kind, tuple(s.cri))
                        print("one step %s %s %s %s %d threads problem %d (%s) k=%d: %s"
                              % (name, arith, label, kw, forced, i, members[i][0], ks[i], SB.fmt(ratios)))
                        _worst(worst, ratios)
                finally:
                    sb.destroy()
            print("one step %s %s %s %s [%s] worst: %s" % (name, arith, label, kw, "; ".join(paths), SB.fmt(worst)))
