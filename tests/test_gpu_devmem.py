"""GPU: the round calls of the six own-A batch families on DEVICE memory (thip_<family>_set_bc_dev / _set_a_dev / _set_iterates_dev /
_solutions_dev; Python set_bc_dev, set_a_dev, set_iterates_dev, solutions_dev).  Each is defined by the host call it mirrors, so every
comparison is bitwise -- precond(i), iterate(i), status(i), at once and after 10 further iterations, under both state arithmetics,
at every workgroup size a family's test hook forces -- between a batch that took the host call and twins that took the _dev call
with the same floats in a DeviceBuffer and in a torch tensor.  There is no tolerance in this file."""
import ctypes as C

import numpy as np
import pytest

from ownbatch_cases import F, T, _dense_of, _edge, _term_problem, _View  # noqa: F401  (T: the fixture)
from seta_cases import new_set, perturbed_a, set_a, triple_at, values_at
from setbc_cases import FAMILIES, RAGGED, Fam, full, param, perturbed, rowsums, same, with_bc
from sparse_cases import identity_problem, lengths_problem, zero_problem

pytestmark = pytest.mark.gpu

RUNNING, EXCESS = -1, 3
SPARSE = ("sparse", "raggedsparse")
FORMS = ("buffer", "torch")


@pytest.fixture(scope="module")
def fams(T):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Fam(T, name)
        return made[name]
    return get


class Held:
    """device copies of host arrays in one of the two forms, alive until free()"""

    def __init__(self, T, form):
        self.T, self.form, self.bufs = T, form, []

    def __call__(self, a):
        a = np.ascontiguousarray(a, F).ravel()
        if self.form == "torch":
            import torch
            t = torch.from_numpy(a.copy()).cuda()
            torch.cuda.synchronize()
            self.bufs.append(t)
            return t
        d = self.T.DeviceBuffer.from_host(a)
        self.bufs.append(d)
        return d

    def free(self):
        for b in self.bufs:
            if hasattr(b, "free"):
                b.free()
        self.bufs = []


def _cat(vs):
    return np.concatenate([np.asarray(v, F).ravel() for v in vs])


def _values(fam, olds, news):
    return _cat([values_at(o, d) for o, d in zip(olds, news)] if fam.sparse else [d.mat_a for d in news])


def _host(fam, sb, setter, olds, news, its, keep, first=0):
    if setter == "a":
        set_a(fam, sb, olds, news, first=first, keep=keep)
    elif setter == "bc":
        fam.set_bc(sb, news, first=first, keep=keep)
    else:
        sb.set_iterates([x for x, _ in its], [y for _, y in its], first=first)


def _dev(fam, sb, setter, olds, news, its, keep, up, first=0):
    n = len(news)
    if setter == "a":
        sb.set_a_dev(up(_values(fam, olds, news)), first=first, count=n, keep_iterate=keep)
    elif setter == "bc":
        rows = [d.vec_b_rowabs for d in news]
        assert all(r is None for r in rows) or all(r is not None for r in rows)
        sb.set_bc_dev(up(_cat([d.vec_b for d in news])), up(_cat([d.vec_c for d in news])),
                      None if rows[0] is None else up(_cat(rows)), first=first, count=n, keep_iterate=keep)
    else:
        sb.set_iterates_dev(up(_cat([x for x, _ in its])), up(_cat([y for _, y in its])), first=first, count=n)


def _news(setter, ds, keep):
    if setter == "a":
        return new_set(ds)
    new = [perturbed(d, 3 + i) for i, d in enumerate(ds)]
    if keep:                                    # (the kept half of the cases carries explicit row sums, the fresh half |b|)
        new = [with_bc(d, d.vec_b, d.vec_c, rowabs=rowsums(d, 20 + i)) for i, d in enumerate(new)]
    return new


def _agree(batches, P, tag, steps=10, poll=7):
    X = batches[0]
    for Y in batches[1:]:
        for i in range(P):
            same(full(X, i), full(Y, i), tag + ("at once", i))
    for sb in batches:
        sb.run(steps, poll_every=poll)
    for Y in batches[1:]:
        for i in range(P):
            same(full(X, i), full(Y, i), tag + (steps, i))


# ---- 1. every family, every setter, both keep_iterate values ------------------------------------------------------------------------

CASES = [("a", False), ("a", True), ("bc", False), ("bc", True), ("iterates", False)]


@pytest.mark.parametrize("setter,keep", CASES)
@pytest.mark.parametrize("name", FAMILIES)
def test_setters_bitwise(T, fams, name, setter, keep):
    fam = fams(name)
    for arith in ("plain", "compensated"):
        p = param(T, arith)
        for label, ds, _, kws in fam.sets:
            news = _news(setter, ds, keep)
            for kw in kws:
                for forced in fam.forced:
                    batches = [fam.make(ds, p, forced, **kw) for _ in range(3)]
                    ups = [Held(T, form) for form in FORMS]
                    try:
                        its = None
                        if setter == "iterates":                 # some iterate of each problem: a twin's after three iterations
                            batches[2].run(3, poll_every=3)
                            its = [batches[2].iterate(i) for i in range(len(ds))]
                            batches[2].reinit()
                        for sb in batches:
                            sb.run(7, poll_every=7)
                        _host(fam, batches[0], setter, ds, news, its, keep)
                        for sb, up in zip(batches[1:], ups):
                            _dev(fam, sb, setter, ds, news, its, keep, up)
                            assert sb.info()["live"] == len(ds)
                        _agree(batches, len(ds), (name, setter, keep, arith, label, str(kw), forced))
                        assert batches[0].status(0).iters == 10
                    finally:
                        for sb in batches:
                            sb.destroy()
                        for up in ups:
                            up.free()


@pytest.mark.parametrize("name", FAMILIES)
def test_stopped_problems_run_again(T, fams, name):
    """a problem stopped by max_iter and one whose iteration ended through tau = 0: the kept setters start them again, host and device
    route alike"""
    from tau_zero_problems import _lp_layout
    from tau_zero_problems import family as tz_family
    from totsu_amd import _lib
    fam = fams(name)
    label, ds, _, kws = fam.sets[0]
    f1 = _dense_of(tz_family("F1"))
    f1.vec_b_rowabs = None
    feasible = with_bc(f1, _lp_layout(64, 126, 1)[4], f1.vec_c)
    kw1 = {"nnz_caps": [0, 0]} if name == "raggedsparse" else {}
    kw = kws[-1]
    cases = [("excess", ds, param(T, max_iter=5), kw, _lib.ST_EXCESS_ITER),
             ("tau zero", [f1, f1], param(T, eps_acc=1e-5, eps_inf=1e-5, max_iter=5000),
              dict(kw1, **{k: v for k, v in kw.items() if k != "nnz_caps"}), _lib.ST_INFEASIBLE)]
    for what, held, p, kw, state in cases:
        for setter in ("a", "bc", "iterates"):
            news = [feasible, feasible] if what == "tau zero" and setter == "bc" else _news(setter, held, False)
            batches = [fam.make(held, p, **kw) for _ in range(2)]
            up = Held(T, "buffer")
            try:
                for sb in batches:
                    res = sb.run(-1, poll_every=64)
                    assert [r.state for r in res] == [state] * len(held), (what, [r.state for r in res])
                its = [batches[0].raw_iterate(i) for i in range(len(held))]
                assert what != "tau zero" or all(x[-1] <= 1e-12 for x, _ in its)
                _host(fam, batches[0], setter, held, news, its, True)
                _dev(fam, batches[1], setter, held, news, its, True, up)
                for sb in batches:
                    assert sb.info()["live"] == len(held)
                    assert [s.state for s in sb.statuses()] == [RUNNING] * len(held)
                _agree(batches, len(held), (name, what, setter), steps=4, poll=4)
            finally:
                for sb in batches:
                    sb.destroy()
                up.free()


# ---- 2. solutions_dev ---------------------------------------------------------------------------------------------------------------

GUARD = 16
PATTERN = np.float32(-12345.625)


def _check_solutions_dev(T, sb, P, tag):
    want, stat = sb.solutions(), sb.statuses()
    for first, count in ((0, None), (P // 3, max(1, P // 4)), (P - 1, 1)):
        n = P - first if count is None else count
        wx, wy = _cat([want[first + k][0] for k in range(n)]), _cat([want[first + k][1] for k in range(n)])
        ws = np.array([stat[first + k].state for k in range(n)], dtype=np.int32)
        x, y, st = sb.solutions_dev(first, count)
        try:
            assert np.array_equal(x.to_host().view(np.uint32), wx.view(np.uint32)), (tag, first, "x")
            assert np.array_equal(y.to_host().view(np.uint32), wy.view(np.uint32)), (tag, first, "y")
            assert np.array_equal(st.to_host().view(np.int32), ws), (tag, first, "state")
        finally:
            for d in (x, y, st):
                d.free()
        # the same into guarded buffers of the caller's, and into torch tensors: nothing outside the range's part is written
        bufs = [T.DeviceBuffer.from_host(np.full(w.size + 2 * GUARD, PATTERN, F)) for w in (wx, wy, ws)]
        try:
            views = [_View(T, b, GUARD, w.size) for b, w in zip(bufs, (wx, wy, ws))]
            out = sb.solutions_dev(first, count, out_x=views[0], out_y=views[1], out_state=views[2])
            assert out[0] is views[0] and out[2] is views[2]
            for b, w in zip(bufs, (wx, wy, ws.view(F))):
                got = b.to_host()
                assert np.array_equal(got[GUARD:GUARD + w.size].view(np.uint32), w.view(np.uint32)), (tag, first)
                assert np.all(got[:GUARD] == PATTERN) and np.all(got[GUARD + w.size:] == PATTERN), (tag, first, "guard")
        finally:
            for b in bufs:
                b.free()
    import torch
    tx, ty = torch.zeros(sum(w[0].size for w in want), dtype=torch.float32, device="cuda"), torch.zeros(sum(w[1].size for w in want), dtype=torch.float32, device="cuda")
    ts = torch.zeros(P, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    sb.solutions_dev(out_x=tx, out_y=ty, out_state=ts)
    assert np.array_equal(tx.cpu().numpy().view(np.uint32), _cat([w[0] for w in want]).view(np.uint32)), tag
    assert np.array_equal(ty.cpu().numpy().view(np.uint32), _cat([w[1] for w in want]).view(np.uint32)), tag
    assert ts.cpu().numpy().tolist() == [s.state for s in stat], tag
    return stat


@pytest.mark.parametrize("name", FAMILIES)
def test_solutions_dev(T, fams, name):
    fam = fams(name)
    P = 300
    if name in RAGGED:                                           # the set cycled to 300: stopped by max_iter, some restarted and running
        for kw0 in fam.sets[0][3]:
            cyc, kw = fam.cycled(0, P, kw0)
            sb = fam.make(cyc, param(T, max_iter=12), **kw)
            try:
                sb.run(-1, poll_every=64)
                fam.set_bc(sb, cyc[100:140], first=100)
                sb.run(3, poll_every=3)
                stat = _check_solutions_dev(T, sb, P, (name, str(kw0)))
                assert sorted({s.state for s in stat}) == [RUNNING, EXCESS]
            finally:
                sb.destroy()
        return
    ds = [_term_problem(i) for i in range(P)]                    # tests/test_gpu_setbc.py's mix
    for kw in fam.sets[0][3]:
        sb = fam.make(ds, param(T, eps_acc=1e-5, eps_inf=1e-5, max_iter=100000), **kw)
        try:
            res = sb.run(-1, poll_every=64)
            assert sorted({r.state for r in res}) == [0, 1, 2]
            fam.set_bc(sb, ds[:30])
            sb.set_param(param(T, eps_acc=1e-5, eps_inf=1e-5, max_iter=5))
            sb.run(-1, poll_every=5)
            fam.set_bc(sb, ds[:9])
            sb.run(2, poll_every=2)
            stat = _check_solutions_dev(T, sb, P, (name, str(kw)))
            assert [s.state for s in stat[:9]] == [RUNNING] * 9 and [s.state for s in stat[9:30]] == [EXCESS] * 21
            assert {s.state for s in stat[30:]} == {0, 1, 2} and any(s.kind == 1 and s.tau == 0.0 for s in stat[30:])
        finally:
            sb.destroy()


# ---- 3. the dense copy kernel -------------------------------------------------------------------------------------------------------

def _chunk():
    from totsu_amd import _lib
    return _lib.load().thip_test_ownbatch_copy_chunk()


def test_copy_into_a_ragged_batch_of_many_allocations(T):
    """m n = 1, 3, 4, 5, C - 1, C, C + 1 for the copy kernel's chunk C, 300 x 1 beside 1 x 1, up to 157 x 157, every problem's A in a
    DeviceBuffer of its own; the source starts 4 bytes off a 16-byte boundary; the first and the last problem lie outside the range"""
    Cc = _chunk()
    assert Cc == 4096
    shapes = [(7, 3), (1, 1), (3, 1), (4, 1), (5, 1), (65, 63), (64, 64), (241, 17), (300, 1), (157, 157), (1, 1), (9, 2)]
    assert [m * n for m, n in shapes[1:8]] == [1, 3, 4, 5, Cc - 1, Cc, Cc + 1]
    ds = [_edge(m, n, s) for s, (m, n) in enumerate(shapes)]
    new = new_set(ds)
    p = param(T)
    own = [T.DeviceBuffer.from_host(d.mat_a) for d in ds]
    import copy
    held = []
    for d, buf in zip(ds, own):
        e = copy.copy(d)
        e.mat_a = buf
        held.append(e)
    X, Y = T.RaggedBatchSolver(held, p), T.RaggedBatchSolver.from_dense(ds, p)
    first, count = 1, len(ds) - 2
    vals = _cat([d.mat_a for d in new[first:first + count]])
    src = T.DeviceBuffer.from_host(np.concatenate([np.zeros(1, F), vals, np.zeros(3, F)]))
    try:
        assert src.ptr % 16 == 0
        for sb in (X, Y):
            sb.run(7, poll_every=7)
        dev = X.info()["device_bytes"]
        X.set_a_dev(_View(T, src, 1, vals.size), first=first, count=count, keep_iterate=True)
        assert X.info()["device_bytes"] == dev                   # in place: nothing is allocated on the device
        Y.set_a([d.mat_a for d in new[first:first + count]], first=first, keep_iterate=True)
        for i, (d, e, buf) in enumerate(zip(ds, new, own)):      # the slots' A is the source, the neighbours' is what it was
            want = e.mat_a if first <= i < first + count else d.mat_a
            assert np.array_equal(buf.to_host().view(np.uint32), np.asarray(want, F).view(np.uint32)), i
        _agree([Y, X], len(ds), ("ragged copy",))
    finally:
        X.destroy()
        Y.destroy()
        for b in own + [src]:
            b.free()


@pytest.mark.parametrize("name,m,n", [("small", 81, 41), ("mid", 157, 157)])
def test_copy_after_replace_four_allocations(T, fams, name, m, n):
    """m n % 4 != 0, so the slot bases in the caller's buffer are unaligned; three slots were replaced, so the destinations lie in four
    allocations; one call covers them, and problems 0 and 5 outside the range keep their A"""
    fam = fams(name)
    P = 6
    ds = [_edge(m, n, s) for s in range(P)]
    assert (m * n) % 4
    mid = [perturbed_a(d, 40 + i) for i, d in enumerate(ds)]
    new = new_set(ds, base=80)
    p = param(T)
    a = np.stack([d.mat_a for d in ds])
    base = T.DeviceBuffer.from_host(a)
    b, c = np.stack([d.vec_b for d in ds]), np.stack([d.vec_c for d in ds])
    X = fam.cls(n, m, base, b, c, ds[0].seg_type, ds[0].seg_len, p)
    Y = fam.cls(n, m, a, b, c, ds[0].seg_type, ds[0].seg_len, p)
    own = {i: T.DeviceBuffer.from_host(mid[i].mat_a) for i in (1, 2, 4)}
    first, count = 1, 4
    vals = _cat([d.mat_a for d in new[first:first + count]])
    src = T.DeviceBuffer.from_host(vals)
    try:
        for i, buf in own.items():
            X.replace(i, buf, ds[i].vec_b, ds[i].vec_c)
            Y.replace(i, mid[i].mat_a, ds[i].vec_b, ds[i].vec_c)
        for sb in (X, Y):
            sb.run(7, poll_every=7)
        X.set_a_dev(src, first=first, count=count)
        Y.set_a([d.mat_a for d in new[first:first + count]], first=first)
        got = base.to_host().reshape(P, m * n)
        for i in range(P):
            want = new[i].mat_a if first <= i < first + count else ds[i].mat_a
            if i in own:
                assert np.array_equal(own[i].to_host(), np.asarray(new[i].mat_a, F)), i
                assert np.array_equal(got[i], np.asarray(ds[i].mat_a, F)), i        # (the buffer the slot left is not written)
            else:
                assert np.array_equal(got[i], np.asarray(want, F)), i
        _agree([Y, X], P, (name, "four allocations"))
    finally:
        X.destroy()
        Y.destroy()
        for buf in list(own.values()) + [base, src]:
            buf.free()


# ---- 4. the in-place form -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,m,n", [("small", 80, 40), ("mid", 160, 96), ("sdp", 45, 6)])
def test_in_place_form(T, fams, name, m, n):
    from totsu_amd._lib import lib
    fam = fams(name)
    label, ds, _, _ = fam.sets[0]
    assert (ds[0].m, ds[0].n) == (m, n)
    new = new_set(ds)
    p = param(T)
    a = np.stack([np.asarray(d.mat_a, F) for d in ds])
    b, c = np.stack([d.vec_b for d in ds]), np.stack([d.vec_c for d in ds])
    base = T.DeviceBuffer.from_host(a)
    X = fam.cls(n, m, base, b, c, ds[0].seg_type, ds[0].seg_len, p)
    Y = fam.cls(n, m, a, b, c, ds[0].seg_type, ds[0].seg_len, p)
    try:
        for sb in (X, Y):
            sb.run(7, poll_every=7)
        vals = _cat([d.mat_a for d in new])
        lib.thip_h2d(base.ptr, vals.ctypes.data, vals.size)      # the caller rewrites its own buffer ..
        dev = X.info()["device_bytes"]
        X.set_a_dev(None, keep_iterate=True)                     # .. and says so
        assert X.info()["device_bytes"] == dev
        Y.set_a([d.mat_a for d in new], keep_iterate=True)
        _agree([Y, X], len(ds), (name, "in place"))
    finally:
        X.destroy()
        Y.destroy()
        base.free()


# ---- 5. sparse: the blob the device route makes -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SPARSE)
def test_the_blob_after_set_a_dev(T, fams, name):
    """rows and columns of 0, 1, 32, 33, 65 (and more) entries, the zero matrix, [I; -I], explicit zeros; resident and streamed"""
    fam = fams(name)
    p = param(T)
    cases = [("rows", lengths_problem(False, 0)), ("cols", lengths_problem(True, 0)), ("zero", zero_problem()),
             ("identity", identity_problem(0)), ("rows-explicit-zeros", lengths_problem(False, 1))]
    lens = set()
    for _, d in cases[:2]:
        cp, ri, _ = triple_at(d, d)
        lens |= set(np.diff(cp).tolist()) | set(np.bincount(ri, minlength=d.m).tolist())
    assert {0, 1, 32, 33, 65} <= lens
    groups = [[d] for _, d in cases] if name == "sparse" else [[d for _, d in cases]]
    labels = [[l] for l, _ in cases] if name == "sparse" else [[l for l, _ in cases]]
    for ds, ls in zip(groups, labels):
        for resident in (1, 0):
            if resident == 1 and name == "sparse" and ls[0] in ("rows", "cols", "rows-explicit-zeros"):
                kw = {}                                          # (whatever create chose: forcing residence may not fit)
            else:
                kw = {"force_resident": resident}
            X, Y = fam.make(ds, p, **kw), fam.make(ds, p, **kw)
            up = Held(T, "buffer")
            try:
                new = [perturbed_a(d, 70 + i, zeros=5 if "zeros" in l else 0) for i, (d, l) in enumerate(zip(ds, ls))]
                for sb in (X, Y):
                    sb.run(3, poll_every=3)
                set_a(fam, X, ds, new)
                vals = _values(fam, ds, new)
                Y.set_a_dev(up(vals if vals.size else np.zeros(1, F)))
                for i in range(len(ds)):
                    assert np.array_equal(Y.blob(i), X.blob(i)), (name, ls[i], resident)
                _agree([X, Y], len(ds), (name, str(ls), resident), steps=5, poll=5)
            finally:
                X.destroy()
                Y.destroy()
                up.free()


# ---- 6. a whole round on the device -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mid", "sparse"])
def test_a_whole_round_on_the_device(T, fams, name):
    import torch
    fam = fams(name)
    label, ds, _, kws = fam.sets[0]
    p = param(T, eps_acc=1e-4)
    X, Y = fam.make(ds, p, **kws[0]), fam.make(ds, p, **kws[0])
    try:
        for sb in (X, Y):
            sb.run(10, poll_every=10)
        for rnd in range(2):
            new_a = new_set(ds, base=10 * rnd)
            new_bc = [perturbed(d, 50 + 10 * rnd + i) for i, d in enumerate(ds)]
            set_a(fam, X, ds, new_a, keep=True)
            fam.set_bc(X, new_bc, keep=True)
            X.run(40, poll_every=16)
            want, stat = X.solutions(), X.statuses()
            tv = torch.from_numpy(_values(fam, ds, new_a)).cuda()
            tb, tc = torch.from_numpy(_cat([d.vec_b for d in new_bc])).cuda(), torch.from_numpy(_cat([d.vec_c for d in new_bc])).cuda()
            Y.set_a_dev(tv, keep_iterate=True)
            Y.set_bc_dev(tb, tc, keep_iterate=True)
            Y.run(40, poll_every=16)
            x, y, st = Y.solutions_dev()
            assert np.array_equal(x.to_host().view(np.uint32), _cat([w[0] for w in want]).view(np.uint32)), (name, rnd)
            assert np.array_equal(y.to_host().view(np.uint32), _cat([w[1] for w in want]).view(np.uint32)), (name, rnd)
            assert st.to_host().view(np.int32).tolist() == [s.state for s in stat]
            for i in range(len(ds)):
                same(full(X, i), full(Y, i), (name, rnd, i))
            for d in (x, y, st):
                d.free()
    finally:
        X.destroy()
        Y.destroy()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------

def _addresses(sb):
    from totsu_amd._lib import lib
    addr, size = (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    lib.thip_test_ownbatch_addresses(sb.h, addr, size)
    return list(addr), list(size)


@pytest.mark.parametrize("name", FAMILIES)
def test_refusals(T, fams, name):
    from totsu_amd import _lib
    fam = fams(name)
    label, ds, _, kws = fam.sets[0]
    P = len(ds)
    cyc, kw = fam.cycled(0, 6, kws[-1])
    P, first, count = 6, 1, 4
    new = new_set(cyc)
    sb = fam.make(cyc, param(T), **kw)
    try:
        sb.run(5, poll_every=5)
        sb.set_bc_dev(T.DeviceBuffer.from_host(_cat([d.vec_b for d in cyc])), T.DeviceBuffer.from_host(_cat([d.vec_c for d in cyc])))
        warm = [sb.iterate(i) for i in range(P)]
        hx, hy = T.DeviceBuffer.from_host(_cat([x for x, _ in warm])), T.DeviceBuffer.from_host(_cat([y for _, y in warm]))
        sb.set_iterates_dev(hx, hy)
        for d in sb.solutions_dev() + (hx, hy):
            d.free()
        sb.run(2, poll_every=2)                                  # (the store, the staging buffers and the tables exist from here on)
        want = [full(sb, i) for i in range(P)]
        blobs = [sb.blob(i) for i in range(P)] if fam.sparse else None
        info = sb.info()

        def unchanged():
            now = sb.info()
            assert (now["device_bytes"], now["live"]) == (info["device_bytes"], info["live"])
            for i in range(P):
                same(full(sb, i), want[i])
                assert blobs is None or np.array_equal(sb.blob(i), blobs[i])

        def refused(match, fn, *a, **k):
            with pytest.raises(ValueError, match=match):
                fn(*a, **k)
            unchanged()

        olds, news = cyc[first:first + count], new[first:first + count]
        sizes = [int(sb._a_size(first + k)) for k in range(count)]
        at = int(sum(sizes[:2]))                                  # where problem first + 2's values begin
        if sizes[2] > 0:
            for poison in (np.nan, np.inf):
                v = _values(fam, olds, news)
                v[at + sizes[2] // 2] = poison
                buf = T.DeviceBuffer.from_host(v)
                for keep in (False, True):
                    refused("problem %d: a value of A is not finite" % (first + 2), sb.set_a_dev, buf, first=first, count=count, keep_iterate=keep)
                buf.free()
        its = [sb.iterate(first + k) for k in range(count)]
        for what, where, value in (("tau", 0, -1.0), ("tau", 0, np.nan), ("kappa", 1, 0.5)):
            xs, ys = [x.copy() for x, _ in its], [y.copy() for _, y in its]
            (xs if where == 0 else ys)[2][-1] = value
            bx, by = T.DeviceBuffer.from_host(_cat(xs)), T.DeviceBuffer.from_host(_cat(ys))
            refused("problem %d: a start's %s" % (first + 2, what), sb.set_iterates_dev, bx, by, first=first, count=count)
            bx.free()
            by.free()
        some = T.DeviceBuffer(1 << 16, zero=True)
        for a in ((P, 1), (0, P + 1), (-1, 1), (0, 0)):          # a range outside the batch
            refused("no problems", sb.set_a_dev, some, *a)
            refused("no problems", sb.set_bc_dev, some, some, None, *a)
            refused("no problems", sb.set_iterates_dev, some, some, *a)
            refused("no problems", sb.solutions_dev, *a)
        fn = lambda which: getattr(_lib.load(), sb._prefix + which)     # noqa: E731  (and by return code at the C ABI)
        for args in ((sb.h, P, 1), (sb.h, 0, 0), (sb.h, -1, 1), (sb.h, 0, P + 1), (None, 0, 1)):
            assert fn("set_a_dev")(args[0], args[1], args[2], some.ptr, 0) == _lib.E_INVALID
            assert fn("set_bc_dev")(args[0], args[1], args[2], some.ptr, some.ptr, None, None, 0) == _lib.E_INVALID
            assert fn("set_iterates_dev")(args[0], args[1], args[2], some.ptr, some.ptr) == _lib.E_INVALID
            assert fn("solutions_dev")(args[0], args[1], args[2], some.ptr, some.ptr, None) == _lib.E_INVALID
        assert fn("set_bc_dev")(sb.h, 0, 1, None, some.ptr, None, None, 0) == _lib.E_INVALID
        assert fn("set_iterates_dev")(sb.h, 0, 1, some.ptr, None) == _lib.E_INVALID
        unchanged()
        short = T.DeviceBuffer(1)
        if sum(sizes) > 1:
            refused(r"values: 1 entries where %d are needed" % sum(sizes), sb.set_a_dev, short, first=first, count=count)
        refused("out_x", sb.solutions_dev, out_x=short)
        if fam.sparse:
            refused("null values of A", sb.set_a_dev, None, first=first, count=count)
        # memory the batch owns: its arena as an output, its staging buffer and its store as inputs
        addr, size = _addresses(sb)
        assert all(addr) and all(size) and size[0] == info["arena_bytes"]
        arena = _View(T, type("B", (), {"ptr": addr[0]})(), 0, size[0] // 4)
        refused("overlaps memory the batch owns", sb.solutions_dev, out_x=arena)
        refused("overlaps memory the batch owns", sb.solutions_dev, first=0, count=1, out_state=_View(T, arena, size[0] // 4 - 1, 1))
        for k in (1, 2):
            owned = _View(T, type("B", (), {"ptr": addr[k]})(), 0, size[k] // 4)
            assert fn("set_bc_dev")(sb.h, 0, 1, owned.ptr, some.ptr, None, None, 1) == _lib.E_INVALID
            assert fn("set_iterates_dev")(sb.h, 0, 1, some.ptr, owned.ptr) == _lib.E_INVALID
            assert fn("set_a_dev")(sb.h, 0, 1, owned.ptr, 1) == _lib.E_INVALID
        unchanged()
        sb.run(2, poll_every=2)                                  # and the batch still runs and takes a device round
        assert [s.iters for s in sb.statuses()] == [4] * P
        buf = T.DeviceBuffer.from_host(_values(fam, olds, news))
        sb.set_a_dev(buf, first=first, count=count, keep_iterate=True)
        assert [s.iters for s in sb.statuses()] == [4, 0, 0, 0, 0, 4]
        for b in (some, short, buf):
            b.free()
    finally:
        sb.destroy()


@pytest.mark.parametrize("name", ["small", "mid", "ragged"])
def test_dense_refusals_in_slot_memory(T, fams, name):
    """the in-place form with a NaN in slot memory, and a dev_values that overlaps a slot's A without being the in-place form"""
    import copy
    from totsu_amd._lib import lib
    fam = fams(name)
    label, ds, _, _ = fam.sets[0]
    ds = (ds * 3)[:4]
    p = param(T)
    own = [T.DeviceBuffer.from_host(d.mat_a) for d in ds]
    if name == "ragged":
        held = []
        for d, buf in zip(ds, own):
            e = copy.copy(d)
            e.mat_a = buf
            held.append(e)
        sb = T.RaggedBatchSolver(held, p)
    else:
        sb = fam.make(ds, p)
        for i, (d, buf) in enumerate(zip(ds, own)):
            sb.replace(i, buf, d.vec_b, d.vec_c)
    try:
        sb.run(5, poll_every=5)
        want = [full(sb, i) for i in range(4)]
        dev = sb.info()["device_bytes"]
        with pytest.raises(ValueError, match="overlaps the A of a slot"):
            sb.set_a_dev(own[2], first=2, count=1)               # exactly slot 2's A: the in-place form is written with None
        with pytest.raises(ValueError, match="overlaps the A of a slot"):
            sb.set_a_dev(own[3], first=3, count=1, keep_iterate=True)
        bad = np.asarray(ds[2].mat_a, F).copy()
        bad[bad.size // 2] = np.nan
        lib.thip_h2d(own[2].ptr, bad.ctypes.data, bad.size)
        for keep in (False, True):
            with pytest.raises(ValueError, match="problem 2: a value of A is not finite"):
                sb.set_a_dev(None, keep_iterate=keep)
        good = np.asarray(ds[2].mat_a, F)
        lib.thip_h2d(own[2].ptr, good.ctypes.data, good.size)
        assert sb.info()["device_bytes"] == dev
        for i in range(4):
            same(full(sb, i), want[i])
        sb.set_a_dev(None, keep_iterate=True)                    # the values are back: taken
        assert [s.iters for s in sb.statuses()] == [0] * 4
    finally:
        sb.destroy()
        for b in own:
            b.free()


# ---- 8. bytes moved -----------------------------------------------------------------------------------------------------------------

def _moved(sb):
    from totsu_amd._lib import lib
    up, down = C.c_uint64(), C.c_uint64()
    lib.thip_test_ownbatch_last_transfer(sb.h, C.byref(up), C.byref(down))
    return up.value, down.value


def test_bytes_moved(T, fams):
    """conditions, not measurements: the dense update moves a table only, the read-out nothing"""
    fam = fams("mid")
    m, n, P = 160, 96, 8
    ds = [_edge(m, n, s) for s in range(P)]
    new = new_set(ds)
    sb = fam.make(ds, param(T))
    buf = T.DeviceBuffer.from_host(_cat([d.mat_a for d in new]))
    try:
        sb.run(3, poll_every=3)
        for first, count in ((0, P), (2, 3)):
            sb.set_a_dev(_View(T, buf, first * m * n, count * m * n), first=first, count=count, keep_iterate=True)
            h2d, d2h = _moved(sb)
            assert 0 < h2d <= 64 * count and h2d < 4 * m * n, (h2d, count)
        x, y, st = sb.solutions_dev(sync=False)
        assert _moved(sb) == (0, 0)
        from totsu_amd._lib import lib
        lib.thip_sync()
        for d in (x, y, st):
            d.free()
    finally:
        sb.destroy()
        buf.free()
