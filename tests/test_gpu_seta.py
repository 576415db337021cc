"""GPU: set_a of the six own-A batch families (thip_<family>_set_a).  A range of problems takes new values of A and keeps its shape,
cone layout, b, c, row sums and -- a sparse family -- its pattern.  The definition everything is held to is the route that existed
before: replace(i, the new A, the slot's present b, c, rowabs) on every slot of a second batch -- bit for bit in the preconditioner,
the iterate and the status block, at once and after 1, 10 and 50 further iterations, at every workgroup size a family can run, under
both state arithmetics, resident and streamed -- and, with the iterate kept, replace(..., start=iterate(i)); under plain arithmetic
the continuation pins the carried pair that set_a forms again.  The f64 oracle on (new A, b, c) guards against both routes being wrong
together; its tolerance is tests/warm_cases.py::iterate_tol, the number the set_bc tests apply, at iterates 0, 1 and 9 and, for
every problem with a PSD cone, at iterate 49 as the families' own tests (an oracle run of its own for those: the shared runs of
warm_cases.oracle_run end at 19).  The sparse families' blob after set_a is read back through a test hook and compared
with sparsebatch.pack of the pattern with the new values, word for word."""
import numpy as np
import pytest

from ownbatch_cases import F, T, _dense_of, _edge, _oracle, _View  # noqa: F401  (T: the fixture)
from seta_cases import new_set, perturbed_a, replace_a, set_a, triple_at, values_at, with_a
from setbc_cases import FAMILIES, RAGGED, Fam, full, param, perturbed, rowsums, same, with_bc
from sparse_cases import csc_of, identity_problem, lengths_problem, zero_problem
from warm_cases import PSD, iterate_tol, snap_xy

pytestmark = pytest.mark.gpu

RUNNING = -1
SPARSE = ("sparse", "raggedsparse")


@pytest.fixture(scope="module")
def fams(T):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Fam(T, name)
        return made[name]
    return get


def _walk(X, Y, P, tag, steps=(1, 10, 50), poll=64):
    """X and Y hold the same state now and after 1, 10 and 50 further iterations"""
    for i in range(P):
        same(full(X, i), full(Y, i), tag + ("at once", i))
    done = 0
    for j in steps:
        X.run(j - done, poll_every=poll)
        Y.run(j - done, poll_every=poll)
        done = j
        for i in range(P):
            same(full(X, i), full(Y, i), tag + (j, i))
            assert X.status(i).iters == j, tag


# ---- 1. fresh, bitwise --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arith", ["plain", "compensated"])
@pytest.mark.parametrize("name", FAMILIES)
def test_fresh_bitwise(T, fams, name, arith):
    fam = fams(name)
    p = param(T, arith)
    for label, ds, _, kws in fam.sets:
        new = new_set(ds)
        for kw in kws:
            for forced in fam.forced:
                X, Y = fam.make(ds, p, forced, **kw), fam.make(ds, p, forced, **kw)
                try:
                    X.run(10, poll_every=7)
                    dev = X.info()["device_bytes"]
                    set_a(fam, X, ds, new)
                    assert X.info()["live"] == len(ds)
                    if not fam.sparse:
                        assert X.info()["device_bytes"] == dev      # in place: nothing is allocated
                    for i, d in enumerate(new):
                        replace_a(fam, Y, i, ds[i], d)
                    for i in range(len(ds)):
                        st = X.status(i)
                        assert (st.state, st.iters, st.kind, st.tau, st.kappa) == (RUNNING, 0, 0, 1.0, 0.0)
                    _walk(X, Y, len(ds), (name, arith, label, str(kw), forced), poll=7)
                finally:
                    X.destroy()
                    Y.destroy()


# ---- 2. keep, bitwise, on running problems ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arith", ["plain", "compensated"])
@pytest.mark.parametrize("name", FAMILIES)
def test_keep_bitwise_on_running_problems(T, fams, name, arith):
    fam = fams(name)
    p = param(T, arith)
    for label, ds, _, kws in fam.sets:
        new = new_set(ds)
        for kw in kws:
            for forced in fam.forced:
                X, Y = fam.make(ds, p, forced, **kw), fam.make(ds, p, forced, **kw)
                try:
                    X.run(10, poll_every=7)
                    Y.run(10, poll_every=7)
                    its = [X.iterate(i) for i in range(len(ds))]
                    set_a(fam, X, ds, new, keep=True)
                    for i, d in enumerate(new):
                        replace_a(fam, Y, i, ds[i], d, start=Y.iterate(i))
                    for i in range(len(ds)):                 # the iterate is the one that lay in the arena
                        x, y = X.iterate(i)
                        assert np.array_equal(x, its[i][0]) and np.array_equal(y, its[i][1])
                        st = X.status(i)
                        assert (st.state, st.iters, st.kind, tuple(st.cri)) == (RUNNING, 0, 0, (0.0, 0.0, 0.0))
                    _walk(X, Y, len(ds), (name, arith, label, str(kw), forced), poll=7)
                finally:
                    X.destroy()
                    Y.destroy()


# ---- 3. after a set_bc: the slot points into the store --------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["none", "explicit", "mixed"])
@pytest.mark.parametrize("name", FAMILIES)
def test_after_a_set_bc(T, fams, name, case):
    fam = fams(name)
    p = param(T)
    label, ds, _, kws = fam.sets[0]
    held = [with_bc(d, d.vec_b, d.vec_c, rowabs=rowsums(d, i)) for i, d in enumerate(ds)]
    bc = [perturbed(d, i) for i, d in enumerate(held)]
    for i, d in enumerate(bc):
        has = {"none": False, "explicit": True, "mixed": i % 2 == 0}[case]
        bc[i] = with_bc(d, d.vec_b, d.vec_c, rowabs=rowsums(d, 10 + i) if has else None)
    new = [with_a(d, e.mat_a) for d, e in zip(bc, new_set(ds))]        # the new A with the b, c and row sums the store holds
    for kw in kws:
        for keep in (False, True):
            X, Y = fam.make(held, p, **kw), fam.make(held, p, **kw)
            try:
                X.run(3, poll_every=3)
                Y.run(3, poll_every=3)
                fam.set_bc(X, bc, keep=keep)
                dev = X.info()["device_bytes"]
                set_a(fam, X, ds, new, keep=keep)
                if not fam.sparse:
                    assert X.info()["device_bytes"] == dev
                for i, d in enumerate(new):
                    replace_a(fam, Y, i, ds[i], d, start=Y.iterate(i) if keep else None)
                _walk(X, Y, len(ds), (name, case, str(kw), keep), steps=(1, 10))
            finally:
                X.destroy()
                Y.destroy()


# ---- 4. the composition: set_a(keep) + set_bc(keep) is a round that moves all three ---------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_the_composition(T, fams, name):
    fam = fams(name)
    for arith in ("plain", "compensated"):
        p = param(T, arith)
        for label, ds, _, kws in fam.sets:
            new = [with_a(b, a.mat_a) for a, b in zip(new_set(ds), [perturbed(d, 30 + i) for i, d in enumerate(ds)])]
            for i in range(0, len(new), 2):
                new[i] = with_bc(new[i], new[i].vec_b, new[i].vec_c, rowabs=rowsums(new[i], 60 + i))
            for kw in kws:
                X, Y = fam.make(ds, p, **kw), fam.make(ds, p, **kw)
                try:
                    X.run(10, poll_every=10)
                    Y.run(10, poll_every=10)
                    set_a(fam, X, ds, new, keep=True)
                    fam.set_bc(X, new, keep=True)
                    for i, d in enumerate(new):
                        replace_a(fam, Y, i, ds[i], d, start=Y.iterate(i))
                    _walk(X, Y, len(ds), (name, arith, label, str(kw)), steps=(1, 10))
                finally:
                    X.destroy()
                    Y.destroy()


# ---- 5. the oracle ------------------------------------------------------------------------------------------------------------------

def _rel(got, want):
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-6)


PSD_ITERS = [0, 1, 9, 49]              # tests/ownbatch_cases.py's SDP_ITERS: what the families' own tests check with a PSD cone
_PSD_RUNS = {}


def _psd_run(key, d):
    """the oracle's snapshots of a problem with a PSD cone at PSD_ITERS (computed once per key and never changed)"""
    if key not in _PSD_RUNS:
        ro = _oracle(d, PSD_ITERS)
        assert len(ro.trace) > max(PSD_ITERS), key
        _PSD_RUNS[key] = ro
    return _PSD_RUNS[key]


def _psd_snap(ro, d, it):
    N = d.n + 2 * d.m + 1
    s = ro.snaps[PSD_ITERS.index(it)]
    return s[:N], s[N:]


@pytest.mark.parametrize("name", FAMILIES)
def test_against_the_oracle(T, fams, name):
    fam = fams(name)
    p = param(T)
    for label, ds, _, kws in fam.sets:
        held = [with_bc(d, d.vec_b, d.vec_c, rowabs=None) for d in ds]             # (|b|: the dense oracle's row sums)
        new = new_set(held)
        psd = [PSD in d.seg_type for d in new]
        ros = [_psd_run((name, label, q), d) if psd[q] else fam.oracle("seta-" + label, q, d, None) for q, d in enumerate(new)]
        for kw in kws:
            X = fam.make(held, p, **kw)
            try:
                X.run(10, poll_every=64)
                set_a(fam, X, held, new)
                done = 0
                for it in (0, 1, 9) + ((49,) if any(psd) else ()):
                    X.run(it + 1 - done, poll_every=64)
                    done = it + 1
                    for i, (ro, d) in enumerate(zip(ros, new)):
                        if it == 49 and not psd[i]:
                            continue
                        x, y = X.iterate(i)
                        rx, ry = _psd_snap(ro, d, it) if psd[i] else snap_xy(ro, d, it)
                        tol = iterate_tol(it, psd[i])
                        ex, ey = _rel(x, rx), _rel(y, ry)
                        print("seta %s %s %s problem %d iterate %d: err x %.2e y %.2e (tol %.2e)" % (name, label, kw, i, it, ex, ey, tol))
                        assert ex <= tol and ey <= tol, (name, label, i, it, ex, ey)
            finally:
                X.destroy()


# ---- 6. a sub-range -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_a_sub_range(T, fams, name):
    fam = fams(name)
    P, first, count = 300, 100, 100
    for kw0 in fam.sets[0][3]:
        cyc, kw = fam.cycled(0, P, kw0)
        olds = cyc[first:first + count]
        new = [perturbed_a(d, k, zeros=3 if k % 7 == 0 else 0) for k, d in enumerate(olds)]
        p = param(T)
        X, Y, Z = (fam.make(cyc, p, **kw) for _ in range(3))
        try:
            if name in RAGGED:                                   # both thread classes lie inside the range (the set cycles)
                assert all(c["n_prob"] >= count // len(fam.sets[0][1]) for c in X.info()["classes"])
            for sb in (X, Y, Z):
                sb.run(10, poll_every=64)
            set_a(fam, X, olds, new, first=first)
            for k, d in enumerate(new):
                replace_a(fam, Y, first + k, olds[k], d)
            assert X.info()["live"] == P
            for sb in (X, Y, Z):
                sb.run(10, poll_every=64)
            for i in range(P):
                inside = first <= i < first + count
                same(full(X, i), full(Y if inside else Z, i), (name, str(kw0), i))
                assert X.status(i).iters == (10 if inside else 20)
        finally:
            for sb in (X, Y, Z):
                sb.destroy()


# ---- 7. a stopped slot runs again ---------------------------------------------------------------------------------------------------

def _f1_feasible(f1):
    """F1 (tests/tau_zero_problems.py: row 0 holds a.x = a.x0, the last row asks 2 a.x <= 2 a.x0 - gap) with its last row scaled by t
    so that t a.x0 = b_last - 1: x0 satisfies every row again.  The same pattern: the row stays dense"""
    from tau_zero_problems import _lp_layout
    a, G, x0, A, b_feas, _ = _lp_layout(64, 126, 1)
    A = np.array(A, np.float64)
    ax0 = float(a @ x0)
    assert abs(ax0) > 1e-3
    t = (float(f1.vec_b[-1]) - 1.0) / ax0
    A[-1] = t * a
    e = with_a(f1, np.asfortranarray(A.astype(F)).ravel(order="F"))
    assert np.all((np.asarray(e.mat_a) != 0) == (np.asarray(f1.mat_a) != 0))
    return e


@pytest.mark.parametrize("name", FAMILIES)
def test_a_stopped_slot_runs_again(T, fams, name):
    from tau_zero_problems import family as tz_family
    from totsu_amd import _lib
    fam = fams(name)
    label, ds, _, kws = fam.sets[0]
    f1 = _dense_of(tz_family("F1"))                              # the infeasible LP, 128 x 64: its iteration ends through tau = 0
    f1.vec_b_rowabs = None
    kw1 = {"nnz_caps": [0, 0]} if name == "raggedsparse" else {}
    cases = [("excess", ds, new_set(ds), param(T, max_iter=5), kw, _lib.ST_EXCESS_ITER, 0) for kw in kws] + \
            [("tau zero", [f1, f1], [_f1_feasible(f1)] * 2, param(T, eps_acc=1e-5, eps_inf=1e-5, max_iter=5000),
              dict(kw1, **{k: v for k, v in kw.items() if k != "nnz_caps"}), _lib.ST_INFEASIBLE, 1) for kw in kws]
    for what, held, new, p, kw, state, kind in cases:
        X, Y, W = (fam.make(held, p, **kw) for _ in range(3))
        try:
            for sb in (X, Y, W):
                res = sb.run(-1, poll_every=64)
                assert [r.state for r in res] == [state] * len(held) and res[0].kind == kind, (what, [(r.state, r.kind, r.iters) for r in res])
            raws = [W.raw_iterate(i) for i in range(len(held))]
            assert all((x[-1] <= 1e-12) == (kind == 1) for x, _ in raws)
            assert W.info()["live"] == 0
            set_a(fam, W, held, new, keep=True)                  # kept: the arena's iterate, running at iteration 0
            for i in range(len(held)):
                st = W.status(i)
                assert (st.state, st.iters, st.kind, tuple(st.cri)) == (RUNNING, 0, 0, (0.0, 0.0, 0.0)), (what, i)
                x, y = W.iterate(i)
                assert x[-1] == raws[i][0][-1] and y[-1] == raws[i][1][-1]
                nm = held[i].n + held[i].m                       # (the raw iterate is the arena's to one rounding: x_s, u, v exactly)
                assert np.array_equal(x[nm:], raws[i][0][nm:]) and np.array_equal(y, raws[i][1])
                assert np.allclose(x[:nm], raws[i][0][:nm], rtol=3e-7, atol=0)
            before = W.info()
            assert before["live"] == len(held)
            kept = [W.iterate(i) for i in range(len(held))]
            W.run(1, poll_every=1)                               # and it advances: launched, and the iterate moves
            after = W.info()
            assert after["workgroups"] - before["workgroups"] == len(held)
            for i in range(len(held)):
                x, y = W.iterate(i)
                assert not (np.array_equal(x, kept[i][0]) and np.array_equal(y, kept[i][1])), (what, i)
            set_a(fam, X, held, new)                             # fresh: the replace route, bit for bit
            for i, d in enumerate(new):
                replace_a(fam, Y, i, held[i], d)
            _walk(X, Y, len(held), (name, what, str(kw)), steps=(1, 4))
        finally:
            for sb in (X, Y, W):
                sb.destroy()


# ---- 8. replace, then set_a, then replace -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_replace_then_set_a_then_replace(T, fams, name):
    """the host's mirror of the slots' pointers (dense) and the recorded entry counts and patterns (sparse) follow the slot"""
    fam = fams(name)
    p = param(T)
    label, ds, _, kws = fam.sets[0]
    P = len(ds)
    for kw in kws:
        X, Y = fam.make(ds, p, **kw), fam.make(ds, p, **kw)
        try:
            # a replace that changes what the slots hold: each slot takes its problem with some entries dropped (sparse: another
            # pattern with fewer entries; dense: another buffer), then set_a speaks about THAT
            dropped = []
            for i, d in enumerate(ds):
                a = np.array(d.mat_a, F)
                nz = np.nonzero(a)[0]
                if nz.size > 8:
                    a[nz[::5]] = 0
                dropped.append(with_a(d, a))
            for sb in (X, Y):
                for i, d in enumerate(dropped):
                    fam.replace(sb, i, d)
            _walk(X, Y, P, (name, str(kw), "replace"), steps=(1, 5))
            one = new_set(dropped, base=20)
            dev = X.info()["device_bytes"]
            set_a(fam, X, dropped, one)
            for i, d in enumerate(one):
                replace_a(fam, Y, i, dropped[i], d)
            _walk(X, Y, P, (name, str(kw), "set_a"), steps=(1, 5))
            if fam.sparse and any(np.count_nonzero(d.mat_a) != np.count_nonzero(e.mat_a) for d, e in zip(ds, dropped)):
                with pytest.raises(ValueError):                  # the counts of the patterns the slots held before
                    set_a(fam, X, ds, new_set(ds))
            two = new_set(ds, base=40)                           # back to the full patterns by replace, and set_a on those
            for sb in (X, Y):
                for i, d in enumerate(two):
                    fam.replace(sb, i, d)
            three = [perturbed_a(d, 50 + i) for i, d in enumerate(two)]
            set_a(fam, X, two, three, keep=True)
            for i, d in enumerate(three):
                replace_a(fam, Y, i, two[i], d, start=Y.iterate(i))
            _walk(X, Y, P, (name, str(kw), "again"), steps=(1, 5))
            if not fam.sparse:
                assert X.info()["device_bytes"] >= dev
        finally:
            X.destroy()
            Y.destroy()


# ---- 9. sparse only: the blob -------------------------------------------------------------------------------------------------------

def _blob_problems():
    zeros = lengths_problem(False, 1)
    return [("rows", lengths_problem(False, 0)), ("cols", lengths_problem(True, 0)), ("zero", zero_problem()),
            ("identity", identity_problem(0)), ("rows-explicit-zeros", zeros)]


@pytest.mark.parametrize("name", SPARSE)
def test_the_blob_after_set_a_is_the_packed_blob(T, fams, name):
    import scipy.sparse as sp
    from totsu_amd import sparsebatch
    fam = fams(name)
    p = param(T)
    cases = _blob_problems()
    groups = [[d] for _, d in cases] if name == "sparse" else [[d for _, d in cases]]
    labels = [[l] for l, _ in cases] if name == "sparse" else [[l for l, _ in cases]]
    for ds, ls in zip(groups, labels):
        for resident in (None, 0):
            kw = {} if resident is None else {"force_resident": 0}
            X, Y = fam.make(ds, p, **kw), fam.make(ds, p, **kw)
            try:
                new = [perturbed_a(d, 70 + i, zeros=5 if "zeros" in l else 0) for i, (d, l) in enumerate(zip(ds, ls))]
                for i, d in enumerate(ds):                       # as created: the packed blob
                    assert np.array_equal(X.blob(i), sparsebatch.pack(d.n, d.m, csc_of(d))[0]), (ls[i], "created")
                X.run(3, poll_every=3)
                set_a(fam, X, ds, new)
                for i, (d, e) in enumerate(zip(ds, new)):
                    want = sparsebatch.pack(d.n, d.m, triple_at(d, e))[0]
                    got = X.blob(i)
                    assert got.size == want.size and np.array_equal(got, want), (name, ls[i], resident, int((got != want).sum()))
                # a scipy matrix of the same pattern: accepted, the same bits as the values array
                mats = []
                for d, e in zip(ds, new):
                    cp, ri, va = triple_at(d, e)
                    mats.append(sp.csc_matrix((va, ri, cp), shape=(d.m, d.n)))
                Y.run(3, poll_every=3)
                Y.set_a(mats)
                for i in range(len(ds)):
                    assert np.array_equal(Y.blob(i), X.blob(i)), (ls[i], "scipy")
                _walk(X, Y, len(ds), (name, str(ls), resident), steps=(1, 5))
            finally:
                X.destroy()
                Y.destroy()


# ---- 10. dense only: an A that starts 4 bytes off a 16-byte boundary ------------------------------------------------------------------

def test_unaligned_a_in_a_device_buffer(T):
    """m % 4 == 0 with every A one float off a 16-byte boundary, in a DeviceBuffer of the caller's: set_a writes that buffer in
    place, is bitwise the replace route, and the load path info() reports is unchanged"""
    ds = [_edge(160, 96, s) for s in range(2)]
    new = new_set(ds)
    p = param(T)
    f = np.float32
    a = np.stack([np.asarray(d.mat_a, f).ravel() for d in ds])
    b = np.stack([np.asarray(d.vec_b, f) for d in ds])
    c = np.stack([np.asarray(d.vec_c, f) for d in ds])
    base = T.DeviceBuffer.from_host(np.concatenate([np.zeros(1, F), a.ravel(), np.zeros(3, F)]))
    assert base.ptr % 16 == 0
    X = T.MidBatchSolver(96, 160, _View(T, base, 1, a.size), b, c, ds[0].seg_type, ds[0].seg_len, p)
    Y = T.MidBatchSolver(96, 160, a, b, c, ds[0].seg_type, ds[0].seg_len, p)
    try:
        assert (X.info()["load_bytes"], Y.info()["load_bytes"]) == (4, 16)
        X.run(10, poll_every=10)
        Y.run(10, poll_every=10)
        dev = X.info()["device_bytes"]
        X.set_a([d.mat_a for d in new], keep_iterate=True)
        for i, d in enumerate(new):
            Y.replace(i, d.mat_a, d.vec_b, d.vec_c, start=Y.iterate(i))
        assert X.info()["load_bytes"] == 4 and X.info()["device_bytes"] == dev
        _walk(X, Y, 2, ("unaligned",), steps=(1, 10))
        got = base.to_host()                                     # the caller's buffer holds the new A, its neighbours untouched
        assert got[0] == 0 and not got[1 + a.size:].any()
        assert np.array_equal(got[1:1 + a.size], np.concatenate([np.asarray(d.mat_a, f) for d in new]))
    finally:
        X.destroy()
        Y.destroy()
        base.free()


# ---- 11. refusals -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", FAMILIES)
def test_refusals(T, fams, name):
    import scipy.sparse as sp
    from totsu_amd import _lib
    fam = fams(name)
    label, ds, _, kws = fam.sets[0]
    new = new_set(ds)
    P = len(ds)
    for kw in kws:
        sb = fam.make(ds, param(T), **kw)
        try:
            sb.run(2, poll_every=2)
            info = sb.info()
            dev, dev_all = info["device_bytes"], info["device_bytes_all"]
            want = [full(sb, i) for i in range(P)]
            blobs = [sb.blob(i) for i in range(P)] if fam.sparse else None
            mats = [values_at(o, d) for o, d in zip(ds, new)] if fam.sparse else [np.array(d.mat_a, F) for d in new]

            def unchanged():
                now = sb.info()
                assert (now["device_bytes"], now["device_bytes_all"], now["live"]) == (dev, dev_all, P)
                for i in range(P):
                    same(full(sb, i), want[i])
                    if blobs is not None:
                        assert np.array_equal(sb.blob(i), blobs[i])

            def bad(match, *a, **k):
                with pytest.raises(ValueError, match=match):
                    sb.set_a(*a, **k)
                unchanged()
            last = P - 1
            big = max(range(P), key=lambda i: mats[i].size)
            bad("problem %d" % last, mats[:last] + [np.append(mats[last], F(1))])              # a wrong length, naming the problem
            if mats[big].size > 1:
                bad("problem %d" % big, mats[:big] + [mats[big][:-1]] + mats[big + 1:])        # (sparse: a count off by one)
                for v in (np.nan, np.inf, -np.inf):
                    poisoned = mats[big].copy()
                    poisoned[poisoned.size // 2] = v
                    bad("problem %d: a value of A is not finite" % big, mats[:big] + [poisoned] + mats[big + 1:])
            bad("no problems", mats, first=1)                                                   # a range past the end
            bad("no problems", mats[:1], first=P)
            bad("no problems", mats[:1], first=-1)
            bad("at least one", [])                                                             # an empty list
            if fam.sparse:                                                                      # a scipy matrix with one entry moved
                cp, ri, va = triple_at(ds[0], new[0])                                          # (sparse40x30: columns neither empty nor full)
                big, d = 0, ds[0]
                col = int(np.nonzero((np.diff(cp) >= 1) & (np.diff(cp) < d.m))[0][0])
                free = sorted(set(range(d.m)) - set(ri[cp[col]:cp[col + 1]].tolist()))
                moved = ri.copy()
                moved[cp[col]:cp[col + 1]] = np.sort(np.append(ri[cp[col]:cp[col + 1]][1:], free[0]))
                bad("replace", [sp.csc_matrix((va, moved, cp), shape=(d.m, d.n))], first=big)
            # the C entry point itself: the same refusals, THIP_E_INVALID, nothing touched
            fn = getattr(_lib.load(), sb._prefix + "set_a")
            flat = np.concatenate(mats).astype(F)
            counts = np.array([a.size for a in mats], np.int64)
            pv, pc = flat.ctypes.data, counts.ctypes.data
            for args in ((sb.h, P, 1), (sb.h, 0, 0), (sb.h, 0, -1), (sb.h, -1, 1), (sb.h, 0, P + 1), (None, 0, 1)):
                assert fn(args[0], args[1], args[2], pv, pc, 0) == _lib.E_INVALID, args
            if flat.size:
                assert fn(sb.h, 0, P, None, pc, 0) == _lib.E_INVALID
                off = counts.copy()
                off[big] += 1
                assert fn(sb.h, 0, P, pv, off.ctypes.data, 1) == _lib.E_INVALID
                nan = flat.copy()
                nan[-1] = np.nan
                assert fn(sb.h, 0, P, nan.ctypes.data, pc, 0) == _lib.E_INVALID
                assert fn(sb.h, 0, P, nan.ctypes.data, None, 1) == _lib.E_INVALID
            unchanged()
            sb.run(2, poll_every=2)                              # and the batch still runs, and takes a set_a (counts: NULL too)
            assert [sb.status(i).iters for i in range(P)] == [4] * P
            assert fn(sb.h, 0, P, pv, None, 0) == 0
            assert [s.iters for s in sb.statuses()] == [0] * P
            sb.set_a(mats)
            assert [s.iters for s in sb.statuses()] == [0] * P
        finally:
            sb.destroy()
