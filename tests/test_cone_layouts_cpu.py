"""CPU: the cone layouts of tests/cone_layouts.py against the f64 oracle alone.  The constructed points are feasible and
complementary; at the iterates the GPU tests compare, the oracle itself puts every (cone type, length) of every layout into all
three branches of the second-order projection (a condition: a layout or seed that loses a branch fails here, before any device
runs it), stays on the tau > 0 branch, and the shape rules send every layout to the family its GPU legs assert."""
import numpy as np
import pytest

import cone_layouts as CL
import oracle as O
from totsu_amd import midbatch as MB
from totsu_amd import sdpbatch as SP
from totsu_amd import smallbatch as SB

RUNS = [(name, seed, inst) for name, L in CL.LAYOUTS.items() for seed in L["seeds"] for inst in L["instances"]]
_ids = ["%s-seed%d-inst%d" % r for r in RUNS]


def _in_cone(t, x, tol):
    """membership of one segment, in f64: 0 outside by more than tol (relative to the segment's size)"""
    x = np.asarray(x, dtype=np.float64)
    scale = max(np.abs(x).max(initial=0.0), 1.0)
    if t == CL.P or x.size <= 1:
        return bool((x >= -tol * scale).all())
    if t == CL.R:
        x = CL.rot(x)
    return bool(x[0] - np.linalg.norm(x[1:]) >= -tol * scale)


def test_layouts_are_what_they_claim():
    for name in CL.LAYOUTS:
        st, sl, beg = CL.segments(name)
        n, m = CL.LAYOUTS[name]["n"], sum(sl)
        cones = [(t, l, b) for t, l, b in zip(st, sl, beg) if t in (CL.S, CL.R)]
        lens = {t: sorted({l for t_, l, _ in cones if t_ == t}) for t in (CL.S, CL.R)}
        if name in ("small", "mid"):
            assert set(lens[CL.S]) >= {0, 1, 2, 3, 64, 65, 66, 129, 130} and set(lens[CL.R]) >= {1, 2, 3, 4, 65, 66, 129, 130}
            starts = [b % 4 for t, l, b in cones if l > 0]
            assert all(starts.count(r) >= 2 for r in (1, 2, 3)), starts                 # several block cones off the multiples of 4
            assert st[-1] == CL.Z and CL.Z in st[1:-1]                                  # a zero segment at the end and one inside
            assert any(a == b_ and a[0] in (CL.S, CL.R) and 0 < a[1] <= 4 for a, b_ in zip(zip(st, sl), zip(st[1:], sl[1:])))
            assert (m * n <= 24576) == (name == "small") and (name == "small" or (n >= 96 and 8 * n + 13 * m <= 32768))
        if name.startswith("short_soc"):
            plain = [l for t, l in zip(st, sl) if t == CL.S]
            assert n >= 96 and max(plain) == 129 and {0, 1, 2, 128, 129} <= set(plain)
            assert sum(plain) + (2 if name.endswith("rot") else 0) == m                 # every row in a cone; one rotated cone of 2
            assert [(t, l) for t, l in zip(st, sl) if t != CL.S] == ([(CL.R, 2)] if name.endswith("rot") else [])
        if name == "long":
            assert n == 100 and {2048, 2049, 1, 2, 300} <= set(lens[CL.S]) and {2048, 2049, 1, 2, 300} <= set(lens[CL.R])
            assert CL.P in st
        if name.startswith("psd"):
            orders = [int(round((np.sqrt(8 * l + 1) - 1) / 2)) for t, l in zip(st, sl) if t == CL.PSD]
            assert (st[0], sl[0]) == (CL.P, 3) and set(orders) >= {1, 2, 3, 32, 33}
            assert (set(orders) >= {64, 65}) == (name == "psd_big")
            assert all(b % 4 != 0 for t, b in zip(st, beg) if t == CL.PSD)
            # SOC 17, rotated 5, 1, 2 and a zero segment; the rotated cone of 2 rows a second time, for the boundary target
            assert [(t, l) for t, l in zip(st, sl) if t in (CL.S, CL.R, CL.Z)] == \
                [(CL.S, 17), (CL.R, 5), (CL.R, 1), (CL.R, 2), (CL.R, 2), (CL.Z, 2)]


@pytest.mark.parametrize("name,seed,inst", RUNS, ids=_ids)
def test_constructed_point_is_feasible_and_complementary(name, seed, inst):
    d = CL.build(name, seed, inst)
    st, sl, beg = CL.segments(name)
    A = np.asarray(d.mat_a, dtype=np.float64).reshape((d.n, d.m)).T
    other = np.concatenate([np.full(l, t != CL.PSD) for t, l in zip(st, sl)])
    # primal: b - A x0 = s0 on every row that is no PSD row, s0 in the cone; the f32 b the solvers get is that b rounded
    r = d.b64 - A @ d.x0 - d.s0
    assert np.abs(r[other]).max() <= 1e-12 * max(np.abs(d.b64).max(), 1.0)
    assert np.abs(d.vec_b - d.b64).max() <= 2.0 ** -24 * np.abs(d.b64).max()
    assert np.abs(d.vec_c - d.c64).max() <= 2.0 ** -24 * np.abs(d.c64).max()
    if not CL.has_psd(name):
        assert np.abs(d.c64 + A.T @ d.y0).max() <= 1e-12 * max(np.abs(d.c64).max(), 1.0)      # dual: c + A^T y0 = 0
    seen = set()
    for i, (t, l, b0) in enumerate(zip(st, sl, beg)):
        s, y = d.s0[b0:b0 + l], d.y0[b0:b0 + l]
        if t == CL.PSD or l == 0:
            continue
        if t == CL.Z:
            assert not s.any()                                       # y0 is free
            continue
        assert _in_cone(t, s, 1e-12) and _in_cone(t, y, 1e-12), (i, t, l)
        assert abs(s @ y) <= 1e-12 * max(np.linalg.norm(s) * np.linalg.norm(y), 1.0), (i, t, l, s @ y)
        if t in (CL.S, CL.R):
            tg = CL.targets(name)[i]
            seen.add(tg)
            if l >= 2:
                want = {0: ("inside", "zero"), 1: ("zero", "inside"), 2: ("boundary", "boundary")}[tg]
                assert (CL.classify(t, s), CL.classify(t, y)) == want, (i, t, l, tg)
    assert seen == {0, 1, 2}


@pytest.mark.parametrize("name,seed,inst", RUNS, ids=_ids)
def test_oracle_alone_covers_every_branch(name, seed, inst):
    """over the compared iterates (a strict layout: those behind iterate 0, whose blocks are projections of the zero vector), over
    x_y and x_s: every (type, length) with two rows or more is seen at zero, inside and on the boundary, every cone of one row at
    zero and positive; no projected segment is outside its cone; kind == 0 throughout"""
    iters, _ = CL.iters_tols(name)
    d, ro = CL.oracle(name, seed, inst)
    assert ro.status == O.EXCESS_ITER and len(ro.trace) > max(iters)
    assert [ro.trace[it][1] for it in iters] == [0] * len(iters)
    assert all(ro.trace[it][0] == it for it in iters)
    strict = CL.LAYOUTS[name]["strict"]
    cov = CL.coverage(name, ro, strict=strict)
    st, sl, _ = CL.segments(name)
    assert set(cov) == {(CL.KIND[t], l) for t, l in zip(st, sl) if t in (CL.S, CL.R) and l > 0}
    for (kind, l), got in sorted(cov.items()):
        assert got == CL.wanted(l), (name, seed, inst, kind, l, sorted(got))
    if seed == CL.LAYOUTS[name]["seeds"][0] and inst == 0:
        # the table of NOTEBOOK.md: at which compared iterate the oracle first shows each branch
        first = {}
        for q, snap in enumerate(ro.snaps):
            if strict and iters[q] == 0:
                continue
            for _, kind, l, which, br in CL.branches(name, snap):
                first.setdefault((kind, l), {}).setdefault(br, "%d%s" % (iters[q], which))
        print("\n%s (m = %d, n = %d), seed %d: first compared iterate and block (y: x_y, s: x_s) of each branch" % (name, d.m, d.n, seed))
        for (kind, l), f in sorted(first.items()):
            print("  %s %4d: %s" % (kind, l, "  ".join("%s %s" % (b, f[b]) for b in sorted(f))))


class _Chosen(Exception):
    pass


def _refused(fits, d):
    try:
        fits(d.n, d.m, d.seg_type, d.seg_len)
    except ValueError:
        return True
    return False


@pytest.mark.parametrize("name", list(CL.LAYOUTS))
def test_conic_batch_sends_each_layout_to_its_family(name, monkeypatch):
    """small / mid / psd to the small / mid / SDP batch by the three rules alone (from_dense is caught before it needs a device);
    long is refused by all three, and so is psd_big (order 65)"""
    def spy(cls, denses, param=None, **kw):
        raise _Chosen(cls.__name__)
    monkeypatch.setattr(SB.SmallBatchSolver, "from_dense", classmethod(spy))
    seeds = CL.LAYOUTS[name]["seeds"]
    ds = [CL.build(name, s) for s in seeds]
    took = [not _refused(f, ds[0]) for f in (SB.fits, MB.fits, SP.fits)]
    want = {"small": "SmallBatchSolver", "mid": "MidBatchSolver", "psd": "SdpBatchSolver", "short_soc": "MidBatchSolver",
            "short_soc_rot": "MidBatchSolver"}.get(name)
    if want is None:
        assert took == [False, False, False]
        with pytest.raises(ValueError, match="FusedSolver"):
            SP.conic_batch(ds)
        return
    assert took == {"SmallBatchSolver": [True, True, True], "MidBatchSolver": [False, True, True],
                    "SdpBatchSolver": [False, False, True]}[want]
    with pytest.raises(_Chosen, match="^%s$" % want):
        SP.conic_batch(ds)
