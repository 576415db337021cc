"""CPU: what the ragged sparse batch decides without a device (thip_raggedsparse_fits, thip_test_raggedsparse_plan) against a numpy
restatement (tests/raggedsparse_cases.py::restate) -- over the set of the GPU tests and over a few hundred random (n, m, density,
layout) draws: the class split by the sparse batch's thread rule, the order of the live lists by entry count, the shared layouts,
the packed arena and the packed blobs (16-byte multiples, the running sum of the capacities), the LDS position of the resident copy
(the problem's own map and its own PSD tail), the resident flag, the classes' LDS -- and the stored form of every slot, the refusals
with the problem's index, and `fits` against `sparsebatch.fits` problem by problem."""
import re

import numpy as np
import pytest

import raggedsparse_cases as RC
from raggedsparse_cases import PSD, RPOS, SOC, ZERO, Shape, check_plan, restate
from sparse_cases import blob_of, csc_of
from ownbatch_cases import tri

from totsu_amd import _lib
from totsu_amd import raggedsparse as RS
from totsu_amd import sparsebatch as SB


def _sp(d):
    return RS.SparseProblem.of_dense(d)


def test_the_plan_of_the_set():
    ds = RC.shapes()
    nnz = [d.nnz for d in ds]
    assert len(ds) == 19 == len({(d.n, d.m) for d in ds})                  # every shape is the only one of its kind
    for force in (None, 256, 1024):
        for res in (None, 0, 1):
            check_plan(RS.plan(ds, force_threads=force, force_resident=res), restate(ds, nnz, None, force, res))
    pl = RS.plan(ds)
    by_name = dict(zip(["%s/%s" % s for s in RC.SET], range(len(ds))))
    big, bigger = by_name["sparse/lp1000x700"], by_name["sparse/lp2000x1000"]
    # too big to reside; lp2000x1000 is the largest map there is.  By the rule those two are the 1024-thread class; the fully dense
    # `mixed` is streamed among the resident members of the 256-thread class, and a forced size puts all of them into one class
    mixed = by_name["part/mixed"]
    assert [pl["resident"][p] for p in (big, bigger, mixed)] == [0, 0, 0] and sum(pl["resident"]) == len(ds) - 3
    assert [pl["cls"][p] for p in (big, bigger, mixed)] == [1, 1, 0] and pl["order"][1] == [bigger, big]
    assert [(c["n_prob"], c["n_resident"]) for c in pl["info"]["classes"]] == [(17, 16), (2, 0)]
    assert pl["info"]["classes"][1]["lds_bytes"] == RC.vector_bytes(ds[bigger]) == 162832
    for force, c in ((256, 0), (1024, 1)):
        f = RS.plan(ds, force_threads=force)["info"]["classes"]
        assert (f[c]["n_prob"], f[c]["n_resident"], f[c]["lds_bytes"]) == (19, 16, 162832) and f[1 - c]["n_prob"] == 0
    assert pl["info"]["max_psd_order"] == 33 and pl["info"]["psd_lds_bytes"] == 49920
    assert pl["order"][1][0] == bigger                                    # the most entries first


def test_capacities_beyond_the_entries():
    ds = RC.shapes()
    nnz = [d.nnz for d in ds]
    caps = [0] * len(ds)
    caps[0], caps[2], caps[12] = ds[0].m * ds[0].n, 8193, 24               # full; across the thread rule; the zero problem with room
    got = RS.plan(ds, nnz_caps=caps)
    check_plan(got, restate(ds, nnz, caps))
    assert got["cls"][2] == 1 and RS.plan(ds)["cls"][2] == 0
    assert got["blob_at"][1] == RC.capacity_bytes(ds[0].n, ds[0].m, 1200)


def _draw(rng):
    kind = rng.integers(0, 5)
    n = int(rng.integers(1, 1400))
    if kind == 0:
        m = int(rng.integers(1, 2200))
        st, sl = [RPOS], [m]
    elif kind == 1:
        a, b, c = (int(v) for v in rng.integers(0, 300, 3))
        st, sl = [ZERO, RPOS, SOC], [a, b, c + 1]
        m = a + b + c + 1
    elif kind == 2:
        k = int(rng.integers(1, 33))
        st, sl, m, n = [PSD, ZERO], [tri(k), k], tri(k) + k, min(n, tri(k))
    elif kind == 3:
        k = int(rng.integers(33, 50))
        st, sl, m, n = [RPOS, PSD], [3, tri(k)], tri(k) + 3, int(rng.integers(1, 40))
    else:
        m = int(rng.integers(1, 60))
        st, sl = [RPOS, RPOS], [m // 2, m - m // 2]
    density = float(rng.choice([0.0, 0.002, 0.01, 0.05, 0.3, 1.0]))
    return Shape(n, m, st, sl, int(round(density * m * n)))


def test_the_plan_of_random_draws():
    rng = np.random.default_rng(20)
    ds = []
    while len(ds) < 300:
        d = _draw(rng)
        try:
            SB.fits(d.n, d.m, d.seg_type, d.seg_len, d.nnz)
        except ValueError:
            continue
        ds.append(d)
    ds += [ds[3], ds[17], ds[3]]                                          # shared layouts
    nnz = [d.nnz for d in ds]
    caps = [int(c) for c in rng.choice([0, 0, 1], len(ds)) * np.minimum(np.array(nnz) + rng.integers(0, 500, len(ds)),
                                                                       [d.m * d.n for d in ds])]
    for kw in ({}, {"force_threads": 256}, {"force_threads": 1024, "force_resident": 0}, {"force_resident": 1}):
        got = RS.plan(ds, nnz_caps=caps, **kw)
        want = restate(ds, nnz, caps, kw.get("force_threads"), kw.get("force_resident"))
        check_plan(got, want)
        assert all(at % 16 == 0 for at in got["blob_at"])
        assert got["info"]["n_layouts"] < len(ds)
    got = RS.plan(ds, nnz_caps=caps)
    assert 0 < got["info"]["n_resident"] < len(ds) and all(c["n_prob"] for c in got["info"]["classes"])
    for d, at, c, r in zip(ds, got["lds_at"], [c or k for c, k in zip(caps, nnz)], got["resident"]):
        assert 4 * at == RC.vector_bytes(d) and r == int(4 * at + RC.capacity_bytes(d.n, d.m, c) <= RC.LDS_MAX)


def test_fits_is_the_sparse_batch_s_rule_problem_by_problem():
    ds = RC.shapes()
    got = RS.fits(ds)
    for d, g in zip(ds, got):
        assert g == SB.fits(d.n, d.m, d.seg_type, d.seg_len, d.nnz), (d.m, d.n)
    caps = [min(d.nnz + 9000, d.m * d.n) for d in ds]
    for d, c, g in zip(ds, caps, RS.fits(ds, caps)):
        assert g == SB.fits(d.n, d.m, d.seg_type, d.seg_len, c), (d.m, d.n, c)
    # and with the matrices themselves: the count is the matrix's
    host = [_sp(RC.host_problem(j)) for j in range(len(RC.SET)) if RC.host_problem(j) is not None]
    assert RS.fits(host) == got[:len(host)]


def test_every_slot_s_stored_form_is_the_restated_blob():
    """the blob of every host-built problem of the set (the one packing both sparse families share) against the numpy restatement,
    and the room the plan gives it"""
    host = [RC.host_problem(j) for j in range(len(RC.SET)) if RC.host_problem(j) is not None]
    pl = RS.plan([_sp(d) for d in host])
    ends = pl["blob_at"][1:] + [pl["info"]["blob_bytes"]]
    for d, at, end in zip(host, pl["blob_at"], ends):
        words, long_len = SB.pack(d.n, d.m, csc_of(d))
        want = blob_of(d.n, d.m, *csc_of(d), long_len=long_len)
        assert np.array_equal(words, want), (d.m, d.n)
        assert end - at == SB.capacity_bytes(d.n, d.m, int(csc_of(d)[0][-1])) >= 4 * words.size and at % 16 == 0


def test_refusals_name_the_problem():
    ds = RC.shapes()
    bad_shapes = [(Shape(3, 2145, [PSD], [2145], 0), "above 64"), (Shape(8, 4097, [RPOS], [4097], 0), "4096"),
                  (Shape(1000, 2020, [RPOS], [2020], 0), "LDS"), (Shape(3, 7, [RPOS], [6], 0), "cover"),
                  (Shape(837, 1176, [PSD], [1176], 0), "LDS"), (Shape(3, 4, [RPOS], [4], 13), "= 12|is 12")]
    for bad, word in bad_shapes:
        for at in (0, 5, len(ds)):
            for fn in (RS.fits, RS.plan):
                with pytest.raises(ValueError, match="problem %d:" % at) as e:
                    fn(ds[:at] + [bad] + ds[at:] + [bad_shapes[0][0]])
                assert re.search(word, str(e.value)), (word, str(e.value))
                if fn is RS.fits:
                    assert e.value.problem == at
    with pytest.raises(ValueError, match="problem 2: .*nnz_cap 1201 exceeds m n = 1200"):
        RS.plan([ds[1], ds[1], ds[0]], nnz_caps=[0, 0, 1201])
    with pytest.raises(ValueError, match="problem 1: .*220 entries where nnz_cap is 10"):
        RS.plan([ds[1], Shape(30, 40, [RPOS], [40], 220)], nnz_caps=[0, 10])
    with pytest.raises(ValueError, match="nnz_caps holds 2 entries where 3 problems"):
        RS.plan(ds[:3], nnz_caps=[0, 0])
    with pytest.raises(ValueError, match="1 .. 1048576"):
        RS.fits([])
    with pytest.raises(ValueError, match="256 or 1024"):
        RS.plan(ds, force_threads=512)
    # the stored form, through the matrices: Python's own checks name the problem as the library's do
    d = RC.host_problem(0)
    cp, ri, va = csc_of(d)
    good = _sp(d)
    for mat, word in (((cp[:-1], ri, va), "colptr holds 30 entries"), ((cp, ri[:-1], va), "differ in length"),
                      (np.zeros((40, 30)), "triple or a scipy.sparse matrix")):
        with pytest.raises(ValueError, match="problem 1: .*%s" % word):
            RS.plan([good, RS.SparseProblem(30, 40, mat, d.vec_b, d.vec_c, [RPOS], [40])])


class _Stop(Exception):
    pass


def test_constructor_refusals_come_before_the_device(monkeypatch):
    S = RS.RaggedSparseBatchSolver

    def stop():
        raise _Stop()
    monkeypatch.setattr(_lib, "ensure_init", stop)
    host = [RC.host_problem(j) for j in (0, 3, 9, 12)]
    with pytest.raises(_Stop):
        S.from_dense(host)
    with pytest.raises(ValueError, match="1 .. 1048576 problems, not 0"):
        S([])
    with pytest.raises(ValueError, match="nnz_caps holds 3 entries where 4 problems"):
        S.from_dense(host, nnz_caps=[0, 0, 0])
    with pytest.raises(ValueError, match="problem 2: .*nnz_cap 2 exceeds m n = 1"):
        S.from_dense(host, nnz_caps=[0, 0, 2, 0])
    for kind in ("vec_b", "vec_c"):
        ps = [_sp(d) for d in host]
        setattr(ps[1], kind, np.asarray(getattr(ps[1], kind))[:-1])
        with pytest.raises(ValueError, match="problem 1: %s" % kind):
            S(ps)
    ps = [_sp(d) for d in host]
    ps[3].n, ps[3].m, ps[3].seg_type, ps[3].seg_len = 3, 2145, [PSD], [2145]
    ps[3].mat, ps[3].vec_b, ps[3].vec_c = (np.zeros(4, np.int64), [], []), np.zeros(2145), np.zeros(3)
    with pytest.raises(ValueError, match="problem 3: .*above 64"):
        S(ps)
    import totsu_amd
    assert totsu_amd.RaggedSparseBatchSolver is S
