"""GPU: the on-chip PSD projection of the own-A batches (sp_project, thip_sdpcones.h) on the hard spectra of tests/psd_spectra.py, in
every form the batches run it in: the old probe (thip_test_sdpbatch_project: 256 threads, x in device memory, a kernel built for 256)
and the four forms of thip_test_sdpbatch_project_form -- 256 | 1024 threads x (x in device memory as the wide batches have it | x
in LDS as every other batch has it), from kernels built for 1024-thread workgroups as the iteration kernels are.

One test is one order: both sides of every change of the K walk (nk = ceil(k / 8) * 4 MFMA steps), of the operands' extent (32 | 33)
and of the live quadrants, and order 20 for the golden iterate.  The reference is eigh in f64 on the f32-rounded input; the bound,
2e-6 ||x||, is the one the chain is held to in tests/test_gpu_eig.py::test_psd_projection_band_edge_regression (the same
coefficients, the same MFMA); tests/test_psd_spectra_cpu.py shows the plain f32 arithmetic within half of it."""
import numpy as np
import pytest

import psd_spectra as PS
from ownbatch_cases import T  # noqa: F401
from psd_spectra import F, tri

pytestmark = pytest.mark.gpu

TOL = 2e-6
OLD = ("old hook", None, None)
FORMS = [OLD] + [("%d threads, %s" % (t, "LDS" if lds else "global"), t, lds) for t in (256, 1024) for lds in (0, 1)]


def _project(T, form, k, xs, rxs=None):
    """the packed matrices xs (count x k (k + 1) / 2) through one form in ONE launch -> the projections[, the rx]"""
    from totsu_amd._lib import lib
    xs = np.ascontiguousarray(xs, dtype=F).reshape(-1, tri(k))
    dx = T.DeviceBuffer.from_host(xs)
    dr = None if rxs is None else T.DeviceBuffer.from_host(np.ascontiguousarray(rxs, dtype=F))
    rp = None if dr is None else dr.ptr
    if form[1] is None:
        lib.thip_test_sdpbatch_project(k, xs.shape[0], dx.ptr, rp)
    else:
        lib.thip_test_sdpbatch_project_form(k, xs.shape[0], form[1], form[2], dx.ptr, rp)
    out = dx.to_host().reshape(xs.shape)
    dx.free()
    if dr is None:
        return out
    r = dr.to_host().reshape(xs.shape)
    dr.free()
    return out, r


_CACHE = {}


def _inputs(k):
    """the cases of order k: tags, the packed f32 matrices, their norms and the f64 references (computed once, never written to)"""
    if k not in _CACHE:
        tags, mats = zip(*PS.cases(k, 0))
        xs = np.stack([PS.packed(m).astype(F) for m in mats])
        ref = np.stack([PS.reference(x, k) for x in xs])
        nrm = np.linalg.norm(xs.astype(np.float64), axis=1)
        for a in (xs, ref, nrm):
            a.setflags(write=False)
        _CACHE[k] = (tags, xs, nrm, ref)
    return _CACHE[k]


@pytest.mark.parametrize("k", sorted(PS.ORDERS + [PS.GOLDEN_ORDER]))
def test_hard_spectra_in_every_form(T, k):
    """Per form and case: finite, within 2e-6 ||x|| of the f64 reference, rx == rx0 - 2 got bitwise.  Per form: Moreau from the
    kernel's outputs alone (P(M) - P(-M) = M within 4e-6 ||M||: twice the tolerance, P(-M) from the same launch), idempotence within
    2e-6 ||M||, the exactly zero rows and columns of the zero-block family exactly zero.  Across forms, bitwise: the old hook ==
    (256, global); (T, LDS) == (T, global) for both T.  256 and 1024 threads add the norm in different orders and are each held to
    the f64 bound alone."""
    tags, xs, nrm, ref = _inputs(k)
    n = len(tags)
    fams = np.array([PS.family_of(t) for t in tags])
    both = np.concatenate([xs, -xs])
    rx0 = np.random.default_rng(k).standard_normal(both.shape).astype(F)
    out = {}
    for form in FORMS:
        got, rx = _project(T, form, k, both, rx0)
        again = _project(T, form, k, got[:n])
        out[form[0]] = (got, again)
        assert np.all(np.isfinite(got)) and np.all(np.isfinite(again)), form[0]
        pos, neg = got[:n].astype(np.float64), got[n:].astype(np.float64)
        err = np.abs(pos - ref).max(axis=1) / nrm
        moreau = np.abs(pos - neg - xs).max(axis=1) / nrm
        idem = np.abs(again.astype(np.float64) - pos).max(axis=1) / nrm
        for fam in dict.fromkeys(fams):
            s = fams == fam
            print("sp_project k = %2d %-20s %-22s err %.2e Moreau %.2e idempotence %.2e (of ||x||; tol %.0e)"
                  % (k, form[0], fam, err[s].max(), moreau[s].max(), idem[s].max(), TOL))
        bad = int(np.argmax(err))
        assert err[bad] <= TOL, (form[0], tags[bad], err[bad])
        bad = int(np.argmax(moreau))
        assert moreau[bad] <= 2 * TOL, (form[0], tags[bad], moreau[bad])
        bad = int(np.argmax(idem))
        assert idem[bad] <= TOL, (form[0], tags[bad], idem[bad])
        assert np.array_equal(rx, rx0 - F(2.0) * got), form[0]    # the reflection that rides in the pack
        h = k // 2
        for i in np.flatnonzero(fams == "zero block"):
            for g in (got[i], got[n + i], again[i]):
                m = PS.unpacked(g, k)
                assert not m[h:].any() and not m[:, h:].any(), (form[0], tags[i])
    for a, b in (("old hook", "256 threads, global"), ("256 threads, LDS", "256 threads, global"),
                 ("1024 threads, LDS", "1024 threads, global")):
        for u, v in zip(out[a], out[b]):
            assert np.array_equal(u, v), (a, b, tags[int(np.argmax((u != v).any(axis=1))) % n])


@pytest.mark.parametrize("k", [17, 49])
def test_a_batch_of_mixed_cases_is_each_one_alone(T, k):
    """tests/test_gpu_sdpbatch.py::test_a_batch_of_projections_is_each_one_alone, in the (1024, LDS) form on a mix of the families"""
    form = ("1024 threads, LDS", 1024, 1)
    tags, xs, _, _ = _inputs(k)
    pick = list(range(0, len(tags), 7))                            # 16 draws per family: every family, another draw each time round
    assert {PS.family_of(tags[i]) for i in pick} == set(PS.FAMILIES)
    rx0 = np.random.default_rng(k).standard_normal((len(pick), tri(k))).astype(F)
    got, rx = _project(T, form, k, xs[pick], rx0)
    for j, i in enumerate(pick):
        g1, r1 = _project(T, form, k, xs[i], rx0[j])
        assert np.array_equal(g1[0], got[j]) and np.array_equal(r1[0], rx[j]), tags[i]


def test_the_form_hook_refuses_what_it_does_not_run(T):
    from totsu_amd import _lib
    from totsu_amd._lib import lib
    x = np.ones(tri(64), F)
    d = T.DeviceBuffer.from_host(x)
    for k, count, threads, in_lds, ptr in [(0, 1, 256, 0, d.ptr), (65, 1, 256, 0, d.ptr), (-1, 1, 1024, 1, d.ptr), (8, 0, 256, 0, d.ptr),
                                           (8, 1, 256, 0, None), (8, 1, 0, 0, d.ptr), (8, 1, 64, 0, d.ptr), (8, 1, 512, 1, d.ptr),
                                           (8, 1, 2048, 0, d.ptr), (8, 1, 256, 2, d.ptr), (8, 1, 1024, -1, d.ptr)]:
        with pytest.raises(_lib.ThipError) as e:
            lib.thip_test_sdpbatch_project_form(k, count, threads, in_lds, ptr, None)
        assert e.value.code == _lib.E_INVALID and _lib.load().thip_last_error(), (k, count, threads, in_lds)
    assert np.array_equal(d.to_host(), x)                          # nothing ran
    d.free()
