"""CPU: the hard spectra of tests/psd_spectra.py are what they say, and the arithmetic of the on-chip PSD projection (proj32: sp_project
of thip_sdpcones.h restated in numpy f32) stays within 1e-6 ||M||_F of the f64 reference on every one of them -- half of the 2e-6 the
kernel itself is held to in tests/test_gpu_sdpcones_spectra.py, so that tolerance is reachable by the arithmetic alone."""
import numpy as np
import pytest

import psd_spectra as PS
from psd_spectra import F

ALL = sorted(PS.ORDERS + [PS.GOLDEN_ORDER])


def test_packing_round_trip():
    rng = np.random.default_rng(0)
    for k in (1, 2, 5):
        b = rng.standard_normal((k, k))
        s = (b + b.T) / 2
        x = PS.packed(s)
        want = [s[r, c] * (np.sqrt(2.0) if r != c else 1.0) for c in range(k) for r in range(c + 1)]      # cone_psd.rs
        assert x.shape == (PS.tri(k),) and np.array_equal(x, np.array(want))
        assert np.allclose(PS.unpacked(x, k), s, rtol=0, atol=1e-15)
        assert abs(np.linalg.norm(x) - np.linalg.norm(s)) <= 1e-14


@pytest.mark.parametrize("k", ALL)
def test_the_generator_builds_what_it_says(k):
    seen = {}
    for tag, m, w in PS.spectra(k, 0):
        fam = PS.family_of(tag)
        seen[fam] = seen.get(fam, 0) + 1
        assert m.shape == (k, k) and m.dtype == np.float64 and np.array_equal(m, m.T), tag
        if w is not None:
            assert np.abs(np.linalg.eigvalsh(m) - np.sort(w)).max() <= 1e-12 * np.abs(w).max(), tag
        if fam == "zero block":
            assert not m[k // 2:].any() and not m[:, k // 2:].any() and m[: k // 2, : k // 2].any()
        if fam == "low-rank PSD":
            assert np.count_nonzero(w) == k // 4 and w.min() == 0.0
        if fam in ("graded", "graded positive", "graded negative", "sweep"):
            assert np.abs(w).max() == 1.0 and np.abs(w).min() >= 0.999 * (1e-6 if fam == "sweep" else 1e-8)
    want = {f: PS.DRAWS for f, least in PS.FAMILIES.items() if k >= least}
    if k == PS.GOLDEN_ORDER:
        want["golden"] = 2
    if k in PS.SWEEP_ORDERS:
        want["sweep"] = 150
    assert seen == want
    assert [t for t, _ in PS.cases(k, 0)] == [t for t, _, _ in PS.spectra(k, 0)]


def test_every_family_and_every_order_is_produced():
    fams = set()
    for k in PS.ORDERS:
        got = {PS.family_of(t) for t, _ in PS.cases(k, 0)}
        assert got, k
        fams |= got
    assert fams == set(PS.FAMILIES) | {"sweep"}
    assert all(set(PS.FAMILIES) <= {PS.family_of(t) for t, _ in PS.cases(k, 0)} for k in PS.ORDERS if k >= 4)
    assert set(PS.SWEEP_ORDERS) <= set(PS.ORDERS) and PS.GOLDEN_ORDER not in PS.ORDERS
    # another seed, other matrices
    a, b = dict(PS.cases(9, 0)), dict(PS.cases(9, 1))
    assert a.keys() == b.keys() and not np.array_equal(a["graded/0"], b["graded/0"])


@pytest.mark.parametrize("k", ALL)
def test_the_f32_arithmetic_reaches_half_the_gpu_tolerance(k):
    worst = {}
    for tag, m in PS.cases(k, 0):
        x = PS.packed(m).astype(F)
        nrm = np.linalg.norm(x.astype(np.float64))
        ref = PS.reference(x, k)
        got = PS.proj32_packed(x, k)
        assert got.dtype == F and np.all(np.isfinite(got)), tag
        if tag.endswith("/0"):
            assert np.array_equal(PS.proj32(m), got), tag
        err = np.abs(got - ref).max() / nrm
        again = np.abs(PS.proj32_packed(got, k) - got).max() / nrm
        moreau = np.abs(got.astype(np.float64) - PS.proj32_packed(-x, k) - x).max() / nrm
        fam = PS.family_of(tag)
        worst[fam] = np.maximum(worst.get(fam, 0.0), [err, again, moreau])
        assert err <= 1e-6, (tag, err)
        assert again <= 1e-6 and moreau <= 2e-6, (tag, again, moreau)
    for fam, (e, i, mo) in worst.items():
        print("proj32 k = %2d %-22s err %.2e idempotence %.2e Moreau %.2e (of ||M||_F)" % (k, fam, e, i, mo))
