"""CPU: the accuracy contract of the tiled sparse products' fixed-point accumulators, checked on the numpy
restatement of the format (tests/sptile_numpy.py) -- one scale per out element, every stored entry rounded on its own -- for the
badly scaled matrices the GPU suite runs (tests/test_gpu_sparse_scaling.py)."""
import numpy as np
import pytest

import sptile_numpy as S

# (case, layout): every case on the single indexed tile; case D also on its own half-dense shape (rows of 3000 entries)
CASES = [(c, "single") for c in "ABCDF"] + [("D", "wide50")]


@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("case,layout", CASES)
def test_restated_accumulators_meet_the_elementwise_bound(case, layout, trans):
    a, x = S.scaled_case(case, layout, trans)
    ref, scale = S.reference(a, x, trans)
    model = S.SpTileModel(a)
    out = model.product(x, trans)
    worst = float((np.abs(out - ref) / (scale + 1e-300)).max())
    # the control: a plain f32 sum, entry after entry, has to pass the same bound -- it is fair
    ctrl = float((np.abs(S.f32_rowwise(a, x, trans) - ref) / (scale + 1e-300)).max())
    print("case %s %s %s: fixed point %.2e, plain f32 %.2e" % (case, layout, "T" if trans else "N", worst, ctrl))
    assert np.all(np.abs(S.f32_rowwise(a, x, trans) - ref) <= 1e-5 * scale + 1e-30)
    assert np.all(np.abs(out - ref) <= 1e-5 * scale + 1e-30)
    # the abs-mode sums that feed the preconditioner: 1e-5 per element, and no non-empty row / column sums to 0
    asum = model.product(None, trans, abs_mode=True)
    aref = np.asarray(abs(a.astype(np.float64)).sum(axis=0 if trans else 1)).ravel()
    assert np.allclose(asum, aref, rtol=1e-5, atol=0.0)
    assert np.all(asum[aref > 0] > 0)


@pytest.mark.parametrize("trans", [False, True])
def test_restated_accumulators_honour_the_documented_bound_beyond_the_window(trans):
    # a 1e6 spike in the in-vector over rows / columns of 10^+-6: the error of an out element that misses the spike is bounded by
    # the formula of include/totsu_f32hip.h -- 1e-5 (|A||x|)_i + 2^-G amax_i max|x|, G = 50 - 2 head_bits
    a, x = S.scaled_case("spike", "single", trans)
    ref, _ = S.reference(a, x, trans)
    model = S.SpTileModel(a)
    assert model.window_bits(trans) == 50 - 2 * S.head_bits((model.col_len if trans else model.row_len).max())
    err = np.abs(model.product(x, trans) - ref)
    assert np.all(err <= model.guarantee(x, trans) + 1e-30)


@pytest.mark.parametrize("case,layout", CASES + [("spike", "single"), ("B", "tall"), ("B", "lite")])
def test_no_partial_sum_reaches_the_conversion_bound(case, layout):
    # spt_add converts a term with one f64 fma: |term * scale| must stay below 2^51 -- for any grouping of an out element's
    # terms into register / wave sums, hence for the sum of the magnitudes of the longest row and column
    for trans in (False, True):
        a, x = S.scaled_case(case, layout, trans)
        model = S.SpTileModel(a)
        longest = (model.col_len if trans else model.row_len).max()
        assert longest <= 2 ** ((model.head_t if trans else model.head_n) - 1)
        assert model.largest_partial_sum(x, trans) < 2.0 ** S.FIX_BITS < S.ADD_LIMIT
        assert model.largest_partial_sum(None, trans, abs_mode=True) < 2.0 ** S.FIX_BITS
    # and by construction: 2^(head - 1) terms of less than 2^(e_i + ex) each, scaled by 2^(50 - head - ex - e_i)
    assert 2.0 ** (model.head_n - 1) * 2.0 ** (S.FIX_BITS - model.head_n) < S.ADD_LIMIT


def test_exponent_codes_fit_one_byte_and_bound_their_rows():
    amax = np.array([0.0, 1e-45, 2.0 ** -127, 2.0 ** -126, 0.75, 1.0, 3.4e38], np.float32)
    e = S.exponent_of(amax)
    assert np.all(e + 127 >= 1) and np.all(e + 127 <= 255)
    assert np.all(amax.astype(np.float64) < 2.0 ** e.astype(np.float64))
    assert list(e[:4]) == [-126, -126, -126, -125] and list(e[4:]) == [0, 1, 128]
    assert [S.head_bits(c) for c in (0, 1, 2, 3, 4, 5, 4096)] == [1, 1, 2, 3, 3, 4, 13]
