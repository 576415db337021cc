"""Hard spectra for the on-chip PSD projection (sp_project, totsu_amd/csrc/thip_sdpcones.h), shared by tests/test_psd_spectra_cpu.py and
tests/test_gpu_sdpcones_spectra.py.  No GPU needed: the packing of cone_psd.rs, symmetric matrices with a prescribed spectrum at the
orders where the kernel changes path, the f64 reference, and a numpy f32 restatement of the kernel's arithmetic (proj32) that shows
what tolerance the arithmetic alone reaches.

The orders: both sides of every change of the K walk nk = ceil(k / 8) * 4 (8|9, 16|17, 24|25, 32|33, 40|41, 48|49, 56|57), the
change of the operands' extent at 32|33, the smallest and the largest.  Order 20 is that of the golden iterate
(tests/golden/psd_k20_band_edge_iterate.npy), which cases(20, ..) yields beside the families."""
import os

import numpy as np

F = np.float32
ORDERS = [1, 2, 7, 8, 9, 16, 17, 24, 25, 31, 32, 33, 40, 41, 48, 49, 56, 57, 63, 64]
GOLDEN_ORDER = 20
SWEEP_ORDERS = (24, 57)
DRAWS = 16
# family -> the smallest order at which it is not degenerate (graded: a second value beside the one that fixes the scale; low rank:
# k / 4 >= 1; pair: k / 3 >= 1; zero block: a graded leading block of order k / 2 >= 2)
FAMILIES = {"graded": 2, "graded positive": 1, "graded negative": 1, "two clusters": 2, "one large, rest +-1e-7": 2,
            "one large, rest -1e-4": 2, "PSD but one -1e-3": 2, "uniform": 2, "low-rank PSD": 4, "complementary pair": 3,
            "zero block": 4}


def tri(k):
    return k * (k + 1) // 2


def packed(M):
    """cone_psd.rs: the upper triangle column by column, off-diagonals times sqrt 2"""
    M = np.asarray(M)
    hi, lo = np.tril_indices(M.shape[0])                           # (0, 0), (1, 0), (1, 1), (2, 0), ..: entry hi (hi + 1) / 2 + lo
    return M[lo, hi] * np.where(hi == lo, 1.0, np.sqrt(2.0)).astype(M.dtype)


def unpacked(x, k):
    x = np.asarray(x)
    hi, lo = np.tril_indices(k)
    M = np.zeros((k, k), x.dtype)
    M[lo, hi] = x / np.where(hi == lo, 1.0, np.sqrt(2.0)).astype(x.dtype)
    M[hi, lo] = M[lo, hi]
    return M


def family_of(tag):
    return tag.split("/")[0]


def _orth(rng, k):
    q, _ = np.linalg.qr(rng.standard_normal((k, k)))
    return q


def _sym(q, w):
    m = (q * w) @ q.T
    return (m + m.T) / 2


def _logu(rng, lo, n):
    return np.exp(rng.uniform(np.log(lo), 0.0, n))


def spectra(k, seed):
    """(tag, M, w): M symmetric f64 of order k, w its intended spectrum (None where M is perturbed or not built from one)"""
    rng = np.random.default_rng([seed, k])
    for fam, least in FAMILIES.items():
        if k < least:
            continue
        for d in range(DRAWS):
            tag = "%s/%d" % (fam, d)
            q = _orth(rng, k)
            if fam in ("graded", "graded positive", "graded negative"):
                w = _logu(rng, 1e-8, k)
                w[0] = 1.0
                w *= rng.choice([-1.0, 1.0], k) if fam == "graded" else (1.0 if fam == "graded positive" else -1.0)
            elif fam == "two clusters":
                w = np.where(np.arange(k) < k // 2, -1.0, 1.0) * (1.0 + 1e-6 * rng.standard_normal(k))
            elif fam == "one large, rest +-1e-7":
                w = 1e-7 * rng.choice([-1.0, 1.0], k)
                w[0] = 1.0
            elif fam == "one large, rest -1e-4":
                w = np.full(k, -1e-4)
                w[0] = 1.0
            elif fam == "PSD but one -1e-3":
                w = rng.uniform(0.1, 1.0, k)
                w[0], w[k - 1] = 1.0, -1e-3
            elif fam == "uniform":
                w = np.linspace(-1.0, 1.0, k)
            elif fam == "low-rank PSD":
                w = np.zeros(k)
                w[: k // 4] = rng.uniform(0.5, 2.0, k // 4)
            elif fam == "complementary pair":
                # P - N, P and N PSD of rank k / 3 each on orthogonal ranges (columns of one q), and a symmetric perturbation
                r = k // 3
                w = np.zeros(k)
                w[:r], w[r: 2 * r] = _logu(rng, 1e-5, r), -_logu(rng, 1e-5, r)
                w[0] = 1.0
                e = rng.standard_normal((k, k))
                e = (e + e.T) / 2
                m = _sym(q, w)
                yield tag, m + 1e-7 * np.linalg.norm(m) / np.linalg.norm(e) * e, None
                continue
            elif fam == "zero block":
                h = k // 2
                wh = _logu(rng, 1e-8, h) * rng.choice([-1.0, 1.0], h)
                wh[0] = 1.0
                m = np.zeros((k, k))
                m[:h, :h] = _sym(_orth(rng, h), wh)
                yield tag, m, np.concatenate([wh, np.zeros(k - h)])
                continue
            yield tag, _sym(q, w), w
    if k == GOLDEN_ORDER:
        d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "psd_k20_band_edge_iterate.npy"))
        for z in range(2):
            yield "golden/%d" % z, unpacked(d[z].astype(np.float64), k), None
    if k in SWEEP_ORDERS:
        # tests/test_gpu_eig.py::test_psd_projection_band_edge_regression: every |lambda| / ||M||_F between 1e-6 and 1 gets hit closely
        rng = np.random.default_rng(5)
        q = _orth(rng, k)
        for trial in range(150):
            mag = np.exp(rng.uniform(np.log(1e-6), 0.0, k)) * rng.choice([-1.0, 1.0], k)
            mag[0] = 1.0                                           # one dominant value fixes the scale
            yield "sweep/%d" % trial, _sym(q, mag), mag


def cases(k, seed=0):
    for tag, m, _ in spectra(k, seed):
        yield tag, m


def reference(x32, k):
    """the projection of the f32-rounded packed input: eigh in f64, the positive part rebuilt -> packed f64"""
    ev, z = np.linalg.eigh(unpacked(np.asarray(x32, F).astype(np.float64), k))
    return packed((z * np.maximum(ev, 0.0)) @ z.T)


# the quintics of sp_project: 11 lifting steps (the first on 1.7 x), 3 minimax steps
_LIFT = (F(4.02942496), F(-3.82532605), F(0.95951948))
_FIRST = (_LIFT[0] * F(1.7), _LIFT[1] * F(4.913), _LIFT[2] * F(14.19857))
_MINIMAX = ((F(2.647997920), F(-1.945904487), F(0.440483961)), (F(1.967564378), F(-1.351306898), F(0.386705679)),
            (F(1.884943743), F(-1.269148602), F(0.384197480)))


def proj32_packed(x, k):
    """sp_project restated in numpy f32 on a packed f32 vector (the products are BLAS's, not the MFMA's: another order of additions)"""
    x = np.asarray(x, F)
    hi, lo = np.tril_indices(k)
    a0 = np.zeros((k, k), F)
    a0[lo, hi] = np.where(hi == lo, x * np.sqrt(F(2.0)), x)        # entry(): the vector's entries, the diagonal times sqrt 2
    a0[hi, lo] = a0[lo, hi]
    fro = F(np.sqrt(np.sum(a0.astype(np.float64) ** 2)))
    s = a0 / fro if fro > 0 else np.zeros_like(a0)
    eye = np.eye(k, dtype=F)
    for it in range(14):
        a, b, c = _FIRST if it == 0 else _LIFT if it < 11 else _MINIMAX[it - 11]
        y = s @ s.T
        s = (c * (y @ y) + b * y + a * eye) @ s
    s = (F(-0.5) * (s @ s.T) + F(1.5) * eye) @ s                   # one Newton-Schulz step
    z = a0 @ s
    out = F(0.5) * (a0 + F(0.5) * (z + z.T))
    assert out.dtype == F
    return np.where(hi == lo, out[lo, hi] / np.sqrt(F(2.0)), out[lo, hi]).astype(F)


def proj32(M):
    M = np.asarray(M)
    return proj32_packed(packed(M.astype(np.float64)).astype(F), M.shape[0])
