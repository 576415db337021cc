"""numpy restatement of the FIXED-POINT ACCUMULATORS of the tiled sparse products (totsu_amd/csrc/thip_sptile.hip: spt_scale,
spt_add and the final conversion of sp_tile_k): the scale of every out element, the rounding of every term, the
exact integer sum.  The device adds some terms in f32 registers before they reach an accumulator (a lane's four entries, a wave's
column, a dense tile's row); here EVERY stored entry is its own term -- the largest number of roundings the format allows.
Also the badly scaled test matrices that tests/test_gpu_sparse_scaling.py and tests/test_sptile_fixedpoint_cpu.py share.
Test infrastructure (host logic), not a fallback of the product."""
import functools

import numpy as np
import scipy.sparse as sp

FIX_BITS = 50           # bits of a partial sum below the sign (SPT_FIX_BITS)
ADD_LIMIT = 2.0 ** 51   # |term * scale| that spt_add's one-fma conversion can take
MIN_EXP = -126          # a row / column exponent is clamped from below (one byte: e + 127 in 1 .. 255)


def head_bits(longest):
    """ceil(log2(longest)) + 1: an out element receives at most 2^(head_bits - 1) terms"""
    b = 0
    while (1 << b) < max(int(longest), 1):
        b += 1
    return b + 1


def exponent_of(amax):
    """e with amax < 2^e (frexp), clamped to >= MIN_EXP; an empty row / column gets MIN_EXP"""
    amax = np.asarray(amax, dtype=np.float32)
    e = np.frexp(amax)[1].astype(np.int64)
    return np.where(amax > 0, np.maximum(e, MIN_EXP), MIN_EXP)


class SpTileModel:
    """the accumulator format of one stored matrix: exponents per row and per column, headroom bits of the two products"""

    def __init__(self, mat):
        self.csr = sp.csr_matrix(mat, dtype=np.float32)
        self.csr.sum_duplicates()
        assert np.isfinite(self.csr.data).all()         # (thip_sptile_create refuses a non-finite stored value)
        self.m, self.n = self.csr.shape
        a = abs(self.csr)
        self.row_amax = np.asarray(a.max(axis=1).toarray()).ravel().astype(np.float32)
        self.col_amax = np.asarray(a.max(axis=0).toarray()).ravel().astype(np.float32)
        self.row_exp, self.col_exp = exponent_of(self.row_amax), exponent_of(self.col_amax)
        self.row_len, self.col_len = np.diff(self.csr.indptr), np.bincount(self.csr.indices, minlength=self.n)
        self.head_n = head_bits(self.row_len.max() if self.m else 1)
        self.head_t = head_bits(self.col_len.max() if self.n else 1)

    def _side(self, trans):
        """(out index of every entry, in index of every entry, values, out exponents, head bits, out length)"""
        coo = self.csr.tocoo()
        if trans:
            return coo.col, coo.row, coo.data, self.col_exp, self.head_t, self.n
        return coo.row, coo.col, coo.data, self.row_exp, self.head_n, self.m

    def shifts(self, x, trans=False, abs_mode=False):
        """k_i: out element i accumulates round(term * 2^k_i)"""
        _, _, _, oexp, head, _ = self._side(trans)
        ex = 1                                          # abs mode: x = 1 < 2^1
        if not abs_mode:
            xmax = np.float32(np.abs(np.asarray(x, np.float32)).max()) if np.size(x) else np.float32(0)
            ex = int(np.frexp(xmax)[1]) if xmax > 0 else 0
        return FIX_BITS - head - ex - oexp

    def _terms(self, x, trans, abs_mode):
        oi, ii, v, _, _, olen = self._side(trans)
        k = self.shifts(x, trans, abs_mode)
        if abs_mode:
            p = np.abs(v)
        else:
            p = v * np.asarray(x, np.float32)[ii]       # the f32 product of the device
        return oi, np.ldexp(p.astype(np.float64), k[oi].astype(np.int32)), k, olen

    def product(self, x, trans=False, abs_mode=False):
        """A x (trans: A^T x; abs_mode: |A| 1) as the accumulators deliver it, f32"""
        if not abs_mode and not np.isfinite(np.asarray(x, np.float32)).all():
            return np.full(self.n if trans else self.m, np.nan, np.float32)
        oi, scaled, k, olen = self._terms(x, trans, abs_mode)
        q = np.rint(scaled)                             # the fma's round-to-nearest-even at the unit
        assert np.abs(q).max(initial=0.0) < ADD_LIMIT
        acc = np.bincount(oi, weights=q, minlength=olen)        # integers below 2^53: the f64 sums are exact
        assert np.abs(acc).max(initial=0.0) < 2.0 ** 53
        return np.ldexp(acc, (-k).astype(np.int32)).astype(np.float32)

    def largest_partial_sum(self, x, trans=False, abs_mode=False):
        """the largest |scaled partial sum| any grouping of an out element's terms can reach (what spt_add may be handed)"""
        oi, scaled, _, olen = self._terms(x, trans, abs_mode)
        return float(np.bincount(oi, weights=np.abs(scaled), minlength=olen).max(initial=0.0))

    def window_bits(self, trans=False):
        """G of the documented bound (include/totsu_f32hip.h beside thip_sptile_mv)"""
        return FIX_BITS - 2 * (self.head_t if trans else self.head_n)

    def guarantee(self, x, trans=False):
        """err_i <= 1e-5 (|A||x|)_i + 2^-G amax_i max|x|, amax_i = the largest |a| of out element i (at least 2^-127)"""
        x64 = np.abs(np.asarray(x, np.float32).astype(np.float64))
        a = abs(self.csr.astype(np.float64))
        ax = (a.T @ x64) if trans else (a @ x64)
        amax = np.maximum((self.col_amax if trans else self.row_amax).astype(np.float64), 2.0 ** (MIN_EXP - 1))
        return 1e-5 * ax + 2.0 ** -self.window_bits(trans) * amax * x64.max(initial=0.0)


# ---------------------------------------------------------------------------------------------------------------------------
# the badly scaled matrices: D1 R D2 with R a fixed random pattern of N(0, 1) entries
# ---------------------------------------------------------------------------------------------------------------------------
# case -> (decades of the OUT side's diagonal, decades of the IN side's diagonal, the in-vector).  The out side is the rows for
# the N product and the columns for the T product: a T-product case is the N-product case of the transposed scaling.
CASES = {
    "A": (3.5, 0.0, "spike1e3"),
    "B": (6.0, 0.0, "normal"),
    "C": (4.0, 4.0, "normal"),
    "D": (6.0, 0.0, "spike1e3"),
    "F": (6.0, 0.0, "loguniform4"),
}
# beyond the window (the stated limit): a 1e6 spike in the in-vector
SPIKE_CASE = (6.0, 0.0, "spike1e6")

LAYOUTS = {
    "single": ((3000, 2000), 0.02),         # one indexed tile
    "staged": ((9000, 6000), 0.01),         # 3 x 2 tiles of ~160 K entries: the staged instance
    "lite": ((64, 300000), 0.0015),         # 74 small tiles in one item: the flat walk of the LITE instance
    "full": ((8242, 4106), None),           # two full tiles without indices beside indexed ones (dense_n / dense_t)
    "tall": ((13000, 70), 0.9),             # tall dense columns: a wave's entries share a column (the wave sum of the T product)
    "wide50": ((2000, 6000), 0.5),          # case D's own: rows of 3000 entries
}


def with_full_tiles(rng):
    """8242 x 4106: tile (0, 0) full, (1, 0) 30 % random, (2, 0) = the last 50 rows, full but not of full height, (0, 1) = 4096 x 10
    full, (1, 1) empty, (2, 1) one entry (the construction of test_gpu_sparse._with_full_tiles)"""
    d = np.zeros((8242, 4106), dtype=np.float32)
    d[:4096, :4096] = rng.standard_normal((4096, 4096))
    blk = rng.standard_normal((4096, 4096))
    blk[rng.uniform(size=blk.shape) > 0.3] = 0.0
    d[4096:8192, :4096] = blk
    d[8192:, :4096] = rng.standard_normal((50, 4096))
    d[:4096, 4096:] = rng.standard_normal((4096, 10))
    d[8200, 4100] = 2.5
    return d


@functools.lru_cache(maxsize=None)
def _pattern(layout):
    shape, density = LAYOUTS[layout]
    rng = np.random.default_rng(1000 + sorted(LAYOUTS).index(layout))
    if density is None:
        r = sp.csr_matrix(with_full_tiles(rng))
    else:
        r = sp.random(shape[0], shape[1], density=density, format="csr", random_state=rng, dtype=np.float64)
        r.data = rng.standard_normal(r.nnz)
    r.sort_indices()
    return r.astype(np.float64)


def _in_vector(kind, length, rng):
    v = rng.standard_normal(length)
    if kind == "spike1e3":
        v[rng.integers(length)] = 1e3
    elif kind == "spike1e6":
        v[rng.integers(length)] = 1e6
    elif kind == "loguniform4":
        v = v * 10.0 ** rng.uniform(-4, 4, length)
    else:
        assert kind == "normal"
    return v.astype(np.float32)


def scaled_case(case, layout, trans, seed=0):
    """(matrix as f32 csr, in-vector f32) of a case for the N product (trans=False) or the T product: the out side of the product
    carries the case's first diagonal, the in side its second"""
    dec_out, dec_in, kind = SPIKE_CASE if case == "spike" else CASES[case]
    r = _pattern(layout)
    m, n = r.shape
    rng = np.random.default_rng([seed, sorted(LAYOUTS).index(layout), int(trans)] + [ord(ch) for ch in case])
    d_out = 10.0 ** rng.uniform(-dec_out, dec_out, n if trans else m)
    d_in = 10.0 ** rng.uniform(-dec_in, dec_in, m if trans else n) if dec_in else np.ones(m if trans else n)
    d_row, d_col = (d_in, d_out) if trans else (d_out, d_in)
    a = (sp.diags(d_row) @ r @ sp.diags(d_col)).tocsr().astype(np.float32)
    a.sort_indices()
    return a, _in_vector(kind, m if trans else n, rng)


def reference(a, x, trans=False):
    """(f64 product of the f32-rounded matrix and vector, |A||x|)"""
    a64, x64 = a.astype(np.float64), np.asarray(x, np.float32).astype(np.float64)
    if trans:
        a64 = a64.T
    return a64 @ x64, abs(a64) @ np.abs(x64)


def f32_rowwise(a, x, trans=False):
    """the plain f32 sum, entry after entry, of every out element: the control the elementwise bound has to be fair to"""
    b = (a.T if trans else a).tocsr().astype(np.float32)
    b.sort_indices()
    p = b.data * np.asarray(x, np.float32)[b.indices]
    out = np.zeros(b.shape[0], np.float32)
    for i in range(b.shape[0]):
        s = p[b.indptr[i]:b.indptr[i + 1]]
        if s.size:
            out[i] = np.cumsum(s, dtype=np.float32)[-1]
    return out
