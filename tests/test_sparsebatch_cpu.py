"""CPU: the sparse own-A batch's rule (thip_sparsebatch_fits), its stored form (thip_test_sparsebatch_pack against the numpy
restatement of tests/sparse_cases.py), every refusal of the stored form, and the Python routes into it -- triples, from_dense's
extraction, scipy matrices.  No device is needed by any of it."""
import numpy as np
import pytest

import sparse_cases as S
from sparse_cases import F, SPB_LONG

ZERO, RPOS, SOC, ROT, PSD = 0, 1, 2, 3, 4
LDS = 163840


@pytest.fixture(scope="module")
def SB():
    from totsu_amd import sparsebatch
    return sparsebatch


def tri(k):
    return k * (k + 1) // 2


def vec_bytes(n, m, tail):
    """the SDP batch's LDS map: 6208 + 8 n + 13 m floats, the class bytes, the PSD tail"""
    return 4 * (6208 + 8 * n + 13 * m) + ((m + 3) & ~3) + tail


def cap_bytes(n, m, nnz_cap):
    return (16 * nnz_cap + 4 * (2 * (m + n) + 4) + 15) & ~15


# ---- the rule ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,n,st,sl,tail", [(560, 528, [PSD, ZERO], [tri(32), 32], 0),
                                            (2000, 1000, [RPOS], [2000], 0),
                                            (1176, 48, [PSD], [tri(48)], 49920)])
def test_fits_on_the_boundary(SB, m, n, st, sl, tail):
    from totsu_amd import sdpbatch
    vec = vec_bytes(n, m, tail)
    assert sdpbatch.fits(n, m, st, sl)[0] == vec
    left = LDS - vec
    thr0 = 1024 if max(m, n) > 1024 else 256
    if cap_bytes(n, m, 0) > left:                                      # 2000 x 1000: the pointers alone do not fit beside the vectors
        assert (m, n) == (2000, 1000) and left == 1008
        assert SB.fits(n, m, st, sl, 0) == (vec, thr0, 0) and SB.fits(n, m, st, sl, 40000) == (vec, 1024, 0)
        return
    last = max(k for k in range(left // 16 + 1) if cap_bytes(n, m, k) <= left)          # the largest resident
    assert 0 < last < m * n and cap_bytes(n, m, last) <= left < cap_bytes(n, m, last + 1)
    lds, thr, res = SB.fits(n, m, st, sl, last)
    assert (lds, res) == (vec + cap_bytes(n, m, last), 1) and lds <= LDS
    assert SB.capacity_bytes(n, m, last) == cap_bytes(n, m, last)
    lds, thr, res = SB.fits(n, m, st, sl, last + 1)
    assert (lds, res) == (vec, 0)                                      # taken all the same: the entries stay in memory
    assert SB.fits(n, m, st, sl, 0) == (vec + cap_bytes(n, m, 0), thr0, 1)
    print("%d x %d: %d bytes beside the vectors, resident up to nnz_cap = %d" % (m, n, left, last))


def test_threads_rule(SB):
    assert SB.fits(1024, 1024, [RPOS], [1024], 8192)[1] == 256
    assert SB.fits(1024, 1024, [RPOS], [1024], 8193)[1] == 1024
    assert SB.fits(1024, 1025, [RPOS], [1025], 10)[1] == 1024
    assert SB.fits(1025, 1024, [RPOS], [1024], 10)[1] == 1024


def test_fits_passes_the_sdp_batch_s_refusals_through(SB):
    from totsu_amd import sdpbatch
    cases = [(10, 4097, [RPOS], [4097]), (4097, 10, [RPOS], [10]), (5, 7, [PSD], [7]), (5, tri(65), [PSD], [tri(65)]),
             (4096, 4096, [RPOS], [4096]), (5, 10, [RPOS], [9]), (40, 1653 + 400, [PSD, RPOS], [tri(57), 400])]
    for n, m, st, sl in cases:
        with pytest.raises(ValueError) as want:
            sdpbatch.fits(n, m, st, sl)
        with pytest.raises(ValueError) as got:
            SB.fits(n, m, st, sl, 0)
        tail = lambda e: str(e.value).split(": ", 1)[-1].split(" -> ")[0]       # (the message without file and line)
        assert tail(got) == tail(want), (n, m, tail(got), tail(want))
    with pytest.raises(ValueError, match="nnz_cap 31 exceeds m n = 30"):
        SB.fits(5, 6, [RPOS], [6], 31)
    assert SB.fits(5, 6, [RPOS], [6], 30)[2] == 1


# ---- the stored form -------------------------------------------------------------------------------------------------------------

def _random_csc(m, n, density, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m, n)).astype(F) * (rng.random((m, n)) < density)
    return A


def _csc(A):
    A = np.asarray(A, F)
    m, n = A.shape
    d = S._D(A, np.zeros(m), np.zeros(n), [RPOS], [m])
    return S.csc_of(d)


def _sections(w, n, m):
    nnz = int(w[n])
    ce = w[n + 1:n + 1 + 2 * nnz]
    rptr = w[n + 1 + 2 * nnz:n + 1 + 2 * nnz + m + 1]
    re = w[n + m + 2 + 2 * nnz:n + m + 2 + 4 * nnz]
    lists = w[n + m + 2 + 4 * nnz:]
    return w[:n + 1], ce, rptr, re, lists


PATTERNS = [(7, 5, 0.5, 1), (40, 30, 0.1, 2), (64, 129, 0.3, 3), (129, 64, 0.6, 4), (33, 33, 1.0, 5), (200, 3, 0.2, 6), (1, 1, 1.0, 7),
            (1, 70, 1.0, 8), (70, 1, 1.0, 9)]


@pytest.mark.parametrize("m,n,density,seed", PATTERNS)
def test_pack_is_the_layout_restated_in_numpy(SB, m, n, density, seed):
    A = _random_csc(m, n, density, seed)
    if m > 8 and n > 8:
        A[3, :] = 0.0                                                  # an empty row and an empty column
        A[:, 5] = 0.0
    cp, ri, va = _csc(A)
    w, long_len = SB.pack(n, m, (cp, ri, va))
    assert long_len == SPB_LONG
    want = S.blob_of(n, m, cp, ri, va)
    assert w.dtype == np.uint32 and np.array_equal(w, want)
    assert w.size == 4 * int(cp[-1]) + m + n + 4 + int(want[n + m + 2 + 4 * int(cp[-1])]) + int(want[n + m + 3 + 4 * int(cp[-1])])
    assert 4 * w.size <= SB.capacity_bytes(n, m, int(cp[-1]))
    # the row order is the column order of the transpose
    wt, _ = SB.pack(m, n, _csc(A.T.copy()))
    cptr, ce, rptr, re, lists = _sections(w, n, m)
    tcptr, tce, trptr, tre, tlists = _sections(wt, m, n)
    assert np.array_equal(rptr, tcptr) and np.array_equal(re, tce) and np.array_equal(cptr, trptr) and np.array_equal(ce, tre)
    nlr, nlc = int(lists[0]), int(lists[1])
    assert (int(tlists[0]), int(tlists[1])) == (nlc, nlr)
    assert np.array_equal(lists[2:2 + nlr], tlists[2 + nlc:]) and np.array_equal(lists[2 + nlr:], tlists[2:2 + nlc])


def test_pack_of_an_empty_matrix(SB):
    w, _ = SB.pack(4, 6, (np.zeros(5, np.int64), np.zeros(0, np.int32), np.zeros(0, F)))
    assert np.array_equal(w, np.zeros(4 + 6 + 4, np.uint32))
    assert np.array_equal(w, S.blob_of(4, 6, np.zeros(5, np.int64), [], []))


def test_rows_and_columns_at_the_long_threshold(SB):
    """rows of SPB_LONG - 1, SPB_LONG, SPB_LONG + 1 entries, and the same in the columns: only the ones above SPB_LONG are listed"""
    L = SPB_LONG
    m = n = L + 8
    A = np.zeros((m, n), F)
    for i, k in ((0, L - 1), (1, L), (2, L + 1), (5, n)):
        A[i, :k] = 1.0 + i
    cp, ri, va = _csc(A)
    w, _ = SB.pack(n, m, (cp, ri, va))
    assert np.array_equal(w, S.blob_of(n, m, cp, ri, va))
    lists = _sections(w, n, m)[4]
    assert lists[0] == 2 and list(lists[2:4]) == [2, 5]
    assert lists[1] == 0                                               # (no column holds more than 4 entries)
    wt, _ = SB.pack(m, n, _csc(A.T.copy()))
    lt = _sections(wt, m, n)[4]
    assert (lt[0], lt[1]) == (0, 2) and list(lt[2:4]) == [2, 5]
    for k in (L, L + 1):                                               # one column of exactly k entries
        B = np.zeros((L + 3, 2), F)
        B[:k, 1] = -1.0
        lb = _sections(SB.pack(2, L + 3, _csc(B))[0], 2, L + 3)[4]
        assert (lb[0], lb[1]) == (0, 1 if k > L else 0)


def test_explicit_zeros_are_kept(SB):
    cp, ri, va = np.array([0, 2, 3], np.int64), np.array([0, 2, 1], np.int32), np.array([0.0, 1.0, -0.0], F)
    w, _ = SB.pack(2, 3, (cp, ri, va))
    assert w[2] == 3 and np.array_equal(w, S.blob_of(2, 3, cp, ri, va))


REFUSALS = [
    ("not monotone from 0", [1, 2, 3], [0, 1, 2], [1, 1, 1], 0),
    ("not monotone from 0", [0, 2, 1], [0, 1], [1, 1], 0),
    ("out of range", [0, 1, 2], [0, 3], [1, 1], 0),
    ("out of range", [0, 1, 2], [0, -1], [1, 1], 0),
    ("not strictly ascending", [0, 2, 2], [1, 1], [1, 1], 0),
    ("not strictly ascending", [0, 2, 2], [2, 0], [1, 1], 0),
    ("not finite", [0, 1, 2], [0, 1], [1, np.inf], 0),
    ("not finite", [0, 1, 2], [0, 1], [np.nan, 1], 0),
    ("2 entries where nnz_cap is 1", [0, 1, 2], [0, 1], [1, 1], 1),
    ("nnz_cap 7 exceeds m n = 6", [0, 1, 2], [0, 1], [1, 1], 7),
]


@pytest.mark.parametrize("words,cp,ri,va,cap", REFUSALS)
def test_every_refusal_of_the_stored_form(SB, words, cp, ri, va, cap):
    """n = 2, m = 3"""
    with pytest.raises(ValueError, match=words):
        SB.pack(2, 3, (np.array(cp, np.int64), np.array(ri, np.int32), np.array(va, F)), nnz_cap=cap)


def test_refusals_of_the_python_layer(SB):
    with pytest.raises(ValueError, match="n \\+ 1 = 3"):
        SB.pack(2, 3, (np.zeros(2, np.int64), [], []))
    with pytest.raises(ValueError, match="differ in length"):
        SB.pack(2, 3, ([0, 1, 1], [0], []))
    with pytest.raises(ValueError, match="colptr ends at 2 where 1 entries"):
        SB.pack(2, 3, ([0, 1, 2], [0], [1.0]))
    with pytest.raises(ValueError, match="triple or a scipy.sparse matrix"):
        SB.pack(2, 3, np.zeros((3, 2)))


# ---- the routes into it ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lp40x30", "mixed145x40", "rows", "cols", "zero", "identity"])
def test_from_dense_s_extraction_gives_the_triples_blobs(SB, name):
    if name in S.SHAPES:
        ds = [S.sparse_problem(name, s) for s in range(2)]
    elif name in ("rows", "cols"):
        ds = [S.lengths_problem(name == "cols", 0)]
    else:
        ds = [S.zero_problem() if name == "zero" else S.identity_problem(0)]
    for d in ds:
        got = SB.csc_of_dense(d.mat_a, d.n, d.m)
        want = S.csc_of(d)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        A = np.asarray(d.mat_a).reshape(d.n, d.m).T
        assert int(got[0][-1]) == int((A != 0).sum())
        assert np.array_equal(SB.pack(d.n, d.m, got)[0], S.blob_of(d.n, d.m, *want))


def test_scipy_input_is_left_as_it_was(SB):
    sp = pytest.importorskip("scipy.sparse")
    A = _random_csc(30, 20, 0.3, 11)
    want = SB.pack(20, 30, _csc(A))[0]
    # a CSC matrix whose indices are not sorted, a COO matrix with duplicates, a CSR matrix
    c = sp.csc_matrix(A)
    for j in range(20):
        s, e = c.indptr[j], c.indptr[j + 1]
        c.indices[s:e] = c.indices[s:e][::-1].copy()
        c.data[s:e] = c.data[s:e][::-1].copy()
    c.has_sorted_indices = False
    coo = sp.coo_matrix(A)
    half = (coo.data / 2).astype(F)
    dup = sp.coo_matrix((np.concatenate([half, half]), (np.concatenate([coo.row, coo.row]), np.concatenate([coo.col, coo.col]))),
                        shape=A.shape)
    for mat in (c, dup, sp.csr_matrix(A)):
        keep = [np.array(getattr(mat, k)).copy() for k in ("data", "indices", "indptr", "row", "col") if hasattr(mat, k)]
        got = SB.pack(20, 30, mat)[0]
        now = [np.array(getattr(mat, k)) for k in ("data", "indices", "indptr", "row", "col") if hasattr(mat, k)]
        assert all(np.array_equal(a, b) for a, b in zip(keep, now))
        if mat is c:
            assert not mat.has_sorted_indices
        assert np.array_equal(got, want)
    with pytest.raises(ValueError, match="shape"):
        SB.pack(30, 20, c)
