"""The problem families of tests/test_gpu_sparsebatch.py (and the patterns of tests/test_sparsebatch_cpu.py): conic programs whose A
is mostly zeros, feasible by construction, with their oracle runs (computed once per session and never changed).  A plain module,
like tests/ownbatch_cases.py, whose helpers it uses.

A construction: A is a masked random matrix with one dense row, one dense column, one empty row and one empty column (from 4 x 4
on); b = A x0 + s0 and c = -A^T y0 with s0, y0 strictly inside the cone -- nonnegative rows U(0.1, 1.1), a second-order cone's
leading entry the norm of the rest plus U(0.5, 1.5), a rotated cone's first two entries likewise, zero-cone rows s0 = 0."""
import numpy as np

import oracle as O
from ownbatch_cases import ITERS, F, _D, _edge, _oracle

ZERO, RPOS, SOC, ROT = 0, 1, 2, 3
SPB_LONG = 32              # thip_sparsebatch.hip; the CPU test asserts that the library says the same

# name: (m, n, density, seg_type, seg_len, problems, oracle iterates)
SHAPES = {
    "lp40x30": (40, 30, 0.10, [RPOS], [40], 3, ITERS),
    "lp257x129": (257, 129, 0.05, [RPOS], [257], 3, ITERS),
    "lp300x200": (300, 200, 0.03, [RPOS], [300], 3, ITERS),
    "lp1000x700": (1000, 700, 0.01, [RPOS], [1000], 2, ITERS[:2]),
    "lp2000x1000": (2000, 1000, 0.005, [RPOS], [2000], 2, ITERS[:2]),
    "mixed145x40": (145, 40, 0.08, [ZERO, RPOS, SOC, SOC, ROT, SOC, RPOS], [3, 40, 17, 70, 5, 1, 9], 3, ITERS),
    "mixed700x300": (700, 300, 0.02, [RPOS, SOC, ZERO, ROT, SOC], [200, 129, 7, 64, 300], 2, ITERS),
}


def interior(rng, seg_type, seg_len, dual):
    """a point strictly inside the product cone (dual: of its dual -- the zero cone's dual is free)"""
    out = []
    for t, l in zip(seg_type, seg_len):
        if t == ZERO:
            v = rng.standard_normal(l) if dual else np.zeros(l)
        elif t == RPOS:
            v = rng.uniform(0.1, 1.1, l)
        else:
            v = rng.standard_normal(l) / np.sqrt(max(l, 1))
            lead = 2 if t == ROT else 1
            r = np.linalg.norm(v[lead:])
            for k in range(min(lead, l)):
                v[k] = r + rng.uniform(0.5, 1.5)
        out.append(v)
    return np.concatenate(out)


def problem_of(A, seg_type, seg_len, rng):
    A = np.asarray(A, F)
    m, n = A.shape
    x0, s0, y0 = rng.standard_normal(n), interior(rng, seg_type, seg_len, False), interior(rng, seg_type, seg_len, True)
    A64 = A.astype(np.float64)
    return _D(A, A64 @ x0 + s0, -A64.T @ y0, seg_type, seg_len)


def masked(m, n, density, rng):
    """the masked random matrix with its dense row (m // 3), dense column (n // 3), empty row (m - 2) and empty column (n - 2)"""
    A = rng.standard_normal((m, n)) / np.sqrt(max(density * n, 1.0))
    A *= rng.random((m, n)) < density
    if m >= 4 and n >= 4:
        A[m // 3, :] = rng.standard_normal(n) / np.sqrt(n)
        A[:, n // 3] = rng.standard_normal(m) / np.sqrt(n)
        A[m - 2, :] = 0.0
        A[:, n - 2] = 0.0
    return A.astype(F)


def sparse_problem(name, seed):
    m, n, density, st, sl = SHAPES[name][:5]
    rng = np.random.default_rng(7919 * seed + 1000 * m + n)
    return problem_of(masked(m, n, density, rng), st, sl, rng)


def lengths_problem(transpose, seed):
    """160 x 140: rows of exactly 0, 1, SPB_LONG - 1, SPB_LONG, SPB_LONG + 1, 63, 64, 65, 128, 129 and 140 entries (the other rows
    hold 3), an LP over the nonnegative cone; transpose: the transposed pattern, 140 x 160, the same lengths in its columns"""
    rng = np.random.default_rng(4242 + seed)
    lens = [0, 1, SPB_LONG - 1, SPB_LONG, SPB_LONG + 1, 63, 64, 65, 128, 129, 140]
    A = np.zeros((160, 140))
    for i in range(160):
        k = lens[i] if i < len(lens) else 3
        cols = rng.choice(140, size=k, replace=False)
        A[i, cols] = rng.standard_normal(k) / np.sqrt(max(k, 1))
    assert [int((A[i] != 0).sum()) for i in range(len(lens))] == lens
    if transpose:
        A = A.T.copy()
    return problem_of(A, [RPOS], [A.shape[0]], rng)


def tiny_problem(m, n, seed):
    """1 x 1 with one entry, one row, one column: every entry present.  The construction of the dense families' edge shapes
    (tests/ownbatch_cases.py::_edge: a normal A / sqrt(n), s0, y0 ~ U(0.1, 1.1)), which the mid batch's tests run at the same three
    shapes and tolerances.  A row of equal entries is no case for these tolerances: with most of a 1 x 300 row at one value, u
    collapses from 0.29 to 1.35e-3 between iterates 0 and 1 (the f64 oracle's figures), and the rounding of ANY f32 update of u,
    3e-8 |u_0|, is then 6e-5 of the iterate's max norm, above the 2e-5 these iterates are held to"""
    return _edge(m, n, seed)


def zero_problem():
    """an all-zero 6 x 4 A with b = linspace(0.5, 1.5) and c = 0"""
    return _D(np.zeros((6, 4), F), np.linspace(0.5, 1.5, 6), np.zeros(4), [RPOS], [6])


def identity_problem(seed, n=40):
    """A = [I; -I], b ~ U(0.5, 1.5), c normal: every product of a pass is exact"""
    rng = np.random.default_rng(555 + seed)
    return _D(np.vstack([np.eye(n), -np.eye(n)]), rng.uniform(0.5, 1.5, 2 * n), rng.standard_normal(n), [RPOS], [2 * n])


_FAMILIES = {}


def sparse_family(name):
    """(list of dense problems, list of oracle results, the iterates the oracle ran), computed once.  The names of SHAPES;
    rows / cols: lengths_problem; tiny1x1, tiny1x300, tiny300x1; zero; identity (no oracle: [])"""
    if name in _FAMILIES:
        return _FAMILIES[name]
    if name in SHAPES:
        count, iters = SHAPES[name][5:]
        ds = [sparse_problem(name, s) for s in range(count)]
    elif name in ("rows", "cols"):
        ds, iters = [lengths_problem(name == "cols", s) for s in range(2)], [0, 1, 9]
    elif name.startswith("tiny"):
        m, n = (int(v) for v in name[4:].split("x"))
        ds, iters = [tiny_problem(m, n, s) for s in range(2)], [0, 1, 9]
    elif name == "zero":
        ds, iters = [zero_problem()], [0, 1, 9]
    else:
        assert name == "identity", name
        ds, iters = [identity_problem(s) for s in range(3)], None
    ros = [] if iters is None else [_oracle(d, iters) for d in ds]
    for ro in ros:
        assert ro.status == O.EXCESS_ITER and len(ro.trace) > max(iters), (name, ro.status_name)
        assert all(tr[1] == 0 for tr in ro.trace[:max(iters) + 1]), name
    _FAMILIES[name] = (ds, ros, iters)
    return _FAMILIES[name]


def csc_of(d):
    """(colptr, rowidx, values) of the entries != 0 of a dense problem, by numpy alone"""
    a = np.asarray(d.mat_a, F).reshape(d.n, d.m)
    cols, rows = np.nonzero(a)
    cp = np.zeros(d.n + 1, np.int64)
    np.cumsum(np.bincount(cols, minlength=d.n), out=cp[1:])
    return cp, rows.astype(np.int32), a[cols, rows]


def blob_of(n, m, colptr, rowidx, values, long_len=SPB_LONG):
    """the stored form restated in numpy: cptr, {value, row} pairs, rptr, {value, column} pairs, the counts and the lists of the long
    rows and columns, as uint32 words"""
    colptr, rowidx = np.asarray(colptr, np.int64), np.asarray(rowidx, np.int64)
    values = np.asarray(values, F)
    nnz = int(colptr[-1])
    rowidx, values = rowidx[:nnz], values[:nnz]
    cols = np.repeat(np.arange(n), np.diff(colptr))
    order = np.lexsort((cols, rowidx))                                   # by row, columns ascending inside a row
    rptr = np.zeros(m + 1, np.int64)
    np.cumsum(np.bincount(rowidx, minlength=m), out=rptr[1:])

    def pairs(v, i):
        w = np.empty(2 * nnz, np.uint32)
        w[0::2], w[1::2] = v.view(np.uint32), i.astype(np.uint32)
        return w
    lrow = np.nonzero(np.diff(rptr) > long_len)[0]
    lcol = np.nonzero(np.diff(colptr) > long_len)[0]
    return np.concatenate([colptr.astype(np.uint32), pairs(values, rowidx), rptr.astype(np.uint32), pairs(values[order], cols[order]),
                           np.array([lrow.size, lcol.size], np.uint32), lrow.astype(np.uint32), lcol.astype(np.uint32)])
