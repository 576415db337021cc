"""What the tests of the mid batch over a 16-bit A share (tests/test_gpu_mid16batch.py, tests/test_mid16batch_cpu.py): the numpy
restatements of both roundings, of the stored block and of the widened matrix W, the planted matrices of the stored-form test, the
edge shapes, and the twin -- a MidBatchSolver over W in f32, which a Mid16BatchSolver must equal bit for bit.  A plain module, like
tests/ownbatch_cases.py.

The stored form (include/totsu_f32hip.h): per problem n columns of ld16 = roundup4(m) 16-bit words, column-major, the pad rows zero;
f16: n floats inv_s behind the matrix; the block a multiple of 16 bytes.
    bf16   the f32 rounded to nearest even to its upper 16 bits: (b + 0x7fff + ((b >> 16) & 1)) >> 16 on the bit pattern b
    f16    inv_s[c] = 2^(e - 14), e the exponent frexp gives the largest |a| of column c (1 for a column of zeros); the word is
           float16(a / inv_s[c]), round to nearest even
    W      bf16: the word shifted left 16 bits; f16: float32(h) * inv_s[c], one f32 multiply"""
import numpy as np

F = np.float32
KINDS = ("bf16", "f16")
A_BF16, A_F16 = 1, 2

ROWS, CK = 256, 8
# tests/test_gpu_midbatch.py::EDGE_SHAPES, restated: (m, n, forced threads or 0)
EDGE_SHAPES = [(1, 1, 0), (1, 300, 0), (300, 1, 0),
               (65, 33, 0), (66, 5, 0), (67, 9, 0),
               (ROWS - 1, 12, 0), (ROWS, 12, 0), (ROWS + 1, 12, 0),
               (40, CK - 1, 0), (40, CK, 0), (40, CK + 1, 0),
               (3 * ROWS, 10, 256), (4 * ROWS, 10, 256), (4 * ROWS + 1, 10, 256),
               (8, 2047, 0), (8, 2048, 0), (8, 2049, 0), (260, 1025, 0)]
STORED_SHAPES = [(160, 80), (65, 33), (66, 5), (67, 9), (1, 1)]      # m % 4 = 0, 1, 2, 3 and one entry


def ld16(m):
    return (int(m) + 3) & ~3


def store_bytes(n, m, kind):
    """the bytes of one problem's block"""
    return (2 * ld16(m) * n + (4 * n if kind == "f16" else 0) + 15) & ~15


def bf16_words(a):
    """to_bf16_k's rule on an array of float32: uint16 words"""
    b = np.ascontiguousarray(a, dtype=F).view(np.uint32).astype(np.uint64)
    special = (b & 0x7f800000) == 0x7f800000
    rounded = ((b + 0x7fff + ((b >> 16) & 1)) >> 16) & 0xffff
    keep = (b >> 16) | np.where((b & 0xffff) != 0, np.uint64(0x40), np.uint64(0))
    return np.where(special, keep, rounded).astype(np.uint16)


def f16_inv_scale(cols):
    """f16_scale_k's rule: cols is (n, m), one row per column of A; float32 (n,)"""
    cols = np.asarray(cols, dtype=F)
    v = np.abs(cols)
    v = np.where(np.isfinite(v), v, 0)
    mx = v.max(axis=1) if cols.shape[1] else np.zeros(cols.shape[0], F)
    _, e = np.frexp(mx)
    with np.errstate(under="ignore"):
        inv = np.ldexp(F(1), e.astype(np.int32) - 14).astype(F)
    return np.where(mx > 0, inv, F(1)).astype(F)


def f16_words(cols, inv):
    """to_f16_k's rule: float16(a / inv_s[c]) as uint16 words"""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        q = (np.asarray(cols, dtype=F) / np.asarray(inv, dtype=F)[:, None]).astype(F)
        return q.astype(np.float16).view(np.uint16)


def stored(mat_a, m, n, kind):
    """(words (n, ld16) with zero pad rows, inv_s (n,) or None) of the column-major f32 mat_a"""
    cols = np.asarray(mat_a, dtype=F).reshape(n, m)
    words = np.zeros((n, ld16(m)), dtype=np.uint16)
    if kind == "bf16":
        words[:, :m] = bf16_words(cols)
        return words, None
    inv = f16_inv_scale(cols)
    words[:, :m] = f16_words(cols, inv)
    return words, inv


def widen(words, inv, m):
    """W as float32, m n column-major"""
    w = np.ascontiguousarray(words[:, :m])
    if inv is None:
        out = (w.astype(np.uint32) << 16).view(F)
    else:
        out = w.view(np.float16).astype(F) * np.asarray(inv, dtype=F)[:, None]
    return np.ascontiguousarray(out, dtype=F).ravel()


def widened_of(mat_a, m, n, kind):
    return widen(*stored(mat_a, m, n, kind), m)


def planted(m, n, seed=0):
    """an m x n matrix (column-major, m n floats) of standard normals with, where the shape has room: exact bf16 ties that round to
    even downwards and upwards, -0, a column of zeros, a column whose largest entry is 3e38, one whose largest is 1e-30, and entries
    that are subnormal in f16 after the column's scaling (and exact f16 ties next to them)"""
    rng = np.random.default_rng(4242 + 100 * m + n + seed)
    a = rng.standard_normal((n, m)).astype(F)                        # a[c]: column c

    def bits(u):
        return np.array([u], dtype=np.uint32).view(F)[0]

    ties = [bits(0x3f808000), bits(0x3f818000), bits(0xbf808000), bits(0xbf818000), F(-0.0), F(0.0)]
    a.ravel()[:min(len(ties), a.size)] = ties[:a.size]
    if n >= 5:
        a[1] = 0.0
        a[2, 0] = 3e38
        a[3] *= F(1e-31)
        a[3, 0] = 1e-30
        # column 4: largest entry 1 (inv_s = 2^-13), entries below 2^-27 are subnormal f16 words after the scaling
        a[4] = 0.0
        a[4, 0] = 1.0
        tail = [F(2.0 ** -30), F(2.0 ** -36), F(1.5 * 2.0 ** -37), F(2.5 * 2.0 ** -37), F(-2.0 ** -37), F(2.0 ** -38), F(2.0 ** -39)]
        k = min(len(tail), m - 1)
        a[4, 1:1 + k] = tail[:k]
    return np.ascontiguousarray(a).ravel()


class WDense:
    """a dense problem with mat_a replaced by another matrix (the fields OwnBatchSolver.from_dense reads)"""

    def __init__(self, d, mat_a):
        self.n, self.m = d.n, d.m
        self.mat_a = np.ascontiguousarray(mat_a, dtype=F)
        self.vec_b, self.vec_c, self.vec_b_rowabs = d.vec_b, d.vec_c, d.vec_b_rowabs
        self.seg_type, self.seg_len = d.seg_type, d.seg_len


def twin_of(T, sb, ds, param=None, **kw):
    """the MidBatchSolver over the widened matrices of the Mid16BatchSolver sb, on the same b, c and cones"""
    return T.MidBatchSolver.from_dense([WDense(d, sb.widened(i)) for i, d in enumerate(ds)], param, **kw)


def state_of(sb, i):
    """everything the contract covers of problem i: iterate, preconditioner and status"""
    st = sb.status(i)
    return sb.iterate(i) + sb.precond(i) + ((st.state, st.iters, st.kind, tuple(st.cri), st.tau, st.kappa, st.norm_b, st.norm_c),)


def assert_same(sb, tw, count, tag=""):
    for i in range(count):
        g, w = state_of(sb, i), state_of(tw, i)
        for k in range(4):
            assert np.array_equal(g[k], w[k]), (tag, i, k, np.abs(g[k] - w[k]).max())
        assert g[4] == w[4], (tag, i, g[4], w[4])
