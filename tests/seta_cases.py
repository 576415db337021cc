"""What the set_a tests share (tests/test_gpu_seta.py, tests/test_seta_cpu.py): the new A of a problem -- every stored entry under 1 %
multiplicative noise with a fixed seed, so the zeros of a dense A stay zeros and from_dense of the sparse families keeps the pattern,
and a variant that sets a few stored entries to exactly 0 (explicit zeros: entries all the same) -- how each family is handed it, the
replace route it is held to, and a numpy restatement of the device's scatter.  The families and their problem sets are
tests/setbc_cases.py's.  A plain module, like tests/setbc_cases.py."""
import copy

import numpy as np

from ownbatch_cases import F
from sparse_cases import csc_of


def with_a(d, mat_a):
    e = copy.copy(d)
    e.mat_a = np.ascontiguousarray(mat_a, F).ravel()
    return e


def perturbed_a(d, seed, zeros=0):
    """d with every entry of A times 1 + 0.01 N(0, 1); zeros: that many of its entries != 0 (when it has more than 8) set to 0"""
    rng = np.random.default_rng(909 + seed)
    a = (np.asarray(d.mat_a, F) * (1 + 0.01 * rng.standard_normal(d.mat_a.size))).astype(F)
    stored = np.nonzero(np.asarray(d.mat_a))[0]
    assert np.all(a[stored] != 0)
    if zeros and stored.size > 8:
        a[rng.choice(stored, size=zeros, replace=False)] = 0
    return with_a(d, a)


def new_set(ds, base=0):
    """a new A for every problem of a set; the last one carries three explicit zeros"""
    return [perturbed_a(d, base + i, zeros=3 if i == len(ds) - 1 else 0) for i, d in enumerate(ds)]


def values_at(old, new):
    """new's entries at the pattern of old's entries != 0, in CSC order: what a sparse family's set_a takes"""
    cp, ri, _ = csc_of(old)
    cols = np.repeat(np.arange(old.n), np.diff(cp))
    return np.asarray(new.mat_a, F).reshape(new.n, new.m)[cols, ri].astype(F)


def triple_at(old, new):
    cp, ri, _ = csc_of(old)
    return cp, ri, values_at(old, new)


def set_a(fam, sb, olds, news, first=0, keep=False):
    """olds: the problems whose pattern the slots hold (a dense family ignores them)"""
    mats = [values_at(o, d) for o, d in zip(olds, news)] if fam.sparse else [d.mat_a for d in news]
    sb.set_a(mats, first=first, keep_iterate=keep)


def replace_a(fam, sb, i, old, new, start=None):
    """the route set_a is held to: replace(i, new's A in old's pattern, new's b, c, rowabs)"""
    sb.replace(i, triple_at(old, new) if fam.sparse else new.mat_a, new.vec_b, new.vec_c, new.vec_b_rowabs, start=start)


def scatter_numpy(blob, n, m, values):
    """the device's scatter restated: the blob (uint32 words, as sparsebatch.pack makes it) with the values of its column order
    replaced by `values` and every row-order entry given the value of its place in the column order, found by a search for the row
    among the ascending rows of the entry's column.  Pointers, index words and lists are not touched"""
    w = np.array(blob, dtype=np.uint32, copy=True)
    v = np.ascontiguousarray(values, F).view(np.uint32)
    nnz = int(w[n])
    assert v.size == nnz
    ce, rptr = n + 1, n + 1 + 2 * nnz
    re = rptr + m + 1
    for i in range(m):
        for r in range(int(w[rptr + i]), int(w[rptr + i + 1])):
            j = int(w[re + 2 * r + 1])
            lo, hi = int(w[j]), int(w[j + 1])
            rows = w[ce + 2 * lo + 1:ce + 2 * hi + 1:2]
            at = lo + int(np.searchsorted(rows, i))
            assert at < hi and int(w[ce + 2 * at + 1]) == i
            w[re + 2 * r] = v[at]
    w[ce:ce + 2 * nnz:2] = v
    return w
