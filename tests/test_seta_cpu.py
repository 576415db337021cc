"""CPU: what set_a does on the host.  The packing of the new values as a function that needs no handle
(totsu_amd.ownbatch.pack_a) with its refusals and their words; the pattern comparison of the sparse classes on a stub that holds
patterns and no handle; the six thip_*_set_a symbols and the two blob hooks in the headers and in the built library; and the device's
scatter restated in numpy (tests/seta_cases.py::scatter_numpy: row-order entries taken to their column-order places by search)
against sparsebatch.pack of the same pattern with the new values, word for word, on rows and columns of 0, 1, 31, 32, 33, 63, 64,
65, 128, 129 and 140 entries -- which fixes the blob the GPU test expects without a device."""
import os
import re

import numpy as np
import pytest

from seta_cases import perturbed_a, scatter_numpy, triple_at, values_at
from sparse_cases import SPB_LONG, blob_of, csc_of, identity_problem, lengths_problem, zero_problem
from totsu_amd.ownbatch import pack_a

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("smallbatch", "midbatch", "sdpbatch", "raggedbatch", "sparsebatch", "raggedsparse")


# ---- packing ------------------------------------------------------------------------------------------------------------------------

def test_pack_one_shape():
    rng = np.random.default_rng(0)
    mats = [rng.standard_normal(15).astype(F) for _ in range(4)]
    count, v, counts = pack_a(7, lambda i: 15, mats, first=2)
    assert count == 4 and v.dtype == F and v.flags["C_CONTIGUOUS"] and counts.dtype == np.int64 and counts.tolist() == [15] * 4
    assert np.array_equal(v, np.concatenate(mats))
    count, v2, _ = pack_a(7, lambda i: 15, np.stack(mats).astype(np.float64), first=3)      # a 2-D array, float64 in
    assert count == 4 and np.array_equal(v2, v) and v2.dtype == F
    count, v3, _ = pack_a(7, lambda i: 15, [a.reshape(5, 3) for a in mats])                # any shape of the right size
    assert np.array_equal(v3, v)
    with pytest.raises(ValueError, match=r"problem 4: a value of A is not finite"):        # a 2-D array names the problem too
        pack_a(7, lambda i: 15, np.where(np.arange(60).reshape(4, 15) == 37, np.inf, 1.0), first=2)
    with pytest.raises(ValueError, match=r"problem 3: 14 values of A where 15 are needed"):
        pack_a(7, lambda i: 15, np.ones((4, 14)), first=3)


def test_pack_ragged_lengths_follow_first():
    sizes = [1, 3200, 15360, 24649, 270]
    mats = [np.full(s, k + 1, F) for k, s in enumerate(sizes[2:])]
    count, v, counts = pack_a(5, lambda i: sizes[i], mats, first=2)
    assert count == 3 and counts.tolist() == sizes[2:] and v.size == sum(sizes[2:]) and v[15360] == 2
    with pytest.raises(ValueError, match=r"problem 1: 15360 values of A where 3200 are needed"):
        pack_a(5, lambda i: sizes[i], mats, first=1)
    count, v, counts = pack_a(3, lambda i: [0, 2, 0][i], [np.zeros(0), np.ones(2), []])     # problems without entries
    assert counts.tolist() == [0, 2, 0] and v.tolist() == [1, 1]


def test_pack_refusals():
    sizes = [6, 20, 2]
    mats = [np.ones(s, F) for s in sizes]

    def bad(match, *a, **k):
        with pytest.raises(ValueError, match=match):
            pack_a(3, lambda i: sizes[i], *a, **k)
    bad(r"problem 1: 21 values of A where 20 are needed", [mats[0], np.ones(21), mats[2]])
    bad(r"problem 2: 1 values of A where 2 are needed", mats[:2] + [np.ones(1)])
    bad(r"problem 1: a value of A is not finite", [mats[0], np.where(np.arange(20) == 7, np.nan, 1.0), mats[2]])
    bad(r"problem 0: a value of A is not finite", [np.array([1, 2, np.inf, 4, 5, 6])] + mats[1:])
    bad(r"problem 2: a value of A is not finite", mats[:2] + [np.array([-np.inf, 0])])
    bad(r"problem 0: a value of A is not finite", [np.full(6, 1e39)] + mats[1:])              # finite in f64, not in f32
    bad(r"at least one", [])
    bad(r"no problems 1 \.\. 3 in a batch of 3", mats, first=1)
    bad(r"no problems 3 \.\. 3 in a batch of 3", mats[:1], first=3)
    bad(r"no problems -1 \.\. -1 in a batch of 3", mats[:1], first=-1)
    count, v, _ = pack_a(3, lambda i: sizes[i], [np.zeros(6), mats[1], mats[2]])                 # zeros are values
    assert count == 3 and not v[:6].any()


# ---- the pattern comparison -----------------------------------------------------------------------------------------------------------

def _stub(cls, ds):
    """an object of the class with the patterns of ds and no handle: what set_a consults before it calls the library"""
    from totsu_amd.sparsebatch import _pattern_of
    sb = cls.__new__(cls)
    sb.h, sb._owned, sb._slot_owned = None, [], {}
    sb.n_prob = len(ds)
    sb.n, sb.m = ds[0].n, ds[0].m
    sb.shapes = [(d.n, d.m) for d in ds]
    sb._patterns = [_pattern_of(csc_of(d)) for d in ds]
    return sb


@pytest.mark.parametrize("which", ["sparse", "raggedsparse"])
def test_the_pattern_comparison(which):
    import scipy.sparse as sp
    import totsu_amd as T
    from totsu_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        pytest.skip("the library is not built")
    cls = {"sparse": T.SparseBatchSolver, "raggedsparse": T.RaggedSparseBatchSolver}[which]
    ds = [lengths_problem(False, 0), lengths_problem(False, 1)] if which == "sparse" else [lengths_problem(False, 0), identity_problem(0)]
    sb = _stub(cls, ds)
    news = [perturbed_a(d, i, zeros=3) for i, d in enumerate(ds)]
    want = [values_at(d, e) for d, e in zip(ds, news)]
    assert [sb._a_size(i) for i in range(2)] == [w.size for w in want]
    for i, (d, e) in enumerate(zip(ds, news)):
        assert sb._a_values(i, want[i]) is want[i]                                              # a plain array: taken as it is
        assert np.array_equal(sb._a_values(i, triple_at(d, e)), want[i])                        # a triple of the slot's pattern
        cp, ri, va = triple_at(d, e)
        mat = sp.csc_matrix((va, ri, cp), shape=(d.m, d.n))                                     # scipy, explicit zeros stored
        assert mat.nnz == want[i].size and np.array_equal(sb._a_values(i, mat), want[i])
        assert np.array_equal(sb._a_values(i, mat.tocsr()), want[i])                            # any scipy format of that pattern
    # the whole packing through the class's hooks
    count, v, counts = pack_a(2, sb._a_size, [want[0], triple_at(ds[1], news[1])], 0, sb._a_values)
    assert count == 2 and np.array_equal(v, np.concatenate(want)) and counts.tolist() == [w.size for w in want]
    # another pattern: one entry moved, one entry dropped (scipy drops nothing by itself: eliminate_zeros does), one added
    d, e = ds[0], news[0]
    cp, ri, va = triple_at(d, e)
    moved = ri.copy()
    col = int(np.nonzero((np.diff(cp) >= 1) & (np.diff(cp) < d.m))[0][0])
    free = sorted(set(range(d.m)) - set(ri[cp[col]:cp[col + 1]].tolist()))
    seg = np.sort(np.append(ri[cp[col]:cp[col + 1]][1:], free[0])).astype(np.int32)
    moved[cp[col]:cp[col + 1]] = seg
    with pytest.raises(ValueError, match=r"problem 0: .*another pattern.*replace"):
        sb._a_values(0, (cp, moved, va))
    with pytest.raises(ValueError, match=r"problem 0: .*another pattern.*replace"):
        sb._a_values(0, sp.csc_matrix((va, moved, cp), shape=(d.m, d.n)))
    dropped = sp.csc_matrix((va, ri, cp), shape=(d.m, d.n))
    dropped.eliminate_zeros()
    assert dropped.nnz == va.size - 3
    with pytest.raises(ValueError, match=r"another pattern"):
        sb._a_values(0, dropped)
    with pytest.raises(ValueError, match=r"another pattern" if which == "sparse" else None):
        sb._a_values(1, triple_at(d, e))                                # problem 0's matrix in slot 1 (ragged: another shape)
    with pytest.raises(ValueError, match=r"problem 0: 3 values of A where %d are needed" % va.size):
        pack_a(2, sb._a_size, [np.ones(3)], 0, sb._a_values)                                    # a count that is off


# ---- the symbols --------------------------------------------------------------------------------------------------------------------

def _declared(header):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(thip_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S))


def test_the_headers_declare_the_new_symbols():
    api, hooks = _declared("totsu_f32hip.h"), _declared("totsu_f32hip_test.h")
    for n in NAMES:
        name = "thip_%s_set_a" % n
        assert name in api and api[name].count(",") + 1 == 6, name
        assert "thip_%s_set_bc" % n in api                                                      # beside set_bc
    for n in ("sparsebatch", "raggedsparse"):
        name = "thip_test_%s_blob" % n
        assert name in hooks and hooks[name].count(",") + 1 == 5, name


def test_the_library_exports_the_new_symbols():
    from totsu_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        pytest.skip("the library is not built")
    lib = _lib.load()
    for name in ["thip_%s_set_a" % n for n in NAMES] + ["thip_test_sparsebatch_blob", "thip_test_raggedsparse_blob"]:
        assert name in _lib.PROTOTYPES, name
        assert getattr(lib, name) is not None, name


# ---- the scatter, restated ----------------------------------------------------------------------------------------------------------

# (the matrices of the GPU blob test, tests/test_gpu_seta.py::_blob_problems)
SCATTER_CASES = {"rows": lambda: lengths_problem(False, 0), "cols": lambda: lengths_problem(True, 0), "zero": zero_problem,
                 "identity": lambda: identity_problem(0), "rows-explicit-zeros": lambda: lengths_problem(False, 1)}


@pytest.mark.parametrize("label", sorted(SCATTER_CASES))
def test_the_scatter_restated_gives_the_packed_blob(label):
    from totsu_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        pytest.skip("the library is not built")
    from totsu_amd import sparsebatch
    d = SCATTER_CASES[label]()
    cp, ri, va = csc_of(d)
    old, long_len = sparsebatch.pack(d.n, d.m, (cp, ri, va))
    assert long_len == SPB_LONG
    lens = sorted(set(np.diff(cp).tolist()) | set(np.bincount(ri, minlength=d.m).tolist()))
    if label in ("rows", "cols", "rows-explicit-zeros"):
        assert set([0, 1, 31, 32, 33, 63, 64, 65, 128, 129, 140]) <= set(lens), lens
    for zeros in (0, 5):
        new = values_at(d, perturbed_a(d, 3, zeros=zeros))
        assert new.size == va.size and (zeros == 0 or va.size <= 8 or int((new == 0).sum()) == zeros)
        want, _ = sparsebatch.pack(d.n, d.m, (cp, ri, new))
        got = scatter_numpy(old, d.n, d.m, new)
        assert got.dtype == np.uint32 and np.array_equal(got, want), label
        assert np.array_equal(want, blob_of(d.n, d.m, cp, ri, new))       # and both are the stored form as numpy restates it
        if va.size:
            assert not np.array_equal(got, old)
