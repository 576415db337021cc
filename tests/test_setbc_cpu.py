"""CPU: what set_bc does on the host and what keep_iterate=True means.  The packing and validation of the Python side as a function
that needs no handle (totsu_amd.ownbatch.pack_bc): the per-problem lengths of a batch of one shape and of a ragged one, the row-sum
mask of a mixed list, the refusals and their words.  The 12 new symbols in the header and in the built library.  And the restatement
of "keep" in f64 (tests/warm_numpy.py, whose loop is untouched): changing (b, c) after iteration k is a fresh preconditioner and
fresh norms on (A, b', c') and a start at the iterate as it stands, iteration 0 -- checked through the oracle's snapshots, which are
what the loop's iterate after iteration k is."""
import os
import re

import numpy as np
import pytest

import warm_numpy as W
from setbc_cases import perturbed
from totsu_amd.ownbatch import pack_bc
from warm_cases import cpu_problems, oracle_run, snap_xy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAMES = ("smallbatch", "midbatch", "sdpbatch", "raggedbatch", "sparsebatch", "raggedsparse")
TOL = 1e-9            # of the iterate's max norm: f64 against f64 (tests/test_warm_start_cpu.py)


def _vecs(shapes, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(m).astype(F) for _, m in shapes], [rng.standard_normal(n).astype(F) for n, _ in shapes]


# ---- packing ------------------------------------------------------------------------------------------------------------------------

def test_pack_one_shape():
    n, m, P = 3, 5, 7
    b, c = _vecs([(n, m)] * 4)
    count, pb, pc, r, has = pack_bc(P, lambda i: (n, m), b, c, first=2)
    assert count == 4 and r is None and has is None
    assert pb.dtype == pc.dtype == F and pb.flags["C_CONTIGUOUS"] and pc.flags["C_CONTIGUOUS"]
    assert np.array_equal(pb, np.concatenate(b)) and np.array_equal(pc, np.concatenate(c))
    # 2-D arrays, float64 in: one row per problem, converted
    count, pb2, pc2, _, _ = pack_bc(P, lambda i: (n, m), np.stack(b).astype(np.float64), np.stack(c).astype(np.float64), first=3)
    assert count == 4 and np.array_equal(pb2, pb) and np.array_equal(pc2, pc) and pb2.dtype == F
    # a list of Nones is no row sums at all
    assert pack_bc(P, lambda i: (n, m), b, c, [None] * 4)[3:] == (None, None)


def test_pack_ragged_lengths_follow_first():
    shapes = [(1, 1), (40, 80), (96, 160), (157, 157), (6, 45)]
    b, c = _vecs(shapes[2:])
    count, pb, pc, r, has = pack_bc(len(shapes), lambda i: shapes[i], b, c, first=2)
    assert count == 3 and pb.size == 160 + 157 + 45 and pc.size == 96 + 157 + 6
    assert np.array_equal(pb[160:317], b[1]) and np.array_equal(pc[96:253], c[1])
    with pytest.raises(ValueError, match="problem 1:"):           # the same vectors one slot early: problem 1 is 80 x 40
        pack_bc(len(shapes), lambda i: shapes[i], b, c, first=1)


def test_pack_row_sum_mask():
    shapes = [(2, 3), (4, 5), (1, 2)]
    b, c = _vecs(shapes)
    rows = [np.full(3, 7, F), None, np.full(2, 9, F)]
    count, pb, pc, r, has = pack_bc(3, lambda i: shapes[i], b, c, rows)
    assert has.dtype == np.uint8 and has.tolist() == [1, 0, 1]
    assert r.dtype == F and r.size == 3 + 5 + 2                   # m floats for every problem, zeros where there are none
    assert r.tolist() == [7, 7, 7, 0, 0, 0, 0, 0, 9, 9]
    count, _, _, r, has = pack_bc(3, lambda i: shapes[i], b, c, [np.ones(3), np.ones(5), np.ones(2)])
    assert has is None and r.size == 10                           # all of them: no mask is needed


def test_pack_refusals():
    shapes = [(2, 3), (4, 5), (1, 2)]
    b, c = _vecs(shapes)

    def at(i):
        return shapes[i]

    def bad(match, *a, **k):
        with pytest.raises(ValueError, match=match):
            pack_bc(3, at, *a, **k)
    bad(r"problem 1: b holds 6 and c 4 entries where m = 5 and n = 4", [b[0], np.zeros(6), b[2]], c)
    bad(r"problem 2: b holds 2 and c 3 entries where m = 2 and n = 1", b, [c[0], c[1], np.zeros(3)])
    bad(r"problem 1: vec_b_rowabs holds 4 entries where m = 5", b, c, [None, np.zeros(4), None])
    bad(r"problem 1: b holds 3 and c 2", b[:2], c[:2], first=1)   # (the range fits, the lengths are those of problems 0 and 1)
    bad(r"at least one", [], [])
    bad(r"3 b where there are 2 c", b, c[:2])
    bad(r"2 vecs_b_rowabs where there are 3 b", b, c, [None, None])
    bad(r"no problems 1 \.\. 3 in a batch of 3", b, c, first=1)
    bad(r"no problems 3 \.\. 3 in a batch of 3", b[:1], c[:1], first=3)
    bad(r"no problems -1 \.\. -1 in a batch of 3", b[:1], c[:1], first=-1)


# ---- the symbols --------------------------------------------------------------------------------------------------------------------

def _new_symbols():
    return ["thip_%s_%s" % (n, f) for n in NAMES for f in ("set_bc", "solutions")]


def test_the_header_declares_the_new_symbols():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "totsu_f32hip.h")).read(), flags=re.S)
    declared = dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(thip_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S))
    for name in _new_symbols():
        assert name in declared, name
        args = declared[name].count(",") + 1
        assert args == (8 if name.endswith("set_bc") else 6), (name, args)


def test_the_library_exports_the_new_symbols():
    from totsu_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        pytest.skip("the library is not built")
    lib = _lib.load()
    for name in _new_symbols():
        assert hasattr(lib, name), "missing symbol %s" % name
        assert name in _lib.PROTOTYPES, name


# ---- keep, restated -----------------------------------------------------------------------------------------------------------------

def _err(got, want):
    return max(np.abs(got[0] - want[0]).max() / max(np.abs(want[0]).max(), 1e-6), np.abs(got[1] - want[1]).max() / max(np.abs(want[1]).max(), 1e-6))


@pytest.mark.parametrize("k", [0, 9])
def test_keep_is_a_fresh_preconditioner_and_a_start_at_the_iterate(k):
    for key, d, pieces in cpu_problems():
        ro = oracle_run(key, d, socp=pieces)
        old, new = W.Problem.of_dense(d), W.Problem.of_dense(perturbed(d, 3))
        assert not np.array_equal(old.Tx, new.Tx) and old.t_tau != new.t_tau and old.norm_b != new.norm_b
        # the loop on (A, b, c) through iteration k: its iterate is the oracle's snapshot
        before = W.run(old, k + 1, snap_iters=(k,))
        assert _err(before.snaps[k], snap_xy(ro, d, k)) <= TOL, (key, k)
        for j in (1, 10):
            # (b, c) changes after iteration k: the loop goes on from the iterate as it stands -- nothing rescaled, iteration 0 --
            # with the preconditioner and the norms of the new data
            kept = W.run(new, j, start=(before.x, before.y), snap_iters=(j - 1,))
            want = W.run(new, j, start=snap_xy(ro, d, k), snap_iters=(j - 1,))
            e = _err(kept.snaps[j - 1], want.snaps[j - 1])
            print("%s keep after iteration %d, %d iterations: err %.2e" % (key, k, j, e))
            assert e <= TOL, (key, k, j, e)
            assert kept.iters == j - 1 and kept.state == W.RUNNING and kept.kind == want.kind
            assert np.allclose(kept.cri, want.cri, rtol=1e-6, atol=1e-12), (key, k, j)
            # and it is not the old problem's continuation, nor the new problem's zero start
            assert _err(kept.snaps[j - 1], snap_xy(ro, d, k + j)) > 1e-6, (key, k, j)
            fresh = W.run(new, j, snap_iters=(j - 1,))
            assert k == 0 or _err(kept.snaps[j - 1], fresh.snaps[j - 1]) > 1e-6, (key, k, j)
