"""`MidBatchSolver`: many MID-SIZE conic programs, each with its OWN dense f32 A (one shape n, m and one cone layout; their own A_p,
b_p, c_p) that is too big for the LDS of a CU (m * n > 24 576, the small batch's limit) -- a few hundred rows and columns each:
scenario sets, MPC horizons, per-fold SVMs, per-agent programs (thip_midbatch_* in include/totsu_f32hip.h).  One workgroup per
problem keeps every vector of the iteration in LDS and STREAMS the problem's A from memory, twice per iteration (the carried
recurrence), with no launch boundary inside an iteration; the host machinery, the methods and the ValueErrors are
`OwnBatchSolver`'s (totsu_amd/ownbatch.py).

Taken: 1 <= m, n <= 4096 whose vectors fit LDS (every shape with 8 n + 13 m <= 32 768 does; `fits` is the rule), the zero,
nonnegative, second-order and rotated second-order cones; "compensated" and "plain" state arithmetic.  Refused (ValueError): PSD
segments, m or n beyond 4096, vectors beyond LDS, segments that do not cover m, no problem at all, arrays of the wrong length.

`own_a_batch(denses)` picks between the two batches by shape."""
from . import _lib
from . import smallbatch as _sb
from .ownbatch import OwnBatchSolver, _fits, first_that_takes
from .smallbatch import SmallBatchSolver


def fits(n, m, seg_type, seg_len):
    """the shape rules alone (thip_midbatch_fits; needs no GPU): (lds_bytes, threads) of one workgroup, or ValueError"""
    return _fits("thip_midbatch_", n, m, seg_type, seg_len)


class MidBatchSolver(SmallBatchSolver):
    """OwnBatchSolver on thip_midbatch_* (a subclass of SmallBatchSolver, as it has always been: what is patched or overridden there
    reaches every family).  force_threads: test hook (256, 1024).  info() adds load_bytes (16 or 4) and
    a_bytes_per_iter (bytes of A read per problem-iteration)."""
    _prefix, _force_hook, _what, _Info = "thip_midbatch_", "thip_test_midbatch_force_threads", "mid", _lib.MidBatchInfo


FAMILIES = ((SmallBatchSolver, _sb.fits), (MidBatchSolver, fits))


def _choose(n, m, seg_type, seg_len):
    return first_that_takes(FAMILIES, n, m, seg_type, seg_len, "neither SmallBatchSolver nor MidBatchSolver takes %d x %d problems "
                            "with this cone layout (%s): run one FusedSolver per problem")


def choose(n, m, seg_type, seg_len):
    """which own-A batch takes the shape -- "small", "mid" -- a plain function of (n, m, seg_type, seg_len) that needs no GPU;
    ValueError (naming FusedSolver) when neither does"""
    return _choose(n, m, seg_type, seg_len)._what


def own_a_batch(denses, param=None, **kw):
    """the batch solver for a list of Prob*.dense() that share a shape and a cone layout and each have their own A: a
    SmallBatchSolver when the small batch's rule takes the shape (A in LDS), a MidBatchSolver when only the mid batch's does (A
    streamed), else a ValueError that names FusedSolver.

    Crossover against one FusedSolver(schedule="carried") per problem in turn (profiles/midbatch_rate.txt, one MI355X): there is
    none in what was measured.  The mid batch wins at every shape and every P that was run, down to P = 16 -- by 2.9x at
    2000 x 1000 and 42x at 256 x 128 there, by 17x and 633x at P = 256 -- so the choice is by shape alone.  Below P = 16 nothing
    was measured; a single problem is FusedSolver's case."""
    denses = OwnBatchSolver.check_same_layout(denses)
    d0 = denses[0]
    return _choose(d0.n, d0.m, d0.seg_type, d0.seg_len).from_dense(denses, param, **kw)
