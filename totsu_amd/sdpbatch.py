"""`SdpBatchSolver`: many small SDPs -- or mixed conic programs with PSD blocks -- each with its OWN dense f32 A (one shape n, m and
one cone layout; their own A_p, b_p, c_p): one relaxation per graph, per scenario, per agent (thip_sdpbatch_* in
include/totsu_f32hip.h).  The kernel is the mid batch's iteration -- one workgroup per problem, every vector in LDS, A streamed twice
per iteration -- with one more cone class: every PSD cone of order k <= 64 is projected by the workgroup itself between the two
passes, on x_y and then on x_s, with f32 MFMAs on operands in LDS, so an iteration has no launch boundary inside.  The host
machinery, the methods and the ValueErrors are `OwnBatchSolver`'s (totsu_amd/ownbatch.py); a layout without PSD segments gives the
mid batch's iterates bit for bit.

Taken: 1 <= m, n <= 4096; the zero, nonnegative, second-order, rotated second-order and PSD cones, every PSD segment of
k (k + 1) / 2 rows with 1 <= k <= 64 (what ProbSDP.dense() holds); an LDS map of at most 163 840 bytes --
4 (6208 + 8 n + 13 m) + roundup4(m), plus 49 920 when the largest PSD order exceeds 32 (`fits` is the rule).  So orders up to 32
cost no LDS at all, an order-48 cone (1176 rows) leaves room for n <= 836, and the largest order whose vectors still fit is 57
(1653 rows, n <= 46): the kernel's own cap of 64 is not reached by any layout.  Refused
(ValueError): a PSD length that is not triangular, an order above 64, m or n beyond 4096, a map beyond LDS, segments that do not
cover m, no problem at all, arrays of the wrong length.

`conic_batch(denses)` picks between the three own-A batches by shape and layout."""
from . import _lib
from . import midbatch as _mb
from .midbatch import MidBatchSolver
from .ownbatch import OwnBatchSolver, _fits, first_that_takes


def fits(n, m, seg_type, seg_len):
    """the shape rules alone (thip_sdpbatch_fits; needs no GPU): (lds_bytes, threads) of one workgroup, or ValueError"""
    return _fits("thip_sdpbatch_", n, m, seg_type, seg_len)


class SdpBatchSolver(MidBatchSolver):
    """the constructor, from_dense, run / run_until_any / status / solution / iterate / precond / replace / info / solve of
    MidBatchSolver, on thip_sdpbatch_*.  force_threads: test hook (256, 1024).  info() adds max_psd_order, n_psd and psd_lds_bytes
    (the LDS the projection adds beyond the vectors)."""
    _prefix, _force_hook, _what, _Info = "thip_sdpbatch_", "thip_test_sdpbatch_force_threads", "SDP", _lib.SdpBatchInfo


def conic_batch(denses, param=None, **kw):
    """the batch solver for a list of Prob*.dense() that share a shape and a cone layout and each have their own A: the first of
    SmallBatchSolver (A in LDS), MidBatchSolver (A streamed) and SdpBatchSolver (A streamed, PSD cones projected on chip) whose
    rule takes the shape and the layout -- so a layout with a PSD segment goes to the SDP batch and every other one where
    own_a_batch sends it --, else a ValueError that names FusedSolver.  
    Crossover against one FusedSolver(schedule="carried") per problem in turn (profiles/sdpbatch_rate.txt, one MI355X): there is none
    in what was measured.  The SDP batch wins at every one of the five layouts run (45 x 6 order 9 .. 1176 x 48 order 48) and every P,
    down to P = 16 -- by 9.2x (560 x 528) to 14x there, by 135x to 222x at P = 256 --, so the choice is by rule alone.  Below P = 16
    nothing was measured; a single problem is FusedSolver's case."""
    denses = OwnBatchSolver.check_same_layout(denses)
    d0 = denses[0]
    cls = first_that_takes(_mb.FAMILIES + ((SdpBatchSolver, fits),), d0.n, d0.m, d0.seg_type, d0.seg_len,
                           "none of SmallBatchSolver, MidBatchSolver and SdpBatchSolver takes %d x %d problems with this cone layout "
                           "(%s): run one FusedSolver per problem")
    return cls.from_dense(denses, param, **kw)
