"""`WideBatchSolver`: many conic programs, each with its OWN dense f32 A (one shape n, m and one cone layout; their own A_p, b_p,
c_p), of EVERY shape up to 4096 x 4096 and every PSD order up to 64 -- the shapes whose vectors do not fit the LDS of a CU, which
`MidBatchSolver` and `SdpBatchSolver` refuse: 2020 x 1000, 4096 x 4096, a PSD cone of order 58 .. 64, order 48 with n > 836
(thip_widebatch_* in include/totsu_f32hip.h).  The kernel is the SDP batch's iteration -- one workgroup per problem, A streamed twice
per iteration, the PSD cones projected by the workgroup itself -- with one difference: only what a pass over A touches lies in LDS
(the iterates x_x u x_y v, the pass results, the class bytes, the PSD operands); every other vector is read and written in place in
the problem's block of the arena (6 n + 11 m floats).  The host machinery, the methods and the ValueErrors are `OwnBatchSolver`'s
(totsu_amd/ownbatch.py); on a shape the mid or the SDP batch also takes, the iterates are theirs bit for bit.

Taken: 1 <= m, n <= 4096; the zero, nonnegative, second-order, rotated second-order and PSD cones, every PSD segment of
k (k + 1) / 2 rows with 1 <= k <= 64; an LDS map of at most 163 840 bytes -- 4 (6208 + 3 n + 3 m) + roundup4(m), plus 49 920 when the
largest PSD order exceeds 32 (`fits` is the rule).  Without such an order every shape fits (4096 x 4096 takes 127 232 bytes); with one
the rule reads 12 (n + m) + roundup4(m) <= 89 088: an order-64 cone alone (m = 2080) takes every n <= 4096, and m = 4096 takes
n <= 2986.  Refused (ValueError, each in its own words): m beyond 4096, n beyond 4096, a PSD length that is not triangular, an order
above 64, a map beyond LDS; segments that do not cover m, no problem at all, arrays of the wrong length.

No chooser returns this class -- `own_a_batch`, `conic_batch` and `ragged_batch` refuse what they refused: against one
FusedSolver(schedule="carried") per problem in turn the wide batch wins only from some number of problems on (README.md has what
was measured), so the choice is the caller's."""
from . import _lib
from .ownbatch import _fits
from .sdpbatch import SdpBatchSolver


def fits(n, m, seg_type, seg_len):
    """the shape rules alone (thip_widebatch_fits; needs no GPU): (lds_bytes, threads) of one workgroup, or ValueError"""
    return _fits("thip_widebatch_", n, m, seg_type, seg_len)


def lds_rule(n, m, max_psd_order=0):
    """the rule's left-hand side, restated: the LDS bytes of one problem's workgroup in the iteration"""
    return 4 * (6208 + 3 * n + 3 * m) + ((m + 3) & ~3) + (49920 if max_psd_order > 32 else 0)


class WideBatchSolver(SdpBatchSolver):
    """the constructor, from_dense, run / run_until_any / status / solution / iterate / precond / replace / set_iterates / set_bc /
    set_a / solutions and their _dev twins / info / solve of SdpBatchSolver, on thip_widebatch_*.  force_threads: test hook (256,
    1024).  info() adds lds_bytes_per_problem (what `fits` reports) and arena_bytes_per_problem (4 (6 n + 11 m))."""
    _prefix, _force_hook, _what, _Info = "thip_widebatch_", "thip_test_widebatch_force_threads", "wide", _lib.WideBatchInfo
