"""`SmallBatchSolver`: hundreds or thousands of SMALL conic programs, each with its OWN dense f32 A (one shape n, m and one cone
layout; their own A_p, b_p, c_p), iterated on chip (thip_smallbatch_* in include/totsu_f32hip.h) -- scenario sets, one problem
per agent, per fold, per pixel.  One workgroup per problem holds the problem's A in the LDS of its CU (m * n <= 24 576) and runs
whole iterations of the reference's loop with no launch boundary inside; a launch advances every running problem by poll_every
iterations, the host then reads all status blocks at once and launches over the problems still running.  The constructor, the
methods and the ValueErrors are `OwnBatchSolver`'s (totsu_amd/ownbatch.py).

Taken: the zero, nonnegative, second-order and rotated second-order cones; "compensated" and "plain" state arithmetic.  Refused
(ValueError): PSD segments, m or n beyond 1024, m * n beyond 24 576, segments that do not cover m, no problem at all, arrays of
the wrong length."""
from . import _lib
from .ownbatch import OwnBatchSolver, _fits


def fits(n, m, seg_type, seg_len):
    """the shape rules alone (thip_smallbatch_fits; needs no GPU): (lds_bytes, threads) of one workgroup, or ValueError"""
    return _fits("thip_smallbatch_", n, m, seg_type, seg_len)


class SmallBatchSolver(OwnBatchSolver):
    """OwnBatchSolver on thip_smallbatch_*.  force_threads: test hook (64, 256, 1024)."""
    _prefix, _force_hook, _what, _Info = "thip_smallbatch_", "thip_test_smallbatch_force_threads", "small", _lib.SmallBatchInfo
