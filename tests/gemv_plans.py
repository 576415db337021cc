"""What the tests of the single-vector dual GEMV's tilings share: the plans the autotune times (gemv_candidates() in
totsu_amd/csrc/thip_gemv.hip, in its order -- thip_test_solver_pin_gemv_plan takes an index into it) and the planning hook."""
import ctypes as C

CANDIDATES = [(1, 8192), (1, 4096), (2, 8192), (2, 2048), (4, 8192), (4, 4096), (4, 2048), (4, 1024), (4, 768)]
BLK, MAXCW = 256, 1024          # threads per workgroup; the most columns a chunk may hold


def plan(m, n, vw, nj=0, target_blocks=0, col0=0, col1=None):
    """thip_test_gemv_plan (no GPU): (plan record as a dict, dual_gemv_scratch_floats(m, n), the solver's split column for n)"""
    from totsu_amd import _lib
    rec, scr, split = _lib.GemvPlanRec(), C.c_size_t(), C.c_size_t()
    _lib.lib.thip_test_gemv_plan(m, n, vw, nj, target_blocks, col0, n if col1 is None else col1, C.byref(rec), C.byref(scr),
                                 C.byref(split))
    return {k: getattr(rec, k) for k, _ in rec._fields_}, scr.value, split.value
