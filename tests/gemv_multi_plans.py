"""What the tests of the multi-vector dual GEMV's tilings share: the plans its autotune times (gemv_multi_candidates() in
totsu_amd/csrc/thip_gemv_multi.hip, in its order -- thip_test_batch_pin_multi_plan takes an index into it), a restatement of the
planner (multi_plan) and of the scratch rule (dual_gemv_multi_scratch_floats) in plain Python, and the planning hook."""
import ctypes as C

import numpy as np

CANDIDATES = [(1, 8192), (1, 4096), (1, 2048), (2, 8192), (2, 4096), (2, 2048), (2, 1024)]
BLK, VW, MCW = 256, 4, 256          # threads per workgroup; rows per load; the most columns a chunk may hold (the LDS limit)
INSTANCES = [2, 4, 8]
FORMS = [(2, 1), (2, 2), (4, 1), (4, 2), (8, 1)]          # (kernel instance, row groups per lane) the library has kernels for
# the (instance, candidate index) pairs the autotune can pick: NV = 8 holds one row group per lane
PAIRS = [(inst, k) for inst in INSTANCES for k, (nj, _) in enumerate(CANDIDATES) if inst < 8 or nj == 1]
FIELDS = ("vw", "nj", "ku", "tiles", "chunks", "cols_per_chunk", "m_load")


def _up(v, a):
    return (v + a - 1) // a * a


def restated_plan(m, n, instance, nj=0, target_blocks=0):
    """multi_plan in plain integers: the fields of the plan record the hook fills"""
    nj = 2 if (nj >= 2 and instance < 8) else 1
    tile = BLK * VW * nj
    tiles = -(-m // tile)
    tb = int(float(m) * float(n) * 4.0 / 2.0e5)          # 0.2 MB of A per workgroup, 2048 .. 8192 workgroups
    tb = min(max(tb, 2048), 8192)
    if target_blocks > 0:
        tb = target_blocks
    chunks = max(tb // tiles, 1)
    cpc = -(-n // chunks)
    cpc = max(cpc, 16 if float(m) * float(n) * 4.0 < 64.0e6 else 32)
    cpc = min(_up(cpc, 8), MCW)
    return {"vw": VW, "nj": nj, "ku": 8 // nj, "tiles": tiles, "chunks": -(-n // cpc), "cols_per_chunk": cpc, "m_load": _up(m, VW)}


def restated_scratch(m, n):
    """dual_gemv_multi_scratch_floats: the most any plan the library can come to run needs, + 64"""
    best = 0
    for inst in (2, 8):
        for nj, tb in [(0, 0)] + CANDIDATES:
            p = restated_plan(m, n, inst, nj, tb)
            best = max(best, p["chunks"] * _up(m, 4) + p["tiles"] * _up(n, 4))
    return best + 64


def plan(m, n, instance, nj=0, tb=0):
    """thip_test_gemv_multi_plan (no GPU): (the plan record's fields in use as a dict, dual_gemv_multi_scratch_floats(m, n))"""
    from totsu_amd import _lib
    rec, scr = _lib.GemvPlanRec(), C.c_size_t()
    _lib.lib.thip_test_gemv_multi_plan(m, n, instance, nj, tb, C.byref(rec), C.byref(scr))
    assert (rec.chunks2, rec.cols_per_chunk2, rec.reserved) == (0, 0, 0)
    return {k: getattr(rec, k) for k in FIELDS}, scr.value


def blocks_for(m, n, instance, nj, cpc):
    """a target_blocks under which the planner gives exactly `cpc` columns per chunk on this shape (None: there is none)"""
    tiles = -(-m // (BLK * VW * (2 if nj >= 2 and instance < 8 else 1)))
    for chunks in range(1, n + 1):
        if restated_plan(m, n, instance, nj, chunks * tiles)["cols_per_chunk"] == cpc:
            return chunks * tiles
    return None


# ---- the LPs of the solver-level tests ------------------------------------------------------------------------------------------

ITERS, TOLS = [0, 1, 9], [2e-5, 2e-5, 1e-4]          # iterates 0, 1, 9 relative to the iterate's max norm (tests/test_gpu_batch.py)
PIN_SHAPE = (6, 300_000)                             # the seven candidates are seven different plans here
TUNE_SHAPE = (4096, 1024)                            # m n = 2^22: the least matrix the autotune times


def lp_data(m, n):
    """one nonnegative cone of m rows: A standard normal, b_i ~ U(0, 1), c_i ~ -U(0, 1) for eight instances, all from default_rng(3)"""
    rng = np.random.default_rng(3)
    a = rng.standard_normal((m, n)).astype(np.float32)
    bs, cs = [], []
    for _ in range(8):
        bs.append(rng.uniform(0, 1, m).astype(np.float32))
        cs.append((-rng.uniform(0, 1, n)).astype(np.float32))
    return a, bs, cs
