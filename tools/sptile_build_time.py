"""Build time of the tiled sparse copy (thip_sptile.hip) by route, on dense, mostly-zero matrices of a few hundred MB as the Prob*
builders produce them (tests/problems.l1reg_lp, partitioning_sdp through ProbSDP.dense()):
  host CSC       thip_sptile_create from host CSC arrays (single-threaded assembly on the host) -- and what a caller that holds the
                 matrix dense pays in front of it, scipy.sparse.csc_matrix(dense)
  device dense   SpTile.from_dense from the dense array already on the device (two passes: count, plan, fill)
  host dense     SpTile.from_dense from the host array, streamed twice through one staging buffer (no dense device copy)
One line per route, best of three; the routes build the same object (checked with thip_test_sptile_equal).  A record, not a gate; its
output is kept under profiles/.
    python tools/sptile_build_time.py"""
import ctypes as C
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import totsu_amd as T  # noqa: E402
from totsu_amd import _lib  # noqa: E402
from totsu_amd._lib import lib  # noqa: E402
from totsu_amd.sparse import SpTile  # noqa: E402


def best_of(f, reps=3):
    best, out = 1e30, None
    for _ in range(reps):
        if out is not None:
            out.free()
        lib.thip_sync()
        t0 = time.perf_counter()
        out = f()
        lib.thip_sync()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3, out


def instances():
    from problems import l1reg_lp, partitioning_sdp
    c, G, h = l1reg_lp(2500, seed=0)
    yield "l1reg_lp(l=2500)", np.asfortranarray(G, dtype=np.float32)
    w, syms_f, mat_a, vec_b = partitioning_sdp(12, 10, seed=0)
    l, n = 120, w.size
    mb = lambda typ: T.MatBuild(T.F32HIP, typ)
    sdp = T.ProbSDP(mb(T.MatType.General(n, 1)).set_array(w.reshape(-1, 1)), [mb(T.MatType.SymPack(l)).set_array(s_) for s_ in syms_f],
                    mb(T.MatType.General(l, n)).set_array(mat_a), mb(T.MatType.General(l, 1)).set_array(vec_b.reshape(-1, 1)), 1e-12)
    d = sdp.dense()
    yield "partitioning_sdp(12, 10) through ProbSDP.dense()", np.asarray(d.mat_a, np.float32).reshape((d.m, d.n), order="F")
    sdp.drop()


def main():
    _lib.init()
    for name, A in instances():
        m, n = A.shape
        flat = A.ravel(order="F")
        t0 = time.perf_counter()
        csc = sp.csc_matrix(A)
        t_scipy = (time.perf_counter() - t0) * 1e3
        colptr, rowidx, vals = csc.indptr.astype(np.int64), csc.indices.astype(np.int32), csc.data.astype(np.float32)
        print("%s: %d x %d, %.0f MB dense, nnz %d (%.2f %%)" % (name, m, n, A.nbytes / 1e6, csc.nnz, 100.0 * csc.nnz / A.size))
        t_h, H = best_of(lambda: SpTile.from_csc_arrays(m, n, colptr, rowidx, vals))
        print("  host CSC     (thip_sptile_create)                  %9.1f ms   (+ scipy.sparse.csc_matrix(dense): %.1f ms)" % (t_h, t_scipy))
        buf = T.DeviceBuffer.from_host(flat)
        t_d, D = best_of(lambda: SpTile.from_dense(buf, m, n))
        print("  device dense (SpTile.from_dense, DeviceBuffer)      %9.1f ms" % t_d)
        t_s, Dh = best_of(lambda: SpTile.from_dense(flat, m, n))
        print("  host dense   (SpTile.from_dense, streamed twice)    %9.1f ms" % t_s)
        diff = C.c_int(-1)
        for other in (D, Dh):
            lib.thip_test_sptile_equal(H.h, other.h, C.byref(diff))
            assert diff.value == 0, diff.value
        for o in (H, D, Dh, buf):
            o.free()


if __name__ == "__main__":
    main()
