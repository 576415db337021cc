"""`SparseMatOp`: a sparse matrix as a linear `Operator` (totsu_core/src/solver/operator.rs:11-156) for the trait-level
`Solver(F32HIP)` -- the user-defined-operator pattern of examples/imgnr_udef/src/prob_op_a.rs with the matrix kept
sparse on the device.  Default: ONE tiled copy serving `op` and `trans_op` (`SpTile`, thip_sptile_*); `two_copies=True`
keeps the round-5 form, CSR of A and of A^T (one right-hand side per call; the A/B leg of bench.py's sparse workloads).
Both forms give bitwise reproducible sums."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib


class _DevInts:
    def __init__(self, a, dtype):
        a = np.ascontiguousarray(a, dtype=dtype)
        self.nbytes = a.nbytes
        nfl = max((a.nbytes + 3) // 4, 1)
        p = C.c_void_p()
        lib.thip_alloc(nfl, C.byref(p))
        self.ptr = p.value
        if a.nbytes:
            pad = np.zeros(nfl * 4, dtype=np.uint8)
            pad[:a.nbytes] = a.view(np.uint8)
            lib.thip_h2d(self.ptr, pad.ctypes.data, nfl)

    def free(self):
        if self.ptr is not None:
            lib.thip_free(self.ptr)
            self.ptr = None


class _Csr:
    def __init__(self, m):
        m = m.tocsr()
        m.sort_indices()
        self.shape = m.shape
        self.nnz = int(m.nnz)
        self.rowptr = _DevInts(m.indptr, np.int64)
        self.colidx = _DevInts(m.indices, np.int32)
        self.vals = _DevInts(m.data.astype(np.float32).view(np.int32), np.int32)

    def mv(self, alpha, x, beta, y, abs_mode=0):
        # abs mode ignores x (taken as all-ones): pass a pointer that does not alias y
        xp = self.vals.ptr if abs_mode else x.dev()
        lib.thip_spmv_csr(self.shape[0], self.shape[1], self.nnz, self.rowptr.ptr, self.colidx.ptr, self.vals.ptr,
                          float(alpha), xp, float(beta), y.dev(), abs_mode)

    def free(self):
        for d in (self.rowptr, self.colidx, self.vals):
            d.free()


class SpTile:
    """A sparse matrix held ONCE on the device in 4096 x 4096 tiles (thip_sptile_*, totsu_amd/csrc/thip_sptile.hip): both
    products stream the same stored entries.  Built from a scipy.sparse matrix through its CSC arrays on the host, or -- `from_dense`,
    `Builder` -- on the device from a dense column-major array, which is what every Prob* builder and MatBuild produce."""

    def __init__(self, mat):
        _lib.ensure_init()
        m = mat.tocsc()
        if not m.has_sorted_indices:
            m = m.sorted_indices()      # (a copy: tocsc() of a CSC matrix is the caller's own object)
        self.shape = m.shape
        self.nnz = int(m.nnz)
        colptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
        rowidx = np.ascontiguousarray(m.indices, dtype=np.int32)
        vals = np.ascontiguousarray(m.data, dtype=np.float32)
        h = C.c_void_p()
        lib.thip_sptile_create(self.shape[0], self.shape[1], self.nnz, colptr.ctypes.data, rowidx.ctypes.data,
                               vals.ctypes.data, C.byref(h))
        self.h = h

    @staticmethod
    def from_csc_arrays(n_row, n_col, colptr, rowidx, vals):
        """host CSC arrays as they are (int64 / int32 / float32): no scipy object in between (bench.py's GB-sized operators)"""
        _lib.ensure_init()
        self = SpTile.__new__(SpTile)
        self.shape = (int(n_row), int(n_col))
        self.nnz = int(vals.size)
        assert colptr.dtype == np.int64 and rowidx.dtype == np.int32 and vals.dtype == np.float32
        assert colptr.flags.c_contiguous and rowidx.flags.c_contiguous and vals.flags.c_contiguous
        h = C.c_void_p()
        lib.thip_sptile_create(self.shape[0], self.shape[1], self.nnz, colptr.ctypes.data, rowidx.ctypes.data,
                               vals.ctypes.data, C.byref(h))
        self.h = h
        return self

    class Builder:
        """thip_sptile_builder_*: the tiled copy from dense column-major panels ON THE DEVICE, in two passes -- count every column
        once, plan(), fill every column once, finish() -- for callers that produce panels themselves.  A panel is a DeviceBuffer (or
        a device address) holding columns [c0, c0 + ncols) with leading dimension ld >= n_row; panels may come in any order and width,
        and may all live in one staging buffer refilled between the calls."""

        def __init__(self, n_row, n_col):
            _lib.ensure_init()
            self.shape = (int(n_row), int(n_col))
            self.planned = None
            h = C.c_void_p()
            lib.thip_sptile_builder_create(self.shape[0], self.shape[1], C.byref(h))
            self.h = h

        def _panel(self, panel, ncols, ld):
            ld = self.shape[0] if ld is None else int(ld)
            ptr = getattr(panel, "ptr", panel)
            if hasattr(panel, "n") and ncols > 0 and ld >= self.shape[0]:
                assert panel.n >= (ncols - 1) * ld + self.shape[0], "panel buffer shorter than its columns"
            return ptr, ld

        def count(self, c0, ncols, panel, ld=None):
            ptr, ld = self._panel(panel, int(ncols), ld)
            lib.thip_sptile_builder_count(self.h, int(c0), int(ncols), ptr, ld)

        def plan(self):
            """after every column was counted: allocates the store and reports what the finished object's info() will -- nnz, tiles
            held without indices, entries that carry an index, bytes one product streams"""
            nz, nd, ni, bp = C.c_size_t(), C.c_int(), C.c_size_t(), C.c_size_t()
            lib.thip_sptile_builder_plan(self.h, C.byref(nz), C.byref(nd), C.byref(ni), C.byref(bp))
            self.planned = {"nnz": nz.value, "dense_tiles": nd.value, "indexed_entries": ni.value, "bytes_per_product": bp.value}
            return dict(self.planned)

        def fill(self, c0, ncols, panel, ld=None):
            ptr, ld = self._panel(panel, int(ncols), ld)
            lib.thip_sptile_builder_fill(self.h, int(c0), int(ncols), ptr, ld)

        def finish(self):
            """the finished SpTile (the caller frees it); the builder is destroyed"""
            h = C.c_void_p()
            lib.thip_sptile_builder_finish(self.h, C.byref(h))
            out = SpTile.__new__(SpTile)
            out.shape, out.nnz, out.h = self.shape, int(self.planned["nnz"]), h
            self.destroy()
            return out

        def destroy(self):
            if getattr(self, "h", None) is not None:
                lib.thip_sptile_builder_destroy(self.h)
                self.h = None

        def __del__(self):
            try:
                self.destroy()
            except Exception:
                pass

    @staticmethod
    def _dense_feed(a, n_row, n_col, ld=None, panel_cols=None):
        """-> (pass, release): pass(f) calls f(c0, ncols, panel, ld) once per panel of the dense column-major matrix `a`.  A
        DeviceBuffer holding the whole matrix is one panel.  A host array -- flat column-major with leading dimension ld, or 2-D
        (n_row, n_col), read column by column: no F-ordered copy of the whole is made -- is streamed through ONE staging DeviceBuffer
        of panel_cols columns (default: about 256 MB of them) with thip_h2d, so the dense matrix never exists on the device."""
        from .fused import DeviceBuffer
        n_row, n_col = int(n_row), int(n_col)
        if isinstance(a, DeviceBuffer):
            ld_ = n_row if ld is None else int(ld)
            return (lambda f: f(0, n_col, a, ld_)), (lambda: None)
        a = np.asarray(a)
        two_d = a.ndim == 2
        if two_d:
            assert a.shape == (n_row, n_col) and ld is None
            ld_ = n_row
        else:
            ld_ = n_row if ld is None else int(ld)
            assert ld_ >= n_row and (n_col == 0 or a.size >= (n_col - 1) * ld_ + n_row)
        pc = max(1, (256 << 20) // (4 * max(ld_, 1))) if panel_cols is None else max(1, int(panel_cols))
        pc = max(1, min(pc, n_col))
        stage = DeviceBuffer(max(pc * ld_, 1))

        def run(f):
            for c0 in range(0, n_col, pc):
                nc = min(pc, n_col - c0)
                if two_d:
                    host = np.ascontiguousarray(a[:, c0:c0 + nc].T, dtype=np.float32)      # nc columns, each contiguous
                else:
                    host = np.ascontiguousarray(a[c0 * ld_:min(a.size, (c0 + nc) * ld_)], dtype=np.float32)
                if host.size:
                    lib.thip_h2d(stage.ptr, host.ctypes.data, host.size)
                f(c0, nc, stage, ld_)
        return run, stage.free

    @staticmethod
    def from_dense(a, n_row, n_col, ld=None, panel_cols=None):
        """The tiled copy of a DENSE column-major n_row x n_col matrix, zeros dropped (an entry is stored iff its bit pattern
        without the sign is non-zero): the object SpTile(scipy.sparse.csc_matrix(a)) builds, made on the device in two passes over
        the matrix.  `a`: a DeviceBuffer holding the whole matrix (leading dimension ld, default n_row) -- the count / plan / fill /
        finish sequence of thip_sptile_from_dense, through the builder so that nnz is known --, or a host array (flat column-major
        or 2-D), streamed twice through one staging buffer of panel_cols columns (see _dense_feed)."""
        b = SpTile.Builder(n_row, n_col)
        run, release = SpTile._dense_feed(a, n_row, n_col, ld, panel_cols)
        try:
            run(b.count)
            b.plan()
            run(b.fill)
            return b.finish()
        finally:
            b.destroy()
            release()

    def mv(self, transpose, alpha, x, beta, y, abs_mode=0):
        xp = y.dev() if abs_mode else x.dev()          # abs mode ignores x (taken as all-ones)
        lib.thip_sptile_mv(self.h, 1 if transpose else 0, float(alpha), xp, float(beta), y.dev(), abs_mode)

    def info(self):
        nz, by = C.c_size_t(), C.c_size_t()
        t, i_n, i_t, s_n, s_t = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        lib.thip_sptile_info(self.h, C.byref(nz), C.byref(t), C.byref(i_n), C.byref(i_t), C.byref(s_n), C.byref(s_t), C.byref(by))
        nd, ni, bp = C.c_int(), C.c_size_t(), C.c_size_t()
        lib.thip_sptile_layout(self.h, C.byref(nd), C.byref(ni), C.byref(bp))
        return {"nnz": self.nnz, "nnz_stored": nz.value, "tiles": t.value, "items_n": i_n.value, "items_t": i_t.value,
                "slices_n": s_n.value, "slices_t": s_t.value, "device_bytes": by.value,
                "dense_tiles": nd.value, "indexed_entries": ni.value, "bytes_per_product": bp.value}

    def free(self):
        if getattr(self, "h", None) is not None:
            lib.thip_sptile_destroy(self.h)
            self.h = None


class SparseMatOp:
    """Operator over a scipy.sparse matrix, for L = F32HIP."""

    def __init__(self, L, mat, two_copies=False):
        """two_copies: the round-5 form (CSR of A and CSR of A^T, both gathers deterministic); default: one tiled copy"""
        assert getattr(L, "name", "") == "F32HIP"
        _lib.ensure_init()
        self.L = L
        self.n_row, self.n_col = mat.shape
        self.t = None if two_copies else SpTile(mat)
        self.a = _Csr(mat) if two_copies else None
        self.at = _Csr(mat.T) if two_copies else None

    def size(self):
        return (self.n_row, self.n_col)

    def op(self, alpha, x, beta, y):
        assert x.len() == self.n_col and y.len() == self.n_row
        if self.n_row and self.n_col:
            self.t.mv(False, alpha, x, beta, y) if self.t else self.a.mv(alpha, x, beta, y)
        else:
            self.L.scale(beta, y)

    def trans_op(self, alpha, x, beta, y):
        assert x.len() == self.n_row and y.len() == self.n_col
        if self.n_row and self.n_col:
            self.t.mv(True, alpha, x, beta, y) if self.t else self.at.mv(alpha, x, beta, y)
        else:
            self.L.scale(beta, y)

    def absadd_cols(self, tau):          # tau[c] += sum_r |A(r,c)|  (operator.rs:82-113 reference semantics)
        assert tau.len() == self.n_col
        if self.n_row and self.n_col:
            self.t.mv(True, 1.0, None, 1.0, tau, abs_mode=1) if self.t else self.at.mv(1.0, None, 1.0, tau, abs_mode=1)

    def absadd_rows(self, sigma):
        assert sigma.len() == self.n_row
        if self.n_row and self.n_col:
            self.t.mv(False, 1.0, None, 1.0, sigma, abs_mode=1) if self.t else self.a.mv(1.0, None, 1.0, sigma, abs_mode=1)

    def drop(self):
        for d in (self.t, self.a, self.at):
            if d is not None:
                d.free()


# the read rates the README records for the two schedules, as fractions of the HBM peak: the dense one-pass sweep, and the tiled
# products on the worst scattered pattern
DENSE_RATE, TILED_WORST_RATE = 0.90, 0.53


def choose_layout(n_row, n_col, bytes_per_product):
    """"tiled" or "dense" for a matrix whose tiled copy streams `bytes_per_product` bytes per product (SpTile.info(), Builder.plan()).
    Per iteration the dense one-pass schedule reads 4 n_row n_col bytes once, the tiled schedule reads bytes_per_product twice, and
    the tiled products run at best 1.7 times slower per byte on a scattered pattern (0.90 / 0.53 of peak, the README's recorded
    rates).  The rule: tiled iff 2 * 1.7 * bytes_per_product < 4 * n_row * n_col.  That 1.7 is a MODEL built from two recorded rates,
    not a measured crossover.  Pure host code."""
    return "tiled" if 2 * 1.7 * int(bytes_per_product) < 4 * int(n_row) * int(n_col) else "dense"
