/*
 * totsu_f32hip.h -- C ABI of libtotsu_f32hip.so, the MI355X (gfx950) linear-algebra backend for
 * Totsu's first-order conic solver.  This is the drop-in boundary: a Rust `totsu_f32hip` crate
 * (`F32HIP: LinAlgEx`, `F32HIPSlice: SliceLike`) binds exactly these entry points,
 * the way `totsu_f32cuda` binds cuBLAS / cuSOLVER.
 *
 * Conventions
 *   - every `float *` / `const float *` is a DEVICE pointer unless the name starts with `host_`;
 *   - every call enqueues on the context stream (thip_set_stream) and returns without
 *     synchronising, except the ones that return a host scalar (marked SYNC).  This holds as stated by DEFAULT and
 *     always while a caller-provided stream is installed.  A host that drives everything through this API may opt into
 *     deferred execution of small calls with thip_set_lazy_gemv(1) (see there): those calls are then enqueued at the
 *     latest when the next non-deferred entry point -- including thip_get_stream / thip_sync -- is entered, so call
 *     order is still what every thip_* caller observes, but work the HOST enqueues by itself on the stream must be
 *     preceded by thip_get_stream();
 *   - return value: 0 = ok, otherwise a hipError_t (or THIP_E_* below); thip_last_error() gives text.
 *     The reference backends assert on library status (f32cuda.rs:38 etc.): a binding should
 *     `assert_eq!(rc, 0)`;
 *   - zero-length vectors and zero-sized matrices are legal everywhere (matop.rs:83-85);
 *   - one context per process (one process per GPU); like the reference's backends (thread_local state, !Send types)
 *     the API is meant to be driven from one host thread -- uploads and the shared scratch are mutex-protected, and
 *     separate thip_solver objects may be driven from separate threads (they own their scratch);
 *   - citations are relative to /root/reference/solver_rust_conic/.
 */
#ifndef TOTSU_F32HIP_H
#define TOTSU_F32HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define THIP_E_INVALID   10001   /* bad argument */
#define THIP_E_NOTINIT   10002
#define THIP_E_NOGPU     10003   /* no HIP device: the product path fails loudly, there is no CPU fallback */
#define THIP_E_WORK      10004   /* work buffer too short */
#define THIP_E_NOCONV    10005   /* eigen iteration did not converge */
#define THIP_E_TIMEOUT   10006   /* a bounded device-side wait ran out (a peer rank or its host stalled, or the one-pass kernel
                                  * gave up on some rank of a column-sharded run): the solve cannot go on consistently */

/* ---------------------------------------------------------------------------------------------
 * Context.  Replaces totsu_f32cuda/src/cuda_mgr.rs:24-111 (context + cuBLAS/cuSOLVER handles,
 * device 0 only there; any device here).
 * ------------------------------------------------------------------------------------------- */
int  thip_init(int device);                        /* cuda_mgr.rs:30-60 */
int  thip_shutdown(void);
int  thip_device_count(int *host_count);
int  thip_set_stream(void *hip_stream);            /* NULL = the context's own stream */
/* (device memory handed to a call -- the dev_* arrays of create, replace and the thip_*batch _dev calls -- is read and written on
 * this stream: a caller that produces it on another stream orders that work first, and reads what _solutions_dev wrote only after
 * this stream reached the launch) */
void *thip_get_stream(void);                       /* runs what is deferred first; NULL = that failed (thip_last_error) */
int  thip_sync(void);                              /* SYNC */
const char *thip_last_error(void);
const char *thip_version(void);

/* device memory: replaces cuda_mgr.rs:119-138 (buf_from_slice / buf_zeroes) and
 * f32cuda_slice.rs:343-355 (sync_from_dev / sync_from_host) */
int thip_alloc(size_t n, float **out);             /* n floats, 256-byte aligned, NOT zeroed */
int thip_alloc_zeroed(size_t n, float **out);
int thip_free(float *p);
int thip_h2d(float *dst, const float *host_src, size_t n);     /* async on the stream (pageable src: staged) */
int thip_d2h(float *host_dst, const float *src, size_t n);     /* SYNC */
int thip_get(const float *x, size_t idx, float *host_out);     /* SYNC; SliceLike::get, slicelike.rs:54-59 */
int thip_set(float *x, size_t idx, float val);                 /*       SliceLike::set, slicelike.rs:62-69 */

/* ---------------------------------------------------------------------------------------------
 * LinAlg (totsu_core/src/solver/linalg.rs:10-68); CUDA counterparts f32cuda.rs:27-136
 * ------------------------------------------------------------------------------------------- */
int thip_norm(size_t n, const float *x, float *host_out);                       /* SYNC  linalg.rs:22  (cublasSnrm2, f32cuda.rs:27-42) */
int thip_copy(size_t n, const float *x, float *y);                              /*       linalg.rs:29  (f32cuda.rs:44-57) */
int thip_scale(size_t n, float alpha, float *x);                                /*       linalg.rs:35  (f32cuda.rs:59-69) */
int thip_add(size_t n, float alpha, const float *x, float *y);                  /*       linalg.rs:42  (f32cuda.rs:71-84) */
int thip_adds(size_t n, float s, float *y);                                     /*       linalg.rs:49  (f32cuda.rs:86-99) */
int thip_abssum(size_t len, const float *x, size_t incx, float *host_out);      /* SYNC  linalg.rs:56  (f32cuda.rs:101-121); sums |x[0]|,|x[incx]|,.. < len */
int thip_transform_di(size_t n, float alpha, const float *d, const float *x,
                      float beta, float *y);                                    /*       linalg.rs:67  (cublasSsbmv k=0, f32cuda.rs:123-136) */

/* ---------------------------------------------------------------------------------------------
 * LinAlgEx (totsu_core/src/linalg_ex.rs:7-66); CUDA counterparts f32cuda.rs:144-370
 * ------------------------------------------------------------------------------------------- */
/* y = alpha * G^(T) x + beta * y, G column-major n_row x n_col, lda = n_row.
 * linalg_ex.rs:23 (cublasSgemv, f32cuda.rs:144-171) */
int thip_transform_ge(int transpose, size_t n_row, size_t n_col, float alpha, const float *mat,
                      const float *x, float beta, float *y);
/* OPT-IN deferred, batched execution of small calls (off by default; off while a caller stream is installed with
 * thip_set_stream): thip_transform_ge on matrices <= 64 MB, thip_scale / thip_add on vectors <= 1024 long and the
 * single-cone projections thip_proj_soc / _rotsoc / _rpos / _zero are RECORDED instead of launched.  A composite operator
 * issues them per block (ProbSOCPOpA / ProbSOCPOpB, socp.rs:77-130,194-246: 5000 per product at BASELINE configs[2];
 * ProbSOCPCone::proj, socp.rs:296-313: 1000 per projection); the library runs the record -- one grouped launch per kind
 * of product plus one finishing launch, one launch for a run of projections -- as soon as ANY other entry point is
 * called or a new call would read or overwrite a pending result, so call order is still what every caller of this API
 * observes.  Contributions to the same y are summed in a fixed order of their own (last-bit differences from sequential
 * accumulation).  Errors of a deferred call surface at the entry point that runs the record.  The trait-level hosts
 * (include/totsu_f32hip.hpp Solver, totsu_amd.Solver, the Rust crate's init()) switch it on for their own calls;
 * THIP_LAZY_GEMV=1 switches it on from the environment. */
int thip_set_lazy_gemv(int on);
int thip_get_lazy_gemv(int *host_on);
int thip_lazy_gemv_stats(int64_t *host_deferred, int64_t *host_flushes);
/* a flushed segment is kept as a plan (call list, device tables, launch geometry); the loop repeats its call sequence
 * every iteration, so the next pass re-uses the plan (hit) instead of analysing and building again (miss) */
int thip_lazy_plan_stats(int64_t *host_hits, int64_t *host_misses);
/* read-ahead of SYNC scalars (deferred mode only): the thip_get / thip_norm calls of a host loop that asks for the same
 * addresses every pass -- the reference's ConeSOC::proj, cone_soc.rs:44-47, 2 reads per cone -- are learnt, and on the next
 * pass the first read fetches all of them with one kernel and one transfer (a fetch); the others are served from the host
 * copy as long as each request is the predicted one and nothing issued in between writes a range still to be read */
int thip_lazy_read_stats(int64_t *host_served, int64_t *host_fetches);
/* y = alpha * S x + beta * y, S symmetric, packed upper by columns.  linalg_ex.rs:37 (cublasSspmv, f32cuda.rs:174-187) */
int thip_transform_sp(size_t n, float alpha, const float *mat, const float *x, float beta, float *y);
/* Reduced-precision STORAGE of a dense operator (not part of the reference's trait surface):
 * bf16 elements (round to nearest even), f32 accumulation.  mat16 is column-major with leading dimension ld16 >= n_row
 * (a multiple of 8 and a 16-byte aligned base give the 16-byte-load kernel); rows n_row..ld16 are written as zeros.
 * thip_transform_ge_bf16 has the semantics of thip_transform_ge on the rounded matrix. */
enum { THIP_A_F32 = 0, THIP_A_BF16 = 1, THIP_A_F16 = 2 };
int thip_to_bf16(size_t n_row, size_t n_col, const float *mat, uint16_t *mat16, size_t ld16);
int thip_transform_ge_bf16(int transpose, size_t n_row, size_t n_col, float alpha, const uint16_t *mat16, size_t ld16,
                           const float *x, float beta, float *y);
/* The same with IEEE f16 elements and one power-of-two scale per column (8x finer rounding than bf16 at the same
 * bytes; the scale keeps any f32 column inside f16's range): stored(r, c) = f16(a(r, c) * s_c), s_c the power of two
 * that brings the column's largest magnitude into [2^13, 2^14); inv_scale[c] = 1 / s_c (n_col floats, written by
 * thip_to_f16, read by the products). */
int thip_to_f16(size_t n_row, size_t n_col, const float *mat, uint16_t *mat16, size_t ld16, float *inv_scale);
int thip_transform_ge_f16(int transpose, size_t n_row, size_t n_col, float alpha, const uint16_t *mat16, size_t ld16,
                          const float *inv_scale, const float *x, float beta, float *y);
/* linalg_ex.rs:44 (f32cuda.rs:243-251) */
size_t thip_map_eig_worklen(size_t n);
/* linalg_ex.rs:64-65 with the two closures that exist in the reference, evaluated on the device:
 *   map_kind 0: e > 0 -> e            (cone_psd.rs:69-76)
 *   map_kind 1: e > 0 -> sqrt(e)      (totsu/src/matbuild/mod.rs:231-238)
 * mat: packed upper by columns, length n(n+1)/2, in/out; scale_diag applied as f64lapack.rs:195-255. */
int thip_map_eig(size_t n, float *mat, int has_scale, float scale_diag, float eps_zero,
                 float *work, size_t worklen, int map_kind);
/* arbitrary host closure, two phases (keeps the `M: Fn(F)->Option<F>` contract of linalg_ex.rs:64-65):
 *   1) decompose: eigenvalues -> host_w[n] (SYNC), eigenvectors stay in work;
 *   2) the host applies its closure: host_e[i] = mapped value, host_keep[i] = 1 for Some, 0 for None;
 *   3) rebuild: mat <- sum_i keep_i * e_i z_i z_i^T, diag scaled back, repacked. */
int thip_eig_decompose(size_t n, float *mat, int has_scale, float scale_diag, float eps_zero,
                       float *work, size_t worklen, float *host_w);
int thip_eig_rebuild(size_t n, float *mat, int has_scale, float scale_diag,
                     float *work, size_t worklen, const float *host_e, const uint8_t *host_keep);
/* which engine served the last decomposition of order > 32 on this context (dsyevr / syevdx in the reference,
 * f64lapack.rs:78-108, f32cuda.rs:253-263): *host_engine = 1 host QL + rotation replay, 2 = device multisection + twisted
 * factorisation (certified), 3 = 2 failed its certificate and 1 took over; *host_polish = Newton-Schulz polish steps
 * applied; host_cert[0] = ||Z Z^T - I||_F, host_cert[1] = largest relative residual of the tridiagonal stage,
 * host_cert[2] = how the Householder reduction ran: 1 / 2 one persistent launch (device / one XCD), 0 one launch per reflector, -1 the
 * persistent launch gave up (a bounded spin ran out) and the launches took over.  host_cert holds 3 floats. */
int thip_eig_engine_info(int *host_engine, int *host_polish, float *host_cert);

/* Sparse operators: y = alpha * A x + beta * y, A in CSR (int64 row pointers, int32 column indices,
 * all on the device); abs_mode != 0 uses |A| and x = 1 (MatOp::absadd_*, matop.rs:98-117).  The transposed product
 * is the same call on the CSR of A^T.  Backs a user-level `Operator` (operator.rs:11-156) on the trait-level path. */
int thip_spmv_csr(size_t n_row, size_t n_col, size_t nnz, const int64_t *dev_rowptr, const int32_t *dev_colidx,
                  const float *vals, float alpha, const float *x, float beta, float *y, int abs_mode);

/* A sparse operator held ONCE on the device and serving both products (round 6): built from the caller's HOST arrays in
 * compressed-sparse-column form (int64 column pointers, int32 row indices, f32 values -- what a MatBuild<General> with its zeros
 * dropped holds, matbuild/mod.rs:22-41) into 4096 x 4096 tiles of {value, local row | local column << 16} entries; both A x and
 * A^T y stream the same 8 bytes per entry with 16-byte loads and scatter into LDS accumulators -- no second copy of the values,
 * no global atomics (thip_sptile.hip has the measurements behind the format).  The accumulators are 64-bit fixed-point words fed by
 * integer LDS adds: the sums are bitwise reproducible from run to run.  Rows inside a column may come in any order; where they ascend,
 * a tile of full height whose every column holds all 4096 rows (a dense block of the matrix) is stored WITHOUT its index words -- 4 bytes
 * per entry on the device and per product (thip_sptile_layout reports how many).
 * thip_sptile_mv is `Operator::op / trans_op` (operator.rs:40-75) for such an operator: y = alpha A x + beta y,
 * transpose != 0: A^T; abs_mode != 0: |A| and x = 1 (absadd_rows / absadd_cols, operator.rs:82-154).  x, y on the device.
 * ACCURACY.  Every out element i (a row of A x, a column of A^T x) accumulates in fixed point with a scale OF ITS OWN, taken from
 * amax_i, the largest stored |a| of that row / column, and from max|x|.  With head_bits = ceil(log2(longest row (A x) or column
 * (A^T x))) + 1 and G = 50 - 2 head_bits,
 *         |out_i - (A x)_i|  <=  1e-5 (|A||x|)_i  +  2^-G  amax_i  max|x|        (amax_i no smaller than 2^-127)
 * -- the first term is the f32 rounding of the products and of the partial sums kept in registers, the second the fixed-point
 * rounding: at most 2^(head_bits - 1) adds of half a unit 2^-(50 - head_bits) 2^e_i 2^ex, 2^e_i <= 2 amax_i, 2^ex <= 2 max|x|.
 * A row or column that is small as a whole keeps its bits (its amax_i is small with it); an entry of x far below max|x| -- 2^-(G - 17)
 * of it and less -- contributes with the absolute resolution that max|x| sets.  abs_mode: x = 1, so the bound is relative to amax_i
 * alone and a non-empty row or column never sums to 0.  A non-finite entry of x answers NaN in every element of y.
 * thip_sptile_create returns THIP_E_INVALID for a stored value that is not finite (an integer accumulator cannot carry it) and
 * for n_col > 0 without column pointers (also when nnz == 0: the n_col + 1 pointers are always read).
 * thip_sptile_mv on one handle must not run from two host threads at once (it uses a workspace the handle owns), while any
 * number of solvers may share one handle (thip_solver_set_sptile: each brings its own workspace). */
typedef struct thip_sptile thip_sptile;
int thip_sptile_create(size_t n_row, size_t n_col, size_t nnz, const int64_t *host_colptr, const int32_t *host_rowidx,
                       const float *host_vals, thip_sptile **out);
int thip_sptile_destroy(thip_sptile *mat);
int thip_sptile_mv(thip_sptile *mat, int transpose, float alpha, const float *x, float beta, float *y, int abs_mode);
/* stored entries (tiles padded to whole 16-byte quads), tiles, work items and slices (partial sums per block) of the two
 * products, bytes on the device */
int thip_sptile_info(const thip_sptile *mat, size_t *host_nnz_stored, int *host_tiles, int *host_items_n, int *host_items_t,
                     int *host_slices_n, int *host_slices_t, size_t *host_bytes);
/* how the entries are stored: tiles held without indices (full 4096-row tiles whose every column is full: 4 bytes per entry),
 * entries that carry an index (8 bytes per entry), and the bytes of entries ONE product streams */
int thip_sptile_layout(const thip_sptile *mat, int *host_dense_tiles, size_t *host_indexed_entries, size_t *host_bytes_per_product);

/* The SAME object built on the device from DENSE column-major panels -- what every Prob* builder and MatBuild produce: a dense,
 * mostly-zero array -- in two passes over the panels: count every column once, plan, fill every column once, finish.  The result is
 * the object thip_sptile_create builds from the CSC form of the same matrix with its zeros dropped: same directory, items, exponent
 * codes, indices and values, bit for bit, whatever the panel widths, the panel order or ld.
 *  - dev_panel: columns [c0, c0 + ncols) on the DEVICE, column-major, leading dimension ld >= n_row.  Rows n_row .. ld - 1 of a
 *    panel are never read as data.  Panels may come in any order and any widths from 1 to n_col (no alignment with 4096), and the
 *    two passes may split the columns differently; each pass covers every column exactly once.  A panel may live in one staging
 *    buffer that the caller refills between calls (the calls are ordered on the library's stream).
 *  - an entry is stored iff (bits & 0x7fffffff) != 0: +0.0 and -0.0 are dropped, subnormals are kept, in every denormal mode.
 *  - THIP_E_INVALID, with nothing launched: a column counted or filled twice; a panel outside [0, n_col); ld < n_row; plan with
 *    columns missing; fill before plan; finish with columns unfilled; a null panel with ncols > 0 and n_row > 0.
 *  - a non-finite value sets a device flag in the count pass and plan returns THIP_E_INVALID (the rule of thip_sptile_create).
 *  - a panel whose non-zero pattern differs between the passes never makes the fill write outside that column's counted segment:
 *    every write is bounded by the counted length, a device flag is raised and finish returns THIP_E_INVALID.
 *  - plan reports what thip_sptile_info / _layout will report of the finished object (any pointer may be NULL), so that a caller
 *    can decide before pass 2; it allocates the store.
 *  - finish hands the object over (thip_sptile_destroy frees it); the builder is destroyed separately, at any stage.
 * DEVICE MEMORY during a build: the final store; the count table, one int32 per (column, block of 4096 rows) = n_col x
 * ceil(n_row / 4096) words, 1 / 4096 of the dense bytes; a length and a maximum per row and a maximum per column; the tile
 * directory.  Nothing proportional to n_row x n_col: with the panels streamed through a staging buffer the dense matrix never
 * exists on the device. */
typedef struct thip_sptile_builder thip_sptile_builder;
int thip_sptile_builder_create(size_t n_row, size_t n_col, thip_sptile_builder **out);
int thip_sptile_builder_count(thip_sptile_builder *b, size_t c0, size_t ncols, const float *dev_panel, size_t ld);
int thip_sptile_builder_plan(thip_sptile_builder *b, size_t *host_nnz, int *host_dense_tiles, size_t *host_indexed_entries,
                             size_t *host_bytes_per_product);
int thip_sptile_builder_fill(thip_sptile_builder *b, size_t c0, size_t ncols, const float *dev_panel, size_t ld);
int thip_sptile_builder_finish(thip_sptile_builder *b, thip_sptile **out);
int thip_sptile_builder_destroy(thip_sptile_builder *b);
/* the whole matrix is on the device: count, plan, fill, finish */
int thip_sptile_from_dense(size_t n_row, size_t n_col, const float *dev_mat, size_t ld, thip_sptile **out);

/* ---------------------------------------------------------------------------------------------
 * Device-resident variants used by the fused path (no host round trip).  They replace host loops
 * in totsu_core that a generic backend cannot intercept ("hard parts").
 * ------------------------------------------------------------------------------------------- */
int thip_norm_dev(size_t n, const float *x, float *dev_out);                    /* ||x||_2 -> *dev_out */
int thip_dot_dev(size_t n, const float *x, const float *y, float *dev_out);     /* x.y -> *dev_out */
int thip_abssum_dev(size_t len, const float *x, size_t incx, float *dev_out);

/* MatOp::absadd_impl for General (matop.rs:98-117) in one pass each: tau[c] += sum_r |G(r,c)|,
 * sigma[r] += sum_c |G(r,c)| -- replaces n + m blocking cublasSasum calls */
int thip_absadd_cols(size_t n_row, size_t n_col, const float *mat, float *tau);
int thip_absadd_rows(size_t n_row, size_t n_col, const float *mat, float *sigma);
/* SymPack arm, matop.rs:119-136 */
int thip_absadd_sympack(size_t n, const float *mat, float *y);
/* calc_precond host loops, solver.rs:501-506: x[i] = 1 / max(x[i], eps_zero) */
int thip_recip_max(size_t n, float eps_zero, float *x);

/* Stacking the blocks of a composite operator into ONE column-major matrix on the device (what
 * ProbLPOpA / ProbSOCPOpA / ProbSDPOpA are, lp.rs:76-98, socp.rs:77-130, sdp.rs:75-97, seen as a single MatOp):
 * dst(r, c) = sign * src(r, c) for an n_row x n_col column-major block (lda = n_row), dst pointing at the block's first
 * row inside a matrix of leading dimension ld_dst; transposed != 0: src is an n_col-vector written as ONE row (the
 * -c_i^T rows of socp.rs:88-93). */
int thip_copy_block(int transposed, size_t n_row, size_t n_col, float sign, const float *src, float *dst, size_t ld_dst);

/* Cone projections (totsu_core/src/cone_*.rs) on device-resident vectors */
enum { THIP_CONE_ZERO = 0, THIP_CONE_RPOS = 1, THIP_CONE_SOC = 2, THIP_CONE_ROTSOC = 3, THIP_CONE_PSD = 4 };
int thip_proj_zero(int dual_cone, size_t n, float *x);          /* cone_zero.rs:38-44 */
int thip_proj_rpos(size_t n, float *x);                         /* cone_rpos.rs:38-45 (host loop in the reference) */
int thip_proj_soc(size_t n, float *x);                          /* cone_soc.rs:38-65, one cone */
int thip_proj_rotsoc(size_t n, float *x);                       /* cone_rotsoc.rs:38-65, one cone */
/* many cones in one launch: cone i occupies x[host_offs[i] .. host_offs[i+1]); rotated != 0 -> ConeRotSOC.
 * Replaces the per-cone loop of ProbSOCPCone::proj (totsu/src/problem/socp.rs:296-313). */
int thip_proj_soc_batched(float *x, const int64_t *dev_offs, size_t n_cones, int rotated, size_t max_len);
/* ConePSD::proj, cone_psd.rs:56-79: returns THIP_E_WORK on work shortage (-> Err(())) */
int thip_proj_psd(size_t sn, float *x, float eps_zero, float *work, size_t worklen);
/* the `group` closure of solver.rs:509-520 applied to many blocks at once (product_group) */
int thip_group_min_batched(float *dp_tau, const int64_t *dev_offs, size_t n_groups, size_t max_len);

/* ---------------------------------------------------------------------------------------------
 * Fused conic iteration on the device.  Native restatement of
 * totsu_core/src/solver/solver.rs:340-657 (SolverCore) for operators that are dense matrices:
 * all per-iteration arithmetic, the projections and the termination test run on the GPU; the host
 * only polls a status word.
 * ------------------------------------------------------------------------------------------- */
typedef struct thip_solver thip_solver;

/* Arithmetic of the iterate updates x += T o tx, y += S o ty (solver.rs:542,560) of the fused loop.  Storage and
 * every product stay f32 either way.
 *   THIP_STATE_COMPENSATED: each of the five iterate vectors (x_x, x_y, x_s, u, v) carries a Kahan term, O(n + m)
 *     floats next to an m x n matrix.  Without it the f32 iterate stops moving once an update is below half an ulp of
 *     the entry it is added to, and the dual criterion floors (1.6e-4 on the n = 50 000 SOCP) -- a floor
 *     the reference's own f32 backend shares, which is why it is run at eps_acc = 1e-3 (benchmark_lp/src/main.rs:62-65);
 *   THIP_STATE_PLAIN: x + inc in plain f32, the reference's literal arithmetic. */
enum { THIP_STATE_COMPENSATED = 0, THIP_STATE_PLAIN = 1 };

/* ABI 3 (thip_version): thip_param grew by state_arith + reserved in round 2 (32 -> 40 bytes): callers built against the
 * 32-byte struct must be rebuilt.  Its zero value selects THIP_STATE_COMPENSATED, i.e. the DEFAULT fused loop does not
 * perform the reference's literal f32 iterate additions (solver.rs:542,560); set THIP_STATE_PLAIN for those. */
typedef struct thip_param {           /* solver.rs:13-41 */
    int64_t max_iter;                 /* < 0: None */
    float   eps_acc, eps_inf, eps_zero;
    int64_t log_period;               /* 0: no periodic log */
    int32_t state_arith;              /* THIP_STATE_* (not in the reference; zero-initialised = the default) */
    int32_t reserved;                 /* 0 */
} thip_param;

enum { THIP_ST_RUNNING = -1,
       THIP_ST_OK = 0, THIP_ST_UNBOUNDED = 1, THIP_ST_INFEASIBLE = 2, THIP_ST_EXCESS_ITER = 3,
       THIP_ST_INVALID_OP = 4, THIP_ST_WORK_SHORTAGE = 5, THIP_ST_CONE_FAILURE = 6 };   /* solver_error.rs:3-17 */

enum { THIP_SCHED_REFERENCE = 0,   /* 6 single GEMVs per iteration, the reference's op sequence (solver.rs:122-597) */
       THIP_SCHED_FUSED     = 1,   /* 3 passes over A: N and T products of one stage share a tile read */
       THIP_SCHED_CARRIED   = 2,   /* 2 passes: K*rx obtained by linearity from the criteria products */
       THIP_SCHED_SWEEP     = 3 }; /* 1 pass: per column, both dots, the x_x / u updates and both axpys while the column is in
                                    * registers (thip_sweep.hip; dense f32 A on one GPU, else the carried schedule runs) */

typedef struct thip_problem {
    size_t n, m;                      /* A is m x n (local rows if sharded) */
    const float *mat_a;               /* device, column-major, lda = m */
    const float *vec_b;               /* device, m */
    const float *vec_c;               /* device, n */
    const float *vec_b_rowabs;        /* device, m, or NULL: what op_b.absadd_rows adds per row (default |b|).
                                         ProbSOCPOpB adds scl_d, not |scl_d| (socp.rs:259-279) */
    size_t n_seg;                     /* product cone over consecutive segments of the m rows */
    const int32_t *host_seg_type;     /* THIP_CONE_* */
    const int64_t *host_seg_len;
} thip_problem;

typedef struct thip_status {
    int32_t state;                    /* THIP_ST_* */
    int64_t iter;                     /* index i of the last executed iteration */
    int32_t kind;                     /* 0: pri_dual_gap valid, 1: unbdd_infeas valid */
    float   cri[3];
    float   tau, kappa;
    float   norm_b, norm_c;
} thip_status;

/* collective hook for a row-sharded A: sum-all-reduce `n` floats in place on the
 * given stream.  NULL = single GPU. */
typedef int (*thip_allreduce_fn)(void *ctx, float *dev_buf, size_t n, void *hip_stream);

/* Native RCCL (xGMI) communicator, one per process: rank 0 creates the 128-byte id, the launcher distributes it
 * (e.g. one torch.distributed broadcast), every rank calls thip_comm_init.  thip_solver_use_rccl installs an
 * all-reduce that is enqueued on the library's own stream (no event hand-off to a communication stream). */
int thip_comm_unique_id(uint8_t *host_id128);
int thip_comm_init(int rank, int world, const uint8_t *host_id128);
int thip_comm_allreduce(float *dev_buf, size_t n);       /* in-place float sum over the ranks, on the context stream */
int thip_comm_count(int *host_ranks);                    /* ranks of the live communicator, read back from RCCL (ncclCommCount); 0 = none */
int thip_comm_destroy(void);
int thip_solver_use_rccl(thip_solver *s);                /* before thip_solver_init */

/* One-shot all-reduce over peer-mapped buffers (third transport behind thip_solver_set_allreduce), for the latency-bound
 * messages of the loop (n + 1024 floats: 204 KB at BASELINE configs[2]): every rank publishes its contribution in a slot
 * the peers have mapped (hipIpcGetMemHandle / hipIpcOpenMemHandle), reads its N - 1 peers directly -- one xGMI link
 * each -- and sums in rank order (identical bits on every rank); ONE launch per call, a 4-byte flag handshake per
 * chunk of 2048 floats, no trailing barrier (slots alternate by call parity).  Up to 16 ranks, messages up to 2 MB;
 * works between processes sharing one GPU as well (that is how a 1-GPU box tests it).
 *   every rank: thip_oneshot_init(rank, world, max_floats, handle)    -> its 64-byte IPC handle
 *   the launcher all-gathers the handles (rank order)                  -> thip_oneshot_connect(handles[world * 64])
 *   thip_solver_use_oneshot(s) before thip_solver_init; thip_oneshot_destroy() after a barrier at the end.
 * A rank that waits more than ~4 s for a peer gives up and raises an error word instead of hanging the GPU:
 * thip_oneshot_error (SYNC) reads it.  The collective runs on whatever stream the overlap mode hands it. */
int thip_oneshot_init(int rank, int world, size_t max_floats, uint8_t *host_handle64);
int thip_oneshot_connect(const uint8_t *host_handles);
int thip_oneshot_allreduce(float *dev_buf, size_t n);    /* in-place float sum over the ranks, on the context stream */
int thip_oneshot_error(int *host_err);                   /* SYNC */
int thip_oneshot_destroy(void);
int thip_solver_use_oneshot(thip_solver *s);             /* before thip_solver_init */

int thip_solver_create(const thip_problem *prob, const thip_param *par, int schedule, thip_solver **out);
/* Sparse A for the fused loop (before thip_solver_init; prob->mat_a may then be NULL): CSR of A (m x n) and CSR of
 * A^T (n x m), int64 row pointers / int32 column indices / f32 values, all on the device.  Each stage then costs one
 * gather over A and one over A^T instead of a pass over a dense matrix. */
int thip_solver_set_csr(thip_solver *s, size_t nnz,
                        const int64_t *dev_rowptr, const int32_t *dev_colidx, const float *dev_vals,
                        const int64_t *dev_t_rowptr, const int32_t *dev_t_colidx, const float *dev_t_vals);
/* Sparse A for the fused loop, ONE copy (before thip_solver_init; prob->mat_a may be NULL; `mat` must outlive the solver).
 * Every schedule runs on it; THIP_SCHED_SWEEP is the one-pass recurrence in three launches -- A^T [v x_y], the per-column
 * updates, A [u x_x'] -- 16 bytes per stored entry and iteration (thip_solver_set_csr's two copies under the carried schedule:
 * 32).  Replaces SolverCore's op / trans_op calls on a user's sparse Operator (solver.rs:109-157). */
int thip_solver_set_sptile(thip_solver *s, thip_sptile *mat);
int thip_solver_set_allreduce(thip_solver *s, thip_allreduce_fn fn, void *ctx);
/* Row-sharded runs: where the all-reduce of a stage's A^T y runs relative to the other work (solver.rs:146 vs 149,
 * 122 vs 125 are the independences used).  May be switched between thip_solver_run calls.
 *   THIP_OVERLAP_OFF (0, default)  in order on the launch stream;
 *   THIP_OVERLAP_LOCAL_ROWS (1)    on a side HIP stream of the solver (event in / event out) while the launch stream goes
 *       on with the stage's work on the LOCAL rows (the x_y / x_s update and the cone projections in the x-stage, the v
 *       update in the y-stage); the x_x / u / tau / kappa updates wait for it.  Results are bitwise those of mode 0.
 *       Hides ~10 us of work and costs two launches + two event hand-offs per stage (+27 us at world size 1);
 *   THIP_OVERLAP_COLUMN_PIPELINE (2)  carried schedule, dense A: every stage's products run as two launches over the
 *       column halves [0, n1) and [n1, n) (n1 on a boundary of the GEMV plan's column chunks), and the all-reduce of a
 *       half's A^T y travels on the side stream under the NEXT half-launch, which only needs the entries of the other
 *       half; the sharded block partials ride with the second half; the termination test of iteration k is enqueued
 *       after the first half-launch of iteration k + 1 (which writes scratch only).  Every collective has a whole
 *       half-pass over the local A to complete in.  Costs six more launches per iteration;
 *   THIP_OVERLAP_COLUMN_INORDER (3)   the kernels of mode 2 with the collectives in order on the launch stream: the
 *       bitwise reference of mode 2 (same arithmetic, no concurrency).
 * Modes 2 / 3 fall back to 1 / 0 where the pipeline does not apply (thip_solver_overlap_info tells).  In modes 1 and 2
 * the hook receives the side stream; a hook that ignores its stream argument stays correct (and un-overlapped). */
enum { THIP_OVERLAP_OFF = 0, THIP_OVERLAP_LOCAL_ROWS = 1, THIP_OVERLAP_COLUMN_PIPELINE = 2, THIP_OVERLAP_COLUMN_INORDER = 3 };
int thip_solver_set_overlap(thip_solver *s, int mode);
/* GEMV plan autotune of this solver (thip_solver_init times nine tilings on the actual matrix and keeps the fastest).
 * For a given plan every result is bitwise reproducible run to run; two solves that autotune to different plans agree
 * to f32 round-off only.  on = 0: the shape heuristic, whatever the timings -- bit-reproducible across runs and hosts.
 * Before thip_solver_init (or between runs: takes effect at the next init / storage switch). */
int thip_solver_set_gemv_autotune(thip_solver *s, int on);
/* Leading-dimension padding of the library-owned f32 copy of A (made when m is not a multiple of `floats`, default 16 =
 * 64 bytes, and the copy fits a third of the free HBM): 0 = never copy (stream the caller's matrix as
 * it is).  Before thip_solver_init. */
int thip_solver_set_lda_pad(thip_solver *s, int floats);
/* the mode the next thip_solver_run will actually use, GEMV launches per pass over A (2 when column-split) and the split
 * column n1 (0 = none) */
int thip_solver_overlap_info(thip_solver *s, int *host_mode, int *host_launches_per_pass, size_t *host_split_col);
/* Storage of the dense A the iteration streams: THIP_A_F32 (default: prob->mat_a as given), or THIP_A_BF16 /
 * THIP_A_F16 (a library-owned 16-bit copy, made on the first request; f16 is column-scaled and rounds 8x finer than
 * bf16: half the bytes per pass, the problem solved is the one with the ROUNDED matrix).  Before thip_solver_init the preconditioners are computed from the stored form; between
 * thip_solver_run calls it switches the operator of the running iteration (e.g. bf16 passes first, f32 passes to
 * finish on the exact matrix) -- the iteration is a fixed-point method, so the iterate carries over.
 * prob->mat_a must stay valid while THIP_A_F32 may still be selected. */
int thip_solver_set_a_storage(thip_solver *s, int a_kind);
/* A caller-built bf16 matrix (thip_to_bf16 on column blocks, or any producer of bf16 bit patterns), column-major with
 * leading dimension ld16 >= m; before thip_solver_init; prob->mat_a may then be NULL (and THIP_A_F32 cannot be
 * selected).  The f32 matrix never has to exist as a whole: a 16-bit A is half the HBM footprint, e.g. BASELINE.json's
 * 320 GB LP (configs[4]) is 160 GB and fits one 288 GB MI355X.  The matrix stays caller-owned. */
int thip_solver_set_a_bf16(thip_solver *s, const uint16_t *mat16, size_t ld16);
/* the same for a caller-built f16 matrix with its per-column inverse scales (thip_to_f16) */
int thip_solver_set_a_f16(thip_solver *s, const uint16_t *mat16, size_t ld16, const float *inv_scale);
int thip_solver_init(thip_solver *s);                                 /* calc_norms + init_vecs + calc_precond, solver.rs:460-524 */
/* enqueue up to max_steps iterations (the device stops by itself on termination), poll every
 * `poll_every` iterations; returns when terminated or after max_steps.  SYNC. */
int thip_solver_run(thip_solver *s, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_solver_status(thip_solver *s, thip_status *host_status);     /* SYNC */
/* Continue a solve that ended THIP_ST_OK / THIP_ST_EXCESS_ITER (criteria kind 0): undoes the final 1/tau scaling of
 * solver.rs:397-400 and clears the termination, so that thip_solver_run goes on from the same iterate -- after
 * thip_solver_set_a_storage (finish on the exact matrix) or thip_solver_set_param (a tighter eps_acc, a larger
 * max_iter).  A no-op on a running solve. */
int thip_solver_resume(thip_solver *s);
int thip_solver_set_param(thip_solver *s, const thip_param *par);
/* solver.rs:317-320: x = work[0..n], y = work[n..n+m] */
int thip_solver_solution(thip_solver *s, float *host_x, float *host_y);
/* raw iterate (x: n+2m+1, y: n+m+1, reference layout solver.rs:349-355), for parity tests */
int thip_solver_iterate(thip_solver *s, float *host_x, float *host_y);
/* After thip_solver_init: the solver goes on from the iterate (host_x, host_y) -- the layouts of thip_solver_iterate, of a RUNNING
 * solver (a terminated one's x_x, x_y come back divided by tau) -- instead of x = 0, y = 0, tau = 1.  Uploads x_x, x_y, x_s, u, v, zeroes
 * the Kahan terms, writes tau and kappa and resets the status block (iteration 0, RUNNING; norms and preconditioner stay); the
 * carried schedules' A x_x, A^T x_y are recomputed by one pass over the stored form of A now in use, the one-pass schedule restarts
 * from the iterate as a consistent one.  Any A: dense in any stored form, the two-CSR form, the tiled sparse copy.  Synchronous.
 * THIP_E_INVALID: a null argument, a solver not initialised, an all-reduce or a column shard set (multi-GPU starts are not offered), a
 * tau that is negative or not finite, a kappa that is positive or not finite. */
int thip_solver_set_iterate(thip_solver *s, const float *host_x, const float *host_y);
int thip_solver_precond(thip_solver *s, float *host_dp_tau, float *host_dp_sigma);
int thip_solver_destroy(thip_solver *s);
/* physical passes over A per iteration of the schedule in use, and bytes one pass reads */
int thip_solver_passes(const thip_solver *s, int *host_passes, size_t *host_bytes_per_pass);
/* the schedule the next thip_solver_run will execute: the one given to thip_solver_create, or THIP_SCHED_CARRIED when
 * THIP_SCHED_SWEEP was asked for and the one-pass kernel cannot take this problem (sharded rows, sparse or 16-bit A,
 * m or lda not a multiple of 4, fewer than 40 column panels per group, a device that is not 8 XCDs x 32 CUs, a failed
 * placement census) */
int thip_solver_schedule_in_use(thip_solver *s, int *host_schedule);
/* THIP_SCHED_SWEEP is considered for matrices of at least this many bytes (default 128 MiB); above it thip_solver_init
 * times the kernel's geometries on the matrix and keeps the carried schedule if none beats an estimate of its two passes
 * (measured on square-ish SOCPs: the carried schedule stays at 190 MB, the sweep is 1.37x faster at 274 MB, 1.58x at
 * 512 MB, 1.7x at 2 GB, 2.0x at 20 GB; a 1 200 x 100 000 matrix keeps the carried schedule, 100 000 x 1 200 gains 1.53x);
 * 0 = whenever the kernel can take the shape, unconditionally.  Before thip_solver_init. */
int thip_solver_set_sweep_min_bytes(thip_solver *s, size_t bytes);
/* the geometry of the one-pass kernel chosen for this solver (thip_solver_init times the candidates on the actual matrix
 * unless thip_solver_set_gemv_autotune(s, 0)): workgroups per column group, columns per panel, 16-byte slots per thread,
 * and its measured time per sweep in ms (0 = not timed); all 0 when the one-pass schedule is not in use */
int thip_solver_sweep_plan(thip_solver *s, int *host_members, int *host_cols_per_panel, int *host_slots, float *host_ms);
/* N > 1 with THIP_SCHED_SWEEP: the problem given to thip_solver_create is this rank's block of COLUMNS -- mat_a is
 * m x n_local (all m rows), vec_c its n_local entries, vec_b and the cone segments the whole problem's -- the n-vectors are
 * sharded, the m-vectors replicated and updated redundantly, and the hook of thip_solver_set_allreduce is called ONCE per
 * iteration on 2 * roundup(m, 64) + 2048 floats (the two N products and the block partials of the sums over n; one call
 * more in thip_solver_init).  Every rank must get bitwise the same sums back (RCCL, the one-shot transport and a host sum
 * all do).  thip_solver_solution / _iterate return this rank's block of x and the whole y.  Before thip_solver_init. */
int thip_solver_set_column_shard(thip_solver *s, int on);
/* Can the one-pass kernel run on this device for an m x n_local block (geometry + one placement census, no collective)?
 * A multi-rank host asks every rank and takes the minimum BEFORE building column-sharded solvers: a rank that found out
 * inside thip_solver_init would leave the others waiting in their first all-reduce.  elem = the stored form of A the run
 * will stream (THIP_A_F32 / THIP_A_BF16 / THIP_A_F16: a 16-bit plan has eight rows per slot and caps of its own).
 * A rank whose plan still fails later (a re-plan inside thip_solver_run after thip_solver_set_a_storage /
 * _set_sweep_min_bytes) takes part in the peers' collectives with its fault flag raised: every rank of the run returns
 * THIP_E_TIMEOUT at the same batch. */
int thip_sweep_probe(size_t m, size_t n_local, size_t lda, int elem, int *host_ok);

/* ---------------------------------------------------------------------------------------------
 * A batch of problems that share A: B instances with their own b_i, c_i over ONE dense f32 matrix and one cone layout (a
 * regularisation path, a parameter sweep, a set of scenarios: what the reference serves by handing op_c / op_a / op_b to every
 * Solver::solve call, solver.rs:285-321), iterated in lockstep under the 2-pass carried schedule.  One multi-vector launch
 * (thip_gemv_multi.hip) forms the products of up to eight instances from ONE read of A, so an iteration of the batch costs
 * 2 * ceil(B / 8) passes over A instead of 2 B.  Everything after the products is the ordinary solver's own kernels on the
 * instance's own state: the instances do not interact, each one stops by its own termination test and is then frozen (iterate
 * and iteration count) while the others go on; a group whose members have all stopped is no longer launched.
 * Limits: dense f32 A on one GPU (no sparse, 16-bit or sharded A, no one-pass schedule), 1 .. THIP_BATCH_MAX instances.
 * A is held once: the caller's array and, when m is no multiple of 16 floats, one library-owned padded copy for all instances.
 * ------------------------------------------------------------------------------------------- */
typedef struct thip_batch thip_batch;
#define THIP_BATCH_MAX 64
#define THIP_BATCH_GROUP_DEFAULT 8    /* instances per multi-vector launch (thip_batch_set_max_group) */
typedef struct thip_batch_info_t {
    int32_t n_inst, max_group;        /* instances; instances per launch */
    int32_t groups;                   /* launches per pass: ceil(n_inst / max_group) */
    int32_t passes_per_iteration;     /* 2 * groups */
    int32_t a_copies;                 /* library-owned copies of A held by the batch: 0, or 1 (the padded copy) */
    int32_t reserved;
    size_t  a_bytes;                  /* bytes of that copy */
    size_t  bytes_per_pass;           /* 4 m n */
    size_t  arena_bytes;              /* the instances' state vectors, summed */
    size_t  device_bytes;             /* everything the batch holds on the device (copy of A, arenas, GEMV scratch, tables) */
    int32_t plan_nj[4], plan_blocks[4];   /* tuned tiling of the multi-vector kernel by instance, [1] NV = 2, [2] NV = 4, [3] NV = 8 */
    float   plan_ms[4];               /* (0 = the shape heuristic) and its measured ms per launch + second stage */
} thip_batch_info_t;
/* prob_template: n, m, mat_a, the cone segments and (optionally) vec_b_rowabs shared by all instances; its vec_b / vec_c are not
 * read.  host_vec_b / host_vec_c: HOST arrays of n_inst DEVICE pointers (m / n floats each), caller-owned like mat_a.
 * THIP_E_INVALID: n_inst < 1 or > THIP_BATCH_MAX, a null array or entry, no dense mat_a (a sparse operator cannot be batched),
 * a mat_a that is not 16-byte aligned, bad cone segments. */
int thip_batch_create(const thip_problem *prob_template, int n_inst, const float *const *host_vec_b,
                      const float *const *host_vec_c, const thip_param *par, thip_batch **out);
/* the stored form of A: THIP_A_F32 is the only one a batch takes (THIP_E_INVALID for the 16-bit kinds) */
int thip_batch_set_a_storage(thip_batch *b, int a_kind);
/* the autotune of the GEMV tilings (the multi-vector kernel's per group size in use, on the actual matrix; a group of one uses
 * the instance's own single-vector plan): on = 0 pins the shape heuristic -- bit-reproducible.  Before thip_batch_init. */
int thip_batch_set_gemv_autotune(thip_batch *b, int on);
/* instances per multi-vector launch: 2, 4 or 8 (default THIP_BATCH_GROUP_DEFAULT).  Before thip_batch_init. */
int thip_batch_set_max_group(thip_batch *b, int max_group);
int thip_batch_set_param(thip_batch *b, const thip_param *par);      /* thip_solver_set_param on every instance */
/* every instance's norms, init_vecs and preconditioner (the |A| row and column sums once for all), the carried products primed */
int thip_batch_init(thip_batch *b);
/* every RUNNING instance advances by up to max_steps iterations (< 0: until all have stopped), poll_every iterations enqueued
 * back to back between looks at the status records; host_status: n_inst records or NULL.  SYNC. */
int thip_batch_run(thip_batch *b, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_batch_status(thip_batch *b, int i, thip_status *host_status);                       /* SYNC; thip_solver_status of instance i */
int thip_batch_solution(thip_batch *b, int i, float *host_x, float *host_y);                 /* thip_solver_solution of instance i */
int thip_batch_iterate(thip_batch *b, int i, float *host_x, float *host_y);                  /* thip_solver_iterate of instance i */
int thip_batch_precond(thip_batch *b, int i, float *host_dp_tau, float *host_dp_sigma);      /* thip_solver_precond of instance i */
int thip_batch_info(const thip_batch *b, thip_batch_info_t *host_info);
/* how n_inst instances are grouped into launches of at most max_group: *host_groups, and the members of each (host_members:
 * up to THIP_BATCH_MAX ints or NULL).  Needs no device. */
int thip_batch_grouping(int n_inst, int max_group, int *host_groups, int *host_members);
int thip_batch_destroy(thip_batch *b);

/* ---- a batch as a set of SLOTS that problems stream through, and launches that follow the live set (both opt-in: without
 * these calls a batch behaves as described above, bit for bit) ----
 *
 * thip_batch_replace: after thip_batch_init.  Slot i -- running or stopped, for whatever reason -- is pointed at the new
 * caller-owned device vectors (m / n floats) and becomes exactly what thip_batch_init would have made of an instance created with
 * them: norms of b and c, x = 0, y = 0, tau = 1, the preconditioner and group minima from the batch's shared |A| sums (no pass
 * over A), Kahan terms zero, the (zero) carried products of the start iterate, iteration count 0, state RUNNING.  No other
 * instance is touched.  The launches go into the stream in order; the call reads the retired occupant's status first (a
 * synchronise), so the old b / c are no longer read once it has returned: the caller may free them AFTER the call returns, not
 * before.  THIP_E_INVALID: a null argument, no such slot, a batch that is not initialised. */
int thip_batch_replace(thip_batch *b, int i, const float *dev_vec_b, const float *dev_vec_c);
/* thip_solver_set_iterate of slot i, after thip_batch_init or thip_batch_replace; the slot is live again.  Its carried products cost
 * one single-vector pass over A for that slot.  The iterations the slot had made stay in thip_batch_counters' instance_iterations, as a
 * replaced occupant's do. */
int thip_batch_set_iterate(thip_batch *b, int i, const float *host_x, const float *host_y);
/* on = 1: at every poll the instances the host saw RUNNING are packed in ascending index order into groups of at most max_group
 * (thip_batch_live_grouping), so a pass costs ceil(live / max_group) launches; a group of k runs on the kernel instance of k
 * vectors, a group of one on the single-vector kernel.  thip_batch_init then tunes every kernel instance the batch can come to
 * use (NV = 2, 4, 8 up to max_group and the single-vector plan, once, shared by all instances); thip_batch_run tunes nothing.
 * on = 0 (default): the groups fixed by index at init.  Before thip_batch_init (THIP_E_INVALID after it). */
int thip_batch_set_regroup(thip_batch *b, int on);
/* thip_batch_run that returns at the first poll which finds stopped an instance that was RUNNING when the call began (and, like
 * it, when nothing is running or after max_steps iterations).  SYNC. */
int thip_batch_run_until_any(thip_batch *b, int64_t max_steps, int64_t poll_every, thip_status *host_status);
/* the regroup rule: host_live[n_inst] (non-zero = running) -> *host_groups launches per pass, their sizes (host_group_sizes: up
 * to THIP_BATCH_MAX ints or NULL; full groups first, the rest last) and the live instance indices in launch order (host_members:
 * up to THIP_BATCH_MAX ints or NULL).  Needs no device. */
int thip_batch_live_grouping(int n_inst, int max_group, const int *host_live, int *host_groups, int *host_group_sizes,
                             int *host_members);
/* what thip_batch_run / thip_batch_run_until_any have issued since thip_batch_init (which zeroes the counters) */
typedef struct thip_batch_counters_t {
    int64_t launches[4];              /* product launches by kernel instance: [0] single-vector, [1] NV = 2, [2] NV = 4, [3] NV = 8 */
    int64_t passes;                   /* their sum: passes over A */
    int64_t instance_iterations;      /* iterations completed, summed over the slots (a retired occupant's count is added when its
                                         slot is replaced) */
    int64_t replaced;                 /* thip_batch_replace calls */
    int32_t live, groups_now;         /* as of the last poll: instances RUNNING, launches per pass */
} thip_batch_counters_t;
int thip_batch_counters(const thip_batch *b, thip_batch_counters_t *host);

/* ---------------------------------------------------------------------------------------------
 * Many SMALL problems, each with its own A, iterated on chip (thip_smallbatch.hip).
 * n_prob problems share n, m and the cone layout and differ in A, b, c (and vec_b_rowabs): problem p's data is at
 * dev_mats_a + p m n (column-major, lda = m), dev_vecs_b + p m, dev_vecs_c + p n, dev_vecs_b_rowabs + p m (or NULL: |b|); the
 * arrays stay the caller's and must outlive the object.  One launch gives ONE workgroup to each problem still running: it holds
 * the problem's A in the LDS of its CU and runs min(poll_every, steps left) whole iterations of the reference's loop -- both
 * products, the updates, the cone projections, the termination test -- with no launch boundary inside; the host then reads
 * every status block in one transfer and launches again over the problems still RUNNING.  A problem's iterates depend on its own
 * data and the workgroup size alone: not on its index, its neighbours, or how the iterations were cut into launches.
 * Accepted (else THIP_E_INVALID): 1 <= m <= 1024, 1 <= n <= 1024, m n <= 24576, segments of the zero, nonnegative, second-order
 * and rotated second-order cones that cover m (no PSD segment), 1 <= n_prob <= 1048576.  Both THIP_STATE_* arithmetics.
 * status / solution / iterate / precond of problem i mean what thip_solver_* mean (the final 1/tau scaling is applied to what
 * solution and iterate return once the problem has terminated).
 * ------------------------------------------------------------------------------------------- */
typedef struct thip_smallbatch thip_smallbatch;
typedef struct thip_smallbatch_info_t {
    int32_t n_prob, threads;          /* problems; threads per workgroup (64, 256 or 1024, by shape) */
    int32_t lds_bytes, live;          /* LDS of one workgroup; problems RUNNING as of the last poll */
    size_t  arena_bytes;              /* the problems' state (iterates, Kahan terms, preconditioner) */
    size_t  device_bytes;             /* everything this object allocated on the device */
    size_t  device_bytes_all;         /* the same, summed over every thip_smallbatch alive in the process */
    int64_t launches, workgroups;     /* issued by run / run_until_any since thip_smallbatch_init */
} thip_smallbatch_info_t;
/* the shape rules alone (needs no device): 0 and the LDS bytes / threads of one workgroup, or THIP_E_INVALID */
int thip_smallbatch_fits(size_t n, size_t m, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                         size_t *host_lds_bytes, int *host_threads);
int thip_smallbatch_create(size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b,
                           const float *dev_vecs_c, const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type,
                           const int64_t *host_seg_len, const thip_param *par, thip_smallbatch **out);
int thip_smallbatch_set_param(thip_smallbatch *h, const thip_param *par);
/* norms, preconditioner and the zero start iterate of every problem, on chip (one launch) */
int thip_smallbatch_init(thip_smallbatch *h);
/* every RUNNING problem advances by up to max_steps iterations (< 0: until all have stopped); host_status: n_prob entries or NULL */
int thip_smallbatch_run(thip_smallbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
/* the same, back at the first poll that finds stopped a problem that was RUNNING when the call began */
int thip_smallbatch_run_until_any(thip_smallbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_smallbatch_status(thip_smallbatch *h, int i, thip_status *host_status);
int thip_smallbatch_solution(thip_smallbatch *h, int i, float *host_x, float *host_y);
int thip_smallbatch_iterate(thip_smallbatch *h, int i, float *host_x, float *host_y);
int thip_smallbatch_precond(thip_smallbatch *h, int i, float *host_dp_tau, float *host_dp_sigma);
/* slot i -- running or stopped -- takes new data (one problem each; dev_vec_b_rowabs may be NULL) and is initialised afresh;
 * no other slot is touched */
int thip_smallbatch_replace(thip_smallbatch *h, int i, const float *dev_mat_a, const float *dev_vec_b, const float *dev_vec_c,
                            const float *dev_vec_b_rowabs);
/* problems first .. first + count - 1 start from the given iterates instead of x = 0, y = 0, tau = 1: after thip_smallbatch_init or
 * _replace, whose norms and preconditioner stay.  host_x: the problems' x one after another, n + 2 m + 1 floats each (x_x, x_y, x_s,
 * tau); host_y: n + m + 1 each (u, v, kappa) -- the layout thip_smallbatch_iterate writes (of a RUNNING problem: a stopped one's
 * x_x, x_y come back divided by tau).  The Kahan terms, r_tau and the criteria are zero, the iteration count 0, the problems RUNNING
 * again; the streamed families form the carried pair A x_x, A^T x_y of the iterate.  One upload and one launch (one per workgroup-
 * size class where the problems have their own shapes, every length then the problem's own); synchronous.  The iterates are packed into pinned host
 * memory and uploaded to a staging buffer, both the handle's, grown to the largest call and freed by _destroy; the device one is counted
 * in device_bytes.  THIP_E_INVALID: a null
 * argument, a handle not initialised, a range outside the batch, count < 1, a tau that is negative or not finite, a kappa that is
 * positive or not finite; every other entry is the caller's, as A, b and c are.  The same under every thip_*batch prefix */
int thip_smallbatch_set_iterates(thip_smallbatch *h, int first, int count, const float *host_x, const float *host_y);
/* problems first .. first + count - 1 take a new b and c (and the row sums that go with b) and KEEP their A, which stays where it is on
 * the device: no pass of A through the host or the bus, one upload, one launch (one per workgroup-size class where the problems have
 * their own shapes) and one read of the range's status blocks for all of them; synchronous.  host_b: the problems' b one after
 * another, m floats each (every length the problem's own); host_c: n each.  host_b_rowabs: m floats for every problem of the range,
 * or NULL: no problem has row sums (|b| is used, as where _create was given none).  host_has_rowabs: one byte per problem, 0: the
 * problem's part of host_b_rowabs is ignored (|b|), or NULL: all of them count.
 * keep_iterate == 0: each problem ends exactly as thip_smallbatch_replace(i, its present A, b, c, rowabs) leaves it, bit for bit --
 * preconditioner, norms, the zero iterate, iteration 0, RUNNING.  keep_iterate != 0: the preconditioner and the norms of the new
 * data, and the iterate as it lies in the arena kept -- x_x, x_y, x_s, tau | u, v, kappa without the read-out's scaling -- with
 * the Kahan terms, r_tau and the criteria zero, iteration 0, RUNNING again whether it was running or had stopped (a tau of 0
 * included): what _replace followed by _set_iterates on the problem's own raw iterate gives, without either upload.  The streamed
 * families keep the carried pair A x_x, A^T x_y, which depends on neither b nor c.
 * The first call that is taken allocates the handle's own store of b, c and row sums for the whole batch (2 m + n floats per problem,
 * counted in device_bytes, freed by _destroy); the kernel copies each problem's part there and points the slot's b, c and row sums
 * at it -- the slot's A pointer is not touched -- and a later _replace points the slot back at the caller's arrays.  The data is
 * packed into the staging buffers of _set_iterates.  THIP_E_INVALID, before anything is allocated, uploaded or changed: a null
 * handle, a handle not initialised, a range outside the batch, count < 1, a null host_b or host_c.  Values are not examined, as
 * _replace examines none.  The same under every thip_*batch prefix */
int thip_smallbatch_set_bc(thip_smallbatch *h, int first, int count, const float *host_b, const float *host_c,
                           const float *host_b_rowabs, const uint8_t *host_has_rowabs, int keep_iterate);
/* thip_smallbatch_solution of the problems first .. first + count - 1 in one read-out: a kernel gathers their x_x and x_y from the arena
 * into the staging buffer, one copy brings that down and one the range's status blocks, and the host applies the final 1/tau scaling
 * to each problem's part as _solution does -- the same bits.  host_x: n floats per problem, one after another (every length the
 * problem's own); host_y: m each; either may be NULL, and with both NULL only the statuses are read.  host_status: count entries or
 * NULL.  THIP_E_INVALID: a null handle, a handle not initialised, a range outside the batch, count < 1.  The same under every
 * thip_*batch prefix */
int thip_smallbatch_solutions(thip_smallbatch *h, int first, int count, float *host_x, float *host_y, thip_status *host_status);
/* problems first .. first + count - 1 take NEW VALUES of A and keep their shape, cone layout, b, c and row sums (and, a sparse
 * family, their pattern): a round of a successive linearisation, a time-varying model, a re-weighted relaxation in one call and
 * one launch (one per workgroup-size class where the problems have their own shapes); synchronous.  host_values: the problems'
 * values one after another.  A dense family (smallbatch, midbatch, sdpbatch, raggedbatch): the problem's own m n floats,
 * column-major, as _create and _replace take them.  A sparse family (sparsebatch, raggedsparse): the values in the CSC order of the
 * slot's PRESENT pattern, as many as the slot holds now -- the host_values a (colptr, rowidx, values) triple of that pattern would
 * carry; explicit zeros stay entries.  host_counts: count entries, how many values each problem brings, or NULL: exactly what it
 * needs; a count that differs from m n (dense) or from the slot's present entry count (sparse) is refused -- another pattern is
 * _replace's.
 * WHERE THE VALUES GO.  Dense: into the memory the slot's A pointer points at, OVERWRITTEN IN PLACE -- the buffer handed to _create
 * or _replace is written by _set_a; the host copies straight to the slots' addresses, one copy per run of slots that lie one behind
 * the other (a batch as created is one run); no second store of A is made, device_bytes does not grow and the alignment, so the
 * 16-byte or 4-byte load path, is what it was.  Sparse: one upload of 4 bytes per entry into the staging buffers of _set_iterates,
 * and a kernel writes both stored orders of each blob on the device (a launch of its own ahead of the next).
 * keep_iterate == 0: each problem ends exactly as _replace(i, the new A, its present b, c, rowabs) leaves it, bit for bit.
 * keep_iterate != 0: the preconditioner and the norms of the new data; x_x, x_y, x_s, tau | u, v, kappa stay as they lie in the
 * arena, the Kahan terms, r_tau and the criteria are zero, iteration 0, RUNNING again whether the problem was running or had
 * stopped; the streamed families form the carried pair A x_x, A^T x_y again from the new A.  For a running problem that is
 * _replace(i, new A, ..) followed by _set_iterates on its own iterate, bit for bit.  b, c and the row sums are read where the slot
 * points now -- the caller's arrays, or the handle's store after a _set_bc -- and never moved; _set_a(keep) followed by
 * _set_bc(keep) is a round that moves all three.
 * THIP_E_INVALID, before anything is uploaded or touched (every problem's readable state is unchanged): a null handle, a handle not
 * initialised, a range outside the batch, count < 1, null values, a wrong count (the message names the problem), a value that is
 * not finite.  Not done: values taken from device memory, a change of pattern (_replace).  The same under every thip_*batch
 * prefix and thip_raggedsparse */
int thip_smallbatch_set_a(thip_smallbatch *h, int first, int count, const float *host_values, const int64_t *host_counts,
                          int keep_iterate);
/* THE ROUND CALLS ON DEVICE MEMORY: _set_bc, _set_a, _set_iterates and _solutions for a caller whose round is produced, and whose
 * answers are used, on the GPU.  Every dev_* argument is float32 device memory, packed problem after problem for the range first ..
 * first + count - 1, each problem in its own lengths: the layouts the host calls take.  Each call is DEFINED by the host call it
 * mirrors: handed the same floats, _set_bc_dev, _set_a_dev and _set_iterates_dev leave the range -- arena, preconditioner, carried
 * pair, status blocks, slots, the handle's b / c store, the live list -- as the host call leaves it, bit for bit, for both values of
 * keep_iterate, for running and stopped problems; _solutions_dev writes what _solutions returns, bit for bit.
 * _set_bc_dev: dev_b_rowabs may be NULL; host_has_rowabs (HOST memory, one byte per problem) may be NULL; b and c are not examined.
 * A kernel builds the staged form of the host call in the handle's staging buffer and the set_bc kernels run on it unchanged.
 * _set_a_dev, a dense family: dev_values != NULL: the values are copied device to device, by one kernel launch for the whole range
 * whatever allocations the slots lie in, into the memory each slot's A pointer points at (in place, nothing is allocated).
 * dev_values == NULL: the caller has ALREADY rewritten A where the slots read it (the buffer handed to _create or _replace): nothing
 * is copied, the handle only initialises again from what lies there -- the zero-copy form.  A dev_values that overlaps the A of a
 * slot of the range is THIP_E_INVALID: the exact in-place form is written with NULL.  A sparse family: dev_values holds 4 bytes per
 * stored entry in the CSC order of each slot's present pattern; the scatter kernel reads them where they lie, by a table of the
 * host's record of the slots' counts, which is all that goes up; NULL is refused.  The tables of every call (a few dozen bytes per
 * problem) and the verdict words lie in pinned host memory mapped for the device, so a dense _set_a_dev allocates no device memory.
 * _set_iterates_dev: dev_x, dev_y as _set_iterates' host_x, host_y; a kernel copies them into the staged layout and the start
 * kernels run on it unchanged.
 * _solutions_dev: dev_x (n floats per problem), dev_y (m each), dev_state (one int32 per problem: its THIP_ST_* state); each may
 * be NULL.  The final scaling is applied on the device -- rt = 1 / tau correctly rounded, then rt * v, when kind == 0 and the state
 * is OK or ExcessIter, else the floats as they lie.  It DOES NOT SYNCHRONISE: it returns after the launch on the library's stream
 * and copies nothing to the host (a batch of many shapes uploads one table with its first call, counted in device_bytes).
 * REFUSALS, all THIP_E_INVALID with the batch bit-identical to the one before the call: a null handle, a handle not initialised,
 * a range outside the batch, count < 1, a null array where one is needed, an array that is not 4-byte aligned; any input or output
 * range that overlaps memory the handle owns (its arena, its staging buffers, its b / c store, a sparse family's blobs); and what
 * the host calls find by scanning: a check kernel -- one launch, one verdict word per problem, written into pinned host memory and
 * read by the host behind a synchronisation BEFORE any copy, scatter or set kernel is launched -- looks for a value of A that is not finite (the in-place form: in the slots'
 * own A) and for a start's tau that is negative or not finite or kappa that is positive or not finite; the message names the first
 * problem at fault.
 * STREAM: everything is enqueued on the library's stream (thip_get_stream / thip_set_stream).  A caller that produces the data on
 * another stream orders that work before the call (an event the library's stream waits for, or a synchronisation); the three
 * _set_*_dev calls end with the read of the range's status blocks and so synchronise, as their host twins do.
 * Not done: pinned-host inputs, asynchronous _set_* calls, BatchSolver (shared A).  The same under every thip_*batch prefix and
 * thip_raggedsparse */
int thip_smallbatch_set_bc_dev(thip_smallbatch *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_b_rowabs,
    const uint8_t *host_has_rowabs, int keep_iterate);
int thip_smallbatch_set_a_dev(thip_smallbatch *h, int first, int count, const float *dev_values, int keep_iterate);
int thip_smallbatch_set_iterates_dev(thip_smallbatch *h, int first, int count, const float *dev_x, const float *dev_y);
int thip_smallbatch_solutions_dev(thip_smallbatch *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state);
int thip_smallbatch_info(const thip_smallbatch *h, thip_smallbatch_info_t *host_info);
int thip_smallbatch_destroy(thip_smallbatch *h);

/* ---------------------------------------------------------------------------------------------
 * Many MID-SIZE problems, each with its own A, too big for LDS: A streamed per workgroup (thip_midbatch.hip).
 * The interface is thip_smallbatch's, one for one: the same arrays (problem p's A at dev_mats_a + p m n, column-major, lda = m,
 * read in place and never written), the same slots, polls, status / solution / iterate / precond and replace.  One launch gives
 * ONE workgroup to each problem still running: it holds every vector of the iteration in the LDS of its CU, reads A twice per
 * iteration from memory (the carried recurrence) and runs min(poll_every, steps left) whole iterations.
 * Accepted: 1 <= m, n <= 4096 whose vectors fit LDS -- 4 (6208 + 8 n + 13 m) + roundup4(m) <= 163 840 bytes, which holds for every
 * 8 n + 13 m <= 32 768 --, zero / nonnegative / second-order / rotated second-order segments that cover m, 1 <= n_prob <= 1 048 576.
 * Everything else is THIP_E_INVALID before anything is allocated.  A problem's iterates do not depend on its index, its
 * neighbours or how the iterations are cut into launches.
 * ------------------------------------------------------------------------------------------- */
typedef struct thip_midbatch thip_midbatch;
typedef struct thip_midbatch_info_t {
    int32_t n_prob, threads;          /* problems; threads per workgroup (256 or 1024, by shape) */
    int32_t lds_bytes, live;          /* LDS of one workgroup; problems RUNNING as of the last poll */
    size_t  arena_bytes;              /* the problems' state (iterates, Kahan terms, preconditioner, the carried products) */
    size_t  device_bytes;             /* everything this object allocated on the device */
    size_t  device_bytes_all;         /* the same, summed over every thip_midbatch alive in the process */
    int64_t launches, workgroups;     /* issued by run / run_until_any since thip_midbatch_init */
    int32_t load_bytes, reserved;     /* 16: every problem's A is read with 16-byte loads (m % 4 == 0, bases aligned); else 4 */
    size_t  a_bytes_per_iter;         /* bytes of A read per problem-iteration: 2 m n 4 */
} thip_midbatch_info_t;
/* the shape rules alone (needs no device): 0 and the LDS bytes / threads of one workgroup, or THIP_E_INVALID */
int thip_midbatch_fits(size_t n, size_t m, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                       size_t *host_lds_bytes, int *host_threads);
int thip_midbatch_create(size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b,
                         const float *dev_vecs_c, const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type,
                         const int64_t *host_seg_len, const thip_param *par, thip_midbatch **out);
int thip_midbatch_set_param(thip_midbatch *h, const thip_param *par);
int thip_midbatch_init(thip_midbatch *h);
int thip_midbatch_run(thip_midbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_midbatch_run_until_any(thip_midbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_midbatch_status(thip_midbatch *h, int i, thip_status *host_status);
int thip_midbatch_solution(thip_midbatch *h, int i, float *host_x, float *host_y);
int thip_midbatch_iterate(thip_midbatch *h, int i, float *host_x, float *host_y);
int thip_midbatch_precond(thip_midbatch *h, int i, float *host_dp_tau, float *host_dp_sigma);
int thip_midbatch_replace(thip_midbatch *h, int i, const float *dev_mat_a, const float *dev_vec_b, const float *dev_vec_c,
                          const float *dev_vec_b_rowabs);
int thip_midbatch_set_iterates(thip_midbatch *h, int first, int count, const float *host_x, const float *host_y);
int thip_midbatch_set_bc(thip_midbatch *h, int first, int count, const float *host_b, const float *host_c,
                         const float *host_b_rowabs, const uint8_t *host_has_rowabs, int keep_iterate);
int thip_midbatch_solutions(thip_midbatch *h, int first, int count, float *host_x, float *host_y, thip_status *host_status);
int thip_midbatch_set_a(thip_midbatch *h, int first, int count, const float *host_values, const int64_t *host_counts, int keep_iterate);
int thip_midbatch_set_bc_dev(thip_midbatch *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_b_rowabs,
    const uint8_t *host_has_rowabs, int keep_iterate);
int thip_midbatch_set_a_dev(thip_midbatch *h, int first, int count, const float *dev_values, int keep_iterate);
int thip_midbatch_set_iterates_dev(thip_midbatch *h, int first, int count, const float *dev_x, const float *dev_y);
int thip_midbatch_solutions_dev(thip_midbatch *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state);
int thip_midbatch_info(const thip_midbatch *h, thip_midbatch_info_t *host_info);
int thip_midbatch_destroy(thip_midbatch *h);

/* ---------------------------------------------------------------------------------------------
 * The mid batch over a LIBRARY-OWNED 16-BIT COPY of every problem's A (thip_mid16batch.hip): thip_midbatch's shapes
 * (thip_mid16batch_fits is thip_midbatch_fits), cones, iteration and interface, half the bytes of A per pass and half the memory.
 * The stored form is a property of the handle, fixed at create: a_kind = THIP_A_BF16 or THIP_A_F16 (thip_mid16batch_create: f16);
 * THIP_A_F32 is refused -- that is thip_midbatch.  dev_mats_a is the f32 stack thip_midbatch_create takes; it is converted by one
 * launch and NOT referenced after create returns.  replace / set_a / set_a_dev take f32 values and convert them into the slot's
 * block; set_a_dev(NULL), the in-place form, is refused: no f32 A lies in place.
 * The store, per problem: n columns of ld16 = roundup4(m) 16-bit words, column-major, the pad rows zero; THIP_A_F16: n floats inv_s
 * behind the matrix; the block padded to a multiple of 16 bytes.  bf16: the f32 rounded to nearest even to its upper 16 bits.
 * f16: inv_s[c] = 2^(e - 14), e the exponent frexp gives the column's largest finite |a| (1 for a column of zeros), and the word
 * f16(a / inv_s[c]), round to nearest even (the roundings of thip_solver_set_a_dtype).
 * The contract: with W the WIDENED matrix -- W(r, c) the bf16 word shifted left 16 bits, or float(h(r, c)) * inv_s[c] in f32 -- the
 * batch is BIT FOR BIT a thip_midbatch created over W in f32: preconditioner, iterates, compensation terms, status blocks and
 * verdicts, at every workgroup size, in both state arithmetics, however the iterations are cut into launches.  The problem solved
 * is the one with the rounded matrix; its end iterate is a start (thip_midbatch_set_iterates) for the exact one.
 * ------------------------------------------------------------------------------------------- */
typedef struct thip_mid16batch thip_mid16batch;
typedef struct thip_mid16batch_info_t {
    int32_t n_prob, threads;          /* as thip_midbatch_info_t ... */
    int32_t lds_bytes, live;
    size_t  arena_bytes;
    size_t  device_bytes;             /* everything this object allocated on the device, the store included */
    size_t  device_bytes_all;
    int64_t launches, workgroups;
    int32_t load_bytes, a_dtype;      /* 8 for every shape: a lane's 4 rows of a column are one load; THIP_A_BF16 / THIP_A_F16 */
    size_t  a_bytes_per_iter;         /* bytes of the store read per problem-iteration: 2 (2 ld16 n + (f16: 4 n)) */
    size_t  a_store_bytes;            /* the store: n_prob blocks */
} thip_mid16batch_info_t;
int thip_mid16batch_fits(size_t n, size_t m, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                         size_t *host_lds_bytes, int *host_threads);
/* the bytes of one problem's block of the store (needs no device) */
int thip_mid16batch_store_bytes(size_t n, size_t m, int a_kind, size_t *host_bytes);
int thip_mid16batch_create(size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b,
                           const float *dev_vecs_c, const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type,
                           const int64_t *host_seg_len, const thip_param *par, thip_mid16batch **out);
int thip_mid16batch_create_kind(size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b,
                                const float *dev_vecs_c, const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type,
                                const int64_t *host_seg_len, const thip_param *par, int a_kind, thip_mid16batch **out);
int thip_mid16batch_set_param(thip_mid16batch *h, const thip_param *par);
int thip_mid16batch_init(thip_mid16batch *h);
int thip_mid16batch_run(thip_mid16batch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_mid16batch_run_until_any(thip_mid16batch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_mid16batch_status(thip_mid16batch *h, int i, thip_status *host_status);
int thip_mid16batch_solution(thip_mid16batch *h, int i, float *host_x, float *host_y);
int thip_mid16batch_iterate(thip_mid16batch *h, int i, float *host_x, float *host_y);
int thip_mid16batch_precond(thip_mid16batch *h, int i, float *host_dp_tau, float *host_dp_sigma);
int thip_mid16batch_replace(thip_mid16batch *h, int i, const float *dev_mat_a, const float *dev_vec_b, const float *dev_vec_c,
                            const float *dev_vec_b_rowabs);
int thip_mid16batch_set_iterates(thip_mid16batch *h, int first, int count, const float *host_x, const float *host_y);
int thip_mid16batch_set_bc(thip_mid16batch *h, int first, int count, const float *host_b, const float *host_c,
                           const float *host_b_rowabs, const uint8_t *host_has_rowabs, int keep_iterate);
int thip_mid16batch_solutions(thip_mid16batch *h, int first, int count, float *host_x, float *host_y, thip_status *host_status);
int thip_mid16batch_set_a(thip_mid16batch *h, int first, int count, const float *host_values, const int64_t *host_counts, int keep_iterate);
int thip_mid16batch_set_bc_dev(thip_mid16batch *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_b_rowabs,
    const uint8_t *host_has_rowabs, int keep_iterate);
int thip_mid16batch_set_a_dev(thip_mid16batch *h, int first, int count, const float *dev_values, int keep_iterate);
int thip_mid16batch_set_iterates_dev(thip_mid16batch *h, int first, int count, const float *dev_x, const float *dev_y);
int thip_mid16batch_solutions_dev(thip_mid16batch *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state);
/* problem i's block as it lies in the store: n ld16 words, and (THIP_A_F16; else untouched) the n column scales.  Either may be NULL */
int thip_mid16batch_stored(thip_mid16batch *h, int i, uint16_t *host_words, float *host_inv_scale);
int thip_mid16batch_info(const thip_mid16batch *h, thip_mid16batch_info_t *host_info);
int thip_mid16batch_destroy(thip_mid16batch *h);

/* ---------------------------------------------------------------------------------------------
 * Many small SDPs (or mixed programs with PSD blocks), each with its own A: the mid batch's iteration with every PSD cone projected
 * on chip by the problem's own workgroup, between the two passes over A (thip_sdpbatch.hip).  The interface is
 * thip_midbatch's, one for one, and a layout without PSD segments gives thip_midbatch's iterates bit for bit.
 * Accepted: 1 <= m, n <= 4096, segments of all five cones that cover m, every PSD segment of k (k + 1) / 2 rows with 1 <= k <= 64
 * (packed upper triangle by columns, off-diagonals times sqrt 2: what ProbSDP produces), an LDS map of at most 163 840 bytes --
 * 4 (6208 + 8 n + 13 m) + roundup4(m), plus 49 920 when the largest PSD order exceeds 32 --, 1 <= n_prob <= 1 048 576.
 * Everything else is THIP_E_INVALID before anything is allocated.
 * ------------------------------------------------------------------------------------------- */
typedef struct thip_sdpbatch thip_sdpbatch;
typedef struct thip_sdpbatch_info_t {
    int32_t n_prob, threads;          /* as thip_midbatch_info_t ... */
    int32_t lds_bytes, live;
    size_t  arena_bytes;
    size_t  device_bytes;
    size_t  device_bytes_all;         /* summed over every thip_sdpbatch alive in the process */
    int64_t launches, workgroups;
    int32_t load_bytes, reserved;
    size_t  a_bytes_per_iter;
    int32_t max_psd_order, n_psd;     /* ... and: the largest PSD order of the layout (0: none), the number of PSD segments */
    size_t  psd_lds_bytes;            /* LDS the projection adds beyond the vectors: 0 (orders <= 32 overlay the pass scratch) or 49 920 */
} thip_sdpbatch_info_t;
/* the shape rules alone (needs no device): 0 and the LDS bytes / threads of one workgroup, or THIP_E_INVALID */
int thip_sdpbatch_fits(size_t n, size_t m, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                       size_t *host_lds_bytes, int *host_threads);
int thip_sdpbatch_create(size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b,
                         const float *dev_vecs_c, const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type,
                         const int64_t *host_seg_len, const thip_param *par, thip_sdpbatch **out);
int thip_sdpbatch_set_param(thip_sdpbatch *h, const thip_param *par);
int thip_sdpbatch_init(thip_sdpbatch *h);
int thip_sdpbatch_run(thip_sdpbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_sdpbatch_run_until_any(thip_sdpbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_sdpbatch_status(thip_sdpbatch *h, int i, thip_status *host_status);
int thip_sdpbatch_solution(thip_sdpbatch *h, int i, float *host_x, float *host_y);
int thip_sdpbatch_iterate(thip_sdpbatch *h, int i, float *host_x, float *host_y);
int thip_sdpbatch_precond(thip_sdpbatch *h, int i, float *host_dp_tau, float *host_dp_sigma);
int thip_sdpbatch_replace(thip_sdpbatch *h, int i, const float *dev_mat_a, const float *dev_vec_b, const float *dev_vec_c,
                          const float *dev_vec_b_rowabs);
int thip_sdpbatch_set_iterates(thip_sdpbatch *h, int first, int count, const float *host_x, const float *host_y);
int thip_sdpbatch_set_bc(thip_sdpbatch *h, int first, int count, const float *host_b, const float *host_c,
                         const float *host_b_rowabs, const uint8_t *host_has_rowabs, int keep_iterate);
int thip_sdpbatch_solutions(thip_sdpbatch *h, int first, int count, float *host_x, float *host_y, thip_status *host_status);
int thip_sdpbatch_set_a(thip_sdpbatch *h, int first, int count, const float *host_values, const int64_t *host_counts, int keep_iterate);
int thip_sdpbatch_set_bc_dev(thip_sdpbatch *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_b_rowabs,
    const uint8_t *host_has_rowabs, int keep_iterate);
int thip_sdpbatch_set_a_dev(thip_sdpbatch *h, int first, int count, const float *dev_values, int keep_iterate);
int thip_sdpbatch_set_iterates_dev(thip_sdpbatch *h, int first, int count, const float *dev_x, const float *dev_y);
int thip_sdpbatch_solutions_dev(thip_sdpbatch *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state);
int thip_sdpbatch_info(const thip_sdpbatch *h, thip_sdpbatch_info_t *host_info);
int thip_sdpbatch_destroy(thip_sdpbatch *h);

/* ---------------------------------------------------------------------------------------------
 * The WIDE batch: thip_sdpbatch's iteration on every shape up to 4096 x 4096 (thip_widebatch.hip).  Only what a pass
 * over A touches lies in LDS -- the iterates x_x u x_y v, the pass results, the class bytes --; every other vector of the iteration is
 * read and written in place in the problem's block of the arena (6 n + 11 m floats), so the shape rule is no longer the vectors'.
 * The interface is thip_sdpbatch's, one for one, and on a shape that thip_midbatch / thip_sdpbatch also takes the iterates, the status
 * blocks and the first 6 n + 10 m floats of a problem's arena block are theirs bit for bit.
 * Accepted: 1 <= m, n <= 4096, segments of all five cones that cover m, every PSD segment of k (k + 1) / 2 rows with 1 <= k <= 64, an
 * LDS map of at most 163 840 bytes -- 4 (6208 + 3 n + 3 m) + roundup4(m), plus 49 920 when the largest PSD order exceeds 32: without
 * such an order every shape fits (4096 x 4096 takes 127 232 bytes), with one 12 (n + m) + roundup4(m) <= 89 088 --,
 * 1 <= n_prob <= 1 048 576.  Everything else is THIP_E_INVALID before anything is allocated.  No chooser returns this family: whether
 * it beats one thip_solver per problem in turn depends on the number of problems (README.md).
 * ------------------------------------------------------------------------------------------- */
typedef struct thip_widebatch thip_widebatch;
typedef struct thip_widebatch_info_t {
    int32_t n_prob, threads;          /* as thip_sdpbatch_info_t ... */
    int32_t lds_bytes, live;
    size_t  arena_bytes;
    size_t  device_bytes;
    size_t  device_bytes_all;         /* summed over every thip_widebatch alive in the process */
    int64_t launches, workgroups;
    int32_t load_bytes, reserved;
    size_t  a_bytes_per_iter;
    int32_t max_psd_order, n_psd;
    size_t  psd_lds_bytes;
    size_t  lds_bytes_per_problem;    /* ... and: the LDS of one problem's workgroup in the iteration (what thip_widebatch_fits reports) */
    size_t  arena_bytes_per_problem;  /* one problem's block of the arena: 4 (6 n + 11 m) */
} thip_widebatch_info_t;
/* the shape rules alone (needs no device): 0 and the LDS bytes / threads of one workgroup, or THIP_E_INVALID */
int thip_widebatch_fits(size_t n, size_t m, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                        size_t *host_lds_bytes, int *host_threads);
int thip_widebatch_create(size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b,
                          const float *dev_vecs_c, const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type,
                          const int64_t *host_seg_len, const thip_param *par, thip_widebatch **out);
int thip_widebatch_set_param(thip_widebatch *h, const thip_param *par);
int thip_widebatch_init(thip_widebatch *h);
int thip_widebatch_run(thip_widebatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_widebatch_run_until_any(thip_widebatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_widebatch_status(thip_widebatch *h, int i, thip_status *host_status);
int thip_widebatch_solution(thip_widebatch *h, int i, float *host_x, float *host_y);
int thip_widebatch_iterate(thip_widebatch *h, int i, float *host_x, float *host_y);
int thip_widebatch_precond(thip_widebatch *h, int i, float *host_dp_tau, float *host_dp_sigma);
int thip_widebatch_replace(thip_widebatch *h, int i, const float *dev_mat_a, const float *dev_vec_b, const float *dev_vec_c,
                           const float *dev_vec_b_rowabs);
int thip_widebatch_set_iterates(thip_widebatch *h, int first, int count, const float *host_x, const float *host_y);
int thip_widebatch_set_bc(thip_widebatch *h, int first, int count, const float *host_b, const float *host_c,
                          const float *host_b_rowabs, const uint8_t *host_has_rowabs, int keep_iterate);
int thip_widebatch_solutions(thip_widebatch *h, int first, int count, float *host_x, float *host_y, thip_status *host_status);
int thip_widebatch_set_a(thip_widebatch *h, int first, int count, const float *host_values, const int64_t *host_counts, int keep_iterate);
int thip_widebatch_set_bc_dev(thip_widebatch *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_b_rowabs,
    const uint8_t *host_has_rowabs, int keep_iterate);
int thip_widebatch_set_a_dev(thip_widebatch *h, int first, int count, const float *dev_values, int keep_iterate);
int thip_widebatch_set_iterates_dev(thip_widebatch *h, int first, int count, const float *dev_x, const float *dev_y);
int thip_widebatch_solutions_dev(thip_widebatch *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state);
int thip_widebatch_info(const thip_widebatch *h, thip_widebatch_info_t *host_info);
int thip_widebatch_destroy(thip_widebatch *h);

/* ---------------------------------------------------------------------------------------------
 * The wide batch over a LIBRARY-OWNED 16-BIT COPY of every problem's A (thip_wide16batch.hip): thip_widebatch's shapes
 * (thip_wide16batch_fits is thip_widebatch_fits, PSD cones included), cones, iteration and interface; the store, its two rounding rules,
 * a_kind and the calls that convert are thip_mid16batch's, word for word (thip_wide16batch_create: f16; THIP_A_F32 is refused -- that
 * is thip_widebatch; dev_mats_a is NOT referenced after create returns; set_a_dev(NULL) is refused: no f32 A lies in place).
 * The contract: with W the WIDENED matrix (as thip_mid16batch defines it) the batch is BIT FOR BIT a thip_widebatch created over W in
 * f32: the whole arena block (6 n + 11 m floats), preconditioner, iterates, compensation terms, status blocks and verdicts, at both
 * workgroup sizes, in both state arithmetics, however the iterations are cut into launches.  The problem solved is the one with the
 * rounded matrix; its end iterate is a start (thip_widebatch_set_iterates) for the exact one.  No chooser returns this family.
 * ------------------------------------------------------------------------------------------- */
typedef struct thip_wide16batch thip_wide16batch;
typedef struct thip_wide16batch_info_t {
    int32_t n_prob, threads;          /* as thip_widebatch_info_t ... */
    int32_t lds_bytes, live;
    size_t  arena_bytes;
    size_t  device_bytes;             /* everything this object allocated on the device, the store included */
    size_t  device_bytes_all;         /* summed over every thip_wide16batch alive in the process */
    int64_t launches, workgroups;
    int32_t load_bytes, a_dtype;      /* 8 for every shape: a lane's 4 rows of a column are one load; THIP_A_BF16 / THIP_A_F16 */
    size_t  a_bytes_per_iter;         /* bytes of the store read per problem-iteration: 2 (2 ld16 n + (f16: 4 n)) */
    int32_t max_psd_order, n_psd;
    size_t  psd_lds_bytes;
    size_t  lds_bytes_per_problem;    /* what thip_wide16batch_fits reports */
    size_t  arena_bytes_per_problem;  /* one problem's block of the arena: 4 (6 n + 11 m) */
    size_t  a_store_bytes;            /* ... and the store: n_prob blocks */
} thip_wide16batch_info_t;
/* the shape rules alone (needs no device): thip_widebatch_fits' */
int thip_wide16batch_fits(size_t n, size_t m, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                          size_t *host_lds_bytes, int *host_threads);
/* the bytes of one problem's block of the store (needs no device): thip_mid16batch_store_bytes' */
int thip_wide16batch_store_bytes(size_t n, size_t m, int a_kind, size_t *host_bytes);
int thip_wide16batch_create(size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b,
                            const float *dev_vecs_c, const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type,
                            const int64_t *host_seg_len, const thip_param *par, thip_wide16batch **out);
int thip_wide16batch_create_kind(size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b,
                                 const float *dev_vecs_c, const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type,
                                 const int64_t *host_seg_len, const thip_param *par, int a_kind, thip_wide16batch **out);
int thip_wide16batch_set_param(thip_wide16batch *h, const thip_param *par);
int thip_wide16batch_init(thip_wide16batch *h);
int thip_wide16batch_run(thip_wide16batch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_wide16batch_run_until_any(thip_wide16batch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_wide16batch_status(thip_wide16batch *h, int i, thip_status *host_status);
int thip_wide16batch_solution(thip_wide16batch *h, int i, float *host_x, float *host_y);
int thip_wide16batch_iterate(thip_wide16batch *h, int i, float *host_x, float *host_y);
int thip_wide16batch_precond(thip_wide16batch *h, int i, float *host_dp_tau, float *host_dp_sigma);
int thip_wide16batch_replace(thip_wide16batch *h, int i, const float *dev_mat_a, const float *dev_vec_b, const float *dev_vec_c,
                             const float *dev_vec_b_rowabs);
int thip_wide16batch_set_iterates(thip_wide16batch *h, int first, int count, const float *host_x, const float *host_y);
int thip_wide16batch_set_bc(thip_wide16batch *h, int first, int count, const float *host_b, const float *host_c,
                            const float *host_b_rowabs, const uint8_t *host_has_rowabs, int keep_iterate);
int thip_wide16batch_solutions(thip_wide16batch *h, int first, int count, float *host_x, float *host_y, thip_status *host_status);
int thip_wide16batch_set_a(thip_wide16batch *h, int first, int count, const float *host_values, const int64_t *host_counts, int keep_iterate);
int thip_wide16batch_set_bc_dev(thip_wide16batch *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_b_rowabs,
    const uint8_t *host_has_rowabs, int keep_iterate);
int thip_wide16batch_set_a_dev(thip_wide16batch *h, int first, int count, const float *dev_values, int keep_iterate);
int thip_wide16batch_set_iterates_dev(thip_wide16batch *h, int first, int count, const float *dev_x, const float *dev_y);
int thip_wide16batch_solutions_dev(thip_wide16batch *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state);
/* problem i's block as it lies in the store: n ld16 words, and (THIP_A_F16; else untouched) the n column scales.  Either may be NULL */
int thip_wide16batch_stored(thip_wide16batch *h, int i, uint16_t *host_words, float *host_inv_scale);
int thip_wide16batch_info(const thip_wide16batch *h, thip_wide16batch_info_t *host_info);
int thip_wide16batch_destroy(thip_wide16batch *h);

/* ---------------------------------------------------------------------------------------------
 * The RAGGED batch: many conic programs, each with its own dense f32 A, its own n_p, m_p and its own cone layout, in one batch
 * (thip_raggedbatch.hip).  The iteration is thip_sdpbatch's on every problem -- one workgroup per running problem,
 * its vectors in LDS, its A streamed twice per iteration, its PSD cones projected on chip --, and a problem's iterates are, bit for
 * bit, those of a thip_midbatch / thip_sdpbatch that holds it alone.  A problem is taken exactly when thip_sdpbatch_fits takes it.
 * The arrays: one device array per kind (A, b, c, the row sums) and, per problem, its offset into it IN FLOATS (host_at_*), so the
 * caller decides where every A lies: an A whose address is a multiple of 16 bytes and whose m_p is a multiple of 4 is read with
 * 16-byte loads, every other one with 4-byte loads of the same entries.  Problem p's A is column-major, lda = m_p.  The cone
 * segments are concatenated problem after problem; host_n_seg[p] says how many belong to problem p.  host_at_rowabs[p] == -1 (or a
 * NULL array): problem p carries no row sums and uses |b|.
 * A launch has one workgroup size and one LDS size: the problems are split by shape into a 256-thread and a 1024-thread class
 * (m_p n_p <= 8192: 256), each with the largest LDS map of its members, and every poll makes one launch per class that has a
 * running problem, the longest problems (m_p n_p) first.  Problems take 6 n_p + 10 m_p floats of the arena each, packed; identical
 * layouts (m, segments) share one cone table.  1 <= n_prob <= 1 048 576.  Everything else is THIP_E_INVALID before anything is
 * allocated, and the message names the first problem refused.
 * Lengths are the problem's own: solution(i) writes n_i and m_i floats, iterate(i) n_i + 2 m_i + 1 and n_i + m_i + 1, precond(i)
 * the same.  replace(i, ...) hands slot i new data of ITS shape and layout: the init kernel on that slot.
 * ------------------------------------------------------------------------------------------- */
typedef struct thip_raggedbatch thip_raggedbatch;
typedef struct thip_raggedbatch_class_t {
    int32_t n_prob, live;             /* members; members RUNNING as of the last poll */
    int32_t threads, lds_bytes;       /* of every workgroup of the class: 256 or 1024; the largest map of its members */
    int64_t launches, workgroups;     /* issued by run / run_until_any since thip_raggedbatch_init */
} thip_raggedbatch_class_t;
typedef struct thip_raggedbatch_info_t {
    int32_t n_prob, live;
    int32_t n_layouts, n_load16;      /* distinct (m, segments) tables; problems whose A is read with 16-byte loads */
    size_t  arena_bytes;              /* the problems' state, packed: 4 sum (6 n_p + 10 m_p) */
    size_t  device_bytes;             /* everything this object allocated on the device */
    size_t  device_bytes_all;         /* the same, summed over every thip_raggedbatch alive in the process */
    int64_t launches, workgroups;     /* summed over the classes */
    size_t  a_bytes_per_iter;         /* bytes of A read when every problem advances one iteration: sum 2 m_p n_p 4 */
    thip_raggedbatch_class_t cls[2];  /* the 256-thread class, the 1024-thread class */
} thip_raggedbatch_info_t;
/* the shape rules alone (needs no device): 0, or THIP_E_INVALID with the index of the first problem refused in *host_first_refused
 * (-1: the refusal names no problem).  host_lds_bytes / host_threads: n_prob entries, what one workgroup of the problem alone
 * would take; either may be NULL */
int thip_raggedbatch_fits(size_t n_prob, const size_t *host_n, const size_t *host_m, const size_t *host_n_seg,
                          const int32_t *host_seg_type, const int64_t *host_seg_len, int *host_first_refused,
                          size_t *host_lds_bytes, int *host_threads);
int thip_raggedbatch_create(size_t n_prob, const size_t *host_n, const size_t *host_m, const float *dev_a, const int64_t *host_at_a,
                            const float *dev_b, const int64_t *host_at_b, const float *dev_c, const int64_t *host_at_c,
                            const float *dev_b_rowabs, const int64_t *host_at_rowabs, const size_t *host_n_seg,
                            const int32_t *host_seg_type, const int64_t *host_seg_len, const thip_param *par,
                            thip_raggedbatch **out);
int thip_raggedbatch_set_param(thip_raggedbatch *h, const thip_param *par);
int thip_raggedbatch_init(thip_raggedbatch *h);
int thip_raggedbatch_run(thip_raggedbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_raggedbatch_run_until_any(thip_raggedbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_raggedbatch_status(thip_raggedbatch *h, int i, thip_status *host_status);
int thip_raggedbatch_solution(thip_raggedbatch *h, int i, float *host_x, float *host_y);
int thip_raggedbatch_iterate(thip_raggedbatch *h, int i, float *host_x, float *host_y);
int thip_raggedbatch_precond(thip_raggedbatch *h, int i, float *host_dp_tau, float *host_dp_sigma);
int thip_raggedbatch_replace(thip_raggedbatch *h, int i, const float *dev_mat_a, const float *dev_vec_b, const float *dev_vec_c,
                             const float *dev_vec_b_rowabs);
int thip_raggedbatch_set_iterates(thip_raggedbatch *h, int first, int count, const float *host_x, const float *host_y);
int thip_raggedbatch_set_bc(thip_raggedbatch *h, int first, int count, const float *host_b, const float *host_c,
                            const float *host_b_rowabs, const uint8_t *host_has_rowabs, int keep_iterate);
int thip_raggedbatch_solutions(thip_raggedbatch *h, int first, int count, float *host_x, float *host_y, thip_status *host_status);
int thip_raggedbatch_set_a(thip_raggedbatch *h, int first, int count, const float *host_values, const int64_t *host_counts, int keep_iterate);
int thip_raggedbatch_set_bc_dev(thip_raggedbatch *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_b_rowabs,
    const uint8_t *host_has_rowabs, int keep_iterate);
int thip_raggedbatch_set_a_dev(thip_raggedbatch *h, int first, int count, const float *dev_values, int keep_iterate);
int thip_raggedbatch_set_iterates_dev(thip_raggedbatch *h, int first, int count, const float *dev_x, const float *dev_y);
int thip_raggedbatch_solutions_dev(thip_raggedbatch *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state);
int thip_raggedbatch_info(const thip_raggedbatch *h, thip_raggedbatch_info_t *host_info);
int thip_raggedbatch_destroy(thip_raggedbatch *h);

/* ---------------------------------------------------------------------------------------------
 * Many problems of one shape n, m and one cone layout, each with its own SPARSE A with its own pattern (thip_sparsebatch.hip;
 * DESIGN.md 4.2).  The iteration is thip_sdpbatch's -- one workgroup per running problem, its vectors in LDS, all five cones, PSD
 * orders <= 64 projected on chip --, but a pass walks the problem's entries instead of streaming m n floats.  Problem p arrives as
 * HOST CSC arrays (column pointers from 0, row indices strictly ascending inside a column, f32 values; explicit zeros are kept as
 * entries); the library packs every problem on the host into a blob of 4-byte words that holds the entries twice, in column order
 * and in row order, and uploads all of them in one copy.  Every slot reserves the same capacity,
 * 16 nnz_cap + 4 (2 (m + n) + 4) bytes rounded up to 16, so replace can hand a slot another pattern of at most nnz_cap entries.
 * The rule is thip_sdpbatch_fits' on (n, m, layout).  The blob is RESIDENT -- copied into LDS once per launch and read there -- when
 * the LDS map of thip_sdpbatch plus the capacity is at most 163 840 bytes; otherwise the batch is taken all the same and every pass
 * reads the entries from memory (STREAMED).  Both give the same bits.  Refused (THIP_E_INVALID, before anything is allocated):
 * column pointers that are not monotone from 0, a row index out of range or not strictly ascending, a value that is not finite,
 * more entries than nnz_cap, nnz_cap > m n, and what thip_sdpbatch_fits refuses.
 * ------------------------------------------------------------------------------------------- */
typedef struct thip_sparsebatch thip_sparsebatch;
typedef struct thip_sparsebatch_info_t {
    int32_t n_prob, threads;          /* as thip_midbatch_info_t ... */
    int32_t lds_bytes, live;
    size_t  arena_bytes;
    size_t  device_bytes;             /* everything this object allocated on the device, the blobs among it */
    size_t  device_bytes_all;         /* summed over every thip_sparsebatch alive in the process */
    int64_t launches, workgroups;
    size_t  a_bytes_per_iter;         /* bytes of A read from memory per problem-iteration: 0 when resident, else twice the blob's
                                         used bytes (the mean over the slots) */
    int32_t max_psd_order, n_psd;     /* as thip_sdpbatch_info_t */
    size_t  psd_lds_bytes;
    size_t  nnz_cap;                  /* entries a slot can take */
    size_t  nnz_total;                /* entries held, summed over the slots */
    size_t  blob_bytes;               /* the capacity every slot reserves */
    int32_t resident, reserved;       /* 1: the blob is read from LDS, 0: from memory */
} thip_sparsebatch_info_t;
/* the rule alone (needs no device): 0 and the LDS bytes / threads of one workgroup and whether a blob of capacity nnz_cap is
 * resident, or THIP_E_INVALID */
int thip_sparsebatch_fits(size_t n, size_t m, size_t nnz_cap, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                          size_t *host_lds_bytes, int *host_threads, int *host_resident);
/* host_colptr: n_prob (n + 1) column pointers, each problem's from 0; problem p's row indices and values are the
 * host_colptr[p (n + 1) + n] entries of host_rowidx / host_values from host_start[p] on.  dev_vecs_b, dev_vecs_c,
 * dev_vecs_b_rowabs (may be NULL: |b|): device arrays, problem after problem.  nnz_cap: 0 = the largest entry count given */
int thip_sparsebatch_create(size_t n, size_t m, size_t n_prob, const int64_t *host_colptr, const int64_t *host_start,
                            const int32_t *host_rowidx, const float *host_values, const float *dev_vecs_b, const float *dev_vecs_c,
                            const float *dev_vecs_b_rowabs, size_t nnz_cap, size_t n_seg, const int32_t *host_seg_type,
                            const int64_t *host_seg_len, const thip_param *par, thip_sparsebatch **out);
int thip_sparsebatch_set_param(thip_sparsebatch *h, const thip_param *par);
int thip_sparsebatch_init(thip_sparsebatch *h);
int thip_sparsebatch_run(thip_sparsebatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_sparsebatch_run_until_any(thip_sparsebatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_sparsebatch_status(thip_sparsebatch *h, int i, thip_status *host_status);
int thip_sparsebatch_solution(thip_sparsebatch *h, int i, float *host_x, float *host_y);
int thip_sparsebatch_iterate(thip_sparsebatch *h, int i, float *host_x, float *host_y);
int thip_sparsebatch_precond(thip_sparsebatch *h, int i, float *host_dp_tau, float *host_dp_sigma);
/* slot i -- running or stopped -- takes the host CSC arrays of one problem (any pattern of at most nnz_cap entries) and device
 * b, c, row sums, and is initialised afresh; no other slot is touched */
int thip_sparsebatch_replace(thip_sparsebatch *h, int i, const int64_t *host_colptr, const int32_t *host_rowidx,
                             const float *host_values, const float *dev_vec_b, const float *dev_vec_c, const float *dev_vec_b_rowabs);
int thip_sparsebatch_set_iterates(thip_sparsebatch *h, int first, int count, const float *host_x, const float *host_y);
int thip_sparsebatch_set_bc(thip_sparsebatch *h, int first, int count, const float *host_b, const float *host_c,
                            const float *host_b_rowabs, const uint8_t *host_has_rowabs, int keep_iterate);
int thip_sparsebatch_solutions(thip_sparsebatch *h, int first, int count, float *host_x, float *host_y, thip_status *host_status);
int thip_sparsebatch_set_a(thip_sparsebatch *h, int first, int count, const float *host_values, const int64_t *host_counts, int keep_iterate);
int thip_sparsebatch_set_bc_dev(thip_sparsebatch *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_b_rowabs,
    const uint8_t *host_has_rowabs, int keep_iterate);
int thip_sparsebatch_set_a_dev(thip_sparsebatch *h, int first, int count, const float *dev_values, int keep_iterate);
int thip_sparsebatch_set_iterates_dev(thip_sparsebatch *h, int first, int count, const float *dev_x, const float *dev_y);
int thip_sparsebatch_solutions_dev(thip_sparsebatch *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state);
int thip_sparsebatch_info(const thip_sparsebatch *h, thip_sparsebatch_info_t *host_info);
int thip_sparsebatch_destroy(thip_sparsebatch *h);

/* ---------------------------------------------------------------------------------------------
 * The RAGGED SPARSE batch: many conic programs in one batch, each with its own SPARSE A with its own pattern, its own n_p, m_p and
 * its own cone layout (thip_raggedsparse.hip).  The ragged batch's lookup and the sparse batch's stored form together:
 * one workgroup per running problem finds its problem in a table of descriptors and walks that problem's packed entries.  A
 * problem's preconditioner, iterates and status are, bit for bit, those of a thip_sparsebatch that holds it alone at the same
 * workgroup size.
 * A problem is taken exactly when thip_sdpbatch_fits takes its (n_p, m_p, layout) and its capacity is at most m_p n_p.  Slot p
 * reserves 16 cap_p + 4 (2 (m_p + n_p) + 4) bytes rounded up to 16 of the packed blobs; cap_p is the problem's own entry count unless
 * host_nnz_cap gives more (NULL, or an entry of 0: the own count), so replace can hand the slot another pattern of at most cap_p
 * entries.  The workgroup size is the sparse batch's rule on (n_p, m_p, cap_p): 256 threads when max(m_p, n_p) <= 1024 and
 * cap_p <= 8192, else 1024 -- two classes, one launch per class and poll, a class's live list by descending entry count.  A problem
 * is RESIDENT (its blob copied into LDS once per launch) exactly when the LDS map of thip_sdpbatch for it plus its capacity is at
 * most 163 840 bytes -- per problem: resident and streamed members share a class and a launch -- and a class's LDS is the largest
 * need of its members.  The state is packed, 6 n_p + 10 m_p floats each; identical layouts share one cone table.
 * The arrays: the column pointers of all problems concatenated (n_p + 1 each, from 0), problem p's row indices and values the
 * entries of host_rowidx / host_values from host_start[p] on; b, c and the row sums one device array per kind with per-problem
 * offsets IN FLOATS, the cone segments concatenated, as in thip_raggedbatch_create.  Every problem's arrays are checked on the host
 * (the refusals of thip_sparsebatch_create) before anything is allocated, and a refusal names the first problem refused.
 * Lengths are the problem's own, as in the ragged batch.  1 <= n_prob <= 1 048 576.
 * ------------------------------------------------------------------------------------------- */
typedef struct thip_raggedsparse thip_raggedsparse;
typedef struct thip_raggedsparse_class_t {
    int32_t n_prob, live;             /* members; members RUNNING as of the last poll */
    int32_t threads, lds_bytes;       /* of every workgroup of the class: 256 or 1024; the largest need of its members */
    int64_t launches, workgroups;     /* issued by run / run_until_any since thip_raggedsparse_init */
    int32_t n_resident, reserved;     /* members whose blob is read from LDS */
} thip_raggedsparse_class_t;
typedef struct thip_raggedsparse_info_t {
    int32_t n_prob, live;
    int32_t n_layouts, n_resident;    /* distinct (m, segments) tables; problems whose blob is read from LDS */
    size_t  arena_bytes;              /* the problems' state, packed: 4 sum (6 n_p + 10 m_p) */
    size_t  device_bytes;             /* everything this object allocated on the device, the blobs among it */
    size_t  device_bytes_all;         /* the same, summed over every thip_raggedsparse alive in the process */
    int64_t launches, workgroups;     /* summed over the classes */
    size_t  a_bytes_per_iter;         /* bytes of A read from memory when every problem advances one iteration: twice the used
                                         bytes of the blobs that are not resident */
    int32_t max_psd_order, n_psd;     /* the largest PSD order of any problem; PSD cones, summed over the problems */
    size_t  psd_lds_bytes;            /* the largest operand tail of any problem */
    size_t  nnz_total;                /* entries held, summed over the slots */
    size_t  blob_bytes;               /* the capacities the slots reserve, summed */
    thip_raggedsparse_class_t cls[2]; /* the 256-thread class, the 1024-thread class */
} thip_raggedsparse_info_t;
/* the rules alone (needs no device): 0, or THIP_E_INVALID with the index of the first problem refused in *host_first_refused (-1:
 * the refusal names no problem).  host_nnz_cap: the capacities (NULL: 0 entries each).  host_lds_bytes / host_threads /
 * host_resident: n_prob entries, what one workgroup of the problem takes; each may be NULL */
int thip_raggedsparse_fits(size_t n_prob, const size_t *host_n, const size_t *host_m, const size_t *host_nnz_cap,
                           const size_t *host_n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                           int *host_first_refused, size_t *host_lds_bytes, int *host_threads, int *host_resident);
int thip_raggedsparse_create(size_t n_prob, const size_t *host_n, const size_t *host_m, const int64_t *host_colptr,
                             const int64_t *host_start, const int32_t *host_rowidx, const float *host_values,
                             const size_t *host_nnz_cap, const float *dev_b, const int64_t *host_at_b, const float *dev_c,
                             const int64_t *host_at_c, const float *dev_b_rowabs, const int64_t *host_at_rowabs,
                             const size_t *host_n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                             const thip_param *par, thip_raggedsparse **out);
int thip_raggedsparse_set_param(thip_raggedsparse *h, const thip_param *par);
int thip_raggedsparse_init(thip_raggedsparse *h);
int thip_raggedsparse_run(thip_raggedsparse *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_raggedsparse_run_until_any(thip_raggedsparse *h, int64_t max_steps, int64_t poll_every, thip_status *host_status);
int thip_raggedsparse_status(thip_raggedsparse *h, int i, thip_status *host_status);
int thip_raggedsparse_solution(thip_raggedsparse *h, int i, float *host_x, float *host_y);
int thip_raggedsparse_iterate(thip_raggedsparse *h, int i, float *host_x, float *host_y);
int thip_raggedsparse_precond(thip_raggedsparse *h, int i, float *host_dp_tau, float *host_dp_sigma);
/* slot i -- running or stopped -- takes the host CSC arrays of another problem of ITS shape and layout (any pattern of at most
 * cap_i entries) and device b, c, row sums, and is initialised afresh; no other slot is touched, and a refusal leaves slot i as
 * it was */
int thip_raggedsparse_replace(thip_raggedsparse *h, int i, const int64_t *host_colptr, const int32_t *host_rowidx,
                              const float *host_values, const float *dev_vec_b, const float *dev_vec_c,
                              const float *dev_vec_b_rowabs);
int thip_raggedsparse_set_iterates(thip_raggedsparse *h, int first, int count, const float *host_x, const float *host_y);
int thip_raggedsparse_set_bc(thip_raggedsparse *h, int first, int count, const float *host_b, const float *host_c,
                             const float *host_b_rowabs, const uint8_t *host_has_rowabs, int keep_iterate);
int thip_raggedsparse_solutions(thip_raggedsparse *h, int first, int count, float *host_x, float *host_y, thip_status *host_status);
int thip_raggedsparse_set_a(thip_raggedsparse *h, int first, int count, const float *host_values, const int64_t *host_counts, int keep_iterate);
int thip_raggedsparse_set_bc_dev(thip_raggedsparse *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_b_rowabs,
    const uint8_t *host_has_rowabs, int keep_iterate);
int thip_raggedsparse_set_a_dev(thip_raggedsparse *h, int first, int count, const float *dev_values, int keep_iterate);
int thip_raggedsparse_set_iterates_dev(thip_raggedsparse *h, int first, int count, const float *dev_x, const float *dev_y);
int thip_raggedsparse_solutions_dev(thip_raggedsparse *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state);
int thip_raggedsparse_info(const thip_raggedsparse *h, thip_raggedsparse_info_t *host_info);
int thip_raggedsparse_destroy(thip_raggedsparse *h);

/* What THIS device streams: a bare non-temporal read of `bytes` at dev_ptr (device memory, 16-byte aligned -- e.g. the
 * solver's own A), best and average of `reps` timed launches per grid (HIP events).  bench.py prints it beside the
 * sweep's rate: the boxes of one pool differ by several percent, and a roofline fraction means little without it. */
int thip_stream_probe(const void *dev_ptr, size_t bytes, int reps, float *host_best_ms, float *host_avg_ms);

/* The one-pass kernel is persistent and every wait in it is bounded.  When a workgroup gives up (placement changed under
 * it, a peer workgroup was withheld), thip_solver_run restores the iterate of the last completed batch from a device
 * snapshot, re-arms the kernel's census and tries the batch once more; a second failure in a row hands the rest of the
 * solve to the 2-pass carried schedule (thip_solver_schedule_in_use then says THIP_SCHED_CARRIED); a
 * column-sharded run, which has no 2-pass form, raises the fault through its all-reduce so that every rank restores the
 * same iterate and retries together, and fails with THIP_E_TIMEOUT on every rank at once after two retries.
 * host_faults = recoveries so far in this solve, host_last_word = the kernel's error word of the last one (1, 2 census,
 * 3 a gather ran out of spins), host_restored_iter = the iteration the restored snapshot held (-1: none). */
int thip_solver_sweep_faults(thip_solver *s, int *host_faults, int *host_last_word, int64_t *host_restored_iter);
/* partial dots published with agent-scope (sc1) stores (1), with plain stores that stay in the group's L2 (0), or by the
 * verdict of the process's publish-scope self-test (-1, the default); between thip_solver_run calls */
int thip_solver_set_sweep_publish(thip_solver *s, int agent_scope);
/* The publish-scope self-test: once per process, before the first plan of the one-pass kernel, 200 sweeps of a scratch matrix
 * with 32 members per group, a short polling bound and the kernel's poll counters decide whether plain-store publishing is
 * visible to the gatherers on this driver / firmware (0) or every solver publishes at agent scope (1).  mode 0: the cached
 * verdict (run now if need be); 1: run again; 2: run again and count it as failed (test hook).  host_info (4 ints): the
 * kernel's error word, polls summed over all gathers, the most polls any one gather needed, sweeps run.
 * THIP_SWEEP_PUBLISH=0 / 1 in the environment pins the verdict without a test. */
int thip_sweep_publish_selftest(int mode, int *host_agent_scope, int *host_info);


/* the GEMV tiling chosen by the create-time autotune (rows groups per lane, grid size, its measured ms); 0 = heuristic */
int thip_solver_gemv_plan(const thip_solver *s, int *host_nj, int *host_blocks, float *host_ms);

/* per-launch timing of the pass over A in the fused loop (HIP events on the launch stream): enable, run, then read the
 * number of timed launches and their summed duration.  Used by bench.py's roofline.  on = 0: off; on = N >= 1: every N-th
 * launch is timed (an event pair costs the stream 3-5 us: with N = 1 that is 9 % of a 0.14 ms iteration). */
int thip_prof_enable(int on);
/* the same for the PSD cones of the fused loop: one span per iteration around the projection chains of all its PSD blocks
 * (x_y and x_s together): number of spans timed and their summed duration -- bench.py's roofline_eig */
int thip_prof_read_psd(int64_t *host_spans, double *host_total_ms);
int thip_prof_read(int64_t *host_launches, double *host_total_ms);     /* SYNC */

/* ---------------------------------------------------------------------------------------------
 * Synthetic data on the device (bench / tests): counter-based generator keyed by
 * (seed, stream, index), bit-identical to oracle/totsu_oracle.c:oc_rng_*.
 * kind 0: U[0,1) ; kind 1: approx N(0,1) (Irwin-Hall 4).  out[i] = scale * g(idx0 + i) + shift.
 * For a column-major block: index of element (r,c) is (row0 + r) + (col0 + c) * ld_index.
 * ------------------------------------------------------------------------------------------- */
int thip_gen_vector(float *out, size_t n, uint64_t seed, uint64_t stream, uint64_t idx0,
                    int kind, float scale, float shift);
int thip_gen_matrix(float *out, size_t n_row, size_t n_col, size_t lda, uint64_t seed, uint64_t stream,
                    uint64_t row0, uint64_t col0, uint64_t ld_index, int kind, float scale, float shift);
/* out(r, c) = value if row0 + r == c else 0 over an n_row x n_col block (the -I rows of the benchmark_lp matrix,
 * experimental/benchmark_lp/src/main.rs:27-40) */
int thip_gen_identity(float *out, size_t n_row, size_t n_col, size_t lda, uint64_t row0, float value);

/* Test hooks and timing probes (thip_test_*: fault injection, engine switches, the kernels alone) are declared in
 * totsu_f32hip_test.h: exported by the same library, used by tests/ and tools/, not part of the interface a binding wraps. */

#ifdef __cplusplus
}
#endif
#endif /* TOTSU_F32HIP_H */
