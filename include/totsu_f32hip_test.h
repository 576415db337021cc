/* totsu_f32hip_test.h -- test hooks and timing probes of libtotsu_f32hip.so.
 *
 * Everything here is exported by the same shared library as include/totsu_f32hip.h but is NOT part of the interface a
 * binding wraps (the Rust crate declares them behind its `test-hooks` feature): fault injection into the persistent
 * kernel's recovery paths, switches that force an engine, and entry points that run one kernel alone so that
 * tests/ can compare it with numpy / the oracle and tools/ can time it.  None of them is called by the product path. */
#ifndef TOTSU_F32HIP_TEST_H
#define TOTSU_F32HIP_TEST_H

#include "totsu_f32hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* test switch: 0 = the library's choice, 1 = the QL engine, 2 = the device engine with its certificate forced to fail
 * (exercises the hand-over); + 4 = the Householder reduction as ONE persistent launch over the whole device (granule
 * all-gather per reflector over the fabric), + 8 = the same on the workgroups of one XCD (through its L2: the default up
 * to order 1024), + 12 = one launch per reflector (the default above); + 16 = the one-XCD launch is started with a role
 * missing, so that its bounded spins run out (the time-out path: the launches must take over).  Every call also forgets
 * that a persistent launch ever gave up.  DESIGN.md 4.5 */
int thip_test_eig_force(int engine);

/* TEST HOOK: installs a stand-in "collective" that does no arithmetic (the sum over ONE rank) and only takes time: a
 * device spin of latency_us microseconds on the stream the hook is given.  Lets a 1-GPU box measure what each overlap
 * mode hides of a collective's latency (tests/test_gpu_sharded.py). */
int thip_test_spin_allreduce(thip_solver *s, int latency_us);

/* TEST HOOK: kind 1 = the placement census of the next plan (thip_solver_init) reports a bad placement; kind 2 = one
 * workgroup of the after_sweeps-th regular sweep from now withholds its partial dots (once: a transient -- thip_solver_run
 * restores, re-arms and goes on with the one-pass schedule); kind 7 = the same in EVERY sweep from then on (a placement that
 * stays wrong: the second failure hands over to the 2-pass schedule); spin_max > 0 shortens the
 * bound of the gathers' polling loops (default ~2 s) so that a test does not wait for it.  kind 0 clears.
 * kind 3 / 4 (no fault): run the two m-kernels of a step as two launches also where the cones are all element-wise
 * (the form problems with block cones always take) / merged again -- lets a test compare the two forms.
 * kind 5 / 6 (no fault): launch the termination test after every sweep / fold it into the next step's m-kernel again
 * (the default where the m-tail is one of the merged forms: it is launched only when the host is about to look). */
int thip_test_sweep_fault(thip_solver *s, int kind, int64_t after_sweeps, int spin_max);

/* TEST HOOK (SYNC): the Kahan terms of the current iterate (thip_param.state_arith; zeros under THIP_STATE_PLAIN), n floats for
 * x_x and u, m floats for x_y, x_s and v, any pointer may be NULL -- so that a test can check a compensated update bit for bit
 * from the outside -- and the form of the m-tail the last one-pass step launched: 0 none yet, 1 merged (element-wise cones), 2 a
 * wave per cone, 3 three launches; + 4 where the row kernels ran one thread per row (a tiled sparse A with few slices). */
int thip_test_solver_kahan(thip_solver *s, float *host_kx, float *host_ky, float *host_ks, float *host_ku, float *host_kv,
                           int *host_mtail_form);

/* test entry point of the one-pass kernel (thip_sweep.hip): one sweep over the m x n matrix A (device, column-major),
 *   gT = A^T v ; g3 = A^T xy ; u <- u + Su o (-(gP - 2 g3) - c rtau) unless `first` ; gP <- g3 ;
 *   xx_out = xx_in + Tx o (gT + c kappa) ; hN = A u ; h3 = A xx_out            (Kahan terms ku / kx_* may be NULL)
 * `reps` launches are timed with HIP events (reps > 1 only with first != 0, which is idempotent); host_info (8 ints):
 * [0] = the kernel's error word (0 = ok), [1] = members per group, [2] = groups, [3] = panels per group, [4] = 16-byte
 * slots per streaming thread, [5] = polls of all gathers that found a granule missing (summed over workgroups and launches),
 * [6] = the most polls any one gather needed.  force_members > 0: that many workgroups per column group instead of the planner's choice
 * (a power of two the rows fit); pub_agent != 0: partial dots published with agent-scope (sc1) stores.  host_info[7] = columns per
 * panel.
 * pin_g != 0: the EXACT geometry -- pin_w columns per panel (1, 2; 4 for 16-bit elements) and pin_g members per group, whatever the
 * planner would choose, also a group size below the one its few-columns rule raises it to (groups without columns idle); `variant`
 * and `force_members` are then not read.  What the kernel itself needs stays enforced, THIP_E_INVALID with nothing launched: m a
 * multiple of the rows per 16-byte slot (4, 16-bit: 8), lda >= m, n >= 40 pin_w, pin_g a power of two up to 32 whose
 * ceil(m / pin_g) rows fit the slots the (elem, pin_w) family has instances for. */
typedef struct thip_sweep_test {
    size_t m, n, lda;
    const float *mat_a, *v, *xy, *c, *su, *tx;
    float *u, *ku;
    const float *xx_in, *kx_in;
    float *xx_out, *kx_out, *gp, *hn, *h3;
    float kappa, rtau;
    int32_t first, reps;
    int32_t force_members, pub_agent;
    int32_t variant, elem;          /* variant: columns per panel -- f32: 0 = one, 12 = two; 16-bit elem: 1, 2, 4 (0 = the planner's
                                     * preference).  elem: THIP_A_F32, or THIP_A_BF16 / THIP_A_F16: mat_a then points at 16-bit entries, lda in entries */
    const float *inv_s;             /* THIP_A_F16: 1 / scale per column (thip_to_f16), else NULL */
    float *host_sums;               /* optional, 4 floats on the HOST: the sums over n the sweep leaves for the criteria and the scalar
                                     * updates (tau taken as 1): ||c + A^T xy||^2, c.xx_in, c.u, c.(xx_in - 2 xx_out) */
    int32_t pin_w, pin_g;           /* pin_g != 0: exactly this geometry (above) */
} thip_sweep_test;
int thip_test_sweep(const thip_sweep_test *t, float *host_ms, int *host_info);

/* One geometry of the one-pass kernel: members (workgroups) per column group, groups (members x ngroups = 256), rows per member,
 * columns per group, panels per group, 16-byte slots per streaming thread, columns per panel, the element kind; the padded length of
 * a group's share of an N product in floats, and the 8-byte words of the granule ring. */
typedef struct thip_sweep_plan_rec {
    int32_t members, ngroups, rows_per_member, cols_per_group, npan, nslot, cols_per_panel, elem;
    size_t mpad, gran_words;
} thip_sweep_plan_rec;

/* The planning of the one-pass kernel with nothing launched (needs no GPU and no thip_init; a device of 256 CUs is assumed): the
 * geometry for an m x n matrix of `elem` with leading dimension lda at cols_per_panel columns per panel -- force_members = 0: the
 * smallest group size the rows fit times gmul (1, 2, 4, 8), raised by the few-columns rule, as the solver's candidates are made;
 * force_members > 0: exactly that group size, as thip_sweep_test.pin_g (gmul is not read).  THIP_E_INVALID where the kernel has no
 * instance for it.  host_candidates (room for 6) / host_n_candidates: the geometries the solver's plan autotune would time on this
 * matrix, in its order -- thip_test_solver_pin_sweep_plan takes an index into this list.  Any pointer may be NULL. */
int thip_test_sweep_plan(size_t m, size_t n, size_t lda, int elem, int cols_per_panel, int gmul, int force_members,
                         thip_sweep_plan_rec *host_plan, thip_sweep_plan_rec *host_candidates, int *host_n_candidates);

/* TEST HOOK: pins the geometry of the one-pass kernel for the stored form of A in use to the candidate_index-th of the geometries
 * the plan autotune would time on this matrix (thip_test_sweep_plan lists them), installed the way the autotune installs its pick but
 * without a timing sweep and without the slower-than-the-carried-schedule safety net; -1: back to the library's choice.  After
 * thip_solver_init, before the first run.  thip_solver_sweep_plan reports the pinned geometry.  THIP_E_INVALID, the solver left as
 * it was: an index the matrix does not offer, or a solver the one-pass kernel does not run for. */
int thip_test_solver_pin_sweep_plan(thip_solver *s, int candidate_index);

/* test entry point for the matrix-core GEMM of the PSD projection chain: C = alpha * A * B + beta * D + gamma * I_n
 * with A symmetric and B arbitrary, all ld x ld column-major, ld a multiple of 64, zero padded beyond n */
int thip_test_gemm_sym(int n, int ld, float alpha, const float *A, const float *B, float beta, const float *D,
                       float gamma, float *C);
/* the same for either shape and either kernel of the chain, nb matrices per launch (item i at offset i * ld * ld of every
 * operand).  shape 0: C = alpha * X^T * Y + beta * D + gamma * I_n, for operands whose result is symmetric (X = Y, or
 * both symmetric and commuting) -- only the lower triangle of tiles is computed, the rest mirrored; shape 1 =
 * thip_test_gemm_sym (X symmetric, Y general).  kernel 0: the library's choice; 1: one 32 x 32 tile per workgroup;
 * 2: 32 x 64 blocks (what the library picks when a launch has more tiles than the device has CUs) */
int thip_test_gemm_chain(int shape, int kernel, int n, int ld, int nb, float alpha, const float *X, const float *Y,
                         float beta, const float *D, float gamma, float *C);
/* test entry point for the all-symmetric products of the round-5 chain: O_p = alpha_p * A * B_p + beta_p * B_p + gamma_p * I_n
 * for A, B_p symmetric ld x ld (ld a multiple of 64 up to 512, nb items ld * ld apart), computed on the lower triangle of
 * 32 x 32 tiles and mirrored; with dsym_p != 0 the diagonal tiles are averaged with their transpose.  coef = { alpha0, beta0,
 * gamma0, dsym0, alpha1, beta1, gamma1, dsym1 }; B1 == NULL: one product.  kernel 0: the two-product kernel with the
 * library's tiles-per-workgroup; 1..3: that number forced; 4 / 5: the one-tile / 32 x 64 block kernels (one product) */
int thip_test_gemm_dual(int kernel, int n, int ld, int nb, const float *A, const float *B0, const float *B1, const float *coef,
                        float *O0, float *O1);
/* timing probe of the chain's launch shapes (tools/psd_chain_probe.py): `reps` dependent launches of ld x ld products,
 * *host_us = microseconds per launch.  mode 0 / 1: 32 x 64 blocks, batch of two, symmetric / general result; 2: one tile
 * per workgroup, symmetric, batch of two; 3: the same, one item; 4: mode 3 on two streams at once (per launch PAIR);
 * 5: one tile per workgroup, general, one item; 6-8: the two-product kernel (two products / one with averaged diagonal tiles /
 * one with the packed output); 9: mode 0 with averaged diagonal tiles */
int thip_test_chain_probe(int mode, int ld, int reps, float *host_us);
/* timing probe of the tiled sparse products (tools/sptile_rate.py): `reps` launches each of A^T [y0 y1] and A [x0 x1] on `mat`
 * (vectors of ones, two right-hand sides as in the one-pass recurrence); host_ms[0] / [1] = best milliseconds per launch of the
 * T / N product, host_ms[2] / [3] their averages */
int thip_test_sptile_time(thip_sptile *mat, int reps, float *host_ms);
/* TEST HOOK (SYNC): downloads two tiled sparse objects and compares every part, in this order: 1 dimensions and nnz; 2 nnz_pad, nidx,
 * ndense, max_visit; 3 headN and headT; 4 slN, slT and the item counts; 5 tiles; 6 order; 7 itemsN and itemsT; 8 rexp and cexp;
 * 9 idx; 10 vals, bit for bit.  *host_first_difference = 0 when the objects are equal, else the number of the first differing part. */
int thip_test_sptile_equal(const thip_sptile *a, const thip_sptile *b, int *host_first_difference);

/* test entry point of the multi-vector dual GEMV (thip_gemv_multi.hip; tests/test_gpu_batch.py, tools/batch_rate.py): ONE launch of
 * the m x n matrix `mat` (device, column-major, lda = m; streamed from a zero-padded copy when m % 16 != 0, as the batch object does)
 * against nv = 2 .. 8 pairs, its partial sums finished into out_n[i] = A xn[i] (m) and out_t[i] = A^T xt[i] (n).  The four host arrays
 * hold nv DEVICE pointers.  host_stopped[i] != 0 (may be NULL): slot i's stop flag is set -- its outputs are left as they are.
 * nj / target_blocks > 0 pin the tiling (0: the shape heuristic).  nv = 1 runs the single-vector dual_gemv_k the same way (the
 * yardstick).  The launch is repeated `reps` times; *host_ms = the best time of one launch (HIP events). */
int thip_test_gemv_multi(size_t m, size_t n, const float *mat, int nv, const float *const *host_xn, const float *const *host_xt,
                         float *const *host_out_n, float *const *host_out_t, const int *host_stopped, int nj, int target_blocks,
                         int reps, float *host_ms);

/* The plan one launch of the single-vector dual GEMV ran (or would run) under: rows per load (4: f32, 8: 16-bit, 1: the unaligned
 * fallback), row groups per lane, columns per unrolled step, the grid (row tiles x column chunks), columns per chunk, and the form
 * of the partial last row tile: m_load > 0 = unguarded whole-vector loads of rows below m_load, 0 = the per-lane guarded form.  A call
 * split at a column reports the chunk rows and chunk widths of the two launches (chunks / chunks2, cols_per_chunk / cols_per_chunk2). */
typedef struct thip_gemv_plan_rec {
    int32_t vw, nj, ku, tiles, chunks, cols_per_chunk, m_load;
    int32_t chunks2, cols_per_chunk2, reserved;
} thip_gemv_plan_rec;

#define THIP_TEST_E_GUARD 10901   /* thip_test_dual_gemv, thip_test_dual_gemv_multi: a word behind the partial-sum scratch changed */

/* test entry point of the single-vector dual GEMV (thip_gemv.hip; tests/test_gpu_gemv_tilings.py): ONE pinned instance of the kernel
 * alone, its partial sums finished into out_n = A xn (m floats) and / or out_t = A^T xt (n floats), all on the device.
 *   mat, lda, kind, inv_scale, pad_zero: the stored matrix exactly as it lies in device memory -- column-major, lda >= m in elements
 *     of `kind` (THIP_A_F32 / THIP_A_BF16 / THIP_A_F16; F16 with its n per-column 1 / scale); pad_zero != 0 promises that the rows
 *     m .. lda - 1 are zeros (the library's own copies), which lets a partial last row tile load whole vectors;
 *   do_n / do_t: the products to compute (both: from one read of A); abs_mode: |A| times ones (xn / xt not read);
 *   nj, target_blocks >= 0: the tiling hint, any values (0 / 0: none -- the shape heuristic);
 *   col_split: 0 = one launch over all columns; else a multiple of 8 below n: two launches over [0, c) and [c, n) that fill consecutive
 *     chunk rows of the partial sums, as the column-split pipeline of the solver issues them;
 *   stopped != 0: the device stop flag is set -- the kernels and the second stage return at once, the outputs stay as given.
 * The partial sums go to a scratch of the solver's own size filled with NaNs beforehand (a sum that is consumed but was never written
 * shows in the result) with a guard tail behind it: THIP_TEST_E_GUARD when the tail changed.  THIP_E_INVALID, nothing launched: lda < m,
 * a null vector a product needs, f16 without scales, a bad col_split.  *host_plan (may be NULL): the plan that ran. */
typedef struct thip_gemv_test {
    size_t m, n, lda;
    const void *mat;
    const float *inv_scale;
    int32_t kind, pad_zero;
    const float *xn, *xt;
    float *out_n, *out_t;
    int32_t do_n, do_t, abs_mode, nj, target_blocks, stopped;
    size_t col_split;
} thip_gemv_test;
int thip_test_dual_gemv(const thip_gemv_test *t, thip_gemv_plan_rec *host_plan);

/* the same planning with nothing launched (needs no GPU and no thip_init): the plan of one launch over the columns [col0, col1) of an
 * m x n matrix read vw = 4, 8 or 1 rows per load under the hint (nj, target_blocks), the floats dual_gemv_scratch_floats(m, n) reserves
 * for any plan's partial sums (a solver allocates twice that), and the column at which the solver's column-split pipeline splits n
 * columns (0: it does not).  m_load is that of a matrix whose rows below m are not known to be zeros. */
int thip_test_gemv_plan(size_t m, size_t n, int vw, int nj, int target_blocks, size_t col0, size_t col1,
                        thip_gemv_plan_rec *host_plan, size_t *host_scratch_floats, size_t *host_split_col);

/* The planning of the multi-vector dual GEMV with nothing launched (needs no GPU and no thip_init): the plan the kernel instance
 * NV = `instance` (2, 4 or 8) runs an m x n matrix under with the hint (nj, target_blocks) (0 / 0: none) -- vw = 4, nj (1 on NV = 8
 * whatever the hint), ku = 8 / nj, tiles, chunks, cols_per_chunk, m_load = m rounded up to 4 -- and the floats
 * dual_gemv_multi_scratch_floats(m, n) reserves per slot for any plan's partial sums.  THIP_E_INVALID: m or n = 0, an instance other
 * than 2, 4, 8, a negative hint.  Either pointer may be NULL. */
int thip_test_gemv_multi_plan(size_t m, size_t n, int instance, int nj, int target_blocks, thip_gemv_plan_rec *host_plan,
                              size_t *host_scratch_floats);

/* test entry point of the multi-vector dual GEMV (thip_gemv_multi.hip; tests/test_gpu_gemv_multi_tilings.py), the analogue of
 * thip_test_dual_gemv: ONE pinned launch alone, its partial sums finished into out_n[i] = A xn[i] (m floats) and out_t[i] = A^T xt[i]
 * (n floats) for the slots i < nv that are not stopped.
 *   mat: device, column-major, lda = m, 16-byte aligned; streamed from a zero-padded copy when m % 16 != 0, exactly as the batch does;
 *   nv = 2 .. 8; xn, xt, out_n, out_t: HOST arrays of nv DEVICE pointers; stopped (may be NULL): nv flags on the host -- slot i's stop
 *     flag is set, its outputs are left as they are (all set: the kernel returns at entry);
 *   nj, target_blocks >= 0: the tiling hint, any values (0 / 0: none -- the shape heuristic).
 * Every slot's scratch has the batch's own size (the larger of the single-vector and the multi-vector scratch), is filled with NaNs
 * beforehand (a sum that is consumed but was never written shows in the result) and has a guard tail behind it: THIP_TEST_E_GUARD when
 * a tail changed; the padded copy has a tile of NaNs behind it.  THIP_E_INVALID, nothing launched: nv outside 2 .. 8, a null pointer, m or n = 0, a negative hint, a misaligned mat,
 * more column chunks than a launch takes.  *host_plan (may be NULL): the plan that ran (zeros: nothing ran). */
typedef struct thip_gemv_multi_test {
    size_t m, n;
    const float *mat;
    int32_t nv, nj, target_blocks, reserved;
    const float *const *xn, *const *xt;
    float *const *out_n, *const *out_t;
    const int32_t *stopped;
} thip_gemv_multi_test;
int thip_test_dual_gemv_multi(const thip_gemv_multi_test *t, thip_gemv_plan_rec *host_plan);

/* TEST HOOK: pins the tiling of the multi-vector kernel instance NV = `instance` (2, 4 or 8) of a batch to the candidate_index-th of
 * the plans its autotune times (gemv_multi_candidates), as if the autotune had picked it; -1: back to untuned (the shape heuristic).
 * After thip_batch_init, before the first run.  THIP_E_INVALID: an index out of range, or a candidate with two row groups per lane for
 * NV = 8, which the autotune never picks. */
int thip_test_batch_pin_multi_plan(thip_batch *b, int instance, int candidate_index);

/* TEST HOOK: the plan the most recent multi-vector launch of the kernel instance NV = `instance` of this batch ran under (zeros: that
 * instance has not been launched). */
int thip_test_batch_last_multi_plan(const thip_batch *b, int instance, thip_gemv_plan_rec *host_plan);

/* TEST HOOK: pins the tiling of the dual GEMV for the stored form of A and the launch form (one launch per pass, or the column-split
 * pipeline) the next thip_solver_run will use to the candidate_index-th of the plans the autotune times, as if the autotune had picked
 * it; -1: back to the shape heuristic.  After thip_solver_init, before the first run.  THIP_E_INVALID: an index out of range. */
int thip_test_solver_pin_gemv_plan(thip_solver *s, int candidate_index);

/* TEST HOOK: the workgroup size of a small batch (thip_smallbatch.hip): 64, 256 or 1024 threads, 0 = by shape.  Before
 * thip_smallbatch_init. */
int thip_test_smallbatch_force_threads(thip_smallbatch *h, int threads);

/* TEST HOOK: the workgroup size of a mid batch (thip_midbatch.hip): 256 or 1024 threads, 0 = by shape.  Before
 * thip_midbatch_init. */
int thip_test_midbatch_force_threads(thip_midbatch *h, int threads);

/* TEST HOOK: the workgroup size of a mid16 batch (thip_mid16batch.hip): 256 or 1024 threads, 0 = by shape.  Before
 * thip_mid16batch_init. */
int thip_test_mid16batch_force_threads(thip_mid16batch *h, int threads);

/* TEST HOOK: the workgroup size of an SDP batch (thip_sdpbatch.hip): 256 or 1024 threads, 0 = by shape.  Before
 * thip_sdpbatch_init. */
int thip_test_sdpbatch_force_threads(thip_sdpbatch *h, int threads);

/* TEST HOOK: the workgroup size of a wide batch (thip_widebatch.hip): 256 or 1024 threads, 0 = by shape.  Before
 * thip_widebatch_init. */
int thip_test_widebatch_force_threads(thip_widebatch *h, int threads);

/* TEST HOOK: the workgroup size of a wide16 batch (thip_wide16batch.hip): 256 or 1024 threads, 0 = by shape.  Before
 * thip_wide16batch_init. */
int thip_test_wide16batch_force_threads(thip_wide16batch *h, int threads);

/* TEST HOOK: the SDP batch kernel's own PSD projection alone: `count` packed matrices of order k (1 .. 64; k (k + 1) / 2 floats each,
 * one after another at dev_packed, off-diagonals times sqrt 2) are projected in place, one workgroup each, in ONE launch;
 * dev_rx_or_null != NULL: rx <- rx - 2 x of the same layout rides in the pack. */
int thip_test_sdpbatch_project(int k, int count, float *dev_packed, float *dev_rx_or_null);

/* TEST HOOK: the same projection in the forms the own-A batches run it in (same contract as thip_test_sdpbatch_project), from a
 * kernel compiled for 1024-thread workgroups as the iteration kernels are.  threads: 256 or 1024.  in_lds 0: on the device arrays
 * themselves (the wide batches: the vectors lie in the arena); 1: the workgroup copies its matrix (and rx) into LDS behind the
 * operands, projects there (the other batches: every vector in LDS) and copies the result back.  Anything else is refused. */
int thip_test_sdpbatch_project_form(int k, int count, int threads, int in_lds, float *dev_packed, float *dev_rx_or_null);

/* TEST HOOK: the workgroup size of a ragged batch (thip_raggedbatch.hip): 256 or 1024 threads put every problem in that one
 * class, 0 = by shape.  Before thip_raggedbatch_init. */
int thip_test_raggedbatch_force_threads(thip_raggedbatch *h, int threads);

/* TEST HOOK: the launch plan thip_raggedbatch_create would make (needs no device), for the arrays of thip_raggedbatch_fits and a
 * forced workgroup size (0: by shape).  host_class[p]: 0 (256 threads) or 1 (1024); host_order: the 256-thread class's members
 * in the order of its live list, then the 1024-thread class's; host_layout[p]: the index of problem p's cone table;
 * host_arena_at[p]: where its state starts in the arena, in floats -- n_prob entries each, any may be NULL.  host_info: the
 * counts, the classes' thread counts and LDS bytes, n_layouts, arena_bytes and a_bytes_per_iter (NULL: not wanted). */
int thip_test_raggedbatch_plan(size_t n_prob, const size_t *host_n, const size_t *host_m, const size_t *host_n_seg,
                               const int32_t *host_seg_type, const int64_t *host_seg_len, int force_threads, int *host_class,
                               int *host_order, int *host_layout, int64_t *host_arena_at, thip_raggedbatch_info_t *host_info);

/* TEST HOOK: the workgroup size of a sparse batch (thip_sparsebatch.hip): 256 or 1024 threads, 0 = by shape.  Before
 * thip_sparsebatch_init. */
int thip_test_sparsebatch_force_threads(thip_sparsebatch *h, int threads);

/* TEST HOOK: where a sparse batch reads its blobs: 0 from memory (streamed), 1 from LDS (resident; THIP_E_INVALID when the blob does
 * not fit beside the vectors).  Before thip_sparsebatch_init. */
int thip_test_sparsebatch_force_resident(thip_sparsebatch *h, int resident);

/* TEST HOOK: slot i's blob as it lies on the device (what thip_sparsebatch_create / _replace packed, or thip_sparsebatch_set_a
 * scattered new values into): host_used_words receives the words it uses; host_words (may be NULL): cap_words words to receive them.
 * THIP_E_INVALID: a null handle, no such problem, fewer words offered than used. */
int thip_test_sparsebatch_blob(thip_sparsebatch *h, int i, uint32_t *host_words, size_t cap_words, size_t *host_used_words);

/* TEST HOOK: the blob thip_sparsebatch_create would store for one problem given as host CSC arrays (needs no device), with every
 * refusal of the stored form (nnz_cap: 0 = m n).  host_used_words: the words the blob uses; host_words (may be NULL): cap_words words
 * to receive them; host_long (may be NULL): the row length above which a row is summed by a wave. */
int thip_test_sparsebatch_pack(size_t n, size_t m, const int64_t *host_colptr, const int32_t *host_rowidx, const float *host_values,
                               size_t nnz_cap, uint32_t *host_words, size_t cap_words, size_t *host_used_words, int *host_long);

/* TEST HOOK: the workgroup size of a ragged sparse batch (thip_raggedsparse.hip): 256 or 1024 threads put every problem in that one
 * class, 0 = by the sparse batch's rule.  Before thip_raggedsparse_init. */
int thip_test_raggedsparse_force_threads(thip_raggedsparse *h, int threads);

/* TEST HOOK: thip_test_sparsebatch_blob for a ragged sparse batch. */
int thip_test_raggedsparse_blob(thip_raggedsparse *h, int i, uint32_t *host_words, size_t cap_words, size_t *host_used_words);

/* TEST HOOK: who of a ragged sparse batch reads its blob from LDS: 0 nobody, 1 everybody who fits (the rule).  Before
 * thip_raggedsparse_init. */
int thip_test_raggedsparse_force_resident(thip_raggedsparse *h, int resident);

/* TEST HOOK: the plan thip_raggedsparse_create would make (needs no device) for problems of host_nnz[p] entries (NULL: the
 * capacities) in slots of host_nnz_cap[p] (NULL or 0: the own count), a forced workgroup size (0: by the rule) and a forced residency
 * (-1: the rule, 0, 1).  host_class[p]: 0 (256 threads) or 1 (1024); host_order: the 256-thread class's members in the order of its
 * live list, then the 1024-thread class's; host_layout[p]: the index of problem p's cone table; host_arena_at[p]: where its state
 * starts in the arena, in floats; host_blob_at[p]: where its blob starts, in bytes; host_lds_at[p]: where the resident copy lies in
 * LDS, in floats; host_resident[p] -- n_prob entries each, any may be NULL.  host_info: the part of info() that needs no device
 * (NULL: not wanted). */
int thip_test_raggedsparse_plan(size_t n_prob, const size_t *host_n, const size_t *host_m, const size_t *host_nnz,
                                const size_t *host_nnz_cap, const size_t *host_n_seg, const int32_t *host_seg_type,
                                const int64_t *host_seg_len, int force_threads, int force_resident, int *host_class, int *host_order,
                                int *host_layout, int64_t *host_arena_at, int64_t *host_blob_at, int *host_lds_at, int *host_resident,
                                thip_raggedsparse_info_t *host_info);

/* TEST HOOKS of the round calls on device memory (thip_NAME_set_bc_dev ..; h: a handle of any own-A batch family).
 * _addresses reports ADDRESSES ONLY: host_addr[0 .. 2], host_bytes[0 .. 2] <- where the handle's arena, its device staging buffer
 * and its b / c store lie and how many bytes each holds (0, 0: not allocated yet).
 * _last_transfer: the bytes the last _dev call on the handle moved host -> device and device -> host (tables, verdict words, status
 * blocks; a call that was refused early leaves zeros).
 * _overlap: 1 when the byte ranges [a, a + a_bytes) and [b, b + b_bytes) share a byte, else 0 -- the rule of the refusals (no device).
 * _offsets: where each problem's part begins in the packed arrays of a range of `count` problems of the shapes host_n, host_m (no
 * device): host_at holds 5 rows of count + 1 entries, in floats -- c / a solution's x (n each), b / row sums / a solution's y (m),
 * an iterate's x (n + 2 m + 1), its y (n + m + 1), a dense A (m n); the last entry of a row is the array's length.
 * _copy_chunk: the floats one workgroup of the dense copy kernel moves */
int thip_test_ownbatch_addresses(void *h, uint64_t *host_addr, uint64_t *host_bytes);
int thip_test_ownbatch_last_transfer(void *h, uint64_t *host_h2d_bytes, uint64_t *host_d2h_bytes);
int thip_test_ownbatch_overlap(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes);
int thip_test_ownbatch_offsets(size_t count, const size_t *host_n, const size_t *host_m, int64_t *host_at);
int thip_test_ownbatch_copy_chunk(void);

#ifdef __cplusplus
}
#endif
#endif /* TOTSU_F32HIP_TEST_H */
