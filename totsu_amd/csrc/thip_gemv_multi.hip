// thip_gemv_multi.hip -- the dual GEMV of thip_gemv.hip against NV pairs of vectors from ONE read of A: for i < nv the partial
// sums of A xn_i (m) and A^T xt_i (n), for a batch of problems that share A (thip_batch, thip_solver_batch.inc).
//
// Same streaming discipline as dual_gemv_k: non-temporal 16-byte loads of the f32 column-major matrix straight into registers
// (no LDS staging of A), per-lane N accumulators over a chunk of columns, the T dots of KU columns reduced across the wave with
// the transpose-reduce butterfly and across the four waves through LDS, a deterministic second stage (post_k / finalize_partials),
// no atomics.  The partial sums of slot i land in ITS scratch in the layout of GemvPartials, so every consumer is unchanged.
//
// What differs is the budget.  Registers per lane: NV * 4 NJ accumulators + NV * 4 NJ entries of xt + 4 NJ KU entries of A in
// flight (+ KU dots of the slot being reduced); the xn values are wave-uniform and stay in SGPRs.  NV = 8 therefore runs one row
// group per lane (NJ = 1: 32 + 32 + 32), NV = 2 and 4 also two (NJ = 2, KU = 4).  VALU: 2 FMAs per loaded entry and slot -- at
// NV = 8 that is 8 flop per byte of A, half the f32 vector rate of the part at 8 TB/s only when the FMAs are the packed ones
// (v_pk_fma_f32), so both products are written on 2-vectors.  LDS: NV * 4 waves * MCW floats, hence MCW = 256 columns per chunk
// (32 KiB at NV = 8).
//
// The matrix must allow whole 16-byte loads of every row group of the last tile: lda % 4 == 0, a 16-byte aligned base, and either
// m % 4 == 0 or rows m .. lda - 1 zeros of the library's own padded copy (DenseA::pad_zero) -- the batch object guarantees it, so
// there is no guarded (scalar-load) form.
#include "thip_common.h"
#include "thip_gemv_reduce.h"

#include <algorithm>
#include <vector>

using namespace thip;

namespace {

constexpr int BLK = 256;
constexpr int MCW = 256;      // max columns per chunk
constexpr int VW = 4;

typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

// One step: K columns of the block's row tile against every live slot.  CLAMP: the partial last row tile -- row group j of this
// lane loads from rofs[j], its own rows where they exist and the tile's first rows where they do not (the stray values meet
// xt = 0 and a guarded store, as in dual_gemv_k)
template <int NV, int NJ, int K, bool CLAMP>
__device__ __forceinline__ void mstep(const float *__restrict__ A, size_t lda, int r_first, int c, int cc, const MultiTab &tab,
                                      unsigned live, const f32x2_t (&xtv)[NV][NJ][2], f32x2_t (&accN)[NV][NJ][2],
                                      float *ldsT_wave, int lane, const int (&rofs)[NJ])
{
    f32x4_t av[K][NJ];
#pragma unroll
    for (int u = 0; u < K; ++u) {
        const float *col = A + (size_t)(c + u) * lda + (CLAMP ? 0 : r_first);
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            av[u][j] = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t *>(col + (CLAMP ? rofs[j] : j * (BLK * VW))));
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (!((live >> i) & 1u)) continue;          // wave-uniform: an unused or stopped slot multiplies nothing
        const float *__restrict__ xn = tab.xn[i];
        float p[K];
#pragma unroll
        for (int u = 0; u < K; ++u) {
            const float xs = xn[c + u];
            const f32x2_t xs2 = { xs, xs };
            f32x2_t s2 = { 0.0f, 0.0f };
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const f32x2_t a2 = { av[u][j][2 * h], av[u][j][2 * h + 1] };
                    accN[i][j][h] = __builtin_elementwise_fma(a2, xs2, accN[i][j][h]);
                    s2 = __builtin_elementwise_fma(a2, xtv[i][j][h], s2);
                }
            p[u] = s2[0] + s2[1];
        }
        const float r = multi_reduce<K>(p, lane);
        constexpr int SH = 6 - Log2<K>::v;
        if ((lane & ((64 >> Log2<K>::v) - 1)) == 0) ldsT_wave[i * (4 * MCW) + cc + (lane >> SH)] = r;
    }
}

template <int NV, int NJ, int KU>
__global__ __launch_bounds__(BLK) void dual_gemv_multi_k(const float *__restrict__ A, size_t lda, int m, int n, MultiTab tab,
                                                         int nv, int nN, size_t strideN, size_t strideT, int cols_per_chunk,
                                                         int m_load)
{
    // the launch runs as long as any instance of its group is live
    unsigned live = 0;
#pragma unroll
    for (int i = 0; i < NV; ++i)
        if (i < nv && (tab.stop[i] == nullptr || *tab.stop[i] == 0)) live |= 1u << i;
    if (live == 0) return;
    __shared__ float ldsT[NV * 4 * MCW];

    constexpr int TILE = BLK * VW * NJ;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tile = blockIdx.x, chunk = blockIdx.y;
    const int r_first = tile * TILE + tid * VW;
    const int c0 = chunk * cols_per_chunk;
    const int c1 = min(n, c0 + cols_per_chunk);

    f32x2_t xtv[NV][NJ][2], accN[NV][NJ][2];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const bool on = (live >> i) & 1u;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r = r_first + j * (BLK * VW) + 2 * h;
                accN[i][j][h] = f32x2_t{ 0.0f, 0.0f };
                xtv[i][j][h] = f32x2_t{ (on && r < m) ? tab.xt[i][r] : 0.0f, (on && r + 1 < m) ? tab.xt[i][r + 1] : 0.0f };
            }
    }

    float *ldsT_wave = ldsT + wave * MCW;
    int rofs[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) rofs[j] = 0;
    int c = c0;
    if ((tile + 1) * TILE <= m) {
        for (; c + KU <= c1; c += KU) mstep<NV, NJ, KU, false>(A, lda, r_first, c, c - c0, tab, live, xtv, accN, ldsT_wave, lane, rofs);
        for (; c < c1; ++c)          mstep<NV, NJ, 1, false>(A, lda, r_first, c, c - c0, tab, live, xtv, accN, ldsT_wave, lane, rofs);
    } else {
        // the partial last tile: m_load = the rows whole vectors may load (m rounded up to 4, never beyond lda)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int r = r_first + j * (BLK * VW);
            rofs[j] = (r + VW <= m_load) ? r : tile * TILE;
        }
        for (; c + KU <= c1; c += KU) mstep<NV, NJ, KU, true>(A, lda, r_first, c, c - c0, tab, live, xtv, accN, ldsT_wave, lane, rofs);
        for (; c < c1; ++c)          mstep<NV, NJ, 1, true>(A, lda, r_first, c, c - c0, tab, live, xtv, accN, ldsT_wave, lane, rofs);
    }

#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (!((live >> i) & 1u)) continue;
        float *dst = tab.scr[i] + (size_t)chunk * strideN;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int r = r_first + j * (BLK * VW);
            if (r + VW <= m) {
                *reinterpret_cast<float4 *>(dst + r) = make_float4(accN[i][j][0][0], accN[i][j][0][1], accN[i][j][1][0], accN[i][j][1][1]);
            } else {
#pragma unroll
                for (int k = 0; k < VW; ++k) if (r + k < m) dst[r + k] = accN[i][j][k >> 1][k & 1];
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (!((live >> i) & 1u)) continue;
        float *dst = tab.scr[i] + (size_t)nN * strideN + (size_t)tile * strideT + c0;
        const float *l = ldsT + i * (4 * MCW);
        for (int t = tid; t < c1 - c0; t += BLK) dst[t] = (l[t] + l[MCW + t]) + (l[2 * MCW + t] + l[3 * MCW + t]);
    }
}

struct MPlan { int nj, tiles, chunks, cpc, m_load; size_t strideN, strideT; };

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The tiling per instance: NV = 8 holds one row group per lane; NV = 2 and 4 take hint.nj = 1 (8 columns in flight) or 2 (4)
MPlan multi_plan(size_t n_row, size_t n_col, int inst, const GemvHint *hint)
{
    MPlan p;
    p.nj = (hint && hint->nj >= 2 && inst < 8) ? 2 : 1;
    const size_t tile = (size_t)BLK * VW * p.nj;
    p.tiles = (int)((n_row + tile - 1) / tile);
    // the grid rule of the single-vector plan (thip_gemv.hip make_plan): 0.2 MB of A per workgroup, 2048 .. 8192 workgroups
    int target_blocks = (int)((double)n_row * (double)n_col * 4.0 / 2.0e5);
    if (target_blocks < 2048) target_blocks = 2048;
    if (target_blocks > 8192) target_blocks = 8192;
    if (hint && hint->target_blocks > 0) target_blocks = hint->target_blocks;
    int chunks = target_blocks / p.tiles;
    if (chunks < 1) chunks = 1;
    int cpc = (int)((n_col + chunks - 1) / chunks);
    const int mincpc = ((double)n_row * (double)n_col * 4.0 < 64.0e6) ? 16 : 32;
    if (cpc < mincpc) cpc = mincpc;
    cpc = (int)round_up(cpc, 8);
    if (cpc > MCW) cpc = MCW;
    p.cpc = cpc;
    p.chunks = (int)((n_col + cpc - 1) / cpc);
    p.strideN = round_up(n_row, 4);
    p.strideT = round_up(n_col, 4);
    p.m_load = (int)round_up(n_row, VW);
    return p;
}

// the plan as the test hooks report it (thip_gemv_plan_rec: rows per load, row groups per lane, columns per unrolled step, the grid)
void multi_plan_record(const MPlan &p, thip_gemv_plan_rec *r)
{
    *r = thip_gemv_plan_rec{};
    r->vw = VW; r->nj = p.nj; r->ku = 8 / p.nj; r->tiles = p.tiles; r->chunks = p.chunks; r->cols_per_chunk = p.cpc;
    r->m_load = p.m_load;
}

bool multi_dims_ok(size_t n_row, size_t n_col) { return n_row <= 0x7fffffffull - 8192 && n_col <= 0x7fffffffull; }

}  // namespace

namespace thip {

int gemv_multi_instance(int nv)
{
    return nv <= 1 ? 1 : (nv <= 2 ? 2 : (nv <= 4 ? 4 : 8));
}

const GemvHint *gemv_multi_candidates(int *count)
{
    static const GemvHint c[] = { {1, 8192}, {1, 4096}, {1, 2048}, {2, 8192}, {2, 4096}, {2, 2048}, {2, 1024} };
    *count = (int)(sizeof(c) / sizeof(c[0]));
    return c;
}

size_t dual_gemv_multi_scratch_floats(size_t n_row, size_t n_col)
{
    size_t best = 0;
    int nc = 0;
    const GemvHint *c = gemv_multi_candidates(&nc);
    for (int inst = 2; inst <= 8; inst *= 4)          // (the NV = 8 instance keeps one row group per lane whatever the hint)
        for (int i = -1; i < nc; ++i) {
            const MPlan p = multi_plan(n_row, n_col, inst, i < 0 ? nullptr : &c[i]);
            const size_t f = (size_t)p.chunks * p.strideN + (size_t)p.tiles * p.strideT;
            if (f > best) best = f;
        }
    return best + 64;
}

int dual_gemv_multi_partials(hipStream_t st, size_t n_row, size_t n_col, const DenseA &A, int nv, const float *const *xn,
                             const float *const *xt, float *const *scratch, size_t scratch_floats, const int *const *stop,
                             GemvPartials *out, const GemvHint *hint, thip_gemv_plan_rec *plan_out)
{
    if (nv < 2 || nv > GEMV_MULTI_MAX) return fail(THIP_E_INVALID, "a multi-vector launch takes 2 .. 8 vector pairs", __FILE__, __LINE__);
    for (int i = 0; i < nv; ++i) out[i] = GemvPartials{};
    if (n_row == 0 || n_col == 0) return 0;
    if (!multi_dims_ok(n_row, n_col)) return fail(THIP_E_INVALID, "matrix dimension > 2^31", __FILE__, __LINE__);
    if (A.kind != THIP_A_F32 || !A.vec_ok() || A.lda < n_row)
        return fail(THIP_E_INVALID, "the multi-vector product streams an f32 matrix with 16-byte aligned columns", __FILE__, __LINE__);
    if (n_row % VW != 0 && !(A.pad_zero && A.lda >= round_up(n_row, VW)))
        return fail(THIP_E_INVALID, "the multi-vector product needs m % 4 == 0 or the library's zero-padded copy", __FILE__, __LINE__);
    const int inst = gemv_multi_instance(nv);
    const MPlan p = multi_plan(n_row, n_col, inst, hint);
    if (p.chunks > 65535) return fail(THIP_E_INVALID, "too many column chunks for one launch", __FILE__, __LINE__);
    const size_t need = (size_t)p.chunks * p.strideN + (size_t)p.tiles * p.strideT;
    if (need > scratch_floats) return fail(THIP_E_WORK, "gemv scratch too small", __FILE__, __LINE__);
    MultiTab tab{};
    for (int i = 0; i < nv; ++i) {
        if (!xn[i] || !xt[i] || !scratch[i]) return fail(THIP_E_INVALID, "null vector in a multi-vector launch", __FILE__, __LINE__);
        tab.xn[i] = xn[i]; tab.xt[i] = xt[i]; tab.scr[i] = scratch[i]; tab.stop[i] = stop ? stop[i] : nullptr;
        out[i].partN = scratch[i]; out[i].nN = p.chunks; out[i].strideN = p.strideN;
        out[i].partT = scratch[i] + (size_t)p.chunks * p.strideN; out[i].nT = p.tiles; out[i].strideT = p.strideT;
    }
    const dim3 g(p.tiles, p.chunks), b(BLK);
    const float *mat = (const float *)A.mat;
    const int m = (int)n_row, n = (int)n_col;
#define THIP_MULTI_LAUNCH(NV, NJ, KU)                                                                                       \
    hipLaunchKernelGGL((dual_gemv_multi_k<NV, NJ, KU>), g, b, 0, st, mat, A.lda, m, n, tab, nv, p.chunks, p.strideN, p.strideT, \
                       p.cpc, p.m_load)
    if (inst == 2) { if (p.nj == 2) THIP_MULTI_LAUNCH(2, 2, 4); else THIP_MULTI_LAUNCH(2, 1, 8); }
    else if (inst == 4) { if (p.nj == 2) THIP_MULTI_LAUNCH(4, 2, 4); else THIP_MULTI_LAUNCH(4, 1, 8); }
    else THIP_MULTI_LAUNCH(8, 1, 8);
#undef THIP_MULTI_LAUNCH
    THIP_LAUNCH_CHECK();
    if (plan_out) multi_plan_record(p, plan_out);
    return 0;
}

}  // namespace thip

extern "C" {

// TEST HOOK (totsu_f32hip_test.h): one multi-vector launch alone, its partial sums finished into the callers' vectors
int thip_test_gemv_multi(size_t m, size_t n, const float *mat, int nv, const float *const *host_xn, const float *const *host_xt,
                         float *const *host_out_n, float *const *host_out_t, const int *host_stopped, int nj, int target_blocks,
                         int reps, float *host_ms)
{
    THIP_NEED_INIT();
    if (!mat || !host_xn || !host_xt || !host_out_n || !host_out_t || nv < 1 || nv > GEMV_MULTI_MAX || m == 0 || n == 0)
        return fail(THIP_E_INVALID, "bad argument", __FILE__, __LINE__);
    hipStream_t st = ctx().stream;
    // the stored form the batch object streams: the caller's matrix, or the zero-padded copy when m is no multiple of 16 floats
    float *pad = nullptr, *scr = nullptr;
    int *flags = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    DenseA A = dense_f32(mat, m);
    const size_t per = round_up(std::max(dual_gemv_multi_scratch_floats(m, n), dual_gemv_scratch_floats(m, n)), 64);
    int rc = 0;
    float best = 1e30f;
    // (one exit: everything allocated here is released whatever fails)
    auto body = [&]() -> int {
        if (m % 16 != 0) {
            const size_t ld = round_up(m, 16);
            THIP_TRY(hipMalloc((void **)&pad, ld * n * sizeof(float)));
            THIP_TRY(hipMemsetAsync(pad, 0, ld * n * sizeof(float), st));
            THIP_TRY(hipMemcpy2DAsync(pad, ld * sizeof(float), mat, m * sizeof(float), m * sizeof(float), n, hipMemcpyDeviceToDevice, st));
            A = DenseA{ pad, ld, THIP_A_F32, nullptr, true };
        }
        THIP_TRY(hipMalloc((void **)&scr, per * nv * sizeof(float)));
        THIP_TRY(hipMalloc((void **)&flags, GEMV_MULTI_MAX * sizeof(int)));
        int hf[GEMV_MULTI_MAX] = { 0 };
        for (int i = 0; i < nv; ++i) hf[i] = (host_stopped && host_stopped[i]) ? 1 : 0;
        THIP_TRY(hipMemcpyAsync(flags, hf, sizeof(hf), hipMemcpyHostToDevice, st));
        THIP_TRY(hipEventCreate(&e0));
        THIP_TRY(hipEventCreate(&e1));
        float *scrs[GEMV_MULTI_MAX];
        const int *stops[GEMV_MULTI_MAX];
        GemvPartials gp[GEMV_MULTI_MAX];
        for (int i = 0; i < nv; ++i) { scrs[i] = scr + (size_t)i * per; stops[i] = flags + i; }
        const GemvHint hint{ nj, target_blocks };
        const GemvHint *h = (nj > 0 || target_blocks > 0) ? &hint : nullptr;
        for (int rep = 0; rep < (reps > 0 ? reps : 1); ++rep) {
            THIP_TRY(hipEventRecord(e0, st));
            if (nv == 1) THIP_RC(dual_gemv_partials(st, m, n, A, host_xn[0], host_xt[0], true, true, false, scrs[0], per, &gp[0], stops[0], h));
            else THIP_RC(dual_gemv_multi_partials(st, m, n, A, nv, host_xn, host_xt, scrs, per, stops, gp, h));
            THIP_TRY(hipEventRecord(e1, st));
            THIP_TRY(hipEventSynchronize(e1));
            float t = 0.0f;
            THIP_TRY(hipEventElapsedTime(&t, e0, e1));
            if (t < best) best = t;
        }
        for (int i = 0; i < nv; ++i) {
            if (hf[i]) continue;          // a stopped slot leaves no sums: its outputs stay as they are
            THIP_RC(finalize_partials(st, m, gp[i].partN, gp[i].nN, gp[i].strideN, 1.0f, 0.0f, host_out_n[i], nullptr));
            THIP_RC(finalize_partials(st, n, gp[i].partT, gp[i].nT, gp[i].strideT, 1.0f, 0.0f, host_out_t[i], nullptr));
        }
        THIP_TRY(hipStreamSynchronize(st));
        return 0;
    };
    rc = body();
    if (rc != 0) hipStreamSynchronize(st);
    if (e0) hipEventDestroy(e0);
    if (e1) hipEventDestroy(e1);
    hipFree(pad); hipFree(scr); hipFree(flags);
    if (host_ms) *host_ms = best;
    return rc;
}

// TEST HOOK (totsu_f32hip_test.h): the planning of the multi-vector kernel with nothing launched
int thip_test_gemv_multi_plan(size_t m, size_t n, int instance, int nj, int target_blocks, thip_gemv_plan_rec *host_plan,
                              size_t *host_scratch_floats)
{
    if (m == 0 || n == 0 || !multi_dims_ok(m, n) || !(instance == 2 || instance == 4 || instance == 8) || nj < 0 || target_blocks < 0)
        return fail(THIP_E_INVALID, "bad argument", __FILE__, __LINE__);
    const GemvHint hint{ nj, target_blocks };
    const MPlan p = multi_plan(m, n, instance, (nj > 0 || target_blocks > 0) ? &hint : nullptr);
    if (host_plan) multi_plan_record(p, host_plan);
    if (host_scratch_floats) *host_scratch_floats = dual_gemv_multi_scratch_floats(m, n);
    return 0;
}

// TEST HOOK (totsu_f32hip_test.h): one pinned launch of the multi-vector kernel alone, every slot's scratch the batch's own size,
// NaNs beforehand and a guard tail behind it
int thip_test_dual_gemv_multi(const thip_gemv_multi_test *t, thip_gemv_plan_rec *host_plan)
{
    THIP_NEED_INIT();
    if (host_plan) *host_plan = thip_gemv_plan_rec{};
    if (!t || !t->mat || !t->xn || !t->xt || !t->out_n || !t->out_t || t->nv < 2 || t->nv > GEMV_MULTI_MAX || t->m == 0 || t->n == 0
        || !multi_dims_ok(t->m, t->n) || t->nj < 0 || t->target_blocks < 0 || ((uintptr_t)t->mat & 15u) != 0)
        return fail(THIP_E_INVALID, "bad argument", __FILE__, __LINE__);
    const int nv = t->nv;
    for (int i = 0; i < nv; ++i)
        if (!t->xn[i] || !t->xt[i] || !t->out_n[i] || !t->out_t[i])
            return fail(THIP_E_INVALID, "null vector in a multi-vector launch", __FILE__, __LINE__);
    const size_t m = t->m, n = t->n;
    const GemvHint hint{ t->nj, t->target_blocks };
    const GemvHint *h = (t->nj > 0 || t->target_blocks > 0) ? &hint : nullptr;
    // the batch's own allocation per slot (batch_create_impl) -- what the launch is about to need is refused here, not after it
    const size_t per = std::max(dual_gemv_scratch_floats(m, n), dual_gemv_multi_scratch_floats(m, n));
    {
        const MPlan p = multi_plan(m, n, gemv_multi_instance(nv), h);
        if (p.chunks > 65535) return fail(THIP_E_INVALID, "too many column chunks for one launch", __FILE__, __LINE__);
        if ((size_t)p.chunks * p.strideN + (size_t)p.tiles * p.strideT > per) return fail(THIP_E_WORK, "gemv scratch too small", __FILE__, __LINE__);
    }
    constexpr size_t GUARD = 256, PAD_TAIL = 2 * BLK * VW;
    constexpr unsigned NAN_WORD = 0x7fc00abcu, GUARD_WORD = 0x5a5a5a5au;
    const size_t slot = round_up(per, 4) + GUARD;          // [0, per) the scratch, [per, slot) its guard tail
    hipStream_t st = ctx().stream;
    float *pad = nullptr, *scr = nullptr;
    int *flags = nullptr;
    DenseA A = dense_f32(t->mat, m);
    thip_gemv_plan_rec rec{};
    // (one exit: everything allocated here is released whatever fails)
    auto body = [&]() -> int {
        if (m % 16 != 0) {
            // the stored form the batch object streams, with a tile of NaNs behind it: a load that strays past the copy stays inside
            // this allocation and shows in the result
            const size_t ld = round_up(m, 16);
            THIP_TRY(hipMalloc((void **)&pad, (ld * n + PAD_TAIL) * sizeof(float)));
            THIP_TRY(hipMemsetAsync(pad, 0, ld * n * sizeof(float), st));
            THIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(pad + ld * n), (int)NAN_WORD, PAD_TAIL, st));
            THIP_TRY(hipMemcpy2DAsync(pad, ld * sizeof(float), t->mat, m * sizeof(float), m * sizeof(float), n, hipMemcpyDeviceToDevice, st));
            A = DenseA{ pad, ld, THIP_A_F32, nullptr, true };
        }
        THIP_TRY(hipMalloc((void **)&scr, slot * nv * sizeof(float)));
        THIP_TRY(hipMalloc((void **)&flags, GEMV_MULTI_MAX * sizeof(int)));
        int hf[GEMV_MULTI_MAX] = { 0 };
        float *scrs[GEMV_MULTI_MAX];
        const int *stops[GEMV_MULTI_MAX];
        GemvPartials gp[GEMV_MULTI_MAX];
        for (int i = 0; i < nv; ++i) {
            hf[i] = (t->stopped && t->stopped[i]) ? 1 : 0;
            scrs[i] = scr + (size_t)i * slot; stops[i] = flags + i;
            THIP_TRY(hipMemsetD32Async((hipDeviceptr_t)scrs[i], (int)NAN_WORD, per, st));
            THIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(scrs[i] + per), (int)GUARD_WORD, slot - per, st));
        }
        THIP_TRY(hipMemcpyAsync(flags, hf, sizeof(hf), hipMemcpyHostToDevice, st));
        THIP_RC(dual_gemv_multi_partials(st, m, n, A, nv, t->xn, t->xt, scrs, per, stops, gp, h, &rec));
        for (int i = 0; i < nv; ++i) {
            if (hf[i]) continue;          // a stopped slot leaves no sums: its outputs stay as they are
            THIP_RC(finalize_partials(st, m, gp[i].partN, gp[i].nN, gp[i].strideN, 1.0f, 0.0f, t->out_n[i], nullptr));
            THIP_RC(finalize_partials(st, n, gp[i].partT, gp[i].nT, gp[i].strideT, 1.0f, 0.0f, t->out_t[i], nullptr));
        }
        std::vector<unsigned> tail((slot - per) * nv);
        for (int i = 0; i < nv; ++i)
            THIP_TRY(hipMemcpyAsync(tail.data() + (size_t)i * (slot - per), scrs[i] + per, (slot - per) * sizeof(unsigned),
                                    hipMemcpyDeviceToHost, st));
        THIP_TRY(hipStreamSynchronize(st));
        for (unsigned w : tail)
            if (w != GUARD_WORD) return fail(THIP_TEST_E_GUARD, "a launch wrote behind a slot's gemv scratch", __FILE__, __LINE__);
        return 0;
    };
    const int rc = body();
    if (rc != 0) hipStreamSynchronize(st);
    hipFree(pad); hipFree(scr); hipFree(flags);
    if (host_plan) *host_plan = rec;
    return rc;
}

}  // extern "C"
