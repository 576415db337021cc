// thip_smallbatch.hip -- thip_smallbatch: many small conic programs, each with its OWN dense f32 A (shared n, m and cone layout), iterated on
// chip.  A launch of smallbatch_k gives one workgroup to each live problem: the workgroup loads its A into LDS (m n <= 24 576 floats
// = 96 KiB of the CU's 160 KiB), its state from the problem's arena, runs up to `steps` iterations of the reference's loop
// (solver.rs:340-458; oracle/totsu_oracle.c core_solve) with no launch boundary inside an iteration, and writes the state back.
//
// Recurrence: the 3-pass ("fused") one -- A u / A^T v, A rx_x / A^T rx_y, A x_x / A^T x_y, each pair from LDS.  A pass over an
// LDS-resident A is a few hundred cycles, so the carried form's saved pass is not worth its two extra state vectors and its second
// rounding of K rx.  The element-wise arithmetic is that of xupdate_k / ycrit_k / status_eval (thip_solver_kernels.inc) and of
// soc_k / group_min_k (thip_cone.hip).
//
// LDS: A with leading dimension lda = m | 1 (odd): the row walk of A x has consecutive lanes on consecutive words, the column walk of
// A^T y has consecutive lanes lda words apart -- an odd stride visits every bank once.  Behind A: every vector of the iteration.
//
// Sums: per-thread fmaf chains, DPP wave sums, then the waves' values through LDS added in wave order (f64).  No atomics: a
// problem's result is a function of (its data, the workgroup size) alone -- not of its index, its neighbours or the launch.
//
// The status block, the slots, the device functions that do not touch A and the host machinery are shared with the streamed
// mid-size batch (thip_midbatch.hip): thip_ownbatch.h.
#include "thip_ownbatch.h"

#include <mutex>

using namespace thip;

namespace {

constexpr size_t SB_MAX_DIM = 1024, SB_MAX_AREA = 24576, SB_LDS_MAX = OB_LDS_MAX;

struct SbArgs {
    int n, m, lda, n_cones, comp, steps;
    int first;                              // live == NULL: workgroup k serves problem first + k
    const int *live;                        // else problem live[k]
    const SbSlot *slots;
    float *arena; size_t stride;            // problem p's state: arena + p * stride
    SbStatus *st;
    const unsigned char *cls;               // 0 zero cone, 1 nonnegative, 2 member of a block cone
    const int *cones;                       // (beg, end, rotated) per block cone
    float eps_acc, eps_inf, eps_zero; long long max_iter;
};

// the LDS map, in floats.  [sh 64][red 2 T][A lda n] then the vectors; the class bytes last
struct SbMap {
    int sh, red, A, xx, u, kx, ku, xy, xs, v, ky, ks, kv, Tx, Ty, Ts, Sv, b, c, rxx, rxy, rxs, g, h, cls, floats;
    __host__ __device__ SbMap(int n, int m, int lda, int T)
    {
        int o = 0;
        auto take = [&](int k) { const int r = o; o += k; return r; };
        sh = take(64); red = take(2 * T); A = take(lda * n);
        xx = take(n); u = take(n); kx = take(n); ku = take(n);                                   // the arena's order: mutable part
        xy = take(m); xs = take(m); v = take(m); ky = take(m); ks = take(m); kv = take(m);
        Tx = take(n); Ty = take(m); Ts = take(m); Sv = take(m);                                  // constant after init
        b = take(m); c = take(n); rxx = take(n); rxy = take(m); rxs = take(m); g = take(n); h = take(m);
        cls = o; floats = o;
    }
    __host__ __device__ size_t bytes(int m) const { return (size_t)floats * 4 + (size_t)((m + 3) & ~3); }
};
__host__ __device__ inline int sb_lda(int m) { return m | 1; }
__host__ __device__ inline size_t sb_stride(size_t n, size_t m) { return 5 * n + 9 * m; }

// A (global, column-major, lda = m, contiguous) -> LDS with leading dimension lda.  16-byte loads when the base allows them
__device__ __forceinline__ void load_a(const float *__restrict__ src, float *A, int m, int n, int lda)
{
    const int mn = m * n;
    const bool al = ((uintptr_t)src & 15u) == 0;
    for (int e = (int)threadIdx.x * 4; e < mn; e += (int)blockDim.x * 4) {
        float t[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        if (al && e + 3 < mn) {
            const float4 q = *reinterpret_cast<const float4 *>(src + e);
            t[0] = q.x; t[1] = q.y; t[2] = q.z; t[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) if (e + k < mn) t[k] = src[e + k];
        }
        int c = e / m, r = e - c * m;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (e + k < mn) A[r + c * lda] = t[k];
            if (++r == m) { r = 0; ++c; }
        }
    }
}

// one of the two products: out[i] = sum_j M(i, j) x[j], i < ni, j < nj, M(i, j) = A[i * si + j * sj].  The workgroup is
// S = T / roundup64(ni) slices of the j range (slice s takes j = s, s + S, ..: four accumulators, then the slices in order)
template <bool ABS>
__device__ __forceinline__ void product_part(const float *A, int si, int sj, int ni, int nj, const float *x, float *out, float *red)
{
    const int T = (int)blockDim.x, tid = (int)threadIdx.x;
    const int ip = (ni + 63) & ~63;
    const int S = ip >= T ? 1 : T / ip;
    auto dot = [&](int i, int s) {
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
        const float *row = A + i * si;
        int j = s;
        for (; j + 3 * S < nj; j += 4 * S) {
            const float m0 = row[j * sj], m1 = row[(j + S) * sj], m2 = row[(j + 2 * S) * sj], m3 = row[(j + 3 * S) * sj];
            if (ABS) { a0 += fabsf(m0); a1 += fabsf(m1); a2 += fabsf(m2); a3 += fabsf(m3); }
            else { a0 = fmaf(m0, x[j], a0); a1 = fmaf(m1, x[j + S], a1); a2 = fmaf(m2, x[j + 2 * S], a2); a3 = fmaf(m3, x[j + 3 * S], a3); }
        }
        for (; j < nj; j += S) {
            const float m0 = row[j * sj];
            if (ABS) a0 += fabsf(m0); else a0 = fmaf(m0, x[j], a0);
        }
        return (a0 + a1) + (a2 + a3);
    };
    if (S == 1) {
        for (int i = tid; i < ni; i += T) out[i] = dot(i, 0);
    } else {
        const int i = tid % ip, s = tid / ip;
        if (s < S && i < ni) red[s * ip + i] = dot(i, s);
    }
}
__device__ __forceinline__ void product_finish(int ni, float *out, const float *red)
{
    const int T = (int)blockDim.x, tid = (int)threadIdx.x;
    const int ip = (ni + 63) & ~63;
    const int S = ip >= T ? 1 : T / ip;
    if (S > 1 && tid < ni) {
        float a = red[tid];
        for (int s = 1; s < S; ++s) a += red[s * ip + tid];
        out[tid] = a;
    }
}
// h = A xn (m), g = A^T xt (n); a barrier before (the inputs) is the caller's, the results are visible on return
template <bool ABS>
__device__ __forceinline__ void products(const float *A, int lda, int m, int n, const float *xn, const float *xt, float *h, float *g,
                                         float *red)
{
    product_part<ABS>(A, 1, lda, m, n, xn, h, red);
    product_part<ABS>(A, lda, 1, n, m, xt, g, red + blockDim.x);
    __syncthreads();
    product_finish(m, h, red);
    product_finish(n, g, red + blockDim.x);
    __syncthreads();
}

extern __shared__ float sb_lds[];

// calc_norms, calc_precond and init_vecs (solver.rs:460-524) of one problem per workgroup: init_sums_k / init_scalars_k /
// precond_k / group_min_k, with the |A| sums from LDS
__global__ __launch_bounds__(1024) void smallbatch_init_k(const SbArgs a)
{
    const int p = a.live ? a.live[blockIdx.x] : a.first + (int)blockIdx.x;
    const int n = a.n, m = a.m, lda = a.lda, T = (int)blockDim.x, tid = (int)threadIdx.x;
    const SbMap L(n, m, lda, T);
    float *S = sb_lds;
    const SbSlot sl = a.slots[p];
    load_a(sl.a, S + L.A, m, n, lda);
    for (int i = tid; i < m; i += T) S[L.b + i] = sl.b[i];
    for (int i = tid; i < n; i += T) S[L.c + i] = sl.c[i];
    __syncthreads();
    float q[4] = { 0.0f, 0.0f, 0.0f, 0.0f };              // sum b^2, sum |b|, sum c^2, sum |c|
    for (int i = tid; i < m; i += T) { const float t = S[L.b + i]; q[0] = fmaf(t, t, q[0]); q[1] += fabsf(t); }
    for (int i = tid; i < n; i += T) { const float t = S[L.c + i]; q[2] = fmaf(t, t, q[2]); q[3] += fabsf(t); }
    block_sums<4>(q, S + L.sh);
    products<true>(S + L.A, lda, m, n, nullptr, nullptr, S + L.h, S + L.g, S + L.red);      // h = |A| row sums, g = column sums
    float *ar = a.arena + (size_t)p * a.stride;
    float *gTx = ar + 4 * n + 6 * m, *gTy = gTx + n, *gTs = gTy + m, *gSv = gTs + m;
    for (int i = tid; i < n; i += T) {
        const float t = S[L.g + i] + fabsf(S[L.c + i]);
        gTx[i] = 1.0f / fmaxf(t, a.eps_zero);
    }
    for (int i = tid; i < m; i += T) {
        const float t = S[L.h + i] + (sl.rowabs ? sl.rowabs[i] : fabsf(S[L.b + i]));
        S[L.Ty + i] = 1.0f / fmaxf(t, a.eps_zero);
        S[L.Ts + i] = 1.0f / fmaxf(1.0f, a.eps_zero);
        gSv[i] = 1.0f / fmaxf(t + 1.0f, a.eps_zero);
    }
    __syncthreads();
    {   // product_group (solver.rs:509-523): the minimum over each block cone, one wave per cone
        const int lane = tid & 63, w = tid >> 6, nw = T >> 6;
        for (int k = w; k < a.n_cones; k += nw) {
            const int beg = a.cones[3 * k], end = a.cones[3 * k + 1];
            for (int which = 0; which < 2; ++which) {
                float *t = S + (which ? L.Ts : L.Ty);
                float mn = __builtin_inff();
                for (int i = beg + lane; i < end; i += 64) mn = fminf(mn, t[i]);
                mn = wave_min(mn);
                for (int i = beg + lane; i < end; i += 64) t[i] = mn;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < m; i += T) { gTy[i] = S[L.Ty + i]; gTs[i] = S[L.Ts + i]; }
    for (int i = tid; i < 4 * n + 6 * m; i += T) ar[i] = 0.0f;      // init_vecs: x = 0, y = 0 (and the Kahan terms)
    if (tid == 0) {
        SbStatus s;
        s.stop = 0; s.state = THIP_ST_RUNNING; s.kind = 0; s.pad = 0; s.iter = 0;
        s.cri[0] = s.cri[1] = s.cri[2] = 0.0f;
        s.tau = 1.0f; s.kappa = 0.0f; s.r_tau = 0.0f;
        const float nb = sqrtf(q[0]), nc = sqrtf(q[2]);      // fr_norm (solver.rs:85-107)
        s.norm_b = sqrtf(nb * nb);
        s.norm_c = sqrtf(nc * nc);
        const float tau_tau = q[3] + q[1];
        s.t_tau = 1.0f / fmaxf(tau_tau, a.eps_zero);
        s.s_kappa = 1.0f / fmaxf(tau_tau, a.eps_zero);
        a.st[p] = s;
    }
}

__global__ __launch_bounds__(1024) void smallbatch_k(const SbArgs a)
{
    const int p = a.live ? a.live[blockIdx.x] : a.first + (int)blockIdx.x;
    SbStatus *const gst = a.st + p;
    if (gst->stop != 0) return;
    const int n = a.n, m = a.m, lda = a.lda, T = (int)blockDim.x, tid = (int)threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6, nw = T >> 6;
    const bool comp = a.comp != 0;
    const SbMap L(n, m, lda, T);
    float *S = sb_lds;
    float *const A = S + L.A, *const sh = S + L.sh, *const red = S + L.red;
    float *const xx = S + L.xx, *const u = S + L.u, *const kx = S + L.kx, *const ku = S + L.ku;
    float *const xy = S + L.xy, *const xs = S + L.xs, *const v = S + L.v, *const ky = S + L.ky, *const ks = S + L.ks, *const kv = S + L.kv;
    const float *const Tx = S + L.Tx, *const Ty = S + L.Ty, *const Ts = S + L.Ts, *const Sv = S + L.Sv;
    const float *const b = S + L.b, *const c = S + L.c;
    float *const rxx = S + L.rxx, *const rxy = S + L.rxy, *const rxs = S + L.rxs, *const g = S + L.g, *const h = S + L.h;
    unsigned char *const cls = reinterpret_cast<unsigned char *>(S + L.cls);

    // ---- load ----
    const SbSlot sl = a.slots[p];
    float *const ar = a.arena + (size_t)p * a.stride;
    load_a(sl.a, A, m, n, lda);
    {
        const int nstate = 5 * n + 9 * m;                  // the arena's order is the LDS order from xx on
        for (int i = tid; i < nstate; i += T) xx[i] = ar[i];
    }
    for (int i = tid; i < m; i += T) { S[L.b + i] = sl.b[i]; cls[i] = a.cls[i]; }
    for (int i = tid; i < n; i += T) S[L.c + i] = sl.c[i];
    float tau = gst->tau, kappa = gst->kappa, rtau = gst->r_tau;
    const float norm_b = gst->norm_b, norm_c = gst->norm_c, t_tau = gst->t_tau, s_kappa = gst->s_kappa;
    long long iter = gst->iter;
    int state = THIP_ST_RUNNING, kind = gst->kind;
    float cri0 = gst->cri[0], cri1 = gst->cri[1], cri2 = gst->cri[2];
    __syncthreads();

    for (int step = 0; step < a.steps; ++step) {
        // ---- x += T o (-K^T y): h = A u, g = A^T v; c.u, b.v (xupdate_k) ----
        float q[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        for (int i = tid; i < n; i += T) q[0] = fmaf(c[i], u[i], q[0]);
        for (int i = tid; i < m; i += T) q[1] = fmaf(b[i], v[i], q[1]);
        products<false>(A, lda, m, n, u, v, h, g, red);
        block_sums<2>(q, sh);
        for (int i = tid; i < n; i += T) {
            const float old = xx[i];
            const float nx = sb_comp_add(old, Tx[i] * (g[i] + c[i] * kappa), kx, i, comp);
            xx[i] = nx;
            rxx[i] = old - 2.0f * nx;
        }
        for (int i = tid; i < m; i += T) {
            const unsigned char k = cls[i];
            const float oy = xy[i], os = xs[i];
            float ny = sb_comp_add(oy, Ty[i] * (b[i] * kappa - h[i]), ky, i, comp);
            float ns = sb_comp_add(os, Ts[i] * v[i], ks, i, comp);
            if (k == 1) { ny = fmaxf(ny, 0.0f); ns = fmaxf(ns, 0.0f); }
            else if (k == 0) { ns = 0.0f; }
            xy[i] = ny;
            xs[i] = ns;
            rxy[i] = (k < 2) ? oy - 2.0f * ny : oy;
            rxs[i] = (k < 2) ? os - 2.0f * ns : os;
        }
        {
            const float old = tau;
            tau = fmaxf(old + t_tau * (-q[0] - q[1]), 0.0f);      // solver.rs:551-552
            rtau = old - 2.0f * tau;
        }
        __syncthreads();
        // ---- the block cones: one wave per cone, x_y then x_s ----
        if (a.n_cones > 0) {
            for (int k = wv; k < a.n_cones; k += nw) {
                const int beg = a.cones[3 * k], end = a.cones[3 * k + 1], rot = a.cones[3 * k + 2];
                sb_soc(xy, rxy, beg, end, rot, lane);
                sb_soc(xs, rxs, beg, end, rot, lane);
            }
            __syncthreads();
        }
        // ---- y += S o (-K rx): h = A rx_x, g = A^T rx_y; c.rx_x, b.rx_y (ycrit_k) ----
        q[0] = q[1] = 0.0f;
        for (int i = tid; i < n; i += T) q[0] = fmaf(c[i], rxx[i], q[0]);
        for (int i = tid; i < m; i += T) q[1] = fmaf(b[i], rxy[i], q[1]);
        products<false>(A, lda, m, n, rxx, rxy, h, g, red);
        block_sums<2>(q, sh);
        for (int i = tid; i < n; i += T) u[i] = sb_comp_add(u[i], Tx[i] * (-g[i] - c[i] * rtau), ku, i, comp);
        for (int i = tid; i < m; i += T) v[i] = sb_comp_add(v[i], Sv[i] * (h[i] + rxs[i] - b[i] * rtau), kv, i, comp);
        kappa = fminf(kappa + s_kappa * (q[0] + q[1]), 0.0f);     // solver.rs:566-567
        __syncthreads();
        // ---- criteria: h = A x_x, g = A^T x_y (post_k / ycrit_k / status_eval) ----
        products<false>(A, lda, m, n, xx, xy, h, g, red);
        const bool conv = tau > a.eps_zero;
        const float rt = conv ? 1.0f / tau : 1.0f;
        q[0] = q[1] = q[2] = q[3] = 0.0f;                          // ||p||^2, b.x_y, ||d||^2, c.x_x
        for (int i = tid; i < m; i += T) {
            const float bi = b[i];
            float pr;
            if (conv) { pr = xs[i] * rt - bi; pr = fmaf(rt, h[i], pr); }
            else pr = xs[i] + h[i];
            q[0] = fmaf(pr, pr, q[0]);
            q[1] = fmaf(bi, xy[i], q[1]);
        }
        for (int i = tid; i < n; i += T) {
            const float ci = c[i];
            const float d = conv ? fmaf(rt, g[i], ci) : g[i];
            q[2] = fmaf(d, d, q[2]);
            q[3] = fmaf(ci, xx[i], q[3]);
        }
        block_sums<4>(q, sh);
        const float pp = q[0], by = q[1], dd = q[2], cx = q[3];
        const bool excess_iter = (a.max_iter >= 0) ? (iter + 1 >= a.max_iter) : false;
        const float norm_p = sqrtf(pp), norm_d = sqrtf(dd);
        if (conv) {
            const float g_x = rt * cx;
            const float g_y = rt * by;
            const float gg = g_x + g_y;
            kind = 0;
            cri0 = norm_p / (1.0f + norm_b);
            cri1 = norm_d / (1.0f + norm_c);
            cri2 = fabsf(gg) / (1.0f + fabsf(g_x) + fabsf(g_y));
            const bool term_conv = (cri0 <= a.eps_acc) && (cri1 <= a.eps_acc) && (cri2 <= a.eps_acc);
            if (term_conv) state = THIP_ST_OK;
            else if (excess_iter) state = THIP_ST_EXCESS_ITER;
        } else {
            const float m_cx = -cx;
            const float m_by = -by;
            kind = 1;
            cri0 = (m_cx > a.eps_zero) ? norm_p * norm_c / m_cx : __builtin_inff();
            cri1 = (m_by > a.eps_zero) ? norm_d * norm_b / m_by : __builtin_inff();
            cri2 = 0.0f;
            if (cri0 <= a.eps_inf) state = THIP_ST_UNBOUNDED;
            else if (cri1 <= a.eps_inf) state = THIP_ST_INFEASIBLE;
            else if (excess_iter) state = THIP_ST_EXCESS_ITER;
        }
        if (state != THIP_ST_RUNNING) break;                       // (uniform: every thread holds the same sums)
        iter += 1;
    }

    // ---- store ----
    __syncthreads();
    {
        const int nmut = 4 * n + 6 * m;
        for (int i = tid; i < nmut; i += T) ar[i] = xx[i];
    }
    if (tid == 0) {
        gst->tau = tau; gst->kappa = kappa; gst->r_tau = rtau; gst->iter = iter;
        gst->kind = kind; gst->cri[0] = cri0; gst->cri[1] = cri1; gst->cri[2] = cri2;
        gst->state = state;
        gst->stop = state != THIP_ST_RUNNING ? 1 : 0;
    }
}

size_t g_sb_bytes = 0;                      // device memory held by every thip_smallbatch of the process

const ObText SB_TEXT = { "small batch not initialised", "null small batch", "a small batch holds 1 .. 1048576 problems",
                         "a small batch takes no PSD segment" };

int sb_threads_for(size_t n, size_t m)
{
    const size_t area = n * m;
    return area <= 1024 ? 64 : (area <= 8192 ? 256 : 1024);
}

// the shape rules (no device needed).  On success *cones holds (beg, end, rotated) per block cone and *cls the class bytes
int sb_check(size_t n, size_t m, size_t n_seg, const int32_t *seg_type, const int64_t *seg_len, std::vector<int> *cones,
             std::vector<unsigned char> *cls)
{
    if (m < 1 || m > SB_MAX_DIM || n < 1 || n > SB_MAX_DIM)
        return fail(THIP_E_INVALID, "a small batch takes 1 <= m <= 1024 and 1 <= n <= 1024", __FILE__, __LINE__);
    if (m * n > SB_MAX_AREA) return fail(THIP_E_INVALID, "a small batch takes m * n <= 24576 (96 KiB of A on chip)", __FILE__, __LINE__);
    return ob_segments(SB_TEXT, m, n_seg, seg_type, seg_len, cones, cls);
}

}  // namespace

struct thip_smallbatch : OwnBatch {};

namespace {

int sb_attr()
{
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    std::call_once(once, [&]() {
        err = hipFuncSetAttribute(reinterpret_cast<const void *>(&smallbatch_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SB_LDS_MAX);
        if (err == hipSuccess)
            err = hipFuncSetAttribute(reinterpret_cast<const void *>(&smallbatch_init_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)SB_LDS_MAX);
    });
    THIP_TRY(err);
    return 0;
}

void sb_plan(OwnBatch *h)
{
    h->threads = h->forced ? h->forced : sb_threads_for(h->n, h->m);
    h->lds = SbMap((int)h->n, (int)h->m, sb_lda((int)h->m), h->threads).bytes((int)h->m);
}

SbArgs sb_args(const OwnBatch *h)
{
    SbArgs a{};
    a.n = (int)h->n; a.m = (int)h->m; a.lda = sb_lda((int)h->m); a.n_cones = (int)(h->cones.size() / 3);
    a.comp = h->par.state_arith == THIP_STATE_COMPENSATED; a.steps = 0; a.first = 0; a.live = nullptr;
    a.slots = h->slots; a.arena = h->arena; a.stride = h->stride; a.st = h->dst; a.cls = h->cls_dev; a.cones = h->cones_dev;
    a.eps_acc = h->par.eps_acc; a.eps_inf = h->par.eps_inf; a.eps_zero = h->par.eps_zero; a.max_iter = h->par.max_iter;
    return a;
}

int sb_launch_init(OwnBatch *h, int first, int count)
{
    SbArgs a = sb_args(h);
    a.first = first;
    hipLaunchKernelGGL(smallbatch_init_k, dim3((unsigned)count), dim3((unsigned)h->threads), h->lds, ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

int sb_launch_run(OwnBatch *h, int count, int steps, const int *live)
{
    SbArgs a = sb_args(h);
    a.steps = steps;
    a.live = live;
    hipLaunchKernelGGL(smallbatch_k, dim3((unsigned)count), dim3((unsigned)h->threads), h->lds, ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int thip_smallbatch_fits(size_t n, size_t m, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                         size_t *host_lds_bytes, int *host_threads)
{
    THIP_RC(sb_check(n, m, n_seg, host_seg_type, host_seg_len, nullptr, nullptr));
    const int t = sb_threads_for(n, m);
    if (host_threads) *host_threads = t;
    // (the figure is that of the widest workgroup a test may force: no accepted shape can fail to launch)
    if (host_lds_bytes) *host_lds_bytes = SbMap((int)n, (int)m, sb_lda((int)m), t).bytes((int)m);
    if (SbMap((int)n, (int)m, sb_lda((int)m), 1024).bytes((int)m) > SB_LDS_MAX)
        return fail(THIP_E_INVALID, "the problem does not fit the LDS of one CU", __FILE__, __LINE__);
    return 0;
}

int thip_smallbatch_destroy(thip_smallbatch *h)
{
    if (!h) return 0;
    ob_destroy(h);
    delete h;
    return 0;
}

int thip_smallbatch_create(size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b, const float *dev_vecs_c,
                           const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                           const thip_param *par, thip_smallbatch **out)
{
    if (!out) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *out = nullptr;
    THIP_NEED_INIT();
    THIP_RC(ob_create_args(SB_TEXT, n_prob, dev_mats_a, dev_vecs_b, dev_vecs_c, dev_vecs_b_rowabs, par));
    thip_smallbatch *h = new thip_smallbatch();
    h->text = &SB_TEXT; h->total = &g_sb_bytes; h->launch_init = sb_launch_init; h->launch_run = sb_launch_run;
    // every refusal comes before the first allocation
    int rc = sb_check(n, m, n_seg, host_seg_type, host_seg_len, &h->cones, &h->cls);
    if (rc == 0) rc = thip_smallbatch_fits(n, m, n_seg, host_seg_type, host_seg_len, nullptr, nullptr);
    if (rc != 0) { delete h; return rc; }
    h->n = n; h->m = m; h->n_prob = n_prob;
    h->par = *par;
    h->stride = sb_stride(n, m);
    sb_plan(h);
    rc = sb_attr();
    if (rc == 0) rc = ob_build(h, dev_mats_a, dev_vecs_b, dev_vecs_c, dev_vecs_b_rowabs);
    if (rc != 0) { thip_smallbatch_destroy(h); return rc; }
    *out = h;
    return 0;
}

int thip_smallbatch_set_param(thip_smallbatch *h, const thip_param *par) { return ob_set_param(h, par); }

int thip_smallbatch_init(thip_smallbatch *h) { return ob_init(h, SB_TEXT); }

int thip_smallbatch_run(thip_smallbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{
    if (!h) { THIP_NEED_INIT(); return fail(THIP_E_INVALID, SB_TEXT.uninit, __FILE__, __LINE__); }
    return ob_run(h, max_steps, poll_every, host_status, false);
}

int thip_smallbatch_run_until_any(thip_smallbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{
    if (!h) { THIP_NEED_INIT(); return fail(THIP_E_INVALID, SB_TEXT.uninit, __FILE__, __LINE__); }
    return ob_run(h, max_steps, poll_every, host_status, true);
}

int thip_smallbatch_status(thip_smallbatch *h, int i, thip_status *host_status)
{
    if (!h) { THIP_NEED_INIT(); return fail(THIP_E_INVALID, SB_TEXT.uninit, __FILE__, __LINE__); }
    return ob_status(h, i, host_status);
}

int thip_smallbatch_solution(thip_smallbatch *h, int i, float *host_x, float *host_y)
{
    if (!h) { THIP_NEED_INIT(); return fail(THIP_E_INVALID, SB_TEXT.uninit, __FILE__, __LINE__); }
    return ob_solution(h, i, host_x, host_y);
}

int thip_smallbatch_iterate(thip_smallbatch *h, int i, float *host_x, float *host_y)
{
    if (!h) { THIP_NEED_INIT(); return fail(THIP_E_INVALID, SB_TEXT.uninit, __FILE__, __LINE__); }
    return ob_iterate(h, i, host_x, host_y);
}

int thip_smallbatch_precond(thip_smallbatch *h, int i, float *host_dp_tau, float *host_dp_sigma)
{
    if (!h) { THIP_NEED_INIT(); return fail(THIP_E_INVALID, SB_TEXT.uninit, __FILE__, __LINE__); }
    return ob_precond(h, i, host_dp_tau, host_dp_sigma);
}

int thip_smallbatch_replace(thip_smallbatch *h, int i, const float *dev_mat_a, const float *dev_vec_b, const float *dev_vec_c,
                            const float *dev_vec_b_rowabs)
{
    if (!h) { THIP_NEED_INIT(); return fail(THIP_E_INVALID, SB_TEXT.uninit, __FILE__, __LINE__); }
    return ob_replace(h, i, dev_mat_a, dev_vec_b, dev_vec_c, dev_vec_b_rowabs);
}

int thip_smallbatch_info(const thip_smallbatch *h, thip_smallbatch_info_t *host_info)
{
    if (!h || !host_info) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    thip_smallbatch_info_t &o = *host_info;
    memset(&o, 0, sizeof(o));
    o.n_prob = (int32_t)h->n_prob; o.threads = h->threads; o.lds_bytes = (int32_t)h->lds; o.live = (int32_t)h->live.size();
    o.arena_bytes = h->stride * h->n_prob * sizeof(float);
    o.device_bytes = h->bytes;
    o.device_bytes_all = g_sb_bytes;
    o.launches = h->launches; o.workgroups = h->workgroups;
    return 0;
}

int thip_test_smallbatch_force_threads(thip_smallbatch *h, int threads)
{
    if (!h) return fail(THIP_E_INVALID, "null small batch", __FILE__, __LINE__);
    if (threads != 0 && threads != 64 && threads != 256 && threads != 1024)
        return fail(THIP_E_INVALID, "the workgroup size is 64, 256 or 1024 (0: by shape)", __FILE__, __LINE__);
    if (h->inited) return fail(THIP_E_INVALID, "thip_test_smallbatch_force_threads comes before thip_smallbatch_init", __FILE__, __LINE__);
    h->forced = threads;
    sb_plan(h);
    return 0;
}

}  // extern "C"
