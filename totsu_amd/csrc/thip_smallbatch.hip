// thip_smallbatch.hip -- thip_smallbatch: many small conic programs, each with its OWN dense f32 A (shared n, m and cone layout), iterated on
// chip.  A launch of smallbatch_k gives one workgroup to each live problem: the workgroup loads its A into LDS (m n <= 24 576 floats
// = 96 KiB of the CU's 160 KiB), its state from the problem's arena, runs up to `steps` iterations of the reference's loop
// (solver.rs:340-458; oracle/totsu_oracle.c core_solve) with no launch boundary inside an iteration, and writes the state back.
//
// Recurrence: the 3-pass ("fused") one -- A u / A^T v, A rx_x / A^T rx_y, A x_x / A^T x_y, each pair from LDS.  A pass over an
// LDS-resident A is a few hundred cycles, so the carried form's saved pass is not worth its two extra state vectors and its second
// rounding of K rx.  The element-wise arithmetic is thip_step.h's, as in every other loop of the step; the preconditioner's
// minimum over a block cone is group_min_k's (thip_cone.hip).
//
// LDS: A with leading dimension lda = m | 1 (odd): the row walk of A x has consecutive lanes on consecutive words, the column walk of
// A^T y has consecutive lanes lda words apart -- an odd stride visits every bank once.  Behind A: every vector of the iteration.
//
// Sums: per-thread fmaf chains, DPP wave sums, then the waves' values through LDS added in wave order (f64).  No atomics: a
// problem's result is a function of (its data, the workgroup size) alone -- not of its index, its neighbours or the launch.
//
// This file: the LDS map, the products from LDS, the two kernels, the shape rule (sb_check), the thread choice and the family's
// table.  The launch arguments, the status block, the slots, the init kernel's body, the criteria and status_eval, and the whole
// host side behind the C API are shared with the streamed batches (thip_midbatch.hip, thip_sdpbatch.hip): thip_ownbatch.h.
#define OB_DEFINE_HOOKS 1      // (thip_test_ownbatch_*: this translation unit defines them)
#include "thip_ownbatch.h"

using namespace thip;

namespace {

constexpr size_t SB_MAX_DIM = 1024, SB_MAX_AREA = 24576;

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

struct SbShape { int n, m, lda; };
using SbArgs = ObArgsT<SbShape>;

extern __shared__ float sb_lds[];

// ob_init_body with the |A| sums from LDS
__global__ __launch_bounds__(1024) void smallbatch_init_k(const SbArgs a)
{
    const int n = a.n, m = a.m, lda = a.lda;
    const SbMap L(n, m, lda, (int)blockDim.x);
    float *S = sb_lds;
    ob_init_body(a, ob_problem(a.live, a.first), L, S, [&](const float *src) {
        load_a(src, S + L.A, m, n, lda);
        __syncthreads();
        products<true>(S + L.A, lda, m, n, nullptr, nullptr, S + L.h, S + L.g, S + L.red);      // h = |A| row sums, g = column sums
    });
}

__global__ __launch_bounds__(1024) void smallbatch_k(const SbArgs a)
{
    const int p = ob_problem(a.live, a.first);
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
    ObScalars s;
    s.load(gst);
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
            const float nx = kahan_add_at(old, inc_xx(Tx[i], g[i], c[i], s.kappa), comp, kx, i);
            xx[i] = nx;
            rxx[i] = rx_fold(old, nx);
        }
        for (int i = tid; i < m; i += T) {
            const unsigned char k = cls[i];
            const float oy = xy[i], os = xs[i];
            float ny = kahan_add_at(oy, inc_xy(Ty[i], b[i], s.kappa, h[i]), comp, ky, i);
            float ns = kahan_add_at(os, inc_xs(Ts[i], v[i]), comp, ks, i);
            cone_elementwise(k, ny, ns);
            xy[i] = ny;
            xs[i] = ns;
            rxy[i] = cone_rx(k, oy, ny);
            rxs[i] = cone_rx(k, os, ns);
        }
        {
            const float old = s.tau;
            s.tau = fmaxf(old + s.t_tau * (-q[0] - q[1]), 0.0f);      // solver.rs:551-552
            s.rtau = old - 2.0f * s.tau;
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
        for (int i = tid; i < n; i += T) u[i] = kahan_add_at(u[i], inc_u(Tx[i], g[i], c[i], s.rtau), comp, ku, i);
        for (int i = tid; i < m; i += T) v[i] = kahan_add_at(v[i], inc_v(Sv[i], h[i], rxs[i], b[i], s.rtau), comp, kv, i);
        s.kappa = fminf(s.kappa + s.s_kappa * (q[0] + q[1]), 0.0f);     // solver.rs:566-567
        __syncthreads();
        // ---- criteria: h = A x_x, g = A^T x_y (post_k / ycrit_k / status_eval) ----
        products<false>(A, lda, m, n, xx, xy, h, g, red);
        ob_criteria_sums(q, n, m, s.tau, a.eps_zero, b, c, xx, xy, xs, h, g, sh);
        ob_status_eval(s, ObLimits{ a.eps_acc, a.eps_inf, a.eps_zero, a.max_iter }, q[0], q[1], q[2], q[3]);
        if (s.state != THIP_ST_RUNNING) break;                     // (uniform: every thread holds the same sums)
        s.iter += 1;
    }

    // ---- store ----
    __syncthreads();
    {
        const int nmut = 4 * n + 6 * m;
        for (int i = tid; i < nmut; i += T) ar[i] = xx[i];
    }
    if (tid == 0) s.store(gst);
}

// a problem starts from a given iterate (thip_smallbatch_set_iterates).  The three-pass recurrence carries no products, so the
// workgroup writes the mutable part of the arena -- xx u kx ku | xy xs v ky ks kv, the Kahan terms zero -- and the status block
struct SbStartArgs { SbArgs sb; ObStart s; };

__global__ __launch_bounds__(1024) void smallbatch_start_k(const SbStartArgs a)
{
    const int p = ob_problem(a.sb.live, a.sb.first);
    const int n = a.sb.n, m = a.sb.m, T = (int)blockDim.x, tid = (int)threadIdx.x;
    const float *const x = ob_staged(a.s), *const y = x + n + 2 * m + 1;      // x_x x_y x_s tau | u v kappa
    float *const ar = a.sb.arena + (size_t)p * a.sb.stride;
    float *const gy = ar + 4 * n;
    for (int i = tid; i < n; i += T) {
        ar[i] = x[i]; ar[n + i] = y[i];
        ar[2 * n + i] = 0.0f; ar[3 * n + i] = 0.0f;
    }
    for (int i = tid; i < m; i += T) {
        gy[i] = x[n + i]; gy[m + i] = x[n + m + i]; gy[2 * m + i] = y[n + i];
        gy[3 * m + i] = 0.0f; gy[4 * m + i] = 0.0f; gy[5 * m + i] = 0.0f;
    }
    if (tid == 0) ob_start_status(a.sb.st + p, x[n + 2 * m], y[n + m]);
}

// a problem takes a new (b, c) and keeps its A (thip_smallbatch_set_bc): ob_init_body on the staged data, the |A| sums from LDS
struct SbSetBcArgs { SbArgs sb; ObSetBc s; };

__global__ __launch_bounds__(1024) void smallbatch_setbc_k(const SbSetBcArgs a)
{
    const int n = a.sb.n, m = a.sb.m, lda = a.sb.lda;
    const SbMap L(n, m, lda, (int)blockDim.x);
    float *S = sb_lds;
    ob_init_body(a.sb, ob_problem(a.sb.live, a.sb.first), L, S, [&](const float *src) {
        load_a(src, S + L.A, m, n, lda);
        __syncthreads();
        products<true>(S + L.A, lda, m, n, nullptr, nullptr, S + L.h, S + L.g, S + L.red);
    }, ObUniform(), ObTakeBc{ a.s });
}

// a problem's A has new values (thip_smallbatch_set_a): ob_init_body on the slot's own b, c and row sums, the |A| sums from LDS, the
// ending taken from the call.  The three-pass recurrence carries no pair
struct SbSetAArgs { SbArgs sb; int keep; };

__global__ __launch_bounds__(1024) void smallbatch_seta_k(const SbSetAArgs a)
{
    const int n = a.sb.n, m = a.sb.m, lda = a.sb.lda;
    const SbMap L(n, m, lda, (int)blockDim.x);
    float *S = sb_lds;
    ob_init_body(a.sb, ob_problem(a.sb.live, a.sb.first), L, S, [&](const float *src) {
        load_a(src, S + L.A, m, n, lda);
        __syncthreads();
        products<true>(S + L.A, lda, m, n, nullptr, nullptr, S + L.h, S + L.g, S + L.red);
    }, ObUniform(), ObKeepA{ a.keep });
}

const ObText SB_TEXT = { "small batch not initialised", "null small batch", "a small batch holds 1 .. 1048576 problems",
                         "a small batch takes no PSD segment", "the workgroup size is 64, 256 or 1024 (0: by shape)",
                         "thip_test_smallbatch_force_threads comes before thip_smallbatch_init" };

int sb_threads_for(size_t n, size_t m)
{
    const size_t area = n * m;
    return area <= 1024 ? 64 : (area <= 8192 ? 256 : 1024);
}

// the shape rules (no device needed).  On success *cones holds (beg, end, rotated) per block cone and *cls the class bytes
int sb_check(size_t n, size_t m, size_t n_seg, const int32_t *seg_type, const int64_t *seg_len, std::vector<int> *cones,
             std::vector<unsigned char> *cls, ObPsd *)
{
    if (m < 1 || m > SB_MAX_DIM || n < 1 || n > SB_MAX_DIM)
        return fail(THIP_E_INVALID, "a small batch takes 1 <= m <= 1024 and 1 <= n <= 1024", __FILE__, __LINE__);
    if (m * n > SB_MAX_AREA) return fail(THIP_E_INVALID, "a small batch takes m * n <= 24576 (96 KiB of A on chip)", __FILE__, __LINE__);
    return ob_segments(SB_TEXT, m, n_seg, seg_type, seg_len, cones, cls);
}

size_t sb_lds_for(size_t n, size_t m, int threads, const ObPsd &)
{
    return SbMap((int)n, (int)m, sb_lda((int)m), threads).bytes((int)m);
}

SbArgs sb_args(const ObArgs &a)
{
    SbArgs b{};
    b.n = a.n; b.m = a.m; b.lda = sb_lda(a.m);
    static_cast<ObCounts &>(b) = a;
    static_cast<ObRest &>(b) = a;
    return b;
}

int sb_launch(const OwnBatch *h, bool run, const ObArgs &a, unsigned count)
{
    return ob_launch(h, run ? smallbatch_k : smallbatch_init_k, sb_args(a), count);
}

int sb_start(const OwnBatch *h, const ObArgs &a, const ObStart &s, unsigned count)
{
    return ob_launch(h, smallbatch_start_k, SbStartArgs{ sb_args(a), s }, count);
}

int sb_setbc(const OwnBatch *h, const ObArgs &a, const ObSetBc &s, unsigned count)
{
    return ob_launch(h, smallbatch_setbc_k, SbSetBcArgs{ sb_args(a), s }, count);
}

int sb_seta(const OwnBatch *h, const ObArgs &a, const ObSetA &s, unsigned count)
{
    return ob_launch(h, smallbatch_seta_k, SbSetAArgs{ sb_args(a), s.keep }, count);
}

ObFamily SB_FAMILY = { SB_TEXT, { 64, 256, 1024 }, false, sb_check, sb_threads_for, sb_lds_for, sb_stride, sb_launch, sb_start, sb_setbc,
                       sb_seta,
                       { (const void *)smallbatch_k, (const void *)smallbatch_init_k, (const void *)smallbatch_start_k,
                         (const void *)smallbatch_setbc_k, (const void *)smallbatch_seta_k, nullptr } };

}  // namespace

struct thip_smallbatch : OwnBatch {};

OB_DEFINE_API(smallbatch, SB_FAMILY, ObInfo)
