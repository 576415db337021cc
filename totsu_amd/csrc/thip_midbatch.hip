// thip_midbatch.hip -- thip_midbatch: many MID-SIZE conic programs, each with its OWN dense f32 A (shared n, m and cone layout), too big
// for the LDS of a CU (thip_smallbatch.hip) and far too small for the big-A schedules to be anything but launch-bound.  A launch of
// midbatch_k gives one workgroup to each live problem: every vector of the iteration lives in LDS, A is STREAMED from the caller's
// array (column-major, lda = m, never copied, never written), `steps` whole iterations per launch with no launch boundary inside.
//
// Recurrence: the carried one -- two passes over A per iteration.  Pass 1 forms h = A u, g = A^T v for the x-update
// and the cones; pass 2 forms h = A x_x, g = A^T x_y of the NEW iterate, which serves the criteria and, through
// A rx_x = A x_k - 2 A x_{k+1} (likewise A^T rx_y, c.rx_x, b.rx_y), the y-update.  The pair (A x_k, A^T x_y,k) is carried in the
// arena behind the preconditioner, so a launch boundary changes nothing (tested bitwise).
//
// A pass (mb_pass): the rows are cut into tiles of MB_ROWS = 256 (a lane holds 4 consecutive rows: one 16-byte load per column when
// m % 4 == 0 and the problem's base is 16-byte aligned, four 4-byte loads of the same entries otherwise -- the same lanes hold the
// same entries, so both paths add in the same order), the columns into chunks of MB_CK = 8.  With R row tiles and nw waves the
// workgroup is R x S units, S = max(1, nw / R) column slices (slice s takes the chunks s, s + S, ..); wave w serves the units
// w, w + nw, ...  A unit loads the 8 columns of a chunk at once (8 independent loads in flight per lane), and every loaded entry
// feeds both h += A[:, j] xn[j] (row sums in registers across the unit's chunks) and g[j] = A[:, j] . xt (a DPP wave sum per column).
// The R partial g of a column meet in LDS (gp) per batch of CB = max(8, 2048 / R rounded down to 8) columns and are added in tile
// order; the S partial h of a row meet in LDS (hp) and are added in slice order.  No atomics: a problem's iterates are a function of
// (its data, the workgroup size, these constants) alone -- not of its index, its neighbours or the launch.
//
// LDS, in floats: [sh 64][hp 4096][gp 2048], then xx u kx ku | xy xs v ky ks kv | Tx Ty Ts Sv | hx gx (the arena's order), then
// b c rxs g h: 8 n + 13 m floats of vectors, and the class bytes.  mb_fits is the single source of the limit.
//
// The rest of the iteration is the small batch's, on the same device functions (thip_ownbatch.h): sb_comp_add, the class bytes,
// one wave per block cone (sb_soc), block_sums, both endings of status_eval.
#include "thip_ownbatch.h"

#include <mutex>

using namespace thip;

namespace {

constexpr int MB_ROWS = 256, MB_CK = 8, MB_SCRH = 4096, MB_SCRG = 2048;
constexpr size_t MB_MAX_DIM = 4096, MB_LDS_MAX = OB_LDS_MAX;

struct MbArgs {
    int n, m, n_cones, comp, steps;
    int first;                              // live == NULL: workgroup k serves problem first + k
    const int *live;                        // else problem live[k]
    const SbSlot *slots;
    float *arena; size_t stride;            // problem p's state: arena + p * stride
    SbStatus *st;
    const unsigned char *cls;               // 0 zero cone, 1 nonnegative, 2 member of a block cone
    const int *cones;                       // (beg, end, rotated) per block cone
    float eps_acc, eps_inf, eps_zero; long long max_iter;
};

struct MbMap {
    int sh, hp, gp, xx, u, kx, ku, xy, xs, v, ky, ks, kv, Tx, Ty, Ts, Sv, hx, gx, b, c, rxs, g, h, cls, floats;
    __host__ __device__ MbMap(int n, int m)
    {
        int o = 0;
        auto take = [&](int k) { const int r = o; o += k; return r; };
        sh = take(64); hp = take(MB_SCRH); gp = take(MB_SCRG);
        xx = take(n); u = take(n); kx = take(n); ku = take(n);                                   // the arena's order: mutable part
        xy = take(m); xs = take(m); v = take(m); ky = take(m); ks = take(m); kv = take(m);
        Tx = take(n); Ty = take(m); Ts = take(m); Sv = take(m);                                  // constant after init
        hx = take(m); gx = take(n);                                                              // carried: A x_x, A^T x_y
        b = take(m); c = take(n); rxs = take(m); g = take(n); h = take(m);
        cls = o; floats = o;
    }
    __host__ __device__ size_t bytes(int m) const { return (size_t)floats * 4 + (size_t)((m + 3) & ~3); }
};
__host__ __device__ inline size_t mb_stride(size_t n, size_t m) { return 6 * n + 10 * m; }

// h = A xn (m), g = A^T xt (n) from ONE read of A (ABS: the row and column sums of |A|).  A: global, column-major, lda = m.
// Begins and ends with a barrier: the inputs written before the call are seen, the results are visible on return.
template <bool ABS, bool VEC>
__device__ __forceinline__ void mb_pass_t(const float *__restrict__ A, int m, int n, const float *xn, const float *xt, float *h, float *g,
                                          float *hp, float *gp)
{
    const int T = (int)blockDim.x, tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, nw = T >> 6;
    const int R = (m + MB_ROWS - 1) / MB_ROWS;
    const int S = R >= nw ? 1 : nw / R;
    const int CB = max(MB_CK, (MB_SCRG / R) & ~(MB_CK - 1));
    __syncthreads();
    for (int cb0 = 0; cb0 < n; cb0 += CB) {
        const int cbn = min(CB, n - cb0);
        const int nch = (cbn + MB_CK - 1) / MB_CK;
        for (int unit = w; unit < R * S; unit += nw) {
            const int r = unit % R, s = unit / R;
            const int row = r * MB_ROWS + lane * 4;
            const bool in0 = row < m, in1 = row + 1 < m, in2 = row + 2 < m, in3 = row + 3 < m;
            float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;
            if (ABS) {
                t0 = t1 = t2 = t3 = 1.0f;
            } else {
                if (in0) t0 = xt[row];
                if (in1) t1 = xt[row + 1];
                if (in2) t2 = xt[row + 2];
                if (in3) t3 = xt[row + 3];
            }
            auto ld = [&](int j) {
                float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                const float *p = A + (size_t)j * (size_t)m + row;
                if (VEC) {
                    if (in0) q = *reinterpret_cast<const float4 *>(p);      // (m % 4 == 0: all four rows or none)
                } else {
                    if (in0) q.x = p[0];
                    if (in1) q.y = p[1];
                    if (in2) q.z = p[2];
                    if (in3) q.w = p[3];
                }
                if (ABS) { q.x = fabsf(q.x); q.y = fabsf(q.y); q.z = fabsf(q.z); q.w = fabsf(q.w); }
                return q;
            };
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
            for (int ch = s; ch < nch; ch += S) {
                const int j0 = cb0 + ch * MB_CK;
                const int nj = min(MB_CK, cb0 + cbn - j0);
                float4 q[MB_CK];
                float xj[MB_CK];
                if (nj == MB_CK) {
#pragma unroll
                    for (int k = 0; k < MB_CK; ++k) q[k] = ld(j0 + k);
#pragma unroll
                    for (int k = 0; k < MB_CK; ++k) xj[k] = ABS ? 1.0f : xn[j0 + k];
                } else {
#pragma unroll
                    for (int k = 0; k < MB_CK; ++k) {
                        q[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        xj[k] = 0.0f;
                        if (k < nj) { q[k] = ld(j0 + k); xj[k] = ABS ? 1.0f : xn[j0 + k]; }
                    }
                }
#pragma unroll
                for (int k = 0; k < MB_CK; ++k) {
                    a0 = fmaf(q[k].x, xj[k], a0); a1 = fmaf(q[k].y, xj[k], a1);
                    a2 = fmaf(q[k].z, xj[k], a2); a3 = fmaf(q[k].w, xj[k], a3);
                    float d = q[k].x * t0;
                    d = fmaf(q[k].y, t1, d); d = fmaf(q[k].z, t2, d); d = fmaf(q[k].w, t3, d);
                    d = wave_sum_dpp(d);
                    if (lane == 0 && k < nj) gp[r * CB + (j0 + k - cb0)] = d;
                }
            }
            // the unit's row sums: (s, row) is this lane's alone
            float *hs = hp + s * m + row;
            if (cb0 == 0) {
                if (in0) hs[0] = a0;
                if (in1) hs[1] = a1;
                if (in2) hs[2] = a2;
                if (in3) hs[3] = a3;
            } else {
                if (in0) hs[0] += a0;
                if (in1) hs[1] += a1;
                if (in2) hs[2] += a2;
                if (in3) hs[3] += a3;
            }
        }
        __syncthreads();
        for (int t = tid; t < cbn; t += T) {
            float acc = gp[t];
            for (int r = 1; r < R; ++r) acc += gp[r * CB + t];
            g[cb0 + t] = acc;
        }
        __syncthreads();
    }
    for (int i = tid; i < m; i += T) {
        float acc = hp[i];
        for (int s = 1; s < S; ++s) acc += hp[s * m + i];
        h[i] = acc;
    }
    __syncthreads();
}

template <bool ABS>
__device__ __forceinline__ void mb_pass(const float *A, bool vec, int m, int n, const float *xn, const float *xt, float *h, float *g,
                                        float *hp, float *gp)
{
    if (vec) mb_pass_t<ABS, true>(A, m, n, xn, xt, h, g, hp, gp);
    else mb_pass_t<ABS, false>(A, m, n, xn, xt, h, g, hp, gp);
}

__device__ __forceinline__ bool mb_vec(const float *a, int m) { return (m & 3) == 0 && ((uintptr_t)a & 15u) == 0; }

extern __shared__ float mb_lds[];

// calc_norms, calc_precond and init_vecs (solver.rs:460-524) of one problem per workgroup, as smallbatch_init_k, with the |A| sums
// from one streamed pass
__global__ __launch_bounds__(1024) void midbatch_init_k(const MbArgs a)
{
    const int p = a.live ? a.live[blockIdx.x] : a.first + (int)blockIdx.x;
    const int n = a.n, m = a.m, T = (int)blockDim.x, tid = (int)threadIdx.x;
    const MbMap L(n, m);
    float *S = mb_lds;
    const SbSlot sl = a.slots[p];
    for (int i = tid; i < m; i += T) S[L.b + i] = sl.b[i];
    for (int i = tid; i < n; i += T) S[L.c + i] = sl.c[i];
    __syncthreads();
    float q[4] = { 0.0f, 0.0f, 0.0f, 0.0f };              // sum b^2, sum |b|, sum c^2, sum |c|
    for (int i = tid; i < m; i += T) { const float t = S[L.b + i]; q[0] = fmaf(t, t, q[0]); q[1] += fabsf(t); }
    for (int i = tid; i < n; i += T) { const float t = S[L.c + i]; q[2] = fmaf(t, t, q[2]); q[3] += fabsf(t); }
    block_sums<4>(q, S + L.sh);
    mb_pass<true>(sl.a, mb_vec(sl.a, m), m, n, nullptr, nullptr, S + L.h, S + L.g, S + L.hp, S + L.gp);      // |A| row / column sums
    float *ar = a.arena + (size_t)p * a.stride;
    float *gTx = ar + 4 * n + 6 * m, *gTy = gTx + n, *gTs = gTy + m, *gSv = gTs + m, *gcar = gSv + m;
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
    for (int i = tid; i < m + n; i += T) gcar[i] = 0.0f;            // A 0, A^T 0
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

__global__ __launch_bounds__(1024) void midbatch_k(const MbArgs a)
{
    const int p = a.live ? a.live[blockIdx.x] : a.first + (int)blockIdx.x;
    SbStatus *const gst = a.st + p;
    if (gst->stop != 0) return;
    const int n = a.n, m = a.m, T = (int)blockDim.x, tid = (int)threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6, nw = T >> 6;
    const bool comp = a.comp != 0;
    const MbMap L(n, m);
    float *S = mb_lds;
    float *const sh = S + L.sh, *const hp = S + L.hp, *const gp = S + L.gp;
    float *const xx = S + L.xx, *const u = S + L.u, *const kx = S + L.kx, *const ku = S + L.ku;
    float *const xy = S + L.xy, *const xs = S + L.xs, *const v = S + L.v, *const ky = S + L.ky, *const ks = S + L.ks, *const kv = S + L.kv;
    const float *const Tx = S + L.Tx, *const Ty = S + L.Ty, *const Ts = S + L.Ts, *const Sv = S + L.Sv;
    float *const hx = S + L.hx, *const gx = S + L.gx;
    const float *const b = S + L.b, *const c = S + L.c;
    float *const rxs = S + L.rxs, *const g = S + L.g, *const h = S + L.h;
    unsigned char *const cls = reinterpret_cast<unsigned char *>(S + L.cls);

    // ---- load ----
    const SbSlot sl = a.slots[p];
    const float *const A = sl.a;
    const bool vec = mb_vec(A, m);
    float *const ar = a.arena + (size_t)p * a.stride;
    {
        const int nstate = 6 * n + 10 * m;                 // the arena's order is the LDS order from xx on
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
        // ---- x += T o (-K^T y): h = A u, g = A^T v; c.u, b.v, and c.x_x, b.x_y of the iterate that is about to move ----
        float q[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        for (int i = tid; i < n; i += T) { q[0] = fmaf(c[i], u[i], q[0]); q[2] = fmaf(c[i], xx[i], q[2]); }
        for (int i = tid; i < m; i += T) { q[1] = fmaf(b[i], v[i], q[1]); q[3] = fmaf(b[i], xy[i], q[3]); }
        mb_pass<false>(A, vec, m, n, u, v, h, g, hp, gp);
        block_sums<4>(q, sh);
        const float cx_old = q[2], by_old = q[3];
        for (int i = tid; i < n; i += T) xx[i] = sb_comp_add(xx[i], Tx[i] * (g[i] + c[i] * kappa), kx, i, comp);
        for (int i = tid; i < m; i += T) {
            const unsigned char k = cls[i];
            const float oy = xy[i], os = xs[i];
            float ny = sb_comp_add(oy, Ty[i] * (b[i] * kappa - h[i]), ky, i, comp);
            float ns = sb_comp_add(os, Ts[i] * v[i], ks, i, comp);
            if (k == 1) { ny = fmaxf(ny, 0.0f); ns = fmaxf(ns, 0.0f); }
            else if (k == 0) { ns = 0.0f; }
            xy[i] = ny;
            xs[i] = ns;
            h[i] = oy;                                             // (rx_y is not needed: what sb_soc writes there is dropped)
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
                sb_soc(xy, h, beg, end, rot, lane);
                sb_soc(xs, rxs, beg, end, rot, lane);
            }
        }
        // ---- h = A x_x, g = A^T x_y of the new iterate: the criteria, and K rx = K x_k - 2 K x_{k+1} ----
        mb_pass<false>(A, vec, m, n, xx, xy, h, g, hp, gp);
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
        // ---- y += S o (-K rx) (ycrit_k), the pair carried on ----
        for (int i = tid; i < n; i += T) {
            const float gn = g[i];
            u[i] = sb_comp_add(u[i], Tx[i] * (-(gx[i] - 2.0f * gn) - c[i] * rtau), ku, i, comp);
            gx[i] = gn;
        }
        for (int i = tid; i < m; i += T) {
            const float hn = h[i];
            v[i] = sb_comp_add(v[i], Sv[i] * ((hx[i] - 2.0f * hn) + rxs[i] - b[i] * rtau), kv, i, comp);
            hx[i] = hn;
        }
        kappa = fminf(kappa + s_kappa * ((cx_old - 2.0f * cx) + (by_old - 2.0f * by)), 0.0f);     // solver.rs:566-567
        // ---- status_eval ----
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
        float *const gcar = ar + 5 * n + 9 * m;
        for (int i = tid; i < m + n; i += T) gcar[i] = hx[i];      // (gx follows hx)
    }
    if (tid == 0) {
        gst->tau = tau; gst->kappa = kappa; gst->r_tau = rtau; gst->iter = iter;
        gst->kind = kind; gst->cri[0] = cri0; gst->cri[1] = cri1; gst->cri[2] = cri2;
        gst->state = state;
        gst->stop = state != THIP_ST_RUNNING ? 1 : 0;
    }
}

size_t g_mb_bytes = 0;                      // device memory held by every thip_midbatch of the process

const ObText MB_TEXT = { "mid batch not initialised", "null mid batch", "a mid batch holds 1 .. 1048576 problems",
                         "a mid batch takes no PSD segment" };

int mb_threads_for(size_t n, size_t m) { return n * m <= 8192 ? 256 : 1024; }

// the shape rules (no device needed): the single source of the limit
int mb_check(size_t n, size_t m, size_t n_seg, const int32_t *seg_type, const int64_t *seg_len, std::vector<int> *cones,
             std::vector<unsigned char> *cls)
{
    if (m < 1 || m > MB_MAX_DIM || n < 1 || n > MB_MAX_DIM)
        return fail(THIP_E_INVALID, "a mid batch takes 1 <= m <= 4096 and 1 <= n <= 4096", __FILE__, __LINE__);
    THIP_RC(ob_segments(MB_TEXT, m, n_seg, seg_type, seg_len, cones, cls));
    if (MbMap((int)n, (int)m).bytes((int)m) > MB_LDS_MAX)
        return fail(THIP_E_INVALID, "the vectors of the problem (8 n + 13 m floats and 24 832 bytes) do not fit the LDS of one CU", __FILE__,
                    __LINE__);
    return 0;
}

}  // namespace

struct thip_midbatch : OwnBatch {
    std::vector<unsigned char> unaligned;   // per slot: the problem's A is not 16-byte aligned
    size_t n_unaligned = 0;
};

namespace {

int mb_attr()
{
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    std::call_once(once, [&]() {
        err = hipFuncSetAttribute(reinterpret_cast<const void *>(&midbatch_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MB_LDS_MAX);
        if (err == hipSuccess)
            err = hipFuncSetAttribute(reinterpret_cast<const void *>(&midbatch_init_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)MB_LDS_MAX);
    });
    THIP_TRY(err);
    return 0;
}

void mb_plan(OwnBatch *h)
{
    h->threads = h->forced ? h->forced : mb_threads_for(h->n, h->m);
    h->lds = MbMap((int)h->n, (int)h->m).bytes((int)h->m);
}

MbArgs mb_args(const OwnBatch *h)
{
    MbArgs a{};
    a.n = (int)h->n; a.m = (int)h->m; a.n_cones = (int)(h->cones.size() / 3);
    a.comp = h->par.state_arith == THIP_STATE_COMPENSATED; a.steps = 0; a.first = 0; a.live = nullptr;
    a.slots = h->slots; a.arena = h->arena; a.stride = h->stride; a.st = h->dst; a.cls = h->cls_dev; a.cones = h->cones_dev;
    a.eps_acc = h->par.eps_acc; a.eps_inf = h->par.eps_inf; a.eps_zero = h->par.eps_zero; a.max_iter = h->par.max_iter;
    return a;
}

int mb_launch_init(OwnBatch *h, int first, int count)
{
    MbArgs a = mb_args(h);
    a.first = first;
    hipLaunchKernelGGL(midbatch_init_k, dim3((unsigned)count), dim3((unsigned)h->threads), h->lds, ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

int mb_launch_run(OwnBatch *h, int count, int steps, const int *live)
{
    MbArgs a = mb_args(h);
    a.steps = steps;
    a.live = live;
    hipLaunchKernelGGL(midbatch_k, dim3((unsigned)count), dim3((unsigned)h->threads), h->lds, ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

}  // namespace

#define MB_NEED(h)                                                                  \
    do {                                                                            \
        if (!(h)) { THIP_NEED_INIT(); return fail(THIP_E_INVALID, MB_TEXT.uninit, __FILE__, __LINE__); } \
    } while (0)

extern "C" {

int thip_midbatch_fits(size_t n, size_t m, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                       size_t *host_lds_bytes, int *host_threads)
{
    THIP_RC(mb_check(n, m, n_seg, host_seg_type, host_seg_len, nullptr, nullptr));
    if (host_threads) *host_threads = mb_threads_for(n, m);
    if (host_lds_bytes) *host_lds_bytes = MbMap((int)n, (int)m).bytes((int)m);      // (the same for every workgroup size)
    return 0;
}

int thip_midbatch_destroy(thip_midbatch *h)
{
    if (!h) return 0;
    ob_destroy(h);
    delete h;
    return 0;
}

int thip_midbatch_create(size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b, const float *dev_vecs_c,
                         const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                         const thip_param *par, thip_midbatch **out)
{
    if (!out) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *out = nullptr;
    THIP_NEED_INIT();
    THIP_RC(ob_create_args(MB_TEXT, n_prob, dev_mats_a, dev_vecs_b, dev_vecs_c, dev_vecs_b_rowabs, par));
    thip_midbatch *h = new thip_midbatch();
    h->text = &MB_TEXT; h->total = &g_mb_bytes; h->launch_init = mb_launch_init; h->launch_run = mb_launch_run;
    // every refusal comes before the first allocation
    int rc = mb_check(n, m, n_seg, host_seg_type, host_seg_len, &h->cones, &h->cls);
    if (rc != 0) { delete h; return rc; }
    h->n = n; h->m = m; h->n_prob = n_prob;
    h->par = *par;
    h->stride = mb_stride(n, m);
    mb_plan(h);
    h->unaligned.assign(n_prob, 0);
    for (size_t p = 0; p < n_prob; ++p) {
        h->unaligned[p] = (((uintptr_t)(dev_mats_a + p * m * n)) & 15u) != 0;
        h->n_unaligned += h->unaligned[p];
    }
    rc = mb_attr();
    if (rc == 0) rc = ob_build(h, dev_mats_a, dev_vecs_b, dev_vecs_c, dev_vecs_b_rowabs);
    if (rc != 0) { thip_midbatch_destroy(h); return rc; }
    *out = h;
    return 0;
}

int thip_midbatch_set_param(thip_midbatch *h, const thip_param *par) { return ob_set_param(h, par); }

int thip_midbatch_init(thip_midbatch *h) { return ob_init(h, MB_TEXT); }

int thip_midbatch_run(thip_midbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{
    MB_NEED(h);
    return ob_run(h, max_steps, poll_every, host_status, false);
}

int thip_midbatch_run_until_any(thip_midbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{
    MB_NEED(h);
    return ob_run(h, max_steps, poll_every, host_status, true);
}

int thip_midbatch_status(thip_midbatch *h, int i, thip_status *host_status)
{
    MB_NEED(h);
    return ob_status(h, i, host_status);
}

int thip_midbatch_solution(thip_midbatch *h, int i, float *host_x, float *host_y)
{
    MB_NEED(h);
    return ob_solution(h, i, host_x, host_y);
}

int thip_midbatch_iterate(thip_midbatch *h, int i, float *host_x, float *host_y)
{
    MB_NEED(h);
    return ob_iterate(h, i, host_x, host_y);
}

int thip_midbatch_precond(thip_midbatch *h, int i, float *host_dp_tau, float *host_dp_sigma)
{
    MB_NEED(h);
    return ob_precond(h, i, host_dp_tau, host_dp_sigma);
}

int thip_midbatch_replace(thip_midbatch *h, int i, const float *dev_mat_a, const float *dev_vec_b, const float *dev_vec_c,
                          const float *dev_vec_b_rowabs)
{
    MB_NEED(h);
    THIP_RC(ob_replace(h, i, dev_mat_a, dev_vec_b, dev_vec_c, dev_vec_b_rowabs));
    const unsigned char un = ((uintptr_t)dev_mat_a & 15u) != 0;
    h->n_unaligned += un;
    h->n_unaligned -= h->unaligned[(size_t)i];
    h->unaligned[(size_t)i] = un;
    return 0;
}

int thip_midbatch_info(const thip_midbatch *h, thip_midbatch_info_t *host_info)
{
    if (!h || !host_info) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    thip_midbatch_info_t &o = *host_info;
    memset(&o, 0, sizeof(o));
    o.n_prob = (int32_t)h->n_prob; o.threads = h->threads; o.lds_bytes = (int32_t)h->lds; o.live = (int32_t)h->live.size();
    o.arena_bytes = h->stride * h->n_prob * sizeof(float);
    o.device_bytes = h->bytes;
    o.device_bytes_all = g_mb_bytes;
    o.launches = h->launches; o.workgroups = h->workgroups;
    o.load_bytes = ((h->m & 3) == 0 && h->n_unaligned == 0) ? 16 : 4;
    o.a_bytes_per_iter = 2 * h->m * h->n * sizeof(float);
    return 0;
}

int thip_test_midbatch_force_threads(thip_midbatch *h, int threads)
{
    if (!h) return fail(THIP_E_INVALID, "null mid batch", __FILE__, __LINE__);
    if (threads != 0 && threads != 256 && threads != 1024)
        return fail(THIP_E_INVALID, "the workgroup size is 256 or 1024 (0: by shape)", __FILE__, __LINE__);
    if (h->inited) return fail(THIP_E_INVALID, "thip_test_midbatch_force_threads comes before thip_midbatch_init", __FILE__, __LINE__);
    h->forced = threads;
    mb_plan(h);
    return 0;
}

}  // extern "C"
