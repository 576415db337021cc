// thip_ownbatch.h -- what the "every problem has its OWN A" batches share (thip_smallbatch.hip: A in LDS; thip_midbatch.hip,
// thip_sdpbatch.hip and thip_raggedbatch.hip: A streamed from memory, thip_midstream.h; thip_mid16batch.hip: a 16-bit copy of A that the
// family owns, streamed -- ObStore).
//   device: the launch arguments (ObArgs), the status block and the slot of a problem, the problem's scalars (ObScalars), the
//           init kernel's body (ob_init_body), the criteria sums and status_eval (ob_criteria_sums, ob_status_eval), and the
//           functions of the iteration that do not touch A (block_sums; thip_step.h: the arithmetic every loop shares).  The two recurrences -- three passes
//           from LDS, two carried passes from memory -- stay with their families.
//           The init body takes its b, c and row sums from the slot (init, replace; set_a: ObKeepA, which may keep the iterate) or
//           from a staging area (set_bc: ObTakeBc);
//           ownbatch_gather_k collects a range's x_x and x_y for one read-out (solutions).
//   host:   slots, arena, all 64-byte status blocks in one copy, the live list, replace as the init kernel on one slot, and the C
//           API itself: a family is a table (ObFamily: its words, its shape rule, its thread choice, its LDS map's size, its
//           kernels) and one OB_DEFINE_API line that emits its extern "C" entry points over the generic bodies below.
// Included once by each of the translation units: everything here is internal to the one that includes it.
#pragma once

#include "thip_common.h"
#include "thip_step.h"

#include <algorithm>
#include <mutex>
#include <stdio.h>
#include <string.h>
#include <vector>

namespace {

using namespace thip;

constexpr size_t OB_MAX_PROB = 1048576, OB_LDS_MAX = 163840;

struct SbStatus {                // 64 bytes, one per problem; the host copies all of them in one transfer
    int       stop;              // != 0: the problem's workgroup returns at entry
    int       state;             // THIP_ST_*
    int       kind, pad;
    long long iter;              // index of the iteration being / last executed
    float     cri[3];
    float     tau, kappa, norm_b, norm_c;
    float     t_tau, s_kappa;    // preconditioner entries of tau / kappa
    float     r_tau;
};
static_assert(sizeof(SbStatus) == 64, "SbStatus is copied as an array");

struct SbSlot { const float *a, *b, *c, *rowabs; };      // where problem p's data lives (rowabs may be NULL: |b|)

// what every kernel of every family is launched with: the family's shape words (ObShape: n, m; the small batch adds lda), then
// ObCounts and ObRest.  One text, two layouts: each family keeps the argument block its iteration kernel had before the families
// were merged, because the compiler allocates the kernel's scalar registers differently for another block.  smallbatch_k without
// its lda word behind m (computed in the kernel, or placed elsewhere) reloads 8 more spilled SGPRs in its product loops;
// midbatch_k and sdpbatch_k with an lda word they do not use reload 6 more.  Either costs 0.6 to 1.0 % (NOTEBOOK 19)
struct ObShape { int n, m; };
struct ObCounts {
    int n_cones, comp, steps;
    int first;                              // live == NULL: workgroup k serves problem first + k
};
struct ObRest {
    const int *live;                        // else problem live[k]
    const SbSlot *slots;
    float *arena; size_t stride;            // problem p's state: arena + p * stride
    SbStatus *st;
    const unsigned char *cls;               // 0 zero cone, 1 nonnegative, 2 member of a block cone
    const int *cones;                       // (beg, end, kind) per block cone: 0 second-order, 1 rotated, 1 + k a PSD cone of order k
    float eps_acc, eps_inf, eps_zero; long long max_iter;
};
template <class SHAPE> struct ObArgsT : SHAPE, ObCounts, ObRest {};
using ObArgs = ObArgsT<ObShape>;

// the problem this workgroup serves.  The fields by value, here and in ObLimits: smallbatch_k never hands out the address of its
// argument block, and the compiler then knows that the pointers it loads through it (the slot's A, b, c) are global -- with the
// address taken they become flat loads
__device__ __forceinline__ int ob_problem(const int *live, int first) { return live ? live[blockIdx.x] : first + (int)blockIdx.x; }

// the seam between the shared bodies and a batch's bookkeeping: which problem the workgroup serves, where that problem's block of
// the arena begins and how many floats it carries behind the preconditioner.  ObUniform: one stride for every problem (the three
// uniform families; the words are the ones the bodies held before the seam, at the places they held them).  The ragged batch
// (thip_raggedbatch.hip) hands in what it read from its problem's descriptor
struct ObUniform {
    template <class ARGS> __device__ __forceinline__ int problem(const ARGS &a) const { return ob_problem(a.live, a.first); }
    template <class ARGS> __device__ __forceinline__ float *block(const ARGS &a, int p) const { return a.arena + (size_t)p * a.stride; }
    template <class ARGS> __device__ __forceinline__ int carried(const ARGS &a, int n, int m) const { return (int)a.stride - (5 * n + 9 * m); }
};

// Q sums over the workgroup; every thread gets every result.  sh: 64 floats of LDS
template <int Q>
__device__ __forceinline__ void block_sums(float *q, float *sh)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int k = 0; k < Q; ++k) q[k] = wave_sum_dpp(q[k]);
    __syncthreads();                        // (the previous sums have been read)
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < Q; ++k) sh[w * 4 + k] = q[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        double a = 0.0;
        for (int j = 0; j < nw; ++j) a += (double)sh[j * 4 + k];
        q[k] = (float)a;
    }
}

// one cone by one wave, with rx <- rx - 2 x folded in: the factor in f32 (thip_step.h)
__device__ __forceinline__ void sb_soc(float *x, float *rx, int beg, int end, int rotated, int lane)
{
    __builtin_assume(rx != nullptr);
    soc_project<float, int, false>(x, rx, beg, end, rotated, lane, 64, nullptr);
}

// the scalars of a problem, held in registers across a launch: from its status block and back
struct ObScalars {
    float tau, kappa, rtau, norm_b, norm_c, t_tau, s_kappa;
    long long iter;
    int state, kind;
    float cri0, cri1, cri2;
    __device__ __forceinline__ void load(const SbStatus *g)
    {
        tau = g->tau; kappa = g->kappa; rtau = g->r_tau;
        norm_b = g->norm_b; norm_c = g->norm_c; t_tau = g->t_tau; s_kappa = g->s_kappa;
        iter = g->iter;
        state = THIP_ST_RUNNING; kind = g->kind;
        cri0 = g->cri[0]; cri1 = g->cri[1]; cri2 = g->cri[2];
    }
    __device__ __forceinline__ void store(SbStatus *g) const      // (one thread)
    {
        g->tau = tau; g->kappa = kappa; g->r_tau = rtau; g->iter = iter;
        g->kind = kind; g->cri[0] = cri0; g->cri[1] = cri1; g->cri[2] = cri2;
        g->state = state;
        g->stop = state != THIP_ST_RUNNING ? 1 : 0;
    }
};

// calc_norms, calc_precond and init_vecs (solver.rs:460-524) of problem p by one workgroup: init_sums_k / init_scalars_k /
// precond_k / group_min_k.  L: the family's LDS map (sh, b, c, g, h, Ty, Ts are used), S: the LDS.  abs_sums() leaves the row sums
// of |A| in S[L.h ..] and the column sums in S[L.g ..], visible to every thread on return.  product_group takes the minimum over
// every block cone, second-order or PSD.  What the family carries in the arena behind the preconditioner (the stride says how
// much) starts at zero: A 0, A^T 0.
// SRC: where b, c and the row sums come from and how the body ends.  ObSlotData, the init kernels': they are the slot's, the state
// starts at zero.  ObTakeBc (below), the set_bc kernels': they lie in a staging area and go into the handle's store, the A is the one
// the slot points at, and the iterate may stay -- one text, so a problem that takes a new (b, c) gets the |A| sums, the cone minima
// and the norms by the instructions an init on that data runs
struct ObSlotData {
    __device__ __forceinline__ SbSlot data(const SbSlot &sl, int, int, int, int, int) const { return sl; }
    __device__ __forceinline__ bool keeps() const { return false; }
    __device__ __forceinline__ void point(const SbSlot *, int, int, int, const SbSlot &) const {}
};

template <class ARGS, class MAP, class SUMS, class AT = ObUniform, class SRC = ObSlotData>
__device__ __forceinline__ void ob_init_body(const ARGS &a, int p, const MAP &L, float *S, const SUMS &abs_sums, const AT &at = AT(),
                                             const SRC &src = SRC())
{
    const int n = a.n, m = a.m, T = (int)blockDim.x, tid = (int)threadIdx.x;
    const SbSlot sl = a.slots[p];
    const SbSlot d = src.data(sl, p, n, m, T, tid);       // (a, b, c, rowabs as the body reads them)
    for (int i = tid; i < m; i += T) S[L.b + i] = d.b[i];
    for (int i = tid; i < n; i += T) S[L.c + i] = d.c[i];
    __syncthreads();
    float q[4] = { 0.0f, 0.0f, 0.0f, 0.0f };              // sum b^2, sum |b|, sum c^2, sum |c|
    for (int i = tid; i < m; i += T) { const float t = S[L.b + i]; q[0] = fmaf(t, t, q[0]); q[1] += fabsf(t); }
    for (int i = tid; i < n; i += T) { const float t = S[L.c + i]; q[2] = fmaf(t, t, q[2]); q[3] += fabsf(t); }
    block_sums<4>(q, S + L.sh);
    abs_sums(sl.a);
    float *ar = at.block(a, p);
    float *gTx = ar + 4 * n + 6 * m, *gTy = gTx + n, *gTs = gTy + m, *gSv = gTs + m, *gcar = gSv + m;
    for (int i = tid; i < n; i += T) {
        const float t = S[L.g + i] + fabsf(S[L.c + i]);
        gTx[i] = 1.0f / fmaxf(t, a.eps_zero);
    }
    for (int i = tid; i < m; i += T) {
        const float t = S[L.h + i] + (d.rowabs ? d.rowabs[i] : fabsf(S[L.b + i]));
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
    const bool keep = src.keeps();
    if (!keep) {
        for (int i = tid; i < 4 * n + 6 * m; i += T) ar[i] = 0.0f;      // init_vecs: x = 0, y = 0 (and the Kahan terms)
        const int ncar = at.carried(a, n, m);
        for (int i = tid; i < ncar; i += T) gcar[i] = 0.0f;
    } else {                                // the iterate and what is carried behind the preconditioner stay: the Kahan terms alone
        float *const gy = ar + 4 * n;
        for (int i = tid; i < 2 * n; i += T) ar[2 * n + i] = 0.0f;          // kx ku
        for (int i = tid; i < 3 * m; i += T) gy[3 * m + i] = 0.0f;          // ky ks kv
    }
    if (tid == 0) {
        SbStatus s;
        s.stop = 0; s.state = THIP_ST_RUNNING; s.kind = 0; s.pad = 0; s.iter = 0;
        s.cri[0] = s.cri[1] = s.cri[2] = 0.0f;
        s.tau = 1.0f; s.kappa = 0.0f; s.r_tau = 0.0f;
        if (keep) { s.tau = a.st[p].tau; s.kappa = a.st[p].kappa; }
        const float nb = sqrtf(q[0]), nc = sqrtf(q[2]);      // fr_norm (solver.rs:85-107)
        s.norm_b = sqrtf(nb * nb);
        s.norm_c = sqrtf(nc * nc);
        const float tau_tau = q[3] + q[1];
        s.t_tau = 1.0f / fmaxf(tau_tau, a.eps_zero);
        s.s_kappa = 1.0f / fmaxf(tau_tau, a.eps_zero);
        a.st[p] = s;
        src.point(a.slots, p, n, m, d);
    }
}

// the sums of the criteria of the iterate (x_x, x_y, x_s) given h = A x_x, g = A^T x_y: q <- ||p||^2, b.x_y, ||d||^2, c.x_x
// conv (tau > eps_zero) and rt (1 / tau then, else 1) are formed here, from tau, not handed in: the compiler then sees that rt is
// 1 / tau wherever conv holds.  p and d are crit_p's and crit_d's (thip_step.h), written out: those form conv and rt per call, which
// the compiler hoists out of a loop but not out of two -- one more division per iteration here
__device__ __forceinline__ void ob_criteria_sums(float *q, int n, int m, float tau, float eps_zero, const float *b, const float *c,
                                                 const float *xx, const float *xy, const float *xs, const float *h, const float *g,
                                                 float *sh)
{
    const int T = (int)blockDim.x, tid = (int)threadIdx.x;
    const bool conv = tau > eps_zero;
    const float rt = conv ? 1.0f / tau : 1.0f;
    q[0] = q[1] = q[2] = q[3] = 0.0f;
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
}

// where a problem stops (thip_param's fields; passed by value, see ob_problem)
struct ObLimits { float eps_acc, eps_inf, eps_zero; long long max_iter; };

// the verdict on those sums into s, whose tau is the new iterate's.  Uniform: every thread holds the same sums
__device__ __forceinline__ void ob_status_eval(ObScalars &s, const ObLimits a, float pp, float by, float dd, float cx)
{
    const StepVerdict o = step_verdict(s.tau, s.iter, s.norm_b, s.norm_c, a.eps_acc, a.eps_inf, a.eps_zero, a.max_iter, pp, by, dd, cx,
                                       s.state);
    s.kind = o.kind; s.cri0 = o.cri0; s.cri1 = o.cri1; s.cri2 = o.cri2;
    s.state = o.state;
}

// where the iterates a start kernel hands to its problems lie (thip_NAME_set_iterates): workgroup k's begins at stage + at[k], or
// (at == NULL: one shape) at stage + k * per.  A problem's part is x = (x_x, x_y, x_s, tau) and then y = (u, v, kappa), the layout
// thip_NAME_iterate writes
struct ObStart { const float *stage; const long long *at; long long per; };

__device__ __forceinline__ const float *ob_staged(const ObStart &s)
{
    return s.stage + (s.at ? s.at[blockIdx.x] : (long long)blockIdx.x * s.per);
}

// the status block of a problem that starts from a given iterate (one thread): iteration 0, running, nothing judged yet.  What init
// made of the problem's data -- the norms and the preconditioner's two scalars -- stays
__device__ __forceinline__ void ob_start_status(SbStatus *g, float tau, float kappa)
{
    g->tau = tau; g->kappa = kappa; g->r_tau = 0.0f;
    g->iter = 0; g->kind = 0;
    g->cri[0] = g->cri[1] = g->cri[2] = 0.0f;
    g->state = THIP_ST_RUNNING;
    g->stop = 0;
}

// what a set_bc kernel is handed beside the family's launch arguments (thip_NAME_set_bc).  s: where the workgroups' new data lies in
// the staging area, as a start kernel's iterates do; a problem's part is one word (!= 0: row sums follow) and then b (m), c (n) and
// the row sums that go with b (m; ignored when the word is 0).  store: the handle's own b / c / rowabs of every problem, problem p's
// 2 m + n floats (b, c, rowabs) at store + store_at[p], or (store_at == NULL: one shape) at store + p * store_per.  keep: the
// iterate stays
struct ObSetBc { ObStart s; float *store; const long long *store_at; long long store_per; int keep; };

// ob_init_body's SRC of a problem that takes a new (b, c) and keeps its A.  data: the workgroup copies its part of the staging area
// into the problem's place in the store and the body reads the staged values (the same floats).  keeps: keep == 0 is init's ending.
// keep != 0: the iterate as it lies in the arena stays -- x_x, x_y, x_s | u, v, and tau, kappa in the status block -- the Kahan
// terms go to zero and the status is that of a start: iteration 0, running, nothing judged; what a streamed family carries, A x_x
// and A^T x_y, stays too: it is a function of A and the iterate alone, the pair a start kernel would form again from them.
// point (one thread, last): the slot's b, c, rowabs point into the store from now on; its A pointer is not touched
struct ObTakeBc {
    ObSetBc sb;
    __device__ __forceinline__ float *place(int p) const { return sb.store + (sb.store_at ? sb.store_at[p] : (long long)p * sb.store_per); }
    __device__ __forceinline__ SbSlot data(const SbSlot &sl, int p, int n, int m, int T, int tid) const
    {
        const float *const part = ob_staged(sb.s);
        const bool has_r = reinterpret_cast<const int *>(part)[0] != 0;
        const float *const nb = part + 1, *const nc = nb + m, *const nr = nc + n;
        float *const kb = place(p), *const kc = kb + m, *const kr = kc + n;
        for (int i = tid; i < m; i += T) { kb[i] = nb[i]; if (has_r) kr[i] = nr[i]; }
        for (int i = tid; i < n; i += T) kc[i] = nc[i];
        return SbSlot{ sl.a, nb, nc, has_r ? nr : nullptr };
    }
    __device__ __forceinline__ bool keeps() const { return sb.keep != 0; }
    __device__ __forceinline__ void point(const SbSlot *slots, int p, int n, int m, const SbSlot &d) const
    {
        float *const kb = place(p);
        SbSlot ns;
        ns.a = d.a; ns.b = kb; ns.c = kb + m; ns.rowabs = d.rowabs ? kb + m + n : nullptr;
        const_cast<SbSlot *>(slots)[p] = ns;
    }
};

// what a set_a kernel is handed beside the family's launch arguments (thip_NAME_set_a).  The dense families' new A is already where
// the slot's `a` points when the kernel starts (the host copied it there) and s is unused; the sparse families' new values lie in the
// staging area, workgroup k's at s.stage + s.at[k], and a scatter launch ahead of the kernel has written them into the blob.
// keep: the iterate stays
struct ObSetA { ObStart s; int keep; };

// ob_init_body's SRC of a problem whose A has new values (the set_a kernels'): b, c and the row sums are the slot's, whatever it
// points at now -- caller memory, or the handle's store after a set_bc -- read, never moved; the slot is not rewritten.  keeps: as
// ObTakeBc's, taken from the call.  Unlike there the pair a streamed family carries depends on what changed: the kernel forms it
// again behind the body (thip_midstream.h: mb_seta_body)
struct ObKeepA {
    int keep;
    __device__ __forceinline__ SbSlot data(const SbSlot &sl, int, int, int, int, int) const { return sl; }
    __device__ __forceinline__ bool keeps() const { return keep != 0; }
    __device__ __forceinline__ void point(const SbSlot *, int, int, int, const SbSlot &) const {}
};

// x_x and x_y of the problems of a range from the arena into one buffer (thip_NAME_solutions): workgroup k serves problem first + k,
// whose block begins at arena + at[4 k] and whose n, m are at[4 k + 1], at[4 k + 2]; its x_x then x_y go to out + at[4 k + 3].
// at == NULL: one shape -- arena + (first + k) * stride, n, m, out + k * (n + m)
struct ObGather { const float *arena; const long long *at; size_t stride; int n, m, first; float *out; };

__global__ __launch_bounds__(256) void ownbatch_gather_k(const ObGather g)
{
    const long long k = blockIdx.x;
    const float *ar = g.at ? g.arena + g.at[4 * k] : g.arena + (size_t)(g.first + k) * g.stride;
    const int n = g.at ? (int)g.at[4 * k + 1] : g.n, m = g.at ? (int)g.at[4 * k + 2] : g.m;
    float *out = g.out + (g.at ? g.at[4 * k + 3] : k * (long long)(n + m));
    for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) out[i] = ar[i];
    for (int i = (int)threadIdx.x; i < m; i += (int)blockDim.x) out[n + i] = ar[4 * n + i];
}

// ---- the round calls on device memory (thip_NAME_set_bc_dev / _set_a_dev / _set_iterates_dev / _solutions_dev) -------------------
// Four kernels, each a launch of its own ahead of the family's set kernel: none writes a word that it or a kernel fused behind it
// reads, so a store never meets a (possibly scalar) load of the same word without a kernel boundary between them.

// one part of a range as the check and the copy kernels see it: n floats at src, which go to dst
struct ObDevRow { const float *src; float *dst; long long n; };

constexpr int OB_COPY_CHUNK = 4096;         // floats per workgroup of ownbatch_copy_a_k: 256 threads, four 16-byte moves each

// the scan the host cannot make: one workgroup and one verdict word per problem.  mode 0: row k's n floats at src are finite (v - v
// == 0; ob_seta_check's rule) or verdict[k] = 1.  mode 1: the float at src is a start's tau, the one at dst its kappa
// (ob_start_scalars' rule): 1 for a tau that is negative or not finite, 2 for a kappa that is positive or not finite.  Every word
// of the verdict is written
__global__ __launch_bounds__(256) void ownbatch_check_k(const ObDevRow *rows, int mode, int *verdict)
{
    const ObDevRow r = rows[blockIdx.x];
    const int T = (int)blockDim.x, tid = (int)threadIdx.x;
    if (mode == 1) {                        // (uniform: the mode is an argument)
        if (tid == 0) {
            const float tau = r.src[0], kappa = r.dst[0];
            int v = 0;
            if (!(tau >= 0.0f) || tau - tau != 0.0f) v = 1;
            else if (!(kappa <= 0.0f) || kappa - kappa != 0.0f) v = 2;
            verdict[blockIdx.x] = v;
        }
        return;
    }
    int bad = 0;
    long long done = 0;
    if (((uintptr_t)r.src & 15u) == 0) {
        const long long n4 = r.n >> 2;
        const float4 *s4 = reinterpret_cast<const float4 *>(r.src);
        for (long long i = tid; i < n4; i += T) {
            const float4 v = s4[i];
            bad |= (v.x - v.x != 0.0f) | (v.y - v.y != 0.0f) | (v.z - v.z != 0.0f) | (v.w - v.w != 0.0f);
        }
        done = n4 << 2;
    }
    for (long long i = done + tid; i < r.n; i += T) { const float v = r.src[i]; bad |= v - v != 0.0f; }
    bad = __syncthreads_or(bad);
    if (tid == 0) verdict[blockIdx.x] = bad != 0;
}

// the streaming copy: workgroup (k, j) moves floats j C .. of row k, C = OB_COPY_CHUNK, whatever allocations the rows lie in.  16-byte
// loads and stores where both sides of the chunk are 16-byte aligned (a chunk is a multiple of 16 bytes, so every chunk of a row
// is or none), 4-byte ones otherwise; the tail of the last chunk by 4-byte moves
__global__ __launch_bounds__(256) void ownbatch_copy_a_k(const ObDevRow *rows)
{
    const ObDevRow r = rows[blockIdx.x];
    const long long beg = (long long)blockIdx.y * OB_COPY_CHUNK;
    if (beg >= r.n) return;
    const int cnt = (int)(r.n - beg < OB_COPY_CHUNK ? r.n - beg : OB_COPY_CHUNK), tid = (int)threadIdx.x, T = (int)blockDim.x;
    const float *s = r.src + beg;
    float *d = r.dst + beg;
    int done = 0;
    if ((((uintptr_t)s | (uintptr_t)d) & 15u) == 0) {
        const int n4 = cnt >> 2;
        const float4 *s4 = reinterpret_cast<const float4 *>(s);
        float4 *d4 = reinterpret_cast<float4 *>(d);
        int i = tid;
        for (; i + 3 * T < n4; i += 4 * T) {                     // (a full chunk: the thread's four loads in flight together)
            const float4 a = s4[i], b = s4[i + T], c = s4[i + 2 * T], e = s4[i + 3 * T];
            d4[i] = a; d4[i + T] = b; d4[i + 2 * T] = c; d4[i + 3 * T] = e;
        }
        for (; i < n4; i += T) d4[i] = s4[i];
        done = n4 << 2;
    }
    for (int i = done + tid; i < cnt; i += T) d[i] = s[i];
}

// one problem's new b, c and row sums (r: NULL, none) into the staged form the set_bc kernels read (ob_setbc_pack's, at `to`)
struct ObBcRow { const float *b, *c, *r; float *to; int n, m; };

__global__ __launch_bounds__(256) void ownbatch_stage_bc_k(const ObBcRow *rows)
{
    const ObBcRow q = rows[blockIdx.x];
    const int T = (int)blockDim.x, tid = (int)threadIdx.x;
    if (tid == 0) reinterpret_cast<int *>(q.to)[0] = q.r != nullptr;
    float *const b = q.to + 1, *const c = b + q.m, *const r = c + q.n;
    for (int i = tid; i < q.m; i += T) { b[i] = q.b[i]; r[i] = q.r ? q.r[i] : 0.0f; }
    for (int i = tid; i < q.n; i += T) c[i] = q.c[i];
}

// ownbatch_gather_k with ob_finalize's rule and the state word: problem first + k's x_x to x + its place, its x_y to y + its place,
// its state to state[k] (each of x, y, state may be NULL).  at == NULL: one shape -- the places are k n and k m.  Else at holds, for
// EVERY problem p of the batch, (block, n, m, the x's before p, the y's before p), and x0, y0 are those of `first`.  The scaling is
// rt = 1 / tau, correctly rounded, then rt * v, when kind == 0 and the state is OK or ExcessIter; else the floats as they lie
struct ObGatherDev {
    const float *arena; const SbStatus *st; const long long *at; size_t stride; int n, m, first; long long x0, y0;
    float *x, *y; int *state;
};

__global__ __launch_bounds__(256) void ownbatch_gather_final_k(const ObGatherDev g)
{
    const long long k = blockIdx.x, p = g.first + k;
    const long long *const t = g.at ? g.at + 5 * p : nullptr;
    const float *ar = t ? g.arena + t[0] : g.arena + (size_t)p * g.stride;
    const int n = t ? (int)t[1] : g.n, m = t ? (int)t[2] : g.m;
    const int state = g.st[p].state, kind = g.st[p].kind;
    const bool scale = kind == 0 && (state == THIP_ST_OK || state == THIP_ST_EXCESS_ITER);
    const float rt = scale ? __fdiv_rn(1.0f, g.st[p].tau) : 1.0f;
    if (g.x) {
        float *out = g.x + (t ? t[3] - g.x0 : k * (long long)n);
        for (int i = (int)threadIdx.x; i < n; i += (int)blockDim.x) out[i] = scale ? __fmul_rn(rt, ar[i]) : ar[i];
    }
    if (g.y) {
        float *out = g.y + (t ? t[4] - g.y0 : k * (long long)m);
        for (int i = (int)threadIdx.x; i < m; i += (int)blockDim.x) out[i] = scale ? __fmul_rn(rt, ar[4 * n + i]) : ar[4 * n + i];
    }
    if (g.state && threadIdx.x == 0) g.state[k] = state;
}

__global__ void ownbatch_slots_k(SbSlot *slots, int n_prob, const float *a, const float *b, const float *c, const float *rowabs,
                                 size_t m, size_t n)
{
    for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < (size_t)n_prob; p += (size_t)gridDim.x * blockDim.x) {
        SbSlot s;
        s.a = a + p * m * n; s.b = b + p * m; s.c = c + p * n; s.rowabs = rowabs ? rowabs + p * m : nullptr;
        slots[p] = s;
    }
}

// ---- the host side ------------------------------------------------------------------------------------------------------------

// a family's words for its refusals
struct ObText { const char *uninit, *null_h, *count, *no_psd, *force_sizes, *force_late; };

// what the PSD cones of a layout add (all zero in a family that takes none)
struct ObPsd { int max_k = 0, n_psd = 0; size_t tail_bytes = 0; };

struct OwnBatch;

// a family that owns its matrix store -- a converted copy of every problem's A (the mid16 batch: 16-bit words) -- hands in these
// three.  create: allocates the whole store with ob_alloc (so no array handed to a _dev call may overlap it), records it in the
// handle (a_store, a_block, a_kind: `arg` is the create call's word for the stored form), converts every problem from the f32 stack
// at dev_mats_a and points every slot at its block; called once, behind ob_build, and the f32 stack is not referenced after it
// returns.  convert: the problems first .. first + count - 1 again, from `count` f32 matrices (m n floats each, column-major) that
// lie one after another in device memory at dev_src -- one launch for the range.  slot: the pointer problem p's slot holds
struct ObStore {
    int (*create)(OwnBatch *h, const float *dev_mats_a, int arg);
    int (*convert)(OwnBatch *h, int first, int count, const float *dev_src);
    const float *(*slot)(const OwnBatch *h, size_t p);
};

// a family: everything the generic API bodies below need to know about it
struct ObFamily {
    ObText text;
    int forced[3];                          // the workgroup sizes force_threads takes (0: no further one)
    bool streams;                           // A is read in place: the handle records which slots hold an unaligned one
    // the shape rule (no device needed), the single source of the family's limit.  On success *cones holds (beg, end, kind) per
    // block cone, *cls the class bytes and *psd what the PSD cones add (each may be null)
    int (*check)(size_t n, size_t m, size_t n_seg, const int32_t *seg_type, const int64_t *seg_len, std::vector<int> *cones,
                 std::vector<unsigned char> *cls, ObPsd *psd);
    int (*threads_for)(size_t n, size_t m);
    size_t (*lds_for)(size_t n, size_t m, int threads, const ObPsd &psd);
    size_t (*stride_for)(size_t n, size_t m);
    int (*launch)(const OwnBatch *h, bool run, const ObArgs &a, unsigned count);      // the init kernel or the iteration
    int (*start)(const OwnBatch *h, const ObArgs &a, const ObStart &s, unsigned count);      // the start kernel (NULL: by class)
    int (*setbc)(const OwnBatch *h, const ObArgs &a, const ObSetBc &s, unsigned count);      // the set_bc kernel (NULL: by class)
    // the set_a kernel (a sparse family: the scatter launch ahead of it; NULL: by class)
    int (*seta)(const OwnBatch *h, const ObArgs &a, const ObSetA &s, unsigned count);
    const void *kernels[12];                // every kernel that asks for more than 64 KiB of LDS
    // NULL, or the family OWNS its matrix store (ObStore, below): the slots' `a` point into it, never at caller memory
    const ObStore *store = nullptr;
    size_t total = 0;                       // device memory held by every handle of the family
    std::once_flag attr_once;
    hipError_t attr_err = hipSuccess;
};

// what a handle of any family is.  The arena holds, per problem, `stride` floats: xx u kx ku | xy xs v ky ks kv | Tx Ty Ts Sv and
// then whatever else the family carries
struct OwnBatch {
    ObFamily *fam = nullptr;
    size_t n = 0, m = 0, n_prob = 0;
    thip_param par{};
    std::vector<int> cones;
    std::vector<unsigned char> cls;
    int threads = 0, forced = 0;
    size_t lds = 0, stride = 0, bytes = 0;
    float *arena = nullptr;
    SbStatus *dst = nullptr, *hst = nullptr;
    SbSlot *slots = nullptr;
    int *live_dev = nullptr, *cones_dev = nullptr;
    unsigned char *cls_dev = nullptr;
    std::vector<int> live;
    bool inited = false;
    int64_t launches = 0, workgroups = 0;
    ObPsd psd;
    // where set_iterates packs its iterates (pinned host memory) and where it uploads them: grown on demand, the handle's
    void *stage = nullptr, *stage_host = nullptr; size_t stage_bytes = 0;
    // the handle's own b / c / rowabs of every problem, allocated by the first set_bc: problem p's 2 m_p + n_p floats at bc_at[p]
    // (bc_at_dev: the same on the device, for a handle of many shapes; NULL: p * (2 m + n))
    float *bc_store = nullptr; long long *bc_at_dev = nullptr;
    // the host's mirror of every slot's `a` pointer (create, replace): where set_a of a dense family copies a problem's new A
    // slot_base: the base of the allocation that pointer lies in (0: not asked yet; odd: the runtime does not know it, the slot is
    // on its own) -- two slots whose A happen to lie one behind the other in DIFFERENT allocations are never served by one copy
    std::vector<const float *> slot_a;
    std::vector<uintptr_t> slot_base;
    std::vector<unsigned char> unaligned;   // (a family that streams A) per slot: the problem's A is not 16-byte aligned
    size_t n_unaligned = 0;                 // how many: decides the load path info() reports
    // every device allocation of the handle (ob_alloc): what no array handed to a _dev call may overlap
    std::vector<std::pair<uintptr_t, size_t>> owned;
    // a handle of many shapes: solutions_dev's table of every problem (block, n, m, x's before, y's before), made by its first call
    long long *sol_at_dev = nullptr;
    // the tables the kernels of a _dev call read and the verdict words its check kernel writes: pinned host memory mapped into the
    // device's address space (tab_dev: the same bytes as the kernels address them), grown on demand -- NOT device memory, so that a
    // call which moves A in place allocates none
    void *tab_host = nullptr, *tab_dev = nullptr; size_t tab_bytes = 0;
    size_t last_h2d = 0, last_d2h = 0;      // what the last _dev call moved between host and device (thip_test_ownbatch_last_transfer)
    // a family that owns its matrix store (ObStore): the store, the bytes of one problem's block and the stored form
    void *a_store = nullptr; size_t a_block = 0; int a_kind = 0;
};

// the cone segments (no device needed).  On success *cones holds (beg, end, kind) per block cone -- kind 0: second-order, 1: rotated,
// 1 + k: a PSD cone of order k -- and *cls the class bytes.  psd_max: the largest PSD order the family takes (0: it takes no PSD
// segment and refuses one in its own words, tx.no_psd)
int ob_segments(const ObText &tx, size_t m, size_t n_seg, const int32_t *seg_type, const int64_t *seg_len, std::vector<int> *cones,
                std::vector<unsigned char> *cls, int psd_max = 0)
{
    if (n_seg && (!seg_type || !seg_len)) return fail(THIP_E_INVALID, "null cone segments", __FILE__, __LINE__);
    int64_t off = 0;
    if (cls) cls->assign(m, 2);
    for (size_t i = 0; i < n_seg; ++i) {
        const int64_t l = seg_len[i];
        if (l < 0 || seg_type[i] < 0 || seg_type[i] > THIP_CONE_PSD) return fail(THIP_E_INVALID, "bad cone segment", __FILE__, __LINE__);
        int kind = seg_type[i] == THIP_CONE_ROTSOC ? 1 : 0;
        if (seg_type[i] == THIP_CONE_PSD) {
            if (psd_max == 0) return fail(THIP_E_INVALID, tx.no_psd, __FILE__, __LINE__);
            int64_t k = 0;
            while (k <= psd_max && k * (k + 1) / 2 < l) ++k;
            if (k > psd_max) return fail(THIP_E_INVALID, "a PSD segment of an order above 64: the batch projects orders 1 .. 64", __FILE__, __LINE__);
            if (l == 0 || k * (k + 1) / 2 != l)
                return fail(THIP_E_INVALID, "a PSD segment of order k holds k (k + 1) / 2 rows, k >= 1: not a triangular number", __FILE__,
                            __LINE__);
            kind = 1 + (int)k;
        }
        if (off + l > (int64_t)m) return fail(THIP_E_INVALID, "cone segments do not cover m rows", __FILE__, __LINE__);
        if (seg_type[i] == THIP_CONE_ZERO || seg_type[i] == THIP_CONE_RPOS) {
            if (cls) for (int64_t r = 0; r < l; ++r) (*cls)[(size_t)(off + r)] = seg_type[i] == THIP_CONE_ZERO ? 0 : 1;
        } else if (cones) {
            cones->push_back((int)off); cones->push_back((int)(off + l)); cones->push_back(kind);
        }
        off += l;
    }
    if ((size_t)off != m) return fail(THIP_E_INVALID, "cone segments do not cover m rows", __FILE__, __LINE__);
    return 0;
}

int ob_alloc(OwnBatch *h, void **p, size_t bytes)
{
    THIP_TRY(hipMalloc(p, bytes));
    h->bytes += bytes; h->fam->total += bytes;
    h->owned.emplace_back((uintptr_t)*p, bytes);
    return 0;
}

void ob_plan(OwnBatch *h)
{
    h->threads = h->forced ? h->forced : h->fam->threads_for(h->n, h->m);
    h->lds = h->fam->lds_for(h->n, h->m, h->threads, h->psd);
}

ObArgs ob_args(const OwnBatch *h)
{
    ObArgs a{};
    a.n = (int)h->n; a.m = (int)h->m; a.n_cones = (int)(h->cones.size() / 3);
    a.comp = h->par.state_arith == THIP_STATE_COMPENSATED; a.steps = 0; a.first = 0; a.live = nullptr;
    a.slots = h->slots; a.arena = h->arena; a.stride = h->stride; a.st = h->dst; a.cls = h->cls_dev; a.cones = h->cones_dev;
    a.eps_acc = h->par.eps_acc; a.eps_inf = h->par.eps_inf; a.eps_zero = h->par.eps_zero; a.max_iter = h->par.max_iter;
    return a;
}

// the init kernel on the problems first .. first + count - 1
int ob_launch_init(OwnBatch *h, int first, int count)
{
    ObArgs a = ob_args(h);
    a.first = first;
    return h->fam->launch(h, false, a, (unsigned)count);
}

// `steps` iterations of `count` problems: those of the list, or (live == NULL) the first `count`
int ob_launch_run(OwnBatch *h, int count, int steps, const int *live)
{
    ObArgs a = ob_args(h);
    a.steps = steps;
    a.live = live;
    return h->fam->launch(h, true, a, (unsigned)count);
}

// what a family's launch hook does with the kernel it chose
template <class ARGS>
int ob_launch(const OwnBatch *h, void (*kernel)(ARGS), const ARGS &a, unsigned count)
{
    hipLaunchKernelGGL(kernel, dim3(count), dim3((unsigned)h->threads), h->lds, ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

// every kernel of the family may ask for the whole LDS of a CU (once per process)
int ob_attr(ObFamily &f)
{
    std::call_once(f.attr_once, [&]() {
        for (const void *k : f.kernels)
            if (k && f.attr_err == hipSuccess)
                f.attr_err = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)OB_LDS_MAX);
    });
    const hipError_t err = f.attr_err;
    THIP_TRY(err);
    return 0;
}

void ob_status_out(const SbStatus &s, thip_status *o)
{
    o->state = s.state; o->iter = s.iter; o->kind = s.kind;
    o->cri[0] = s.cri[0]; o->cri[1] = s.cri[1]; o->cri[2] = s.cri[2];
    o->tau = s.tau; o->kappa = s.kappa; o->norm_b = s.norm_b; o->norm_c = s.norm_c;
}

// every status block in one transfer; the live set from it
int ob_poll(OwnBatch *h, thip_status *host_status)
{
    hipStream_t st = ctx().stream;
    THIP_TRY(hipMemcpyAsync(h->hst, h->dst, h->n_prob * sizeof(SbStatus), hipMemcpyDeviceToHost, st));
    THIP_TRY(hipStreamSynchronize(st));
    h->live.clear();
    for (size_t p = 0; p < h->n_prob; ++p) {
        if (h->hst[p].state == THIP_ST_RUNNING) h->live.push_back((int)p);
        if (host_status) ob_status_out(h->hst[p], host_status + p);
    }
    return 0;
}

int ob_run(const ObFamily &f, OwnBatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status, bool until_any)
{
    THIP_NEED_INIT();
    if (!h || !h->inited) return fail(THIP_E_INVALID, f.text.uninit, __FILE__, __LINE__);
    if (poll_every <= 0) poll_every = 16;
    hipStream_t st = ctx().stream;
    THIP_RC(ob_poll(h, host_status));
    const size_t live0 = h->live.size();
    int64_t done = 0;
    while (!h->live.empty() && (max_steps < 0 || done < max_steps) && !(until_any && h->live.size() < live0)) {
        int64_t batch = poll_every;
        if (max_steps >= 0 && done + batch > max_steps) batch = max_steps - done;
        if (batch > 1 << 20) batch = 1 << 20;
        const bool all = h->live.size() == h->n_prob;          // (then workgroup k serves problem k: no list)
        if (!all) THIP_TRY(hipMemcpyAsync(h->live_dev, h->live.data(), h->live.size() * sizeof(int), hipMemcpyHostToDevice, st));
        THIP_RC(ob_launch_run(h, (int)h->live.size(), (int)batch, all ? nullptr : h->live_dev));
        h->launches += 1;
        h->workgroups += (int64_t)h->live.size();
        done += batch;
        THIP_RC(ob_poll(h, host_status));       // (synchronises: the list the launch read is the host's to rewrite)
    }
    return 0;
}

int ob_member(const ObFamily &f, OwnBatch *h, int i)
{
    if (!h || !h->inited) return fail(THIP_E_INVALID, f.text.uninit, __FILE__, __LINE__);
    if (i < 0 || (size_t)i >= h->n_prob) return fail(THIP_E_INVALID, "no such problem", __FILE__, __LINE__);
    return 0;
}

// problem i's status block, fresh from the device
int ob_status_one(OwnBatch *h, int i)
{
    hipStream_t st = ctx().stream;
    THIP_TRY(hipMemcpyAsync(h->hst + i, h->dst + i, sizeof(SbStatus), hipMemcpyDeviceToHost, st));
    THIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// the final 1/tau scaling of a terminated iterate (solver.rs:397-400; finalize_k), applied to the copy that is read
void ob_finalize(const SbStatus &s, float *x, size_t n)
{
    const bool scale = (s.kind == 0) && (s.state == THIP_ST_OK || s.state == THIP_ST_EXCESS_ITER);
    if (!scale || !x) return;
    const float rt = 1.0f / s.tau;
    for (size_t i = 0; i < n; ++i) x[i] = rt * x[i];
}

// (H: the family's handle type, which is what is deleted)
template <class H>
int ob_destroy(H *h)
{
    if (!h) return 0;
    if (ctx().inited) hipStreamSynchronize(ctx().stream);
    hipFree(h->arena); hipFree(h->dst); hipFree(h->slots); hipFree(h->live_dev); hipFree(h->cones_dev); hipFree(h->cls_dev);
    hipFree(h->stage); hipFree(h->bc_store); hipFree(h->bc_at_dev); hipFree(h->sol_at_dev); hipFree(h->a_store);
    if (h->stage_host) hipHostFree(h->stage_host);
    if (h->tab_host) hipHostFree(h->tab_host);
    if (h->hst) hipHostFree(h->hst);
    h->fam->total -= h->bytes;
    delete h;
    return 0;
}

// everything a handle holds on the device (n, m, n_prob, stride, cones and cls are set)
int ob_build(OwnBatch *h, const float *a, const float *b, const float *c, const float *rowabs)
{
    hipStream_t st = ctx().stream;
    const size_t n_prob = h->n_prob, m = h->m;
    h->slot_a.assign(n_prob, nullptr);
    h->slot_base.assign(n_prob, 0);
    for (size_t p = 0; a && p < n_prob; ++p) h->slot_a[p] = a + p * m * h->n;      // (ownbatch_slots_k's rule)
    THIP_RC(ob_alloc(h, (void **)&h->arena, h->stride * n_prob * sizeof(float)));
    THIP_RC(ob_alloc(h, (void **)&h->dst, n_prob * sizeof(SbStatus)));
    THIP_RC(ob_alloc(h, (void **)&h->slots, n_prob * sizeof(SbSlot)));
    THIP_RC(ob_alloc(h, (void **)&h->live_dev, n_prob * sizeof(int)));
    THIP_RC(ob_alloc(h, (void **)&h->cls_dev, (m + 3) & ~(size_t)3));
    THIP_RC(ob_alloc(h, (void **)&h->cones_dev, std::max<size_t>(h->cones.size(), 3) * sizeof(int)));
    THIP_TRY(hipHostMalloc((void **)&h->hst, n_prob * sizeof(SbStatus), hipHostMallocDefault));
    THIP_TRY(hipMemcpy(h->cls_dev, h->cls.data(), m, hipMemcpyHostToDevice));
    if (!h->cones.empty()) THIP_TRY(hipMemcpy(h->cones_dev, h->cones.data(), h->cones.size() * sizeof(int), hipMemcpyHostToDevice));
    THIP_TRY(hipMemsetAsync(h->dst, 0, n_prob * sizeof(SbStatus), st));
    hipLaunchKernelGGL(ownbatch_slots_k, dim3(grid_for(n_prob, 256, 1024)), dim3(256), 0, st, h->slots, (int)n_prob, a, b, c, rowabs, m,
                       h->n);
    THIP_LAUNCH_CHECK();
    return 0;
}

int ob_set_param(OwnBatch *h, const thip_param *par)
{
    if (!h || !par) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (par->state_arith != THIP_STATE_COMPENSATED && par->state_arith != THIP_STATE_PLAIN)
        return fail(THIP_E_INVALID, "bad thip_param.state_arith", __FILE__, __LINE__);
    h->par = *par;
    return 0;
}

int ob_init(const ObFamily &f, OwnBatch *h)
{
    THIP_NEED_INIT();
    if (!h) return fail(THIP_E_INVALID, f.text.null_h, __FILE__, __LINE__);
    THIP_RC(ob_launch_init(h, 0, (int)h->n_prob));
    h->launches = 0; h->workgroups = 0;
    h->inited = true;
    return ob_poll(h, nullptr);
}

int ob_status(const ObFamily &f, OwnBatch *h, int i, thip_status *host_status)
{
    THIP_NEED_INIT();
    THIP_RC(ob_member(f, h, i));
    if (!host_status) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    THIP_RC(ob_status_one(h, i));
    ob_status_out(h->hst[i], host_status);
    return 0;
}

// solution, iterate and precond of problem i, whose block of the arena is ar and whose shape is n, m (the _at forms: a handle of one
// shape passes its own, the ragged batch the problem's)
int ob_solution_at(OwnBatch *h, int i, const float *ar, size_t n, size_t m, float *host_x, float *host_y)
{
    THIP_RC(ob_status_one(h, i));
    if (host_x) THIP_RC(thip_d2h(host_x, ar, n));
    if (host_y) THIP_RC(thip_d2h(host_y, ar + 4 * n, m));
    ob_finalize(h->hst[i], host_x, n);
    ob_finalize(h->hst[i], host_y, m);
    return 0;
}

int ob_iterate_at(OwnBatch *h, int i, const float *ar, size_t n, size_t m, float *host_x, float *host_y)
{
    THIP_RC(ob_status_one(h, i));                            // ar: xx u kx ku | xy xs v ..
    if (host_x) {
        THIP_RC(thip_d2h(host_x, ar, n));
        THIP_RC(thip_d2h(host_x + n, ar + 4 * n, 2 * m));
        host_x[n + m + m] = h->hst[i].tau;
        ob_finalize(h->hst[i], host_x, n + m);              // (x_x and x_y are adjacent in the copy)
    }
    if (host_y) {
        THIP_RC(thip_d2h(host_y, ar + n, n));
        THIP_RC(thip_d2h(host_y + n, ar + 4 * n + 2 * m, m));
        host_y[n + m] = h->hst[i].kappa;
    }
    return 0;
}

int ob_precond_at(OwnBatch *h, int i, const float *ar, size_t n, size_t m, float *host_dp_tau, float *host_dp_sigma)
{
    THIP_RC(ob_status_one(h, i));
    const float *k = ar + 4 * n + 6 * m;                                    // Tx Ty Ts Sv
    if (host_dp_tau) {
        THIP_RC(thip_d2h(host_dp_tau, k, n + 2 * m));
        host_dp_tau[n + 2 * m] = h->hst[i].t_tau;
    }
    if (host_dp_sigma) {
        THIP_RC(thip_d2h(host_dp_sigma, k, n));                             // sigma_n = tau_x
        THIP_RC(thip_d2h(host_dp_sigma + n, k + n + 2 * m, m));
        host_dp_sigma[n + m] = h->hst[i].s_kappa;
    }
    return 0;
}

int ob_solution(const ObFamily &f, OwnBatch *h, int i, float *host_x, float *host_y)
{
    THIP_NEED_INIT();
    THIP_RC(ob_member(f, h, i));
    return ob_solution_at(h, i, h->arena + (size_t)i * h->stride, h->n, h->m, host_x, host_y);
}

int ob_iterate(const ObFamily &f, OwnBatch *h, int i, float *host_x, float *host_y)
{
    THIP_NEED_INIT();
    THIP_RC(ob_member(f, h, i));
    return ob_iterate_at(h, i, h->arena + (size_t)i * h->stride, h->n, h->m, host_x, host_y);
}

int ob_precond(const ObFamily &f, OwnBatch *h, int i, float *host_dp_tau, float *host_dp_sigma)
{
    THIP_NEED_INIT();
    THIP_RC(ob_member(f, h, i));
    return ob_precond_at(h, i, h->arena + (size_t)i * h->stride, h->n, h->m, host_dp_tau, host_dp_sigma);
}

int ob_dev_foreign(const OwnBatch *h, const void *p, size_t bytes, const char *what);      // (below, with the _dev calls)

int ob_replace(const ObFamily &f, OwnBatch *h, int i, const float *dev_mat_a, const float *dev_vec_b, const float *dev_vec_c, const float *dev_vec_b_rowabs)
{
    THIP_NEED_INIT();
    THIP_RC(ob_member(f, h, i));
    if (!dev_mat_a || !dev_vec_b || !dev_vec_c) return fail(THIP_E_INVALID, "null A, b or c", __FILE__, __LINE__);
    if (((uintptr_t)dev_mat_a | (uintptr_t)dev_vec_b | (uintptr_t)dev_vec_c | (uintptr_t)dev_vec_b_rowabs) & 3u)
        return fail(THIP_E_INVALID, "the arrays hold floats: 4-byte alignment", __FILE__, __LINE__);
    if (f.store) {                          // the new A goes into slot i's block of the store, which the slot keeps pointing at
        THIP_RC(ob_dev_foreign(h, dev_mat_a, h->m * h->n * sizeof(float), "dev_mat_a"));
        THIP_RC(f.store->convert(h, i, 1, dev_mat_a));
        dev_mat_a = f.store->slot(h, (size_t)i);
    }
    const SbSlot s{ dev_mat_a, dev_vec_b, dev_vec_c, dev_vec_b_rowabs };
    THIP_TRY(hipMemcpyAsync(h->slots + i, &s, sizeof(SbSlot), hipMemcpyHostToDevice, ctx().stream));
    THIP_TRY(hipStreamSynchronize(ctx().stream));           // (s is a local)
    THIP_RC(ob_launch_init(h, i, 1));
    const auto at = std::lower_bound(h->live.begin(), h->live.end(), i);
    if (at == h->live.end() || *at != i) h->live.insert(at, i);
    THIP_RC(ob_status_one(h, i));
    if (!h->slot_a.empty()) { h->slot_a[(size_t)i] = dev_mat_a; h->slot_base[(size_t)i] = 0; }
    if (f.streams) {
        const unsigned char un = ((uintptr_t)dev_mat_a & 15u) != 0;
        h->n_unaligned += un;
        h->n_unaligned -= h->unaligned[(size_t)i];
        h->unaligned[(size_t)i] = un;
    }
    return 0;
}

// tau and kappa of a start: the last entries of x and y
int ob_start_scalars(const float *x, const float *y, size_t n, size_t m)
{
    const float tau = x[n + 2 * m], kappa = y[n + m];
    if (!(tau >= 0.0f) || tau - tau != 0.0f) return fail(THIP_E_INVALID, "a start's tau is finite and not negative", __FILE__, __LINE__);
    if (!(kappa <= 0.0f) || kappa - kappa != 0.0f) return fail(THIP_E_INVALID, "a start's kappa is finite and not positive", __FILE__, __LINE__);
    return 0;
}

// every refusal of a start that needs no shape
int ob_start_range(const ObFamily &f, const OwnBatch *h, int first, int count, const float *host_x, const float *host_y)
{
    if (!h) return fail(THIP_E_INVALID, f.text.null_h, __FILE__, __LINE__);
    if (!h->inited) return fail(THIP_E_INVALID, f.text.uninit, __FILE__, __LINE__);
    if (!host_x || !host_y) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (count < 1 || first < 0 || (size_t)first + (size_t)count > h->n_prob)
        return fail(THIP_E_INVALID, "no such range of problems", __FILE__, __LINE__);
    return 0;
}

// `bytes` of staging for a start: a device buffer (counted in device_bytes) and its pinned twin on the host, both the handle's, freed
// by destroy and grown to the largest call -- a start per slot, replace(start=) in a loop, pays no allocation, and the one upload
// is a DMA from the memory the iterates were packed into.  *host: where the caller packs
int ob_stage_reserve(OwnBatch *h, size_t bytes, void **host)
{
    if (h->stage_bytes < bytes) {
        THIP_TRY(hipStreamSynchronize(ctx().stream));
        THIP_TRY(hipFree(h->stage));
        h->owned.erase(std::remove_if(h->owned.begin(), h->owned.end(), [&](const std::pair<uintptr_t, size_t> &o) { return o.first == (uintptr_t)h->stage; }),
                       h->owned.end());
        h->stage = nullptr;
        if (h->stage_host) THIP_TRY(hipHostFree(h->stage_host));
        h->stage_host = nullptr;
        h->bytes -= h->stage_bytes; h->fam->total -= h->stage_bytes;
        h->stage_bytes = 0;
        THIP_TRY(hipHostMalloc(&h->stage_host, bytes, hipHostMallocDefault));
        THIP_RC(ob_alloc(h, &h->stage, bytes));
        h->stage_bytes = bytes;
    }
    *host = h->stage_host;
    return 0;
}

// the host's books behind the kernels that start problems again: the problems first .. first + count - 1 are running, their status
// blocks fresh (synchronises)
int ob_restarted(OwnBatch *h, int first, int count)
{
    hipStream_t st = ctx().stream;
    THIP_TRY(hipMemcpyAsync(h->hst + first, h->dst + first, (size_t)count * sizeof(SbStatus), hipMemcpyDeviceToHost, st));
    THIP_TRY(hipStreamSynchronize(st));
    std::vector<int> merged;                                     // (the live list is sorted: the range goes in as one run)
    merged.reserve(h->live.size() + (size_t)count);
    for (int p : h->live) if (p < first) merged.push_back(p);
    for (int p = first; p < first + count; ++p) merged.push_back(p);
    for (int p : h->live) if (p >= first + count) merged.push_back(p);
    h->live.swap(merged);
    return 0;
}

// the `bytes` packed into the handle's pinned buffer up, `launch` (the start kernels on them), and the host's books: the problems
// first .. first + count - 1 are running again, their status blocks fresh
template <class LAUNCH>
int ob_start_staged(OwnBatch *h, int first, int count, size_t bytes, const LAUNCH &launch)
{
    hipStream_t st = ctx().stream;
    void *const stage = h->stage;
    THIP_TRY(hipMemcpyAsync(stage, h->stage_host, bytes, hipMemcpyHostToDevice, st));
    const int rc = launch(stage);
    if (rc != 0) { hipStreamSynchronize(st); return rc; }      // (the copy may still be reading the pinned buffer)
    return ob_restarted(h, first, count);
}

// thip_NAME_set_iterates of a family of one shape: one upload, one launch
int ob_set_iterates(const ObFamily &f, OwnBatch *h, int first, int count, const float *host_x, const float *host_y)
{
    THIP_NEED_INIT();
    THIP_RC(ob_start_range(f, h, first, count, host_x, host_y));
    const size_t n = h->n, m = h->m, nx = n + 2 * m + 1, ny = n + m + 1, per = nx + ny;
    for (int k = 0; k < count; ++k) THIP_RC(ob_start_scalars(host_x + (size_t)k * nx, host_y + (size_t)k * ny, n, m));
    const size_t bytes = per * (size_t)count * sizeof(float);
    void *pinned = nullptr;
    THIP_RC(ob_stage_reserve(h, bytes, &pinned));
    float *const host = static_cast<float *>(pinned);
    for (int k = 0; k < count; ++k) {
        memcpy(host + (size_t)k * per, host_x + (size_t)k * nx, nx * sizeof(float));
        memcpy(host + (size_t)k * per + nx, host_y + (size_t)k * ny, ny * sizeof(float));
    }
    return ob_start_staged(h, first, count, bytes, [&](const void *stage) {
        ObArgs a = ob_args(h);
        a.first = first;
        return f.start(h, a, ObStart{ static_cast<const float *>(stage), nullptr, (long long)per }, (unsigned)count);
    });
}

// every refusal of a set_bc that needs no shape
int ob_setbc_range(const ObFamily &f, const OwnBatch *h, int first, int count, const float *host_b, const float *host_c)
{
    if (!h) return fail(THIP_E_INVALID, f.text.null_h, __FILE__, __LINE__);
    if (!h->inited) return fail(THIP_E_INVALID, f.text.uninit, __FILE__, __LINE__);
    if (!host_b || !host_c) return fail(THIP_E_INVALID, "null b or c", __FILE__, __LINE__);
    if (count < 1 || first < 0 || (size_t)first + (size_t)count > h->n_prob)
        return fail(THIP_E_INVALID, "no such range of problems", __FILE__, __LINE__);
    return 0;
}

// the handle's own b / c / rowabs store, allocated by the first set_bc that is taken: `floats` for the whole batch, and (at != NULL:
// a handle of many shapes) where each problem's part begins
int ob_setbc_store(OwnBatch *h, size_t floats, const std::vector<long long> *at)
{
    if (h->bc_store) return 0;
    if (at) {                               // (the offsets first: the store, which says that both are there, comes last)
        if (!h->bc_at_dev) THIP_RC(ob_alloc(h, (void **)&h->bc_at_dev, at->size() * sizeof(long long)));
        THIP_TRY(hipMemcpy(h->bc_at_dev, at->data(), at->size() * sizeof(long long), hipMemcpyHostToDevice));
    }
    return ob_alloc(h, (void **)&h->bc_store, floats * sizeof(float));
}

// one problem's part of a set_bc upload at `to`, 1 + 2 m + n floats: the word, b, c and the row sums.  r: the problem's row sums or
// NULL
void ob_setbc_pack(float *to, size_t n, size_t m, const float *b, const float *c, const float *r)
{
    const int has = r != nullptr;
    memcpy(to, &has, sizeof(int));
    memcpy(to + 1, b, m * sizeof(float));
    memcpy(to + 1 + m, c, n * sizeof(float));
    if (r) memcpy(to + 1 + m + n, r, m * sizeof(float));
    else memset(to + 1 + m + n, 0, m * sizeof(float));
}

// thip_NAME_set_bc of a family of one shape: one upload, one launch
int ob_set_bc(const ObFamily &f, OwnBatch *h, int first, int count, const float *host_b, const float *host_c, const float *host_r,
              const uint8_t *host_has, int keep)
{
    THIP_NEED_INIT();
    THIP_RC(ob_setbc_range(f, h, first, count, host_b, host_c));
    const size_t n = h->n, m = h->m, per = 1 + 2 * m + n, bytes = per * (size_t)count * sizeof(float);
    THIP_RC(ob_setbc_store(h, (2 * m + n) * h->n_prob, nullptr));
    void *pinned = nullptr;
    THIP_RC(ob_stage_reserve(h, bytes, &pinned));
    float *const host = static_cast<float *>(pinned);
    for (int k = 0; k < count; ++k) {
        const bool has = host_r && (!host_has || host_has[k]);
        ob_setbc_pack(host + (size_t)k * per, n, m, host_b + (size_t)k * m, host_c + (size_t)k * n, has ? host_r + (size_t)k * m : nullptr);
    }
    return ob_start_staged(h, first, count, bytes, [&](const void *stage) {
        ObArgs a = ob_args(h);
        a.first = first;
        const ObSetBc s{ ObStart{ static_cast<const float *>(stage), nullptr, (long long)per }, h->bc_store, nullptr,
                         (long long)(2 * m + n), keep != 0 };
        return f.setbc(h, a, s, (unsigned)count);
    });
}

// every refusal of a set_a, before anything is uploaded or touched: the handle, the range, each problem's count (host_counts, or NULL:
// the values are need(p) per problem, one after another) and every value finite (spb_validate's rule; an explicit zero is a value).
// what: the family's words for what a problem's count is.  *total: the floats host_values holds
constexpr const char *OB_SETA_DENSE = "its m n entries are needed";
constexpr const char *OB_SETA_SPARSE = "its stored entries are needed (another pattern: _replace)";

template <class NEED>
int ob_seta_check(const ObFamily &f, const OwnBatch *h, int first, int count, const float *host_values, const int64_t *host_counts,
                  const NEED &need, const char *what, size_t *total)
{
    if (!h) return fail(THIP_E_INVALID, f.text.null_h, __FILE__, __LINE__);
    if (!h->inited) return fail(THIP_E_INVALID, f.text.uninit, __FILE__, __LINE__);
    if (count < 1 || first < 0 || (size_t)first + (size_t)count > h->n_prob)
        return fail(THIP_E_INVALID, "no such range of problems", __FILE__, __LINE__);
    char msg[160];
    size_t sum = 0;
    for (int k = 0; k < count; ++k) {
        const size_t want = need(first + k);
        if (host_counts && (host_counts[k] < 0 || (size_t)host_counts[k] != want)) {
            snprintf(msg, sizeof(msg), "problem %d: %lld values of A where %zu, %s", first + k, (long long)host_counts[k], want, what);
            return fail(THIP_E_INVALID, msg, __FILE__, __LINE__);
        }
        sum += want;
    }
    if (sum && !host_values) return fail(THIP_E_INVALID, "null values of A", __FILE__, __LINE__);
    const float *v = host_values;
    for (int k = 0; k < count; ++k) {
        const size_t want = need(first + k);
        for (size_t e = 0; e < want; ++e)
            if (v[e] - v[e] != 0.0f) {
                snprintf(msg, sizeof(msg), "problem %d: a value of A is not finite", first + k);
                return fail(THIP_E_INVALID, msg, __FILE__, __LINE__);
            }
        v += want;
    }
    *total = sum;
    return 0;
}

// the allocation slot p's A lies in, asked of the runtime once per slot and pointer
uintptr_t ob_slot_base(OwnBatch *h, size_t p)
{
    if (h->slot_base[p] == 0) {
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)const_cast<float *>(h->slot_a[p])) == hipSuccess && base && !((uintptr_t)base & 1u))
            h->slot_base[p] = (uintptr_t)base;
        else {
            (void)hipGetLastError();
            h->slot_base[p] = ((uintptr_t)p << 1) | 1u;
        }
    }
    return h->slot_base[p];
}

// the new A of the problems first .. first + count - 1 of a dense family from the host straight to where their slots' `a` point, one
// copy per run of slots that lie one behind the other in one allocation (a batch as created is one run).  floats(p): problem p's m n
template <class FLOATS>
int ob_seta_copy(OwnBatch *h, int first, int count, const float *host_values, const FLOATS &floats)
{
    hipStream_t st = ctx().stream;
    const float *src = host_values;
    for (int k = 0; k < count;) {
        const float *const to = h->slot_a[(size_t)(first + k)];
        size_t run = floats(first + k);
        int j = k + 1;
        while (j < count && h->slot_a[(size_t)(first + j)] == to + run && ob_slot_base(h, (size_t)(first + j)) == ob_slot_base(h, (size_t)(first + k))) {
            run += floats(first + j);
            ++j;
        }
        THIP_TRY(hipMemcpyAsync(const_cast<float *>(to), src, run * sizeof(float), hipMemcpyHostToDevice, st));
        src += run;
        k = j;
    }
    return 0;
}

// thip_NAME_set_a of a dense family of one shape: the copies, one launch
int ob_set_a(const ObFamily &f, OwnBatch *h, int first, int count, const float *host_values, const int64_t *host_counts, int keep)
{
    THIP_NEED_INIT();
    const size_t per = h ? h->m * h->n : 0;
    size_t total = 0;
    THIP_RC(ob_seta_check(f, h, first, count, host_values, host_counts, [&](int) { return per; }, OB_SETA_DENSE, &total));
    int rc = 0;
    if (f.store) {                          // the sparse families' route: up to the handle's stage, a convert launch of its own
        void *pinned = nullptr;
        THIP_RC(ob_stage_reserve(h, total * sizeof(float), &pinned));
        memcpy(pinned, host_values, total * sizeof(float));
        THIP_TRY(hipMemcpyAsync(h->stage, pinned, total * sizeof(float), hipMemcpyHostToDevice, ctx().stream));
        rc = f.store->convert(h, first, count, static_cast<const float *>(h->stage));
    } else {
        rc = ob_seta_copy(h, first, count, host_values, [&](int) { return per; });
    }
    if (rc == 0) {
        ObArgs a = ob_args(h);
        a.first = first;
        rc = f.seta(h, a, ObSetA{ ObStart{ nullptr, nullptr, 0 }, keep != 0 }, (unsigned)count);
    }
    if (rc != 0) { hipStreamSynchronize(ctx().stream); return rc; }      // (a copy may still be reading the caller's values)
    return ob_restarted(h, first, count);
}

// thip_NAME_solutions: the gather kernel on the range into the staging buffer (`at`: the table of a handle of many shapes, which goes
// up in front of it; empty: one shape), one copy of that buffer and one of the range's status blocks down, and ob_finalize on each
// problem's part -- what thip_NAME_solution does to its three copies.  shape(p, &n, &m), block(p): problem p's shape and where its
// block of the arena begins, in floats.  Both of host_x and host_y NULL: the status blocks alone
template <class SHAPE, class BLOCK>
int ob_solutions_t(const ObFamily &f, OwnBatch *h, int first, int count, float *host_x, float *host_y, thip_status *host_status, bool table,
                   const SHAPE &shape, const BLOCK &block)
{
    THIP_NEED_INIT();
    if (!h) return fail(THIP_E_INVALID, f.text.null_h, __FILE__, __LINE__);
    if (!h->inited) return fail(THIP_E_INVALID, f.text.uninit, __FILE__, __LINE__);
    if (count < 1 || first < 0 || (size_t)first + (size_t)count > h->n_prob)
        return fail(THIP_E_INVALID, "no such range of problems", __FILE__, __LINE__);
    hipStream_t st = ctx().stream;
    const size_t cnt = (size_t)count, head = table ? cnt * 4 * sizeof(long long) : 0;
    const bool vectors = host_x || host_y;
    size_t floats = 0;
    if (vectors) {
        for (size_t k = 0; k < cnt; ++k) { size_t n, m; shape(first + (int)k, &n, &m); floats += n + m; }
        void *pinned = nullptr;
        THIP_RC(ob_stage_reserve(h, head + std::max<size_t>(floats, 1) * sizeof(float), &pinned));
        unsigned char *const dev = static_cast<unsigned char *>(h->stage);
        ObGather g{ h->arena, nullptr, h->stride, (int)h->n, (int)h->m, first, reinterpret_cast<float *>(dev + head) };
        if (table) {
            long long *at = static_cast<long long *>(pinned);
            size_t o = 0;
            for (size_t k = 0; k < cnt; ++k) {
                size_t n, m;
                shape(first + (int)k, &n, &m);
                at[4 * k] = block(first + (int)k); at[4 * k + 1] = (long long)n; at[4 * k + 2] = (long long)m; at[4 * k + 3] = (long long)o;
                o += n + m;
            }
            THIP_TRY(hipMemcpyAsync(dev, pinned, head, hipMemcpyHostToDevice, st));
            g.at = reinterpret_cast<const long long *>(dev);
        }
        hipLaunchKernelGGL(ownbatch_gather_k, dim3((unsigned)count), dim3(256), 0, st, g);
        THIP_LAUNCH_CHECK();
        THIP_TRY(hipMemcpyAsync(static_cast<unsigned char *>(pinned) + head, dev + head, floats * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    THIP_TRY(hipMemcpyAsync(h->hst + first, h->dst + first, cnt * sizeof(SbStatus), hipMemcpyDeviceToHost, st));
    THIP_TRY(hipStreamSynchronize(st));
    const float *got = vectors ? reinterpret_cast<const float *>(static_cast<unsigned char *>(h->stage_host) + head) : nullptr;
    for (size_t k = 0; k < cnt; ++k) {
        const SbStatus &s = h->hst[(size_t)first + k];
        if (vectors) {
            size_t n, m;
            shape(first + (int)k, &n, &m);
            if (host_x) { memcpy(host_x, got, n * sizeof(float)); ob_finalize(s, host_x, n); host_x += n; }
            if (host_y) { memcpy(host_y, got + n, m * sizeof(float)); ob_finalize(s, host_y, m); host_y += m; }
            got += n + m;
        }
        if (host_status) ob_status_out(s, host_status + k);
    }
    return 0;
}

int ob_solutions(const ObFamily &f, OwnBatch *h, int first, int count, float *host_x, float *host_y, thip_status *host_status)
{
    return ob_solutions_t(f, h, first, count, host_x, host_y, host_status, false,
                          [&](int, size_t *n, size_t *m) { *n = h->n; *m = h->m; }, [](int) { return 0ll; });
}

// ---- the round calls on device memory: the host side -----------------------------------------------------------------------------
// Each is its host twin with the packing done by a kernel: the tables go up (a few dozen bytes per problem), the check kernel's
// verdict comes down BEFORE anything is copied, scattered or set, the data moves device to device into the layout the host call
// uploads, and the family's set kernel runs as it does there.

// two ranges of bytes share one
bool ob_overlap(uintptr_t a, size_t na, uintptr_t b, size_t nb) { return na && nb && a < b + nb && b < a + na; }

// the lengths of one problem's part in each packed array of a range: 0 c / a solution's x (n), 1 b / row sums / a solution's y (m),
// 2 an iterate's x (n + 2 m + 1), 3 its y (n + m + 1), 4 a dense A (m n).  A range's array is its problems' parts one after another
constexpr int OB_DEV_KINDS = 5;
void ob_dev_lengths(size_t n, size_t m, long long *len)
{
    len[0] = (long long)n; len[1] = (long long)m; len[2] = (long long)(n + 2 * m + 1); len[3] = (long long)(n + m + 1);
    len[4] = (long long)(m * n);
}

// an array handed to a _dev call holds floats and lies outside everything the handle owns
int ob_dev_foreign(const OwnBatch *h, const void *p, size_t bytes, const char *what)
{
    char msg[160];
    if ((uintptr_t)p & 3u) {
        snprintf(msg, sizeof(msg), "%s: the arrays hold floats: 4-byte alignment", what);
        return fail(THIP_E_INVALID, msg, __FILE__, __LINE__);
    }
    for (const auto &o : h->owned)
        if (p && ob_overlap((uintptr_t)p, bytes, o.first, o.second)) {
            snprintf(msg, sizeof(msg), "%s overlaps memory the batch owns (its arena, its staging buffer, its store of b and c)", what);
            return fail(THIP_E_INVALID, msg, __FILE__, __LINE__);
        }
    return 0;
}

int ob_dev_range(const ObFamily &f, OwnBatch *h, int first, int count)
{
    if (!h) return fail(THIP_E_INVALID, f.text.null_h, __FILE__, __LINE__);
    if (!h->inited) return fail(THIP_E_INVALID, f.text.uninit, __FILE__, __LINE__);
    if (count < 1 || first < 0 || (size_t)first + (size_t)count > h->n_prob)
        return fail(THIP_E_INVALID, "no such range of problems", __FILE__, __LINE__);
    h->last_h2d = h->last_d2h = 0;
    return 0;
}

// `bytes` of pinned, device-mapped host memory for a _dev call's tables and verdict words
int ob_tab_reserve(OwnBatch *h, size_t bytes)
{
    if (h->tab_bytes >= bytes) return 0;
    THIP_TRY(hipStreamSynchronize(ctx().stream));
    if (h->tab_host) THIP_TRY(hipHostFree(h->tab_host));
    h->tab_host = h->tab_dev = nullptr; h->tab_bytes = 0;
    THIP_TRY(hipHostMalloc(&h->tab_host, bytes, hipHostMallocMapped));
    THIP_TRY(hipHostGetDevicePointer(&h->tab_dev, h->tab_host, 0));
    h->tab_bytes = bytes;
    return 0;
}

// the buffers of a _dev call, each part a multiple of 16 bytes.  [verdict | tables] in the handle's pinned, device-mapped memory
// (tab / tab_dev: as the host and as the kernels address it): one verdict word per problem, written by the check kernel and read by
// the host behind a synchronisation, and the rows the new kernels read -- a few dozen bytes per problem over the bus, no device
// memory.  [head | floats] in the staging buffers of the host calls (pin / dev): the layout the host twin uploads -- where each
// workgroup's part lies and the classes' lists; the parts -- which the family's kernels read as they do there
struct ObDevStage {
    size_t verdict = 0, tables = 0, head = 0, floats = 0;
    unsigned char *tab = nullptr, *tab_dev = nullptr, *pin = nullptr, *dev = nullptr;
    static size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }
    int reserve(OwnBatch *h)
    {
        verdict = up16(verdict); tables = up16(tables); head = up16(head); floats = up16(floats);
        THIP_RC(ob_tab_reserve(h, std::max<size_t>(verdict + tables, 16)));
        tab = static_cast<unsigned char *>(h->tab_host);
        tab_dev = static_cast<unsigned char *>(h->tab_dev);
        if (head + floats) {
            void *p = nullptr;
            THIP_RC(ob_stage_reserve(h, head + floats, &p));
            pin = static_cast<unsigned char *>(p);
            dev = static_cast<unsigned char *>(h->stage);
        }
        return 0;
    }
    unsigned char *rows() const { return tab + verdict; }                   // (the host's view of the tables)
    const unsigned char *rows_dev() const { return tab_dev + verdict; }     // (the kernels')
    size_t at_head() const { return 0; }
    size_t at_floats() const { return head; }
    // the head up; the tables are read where they lie
    int upload(OwnBatch *h) const
    {
        h->last_h2d += tables;
        if (head == 0) return 0;
        THIP_TRY(hipMemcpyAsync(dev, pin, head, hipMemcpyHostToDevice, ctx().stream));
        h->last_h2d += head;
        return 0;
    }
    // the check kernel on the `count` rows at the tables' beginning and its verdict (synchronises): *row < 0, or the first row at
    // fault and in *why its word
    int check(OwnBatch *h, int count, int mode, int *row, int *why) const
    {
        hipStream_t st = ctx().stream;
        hipLaunchKernelGGL(ownbatch_check_k, dim3((unsigned)count), dim3(256), 0, st, reinterpret_cast<const ObDevRow *>(rows_dev()), mode,
                           reinterpret_cast<int *>(tab_dev));
        THIP_LAUNCH_CHECK();
        THIP_TRY(hipStreamSynchronize(st));
        h->last_d2h += (size_t)count * sizeof(int);
        *row = -1; *why = 0;
        const volatile int *v = reinterpret_cast<const volatile int *>(tab);
        for (int k = 0; k < count && *row < 0; ++k)
            if (v[k] != 0) { *row = k; *why = v[k]; }
        return 0;
    }
};

// ownbatch_copy_a_k on the `count` rows at dev_rows, the longest of which holds `most` floats
int ob_dev_copy(const ObDevRow *dev_rows, size_t count, size_t most)
{
    const size_t chunks = (most + OB_COPY_CHUNK - 1) / OB_COPY_CHUNK;
    if (count == 0 || chunks == 0) return 0;
    if (chunks > 65535) return fail(THIP_E_INVALID, "a problem's part is too long for one copy launch", __FILE__, __LINE__);
    hipLaunchKernelGGL(ownbatch_copy_a_k, dim3((unsigned)count, (unsigned)chunks), dim3(256), 0, ctx().stream, dev_rows);
    THIP_LAUNCH_CHECK();
    return 0;
}

// what every set_*_dev ends with: the family's launches, then the host's books (synchronises)
template <class LAUNCH>
int ob_dev_finish(OwnBatch *h, int first, int count, const LAUNCH &launch)
{
    const int rc = launch();
    if (rc != 0) { hipStreamSynchronize(ctx().stream); return rc; }
    h->last_d2h += (size_t)count * sizeof(SbStatus);
    return ob_restarted(h, first, count);
}

// thip_NAME_set_a_dev of a dense family.  floats(p): problem p's m n.  dev_values == NULL: the caller has rewritten A where the slots
// read it, and the check kernel scans that.  launch(): the family's set_a kernel(s) on the range
template <class FLOATS, class LAUNCH>
int ob_set_a_dev_dense_t(const ObFamily &f, OwnBatch *h, int first, int count, const float *dev_values, const FLOATS &floats,
                         const LAUNCH &launch)
{
    THIP_NEED_INIT();
    THIP_RC(ob_dev_range(f, h, first, count));
    const size_t cnt = (size_t)count;
    size_t total = 0, most = 0;
    for (size_t k = 0; k < cnt; ++k) { const size_t w = floats(first + (int)k); total += w; most = std::max(most, w); }
    if (dev_values) {
        THIP_RC(ob_dev_foreign(h, dev_values, total * sizeof(float), "dev_values"));
        for (size_t k = 0; k < cnt; ++k)
            if (ob_overlap((uintptr_t)dev_values, total * sizeof(float), (uintptr_t)h->slot_a[(size_t)first + k],
                           floats(first + (int)k) * sizeof(float)))
                return fail(THIP_E_INVALID, "dev_values overlaps the A of a slot of the range (the in-place form: NULL)", __FILE__, __LINE__);
    }
    ObDevStage sg;
    sg.verdict = cnt * sizeof(int); sg.tables = cnt * sizeof(ObDevRow);
    THIP_RC(sg.reserve(h));
    ObDevRow *rows = reinterpret_cast<ObDevRow *>(sg.rows());
    const float *src = dev_values;
    for (size_t k = 0; k < cnt; ++k) {
        float *const to = const_cast<float *>(h->slot_a[(size_t)first + k]);
        const size_t w = floats(first + (int)k);
        rows[k] = ObDevRow{ dev_values ? src : to, to, (long long)w };
        src += w;
    }
    THIP_RC(sg.upload(h));
    int row, why;
    THIP_RC(sg.check(h, count, 0, &row, &why));
    if (row >= 0) {
        char msg[96];
        snprintf(msg, sizeof(msg), "problem %d: a value of A is not finite", first + row);
        return fail(THIP_E_INVALID, msg, __FILE__, __LINE__);
    }
    if (dev_values) THIP_RC(ob_dev_copy(reinterpret_cast<const ObDevRow *>(sg.rows_dev()), cnt, most));
    return ob_dev_finish(h, first, count, launch);
}

// thip_NAME_set_a_dev of a family that owns its matrix store: the values are converted from where they lie into the slots' blocks, one
// launch, behind the check kernel's verdict.  There is no in-place form: no f32 A lies behind the slots
template <class LAUNCH>
int ob_set_a_dev_store(const ObFamily &f, OwnBatch *h, int first, int count, const float *dev_values, const LAUNCH &launch)
{
    THIP_NEED_INIT();
    THIP_RC(ob_dev_range(f, h, first, count));
    if (!dev_values)
        return fail(THIP_E_INVALID, "null values of A: this batch holds a converted copy of every A and no f32 A lies in place to be read "
                                    "again (hand the values in)", __FILE__, __LINE__);
    const size_t cnt = (size_t)count, per = h->m * h->n;
    THIP_RC(ob_dev_foreign(h, dev_values, cnt * per * sizeof(float), "dev_values"));
    ObDevStage sg;
    sg.verdict = cnt * sizeof(int); sg.tables = cnt * sizeof(ObDevRow);
    THIP_RC(sg.reserve(h));
    ObDevRow *rows = reinterpret_cast<ObDevRow *>(sg.rows());
    for (size_t k = 0; k < cnt; ++k) rows[k] = ObDevRow{ dev_values + k * per, nullptr, (long long)per };
    THIP_RC(sg.upload(h));
    int row, why;
    THIP_RC(sg.check(h, count, 0, &row, &why));
    if (row >= 0) {
        char msg[96];
        snprintf(msg, sizeof(msg), "problem %d: a value of A is not finite", first + row);
        return fail(THIP_E_INVALID, msg, __FILE__, __LINE__);
    }
    THIP_RC(f.store->convert(h, first, count, dev_values));
    return ob_dev_finish(h, first, count, launch);
}

int ob_set_a_dev(const ObFamily &f, OwnBatch *h, int first, int count, const float *dev_values, int keep)
{
    if (f.store)
        return ob_set_a_dev_store(f, h, first, count, dev_values, [&]() {
            ObArgs a = ob_args(h);
            a.first = first;
            return f.seta(h, a, ObSetA{ ObStart{ nullptr, nullptr, 0 }, keep != 0 }, (unsigned)count);
        });
    const size_t per = h ? h->m * h->n : 0;
    return ob_set_a_dev_dense_t(f, h, first, count, dev_values, [&](int) { return per; }, [&]() {
        ObArgs a = ob_args(h);
        a.first = first;
        return f.seta(h, a, ObSetA{ ObStart{ nullptr, nullptr, 0 }, keep != 0 }, (unsigned)count);
    });
}

// thip_NAME_set_a_dev of a sparse family: the values stay where the caller holds them, need(p) per problem one after another, and
// the scatter kernel reads them there.  head: the bytes of the host twin's head; fill(pin_head, at_p): writes it, at_p[k] being where
// problem first + k's values begin (in floats); launch(dev_head): the scatter and the set_a kernel(s) with ObStart{ dev_values, .. }
template <class NEED, class FILL, class LAUNCH>
int ob_set_a_dev_sparse_t(const ObFamily &f, OwnBatch *h, int first, int count, const float *dev_values, const NEED &need, size_t head,
                          const FILL &fill, const LAUNCH &launch)
{
    THIP_NEED_INIT();
    THIP_RC(ob_dev_range(f, h, first, count));
    if (!dev_values)
        return fail(THIP_E_INVALID, "null values of A: a sparse batch is handed its values (the in-place form is a dense batch's)", __FILE__,
                    __LINE__);
    const size_t cnt = (size_t)count;
    std::vector<long long> at_p(cnt);
    size_t total = 0;
    for (size_t k = 0; k < cnt; ++k) { at_p[k] = (long long)total; total += need(first + (int)k); }
    THIP_RC(ob_dev_foreign(h, dev_values, total * sizeof(float), "dev_values"));
    ObDevStage sg;
    sg.verdict = cnt * sizeof(int); sg.tables = cnt * sizeof(ObDevRow); sg.head = head;
    THIP_RC(sg.reserve(h));
    ObDevRow *rows = reinterpret_cast<ObDevRow *>(sg.rows());
    for (size_t k = 0; k < cnt; ++k) rows[k] = ObDevRow{ dev_values + at_p[k], nullptr, (long long)need(first + (int)k) };
    fill(sg.pin + sg.at_head(), at_p);
    THIP_RC(sg.upload(h));
    int row, why;
    THIP_RC(sg.check(h, count, 0, &row, &why));
    if (row >= 0) {
        char msg[96];
        snprintf(msg, sizeof(msg), "problem %d: a value of A is not finite", first + row);
        return fail(THIP_E_INVALID, msg, __FILE__, __LINE__);
    }
    const unsigned char *const dev_head = sg.dev + sg.at_head();
    return ob_dev_finish(h, first, count, [&]() { return launch(dev_head); });
}

// thip_NAME_set_iterates_dev.  shape(p, &n, &m); head, fill as above with at_p[k] where problem first + k's staged iterate begins;
// launch(dev_head, dev_floats): the start kernel(s).  The iterates are copied into the staged layout (x then y per problem) by
// ownbatch_copy_a_k, two rows per problem, and the start kernels read them as they read an upload
template <class SHAPE, class FILL, class LAUNCH>
int ob_set_iterates_dev_t(const ObFamily &f, OwnBatch *h, int first, int count, const float *dev_x, const float *dev_y, const SHAPE &shape,
                          size_t head, const FILL &fill, const LAUNCH &launch)
{
    THIP_NEED_INIT();
    THIP_RC(ob_dev_range(f, h, first, count));
    if (!dev_x || !dev_y) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    const size_t cnt = (size_t)count;
    std::vector<long long> at_p(cnt);
    size_t floats = 0, sum_x = 0, sum_y = 0, most = 0;
    for (size_t k = 0; k < cnt; ++k) {
        size_t n, m;
        shape(first + (int)k, &n, &m);
        long long len[OB_DEV_KINDS];
        ob_dev_lengths(n, m, len);
        at_p[k] = (long long)floats;
        floats += (size_t)(len[2] + len[3]); sum_x += (size_t)len[2]; sum_y += (size_t)len[3];
        most = std::max(most, (size_t)len[2]);
    }
    THIP_RC(ob_dev_foreign(h, dev_x, sum_x * sizeof(float), "dev_x"));
    THIP_RC(ob_dev_foreign(h, dev_y, sum_y * sizeof(float), "dev_y"));
    ObDevStage sg;
    sg.verdict = cnt * sizeof(int); sg.tables = 3 * cnt * sizeof(ObDevRow); sg.head = head; sg.floats = floats * sizeof(float);
    THIP_RC(sg.reserve(h));
    ObDevRow *rows = reinterpret_cast<ObDevRow *>(sg.rows());
    float *const to = reinterpret_cast<float *>(sg.dev + sg.at_floats());
    {
        const float *x = dev_x, *y = dev_y;
        for (size_t k = 0; k < cnt; ++k) {
            size_t n, m;
            shape(first + (int)k, &n, &m);
            long long len[OB_DEV_KINDS];
            ob_dev_lengths(n, m, len);
            const size_t nx = (size_t)len[2], ny = (size_t)len[3];
            rows[k] = ObDevRow{ x + nx - 1, const_cast<float *>(y + ny - 1), 1 };          // (the check's: tau, kappa)
            rows[cnt + 2 * k] = ObDevRow{ x, to + at_p[k], (long long)nx };
            rows[cnt + 2 * k + 1] = ObDevRow{ y, to + at_p[k] + nx, (long long)ny };
            x += nx; y += ny;
        }
    }
    fill(sg.pin + sg.at_head(), at_p);
    THIP_RC(sg.upload(h));
    int row, why;
    THIP_RC(sg.check(h, count, 1, &row, &why));
    if (row >= 0) {
        char msg[128];
        snprintf(msg, sizeof(msg), "problem %d: %s", first + row, why == 1 ? "a start's tau is finite and not negative"
                                                                             : "a start's kappa is finite and not positive");
        return fail(THIP_E_INVALID, msg, __FILE__, __LINE__);
    }
    THIP_RC(ob_dev_copy(reinterpret_cast<const ObDevRow *>(sg.rows_dev()) + cnt, 2 * cnt, most));
    const unsigned char *const dev_head = sg.dev + sg.at_head();
    return ob_dev_finish(h, first, count, [&]() { return launch(dev_head, to); });
}

int ob_set_iterates_dev(const ObFamily &f, OwnBatch *h, int first, int count, const float *dev_x, const float *dev_y)
{
    const long long per = h ? (long long)(2 * h->n + 3 * h->m + 2) : 0;
    return ob_set_iterates_dev_t(f, h, first, count, dev_x, dev_y, [&](int, size_t *n, size_t *m) { *n = h->n; *m = h->m; }, 0,
                                 [](unsigned char *, const std::vector<long long> &) {},
                                 [&](const unsigned char *, const float *staged) {
                                     ObArgs a = ob_args(h);
                                     a.first = first;
                                     return f.start(h, a, ObStart{ staged, nullptr, per }, (unsigned)count);
                                 });
}

// thip_NAME_set_bc_dev.  store(): the handle's b / c store is there (the host twin's rule).  ownbatch_stage_bc_k builds each problem's
// staged part -- the word, b, c, the row sums -- from the three device arrays; the set_bc kernels run unchanged on it
template <class SHAPE, class STORE, class FILL, class LAUNCH>
int ob_set_bc_dev_t(const ObFamily &f, OwnBatch *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_r,
                    const uint8_t *host_has, const SHAPE &shape, const STORE &store, size_t head, const FILL &fill, const LAUNCH &launch)
{
    THIP_NEED_INIT();
    THIP_RC(ob_dev_range(f, h, first, count));
    if (!dev_b || !dev_c) return fail(THIP_E_INVALID, "null b or c", __FILE__, __LINE__);
    const size_t cnt = (size_t)count;
    std::vector<long long> at_p(cnt);
    size_t floats = 0, sum_n = 0, sum_m = 0;
    for (size_t k = 0; k < cnt; ++k) {
        size_t n, m;
        shape(first + (int)k, &n, &m);
        long long len[OB_DEV_KINDS];
        ob_dev_lengths(n, m, len);
        at_p[k] = (long long)floats;
        floats += (size_t)(1 + 2 * len[1] + len[0]); sum_n += (size_t)len[0]; sum_m += (size_t)len[1];
    }
    THIP_RC(ob_dev_foreign(h, dev_b, sum_m * sizeof(float), "dev_b"));
    THIP_RC(ob_dev_foreign(h, dev_c, sum_n * sizeof(float), "dev_c"));
    THIP_RC(ob_dev_foreign(h, dev_r, sum_m * sizeof(float), "dev_b_rowabs"));
    THIP_RC(store());
    ObDevStage sg;
    sg.tables = cnt * sizeof(ObBcRow); sg.head = head; sg.floats = floats * sizeof(float);
    THIP_RC(sg.reserve(h));
    ObBcRow *rows = reinterpret_cast<ObBcRow *>(sg.rows());
    float *const to = reinterpret_cast<float *>(sg.dev + sg.at_floats());
    {
        const float *b = dev_b, *c = dev_c, *r = dev_r;
        for (size_t k = 0; k < cnt; ++k) {
            size_t n, m;
            shape(first + (int)k, &n, &m);
            const bool has = dev_r && (!host_has || host_has[k]);
            rows[k] = ObBcRow{ b, c, has ? r : nullptr, to + at_p[k], (int)n, (int)m };
            b += m; c += n;
            if (r) r += m;
        }
    }
    fill(sg.pin + sg.at_head(), at_p);
    THIP_RC(sg.upload(h));
    hipLaunchKernelGGL(ownbatch_stage_bc_k, dim3((unsigned)count), dim3(256), 0, ctx().stream,
                       reinterpret_cast<const ObBcRow *>(sg.rows_dev()));
    THIP_LAUNCH_CHECK();
    const unsigned char *const dev_head = sg.dev + sg.at_head();
    return ob_dev_finish(h, first, count, [&]() { return launch(dev_head, to); });
}

int ob_set_bc_dev(const ObFamily &f, OwnBatch *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_r,
                  const uint8_t *host_has, int keep)
{
    return ob_set_bc_dev_t(f, h, first, count, dev_b, dev_c, dev_r, host_has, [&](int, size_t *n, size_t *m) { *n = h->n; *m = h->m; },
                           [&]() { return ob_setbc_store(h, (2 * h->m + h->n) * h->n_prob, nullptr); }, 0,
                           [](unsigned char *, const std::vector<long long> &) {},
                           [&](const unsigned char *, const float *staged) {
                               ObArgs a = ob_args(h);
                               a.first = first;
                               const ObSetBc s{ ObStart{ staged, nullptr, (long long)(1 + 2 * h->m + h->n) }, h->bc_store, nullptr,
                                                (long long)(2 * h->m + h->n), keep != 0 };
                               return f.setbc(h, a, s, (unsigned)count);
                           });
}

// thip_NAME_solutions_dev: one launch, nothing comes down and nothing is waited for.  table: a handle of many shapes, whose table
// of every problem goes up once, with the first call (block(p): where problem p's block of the arena begins, in floats)
template <class SHAPE, class BLOCK>
int ob_solutions_dev_t(const ObFamily &f, OwnBatch *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state, bool table,
                       const SHAPE &shape, const BLOCK &block)
{
    THIP_NEED_INIT();
    THIP_RC(ob_dev_range(f, h, first, count));
    size_t x0 = 0, y0 = 0, sum_n = 0, sum_m = 0;
    for (size_t p = 0; p < (size_t)first + (size_t)count; ++p) {
        size_t n, m;
        shape((int)p, &n, &m);
        if (p < (size_t)first) { x0 += n; y0 += m; } else { sum_n += n; sum_m += m; }
    }
    THIP_RC(ob_dev_foreign(h, dev_x, sum_n * sizeof(float), "dev_x"));
    THIP_RC(ob_dev_foreign(h, dev_y, sum_m * sizeof(float), "dev_y"));
    THIP_RC(ob_dev_foreign(h, dev_state, (size_t)count * sizeof(int32_t), "dev_state"));
    if (!dev_x && !dev_y && !dev_state) return 0;
    if (table && !h->sol_at_dev) {
        std::vector<long long> at(5 * h->n_prob);
        size_t ox = 0, oy = 0;
        for (size_t p = 0; p < h->n_prob; ++p) {
            size_t n, m;
            shape((int)p, &n, &m);
            at[5 * p] = block((int)p); at[5 * p + 1] = (long long)n; at[5 * p + 2] = (long long)m;
            at[5 * p + 3] = (long long)ox; at[5 * p + 4] = (long long)oy;
            ox += n; oy += m;
        }
        long long *dev = nullptr;
        THIP_RC(ob_alloc(h, (void **)&dev, at.size() * sizeof(long long)));
        h->sol_at_dev = dev;
        THIP_TRY(hipMemcpy(dev, at.data(), at.size() * sizeof(long long), hipMemcpyHostToDevice));
        h->last_h2d += at.size() * sizeof(long long);
    }
    const ObGatherDev g{ h->arena, h->dst, table ? h->sol_at_dev : nullptr, h->stride, (int)h->n, (int)h->m, first, (long long)x0,
                         (long long)y0, dev_x, dev_y, dev_state };
    hipLaunchKernelGGL(ownbatch_gather_final_k, dim3((unsigned)count), dim3(256), 0, ctx().stream, g);
    THIP_LAUNCH_CHECK();
    return 0;
}

int ob_solutions_dev(const ObFamily &f, OwnBatch *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state)
{
    return ob_solutions_dev_t(f, h, first, count, dev_x, dev_y, dev_state, false, [&](int, size_t *n, size_t *m) { *n = h->n; *m = h->m; },
                              [](int) { return 0ll; });
}

// the shape rules alone: the family's check (which fills *cones, *cls and *psd when they are given), its thread choice and the LDS of
// one workgroup
int ob_fits(const ObFamily &f, size_t n, size_t m, size_t n_seg, const int32_t *seg_type, const int64_t *seg_len, size_t *host_lds_bytes,
            int *host_threads, std::vector<int> *cones = nullptr, std::vector<unsigned char> *cls = nullptr, ObPsd *psd_out = nullptr)
{
    ObPsd psd;
    THIP_RC(f.check(n, m, n_seg, seg_type, seg_len, cones, cls, &psd));
    const int t = f.threads_for(n, m);
    if (host_threads) *host_threads = t;
    if (host_lds_bytes) *host_lds_bytes = f.lds_for(n, m, t, psd);
    // (the bound is on the widest workgroup a test may force: no accepted shape can fail to launch)
    if (f.lds_for(n, m, *std::max_element(f.forced, f.forced + 3), psd) > OB_LDS_MAX)
        return fail(THIP_E_INVALID, "the problem does not fit the LDS of one CU", __FILE__, __LINE__);
    if (psd_out) *psd_out = psd;
    return 0;
}

// H: the family's handle type.  Every refusal comes before the first allocation; a later failure destroys what was built
template <class H>
int ob_create(ObFamily &f, size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b, const float *dev_vecs_c,
              const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
              const thip_param *par, H **out, int store_arg = 0)
{
    if (!out) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *out = nullptr;
    THIP_NEED_INIT();
    const ObText &tx = f.text;
    if (!par || !dev_mats_a || !dev_vecs_b || !dev_vecs_c) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (n_prob < 1 || n_prob > OB_MAX_PROB) return fail(THIP_E_INVALID, tx.count, __FILE__, __LINE__);
    if (par->state_arith != THIP_STATE_COMPENSATED && par->state_arith != THIP_STATE_PLAIN)
        return fail(THIP_E_INVALID, "bad thip_param.state_arith", __FILE__, __LINE__);
    if (((uintptr_t)dev_mats_a | (uintptr_t)dev_vecs_b | (uintptr_t)dev_vecs_c | (uintptr_t)dev_vecs_b_rowabs) & 3u)
        return fail(THIP_E_INVALID, "the arrays hold floats: 4-byte alignment", __FILE__, __LINE__);
    H *h = new H();
    h->fam = &f;
    int rc = ob_fits(f, n, m, n_seg, host_seg_type, host_seg_len, nullptr, nullptr, &h->cones, &h->cls, &h->psd);
    if (rc != 0) { delete h; return rc; }
    h->n = n; h->m = m; h->n_prob = n_prob;
    h->par = *par;
    h->stride = f.stride_for(n, m);
    ob_plan(h);
    if (f.streams) {
        h->unaligned.assign(n_prob, 0);
        for (size_t p = 0; p < n_prob; ++p) {
            h->unaligned[p] = (((uintptr_t)(dev_mats_a + p * m * n)) & 15u) != 0;
            h->n_unaligned += h->unaligned[p];
        }
    }
    rc = ob_attr(f);
    if (rc == 0) rc = ob_build(h, dev_mats_a, dev_vecs_b, dev_vecs_c, dev_vecs_b_rowabs);
    if (rc == 0 && f.store) rc = f.store->create(h, dev_mats_a, store_arg);
    if (rc != 0) { ob_destroy(h); return rc; }
    *out = h;
    return 0;
}

// the fields every family's info record begins with
struct ObInfo {
    template <class INFO>
    void operator()(const OwnBatch *h, INFO &o) const
    {
        o.n_prob = (int32_t)h->n_prob; o.threads = h->threads; o.lds_bytes = (int32_t)h->lds; o.live = (int32_t)h->live.size();
        o.arena_bytes = h->stride * h->n_prob * sizeof(float);
        o.device_bytes = h->bytes;
        o.device_bytes_all = h->fam->total;
        o.launches = h->launches; o.workgroups = h->workgroups;
    }
};

// FILL: ObInfo, or the family's functor that adds to it
template <class INFO, class FILL>
int ob_info_out(const OwnBatch *h, INFO *host_info, FILL fill)
{
    if (!h || !host_info) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    memset(host_info, 0, sizeof(*host_info));
    fill(h, *host_info);
    return 0;
}

int ob_force_threads(const ObFamily &f, OwnBatch *h, int threads)
{
    if (!h) return fail(THIP_E_INVALID, f.text.null_h, __FILE__, __LINE__);
    if (threads != 0 && std::find(f.forced, f.forced + 3, threads) == f.forced + 3)
        return fail(THIP_E_INVALID, f.text.force_sizes, __FILE__, __LINE__);
    if (h->inited) return fail(THIP_E_INVALID, f.text.force_late, __FILE__, __LINE__);
    h->forced = threads;
    ob_plan(h);
    return 0;
}

}  // namespace

// the C API of a family (the declarations of include/totsu_f32hip.h and include/totsu_f32hip_test.h): NAME as in thip_NAME_create,
// FAM its ObFamily, FILL what fills its info record.  struct thip_NAME, the handle, is the family's to define (an OwnBatch)
#define OB_DEFINE_API(NAME, FAM, FILL)                                                                                              \
    extern "C" {                                                                                                                    \
    int thip_##NAME##_fits(size_t n, size_t m, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,             \
                           size_t *host_lds_bytes, int *host_threads)                                                               \
    { return ob_fits(FAM, n, m, n_seg, host_seg_type, host_seg_len, host_lds_bytes, host_threads); }                                \
    int thip_##NAME##_destroy(thip_##NAME *h) { return ob_destroy(h); }                                                             \
    int thip_##NAME##_create(size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b,                   \
                             const float *dev_vecs_c, const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type,   \
                             const int64_t *host_seg_len, const thip_param *par, thip_##NAME **out)                                 \
    { return ob_create(FAM, n, m, n_prob, dev_mats_a, dev_vecs_b, dev_vecs_c, dev_vecs_b_rowabs, n_seg, host_seg_type,              \
                       host_seg_len, par, out); }                                                                                   \
    int thip_##NAME##_set_param(thip_##NAME *h, const thip_param *par) { return ob_set_param(h, par); }                             \
    int thip_##NAME##_init(thip_##NAME *h) { return ob_init(FAM, h); }                                                              \
    int thip_##NAME##_run(thip_##NAME *h, int64_t max_steps, int64_t poll_every, thip_status *host_status)                          \
    { return ob_run(FAM, h, max_steps, poll_every, host_status, false); }                                                           \
    int thip_##NAME##_run_until_any(thip_##NAME *h, int64_t max_steps, int64_t poll_every, thip_status *host_status)                \
    { return ob_run(FAM, h, max_steps, poll_every, host_status, true); }                                                            \
    int thip_##NAME##_status(thip_##NAME *h, int i, thip_status *host_status) { return ob_status(FAM, h, i, host_status); }         \
    int thip_##NAME##_solution(thip_##NAME *h, int i, float *host_x, float *host_y) { return ob_solution(FAM, h, i, host_x, host_y); } \
    int thip_##NAME##_iterate(thip_##NAME *h, int i, float *host_x, float *host_y) { return ob_iterate(FAM, h, i, host_x, host_y); } \
    int thip_##NAME##_precond(thip_##NAME *h, int i, float *host_dp_tau, float *host_dp_sigma)                                      \
    { return ob_precond(FAM, h, i, host_dp_tau, host_dp_sigma); }                                                                   \
    int thip_##NAME##_replace(thip_##NAME *h, int i, const float *dev_mat_a, const float *dev_vec_b, const float *dev_vec_c,        \
                              const float *dev_vec_b_rowabs)                                                                        \
    { return ob_replace(FAM, h, i, dev_mat_a, dev_vec_b, dev_vec_c, dev_vec_b_rowabs); }                                            \
    int thip_##NAME##_set_iterates(thip_##NAME *h, int first, int count, const float *host_x, const float *host_y)                  \
    { return ob_set_iterates(FAM, h, first, count, host_x, host_y); }                                                               \
    int thip_##NAME##_set_bc(thip_##NAME *h, int first, int count, const float *host_b, const float *host_c,                        \
                             const float *host_b_rowabs, const uint8_t *host_has_rowabs, int keep_iterate)                          \
    { return ob_set_bc(FAM, h, first, count, host_b, host_c, host_b_rowabs, host_has_rowabs, keep_iterate); }                       \
    int thip_##NAME##_solutions(thip_##NAME *h, int first, int count, float *host_x, float *host_y, thip_status *host_status)       \
    { return ob_solutions(FAM, h, first, count, host_x, host_y, host_status); }                                                     \
    int thip_##NAME##_set_a(thip_##NAME *h, int first, int count, const float *host_values, const int64_t *host_counts,             \
                            int keep_iterate)                                                                                       \
    { return ob_set_a(FAM, h, first, count, host_values, host_counts, keep_iterate); }                                              \
    int thip_##NAME##_set_bc_dev(thip_##NAME *h, int first, int count, const float *dev_b, const float *dev_c,                      \
                                 const float *dev_b_rowabs, const uint8_t *host_has_rowabs, int keep_iterate)                       \
    { return ob_set_bc_dev(FAM, h, first, count, dev_b, dev_c, dev_b_rowabs, host_has_rowabs, keep_iterate); }                      \
    int thip_##NAME##_set_a_dev(thip_##NAME *h, int first, int count, const float *dev_values, int keep_iterate)                    \
    { return ob_set_a_dev(FAM, h, first, count, dev_values, keep_iterate); }                                                        \
    int thip_##NAME##_set_iterates_dev(thip_##NAME *h, int first, int count, const float *dev_x, const float *dev_y)                \
    { return ob_set_iterates_dev(FAM, h, first, count, dev_x, dev_y); }                                                             \
    int thip_##NAME##_solutions_dev(thip_##NAME *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state)           \
    { return ob_solutions_dev(FAM, h, first, count, dev_x, dev_y, dev_state); }                                                     \
    int thip_##NAME##_info(const thip_##NAME *h, thip_##NAME##_info_t *host_info) { return ob_info_out(h, host_info, FILL()); }       \
    int thip_test_##NAME##_force_threads(thip_##NAME *h, int threads) { return ob_force_threads(FAM, h, threads); }                 \
    }

// the test hooks every family shares (include/totsu_f32hip_test.h), defined by the one translation unit that asks for them.  h: a
// handle of any own-A family -- each is an OwnBatch first, and every translation unit compiles this header's one definition of it
#ifdef OB_DEFINE_HOOKS
extern "C" {
int thip_test_ownbatch_addresses(void *h, uint64_t *host_addr, uint64_t *host_bytes)
{
    const OwnBatch *b = static_cast<const OwnBatch *>(h);
    if (!b || !host_addr || !host_bytes) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    const void *const what[3] = { b->arena, b->stage, b->bc_store };
    for (int k = 0; k < 3; ++k) {
        host_addr[k] = (uint64_t)(uintptr_t)what[k];
        host_bytes[k] = 0;
        for (const auto &o : b->owned)
            if (what[k] && o.first == (uintptr_t)what[k]) host_bytes[k] = o.second;
    }
    return 0;
}
int thip_test_ownbatch_last_transfer(void *h, uint64_t *host_h2d_bytes, uint64_t *host_d2h_bytes)
{
    const OwnBatch *b = static_cast<const OwnBatch *>(h);
    if (!b || !host_h2d_bytes || !host_d2h_bytes) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *host_h2d_bytes = b->last_h2d; *host_d2h_bytes = b->last_d2h;
    return 0;
}
int thip_test_ownbatch_overlap(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes)
{
    return ob_overlap((uintptr_t)a, (size_t)a_bytes, (uintptr_t)b, (size_t)b_bytes) ? 1 : 0;
}
int thip_test_ownbatch_offsets(size_t count, const size_t *host_n, const size_t *host_m, int64_t *host_at)
{
    if (!host_n || !host_m || !host_at) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    long long sum[OB_DEV_KINDS] = { 0, 0, 0, 0, 0 }, len[OB_DEV_KINDS];
    for (size_t k = 0; k <= count; ++k) {
        for (int q = 0; q < OB_DEV_KINDS; ++q) host_at[(size_t)q * (count + 1) + k] = sum[q];
        if (k == count) break;
        ob_dev_lengths(host_n[k], host_m[k], len);
        for (int q = 0; q < OB_DEV_KINDS; ++q) sum[q] += len[q];
    }
    return 0;
}
int thip_test_ownbatch_copy_chunk(void) { return OB_COPY_CHUNK; }
}
#endif
