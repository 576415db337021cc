// thip_ownbatch.h -- what the "every problem has its OWN A" batches share (thip_smallbatch.hip: A in LDS; thip_midbatch.hip and
// thip_sdpbatch.hip: A streamed from memory, thip_midstream.h): the status block and the slot of a problem, the device functions of
// the iteration that do not touch A (block_sums, sb_comp_add, sb_soc), and the host machinery -- slots, arena, all 64-byte status
// blocks in one copy, the live list, replace as the init kernel on one slot.  A family supplies its two launches, its shape rule
// and its words for the refusals.
// Included once by each of the translation units: everything here is internal to the one that includes it.
#pragma once

#include "thip_common.h"

#include <algorithm>
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

// comp_add of thip_solver_kernels.inc
__device__ __forceinline__ float sb_comp_add(float x, float inc, float *k, int i, bool comp)
{
    if (!comp) return x + inc;
    const float y = inc - k[i];
    const float t = x + y;
    k[i] = (t - x) - y;
    return t;
}

// soc_k of thip_cone.hip for one cone by one wave, with rx <- rx - 2 x folded in (cone_soc.rs:38-65, cone_rotsoc.rs:38-65)
__device__ __forceinline__ void sb_soc(float *x, float *rx, int beg, int end, int rotated, int lane)
{
    const int len = end - beg;
    if (len <= 0) return;
    const float fsqrt2 = sqrtf(2.0f);
    if (rotated && len == 1) {
        if (lane == 0) {
            const float v = fmaxf(x[beg], 0.0f);
            x[beg] = v;
            rx[beg] = rx[beg] - 2.0f * v;
        }
        return;
    }
    float s0, v1 = 0.0f;
    if (rotated) {
        const float r = x[beg], s = x[beg + 1];
        s0 = (r + s) / fsqrt2;
        v1 = (r - s) / fsqrt2;
    } else {
        s0 = x[beg];
    }
    double acc = 0.0;
    for (int i = beg + 1 + lane; i < end; i += 64) {
        const double t = (double)((rotated && i == beg + 1) ? v1 : x[i]);
        acc += t * t;
    }
    const float norm_v = (float)sqrt(wave_sum_d(acc));
    float f, s_new;
    if (norm_v <= -s0) { f = 0.0f; s_new = 0.0f; }
    else if (norm_v <= s0) { f = 1.0f; s_new = s0; }
    else { f = (1.0f + s0 / norm_v) / 2.0f; s_new = (norm_v + s0) / 2.0f; }
    if (!rotated) {
        if (lane == 0) {
            x[beg] = s_new;
            rx[beg] = rx[beg] - 2.0f * s_new;
        }
        for (int i = beg + 1 + lane; i < end; i += 64) {
            const float nv = (f == 1.0f) ? x[i] : f * x[i];
            x[i] = nv;
            rx[i] = rx[i] - 2.0f * nv;
        }
    } else {
        const float v1n = f * v1;
        for (int i = beg + 2 + lane; i < end; i += 64) {
            const float nv = (f == 1.0f) ? x[i] : f * x[i];
            x[i] = nv;
            rx[i] = rx[i] - 2.0f * nv;
        }
        if (lane == 0) {
            const float a = (s_new + v1n) / fsqrt2, b = (s_new - v1n) / fsqrt2;
            x[beg] = a;
            x[beg + 1] = b;
            rx[beg] = rx[beg] - 2.0f * a;
            rx[beg + 1] = rx[beg + 1] - 2.0f * b;
        }
    }
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
struct ObText { const char *uninit, *null_h, *count, *no_psd; };

// what a handle of either family is.  The arena holds, per problem, `stride` floats: xx u kx ku | xy xs v ky ks kv | Tx Ty Ts Sv and
// then whatever else the family carries
struct OwnBatch {
    const ObText *text = nullptr;
    size_t *total = nullptr;                // device memory held by every handle of the family
    int (*launch_init)(OwnBatch *, int first, int count) = nullptr;
    int (*launch_run)(OwnBatch *, int count, int steps, const int *live) = nullptr;
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
    h->bytes += bytes; *h->total += bytes;
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

int ob_run(OwnBatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status, bool until_any)
{
    THIP_NEED_INIT();
    if (!h || !h->inited) return fail(THIP_E_INVALID, h ? h->text->uninit : "null batch", __FILE__, __LINE__);
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
        THIP_RC(h->launch_run(h, (int)h->live.size(), (int)batch, all ? nullptr : h->live_dev));
        h->launches += 1;
        h->workgroups += (int64_t)h->live.size();
        done += batch;
        THIP_RC(ob_poll(h, host_status));       // (synchronises: the list the launch read is the host's to rewrite)
    }
    return 0;
}

int ob_member(OwnBatch *h, int i)
{
    if (!h || !h->inited) return fail(THIP_E_INVALID, h ? h->text->uninit : "null batch", __FILE__, __LINE__);
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

int ob_destroy(OwnBatch *h)
{
    if (ctx().inited) hipStreamSynchronize(ctx().stream);
    hipFree(h->arena); hipFree(h->dst); hipFree(h->slots); hipFree(h->live_dev); hipFree(h->cones_dev); hipFree(h->cls_dev);
    if (h->hst) hipHostFree(h->hst);
    *h->total -= h->bytes;
    return 0;
}

// the refusals of create that do not depend on the shape
int ob_create_args(const ObText &tx, size_t n_prob, const float *a, const float *b, const float *c, const float *rowabs,
                   const thip_param *par)
{
    if (!par || !a || !b || !c) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (n_prob < 1 || n_prob > OB_MAX_PROB) return fail(THIP_E_INVALID, tx.count, __FILE__, __LINE__);
    if (par->state_arith != THIP_STATE_COMPENSATED && par->state_arith != THIP_STATE_PLAIN)
        return fail(THIP_E_INVALID, "bad thip_param.state_arith", __FILE__, __LINE__);
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)rowabs) & 3u)
        return fail(THIP_E_INVALID, "the arrays hold floats: 4-byte alignment", __FILE__, __LINE__);
    return 0;
}

// everything a handle holds on the device (n, m, n_prob, stride, cones and cls are set)
int ob_build(OwnBatch *h, const float *a, const float *b, const float *c, const float *rowabs)
{
    hipStream_t st = ctx().stream;
    const size_t n_prob = h->n_prob, m = h->m;
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

int ob_init(OwnBatch *h, const ObText &tx)
{
    THIP_NEED_INIT();
    if (!h) return fail(THIP_E_INVALID, tx.null_h, __FILE__, __LINE__);
    THIP_RC(h->launch_init(h, 0, (int)h->n_prob));
    h->launches = 0; h->workgroups = 0;
    h->inited = true;
    return ob_poll(h, nullptr);
}

int ob_status(OwnBatch *h, int i, thip_status *host_status)
{
    THIP_NEED_INIT();
    THIP_RC(ob_member(h, i));
    if (!host_status) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    THIP_RC(ob_status_one(h, i));
    ob_status_out(h->hst[i], host_status);
    return 0;
}

int ob_solution(OwnBatch *h, int i, float *host_x, float *host_y)
{
    THIP_NEED_INIT();
    THIP_RC(ob_member(h, i));
    THIP_RC(ob_status_one(h, i));
    const float *ar = h->arena + (size_t)i * h->stride;
    if (host_x) THIP_RC(thip_d2h(host_x, ar, h->n));
    if (host_y) THIP_RC(thip_d2h(host_y, ar + 4 * h->n, h->m));
    ob_finalize(h->hst[i], host_x, h->n);
    ob_finalize(h->hst[i], host_y, h->m);
    return 0;
}

int ob_iterate(OwnBatch *h, int i, float *host_x, float *host_y)
{
    THIP_NEED_INIT();
    THIP_RC(ob_member(h, i));
    THIP_RC(ob_status_one(h, i));
    const size_t n = h->n, m = h->m;
    const float *ar = h->arena + (size_t)i * h->stride;      // xx u kx ku | xy xs v ..
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

int ob_precond(OwnBatch *h, int i, float *host_dp_tau, float *host_dp_sigma)
{
    THIP_NEED_INIT();
    THIP_RC(ob_member(h, i));
    THIP_RC(ob_status_one(h, i));
    const size_t n = h->n, m = h->m;
    const float *k = h->arena + (size_t)i * h->stride + 4 * n + 6 * m;      // Tx Ty Ts Sv
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

int ob_replace(OwnBatch *h, int i, const float *dev_mat_a, const float *dev_vec_b, const float *dev_vec_c, const float *dev_vec_b_rowabs)
{
    THIP_NEED_INIT();
    THIP_RC(ob_member(h, i));
    if (!dev_mat_a || !dev_vec_b || !dev_vec_c) return fail(THIP_E_INVALID, "null A, b or c", __FILE__, __LINE__);
    if (((uintptr_t)dev_mat_a | (uintptr_t)dev_vec_b | (uintptr_t)dev_vec_c | (uintptr_t)dev_vec_b_rowabs) & 3u)
        return fail(THIP_E_INVALID, "the arrays hold floats: 4-byte alignment", __FILE__, __LINE__);
    const SbSlot s{ dev_mat_a, dev_vec_b, dev_vec_c, dev_vec_b_rowabs };
    THIP_TRY(hipMemcpyAsync(h->slots + i, &s, sizeof(SbSlot), hipMemcpyHostToDevice, ctx().stream));
    THIP_TRY(hipStreamSynchronize(ctx().stream));           // (s is a local)
    THIP_RC(h->launch_init(h, i, 1));
    const auto at = std::lower_bound(h->live.begin(), h->live.end(), i);
    if (at == h->live.end() || *at != i) h->live.insert(at, i);
    return ob_status_one(h, i);
}

}  // namespace
