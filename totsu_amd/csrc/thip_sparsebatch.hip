// thip_sparsebatch.hip -- thip_sparsebatch: many conic programs of one shape n, m and one cone layout, each with its OWN SPARSE A with
// its own pattern.  The fifth own-A family: the mid batch's iteration (thip_midstream.h: one workgroup per problem, every vector in
// LDS, the carried recurrence, `steps` whole iterations per launch) and the SDP batch's cones (thip_sdpcones.h: all five cones, PSD
// orders <= 64 projected on chip) with another matrix policy -- the slot's `a` pointer is the address of the problem's BLOB, the
// entries of A packed on the host, and a pass walks the entries instead of streaming m n floats.
//
// The blob, the pass over it (spb_pass), the matrix policy (SpbA) and the host side of the stored form (the capacity, the thread
// rule, spb_validate, spb_pack) are thip_sparsepass.h's, one text with thip_raggedsparse.hip.
//
// RESIDENT: when MbMap.bytes + the PSD tail + the blob's capacity fit the LDS of a CU the blob is copied into LDS once per launch
// (16-byte loads) behind the PSD tail and every pass reads it there; otherwise the same code reads the blob in memory (STREAMED: per
// lane 8-byte loads, poorly coalesced -- the fallback).  Both give the same bits.
//
// This file: the two kernels, the family's table and the C API (the generic bodies of
// thip_ownbatch.h; create and replace are the family's own: they take host CSC arrays).
#include "thip_sparsepass.h"

using namespace thip;

namespace {

struct SpbArgs { ObArgs mb; int tail, at, resident; };

__global__ __launch_bounds__(1024) void sparsebatch_init_k(const SpbArgs a) { mb_init_body(a.mb, ObUniform(), SpbA{ a.at, a.resident }); }

__global__ __launch_bounds__(1024) void sparsebatch_k(const SpbArgs a)
{
    mb_iterate_body(a.mb, SpCones{ a.tail }, ObUniform(), SpbA{ a.at, a.resident });
}

// a problem starts from a given iterate (thip_sparsebatch_set_iterates): the pair A x_x, A^T x_y from the blob, resident or streamed
struct SpbStartArgs { ObArgs mb; int at, resident; ObStart s; };

__global__ __launch_bounds__(1024) void sparsebatch_start_k(const SpbStartArgs a)
{
    mb_start_body(a.mb, ob_staged(a.s), ObUniform(), SpbA{ a.at, a.resident });
}

// a problem takes a new (b, c) and keeps its blob (thip_sparsebatch_set_bc): the |A| sums from the blob, resident or streamed
struct SpbSetBcArgs { ObArgs mb; int at, resident; ObSetBc s; };

__global__ __launch_bounds__(1024) void sparsebatch_setbc_k(const SpbSetBcArgs a)
{
    mb_setbc_body(a.mb, a.s, ObUniform(), SpbA{ a.at, a.resident });
}

// a problem's A has new values in its present pattern (thip_sparsebatch_set_a): the scatter into the blob in memory, a launch of its
// own (thip_sparsepass.h says why), then init's body on the new blob, resident or streamed, and under keep the pair again
struct SpbScatterArgs { ObArgs mb; ObStart s; };

__global__ __launch_bounds__(1024) void sparsebatch_scatter_k(const SpbScatterArgs a)
{
    const int p = ob_problem(a.mb.live, a.mb.first);
    spb_scatter(const_cast<unsigned *>(reinterpret_cast<const unsigned *>(a.mb.slots[p].a)), a.mb.m, a.mb.n, ob_staged(a.s));
}

struct SpbSetAArgs { ObArgs mb; int at, resident, keep; };

__global__ __launch_bounds__(1024) void sparsebatch_seta_k(const SpbSetAArgs a)
{
    mb_seta_body(a.mb, a.keep, ObUniform(), SpbA{ a.at, a.resident });
}

__global__ void sparsebatch_slots_k(SbSlot *slots, int n_prob, const unsigned *blobs, size_t cap_words)
{
    for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < (size_t)n_prob; p += (size_t)gridDim.x * blockDim.x)
        slots[p].a = reinterpret_cast<const float *>(blobs + p * cap_words);
}

// ---- the host side ------------------------------------------------------------------------------------------------------------

const ObText SPB_TEXT = { "sparse batch not initialised", "null sparse batch", "a sparse batch holds 1 .. 1048576 problems", nullptr,
                          "the workgroup size is 256 or 1024 (0: by shape)",
                          "thip_test_sparsebatch_force_threads comes before thip_sparsebatch_init" };

}  // namespace

struct thip_sparsebatch : OwnBatch {
    size_t nnz_cap = 0, nnz_total = 0, cap_words = 0, used_words = 0;     // used_words: summed over the slots
    uint32_t *blobs = nullptr;
    std::vector<uint32_t> slot_nnz, slot_used;
    int resident = 0, force_resident = -1;
};

namespace {

bool spb_can_reside(const thip_sparsebatch *h)
{
    return sp_lds_for(h->n, h->m, 0, h->psd) + h->cap_words * 4 <= OB_LDS_MAX;
}

// the workgroup size, the mode and the LDS of one workgroup
void spb_plan(thip_sparsebatch *h)
{
    h->threads = h->forced ? h->forced : spb_threads_for(h->n, h->m, h->nnz_cap);
    h->resident = h->force_resident >= 0 ? h->force_resident : (spb_can_reside(h) ? 1 : 0);
    h->lds = sp_lds_for(h->n, h->m, h->threads, h->psd) + (h->resident ? h->cap_words * 4 : 0);
}

int spb_launch(const OwnBatch *ob, bool run, const ObArgs &a, unsigned count)
{
    const thip_sparsebatch *h = static_cast<const thip_sparsebatch *>(ob);
    const int tail = (int)(MbMap((int)h->n, (int)h->m).bytes((int)h->m) / sizeof(float));
    const SpbArgs s{ a, tail, tail + (int)(h->psd.tail_bytes / sizeof(float)), h->resident };
    return ob_launch(ob, run ? sparsebatch_k : sparsebatch_init_k, s, count);
}

int spb_start(const OwnBatch *ob, const ObArgs &a, const ObStart &s, unsigned count)
{
    const thip_sparsebatch *h = static_cast<const thip_sparsebatch *>(ob);
    const int tail = (int)(MbMap((int)h->n, (int)h->m).bytes((int)h->m) / sizeof(float));
    return ob_launch(ob, sparsebatch_start_k, SpbStartArgs{ a, tail + (int)(h->psd.tail_bytes / sizeof(float)), h->resident, s }, count);
}

int spb_threads_unused(size_t, size_t) { return 1024; }      // (the table's thread choice knows no nnz_cap: spb_plan decides)

int spb_setbc(const OwnBatch *ob, const ObArgs &a, const ObSetBc &s, unsigned count)
{
    const thip_sparsebatch *h = static_cast<const thip_sparsebatch *>(ob);
    const int tail = (int)(MbMap((int)h->n, (int)h->m).bytes((int)h->m) / sizeof(float));
    return ob_launch(ob, sparsebatch_setbc_k, SpbSetBcArgs{ a, tail + (int)(h->psd.tail_bytes / sizeof(float)), h->resident, s }, count);
}

// the scatter (no LDS) and then the set_a kernel
int spb_seta(const OwnBatch *ob, const ObArgs &a, const ObSetA &s, unsigned count)
{
    const thip_sparsebatch *h = static_cast<const thip_sparsebatch *>(ob);
    const int tail = (int)(MbMap((int)h->n, (int)h->m).bytes((int)h->m) / sizeof(float));
    hipLaunchKernelGGL(sparsebatch_scatter_k, dim3(count), dim3((unsigned)h->threads), 0, ctx().stream, SpbScatterArgs{ a, s.s });
    THIP_LAUNCH_CHECK();
    return ob_launch(ob, sparsebatch_seta_k, SpbSetAArgs{ a, tail + (int)(h->psd.tail_bytes / sizeof(float)), h->resident, s.keep }, count);
}

ObFamily SPB_FAMILY = { SPB_TEXT, { 256, 1024, 0 }, false, sp_check, spb_threads_unused, sp_lds_for, mb_stride, spb_launch, spb_start,
                        spb_setbc, spb_seta,
                        { (const void *)sparsebatch_k, (const void *)sparsebatch_init_k, (const void *)sparsebatch_start_k,
                          (const void *)sparsebatch_setbc_k, (const void *)sparsebatch_seta_k, nullptr } };

// the rule (no device needed): sp_check's on (n, m, layout); the blob is resident when it fits behind the vectors and the PSD tail
int spb_fits(size_t n, size_t m, size_t nnz_cap, size_t n_seg, const int32_t *seg_type, const int64_t *seg_len, size_t *host_lds_bytes,
             int *host_threads, int *host_resident, std::vector<int> *cones = nullptr, std::vector<unsigned char> *cls = nullptr,
             ObPsd *psd_out = nullptr)
{
    ObPsd psd;
    THIP_RC(sp_check(n, m, n_seg, seg_type, seg_len, cones, cls, &psd));
    if (nnz_cap > m * n) {
        char msg[120];
        snprintf(msg, sizeof(msg), "nnz_cap %zu exceeds m n = %zu", nnz_cap, m * n);
        return fail(THIP_E_INVALID, msg, __FILE__, __LINE__);
    }
    const size_t vec = sp_lds_for(n, m, 0, psd), cap = spb_cap_bytes(n, m, nnz_cap);
    const bool res = vec + cap <= OB_LDS_MAX;
    if (host_lds_bytes) *host_lds_bytes = vec + (res ? cap : 0);
    if (host_threads) *host_threads = spb_threads_for(n, m, nnz_cap);
    if (host_resident) *host_resident = res ? 1 : 0;
    if (psd_out) *psd_out = psd;
    return 0;
}

struct SpbInfo {
    void operator()(const OwnBatch *ob, thip_sparsebatch_info_t &o) const
    {
        const thip_sparsebatch *h = static_cast<const thip_sparsebatch *>(ob);
        ObInfo()(ob, o);
        o.max_psd_order = h->psd.max_k; o.n_psd = h->psd.n_psd;
        o.psd_lds_bytes = h->psd.tail_bytes;
        o.nnz_cap = h->nnz_cap; o.nnz_total = h->nnz_total; o.blob_bytes = h->cap_words * 4;
        o.resident = h->resident;
        o.a_bytes_per_iter = h->resident ? 0 : 2 * 4 * (h->used_words / h->n_prob);
    }
};

int spb_destroy(thip_sparsebatch *h)
{
    if (!h) return 0;
    if (ctx().inited) hipStreamSynchronize(ctx().stream);
    hipFree(h->blobs);
    return ob_destroy(h);
}

// slot i's record of what it holds
void spb_account(thip_sparsebatch *h, size_t i, size_t nnz, size_t used)
{
    h->nnz_total += nnz; h->nnz_total -= h->slot_nnz[i];
    h->used_words += used; h->used_words -= h->slot_used[i];
    h->slot_nnz[i] = (uint32_t)nnz; h->slot_used[i] = (uint32_t)used;
}

}  // namespace

extern "C" {

int thip_sparsebatch_fits(size_t n, size_t m, size_t nnz_cap, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                          size_t *host_lds_bytes, int *host_threads, int *host_resident)
{
    return spb_fits(n, m, nnz_cap, n_seg, host_seg_type, host_seg_len, host_lds_bytes, host_threads, host_resident);
}

int thip_sparsebatch_destroy(thip_sparsebatch *h) { return spb_destroy(h); }

int thip_sparsebatch_create(size_t n, size_t m, size_t n_prob, const int64_t *host_colptr, const int64_t *host_start,
                            const int32_t *host_rowidx, const float *host_values, const float *dev_vecs_b, const float *dev_vecs_c,
                            const float *dev_vecs_b_rowabs, size_t nnz_cap, size_t n_seg, const int32_t *host_seg_type,
                            const int64_t *host_seg_len, const thip_param *par, thip_sparsebatch **out)
{
    if (!out) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *out = nullptr;
    THIP_NEED_INIT();
    if (!par || !host_colptr || !host_start || !dev_vecs_b || !dev_vecs_c) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (n_prob < 1 || n_prob > OB_MAX_PROB) return fail(THIP_E_INVALID, SPB_TEXT.count, __FILE__, __LINE__);
    if (par->state_arith != THIP_STATE_COMPENSATED && par->state_arith != THIP_STATE_PLAIN)
        return fail(THIP_E_INVALID, "bad thip_param.state_arith", __FILE__, __LINE__);
    if (((uintptr_t)dev_vecs_b | (uintptr_t)dev_vecs_c | (uintptr_t)dev_vecs_b_rowabs) & 3u)
        return fail(THIP_E_INVALID, "the arrays hold floats: 4-byte alignment", __FILE__, __LINE__);
    // the shape first (so that n, m are sane), then every problem's arrays, then nnz_cap: all before the first allocation
    THIP_RC(spb_fits(n, m, 0, n_seg, host_seg_type, host_seg_len, nullptr, nullptr, nullptr));
    size_t largest = 0;
    for (size_t p = 0; p < n_prob; ++p) {
        const int64_t *cp = host_colptr + p * (n + 1);
        if (host_start[p] < 0) return fail(THIP_E_INVALID, "a negative start offset", __FILE__, __LINE__);
        THIP_RC(spb_validate(n, m, cp, host_rowidx ? host_rowidx + host_start[p] : nullptr, host_values ? host_values + host_start[p] : nullptr,
                             nnz_cap ? nnz_cap : m * n, (long)p));
        largest = std::max(largest, (size_t)cp[n]);
    }
    if (nnz_cap == 0) nnz_cap = largest;
    thip_sparsebatch *h = new thip_sparsebatch();
    h->fam = &SPB_FAMILY;
    int rc = spb_fits(n, m, nnz_cap, n_seg, host_seg_type, host_seg_len, nullptr, nullptr, nullptr, &h->cones, &h->cls, &h->psd);
    if (rc != 0) { delete h; return rc; }
    h->n = n; h->m = m; h->n_prob = n_prob;
    h->par = *par;
    h->stride = mb_stride(n, m);
    h->nnz_cap = nnz_cap;
    h->cap_words = spb_cap_bytes(n, m, nnz_cap) / 4;
    h->slot_nnz.assign(n_prob, 0); h->slot_used.assign(n_prob, 0);
    spb_plan(h);
    // every blob packed on the host, one copy up
    std::vector<uint32_t> host(h->cap_words * n_prob, 0u);
    for (size_t p = 0; p < n_prob; ++p) {
        const int64_t *cp = host_colptr + p * (n + 1);
        const size_t used = spb_pack(n, m, cp, host_rowidx + host_start[p], host_values + host_start[p], host.data() + p * h->cap_words);
        spb_account(h, p, (size_t)cp[n], used);
    }
    rc = ob_attr(SPB_FAMILY);
    if (rc == 0) rc = ob_alloc(h, (void **)&h->blobs, host.size() * sizeof(uint32_t));
    if (rc == 0) rc = ob_build(h, nullptr, dev_vecs_b, dev_vecs_c, dev_vecs_b_rowabs);
    if (rc == 0) {
        const hipError_t e = hipMemcpy(h->blobs, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) rc = fail((int)e, "hipMemcpy of the blobs", __FILE__, __LINE__);
    }
    if (rc == 0) {
        hipLaunchKernelGGL(sparsebatch_slots_k, dim3(grid_for(n_prob, 256, 1024)), dim3(256), 0, ctx().stream, h->slots, (int)n_prob,
                           h->blobs, h->cap_words);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = fail((int)e, "sparsebatch_slots_k", __FILE__, __LINE__);
    }
    if (rc != 0) { spb_destroy(h); return rc; }
    *out = h;
    return 0;
}

int thip_sparsebatch_set_param(thip_sparsebatch *h, const thip_param *par) { return ob_set_param(h, par); }
int thip_sparsebatch_init(thip_sparsebatch *h) { return ob_init(SPB_FAMILY, h); }
int thip_sparsebatch_run(thip_sparsebatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{ return ob_run(SPB_FAMILY, h, max_steps, poll_every, host_status, false); }
int thip_sparsebatch_run_until_any(thip_sparsebatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{ return ob_run(SPB_FAMILY, h, max_steps, poll_every, host_status, true); }
int thip_sparsebatch_status(thip_sparsebatch *h, int i, thip_status *host_status) { return ob_status(SPB_FAMILY, h, i, host_status); }
int thip_sparsebatch_solution(thip_sparsebatch *h, int i, float *host_x, float *host_y) { return ob_solution(SPB_FAMILY, h, i, host_x, host_y); }
int thip_sparsebatch_iterate(thip_sparsebatch *h, int i, float *host_x, float *host_y) { return ob_iterate(SPB_FAMILY, h, i, host_x, host_y); }
int thip_sparsebatch_precond(thip_sparsebatch *h, int i, float *host_dp_tau, float *host_dp_sigma)
{ return ob_precond(SPB_FAMILY, h, i, host_dp_tau, host_dp_sigma); }
int thip_sparsebatch_set_iterates(thip_sparsebatch *h, int first, int count, const float *host_x, const float *host_y)
{ return ob_set_iterates(SPB_FAMILY, h, first, count, host_x, host_y); }
int thip_sparsebatch_set_bc(thip_sparsebatch *h, int first, int count, const float *host_b, const float *host_c,
                            const float *host_b_rowabs, const uint8_t *host_has_rowabs, int keep_iterate)
{ return ob_set_bc(SPB_FAMILY, h, first, count, host_b, host_c, host_b_rowabs, host_has_rowabs, keep_iterate); }
int thip_sparsebatch_solutions(thip_sparsebatch *h, int first, int count, float *host_x, float *host_y, thip_status *host_status)
{ return ob_solutions(SPB_FAMILY, h, first, count, host_x, host_y, host_status); }
int thip_sparsebatch_info(const thip_sparsebatch *h, thip_sparsebatch_info_t *host_info) { return ob_info_out(h, host_info, SpbInfo()); }

// one upload -- where each workgroup's values begin (the counts differ), then the values, 4 bytes per entry -- and two launches
int thip_sparsebatch_set_a(thip_sparsebatch *h, int first, int count, const float *host_values, const int64_t *host_counts, int keep_iterate)
{
    THIP_NEED_INIT();
    size_t total = 0;
    THIP_RC(ob_seta_check(SPB_FAMILY, h, first, count, host_values, host_counts, [&](int p) { return (size_t)h->slot_nnz[(size_t)p]; },
                          OB_SETA_SPARSE, &total));
    const size_t cnt = (size_t)count, head = cnt * sizeof(long long), bytes = head + total * sizeof(float);
    void *pinned = nullptr;
    THIP_RC(ob_stage_reserve(h, bytes, &pinned));
    long long *const at = static_cast<long long *>(pinned);
    size_t o = 0;
    for (size_t k = 0; k < cnt; ++k) { at[k] = (long long)o; o += h->slot_nnz[(size_t)first + k]; }
    if (total) memcpy(static_cast<unsigned char *>(pinned) + head, host_values, total * sizeof(float));
    return ob_start_staged(h, first, count, bytes, [&](const void *stage) {
        const unsigned char *const dev = static_cast<const unsigned char *>(stage);
        ObArgs a = ob_args(h);
        a.first = first;
        const ObSetA s{ ObStart{ reinterpret_cast<const float *>(dev + head), reinterpret_cast<const long long *>(dev), 0 }, keep_iterate != 0 };
        return SPB_FAMILY.seta(h, a, s, (unsigned)count);
    });
}

int thip_sparsebatch_set_bc_dev(thip_sparsebatch *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_b_rowabs,
                                const uint8_t *host_has_rowabs, int keep_iterate)
{ return ob_set_bc_dev(SPB_FAMILY, h, first, count, dev_b, dev_c, dev_b_rowabs, host_has_rowabs, keep_iterate); }
int thip_sparsebatch_set_iterates_dev(thip_sparsebatch *h, int first, int count, const float *dev_x, const float *dev_y)
{ return ob_set_iterates_dev(SPB_FAMILY, h, first, count, dev_x, dev_y); }
int thip_sparsebatch_solutions_dev(thip_sparsebatch *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state)
{ return ob_solutions_dev(SPB_FAMILY, h, first, count, dev_x, dev_y, dev_state); }

// the values stay where the caller holds them: only the table of where each workgroup's begin goes up, and the scatter reads them there
int thip_sparsebatch_set_a_dev(thip_sparsebatch *h, int first, int count, const float *dev_values, int keep_iterate)
{
    const size_t cnt = count > 0 ? (size_t)count : 0;
    return ob_set_a_dev_sparse_t(SPB_FAMILY, h, first, count, dev_values, [&](int p) { return (size_t)h->slot_nnz[(size_t)p]; },
                                 cnt * sizeof(long long),
                                 [&](unsigned char *pin, const std::vector<long long> &at_p) { memcpy(pin, at_p.data(), cnt * sizeof(long long)); },
                                 [&](const unsigned char *dev_head) {
                                     ObArgs a = ob_args(h);
                                     a.first = first;
                                     const ObSetA s{ ObStart{ dev_values, reinterpret_cast<const long long *>(dev_head), 0 }, keep_iterate != 0 };
                                     return SPB_FAMILY.seta(h, a, s, (unsigned)count);
                                 });
}

int thip_sparsebatch_replace(thip_sparsebatch *h, int i, const int64_t *host_colptr, const int32_t *host_rowidx, const float *host_values,
                             const float *dev_vec_b, const float *dev_vec_c, const float *dev_vec_b_rowabs)
{
    THIP_NEED_INIT();
    THIP_RC(ob_member(SPB_FAMILY, h, i));
    if (!host_colptr || !dev_vec_b || !dev_vec_c) return fail(THIP_E_INVALID, "null A, b or c", __FILE__, __LINE__);
    THIP_RC(spb_validate(h->n, h->m, host_colptr, host_rowidx, host_values, h->nnz_cap, -1));
    std::vector<uint32_t> host(h->cap_words, 0u);
    const size_t used = spb_pack(h->n, h->m, host_colptr, host_rowidx, host_values, host.data());
    uint32_t *const blob = h->blobs + (size_t)i * h->cap_words;
    THIP_TRY(hipStreamSynchronize(ctx().stream));                // (no launch is reading the slot)
    THIP_TRY(hipMemcpy(blob, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    THIP_RC(ob_replace(SPB_FAMILY, h, i, reinterpret_cast<const float *>(blob), dev_vec_b, dev_vec_c, dev_vec_b_rowabs));
    spb_account(h, (size_t)i, (size_t)host_colptr[h->n], used);
    return 0;
}

int thip_test_sparsebatch_force_threads(thip_sparsebatch *h, int threads)
{
    THIP_RC(ob_force_threads(SPB_FAMILY, h, threads));
    spb_plan(h);
    return 0;
}

int thip_test_sparsebatch_force_resident(thip_sparsebatch *h, int resident)
{
    if (!h) return fail(THIP_E_INVALID, SPB_TEXT.null_h, __FILE__, __LINE__);
    if (resident != 0 && resident != 1) return fail(THIP_E_INVALID, "the mode is 0 (streamed) or 1 (resident)", __FILE__, __LINE__);
    if (h->inited) return fail(THIP_E_INVALID, "thip_test_sparsebatch_force_resident comes before thip_sparsebatch_init", __FILE__, __LINE__);
    if (resident == 1 && !spb_can_reside(h))
        return fail(THIP_E_INVALID, "the blob does not fit the LDS left beside the vectors: it cannot be resident", __FILE__, __LINE__);
    h->force_resident = resident;
    spb_plan(h);
    return 0;
}

int thip_test_sparsebatch_blob(thip_sparsebatch *h, int i, uint32_t *host_words, size_t cap_words, size_t *host_used_words)
{
    THIP_NEED_INIT();
    if (!h || !host_used_words) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (i < 0 || (size_t)i >= h->n_prob) return fail(THIP_E_INVALID, "no such problem", __FILE__, __LINE__);
    const size_t used = h->slot_used[(size_t)i];
    *host_used_words = used;
    if (!host_words) return 0;
    if (cap_words < used) return fail(THIP_E_INVALID, "the blob holds more words than were offered", __FILE__, __LINE__);
    THIP_TRY(hipStreamSynchronize(ctx().stream));
    THIP_TRY(hipMemcpy(host_words, h->blobs + (size_t)i * h->cap_words, used * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int thip_test_sparsebatch_pack(size_t n, size_t m, const int64_t *host_colptr, const int32_t *host_rowidx, const float *host_values,
                               size_t nnz_cap, uint32_t *host_words, size_t cap_words, size_t *host_used_words, int *host_long)
{
    if (!host_colptr || !host_used_words) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (host_long) *host_long = SPB_LONG;
    if (n < 1 || m < 1 || n > MB_MAX_DIM || m > MB_MAX_DIM) return fail(THIP_E_INVALID, "1 <= m, n <= 4096", __FILE__, __LINE__);
    if (nnz_cap > m * n) {
        char msg[120];
        snprintf(msg, sizeof(msg), "nnz_cap %zu exceeds m n = %zu", nnz_cap, m * n);
        return fail(THIP_E_INVALID, msg, __FILE__, __LINE__);
    }
    THIP_RC(spb_validate(n, m, host_colptr, host_rowidx, host_values, nnz_cap ? nnz_cap : m * n, -1));
    const size_t need = spb_cap_bytes(n, m, (size_t)host_colptr[n]) / 4;
    std::vector<uint32_t> tmp(need, 0u);
    const size_t used = spb_pack(n, m, host_colptr, host_rowidx, host_values, tmp.data());
    *host_used_words = used;
    if (host_words) {
        if (cap_words < used) return fail(THIP_E_INVALID, "the blob needs more words than were offered", __FILE__, __LINE__);
        memcpy(host_words, tmp.data(), used * sizeof(uint32_t));
    }
    return 0;
}

}  // extern "C"
