// thip_sparsebatch.hip -- thip_sparsebatch: many conic programs of one shape n, m and one cone layout, each with its OWN SPARSE A with
// its own pattern.  The fifth own-A family: the mid batch's iteration (thip_midstream.h: one workgroup per problem, every vector in
// LDS, the carried recurrence, `steps` whole iterations per launch) and the SDP batch's cones (thip_sdpcones.h: all five cones, PSD
// orders <= 64 projected on chip) with another matrix policy -- the slot's `a` pointer is the address of the problem's BLOB, the
// entries of A packed on the host, and a pass walks the entries instead of streaming m n floats.
//
// The blob, in 4-byte words (spb_pack; nnz = cptr[n]):
//   cptr[n + 1]                 column order: the column pointers, from 0
//   nnz x { f32 value, u32 row }          the entries column after column, rows ascending inside a column
//   rptr[m + 1]                 row order: the row pointers, from 0
//   nnz x { f32 value, u32 column }       the same entries row after row, columns ascending inside a row
//   nlr, nlc                    how many rows / columns hold more than SPB_LONG entries
//   nlr rows, nlc columns       those, ascending
// 4 nnz + m + n + 4 + nlr + nlc words; every slot reserves spb_cap_bytes(nnz_cap) = 16 nnz_cap + 4 (2 (m + n) + 4) bytes rounded up to
// 16, so replace can hand a slot another pattern.  The pairs lie at 4-byte alignment (no padding word anywhere: the capacity is exact
// for a full matrix) and are read as two words.
//
// The pass (spb_pass): h = A xn from the row order, g = A^T xt from the column order.  A row of <= SPB_LONG entries is summed by one
// lane -- a serial fmaf chain in stored order from +0, thread t takes the rows t, t + T, .. --, a row on the long list by one wave:
// lane l the entries l, l + 64, .. in a serial chain, then wave_sum_dpp; wave w takes the long rows w, w + nw, ..  The columns
// likewise.  One barrier at entry, one at exit, none between the two products; no atomics: the bits of a product are a function of
// (the problem's data, SPB_LONG) alone, a problem's iterates of (its data, the workgroup size, the constants).
//
// RESIDENT: when MbMap.bytes + the PSD tail + the blob's capacity fit the LDS of a CU the blob is copied into LDS once per launch
// (16-byte loads) behind the PSD tail and every pass reads it there; otherwise the same code reads the blob in memory (STREAMED: per
// lane 8-byte loads, poorly coalesced -- the fallback).  Both give the same bits.
//
// This file: the pass, the policy, the two kernels, the packing, the family's table and the C API (the generic bodies of
// thip_ownbatch.h; create and replace are the family's own: they take host CSC arrays).
#include "thip_sdpcones.h"

#include <math.h>
#include <stdio.h>

using namespace thip;

namespace {

#ifndef SPB_LONG
#define SPB_LONG 32
#endif
static_assert(SPB_LONG >= 1, "a row is short or long");

struct SpbEntry { float v; unsigned i; };

// h[i] = sum over the entries of row / column i (ptr, ent: one order of the blob), x gathered by the entry's index; list: the nl long ones
template <bool ABS>
__device__ __forceinline__ void spb_half(const unsigned *ptr, const unsigned *ent, const unsigned *list, int nl, int cnt,
                                         const float *x, float *out)
{
    const int T = (int)blockDim.x, tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = T >> 6;
    auto term = [&](unsigned e, float acc) {
        const float v = __uint_as_float(ent[2 * e]);
        return ABS ? acc + fabsf(v) : fmaf(v, x[ent[2 * e + 1]], acc);
    };
    for (int i = tid; i < cnt; i += T) {
        const unsigned beg = ptr[i], end = ptr[i + 1];
        if (end - beg > (unsigned)SPB_LONG) continue;
        float acc = 0.0f;
        for (unsigned e = beg; e < end; ++e) acc = term(e, acc);
        out[i] = acc;
    }
    for (int k = wv; k < nl; k += nw) {                           // (uniform per wave)
        const unsigned i = list[k];
        const unsigned beg = ptr[i], end = ptr[i + 1];
        float acc = 0.0f;
        for (unsigned e = beg + (unsigned)lane; e < end; e += 64u) acc = term(e, acc);
        acc = wave_sum_dpp(acc);
        if (lane == 0) out[i] = acc;
    }
}

// h = A xn (m), g = A^T xt (n) from the blob w (ABS: the row and column sums of |A|).  RESIDENT: w is in LDS, else in memory -- one
// text.  Begins and ends with a barrier, as mb_pass does
template <bool ABS, bool RESIDENT>
__device__ __forceinline__ void spb_pass(const unsigned *w, int m, int n, const float *xn, const float *xt, float *h, float *g)
{
    __syncthreads();
    const unsigned nnz = w[n];
    const unsigned *const cptr = w, *const ce = w + n + 1;
    const unsigned *const rptr = ce + 2 * (size_t)nnz, *const re = rptr + m + 1;
    const unsigned *const lists = re + 2 * (size_t)nnz;
    const int nlr = (int)lists[0], nlc = (int)lists[1];
    spb_half<ABS>(rptr, re, lists + 2, nlr, m, xn, h);
    spb_half<ABS>(cptr, ce, lists + 2 + nlr, nlc, n, xt, g);
    __syncthreads();
}

// the matrix policy (thip_midstream.h) of a sparse A: the slot's `a` is the blob's address.  at: where the resident copy lies in
// LDS, in floats (behind the PSD tail); resident: the launch holds the blob in LDS
struct SpbA {
    int at, resident;
    struct Mat { const unsigned *w; };
    __device__ __forceinline__ Mat open(const float *a, int m, int n, float *S) const
    {
        const unsigned *const w = reinterpret_cast<const unsigned *>(a);
        if (resident) {
            const unsigned nnz = w[n];
            const size_t lists = (size_t)n + 1 + (size_t)m + 1 + 4 * (size_t)nnz;
            const unsigned used = (unsigned)lists + 2u + w[lists] + w[lists + 1];      // <= the capacity: spb_pack
            const uint4 *const src = reinterpret_cast<const uint4 *>(w);                // (a slot's blob is 16-byte aligned and the
            unsigned *const dst = reinterpret_cast<unsigned *>(S + at);                 // capacity a multiple of 16)
            for (unsigned i = threadIdx.x; i < (used + 3u) / 4u; i += blockDim.x) {
                const uint4 q = src[i];
                dst[4 * i] = q.x; dst[4 * i + 1] = q.y; dst[4 * i + 2] = q.z; dst[4 * i + 3] = q.w;
            }
        }
        return Mat{ w };
    }
    template <bool ABS>
    __device__ __forceinline__ void pass(const Mat &M, int m, int n, const float *xn, const float *xt, float *h, float *g, float *,
                                         float *) const
    {
        if (resident) spb_pass<ABS, true>(reinterpret_cast<const unsigned *>(mb_lds + at), m, n, xn, xt, h, g);
        else spb_pass<ABS, false>(M.w, m, n, xn, xt, h, g);
    }
};

struct SpbArgs { ObArgs mb; int tail, at, resident; };

__global__ __launch_bounds__(1024) void sparsebatch_init_k(const SpbArgs a) { mb_init_body(a.mb, ObUniform(), SpbA{ a.at, a.resident }); }

__global__ __launch_bounds__(1024) void sparsebatch_k(const SpbArgs a)
{
    mb_iterate_body(a.mb, SpCones{ a.tail }, ObUniform(), SpbA{ a.at, a.resident });
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

size_t spb_cap_bytes(size_t n, size_t m, size_t nnz_cap) { return (16 * nnz_cap + 4 * (2 * (m + n) + 4) + 15) & ~(size_t)15; }

int spb_threads_for(size_t n, size_t m, size_t nnz_cap) { return std::max(m, n) <= 1024 && nnz_cap <= 8192 ? 256 : 1024; }

// one problem's CSC arrays (colptr: n + 1 entries from 0; rowidx, val: colptr[n] entries): every refusal of the stored form
int spb_validate(size_t n, size_t m, const int64_t *colptr, const int32_t *rowidx, const float *val, size_t nnz_cap, long prob)
{
    char msg[200];
    auto refuse = [&](const char *what) {
        if (prob >= 0) snprintf(msg, sizeof(msg), "problem %ld: %s", prob, what);
        else snprintf(msg, sizeof(msg), "%s", what);
        return fail(THIP_E_INVALID, msg, __FILE__, __LINE__);
    };
    if (colptr[0] != 0) return refuse("the column pointers are not monotone from 0");
    for (size_t j = 0; j < n; ++j)
        if (colptr[j + 1] < colptr[j]) return refuse("the column pointers are not monotone from 0");
    const int64_t nnz = colptr[n];
    if ((uint64_t)nnz > (uint64_t)m * n || (uint64_t)nnz > nnz_cap) {
        char what[120];
        snprintf(what, sizeof(what), "%lld entries where nnz_cap is %zu", (long long)nnz, nnz_cap);
        return refuse(what);
    }
    if (nnz && (!rowidx || !val)) return refuse("null row indices or values");
    for (size_t j = 0; j < n; ++j)
        for (int64_t e = colptr[j]; e < colptr[j + 1]; ++e) {
            if (rowidx[e] < 0 || (size_t)rowidx[e] >= m) return refuse("a row index is out of range");
            if (e > colptr[j] && rowidx[e] <= rowidx[e - 1]) return refuse("the row indices of a column are not strictly ascending");
            if (!isfinite(val[e])) return refuse("a value of A is not finite");
        }
    return 0;
}

// the blob of a validated problem into out (spb_cap_bytes(nnz) / 4 words are enough); returns the words used
size_t spb_pack(size_t n, size_t m, const int64_t *colptr, const int32_t *rowidx, const float *val, uint32_t *out)
{
    const size_t nnz = (size_t)colptr[n];
    uint32_t *cptr = out, *ce = out + n + 1, *rptr = ce + 2 * nnz, *re = rptr + m + 1, *lists = re + 2 * nnz;
    auto bits = [](float v) { uint32_t u; memcpy(&u, &v, 4); return u; };
    for (size_t j = 0; j <= n; ++j) cptr[j] = (uint32_t)colptr[j];
    for (size_t i = 0; i <= m; ++i) rptr[i] = 0;
    for (size_t e = 0; e < nnz; ++e) { ce[2 * e] = bits(val[e]); ce[2 * e + 1] = (uint32_t)rowidx[e]; rptr[rowidx[e] + 1] += 1; }
    for (size_t i = 0; i < m; ++i) rptr[i + 1] += rptr[i];
    std::vector<uint32_t> next(rptr, rptr + m);
    for (size_t j = 0; j < n; ++j)                                  // (columns in order: ascending inside every row)
        for (int64_t e = colptr[j]; e < colptr[j + 1]; ++e) {
            const uint32_t at = next[(size_t)rowidx[e]]++;
            re[2 * at] = bits(val[e]); re[2 * at + 1] = (uint32_t)j;
        }
    uint32_t nlr = 0, nlc = 0;
    for (size_t i = 0; i < m; ++i) if (rptr[i + 1] - rptr[i] > (uint32_t)SPB_LONG) lists[2 + nlr++] = (uint32_t)i;
    for (size_t j = 0; j < n; ++j) if (cptr[j + 1] - cptr[j] > (uint32_t)SPB_LONG) lists[2 + nlr + nlc++] = (uint32_t)j;
    lists[0] = nlr; lists[1] = nlc;
    return (size_t)(lists - out) + 2 + nlr + nlc;
}

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

int spb_threads_unused(size_t, size_t) { return 1024; }      // (the table's thread choice knows no nnz_cap: spb_plan decides)

ObFamily SPB_FAMILY = { SPB_TEXT, { 256, 1024, 0 }, false, sp_check, spb_threads_unused, sp_lds_for, mb_stride, spb_launch,
                        { (const void *)sparsebatch_k, (const void *)sparsebatch_init_k, nullptr } };

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
int thip_sparsebatch_info(const thip_sparsebatch *h, thip_sparsebatch_info_t *host_info) { return ob_info_out(h, host_info, SpbInfo()); }

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
