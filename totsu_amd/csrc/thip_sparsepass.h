// thip_sparsepass.h -- what the batches that hold each problem's own SPARSE A as packed entries share (thip_sparsebatch.hip: one
// shape and one cone layout per batch; thip_raggedsparse.hip: every problem its own shape, layout and pattern): the blob's pass
// (spb_half, spb_pass), the matrix policy of the shared bodies (SpbA; thip_midstream.h), and the host side of the stored form -- the
// capacity of a slot, the thread rule, every refusal of a problem's CSC arrays (spb_validate) and the packing (spb_pack) -- and
// spb_scatter, which gives a blob new values on the device where the pattern stays.  One text:
// a problem's products are the same bits in either family.
// Included once by each of the two translation units (on top of thip_sdpcones.h): everything here is internal to the one that
// includes it.
//
// The blob, in 4-byte words (spb_pack; nnz = cptr[n]):
//   cptr[n + 1]                 column order: the column pointers, from 0
//   nnz x { f32 value, u32 row }          the entries column after column, rows ascending inside a column
//   rptr[m + 1]                 row order: the row pointers, from 0
//   nnz x { f32 value, u32 column }       the same entries row after row, columns ascending inside a row
//   nlr, nlc                    how many rows / columns hold more than SPB_LONG entries
//   nlr rows, nlc columns       those, ascending
// 4 nnz + m + n + 4 + nlr + nlc words; a slot reserves spb_cap_bytes(nnz_cap) = 16 nnz_cap + 4 (2 (m + n) + 4) bytes rounded up to
// 16, so replace can hand a slot another pattern.  The pairs lie at 4-byte alignment (no padding word anywhere: the capacity is exact
// for a full matrix) and are read as two words.
//
// The pass (spb_pass): h = A xn from the row order, g = A^T xt from the column order.  A row of <= SPB_LONG entries is summed by one
// lane -- a serial fmaf chain in stored order from +0, thread t takes the rows t, t + T, .. --, a row on the long list by one wave:
// lane l the entries l, l + 64, .. in a serial chain, then wave_sum_dpp; wave w takes the long rows w, w + nw, ..  The columns
// likewise.  One barrier at entry, one at exit, none between the two products; no atomics: the bits of a product are a function of
// (the problem's data, SPB_LONG) alone, a problem's iterates of (its data, the workgroup size, the constants).
#pragma once

#include "thip_sdpcones.h"

#include <math.h>
#include <stdio.h>

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

// new values into a blob whose pattern stays (thip_NAME_set_a), by one workgroup: w is the blob IN MEMORY, val the nnz new values in
// the column order of its pattern.  The column order takes them as they come, ce[2 e] = val[e].  A row-order entry r of row i holds
// the value of the entry (i, j = re[2 r + 1]), whose place in the column order is found by a binary search for i among the strictly
// ascending rows of column j, ce[2 cptr[j] + 1 ..] -- re[2 r] = val[that place].  The rows are dealt as spb_half deals them: a row
// of <= SPB_LONG entries to one lane, a row on the long list to one wave, lanes striding its entries.  Pointers, index words and the
// long lists are read, never written; every value comes from val, none from the blob, so the two orders are written in any order and
// no word written here is read here.  The result is, word for word, what spb_pack makes of the pattern with the new values.
// The launch is its own, ahead of the kernel that reads the blob (the |A| pass of init, the copy into LDS): values stored by vector
// stores here must not meet a scalar load of the same words that the compiler chose in the same kernel, and a kernel boundary makes
// them visible to every later load of any kind -- one launch per call is the price
__device__ __forceinline__ void spb_scatter(unsigned *w, int m, int n, const float *val)
{
    const int T = (int)blockDim.x, tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = T >> 6;
    const unsigned nnz = w[n];
    const unsigned *const cptr = w;
    unsigned *const ce = w + n + 1;
    const unsigned *const rptr = ce + 2 * (size_t)nnz;
    unsigned *const re = w + n + 1 + 2 * (size_t)nnz + m + 1;
    const unsigned *const lists = re + 2 * (size_t)nnz;
    const int nlr = (int)lists[0];
    auto place = [&](unsigned r, unsigned i) {
        const unsigned j = re[2 * r + 1];
        const unsigned end = cptr[j + 1];
        unsigned lo = cptr[j], hi = end;
        while (lo < hi) {
            const unsigned mid = lo + (hi - lo) / 2;
            if (ce[2 * mid + 1] < i) lo = mid + 1; else hi = mid;
        }
        if (lo < end && ce[2 * lo + 1] == i) re[2 * r] = __float_as_uint(val[lo]);      // (always, in a blob spb_pack made)
    };
    for (int i = tid; i < m; i += T) {
        const unsigned beg = rptr[i], end = rptr[i + 1];
        if (end - beg > (unsigned)SPB_LONG) continue;
        for (unsigned r = beg; r < end; ++r) place(r, (unsigned)i);
    }
    for (int k = wv; k < nlr; k += nw) {                          // (uniform per wave)
        const unsigned i = lists[2 + k];
        const unsigned beg = rptr[i], end = rptr[i + 1];
        for (unsigned r = beg + (unsigned)lane; r < end; r += 64u) place(r, i);
    }
    for (unsigned e = (unsigned)tid; e < nnz; e += (unsigned)T) ce[2 * e] = __float_as_uint(val[e]);
}

// ---- the host side ------------------------------------------------------------------------------------------------------------

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
