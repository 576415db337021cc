// thip_store16.h -- the LIBRARY-OWNED 16-bit store of every problem's A, as the families over one share it (thip_mid16batch.hip,
// thip_wide16batch.hip): the conversion of a range of f32 matrices into their blocks in one launch, the kernel that points every slot
// at its block, the store's hooks (thip_ownbatch.h: ObStore) and the read-back of a block.  The stored form and the pass over it are
// thip_midstream.h's (mb16_block_bytes, mb16_pass_t).  Included once by each of the two translation units: everything here is
// internal to the one that includes it.
//
// The stored form -- per problem n columns of ld16 = roundup4(m) 16-bit words, column-major, the pad rows zero; for THIP_A_F16 n floats
// inv_s behind the matrix; the block a multiple of 16 bytes.  THIP_A_BF16: the word is the f32 rounded to nearest even to its upper
// half (thip_gemv.hip: to_bf16_k's rule).  THIP_A_F16: inv_s[c] = 2^(e - 14) with e the exponent frexp gives the column's largest
// finite |a| (1 for a column of zeros), the word f16(a / inv_s[c]) (f16_scale_k's and to_f16_k's rules).  Both are restated here for a
// whole range of problems in one launch: mid16batch_convert_k.
#pragma once

#include "thip_midstream.h"

#include <math.h>

namespace {

using namespace thip;

// f32 source in, store out: `count` matrices (m n floats each, column-major, one after another at src) into the blocks of the problems
// first .. first + count - 1.  One workgroup per (problem, column), grid-strided: the column's scale (f16), then its ld16 words
struct M16Convert { const float *src; unsigned char *store; size_t block; int n, m, first, count, kind; };

__global__ __launch_bounds__(256) void mid16batch_convert_k(const M16Convert c)
{
    __shared__ float sh[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m = c.m, n = c.n, ld16 = (m + 3) & ~3;
    const size_t total = (size_t)c.count * (size_t)n;
    for (size_t u = blockIdx.x; u < total; u += gridDim.x) {
        const size_t k = u / (size_t)n;
        const int col = (int)(u - k * (size_t)n);
        const float *const src = c.src + u * (size_t)m;                // (the matrices lie one after another: column u of the stack)
        unsigned char *const blk = c.store + ((size_t)c.first + k) * c.block;
        uint16_t *const dst = reinterpret_cast<uint16_t *>(blk) + (size_t)col * (size_t)ld16;
        float inv = 1.0f;
        if (c.kind == THIP_A_F16) {                                    // (uniform: an argument)
            float mx = 0.0f;
            for (int r = tid; r < m; r += 256) {
                const float v = fabsf(src[r]);
                if (v > mx && v <= 3.4028235e38f) mx = v;              // inf / nan do not set the scale
            }
            mx = -wave_min(-mx);
            __syncthreads();                                           // (the previous column's maxima have been read)
            if (lane == 0) sh[w] = mx;
            __syncthreads();
            mx = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
            if (mx > 0.0f) {
                int e;
                (void)frexpf(mx, &e);                                  // mx = f * 2^e, f in [0.5, 1)  =>  mx * 2^(14 - e) in [2^13, 2^14)
                inv = ldexpf(1.0f, e - 14);
            }
            if (tid == 0) reinterpret_cast<float *>(reinterpret_cast<uint16_t *>(blk) + (size_t)n * (size_t)ld16)[col] = inv;
        }
        for (int r = tid; r < ld16; r += 256) {
            unsigned out = 0;
            if (r < m) {
                if (c.kind == THIP_A_BF16) {
                    const unsigned b = __float_as_uint(src[r]);
                    if ((b & 0x7f800000u) == 0x7f800000u) out = (b >> 16) | ((b & 0xffffu) ? 0x40u : 0u);      // inf / nan
                    else out = (b + 0x7fffu + ((b >> 16) & 1u)) >> 16;
                } else {
                    const _Float16 hv = (_Float16)(src[r] / inv);
                    out = __builtin_bit_cast(unsigned short, hv);
                }
            }
            dst[r] = (uint16_t)out;
        }
    }
}

// every slot's `a`: its block of the store
__global__ void mid16batch_slots_k(SbSlot *slots, int n_prob, const unsigned char *store, size_t block)
{
    for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < (size_t)n_prob; p += (size_t)gridDim.x * blockDim.x)
        slots[p].a = reinterpret_cast<const float *>(store + p * block);
}

bool m16_bf16(const OwnBatch *h) { return h->a_kind == THIP_A_BF16; }

// ---- the store (ObStore) ---------------------------------------------------------------------------------------------------------

const float *m16_slot(const OwnBatch *h, size_t p)
{
    return reinterpret_cast<const float *>(static_cast<const unsigned char *>(h->a_store) + p * h->a_block);
}

int m16_convert(OwnBatch *h, int first, int count, const float *dev_src)
{
    const M16Convert c{ dev_src, static_cast<unsigned char *>(h->a_store), h->a_block, (int)h->n, (int)h->m, first, count, h->a_kind };
    hipLaunchKernelGGL(mid16batch_convert_k, dim3(grid_for((size_t)count * h->n, 1, 1u << 20)), dim3(256), 0, ctx().stream, c);
    THIP_LAUNCH_CHECK();
    return 0;
}

int m16_create(OwnBatch *h, const float *dev_mats_a, int kind)
{
    hipStream_t st = ctx().stream;
    h->a_kind = kind == THIP_A_BF16 ? THIP_A_BF16 : THIP_A_F16;        // (thip_NAME_create: f16)
    h->a_block = mb16_block_bytes(h->n, h->m, h->a_kind);
    THIP_RC(ob_alloc(h, &h->a_store, h->a_block * h->n_prob));
    THIP_RC(m16_convert(h, 0, (int)h->n_prob, dev_mats_a));
    hipLaunchKernelGGL(mid16batch_slots_k, dim3(grid_for(h->n_prob, 256, 1024)), dim3(256), 0, st, h->slots, (int)h->n_prob,
                       static_cast<const unsigned char *>(h->a_store), h->a_block);
    THIP_LAUNCH_CHECK();
    for (size_t p = 0; p < h->n_prob; ++p) h->slot_a[p] = m16_slot(h, p);
    THIP_TRY(hipStreamSynchronize(st));                                // (the f32 stack is the caller's again)
    return 0;
}

const ObStore M16_STORE = { m16_create, m16_convert, m16_slot };

// thip_NAME_stored: problem i's block as it lies in the store (the caller has checked that i is a member)
int m16_stored(const OwnBatch *h, int i, uint16_t *host_words, float *host_inv_scale)
{
    const unsigned char *const blk = reinterpret_cast<const unsigned char *>(m16_slot(h, (size_t)i));
    const size_t words = mb16_ld(h->m) * h->n;
    THIP_TRY(hipStreamSynchronize(ctx().stream));
    if (host_words) THIP_TRY(hipMemcpy(host_words, blk, words * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (host_inv_scale && h->a_kind == THIP_A_F16)
        THIP_TRY(hipMemcpy(host_inv_scale, blk + words * sizeof(uint16_t), h->n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace
