// thip_mid16batch.hip -- thip_mid16batch: the mid batch (thip_midbatch.hip: many MID-SIZE conic programs of one shape and cone layout,
// each with its OWN dense A, one workgroup per problem, every vector in LDS, A streamed twice per iteration) over a LIBRARY-OWNED
// 16-bit copy of every problem's A: half the bytes per pass, half the memory, one load path for every m.
//
// The stored form (thip_midstream.h: mb16_pass_t) -- per problem n columns of ld16 = roundup4(m) 16-bit words, column-major, the pad
// rows zero; for THIP_A_F16 n floats inv_s behind the matrix; the block a multiple of 16 bytes.  THIP_A_BF16: the word is the f32
// rounded to nearest even to its upper half (thip_gemv.hip: to_bf16_k's rule).  THIP_A_F16: inv_s[c] = 2^(e - 14) with e the exponent
// frexp gives the column's largest finite |a| (1 for a column of zeros), the word f16(a / inv_s[c]) (f16_scale_k's and to_f16_k's
// rules).  Both are restated here for a whole range of problems in one launch: mid16batch_convert_k.
//
// The contract: the batch is, bit for bit, a thip_midbatch that holds the WIDENED matrix W in f32 -- W(r, c) the bf16 word shifted
// left 16 bits, or float(h(r, c)) * inv_s[c] in f32 -- preconditioner, iterates, Kahan terms, carried pair, status blocks, at every
// workgroup size, in both state arithmetics, however the iterations are cut into launches: the pass deals the entries to the lanes and
// orders the additions as mb_pass_t does.  The problem solved is the one with the rounded matrix.
//
// This file: the five kernels (per stored form), the conversion, the store's hooks (thip_ownbatch.h: ObStore), the family's table and
// what the family adds to the C API; the rest of the API is thip_ownbatch.h's.
#include "thip_midstream.h"

#include <math.h>

using namespace thip;

namespace {

template <int KIND>
__global__ __launch_bounds__(1024) void mid16batch_init_k(const ObArgs a) { mb_init_body(a, ObUniform(), MbDenseA16<KIND>()); }

template <int KIND>
__global__ __launch_bounds__(1024) void mid16batch_k(const ObArgs a) { mb_iterate_body(a, MbNoPsd(), ObUniform(), MbDenseA16<KIND>()); }

struct M16StartArgs { ObArgs mb; ObStart s; };

template <int KIND>
__global__ __launch_bounds__(1024) void mid16batch_start_k(const M16StartArgs a)
{
    mb_start_body(a.mb, ob_staged(a.s), ObUniform(), MbDenseA16<KIND>());
}

struct M16SetBcArgs { ObArgs mb; ObSetBc s; };

template <int KIND>
__global__ __launch_bounds__(1024) void mid16batch_setbc_k(const M16SetBcArgs a) { mb_setbc_body(a.mb, a.s, ObUniform(), MbDenseA16<KIND>()); }

struct M16SetAArgs { ObArgs mb; int keep; };

template <int KIND>
__global__ __launch_bounds__(1024) void mid16batch_seta_k(const M16SetAArgs a) { mb_seta_body(a.mb, a.keep, ObUniform(), MbDenseA16<KIND>()); }

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

const ObText M16_TEXT = { "mid16 batch not initialised", "null mid16 batch", "a mid16 batch holds 1 .. 1048576 problems",
                          "a mid16 batch takes no PSD segment (PSD cones over a 16-bit A are not built; thip_sdpbatch streams f32)",
                          "the workgroup size is 256 or 1024 (0: by shape)",
                          "thip_test_mid16batch_force_threads comes before thip_mid16batch_init" };

// the shape rule is the mid batch's, unchanged (the LDS map is MbMap): a PSD segment in this family's words, then thip_midbatch_fits
int m16_check(size_t n, size_t m, size_t n_seg, const int32_t *seg_type, const int64_t *seg_len, std::vector<int> *cones,
              std::vector<unsigned char> *cls, ObPsd *)
{
    for (size_t i = 0; seg_type && i < n_seg; ++i)
        if (seg_type[i] == THIP_CONE_PSD) return fail(THIP_E_INVALID, M16_TEXT.no_psd, __FILE__, __LINE__);
    THIP_RC(thip_midbatch_fits(n, m, n_seg, seg_type, seg_len, nullptr, nullptr));
    return ob_segments(M16_TEXT, m, n_seg, seg_type, seg_len, cones, cls);
}

size_t m16_lds_for(size_t n, size_t m, int, const ObPsd &) { return MbMap((int)n, (int)m).bytes((int)m); }

bool m16_bf16(const OwnBatch *h) { return h->a_kind == THIP_A_BF16; }

int m16_launch(const OwnBatch *h, bool run, const ObArgs &a, unsigned count)
{
    void (*const k)(ObArgs) = m16_bf16(h) ? (run ? mid16batch_k<THIP_A_BF16> : mid16batch_init_k<THIP_A_BF16>)
                                          : (run ? mid16batch_k<THIP_A_F16> : mid16batch_init_k<THIP_A_F16>);
    return ob_launch(h, k, a, count);
}

int m16_start(const OwnBatch *h, const ObArgs &a, const ObStart &s, unsigned count)
{
    void (*const k)(M16StartArgs) = m16_bf16(h) ? mid16batch_start_k<THIP_A_BF16> : mid16batch_start_k<THIP_A_F16>;
    return ob_launch(h, k, M16StartArgs{ a, s }, count);
}

int m16_setbc(const OwnBatch *h, const ObArgs &a, const ObSetBc &s, unsigned count)
{
    void (*const k)(M16SetBcArgs) = m16_bf16(h) ? mid16batch_setbc_k<THIP_A_BF16> : mid16batch_setbc_k<THIP_A_F16>;
    return ob_launch(h, k, M16SetBcArgs{ a, s }, count);
}

int m16_seta(const OwnBatch *h, const ObArgs &a, const ObSetA &s, unsigned count)
{
    void (*const k)(M16SetAArgs) = m16_bf16(h) ? mid16batch_seta_k<THIP_A_BF16> : mid16batch_seta_k<THIP_A_F16>;
    return ob_launch(h, k, M16SetAArgs{ a, s.keep }, count);
}

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
    h->a_kind = kind == THIP_A_BF16 ? THIP_A_BF16 : THIP_A_F16;        // (thip_mid16batch_create: f16)
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

ObFamily M16_FAMILY = { M16_TEXT, { 256, 1024, 0 }, false, m16_check, mb_threads_for, m16_lds_for, mb_stride, m16_launch, m16_start,
                        m16_setbc, m16_seta,
                        { (const void *)mid16batch_k<THIP_A_BF16>, (const void *)mid16batch_init_k<THIP_A_BF16>,
                          (const void *)mid16batch_start_k<THIP_A_BF16>, (const void *)mid16batch_setbc_k<THIP_A_BF16>,
                          (const void *)mid16batch_seta_k<THIP_A_BF16>, (const void *)mid16batch_k<THIP_A_F16>,
                          (const void *)mid16batch_init_k<THIP_A_F16>, (const void *)mid16batch_start_k<THIP_A_F16>,
                          (const void *)mid16batch_setbc_k<THIP_A_F16>, (const void *)mid16batch_seta_k<THIP_A_F16>, nullptr, nullptr },
                        &M16_STORE };

int m16_kind(int a_kind)
{
    if (a_kind == THIP_A_F32)
        return fail(THIP_E_INVALID, "a mid16 batch stores A in 16 bits (THIP_A_BF16 or THIP_A_F16): f32 A is thip_midbatch's (MidBatchSolver)",
                    __FILE__, __LINE__);
    if (a_kind != THIP_A_BF16 && a_kind != THIP_A_F16)
        return fail(THIP_E_INVALID, "unknown stored form of A: a mid16 batch takes THIP_A_BF16 or THIP_A_F16", __FILE__, __LINE__);
    return 0;
}

}  // namespace

struct thip_mid16batch : OwnBatch {};

OB_DEFINE_API(mid16batch, M16_FAMILY, Mb16Info)

extern "C" {

int thip_mid16batch_create_kind(size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b, const float *dev_vecs_c,
                                const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                                const thip_param *par, int a_kind, thip_mid16batch **out)
{
    if (!out) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *out = nullptr;
    THIP_RC(m16_kind(a_kind));
    return ob_create(M16_FAMILY, n, m, n_prob, dev_mats_a, dev_vecs_b, dev_vecs_c, dev_vecs_b_rowabs, n_seg, host_seg_type, host_seg_len,
                     par, out, a_kind);
}

int thip_mid16batch_store_bytes(size_t n, size_t m, int a_kind, size_t *host_bytes)
{
    if (!host_bytes) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    THIP_RC(m16_kind(a_kind));
    *host_bytes = mb16_block_bytes(n, m, a_kind);
    return 0;
}

int thip_mid16batch_stored(thip_mid16batch *h, int i, uint16_t *host_words, float *host_inv_scale)
{
    THIP_NEED_INIT();
    THIP_RC(ob_member(M16_FAMILY, h, i));
    const unsigned char *const blk = reinterpret_cast<const unsigned char *>(m16_slot(h, (size_t)i));
    const size_t words = mb16_ld(h->m) * h->n;
    THIP_TRY(hipStreamSynchronize(ctx().stream));
    if (host_words) THIP_TRY(hipMemcpy(host_words, blk, words * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (host_inv_scale && h->a_kind == THIP_A_F16)
        THIP_TRY(hipMemcpy(host_inv_scale, blk + words * sizeof(uint16_t), h->n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

}
