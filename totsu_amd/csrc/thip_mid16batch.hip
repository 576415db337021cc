// thip_mid16batch.hip -- thip_mid16batch: the mid batch (thip_midbatch.hip: many MID-SIZE conic programs of one shape and cone layout,
// each with its OWN dense A, one workgroup per problem, every vector in LDS, A streamed twice per iteration) over a LIBRARY-OWNED
// 16-bit copy of every problem's A: half the bytes per pass, half the memory, one load path for every m.
//
// The stored form, its two rounding rules, the conversion of a range in one launch (mid16batch_convert_k) and the store's hooks
// (thip_ownbatch.h: ObStore) are thip_store16.h's, shared with the wide family over the same store (thip_wide16batch.hip); the pass
// over a block is thip_midstream.h's (mb16_pass_t).
//
// The contract: the batch is, bit for bit, a thip_midbatch that holds the WIDENED matrix W in f32 -- W(r, c) the bf16 word shifted
// left 16 bits, or float(h(r, c)) * inv_s[c] in f32 -- preconditioner, iterates, Kahan terms, carried pair, status blocks, at every
// workgroup size, in both state arithmetics, however the iterations are cut into launches: the pass deals the entries to the lanes and
// orders the additions as mb_pass_t does.  The problem solved is the one with the rounded matrix.
//
// This file: the five kernels (per stored form), the family's table and what the family adds to the C API; the rest of the API is
// thip_ownbatch.h's.
#include "thip_store16.h"

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
    return m16_stored(h, i, host_words, host_inv_scale);
}

}
