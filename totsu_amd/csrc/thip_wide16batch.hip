// thip_wide16batch.hip -- thip_wide16batch: the wide batch (thip_widebatch.hip: many conic programs of one shape and cone layout, each
// with its OWN dense A, of EVERY shape up to 4096 x 4096 and every PSD order up to 64, one workgroup per problem, all but the pass
// vectors left in the problem's block of the arena) over a LIBRARY-OWNED 16-bit copy of every problem's A (thip_store16.h: the mid16
// batch's store, word for word): half the bytes per pass and half the memory on exactly the shapes where A is all that counts.  The
// ninth own-A family, and a composition of the three seams of thip_midstream.h's bodies, nothing else: the matrix policy
// MbDenseA16<KIND>, the cone hook SpCones, the vector placement WbInArena.
//
// The contract: the batch is, bit for bit, a thip_widebatch that holds the WIDENED matrix W in f32 -- W(r, c) the bf16 word shifted
// left 16 bits, or float(h(r, c)) * inv_s[c] in f32 -- the whole arena block (6 n + 11 m floats), the status blocks, the
// preconditioner, at both workgroup sizes, in both state arithmetics, however the iterations are cut into launches: mb16_pass_t deals
// the entries to the lanes and orders the additions as mb_pass_t does, and everything outside the pass is the wide batch's text.  On
// a layout without PSD cones that the mid batch takes, the first 6 n + 10 m floats of a block are a thip_mid16batch's.
//
// The memory paths: the pass reads A and inv_s through __restrict__ and address-space casts (mb16_pass_t) and nothing else; its
// vector arguments are the ones WbMap keeps in LDS.  No vector that lies in the arena is read through __restrict__, a scalar or a
// non-temporal path (thip_wideplace.h).
//
// This file: the five kernels (per stored form), the family's table and what the family adds to the C API; the rest of the API is
// thip_ownbatch.h's.
#include "thip_wideplace.h"
#include "thip_store16.h"

using namespace thip;

namespace {

template <int KIND>
__global__ __launch_bounds__(1024) void wide16batch_init_k(const ObArgs a) { mb_init_body(a, ObUniform(), MbDenseA16<KIND>(), WbInArena()); }

struct W16Args { ObArgs mb; int tail; };

template <int KIND>
__global__ __launch_bounds__(1024) void wide16batch_k(const W16Args a)
{
    mb_iterate_body(a.mb, SpCones{ a.tail }, ObUniform(), MbDenseA16<KIND>(), WbInArena());
}

struct W16StartArgs { ObArgs mb; ObStart s; };

template <int KIND>
__global__ __launch_bounds__(1024) void wide16batch_start_k(const W16StartArgs a)
{
    mb_start_body(a.mb, ob_staged(a.s), ObUniform(), MbDenseA16<KIND>(), WbInArena());
}

struct W16SetBcArgs { ObArgs mb; ObSetBc s; };

template <int KIND>
__global__ __launch_bounds__(1024) void wide16batch_setbc_k(const W16SetBcArgs a)
{
    mb_setbc_body(a.mb, a.s, ObUniform(), MbDenseA16<KIND>(), WbInArena());
}

struct W16SetAArgs { ObArgs mb; int keep; };

template <int KIND>
__global__ __launch_bounds__(1024) void wide16batch_seta_k(const W16SetAArgs a)
{
    mb_seta_body(a.mb, a.keep, ObUniform(), MbDenseA16<KIND>(), WbInArena());
}

const ObText W16_TEXT = { "wide16 batch not initialised", "null wide16 batch", "a wide16 batch holds 1 .. 1048576 problems", nullptr,
                          "the workgroup size is 256 or 1024 (0: by shape)",
                          "thip_test_wide16batch_force_threads comes before thip_wide16batch_init" };

// the init-time kernels ask for the larger of the two maps (wb_lds_init), the iteration and the start for the iteration's
int w16_launch(const OwnBatch *h, bool run, const ObArgs &a, unsigned count)
{
    if (!run) return wb_launch_lds(h, m16_bf16(h) ? wide16batch_init_k<THIP_A_BF16> : wide16batch_init_k<THIP_A_F16>, a, count, wb_lds_init(h));
    return ob_launch(h, m16_bf16(h) ? wide16batch_k<THIP_A_BF16> : wide16batch_k<THIP_A_F16>, W16Args{ a, wb_tail(h) }, count);
}

int w16_start(const OwnBatch *h, const ObArgs &a, const ObStart &s, unsigned count)
{
    return ob_launch(h, m16_bf16(h) ? wide16batch_start_k<THIP_A_BF16> : wide16batch_start_k<THIP_A_F16>, W16StartArgs{ a, s }, count);
}

int w16_setbc(const OwnBatch *h, const ObArgs &a, const ObSetBc &s, unsigned count)
{
    return wb_launch_lds(h, m16_bf16(h) ? wide16batch_setbc_k<THIP_A_BF16> : wide16batch_setbc_k<THIP_A_F16>, W16SetBcArgs{ a, s }, count,
                         wb_lds_init(h));
}

int w16_seta(const OwnBatch *h, const ObArgs &a, const ObSetA &s, unsigned count)
{
    return wb_launch_lds(h, m16_bf16(h) ? wide16batch_seta_k<THIP_A_BF16> : wide16batch_seta_k<THIP_A_F16>, W16SetAArgs{ a, s.keep }, count,
                         wb_lds_init(h));
}

// streams = false: the store is aligned and there is one load path.  The rule, the LDS and the stride are the wide batch's
ObFamily W16_FAMILY = { W16_TEXT, { 256, 1024, 0 }, false, wb_check, mb_threads_for, wb_lds_for, wb_stride, w16_launch, w16_start,
                        w16_setbc, w16_seta,
                        { (const void *)wide16batch_k<THIP_A_BF16>, (const void *)wide16batch_init_k<THIP_A_BF16>,
                          (const void *)wide16batch_start_k<THIP_A_BF16>, (const void *)wide16batch_setbc_k<THIP_A_BF16>,
                          (const void *)wide16batch_seta_k<THIP_A_BF16>, (const void *)wide16batch_k<THIP_A_F16>,
                          (const void *)wide16batch_init_k<THIP_A_F16>, (const void *)wide16batch_start_k<THIP_A_F16>,
                          (const void *)wide16batch_setbc_k<THIP_A_F16>, (const void *)wide16batch_seta_k<THIP_A_F16>, nullptr, nullptr },
                        &M16_STORE };

int w16_kind(int a_kind)
{
    if (a_kind == THIP_A_F32)
        return fail(THIP_E_INVALID, "a wide16 batch stores A in 16 bits (THIP_A_BF16 or THIP_A_F16): f32 A is thip_widebatch's (WideBatchSolver)",
                    __FILE__, __LINE__);
    if (a_kind != THIP_A_BF16 && a_kind != THIP_A_F16)
        return fail(THIP_E_INVALID, "unknown stored form of A: a wide16 batch takes THIP_A_BF16 or THIP_A_F16", __FILE__, __LINE__);
    return 0;
}

// the wide batch's fields and the 16-bit store's
struct W16Info {
    void operator()(const OwnBatch *h, thip_wide16batch_info_t &o) const
    {
        Mb16Info()(h, o);
        wb_info_fill(h, o);
    }
};

}  // namespace

struct thip_wide16batch : OwnBatch {};

OB_DEFINE_API(wide16batch, W16_FAMILY, W16Info)

extern "C" {

int thip_wide16batch_create_kind(size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b, const float *dev_vecs_c,
                                 const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                                 const thip_param *par, int a_kind, thip_wide16batch **out)
{
    if (!out) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *out = nullptr;
    THIP_RC(w16_kind(a_kind));
    return ob_create(W16_FAMILY, n, m, n_prob, dev_mats_a, dev_vecs_b, dev_vecs_c, dev_vecs_b_rowabs, n_seg, host_seg_type, host_seg_len,
                     par, out, a_kind);
}

int thip_wide16batch_store_bytes(size_t n, size_t m, int a_kind, size_t *host_bytes)
{
    if (!host_bytes) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    THIP_RC(w16_kind(a_kind));
    *host_bytes = mb16_block_bytes(n, m, a_kind);
    return 0;
}

int thip_wide16batch_stored(thip_wide16batch *h, int i, uint16_t *host_words, float *host_inv_scale)
{
    THIP_NEED_INIT();
    THIP_RC(ob_member(W16_FAMILY, h, i));
    return m16_stored(h, i, host_words, host_inv_scale);
}

}
