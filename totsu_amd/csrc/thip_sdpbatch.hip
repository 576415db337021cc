// thip_sdpbatch.hip -- thip_sdpbatch: many small SDPs (and mixed conic programs with PSD blocks), each with its OWN dense f32 A, one
// shape n, m and one cone layout.  The third own-A family: the mid batch's iteration unchanged (thip_midstream.h: one workgroup per
// problem, every vector in LDS, A streamed twice per iteration, the carried pair in the arena) with one more cone class in the
// block-cone phase between the two passes -- every PSD cone of order k <= 64 is projected by the workgroup itself, on x_y and then on
// x_s, so an iteration of a small SDP has no launch boundary inside it.
//
// The projection (sdp_project) is polar_small_k's (thip_eig_gemm.inc): Pi(M) = (M + M sign(M)) / 2 with sign(M) from the 45-product
// quintic polar chain on M / ||M||_F (11 lifting quintics, the first on 1.7 x; 3 minimax quintics; 1 Newton-Schulz step -- the same
// coefficients, so the same (0, 1.85] band), operands row-major in LDS at an odd pitch, __builtin_amdgcn_mfma_f32_32x32x2f32 with
// one 32 x 32 quadrant of the result per wave, a DIVISION by the norm per element (the exact zero matrix stays zero, a subnormal
// norm does not overflow), the packing of cone_psd.rs (off-diagonals carry sqrt 2 in the vector: the diagonal is multiplied by
// sqrt 2 on the way in and divided on the way out) and the symmetrised pack with rx <- rx - 2 x riding in it.  What differs:
//   * FOUR operands, not five: M is needed only by the last product M sign(M), and is unpacked again from the packed vector (which
//     is not written before the pack) into an operand that is dead by then;
//   * the operand extent follows the order: k <= 32 takes 32 x 33 operands and one wave, above that 64 x 65 and four;
//   * K is walked in chunks of 4 MFMA steps with a run-time count (ceil(k / 2) rounded up to 4, the padding is zero) instead of a
//     compile-time unroll of up to 32: a 1024-thread workgroup has 128 VGPRs per lane, and one instance serves every order.
// Cones are projected one after another, x_y then x_s, by waves 0 .. 3 (the simple form; the other waves of a 1024-thread workgroup
// wait at the barriers).
//
// LDS: the mid batch's map, and the operands.  During the cone phase the pass scratch hp, gp (6144 floats) is dead:
//   largest order <= 32: four 32 x 33 operands (4224 floats) lie in it -- the projection adds nothing;
//   largest order  > 32: one 64 x 65 operand (4160 floats) lies in it, three more follow the class bytes: 3 * 64 * 65 * 4 = 49 920 bytes.
// sp_check (thip_sdpcones.h, with the projection itself: the ragged batch of thip_raggedbatch.hip runs the same cones under the same
// rule) is the single source of the rule.  No atomics: a problem's iterates are a function of (its data, the workgroup size, the
// constants) alone.
//
// This file: the kernels and the family's table; the C API is thip_ownbatch.h's, instantiated by one line;
// thip_test_sdpbatch_project follows it.
#include "thip_sdpcones.h"

using namespace thip;

namespace {

struct SpArgs { ObArgs mb; int tail; };

__global__ __launch_bounds__(1024) void sdpbatch_init_k(const ObArgs a) { mb_init_body(a); }

__global__ __launch_bounds__(1024) void sdpbatch_k(const SpArgs a) { mb_iterate_body(a.mb, SpCones{ a.tail }); }

// a problem starts from a given iterate (thip_sdpbatch_set_iterates): no cone is projected, the launch keeps the family's LDS size
struct SpStartArgs { ObArgs mb; ObStart s; };

__global__ __launch_bounds__(1024) void sdpbatch_start_k(const SpStartArgs a) { mb_start_body(a.mb, ob_staged(a.s)); }

// a problem takes a new (b, c) and keeps its A (thip_sdpbatch_set_bc): no cone is projected, the launch keeps the family's LDS size
struct SpSetBcArgs { ObArgs mb; ObSetBc s; };

__global__ __launch_bounds__(1024) void sdpbatch_setbc_k(const SpSetBcArgs a) { mb_setbc_body(a.mb, a.s); }

// a problem's A has new values (thip_sdpbatch_set_a): no cone is projected, the launch keeps the family's LDS size
struct SpSetAArgs { ObArgs mb; int keep; };

__global__ __launch_bounds__(1024) void sdpbatch_seta_k(const SpSetAArgs a) { mb_seta_body(a.mb, a.keep); }

// thip_test_sdpbatch_project: the projection alone, one workgroup per packed matrix.  LDS: [shd 64][operands]
__global__ __launch_bounds__(256) void sdpbatch_project_k(int k, float *packed, float *rx)
{
    const size_t len = (size_t)k * (size_t)(k + 1) / 2;
    float *S = mb_lds;
    sp_project_any(packed + blockIdx.x * len, rx != nullptr ? rx + blockIdx.x * len : nullptr, k, S + 64, S + 64 + SP_OP64,
                   reinterpret_cast<double *>(S));
}

// thip_test_sdpbatch_project_form: the projection in the forms the batches run it in, from a kernel built for 1024-thread workgroups
// as the iteration kernels are.  LDS false: x (and rx) where they lie in device memory (SpCones::placed); true: copied behind the
// operands and projected there (SpCones::operator()), the result copied back.  LDS: [shd 64][operands][x][rx]
template <bool LDS>
__global__ __launch_bounds__(1024) void sdpbatch_project_form_k(int k, float *packed, float *rx)
{
    const int len = k * (k + 1) / 2, ops = 64 + (k <= 32 ? 4 * SP_OP32 : 4 * SP_OP64);
    float *S = mb_lds, *x = packed + (size_t)blockIdx.x * len, *r = rx != nullptr ? rx + (size_t)blockIdx.x * len : nullptr;
    if (!LDS) {
        sp_project_any(x, r, k, S + 64, S + 64 + SP_OP64, reinterpret_cast<double *>(S));
        return;
    }
    float *xl = S + ops, *rl = r != nullptr ? xl + len : nullptr;
    for (int e = (int)threadIdx.x; e < len; e += (int)blockDim.x) {
        xl[e] = x[e];
        if (r != nullptr) rl[e] = r[e];
    }
    __syncthreads();
    sp_project_any(xl, rl, k, S + 64, S + 64 + SP_OP64, reinterpret_cast<double *>(S));
    for (int e = (int)threadIdx.x; e < len; e += (int)blockDim.x) {
        x[e] = xl[e];
        if (r != nullptr) r[e] = rl[e];
    }
}

int sp_launch(const OwnBatch *h, bool run, const ObArgs &a, unsigned count)
{
    if (!run) return ob_launch(h, sdpbatch_init_k, a, count);
    return ob_launch(h, sdpbatch_k, SpArgs{ a, (int)(MbMap((int)h->n, (int)h->m).bytes((int)h->m) / sizeof(float)) }, count);
}

int sp_start(const OwnBatch *h, const ObArgs &a, const ObStart &s, unsigned count)
{
    return ob_launch(h, sdpbatch_start_k, SpStartArgs{ a, s }, count);
}

int sp_setbc(const OwnBatch *h, const ObArgs &a, const ObSetBc &s, unsigned count)
{
    return ob_launch(h, sdpbatch_setbc_k, SpSetBcArgs{ a, s }, count);
}

int sp_seta(const OwnBatch *h, const ObArgs &a, const ObSetA &s, unsigned count)
{
    return ob_launch(h, sdpbatch_seta_k, SpSetAArgs{ a, s.keep }, count);
}

// (the third entry of the table's kernels and the last two are this family's: the projection probes ask for the large LDS too)
ObFamily SP_FAMILY = { SP_TEXT, { 256, 1024, 0 }, true, sp_check, mb_threads_for, sp_lds_for, mb_stride, sp_launch, sp_start, sp_setbc,
                       sp_seta,
                       { (const void *)sdpbatch_k, (const void *)sdpbatch_init_k, (const void *)sdpbatch_project_k,
                         (const void *)sdpbatch_start_k, (const void *)sdpbatch_setbc_k, (const void *)sdpbatch_seta_k,
                         (const void *)sdpbatch_project_form_k<false>, (const void *)sdpbatch_project_form_k<true> } };

// thip_midbatch_info_t's fields, and the PSD cones'
struct SpInfo {
    void operator()(const OwnBatch *h, thip_sdpbatch_info_t &o) const
    {
        MbInfo()(h, o);
        o.max_psd_order = h->psd.max_k; o.n_psd = h->psd.n_psd;
        o.psd_lds_bytes = h->psd.tail_bytes;
    }
};

}  // namespace

struct thip_sdpbatch : OwnBatch {};

OB_DEFINE_API(sdpbatch, SP_FAMILY, SpInfo)

extern "C" {

int thip_test_sdpbatch_project(int k, int count, float *dev_packed, float *dev_rx_or_null)
{
    THIP_NEED_INIT();
    if (k < 1 || k > SP_MAX_ORDER) return fail(THIP_E_INVALID, "thip_test_sdpbatch_project: 1 <= k <= 64", __FILE__, __LINE__);
    if (count < 1 || !dev_packed) return fail(THIP_E_INVALID, "thip_test_sdpbatch_project: no matrix", __FILE__, __LINE__);
    THIP_RC(ob_attr(SP_FAMILY));
    const size_t lds = (64 + (k <= 32 ? 4 * (size_t)SP_OP32 : 4 * (size_t)SP_OP64)) * sizeof(float);
    hipLaunchKernelGGL(sdpbatch_project_k, dim3((unsigned)count), dim3(256), lds, ctx().stream, k, dev_packed, dev_rx_or_null);
    THIP_LAUNCH_CHECK();
    return 0;
}

int thip_test_sdpbatch_project_form(int k, int count, int threads, int in_lds, float *dev_packed, float *dev_rx_or_null)
{
    THIP_NEED_INIT();
    if (k < 1 || k > SP_MAX_ORDER) return fail(THIP_E_INVALID, "thip_test_sdpbatch_project_form: 1 <= k <= 64", __FILE__, __LINE__);
    if (count < 1 || !dev_packed) return fail(THIP_E_INVALID, "thip_test_sdpbatch_project_form: no matrix", __FILE__, __LINE__);
    if (threads != 256 && threads != 1024)
        return fail(THIP_E_INVALID, "thip_test_sdpbatch_project_form: the workgroup size is 256 or 1024", __FILE__, __LINE__);
    if (in_lds != 0 && in_lds != 1) return fail(THIP_E_INVALID, "thip_test_sdpbatch_project_form: in_lds is 0 or 1", __FILE__, __LINE__);
    THIP_RC(ob_attr(SP_FAMILY));
    const size_t len = (size_t)k * (size_t)(k + 1) / 2;
    const size_t lds = (64 + (k <= 32 ? 4 * (size_t)SP_OP32 : 4 * (size_t)SP_OP64) + (in_lds ? 2 * len : 0)) * sizeof(float);
    if (in_lds)
        hipLaunchKernelGGL(sdpbatch_project_form_k<true>, dim3((unsigned)count), dim3((unsigned)threads), lds, ctx().stream, k,
                           dev_packed, dev_rx_or_null);
    else
        hipLaunchKernelGGL(sdpbatch_project_form_k<false>, dim3((unsigned)count), dim3((unsigned)threads), lds, ctx().stream, k,
                           dev_packed, dev_rx_or_null);
    THIP_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
