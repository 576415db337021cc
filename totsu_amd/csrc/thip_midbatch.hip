// thip_midbatch.hip -- thip_midbatch: many MID-SIZE conic programs, each with its OWN dense f32 A (shared n, m and cone layout), too big
// for the LDS of a CU (thip_smallbatch.hip) and far too small for the big-A schedules to be anything but launch-bound.  A launch of
// midbatch_k gives one workgroup to each live problem: every vector of the iteration lives in LDS, A is STREAMED from the caller's
// array (column-major, lda = m, never copied, never written), `steps` whole iterations per launch with no launch boundary inside.
//
// Recurrence: the carried one -- two passes over A per iteration.  Pass 1 forms h = A u, g = A^T v for the x-update
// and the cones; pass 2 forms h = A x_x, g = A^T x_y of the NEW iterate, which serves the criteria and, through
// A rx_x = A x_k - 2 A x_{k+1} (likewise A^T rx_y, c.rx_x, b.rx_y), the y-update.  The pair (A x_k, A^T x_y,k) is carried in the
// arena behind the preconditioner, so a launch boundary changes nothing (tested bitwise).
//
// The LDS map, the pass over A (mb_pass) and the bodies of both kernels are thip_midstream.h's, shared with the SDP batch
// (thip_sdpbatch.hip), which adds PSD cones to the block-cone phase; this family takes none.  mb_check is the single source of the limit.
//
// The rest of the iteration is the small batch's, on the same device functions (thip_step.h, thip_ownbatch.h): the class bytes,
// one wave per block cone (sb_soc), block_sums, both endings of status_eval.
//
// This file: the two kernels, the shape rule and the family's table; the C API is thip_ownbatch.h's, instantiated by the last line.
#include "thip_midstream.h"

using namespace thip;

namespace {

__global__ __launch_bounds__(1024) void midbatch_init_k(const ObArgs a) { mb_init_body(a); }

__global__ __launch_bounds__(1024) void midbatch_k(const ObArgs a) { mb_iterate_body(a, MbNoPsd()); }

// a problem starts from a given iterate (thip_midbatch_set_iterates): its own argument block, the iteration's by value
struct MbStartArgs { ObArgs mb; ObStart s; };

__global__ __launch_bounds__(1024) void midbatch_start_k(const MbStartArgs a) { mb_start_body(a.mb, ob_staged(a.s)); }

// a problem takes a new (b, c) and keeps its A (thip_midbatch_set_bc)
struct MbSetBcArgs { ObArgs mb; ObSetBc s; };

__global__ __launch_bounds__(1024) void midbatch_setbc_k(const MbSetBcArgs a) { mb_setbc_body(a.mb, a.s); }

// a problem's A has new values (thip_midbatch_set_a)
struct MbSetAArgs { ObArgs mb; int keep; };

__global__ __launch_bounds__(1024) void midbatch_seta_k(const MbSetAArgs a) { mb_seta_body(a.mb, a.keep); }

const ObText MB_TEXT = { "mid batch not initialised", "null mid batch", "a mid batch holds 1 .. 1048576 problems",
                         "a mid batch takes no PSD segment", "the workgroup size is 256 or 1024 (0: by shape)",
                         "thip_test_midbatch_force_threads comes before thip_midbatch_init" };

// the shape rules (no device needed): the single source of the limit
int mb_check(size_t n, size_t m, size_t n_seg, const int32_t *seg_type, const int64_t *seg_len, std::vector<int> *cones,
             std::vector<unsigned char> *cls, ObPsd *)
{
    if (m < 1 || m > MB_MAX_DIM || n < 1 || n > MB_MAX_DIM)
        return fail(THIP_E_INVALID, "a mid batch takes 1 <= m <= 4096 and 1 <= n <= 4096", __FILE__, __LINE__);
    THIP_RC(ob_segments(MB_TEXT, m, n_seg, seg_type, seg_len, cones, cls));
    if (MbMap((int)n, (int)m).bytes((int)m) > OB_LDS_MAX)
        return fail(THIP_E_INVALID, "the vectors of the problem (8 n + 13 m floats and 24 832 bytes) do not fit the LDS of one CU", __FILE__,
                    __LINE__);
    return 0;
}

// (the same for every workgroup size)
size_t mb_lds_for(size_t n, size_t m, int, const ObPsd &) { return MbMap((int)n, (int)m).bytes((int)m); }

int mb_launch(const OwnBatch *h, bool run, const ObArgs &a, unsigned count)
{
    return ob_launch(h, run ? midbatch_k : midbatch_init_k, a, count);
}

int mb_start(const OwnBatch *h, const ObArgs &a, const ObStart &s, unsigned count)
{
    return ob_launch(h, midbatch_start_k, MbStartArgs{ a, s }, count);
}

int mb_setbc(const OwnBatch *h, const ObArgs &a, const ObSetBc &s, unsigned count)
{
    return ob_launch(h, midbatch_setbc_k, MbSetBcArgs{ a, s }, count);
}

int mb_seta(const OwnBatch *h, const ObArgs &a, const ObSetA &s, unsigned count)
{
    return ob_launch(h, midbatch_seta_k, MbSetAArgs{ a, s.keep }, count);
}

ObFamily MB_FAMILY = { MB_TEXT, { 256, 1024, 0 }, true, mb_check, mb_threads_for, mb_lds_for, mb_stride, mb_launch, mb_start, mb_setbc,
                       mb_seta,
                       { (const void *)midbatch_k, (const void *)midbatch_init_k, (const void *)midbatch_start_k,
                         (const void *)midbatch_setbc_k, (const void *)midbatch_seta_k, nullptr } };

}  // namespace

struct thip_midbatch : OwnBatch {};

OB_DEFINE_API(midbatch, MB_FAMILY, MbInfo)
