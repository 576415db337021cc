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
// The rest of the iteration is the small batch's, on the same device functions (thip_ownbatch.h): sb_comp_add, the class bytes,
// one wave per block cone (sb_soc), block_sums, both endings of status_eval.
#include "thip_midstream.h"

#include <mutex>

using namespace thip;

namespace {

__global__ __launch_bounds__(1024) void midbatch_init_k(const MbArgs a) { mb_init_body(a); }

__global__ __launch_bounds__(1024) void midbatch_k(const MbArgs a) { mb_iterate_body(a, MbNoPsd()); }

size_t g_mb_bytes = 0;                      // device memory held by every thip_midbatch of the process

const ObText MB_TEXT = { "mid batch not initialised", "null mid batch", "a mid batch holds 1 .. 1048576 problems",
                         "a mid batch takes no PSD segment" };

// the shape rules (no device needed): the single source of the limit
int mb_check(size_t n, size_t m, size_t n_seg, const int32_t *seg_type, const int64_t *seg_len, std::vector<int> *cones,
             std::vector<unsigned char> *cls)
{
    if (m < 1 || m > MB_MAX_DIM || n < 1 || n > MB_MAX_DIM)
        return fail(THIP_E_INVALID, "a mid batch takes 1 <= m <= 4096 and 1 <= n <= 4096", __FILE__, __LINE__);
    THIP_RC(ob_segments(MB_TEXT, m, n_seg, seg_type, seg_len, cones, cls));
    if (MbMap((int)n, (int)m).bytes((int)m) > MB_LDS_MAX)
        return fail(THIP_E_INVALID, "the vectors of the problem (8 n + 13 m floats and 24 832 bytes) do not fit the LDS of one CU", __FILE__,
                    __LINE__);
    return 0;
}

}  // namespace

struct thip_midbatch : MbHandle {};

namespace {

int mb_attr()
{
    static std::once_flag once;
    static hipError_t err = hipSuccess;
    std::call_once(once, [&]() {
        err = hipFuncSetAttribute(reinterpret_cast<const void *>(&midbatch_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MB_LDS_MAX);
        if (err == hipSuccess)
            err = hipFuncSetAttribute(reinterpret_cast<const void *>(&midbatch_init_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)MB_LDS_MAX);
    });
    THIP_TRY(err);
    return 0;
}

void mb_plan(OwnBatch *h)
{
    h->threads = h->forced ? h->forced : mb_threads_for(h->n, h->m);
    h->lds = MbMap((int)h->n, (int)h->m).bytes((int)h->m);
}

int mb_launch_init(OwnBatch *h, int first, int count)
{
    MbArgs a = mb_args(h);
    a.first = first;
    hipLaunchKernelGGL(midbatch_init_k, dim3((unsigned)count), dim3((unsigned)h->threads), h->lds, ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

int mb_launch_run(OwnBatch *h, int count, int steps, const int *live)
{
    MbArgs a = mb_args(h);
    a.steps = steps;
    a.live = live;
    hipLaunchKernelGGL(midbatch_k, dim3((unsigned)count), dim3((unsigned)h->threads), h->lds, ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

}  // namespace

#define MB_NEED(h)                                                                  \
    do {                                                                            \
        if (!(h)) { THIP_NEED_INIT(); return fail(THIP_E_INVALID, MB_TEXT.uninit, __FILE__, __LINE__); } \
    } while (0)

extern "C" {

int thip_midbatch_fits(size_t n, size_t m, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                       size_t *host_lds_bytes, int *host_threads)
{
    THIP_RC(mb_check(n, m, n_seg, host_seg_type, host_seg_len, nullptr, nullptr));
    if (host_threads) *host_threads = mb_threads_for(n, m);
    if (host_lds_bytes) *host_lds_bytes = MbMap((int)n, (int)m).bytes((int)m);      // (the same for every workgroup size)
    return 0;
}

int thip_midbatch_destroy(thip_midbatch *h)
{
    if (!h) return 0;
    ob_destroy(h);
    delete h;
    return 0;
}

int thip_midbatch_create(size_t n, size_t m, size_t n_prob, const float *dev_mats_a, const float *dev_vecs_b, const float *dev_vecs_c,
                         const float *dev_vecs_b_rowabs, size_t n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len,
                         const thip_param *par, thip_midbatch **out)
{
    if (!out) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *out = nullptr;
    THIP_NEED_INIT();
    THIP_RC(ob_create_args(MB_TEXT, n_prob, dev_mats_a, dev_vecs_b, dev_vecs_c, dev_vecs_b_rowabs, par));
    thip_midbatch *h = new thip_midbatch();
    h->text = &MB_TEXT; h->total = &g_mb_bytes; h->launch_init = mb_launch_init; h->launch_run = mb_launch_run;
    // every refusal comes before the first allocation
    int rc = mb_check(n, m, n_seg, host_seg_type, host_seg_len, &h->cones, &h->cls);
    if (rc != 0) { delete h; return rc; }
    h->n = n; h->m = m; h->n_prob = n_prob;
    h->par = *par;
    h->stride = mb_stride(n, m);
    mb_plan(h);
    mb_note_alignment(h, dev_mats_a);
    rc = mb_attr();
    if (rc == 0) rc = ob_build(h, dev_mats_a, dev_vecs_b, dev_vecs_c, dev_vecs_b_rowabs);
    if (rc != 0) { thip_midbatch_destroy(h); return rc; }
    *out = h;
    return 0;
}

int thip_midbatch_set_param(thip_midbatch *h, const thip_param *par) { return ob_set_param(h, par); }

int thip_midbatch_init(thip_midbatch *h) { return ob_init(h, MB_TEXT); }

int thip_midbatch_run(thip_midbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{
    MB_NEED(h);
    return ob_run(h, max_steps, poll_every, host_status, false);
}

int thip_midbatch_run_until_any(thip_midbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{
    MB_NEED(h);
    return ob_run(h, max_steps, poll_every, host_status, true);
}

int thip_midbatch_status(thip_midbatch *h, int i, thip_status *host_status)
{
    MB_NEED(h);
    return ob_status(h, i, host_status);
}

int thip_midbatch_solution(thip_midbatch *h, int i, float *host_x, float *host_y)
{
    MB_NEED(h);
    return ob_solution(h, i, host_x, host_y);
}

int thip_midbatch_iterate(thip_midbatch *h, int i, float *host_x, float *host_y)
{
    MB_NEED(h);
    return ob_iterate(h, i, host_x, host_y);
}

int thip_midbatch_precond(thip_midbatch *h, int i, float *host_dp_tau, float *host_dp_sigma)
{
    MB_NEED(h);
    return ob_precond(h, i, host_dp_tau, host_dp_sigma);
}

int thip_midbatch_replace(thip_midbatch *h, int i, const float *dev_mat_a, const float *dev_vec_b, const float *dev_vec_c,
                          const float *dev_vec_b_rowabs)
{
    MB_NEED(h);
    THIP_RC(ob_replace(h, i, dev_mat_a, dev_vec_b, dev_vec_c, dev_vec_b_rowabs));
    mb_note_replaced(h, i, dev_mat_a);
    return 0;
}

int thip_midbatch_info(const thip_midbatch *h, thip_midbatch_info_t *host_info)
{
    if (!h || !host_info) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    memset(host_info, 0, sizeof(*host_info));
    mb_info(h, g_mb_bytes, *host_info);
    return 0;
}

int thip_test_midbatch_force_threads(thip_midbatch *h, int threads)
{
    if (!h) return fail(THIP_E_INVALID, "null mid batch", __FILE__, __LINE__);
    if (threads != 0 && threads != 256 && threads != 1024)
        return fail(THIP_E_INVALID, "the workgroup size is 256 or 1024 (0: by shape)", __FILE__, __LINE__);
    if (h->inited) return fail(THIP_E_INVALID, "thip_test_midbatch_force_threads comes before thip_midbatch_init", __FILE__, __LINE__);
    h->forced = threads;
    mb_plan(h);
    return 0;
}

}  // extern "C"
