// thip_raggedbatch.hip -- thip_raggedbatch: many conic programs, each with its OWN dense f32 A, its OWN shape n_p, m_p and its OWN cone
// layout, in one batch.  The fourth own-A family: the SDP batch's iteration unchanged (thip_midstream.h's bodies with SpCones of
// thip_sdpcones.h: one workgroup per running problem, every vector in LDS, A streamed twice per iteration, the PSD cones projected on
// chip), on a problem the workgroup looks up instead of being launched with.
//
// What was uniform in the three other families lives in their launch arguments (ObShape, one cls, one cones, arena + p * stride).
// Here workgroup k finds its problem p as they do (the live list, or first + k), reads p's descriptor (RbDesc: n, m, n_cones, where
// its cone triples and class bytes start in the concatenated tables, where its state starts in the arena) with uniform loads, builds
// the ObArgs of that problem BY VALUE and runs the shared bodies on it through their seam (thip_ownbatch.h: ObUniform / RbAt -- which
// problem, where its arena block is, how long its carried tail).  The LDS map is MbMap(n_p, m_p), the PSD operand tail starts at that
// map's end, the 16-byte or 4-byte load path is chosen by mb_vec on the problem's own pointer.  So a problem's iterates are, bit for
// bit, those of a mid batch / SDP batch that holds it alone at the same workgroup size (tests/test_gpu_raggedbatch.py).
//
// A launch has one workgroup size and one dynamic LDS size: the handle splits its problems by mb_threads_for(n_p, m_p) into a
// 256-thread and a 1024-thread class (a forced size puts every problem in one), each with the largest sp_lds_for of its members,
// and every poll makes one launch per class that has a running problem.  A class's live list is ordered by descending m_p n_p, ties
// by index: the longest workgroups start first.  No result depends on that order, on the class or on the cuts.  Problems take
// mb_stride(n_p, m_p) floats of the arena each, packed; identical layouts (m, seg_type, seg_len) share one entry of the tables.
// rb_plan is the single source of all of this and needs no device; a problem is taken exactly when sp_check takes it.
//
// This file: the two kernels, the plan, the handle and the C API (RbAt and the launches by class -- init, run -- are
// thip_raggedhost.h's, one text with thip_raggedsparse.hip).  The API bodies are thip_ownbatch.h's where a handle of one shape
// and a handle of many do the same thing (poll, status, replace, set_param, destroy; solution / iterate / precond through their
// _at forms with the problem's own n, m and block); create and info are this family's own.
#include "thip_raggedhost.h"

#include <map>
#include <tuple>

using namespace thip;

namespace {

// what a workgroup reads about its problem (one 32-byte uniform load)
struct RbDesc {
    int n, m, n_cones;
    int cones_at;                           // where its (beg, end, kind) triples start in the cone table, in ints
    int cls_at, pad;                        // where its class bytes start in the class table
    long long arena_at;                     // where its mb_stride(n, m) floats of state start in the arena
};
static_assert(sizeof(RbDesc) == 32, "RbDesc is copied as an array");

// mb: the words every problem shares (cls, cones and arena are the tables' and the arena's bases; n, m, n_cones, stride unused)
struct RbArgs { ObArgs mb; const RbDesc *desc; };

// the launch arguments a uniform batch of this workgroup's problem alone would have had
__device__ __forceinline__ ObArgs rb_problem(const RbArgs &a, RbAt &at)
{
    const int p = ob_problem(a.mb.live, a.mb.first);
    const RbDesc d = a.desc[p];
    ObArgs b = a.mb;
    b.n = d.n; b.m = d.m; b.n_cones = d.n_cones;
    b.cones = a.mb.cones + d.cones_at;
    b.cls = a.mb.cls + d.cls_at;
    at.p = p; at.ar = a.mb.arena + d.arena_at;
    return b;
}

__global__ __launch_bounds__(1024) void raggedbatch_init_k(const RbArgs a)
{
    RbAt at;
    const ObArgs b = rb_problem(a, at);
    mb_init_body(b, at);
}

__global__ __launch_bounds__(1024) void raggedbatch_k(const RbArgs a)
{
    RbAt at;
    const ObArgs b = rb_problem(a, at);
    mb_iterate_body(b, SpCones{ (int)(MbMap(b.n, b.m).bytes(b.m) / sizeof(float)) }, at);
}

// a problem starts from a given iterate (thip_raggedbatch_set_iterates): one launch per class, the problems by list
struct RbStartArgs { RbArgs rb; ObStart s; };

__global__ __launch_bounds__(1024) void raggedbatch_start_k(const RbStartArgs a)
{
    RbAt at;
    const ObArgs b = rb_problem(a.rb, at);
    mb_start_body(b, ob_staged(a.s), at);
}

// a problem takes a new (b, c) and keeps its A (thip_raggedbatch_set_bc): one launch per class, the problems by list
struct RbSetBcArgs { RbArgs rb; ObSetBc s; };

__global__ __launch_bounds__(1024) void raggedbatch_setbc_k(const RbSetBcArgs a)
{
    RbAt at;
    const ObArgs b = rb_problem(a.rb, at);
    mb_setbc_body(b, a.s, at);
}

// a problem's A has new values (thip_raggedbatch_set_a): one launch per class, the problems by list
struct RbSetAArgs { RbArgs rb; int keep; };

__global__ __launch_bounds__(1024) void raggedbatch_seta_k(const RbSetAArgs a)
{
    RbAt at;
    const ObArgs b = rb_problem(a.rb, at);
    mb_seta_body(b, a.keep, at);
}

// ---- the host side ------------------------------------------------------------------------------------------------------------

const ObText RB_TEXT = { "ragged batch not initialised", "null ragged batch", "a ragged batch holds 1 .. 1048576 problems", nullptr,
                         "the workgroup size is 256 or 1024 (0: by shape)",
                         "thip_test_raggedbatch_force_threads comes before thip_raggedbatch_init" };

int rb_launch_hook(const OwnBatch *h, bool run, const ObArgs &a, unsigned count);

// the shape rule is the SDP batch's (sp_check); the launch hook serves ob_replace: the init kernel on one slot
ObFamily RB_FAMILY = { RB_TEXT, { 256, 1024, 0 }, true, sp_check, mb_threads_for, sp_lds_for, mb_stride, rb_launch_hook, nullptr,
                       nullptr, nullptr,
                       { (const void *)raggedbatch_k, (const void *)raggedbatch_init_k, (const void *)raggedbatch_start_k,
                         (const void *)raggedbatch_setbc_k, (const void *)raggedbatch_seta_k, nullptr } };

struct RbProb { size_t n, m, lds; int layout, cls; };

// everything create decides before it allocates (no device needed)
struct RbPlan {
    std::vector<RbProb> prob;
    std::vector<RbDesc> desc;
    std::vector<int> cones;                 // the layouts' triples, one layout after another
    std::vector<unsigned char> cls;         // the layouts' class bytes
    int n_layouts = 0;
    size_t arena_floats = 0, a_bytes = 0;
    // the classes: 0 of 256 threads, 1 of 1024.  members: in the order of the class's live list
    std::vector<int> members[2];
    size_t lds[2] = { 0, 0 };
};

// the class split and the order within a class; forced: 0, 256 or 1024
void rb_classes(RbPlan &pl, int forced)
{
    for (int c = 0; c < 2; ++c) { pl.members[c].clear(); pl.lds[c] = 0; }
    for (size_t p = 0; p < pl.prob.size(); ++p) {
        RbProb &q = pl.prob[p];
        q.cls = (forced ? forced : mb_threads_for(q.n, q.m)) == RB_THREADS[1];
        pl.members[q.cls].push_back((int)p);
        pl.lds[q.cls] = std::max(pl.lds[q.cls], q.lds);
    }
    for (int c = 0; c < 2; ++c)             // descending m n, ties by index (the members are in index order: a stable sort keeps it)
        std::stable_sort(pl.members[c].begin(), pl.members[c].end(), [&](int x, int y) {
            return pl.prob[(size_t)x].m * pl.prob[(size_t)x].n > pl.prob[(size_t)y].m * pl.prob[(size_t)y].n;
        });
}

int rb_plan(size_t n_prob, const size_t *host_n, const size_t *host_m, const size_t *host_n_seg, const int32_t *seg_type,
            const int64_t *seg_len, int forced, RbPlan &pl, int *first_refused, size_t *host_lds_bytes, int *host_threads)
{
    if (first_refused) *first_refused = -1;
    if (n_prob < 1 || n_prob > OB_MAX_PROB) return fail(THIP_E_INVALID, RB_TEXT.count, __FILE__, __LINE__);
    if (!host_n || !host_m || !host_n_seg) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (forced != 0 && forced != RB_THREADS[0] && forced != RB_THREADS[1]) return fail(THIP_E_INVALID, RB_TEXT.force_sizes, __FILE__, __LINE__);
    std::map<std::tuple<size_t, std::vector<int32_t>, std::vector<int64_t>>, int> seen;
    std::vector<int> lay_cones_at, lay_cls_at, lay_n_cones;
    pl.prob.resize(n_prob);
    pl.desc.resize(n_prob);
    size_t seg0 = 0;
    for (size_t p = 0; p < n_prob; ++p) {
        const size_t n = host_n[p], m = host_m[p], ns = host_n_seg[p];
        const int32_t *st = ns ? seg_type + seg0 : nullptr;
        const int64_t *sl = ns ? seg_len + seg0 : nullptr;
        if (ns && (!seg_type || !seg_len)) return rb_refuse(p, fail(THIP_E_INVALID, "null cone segments", __FILE__, __LINE__), first_refused);
        std::vector<int> cones;
        std::vector<unsigned char> cls;
        size_t lds = 0;
        int thr = 0;
        const int rc = ob_fits(RB_FAMILY, n, m, ns, st, sl, &lds, &thr, &cones, &cls);
        if (rc != 0) return rb_refuse(p, rc, first_refused);
        if (host_lds_bytes) host_lds_bytes[p] = lds;
        if (host_threads) host_threads[p] = thr;
        auto key = std::make_tuple(m, std::vector<int32_t>(st, st + ns), std::vector<int64_t>(sl, sl + ns));
        auto it = seen.find(key);
        if (it == seen.end()) {
            if (pl.cones.size() + cones.size() > (size_t)1 << 30 || pl.cls.size() + cls.size() > (size_t)1 << 30)
                return rb_refuse(p, fail(THIP_E_INVALID, "the distinct cone layouts of a ragged batch hold at most 2^30 rows", __FILE__, __LINE__),
                                 first_refused);
            it = seen.emplace(std::move(key), (int)lay_cls_at.size()).first;
            lay_cones_at.push_back((int)pl.cones.size());
            lay_cls_at.push_back((int)pl.cls.size());
            lay_n_cones.push_back((int)(cones.size() / 3));
            pl.cones.insert(pl.cones.end(), cones.begin(), cones.end());
            pl.cls.insert(pl.cls.end(), cls.begin(), cls.end());
        }
        const int lay = it->second;
        pl.prob[p] = RbProb{ n, m, lds, lay, 0 };
        RbDesc &d = pl.desc[p];
        d.n = (int)n; d.m = (int)m; d.n_cones = lay_n_cones[(size_t)lay];
        d.cones_at = lay_cones_at[(size_t)lay]; d.cls_at = lay_cls_at[(size_t)lay]; d.pad = 0;
        d.arena_at = (long long)pl.arena_floats;
        pl.arena_floats += mb_stride(n, m);
        pl.a_bytes += 2 * m * n * sizeof(float);
        seg0 += ns;
    }
    pl.n_layouts = (int)lay_cls_at.size();
    rb_classes(pl, forced);
    return 0;
}

}  // namespace

struct thip_raggedbatch : OwnBatch {
    RbPlan pl;
    RbDesc *desc_dev = nullptr;
    std::vector<int> cl_live[2];            // the classes' live lists as of the last launch
    int64_t cl_launches[2] = { 0, 0 }, cl_workgroups[2] = { 0, 0 };
};

namespace {

RbArgs rb_args(const thip_raggedbatch *h)
{
    RbArgs a{ ob_args(h), h->desc_dev };
    a.mb.n = a.mb.m = a.mb.n_cones = 0;
    a.mb.stride = 0;
    return a;
}

// class c's kernel -- the init kernel or `steps` iterations -- on `count` problems: those of the list, or (live == NULL) first ..
int rg_launch(const thip_raggedbatch *h, bool run, int c, unsigned count, int steps, const int *live, int first)
{
    RbArgs a = rb_args(h);
    a.mb.steps = steps; a.mb.live = live; a.mb.first = first;
    hipLaunchKernelGGL(run ? raggedbatch_k : raggedbatch_init_k, dim3(count), dim3((unsigned)RB_THREADS[c]), h->pl.lds[c], ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

// class c's start kernel on the `count` problems of the list, workgroup k's iterate at s.at[k]
int rg_start(const thip_raggedbatch *h, int c, unsigned count, const int *live, const ObStart &s)
{
    RbStartArgs a{ rb_args(h), s };
    a.rb.mb.live = live;
    hipLaunchKernelGGL(raggedbatch_start_k, dim3(count), dim3((unsigned)RB_THREADS[c]), h->pl.lds[c], ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

// class c's set_bc kernel on the `count` problems of the list, workgroup k's data at s.s.at[k]
int rg_setbc(const thip_raggedbatch *h, int c, unsigned count, const int *live, const ObSetBc &s)
{
    RbSetBcArgs a{ rb_args(h), s };
    a.rb.mb.live = live;
    hipLaunchKernelGGL(raggedbatch_setbc_k, dim3(count), dim3((unsigned)RB_THREADS[c]), h->pl.lds[c], ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

// class c's set_a kernel on the `count` problems of the list (their new A lies behind their slots' pointers already)
int rg_seta(const thip_raggedbatch *h, int c, unsigned count, const int *live, const ObSetA &s)
{
    RbSetAArgs a{ rb_args(h), s.keep };
    a.rb.mb.live = live;
    hipLaunchKernelGGL(raggedbatch_seta_k, dim3(count), dim3((unsigned)RB_THREADS[c]), h->pl.lds[c], ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

// (ob_replace's init launch: one slot, by its class)
int rb_launch_hook(const OwnBatch *ob, bool run, const ObArgs &a, unsigned count)
{
    const thip_raggedbatch *h = static_cast<const thip_raggedbatch *>(ob);
    if (run || count != 1 || a.live || a.first < 0 || (size_t)a.first >= h->n_prob)
        return fail(THIP_E_INVALID, "a ragged batch launches by class", __FILE__, __LINE__);
    return rg_launch(h, false, h->pl.prob[(size_t)a.first].cls, 1, 0, nullptr, a.first);
}

// problem i's block of the arena
const float *rb_block(const thip_raggedbatch *h, int i) { return h->arena + h->pl.desc[(size_t)i].arena_at; }

void rb_info_fill(const RbPlan &pl, thip_raggedbatch_info_t &o)
{
    o.n_prob = (int32_t)pl.prob.size();
    o.n_layouts = pl.n_layouts;
    o.arena_bytes = pl.arena_floats * sizeof(float);
    o.a_bytes_per_iter = pl.a_bytes;
    for (int c = 0; c < 2; ++c) {
        o.cls[c].n_prob = (int32_t)pl.members[c].size();
        o.cls[c].threads = RB_THREADS[c];
        o.cls[c].lds_bytes = (int32_t)pl.lds[c];
    }
}

int rb_info(const thip_raggedbatch *h, thip_raggedbatch_info_t *o)
{
    if (!h || !o) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    memset(o, 0, sizeof(*o));
    rb_info_fill(h->pl, *o);
    o->live = (int32_t)h->live.size();
    o->device_bytes = h->bytes;
    o->device_bytes_all = h->fam->total;
    o->launches = h->launches; o->workgroups = h->workgroups;
    for (int p : h->live) o->cls[h->pl.prob[(size_t)p].cls].live += 1;
    for (size_t p = 0; p < h->n_prob; ++p) o->n_load16 += (h->pl.prob[p].m & 3) == 0 && !h->unaligned[p];
    for (int c = 0; c < 2; ++c) { o->cls[c].launches = h->cl_launches[c]; o->cls[c].workgroups = h->cl_workgroups[c]; }
    return 0;
}

int rb_destroy(thip_raggedbatch *h)
{
    if (!h) return 0;
    if (ctx().inited) hipStreamSynchronize(ctx().stream);
    hipFree(h->desc_dev);
    return ob_destroy(h);
}

// Every refusal comes before the first allocation; a later failure destroys what was built
int rb_create(size_t n_prob, const size_t *host_n, const size_t *host_m, const float *dev_a, const int64_t *at_a, const float *dev_b,
              const int64_t *at_b, const float *dev_c, const int64_t *at_c, const float *dev_r, const int64_t *at_r,
              const size_t *host_n_seg, const int32_t *seg_type, const int64_t *seg_len, const thip_param *par, thip_raggedbatch **out)
{
    if (!out) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *out = nullptr;
    THIP_NEED_INIT();
    if (!par || !dev_a || !dev_b || !dev_c || !at_a || !at_b || !at_c) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (par->state_arith != THIP_STATE_COMPENSATED && par->state_arith != THIP_STATE_PLAIN)
        return fail(THIP_E_INVALID, "bad thip_param.state_arith", __FILE__, __LINE__);
    if (((uintptr_t)dev_a | (uintptr_t)dev_b | (uintptr_t)dev_c | (uintptr_t)dev_r) & 3u)
        return fail(THIP_E_INVALID, "the arrays hold floats: 4-byte alignment", __FILE__, __LINE__);
    thip_raggedbatch *h = new thip_raggedbatch();
    h->fam = &RB_FAMILY;
    int rc = rb_plan(n_prob, host_n, host_m, host_n_seg, seg_type, seg_len, 0, h->pl, nullptr, nullptr, nullptr);
    for (size_t p = 0; rc == 0 && p < n_prob; ++p)
        if (at_a[p] < 0 || at_b[p] < 0 || at_c[p] < 0 || (dev_r && at_r && at_r[p] < -1))
            rc = fail(THIP_E_INVALID, "a negative offset (only a problem's row sums may be absent: -1)", __FILE__, __LINE__);
    if (rc != 0) { delete h; return rc; }
    h->n_prob = n_prob;
    h->par = *par;
    std::vector<SbSlot> slots(n_prob);
    h->unaligned.assign(n_prob, 0);
    h->slot_a.assign(n_prob, nullptr);
    h->slot_base.assign(n_prob, 0);
    for (size_t p = 0; p < n_prob; ++p) {
        slots[p] = SbSlot{ dev_a + at_a[p], dev_b + at_b[p], dev_c + at_c[p], (dev_r && at_r && at_r[p] >= 0) ? dev_r + at_r[p] : nullptr };
        h->slot_a[p] = slots[p].a;
        h->unaligned[p] = ((uintptr_t)slots[p].a & 15u) != 0;
        h->n_unaligned += h->unaligned[p];
    }
    rc = ob_attr(RB_FAMILY);
    auto build = [&]() -> int {
        const RbPlan &pl = h->pl;
        THIP_RC(ob_alloc(h, (void **)&h->arena, pl.arena_floats * sizeof(float)));
        THIP_RC(ob_alloc(h, (void **)&h->dst, n_prob * sizeof(SbStatus)));
        THIP_RC(ob_alloc(h, (void **)&h->slots, n_prob * sizeof(SbSlot)));
        THIP_RC(ob_alloc(h, (void **)&h->live_dev, n_prob * sizeof(int)));
        THIP_RC(ob_alloc(h, (void **)&h->desc_dev, n_prob * sizeof(RbDesc)));
        THIP_RC(ob_alloc(h, (void **)&h->cls_dev, (pl.cls.size() + 3) & ~(size_t)3));
        THIP_RC(ob_alloc(h, (void **)&h->cones_dev, std::max<size_t>(pl.cones.size(), 3) * sizeof(int)));
        THIP_TRY(hipHostMalloc((void **)&h->hst, n_prob * sizeof(SbStatus), hipHostMallocDefault));
        THIP_TRY(hipMemcpy(h->cls_dev, pl.cls.data(), pl.cls.size(), hipMemcpyHostToDevice));
        if (!pl.cones.empty()) THIP_TRY(hipMemcpy(h->cones_dev, pl.cones.data(), pl.cones.size() * sizeof(int), hipMemcpyHostToDevice));
        THIP_TRY(hipMemcpy(h->desc_dev, pl.desc.data(), n_prob * sizeof(RbDesc), hipMemcpyHostToDevice));
        THIP_TRY(hipMemcpy(h->slots, slots.data(), n_prob * sizeof(SbSlot), hipMemcpyHostToDevice));
        THIP_TRY(hipMemset(h->dst, 0, n_prob * sizeof(SbStatus)));
        return 0;
    };
    if (rc == 0) rc = build();
    if (rc != 0) { rb_destroy(h); return rc; }
    *out = h;
    return 0;
}

int rb_member(thip_raggedbatch *h, int i)
{
    THIP_NEED_INIT();
    return ob_member(RB_FAMILY, h, i);
}

}  // namespace

extern "C" {

int thip_raggedbatch_fits(size_t n_prob, const size_t *host_n, const size_t *host_m, const size_t *host_n_seg,
                          const int32_t *host_seg_type, const int64_t *host_seg_len, int *host_first_refused, size_t *host_lds_bytes,
                          int *host_threads)
{
    RbPlan pl;
    return rb_plan(n_prob, host_n, host_m, host_n_seg, host_seg_type, host_seg_len, 0, pl, host_first_refused, host_lds_bytes, host_threads);
}

int thip_raggedbatch_create(size_t n_prob, const size_t *host_n, const size_t *host_m, const float *dev_a, const int64_t *host_at_a,
                            const float *dev_b, const int64_t *host_at_b, const float *dev_c, const int64_t *host_at_c,
                            const float *dev_b_rowabs, const int64_t *host_at_rowabs, const size_t *host_n_seg,
                            const int32_t *host_seg_type, const int64_t *host_seg_len, const thip_param *par, thip_raggedbatch **out)
{
    return rb_create(n_prob, host_n, host_m, dev_a, host_at_a, dev_b, host_at_b, dev_c, host_at_c, dev_b_rowabs, host_at_rowabs,
                     host_n_seg, host_seg_type, host_seg_len, par, out);
}

int thip_raggedbatch_set_param(thip_raggedbatch *h, const thip_param *par) { return ob_set_param(h, par); }
int thip_raggedbatch_init(thip_raggedbatch *h) { return rg_init(RB_TEXT, h); }
int thip_raggedbatch_run(thip_raggedbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{ return rg_run(RB_TEXT, h, max_steps, poll_every, host_status, false); }
int thip_raggedbatch_run_until_any(thip_raggedbatch *h, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{ return rg_run(RB_TEXT, h, max_steps, poll_every, host_status, true); }
int thip_raggedbatch_status(thip_raggedbatch *h, int i, thip_status *host_status) { return ob_status(RB_FAMILY, h, i, host_status); }

int thip_raggedbatch_solution(thip_raggedbatch *h, int i, float *host_x, float *host_y)
{
    THIP_RC(rb_member(h, i));
    return ob_solution_at(h, i, rb_block(h, i), h->pl.prob[(size_t)i].n, h->pl.prob[(size_t)i].m, host_x, host_y);
}

int thip_raggedbatch_iterate(thip_raggedbatch *h, int i, float *host_x, float *host_y)
{
    THIP_RC(rb_member(h, i));
    return ob_iterate_at(h, i, rb_block(h, i), h->pl.prob[(size_t)i].n, h->pl.prob[(size_t)i].m, host_x, host_y);
}

int thip_raggedbatch_precond(thip_raggedbatch *h, int i, float *host_dp_tau, float *host_dp_sigma)
{
    THIP_RC(rb_member(h, i));
    return ob_precond_at(h, i, rb_block(h, i), h->pl.prob[(size_t)i].n, h->pl.prob[(size_t)i].m, host_dp_tau, host_dp_sigma);
}

// (the slot keeps its descriptor: new data of the same shape and layout, the init kernel on that slot)
int thip_raggedbatch_replace(thip_raggedbatch *h, int i, const float *dev_mat_a, const float *dev_vec_b, const float *dev_vec_c,
                             const float *dev_vec_b_rowabs)
{ return ob_replace(RB_FAMILY, h, i, dev_mat_a, dev_vec_b, dev_vec_c, dev_vec_b_rowabs); }

int thip_raggedbatch_set_iterates(thip_raggedbatch *h, int first, int count, const float *host_x, const float *host_y)
{ return rg_set_iterates(RB_FAMILY, h, first, count, host_x, host_y); }

int thip_raggedbatch_set_bc(thip_raggedbatch *h, int first, int count, const float *host_b, const float *host_c,
                            const float *host_b_rowabs, const uint8_t *host_has_rowabs, int keep_iterate)
{ return rg_set_bc(RB_FAMILY, h, first, count, host_b, host_c, host_b_rowabs, host_has_rowabs, keep_iterate); }

int thip_raggedbatch_solutions(thip_raggedbatch *h, int first, int count, float *host_x, float *host_y, thip_status *host_status)
{ return rg_solutions(RB_FAMILY, h, first, count, host_x, host_y, host_status); }

int thip_raggedbatch_set_a(thip_raggedbatch *h, int first, int count, const float *host_values, const int64_t *host_counts, int keep_iterate)
{ return rg_set_a_dense(RB_FAMILY, h, first, count, host_values, host_counts, keep_iterate); }

int thip_raggedbatch_set_bc_dev(thip_raggedbatch *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_b_rowabs,
                                const uint8_t *host_has_rowabs, int keep_iterate)
{ return rg_set_bc_dev(RB_FAMILY, h, first, count, dev_b, dev_c, dev_b_rowabs, host_has_rowabs, keep_iterate); }

int thip_raggedbatch_set_a_dev(thip_raggedbatch *h, int first, int count, const float *dev_values, int keep_iterate)
{ return rg_set_a_dev_dense(RB_FAMILY, h, first, count, dev_values, keep_iterate); }

int thip_raggedbatch_set_iterates_dev(thip_raggedbatch *h, int first, int count, const float *dev_x, const float *dev_y)
{ return rg_set_iterates_dev(RB_FAMILY, h, first, count, dev_x, dev_y); }

int thip_raggedbatch_solutions_dev(thip_raggedbatch *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state)
{ return rg_solutions_dev(RB_FAMILY, h, first, count, dev_x, dev_y, dev_state); }

int thip_raggedbatch_info(const thip_raggedbatch *h, thip_raggedbatch_info_t *host_info) { return rb_info(h, host_info); }
int thip_raggedbatch_destroy(thip_raggedbatch *h) { return rb_destroy(h); }

int thip_test_raggedbatch_force_threads(thip_raggedbatch *h, int threads)
{
    THIP_RC(ob_force_threads(RB_FAMILY, h, threads));
    rb_classes(h->pl, threads);
    return 0;
}

int thip_test_raggedbatch_plan(size_t n_prob, const size_t *host_n, const size_t *host_m, const size_t *host_n_seg,
                               const int32_t *host_seg_type, const int64_t *host_seg_len, int force_threads, int *host_class,
                               int *host_order, int *host_layout, int64_t *host_arena_at, thip_raggedbatch_info_t *host_info)
{
    RbPlan pl;
    THIP_RC(rb_plan(n_prob, host_n, host_m, host_n_seg, host_seg_type, host_seg_len, force_threads, pl, nullptr, nullptr, nullptr));
    for (size_t p = 0; p < n_prob; ++p) {
        if (host_class) host_class[p] = pl.prob[p].cls;
        if (host_layout) host_layout[p] = pl.prob[p].layout;
        if (host_arena_at) host_arena_at[p] = pl.desc[p].arena_at;
    }
    if (host_order) {
        size_t k = 0;
        for (int c = 0; c < 2; ++c)
            for (int p : pl.members[c]) host_order[k++] = p;
    }
    if (host_info) {
        memset(host_info, 0, sizeof(*host_info));
        rb_info_fill(pl, *host_info);
    }
    return 0;
}

}  // extern "C"
