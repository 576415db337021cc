// thip_raggedsparse.hip -- thip_raggedsparse: many conic programs in one batch, each with its OWN SPARSE A, its own pattern, its OWN
// shape n_p, m_p and its OWN cone layout.  The sixth own-A family, where the two seams of thip_midstream.h's bodies meet: the ragged
// batch's locator (thip_raggedbatch.hip: workgroup k looks its problem up in a table of descriptors and builds that problem's ObArgs
// by value) and the sparse batch's matrix policy (thip_sparsepass.h: the slot's `a` is the address of the problem's blob, a pass walks
// the entries).  No text of the iteration or of the pass is this file's: a problem's preconditioner, iterates and status are, bit for
// bit, those of a thip_sparsebatch that holds it alone at the same workgroup size (tests/test_gpu_raggedsparse.py).
//
// The descriptor (RsDesc, 48 bytes, read with uniform loads) holds what the ragged batch's holds -- n, m, n_cones, where the
// problem's cone triples and class bytes start in the concatenated tables, where its state starts in the arena -- and three things
// more: where the problem's blob starts (bytes from the base of the blobs; the slot's `a` is that address), where the resident copy
// lies in LDS (floats: behind this problem's own MbMap(n_p, m_p) and its own PSD tail, not the class's), and whether THIS problem
// is resident.  Residency is per problem, not per launch: in one launch some workgroups hold their blob in LDS and others read it
// from memory, and SpbA's pass runs spb_pass<_, true> or spb_pass<_, false> accordingly.  Both give the same bits.
//
// The plan (rs_plan, rs_classes: no device needed, the single source of all of it).  A problem is taken exactly when sp_check takes
// its (n_p, m_p, layout) and cap_p <= m_p n_p; cap_p, the entries slot p can take, is the problem's own entry count unless the caller
// gives more.  The workgroup size is spb_threads_for(n_p, m_p, cap_p) -- the sparse family's rule -- which splits the problems into a
// 256-thread and a 1024-thread class (a forced size puts every problem in one).  A problem is resident exactly when
// sp_lds_for(n_p, m_p, 0, psd_p) + spb_cap_bytes(n_p, m_p, cap_p) <= OB_LDS_MAX; a class's dynamic LDS is the largest
// sp_lds_for + (resident ? capacity : 0) of its members.  Every poll makes one launch per class that has a running problem.  A class's
// live list runs by descending entry count (as of create), ties by index: a pass costs the entries, not m n.  No result depends on that
// order, on the class or on the launch cuts.  The blobs are packed, slot p reserving spb_cap_bytes(n_p, m_p, cap_p) bytes from a
// multiple of 16; the state is packed, mb_stride(n_p, m_p) floats each; identical layouts share one cone table and one class-byte
// table.  Every problem's CSC arrays go through spb_validate on the host before anything is uploaded.
//
// Not here: classes cut further by LDS size (a class takes the LDS of its largest member, which bounds how many of its workgroups a
// CU holds), a replace that changes a slot's shape or layout, and any automatic choice between this family and the dense ones.
//
// This file: the two kernels, the plan, the handle and the C API (RbAt and the launches by class -- init, run -- are
// thip_raggedhost.h's, one text with thip_raggedbatch.hip; thip_ownbatch.h's generic bodies where a handle of one shape and a
// handle of many do the same thing: poll, status, set_param, destroy, the slot's part of replace, solution / iterate / precond through
// their _at forms; create, replace's blob and info are this family's own).
#include "thip_raggedhost.h"
#include "thip_sparsepass.h"

#include <map>
#include <tuple>

using namespace thip;

namespace {

// what a workgroup reads about its problem (48 bytes of uniform loads)
struct RsDesc {
    int n, m, n_cones;
    int cones_at;                           // where its (beg, end, kind) triples start in the cone table, in ints
    int cls_at;                             // where its class bytes start in the class table
    int lds_at;                             // where its blob's resident copy lies in LDS, in floats: its own map, then its own PSD tail
    long long arena_at;                     // where its mb_stride(n, m) floats of state start in the arena
    long long blob_at;                      // where its blob starts, in bytes from the base of the blobs (a multiple of 16)
    int resident, pad;                      // 1: the workgroup copies the blob into LDS at launch entry and reads it there
};
static_assert(sizeof(RsDesc) == 48, "RsDesc is copied as an array");

// mb: the words every problem shares (cls, cones and arena are the tables' and the arena's bases; n, m, n_cones, stride unused)
struct RsArgs { ObArgs mb; const RsDesc *desc; };

// the launch arguments and the matrix policy a sparse batch of this workgroup's problem alone would have had
__device__ __forceinline__ ObArgs rs_problem(const RsArgs &a, RbAt &at, SpbA &mat)
{
    const int p = ob_problem(a.mb.live, a.mb.first);
    const RsDesc d = a.desc[p];
    ObArgs b = a.mb;
    b.n = d.n; b.m = d.m; b.n_cones = d.n_cones;
    b.cones = a.mb.cones + d.cones_at;
    b.cls = a.mb.cls + d.cls_at;
    at.p = p; at.ar = a.mb.arena + d.arena_at;
    mat.at = d.lds_at; mat.resident = d.resident;
    return b;
}

__global__ __launch_bounds__(1024) void raggedsparse_init_k(const RsArgs a)
{
    RbAt at;
    SpbA mat;
    const ObArgs b = rs_problem(a, at, mat);
    mb_init_body(b, at, mat);
}

__global__ __launch_bounds__(1024) void raggedsparse_k(const RsArgs a)
{
    RbAt at;
    SpbA mat;
    const ObArgs b = rs_problem(a, at, mat);
    mb_iterate_body(b, SpCones{ (int)(MbMap(b.n, b.m).bytes(b.m) / sizeof(float)) }, at, mat);
}

// a problem starts from a given iterate (thip_raggedsparse_set_iterates): one launch per class, the problems by list, each
// resident or streamed as its descriptor says
struct RsStartArgs { RsArgs rs; ObStart s; };

__global__ __launch_bounds__(1024) void raggedsparse_start_k(const RsStartArgs a)
{
    RbAt at;
    SpbA mat;
    const ObArgs b = rs_problem(a.rs, at, mat);
    mb_start_body(b, ob_staged(a.s), at, mat);
}

// a problem takes a new (b, c) and keeps its blob (thip_raggedsparse_set_bc): one launch per class, the problems by list, each
// resident or streamed as its descriptor says
struct RsSetBcArgs { RsArgs rs; ObSetBc s; };

__global__ __launch_bounds__(1024) void raggedsparse_setbc_k(const RsSetBcArgs a)
{
    RbAt at;
    SpbA mat;
    const ObArgs b = rs_problem(a.rs, at, mat);
    mb_setbc_body(b, a.s, at, mat);
}

// a problem's A has new values in its present pattern (thip_raggedsparse_set_a): per class the scatter into the blobs in memory,
// a launch of its own (thip_sparsepass.h says why), then init's body on each new blob, resident or streamed as the descriptor says
struct RsScatterArgs { RsArgs rs; ObStart s; };

__global__ __launch_bounds__(1024) void raggedsparse_scatter_k(const RsScatterArgs a)
{
    const int p = ob_problem(a.rs.mb.live, a.rs.mb.first);
    const RsDesc d = a.rs.desc[p];
    spb_scatter(const_cast<unsigned *>(reinterpret_cast<const unsigned *>(a.rs.mb.slots[p].a)), d.m, d.n, ob_staged(a.s));
}

struct RsSetAArgs { RsArgs rs; int keep; };

__global__ __launch_bounds__(1024) void raggedsparse_seta_k(const RsSetAArgs a)
{
    RbAt at;
    SpbA mat;
    const ObArgs b = rs_problem(a.rs, at, mat);
    mb_seta_body(b, a.keep, at, mat);
}

// ---- the host side ------------------------------------------------------------------------------------------------------------

const ObText RS_TEXT = { "ragged sparse batch not initialised", "null ragged sparse batch", "a ragged sparse batch holds 1 .. 1048576 problems",
                         nullptr, "the workgroup size is 256 or 1024 (0: by shape)",
                         "thip_test_raggedsparse_force_threads comes before thip_raggedsparse_init" };

int rs_launch_hook(const OwnBatch *h, bool run, const ObArgs &a, unsigned count);
int rs_threads_unused(size_t, size_t) { return 1024; }       // (the table's thread choice knows no capacity: rs_classes decides)

// the shape rule is the SDP batch's (sp_check); the launch hook serves ob_replace: the init kernel on one slot
ObFamily RS_FAMILY = { RS_TEXT, { 256, 1024, 0 }, false, sp_check, rs_threads_unused, sp_lds_for, mb_stride, rs_launch_hook, nullptr,
                       nullptr, nullptr,
                       { (const void *)raggedsparse_k, (const void *)raggedsparse_init_k, (const void *)raggedsparse_start_k,
                         (const void *)raggedsparse_setbc_k, (const void *)raggedsparse_seta_k, nullptr } };

struct RsProb {
    size_t n, m, cap, nnz;                  // cap: the entries the slot can take; nnz: those it was planned with
    size_t vec_lds, cap_bytes;              // sp_lds_for of the problem alone; spb_cap_bytes(n, m, cap)
    ObPsd psd;
    int layout, cls, resident;
    bool can_reside() const { return vec_lds + cap_bytes <= OB_LDS_MAX; }
};

// everything create decides before it allocates (no device needed)
struct RsPlan {
    std::vector<RsProb> prob;
    std::vector<RsDesc> desc;
    std::vector<int> cones;                 // the layouts' triples, one layout after another
    std::vector<unsigned char> cls;         // the layouts' class bytes
    int n_layouts = 0;
    size_t arena_floats = 0, blob_bytes = 0, nnz_total = 0;
    // the classes: 0 of 256 threads, 1 of 1024.  members: in the order of the class's live list
    std::vector<int> members[2];
    size_t lds[2] = { 0, 0 };
    int n_res[2] = { 0, 0 };
};

// the class split, who is resident, the classes' LDS and the order within a class.  forced: 0, 256 or 1024; force_resident: 0 nobody,
// else (1, or -1: the rule) everybody who fits
void rs_classes(RsPlan &pl, int forced, int force_resident)
{
    for (int c = 0; c < 2; ++c) { pl.members[c].clear(); pl.lds[c] = 0; pl.n_res[c] = 0; }
    for (size_t p = 0; p < pl.prob.size(); ++p) {
        RsProb &q = pl.prob[p];
        q.cls = (forced ? forced : spb_threads_for(q.n, q.m, q.cap)) == RB_THREADS[1];
        q.resident = force_resident != 0 && q.can_reside();
        pl.desc[p].resident = q.resident;
        pl.members[q.cls].push_back((int)p);
        pl.lds[q.cls] = std::max(pl.lds[q.cls], q.vec_lds + (q.resident ? q.cap_bytes : 0));
        pl.n_res[q.cls] += q.resident;
    }
    for (int c = 0; c < 2; ++c)             // descending entry count, ties by index (the members are in index order: a stable sort keeps it)
        std::stable_sort(pl.members[c].begin(), pl.members[c].end(),
                         [&](int x, int y) { return pl.prob[(size_t)x].nnz > pl.prob[(size_t)y].nnz; });
}

// what a plan is made from.  Either the problems' CSC arrays (colptr: the column pointers of all problems, n_p + 1 each, one problem
// after another; problem p's row indices and values start at start[p]) -- then every problem goes through spb_validate -- or the entry
// counts alone (nnz; NULL: the capacities).  cap: the entries each slot can take (NULL or an entry of 0: the problem's own count)
struct RsInput {
    const size_t *n, *m, *cap, *nnz;
    const int64_t *colptr, *start;
    const int32_t *rowidx;
    const float *values;
    const size_t *n_seg;
    const int32_t *seg_type;
    const int64_t *seg_len;
};

int rs_plan(size_t n_prob, const RsInput &in, int forced, int force_resident, RsPlan &pl, int *first_refused)
{
    if (first_refused) *first_refused = -1;
    if (n_prob < 1 || n_prob > OB_MAX_PROB) return fail(THIP_E_INVALID, RS_TEXT.count, __FILE__, __LINE__);
    if (!in.n || !in.m || !in.n_seg || (in.colptr && !in.start)) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (forced != 0 && forced != RB_THREADS[0] && forced != RB_THREADS[1]) return fail(THIP_E_INVALID, RS_TEXT.force_sizes, __FILE__, __LINE__);
    std::map<std::tuple<size_t, std::vector<int32_t>, std::vector<int64_t>>, int> seen;
    std::vector<int> lay_cones_at, lay_cls_at, lay_n_cones;
    pl.prob.resize(n_prob);
    pl.desc.resize(n_prob);
    size_t seg0 = 0, cp0 = 0;
    for (size_t p = 0; p < n_prob; ++p) {
        const size_t n = in.n[p], m = in.m[p], ns = in.n_seg[p];
        const int32_t *st = ns ? in.seg_type + seg0 : nullptr;
        const int64_t *sl = ns ? in.seg_len + seg0 : nullptr;
        if (ns && (!in.seg_type || !in.seg_len)) return rb_refuse(p, fail(THIP_E_INVALID, "null cone segments", __FILE__, __LINE__), first_refused);
        std::vector<int> cones;
        std::vector<unsigned char> cls;
        ObPsd psd;
        const int rc = sp_check(n, m, ns, st, sl, &cones, &cls, &psd);      // (first: n and m are sane from here on)
        if (rc != 0) return rb_refuse(p, rc, first_refused);
        const size_t given = in.cap ? in.cap[p] : 0;
        if (given > m * n) {
            char msg[120];
            snprintf(msg, sizeof(msg), "nnz_cap %zu exceeds m n = %zu", given, m * n);
            return rb_refuse(p, fail(THIP_E_INVALID, msg, __FILE__, __LINE__), first_refused);
        }
        size_t nnz;
        if (in.colptr) {                    // the stored form: every index the device will see is checked here
            const int64_t *cp = in.colptr + cp0;
            if (in.start[p] < 0) return rb_refuse(p, fail(THIP_E_INVALID, "a negative start offset", __FILE__, __LINE__), first_refused);
            const int bad = spb_validate(n, m, cp, in.rowidx ? in.rowidx + in.start[p] : nullptr, in.values ? in.values + in.start[p] : nullptr,
                                         given ? given : m * n, (long)p);
            if (bad != 0) { if (first_refused) *first_refused = (int)p; return bad; }
            nnz = (size_t)cp[n];
        } else {
            nnz = in.nnz ? in.nnz[p] : given;
            if (nnz > m * n || (given && nnz > given)) {
                char msg[120];
                snprintf(msg, sizeof(msg), "%zu entries where nnz_cap is %zu", nnz, given ? given : m * n);
                return rb_refuse(p, fail(THIP_E_INVALID, msg, __FILE__, __LINE__), first_refused);
            }
        }
        const size_t cap = given ? given : nnz;
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
        RsProb &q = pl.prob[p];
        q = RsProb{ n, m, cap, nnz, sp_lds_for(n, m, 0, psd), spb_cap_bytes(n, m, cap), psd, lay, 0, 0 };
        RsDesc &d = pl.desc[p];
        d.n = (int)n; d.m = (int)m; d.n_cones = lay_n_cones[(size_t)lay];
        d.cones_at = lay_cones_at[(size_t)lay]; d.cls_at = lay_cls_at[(size_t)lay];
        d.lds_at = (int)(q.vec_lds / sizeof(float));       // MbMap(n, m).bytes(m) and the PSD tail are both whole floats
        d.arena_at = (long long)pl.arena_floats;
        // the blobs are packed: every capacity is a multiple of 16 bytes, so every slot starts at a multiple of 16 from the base
        // (which hipMalloc aligns) and reserves its whole capacity -- what keeps SpbA::open's 16-byte copy loop, which reads the used
        // words rounded up to four, inside the slot
        d.blob_at = (long long)pl.blob_bytes;
        d.resident = 0; d.pad = 0;
        pl.arena_floats += mb_stride(n, m);
        pl.blob_bytes += q.cap_bytes;
        pl.nnz_total += nnz;
        seg0 += ns;
        cp0 += n + 1;
    }
    pl.n_layouts = (int)lay_cls_at.size();
    rs_classes(pl, forced, force_resident);
    return 0;
}

}  // namespace

struct thip_raggedsparse : OwnBatch {
    RsPlan pl;
    RsDesc *desc_dev = nullptr;
    unsigned char *blobs = nullptr;
    std::vector<uint32_t> slot_used;        // the words of its capacity each slot uses
    int force_resident = -1;
    std::vector<int> cl_live[2];            // the classes' live lists as of the last launch
    int64_t cl_launches[2] = { 0, 0 }, cl_workgroups[2] = { 0, 0 };
};

namespace {

RsArgs rs_args(const thip_raggedsparse *h)
{
    RsArgs a{ ob_args(h), h->desc_dev };
    a.mb.n = a.mb.m = a.mb.n_cones = 0;
    a.mb.stride = 0;
    return a;
}

// class c's kernel -- the init kernel or `steps` iterations -- on `count` problems: those of the list, or (live == NULL) first ..
int rg_launch(const thip_raggedsparse *h, bool run, int c, unsigned count, int steps, const int *live, int first)
{
    RsArgs a = rs_args(h);
    a.mb.steps = steps; a.mb.live = live; a.mb.first = first;
    hipLaunchKernelGGL(run ? raggedsparse_k : raggedsparse_init_k, dim3(count), dim3((unsigned)RB_THREADS[c]), h->pl.lds[c], ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

// class c's start kernel on the `count` problems of the list, workgroup k's iterate at s.at[k]
int rg_start(const thip_raggedsparse *h, int c, unsigned count, const int *live, const ObStart &s)
{
    RsStartArgs a{ rs_args(h), s };
    a.rs.mb.live = live;
    hipLaunchKernelGGL(raggedsparse_start_k, dim3(count), dim3((unsigned)RB_THREADS[c]), h->pl.lds[c], ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

// class c's set_bc kernel on the `count` problems of the list, workgroup k's data at s.s.at[k]
int rg_setbc(const thip_raggedsparse *h, int c, unsigned count, const int *live, const ObSetBc &s)
{
    RsSetBcArgs a{ rs_args(h), s };
    a.rs.mb.live = live;
    hipLaunchKernelGGL(raggedsparse_setbc_k, dim3(count), dim3((unsigned)RB_THREADS[c]), h->pl.lds[c], ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

// class c's scatter (no LDS) and then its set_a kernel on the `count` problems of the list, workgroup k's values at s.s.at[k]
int rg_seta(const thip_raggedsparse *h, int c, unsigned count, const int *live, const ObSetA &s)
{
    RsScatterArgs sc{ rs_args(h), s.s };
    sc.rs.mb.live = live;
    hipLaunchKernelGGL(raggedsparse_scatter_k, dim3(count), dim3((unsigned)RB_THREADS[c]), 0, ctx().stream, sc);
    THIP_LAUNCH_CHECK();
    RsSetAArgs a{ rs_args(h), s.keep };
    a.rs.mb.live = live;
    hipLaunchKernelGGL(raggedsparse_seta_k, dim3(count), dim3((unsigned)RB_THREADS[c]), h->pl.lds[c], ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

// (ob_replace's init launch: one slot, by its class)
int rs_launch_hook(const OwnBatch *ob, bool run, const ObArgs &a, unsigned count)
{
    const thip_raggedsparse *h = static_cast<const thip_raggedsparse *>(ob);
    if (run || count != 1 || a.live || a.first < 0 || (size_t)a.first >= h->n_prob)
        return fail(THIP_E_INVALID, "a ragged sparse batch launches by class", __FILE__, __LINE__);
    return rg_launch(h, false, h->pl.prob[(size_t)a.first].cls, 1, 0, nullptr, a.first);
}

// the descriptors as the plan has them now (the test hooks change the resident flags between create and init), then the init kernel
// on every problem, class by class
int rs_init(thip_raggedsparse *h)
{
    THIP_NEED_INIT();
    if (!h) return fail(THIP_E_INVALID, RS_TEXT.null_h, __FILE__, __LINE__);
    THIP_TRY(hipStreamSynchronize(ctx().stream));
    THIP_TRY(hipMemcpy(h->desc_dev, h->pl.desc.data(), h->n_prob * sizeof(RsDesc), hipMemcpyHostToDevice));
    return rg_init(RS_TEXT, h);
}

// problem i's block of the arena
const float *rs_block(const thip_raggedsparse *h, int i) { return h->arena + h->pl.desc[(size_t)i].arena_at; }

// the part of info() that needs no device
void rs_info_fill(const RsPlan &pl, thip_raggedsparse_info_t &o)
{
    o.n_prob = (int32_t)pl.prob.size();
    o.n_layouts = pl.n_layouts;
    o.arena_bytes = pl.arena_floats * sizeof(float);
    o.nnz_total = pl.nnz_total;
    o.blob_bytes = pl.blob_bytes;
    for (const RsProb &q : pl.prob) {
        o.max_psd_order = std::max(o.max_psd_order, (int32_t)q.psd.max_k);
        o.n_psd += q.psd.n_psd;
        o.psd_lds_bytes = std::max(o.psd_lds_bytes, q.psd.tail_bytes);
    }
    for (int c = 0; c < 2; ++c) {
        o.cls[c].n_prob = (int32_t)pl.members[c].size();
        o.cls[c].threads = RB_THREADS[c];
        o.cls[c].lds_bytes = (int32_t)pl.lds[c];
        o.cls[c].n_resident = pl.n_res[c];
        o.n_resident += pl.n_res[c];
    }
}

int rs_info(const thip_raggedsparse *h, thip_raggedsparse_info_t *o)
{
    if (!h || !o) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    memset(o, 0, sizeof(*o));
    rs_info_fill(h->pl, *o);
    o->live = (int32_t)h->live.size();
    o->device_bytes = h->bytes;
    o->device_bytes_all = h->fam->total;
    o->launches = h->launches; o->workgroups = h->workgroups;
    for (int p : h->live) o->cls[h->pl.prob[(size_t)p].cls].live += 1;
    for (size_t p = 0; p < h->n_prob; ++p)
        if (!h->pl.prob[p].resident) o->a_bytes_per_iter += 2 * 4 * (size_t)h->slot_used[p];
    for (int c = 0; c < 2; ++c) { o->cls[c].launches = h->cl_launches[c]; o->cls[c].workgroups = h->cl_workgroups[c]; }
    return 0;
}

int rs_destroy(thip_raggedsparse *h)
{
    if (!h) return 0;
    if (ctx().inited) hipStreamSynchronize(ctx().stream);
    hipFree(h->desc_dev);
    hipFree(h->blobs);
    return ob_destroy(h);
}

// Every refusal comes before the first allocation; a later failure destroys what was built
int rs_create(size_t n_prob, const RsInput &in, const float *dev_b, const int64_t *at_b, const float *dev_c, const int64_t *at_c,
              const float *dev_r, const int64_t *at_r, const thip_param *par, thip_raggedsparse **out)
{
    if (!out) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *out = nullptr;
    THIP_NEED_INIT();
    if (!par || !in.colptr || !in.start || !dev_b || !dev_c || !at_b || !at_c) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (par->state_arith != THIP_STATE_COMPENSATED && par->state_arith != THIP_STATE_PLAIN)
        return fail(THIP_E_INVALID, "bad thip_param.state_arith", __FILE__, __LINE__);
    if (((uintptr_t)dev_b | (uintptr_t)dev_c | (uintptr_t)dev_r) & 3u)
        return fail(THIP_E_INVALID, "the arrays hold floats: 4-byte alignment", __FILE__, __LINE__);
    thip_raggedsparse *h = new thip_raggedsparse();
    h->fam = &RS_FAMILY;
    int rc = rs_plan(n_prob, in, 0, -1, h->pl, nullptr);
    for (size_t p = 0; rc == 0 && p < n_prob; ++p)
        if (at_b[p] < 0 || at_c[p] < 0 || (dev_r && at_r && at_r[p] < -1))
            rc = fail(THIP_E_INVALID, "a negative offset (only a problem's row sums may be absent: -1)", __FILE__, __LINE__);
    if (rc != 0) { delete h; return rc; }
    h->n_prob = n_prob;
    h->par = *par;
    const RsPlan &pl = h->pl;
    // every blob packed on the host, one copy up
    std::vector<uint32_t> host(std::max<size_t>(pl.blob_bytes / 4, 4), 0u);
    h->slot_used.assign(n_prob, 0);
    size_t cp0 = 0;
    for (size_t p = 0; p < n_prob; ++p) {
        const RsProb &q = pl.prob[p];
        h->slot_used[p] = (uint32_t)spb_pack(q.n, q.m, in.colptr + cp0, in.rowidx + in.start[p], in.values + in.start[p],
                                             host.data() + pl.desc[p].blob_at / 4);
        cp0 += q.n + 1;
    }
    rc = ob_attr(RS_FAMILY);
    auto build = [&]() -> int {
        THIP_RC(ob_alloc(h, (void **)&h->arena, pl.arena_floats * sizeof(float)));
        THIP_RC(ob_alloc(h, (void **)&h->dst, n_prob * sizeof(SbStatus)));
        THIP_RC(ob_alloc(h, (void **)&h->slots, n_prob * sizeof(SbSlot)));
        THIP_RC(ob_alloc(h, (void **)&h->live_dev, n_prob * sizeof(int)));
        THIP_RC(ob_alloc(h, (void **)&h->desc_dev, n_prob * sizeof(RsDesc)));
        THIP_RC(ob_alloc(h, (void **)&h->cls_dev, (pl.cls.size() + 3) & ~(size_t)3));
        THIP_RC(ob_alloc(h, (void **)&h->cones_dev, std::max<size_t>(pl.cones.size(), 3) * sizeof(int)));
        THIP_RC(ob_alloc(h, (void **)&h->blobs, host.size() * sizeof(uint32_t)));
        THIP_TRY(hipHostMalloc((void **)&h->hst, n_prob * sizeof(SbStatus), hipHostMallocDefault));
        std::vector<SbSlot> slots(n_prob);
        for (size_t p = 0; p < n_prob; ++p)
            slots[p] = SbSlot{ reinterpret_cast<const float *>(h->blobs + pl.desc[p].blob_at), dev_b + at_b[p], dev_c + at_c[p],
                               (dev_r && at_r && at_r[p] >= 0) ? dev_r + at_r[p] : nullptr };
        THIP_TRY(hipMemcpy(h->cls_dev, pl.cls.data(), pl.cls.size(), hipMemcpyHostToDevice));
        if (!pl.cones.empty()) THIP_TRY(hipMemcpy(h->cones_dev, pl.cones.data(), pl.cones.size() * sizeof(int), hipMemcpyHostToDevice));
        THIP_TRY(hipMemcpy(h->desc_dev, pl.desc.data(), n_prob * sizeof(RsDesc), hipMemcpyHostToDevice));
        THIP_TRY(hipMemcpy(h->slots, slots.data(), n_prob * sizeof(SbSlot), hipMemcpyHostToDevice));
        THIP_TRY(hipMemcpy(h->blobs, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        THIP_TRY(hipMemset(h->dst, 0, n_prob * sizeof(SbStatus)));
        return 0;
    };
    if (rc == 0) rc = build();
    if (rc != 0) { rs_destroy(h); return rc; }
    *out = h;
    return 0;
}

int rs_member(thip_raggedsparse *h, int i)
{
    THIP_NEED_INIT();
    return ob_member(RS_FAMILY, h, i);
}

}  // namespace

extern "C" {

int thip_raggedsparse_fits(size_t n_prob, const size_t *host_n, const size_t *host_m, const size_t *host_nnz_cap, const size_t *host_n_seg,
                           const int32_t *host_seg_type, const int64_t *host_seg_len, int *host_first_refused, size_t *host_lds_bytes,
                           int *host_threads, int *host_resident)
{
    RsPlan pl;
    const RsInput in{ host_n, host_m, host_nnz_cap, nullptr, nullptr, nullptr, nullptr, nullptr, host_n_seg, host_seg_type, host_seg_len };
    THIP_RC(rs_plan(n_prob, in, 0, -1, pl, host_first_refused));
    for (size_t p = 0; p < n_prob; ++p) {
        const RsProb &q = pl.prob[p];
        if (host_lds_bytes) host_lds_bytes[p] = q.vec_lds + (q.resident ? q.cap_bytes : 0);
        if (host_threads) host_threads[p] = RB_THREADS[q.cls];
        if (host_resident) host_resident[p] = q.resident;
    }
    return 0;
}

int thip_raggedsparse_create(size_t n_prob, const size_t *host_n, const size_t *host_m, const int64_t *host_colptr, const int64_t *host_start,
                             const int32_t *host_rowidx, const float *host_values, const size_t *host_nnz_cap, const float *dev_b,
                             const int64_t *host_at_b, const float *dev_c, const int64_t *host_at_c, const float *dev_b_rowabs,
                             const int64_t *host_at_rowabs, const size_t *host_n_seg, const int32_t *host_seg_type,
                             const int64_t *host_seg_len, const thip_param *par, thip_raggedsparse **out)
{
    const RsInput in{ host_n, host_m, host_nnz_cap, nullptr, host_colptr, host_start, host_rowidx, host_values, host_n_seg, host_seg_type,
                      host_seg_len };
    return rs_create(n_prob, in, dev_b, host_at_b, dev_c, host_at_c, dev_b_rowabs, host_at_rowabs, par, out);
}

int thip_raggedsparse_set_param(thip_raggedsparse *h, const thip_param *par) { return ob_set_param(h, par); }
int thip_raggedsparse_init(thip_raggedsparse *h) { return rs_init(h); }
int thip_raggedsparse_run(thip_raggedsparse *h, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{ return rg_run(RS_TEXT, h, max_steps, poll_every, host_status, false); }
int thip_raggedsparse_run_until_any(thip_raggedsparse *h, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{ return rg_run(RS_TEXT, h, max_steps, poll_every, host_status, true); }
int thip_raggedsparse_status(thip_raggedsparse *h, int i, thip_status *host_status) { return ob_status(RS_FAMILY, h, i, host_status); }

int thip_raggedsparse_solution(thip_raggedsparse *h, int i, float *host_x, float *host_y)
{
    THIP_RC(rs_member(h, i));
    return ob_solution_at(h, i, rs_block(h, i), h->pl.prob[(size_t)i].n, h->pl.prob[(size_t)i].m, host_x, host_y);
}

int thip_raggedsparse_iterate(thip_raggedsparse *h, int i, float *host_x, float *host_y)
{
    THIP_RC(rs_member(h, i));
    return ob_iterate_at(h, i, rs_block(h, i), h->pl.prob[(size_t)i].n, h->pl.prob[(size_t)i].m, host_x, host_y);
}

int thip_raggedsparse_precond(thip_raggedsparse *h, int i, float *host_dp_tau, float *host_dp_sigma)
{
    THIP_RC(rs_member(h, i));
    return ob_precond_at(h, i, rs_block(h, i), h->pl.prob[(size_t)i].n, h->pl.prob[(size_t)i].m, host_dp_tau, host_dp_sigma);
}

// (the slot keeps its descriptor: another pattern of at most cap_i entries of the same shape and layout, then the init kernel on
// that slot.  Every refusal comes before the slot's blob is touched)
int thip_raggedsparse_replace(thip_raggedsparse *h, int i, const int64_t *host_colptr, const int32_t *host_rowidx, const float *host_values,
                              const float *dev_vec_b, const float *dev_vec_c, const float *dev_vec_b_rowabs)
{
    THIP_RC(rs_member(h, i));
    if (!host_colptr || !dev_vec_b || !dev_vec_c) return fail(THIP_E_INVALID, "null A, b or c", __FILE__, __LINE__);
    if (((uintptr_t)dev_vec_b | (uintptr_t)dev_vec_c | (uintptr_t)dev_vec_b_rowabs) & 3u)
        return fail(THIP_E_INVALID, "the arrays hold floats: 4-byte alignment", __FILE__, __LINE__);
    RsProb &q = h->pl.prob[(size_t)i];
    THIP_RC(spb_validate(q.n, q.m, host_colptr, host_rowidx, host_values, q.cap, -1));
    std::vector<uint32_t> host(q.cap_bytes / 4, 0u);
    const size_t used = spb_pack(q.n, q.m, host_colptr, host_rowidx, host_values, host.data());
    unsigned char *const blob = h->blobs + h->pl.desc[(size_t)i].blob_at;
    THIP_TRY(hipStreamSynchronize(ctx().stream));                // (no launch is reading the slot)
    THIP_TRY(hipMemcpy(blob, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    THIP_RC(ob_replace(RS_FAMILY, h, i, reinterpret_cast<const float *>(blob), dev_vec_b, dev_vec_c, dev_vec_b_rowabs));
    const size_t nnz = (size_t)host_colptr[q.n];
    h->pl.nnz_total += nnz; h->pl.nnz_total -= q.nnz;
    q.nnz = nnz;
    h->slot_used[(size_t)i] = (uint32_t)used;
    return 0;
}

int thip_raggedsparse_set_iterates(thip_raggedsparse *h, int first, int count, const float *host_x, const float *host_y)
{ return rg_set_iterates(RS_FAMILY, h, first, count, host_x, host_y); }

int thip_raggedsparse_set_bc(thip_raggedsparse *h, int first, int count, const float *host_b, const float *host_c,
                             const float *host_b_rowabs, const uint8_t *host_has_rowabs, int keep_iterate)
{ return rg_set_bc(RS_FAMILY, h, first, count, host_b, host_c, host_b_rowabs, host_has_rowabs, keep_iterate); }

int thip_raggedsparse_solutions(thip_raggedsparse *h, int first, int count, float *host_x, float *host_y, thip_status *host_status)
{ return rg_solutions(RS_FAMILY, h, first, count, host_x, host_y, host_status); }

int thip_raggedsparse_set_a(thip_raggedsparse *h, int first, int count, const float *host_values, const int64_t *host_counts, int keep_iterate)
{
    return rg_set_a_sparse(RS_FAMILY, h, first, count, host_values, host_counts, keep_iterate,
                           [&](int p) { return h->pl.prob[(size_t)p].nnz; });
}

int thip_raggedsparse_set_bc_dev(thip_raggedsparse *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_b_rowabs,
                                 const uint8_t *host_has_rowabs, int keep_iterate)
{ return rg_set_bc_dev(RS_FAMILY, h, first, count, dev_b, dev_c, dev_b_rowabs, host_has_rowabs, keep_iterate); }

// (the values stay where the caller holds them: the scatter kernels read them there, by a table of the host's counts)
int thip_raggedsparse_set_a_dev(thip_raggedsparse *h, int first, int count, const float *dev_values, int keep_iterate)
{
    return rg_set_a_dev_sparse(RS_FAMILY, h, first, count, dev_values, keep_iterate, [&](int p) { return h->pl.prob[(size_t)p].nnz; });
}

int thip_raggedsparse_set_iterates_dev(thip_raggedsparse *h, int first, int count, const float *dev_x, const float *dev_y)
{ return rg_set_iterates_dev(RS_FAMILY, h, first, count, dev_x, dev_y); }

int thip_raggedsparse_solutions_dev(thip_raggedsparse *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state)
{ return rg_solutions_dev(RS_FAMILY, h, first, count, dev_x, dev_y, dev_state); }

int thip_raggedsparse_info(const thip_raggedsparse *h, thip_raggedsparse_info_t *host_info) { return rs_info(h, host_info); }
int thip_raggedsparse_destroy(thip_raggedsparse *h) { return rs_destroy(h); }

int thip_test_raggedsparse_force_threads(thip_raggedsparse *h, int threads)
{
    THIP_RC(ob_force_threads(RS_FAMILY, h, threads));
    rs_classes(h->pl, threads, h->force_resident);
    return 0;
}

int thip_test_raggedsparse_force_resident(thip_raggedsparse *h, int resident)
{
    if (!h) return fail(THIP_E_INVALID, RS_TEXT.null_h, __FILE__, __LINE__);
    if (resident != 0 && resident != 1) return fail(THIP_E_INVALID, "the mode is 0 (nobody resident) or 1 (everybody who fits)", __FILE__, __LINE__);
    if (h->inited) return fail(THIP_E_INVALID, "thip_test_raggedsparse_force_resident comes before thip_raggedsparse_init", __FILE__, __LINE__);
    h->force_resident = resident;
    rs_classes(h->pl, h->forced, resident);
    return 0;
}

int thip_test_raggedsparse_blob(thip_raggedsparse *h, int i, uint32_t *host_words, size_t cap_words, size_t *host_used_words)
{
    THIP_NEED_INIT();
    if (!h || !host_used_words) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (i < 0 || (size_t)i >= h->n_prob) return fail(THIP_E_INVALID, "no such problem", __FILE__, __LINE__);
    const size_t used = h->slot_used[(size_t)i];
    *host_used_words = used;
    if (!host_words) return 0;
    if (cap_words < used) return fail(THIP_E_INVALID, "the blob holds more words than were offered", __FILE__, __LINE__);
    THIP_TRY(hipStreamSynchronize(ctx().stream));
    THIP_TRY(hipMemcpy(host_words, h->blobs + h->pl.desc[(size_t)i].blob_at, used * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

int thip_test_raggedsparse_plan(size_t n_prob, const size_t *host_n, const size_t *host_m, const size_t *host_nnz, const size_t *host_nnz_cap,
                                const size_t *host_n_seg, const int32_t *host_seg_type, const int64_t *host_seg_len, int force_threads,
                                int force_resident, int *host_class, int *host_order, int *host_layout, int64_t *host_arena_at,
                                int64_t *host_blob_at, int *host_lds_at, int *host_resident, thip_raggedsparse_info_t *host_info)
{
    RsPlan pl;
    if (force_resident < -1 || force_resident > 1) return fail(THIP_E_INVALID, "the mode is -1 (the rule), 0 or 1", __FILE__, __LINE__);
    const RsInput in{ host_n, host_m, host_nnz_cap, host_nnz, nullptr, nullptr, nullptr, nullptr, host_n_seg, host_seg_type, host_seg_len };
    THIP_RC(rs_plan(n_prob, in, force_threads, force_resident, pl, nullptr));
    for (size_t p = 0; p < n_prob; ++p) {
        if (host_class) host_class[p] = pl.prob[p].cls;
        if (host_layout) host_layout[p] = pl.prob[p].layout;
        if (host_arena_at) host_arena_at[p] = pl.desc[p].arena_at;
        if (host_blob_at) host_blob_at[p] = pl.desc[p].blob_at;
        if (host_lds_at) host_lds_at[p] = pl.desc[p].lds_at;
        if (host_resident) host_resident[p] = pl.desc[p].resident;
    }
    if (host_order) {
        size_t k = 0;
        for (int c = 0; c < 2; ++c)
            for (int p : pl.members[c]) host_order[k++] = p;
    }
    if (host_info) {
        memset(host_info, 0, sizeof(*host_info));
        rs_info_fill(pl, *host_info);
    }
    return 0;
}

}  // extern "C"
