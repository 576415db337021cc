// thip_solver_batch.inc -- part of thip_solver.hip: thip_batch, B problems over the SAME dense f32 A (their own b_i, c_i) iterated in
// lockstep under the 2-pass carried schedule, so that a pass over A serves up to eight of them: per iteration and group of
// instances ONE multi-vector launch (thip_gemv_multi.hip) forms every member's A u_i, A^T v_i, then each member's stage-X tail runs;
// one more launch forms A x_x_i, A^T x_y_i, then each member's stage-C tail.  The tails, the cones, the termination test and the
// state they work on are those of an ordinary thip_solver (stage_x_tail / stage_c_tail of thip_solver_passes.inc): the instances do
// not interact, and an instance that has stopped is frozen by its own stop flag while the others go on.
//
// The stored form of A exists once: the caller's array and -- when m is no multiple of 16 floats -- ONE library-owned padded copy,
// which every instance borrows through its StoredA (the batch frees it).  The |A| row and column sums of the preconditioner are
// computed once.  Passes over A per iteration: 2 * ceil(B / max_group) instead of 2 B.
//
// The instances are slots: thip_batch_replace hands one the next problem (b, c by pointer, a fresh init from the shared |A| sums), and
// with thip_batch_set_regroup the launches of a pass are formed anew from the live instances after every poll -- ceil(live / max_group)
// of them.  Both are host-side bookkeeping over the same kernels; without them the groups stay fixed by index as above.

struct thip_batch {
    size_t n = 0, m = 0;
    std::vector<thip_solver *> inst;
    std::vector<char> live;              // host copy: instance i was RUNNING at the last poll
    const float *a_f32 = nullptr;
    float *pad = nullptr; size_t ldpad = 0;
    float *rowabs = nullptr, *colabs = nullptr;
    size_t scr_floats = 0;               // GEMV scratch of every instance
    GemvPlan mplan[4];                   // tuned tilings of the multi-vector kernel, by instance: [1] NV = 2, [2] NV = 4, [3] NV = 8
    thip_gemv_plan_rec last_mplan[4]{};  // what the latest launch of each instance ran under (thip_test_batch_last_multi_plan)
    int autotune = -1;                   // as thip_solver::autotune
    int max_group = THIP_BATCH_GROUP_DEFAULT;
    bool regroup = false;                // the launches follow the live set (thip_batch_set_regroup)
    bool inited = false;
    thip_batch_counters_t ctr{};         // what run / run_until_any issued since init; instance_iterations: the retired occupants' only
    DenseA A() const { return pad ? DenseA{ pad, ldpad, THIP_A_F32, nullptr, true } : dense_f32(a_f32, m); }
};

namespace {

int plan_slot(int instance) { return instance == 2 ? 1 : (instance == 4 ? 2 : 3); }

// B instances as groups of at most max_group, the last one holding the rest: (first instance, members) per group
void batch_groups(int n_inst, int max_group, std::vector<std::pair<int, int>> *out)
{
    out->clear();
    for (int i = 0; i < n_inst; i += max_group) out->push_back({ i, std::min(max_group, n_inst - i) });
}

// the regroup rule: the live instances in ascending index order (members), cut into groups of at most max_group -- (offset into
// members, size) per group, full groups first and the rest last
void live_groups(int n_inst, int max_group, const char *live, std::vector<int> *members, std::vector<std::pair<int, int>> *out)
{
    members->clear();
    for (int i = 0; i < n_inst; ++i) if (live[i]) members->push_back(i);
    batch_groups((int)members->size(), max_group, out);
}

int counter_slot(int members) { return members == 1 ? 0 : plan_slot(gemv_multi_instance(members)); }

const GemvHint *batch_hint(const thip_batch *b, int members)
{
    const GemvPlan &p = b->mplan[plan_slot(gemv_multi_instance(members))];
    return p.tuned ? &p.hint : nullptr;
}

// one pass over A for a group, given as the list of its members' indices: which = 0 the stage-X products (u, v), 1 the stage-C
// products (x_x, x_y); stop = the members' own flags (nullptr: unconditionally, outside the loop)
int batch_products(thip_batch *b, const int *idx, int members, int which, bool with_stop, GemvPartials *gp, const GemvHint *hint)
{
    hipStream_t st = ctx().stream;
    if (members == 1) {          // the single-vector kernel under the instance's own plan
        thip_solver *s = b->inst[idx[0]];
        if (with_stop) return which == 0 ? products(s, s->u, s->v, gp, s->h1, s->g1) : products(s, s->xx, s->xy, gp, s->h3, s->g3);
        *gp = GemvPartials{};
        if (s->m == 0 || s->n == 0) return 0;
        return dual_gemv_partials(st, s->m, s->n, b->A(), which == 0 ? s->u : s->xx, which == 0 ? s->v : s->xy, true, true, false,
                                  s->gemv_scr, s->gemv_scr_n, gp, nullptr, s->hint_in_use());
    }
    const float *xn[GEMV_MULTI_MAX], *xt[GEMV_MULTI_MAX];
    float *scr[GEMV_MULTI_MAX];
    const int *stop[GEMV_MULTI_MAX];
    for (int j = 0; j < members; ++j) {
        thip_solver *s = b->inst[idx[j]];
        xn[j] = which == 0 ? s->u : s->xx; xt[j] = which == 0 ? s->v : s->xy;
        scr[j] = s->gemv_scr; stop[j] = with_stop ? &s->dst->stop : nullptr;
    }
    prof_begin(st);
    THIP_RC(dual_gemv_multi_partials(st, b->m, b->n, b->A(), members, xn, xt, scr, b->scr_floats, stop, gp, hint,
                                     &b->last_mplan[plan_slot(gemv_multi_instance(members))]));
    prof_end(st);
    return 0;
}

// the same for members first .. first + members - 1
int batch_products(thip_batch *b, int first, int members, int which, bool with_stop, GemvPartials *gp, const GemvHint *hint)
{
    int idx[GEMV_MULTI_MAX];
    for (int j = 0; j < members; ++j) idx[j] = first + j;
    return batch_products(b, idx, members, which, with_stop, gp, hint);
}

// the padded copy (m % 16 != 0), made once and refreshed by every init: the caller may have rewritten A in place between solves
int batch_ensure_pad(thip_batch *b)
{
    hipStream_t st = ctx().stream;
    const size_t m = b->m, n = b->n;
    if (m == 0 || n == 0 || m % 16 == 0) return 0;
    const size_t ld = (m + 15) / 16 * 16;
    if (!b->pad) {
        THIP_TRY(hipMalloc((void **)&b->pad, ld * n * sizeof(float)));
        b->ldpad = ld;
        THIP_TRY(hipMemsetAsync(b->pad, 0, ld * n * sizeof(float), st));
    }
    THIP_TRY(hipMemcpy2DAsync(b->pad, ld * sizeof(float), b->a_f32, m * sizeof(float), m * sizeof(float), n, hipMemcpyDeviceToDevice, st));
    for (thip_solver *s : b->inst) { s->sa.pad = b->pad; s->sa.ldpad = ld; }      // borrowed: thip_batch_destroy takes it back
    return 0;
}

// Times the tilings of the multi-vector kernel on THIS matrix for one group size (the loop of autotune_gemv: the second reduction
// stage of every member is part of a plan's price) and keeps the fastest.  Switched off like the single-vector autotune.
int autotune_multi(thip_batch *b, int first, int members)
{
    const char *env = getenv("THIP_GEMV_AUTOTUNE");
    if (b->autotune == 0 || (b->autotune < 0 && env && atoi(env) == 0)) return 0;
    if (members < 2 || b->m * b->n < (size_t)1 << 22) return 0;
    const int instance = gemv_multi_instance(members);
    GemvPlan &plan = b->mplan[plan_slot(instance)];
    if (plan.tuned) return 0;
    hipStream_t st = ctx().stream;
    hipEvent_t e0, e1;
    THIP_TRY(hipEventCreate(&e0));
    THIP_TRY(hipEventCreate(&e1));
    int nc = 0;
    const GemvHint *c = gemv_multi_candidates(&nc);
    GemvPartials gp[GEMV_MULTI_MAX];
    float best = 1e30f;
    GemvHint pick{0, 0};
    for (int w = 0; w < 3; ++w) THIP_RC(batch_products(b, first, members, 0, false, gp, nullptr));
    for (int i = 0; i < nc; ++i) {
        if (instance == 8 && c[i].nj != 1) continue;          // (that instance holds one row group per lane)
        float ms = 1e30f;
        for (int rep = 0; rep < 5; ++rep) {
            THIP_TRY(hipEventRecord(e0, st));
            THIP_RC(batch_products(b, first, members, 0, false, gp, &c[i]));
            for (int j = 0; j < members; ++j) {
                thip_solver *s = b->inst[first + j];
                THIP_RC(finalize_partials(st, s->m, gp[j].partN, gp[j].nN, gp[j].strideN, 1.0f, 0.0f, s->h2, nullptr));
                THIP_RC(finalize_partials(st, s->n, gp[j].partT, gp[j].nT, gp[j].strideT, 1.0f, 0.0f, s->g2, nullptr));
            }
            THIP_TRY(hipEventRecord(e1, st));
            THIP_TRY(hipEventSynchronize(e1));
            float t = 0.0f;
            THIP_TRY(hipEventElapsedTime(&t, e0, e1));
            if (rep > 0 && t < ms) ms = t;
        }
        if (ms < best) { best = ms; pick = c[i]; }
    }
    plan = GemvPlan{ pick, true, best };
    THIP_TRY(hipEventDestroy(e0));
    THIP_TRY(hipEventDestroy(e1));
    return 0;
}

int batch_poll(thip_batch *b, thip_status *host_status)
{
    for (size_t i = 0; i < b->inst.size(); ++i) {
        THIP_RC(poll(b->inst[i], host_status ? host_status + i : nullptr));
        b->live[i] = b->inst[i]->hst->state == THIP_ST_RUNNING;
    }
    return 0;
}

int batch_create_impl(const thip_problem *prob, int n_inst, const float *const *host_vec_b, const float *const *host_vec_c,
                      const thip_param *par, thip_batch *b)
{
    b->n = prob->n; b->m = prob->m; b->a_f32 = prob->mat_a;
    b->live.assign((size_t)n_inst, 0);
    for (int i = 0; i < n_inst; ++i) {
        thip_problem pi = *prob;
        pi.vec_b = host_vec_b[i]; pi.vec_c = host_vec_c[i];
        thip_solver *s = nullptr;
        const int rc = solver_create_impl(&pi, par, THIP_SCHED_CARRIED, &s);
        if (s) b->inst.push_back(s);
        if (rc != 0) return rc;
    }
    if (b->m && b->n) {
        b->scr_floats = std::max(dual_gemv_scratch_floats(b->m, b->n), dual_gemv_multi_scratch_floats(b->m, b->n));
        THIP_TRY(hipMalloc((void **)&b->rowabs, b->m * sizeof(float)));
        THIP_TRY(hipMalloc((void **)&b->colabs, b->n * sizeof(float)));
    }
    return 0;
}

}  // namespace

extern "C" {

int thip_batch_grouping(int n_inst, int max_group, int *host_groups, int *host_members)
{
    if (n_inst < 1 || n_inst > THIP_BATCH_MAX || (max_group != 2 && max_group != 4 && max_group != 8) || !host_groups)
        return fail(THIP_E_INVALID, "bad argument", __FILE__, __LINE__);
    std::vector<std::pair<int, int>> g;
    batch_groups(n_inst, max_group, &g);
    *host_groups = (int)g.size();
    if (host_members) for (size_t i = 0; i < g.size(); ++i) host_members[i] = g[i].second;
    return 0;
}

int thip_batch_create(const thip_problem *prob_template, int n_inst, const float *const *host_vec_b, const float *const *host_vec_c,
                      const thip_param *par, thip_batch **out)
{
    if (!out) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *out = nullptr;
    THIP_NEED_INIT();
    if (!prob_template || !par || !host_vec_b || !host_vec_c) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (n_inst < 1 || n_inst > THIP_BATCH_MAX) return fail(THIP_E_INVALID, "a batch holds 1 .. 64 instances", __FILE__, __LINE__);
    if (!prob_template->mat_a && prob_template->m && prob_template->n)
        return fail(THIP_E_INVALID, "a batch streams a dense f32 A (sparse and 16-bit storage are not taken)", __FILE__, __LINE__);
    for (int i = 0; i < n_inst; ++i)
        if ((!host_vec_b[i] && prob_template->m) || (!host_vec_c[i] && prob_template->n))
            return fail(THIP_E_INVALID, "null b or c of an instance", __FILE__, __LINE__);
    if (prob_template->m && prob_template->n && !dense_f32(prob_template->mat_a, (prob_template->m + 15) / 16 * 16).vec_ok())
        return fail(THIP_E_INVALID, "mat_a must be 16-byte aligned", __FILE__, __LINE__);
    thip_batch *b = new thip_batch();
    const int rc = batch_create_impl(prob_template, n_inst, host_vec_b, host_vec_c, par, b);
    if (rc != 0) { thip_batch_destroy(b); return rc; }
    *out = b;
    return 0;
}

int thip_batch_set_a_storage(thip_batch *b, int a_kind)
{
    if (!b) return fail(THIP_E_INVALID, "null batch", __FILE__, __LINE__);
    if (a_kind != THIP_A_F32) return fail(THIP_E_INVALID, "a batch streams A in f32 only", __FILE__, __LINE__);
    return 0;
}

int thip_batch_set_gemv_autotune(thip_batch *b, int on)
{
    if (!b) return fail(THIP_E_INVALID, "null batch", __FILE__, __LINE__);
    b->autotune = on != 0;
    if (!on) for (GemvPlan &p : b->mplan) p.tuned = false;
    for (thip_solver *s : b->inst) THIP_RC(thip_solver_set_gemv_autotune(s, on));
    return 0;
}

int thip_batch_set_max_group(thip_batch *b, int max_group)
{
    if (!b || (max_group != 2 && max_group != 4 && max_group != 8)) return fail(THIP_E_INVALID, "the group size is 2, 4 or 8", __FILE__, __LINE__);
    if (b->inited) return fail(THIP_E_INVALID, "thip_batch_set_max_group comes before thip_batch_init", __FILE__, __LINE__);
    b->max_group = max_group;
    return 0;
}

int thip_batch_set_param(thip_batch *b, const thip_param *par)
{
    if (!b || !par) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    for (thip_solver *s : b->inst) THIP_RC(thip_solver_set_param(s, par));
    return 0;
}

int thip_batch_init(thip_batch *b)
{
    THIP_NEED_INIT();
    if (!b) return fail(THIP_E_INVALID, "null batch", __FILE__, __LINE__);
    hipStream_t st = ctx().stream;
    THIP_RC(batch_ensure_pad(b));
    for (thip_solver *s : b->inst) {
        if (!s->gemv_scr && b->scr_floats) {
            THIP_TRY(hipMalloc((void **)&s->gemv_scr, b->scr_floats * sizeof(float)));
            s->gemv_scr_n = b->scr_floats;
        }
        THIP_RC(init_reset(s));
        s->hst->iter = 0;            // (the host record is next written by a poll: thip_batch_counters reads it before that)
    }
    // the |A| row and column sums of the preconditioner: one pass for all instances
    if (b->m && b->n) THIP_RC(abs_sums(b->inst[0], b->rowabs, b->colabs));
    for (thip_solver *s : b->inst) {
        THIP_RC(init_norms_precond(s, b->rowabs, b->colabs));
        s->split_plan = false;
        s->inited = true;
    }
    const int B = (int)b->inst.size();
    std::vector<std::pair<int, int>> groups;
    batch_groups(B, b->max_group, &groups);
    if (b->regroup) {
        // every kernel instance the live set can come to be served by: NV = 2, 4, 8 as far as max_group and B reach, and the
        // single-vector plan -- timed once on instance 0 and handed to the others (the matrix is the same)
        for (int nv = 2; nv <= b->max_group; nv *= 2) {
            const int members = std::min(nv, B);
            if (members >= 2 && gemv_multi_instance(members) == nv) THIP_RC(autotune_multi(b, 0, members));
        }
        THIP_RC(autotune_gemv(b->inst[0]));
        for (thip_solver *s : b->inst) s->plan[0][0] = b->inst[0]->plan[0][0];
    } else {
        for (auto &g : groups) {
            if (g.second == 1) THIP_RC(autotune_gemv(b->inst[g.first]));
            else THIP_RC(autotune_multi(b, g.first, g.second));
        }
    }
    // the carried products gP = A^T x_y, hP = A x_x of the start iterate (what rebuild_carried does for one solver), a pass per group
    for (auto &g : groups) {
        GemvPartials gp[GEMV_MULTI_MAX];
        if (b->m == 0 || b->n == 0) break;
        THIP_RC(batch_products(b, g.first, g.second, 1, false, gp, batch_hint(b, g.second)));
        for (int j = 0; j < g.second; ++j) {
            thip_solver *s = b->inst[g.first + j];
            THIP_RC(finalize_partials(st, s->m, gp[j].partN, gp[j].nN, gp[j].strideN, 1.0f, 0.0f, s->hP, nullptr));
            THIP_RC(finalize_partials(st, s->n, gp[j].partT, gp[j].nT, gp[j].strideT, 1.0f, 0.0f, s->gP, nullptr));
        }
    }
    for (size_t i = 0; i < b->inst.size(); ++i) b->live[i] = 1;
    b->ctr = thip_batch_counters_t{};
    b->ctr.live = B;
    b->ctr.groups_now = (int32_t)groups.size();
    b->inited = true;
    return 0;
}

// thip_batch_run and thip_batch_run_until_any.  The launches of a pass: the groups fixed by index, each launched while a member is
// live (its stopped members are masked by their stop flags) -- or, regroup, the live instances packed anew after every poll
static int batch_run_impl(thip_batch *b, int64_t max_steps, int64_t poll_every, thip_status *host_status, bool until_any)
{
    THIP_NEED_INIT();
    if (!b || !b->inited) return fail(THIP_E_INVALID, "batch not initialised", __FILE__, __LINE__);
    if (poll_every <= 0) poll_every = 16;
    const int B = (int)b->inst.size();
    std::vector<int> members(B);
    std::vector<std::pair<int, int>> fixed, groups;      // (offset into members, size)
    batch_groups(B, b->max_group, &fixed);
    auto any_live = [&](int first, int n) {
        for (int j = 0; j < n; ++j) if (b->live[first + j]) return true;
        return false;
    };
    // after a poll: the launches of the next iterations, and what the counters say of the live set
    auto regroup = [&]() {
        if (b->regroup) {
            live_groups(B, b->max_group, b->live.data(), &members, &groups);
        } else {
            members.resize(B);
            for (int i = 0; i < B; ++i) members[i] = i;
            groups.clear();
            for (auto &g : fixed) if (any_live(g.first, g.second)) groups.push_back(g);      // every member stopped: skipped
        }
        int live = 0;
        for (int i = 0; i < B; ++i) live += b->live[i] != 0;
        b->ctr.live = live;
        b->ctr.groups_now = (int32_t)groups.size();
    };
    THIP_RC(batch_poll(b, host_status));
    regroup();
    const std::vector<char> was_live = b->live;
    auto one_stopped = [&]() {
        for (int i = 0; i < B; ++i) if (was_live[i] && !b->live[i]) return true;
        return false;
    };
    int64_t done = 0;
    while (any_live(0, B) && (max_steps < 0 || done < max_steps) && !(until_any && one_stopped())) {
        int64_t batch = poll_every;
        if (max_steps >= 0 && done + batch > max_steps) batch = max_steps - done;
        for (int64_t k = 0; k < batch; ++k) {
            prof_tick();
            for (int which = 0; which < 2; ++which)
                for (auto &g : groups) {
                    const int *idx = members.data() + g.first;
                    GemvPartials gp[GEMV_MULTI_MAX];
                    THIP_RC(batch_products(b, idx, g.second, which, true, gp, g.second > 1 ? batch_hint(b, g.second) : nullptr));
                    b->ctr.launches[counter_slot(g.second)] += 1;
                    b->ctr.passes += 1;
                    for (int j = 0; j < g.second; ++j) {
                        if (!b->live[idx[j]]) continue;        // (its kernels would return at entry)
                        THIP_RC(which == 0 ? stage_x_tail(b->inst[idx[j]], gp[j]) : stage_c_tail(b->inst[idx[j]], gp[j]));
                    }
                }
        }
        done += batch;
        THIP_RC(batch_poll(b, host_status));
        regroup();
    }
    return 0;
}

int thip_batch_run(thip_batch *b, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{
    return batch_run_impl(b, max_steps, poll_every, host_status, false);
}

int thip_batch_run_until_any(thip_batch *b, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{
    return batch_run_impl(b, max_steps, poll_every, host_status, true);
}

int thip_batch_set_regroup(thip_batch *b, int on)
{
    if (!b) return fail(THIP_E_INVALID, "null batch", __FILE__, __LINE__);
    if (b->inited) return fail(THIP_E_INVALID, "thip_batch_set_regroup comes before thip_batch_init", __FILE__, __LINE__);
    b->regroup = on != 0;
    return 0;
}

int thip_batch_replace(thip_batch *b, int i, const float *dev_vec_b, const float *dev_vec_c)
{
    THIP_NEED_INIT();
    if (!b || !b->inited) return fail(THIP_E_INVALID, "batch not initialised", __FILE__, __LINE__);
    if (i < 0 || (size_t)i >= b->inst.size()) return fail(THIP_E_INVALID, "no such instance", __FILE__, __LINE__);
    if ((!dev_vec_b && b->m) || (!dev_vec_c && b->n)) return fail(THIP_E_INVALID, "null b or c", __FILE__, __LINE__);
    thip_solver *s = b->inst[(size_t)i];
    THIP_RC(poll(s, nullptr));                  // the retired occupant's iteration count; nothing reads its b / c after this
    b->ctr.instance_iterations += s->hst->iter;
    b->ctr.replaced += 1;
    s->b = dev_vec_b; s->c = dev_vec_c;
    // what thip_batch_init does to an instance, from the shared |A| sums.  init_reset zeroes the whole arena: the iterate, the
    // Kahan terms, and gP / hP -- which are the carried products of the start iterate x = 0, y = 0 as they stand
    THIP_RC(init_reset(s));
    s->hst->iter = 0;
    THIP_RC(init_norms_precond(s, b->rowabs, b->colabs));
    s->split_plan = false;
    s->inited = true;
    if (!b->live[(size_t)i]) { b->live[(size_t)i] = 1; b->ctr.live += 1; }
    // (groups_now follows at the next poll, which every run begins with)
    return 0;
}

// slot i goes on from the given iterate (after thip_batch_init / _replace): what thip_solver_set_iterate does to one solver, on the
// slot's instance -- its carried products by ONE single-vector pass over A for that slot -- and the slot is live again
int thip_batch_set_iterate(thip_batch *b, int i, const float *host_x, const float *host_y)
{
    THIP_NEED_INIT();
    if (!b || !b->inited) return fail(THIP_E_INVALID, "batch not initialised", __FILE__, __LINE__);
    if (i < 0 || (size_t)i >= b->inst.size()) return fail(THIP_E_INVALID, "no such instance", __FILE__, __LINE__);
    long long retired = 0;                      // the iterations the slot had made count on, as a replaced occupant's do
    THIP_RC(solver_set_iterate(b->inst[(size_t)i], host_x, host_y, &retired));
    b->ctr.instance_iterations += retired;
    if (!b->live[(size_t)i]) { b->live[(size_t)i] = 1; b->ctr.live += 1; }
    return 0;
}

int thip_batch_live_grouping(int n_inst, int max_group, const int *host_live, int *host_groups, int *host_group_sizes, int *host_members)
{
    if (n_inst < 1 || n_inst > THIP_BATCH_MAX || (max_group != 2 && max_group != 4 && max_group != 8) || !host_live || !host_groups)
        return fail(THIP_E_INVALID, "bad argument", __FILE__, __LINE__);
    std::vector<char> live((size_t)n_inst);
    for (int i = 0; i < n_inst; ++i) live[(size_t)i] = host_live[i] != 0;
    std::vector<int> members;
    std::vector<std::pair<int, int>> g;
    live_groups(n_inst, max_group, live.data(), &members, &g);
    *host_groups = (int)g.size();
    if (host_group_sizes) for (size_t k = 0; k < g.size(); ++k) host_group_sizes[k] = g[k].second;
    if (host_members) for (size_t k = 0; k < members.size(); ++k) host_members[k] = members[k];
    return 0;
}

int thip_batch_counters(const thip_batch *b, thip_batch_counters_t *host)
{
    if (!b || !host) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *host = b->ctr;
    if (b->inited) for (const thip_solver *s : b->inst) host->instance_iterations += s->hst->iter;      // the current occupants, as of the last poll
    return 0;
}

static thip_solver *batch_member(thip_batch *b, int i)
{
    if (!b || i < 0 || (size_t)i >= b->inst.size()) { fail(THIP_E_INVALID, "no such instance", __FILE__, __LINE__); return nullptr; }
    return b->inst[(size_t)i];
}

int thip_batch_status(thip_batch *b, int i, thip_status *host_status)
{
    thip_solver *s = batch_member(b, i);
    return s ? thip_solver_status(s, host_status) : THIP_E_INVALID;
}

int thip_batch_solution(thip_batch *b, int i, float *host_x, float *host_y)
{
    thip_solver *s = batch_member(b, i);
    return s ? thip_solver_solution(s, host_x, host_y) : THIP_E_INVALID;
}

int thip_batch_iterate(thip_batch *b, int i, float *host_x, float *host_y)
{
    thip_solver *s = batch_member(b, i);
    return s ? thip_solver_iterate(s, host_x, host_y) : THIP_E_INVALID;
}

int thip_batch_precond(thip_batch *b, int i, float *host_dp_tau, float *host_dp_sigma)
{
    thip_solver *s = batch_member(b, i);
    return s ? thip_solver_precond(s, host_dp_tau, host_dp_sigma) : THIP_E_INVALID;
}

int thip_batch_info(const thip_batch *b, thip_batch_info_t *host_info)
{
    if (!b || !host_info) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    thip_batch_info_t &o = *host_info;
    memset(&o, 0, sizeof(o));
    o.n_inst = (int32_t)b->inst.size();
    o.max_group = b->max_group;
    o.a_copies = b->pad ? 1 : 0;
    o.a_bytes = b->pad ? b->ldpad * b->n * sizeof(float) : 0;
    std::vector<std::pair<int, int>> groups;
    batch_groups((int)b->inst.size(), b->max_group, &groups);
    o.groups = (int32_t)groups.size();
    o.passes_per_iteration = 2 * o.groups;
    o.bytes_per_pass = b->m * b->n * sizeof(float);
    size_t dev = o.a_bytes + (b->rowabs ? b->m * sizeof(float) : 0) + (b->colabs ? b->n * sizeof(float) : 0);
    for (const thip_solver *s : b->inst) {
        o.arena_bytes += s->arena_n * sizeof(float);
        dev += s->arena_n * sizeof(float) + s->gemv_scr_n * sizeof(float) + (4 * PG + 4 * EG) * sizeof(float) + (s->m ? s->m : 1)
               + s->psd_worklen * sizeof(float) + sizeof(DevStatus);
    }
    o.device_bytes = dev;
    for (int q = 1; q < 4; ++q) {
        o.plan_nj[q] = b->mplan[q].tuned ? b->mplan[q].hint.nj : 0;
        o.plan_blocks[q] = b->mplan[q].tuned ? b->mplan[q].hint.target_blocks : 0;
        o.plan_ms[q] = b->mplan[q].ms;
    }
    return 0;
}

// TEST HOOK (totsu_f32hip_test.h): a candidate tiling of one kernel instance installed the way autotune_multi installs its pick
int thip_test_batch_pin_multi_plan(thip_batch *b, int instance, int candidate_index)
{
    int nc = 0;
    const GemvHint *c = gemv_multi_candidates(&nc);
    if (!b || !b->inited || !(instance == 2 || instance == 4 || instance == 8) || candidate_index < -1 || candidate_index >= nc)
        return fail(THIP_E_INVALID, "null or uninitialised batch, or no such instance or candidate plan", __FILE__, __LINE__);
    if (candidate_index >= 0 && instance == 8 && c[candidate_index].nj != 1)
        return fail(THIP_E_INVALID, "the NV = 8 instance holds one row group per lane: the autotune never picks this plan", __FILE__, __LINE__);
    b->mplan[plan_slot(instance)] = candidate_index < 0 ? GemvPlan{} : GemvPlan{ c[candidate_index], true, 0.0f };
    return 0;
}

// TEST HOOK (totsu_f32hip_test.h): the plan of the latest multi-vector launch of one kernel instance (zeros: none yet)
int thip_test_batch_last_multi_plan(const thip_batch *b, int instance, thip_gemv_plan_rec *host_plan)
{
    if (!b || !host_plan || !(instance == 2 || instance == 4 || instance == 8))
        return fail(THIP_E_INVALID, "null argument or no such instance", __FILE__, __LINE__);
    *host_plan = b->last_mplan[plan_slot(instance)];
    return 0;
}

int thip_batch_destroy(thip_batch *b)
{
    if (!b) return 0;
    if (ctx().inited) hipStreamSynchronize(ctx().stream);
    for (thip_solver *s : b->inst) {
        s->sa.pad = nullptr; s->sa.ldpad = 0;          // the padded copy was borrowed
        thip_solver_destroy(s);
    }
    hipFree(b->pad); hipFree(b->rowabs); hipFree(b->colabs);
    delete b;
    return 0;
}

}  // extern "C"
