// thip_solver_api.inc -- part of thip_solver.hip: the extern "C" entry points (thip_solver_*, thip_prof_*).

extern "C" {

static int solver_create_impl(const thip_problem *prob, const thip_param *par, int schedule, thip_solver **out)
{
    THIP_NEED_INIT();
    if (!prob || !par || !out) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (schedule < 0 || schedule > THIP_SCHED_SWEEP) return fail(THIP_E_INVALID, "bad schedule", __FILE__, __LINE__);
    int64_t tot = 0;
    for (size_t i = 0; i < prob->n_seg; ++i) {
        if (prob->host_seg_len[i] < 0 || prob->host_seg_type[i] < 0 || prob->host_seg_type[i] > THIP_CONE_PSD)
            return fail(THIP_E_INVALID, "bad cone segment", __FILE__, __LINE__);
        tot += prob->host_seg_len[i];
    }
    if ((size_t)tot != prob->m) return fail(THIP_E_INVALID, "cone segments do not cover m rows", __FILE__, __LINE__);

    thip_solver *s = new thip_solver();
    *out = s;                      // the caller releases it if anything below fails
    s->n = prob->n; s->m = prob->m;
    s->sa.f32 = prob->mat_a; s->sa.m = prob->m; s->b = prob->vec_b; s->c = prob->vec_c; s->b_rowabs = prob->vec_b_rowabs;
    s->par = *par; s->schedule = schedule;
    s->seg_type.assign(prob->host_seg_type, prob->host_seg_type + prob->n_seg);
    s->seg_len.assign(prob->host_seg_len, prob->host_seg_len + prob->n_seg);
    hipStream_t st = ctx().stream;
    const size_t n = s->n, m = s->m;

    // ---- cone tables ----
    std::vector<unsigned char> cls(m ? m : 1, 2);
    std::vector<int64_t> sb, se, rb, re, gb, ge;
    int64_t off = 0;
    size_t psd_kmax = 0;
    for (size_t i = 0; i < s->seg_type.size(); ++i) {
        const int64_t l = s->seg_len[i];
        switch (s->seg_type[i]) {
        case THIP_CONE_ZERO: for (int64_t r = 0; r < l; ++r) cls[off + r] = 0; break;
        case THIP_CONE_RPOS: for (int64_t r = 0; r < l; ++r) cls[off + r] = 1; break;
        case THIP_CONE_SOC:
            sb.push_back(off); se.push_back(off + l); gb.push_back(off); ge.push_back(off + l);
            if ((size_t)l > s->soc_max) s->soc_max = (size_t)l;
            break;
        case THIP_CONE_ROTSOC:
            rb.push_back(off); re.push_back(off + l); gb.push_back(off); ge.push_back(off + l);
            if ((size_t)l > s->rot_max) s->rot_max = (size_t)l;
            break;
        case THIP_CONE_PSD: {
            const size_t k = (size_t)((std::sqrt((double)(8 * l + 1)) - 1.0) / 2.0 + 0.5);
            if ((int64_t)(k * (k + 1) / 2) != l) { return fail(THIP_E_INVALID, "PSD segment is not triangular", __FILE__, __LINE__); }
            s->psd.push_back({off, l});
            for (int64_t r = 0; r < l; ++r) cls[off + r] = 3;
            gb.push_back(off); ge.push_back(off + l);
            if (k > psd_kmax) psd_kmax = k;
            break; }
        }
        if ((size_t)l > s->grp_max && s->seg_type[i] >= THIP_CONE_SOC) s->grp_max = (size_t)l;
        off += l;
    }
    s->n_soc = sb.size(); s->n_rot = rb.size(); s->n_grp = gb.size();
    {
        int64_t soc_rows = 0;
        for (size_t i = 0; i < sb.size(); ++i) soc_rows += se[i] - sb[i];
        s->all_soc_short = m > 0 && !sb.empty() && rb.empty() && (size_t)soc_rows == m && s->soc_max <= 129;
    }
    auto up64 = [&](const std::vector<int64_t> &h, int64_t **d) -> int {
        *d = nullptr;
        if (h.empty()) return 0;
        THIP_TRY(hipMalloc((void **)d, h.size() * sizeof(int64_t)));
        THIP_TRY(hipMemcpy(*d, h.data(), h.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        return 0;
    };
    THIP_RC(up64(sb, &s->soc_beg)); THIP_RC(up64(se, &s->soc_end));
    THIP_RC(up64(rb, &s->rot_beg)); THIP_RC(up64(re, &s->rot_end));
    THIP_RC(up64(gb, &s->grp_beg)); THIP_RC(up64(ge, &s->grp_end));
    THIP_TRY(hipMalloc((void **)&s->cls, cls.size()));
    THIP_TRY(hipMemcpy(s->cls, cls.data(), cls.size(), hipMemcpyHostToDevice));
    {
        std::map<size_t, std::vector<int64_t>> by_order;
        for (auto &pr : s->psd) {
            const size_t k = (size_t)((std::sqrt((double)(8 * pr.second + 1)) - 1.0) / 2.0 + 0.5);
            if (k <= psd_small_max()) by_order[k].push_back(pr.first);
        }
        for (auto &kv : by_order) {
            thip_solver::PsdGroup g{ kv.first, (int)kv.second.size(), nullptr };
            THIP_RC(up64(kv.second, &g.dev_offs));
            s->psd_groups.push_back(g);
        }
    }
    if (psd_kmax) {
        s->psd_worklen = 2 * thip_map_eig_worklen(psd_kmax);
        THIP_TRY(hipMalloc((void **)&s->psd_work, s->psd_worklen * sizeof(float)));
    }

    // ---- vectors ----
    const size_t pn = pad64(n + TAIL), pm = pad64(m + 1);
    if (par->state_arith != THIP_STATE_COMPENSATED && par->state_arith != THIP_STATE_PLAIN)
        return fail(THIP_E_INVALID, "bad thip_param.state_arith", __FILE__, __LINE__);
    const size_t total = 10 * pn /* xx u Tx Su rxx g1 g2 g3 gP xx2 */ + 13 * pm + 64 + 3 * pn + 3 * pm /* Kahan terms */;
    THIP_TRY(hipMalloc((void **)&s->arena, total * sizeof(float)));
    THIP_TRY(hipMemsetAsync(s->arena, 0, total * sizeof(float), st));
    s->arena_n = total;
    float *p = s->arena;
    auto take = [&](size_t k) { float *r = p; p += k; return r; };
    s->xx = take(pn); s->u = take(pn); s->Tx = take(pn); s->Su = take(pn); s->rxx = take(pn);
    s->g1 = take(pn); s->g2 = take(pn); s->g3 = take(pn); s->gP = take(pn); s->xx2 = take(pn);
    s->xy = take(pm); s->xs = take(pm); s->v = take(pm); s->Ty = take(pm); s->Ts = take(pm); s->Sv = take(pm);
    s->rxy = take(pm); s->rxs = take(pm); s->h1 = take(pm); s->h2 = take(pm); s->h3 = take(pm); s->hP = take(pm);
    (void)take(pm);
    s->dotc = take(64);
    s->kx = take(pn); s->ku = take(pn); s->ky = take(pm); s->ks = take(pm); s->kv = take(pm); s->kx2 = take(pn);
    s->kahan_n = 3 * pn + 3 * pm;
    s->xx_home = s->xx; s->kx_home = s->kx;
    s->pn_len = pn; s->pm_len = pm;
    THIP_TRY(hipHostMalloc((void **)&s->hflags, 8 * sizeof(unsigned), hipHostMallocDefault));

    THIP_TRY(hipMalloc((void **)&s->part, (4 * PG + 4 * EG) * sizeof(float)));
    // the dense GEMV partial-sum scratch (~ m n / 256 floats) is allocated by thip_solver_init, and only for a dense A
    // (thip_solver_set_csr comes between create and init: a sparse 1e6 x 1e6 operator must not pay 15 GB for it)
    THIP_TRY(hipMalloc((void **)&s->dst, sizeof(DevStatus)));
    THIP_TRY(hipMemsetAsync(s->dst, 0, sizeof(DevStatus), st));
    THIP_TRY(hipHostMalloc((void **)&s->hst, sizeof(DevStatus), hipHostMallocDefault));
    return 0;
}

int thip_solver_create(const thip_problem *prob, const thip_param *par, int schedule, thip_solver **out)
{
    if (!out) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *out = nullptr;
    thip_solver *s = nullptr;
    const int rc = solver_create_impl(prob, par, schedule, &s);
    if (rc != 0) {
        if (s) thip_solver_destroy(s);      // partial device allocations (e.g. out of memory half-way)
        return rc;
    }
    *out = s;
    return 0;
}

int thip_solver_set_csr(thip_solver *s, size_t nnz, const int64_t *dev_rowptr, const int32_t *dev_colidx,
                        const float *dev_vals, const int64_t *dev_t_rowptr, const int32_t *dev_t_colidx,
                        const float *dev_t_vals)
{
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    if (!dev_rowptr || !dev_t_rowptr) return fail(THIP_E_INVALID, "null CSR arrays", __FILE__, __LINE__);
    if (s->op != A_TILED) s->op = A_CSR2;      // (a tiled copy, once given, is the operator)
    s->csr = Csr2{ nnz, dev_rowptr, dev_t_rowptr, dev_colidx, dev_t_colidx, dev_vals, dev_t_vals };
    return 0;
}

int thip_solver_set_sptile(thip_solver *s, thip_sptile *mat)
{
    if (!s || !mat) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (s->inited) return fail(THIP_E_INVALID, "thip_solver_set_sptile comes before thip_solver_init", __FILE__, __LINE__);
    size_t m = 0, n = 0, nnz = 0;
    sptile_dims(mat, &m, &n, &nnz);
    if (m != s->m || n != s->n) return fail(THIP_E_INVALID, "the sparse operator's shape is not the problem's m x n", __FILE__, __LINE__);
    s->op = A_TILED; s->spt = mat;
    return 0;
}

int thip_solver_set_allreduce(thip_solver *s, thip_allreduce_fn fn, void *c)
{
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    s->allreduce = fn; s->allreduce_ctx = c;
    return 0;
}

int thip_solver_set_overlap(thip_solver *s, int on)
{
    THIP_NEED_INIT();
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    if (on < 0 || on > 3) return fail(THIP_E_INVALID, "overlap mode is 0 .. 3", __FILE__, __LINE__);
    if (on && !s->side) {
        THIP_TRY(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));
        THIP_TRY(hipEventCreateWithFlags(&s->ev_in, hipEventDisableTiming));
        THIP_TRY(hipEventCreateWithFlags(&s->ev_out, hipEventDisableTiming));
        for (int k = 0; k < 4; ++k) {
            THIP_TRY(hipEventCreateWithFlags(&s->sev_in[k], hipEventDisableTiming));
            THIP_TRY(hipEventCreateWithFlags(&s->sev_out[k], hipEventDisableTiming));
        }
    }
    if (s->side && ctx().inited) THIP_TRY(hipStreamSynchronize(s->side));
    if (on == 2 && !s->gflags) {
        // THIP_PIPE_GATES=0: cross-stream events instead of the device-flag hand-offs
        static const int gates_on = getenv("THIP_PIPE_GATES") ? atoi(getenv("THIP_PIPE_GATES")) : 1;
        THIP_TRY(hipExtMallocWithFlags((void **)&s->gflags, 16 * sizeof(unsigned), hipDeviceMallocUncached));
        THIP_TRY(hipMemset(s->gflags, 0, 16 * sizeof(unsigned)));
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx().device) != hipSuccess || khz <= 0) khz = 100000;
        s->gate_ticks = (long long)khz * 2000ll;
        s->use_gates = gates_on != 0;
    }
    s->overlap = on;
    return 0;
}

// thip_solver_init in its parts, so that a batch of solvers sharing A (thip_solver_batch.inc) initialises its instances with the same
// launches.  The per-solve host state and init_vecs (solver.rs:483-494): x = 0, y = 0, tau = 1
static int init_reset(thip_solver *s)
{
    hipStream_t st = ctx().stream;
    // per-solve host state: a solver may be initialised again after a solve that terminated
    s->finalized = false;
    s->carried_stale = false;
    s->hst->state = THIP_ST_RUNNING;
    s->xx = s->xx_home; s->kx = s->kx_home; s->xbuf = 0;
    s->sw_first = true; s->sweep_state = 0; s->pn_par = 0; s->status_pending = false; s->step_par = 0; s->pm_par = 0;
    s->sweep_faults = 0; s->sweep_fault_word = 0; s->sweep_fault_iter = -1; s->snap_iter = -1;
    // init_vecs (solver.rs:483-494): x = 0, y = 0, tau = 1
    THIP_TRY(hipMemsetAsync(s->arena, 0, s->arena_n * sizeof(float), st));
    hipLaunchKernelGGL(init_status_k, dim3(1), dim3(1), 0, st, s->dst, 0.0f);
    return 0;
}

static int init_norms_precond(thip_solver *s, const float *shared_rowabs, const float *shared_colabs);

int thip_solver_init(thip_solver *s)
{
    THIP_NEED_INIT();
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    hipStream_t st = ctx().stream;
    THIP_RC(ensure_gemv_scratch(s));
    if (!s->sa.is16()) THIP_RC(ensure_apad(s, true));      // a fresh solve re-reads the caller's A (it may have changed in place)
    THIP_RC(init_reset(s));
    THIP_RC(sweep_prepare(s));        // (its plan autotune runs idempotent sweeps: after the stop flag has been cleared)
    if (s->sw_part) THIP_TRY(hipMemsetAsync(s->sw_part, 0, 12 * EG * sizeof(float), st));
    THIP_TRY(hipMemsetAsync(s->arena, 0, s->arena_n * sizeof(float), st));
    THIP_RC(init_norms_precond(s, nullptr, nullptr));
    s->split_plan = false;           // the one-launch form here; the column-split form is tuned by the first run that uses it
    if (!sweep_active(s)) THIP_RC(autotune_gemv(s));      // (a run that falls back to the dual GEMV tunes it then: prepare_split)
    s->inited = true;
    return 0;
}

// calc_norms and calc_precond (solver.rs:460-481, 496-524).  shared_rowabs / shared_colabs != NULL: the |A| row and column sums as
// finished vectors computed elsewhere (a batch: once for all its instances) instead of by a pass of this solver's own
static int init_norms_precond(thip_solver *s, const float *shared_rowabs, const float *shared_colabs)
{
    hipStream_t st = ctx().stream;
    const size_t n = s->n, m = s->m;
    const unsigned g = egrid(n > m ? n : m);
    // calc_norms (solver.rs:460-481) + scalar parts of abssum (solver.rs:171-172)
    hipLaunchKernelGGL(init_sums_k, dim3(g), dim3(BLK), 0, st, (int)m, s->b, (int)n, s->c, s->part);
    float *sums = s->g1 + n;        // [0] sum b^2, [1] sum |b|  (sharded -> all-reduce)
    float *loc = s->dotc + 8;       // [0] sum c^2, [1] sum |c|
    hipLaunchKernelGGL(sum_partials_k, dim3(1), dim3(BLK), 0, st, 2, (int)g, s->part, sums, (const int *)nullptr);
    hipLaunchKernelGGL(sum_partials_k, dim3(1), dim3(BLK), 0, st, 2, (int)g, s->part + 2 * g, loc, (const int *)nullptr);

    // |A| column sums (sharded partial -> all-reduce with the two scalars in the tail) and row sums
    const float *colabs = s->g1, *rowabs = s->h1;
    if (shared_rowabs && shared_colabs) { rowabs = shared_rowabs; colabs = shared_colabs; }
    else THIP_RC(abs_sums(s, s->h1, s->g1));
    if (s->col_shard) {
        // this rank holds a block of columns: b and the m-vectors are replicated, c is its block.  What the ranks have to
        // add up is the |A| row sums and sum c^2, sum |c| (the b sums and the column sums are complete as they are)
        if (!sweep_active(s))
            return fail(THIP_E_INVALID, "a column-sharded run needs THIP_SCHED_SWEEP and a shape its kernel takes", __FILE__, __LINE__);
        if (s->cs_n < m + 2) return fail(THIP_E_INVALID, "column-shard buffer too small", __FILE__, __LINE__);
        THIP_TRY(hipMemcpyAsync(s->cs_buf, rowabs, m * sizeof(float), hipMemcpyDeviceToDevice, st));
        THIP_TRY(hipMemcpyAsync(s->cs_buf + m, loc, 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
        THIP_RC(do_allreduce(s, s->cs_buf, s->cs_n));
        THIP_TRY(hipMemcpyAsync(s->h1, s->cs_buf, m * sizeof(float), hipMemcpyDeviceToDevice, st));
        THIP_TRY(hipMemcpyAsync(loc, s->cs_buf + m, 2 * sizeof(float), hipMemcpyDeviceToDevice, st));
        THIP_TRY(hipMemsetAsync(s->cs_buf, 0, s->cs_n * sizeof(float), st));
    } else {
        THIP_RC(do_allreduce(s, s->g1, n + 2));
    }
    hipLaunchKernelGGL(init_scalars_k, dim3(1), dim3(1), 0, st, sums, loc, s->par.eps_zero, s->dst);
    hipLaunchKernelGGL(precond_k, dim3(g), dim3(BLK), 0, st, (int)n, (int)m, colabs, rowabs, s->c, s->b, s->b_rowabs,
                       s->par.eps_zero, s->Tx, s->Ty, s->Ts, s->Su, s->Sv);
    // product_group (solver.rs:521-523): per block cone, dp_tau's x_y and x_s parts <- their minimum
    THIP_RC(group_min_batched(st, s->Ty, s->grp_beg, s->grp_end, s->n_grp, s->grp_max));
    THIP_RC(group_min_batched(st, s->Ts, s->grp_beg, s->grp_end, s->n_grp, s->grp_max));
    // scratch vectors used above must read as zero again for the carried products (A x_0 = 0)
    THIP_TRY(hipMemsetAsync(s->g1, 0, (n + TAIL) * sizeof(float), st));
    THIP_TRY(hipMemsetAsync(s->h1, 0, (m ? m : 1) * sizeof(float), st));
    THIP_LAUNCH_CHECK();
    return 0;
}

// A column shard whose (re-)plan of the one-pass kernel failed on THIS rank (thip_solver_set_a_storage / _set_sweep_min_bytes
// re-plan inside run(); the 16-bit plan rejecting the shape, a timing sweep raising the error word, a placement census that
// changed): there is no 2-pass form over a column block, and the peers are already sweeping -- their next batch holds one
// all-reduce per iteration (+ one when it starts from a consistent iterate).  This rank takes part in exactly those
// collectives with its fault flag raised (the tail slot every rank's termination test reads), for the three attempts the
// peers make from their snapshot, so that every rank of the run returns THIP_E_TIMEOUT at the same batch instead of one
// rank iterating a row-sharded schedule on a column block while the others wait in a collective of another size.
static int col_shard_abort(thip_solver *s, int64_t max_steps, int64_t poll_every)
{
    hipStream_t st = ctx().stream;
    const size_t mpad = pad64(s->m);                  // SweepGeom::mpad of every plan of this m (rows round to 4 or 8, mpad to 64)
    const size_t need = cs_floats(mpad);
    if (s->cs_n != need) {
        if (s->cs_buf) { THIP_TRY(hipStreamSynchronize(st)); THIP_TRY(hipFree(s->cs_buf)); s->cs_buf = nullptr; }
        THIP_TRY(hipMalloc((void **)&s->cs_buf, need * sizeof(float)));
        s->cs_n = need;
    }
    int64_t batch = poll_every;
    if (max_steps >= 0 && batch > max_steps) batch = max_steps;
    const float one = 1.0f;
    bool first = s->sw_first;
    for (int attempt = 0; attempt < COL_SHARD_ATTEMPTS; ++attempt) {
        const int64_t calls = batch + (first ? 1 : 0);
        for (int64_t k = 0; k < calls; ++k) {
            THIP_TRY(hipMemsetAsync(s->cs_buf, 0, need * sizeof(float), st));
            THIP_TRY(hipMemcpyAsync(s->cs_buf + cs_flag_slot(mpad), &one, sizeof(float), hipMemcpyHostToDevice, st));
            THIP_RC(do_allreduce(s, s->cs_buf, s->cs_n));
        }
        THIP_TRY(hipStreamSynchronize(st));
        first = true;                                 // the peers restore their snapshot: a consistent iterate
    }
    s->sweep_faults += 1;
    s->sweep_fault_word = 5u;                         // 5: this rank could not plan the kernel at all
    return fail(THIP_E_TIMEOUT, "the one-pass kernel could not be planned on this rank of a column-sharded run: every rank stops", __FILE__, __LINE__);
}

int thip_solver_run(thip_solver *s, int64_t max_steps, int64_t poll_every, thip_status *host_status)
{
    THIP_NEED_INIT();
    if (!s || !s->inited) return fail(THIP_E_INVALID, "solver not initialised", __FILE__, __LINE__);
    if (poll_every <= 0) poll_every = 16;
    int64_t done = 0;
    THIP_RC(poll(s, host_status));
    if (s->carried_stale && s->hst->state == THIP_ST_RUNNING) THIP_RC(rebuild_carried(s));
    THIP_RC(sweep_prepare(s));
    bool sweep = sweep_active(s);
    if (s->col_shard && !sweep) {
        // a column shard that was never going to sweep is a caller's mistake, not a fault to be raised through collectives
        // (without a hook do_allreduce is a no-op: the "abort" would spin through dummy calls and report a time-out)
        if (s->allreduce == nullptr) return fail(THIP_E_INVALID, "a column-sharded solver needs an all-reduce (thip_solver_set_allreduce / _use_rccl / _use_oneshot)", __FILE__, __LINE__);
        if (s->schedule != THIP_SCHED_SWEEP) return fail(THIP_E_INVALID, "a column-sharded solver runs THIP_SCHED_SWEEP only", __FILE__, __LINE__);
        if (s->op != A_DENSE) return fail(THIP_E_INVALID, "column shards are for a dense A", __FILE__, __LINE__);
        if (s->hst->state != THIP_ST_RUNNING || max_steps == 0) return 0;      // nothing would run on any rank
        return col_shard_abort(s, max_steps, poll_every);
    }
    THIP_RC(prepare_split(s));
    bool split = split_active(s);
    if (!sweep) s->sw_first = true;         // whatever runs instead leaves a consistent iterate and gP / hP of it
    if (sweep && s->hst->state == THIP_ST_RUNNING) THIP_RC(snapshot(s, false));      // the iterate this run starts from
    int retries = 0;
    while (s->hst->state == THIP_ST_RUNNING && (max_steps < 0 || done < max_steps)) {
        int64_t batch = poll_every;
        if (max_steps >= 0 && done + batch > max_steps) batch = max_steps - done;
        for (int64_t k = 0; k < batch; ++k) {
            prof_tick();
            THIP_RC(sweep ? one_iteration_sweep(s, k + 1 == batch) : (split ? one_iteration_split(s) : one_iteration(s)));
        }
        if (s->tail_pending) THIP_RC(split_tail(s));       // drain the pipeline before the host looks
        // every bounded device-side wait of the batch: did one run out?
        unsigned sw_err = 0, peer_fault = 0;
        THIP_RC(batch_faults(s, sweep, &sw_err, &peer_fault));
        // column-sharded: the verdict is the all-reduced one, so that every rank takes the same branch at the same batch
        if (sweep && (s->col_shard ? peer_fault != 0u : sw_err != 0u)) {
            s->sweep_faults += 1;
            s->sweep_fault_word = sw_err != 0u ? sw_err : 4u;       // 4: a peer rank's kernel
            s->sweep_fault_iter = s->snap_iter;
            THIP_RC(snapshot(s, true));                            // back to the last batch that completed
            if (s->col_shard) {
                // a column shard has no 2-pass form to fall back to: every rank restores and retries together (a transient --
                // another process on the GPU for a moment -- passes; a placement that stays wrong fails cleanly everywhere)
                if (++retries > COL_SHARD_ATTEMPTS - 1)
                    return fail(THIP_E_TIMEOUT, "the one-pass kernel gave up on some rank of a column-sharded run (3 attempts from the same iterate)", __FILE__, __LINE__);
                THIP_RC(sweep_rearm(s));
            } else if (++retries <= 1 && s->sweep_faults < 3) {
                // (at most three faults per solve: a disturbance that keeps coming back costs a ~2 s spin-out and a re-run batch
                // each time -- from the third on the rest of the solve runs the 2-pass schedule)
                // one GPU: a transient (another process on the device for a moment) should not halve the rate of the 100 000
                // iterations that may follow -- clean census, ring and error word and give the one-pass schedule ONE more batch
                // from the restored iterate before giving it up
                THIP_RC(sweep_rearm(s));
            } else {
                s->sweep_state = -1;                               // for the rest of this solve: the 2-pass schedule
                THIP_RC(prepare_split(s));                         // (tunes the GEMV plan if that has not happened yet)
                split = split_active(s);
                THIP_RC(rebuild_carried(s));
                sweep = false;
            }
            continue;                                              // the batch is run again (done has not moved)
        }
        retries = 0;
        done += batch;
        THIP_RC(poll(s, host_status));
        if (sweep && s->hst->state == THIP_ST_RUNNING) THIP_RC(snapshot(s, false));
    }
    return 0;
}

int thip_solver_status(thip_solver *s, thip_status *host_status)
{
    THIP_NEED_INIT();
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    return poll(s, host_status);
}

int thip_solver_solution(thip_solver *s, float *host_x, float *host_y)
{
    THIP_NEED_INIT();
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    THIP_RC(poll(s, nullptr));           // a terminated iterate gets its final scaling before it is read
    if (host_x) THIP_RC(thip_d2h(host_x, s->xx, s->n));
    if (host_y) THIP_RC(thip_d2h(host_y, s->xy, s->m));
    return 0;
}

int thip_solver_iterate(thip_solver *s, float *host_x, float *host_y)
{
    THIP_NEED_INIT();
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    const size_t n = s->n, m = s->m;
    THIP_RC(poll(s, nullptr));
    if (host_x) {
        THIP_RC(thip_d2h(host_x, s->xx, n));
        THIP_RC(thip_d2h(host_x + n, s->xy, m));
        THIP_RC(thip_d2h(host_x + n + m, s->xs, m));
        host_x[n + m + m] = s->hst->tau;
    }
    if (host_y) {
        THIP_RC(thip_d2h(host_y, s->u, n));
        THIP_RC(thip_d2h(host_y + n, s->v, m));
        host_y[n + m] = s->hst->kappa;
    }
    return 0;
}

// thip_solver_set_iterate / thip_batch_set_iterate: the solver goes on from the given iterate instead of x = 0, y = 0, tau = 1.  What
// snapshot(s, true) restores is the list: x_x (into whichever buffer is the iterate's now), u, x_y x_s v, the Kahan terms (zero: a
// start hands none over), the status block, and hP -- with gP, by one pass over the stored form of A now in use (rebuild_carried)
// (*retired: the iteration count the solver had reached, which the start resets)
static int solver_set_iterate(thip_solver *s, const float *host_x, const float *host_y, long long *retired = nullptr)
{
    THIP_NEED_INIT();
    if (!s || !s->inited) return fail(THIP_E_INVALID, "solver not initialised", __FILE__, __LINE__);
    if (!host_x || !host_y) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (s->allreduce != nullptr || s->col_shard)
        return fail(THIP_E_INVALID, "a start iterate is for one GPU: not with an all-reduce or a column shard", __FILE__, __LINE__);
    const size_t n = s->n, m = s->m;
    const float tau = host_x[n + 2 * m], kappa = host_y[n + m];
    if (!(tau >= 0.0f) || tau - tau != 0.0f) return fail(THIP_E_INVALID, "a start's tau is finite and not negative", __FILE__, __LINE__);
    if (!(kappa <= 0.0f) || kappa - kappa != 0.0f) return fail(THIP_E_INVALID, "a start's kappa is finite and not positive", __FILE__, __LINE__);
    hipStream_t st = ctx().stream;
    THIP_RC(poll(s, nullptr));                   // (synchronises; the host copy of the status block, whose constant part stays)
    if (retired) *retired = s->hst->iter;
    THIP_RC(thip_h2d(s->xx, host_x, n));
    THIP_RC(thip_h2d(s->xy, host_x + n, m));
    THIP_RC(thip_h2d(s->xs, host_x + n + m, m));
    THIP_RC(thip_h2d(s->u, host_y, n));
    THIP_RC(thip_h2d(s->v, host_y + n, m));
    THIP_TRY(hipMemsetAsync(s->kx_home, 0, s->kahan_n * sizeof(float), st));     // (kx ku ky ks kv and the sweep's kx2)
    DevStatus d = *s->hst;
    d.stop = 0; d.state = THIP_ST_RUNNING; d.kind = 0; d.xbuf = s->xbuf; d.iter = 0; d.fault = 0;
    d.cri[0] = d.cri[1] = d.cri[2] = 0.0f;
    d.tau = tau; d.kappa = kappa; d.r_tau = 0.0f;
    *s->hst = d;
    THIP_TRY(hipMemcpyAsync(s->dst, s->hst, sizeof(DevStatus), hipMemcpyHostToDevice, st));
    THIP_TRY(hipStreamSynchronize(st));
    s->finalized = false;
    s->status_pending = false;
    s->sw_first = true;                          // the given iterate is a consistent one: the next sweep step starts from it
    s->snap_iter = -1;
    THIP_RC(rebuild_carried(s));
    THIP_TRY(hipStreamSynchronize(st));          // (the host arrays are the caller's, and so is the moment the start has landed)
    return 0;
}

int thip_solver_set_iterate(thip_solver *s, const float *host_x, const float *host_y) { return solver_set_iterate(s, host_x, host_y); }

int thip_solver_precond(thip_solver *s, float *host_dp_tau, float *host_dp_sigma)
{
    THIP_NEED_INIT();
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    const size_t n = s->n, m = s->m;
    THIP_RC(poll(s, nullptr));
    if (host_dp_tau) {
        THIP_RC(thip_d2h(host_dp_tau, s->Tx, n));
        THIP_RC(thip_d2h(host_dp_tau + n, s->Ty, m));
        THIP_RC(thip_d2h(host_dp_tau + n + m, s->Ts, m));
        host_dp_tau[n + m + m] = s->hst->t_tau;
    }
    if (host_dp_sigma) {
        THIP_RC(thip_d2h(host_dp_sigma, s->Su, n));
        THIP_RC(thip_d2h(host_dp_sigma + n, s->Sv, m));
        host_dp_sigma[n + m] = s->hst->s_kappa;
    }
    return 0;
}

static int set_a16_external(thip_solver *s, const uint16_t *mat16, size_t ld16, int kind, const float *inv_scale)
{
    THIP_NEED_INIT();
    if (!s || !mat16) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (s->inited) return fail(THIP_E_INVALID, "a caller-built 16-bit matrix must precede thip_solver_init", __FILE__, __LINE__);
    if (s->op != A_DENSE) return fail(THIP_E_INVALID, "storage kinds apply to a dense A", __FILE__, __LINE__);
    if (ld16 < s->m) return fail(THIP_E_INVALID, "ld16 < m", __FILE__, __LINE__);
    if (kind == THIP_A_F16 && !inv_scale) return fail(THIP_E_INVALID, "f16 storage needs the per-column scales", __FILE__, __LINE__);
    StoredA &sa = s->sa;
    THIP_TRY(sa.free16());
    sa.a16 = const_cast<uint16_t *>(mat16);      // caller-owned, only ever read
    sa.inv_s = const_cast<float *>(inv_scale);
    sa.ld16 = ld16;
    sa.kind = sa.kind16 = kind;
    return 0;
}

int thip_solver_set_a_bf16(thip_solver *s, const uint16_t *mat16, size_t ld16)
{
    return set_a16_external(s, mat16, ld16, THIP_A_BF16, nullptr);
}

int thip_solver_set_a_f16(thip_solver *s, const uint16_t *mat16, size_t ld16, const float *inv_scale)
{
    return set_a16_external(s, mat16, ld16, THIP_A_F16, inv_scale);
}

int thip_solver_set_a_storage(thip_solver *s, int a_kind)
{
    THIP_NEED_INIT();
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    if (a_kind != THIP_A_F32 && a_kind != THIP_A_BF16 && a_kind != THIP_A_F16)
        return fail(THIP_E_INVALID, "bad storage kind", __FILE__, __LINE__);
    if (s->op != A_DENSE) return fail(THIP_E_INVALID, "storage kinds apply to a dense A", __FILE__, __LINE__);
    StoredA &sa = s->sa;
    if (a_kind == THIP_A_F32 && !sa.f32 && s->m && s->n) return fail(THIP_E_INVALID, "no f32 matrix was given", __FILE__, __LINE__);
    if (a_kind != THIP_A_F32 && sa.kind16 != a_kind && s->m && s->n) {
        // (re)build the library-owned 16-bit copy in the requested format
        if (!sa.f32) return fail(THIP_E_INVALID, "no f32 matrix to convert", __FILE__, __LINE__);
        if (sa.a16 && !sa.a16_owned) return fail(THIP_E_INVALID, "the 16-bit matrix is caller-built", __FILE__, __LINE__);
        hipStream_t st = ctx().stream;
        if (!sa.a16) {
            sa.ld16 = (s->m + 7) / 8 * 8;
            THIP_TRY(hipMalloc((void **)&sa.a16, sa.ld16 * s->n * sizeof(uint16_t)));
            sa.a16_owned = true;
        }
        if (a_kind == THIP_A_F16) {
            if (!sa.inv_s) { THIP_TRY(hipMalloc((void **)&sa.inv_s, s->n * sizeof(float))); sa.inv_s_owned = true; }
            THIP_RC(to_f16(st, s->m, s->n, sa.f32, sa.a16, sa.ld16, sa.inv_s));
        } else {
            THIP_RC(to_bf16(st, s->m, s->n, sa.f32, sa.a16, sa.ld16));
        }
        sa.kind16 = a_kind;
        stored_form_changed(s, PLANS_16);
    }
    if (sa.kind != a_kind) {
        sa.kind = a_kind;
        stored_form_changed(s, KIND);      // (inside a solve: gP / hP rebuilt by the next thip_solver_run, after thip_solver_resume)
    }
    if (s->inited && a_kind == THIP_A_F32) THIP_RC(ensure_apad(s, false));      // first f32 pass of this solve
    if (s->inited) THIP_RC(autotune_gemv(s));      // a switch inside a running solve: tune the other kernel once
    return 0;
}

int thip_solver_set_param(thip_solver *s, const thip_param *par)
{
    if (!s || !par) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    if (par->state_arith != THIP_STATE_COMPENSATED && par->state_arith != THIP_STATE_PLAIN)
        return fail(THIP_E_INVALID, "bad thip_param.state_arith", __FILE__, __LINE__);
    // compensation switched on inside a solve starts from clean Kahan terms
    if (s->par.state_arith != par->state_arith && par->state_arith == THIP_STATE_COMPENSATED && s->kx && ctx().inited)
        THIP_TRY(hipMemsetAsync(s->kx_home, 0, s->kahan_n * sizeof(float), ctx().stream));
    s->par = *par;
    return 0;
}

int thip_solver_resume(thip_solver *s)
{
    THIP_NEED_INIT();
    if (!s || !s->inited) return fail(THIP_E_INVALID, "solver not initialised", __FILE__, __LINE__);
    THIP_RC(poll(s, nullptr));
    const int state = s->hst->state;
    if (state == THIP_ST_RUNNING) return 0;
    if (!(s->hst->kind == 0 && (state == THIP_ST_OK || state == THIP_ST_EXCESS_ITER)))
        return fail(THIP_E_INVALID, "only a solve that ended Converged / ExcessIter (tau > eps_zero) can be resumed",
                    __FILE__, __LINE__);
    hipStream_t st = ctx().stream;
    const unsigned g = egrid(s->n > s->m ? s->n : s->m);
    if (s->finalized) hipLaunchKernelGGL(resume_k, dim3(g), dim3(BLK), 0, st, (int)s->n, (int)s->m, s->xx, s->xy, s->dst);
    s->finalized = false;
    hipLaunchKernelGGL(resume_flags_k, dim3(1), dim3(1), 0, st, s->dst);
    THIP_LAUNCH_CHECK();
    return 0;
}

int thip_solver_passes(const thip_solver *s, int *host_passes, size_t *host_bytes_per_pass)
{
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    int passes = 0; size_t bytes = 0;
    traffic(s, host_passes ? host_passes : &passes, host_bytes_per_pass ? host_bytes_per_pass : &bytes);
    return 0;
}

int thip_solver_schedule_in_use(thip_solver *s, int *host_schedule)
{
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    THIP_NEED_INIT();
    if (s->inited) THIP_RC(sweep_prepare(s));
    if (host_schedule) *host_schedule = (s->schedule == THIP_SCHED_SWEEP && !sweep_active(s)) ? THIP_SCHED_CARRIED : s->schedule;
    return 0;
}

int thip_solver_set_column_shard(thip_solver *s, int on)
{
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    if (s->inited && (on != 0) != s->col_shard)
        return fail(THIP_E_INVALID, "thip_solver_set_column_shard comes before thip_solver_init (the norms and preconditioners depend on it)", __FILE__, __LINE__);
    s->col_shard = on != 0;
    s->sweep_state = 0;
    return 0;
}

int thip_solver_set_sweep_min_bytes(thip_solver *s, size_t bytes)
{
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    s->sweep_min_bytes = bytes;
    s->sweep_state = 0;           // re-planned by the next run / query; sweep_prepare restarts the schedule (sw_first) when it does
    return 0;
}

int thip_solver_sweep_faults(thip_solver *s, int *host_faults, int *host_last_word, int64_t *host_restored_iter)
{
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    if (host_faults) *host_faults = s->sweep_faults;
    if (host_last_word) *host_last_word = (int)s->sweep_fault_word;
    if (host_restored_iter) *host_restored_iter = s->sweep_faults ? (int64_t)s->sweep_fault_iter : -1;
    return 0;
}

int thip_test_sweep_fault(thip_solver *s, int kind, int64_t after_sweeps, int spin_max)
{
    if (!s || kind < 0 || kind > 7) return fail(THIP_E_INVALID, "bad argument", __FILE__, __LINE__);
    if (kind == 5 || kind == 6) { s->no_fold = kind == 5; return 0; }      // 5 / 6: the termination test as its own launch / folded again
    if (kind >= 3 && kind <= 4) { s->no_merge = kind == 3; return 0; }       // 3 / 4: the step's m-kernels as two launches / merged again
    s->fault_kind = kind; s->fault_after = (kind == 2 || kind == 7) ? (long long)after_sweeps : -1;
    s->spin_max = spin_max > 0 ? spin_max : 0;
    return 0;
}

int thip_test_solver_kahan(thip_solver *s, float *host_kx, float *host_ky, float *host_ks, float *host_ku, float *host_kv, int *host_mtail_form)
{
    THIP_NEED_INIT();
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    const size_t n = s->n, m = s->m;
    THIP_RC(poll(s, nullptr));
    if (host_kx) THIP_RC(thip_d2h(host_kx, s->kx, n));
    if (host_ky) THIP_RC(thip_d2h(host_ky, s->ky, m));
    if (host_ks) THIP_RC(thip_d2h(host_ks, s->ks, m));
    if (host_ku) THIP_RC(thip_d2h(host_ku, s->ku, n));
    if (host_kv) THIP_RC(thip_d2h(host_kv, s->kv, m));
    if (host_mtail_form) *host_mtail_form = s->mtail_form;
    return 0;
}

int thip_solver_set_sweep_publish(thip_solver *s, int agent_scope)
{
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    s->pub_agent = agent_scope < 0 ? -1 : (agent_scope != 0);
    return 0;
}

int thip_solver_set_gemv_autotune(thip_solver *s, int on)
{
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    s->autotune = on != 0;
    if (!on) stored_form_changed(s, PLANS_F32 | PLANS_16);        // back to the shape heuristic: the plan no longer depends on timings
    return 0;
}

int thip_solver_set_lda_pad(thip_solver *s, int floats)
{
    if (!s || floats < 0) return fail(THIP_E_INVALID, "bad argument", __FILE__, __LINE__);
    if (s->inited) return fail(THIP_E_INVALID, "thip_solver_set_lda_pad must precede thip_solver_init", __FILE__, __LINE__);
    s->lda_pad = floats;
    return 0;
}

int thip_solver_overlap_info(thip_solver *s, int *host_mode, int *host_launches_per_pass, size_t *host_split_col)
{
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    THIP_RC(prepare_split(s));
    const bool split = split_active(s);
    // what the next thip_solver_run will do: modes 2 / 3 fall back to 1 / 0 where the pipeline does not apply (no
    // collective installed, sparse A, a schedule other than carried, fewer than two column chunks)
    if (host_mode) *host_mode = split ? s->overlap : (s->overlap == 2 ? 1 : (s->overlap == 3 ? 0 : s->overlap));
    if (host_launches_per_pass) *host_launches_per_pass = split ? 2 : 1;
    if (host_split_col) *host_split_col = split ? s->n1 : 0;
    return 0;
}

static int spin_allreduce(void *c, float *, size_t, void *stream)
{
    const thip_solver *s = static_cast<const thip_solver *>(c);
    if (s->spin_ticks > 0) hipLaunchKernelGGL(spin_k, dim3(1), dim3(1), 0, (hipStream_t)stream, s->spin_ticks);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

int thip_test_spin_allreduce(thip_solver *s, int latency_us)
{
    THIP_NEED_INIT();
    if (!s || latency_us < 0) return fail(THIP_E_INVALID, "bad argument", __FILE__, __LINE__);
    int khz = 0;
    THIP_TRY(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx().device));
    if (khz <= 0) khz = 100000;
    s->spin_ticks = (long long)latency_us * khz / 1000;
    return thip_solver_set_allreduce(s, spin_allreduce, s);
}

int thip_solver_gemv_plan(const thip_solver *s, int *host_nj, int *host_blocks, float *host_ms)
{
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    const GemvHint *h = s->hint_in_use();
    if (host_nj) *host_nj = h ? h->nj : 0;
    if (host_blocks) *host_blocks = h ? h->target_blocks : 0;
    if (host_ms) *host_ms = s->plan_in_use().ms;
    return 0;
}

// TEST HOOK (totsu_f32hip_test.h): a candidate tiling installed the way the autotune installs its pick
int thip_test_solver_pin_gemv_plan(thip_solver *s, int candidate_index)
{
    THIP_NEED_INIT();
    int nc = 0;
    const GemvHint *c = gemv_candidates(&nc);
    if (!s || !s->inited || candidate_index < -1 || candidate_index >= nc)
        return fail(THIP_E_INVALID, "null or uninitialised solver, or no such candidate plan", __FILE__, __LINE__);
    THIP_RC(prepare_split(s));                   // the launch form of the next run (and its own tuning, where that is due)
    if (candidate_index < 0) s->plan[s->sa.in_use().is16()][s->split_plan] = GemvPlan{};
    else set_gemv_plan(s, s->split_plan, c[candidate_index], 0.0f);
    return prepare_split(s);                     // the chunk rows of the split form under the plan now in use
}

int thip_solver_sweep_plan(thip_solver *s, int *host_members, int *host_cols_per_panel, int *host_slots, float *host_ms)
{
    THIP_NEED_INIT();
    if (!s) return fail(THIP_E_INVALID, "null solver", __FILE__, __LINE__);
    if (s->inited) THIP_RC(sweep_prepare(s));
    const bool on = sweep_active(s);
    if (host_members) *host_members = on ? s->sgeom.G : 0;
    if (host_cols_per_panel) *host_cols_per_panel = on ? s->sgeom.w : 0;
    if (host_slots) *host_slots = on ? s->sgeom.nslot : 0;
    if (host_ms) *host_ms = on ? s->sw_plan_ms : 0.0f;
    return 0;
}

// TEST HOOK (totsu_f32hip_test.h): a candidate geometry installed the way the plan autotune installs its pick
int thip_test_solver_pin_sweep_plan(thip_solver *s, int candidate_index)
{
    THIP_NEED_INIT();
    if (!s || !s->inited || candidate_index < -1)
        return fail(THIP_E_INVALID, "null or uninitialised solver, or no such candidate geometry", __FILE__, __LINE__);
    if (candidate_index >= 0) {
        // looked up before anything changes: a refused pin leaves the plan in use as it is
        SweepGeom cand[6];
        if (s->op != A_DENSE || s->schedule != THIP_SCHED_SWEEP || (s->allreduce != nullptr) != s->col_shard || s->m == 0 || s->n == 0
            || candidate_index >= sweep_offer(s, cand, nullptr))
            return fail(THIP_E_INVALID, "the one-pass kernel does not offer this candidate geometry for the solver's matrix", __FILE__, __LINE__);
    }
    const int pin_before = s->sweep_pin;
    s->sweep_pin = candidate_index;
    s->sweep_state = 0;
    THIP_RC(sweep_prepare(s));
    if (candidate_index >= 0 && (s->sweep_state != 1 || s->sweep_pin != candidate_index)) {
        // (the schedule is off for this solve: below thip_solver_set_sweep_min_bytes, THIP_SWEEP_OFF, a placement other than 8 x 32)
        s->sweep_pin = pin_before;
        s->sweep_state = 0;
        return fail(THIP_E_INVALID, "the one-pass schedule does not run for this solver: nothing to pin", __FILE__, __LINE__);
    }
    return 0;
}

int thip_prof_enable(int on)
{
    THIP_NEED_INIT();
    // on = 0: off; on = N >= 1: every N-th span of each kind is timed (1: all of them)
    for (Prof *p : { &g_prof, &g_prof_psd }) {
        p->on = on > 0;
        p->period = on > 0 ? on : 1;
        p->seen = 0; p->open = false; p->iter_open = true;
        p->used = 0; p->total_ms = 0.0; p->launches = 0;
    }
    return 0;
}

static int prof_collect(Prof &p, int64_t *host_count, double *host_total_ms)
{
    THIP_TRY(hipStreamSynchronize(ctx().stream));
    for (size_t i = 0; i + 1 < p.used; i += 2) {
        float ms = 0.0f;
        THIP_TRY(hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]));
        p.total_ms += ms;
        p.launches += 1;
    }
    p.used = 0;
    if (host_count) *host_count = p.launches;
    if (host_total_ms) *host_total_ms = p.total_ms;
    return 0;
}

int thip_prof_read_psd(int64_t *host_spans, double *host_total_ms)
{
    THIP_NEED_INIT();
    return prof_collect(g_prof_psd, host_spans, host_total_ms);
}

int thip_prof_read(int64_t *host_launches, double *host_total_ms)
{
    THIP_NEED_INIT();
    return prof_collect(g_prof, host_launches, host_total_ms);
}

int thip_solver_destroy(thip_solver *s)
{
    if (!s) return 0;
    if (ctx().inited) hipStreamSynchronize(ctx().stream);
    if (s->side) { hipStreamSynchronize(s->side); hipStreamDestroy(s->side); }
    if (s->ev_in) hipEventDestroy(s->ev_in);
    if (s->ev_out) hipEventDestroy(s->ev_out);
    for (int k = 0; k < 4; ++k) { if (s->sev_in[k]) hipEventDestroy(s->sev_in[k]); if (s->sev_out[k]) hipEventDestroy(s->sev_out[k]); }
    if (s->gflags) hipFree(s->gflags);
    hipFree(s->cls); hipFree(s->soc_beg); hipFree(s->soc_end); hipFree(s->rot_beg); hipFree(s->rot_end);
    for (auto &g : s->psd_groups) hipFree(g.dev_offs);
    hipFree(s->grp_beg); hipFree(s->grp_end); hipFree(s->psd_work); hipFree(s->arena); hipFree(s->part);
    hipFree(s->gemv_scr); hipFree(s->dst); (void)s->sa.free_pad(); (void)s->sa.free16();
    hipFree(s->sw_partT); hipFree(s->spt_xmax);
    hipFree(s->sw_partH); hipFree(s->sw_gran); hipFree(s->sw_census); hipFree(s->sw_part); hipFree(s->cs_buf);
    if (s->hst) hipHostFree(s->hst);
    if (s->hflags) hipHostFree(s->hflags);
    hipFree(s->snap); hipFree(s->snap_st);
    delete s;
    return 0;
}

}  // extern "C"

