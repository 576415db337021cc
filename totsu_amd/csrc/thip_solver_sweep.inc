// thip_solver_sweep.inc -- part of thip_solver.hip: THIP_SCHED_SWEEP on the host (dense one-pass kernel, or the tiled sparse copy in
// three launches), its plan autotune, the padded copy of A.
namespace {

// ---------------------------------------------------------------------------------------------------
// THIP_SCHED_SWEEP on the host
// ---------------------------------------------------------------------------------------------------
// Can the next run use the one-pass kernel?  Dense f32 A on one GPU in a shape sweep_plan() takes, on a device whose
// placement census came out as 8 x 32 in a dry run.  Examined once per (re)initialisation.
int sweep_pass(thip_solver *s, int first, int np_m = 0, bool timing = false);

// the launch state of a solver on the tiled sparse copy -- the partial-sum buffers (zeroed once: a block without entries is never
// written), the block maxima of the in-vectors -- and the words the sweep schedule's host side reads (error word, block partials)
int spt_buffers(thip_solver *s)
{
    hipStream_t st = ctx().stream;
    if (!s->sw_partT) {
        const size_t fh = std::max<size_t>(sptile_part_floats(s->spt, false), 64), ft = std::max<size_t>(sptile_part_floats(s->spt, true), 64);
        if (s->sw_partH) { THIP_TRY(hipFree(s->sw_partH)); s->sw_partH = nullptr; }
        THIP_TRY(hipMalloc((void **)&s->sw_partH, fh * sizeof(float)));
        THIP_TRY(hipMalloc((void **)&s->sw_partT, ft * sizeof(float)));
        THIP_TRY(hipMalloc((void **)&s->spt_xmax, 2 * SPT_NMAX * sizeof(float)));
        THIP_TRY(hipMemsetAsync(s->sw_partH, 0, fh * sizeof(float), st));
        THIP_TRY(hipMemsetAsync(s->sw_partT, 0, ft * sizeof(float), st));
        THIP_TRY(hipMemsetAsync(s->spt_xmax, 0, 2 * SPT_NMAX * sizeof(float), st));
    }
    if (!s->sw_census) {
        THIP_TRY(hipMalloc((void **)&s->sw_census, 64 * sizeof(unsigned)));
        THIP_TRY(hipMalloc((void **)&s->sw_part, 12 * EG * sizeof(float)));
        THIP_TRY(hipMemsetAsync(s->sw_census, 0, 64 * sizeof(unsigned), st));
        THIP_TRY(hipMemsetAsync(s->sw_part, 0, 12 * EG * sizeof(float), st));
    }
    return 0;
}

// the rows the kernel sweeps on the stored form of A in use (a library-owned copy has zero rows behind row m, and every m-vector of
// the arena has zeros behind entry m) and the geometries it offers there (THIP_SWEEP_CLASS pins one); how many
int sweep_offer(const thip_solver *s, SweepGeom *cand, size_t *m_eff_out)
{
    const DenseA A = s->sa.in_use();              // f32, or the 16-bit form the iteration streams now
    const size_t epv = A.vec_elems();
    const size_t m_up = (s->m + epv - 1) / epv * epv;
    const size_t m_eff = (A.pad_zero && A.lda >= m_up) ? m_up : s->m;
    if (m_eff_out) *m_eff_out = m_eff;
    if (getenv("THIP_SWEEP_CLASS")) return sweep_plan(m_eff, s->n, A, &cand[0]) == 0 ? 1 : 0;
    return sweep_candidates(m_eff, s->n, A, cand, 6);
}

int sweep_prepare(thip_solver *s)
{
    if (s->op == A_TILED) {
        // the tiled sparse copy: no persistent kernel, no placement census, no geometry to time -- the one-pass recurrence
        // in three launches (sweep_pass) whenever it was asked for on one GPU
        THIP_RC(spt_buffers(s));
        if (s->schedule != THIP_SCHED_SWEEP || s->allreduce != nullptr || s->col_shard || s->m == 0 || s->n == 0) return 0;
        if (s->sweep_state != 0) return 0;
        s->sw_first = true;
        s->sgeom = SweepGeom{};
        s->sgeom.ngroups = sptile_slices(s->spt, false);
        s->sgeom.mpad = sptile_pad(s->spt, false);
        s->sgeom.m_eff = (int)s->m;
        s->sw_plan_ms = 0.0f;
        s->sweep_state = 1;
        return 0;
    }
    if (s->schedule != THIP_SCHED_SWEEP) return 0;
    if ((s->allreduce != nullptr) != s->col_shard) return 0;      // row shards run the carried schedule; column shards need the hook
    if (s->op != A_DENSE || s->m == 0 || s->n == 0) return 0;      // not now (may change)
    if (s->sweep_state != 0) return 0;
    s->sweep_state = -1;
    // a (re-)plan restarts the schedule from the consistent iterate: the timing sweeps below rewrite the groups' shares and
    // the granule ring, so whatever a previous run left of them is gone (a first = 1 sweep rebuilds all of it)
    s->sw_first = true;
    static const int env_off = getenv("THIP_SWEEP_OFF") ? atoi(getenv("THIP_SWEEP_OFF")) : 0;
    if (env_off) return 0;
    const DenseA A = s->sa.in_use();              // f32, or the 16-bit form the iteration streams now
    const int elem = A.kind;
    const size_t esize = A.elem_bytes();
    if (!s->col_shard && s->m * s->n * esize < s->sweep_min_bytes) return 0;
    // how the partial dots are published in this process: decided HERE, at plan time (the self-test allocates 64 MB and
    // synchronises; left to the first sweep_pass it ran in the middle of the first batch when the autotune is off)
    (void)sweep_publish_default();
    // the geometries the kernel offers for this matrix (group size, columns per panel)
    SweepGeom cand[6];
    size_t m_eff = 0;
    int nc = sweep_offer(s, cand, &m_eff);
    if (nc == 0) return 0;
    // TEST HOOK (thip_test_solver_pin_sweep_plan): that candidate alone, installed untimed.  A pin the matrix no longer offers (the
    // stored form changed under it) is dropped
    if (s->sweep_pin >= nc) s->sweep_pin = -1;
    const bool pinned = s->sweep_pin >= 0;
    if (pinned) { cand[0] = cand[s->sweep_pin]; nc = 1; }
    hipStream_t st = ctx().stream;
    if (!s->sw_census) {
        THIP_TRY(hipMalloc((void **)&s->sw_census, 64 * sizeof(unsigned)));
        THIP_TRY(hipMalloc((void **)&s->sw_part, 12 * EG * sizeof(float)));
    }
    THIP_TRY(hipMemsetAsync(s->sw_census, 0, 64 * sizeof(unsigned), st));
    s->sw_seq = 0;
    THIP_RC(sweep_census_dry_run(st, s->sw_census, s->sw_seq++));
    unsigned hc[10];
    THIP_TRY(hipMemcpyAsync(hc, s->sw_census, sizeof(hc), hipMemcpyDeviceToHost, st));
    THIP_TRY(hipStreamSynchronize(st));
    if (s->fault_kind == 1) { hc[9] = 2u; s->fault_kind = 0; }      // TEST HOOK: "the placement is not 8 x 32"
    if (hc[9] != 0u) return 0;                      // not 32 workgroups per XCD: the carried schedule runs
    size_t maxH = 0, maxG = 0;
    for (int c = 0; c < nc; ++c) {
        cand[c].m_eff = (int)m_eff;
        maxH = std::max(maxH, (size_t)cand[c].ngroups * 2 * cand[c].mpad);
        maxG = std::max(maxG, sweep_gran_words(cand[c]));
    }
    if (s->sw_partH) { THIP_TRY(hipFree(s->sw_partH)); s->sw_partH = nullptr; }
    if (s->sw_gran) { THIP_TRY(hipFree(s->sw_gran)); s->sw_gran = nullptr; }
    THIP_TRY(hipMalloc((void **)&s->sw_partH, maxH * sizeof(float)));
    THIP_TRY(hipMalloc((void **)&s->sw_gran, maxG * sizeof(unsigned long long)));
    THIP_TRY(hipMemsetAsync(s->sw_partH, 0, maxH * sizeof(float), st));
    THIP_TRY(hipMemsetAsync(s->sw_gran, 0, maxG * sizeof(unsigned long long), st));
    SweepGeom g = cand[0];
    s->sw_plan_ms = 0.0f;
    const char *env_at = getenv("THIP_GEMV_AUTOTUNE");
    const bool tune = !pinned && !(s->autotune == 0 || (s->autotune < 0 && env_at && atoi(env_at) == 0));
    if (tune) {
        // time every geometry on the actual matrix, like the GEMV plans: idempotent sweeps (first = 1: u stays, x_x goes
        // to the buffer that is not the iterate, gP is rewritten with what it has to hold anyway); one warm-up, five timed
        // one by one
        hipEvent_t e0, e1;
        THIP_TRY(hipEventCreate(&e0));
        THIP_TRY(hipEventCreate(&e1));
        constexpr int REP = 7;
        float med[6], spread[6], cost[6];
        for (int c = 0; c < nc; ++c) {
            s->sgeom = cand[c];
            THIP_TRY(hipMemsetAsync(s->sw_gran, 0, maxG * sizeof(unsigned long long), st));
            THIP_RC(sweep_pass(s, 1, 0, true));
            float t[REP];
            for (int r = 0; r < REP; ++r) {
                THIP_TRY(hipEventRecord(e0, st));
                THIP_RC(sweep_pass(s, 1, 0, true));
                THIP_TRY(hipEventRecord(e1, st));
                THIP_TRY(hipEventSynchronize(e1));
                THIP_TRY(hipEventElapsedTime(&t[r], e0, e1));
            }
            unsigned err = 0;
            THIP_TRY(hipMemcpy(&err, s->sw_census + 9, sizeof(err), hipMemcpyDeviceToHost));
            if (err != 0u) {
                // a ticket was off or a spin ran out: the carried schedule runs.  Inside a running solve (a re-plan after
                // thip_solver_set_sweep_min_bytes) the timing sweeps have rewritten gP: rebuilt before the next step
                hipEventDestroy(e0); hipEventDestroy(e1);
                s->carried_stale = true;
                return 0;
            }
            std::sort(t, t + REP);
            med[c] = t[REP / 2];
            spread[c] = (t[REP - 1] - t[0]) / t[REP / 2];
            // what a geometry costs OUTSIDE the kernel: the next step's m-tail reads every group's share of the two N
            // products (2 m floats per group; 20 MB at the 10 000-variable LP with 128 groups) at a few TB/s
            cost[c] = med[c] + (float)((double)cand[c].ngroups * 2.0 * (double)s->m * sizeof(float) / 3.0e12 * 1e3);
        }
        hipEventDestroy(e0); hipEventDestroy(e1);
        // the default geometry (candidate 0) keeps its place unless another one wins by more than repeated sweeps of either
        // differ among themselves (at least 2 %): a geometry that flips with the noise flips the order of the sums -- the
        // bits of every later iterate -- with it
        int bi = 0;
        for (int c = 1; c < nc; ++c) {
            const float margin = std::max(0.02f, std::max(spread[bi], spread[c]));
            if (cost[c] < cost[bi] * (1.0f - margin)) bi = c;
        }
        g = cand[bi];
        s->sw_plan_ms = med[bi];
        THIP_TRY(hipMemsetAsync(s->sw_gran, 0, maxG * sizeof(unsigned long long), st));
        // a safety net for shapes the kernel takes badly (e.g. very few rows per workgroup): a sweep that is not faster
        // than the two passes of the carried schedule gives way to it -- unless the caller asked for the one-pass schedule
        // "whenever the kernel can take the shape" (sweep_min_bytes = 0).  The two passes are priced at the dual GEMV's
        // usual 6.2 TB/s first, and when that is anywhere near, with the carried plan's own MEASURED pass
        if (!s->col_shard && s->sweep_min_bytes != 0) {
            double carried_ms = 2.0 * (double)s->m * (double)s->n * esize / 6.2e12 * 1e3 + 0.03;
            if ((double)s->sw_plan_ms > 0.75 * carried_ms) {
                THIP_RC(autotune_gemv(s));
                const GemvPlan &one = s->plan[elem != 0][0];       // (the one-launch form: no collective on this path)
                const float pass_ms = one.tuned ? one.ms : 0.0f;
                if (pass_ms > 0.0f) carried_ms = 2.0 * (double)pass_ms + 0.03;
            }
            if ((double)s->sw_plan_ms > carried_ms) return 0;
        }
    }
    if (s->col_shard) {
        const size_t need = cs_floats(g.mpad);            // [A u ; A x_x ; 4 x EG sums over n ; "my kernel gave up" flag]
        if (s->cs_n != need) {
            if (s->cs_buf) { THIP_TRY(hipFree(s->cs_buf)); s->cs_buf = nullptr; }
            THIP_TRY(hipMalloc((void **)&s->cs_buf, need * sizeof(float)));
            s->cs_n = need;
        }
        THIP_TRY(hipMemsetAsync(s->cs_buf, 0, need * sizeof(float), st));
    }
    s->sgeom = g;
    s->sgeom.m_eff = (int)m_eff;
    s->sweep_state = 1;
    return 0;
}

bool sweep_active(const thip_solver *s)
{
    if (s->schedule != THIP_SCHED_SWEEP || s->sweep_state != 1) return false;
    if (s->op == A_TILED) return s->allreduce == nullptr && !s->col_shard;
    const DenseA A = s->sa.in_use();
    if (s->op != A_DENSE || (s->allreduce != nullptr) != s->col_shard || s->sgeom.elem != A.kind) return false;       // (planned for the stored form of A in use now)
    // planned on the padded copy (m not a multiple of the rows per slot): only while that copy is the matrix in use
    return (size_t)s->sgeom.m_eff == s->m || (A.pad_zero && A.lda >= (size_t)s->sgeom.m_eff);
}

int sweep_pass(thip_solver *s, int first, int np_m, bool timing)
{
    hipStream_t st = ctx().stream;
    const SweepGeom &g = s->sgeom;
    SweepArgs a;
    const DenseA A = s->sa.in_use();
    a.A = reinterpret_cast<const float *>(A.mat); a.lda = A.lda; a.m = g.m_eff; a.n = (int)s->n;
    a.inv_s = A.inv_s;
    a.G = g.G; a.rows_per_member = g.rows_per_member; a.cols_per_group = g.cols_per_group;
    a.v = s->v; a.xy = s->xy; a.c = s->c; a.Su = s->Su; a.Tx = s->Tx;
    a.u = s->u; a.ku = s->comp() ? s->ku : nullptr;
    const bool b0 = s->xbuf == 0;        // s->xx is the arena's own buffer
    a.xx_in = s->xx; a.xx_out = b0 ? s->xx2 : s->xx_home;
    a.kx_in = s->comp() ? s->kx : nullptr; a.kx_out = s->comp() ? (b0 ? s->kx2 : s->kx_home) : nullptr;
    a.gP = s->gP;
    a.partH = s->sw_partH; a.mpad = g.mpad; a.gran = s->sw_gran; a.census = s->sw_census;
    a.seq = s->sw_seq++; a.tagbase = s->sw_tag; s->sw_tag += (unsigned)g.npan + 1u;
    a.first = first; a.dbg = 0;
    a.stop = &s->dst->stop; a.kappa_p = &s->dst->kappa; a.rtau_p = &s->dst->r_tau;
    a.tau_p = &s->dst->tau; a.eps_zero = s->par.eps_zero;
    a.kappa_out = nullptr; a.skappa_p = &s->dst->s_kappa; a.pm_brx = nullptr; a.np_m = 0; a.pn_count = 0;
    // the sums over n: two buffers by launch parity -- this launch writes one, its kappa update reads what the previous
    // sweep left in the other (column-sharded: what came back from the all-reduce, which no sweep writes)
    const int par = s->pn_par ^ 1;
    a.pn = s->sw_part + (size_t)par * 2 * EG; a.pn_stride = 256;
    a.pn_in = s->sw_part + (size_t)s->pn_par * 2 * EG; a.pn_in_stride = 256;
    if (timing) {
        // a REGULAR sweep's instruction stream and memory traffic (the u update, its Kahan term, five column stores per turn)
        // that changes nothing of the iterate: u / ku go to scratch n-vectors, kappa stays.  The geometries are timed like this:
        // timed as first = 1 sweeps (no u update) the plan autotune picked the 16-bit geometry that is 4 % slower in the loop
        // about every other run (two columns per panel: 1.56 ms as timed, 1.63 in the loop; four: 1.58 / 1.55)
        a.first = 0;
        a.u = s->g1; a.ku = s->comp() ? s->g2 : nullptr;
    } else if (!first) {
        // the sweep of a regular step opens with the kappa update: c.rx_x from the previous sweep's partials, b.rx_y from sw_vm_k
        const unsigned gm_ = np_m > 0 ? (unsigned)np_m : egrid(s->m);      // block partials per sum over m (the m-kernel's grid)
        a.kappa_p = &s->dst->kappa_in; a.kappa_out = &s->dst->kappa;
        a.pm_brx = s->sw_part + (size_t)(4 + 4 * s->pm_par) * EG + gm_; a.np_m = (int)gm_;
        a.pn_count = 256;
        if (s->col_shard) { a.pn_in = s->cs_buf + 2 * g.mpad; a.pn_in_stride = (int)EG; a.pn_count = (int)EG; }
    }
    s->pn_par = par;
    a.spin_max = s->spin_max > 0 ? s->spin_max : SW_SPIN_MAX;
    a.pub_agent = s->pub_agent >= 0 ? s->pub_agent : sweep_publish_default();
    a.fault = 0;
    if (!first && s->fault_kind == 2 && s->fault_after >= 0 && s->fault_after-- == 0) { a.fault = 1; s->fault_kind = 0; }
    if (!first && s->fault_kind == 7 && (s->fault_after < 0 || s->fault_after-- <= 0)) { a.fault = 1; s->fault_after = -1; }      // every sweep from then on
    if (s->op == A_TILED) {
        // A^T [v x_y] -> per column: u_k[j], x_x_{k+1}[j], kappa, the sums over n -> A [u_k x_x_{k+1}] as the slices' shares
        prof_begin(st);
        THIP_RC(sptile_product(st, s->spt, true, a.v, a.xy, s->sw_partT, s->spt_xmax, 0, a.stop));
        prof_end(st);
        THIP_RC(sptile_colupdate(st, s->spt, a, s->sw_partT, s->spt_xmax));
        prof_begin(st);
        THIP_RC(sptile_product(st, s->spt, false, a.u, a.xx_out, s->sw_partH, s->spt_xmax, 0, a.stop, true));      // (sp_col_k left the block maxima)
        prof_end(st);
        return 0;
    }
    prof_begin(st);
    THIP_RC(sweep_launch(st, g, a));
    prof_end(st);
    return 0;
}

void sweep_swap(thip_solver *s)
{
    const bool b0 = s->xbuf == 0;
    s->xx = b0 ? s->xx2 : s->xx_home;
    s->kx = b0 ? s->kx2 : s->kx_home;
    s->xbuf ^= 1;
}

// last: the host looks at the status block after this iteration (end of a polling batch / of the run)
int one_iteration_sweep(thip_solver *s, bool last)
{
    hipStream_t st = ctx().stream;
    const int m = (int)s->m;
    const unsigned gm = egrid(s->m);
    const float ez = s->par.eps_zero;
    const bool cols = s->col_shard;
    // sums over n: [0] ||d||^2 [1] c.x_x [2] c.u [3] c.rx_x -- one partial per workgroup of the sweep; column-sharded: EG
    // slots each (the same on every rank, the unused ones stay zero) behind the two N products in the buffer that is
    // all-reduced
    // (the sweep itself writes 4 x 256 to one of two buffers by launch parity: pn_now(); sw_gsum_k moves them into the tail)
    auto pn_now = [&]() -> float * { return cols ? s->cs_buf + 2 * s->sgeom.mpad : s->sw_part + (size_t)s->pn_par * 2 * EG; };
    const int pns = cols ? (int)EG : 256;         // one slot per workgroup of the sweep (256), EG in the all-reduced buffer
    // sums over m: [0] b.v [1] b.rx_y [2] ||p||^2 [3] b.x_y, gmm block partials each -- two buffers: a merged m-kernel that
    // evaluates the previous iterate's termination test at its head reads one (the previous step's) and writes the other
    auto pm_cur = [&]() -> float * { return s->sw_part + (size_t)(4 + 4 * s->pm_par) * EG; };
    float *const ky = s->comp() ? s->ky : nullptr, *const ks = s->comp() ? s->ks : nullptr;
    float *const kv = s->comp() ? s->kv : nullptr;
    auto post = [&]() -> int {
        // (the sums over n -- ||d||^2, c.x_x, c.u, c.rx_x -- come out of the sweep itself: SweepArgs::pn)
        if (cols) {
            hipLaunchKernelGGL(sw_gsum_k, dim3(gm), dim3(BLK), 0, st, m, s->sgeom.ngroups, s->sgeom.mpad, s->sw_partH, s->cs_buf, s->dst,
                               s->sw_part + (size_t)s->pn_par * 2 * EG, s->sw_census + 9);
            THIP_RC(do_allreduce(s, s->cs_buf, s->cs_n));
        }
        return 0;
    };
    // no block cones (an LP: zero / nonneg rows only): the two m-kernels of a step are one launch
    const bool merge = s->n_soc == 0 && s->n_rot == 0 && s->psd.empty() && !s->no_merge;
    // every row in a (plain) second-order cone of at most 129 rows: the three m-launches of a step are one, a wave per cone
    const bool cone_merge = !merge && !s->no_merge && s->all_soc_short;
    const unsigned gx = merge ? grid_for(s->m, 64, EG) : grid_for(s->m, 64, 4096);      // (merged: its block partials fill gm slots)
    const unsigned gc = grid_for(s->n_soc, 1, EG);       // a workgroup per cone
    const unsigned gmm = merge ? gx : (cone_merge ? gc : gm);           // block partials per sum over m
    if (s->sw_first) {
        // from a consistent iterate (x_0, or wherever a run stopped): u is current, so the sweep leaves it alone
        THIP_RC(sweep_pass(s, 1, (int)gmm));
        THIP_RC(post());
        hipLaunchKernelGGL(sw_bv_k, dim3(gmm), dim3(BLK), 0, st, m, s->b, s->v, pm_cur(), s->dst);
        hipLaunchKernelGGL(sw_tau_k, dim3(1), dim3(BLK), 0, st, s->dst, pn_now() + 2 * pns, pns, pm_cur(), (int)gmm);
        s->sw_first = false;
        s->status_pending = false;
    }
    // the termination test of iterate k: by status_k after the sweep when the host is about to look, else by every block of
    // the NEXT step's (first) m-kernel at its head
    auto stat_args = [&](float *pmb) -> StatArgs {
        return StatArgs{ pns, pn_now(), pmb + 2 * gmm, pmb + 3 * gmm, (int)gmm, pn_now() + 2 * pns, pns, pmb, (int)gmm,
                         cols ? (const float *)(s->cs_buf + cs_flag_slot(s->sgeom.mpad)) : (const float *)nullptr,
                         s->par.eps_acc, s->par.eps_inf, ez, (long long)s->par.max_iter, s->xbuf };
    };
    const bool foldable = !s->no_fold;
    const int fold = (foldable && s->status_pending) ? 1 : 0;
    const StatArgs sa_prev = stat_args(pm_cur());          // (read by the head only when fold != 0)
    // a merged kernel writes its sums over m while other blocks still read the previous step's at their head: the other buffer
    // (the three-launch form writes them in sw_vm_k, a later launch: one buffer)
    if (foldable && (merge || cone_merge)) s->pm_par ^= 1;
    float *const pm = pm_cur();
    // (a sparse operator with at most four slices per row block: the one-thread-per-row form of the two sw_xm_k launches)
    const bool flat_rows = s->op == A_TILED && !cols && s->sgeom.ngroups <= 4;
    const unsigned xm_threads = (flat_rows && s->m > (size_t)EG * 1024) ? 1024u : (unsigned)BLK;
    s->mtail_form = (merge ? 1 : (cone_merge ? 2 : 3)) + ((flat_rows && !cone_merge) ? 4 : 0);
    if (merge) {
        hipLaunchKernelGGL((flat_rows ? sw_xm_k<true, true> : sw_xm_k<true, false>), dim3(gx), dim3(xm_threads), 0, st, m, cols ? 1 : s->sgeom.ngroups, s->sgeom.mpad,
                           cols ? s->cs_buf : s->sw_partH, s->h3, s->b, s->v, s->Ty, s->Ts, s->cls, s->xy, s->xs, s->rxy, s->rxs,
                           s->dst, ky, ks, s->hP, s->Sv, kv, ez, pm, sa_prev, fold, s->step_par);
        s->step_par ^= 1;
    } else if (cone_merge) {
        hipLaunchKernelGGL(sw_cone_k, dim3(gc), dim3(BLK), 0, st, (int)s->n_soc, s->soc_beg, s->soc_end, cols ? 1 : s->sgeom.ngroups,
                           s->sgeom.mpad, cols ? s->cs_buf : s->sw_partH, s->b, s->v, s->Ty, s->Ts, s->xy, s->xs, s->rxy, s->rxs,
                           s->dst, ky, ks, s->hP, s->Sv, kv, ez, pm, sa_prev, fold, s->step_par);
        s->step_par ^= 1;
    } else {
        hipLaunchKernelGGL((flat_rows ? sw_xm_k<false, true> : sw_xm_k<false, false>), dim3(gx), dim3(xm_threads), 0, st, m, cols ? 1 : s->sgeom.ngroups, s->sgeom.mpad,
                           cols ? s->cs_buf : s->sw_partH, s->h3, s->b, s->v, s->Ty, s->Ts, s->cls, s->xy, s->xs, s->rxy, s->rxs,
                           s->dst, ky, ks, s->hP, s->Sv, kv, ez, pm, sa_prev, fold, s->step_par);
        s->step_par ^= 1;
        THIP_RC(project_blocks(s));
        hipLaunchKernelGGL(sw_vm_k, dim3(gm), dim3(BLK), 0, st, m, s->h3, s->hP, s->b, s->rxs, s->rxy, s->Sv, s->v, kv, s->xs,
                           s->xy, ez, s->dst, pm);
    }
    // (kappa_k is formed by the sweep's workgroups at entry: SweepArgs::kappa_out)
    sweep_swap(s);                                // x_x_k (formed by the previous sweep) is now the iterate
    THIP_RC(sweep_pass(s, 0, (int)gmm));
    THIP_RC(post());
    if (last || !foldable) {
        hipLaunchKernelGGL(status_k, dim3(1), dim3(BLK), 0, st, stat_args(pm), s->dst);
        s->status_pending = false;
    } else {
        s->status_pending = true;
    }
    THIP_LAUNCH_CHECK();
    return 0;
}

// The f32 passes stream a library-owned copy of A whose leading dimension is padded to a multiple of 16 floats (64 bytes)
// when m is not one already: aligned columns (measured on row shards of the 50 000-column SOCP: columns of 50 000 B,
// m = 12 500, 6.32 -> 6.79 TB/s; of 100 000 B 6.3 -> 6.7 TB/s; a 128-byte pitch gains nothing more) and a partial last
// row tile that may run the unguarded kernel body (DESIGN.md 4.1a/b).  Made only when an f32 pass is about to run (never
// while the solve streams a 16-bit copy) and when it leaves two thirds of the free HBM untouched (a 40 GB shard of
// BASELINE configs[4] on a 288 GB part: yes); refreshed by every thip_solver_init, so a caller that rewrites mat_a in
// place between solves is seen.  THIP_LDA_PAD = the multiple in floats (default 16; 0 = never copy); the API form is
// thip_solver_set_lda_pad.
int ensure_apad(thip_solver *s, bool refresh)
{
    StoredA &sa = s->sa;
    if (s->op != A_DENSE || !sa.f32 || s->m == 0 || s->n == 0) return 0;
    hipStream_t st = ctx().stream;
    const size_t m = s->m, n = s->n;
    size_t padto = 16;
    if (s->lda_pad >= 0) padto = (size_t)s->lda_pad;
    else if (getenv("THIP_LDA_PAD")) padto = (size_t)atoi(getenv("THIP_LDA_PAD"));
    const size_t ld = (padto == 0 || m % padto == 0) ? 0 : (m + padto - 1) / padto * padto;      // 0: no copy wanted
    if (sa.pad && sa.ldpad != ld) {      // freed, or re-pitched below
        THIP_TRY(hipStreamSynchronize(st));
        THIP_TRY(sa.free_pad());
        stored_form_changed(s, PLANS_F32);
    }
    if (ld == 0) return 0;
    bool fresh = false;
    if (!sa.pad) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        if (ld * n * sizeof(float) >= free_b / 3) return 0;
        THIP_TRY(hipMalloc((void **)&sa.pad, ld * n * sizeof(float)));
        sa.ldpad = ld;
        THIP_TRY(hipMemsetAsync(sa.pad, 0, ld * n * sizeof(float), st));
        fresh = true;
        stored_form_changed(s, PLANS_F32);             // the plans were timed on the other pitch
    }
    if (fresh || refresh)
        THIP_TRY(hipMemcpy2DAsync(sa.pad, ld * sizeof(float), sa.f32, m * sizeof(float), m * sizeof(float), n,
                                  hipMemcpyDeviceToDevice, st));
    return 0;
}

}  // namespace
