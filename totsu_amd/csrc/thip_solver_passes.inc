// thip_solver_passes.inc -- part of thip_solver.hip: the schedules that read A 2-6 times per iteration (reference / fused / carried),
// the column-split pipeline of row-sharded runs, the GEMV plan autotune.
namespace {

bool sweep_active(const thip_solver *s);

// ---- what depends on the operator kind, side by side: a stage's products, the preconditioner's abs sums, the traffic ----------
// one product of a sparse operator as a finished vector (t: with A^T; abs_mode: |A| times ones).  Tiled copy: a pass over the
// stored entries, then its slices added up; two-CSR form: a gather over the CSR of A or of A^T
int spt_product(thip_solver *s, bool t, const float *in, int abs_mode, const int *stop, float *out)
{
    hipStream_t st = ctx().stream;
    float *part = t ? s->sw_partT : s->sw_partH;
    if (!abs_mode) prof_begin(st);
    THIP_RC(sptile_product(st, s->spt, t, in, nullptr, part, s->spt_xmax, abs_mode, stop));
    if (!abs_mode) prof_end(st);
    return finalize_partials(st, t ? s->n : s->m, part, sptile_slices(s->spt, t), 2 * sptile_pad(s->spt, t), 1.0f, 0.0f, out, nullptr);
}
int csr_product(const thip_solver *s, bool t, const float *in, int abs_mode, float *out)
{
    const Csr2 &a = s->csr;
    return t ? thip_spmv_csr(s->n, s->m, a.nnz, a.trp, a.tci, a.tsv, 1.0f, abs_mode ? a.tsv : in, 0.0f, out, abs_mode)
             : thip_spmv_csr(s->m, s->n, a.nnz, a.rp, a.ci, a.sv, 1.0f, abs_mode ? a.sv : in, 0.0f, out, abs_mode);
}

// one stage's products: A xn (m) and A^T xt (n).  Dense: as partial sums -- the fused and carried schedules read A once (dual
// launch), the reference schedule issues the reference's two single GEMVs.  Sparse: hN and gT as finished vectors; nN = nT = -1
// tells post_k to take them as they are (the stop flag is honoured by the consumers: a stray product is harmless).
int products(thip_solver *s, const float *xn, const float *xt, GemvPartials *gp, float *hN, float *gT)
{
    hipStream_t st = ctx().stream;
    const int *stop = &s->dst->stop;
    gp->partN = gp->partT = nullptr; gp->nN = gp->nT = 0; gp->strideN = gp->strideT = 0;
    if (s->m == 0 || s->n == 0) return 0;     // zero-sized operator: products are 0 (matop.rs:83-85)
    const DenseA A = s->sa.in_use();
    const GemvHint *hint = s->hint_in_use();
    switch (s->op) {
    case A_TILED:
        THIP_RC(spt_product(s, false, xn, 0, stop, hN));
        THIP_RC(spt_product(s, true, xt, 0, stop, gT));
        break;
    case A_CSR2:
        prof_begin(st);
        THIP_RC(csr_product(s, false, xn, 0, hN));
        THIP_RC(csr_product(s, true, xt, 0, gT));
        prof_end(st);
        break;
    case A_DENSE:
        if (s->schedule == THIP_SCHED_REFERENCE) {
            GemvPartials a, b;
            const size_t half = s->gemv_scr_n / 2;
            prof_begin(st);
            THIP_RC(dual_gemv_partials(st, s->m, s->n, A, nullptr, xt, false, true, false, s->gemv_scr, half, &a, stop, hint));
            prof_end(st);
            prof_begin(st);
            THIP_RC(dual_gemv_partials(st, s->m, s->n, A, xn, nullptr, true, false, false, s->gemv_scr + half, half, &b, stop, hint));
            prof_end(st);
            gp->partT = a.partT; gp->nT = a.nT; gp->strideT = a.strideT;
            gp->partN = b.partN; gp->nN = b.nN; gp->strideN = b.strideN;
        } else {
            prof_begin(st);
            THIP_RC(dual_gemv_partials(st, s->m, s->n, A, xn, xt, true, true, false, s->gemv_scr, s->gemv_scr_n, gp, stop, hint));
            prof_end(st);
        }
    }
    if (s->op != A_DENSE) gp->nN = gp->nT = -1;
    return 0;
}

// |A| row sums (m) and column sums (n) of the preconditioner (solver.rs:171-172), as finished vectors
int abs_sums(thip_solver *s, float *rowabs, float *colabs)
{
    hipStream_t st = ctx().stream;
    GemvPartials gp;
    if (s->n == 0 || s->m == 0) return 0;
    switch (s->op) {
    case A_TILED:
        THIP_RC(spt_product(s, false, s->c, 1, nullptr, rowabs));
        return spt_product(s, true, s->c, 1, nullptr, colabs);
    case A_CSR2:
        THIP_RC(csr_product(s, false, nullptr, 1, rowabs));
        return csr_product(s, true, nullptr, 1, colabs);
    case A_DENSE:      // solver-owned scratch (several solvers may share the context, e.g. one per thread)
        THIP_RC(dual_gemv_partials(st, s->m, s->n, s->sa.in_use(), nullptr, nullptr, true, true, true, s->gemv_scr, s->gemv_scr_n,
                                   &gp, nullptr));
        THIP_RC(finalize_partials(st, s->m, gp.partN, gp.nN, gp.strideN, 1.0f, 0.0f, rowabs, nullptr));
        return finalize_partials(st, s->n, gp.partT, gp.nT, gp.strideT, 1.0f, 0.0f, colabs, nullptr);
    }
    return 0;
}

// passes over the operator per iteration and the algorithmic bytes of one
void traffic(const thip_solver *s, int *passes, size_t *bytes)
{
    const bool ref = s->schedule == THIP_SCHED_REFERENCE;
    const int stages = (ref || s->schedule == THIP_SCHED_FUSED) ? 3 : (sweep_active(s) ? 1 : 2);
    // a stage reads a dense / two-CSR A once (the reference schedule: in its two single GEMVs); of the tiled copy every product is
    // one pass over the stored entries (8 bytes each)
    *passes = (ref || s->op == A_TILED) ? 2 * stages : stages;
    switch (s->op) {
    case A_TILED:
        *bytes = sptile_bytes_per_pass(s->spt);
        break;
    case A_CSR2:
        *bytes = 2 * s->csr.nnz * (sizeof(float) + sizeof(int32_t));
        break;
    case A_DENSE:      // SURVEY.md 8d: 4 m n, or 2 m n for a 16-bit A; the padding rows of a library-owned copy (at most 15 per
                       // column) are zeros that the kernel never loads
        *bytes = s->m * s->n * s->sa.in_use().elem_bytes();
    }
}

int project_blocks(thip_solver *s)
{
    hipStream_t st = ctx().stream;
    const int *stop = &s->dst->stop;
    // SOC / RotSOC / PSD are self-dual (cone_soc.rs:38, cone_psd.rs:56): x_y and x_s get the same projection
    THIP_RC(soc_batched2(st, s->xy, s->xs, s->rxy, s->rxs, s->soc_beg, s->soc_end, s->n_soc, 0, s->soc_max, stop));
    THIP_RC(soc_batched2(st, s->xy, s->xs, s->rxy, s->rxs, s->rot_beg, s->rot_end, s->n_rot, 1, s->rot_max, stop));
    if (!s->psd.empty()) {
        // the x_y and x_s blocks of a cone go through the projection chain together (2 items per launch)
        // the reflection rx <- rx - 2 x of the projected rows rides in the projection kernels' pack when every cone's
        // engine takes it (the polar kernels do)
        bool fold = true;
        for (auto &pr : s->psd) {
            const size_t k = (size_t)((std::sqrt((double)(8 * pr.second + 1)) - 1.0) / 2.0 + 0.5);
            fold = fold && psd_project_takes_rx(k);
        }
        prof_begin(st, g_prof_psd);
        for (auto &g : s->psd_groups)
            THIP_RC(eig_psd_project_small(st, g.k, s->xy, g.dev_offs, g.count, 1, std::sqrt(2.0f), stop, 2, s->xs - s->xy,
                                          fold ? s->rxy : nullptr, s->rxs - s->rxy));
        for (auto &pr : s->psd) {
            const size_t sn = (size_t)pr.second;
            const size_t k = (size_t)((std::sqrt((double)(8 * sn + 1)) - 1.0) / 2.0 + 0.5);
            if (k <= psd_small_max()) continue;           // went with its group
            THIP_RC(eig_psd_project(st, k, s->xy + pr.first, 1, std::sqrt(2.0f), s->par.eps_zero, s->psd_work,
                                    s->psd_worklen, 0, stop, 2, s->xs - s->xy, fold ? s->rxy + pr.first : nullptr,
                                    s->rxs - s->rxy));
        }
        prof_end(st, g_prof_psd);
        if (fold) return 0;
        hipLaunchKernelGGL(rx_psd_k, dim3(egrid(s->m)), dim3(BLK), 0, st, (int)s->m, s->cls, s->xy, s->xs, s->rxy, s->rxs, s->dst);
    }
    return 0;
}

// What every stage of one_iteration works with: grids, the block-partial buffers, the Kahan terms in use
struct IterCtx {
    thip_solver *s; hipStream_t st; int n, m; unsigned g, gq; float *part, *part_y; bool carried, local, split; float ez;
    size_t arcount; float *kx, *ky, *ks, *ku, *kv;
    explicit IterCtx(thip_solver *s_) : s(s_)
    {
        st = ctx().stream;
        n = (int)s->n; m = (int)s->m;
        g = egrid(s->n > s->m ? s->n : s->m);
        part = s->part;
        carried = s->carried_like();
        ez = s->par.eps_zero;
        // post_k leaves its sums as block partials: q0 (over the replicated n-vectors) in `part`, q1..q3 (over the local
        // rows) in `part` too on a single GPU, or -- row-sharded -- in the tail of the n-vector that is all-reduced next,
        // with a fixed grid of NPS blocks so that every rank fills the same NPS slots per sum.
        local = s->allreduce == nullptr;
        gq = local ? grid_for(s->n > s->m ? s->n : s->m, 64, PG) : NPS;
        arcount = s->n + TAIL;
        part_y = s->part + 4 * PG;          // ycrit_k's own partials (read by status_k)
        split = !local && (s->overlap == 1 || s->overlap == 2);   // m-part under the all-reduce, n-part after it
        kx = s->comp() ? s->kx : nullptr; ky = s->comp() ? s->ky : nullptr;
        ks = s->comp() ? s->ks : nullptr; ku = s->comp() ? s->ku : nullptr;
        kv = s->comp() ? s->kv : nullptr;
    }
    float *shp(float *nvec) const { return local ? part : nvec + s->n; }
};

// ---- stage X after its products: x update (solver.rs:538-555) ------------------------------------
int stage_x_tail(thip_solver *s, const GemvPartials &gp)
{
    const IterCtx c(s);
    hipStream_t st = c.st;
    const int n = c.n, m = c.m;
    const unsigned g = c.g, gq = c.gq;
    float *const part = c.part;
    auto xupdate = [&](int do_n, int do_m) {
        hipLaunchKernelGGL(xupdate_k, dim3(g), dim3(BLK), 0, st, n, m, s->g1, s->h1, s->c, s->b, s->v, s->Tx, s->Ty, s->Ts,
                           s->cls, s->xx, s->xy, s->xs, s->rxx, s->rxy, s->rxs, s->dst, part, (int)gq, c.shp(s->g1) + gq, (int)gq,
                           do_n, do_m, do_n, c.kx, c.ky, c.ks);
    };
    hipLaunchKernelGGL(post_k, dim3(gq), dim3(BLK), 0, st, n, m, gp.partT, gp.nT, gp.strideT, s->g1, gp.partN, gp.nN,
                       gp.strideN, s->h1, s->c, s->u, s->b, s->v, 0, (const float *)nullptr, (const float *)nullptr,
                       (const float *)nullptr, c.ez, part, c.shp(s->g1), s->dst, 1);
    THIP_RC(allreduce_begin(s, s->g1, c.arcount));
    if (c.split) {
        xupdate(0, 1);
        THIP_RC(project_blocks(s));      // the block cones live on the local rows
        THIP_RC(allreduce_end(s));
        xupdate(1, 0);
    } else {
        THIP_RC(allreduce_end(s));
        xupdate(1, 1);
        THIP_RC(project_blocks(s));
    }
    return 0;
}

// ---- stage Y: y update from K rx (solver.rs:557-567), own products (the schedules that do not carry them) ----
int stage_y(thip_solver *s)
{
    const IterCtx c(s);
    hipStream_t st = c.st;
    const int n = c.n, m = c.m;
    const unsigned g = c.g, gq = c.gq;
    float *const part = c.part;
    GemvPartials gp;
    THIP_RC(products(s, s->rxx, s->rxy, &gp, s->h2, s->g2));
    hipLaunchKernelGGL(post_k, dim3(gq), dim3(BLK), 0, st, n, m, gp.partT, gp.nT, gp.strideT, s->g2, gp.partN, gp.nN,
                       gp.strideN, s->h2, s->c, s->rxx, s->b, s->rxy, 0, (const float *)nullptr,
                       (const float *)nullptr, (const float *)nullptr, c.ez, part, c.shp(s->g2), s->dst, 1);
    auto yupdate = [&](int do_n, int do_m) {
        hipLaunchKernelGGL(ycrit_k, dim3(g), dim3(BLK), 0, st, n, m, 1, 0, 0, (const float *)nullptr,
                           (const float *)nullptr, (float *)nullptr, (float *)nullptr, s->g2, s->h2, s->c, s->b, s->rxs,
                           s->Su, s->Sv, s->u, s->v, s->xx, c.ez, c.part_y, s->dst, part, (int)gq, c.shp(s->g2) + gq, (int)gq,
                           do_n, do_m, do_n, 0, (int)g, c.ku, c.kv);
    };
    THIP_RC(allreduce_begin(s, s->g2, c.arcount));
    if (c.split) { yupdate(0, 1); THIP_RC(allreduce_end(s)); yupdate(1, 0); }
    else         { THIP_RC(allreduce_end(s)); yupdate(1, 1); }
    return 0;
}

// ---- stage C after its products: criteria of the new iterate (solver.rs:573-656), the carried y update, the termination test ----
int stage_c_tail(thip_solver *s, const GemvPartials &gp)
{
    const IterCtx c(s);
    hipStream_t st = c.st;
    const int n = c.n, m = c.m;
    const unsigned g = c.g, gq = c.gq;
    float *const part = c.part;
    const bool carried = c.carried;
    // block partials: q0 = c.rx_x, q1 = b.rx_y (carried), q2 = ||p||^2, q3 = b.x_y
    hipLaunchKernelGGL(post_k, dim3(gq), dim3(BLK), 0, st, n, m, gp.partT, gp.nT, gp.strideT, s->g3, gp.partN, gp.nN,
                       gp.strideN, s->h3, carried ? s->c : (const float *)nullptr, s->rxx,
                       carried ? s->b : (const float *)nullptr, s->rxy, 1, s->xs, s->xy, s->b, c.ez, part, c.shp(s->g3), s->dst, 1);
    auto ycrit = [&](int do_n, int do_m) {
        hipLaunchKernelGGL(ycrit_k, dim3(g), dim3(BLK), 0, st, n, m, carried ? 1 : 0, 1, 1, s->g3, s->h3, s->gP, s->hP,
                           (const float *)nullptr, (const float *)nullptr, s->c, s->b, s->rxs, s->Su, s->Sv, s->u, s->v, s->xx,
                           c.ez, c.part_y, s->dst, part, (int)gq, c.shp(s->g3) + gq, (int)gq, do_n, do_m, do_n, 0, (int)g, c.ku, c.kv);
    };
    THIP_RC(allreduce_begin(s, s->g3, c.arcount));
    if (c.split && carried) { ycrit(0, 1); THIP_RC(allreduce_end(s)); ycrit(1, 0); }
    else                    { THIP_RC(allreduce_end(s)); ycrit(1, 1); }
    {
        const StatArgs sa{ (int)g, c.part_y, c.shp(s->g3) + 2 * gq, c.shp(s->g3) + 3 * gq, (int)gq, nullptr, 0, nullptr, 0, nullptr,
                           s->par.eps_acc, s->par.eps_inf, c.ez, (long long)s->par.max_iter, s->xbuf };
        hipLaunchKernelGGL(status_k, dim3(1), dim3(BLK), 0, st, sa, s->dst);
    }
    THIP_LAUNCH_CHECK();
    return 0;
}

// One iteration = the products of a stage, then its tail.  The tails take the partial sums from wherever the product left them:
// a batch of solvers that share A (thip_solver_batch.inc) forms them for several instances from one read of A.
int one_iteration(thip_solver *s)
{
    GemvPartials gp;
    THIP_RC(products(s, s->u, s->v, &gp, s->h1, s->g1));
    THIP_RC(stage_x_tail(s, gp));
    if (!s->carried_like()) THIP_RC(stage_y(s));
    THIP_RC(products(s, s->xx, s->xy, &gp, s->h3, s->g3));
    return stage_c_tail(s, gp);
}

// ---------------------------------------------------------------------------------------------------
// Column-split pipeline for row-sharded runs (thip_solver_set_overlap(s, 2); carried schedule, dense A).
//
// A stage's products only need, column range by column range, the all-reduced entries of the n-vector they multiply
// (solver.rs:146 vs 149, 122 vs 125: the N product of columns [a, b) reads x[a .. b) only).  So every stage runs as two
// launches over the column halves H1 = [0, n1) and H2 = [n1, n), and the all-reduce of a half's A^T y travels on the
// side stream while the NEXT half-launch streams its part of A:
//
//   X.1  gemv(H1; u, v)  post -> g1[H1]                         AR(g1[H1])   ---------.
//        [tail of the previous iteration: wait AR(g3[H2]) ; u[H2], kappa, criteria ; termination test]
//   X.2  gemv(H2; u, v)  post -> g1[H2], h1, b.v partials       AR(g1[H2] + tail) ----|--.
//        wait AR(g1[H1]) <----------------------------------------------------------'  |
//        x_x[H1], x_y, x_s, block cones                                                 |
//   C.1  gemv(H1; x_x, x_y)  post -> g3[H1]                     AR(g3[H1])   ---------. |
//        wait AR(g1[H2]) <------------------------------------------------------------|-'
//        x_x[H2], tau                                                                  |
//   C.2  gemv(H2; x_x, x_y)  post -> g3[H2], h3, criteria sums  AR(g3[H2] + tail) ----|--.  (consumed by the tail above)
//        wait AR(g3[H1]) <------------------------------------------------------------'
//        u[H1], v
//
// Every collective has a whole half-launch (0.19 ms on a 1/8 shard of BASELINE configs[2]) to complete in.  The sharded
// block partials ride with the second half.  The termination test of iteration k is enqueued after the first
// half-launch of iteration k + 1; that launch and its reduction only write scratch (partial sums, g1[H1]), so the
// iterate is still exactly the one of stopping at iteration k.  The split column n1 is a function of n alone -- every
// rank must issue collectives of the same lengths, whatever plan its own autotune picked; each half-launch has its own
// column chunks and fills consecutive chunk rows of the partial sums (dual_gemv_partials_cols).  Mode 3 enqueues the same
// kernels with the collectives in order and no skew: the iterates of modes 2 and 3 are bitwise equal
// (tests/test_gpu_sharded.py).
// ---------------------------------------------------------------------------------------------------
// The split column is the SAME on every rank (it sets the lengths of the collectives): a function of n alone, never of a
// rank's own tuned plan.  A multiple of 8 floats keeps every buffer offset 32-byte aligned.
size_t split_column(const thip_solver *s)
{
    if (s->op != A_DENSE || s->m == 0) return 0;
    return gemv_split_column(s->n);
}

bool split_active(const thip_solver *s)
{
    return s->split_plan && s->n1 > 0 && s->n1 < s->n;
}

int autotune_gemv(thip_solver *s);

// THE place a tiling is installed for the stored form in use and a launch form (split: the column-split pipeline): the autotune's
// pick, or a test's pin (thip_test_solver_pin_gemv_plan)
void set_gemv_plan(thip_solver *s, bool split, GemvHint hint, float ms)
{
    s->plan[s->sa.in_use().is16()][split] = GemvPlan{ hint, true, ms };
}

// decides the form of the next run: column-split (its own tuned plan, its split column) or one launch per pass
int prepare_split(thip_solver *s)
{
    s->split_plan = s->overlap >= 2 && s->allreduce != nullptr && s->op == A_DENSE && s->carried_like()
                    && s->m > 0 && s->n > 0;
    s->n1 = 0;
    if (s->inited && !sweep_active(s)) THIP_RC(autotune_gemv(s));        // once per stored form and launch form (a no-op afterwards)
    if (!s->split_plan) return 0;
    s->n1 = split_column(s);
    if (s->n1 == 0 || s->n1 >= s->n) { s->split_plan = false; s->n1 = 0; return 0; }
    // chunk rows the two half-launches fill under the plan in use
    s->rows1 = dual_gemv_chunk_rows(s->m, s->n1, s->sa.in_use(), s->hint_in_use(), nullptr);
    s->rows2 = dual_gemv_chunk_rows(s->m, s->n - s->n1, s->sa.in_use(), s->hint_in_use(), nullptr);
    return 0;
}

int ar_begin(thip_solver *s, int slot, float *buf, size_t count)
{
    if (s->overlap != 2) return do_allreduce(s, buf, count);
    hipStream_t st = ctx().stream;
    if (s->use_gates) {
        const unsigned v = ++s->gseq[slot];
        hipLaunchKernelGGL(signal_k, dim3(1), dim3(1), 0, st, s->gflags + slot, v);
        hipLaunchKernelGGL(gate_k, dim3(1), dim3(1), 0, s->side, s->gflags + slot, v, s->gate_ticks, s->gflags + 8, &s->dst->stop);
        const int rc = s->allreduce(s->allreduce_ctx, buf, count, (void *)s->side);
        if (rc != 0) return fail(rc, "all-reduce callback failed", __FILE__, __LINE__);
        hipLaunchKernelGGL(signal_k, dim3(1), dim3(1), 0, s->side, s->gflags + 4 + slot, v);
        THIP_LAUNCH_CHECK();
        return 0;
    }
    THIP_TRY(hipEventRecord(s->sev_in[slot], st));
    THIP_TRY(hipStreamWaitEvent(s->side, s->sev_in[slot], 0));
    const int rc = s->allreduce(s->allreduce_ctx, buf, count, (void *)s->side);
    if (rc != 0) return fail(rc, "all-reduce callback failed", __FILE__, __LINE__);
    THIP_TRY(hipEventRecord(s->sev_out[slot], s->side));
    return 0;
}

int ar_wait(thip_solver *s, int slot)
{
    if (s->overlap != 2) return 0;
    if (s->use_gates) {
        hipLaunchKernelGGL(gate_k, dim3(1), dim3(1), 0, ctx().stream, s->gflags + 4 + slot, s->gseq[slot], s->gate_ticks,
                           s->gflags + 8, &s->dst->stop);
        THIP_LAUNCH_CHECK();
        return 0;
    }
    THIP_TRY(hipStreamWaitEvent(ctx().stream, s->sev_out[slot], 0));
    return 0;
}

int products_cols(thip_solver *s, const float *xn, const float *xt, GemvPartials *gp, int half)
{
    hipStream_t st = ctx().stream;
    prof_begin(st);
    THIP_RC(dual_gemv_partials_cols(st, s->m, s->n, s->sa.in_use(), xn, xt, true, true, false, s->gemv_scr, s->gemv_scr_n, gp,
                                    &s->dst->stop, s->hint_in_use(), half ? s->n1 : 0, half ? s->n : s->n1,
                                    half ? s->rows1 : 0, s->rows1 + s->rows2, nullptr));
    prof_end(st);
    return 0;
}

struct SplitCtx {
    thip_solver *s; hipStream_t st; int m; unsigned g; size_t n1, n2;
    float *partX, *partC, *part_y, *kx, *ky, *ks, *ku, *kv; float ez;
};

SplitCtx split_ctx(thip_solver *s)
{
    SplitCtx c;
    c.s = s; c.st = ctx().stream; c.m = (int)s->m; c.g = egrid(s->n > s->m ? s->n : s->m);
    c.n1 = s->n1; c.n2 = s->n - s->n1;
    c.partX = s->part; c.partC = s->part + 2 * NPS; c.part_y = s->part + 4 * PG;
    const bool k = s->comp();
    c.kx = k ? s->kx : nullptr; c.ky = k ? s->ky : nullptr; c.ks = k ? s->ks : nullptr;
    c.ku = k ? s->ku : nullptr; c.kv = k ? s->kv : nullptr;
    c.ez = s->par.eps_zero;
    return c;
}

// y update of one column range of u (+ the v rows, + kappa) and that range's share of the criteria sums
void split_ycrit(const SplitCtx &c, int half, int do_m, int do_kappa)
{
    thip_solver *s = c.s;
    const size_t c0 = half ? c.n1 : 0, len = half ? c.n2 : c.n1;
    hipLaunchKernelGGL(ycrit_k, dim3(c.g), dim3(BLK), 0, c.st, (int)len, c.m, 1, 1, 1, s->g3 + c0, s->h3, s->gP + c0, s->hP,
                       (const float *)nullptr, (const float *)nullptr, s->c + c0, s->b, s->rxs, s->Su + c0, s->Sv, s->u + c0,
                       s->v, s->xx + c0, c.ez, c.part_y, s->dst, c.partC, (int)(2 * NPS), s->g3 + s->n + NPS, (int)NPS,
                       1, do_m, do_kappa, half * (int)c.g, 2 * (int)c.g, c.ku ? c.ku + c0 : (float *)nullptr, c.kv);
}

// what iteration k leaves for after its last all-reduce: u[H2], kappa, the H2 share of the criteria, the termination test
int split_tail(thip_solver *s)
{
    const SplitCtx c = split_ctx(s);
    THIP_RC(ar_wait(s, 3));
    split_ycrit(c, 1, 0, 1);
    {
        const StatArgs sa{ 2 * (int)c.g, c.part_y, s->g3 + s->n + 2 * NPS, s->g3 + s->n + 3 * NPS, (int)NPS, nullptr, 0, nullptr, 0, nullptr,
                           s->par.eps_acc, s->par.eps_inf, c.ez, (long long)s->par.max_iter, s->xbuf };
        hipLaunchKernelGGL(status_k, dim3(1), dim3(BLK), 0, c.st, sa, s->dst);
    }
    THIP_LAUNCH_CHECK();
    s->tail_pending = false;
    return 0;
}

int one_iteration_split(thip_solver *s)
{
    const SplitCtx c = split_ctx(s);
    hipStream_t st = c.st;
    const int m = c.m;
    const size_t n = s->n, n1 = c.n1, n2 = c.n2;
    GemvPartials gp;
    // second reduction stage of one column range (+ the m-part and the sharded sums with the last range)
    auto post = [&](float *gvec, float *hvec, int half, const float *dn_b, const float *dm_b, int crit, float *prep) {
        const size_t c0 = half ? n1 : 0, len = half ? n2 : n1;
        hipLaunchKernelGGL(post_k, dim3(NPS), dim3(BLK), 0, st, (int)len, m, gp.partT + c0, gp.nT, gp.strideT, gvec + c0,
                           gp.partN, gp.nN, gp.strideN, hvec, s->c + c0, dn_b + c0, s->b, dm_b, crit, s->xs, s->xy, s->b,
                           c.ez, prep + (size_t)half * NPS, gvec + n, s->dst, half);
    };
    auto xupd = [&](int half, int do_m, int do_tau) {
        const size_t c0 = half ? n1 : 0, len = half ? n2 : n1;
        hipLaunchKernelGGL(xupdate_k, dim3(c.g), dim3(BLK), 0, st, (int)len, m, s->g1 + c0, s->h1, s->c + c0, s->b, s->v,
                           s->Tx + c0, s->Ty, s->Ts, s->cls, s->xx + c0, s->xy, s->xs, s->rxx + c0, s->rxy, s->rxs, s->dst,
                           c.partX, (int)(2 * NPS), s->g1 + n + NPS, (int)NPS, 1, do_m, do_tau,
                           c.kx ? c.kx + c0 : (float *)nullptr, c.ky, c.ks);
    };

    // ---- stage X, first half ----
    THIP_RC(products_cols(s, s->u, s->v, &gp, 0));
    post(s->g1, s->h1, 0, s->u, s->v, 0, c.partX);
    THIP_RC(ar_begin(s, 0, s->g1, n1));
    if (s->tail_pending) THIP_RC(split_tail(s));           // the previous iteration ends here
    // ---- stage X, second half ----
    THIP_RC(products_cols(s, s->u, s->v, &gp, 1));
    post(s->g1, s->h1, 1, s->u, s->v, 0, c.partX);
    THIP_RC(ar_begin(s, 1, s->g1 + n1, n2 + TAIL));
    THIP_RC(ar_wait(s, 0));
    xupd(0, 1, 0);
    THIP_RC(project_blocks(s));
    // ---- stage C, first half ----
    THIP_RC(products_cols(s, s->xx, s->xy, &gp, 0));
    post(s->g3, s->h3, 0, s->rxx, s->rxy, 0, c.partC);
    THIP_RC(ar_begin(s, 2, s->g3, n1));
    THIP_RC(ar_wait(s, 1));
    xupd(1, 0, 1);
    // ---- stage C, second half ----
    THIP_RC(products_cols(s, s->xx, s->xy, &gp, 1));
    post(s->g3, s->h3, 1, s->rxx, s->rxy, 1, c.partC);
    THIP_RC(ar_begin(s, 3, s->g3 + n1, n2 + TAIL));
    THIP_RC(ar_wait(s, 2));
    split_ycrit(c, 0, 1, 0);
    THIP_LAUNCH_CHECK();
    s->tail_pending = true;
    if (s->overlap != 2) THIP_RC(split_tail(s));           // in order: no skew
    return 0;
}

// Times the candidate tilings of the dual GEMV on THIS matrix (two launches each, the second one timed with HIP
// events) and keeps the fastest: a handful of passes over A, once per solve.  THIP_GEMV_AUTOTUNE=0 disables it.
int autotune_gemv(thip_solver *s)
{
    const char *env = getenv("THIP_GEMV_AUTOTUNE");
    if (s->autotune == 0 || (s->autotune < 0 && env && atoi(env) == 0) || getenv("THIP_GEMV_NJ") || getenv("THIP_GEMV_BLOCKS")) return 0;
    if (s->op != A_DENSE || s->m * s->n < (size_t)1 << 22) return 0;   // sparse, or tiny: nothing to tune
    const bool sp = s->split_plan;
    const DenseA A = s->sa.in_use();
    GemvPlan &plan = s->plan[A.is16()][sp];
    if (plan.tuned) return 0;
    hipStream_t st = ctx().stream;
    hipEvent_t e0, e1;
    THIP_TRY(hipEventCreate(&e0));
    THIP_TRY(hipEventCreate(&e1));
    int nc = 0;
    const GemvHint *c = gemv_candidates(&nc);
    float best = 1e30f;
    GemvPartials gp;
    GemvHint pick{0, 0};
    // one pass in the form the iteration will use: one launch, or (split) two launches over the column halves of the
    // candidate's own chunking
    auto one_pass = [&](const GemvHint *h) -> int {
        const size_t n1 = sp ? split_column(s) : 0;
        if (n1 == 0 || n1 >= s->n)
            return dual_gemv_partials(st, s->m, s->n, A, s->u, s->v, true, true, false, s->gemv_scr, s->gemv_scr_n, &gp, nullptr, h);
        const int r1 = dual_gemv_chunk_rows(s->m, n1, A, h, nullptr);
        const int r2 = dual_gemv_chunk_rows(s->m, s->n - n1, A, h, nullptr);
        THIP_RC(dual_gemv_partials_cols(st, s->m, s->n, A, s->u, s->v, true, true, false, s->gemv_scr, s->gemv_scr_n, &gp, nullptr, h,
                                        0, n1, 0, r1 + r2, nullptr));
        return dual_gemv_partials_cols(st, s->m, s->n, A, s->u, s->v, true, true, false, s->gemv_scr, s->gemv_scr_n, &gp, nullptr, h,
                                       n1, s->n, r1, r1 + r2, nullptr);
    };
    for (int w = 0; w < 3; ++w)         // clocks and caches settle before anything is timed
        THIP_RC(one_pass(nullptr));
    // inputs: the iterate if the loop is already running (storage switch), else zeros -- timing does not depend on them
    for (int i = 0; i < nc; ++i) {
        float ms = 1e30f;
        for (int rep = 0; rep < 5; ++rep) {
            THIP_TRY(hipEventRecord(e0, st));
            THIP_RC(one_pass(&c[i]));
            // the second reduction stage is part of the price of a plan (finer grids leave more partials to post_k):
            // time it too, into g2 / h2, which every schedule rewrites before reading
            THIP_RC(finalize_partials(st, s->m, gp.partN, gp.nN, gp.strideN, 1.0f, 0.0f, s->h2, nullptr));
            THIP_RC(finalize_partials(st, s->n, gp.partT, gp.nT, gp.strideT, 1.0f, 0.0f, s->g2, nullptr));
            THIP_TRY(hipEventRecord(e1, st));
            THIP_TRY(hipEventSynchronize(e1));
            float t = 0.0f;
            THIP_TRY(hipEventElapsedTime(&t, e0, e1));
            if (rep > 0 && t < ms) ms = t;
        }
        if (ms < best) { best = ms; pick = c[i]; }
    }
    set_gemv_plan(s, sp, pick, best);
    THIP_TRY(hipEventDestroy(e0));
    THIP_TRY(hipEventDestroy(e1));
    return 0;
}

// The carried schedule keeps gP = A^T x_y and hP = A x_x of the current iterate (ycrit_k).  After the stored form of A
// has been switched inside a solve (16-bit passes first, f32 passes to finish) they still hold the products with the
// OLD matrix: the first y-update would mix A_old and A_new, a one-off error of (A_old - A)^T x ~ 2^-9 .. 2^-12 relative,
// far above the step size near convergence.  Recompute them with the matrix now in use: one pass over A.
int rebuild_carried(thip_solver *s)
{
    s->carried_stale = false;
    if (!s->carried_like() || s->m == 0 || s->n == 0) return 0;
    hipStream_t st = ctx().stream;
    GemvPartials gp;
    THIP_RC(products(s, s->xx, s->xy, &gp, s->hP, s->gP));
    if (gp.nN >= 0) {      // dense: finish the partial sums (the sparse products are finished vectors already)
        THIP_RC(finalize_partials(st, s->m, gp.partN, gp.nN, gp.strideN, 1.0f, 0.0f, s->hP, nullptr));
        THIP_RC(finalize_partials(st, s->n, gp.partT, gp.nT, gp.strideT, 1.0f, 0.0f, s->gP, nullptr));
    }
    THIP_RC(do_allreduce(s, s->gP, s->n));
    return 0;
}

}  // namespace
