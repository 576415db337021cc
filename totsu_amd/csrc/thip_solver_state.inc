// thip_solver_state.inc -- part of thip_solver.hip: the solver object, the launch timers of bench.py's rooflines, the all-reduce hooks.

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------

// The operator the iteration applies, decided once by thip_solver_create / _set_csr / _set_sptile: a dense matrix (in one of its
// stored forms: StoredA), the CSR of A and of A^T, or ONE tiled copy serving both products (thip_sptile.hip)
enum OpKind { A_DENSE = 0, A_CSR2, A_TILED };
struct Csr2 { size_t nnz; const int64_t *rp, *trp; const int32_t *ci, *tci; const float *sv, *tsv; };

// The stored forms of a dense A and which one the iteration streams: the caller's f32 matrix (ld = m); a library-owned f32 copy
// with the leading dimension padded to a multiple of 16 floats (m % 16 != 0, e.g. the k = 500 SDP: m = 125 250; a 12 500-row shard),
// made by ensure_apad() when an f32 pass is about to run and the copy fits a third of the free HBM; ONE 16-bit copy at a time,
// library-owned (ld16 = m rounded to 8) or caller-built: kind16 = bf16 or scaled f16, inv_s = the f16 column scales
struct StoredA {
    size_t m = 0; const float *f32 = nullptr;
    float *pad = nullptr; size_t ldpad = 0;
    uint16_t *a16 = nullptr; size_t ld16 = 0; bool a16_owned = false; int kind16 = 0;
    float *inv_s = nullptr; bool inv_s_owned = false;
    int kind = THIP_A_F32;        // the form in use: THIP_A_F32, or the 16-bit copy's kind
    bool is16() const { return kind != THIP_A_F32; }
    // (pad_zero: rows m .. lda - 1 of the matrix in use are zeros written by this library -- its padded f32 copy, or a 16-bit copy it made)
    DenseA in_use() const
    {
        if (is16()) return DenseA{ a16, ld16, kind, kind == THIP_A_F16 ? inv_s : nullptr, a16_owned };
        return pad ? DenseA{ pad, ldpad, THIP_A_F32, nullptr, true } : DenseA{ f32, m, THIP_A_F32, nullptr, false };
    }
    hipError_t free_pad() { float *p = pad; pad = nullptr; ldpad = 0; return hipFree(p); }
    hipError_t free16()          // (a caller-built copy is only forgotten)
    {
        const hipError_t e0 = a16_owned ? hipFree(a16) : hipSuccess, e1 = inv_s_owned ? hipFree(inv_s) : hipSuccess;
        a16 = nullptr; inv_s = nullptr; a16_owned = inv_s_owned = false;
        return e0 != hipSuccess ? e0 : e1;
    }
};
// a tuned tiling of the dual GEMV and the time of one pass under it
struct GemvPlan { GemvHint hint{0, 0}; bool tuned = false; float ms = 0.0f; };

struct thip_solver {
    size_t n = 0, m = 0;
    const float *b = nullptr, *c = nullptr, *b_rowabs = nullptr;
    thip_param par{};
    int schedule = THIP_SCHED_FUSED;

    thip_allreduce_fn allreduce = nullptr;
    void *allreduce_ctx = nullptr;
    // overlap (thip_solver_set_overlap): 0 in order on the launch stream; 1 the stage's all-reduce on `side` (event in /
    // event out) under the stage's local-row work; 2 column-split pipeline (one_iteration_split); 3 the kernels of 2
    // with the collectives in order (its bitwise reference)
    int overlap = 0;
    hipStream_t side = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    hipEvent_t sev_in[4] = { nullptr, nullptr, nullptr, nullptr }, sev_out[4] = { nullptr, nullptr, nullptr, nullptr };
    size_t n1 = 0;                // split column of modes 2 / 3 (the same on every rank: a function of n); 0: no split
    int rows1 = 0, rows2 = 0;     // chunk rows of partial sums the two half-launches fill under the plan in use
    bool tail_pending = false;    // mode 2: the last column half of the y update + the termination test of the previous
                                  // iteration are still to be enqueued (they wait for its last all-reduce)
    long long spin_ticks = 0;     // thip_test_spin_allreduce
    // hand-offs of mode 2 through device flags instead of events (signal_k / gate_k): [0..3] "producer done", [4..7]
    // "collective done", [8] error word; values = per-slot call counters.  (Folding the signal into the producer's last
    // block and the gate into the consumer's entry was built and measured SLOWER, 848 vs 839 us: an agent-scope acquire
    // in every consumer block invalidates its XCD's L2.)
    bool use_gates = false;
    unsigned *gflags = nullptr;
    unsigned gseq[4] = { 0, 0, 0, 0 };
    long long gate_ticks = 0;

    OpKind op = A_DENSE;
    StoredA sa;
    Csr2 csr{};
    // the tiled copy (caller-held, possibly shared with other solvers) and this solver's launch state for it (spt_buffers): the
    // slices' shares of the N products go to sw_partH (the buffer the one-pass schedule's m-tail reads), those of the T products
    // to sw_partT; spt_xmax = the block maxima of the in-vectors of the product in flight (2 x SPT_NMAX floats)
    thip_sptile *spt = nullptr; float *sw_partT = nullptr, *spt_xmax = nullptr;

    // cone structure
    std::vector<int32_t> seg_type;
    std::vector<int64_t> seg_len;
    unsigned char *cls = nullptr;                 // per-row class for the element-wise cones
    int64_t *soc_beg = nullptr, *soc_end = nullptr; size_t n_soc = 0, soc_max = 0;
    int64_t *rot_beg = nullptr, *rot_end = nullptr; size_t n_rot = 0, rot_max = 0;
    int64_t *grp_beg = nullptr, *grp_end = nullptr; size_t n_grp = 0, grp_max = 0;
    std::vector<std::pair<int64_t, int64_t>> psd;  // (offset, packed length)
    // PSD cones of order <= 64, grouped by order: one launch projects the x_y and x_s blocks of every cone of a group
    struct PsdGroup { size_t k; int count; int64_t *dev_offs; };
    std::vector<PsdGroup> psd_groups;
    float *psd_work = nullptr; size_t psd_worklen = 0;

    // device vectors (one arena)
    float *arena = nullptr; size_t arena_n = 0;
    float *xx, *xy, *xs, *u, *v, *Tx, *Ty, *Ts, *Su, *Sv, *rxx, *rxy, *rxs;
    float *g1, *h1, *g2, *h2, *g3, *h3, *gP, *hP;
    // Kahan terms of the five iterate vectors (always allocated: O(n + m) floats); passed to the kernels when
    // par.state_arith == THIP_STATE_COMPENSATED, NULL (plain f32 additions) otherwise
    float *kx = nullptr, *ky = nullptr, *ks = nullptr, *ku = nullptr, *kv = nullptr;
    bool comp() const { return par.state_arith == THIP_STATE_COMPENSATED; }
    bool carried_like() const { return schedule == THIP_SCHED_CARRIED || schedule == THIP_SCHED_SWEEP; }
    size_t kahan_n = 0;                              // kx .. kv are contiguous: kahan_n floats from kx
    float *part = nullptr;                           // block partials (4 * EG)
    float *dotc = nullptr;                           // local scalars: [0] c.u, [1] c.rx_x, [2..3] dd,cx
    float *gemv_scr = nullptr; size_t gemv_scr_n = 0;
    // The tuned plans of the dual GEMV, one per stored element width and launch form: [16-bit copy in use][column split].  The
    // column-split form (overlap modes 2 / 3) has its own: a half-launch has half the workgroups of the whole-matrix launch, so
    // the best tiling differs (the 12 500 x 50 000 shard: ~1k tall tiles unsplit)
    GemvPlan plan[2][2];
    bool split_plan = false;      // the next run streams A as two column-half launches per pass
    int lda_pad = -1;             // thip_solver_set_lda_pad: -1 = default (16 floats, or THIP_LDA_PAD), 0 = never copy
    int autotune = -1;            // thip_solver_set_gemv_autotune: -1 = default (on, or THIP_GEMV_AUTOTUNE), 0 / 1
    const GemvPlan &plan_in_use() const { return plan[sa.is16()][split_plan]; }
    const GemvHint *hint_in_use() const { return plan_in_use().tuned ? &plan_in_use().hint : nullptr; }
    // THIP_SCHED_SWEEP (thip_sweep.hip): the second x_x buffer (x_x_{k+1} is formed while x_x_k is still the iterate), its
    // Kahan term, the groups' shares of the N products, the granule ring, the census words, block partials
    float *xx2 = nullptr, *kx2 = nullptr, *xx_home = nullptr, *kx_home = nullptr;
    int xbuf = 0;                 // which of the two buffers s->xx points at (0: the arena's own)
    SweepGeom sgeom{};
    int sweep_state = 0;          // 0 not examined, 1 usable, -1 not usable for this problem / device
    bool sw_first = true;         // the next sweep step starts from a consistent iterate (no u update, no test)
    float *sw_partH = nullptr; unsigned long long *sw_gran = nullptr; unsigned *sw_census = nullptr;
    float *sw_part = nullptr;     // 8 * EG block partials
    unsigned sw_seq = 0, sw_tag = 0;
    int sweep_pin = -1;           // thip_test_solver_pin_sweep_plan: the candidate geometry to install untimed (-1: the library's choice)
    float sw_plan_ms = 0.0f;      // the chosen geometry's time per sweep as measured by the plan autotune (0: not tuned)
    // column-sharded sweep (thip_solver_set_column_shard): this rank holds a block of COLUMNS of A (all m rows), the
    // n-vectors are its block, the m-vectors are replicated; one all-reduce per iteration of cs_buf = [A u (mpad) ;
    // A x_x (mpad) ; 4 x EG block partials of the sums over n]
    bool col_shard = false;
    float *cs_buf = nullptr; size_t cs_n = 0;
    size_t sweep_min_bytes = (size_t)128 << 20;     // thip_solver_set_sweep_min_bytes: smaller matrices run the carried schedule
    bool all_soc_short = false;   // every row belongs to a plain second-order cone of <= 129 rows (sw_cone_k)
    bool no_fold = false;         // thip_test_sweep_fault(kind 5): the termination test as a launch of its own in every iteration
    bool status_pending = false;  // the last enqueued iteration's termination test has not been evaluated yet (the next m-kernel's head does)
    int step_par = 0;             // parity of the tau / iter copies the next m-kernel reads
    int pm_par = 0;               // which of the two buffers of sums over m (sw_part + (4 + 4 par) EG) holds the latest
    int mtail_form = 0;           // the m-tail the last one-pass step launched (thip_test_solver_kahan): 0 none yet, 1 merged (sw_xm_k<MERGE>),
                                  // 2 a wave per cone (sw_cone_k), 3 three launches (sw_xm_k + block cones + sw_vm_k); + 4: one thread per row (FLAT)
    bool no_merge = false;        // thip_test_sweep_fault(kind 3): the two m-kernels of a step as two launches also without block cones
    int pn_par = 0;               // which of the two buffers of sums over n (sw_part + par * 2 EG) the LAST sweep wrote
    int pub_agent = -1;           // thip_solver_set_sweep_publish: 0 plain stores, 1 agent scope, -1 what the process's self-test said
    // recovery when the persistent kernel gives up (thip_solver_run): a device copy of the consistent iterate of the last
    // completed batch -- x_x, u, (x_y x_s v), their Kahan terms, the status block
    float *snap = nullptr; DevStatus *snap_st = nullptr; long long snap_iter = -1;
    size_t pn_len = 0, pm_len = 0;                  // padded lengths of an n- / m-vector of the arena
    unsigned *hflags = nullptr;                     // pinned: [0] sweep error word [1] gate error [2] one-shot error [3] DevStatus.fault
    int sweep_faults = 0; unsigned sweep_fault_word = 0; long long sweep_fault_iter = -1;
    int fault_kind = 0; long long fault_after = -1; int spin_max = 0;      // thip_test_sweep_fault
    DevStatus *dst = nullptr;
    DevStatus *hst = nullptr;                        // pinned
    bool inited = false;
    bool finalized = false;      // finalize_k has been applied to the terminated iterate
    bool carried_stale = false;  // the stored form of A changed under a running carried schedule: gP / hP must be rebuilt
};

namespace {

size_t pad64(size_t v) { return (v + 63) / 64 * 64; }

// The protocol of a column-sharded run, in ONE place -- thip_solver_run, sweep_prepare, the termination test and col_shard_abort
// (a rank that cannot plan its kernel and has to mirror its peers' collectives) must agree on it, or ranks end up in all-reduces
// of different lengths: the all-reduced buffer [A u (mpad) ; A x_x (mpad) ; 4 x EG sums over n ; fault flag + padding (64)] and
// the number of attempts every rank makes from the same snapshot before all of them return THIP_E_TIMEOUT.
constexpr int COL_SHARD_ATTEMPTS = 3;
inline size_t cs_flag_slot(size_t mpad) { return 2 * mpad + 4 * EG; }
inline size_t cs_floats(size_t mpad) { return cs_flag_slot(mpad) + 64; }

// optional per-launch timing of the dominant kernel (bench.py roofline): HIP event pairs recorded on the
// launch stream around every GEMV kernel of products()
struct Prof {
    bool on = false;
    int period = 1;                 // the spans of every period-th ITERATION are timed (an event pair costs the stream 3-5 us: 9 % of
                                    // a 0.14 ms iteration).  By iteration, not by span: a schedule with two kinds of span per iteration
                                    // (A^T pass then A pass; the two half-launches of the column split; the two products of the tiled
                                    // sparse copy) would otherwise, with an even period, only ever time one kind
    long long seen = 0;             // iterations begun since thip_prof_enable
    bool iter_open = true;          // the spans of the current iteration are timed
    bool open = false;              // the current span is one of the timed ones
    std::vector<hipEvent_t> ev;     // pairs
    size_t used = 0;
    double total_ms = 0.0;
    long long launches = 0;
} g_prof, g_prof_psd;      // the pass over A; the PSD cones' projection chains of an iteration (bench.py's roofline_eig)

void prof_begin(hipStream_t st, Prof &p = g_prof)
{
    if (!p.on) return;
    p.open = p.iter_open;
    if (!p.open) return;
    if (p.used + 2 > p.ev.size()) {
        for (int i = 0; i < 64; ++i) { hipEvent_t e; hipEventCreate(&e); p.ev.push_back(e); }
    }
    hipEventRecord(p.ev[p.used], st);
}
// once per iteration of thip_solver_run
void prof_tick()
{
    for (Prof *p : { &g_prof, &g_prof_psd })
        if (p->on) p->iter_open = (p->seen++ % p->period) == 0;
}
void prof_end(hipStream_t st, Prof &p = g_prof)
{
    if (!p.on || !p.open) return;
    hipEventRecord(p.ev[p.used + 1], st);
    p.used += 2;
    p.open = false;
}

}  // namespace
namespace thip {
void prof_release()
{
    for (Prof *p : { &g_prof, &g_prof_psd }) {
        for (hipEvent_t e : p->ev) hipEventDestroy(e);
        p->ev.clear();
        p->used = 0; p->on = false;
    }
}
}  // namespace thip
namespace {

int do_allreduce(thip_solver *s, float *buf, size_t count)
{
    if (!s->allreduce) return 0;
    const int rc = s->allreduce(s->allreduce_ctx, buf, count, (void *)ctx().stream);
    if (rc != 0) return fail(rc, "all-reduce callback failed", __FILE__, __LINE__);
    return 0;
}

// The all-reduce of a stage, optionally on the solver's side stream (overlap): begin = "the producer kernel has been
// enqueued on the launch stream": the side stream waits for it (event in) and runs the collective; end = the launch
// stream waits for the collective (event out) before the first consumer.  Whatever is enqueued on the launch stream
// between begin and end -- the stage's work on the local rows -- overlaps the collective.  Without overlap the
// collective is enqueued in order on the launch stream (begin) and end is a no-op.
int allreduce_begin(thip_solver *s, float *buf, size_t count)
{
    if (!s->allreduce) return 0;
    if (!(s->overlap == 1 || s->overlap == 2)) return do_allreduce(s, buf, count);
    hipStream_t st = ctx().stream;
    THIP_TRY(hipEventRecord(s->ev_in, st));
    THIP_TRY(hipStreamWaitEvent(s->side, s->ev_in, 0));
    const int rc = s->allreduce(s->allreduce_ctx, buf, count, (void *)s->side);
    if (rc != 0) return fail(rc, "all-reduce callback failed", __FILE__, __LINE__);
    THIP_TRY(hipEventRecord(s->ev_out, s->side));
    return 0;
}
int allreduce_end(thip_solver *s)
{
    if (!s->allreduce || !(s->overlap == 1 || s->overlap == 2)) return 0;
    THIP_TRY(hipStreamWaitEvent(ctx().stream, s->ev_out, 0));
    return 0;
}

unsigned egrid(size_t n) { return grid_for(n, BLK, EG); }

// EVERY change of the stored form of A goes through here; nothing else clears a plan's validity.  PLANS_F32: the padded f32 copy
// was freed, re-pitched or freshly made (the f32 plans were timed on the other pitch); PLANS_16: the library's 16-bit copy was
// (re)built in another format; both: the autotune was switched off (back to the shape heuristic); KIND: the form in use changed --
// the one-pass schedule is planned per stored form (another kernel instance), and inside a solve gP / hP of the carried
// schedules still hold products with the old matrix (rebuild_carried, by the next thip_solver_run)
enum { PLANS_F32 = 1, PLANS_16 = 2, KIND = 4 };
void stored_form_changed(thip_solver *s, unsigned what)
{
    if (what & PLANS_F32) s->plan[0][0].tuned = s->plan[0][1].tuned = false;
    if (what & PLANS_16) s->plan[1][0].tuned = s->plan[1][1].tuned = false;
    if (what & KIND) { s->sweep_state = 0; s->carried_stale = s->carried_stale || s->inited; }
}

int ensure_gemv_scratch(thip_solver *s)
{
    if (s->gemv_scr || s->op != A_DENSE || s->m == 0 || s->n == 0) return 0;
    s->gemv_scr_n = 2 * dual_gemv_scratch_floats(s->m, s->n);
    THIP_TRY(hipMalloc((void **)&s->gemv_scr, s->gemv_scr_n * sizeof(float)));
    return 0;
}

}  // namespace
