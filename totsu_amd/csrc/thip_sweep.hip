// thip_sweep.hip -- ONE pass over A per iteration of the conic loop (THIP_SCHED_SWEEP; dense f32 A on one GPU).
//
// The carried schedule reads A twice per iteration because the second pair of products takes the vectors the first pair
// produced (solver.rs:538-560: x_{k+1} needs K^T y_k, y_{k+1} needs K (x_k - 2 x_{k+1})).  But WHICH entries a product
// needs, and when they exist, is finer than that:
//   * x_x has no cone (solver.rs:546-549 project x_y and x_s only), so x_x_{k+1}[j] = x_x_k[j] + T_x[j] ((A^T v_k)[j] + c[j] kappa_k)
//     is known as soon as COLUMN j has been multiplied with v_k -- and column j is then still in registers for the
//     N product A x_x_{k+1} that the y update and the criteria want (solver.rs:125, 594);
//   * u has no projection either (solver.rs:562-567 clamp kappa only): u_k[j] = u_{k-1}[j] + S_u[j] (-(A^T rx_y_{k-1})[j] - c[j] rtau_{k-1})
//     needs column j times the m-vector x_y_k (carried form: A^T rx_y = A^T x_y_{k-1} - 2 A^T x_y_k), and then feeds
//     the N product A u_k of the next x update (solver.rs:149).
// So one sweep over the columns does, per column j: two dots (with v_k and with x_y_k), two scalar updates (u_k[j],
// x_x_{k+1}[j]), two axpys (A u_k, A x_x_{k+1}).  Everything else of the iteration is O(n + m) work between sweeps
// (thip_solver.hip: sw_* kernels).  The recurrences are the reference's, evaluated in a skewed order; no value is
// obtained differently from the carried schedule except for the order of the floating-point sums.
//
// The kernel.  A column (m floats, 400 KB at BASELINE configs[2]) does not fit one CU, and the dot must be complete
// before the axpy can start.  So G workgroups on one XCD form a GROUP (G = 8 or 16 at configs[2]; 1 .. 32, chosen by
// sweep_plan_one / timed by thip_solver.hip): a member owns a fixed range of rows -- its slices of v and x_y and its N
// accumulators live in registers for the whole sweep -- the group walks its share of the columns in PANELS of W = 1 or
// 2 columns, and the only thing that crosses CUs is an all-gather of the members' 2 W partial dots per panel through the
// L2 the group shares (8-byte {value, tag} granules: plain stores stay in that L2, sc1 loads are served by it; the
// hand-off thip_eig.hip's one-XCD Householder reduction uses).  A gather takes microseconds under load, a panel
// 1 - 2 us of HBM stream, so a panel stays ON THE CHIP from its loads to its axpy: a ring of LAGL + 1 register stages
// (statically indexed: the loop is unrolled by the ring length), then LS more panels parked in LDS by the thread that
// loaded them.  7 waves of a workgroup stream; the 8th is a service wave (publishes the workgroup's partial dots, gathers
// the group's granules, does the scalar updates, prefetches the per-column data): a polling wave has to drain its own
// loads (vmcnt is in order), so it must not be one that prefetches A.  What a geometry fixes is the BYTES a workgroup
// stages per panel (W x rows x 4): fewer members per group (more rows each, one column per panel) buy longer intervals
// for the service wave's dependent chain and fewer workgroups that can hold a group up -- 32 members with 2-column
// panels ran at 0.65 of the HBM peak, 8 members with 1-column panels at 0.85 - 0.89 (DESIGN.md 4.7 has the steps).
// An interval's cross-lane sums are DPP adds (streaming waves: per row of 16 lanes, the service wave adds the 7 x 4 row
// sums; the gather: the members of a quantity sit in an aligned block of lanes), never ds_bpermute chains, and the service
// wave runs at priority 3: at 16-bit storage an interval is ~1 us and that chain, not HBM, was what it waited for
// (DESIGN.md 4.8).
// Every spin is bounded; a workgroup that gives up raises the error word and the host reports a failed run.  A census at
// kernel entry (XCC_ID + tickets) checks that exactly 32 workgroups sit on every XCD -- i.e. one per CU, all resident --
// before anything is written; thip_solver.hip runs it once as a dry run and falls back to the carried schedule if the
// placement is not the expected one.
#include "thip_sweep_kernel.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <mutex>
#include <string>
#include <sys/stat.h>
#include <unistd.h>

using namespace thip;

namespace thip {

__global__ __launch_bounds__(SW_THREADS) void sweep_census_k(unsigned *census, unsigned seq)
{
    if (threadIdx.x == 0) { int g, mbr; (void)sw_census(census, seq, 32, &g, &mbr); }
}

}  // namespace thip

namespace thip {

namespace {
// THIP_SWEEP_CLASS (experiments): 0 = two columns per panel, 1 = one column per panel with twice the default group size,
// 2 / unset = the default geometry of sweep_plan_one(W = 1)
int sweep_class()
{
    static const int v = getenv("THIP_SWEEP_CLASS") ? atoi(getenv("THIP_SWEEP_CLASS")) : 2;
    return v >= 0 && v < 3 ? v : 0;
}
}  // namespace

// One candidate geometry: W columns per panel (1 or 2: the two families of kernel instances), the smallest group size
// the family's row capacity allows times gmul.  0 when the kernel can take the matrix that way.
// exact (thip_test_sweep's pin, thip_test_sweep_plan): force_G is THE group size -- any power of two up to 32 whose members' rows
// fit the family, also one below what the few-columns rule would raise it to (the kernel runs groups without columns; the rule is
// there so that no workgroup idles).  num_cu < 0: this device's.
static int sweep_plan_one(size_t m, size_t n, const DenseA &A, int W, int gmul, SweepGeom *g, int force_G = 0, bool exact = false,
                          int num_cu = -1)
{
    const int elem = A.kind;
    const size_t epv = A.vec_elems();                // rows per 16-byte slot
    if (m == 0 || n == 0 || m % epv != 0 || !A.vec_ok()) return 1;
    if (W != 1 && W != 2 && W != 4) return 1;
    if (m > 0x7fffffffull || n > ((size_t)1 << 30) || n < (size_t)40 * W) return 1;
    if ((num_cu < 0 ? ctx().num_cu : num_cu) != 256) return 1;
    const size_t slot_rows = (size_t)SW_CT * epv;
    // slots per streaming thread a kernel instance exists for: f32 1 .. 7 (one column per panel) / 1 .. 2 (two); 16-bit
    // storage keeps twice the rows per slot in registers (v, x_y, two accumulators: 32 VGPRs per slot): 1 .. 4 / 3 / 2
    const int max_slots = elem ? (W == 1 ? 4 : (W == 2 ? 3 : 2)) : (W == 1 ? 7 : 3);
    if (W == 4 && !elem) return 1;
    const size_t cap = slot_rows * max_slots;
    auto rows_of = [&](int G_) { return ((m + G_ - 1) / G_ + epv - 1) / epv * epv; };
    int G = 1;
    if (exact) {
        if (force_G < 1 || force_G > 32 || (force_G & (force_G - 1)) != 0 || rows_of(force_G) > cap) return 1;
        G = force_G;
    } else {
        while (G < 32 && rows_of(G) > cap) G *= 2;
        if (rows_of(G) > cap) return 1;
        for (int k = 1; k < gmul; k *= 2) { if (G >= 32) return 1; G *= 2; }
        // few columns: fewer, larger groups, so that every group has its 40 panels and no workgroup idles
        while (G < 32 && (size_t)(256 / G) * 40 * W > n) { if (gmul > 1) return 1; G *= 2; }
        if (force_G) {          // thip_test_sweep: a given group size (a power of two the rows fit)
            if (force_G < G || force_G > 32 || (force_G & (force_G - 1)) != 0) return 1;
            G = force_G;
        }
    }
    const size_t rpm = rows_of(G);
    const int ngroups = 256 / G;
    size_t cpg = (n + ngroups - 1) / ngroups;
    if (cpg < (size_t)40 * W) cpg = (size_t)40 * W;      // with few columns some groups idle
    cpg = (cpg + W - 1) / W * W;
    const int need = (int)((rpm + slot_rows - 1) / slot_rows);
    g->G = G; g->ngroups = ngroups; g->rows_per_member = (int)rpm; g->cols_per_group = (int)cpg;
    // 16-byte slots per streaming thread: what the member's rows need (round 3 offered 4 or 7 only: the 10 000 rows per member
    // of the n = 10 000 LP ran 7 slots at 80 % of their lanes, the 7 829 of the k = 500 SDP at 62 %)
    g->nslot = need;
    g->mpad = (m + 63) / 64 * 64;
    g->w = W; g->variant = 0;
    g->npan = (int)(cpg / W);
    g->m_eff = (int)m;
    g->elem = elem;
    return 0;
}

// geometry for an m x n matrix; 0 when the sweep kernel can take it.  The default: one column per panel, the fewest
// workgroups per column the rows allow (8 at BASELINE configs[2]); THIP_SWEEP_CLASS = 0 / 1 force the others.
// 16-bit storage: two columns per panel first (a 16-bit column is half the bytes: the interval of a one-column panel is
// too short for the service wave's chain)
int sweep_plan(size_t m, size_t n, const DenseA &A, SweepGeom *g)
{
    if (A.is16()) {
        // THIP_SWEEP16_GEOM = "W:gmul" pins the 16-bit geometry (experiments; with THIP_SWEEP_CLASS set so that the solver does not
        // time the candidates)
        if (const char *e = getenv("THIP_SWEEP16_GEOM")) {
            int w = 1, gm = 1;
            if (sscanf(e, "%d:%d", &w, &gm) == 2 && sweep_plan_one(m, n, A, w, gm, g) == 0) return 0;
        }
        if (sweep_plan_one(m, n, A, 2, 1, g) == 0) return 0;
        return sweep_plan_one(m, n, A, 1, 1, g);
    }
    const int cls = sweep_class();
    if (cls == 0 && sweep_plan_one(m, n, A, 2, 1, g) == 0) return 0;
    if (cls == 1 && sweep_plan_one(m, n, A, 1, 2, g) == 0) return 0;
    return sweep_plan_one(m, n, A, 1, 1, g);
}

// the geometries worth timing on a given matrix (thip_solver.hip times them on the actual matrix, like the GEMV plans)
static int sweep_candidates_on(size_t m, size_t n, const DenseA &A, SweepGeom *out, int max_out, int num_cu)
{
    static const int cand32[6][2] = { { 1, 1 }, { 1, 2 }, { 1, 4 }, { 2, 1 }, { 2, 2 }, { 1, 8 } };
    // (16-bit: one column per panel first since the interval's sums are DPP adds -- before, two columns were the safer default)
    static const int cand16[6][2] = { { 1, 1 }, { 4, 1 }, { 2, 1 }, { 2, 2 }, { 4, 2 }, { 1, 2 } };
    const int (*cand)[2] = A.is16() ? cand16 : cand32;
    int k = 0;
    for (int c = 0; c < 6 && k < max_out; ++c) {
        SweepGeom g;
        if (sweep_plan_one(m, n, A, cand[c][0], cand[c][1], &g, 0, false, num_cu) != 0) continue;
        bool dup = false;
        for (int j = 0; j < k; ++j) dup = dup || (out[j].G == g.G && out[j].w == g.w && out[j].nslot == g.nslot);
        if (!dup) out[k++] = g;
    }
    return k;
}
int sweep_candidates(size_t m, size_t n, const DenseA &A, SweepGeom *out, int max_out)
{
    return sweep_candidates_on(m, n, A, out, max_out, -1);
}

// the ring of every group + one spare 128-byte line per workgroup (the service wave's unconditional stores, thip_sweep_kernel.h)
size_t sweep_gran_words(const SweepGeom &g) { return (size_t)g.ngroups * SW_RING * g.G * (2 * g.w) + 256 * 16; }

int sweep_census_dry_run(hipStream_t st, unsigned *census, unsigned seq)
{
    hipLaunchKernelGGL(sweep_census_k, dim3(256), dim3(SW_THREADS), 0, st, census, seq);
    THIP_LAUNCH_CHECK();
    return 0;
}

int sweep_launch(hipStream_t st, const SweepGeom &g, const SweepArgs &a)
{
    if (g.elem != 0) return sweep_launch16(st, g, a);
    // <slots, columns per panel, LAGL, DLAG, LS>: 3 register stages + 3 LDS panels for every slot count.  Round 3's deeper
    // rings for few slots (9 stages + 5 .. 8 panels) and the 4 + 3 / 4 + 4 forms for 5 / 6 slots were timed against it
    // (profiles/r04_sweep_ring_depth_and_publish_scope.txt, r04_sweep_small_slot_ring_depth.txt): a launch runs
    // npan + LAGL + LS intervals and the last LAGL + LS load nothing -- 5 - 10 us per launch in favour of the shallow ring at
    // every slot count, nothing lost on long sweeps; one panel less (3 + 2) makes every gather poll once.
    if (g.w == 2) {
        // two columns per panel: half the column groups of the one-column geometry with the same bytes per panel (the m-tail
        // reads every group's share of the two N products: 20 MB at the n = 10 000 LP with 128 groups)
        switch (g.nslot) {
        case 1: return sweep_go<1, 2, 2, 1, 3>(st, a);
        case 2: return sweep_go<2, 2, 2, 1, 3>(st, a);
        default: return sweep_go<3, 2, 2, 1, 3>(st, a);
        }
    }
    switch (g.nslot) {
    case 1: return sweep_go<1, 1, 2, 1, 3>(st, a);
    case 2: return sweep_go<2, 1, 2, 1, 3>(st, a);
    case 3: return sweep_go<3, 1, 2, 1, 3>(st, a);
    case 4: return sweep_go<4, 1, 2, 1, 3>(st, a);
    case 5: return sweep_go<5, 1, 2, 1, 3>(st, a);
    case 6: return sweep_go<6, 1, 2, 1, 3>(st, a);
    default: return sweep_go<7, 1, 2, 1, 3>(st, a);
    }
}

}  // namespace thip

// ---------------------------------------------------------------------------------------------------
// thip_test_sweep: the kernel alone, for tests/test_gpu_sweep.py and tools (include/totsu_f32hip.h)
// ---------------------------------------------------------------------------------------------------
namespace {
__global__ void sw_test_reduce_k(int m, int ngroups, size_t mpad, const float *__restrict__ partH, float *__restrict__ hN,
                                 float *__restrict__ h3)
{
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)m; i += (size_t)gridDim.x * blockDim.x) {
        float a = 0.0f, b = 0.0f;
        for (int g = 0; g < ngroups; ++g) { a += partH[((size_t)g * 2 + 0) * mpad + i]; b += partH[((size_t)g * 2 + 1) * mpad + i]; }
        hN[i] = a; h3[i] = b;
    }
}
}  // namespace

static int run_test_sweep(const thip_sweep_test *t, int spin_max, float *host_ms, int *host_info)
{
    if (!t) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    SweepGeom g;
    if (t->elem < 0 || t->elem > THIP_A_F16 || (t->elem == THIP_A_F16 && !t->inv_s))
        return fail(THIP_E_INVALID, "bad element kind", __FILE__, __LINE__);
    // 16-bit: `variant` = columns per panel (1, 2 or 4; else the planner's preference)
    // (f32: variant 12 = two columns per panel)
    const int w16 = t->elem ? ((t->variant == 1 || t->variant == 2 || t->variant == 4) ? t->variant : 0) : (t->variant == 12 ? 2 : 0);
    const DenseA A{ t->mat_a, t->lda, t->elem, t->inv_s, false };
    if (t->pin_g != 0) {
        // the exact geometry: pin_w columns per panel, pin_g members per group, or nothing is launched
        if (!t->mat_a || t->lda < t->m || sweep_plan_one(t->m, t->n, A, t->pin_w, 1, &g, t->pin_g, true) != 0)
            return fail(THIP_E_INVALID, "the one-pass kernel has no instance for the pinned geometry on this shape", __FILE__, __LINE__);
    } else
    if (w16 ? sweep_plan_one(t->m, t->n, A, w16, 1, &g, t->force_members) != 0
        : (t->force_members > 0 ? sweep_plan_one(t->m, t->n, A, t->elem ? 2 : 1, 1, &g, t->force_members)
                                : sweep_plan(t->m, t->n, A, &g)) != 0)
        return fail(THIP_E_INVALID, "the one-pass kernel cannot take this shape", __FILE__, __LINE__);
    hipStream_t st = ctx().stream;
    unsigned long long *gran = nullptr;
    unsigned *census = nullptr;
    float *partH = nullptr, *scal = nullptr, *pnbuf = nullptr;
    THIP_TRY(hipMalloc((void **)&gran, sweep_gran_words(g) * sizeof(unsigned long long)));
    THIP_TRY(hipMalloc((void **)&census, 160 * sizeof(unsigned)));
    THIP_TRY(hipMalloc((void **)&partH, (size_t)g.ngroups * 2 * g.mpad * sizeof(float)));
    THIP_TRY(hipMalloc((void **)&scal, 4 * sizeof(float)));
    THIP_TRY(hipMalloc((void **)&pnbuf, 4 * 256 * sizeof(float)));
    THIP_TRY(hipMemsetAsync(pnbuf, 0, 4 * 256 * sizeof(float), st));
    THIP_TRY(hipMemsetAsync(gran, 0, sweep_gran_words(g) * sizeof(unsigned long long), st));
    THIP_TRY(hipMemsetAsync(census, 0, 160 * sizeof(unsigned), st));
    THIP_TRY(hipMemsetAsync(partH, 0, (size_t)g.ngroups * 2 * g.mpad * sizeof(float), st));
    const float hs[4] = { 0.0f, t->kappa, t->rtau, 1.0f };       // [0] doubles as the stop flag (int 0)
    THIP_TRY(hipMemcpyAsync(scal, hs, sizeof(hs), hipMemcpyHostToDevice, st));
    SweepArgs a;
    a.A = t->mat_a; a.lda = t->lda; a.m = (int)t->m; a.n = (int)t->n; a.inv_s = t->inv_s;
    a.G = g.G; a.rows_per_member = g.rows_per_member; a.cols_per_group = g.cols_per_group;
    a.v = t->v; a.xy = t->xy; a.c = t->c; a.Su = t->su; a.Tx = t->tx; a.u = t->u; a.ku = t->ku;
    a.xx_in = t->xx_in; a.kx_in = t->kx_in; a.xx_out = t->xx_out; a.kx_out = t->kx_out; a.gP = t->gp;
    a.partH = partH; a.mpad = g.mpad; a.gran = gran; a.census = census;
    a.first = t->first;
    a.pn = pnbuf; a.pn_stride = 256; a.tau_p = scal + 3; a.eps_zero = 1e-12f;          // tau = 1: d = c + A^T x_y
    a.kappa_out = nullptr; a.skappa_p = nullptr; a.pm_brx = nullptr; a.np_m = 0; a.pn_count = 0;
    a.pn_in = nullptr; a.pn_in_stride = 0; a.spin_max = spin_max; a.fault = 0; a.pub_agent = t->pub_agent != 0;
    a.dbg = getenv("THIP_SWEEP_DBG") ? atoi(getenv("THIP_SWEEP_DBG")) : 0;
    a.stop = reinterpret_cast<const int *>(scal); a.kappa_p = scal + 1; a.rtau_p = scal + 2;
    unsigned seq = 0, tagbase = 0;
    THIP_RC(sweep_census_dry_run(st, census, seq++));
    hipEvent_t e0, e1;
    THIP_TRY(hipEventCreate(&e0)); THIP_TRY(hipEventCreate(&e1));
    const int reps = t->reps > 0 ? t->reps : 1;
    float best = 1e30f, tot = 0.0f;
    for (int r = 0; r < reps; ++r) {
        a.seq = seq++; a.tagbase = tagbase; tagbase += (unsigned)g.npan + 1u;
        THIP_TRY(hipEventRecord(e0, st));
        THIP_RC(sweep_launch(st, g, a));
        THIP_TRY(hipEventRecord(e1, st));
        THIP_TRY(hipEventSynchronize(e1));
        float ms = 0.0f;
        THIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        tot += ms; if (ms < best) best = ms;
    }
    hipLaunchKernelGGL(sw_test_reduce_k, dim3(256), dim3(256), 0, st, (int)t->m, g.ngroups, g.mpad, partH, t->hn, t->h3);
    THIP_LAUNCH_CHECK();
    unsigned hc[160];
    float hpn[4 * 256];
    THIP_TRY(hipMemcpyAsync(hc, census, sizeof(hc), hipMemcpyDeviceToHost, st));
    THIP_TRY(hipMemcpyAsync(hpn, pnbuf, sizeof(hpn), hipMemcpyDeviceToHost, st));
    THIP_TRY(hipStreamSynchronize(st));
    if (t->host_sums) {
        // the workgroups' partial sums over n of the last launch, added up: ||d||^2, c.x_x, c.u, c.(x_x - 2 x_x')
        for (int q = 0; q < 4; ++q) {
            double acc = 0.0;
            for (int k = 0; k < 256; ++k) acc += (double)hpn[q * 256 + k];
            t->host_sums[q] = (float)acc;
        }
    }
    if (host_ms) { host_ms[0] = best; host_ms[1] = tot / reps; }
    if (host_info) {
        host_info[0] = (int)hc[9]; host_info[1] = g.G; host_info[2] = g.ngroups; host_info[3] = g.npan; host_info[4] = g.nslot;
        host_info[5] = (int)hc[18]; host_info[6] = (int)hc[19]; host_info[7] = g.w;
    }
#ifdef SW_PROFILE
    fprintf(stderr, "service wave, 10 ns ticks: wait %u, cold+publish %u, tags+poll %u, reduce+math+stores %u, loads %u, barrier %u; intervals that polled %u, polls %u\n",
            hc[10], hc[11], hc[12], hc[13], hc[14], hc[15], hc[16], hc[17]);
    if (getenv("SW_PROFILE_MISSES"))
        for (int i = 0; i < 5; ++i) fprintf(stderr, "miss %d: panel %u lanes %08x%08x\n", i, hc[24 + 3 * i], hc[26 + 3 * i], hc[25 + 3 * i]);
    fprintf(stderr, "streaming wave 0 of workgroup (0, 0), us since kernel entry: census done %.2f, v / x_y loaded %.2f, fill done %.2f, steady loop done %.2f, drain done %.2f, stores done %.2f\n",
            hc[150] * 0.01, hc[151] * 0.01, hc[152] * 0.01, hc[153] * 0.01, hc[154] * 0.01, hc[155] * 0.01);
#endif
    hipEventDestroy(e0); hipEventDestroy(e1);
    hipFree(gran); hipFree(census); hipFree(partH); hipFree(scal); hipFree(pnbuf);
    return 0;
}

extern "C" int thip_test_sweep(const thip_sweep_test *t, float *host_ms, int *host_info)
{
    THIP_NEED_INIT();
    return run_test_sweep(t, SW_SPIN_MAX, host_ms, host_info);
}

// the planning alone (totsu_f32hip_test.h): no GPU, no thip_init -- a device of 256 CUs is assumed
static void sweep_plan_record(const SweepGeom &g, thip_sweep_plan_rec *r)
{
    r->members = g.G; r->ngroups = g.ngroups; r->rows_per_member = g.rows_per_member; r->cols_per_group = g.cols_per_group;
    r->npan = g.npan; r->nslot = g.nslot; r->cols_per_panel = g.w; r->elem = g.elem;
    r->mpad = g.mpad; r->gran_words = sweep_gran_words(g);
}

extern "C" int thip_test_sweep_plan(size_t m, size_t n, size_t lda, int elem, int cols_per_panel, int gmul, int force_members,
                                    thip_sweep_plan_rec *host_plan, thip_sweep_plan_rec *host_candidates, int *host_n_candidates)
{
    if (elem < 0 || elem > THIP_A_F16 || gmul < 1 || force_members < 0 || lda < m)
        return fail(THIP_E_INVALID, "bad argument", __FILE__, __LINE__);
    // (the matrix itself is not needed: any 16-byte aligned address stands for it)
    const DenseA A{ reinterpret_cast<const void *>((uintptr_t)4096), lda, elem, nullptr, false };
    if (host_candidates || host_n_candidates) {
        SweepGeom cand[6];
        const int nc = sweep_candidates_on(m, n, A, cand, 6, 256);
        if (host_candidates) for (int c = 0; c < nc; ++c) sweep_plan_record(cand[c], host_candidates + c);
        if (host_n_candidates) *host_n_candidates = nc;
    }
    if (host_plan) {
        SweepGeom g;
        if (sweep_plan_one(m, n, A, cols_per_panel, gmul, &g, force_members, force_members > 0, 256) != 0)
            return fail(THIP_E_INVALID, "the one-pass kernel has no instance for this geometry on this shape", __FILE__, __LINE__);
        sweep_plan_record(g, host_plan);
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// The publish-scope self-test (round 5).  The groups' partial dots travel through granules that the publisher stores at
// WAVEFRONT scope (a plain store that stays in the XCD's L2, which all members of a group share) and the gatherers read
// with agent-scope loads: outside the memory model's guarantees, kept because it measured 3-5 % faster than the documented
// sc1 form and has never failed.  What would make it fail is a change of the L2's write policy under it (driver, firmware):
// the store would sit in a place the gatherers' loads do not look, every gather would poll until its bound, and a solve
// would limp from time-out to time-out.  So, once per process, before the first plan: SELFTEST_SWEEPS idempotent sweeps of
// a scratch 32 768 x 512 matrix (64 MB) with 32 members per group (64 intervals each: ~400 000 granule hand-offs, ~10 ms),
// a short polling bound, and the kernel's own poll counters.  A hand-off that is merely late polls a few times; one that is
// not visible polls to the bound.  Error word raised, or any gather needing more than SELFTEST_MAX_POLLS: every solver of
// this process publishes at agent scope (slower, inside the model) -- thip_solver_set_sweep_publish overrides either way.
// ---------------------------------------------------------------------------------------------------
namespace {
constexpr int SELFTEST_SWEEPS = 200, SELFTEST_SPIN = 50000, SELFTEST_MAX_POLLS = 4096;
std::atomic<int> g_pub_state{ -1 };   // -1 not run, 0 wavefront-scope publish passed, 1 agent scope (failed, or no 8 x 32 device)
std::mutex g_pub_mutex;               // solvers on several host threads: one of them runs the self-test, the others wait for it
int g_pub_info[4] = { 0, 0, 0, 0 };   // error word, polls summed, most polls of one gather, sweeps run (0: verdict read from the cache file)
int g_pub_force_fail = 0;

// The verdict is a property of (device, driver, runtime): it is kept in a file so that a process does not spend 52 ms (200 sweeps
// of 252 us: 1.5 % of the k = 500 SDP's 3.5 s time-to-eps) on it at every start.  $THIP_CACHE_DIR, else $XDG_CACHE_HOME/totsu_f32hip,
// else ~/.cache/totsu_f32hip; the file name carries device name, PCI bus, driver and runtime versions (a driver change under the
// library is what the test exists for: it changes the key).  A FAILED verdict is trusted for a day only.
std::string publish_cache_path()
{
    const char *dir = getenv("THIP_CACHE_DIR");
    std::string base;
    if (dir && *dir) base = dir;
    else if (getenv("XDG_CACHE_HOME") && *getenv("XDG_CACHE_HOME")) base = std::string(getenv("XDG_CACHE_HOME")) + "/totsu_f32hip";
    else if (getenv("HOME") && *getenv("HOME")) base = std::string(getenv("HOME")) + "/.cache/totsu_f32hip";
    else return std::string();
    hipDeviceProp_t prop;
    int drv = 0, rt = 0;
    if (hipGetDeviceProperties(&prop, ctx().device) != hipSuccess) { (void)hipGetLastError(); return std::string(); }
    (void)hipDriverGetVersion(&drv); (void)hipRuntimeGetVersion(&rt);
    char name[512];
    snprintf(name, sizeof(name), "publish_scope_%s_%s_bus%02x_drv%d_rt%d", prop.name, prop.gcnArchName, prop.pciBusID, drv, rt);
    for (char *c = name; *c; ++c) if (!((*c >= 'a' && *c <= 'z') || (*c >= 'A' && *c <= 'Z') || (*c >= '0' && *c <= '9') || *c == '_')) *c = '-';
    (void)mkdir(base.substr(0, base.find_last_of('/')).c_str(), 0755);
    (void)mkdir(base.c_str(), 0755);
    return base + "/" + name;
}
int publish_cache_read()
{
    static const int off = getenv("THIP_NO_CACHE") ? atoi(getenv("THIP_NO_CACHE")) : 0;
    if (off) return -1;
    const std::string p = publish_cache_path();
    if (p.empty()) return -1;
    FILE *f = fopen(p.c_str(), "r");
    if (!f) return -1;
    int verdict = -1; long long when = 0;
    const int got = fscanf(f, "%d %lld", &verdict, &when);
    fclose(f);
    if (got != 2 || (verdict != 0 && verdict != 1)) return -1;
    if (verdict == 1 && (long long)time(nullptr) - when > 86400) return -1;
    return verdict;
}
void publish_cache_write(int verdict)
{
    static const int off = getenv("THIP_NO_CACHE") ? atoi(getenv("THIP_NO_CACHE")) : 0;
    if (off) return;
    const std::string p = publish_cache_path();
    if (p.empty()) return;
    const std::string tmp = p + ".tmp" + std::to_string((long long)getpid());
    FILE *f = fopen(tmp.c_str(), "w");
    if (!f) return;
    fprintf(f, "%d %lld\n", verdict, (long long)time(nullptr));
    fclose(f);
    (void)rename(tmp.c_str(), p.c_str());
}

int publish_selftest_run()
{
    const size_t m = 32768, n = 512;
    float *A = nullptr, *vec = nullptr;
    g_pub_info[0] = g_pub_info[1] = g_pub_info[2] = g_pub_info[3] = 0;
    if (hipMalloc((void **)&A, m * n * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); g_pub_state = 1; return 0; }
    const size_t nv = 6 * m + 12 * n;
    if (hipMalloc((void **)&vec, nv * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); hipFree(A); g_pub_state = 1; return 0; }
    hipStream_t st = ctx().stream;
    if (hipMemsetAsync(A, 0, m * n * sizeof(float), st) != hipSuccess || hipMemsetAsync(vec, 0, nv * sizeof(float), st) != hipSuccess) {
        (void)hipGetLastError(); hipFree(A); hipFree(vec); g_pub_state = 1; return 0;
    }
    thip_sweep_test t;
    memset(&t, 0, sizeof(t));
    float *p = vec;
    auto take = [&](size_t k) { float *q = p; p += k; return q; };
    t.m = m; t.n = n; t.lda = m; t.mat_a = A;
    t.v = take(m); t.xy = take(m); t.hn = take(m); t.h3 = take(m); p += 2 * m;
    t.c = take(n); t.su = take(n); t.tx = take(n); t.u = take(n); t.ku = take(n); t.xx_in = take(n); t.kx_in = take(n);
    t.xx_out = take(n); t.kx_out = take(n); t.gp = take(n);
    t.kappa = 0.0f; t.rtau = 1.0f; t.first = 1; t.reps = SELFTEST_SWEEPS; t.force_members = 32; t.pub_agent = 0;
    int info[8] = { 0 };
    float ms[2];
    const int rc = run_test_sweep(&t, SELFTEST_SPIN, ms, info);
    const hipError_t se = hipStreamSynchronize(st);
    hipFree(A); hipFree(vec);
    if (se != hipSuccess) { (void)hipGetLastError(); g_pub_state = 1; g_pub_info[0] = -1; return 0; }
    if (rc != 0) { g_pub_state = 1; g_pub_info[0] = -1; return 0; }      // no 8 x 32 placement, or the shape was refused: the documented form
    g_pub_info[0] = info[0]; g_pub_info[1] = info[5]; g_pub_info[2] = info[6]; g_pub_info[3] = SELFTEST_SWEEPS;
    const bool ok = info[0] == 0 && info[6] <= SELFTEST_MAX_POLLS && !g_pub_force_fail;
    g_pub_state = ok ? 0 : 1;
    return 0;
}
}  // namespace

namespace thip {
// 0: partial dots published with plain stores (the self-test passed), 1: at agent scope
int sweep_publish_default()
{
    if (g_pub_state.load() < 0) {
        std::lock_guard<std::mutex> lock(g_pub_mutex);
        if (g_pub_state.load() < 0) {
            static const int env = getenv("THIP_SWEEP_PUBLISH") ? atoi(getenv("THIP_SWEEP_PUBLISH")) : -1;      // 0 / 1: no self-test
            const int cached = (env == 0 || env == 1) ? -1 : publish_cache_read();
            if (env == 0 || env == 1) g_pub_state = env;
            else if (cached >= 0) g_pub_state = cached;
            else {
                if (publish_selftest_run() != 0) g_pub_state = 1;
                publish_cache_write(g_pub_state.load());
            }
        }
    }
    return g_pub_state.load();
}
}  // namespace thip

extern "C" int thip_sweep_publish_selftest(int mode, int *host_agent_scope, int *host_info)
{
    THIP_NEED_INIT();
    // mode 0: the cached verdict (run now if it has not been); 1: run again; 2: run again and treat it as FAILED (test hook)
    if (mode < 0 || mode > 2) return fail(THIP_E_INVALID, "thip_sweep_publish_selftest: mode 0, 1 or 2", __FILE__, __LINE__);
    if (mode != 0) {
        // (a forced run is a test's: its verdict does not go to the cache file)
        std::lock_guard<std::mutex> lock(g_pub_mutex);
        g_pub_force_fail = mode == 2; THIP_RC(publish_selftest_run()); g_pub_force_fail = 0;
    }
    const int v = sweep_publish_default();
    if (host_agent_scope) *host_agent_scope = v;
    if (host_info) for (int i = 0; i < 4; ++i) host_info[i] = g_pub_info[i];
    return 0;
}

// Can the one-pass kernel run on THIS device for an m x n_local block (leading dimension lda)?  Geometry + one placement
// census, no collective: a multi-rank host asks every rank and takes the minimum BEFORE it builds column-sharded solvers
// (a rank that found out inside thip_solver_init would leave the others waiting in their first all-reduce).
// elem = the stored form the run will stream (THIP_A_F32 / _BF16 / _F16): a 16-bit plan has 8 rows per slot and its own caps.
extern "C" int thip_sweep_probe(size_t m, size_t n_local, size_t lda, int elem, int *host_ok)
{
    THIP_NEED_INIT();
    if (!host_ok || elem < 0 || elem > 2) return fail(THIP_E_INVALID, "bad argument", __FILE__, __LINE__);
    *host_ok = 0;
    SweepGeom g;
    const size_t epv = elem ? 8 : 4;              // rows per 16-byte vector: the library's own copy pads rows and pitch to it
    // (the matrix itself is not needed: any 16-byte aligned address stands for it)
    const DenseA A{ reinterpret_cast<const void *>((uintptr_t)4096), (lda + epv - 1) / epv * epv, elem, nullptr, false };
    if (sweep_plan((m + epv - 1) / epv * epv, n_local, A, &g) != 0) return 0;
    unsigned *census = nullptr;
    THIP_TRY(hipMalloc((void **)&census, 16 * sizeof(unsigned)));
    hipStream_t st = ctx().stream;
    THIP_TRY(hipMemsetAsync(census, 0, 16 * sizeof(unsigned), st));
    THIP_RC(sweep_census_dry_run(st, census, 0));
    unsigned hc[10];
    THIP_TRY(hipMemcpyAsync(hc, census, sizeof(hc), hipMemcpyDeviceToHost, st));
    THIP_TRY(hipStreamSynchronize(st));
    hipFree(census);
    *host_ok = hc[9] == 0u ? 1 : 0;
    return 0;
}

// ---------------------------------------------------------------------------------------------------
// thip_stream_probe: what THIS device streams -- a bare non-temporal read of `bytes` at dev_ptr (16-byte aligned; e.g. the
// solver's own A), eight 16-byte loads in flight per lane, nothing else.  bench.py prints it beside the sweep's rate, so
// that "fraction of what the box can read" is known for the box a line was measured on (boxes of one pool differ by 7 %).
// ---------------------------------------------------------------------------------------------------
namespace {
__global__ __launch_bounds__(256) void stream_read_k(const f32x4 *__restrict__ p, size_t n4, float *out)
{
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    f32x4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (; i + 7 * stride < n4; i += 8 * stride) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(p + i + u * stride);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; i < n4; i += stride) acc += __builtin_nontemporal_load(p + i);
    const float s = acc[0] + acc[1] + acc[2] + acc[3];
    if (s == 123.456f) out[0] = s;      // keeps the loads alive
}

// the same bytes as 32 KB contiguous pieces per workgroup and step (what a persistent kernel's workgroup reads per column):
// DRAM pages are walked in longer runs than by the grid-stride form; the probe reports the better of the two
__global__ __launch_bounds__(256) void stream_read_chunks_k(const f32x4 *__restrict__ p, size_t n4, float *out)
{
    constexpr size_t CH = 256 * 8;                  // 16-byte vectors per chunk
    const size_t nch = n4 / CH;
    f32x4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
    for (size_t c = blockIdx.x; c < nch; c += gridDim.x) {
        const f32x4 *q = p + c * CH + threadIdx.x;
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = __builtin_nontemporal_load(q + u * 256);
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (size_t i = nch * CH + (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) acc += __builtin_nontemporal_load(p + i);
    const float s = acc[0] + acc[1] + acc[2] + acc[3];
    if (s == 123.456f) out[0] = s;
}
// the access pattern of the one-pass kernel itself, without its arithmetic: 256 persistent workgroups of 512 threads, 56 KB
// contiguous per workgroup and step, three steps (21 loads per lane) in flight
__global__ __launch_bounds__(512) void stream_read_persistent_k(const f32x4 *__restrict__ p, size_t n4, float *out)
{
    constexpr size_t CH = 512 * 7;
    const size_t nch = n4 / CH;
    f32x4 acc = { 0.0f, 0.0f, 0.0f, 0.0f };
    f32x4 v[3][7];
    size_t c = blockIdx.x;
    const size_t step = gridDim.x;
#define SRP_LOAD(S, C_) do { const f32x4 *q = p + (C_) * CH + threadIdx.x; _Pragma("unroll") for (int u = 0; u < 7; ++u) v[S][u] = __builtin_nontemporal_load(q + u * 512); } while (0)
#define SRP_USE(S) do { _Pragma("unroll") for (int u = 0; u < 7; ++u) acc += v[S][u]; } while (0)
    if (c < nch) SRP_LOAD(0, c);
    if (c + step < nch) SRP_LOAD(1, c + step);
    for (; c + 4 * step < nch; c += 3 * step) {
        SRP_LOAD(2, c + 2 * step); SRP_USE(0);
        SRP_LOAD(0, c + 3 * step); SRP_USE(1);
        SRP_LOAD(1, c + 4 * step); SRP_USE(2);
    }
    // tail: at most four chunks of this workgroup are left, two of them loaded
    if (c < nch) SRP_USE(0);
    if (c + step < nch) SRP_USE(1);
    for (size_t d = c + 2 * step; d < nch; d += step) { SRP_LOAD(2, d); SRP_USE(2); }
#undef SRP_LOAD
#undef SRP_USE
    for (size_t i = nch * CH + (size_t)blockIdx.x * 512 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 512) acc += __builtin_nontemporal_load(p + i);
    const float s_ = acc[0] + acc[1] + acc[2] + acc[3];
    if (s_ == 123.456f) out[0] = s_;
}
}  // namespace

extern "C" int thip_stream_probe(const void *dev_ptr, size_t bytes, int reps, float *host_best_ms, float *host_avg_ms)
{
    THIP_NEED_INIT();
    if (!dev_ptr || bytes < 16 || ((uintptr_t)dev_ptr & 15u) != 0) return fail(THIP_E_INVALID, "bad buffer", __FILE__, __LINE__);
    hipStream_t st = ctx().stream;
    const size_t n4 = bytes / 16;
    hipEvent_t e0, e1;
    THIP_TRY(hipEventCreate(&e0)); THIP_TRY(hipEventCreate(&e1));
    if (reps < 1) reps = 1;
    float best = 1e30f, best_avg = 1e30f;
    // grid-stride form at the grids tools/stream_probe.hip found within 2 % of each other at 0.4 - 20 GB, the chunked form at 8
    // and 16 resident workgroups per CU, the persistent form at one and two workgroups per CU; one warm-up each; the best
    // form's best and average launch
    const unsigned grids[7] = { 4096u, 8192u, 16384u, 2048u, 4096u, 256u, 512u };
    for (int f = 0; f < 7; ++f) {
        const unsigned blocks = grids[f];
        const int form = f < 3 ? 0 : (f < 5 ? 1 : 2);        // grid-stride / 32 KB chunks / persistent 56 KB chunks, 3 in flight
        if ((size_t)blocks * 256 * 8 > n4 && f != 0) continue;
        float tot = 0.0f, mn = 1e30f;
        for (int r = 0; r <= reps; ++r) {
            THIP_TRY(hipEventRecord(e0, st));
            const f32x4 *src = reinterpret_cast<const f32x4 *>(dev_ptr);
            if (form == 2) hipLaunchKernelGGL(stream_read_persistent_k, dim3(blocks), dim3(512), 0, st, src, n4, ctx().dev_scalar);
            else if (form == 1) hipLaunchKernelGGL(stream_read_chunks_k, dim3(blocks), dim3(256), 0, st, src, n4, ctx().dev_scalar);
            else hipLaunchKernelGGL(stream_read_k, dim3(blocks), dim3(256), 0, st, src, n4, ctx().dev_scalar);
            THIP_TRY(hipEventRecord(e1, st));
            THIP_TRY(hipEventSynchronize(e1));
            float ms = 0.0f;
            THIP_TRY(hipEventElapsedTime(&ms, e0, e1));
            if (r == 0) continue;
            tot += ms;
            if (ms < mn) mn = ms;
        }
        if (mn < best) { best = mn; best_avg = tot / reps; }
    }
    THIP_LAUNCH_CHECK();
    hipEventDestroy(e0); hipEventDestroy(e1);
    if (host_best_ms) *host_best_ms = best;
    if (host_avg_ms) *host_avg_ms = best_avg;
    return 0;
}
