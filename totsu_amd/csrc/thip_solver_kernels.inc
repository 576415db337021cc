// thip_solver_kernels.inc -- part of thip_solver.hip (one translation unit): the status block and the device kernels of the
// iteration -- reductions behind a pass over A, the element-wise updates, the m-tail of the one-pass schedule, the termination test.
namespace {

constexpr int BLK = 256;
constexpr unsigned NPS = 256;    // sharded run: post_k's grid = number of block partials per sharded sum
constexpr int TAIL = 4 * NPS;    // block partials of up to 3 sharded sums riding behind an n-vector through the all-reduce
constexpr unsigned EG = 512;     // max blocks of the elementwise kernels (block partials per quantity)
constexpr unsigned PG = 4096;    // max blocks of post_k (64 elements per block)

// device status block (copied whole to the host when polling)
struct DevStatus {
    int       stop;              // != 0: every kernel returns at entry
    int       state;             // THIP_ST_*
    int       kind;
    int       xbuf;              // sweep schedule: which of the two x_x buffers holds the iterate the device stopped at
    long long iter;              // index of the iteration being / last executed
    float     cri[3];
    float     tau, kappa;
    float     norm_b, norm_c;
    float     t_tau, s_kappa;    // preconditioner entries of tau / kappa
    float     r_tau;             // rx_tau
    float     kappa_in;          // sweep schedule: kappa_{k-1} as sw_vm_k left it for the sweep that forms kappa_k
    float     tau_next, r_tau_next;   // sweep schedule: tau_{k+1} and rx_tau as the termination test of iterate k left them for the
                                 // next step's m-kernel (which commits them): no block of that kernel reads what another writes
    float     tau_r[2]; long long iter_r[2];   // sweep schedule with the termination test folded into the next step's m-kernel: tau
                                 // and the iteration index in two copies by step parity -- every block of that kernel reads one
                                 // copy, its block 0 writes the other (and tau / iter themselves, which no block of it reads)
    int       fault;             // column-sharded sweep: some rank's one-pass kernel gave up (seen by every rank in the same
                                 // all-reduce, thip_solver_run restores the snapshot on all of them together)
};

// ---------------------------------------------------------------------------------------------------
// kernels.  One iteration of the carried schedule is 7 launches (8 with block cones):
//   gemv, post, [all-reduce], xupdate, soc | gemv, post, [all-reduce], ycrit, status
// The stage's dots are left as block partials by post_k and summed by their consumers (block 0 / the status block).
// In a row-sharded run the block partials of the SHARDED sums (b.v, ||p||^2, b.x_y, b.rx_y) are written straight into
// the tail of the n-vector that is all-reduced (the sum over ranks of block partials is the block partials of the
// global sum), so the sharded path has the single-GPU launch count.  With overlap on, xupdate / ycrit run as two
// launches: the m-part (local rows: needs no collective) while the all-reduce is in flight on the side stream, the
// n-part after it.  The final 1/tau scaling is not a per-iteration launch: the host applies it once when it sees the
// terminated state.
// ---------------------------------------------------------------------------------------------------

// sum over k = k0, k0 + 4, k0 + 8, .. < np of p[k * stride] in f64 with eight independent loads in flight per lane:
// the second reduction stage is a latency chain over ~100-200 partials per element, not a bandwidth problem
__device__ __forceinline__ double sum_partials4(const float *__restrict__ p, size_t stride, int k0, int np)
{
    double s[8] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    int k = k0;
    for (; k + 28 < np; k += 32) {
        float a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = p[(size_t)(k + 4 * u) * stride];
#pragma unroll
        for (int u = 0; u < 8; ++u) s[u] += (double)a[u];
    }
    for (; k < np; k += 4) s[0] += (double)p[(size_t)k * stride];
    return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

// After a dual GEMV: second reduction stage of both products + the stage's sharded / replicated reductions.
//   g[i] = sum_k partT[k][i] (n) ; h[i] = sum_k partN[k][i] (m)
//   q0 = dn_a . dn_b over n (optional) ; q1 = dm_a . dm_b over m (optional)
//   crit != 0: q2 = ||p||^2, q3 = b . x_y with
//      tau > eps_zero: p = x_s/tau - b + h/tau (solver.rs:592-594) ; else p = x_s + h (solver.rs:631-632)
// block partials: q0 (a sum over the replicated n-vectors) -> part_rep[blockIdx.x];
//   q1..q3 (sums over the local rows) -> part_sh[q * gridDim.x + blockIdx.x] (part_sh = the all-reduce tail when sharded)
__global__ __launch_bounds__(BLK) void post_k(int n, int m,
                                             const float *__restrict__ partT, int nT, size_t strideT, float *__restrict__ g,
                                             const float *__restrict__ partN, int nN, size_t strideN, float *__restrict__ h,
                                             const float *__restrict__ dn_a, const float *__restrict__ dn_b,
                                             const float *__restrict__ dm_a, const float *__restrict__ dm_b,
                                             int crit, const float *__restrict__ xs, const float *__restrict__ xy,
                                             const float *__restrict__ b, float eps_zero,
                                             float *__restrict__ part_rep, float *__restrict__ part_sh,
                                             const DevStatus *st, int do_m)
{
    if (st->stop != 0) return;
    // do_m == 0 (column-split runs, first half): the n-part only -- g over the given column range and its q0 partial;
    // the m-part and q1 .. q3 belong to the launch that follows the last column range
    // 256 threads = 64 elements x 4 partial-index lanes: the sum over the ~100 partials of one element is split
    // four ways (4x the loads in flight), combined through LDS, and lane 0 of each element does the epilogue
    __shared__ float sh[16];
    __shared__ double comb[3][64];       // the second reduction stage accumulates in f64 (free here; see DESIGN.md 5, f32 floor)
    const int e = threadIdx.x & 63, kq = threadIdx.x >> 6;
    const size_t gstride = (size_t)gridDim.x * 64;
    float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, q3 = 0.0f;
    const float tau = st->tau;

    for (size_t i0 = blockIdx.x * (size_t)64; i0 < (size_t)n; i0 += gstride) {
        const size_t i = i0 + e;
        double sd = 0.0;
        if (i < (size_t)n) sd = sum_partials4(partT + i, strideT, kq, nT);
        if (kq > 0) comb[kq - 1][e] = sd;
        __syncthreads();
        if (kq == 0 && i < (size_t)n) {
            float s;
            if (nT >= 0) { s = (float)((sd + comb[0][e]) + (comb[1][e] + comb[2][e])); g[i] = s; }
            else s = g[i];                    // nT < 0: g already holds the finished product (sparse path)
            if (dn_a) q0 = fmaf(dn_a[i], dn_b[i], q0);
        }
        __syncthreads();
    }
    if (do_m)
    for (size_t i0 = blockIdx.x * (size_t)64; i0 < (size_t)m; i0 += gstride) {
        const size_t i = i0 + e;
        double sd = 0.0;
        if (i < (size_t)m) sd = sum_partials4(partN + i, strideN, kq, nN);
        if (kq > 0) comb[kq - 1][e] = sd;
        __syncthreads();
        if (kq == 0 && i < (size_t)m) {
            float s;
            if (nN >= 0) { s = (float)((sd + comb[0][e]) + (comb[1][e] + comb[2][e])); h[i] = s; }
            else s = h[i];
            if (dm_a) q1 = fmaf(dm_a[i], dm_b[i], q1);
            if (crit) {
                const float bi = b[i];
                const float p = crit_p(tau, eps_zero, xs[i], bi, s);
                q2 = fmaf(p, p, q2);
                q3 = fmaf(bi, xy[i], q3);
            }
        }
        __syncthreads();
    }
    q0 = block_sum(q0, sh);
    if (threadIdx.x == 0) part_rep[blockIdx.x] = q0;
    if (!do_m) return;
    q1 = block_sum(q1, sh);
    if (threadIdx.x == 0) part_sh[gridDim.x + blockIdx.x] = q1;
    if (crit) {
        q2 = block_sum(q2, sh); q3 = block_sum(q3, sh);
        if (threadIdx.x == 0) { part_sh[2 * gridDim.x + blockIdx.x] = q2; part_sh[3 * gridDim.x + blockIdx.x] = q3; }
    }
}

// sum of np block partials by one whole block (f64 accumulation); the result is valid in every thread.
// shd: 16 doubles of LDS.
__device__ __forceinline__ float block_sum_of_partials(const float *part, int np, double *shd)
{
    double acc = 0.0;
    for (int k = threadIdx.x; k < np; k += BLK) acc += (double)part[k];
    acc = block_sum_d(acc, shd);
    __syncthreads();
    return (float)acc;
}

// x + inc, compensated (kahan_add, thip_step.h) where the iterate has Kahan terms: k != NULL
__device__ __forceinline__ float comp_add(float x, float inc, float *k, size_t i) { return kahan_add_at(x, inc, k != nullptr, k, i); }

// x-update, solver.rs:538-555 (everything except the block cones):
//   x += T o tx with tx = -K^T y (SelfDualEmbed::trans_op, solver.rs:133-157):
//     x_x += Tx o ( gT + c kappa)        gT = A^T v   (after the all-reduce)
//     x_y += Ty o (-hN + b kappa)        hN = A u
//     x_s += Ts o ( v )
//     tau += Ttau (-c.u - b.v) ; tau <- max(tau, 0)                       (solver.rs:551-552)
//   element-wise cones folded in: cls 0 = zero cone (dual: identity, primal: 0; cone_zero.rs:38-44),
//   cls 1 = nonneg (max(.,0) both; cone_rpos.rs:38-45), cls >= 2 = member of a block cone (projected by the
//   next launch, which also finishes rx for those rows);
//   rx = x_k - 2 x_{k+1} (solver.rs:538,555) for x_x, tau and the cls 0/1 rows; rx = x_k for block-cone rows.
__global__ __launch_bounds__(BLK) void xupdate_k(int n, int m, const float *__restrict__ gT, const float *__restrict__ hN,
                                                const float *__restrict__ c, const float *__restrict__ b,
                                                const float *__restrict__ v, const float *__restrict__ Tx,
                                                const float *__restrict__ Ty, const float *__restrict__ Ts,
                                                const unsigned char *__restrict__ cls,
                                                float *__restrict__ xx, float *__restrict__ xy, float *__restrict__ xs,
                                                float *__restrict__ rxx, float *__restrict__ rxy, float *__restrict__ rxs,
                                                DevStatus *st, const float *ps_c, int np_c, const float *ps_b, int np_b,
                                                int do_n, int do_m, int do_tau,
                                                float *__restrict__ kx, float *__restrict__ ky, float *__restrict__ ks)
{
    if (st->stop != 0) return;
    // do_tau: the tau update (with do_n in one launch; column-split runs give the x_x rows as two ranges -- n and the
    // n-pointers then describe a range -- and update tau with the second)
    // kx / ky / ks != NULL: compensated (Kahan) accumulation of the iterate -- see comp_add
    // do_n: the x_x rows and tau (need the all-reduced gT and b.v); do_m: the x_y / x_s rows (local).  Both in one
    // launch, or the m-part first while the all-reduce is in flight.
    // block 0 sums post_k's block partials of c.u (ps_c) and b.v (ps_b: all-reduced block partials when sharded)
    float dc = 0.0f, db = 0.0f;
    if (do_tau && blockIdx.x == 0) {
        __shared__ double shd[16];
        dc = block_sum_of_partials(ps_c, np_c, shd);
        db = block_sum_of_partials(ps_b, np_b, shd);
    }
    const float kappa = st->kappa;
    const size_t gstride = (size_t)gridDim.x * BLK;
    if (do_n)
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)n; i += gstride) {
        const float old = xx[i];
        const float nw = comp_add(old, inc_xx(Tx[i], gT[i], c[i], kappa), kx, i);
        xx[i] = nw;
        rxx[i] = rx_fold(old, nw);
    }
    if (do_m)
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)m; i += gstride) {
        const unsigned char k = cls[i];
        const float oy = xy[i], os = xs[i];
        float ny = comp_add(oy, inc_xy(Ty[i], b[i], kappa, hN[i]), ky, i);
        float ns = comp_add(os, inc_xs(Ts[i], v[i]), ks, i);
        cone_elementwise(k, ny, ns);
        xy[i] = ny;
        xs[i] = ns;
        rxy[i] = cone_rx(k, oy, ny);
        rxs[i] = cone_rx(k, os, ns);
    }
    if (do_tau && blockIdx.x == 0 && threadIdx.x == 0) {
        // every other thread only reads st->kappa / st->stop; tau is written by this thread alone
        const float old = st->tau;
        float t = old + st->t_tau * (-dc - db);
        t = fmaxf(t, 0.0f);
        st->tau = t;
        st->r_tau = old - 2.0f * t;
    }
}

// rx <- rx - 2 x on the rows of PSD blocks (cls 3), after their projection
__global__ void rx_psd_k(int m, const unsigned char *__restrict__ cls, const float *__restrict__ xy,
                         const float *__restrict__ xs, float *__restrict__ rxy, float *__restrict__ rxs,
                         const DevStatus *st)
{
    if (st->stop != 0) return;
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)m; i += (size_t)gridDim.x * BLK)
        if (cls[i] == 3) { rxy[i] = rxy[i] - 2.0f * xy[i]; rxs[i] = rxs[i] - 2.0f * xs[i]; }
}

// y-update, solver.rs:557-567 with ty = -K rx (SelfDualEmbed::op solver.rs:109-131):
//   u += Su o (-g2 - c rtau)          g2 = A^T rx_y
//   v += Sv o ( h2 + rx_s - b rtau)   h2 = A rx_x
//   kappa += Skappa (c.rx_x + b.rx_y) ; kappa <- min(kappa, 0)
// carried != 0: g2 = gP - 2 g3, h2 = hP - 2 h3 from the criteria products of x_k (gP, hP) and x_{k+1} (g3, h3),
//   which then become the previous ones;  carried == 0: g2 / h2 are given.
// docrit != 0: also the n-part of the criteria: block partials of ||d||^2 and c.x_x,
//   d = c + (A^T x_y)/tau (solver.rs:596-597) or A^T x_y (solver.rs:634)
__global__ __launch_bounds__(BLK) void ycrit_k(int n, int m, int doy, int carried, int docrit,
                                              const float *__restrict__ g3, const float *__restrict__ h3,
                                              float *__restrict__ gP, float *__restrict__ hP,
                                              const float *__restrict__ g2in, const float *__restrict__ h2in,
                                              const float *__restrict__ c, const float *__restrict__ b,
                                              const float *__restrict__ rxs, const float *__restrict__ Su,
                                              const float *__restrict__ Sv, float *__restrict__ u, float *__restrict__ v,
                                              const float *__restrict__ xx, float eps_zero, float *__restrict__ part,
                                              DevStatus *st, const float *ps_c, int np_c, const float *ps_b, int np_b,
                                              int do_n, int do_m, int do_kappa, int pbase, int pstride,
                                              float *__restrict__ ku, float *__restrict__ kv)
{
    if (st->stop != 0) return;
    // do_kappa: the kappa update (with do_n in one launch; column-split runs give the u rows as two ranges and update
    // kappa with the second).  The criteria partials of this launch go to part[pbase + block] (||d||^2) and
    // part[pstride + pbase + block] (c.x_x): one launch pbase = 0, pstride = gridDim.x
    // do_n: the u rows, kappa and the n-part of the criteria (need the all-reduced products); do_m: the v rows (local)
    __shared__ float sh[16];
    float dc = 0.0f, db = 0.0f;      // c.rx_x and b.rx_y: block partials of post_k summed here by block 0
    if (doy && do_kappa && blockIdx.x == 0) {
        __shared__ double shd[16];
        dc = block_sum_of_partials(ps_c, np_c, shd);
        db = block_sum_of_partials(ps_b, np_b, shd);
    }
    const float rtau = st->r_tau;
    const float tau = st->tau;
    const size_t gstride = (size_t)gridDim.x * BLK;
    float dd = 0.0f, cx = 0.0f;
    if (do_n)
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)n; i += gstride) {
        const float ci = c[i];
        if (doy) {
            float g2;
            if (carried) { const float nw = g3[i]; g2 = rx_fold(gP[i], nw); gP[i] = nw; }
            else g2 = g2in[i];
            u[i] = comp_add(u[i], inc_u(Su[i], g2, ci, rtau), ku, i);
        }
        if (docrit) {
            const float d = crit_d(tau, eps_zero, ci, g3[i]);
            dd = fmaf(d, d, dd);
            cx = fmaf(ci, xx[i], cx);
        }
    }
    if (doy) {
        if (do_m)
        for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)m; i += gstride) {
            float h2;
            if (carried) { const float nw = h3[i]; h2 = rx_fold(hP[i], nw); hP[i] = nw; }
            else h2 = h2in[i];
            v[i] = comp_add(v[i], inc_v(Sv[i], h2, rxs[i], b[i], rtau), kv, i);
        }
        if (do_kappa && blockIdx.x == 0 && threadIdx.x == 0) {
            const float k = st->kappa + st->s_kappa * (dc + db);
            st->kappa = fminf(k, 0.0f);       // solver.rs:566-567
        }
    }
    if (docrit && do_n) {
        dd = block_sum(dd, sh);
        cx = block_sum(cx, sh);
        if (threadIdx.x == 0) { part[pbase + blockIdx.x] = dd; part[pstride + pbase + blockIdx.x] = cx; }
    }
}

// the termination test, solver.rs:381-451 + the tails of criteria_conv / criteria_inf (solver.rs:599-611,
// 636-655).  status_eval is run by a whole block of at least 256 threads: six sums of block partials (f64 accumulation), each by ONE
// wave, two per wave, all loads in flight together and one barrier; every thread then holds the verdict.  status_k -- one
// block -- commits it; the merged m-kernels of the one-pass schedule evaluate it at their head in EVERY block (same inputs,
// same arithmetic, same verdict) so that the test of iterate k needs no launch of its own between sweep k and step k + 1.
struct StatArgs {
    int np; const float *part;                       // sums over n: ||d||^2 = part[0 .. np), c.x_x = part[np .. 2 np)
    const float *ps_pp, *ps_by; int npsum;           // sums over m: ||p||^2, b.x_y (post_k's / the m-kernel's block partials)
    const float *ps_cu; int np_cu; const float *ps_bv; int np_bv;      // sweep schedule: c.u, b.v -> the next tau; else NULL
    const float *fault_flag;                         // column-sharded sweep: the all-reduced "a kernel gave up" flag, else NULL
    float eps_acc, eps_inf, eps_zero; long long max_iter; int xbuf;
};
struct StatOut { int state, kind; float cri[3]; float tau_next, r_tau_next; };      // state: THIP_ST_*, or -2: a peer's fault

__device__ __forceinline__ StatOut status_eval(const StatArgs &a, float tau, long long i, float norm_b, float norm_c, float t_tau,
                                               double *sums /* 8 doubles of LDS */)
{
    StatOut o;
    o.state = THIP_ST_RUNNING; o.kind = 0; o.cri[0] = o.cri[1] = o.cri[2] = 0.0f; o.tau_next = tau; o.r_tau_next = 0.0f;
    if (a.fault_flag != nullptr && *a.fault_flag > 0.0f) { o.state = -2; return o; }      // (uniform: every thread reads the same word)
    {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        const float *src[2] = { nullptr, nullptr };
        int cnt[2] = { 0, 0 };
        if (w < 4) {            // (the first four waves of the block; a wider block's other waves only wait at the barrier)
        switch (w) {
        case 0: src[0] = a.ps_pp; cnt[0] = a.npsum; src[1] = a.ps_cu; cnt[1] = a.ps_cu ? a.np_cu : 0; break;
        case 1: src[0] = a.ps_by; cnt[0] = a.npsum; src[1] = a.ps_bv; cnt[1] = a.ps_bv ? a.np_bv : 0; break;
        case 2: src[0] = a.part; cnt[0] = a.np; break;
        default: src[0] = a.part + a.np; cnt[0] = a.np; break;
        }
        double acc[2] = { 0.0, 0.0 };
#pragma unroll
        for (int q = 0; q < 2; ++q)
            for (int k = lane; k < cnt[q]; k += 64) acc[q] += (double)src[q][k];
        acc[0] = wave_sum_d(acc[0]);
        acc[1] = wave_sum_d(acc[1]);
        if (lane == 0) { sums[w] = acc[0]; sums[4 + w] = acc[1]; }
        }
    }
    __syncthreads();
    const float pp = (float)sums[0], by = (float)sums[1];
    const float dd = (float)sums[2], cx = (float)sums[3];
    const float dcu = (float)sums[4], dbv = (float)sums[5];
    const StepVerdict sv = step_verdict(tau, i, norm_b, norm_c, a.eps_acc, a.eps_inf, a.eps_zero, a.max_iter, pp, by, dd, cx,
                                        THIP_ST_RUNNING);
    const int state = sv.state;
    o.kind = sv.kind; o.cri[0] = sv.cri0; o.cri[1] = sv.cri1; o.cri[2] = sv.cri2;
    o.state = state;
    if (state == THIP_ST_RUNNING && a.ps_cu != nullptr) {
        // sweep schedule: c.u_k and b.v_k are complete here too -- the tau update of the NEXT step (solver.rs:551-552)
        const float t = fmaxf(tau + t_tau * (-dcu - dbv), 0.0f);
        o.tau_next = t;
        o.r_tau_next = tau - 2.0f * t;
    }
    return o;
}

// what ONE thread writes for a verdict that ends the loop (or for a peer's fault); a RUNNING verdict is committed by its
// caller (status_k here; the m-kernels at their end)
__device__ __forceinline__ void status_commit_stop(DevStatus *st, const StatOut &o, int xbuf)
{
    if (o.state == -2) { st->fault = 1; st->stop = 1; return; }
    st->kind = o.kind; st->cri[0] = o.cri[0]; st->cri[1] = o.cri[1]; st->cri[2] = o.cri[2];
    st->state = o.state; st->xbuf = xbuf; st->stop = 1;      // later launches are no-ops
}

__global__ __launch_bounds__(BLK) void status_k(const StatArgs a, DevStatus *st)
{
    if (st->stop != 0) return;
    __shared__ double sums[8];
    const long long i = st->iter;
    const StatOut o = status_eval(a, st->tau, i, st->norm_b, st->norm_c, st->t_tau, sums);
    if (threadIdx.x != 0) return;
    if (o.state != THIP_ST_RUNNING) { status_commit_stop(st, o, a.xbuf); return; }
    st->kind = o.kind; st->cri[0] = o.cri[0]; st->cri[1] = o.cri[1]; st->cri[2] = o.cri[2];
    st->iter = i + 1;
    if (a.ps_cu != nullptr) { st->tau_next = o.tau_next; st->r_tau_next = o.r_tau_next; }
}

// ---------------------------------------------------------------------------------------------------
// THIP_SCHED_SWEEP: the O(n + m) work between two sweeps over A (thip_sweep.hip).  Step k (k >= 1) is
//   sw_xm_k   tau_k ; x_y_k, x_s_k from hN = A u_{k-1} (the groups' shares summed here), element-wise cones, rx
//   [block cones]
//   sw_vm_k   v_k from h2 = hP - 2 h3 (h3 = A x_x_k, carried form) ; partial sums of b.v_k, b.rx_y, ||p_k||^2, b.x_y_k
//   SWEEP     kappa_k (every workgroup for itself, at entry) ; u_k, x_x_{k+1}, gP = A^T x_y_k, the shares of A u_k and A x_x_{k+1}, and -- per workgroup, over the columns it
//             writes -- the partial sums over n: ||d_k||^2, c.x_x_k, c.u_k, c.rx_x_k
//   status_k  the termination test of iterate k (solver.rs:381-451)
// The arithmetic of every update is thip_step.h's.
// ---------------------------------------------------------------------------------------------------
// row i's shares of hN = A u (sa) and of A x_x (sb): the quarter kq of the groups, 32 / 8 / 1 at a time.  Sixteen loads in flight,
// added in the order of the plain loop: the shares were written by workgroups on other XCDs, so every one of them is a trip to
// the Infinity Cache.  !ok: both zero, nothing read
__device__ __forceinline__ void sum_shares(const float *partH, size_t mpad, int ngroups, int kq, size_t i, bool ok,
                                           float &sa, float &sb)
{
    float sa0 = 0.0f, sa1 = 0.0f, sb0 = 0.0f, sb1 = 0.0f;
    if (ok) {
        int g = kq;
        for (; g + 28 < ngroups; g += 32) {
            float t[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float *q = partH + (size_t)(g + 8 * j) * 2 * mpad + i;
                t[4 * j] = q[0]; t[4 * j + 1] = q[mpad]; t[4 * j + 2] = q[8 * mpad]; t[4 * j + 3] = q[9 * mpad];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) { sa0 += t[4 * j]; sb0 += t[4 * j + 1]; sa1 += t[4 * j + 2]; sb1 += t[4 * j + 3]; }
        }
        for (; g + 4 < ngroups; g += 8) {
            const float *q = partH + (size_t)g * 2 * mpad + i;
            sa0 += q[0]; sb0 += q[mpad]; sa1 += q[8 * mpad]; sb1 += q[9 * mpad];
        }
        if (g < ngroups) { sa0 += partH[((size_t)g * 2 + 0) * mpad + i]; sb0 += partH[((size_t)g * 2 + 1) * mpad + i]; }
    }
    sa = sa0 + sa1; sb = sb0 + sb1;
}

// MERGE (no block cones: every row's projection is element-wise): the same launch also does sw_vm_k's part of the row -- v_k,
// the sums over m -- with tau_k / rx_tau as the previous termination test left them (DevStatus::tau_next), and leaves its
// four block partials in `part` (gridDim.x each)
// FLAT (at most four shares per row -- a sparse operator's slices): one thread per row, no combine through LDS, no barrier.  The
// 64 x 4 shape walks m in steps of 64 rows per block with two barriers each: at m = 9 M (a stencil) that is 275 dependent steps,
// 879 us for what is 0.6 GB of traffic.  The sum over the shares keeps the association of the 4-lane form: (g0 + g1) + (g2 + g3).
// (FLAT runs with 256 or, for m beyond EG x 1024 rows, 1024 threads per block: the grid is capped at EG blocks -- the block partials' slots)
template <bool MERGE, bool FLAT = false>
__global__ __launch_bounds__(FLAT ? 1024 : BLK) void sw_xm_k(int m, int ngroups, size_t mpad, const float *__restrict__ partH,
                                              float *__restrict__ h3, const float *__restrict__ b,
                                              float *__restrict__ v, const float *__restrict__ Ty,
                                              const float *__restrict__ Ts, const unsigned char *__restrict__ cls,
                                              float *__restrict__ xy, float *__restrict__ xs, float *__restrict__ rxy,
                                              float *__restrict__ rxs, DevStatus *st, float *__restrict__ ky, float *__restrict__ ks,
                                              float *__restrict__ hP, const float *__restrict__ Sv, float *__restrict__ kv,
                                              float eps_zero, float *__restrict__ part, const StatArgs sa, int fold, int par)
{
    if (st->stop != 0) return;
    // fold != 0: the termination test of the PREVIOUS iterate has had no launch of its own -- every block evaluates it here,
    // from the same sums, before anything is written; a verdict that ends the loop leaves the iterate alone (the launches
    // behind this one -- block cones, sw_vm_k, the sweep -- return at entry on the stop flag block 0 raises)
    float tau, rtau;
    StatOut so;
    long long it0 = 0;
    if (fold) {
        __shared__ double ssum[8];
        it0 = st->iter_r[par];
        so = status_eval(sa, st->tau_r[par], it0, st->norm_b, st->norm_c, st->t_tau, ssum);
        if (so.state != THIP_ST_RUNNING) {
            if (blockIdx.x == 0 && threadIdx.x == 0) status_commit_stop(st, so, sa.xbuf);
            return;
        }
        tau = so.tau_next; rtau = so.r_tau_next;
    } else {
        tau = st->tau_next; rtau = st->r_tau_next;      // tau_k, rx_tau as status_k / sw_tau_k left them (read-only here)
    }
    const float kappa = st->kappa;
    float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, q3 = 0.0f;
    // 256 threads = 64 rows x 4 group lanes (post_k's shape): the sum over the groups' shares of one row -- up to 256 of
    // them, 128 at the 10 000-variable LP -- is split four ways, combined through LDS, and lane 0 of a row does the update
    auto row = [&](const size_t i, const float hN, const float hx) {
            const unsigned char k = cls[i];
            const float oy = xy[i], os = xs[i], bi = b[i], vi = v[i];
            float ny = comp_add(oy, inc_xy(Ty[i], bi, kappa, hN), ky, i);
            float ns = comp_add(os, inc_xs(Ts[i], vi), ks, i);
            cone_elementwise(k, ny, ns);
            xy[i] = ny;
            xs[i] = ns;
            const float ry = cone_rx(k, oy, ny), rs = cone_rx(k, os, ns);
            rxy[i] = ry;
            rxs[i] = rs;
            if constexpr (MERGE) {
                // sw_vm_k's row: v_k from h2 = hP - 2 h3 (h3 = A x_x_k) ; the criteria sums over m
                const float h2 = rx_fold(hP[i], hx);
                hP[i] = hx;
                const float vn = comp_add(vi, inc_v(Sv[i], h2, rs, bi, rtau), kv, i);
                v[i] = vn;
                q0 = fmaf(bi, vn, q0);
                q1 = fmaf(bi, ry, q1);
                const float p = crit_p(tau, eps_zero, ns, bi, hx);
                q2 = fmaf(p, p, q2);
                q3 = fmaf(bi, ny, q3);
            } else {
                h3[i] = hx;
            }
    };
    if constexpr (FLAT) {
        const size_t gstride = (size_t)gridDim.x * blockDim.x;
        for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)m; i += gstride) {
            float sa[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, sb[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (g < ngroups) { sa[g] = partH[((size_t)g * 2 + 0) * mpad + i]; sb[g] = partH[((size_t)g * 2 + 1) * mpad + i]; }
            row(i, (sa[0] + sa[1]) + (sa[2] + sa[3]), (sb[0] + sb[1]) + (sb[2] + sb[3]));
        }
    } else {
    __shared__ float comb[2][3][64];
    const int e = threadIdx.x & 63, kq = threadIdx.x >> 6;
    const size_t gstride = (size_t)gridDim.x * 64;
    for (size_t i0 = blockIdx.x * (size_t)64; i0 < (size_t)m; i0 += gstride) {
        const size_t i = i0 + e;
        float sa, sb;
        sum_shares(partH, mpad, ngroups, kq, i, i < (size_t)m, sa, sb);
        if (kq > 0) { comb[0][kq - 1][e] = sa; comb[1][kq - 1][e] = sb; }
        __syncthreads();
        if (kq == 0 && i < (size_t)m) {
            const float hN = (sa + comb[0][0][e]) + (comb[0][1][e] + comb[0][2][e]);
            const float hx = (sb + comb[1][0][e]) + (comb[1][1][e] + comb[1][2][e]);
            row(i, hN, hx);
        }
        __syncthreads();
    }
    }
    if constexpr (MERGE) {
        __shared__ float sh[16];
        q0 = block_sum(q0, sh); q1 = block_sum(q1, sh); q2 = block_sum(q2, sh); q3 = block_sum(q3, sh);
        if (threadIdx.x == 0) {
            part[blockIdx.x] = q0; part[gridDim.x + blockIdx.x] = q1;
            part[2 * gridDim.x + blockIdx.x] = q2; part[3 * gridDim.x + blockIdx.x] = q3;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->tau = tau;
        st->r_tau = rtau;
        if (MERGE) st->kappa_in = kappa;          // nobody writes kappa between here and the sweep
        st->tau_r[par ^ 1] = tau;
        if (fold) {
            st->kind = so.kind; st->cri[0] = so.cri[0]; st->cri[1] = so.cri[1]; st->cri[2] = so.cri[2];
            st->iter = it0 + 1; st->iter_r[par ^ 1] = it0 + 1;
        } else {
            st->iter_r[par ^ 1] = st->iter;
        }
    }
}

// Every row in a second-order cone of at most 129 rows (BASELINE configs[2]: 1000 cones of 100): the WHOLE m-tail of a step
// as one launch, one workgroup per cone (looping when there are more than EG cones) -- sw_xm_k's row: the groups' shares
// summed by four lanes per row exactly as there, x_y / x_s; then on the workgroup's first wave the projection of both
// blocks (cone_soc.rs:38-65; soc_k's lane <-> row mapping and f64 sum of squares, soc_scale in f32) and sw_vm_k's row (v, the sums over m).
// Lane l of that wave holds rows beg + 1 + l and beg + 65 + l, lane 0 also the cone's first row.  Every per-row value has
// the arithmetic of the three-launch form; only the block partials of the four sums over m are grouped differently.
__global__ __launch_bounds__(BLK) void sw_cone_k(int n_cones, const int64_t *__restrict__ begs, const int64_t *__restrict__ ends,
                                                int ngroups, size_t mpad, const float *__restrict__ partH,
                                                const float *__restrict__ b, float *__restrict__ v, const float *__restrict__ Ty,
                                                const float *__restrict__ Ts, float *__restrict__ xy, float *__restrict__ xs,
                                                float *__restrict__ rxy, float *__restrict__ rxs, DevStatus *st,
                                                float *__restrict__ ky, float *__restrict__ ks, float *__restrict__ hP,
                                                const float *__restrict__ Sv, float *__restrict__ kv, float eps_zero,
                                                float *__restrict__ part, const StatArgs sa, int fold, int par)
{
    if (st->stop != 0) return;
    const int e = threadIdx.x & 63, kq = threadIdx.x >> 6;
    float tau, rtau;                               // (the folded termination test: see sw_xm_k)
    StatOut so;
    long long it0 = 0;
    if (fold) {
        __shared__ double ssum[8];
        it0 = st->iter_r[par];
        so = status_eval(sa, st->tau_r[par], it0, st->norm_b, st->norm_c, st->t_tau, ssum);
        if (so.state != THIP_ST_RUNNING) {
            if (blockIdx.x == 0 && threadIdx.x == 0) status_commit_stop(st, so, sa.xbuf);
            return;
        }
        tau = so.tau_next; rtau = so.r_tau_next;
    } else {
        tau = st->tau_next; rtau = st->r_tau_next;
    }
    const float kappa = st->kappa;
    __shared__ float comb[3][2][3][64];           // [row slot][product][lane quarter - 1][row lane]
    float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, q3 = 0.0f;
    for (int cone = blockIdx.x; cone < n_cones; cone += gridDim.x) {
        const int64_t beg = begs[cone], end = ends[cone];
        if (end <= beg) continue;                  // (uniform over the workgroup)
        // slot 0 / 1: rows beg + 1 + e (+ 64); slot 2: the first row (lane 0)
        const size_t idx[3] = { (size_t)(beg + 1 + e), (size_t)(beg + 65 + e), (size_t)beg };
        const bool ok[3] = { beg + 1 + e < end, beg + 65 + e < end, e == 0 };
        // the first wave's row data: requested before the shares, used after the barrier (one round trip for everything)
        // (the Kahan terms, hP and Sv too: the cone phase below is then arithmetic and stores only -- with them fetched where
        // they are used it was three dependent round trips per cone, 20 us per launch at configs[2])
        float oy[3], os[3], bi[3], vi[3], tyv[3], tsv[3], kyv[3], ksv[3], kvv[3], hPv[3], svv[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            oy[k] = os[k] = bi[k] = vi[k] = tyv[k] = tsv[k] = kyv[k] = ksv[k] = kvv[k] = hPv[k] = svv[k] = 0.0f;
            if (kq == 0 && ok[k]) {
                const size_t i = idx[k];
                oy[k] = xy[i]; os[k] = xs[i]; bi[k] = b[i]; vi[k] = v[i]; tyv[k] = Ty[i]; tsv[k] = Ts[i];
                hPv[k] = hP[i]; svv[k] = Sv[i];
                if (ky) kyv[k] = ky[i];
                if (ks) ksv[k] = ks[i];
                if (kv) kvv[k] = kv[i];
            }
        }
        float sas[3], sbs[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            // the shares of row idx[k]: this thread's quarter of the groups, in sw_xm_k's order
            sum_shares(partH, mpad, ngroups, kq, idx[k], ok[k], sas[k], sbs[k]);
            if (kq > 0) { comb[k][0][kq - 1][e] = sas[k]; comb[k][1][kq - 1][e] = sbs[k]; }
        }
        __syncthreads();
        float hNs[3] = { 0.0f, 0.0f, 0.0f }, hxs[3] = { 0.0f, 0.0f, 0.0f };
        if (kq == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                hNs[k] = (sas[k] + comb[k][0][0][e]) + (comb[k][0][1][e] + comb[k][0][2][e]);
                hxs[k] = (sbs[k] + comb[k][1][0][e]) + (comb[k][1][1][e] + comb[k][1][2][e]);
            }
        }
        __syncthreads();                           // (the next cone's shares may overwrite comb)
        if (kq != 0) continue;                     // the cone itself is the first wave's (no barrier below)
        float ny[3], ns[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ny[k] = ns[k] = 0.0f;
            if (!ok[k]) continue;
            const size_t i = idx[k];
            ny[k] = kahan_add_to(oy[k], inc_xy(tyv[k], bi[k], kappa, hNs[k]), ky != nullptr, kyv[k], ky, i);
            ns[k] = kahan_add_to(os[k], inc_xs(tsv[k], vi[k]), ks != nullptr, ksv[k], ks, i);
        }
        // the projection of the x_y block and of the x_s block (not rotated; the factor in f32)
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            float *x = which ? ns : ny;
            const float s0 = __shfl(x[2], 0, 64);
            double acc = 0.0;
            if (ok[0]) acc += (double)x[0] * (double)x[0];
            if (ok[1]) acc += (double)x[1] * (double)x[1];
            const float norm_v = (float)sqrt(wave_sum_d(acc));
            float f, s_new;
            soc_scale<float>(s0, norm_v, f, s_new);
            x[2] = s_new;
            if (f != 1.0f) { x[0] = soc_scaled<float>(f, x[0]); x[1] = soc_scaled<float>(f, x[1]); }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (!ok[k]) continue;
            const size_t i = idx[k];
            xy[i] = ny[k];
            xs[i] = ns[k];
            const float ry = rx_fold(oy[k], ny[k]), rs = rx_fold(os[k], ns[k]);
            rxy[i] = ry;
            rxs[i] = rs;
            const float hx = hxs[k];
            const float h2 = rx_fold(hPv[k], hx);
            hP[i] = hx;
            const float vn = kahan_add_to(vi[k], inc_v(svv[k], h2, rs, bi[k], rtau), kv != nullptr, kvv[k], kv, i);
            v[i] = vn;
            q0 = fmaf(bi[k], vn, q0);
            q1 = fmaf(bi[k], ry, q1);
            const float p = crit_p(tau, eps_zero, ns[k], bi[k], hx);
            q2 = fmaf(p, p, q2);
            q3 = fmaf(bi[k], ny[k], q3);
        }
    }
    if (kq == 0) {
        q0 = wave_sum(q0); q1 = wave_sum(q1); q2 = wave_sum(q2); q3 = wave_sum(q3);
        if (e == 0) {
            part[blockIdx.x] = q0; part[gridDim.x + blockIdx.x] = q1;
            part[2 * gridDim.x + blockIdx.x] = q2; part[3 * gridDim.x + blockIdx.x] = q3;
            if (blockIdx.x == 0) {
                st->tau = tau;
                st->r_tau = rtau;
                st->kappa_in = kappa;
                st->tau_r[par ^ 1] = tau;
                if (fold) {
                    st->kind = so.kind; st->cri[0] = so.cri[0]; st->cri[1] = so.cri[1]; st->cri[2] = so.cri[2];
                    st->iter = it0 + 1; st->iter_r[par ^ 1] = it0 + 1;
                } else {
                    st->iter_r[par ^ 1] = st->iter;
                }
            }
        }
    }
}

// (re)start of the one-pass schedule: the tau update a regular step takes from the previous termination test
__global__ __launch_bounds__(BLK) void sw_tau_k(DevStatus *st, const float *ps_cu, int np_cu, const float *ps_bv, int np_bv)
{
    if (st->stop != 0) return;
    // (summed as status_k sums them: one wave per quantity)
    __shared__ double sums[2];
    {
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        if (w < 2) {
            const float *src = w == 0 ? ps_cu : ps_bv;
            const int cnt = w == 0 ? np_cu : np_bv;
            double acc = 0.0;
            for (int k = lane; k < cnt; k += 64) acc += (double)src[k];
            acc = wave_sum_d(acc);
            if (lane == 0) sums[w] = acc;
        }
    }
    __syncthreads();
    const float dc = (float)sums[0], db = (float)sums[1];
    if (threadIdx.x == 0) {
        const float old = st->tau;
        const float t = fmaxf(old + st->t_tau * (-dc - db), 0.0f);
        st->tau_next = t;
        st->r_tau_next = old - 2.0f * t;
    }
}

// part: [0] b.v_k, [1] b.rx_y, [2] ||p_k||^2, [3] b.x_y_k, gridDim.x block partials each
__global__ __launch_bounds__(BLK) void sw_vm_k(int m, const float *__restrict__ h3, float *__restrict__ hP,
                                              const float *__restrict__ b, const float *__restrict__ rxs,
                                              const float *__restrict__ rxy, const float *__restrict__ Sv,
                                              float *__restrict__ v, float *__restrict__ kv, const float *__restrict__ xs,
                                              const float *__restrict__ xy, float eps_zero, DevStatus *st,
                                              float *__restrict__ part)
{
    if (st->stop != 0) return;
    __shared__ float sh[16];
    if (blockIdx.x == 0 && threadIdx.x == 0) st->kappa_in = st->kappa;      // nobody writes kappa between here and the sweep
    const float rtau = st->r_tau, tau = st->tau;
    float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, q3 = 0.0f;
    const size_t gstride = (size_t)gridDim.x * BLK;
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)m; i += gstride) {
        const float nw = h3[i], bi = b[i];
        const float h2 = rx_fold(hP[i], nw);
        hP[i] = nw;
        const float vn = comp_add(v[i], inc_v(Sv[i], h2, rxs[i], bi, rtau), kv, i);
        v[i] = vn;
        q0 = fmaf(bi, vn, q0);
        q1 = fmaf(bi, rxy[i], q1);
        const float p = crit_p(tau, eps_zero, xs[i], bi, nw);
        q2 = fmaf(p, p, q2);
        q3 = fmaf(bi, xy[i], q3);
    }
    q0 = block_sum(q0, sh); q1 = block_sum(q1, sh); q2 = block_sum(q2, sh); q3 = block_sum(q3, sh);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = q0; part[gridDim.x + blockIdx.x] = q1;
        part[2 * gridDim.x + blockIdx.x] = q2; part[3 * gridDim.x + blockIdx.x] = q3;
    }
}

// (re)start of the one-pass schedule from a consistent iterate: block partials of b.v (a step leaves them for the next
// one's tau update; whatever ran before this -- nothing, or the carried schedule -- did not)
__global__ __launch_bounds__(BLK) void sw_bv_k(int m, const float *__restrict__ b, const float *__restrict__ v,
                                              float *__restrict__ part, const DevStatus *st)
{
    if (st->stop != 0) return;
    __shared__ float sh[16];
    float q = 0.0f;
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)m; i += (size_t)gridDim.x * BLK) q = fmaf(b[i], v[i], q);
    q = block_sum(q, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = q;
}

// column-sharded runs: the groups' shares of the two N products summed into the buffer that is all-reduced
// + this rank's 4 x 256 sums over n (the sweep wrote them to its own buffer) into the 4 x EG slots of the tail, and this
// rank's "my kernel gave up" flag behind them
__global__ __launch_bounds__(BLK) void sw_gsum_k(int m, int ngroups, size_t mpad, const float *__restrict__ partH,
                                                float *__restrict__ out, const DevStatus *st, const float *__restrict__ pn_loc,
                                                const unsigned *__restrict__ errw)
{
    if (st->stop != 0) return;
    if (blockIdx.x == 0) {
        float *tail = out + 2 * mpad;
        for (int q = 0; q < 4; ++q) tail[q * (int)EG + threadIdx.x] = pn_loc[q * 256 + threadIdx.x];      // BLK == 256 workgroups of the sweep
        if (threadIdx.x == 0) tail[4 * EG] = *errw != 0u ? 1.0f : 0.0f;
    }
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)m; i += (size_t)gridDim.x * BLK) {
        float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f, b0 = 0.0f, b1 = 0.0f, b2 = 0.0f, b3 = 0.0f;      // as in sw_xm_k
        int g = 0;
        for (; g + 4 <= ngroups; g += 4) {
            const float *q = partH + (size_t)g * 2 * mpad + i;
            a0 += q[0]; b0 += q[mpad]; a1 += q[2 * mpad]; b1 += q[3 * mpad];
            a2 += q[4 * mpad]; b2 += q[5 * mpad]; a3 += q[6 * mpad]; b3 += q[7 * mpad];
        }
        for (; g < ngroups; ++g) { a0 += partH[((size_t)g * 2 + 0) * mpad + i]; b0 += partH[((size_t)g * 2 + 1) * mpad + i]; }
        out[i] = (a0 + a1) + (a2 + a3); out[mpad + i] = (b0 + b1) + (b2 + b3);
    }
}

// solver.rs:397-400: on Converged / ExcessIter in the tau > eps_zero branch, x_x and x_y are scaled by 1/tau.  Launched
// once, by the host, when it first sees the terminated state (poll()): status_k itself raises the stop flag, so
// nothing else touches the iterate in between and no per-iteration launch is spent on a no-op.
__global__ void finalize_k(int n, int m, float *__restrict__ xx, float *__restrict__ xy, const DevStatus *st)
{
    const bool scale = (st->kind == 0) && (st->state == THIP_ST_OK || st->state == THIP_ST_EXCESS_ITER);
    if (!scale) return;
    const float rt = 1.0f / st->tau;
    const size_t gstride = (size_t)gridDim.x * BLK;
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)n; i += gstride) xx[i] = rt * xx[i];
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)m; i += gstride) xy[i] = rt * xy[i];
}

// thip_solver_resume: undo finalize_k (x_x, x_y back to the homogeneous iterate) and clear the termination
__global__ void resume_k(int n, int m, float *__restrict__ xx, float *__restrict__ xy, const DevStatus *st)
{
    const float tau = st->tau;
    const size_t gstride = (size_t)gridDim.x * BLK;
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)n; i += gstride) xx[i] = tau * xx[i];
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)m; i += gstride) xy[i] = tau * xy[i];
}
__global__ void resume_flags_k(DevStatus *st)
{
    st->state = THIP_ST_RUNNING;
    st->iter = st->iter + 1;
    st->stop = 0;
}

// sum of `np` block partials of `nq` quantities (part[q*np + k]) -> out[q]; one block (init only)
__global__ void sum_partials_k(int nq, int np, const float *__restrict__ part, float *__restrict__ out,
                               const int *__restrict__ stop)
{
    if (stop != nullptr && *stop != 0) return;
    __shared__ double shd[16];
    for (int q = 0; q < nq; ++q) {
        double acc = 0.0;
        for (int k = threadIdx.x; k < np; k += blockDim.x) acc += (double)part[(size_t)q * np + k];
        acc = block_sum_d(acc, shd);
        if (threadIdx.x == 0) out[q] = (float)acc;
        __syncthreads();
    }
}

__global__ void init_status_k(DevStatus *st, float norm_b_sq_dummy)
{
    (void)norm_b_sq_dummy;
    st->stop = 0; st->state = THIP_ST_RUNNING; st->kind = 0; st->iter = 0; st->fault = 0;
    st->cri[0] = st->cri[1] = st->cri[2] = 0.0f;
    st->tau = 1.0f; st->kappa = 0.0f; st->r_tau = 0.0f;
}

// norms + scalar preconditioner entries (solver.rs:460-481, 159-183, 501-506)
//   sums[0] = sum b^2 (all-reduced), sums[1] = sum |b| (all-reduced), loc[0] = sum c^2, loc[1] = sum |c|
__global__ void init_scalars_k(const float *__restrict__ sums, const float *__restrict__ loc, float eps_zero,
                               DevStatus *st)
{
    // fr_norm (solver.rs:85-107): n = norm(col); sq_norm += n*n; sqrt(sq_norm)
    const float nb = sqrtf(sums[0]), nc = sqrtf(loc[0]);
    st->norm_b = sqrtf(nb * nb);
    st->norm_c = sqrtf(nc * nc);
    const float tau_tau = loc[1] + sums[1];            // c.absadd_cols + b.absadd_cols (solver.rs:171-172)
    st->t_tau = 1.0f / fmaxf(tau_tau, eps_zero);
    st->s_kappa = 1.0f / fmaxf(tau_tau, eps_zero);     // sigma_1 = tau_tau (solver.rs:182)
}

// block partials of sum b^2, sum |b| (q0,q1 over m) and sum c^2, sum |c| (q2,q3 over n)
__global__ void init_sums_k(int m, const float *__restrict__ b, int n, const float *__restrict__ c,
                            float *__restrict__ part)
{
    __shared__ float sh[16];
    float b2 = 0.0f, b1 = 0.0f, c2 = 0.0f, c1 = 0.0f;
    const size_t gstride = (size_t)gridDim.x * BLK;
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)m; i += gstride) { const float t = b[i]; b2 = fmaf(t, t, b2); b1 += fabsf(t); }
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)n; i += gstride) { const float t = c[i]; c2 = fmaf(t, t, c2); c1 += fabsf(t); }
    b2 = block_sum(b2, sh); b1 = block_sum(b1, sh); c2 = block_sum(c2, sh); c1 = block_sum(c1, sh);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = b2; part[gridDim.x + blockIdx.x] = b1;
        part[2 * gridDim.x + blockIdx.x] = c2; part[3 * gridDim.x + blockIdx.x] = c1;
    }
}

// vector preconditioners (solver.rs:159-183 then 501-506):
//   tau_x = colabs(A) + |c| ; tau_y = rowabs(A) + rowabs(b) ; tau_s = 1
//   sigma_n = tau_x ; sigma_m = tau_y + tau_s
__global__ void precond_k(int n, int m, const float *__restrict__ colabs, const float *__restrict__ rowabs,
                          const float *__restrict__ c, const float *__restrict__ b, const float *__restrict__ b_rowabs,
                          float eps_zero, float *__restrict__ Tx, float *__restrict__ Ty, float *__restrict__ Ts,
                          float *__restrict__ Su, float *__restrict__ Sv)
{
    const size_t gstride = (size_t)gridDim.x * BLK;
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)n; i += gstride) {
        const float t = colabs[i] + fabsf(c[i]);
        const float r = 1.0f / fmaxf(t, eps_zero);
        Tx[i] = r; Su[i] = r;
    }
    for (size_t i = blockIdx.x * (size_t)BLK + threadIdx.x; i < (size_t)m; i += gstride) {
        const float t = rowabs[i] + (b_rowabs ? b_rowabs[i] : fabsf(b[i]));
        Ty[i] = 1.0f / fmaxf(t, eps_zero);
        Ts[i] = 1.0f / fmaxf(1.0f, eps_zero);
        Sv[i] = 1.0f / fmaxf(t + 1.0f, eps_zero);
    }
}

// Cross-stream hand-offs of the column-split pipeline without events: the producer stream runs signal_k after its last
// kernel (in stream order), the consumer stream runs gate_k, which spins until the flag has reached the value.  A
// hipEventRecord / hipStreamWaitEvent pair leaves ~13 us of idle stream behind the record on this part (rocprof timeline,
// DESIGN.md 6.1); a one-thread kernel boundary costs 2-3 us.  Every gate is enqueued (host order) after its signal, so
// the pair is satisfiable on any queue mapping; a gate gives up after ~2 s and raises err instead of hanging the GPU.
__global__ void signal_k(unsigned *flag, unsigned val)
{
    __hip_atomic_store(flag, val, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void gate_k(const unsigned *flag, unsigned val, long long timeout_ticks, unsigned *err, int *stop)
{
    const long long t0 = wall_clock64();
    while ((int)(__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - val) < 0) {
        __builtin_amdgcn_s_sleep(4);
        if (wall_clock64() - t0 > timeout_ticks) {
            // the sums this gate waits for never came: nothing enqueued behind it may touch the iterate (every kernel of the
            // loop returns at entry on the stop flag); the host reads the error word after the batch (thip_solver_run)
            atomicExch(err, 1u);
            __hip_atomic_store(stop, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
    }
}

// thip_test_spin_allreduce: a stand-in collective that only takes time -- one thread spinning on the constant-rate
// device clock for `ticks`, on whatever stream the hook is given
__global__ void spin_k(long long ticks)
{
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}

// the snapshot of the consistent iterate the one-pass schedule keeps per batch (and its restore): seven contiguous pieces
// of the arena and the status block in ONE launch
struct SnapArgs { const float *src[7]; float *dst[7]; size_t len[7]; const DevStatus *st_src; DevStatus *st_dst; };
__global__ __launch_bounds__(BLK) void snap_copy_k(const SnapArgs a)
{
    typedef float f4 __attribute__((ext_vector_type(4)));
    const size_t stride = (size_t)gridDim.x * BLK;
    for (int q = 0; q < 7; ++q) {
        const f4 *sp = reinterpret_cast<const f4 *>(a.src[q]);
        f4 *dp = reinterpret_cast<f4 *>(a.dst[q]);
        for (size_t i = (size_t)blockIdx.x * BLK + threadIdx.x; i < a.len[q] / 4; i += stride) dp[i] = sp[i];      // lengths are multiples of 64
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.st_dst = *a.st_src;
}

}  // namespace
