// thip_step.h -- the per-element arithmetic of one step of the iteration (solver.rs:538-567) and of its termination test
// (solver.rs:381-451), once, for every loop that carries it: the reference / fused / carried schedules and the m-tail of the
// one-pass schedule (thip_solver_kernels.inc), the cone projections (thip_cone.hip) and the own-A batches (thip_ownbatch.h,
// thip_smallbatch.hip, thip_midstream.h).  Plain functions of register values: nothing here touches A, a launch shape or LDS.
// Copies that remain, each because the shared text compiled to more or other instructions there (NOTEBOOK 21): the one-pass
// kernel's epilogue (thip_sweep_kernel.h) and the tiled sparse copy's (thip_sptile.hip) hold the Kahan add, the u / x_x increments
// and crit_d -- sweep_k sits on the 256-VGPR cliff and is left as compiled; ob_criteria_sums (thip_ownbatch.h) spells p and d out
// under one 1 / tau for its two loops (crit_p and crit_d there each form their own); sw_xm_k and sw_cone_k each hold the folded test.
//
// Three rules shape these functions (NOTEBOOK 19): a function that needs conv / rt takes tau and forms them itself (handed in, the
// compiler loses rt == 1 / tau under conv and adds a select per trip); a verdict keeps the state in a local and writes it once;
// fields of a kernel's argument block go in by value (with the block's address taken the slot's loads become flat loads).
#pragma once

#include "thip_common.h"

namespace thip {

// x + inc, optionally compensated: k carries the rounding error of the previous additions into this entry (Kahan).
// The f32 iterate otherwise stops moving once an update is below half an ulp of the entry while the dual residual
// is still ~1e-5..1e-4 (a floor the reference's f32 arithmetic has too; numpy emulation: 6.3e-6 -> 1e-7 at n = 200).
__device__ __forceinline__ float kahan_add(float x, float inc, bool comp, float &k)
{
    if (!comp) return x + inc;
    const float y = inc - k;
    const float t = x + y;
    k = (t - x) - y;
    return t;
}

// kahan_add for call sites that hold a pointer: the term is kval = k[i], already loaded (kahan_add_to), or loaded here
// (kahan_add_at); the new term goes to k[i].  k is neither read nor written unless comp
__device__ __forceinline__ float kahan_add_to(float x, float inc, bool comp, float kval, float *k, size_t i)
{
    if (!comp) return x + inc;
    const float r = kahan_add(x, inc, true, kval);
    k[i] = kval;
    return r;
}
__device__ __forceinline__ float kahan_add_at(float x, float inc, bool comp, float *k, size_t i)
{ if (!comp) return x + inc; return kahan_add_to(x, inc, true, k[i], k, i); }

// ---- the increments (SelfDualEmbed::trans_op solver.rs:133-157 and ::op solver.rs:109-131 under the preconditioner) -------------
// x += T o (-K^T y), solver.rs:538-555:   x_x += Tx o (gT + c kappa), gT = A^T v ; x_y += Ty o (-hN + b kappa), hN = A u ; x_s += Ts o v
__device__ __forceinline__ float inc_xx(float Tx, float gT, float c, float kappa) { return Tx * (gT + c * kappa); }
__device__ __forceinline__ float inc_xy(float Ty, float b, float kappa, float hN) { return Ty * (b * kappa - hN); }
__device__ __forceinline__ float inc_xs(float Ts, float v) { return Ts * v; }
// y += S o (-K rx), solver.rs:557-567:   u += Su o (-g2 - c rtau), g2 = A^T rx_y ; v += Sv o (h2 + rx_s - b rtau), h2 = A rx_x
__device__ __forceinline__ float inc_u(float Su, float g2, float c, float rtau) { return Su * (-g2 - c * rtau); }
__device__ __forceinline__ float inc_v(float Sv, float h2, float rxs, float b, float rtau) { return Sv * (h2 + rxs - b * rtau); }
// rx = x_k - 2 x_{k+1} (solver.rs:538,555), and by linearity the carried form of a product with it: K rx = K x_k - 2 K x_{k+1}
__device__ __forceinline__ float rx_fold(float old, float nw) { return old - 2.0f * nw; }

// the element-wise cones of one row by its class byte, and rx: k = 0 zero cone (dual: identity, primal: 0; cone_zero.rs:38-44),
// k = 1 nonnegative (max(., 0) both; cone_rpos.rs:38-45), k >= 2 member of a block cone -- projected later, which also finishes
// rx for those rows, so rx = x_k there
__device__ __forceinline__ void cone_elementwise(unsigned char k, float &ny, float &ns)
{
    if (k == 1) { ny = fmaxf(ny, 0.0f); ns = fmaxf(ns, 0.0f); }
    else if (k == 0) { ns = 0.0f; }
}
__device__ __forceinline__ float cone_rx(unsigned char k, float old, float nw) { return (k < 2) ? rx_fold(old, nw) : old; }

// ---- second-order and rotated second-order cones (cone_soc.rs:38-65, cone_rotsoc.rs:38-65) ----------------------------------------
// cone_soc.rs:49-61: the factor f of the tail and the new head from the head s0 and ||v||.  F: the type the factor, the new head
// and (soc_scaled) the products with the factor are formed in.  In f32 1 + s0 / ||v|| cancels near s0 = -||v|| (one ulp inside that
// edge the f32 factor is off by a quarter of its value), and one ulp inside s0 = ||v|| it rounds to 1; in f64 each result is the
// f64 one rounded once.  soc_k forms them in f64; the own-A batches and the one-launch m-tail in f32, as recorded in their bits
template <class F>
__device__ __forceinline__ void soc_scale(float s0, float norm_v, F &f, float &s_new)
{
    if (norm_v <= -s0) { f = (F)0; s_new = 0.0f; }
    else if (norm_v <= s0) { f = (F)1; s_new = s0; }
    else { f = ((F)1 + (F)s0 / (F)norm_v) / (F)2; s_new = (float)(((F)norm_v + (F)s0) / (F)2); }
}
template <class F>
__device__ __forceinline__ float soc_scaled(F f, float x) { return (float)(f * (F)x); }

// one cone x[beg .. end) by one group of gsz lanes (gid: this lane's index in it): a wave, or with BLOCK the 256-thread block
// (shd: 16 doubles of LDS).  rx != NULL: after the projection rx <- rx - 2 x over the cone's rows (solver.rs:555 folded in); without
// it a cone that is left unchanged is not written.  I: the type of the row indices
template <class F, class I, bool BLOCK>
__device__ __forceinline__ void soc_project(float *x, float *rx, I beg, I end, int rotated, int gid, int gsz, double *shd)
{
    const I len = end - beg;
    if (len <= 0) return;                  // uniform per group
    const float fsqrt2 = sqrtf(2.0f);

    if (rotated && len == 1) {             // cone_rotsoc.rs:46-49
        if (gid == 0) {
            const float v = fmaxf(x[beg], 0.0f);
            x[beg] = v;
            if (rx) rx[beg] = rx_fold(rx[beg], v);
        }
        return;
    }

    float s0, v1 = 0.0f;
    if (rotated) {                         // cone_rotsoc.rs:51-54
        const float r = x[beg], s = x[beg + 1];
        s0 = (r + s) / fsqrt2;
        v1 = (r - s) / fsqrt2;
    } else {
        s0 = x[beg];
    }

    // ||v|| over x[beg+1 .. end): the reference takes LinAlg::norm (cone_soc.rs:47), an nrm2 that neither underflows nor
    // overflows on the squares -- here the squares are f64
    double acc = 0.0;
    for (I i = beg + 1 + gid; i < end; i += gsz) {
        const double t = (double)((rotated && i == beg + 1) ? v1 : x[i]);
        acc += t * t;
    }
    const double sumsq = BLOCK ? block_sum_d(acc, shd) : wave_sum_d(acc);
    const float norm_v = (float)sqrt(sumsq);

    F f;
    float s_new;
    soc_scale<F>(s0, norm_v, f, s_new);

    if (!rotated) {
        if (f == (F)1 && rx == nullptr) return;
        if (gid == 0) {
            x[beg] = s_new;
            if (rx) rx[beg] = rx_fold(rx[beg], s_new);
        }
        for (I i = beg + 1 + gid; i < end; i += gsz) {
            const float nv = (f == (F)1) ? x[i] : soc_scaled<F>(f, x[i]);
            x[i] = nv;
            if (rx) rx[i] = rx_fold(rx[i], nv);
        }
    } else {
        const float v1n = soc_scaled<F>(f, v1);
        for (I i = beg + 2 + gid; i < end; i += gsz) {
            const float nv = (f == (F)1) ? x[i] : soc_scaled<F>(f, x[i]);
            x[i] = nv;
            if (rx) rx[i] = rx_fold(rx[i], nv);
        }
        if (gid == 0) {                    // cone_rotsoc.rs:58-61
            const float a = (s_new + v1n) / fsqrt2, b = (s_new - v1n) / fsqrt2;
            x[beg] = a;
            x[beg + 1] = b;
            if (rx) { rx[beg] = rx_fold(rx[beg], a); rx[beg + 1] = rx_fold(rx[beg + 1], b); }
        }
    }
}

// ---- the criteria (criteria_conv solver.rs:592-597, criteria_inf solver.rs:631-634) and the verdict --------------------------------
// one entry of p:  tau > eps_zero: x_s / tau - b + h / tau, h = A x_x (solver.rs:592-594) ; else x_s + h (solver.rs:631-632)
__device__ __forceinline__ float crit_p(float tau, float eps_zero, float xs, float b, float h)
{
    float p;
    if (tau > eps_zero) { const float rt = 1.0f / tau; p = xs * rt - b; p = fmaf(rt, h, p); }
    else p = xs + h;
    return p;
}

// one entry of d:  tau > eps_zero: c + g / tau, g = A^T x_y (solver.rs:596-597) ; else g (solver.rs:634)
__device__ __forceinline__ float crit_d(float tau, float eps_zero, float c, float g) { return (tau > eps_zero) ? fmaf(1.0f / tau, g, c) : g; }

// the termination test (solver.rs:381-451 + the tails of criteria_conv / criteria_inf, solver.rs:599-611, 636-655) of the iterate
// whose tau this is, from the four sums pp = ||p||^2, by = b.x_y, dd = ||d||^2, cx = c.x_x: the kind (0: tau > eps_zero, the
// criteria of convergence; 1: tau -> 0, those of unboundedness and infeasibility), the three criteria and the state (THIP_ST_*;
// `state` as given where the loop goes on).  Uniform where every thread holds the same sums
struct StepVerdict { int state, kind; float cri0, cri1, cri2; };
__device__ __forceinline__ StepVerdict step_verdict(float tau, long long iter, float norm_b, float norm_c, float eps_acc,
                                                    float eps_inf, float eps_zero, long long max_iter, float pp, float by,
                                                    float dd, float cx, int state)
{
    StepVerdict o;
    const bool excess_iter = (max_iter >= 0) ? (iter + 1 >= max_iter) : false;
    const float norm_p = sqrtf(pp), norm_d = sqrtf(dd);
    if (tau > eps_zero) {
        const float rt = 1.0f / tau;
        const float g_x = rt * cx;
        const float g_y = rt * by;
        const float g = g_x + g_y;
        const float cri_pri = norm_p / (1.0f + norm_b);
        const float cri_dual = norm_d / (1.0f + norm_c);
        const float cri_gap = fabsf(g) / (1.0f + fabsf(g_x) + fabsf(g_y));
        o.kind = 0; o.cri0 = cri_pri; o.cri1 = cri_dual; o.cri2 = cri_gap;
        const bool term_conv = (cri_pri <= eps_acc) && (cri_dual <= eps_acc) && (cri_gap <= eps_acc);
        if (term_conv) state = THIP_ST_OK;
        else if (excess_iter) state = THIP_ST_EXCESS_ITER;
    } else {
        const float m_cx = -cx;
        const float m_by = -by;
        const float cri_unbdd = (m_cx > eps_zero) ? norm_p * norm_c / m_cx : __builtin_inff();
        const float cri_infeas = (m_by > eps_zero) ? norm_d * norm_b / m_by : __builtin_inff();
        o.kind = 1; o.cri0 = cri_unbdd; o.cri1 = cri_infeas; o.cri2 = 0.0f;
        const bool term_unbdd = cri_unbdd <= eps_inf, term_infeas = cri_infeas <= eps_inf;
        if (term_unbdd) state = THIP_ST_UNBOUNDED;
        else if (term_infeas) state = THIP_ST_INFEASIBLE;
        else if (excess_iter) state = THIP_ST_EXCESS_ITER;
    }
    o.state = state;
    return o;
}

}  // namespace thip
