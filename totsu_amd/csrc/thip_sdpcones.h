// thip_sdpcones.h -- the PSD cones of the streamed own-A batches, shared by the SDP batch (thip_sdpbatch.hip) and the ragged batch
// (thip_raggedbatch.hip): the projection of one cone of order k <= 64 by the problem's own workgroup (sp_project; described at the
// top of thip_sdpbatch.hip), the hook of the block-cone phase that walks a problem's PSD cones (SpCones), and the shape rule both
// batches take a problem by (sp_check, sp_lds_for: no device needed).  thip_widebatch.hip runs the same cones on vectors that lie in
// the arena (SpCones::placed) under a rule of its own.
// Included once by each of the translation units that run PSD cones (on top of thip_midstream.h): everything here is internal to the one that
// includes it.
#pragma once

#include "thip_midstream.h"

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int SP_MAX_ORDER = 64, SP_OP32 = 32 * 33, SP_OP64 = 64 * 65;
static_assert(4 * SP_OP32 <= MB_SCRH + MB_SCRG && SP_OP64 <= MB_SCRH + MB_SCRG, "the operands that overlay the pass scratch fit it");

// floats the projection adds behind the class bytes for a layout whose largest PSD order is max_k (0: no PSD cone)
__host__ __device__ inline size_t sp_tail_floats(int max_k) { return max_k > 32 ? 3 * (size_t)SP_OP64 : 0; }

// C = alpha * (FORM 0: A B^T, FORM 1: A B) + beta * D + gamma * I_k on this wave's quadrant (ps_gemm of thip_eig_gemm.inc with
// a run-time number of MFMA steps nk, a multiple of 4; the columns k .. 2 nk - 1 are zero padding inside the operands).
// Operands: row-major, pitch P.  Ends with a barrier
template <int FORM, int P>
__device__ __forceinline__ void sp_gemm(float *C, const float *A, const float *B, const float *D, float alpha, float beta, float gamma,
                                        int k, int nk, int qi, int qj, int h, int li, bool live)
{
    if (live) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const float *pa = A + (32 * qi + li) * P + h;
        const float *pb = FORM == 0 ? B + (32 * qj + li) * P + h : B + h * P + 32 * qj + li;
        constexpr int SB = FORM == 0 ? 2 : 2 * P;
        for (int u0 = 0; u0 < nk; u0 += 4) {
            float av[4], bv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { av[u] = pa[2 * (u0 + u)]; bv[u] = pb[SB * (u0 + u)]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = 32 * qi + (r & 3) + 8 * (r >> 2) + 4 * h, j = 32 * qj + li;
            float v = alpha * acc[r];
            if (D != nullptr) v = fmaf(beta, D[i * P + j], v);
            if (i == j && i < k) v += gamma;
            C[i * P + j] = v;
        }
    }
    __syncthreads();
}

// x (packed, k (k + 1) / 2 entries) <- its projection onto the PSD cone, by the whole workgroup (every thread calls; blockDim.x a
// multiple of 64, >= 256 when E == 64); rx != nullptr: rx <- rx - 2 x rides in the pack.  E: the operands' extent (32: k <= 32, 64),
// o0 .. o3: four operands of E * (E + 1) floats, shd: 16 doubles.  Begins with the caller's barrier behind it (x is visible), ends
// with a barrier (x, rx are visible, the operands are free)
template <int E>
__device__ __forceinline__ void sp_project(float *x, float *rx, int k, float *o0, float *o1, float *o2, float *o3, double *shd)
{
    constexpr int P = E + 1;
    // (the thread index is made opaque here: every per-lane address below is then computed inside the projection instead of being
    // hoisted out of the iteration loop, where it would be live across the passes over A and push the kernel into scratch)
    int tid = (int)threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int T = (int)blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int qi = wave >> 1, qj = wave & 1, h = lane >> 5, li = lane & 31;
    // a quadrant that is all padding is neither computed nor read (the operands' padding is zero from the unpack on)
    const bool live = wave < (E == 32 ? 1 : 4) && 32 * qi < k && 32 * qj < k;
    const int nk = ((k + 7) / 8) * 4;
    const float scale = sqrtf(2.0f);
    auto entry = [&](int r, int c) {
        float v = 0.0f;
        if (r < k && c < k) {
            const int lo = r < c ? r : c, hi = r < c ? c : r;
            v = x[hi * (hi + 1) / 2 + lo];
            if (r == c) v *= scale;
        }
        return v;
    };
    double acc = 0.0;
    for (int e = tid; e < E * E; e += T) {
        const int r = e % E, c = e / E;
        const float v = entry(r, c);
        acc += (double)v * (double)v;
        o0[r * P + c] = v;
        o1[r * P + c] = 0.0f; o2[r * P + c] = 0.0f; o3[r * P + c] = 0.0f;
    }
    acc = block_sum_d(acc, shd);
    const float fro = (float)sqrt(acc);
    // a DIVISION per element, not a multiplication by 1 / fro: the reciprocal of a subnormal norm is infinite (a slack block on its
    // way to zero gets there), and 0 * inf poisons the iterate.  The exact zero matrix stays zero.
    for (int e = tid; e < E * E; e += T) {
        const int o = (e % E) * P + e / E;
        o0[o] = fro > 0.0f ? o0[o] / fro : 0.0f;
    }
    __syncthreads();
    float *S = o0, *Z = o1, *const Y = o2, *const Tm = o3;
#pragma unroll 1
    for (int it = 0; it < 14; ++it) {
        // 11 lifting quintics (the first on 1.7 x; band [0.3, 1.7], gain 3.94), 3 minimax quintics
        float a, b, c;
        if (it == 0) { a = 4.02942496f * 1.7f; b = -3.82532605f * 4.913f; c = 0.95951948f * 14.19857f; }
        else if (it < 11) { a = 4.02942496f; b = -3.82532605f; c = 0.95951948f; }
        else if (it == 11) { a = 2.647997920f; b = -1.945904487f; c = 0.440483961f; }
        else if (it == 12) { a = 1.967564378f; b = -1.351306898f; c = 0.386705679f; }
        else { a = 1.884943743f; b = -1.269148602f; c = 0.384197480f; }
        sp_gemm<0, P>(Y, S, S, nullptr, 1.0f, 0.0f, 0.0f, k, nk, qi, qj, h, li, live);          // Y = S S^T
        sp_gemm<1, P>(Tm, Y, Y, Y, c, b, a, k, nk, qi, qj, h, li, live);                        // T = c Y Y + b Y + a I
        sp_gemm<1, P>(Z, Tm, S, nullptr, 1.0f, 0.0f, 0.0f, k, nk, qi, qj, h, li, live);         // Z = T S
        float *t = S; S = Z; Z = t;
    }
    sp_gemm<0, P>(Tm, S, S, nullptr, -0.5f, 0.0f, 1.5f, k, nk, qi, qj, h, li, live);            // one Newton-Schulz step
    sp_gemm<1, P>(Z, Tm, S, nullptr, 1.0f, 0.0f, 0.0f, k, nk, qi, qj, h, li, live);
    { float *t = S; S = Z; Z = t; }
    for (int e = tid; e < E * E; e += T) Y[(e % E) * P + e / E] = entry(e % E, e / E);           // M again: Y is dead, x is unwritten
    __syncthreads();
    sp_gemm<1, P>(Z, Y, S, nullptr, 1.0f, 0.0f, 0.0f, k, nk, qi, qj, h, li, live);              // M sign(M)
    for (int e = tid; e < E * E; e += T) {
        const int r = e % E, c = e / E;
        if (r <= c && c < k) {
            float v = 0.5f * (Y[r * P + c] + 0.5f * (Z[r * P + c] + Z[c * P + r]));
            if (r == c) v = v / scale;
            const int o = c * (c + 1) / 2 + r;
            x[o] = v;
            if (rx != nullptr) rx[o] = rx[o] - 2.0f * v;
        }
    }
    __syncthreads();
}

// scr: SP_OP64 (4 * SP_OP32 fits) floats; tail: 3 * SP_OP64 floats, touched only when k > 32
__device__ __forceinline__ void sp_project_any(float *x, float *rx, int k, float *scr, float *tail, double *shd)
{
    if (k <= 32) sp_project<32>(x, rx, k, scr, scr + SP_OP32, scr + 2 * SP_OP32, scr + 3 * SP_OP32, shd);
    else sp_project<64>(x, rx, k, scr, tail, tail + SP_OP64, tail + 2 * SP_OP64, shd);
}

// the PSD cones of the block-cone phase: one after another, x_y (whose reflection is not needed) then x_s.  operator(): every vector
// in LDS by MbMap; placed: x_y, x_s and rx_s where the body's vector placement says they lie (thip_midstream.h: MbVecs) -- the same
// walk (restated: the first form is left as it compiles)
struct SpCones {
    static constexpr bool psd = true;
    int tail;                               // where the operands behind the class bytes begin, in floats
    __device__ __forceinline__ void operator()(float *S, const MbMap &L, const ObArgs &a) const
    {
        for (int c = 0; c < a.n_cones; ++c) {
            const int kind = a.cones[3 * c + 2];
            if (kind < 2) continue;
            const int beg = a.cones[3 * c];
#pragma unroll 1
            for (int which = 0; which < 2; ++which)
                sp_project_any(S + (which ? L.xs : L.xy) + beg, which ? S + L.rxs + beg : nullptr, kind - 1, S + L.hp, S + tail,
                               reinterpret_cast<double *>(S + L.sh));
        }
    }
    __device__ __forceinline__ void placed(const MbVecs &V, const ObArgs &a) const
    {
        for (int c = 0; c < a.n_cones; ++c) {
            const int kind = a.cones[3 * c + 2];
            if (kind < 2) continue;
            const int beg = a.cones[3 * c];
#pragma unroll 1
            for (int which = 0; which < 2; ++which)
                sp_project_any((which ? V.xs : V.xy) + beg, which ? V.rxs + beg : nullptr, kind - 1, V.hp, V.lds + tail,
                               reinterpret_cast<double *>(V.sh));
        }
    }
};

const ObText SP_TEXT = { "SDP batch not initialised", "null SDP batch", "an SDP batch holds 1 .. 1048576 problems", nullptr,
                         "the workgroup size is 256 or 1024 (0: by shape)",
                         "thip_test_sdpbatch_force_threads comes before thip_sdpbatch_init" };

// the mid batch's map, and the operands behind the class bytes (the same for every workgroup size)
size_t sp_lds_for(size_t n, size_t m, int, const ObPsd &psd) { return MbMap((int)n, (int)m).bytes((int)m) + psd.tail_bytes; }

// the shape rules (no device needed): the single source of the limit
int sp_check(size_t n, size_t m, size_t n_seg, const int32_t *seg_type, const int64_t *seg_len, std::vector<int> *cones,
             std::vector<unsigned char> *cls, ObPsd *psd)
{
    if (m < 1 || m > MB_MAX_DIM || n < 1 || n > MB_MAX_DIM)
        return fail(THIP_E_INVALID, "an SDP batch takes 1 <= m <= 4096 and 1 <= n <= 4096", __FILE__, __LINE__);
    std::vector<int> local;
    if (!cones) cones = &local;
    THIP_RC(ob_segments(SP_TEXT, m, n_seg, seg_type, seg_len, cones, cls, SP_MAX_ORDER));
    ObPsd s;
    for (size_t i = 0; i + 2 < cones->size(); i += 3)
        if ((*cones)[i + 2] >= 2) { s.n_psd += 1; s.max_k = std::max(s.max_k, (*cones)[i + 2] - 1); }
    s.tail_bytes = sp_tail_floats(s.max_k) * sizeof(float);
    if (sp_lds_for(n, m, 0, s) > OB_LDS_MAX)
        return fail(THIP_E_INVALID, "the vectors of the problem (8 n + 13 m floats and 24 832 bytes) and the three operands a PSD order "
                                    "above 32 adds (49 920 bytes) do not fit the LDS of one CU", __FILE__, __LINE__);
    if (psd) *psd = s;
    return 0;
}

}  // namespace
