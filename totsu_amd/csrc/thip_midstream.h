// thip_midstream.h -- what the batches that STREAM each problem's own A share (thip_midbatch.hip: the zero, nonnegative and
// second-order cones; thip_sdpbatch.hip: those and PSD cones projected on chip; thip_raggedbatch.hip: the same on problems of
// different shapes, through the locator seam of the bodies; thip_sparsebatch.hip: a sparse A held as packed entries, through the
// matrix-policy seam; thip_raggedsparse.hip: both seams at once; thip_mid16batch.hip: the mid batch over a 16-bit copy of A, through the
// matrix-policy seam; thip_widebatch.hip: the SDP batch's iteration with all but the pass vectors left in the arena, through the
// vector-placement seam): the LDS map of a problem's vectors, the pass over A (mb_pass), the iteration's body -- the carried recurrence,
// two passes per iteration, every vector in LDS -- with one hook in the block-cone phase between the two passes, the thread choice
// and what they add to the info record.  The init kernel's body, the criteria, status_eval, the launch arguments and the whole host side are every family's: thip_ownbatch.h.
// Included once by each of the seven translation units (on top of thip_ownbatch.h): everything here is internal to the one that
// includes it.
//
// A pass (mb_pass): the rows are cut into tiles of MB_ROWS = 256 (a lane holds 4 consecutive rows: one 16-byte load per column when
// m % 4 == 0 and the problem's base is 16-byte aligned, four 4-byte loads of the same entries otherwise -- the same lanes hold the
// same entries, so both paths add in the same order), the columns into chunks of MB_CK = 8.  With R row tiles and nw waves the
// workgroup is R x S units, S = max(1, nw / R) column slices (slice s takes the chunks s, s + S, ..); wave w serves the units
// w, w + nw, ...  A unit loads the 8 columns of a chunk at once (8 independent loads in flight per lane), and every loaded entry
// feeds both h += A[:, j] xn[j] (row sums in registers across the unit's chunks) and g[j] = A[:, j] . xt (a DPP wave sum per column).
// The R partial g of a column meet in LDS (gp) per batch of CB = max(8, 2048 / R rounded down to 8) columns and are added in tile
// order; the S partial h of a row meet in LDS (hp) and are added in slice order.  No atomics: a problem's iterates are a function of
// (its data, the workgroup size, these constants) alone -- not of its index, its neighbours or the launch.
//
// LDS, in floats: [sh 64][hp 4096][gp 2048], then xx u kx ku | xy xs v ky ks kv | Tx Ty Ts Sv | hx gx (the arena's order), then
// b c rxs g h: 8 n + 13 m floats of vectors, and the class bytes.
#pragma once

#include "thip_ownbatch.h"

namespace {

constexpr int MB_ROWS = 256, MB_CK = 8, MB_SCRH = 4096, MB_SCRG = 2048;
constexpr size_t MB_MAX_DIM = 4096;

struct MbMap {
    int sh, hp, gp, xx, u, kx, ku, xy, xs, v, ky, ks, kv, Tx, Ty, Ts, Sv, hx, gx, b, c, rxs, g, h, cls, floats;
    __host__ __device__ MbMap(int n, int m)
    {
        int o = 0;
        auto take = [&](int k) { const int r = o; o += k; return r; };
        sh = take(64); hp = take(MB_SCRH); gp = take(MB_SCRG);
        xx = take(n); u = take(n); kx = take(n); ku = take(n);                                   // the arena's order: mutable part
        xy = take(m); xs = take(m); v = take(m); ky = take(m); ks = take(m); kv = take(m);
        Tx = take(n); Ty = take(m); Ts = take(m); Sv = take(m);                                  // constant after init
        hx = take(m); gx = take(n);                                                              // carried: A x_x, A^T x_y
        b = take(m); c = take(n); rxs = take(m); g = take(n); h = take(m);
        cls = o; floats = o;
    }
    __host__ __device__ size_t bytes(int m) const { return (size_t)floats * 4 + (size_t)((m + 3) & ~3); }
};
__host__ __device__ inline size_t mb_stride(size_t n, size_t m) { return 6 * n + 10 * m; }

// h = A xn (m), g = A^T xt (n) from ONE read of A (ABS: the row and column sums of |A|).  A: global, column-major, lda = m.
// Begins and ends with a barrier: the inputs written before the call are seen, the results are visible on return.
template <bool ABS, bool VEC>
__device__ __forceinline__ void mb_pass_t(const float *__restrict__ A, int m, int n, const float *xn, const float *xt, float *h, float *g,
                                          float *hp, float *gp)
{
    const int T = (int)blockDim.x, tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6, nw = T >> 6;
    const int R = (m + MB_ROWS - 1) / MB_ROWS;
    const int S = R >= nw ? 1 : nw / R;
    const int CB = max(MB_CK, (MB_SCRG / R) & ~(MB_CK - 1));
    __syncthreads();
    for (int cb0 = 0; cb0 < n; cb0 += CB) {
        const int cbn = min(CB, n - cb0);
        const int nch = (cbn + MB_CK - 1) / MB_CK;
        for (int unit = w; unit < R * S; unit += nw) {
            const int r = unit % R, s = unit / R;
            const int row = r * MB_ROWS + lane * 4;
            const bool in0 = row < m, in1 = row + 1 < m, in2 = row + 2 < m, in3 = row + 3 < m;
            float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;
            if (ABS) {
                t0 = t1 = t2 = t3 = 1.0f;
            } else {
                if (in0) t0 = xt[row];
                if (in1) t1 = xt[row + 1];
                if (in2) t2 = xt[row + 2];
                if (in3) t3 = xt[row + 3];
            }
            auto ld = [&](int j) {
                float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                const float *p = A + (size_t)j * (size_t)m + row;
                if (VEC) {
                    if (in0) q = *reinterpret_cast<const float4 *>(p);      // (m % 4 == 0: all four rows or none)
                } else {
                    if (in0) q.x = p[0];
                    if (in1) q.y = p[1];
                    if (in2) q.z = p[2];
                    if (in3) q.w = p[3];
                }
                if (ABS) { q.x = fabsf(q.x); q.y = fabsf(q.y); q.z = fabsf(q.z); q.w = fabsf(q.w); }
                return q;
            };
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
            for (int ch = s; ch < nch; ch += S) {
                const int j0 = cb0 + ch * MB_CK;
                const int nj = min(MB_CK, cb0 + cbn - j0);
                float4 q[MB_CK];
                float xj[MB_CK];
                if (nj == MB_CK) {
#pragma unroll
                    for (int k = 0; k < MB_CK; ++k) q[k] = ld(j0 + k);
#pragma unroll
                    for (int k = 0; k < MB_CK; ++k) xj[k] = ABS ? 1.0f : xn[j0 + k];
                } else {
#pragma unroll
                    for (int k = 0; k < MB_CK; ++k) {
                        q[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        xj[k] = 0.0f;
                        if (k < nj) { q[k] = ld(j0 + k); xj[k] = ABS ? 1.0f : xn[j0 + k]; }
                    }
                }
#pragma unroll
                for (int k = 0; k < MB_CK; ++k) {
                    a0 = fmaf(q[k].x, xj[k], a0); a1 = fmaf(q[k].y, xj[k], a1);
                    a2 = fmaf(q[k].z, xj[k], a2); a3 = fmaf(q[k].w, xj[k], a3);
                    float d = q[k].x * t0;
                    d = fmaf(q[k].y, t1, d); d = fmaf(q[k].z, t2, d); d = fmaf(q[k].w, t3, d);
                    d = wave_sum_dpp(d);
                    if (lane == 0 && k < nj) gp[r * CB + (j0 + k - cb0)] = d;
                }
            }
            // the unit's row sums: (s, row) is this lane's alone
            float *hs = hp + s * m + row;
            if (cb0 == 0) {
                if (in0) hs[0] = a0;
                if (in1) hs[1] = a1;
                if (in2) hs[2] = a2;
                if (in3) hs[3] = a3;
            } else {
                if (in0) hs[0] += a0;
                if (in1) hs[1] += a1;
                if (in2) hs[2] += a2;
                if (in3) hs[3] += a3;
            }
        }
        __syncthreads();
        for (int t = tid; t < cbn; t += T) {
            float acc = gp[t];
            for (int r = 1; r < R; ++r) acc += gp[r * CB + t];
            g[cb0 + t] = acc;
        }
        __syncthreads();
    }
    for (int i = tid; i < m; i += T) {
        float acc = hp[i];
        for (int s = 1; s < S; ++s) acc += hp[s * m + i];
        h[i] = acc;
    }
    __syncthreads();
}

template <bool ABS>
__device__ __forceinline__ void mb_pass(const float *A, bool vec, int m, int n, const float *xn, const float *xt, float *h, float *g,
                                        float *hp, float *gp)
{
    if (vec) mb_pass_t<ABS, true>(A, m, n, xn, xt, h, g, hp, gp);
    else mb_pass_t<ABS, false>(A, m, n, xn, xt, h, g, hp, gp);
}

__device__ __forceinline__ bool mb_vec(const float *a, int m) { return (m & 3) == 0 && ((uintptr_t)a & 15u) == 0; }

// ---- the pass over a 16-bit store (thip_mid16batch.hip) --------------------------------------------------------------------------
// A problem's block of the store: n columns of ld16 = roundup4(m) 16-bit words, column-major, the pad rows zero; KIND THIP_A_F16: n
// floats inv_s behind the matrix; the block a multiple of 16 bytes.  The WIDENED matrix W is what a pass works on: THIP_A_BF16 the word
// shifted left 16 bits, THIP_A_F16 float(h) * inv_s[c] (one f32 multiply per entry, at widen time).  mb16_pass_t is mb_pass_t on W:
// the same lanes hold the same entries (a lane's 4 consecutive rows are one 8-byte load: ld16 is a multiple of 4 and the block is
// aligned, so there is no other path), the same chunks go to the same slices and every sum is formed in mb_pass_t's order -- a pad
// entry is +0 and adds what that pass's unloaded zero adds.  A unit keeps two chunks of 8 columns in flight (128 bytes per lane, as
// the f32 pass holds) and works them off one after the other, in the chunk order of mb_pass_t.
constexpr size_t mb16_ld(size_t m) { return (m + 3) & ~(size_t)3; }
__host__ __device__ inline size_t mb16_block_bytes(size_t n, size_t m, int kind)
{
    return (2 * mb16_ld(m) * n + (kind == THIP_A_F16 ? 4 * n : 0) + 15) & ~(size_t)15;
}

// the store is global memory: said to the compiler, which does not see it of a pointer that went through the slot and a cast of its
// element type (the loads would be flat ones)
typedef unsigned mb16_u2 __attribute__((ext_vector_type(2)));
typedef const mb16_u2 __attribute__((address_space(1))) *mb16_gword;
typedef const float __attribute__((address_space(1))) *mb16_gscale;

template <int KIND>
__device__ __forceinline__ float4 mb16_widen(const mb16_u2 r, float sc)
{
    float4 q;
    if (KIND == THIP_A_BF16) {
        q.x = __uint_as_float(r.x << 16); q.y = __uint_as_float(r.x & 0xffff0000u);
        q.z = __uint_as_float(r.y << 16); q.w = __uint_as_float(r.y & 0xffff0000u);
    } else {
        // W is the ROUNDED product: the multiply must not be contracted into an addition that follows it after inlining (the |A|
        // pass adds q * 1, which the compiler would otherwise turn into one fma of the word, the scale and the sum)
#pragma clang fp contract(off)
        typedef _Float16 mb16_h2 __attribute__((ext_vector_type(2)));
        const unsigned rx = r.x, ry = r.y;                 // (scalars: a bit cast of a vector's element would read element 0 for both)
        const mb16_h2 lo = __builtin_bit_cast(mb16_h2, rx), hi = __builtin_bit_cast(mb16_h2, ry);
        q.x = (float)lo.x * sc; q.y = (float)lo.y * sc; q.z = (float)hi.x * sc; q.w = (float)hi.y * sc;
    }
    return q;
}

// A: the block as 8-byte words (a column is ld2 = ld16 / 4 of them), inv_s: the f16 column scales (unused for bf16)
template <int KIND, bool ABS>
__device__ __forceinline__ void mb16_pass_t(const uint2 *__restrict__ A, const float *__restrict__ inv_s, int ld2, int m, int n,
                                            const float *xn, const float *xt, float *h, float *g, float *hp, float *gp)
{
    const int T = (int)blockDim.x, tid = (int)threadIdx.x, lane = tid & 63, nw = T >> 6;
    // (the wave's index in a scalar register: units, chunks and column bases are then uniform to the compiler too, and a load is a
    // scalar base plus the lane's 32-bit offset, not a 64-bit address per lane and column)
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int R = (m + MB_ROWS - 1) / MB_ROWS;
    const int S = R >= nw ? 1 : nw / R;
    const int CB = max(MB_CK, (MB_SCRG / R) & ~(MB_CK - 1));
    __syncthreads();
    for (int cb0 = 0; cb0 < n; cb0 += CB) {
        const int cbn = min(CB, n - cb0);
        const int nch = (cbn + MB_CK - 1) / MB_CK;
        for (int unit = w; unit < R * S; unit += nw) {
            const int r = unit % R, s = unit / R;
            const int row = r * MB_ROWS + lane * 4;
            const bool in0 = row < m, in1 = row + 1 < m, in2 = row + 2 < m, in3 = row + 3 < m;
            float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;
            if (ABS) {
                t0 = t1 = t2 = t3 = 1.0f;
            } else {
                if (in0) t0 = xt[row];
                if (in1) t1 = xt[row + 1];
                if (in2) t2 = xt[row + 2];
                if (in3) t3 = xt[row + 3];
            }
            const char *const tile = reinterpret_cast<const char *>(A + r * (MB_ROWS / 4));      // (uniform)
            const unsigned voff = (unsigned)lane * 8u;
            float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
            // the 8 columns from j0 on (nj of them exist) as they were loaded
            auto fetch = [&](mb16_u2 (&raw)[MB_CK], int j0, int nj) {
                if (nj == MB_CK) {                                                        // (uniform: the loads go out together)
#pragma unroll
                    for (int k = 0; k < MB_CK; ++k) {
                        raw[k] = mb16_u2{ 0u, 0u };
                        if (in0) raw[k] = *(mb16_gword)(tile + (size_t)(j0 + k) * (size_t)ld2 * 8u + voff);
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < MB_CK; ++k) {
                        raw[k] = mb16_u2{ 0u, 0u };
                        if (in0 && k < nj)                                               // (row < m: the whole word lies in the column)
                            raw[k] = *(mb16_gword)(tile + (size_t)(j0 + k) * (size_t)ld2 * 8u + voff);
                    }
                }
            };
            auto work = [&](const mb16_u2 (&raw)[MB_CK], int j0, int nj) {
                const int ju = j0;                                                        // (the chunk is the wave's: a uniform index)
#pragma unroll
                for (int k = 0; k < MB_CK; ++k) {
                    float xjk = 0.0f, sck = 1.0f;
                    if (k < nj) {
                        xjk = ABS ? 1.0f : xn[ju + k];
                        if (KIND == THIP_A_F16) sck = ((mb16_gscale)inv_s)[ju + k];
                    }
                    float4 q = mb16_widen<KIND>(raw[k], sck);
                    if (ABS) { q.x = fabsf(q.x); q.y = fabsf(q.y); q.z = fabsf(q.z); q.w = fabsf(q.w); }
                    a0 = fmaf(q.x, xjk, a0); a1 = fmaf(q.y, xjk, a1);
                    a2 = fmaf(q.z, xjk, a2); a3 = fmaf(q.w, xjk, a3);
                    float d = q.x * t0;
                    d = fmaf(q.y, t1, d); d = fmaf(q.z, t2, d); d = fmaf(q.w, t3, d);
                    d = wave_sum_dpp(d);
                    if (lane == 0 && k < nj) gp[r * CB + (ju + k - cb0)] = d;
                }
            };
            for (int ch = s; ch < nch; ch += 2 * S) {
                const int jA = cb0 + ch * MB_CK, jB = jA + S * MB_CK;
                const int njA = min(MB_CK, cb0 + cbn - jA);
                const bool two = ch + S < nch;                                            // (uniform)
                const int njB = two ? min(MB_CK, cb0 + cbn - jB) : 0;
                mb16_u2 ra[MB_CK], rb[MB_CK];
                fetch(ra, jA, njA);
                fetch(rb, jB, njB);
                __builtin_amdgcn_sched_barrier(0);                                        // (every load issued before the first use;
                work(ra, jA, njA);                                                        // the second chunk's words stay packed until
                __builtin_amdgcn_sched_barrier(0);                                        // the first is worked off: registers)
                if (two) work(rb, jB, njB);
            }
            // the unit's row sums: (s, row) is this lane's alone
            float *hs = hp + s * m + row;
            if (cb0 == 0) {
                if (in0) hs[0] = a0;
                if (in1) hs[1] = a1;
                if (in2) hs[2] = a2;
                if (in3) hs[3] = a3;
            } else {
                if (in0) hs[0] += a0;
                if (in1) hs[1] += a1;
                if (in2) hs[2] += a2;
                if (in3) hs[3] += a3;
            }
        }
        __syncthreads();
        for (int t = tid; t < cbn; t += T) {
            float acc = gp[t];
            for (int r = 1; r < R; ++r) acc += gp[r * CB + t];
            g[cb0 + t] = acc;
        }
        __syncthreads();
    }
    for (int i = tid; i < m; i += T) {
        float acc = hp[i];
        for (int s = 1; s < S; ++s) acc += hp[s * m + i];
        h[i] = acc;
    }
    __syncthreads();
}

// ---- the vector placement: the third seam of the bodies (beside AT and MAT) -------------------------------------------------------
// Where each vector of an iteration lives.  MbInLds, every family's but one: all of them in LDS by MbMap, the arena block copied in
// at launch entry and out at exit -- the bodies hold that text themselves, under `if constexpr (VP::in_lds)`, as they held it before
// the seam (a helper per phase would be optimised on its own before it is inlined, and the kernels would no longer be the ones they
// were).  Any other placement hands the body an MbVecs -- every vector as the body addresses it, wherever it lies (vecs: those in
// LDS, from its map alone; place: those in the problem's arena block or behind its slot, once the body knows them) -- and says what
// the load phase copies into LDS (load), what the store phase copies back (store_mut), where a start puts the iterate it is handed
// (start_fill), and which map the init-time bodies lay b c g h Ty Ts out by (InitMap; sync_maps: the barrier between a use of that
// map and one of the iteration's where the two overlap).  The arithmetic between those phases is one text for every placement.
// thip_widebatch.hip hands in the placement that leaves all but the pass's inputs and outputs in the arena.
// Vectors that are NOT in LDS are exchanged between lanes only across __syncthreads() -- a workgroup-scope release and acquire, which
// covers the plain global stores and loads of one workgroup -- and are never read through __restrict__ or non-temporal paths.
struct MbVecs {
    float *lds;                                                                 // the map's base (the PSD tail lies behind the map)
    float *sh, *hp, *gp;
    float *xx, *u, *kx, *ku, *xy, *xs, *v, *ky, *ks, *kv;
    const float *Tx, *Ty, *Ts, *Sv;
    float *hx, *gx;
    const float *b, *c;
    float *rxs, *g, *h;
    unsigned char *cls;
};

struct MbInLds {
    static constexpr bool in_lds = true;
    using Map = MbMap;
    using InitMap = MbMap;
};

extern __shared__ float mb_lds[];

// the block-cone phase of a family without PSD cones: nothing beside the second-order cones
struct MbNoPsd {
    static constexpr bool psd = false;
    __device__ __forceinline__ void operator()(float *, const MbMap &, const ObArgs &) const {}
    __device__ __forceinline__ void placed(const MbVecs &, const ObArgs &) const {}
};

// the matrix policy of the two bodies: what the slot's `a` pointer means and what is loaded at launch entry (open: called by every
// thread, before the barrier that ends the body's load phase), and how a pass is called.  MbDenseA: the pointer is the problem's
// dense column-major A, nothing is loaded, the pass streams it (mb_pass).  thip_sparsebatch.hip hands in the policy of a sparse A
struct MbDenseA {
    struct Mat { const float *A; bool vec; };
    __device__ __forceinline__ Mat open(const float *a, int m, int, float *) const { return Mat{ a, mb_vec(a, m) }; }
    template <bool ABS>
    __device__ __forceinline__ void pass(const Mat &M, int m, int n, const float *xn, const float *xt, float *h, float *g, float *hp,
                                         float *gp) const
    {
        mb_pass<ABS>(M.A, M.vec, m, n, xn, xt, h, g, hp, gp);
    }
};

// MbDenseA16<KIND>: the pointer is the problem's block of a 16-bit store (above), nothing is loaded, the pass streams the block and
// works on the widened matrix (mb16_pass_t) -- the |A| sums of the preconditioner included, so they are those of W
template <int KIND>
struct MbDenseA16 {
    struct Mat { const uint2 *A; const float *inv_s; int ld2; };
    __device__ __forceinline__ Mat open(const float *a, int m, int n, float *) const
    {
        const int ld16 = (m + 3) & ~3;
        const uint16_t *const words = reinterpret_cast<const uint16_t *>(a);
        return Mat{ reinterpret_cast<const uint2 *>(a), reinterpret_cast<const float *>(words + (size_t)n * (size_t)ld16), ld16 >> 2 };
    }
    template <bool ABS>
    __device__ __forceinline__ void pass(const Mat &M, int m, int n, const float *xn, const float *xt, float *h, float *g, float *hp,
                                         float *gp) const
    {
        mb16_pass_t<KIND, ABS>(M.A, M.inv_s, M.ld2, m, n, xn, xt, h, g, hp, gp);
    }
};

// ob_init_body with the |A| sums from one pass
template <class AT = ObUniform, class MAT = MbDenseA, class VP = MbInLds>
__device__ __forceinline__ void mb_init_body(const ObArgs &a, const AT &at = AT(), const MAT &mat = MAT(), const VP & = VP())
{
    const int n = a.n, m = a.m;
    const typename VP::InitMap L(n, m);
    float *S = mb_lds;
    ob_init_body(a, at.problem(a), L, S, [&](const float *A) {
        mat.template pass<true>(mat.open(A, m, n, S), m, n, nullptr, nullptr, S + L.h, S + L.g, S + L.hp, S + L.gp);
    }, at);
}

// ob_init_body on a staged (b, c), the |A| sums from the same pass: a problem takes a new (b, c) and keeps the A its slot points at
template <class AT = ObUniform, class MAT = MbDenseA, class VP = MbInLds>
__device__ __forceinline__ void mb_setbc_body(const ObArgs &a, const ObSetBc &sb, const AT &at = AT(), const MAT &mat = MAT(),
                                              const VP & = VP())
{
    const int n = a.n, m = a.m;
    const typename VP::InitMap L(n, m);
    float *S = mb_lds;
    ob_init_body(a, at.problem(a), L, S, [&](const float *A) {
        mat.template pass<true>(mat.open(A, m, n, S), m, n, nullptr, nullptr, S + L.h, S + L.g, S + L.hp, S + L.gp);
    }, at, ObTakeBc{ sb });
}

// `steps` whole iterations of one problem by one workgroup.  PSD: what the family does with its PSD cones between the two passes
// (called by every thread, after the second-order cones; hp, gp and g are dead there).  AT: which problem and where its arena block
// lies (thip_ownbatch.h: ObUniform, or the ragged batch's descriptor).  MAT: the matrix policy (above).  VP: the vector placement
// (above)
template <class PSD, class AT = ObUniform, class MAT = MbDenseA, class VP = MbInLds>
__device__ __forceinline__ void mb_iterate_body(const ObArgs &a, const PSD &psd_cones, const AT &at = AT(), const MAT &mat = MAT(),
                                                const VP &vp = VP())
{
    const int p = at.problem(a);
    SbStatus *const gst = a.st + p;
    if (gst->stop != 0) return;
    const int n = a.n, m = a.m, T = (int)blockDim.x, tid = (int)threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6, nw = T >> 6;
    const bool comp = a.comp != 0;
    const typename VP::Map L(n, m);
    float *S = mb_lds;
    float *sh, *hp, *gp, *xx, *u, *kx, *ku, *xy, *xs, *v, *ky, *ks, *kv, *hx, *gx, *rxs, *g, *h;
    const float *Tx, *Ty, *Ts, *Sv, *b, *c;
    unsigned char *cls;
    if constexpr (VP::in_lds) {
        sh = S + L.sh; hp = S + L.hp; gp = S + L.gp;
        xx = S + L.xx; u = S + L.u; kx = S + L.kx; ku = S + L.ku;
        xy = S + L.xy; xs = S + L.xs; v = S + L.v; ky = S + L.ky; ks = S + L.ks; kv = S + L.kv;
        Tx = S + L.Tx; Ty = S + L.Ty; Ts = S + L.Ts; Sv = S + L.Sv;
        hx = S + L.hx; gx = S + L.gx;
        b = S + L.b; c = S + L.c;
        rxs = S + L.rxs; g = S + L.g; h = S + L.h;
        cls = reinterpret_cast<unsigned char *>(S + L.cls);
    }

    // ---- load ----
    const SbSlot sl = a.slots[p];
    const auto A = mat.open(sl.a, m, n, S);
    float *const ar = at.block(a, p);
    [[maybe_unused]] MbVecs V{};                           // (a placement other than LDS alone uses it: where each vector lies)
    if constexpr (VP::in_lds) {
        {
            const int nstate = 6 * n + 10 * m;             // the arena's order is the LDS order from xx on
            for (int i = tid; i < nstate; i += T) xx[i] = ar[i];
        }
        for (int i = tid; i < m; i += T) { S[L.b + i] = sl.b[i]; cls[i] = a.cls[i]; }
        for (int i = tid; i < n; i += T) S[L.c + i] = sl.c[i];
    } else {
        V = vp.vecs(S, L);
        vp.place(V, ar, sl, n, m);
        sh = V.sh; hp = V.hp; gp = V.gp;
        xx = V.xx; u = V.u; kx = V.kx; ku = V.ku;
        xy = V.xy; xs = V.xs; v = V.v; ky = V.ky; ks = V.ks; kv = V.kv;
        Tx = V.Tx; Ty = V.Ty; Ts = V.Ts; Sv = V.Sv;
        hx = V.hx; gx = V.gx;
        b = V.b; c = V.c;
        rxs = V.rxs; g = V.g; h = V.h;
        cls = V.cls;
        vp.load(V, ar, a.cls, n, m, T, tid);
    }
    ObScalars s;
    s.load(gst);
    __syncthreads();

    for (int step = 0; step < a.steps; ++step) {
        // ---- x += T o (-K^T y): h = A u, g = A^T v; c.u, b.v, and c.x_x, b.x_y of the iterate that is about to move ----
        float q[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        for (int i = tid; i < n; i += T) { q[0] = fmaf(c[i], u[i], q[0]); q[2] = fmaf(c[i], xx[i], q[2]); }
        for (int i = tid; i < m; i += T) { q[1] = fmaf(b[i], v[i], q[1]); q[3] = fmaf(b[i], xy[i], q[3]); }
        mat.template pass<false>(A, m, n, u, v, h, g, hp, gp);
        block_sums<4>(q, sh);
        const float cx_old = q[2], by_old = q[3];
        for (int i = tid; i < n; i += T) xx[i] = kahan_add_at(xx[i], inc_xx(Tx[i], g[i], c[i], s.kappa), comp, kx, i);
        for (int i = tid; i < m; i += T) {
            const unsigned char k = cls[i];
            const float oy = xy[i], os = xs[i];
            float ny = kahan_add_at(oy, inc_xy(Ty[i], b[i], s.kappa, h[i]), comp, ky, i);
            float ns = kahan_add_at(os, inc_xs(Ts[i], v[i]), comp, ks, i);
            cone_elementwise(k, ny, ns);
            xy[i] = ny;
            xs[i] = ns;
            h[i] = oy;                                             // (rx_y is not needed: what sb_soc writes there is dropped)
            rxs[i] = cone_rx(k, os, ns);
        }
        {
            const float old = s.tau;
            s.tau = fmaxf(old + s.t_tau * (-q[0] - q[1]), 0.0f);      // solver.rs:551-552
            s.rtau = old - 2.0f * s.tau;
        }
        __syncthreads();
        // ---- the block cones: one wave per second-order cone, x_y then x_s; then the family's PSD cones ----
        if (a.n_cones > 0) {
            for (int k = wv; k < a.n_cones; k += nw) {
                const int beg = a.cones[3 * k], end = a.cones[3 * k + 1], rot = a.cones[3 * k + 2];
                if (PSD::psd && rot >= 2) continue;
                sb_soc(xy, h, beg, end, rot, lane);
                sb_soc(xs, rxs, beg, end, rot, lane);
            }
        }
        if constexpr (VP::in_lds) psd_cones(S, L, a);
        else psd_cones.placed(V, a);
        // ---- h = A x_x, g = A^T x_y of the new iterate: the criteria, and K rx = K x_k - 2 K x_{k+1} ----
        mat.template pass<false>(A, m, n, xx, xy, h, g, hp, gp);
        ob_criteria_sums(q, n, m, s.tau, a.eps_zero, b, c, xx, xy, xs, h, g, sh);
        const float pp = q[0], by = q[1], dd = q[2], cx = q[3];
        // ---- y += S o (-K rx) (ycrit_k), the pair carried on ----
        for (int i = tid; i < n; i += T) {
            const float gn = g[i];
            u[i] = kahan_add_at(u[i], inc_u(Tx[i], rx_fold(gx[i], gn), c[i], s.rtau), comp, ku, i);
            gx[i] = gn;
        }
        for (int i = tid; i < m; i += T) {
            const float hn = h[i];
            v[i] = kahan_add_at(v[i], inc_v(Sv[i], rx_fold(hx[i], hn), rxs[i], b[i], s.rtau), comp, kv, i);
            hx[i] = hn;
        }
        s.kappa = fminf(s.kappa + s.s_kappa * ((cx_old - 2.0f * cx) + (by_old - 2.0f * by)), 0.0f);     // solver.rs:566-567
        ob_status_eval(s, ObLimits{ a.eps_acc, a.eps_inf, a.eps_zero, a.max_iter }, pp, by, dd, cx);
        if (s.state != THIP_ST_RUNNING) break;                     // (uniform: every thread holds the same sums)
        s.iter += 1;
    }

    // ---- store ----
    __syncthreads();
    if constexpr (VP::in_lds) {
        const int nmut = 4 * n + 6 * m;
        for (int i = tid; i < nmut; i += T) ar[i] = xx[i];
        float *const gcar = ar + 5 * n + 9 * m;
        for (int i = tid; i < m + n; i += T) gcar[i] = hx[i];      // (gx follows hx)
    } else {
        vp.store_mut(V, ar, n, m, T, tid);                 // (everything else was updated where it lies)
    }
    if (tid == 0) s.store(gst);
}

// a problem starts from a given iterate (thip_NAME_set_iterates): its workgroup loads the staged (x, y) at `it` into the map, forms the
// carried pair of that iterate -- h = A x_x, g = A^T x_y, the call the iteration's second pass makes, so a run that is handed
// its own iterate continues bit for bit -- and writes the mutable part of the arena (Kahan terms zero), the pair and the status
// block.  The slot's data, the preconditioner and the norms stay as init left them.  AT, MAT, VP: the seams of the two bodies above
template <class AT = ObUniform, class MAT = MbDenseA, class VP = MbInLds>
__device__ __forceinline__ void mb_start_body(const ObArgs &a, const float *it, const AT &at = AT(), const MAT &mat = MAT(),
                                              const VP &vp = VP())
{
    const int p = at.problem(a);
    const int n = a.n, m = a.m, T = (int)blockDim.x, tid = (int)threadIdx.x;
    const typename VP::Map L(n, m);
    float *S = mb_lds;
    float *const xx = S + L.xx, *const xy = S + L.xy, *const h = S + L.h, *const g = S + L.g;       // (in LDS under every placement)
    const float *const x = it, *const y = it + n + 2 * m + 1;       // x_x x_y x_s tau | u v kappa
    const SbSlot sl = a.slots[p];
    const auto A = mat.open(sl.a, m, n, S);
    [[maybe_unused]] MbVecs V{};                           // (a placement other than LDS alone uses it)
    if constexpr (VP::in_lds) {
        for (int i = tid; i < n; i += T) {
            xx[i] = x[i]; S[L.u + i] = y[i];
            S[L.kx + i] = 0.0f; S[L.ku + i] = 0.0f;
        }
        for (int i = tid; i < m; i += T) {
            xy[i] = x[n + i]; S[L.xs + i] = x[n + m + i]; S[L.v + i] = y[n + i];
            S[L.ky + i] = 0.0f; S[L.ks + i] = 0.0f; S[L.kv + i] = 0.0f;
        }
    } else {
        V = vp.vecs(S, L);
        vp.place(V, at.block(a, p), sl, n, m);
        vp.start_fill(V, x, y, n, m, T, tid);
    }
    mat.template pass<false>(A, m, n, xx, xy, h, g, S + L.hp, S + L.gp);
    float *const ar = at.block(a, p);
    {
        if constexpr (VP::in_lds) {
            const int nmut = 4 * n + 6 * m;                // the arena's order is the LDS order from xx on
            for (int i = tid; i < nmut; i += T) ar[i] = xx[i];
        } else {
            vp.store_mut(V, ar, n, m, T, tid);
        }
        float *const gcar = ar + 5 * n + 9 * m;
        for (int i = tid; i < m; i += T) gcar[i] = h[i];
        for (int i = tid; i < n; i += T) gcar[m + i] = g[i];
    }
    if (tid == 0) ob_start_status(a.st + p, x[n + 2 * m], y[n + m]);
}

// a problem's A has new values (thip_NAME_set_a): ob_init_body on the slot's own b, c and row sums with the |A| sums from one pass
// over the A that lies behind the slot's pointer now, the ending taken from the call (ObKeepA).  keep == 0: init's ending, the
// carried pair zero.  keep != 0: the pair depends on A, so it is formed again from the iterate that stays in the arena -- x_x and
// x_y into the map, then h = A x_x, g = A^T x_y by the call the iteration's second pass makes, as mb_start_body forms it (restated
// here: that body is left as it compiles) -- and written behind the preconditioner.  The matrix is opened once, ahead of the body:
// a resident blob stays in LDS for both passes (the body touches neither its place nor the PSD tail in front of it)
template <class AT = ObUniform, class MAT = MbDenseA, class VP = MbInLds>
__device__ __forceinline__ void mb_seta_body(const ObArgs &a, int keep, const AT &at = AT(), const MAT &mat = MAT(), const VP &vp = VP())
{
    const int n = a.n, m = a.m, T = (int)blockDim.x, tid = (int)threadIdx.x;
    const int p = at.problem(a);
    const typename VP::InitMap L(n, m);
    float *S = mb_lds;
    const auto A = mat.open(a.slots[p].a, m, n, S);
    ob_init_body(a, p, L, S, [&](const float *) {
        mat.template pass<true>(A, m, n, nullptr, nullptr, S + L.h, S + L.g, S + L.hp, S + L.gp);
    }, at, ObKeepA{ keep });
    if (keep == 0) return;                                  // (uniform: a launch argument)
    const typename VP::Map Li(n, m);                        // (the iteration's map; MbInLds: the same one)
    float *const xx = S + Li.xx, *const xy = S + Li.xy, *const h = S + Li.h, *const g = S + Li.g;
    float *const ar = at.block(a, p);
    if constexpr (!VP::in_lds) vp.sync_maps();
    for (int i = tid; i < n; i += T) xx[i] = ar[i];         // (the body's keep ending writes the Kahan terms alone)
    for (int i = tid; i < m; i += T) xy[i] = ar[4 * n + i];
    mat.template pass<false>(A, m, n, xx, xy, h, g, S + Li.hp, S + Li.gp);
    float *const gcar = ar + 5 * n + 9 * m;
    for (int i = tid; i < m; i += T) gcar[i] = h[i];
    for (int i = tid; i < n; i += T) gcar[m + i] = g[i];
}

// ---- the host side ------------------------------------------------------------------------------------------------------------

int mb_threads_for(size_t n, size_t m) { return n * m <= 8192 ? 256 : 1024; }

// the fields of thip_midbatch_info_t, which both families' records begin with
struct MbInfo {
    template <class INFO>
    void operator()(const OwnBatch *h, INFO &o) const
    {
        ObInfo()(h, o);
        o.load_bytes = ((h->m & 3) == 0 && h->n_unaligned == 0) ? 16 : 4;
        o.a_bytes_per_iter = 2 * h->m * h->n * sizeof(float);
    }
};

// the same for a family over a 16-bit store (thip_mid16batch_info_t): one load path, the stored bytes read twice per iteration
struct Mb16Info {
    template <class INFO>
    void operator()(const OwnBatch *h, INFO &o) const
    {
        ObInfo()(h, o);
        o.load_bytes = 8;
        o.a_bytes_per_iter = 2 * (2 * mb16_ld(h->m) * h->n + (h->a_kind == THIP_A_F16 ? 4 * h->n : 0));
        o.a_dtype = h->a_kind;
        o.a_store_bytes = h->a_block * h->n_prob;
    }
};

}  // namespace
