// thip_wideplace.h -- what the two WIDE own-A families share (thip_widebatch.hip: f32 A streamed in place; thip_wide16batch.hip: a
// library-owned 16-bit copy of A): the two LDS maps, the vector placement that leaves all but the pass vectors in the problem's block
// of the arena, the arena's stride, the shape rule and the launch of an init-time kernel.  Included once by each of the two
// translation units (on top of thip_sdpcones.h): everything here is internal to the one that includes it.
//
// In LDS (WbMap): [sh 64][hp 4096][gp 2048], the pass inputs xx u xy v, the pass outputs g h, the class bytes, and -- a PSD order above
// 32 -- the three operands of the projection behind the class bytes, as in the SDP batch: 4 (6208 + 3 n + 3 m) + roundup4(m) bytes,
// plus 49 920.  In the arena, in the mid batch's layout: kx ku | xs ky ks kv | Tx Ty Ts Sv | hx gx, then rx_s (m more floats: the
// stride is 6 n + 11 m); b and c are read through the slot's pointers.  xx u xy v are loaded at launch entry and stored at exit.
// Everything else is updated where it lies, so a launch cut can change no bit by construction.
//
// The vectors in the arena are exchanged between lanes only across __syncthreads() (the element-wise phase, then sb_soc and the PSD
// unpack; the pass, then the element-wise phase): the barrier is a workgroup-scope release and acquire, the workgroup's waves share one
// vector L1, and nothing here reads these vectors through __restrict__ or non-temporal paths (a scalar or read-only path could serve a
// stale value inside the workgroup).
//
// The init-time bodies (init, set_bc, set_a) lay b c g h Ty Ts out by a map of their own (WbInitMap: 4 (6208 + 2 n + 4 m) bytes, at
// most 123 136), and their launches ask for the larger of the two maps.  wb_check is the single source of the rule.
#pragma once

#include "thip_sdpcones.h"

namespace {

using namespace thip;

// the iteration's map: what a pass touches, and the class bytes
struct WbMap {
    int sh, hp, gp, xx, u, xy, v, g, h, cls, floats;
    __host__ __device__ WbMap(int n, int m)
    {
        int o = 0;
        auto take = [&](int k) { const int r = o; o += k; return r; };
        sh = take(64); hp = take(MB_SCRH); gp = take(MB_SCRG);
        xx = take(n); u = take(n); xy = take(m); v = take(m);
        g = take(n); h = take(m);
        cls = o; floats = o;
    }
    __host__ __device__ size_t bytes(int m) const { return (size_t)floats * 4 + (size_t)((m + 3) & ~3); }
};

// the init-time bodies' map: what ob_init_body keeps in LDS
struct WbInitMap {
    int sh, hp, gp, b, c, g, h, Ty, Ts, floats;
    __host__ __device__ WbInitMap(int n, int m)
    {
        int o = 0;
        auto take = [&](int k) { const int r = o; o += k; return r; };
        sh = take(64); hp = take(MB_SCRH); gp = take(MB_SCRG);
        b = take(m); c = take(n); g = take(n); h = take(m); Ty = take(m); Ts = take(m);
        floats = o;
    }
    __host__ __device__ size_t bytes() const { return (size_t)floats * 4; }
};

// the arena block: the mid batch's, and rx_s behind the carried pair
__host__ __device__ inline size_t wb_stride(size_t n, size_t m) { return mb_stride(n, m) + m; }

// the placement: the pass's inputs and outputs in LDS, every other vector where it lies in the arena block (ar) or behind the slot
struct WbInArena {
    static constexpr bool in_lds = false;
    using Map = WbMap;
    using InitMap = WbInitMap;
    __device__ __forceinline__ MbVecs vecs(float *S, const WbMap &L) const
    {
        MbVecs V{};
        V.lds = S;
        V.sh = S + L.sh; V.hp = S + L.hp; V.gp = S + L.gp;
        V.xx = S + L.xx; V.u = S + L.u; V.xy = S + L.xy; V.v = S + L.v;
        V.g = S + L.g; V.h = S + L.h;
        V.cls = reinterpret_cast<unsigned char *>(S + L.cls);
        return V;
    }
    __device__ __forceinline__ void place(MbVecs &V, float *ar, const SbSlot &sl, int n, int m) const
    {
        float *const gy = ar + 4 * n, *const gT = gy + 6 * m;        // xx u kx ku | xy xs v ky ks kv | Tx Ty Ts Sv | hx gx | rxs
        V.kx = ar + 2 * n; V.ku = ar + 3 * n;
        V.xs = gy + m; V.ky = gy + 3 * m; V.ks = gy + 4 * m; V.kv = gy + 5 * m;
        V.Tx = gT; V.Ty = gT + n; V.Ts = gT + n + m; V.Sv = gT + n + 2 * m;
        V.hx = gT + n + 3 * m; V.gx = gT + n + 4 * m;
        V.b = sl.b; V.c = sl.c;
        V.rxs = gT + 2 * n + 4 * m;
    }
    // launch entry: the four iterate vectors and the class bytes into the map (open: the caller's barrier follows)
    __device__ __forceinline__ void load(const MbVecs &V, const float *ar, const unsigned char *gcls, int n, int m, int T, int tid) const
    {
        for (int i = tid; i < n; i += T) { V.xx[i] = ar[i]; V.u[i] = ar[n + i]; }
        const float *const gy = ar + 4 * n;
        for (int i = tid; i < m; i += T) { V.xy[i] = gy[i]; V.v[i] = gy[2 * m + i]; V.cls[i] = gcls[i]; }
    }
    // a start: the staged iterate x = (x_x x_y x_s tau), y = (u v kappa) into the mutable vectors, the Kahan terms zero
    __device__ __forceinline__ void start_fill(const MbVecs &V, const float *x, const float *y, int n, int m, int T, int tid) const
    {
        for (int i = tid; i < n; i += T) {
            V.xx[i] = x[i]; V.u[i] = y[i];
            V.kx[i] = 0.0f; V.ku[i] = 0.0f;
        }
        for (int i = tid; i < m; i += T) {
            V.xy[i] = x[n + i]; V.xs[i] = x[n + m + i]; V.v[i] = y[n + i];
            V.ky[i] = 0.0f; V.ks[i] = 0.0f; V.kv[i] = 0.0f;
        }
    }
    __device__ __forceinline__ void store_mut(const MbVecs &V, float *ar, int n, int m, int T, int tid) const
    {
        for (int i = tid; i < n; i += T) { ar[i] = V.xx[i]; ar[n + i] = V.u[i]; }
        float *const gy = ar + 4 * n;
        for (int i = tid; i < m; i += T) { gy[i] = V.xy[i]; gy[2 * m + i] = V.v[i]; }
    }
    // the init-time map and the iteration's overlap: every thread is done with the one before the other is written
    __device__ __forceinline__ void sync_maps() const { __syncthreads(); }
};

// the iteration's map and the operands behind the class bytes (the same for every workgroup size): what the rule bounds and what
// fits and info report
size_t wb_lds_for(size_t n, size_t m, int, const ObPsd &psd) { return WbMap((int)n, (int)m).bytes((int)m) + psd.tail_bytes; }

// what a launch of an init-time kernel asks for: the larger of the two maps (the init-time one is the larger for m well above n)
size_t wb_lds_init(const OwnBatch *h) { return std::max(h->lds, WbInitMap((int)h->n, (int)h->m).bytes()); }

// where the PSD tail begins, in floats: what the iteration kernel is handed for SpCones
int wb_tail(const OwnBatch *h) { return (int)(WbMap((int)h->n, (int)h->m).bytes((int)h->m) / sizeof(float)); }

// the shape rules (no device needed): the single source of the limit.  Every refusal is in these words, whichever family asks (every
// PSD order to SP_MAX_ORDER is taken, so no family's own word for a PSD segment is reached)
int wb_check(size_t n, size_t m, size_t n_seg, const int32_t *seg_type, const int64_t *seg_len, std::vector<int> *cones,
             std::vector<unsigned char> *cls, ObPsd *psd)
{
    static const ObText no_words = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    if (m < 1 || m > MB_MAX_DIM) return fail(THIP_E_INVALID, "a wide batch takes 1 <= m <= 4096 rows", __FILE__, __LINE__);
    if (n < 1 || n > MB_MAX_DIM) return fail(THIP_E_INVALID, "a wide batch takes 1 <= n <= 4096 columns", __FILE__, __LINE__);
    std::vector<int> local;
    if (!cones) cones = &local;
    THIP_RC(ob_segments(no_words, m, n_seg, seg_type, seg_len, cones, cls, SP_MAX_ORDER));
    ObPsd s;
    for (size_t i = 0; i + 2 < cones->size(); i += 3)
        if ((*cones)[i + 2] >= 2) { s.n_psd += 1; s.max_k = std::max(s.max_k, (*cones)[i + 2] - 1); }
    s.tail_bytes = sp_tail_floats(s.max_k) * sizeof(float);
    if (wb_lds_for(n, m, 0, s) > OB_LDS_MAX)            // (the init-time map is at most 123 136 bytes: it always fits)
        return fail(THIP_E_INVALID, "the pass vectors of the problem (3 n + 3 m floats, the class bytes and 24 832 bytes) and the three "
                                    "operands a PSD order above 32 adds (49 920 bytes) do not fit the LDS of one CU", __FILE__, __LINE__);
    if (psd) *psd = s;
    return 0;
}

template <class ARGS>
int wb_launch_lds(const OwnBatch *h, void (*kernel)(ARGS), const ARGS &a, unsigned count, size_t lds)
{
    hipLaunchKernelGGL(kernel, dim3(count), dim3((unsigned)h->threads), lds, ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

// what the wide families add to an info record behind the SDP batch's fields: what one problem takes, the LDS of its workgroup and
// its block of the arena
template <class INFO>
void wb_info_fill(const OwnBatch *h, INFO &o)
{
    o.max_psd_order = h->psd.max_k; o.n_psd = h->psd.n_psd;
    o.psd_lds_bytes = h->psd.tail_bytes;
    o.lds_bytes_per_problem = h->lds;
    o.arena_bytes_per_problem = h->stride * sizeof(float);
}

}  // namespace
