// thip_widebatch.hip -- thip_widebatch: many conic programs, each with its OWN dense f32 A (shared n, m and cone layout), of EVERY shape
// up to 4096 x 4096 and every PSD order up to 64.  The eighth own-A family: the SDP batch's iteration (thip_midstream.h's bodies, the
// carried recurrence, A streamed in place by mb_pass, SpCones between the two passes) with one difference -- where each vector lives.
// The mid and SDP batches keep all 8 n + 13 m floats of an iteration in LDS, which is what limits their shapes; here only what a pass
// over A touches lies there, and every other vector is read and written IN PLACE in the problem's block of the arena, by the same
// tid-strided loops (about 25 m + 12 n floats of traffic per iteration, against 2 m n floats of A).
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
//
// This file: the two maps, the placement, the kernels and the family's table; the C API is thip_ownbatch.h's, instantiated by the
// last line.
#include "thip_sdpcones.h"

using namespace thip;

namespace {

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

struct WbArgs { ObArgs mb; int tail; };

__global__ __launch_bounds__(1024) void widebatch_init_k(const ObArgs a) { mb_init_body(a, ObUniform(), MbDenseA(), WbInArena()); }

__global__ __launch_bounds__(1024) void widebatch_k(const WbArgs a)
{
    mb_iterate_body(a.mb, SpCones{ a.tail }, ObUniform(), MbDenseA(), WbInArena());
}

// a problem starts from a given iterate (thip_widebatch_set_iterates)
struct WbStartArgs { ObArgs mb; ObStart s; };

__global__ __launch_bounds__(1024) void widebatch_start_k(const WbStartArgs a)
{
    mb_start_body(a.mb, ob_staged(a.s), ObUniform(), MbDenseA(), WbInArena());
}

// a problem takes a new (b, c) and keeps its A (thip_widebatch_set_bc)
struct WbSetBcArgs { ObArgs mb; ObSetBc s; };

__global__ __launch_bounds__(1024) void widebatch_setbc_k(const WbSetBcArgs a)
{
    mb_setbc_body(a.mb, a.s, ObUniform(), MbDenseA(), WbInArena());
}

// a problem's A has new values (thip_widebatch_set_a)
struct WbSetAArgs { ObArgs mb; int keep; };

__global__ __launch_bounds__(1024) void widebatch_seta_k(const WbSetAArgs a)
{
    mb_seta_body(a.mb, a.keep, ObUniform(), MbDenseA(), WbInArena());
}

const ObText WB_TEXT = { "wide batch not initialised", "null wide batch", "a wide batch holds 1 .. 1048576 problems", nullptr,
                         "the workgroup size is 256 or 1024 (0: by shape)",
                         "thip_test_widebatch_force_threads comes before thip_widebatch_init" };

// the iteration's map and the operands behind the class bytes (the same for every workgroup size): what the rule bounds and what
// fits and info report
size_t wb_lds_for(size_t n, size_t m, int, const ObPsd &psd) { return WbMap((int)n, (int)m).bytes((int)m) + psd.tail_bytes; }

// what a launch of an init-time kernel asks for: the larger of the two maps (the init-time one is the larger for m well above n)
size_t wb_lds_init(const OwnBatch *h) { return std::max(h->lds, WbInitMap((int)h->n, (int)h->m).bytes()); }

// the shape rules (no device needed): the single source of the limit
int wb_check(size_t n, size_t m, size_t n_seg, const int32_t *seg_type, const int64_t *seg_len, std::vector<int> *cones,
             std::vector<unsigned char> *cls, ObPsd *psd)
{
    if (m < 1 || m > MB_MAX_DIM) return fail(THIP_E_INVALID, "a wide batch takes 1 <= m <= 4096 rows", __FILE__, __LINE__);
    if (n < 1 || n > MB_MAX_DIM) return fail(THIP_E_INVALID, "a wide batch takes 1 <= n <= 4096 columns", __FILE__, __LINE__);
    std::vector<int> local;
    if (!cones) cones = &local;
    THIP_RC(ob_segments(WB_TEXT, m, n_seg, seg_type, seg_len, cones, cls, SP_MAX_ORDER));
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

int wb_launch(const OwnBatch *h, bool run, const ObArgs &a, unsigned count)
{
    if (!run) return wb_launch_lds(h, widebatch_init_k, a, count, wb_lds_init(h));
    return ob_launch(h, widebatch_k, WbArgs{ a, (int)(WbMap((int)h->n, (int)h->m).bytes((int)h->m) / sizeof(float)) }, count);
}

int wb_start(const OwnBatch *h, const ObArgs &a, const ObStart &s, unsigned count)
{
    return ob_launch(h, widebatch_start_k, WbStartArgs{ a, s }, count);
}

int wb_setbc(const OwnBatch *h, const ObArgs &a, const ObSetBc &s, unsigned count)
{
    return wb_launch_lds(h, widebatch_setbc_k, WbSetBcArgs{ a, s }, count, wb_lds_init(h));
}

int wb_seta(const OwnBatch *h, const ObArgs &a, const ObSetA &s, unsigned count)
{
    return wb_launch_lds(h, widebatch_seta_k, WbSetAArgs{ a, s.keep }, count, wb_lds_init(h));
}

ObFamily WB_FAMILY = { WB_TEXT, { 256, 1024, 0 }, true, wb_check, mb_threads_for, wb_lds_for, wb_stride, wb_launch, wb_start, wb_setbc,
                       wb_seta,
                       { (const void *)widebatch_k, (const void *)widebatch_init_k, (const void *)widebatch_start_k,
                         (const void *)widebatch_setbc_k, (const void *)widebatch_seta_k, nullptr } };

// thip_sdpbatch_info_t's fields, and what one problem takes: the LDS of its workgroup and its block of the arena
struct WbInfo {
    void operator()(const OwnBatch *h, thip_widebatch_info_t &o) const
    {
        MbInfo()(h, o);
        o.max_psd_order = h->psd.max_k; o.n_psd = h->psd.n_psd;
        o.psd_lds_bytes = h->psd.tail_bytes;
        o.lds_bytes_per_problem = h->lds;
        o.arena_bytes_per_problem = h->stride * sizeof(float);
    }
};

}  // namespace

struct thip_widebatch : OwnBatch {};

OB_DEFINE_API(widebatch, WB_FAMILY, WbInfo)
