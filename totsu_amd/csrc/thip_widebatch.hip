// thip_widebatch.hip -- thip_widebatch: many conic programs, each with its OWN dense f32 A (shared n, m and cone layout), of EVERY shape
// up to 4096 x 4096 and every PSD order up to 64.  The eighth own-A family: the SDP batch's iteration (thip_midstream.h's bodies, the
// carried recurrence, A streamed in place by mb_pass, SpCones between the two passes) with one difference -- where each vector lives.
// The mid and SDP batches keep all 8 n + 13 m floats of an iteration in LDS, which is what limits their shapes; here only what a pass
// over A touches lies there, and every other vector is read and written IN PLACE in the problem's block of the arena, by the same
// tid-strided loops (about 25 m + 12 n floats of traffic per iteration, against 2 m n floats of A).
//
// The maps, the placement, the shape rule and the rule for the memory paths of a vector that lies in the arena are thip_wideplace.h's,
// shared with the family over a 16-bit copy of A (thip_wide16batch.hip).
//
// This file: the kernels and the family's table; the C API is thip_ownbatch.h's, instantiated by the last line.
#include "thip_wideplace.h"

using namespace thip;

namespace {

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

int wb_launch(const OwnBatch *h, bool run, const ObArgs &a, unsigned count)
{
    if (!run) return wb_launch_lds(h, widebatch_init_k, a, count, wb_lds_init(h));
    return ob_launch(h, widebatch_k, WbArgs{ a, wb_tail(h) }, count);
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
        wb_info_fill(h, o);
    }
};

}  // namespace

struct thip_widebatch : OwnBatch {};

OB_DEFINE_API(widebatch, WB_FAMILY, WbInfo)
