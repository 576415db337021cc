// thip_raggedhost.h -- what the two batches whose problems each have their own shape share (thip_raggedbatch.hip: dense A;
// thip_raggedsparse.hip: sparse A): the locator seam's other side (RbAt: the problem and its arena block as read from its
// descriptor) and the host side of a handle that launches by workgroup-size class -- one launch per class that has a running
// problem, the classes' live lists side by side in live_dev, the classes' counters, init, run and run_until_any.  The handle H is an
// OwnBatch with `pl` (a plan with members[2]: the classes' members in the order of their live lists), cl_live[2], cl_launches[2],
// cl_workgroups[2]; its translation unit gives rg_launch(const H *, run, class, count, steps, live, first), the class's kernel.
// Included once by each of the two translation units (on top of thip_sdpcones.h): everything here is internal to the one that
// includes it.
#pragma once

#include "thip_sdpcones.h"

#include <string>

namespace {

// the seam's other side (ObUniform, thip_ownbatch.h): the problem and its block as read from the descriptor
struct RbAt {
    int p; float *ar;
    __device__ __forceinline__ int problem(const ObArgs &) const { return p; }
    __device__ __forceinline__ float *block(const ObArgs &, int) const { return ar; }
    __device__ __forceinline__ int carried(const ObArgs &, int n, int m) const { return n + m; }      // mb_stride - (5 n + 9 m)
};

constexpr int RB_THREADS[2] = { 256, 1024 };

// a refusal of problem p: the rule's own words behind the index
int rb_refuse(size_t p, int rc, int *first_refused)
{
    if (first_refused) *first_refused = (int)p;
    const std::string why = thip_last_error();
    const std::string msg = "problem " + std::to_string(p) + ": " + why;
    return fail(rc, msg.c_str(), __FILE__, __LINE__);
}

// where class c's list lies in live_dev
template <class H>
size_t rg_list_at(const H *h, int c) { return c == 0 ? 0 : h->pl.members[0].size(); }

// one launch per class with a member in lists[c] (which the launches read until the next synchronisation)
template <class H>
int rg_launch_lists(H *h, bool run, int steps, const std::vector<int> *lists)
{
    hipStream_t st = ctx().stream;
    for (int c = 0; c < 2; ++c) {
        const std::vector<int> &l = lists[c];
        if (l.empty()) continue;
        int *dev = h->live_dev + rg_list_at(h, c);
        THIP_TRY(hipMemcpyAsync(dev, l.data(), l.size() * sizeof(int), hipMemcpyHostToDevice, st));
        THIP_RC(rg_launch(h, run, c, (unsigned)l.size(), steps, dev, 0));
        if (run) {
            h->cl_launches[c] += 1; h->cl_workgroups[c] += (int64_t)l.size();
            h->launches += 1; h->workgroups += (int64_t)l.size();
        }
    }
    return 0;
}

template <class H>
int rg_init(const ObText &tx, H *h)
{
    THIP_NEED_INIT();
    if (!h) return fail(THIP_E_INVALID, tx.null_h, __FILE__, __LINE__);
    THIP_RC(rg_launch_lists(h, false, 0, h->pl.members));
    h->launches = h->workgroups = 0;
    for (int c = 0; c < 2; ++c) { h->cl_launches[c] = h->cl_workgroups[c] = 0; h->cl_live[c].clear(); }
    h->inited = true;
    return ob_poll(h, nullptr);
}

template <class H>
int rg_run(const ObText &tx, H *h, int64_t max_steps, int64_t poll_every, thip_status *host_status, bool until_any)
{
    THIP_NEED_INIT();
    if (!h || !h->inited) return fail(THIP_E_INVALID, tx.uninit, __FILE__, __LINE__);
    if (poll_every <= 0) poll_every = 16;
    THIP_RC(ob_poll(h, host_status));
    const size_t live0 = h->live.size();
    int64_t done = 0;
    while (!h->live.empty() && (max_steps < 0 || done < max_steps) && !(until_any && h->live.size() < live0)) {
        int64_t batch = poll_every;
        if (max_steps >= 0 && done + batch > max_steps) batch = max_steps - done;
        if (batch > 1 << 20) batch = 1 << 20;
        for (int c = 0; c < 2; ++c) {       // the running members, in the class's order (its members are not contiguous in p)
            h->cl_live[c].clear();
            for (int p : h->pl.members[c])
                if (h->hst[p].state == THIP_ST_RUNNING) h->cl_live[c].push_back(p);
        }
        THIP_RC(rg_launch_lists(h, true, (int)batch, h->cl_live));
        done += batch;
        THIP_RC(ob_poll(h, host_status));       // (synchronises: the lists the launches read are the host's to rewrite)
    }
    return 0;
}

}  // namespace
