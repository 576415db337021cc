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

// thip_NAME_set_iterates of a handle that launches by class: every length is the problem's own.  One upload -- where each
// workgroup's iterate lies (in floats from the first one), the classes' lists side by side, the iterates -- and one launch per class
// with a member in the range
template <class H>
int rg_set_iterates(const ObFamily &f, H *h, int first, int count, const float *host_x, const float *host_y)
{
    THIP_NEED_INIT();
    THIP_RC(ob_start_range(f, h, first, count, host_x, host_y));
    const size_t cnt = (size_t)count, head = cnt * sizeof(long long) + ((cnt + 1) & ~(size_t)1) * sizeof(int);
    std::vector<long long> at_p(cnt);
    std::vector<int> members[2];
    size_t floats = 0;
    {
        const float *x = host_x, *y = host_y;
        for (size_t k = 0; k < cnt; ++k) {
            const auto &q = h->pl.prob[(size_t)first + k];
            THIP_RC(ob_start_scalars(x, y, q.n, q.m));
            at_p[k] = (long long)floats;
            members[q.cls].push_back(first + (int)k);
            floats += 2 * q.n + 3 * q.m + 2;
            x += q.n + 2 * q.m + 1; y += q.n + q.m + 1;
        }
    }
    const size_t bytes = head + floats * sizeof(float);
    void *pinned = nullptr;
    THIP_RC(ob_stage_reserve(h, bytes, &pinned));
    unsigned char *const host = static_cast<unsigned char *>(pinned);
    long long *const at = reinterpret_cast<long long *>(host);
    int *const list = reinterpret_cast<int *>(host + cnt * sizeof(long long));
    float *const it = reinterpret_cast<float *>(host + head);
    {
        const float *x = host_x, *y = host_y;
        for (size_t k = 0; k < cnt; ++k) {
            const auto &q = h->pl.prob[(size_t)first + k];
            const size_t nx = q.n + 2 * q.m + 1, ny = q.n + q.m + 1;
            memcpy(it + at_p[k], x, nx * sizeof(float));
            memcpy(it + at_p[k] + nx, y, ny * sizeof(float));
            x += nx; y += ny;
        }
        size_t k = 0;
        for (int c = 0; c < 2; ++c)
            for (int p : members[c]) { list[k] = p; at[k] = at_p[(size_t)(p - first)]; ++k; }
    }
    return ob_start_staged(h, first, count, bytes, [&](const void *stage) {
        const unsigned char *const dev = static_cast<const unsigned char *>(stage);
        size_t k = 0;
        for (int c = 0; c < 2; ++c) {
            if (members[c].empty()) continue;
            const ObStart s{ reinterpret_cast<const float *>(dev + head), reinterpret_cast<const long long *>(dev) + k, 0 };
            THIP_RC(rg_start(h, c, (unsigned)members[c].size(), reinterpret_cast<const int *>(dev + cnt * sizeof(long long)) + k, s));
            k += members[c].size();
        }
        return 0;
    });
}

// thip_NAME_set_bc of a handle that launches by class: every length is the problem's own.  One upload -- where each workgroup's
// data lies (in floats from the first part), the classes' lists side by side, the parts -- and one launch per class with a member
// in the range.  The handle's store is packed by problem, 2 m_p + n_p floats each
template <class H>
int rg_set_bc(const ObFamily &f, H *h, int first, int count, const float *host_b, const float *host_c, const float *host_r,
              const uint8_t *host_has, int keep)
{
    THIP_NEED_INIT();
    THIP_RC(ob_setbc_range(f, h, first, count, host_b, host_c));
    const size_t cnt = (size_t)count, head = cnt * sizeof(long long) + ((cnt + 1) & ~(size_t)1) * sizeof(int);
    std::vector<long long> at_p(cnt);
    std::vector<int> members[2];
    size_t floats = 0;
    for (size_t k = 0; k < cnt; ++k) {
        const auto &q = h->pl.prob[(size_t)first + k];
        at_p[k] = (long long)floats;
        members[q.cls].push_back(first + (int)k);
        floats += 1 + 2 * q.m + q.n;
    }
    if (!h->bc_store) {
        std::vector<long long> store_at(h->n_prob);
        size_t total = 0;
        for (size_t p = 0; p < h->n_prob; ++p) { store_at[p] = (long long)total; total += 2 * h->pl.prob[p].m + h->pl.prob[p].n; }
        THIP_RC(ob_setbc_store(h, total, &store_at));
    }
    const size_t bytes = head + floats * sizeof(float);
    void *pinned = nullptr;
    THIP_RC(ob_stage_reserve(h, bytes, &pinned));
    unsigned char *const host = static_cast<unsigned char *>(pinned);
    long long *const at = reinterpret_cast<long long *>(host);
    int *const list = reinterpret_cast<int *>(host + cnt * sizeof(long long));
    float *const parts = reinterpret_cast<float *>(host + head);
    {
        const float *b = host_b, *c = host_c, *r = host_r;
        for (size_t k = 0; k < cnt; ++k) {
            const auto &q = h->pl.prob[(size_t)first + k];
            const bool has = host_r && (!host_has || host_has[k]);
            ob_setbc_pack(parts + at_p[k], q.n, q.m, b, c, has ? r : nullptr);
            b += q.m; c += q.n;
            if (r) r += q.m;
        }
        size_t k = 0;
        for (int c2 = 0; c2 < 2; ++c2)
            for (int p : members[c2]) { list[k] = p; at[k] = at_p[(size_t)(p - first)]; ++k; }
    }
    return ob_start_staged(h, first, count, bytes, [&](const void *stage) {
        const unsigned char *const dev = static_cast<const unsigned char *>(stage);
        size_t k = 0;
        for (int c = 0; c < 2; ++c) {
            if (members[c].empty()) continue;
            const ObSetBc s{ ObStart{ reinterpret_cast<const float *>(dev + head), reinterpret_cast<const long long *>(dev) + k, 0 },
                             h->bc_store, h->bc_at_dev, 0, keep != 0 };
            THIP_RC(rg_setbc(h, c, (unsigned)members[c].size(), reinterpret_cast<const int *>(dev + cnt * sizeof(long long)) + k, s));
            k += members[c].size();
        }
        return 0;
    });
}

// the classes' members among the problems first .. first + count - 1
template <class H>
void rg_members(const H *h, int first, int count, std::vector<int> *members)
{
    for (int k = 0; k < count; ++k) members[h->pl.prob[(size_t)(first + k)].cls].push_back(first + k);
}

// thip_NAME_set_a of a DENSE handle that launches by class: problem p's m_p n_p values go from the host straight behind the slot's
// pointer (ob_seta_copy), the classes' lists into live_dev as a run's do -- nothing is allocated -- and one launch per class with a
// member in the range runs rg_seta
template <class H>
int rg_set_a_dense(const ObFamily &f, H *h, int first, int count, const float *host_values, const int64_t *host_counts, int keep)
{
    THIP_NEED_INIT();
    auto need = [&](int p) { return h->pl.prob[(size_t)p].m * h->pl.prob[(size_t)p].n; };
    size_t total = 0;
    THIP_RC(ob_seta_check(f, h, first, count, host_values, host_counts, need, OB_SETA_DENSE, &total));
    std::vector<int> members[2], list;                          // (list: read by its copy until ob_restarted synchronises)
    rg_members(h, first, count, members);
    for (int c = 0; c < 2; ++c) list.insert(list.end(), members[c].begin(), members[c].end());
    hipStream_t st = ctx().stream;
    auto go = [&]() -> int {
        THIP_RC(ob_seta_copy(h, first, count, host_values, need));
        THIP_TRY(hipMemcpyAsync(h->live_dev, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, st));
        size_t k = 0;
        for (int c = 0; c < 2; ++c) {
            if (members[c].empty()) continue;
            THIP_RC(rg_seta(h, c, (unsigned)members[c].size(), h->live_dev + k, ObSetA{ ObStart{ nullptr, nullptr, 0 }, keep != 0 }));
            k += members[c].size();
        }
        return 0;
    };
    const int rc = go();
    if (rc != 0) { hipStreamSynchronize(st); return rc; }
    return ob_restarted(h, first, count);
}

// thip_NAME_set_a of a SPARSE handle that launches by class: the values in the CSC order of each slot's present pattern, need(p) of
// them.  One upload into the staging buffers -- where each workgroup's values lie (in floats from the first), the classes' lists side
// by side, the values -- and per class with a member in the range rg_seta, which scatters them into the blobs first
template <class H, class NEED>
int rg_set_a_sparse(const ObFamily &f, H *h, int first, int count, const float *host_values, const int64_t *host_counts, int keep,
                    const NEED &need)
{
    THIP_NEED_INIT();
    size_t total = 0;
    THIP_RC(ob_seta_check(f, h, first, count, host_values, host_counts, need, OB_SETA_SPARSE, &total));
    const size_t cnt = (size_t)count, head = cnt * sizeof(long long) + ((cnt + 1) & ~(size_t)1) * sizeof(int);
    std::vector<long long> at_p(cnt);
    std::vector<int> members[2];
    rg_members(h, first, count, members);
    size_t o = 0;
    for (size_t k = 0; k < cnt; ++k) { at_p[k] = (long long)o; o += need(first + (int)k); }
    const size_t bytes = head + total * sizeof(float);
    void *pinned = nullptr;
    THIP_RC(ob_stage_reserve(h, bytes, &pinned));
    unsigned char *const host = static_cast<unsigned char *>(pinned);
    long long *const at = reinterpret_cast<long long *>(host);
    int *const list = reinterpret_cast<int *>(host + cnt * sizeof(long long));
    if (total) memcpy(host + head, host_values, total * sizeof(float));
    {
        size_t k = 0;
        for (int c = 0; c < 2; ++c)
            for (int p : members[c]) { list[k] = p; at[k] = at_p[(size_t)(p - first)]; ++k; }
    }
    return ob_start_staged(h, first, count, bytes, [&](const void *stage) {
        const unsigned char *const dev = static_cast<const unsigned char *>(stage);
        size_t k = 0;
        for (int c = 0; c < 2; ++c) {
            if (members[c].empty()) continue;
            const ObSetA s{ ObStart{ reinterpret_cast<const float *>(dev + head), reinterpret_cast<const long long *>(dev) + k, 0 },
                            keep != 0 };
            THIP_RC(rg_seta(h, c, (unsigned)members[c].size(), reinterpret_cast<const int *>(dev + cnt * sizeof(long long)) + k, s));
            k += members[c].size();
        }
        return 0;
    });
}

// ---- the round calls on device memory (thip_ownbatch.h) of a handle that launches by class -----------------------------------------

// the head of a range's staged layout, as the host calls above build it: where each workgroup's part lies, then the classes' lists
size_t rg_head_bytes(size_t cnt) { return cnt * sizeof(long long) + ((cnt + 1) & ~(size_t)1) * sizeof(int); }

// that head into pinned memory (at_p[k]: where problem first + k's part begins), and the classes' members of the range
template <class H>
void rg_head_fill(const H *h, int first, int count, const std::vector<long long> &at_p, unsigned char *pin, std::vector<int> *members)
{
    long long *const at = reinterpret_cast<long long *>(pin);
    int *const list = reinterpret_cast<int *>(pin + (size_t)count * sizeof(long long));
    members[0].clear(); members[1].clear();
    rg_members(h, first, count, members);
    size_t k = 0;
    for (int c = 0; c < 2; ++c)
        for (int p : members[c]) { list[k] = p; at[k] = at_p[(size_t)(p - first)]; ++k; }
}

// fn(c, the class's count, its list, its places) for each class with a member in the range, from the head on the device
template <class FN>
int rg_by_class(const std::vector<int> *members, size_t cnt, const unsigned char *dev_head, const FN &fn)
{
    size_t k = 0;
    for (int c = 0; c < 2; ++c) {
        if (members[c].empty()) continue;
        THIP_RC(fn(c, (unsigned)members[c].size(), reinterpret_cast<const int *>(dev_head + cnt * sizeof(long long)) + k,
                   reinterpret_cast<const long long *>(dev_head) + k));
        k += members[c].size();
    }
    return 0;
}

template <class H>
int rg_set_iterates_dev(const ObFamily &f, H *h, int first, int count, const float *dev_x, const float *dev_y)
{
    std::vector<int> members[2];
    const size_t cnt = count > 0 ? (size_t)count : 0;
    return ob_set_iterates_dev_t(f, h, first, count, dev_x, dev_y,
                                 [&](int p, size_t *n, size_t *m) { *n = h->pl.prob[(size_t)p].n; *m = h->pl.prob[(size_t)p].m; },
                                 rg_head_bytes(cnt),
                                 [&](unsigned char *pin, const std::vector<long long> &at_p) { rg_head_fill(h, first, count, at_p, pin, members); },
                                 [&](const unsigned char *dev_head, const float *staged) {
                                     return rg_by_class(members, cnt, dev_head, [&](int c, unsigned n_c, const int *list, const long long *at) {
                                         return rg_start(h, c, n_c, list, ObStart{ staged, at, 0 });
                                     });
                                 });
}

template <class H>
int rg_set_bc_dev(const ObFamily &f, H *h, int first, int count, const float *dev_b, const float *dev_c, const float *dev_r,
                  const uint8_t *host_has, int keep)
{
    std::vector<int> members[2];
    const size_t cnt = count > 0 ? (size_t)count : 0;
    return ob_set_bc_dev_t(f, h, first, count, dev_b, dev_c, dev_r, host_has,
                           [&](int p, size_t *n, size_t *m) { *n = h->pl.prob[(size_t)p].n; *m = h->pl.prob[(size_t)p].m; },
                           [&]() -> int {
                               if (h->bc_store) return 0;
                               std::vector<long long> store_at(h->n_prob);
                               size_t total = 0;
                               for (size_t p = 0; p < h->n_prob; ++p) { store_at[p] = (long long)total; total += 2 * h->pl.prob[p].m + h->pl.prob[p].n; }
                               return ob_setbc_store(h, total, &store_at);
                           },
                           rg_head_bytes(cnt),
                           [&](unsigned char *pin, const std::vector<long long> &at_p) { rg_head_fill(h, first, count, at_p, pin, members); },
                           [&](const unsigned char *dev_head, const float *staged) {
                               return rg_by_class(members, cnt, dev_head, [&](int c, unsigned n_c, const int *list, const long long *at) {
                                   return rg_setbc(h, c, n_c, list, ObSetBc{ ObStart{ staged, at, 0 }, h->bc_store, h->bc_at_dev, 0, keep != 0 });
                               });
                           });
}

// (dense: the classes' lists go into live_dev as a run's do, and the host twin's)
template <class H>
int rg_set_a_dev_dense(const ObFamily &f, H *h, int first, int count, const float *dev_values, int keep)
{
    std::vector<int> members[2], list;                          // (list: read by its copy until ob_restarted synchronises)
    return ob_set_a_dev_dense_t(f, h, first, count, dev_values,
                                [&](int p) { return h->pl.prob[(size_t)p].m * h->pl.prob[(size_t)p].n; }, [&]() -> int {
        rg_members(h, first, count, members);
        for (int c = 0; c < 2; ++c) list.insert(list.end(), members[c].begin(), members[c].end());
        THIP_TRY(hipMemcpyAsync(h->live_dev, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, ctx().stream));
        h->last_h2d += list.size() * sizeof(int);
        size_t k = 0;
        for (int c = 0; c < 2; ++c) {
            if (members[c].empty()) continue;
            THIP_RC(rg_seta(h, c, (unsigned)members[c].size(), h->live_dev + k, ObSetA{ ObStart{ nullptr, nullptr, 0 }, keep != 0 }));
            k += members[c].size();
        }
        return 0;
    });
}

template <class H, class NEED>
int rg_set_a_dev_sparse(const ObFamily &f, H *h, int first, int count, const float *dev_values, int keep, const NEED &need)
{
    std::vector<int> members[2];
    const size_t cnt = count > 0 ? (size_t)count : 0;
    return ob_set_a_dev_sparse_t(f, h, first, count, dev_values, need, rg_head_bytes(cnt),
                                 [&](unsigned char *pin, const std::vector<long long> &at_p) { rg_head_fill(h, first, count, at_p, pin, members); },
                                 [&](const unsigned char *dev_head) {
                                     return rg_by_class(members, cnt, dev_head, [&](int c, unsigned n_c, const int *list, const long long *at) {
                                         return rg_seta(h, c, n_c, list, ObSetA{ ObStart{ dev_values, at, 0 }, keep != 0 });
                                     });
                                 });
}

template <class H>
int rg_solutions_dev(const ObFamily &f, H *h, int first, int count, float *dev_x, float *dev_y, int32_t *dev_state)
{
    return ob_solutions_dev_t(f, h, first, count, dev_x, dev_y, dev_state, true,
                              [&](int p, size_t *n, size_t *m) { *n = h->pl.prob[(size_t)p].n; *m = h->pl.prob[(size_t)p].m; },
                              [&](int p) { return (long long)h->pl.desc[(size_t)p].arena_at; });
}

// thip_NAME_solutions of a handle of many shapes: the gather kernel by a table of the range's blocks, shapes and places
template <class H>
int rg_solutions(const ObFamily &f, H *h, int first, int count, float *host_x, float *host_y, thip_status *host_status)
{
    return ob_solutions_t(f, h, first, count, host_x, host_y, host_status, true,
                          [&](int p, size_t *n, size_t *m) { *n = h->pl.prob[(size_t)p].n; *m = h->pl.prob[(size_t)p].m; },
                          [&](int p) { return (long long)h->pl.desc[(size_t)p].arena_at; });
}

}  // namespace
