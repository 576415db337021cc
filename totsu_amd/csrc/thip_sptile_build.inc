// thip_sptile_build.inc -- the tiled sparse copy built ON THE DEVICE from dense column-major panels (included by thip_sptile.hip).
//
// Every builder the project mirrors (ProbLP / ProbSOCP / ProbSDP / ProbQP / ProbQCQP, MatBuild) produces a dense, column-major,
// mostly-zero array; thip_sptile_create wants CSC arrays and assembles the store single-threaded on the host.  This route makes
// the SAME object (thip_test_sptile_equal) in two passes over the panels, which may be streamed through one staging buffer, so a
// dense device copy of a mostly-zero A never has to exist:
//   pass 1 (spt_count_k): a workgroup owns a row block of 4096 rows over a run of the panel's columns; thread t holds rows
//       4 t .. 4 t + 3 of the block (one 16-byte load per column).  Per column: the non-zero count of the (column, row block) segment
//       into the count table, the column's max |a| merged across row blocks by an integer max on the bit pattern.  Per row: count and
//       max |a| stay in registers across the columns and are added to the row arrays once per workgroup.  Nothing per entry is atomic.
//   plan (host): the table (n_col x row blocks int32: 1 / 4096 of the dense bytes) comes down, the planners of thip_sptile.hip -- the
//       ones thip_sptile_create runs -- make the directory, the codes and the items, the table goes back up as the inclusive scan
//       along the columns of each tile: a segment's offset inside its tile and its length are two neighbouring words.
//   pass 2 (spt_fill_k): per segment a stream compaction in row order -- four 64-bit ballots (one per row of the lane's quad), a
//       lane-prefix popcount, the waves' totals through LDS -- writes vals[e0 + offset + rank] and, for an indexed tile, the index
//       word.  Every write is bounded by the COUNTED length of the segment: a panel whose pattern differs between the passes raises
//       a flag (finish answers THIP_E_INVALID) and never writes outside its segment.
//   finish (spt_tail_k): a tile's tail up to the next quad gets value 0 and the index of its last real entry, as build() does.
// An entry is stored iff (bits & 0x7fffffff) != 0 -- the bit pattern, not v != 0.0f: no denormal mode changes the answer.

namespace thip {

constexpr int SPB_THREADS = SPT_TB / 4;         // a thread per quad of a row block
constexpr int SPB_STAGE = 64;                   // columns whose counts / maxima a workgroup collects in LDS before it writes them out

struct SpbArgs {
    const float *panel; size_t ld;
    size_t c0; int ncols, cols_per_wg;          // the panel's first column in the matrix; a workgroup takes cols_per_wg of its columns
    size_t m, n;
    int vec;                                    // the panel allows 16-byte loads (base and ld on 16 bytes)
    int *tab;                                   // [row block][n]: counts (pass 1), inclusive scan within a tile's columns (pass 2)
    int *rowlen; unsigned *rowmax, *colmax;
    int *flags;                                 // [0]: a non-finite value (pass 1), [1]: the pattern of pass 2 is not the counted one
    // pass 2
    int ncw; const int *tile_of; const SptTile *tiles; float *vals; int *idx;
};

// rows r .. r + 3 of a column as bit patterns; a row at or past m reads as zero and is never loaded (rows m .. ld - 1 are padding)
__device__ __forceinline__ uint4 spb_load(const float *col, size_t r, size_t m, bool vec)
{
    uint4 q = make_uint4(0u, 0u, 0u, 0u);
    if (vec && r + 4 <= m) {
        const i32x4 v = __builtin_nontemporal_load(reinterpret_cast<const i32x4 *>(col + r));
        q = make_uint4((unsigned)v[0], (unsigned)v[1], (unsigned)v[2], (unsigned)v[3]);
    } else {
        if (r < m) q.x = __float_as_uint(col[r]);
        if (r + 1 < m) q.y = __float_as_uint(col[r + 1]);
        if (r + 2 < m) q.z = __float_as_uint(col[r + 2]);
        if (r + 3 < m) q.w = __float_as_uint(col[r + 3]);
    }
    return q;
}

__device__ __forceinline__ unsigned spb_wave_max(unsigned v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, d, 64));
    return v;
}

__global__ __launch_bounds__(SPB_THREADS) void spt_count_k(const SpbArgs a)
{
    __shared__ int s_cnt[SPB_STAGE];
    __shared__ unsigned s_max[SPB_STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t rb = blockIdx.x;
    const int j0 = (int)blockIdx.y * a.cols_per_wg, j1 = min(a.ncols, j0 + a.cols_per_wg);
    const size_t r = rb * SPT_TB + 4 * (size_t)tid;
    int rc[4] = { 0, 0, 0, 0 };
    unsigned rm[4] = { 0u, 0u, 0u, 0u };
    bool bad = false;
    for (int jb = j0; jb < j1; jb += SPB_STAGE) {
        const int nb = min(SPB_STAGE, j1 - jb);
        if (tid < SPB_STAGE) { s_cnt[tid] = 0; s_max[tid] = 0u; }
        __syncthreads();
        for (int kb = 0; kb < nb; kb += 4) {
            uint4 q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {       // four columns in flight (past the end: the last one again, not used)
                const int k = min(kb + u, nb - 1);
                q[u] = spb_load(a.panel + (size_t)(jb + k) * a.ld, r, a.m, a.vec != 0);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (kb + u >= nb) break;        // (uniform)
                const unsigned w[4] = { q[u].x & 0x7fffffffu, q[u].y & 0x7fffffffu, q[u].z & 0x7fffffffu, q[u].w & 0x7fffffffu };
                int c = 0;
                unsigned mx = 0u;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool nz = w[e] != 0u;
                    rc[e] += nz ? 1 : 0;
                    rm[e] = max(rm[e], w[e]);
                    mx = max(mx, w[e]);
                    c += __popcll(__ballot(nz));
                }
                bad |= mx >= 0x7f800000u;
                mx = spb_wave_max(mx);
                if (lane == 0 && c != 0) { atomicAdd(&s_cnt[kb + u], c); atomicMax(&s_max[kb + u], mx); }      // (LDS, one per wave and column)
            }
        }
        __syncthreads();
        if (tid < nb) {
            // this workgroup alone owns the (row block, column) words of the table; the column's maximum is shared with the other row blocks
            const size_t j = a.c0 + (size_t)(jb + tid);
            a.tab[rb * a.n + j] = s_cnt[tid];
            if (s_max[tid] != 0u) atomicMax(&a.colmax[j], s_max[tid]);
        }
        __syncthreads();
    }
    // the rows: once per workgroup.  Panels are serialised on the stream; where ONE workgroup takes all the panel's columns of its row
    // block a plain read-modify-write does, where the columns are split for occupancy the workgroups of a row block meet in an
    // integer add / max (order-independent; one per row and workgroup that found something there, nothing per entry)
    const bool alone = gridDim.y == 1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (r + e >= a.m || rc[e] == 0) continue;
        if (alone) { a.rowlen[r + e] += rc[e]; a.rowmax[r + e] = max(a.rowmax[r + e], rm[e]); }
        else { atomicAdd(&a.rowlen[r + e], rc[e]); atomicMax(&a.rowmax[r + e], rm[e]); }
    }
    if (bad) a.flags[0] = 1;
}

__global__ __launch_bounds__(SPB_THREADS) void spt_fill_k(const SpbArgs a)
{
    constexpr int NW = SPB_THREADS / 64;
    __shared__ int s_w[2][NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t rb = blockIdx.x;
    const int j0 = (int)blockIdx.y * a.cols_per_wg, j1 = min(a.ncols, j0 + a.cols_per_wg);
    const size_t r = rb * SPT_TB + 4 * (size_t)tid;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int *const trow = a.tab + rb * a.n;
    uint4 qn = make_uint4(0u, 0u, 0u, 0u);
    if (j0 < j1) qn = spb_load(a.panel + (size_t)j0 * a.ld, r, a.m, a.vec != 0);
    for (int j = j0; j < j1; ++j) {
        const uint4 q = qn;
        if (j + 1 < j1) qn = spb_load(a.panel + (size_t)(j + 1) * a.ld, r, a.m, a.vec != 0);     // the next column is in flight
        const size_t gj = a.c0 + (size_t)j;
        const int lc = (int)(gj & (SPT_TB - 1));
        // the counted segment: [excl, incl) of its tile, in the tile's own entry order (column, then row)
        const int incl = trow[gj], excl = lc ? trow[gj - 1] : 0, lim = incl - excl;
        const unsigned w[4] = { q.x, q.y, q.z, q.w };
        bool nz[4];
        int pre = 0, wt = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            nz[e] = (w[e] & 0x7fffffffu) != 0u;
            const unsigned long long b = __ballot(nz[e]);
            pre += __popcll(b & below);
            wt += __popcll(b);
        }
        const int par = j & 1;          // (two sets of totals: a wave may be a column ahead of another, never two -- one barrier per column)
        if (lane == 0) s_w[par][wave] = wt;
        __syncthreads();
        int woff = 0, total = 0;
#pragma unroll
        for (int k = 0; k < NW; ++k) { const int t = s_w[par][k]; total += t; if (k < wave) woff += t; }
        const int ti = a.tile_of[rb * (size_t)a.ncw + (gj >> 12)];
        if (ti >= 0) {
            const SptTile tl = a.tiles[ti];
            int rank = woff + pre;      // of the lane's first entry, in row order: the lanes below hold the rows above
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!nz[e]) continue;
                if (rank < lim) {       // never past the counted length, whatever the panel holds now
                    a.vals[tl.e0 + excl + rank] = __uint_as_float(w[e]);
                    if (!tl.dense) a.idx[tl.i0 + excl + rank] = (int)((unsigned)(4 * tid + e) | ((unsigned)lc << 16));
                }
                ++rank;
            }
        }
        if (tid == 0 && total != lim) a.flags[1] = 1;
    }
}

// the tails: entries [real, cnt) of an indexed tile (a dense tile has none)
__global__ void spt_tail_k(const SptTile *tiles, const int *real, int ntiles, float *vals, int *idx)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ntiles) return;
    const SptTile t = tiles[i];
    const int re = real[i];
    if (t.dense || re <= 0) return;
    const int last = idx[t.i0 + re - 1];
    for (int k = re; k < t.cnt; ++k) { vals[t.e0 + k] = 0.0f; idx[t.i0 + k] = last; }
}

}  // namespace thip

struct thip_sptile_builder {
    size_t m = 0, n = 0;
    thip_sptile *M = nullptr;           // the object being built; finish hands it over
    int *tab = nullptr, *rowlen = nullptr, *flags = nullptr, *tile_of = nullptr, *real = nullptr;
    unsigned *rowmax = nullptr, *colmax = nullptr;
    std::vector<char> counted, filled;
    size_t ncounted = 0, nfilled = 0;
    bool planned = false;
};

namespace {

template <class T>
int dev_zeroed(T **d, size_t count)
{
    *d = nullptr;
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    THIP_TRY(hipMalloc((void **)d, bytes));
    THIP_TRY(hipMemsetAsync(*d, 0, bytes, ctx().stream));
    return 0;
}

// the checks of a panel (both passes); marks its columns in `seen` when they pass.  Nothing is launched on an error.
int spb_take_panel(thip_sptile_builder *b, std::vector<char> &seen, size_t &nseen, size_t c0, size_t ncols, const float *panel, size_t ld)
{
    if (c0 > b->n || ncols > b->n - c0) return fail(THIP_E_INVALID, "panel outside the matrix's columns", __FILE__, __LINE__);
    if (ld < b->m) return fail(THIP_E_INVALID, "leading dimension below n_row", __FILE__, __LINE__);
    if (!panel && ncols > 0 && b->m > 0) return fail(THIP_E_INVALID, "null panel", __FILE__, __LINE__);
    for (size_t j = c0; j < c0 + ncols; ++j)
        if (seen[j]) return fail(THIP_E_INVALID, "a column given twice in one pass", __FILE__, __LINE__);
    for (size_t j = c0; j < c0 + ncols; ++j) seen[j] = 1;
    nseen += ncols;
    return 0;
}

int spb_launch(thip_sptile_builder *b, bool fill, size_t c0, size_t ncols, const float *panel, size_t ld)
{
    if (ncols == 0 || b->m == 0) return 0;
    const thip_sptile *M = b->M;
    SpbArgs a;
    a.panel = panel; a.ld = ld; a.c0 = c0; a.ncols = (int)ncols; a.m = b->m; a.n = b->n;
    a.vec = ((reinterpret_cast<uintptr_t>(panel) & 15) == 0 && (ld & 3) == 0) ? 1 : 0;
    a.tab = b->tab; a.rowlen = b->rowlen; a.rowmax = b->rowmax; a.colmax = b->colmax; a.flags = b->flags;
    a.ncw = M->ncw; a.tile_of = b->tile_of; a.tiles = M->tiles; a.vals = reinterpret_cast<float *>(M->vals); a.idx = reinterpret_cast<int *>(M->idx);
    // a row block's columns are split over enough workgroups to fill the device, at least SPB_STAGE columns each
    const size_t want = std::max<size_t>(1, 1024 / (size_t)M->nrb);
    const size_t chunks = std::max<size_t>(1, std::min(want, (ncols + SPB_STAGE - 1) / SPB_STAGE));
    a.cols_per_wg = (int)((ncols + chunks - 1) / chunks);
    const dim3 grid((unsigned)M->nrb, (unsigned)((ncols + a.cols_per_wg - 1) / a.cols_per_wg));
    if (fill) hipLaunchKernelGGL(spt_fill_k, grid, dim3(SPB_THREADS), 0, ctx().stream, a);
    else hipLaunchKernelGGL(spt_count_k, grid, dim3(SPB_THREADS), 0, ctx().stream, a);
    THIP_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" {

int thip_sptile_builder_create(size_t n_row, size_t n_col, thip_sptile_builder **out)
{
    THIP_NEED_INIT();
    if (!out) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *out = nullptr;
    thip_sptile_builder *b = new thip_sptile_builder();
    b->m = n_row; b->n = n_col;
    b->M = new thip_sptile();
    auto make = [&]() -> int {
        THIP_RC(plan_dims(b->M, n_row, n_col));
        b->counted.assign(n_col ? n_col : 1, 0); b->filled.assign(n_col ? n_col : 1, 0);
        THIP_RC(dev_zeroed(&b->tab, (size_t)b->M->nrb * n_col));
        THIP_RC(dev_zeroed(&b->rowlen, n_row));
        THIP_RC(dev_zeroed(&b->rowmax, n_row));
        THIP_RC(dev_zeroed(&b->colmax, n_col));
        THIP_RC(dev_zeroed(&b->flags, 2));
        return 0;
    };
    const int rc = make();
    if (rc != 0) { thip_sptile_builder_destroy(b); return rc; }
    *out = b;
    return 0;
}

int thip_sptile_builder_count(thip_sptile_builder *b, size_t c0, size_t ncols, const float *dev_panel, size_t ld)
{
    THIP_NEED_INIT();
    if (!b || !b->M) return fail(THIP_E_INVALID, "null or finished builder", __FILE__, __LINE__);
    if (b->planned) return fail(THIP_E_INVALID, "count after plan", __FILE__, __LINE__);
    THIP_RC(spb_take_panel(b, b->counted, b->ncounted, c0, ncols, dev_panel, ld));
    return spb_launch(b, false, c0, ncols, dev_panel, ld);
}

int thip_sptile_builder_plan(thip_sptile_builder *b, size_t *host_nnz, int *host_dense_tiles, size_t *host_indexed_entries,
                             size_t *host_bytes_per_product)
{
    THIP_NEED_INIT();
    if (!b || !b->M) return fail(THIP_E_INVALID, "null or finished builder", __FILE__, __LINE__);
    if (b->planned) return fail(THIP_E_INVALID, "planned twice", __FILE__, __LINE__);
    if (b->ncounted != b->n) return fail(THIP_E_INVALID, "plan with columns not counted", __FILE__, __LINE__);
    thip_sptile *M = b->M;
    const size_t m = b->m, n = b->n, nrb = (size_t)M->nrb, ncw = (size_t)M->ncw;
    THIP_TRY(hipStreamSynchronize(ctx().stream));
    int flags[2] = { 0, 0 };
    THIP_TRY(hipMemcpy(flags, b->flags, sizeof(flags), hipMemcpyDeviceToHost));
    if (flags[0]) return fail(THIP_E_INVALID, "non-finite stored value", __FILE__, __LINE__);
    std::vector<int> tab(nrb * n ? nrb * n : 1, 0), rowlen(m ? m : 1, 0);
    SptCounts C;
    C.cnt.assign(nrb * ncw ? nrb * ncw : 1, 0);
    C.unsorted.assign(ncw ? ncw : 1, 0);            // (a dense column's rows ascend)
    C.rowmax.assign(m ? m : 1, 0.0f); C.colmax.assign(n ? n : 1, 0.0f);
    if (nrb * n) THIP_TRY(hipMemcpy(tab.data(), b->tab, nrb * n * sizeof(int), hipMemcpyDeviceToHost));
    if (m) {
        THIP_TRY(hipMemcpy(rowlen.data(), b->rowlen, m * sizeof(int), hipMemcpyDeviceToHost));
        THIP_TRY(hipMemcpy(C.rowmax.data(), b->rowmax, m * sizeof(float), hipMemcpyDeviceToHost));     // (|a| as its bit pattern)
    }
    if (n) THIP_TRY(hipMemcpy(C.colmax.data(), b->colmax, n * sizeof(float), hipMemcpyDeviceToHost));
    C.max_row = m ? *std::max_element(rowlen.begin(), rowlen.end()) : 0;
    size_t nnz = 0;
    for (size_t j = 0; j < n; ++j) {
        int64_t col = 0;
        for (size_t rb = 0; rb < nrb; ++rb) { const int c = tab[rb * n + j]; col += c; C.cnt[rb * ncw + j / SPT_TB] += c; }
        C.max_col = std::max(C.max_col, col);
        nnz += (size_t)col;
    }
    M->nnz = nnz;
    SptPlan P;
    THIP_RC(plan_directory(M, C, P));
    plan_items(M, P);
    // the table becomes the inclusive scan along the columns of each tile; the tiles' real lengths for the tails
    for (size_t rb = 0; rb < nrb; ++rb)
        for (size_t j = 0; j < n; ++j)
            if (j % SPT_TB) tab[rb * n + j] += tab[rb * n + j - 1];
    std::vector<int> real(P.tiles.size() ? P.tiles.size() : 1, 0);
    for (size_t t = 0; t < P.tiles.size(); ++t) real[t] = (int)C.cnt[(size_t)P.tiles[t].rb * ncw + P.tiles[t].cw];
    if (nrb * n) THIP_TRY(hipMemcpy(b->tab, tab.data(), nrb * n * sizeof(int), hipMemcpyHostToDevice));
    THIP_RC(upload(P.tile_of, &b->tile_of));
    THIP_RC(upload(real, &b->real));
    // the store (sizes as build() makes them); an empty one reads as zeros
    const size_t nv = M->nnz_pad ? M->nnz_pad : 4, ni = M->nidx ? M->nidx : 4;
    THIP_TRY(hipMalloc((void **)&M->vals, nv * sizeof(float)));
    THIP_TRY(hipMalloc((void **)&M->idx, ni * sizeof(int32_t)));
    if (!M->nnz_pad) THIP_TRY(hipMemset(M->vals, 0, nv * sizeof(float)));
    if (!M->nidx) THIP_TRY(hipMemset(M->idx, 0, ni * sizeof(int32_t)));
    THIP_RC(upload_plan(M, P));
    b->planned = true;
    if (host_nnz) *host_nnz = M->nnz;
    if (host_dense_tiles) *host_dense_tiles = M->ndense;
    if (host_indexed_entries) *host_indexed_entries = M->nidx;
    if (host_bytes_per_product) *host_bytes_per_product = sptile_bytes_per_pass(M);
    return 0;
}

int thip_sptile_builder_fill(thip_sptile_builder *b, size_t c0, size_t ncols, const float *dev_panel, size_t ld)
{
    THIP_NEED_INIT();
    if (!b || !b->M) return fail(THIP_E_INVALID, "null or finished builder", __FILE__, __LINE__);
    if (!b->planned) return fail(THIP_E_INVALID, "fill before plan", __FILE__, __LINE__);
    THIP_RC(spb_take_panel(b, b->filled, b->nfilled, c0, ncols, dev_panel, ld));
    return spb_launch(b, true, c0, ncols, dev_panel, ld);
}

int thip_sptile_builder_finish(thip_sptile_builder *b, thip_sptile **out)
{
    THIP_NEED_INIT();
    if (!b || !b->M || !out) return fail(THIP_E_INVALID, "null argument or finished builder", __FILE__, __LINE__);
    *out = nullptr;
    if (!b->planned) return fail(THIP_E_INVALID, "finish before plan", __FILE__, __LINE__);
    if (b->nfilled != b->n) return fail(THIP_E_INVALID, "finish with columns not filled", __FILE__, __LINE__);
    thip_sptile *M = b->M;
    if (M->ntiles > 0) {
        hipLaunchKernelGGL(spt_tail_k, dim3((M->ntiles + 255) / 256), dim3(256), 0, ctx().stream, M->tiles, b->real, M->ntiles,
                           reinterpret_cast<float *>(M->vals), reinterpret_cast<int *>(M->idx));
        THIP_LAUNCH_CHECK();
    }
    THIP_TRY(hipStreamSynchronize(ctx().stream));
    int flags[2] = { 0, 0 };
    THIP_TRY(hipMemcpy(flags, b->flags, sizeof(flags), hipMemcpyDeviceToHost));
    if (flags[1]) return fail(THIP_E_INVALID, "the panels of the fill pass do not have the counted non-zero pattern", __FILE__, __LINE__);
    *out = M;
    b->M = nullptr;
    return 0;
}

int thip_sptile_builder_destroy(thip_sptile_builder *b)
{
    if (!b) return 0;
    if (ctx().inited) (void)hipStreamSynchronize(ctx().stream);
    for (void *p : { (void *)b->tab, (void *)b->rowlen, (void *)b->flags, (void *)b->tile_of, (void *)b->real, (void *)b->rowmax, (void *)b->colmax })
        if (p) (void)hipFree(p);
    if (b->M) thip_sptile_destroy(b->M);
    delete b;
    return 0;
}

int thip_sptile_from_dense(size_t n_row, size_t n_col, const float *dev_mat, size_t ld, thip_sptile **out)
{
    THIP_NEED_INIT();
    if (!out) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    *out = nullptr;
    thip_sptile_builder *b = nullptr;
    THIP_RC(thip_sptile_builder_create(n_row, n_col, &b));
    int rc = thip_sptile_builder_count(b, 0, n_col, dev_mat, ld);
    if (rc == 0) rc = thip_sptile_builder_plan(b, nullptr, nullptr, nullptr, nullptr);
    if (rc == 0) rc = thip_sptile_builder_fill(b, 0, n_col, dev_mat, ld);
    if (rc == 0) rc = thip_sptile_builder_finish(b, out);
    thip_sptile_builder_destroy(b);
    return rc;
}

// TEST HOOK: both objects downloaded and compared part by part (include/totsu_f32hip_test.h gives the order)
int thip_test_sptile_equal(const thip_sptile *A, const thip_sptile *B, int *host_first_difference)
{
    THIP_NEED_INIT();
    if (!A || !B || !host_first_difference) return fail(THIP_E_INVALID, "null argument", __FILE__, __LINE__);
    THIP_TRY(hipStreamSynchronize(ctx().stream));
    int part = 0, rc = 0;
    auto differ = [&](const void *da, const void *db, size_t bytes) -> bool {
        if (bytes == 0 || rc != 0) return false;
        std::vector<unsigned char> ha(bytes), hb(bytes);
        hipError_t e = hipMemcpy(ha.data(), da, bytes, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(hb.data(), db, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { rc = fail((int)e, "hipMemcpy", __FILE__, __LINE__); return false; }
        return std::memcmp(ha.data(), hb.data(), bytes) != 0;
    };
    static_assert(sizeof(SptTile) == 32 && sizeof(SptItem) == 32, "records without padding: compared as bytes");
    const size_t rexp_b = (size_t)A->nrb * SPT_TB, cexp_b = (size_t)A->ncw * SPT_TB;
    if (A->m != B->m || A->n != B->n || A->nnz != B->nnz) part = 1;
    else if (A->nnz_pad != B->nnz_pad || A->nidx != B->nidx || A->ndense != B->ndense || A->max_visit != B->max_visit) part = 2;
    else if (A->headN != B->headN || A->headT != B->headT) part = 3;
    else if (A->slN != B->slN || A->slT != B->slT || A->nN != B->nN || A->nT != B->nT) part = 4;
    else if (A->ntiles != B->ntiles || differ(A->tiles, B->tiles, (size_t)A->ntiles * sizeof(SptTile))) part = 5;
    else if (differ(A->order, B->order, (size_t)A->ntiles * sizeof(int))) part = 6;
    else if (differ(A->itemsN, B->itemsN, (size_t)A->nN * sizeof(SptItem)) || differ(A->itemsT, B->itemsT, (size_t)A->nT * sizeof(SptItem))) part = 7;
    else if (differ(A->rexp, B->rexp, rexp_b) || differ(A->cexp, B->cexp, cexp_b)) part = 8;
    else if (differ(A->idx, B->idx, A->nidx * sizeof(int32_t))) part = 9;
    else if (differ(A->vals, B->vals, A->nnz_pad * sizeof(float))) part = 10;
    if (rc != 0) return rc;
    *host_first_difference = part;
    return 0;
}

}  // extern "C"
