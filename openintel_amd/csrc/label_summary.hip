// label_summary.hip -- oi_label_summary: the social_summary sums of the posts of each cluster of a labelling, per time bucket
// or per key of the documents' group attribute.
//
// The member of the summing tallies that decides a document by a LABEL.  Its siblings decide it by sim(q, d) >= t_q over a
// stream of the corpus (oi_volume.h) or by the terms it contains (mention.hip); this one reads 4 bytes of label per row, 8 of
// attributes for a labelled row when a clause needs them and 8 of signals for a row that reached a cell.  The clauses, the cell
// and the fold are the family's: oi_doc_passes, vo_bucket / vo_key (oi_volume.h), sm_add / sm_fold (oi_summary_cell.h); the
// ranked finish is the leaderboard's (cosine_groups.hip: oi_launch_groups_finish).  Every sum is an integer sum, so the
// records do not depend on the grid, the route or the order of the atomics.
//
//   ls_cells_kernel   the pass.  A workgroup walks RANGES of LS_RANGE_ROWS consecutive rows (range = its number, then + the
//                     grid), a wave a quarter of the range in BLOCKS of LS_BLOCK_ROWS rows, LS_UNROLL blocks at a time: one
//                     label per lane (a non-temporal load: the labels are read once), then the attribute words of the lanes
//                     whose label is a cluster, then the signal words of the lanes that reached a cell -- the loads of a stage
//                     are issued for all LS_UNROLL blocks before the next stage tests them.
//                     LOCAL (n_clusters * n_cells <= LS_LOCAL_CELLS): the workgroup adds into its own cells in LDS and flushes
//                     the non-zero words when its rows are done, the 64-bit sum through the thread of its low word -- with 8
//                     clusters x 24 buckets every row of the corpus aims at 192 cells, and global atomics on one address
//                     serialise across the whole device.
//                     GLOBAL (more cells): atomics go to the cells in the workspace; lanes of a wave with the same (cell, flag
//                     word) leave as one count atomic and one sum atomic for the LS_AGG most common pairs (posts of one hot
//                     ticker arrive in runs), what is left goes alone.
//   the finish        dense: groups_finish_kernel folds every cell; ranked: groups_finish_kernel makes the rank keys and
//                     groups_rank_kernel selects, sorts and writes, one workgroup per cluster.
#include "oi_summary_cell.h"
#include "oi_volume.h"

// ------------------------------------------------------------------ shape constants (tests/test_label_summary_abi.py reads them)
constexpr uint32_t LS_BLOCK_ROWS = 64;     // rows whose labels a wave reads at once, one per lane
constexpr uint32_t LS_RANGE_ROWS = 2048;   // rows per range of the pass
constexpr uint32_t LS_THREADS = 256;       // 4 waves
constexpr uint32_t LS_LOCAL_CELLS = 1024;  // up to here a workgroup keeps the call's cells in LDS: 64 KB
constexpr uint32_t LS_UNROLL = 2;          // blocks of a wave whose loads are in flight together
constexpr uint32_t LS_AGG = 4;             // (cell, flag word) pairs of a wave block that leave as one atomic each, global route
constexpr uint32_t LS_GRID_PER_CU = 4;     // workgroups per CU at the most
constexpr uint32_t LS_WAVE_ROWS = LS_RANGE_ROWS / (LS_THREADS / 64);
static_assert(LS_WAVE_ROWS % (LS_BLOCK_ROWS * LS_UNROLL) == 0 && LS_BLOCK_ROWS == 64, "a wave's share of a range is whole trips of one row per lane");
static_assert(LS_LOCAL_CELLS * SM_CELL_WORDS * 4 <= 64 * 1024, "the local cells fit the default dynamic LDS");
static_assert(LS_LOCAL_CELLS >= OI_MAX_VOLUME_BUCKETS, "a one-cluster time axis is always local");

struct LsArgs {
    const uint32_t *labels; // [n]
    const uint2 *attrs;     // {group, stamp} per local row; null when no clause reads them
    const uint2 *sig;       // the signal records
    uint32_t *cells;        // [K][n_cells][SM_CELL_WORDS], zeroed by the launcher
    uint4 filt;
    uint64_t n, n_ranges;
    uint32_t K, n_cells;
    uint32_t origin, width; // clause 2: TIME {stamp_origin, bucket_width}, KEY {key_mask, its shift}
    uint32_t has_filt;
};

// the 64-bit sum of v over the lanes of `mask`, in every lane
__device__ __forceinline__ long long ls_masked_sum(bool in_mask, int32_t v) {
    long long s = in_mask ? (long long)v : 0ll;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, OI_WAVE);
    return s;
}

// The global route's add of a block: whole waves enter.  The record sg = {pol_q30 bits, flag word} of an active lane goes into
// its cell; the lanes of the leader's (cell, flag word) pair leave as one count atomic and, when their polarities do not cancel,
// one sum atomic.
__device__ __forceinline__ void ls_global_add(uint32_t *cells, bool active, uint32_t cell, const uint2 sg) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t pair = cell * SM_CELL_WORDS + sg.y; // (cell < 2^20, sg.y < 12)
#pragma unroll
    for (uint32_t r = 0; r < LS_AGG; ++r) {
        const unsigned long long m = __ballot(active);
        if (!m) return;
        const uint32_t leader = (uint32_t)__builtin_ctzll(m);
        const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)pair, (int)leader);
        const bool same = active && pair == p0;
        const unsigned long long ms = __ballot(same);
        // (wave-uniform) a leader alone in its pair adds its own polarity: no wave sum
        const long long sum = (ms & (ms - 1ull)) == 0ull ? (long long)(int32_t)sg.x : ls_masked_sum(same, (int32_t)sg.x);
        if (lane == leader) {
            atomicAdd(cells + p0, (uint32_t)__popcll(ms));
            if (sum != 0ll)
                atomicAdd(reinterpret_cast<unsigned long long *>(cells + (size_t)(p0 / SM_CELL_WORDS) * SM_CELL_WORDS + SM_CELL_SUM),
                          (unsigned long long)sum);
        }
        active = active && !same;
    }
    if (active) sm_add(cells, cell, sg);
}

template <bool KEY_AXIS, bool LOCAL>
__global__ __launch_bounds__(LS_THREADS) void ls_cells_kernel(const LsArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t ls_local[]; // LOCAL: [K * n_cells][SM_CELL_WORDS]
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t words = a.K * a.n_cells * SM_CELL_WORDS;
    if (LOCAL) {
        for (uint32_t i = tid; i < words; i += LS_THREADS) ls_local[i] = 0u;
        __syncthreads();
    }
    const bool with_attrs = a.attrs != nullptr; // (uniform)
    for (uint64_t range = blockIdx.x; range < a.n_ranges; range += gridDim.x) {
        for (uint32_t trip = 0; trip < LS_WAVE_ROWS / (LS_BLOCK_ROWS * LS_UNROLL); ++trip) {
            const uint64_t base = range * LS_RANGE_ROWS + (uint64_t)wave * LS_WAVE_ROWS + (uint64_t)trip * (LS_BLOCK_ROWS * LS_UNROLL);
            if (base >= a.n) break; // (wave-uniform)
            uint64_t d[LS_UNROLL];
            uint32_t lab[LS_UNROLL], cell[LS_UNROLL];
            bool hit[LS_UNROLL];
            uint2 at[LS_UNROLL], sg[LS_UNROLL];
#pragma unroll
            for (uint32_t u = 0; u < LS_UNROLL; ++u) {
                d[u] = base + (uint64_t)u * LS_BLOCK_ROWS + lane;
                lab[u] = d[u] < a.n ? __builtin_nontemporal_load(a.labels + d[u]) : 0xFFFFFFFFu;
            }
#pragma unroll
            for (uint32_t u = 0; u < LS_UNROLL; ++u) {
                hit[u] = lab[u] < a.K; // (a label < K was read: d < n)
                at[u] = make_uint2(0u, 0u);
                if (hit[u] && with_attrs) at[u] = a.attrs[d[u]];
            }
#pragma unroll
            for (uint32_t u = 0; u < LS_UNROLL; ++u) {
                if (hit[u] && a.has_filt) hit[u] = oi_doc_passes(a.filt, at[u]);
                uint32_t x = 0;
                if (hit[u]) {
                    if constexpr (KEY_AXIS) hit[u] = vo_key(at[u].x, a.origin, a.width, a.n_cells, &x);
                    else hit[u] = vo_bucket(at[u].y, a.origin, a.width, a.n_cells, &x);
                }
                cell[u] = hit[u] ? lab[u] * a.n_cells + x : 0u; // (< K * n_cells <= OI_MAX_GROUP_CELLS)
                sg[u] = make_uint2(0u, 0u);
                if (hit[u]) sg[u] = a.sig[d[u]];
            }
#pragma unroll
            for (uint32_t u = 0; u < LS_UNROLL; ++u) {
                if constexpr (LOCAL) {
                    if (hit[u]) sm_add(ls_local, cell[u], sg[u]);
                } else {
                    ls_global_add(a.cells, hit[u], cell[u], sg[u]);
                }
            }
        }
    }
    if (LOCAL) {
        // the workgroup's sums leave: every non-zero count, and the 64-bit sum through the thread of its low word
        __syncthreads();
        for (uint32_t v = tid; v < words; v += LS_THREADS) {
            const uint32_t k = v % SM_CELL_WORDS;
            if (k < 12u) {
                const uint32_t x = ls_local[v];
                if (x) { atomicAdd(a.cells + v, x); ls_local[v] = 0u; }
            } else if (k == SM_CELL_SUM) {
                const unsigned long long x = *reinterpret_cast<const unsigned long long *>(ls_local + v);
                if (x) {
                    atomicAdd(reinterpret_cast<unsigned long long *>(a.cells + v), x);
                    ls_local[v] = 0u;
                    ls_local[v + 1] = 0u;
                }
            }
        }
    }
}

// ------------------------------------------------------------------ host
// Device labels [n_docs] in; dense (spec.top == 0): device records [n_clusters][n_cells] out; ranked: records and keys
// [n_clusters][top], counts and (may be null) qualified [n_clusters] out.  `filter` is the host's (by value into the launch) or
// null.  Asynchronous on the ctx stream.  The argument and state checks are api.hip's.
int oi_launch_label_summary(oi_index *idx, const uint32_t *d_labels, uint32_t K, const oi_label_summary_spec &sp, const oi_doc_filter *filter,
                            oi_social_counters *d_records, uint32_t *d_keys, uint32_t *d_counts, uint32_t *d_qualified) {
    static_assert(sizeof(oi_social_counters) == 64, "one record per cell");
    static_assert(sizeof(oi_label_summary_spec) == 32, "the spec is 32 bytes");
    oi_ctx *ctx = idx->ctx;
    hipStream_t st = ctx->stream;
    const bool key_axis = sp.axis == OI_LABEL_AXIS_KEY;
    const uint64_t n_cells = (uint64_t)K * sp.n_cells;
    // the workspace: the cells | the rank keys of a ranked call
    const size_t cb = n_cells * SM_CELL_WORDS * 4, kb = sp.top ? n_cells * sizeof(uint64_t) : 0;
    DevBuf &ws = ctx->buf("label_summary");
    OI_CHECK(ws.ensure(cb + kb));
    uint32_t *cells = ws.as<uint32_t>();
    OI_HIP_CHECK(hipMemsetAsync(cells, 0, cb, st));
    const uint64_t n = idx->n_docs;
    if (n) {
        LsArgs a;
        a.labels = d_labels;
        a.attrs = (key_axis || filter || sp.bucket_width) ? idx->doc_attrs.as<uint2>() : nullptr;
        a.sig = idx->signals.as<uint2>();
        a.cells = cells;
        a.filt = oi_filter_words(filter);
        a.n = n;
        a.n_ranges = (n + LS_RANGE_ROWS - 1) / LS_RANGE_ROWS;
        a.K = K;
        a.n_cells = sp.n_cells;
        a.origin = sp.stamp_origin;
        a.width = key_axis ? (uint32_t)__builtin_ctz(sp.stamp_origin) : sp.bucket_width;
        a.has_filt = filter ? 1u : 0u;
        const bool local = n_cells <= LS_LOCAL_CELLS;
        const size_t lds = local ? cb : 0;
        // as many workgroups per CU as their cells leave room for in its 160 KB of LDS, LS_GRID_PER_CU at the most
        const uint32_t per_cu = local ? (uint32_t)std::min<size_t>(LS_GRID_PER_CU, std::max<size_t>(1, (160 * 1024) / std::max<size_t>(lds, 1))) : LS_GRID_PER_CU;
        const dim3 grid((uint32_t)std::min<uint64_t>(a.n_ranges, (uint64_t)ctx->num_cus * per_cu));
        ProfScope ps(ctx, "label_summary");
        if (key_axis) {
            if (local) hipLaunchKernelGGL((ls_cells_kernel<true, true>), grid, dim3(LS_THREADS), lds, st, a);
            else hipLaunchKernelGGL((ls_cells_kernel<true, false>), grid, dim3(LS_THREADS), 0, st, a);
        } else {
            if (local) hipLaunchKernelGGL((ls_cells_kernel<false, true>), grid, dim3(LS_THREADS), lds, st, a);
            else hipLaunchKernelGGL((ls_cells_kernel<false, false>), grid, dim3(LS_THREADS), 0, st, a);
        }
        OI_HIP_CHECK(hipGetLastError());
    }
    return oi_launch_groups_finish(ctx, cells, n_cells, sp.n_cells, sp.top, sp.rank_by, sp.min_total, reinterpret_cast<uint64_t *>(ws.as<uint8_t>() + cb),
                                   "label_summary_rank", d_records, d_keys, d_counts, d_qualified);
}
