// label_exemplars.hip -- oi_label_exemplars: the stored posts closest to the centroid of their own cluster.
// The definition is the header's; what follows is how it runs.  A call is  score, then (hist, scan) per radix pass, then
// collect and sort: no host synchronise between them, and nothing whose cost is n_clusters x n_docs.
//
//   le_score_kernel    the stream of the MEMBER rows.  A workgroup walks RANGES of LE_RANGE_ROWS consecutive rows (range = its
//                      number, then + the grid), a wave a quarter of the range in BLOCKS of LE_BLOCK_ROWS rows: one label per
//                      lane, and the attribute word only under a filter.  The members of a block (label < n_clusters, filter
//                      passed) are taken LE_UNROLL at a time off the ballot, so a non-member never reaches an address; their
//                      row loads are issued together (NV float4 per lane and row, as vo_exact_kernel holds a row), the centroid
//                      of each row's label comes through L2 with ordinary loads.  The f32 value is the family's: vo_load_row4,
//                      vo_chain4 in ascending j, oi_wave_sum.  The sim goes back to the row's lane, which stores ONE word per
//                      row: keys[d] = oi_f32_key(sim), or LE_NO_KEY = 0 for a row that is no member or whose sim is NaN
//                      (oi_f32_key never returns 0 for a number: 0 would be the key of a NaN with every bit set).
//   le_hist_kernel     one pass of a SEGMENTED radix select, all clusters at once.  The order of a cluster's members is that of
//                      the composite word  comp = key << RB | (~row & (2^RB - 1)),  RB = the bits of n_docs - 1 rounded up to
//                      whole digits: comp descending IS oi_rank_key descending (one doc_id_base for all rows).  A pass reads the
//                      4-byte key and the 4-byte label of every row and adds the digit of the rows whose comp still agrees with
//                      their cluster's prefix to hist[label][digit]; equal (label, digit) pairs of a wave leave as one atomic,
//                      and with at most LE_LOCAL_CLUSTERS clusters a workgroup adds in LDS first.
//   le_scan_kernel     one workgroup, a wave per cluster: the digit that holds the cluster's kk-th member from the top; the
//                      prefix takes it, kk drops by the members above.  A cluster is DONE when the digit's bin is wanted whole
//                      (its count == kk: no tie is cut; the last pass always ends so, comp being unique) or when it has fewer
//                      than `top` members at all.  A done cluster's cut is  comp >= prefix << shift.  The score digits come
//                      first, the row digits after them: a score shared by more rows than there are places left -- retweets --
//                      is refined on the row bits by the same passes.  When no cluster is left open the remaining passes exit
//                      at once (one word of state, read by every workgroup).
//   le_collect_kernel  the third kind of pass over keys and labels: a member at or above its cluster's cut claims a slot of the
//                      cluster's list (at most `top` do, by construction) and leaves its oi_rank_key there.
//   le_sort_kernel     a workgroup per cluster: the slots sorted by rank key in LDS (bitonic, unique keys: the order of arrival
//                      is gone), then scores, global docs and counts, the tail padded with (0, 0xFFFFFFFF).
#include "oi_volume.h"

// ------------------------------------------------------------------ shape constants (tests/test_exemplars_abi.py reads them)
constexpr uint32_t LE_BLOCK_ROWS = 64;    // rows whose labels a wave reads at once, one per lane
constexpr uint32_t LE_RANGE_ROWS = 2048;  // rows per range of the score pass
constexpr uint32_t LE_RADIX_BITS = 8;     // bits per pass of the select: hist is [n_clusters][256]
constexpr uint32_t LE_THREADS = 256;      // le_score / le_hist / le_collect: 4 waves
constexpr uint32_t LE_UNROLL = 4;         // member rows whose loads are in flight together
constexpr uint32_t LE_SORT_THREADS = 1024;
constexpr uint32_t LE_BINS = 1u << LE_RADIX_BITS;
constexpr uint32_t LE_LOCAL_CLUSTERS = 64; // up to here a workgroup of the select keeps its histogram in LDS: 64 KB
constexpr uint32_t LE_WAVE_ROWS = LE_RANGE_ROWS / (LE_THREADS / 64);
static_assert(LE_WAVE_ROWS % LE_BLOCK_ROWS == 0 && LE_BLOCK_ROWS == 64, "a wave's share of a range is whole blocks of one row per lane");
static_assert(32 % LE_RADIX_BITS == 0 && LE_BINS == 4 * 64, "whole digits per key word; le_scan_kernel reads four bins per lane");
static_assert(LE_LOCAL_CLUSTERS * LE_BINS * 4 <= 64 * 1024, "the local histogram fits the default dynamic LDS");
static_assert(OI_MAX_DEPTH == LE_SORT_THREADS, "le_sort_kernel holds a list as one key per thread");

#define LE_NO_KEY 0u

// a cluster's select state; zeroed per call except kk = top
struct LeCluster {
    unsigned long long prefix; // the digits chosen so far
    uint32_t kk;               // the rank wanted among the members that agree with prefix, >= 1 while open
    uint32_t shift;            // done: the cut is comp >= prefix << shift
    uint32_t done, claimed;    // claimed: slots taken by le_collect_kernel
    uint32_t pad[2];
};
static_assert(sizeof(LeCluster) == 32, "LeCluster");

__device__ __forceinline__ unsigned long long le_comp(uint32_t key, uint32_t row, uint32_t rb) {
    return ((unsigned long long)key << rb) | ((unsigned long long)(uint32_t)~row & ((1ull << rb) - 1ull)); // (rb <= 32)
}

// ------------------------------------------------------------------ the score pass
template <int NV, bool BF16, bool FILT>
__global__ __launch_bounds__(LE_THREADS) void le_score_kernel(const void *__restrict__ rows, const uint32_t *__restrict__ labels,
                                                              const uint2 *__restrict__ attrs, uint4 filt, uint64_t n, uint32_t dim,
                                                              uint32_t K, uint64_t n_ranges, const float *__restrict__ cent,
                                                              uint32_t *__restrict__ keys) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t nvec = dim >> 2;
    const size_t row_bytes = (size_t)dim * (BF16 ? 2 : 4);
    for (uint64_t range = blockIdx.x; range < n_ranges; range += gridDim.x) {
        for (uint32_t blk = 0; blk < LE_WAVE_ROWS / LE_BLOCK_ROWS; ++blk) {
            const uint64_t base = range * LE_RANGE_ROWS + (uint64_t)wave * LE_WAVE_ROWS + (uint64_t)blk * LE_BLOCK_ROWS;
            if (base >= n) break; // (wave-uniform)
            const uint64_t d = base + lane;
            const bool in = d < n;
            const uint32_t lab = in ? labels[d] : 0xFFFFFFFFu;
            bool member = lab < K;
            if (FILT && member) member = oi_doc_passes(filt, attrs[d]); // (a label < K was read: d < n)
            float sim = __builtin_nanf(""); // of this lane's row; NaN (no key) for a row that is not a member
            unsigned long long m = __ballot(member);
            while (m != 0ull) { // (wave-uniform) the next LE_UNROLL members of the block
                uint32_t rl[LE_UNROLL], cl[LE_UNROLL];
                float4 x[LE_UNROLL][NV];
#pragma unroll
                for (uint32_t u = 0; u < LE_UNROLL; ++u) {
                    rl[u] = 64u;
                    if (m != 0ull) {
                        rl[u] = (uint32_t)__builtin_ctzll(m);
                        m &= m - 1ull;
                    }
                    // (a slot without a row loads no row and reads centroid 0: nothing out of bounds)
                    cl[u] = rl[u] < 64u ? (uint32_t)__builtin_amdgcn_readlane((int)lab, (int)(rl[u] & 63u)) : 0u;
                }
#pragma unroll
                for (uint32_t u = 0; u < LE_UNROLL; ++u) {
                    const void *xr = reinterpret_cast<const unsigned char *>(rows) + (base + (rl[u] & 63u)) * row_bytes;
#pragma unroll
                    for (int j = 0; j < NV; ++j) {
                        const uint32_t v = lane + 64u * j;
                        x[u][j] = (rl[u] < 64u && v < nvec) ? vo_load_row4<BF16>(xr, v) : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                }
                float a[LE_UNROLL];
#pragma unroll
                for (uint32_t u = 0; u < LE_UNROLL; ++u) a[u] = 0.f;
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const uint32_t v = lane + 64u * j;
                    if (v < nvec) {
                        float4 y[LE_UNROLL];
#pragma unroll
                        for (uint32_t u = 0; u < LE_UNROLL; ++u) y[u] = reinterpret_cast<const float4 *>(cent)[(size_t)cl[u] * nvec + v];
#pragma unroll
                        for (uint32_t u = 0; u < LE_UNROLL; ++u) a[u] = vo_chain4(x[u][j], y[u], a[u]);
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < LE_UNROLL; ++u) {
                    if (rl[u] >= 64u) break; // (wave-uniform)
                    const float s = oi_wave_sum(a[u]); // (the same in every lane)
                    if (lane == rl[u]) sim = s;
                }
            }
            if (in) keys[d] = sim == sim ? oi_f32_key(sim) : LE_NO_KEY;
        }
    }
}

// ------------------------------------------------------------------ the select
// hist[c][digit] += 1 for the active lanes: lanes of one (cluster, digit) pair leave as one atomic, for the four most common
// pairs of the wave; what is left goes alone.
__device__ __forceinline__ void le_hist_add(uint32_t *hist, bool active, uint32_t cell) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const unsigned long long m = __ballot(active);
        if (!m) return;
        const uint32_t leader = (uint32_t)__builtin_ctzll(m);
        const uint32_t c0 = (uint32_t)__builtin_amdgcn_readlane((int)cell, (int)leader);
        const bool same = active && cell == c0;
        const unsigned long long ms = __ballot(same);
        if (lane == leader) atomicAdd(&hist[c0], (uint32_t)__popcll(ms));
        active = active && !same;
    }
    if (active) atomicAdd(&hist[cell], 1u);
}

// LOCAL (n_clusters <= LE_LOCAL_CLUSTERS): the workgroup adds into its own [n_clusters][LE_BINS] words of LDS and flushes the
// non-zero ones when its rows are done -- with few clusters the first pass sends every row of the corpus to a handful of
// addresses, and global atomics on one address serialise across the whole device.
template <bool LOCAL>
__global__ __launch_bounds__(LE_THREADS) void le_hist_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels, uint64_t n,
                                                             uint32_t K, uint32_t rb, uint32_t shift, const uint32_t *__restrict__ open,
                                                             const LeCluster *__restrict__ cl, uint32_t *__restrict__ hist_global) {
    extern __shared__ uint32_t le_local[]; // LOCAL: [K][LE_BINS]
    if (*open == 0u) return; // every cluster has its cut (uniform over the grid)
    uint32_t *hist = hist_global;
    if (LOCAL) {
        for (uint32_t i = threadIdx.x; i < K * LE_BINS; i += LE_THREADS) le_local[i] = 0u;
        __syncthreads();
        hist = le_local;
    }
    const uint64_t step = (uint64_t)gridDim.x * LE_THREADS;
    const uint64_t n_up = (n + 63u) & ~(uint64_t)63u; // (whole waves enter le_hist_add)
    for (uint64_t d = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x; d < n_up; d += step) {
        bool active = false;
        uint32_t cell = 0;
        if (d < n) {
            const uint32_t key = keys[d];
            if (key != LE_NO_KEY) { // (a key was stored: the label is < K)
                const uint32_t c = labels[d];
                const unsigned long long comp = le_comp(key, (uint32_t)d, rb);
                // (the first pass of a 64-bit composite has nothing above its digit: the prefix is 0)
                const unsigned long long above = shift + LE_RADIX_BITS >= 64u ? 0ull : comp >> (shift + LE_RADIX_BITS);
                active = cl[c].done == 0u && above == cl[c].prefix;
                cell = c * LE_BINS + (uint32_t)((comp >> shift) & (LE_BINS - 1u));
            }
        }
        le_hist_add(hist, active, cell);
    }
    if (LOCAL) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < K * LE_BINS; i += LE_THREADS)
            if (le_local[i] != 0u) atomicAdd(&hist_global[i], le_local[i]);
    }
}

// kk = top for every cluster (the rest of the state is zeroed by the launcher); one pass is open.
__global__ __launch_bounds__(256) void le_preset_kernel(uint32_t K, uint32_t top, LeCluster *cl, uint32_t *open) {
    for (uint32_t c = threadIdx.x; c < K; c += 256u) cl[c].kk = top;
    if (threadIdx.x == 0u) open[0] = 1u;
}

// One workgroup, a wave per cluster at a time.  Reads and clears hist; *open_next = the clusters still open.
__global__ __launch_bounds__(1024) void le_scan_kernel(uint32_t K, uint32_t shift, const uint32_t *__restrict__ open, uint32_t *open_next,
                                                       LeCluster *cl, uint32_t *hist) {
    __shared__ uint32_t left;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0u) left = 0u;
    __syncthreads();
    if (*open != 0u) { // (uniform)
        for (uint32_t c = wave; c < K; c += 1024u / 64u) {
            LeCluster s = cl[c];
            if (s.done != 0u) continue; // (wave-uniform)
            // lane l holds the bins 255 - 4 l .. 252 - 4 l: from the top, in lane order
            uint32_t *h = hist + (size_t)c * LE_BINS + (LE_BINS - 4u - 4u * lane);
            const uint4 b = *reinterpret_cast<const uint4 *>(h); // (b.w is the highest bin of the four)
            *reinterpret_cast<uint4 *>(h) = make_uint4(0u, 0u, 0u, 0u);
            const uint32_t mine = b.x + b.y + b.z + b.w;
            const uint32_t incl = oi_wave_incl_scan(mine);
            const unsigned long long ball = __ballot(incl >= s.kk);
            if (ball == 0ull) {
                // fewer members agree with the prefix than are wanted: only on the first pass (later kk <= the chosen bin's
                // count), so the cluster has fewer than `top` members and every one of them is listed
                if (lane == 0u) {
                    s.prefix = 0ull;
                    s.shift = 0u;
                    s.done = 1u;
                    cl[c] = s;
                }
                continue;
            }
            const uint32_t l1 = (uint32_t)__builtin_ctzll(ball);
            const uint32_t before = (uint32_t)__builtin_amdgcn_readlane((int)(incl - mine), (int)l1);
            const uint32_t bw = (uint32_t)__builtin_amdgcn_readlane((int)b.w, (int)l1), bz = (uint32_t)__builtin_amdgcn_readlane((int)b.z, (int)l1),
                           by = (uint32_t)__builtin_amdgcn_readlane((int)b.y, (int)l1), bx = (uint32_t)__builtin_amdgcn_readlane((int)b.x, (int)l1);
            if (lane == 0u) {
                uint32_t kk = s.kk - before, digit = LE_BINS - 1u - 4u * l1, cnt = bw;
                if (kk > cnt) { kk -= cnt; --digit; cnt = bz; }
                if (kk > cnt) { kk -= cnt; --digit; cnt = by; }
                if (kk > cnt) { kk -= cnt; --digit; cnt = bx; }
                s.prefix = (s.prefix << LE_RADIX_BITS) | digit;
                s.kk = kk;
                if (kk == cnt || shift == 0u) { // the bin is wanted whole: the cut is its lower edge
                    s.shift = shift;
                    s.done = 1u;
                } else {
                    atomicAdd(&left, 1u);
                }
                cl[c] = s;
            }
        }
    }
    __syncthreads();
    if (tid == 0u) *open_next = left;
}

__global__ __launch_bounds__(LE_THREADS) void le_collect_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels, uint64_t n,
                                                                uint32_t rb, uint32_t top, uint32_t doc_id_base, LeCluster *cl,
                                                                unsigned long long *__restrict__ slots) {
    const uint64_t step = (uint64_t)gridDim.x * LE_THREADS;
    for (uint64_t d = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x; d < n; d += step) {
        const uint32_t key = keys[d];
        if (key == LE_NO_KEY) continue;
        const uint32_t c = labels[d];
        const unsigned long long prefix = cl[c].prefix;
        const uint32_t shift = cl[c].shift;
        if ((le_comp(key, (uint32_t)d, rb) >> shift) < prefix) continue;
        const uint32_t pos = atomicAdd(&cl[c].claimed, 1u);
        if (pos < top) slots[(size_t)c * top + pos] = ((unsigned long long)key << 32) | (unsigned long long)(uint32_t)~(doc_id_base + (uint32_t)d);
    }
}

// A workgroup per cluster, a key per thread: bitonic sort, descending.  An empty slot is key 0, below every member's.
__global__ __launch_bounds__(LE_SORT_THREADS) void le_sort_kernel(const LeCluster *__restrict__ cl, const unsigned long long *__restrict__ slots,
                                                                  uint32_t top, float *__restrict__ scores, uint32_t *__restrict__ docs,
                                                                  uint32_t *__restrict__ counts) {
    __shared__ unsigned long long sk[LE_SORT_THREADS];
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    const uint32_t count = cl[c].claimed < top ? cl[c].claimed : top;
    uint32_t width = 64u; // the power of two that holds the list (uniform)
    while (width < top) width <<= 1;
    sk[tid] = tid < count ? slots[(size_t)c * top + tid] : 0ull;
    __syncthreads();
    for (uint32_t k = 2; k <= width; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t other = tid ^ j;
            if (tid < width && other > tid) {
                const unsigned long long a = sk[tid], b = sk[other];
                const bool desc = (tid & k) == 0u;
                if (desc ? a < b : a > b) { sk[tid] = b; sk[other] = a; }
            }
            __syncthreads();
        }
    }
    if (tid < top) {
        const unsigned long long k = sk[tid];
        const bool valid = tid < count;
        scores[(size_t)c * top + tid] = valid ? oi_rank_key_score(k) : 0.f;
        docs[(size_t)c * top + tid] = valid ? oi_rank_key_doc(k) : 0xFFFFFFFFu;
    }
    if (tid == 0u) counts[c] = count;
}

// ------------------------------------------------------------------ host
// the workspace "exemplars": open words | cluster states | hist | keys | slots | rounded centroids (bf16 corpus)
struct LeWorkspace {
    StageLayout lay{256};
    size_t open, clusters, hist, keys, slots, rounded;
    LeWorkspace(uint64_t n, uint32_t K, uint32_t dim, uint32_t top, bool bf16) {
        open = lay.add(256);
        clusters = lay.add(sizeof(LeCluster) * (size_t)K);
        hist = lay.add(sizeof(uint32_t) * (size_t)K * LE_BINS);
        keys = lay.add(sizeof(uint32_t) * (size_t)n);
        slots = lay.add(sizeof(uint64_t) * (size_t)K * top);
        rounded = lay.add(bf16 ? sizeof(float) * (size_t)K * dim : 0);
    }
};

template <int NV, bool BF16>
static void le_launch_score(oi_ctx *ctx, uint32_t grid, const void *rows, const uint32_t *labels, const uint2 *attrs, uint4 filt, bool has_filt,
                            uint64_t n, uint32_t dim, uint32_t K, uint64_t n_ranges, const float *cent, uint32_t *keys) {
    if (has_filt)
        hipLaunchKernelGGL((le_score_kernel<NV, BF16, true>), dim3(grid), dim3(LE_THREADS), 0, ctx->stream, rows, labels, attrs, filt, n, dim, K,
                           n_ranges, cent, keys);
    else
        hipLaunchKernelGGL((le_score_kernel<NV, BF16, false>), dim3(grid), dim3(LE_THREADS), 0, ctx->stream, rows, labels, attrs, filt, n, dim, K,
                           n_ranges, cent, keys);
}

// Device labels [n_docs] and centroids [K][dim] in, device scores / docs [K][top] and counts [K] out; asynchronous on the ctx
// stream.  The argument and state checks are api.hip's.
int oi_launch_label_exemplars(oi_index *idx, const uint32_t *d_labels, const float *d_centroids, uint32_t K, uint32_t top,
                              const oi_doc_filter *filter, float *d_scores, uint32_t *d_docs, uint32_t *d_counts) {
    static_assert(sizeof(oi_doc_filter) == sizeof(uint4), "oi_doc_filter is 16 bytes");
    static_assert(OI_MAX_DIM <= 1024u, "le_score_kernel holds a row in at most 4 float4 per lane");
    oi_ctx *ctx = idx->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = idx->n_docs;
    const uint32_t dim = idx->dim;
    const bool bf16 = idx->rows_bf16 != nullptr;
    const LeWorkspace L(n, K, dim, top, bf16);
    DevBuf &ws = ctx->buf("exemplars");
    OI_CHECK(ws.ensure(L.lay.total()));
    uint32_t *open = L.lay.at<uint32_t>(ws.p, L.open); // open[p]: clusters open before pass p (open[0] = 1)
    LeCluster *cl = L.lay.at<LeCluster>(ws.p, L.clusters);
    uint32_t *hist = L.lay.at<uint32_t>(ws.p, L.hist), *keys = L.lay.at<uint32_t>(ws.p, L.keys);
    unsigned long long *slots = L.lay.at<unsigned long long>(ws.p, L.slots);
    float *rounded = L.lay.at<float>(ws.p, L.rounded);

    // the composite's row bits, in whole digits, and the passes of the select
    uint32_t rb = 0;
    while (rb < 32u && n > 0 && ((n - 1) >> rb) != 0ull) rb += LE_RADIX_BITS;
    const uint32_t passes = (32u + rb) / LE_RADIX_BITS; // 4 .. 8
    static_assert(256 >= sizeof(uint32_t) * (64 / LE_RADIX_BITS + 1), "the open words fit the head of the workspace");

    OI_HIP_CHECK(hipMemsetAsync(ws.p, 0, L.keys, st)); // the open words, the cluster states and the histograms
    const float *cent = d_centroids;
    if (bf16) {
        OI_CHECK(oi_launch_volume_round_queries(ctx, d_centroids, (uint64_t)K * dim, rounded));
        cent = rounded;
    }
    const void *rows = bf16 ? (const void *)idx->rows_bf16 : (const void *)idx->rows;
    const uint2 *attrs = filter ? idx->doc_attrs.as<uint2>() : nullptr;
    const uint4 filt = oi_filter_words(filter);
    const uint64_t n_ranges = (n + LE_RANGE_ROWS - 1) / LE_RANGE_ROWS;
    if (n) {
        ProfScope ps(ctx, "exemplar_score");
        // four workgroups of four waves per CU, each wave with LE_UNROLL rows in flight
        const uint32_t grid = (uint32_t)std::min<uint64_t>(n_ranges, (uint64_t)ctx->num_cus * 4);
        const uint32_t nv = (dim / 4 + 63) / 64; // float4 per lane: 1 .. 4
#define LE_SCORE(NV, BF) le_launch_score<NV, BF>(ctx, grid, rows, d_labels, attrs, filt, filter != nullptr, n, dim, K, n_ranges, cent, keys)
        if (bf16) {
            if (nv <= 1) LE_SCORE(1, true); else if (nv == 2) LE_SCORE(2, true); else if (nv == 3) LE_SCORE(3, true); else LE_SCORE(4, true);
        } else {
            if (nv <= 1) LE_SCORE(1, false); else if (nv == 2) LE_SCORE(2, false); else if (nv == 3) LE_SCORE(3, false); else LE_SCORE(4, false);
        }
#undef LE_SCORE
        OI_HIP_CHECK(hipGetLastError());
    }
    const uint32_t flat = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + LE_THREADS - 1) / LE_THREADS, (uint64_t)ctx->num_cus * 8));
    {
        ProfScope ps(ctx, "exemplar_select");
        hipLaunchKernelGGL(le_preset_kernel, dim3(1), dim3(256), 0, st, K, top, cl, open);
        for (uint32_t p = 0; p < passes; ++p) {
            const uint32_t shift = (passes - 1u - p) * LE_RADIX_BITS;
            if (n && K <= LE_LOCAL_CLUSTERS)
                hipLaunchKernelGGL(le_hist_kernel<true>, dim3(flat), dim3(LE_THREADS), sizeof(uint32_t) * K * LE_BINS, st, keys, d_labels, n, K,
                                   rb, shift, open + p, cl, hist);
            else if (n)
                hipLaunchKernelGGL(le_hist_kernel<false>, dim3(flat), dim3(LE_THREADS), 0, st, keys, d_labels, n, K, rb, shift, open + p, cl, hist);
            hipLaunchKernelGGL(le_scan_kernel, dim3(1), dim3(1024), 0, st, K, shift, open + p, open + p + 1, cl, hist);
        }
        OI_HIP_CHECK(hipGetLastError());
    }
    {
        ProfScope ps(ctx, "exemplar_emit");
        if (n) hipLaunchKernelGGL(le_collect_kernel, dim3(flat), dim3(LE_THREADS), 0, st, keys, d_labels, n, rb, top, idx->doc_id_base, cl, slots);
        hipLaunchKernelGGL(le_sort_kernel, dim3(K), dim3(LE_SORT_THREADS), 0, st, cl, slots, top, d_scores, d_docs, d_counts);
        OI_HIP_CHECK(hipGetLastError());
    }
    return OI_OK;
}
