// cosine_groups.hip -- oi_similar_groups: the social_summary sums of the documents like a query, per KEY of the documents'
// group attribute (a ticker id, say), dense or ranked on the device.
//
// The third tally of the threshold family (oi_volume.h).  The three clauses are the summary's with "bucket" replaced by
// "key": a document passes filters[q], has key(d) = (group[d] & key_mask) >> ctz(key_mask) < n_keys, and sim(q, d) >= t_q.
// The family's kernels evaluate clause 2 on the group instead of the stamp for a tally with KEY_AXIS; everything else -- the
// stream of the screening copy, the band, the exact route, the gated fallback -- is the summary's, and so is the cell
// (oi_summary_cell.h: 16 words, one u32 atomic per hit and a 64-bit one for a non-zero polarity).  Integer sums: the cells do
// not depend on the route or on the order of the atomics.
//
// What is new is the finish, two steps on the ctx stream:
//   (a) groups_finish_kernel folds every cell: dense output (top == 0) takes the record; ranked output takes the cell's
//       64-bit RANK KEY  v << 32 | ~key  (v = the record's total / spec_count / bullish / bearish), or 0 for a key whose total
//       is below the bar -- the library's usual key: "v descending, key ascending" is descending u64 order, keys are distinct.
//   (b) groups_rank_kernel, one workgroup per query: the top `top` of up to 65 536 rank keys by radix select (8-bit digits
//       from the highest byte any key uses; out of LDS when n_keys <= 8192, over the key array otherwise), a bitonic sort of the
//       selected ones, then the key, the folded record and the counts are written.
#include "oi_summary_cell.h"
#include "oi_volume.h"

#define GR_THREADS 1024
#define GR_MAX_TOP 1024     // == OI_MAX_DEPTH
#define GR_LDS_KEYS 8192    // 64 KB of rank keys: above it the passes read the key array in the workspace

// ------------------------------------------------------------------ finish (a): cells -> records, or rank keys
__global__ __launch_bounds__(256) void groups_finish_kernel(const uint32_t *__restrict__ cells, uint64_t n_cells, uint32_t n_keys,
                                                            uint32_t rank_by, uint32_t min_total, oi_social_counters *__restrict__ out,
                                                            uint64_t *__restrict__ rank_keys) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += (uint64_t)gridDim.x * blockDim.x) {
        if (!rank_keys) { // (uniform) dense output
            sm_fold(cells + i * SM_CELL_WORDS, out + i);
            continue;
        }
        oi_social_counters o;
        sm_fold(cells + i * SM_CELL_WORDS, &o);
        const uint64_t v = rank_by == OI_GROUP_RANK_TOTAL ? o.total : rank_by == OI_GROUP_RANK_SPEC ? o.spec_count
                         : rank_by == OI_GROUP_RANK_BULLISH ? o.bullish : o.bearish; // (sums of u32 counts of at most 2^32 - 1 rows)
        const uint32_t key = (uint32_t)(i % n_keys);
        rank_keys[i] = o.total >= min_total ? (v << 32) | (uint32_t)~key : 0ull; // (min_total >= 1; ~key != 0: never 0 when listed)
    }
}

// ------------------------------------------------------------------ finish (b): the ranking
// hist[digit] += 1 for the active lanes; the two most common digits of the wave go in as one atomic each (counts of a few
// posts per key share their leading bytes: nearly every key of a pass has the same digit)
__device__ __forceinline__ void gr_hist_add(uint32_t *hist, bool active, uint32_t digit) {
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned long long m = __ballot(active);
        if (!m) return;
        const uint32_t leader = (uint32_t)__builtin_ctzll(m);
        const uint32_t d0 = (uint32_t)__shfl((int)digit, (int)leader, OI_WAVE);
        const unsigned long long same = __ballot(active && digit == d0);
        if (lane == leader) atomicAdd(&hist[d0], (uint32_t)__popcll(same));
        active = active && digit != d0;
    }
    if (active) atomicAdd(&hist[digit], 1u);
}

// wave-aggregated append of the lanes' keys to dst (cap entries); *count counts every taken key, stored or not
__device__ __forceinline__ void gr_append(uint64_t *dst, uint32_t *count, uint32_t cap, bool take, uint64_t key) {
    const unsigned long long m = __ballot(take);
    if (!m) return;
    const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__builtin_ctzll(m);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, (int)leader, OI_WAVE);
    const uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (take && pos < cap) dst[pos] = key;
}

// In-LDS bitonic sort, descending, P a power of two <= 2 * GR_THREADS; all threads call.
__device__ __forceinline__ void gr_sort_desc(uint64_t *a, uint32_t P) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t size = 2; size <= P; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            if (tid < (P >> 1)) {
                const uint32_t lo = 2 * tid - (tid & (stride - 1)), hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const uint64_t x = a[lo], y = a[hi];
                if ((x < y) == desc) { a[lo] = y; a[hi] = x; }
            }
            __syncthreads();
        }
    }
}

// One workgroup per query.  rank_keys[q][n_keys]: 0 = not listed.  Writes keys_out[q][top], records_out[q][top] (entries past
// the count: key 0xFFFFFFFF, an all-zero record), counts_out[q] and, when given, qualified_out[q].
__global__ __launch_bounds__(GR_THREADS) void groups_rank_kernel(const uint64_t *__restrict__ rank_keys, const uint32_t *__restrict__ cells,
                                                                 uint32_t n_keys, uint32_t top, oi_social_counters *__restrict__ records_out,
                                                                 uint32_t *__restrict__ keys_out, uint32_t *__restrict__ counts_out,
                                                                 uint32_t *__restrict__ qualified_out) {
    __shared__ uint32_t hist[256];
    __shared__ uint64_t sel[GR_MAX_TOP];
    __shared__ uint64_t lds_keys[GR_LDS_KEYS];
    __shared__ uint32_t s_cnt, s_kk, s_bin_cnt, s_qual;
    __shared__ uint64_t s_prefix;
    __shared__ unsigned long long s_max;

    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const uint64_t *gk = rank_keys + (uint64_t)q * n_keys;
    const bool in_lds = n_keys <= GR_LDS_KEYS; // (uniform)
    if (tid == 0) { s_cnt = 0; s_qual = 0; s_max = 0ull; }
    __syncthreads();
    {
        // the listed keys are counted, the largest found (it says which byte the select starts at), a small array staged
        uint32_t mine = 0;
        unsigned long long mx = 0ull;
        for (uint32_t i = tid; i < n_keys; i += GR_THREADS) {
            const uint64_t k = gk[i];
            if (in_lds) lds_keys[i] = k;
            mine += k != 0ull ? 1u : 0u;
            mx = k > mx ? k : mx;
        }
        mine = oi_wave_sum(mine);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long v = __shfl_xor(mx, o, OI_WAVE);
            mx = v > mx ? v : mx;
        }
        if (lane == 0 && mine) { atomicAdd(&s_qual, mine); atomicMax(&s_max, mx); }
    }
    __syncthreads();
    const uint32_t qual = s_qual, m = qual < top ? qual : top;
    // every pass sees the same keys; all lanes of a wave make the same number of steps (the helpers vote); 0 = no key
    auto for_each = [&](auto &&f) {
        for (uint32_t i0 = 0; i0 < n_keys; i0 += GR_THREADS) {
            const uint32_t i = i0 + tid;
            f(i < n_keys ? (in_lds ? lds_keys[i] : gk[i]) : 0ull);
        }
    };
    if (qual <= top) {
        for_each([&](uint64_t k) { gr_append(sel, &s_cnt, GR_MAX_TOP, k != 0ull, k); });
        __syncthreads();
    } else {
        // radix select of the top-th largest listed key: 8-bit digits from the highest byte in use (qual > top >= 1: s_max != 0)
        int shift = 56 - 8 * (__builtin_clzll(s_max) >> 3);
        if (tid == 0) { s_prefix = 0; s_kk = top; }
        for (;; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            const uint64_t prefix = s_prefix;
            const bool first = shift == 56;
            for_each([&](uint64_t k) {
                gr_hist_add(hist, k != 0ull && (first || (k >> ((shift + 8) & 63)) == prefix), (uint32_t)(k >> shift) & 255u);
            });
            __syncthreads();
            if (tid < 64) { // wave 0: the digit holding the kk-th key counted from the top
                const uint32_t kk = s_kk;
                uint32_t mine = 0;
                for (int i = 0; i < 4; ++i) mine += hist[255 - (tid * 4 + i)];
                const uint32_t incl = oi_wave_incl_scan(mine);
                const unsigned long long ball = __ballot(incl >= kk);
                const uint32_t owner = ball ? (uint32_t)__builtin_ctzll(ball) : 63u;
                if (tid == owner) {
                    uint32_t cum = incl - mine;
                    int d = 255 - (int)(tid * 4);
                    for (int i = 0; i < 3; ++i, --d) {
                        const uint32_t c = hist[d];
                        if (cum + c >= kk) break;
                        cum += c;
                    }
                    s_prefix = (prefix << 8) | (uint64_t)d;
                    s_kk = kk - cum;
                    s_bin_cnt = hist[d];
                }
            }
            __syncthreads();
            if (s_bin_cnt == 1 || shift == 0) break;
        }
        // every listed key whose top bits are >= prefix is selected: exactly `top` of them (keys are distinct)
        const uint64_t prefix = s_prefix;
        for_each([&](uint64_t k) { gr_append(sel, &s_cnt, GR_MAX_TOP, k != 0ull && (k >> shift) >= prefix, k); });
        __syncthreads();
    }
    uint32_t P = 2;
    while (P < m) P <<= 1;
    for (uint32_t i = m + tid; i < P; i += GR_THREADS) sel[i] = 0ull; // lowest possible key
    __syncthreads();
    gr_sort_desc(sel, P);
    for (uint32_t i = tid; i < top; i += GR_THREADS) {
        const uint32_t key = i < m ? ~(uint32_t)sel[i] : 0xFFFFFFFFu;
        oi_social_counters *rec = records_out + (uint64_t)q * top + i;
        if (i < m) sm_fold(cells + ((uint64_t)q * n_keys + key) * SM_CELL_WORDS, rec); // (key < n_keys: finish (a) made it from the cell's index)
        else *rec = oi_social_counters{};
        keys_out[(uint64_t)q * top + i] = key;
    }
    if (tid == 0) {
        counts_out[q] = m;
        if (qualified_out) qualified_out[q] = qual;
    }
}

// ------------------------------------------------------------------ the finish of a key-axis tally, on the ctx stream
// cells [n_cells / n_keys][n_keys] -> the caller's arrays.  top == 0: dense records, nothing else is written.  top >= 1: the
// ranked output, with n_cells u64 of the caller's workspace behind rank_keys, timed under `rank_tag`.  (oi_similar_groups and
// oi_label_summary share it: one ranking.)
int oi_launch_groups_finish(oi_ctx *ctx, const uint32_t *cells, uint64_t n_cells, uint32_t n_keys, uint32_t top, uint32_t rank_by,
                            uint32_t min_total, uint64_t *rank_keys, const char *rank_tag, oi_social_counters *d_records, uint32_t *d_keys,
                            uint32_t *d_counts, uint32_t *d_qualified) {
    const dim3 grid((uint32_t)std::min<uint64_t>((n_cells + 255) / 256, 1024));
    if (top == 0) {
        hipLaunchKernelGGL(groups_finish_kernel, grid, dim3(256), 0, ctx->stream, cells, n_cells, n_keys, 0u, 0u, d_records, (uint64_t *)nullptr);
        OI_HIP_CHECK(hipGetLastError());
        return OI_OK;
    }
    ProfScope ps(ctx, rank_tag);
    hipLaunchKernelGGL(groups_finish_kernel, grid, dim3(256), 0, ctx->stream, cells, n_cells, n_keys, rank_by, std::max(min_total, 1u),
                       (oi_social_counters *)nullptr, rank_keys);
    OI_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(groups_rank_kernel, dim3((uint32_t)(n_cells / n_keys)), dim3(GR_THREADS), 0, ctx->stream, rank_keys, cells, n_keys, top,
                       d_records, d_keys, d_counts, d_qualified);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// ------------------------------------------------------------------ the key-axis tally
// SmSum's cell and thresholds (cosine_summary.hip) with clause 2 on the key; the host part carries what the finish needs.
struct GrOut {
    oi_social_counters *records;
    uint32_t *keys, *counts, *qualified;
};
struct GrSum {
    float thr_all;
    const uint2 *sig;      // the index's signal records
    uint32_t *cells;
    uint32_t n_keys, top, rank_by, min_total; // (host: finish)
    typedef const float *__restrict__ Thr;
    typedef uint2 Rec;
    __device__ __forceinline__ float thr(uint32_t q, Thr thr_q) const { return thr_q ? thr_q[q] : thr_all; }
    __device__ __forceinline__ Rec load(uint64_t row) const { return sig[row]; }
    __device__ __forceinline__ void add(uint64_t cell, const Rec sg) const { sm_add(cells, cell, sg); }

    static constexpr uint32_t CELL_WORDS = SM_CELL_WORDS;
    static constexpr bool KEY_AXIS = true, EXCLUSIVE = false;
    static constexpr VoNames NAMES = {"groups_state", "groups_runs", "groups_q_rounded", "groups_q_bf16",
                                      "groups", "groups_band", "groups_exact", "groups_fallback"};
    static const float *thr_block(const float *thr_q, uint32_t q0) { return thr_q ? thr_q + q0 : nullptr; }
    int finish(oi_ctx *ctx, uint64_t n_cells, const GrOut *out) const {
        uint64_t *rank_keys = nullptr;
        if (top != 0) {
            DevBuf &kb = ctx->buf("groups_keys");
            OI_CHECK(kb.ensure(n_cells * sizeof(uint64_t)));
            rank_keys = kb.as<uint64_t>();
        }
        return oi_launch_groups_finish(ctx, cells, n_cells, n_keys, top, rank_by, min_total, rank_keys, "groups_rank", out->records, out->keys,
                                       out->counts, out->qualified);
    }
};

// Device queries / thresholds / filters in, device outputs out; asynchronous on the ctx stream (vo_launch_similar).
int oi_launch_similar_groups(oi_index *idx, const float *d_q, uint32_t B, const oi_groups_spec &sp, const float *d_thr, const uint4 *d_filt,
                             oi_social_counters *d_records, uint32_t *d_keys, uint32_t *d_counts, uint32_t *d_qualified) {
    static_assert(sizeof(oi_social_counters) == 64, "one record per cell");
    static_assert(GR_MAX_TOP == OI_MAX_DEPTH, "the rank kernel's list");
    // the family's three u32 of clause 2 carry the key: mask, shift, n_keys
    const oi_volume_spec vs = {sp.threshold, sp.key_mask, (uint32_t)__builtin_ctz(sp.key_mask), sp.n_keys};
    const GrOut out = {d_records, d_keys, d_counts, d_qualified};
    return vo_launch_similar(idx, d_q, B, vs, d_thr, d_filt,
                             GrSum{sp.threshold, idx->signals.as<uint2>(), nullptr, sp.n_keys, sp.top, sp.rank_by, sp.min_total}, &out);
}
