// label_terms.hip -- the distinguishing terms of each cluster of posts: oi_label_term_counts, oi_label_terms_rank
// and their composition oi_label_terms.  The lexical counterpart of oi_label_sums (centroids.hip): labels in, integers out.
//
//   lt_plan_kernel    the first term of every TASK of the count pass.
//   lt_count_kernel   counts[t][c] = documents d with labels[d] == c < n_clusters that have a posting for term t: one pass over the
//                     postings (bm25.hip states the layout) with one label gather and one LDS atomic per posting.
//   lt_sizes_kernel   sizes[c] = rows with labels[d] == c: one pass over the labels, a per-wave fold, one atomic per wave and cluster.
//   lt_rank_kernel    per slice of LT_RANK_SLICE terms and cluster, the best `top` terms of the slice under the three-part order.
//   lt_merge_kernel   LT_MERGE_FAN sorted lists of a cluster into one; the last round writes the records.
//   lt_put_sizes_kernel  the host's sizes (a kernel argument) into the rank's workspace: the call stays asynchronous.
//
// lt_count_kernel.  The posting array is cut every LT_SPLIT_POSTINGS postings; task j is the cut [j S, (j + 1) S).  A term with
// fewer than LT_SPLIT_POSTINGS postings is LIGHT and belongs whole to the task its first posting falls in, so a task reads fewer
// than 2 S postings; one with that many or more is SPLIT at the cuts, and every task counts the piece inside its cut.  A task's
// terms are the run [first_term[j], first_term[j + 1]) of the plan (terms without a posting have a start too, and are skipped);
// a split term can only be the last of them that has postings, or the one before the first.  The waves of a workgroup take the
// light terms in turn and a quarter of a split piece each.  A wave keeps the term's n_clusters counters in its own LDS words,
// replicated 2^rep times ([cluster][lane mod 2^rep]: with few clusters the lanes of one label do not meet on one word), folds
// the replicas with shuffles and writes: a light term leaves as plain contiguous stores of its n_clusters words, a split piece
// adds its non-zero words with global integer atomics (the table is zeroed by the launcher).
// The block of posting i of term t is the b with cell_start[t n_win + 2 b] <= i < cell_start[t n_win + 2 b + 2].  A wave walks a
// range 64 postings at a time and carries the current block and its end: while the 64 stay inside it no bound is read.  When a
// lane leaves it the wave holds a WINDOW of 64 block ends in LDS (one load of the term's row of cell_start, a lane per block),
// a lane bisects the window (six LDS reads), and the window moves on by 64 blocks while a lane lies behind it.  A piece of a
// split term finds its first block by one bisection of the row; a light term starts at block 0.
// Every bound is held inside the arrays whatever cell_start says: i < hi <= n_postings, a row index <= n_win, the document < n_docs
// before its label is read, the label < n_clusters before it reaches an address.
//
// lt_rank_kernel / lt_merge_kernel.  A list entry is two u64 that order like the definition: k1 = excess with its sign bit
// flipped, k2 = counts << 32 | ~term; larger (k1, k2) is better and (0, 0) is "no entry" (a real entry has counts >= 1).  The
// 64-bit rank keys of oi_select_rank.h cannot hold it -- the excess alone needs 63 bits and a sign -- so the lists are pairs.
// One wave per (slice, 64 clusters): lane = cluster, the term's row is read coalesced, dfA is the wave's sum of the row, and
// each lane inserts into its own sorted list in LDS ([position][lane]: no two lanes share a bank).  The order is total, so any
// schedule of slices and rounds writes the same bytes.
#include "oi_device.h"
#include "oi_internal.h"

#include <algorithm>

// ------------------------------------------------------------------ shape constants (tests/test_label_terms_abi.py reads them)
constexpr uint32_t LT_THREADS = 256;           // threads per workgroup of the count pass: 4 waves
constexpr uint32_t LT_SPLIT_POSTINGS = 16384;  // postings per task cut; a term with this many postings or more is split
constexpr uint32_t LT_HIST_WORDS = 256;        // LDS counters per wave: n_clusters x replicas
constexpr uint32_t LT_TERM_BATCH = 64;         // light terms whose bounds a wave reads at once, one per lane
constexpr uint32_t LT_RANK_SLICE = 1024;       // terms per slice of the rank's first level
constexpr uint32_t LT_RANK_UNROLL = 4;         // rows of the table in flight per wave of the rank
constexpr uint32_t LT_MERGE_FAN = 64;          // lists merged by one wave, one per lane
static_assert(LT_HIST_WORDS >= OI_MAX_CENTROIDS && LT_HIST_WORDS % 64 == 0, "a wave's counters hold every cluster once");
static_assert(OI_MAX_LABEL_TERMS == 64, "the final merge finishes one record per lane");
static_assert(LT_SPLIT_POSTINGS % 64 == 0, "a wave's quarter of a split piece is whole steps");

#define LT_R OI_BM25_BLOCK_DOCS

// the wave's LDS words written by some lanes are read by others: keep the accesses in program order
__device__ __forceinline__ void lt_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ uint64_t lt_min64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t lt_wave_sum64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, OI_WAVE);
    return v;
}

// first_term[j] = the first term whose list starts at or after posting j S (vocab: none), j in [0, n_tasks]
__global__ __launch_bounds__(256) void lt_plan_kernel(const uint32_t *__restrict__ cell_start, uint32_t n_win, uint32_t vocab, uint32_t n_postings,
                                                      uint32_t n_tasks, uint32_t *__restrict__ first_term) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n_tasks) return;
    const uint64_t target = (uint64_t)j * LT_SPLIT_POSTINGS;
    uint32_t lo = 0, hi = vocab; // the answer is in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)min(cell_start[(uint64_t)mid * n_win], n_postings) >= target) hi = mid;
        else lo = mid + 1;
    }
    first_term[j] = lo;
}

struct LtArgs {
    const uint2 *postings;
    const uint32_t *cell_start, *first_term, *labels;
    uint64_t n_docs;
    uint32_t n_postings, vocab, n_win, K, rep_log2, n_tasks;
    uint32_t *counts;
};

// One wave: postings [lo, hi) of term t into the wave's counters, then out.  ATOMIC: a piece of a split term.
// GATHER / WALK = false exist in -DOI_ABLATION builds only ("timings only, results wrong by construction"): no label gather
// (label = document mod n_clusters), no block search (every posting in block 0); lt_count_kernel's SPLIT_ADDS = false stores the
// pieces of a split term instead of adding them.
template <bool GATHER, bool WALK>
__device__ __forceinline__ void lt_wave_term(const LtArgs &a, uint32_t t, uint32_t lo, uint32_t hi, bool atomic, uint32_t *hist, uint32_t *fold,
                                             uint32_t lane) {
    const uint32_t *row = a.cell_start + (uint64_t)t * a.n_win;
    const uint32_t nb = a.n_win >> 1, rep_mask = (1u << a.rep_log2) - 1u;
    // (wave-uniform) the current block and its end; the WINDOW: fold[k] = the end of block win_blk + k, k < 64 (0xFFFFFFFF behind
    // the last block: every posting ends before that), win_max = fold[63].  cur_end = 0 sends the first step through the search.
    uint32_t cur_blk = 0, cur_end = 0, win_blk = 0, win_max = 0;
    bool loaded = false;
    if (WALK && atomic) { // a piece starts anywhere in its term: its first posting's block by bisection, once
        uint32_t blo = 0, bhi = nb - 1u;
        while (blo < bhi) {
            const uint32_t mid = (blo + bhi) >> 1;
            if (row[2u * mid + 2u] > lo) bhi = mid;
            else blo = mid + 1u;
        }
        win_blk = blo;
    }
    auto load_window = [&]() {
        lt_wave_sync();
        const uint32_t wb = win_blk + lane;
        const uint32_t e = wb < nb ? row[2u * wb + 2u] : 0xFFFFFFFFu;
        fold[lane] = e;
        win_max = (uint32_t)__shfl((int)e, 63);
        lt_wave_sync();
    };
    for (uint32_t i0 = lo; i0 < hi; i0 += 64) {
        const uint32_t i = i0 + lane;
        const bool valid = i < hi;
        const uint2 p = valid ? a.postings[i] : make_uint2(0xFFFFFFFFu, 0u);
        uint32_t b = cur_blk;
        if (WALK && __ballot(valid && i >= cur_end) != 0ull) { // (wave-uniform) a lane has left the current block
            bool pending = valid && i >= cur_end;
            if (!loaded) {
                load_window();
                loaded = true;
            }
            for (;;) { // the lanes leave in posting order, so the window only moves forward
                if (pending && i < win_max) { // the smallest k with fold[k] > i
                    uint32_t klo = 0, khi = 63;
                    while (klo < khi) {
                        const uint32_t mid = (klo + khi) >> 1;
                        if (fold[mid] > i) khi = mid;
                        else klo = mid + 1u;
                    }
                    b = win_blk + klo;
                    pending = false;
                }
                if (__ballot(pending) == 0ull) break;
                win_blk += 64u;
                load_window();
            }
            b = min(b, nb - 1u);
            cur_blk = (uint32_t)__shfl((int)b, (int)min(63u, hi - 1u - i0)); // the last posting of the step was placed last: in this window
            const uint32_t k = cur_blk - win_blk;
            cur_end = k < 64u ? fold[k] : 0u;
        }
        if (valid) {
            const uint64_t doc = (uint64_t)b * LT_R + p.x;
            if (p.x < LT_R && doc < a.n_docs) {
                const uint32_t l = GATHER ? a.labels[doc] : (uint32_t)(doc % a.K);
                if (l < a.K) atomicAdd(&hist[(l << a.rep_log2) + (lane & rep_mask)], 1u);
            }
        }
    }
    // fold the replicas: the lanes of a group of 2^rep consecutive words hold one cluster's
    lt_wave_sync();
    const uint32_t words = a.K << a.rep_log2;
    for (uint32_t w0 = 0; w0 < words; w0 += 64) {
        const uint32_t w = w0 + lane;
        uint32_t v = 0;
        if (w < words) {
            v = hist[w];
            hist[w] = 0u;
        }
        for (uint32_t o = 1; o <= rep_mask; o <<= 1) v += (uint32_t)__shfl_xor((int)v, (int)o, OI_WAVE);
        if (w < words && (lane & rep_mask) == 0u) fold[w >> a.rep_log2] = v;
    }
    lt_wave_sync();
    uint32_t *out = a.counts + (uint64_t)t * a.K;
    for (uint32_t c = lane; c < a.K; c += 64) {
        const uint32_t v = fold[c];
        if (!atomic) out[c] = v;
        else if (v != 0u) atomicAdd(out + c, v);
    }
    lt_wave_sync();
}

template <bool GATHER, bool WALK, bool SPLIT_ADDS>
__global__ __launch_bounds__(LT_THREADS) void lt_count_kernel(const LtArgs a) {
    constexpr uint32_t NW = LT_THREADS / 64;
    __shared__ uint32_t s_hist[NW][LT_HIST_WORDS], s_fold[NW][LT_HIST_WORDS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t *hist = s_hist[wave], *fold = s_fold[wave];
    for (uint32_t i = lane; i < LT_HIST_WORDS; i += 64) hist[i] = 0u;
    lt_wave_sync();
    // the start of term t's list, held inside the array (t == vocab: the end of the last list)
    auto start_of = [&](uint32_t t) -> uint32_t { return min(a.cell_start[(uint64_t)t * a.n_win], a.n_postings); };
    // a split piece [lo, hi): a quarter (in whole steps) per wave
    auto piece = [&](uint32_t t, uint32_t lo, uint32_t hi) {
        const uint32_t per = ((hi - lo + NW - 1u) / NW + 63u) & ~63u;
        const uint32_t wlo = min(lo + wave * per, hi), whi = min(wlo + per, hi);
        if (wlo < whi) lt_wave_term<GATHER, WALK>(a, t, wlo, whi, SPLIT_ADDS, hist, fold, lane);
    };
    for (uint32_t task = blockIdx.x; task < a.n_tasks; task += gridDim.x) {
        const uint64_t cut_lo = (uint64_t)task * LT_SPLIT_POSTINGS;
        const uint32_t cut_hi = (uint32_t)lt_min64(cut_lo + LT_SPLIT_POSTINGS, a.n_postings);
        const uint32_t t0 = min(a.first_term[task], a.vocab);
        uint32_t t1 = max(min(a.first_term[task + 1], a.vocab), t0);
        if (t0 > 0u) { // the term before the first: a split term that reaches into this cut
            const uint32_t s = start_of(t0 - 1u), e = max(start_of(t0), s);
            if (e - s >= LT_SPLIT_POSTINGS && (uint64_t)s < cut_lo && (uint64_t)e > cut_lo) piece(t0 - 1u, (uint32_t)cut_lo, min(e, cut_hi));
        }
        if (t1 > t0) { // the last term of the run: split if it is heavy (then no term behind it starts in this cut)
            const uint32_t s = start_of(t1 - 1u), e = max(start_of(t1), s);
            if (e - s >= LT_SPLIT_POSTINGS) {
                if ((uint64_t)s >= cut_lo && s < cut_hi) piece(t1 - 1u, s, min(e, cut_hi));
                --t1;
            }
        }
        // the light terms, in turn among the waves; a lane reads the bounds of one term of the wave's next LT_TERM_BATCH
        for (uint32_t tb = t0 + wave; tb < t1; tb += NW * LT_TERM_BATCH) {
            const uint32_t mine = tb + lane * NW;
            uint32_t s = 0, e = 0;
            if (mine < t1) {
                s = start_of(mine);
                e = max(start_of(mine + 1u), s);
            }
            const unsigned long long busy = __ballot(e > s && e - s < LT_SPLIT_POSTINGS); // (a heavy term here is an inconsistent plan: left out)
            for (unsigned long long m = busy; m != 0ull; m &= m - 1ull) {
                const uint32_t k = (uint32_t)__builtin_ctzll(m);
                lt_wave_term<GATHER, WALK>(a, tb + k * NW, (uint32_t)__shfl((int)s, (int)k), (uint32_t)__shfl((int)e, (int)k), false, hist, fold, lane);
            }
        }
    }
}

// sizes[c] += rows with labels[d] == c; zeroed by the launcher
__global__ __launch_bounds__(256) void lt_sizes_kernel(const uint32_t *__restrict__ labels, uint64_t n, uint32_t K, unsigned long long *__restrict__ sizes) {
    __shared__ uint32_t s_cnt[4][OI_MAX_CENTROIDS];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t *cnt = s_cnt[wave];
    for (uint32_t c = lane; c < K; c += 64) cnt[c] = 0u;
    lt_wave_sync();
    for (uint64_t i0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~(uint64_t)63; i0 < n; i0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = i0 + lane;
        const uint32_t l = i < n ? labels[i] : 0xFFFFFFFFu;
        const uint32_t l0 = (uint32_t)__shfl((int)l, 0);
        if (__all(l == l0)) { // one label on the step (wave-uniform): one add
            if (lane == 0u && l0 < K) cnt[l0] += 64u;
        } else if (l < K) {
            atomicAdd(&cnt[l], 1u);
        }
    }
    lt_wave_sync();
    for (uint32_t c = lane; c < K; c += 64)
        if (cnt[c] != 0u) atomicAdd(sizes + c, (unsigned long long)cnt[c]);
}

// ------------------------------------------------------------------ the ranked cut
struct LtSizes {
    uint64_t v[OI_MAX_CENTROIDS];
};
__global__ __launch_bounds__(256) void lt_put_sizes_kernel(const LtSizes s, uint32_t K, uint64_t *out) {
    if (threadIdx.x < K) out[threadIdx.x] = s.v[threadIdx.x];
}

__device__ __forceinline__ bool lt_better(uint64_t a1, uint64_t a2, uint64_t b1, uint64_t b2) { return a1 > b1 || (a1 == b1 && a2 > b2); }

// part[(slice * K + c) * top + r] = the r-th best entry of cluster c among the slice's terms, (0, 0) behind the last
__global__ __launch_bounds__(64) void lt_rank_kernel(const uint32_t *__restrict__ counts, const uint64_t *__restrict__ sizes, uint32_t vocab, uint32_t K,
                                                     uint32_t top, uint32_t min_df, ulonglong2 *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lt_smem[];
    uint64_t *l1 = reinterpret_cast<uint64_t *>(lt_smem), *l2 = l1 + (size_t)top * 64; // [top][64] each
    const uint32_t lane = threadIdx.x, slice = blockIdx.x, c = blockIdx.y * 64u + lane;
    const bool mine = c < K;
    const uint32_t chunks = (K + 63u) / 64u, need = max(min_df, 1u);
    uint64_t part_sum = 0;
    for (uint32_t j = lane; j < K; j += 64) part_sum += sizes[j];
    const uint64_t A = lt_wave_sum64(part_sum), size_c = mine ? sizes[c] : 0ull;
    uint32_t n = 0;
    const uint32_t t_begin = slice * LT_RANK_SLICE, t_end = (uint32_t)lt_min64((uint64_t)t_begin + LT_RANK_SLICE, vocab);
    for (uint32_t tb = t_begin; tb < t_end; tb += LT_RANK_UNROLL) {
        uint64_t sum[LT_RANK_UNROLL];
        uint32_t own[LT_RANK_UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < LT_RANK_UNROLL; ++u) {
            const uint32_t t = tb + u;
            sum[u] = 0;
            own[u] = 0;
            if (t < t_end) {
                const uint32_t *row = counts + (uint64_t)t * K;
                for (uint32_t j = 0; j < chunks; ++j)
                    if (j * 64u + lane < K) sum[u] += row[j * 64u + lane];
                if (mine) own[u] = row[c];
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < LT_RANK_UNROLL; ++u) sum[u] = lt_wave_sum64(sum[u]); // dfA, before the lanes part ways
#pragma unroll
        for (uint32_t u = 0; u < LT_RANK_UNROLL; ++u) {
            const uint32_t t = tb + u;
            const uint64_t dfa = sum[u];
            if (t >= t_end || !mine || own[u] < need) continue;
            const uint64_t k1 = ((uint64_t)own[u] * A - size_c * dfa) ^ 0x8000000000000000ull; // (two's complement: wraps for an inconsistent table)
            const uint64_t k2 = ((uint64_t)own[u] << 32) | (uint32_t)~t;
            if (n == top && !lt_better(k1, k2, l1[(n - 1u) * 64u + lane], l2[(n - 1u) * 64u + lane])) continue;
            uint32_t pos = n < top ? n++ : top - 1u;
            while (pos > 0u && lt_better(k1, k2, l1[(pos - 1u) * 64u + lane], l2[(pos - 1u) * 64u + lane])) {
                l1[pos * 64u + lane] = l1[(pos - 1u) * 64u + lane];
                l2[pos * 64u + lane] = l2[(pos - 1u) * 64u + lane];
                --pos;
            }
            l1[pos * 64u + lane] = k1;
            l2[pos * 64u + lane] = k2;
        }
    }
    if (!mine) return;
    ulonglong2 *o = part + ((uint64_t)slice * K + c) * top;
    for (uint32_t r = 0; r < top; ++r) o[r] = r < n ? make_ulonglong2(l1[r * 64u + lane], l2[r * 64u + lane]) : make_ulonglong2(0ull, 0ull);
}

// lists [blockIdx.x * LT_MERGE_FAN ..) of cluster blockIdx.y, one per lane, into one.  records == null: the list goes to
// out[(blockIdx.x * K + c) * top ..); else (the last round, one workgroup per cluster) it leaves as the call's records.
__global__ __launch_bounds__(64) void lt_merge_kernel(const ulonglong2 *__restrict__ in, uint32_t n_lists, uint32_t K, uint32_t top,
                                                      ulonglong2 *__restrict__ out, const uint32_t *__restrict__ counts,
                                                      oi_label_term *__restrict__ records, uint32_t *__restrict__ n_out) {
    __shared__ ulonglong2 s_win[OI_MAX_LABEL_TERMS];
    const uint32_t lane = threadIdx.x, c = blockIdx.y, li = blockIdx.x * LT_MERGE_FAN + lane;
    const ulonglong2 *list = in + ((uint64_t)(li < n_lists ? li : 0u) * K + c) * top;
    uint32_t head = 0, n = 0;
    uint64_t c1 = 0, c2 = 0; // the head of the lane's list; (0, 0): used up
    if (li < n_lists) {
        const ulonglong2 v = list[0];
        c1 = v.x;
        c2 = v.y;
    }
    for (; n < top; ++n) {
        uint64_t b1 = c1, b2 = c2;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t o1 = (uint64_t)__shfl_xor((unsigned long long)b1, o, OI_WAVE), o2 = (uint64_t)__shfl_xor((unsigned long long)b2, o, OI_WAVE);
            const bool take = lt_better(o1, o2, b1, b2);
            b1 = take ? o1 : b1;
            b2 = take ? o2 : b2;
        }
        const unsigned long long who = __ballot(c1 == b1 && c2 == b2 && c2 != 0ull);
        if (who == 0ull) break; // every list is used up (wave-uniform)
        if (lane == (uint32_t)__builtin_ctzll(who)) {
            s_win[n] = make_ulonglong2(c1, c2);
            ++head;
            c1 = c2 = 0ull;
            if (head < top) {
                const ulonglong2 v = list[head];
                c1 = v.x;
                c2 = v.y;
            }
        }
    }
    __syncthreads();
    if (!records) {
        ulonglong2 *o = out + ((uint64_t)blockIdx.x * K + c) * top;
        for (uint32_t r = lane; r < top; r += 64) {
            ulonglong2 v = make_ulonglong2(0ull, 0ull);
            if (r < n) v = s_win[r];
            o[r] = v;
        }
        return;
    }
    for (uint32_t r = lane; r < top; r += 64) {
        uint32_t term = 0xFFFFFFFFu, df_cluster = 0, df_assigned = 0;
        int64_t excess = 0;
        if (r < n) {
            const ulonglong2 k = s_win[r];
            term = ~(uint32_t)k.y;
            df_cluster = (uint32_t)(k.y >> 32);
            excess = (int64_t)(k.x ^ 0x8000000000000000ull);
            uint64_t dfa = 0;
            const uint32_t *row = counts + (uint64_t)term * K;
            for (uint32_t j = 0; j < K; ++j) dfa += row[j];
            df_assigned = (uint32_t)dfa;
        }
        oi_label_term *o = records + (uint64_t)c * top + r;
        o->term = term;
        o->df_cluster = df_cluster;
        o->df_assigned = df_assigned;
        o->reserved = 0u;
        o->excess = excess;
    }
    if (lane == 0u) n_out[c] = n;
}

// ------------------------------------------------------------------ host
// Device labels in, device table [vocab][n_clusters] and sizes [n_clusters] out (zeroed here); asynchronous on the ctx stream.
int oi_launch_label_term_counts(oi_index *idx, const uint32_t *d_labels, uint32_t K, uint32_t *d_counts, uint64_t *d_sizes) {
    oi_ctx *ctx = idx->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = idx->n_docs;
    ProfScope ps(ctx, "label_term_counts");
    OI_HIP_CHECK(hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * (size_t)idx->vocab * K, st));
    OI_HIP_CHECK(hipMemsetAsync(d_sizes, 0, sizeof(uint64_t) * (size_t)K, st));
    if (n == 0) return OI_OK;
    {
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->num_cus * 8);
        hipLaunchKernelGGL(lt_sizes_kernel, dim3(blocks), dim3(256), 0, st, d_labels, n, K, reinterpret_cast<unsigned long long *>(d_sizes));
        OI_HIP_CHECK(hipGetLastError());
    }
    if (idx->n_postings == 0 || idx->n_win == 0) return OI_OK;
    const uint32_t n_postings = (uint32_t)idx->n_postings, n_tasks = n_postings / LT_SPLIT_POSTINGS + 1u;
    DevBuf &plan = ctx->buf("label_terms_plan");
    OI_CHECK(plan.ensure(sizeof(uint32_t) * ((size_t)n_tasks + 1)));
    hipLaunchKernelGGL(lt_plan_kernel, dim3((n_tasks + 1 + 255) / 256), dim3(256), 0, st, idx->cell_start.as<uint32_t>(), idx->n_win, idx->vocab,
                       n_postings, n_tasks, plan.as<uint32_t>());
    OI_HIP_CHECK(hipGetLastError());
    uint32_t rep_log2 = 0;
    while (rep_log2 < 6 && (K << (rep_log2 + 1)) <= LT_HIST_WORDS) ++rep_log2;
    const LtArgs a = {idx->postings.as<uint2>(), idx->cell_start.as<uint32_t>(), plan.as<uint32_t>(), d_labels, n, n_postings, idx->vocab, idx->n_win,
                      K, rep_log2, n_tasks, d_counts};
    const uint32_t wgs = std::min<uint32_t>(n_tasks, (uint32_t)ctx->num_cus * 8);
#ifdef OI_ABLATION
    const char *abl = oi_ablation_env("OI_LT_ABLATE"); // "gather", "walk" or "adds": that part of the pass is left out
    if (abl && abl[0]) {
        if (abl[0] == 'g') hipLaunchKernelGGL((lt_count_kernel<false, true, true>), dim3(wgs), dim3(LT_THREADS), 0, st, a);
        else if (abl[0] == 'w') hipLaunchKernelGGL((lt_count_kernel<true, false, true>), dim3(wgs), dim3(LT_THREADS), 0, st, a);
        else hipLaunchKernelGGL((lt_count_kernel<true, true, false>), dim3(wgs), dim3(LT_THREADS), 0, st, a);
        OI_HIP_CHECK(hipGetLastError());
        return OI_OK;
    }
#endif
    hipLaunchKernelGGL((lt_count_kernel<true, true, true>), dim3(wgs), dim3(LT_THREADS), 0, st, a);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// what oi_launch_label_terms_rank needs behind `scratch`: the sizes, then the lists of the first level and of the merge rounds
size_t oi_label_terms_rank_scratch(uint32_t vocab, uint32_t K, uint32_t top) {
    const size_t n_slices = ((size_t)vocab + LT_RANK_SLICE - 1) / LT_RANK_SLICE, n_next = (n_slices + LT_MERGE_FAN - 1) / LT_MERGE_FAN;
    return sizeof(LtSizes) + sizeof(ulonglong2) * (n_slices + n_next) * K * top;
}

// Device table in, device records [n_clusters][top] and n [n_clusters] out; the sizes are the host's (sizes_host, passed by value)
// or, with sizes_host == null, the device's d_sizes.  Asynchronous on the ctx stream.
int oi_launch_label_terms_rank(oi_ctx *ctx, const uint32_t *d_counts, const uint64_t *sizes_host, const uint64_t *d_sizes, uint32_t vocab,
                               uint32_t K, uint32_t top, uint32_t min_df, void *scratch, oi_label_term *d_terms, uint32_t *d_n) {
    hipStream_t st = ctx->stream;
    ProfScope ps(ctx, "label_terms_rank");
    uint8_t *w = static_cast<uint8_t *>(scratch);
    if (sizes_host) {
        LtSizes s;
        memset(&s, 0, sizeof(s));
        memcpy(s.v, sizes_host, sizeof(uint64_t) * K);
        hipLaunchKernelGGL(lt_put_sizes_kernel, dim3(1), dim3(256), 0, st, s, K, reinterpret_cast<uint64_t *>(w));
        OI_HIP_CHECK(hipGetLastError());
        d_sizes = reinterpret_cast<const uint64_t *>(w);
    }
    uint32_t n_lists = (vocab + LT_RANK_SLICE - 1) / LT_RANK_SLICE;
    ulonglong2 *cur = reinterpret_cast<ulonglong2 *>(w + sizeof(LtSizes));
    ulonglong2 *nxt = cur + (size_t)n_lists * K * top;
    const size_t lds = sizeof(uint64_t) * 2 * 64 * (size_t)top;
    OI_CHECK(oi_dyn_lds(ctx, (const void *)lt_rank_kernel, sizeof(uint64_t) * 2 * 64 * (size_t)OI_MAX_LABEL_TERMS));
    hipLaunchKernelGGL(lt_rank_kernel, dim3(n_lists, (K + 63) / 64), dim3(64), lds, st, d_counts, d_sizes, vocab, K, top, min_df, cur);
    OI_HIP_CHECK(hipGetLastError());
    while (n_lists > LT_MERGE_FAN) { // (each round's output fits where the round before the last one wrote: it is at most 1/64 of it)
        const uint32_t n_out_lists = (n_lists + LT_MERGE_FAN - 1) / LT_MERGE_FAN;
        hipLaunchKernelGGL(lt_merge_kernel, dim3(n_out_lists, K), dim3(64), 0, st, cur, n_lists, K, top, nxt, d_counts, (oi_label_term *)nullptr,
                           (uint32_t *)nullptr);
        OI_HIP_CHECK(hipGetLastError());
        std::swap(cur, nxt);
        n_lists = n_out_lists;
    }
    hipLaunchKernelGGL(lt_merge_kernel, dim3(1, K), dim3(64), 0, st, cur, n_lists, K, top, (ulonglong2 *)nullptr, d_counts, d_terms, d_n);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}
