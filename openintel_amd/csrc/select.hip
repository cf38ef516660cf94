// select.hip -- candidate-pool top-k selection, list merge and reciprocal-rank fusion.
//
// Every ranked list in this library is a set of 64-bit rank keys
//   key = orderable(score) << 32 | ~doc_id        (oi_device.h)
// so "score descending, doc id ascending" is plain descending u64 order and keys of
// distinct docs are distinct.  One workgroup (1024 threads = 16 waves) owns one query.
//
// select_flat_kernel (the pool as one flat array: every product launch) runs sel_flat_select<KPT>, a sequence of stages
// over a key holder (SelKeys<KPT>: registers, or re-loading for KPT == 0):
//   sel_take_all      n <= k: everything
//   sel_margin_bins   margin mode: two 11-bit passes, verdict mask, direct carry write, the prediction
//   sel_sampled_cut   pools above SEL_CAND keys: a sampled threshold, then the select over the cut
//   sel_exact         the exact radix select over the whole pool
//   sel_margin_exact  margin mode behind an exact select: everything within eps2 of the k-th score
// and ends in sel_finish (sorted output / smallest key, compaction, threshold raise) or, for a margin result, in
// sel_finish_margin.  select_topk_kernel (more than SEL_MAX_SEGS segments, OI_SELECT_V1) puts a segment walk or an LDS
// gather in front of the same sel_threshold and sel_finish.  Then lists_to_pool_kernel and rrf_kernel.
#include "oi_device.h"
#include "oi_internal.h"

#define SEL_THREADS 1024
#define SEL_MAX_SEGS 4096
#ifdef OI_ABLATION
// OI_SELECT_STAMPS=1 (ablation builds): query 0's thread 0 prints where a select_flat launch spends its cycles
__device__ int sel_dbg_on;
__device__ unsigned long long sel_dbg_t[16];
#define SEL_STAMP(i) do { if (sel_dbg_on && blockIdx.x == 0 && threadIdx.x == 0) sel_dbg_t[i] = __builtin_readcyclecounter(); } while (0)
#else
#define SEL_STAMP(i) do { } while (0)
#endif
#ifdef OI_ABLATION
#define SEL_RANK_SELFCHECK 1 // (sel_rank_bin2k: OI_SELECT_STAMPS=2 checks it against the plain walk)
#endif
#include "oi_select_rank.h"

#define SEL_MAX 1024  // == OI_MAX_DEPTH

// One select launch: the pools (PoolView), the request, the optional behaviour (SelectExtra; its margin-mode members are
// null / 0 outside margin mode).  oi_launch_select fills it once; both kernels take it by value.
struct SelArgs {
    uint64_t *pools;
    uint32_t *carry_cnt, *seg_cnt, *tau_keys, *overflow;
    uint64_t pool_stride;
    uint32_t carry_cap, seg_cap, n_segs, seg_cnt_stride, k, out_stride;
    int compact;
    float *out_scores;
    uint32_t *out_docs, *out_counts;
    const float *eps2, *row_meta, *row_qn, *row_cq;
    const uint32_t *run_gate, *skip;
    uint32_t *margin_gate, *spec_tau, *spec_max;
    uint64_t *cand;
    uint32_t skip_base, cand_cap, meta_base, spec_rank;
};

// In-LDS bitonic sort, descending, P a power of two <= 2048, all SEL_THREADS threads call.
__device__ void bitonic_sort_desc(uint64_t *a, uint32_t P) {
    const uint32_t tid = threadIdx.x;
    for (uint32_t size = 2; size <= P; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t t = tid; t < (P >> 1); t += SEL_THREADS) {
                uint32_t lo = 2 * t - (t & (stride - 1));
                uint32_t hi = lo + stride;
                bool desc = ((lo & size) == 0);
                uint64_t x = a[lo], y = a[hi];
                if ((x < y) == desc) { a[lo] = y; a[hi] = x; }
            }
            __syncthreads();
        }
    }
}

#define SEL_KPT_MAX 32
#define SEL_CAND 4096

// Per-row margins of a margin select (the int8 screening tier, cosine_screen_i8.hip): keys are LOWER bounds l_r of rows whose upper
// bound is l_r + 2 (e_r qn + cq); a key passing the global margin (eps2 = the largest such width) is kept only when its own upper
// bound reaches the k-th key, less a guard for the f32 rounding of the test.  meta: {scale, e_r} per row (row = doc - base);
// null: no row margins.
struct SelRowMargin {
    const float *meta;
    uint32_t base;
    float qn, cq;
};
// (the gather and the test apart: the fast margin path issues a group of gathers before it evaluates any)
__device__ __forceinline__ float sel_row_e(const SelRowMargin &rm, uint64_t kv) {
    return rm.meta[2 * (uint64_t)(oi_rank_key_doc(kv) - rm.base) + 1];
}
__device__ __forceinline__ bool sel_row_test(const SelRowMargin &rm, uint64_t kv, float e, float edge, float eps2) {
    const float u = oi_rank_key_score(kv) + 2.002f * (e * rm.qn + rm.cq);
    return u >= edge - 9.5367431640625e-07f * (fabsf(edge) + eps2);
}
__device__ __forceinline__ bool sel_row_keep(const SelRowMargin &rm, uint64_t kv, float edge, float eps2) {
    if (!rm.meta) return true;
    return sel_row_test(rm, kv, sel_row_e(rm, kv), edge, eps2);
}

// hist[digit] += 1 for the active lanes; the two most common digits of the wave go in as one atomic each
__device__ __forceinline__ void sel_hist_add(uint32_t *hist, bool active, uint32_t digit) {
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

// wave-aggregated append of the lanes' keys to dst; *count counts every taken key, stored or not
__device__ __forceinline__ void sel_append(uint64_t *dst, uint32_t *count, uint32_t cap, bool take, uint64_t key) {
    const unsigned long long m = __ballot(take);
    if (!m) return;
    const uint32_t lane = threadIdx.x & 63, leader = (uint32_t)__builtin_ctzll(m);
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, (int)leader, OI_WAVE);
    const uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    if (take && pos < cap) dst[pos] = key;
}

// The smallest of a[0..m) into *min_key (an LDS word, ~0 or a larger candidate on entry; readable after the next barrier).
__device__ __forceinline__ void sel_min_key(const uint64_t *a, uint32_t m, unsigned long long *min_key) {
    unsigned long long lo = ~0ull;
    for (uint32_t i = threadIdx.x; i < m; i += SEL_THREADS) lo = a[i] < lo ? a[i] : lo;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long v = __shfl_xor(lo, o, OI_WAVE);
        lo = v < lo ? v : lo;
    }
    if ((threadIdx.x & 63) == 0 && lo != ~0ull) atomicMin(min_key, lo);
}

// Radix select over the keys `for_each` enumerates (f(valid, key), same keys on every call, wave-uniform trip counts: f
// ballots): finds (shift, prefix) such that exactly kk of them have (key >> shift) >= prefix.  Needs kk <= their number,
// distinct keys; all threads call.  Reads nothing of rx, leaves nothing in it.
template <class FE>
__device__ __forceinline__ void sel_threshold(FE &&for_each, uint32_t kk_in, SelRadix &rx, int &shift_out, uint64_t &prefix_out) {
    const uint32_t tid = threadIdx.x;
    if (tid == 0) { rx.prefix = 0; rx.kk = kk_in; }
    int shift = 56;
    for (;; shift -= 8) {
        if (tid < 256) rx.hist[tid] = 0;
        __syncthreads();
        const uint64_t prefix = rx.prefix;
        const bool top = shift == 56;
        for_each([&](bool valid, uint64_t kv) {
            sel_hist_add(rx.hist, valid && (top || (kv >> ((shift + 8) & 63)) == prefix), (uint32_t)(kv >> shift) & 255u);
        });
        __syncthreads();
        if (tid < 64) { // wave 0: the digit holding the kk-th key counted from the top
            const uint32_t kk = rx.kk;
            uint32_t mine = 0;
            for (int i = 0; i < 4; ++i) mine += rx.hist[255 - (tid * 4 + i)];
            uint32_t incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = __shfl_up(incl, o, OI_WAVE);
                if ((int)tid >= o) incl += v;
            }
            const unsigned long long ball = __ballot(incl >= kk);
            const uint32_t owner = ball ? (uint32_t)__builtin_ctzll(ball) : 63u;
            if (tid == owner) {
                uint32_t cum = incl - mine;
                int d = 255 - (int)(tid * 4);
                for (int i = 0; i < 3; ++i, --d) {
                    const uint32_t c = rx.hist[d];
                    if (cum + c >= kk) break;
                    cum += c;
                }
                rx.prefix = (prefix << 8) | (uint64_t)d;
                rx.kk = kk - cum;
                rx.bin_cnt = rx.hist[d];
            }
        }
        __syncthreads();
        if (rx.bin_cnt == 1 || shift == 0) break;
    }
    shift_out = shift;
    prefix_out = rx.prefix;
    __syncthreads(); // rx.prefix / rx.kk may be rewritten by the next call
}

// ... of the array a[0..m), m >= r
__device__ __forceinline__ uint32_t sel_rth_score_key_of(const uint64_t *a, uint32_t m, uint32_t r, SelShared &sh) {
    const uint32_t tid = threadIdx.x;
    return sel_rth_score_key([&](auto &&f) {
        for (uint32_t i0 = 0; i0 < m; i0 += SEL_THREADS) f(i0 + tid < m, a[i0 + tid < m ? i0 + tid : 0]);
    }, r, sh);
}

// The tail of both kernels.  Reads sel[0..m), the selected set (LDS, barrier passed), and *min_key (LDS, ~0).  Sorted output is
// needed only for a final list (a.out_scores); an intermediate compaction just needs the set and its smallest key, left in
// *min_key.  a.compact: the pool is rewritten as carry = the selected keys, all segments empty, and the threshold raised to the
// k-th score, so the next corpus chunk appends after them.  All threads call; returns past a barrier.
__device__ __forceinline__ void sel_finish(const SelArgs &a, uint32_t q, uint64_t *pool, uint32_t *segc, uint64_t *sel, uint32_t m,
                                           unsigned long long *min_key) {
    const uint32_t tid = threadIdx.x;
    if (a.out_scores) {
        uint32_t P = 2;
        while (P < m) P <<= 1;
        for (uint32_t i = m + tid; i < P; i += SEL_THREADS) sel[i] = 0; // lowest possible key
        __syncthreads();
        bitonic_sort_desc(sel, P);
        for (uint32_t i = tid; i < m; i += SEL_THREADS) {
            const uint64_t key = sel[i];
            a.out_scores[(uint64_t)q * a.out_stride + i] = oi_rank_key_score(key);
            a.out_docs[(uint64_t)q * a.out_stride + i] = oi_rank_key_doc(key);
        }
        if (tid == 0) { a.out_counts[q] = m; *min_key = m ? sel[m - 1] : 0; }
    } else {
        sel_min_key(sel, m, min_key);
    }
    __syncthreads();
    if (a.compact) {
        for (uint32_t i = tid; i < m; i += SEL_THREADS) pool[i] = sel[i];
        for (uint32_t sg = tid; sg < a.n_segs; sg += SEL_THREADS) segc[sg] = 0;
        if (tid == 0) {
            a.carry_cnt[q] = m;
            if (m == a.k && a.tau_keys && !a.eps2) { // k docs at or above this score exist: a valid lower bound of the final
                // k-th, so later chunks may drop anything strictly below it (a margin-mode pool of exactly k keys keeps its
                // threshold: that bound needs the margin)
                const uint32_t t = (uint32_t)(*min_key >> 32);
                if (t > a.tau_keys[q]) a.tau_keys[q] = t;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// select_flat_kernel: the selection with the pool seen as ONE flat array.
//
// select_topk_kernel (below) walks the pool a segment at a time (one wave per segment: a dependent count -> keys
// load chain per segment, repeated on every radix pass when the pool does not fit its LDS copy); with the
// 256 short segments a cosine chunk leaves behind, that chain IS the select (40-120 us per launch, on the
// critical path between two corpus chunks).  Here
//   * the segment counts are scanned once into LDS offsets; flat index -> (segment, slot) is one binary
//     search per lane and then a forward walk, because wave w owns the contiguous flat range
//     [w*kpt*64, (w+1)*kpt*64) and reads it 64 consecutive keys per load (coalesced, all loads in flight);
//   * the keys then live in REGISTERS (<= 32 per thread: pools up to 32K keys) for everything that follows;
//     larger pools re-load through the same flat view on every pass;
//   * pools above 4K keys are cut down first: the threshold that keeps ~2k keys is read off a 1024-key
//     sample (radix select over one key per thread), one filter pass moves the survivors to LDS, and the
//     exact selection runs over those.  A sample that keeps fewer than k or more than 4096 keys falls back
//     to the exact passes over the whole pool: the RESULT never depends on the sample;
//   * histogram and append atomics are aggregated per wave first (the leading digits of a pool of
//     near-threshold scores are nearly all equal, i.e. one LDS address).
struct SelFlat {
    const uint64_t *pool;
    const uint32_t *seg_off; // LDS, n_segs + 1 entries, seg_off[n_segs] = keys in segments
    uint32_t n, c0, carry_cap, seg_cap, n_segs, steps;
};
// A lane's position in the flat view: segment sg holds the segment-relative flat indices [lo, hi).
struct SelCursor {
    uint32_t sg, lo, hi;
};
// flat index i < n  ->  cursor at its segment (binary search; indices inside the carry region map to e = 0)
__device__ __forceinline__ SelCursor sel_seek(const SelFlat &K, uint32_t i) {
    const uint32_t e = i < K.c0 ? 0u : i - K.c0;
    uint32_t lo = 0, hi = K.n_segs; // seg_off[lo] <= e < seg_off[hi]
    for (uint32_t s = 0; s < K.steps; ++s) {
        const uint32_t mid = (lo + hi) >> 1;
        const bool up = K.seg_off[mid] <= e;
        lo = up ? mid : lo;
        hi = up ? hi : mid;
    }
    SelCursor c;
    c.sg = lo; c.lo = K.seg_off[lo]; c.hi = K.seg_off[lo + 1];
    return c;
}
// pool offset of flat index i < n, i >= every index this cursor was used for before (forward walk)
__device__ __forceinline__ uint64_t sel_at(const SelFlat &K, SelCursor &c, uint32_t i) {
    if (i < K.c0) return i;
    const uint32_t e = i - K.c0;
    while (e >= c.hi) { // e < seg_off[n_segs]: stops at the segment that holds e (skips empty ones)
        ++c.sg;
        c.lo = c.hi;
        c.hi = K.seg_off[c.sg + 1];
    }
    return (uint64_t)K.carry_cap + (uint64_t)c.sg * K.seg_cap + (e - c.lo);
}

// Margin mode of one query (eps2 >= 0; the bf16 screen of cosine_prefilter.hip, the int8 tier): the result is not the top k but
// EVERY key whose score is within eps2 of the k-th largest score -- the set that must survive for the exact top k to be inside it.
struct SelMargin {
    float eps2;           // < 0: not a margin select; +inf: a query without a bound (keeps everything, raises nothing)
    // the screen's two-class margin: keys of docs marked in this bitmap (bit doc - skip_base) do not take part -- they are scored
    // exactly whatever happens here, and their screen scores must not move the threshold (cosine_prefilter.hip).  Null: none
    const uint32_t *skip;
    uint32_t skip_base;
    uint64_t *cand;       // the survivors' staging buffer (LDS, or the caller's global one) of `cap` keys
    uint32_t cap;
    uint64_t *carry;      // this query's carry region: sel_margin_bins with the keys in registers writes the survivors there
    uint32_t spec_rank;   // r > 0: the prediction, the r-th largest score key among the survivors kept (sel_rth_score_key)
    SelRowMargin rows;    // meta == nullptr: none (also when eps2 is +inf)
};
// What a select leaves: m keys in sel[], or -- in_cand, margin mode -- m survivors (at most M.cap; overflow: there were more,
// the caller opens the exact pipeline) in M.cand, or in M.carry already (in_carry), tau = the orderable key of (k-th score -
// eps2), the next chunk's threshold, and spec_key = the prediction where the stage already made it.
struct SelResult {
    uint32_t m;
    bool in_cand, overflow, in_carry;
    uint32_t tau, spec_key;
};
// ... of a margin stage that counted c survivors into a buffer of cap keys
__device__ __forceinline__ SelResult sel_margin_result(uint32_t c, uint32_t cap, uint32_t tau, bool in_carry) {
    return SelResult{c > cap ? cap : c, true, c > cap, in_carry, tau, 0u};
}

// The keys of a thread.  KPT > 0: they live in registers (n <= KPT * SEL_THREADS), key[j] = flat index first + 64 j, dead bit j =
// key[j] is a skipped doc's; KPT == 0: for_each re-loads them through the flat view on every pass.  kpt = keys per thread; wave
// w owns [w*kpt*64, (w+1)*kpt*64).  for_each(f) calls f(valid, key) kpt times (wave-uniform; 4-rounded for KPT == 0).
template <int KPT>
struct SelKeys {
    static constexpr int NR = KPT > 0 ? KPT : 1;
    const SelFlat &K;
    const uint32_t *const skip;
    const uint32_t skip_base;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = K.n;
    const uint32_t kpt = (n + SEL_THREADS - 1) / SEL_THREADS;
    const uint32_t first = wv * kpt * 64 + lane, last = n - 1;
    uint64_t key[NR];
    uint32_t dead = 0;

    __device__ __forceinline__ SelKeys(const SelFlat &K_, const SelMargin &M) : K(K_), skip(M.skip), skip_base(M.skip_base) {}
    __device__ __forceinline__ bool skipped(uint64_t kv) const {
        const uint32_t d = oi_rank_key_doc(kv) - skip_base;
        return (skip[d >> 5] >> (d & 31u)) & 1u;
    }
    // key[j] is a key of the pool (j < kpt) and takes part
    __device__ __forceinline__ bool live(int j) const { return first + (uint32_t)j * 64 < n && !((dead >> j) & 1u); }
    __device__ __forceinline__ void load() { // n > 0
        if constexpr (KPT > 0) {
            SelCursor cur = sel_seek(K, first < n ? first : last);
            uint64_t at = sel_at(K, cur, first < n ? first : last);
#pragma unroll
            for (int j = 0; j < KPT; ++j) { // loads unpredicated (a slot past the end re-reads the previous key): all in flight
                const uint32_t i = first + (uint32_t)j * 64;
                if ((uint32_t)j < kpt && i < n) at = sel_at(K, cur, i); // the cursor only walks forward
                key[j] = K.pool[at];
            }
            if (skip) {
#pragma unroll
                for (int j = 0; j < KPT; ++j)
                    if ((uint32_t)j < kpt && first + (uint32_t)j * 64 < n && skipped(key[j])) dead |= 1u << j;
            }
        }
    }
    template <class F>
    __device__ __forceinline__ void for_each(F &&f) const {
        if constexpr (KPT > 0) {
#pragma unroll
            for (int j = 0; j < KPT; ++j)
                if ((uint32_t)j < kpt) f(live(j), key[j]); // uniform guard
        } else {
            SelCursor cur = sel_seek(K, first < n ? first : last);
            uint64_t at = sel_at(K, cur, first < n ? first : last);
            for (uint32_t j0 = 0; j0 < kpt; j0 += 4) { // four loads in flight per thread
                uint64_t kx[4];
                bool ok[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t i = first + (j0 + u) * 64;
                    ok[u] = j0 + u < kpt && i < n;
                    if (ok[u]) at = sel_at(K, cur, i);
                    kx[u] = K.pool[at];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) f(ok[u] && !(skip && skipped(kx[u])), kx[u]);
            }
        }
    }
};

// ---- stage: take-all (n <= k).  Leaves every live key in sel[], sh.cnt = their number (0 on entry); returns it.
template <int KPT>
__device__ __forceinline__ uint32_t sel_take_all(const SelKeys<KPT> &H, SelShared &sh, uint64_t *sel) {
    H.for_each([&](bool valid, uint64_t kv) { sel_append(sel, &sh.cnt, 2 * SEL_MAX, valid, kv); });
    __syncthreads();
    return H.skip ? sh.cnt : H.n; // (skipped keys were not appended)
}

// ---- stage: margin bins, the fast path of margin mode.  What the next chunk and the rescoring need is ANY lower bound tau' of the
// k-th largest screen score and every key within eps2 of tau' -- not the k-th key itself.  Two passes of 11-bit digits
// over the valid keys find the 22-bit bin (sign, exponent, 13 bits of mantissa) that holds the k-th largest; its LOWER
// EDGE is tau': at least k keys are >= it, and it is below the k-th score by < 2^-13 of its size, ~1e-5 where the margin
// is ~4e-3, so the survivor set grows by a fraction of a percent.  (The exact stages: a 1024-key sample, 4-7 passes of
// 8-bit digits over the sample, a cut, 4-7 more over the cut, the k-th key, then the margin filter -- 25-30 us per launch
// between two corpus chunks; this one: two histogram passes and the filter.)
// Uses sh.hist2k and sh.rx (free on entry and on return); sh.cnt (0 on entry) = the survivors on return.  Fewer than k valid
// keys: in_cand stays false, nothing but hist2k / rx was touched, and the exact stages follow.
template <int KPT>
__device__ __forceinline__ SelResult sel_margin_bins(const SelKeys<KPT> &H, uint32_t k, const SelMargin &M, SelShared &sh) {
    const uint32_t tid = H.tid, lane = H.lane, kpt = H.kpt;
    const float eps2 = M.eps2;
    SelResult R = {};
    uint32_t kk = k, pfx = 0;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int shift = 53 - 11 * pass;
        sh.hist2k[tid] = 0;
        sh.hist2k[tid + SEL_THREADS] = 0;
        __syncthreads();
        if (pass == 0) {
            sel_hist_leading([&](auto &&f) { H.for_each(f); }, sh);
        } else { // 11 bits of mantissa inside one leading bin: spread over the 2048 addresses, plain atomics
            H.for_each([&](bool valid, uint64_t kv) {
                if (valid && (uint32_t)(kv >> 53) == pfx) atomicAdd(&sh.hist2k[(uint32_t)(kv >> shift) & 2047u], 1u);
            });
        }
        __syncthreads();
        sel_rank_bin2k(sh, kk, pass);
        const bool enough = sh.rx.bin_cnt != 0xFFFFFFFFu;
        const uint32_t d = (uint32_t)sh.rx.prefix;
        kk = sh.rx.kk;
        __syncthreads(); // (sh.rx's words are rewritten by the next pass or the exact stages)
        if (!enough) return R;
        if (pass == 0) pfx = d;
        else pfx = (pfx << 11) | d;
        SEL_STAMP(3 + pass);
    }
    uint32_t tkey = pfx << 10; // the bin's lower edge as a 32-bit score key
    tkey = tkey < 0x007FFFFFu ? 0x007FFFFFu : tkey; // (below key(-inf) the bit pattern is a NaN's: -inf instead)
    const uint32_t t32 = eps2 < __builtin_inff() ? oi_f32_key(oi_key_f32(tkey) - eps2) : 0u;
    // the filter: a thread counts its survivors, the wave takes ONE slot range for all of them
    uint32_t mine = 0;
    const float edge = oi_key_f32(tkey);
    auto keep = [&](bool valid, uint64_t kv) { return valid && (uint32_t)(kv >> 32) >= t32 && sel_row_keep(M.rows, kv, edge, eps2); };
    uint32_t verdict = 0; // KPT > 0, bit j: key[j] survives -- each key is tested ONCE, the storing pass reads the mask
    if constexpr (KPT > 0) {
#pragma unroll
        for (int j = 0; j < KPT; ++j) // the cheap global test first
            if ((uint32_t)j < kpt && H.live(j) && (uint32_t)(H.key[j] >> 32) >= t32) verdict |= 1u << j;
        if (M.rows.meta) { // the row test: the gathers of a group of keys that passed are issued together, then evaluated
            constexpr int G = KPT < 8 ? KPT : 8;
#pragma unroll
            for (int j0 = 0; j0 < KPT; j0 += G) {
                if ((uint32_t)j0 < kpt) { // (uniform)
                    float e[G];
#pragma unroll
                    for (int u = 0; u < G; ++u) e[u] = (verdict >> (j0 + u)) & 1u ? sel_row_e(M.rows, H.key[j0 + u]) : 0.f;
#pragma unroll
                    for (int u = 0; u < G; ++u)
                        if (((verdict >> (j0 + u)) & 1u) && !sel_row_test(M.rows, H.key[j0 + u], e[u], edge, eps2)) verdict &= ~(1u << (j0 + u));
                }
            }
        }
        mine = (uint32_t)__popc(verdict);
    } else {
        H.for_each([&](bool valid, uint64_t kv) { mine += keep(valid, kv) ? 1u : 0u; });
    }
    const uint32_t incl = oi_wave_incl_scan(mine);
    const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    uint32_t base = 0;
    if (lane == 0 && tot) base = atomicAdd(&sh.cnt, tot);
    uint32_t pos = (uint32_t)__builtin_amdgcn_readfirstlane((int)base) + incl - mine;
    uint32_t stored = 0; // KPT > 0, bit j: key[j] went into the carry region (all of verdict unless the survivors overflow it)
    if constexpr (KPT > 0) { // every key of the pool has been in registers since before the first barrier: straight to the carry region
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            if ((verdict >> j) & 1u) {
                if (pos < M.cap) { M.carry[pos] = H.key[j]; stored |= 1u << j; }
                ++pos;
            }
        }
    } else {
        H.for_each([&](bool valid, uint64_t kv) {
            if (keep(valid, kv)) {
                if (pos < M.cap) M.cand[pos] = kv;
                ++pos;
            }
        });
    }
    __syncthreads();
    R = sel_margin_result(sh.cnt, M.cap, t32, KPT > 0);
    SEL_STAMP(5);
    if constexpr (KPT > 0) {
        if (M.spec_rank && R.m >= M.spec_rank) // (uniform) the prediction, over the keys that were stored
            R.spec_key = sel_rth_score_key([&](auto &&f) {
#pragma unroll
                for (int j = 0; j < KPT; ++j)
                    if ((uint32_t)j < kpt) f((stored >> j) & 1u, H.key[j]);
            }, M.spec_rank, sh);
    }
    return R;
}

// ---- stage: sampled cut (pools above SEL_CAND keys).  One key per thread, spread over the wave's range, is the sample; the
// threshold that keeps ~2k keys is read off it and the keys above it go to cand[] (LDS).  True: the cut held between k and
// SEL_CAND keys and sel[0..k) is the top k, sh.cnt = k.  False: the sample misjudged the pool, sh.cnt = 0 as on entry, cand[]
// is garbage, and sel_exact follows.  Uses sh.rx and sh.n_samples.
template <int KPT>
__device__ __forceinline__ bool sel_sampled_cut(const SelKeys<KPT> &H, uint32_t k, SelShared &sh, uint64_t *sel, uint64_t *cand) {
    const uint32_t tid = H.tid, lane = H.lane, kpt = H.kpt, first = H.first, last = H.last, n = H.n;
    int shift;
    uint64_t prefix;
    const uint32_t js = lane % kpt, is = first + js * 64;
    bool sv = is < n;
    uint64_t sk;
    if constexpr (KPT > 0) {
        sk = H.key[0];
#pragma unroll
        for (int j = 1; j < KPT; ++j) sk = (uint32_t)j == js ? H.key[j] : sk;
        sv = sv && !((H.dead >> js) & 1u);
    } else {
        SelCursor cur = sel_seek(H.K, sv ? is : last);
        sk = H.K.pool[sel_at(H.K, cur, sv ? is : last)];
        sv = sv && !(H.skip && H.skipped(sk));
    }
    if (tid == 0) sh.n_samples = 0;
    __syncthreads();
    {
        const unsigned long long m = __ballot(sv);
        if (lane == 0 && m) atomicAdd(&sh.n_samples, (uint32_t)__popcll(m));
    }
    __syncthreads();
    const uint32_t ns = sh.n_samples;
    uint32_t r = (uint32_t)(((uint64_t)ns * (2 * k) + n - 1) / n) + 1; // keeps ~2k keys (+1 sample of margin)
    r = r > ns ? ns : r;
    sel_threshold([&](auto &&f) { f(sv, sk); }, r, sh.rx, shift, prefix);
    H.for_each([&](bool valid, uint64_t kv) { sel_append(cand, &sh.cnt, SEL_CAND, valid && (kv >> shift) >= prefix, kv); });
    __syncthreads();
    const uint32_t c = sh.cnt;
    __syncthreads();
    if (tid == 0) sh.cnt = 0;
    __syncthreads();
    if (c >= k && c <= SEL_CAND) { // the top k of the pool are the top k of cand[0..c)
        uint64_t ck[SEL_CAND / SEL_THREADS];
#pragma unroll
        for (int j = 0; j < SEL_CAND / SEL_THREADS; ++j) {
            const uint32_t i = (uint32_t)j * SEL_THREADS + tid;
            ck[j] = cand[i < c ? i : c - 1];
        }
        auto cand_each = [&](auto &&f) {
#pragma unroll
            for (int j = 0; j < SEL_CAND / SEL_THREADS; ++j)
                if ((uint32_t)j * SEL_THREADS < c) f((uint32_t)j * SEL_THREADS + tid < c, ck[j]);
        };
        if (c == k) { // nothing to select
            cand_each([&](bool valid, uint64_t kv) { sel_append(sel, &sh.cnt, SEL_MAX, valid, kv); });
        } else {
            sel_threshold(cand_each, k, sh.rx, shift, prefix);
            cand_each([&](bool valid, uint64_t kv) { sel_append(sel, &sh.cnt, SEL_MAX, valid && (kv >> shift) >= prefix, kv); });
        }
        __syncthreads();
        return true;
    }
    return false;
}

// ---- stage: exact select (n > k).  Radix select over every live key; sel[] takes the keys at or above the k-th, sh.cnt (0 on
// entry) their number: k, or all of them when fewer than k are live.  Uses sh.rx.
template <int KPT>
__device__ __forceinline__ void sel_exact(const SelKeys<KPT> &H, uint32_t k, SelShared &sh, uint64_t *sel) {
    int shift;
    uint64_t prefix;
    sel_threshold([&](auto &&f) { H.for_each(f); }, k, sh.rx, shift, prefix);
    // every key whose top bits are >= prefix is selected: exactly k of them (keys are distinct)
    H.for_each([&](bool valid, uint64_t kv) { sel_append(sel, &sh.cnt, SEL_MAX, valid && (kv >> shift) >= prefix, kv); });
    __syncthreads();
}

// ---- stage: exact margin filter, margin mode behind an exact select.  sel[0..k) is the top k (barrier passed), sh.min_key is ~0:
// the k-th key is the smallest selected one; everything within eps2 of its score goes to M.cand, sh.cnt = their number.
template <int KPT>
__device__ __forceinline__ SelResult sel_margin_exact(const SelKeys<KPT> &H, uint32_t k, const SelMargin &M, SelShared &sh, const uint64_t *sel) {
    const float eps2 = M.eps2;
    __syncthreads(); // everyone has read sh.cnt before it is reset below
    sel_min_key(sel, k, &sh.min_key);
    if (H.tid == 0) sh.cnt = 0;
    __syncthreads();
    // an infinite margin (a query without a bound, cosine_prefilter.hip) keeps everything and never raises the threshold
    const uint32_t t32 = eps2 < __builtin_inff() ? oi_f32_key(oi_key_f32((uint32_t)(sh.min_key >> 32)) - eps2) : 0u;
    const float edge = oi_key_f32((uint32_t)(sh.min_key >> 32));
    H.for_each([&](bool valid, uint64_t kv) {
        sel_append(M.cand, &sh.cnt, M.cap, valid && (uint32_t)(kv >> 32) >= t32 && sel_row_keep(M.rows, kv, edge, eps2), kv);
    });
    __syncthreads();
    return sel_margin_result(sh.cnt, M.cap, t32, false);
}

// Selects the top min(n, k) keys of K into sel[] (R.m of them), or in margin mode the survivors (R.in_cand, see SelResult).
// sh.cnt == 0 and sh.min_key == ~0 on entry; cand: SEL_CAND keys of LDS for the sampled cut.
template <int KPT>
__device__ __forceinline__ SelResult sel_flat_select(const SelFlat &K, uint32_t k, const SelMargin &M, SelShared &sh, uint64_t *sel, uint64_t *cand) {
    SelResult R = {};
    const uint32_t n = K.n;
    if (n == 0) return R;
    SelKeys<KPT> H(K, M);
    H.load();
    if (n <= k) return SelResult{sel_take_all(H, sh, sel)};
    SEL_STAMP(2);
    if (M.eps2 >= 0.f) {
        R = sel_margin_bins(H, k, M, sh);
        if (R.in_cand) return R;
    }
    bool selected = false; // sel[0..k) holds the top k
    if (KPT != 4 && n > SEL_CAND) selected = sel_sampled_cut(H, k, sh, sel, cand);
    if (!selected) sel_exact(H, k, sh, sel);
    R.m = sh.cnt < k ? sh.cnt : k;
    if (!(M.eps2 >= 0.f) || R.m < k) return R;
    return sel_margin_exact(H, k, M, sh, sel);
}

// The register class of a pool of n keys: f(SelClass<KPT>), KPT = 0 for the re-loading class.
template <int KPT> struct SelClass { static constexpr int value = KPT; };
template <class F>
__device__ __forceinline__ SelResult sel_dispatch(uint32_t n, F &&f) {
    if (n <= 4 * SEL_THREADS) return f(SelClass<4>{});
    if (n <= 8 * SEL_THREADS) return f(SelClass<8>{});
    if (n <= 16 * SEL_THREADS) return f(SelClass<16>{});
    if (n <= SEL_KPT_MAX * SEL_THREADS) return f(SelClass<SEL_KPT_MAX>{});
    return f(SelClass<0>{});
}

// The tail of a margin select: R.m survivors, an unsorted superset of the top k, only ever compacted -- into the carry region
// (unless the stage wrote them there), all segments empty, the threshold raised to R.tau, the gate opened on overflow, and with
// a.spec_rank the speculative threshold's words.  All threads call.
__device__ __forceinline__ void sel_finish_margin(const SelArgs &a, uint32_t q, uint64_t *pool, uint32_t *segc, const SelMargin &M,
                                                  const SelResult &R, SelShared &sh) {
    const uint32_t tid = threadIdx.x, m = R.m;
    if (R.overflow && tid == 0 && a.margin_gate) *a.margin_gate = 1u;
    if (!R.in_carry)
        for (uint32_t i = tid; i < m; i += SEL_THREADS) pool[i] = M.cand[i];
    for (uint32_t sg = tid; sg < a.n_segs; sg += SEL_THREADS) segc[sg] = 0;
    uint32_t spec_key = R.spec_key;
    if (a.spec_rank && !R.in_carry && m >= a.spec_rank) spec_key = sel_rth_score_key_of(M.cand, m, a.spec_rank, sh); // (uniform)
    if (tid == 0) {
        a.carry_cnt[q] = m;
        uint32_t tau = a.tau_keys ? a.tau_keys[q] : 0u;
        if (a.tau_keys && R.tau > tau) a.tau_keys[q] = tau = R.tau;
        if (a.spec_rank) sel_spec_words(m >= a.spec_rank, spec_key, M.eps2, tau, a.spec_tau + q, a.spec_max + q);
    }
}

__global__ __launch_bounds__(SEL_THREADS) void select_flat_kernel(const SelArgs a) {
    // run_gate: this launch belongs to the gated exact pipeline (cosine_prefilter.hip) and only runs when the
    // screen gave up.  eps2: margin mode (SelMargin); its overflow opens that gate.
    if (a.run_gate && *a.run_gate == 0u) return;
    __shared__ SelShared sh;
    __shared__ uint64_t sel[2 * SEL_MAX];
    __shared__ uint64_t cand[SEL_CAND];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n_segs = a.n_segs;
    uint64_t *pool = a.pools + (uint64_t)q * a.pool_stride;
    uint32_t *segc = a.seg_cnt + (uint64_t)q * a.seg_cnt_stride;
    SEL_STAMP(0);
    const uint32_t c0_raw = a.carry_cnt[q];    // (issued beside the segment counts: not a second round trip after the scan)
    SelMargin M;
    M.eps2 = a.eps2 ? a.eps2[q] : -1.f;
    M.skip = a.skip; M.skip_base = a.skip_base; M.carry = pool; M.spec_rank = a.spec_rank;
    // margin candidates: LDS (4096 keys), or a global buffer of the caller's (the int8 tier: OI_I8_CARRY keys), copied into the
    // carry region after the pass that reads the pool
    M.cand = a.cand ? a.cand + (uint64_t)q * a.cand_cap : cand;
    M.cap = a.cand ? a.cand_cap : SEL_CAND;
    M.rows = SelRowMargin{a.row_meta && M.eps2 < __builtin_inff() ? a.row_meta : nullptr, a.meta_base, a.row_meta ? a.row_qn[q] : 0.f,
                          a.row_meta ? a.row_cq[q] : 0.f};

    // exclusive scan of the (clamped) segment counts -> sh.seg_off; SEL_MAX_SEGS / SEL_THREADS = 4 per thread
    constexpr int SPT = SEL_MAX_SEGS / SEL_THREADS;
    uint32_t c[SPT], local = 0;
#pragma unroll
    for (int u = 0; u < SPT; ++u) {
        const uint32_t sg = tid * SPT + u;
        uint32_t v = segc[sg < n_segs ? sg : 0];
        if (sg >= n_segs) v = 0;
        if (v > a.seg_cap) { *a.overflow = 1u; v = a.seg_cap; }
        c[u] = v;
        local += v;
    }
    const uint32_t incl = oi_wave_incl_scan(local);
    if (lane == 63) sh.wave_tot[wv] = incl;
    if (tid == 0) { sh.cnt = 0; sh.min_key = ~0ull; }
    __syncthreads();
    uint32_t base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SEL_THREADS / 64; ++w) {
        const uint32_t t = sh.wave_tot[w];
        base += (uint32_t)w < wv ? t : 0u;
        total += t;
    }
    uint32_t run = base + incl - local;
#pragma unroll
    for (int u = 0; u < SPT; ++u) {
        const uint32_t sg = tid * SPT + u;
        if (sg < n_segs) sh.seg_off[sg] = run;
        run += c[u];
    }
    if (tid == 0) sh.seg_off[n_segs] = total;
    __syncthreads();

    SelFlat K;
    K.pool = pool; K.seg_off = sh.seg_off; K.carry_cap = a.carry_cap; K.seg_cap = a.seg_cap; K.n_segs = n_segs;
    K.c0 = c0_raw < a.carry_cap ? c0_raw : a.carry_cap;
    K.n = K.c0 + total;
    K.steps = 0;
    while ((1u << K.steps) < n_segs) ++K.steps;
    SEL_STAMP(1);

    const SelResult R = sel_dispatch(K.n, [&](auto cls) { return sel_flat_select<decltype(cls)::value>(K, a.k, M, sh, sel, cand); });
    const uint32_t m = R.m;
    if (R.in_cand) {
        sel_finish_margin(a, q, pool, segc, M, R, sh);
#ifdef OI_ABLATION
        __syncthreads();
        if (sel_dbg_on && blockIdx.x == 0 && tid == 0) {
            const unsigned long long e = __builtin_readcyclecounter();
            printf("select margin n=%u m=%u segs=%u: scan %llu, loads+skip %llu, pass0 %llu, pass1 %llu, filter %llu, compact %llu (cycles)\n", K.n, m, n_segs,
                   sel_dbg_t[1] - sel_dbg_t[0], sel_dbg_t[2] - sel_dbg_t[1], sel_dbg_t[3] - sel_dbg_t[2], sel_dbg_t[4] - sel_dbg_t[3], sel_dbg_t[5] - sel_dbg_t[4], e - sel_dbg_t[5]);
        }
#endif
        return;
    }
    sel_finish(a, q, pool, segc, sel, m, &sh.min_key);
    if (a.compact && a.spec_rank) { // a margin select of a pool of <= k keys (or of fewer than k valid ones): the prediction all the same
        __syncthreads();
        uint32_t spec_key = 0;
        if (m >= a.spec_rank) spec_key = sel_rth_score_key_of(sel, m, a.spec_rank, sh); // (uniform)
        if (tid == 0) sel_spec_words(m >= a.spec_rank, spec_key, M.eps2, a.tau_keys ? a.tau_keys[q] : 0u, a.spec_tau + q, a.spec_max + q);
    }
}

// ---------------------------------------------------------------------------------------------------
// select_topk_kernel: the selection a segment at a time, for pools of more than SEL_MAX_SEGS segments (a BM25 shard of more
// than 134M docs) and for A/B runs (OI_SELECT_V1).  Small pools are gathered into LDS once and the radix select runs out of
// LDS; large pools are scanned in place, one wave per segment, on every pass.  Plain selects only: a margin or gated launch
// takes the flat kernel.
#define SEL_LDS_KEYS 8192

__global__ __launch_bounds__(SEL_THREADS) void select_topk_kernel(const SelArgs a) {
    __shared__ SelRadix rx;
    __shared__ uint64_t sel[2 * SEL_MAX];
    __shared__ uint64_t lds_keys[SEL_LDS_KEYS];
    __shared__ uint32_t s_cnt, s_total;
    __shared__ unsigned long long s_min;

    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, k = a.k;
    uint64_t *pool = a.pools + (uint64_t)q * a.pool_stride;
    uint32_t *segc = a.seg_cnt + (uint64_t)q * a.seg_cnt_stride;
    const uint32_t c0 = a.carry_cnt[q] < a.carry_cap ? a.carry_cnt[q] : a.carry_cap;
    if (tid == 0) { s_cnt = 0; s_total = 0; s_min = ~0ull; }
    __syncthreads();
    {
        uint32_t local = 0;
        for (uint32_t sg = tid; sg < a.n_segs; sg += SEL_THREADS) {
            uint32_t c = segc[sg];
            if (c > a.seg_cap) { *a.overflow = 1u; c = a.seg_cap; }
            local += c;
        }
        local = oi_wave_sum(local);
        if ((tid & 63) == 0 && local) atomicAdd(&s_total, local);
    }
    __syncthreads();
    const uint32_t n = c0 + s_total;
    bool gathered = false; // everything is in lds_keys[0..n)
    // f(valid, key) over the pool; trip counts are uniform over a wave (valid = false past the end), as f's ballots need
    auto for_each = [&](auto &&f) {
        if (gathered) {
            for (uint32_t i0 = 0; i0 < n; i0 += SEL_THREADS) f(i0 + tid < n, lds_keys[i0 + tid < n ? i0 + tid : 0]);
            return;
        }
        for (uint32_t i0 = 0; i0 < c0; i0 += SEL_THREADS) f(i0 + tid < c0, pool[i0 + tid < c0 ? i0 + tid : 0]);
        for (uint32_t sg = wv; sg < a.n_segs; sg += SEL_THREADS / 64) {
            uint32_t c = segc[sg];
            if (c > a.seg_cap) c = a.seg_cap;
            const uint64_t *base = pool + a.carry_cap + (uint64_t)sg * a.seg_cap;
            for (uint32_t i0 = 0; i0 < c; i0 += 64) f(i0 + lane < c, base[i0 + lane < c ? i0 + lane : 0]);
        }
    };
    if (n <= SEL_LDS_KEYS) {
        for_each([&](bool valid, uint64_t key) { sel_append(lds_keys, &s_cnt, SEL_LDS_KEYS, valid, key); });
        __syncthreads();
        gathered = true;
        if (tid == 0) s_cnt = 0;
        __syncthreads();
    }
    if (n <= k) {
        for_each([&](bool valid, uint64_t key) { sel_append(sel, &s_cnt, 2 * SEL_MAX, valid, key); });
    } else {
        int shift;
        uint64_t prefix;
        sel_threshold(for_each, k, rx, shift, prefix);
        // every key whose top bits are >= prefix is selected: exactly k of them (keys are distinct)
        for_each([&](bool valid, uint64_t key) { sel_append(sel, &s_cnt, SEL_MAX, valid && (key >> shift) >= prefix, key); });
    }
    __syncthreads();
    sel_finish(a, q, pool, segc, sel, s_cnt < k ? s_cnt : k, &s_min);
}

int oi_launch_select(oi_ctx *ctx, const PoolView &pool, uint32_t n_queries, uint32_t k, bool compact,
                     float *out_scores, uint32_t *out_docs, uint32_t *out_counts, uint32_t out_stride,
                     const SelectExtra *extra) {
    if (n_queries == 0) return OI_OK;
    OI_REQUIRE(k >= 1 && k <= OI_MAX_DEPTH && k <= pool.carry_cap, "select: k=%u outside [1,%u]", k, OI_MAX_DEPTH);
    ProfScope ps(ctx, "select");
    static const bool v1 = oi_ablation_env("OI_SELECT_V1") != nullptr; // A/B switch: the segment-walking kernel
#ifdef OI_ABLATION
    static const bool stamps = [] {
        const int on = oi_ablation_env("OI_SELECT_STAMPS") ? std::max(1, atoi(oi_ablation_env("OI_SELECT_STAMPS"))) : 0;
        (void)hipMemcpyToSymbol(HIP_SYMBOL(sel_dbg_on), &on, sizeof(int));
        return on != 0;
    }();
    (void)stamps;
#endif
    const bool special = extra && (extra->eps2 || extra->run_gate);
    if (special) {
        OI_REQUIRE(pool.n_segs <= SEL_MAX_SEGS, "select: %u segments (margin / gated selects take <= %u)", pool.n_segs, SEL_MAX_SEGS);
        const uint32_t mcap = extra->cand ? extra->cand_cap : SEL_CAND;
        OI_REQUIRE(!extra->eps2 || (compact && !out_scores && pool.carry_cap >= mcap),
                   "select: margin mode compacts into a carry region of >= %u keys", mcap);
    }
    const bool spec = extra && extra->spec_rank;
    OI_REQUIRE(!spec || (extra->eps2 && extra->spec_tau && extra->spec_max && pool.tau_keys),
               "select: a speculative threshold needs margin mode, thresholds and both output arrays");
    const SelectExtra none{}, &x = extra ? *extra : none;
    const bool margin = x.eps2 != nullptr; // (the members below mean something in margin mode only)
    SelArgs a;
    a.pools = pool.keys; a.carry_cnt = pool.carry_cnt; a.seg_cnt = pool.seg_cnt; a.tau_keys = pool.tau_keys;
    a.pool_stride = pool.stride; a.carry_cap = pool.carry_cap; a.seg_cap = pool.seg_cap; a.n_segs = pool.n_segs;
    a.seg_cnt_stride = pool.seg_cnt_stride; a.overflow = pool.overflow;
    a.k = k; a.compact = compact ? 1 : 0;
    a.out_scores = out_scores; a.out_docs = out_docs; a.out_counts = out_counts; a.out_stride = out_stride;
    a.eps2 = x.eps2; a.margin_gate = x.margin_gate; a.run_gate = x.run_gate;
    a.skip = margin ? x.skip_bitmap : nullptr; a.skip_base = x.skip_base;
    a.cand = margin ? x.cand : nullptr; a.cand_cap = margin ? x.cand_cap : 0u;
    a.row_meta = margin ? x.row_meta : nullptr; a.meta_base = x.meta_base; a.row_qn = x.row_qn; a.row_cq = x.row_cq;
    a.spec_rank = x.spec_rank; a.spec_tau = x.spec_tau; a.spec_max = x.spec_max;
    if ((!v1 || special) && pool.n_segs <= SEL_MAX_SEGS)
        hipLaunchKernelGGL(select_flat_kernel, dim3(n_queries), dim3(SEL_THREADS), 0, ctx->stream, a);
    else
        hipLaunchKernelGGL(select_topk_kernel, dim3(n_queries), dim3(SEL_THREADS), 0, ctx->stream, a);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// [n_shards][n_queries][depth] lists -> pool segment s of query q = shard s's list (keys rebuilt).
__global__ void lists_to_pool_kernel(const float *scores, const uint32_t *docs, const uint32_t *counts,
                                     uint64_t shard_stride, uint64_t count_stride, uint32_t n_queries,
                                     uint32_t depth, uint64_t *pools, uint32_t *carry_cnt,
                                     uint32_t *seg_cnt, uint64_t pool_stride, uint32_t carry_cap,
                                     uint32_t seg_cnt_stride) {
    const uint32_t q = blockIdx.x, sh = blockIdx.y;
    uint32_t c = counts[(uint64_t)sh * count_stride + q];
    if (c > depth) c = depth;
    const uint64_t src = (uint64_t)sh * shard_stride + (uint64_t)q * depth;
    uint64_t *seg = pools + (uint64_t)q * pool_stride + carry_cap + (uint64_t)sh * depth;
    for (uint32_t i = threadIdx.x; i < c; i += blockDim.x) seg[i] = oi_rank_key(scores[src + i], docs[src + i]);
    if (threadIdx.x == 0) {
        seg_cnt[(uint64_t)q * seg_cnt_stride + sh] = c;
        if (sh == 0) carry_cnt[q] = 0;
    }
}

int oi_launch_lists_to_pool(oi_ctx *ctx, const float *scores, const uint32_t *docs,
                            const uint32_t *counts, uint64_t shard_stride, uint64_t count_stride,
                            uint32_t n_shards, uint32_t n_queries, uint32_t depth, const PoolView &pool) {
    if (n_queries == 0) return OI_OK;
    OI_REQUIRE(pool.seg_cap == depth && pool.n_segs == n_shards, "merge: pool geometry mismatch");
    hipLaunchKernelGGL(lists_to_pool_kernel, dim3(n_queries, n_shards), dim3(256), 0, ctx->stream, scores, docs,
                       counts, shard_stride, count_stride, n_queries, depth, pool.keys, pool.carry_cnt, pool.seg_cnt, pool.stride,
                       pool.carry_cap, pool.seg_cnt_stride);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// Reciprocal-rank fusion of two ranked lists per query.
//   rrf(d) = [d in A at rank i] 1/(60+i)  +  [d in B at rank j] 1/(60+j)     (f32, A before B)
// LDS hash table over list A's doc ids; union built in LDS; bitonic sort; top-k out.
#define RRF_HASH 4096
__global__ __launch_bounds__(SEL_THREADS) void rrf_kernel(const uint32_t *docs_a, const uint32_t *counts_a,
                                                          const uint32_t *docs_b, const uint32_t *counts_b,
                                                          uint32_t depth, uint32_t k, float *scores_out,
                                                          uint32_t *docs_out, uint32_t *counts_out) {
    __shared__ uint32_t h_doc[RRF_HASH];
    __shared__ uint32_t h_idx[RRF_HASH]; // rank index in A + 1, 0 = empty
    __shared__ uint32_t a_match[SEL_MAX]; // rank index in B + 1 of the same doc, 0 = none
    __shared__ uint64_t u[2 * SEL_MAX];
    __shared__ uint32_t s_extra;

    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    uint32_t na = counts_a[q], nb = counts_b[q];
    if (na > depth) na = depth;
    if (nb > depth) nb = depth;
    const uint32_t *da = docs_a + (uint64_t)q * depth, *db = docs_b + (uint64_t)q * depth;

    for (uint32_t i = tid; i < RRF_HASH; i += SEL_THREADS) h_idx[i] = 0;
    for (uint32_t i = tid; i < SEL_MAX; i += SEL_THREADS) a_match[i] = 0;
    if (tid == 0) s_extra = 0;
    __syncthreads();
    for (uint32_t i = tid; i < na; i += SEL_THREADS) {
        uint32_t d = da[i];
        uint32_t h = (d * 2654435761u) >> 20; // 12 bits
        for (;;) {
            uint32_t prev = atomicCAS(&h_idx[h], 0u, i + 1);
            if (prev == 0) { h_doc[h] = d; break; }
            h = (h + 1) & (RRF_HASH - 1);
        }
    }
    __syncthreads();
    // list B: look each doc up in A; unmatched docs become their own union entries
    for (uint32_t j = tid; j < nb; j += SEL_THREADS) {
        uint32_t d = db[j];
        uint32_t h = (d * 2654435761u) >> 20;
        uint32_t hit = 0;
        for (;;) {
            uint32_t ix = h_idx[h];
            if (ix == 0) break;
            if (h_doc[h] == d) { hit = ix; break; }
            h = (h + 1) & (RRF_HASH - 1);
        }
        if (hit) a_match[hit - 1] = j + 1;
        else {
            uint32_t pos = atomicAdd(&s_extra, 1u);
            float c = 1.0f / (60.0f + (float)(j + 1));
            u[na + pos] = oi_rank_key(c, d);
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < na; i += SEL_THREADS) {
        float s = 1.0f / (60.0f + (float)(i + 1));
        uint32_t j1 = a_match[i];
        if (j1) s = s + 1.0f / (60.0f + (float)j1);
        u[i] = oi_rank_key(s, da[i]);
    }
    __syncthreads();
    const uint32_t m = na + s_extra;
    uint32_t P = 2;
    while (P < m) P <<= 1;
    for (uint32_t i = m + tid; i < P; i += SEL_THREADS) u[i] = 0;
    __syncthreads();
    bitonic_sort_desc(u, P);
    const uint32_t out = m < k ? m : k;
    for (uint32_t i = tid; i < out; i += SEL_THREADS) {
        scores_out[(uint64_t)q * k + i] = oi_rank_key_score(u[i]);
        docs_out[(uint64_t)q * k + i] = oi_rank_key_doc(u[i]);
    }
    if (tid == 0) counts_out[q] = out;
}

int oi_launch_rrf(oi_ctx *ctx, const uint32_t *docs_a, const uint32_t *counts_a, const uint32_t *docs_b,
                  const uint32_t *counts_b, uint32_t n_queries, uint32_t depth, uint32_t k,
                  float *scores_out, uint32_t *docs_out, uint32_t *counts_out) {
    if (n_queries == 0) return OI_OK;
    OI_REQUIRE(depth >= 1 && depth <= OI_MAX_DEPTH, "rrf: depth=%u outside [1,%u]", depth, OI_MAX_DEPTH);
    OI_REQUIRE(k >= 1 && k <= OI_MAX_DEPTH, "rrf: k=%u outside [1,%u]", k, OI_MAX_DEPTH);
    ProfScope ps(ctx, "rrf");
    hipLaunchKernelGGL(rrf_kernel, dim3(n_queries), dim3(SEL_THREADS), 0, ctx->stream, docs_a, counts_a,
                       docs_b, counts_b, depth, k, scores_out, docs_out, counts_out);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}
