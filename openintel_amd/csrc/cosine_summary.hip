// cosine_summary.hip -- oi_similar_summary: the social_summary sums of the documents like a query, per time bucket
// (DESIGN 4.11), and the signal records of an index they are summed from (oi_index_set_signals).
//
// The sibling of cosine_volume.hip: the same three clauses decide which documents a (query, bucket) cell takes -- filter,
// bucket, sim(q, d) >= t_q, with sim the one f32 value of the rescoring chain -- and the same kernels evaluate them (the
// threshold family of oi_volume.h, instantiated here with the summing tally).  What differs is the tally: a hit adds the row's
// 8-byte SIGNAL RECORD {pol_q30, flags} to the cell instead of a 1, and every query brings its own threshold t_q.
//
// A cell is 16 words: 12 u32 counts indexed by the record's flag combination class + 3 spec + 6 source, then the i64 sum of
// pol_q30 (words 12, 13), then two words of padding.  A hit costs ONE u32 atomic, and one 64-bit atomic more only when the
// post's polarity is not zero (most posts hit no lexicon word).  Every sum is an integer sum, so the result does not depend
// on the order of the atomics or on the route that found a hit; summary_finish_kernel folds a cell into oi_social_counters.
// The cell itself (sm_add; sm_fold for the other finish) is oi_summary_cell.h's, shared with cosine_groups.hip.
#include "oi_summary_cell.h"
#include "oi_volume.h"

// ------------------------------------------------------------------ the signal records
// Polarity::new (polarity.rs:8-14: NaN -> 0, clamp to [-1, 1]), then the reference's comparisons on that f64 value; v * 2^30
// is exact in f64 and rint rounds to nearest even, |pol_q30| <= 2^30.
__global__ __launch_bounds__(256) void summary_pack_signals_kernel(const double *__restrict__ pol, const uint8_t *__restrict__ spec,
                                                                   const uint8_t *__restrict__ sources, uint64_t n, double tau,
                                                                   uint2 *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        double v = pol[i];
        v = v != v ? 0.0 : (v < -1.0 ? -1.0 : (v > 1.0 ? 1.0 : v));
        const uint32_t cls = v > tau ? SM_BULLISH : (v < -tau ? SM_BEARISH : SM_NEUTRAL);
        const uint32_t flags = cls + 3u * (spec[i] != 0) + 6u * (sources && sources[i] != 0);
        out[i] = make_uint2((uint32_t)(int32_t)rint(v * 1073741824.0), flags);
    }
}

// A cell's 12 counts folded into the caller's record; polarity_sum = (double)(sum of pol_q30) * 2^-30, one rounding at most
// (the conversion: the scaling by a power of two is exact).  (sm_fold's statements, kept here as they were: through the
// helper hipcc allocates this kernel's registers differently, and the kernels the existing calls launch do not move.)
__global__ __launch_bounds__(256) void summary_finish_kernel(const uint32_t *__restrict__ cells, uint64_t n_cells,
                                                             oi_social_counters *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t *c = cells + i * SM_CELL_WORDS;
        uint64_t cls[3] = {0, 0, 0}, spec = 0, src1 = 0, total = 0;
#pragma unroll
        for (uint32_t f = 0; f < 12; ++f) {
            const uint64_t k = c[f];
            total += k;
            cls[f % 3u] += k;
            if ((f / 3u) & 1u) spec += k;
            if (f >= 6u) src1 += k;
        }
        oi_social_counters o;
        o.total = total;
        o.by_source[0] = total - src1;
        o.by_source[1] = src1;
        o.bullish = cls[SM_BULLISH];
        o.bearish = cls[SM_BEARISH];
        o.neutral = cls[SM_NEUTRAL];
        o.spec_count = spec;
        o.polarity_sum = (double)*reinterpret_cast<const long long *>(c + SM_CELL_SUM) * (1.0 / 1073741824.0);
        out[i] = o;
    }
}

// ------------------------------------------------------------------ the summing tally
// A cell is 16 words, a hit adds the row's record (sm_add); thr_q: the queries' own thresholds, or null: thr for all.
struct SmSum {
    float thr_all;
    const uint2 *sig;      // the index's signal records
    uint32_t *cells;
    typedef const float *__restrict__ Thr;
    typedef uint2 Rec;
    __device__ __forceinline__ float thr(uint32_t q, Thr thr_q) const { return thr_q ? thr_q[q] : thr_all; }
    __device__ __forceinline__ Rec load(uint64_t row) const { return sig[row]; }
    __device__ __forceinline__ void add(uint64_t cell, const Rec sg) const { sm_add(cells, cell, sg); }

    static constexpr uint32_t CELL_WORDS = SM_CELL_WORDS;
    static constexpr bool KEY_AXIS = false, EXCLUSIVE = false;
    static constexpr VoNames NAMES = {"summary_state", "summary_runs", "summary_q_rounded", "summary_q_bf16",
                                      "summary", "summary_band", "summary_exact", "summary_fallback"};
    static const float *thr_block(const float *thr_q, uint32_t q0) { return thr_q ? thr_q + q0 : nullptr; }
    int finish(oi_ctx *ctx, uint64_t n_cells, oi_social_counters *d_out) const {
        hipLaunchKernelGGL(summary_finish_kernel, dim3((uint32_t)std::min<uint64_t>((n_cells + 255) / 256, 1024)), dim3(256), 0, ctx->stream,
                           cells, n_cells, d_out);
        OI_HIP_CHECK(hipGetLastError());
        return OI_OK;
    }
};

// ------------------------------------------------------------------ host
int oi_launch_pack_signals(oi_ctx *ctx, const double *d_pol, const uint8_t *d_spec, const uint8_t *d_sources, uint64_t n, double tau,
                           uint2 *d_out) {
    if (n == 0) return OI_OK;
    hipLaunchKernelGGL(summary_pack_signals_kernel, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, ctx->stream,
                       d_pol, d_spec, d_sources, n, tau, d_out);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// Device queries / thresholds / filters in, device records out; asynchronous on the ctx stream (vo_launch_similar).
int oi_launch_similar_summary(oi_index *idx, const float *d_q, uint32_t B, const oi_summary_spec &sp, const float *d_thr,
                              const uint4 *d_filt, oi_social_counters *d_out) {
    static_assert(sizeof(oi_social_counters) == 64, "one record per cell");
    const oi_volume_spec vs = {sp.threshold, sp.stamp_origin, sp.bucket_width, sp.n_buckets};
    return vo_launch_similar(idx, d_q, B, vs, d_thr, d_filt, SmSum{sp.threshold, idx->signals.as<uint2>(), nullptr}, d_out);
}
