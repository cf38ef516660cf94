// cosine_volume.hip -- oi_similar_volume: how many documents are like a query, per time bucket.
//
// Builder-defined like the rest of the retrieval path (the reference has none).  The aggregation
// counterpart of the filtered search: every other retrieval call returns a ranked list of at most 1024 rows, this one keeps a
// COUNT -- counts[q][b] = documents that pass query q's filter, fall into time bucket b and have sim(q, d) >= t.
//
// sim is ONE f32 value whatever the route: the rescoring chain of pf_rescore_kernel (lane l takes the float4s l, l + 64, ..
// in k order with single fused multiply-adds -- oi_fma_unpacked -- then the wave butterfly sum).  Two routes compute it:
//   1. screen (f32 corpus, d in {384, 768}, a bf16 screening copy, a screen mode, every query with a bound): ONE stream of the
//      copy through cosine_copy_screen's tile loop (vo_stream_kernel).  The screen score s~ of a pair differs from sim by at
//      most eps_q (cosine_prefilter.hip: the bound is measured, and it is stated against the rescoring kernel's value), so with
//      lo = t - eps_q and hi = t + eps_q rounded outward
//          s~ >= hi  =>  sim >= s~ - eps_q >= t      a PROVEN hit: counted at once, its row is never read in f32
//          s~ <  lo  =>  sim <= s~ + eps_q <  t      a proven miss: costs one compare, like a row the screen drops
//      and only the BAND lo <= s~ < hi is undecided: {query, row} goes to one flat buffer, vo_band_kernel computes sim from
//      the f32 rows and counts it when sim >= t.  The bound does not hold for the index's LONG rows (two-class margin): the
//      stream clears them and the band kernel scores every (query, long row) pair.  A band that does not fit its buffer, or a
//      query without a bound, opens the gated launches of route 2 in the same call (the histogram cleared first).
//   2. exact (everything else): vo_exact_kernel, no MFMA -- a wave reads a row once into registers and runs the chain
//      against every query of the batch.
// Both routes evaluate the same chain in the same order: the counts agree bit for bit.
// The kernels and the host driver are the threshold family's (oi_volume.h); this file holds its counting tally.
#include "oi_volume.h"

// The counting tally: a cell is one u32, a hit adds 1 to it, one threshold for the batch.
struct VoCount {
    uint32_t *cells;
    typedef float Thr;
    struct Rec {};
    __device__ __forceinline__ float thr(uint32_t, float t) const { return t; }
    __device__ __forceinline__ Rec load(uint64_t) const { return Rec{}; }
    __device__ __forceinline__ void add(uint64_t cell, Rec) const { atomicAdd(&cells[cell], 1u); }

    static constexpr uint32_t CELL_WORDS = 1;
    static constexpr bool KEY_AXIS = false, EXCLUSIVE = false;
    static constexpr VoNames NAMES = {"volume_state", "volume_runs", "volume_q_rounded", "volume_q_bf16",
                                      "volume", "volume_band", "volume_exact", "volume_fallback"};
    static float thr_block(float t, uint32_t) { return t; }
    int finish(oi_ctx *ctx, uint64_t n_cells, uint32_t *d_counts) const {
        OI_HIP_CHECK(hipMemcpyAsync(d_counts, cells, n_cells * 4, hipMemcpyDeviceToDevice, ctx->stream));
        return OI_OK;
    }
};

// The queries of a bf16 corpus, rounded the way its scorer rounds them (cb_stage_queries: RNE, inf / NaN truncated) and
// widened back to f32 for the chain.
__global__ __launch_bounds__(256) void volume_round_queries_kernel(const float *__restrict__ q, uint64_t total, float *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        out[i] = __uint_as_float(oi_f32_to_bf16_rne(q[i]) << 16);
    }
}

int oi_launch_volume_round_queries(oi_ctx *ctx, const float *d_q, uint64_t total, float *d_out) {
    hipLaunchKernelGGL(volume_round_queries_kernel, dim3((uint32_t)std::min<uint64_t>((total + 255) / 256, 1024)), dim3(256), 0, ctx->stream,
                       d_q, total, d_out);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// Device queries / filters in, device counts out; asynchronous on the ctx stream (vo_launch_similar).
int oi_launch_similar_volume(oi_index *idx, const float *d_q, uint32_t B, const oi_volume_spec &sp, const uint4 *d_filt,
                             uint32_t *d_counts) {
    return vo_launch_similar(idx, d_q, B, sp, sp.threshold, d_filt, VoCount{nullptr}, d_counts);
}
