// cosine_share.hip -- oi_similar_share: the social_summary sums of the posts like a BATCH of queries, every post counted at
// most once, under the query it is most like.
//
// The exclusive form of the threshold family (oi_volume.h).  A query q is a CANDIDATE of a document d when d passes
// filters[q] and sim(q, d) >= t_q (clauses 1 and 3 of oi_similar_summary); the WINNER of d is the candidate with the largest
// sim, ties to the smallest q; d is ASSIGNED when it has a winner and a bucket (clause 2), and only then enters cell
// (winner, bucket) and gets a label.  sim is the one f32 value of the rescoring chain on every route, so the winner is a
// function of the inputs alone.  The kernels and the plan are the family's, instantiated with the EXCLUSIVE tally below
// (the stream's sole-candidate proof, the band's publish, the exact route's running pair and the label clear are the
// branches of that axis in oi_volume.h).  What is this file's own:
//   ShTally            assign: clause 2, the cell (the summary's: oi_summary_cell.h), the label.  publish: a candidate pair of
//                      the band does atomicMax(best[row], key), key = ordered_u32(sim) << 32 | ~q (descending u64 order = sim
//                      descending, q ascending; never 0), and keeps the key's high word beside the pair.  begin: the labels
//                      and best preset per call.
//   sh_commit_kernel   one thread per pair of the band kernel: the pair whose key equals best[row] assigns the row.  Keys of one
//                      row differ in q, so exactly one pair wins.  Launched behind the band, inside its profile span.
//   sh_finish_kernel   cells -> records (sm_fold).
#include "oi_summary_cell.h"
#include "oi_volume.h"

__device__ __forceinline__ uint64_t sh_key(uint32_t sim_key, uint32_t q) { return ((uint64_t)sim_key << 32) | (uint32_t)~q; }

struct ShTally;
// (defined below the tally, whose commit hook launches it)
__global__ __launch_bounds__(256) void sh_commit_kernel(const uint64_t *__restrict__ band, uint32_t band_cap, const uint32_t *__restrict__ state,
                                                        uint32_t n_queries, const uint32_t *__restrict__ long_list, uint32_t n_long,
                                                        const uint2 *__restrict__ attrs, uint32_t origin, uint32_t width, uint32_t n_buckets,
                                                        const ShTally tally);

__global__ __launch_bounds__(256) void sh_finish_kernel(const uint32_t *__restrict__ cells, uint64_t n_cells,
                                                        oi_social_counters *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += (uint64_t)gridDim.x * blockDim.x)
        sm_fold(cells + i * SM_CELL_WORDS, out + i);
}

// ------------------------------------------------------------------ the exclusive tally
struct ShTally {
    float thr_all;
    const uint2 *sig;          // the index's signal records
    uint32_t *cells;           // [n_queries][n_buckets] cells of SM_CELL_WORDS
    uint32_t *labels;          // [n_rows], or null
    unsigned long long *best;  // [n_rows] the largest key a band pair published for the row; 0: none (screen route only)
    uint32_t *sim_keys;        // the key's high word beside pair i of the band kernel; 0: not a candidate (ordered_u32 of a
                               // score that is not a NaN is never 0)
    typedef const float *__restrict__ Thr;
    typedef uint2 Rec;
    __device__ __forceinline__ float thr(uint32_t q, Thr thr_q) const { return thr_q ? thr_q[q] : thr_all; }
    __device__ __forceinline__ void assign_cell(uint64_t cell, uint32_t q, uint64_t row) const {
        sm_add(cells, cell, sig[row]);
        if (labels) labels[row] = q;
    }
    // the row is assigned to query q: clause 2, the tally, the label
    __device__ __forceinline__ void assign(uint32_t q, uint32_t row, const uint2 *__restrict__ attrs, uint32_t origin, uint32_t width,
                                           uint32_t n_buckets) const {
        uint32_t b = 0;
        if (width != 0u && !vo_bucket(attrs[row].y, origin, width, n_buckets, &b)) return;
        assign_cell((uint64_t)q * n_buckets + b, q, row);
    }
    __device__ __forceinline__ void publish(uint32_t pair, uint32_t q, uint32_t row, float s, bool candidate) const {
        uint32_t sk = 0;
        if (candidate) {
            sk = oi_f32_key(s);
            atomicMax(best + row, (unsigned long long)sh_key(sk, q));
        }
        sim_keys[pair] = sk;
    }

    static constexpr uint32_t CELL_WORDS = SM_CELL_WORDS;
    static constexpr bool KEY_AXIS = false, EXCLUSIVE = true;
    static constexpr VoNames NAMES = {"share_state", "share_runs", "share_q_rounded", "share_q_bf16",
                                      "share", "share_band", "share_exact", "share_fallback"};
    static const float *thr_block(const float *thr_q, uint32_t q0) { return thr_q ? thr_q + q0 : nullptr; }
    // before the routes: every label is VO_NO_QUERY; on the screen route best is zeroed -- 8 B per row written against the
    // 2 dim B per row the stream reads, and a call that ended early (or a smaller view's call on the same context) can leave
    // nothing behind
    int begin(oi_ctx *ctx, uint64_t n, bool screen) {
        if (labels && n) OI_HIP_CHECK(hipMemsetAsync(labels, 0xFF, n * sizeof(uint32_t), ctx->stream));
        if (!screen) return OI_OK;
        DevBuf &kb = ctx->buf("share_keys"), &bb = ctx->buf("share_best");
        OI_CHECK(kb.ensure(sizeof(uint32_t) * ((size_t)VO_BAND_CAP + (size_t)64 * OI_LONG_ROWS_MAX)));
        OI_CHECK(bb.ensure(sizeof(uint64_t) * n));
        OI_HIP_CHECK(hipMemsetAsync(bb.p, 0, sizeof(uint64_t) * n, ctx->stream));
        sim_keys = kb.as<uint32_t>();
        best = bb.as<unsigned long long>();
        return OI_OK;
    }
    // behind the band kernel
    int commit(oi_ctx *ctx, const uint64_t *band, const uint32_t *state, uint32_t B, const uint32_t *long_list, uint32_t n_long,
               const uint2 *attrs, const oi_volume_spec &sp) const {
        hipLaunchKernelGGL(sh_commit_kernel, dim3((uint32_t)ctx->num_cus * 4), dim3(256), 0, ctx->stream, band, VO_BAND_CAP, state, B,
                           long_list, n_long, attrs, sp.stamp_origin, sp.bucket_width, sp.n_buckets, *this);
        OI_HIP_CHECK(hipGetLastError());
        return OI_OK;
    }
    int finish(oi_ctx *ctx, uint64_t n_cells, oi_social_counters *d_out) const {
        hipLaunchKernelGGL(sh_finish_kernel, dim3((uint32_t)std::min<uint64_t>((n_cells + 255) / 256, 1024)), dim3(256), 0, ctx->stream,
                           cells, n_cells, d_out);
        OI_HIP_CHECK(hipGetLastError());
        return OI_OK;
    }
};

// One thread per pair of the band kernel: the pair that holds its row's best key assigns the row.
__global__ __launch_bounds__(256) void sh_commit_kernel(const uint64_t *__restrict__ band, uint32_t band_cap, const uint32_t *__restrict__ state,
                                                        uint32_t n_queries, const uint32_t *__restrict__ long_list, uint32_t n_long,
                                                        const uint2 *__restrict__ attrs, uint32_t origin, uint32_t width, uint32_t n_buckets,
                                                        const ShTally tally) {
    if ((state[VO_GATE] | state[VO_OVERFLOW]) != 0u) return;
    uint32_t c0 = state[VO_BAND_CNT];
    c0 = c0 < band_cap ? c0 : band_cap;
    const uint32_t c = c0 + n_queries * n_long;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < c; i += gridDim.x * blockDim.x) {
        const uint32_t sk = tally.sim_keys[i];
        if (sk == 0u) continue;
        uint32_t q, row;
        if (i < c0) {
            const uint64_t k = band[i];
            q = (uint32_t)(k >> 32);
            row = (uint32_t)k;
        } else {
            q = (i - c0) / n_long;
            row = long_list[(i - c0) % n_long];
        }
        if (tally.best[row] == sh_key(sk, q)) tally.assign(q, row, attrs, origin, width, n_buckets);
    }
}

// ------------------------------------------------------------------ host
// Device queries / thresholds / filters in, device records (and labels, may be null) out; asynchronous on the ctx stream
// (vo_launch_similar).
int oi_launch_similar_share(oi_index *idx, const float *d_q, uint32_t B, const oi_summary_spec &sp, const float *d_thr, const uint4 *d_filt,
                            oi_social_counters *d_out, uint32_t *d_labels) {
    static_assert(sizeof(oi_social_counters) == 64, "one record per cell");
    const oi_volume_spec vs = {sp.threshold, sp.stamp_origin, sp.bucket_width, sp.n_buckets};
    return vo_launch_similar(idx, d_q, B, vs, d_thr, d_filt, ShTally{sp.threshold, idx->signals.as<uint2>(), nullptr, d_labels, nullptr, nullptr},
                             d_out);
}
