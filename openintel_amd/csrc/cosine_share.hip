// cosine_share.hip -- oi_similar_share: the social_summary sums of the posts like a BATCH of queries, every post counted at
// most once, under the query it is most like.
//
// The exclusive form of the threshold family (oi_volume.h).  A query q is a CANDIDATE of a document d when d passes
// filters[q] and sim(q, d) >= t_q (clauses 1 and 3 of oi_similar_summary); the WINNER of d is the candidate with the largest
// sim, ties to the smallest q; d is ASSIGNED when it has a winner and a bucket (clause 2), and only then enters cell
// (winner, bucket) and gets a label.  sim is the one f32 value of the rescoring chain on every route, so the winner is a
// function of the inputs alone.  The cell is the summary's (oi_summary_cell.h); the kernels are this file's own, built from
// the family's parts:
//   route 1  sh_stream_kernel   the tile loop of vo_stream_kernel over the screening copy, the whole batch (<= 64 queries)
//                               in one launch, so a row's candidates all meet in one tile.  Behind the ballot a row's surviving
//                               bits are counted over the half-wave and the query tiles: ONE bit whose score clears `hi` is a
//                               proven sole candidate (every other query is proven below its threshold) and is tallied at
//                               once; every other surviving bit goes to the band as a {query, row} pair.
//            sh_band_kernel     vo_band_kernel's exact chain over the band's pairs and the (query, long row) pairs; a
//                               candidate publishes atomicMax(best[row], key), key = ordered_u32(sim) << 32 | ~q (descending
//                               u64 order = sim descending, q ascending; never 0), and keeps the key's high word beside the pair.
//            sh_commit_kernel   one thread per pair: the pair whose key equals best[row] tallies the row and writes its label.
//                               Keys of one row differ in q, so exactly one pair wins.
//   route 2  sh_exact_kernel    vo_exact_kernel's row-in-registers loop with a running (best sim, q), replaced only on `>`;
//                               one tally and one label per row.  Also the gated fallback of route 1 (a query without a
//                               bound, band overflow) after sh_fallback_clear_kernel has cleared the cells AND the labels.
//   finish   sh_finish_kernel   cells -> records (sm_fold).
#include "oi_summary_cell.h"
#include "oi_volume.h"

#define SH_NO_LABEL 0xFFFFFFFFu

// What the kernels need of a call beside the rows and the queries, by value.  thr_q is a kernel parameter of its own (the
// reason is stated at the head of oi_volume.h).
struct ShTally {
    float thr_all;
    const uint2 *sig;   // the index's signal records
    uint32_t *cells;    // [n_queries][n_buckets] cells of SM_CELL_WORDS
    uint32_t *labels;   // [n_rows], or null
    __device__ __forceinline__ float thr(uint32_t q, const float *__restrict__ thr_q) const { return thr_q ? thr_q[q] : thr_all; }
    // the row is assigned to query q: clause 2, the tally, the label
    __device__ __forceinline__ void assign(uint32_t q, uint32_t row, const uint2 *__restrict__ attrs, uint32_t origin, uint32_t width,
                                           uint32_t n_buckets) const {
        uint32_t b = 0;
        if (width != 0u && !vo_bucket(attrs[row].y, origin, width, n_buckets, &b)) return;
        sm_add(cells, (uint64_t)q * n_buckets + b, sig[row]);
        if (labels) labels[row] = q;
    }
};

__device__ __forceinline__ uint64_t sh_key(uint32_t sim_key, uint32_t q) { return ((uint64_t)sim_key << 32) | (uint32_t)~q; }

// ------------------------------------------------------------------ route 1: the stream
// vo_stream_kernel's tile loop and thresholds; n_queries <= 32 NQT <= 64 is the WHOLE batch.
template <int D, int NQT, int NBUF, bool FILT>
__global__ __launch_bounds__(256, 1) void sh_stream_kernel(
    const uint16_t *__restrict__ rows, uint64_t n_rows,
    const uint16_t *__restrict__ queries, // bf16 [32*NQT][D], zero padded (pf_stage_queries_kernel)
    uint32_t n_queries, const float *__restrict__ thr_q, const float *__restrict__ eps2, const uint32_t *__restrict__ state_in,
    const uint4 *__restrict__ filt, const uint2 *__restrict__ attrs, uint32_t origin, uint32_t width, uint32_t n_buckets,
    const uint32_t *__restrict__ long_bitmap, const ShTally tally, uint64_t *band, uint32_t band_cap, uint32_t *band_cnt,
    uint32_t *overflow) {
    using Ring = OiCopyRing<D, NBUF>;
    static_assert(vo_lds(NBUF) <= 160 * 1024, "LDS");
    static_assert(NQT <= 2, "the batch is at most 64 queries");

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[]; // [4][NBUF][4 KiB] of ring, then the staged band pairs

    if (state_in[VO_GATE] != 0u) return; // a query of the batch has no bound: route 2 assigns the batch (uniform over the grid)
    OI_CLAIM_WHOLE_SIMD(); // (MFMA kernel: nothing else may run on this CU -- oi_device.h)
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t li = lane & 31, lh = lane >> 5;
    uint64_t *stage_keys = reinterpret_cast<uint64_t *>(smem + oi_ring_lds(NBUF)) + w * OI_STAGE; // the wave's staged band pairs
    uint32_t st_head = 0, st_n = 0; // wave-uniform: first staged entry (mod OI_STAGE), staged entries (< OI_STAGE_FLUSH between tiles)

    oi_bf16x8 qreg[NQT][D / 16];
    oi_tile_load_queries<D, NQT>(qreg, queries, li, lh);
    // the two thresholds of the queries this lane tests, rounded OUTWARD from eps2 exactly as vo_stream_kernel does
    float lo[NQT], hi[NQT];
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const uint32_t q = 32u * t + li;
        lo[t] = hi[t] = __builtin_nanf("");
        if (q < n_queries) {
            const float e = 0.5f * eps2[q], tq = tally.thr(q, thr_q);
            lo[t] = nextafterf(tq - e, -__builtin_inff());
            hi[t] = nextafterf(tq + e, __builtin_inff());
        }
    }

    const OiWaveTiles wt = oi_wave_tiles(0, n_rows, w);
    if (wt.my_nt) {
        Ring ring;
        ring.begin(wt, rows, smem + w * Ring::BYTES, lane);
        for (uint64_t ti = 0; ti < wt.my_nt; ++ti) {
            oi_f32x16 acc[NQT];
            ring.template tile<NQT>(acc, qreg);

            // ---- the epilogue: register r of query tile t holds D[row oi_tile_row(row0, r, lh)][query 32 t + li].  The test is
            // the family's (one compare per score); everything else is behind the ballot.
            const uint64_t row0 = wt.row0(ti);
            uint32_t m = oi_tile_pass_mask<NQT>(acc, lo);
            if (__builtin_amdgcn_ballot_w64(m != 0u) != 0ull) {
                m = oi_tile_mask_ragged(m, n_rows - row0, lh);
                if constexpr (FILT) m = oi_filter_tile<NQT>(m, filt, attrs, row0, lh, li);
                if (long_bitmap) { // (the bound does not hold for a long row: the band kernel scores it against every query)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (m & (0x00010001u << r)) {
                            const uint32_t row = oi_tile_row((uint32_t)row0, r, lh);
                            if ((long_bitmap[row >> 5] >> (row & 31)) & 1u) m &= ~(0x00010001u << r);
                        }
                }
                // A row's bits lie in the 32 lanes of its half-wave (lane = li + 32 lh) and the NQT tiles: one ballot per
                // (tile, register) counts them for both halves.  One bit at or above hi: proven, tallied here.  Else: the band.
                uint32_t mb = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const uint32_t rbits = m & (0x00010001u << r);
                    uint32_t cnt = 0;
#pragma unroll
                    for (int t = 0; t < NQT; ++t) {
                        const uint64_t bal = __builtin_amdgcn_ballot_w64((rbits & (1u << (16 * t + r))) != 0u);
                        cnt += (uint32_t)__builtin_popcount(lh ? (uint32_t)(bal >> 32) : (uint32_t)bal);
                    }
                    if (rbits) {
                        bool proven = false;
                        if (cnt == 1u) {
#pragma unroll
                            for (int t = 0; t < NQT; ++t)
                                if ((rbits & (1u << (16 * t + r))) && acc[t][r] >= hi[t]) {
                                    tally.assign(32u * t + li, oi_tile_row((uint32_t)row0, r, lh), attrs, origin, width, n_buckets);
                                    proven = true;
                                }
                        }
                        if (!proven) mb |= rbits;
                    }
                }
                if (__builtin_amdgcn_ballot_w64(mb != 0u) != 0ull) {
                    const uint32_t cnt = (uint32_t)__builtin_popcount(mb);
                    const uint32_t incl = oi_wave_incl_scan(cnt);
                    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                    if (total <= OI_STAGE - OI_STAGE_FLUSH) {
                        // SPARSE (the usual tile): staged in LDS, 64 pairs leave with one claim and one store instruction
                        uint32_t idx = st_head + st_n + incl - cnt;
#pragma unroll
                        for (int t = 0; t < NQT; ++t)
#pragma unroll
                            for (int r = 0; r < 16; ++r)
                                if (mb & (1u << (16 * t + r))) {
                                    const uint32_t row = oi_tile_row((uint32_t)row0, r, lh);
                                    stage_keys[idx & (OI_STAGE - 1)] = ((uint64_t)(32u * t + li) << 32) | row;
                                    ++idx;
                                }
                        st_n += total;
                        while (st_n >= OI_STAGE_FLUSH) {
                            VO_STAGE_FLUSH_TO_BAND(OI_STAGE_FLUSH);
                        }
                    } else {
                        // DENSE (overlapping narratives, a threshold inside a cluster): one claim for the tile, straight to the buffer
                        uint32_t base = 0;
                        if (lane == 0) base = atomicAdd(band_cnt, total);
                        base = __builtin_amdgcn_readfirstlane(base);
                        uint32_t pos = base + incl - cnt;
#pragma unroll
                        for (int t = 0; t < NQT; ++t)
#pragma unroll
                            for (int r = 0; r < 16; ++r)
                                if (mb & (1u << (16 * t + r))) {
                                    const uint32_t row = oi_tile_row((uint32_t)row0, r, lh);
                                    if (pos < band_cap && pos >= base) band[pos] = ((uint64_t)(32u * t + li) << 32) | row;
                                    else *overflow = 1u;
                                    ++pos;
                                }
                    }
                }
            }
            ring.next(wt, rows, ti);
        }
        if (st_n) {
            VO_STAGE_FLUSH_TO_BAND(st_n);
        }
        ring.end();
    }
}

// ------------------------------------------------------------------ route 1: the band and the long rows
// vo_band_kernel's pairs and chain: pairs [0, c0) are the band buffer's {query, local row}; pairs c0 + q * n_long + j are
// (query q, long row j), which have seen neither filter nor threshold yet.  A candidate publishes its key; sim_keys[i] keeps
// the key's high word beside pair i (0: not a candidate -- ordered_u32 of a score that is not a NaN is never 0).
__global__ __launch_bounds__(256) void sh_band_kernel(const float *__restrict__ rows, uint32_t dim, const float *__restrict__ queries,
                                                      uint32_t n_queries, const float *__restrict__ thr_q, const uint64_t *__restrict__ band,
                                                      uint32_t band_cap, const uint32_t *__restrict__ state,
                                                      const uint32_t *__restrict__ long_list, uint32_t n_long,
                                                      const uint4 *__restrict__ filt, const uint2 *__restrict__ attrs, const ShTally tally,
                                                      unsigned long long *best, uint32_t *__restrict__ sim_keys) {
    if ((state[VO_GATE] | state[VO_OVERFLOW]) != 0u) return; // route 2 assigns the batch
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    uint32_t c0 = state[VO_BAND_CNT];
    c0 = c0 < band_cap ? c0 : band_cap;
    const uint32_t c = c0 + n_queries * n_long;
    const uint32_t nvec = dim >> 2;
    for (uint32_t i0 = wave * 4u; i0 < c; i0 += n_waves * 4u) {
        uint32_t q[4], row[4];
        const float4 *x[4], *y[4];
        float a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = i0 + u < c ? i0 + u : c - 1u; // (past the end: the last pair again, not published)
            if (i < c0) {
                const uint64_t k = band[i];
                q[u] = (uint32_t)(k >> 32);
                row[u] = (uint32_t)k;
            } else {
                q[u] = (i - c0) / n_long;
                row[u] = long_list[(i - c0) % n_long];
            }
            x[u] = reinterpret_cast<const float4 *>(rows + (uint64_t)row[u] * dim);
            y[u] = reinterpret_cast<const float4 *>(queries + (uint64_t)q[u] * dim);
            a[u] = 0.f;
        }
        for (uint32_t v = lane; v < nvec; v += 64) {
            float4 xv[4], yv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { xv[u] = oi_load_stream(x[u] + v); yv[u] = y[u][v]; }
#pragma unroll
            for (int u = 0; u < 4; ++u) a[u] = vo_chain4(xv[u], yv[u], a[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float s = oi_wave_sum(a[u]), tq = tally.thr(q[u], thr_q);
            if (lane == 0 && i0 + u < c) {
                uint32_t sk = 0;
                if (s >= tq && (!filt || oi_doc_passes(filt[q[u]], attrs[row[u]]))) {
                    sk = oi_f32_key(s);
                    atomicMax(best + row[u], (unsigned long long)sh_key(sk, q[u]));
                }
                sim_keys[i0 + u] = sk;
            }
        }
    }
}

// One thread per pair of sh_band_kernel: the pair that holds its row's best key assigns the row.
__global__ __launch_bounds__(256) void sh_commit_kernel(const uint64_t *__restrict__ band, uint32_t band_cap, const uint32_t *__restrict__ state,
                                                        uint32_t n_queries, const uint32_t *__restrict__ long_list, uint32_t n_long,
                                                        const uint2 *__restrict__ attrs, uint32_t origin, uint32_t width, uint32_t n_buckets,
                                                        const ShTally tally, const unsigned long long *__restrict__ best,
                                                        const uint32_t *__restrict__ sim_keys) {
    if ((state[VO_GATE] | state[VO_OVERFLOW]) != 0u) return;
    uint32_t c0 = state[VO_BAND_CNT];
    c0 = c0 < band_cap ? c0 : band_cap;
    const uint32_t c = c0 + n_queries * n_long;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < c; i += gridDim.x * blockDim.x) {
        const uint32_t sk = sim_keys[i];
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
        if (best[row] == sh_key(sk, q)) tally.assign(q, row, attrs, origin, width, n_buckets);
    }
}

// ------------------------------------------------------------------ route 2: exact for every shape
// vo_exact_kernel's walk: a wave holds its row in registers and runs the chain against the queries in ascending order, four
// at a time, with a running (best sim, q) that is replaced only on `>` (ties keep the smallest q).  The sums are the same in
// every lane (a butterfly of commutative adds), so the running pair is wave-uniform; lane 0 assigns.  state != null: the
// gated fallback of route 1.
template <int NV, bool BF16>
__global__ __launch_bounds__(256) void sh_exact_kernel(const void *__restrict__ rows, uint64_t n_rows, uint32_t dim,
                                                       const float *__restrict__ queries, uint32_t n_queries, const float *__restrict__ thr_q,
                                                       const uint32_t *__restrict__ state, const uint4 *__restrict__ filt,
                                                       const uint2 *__restrict__ attrs, uint32_t origin, uint32_t width,
                                                       uint32_t n_buckets, const ShTally tally) {
    if (state && (state[VO_GATE] | state[VO_OVERFLOW]) == 0u) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint32_t nvec = dim >> 2;
    const size_t row_bytes = (size_t)dim * (BF16 ? 2 : 4);
    for (uint64_t r = wave; r < n_rows; r += n_waves) {
        const void *xr = reinterpret_cast<const unsigned char *>(rows) + r * row_bytes;
        float4 x[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const uint32_t v = lane + 64u * j;
            x[j] = v < nvec ? vo_load_row4<BF16>(xr, v) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        uint2 at = make_uint2(0u, 0u);
        uint32_t b = 0;
        if (attrs) {
            at = attrs[r];
            if (!vo_bucket(at.y, origin, width, n_buckets, &b)) continue; // (wave-uniform) no bucket: never assigned
        }
        float best_s = 0.f;
        uint32_t best_q = SH_NO_LABEL;
        for (uint32_t q0 = 0; q0 < n_queries; q0 += 4) {
            const float4 *y[4];
            float a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t q = q0 + u < n_queries ? q0 + u : n_queries - 1u; // (past the end: the last query again, not a candidate)
                y[u] = reinterpret_cast<const float4 *>(queries + (uint64_t)q * dim);
                a[u] = 0.f;
            }
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const uint32_t v = lane + 64u * j;
                if (v < nvec) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) a[u] = vo_chain4(x[j], y[u][v], a[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float s = oi_wave_sum(a[u]); // (-0 > +0 is false: the two tie here as they do in the band's key)
                if (q0 + u < n_queries && s >= tally.thr(q0 + u, thr_q) && (!filt || oi_doc_passes(filt[q0 + u], at)) &&
                    (best_q == SH_NO_LABEL || s > best_s)) {
                    best_s = s;
                    best_q = q0 + u;
                }
            }
        }
        if (lane == 0 && best_q != SH_NO_LABEL) {
            sm_add(tally.cells, (uint64_t)best_q * n_buckets + b, tally.sig[r]);
            if (tally.labels) tally.labels[r] = best_q;
        }
    }
}

// The fallback begins: the cells AND the labels of the abandoned stream are cleared and the run is counted (oi_profile_read).
__global__ __launch_bounds__(256) void sh_fallback_clear_kernel(uint32_t *cells, uint64_t words, uint32_t *labels, uint64_t n_rows,
                                                                const uint32_t *__restrict__ state, uint32_t *runs) {
    if ((state[VO_GATE] | state[VO_OVERFLOW]) == 0u) return;
    const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = i0; i < words; i += step) cells[i] = 0u;
    if (labels)
        for (uint64_t i = i0; i < n_rows; i += step) labels[i] = SH_NO_LABEL;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(runs, 1u);
}

__global__ __launch_bounds__(256) void sh_finish_kernel(const uint32_t *__restrict__ cells, uint64_t n_cells,
                                                        oi_social_counters *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += (uint64_t)gridDim.x * blockDim.x)
        sm_fold(cells + i * SM_CELL_WORDS, out + i);
}

// ------------------------------------------------------------------ host
template <int D, int NQT, bool FILT>
static int sh_launch_stream(oi_ctx *ctx, uint32_t grid, const uint16_t *rows, uint64_t n, const uint16_t *q, uint32_t nq, const float *thr,
                            const float *eps2, uint32_t *state, const uint4 *filt, const uint2 *attrs, const oi_summary_spec &sp,
                            const uint32_t *long_bitmap, const ShTally &tally, uint64_t *band) {
    constexpr size_t smem = vo_lds(VO_NBUF);
    OI_CHECK(oi_dyn_lds(ctx, reinterpret_cast<const void *>(sh_stream_kernel<D, NQT, VO_NBUF, FILT>), smem));
    hipLaunchKernelGGL((sh_stream_kernel<D, NQT, VO_NBUF, FILT>), dim3(grid), dim3(256), smem, ctx->stream, rows, n, q, nq, thr, eps2, state,
                       filt, attrs, sp.stamp_origin, sp.bucket_width, sp.n_buckets, long_bitmap, tally, band, VO_BAND_CAP,
                       state + VO_BAND_CNT, state + VO_OVERFLOW);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

template <bool BF16>
static int sh_launch_exact(oi_ctx *ctx, const void *rows, uint64_t n, uint32_t dim, const float *q, uint32_t B, const float *thr,
                           const uint32_t *state, const uint4 *filt, const uint2 *attrs, const oi_summary_spec &sp, const ShTally &tally) {
    const uint32_t nv = (dim / 4 + 63) / 64; // float4 per lane: 1 .. 4 (OI_MAX_DIM = 1024)
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((n + 3) / 4, (uint64_t)ctx->num_cus * 8));
#define SH_EXACT(NV)                                                                                                             \
    hipLaunchKernelGGL((sh_exact_kernel<NV, BF16>), dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, rows, n, dim, q, B, thr, state, \
                       filt, attrs, sp.stamp_origin, sp.bucket_width, sp.n_buckets, tally)
    if (nv <= 1) SH_EXACT(1);
    else if (nv == 2) SH_EXACT(2);
    else if (nv == 3) SH_EXACT(3);
    else SH_EXACT(4);
#undef SH_EXACT
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// Device queries / thresholds / filters in, device records (and labels, may be null) out; asynchronous on the ctx stream.
// vo_launch_similar's plan with the routes above; the argument and state checks are the entry point's (api.hip).
int oi_launch_similar_share(oi_index *idx, const float *d_q, uint32_t B, const oi_summary_spec &sp, const float *d_thr, const uint4 *d_filt,
                            oi_social_counters *d_out, uint32_t *d_labels) {
    static_assert(sizeof(oi_social_counters) == 64, "one record per cell");
    static_assert(OI_MAX_DIM <= 1024u, "sh_exact_kernel holds a row in at most 4 float4 per lane");
    oi_ctx *ctx = idx->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = idx->n_docs;
    const uint32_t dim = idx->dim;
    const uint64_t n_cells = (uint64_t)B * sp.n_buckets, words = n_cells * SM_CELL_WORDS;
    const uint2 *attrs = (d_filt || sp.bucket_width) ? idx->doc_attrs.as<uint2>() : nullptr;
    // state (16 B, see VO_GATE ..) and the cells behind it, zeroed per call; the fallback-run counter lives on
    DevBuf &sb = ctx->buf("share_state"), &rb = ctx->buf("share_runs");
    OI_CHECK(sb.ensure(64 + words * 4));
    if (!rb.p) {
        OI_CHECK(rb.ensure(16));
        OI_HIP_CHECK(hipMemsetAsync(rb.p, 0, 16, st));
    }
    uint32_t *state = sb.as<uint32_t>();
    const ShTally tally = {sp.threshold, idx->signals.as<uint2>(), state + 16, d_labels};
    OI_HIP_CHECK(hipMemsetAsync(sb.p, 0, 64 + words * 4, st));
    if (d_labels && n) OI_HIP_CHECK(hipMemsetAsync(d_labels, 0xFF, n * sizeof(uint32_t), st)); // every row: SH_NO_LABEL
    const float *q = d_q;
    if (idx->rows_bf16) {
        DevBuf &qr = ctx->buf("share_q_rounded");
        const uint64_t total = (uint64_t)B * dim;
        OI_CHECK(qr.ensure(total * 4));
        OI_CHECK(oi_launch_volume_round_queries(ctx, d_q, total, qr.as<float>()));
        q = qr.as<float>();
    }
    const int mode = ctx->cosine_mode;
    const bool screen = n > 0 && B <= 64 && (mode == OI_COSINE_SCREEN || mode == OI_COSINE_SCREEN_COPY) && oi_index_screenable(idx) &&
                        idx->screen_copy.p;
    if (n == 0) {
        // (nothing to assign)
    } else if (!screen) {
        ProfScope ps(ctx, "share_exact");
        if (idx->rows_bf16) OI_CHECK(sh_launch_exact<true>(ctx, idx->rows_bf16, n, dim, q, B, d_thr, nullptr, d_filt, attrs, sp, tally));
        else OI_CHECK(sh_launch_exact<false>(ctx, idx->rows, n, dim, q, B, d_thr, nullptr, d_filt, attrs, sp, tally));
    } else {
        const uint32_t n_padded = (B + 31u) & ~31u, n_long = idx->n_long;
        DevBuf &qb = ctx->buf("share_q_bf16"), &bb = ctx->buf("volume_band"); // (one band buffer for the family: one call at a time)
        DevBuf &kb = ctx->buf("share_keys"), &best = ctx->buf("share_best");
        const size_t qb_bytes = (sizeof(uint16_t) * (size_t)(n_padded + 64) * dim + 255) & ~(size_t)255;
        OI_CHECK(qb.ensure(qb_bytes + sizeof(float) * B));
        OI_CHECK(bb.ensure(sizeof(uint64_t) * (size_t)VO_BAND_CAP));
        OI_CHECK(kb.ensure(sizeof(uint32_t) * ((size_t)VO_BAND_CAP + (size_t)64 * OI_LONG_ROWS_MAX)));
        OI_CHECK(best.ensure(sizeof(uint64_t) * n));
        // best is zeroed per call: 8 B per row written against the 2 dim B per row the stream reads, and a call that ended early
        // (or a smaller view's call on the same context) can leave nothing behind
        OI_HIP_CHECK(hipMemsetAsync(best.p, 0, sizeof(uint64_t) * n, st));
        uint16_t *q16 = qb.as<uint16_t>();
        float *eps2 = reinterpret_cast<float *>(qb.as<unsigned char>() + qb_bytes);
        OI_CHECK(oi_launch_screen_stage(ctx, q, B, dim, idx->max_row_norm.as<uint32_t>(), q16, eps2, state + VO_GATE));
        const uint32_t *lbm = n_long ? idx->long_bitmap.as<uint32_t>() : nullptr;
        const uint32_t *llist = n_long ? idx->long_list.as<uint32_t>() : nullptr;
        uint32_t grid = 0, seg_cap = 0;
        oi_cosine_screen_geometry(ctx, n, &grid, &seg_cap); // (the persistent grid of the screens: 7/8 of the CUs)
        {
            ProfScope ps(ctx, "share");
#define SH_SCREEN(DD, T)                                                                                                             \
    OI_CHECK(d_filt ? (sh_launch_stream<DD, T, true>(ctx, grid, idx->screen_copy.as<uint16_t>(), n, q16, B, d_thr, eps2, state, d_filt, \
                                                     attrs, sp, lbm, tally, bb.as<uint64_t>()))                                      \
                    : (sh_launch_stream<DD, T, false>(ctx, grid, idx->screen_copy.as<uint16_t>(), n, q16, B, d_thr, eps2, state, d_filt, \
                                                      attrs, sp, lbm, tally, bb.as<uint64_t>())))
            if (dim == 768) { if (B > 32) SH_SCREEN(768, 2); else SH_SCREEN(768, 1); }
            else { if (B > 32) SH_SCREEN(384, 2); else SH_SCREEN(384, 1); }
#undef SH_SCREEN
        }
        {
            ProfScope ps(ctx, "share_band");
            hipLaunchKernelGGL(sh_band_kernel, dim3((uint32_t)ctx->num_cus * 4), dim3(256), 0, st, idx->rows, dim, q, B, d_thr,
                               bb.as<uint64_t>(), VO_BAND_CAP, state, llist, n_long, d_filt, attrs, tally,
                               best.as<unsigned long long>(), kb.as<uint32_t>());
            OI_HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(sh_commit_kernel, dim3((uint32_t)ctx->num_cus * 4), dim3(256), 0, st, bb.as<uint64_t>(), VO_BAND_CAP, state, B,
                               llist, n_long, attrs, sp.stamp_origin, sp.bucket_width, sp.n_buckets, tally,
                               best.as<unsigned long long>(), kb.as<uint32_t>());
            OI_HIP_CHECK(hipGetLastError());
        }
        {
            // the gated fallback: both launches exit at once unless the band overflowed or a query has no bound
            ProfScope ps(ctx, "share_fallback");
            const uint64_t most = std::max<uint64_t>(words, d_labels ? n : 0);
            hipLaunchKernelGGL(sh_fallback_clear_kernel, dim3((uint32_t)std::min<uint64_t>((most + 255) / 256, 1024)), dim3(256), 0, st,
                               tally.cells, words, d_labels, n, state, rb.as<uint32_t>());
            OI_HIP_CHECK(hipGetLastError());
            OI_CHECK(sh_launch_exact<false>(ctx, idx->rows, n, dim, q, B, d_thr, state, d_filt, attrs, sp, tally));
        }
    }
    hipLaunchKernelGGL(sh_finish_kernel, dim3((uint32_t)std::min<uint64_t>((n_cells + 255) / 256, 1024)), dim3(256), 0, st, tally.cells,
                       n_cells, d_out);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}
