// oi_volume.h -- the threshold family: oi_similar_volume (cosine_volume.hip), oi_similar_summary
// (cosine_summary.hip, 4.11), oi_similar_groups (cosine_groups.hip, 4.12) and oi_similar_share (cosine_share.hip, 4.13) are ONE set
// of kernels and one host driver, written here once as templates over a TALLY: what a document that passes the three clauses
// (filter, bucket, sim >= t_q) adds to its (query, bucket) cell.
//
// A tally is a small struct passed to the kernels by value (it sits in the kernel arguments where the output pointer would):
//   device   uint32_t *cells;                    the call's cells, CELL_WORDS u32 each (the driver sets and slices it)
//            Thr                                  the type of the kernels' threshold argument (float, or const float *__restrict__:
//                                                 an array wants a kernel parameter of its own -- a pointer inside a by-value
//                                                 struct is not __restrict__, and its uniform loads stop being scalar loads)
//            float thr(q, Thr t)                  the threshold of query q of the launch
//            Rec, Rec load(row)                   what a row adds; the stream loads it at the row's first proven hit
//            void add(cell, Rec)                  one hit
//   host     CELL_WORDS, NAMES                    words per cell; the workspace names and profile tags
//            KEY_AXIS                             false: clause 2 is the time bucket of the row's stamp (vo_bucket).  true: it is the
//                                                 KEY of the row's group (vo_key), and the kernels' three u32 arguments
//                                                 origin / width / n_buckets carry key_mask / its shift / n_keys
//            EXCLUSIVE                            false: every (query, row) pair is decided on its own (load / add above).  true:
//                                                 a row enters ONE cell, that of its best candidate query -- see below
//            Thr thr_block(Thr, q0)               the threshold argument of the launch that begins at query q0
//            int finish(ctx, n_cells, out)        cells -> the caller's array, on the ctx stream
// An EXCLUSIVE tally has no load / add.  The kernels compare a row's candidates first (the stream: a sole surviving bit at or
// above hi is proven, every other bit goes to the band; the band: every candidate pair is published, a later pass picks the
// row's best; the exact route: a running best pair per row; the fallback's clear takes the labels too) and call
//   device   void assign(q, row, attrs, origin, width, n_buckets)   row is q's: clause 2, then the cell (the stream's proven rows)
//            void assign_cell(cell, q, row)                          the same with clause 2 already evaluated (the exact route)
//            void publish(pair, q, row, sim, candidate)              pair of the band kernel: every pair of the launch, once
//            uint32_t *labels;                                       [n_rows] or null: the query a row went to, VO_NO_QUERY
//   host     int begin(ctx, n_rows, screen)       before the routes: its per-call presets and workspaces
//            int commit(ctx, band, state, B, long_list, n_long, attrs, spec)   behind the band kernel, inside its profile span
// and its stream route takes a batch of at most 64 queries (one launch: a row's candidates must all meet in one tile).
// VoCount (cosine_volume.hip), SmSum (cosine_summary.hip), GrSum (cosine_groups.hip, the key axis) and ShTally (cosine_share.hip,
// the exclusive one) are the four there are.
// The stream kernel's tile pipeline (query block, tile ownership, the bf16 copy ring, the score test) is oi_screen_tile.h's, shared
// with cosine_copy_screen; its own are the two thresholds and the tallying epilogue with the band staging.
#pragma once

#include <algorithm>
#include <cmath>

#include "oi_device.h"
#include "oi_internal.h"
#include "oi_lds_dma.h"
#include "oi_screen_tile.h"

#define VO_BAND_CAP (4u << 20)       // undecided pairs per call: 32 MB, the collapse mask's budget
#define VO_NBUF 8                    // the copy screen's ring depth (cosine_screen_copy.hip: depth is not what holds the stream)
// state words of a call (zeroed by it): [0] gate (a query without a bound), [1] band overflow, [2] band fill
#define VO_GATE 0
#define VO_OVERFLOW 1
#define VO_BAND_CNT 2
#define VO_NO_QUERY 0xFFFFFFFFu      // an exclusive tally's label of a row that no query takes
// dynamic LDS of vo_stream_kernel: the four rings, then the waves' staged band pairs
constexpr size_t vo_lds(int nbuf) { return oi_ring_lds(nbuf) + 4 * OI_STAGE * 8; }

// Clause 2 of the definition: the bucket of a stamp.  stamp >= origin makes the 32-bit difference exact, so origin + n * width
// may exceed 2^32 without a 64-bit division.
__device__ __forceinline__ bool vo_bucket(uint32_t stamp, uint32_t origin, uint32_t width, uint32_t n_buckets, uint32_t *b) {
    if (width == 0u) { *b = 0u; return true; }
    if (stamp < origin) return false;
    const uint32_t k = (stamp - origin) / width;
    *b = k;
    return k < n_buckets;
}

// Clause 2 on the key axis (oi_similar_groups): key = (group & mask) >> shift; a key >= n_keys belongs to no cell.
__device__ __forceinline__ bool vo_key(uint32_t group, uint32_t mask, uint32_t shift, uint32_t n_keys, uint32_t *b) {
    const uint32_t k = (group & mask) >> shift;
    *b = k;
    return k < n_keys;
}
// Clause 2 of a tally, for a row whose attributes are at hand.
template <class Tally>
__device__ __forceinline__ bool vo_cell(const uint2 at, uint32_t origin, uint32_t width, uint32_t n_buckets, uint32_t *b) {
    if constexpr (Tally::KEY_AXIS) return vo_key(at.x, origin, width, n_buckets, b);
    else return vo_bucket(at.y, origin, width, n_buckets, b);
}

// The first NF staged band pairs of the wave leave for the band buffer: ONE atomic claims their room, one store instruction
// writes them.  (A macro for the reason OI_STAGE_FLUSH_TO_POOL is one.)  Reads from the enclosing kernel: lane, st_head, st_n,
// stage_keys, band, band_cnt, band_cap, overflow.
#define VO_STAGE_FLUSH_TO_BAND(NF)                                                                                     \
    do {                                                                                                               \
        const uint32_t nf_ = (NF);                                                                                     \
        asm volatile("" ::: "memory");                                                                                 \
        uint32_t base_ = 0;                                                                                            \
        if (lane == 0) base_ = atomicAdd(band_cnt, nf_);                                                               \
        base_ = __builtin_amdgcn_readfirstlane(base_);                                                                 \
        if (lane < nf_) {                                                                                              \
            const uint64_t key_ = stage_keys[(st_head + lane) & (OI_STAGE - 1)];                                       \
            if (base_ + lane < band_cap && base_ + lane >= base_) band[base_ + lane] = key_;                           \
            else *overflow = 1u;                                                                                       \
        }                                                                                                              \
        asm volatile("" ::: "memory");                                                                                 \
        st_head = (st_head + nf_) & (OI_STAGE - 1);                                                                    \
        st_n -= nf_;                                                                                                   \
    } while (0)

// ------------------------------------------------------------------ the chain
// Four floats of a stored row as the chain sees them: f32 as they are, bf16 widened exactly.
template <bool BF16>
__device__ __forceinline__ float4 vo_load_row4(const void *row, uint32_t v) {
    if constexpr (BF16) {
        const uint2 u = oi_load_stream(reinterpret_cast<const uint2 *>(row) + v);
        return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xFFFF0000u), __uint_as_float(u.y << 16),
                           __uint_as_float(u.y & 0xFFFF0000u));
    } else {
        return oi_load_stream(reinterpret_cast<const float4 *>(row) + v);
    }
}
// one float4 step of pf_rescore_kernel's chain: single v_fma_f32 each (oi_device.h: a packed op_sel fma beside another
// lane's MFMA stream has produced a wrong score)
__device__ __forceinline__ float vo_chain4(const float4 x, const float4 y, float a) {
    a = oi_fma_unpacked(x.x, y.x, a); a = oi_fma_unpacked(x.y, y.y, a);
    a = oi_fma_unpacked(x.z, y.z, a); a = oi_fma_unpacked(x.w, y.w, a);
    return a;
}

// ------------------------------------------------------------------ route 1: the stream
// The tile pipeline of oi_screen_tile.h (see there for the ring, its counted waits and the operand layout) over ALL rows in one
// launch, with the tallying epilogue.  FILT: the queries carry doc filters.  attrs is also set when only buckets are asked for.
template <int D, int NQT, int NBUF, bool FILT, class Tally>
__global__ __launch_bounds__(256, 1) void vo_stream_kernel(
    const uint16_t *__restrict__ rows, uint64_t n_rows,
    const uint16_t *__restrict__ queries, // bf16 [32*NQT][D], zero padded (pf_stage_queries_kernel)
    uint32_t n_queries, uint32_t q_base, typename Tally::Thr thr, const float *__restrict__ eps2, const uint32_t *__restrict__ state_in,
    const uint4 *__restrict__ filt, const uint2 *__restrict__ attrs, uint32_t origin, uint32_t width, uint32_t n_buckets,
    const uint32_t *__restrict__ long_bitmap, const Tally tally, uint64_t *band, uint32_t band_cap, uint32_t *band_cnt,
    uint32_t *overflow) {
    using Ring = OiCopyRing<D, NBUF>;
    static_assert(vo_lds(NBUF) <= 160 * 1024, "LDS");

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[]; // [4][NBUF][4 KiB] of ring, then the staged band pairs

    if (state_in[VO_GATE] != 0u) return; // a query of the batch has no bound: route 2 tallies the batch (uniform over the grid)
    OI_CLAIM_WHOLE_SIMD(); // (MFMA kernel: nothing else may run on this CU -- oi_device.h)
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t li = lane & 31, lh = lane >> 5;
    uint64_t *stage_keys = reinterpret_cast<uint64_t *>(smem + oi_ring_lds(NBUF)) + w * OI_STAGE; // the wave's staged band pairs
    uint32_t st_head = 0, st_n = 0; // wave-uniform: first staged entry (mod OI_STAGE), staged entries (< OI_STAGE_FLUSH between tiles)

    oi_bf16x8 qreg[NQT][D / 16];
    oi_tile_load_queries<D, NQT>(qreg, queries, li, lh);
    // the two thresholds of the queries this lane tests, from the query's own t_q, rounded OUTWARD (eps_q is half of what the
    // staging kernel stores: it keeps 2 eps for the margin selects); no query in the slot, or a NaN t_q = NaN, which no score is >=
    float lo[NQT], hi[NQT];
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const uint32_t q = 32u * t + li;
        lo[t] = hi[t] = __builtin_nanf("");
        if (q < n_queries) {
            const float e = 0.5f * eps2[q], tq = tally.thr(q, thr);
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

            // ---- the tallying epilogue, straight out of the accumulators: register r of query tile t holds
            // D[row oi_tile_row(row0, r, lh)][query 32 t + li].  The test costs what the screen's costs (one compare per score);
            // everything else is behind the ballot.
            const uint64_t row0 = wt.row0(ti);
            uint32_t m = oi_tile_pass_mask<NQT>(acc, lo);
            if (__builtin_amdgcn_ballot_w64(m != 0u) != 0ull) {
                m = oi_tile_mask_ragged(m, n_rows - row0, lh);
                if constexpr (FILT) m = oi_filter_tile<NQT>(m, filt, attrs, row0, lh, li);
                uint32_t mb = 0;
                if constexpr (Tally::EXCLUSIVE) {
                    // The launch holds the WHOLE batch (vo_launch_similar screens an exclusive tally only at B <= 64, in one
                    // launch): a sole bit proves nothing about the queries of another slice.  So q_base is 0 here and 32 t + li
                    // is the query's own number, as the label and the cell want it.
                    static_assert(NQT <= 2, "an exclusive batch is at most 64 queries");
                    if (long_bitmap) { // (the bound does not hold for a long row: the band kernel scores it against every query)
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            if (m & (0x00010001u << r)) {
                                const uint32_t row = oi_tile_row((uint32_t)row0, r, lh);
                                if ((long_bitmap[row >> 5] >> (row & 31)) & 1u) m &= ~(0x00010001u << r);
                            }
                    }
                    // A row's bits lie in the 32 lanes of its half-wave (lane = li + 32 lh) and the NQT tiles: one ballot per
                    // (tile, register) counts them for both halves.  ONE bit, at or above hi: a proven sole candidate (every
                    // other query is proven below its threshold), assigned here.  Else every bit of the row goes to the band.
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
                } else {
                    // per row with a bit left: its bucket (the stamp is loaded for such rows only) and the long-row bitmap; then
                    // a proven hit is tallied (the row's record loaded at its first one), a band pair keeps its bit
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        if (m & (0x00010001u << r)) {
                            const uint32_t row = oi_tile_row((uint32_t)row0, r, lh);
                            uint32_t b = 0;
                            bool ok = true;
                            if constexpr (Tally::KEY_AXIS) ok = vo_key(attrs[row].x, origin, width, n_buckets, &b);
                            else if (width != 0u) ok = vo_bucket(attrs[row].y, origin, width, n_buckets, &b);
                            if (long_bitmap && ((long_bitmap[row >> 5] >> (row & 31)) & 1u)) ok = false; // (the bound does not hold: band kernel)
                            if (ok) {
                                bool have = false;
                                typename Tally::Rec rec{};
#pragma unroll
                                for (int t = 0; t < NQT; ++t)
                                    if (m & (1u << (16 * t + r))) {
                                        if (acc[t][r] >= hi[t]) {
                                            if (!have) { rec = tally.load(row); have = true; }
                                            tally.add((uint64_t)(32u * t + li) * n_buckets + b, rec);
                                        } else mb |= 1u << (16 * t + r);
                                    }
                            }
                        }
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
                                    stage_keys[idx & (OI_STAGE - 1)] = ((uint64_t)(q_base + 32u * t + li) << 32) | row;
                                    ++idx;
                                }
                        st_n += total;
                        while (st_n >= OI_STAGE_FLUSH) {
                            VO_STAGE_FLUSH_TO_BAND(OI_STAGE_FLUSH);
                        }
                    } else {
                        // DENSE (a threshold inside a cluster of near-equal scores): one claim for the tile, straight to the buffer
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
                                    if (pos < band_cap && pos >= base) band[pos] = ((uint64_t)(q_base + 32u * t + li) << 32) | row;
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
// One wave-iteration per pair, four rows in flight like the rescoring kernel.  Pairs [0, c0) are the band buffer's
// {query, local row}; pairs c0 + q * n_long + j are (query q, long row j) -- those have seen neither filter nor bucket yet.
template <class Tally>
__global__ __launch_bounds__(256) void vo_band_kernel(const float *__restrict__ rows, uint32_t dim, const float *__restrict__ queries,
                                                      uint32_t n_queries, typename Tally::Thr thr, const uint64_t *__restrict__ band,
                                                      uint32_t band_cap, const uint32_t *__restrict__ state,
                                                      const uint32_t *__restrict__ long_list, uint32_t n_long,
                                                      const uint4 *__restrict__ filt, const uint2 *__restrict__ attrs,
                                                      uint32_t origin, uint32_t width, uint32_t n_buckets, const Tally tally) {
    if ((state[VO_GATE] | state[VO_OVERFLOW]) != 0u) return; // route 2 tallies the batch
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
            const uint32_t i = i0 + u < c ? i0 + u : c - 1u; // (past the end: the last pair again, not counted)
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
            // (t_q is read ahead of the test: with the call inside the condition hipcc lays the whole kernel out differently)
            const float s = oi_wave_sum(a[u]), tq = tally.thr(q[u], thr);
            if constexpr (Tally::EXCLUSIVE) {
                // every pair of the launch leaves its word for the commit; clause 2 is the assignment's
                if (lane == 0 && i0 + u < c)
                    tally.publish(i0 + u, q[u], row[u], s, s >= tq && (!filt || oi_doc_passes(filt[q[u]], attrs[row[u]])));
            } else if (lane == 0 && i0 + u < c && s >= tq) {
                uint32_t b = 0;
                bool ok = true;
                if (attrs) {
                    const uint2 at = attrs[row[u]];
                    if (filt) ok = oi_doc_passes(filt[q[u]], at);
                    ok = ok && vo_cell<Tally>(at, origin, width, n_buckets, &b);
                }
                if (ok) tally.add((uint64_t)q[u] * n_buckets + b, tally.load(row[u]));
            }
        }
    }
}

// ------------------------------------------------------------------ route 2: exact for every shape
// Waves walk the rows; a wave holds its row (and its record) in registers (NV float4 per lane) and runs the chain against
// the queries, four at a time.  state != null: the gated fallback of route 1 (exits at once unless the gate or the overflow flag is up).
template <int NV, bool BF16, class Tally>
__global__ __launch_bounds__(256) void vo_exact_kernel(const void *__restrict__ rows, uint64_t n_rows, uint32_t dim,
                                                       const float *__restrict__ queries, uint32_t n_queries, typename Tally::Thr thr,
                                                       const uint32_t *__restrict__ state, const uint4 *__restrict__ filt,
                                                       const uint2 *__restrict__ attrs, uint32_t origin, uint32_t width,
                                                       uint32_t n_buckets, const Tally tally) {
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
            if (!vo_cell<Tally>(at, origin, width, n_buckets, &b)) continue; // (wave-uniform)
        }
        typename Tally::Rec rec{};
        if constexpr (!Tally::EXCLUSIVE) rec = tally.load(r);
        // the exclusive tally's running pair: replaced only on `>`, so ties keep the smallest q.  The sums are the same in every
        // lane (a butterfly of commutative adds), so the pair is wave-uniform.  (-0 > +0 is false: the two tie, as their keys do.)
        float best_s = 0.f;
        uint32_t best_q = VO_NO_QUERY;
        for (uint32_t q0 = 0; q0 < n_queries; q0 += 4) {
            const float4 *y[4];
            float a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t q = q0 + u < n_queries ? q0 + u : n_queries - 1u; // (past the end: the last query again, not counted)
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
                const float s = oi_wave_sum(a[u]);
                if constexpr (Tally::EXCLUSIVE) {
                    if (q0 + u < n_queries && s >= tally.thr(q0 + u, thr) && (!filt || oi_doc_passes(filt[q0 + u], at)) &&
                        (best_q == VO_NO_QUERY || s > best_s)) {
                        best_s = s;
                        best_q = q0 + u;
                    }
                } else if (lane == 0 && q0 + u < n_queries && s >= tally.thr(q0 + u, thr) && (!filt || oi_doc_passes(filt[q0 + u], at)))
                    tally.add((uint64_t)(q0 + u) * n_buckets + b, rec);
            }
        }
        if constexpr (Tally::EXCLUSIVE)
            if (lane == 0 && best_q != VO_NO_QUERY) tally.assign_cell((uint64_t)best_q * n_buckets + b, best_q, r);
    }
}

// The fallback begins: every word of every cell of the abandoned screen route is cleared and the run is counted
// (oi_profile_read).  (A template only so that both translation units may hold it.)
template <class Tally>
__global__ __launch_bounds__(256) void vo_fallback_clear_kernel(uint32_t *cells, uint64_t words, const uint32_t *__restrict__ state,
                                                                uint32_t *runs) {
    if ((state[VO_GATE] | state[VO_OVERFLOW]) == 0u) return;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x) cells[i] = 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(runs, 1u);
}
// An exclusive tally's: the labels of the abandoned stream go too (labels may be null).  An overload, not one more parameter of
// the kernel above: a template's parameter list is part of its instances' names, and the three that exist do not move.
template <class Tally>
__global__ __launch_bounds__(256) void vo_fallback_clear_kernel(uint32_t *cells, uint64_t words, uint32_t *labels, uint64_t n_rows,
                                                                const uint32_t *__restrict__ state, uint32_t *runs) {
    if ((state[VO_GATE] | state[VO_OVERFLOW]) == 0u) return;
    const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = i0; i < words; i += step) cells[i] = 0u;
    if (labels)
        for (uint64_t i = i0; i < n_rows; i += step) labels[i] = VO_NO_QUERY;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(runs, 1u);
}

// ------------------------------------------------------------------ host
// the workspace names and profile tags of a tally
struct VoNames {
    const char *state, *runs, *q_rounded, *q_bf16;        // ctx->buf
    const char *stream, *band, *exact, *fallback;         // ProfScope
};

template <int D, int NQT, bool FILT, class Tally>
static int vo_launch_stream(oi_ctx *ctx, uint32_t grid, const uint16_t *rows, uint64_t n, const uint16_t *q, uint32_t nq, uint32_t q_base,
                            typename Tally::Thr thr, const float *eps2, uint32_t *state, const uint4 *filt, const uint2 *attrs,
                            const oi_volume_spec &sp, const uint32_t *long_bitmap, const Tally &tally, uint64_t *band) {
    constexpr size_t smem = vo_lds(VO_NBUF);
    OI_CHECK(oi_dyn_lds(ctx, reinterpret_cast<const void *>(vo_stream_kernel<D, NQT, VO_NBUF, FILT, Tally>), smem));
    hipLaunchKernelGGL((vo_stream_kernel<D, NQT, VO_NBUF, FILT, Tally>), dim3(grid), dim3(256), smem, ctx->stream, rows, n, q, nq, q_base, thr,
                       eps2, state, filt, attrs, sp.stamp_origin, sp.bucket_width, sp.n_buckets, long_bitmap, tally, band,
                       VO_BAND_CAP, state + VO_BAND_CNT, state + VO_OVERFLOW);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

template <bool BF16, class Tally>
static int vo_launch_exact(oi_ctx *ctx, const void *rows, uint64_t n, uint32_t dim, const float *q, uint32_t B, typename Tally::Thr thr,
                           const uint32_t *state, const uint4 *filt, const uint2 *attrs, const oi_volume_spec &sp, const Tally &tally) {
    const uint32_t nv = (dim / 4 + 63) / 64; // float4 per lane: 1 .. 4 (OI_MAX_DIM = 1024)
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((n + 3) / 4, (uint64_t)ctx->num_cus * 8));
#define VO_EXACT(NV)                                                                                                                  \
    hipLaunchKernelGGL((vo_exact_kernel<NV, BF16, Tally>), dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, rows, n, dim, q, B, thr, \
                       state, filt, attrs, sp.stamp_origin, sp.bucket_width, sp.n_buckets, tally)
    if (nv <= 1) VO_EXACT(1);
    else if (nv == 2) VO_EXACT(2);
    else if (nv == 3) VO_EXACT(3);
    else VO_EXACT(4);
#undef VO_EXACT
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// One call of the family.  (On the key axis sp carries {threshold, key_mask, shift, n_keys}.)  Device queries / filters (and, in thr, possibly thresholds) in, the tally's finished cells out;
// asynchronous on the ctx stream.  The argument and state checks are the entry point's (api.hip).  tally comes with everything
// but its cells.
template <class Tally, class Out>
static int vo_launch_similar(oi_index *idx, const float *d_q, uint32_t B, const oi_volume_spec &sp, typename Tally::Thr thr,
                             const uint4 *d_filt, Tally tally, Out *d_out) {
    static_assert(OI_MAX_DIM <= 1024u, "vo_exact_kernel holds a row in at most 4 float4 per lane");
    constexpr VoNames N = Tally::NAMES;
    oi_ctx *ctx = idx->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = idx->n_docs;
    const uint32_t dim = idx->dim;
    const uint64_t n_cells = (uint64_t)B * sp.n_buckets, words = n_cells * Tally::CELL_WORDS;
    const uint2 *attrs = (Tally::KEY_AXIS || d_filt || sp.bucket_width) ? idx->doc_attrs.as<uint2>() : nullptr; // (the key axis always reads the group)
    // state (16 B, see VO_GATE ..) and the cells behind it, zeroed per call; the fallback-run counter lives on
    DevBuf &sb = ctx->buf(N.state), &rb = ctx->buf(N.runs);
    OI_CHECK(sb.ensure(64 + words * 4));
    if (!rb.p) {
        OI_CHECK(rb.ensure(16));
        OI_HIP_CHECK(hipMemsetAsync(rb.p, 0, 16, st));
    }
    uint32_t *state = sb.as<uint32_t>();
    tally.cells = state + 16;
    OI_HIP_CHECK(hipMemsetAsync(sb.p, 0, 64 + words * 4, st));
    const float *q = d_q;
    if (idx->rows_bf16) {
        DevBuf &qr = ctx->buf(N.q_rounded);
        const uint64_t total = (uint64_t)B * dim;
        OI_CHECK(qr.ensure(total * 4));
        OI_CHECK(oi_launch_volume_round_queries(ctx, d_q, total, qr.as<float>()));
        q = qr.as<float>();
    }
    const int mode = ctx->cosine_mode;
    // (an exclusive tally's stream takes the whole batch in one launch, so that a row's candidates all meet in one tile)
    const bool screen = n > 0 && (!Tally::EXCLUSIVE || B <= 64u) && (mode == OI_COSINE_SCREEN || mode == OI_COSINE_SCREEN_COPY) &&
                        oi_index_screenable(idx) && idx->screen_copy.p;
    if constexpr (Tally::EXCLUSIVE) OI_CHECK(tally.begin(ctx, n, screen));
    if (n == 0) {
        // (nothing to tally)
    } else if (!screen) {
        ProfScope ps(ctx, N.exact);
        if (idx->rows_bf16) OI_CHECK(vo_launch_exact<true>(ctx, idx->rows_bf16, n, dim, q, B, thr, nullptr, d_filt, attrs, sp, tally));
        else OI_CHECK(vo_launch_exact<false>(ctx, idx->rows, n, dim, q, B, thr, nullptr, d_filt, attrs, sp, tally));
    } else {
        const uint32_t n_padded = (B + 31u) & ~31u;
        DevBuf &qb = ctx->buf(N.q_bf16), &bb = ctx->buf("volume_band"); // (one band buffer for the family: one call at a time)
        const size_t qb_bytes = (sizeof(uint16_t) * (size_t)(n_padded + 64) * dim + 255) & ~(size_t)255;
        OI_CHECK(qb.ensure(qb_bytes + sizeof(float) * B));
        OI_CHECK(bb.ensure(sizeof(uint64_t) * (size_t)VO_BAND_CAP));
        uint16_t *q16 = qb.as<uint16_t>();
        float *eps2 = reinterpret_cast<float *>(qb.as<unsigned char>() + qb_bytes);
        OI_CHECK(oi_launch_screen_stage(ctx, q, B, dim, idx->max_row_norm.as<uint32_t>(), q16, eps2, state + VO_GATE));
        const uint32_t *lbm = idx->n_long ? idx->long_bitmap.as<uint32_t>() : nullptr;
        const uint32_t *llist = idx->n_long ? idx->long_list.as<uint32_t>() : nullptr;
        uint32_t grid = 0, seg_cap = 0;
        oi_cosine_screen_geometry(ctx, n, &grid, &seg_cap); // (the persistent grid of the screens: 7/8 of the CUs)
        {
            ProfScope ps(ctx, N.stream);
            for (uint32_t q0 = 0; q0 < B; q0 += 64) { // the slice of every per-query argument for the queries q0 .. q0 + nq
                const uint32_t nq = std::min(64u, B - q0);
                const uint16_t *qp = q16 + (uint64_t)q0 * dim;
                const uint4 *fp = d_filt ? d_filt + q0 : nullptr;
                const typename Tally::Thr tp = Tally::thr_block(thr, q0);
                Tally tb = tally;
                tb.cells += (uint64_t)q0 * sp.n_buckets * Tally::CELL_WORDS;
#define VO_SCREEN(DD, T)                                                                                                           \
    OI_CHECK(d_filt ? (vo_launch_stream<DD, T, true>(ctx, grid, idx->screen_copy.as<uint16_t>(), n, qp, nq, q0, tp, eps2 + q0, state, \
                                                     fp, attrs, sp, lbm, tb, bb.as<uint64_t>()))                                   \
                    : (vo_launch_stream<DD, T, false>(ctx, grid, idx->screen_copy.as<uint16_t>(), n, qp, nq, q0, tp, eps2 + q0, state, \
                                                      fp, attrs, sp, lbm, tb, bb.as<uint64_t>())))
                if (dim == 768) { if (nq > 32) VO_SCREEN(768, 2); else VO_SCREEN(768, 1); }
                else { if (nq > 32) VO_SCREEN(384, 2); else VO_SCREEN(384, 1); }
#undef VO_SCREEN
            }
        }
        {
            ProfScope ps(ctx, N.band);
            hipLaunchKernelGGL(vo_band_kernel<Tally>, dim3((uint32_t)ctx->num_cus * 4), dim3(256), 0, st, idx->rows, dim, q, B, thr,
                               bb.as<uint64_t>(), VO_BAND_CAP, state, llist, idx->n_long, d_filt, attrs, sp.stamp_origin, sp.bucket_width,
                               sp.n_buckets, tally);
            OI_HIP_CHECK(hipGetLastError());
            if constexpr (Tally::EXCLUSIVE) OI_CHECK(tally.commit(ctx, bb.as<uint64_t>(), state, B, llist, idx->n_long, attrs, sp));
        }
        {
            // the gated fallback: both launches exit at once unless the band overflowed or a query has no bound
            ProfScope ps(ctx, N.fallback);
            if constexpr (Tally::EXCLUSIVE) {
                const uint64_t most = std::max<uint64_t>(words, tally.labels ? n : 0);
                hipLaunchKernelGGL(vo_fallback_clear_kernel<Tally>, dim3((uint32_t)std::min<uint64_t>((most + 255) / 256, 1024)), dim3(256), 0,
                                   st, tally.cells, words, tally.labels, n, state, rb.as<uint32_t>());
            } else {
                hipLaunchKernelGGL(vo_fallback_clear_kernel<Tally>, dim3((uint32_t)std::min<uint64_t>((words + 255) / 256, 1024)), dim3(256), 0,
                                   st, tally.cells, words, state, rb.as<uint32_t>());
            }
            OI_HIP_CHECK(hipGetLastError());
            OI_CHECK(vo_launch_exact<false>(ctx, idx->rows, n, dim, q, B, thr, state, d_filt, attrs, sp, tally));
        }
    }
    return tally.finish(ctx, n_cells, d_out);
}
