// cosine_summary.hip -- oi_similar_summary: the social_summary sums of the documents like a query, per time bucket
// (DESIGN 4.11), and the signal records of an index they are summed from (oi_index_set_signals).
//
// The sibling of cosine_volume.hip: the same three clauses decide which documents a (query, bucket) cell takes -- filter,
// bucket, sim(q, d) >= t_q, with sim the one f32 value of the rescoring chain -- and the same three routes evaluate them
// (oi_volume.h holds what the two files share).  What differs is the epilogue: a hit adds the row's 8-byte SIGNAL RECORD
// {pol_q30, flags} to the cell instead of a 1, and every query brings its own threshold t_q.
//
// A cell is 16 words: 12 u32 counts indexed by the record's flag combination class + 3 spec + 6 source, then the i64 sum of
// pol_q30 (words 12, 13), then two words of padding.  A hit costs ONE u32 atomic, and one 64-bit atomic more only when the
// post's polarity is not zero (most posts hit no lexicon word).  Every sum is an integer sum, so the result does not depend
// on the order of the atomics or on the route that found a hit; summary_finish_kernel folds a cell into oi_social_counters.
#include <algorithm>
#include <cmath>

#include "oi_volume.h"

#define SM_CELL_WORDS 16
#define SM_CELL_SUM 12   // word offset of the i64 sum inside a cell (8-byte aligned: cells are 64 B)
// classes of a record, as social_summary_kernel tests them (speculation_engine.rs:87-95)
#define SM_BULLISH 0u
#define SM_BEARISH 1u
#define SM_NEUTRAL 2u

// One hit: the record sg = {pol_q30 bits, flag combination < 12} of the row goes into cell `cell`.
__device__ __forceinline__ void sm_add(uint32_t *cells, uint64_t cell, const uint2 sg) {
    uint32_t *c = cells + cell * SM_CELL_WORDS;
    atomicAdd(c + sg.y, 1u);
    if (sg.x != 0u)
        atomicAdd(reinterpret_cast<unsigned long long *>(c + SM_CELL_SUM), (unsigned long long)(long long)(int32_t)sg.x);
}

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

// ------------------------------------------------------------------ route 1: the stream
// cosine_volume_screen's tile loop, ring, register-resident queries and band staging, with the summing epilogue and
// per-query thresholds.  sig: the index's signal records, read only for rows with a proven hit.
template <int D, int NQT, int NBUF, bool FILT>
__global__ __launch_bounds__(256, 1) void cosine_summary_screen(
    const uint16_t *__restrict__ rows, uint64_t n_rows,
    const uint16_t *__restrict__ queries, // bf16 [32*NQT][D], zero padded (pf_stage_queries_kernel)
    uint32_t n_queries, uint32_t q_base, float thr, const float *__restrict__ thr_q /* [n_queries] or null: thr for all */,
    const float *__restrict__ eps2, const uint32_t *__restrict__ state_in,
    const uint4 *__restrict__ filt, const uint2 *__restrict__ attrs, uint32_t origin, uint32_t width, uint32_t n_buckets,
    const uint32_t *__restrict__ long_bitmap, const uint2 *__restrict__ sig, uint32_t *cells, uint64_t *band, uint32_t band_cap, uint32_t *band_cnt,
    uint32_t *overflow) {
    constexpr int NKC = D / VO_SLOT_K;    // ring slots per tile
    constexpr int P = NBUF - 1;           // slots in flight ahead of the one being consumed
    constexpr int KSTEPS = D / 16;        // MFMA groups per tile: four per slot
    constexpr uint32_t RING = NBUF * VO_SLOT_BYTES;
    static_assert(D % VO_SLOT_K == 0 && P >= 1 && P <= 2 * NKC, "unsupported ring depth for this D");
    static_assert(NQT * KSTEPS * 4 <= 400, "the query block must fit the register file");
    static_assert(4 * RING + 4 * OI_STAGE * 8 <= 160 * 1024, "LDS");

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    unsigned char *ring = smem; // [4][NBUF][4 KiB]

    if (state_in[VO_GATE] != 0u) return; // a query of the batch has no bound: route 2 sums the batch (uniform over the grid)
    OI_CLAIM_WHOLE_SIMD(); // (MFMA kernel: nothing else may run on this CU -- oi_device.h)
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t li = lane & 31, lh = lane >> 5;
    uint64_t *stage_keys = reinterpret_cast<uint64_t *>(smem + 4 * RING) + w * OI_STAGE; // the wave's staged band pairs
    uint32_t st_head = 0, st_n = 0; // wave-uniform: first staged entry (mod OI_STAGE), staged entries (< OI_STAGE_FLUSH between tiles)

    // ---- every query over the whole K, in registers for the whole launch: B[k = 16 s + 8 lh + 0..7][n = li]
    vo_bf16x8 qreg[NQT][KSTEPS];
#pragma unroll
    for (int t = 0; t < NQT; ++t)
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
            qreg[t][s] = *reinterpret_cast<const vo_bf16x8 *>(queries + (uint64_t)(32 * t + li) * D + 16 * s + 8 * lh);
    // the two thresholds of the queries this lane tests, from the query's OWN t_q, rounded OUTWARD (eps_q is half of what the
    // staging kernel stores); no query in the slot, or a NaN t_q = NaN, which no score is >=
    float lo[NQT], hi[NQT];
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const uint32_t q = 32u * t + li;
        lo[t] = hi[t] = __builtin_nanf("");
        if (q < n_queries) {
            const float e = 0.5f * eps2[q], tq = thr_q ? thr_q[q] : thr;
            lo[t] = nextafterf(tq - e, -__builtin_inff());
            hi[t] = nextafterf(tq + e, __builtin_inff());
        }
    }

    // ---- tiles of this WAVE: (blockIdx.x * 4 + w), + 4 * gridDim.x, ...
    const uint64_t n_tiles = (n_rows + VO_TILE_ROWS - 1) / VO_TILE_ROWS;
    const uint64_t first = (uint64_t)blockIdx.x * 4 + w, stride = (uint64_t)gridDim.x * 4;
    const uint64_t my_nt = first < n_tiles ? (n_tiles - first + stride - 1) / stride : 0;

    if (my_nt) {
        uint32_t voff[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const uint32_t prow = 8 * m + (lane >> 3);
            voff[m] = prow * (uint32_t)(D * 2) + (((lane & 7) ^ ((prow >> 1) & 7)) << 4);
        }
        const uint32_t ring_w = oi_lds_addr(ring) + w * RING;
        const unsigned char *ring_rd = ring + w * RING;
        uint32_t frag_off[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) frag_off[g] = li * 128 + (((2 * g + lh) ^ ((li >> 1) & 7)) << 4);

        auto tile_row0 = [&](uint64_t ti) { return (first + ti * stride) * (uint64_t)VO_TILE_ROWS; };
        auto tile_srd = [&](uint64_t ti) { // past this wave's last tile: an EMPTY descriptor (loads return zeros)
            const uint64_t r0 = tile_row0(ti < my_nt ? ti : 0);
            return oi_make_srd(rows + r0 * D, ti < my_nt ? (n_rows - r0) * (uint64_t)(D * 2) : 0ull);
        };
        oi_u32x4 s0 = tile_srd(0), s1 = tile_srd(1), s2 = tile_srd(2);
        // Every load hipcc knows about (queries, margins) is retired HERE, with a wait it models (oi_lds_dma.h)
        __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0) only
        oi_static_for<0, P>([&](auto j_) { // prologue: logical slots 0..P-1 (tile j / NKC, slot j % NKC) into ring slots 0..P-1
            constexpr int j = decltype(j_)::value;
            constexpr int tj = j / NKC, kj = j % NKC;
#pragma unroll
            for (int m = 0; m < 4; ++m)
                oi_dma_piece(tj == 0 ? s0 : (tj == 1 ? s1 : s2), voff[m], kj * 128, ring_w + j * VO_SLOT_BYTES + m * 1024);
        });
        uint32_t rd_off = 0, wr_off = (NBUF - 1) * VO_SLOT_BYTES;

        for (uint64_t ti = 0; ti < my_nt; ++ti) {
            vo_f32x16 acc[NQT];
#pragma unroll
            for (int t = 0; t < NQT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

            oi_wait_vm<4 * (P - 1)>();
            vo_bf16x8 a_cur = *reinterpret_cast<const vo_bf16x8 *>(ring_rd + rd_off + frag_off[0]);
            oi_static_for<0, NKC * 4>([&](auto gi_) {
                constexpr int gi = decltype(gi_)::value;
                constexpr int kc = gi / 4, g = gi % 4;
                constexpr int sn = kc + P;           // logical slot (relative to this tile) refilled during this slot
                constexpr int tn = sn / NKC, kn = sn % NKC;
                vo_bf16x8 a_nxt = a_cur;
                if constexpr (g < 3) a_nxt = *reinterpret_cast<const vo_bf16x8 *>(ring_rd + rd_off + frag_off[g + 1]);
#pragma unroll
                for (int t = 0; t < NQT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_cur, qreg[t][gi], acc[t], 0, 0, 0);
                oi_dma_piece(tn == 0 ? s0 : (tn == 1 ? s1 : s2), voff[g], kn * 128, ring_w + wr_off + g * 1024);
                if constexpr (g == 3) {
                    wr_off = rd_off;
                    rd_off = rd_off + VO_SLOT_BYTES == RING ? 0u : rd_off + VO_SLOT_BYTES;
                    if constexpr (kc + 1 < NKC) {
                        oi_wait_vm<4 * (P - 1)>();
                        a_nxt = *reinterpret_cast<const vo_bf16x8 *>(ring_rd + rd_off + frag_off[0]);
                    }
                }
                a_cur = a_nxt;
            });

            // ---- the summing epilogue, straight out of the accumulators: register r of query tile t holds
            // D[row (r&3) + 8 (r>>2) + 4 lh][query 32 t + li].  The test costs what the screen's costs (one compare per score);
            // everything else is behind the ballot.
            const uint64_t row0 = tile_row0(ti);
            uint32_t m = 0;
#pragma unroll
            for (int t = 0; t < NQT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) m |= acc[t][r] >= lo[t] ? 1u << (16 * t + r) : 0u;
            if (__builtin_amdgcn_ballot_w64(m != 0u) != 0ull) {
                if (n_rows - row0 < (uint64_t)VO_TILE_ROWS) { // the ragged last tile: rows past the end read as zeros
                    const uint32_t left = (uint32_t)(n_rows - row0);
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if ((uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * lh >= left) m &= ~(0x00010001u << r);
                }
                if constexpr (FILT) m = oi_filter_tile<NQT>(m, filt, attrs, row0, lh, li);
                // per row with a bit left: its bucket (the stamp is loaded for such rows only) and the long-row bitmap; then
                // a proven hit adds the row's signal record (loaded at the row's first proven hit) to its cell, a band pair
                // keeps its bit
                uint32_t mb = 0;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (m & (0x00010001u << r)) {
                        const uint32_t row = (uint32_t)row0 + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * lh;
                        uint32_t b = 0;
                        bool ok = true;
                        if (width != 0u) ok = vo_bucket(attrs[row].y, origin, width, n_buckets, &b);
                        if (long_bitmap && ((long_bitmap[row >> 5] >> (row & 31)) & 1u)) ok = false; // (the bound does not hold: band kernel)
                        if (ok) {
                            bool have = false;
                            uint2 sg = make_uint2(0u, 0u);
#pragma unroll
                            for (int t = 0; t < NQT; ++t)
                                if (m & (1u << (16 * t + r))) {
                                    if (acc[t][r] >= hi[t]) {
                                        if (!have) { sg = sig[row]; have = true; }
                                        sm_add(cells, (uint64_t)(32u * t + li) * n_buckets + b, sg);
                                    } else mb |= 1u << (16 * t + r);
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
                                    const uint32_t row = (uint32_t)row0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
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
                                    const uint32_t row = (uint32_t)row0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                                    if (pos < band_cap && pos >= base) band[pos] = ((uint64_t)(q_base + 32u * t + li) << 32) | row;
                                    else *overflow = 1u;
                                    ++pos;
                                }
                    }
                }
            }
            s0 = s1;
            s1 = s2;
            s2 = tile_srd(ti + 3);
        }
        if (st_n) {
            VO_STAGE_FLUSH_TO_BAND(st_n);
        }
        oi_wait_vm<0>(); // the zero-filling refills issued past the last tile have landed before the LDS goes back
    }
}

// ------------------------------------------------------------------ route 1: the band and the long rows
// volume_band_kernel with the query's own threshold and the record's atomics.
__global__ __launch_bounds__(256) void summary_band_kernel(const float *__restrict__ rows, uint32_t dim, const float *__restrict__ queries,
                                                           uint32_t n_queries, float thr, const float *__restrict__ thr_q,
                                                           const uint64_t *__restrict__ band, uint32_t band_cap,
                                                           const uint32_t *__restrict__ state, const uint32_t *__restrict__ long_list,
                                                           uint32_t n_long, const uint4 *__restrict__ filt, const uint2 *__restrict__ attrs,
                                                           uint32_t origin, uint32_t width, uint32_t n_buckets,
                                                           const uint2 *__restrict__ sig, uint32_t *cells) {
    if ((state[VO_GATE] | state[VO_OVERFLOW]) != 0u) return; // route 2 sums the batch
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
            const float s = oi_wave_sum(a[u]);
            if (lane == 0 && i0 + u < c && s >= (thr_q ? thr_q[q[u]] : thr)) {
                uint32_t b = 0;
                bool ok = true;
                if (attrs) {
                    const uint2 at = attrs[row[u]];
                    if (filt) ok = oi_doc_passes(filt[q[u]], at);
                    ok = ok && vo_bucket(at.y, origin, width, n_buckets, &b);
                }
                if (ok) sm_add(cells, (uint64_t)q[u] * n_buckets + b, sig[row[u]]);
            }
        }
    }
}

// ------------------------------------------------------------------ route 2: exact for every shape
// volume_exact_kernel's shape: a wave holds its row (and now its record) and runs the chain against the queries, four at a
// time.  state != null: the gated fallback of route 1.
template <int NV, bool BF16>
__global__ __launch_bounds__(256) void summary_exact_kernel(const void *__restrict__ rows, uint64_t n_rows, uint32_t dim,
                                                            const float *__restrict__ queries, uint32_t n_queries, float thr,
                                                            const float *__restrict__ thr_q, const uint32_t *__restrict__ state,
                                                            const uint4 *__restrict__ filt, const uint2 *__restrict__ attrs,
                                                            uint32_t origin, uint32_t width, uint32_t n_buckets,
                                                            const uint2 *__restrict__ sig, uint32_t *cells) {
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
            if (!vo_bucket(at.y, origin, width, n_buckets, &b)) continue; // (wave-uniform)
        }
        const uint2 sg = sig[r];
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
                if (lane == 0 && q0 + u < n_queries && s >= (thr_q ? thr_q[q0 + u] : thr) && (!filt || oi_doc_passes(filt[q0 + u], at)))
                    sm_add(cells, (uint64_t)(q0 + u) * n_buckets + b, sg);
            }
        }
    }
}

// The fallback begins: ALL 16 words of every cell of the abandoned screen route are cleared, the i64 sums included, and the
// run is counted (oi_profile_read).
__global__ __launch_bounds__(256) void summary_fallback_clear_kernel(uint32_t *cells, uint64_t words, const uint32_t *__restrict__ state,
                                                                     uint32_t *runs) {
    if ((state[VO_GATE] | state[VO_OVERFLOW]) == 0u) return;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x) cells[i] = 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(runs, 1u);
}

// A cell's 12 counts folded into the caller's record; polarity_sum = (double)(sum of pol_q30) * 2^-30, one rounding at most
// (the conversion: the scaling by a power of two is exact).
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

// ------------------------------------------------------------------ host
int oi_launch_pack_signals(oi_ctx *ctx, const double *d_pol, const uint8_t *d_spec, const uint8_t *d_sources, uint64_t n, double tau,
                           uint2 *d_out) {
    if (n == 0) return OI_OK;
    hipLaunchKernelGGL(summary_pack_signals_kernel, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 4096)), dim3(256), 0, ctx->stream,
                       d_pol, d_spec, d_sources, n, tau, d_out);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// what every launch of a call shares
struct SummaryArgs {
    float thr;            // used when thr_q is null
    const float *thr_q;   // [n_queries] device, or null
    const uint4 *filt;
    const uint2 *attrs;
    uint32_t origin, width, n_buckets;
    const uint2 *sig;
    uint32_t *cells;
};

template <int D, int NQT, bool FILT>
static int launch_summary_screen(oi_ctx *ctx, uint32_t grid, const uint16_t *rows, uint64_t n, const uint16_t *q, uint32_t nq, uint32_t q0,
                                 const float *eps2, uint32_t *state, const SummaryArgs &a, const uint32_t *long_bitmap, uint64_t *band) {
    constexpr size_t smem = 4 * VO_NBUF * VO_SLOT_BYTES + 4 * OI_STAGE * 8;
    OI_CHECK(oi_dyn_lds(ctx, reinterpret_cast<const void *>(cosine_summary_screen<D, NQT, VO_NBUF, FILT>), smem));
    hipLaunchKernelGGL((cosine_summary_screen<D, NQT, VO_NBUF, FILT>), dim3(grid), dim3(256), smem, ctx->stream, rows, n, q, nq, q0, a.thr,
                       a.thr_q ? a.thr_q + q0 : nullptr, eps2, state, a.filt ? a.filt + q0 : nullptr, a.attrs, a.origin, a.width,
                       a.n_buckets, long_bitmap, a.sig, a.cells + (uint64_t)q0 * a.n_buckets * SM_CELL_WORDS, band, VO_BAND_CAP,
                       state + VO_BAND_CNT, state + VO_OVERFLOW);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

template <bool BF16>
static int launch_summary_exact(oi_ctx *ctx, const void *rows, uint64_t n, uint32_t dim, const float *q, uint32_t B, const uint32_t *state,
                                const SummaryArgs &a) {
    const uint32_t nv = (dim / 4 + 63) / 64; // float4 per lane: 1 .. 4 (OI_MAX_DIM = 1024)
    const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((n + 3) / 4, (uint64_t)ctx->num_cus * 8));
#define SM_EXACT(NV)                                                                                                               \
    hipLaunchKernelGGL((summary_exact_kernel<NV, BF16>), dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, rows, n, dim, q, B, a.thr, \
                       a.thr_q, state, a.filt, a.attrs, a.origin, a.width, a.n_buckets, a.sig, a.cells)
    if (nv <= 1) SM_EXACT(1);
    else if (nv == 2) SM_EXACT(2);
    else if (nv == 3) SM_EXACT(3);
    else SM_EXACT(4);
#undef SM_EXACT
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// Device queries / thresholds / filters in, device records out; asynchronous on the ctx stream.  The argument and state
// checks are the entry point's (api.hip).  The route is chosen exactly as oi_launch_similar_volume chooses it.
int oi_launch_similar_summary(oi_index *idx, const float *d_q, uint32_t B, const oi_summary_spec &sp, const float *d_thr,
                              const uint4 *d_filt, oi_social_counters *d_out) {
    static_assert(OI_MAX_DIM <= 1024u, "summary_exact_kernel holds a row in at most 4 float4 per lane");
    static_assert(sizeof(oi_social_counters) == 64, "one record per cell");
    oi_ctx *ctx = idx->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = idx->n_docs;
    const uint32_t dim = idx->dim;
    const uint64_t n_cells = (uint64_t)B * sp.n_buckets, words = n_cells * SM_CELL_WORDS;
    // state (VO_GATE ..: the volume's words) and the cells behind it, zeroed per call; the fallback-run counter lives on
    DevBuf &sb = ctx->buf("summary_state"), &rb = ctx->buf("summary_runs");
    OI_CHECK(sb.ensure(64 + words * 4));
    if (!rb.p) {
        OI_CHECK(rb.ensure(16));
        OI_HIP_CHECK(hipMemsetAsync(rb.p, 0, 16, st));
    }
    uint32_t *state = sb.as<uint32_t>();
    OI_HIP_CHECK(hipMemsetAsync(sb.p, 0, 64 + words * 4, st));
    SummaryArgs a;
    a.thr = sp.threshold;
    a.thr_q = d_thr;
    a.filt = d_filt;
    a.attrs = (d_filt || sp.bucket_width) ? idx->doc_attrs.as<uint2>() : nullptr;
    a.origin = sp.stamp_origin;
    a.width = sp.bucket_width;
    a.n_buckets = sp.n_buckets;
    a.sig = idx->signals.as<uint2>();
    a.cells = state + 16;
    const float *q = d_q;
    if (idx->rows_bf16) {
        DevBuf &qr = ctx->buf("summary_q_rounded");
        const uint64_t total = (uint64_t)B * dim;
        OI_CHECK(qr.ensure(total * 4));
        OI_CHECK(oi_launch_volume_round_queries(ctx, d_q, total, qr.as<float>()));
        q = qr.as<float>();
    }
    const int mode = ctx->cosine_mode;
    const bool screen = n > 0 && (mode == OI_COSINE_SCREEN || mode == OI_COSINE_SCREEN_COPY) && oi_index_screenable(idx) && idx->screen_copy.p;
    if (n == 0) {
        // (nothing to sum)
    } else if (!screen) {
        ProfScope ps(ctx, "summary_exact");
        if (idx->rows_bf16) OI_CHECK(launch_summary_exact<true>(ctx, idx->rows_bf16, n, dim, q, B, nullptr, a));
        else OI_CHECK(launch_summary_exact<false>(ctx, idx->rows, n, dim, q, B, nullptr, a));
    } else {
        const uint32_t n_padded = (B + 31u) & ~31u;
        DevBuf &qb = ctx->buf("summary_q_bf16"), &bb = ctx->buf("volume_band"); // (the band buffer is the volume's: same size, one call at a time)
        const size_t qb_bytes = (sizeof(uint16_t) * (size_t)(n_padded + 64) * dim + 255) & ~(size_t)255;
        OI_CHECK(qb.ensure(qb_bytes + sizeof(float) * B));
        OI_CHECK(bb.ensure(sizeof(uint64_t) * (size_t)VO_BAND_CAP));
        uint16_t *q16 = qb.as<uint16_t>();
        float *eps2 = reinterpret_cast<float *>(qb.as<unsigned char>() + qb_bytes);
        OI_CHECK(oi_launch_screen_stage(ctx, q, B, dim, idx->max_row_norm.as<uint32_t>(), q16, eps2, state + VO_GATE));
        const uint32_t *lbm = idx->n_long ? idx->long_bitmap.as<uint32_t>() : nullptr;
        uint32_t grid = 0, seg_cap = 0;
        oi_cosine_screen_geometry(ctx, n, &grid, &seg_cap); // (the persistent grid of the screens: 7/8 of the CUs)
        {
            ProfScope ps(ctx, "summary");
            for (uint32_t q0 = 0; q0 < B; q0 += 64) {
                const uint32_t nq = std::min(64u, B - q0);
                const uint16_t *qp = q16 + (uint64_t)q0 * dim;
#define SM_SCREEN(DD, T)                                                                                                              \
    OI_CHECK(d_filt ? (launch_summary_screen<DD, T, true>(ctx, grid, idx->screen_copy.as<uint16_t>(), n, qp, nq, q0, eps2 + q0, state, a, \
                                                          lbm, bb.as<uint64_t>()))                                                    \
                    : (launch_summary_screen<DD, T, false>(ctx, grid, idx->screen_copy.as<uint16_t>(), n, qp, nq, q0, eps2 + q0, state, \
                                                           a, lbm, bb.as<uint64_t>())))
                if (dim == 768) { if (nq > 32) SM_SCREEN(768, 2); else SM_SCREEN(768, 1); }
                else { if (nq > 32) SM_SCREEN(384, 2); else SM_SCREEN(384, 1); }
#undef SM_SCREEN
            }
        }
        {
            ProfScope ps(ctx, "summary_band");
            hipLaunchKernelGGL(summary_band_kernel, dim3((uint32_t)ctx->num_cus * 4), dim3(256), 0, st, idx->rows, dim, q, B, a.thr, a.thr_q,
                               bb.as<uint64_t>(), VO_BAND_CAP, state, idx->n_long ? idx->long_list.as<uint32_t>() : nullptr, idx->n_long,
                               a.filt, a.attrs, a.origin, a.width, a.n_buckets, a.sig, a.cells);
            OI_HIP_CHECK(hipGetLastError());
        }
        {
            // the gated fallback: both launches exit at once unless the band overflowed or a query has no bound
            ProfScope ps(ctx, "summary_fallback");
            hipLaunchKernelGGL(summary_fallback_clear_kernel, dim3((uint32_t)std::min<uint64_t>((words + 255) / 256, 1024)), dim3(256), 0, st,
                               a.cells, words, state, rb.as<uint32_t>());
            OI_HIP_CHECK(hipGetLastError());
            OI_CHECK(launch_summary_exact<false>(ctx, idx->rows, n, dim, q, B, state, a));
        }
    }
    hipLaunchKernelGGL(summary_finish_kernel, dim3((uint32_t)std::min<uint64_t>((n_cells + 255) / 256, 1024)), dim3(256), 0, st, a.cells,
                       n_cells, d_out);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}
