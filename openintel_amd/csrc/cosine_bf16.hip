// cosine_bf16.hip -- the cosine scorer over a bf16 corpus (BASELINE configs[4]: 100M x 1024-d bf16).
//
// Builder-defined like the rest of the retrieval path (the reference has none).  Scores are
// sum_k bf16(q_k) * x_k accumulated in f32 by v_mfma_f32_32x32x16_bf16 (products of two bf16 values
// are exact in f32), i.e. the cosine of the rows AS STORED with the queries rounded to bf16 -- the
// oracle for this kernel does the same rounding and sums in f64.
//
// Regime.  At 2 bytes per element the scorer needs 64 flop per corpus byte at B = 64 while the matrix
// pipes offer ~300: the kernel is HBM-bound (15.4 GB per pass at 10M x 768), so it is built to stream,
// not to keep the MFMA pipe full:
//   * one workgroup per CU, 4 waves, one per SIMD, each owning the full 512-register file.  There is
//     NO K-split here: a wave holds ALL 64 queries over the whole K in registers (64 x 768 bf16 =
//     96 KB = 384 VGPRs per lane, as B operands of the 32x32x16 MFMA) and owns whole 32-row tiles, so
//     waves never meet -- no cross-wave sum, no barrier after the prologue;
//   * each wave streams its tiles through its own LDS ring of 4 KiB slots (32 rows x 128 B = 64 bf16
//     of K): OiCopyRing of oi_screen_tile.h, the ring of the bf16 screens (buffer_load ... lds, P slots
//     ahead, one counted s_waitcnt vmcnt per slot, the prefetch running across tile boundaries and
//     past the last tile against an empty descriptor);
//   * a lane's A fragment (8 consecutive bf16 of its row) is one conflict-free ds_read_b128 per MFMA
//     group; the filter + pool append come straight out of the accumulators (the 32x32 D layout maps
//     a lane to one query column), into this workgroup's private pool segment.
// d = 1024 with 64 queries would need all 512 registers for the queries alone: it runs 32 queries per
// pass (NQT = 1); d = 384 and 768 run 64.
#include <cstdlib>
#include <type_traits>

#include "oi_device.h"
#include "oi_internal.h"
#include "oi_lds_dma.h"
#include "oi_screen_tile.h"

#ifndef OI_BF16_SIB_DEFAULT
#define OI_BF16_SIB_DEFAULT 2 // (round 5: 256-query batches at d = 1024 take their two passes as sibling workgroups on one XCD)
#endif

// ---- ring depth and dynamic LDS of each kernel: what the kernel lays its LDS out by and what its launch asks for
// Solo: the depth that divides the tile's slot count, 8 or 6 slots (the compile-time ring this kernel had needed that; the
// depths stay, they are what was measured).  Behind the four rings: seg_fill[64].
constexpr int cb_solo_nbuf(int d) { return d / OI_SLOT_K % 8 == 0 ? 8 : (d / OI_SLOT_K % 6 == 0 ? 6 : d / OI_SLOT_K); }
constexpr size_t cb_solo_lds(int d) { return oi_ring_lds(cb_solo_nbuf(d)) + 64 * 4; }
// Pair: a wave's half of a tile.  Behind the rings: one partial tile per pair (16 NQT floats per lane), then seg_fill[128].
constexpr int cb_pair_nbuf(int d) { return d / 2 / OI_SLOT_K; }
constexpr int cb_pair_red(int nqt) { return nqt * 16 * 64; }
constexpr size_t cb_pair_lds(int d, int nqt) { return oi_ring_lds(cb_pair_nbuf(d)) + 2 * cb_pair_red(nqt) * 4 + 128 * 4; }
// Query split: a workgroup-shared ring of CQ_NHB half tiles (8 slots each), then seg_fill[128] and the staging ring.
constexpr int CQ_HT_SLOTS = 8;
constexpr uint32_t CQ_HT_BYTES = CQ_HT_SLOTS * OI_SLOT_BYTES;
constexpr int CQ_NHB = 4; // (the refill of half tile h + CQ_NHB is addressed as tile ti + 2)
constexpr size_t CQ_LDS = CQ_NHB * CQ_HT_BYTES + 128 * 4 + OI_STAGE_LDS;

// MFMA with the B operand named as AGPRs.  gfx950's matrix instructions take srcA / srcB from either half of the unified
// register file, but the builtin lets the compiler choose: with more than 256 registers of resident queries it parks the
// excess in AGPRs as SPILL slots and copies four registers back with v_accvgpr_read in front of every MFMA that needs them
// (128 queries split by K over the waves: 304 copies in the tile loop, 8 per group of four MFMAs).  Here the
// whole query block lives in AGPRs and is read from there; the accumulators stay in VGPRs (the epilogue stores them to LDS).
// The compiler does not see the matrix pipe's latency through an asm: a reader of `acc` other than the next cb_mfma_agpr of
// the same accumulator must come after cb_mfma_drain().
__device__ __forceinline__ void cb_mfma_agpr(oi_f32x16 &acc, const oi_bf16x8 &a, const oi_bf16x8 &b) {
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(a), "a"(b));
}
__device__ __forceinline__ void cb_mfma_agpr_first(oi_f32x16 &acc, const oi_bf16x8 &a, const oi_bf16x8 &b) { // acc = a x b
    asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(a), "a"(b));
}
__device__ __forceinline__ void cb_mfma_drain() { // >= 19 wait states: the last MFMA's result is readable by any instruction
    asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
}

// Thresholds (as keys) of the queries this lane filters; no query in the slot: nothing passes.
template <int NQT>
__device__ __forceinline__ void cb_thresholds(uint32_t (&tau)[NQT], const uint32_t *tau_keys, uint32_t n_queries, uint32_t li) {
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const uint32_t q = 32u * t + li;
        tau[t] = q < n_queries ? tau_keys[q] : 0xFFFFFFFFu;
    }
}

// Filter + append of one tile (first row row0), one pool store per survivor: score(t, r) is the lane's score of query
// 32 t + li against row oi_tile_row(row0, r, lh).  In this order: the row exists, the score is no NaN, its key reaches the
// query's threshold, the document passes the query's filter (FILT).
template <int NQT, bool FILT, class Score>
__device__ __forceinline__ void cb_append(Score score, uint64_t row0, uint64_t row_end, const uint32_t (&tau)[NQT], uint32_t li,
                                          uint32_t lh, uint32_t *seg_fill, uint64_t *my_seg, uint64_t pool_stride, uint32_t seg_cap,
                                          uint32_t doc_id_base, uint32_t *overflow, const uint4 *__restrict__ filt,
                                          const uint2 *__restrict__ attrs) {
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const uint32_t q = 32u * t + li;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint64_t row = row0 + oi_tile_row(0u, r, lh);
            const float s = score(t, r);
            if (row < row_end && s == s && oi_f32_key(s) >= tau[t] && (!FILT || oi_doc_passes(filt[q], attrs[row]))) {
                const uint32_t pos = atomicAdd(&seg_fill[q], 1u); // LDS
                if (pos < seg_cap) my_seg[(uint64_t)q * pool_stride + pos] = oi_rank_key(s, doc_id_base + (uint32_t)row);
                else *overflow = 1u;
            }
        }
    }
}

template <int D, int NQT, bool FILT>
__global__ __launch_bounds__(256, 1) void cosine_bf16_filter(
    const uint16_t *__restrict__ rows, uint64_t row_begin, uint64_t row_end,
    const uint16_t *__restrict__ queries, // bf16 [32*NQT][D], zero padded
    uint32_t n_queries, uint32_t doc_id_base, uint64_t *pools, uint32_t *seg_cnt, uint32_t seg_cnt_stride,
    const uint32_t *tau_keys, uint64_t pool_stride, uint32_t carry_cap, uint32_t seg_cap, uint32_t *overflow,
    const uint4 *__restrict__ filt, const uint2 *__restrict__ attrs) { // FILT: the doc filter after the threshold
    constexpr int NBUF = cb_solo_nbuf(D);
    using Ring = OiCopyRing<D, NBUF>;

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];              // [4][NBUF][4 KiB] of ring, then
    uint32_t *seg_fill = reinterpret_cast<uint32_t *>(smem + oi_ring_lds(NBUF));        // [32*NQT]

    OI_CLAIM_WHOLE_SIMD(); // (MFMA kernel: nothing else may run on this CU -- oi_device.h)
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t li = lane & 31, lh = lane >> 5;

    oi_bf16x8 qreg[NQT][D / 16];
    oi_tile_load_queries<D, NQT>(qreg, queries, li, lh);
    uint32_t tau[NQT];
    cb_thresholds<NQT>(tau, tau_keys, n_queries, li);
    if (tid < 32 * NQT) seg_fill[tid] = 0;
    __syncthreads(); // the only barrier before the close: seg_fill is zero before any wave appends

    const OiWaveTiles wt = oi_wave_tiles(row_begin, row_end, w);
    uint64_t *my_seg = pools + carry_cap + (uint64_t)blockIdx.x * seg_cap;
    if (wt.my_nt) {
        Ring ring;
        ring.begin(wt, rows, smem + w * Ring::BYTES, lane);
        for (uint64_t ti = 0; ti < wt.my_nt; ++ti) {
            oi_f32x16 acc[NQT];
            ring.template tile<NQT>(acc, qreg);
            cb_append<NQT, FILT>([&](int t, int r) { return acc[t][r]; }, wt.row0(ti), row_end, tau, li, lh, seg_fill, my_seg,
                                 pool_stride, seg_cap, doc_id_base, overflow, filt, attrs);
            ring.next(wt, rows, ti);
        }
        ring.end();
    }
    oi_pool_close<NQT>(seg_fill, seg_cap, n_queries, seg_cnt, seg_cnt_stride, blockIdx.x);
}

// ------------------------------------------------------------------ more queries per corpus pass
// The kernel above reads the corpus once per 64 queries (32 at d = 1024): at B = 256 that is 4-8 passes
// of an HBM-bound scan.  Here the four waves work as TWO PAIRS; a pair owns whole 32-row tiles and each
// of its waves holds one HALF of K of up to 128 queries in registers (128 x 384 bf16 = 96 KB), streams
// its half of the rows through its own ring (the same OiCopyRing, over a K-slice of D / 2 at kh * D bytes
// into every row), and the two partial 32 x 128 tiles meet once per tile:
// one wave writes its accumulators to LDS, one workgroup barrier, the other adds them to its own and
// filters.  The roles alternate from tile to tile, which balances the epilogue work and makes the one
// barrier enough (a wave has finished reading the buffer before it becomes the writer).
// seg_cnt and its stride, read only at the close, are the LAST arguments here: next to pools hipcc fetches the two pointers
// with one s_load_dwordx4 ahead of the tile loop and holds seg_cnt over the loop in SGPRs this kernel does not have (4 spilled
// to VGPR lanes at d = 768 and 1024; tests/test_screen_ring_schedule.py).
template <int D, int NQT>
__global__ __launch_bounds__(256, 1) void cosine_bf16_pair(
    const uint16_t *__restrict__ rows, uint64_t row_begin, uint64_t row_end,
    const uint16_t *__restrict__ queries, // bf16 [32*NQT][D], zero padded
    uint32_t n_queries, uint32_t doc_id_base, uint64_t *pools, const uint32_t *tau_keys, uint64_t pool_stride,
    uint32_t carry_cap, uint32_t seg_cap, uint32_t *overflow, uint32_t *seg_cnt, uint32_t seg_cnt_stride) {
    constexpr int KH = D / 2;                 // K of one wave
    constexpr int NBUF = cb_pair_nbuf(D);     // a half tile's slots
    constexpr int RED = cb_pair_red(NQT);     // floats of one partial tile
    using Ring = OiCopyRing<D, NBUF, oi_dma_piece_stream, KH>;
    static_assert(cb_pair_lds(D, NQT) <= 160 * 1024, "LDS");

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];           // [4][NBUF][4 KiB] of ring, then
    float *red = reinterpret_cast<float *>(smem + oi_ring_lds(NBUF));                // [2 pairs][RED]
    uint32_t *seg_fill = reinterpret_cast<uint32_t *>(red + 2 * RED);                // [32*NQT]

    OI_CLAIM_WHOLE_SIMD(); // (MFMA kernel: nothing else may run on this CU -- oi_device.h)
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t pr = w >> 1, kh = w & 1;
    const uint32_t li = lane & 31, lh = lane >> 5;

    oi_bf16x8 qreg[NQT][KH / 16]; // this wave's half of K of every query
    oi_tile_load_queries<D, NQT, KH>(qreg, queries, li, lh, kh * KH);
    uint32_t tau[NQT];
    cb_thresholds<NQT>(tau, tau_keys, n_queries, li);
    if (tid < 32 * NQT) seg_fill[tid] = 0;
    __syncthreads();

    // ---- tiles of this PAIR: (blockIdx.x * 2 + pr), + 2 * gridDim.x, ...  Both pairs run the same number of loop trips (the
    // barrier is workgroup-wide): pair 0's, which has the most.  A pair past its last tile needs no test of its own: its
    // descriptor is empty, it streams zeros, and the rows of the tile it addresses lie at or past row_end, so nothing is appended.
    const OiWaveTiles wt = oi_owner_tiles(row_begin, row_end, (uint64_t)blockIdx.x * 2 + pr, (uint64_t)gridDim.x * 2);
    const uint64_t trips = oi_owner_tiles(row_begin, row_end, (uint64_t)blockIdx.x * 2, (uint64_t)gridDim.x * 2).my_nt;
    uint64_t *my_seg = pools + carry_cap + (uint64_t)blockIdx.x * seg_cap;
    float *my_red = red + pr * RED;

    Ring ring;
    ring.begin(wt, rows, smem + w * Ring::BYTES, lane, kh * (uint32_t)(KH * 2));
    // The ring offsets stay the run-time scalars the ring is written for.  NBUF is the half tile's slot count, so without
    // this hipcc proves them constant at every tile's start, turns the 4 NBUF LDS addresses of the pieces into loop
    // invariants and runs out of SGPRs holding them (24 spilled at d = 1024).
    asm volatile("" : "+s"(ring.rd_off), "+s"(ring.wr_off));
    for (uint64_t ti = 0; ti < trips; ++ti) {
        oi_f32x16 acc[NQT];
        ring.template tile<NQT>(acc, qreg);
        // ---- the pair's two halves meet: the writer of this trip parks its partial tile in LDS
        const bool writer = ((ti + kh) & 1) == 0;
        if (writer) {
#pragma unroll
            for (int t = 0; t < NQT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) my_red[(t * 16 + r) * 64 + lane] = acc[t][r];
        }
        __syncthreads();
        if (!writer)
            cb_append<NQT, false>(
                [&](int t, int r) {
                    const float other = my_red[(t * 16 + r) * 64 + lane];
                    return kh == 0 ? acc[t][r] + other : other + acc[t][r]; // (K half 0) + (K half 1)
                },
                wt.row0(ti), row_end, tau, li, lh, seg_fill, my_seg, pool_stride, seg_cap, doc_id_base, overflow, nullptr, nullptr);
        ring.next(wt, rows, ti);
    }
    ring.end();
    oi_pool_close<NQT>(seg_fill, seg_cap, n_queries, seg_cnt, seg_cnt_stride, blockIdx.x);
}

// ------------------------------------------------------------------ 128 queries per corpus pass, split by QUERY
// configs[4] is 256 queries at d = 1024: 32 per pass with the solo kernel, 96 with the pair kernel (three passes).  One CU
// cannot hold more than 128 queries (the 256 x 1024 bf16 block IS the register file of a CU): here a workgroup takes 128, two
// passes.  The four waves split the QUERIES: wave w holds queries 32 w .. 32 w + 31 over the WHOLE K (32 x 1024 bf16 = 64 KB =
// 256 AGPRs), every tile is DMA'd into LDS once (each wave loads a quarter of it) and read by all four waves.  A wave's
// accumulators hold complete scores: no partial tiles, no cross-wave reduction (a K split over the waves spent 2.2 of its
// 8.3 ms per 256-query batch at a 12.5M-row shard on parking and summing partial tiles: DESIGN.md 4.2), and a score is one MFMA
// accumulation chain in K order -- the same bits whatever the query's slot in the batch.  The price is LDS read traffic: every
// fragment feeds ONE MFMA instead of four, 256 KB of ds_read_b128 per tile and CU = 2048 LDS cycles beside 2048 matrix-pipe
// cycles per wave; the kernel is built to keep both busy:
//   * the tile moves as two HALF tiles (512 k = 8 slots of 4 KiB, 32 KB) through a ring of CQ_NHB half-tile buffers; wave w
//     issues the DMA pieces of slots 2 w, 2 w + 1 of every half tile, three half tiles ahead;
//   * ONE barrier per half tile does both jobs: every wave has waited for its own pieces of half tile h (counted vmcnt) before
//     it, so after it all of h is in LDS; and every wave has finished reading h - 1, whose buffer is refilled right after;
//   * fragments are read three slots (4 x 16 B per lane each) ahead of the matrix pipe.
// This ring is workgroup-shared, with a barrier per half tile: another structure than OiCopyRing, and it lives here.
//
// SIBLINGS (SIB = 2).  256 queries are two passes of 128.  With siblings the two passes run as ONE launch: the grid is cut
// into pairs of workgroups that walk the SAME tile sequence, one with queries 0..127 and one with 128..255 (own pool segments,
// own thresholds), so a tile fetched from HBM by whichever sibling gets there first is read by the other out of cache -- HBM
// sees the corpus once per 256 queries instead of twice.  A sibling that hits cache runs faster until it leads and misses: the
// pair stays together by itself, nothing synchronises them.  The siblings are blockIdx 16 a + x and 16 a + 8 + x (x =
// blockIdx % 8): the SAME XCD under round-robin dispatch, so they share its L2.  They read with the default cache policy
// (STREAM off), where a lone pass loads non-temporally: HBM then sees every tile ONCE, 25.63 GB per 256-query batch at
// 12.5M x 1024 by the FETCH_SIZE counter, against 42 GB with non-temporal loads and 51.2 GB without siblings.
template <int SIB>
__global__ __launch_bounds__(256, 1) void cosine_bf16_qsplit(
    const uint16_t *__restrict__ rows, uint64_t row_begin, uint64_t row_end,
    const uint16_t *__restrict__ queries, // bf16 [128 (x 2 with siblings)][1024], zero padded
    uint32_t n_queries, uint32_t doc_id_base, uint64_t *pools, uint32_t *seg_cnt, uint32_t seg_cnt_stride,
    const uint32_t *tau_keys, uint64_t pool_stride, uint32_t carry_cap, uint32_t seg_cap, uint32_t *overflow) {
    constexpr int D = 1024, NHB = CQ_NHB;
    constexpr uint32_t ROW_BYTES = D * 2;
    constexpr bool STREAM = SIB == 0;
    constexpr uint32_t RING = NHB * CQ_HT_BYTES;
    static_assert(NHB == 4 && CQ_LDS <= 160 * 1024, "the refill of half tile h + NHB is addressed as tile ti + 2: NHB = 4");

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    unsigned char *ring = smem;                                                  // [NHB][8 slots][4 KiB]: shared by the four waves
    uint32_t *seg_fill = reinterpret_cast<uint32_t *>(smem + RING);              // [128]
    OI_CLAIM_WHOLE_SIMD(); // (MFMA kernel: nothing else may run on this CU -- oi_device.h)
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);                 // the query tile of this wave
    const uint32_t li = lane & 31, lh = lane >> 5;
    uint64_t *stage_keys = reinterpret_cast<uint64_t *>(smem + RING + 512) + w * OI_STAGE;
    uint32_t *stage_q = reinterpret_cast<uint32_t *>(smem + RING + 512 + 4 * OI_STAGE * 8) + w * OI_STAGE;
    uint32_t st_head = 0, st_n = 0;

    static_assert(SIB == 0 || SIB == 2, "SIB: 0 = a lone pass of 128 queries, 2 = sibling workgroups on one XCD");
    uint32_t half = 0, wg = blockIdx.x, n_wg = gridDim.x; // (siblings: workgroup pair `wg` of n_wg, query half `half`)
    if (SIB == 2) { half = (blockIdx.x >> 3) & 1u; wg = ((blockIdx.x >> 4) << 3) | (blockIdx.x & 7u); n_wg = gridDim.x >> 1; }
    if (half) { // (uniform) the second 128 queries: their block of every per-query array
        queries += (uint64_t)128 * D;
        pools += (uint64_t)128 * pool_stride;
        seg_cnt += (uint64_t)128 * seg_cnt_stride;
        tau_keys += 128;
        n_queries = n_queries > 128u ? n_queries - 128u : 0u;
    } else if (SIB && n_queries > 128u) n_queries = 128u;

    // ---- this wave's 32 queries over the whole K, in registers: B[k = 16 s + 8 lh + 0..7][n = li]
    oi_bf16x8 qreg[1][D / 16];
    oi_tile_load_queries<D, 1>(qreg, queries + (uint64_t)(32 * w) * D, li, lh);
    const uint32_t my_q = 32u * w + li;
    const uint32_t my_tau = my_q < n_queries ? tau_keys[my_q] : 0xFFFFFFFFu;
    const float tau_f[1] = {my_tau <= 0x007FFFFFu ? -__builtin_inff() : oi_key_f32(my_tau)}; // (no query in the slot: NaN, nothing passes)
    if (tid < 128) seg_fill[tid] = 0;

    const OiWaveTiles wt = oi_owner_tiles(row_begin, row_end, wg, n_wg); // the tiles of this workgroup (pair)
    uint64_t *my_seg = pools + carry_cap + (uint64_t)wg * seg_cap;

    uint32_t voff[4], frag_off[4];
    oi_tile_voff<ROW_BYTES>(voff, lane);
    oi_tile_frag_off(frag_off, li, lh);
    const uint32_t ring_w = oi_lds_addr(ring);

    // this wave's pieces of one half tile (slots 2 w and 2 w + 1): K half `hh` of the tile described by `srd`
    auto issue_slot = [&](const oi_u32x4 &srd, uint32_t hh, uint32_t jj, uint32_t buf_off) __attribute__((always_inline)) {
        const uint32_t j = 2u * w + jj;
#pragma unroll
        for (int m = 0; m < 4; ++m)
            oi_dma_piece<STREAM>(srd, voff[m], hh * 1024u + j * 128u, ring_w + buf_off + j * OI_SLOT_BYTES + m * 1024);
    };
    oi_u32x4 s0 = wt.srd<ROW_BYTES>(rows, 0), s1 = wt.srd<ROW_BYTES>(rows, 1), s2 = wt.srd<ROW_BYTES>(rows, 2);
    oi_tile_retire_visible_loads();
    __syncthreads();                    // seg_fill is zero before any wave appends
    // The slot stream is continuous over half tiles and tiles.  Fragments are read THREE slots ahead of the matrix pipe (a slot
    // is four MFMAs = 128 cycles; one slot ahead, the LDS reads -- four waves' fragment traffic plus the DMA writes on one LDS
    // pipe -- came back after ~250 cycles and every slot waited for them: stream and MFMA time ADDED UP, 5.3 + 2.8 ms per batch
    // at a 12.5M-row shard with and without the matrix instructions).  So the reads of half tile h + 1 begin at slot 5 of half
    // tile h, and the ONE barrier per half tile sits there: before it a wave waits for its own DMA pieces of h + 1 (counted
    // vmcnt) -- after it all of h + 1 is in LDS; and every read of half tile h has been issued (the last ones at slot 4) and,
    // by the barrier's lgkmcnt(0), completed -- its buffer is refilled with half tile h + NHB right after the barrier.
    oi_bf16x8 fr[4][4]; // fragments of slots g, g + 1, g + 2 (and the one being read): slot g lives in fr[g % 4]
    if (wt.my_nt) {
        oi_static_for<0, NHB>([&](auto h_) { // prologue: half tiles 0 .. NHB - 1 (tile h / 2, K half h % 2) fill the ring
            constexpr int h = decltype(h_)::value;
            issue_slot(h / 2 == 0 ? s0 : s1, h % 2, 0, h * CQ_HT_BYTES);
            issue_slot(h / 2 == 0 ? s0 : s1, h % 2, 1, h * CQ_HT_BYTES);
        });
        oi_wait_vm<8 * (NHB - 1)>(); // this wave's pieces of half tile 0 ...
    }
    __syncthreads();              // ... and everyone's
    if (wt.my_nt) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) fr[j][g] = *reinterpret_cast<const oi_bf16x8 *>(ring + j * OI_SLOT_BYTES + frag_off[g]);
    }
    uint32_t rd_off = 0; // the buffer of the half tile the matrix pipe is on

    for (uint64_t ti = 0; ti < wt.my_nt; ++ti) {
        oi_f32x16 acc[1];
        oi_static_for<0, 2>([&](auto hh_) {
            constexpr int hh = decltype(hh_)::value;
            const uint32_t nx_off = rd_off + CQ_HT_BYTES == RING ? 0u : rd_off + CQ_HT_BYTES;
            oi_static_for<0, CQ_HT_SLOTS>([&](auto j_) {
                constexpr int j = decltype(j_)::value;
                if constexpr (j == 5) {
                    oi_wait_vm<8 * (NHB - 2)>(); // this wave's pieces of the NEXT half tile are in LDS ...
                    __syncthreads();          // ... and everyone's; everyone has finished reading THIS half tile's buffer
                }
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    if constexpr (hh == 0 && j == 0) { if (g == 0) cb_mfma_agpr_first(acc[0], fr[0][0], qreg[0][0]); else cb_mfma_agpr(acc[0], fr[0][g], qreg[0][g]); }
                    else cb_mfma_agpr(acc[0], fr[j % 4][g], qreg[0][hh * 32 + j * 4 + g]);
                }
                // fragments of the slot three ahead: this half tile's, or (from slot 5 on) the next one's.  AFTER this slot's MFMAs
                // in program order: the registers they go to fed the PREVIOUS slot's MFMAs, all issued a slot ago.
                {
                    const unsigned char *src = j + 3 < CQ_HT_SLOTS ? ring + rd_off + (j + 3) * OI_SLOT_BYTES
                                                                   : ring + nx_off + (j + 3 - CQ_HT_SLOTS) * OI_SLOT_BYTES;
#pragma unroll
                    for (int g = 0; g < 4; ++g) fr[(j + 3) % 4][g] = *reinterpret_cast<const oi_bf16x8 *>(src + frag_off[g]);
                }
                // the refill of THIS half tile's buffer (free since the barrier): half tile h + NHB = K half hh of tile ti + NHB / 2
                if constexpr (j == 5) issue_slot(s2, hh, 0, rd_off);
                if constexpr (j == 6) issue_slot(s2, hh, 1, rd_off);
            });
            rd_off = nx_off;
        });
        cb_mfma_drain(); // the accumulators are read next

        // ---- filter + append (OiPoolSink::append with one query tile, the wave's: query 32 w + li, segment wg)
        const uint64_t row0 = wt.row0(ti);
        const uint32_t m = oi_tile_mask_ragged(oi_tile_pass_mask<1>(acc, tau_f), row_end - row0, lh);
        if (__builtin_amdgcn_ballot_w64(m != 0u) != 0ull) {
            const uint32_t cnt = (uint32_t)__builtin_popcount(m);
            const uint32_t incl = oi_wave_incl_scan(cnt);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            if (total <= OI_STAGE - OI_STAGE_FLUSH) { // sparse tile: staged in LDS, 64 keys leave with one store instruction
                uint32_t idx = st_head + st_n + incl - cnt;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (m & (1u << r)) {
                        stage_keys[idx & (OI_STAGE - 1)] = oi_rank_key(acc[0][r], doc_id_base + oi_tile_row((uint32_t)row0, r, lh));
                        stage_q[idx & (OI_STAGE - 1)] = my_q;
                        ++idx;
                    }
                st_n += total;
                while (st_n >= OI_STAGE_FLUSH) {
                    OI_STAGE_FLUSH_TO_POOL(OI_STAGE_FLUSH);
                }
            } else { // dense tile (no threshold yet): straight to the pool
                uint32_t pos = atomicAdd(&seg_fill[my_q], cnt);
                uint64_t *dst = my_seg + (uint64_t)my_q * pool_stride;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (m & (1u << r)) {
                        if (pos < seg_cap) dst[pos] = oi_rank_key(acc[0][r], doc_id_base + oi_tile_row((uint32_t)row0, r, lh));
                        else *overflow = 1u;
                        ++pos;
                    }
            }
        }
        s0 = s1;
        s1 = s2;
        s2 = wt.srd<ROW_BYTES>(rows, ti + 3);
    }
    if (st_n) { // the staged rest
        OI_STAGE_FLUSH_TO_POOL(st_n);
    }
    oi_wait_vm<0>(); // the zero-filling refills issued past the last tile have landed before the LDS goes back
    oi_pool_close<4>(seg_fill, seg_cap, n_queries, seg_cnt, seg_cnt_stride, wg);
}

// ------------------------------------------------------------------ query staging: f32 -> bf16 (RNE), zero padded
__global__ __launch_bounds__(256) void cb_stage_queries(const float *__restrict__ q, uint32_t n_queries, uint32_t n_padded,
                                                        uint32_t dim, uint16_t *__restrict__ out) {
    const uint64_t total = (uint64_t)n_padded * dim;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = (uint32_t)(i / dim) < n_queries ? (uint16_t)oi_f32_to_bf16_rne(q[i]) : (uint16_t)0;
}

// ------------------------------------------------------------------ host
bool oi_cosine_bf16_supported(uint32_t dim) { return dim == 384 || dim == 768 || dim == 1024; }
// Queries of the next corpus pass.  One wave can hold 64 queries over the whole K (32 at d = 1024); a pair
// holds 96 (three query tiles: with four, the 768-d build spills and loses more than the saved pass).  The
// pair kernel is used when it shortens the plan: always at d = 1024, and at 384 / 768 when passes of 96
// cover what is left in fewer passes than passes of 64.
static uint32_t cb_group(uint32_t dim, uint32_t left) {
    const uint32_t solo = dim == 1024 ? 32u : 64u;
    if (left <= solo) return solo;
    if (dim == 1024) return left > 96u ? 128u : 96u; // 128: cosine_bf16_qsplit (32 queries per wave)
    return (left + 95u) / 96u < (left + 63u) / 64u ? 96u : 64u;
}

// How 256 queries at d = 1024 take their two passes of 128 (cosine_bf16_qsplit): as ONE launch of sibling workgroups sharing
// every tile through their XCD's L2 (see the kernel), or -- OI_BF16_SIB=0, A/B -- as two launches one after the other.
static bool cb_siblings_on() {
    const char *e = oi_ablation_env("OI_BF16_SIB");
    return (e ? atoi(e) : OI_BF16_SIB_DEFAULT) != 0;
}
// Pool geometry of one chunk.  Segments are per workgroup; a workgroup's waves take 4 tiles per round
// (solo kernel) or 2 (pair kernel) -- the cap below covers both.
void oi_cosine_bf16_geometry(const oi_ctx *ctx, uint64_t n_rows, uint32_t *n_segs, uint32_t *seg_cap, bool siblings) {
    const uint64_t n_tiles = (n_rows + OI_TILE_ROWS - 1) / OI_TILE_ROWS;
    const uint64_t quads = (n_tiles + 3) / 4;
    const uint64_t cus = siblings ? std::max<uint64_t>(8, ((uint64_t)ctx->num_cus / 16) * 8) : (uint64_t)ctx->num_cus; // pairs of workgroups: half the grid, whole XCD rounds
    uint64_t grid = quads < cus ? (quads ? quads : 1) : cus;
    if (siblings && grid >= 8) grid -= grid % 8; // (the same-XCD pairing addresses workgroups in groups of 16 = 8 pairs)
    *n_segs = (uint32_t)grid;
    *seg_cap = (uint32_t)((quads + grid - 1) / grid) * 4 * OI_TILE_ROWS;
}

// One launch of a kernel of this file: `grid` workgroups of 256 threads with `lds` bytes of dynamic LDS (the kernel's own
// constexpr above).  tail: what the kernel takes after the arguments all three begin with -- the pool's fill counters, the
// thresholds and geometry, the solo kernel's filter, in the kernel's own order (CB_CNT, CB_POOL below).
template <class Kernel, class... Tail>
static int cb_launch(oi_ctx *ctx, Kernel kernel, uint32_t grid, size_t lds, const uint16_t *rows, uint64_t row_begin,
                     uint64_t row_end, const uint16_t *q, uint32_t nq, uint32_t doc_id_base, const PoolView &p, Tail... tail) {
    OI_CHECK(oi_dyn_lds(ctx, reinterpret_cast<const void *>(kernel), lds));
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, ctx->stream, rows, row_begin, row_end, q, nq, doc_id_base, p.keys,
                       tail...);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// All queries of a batch over rows [row_begin, row_end) of a bf16 corpus.  d_queries: f32 [n_queries][dim].
int oi_launch_cosine_bf16_chunk(oi_ctx *ctx, const uint16_t *rows, uint64_t row_begin, uint64_t row_end, uint32_t dim,
                                const float *d_queries, uint32_t n_queries, uint32_t doc_id_base, PoolView &pool) {
    OI_REQUIRE(oi_cosine_bf16_supported(dim), "cosine (bf16 corpus): dim %u not instantiated (384, 768, 1024)", dim);
    // siblings: every group of this batch is a full pair of 128-query passes (256, 512, ... queries at d = 1024) and the chunk
    // is long enough to give every pair of workgroups a tile
    // A filtered search is pinned to the one-pass-per-group kernel (cosine_bf16_filter), the only one with the
    // doc filter: groups of 32 queries at d = 1024, 64 otherwise, never the pair / query-split kernels or siblings
    const bool filtered = pool.filt != nullptr;
    const bool siblings = !filtered && cb_siblings_on() && dim == 1024 && n_queries >= 256 && n_queries % 256 == 0 &&
                          row_end > row_begin && (row_end - row_begin) >= (uint64_t)OI_TILE_ROWS * ctx->num_cus;
    oi_cosine_bf16_geometry(ctx, row_end > row_begin ? row_end - row_begin : 0, &pool.n_segs, &pool.seg_cap, siblings);
    OI_REQUIRE(pool.n_segs <= pool.seg_cnt_stride && pool.carry_cap + (uint64_t)pool.n_segs * pool.seg_cap <= pool.stride,
               "cosine (bf16 corpus): chunk does not fit the candidate pool");
    if (row_end <= row_begin || n_queries == 0) return OI_OK;
    static const bool solo_only = oi_ablation_env("OI_BF16_SOLO") != nullptr; // A/B: never use the pair kernel
    static const bool no_quad = oi_ablation_env("OI_BF16_NO_QUAD") != nullptr;   // A/B: passes of at most 96 queries at d = 1024
    const uint32_t n_padded = (n_queries + 31u) & ~31u;
    DevBuf &qb = ctx->buf("q_bf16");
    OI_CHECK(qb.ensure(sizeof(uint16_t) * (size_t)(n_padded + 128) * dim));
    {
        const uint64_t total = (uint64_t)n_padded * dim;
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 1024);
        hipLaunchKernelGGL(cb_stage_queries, dim3(blocks), dim3(256), 0, ctx->stream, d_queries, n_queries, n_padded, dim,
                           qb.as<uint16_t>());
        OI_HIP_CHECK(hipGetLastError());
    }
    ProfScope ps(ctx, "cosine");
    for (uint32_t q0 = 0; q0 < n_queries;) {
        const uint32_t left = n_queries - q0;
        uint32_t group = solo_only || filtered ? (dim == 1024 ? 32u : 64u) : cb_group(dim, left);
        if (no_quad && group > 96u) group = 96u;
        if (siblings) group = 256u;
        const uint32_t nq_here = std::min(group, left);
        const uint32_t nqt = (nq_here + 31u) / 32u; // query tiles of 32 in this launch
        const PoolView p = pool.for_queries(q0);
        const uint16_t *qptr = qb.as<uint16_t>() + (uint64_t)q0 * dim;
#define CB_RUN(KERNEL, GRID, LDS, ...) \
    OI_CHECK(cb_launch(ctx, KERNEL, GRID, LDS, rows, row_begin, row_end, qptr, nq_here, doc_id_base, p, __VA_ARGS__))
#define CB_CNT p.seg_cnt, p.seg_cnt_stride
#define CB_POOL p.tau_keys, p.stride, p.carry_cap, p.seg_cap, p.overflow
#define CB_SOLO(DD, T)                                                                                                      \
    CB_RUN((p.filt ? cosine_bf16_filter<DD, T, true> : cosine_bf16_filter<DD, T, false>), p.n_segs, cb_solo_lds(DD), CB_CNT, \
           CB_POOL, p.filt, p.attrs)
#define CB_PAIR(DD, T) CB_RUN((cosine_bf16_pair<DD, T>), p.n_segs, cb_pair_lds(DD, T), CB_POOL, CB_CNT) // (its counters come last)
#define CB_QSPLIT(SIB, GRID) CB_RUN(cosine_bf16_qsplit<SIB>, GRID, CQ_LDS, CB_CNT, CB_POOL)
        const bool pair = nq_here > (dim == 1024 ? 32u : 64u);
        if (dim == 1024) {
            if (nq_here > 128u) CB_QSPLIT(2, 2u * p.n_segs); // (siblings)
            else if (nq_here > 96u) CB_QSPLIT(0, p.n_segs);
            else if (!pair) CB_SOLO(1024, 1);
            else if (nqt == 2) CB_PAIR(1024, 2);
            else CB_PAIR(1024, 3);
        } else if (dim == 768) {
            if (pair) CB_PAIR(768, 3);
            else if (nqt == 1) CB_SOLO(768, 1);
            else CB_SOLO(768, 2);
        } else {
            if (pair) CB_PAIR(384, 3);
            else if (nqt == 1) CB_SOLO(384, 1);
            else CB_SOLO(384, 2);
        }
#undef CB_SOLO
#undef CB_PAIR
#undef CB_QSPLIT
#undef CB_POOL
#undef CB_CNT
#undef CB_RUN
        q0 += nq_here;
    }
    return OI_OK;
}
