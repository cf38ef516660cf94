// oi_screen_tile.h -- the per-wave tile pipeline of the three bf16 screen kernels, each construct written once:
//   cosine_copy_screen (cosine_screen_copy.hip), vo_stream_kernel (oi_volume.h), cosine_screen_filter (cosine_prefilter.hip).
// All three run one persistent workgroup of 4 waves per segment; a wave holds the whole query block as bf16 B operands in
// registers, owns every (4 x grid)-th 32-row tile and streams its tiles through its own LDS ring of 4-KiB slots (32 rows x 128 B)
// with the LDS-DMA loads of oi_lds_dma.h (read THE CONTRACT there first: everything below is written around it).  Here:
//   * the query block preload, the wave's tile ownership with its buffer descriptors, the retiring wait for the loads
//     hipcc knows about, the score test and the ragged-tile mask (the swizzled DMA source offsets: oi_lds_dma.h) (all three kernels);
//   * OiCopyRing: the ring over bf16 rows with a run-time ring offset                    (copy screen and vo_stream_kernel;
//     cosine_screen_filter keeps its own k-loop: a compile-time ring index, two ds_read_b128 and four conversions per k-step);
//     also the ring of the bf16 corpus scorer's solo and pair kernels (cosine_bf16.hip), the pair over a K-slice of half a
//     row; that file takes its tile ownership (oi_owner_tiles), query preload and close (oi_pool_close) from here too;
//   * the threshold decode and OiPoolSink, the survivor epilogue into the candidate pool (copy screen and f32 screen;
//     vo_stream_kernel's band staging has another payload and another claim).
// Everything is force-inlined and by value: the compiler sees three kernel families, not one.
#pragma once

#include "oi_device.h"
#include "oi_lds_dma.h"

typedef float oi_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 oi_bf16x8 __attribute__((ext_vector_type(8)));

#define OI_TILE_ROWS 32
#define OI_SLOT_K 64                 // bf16 of K per ring slot row (128 B)
#define OI_SLOT_BYTES (OI_TILE_ROWS * 128)

// Dynamic LDS of a kernel: 4 waves' rings of nbuf slots, and what the pool sink keeps behind them (seg_fill[64], the staging ring).
constexpr size_t oi_ring_lds(int nbuf) { return (size_t)4 * nbuf * OI_SLOT_BYTES; }
#define OI_POOL_SINK_LDS (64 * 4 + OI_STAGE_LDS)

// Register r of query tile t holds D[row (r&3) + 8 (r>>2) + 4 lh][query 32 t + li]: that row of the tile whose first row is row0.
__device__ __forceinline__ uint32_t oi_tile_row(uint32_t row0, int r, uint32_t lh) { return row0 + (uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * lh; }

// Every query over the wave's K-slice, in registers for the whole launch: B[k = k0 + 16 s + 8 lh + 0..7][n = li].
// queries: bf16 [32 * NQT][D], zero padded (pf_stage_queries_kernel, cb_stage_queries).  KW, k0: the slice's width and where
// it starts (the whole K but for a cosine_bf16_pair wave, which holds one half).
template <int D, int NQT, int KW = D>
__device__ __forceinline__ void oi_tile_load_queries(oi_bf16x8 (&qreg)[NQT][KW / 16], const uint16_t *__restrict__ queries, uint32_t li,
                                                     uint32_t lh, uint32_t k0 = 0) {
    static_assert(NQT * (KW / 16) * 4 <= 400, "the query block must fit the register file");
#pragma unroll
    for (int t = 0; t < NQT; ++t)
#pragma unroll
        for (int s = 0; s < KW / 16; ++s)
            qreg[t][s] = *reinterpret_cast<const oi_bf16x8 *>(queries + (uint64_t)(32 * t + li) * D + k0 + 16 * s + 8 * lh);
}

// Every load hipcc knows about (queries, thresholds, margins) is retired HERE, before the ring starts, with a wait it models:
// otherwise it re-waits for them inside the tile loop and drains the DMA ring.
__device__ __forceinline__ void oi_tile_retire_visible_loads() {
    __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0) only
}

// The tiles of one OWNER (a wave, a pair of waves or a workgroup) among rows [row_begin, row_end): first, + stride, ...
struct OiWaveTiles {
    uint64_t row_begin, row_end, first, stride, my_nt;
    __device__ __forceinline__ uint64_t row0(uint64_t ti) const { return row_begin + (first + ti * stride) * (uint64_t)OI_TILE_ROWS; }
    // rows: row 0 of the corpus.  Past this wave's last tile: an EMPTY descriptor (loads return zeros)
    template <uint32_t ROW_BYTES>
    __device__ __forceinline__ oi_u32x4 srd(const void *rows, uint64_t ti) const {
        const uint64_t r0 = row0(ti < my_nt ? ti : 0);
        return oi_make_srd(reinterpret_cast<const unsigned char *>(rows) + r0 * ROW_BYTES, ti < my_nt ? (row_end - r0) * (uint64_t)ROW_BYTES : 0ull);
    }
};
// Owner `owner` of `n_owners` takes every n_owners-th 32-row tile.
__device__ __forceinline__ OiWaveTiles oi_owner_tiles(uint64_t row_begin, uint64_t row_end, uint64_t owner, uint64_t n_owners) {
    OiWaveTiles t;
    t.row_begin = row_begin;
    t.row_end = row_end;
    const uint64_t n_tiles = (row_end - row_begin + OI_TILE_ROWS - 1) / OI_TILE_ROWS;
    t.first = owner;
    t.stride = n_owners;
    t.my_nt = t.first < n_tiles ? (n_tiles - t.first + t.stride - 1) / t.stride : 0;
    return t;
}
// The tiles of this WAVE, every wave of the grid an owner: oi_owner_tiles(.., blockIdx.x * 4 + w, 4 * gridDim.x).  Written out:
// as that call the operands are evaluated ahead of n_tiles, and the register allocation of every screen kernel moves.
__device__ __forceinline__ OiWaveTiles oi_wave_tiles(uint64_t row_begin, uint64_t row_end, uint32_t w) {
    OiWaveTiles t;
    t.row_begin = row_begin;
    t.row_end = row_end;
    const uint64_t n_tiles = (row_end - row_begin + OI_TILE_ROWS - 1) / OI_TILE_ROWS;
    t.first = (uint64_t)blockIdx.x * 4 + w;
    t.stride = (uint64_t)gridDim.x * 4;
    t.my_nt = t.first < n_tiles ? (n_tiles - t.first + t.stride - 1) / t.stride : 0;
    return t;
}

// Which of the lane's 16 NQT scores reach their query's threshold: bit 16 t + r.  One v_cmp per score; a NaN on either side fails.
template <int NQT>
__device__ __forceinline__ uint32_t oi_tile_pass_mask(const oi_f32x16 (&acc)[NQT], const float (&thr)[NQT]) {
    uint32_t m = 0;
#pragma unroll
    for (int t = 0; t < NQT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) m |= acc[t][r] >= thr[t] ? 1u << (16 * t + r) : 0u;
    return m;
}
// The ragged last tile (rows_left = row_end - row0 < 32): rows past the end read as zeros and are not documents.
__device__ __forceinline__ uint32_t oi_tile_mask_ragged(uint32_t m, uint64_t rows_left, uint32_t lh) {
    if (rows_left < (uint64_t)OI_TILE_ROWS) {
        const uint32_t left = (uint32_t)rows_left;
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (oi_tile_row(0u, r, lh) >= left) m &= ~(0x00010001u << r);
    }
    return m;
}

// ------------------------------------------------------------------ the bf16 copy ring
// A wave's ring of NBUF slots over a K-slice of KW bf16 (the whole row by default) of bf16 rows of D: a tile is NKC = KW / 64
// slots, P = NBUF - 1 slots are in flight ahead of the one being consumed.  Per 16 k of a tile: one conflict-free ds_read_b128, NQT MFMAs, one DMA piece of the slot P ahead.
//   * the ring index is a RUN-TIME scalar (one s_add + s_cselect per slot, one v_add per fragment read), so NBUF is free of
//     the tile's slot count;
//   * the refill of slot s + P always issues (an empty descriptor past the wave's last tile returns zeros), so every counted
//     wait is the same constant, vmcnt(4 (P - 1)), and the tile loop has no tail cases.
// ISSUE: the piece-issue call (oi_dma_piece, or a variant build's stand-in for it).
typedef void (*oi_piece_fn)(const oi_u32x4 &, uint32_t, uint32_t, uint32_t);
__device__ __forceinline__ void oi_dma_piece_stream(const oi_u32x4 &srd, uint32_t voff, uint32_t soff, uint32_t lds_dst) {
    oi_dma_piece(srd, voff, soff, lds_dst);
}

template <int D, int NBUF, oi_piece_fn ISSUE = oi_dma_piece_stream, int KW = D>
struct OiCopyRing {
    static constexpr int NKC = KW / OI_SLOT_K;    // ring slots per tile
    static constexpr int P = NBUF - 1;            // slots in flight ahead of the one being consumed
    static constexpr uint32_t BYTES = NBUF * OI_SLOT_BYTES;
    static constexpr uint32_t ROW_BYTES = D * 2;
    static_assert(KW % OI_SLOT_K == 0 && P >= 1 && P <= 2 * NKC, "unsupported ring depth for this K width");

    uint32_t voff[4], frag_off[4];
    uint32_t ring_w;              // LDS address of the wave's ring (the DMA's side)
    const unsigned char *ring_rd; // the same, for the fragment reads
    uint32_t rd_off, wr_off;      // ring offsets (bytes, wave-uniform): the slot being consumed, and the one vacated before it = the refill target
    oi_u32x4 s0, s1, s2;          // descriptors of the tile being consumed and the two after it (P <= 2 NKC: a refill reaches no further)

    // lds: the wave's BYTES of ring.  k_base (wave-uniform bytes): where the K-slice starts in a row.  Retires the
    // compiler-visible loads and issues the prologue: logical slots 0..P-1 (tile j / NKC, slot j % NKC) into ring slots 0..P-1.
    __device__ __forceinline__ void begin(const OiWaveTiles &wt, const void *rows, unsigned char *lds, uint32_t lane, uint32_t k_base = 0) {
        const uint32_t li = lane & 31, lh = lane >> 5;
        oi_tile_voff<ROW_BYTES>(voff, lane, k_base);
        ring_w = oi_lds_addr(lds);
        ring_rd = lds;
        // fragment of MFMA group g of a slot: row li, bf16 16 g + 8 lh + 0..7 = logical 16-B column 2g + lh (oi_tile_frag_off, written
        // out: as the call the swizzle's operands come out in another order in every kernel on this ring)
#pragma unroll
        for (int g = 0; g < 4; ++g) frag_off[g] = li * 128 + (((2 * g + lh) ^ ((li >> 1) & 7)) << 4);
        s0 = wt.srd<ROW_BYTES>(rows, 0), s1 = wt.srd<ROW_BYTES>(rows, 1), s2 = wt.srd<ROW_BYTES>(rows, 2);
        oi_tile_retire_visible_loads();
        oi_static_for<0, P>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
            constexpr int tj = j / NKC, kj = j % NKC;
#pragma unroll
            for (int m = 0; m < 4; ++m)
                ISSUE(tj == 0 ? s0 : (tj == 1 ? s1 : s2), voff[m], kj * 128, ring_w + j * OI_SLOT_BYTES + m * 1024);
        });
        rd_off = 0, wr_off = (NBUF - 1) * OI_SLOT_BYTES;
    }

    // One tile: acc = its 32 rows x the query block.  Slot kc of the tile sits at rd_off.  Per MFMA group (kc, g): read the next
    // fragment, NQT MFMAs on the current one, DMA piece g of logical slot kc + P into the slot vacated last (wr_off); after
    // g == 3 the counted wait retires slot kc + 1 (P - 1 younger slots stay in flight) and the offsets move on.
    // MFMA = false (variant builds): the stream without the matrix instructions; every score 0, results WRONG.
    template <int NQT, bool MFMA = true>
    __device__ __forceinline__ void tile(oi_f32x16 (&acc)[NQT], const oi_bf16x8 (&qreg)[NQT][KW / 16]) {
#pragma unroll
        for (int t = 0; t < NQT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
        oi_wait_vm<4 * (P - 1)>();
        oi_bf16x8 a_cur = *reinterpret_cast<const oi_bf16x8 *>(ring_rd + rd_off + frag_off[0]);
        oi_static_for<0, NKC * 4>([&](auto gi_) {
            constexpr int gi = decltype(gi_)::value;
            constexpr int kc = gi / 4, g = gi % 4;
            constexpr int sn = kc + P;           // logical slot (relative to this tile) refilled during this slot
            constexpr int tn = sn / NKC, kn = sn % NKC;
            oi_bf16x8 a_nxt = a_cur;
            if constexpr (g < 3) a_nxt = *reinterpret_cast<const oi_bf16x8 *>(ring_rd + rd_off + frag_off[g + 1]);
            if constexpr (MFMA) {
#pragma unroll
                for (int t = 0; t < NQT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_cur, qreg[t][gi], acc[t], 0, 0, 0);
            } else {
                asm volatile("" : : "v"(a_cur));
            }
            ISSUE(tn == 0 ? s0 : (tn == 1 ? s1 : s2), voff[g], kn * 128, ring_w + wr_off + g * 1024);
            if constexpr (g == 3) {
                wr_off = rd_off;
                rd_off = rd_off + OI_SLOT_BYTES == BYTES ? 0u : rd_off + OI_SLOT_BYTES;
                if constexpr (kc + 1 < NKC) {
                    oi_wait_vm<4 * (P - 1)>();
                    a_nxt = *reinterpret_cast<const oi_bf16x8 *>(ring_rd + rd_off + frag_off[0]);
                }
            }
            a_cur = a_nxt;
        });
    }

    // Tile ti is done: the descriptors move on by one tile.
    __device__ __forceinline__ void next(const OiWaveTiles &wt, const void *rows, uint64_t ti) {
        s0 = s1;
        s1 = s2;
        s2 = wt.srd<ROW_BYTES>(rows, ti + 3);
    }
    // The zero-filling refills issued past the last tile have landed before the LDS goes back.
    __device__ __forceinline__ void end() { oi_wait_vm<0>(); }
};

// ------------------------------------------------------------------ the pool epilogue
// Screen thresholds (tau~ - 2 eps) of the queries this lane filters, as FLOATS: for a score s that is not a NaN,
// oi_f32_key(s) >= key  <=>  s >= oi_key_f32(key) (the key is strictly monotone on floats after s + 0 has made -0 a +0, and
// the comparison does not tell -0 from +0 either); keys at or below key(-inf) pass every such score (-inf), keys above
// key(+inf) -- 0xFFFFFFFF: no query in this slot -- map to NaN bit patterns, which no score is >=.  A NaN score fails the
// comparison by itself.  One v_cmp per score instead of the key's five instructions.
template <int NQT>
__device__ __forceinline__ void oi_tile_thresholds(float (&tauf)[NQT], const uint32_t *tau_keys, uint32_t n_queries, uint32_t li) {
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const uint32_t q = 32u * t + li;
        const uint32_t k = q < n_queries ? tau_keys[q] : 0xFFFFFFFFu;
        tauf[t] = k <= 0x007FFFFFu ? -__builtin_inff() : oi_key_f32(k);
    }
}

// The end of a workgroup's launch: every wave's appends are counted (a barrier), then the fill of segment `seg` per query, for the
// 32 * NQT queries of the launch.  (OiPoolSink::close, and the three kernels of cosine_bf16.hip, which append by other routes.)
template <int NQT>
__device__ __forceinline__ void oi_pool_close(const uint32_t *seg_fill, uint32_t seg_cap, uint32_t n_queries, uint32_t *seg_cnt,
                                              uint32_t seg_cnt_stride, uint32_t seg) {
    __syncthreads();
    const uint32_t tid = threadIdx.x;
    if (tid < (n_queries < 32u * NQT ? n_queries : 32u * NQT)) { // (one compare of its own: the opening one is not kept alive over the tile loop)
        const uint32_t c = seg_fill[tid];
        seg_cnt[(uint64_t)tid * seg_cnt_stride + seg] = c < seg_cap ? c : seg_cap;
    }
}

// A workgroup's way into its segment of the candidate pool.  LDS (OI_POOL_SINK_LDS bytes at lds): seg_fill[64], the keys a
// query has in the segment, then the staging ring of oi_lds_dma.h.  The members named like OI_STAGE_FLUSH_TO_POOL's operands
// ARE its operands.  (Force-inlined members of a by-value struct: st_head / st_n stay in SGPRs and nothing goes to scratch --
// unlike the by-reference lambda the macro's note speaks of; tests/test_screen_ring_schedule.py holds that.)
struct OiPoolSink {
    uint32_t *seg_fill;
    uint64_t *stage_keys; // this wave's
    uint32_t *stage_q;
    uint32_t st_head, st_n; // wave-uniform: first staged entry (mod OI_STAGE), staged entries (< OI_STAGE_FLUSH between tiles)
    uint64_t *my_seg;
    uint64_t pool_stride;
    uint32_t seg_cap, doc_id_base, lane;
    uint32_t *overflow;

    // Ends with the only barrier before close(): seg_fill is zero before any wave appends.
    template <int NQT>
    __device__ __forceinline__ void open(unsigned char *lds, uint32_t w, uint64_t *pools, uint32_t carry_cap, uint32_t seg_cap_,
                                         uint64_t pool_stride_, uint32_t doc_id_base_, uint32_t *overflow_) {
        seg_fill = reinterpret_cast<uint32_t *>(lds);
        stage_keys = reinterpret_cast<uint64_t *>(lds + 256) + w * OI_STAGE;
        stage_q = reinterpret_cast<uint32_t *>(lds + 256 + 4 * OI_STAGE * 8) + w * OI_STAGE;
        st_head = 0, st_n = 0;
        my_seg = pools + carry_cap + (uint64_t)blockIdx.x * seg_cap_;
        pool_stride = pool_stride_, seg_cap = seg_cap_, doc_id_base = doc_id_base_, overflow = overflow_;
        lane = threadIdx.x & 63;
        if (threadIdx.x < 32 * NQT) seg_fill[threadIdx.x] = 0;
        __syncthreads();
    }

    // The survivors of one tile (m: oi_tile_pass_mask after oi_tile_mask_ragged), straight out of the accumulators.  Which
    // scores pass was collected in a mask first: a tile without a survivor -- most tiles of the large chunks -- leaves through
    // one ballot.  FILT: the doc filter (oi_filter_tile) after the threshold.
    template <int NQT, bool FILT>
    __device__ __forceinline__ void append(uint32_t m, const oi_f32x16 (&acc)[NQT], uint64_t row0, const uint4 *__restrict__ filt,
                                           const uint2 *__restrict__ attrs) {
        const uint32_t li = lane & 31, lh = lane >> 5;
        if (__builtin_amdgcn_ballot_w64(m != 0u) == 0ull) return;
        if constexpr (FILT) m = oi_filter_tile<NQT>(m, filt, attrs, row0, lh, li);
        const uint32_t cnt = (uint32_t)__builtin_popcount(m);
        const uint32_t incl = oi_wave_incl_scan(cnt);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        if (total <= OI_STAGE - OI_STAGE_FLUSH) {
            // SPARSE tile (every tile once a threshold stands): the survivors go to the wave's LDS staging ring, and 64 of
            // them leave with ONE store instruction.  A store per survivor sat in the same in-order vmcnt queue as the DMA
            // pieces: every counted wait then also waited for slots it did not need yet (the stores behind them), 0.13 ms of
            // the 4.9 ms step at 10M rows (tools/r04_epilogue_probe.sh).
            uint32_t idx = st_head + st_n + incl - cnt;
#pragma unroll
            for (int t = 0; t < NQT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (m & (1u << (16 * t + r))) {
                        const uint32_t row = oi_tile_row((uint32_t)row0, r, lh);
                        stage_keys[idx & (OI_STAGE - 1)] = oi_rank_key(acc[t][r], doc_id_base + row);
                        stage_q[idx & (OI_STAGE - 1)] = 32u * t + li;
                        ++idx;
                    }
            st_n += total;
            while (st_n >= OI_STAGE_FLUSH) {
                OI_STAGE_FLUSH_TO_POOL(OI_STAGE_FLUSH);
            }
        } else {
            // DENSE tile (the first chunk, scored without a threshold: every score passes): straight to the pool, ONE LDS
            // atomic per query for all of a lane's survivors
            uint32_t pos[NQT];
#pragma unroll
            for (int t = 0; t < NQT; ++t) // (both atomics are in flight before the first is waited for; adding 0 is harmless)
                pos[t] = atomicAdd(&seg_fill[32u * t + li], (uint32_t)__builtin_popcount((m >> (16 * t)) & 0xFFFFu));
#pragma unroll
            for (int t = 0; t < NQT; ++t) {
                uint64_t *dst = my_seg + (uint64_t)(32u * t + li) * pool_stride;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (m & (1u << (16 * t + r))) {
                        const uint32_t row = oi_tile_row((uint32_t)row0, r, lh);
                        if (pos[t] < seg_cap) dst[pos[t]] = oi_rank_key(acc[t][r], doc_id_base + row);
                        else *overflow = 1u;
                        ++pos[t];
                    }
                }
            }
        }
    }
    // After the wave's last tile: what is still staged leaves.
    __device__ __forceinline__ void flush_rest() {
        if (st_n) {
            OI_STAGE_FLUSH_TO_POOL(st_n);
        }
    }
    // Every wave's appends are counted (a barrier), then the segment's fill per query.
    template <int NQT>
    __device__ __forceinline__ void close(uint32_t n_queries, uint32_t *seg_cnt, uint32_t seg_cnt_stride) const {
        oi_pool_close<NQT>(seg_fill, seg_cap, n_queries, seg_cnt, seg_cnt_stride, blockIdx.x);
    }
};
