// oi_ksplit_tile.h -- what a K-split f32 kernel is, each construct written once:
//   cosine_ksplit16_filter (cosine_ksplit.hip, f32 MFMAs), cosine_split_filter (cosine_split.hip, six bf16 MFMAs per product).
// Both run one persistent workgroup of 4 waves per segment; the workgroup owns every gridDim.x-th 32-row tile, wave w owns
// k in [w D/4, (w+1) D/4) of it, holds that K-slice of the whole query block in registers and streams its slice of the rows
// through its own LDS ring of 4-KiB slots (32 rows x 32 floats) with the LDS-DMA loads of oi_lds_dma.h (read THE CONTRACT
// there first).  Here:
//   * the workgroup's tile ownership with its buffer descriptors (an EMPTY one past the last tile: a branch-free tile body);
//   * the K-slice ring: its shape from D, the DMA source offsets, the retiring wait for the loads hipcc knows about, the
//     prologue, the piece issue that picks this tile's descriptor or the next one's, the descriptor rotation;
//   * the deferred epilogue: a tile's partial sums go to LDS right after its last MFMA, and the cross-wave sum + filter of
//     tile t rides INSIDE tile t+1's MFMA stream (barrier A, the outputs, barrier B, at the k-steps the kernel picks), so its
//     LDS round trips and VALU work issue in the shadow of the matrix instructions and the ring keeps being refilled.  The
//     four partial tiles are summed in a fixed order, (w0 + w1) + (w2 + w3); survivors go straight into THIS workgroup's
//     private segment of each query's candidate pool (fill counters in LDS): no global atomic, no returning memory operation,
//     hence nothing that would make a wave drain its DMA ring;
//   * on the host: the dynamic LDS, the launch and the pool geometry.
// The kernels keep their query preload, their k-step body with the positions at which it issues pieces and hosts outputs, and
// the map from an epilogue element to (query, row) that follows their MFMA's D layout.  They do NOT share a tile loop: one puts
// its pieces behind MFMA sets, the other behind a scheduled MFMA group.  Everything is force-inlined and by value.
#pragma once

#include "oi_device.h"
#include "oi_internal.h"
#include "oi_lds_dma.h"

#define OI_KS_TILE_ROWS 32
#define OI_KS_SLOT_BYTES 4096 // 32 rows x 128 B (32 floats of K)

__device__ __forceinline__ void oi_ks_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Thresholds of the queries this lane filters: query tile t is W wide, the lane's query in it is li.
template <int W, int NT>
__device__ __forceinline__ void oi_ks_thresholds(uint32_t (&tau)[NT], const uint32_t *tau_keys, uint32_t n_queries, uint32_t li) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const uint32_t q = (uint32_t)W * t + li;
        tau[t] = q < n_queries ? tau_keys[q] : 0xFFFFFFFFu;
    }
}

// Element sum S (OiKsplitTile::sum) of query Q and corpus row ROW is tested against the query's threshold key TAU and against
// PASSES -- the kernel's doc filter, evaluated only behind the threshold, or `true` -- and appended to the workgroup's segment.
// TILE: the kernel's OiKsplitTile.  (A macro: as a force-inlined function the same statements compile to one packed add less
// and three register moves more per output, inside the MFMA stream; cosine_ksplit16_filter<768, 2, false> ran 0.6 % slower --
// DESIGN 4.1b.)
#define OI_KS_OUT(TILE, S, Q, ROW, TAU, PASSES)                                                                     \
    do {                                                                                                            \
        const float s_ = (S);                                                                                       \
        const uint32_t q_ = (Q);                                                                                    \
        const uint64_t row_ = (ROW);                                                                                \
        if ((TILE).have_prev && row_ < (TILE).row_end && s_ == s_ && oi_f32_key(s_) >= (TAU) && (PASSES)) {         \
            const uint32_t pos_ = atomicAdd(&(TILE).seg_fill[q_], 1u); /* LDS */                                    \
            if (pos_ < (TILE).seg_cap)                                                                              \
                (TILE).my_seg[(uint64_t)q_ * (TILE).pool_stride + pos_] = oi_rank_key(s_, (TILE).doc_id_base + (uint32_t)row_); \
            else *(TILE).overflow = 1u;                                                                             \
        }                                                                                                           \
    } while (0)

template <int D, int NQT> // NQT: query tiles of 32
struct OiKsplitTile {
    static constexpr int KS = D / 4;                       // K-slice of one wave (floats)
    static constexpr int NKC = KS / 32;                    // ring slots per tile and wave
    static constexpr int NBUF = NKC <= 6 ? NKC : NKC / 2;  // ring depth: a compile-time ring index, so it divides NKC
    static constexpr int P = NBUF - 1;                     // slots in flight ahead of the one being consumed
    static constexpr int NG = NKC * 2;                     // k-steps of 16 per tile
    static constexpr int RED = NQT * 16 * 64;              // floats of one wave's partial tile
    static constexpr int N_OUT = NQT * 4;                  // epilogue elements per thread and tile
    // dynamic LDS: rings [4][NBUF][4 KiB], partial tiles [4][RED], seg_fill[64]
    static constexpr size_t LDS = 4 * NBUF * OI_KS_SLOT_BYTES + 4 * RED * 4 + 64 * 4;
    static_assert(KS % 32 == 0 && NKC % NBUF == 0 && P >= 1 && P < NKC, "unsupported D");

    const float *rows;
    uint64_t row_begin, row_end, my_nt;
    uint32_t voff[4];
    uint32_t ring_w;              // LDS address of the wave's ring (the DMA's side)
    const unsigned char *ring_rd; // the same, for the fragment reads
    oi_u32x4 cur, nxt;            // descriptors of the tile being consumed and the one after it
    float *red, *my_red;          // the four partial tiles, this wave's
    uint32_t *seg_fill;
    uint64_t *my_seg;
    uint64_t prev_row0, pool_stride; // prev_row0: first corpus row of the tile whose partials sit in `red`
    bool have_prev;                  // false during the first tile: `red` holds nothing yet (begin)
    uint32_t seg_cap, doc_id_base;
    uint32_t *overflow;

    // Zeroes seg_fill (barrier A of the first tile orders it before any append).  false: no tile for this workgroup.
    __device__ __forceinline__ bool open(unsigned char *smem, uint32_t w, const float *rows_, uint64_t row_begin_,
                                         uint64_t row_end_, uint64_t *pools, uint32_t carry_cap, uint32_t seg_cap_,
                                         uint64_t pool_stride_, uint32_t doc_id_base_, uint32_t *overflow_) {
        red = reinterpret_cast<float *>(smem + 4 * NBUF * OI_KS_SLOT_BYTES);
        seg_fill = reinterpret_cast<uint32_t *>(red + 4 * RED);
        my_red = red + w * RED;
        ring_rd = smem + w * (NBUF * OI_KS_SLOT_BYTES);
        ring_w = oi_lds_addr(smem) + w * (NBUF * OI_KS_SLOT_BYTES);
        rows = rows_, row_begin = row_begin_, row_end = row_end_;
        pool_stride = pool_stride_, seg_cap = seg_cap_, doc_id_base = doc_id_base_, overflow = overflow_;
        prev_row0 = 0, have_prev = false;
        if (threadIdx.x < 64) seg_fill[threadIdx.x] = 0;
        const uint64_t n_tiles = (row_end - row_begin + OI_KS_TILE_ROWS - 1) / OI_KS_TILE_ROWS;
        my_nt = blockIdx.x < n_tiles ? (n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
        my_seg = pools + carry_cap + (uint64_t)blockIdx.x * seg_cap;
        return my_nt != 0;
    }
    __device__ __forceinline__ uint64_t row0(uint64_t ti) const {
        return row_begin + (blockIdx.x + ti * gridDim.x) * (uint64_t)OI_KS_TILE_ROWS;
    }
    __device__ __forceinline__ oi_u32x4 srd(uint64_t ti) const {
        const uint64_t r0 = row0(ti < my_nt ? ti : 0);
        return oi_make_srd(rows + r0 * D, ti < my_nt ? (row_end - r0) * (uint64_t)(D * 4) : 0ull);
    }

    // Retires the compiler-visible loads and issues the prologue: slots 0..P-1 of the first tile.  skip: a timing build's "no DMA".
    __device__ __forceinline__ void start_ring(uint32_t lane, uint32_t w, bool skip = false) {
        oi_tile_voff<D * 4>(voff, lane, w * (uint32_t)(KS * 4));
        cur = srd(0), nxt = srd(1);
        __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0) only
#pragma unroll
        for (int kc = 0; kc < P; ++kc)
#pragma unroll
            for (int m = 0; m < 4; ++m) refill(kc, m, skip);
    }
    // Piece m of slot sn (counted from this tile's slot 0, so slot sn - NKC of the next tile from NKC on) into the ring slot
    // that slot sn - NBUF has vacated.  Both are constants where the unrolled k-steps call it.
    __device__ __forceinline__ void refill(int sn, int m, bool skip = false) {
        oi_dma_piece(sn < NKC ? cur : nxt, voff[m], (sn % NKC) * 128, ring_w + (sn % NBUF) * OI_KS_SLOT_BYTES + m * 1024, skip);
    }
    // Tile ti starts: `red` holds tile ti - 1.  (cosine_split_filter with one query tile keeps a statement of its own.)
    __device__ __forceinline__ void begin(uint64_t ti) { have_prev = ti > 0; }
    // Tile ti's MFMAs are done and its partial sums stored to my_red: the descriptors move on by one tile.
    __device__ __forceinline__ void next(uint64_t ti) {
        prev_row0 = row0(ti);
        cur = nxt;
        nxt = srd(ti + 2);
    }

    // Element e of the previous tile, summed over the four waves.
    __device__ __forceinline__ float sum(uint32_t e) const {
        return (red[e] + red[RED + e]) + (red[2 * RED + e] + red[3 * RED + e]);
    }
    // After the last tile its epilogue has no MFMA stream to hide in: last(), the kernel's N_OUT outputs, then close() with the
    // segment's fill per query.  (The loop stays in the kernel: inside close() its LDS reads were not paired -- DESIGN 4.1b.)
    __device__ __forceinline__ void last() { have_prev = true; oi_ks_barrier(); }
    __device__ __forceinline__ void close(uint32_t n_queries, uint32_t *seg_cnt, uint32_t seg_cnt_stride) const {
        oi_ks_barrier();
        const uint32_t tid = threadIdx.x;
        if (tid < 32 * NQT && tid < n_queries) {
            const uint32_t c = seg_fill[tid];
            seg_cnt[(uint64_t)tid * seg_cnt_stride + blockIdx.x] = c < seg_cap ? c : seg_cap;
        }
    }
};

// ------------------------------------------------------------------ host
// Pool geometry for one chunk: one segment per workgroup, sized for the worst case (every score of every tile that workgroup
// owns passes the filter).
inline void oi_cosine_ksplit_geometry(const oi_ctx *ctx, uint64_t n_rows, uint32_t *n_segs, uint32_t *seg_cap) {
    const uint64_t n_tiles = (n_rows + OI_KS_TILE_ROWS - 1) / OI_KS_TILE_ROWS;
    const uint64_t grid = n_tiles < (uint64_t)ctx->num_cus ? n_tiles : (uint64_t)ctx->num_cus;
    *n_segs = (uint32_t)grid;
    *seg_cap = (uint32_t)((n_tiles + grid - 1) / grid) * OI_KS_TILE_ROWS;
}
// One workgroup per segment of p; `more`: what the kernel takes after the arguments the two kernels share.
template <int D, int NQT, class K, class Q, class... More>
static int oi_ksplit_launch(oi_ctx *ctx, K kernel, const float *rows, uint64_t row_begin, uint64_t row_end, const Q *q, uint32_t nq,
                            uint32_t doc_id_base, const PoolView &p, More... more) {
    constexpr size_t lds = OiKsplitTile<D, NQT>::LDS;
    OI_CHECK(oi_dyn_lds(ctx, reinterpret_cast<const void *>(kernel), lds));
    hipLaunchKernelGGL(kernel, dim3(p.n_segs), dim3(256), lds, ctx->stream, rows, row_begin, row_end, q, nq, doc_id_base, p.keys,
                       p.seg_cnt, p.seg_cnt_stride, p.tau_keys, p.stride, p.carry_cap, p.seg_cap, p.overflow, more...);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}
