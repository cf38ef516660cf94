// cosine_ksplit.hip -- the batch (B > 8) cosine scorer for gfx950: exact-f32 MFMA with the
// query block RESIDENT IN REGISTERS and the corpus streamed once through per-wave LDS rings.
//
// Why this shape.  At B = 64, d = 768 the scorer needs 2*64 = 128 flop per corpus byte... per
// 4-byte element, i.e. 32 flop/B: the f32 MFMA peak (157 TF) and the HBM rate (~6.3 TB/s
// achievable) bind at almost the same time (6.3 ms vs 4.9 ms for 10M rows), so the kernel must
// keep the matrix pipes issuing back to back WHILE streaming ~5 TB/s.  A conventional LDS-tiled
// GEMM re-stages the 196 KB query block (it does not fit in 160 KB of LDS) for every row tile.
// Instead:
//   * one persistent workgroup per CU, 4 waves, one per SIMD, each owning the full 512-register
//     file: the K dimension is split over the 4 waves (wave w owns k in [w*D/4, (w+1)*D/4)), so a
//     wave's slice of all 64 queries is 2 * D/8 = 192 VGPRs (d = 768) -- loaded once per launch;
//   * each wave streams ITS K-slice of the rows into ITS OWN LDS ring (6 x 4 KiB) with buffer_load ... lds, 5 slots ahead,
//     ordered only by its own counted s_waitcnt vmcnt -- no barrier for the ring, and the prefetch runs across tile
//     boundaries, under the epilogue (oi_ksplit_tile.h: the ring, the tile ownership, the descriptors);
//   * per 32-row tile (2 row tiles x 4 query tiles of 16) each wave issues D/4/4 * 2 * 4 = 384
//     v_mfma_f32_16x16x4_f32 (32-cycle issue, 4 accumulator registers: 12288 cycles at d = 768), two DMA pieces behind
//     MFMA sets e == 0 and e == 2 of every group of 16 k;
//   * the four partial 32x64 tiles meet in the deferred epilogue of oi_ksplit_tile.h, hosted INSIDE the next tile's MFMA
//     stream: barrier A behind group 1, the outputs spread over the groups after it, barrier B behind the last group.
//
// Operand map (cdna_hip_programming.md section 3): lane l supplies A[i = l&15][k = l>>4] and
// B[k = l>>4][j = l&15]; D[(l>>4)*4 + r][l&15] is accumulator register r.
#include <cstdlib>
#include <type_traits>

#include "oi_ksplit_tile.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int D, int NQT, bool FILT>
__global__ __launch_bounds__(256, 1) void cosine_ksplit16_filter(
    const float *__restrict__ rows, uint64_t row_begin, uint64_t row_end,
    const float *__restrict__ queries, // [32*NQT][D], zero padded
    uint32_t n_queries, uint32_t doc_id_base, uint64_t *pools, uint32_t *seg_cnt, uint32_t seg_cnt_stride,
    const uint32_t *tau_keys, uint64_t pool_stride, uint32_t carry_cap, uint32_t seg_cap, uint32_t *overflow,
    const uint32_t *run_gate, // run_gate != null: part of the gated exact pipeline (cosine_prefilter.hip)
    const uint4 *__restrict__ filt, const uint2 *__restrict__ attrs) { // FILT: the doc filter after the threshold
    if (run_gate && *run_gate == 0u) return;
    OI_CLAIM_WHOLE_SIMD(); // (MFMA kernel: nothing else may run on this CU -- oi_device.h)
    using Tile = OiKsplitTile<D, NQT>;
    constexpr int KS = Tile::KS, NKC = Tile::NKC, NBUF = Tile::NBUF, P = Tile::P, NG = Tile::NG, N_OUT = Tile::N_OUT;
    constexpr int NQ16 = 2 * NQT;        // query tiles of 16
    constexpr int QR = KS / 4;           // query registers per tile (one per k-step of 4)

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t li = lane & 15, kk = lane >> 4;

    // k-step (s, e) of this lane covers k = w*KS + 16 s + 4 kk + e  (any partition of k works as long
    // as A and B agree): both operands are then contiguous float4 per lane.
    float qreg[NQ16][QR];
#pragma unroll
    for (int t = 0; t < NQ16; ++t)
#pragma unroll
        for (int sg = 0; sg < KS / 16; ++sg) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(queries + (uint64_t)(16 * t + li) * D + w * KS + 16 * sg + 4 * kk);
            qreg[t][4 * sg + 0] = v[0]; qreg[t][4 * sg + 1] = v[1]; qreg[t][4 * sg + 2] = v[2]; qreg[t][4 * sg + 3] = v[3];
        }
    uint32_t tau[NQ16];
    oi_ks_thresholds<16>(tau, tau_keys, n_queries, li);

    Tile tile;
    if (!tile.open(smem, w, rows, row_begin, row_end, pools, carry_cap, seg_cap, pool_stride, doc_id_base, overflow)) return;
    // fragment (row tile rt, group g in the slot): row 16 rt + li, logical 16-B column 4 g + kk
    uint32_t frag_off[2][2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const uint32_t row = 16 * rt + li;
            frag_off[rt][g] = row * 128 + (((4 * g + kk) ^ ((row >> 1) & 7)) << 4);
        }
    tile.start_ring(lane, w);

    // element e = tid + 256 i of a partial tile is ((rt*NQ16 + t)*4 + reg)*64 + lane with
    // reg = tid>>6, t = i % NQ16, rt = i / NQ16
    auto epi_out = [&](int i) {
        const float s = tile.sum(tid + 256u * i);
        const uint32_t t = (uint32_t)i % NQ16, rt = (uint32_t)i / NQ16;
        const uint32_t q = 16u * t + li;
        const uint64_t row = tile.prev_row0 + 16u * rt + 4u * kk + w;
        OI_KS_OUT(tile, s, q, row, tau[t], !FILT || oi_doc_passes(filt[q], attrs[row]));
    };
    constexpr int OPG = (N_OUT + (NG - 4) - 1) / (NG - 4);      // outputs hosted per group, groups 2..
    static_assert(NG >= 6, "tile too short to host the deferred epilogue");

    for (uint64_t ti = 0; ti < tile.my_nt; ++ti) {
        tile.begin(ti);
        f32x4 acc[2][NQ16];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int t = 0; t < NQ16; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};

        oi_wait_vm<4 * (P - 1)>();
        f32x4 a0 = *reinterpret_cast<const f32x4 *>(tile.ring_rd + frag_off[0][0]);
        f32x4 a1 = *reinterpret_cast<const f32x4 *>(tile.ring_rd + frag_off[1][0]);
        oi_static_for<0, NG>([&](auto gi_) {
            constexpr int gi = decltype(gi_)::value;
            constexpr int kc = gi / 2, g = gi % 2;
            f32x4 n0 = a0, n1 = a1;
            if constexpr (g == 0) {
                n0 = *reinterpret_cast<const f32x4 *>(tile.ring_rd + (kc % NBUF) * OI_KS_SLOT_BYTES + frag_off[0][1]);
                n1 = *reinterpret_cast<const f32x4 *>(tile.ring_rd + (kc % NBUF) * OI_KS_SLOT_BYTES + frag_off[1][1]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int t = 0; t < NQ16; ++t) {
                    acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], qreg[t][gi * 4 + e], acc[0][t], 0, 0, 0);
                    acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], qreg[t][gi * 4 + e], acc[1][t], 0, 0, 0);
                }
                if (e == 0 || e == 2) tile.refill(kc + P, 2 * g + (e >> 1)); // two DMA pieces per group
            }
            if constexpr (gi == 1) oi_ks_barrier();                                       // (A) partials visible
            if constexpr (gi >= 2 && gi < NG - 1) {
#pragma unroll
                for (int o = 0; o < OPG; ++o)
                    if ((gi - 2) * OPG + o < N_OUT) epi_out((gi - 2) * OPG + o);
            }
            if constexpr (gi == NG - 1) oi_ks_barrier();                                  // (B) `red` is free again
            if constexpr (g == 1 && kc + 1 < NKC) {
                oi_wait_vm<4 * (P - 1)>();
                n0 = *reinterpret_cast<const f32x4 *>(tile.ring_rd + ((kc + 1) % NBUF) * OI_KS_SLOT_BYTES + frag_off[0][0]);
                n1 = *reinterpret_cast<const f32x4 *>(tile.ring_rd + ((kc + 1) % NBUF) * OI_KS_SLOT_BYTES + frag_off[1][0]);
            }
            a0 = n0; a1 = n1;
        });

#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int t = 0; t < NQ16; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) tile.my_red[((rt * NQ16 + t) * 4 + r) * 64 + lane] = acc[rt][t][r];
        tile.next(ti);
    }
    tile.last();
#pragma unroll
    for (int i = 0; i < N_OUT; ++i) epi_out(i);
    tile.close(n_queries, seg_cnt, seg_cnt_stride);
}

template <int D, int NQT>
static int launch_ksplit16(oi_ctx *ctx, const float *rows, uint64_t row_begin, uint64_t row_end, const float *q,
                           uint32_t nq, uint32_t doc_id_base, const PoolView &p, const uint32_t *run_gate) {
    auto kernel = p.filt ? cosine_ksplit16_filter<D, NQT, true> : cosine_ksplit16_filter<D, NQT, false>;
    return oi_ksplit_launch<D, NQT>(ctx, kernel, rows, row_begin, row_end, q, nq, doc_id_base, p, run_gate, p.filt, p.attrs);
}

bool oi_cosine_ksplit_supported(uint32_t dim) { return dim == 384 || dim == 768 || dim == 1024; }

// One group of <= 64 queries (zero padded to 32 or 64 rows at `q`).
int oi_launch_cosine_ksplit(oi_ctx *ctx, const float *rows, uint64_t row_begin, uint64_t row_end, uint32_t dim,
                            const float *q, uint32_t nq, bool two_tiles, uint32_t doc_id_base, const PoolView &p,
                            const uint32_t *run_gate) {
#define OI_KS(DD)                                                                                                 \
    case DD:                                                                                                      \
        return two_tiles ? launch_ksplit16<DD, 2>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p, run_gate) \
                         : launch_ksplit16<DD, 1>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p, run_gate);
    switch (dim) {
        OI_KS(384)
        OI_KS(768)
        OI_KS(1024)
        default:
            oi_set_error("cosine_ksplit: dim %u not instantiated", dim);
            return OI_ERR_UNSUPPORTED;
    }
#undef OI_KS
}
