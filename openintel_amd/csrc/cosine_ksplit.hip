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
//   * each wave streams ITS K-slice of the rows into ITS OWN LDS ring (6 x 4 KiB) with
//     buffer_load ... lds (oi_dma_piece: full 128-B lines, swizzled through the per-lane source
//     offset so the ds_read_b128 fragment reads are conflict-free; a wave-uniform descriptor and a
//     32-bit per-lane offset are short enough to issue under a matrix instruction), 5 slots ahead,
//     ordered only by its own counted s_waitcnt vmcnt -- no barrier for the ring, and the prefetch
//     runs across tile boundaries, under the epilogue;
//   * per 32-row tile (2 row tiles x 4 query tiles of 16) each wave issues D/4/4 * 2 * 4 = 384
//     v_mfma_f32_16x16x4_f32 (32-cycle issue, 4 accumulator registers: 12288 cycles at d = 768),
//     then the four partial 32x64 tiles are summed through LDS in a fixed order, (w0 + w1) +
//     (w2 + w3), compared with the per-query threshold, and the survivors stored straight into THIS
//     workgroup's private segment of each query's candidate pool (fill counters in LDS): no global
//     atomic, no returning memory operation, hence nothing that would make a wave drain its DMA
//     ring;
//   * that epilogue is deferred: a tile's partial sums are written to LDS right after its last
//     MFMA, and the cross-wave sum + filter of tile t rides INSIDE tile t+1's MFMA stream (barrier A
//     behind group 1, the outputs spread over the groups after it, barrier B behind the last group),
//     so its LDS round trips and VALU work issue in the shadow of the matrix instructions.
//
// Operand map (cdna_hip_programming.md section 3): lane l supplies A[i = l&15][k = l>>4] and
// B[k = l>>4][j = l&15]; D[(l>>4)*4 + r][l&15] is accumulator register r.
#include <cstdlib>
#include <type_traits>

#include "oi_device.h"
#include "oi_internal.h"
#include "oi_lds_dma.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

#define KS_TILE_ROWS 32
#define KS_CHUNK_K 32                       // floats of K per ring slot row (128 B)
#define KS_SLOT_BYTES (KS_TILE_ROWS * KS_CHUNK_K * 4) // 4 KiB

__device__ __forceinline__ void ks_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

template <int D, int NQT, bool FILT>
__global__ __launch_bounds__(256, 1) void cosine_ksplit16_filter(
    const float *__restrict__ rows, uint64_t row_begin, uint64_t row_end,
    const float *__restrict__ queries, // [32*NQT][D], zero padded
    uint32_t n_queries, uint32_t doc_id_base, uint64_t *pools, uint32_t *seg_cnt, uint32_t seg_cnt_stride,
    const uint32_t *tau_keys, uint64_t pool_stride, uint32_t carry_cap, uint32_t seg_cap, uint32_t *overflow,
    const uint32_t *run_gate, // run_gate != null: part of the gated exact pipeline (cosine_prefilter.hip)
    const uint4 *__restrict__ filt, const uint2 *__restrict__ attrs) { // FILT: the doc filter after the threshold
    if (run_gate && *run_gate == 0u) return;
    constexpr int KS = D / 4, NKC = KS / KS_CHUNK_K, NBUF = NKC <= 6 ? NKC : NKC / 2, P = NBUF - 1;
    constexpr int NQ16 = 2 * NQT;        // query tiles of 16
    constexpr int QR = KS / 4;           // query registers per tile (one per k-step of 4)
    constexpr int NG = NKC * 2;          // MFMA groups (16 k each) per tile
    static_assert(KS % KS_CHUNK_K == 0 && NKC % NBUF == 0 && P >= 1 && P < NKC, "unsupported D");
    constexpr int RED_FLOATS = NQT * 16 * 64;

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    unsigned char *ring = smem;
    float *red = reinterpret_cast<float *>(smem + 4 * NBUF * KS_SLOT_BYTES);
    uint32_t *seg_fill = reinterpret_cast<uint32_t *>(red + 4 * RED_FLOATS);

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
    OI_CLAIM_WHOLE_SIMD(); // (MFMA kernel: nothing else may run on this CU -- oi_device.h)
            const f32x4 v = *reinterpret_cast<const f32x4 *>(queries + (uint64_t)(16 * t + li) * D + w * KS + 16 * sg + 4 * kk);
            qreg[t][4 * sg + 0] = v[0]; qreg[t][4 * sg + 1] = v[1]; qreg[t][4 * sg + 2] = v[2]; qreg[t][4 * sg + 3] = v[3];
        }
    uint32_t tau[NQ16];
#pragma unroll
    for (int t = 0; t < NQ16; ++t) {
        const uint32_t q = 16u * t + li;
        tau[t] = q < n_queries ? tau_keys[q] : 0xFFFFFFFFu;
    }
    if (tid < 64) seg_fill[tid] = 0;

    const uint64_t n_rows = row_end - row_begin;
    const uint64_t n_tiles = (n_rows + KS_TILE_ROWS - 1) / KS_TILE_ROWS;
    const uint64_t my_nt = blockIdx.x < n_tiles ? (n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    if (my_nt == 0) return;
    uint64_t *my_seg = pools + carry_cap + (uint64_t)blockIdx.x * seg_cap;

    uint32_t voff[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const uint32_t prow = 8 * m + (lane >> 3);
        const uint32_t pcol = ((lane & 7) ^ ((prow >> 1) & 7)) * 4 + w * KS;
        voff[m] = prow * (uint32_t)(D * 4) + pcol * 4u;
    }
    const uint32_t ring_w = oi_lds_addr(ring) + w * (NBUF * KS_SLOT_BYTES);
    const unsigned char *ring_rd = ring + w * (NBUF * KS_SLOT_BYTES);
    // fragment (row tile rt, group g in the slot): row 16 rt + li, logical 16-B column 4 g + kk
    uint32_t frag_off[2][2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const uint32_t row = 16 * rt + li;
            frag_off[rt][g] = row * 128 + (((4 * g + kk) ^ ((row >> 1) & 7)) << 4);
        }
    // Past the workgroup's last tile the descriptor is EMPTY (its loads return zeros): the tile loop then needs no
    // branch around the prefetch and a single set of wait counts -- a branch-free tile body.
    auto tile_srd = [&](uint64_t ti) {
        const uint64_t r0 = row_begin + (blockIdx.x + (ti < my_nt ? ti : 0) * gridDim.x) * (uint64_t)KS_TILE_ROWS;
        return oi_make_srd(rows + r0 * D, ti < my_nt ? (row_end - r0) * (uint64_t)(D * 4) : 0ull);
    };
    oi_u32x4 cur = tile_srd(0), nxt = tile_srd(1);
    __builtin_amdgcn_s_waitcnt(0x0F70); // retire every load hipcc knows about before the DMA ring starts
#pragma unroll
    for (int kc = 0; kc < P; ++kc)
#pragma unroll
        for (int m = 0; m < 4; ++m)
            oi_dma_piece(cur, voff[m], kc * KS_CHUNK_K * 4, ring_w + (kc % NBUF) * KS_SLOT_BYTES + m * 1024);

    float *my_red = red + w * RED_FLOATS;
    uint64_t prev_row0 = 0;
    bool have_prev = false; // false during the first tile: `red` holds nothing yet
    // element e = tid + 256 i of a partial tile is ((rt*NQ16 + t)*4 + reg)*64 + lane with
    // reg = tid>>6, t = i % NQ16, rt = i / NQ16
    auto epi_out = [&](int i) {
        const uint32_t e = tid + 256u * i;
        const float s = (red[e] + red[RED_FLOATS + e]) + (red[2 * RED_FLOATS + e] + red[3 * RED_FLOATS + e]);
        const uint32_t t = (uint32_t)i % NQ16, rt = (uint32_t)i / NQ16;
        const uint32_t q = 16u * t + li;
        const uint64_t row = prev_row0 + 16u * rt + 4u * kk + w;
        if (have_prev && row < row_end && s == s && oi_f32_key(s) >= tau[t] && (!FILT || oi_doc_passes(filt[q], attrs[row]))) {
            const uint32_t pos = atomicAdd(&seg_fill[q], 1u); // LDS
            if (pos < seg_cap) my_seg[(uint64_t)q * pool_stride + pos] = oi_rank_key(s, doc_id_base + (uint32_t)row);
            else *overflow = 1u;
        }
    };
    constexpr int N_OUT = NQT * 4;                              // outputs per thread and tile
    constexpr int OPG = (N_OUT + (NG - 4) - 1) / (NG - 4);      // outputs hosted per group, groups 2..
    static_assert(NG >= 6, "tile too short to host the deferred epilogue");

    for (uint64_t ti = 0; ti < my_nt; ++ti) {
        have_prev = ti > 0;
        f32x4v acc[2][NQ16];
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int t = 0; t < NQ16; ++t) acc[rt][t] = f32x4v{0.f, 0.f, 0.f, 0.f};

        oi_wait_vm<4 * (P - 1)>();
        f32x4 a0 = *reinterpret_cast<const f32x4 *>(ring_rd + frag_off[0][0]);
        f32x4 a1 = *reinterpret_cast<const f32x4 *>(ring_rd + frag_off[1][0]);
        oi_static_for<0, NG>([&](auto gi_) {
            constexpr int gi = decltype(gi_)::value;
            constexpr int kc = gi / 2, g = gi % 2;
            constexpr int sn = kc + P;
            f32x4 n0 = a0, n1 = a1;
            if constexpr (g == 0) {
                n0 = *reinterpret_cast<const f32x4 *>(ring_rd + (kc % NBUF) * KS_SLOT_BYTES + frag_off[0][1]);
                n1 = *reinterpret_cast<const f32x4 *>(ring_rd + (kc % NBUF) * KS_SLOT_BYTES + frag_off[1][1]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
#pragma unroll
                for (int t = 0; t < NQ16; ++t) {
                    acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], qreg[t][gi * 4 + e], acc[0][t], 0, 0, 0);
                    acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], qreg[t][gi * 4 + e], acc[1][t], 0, 0, 0);
                }
                if (e == 0 || e == 2) { // two DMA pieces per group
                    constexpr int dummy = 0; (void)dummy;
                    const int m = 2 * g + (e >> 1);
                    if constexpr (sn < NKC)
                        oi_dma_piece(cur, voff[m], sn * KS_CHUNK_K * 4, ring_w + (sn % NBUF) * KS_SLOT_BYTES + m * 1024);
                    else
                        oi_dma_piece(nxt, voff[m], (sn - NKC) * KS_CHUNK_K * 4,
                                       ring_w + (sn % NBUF) * KS_SLOT_BYTES + m * 1024, false);
                }
            }
            if constexpr (gi == 1) ks_barrier();                                          // (A) partials visible
            if constexpr (gi >= 2 && gi < NG - 1) {
#pragma unroll
                for (int o = 0; o < OPG; ++o)
                    if ((gi - 2) * OPG + o < N_OUT) epi_out((gi - 2) * OPG + o);
            }
            if constexpr (gi == NG - 1) ks_barrier();                                     // (B) `red` is free again
            if constexpr (g == 1 && kc + 1 < NKC) {
                oi_wait_vm<4 * (P - 1)>();
                n0 = *reinterpret_cast<const f32x4 *>(ring_rd + ((kc + 1) % NBUF) * KS_SLOT_BYTES + frag_off[0][0]);
                n1 = *reinterpret_cast<const f32x4 *>(ring_rd + ((kc + 1) % NBUF) * KS_SLOT_BYTES + frag_off[1][0]);
            }
            a0 = n0; a1 = n1;
        });

#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int t = 0; t < NQ16; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) my_red[((rt * NQ16 + t) * 4 + r) * 64 + lane] = acc[rt][t][r];
        prev_row0 = row_begin + (blockIdx.x + ti * gridDim.x) * (uint64_t)KS_TILE_ROWS;
        cur = nxt;
        nxt = tile_srd(ti + 2);
    }
    have_prev = my_nt > 0;
    ks_barrier();
#pragma unroll
    for (int i = 0; i < N_OUT; ++i) epi_out(i);
    ks_barrier();
    if (tid < 32 * NQT && tid < n_queries) {
        const uint32_t c = seg_fill[tid];
        seg_cnt[(uint64_t)tid * seg_cnt_stride + blockIdx.x] = c < seg_cap ? c : seg_cap;
    }
}

template <int D, int NQT>
static int launch_ksplit16(oi_ctx *ctx, const float *rows, uint64_t row_begin, uint64_t row_end, const float *q,
                           uint32_t nq, uint32_t doc_id_base, const PoolView &p) {
    constexpr int KS = D / 4, NKC = KS / KS_CHUNK_K, NBUF = NKC <= 6 ? NKC : NKC / 2;
    constexpr size_t smem = 4 * NBUF * KS_SLOT_BYTES + 4 * (NQT * 16 * 64) * 4 + 64 * 4;
    auto kernel = p.filt ? cosine_ksplit16_filter<D, NQT, true> : cosine_ksplit16_filter<D, NQT, false>;
    OI_CHECK(oi_dyn_lds(ctx, reinterpret_cast<const void *>(kernel), (size_t)(smem)));
    hipLaunchKernelGGL(kernel, dim3(p.n_segs), dim3(256), smem, ctx->stream, rows,
                       row_begin, row_end, q, nq, doc_id_base, p.keys, p.seg_cnt, p.seg_cnt_stride, p.tau_keys,
                       p.stride, p.carry_cap, p.seg_cap, p.overflow, ctx->run_gate, p.filt, p.attrs);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

bool oi_cosine_ksplit_supported(uint32_t dim) { return dim == 384 || dim == 768 || dim == 1024; }

// Pool geometry for one chunk: one segment per workgroup, sized for the worst case (every score of
// every tile that workgroup owns passes the filter).
void oi_cosine_ksplit_geometry(const oi_ctx *ctx, uint64_t n_rows, uint32_t *n_segs, uint32_t *seg_cap) {
    const uint64_t n_tiles = (n_rows + KS_TILE_ROWS - 1) / KS_TILE_ROWS;
    const uint64_t grid = n_tiles < (uint64_t)ctx->num_cus ? n_tiles : (uint64_t)ctx->num_cus;
    *n_segs = (uint32_t)grid;
    *seg_cap = (uint32_t)((n_tiles + grid - 1) / grid) * KS_TILE_ROWS;
}

// One group of <= 64 queries (zero padded to 32 or 64 rows at `q`).
int oi_launch_cosine_ksplit(oi_ctx *ctx, const float *rows, uint64_t row_begin, uint64_t row_end, uint32_t dim,
                            const float *q, uint32_t nq, bool two_tiles, uint32_t doc_id_base, const PoolView &p) {
#define OI_KS(DD)                                                                                       \
    case DD:                                                                                            \
        return two_tiles ? launch_ksplit16<DD, 2>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p) \
                         : launch_ksplit16<DD, 1>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
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
