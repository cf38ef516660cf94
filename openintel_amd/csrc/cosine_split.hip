// cosine_split.hip -- the batch cosine scorer over an f32 corpus with SPLIT-PRECISION products
// (opt-in: oi_set_cosine_mode(ctx, OI_COSINE_SPLIT); the default stays the exact-f32 MFMA kernel).
//
// Every f32 value is the exact sum of three bf16 values, x = h + m + l (8 significant bits each: h is
// x's upper half, m the upper half of the exact remainder x - h, l what is left).  A product of two
// bf16 values is exact in f32, so
//     x * q = (h + m + l)(H + M + L) = hH + (hM + mH) + (mM + hL + lH) + [mL + lM + lL]
// and dropping the bracket (<= 2^-23 relative, below f32's own rounding) gives an f32-grade dot product
// from SIX bf16 MFMAs.  On gfx950 v_mfma_f32_32x32x16_bf16 runs 16x the flop rate of the f32 MFMA, so
// the six cost 3/8 of the f32 instruction's cycles: the scorer stops being matrix-pipe-bound (6.25 ms
// of f32 MFMA per 10M x 768 x 64 batch) and becomes HBM-bound (30.7 GB, ~5.5 ms).  Measured error vs
// f64 on unit vectors: ~4e-8 (plain f32 accumulation: ~1e-7); the parity bar is 1e-5.
//
// Shape: one workgroup per CU, 4 waves splitting K (wave w owns k in [w D/4, (w+1) D/4)):
//   * the wave's K-slice of all 64 queries, already split into (H, M, L) bf16 planes by the staging
//     kernel, lives in registers as MFMA B operands (3 x 96 VGPRs at d = 768);
//   * the f32 rows stream through the wave's own LDS ring (4 KiB slots of 32 rows x 32 floats; oi_ksplit_tile.h: the ring,
//     the tile ownership and the deferred epilogue are the exact-f32 kernel's, cosine_ksplit.hip);
//   * per 16 k: two ds_read_b128 (the lane's 8 consecutive floats), ~44 VALU to split and pack them into
//     the three A operands -- issued in the shadow of the 12 MFMAs (32 cycles each) they feed;
//   * the big term hH accumulates apart from the five small ones (added at the end), then the four waves'
//     partial tiles are summed through LDS in a fixed order, filtered against the per-query threshold and
//     appended to this workgroup's private pool segment -- inside the next tile's MFMA stream: barrier A before
//     k-step EPI_G0, the outputs spread over the k-steps from it, barrier B behind the last one.
#include <cstdlib>
#include <type_traits>

#include "oi_ksplit_tile.h"

typedef float cs_f32x16 __attribute__((ext_vector_type(16)));
typedef float cs_f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 cs_bf16x8 __attribute__((ext_vector_type(8)));

// 8 consecutive floats of a row -> the three bf16x8 A operands (h, m, l), x = h + m + l exactly.
union CsPack {
    uint32_t u[4];
    cs_bf16x8 v;
};
__device__ __forceinline__ void cs_split8(const cs_f32x4 &a, const cs_f32x4 &b, cs_bf16x8 &h, cs_bf16x8 &m, cs_bf16x8 &l) {
    float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    float r1[8], r2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        r1[i] = x[i] - __uint_as_float(__float_as_uint(x[i]) & 0xFFFF0000u);   // exact
        r2[i] = r1[i] - __uint_as_float(__float_as_uint(r1[i]) & 0xFFFF0000u); // exact, <= 8 significant bits
    }
    CsPack ph, pm, pl;
#pragma unroll
    for (int j = 0; j < 4; ++j) { // upper halves of two floats -> one dword: bytes [hi.3, hi.2, lo.3, lo.2]
        ph.u[j] = __builtin_amdgcn_perm(__float_as_uint(x[2 * j + 1]), __float_as_uint(x[2 * j]), 0x07060302u);
        pm.u[j] = __builtin_amdgcn_perm(__float_as_uint(r1[2 * j + 1]), __float_as_uint(r1[2 * j]), 0x07060302u);
        pl.u[j] = __builtin_amdgcn_perm(__float_as_uint(r2[2 * j + 1]), __float_as_uint(r2[2 * j]), 0x07060302u);
    }
    h = ph.v; m = pm.v; l = pl.v;
}

template <int D, int NQT, int DBG = 0> // DBG (diagnostic builds, wrong results): 1 no DMA, 2 no MFMA, 4 no split arithmetic
__global__ __launch_bounds__(256, 1) void cosine_split_filter(
    const float *__restrict__ rows, uint64_t row_begin, uint64_t row_end,
    const uint16_t *__restrict__ qsplit, // bf16 [3 planes: H, M, L][32*NQT][D], zero padded
    uint32_t n_queries, uint32_t doc_id_base, uint64_t *pools, uint32_t *seg_cnt, uint32_t seg_cnt_stride,
    const uint32_t *tau_keys, uint64_t pool_stride, uint32_t carry_cap, uint32_t seg_cap, uint32_t *overflow) {
    OI_CLAIM_WHOLE_SIMD(); // (MFMA kernel: nothing else may run on this CU -- oi_device.h)
    using Tile = OiKsplitTile<D, NQT>;
    constexpr int KS = Tile::KS, NKC = Tile::NKC, NBUF = Tile::NBUF, P = Tile::P, NG = Tile::NG, N_OUT = Tile::N_OUT;
    constexpr int KSTEPS = KS / 16;      // MFMA groups per tile and wave (two per slot)
    static_assert(3 * NQT * KSTEPS * 4 <= 300, "the split query block must fit the register file");

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t li = lane & 31, lh = lane >> 5;

    // ---- this wave's K-slice of every query, three planes: B[k = 16 s + 8 lh + 0..7][n = li]
    cs_bf16x8 qh[NQT][KSTEPS], qm[NQT][KSTEPS], ql[NQT][KSTEPS];
    constexpr uint64_t PLANE = (uint64_t)32 * NQT * D;
#pragma unroll
    for (int t = 0; t < NQT; ++t)
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            const uint64_t o = (uint64_t)(32 * t + li) * D + w * KS + 16 * s + 8 * lh;
            qh[t][s] = *reinterpret_cast<const cs_bf16x8 *>(qsplit + o);
            qm[t][s] = *reinterpret_cast<const cs_bf16x8 *>(qsplit + PLANE + o);
            ql[t][s] = *reinterpret_cast<const cs_bf16x8 *>(qsplit + 2 * PLANE + o);
        }
    uint32_t tau[NQT];
    oi_ks_thresholds<32>(tau, tau_keys, n_queries, li);

    Tile tile;
    if (!tile.open(smem, w, rows, row_begin, row_end, pools, carry_cap, seg_cap, pool_stride, doc_id_base, overflow)) return;
    // fragment (slot half g in {0,1}): the lane's floats 16 g + 8 lh .. + 8 = logical 16-B columns 4g + 2lh, + 1
    uint32_t frag_off[2][2];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int c = 0; c < 2; ++c) frag_off[g][c] = li * 128 + (((4 * g + 2 * lh + c) ^ ((li >> 1) & 7)) << 4);

    tile.start_ring(lane, w, (DBG & 1) != 0);

    // element e = tid + 256 i of a partial tile is (t * 16 + r) * 64 + lane with t = i >> 2, r = (e >> 6) & 15: register r
    // of query tile t, D[row (r&3) + 8 (r>>2) + 4 lh][query 32 t + li]
    auto epi_out = [&](int i) {
        const uint32_t e = tid + 256u * i;
        const float s = tile.sum(e);
        const uint32_t t = i >> 2, r = (e >> 6) & 15u;
        OI_KS_OUT(tile, s, 32u * t + li, tile.prev_row0 + (r & 3u) + 8u * (r >> 2) + 4u * lh, tau[t], true);
    };
    constexpr int EPI_G0 = 1;                                // first k-step with outputs
    constexpr int EPI_PER = (N_OUT + (NG - 2) - 1) / (NG - 2); // outputs per thread and k-step (2 at d = 384)
    constexpr int EPI_STEPS = (N_OUT + EPI_PER - 1) / EPI_PER;
    constexpr int EPI_GB = EPI_G0 + EPI_STEPS;               // k-step of barrier B
    static_assert(EPI_GB <= NG - 1, "tile too short to host the deferred epilogue");

    for (uint64_t ti = 0; ti < tile.my_nt; ++ti) {
        // (`red` holds the previous tile.  With two query tiles the flag is computed from ti here; with one it is carried from the
        // end of the first tile, below.  The other form costs <768, 2> 16 register moves inside its MFMA stream and 0.5 % of its
        // step, and <768, 1> 0.7 % -- DESIGN 4.1b)
        if constexpr (NQT == 2) tile.begin(ti);
        // hH accumulates apart from the five small terms; with one query tile the small terms use two
        // accumulators so that no MFMA waits for the one issued right before it
        cs_f32x16 acc[NQT], cor[NQT], cor2; // (cor2: with one query tile only)
#pragma unroll
        for (int t = 0; t < NQT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc[t][r] = 0.f; cor[t][r] = 0.f; }
#pragma unroll
        for (int r = 0; r < 16; ++r) cor2[r] = 0.f;

        oi_wait_vm<4 * (P - 1)>();
        cs_bf16x8 ah, am, al; // A operands of the current k-step
        {
            const cs_f32x4 f0 = *reinterpret_cast<const cs_f32x4 *>(tile.ring_rd + frag_off[0][0]);
            const cs_f32x4 f1 = *reinterpret_cast<const cs_f32x4 *>(tile.ring_rd + frag_off[0][1]);
            if constexpr ((DBG & 4) != 0) { CsPack pk; pk.u[0] = __float_as_uint(f0[0]); pk.u[1] = __float_as_uint(f0[1]); pk.u[2] = __float_as_uint(f1[0]); pk.u[3] = __float_as_uint(f1[1]); ah = am = al = pk.v; }
            else cs_split8(f0, f1, ah, am, al);
        }
        oi_static_for<0, NG>([&](auto gi_) {
            constexpr int gi = decltype(gi_)::value; // k-step of the tile
            constexpr int kc = gi / 2, g = gi % 2;
            // The NEXT k-step's floats are read now and split into its three operands WHILE this k-step's MFMAs
            // run: one wave per SIMD issues in order, so the split has to sit between the MFMAs in program order
            // (sched_group_barrier below) to execute in their shadow.
            cs_bf16x8 nh = ah, nm = am, nl = al;
            if constexpr (gi + 1 < NG) {
                constexpr int nslot = g == 0 ? kc : kc + 1, nhalf = g == 0 ? 1 : 0;
                const cs_f32x4 f0 = *reinterpret_cast<const cs_f32x4 *>(tile.ring_rd + (nslot % NBUF) * OI_KS_SLOT_BYTES + frag_off[nhalf][0]);
                const cs_f32x4 f1 = *reinterpret_cast<const cs_f32x4 *>(tile.ring_rd + (nslot % NBUF) * OI_KS_SLOT_BYTES + frag_off[nhalf][1]);
                if constexpr ((DBG & 4) != 0) { CsPack pk; pk.u[0] = __float_as_uint(f0[0]); pk.u[1] = __float_as_uint(f0[1]); pk.u[2] = __float_as_uint(f1[0]); pk.u[3] = __float_as_uint(f1[1]); nh = nm = nl = pk.v; }
                else cs_split8(f0, f1, nh, nm, nl);
            }
            // twelve (six) MFMAs, ordered so that consecutive ones never share an accumulator; the small terms
            // are added smallest first
            if constexpr ((DBG & 2) != 0) {
                asm volatile("" ::"v"(ah), "v"(am), "v"(al));
            } else if constexpr (NQT == 2) {
                cor[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, qh[0][gi], cor[0], 0, 0, 0);
                cor[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, qh[1][gi], cor[1], 0, 0, 0);
                cor[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, ql[0][gi], cor[0], 0, 0, 0);
                cor[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, ql[1][gi], cor[1], 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, qh[0][gi], acc[0], 0, 0, 0);
                cor[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, qm[0][gi], cor[0], 0, 0, 0);
                cor[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, qm[1][gi], cor[1], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, qh[1][gi], acc[1], 0, 0, 0);
                cor[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, qh[0][gi], cor[0], 0, 0, 0);
                cor[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, qh[1][gi], cor[1], 0, 0, 0);
                cor[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, qm[0][gi], cor[0], 0, 0, 0);
                cor[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, qm[1][gi], cor[1], 0, 0, 0);
            } else {
                cor[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, qh[0][gi], cor[0], 0, 0, 0);
                cor2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, ql[0][gi], cor2, 0, 0, 0);
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, qh[0][gi], acc[0], 0, 0, 0);
                cor[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, qm[0][gi], cor[0], 0, 0, 0);
                cor2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, qh[0][gi], cor2, 0, 0, 0);
                cor[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, qm[0][gi], cor[0], 0, 0, 0);
            }
            if constexpr ((DBG & 6) == 0) {
                // issue order of this k-step: the two LDS reads of the next fragment first, two MFMAs to cover
                // their latency, then a handful of the split's VALU instructions after every further MFMA
                __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
#pragma unroll
                for (int i = 2; i < NQT * 6; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x002, NQT == 2 ? 6 : 15, 0);
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                }
            }
            // two DMA pieces per k-step: slot kc + P goes into the buffer slot kc - 1 has vacated
#pragma unroll
            for (int m = 2 * g; m < 2 * g + 2; ++m) tile.refill(kc + P, m, (DBG & 1) != 0);
            if constexpr (gi == EPI_G0 - 1 && !(DBG & 8)) oi_ks_barrier();                        // (A) partials visible
            if constexpr (gi >= EPI_G0 && gi < EPI_GB && !(DBG & 8)) {
#pragma unroll
                for (int o = 0; o < EPI_PER; ++o)
                    if ((gi - EPI_G0) * EPI_PER + o < N_OUT) epi_out((gi - EPI_G0) * EPI_PER + o);
            }
            if constexpr (gi == EPI_GB && !(DBG & 8)) oi_ks_barrier();                            // (B) `red` is free again
            // the next k-step reads slot kc + 1 when this one is the slot's first half: it has to have landed
            // (the two pieces of slot kc + P issued just above may still be in flight with P - 2 younger slots)
            if constexpr (g == 0 && kc + 1 < NKC) oi_wait_vm<4 * (P - 2) + 2>();
            ah = nh; am = nm; al = nl;
        });

        // this tile's partial sums -> LDS (summed across the waves during the next tile, or below)
#pragma unroll
        for (int t = 0; t < NQT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                tile.my_red[(t * 16 + r) * 64 + lane] = acc[t][r] + (NQT == 1 ? cor[t][r] + cor2[r] : cor[t][r]);
        tile.next(ti);
        if constexpr (NQT == 1) tile.have_prev = true;
    }
    tile.last();
#pragma unroll
    for (int i = 0; i < N_OUT; ++i) epi_out(i);
    tile.close(n_queries, seg_cnt, seg_cnt_stride);
}

// ------------------------------------------------------------------ query staging: f32 -> (H, M, L) bf16 planes
__global__ __launch_bounds__(256) void cs_stage_queries(const float *__restrict__ q, uint32_t n_queries, uint32_t n_padded,
                                                        uint32_t dim, uint16_t *__restrict__ out) {
    const uint64_t plane = (uint64_t)n_padded * dim;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < plane; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t)(i / dim);
        uint16_t h = 0, m = 0, l = 0;
        if (row < n_queries) {
            const float x = q[i];
            const uint32_t ux = __float_as_uint(x);
            const float r1 = x - __uint_as_float(ux & 0xFFFF0000u);
            const uint32_t u1 = __float_as_uint(r1);
            const float r2 = r1 - __uint_as_float(u1 & 0xFFFF0000u);
            h = (uint16_t)(ux >> 16);
            m = (uint16_t)(u1 >> 16);
            l = (uint16_t)(__float_as_uint(r2) >> 16);
        }
        out[i] = h;
        out[plane + i] = m;
        out[2 * plane + i] = l;
    }
}

// ------------------------------------------------------------------ host
bool oi_cosine_split_supported(uint32_t dim) { return dim == 384 || dim == 768; }

template <int D, int NQT, int DBG = 0>
static int launch_split(oi_ctx *ctx, const float *rows, uint64_t row_begin, uint64_t row_end, const uint16_t *q,
                        uint32_t nq, uint32_t doc_id_base, const PoolView &p) {
    return oi_ksplit_launch<D, NQT>(ctx, cosine_split_filter<D, NQT, DBG>, rows, row_begin, row_end, q, nq, doc_id_base, p);
}

// One group of <= 64 queries (f32, device) over rows [row_begin, row_end); the pool has oi_cosine_ksplit_geometry.
int oi_launch_cosine_split(oi_ctx *ctx, const float *rows, uint64_t row_begin, uint64_t row_end, uint32_t dim,
                           const float *d_queries, uint32_t nq, uint32_t doc_id_base, const PoolView &p) {
    OI_REQUIRE(oi_cosine_split_supported(dim), "cosine (split products): dim %u not instantiated (384, 768)", dim);
    const uint32_t n_padded = nq > 32 ? 64u : 32u;
    DevBuf &qb = ctx->buf("q_split");
    OI_CHECK(qb.ensure(sizeof(uint16_t) * 3ull * 64 * OI_MAX_DIM));
    {
        const uint64_t total = (uint64_t)n_padded * dim;
        hipLaunchKernelGGL(cs_stage_queries, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_queries, nq,
                           n_padded, dim, qb.as<uint16_t>());
        OI_HIP_CHECK(hipGetLastError());
    }
    const uint16_t *q = qb.as<uint16_t>();
#ifdef OI_ABLATION
    static const int dbg = oi_ablation_env("OI_CS_DEBUG") ? atoi(oi_ablation_env("OI_CS_DEBUG")) : 0; // ablation builds (timings only)
    if (dim == 768 && nq > 32 && dbg) {
        switch (dbg) {
            case 1: return launch_split<768, 2, 1>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
            case 2: return launch_split<768, 2, 2>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
            case 4: return launch_split<768, 2, 4>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
            case 6: return launch_split<768, 2, 6>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
            case 8: return launch_split<768, 2, 8>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
            case 9: return launch_split<768, 2, 9>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
            case 15: return launch_split<768, 2, 15>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
            default: break;
        }
    }
#endif
    if (dim == 768) return nq > 32 ? launch_split<768, 2>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p)
                                   : launch_split<768, 1>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
    return nq > 32 ? launch_split<384, 2>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p)
                   : launch_split<384, 1>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
}
