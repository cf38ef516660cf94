// cosine_screen_copy.hip -- the bf16 screen of cosine_prefilter.hip reading the index's bf16 SCREENING COPY of the rows
// (round 5: the default batch scorer of an f32 corpus whenever the index holds the copy -- oi_index_finalize makes it when it
// fits the stated HBM budget).
//
// Builder-defined like the rest of the retrieval path (the reference has none).
//
// What changes against cosine_screen_filter and what does not.  The copy is bf16(x) made ONCE with the screen's own
// conversion (pf_make_copy_kernel: v_cvt_pk_bf16_f32), so the screen's products, the measured E = max |bf16(x) - x|, the
// margin eps_q, the survivors and their exact f32 rescoring FROM THE f32 ROWS are the same: the lists are the same bit for
// bit (tests/test_gpu_prefilter.py).  Only the bytes differ: 2 d per row and batch instead of 4 d -- the kernel is an HBM
// stream, so that is the whole point.
//
// The kernel is setup, the shared tile step and the shared pool epilogue of oi_screen_tile.h (OiCopyRing, OiPoolSink); what
// follows says why they are shaped as they are.
// Kernel shape: cosine_screen_filter's with the conversion gone.  One persistent workgroup on 7/8 of the CUs, 4 waves, no
// K-split: a wave holds all 64 queries over the whole K as bf16 B operands, owns whole 32-row tiles and streams them through
// its own LDS ring of 4 KiB slots (32 rows x 64 bf16) with buffer_load ... lds, ordered by counted s_waitcnt vmcnt.  Per 16 k
// of a tile: one conflict-free ds_read_b128, NQT MFMAs.  Two things are new:
//   * the ring index is a RUN-TIME scalar (one s_add + s_cselect per slot, one v_add per fragment read), so the depth NBUF is
//     free of the tile's slot count (d = 768: 12 slots per tile; the compile-time ring of cosine_bf16.hip has to divide it:
//     6 slots = 20 KB in flight per wave, where the f32 screen keeps 28).  The kernel has 16 K cycles per tile and wave at
//     the HBM rate and needs ~3 K of matrix pipe: the extra scalar work is free, bytes in flight are what it is short of.
//   * the refill of slot s + P always issues (an empty descriptor past the wave's last tile returns zeros), so every
//     counted wait is the same constant and the tile loop has no tail cases.
// Survivors leave through the per-wave LDS staging ring (oi_lds_dma.h, OI_STAGE_FLUSH_TO_POOL: 64 keys per store instruction;
// a store per survivor sits in the same in-order vmcnt queue as the DMA pieces and makes every counted wait wait for more
// than it needs).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "oi_device.h"
#include "oi_internal.h"
#include "oi_lds_dma.h"
#include "oi_screen_tile.h"

// One ring piece: oi_dma_piece, but for the variant builds that take the DMA out of this kernel.
__device__ __forceinline__ void sc_issue_piece(const oi_u32x4 &srd, uint32_t voff, uint32_t soff, uint32_t lds_dst) {
#if defined(SC_AGG_NO_DMA) && SC_AGG_NO_DMA == 1
    // (variant builds, tools/r05_victim_probe.py: which trait of this kernel disturbs a neighbour wave?  The same bytes loaded
    // into registers nobody reads instead of into LDS; the ring is zeroed at the start, every score is 0: results WRONG.)
    const uint32_t so = __builtin_amdgcn_readfirstlane(soff);
    asm volatile("buffer_load_dwordx4 a[100:103], %0, %1, %2 offen " OI_DMA_NT : : "v"(voff), "s"(srd), "s"(so) : "memory", "a100", "a101", "a102", "a103");
#elif defined(SC_AGG_NO_DMA)
    (void)srd; (void)voff; (void)soff; (void)lds_dst; // (variant builds: no loads at all)
#else
    oi_dma_piece(srd, voff, soff, lds_dst);
#endif
}
#ifdef SC_AGG_NO_MFMA // (variant builds: the stream without the matrix instructions; every score 0, results WRONG)
#define SC_MFMA false
#else
#define SC_MFMA true
#endif

// dynamic LDS: the four rings, then the pool sink's seg_fill and staging ring
constexpr size_t sc_lds(int nbuf) { return oi_ring_lds(nbuf) + OI_POOL_SINK_LDS; }

template <int D, int NQT, int NBUF, bool FILT>
__global__ __launch_bounds__(256, 1) void cosine_copy_screen(
    const uint16_t *__restrict__ rows, uint64_t row_begin, uint64_t row_end,
    const uint16_t *__restrict__ queries, // bf16 [32*NQT][D], zero padded (pf_stage_queries_kernel)
    uint32_t n_queries, uint32_t doc_id_base, uint64_t *pools, uint32_t *seg_cnt, uint32_t seg_cnt_stride,
    const uint32_t *tau_keys, uint64_t pool_stride, uint32_t carry_cap, uint32_t seg_cap, uint32_t *overflow,
    const uint4 *__restrict__ filt, const uint2 *__restrict__ attrs) { // FILT: the doc filter (oi_filter_tile) after the threshold
    using Ring = OiCopyRing<D, NBUF, sc_issue_piece>;
    static_assert(sc_lds(NBUF) <= 160 * 1024, "LDS");

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[]; // [4][NBUF][4 KiB] of ring, then the sink's

    OI_CLAIM_WHOLE_SIMD(); // (MFMA kernel: nothing else may run on this CU -- oi_device.h)
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t li = lane & 31, lh = lane >> 5;

    oi_bf16x8 qreg[NQT][D / 16];
    oi_tile_load_queries<D, NQT>(qreg, queries, li, lh);
    float tauf[NQT]; // thresholds (tau~ - 2 eps) as floats: one v_cmp per score; no query in the slot = NaN
    oi_tile_thresholds<NQT>(tauf, tau_keys, n_queries, li);
#ifdef SC_AGG_NO_DMA
    for (uint32_t i = tid; i < oi_ring_lds(NBUF) / 4; i += 256) reinterpret_cast<uint32_t *>(smem)[i] = 0u;
#endif
    OiPoolSink sink;
    sink.open<NQT>(smem + oi_ring_lds(NBUF), w, pools, carry_cap, seg_cap, pool_stride, doc_id_base, overflow);

    const OiWaveTiles wt = oi_wave_tiles(row_begin, row_end, w);
    if (wt.my_nt) {
        Ring ring;
        ring.begin(wt, rows, smem + w * Ring::BYTES, lane);
        for (uint64_t ti = 0; ti < wt.my_nt; ++ti) {
            oi_f32x16 acc[NQT];
            ring.template tile<NQT, SC_MFMA>(acc, qreg);
            const uint64_t row0 = wt.row0(ti);
            const uint32_t m = oi_tile_mask_ragged(oi_tile_pass_mask<NQT>(acc, tauf), row_end - row0, lh);
            sink.append<NQT, FILT>(m, acc, row0, filt, attrs);
            ring.next(wt, rows, ti);
        }
        sink.flush_rest();
        ring.end();
    }
    sink.close<NQT>(n_queries, seg_cnt, seg_cnt_stride);
}

// ------------------------------------------------------------------ host
// Ring depth.  Measured on one box at 10M x 768, 64 queries (tools/r05_copy_sweep.py, profiles/r05a_copy_sweep.jsonl): 6, 7, 8
// and 9 slots all stream at 0.788-0.790 of the HBM spec on 224 CUs and 0.807-0.811 on 240 -- 20 KB in flight per wave is
// already enough, depth is NOT what holds the kernel (the f32 screen's 0.83 on twice the bytes puts the stream itself at
// 7.0 TB/s and a fixed ~58 us per launch on top: ramp, query preload, tail).  8 it is.  OI_COPY_NBUF (ablation builds): 6 / 7 / 9.
#ifndef OI_COPY_NBUF_DEFAULT
#define OI_COPY_NBUF_DEFAULT 8
#endif

template <int D, int NQT, int NBUF, bool FILT>
static int launch_copy_screen_k(oi_ctx *ctx, const uint16_t *rows, uint64_t row_begin, uint64_t row_end, const uint16_t *q,
                                uint32_t nq, uint32_t doc_id_base, const PoolView &p) {
    constexpr size_t smem = sc_lds(NBUF);
    OI_CHECK(oi_dyn_lds(ctx, reinterpret_cast<const void *>(cosine_copy_screen<D, NQT, NBUF, FILT>), (size_t)(smem)));
    hipLaunchKernelGGL((cosine_copy_screen<D, NQT, NBUF, FILT>), dim3(p.n_segs), dim3(256), smem, ctx->stream, rows, row_begin,
                       row_end, q, nq, doc_id_base, p.keys, p.seg_cnt, p.seg_cnt_stride, p.tau_keys, p.stride,
                       p.carry_cap, p.seg_cap, p.overflow, p.filt, p.attrs);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}
template <int D, int NQT, int NBUF>
static int launch_copy_screen(oi_ctx *ctx, const uint16_t *rows, uint64_t row_begin, uint64_t row_end, const uint16_t *q,
                              uint32_t nq, uint32_t doc_id_base, const PoolView &p) {
    return p.filt ? launch_copy_screen_k<D, NQT, NBUF, true>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p)
                  : launch_copy_screen_k<D, NQT, NBUF, false>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
}

template <int D, int NQT>
static int launch_copy_screen_depth(oi_ctx *ctx, int nbuf, const uint16_t *rows, uint64_t row_begin, uint64_t row_end,
                                    const uint16_t *q, uint32_t nq, uint32_t doc_id_base, const PoolView &p) {
#ifdef OI_ABLATION
    if (nbuf == 6) return launch_copy_screen<D, NQT, 6>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
    if (nbuf == 9) return launch_copy_screen<D, NQT, 9>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
    if (nbuf == 7) return launch_copy_screen<D, NQT, 7>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
#endif
    (void)nbuf;
    return launch_copy_screen<D, NQT, OI_COPY_NBUF_DEFAULT>(ctx, rows, row_begin, row_end, q, nq, doc_id_base, p);
}

// All queries of a batch over rows [row_begin, row_end) of the index's bf16 screening copy.  q_bf16: staged by
// oi_launch_screen_stage (the same block the f32 screen reads).  One pass over the copy per 64 queries.  Pool geometry:
// the f32 screen's (oi_cosine_screen_geometry) -- the two kernels are interchangeable chunk by chunk.
int oi_launch_cosine_screen_copy_chunk(oi_ctx *ctx, const uint16_t *copy_rows, uint64_t row_begin, uint64_t row_end, uint32_t dim,
                                       const uint16_t *q_bf16, uint32_t n_queries, uint32_t doc_id_base, PoolView &pool) {
    OI_REQUIRE(oi_cosine_screen_supported(dim), "cosine screen (copy): dim %u not instantiated (384, 768)", dim);
    oi_cosine_screen_geometry(ctx, row_end > row_begin ? row_end - row_begin : 0, &pool.n_segs, &pool.seg_cap);
    OI_REQUIRE(pool.n_segs <= pool.seg_cnt_stride && pool.carry_cap + (uint64_t)pool.n_segs * pool.seg_cap <= pool.stride,
               "cosine screen (copy): chunk does not fit the candidate pool");
    if (row_end <= row_begin || n_queries == 0) return OI_OK;
    const char *nbuf_s = oi_ablation_env("OI_COPY_NBUF"); // (read per call: a sweep tool changes it between runs of one process)
    const int nbuf = nbuf_s ? atoi(nbuf_s) : OI_COPY_NBUF_DEFAULT;
    ProfScope ps(ctx, "cosine");
    for (uint32_t q0 = 0; q0 < n_queries; q0 += 64) {
        const uint32_t nq_here = std::min(64u, n_queries - q0);
        const PoolView p = pool.for_queries(q0);
        const uint16_t *qptr = q_bf16 + (uint64_t)q0 * dim;
        const bool two = nq_here > 32;
        if (dim == 768) {
            if (two) OI_CHECK((launch_copy_screen_depth<768, 2>(ctx, nbuf, copy_rows, row_begin, row_end, qptr, nq_here, doc_id_base, p)));
            else OI_CHECK((launch_copy_screen_depth<768, 1>(ctx, nbuf, copy_rows, row_begin, row_end, qptr, nq_here, doc_id_base, p)));
        } else {
            if (two) OI_CHECK((launch_copy_screen_depth<384, 2>(ctx, nbuf, copy_rows, row_begin, row_end, qptr, nq_here, doc_id_base, p)));
            else OI_CHECK((launch_copy_screen_depth<384, 1>(ctx, nbuf, copy_rows, row_begin, row_end, qptr, nq_here, doc_id_base, p)));
        }
    }
    return OI_OK;
}
