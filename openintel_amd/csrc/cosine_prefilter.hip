// cosine_prefilter.hip -- the f32 corpus scored at HBM speed: a bf16 screen with a PROVEN error bound, then
// exact f32 scores for the few rows that pass it.
//
// Builder-defined like the rest of the retrieval path (the reference has none).
//
// Why.  The exact f32 MFMA scorer (cosine_ksplit.hip) is bound by the f32 matrix pipes and, under them, by the
// chip's power limit (8.8 ms per 64-query batch at 10M x 768 = 70 % of the f32 MFMA peak; the same corpus
// streams from HBM in 5 ms).  A top-k' list does not need the exact score of every row, only of the rows that
// can reach the list.  So:
//   1. screen: s~ = sum_k bf16(x_k) * bf16(q_k), accumulated in f32 by v_mfma_f32_32x32x16_bf16 (1/16 of the
//      f32 MFMA cycles), the f32 rows converted on the fly between LDS and the matrix pipe (v_cvt_pk_bf16_f32,
//      round to nearest even).  The corpus stays f32 in HBM and is read once: the kernel is a stream.
//   2. bound (round 2: re-derived -- the round-1 constant assumed a unit roundoff of 2^-9 for bf16; it is 2^-8,
//      and a product of two rounded values can be off by 2^-7, so that bound was too small by 2x and a row of
//      the exact list could be screened out).  Nothing is assumed about the rounding now; it is MEASURED.  With
//      x~ = bf16(x), q~ = bf16(q), e_x = x~ - x, e_q = q~ - q (both exact in f32):
//          s~ - s  =  sum_k x~_k q~_k - x_k q_k  =  e_x . q~  +  x . e_q
//      so by Cauchy-Schwarz   |s~ - s| <= |e_x| |q~| + |x| |e_q|   for the exact sums, and the f32 accumulation
//      of the screen (products of bf16 values are exact in f32; <= d additions, each off by at most 2^-23 of
//      the running sum even if the matrix pipe truncates) and of the rescoring add <= d 2^-22 |x~| |q~|.  Hence
//          eps_q = E |q~| + X |e_q| + d 2^-22 (X + E) |q~|  (+ an absolute term for flushed denormals)
//      with X = max_r |x_r| and E = max_r |bf16(x_r) - x_r| taken over the corpus when the rows are set (one
//      pass, the same v_cvt_pk_bf16_f32 the screen uses) and |q~|, |e_q| per query at search time.  For
//      unit Gaussian rows at d = 768 that is E ~ 0.5 * 2^-8, |e_q| ~ 0.45 * 2^-8: eps ~ 0.0042, about half
//      of the worst case 2^-7 -- and when every coordinate sits at a bf16 tie (the adversarial case,
//      tests/test_gpu_prefilter.py) E and |e_q| grow to 2^-8 |x| and the margin grows with them: the
//      bound holds for ANY data, it is only tight for typical data.
//   3. keep: if tau~ is the k'-th largest s~ seen so far, at least k' rows have s >= tau~ - eps, so the final
//      k'-th exact score is >= tau~ - eps, and any row of the final list has s~ >= tau~ - 2 eps.  The select
//      after each corpus chunk therefore keeps EVERY key within 2 eps of the k'-th (select.hip, margin mode) and
//      the screen's threshold is tau~ - 2 eps: a superset of the exact list survives, about 2.4 k' keys for
//      unit vectors at d = 768.
//   4. rescore: exact f32 dot products of the survivors only (one wave per (query, row); ~150K rows per batch
//      instead of 640M), then the ordinary sorted top-k' selection over exact keys.
//   5. if a query's survivors do not fit (4096 keys: rows within 2 eps of the threshold -- duplicates, or norms
//      far above the typical row's) or its norm is not finite, a device flag opens the GATED exact launches that
//      follow in the same stream and overwrite the lists: the exact kernel over all rows with the screen's
//      thresholds (still valid lower bounds of the exact k'-th scores), then one selection; with the gate shut
//      both exit at once.  A corpus whose largest norm is not finite is never screened (decided on the host
//      when the rows are set).
// The lists that come out are those of the exact scorer (up to the f32 rounding of two different summation
// orders, which the parity tolerance already covers); tests/test_gpu_prefilter.py checks both regimes.
//
// Kernel shape: cosine_bf16.hip's solo kernel fed with f32 rows.  One workgroup per CU, 4 waves, no K-split:
// a wave holds all 64 queries over the whole K as bf16 B operands (384 VGPRs at d = 768), owns whole 32-row
// tiles and streams them through its own LDS ring of 4 KiB slots (32 rows x 32 floats) with
// buffer_load ... lds, 7 slots ahead, ordered by counted s_waitcnt vmcnt; waves never meet.  Per 16 k of a tile:
// two conflict-free ds_read_b128, four v_cvt_pk_bf16_f32, two MFMAs.  HBM-bound: 4 d bytes per row and batch.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "oi_device.h"
#include "oi_internal.h"
#include "oi_screen_stage.h"
#include "oi_lds_dma.h"
#include "oi_screen_tile.h"

typedef float pf_f32x4 __attribute__((ext_vector_type(4)));

#define PF_SLOT_K 32                 // floats of K per ring slot row (128 B)
// ring depth of cosine_screen_filter: a compile-time ring index, so the depth divides the tile's slot count
constexpr int pf_nbuf(int d) { return (d / PF_SLOT_K) % 8 == 0 ? 8 : ((d / PF_SLOT_K) % 6 == 0 ? 6 : d / PF_SLOT_K); }
// its dynamic LDS: the four rings, then the pool sink's seg_fill and staging ring
constexpr size_t pf_lds(int d) { return oi_ring_lds(pf_nbuf(d)) + OI_POOL_SINK_LDS; }

__device__ __forceinline__ oi_bf16x8 pf_pack(const pf_f32x4 &a, const pf_f32x4 &b) {
    oi_bf16x8 r;
    r[0] = (__bf16)a[0]; r[1] = (__bf16)a[1]; r[2] = (__bf16)a[2]; r[3] = (__bf16)a[3]; // v_cvt_pk_bf16_f32 (RNE)
    r[4] = (__bf16)b[0]; r[5] = (__bf16)b[1]; r[6] = (__bf16)b[2]; r[7] = (__bf16)b[3];
    return r;
}

// oi_tile_thresholds (oi_screen_tile.h) with oi_key_f32 spelled as the flip it is, k ^ (sign clear ? all bits : the sign bit):
// under the k > 0x007FFFFF test the sign test has an equivalent form (k < 0x00800000 as a signed number), and which of the two the
// compiler emits for the call depends on what else the translation unit holds.
template <int NQT>
__device__ __forceinline__ void pf_tile_thresholds(float (&tauf)[NQT], const uint32_t *tau_keys, uint32_t n_queries, uint32_t li) {
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const uint32_t q = 32u * t + li;
        const uint32_t k = q < n_queries ? tau_keys[q] : 0xFFFFFFFFu;
        const uint32_t flip = (int32_t)k > -1 ? 0xFFFFFFFFu : 0x80000000u;
        tauf[t] = k <= 0x007FFFFFu ? -__builtin_inff() : __uint_as_float(k ^ flip);
    }
}

template <int D, int NQT>
__global__ __launch_bounds__(256, 1) void cosine_screen_filter(
    const float *__restrict__ rows, uint64_t row_begin, uint64_t row_end,
    const uint16_t *__restrict__ queries, // bf16 [32*NQT][D], zero padded
    uint32_t n_queries, uint32_t doc_id_base, uint64_t *pools, uint32_t *seg_cnt, uint32_t seg_cnt_stride,
    const uint32_t *tau_keys, uint64_t pool_stride, uint32_t carry_cap, uint32_t seg_cap, uint32_t *overflow) {
    constexpr int NKC = D / PF_SLOT_K;                    // ring slots per tile
    constexpr int NBUF = pf_nbuf(D);
    constexpr int P = NBUF - 1;                           // slots in flight ahead of the one being consumed
    constexpr uint32_t ROW_BYTES = D * 4;
    static_assert(D % PF_SLOT_K == 0 && NKC % NBUF == 0 && P >= 1 && P < NKC, "unsupported D");

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[]; // [4][NBUF][4 KiB] of ring, then the sink's

    OI_CLAIM_WHOLE_SIMD(); // (MFMA kernel: nothing else may run on this CU -- oi_device.h)
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t li = lane & 31, lh = lane >> 5;

    oi_bf16x8 qreg[NQT][D / 16];
    oi_tile_load_queries<D, NQT>(qreg, queries, li, lh);
    float tauf[NQT];
    pf_tile_thresholds<NQT>(tauf, tau_keys, n_queries, li);
    OiPoolSink sink;
    sink.open<NQT>(smem + oi_ring_lds(NBUF), w, pools, carry_cap, seg_cap, pool_stride, doc_id_base, overflow);

    const OiWaveTiles wt = oi_wave_tiles(row_begin, row_end, w);
    if (wt.my_nt) {
        uint32_t voff[4];
        oi_tile_voff<ROW_BYTES>(voff, lane);
        const uint32_t ring_w = oi_lds_addr(smem) + w * (NBUF * OI_SLOT_BYTES);
        const unsigned char *ring_rd = smem + w * (NBUF * OI_SLOT_BYTES);
        // fragment of k-step g of a slot: row li, floats 16 g + 8 lh + 0..7 = logical 16-B columns 4g + 2lh, + 1
        uint32_t frag_off[2][2];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int h = 0; h < 2; ++h) frag_off[g][h] = li * 128 + (((4 * g + 2 * lh + h) ^ ((li >> 1) & 7)) << 4);

        oi_u32x4 cur = wt.srd<ROW_BYTES>(rows, 0), nxt = wt.srd<ROW_BYTES>(rows, 1);
        oi_tile_retire_visible_loads();
#pragma unroll
        for (int kc = 0; kc < P; ++kc) // prologue: slots 0..P-1 of the first tile
#pragma unroll
            for (int m = 0; m < 4; ++m)
                oi_dma_piece(cur, voff[m], kc * 128, ring_w + (kc % NBUF) * OI_SLOT_BYTES + m * 1024);

        for (uint64_t ti = 0; ti < wt.my_nt; ++ti) {
            oi_f32x16 acc[NQT];
#pragma unroll
            for (int t = 0; t < NQT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

            // Slot s of this tile lives in ring buffer s % NBUF.  Per k-step (kc, g): read the next k-step's
            // floats, NQT MFMAs on the current operand, DMA pieces 2g, 2g+1 of slot kc + P into the buffer
            // slot kc - 1 has vacated, convert the floats read; at g == 1 the next k-step is (kc + 1, 0),
            // behind the counted wait that retires slot kc + 1 (P - 1 younger slots stay in flight).
            oi_wait_vm<4 * (P - 1)>();
            oi_bf16x8 a_cur = pf_pack(*reinterpret_cast<const pf_f32x4 *>(ring_rd + frag_off[0][0]),
                                      *reinterpret_cast<const pf_f32x4 *>(ring_rd + frag_off[0][1]));
            oi_static_for<0, NKC * 2>([&](auto gi_) {
                constexpr int gi = decltype(gi_)::value;
                constexpr int kc = gi / 2, g = gi % 2;
                constexpr int sn = kc + P; // slot refilled during this slot's k-steps
                pf_f32x4 f0, f1;
                if constexpr (g == 0) {
                    f0 = *reinterpret_cast<const pf_f32x4 *>(ring_rd + (kc % NBUF) * OI_SLOT_BYTES + frag_off[1][0]);
                    f1 = *reinterpret_cast<const pf_f32x4 *>(ring_rd + (kc % NBUF) * OI_SLOT_BYTES + frag_off[1][1]);
                }
#pragma unroll
                for (int t = 0; t < NQT; ++t)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a_cur, qreg[t][gi], acc[t], 0, 0, 0);
#pragma unroll
                for (int m = 2 * g; m < 2 * g + 2; ++m) {
                    if constexpr (sn < NKC)
                        oi_dma_piece(cur, voff[m], sn * 128, ring_w + (sn % NBUF) * OI_SLOT_BYTES + m * 1024);
                    else
                        oi_dma_piece(nxt, voff[m], (sn - NKC) * 128, ring_w + (sn % NBUF) * OI_SLOT_BYTES + m * 1024);
                }
                if constexpr (g == 1 && kc + 1 < NKC) {
                    oi_wait_vm<4 * (P - 1)>();
                    f0 = *reinterpret_cast<const pf_f32x4 *>(ring_rd + ((kc + 1) % NBUF) * OI_SLOT_BYTES + frag_off[0][0]);
                    f1 = *reinterpret_cast<const pf_f32x4 *>(ring_rd + ((kc + 1) % NBUF) * OI_SLOT_BYTES + frag_off[0][1]);
                }
                if constexpr (gi + 1 < NKC * 2) a_cur = pf_pack(f0, f1);
            });

            const uint64_t row0 = wt.row0(ti);
            const uint32_t m = oi_tile_mask_ragged(oi_tile_pass_mask<NQT>(acc, tauf), row_end - row0, lh);
            sink.append<NQT, false>(m, acc, row0, nullptr, nullptr);
            cur = nxt;
            nxt = wt.srd<ROW_BYTES>(rows, ti + 2);
        }
        sink.flush_rest();
    }
    sink.close<NQT>(n_queries, seg_cnt, seg_cnt_stride);
}

// ------------------------------------------------------------------ norms, eps, query staging
// Over the rows: X = max_r |x_r| and E = max_r |bf16(x_r) - x_r| (f32, as the bits of non-negative floats:
// atomicMax on the bits orders them; a NaN has the largest bits and poisons the maximum on purpose -- the bound
// does not hold for such a corpus).  The conversion is the screen's own (pf_pack -> v_cvt_pk_bf16_f32), so
// whatever it does to a value (round to nearest even, a flushed denormal) is what E measures.
//   out[0] = bits(X), out[1] = bits(E); (double) out[2..3] = sum_r |x_r|^2, out[4..5] = sum_r |bf16(x_r) - x_r|^2 (the RMS
//   norms the two-class margin is cut at, oi_launch_row_norm_classes)
__global__ __launch_bounds__(256) void pf_row_norm_max_kernel(const float *__restrict__ rows, uint64_t n, uint32_t dim,
                                                              uint32_t *out) {
    double sum_x2 = 0.0, sum_e2 = 0.0;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint32_t nvec = dim >> 2;
    float best = 0.f, best_e = 0.f;
    bool bad = false;
    for (uint64_t r = wave; r < n; r += n_waves) {
        const float4 *x = reinterpret_cast<const float4 *>(rows + r * dim);
        float ss = 0.f, se = 0.f;
        for (uint32_t v = lane; v < nvec; v += 64) {
            const float4 a = x[v];
            ss = fmaf(a.x, a.x, ss); ss = fmaf(a.y, a.y, ss); ss = fmaf(a.z, a.z, ss); ss = fmaf(a.w, a.w, ss);
            const pf_f32x4 f = {a.x, a.y, a.z, a.w};
            const oi_bf16x8 b = pf_pack(f, f);
            const float e0 = (float)b[0] - a.x, e1 = (float)b[1] - a.y, e2 = (float)b[2] - a.z, e3 = (float)b[3] - a.w;
            se = fmaf(e0, e0, se); se = fmaf(e1, e1, se); se = fmaf(e2, e2, se); se = fmaf(e3, e3, se);
        }
        ss = oi_wave_sum(ss);
        se = oi_wave_sum(se);
        const float nm = sqrtf(ss), ne = sqrtf(se);
        bad = bad || !(nm == nm) || !(ne == ne);
        best = nm > best ? nm : best;
        best_e = ne > best_e ? ne : best_e;
        sum_x2 += (double)ss;
        sum_e2 += (double)se;
    }
    if (lane == 0) {
        atomicMax(out, bad ? 0x7FC00000u : __float_as_uint(best));
        atomicMax(out + 1, bad ? 0x7FC00000u : __float_as_uint(best_e));
        atomicAdd(reinterpret_cast<double *>(out + 2), sum_x2);
        atomicAdd(reinterpret_cast<double *>(out + 4), sum_e2);
    }
}

// Two classes of rows (round 4).  The margin above uses the LARGEST |x_r| and |bf16(x_r) - x_r| of the
// corpus, so a handful of long rows widened every query's margin until the survivors no longer fitted and the exact kernel
// took over.  Rows with |x_r| > X0 or error norm > E0 (1.5 x the corpus RMS of each, api.hip) are LONG: listed (at most
// `cap`), marked in a bitmap, left out of the screen's threshold logic by the margin selects (select.hip: skip_bitmap) and
// rescored exactly for every query (pf_rescore_kernel: extra_docs).  The margin is then built from the maxima over the
// other rows, which this kernel takes in the same pass.
//   cls[0] = bits(max |x_r|) and cls[1] = bits(max error norm) over the rows that are NOT long, cls[2] = long rows found
__global__ __launch_bounds__(256) void pf_row_norm_class_kernel(const float *__restrict__ rows, uint64_t n, uint32_t dim, float X0,
                                                                float E0, uint32_t *cls, uint32_t *bitmap, uint32_t *list,
                                                                uint32_t cap) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint32_t nvec = dim >> 2;
    float best = 0.f, best_e = 0.f;
    for (uint64_t r = wave; r < n; r += n_waves) {
        const float4 *x = reinterpret_cast<const float4 *>(rows + r * dim);
        float ss = 0.f, se = 0.f;
        for (uint32_t v = lane; v < nvec; v += 64) {
            const float4 a = x[v];
            ss = fmaf(a.x, a.x, ss); ss = fmaf(a.y, a.y, ss); ss = fmaf(a.z, a.z, ss); ss = fmaf(a.w, a.w, ss);
            const pf_f32x4 f = {a.x, a.y, a.z, a.w};
            const oi_bf16x8 b = pf_pack(f, f);
            const float e0 = (float)b[0] - a.x, e1 = (float)b[1] - a.y, e2 = (float)b[2] - a.z, e3 = (float)b[3] - a.w;
            se = fmaf(e0, e0, se); se = fmaf(e1, e1, se); se = fmaf(e2, e2, se); se = fmaf(e3, e3, se);
        }
        ss = oi_wave_sum(ss);
        se = oi_wave_sum(se);
        const float nm = sqrtf(ss), ne = sqrtf(se);
        if (nm > X0 || ne > E0) { // (the same sums in the same order as the pass that set X0 and E0: the same values)
            if (lane == 0) {
                const uint32_t pos = atomicAdd(cls + 2, 1u);
                if (pos < cap) list[pos] = (uint32_t)r;
                atomicOr(bitmap + (r >> 5), 1u << (r & 31));
            }
        } else {
            best = nm > best ? nm : best;
            best_e = ne > best_e ? ne : best_e;
        }
    }
    if (lane == 0) {
        atomicMax(cls, __float_as_uint(best));
        atomicMax(cls + 1, __float_as_uint(best_e));
    }
}

// (the margin of one query, pf_eps, and the per-query staging body: oi_screen_stage.h)
// Per query: bf16 copy (RNE, zero padded to n_padded rows) and the screen's margin 2 eps; a norm that is not
// finite, too large for the bf16 products to stay finite, or too small for its rounding errors to be measured in
// f32 opens the exact pipeline instead (gate).
//   state words: eps2[q] (float) at state + q; *gate at gate.
__global__ __launch_bounds__(256) void pf_stage_queries_kernel(const float *__restrict__ q, uint32_t n_queries,
                                                               uint32_t n_padded, uint32_t dim,
                                                               const uint32_t *__restrict__ max_norm_bits,
                                                               uint16_t *__restrict__ out, float *__restrict__ eps2,
                                                               uint32_t *gate) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t row = wave; row < n_padded; row += n_waves) {
        pf_stage_query_row(q, row, n_queries, dim, max_norm_bits, out, eps2, gate);
    }
}

// Diagnostics (oi_screen_probe): the screen's raw scores.  Same operands and the same instruction as the screen
// (bf16 rows by pf_pack, the staged bf16 queries, v_mfma_f32_32x32x16_bf16 accumulating 16 k at a time in K
// order), one wave per 32 rows x 32 queries; out[q * n_rows + r].
__global__ __launch_bounds__(64) void pf_probe_kernel(const float *__restrict__ rows, uint64_t row_begin, uint32_t n_rows,
                                                      uint32_t dim, const uint16_t *__restrict__ queries,
                                                      uint32_t n_queries, float *__restrict__ out) {
    const uint32_t lane = threadIdx.x, li = lane & 31, lh = lane >> 5;
    const uint32_t r0 = blockIdx.x * 32, q0 = blockIdx.y * 32;
    oi_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const uint32_t row = r0 + li < n_rows ? r0 + li : n_rows - 1; // (rows past the end are not written)
    const float *x = rows + (row_begin + row) * (uint64_t)dim;
    const uint16_t *qq = queries + (uint64_t)(q0 + li) * dim;     // the staged block is zero padded to 32 rows
    for (uint32_t k = 0; k < dim; k += 16) {
        const oi_bf16x8 a = pf_pack(*reinterpret_cast<const pf_f32x4 *>(x + k + 8 * lh),
                                    *reinterpret_cast<const pf_f32x4 *>(x + k + 8 * lh + 4));
        const oi_bf16x8 b = *reinterpret_cast<const oi_bf16x8 *>(qq + k + 8 * lh);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const uint32_t rr = r0 + (r & 3) + 8 * (r >> 2) + 4 * lh, qx = q0 + li;
        if (rr < n_rows && qx < n_queries) out[(uint64_t)qx * n_rows + rr] = acc[r];
    }
}

// The bf16 screening copy (OI_COSINE_SCREEN_COPY, opt-in): every row converted ONCE, with the conversion the screen
// uses on the fly (pf_pack), so E -- and therefore the bound -- is the same; the screen then reads 2 d bytes per row.
__global__ __launch_bounds__(256) void pf_make_copy_kernel(const float *__restrict__ rows, uint64_t n_vec8, uint4 *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_vec8; i += (uint64_t)gridDim.x * blockDim.x) {
        const pf_f32x4 a = *reinterpret_cast<const pf_f32x4 *>(rows + i * 8), b = *reinterpret_cast<const pf_f32x4 *>(rows + i * 8 + 4);
        const oi_bf16x8 v = pf_pack(a, b);
        out[i] = *reinterpret_cast<const uint4 *>(&v);
    }
}
int oi_launch_make_screen_copy(oi_ctx *ctx, const float *rows, uint64_t n, uint32_t dim, uint16_t *out) {
    const uint64_t n_vec8 = n * dim / 8; // dim is a multiple of 16 on this path
    if (n_vec8 == 0) return OI_OK;
    const uint64_t blocks = std::min<uint64_t>((n_vec8 + 255) / 256, (uint64_t)ctx->num_cus * 16);
    hipLaunchKernelGGL(pf_make_copy_kernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, rows, n_vec8, reinterpret_cast<uint4 *>(out));
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// ------------------------------------------------------------------ exact rescoring of the survivors
// One wave per (query, survivor): s = sum_k x_k q_k in f32 (fma chain per lane, butterfly sum), written as an
// exact rank key at the same slot of the output pool's carry region.
__global__ __launch_bounds__(256) void pf_rescore_kernel(const float *__restrict__ rows, uint32_t dim, uint32_t doc_id_base,
                                                         uint64_t n_rows, const float *__restrict__ queries,
                                                         const uint64_t *__restrict__ in_pools, const uint32_t *__restrict__ in_cnt,
                                                         uint64_t in_stride, uint32_t cap, uint64_t *out_pools,
                                                         uint32_t *out_cnt, uint64_t out_stride,
                                                         const uint32_t *__restrict__ extra_docs, uint32_t n_extra,
                                                         const uint32_t *__restrict__ spec_max, const uint32_t *__restrict__ tau_final,
                                                         uint32_t *gate, uint32_t *fail_host,
                                                         const uint4 *__restrict__ filt, const uint2 *__restrict__ attrs) {
    // spec_max != null: the check of the speculative thresholds rides along (spec_max[q] > tau_final[q] voids the batch's screen; no launch of its own): the
    // gated exact pipeline is enqueued after this kernel
    if (spec_max && blockIdx.x == 0 && threadIdx.x == 0 && spec_max[blockIdx.y] > tau_final[blockIdx.y]) {
        gate[0] = 1u;
        if (fail_host) *fail_host = 1u;
    }
    // extra_docs: the index's LONG rows (local row numbers, pf_row_norm_class_kernel) -- scored for every query after its
    // survivors, whatever the screen made of them
    const uint32_t q = blockIdx.y, lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    uint32_t c0 = in_cnt[q];
    c0 = c0 < cap ? c0 : cap;
    const uint32_t c = c0 + n_extra;
    const uint32_t nvec = dim >> 2;
    // filt != null (a filtered search): a long row that fails query q's filter is left out, the ones that pass go to
    // c0 + (their rank among the passing long rows) -- the survivors passed the filter in the screen already
    const uint4 fq = filt ? filt[q] : make_uint4(0u, 0u, 0u, 0u);
    auto long_passing = [&](uint32_t j) { // long rows [0, j) that pass (every lane of the wave calls it, j uniform)
        uint32_t cnt = 0;
        for (uint32_t k0 = 0; k0 < j; k0 += 64) {
            const uint32_t k = k0 + lane;
            cnt += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(k < j && oi_doc_passes(fq, attrs[extra_docs[k]])));
        }
        return cnt;
    };
    const float4 *qv = reinterpret_cast<const float4 *>(queries + (uint64_t)q * dim);
    // four survivors per wave and trip: their rows' loads are all in flight before the first reduction (one row at a
    // time this kernel was a chain of HBM round trips: 68 us for 2450 survivors x 64 queries at d = 768)
    for (uint32_t i0 = wave * 4u; i0 < c; i0 += n_waves * 4u) {
        uint32_t doc[4];
        const float4 *x[4];
        float a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = i0 + u < c ? i0 + u : c - 1u; // (past the end: the last survivor again, not written)
            doc[u] = i < c0 ? oi_rank_key_doc(in_pools[(uint64_t)q * in_stride + i]) : doc_id_base + extra_docs[i - c0];
            const uint64_t r = (uint64_t)(doc[u] - doc_id_base);
            x[u] = reinterpret_cast<const float4 *>(rows + (r < n_rows ? r : 0) * dim);
            a[u] = 0.f;
        }
        for (uint32_t v = lane; v < nvec; v += 64) {
            const float4 yv = qv[v];
            float4 xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) xv[u] = oi_load_stream(x[u] + v); // (each survivor row is read once)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                // (one v_fma_f32 each, NOT the packed form the vectoriser makes of two chains: oi_device.h, oi_fma_unpacked)
                a[u] = oi_fma_unpacked(xv[u].x, yv.x, a[u]); a[u] = oi_fma_unpacked(xv[u].y, yv.y, a[u]);
                a[u] = oi_fma_unpacked(xv[u].z, yv.z, a[u]); a[u] = oi_fma_unpacked(xv[u].w, yv.w, a[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint64_t r = (uint64_t)(doc[u] - doc_id_base);
            float s = oi_wave_sum(a[u]);
            if (!(r < n_rows)) s = 0.f; // (a key outside the shard: cannot happen; scored 0 as before)
            if (filt && i0 + u >= c0 && i0 + u < c) { // (wave-uniform)
                const uint32_t j = i0 + u - c0, slot = c0 + long_passing(j);
                if (lane == 0 && oi_doc_passes(fq, attrs[extra_docs[j]])) out_pools[(uint64_t)q * out_stride + slot] = oi_rank_key(s, doc[u]);
                continue;
            }
            if (lane == 0 && i0 + u < c) out_pools[(uint64_t)q * out_stride + i0 + u] = oi_rank_key(s, doc[u]);
        }
    }
    if (filt) {
        if (blockIdx.x == 0 && threadIdx.x < 64) {
            const uint32_t cf = c0 + long_passing(n_extra);
            if (threadIdx.x == 0) out_cnt[q] = cf;
        }
    } else if (blockIdx.x == 0 && threadIdx.x == 0) out_cnt[q] = c;
}

// (The speculative thresholds between the chunks are made in the margin selects -- select.hip; oi_select_rank.h: sel_spec_words,
// where the prediction is derived -- and checked by pf_rescore_kernel, first thing: above.)

// ------------------------------------------------------------------ host
bool oi_cosine_screen_supported(uint32_t dim) { return dim == 384 || dim == 768; }

// Pool geometry of one chunk: one segment per workgroup; its four waves take 4 tiles per round.
void oi_cosine_screen_geometry(const oi_ctx *ctx, uint64_t n_rows, uint32_t *n_segs, uint32_t *seg_cap) {
    const uint64_t n_tiles = (n_rows + OI_TILE_ROWS - 1) / OI_TILE_ROWS;
    const uint64_t quads = (n_tiles + 3) / 4;
    // The persistent screen takes 7/8 of the CUs, one workgroup each.  It is HBM-bound: 208..224 of 256 CUs stream the corpus as
    // fast as 256 (4.82-4.92 vs 4.97 ms per 10M-row batch), and the CUs left free run the small kernels of whatever else is in
    // flight -- the BM25 leg on the side stream, the selects and the rescoring of another batch scored through a view of the
    // same shard (oi_index_view): 0.817 -> 0.713 ms per batch at 1.25M rows with two batches in flight (tools/dual_stream_probe.py;
    // 192: 0.69-0.72, 160: 0.75, and from 176 down the single-stream time grows).  OI_SCREEN_CUS: A/B switch.
    const char *cus_s = oi_ablation_env("OI_SCREEN_CUS"); // (read per call: sweep tools change it between runs of one process)
    const uint64_t cus = cus_s ? (uint64_t)std::max(1, atoi(cus_s)) : std::max<uint64_t>(1, (uint64_t)ctx->num_cus * 7 / 8);
    static const bool small_full = oi_ablation_env("OI_SCREEN_SMALL_FULL") != nullptr; // A/B: a chunk of <= one quad per CU takes every CU
    const uint64_t grid = small_full && quads <= (uint64_t)ctx->num_cus ? (quads ? quads : 1) : (quads < cus ? (quads ? quads : 1) : cus);
    *n_segs = (uint32_t)grid;
    *seg_cap = (uint32_t)((quads + grid - 1) / grid) * 4 * OI_TILE_ROWS;
}
// The same geometry at a width the caller chooses.  The int8 screen is not HBM-bound at 7/8 of the CUs, so its
// chunks take every CU when nothing else wants one while they run (search.hip: plan_search, screen_wgs).  Everything sized by the
// width is sized for num_cus segments: the state words, the segment counts' stride and the pool's rounding slack (search.hip).
void oi_cosine_screen_geometry(const oi_ctx *ctx, uint64_t n_rows, uint32_t wgs, uint32_t *n_segs, uint32_t *seg_cap) {
    const uint64_t n_tiles = (n_rows + OI_TILE_ROWS - 1) / OI_TILE_ROWS;
    const uint64_t quads = (n_tiles + 3) / 4;
    const uint64_t cus = std::min<uint64_t>(std::max<uint64_t>(1, wgs), std::max<uint64_t>(1, (uint64_t)ctx->num_cus));
    const uint64_t grid = quads < cus ? (quads ? quads : 1) : cus;
    *n_segs = (uint32_t)grid;
    *seg_cap = (uint32_t)((quads + grid - 1) / grid) * 4 * OI_TILE_ROWS;
}

int oi_launch_row_norm_classes(oi_ctx *ctx, const float *rows, uint64_t n, uint32_t dim, float X0, float E0, uint32_t *cls,
                               uint32_t *bitmap, uint32_t *list, uint32_t cap) {
    OI_HIP_CHECK(hipMemsetAsync(cls, 0, 16, ctx->stream));
    OI_HIP_CHECK(hipMemsetAsync(bitmap, 0, ((n + 31) / 32) * 4, ctx->stream));
    uint64_t blocks = (n + 3) / 4;
    const uint64_t capb = (uint64_t)ctx->num_cus * 8;
    if (blocks > capb) blocks = capb;
    hipLaunchKernelGGL(pf_row_norm_class_kernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, rows, n, dim, X0, E0, cls, bitmap,
                       list, cap);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

int oi_launch_row_norm_max(oi_ctx *ctx, const float *rows, uint64_t n, uint32_t dim, uint32_t *max_bits) {
    OI_HIP_CHECK(hipMemsetAsync(max_bits, 0, 24, ctx->stream)); // [0] = X, [1] = E, [2..5] = the two sums of squares (double)
    if (n == 0) return OI_OK;
    uint64_t blocks = (n + 3) / 4;
    const uint64_t cap = (uint64_t)ctx->num_cus * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(pf_row_norm_max_kernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, rows, n, dim, max_bits);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// bf16 queries (padded to a multiple of 32 rows) + per-query margins + gate, once per search
int oi_launch_screen_stage(oi_ctx *ctx, const float *d_queries, uint32_t n_queries, uint32_t dim,
                           const uint32_t *max_norm_bits, uint16_t *q_bf16, float *eps2, uint32_t *gate) {
    const uint32_t n_padded = (n_queries + 31u) & ~31u;
    hipLaunchKernelGGL(pf_stage_queries_kernel, dim3((n_padded + 3) / 4), dim3(256), 0, ctx->stream, d_queries, n_queries,
                       n_padded, dim, max_norm_bits, q_bf16, eps2, gate);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

template <int D, int NQT>
static int launch_screen(oi_ctx *ctx, const float *rows, uint64_t row_begin, uint64_t row_end, const uint16_t *q,
                         uint32_t nq, uint32_t doc_id_base, const PoolView &p) {
    constexpr size_t smem = pf_lds(D);
    OI_CHECK(oi_dyn_lds(ctx, reinterpret_cast<const void *>(cosine_screen_filter<D, NQT>), (size_t)(smem)));
    hipLaunchKernelGGL((cosine_screen_filter<D, NQT>), dim3(p.n_segs), dim3(256), smem, ctx->stream, rows, row_begin,
                       row_end, q, nq, doc_id_base, p.keys, p.seg_cnt, p.seg_cnt_stride, p.tau_keys, p.stride,
                       p.carry_cap, p.seg_cap, p.overflow);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// All queries of a batch over rows [row_begin, row_end): the bf16 screen.  q_bf16: staged by
// oi_launch_screen_stage.  One corpus pass per 64 queries.
int oi_launch_cosine_screen_chunk(oi_ctx *ctx, const float *rows, uint64_t row_begin, uint64_t row_end, uint32_t dim,
                                  const uint16_t *q_bf16, uint32_t n_queries, uint32_t doc_id_base, PoolView &pool) {
    OI_REQUIRE(oi_cosine_screen_supported(dim), "cosine screen: dim %u not instantiated (384, 768)", dim);
    oi_cosine_screen_geometry(ctx, row_end > row_begin ? row_end - row_begin : 0, &pool.n_segs, &pool.seg_cap);
    OI_REQUIRE(pool.n_segs <= pool.seg_cnt_stride && pool.carry_cap + (uint64_t)pool.n_segs * pool.seg_cap <= pool.stride,
               "cosine screen: chunk does not fit the candidate pool");
    OI_REQUIRE(!pool.filt, "cosine screen: a filtered search does not take the f32-stream screen (search.hip routes it)");
    if (row_end <= row_begin || n_queries == 0) return OI_OK;
    ProfScope ps(ctx, "cosine");
    for (uint32_t q0 = 0; q0 < n_queries; q0 += 64) {
        const uint32_t nq_here = std::min(64u, n_queries - q0);
        PoolView p = pool.for_queries(q0); // (no filter here: required above)
        static const bool tau_max = oi_ablation_env("OI_SCREEN_TAU_MAX") != nullptr; // A/B (WRONG results): chunks of >= 1M rows pass nothing
        if (tau_max && row_end - row_begin >= (1u << 20)) {
            DevBuf &tb = ctx->buf("abl_tau_max");
            if (!tb.p) { OI_CHECK(tb.ensure(4096 * 4)); OI_HIP_CHECK(hipMemsetAsync(tb.p, 0xFF, 4096 * 4, ctx->stream)); }
            p.tau_keys = tb.as<uint32_t>();
        }
        const uint16_t *qptr = q_bf16 + (uint64_t)q0 * dim;
        const bool two = nq_here > 32;
        if (dim == 768) {
            if (two) OI_CHECK((launch_screen<768, 2>(ctx, rows, row_begin, row_end, qptr, nq_here, doc_id_base, p)));
            else OI_CHECK((launch_screen<768, 1>(ctx, rows, row_begin, row_end, qptr, nq_here, doc_id_base, p)));
        } else {
            if (two) OI_CHECK((launch_screen<384, 2>(ctx, rows, row_begin, row_end, qptr, nq_here, doc_id_base, p)));
            else OI_CHECK((launch_screen<384, 1>(ctx, rows, row_begin, row_end, qptr, nq_here, doc_id_base, p)));
        }
    }
    return OI_OK;
}

// Exact scores of the screen's survivors: in.carry region (in.carry_cnt keys per query) -> out.carry region.
int oi_launch_rescore(oi_ctx *ctx, const float *rows, uint64_t n_rows, uint32_t dim, uint32_t doc_id_base,
                      const float *d_queries, uint32_t n_queries, const PoolView &in, const PoolView &out,
                      const uint32_t *extra_docs, uint32_t n_extra, const uint32_t *spec_max, const uint32_t *tau_final,
                      uint32_t *gate, uint32_t *fail_host, uint32_t wgs_per_query) {
    if (n_queries == 0) return OI_OK;
    OI_REQUIRE(out.carry_cap >= in.carry_cap + n_extra, "rescore: output pool too small");
    ProfScope ps(ctx, "rescore");
    hipLaunchKernelGGL(pf_rescore_kernel, dim3(wgs_per_query ? wgs_per_query : 64u, n_queries), dim3(256), 0, ctx->stream, rows, dim, doc_id_base, n_rows,
                       d_queries, in.keys, in.carry_cnt, in.stride, in.carry_cap, out.keys, out.carry_cnt, out.stride, extra_docs,
                       n_extra, spec_max, tau_final, gate, fail_host, out.filt, out.attrs);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// Diagnostics: raw screen scores s~ of rows [row_begin, row_begin + n_rows) for every query of the staged block.
int oi_launch_screen_probe(oi_ctx *ctx, const float *rows, uint64_t row_begin, uint32_t n_rows, uint32_t dim,
                           const uint16_t *q_bf16, uint32_t n_queries, float *d_out) {
    if (n_rows == 0 || n_queries == 0) return OI_OK;
    OI_REQUIRE(dim % 16 == 0, "screen probe: dim %u is not a multiple of 16", dim);
    hipLaunchKernelGGL(pf_probe_kernel, dim3((n_rows + 31) / 32, (n_queries + 31) / 32), dim3(64), 0, ctx->stream, rows,
                       row_begin, n_rows, dim, q_bf16, n_queries, d_out);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}
