// cosine_screen_i8.hip -- the FIRST screening tier of an f32 corpus: an int8 copy of the rows (one byte per coordinate, a
// per-row absmax scale) streamed in front of the bf16 screen, with a PER-ROW error bound.  DESIGN.md section 4.1a.
//
// Builder-defined like the rest of the retrieval path (the reference has none).
//
// Why.  The bf16 copy screen (cosine_screen_copy.hip) streams 2 d bytes per row and batch at the HBM rate: tuning it cannot make
// it faster, reading fewer bytes can.  This tier reads d + 8 bytes per row (the i8 values, the row's f32 scale and its f32
// error norm) and keeps every row that can still reach the list; its survivors (a few k' per query) are then given their bf16
// screen keys from the bf16 copy (pf_rescreen_kernel, 2 d bytes per SURVIVOR) and the bf16 pipeline goes on unchanged: final
// margin select, exact f32 rescoring, gate.
//
// The bound.  Row r: x^ = s_r i_r (i_r in [-127, 127], s_r = max |x_r| / 127), e_r >= |x^ - x_r| measured in f64 when the copy
// is made and rounded up.  Query: q^ = a (h + l / 128), h, l in [-127, 127] (a = max |q| / 127, l the rounded remainder); the
// products are two exact integer dot products, S_h = sum i h and S_l = sum i l (|S| <= d 127^2 < 2^24), and
// S = 128 S_h + S_l (< 2^31) is exact in i32.  The screen score is s~ = f32(S) * f32(s_r a / 128) -- three roundings of 2^-24.
//   x^ . q^ - x . q = (x^ - x) . q^ + x . (q^ - q), so |x^ . q^ - x . q| <= e_r |q^| + X |e_q|   (Cauchy-Schwarz)
// with X = max |x_r| over the rows that are not long (the bf16 screen's X) and |e_q| = |q^ - q|, |q^| measured per query in f64.
// The rescoring (an f32 chain) is off the exact dot by <= d 2^-22 |x| |q|, the three roundings of s~ and the few of the test by
// far less than 2^-18 (|x^| |q^|).  So with
//   m_r = e_r |q^| + c_q,   c_q = X |e_q| + (2^-18 + d 2^-22) (X + e_max) (|q^| + |e_q|)  (+ 1e-27 for flushed denormals)
// the rescored f32 score s^ of every row that is not long lies in [l_r, u_r] = [s~ - m_r, s~ + m_r].  Hence:
//   * keys are LOWER bounds l_r: the k'-th largest l so far, tau_l, is <= the k'-th largest s^ of the whole corpus, so every
//     row of the exact list has u_r >= s^ >= tau_l: the kernel keeps (q, r) when u_r >= T, T <= tau_l (per row: the row's own e_r);
//   * the margin select (select.hip, margin mode with eps2 = m2 = 2 max_r m_r) keeps every key with l >= tau_l - m2, a
//     superset of the keys with u >= tau_l (l_r = u_r - 2 m_r >= u_r - m2), and stores tau_l - m2 as the threshold key;
//   * the kernel adds m2 back: T = tau_stored + m2 - 2^-20 (|tau_stored| + m2) <= tau_l whatever the f32 rounding.
// Every row of the exact list survives every chunk; the survivors' bf16 keys then go through the bf16 screen's final margin select,
// which keeps every row whose bf16 score can reach the list (its threshold over a subset of the rows is only lower): the lists are
// the exact rescoring of a superset of the exact list, the same lists as the bf16 screen's.  Long rows are skipped by the selects and
// rescored whatever happens, as before.  A query without a bound (staging) has m2 = inf: it never gets a threshold, overflows and
// opens the gate like the bf16 screen's.
//
// Kernel shape: cosine_copy_screen's.  One persistent workgroup per CU (every CU when nothing runs beside the chunks, 7/8 of them
// otherwise: search.hip, screen_wgs), 4 waves, a wave holds all 64 queries over the
// whole K as i8 hi / lo B operands (384 VGPRs at d = 768, as the bf16 screen), owns whole 32-row tiles and streams them through its
// own LDS ring of 4 KiB slots (32 rows x 128 i8) with buffer_load ... lds, ordered by counted s_waitcnt vmcnt.  Per 32 k of a tile:
// one ds_read_b128, 2 NQT v_mfma_i32_32x32x32_i8 (the cycles of the bf16 32x32x16: the matrix time per tile is the bf16 screen's,
// the bytes are half).  The tile's 32 {scale, e_r} pairs (256 B) ride one more LDS-DMA load, issued a tile ahead.
// The test of a tile against those pairs runs inside the NEXT tile's matrix span, its survivors leave after that span.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "oi_device.h"
#include "oi_internal.h"
#include "oi_screen_stage.h"
#include "oi_lds_dma.h"
#include "oi_screen_i8.h"

typedef int i8s_i32x4 __attribute__((ext_vector_type(4)));
typedef int i8s_i32x16 __attribute__((ext_vector_type(16)));
typedef float i8s_f32x2 __attribute__((ext_vector_type(2)));
template <int N>
struct i8s_ivec {
    typedef int type __attribute__((ext_vector_type(N)));
};

#define I8S_TILE_ROWS 32
#define I8S_SLOT_BYTES (I8S_TILE_ROWS * 128) // 32 rows x 128 i8 of K
#define I8S_META_BYTES 256                   // 32 rows x {scale, e_r}

// ------------------------------------------------------------------ the copy
size_t oi_screen_i8_meta_offset(uint64_t n, uint32_t dim) { return ((size_t)n * dim + 255) & ~(size_t)255; }
size_t oi_screen_i8_bytes(uint64_t n, uint32_t dim) {
    return oi_screen_i8_meta_offset(n, dim) + 8 * ((size_t)n + I8S_PAD_ROWS) + 256;
}

// One wave per row: absmax scale, i = rint(x / s) clamped to [-127, 127], e_r = |s i - x| in f64, rounded up to f32.  e_max over the
// rows that are not long (long_bitmap, may be null) goes to the word after the metadata.
__global__ __launch_bounds__(256) void i8s_make_kernel(const float *__restrict__ rows, uint64_t n, uint32_t dim,
                                                       const uint32_t *__restrict__ long_bitmap, uint32_t *__restrict__ out_i8,
                                                       float *__restrict__ meta, uint32_t *__restrict__ emax_bits) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint32_t nv = dim >> 2; // float4 per row (96 / 192)
    float best = 0.f;
    for (uint64_t r = wave; r < n; r += n_waves) {
        const float4 *x = reinterpret_cast<const float4 *>(rows + r * dim);
        float4 v[3];
        float amax = 0.f;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const uint32_t j = lane + 64u * u;
            v[u] = j < nv ? x[j] : make_float4(0.f, 0.f, 0.f, 0.f);
            amax = fmaxf(amax, fmaxf(fmaxf(fabsf(v[u].x), fabsf(v[u].y)), fmaxf(fabsf(v[u].z), fabsf(v[u].w))));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, OI_WAVE));
        const float s = amax / 127.f;
        double e2 = 0.0;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const uint32_t j = lane + 64u * u;
            const float xs[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            uint32_t packed = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float t = s > 0.f ? rintf(xs[c] / s) : 0.f;
                t = fminf(127.f, fmaxf(-127.f, t));
                const int iv = (int)t;
                const double e = (double)s * (double)iv - (double)xs[c]; // s * iv is exact in f64
                e2 += j < nv ? e * e : 0.0;
                packed |= ((uint32_t)iv & 0xFFu) << (8 * c);
            }
            if (j < nv) out_i8[r * nv + j] = packed;
        }
        e2 = oi_wave_sum(e2);
        const float er = (float)sqrt(e2) * 1.00000095367431640625f; // (1 + 2^-20): rounded up past both roundings
        if (lane == 0) {
            meta[2 * r] = s;
            meta[2 * r + 1] = er;
        }
        const bool is_long = long_bitmap && ((long_bitmap[r >> 5] >> (r & 31)) & 1u);
        if (!is_long) best = fmaxf(best, er);
    }
    if (lane == 0) atomicMax(emax_bits, __float_as_uint(best));
}

int oi_launch_make_screen_i8(oi_ctx *ctx, const float *rows, uint64_t n, uint32_t dim, const uint32_t *long_bitmap, uint8_t *out) {
    OI_REQUIRE(oi_cosine_screen_supported(dim), "int8 screening copy: dim %u not instantiated (384, 768)", dim);
    const size_t mo = oi_screen_i8_meta_offset(n, dim);
    // the padding rows' metadata (read by the last tile's DMA) and e_max start at zero
    OI_HIP_CHECK(hipMemsetAsync(out + mo, 0, 8 * ((size_t)n + I8S_PAD_ROWS) + 256, ctx->stream));
    if (n == 0) return OI_OK;
    uint64_t blocks = (n + 3) / 4;
    const uint64_t cap = (uint64_t)ctx->num_cus * 8;
    if (blocks > cap) blocks = cap;
    float *meta = reinterpret_cast<float *>(out + mo);
    hipLaunchKernelGGL(i8s_make_kernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, rows, n, dim, long_bitmap,
                       reinterpret_cast<uint32_t *>(out), meta, reinterpret_cast<uint32_t *>(meta + 2 * (n + I8S_PAD_ROWS)));
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// ------------------------------------------------------------------ the queries
// One wave per (padded) query: h, l and the four per-query floats at qf[0 np + q] = a, qf[1 np + q] = |q^| (rounded up),
// qf[2 np + q] = c_q, qf[3 np + q] = m2 = 2 (e_max |q^| + c_q), the tier's select margin.  Padding rows: zeros.  A query the bound
// does not hold for (not finite, norm out of the bf16 screen's range) gets m2 = inf and opens the gate.
#define I8S_NORM_LIMIT 1.0e15f
#define I8S_QNORM_MIN 1.0e-12f
// (one query row: all 64 lanes of the wave call)
__device__ __forceinline__ void i8s_stage_query_row(const float *__restrict__ q, uint32_t row, uint32_t n_queries, uint32_t n_padded, uint32_t dim,
                                                    const uint32_t *__restrict__ max_norm_bits, const uint32_t *__restrict__ emax_bits,
                                                    const uint32_t *__restrict__ e2max_bits, float *__restrict__ eps2r,
                                                    int8_t *__restrict__ qi8, float *__restrict__ qf, uint32_t *gate) {
    const uint32_t lane = threadIdx.x & 63;
    const bool real = row < n_queries;
    float amax = 0.f;
    bool fin = true;
    for (uint32_t k = lane; k < dim; k += 64) {
        const float f = real ? q[(uint64_t)row * dim + k] : 0.f;
        fin = fin && (f - f == 0.f);
        amax = fmaxf(amax, fabsf(f));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, OI_WAVE));
    fin = __builtin_amdgcn_ballot_w64(!fin) == 0ull;
    const float a = fin ? amax / 127.f : 0.f;
    double qn2 = 0.0, en2 = 0.0;
    for (uint32_t k = lane; k < dim; k += 64) {
        const float f = real ? q[(uint64_t)row * dim + k] : 0.f;
        float h = 0.f, l = 0.f;
        if (a > 0.f) {
            const float t = f / a;
            h = fminf(127.f, fmaxf(-127.f, rintf(t)));
            l = fminf(127.f, fmaxf(-127.f, rintf((t - h) * 128.f)));
        }
        const double qh = (double)a * ((double)h + (double)l * 0.0078125); // exact in f64
        qn2 += qh * qh;
        en2 += (qh - (double)f) * (qh - (double)f);
        qi8[(uint64_t)row * dim + k] = (int8_t)(int)h;
        qi8[((uint64_t)n_padded + row) * dim + k] = (int8_t)(int)l;
    }
    qn2 = oi_wave_sum(qn2);
    en2 = oi_wave_sum(en2);
    if (lane == 0) {
        const float up = 1.00000095367431640625f; // 1 + 2^-20
        const float qn = (float)sqrt(qn2) * up, en = (float)sqrt(en2) * up;
        const float X = __uint_as_float(max_norm_bits[0]), em = __uint_as_float(*emax_bits);
        const bool ok = fin && amax > 0.f && qn < I8S_NORM_LIMIT && qn >= I8S_QNORM_MIN && X < I8S_NORM_LIMIT && em < I8S_NORM_LIMIT;
        const float rnd = 3.814697265625e-06f + (float)dim * 2.384185791015625e-07f; // 2^-18 + d 2^-22
        const float cq = 1.001f * (X * en + rnd * (X + em) * (qn + en)) + 1.0e-27f;
        const float m2 = 2.002f * (em * qn + cq);
        qf[row] = ok ? a : 0.f;
        qf[n_padded + row] = ok ? qn : 0.f;
        qf[2 * n_padded + row] = ok ? cq : 0.f;
        qf[3 * n_padded + row] = ok || !real ? m2 : __builtin_inff();
        // the residual plane's uniform select margin 2 eps2'_q (screen_i8_residual.hip): e2_max in e_max's place and
        // 2^-21 ((X + e_max) |q^| + m_max) for the recovery of s~ from the key and the roundings of the second product and the sum.
        // It goes where the bf16 screen's 2 eps would stand (eps2r: [n_queries], the final margin select's array): on that tail
        // the bf16 margin has no reader, and this body runs after the bf16 one
        if (e2max_bits && real) {
            const float rec = 4.76837158203125e-07f * ((X + em) * qn + (em * qn + cq));
            const float m2r = 2.002f * (__uint_as_float(*e2max_bits) * qn + cq + rec);
            eps2r[row] = ok ? m2r : __builtin_inff();
        }
        if (real && !ok) *gate = 1u;
    }
}

// The int8 route stages both tiers' blocks in ONE launch: per query row the int8 body above, then the bf16 screen's
// (oi_screen_stage.h: bf16 copy, eps2, gate) -- the words pf_stage_queries_kernel writes, the row read a second time from cache.
__global__ __launch_bounds__(256) void i8s_stage_both_kernel(const float *__restrict__ q, uint32_t n_queries, uint32_t n_padded, uint32_t dim,
                                                             const uint32_t *__restrict__ max_norm_bits, const uint32_t *__restrict__ emax_bits,
                                                             const uint32_t *__restrict__ e2max_bits, float *__restrict__ eps2r,
                                                             int8_t *__restrict__ qi8, float *__restrict__ qf, uint16_t *__restrict__ q_bf16,
                                                             float *__restrict__ eps2, uint32_t *gate) {
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t row = wave; row < n_padded; row += n_waves) {
        pf_stage_query_row(q, row, n_queries, dim, max_norm_bits, q_bf16, eps2, gate);
        i8s_stage_query_row(q, row, n_queries, n_padded, dim, max_norm_bits, emax_bits, e2max_bits, eps2r, qi8, qf, gate);
    }
}

int oi_launch_screen_stage_i8(oi_ctx *ctx, const float *d_queries, uint32_t n_queries, uint32_t dim, const uint32_t *max_norm_bits,
                              const uint8_t *i8_copy, uint64_t n_rows, int8_t *qi8, float *qf, uint32_t *gate, uint16_t *q_bf16,
                              float *eps2, const uint8_t *residual, float *eps2_residual) {
    const uint32_t n_padded = (n_queries + 31u) & ~31u;
    if (n_padded == 0) return OI_OK;
    // residual: the index's residual plane (screen_i8_residual.hip, the int8 copy's layout) -- its margin to eps2_residual[q]
    const uint32_t *e2max = !(residual && eps2_residual) ? nullptr :
        reinterpret_cast<const uint32_t *>(residual + oi_screen_i8_meta_offset(n_rows, dim)) + 2 * (n_rows + I8S_PAD_ROWS);
    const uint32_t *emax = reinterpret_cast<const uint32_t *>(i8_copy + oi_screen_i8_meta_offset(n_rows, dim)) + 2 * (n_rows + I8S_PAD_ROWS);
    hipLaunchKernelGGL(i8s_stage_both_kernel, dim3((n_padded + 3) / 4), dim3(256), 0, ctx->stream, d_queries, n_queries, n_padded, dim,
                       max_norm_bits, emax, e2max, eps2_residual, qi8, qf, q_bf16, eps2, gate);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// ------------------------------------------------------------------ the screen
// One ring piece: oi_dma_piece, but for the ablation builds that take the DMA out of this kernel.
__device__ __forceinline__ void i8s_issue_piece(const oi_u32x4 &srd, uint32_t voff, uint32_t soff, uint32_t lds_dst) {
#ifdef I8S_NO_DMA
    (void)srd; (void)voff; (void)soff; (void)lds_dst; // (ablation builds: no loads at all; results WRONG)
#else
    oi_dma_piece(srd, voff, soff, lds_dst);
#endif
}
// The tile's metadata: 64 lanes x 4 B = 32 rows x {scale, e_r} into the wave's meta slot.
__device__ __forceinline__ void i8s_issue_meta(const oi_u32x4 &srd, uint32_t voff, uint32_t lds_dst) {
#ifdef I8S_NO_DMA
    (void)srd; (void)voff; (void)lds_dst;
#else
    uint32_t keep;
    const uint32_t d = __builtin_amdgcn_readfirstlane(lds_dst);
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "buffer_load_dword %1, %2, 0 offen " OI_DMA_NT "lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(srd), "s"(d)
        : "memory");
#endif
}

// (the lower bound a pair is keyed by, i8s_screen_score and i8s_lower_bound: oi_screen_i8.h -- the residual rescreen recovers s~ from it)

template <int D, int NQT, int NBUF, bool FILT>
__global__ __launch_bounds__(256, 1) void cosine_i8_screen(
    const uint8_t *__restrict__ rows, const float *__restrict__ meta, uint64_t row_begin, uint64_t row_end,
    const int8_t *__restrict__ qhi, const int8_t *__restrict__ qlo, // [32*NQT][D] each (i8s_stage_both_kernel)
    const float *__restrict__ qf, uint32_t qf_stride, uint32_t n_queries, uint32_t doc_id_base, uint64_t *pools, uint32_t *seg_cnt,
    uint32_t seg_cnt_stride, const uint32_t *tau_keys, uint64_t pool_stride, uint32_t carry_cap, uint32_t seg_cap, uint32_t *overflow,
    const uint4 *__restrict__ filt, const uint2 *__restrict__ attrs) { // FILT: the doc filter (oi_filter_tile) after the threshold
    constexpr int NKC = D / 128;          // ring slots per tile
    constexpr int P = NBUF - 1;           // slots in flight ahead of the one being consumed
    constexpr int KSTEPS = D / 32;        // MFMA groups per tile: four per slot
    constexpr uint32_t RING = NBUF * I8S_SLOT_BYTES;
    static_assert(D % 128 == 0 && P >= 2 && P <= 2 * NKC, "unsupported ring depth for this D");
    constexpr uint32_t QLO_LDS = NQT * KSTEPS * 64 * 16; // the lo parts, fragment-major (one conflict-free ds_read_b128 each)
    static_assert(NQT * KSTEPS * 4 <= 200, "the hi query block must fit the register file");
    static_assert(4 * RING + 4 * 2 * I8S_META_BYTES + 256 + OI_STAGE_LDS + QLO_LDS <= 160 * 1024, "LDS");

    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[];
    unsigned char *ring = smem;                                                          // [4][NBUF][4 KiB]
    unsigned char *meta_lds = smem + 4 * RING;                                           // [4][2][256 B]
    uint32_t *seg_fill = reinterpret_cast<uint32_t *>(smem + 4 * RING + 8 * I8S_META_BYTES); // [64]
    unsigned char *stage_base = smem + 4 * RING + 8 * I8S_META_BYTES + 256;
    unsigned char *qlo_lds = stage_base + OI_STAGE_LDS; // [NQT][KSTEPS][64 lanes][16 B], shared by the four waves

    OI_CLAIM_WHOLE_SIMD(); // (MFMA kernel: nothing else may run on this CU -- oi_device.h)
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t li = lane & 31, lh = lane >> 5;
    uint64_t *stage_keys = reinterpret_cast<uint64_t *>(stage_base) + w * OI_STAGE;
    uint32_t *stage_q = reinterpret_cast<uint32_t *>(stage_base + 4 * OI_STAGE * 8) + w * OI_STAGE;
    uint32_t st_head = 0, st_n = 0;

    // ---- every query over the whole K: B[k = 32 s + 16 lh + 0..15][n = li].  The hi parts in registers for the whole launch (192
    // VGPRs at d = 768); the lo parts in LDS, read per MFMA (with both in registers beside the two accumulator sets the query block
    // spilled into the tile loop)
    i8s_i32x4 qh[NQT][KSTEPS];
#pragma unroll
    for (int t = 0; t < NQT; ++t)
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s)
            qh[t][s] = *reinterpret_cast<const i8s_i32x4 *>(qhi + (uint64_t)(32 * t + li) * D + 32 * s + 16 * lh);
    for (uint32_t c = tid; c < (uint32_t)(NQT * KSTEPS * 64); c += 256) {
        const uint32_t t = c / (KSTEPS * 64), s = (c / 64) % KSTEPS, l = c % 64;
        *reinterpret_cast<i8s_i32x4 *>(qlo_lds + c * 16) =
            *reinterpret_cast<const i8s_i32x4 *>(qlo + (uint64_t)(32 * t + (l & 31)) * D + 32 * s + 16 * (l >> 5));
    }
    // per query of this lane: a, |q^|, c_q and the test's right-hand side T - c_q, T = tau + m2 - 2^-20 (|tau| + m2) <= tau_l
    // (no query in the slot: NaN, nothing passes; a threshold key at or below key(-inf): -inf, everything passes)
    float qa[NQT], qn[NQT], cq[NQT], tc[NQT];
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const uint32_t q = 32u * t + li;
        const bool real = q < n_queries;
        const uint32_t k = real ? tau_keys[q] : 0xFFFFFFFFu;
        const float tau = k <= 0x007FFFFFu ? -__builtin_inff() : oi_key_f32(k);
        qa[t] = real ? qf[q] * 0.0078125f : 0.f; // a / 128: S = 128 S_h + S_l counts q^ / a in units of 1/128 (exact)
        qn[t] = real ? qf[qf_stride + q] : 0.f;
        cq[t] = real ? qf[2 * qf_stride + q] : 0.f;
        const float m2 = real ? qf[3 * qf_stride + q] : 0.f;
        const float T = m2 < __builtin_inff() ? (tau + m2) - (fabsf(tau) + m2) * 9.5367431640625e-07f : -__builtin_inff();
        tc[t] = T - cq[t];
    }
    if (tid < 32 * NQT) seg_fill[tid] = 0;
#ifdef I8S_NO_DMA
    for (uint32_t i = tid; i < (4 * RING + 8 * I8S_META_BYTES) / 4; i += 256) reinterpret_cast<uint32_t *>(smem)[i] = 0u; // (ring, meta)
#endif
    __syncthreads(); // the only barrier before the end: seg_fill is zero before any wave appends

    const uint64_t n_rows = row_end - row_begin;
    const uint64_t n_tiles = (n_rows + I8S_TILE_ROWS - 1) / I8S_TILE_ROWS;
    const uint64_t first = (uint64_t)blockIdx.x * 4 + w, stride = (uint64_t)gridDim.x * 4;
    const uint64_t my_nt = first < n_tiles ? (n_tiles - first + stride - 1) / stride : 0;
    uint64_t *my_seg = pools + carry_cap + (uint64_t)blockIdx.x * seg_cap;

    if (my_nt) {
        // the copy screen's piece geometry with D-byte rows: piece m covers tile rows 8m..8m+7; lane l -> row 8m + (l>>3),
        // physical 16-B column l&7 holding LOGICAL column (l&7) ^ ((row>>1)&7)
        uint32_t voff[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const uint32_t prow = 8 * m + (lane >> 3);
            voff[m] = prow * (uint32_t)D + (((lane & 7) ^ ((prow >> 1) & 7)) << 4);
        }
        const uint32_t ring_w = oi_lds_addr(ring) + w * RING;
        const unsigned char *ring_rd = ring + w * RING;
        const uint32_t meta_w = oi_lds_addr(meta_lds) + w * 2 * I8S_META_BYTES;
        const unsigned char *meta_rd = meta_lds + w * 2 * I8S_META_BYTES;
        // fragment of MFMA group g of a slot: row li, i8 32 g + 16 lh + 0..15 = logical 16-B column 2g + lh
        uint32_t frag_off[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) frag_off[g] = li * 128 + (((2 * g + lh) ^ ((li >> 1) & 7)) << 4);

        auto tile_row0 = [&](uint64_t ti) { return row_begin + (first + ti * stride) * (uint64_t)I8S_TILE_ROWS; };
        auto tile_srd = [&](uint64_t ti) { // past this wave's last tile: an EMPTY descriptor (loads return zeros)
            const uint64_t r0 = tile_row0(ti < my_nt ? ti : 0);
            return oi_make_srd(rows + r0 * D, ti < my_nt ? (row_end - r0) * (uint64_t)D : 0ull);
        };
        auto issue_meta = [&](uint64_t ti) { // rows past the end read as zeros (scale 0); called for ti < my_nt only
            const uint64_t r0 = tile_row0(ti);
            i8s_issue_meta(oi_make_srd(meta + 2 * r0, (row_end - r0) * 8ull), lane * 4u, meta_w + (uint32_t)(ti & 1) * I8S_META_BYTES);
        };
        oi_u32x4 s0 = tile_srd(0), s1 = tile_srd(1), s2 = tile_srd(2);
        __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0): every load hipcc knows about is retired here (oi_lds_dma.h)
        oi_static_for<0, P>([&](auto j_) {
            constexpr int j = decltype(j_)::value;
            constexpr int tj = j / NKC, kj = j % NKC;
#pragma unroll
            for (int m = 0; m < 4; ++m)
                i8s_issue_piece(tj == 0 ? s0 : (tj == 1 ? s1 : s2), voff[m], kj * 128, ring_w + j * I8S_SLOT_BYTES + m * 1024);
        });
        issue_meta(0); // (4 NKC pieces younger than it when tile 0's epilogue waits for it)
        uint32_t rd_off = 0, wr_off = (NBUF - 1) * I8S_SLOT_BYTES;
        // The fragment reads run a k-step ahead of the MFMAs that use them (one wave per SIMD: a waited-for LDS round trip is
        // time nothing else fills).  The lo fragments do not depend on the tile, so their rotation runs across tiles: the last
        // k-step of a tile reads the first one's for the next tile.
        auto lo_frag = [&](int t, int s) {
            return *reinterpret_cast<const i8s_i32x4 *>(qlo_lds + ((t * KSTEPS + s) * 64 + lane) * 16);
        };
        i8s_i32x4 b_cur[NQT];
#ifndef I8S_NO_MFMA
#pragma unroll
        for (int t = 0; t < NQT; ++t) b_cur[t] = lo_frag(t, 0);
#endif

        // (the meta load between the pieces only makes a counted wait wait for one piece more)
        oi_wait_vm<4 * (P - 1)>();
        i8s_i32x4 a_cur = *reinterpret_cast<const i8s_i32x4 *>(ring_rd + frag_off[0]);

        // ---- The tile test runs ONE TILE LATE, inside the next tile's matrix span (the matrix pipe was idle through it, and no
        // piece was issued).  After a tile's last MFMA its S = 128 S_h + S_l goes to registers of its own (S); the accumulators
        // are cleared and the next tile starts; k-steps T0 .. T0 + NSL - 1 of that span each test RPK register rows of S against
        // the row's {scale, e_r}, read from the tile's meta slot a k-step ahead.  The survivor path and the refill of the meta
        // slot follow the span; the last tile of a wave is tested after the loop, in the iteration without a span.  Tile 0's span
        // tests a "tile -1" (S = 0, whatever the meta slot holds) whose mask is dropped.
        // The meta ring: tile i's pairs are in slot i & 1, issued at the end of iteration i - 1 (tile 0: before the loop), read by
        // span i + 1 and by the survivor path after it; then the slot takes tile i + 2's.
        // vmcnt: the first meta read of span i + 1 sits in k-step T0 - 1 = 3 behind the ring's own wait vmcnt(4 (P - 1) - 1).
        // Younger than tile i's meta load by then: the 4 NKC pieces of span i, tile i + 1's meta load (span i + 1 exists, so it
        // was issued), three pieces of span i + 1 and whatever the survivor path stored: at least 4 NKC + 4, and the ring's wait
        // leaves no more than 4 (P - 1) - 1 outstanding.  (The iteration without a span waits for everything.)
        constexpr int NS = 16 * NQT;
        constexpr int RPK = KSTEPS >= 20 ? 1 : 2; // register rows tested per k-step
        constexpr int NSL = 16 / RPK, T0 = 4;     // slices, the first slice's k-step
        static_assert(T0 + NSL <= KSTEPS, "the tile test does not fit the span");
        static_assert(4 * NKC + 4 >= 4 * (P - 1) - 1, "the ring's wait in k-step 3 must retire the previous tile's metadata");
        typename i8s_ivec<NS>::type S;
#pragma unroll
        for (int i = 0; i < NS; ++i) S[i] = 0;
        i8s_i32x16 ah[NQT], al[NQT];
        i8s_f32x2 md_cur[RPK];
#pragma unroll
        for (int u = 0; u < RPK; ++u) md_cur[u] = i8s_f32x2{0.f, 0.f};
        // Register r of query tile t holds D[row (r&3) + 8 (r>>2) + 4 lh][query 32 t + li]
        const uint32_t lh32 = 32u * lh;
        auto meta_row = [&](const unsigned char *mt, int r) { // {scale, e_r} of register row r
            return *reinterpret_cast<const i8s_f32x2 *>(mt + lh32 + ((r & 3) + 8 * (r >> 2)) * 8);
        };
        // keep (q, r) when s~ + e_r |q^| + c_q >= T.  Single v_mul_f32 / v_fma_f32: left to itself hipcc pairs the two query
        // tiles' products into v_pk_*_f32 ... op_sel between the MFMAs, the form DESIGN section 7 found losing products there.
        // A lane that keeps a pair also keeps the pair's s~ and e_r (two selects on the compare's own condition): a tile in
        // which no lane kept more than one pair is appended from these, without reading S or the metadata again.  Only a lane
        // with exactly one bit in the tile's unmasked m reads them, and that bit's test wrote them: they are never cleared.
        float cap_sc = 0.f, cap_er = 0.f;
        auto test_row = [&](int t, int r, const i8s_f32x2 md) -> uint32_t {
            const float sc = oi_mul_unpacked((float)S[16 * t + r], oi_mul_unpacked(md[0], qa[t]));
            const bool pass = sc >= oi_fma_unpacked(-md[1], qn[t], tc[t]);
            cap_sc = pass ? sc : cap_sc;
            cap_er = pass ? md[1] : cap_er;
            return pass ? 1u << (16 * t + r) : 0u;
        };

        for (uint64_t ti = 0;; ++ti) {
            const bool live = ti < my_nt; // (the last iteration has no span: it tests and drains the last tile)
            const unsigned char *mt = meta_rd + (uint32_t)((ti + 1) & 1) * I8S_META_BYTES; // tile ti - 1's
            uint32_t m = 0;
            if (live) {
#pragma unroll
                for (int t = 0; t < NQT; ++t)
#pragma unroll
                    for (int r = 0; r < 16; ++r) { ah[t][r] = 0; al[t][r] = 0; }

                oi_static_for<0, NKC * 4>([&](auto gi_) {
                    constexpr int gi = decltype(gi_)::value;
                    constexpr int kc = gi / 4, g = gi % 4;
                    constexpr int sn = kc + P;
                    constexpr int tn = sn / NKC, kn = sn % NKC;
                    // ---- the reads of k-step gi + 1, into registers no MFMA in flight reads
                    i8s_i32x4 a_nxt;
                    if constexpr (g < 3) {
                        a_nxt = *reinterpret_cast<const i8s_i32x4 *>(ring_rd + rd_off + frag_off[g + 1]);
                    } else {
                        // the next slot (after the tile's last slot: the next tile's first; past the last tile: zeros nobody
                        // uses).  Slots kc + 2 .. kc + P - 1 and three pieces of slot kc + P are younger than its pieces.
                        oi_wait_vm<4 * (P - 1) - 1>();
                        const uint32_t nx_off = rd_off + I8S_SLOT_BYTES == RING ? 0u : rd_off + I8S_SLOT_BYTES;
                        a_nxt = *reinterpret_cast<const i8s_i32x4 *>(ring_rd + nx_off + frag_off[0]);
                    }
                    i8s_f32x2 md_nxt[RPK];
                    if constexpr (gi >= T0 - 1 && gi < T0 - 1 + NSL) {
#pragma unroll
                        for (int u = 0; u < RPK; ++u) md_nxt[u] = meta_row(mt, RPK * (gi - (T0 - 1)) + u);
                    }
#ifndef I8S_NO_MFMA // (ablation builds: the stream without the matrix instructions; every score 0, results WRONG)
                    i8s_i32x4 b_nxt[NQT];
#pragma unroll
                    for (int t = 0; t < NQT; ++t) b_nxt[t] = lo_frag(t, (gi + 1) % KSTEPS);
#endif
                    // (without this the compiler sinks the reads back next to their use and waits for each with lgkmcnt(0);
                    // with it it retires them with counted waits -- tests/test_screen_i8_schedule.py)
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int t = 0; t < NQT; ++t) {
#ifndef I8S_NO_MFMA
                        ah[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a_cur, qh[t][gi], ah[t], 0, 0, 0);
                        al[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a_cur, b_cur[t], al[t], 0, 0, 0);
#else
                        asm volatile("" : : "v"(a_cur));
#endif
                        // ---- the previous tile's test, a slice per k-step, under the first query tile's MFMAs (the fences
                        // keep MFMA pair, test, MFMA pair, then the piece and the next reads: left alone the scheduler queues
                        // every test behind the k-step's last MFMA, where the matrix pipe waits for them)
                        if constexpr (gi >= T0 && gi < T0 + NSL) if (t == 0) {
#pragma unroll
                            for (int u = 0; u < RPK; ++u)
#pragma unroll
                                for (int tt = 0; tt < NQT; ++tt) m |= test_row(tt, RPK * (gi - T0) + u, md_cur[u]);
                            asm volatile("" : "+v"(m), "+v"(cap_sc), "+v"(cap_er)); // (the slice stays in its k-step)
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
#ifndef I8S_NO_MFMA
#pragma unroll
                    for (int t = 0; t < NQT; ++t) b_cur[t] = b_nxt[t];
#endif
                    if constexpr (gi >= T0 - 1 && gi < T0 - 1 + NSL) {
#pragma unroll
                        for (int u = 0; u < RPK; ++u) md_cur[u] = md_nxt[u];
                    }
                    i8s_issue_piece(tn == 0 ? s0 : (tn == 1 ? s1 : s2), voff[g], kn * 128, ring_w + wr_off + g * 1024);
                    if constexpr (g == 3) {
                        wr_off = rd_off;
                        rd_off = rd_off + I8S_SLOT_BYTES == RING ? 0u : rd_off + I8S_SLOT_BYTES;
                    }
                    a_cur = a_nxt;
                });
            } else {
                oi_wait_vm<0>(); // the last tile's metadata (and the zero-filling refills issued past the last tile)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const i8s_f32x2 md = meta_row(mt, r);
#pragma unroll
                    for (int t = 0; t < NQT; ++t) m |= test_row(t, r, md);
                }
            }

            // ---- append tile ti - 1's survivors; the key is the lower bound s~ - e_r |q^| - c_q
            const uint64_t row0 = tile_row0(ti ? ti - 1 : 0);
            if (ti == 0) m = 0u; // "tile -1"
            const uint32_t m_tested = m; // every pair whose test wrote cap_sc / cap_er, before the masks below drop some
            if (row_end - row0 < (uint64_t)I8S_TILE_ROWS) { // the ragged last tile: rows past the end read as zeros
                const uint32_t left = (uint32_t)(row_end - row0);
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if ((uint32_t)((r & 3) + 8 * (r >> 2)) + 4u * lh >= left) m &= ~(0x00010001u << r);
            }
#if defined(I8S_NO_DMA) || defined(I8S_NO_MFMA) || defined(I8S_NO_APPEND)
            // (ablation builds: every score is 0 and every pair would pass, where the product passes < 1 % of them: nothing
            // survives here, and the test above still runs -- the compiler cannot tell.  I8S_NO_APPEND alone: the product's
            // kernel with every survivor dropped, i.e. what the two append paths below cost together; results WRONG)
            if (seg_cap != 0xFFFFFFFFu) m = 0u;
#endif
            if (__builtin_amdgcn_ballot_w64(m != 0u) != 0ull) {
                if constexpr (FILT) m = oi_filter_tile<NQT>(m, filt, attrs, row0, lh, li);
                // ---- No lane tested more than one pair in (three tiles of four with a survivor, under a prediction): every
                // survivor is appended from what its test kept.  The position is the count of lanes with a pair below this one
                // (the ascending-lane order of the path below, where a lane's own pairs follow each other), the key the
                // arithmetic of lower_key on the same s~ and e_r.  At most 64 pairs: they are always staged.
                static_assert(64u <= OI_STAGE - OI_STAGE_FLUSH, "a tile of one pair per lane must fit the staging ring");
                if (__builtin_amdgcn_ballot_w64((m_tested & (m_tested - 1u)) != 0u) == 0ull) {
                    const uint64_t has = __builtin_amdgcn_ballot_w64(m != 0u);
                    if (m != 0u) {
                        const uint32_t bit = (uint32_t)__builtin_ctz(m), r = bit & 15u;
                        const bool t1 = NQT > 1 && bit >= 16u;
                        const uint32_t rit = (r & 3) + 8 * (r >> 2) + 4 * lh;
                        const float low = i8s_lower_bound(cap_sc, cap_er, t1 ? qn[NQT - 1] : qn[0], t1 ? cq[NQT - 1] : cq[0]);
                        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(has >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)has, 0u));
                        const uint32_t idx = (st_head + st_n + below) & (OI_STAGE - 1);
                        stage_keys[idx] = oi_rank_key(low, doc_id_base + ((uint32_t)row0 + rit));
                        stage_q[idx] = (t1 ? 32u : 0u) + li;
                    }
                    st_n += (uint32_t)__builtin_popcountll(has);
                    while (st_n >= OI_STAGE_FLUSH) {
                        OI_STAGE_FLUSH_TO_POOL(OI_STAGE_FLUSH);
                    }
                } else {
                    const uint32_t cnt = (uint32_t)__builtin_popcount(m);
                    const uint32_t incl = oi_wave_incl_scan(cnt);
                    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                    // Only the (t, r) some lane kept are visited: `any` is wave-uniform, so S is indexed by a scalar.  Ascending
                    // (t, r) per lane, as the staging order and the pool contents have always been.
                    const uint32_t any = oi_wave_or(m);
                    auto lower_key = [&](int t, uint32_t r) -> uint64_t { // (survivors only: the metadata read again)
                        const uint32_t rit = (r & 3) + 8 * (r >> 2) + 4 * lh;
                        const i8s_f32x2 md = *reinterpret_cast<const i8s_f32x2 *>(mt + rit * 8);
                        const float sc = i8s_screen_score(S[16 * t + r], md[0], qa[t]);
                        return oi_rank_key(i8s_lower_bound(sc, md[1], qn[t], cq[t]), doc_id_base + ((uint32_t)row0 + rit));
                    };
                    if (total <= OI_STAGE - OI_STAGE_FLUSH) {
                        uint32_t idx = st_head + st_n + incl - cnt;
#pragma unroll
                        for (int t = 0; t < NQT; ++t)
                            for (uint32_t wd = (any >> (16 * t)) & 0xFFFFu; wd; wd &= wd - 1) {
                                const uint32_t r = (uint32_t)__builtin_ctz(wd);
                                if (m & (1u << (16 * t + r))) {
                                    stage_keys[idx & (OI_STAGE - 1)] = lower_key(t, r);
                                    stage_q[idx & (OI_STAGE - 1)] = 32u * t + li;
                                    ++idx;
                                }
                            }
                        st_n += total;
                        while (st_n >= OI_STAGE_FLUSH) {
                            OI_STAGE_FLUSH_TO_POOL(OI_STAGE_FLUSH);
                        }
                    } else {
                        uint32_t pos[NQT];
#pragma unroll
                        for (int t = 0; t < NQT; ++t)
                            pos[t] = atomicAdd(&seg_fill[32u * t + li], (uint32_t)__builtin_popcount((m >> (16 * t)) & 0xFFFFu));
#pragma unroll
                        for (int t = 0; t < NQT; ++t) {
                            uint64_t *dst = my_seg + (uint64_t)(32u * t + li) * pool_stride;
                            for (uint32_t wd = (any >> (16 * t)) & 0xFFFFu; wd; wd &= wd - 1) {
                                const uint32_t r = (uint32_t)__builtin_ctz(wd);
                                if (m & (1u << (16 * t + r))) {
                                    if (pos[t] < seg_cap) dst[pos[t]] = lower_key(t, r);
                                    else *overflow = 1u;
                                    ++pos[t];
                                }
                            }
                        }
                    }
                }
            }
            if (!live) break;
            // ---- this tile's S (the survivor path above was the last reader of the previous tile's)
#pragma unroll
            for (int t = 0; t < NQT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) S[16 * t + r] = ah[t][r] * 128 + al[t][r];
            // the next tile's metadata into the slot the previous tile's just left (its reads have all returned: their values
            // were used)
            if (ti + 1 < my_nt) issue_meta(ti + 1);
            s0 = s1;
            s1 = s2;
            s2 = tile_srd(ti + 3);
        }
        if (st_n) {
            OI_STAGE_FLUSH_TO_POOL(st_n);
        }
        oi_wait_vm<0>(); // the zero-filling refills issued past the last tile have landed before the LDS goes back
    }
    __syncthreads();
    if (tid < 32 * NQT && tid < n_queries) {
        const uint32_t c = seg_fill[tid];
        seg_cnt[(uint64_t)tid * seg_cnt_stride + blockIdx.x] = c < seg_cap ? c : seg_cap;
    }
}

template <int D, int NQT, int NBUF, bool FILT>
static int launch_i8_screen_k(oi_ctx *ctx, const uint8_t *rows, const float *meta, uint64_t row_begin, uint64_t row_end, const int8_t *qhi,
                              const int8_t *qlo, const float *qf, uint32_t qf_stride, uint32_t nq, uint32_t doc_id_base, const PoolView &p) {
    constexpr size_t smem = 4 * NBUF * I8S_SLOT_BYTES + 8 * I8S_META_BYTES + 256 + OI_STAGE_LDS + NQT * (D / 32) * 64 * 16;
    OI_CHECK(oi_dyn_lds(ctx, reinterpret_cast<const void *>(cosine_i8_screen<D, NQT, NBUF, FILT>), (size_t)(smem)));
    hipLaunchKernelGGL((cosine_i8_screen<D, NQT, NBUF, FILT>), dim3(p.n_segs), dim3(256), smem, ctx->stream, rows, meta, row_begin, row_end,
                       qhi, qlo, qf, qf_stride, nq, doc_id_base, p.keys, p.seg_cnt, p.seg_cnt_stride, p.tau_keys, p.stride, p.carry_cap,
                       p.seg_cap, p.overflow, p.filt, p.attrs);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}
template <int D, int NQT, int NBUF>
static int launch_i8_screen(oi_ctx *ctx, const uint8_t *rows, const float *meta, uint64_t row_begin, uint64_t row_end, const int8_t *qhi,
                            const int8_t *qlo, const float *qf, uint32_t qf_stride, uint32_t nq, uint32_t doc_id_base, const PoolView &p) {
    return p.filt ? launch_i8_screen_k<D, NQT, NBUF, true>(ctx, rows, meta, row_begin, row_end, qhi, qlo, qf, qf_stride, nq, doc_id_base, p)
                  : launch_i8_screen_k<D, NQT, NBUF, false>(ctx, rows, meta, row_begin, row_end, qhi, qlo, qf, qf_stride, nq, doc_id_base, p);
}

// All queries of a batch over rows [row_begin, row_end) of the index's int8 copy (n_rows_total rows).  qi8 / qf: staged by
// oi_launch_screen_stage_i8.  Pool geometry: the bf16 screens' (oi_cosine_screen_geometry), at `wgs` workgroups when the plan
// chose a width (0: theirs).
int oi_launch_cosine_screen_i8_chunk(oi_ctx *ctx, const uint8_t *i8_copy, uint64_t n_rows_total, uint64_t row_begin, uint64_t row_end,
                                     uint32_t dim, const int8_t *qi8, const float *qf, uint32_t n_queries, uint32_t doc_id_base,
                                     PoolView &pool, uint32_t wgs) {
    OI_REQUIRE(oi_cosine_screen_supported(dim), "cosine screen (int8): dim %u not instantiated (384, 768)", dim);
    OI_REQUIRE(row_end <= n_rows_total, "cosine screen (int8): rows past the copy");
    const uint64_t chunk_rows = row_end > row_begin ? row_end - row_begin : 0;
    if (wgs) oi_cosine_screen_geometry(ctx, chunk_rows, wgs, &pool.n_segs, &pool.seg_cap);
    else oi_cosine_screen_geometry(ctx, chunk_rows, &pool.n_segs, &pool.seg_cap);
    OI_REQUIRE(pool.n_segs <= pool.seg_cnt_stride && pool.carry_cap + (uint64_t)pool.n_segs * pool.seg_cap <= pool.stride,
               "cosine screen (int8): chunk does not fit the candidate pool");
    if (row_end <= row_begin || n_queries == 0) return OI_OK;
    const float *meta = reinterpret_cast<const float *>(i8_copy + oi_screen_i8_meta_offset(n_rows_total, dim));
    const uint32_t np = (n_queries + 31u) & ~31u;
    ProfScope ps(ctx, "cosine");
    for (uint32_t q0 = 0; q0 < n_queries; q0 += 64) {
        const uint32_t nq_here = std::min(64u, n_queries - q0);
        const PoolView p = pool.for_queries(q0);
        const int8_t *qhi = qi8 + (uint64_t)q0 * dim, *qlo = qi8 + ((uint64_t)np + q0) * dim;
        const float *qfp = qf + q0;
        const bool two = nq_here > 32;
        if (dim == 768) {
            if (two) OI_CHECK((launch_i8_screen<768, 2, 6>(ctx, i8_copy, meta, row_begin, row_end, qhi, qlo, qfp, np, nq_here, doc_id_base, p)));
            else OI_CHECK((launch_i8_screen<768, 1, 6>(ctx, i8_copy, meta, row_begin, row_end, qhi, qlo, qfp, np, nq_here, doc_id_base, p)));
        } else {
            if (two) OI_CHECK((launch_i8_screen<384, 2, 6>(ctx, i8_copy, meta, row_begin, row_end, qhi, qlo, qfp, np, nq_here, doc_id_base, p)));
            else OI_CHECK((launch_i8_screen<384, 1, 6>(ctx, i8_copy, meta, row_begin, row_end, qhi, qlo, qfp, np, nq_here, doc_id_base, p)));
        }
    }
    return OI_OK;
}

// ------------------------------------------------------------------ the sample pass
// What the first speculative threshold is read from (search.hip, Plan::sample_rows): the lower-bound score keys of
// rows [0, m) against every query, dense, keys[q][row] of a [padded queries][key_stride] array -- no thresholds, no pools, no
// survivor path.  One 32-row tile per wave, the row fragments straight from global memory (a lane's KSTEPS 16-byte loads are
// all in flight before the first MFMA); the hi and lo query fragments go to LDS once per workgroup, fragment-major as the screen
// keeps its lo parts (a wave with one tile would read 48 KB of hi parts for 24 KB of rows: with the hi parts in registers per
// wave, as in the screen, the launch took 22 us, most of it the query block's trips from L2).
// Register r of query tile t is row (r&3) + 8 (r>>2) + 4 lh of the tile: four consecutive rows per r >> 2, one 16-byte store.
// Key 0 (below every real key) for a row past m, a long row (they must not move a threshold: the margin selects skip them), a
// padding query and a score that is NaN (the screen's test keeps no such pair either).
template <int D, int NQT>
__global__ __launch_bounds__(256, 1) void i8s_sample_kernel(const uint8_t *__restrict__ rows, const float *__restrict__ meta, uint32_t m_rows,
                                                            const int8_t *__restrict__ qhi, const int8_t *__restrict__ qlo,
                                                            const float *__restrict__ qf, uint32_t qf_stride, uint32_t n_queries,
                                                            const uint32_t *__restrict__ long_bitmap, uint32_t *__restrict__ keys,
                                                            uint32_t key_stride) {
    constexpr int KSTEPS = D / 32;
    constexpr uint32_t PART = NQT * KSTEPS * 64; // 16-byte fragments of the hi parts; as many of the lo parts
    static_assert(D % 32 == 0 && KSTEPS * 4 <= 128, "a tile's row fragments must fit the register file");
    static_assert(2 * PART * 16 <= 160 * 1024, "LDS");
    extern __shared__ __attribute__((aligned(1024))) unsigned char smem[]; // [hi, lo][NQT][KSTEPS][64 lanes][16 B]
    OI_CLAIM_WHOLE_SIMD(); // (MFMA kernel: nothing else may run on this CU -- oi_device.h)
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t li = lane & 31, lh = lane >> 5;
    const uint32_t row0 = (blockIdx.x * 4u + w) * I8S_TILE_ROWS; // (a wave past the last tile only helps to fill the LDS)
    const bool has_tile = row0 < m_rows;

    // A[m = li][k = 32 s + 16 lh + 0..15]; a row past the end reads the last row (its keys are 0)
    const uint32_t arow = has_tile ? (row0 + li < m_rows ? row0 + li : m_rows - 1u) : 0u;
    i8s_i32x4 a[KSTEPS];
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) a[s] = *reinterpret_cast<const i8s_i32x4 *>(rows + (uint64_t)arow * D + 32 * s + 16 * lh);
    // B[k = 32 s + 16 (l >> 5) + 0..15][n = l & 31] of query tile t, hi then lo: a thread's NCP fragments are all loaded before the
    // first goes to LDS (as a loop of load, wait, write the copy was NCP trips to L2 one after the other)
    constexpr int NCP = 2 * PART / 256;
    static_assert(NCP * 256 == 2 * PART, "whole trips of the workgroup");
    i8s_i32x4 qv[NCP];
#pragma unroll
    for (int i = 0; i < NCP; ++i) {
        const uint32_t c = tid + 256u * i, f = c % PART, t = f / (KSTEPS * 64), s = (f / 64) % KSTEPS, l = f % 64;
        qv[i] = *reinterpret_cast<const i8s_i32x4 *>((c < PART ? qhi : qlo) + (uint64_t)(32 * t + (l & 31)) * D + 32 * s + 16 * (l >> 5));
    }
#pragma unroll
    for (int i = 0; i < NCP; ++i) *reinterpret_cast<i8s_i32x4 *>(smem + (tid + 256u * i) * 16) = qv[i];
    // {scale, e_r} of this lane's 16 rows: rows 8 j + 4 lh + 0..3 of the tile are 32 contiguous bytes (the copy's metadata is
    // padded by I8S_PAD_ROWS rows of zeros: a ragged tile reads inside it)
    float4 md[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float4 *mp = reinterpret_cast<const float4 *>(meta + 2 * (uint64_t)((has_tile ? row0 : 0u) + 8 * j + 4 * lh));
        md[j][0] = mp[0];
        md[j][1] = mp[1];
    }
    const uint32_t long_word = long_bitmap && has_tile ? long_bitmap[row0 >> 5] : 0u;
    float qa[NQT], qn[NQT], cq[NQT];
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const uint32_t q = 32u * t + li;
        const bool real = q < n_queries;
        qa[t] = real ? qf[q] * 0.0078125f : 0.f; // a / 128, as the screen
        qn[t] = real ? qf[qf_stride + q] : 0.f;
        cq[t] = real ? qf[2 * qf_stride + q] : 0.f;
    }
    __syncthreads(); // the only barrier: the query fragments are in LDS
    if (!has_tile) return;

    i8s_i32x16 ah[NQT], al[NQT];
#pragma unroll
    for (int t = 0; t < NQT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) { ah[t][r] = 0; al[t][r] = 0; }
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s)
#pragma unroll
        for (int t = 0; t < NQT; ++t) {
            const unsigned char *frag = smem + ((t * KSTEPS + s) * 64 + lane) * 16;
            const i8s_i32x4 bh = *reinterpret_cast<const i8s_i32x4 *>(frag), bl = *reinterpret_cast<const i8s_i32x4 *>(frag + PART * 16);
            ah[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], bh, ah[t], 0, 0, 0);
            al[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], bl, al[t], 0, 0, 0);
        }
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const uint32_t q = 32u * t + li;
        const bool real = q < n_queries;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float scale[4] = {md[j][0].x, md[j][0].z, md[j][1].x, md[j][1].z};
            const float er[4] = {md[j][0].y, md[j][0].w, md[j][1].y, md[j][1].w};
            uint32_t k[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint32_t rit = (uint32_t)(c + 8 * j) + 4u * lh;
                const float sc = i8s_screen_score(ah[t][4 * j + c] * 128 + al[t][4 * j + c], scale[c], qa[t]);
                const bool keep = real && row0 + rit < m_rows && !((long_word >> rit) & 1u) && sc == sc;
                k[c] = keep ? oi_f32_key(i8s_lower_bound(sc, er[c], qn[t], cq[t])) : 0u;
            }
            // (key_stride is a multiple of 32: the tile's columns are there for every query, 16-byte aligned)
            *reinterpret_cast<uint4 *>(keys + (uint64_t)q * key_stride + row0 + 8 * j + 4 * lh) = make_uint4(k[0], k[1], k[2], k[3]);
        }
    }
}

template <int D, int NQT>
static int launch_i8_sample(oi_ctx *ctx, const uint8_t *rows, const float *meta, uint32_t m_rows, const int8_t *qhi, const int8_t *qlo,
                            const float *qf, uint32_t qf_stride, uint32_t nq, const uint32_t *long_bitmap, uint32_t *keys, uint32_t key_stride) {
    constexpr size_t smem = 2 * NQT * (D / 32) * 64 * 16;
    OI_CHECK(oi_dyn_lds(ctx, reinterpret_cast<const void *>(i8s_sample_kernel<D, NQT>), smem));
    const uint32_t tiles = (m_rows + I8S_TILE_ROWS - 1) / I8S_TILE_ROWS;
    hipLaunchKernelGGL((i8s_sample_kernel<D, NQT>), dim3((tiles + 3) / 4), dim3(256), smem, ctx->stream, rows, meta, m_rows, qhi, qlo, qf,
                       qf_stride, nq, long_bitmap, keys, key_stride);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

uint32_t oi_screen_i8_sample_stride(uint32_t m_rows) { return (m_rows + 31u) & ~31u; }

// The lower-bound score keys of rows [0, m_rows) of the index's int8 copy against every query of the batch:
// keys[(padded queries)][oi_screen_i8_sample_stride(m_rows)].  qi8 / qf: staged by oi_launch_screen_stage_i8.
int oi_launch_screen_i8_sample(oi_ctx *ctx, const uint8_t *i8_copy, uint64_t n_rows_total, uint32_t m_rows, uint32_t dim, const int8_t *qi8,
                               const float *qf, uint32_t n_queries, const uint32_t *long_bitmap, uint32_t *keys) {
    OI_REQUIRE(oi_cosine_screen_supported(dim), "cosine screen (int8 sample): dim %u not instantiated (384, 768)", dim);
    OI_REQUIRE(m_rows <= n_rows_total, "cosine screen (int8 sample): rows past the copy");
    if (m_rows == 0 || n_queries == 0) return OI_OK;
    const float *meta = reinterpret_cast<const float *>(i8_copy + oi_screen_i8_meta_offset(n_rows_total, dim));
    const uint32_t np = (n_queries + 31u) & ~31u, ks = oi_screen_i8_sample_stride(m_rows);
    // two spans: "sample" is this launch's own tag; "cosine" goes on counting one span per scoring launch of the cosine leg, this
    // one in the pooled first chunk's place (the schedule checks and the scorer's share of a step read that tag)
    ProfScope pc(ctx, "cosine");
    ProfScope ps(ctx, "sample");
    for (uint32_t q0 = 0; q0 < n_queries; q0 += 64) {
        const uint32_t nq_here = std::min(64u, n_queries - q0);
        const int8_t *qhi = qi8 + (uint64_t)q0 * dim, *qlo = qi8 + ((uint64_t)np + q0) * dim;
        uint32_t *kq = keys + (uint64_t)q0 * ks;
        const bool two = nq_here > 32;
        if (dim == 768) {
            if (two) OI_CHECK((launch_i8_sample<768, 2>(ctx, i8_copy, meta, m_rows, qhi, qlo, qf + q0, np, nq_here, long_bitmap, kq, ks)));
            else OI_CHECK((launch_i8_sample<768, 1>(ctx, i8_copy, meta, m_rows, qhi, qlo, qf + q0, np, nq_here, long_bitmap, kq, ks)));
        } else {
            if (two) OI_CHECK((launch_i8_sample<384, 2>(ctx, i8_copy, meta, m_rows, qhi, qlo, qf + q0, np, nq_here, long_bitmap, kq, ks)));
            else OI_CHECK((launch_i8_sample<384, 1>(ctx, i8_copy, meta, m_rows, qhi, qlo, qf + q0, np, nq_here, long_bitmap, kq, ks)));
        }
    }
    return OI_OK;
}

// ------------------------------------------------------------------ the bf16 rescreen
// One wave per (query, survivor), four survivors per trip: s~ = sum_k bf16(x_k) bf16(q_k) from the bf16 copy (products exact in
// f32, summed in f32 in any order: the bf16 bound allows it), written as the row's bf16 screen key over its int8 key, in place.
// Single v_fma_f32 (oi_fma_unpacked), no packed-f32 forms.
__device__ __forceinline__ float i8s_bf16_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float i8s_bf16_hi(uint32_t w) { return __uint_as_float(w & 0xFFFF0000u); }
__global__ __launch_bounds__(256) void pf_rescreen_kernel(const uint16_t *__restrict__ copy, uint64_t n_rows, uint32_t dim,
                                                          uint32_t doc_id_base, const uint16_t *__restrict__ qb, uint64_t *pools,
                                                          const uint32_t *__restrict__ cnt, uint64_t stride, uint32_t cap) {
    const uint32_t q = blockIdx.y, lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    uint32_t c = cnt[q];
    c = c < cap ? c : cap;
    uint64_t *keys = pools + (uint64_t)q * stride;
    const uint32_t nvec = dim >> 3; // 8 bf16 per uint4
    const uint4 *qv = reinterpret_cast<const uint4 *>(qb + (uint64_t)q * dim);
    for (uint32_t i0 = wave * 4u; i0 < c; i0 += n_waves * 4u) {
        uint32_t doc[4];
        const uint4 *x[4];
        float a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = i0 + u < c ? i0 + u : c - 1u;
            doc[u] = oi_rank_key_doc(keys[i]);
            const uint64_t r = (uint64_t)(doc[u] - doc_id_base);
            x[u] = reinterpret_cast<const uint4 *>(copy + (r < n_rows ? r : 0) * dim);
            a[u] = 0.f;
        }
        for (uint32_t v = lane; v < nvec; v += 64) {
            const uint4 yv = qv[v];
            uint4 xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) xv[u] = oi_load_stream(x[u] + v);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t xw[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w}, yw[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    a[u] = oi_fma_unpacked(i8s_bf16_lo(xw[e]), i8s_bf16_lo(yw[e]), a[u]);
                    a[u] = oi_fma_unpacked(i8s_bf16_hi(xw[e]), i8s_bf16_hi(yw[e]), a[u]);
                }
            }
        }
        float s[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] = oi_wave_sum(a[u]);
        // (every lane has read its keys: the four writes go over them)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint64_t r = (uint64_t)(doc[u] - doc_id_base);
            const float sc = r < n_rows ? s[u] : 0.f;
            if (lane == 0 && i0 + u < c) keys[i0 + u] = oi_rank_key(sc, doc[u]);
        }
    }
}

int oi_launch_rescreen_bf16(oi_ctx *ctx, const uint16_t *copy_rows, uint64_t n_rows, uint32_t dim, uint32_t doc_id_base,
                            const uint16_t *q_bf16, uint32_t n_queries, const PoolView &pool) {
    if (n_queries == 0) return OI_OK;
    ProfScope ps(ctx, "rescreen");
    hipLaunchKernelGGL(pf_rescreen_kernel, dim3(32, n_queries), dim3(256), 0, ctx->stream, copy_rows, n_rows, dim, doc_id_base, q_bf16,
                       pool.keys, pool.carry_cnt, pool.stride, pool.carry_cap);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}
