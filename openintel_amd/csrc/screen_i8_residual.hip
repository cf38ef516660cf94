// screen_i8_residual.hip -- the residual plane of the int8 screening copy and the rescreen that reads it.  DESIGN.md section 4.1a.
//
// The int8 tier (cosine_screen_i8.hip) keeps a few k' survivors per query; before the exact f32 rescoring they are thinned once
// more.  The bf16 rescreen (pf_rescreen_kernel) does that from the bf16 copy: 2 d bytes per survivor and a margin that carries the
// bf16 rounding of the rows AND of the queries.  This file does it from a SECOND int8 plane that stores what the first plane's
// rounding left over: d bytes per survivor, and together the two planes are a 15-bit fixed-point row.
//
// The plane.  Row r, first plane x^ = s_r i_r: rho = x - x^ (exact in f64), t_r = max |f32(rho)| / 127, j_r = rint(f32(rho) / t_r)
// in [-127, 127], e2_r >= |s_r i_r + t_r j_r - x_r| measured in f64 and rounded up, as e_r is.  Layout: the int8 copy's (d bytes per
// row; 256-B aligned, {t_r, e2_r} per row + I8S_PAD_ROWS rows of zeros; the bits of e2_max over the rows that are not long).
//
// The rescreen.  The carried key of a survivor is its lower bound l_r = f32(s~ - m_r), m_r = fma(e_r, |q^|, c_q): the first
// plane's score comes back as s' = f32(l_r + m_r), off s~ by at most 2^-23 (|s~| + m_r).  The second plane adds
//   S2 = 128 sum j h + sum j l   (exact in i32: d 127^2 129 < 2^31),   s~2 = f32(s' + f32(f32(S2) f32(t_r a / 128))),
// and x2 = s_r i_r + t_r j_r has x2 . q^ = (s_r a / 128) S + (t_r a / 128) S2, |x2 . q^ - x . q| <= e2_r |q^| + X |e_q|.  With the
// roundings ("Bound of the residual tier") |s~2 - s^| <= eps2'_q = e2_max |q^| + c_q + 2^-21 ((X + e_max) |q^| + m_max)
// for every row that is not long: the margin select behind this launch is the bf16 screen's final one with 2 eps2'_q in eps2's place
// (staged by the int8 staging launch over the bf16 margin, which has no reader on this tail).
#include <algorithm>

#include "oi_device.h"
#include "oi_internal.h"
#include "oi_screen_i8.h"

// ------------------------------------------------------------------ the plane
// One wave per row, i8s_make_kernel's shape: the first plane's bytes and scale are READ (not made again), so the residual is
// that of the copy the screen streams.
__global__ __launch_bounds__(256) void i8r_make_kernel(const float *__restrict__ rows, uint64_t n, uint32_t dim,
                                                       const uint32_t *__restrict__ long_bitmap, const uint32_t *__restrict__ plane1,
                                                       const float *__restrict__ meta1, uint32_t *__restrict__ out_i8,
                                                       float *__restrict__ meta, uint32_t *__restrict__ e2max_bits) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t n_waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint32_t nv = dim >> 2; // float4 per row (96 / 192)
    float best = 0.f;
    for (uint64_t r = wave; r < n; r += n_waves) {
        const float4 *x = reinterpret_cast<const float4 *>(rows + r * dim);
        const double s = (double)meta1[2 * r];
        double rho[3][4];
        float amax = 0.f;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const uint32_t j = lane + 64u * u;
            const float4 v = j < nv ? x[j] : make_float4(0.f, 0.f, 0.f, 0.f);
            const uint32_t p = j < nv ? plane1[r * nv + j] : 0u;
            const float xs[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int iv = (int)(int8_t)(p >> (8 * c));
                rho[u][c] = (double)xs[c] - s * (double)iv; // exact: both within 32 bits of the row's largest exponent
                amax = fmaxf(amax, fabsf((float)rho[u][c]));
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, OI_WAVE));
        const float t = amax / 127.f;
        double e2 = 0.0;
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const uint32_t j = lane + 64u * u;
            uint32_t packed = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float f = t > 0.f ? rintf((float)rho[u][c] / t) : 0.f;
                f = fminf(127.f, fmaxf(-127.f, f));
                const int jv = (int)f;
                const double e = (double)t * (double)jv - rho[u][c]; // t * jv is exact in f64
                e2 += j < nv ? e * e : 0.0;
                packed |= ((uint32_t)jv & 0xFFu) << (8 * c);
            }
            if (j < nv) out_i8[r * nv + j] = packed;
        }
        e2 = oi_wave_sum(e2);
        const float er = (float)sqrt(e2) * 1.00000095367431640625f; // (1 + 2^-20): rounded up past both roundings
        if (lane == 0) {
            meta[2 * r] = t;
            meta[2 * r + 1] = er;
        }
        const bool is_long = long_bitmap && ((long_bitmap[r >> 5] >> (r & 31)) & 1u);
        if (!is_long) best = fmaxf(best, er);
    }
    if (lane == 0) atomicMax(e2max_bits, __float_as_uint(best));
}

// out: oi_screen_i8_bytes(n, dim) bytes, the int8 copy's layout.  i8_copy: the finished first plane of the same rows.
int oi_launch_make_screen_i8_residual(oi_ctx *ctx, const float *rows, uint64_t n, uint32_t dim, const uint32_t *long_bitmap,
                                      const uint8_t *i8_copy, uint8_t *out) {
    OI_REQUIRE(oi_cosine_screen_supported(dim), "residual screening plane: dim %u not instantiated (384, 768)", dim);
    const size_t mo = oi_screen_i8_meta_offset(n, dim);
    // the padding rows' metadata and e2_max start at zero
    OI_HIP_CHECK(hipMemsetAsync(out + mo, 0, 8 * ((size_t)n + I8S_PAD_ROWS) + 256, ctx->stream));
    if (n == 0) return OI_OK;
    uint64_t blocks = (n + 3) / 4;
    const uint64_t cap = (uint64_t)ctx->num_cus * 8;
    if (blocks > cap) blocks = cap;
    float *meta = reinterpret_cast<float *>(out + mo);
    hipLaunchKernelGGL(i8r_make_kernel, dim3((uint32_t)blocks), dim3(256), 0, ctx->stream, rows, n, dim, long_bitmap,
                       reinterpret_cast<const uint32_t *>(i8_copy), reinterpret_cast<const float *>(i8_copy + mo),
                       reinterpret_cast<uint32_t *>(out), meta, reinterpret_cast<uint32_t *>(meta + 2 * (n + I8S_PAD_ROWS)));
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// ------------------------------------------------------------------ the residual rescreen
// One wave per (query, survivor), four survivors per trip (pf_rescreen_kernel's shape): a lane holds 16 bytes of the query's h
// and l for the whole launch and reads 16 bytes of each survivor's residual row (d / 16 = 48 or 24 lanes of the wave).  A row is
// a third of the bf16 rescreen's bytes per lane and trip, so a trip's two dependent round trips (key -> row) would leave the
// kernel waiting, not streaming: the trips are pipelined two deep -- the next trip's rows are issued, and the keys of the trip
// after it are read, before this trip's rows are awaited (two register sets, A and B, taking turns).
// A lane's partial sum 128 sum j h + sum j l (16 coordinates: < 2^26) goes through ONE wave sum per survivor, in DPP steps.
// The score is written as the row's rank key over its int8 key, in place.
// Single v_fma_f32 / v_mul_f32 / v_add_f32, no packed-f32 forms.
__device__ __forceinline__ float i8r_add_unpacked(float x, float y) {
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(y));
    return r;
}
typedef int i8r_i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ int i8r_dot16(const i8r_i32x4 a, const i8r_i32x4 b) {
    int acc = __builtin_amdgcn_sdot4(a[0], b[0], 0, false);
    acc = __builtin_amdgcn_sdot4(a[1], b[1], acc, false);
    acc = __builtin_amdgcn_sdot4(a[2], b[2], acc, false);
    return __builtin_amdgcn_sdot4(a[3], b[3], acc, false);
}
struct I8rTrip { // four survivors on their way: what their keys said, and the loads issued for them
    uint32_t doc[4];
    float lb[4], er[4], tr[4];
    i8r_i32x4 xv[4];
};
__global__ __launch_bounds__(256) void i8r_rescreen_kernel(const uint8_t *__restrict__ plane, const float *__restrict__ meta2,
                                                           const float *__restrict__ meta1, uint64_t n_rows, uint32_t dim,
                                                           uint32_t doc_id_base, const int8_t *__restrict__ qhi,
                                                           const int8_t *__restrict__ qlo, const float *__restrict__ qf,
                                                           uint32_t qf_stride, uint64_t *pools, const uint32_t *__restrict__ cnt,
                                                           uint64_t stride, uint32_t cap) {
    const uint32_t q = blockIdx.y, lane = threadIdx.x & 63;
    const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
    uint32_t c = cnt[q];
    c = c < cap ? c : cap;
    uint64_t *keys = pools + (uint64_t)q * stride;
    const uint32_t nvec = dim >> 4; // 16 i8 per uint4: 48 / 24 lanes
    const bool on = lane < nvec;
    const uint32_t vl = on ? lane : 0u; // (an idle lane reads lane 0's bytes and its products are dropped)
    const i8r_i32x4 hv = reinterpret_cast<const i8r_i32x4 *>(qhi + (uint64_t)q * dim)[vl];
    const i8r_i32x4 lv = reinterpret_cast<const i8r_i32x4 *>(qlo + (uint64_t)q * dim)[vl];
    const float qa = qf[q] * 0.0078125f, qn = qf[qf_stride + q], cq = qf[2 * qf_stride + q]; // a / 128, |q^|, c_q: the screen's words
    const uint32_t step = n_waves * 4u;
    uint32_t i0 = wave * 4u;
    if (i0 >= c) return;

    uint64_t kn[4]; // the raw keys of the trip that is staged next
    auto read_keys = [&](uint32_t at) {
#pragma unroll
        for (int u = 0; u < 4; ++u) kn[u] = keys[at + u < c ? at + u : c - 1u]; // (past the end: the last survivor again, not written)
    };
    auto stage = [&](I8rTrip &t) { // kn -> t: the rows' loads leave here
        uint64_t row[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            t.doc[u] = oi_rank_key_doc(kn[u]);
            t.lb[u] = oi_rank_key_score(kn[u]);
            const uint64_t r = (uint64_t)(t.doc[u] - doc_id_base);
            row[u] = r < n_rows ? r : 0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) // (each survivor row is read once)
            t.xv[u] = __builtin_nontemporal_load(reinterpret_cast<const i8r_i32x4 *>(plane + row[u] * dim) + vl);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            t.er[u] = meta1[2 * row[u] + 1]; // {s_r, e_r}: the first plane's error norm, as the screen read it
            t.tr[u] = meta2[2 * row[u]];     // {t_r, e2_r}: the second plane's scale
        }
    };
    auto finish = [&](const I8rTrip &t, uint32_t at) { // the trip's scores, over its keys (every lane has read them)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int part = on ? 128 * i8r_dot16(t.xv[u], hv) + i8r_dot16(t.xv[u], lv) : 0;
            const int S2 = __builtin_amdgcn_readlane((int)oi_wave_incl_scan((uint32_t)part), 63);
            // s' = l_r + m_r, m_r the very fma i8s_lower_bound subtracted; then the second plane's product
            const float s1 = i8r_add_unpacked(t.lb[u], oi_fma_unpacked(t.er[u], qn, cq));
            const float s2 = i8r_add_unpacked(s1, oi_mul_unpacked((float)S2, oi_mul_unpacked(t.tr[u], qa)));
            const uint64_t r = (uint64_t)(t.doc[u] - doc_id_base);
            const float sc = r < n_rows ? s2 : 0.f;
            if (lane == 0 && at + u < c) keys[at + u] = oi_rank_key(sc, t.doc[u]);
        }
    };

    I8rTrip A, B;
    read_keys(i0);
    stage(A);
    bool more = i0 + step < c; // kn holds (or is about to hold) the keys of trip i0 + step
    if (more) read_keys(i0 + step);
    for (;;) { // A is staged for i0
        if (more) stage(B);
        const bool more2 = more && i0 + 2 * step < c;
        if (more2) read_keys(i0 + 2 * step);
        finish(A, i0);
        if (!more) break;
        i0 += step; // B is staged for i0
        if (more2) stage(A);
        more = more2 && i0 + 2 * step < c;
        if (more) read_keys(i0 + 2 * step);
        finish(B, i0);
        if (!more2) break;
        i0 += step;
    }
}

int oi_launch_rescreen_residual(oi_ctx *ctx, const uint8_t *residual, const uint8_t *i8_copy, uint64_t n_rows, uint32_t dim,
                                uint32_t doc_id_base, const int8_t *qi8, const float *qf, uint32_t n_queries, const PoolView &pool) {
    if (n_queries == 0) return OI_OK;
    const uint32_t np = (n_queries + 31u) & ~31u;
    const size_t mo = oi_screen_i8_meta_offset(n_rows, dim);
    ProfScope ps(ctx, "rescreen");
    // 64 workgroups per query: about five pipelined trips per wave at 5 000 survivors (10M x 768 beside the BM25 leg: 110, 96, 93
    // and 93 us at 16, 32, 64 and 128 workgroups -- profiles/residual_rescreen_ab.json)
    hipLaunchKernelGGL(i8r_rescreen_kernel, dim3(64, n_queries), dim3(256), 0, ctx->stream, residual,
                       reinterpret_cast<const float *>(residual + mo), reinterpret_cast<const float *>(i8_copy + mo), n_rows, dim,
                       doc_id_base, qi8, qi8 + (uint64_t)np * dim, qf, np, pool.keys, pool.carry_cnt, pool.stride, pool.carry_cap);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}
