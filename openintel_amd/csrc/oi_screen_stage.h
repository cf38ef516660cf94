// oi_screen_stage.h -- what the screens stage per query, one wave per (padded) query row.  The bf16 screen's block is written by
// pf_stage_queries_kernel (cosine_prefilter.hip) or, on the int8 route, together with the int8 tier's blocks by one launch of
// i8s_stage_both_kernel (cosine_screen_i8.hip): the same device body, the same words.
#pragma once
#include "oi_device.h"

// The margin of one query (see the header of cosine_prefilter.hip): |s~ - s^| <= eps for every row of the corpus, s^ the rescoring
// kernel's f32 score.  X, E: the corpus maxima above; qn = |q|, qtn = |bf16(q)|, en = |bf16(q) - q|, all f32.
//   * 1.001 covers the f32 rounding of the five norms (sums of <= 1024 squares: 1e-4 at the very most);
//   * squares below 2^-126 may have been flushed out of a norm: each norm is short by at most
//     sqrt(d) 2^-63 < 4e-18, added back here;
//   * products / inputs below 2^-126 may be flushed by the conversions and the matrix pipe: d 2^-120 (X + |q|).
#define PF_NORM_LIMIT 1.0e15f
#define PF_QNORM_MIN 1.0e-12f
__device__ __forceinline__ float pf_eps(float X, float E, float qn, float qtn, float en, uint32_t dim) {
    const float tiny = 4.0e-18f, d = (float)dim;
    const float Xs = X + tiny, Es = E + tiny, qts = qtn + tiny, ens = en + tiny;
    const float acc = d * 2.384185791015625e-07f; // d * 2^-22
    return 1.001f * (Es * qts + Xs * ens + acc * (Xs + Es) * qts) + d * 7.5231638452626401e-37f * (Xs + qn) + 1.0e-30f;
}

// One query row of the bf16 screen's block: bf16 copy (RNE, zero padded to n_padded rows) and the screen's margin 2 eps; a norm
// that is not finite, too large for the bf16 products to stay finite, or too small for its rounding errors to be measured in f32
// opens the exact pipeline instead (gate).  All 64 lanes of the wave call.
__device__ __forceinline__ void pf_stage_query_row(const float *__restrict__ q, uint32_t row, uint32_t n_queries, uint32_t dim,
                                                   const uint32_t *__restrict__ max_norm_bits, uint16_t *__restrict__ out,
                                                   float *__restrict__ eps2, uint32_t *gate) {
    const uint32_t lane = threadIdx.x & 63;
    float ss = 0.f, st = 0.f, se = 0.f;
    for (uint32_t k = lane; k < dim; k += 64) {
        uint16_t v = 0;
        if (row < n_queries) {
            const float f = q[(uint64_t)row * dim + k];
            v = (uint16_t)oi_f32_to_bf16_rne(f);
            const float ft = __uint_as_float((uint32_t)v << 16), e = ft - f; // exact: f rounded to 8 of its 24 bits
            ss = fmaf(f, f, ss);
            st = fmaf(ft, ft, st);
            se = fmaf(e, e, se);
        }
        out[(uint64_t)row * dim + k] = v;
    }
    if (row < n_queries) {
        ss = oi_wave_sum(ss);
        st = oi_wave_sum(st);
        se = oi_wave_sum(se);
        const float qn = sqrtf(ss), qtn = sqrtf(st), en = sqrtf(se);
        const float X = __uint_as_float(max_norm_bits[0]), E = __uint_as_float(max_norm_bits[1]);
        const bool ok = qn < PF_NORM_LIMIT && qn >= PF_QNORM_MIN && qtn < PF_NORM_LIMIT && X < PF_NORM_LIMIT &&
                        E < PF_NORM_LIMIT && en == en; // false for NaN as well
        if (lane == 0) {
            // A query without a bound gets an infinite margin: its threshold never rises, every key stays
            // inside the margin, the survivors overflow and the exact kernel scores it against every row.
            eps2[row] = ok ? 2.0f * pf_eps(X, E, qn, qtn, en, dim) : __builtin_inff();
            if (!ok) *gate = 1u;
        }
    }
}
