// oi_summary_cell.h -- the 16-word cell of the summing tallies: oi_similar_summary (cosine_summary.hip) keeps one
// per (query, time bucket), oi_similar_groups (cosine_groups.hip) one per (query, key).  Layout and reasons are
// stated at the head of cosine_summary.hip.
#pragma once

#include "oi_device.h"
#include "oi_internal.h"

#define SM_CELL_WORDS 16
#define SM_CELL_SUM 12   // word offset of the i64 sum inside a cell (8-byte aligned: cells are 64 B)
// classes of a record, as social_summary_kernel tests them (speculation_engine.rs:87-95)
#define SM_BULLISH 0u
#define SM_BEARISH 1u
#define SM_NEUTRAL 2u

// One hit: the record sg = {pol_q30 bits, flag combination < 12} of the row goes into cell `cell`.
__device__ __forceinline__ void sm_add(uint32_t *cells, uint64_t cell, const uint2 sg) {
    uint32_t *c = cells + cell * SM_CELL_WORDS;
    atomicAdd(c + sg.y, 1u);
    if (sg.x != 0u)
        atomicAdd(reinterpret_cast<unsigned long long *>(c + SM_CELL_SUM), (unsigned long long)(long long)(int32_t)sg.x);
}

// A cell's 12 counts folded into the record *dst; polarity_sum = (double)(sum of pol_q30) * 2^-30, one rounding at most
// (the conversion: the scaling by a power of two is exact).
__device__ __forceinline__ void sm_fold(const uint32_t *c, oi_social_counters *dst) {
    uint64_t cls[3] = {0, 0, 0}, spec = 0, src1 = 0, total = 0;
#pragma unroll
    for (uint32_t f = 0; f < 12; ++f) {
        const uint64_t k = c[f];
        total += k;
        cls[f % 3u] += k;
        if ((f / 3u) & 1u) spec += k;
        if (f >= 6u) src1 += k;
    }
    oi_social_counters o;
    o.total = total;
    o.by_source[0] = total - src1;
    o.by_source[1] = src1;
    o.bullish = cls[SM_BULLISH];
    o.bearish = cls[SM_BEARISH];
    o.neutral = cls[SM_NEUTRAL];
    o.spec_count = spec;
    o.polarity_sum = (double)*reinterpret_cast<const long long *>(c + SM_CELL_SUM) * (1.0 / 1073741824.0);
    *dst = o;
}
