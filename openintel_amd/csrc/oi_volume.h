// oi_volume.h -- what the threshold-counting calls share: oi_similar_volume (cosine_volume.hip) and
// oi_similar_summary (cosine_summary.hip).  The tile geometry and state words of the stream route, the bucket
// clause, the band staging and the f32 chain that defines sim.  Device code only; every function is inlined.
#pragma once

#include "oi_device.h"
#include "oi_internal.h"
#include "oi_lds_dma.h"

typedef float vo_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 vo_bf16x8 __attribute__((ext_vector_type(8)));

#define VO_TILE_ROWS 32
#define VO_SLOT_K 64                 // bf16 of K per ring slot row (128 B)
#define VO_SLOT_BYTES (VO_TILE_ROWS * 128)
#define VO_BAND_CAP (4u << 20)       // undecided pairs per call: 32 MB, the collapse mask's budget
#define VO_NBUF 8                    // the copy screen's ring depth (cosine_screen_copy.hip: depth is not what holds the stream)
// state words of a call (zeroed by it): [0] gate (a query without a bound), [1] band overflow, [2] band fill
#define VO_GATE 0
#define VO_OVERFLOW 1
#define VO_BAND_CNT 2

// Clause 2 of the definition: the bucket of a stamp.  stamp >= origin makes the 32-bit difference exact, so origin + n * width
// may exceed 2^32 without a 64-bit division.
__device__ __forceinline__ bool vo_bucket(uint32_t stamp, uint32_t origin, uint32_t width, uint32_t n_buckets, uint32_t *b) {
    if (width == 0u) { *b = 0u; return true; }
    if (stamp < origin) return false;
    const uint32_t k = (stamp - origin) / width;
    *b = k;
    return k < n_buckets;
}

// The first NF staged band pairs of the wave leave for the band buffer: ONE atomic claims their room, one store instruction
// writes them.  (A macro for the reason OI_STAGE_FLUSH_TO_POOL is one.)  Reads from the enclosing kernel: lane, st_head, st_n,
// stage_keys, band, band_cnt, band_cap, overflow.
#define VO_STAGE_FLUSH_TO_BAND(NF)                                                                                     \
    do {                                                                                                               \
        const uint32_t nf_ = (NF);                                                                                     \
        asm volatile("" ::: "memory");                                                                                 \
        uint32_t base_ = 0;                                                                                            \
        if (lane == 0) base_ = atomicAdd(band_cnt, nf_);                                                               \
        base_ = __builtin_amdgcn_readfirstlane(base_);                                                                 \
        if (lane < nf_) {                                                                                              \
            const uint64_t key_ = stage_keys[(st_head + lane) & (OI_STAGE - 1)];                                       \
            if (base_ + lane < band_cap && base_ + lane >= base_) band[base_ + lane] = key_;                           \
            else *overflow = 1u;                                                                                       \
        }                                                                                                              \
        asm volatile("" ::: "memory");                                                                                 \
        st_head = (st_head + nf_) & (OI_STAGE - 1);                                                                    \
        st_n -= nf_;                                                                                                   \
    } while (0)

// ------------------------------------------------------------------ the chain
// Four floats of a stored row as the chain sees them: f32 as they are, bf16 widened exactly.
template <bool BF16>
__device__ __forceinline__ float4 vo_load_row4(const void *row, uint32_t v) {
    if constexpr (BF16) {
        const uint2 u = oi_load_stream(reinterpret_cast<const uint2 *>(row) + v);
        return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xFFFF0000u), __uint_as_float(u.y << 16),
                           __uint_as_float(u.y & 0xFFFF0000u));
    } else {
        return oi_load_stream(reinterpret_cast<const float4 *>(row) + v);
    }
}
// one float4 step of pf_rescore_kernel's chain: single v_fma_f32 each (oi_device.h: a packed op_sel fma beside another
// lane's MFMA stream has produced a wrong score)
__device__ __forceinline__ float vo_chain4(const float4 x, const float4 y, float a) {
    a = oi_fma_unpacked(x.x, y.x, a); a = oi_fma_unpacked(x.y, y.y, a);
    a = oi_fma_unpacked(x.z, y.z, a); a = oi_fma_unpacked(x.w, y.w, a);
    return a;
}
