// oi_lds_dma.h -- what the streaming kernels share: the LDS-DMA ring primitives (descriptor, one 1-KiB piece, the counted
// wait, the compile-time loop the ring schedules are written in) and the per-wave staging ring the survivors leave through.
// Users: cosine_screen_i8.hip and cosine_bf16_qsplit's half-tile ring (cosine_bf16.hip) directly; oi_ksplit_tile.h: what
// cosine_ksplit and cosine_split (.hip) are written on; and oi_screen_tile.h: the tile pipeline that cosine_prefilter,
// cosine_screen_copy, cosine_bf16 (solo and pair), cosine_volume and cosine_summary (.hip, the last two through oi_volume.h) are
// written on.  bm25_stream.hip takes the address form (oi_dma_lane_word, oi_dma_global_piece) and the runtime-count wait.
//
// THE CONTRACT of an LDS-DMA load (`buffer_load_dwordx4 ... lds`: 64 lanes x 16 B from each lane's own source offset into
// 1 KiB of LDS at M0 + 16 * lane, no register destination):
//   * M0 carries the LDS destination.  It is compiler-reserved and not preserved around an asm statement, so the statement
//     that reads it also saves it, sets it and restores it (a clobber of m0 only draws a warning), with an `s_nop 0` between
//     the s_mov to M0 and the load that reads it.
//   * The LDS destination and the scalar offset are WAVE-UNIFORM by construction, which the compiler cannot always prove:
//     both go through readfirstlane, which makes them the scalar registers the "s" operands need.  The words of the
//     descriptor are made the same way (oi_make_srd).
//   * Range check: the descriptor has stride 0 and `bytes` records (clamped to 4 GiB), and a lane whose offset
//     voff + soff lies past them reads ZEROS.  The ragged last tile of a corpus and every tile after a wave's last one (an
//     EMPTY descriptor, bytes = 0) therefore need no branch and no clamping: the refill always issues, every counted wait is
//     the same constant.
//   * hipcc does not see these loads.  Nothing it emits waits for them, and nothing orders them against the ds_reads of the
//     data but the counted wait oi_wait_vm<N>(): vector-memory operations of a wave retire in issue order, so "at most N
//     outstanding" means everything older than the N youngest has landed.  Every load, store and atomic the compiler DOES
//     know about sits in the same queue: a kernel retires its own (queries, thresholds) with a wait the compiler models
//     before the ring starts (__builtin_amdgcn_s_waitcnt), or hipcc re-waits for them with vmcnt(0) inside the tile loop and
//     drains the ring; and survivors leave 64 at a time through the staging ring below, not one store each.
//   * Before the LDS goes back (kernel end) every DMA has landed: oi_wait_vm<0>().
//   * The `global_load_lds_*` form (bm25_stream.hip: oi_dma_lane_word, oi_dma_global_piece) takes an ADDRESS, not a
//     descriptor: nothing checks a range and no lane reads zeros, so every lane's address must be readable.  That is why
//     the postings array is padded (a chunk may run 1 KiB past its run) and why a lane without a run points at some valid
//     word.  M0 is handled exactly as above (saved, set from a readfirstlane, an s_nop in front of the load, restored), the
//     loads sit in the same in-order queue and are waited for with the same counted waits.
#pragma once

#include <type_traits>

#include "oi_device.h"

typedef uint32_t oi_u32x4 __attribute__((ext_vector_type(4)));

// The LDS byte address of a generic pointer into LDS.
__device__ __forceinline__ uint32_t oi_lds_addr(const void *p) {
    return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) const void *)p;
}
// Wave-uniform buffer descriptor of `bytes` bytes at `base`: stride 0 (raw offsets), size clamped to 4 GiB.
__device__ __forceinline__ oi_u32x4 oi_make_srd(const void *base, uint64_t bytes) {
    const uint64_t b = (uint64_t)base;
    oi_u32x4 r;
    r[0] = __builtin_amdgcn_readfirstlane((uint32_t)b);
    r[1] = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32) & 0xFFFFu); // stride 0
    r[2] = __builtin_amdgcn_readfirstlane((uint32_t)(bytes > 0xFFFFFFFFull ? 0xFFFFFFFFull : bytes));
    r[3] = 0x00020000u;
    return r;
}
// One 1-KiB LDS-DMA piece (8 rows x 128 B of a ring slot): lane l loads 16 B from srd + voff (per lane) + soff (uniform)
// into lds_dst + 16 l.  STREAM = true: the once-read policy of oi_device.h (OI_DMA_NT).  STREAM = false: the default cache
// policy -- sibling workgroups (cosine_bf16.hip) read every tile TWICE on one XCD and want the first read to stay in its L2.
template <bool STREAM = true>
__device__ __forceinline__ void oi_dma_piece(const oi_u32x4 &srd, uint32_t voff, uint32_t soff, uint32_t lds_dst) {
    uint32_t keep;
    const uint32_t d = __builtin_amdgcn_readfirstlane(lds_dst);
    const uint32_t so = __builtin_amdgcn_readfirstlane(soff);
    if constexpr (STREAM)
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %4\n\t"
            "s_nop 0\n\t"
            "buffer_load_dwordx4 %1, %2, %3 offen " OI_DMA_NT "lds\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(voff), "s"(srd), "s"(so), "s"(d)
            : "memory");
    else
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %4\n\t"
            "s_nop 0\n\t"
            "buffer_load_dwordx4 %1, %2, %3 offen lds\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(voff), "s"(srd), "s"(so), "s"(d)
            : "memory");
}
// (skip: a timing build's or a tail's "not this one", decided where the piece is issued)
template <bool STREAM = true>
__device__ __forceinline__ void oi_dma_piece(const oi_u32x4 &srd, uint32_t voff, uint32_t soff, uint32_t lds_dst, bool skip) {
    if (skip) return;
    oi_dma_piece<STREAM>(srd, voff, soff, lds_dst);
}
// Per-lane source of the 4 pieces of a slot (32 rows x 128 B): piece m covers tile rows 8m..8m+7; lane l -> row 8m + (l>>3),
// physical 16-B column l&7 holding LOGICAL column (l&7) ^ ((row>>1)&7), so that the ds_read_b128 fragment reads are
// conflict-free.  ROW_BYTES: 2 D (bf16 rows) or 4 D (f32).  base (wave-uniform bytes): where the wave's K-slice starts in a
// row (OiKsplitTile, oi_ksplit_tile.h; the K half of a cosine_bf16_pair wave through OiCopyRing, oi_screen_tile.h).
// cosine_screen_i8.hip writes the same offsets in a loop of its own (as a call its kernels come out different, and nothing
// bit-exact at every edge stands under them to allow that).
template <uint32_t ROW_BYTES>
__device__ __forceinline__ void oi_tile_voff(uint32_t (&voff)[4], uint32_t lane, uint32_t base = 0) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const uint32_t prow = 8 * m + (lane >> 3);
        voff[m] = prow * ROW_BYTES + base + (((lane & 7) ^ ((prow >> 1) & 7)) << 4);
    }
}
// Where a lane reads its A fragment of MFMA group g inside a slot: row li, bf16 16 g + 8 lh + 0..7 = logical 16-B column 2g + lh.
__device__ __forceinline__ void oi_tile_frag_off(uint32_t (&frag_off)[4], uint32_t li, uint32_t lh) {
#pragma unroll
    for (int g = 0; g < 4; ++g) frag_off[g] = li * 128 + (((2 * g + lh) ^ ((li >> 1) & 7)) << 4);
}
// f(integral_constant<int, I>) for I in [I, N): a ring schedule's slots and waits are compile-time constants.
template <int I, int N, class F>
__device__ __forceinline__ void oi_static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        oi_static_for<I + 1, N>(f);
    }
}
// At most N of this wave's vector-memory operations stay outstanding (see the contract above).
template <int N>
__device__ __forceinline__ void oi_wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
// The same with a wave-uniform RUNTIME count y ("the y issued after the one I need" may stay in flight; the instruction
// takes an immediate, hence the switch).  A smaller y than the truth only waits longer: 12 stands for every y above it.
__device__ __forceinline__ void oi_wait_vm_count(uint32_t y) {
    switch (__builtin_amdgcn_readfirstlane(y)) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
    case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
    case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
    case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
    case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    }
}

// ---- the address form (no descriptor: see the contract).
// One dword per lane from each lane's OWN address into lds_dst + 4 * lane (256 B of LDS).
__device__ __forceinline__ void oi_dma_lane_word(const uint32_t *gptr, uint32_t lds_dst) {
    uint32_t keep;
    const uint32_t d = __builtin_amdgcn_readfirstlane(lds_dst);
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 4\n\t"
        "global_load_lds_dword %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gptr), "s"(d)
        : "memory");
}
// One 1-KiB piece from a WAVE-UNIFORM base (an SGPR pair) plus a per-lane byte offset (16 * lane for a contiguous KiB):
// lane l loads 16 B from base + voff into lds_dst + 16 l.
__device__ __forceinline__ void oi_dma_global_piece(const void *base, uint32_t voff, uint32_t lds_dst) {
    uint32_t keep;
    const uint32_t d = __builtin_amdgcn_readfirstlane(lds_dst);
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %2\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(base), "s"(d)
        : "memory");
}

// ---- survivor staging of the screens and of cosine_bf16_qsplit: OI_STAGE entries per wave (a power of two) in LDS, flushed
// OI_STAGE_FLUSH at a time (fewer than OI_STAGE_FLUSH stay between tiles, so a tile of up to OI_STAGE - OI_STAGE_FLUSH
// survivors is staged).  Layout behind a kernel's own LDS: u64 keys [4 waves][OI_STAGE], then u32 queries [4][OI_STAGE].
#define OI_STAGE 256
#define OI_STAGE_FLUSH 64u
#define OI_STAGE_LDS (4 * OI_STAGE * 12)
// The first NF staged entries of the wave leave for the pool: lane l takes entry st_head + l, its position in its query's
// segment from ONE LDS atomic, one store instruction for all of them.  (A macro: a lambda would take st_head / st_n by
// reference and hipcc then keeps them in scratch.)  The compiler barriers keep the staging writes of other lanes in front of
// these reads, and these reads in front of the next tile's writes (LDS operations of a wave execute in order).
// Reads from the enclosing kernel (or from OiPoolSink, oi_screen_tile.h, whose members carry these names): lane, st_head, st_n (wave-uniform: first staged entry mod OI_STAGE, staged entries),
// stage_keys, stage_q (this wave's), seg_fill, seg_cap, my_seg, pool_stride, overflow.
#define OI_STAGE_FLUSH_TO_POOL(NF)                                                                                     \
    do {                                                                                                               \
        const uint32_t nf_ = (NF);                                                                                     \
        asm volatile("" ::: "memory");                                                                                 \
        if (lane < nf_) {                                                                                              \
            const uint32_t i_ = (st_head + lane) & (OI_STAGE - 1);                                                     \
            const uint64_t key_ = stage_keys[i_];                                                                      \
            const uint32_t q_ = stage_q[i_];                                                                           \
            const uint32_t pos_ = atomicAdd(&seg_fill[q_], 1u);                                                        \
            if (pos_ < seg_cap) my_seg[(uint64_t)q_ * pool_stride + pos_] = key_;                                      \
            else *overflow = 1u;                                                                                       \
        }                                                                                                              \
        asm volatile("" ::: "memory");                                                                                 \
        st_head = (st_head + nf_) & (OI_STAGE - 1);                                                                    \
        st_n -= nf_;                                                                                                   \
    } while (0)
