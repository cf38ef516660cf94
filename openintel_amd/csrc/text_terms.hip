// text_terms.hip -- post text -> hashed BM25 term ids, in text order (include/openintel_hip.h, "Text to term ids").
//
// The tokens are the reference's (src/adapters/analyzer/lexicon.rs:54-58: to_lowercase, split on every char that is not
// ASCII alphanumeric, drop empties), argued at byte level as in lexicon.hip: A-Z fold onto a-z; U+212A (E2 84 AA)
// lowercases to 'k' and joins the token around it; U+0130 (C4 B0) lowercases to 'i' + U+0307, i.e. 'i' followed by a
// separator; no other code point lowercases into [0-9a-z], so every other byte >= 0x80 separates.  A post's first byte
// starts a token.  term = fmix64(FNV-1a64(first 64 lowercased bytes)) mapped onto [0, vocab) by multiply-shift.
//
// Unlike lexicon_scan_kernel, which drops 97 % of the tokens behind a length screen and a Bloom filter, this one hashes
// EVERY token and writes an ordered, compacted stream: a count pass, a prefix sum over the tiles, an emit pass.
//   * The blob is cut into TILES of TT_TILE bytes at fixed 16-byte-aligned addresses, one workgroup each; a lane owns a
//     WINDOW of TT_LANE bytes.  Tiles are cut in the blob, not in posts: the post starts inside a tile are found with one
//     binary search of the offsets, so a 100 000-byte token and 10 000 empty posts are the same code path.
//   * Staging: 16-byte coalesced loads into LDS with a 16-byte halo in front and a 256-byte halo behind (a token that
//     starts in the tile is hashed by the lane that owns its first byte, at most 64 lowercased = 192 raw bytes on).
//     Every 16-byte unit is classified once by the lane that stages it (oi_alnum16) into a bit-per-byte map; units with
//     an E2 or C4 byte take the exact path, which sets the map's bits for E2 84 AA (all three: the token goes on) and for
//     the C4 of C4 B0.  Post starts are a second bitmap.  Token starts S = A & (~(A << 1 | prev) | P) and the
//     continuation map C = A & ~P are mask arithmetic on the lane's 64 bits.
//   * Order without atomics: token t of the blob goes to slot t.  count: popcount(S) summed per tile; rocprim exclusive
//     scan of the tile counts; emit: tile base + the workgroup's exclusive scan of the lane counts + the token's rank in
//     its lane.  text_offsets[i] = rank of the first token start at or after post i's first byte, written by the tile
//     that holds that byte.  The output is a pure function of the input: no grid-size, launch or timing dependence.
#include <cstring>

#include <rocprim/device/device_scan.hpp>

#include "oi_device.h"
#include "oi_internal.h"

#define TT_THREADS 256u
#define TT_LANE 64u                                // bytes per lane window
#define TT_TILE 16384u                             // bytes per workgroup tile (the tests read these two from this file)
#define TT_PRE 16u                                 // halo in front: the byte before the tile, and a U+212A ending there
#define TT_POST 256u                               // halo behind: 64 hashed bytes are at most 192 raw bytes, + look-ahead
#define TT_SPAN (TT_PRE + TT_TILE + TT_POST)       // staged bytes; r = position relative to the tile's first byte, + TT_PRE
#define TT_UNITS (TT_SPAN / 16u)                   // 1041
#define TT_STEPS ((TT_UNITS + TT_THREADS - 1u) / TT_THREADS)
#define TT_BIT0 48u                                // bit of byte r is TT_BIT0 + r: lane window c is u64 number 1 + c
#define TT_W64 ((TT_BIT0 + TT_SPAN) / 64u)         // 261
static_assert(TT_TILE == TT_THREADS * TT_LANE && TT_LANE == 64u, "a lane window is one 64-bit mask");
static_assert((TT_BIT0 + TT_SPAN) % 64u == 0u && TT_SPAN % 16u == 0u, "bitmaps are whole u64 words");
static_assert(TT_POST >= 3u * OI_TEXT_TOKEN_HASH_BYTES + 3u, "the hash never leaves the staged bytes");

struct TtShared {
    uint4 text[TT_UNITS];     // bytes r = 0 .. TT_SPAN
    uint64_t abits[TT_W64];   // 1 = byte belongs to a token (ASCII alnum, E2 84 AA, the C4 of C4 B0)
    uint64_t pbits[TT_W64];   // 1 = first byte of a post (or the end of the last one)
    uint64_t cbits[TT_W64];   // 1 = byte continues the token of the byte before it
    uint64_t sbits[TT_THREADS];  // token starts of lane window c
    uint32_t prefix[TT_THREADS]; // token starts of the tile in front of lane window c
    uint32_t wsum[TT_THREADS / 64u];
    uint32_t total;
};

__device__ __forceinline__ uint32_t tt_byte_mask(uint32_t nbytes) { // low nbytes bytes, 0..4
    return nbytes >= 4u ? 0xFFFFFFFFu : (1u << (8u * nbytes)) - 1u;
}
__device__ __forceinline__ bool tt_has_byte(uint32_t w, uint32_t b) { // some byte of w equals b
    const uint32_t x = w ^ (b * 0x01010101u);
    return ((x - 0x01010101u) & ~x & 0x80808080u) != 0u;
}

// first index j in [0, n] with offsets[j] + skew >= q (offsets non-decreasing; n + 1 entries)
template <class OffT>
__device__ __forceinline__ uint64_t tt_lower_bound(const OffT *offsets, uint64_t n, uint64_t skew, uint64_t q) {
    uint64_t lo = 0, hi = n + 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)offsets[mid] + skew < q) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Stage tile `tile` and build its maps.  `base` = the blob's address rounded down to 16 bytes, skew = what was cut off:
// positions q are relative to base, the text is q in [skew, end).  Returns the token starts of this lane's window and
// j0 = the first post whose start is at or behind the tile's first byte.  Ends with the block in step.
template <class OffT>
__device__ __forceinline__ uint64_t tt_stage(TtShared &s, const uint8_t *base, uint32_t skew, uint64_t end, const OffT *offsets,
                                             uint64_t n, uint64_t tile, uint64_t *j0_out) {
    const uint32_t tid = threadIdx.x;
    const uint64_t g0 = tile * TT_TILE; // q of the tile's first byte; the staged span starts at g0 - TT_PRE
    uint16_t *ab16 = reinterpret_cast<uint16_t *>(s.abits);
    const uint8_t *text8 = reinterpret_cast<const uint8_t *>(s.text);
    for (uint32_t i = tid; i < TT_W64; i += TT_THREADS) s.pbits[i] = 0ull;
    if (tid < 3u) ab16[tid] = 0;
    uint32_t special = 0;
#pragma unroll
    for (uint32_t k = 0; k < TT_STEPS; ++k) {
        const uint32_t v = tid + k * TT_THREADS;
        if (v >= TT_UNITS) continue;
        const int64_t a = (int64_t)g0 + 16 * (int64_t)v - (int64_t)TT_PRE; // q of the unit's first byte (a multiple of 16)
        uint4 x = make_uint4(0u, 0u, 0u, 0u);
        if (a + 16 > (int64_t)skew && a < (int64_t)end) { // the unit holds text (so a >= 0: skew < 16)
            x = *reinterpret_cast<const uint4 *>(base + a);
            if (a < (int64_t)skew || a + 16 > (int64_t)end) { // the blob's first or last unit: bytes outside the text read as 0
                const uint32_t lo = a < (int64_t)skew ? (uint32_t)((int64_t)skew - a) : 0u;
                const uint32_t hi = a + 16 > (int64_t)end ? (uint32_t)((int64_t)end - a) : 16u;
                uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (uint32_t d = 0; d < 4; ++d) {
                    const uint32_t l = lo > 4u * d ? lo - 4u * d : 0u, h = hi > 4u * d ? hi - 4u * d : 0u;
                    w[d] &= tt_byte_mask(h) & ~tt_byte_mask(l);
                }
                x = make_uint4(w[0], w[1], w[2], w[3]);
            }
        }
        s.text[v] = x;
        ab16[3u + v] = (uint16_t)oi_alnum16(x);
        if ((x.x | x.y | x.z | x.w) & 0x80808080u) {
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
            bool sp = false;
#pragma unroll
            for (int d = 0; d < 4; ++d) sp = sp || tt_has_byte(w[d], 0xE2u) || tt_has_byte(w[d], 0xC4u);
            if (sp) special |= 1u << k;
        }
    }
    // post starts inside the staged span (one bit per distinct start; empty posts share theirs)
    const uint64_t j0 = tt_lower_bound(offsets, n, skew, g0);
    *j0_out = j0;
    __syncthreads(); // every word of pbits is zero before any lane sets a bit in it (a lane sets bits in other lanes' words)
    for (uint64_t i = j0 + tid; i <= n; i += TT_THREADS) {
        const uint64_t o = (uint64_t)offsets[i] + skew;
        if (o >= g0 + TT_TILE + TT_POST) break;
        if (o < g0) continue; // (offsets that decrease break the contract; they must not reach outside the bitmap)
        const uint32_t bit = TT_BIT0 + TT_PRE + (uint32_t)(o - g0);
        atomicOr(reinterpret_cast<unsigned long long *>(&s.pbits[bit >> 6]), 1ull << (bit & 63u));
    }
    __syncthreads();
    // the exact path: the two code points whose lowercase is ASCII (rare: a unit with an E2 or a C4 byte)
    if (special) {
#pragma unroll
        for (uint32_t k = 0; k < TT_STEPS; ++k) {
            if (!((special >> k) & 1u)) continue;
            const uint32_t r0 = (tid + k * TT_THREADS) * 16u;
            for (uint32_t r = r0; r < r0 + 16u; ++r) {
                const uint32_t c = text8[r];
                uint64_t m = 0;
                if (c == 0xE2u && r + 2u < TT_SPAN && text8[r + 1u] == 0x84u && text8[r + 2u] == 0xAAu) m = 7ull;
                else if (c == 0xC4u && r + 1u < TT_SPAN && text8[r + 1u] == 0xB0u) m = 1ull;
                if (m) {
                    const uint32_t bit = TT_BIT0 + r, sh = bit & 63u;
                    atomicOr(reinterpret_cast<unsigned long long *>(&s.abits[bit >> 6]), m << sh);
                    if (sh > 61u && (bit >> 6) + 1u < TT_W64)
                        atomicOr(reinterpret_cast<unsigned long long *>(&s.abits[(bit >> 6) + 1u]), m >> (64u - sh));
                }
            }
        }
    }
    __syncthreads();
    const uint64_t A = s.abits[1u + tid], P = s.pbits[1u + tid], prev = s.abits[tid] >> 63;
    s.cbits[1u + tid] = A & ~P;
    if (tid < TT_POST / 64u) s.cbits[1u + TT_THREADS + tid] = s.abits[1u + TT_THREADS + tid] & ~s.pbits[1u + TT_THREADS + tid];
    return A & (~((A << 1) | prev) | P);
}

// The term id of the token whose first byte is staged at r (include/openintel_hip.h has the definition).
__device__ __forceinline__ uint32_t tt_hash_token(const TtShared &s, uint32_t r, uint32_t vocab) {
    const uint8_t *text8 = reinterpret_cast<const uint8_t *>(s.text);
    const uint32_t *cb32 = reinterpret_cast<const uint32_t *>(s.cbits);
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint32_t cnt = 0; cnt < OI_TEXT_TOKEN_HASH_BYTES; ++cnt) {
        const uint32_t c = text8[r];
        uint32_t m = c | 0x20u, step = 1u;            // [0-9A-Za-z] -> [0-9a-z]
        if (c >= 0x80u) {
            if (c == 0xE2u) { m = 'k'; step = 3u; }   // E2 84 AA (only a byte of a mapped code point has its bit set)
            else m = 'i';                             // the C4 of C4 B0; B0 has no bit, so the token ends here
        }
        h = (h ^ (uint64_t)m) * 0x100000001b3ull;
        r += step;
        const uint32_t bit = TT_BIT0 + r;
        if (r >= TT_SPAN || !((cb32[bit >> 5] >> (bit & 31u)) & 1u)) break;
    }
    h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
    return (uint32_t)(((h >> 32) * (uint64_t)vocab) >> 32);
}

template <class OffT>
__global__ __launch_bounds__(TT_THREADS) void text_terms_count_kernel(const uint8_t *base, uint32_t skew, uint64_t end,
                                                                      const OffT *offsets, uint64_t n, uint32_t *tile_count) {
    __shared__ __attribute__((aligned(16))) TtShared s;
    const uint32_t tid = threadIdx.x;
    uint64_t j0;
    const uint64_t S = tt_stage(s, base, skew, end, offsets, n, blockIdx.x, &j0);
    const uint32_t c = oi_wave_sum((uint32_t)__popcll(S));
    if ((tid & 63u) == 0u) s.wsum[tid >> 6] = c;
    __syncthreads();
    if (tid == 0u) tile_count[blockIdx.x] = s.wsum[0] + s.wsum[1] + s.wsum[2] + s.wsum[3];
}

// EMIT = false: the offsets only (the count-only call).
template <class OffT, bool EMIT>
__global__ __launch_bounds__(TT_THREADS) void text_terms_emit_kernel(const uint8_t *base, uint32_t skew, uint64_t end,
                                                                     const OffT *offsets, uint64_t n, const uint64_t *tile_base,
                                                                     uint64_t n_tiles, uint32_t vocab, uint32_t *terms_out,
                                                                     uint64_t capacity, OffT *text_offsets_out) {
    __shared__ __attribute__((aligned(16))) TtShared s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t tile = blockIdx.x, g0 = tile * TT_TILE;
    uint64_t j0;
    uint64_t S = tt_stage(s, base, skew, end, offsets, n, tile, &j0);
    // exclusive scan of the lane counts over the workgroup (fixed shape)
    const uint32_t cnt = (uint32_t)__popcll(S);
    uint32_t incl = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, OI_WAVE);
        if ((int)lane >= o) incl += v;
    }
    if (lane == 63u) s.wsum[wv] = incl;
    __syncthreads();
    uint32_t before = incl - cnt;
    for (uint32_t w = 0; w < wv; ++w) before += s.wsum[w];
    s.prefix[tid] = before;
    s.sbits[tid] = S;
    if (tid == TT_THREADS - 1u) s.total = before + cnt;
    __syncthreads();
    const uint64_t out0 = tile_base[tile];
    // the posts that start in this tile: the rank of the first token start at or behind their first byte
    for (uint64_t i = j0 + tid; i <= n; i += TT_THREADS) {
        const uint64_t o = (uint64_t)offsets[i] + skew;
        if (o >= g0 + TT_TILE) {
            // the end of the text on a tile edge belongs to no tile: the last one writes it (trailing empty posts, entry n)
            if (tile + 1 == n_tiles && o == g0 + TT_TILE) { text_offsets_out[i] = (OffT)(out0 + s.total); continue; }
            break;
        }
        if (o < g0) continue; // (as in tt_stage)
        const uint32_t rel = (uint32_t)(o - g0), c = rel >> 6, b = rel & 63u;
        text_offsets_out[i] = (OffT)(out0 + s.prefix[c] + (uint32_t)__popcll(s.sbits[c] & ((1ull << b) - 1ull)));
    }
    if (EMIT) {
        uint64_t slot = out0 + before;
        const uint32_t r_lane = TT_PRE + tid * TT_LANE;
        while (S) {
            const uint32_t b = (uint32_t)__builtin_ctzll(S);
            S &= S - 1ull;
            const uint32_t term = tt_hash_token(s, r_lane + b, vocab);
            // (never the limiter: the host either checked total <= capacity before this launch or capacity >= (bytes + 1) / 2
            // >= total; kept so that offsets which break the contract cannot make the kernel write outside the buffer)
            if (slot < capacity) terms_out[slot] = term;
            ++slot;
        }
    }
}

// ---------------------------------------------------------------- host side
namespace {

#define TT_STAGE_KEEP ((size_t)16 << 20) // host-call staging buffers larger than this are freed when the call returns

// A query batch's staging stays in the ctx's workspace for the next call; a corpus-sized one (GBs) is given back when the
// call returns, on every path (hipFree waits for the device).
struct TtStageTrim {
    oi_ctx *ctx;
    ~TtStageTrim() {
        for (const char *name : {"tt_stage_in", "tt_stage_off", "tt_stage_terms"})
            if (ctx->buf(name).cap > TT_STAGE_KEEP) ctx->buf(name).release();
    }
};

struct TtPlan {
    const uint8_t *base;
    uint32_t skew;
    uint64_t end, n_tiles;
};

TtPlan tt_plan(const uint8_t *d_blob, uint64_t blob_bytes) {
    TtPlan p;
    const uintptr_t a = reinterpret_cast<uintptr_t>(d_blob);
    p.skew = (uint32_t)(a & 15u);
    p.base = reinterpret_cast<const uint8_t *>(a - p.skew);
    p.end = p.skew + blob_bytes;
    p.n_tiles = blob_bytes ? (p.end + TT_TILE - 1) / TT_TILE : 0;
    return p;
}

// Count pass + scan: leaves the tile bases (n_tiles + 1 entries, the last one the total) in the ctx's workspace.
template <class OffT>
int tt_count(oi_ctx *ctx, const TtPlan &p, const OffT *d_offsets, uint64_t n) {
    hipStream_t st = ctx->stream;
    OI_REQUIRE(p.n_tiles < (1ull << 24), "text terms: %llu bytes in one call (limit 256 GiB)", (unsigned long long)p.end);
    DevBuf &cnt = ctx->buf("tt_count"), &base = ctx->buf("tt_base"), &tmp = ctx->buf("tt_scan_tmp");
    OI_CHECK(cnt.ensure(sizeof(uint32_t) * (p.n_tiles + 1)));
    OI_CHECK(base.ensure(sizeof(uint64_t) * (p.n_tiles + 1)));
    OI_HIP_CHECK(hipMemsetAsync(cnt.as<uint32_t>() + p.n_tiles, 0, sizeof(uint32_t), st));
    ProfScope ps(ctx, "text_count"); // the count kernel and the scan of the tile counts
    hipLaunchKernelGGL(HIP_KERNEL_NAME(text_terms_count_kernel<OffT>), dim3((uint32_t)p.n_tiles), dim3(TT_THREADS), 0, st, p.base,
                       p.skew, p.end, d_offsets, n, cnt.as<uint32_t>());
    OI_HIP_CHECK(hipGetLastError());
    size_t bytes = 0;
    OI_HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, cnt.as<uint32_t>(), base.as<uint64_t>(), (uint64_t)0,
                                         (size_t)(p.n_tiles + 1), rocprim::plus<uint64_t>(), st));
    OI_CHECK(tmp.ensure(bytes ? bytes : 16));
    OI_HIP_CHECK(rocprim::exclusive_scan(tmp.p, bytes, cnt.as<uint32_t>(), base.as<uint64_t>(), (uint64_t)0,
                                         (size_t)(p.n_tiles + 1), rocprim::plus<uint64_t>(), st));
    return OI_OK;
}

template <class OffT>
int tt_emit(oi_ctx *ctx, const TtPlan &p, const OffT *d_offsets, uint64_t n, uint32_t vocab, uint32_t *d_terms,
            uint64_t capacity, OffT *d_text_offsets) {
    const uint64_t *tile_base = ctx->buf("tt_base").as<uint64_t>();
    ProfScope ps(ctx, "text_emit");
    if (d_terms)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(text_terms_emit_kernel<OffT, true>), dim3((uint32_t)p.n_tiles), dim3(TT_THREADS), 0,
                           ctx->stream, p.base, p.skew, p.end, d_offsets, n, tile_base, p.n_tiles, vocab, d_terms, capacity,
                           d_text_offsets);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(text_terms_emit_kernel<OffT, false>), dim3((uint32_t)p.n_tiles), dim3(TT_THREADS), 0,
                           ctx->stream, p.base, p.skew, p.end, d_offsets, n, tile_base, p.n_tiles, vocab, d_terms, capacity,
                           d_text_offsets);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// Count pass + the total on the host (synchronises the stream).  No text: no launch, total 0.
template <class OffT>
int tt_count_total(oi_ctx *ctx, const uint8_t *d_blob, const OffT *d_offsets, uint64_t n, uint64_t blob_bytes, uint64_t *total) {
    *total = 0;
    if (n == 0 || blob_bytes == 0) return OI_OK;
    const TtPlan p = tt_plan(d_blob, blob_bytes);
    OI_CHECK(tt_count(ctx, p, d_offsets, n));
    OI_HIP_CHECK(hipMemcpyAsync(total, ctx->buf("tt_base").as<uint64_t>() + p.n_tiles, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    OI_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return OI_OK;
}

// Device buffers in, device buffers out (ctx locked, device set).  d_terms == NULL: offsets and total only.
template <class OffT>
int tt_run_device(oi_ctx *ctx, const uint8_t *d_blob, const OffT *d_offsets, uint64_t n, uint64_t blob_bytes, uint32_t vocab,
                  uint32_t *d_terms, uint64_t capacity, OffT *d_text_offsets, uint64_t *total_out_host) {
    hipStream_t st = ctx->stream;
    if (total_out_host) *total_out_host = 0;
    if (n == 0 || blob_bytes == 0) { // no text: every offset is 0
        OI_HIP_CHECK(hipMemsetAsync(d_text_offsets, 0, sizeof(OffT) * (n + 1), st));
        return OI_OK;
    }
    const TtPlan p = tt_plan(d_blob, blob_bytes);
    OI_CHECK(tt_count(ctx, p, d_offsets, n));
    const bool check = d_terms && capacity < (blob_bytes + 1) / 2; // two tokens need a separator: more can never come out
    if (total_out_host || check) {
        uint64_t total = 0;
        OI_HIP_CHECK(hipMemcpyAsync(&total, ctx->buf("tt_base").as<uint64_t>() + p.n_tiles, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        OI_HIP_CHECK(hipStreamSynchronize(st));
        if (total_out_host) *total_out_host = total;
        if (sizeof(OffT) == 4 && total > 0xFFFFFFFFull) {
            oi_set_error("query terms: %llu terms do not fit u32 offsets", (unsigned long long)total);
            return OI_ERR_OVERFLOW;
        }
        if (d_terms && total > capacity) {
            oi_set_error("text terms: %llu term ids, term_capacity is %llu", (unsigned long long)total, (unsigned long long)capacity);
            return OI_ERR_OVERFLOW;
        }
    }
    return tt_emit(ctx, p, d_offsets, n, vocab, d_terms, capacity, d_text_offsets);
}

template <class OffT>
int tt_check_args(oi_ctx *ctx, const uint8_t *blob, const OffT *offsets, uint64_t blob_bytes, uint32_t vocab, int location,
                  const void *text_offsets_out) {
    if (!ctx) { oi_set_error("null ctx"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(location == OI_HOST || location == OI_DEVICE, "text terms: bad location %d", location);
    OI_REQUIRE(vocab != 0, "text terms: vocab must be at least 1");
    OI_REQUIRE(offsets && text_offsets_out, "text terms: null offsets");
    OI_REQUIRE(blob || blob_bytes == 0, "text terms: null text blob");
    return OI_OK;
}

// The whole call for either offset width.  OI_HOST: one staging buffer in, the results copied back.
template <class OffT>
int tt_call(oi_ctx *ctx, const uint8_t *blob, const OffT *offsets, uint64_t n, uint64_t blob_bytes, uint32_t vocab, int location,
            uint32_t *terms_out, uint64_t capacity, OffT *text_offsets_out, uint64_t *total_out_host) {
    OI_CHECK(tt_check_args(ctx, blob, offsets, blob_bytes, vocab, location, text_offsets_out));
    if (location == OI_HOST) {
        OI_REQUIRE(offsets[0] == 0, "text terms: offsets[0] must be 0");
        OI_REQUIRE((uint64_t)offsets[n] == blob_bytes, "text terms: offsets[n] = %llu but blob_bytes = %llu",
                   (unsigned long long)offsets[n], (unsigned long long)blob_bytes);
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    if (location == OI_DEVICE)
        return tt_run_device(ctx, blob, offsets, n, blob_bytes, vocab, terms_out, capacity, text_offsets_out, total_out_host);
    hipStream_t st = ctx->stream;
    const size_t off_o = (blob_bytes + 15) & ~(size_t)15, off_bytes = sizeof(OffT) * (n + 1);
    DevBuf &in = ctx->buf("tt_stage_in"), &oo = ctx->buf("tt_stage_off");
    TtStageTrim trim{ctx};
    OI_CHECK(in.ensure(off_o + off_bytes));
    OI_CHECK(oo.ensure(off_bytes));
    uint8_t *d_in = in.as<uint8_t>();
    if (blob_bytes) OI_HIP_CHECK(hipMemcpyAsync(d_in, blob, blob_bytes, hipMemcpyHostToDevice, st));
    OI_HIP_CHECK(hipMemcpyAsync(d_in + off_o, offsets, off_bytes, hipMemcpyHostToDevice, st));
    const OffT *d_offs = reinterpret_cast<const OffT *>(d_in + off_o);
    uint64_t total = 0;
    // the count comes back first, so the ids buffer is exactly as large as the text needs
    OI_CHECK(tt_count_total<OffT>(ctx, d_in, d_offs, n, blob_bytes, &total));
    if (total_out_host) *total_out_host = total;
    if (terms_out && total > capacity) {
        oi_set_error("text terms: %llu term ids, term_capacity is %llu", (unsigned long long)total, (unsigned long long)capacity);
        return OI_ERR_OVERFLOW;
    }
    if (total == 0) { // no token at all: every offset is 0
        OI_HIP_CHECK(hipMemsetAsync(oo.p, 0, off_bytes, st));
    } else {
        uint32_t *d_terms = nullptr;
        if (terms_out) {
            DevBuf &t = ctx->buf("tt_stage_terms");
            OI_CHECK(t.ensure(sizeof(uint32_t) * total));
            d_terms = t.as<uint32_t>();
        }
        OI_CHECK(tt_emit(ctx, tt_plan(d_in, blob_bytes), d_offs, n, vocab, d_terms, total, oo.as<OffT>()));
        if (terms_out) OI_HIP_CHECK(hipMemcpyAsync(terms_out, d_terms, sizeof(uint32_t) * total, hipMemcpyDeviceToHost, st));
    }
    OI_HIP_CHECK(hipMemcpyAsync(text_offsets_out, oo.p, off_bytes, hipMemcpyDeviceToHost, st));
    OI_HIP_CHECK(hipStreamSynchronize(st));
    return OI_OK;
}

} // namespace

extern "C" int oi_text_terms(oi_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, uint64_t n_texts, uint64_t blob_bytes,
                             uint32_t vocab, int location, uint32_t *term_ids_out, uint64_t term_capacity,
                             uint64_t *text_offsets_out, uint64_t *total_out_host) {
    return tt_call<uint64_t>(ctx, blob, offsets, n_texts, blob_bytes, vocab, location, term_ids_out, term_capacity,
                             text_offsets_out, total_out_host);
}

extern "C" int oi_query_terms(oi_ctx *ctx, const uint8_t *blob, const uint32_t *offsets, uint32_t n_queries, uint32_t blob_bytes,
                              uint32_t vocab, int location, uint32_t *query_terms_out, uint64_t term_capacity,
                              uint32_t *q_term_offsets_out, uint64_t *total_out_host) {
    return tt_call<uint32_t>(ctx, blob, offsets, n_queries, blob_bytes, vocab, location, query_terms_out, term_capacity,
                             q_term_offsets_out, total_out_host);
}

extern "C" int oi_index_set_text(oi_index *idx, const uint8_t *blob, const uint64_t *offsets, uint64_t blob_bytes, int location) {
    if (!idx || !offsets) { oi_set_error("null argument"); return OI_ERR_INVALID_ARG; }
    OI_REQUIRE(location == OI_HOST || location == OI_DEVICE, "set_text: bad location %d", location);
    OI_REQUIRE(blob || blob_bytes == 0, "set_text: null text blob");
    if (idx->is_view) { oi_set_error("index view: read-only (set the data on the index it was taken from)"); return OI_ERR_STATE; }
    oi_ctx *ctx = idx->ctx;
    const uint64_t n = idx->n_docs;
    if (location == OI_HOST) {
        OI_REQUIRE(offsets[0] == 0, "set_text: offsets[0] must be 0");
        OI_REQUIRE(offsets[n] == blob_bytes, "set_text: offsets[n_docs] = %llu but blob_bytes = %llu",
                   (unsigned long long)offsets[n], (unsigned long long)blob_bytes);
    }
    std::lock_guard<std::mutex> g(ctx->mu);
    OI_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf stage, terms, toffs; // freed when the call returns: the index keeps its own copy of the forward index
    const uint8_t *d_blob = blob;
    const uint64_t *d_offsets = offsets;
    if (location == OI_HOST) {
        const size_t off_o = (blob_bytes + 15) & ~(size_t)15;
        OI_CHECK(stage.ensure(off_o + sizeof(uint64_t) * (n + 1)));
        if (blob_bytes) OI_HIP_CHECK(hipMemcpyAsync(stage.p, blob, blob_bytes, hipMemcpyHostToDevice, st));
        OI_HIP_CHECK(hipMemcpyAsync(stage.as<uint8_t>() + off_o, offsets, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, st));
        d_blob = stage.as<uint8_t>();
        d_offsets = reinterpret_cast<const uint64_t *>(stage.as<uint8_t>() + off_o);
    }
    OI_CHECK(toffs.ensure(sizeof(uint64_t) * (n + 1)));
    // (device offsets cannot be checked: an entry beyond blob_bytes is written by no tile, and must still be defined)
    OI_HIP_CHECK(hipMemsetAsync(toffs.p, 0, sizeof(uint64_t) * (n + 1), st));
    uint64_t total = 0;
    int rc = tt_count_total<uint64_t>(ctx, d_blob, d_offsets, n, blob_bytes, &total);
    if (rc == OI_OK && total >= 0xFFFFFFFFull) {
        oi_set_error("bm25: %llu tokens in one shard (limit 2^32-1)", (unsigned long long)total);
        rc = OI_ERR_INVALID_ARG;
    }
    if (rc == OI_OK) rc = terms.ensure(sizeof(uint32_t) * (total ? total : 1));
    if (rc == OI_OK) { // one emit pass writes the ids and the offsets; no token at all: every offset stays 0
        if (total) rc = tt_emit(ctx, tt_plan(d_blob, blob_bytes), d_offsets, n, idx->vocab, terms.as<uint32_t>(), total, toffs.as<uint64_t>());
    }
    if (rc == OI_OK) rc = oi_bm25_stage_forward(idx, terms.as<uint32_t>(), toffs.as<uint64_t>());
    (void)hipStreamSynchronize(st); // the staging buffers go out of scope
    return rc;
}
