// collapse.hip -- near-duplicate collapse of ranked lists (oi_collapse_lists / oi_search_collapsed).
//
// Two stages per slice of queries, both on the ctx stream:
//   collapse_gram_kernel   per query, the lower triangle of the Gram matrix of the list's rows on the exact f32 MFMA, compared
//                          with the threshold: one bit per pair (i, j <= i) in a per-query mask of P x P/64 u64 words
//                          (P = depth rounded up to 128).  Rows are read straight from the index by doc id.  Measured, with
//                          the counters that say where its time goes: DESIGN 4.9.
//   collapse_sweep_kernel  one wave per query walks the list in rank order with the kept set as a bitset across lanes:
//                          entry i is kept when (mask row i AND kept) is empty, else counted to the lowest set bit.
//
// Mask words: word w of row i holds pairs (i, 64 w .. 64 w + 63).  The Gram kernel writes every word w <= i / 64 of every row
// below the list's padded length exactly once (whole-word stores, no atomics, no memset); the sweep reads only those.
#include "oi_device.h"
#include "oi_internal.h"

#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define CG_TILE 128            // rows / columns of the output tile of one workgroup (4 waves, each 64 x 64 = 2 x 2 MFMA tiles)
#define CG_BK 32               // K chunk staged in LDS
#define CG_LD (CG_BK + 1)      // +1 float: conflict-free ds_read_b32 down a column
#define CG_INVALID 0xFFFFFFFFu // an entry without a row: past counts[q], or a doc id outside the shard
#define CG_MASK_BUDGET ((size_t)32 << 20) // bytes of mask workspace per slice of queries

// Four consecutive elements of a stored row, widened to f32 (bf16: bits << 16, exact).
template <bool BF16> __device__ __forceinline__ float4 cg_load4(const void *rows, uint64_t elem) {
    if (BF16) {
        const uint2 v = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint16_t *>(rows) + elem);
        return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xFFFF0000u), __uint_as_float(v.y << 16),
                           __uint_as_float(v.y & 0xFFFF0000u));
    }
    return *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(rows) + elem);
}

// Block b -> (query, tile): a query's T tiles are the blocks q % 8 + 8 (T (q / 8) + t), t < T -- all congruent mod 8, so with
// the round-robin placement of workgroups onto the 8 XCDs one query's row panels stay in one XCD's L2 while its tile
// columns re-read them.
template <bool BF16>
__global__ __launch_bounds__(256) void collapse_gram_kernel(const void *__restrict__ rows, uint64_t n_docs, uint32_t dim,
                                                            uint32_t doc_id_base, const uint32_t *__restrict__ docs,
                                                            const uint32_t *__restrict__ counts, uint32_t n_queries,
                                                            uint32_t depth, uint32_t n_tile_rows, float threshold,
                                                            uint64_t *__restrict__ mask) {
    OI_CLAIM_WHOLE_SIMD();
    __shared__ float sA[CG_TILE * CG_LD];
    __shared__ float sB[CG_TILE * CG_LD];
    __shared__ uint32_t sRowA[CG_TILE], sRowB[CG_TILE];
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t li = lane & 31, lh = lane >> 5;
    const uint32_t T = n_tile_rows * (n_tile_rows + 1) / 2;
    const uint32_t q = (blockIdx.x & 7u) + 8u * (blockIdx.x / (8u * T));
    if (q >= n_queries) return;
    uint32_t t = (blockIdx.x >> 3) % T, ti = 0;
    while (t > ti) { t -= ti + 1; ++ti; }
    const uint32_t tj = t; // tj <= ti: the lower triangle
    uint32_t cnt = counts[q];
    if (cnt > depth) cnt = depth;
    if (ti * CG_TILE >= cnt) return; // no entry of the list in this tile row: the sweep never reads these words

    // local rows of the two panels (A: the tile's rows i, B: its columns j)
    if (tid < 2 * CG_TILE) {
        const uint32_t e = (tid < CG_TILE ? ti : tj) * CG_TILE + (tid & (CG_TILE - 1));
        uint32_t local = CG_INVALID;
        if (e < cnt) {
            const uint32_t d = docs[(uint64_t)q * depth + e];
            if (d >= doc_id_base && (uint64_t)(d - doc_id_base) < n_docs) local = d - doc_id_base;
        }
        (tid < CG_TILE ? sRowA : sRowB)[tid & (CG_TILE - 1)] = local;
    }
    __syncthreads();

    // staging: thread -> float4 column cc of rows rr0 + 32 i of each panel.  Two register sets: while chunk c multiplies, chunks
    // c + 1 and c + 2 are on their way, so a gathered row (another page of a 30 GB corpus each: L2 and TLB misses) has two
    // chunks of matrix time -- about 8000 cycles -- to arrive.
    const uint32_t cc = (tid & 7u) << 2, rr0 = tid >> 3;
    // A load has no branch -- an entry without a row reads row 0 (the index has one), a column past dim reads column 0 -- and is
    // zeroed when it is stored, so the eight loads of a chunk issue back to back ahead of its matrix instructions.
    uint64_t oa[4], ob[4];
    bool va[4], vb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t a = sRowA[rr0 + 32u * i], b = sRowB[rr0 + 32u * i];
        va[i] = a != CG_INVALID; vb[i] = b != CG_INVALID;
        oa[i] = va[i] ? (uint64_t)a * dim : 0ull; ob[i] = vb[i] ? (uint64_t)b * dim : 0ull;
    }
    float4 pa[2][4], pb[2][4];
    auto fetch = [&](auto set, uint32_t k0) {
        constexpr int S = decltype(set)::value;
        const uint32_t col = k0 + cc < dim ? k0 + cc : 0u; // (dim is a multiple of 4: a float4 is inside or outside as a whole)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pa[S][i] = cg_load4<BF16>(rows, oa[i] + col);
            pb[S][i] = cg_load4<BF16>(rows, ob[i] + col);
        }
    };
    const uint32_t wr = w >> 1, wc = w & 1u;
    const bool upper = ti == tj && wc > wr; // the diagonal tile's strictly upper 64 x 64 quarter: no word of it is read
    f32x16 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;

    // one chunk: the set's registers into LDS, the set refilled with the chunk two ahead, the products of the staged chunk
    auto chunk = [&](auto set, uint32_t k0) {
        constexpr int S = decltype(set)::value;
        __syncthreads(); // the previous chunk's reads are done
        const bool in = k0 + cc < dim; // (the zero-filled K tail)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 a = in && va[i] ? pa[S][i] : make_float4(0.f, 0.f, 0.f, 0.f), b = in && vb[i] ? pb[S][i] : make_float4(0.f, 0.f, 0.f, 0.f);
            float *da = sA + (rr0 + 32u * i) * CG_LD + cc, *db = sB + (rr0 + 32u * i) * CG_LD + cc;
            da[0] = a.x; da[1] = a.y; da[2] = a.z; da[3] = a.w;
            db[0] = b.x; db[1] = b.y; db[2] = b.z; db[3] = b.w;
        }
        __syncthreads();
        fetch(set, k0 + 2 * CG_BK);
        if (!upper) {
#pragma unroll
            for (int kk = 0; kk < CG_BK; kk += 2) {
                const float a0 = sA[(64u * wr + li) * CG_LD + kk + lh], a1 = sA[(64u * wr + 32u + li) * CG_LD + kk + lh];
                const float b0 = sB[(64u * wc + li) * CG_LD + kk + lh], b1 = sB[(64u * wc + 32u + li) * CG_LD + kk + lh];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    };
    const std::integral_constant<int, 0> set0;
    const std::integral_constant<int, 1> set1;
    fetch(set0, 0u);
    fetch(set1, CG_BK);
    for (uint32_t k0 = 0; k0 < dim; k0 += 2 * CG_BK) {
        chunk(set0, k0);
        if (k0 + CG_BK >= dim) break; // (the same for every wave of the workgroup: the barriers stay matched)
        chunk(set1, k0 + CG_BK);
    }
    if (upper) return;

    // epilogue: the wave's 64 x 64 block is ONE mask word for each of its 64 rows.  acc[m][n][r] of lane (li, lh) is
    // (row 32 m + (r & 3) + 8 (r >> 2) + 4 lh, column 32 n + li): a ballot over the wave gives 32 columns of two rows.
    const bool cv0 = sRowB[64u * wc + li] != CG_INVALID, cv1 = sRowB[64u * wc + 32u + li] != CG_INVALID;
    const uint64_t row_valid = __ballot(sRowA[64u * wr + lane] != CG_INVALID);
    const uint32_t P = n_tile_rows * CG_TILE, W = P / 64u;
    uint64_t *mq = mask + (uint64_t)q * P * W;
    const uint32_t word = 2u * tj + wc;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t rl = 32u * m + (r & 3) + 8u * (r >> 2); // the row of lanes lh = 0; lh = 1: rl + 4
            const uint64_t b0 = __ballot(cv0 && acc[m][0][r] >= threshold), b1 = __ballot(cv1 && acc[m][1][r] >= threshold);
            uint64_t lo = (b0 & 0xFFFFFFFFull) | (b1 << 32), hi = (b0 >> 32) | (b1 & 0xFFFFFFFF00000000ull);
            if (!((row_valid >> rl) & 1ull)) lo = 0;
            if (!((row_valid >> (rl + 4u)) & 1ull)) hi = 0;
            const uint32_t i0 = ti * CG_TILE + 64u * wr + rl;
            if (lane == 0) mq[(uint64_t)i0 * W + word] = lo;
            if (lane == 32) mq[(uint64_t)(i0 + 4u) * W + word] = hi;
        }
}

// One wave per query.  Lane w < 16 holds word w of the kept set.  The mask rows of 64 entries at a time go through LDS (the
// next 64 rows are in registers meanwhile) and a row's words are read one step ahead, so the serial chain of a step is an AND,
// a ballot and a branch.  A collapsed entry only records its representative; the counts are taken in parallel afterwards.
// Integer work only.
#define CS_NOREP 0xFFFFu
__global__ __launch_bounds__(64) void collapse_sweep_kernel(const uint64_t *__restrict__ mask, uint32_t n_tile_rows,
                                                            const float *__restrict__ scores, const uint32_t *__restrict__ docs,
                                                            const uint32_t *__restrict__ counts, uint32_t depth, uint32_t k,
                                                            float *__restrict__ scores_out, uint32_t *__restrict__ docs_out,
                                                            uint32_t *__restrict__ counts_out, uint32_t *__restrict__ dup_out) {
    __shared__ uint64_t sM[64 * 16 + 16];    // (+ one row: the read-ahead of the last step stays inside)
    __shared__ uint32_t sDup[OI_MAX_DEPTH];  // by input entry: 1 + entries collapsed into it (kept entries only)
    __shared__ uint16_t sRep[OI_MAX_DEPTH];  // by input entry: the entry it collapsed into, CS_NOREP for a kept one
    __shared__ uint16_t sKept[OI_MAX_DEPTH]; // the kept entries, in rank order
    const uint32_t q = blockIdx.x, lane = threadIdx.x;
    const uint32_t P = n_tile_rows * CG_TILE, W = P / 64u;
    const uint64_t *mq = mask + (uint64_t)q * P * W;
    uint32_t cnt = counts[q];
    if (cnt > depth) cnt = depth;
    for (uint32_t x = lane; x < cnt; x += 64u) sDup[x] = 1u;
    for (uint32_t x = lane; x < 16u; x += 64u) sM[64u * 16u + x] = 0ull;
    // chunk c = rows 64 c .. 64 c + 63, words 0 .. c of each: lane -> elements x = lane + 64 j, row x >> 4, word x & 15
    uint64_t nx[16];
    auto fetch = [&](uint32_t c) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t x = lane + 64u * j, r = x >> 4, ww = x & 15u;
            nx[j] = ww <= c && 64u * c + r < cnt ? mq[(uint64_t)(64u * c + r) * W + ww] : 0ull;
        }
    };
    uint64_t kept = 0;
    uint32_t n_kept = 0;
    if (cnt) fetch(0);
    for (uint32_t c = 0; 64u * c < cnt; ++c) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 16; ++j) sM[lane + 64u * j] = nx[j];
        __syncthreads();
        if (64u * (c + 1) < cnt) fetch(c + 1);
        const uint32_t end = cnt - 64u * c < 64u ? cnt - 64u * c : 64u;
        const uint32_t col = lane & 15u;
        uint64_t row = sM[col];
        for (uint32_t r = 0; r < end; ++r) {
            const uint64_t next = sM[16u * (r + 1) + col];
            const uint64_t hit = lane <= c ? row & kept : 0ull; // (kept holds entries below this one only)
            const uint64_t lanes = __ballot(hit != 0ull);
            const uint32_t i = 64u * c + r;
            if (lanes == 0ull) {
                if (lane == c) kept |= 1ull << r;
                if (lane == 0) { sKept[n_kept] = (uint16_t)i; sRep[i] = CS_NOREP; }
                ++n_kept;
            } else { // the representative: the lowest set bit of the lowest lane that has one
                const uint32_t first = (uint32_t)__ffsll((unsigned long long)lanes) - 1u;
                if (lane == first) sRep[i] = (uint16_t)(64u * first + (uint32_t)__ffsll((unsigned long long)hit) - 1u);
            }
            row = next;
        }
    }
    __syncthreads();
    for (uint32_t x = lane; x < cnt; x += 64u) {
        const uint32_t rep = sRep[x];
        if (rep != CS_NOREP) atomicAdd(&sDup[rep], 1u);
    }
    __syncthreads();
    const uint32_t n_out = n_kept < k ? n_kept : k;
    for (uint32_t r = lane; r < n_out; r += 64u) {
        const uint32_t i = sKept[r];
        docs_out[(uint64_t)q * k + r] = docs[(uint64_t)q * depth + i];
        if (scores_out) scores_out[(uint64_t)q * k + r] = scores[(uint64_t)q * depth + i];
        if (dup_out) dup_out[(uint64_t)q * k + r] = sDup[i];
    }
    if (lane == 0) counts_out[q] = n_out;
}

// Device lists in, device lists out, asynchronous on the ctx stream.  The batch runs in slices of queries so that the mask
// workspace stays within CG_MASK_BUDGET whatever n_queries is.
int oi_launch_collapse(oi_index *idx, const float *d_scores, const uint32_t *d_docs, const uint32_t *d_counts, uint32_t n_queries,
                       uint32_t depth, float threshold, uint32_t k, float *scores_out, uint32_t *docs_out, uint32_t *counts_out,
                       uint32_t *dup_out) {
    oi_ctx *ctx = idx->ctx;
    OI_REQUIRE(depth >= 1 && depth <= OI_MAX_DEPTH && k >= 1 && k <= OI_MAX_DEPTH, "collapse: depth=%u / k=%u outside [1,%u]", depth, k,
               OI_MAX_DEPTH);
    OI_REQUIRE(idx->dim % 4 == 0 && idx->dim >= 4 && idx->dim <= OI_MAX_DIM, "collapse: dim=%u must be a multiple of 4 in [4,%u]",
               idx->dim, OI_MAX_DIM);
    OI_REQUIRE(idx->rows || idx->rows_bf16, "collapse: the index has no embeddings");
    if (n_queries == 0) return OI_OK;
    const uint32_t ntr = (depth + CG_TILE - 1) / CG_TILE, T = ntr * (ntr + 1) / 2;
    const size_t per_query = (size_t)ntr * CG_TILE * (ntr * CG_TILE / 64) * sizeof(uint64_t); // <= 128 KB
    uint32_t slice = (uint32_t)(CG_MASK_BUDGET / per_query);
    if (slice > n_queries) slice = n_queries;
    DevBuf &mb = ctx->buf("collapse_mask");
    OI_CHECK(mb.ensure(per_query * slice));
    uint64_t *mask = mb.as<uint64_t>();
    for (uint32_t q0 = 0; q0 < n_queries; q0 += slice) {
        const uint32_t nq = n_queries - q0 < slice ? n_queries - q0 : slice;
        const uint32_t *docs = d_docs + (size_t)q0 * depth, *counts = d_counts + q0;
        const uint32_t blocks = ((nq + 7u) / 8u) * 8u * T;
        {
            ProfScope ps(ctx, "collapse_gram");
            if (idx->rows_bf16)
                hipLaunchKernelGGL(collapse_gram_kernel<true>, dim3(blocks), dim3(256), 0, ctx->stream, (const void *)idx->rows_bf16,
                                   idx->n_docs, idx->dim, idx->doc_id_base, docs, counts, nq, depth, ntr, threshold, mask);
            else
                hipLaunchKernelGGL(collapse_gram_kernel<false>, dim3(blocks), dim3(256), 0, ctx->stream, (const void *)idx->rows,
                                   idx->n_docs, idx->dim, idx->doc_id_base, docs, counts, nq, depth, ntr, threshold, mask);
            OI_HIP_CHECK(hipGetLastError());
        }
        {
            ProfScope ps(ctx, "collapse_sweep");
            hipLaunchKernelGGL(collapse_sweep_kernel, dim3(nq), dim3(64), 0, ctx->stream, (const uint64_t *)mask, ntr,
                               d_scores ? d_scores + (size_t)q0 * depth : nullptr, docs, counts, depth, k,
                               scores_out ? scores_out + (size_t)q0 * k : nullptr, docs_out + (size_t)q0 * k, counts_out + q0,
                               dup_out ? dup_out + (size_t)q0 * k : nullptr);
            OI_HIP_CHECK(hipGetLastError());
        }
    }
    return OI_OK;
}
