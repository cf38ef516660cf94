// centroids.hip -- the update step of a clustering over the index: oi_label_sums, oi_centroids_from_sums and the
// small kernel oi_narratives_fit counts its moved rows with.  The assignment step is oi_similar_share (cosine_share.hip).
//
//   ls_sums_kernel        sums[c][k] += fix(x_dk), counts[c] += 1 over the rows d with labels[d] == c < n_clusters;
//                         fix(x) = (int64) rint(clamp(x with NaN -> 0, -1, 1) * 2^30).  Integers: the result is a function of the
//                         inputs alone, whatever the grid and the order of the atomics, and sums of document shards add.
//   cs_centroids_kernel   sums -> unit vectors in f64, one thread per cluster, every operation rounded once (no fma).
//   fm_moved_kernel       rows whose label changed between two assignment steps, and rows that have one.
//
// ls_sums_kernel.  A workgroup owns one SLICE of LS_SLICE floats of the dimension and walks row RANGES of LS_RANGE_ROWS rows
// (range = its lane among the slice's workgroups, then + the number of lanes).  It keeps int64 acc[n_clusters][LS_SLICE] in
// LDS and flushes the non-zero ones with 64-bit integer global atomics when its ranges are done, so the global atomics of a
// call are at most workgroups x n_clusters x LS_SLICE whatever the corpus size.  A wave reads the labels of a BLOCK of
// LS_BLOCK_ROWS rows, one per lane and one block ahead, and compacts the labelled rows (ballot, prefix count, one permute): a
// label >= n_clusters never reaches an address, and what a call costs follows the rows it has to read, not the rows there
// are.  A wave STEP is LS_STEP_ROWS labelled rows of the block: 16 lanes per row, a float4 (or four bf16) per lane; the loads
// of LS_UNROLL steps are issued together, then added with 64-bit LDS atomics.  When the rows of a step carry one label the
// four row groups are added in registers first and one group does the atomics: equal addresses in
// one instruction serialise.  The slot of element (k4, j) of cluster c is (j * 16 + k4) ^ ((c & 1) << 4): the 16 lanes of a
// row touch 128 contiguous bytes, and rows of odd and even clusters fall on different halves of the banks.
// The slice-0 workgroups count the rows.  The outputs are zeroed by the launcher.
#include "oi_internal.h"

#include <algorithm>

// ------------------------------------------------------------------ shape constants (tests/test_centroids_abi.py reads them)
constexpr uint32_t LS_SLICE = 64;          // floats of the dimension per workgroup: 256 B per row and slice
constexpr uint32_t LS_STEP_ROWS = 4;       // labelled rows per wave step (one load instruction): 64 lanes / (LS_SLICE / 4)
constexpr uint32_t LS_UNROLL = 4;          // wave steps whose row loads are in flight together
constexpr uint32_t LS_THREADS = 1024;      // 16 waves per workgroup
constexpr uint32_t LS_BLOCK_ROWS = 64;     // rows whose labels a wave reads at once, one per lane
constexpr uint32_t LS_WG_STEP_ROWS = 1024; // rows a workgroup covers per trip: waves x LS_BLOCK_ROWS
constexpr uint32_t LS_RANGE_ROWS = 2048;   // rows per range
// (one LDS layout for every cluster count: 32.5 KB at 64 clusters, 130 KB at OI_MAX_CENTROIDS)
static_assert(LS_STEP_ROWS * (LS_SLICE / 4) == 64, "a wave step is one wave instruction");
static_assert(LS_WG_STEP_ROWS == LS_THREADS / 64 * LS_BLOCK_ROWS, "the workgroup trip");
static_assert(LS_RANGE_ROWS % LS_WG_STEP_ROWS == 0 && LS_BLOCK_ROWS % (LS_UNROLL * LS_STEP_ROWS) == 0, "a range is whole trips of whole blocks");
static_assert((size_t)OI_MAX_CENTROIDS * (LS_SLICE + 1) * 8 <= 160 * 1024, "the accumulators fit the CU's LDS");

#define LS_NO_LABEL 0xFFFFFFFFu

__device__ __forceinline__ int ls_fix(float x) {
    float v = x == x ? x : 0.f;
    v = fminf(fmaxf(v, -1.f), 1.f);
    return (int)rintf(v * 1073741824.f); // exact product, |result| <= 2^30
}

__device__ __forceinline__ uint32_t ls_slot(uint32_t c, uint32_t j, uint32_t k4) { return (j * 16u + k4) ^ ((c & 1u) << 4); }

// ADDS = false exists in -DOI_ABLATION builds only (OI_LS_NO_ADDS=1: "timings only, results wrong by construction"): the
// labels, the row loads and fix() stay, the LDS atomics go -- each lane keeps a private sum and adds it once at the end.
template <bool BF16, bool ADDS>
__global__ __launch_bounds__(LS_THREADS) void ls_sums_kernel(const void *__restrict__ rows_v, const uint32_t *__restrict__ labels, uint64_t n,
                                                             uint32_t dim, uint32_t K, uint32_t n_slices, uint64_t n_ranges,
                                                             unsigned long long *__restrict__ sums, unsigned long long *__restrict__ counts) {
    extern __shared__ unsigned long long ls_acc[]; // [K][LS_SLICE] sums, then [K] row counts
    unsigned long long *cnt = ls_acc + (size_t)K * LS_SLICE;
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < K * (LS_SLICE + 1u); i += LS_THREADS) ls_acc[i] = 0ull;
    __syncthreads();

    const uint32_t slice = blockIdx.x % n_slices, first = blockIdx.x / n_slices, lanes = gridDim.x / n_slices;
    const uint32_t lane = tid & 63u, wave = tid >> 6, g = lane >> 4, k4 = lane & 15u;
    const uint32_t k = slice * LS_SLICE + k4 * 4u;
    const bool kin = k < dim; // dim is a multiple of 4: the lane's four elements are in or out together
    const bool counting = slice == 0u;
    long long sink = 0;

    // The wave's trips: LS_RANGE_ROWS / LS_WG_STEP_ROWS per range of the workgroup, one BLOCK of LS_BLOCK_ROWS rows each.  A lane
    // reads one label of the block (the next block's before this one is worked on); the labelled rows are compacted with a
    // ballot and one permute, so a step never spends a row group on an unlabelled row and a block without labels costs one
    // coalesced load.  A trip past the end reads nothing: its rows are >= n.
    constexpr uint32_t TRIPS = LS_RANGE_ROWS / LS_WG_STEP_ROWS;
    const uint64_t my_ranges = first < n_ranges ? (n_ranges - first + lanes - 1) / lanes : 0, n_trips = my_ranges * TRIPS;
    auto trip_base = [&](uint64_t j) -> uint64_t {
        if (j >= n_trips) return n;
        return (first + (j / TRIPS) * lanes) * LS_RANGE_ROWS + (j % TRIPS) * LS_WG_STEP_ROWS + wave * LS_BLOCK_ROWS;
    };
    auto load_label = [&](uint64_t base) -> uint32_t { return base + lane < n ? labels[base + lane] : LS_NO_LABEL; };

    uint64_t base_next = trip_base(0);
    uint32_t lab_next = load_label(base_next);
    for (uint64_t j = 0; j < n_trips; ++j) {
        const uint64_t base = base_next;
        const uint32_t lab = lab_next;
        base_next = trip_base(j + 1);
        lab_next = load_label(base_next);
        const unsigned long long mask = __ballot(lab < K);
        if (mask == 0ull) continue; // (wave-uniform)
        const uint32_t n_valid = (uint32_t)__popcll(mask);
        const unsigned long long below = (1ull << lane) - 1ull;
        // position of this lane's row among the block's rows, the labelled ones first, in row order
        const uint32_t pos = lab < K ? (uint32_t)__popcll(mask & below) : n_valid + (uint32_t)__popcll(~mask & below);
        const uint32_t src = (uint32_t)__builtin_amdgcn_ds_permute((int)(pos * 4u), (int)lane); // src[p] = the lane whose row is p-th
        for (uint32_t s0 = 0; s0 < n_valid; s0 += LS_UNROLL * LS_STEP_ROWS) {
            uint32_t L[LS_UNROLL];
            uint4 x[LS_UNROLL]; // the raw 16 (8) bytes of the lane's four elements; zeros where the lane has none
#pragma unroll
            for (uint32_t u = 0; u < LS_UNROLL; ++u) {
                const uint32_t p = s0 + u * LS_STEP_ROWS + g; // <= 63
                const uint32_t sl = (uint32_t)__shfl((int)src, (int)p);
                const uint32_t l = (uint32_t)__shfl((int)lab, (int)sl);
                L[u] = p < n_valid ? l : LS_NO_LABEL;
                x[u] = make_uint4(0u, 0u, 0u, 0u);
                if (L[u] < K && kin) { // (a label < K was read, so its row is < n)
                    const uint64_t row = base + sl;
                    if (BF16) {
                        const uint2 w = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint16_t *>(rows_v) + row * dim + k);
                        x[u].x = w.x;
                        x[u].y = w.y;
                    } else {
                        x[u] = *reinterpret_cast<const uint4 *>(reinterpret_cast<const float *>(rows_v) + row * dim + k);
                    }
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < LS_UNROLL; ++u) {
                if (s0 + u * LS_STEP_ROWS >= n_valid) break; // (wave-uniform)
                const uint32_t Lu = L[u];
                const bool valid = Lu < K;
                int f[4]; // (lanes that hold no element carry zeros)
                if (BF16) {
                    f[0] = ls_fix(__uint_as_float(x[u].x << 16));
                    f[1] = ls_fix(__uint_as_float(x[u].x & 0xFFFF0000u));
                    f[2] = ls_fix(__uint_as_float(x[u].y << 16));
                    f[3] = ls_fix(__uint_as_float(x[u].y & 0xFFFF0000u));
                } else {
                    f[0] = ls_fix(__uint_as_float(x[u].x));
                    f[1] = ls_fix(__uint_as_float(x[u].y));
                    f[2] = ls_fix(__uint_as_float(x[u].z));
                    f[3] = ls_fix(__uint_as_float(x[u].w));
                }
                if (!ADDS) {
                    sink += (long long)f[0] + f[1] + f[2] + f[3];
                    continue;
                }
                const uint32_t L0 = (uint32_t)__shfl((int)Lu, 0);
                if (__all(Lu == L0)) { // one label on the step's four rows (wave-uniform branch; L0 < K: row group 0 is labelled)
                    long long s[4];
#pragma unroll
                    for (uint32_t e = 0; e < 4; ++e) {
                        s[e] = (long long)f[e] + (long long)__shfl_xor(f[e], 16);
                        s[e] += __shfl_xor(s[e], 32);
                    }
                    if (g == 0u && kin) {
#pragma unroll
                        for (uint32_t e = 0; e < 4; ++e) atomicAdd(&ls_acc[L0 * LS_SLICE + ls_slot(L0, e, k4)], (unsigned long long)s[e]);
                    }
                    if (counting && lane == 0u) atomicAdd(&cnt[L0], (unsigned long long)LS_STEP_ROWS);
                } else {
                    if (valid && kin) {
#pragma unroll
                        for (uint32_t e = 0; e < 4; ++e) atomicAdd(&ls_acc[Lu * LS_SLICE + ls_slot(Lu, e, k4)], (unsigned long long)(long long)f[e]);
                    }
                    if (counting && valid && k4 == 0u) atomicAdd(&cnt[Lu], 1ull);
                }
            }
        }
    }
    if (!ADDS) atomicAdd(&ls_acc[lane], (unsigned long long)sink);
    __syncthreads();
    // the flush: thread -> (cluster, element of the slice), consecutive lanes on consecutive elements of sums
    for (uint32_t i = tid; i < K * LS_SLICE; i += LS_THREADS) {
        const uint32_t c = i / LS_SLICE, kk = i % LS_SLICE, ke = slice * LS_SLICE + kk;
        const unsigned long long v = ls_acc[c * LS_SLICE + ls_slot(c, kk & 3u, kk >> 2)];
        if (v != 0ull && ke < dim) atomicAdd(sums + (size_t)c * dim + ke, v);
    }
    if (counting)
        for (uint32_t c = tid; c < K; c += LS_THREADS)
            if (cnt[c] != 0ull) atomicAdd(counts + c, cnt[c]);
}

// One thread per cluster.  v_k = sums * 2^-30 (exact once the sum is a double); n2 accumulated from +0.0 in ascending k, one
// rounded multiply and one rounded add per element; out = (float)(v_k / sqrt(n2)).  An empty cluster (counts == 0 or
// n2 == 0) keeps previous[c] (zeros without one).  out may alias previous: a thread reads element k before it writes it, and
// no other thread touches the cluster.
__global__ __launch_bounds__(64) void cs_centroids_kernel(const long long *__restrict__ sums, const unsigned long long *__restrict__ counts,
                                                          const float *previous, uint32_t K, uint32_t dim, float *out) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= K) return;
    const long long *s = sums + (size_t)c * dim;
    float *o = out + (size_t)c * dim;
    const float *p = previous ? previous + (size_t)c * dim : nullptr;
    double n2 = 0.0;
    if (counts[c] != 0ull)
        for (uint32_t k = 0; k < dim; ++k) {
            const double v = __dmul_rn((double)s[k], 0x1p-30);
            n2 = __dadd_rn(n2, __dmul_rn(v, v));
        }
    if (n2 == 0.0) { // (counts[c] == 0 lands here too)
        for (uint32_t k = 0; k < dim; ++k) o[k] = p ? p[k] : 0.f;
        return;
    }
    const double r = __dsqrt_rn(n2);
    for (uint32_t k = 0; k < dim; ++k) o[k] = (float)__ddiv_rn(__dmul_rn((double)s[k], 0x1p-30), r);
}

// out[0] += rows with cur != prev, out[1] += rows with a label (cur != 0xFFFFFFFF); out is zeroed by the launcher.
__global__ __launch_bounds__(256) void fm_moved_kernel(const uint32_t *__restrict__ cur, const uint32_t *__restrict__ prev, uint64_t n,
                                                       unsigned long long *__restrict__ out) {
    __shared__ unsigned long long part[2];
    if (threadIdx.x < 2u) part[threadIdx.x] = 0ull;
    __syncthreads();
    uint32_t moved = 0, assigned = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = cur[i];
        moved += l != prev[i];
        assigned += l != LS_NO_LABEL;
    }
#pragma unroll
    for (uint32_t o = 32; o > 0; o >>= 1) {
        moved += __shfl_xor(moved, o);
        assigned += __shfl_xor(assigned, o);
    }
    if ((threadIdx.x & 63u) == 0u) {
        if (moved) atomicAdd(&part[0], (unsigned long long)moved);
        if (assigned) atomicAdd(&part[1], (unsigned long long)assigned);
    }
    __syncthreads();
    if (threadIdx.x < 2u && part[threadIdx.x] != 0ull) atomicAdd(out + threadIdx.x, part[threadIdx.x]);
}

// ------------------------------------------------------------------ host
// Device labels in, device sums [n_clusters][dim] and counts [n_clusters] out (zeroed here); asynchronous on the ctx stream.
int oi_launch_label_sums(oi_index *idx, const uint32_t *d_labels, uint32_t K, int64_t *d_sums, uint64_t *d_counts) {
    oi_ctx *ctx = idx->ctx;
    hipStream_t st = ctx->stream;
    const uint32_t dim = idx->dim;
    const uint64_t n = idx->n_docs;
    ProfScope ps(ctx, "label_sums");
    OI_HIP_CHECK(hipMemsetAsync(d_sums, 0, sizeof(int64_t) * (size_t)K * dim, st));
    OI_HIP_CHECK(hipMemsetAsync(d_counts, 0, sizeof(uint64_t) * (size_t)K, st));
    if (n == 0) return OI_OK;
    const uint32_t n_slices = (dim + LS_SLICE - 1) / LS_SLICE;
    const uint64_t n_ranges = (n + LS_RANGE_ROWS - 1) / LS_RANGE_ROWS;
    const size_t lds = sizeof(uint64_t) * (size_t)K * (LS_SLICE + 1);
    // as many workgroups as are resident at once (LDS and the 2048 thread slots of a CU decide), split among the slices
    const uint32_t per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(2, (size_t)160 * 1024 / lds));
    const uint32_t lanes = (uint32_t)std::min<uint64_t>(n_ranges, std::max<uint32_t>(1, (uint32_t)ctx->num_cus * per_cu / n_slices));
    const bool bf16 = idx->rows_bf16 != nullptr;
    const void *rows = bf16 ? (const void *)idx->rows_bf16 : (const void *)idx->rows;
    auto launch = [&](auto kernel) -> int {
        OI_CHECK(oi_dyn_lds(ctx, (const void *)kernel, sizeof(uint64_t) * (size_t)OI_MAX_CENTROIDS * (LS_SLICE + 1)));
        hipLaunchKernelGGL(kernel, dim3(lanes * n_slices), dim3(LS_THREADS), lds, st, rows, d_labels, n, dim, K, n_slices, n_ranges,
                           reinterpret_cast<unsigned long long *>(d_sums), reinterpret_cast<unsigned long long *>(d_counts));
        return OI_OK;
    };
#ifdef OI_ABLATION
    const char *no_adds = oi_ablation_env("OI_LS_NO_ADDS");
    if (no_adds && no_adds[0] == '1') {
        OI_CHECK(bf16 ? launch(ls_sums_kernel<true, false>) : launch(ls_sums_kernel<false, false>));
        OI_HIP_CHECK(hipGetLastError());
        return OI_OK;
    }
#endif
    OI_CHECK(bf16 ? launch(ls_sums_kernel<true, true>) : launch(ls_sums_kernel<false, true>));
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// Device sums / counts / previous (may be null, may be d_out) in, device centroids out; asynchronous on the ctx stream.
int oi_launch_centroids_from_sums(oi_ctx *ctx, const int64_t *d_sums, const uint64_t *d_counts, const float *d_previous, uint32_t K,
                                  uint32_t dim, float *d_out) {
    ProfScope ps(ctx, "centroids");
    hipLaunchKernelGGL(cs_centroids_kernel, dim3((K + 63) / 64), dim3(64), 0, ctx->stream, reinterpret_cast<const long long *>(d_sums),
                       reinterpret_cast<const unsigned long long *>(d_counts), d_previous, K, dim, d_out);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// d_out[0] = rows with d_cur != d_prev, d_out[1] = rows with a label; asynchronous on the ctx stream.
int oi_launch_fit_moved(oi_ctx *ctx, const uint32_t *d_cur, const uint32_t *d_prev, uint64_t n, uint64_t *d_out) {
    ProfScope ps(ctx, "fit_moved");
    OI_HIP_CHECK(hipMemsetAsync(d_out, 0, 2 * sizeof(uint64_t), ctx->stream));
    if (n == 0) return OI_OK;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->num_cus * 8);
    hipLaunchKernelGGL(fm_moved_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_cur, d_prev, n, reinterpret_cast<unsigned long long *>(d_out));
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}
