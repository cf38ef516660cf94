// seeds.hip -- oi_narratives_seed: greedy k-means++ (or farthest-first) seeding of a clustering over the index.
// The definition is the header's; what follows is how it runs.  A call is  init, pick(0), then score(j), pick(j) for
// j = 1 .. n_clusters: two launches per seed, no atomics, no host synchronise between them.
//
//   ns_init_kernel    eligibility (filter, bucket) evaluated ONCE: w[d] = 0xFFFFFFFF (eligible, "no seed yet") or 0, and the
//                     eligible rows of every range.  Every later kernel skips a row with w == 0 without reading it.
//   ns_score_kernel   the stream of the rows.  Pass 1 scores p_0 alone; pass j >= 2 scores the L candidates of seed j - 1.  A
//                     workgroup walks RANGES of NS_RANGE_ROWS consecutive rows (range = its number, then + the grid), a wave a
//                     quarter of the range in BLOCKS of 64 rows, one w per lane.  The commit of the previous pass is fused in:
//                     w = min(w, cw[t*_prev]) first, t*_prev read from the state.  The live rows of a block are taken NS_UNROLL
//                     at a time: their loads are issued together (NV float4 per lane and row, as vo_exact_kernel holds a row),
//                     then each candidate's float4 is read from LDS once and enters the chains of all of them.  The f32 value
//                     is the family's: vo_load_row4, vo_chain4 in ascending j, oi_wave_sum.  The sim goes back to the row's lane,
//                     which takes wc = weight(sim) once per block; cw[t][d] = wc (L > 1) or w[d] = min(w, wc) (L == 1);
//                     part[t][range] = sum of min(w, wc_t)
//                     over the range, a plain store: pot_t of this pass and the range sums the next draw scans.  Farthest-first
//                     also keeps key[range] = max over the range of (new w << 32 | ~row).
//   ns_pick_kernel    one workgroup.  Reduces part to pot_t, takes t* (ties to the smallest t), writes seed j - 1 (the staged
//                     candidate t*, the stored row as f32), found, potential; raises `done` when W == 0 -- every later launch of
//                     the call then exits at once.  Else it draws the next targets r_t = mulhi64(u(j, t), W) and locates each:
//                     a scan over the range sums part[t*], then over the rows of that range (min(w, cw[t*]); before seed 0: the
//                     eligible rows, one each).  Farthest-first takes the largest key instead.  Then it stages the candidates'
//                     rows as f32 for the next pass.
#include "oi_volume.h"

// ------------------------------------------------------------------ shape constants (tests/test_seed_abi.py reads them)
constexpr uint32_t NS_RANGE_ROWS = 2048;  // rows per range: one partial sum per candidate and range
constexpr uint32_t NS_THREADS = 256;      // ns_init / ns_score: 4 waves, a quarter of the range each
constexpr uint32_t NS_BLOCK_ROWS = 64;    // rows whose w a wave reads at once, one per lane
constexpr uint32_t NS_UNROLL = 4;         // live rows whose loads are in flight together, and that share a candidate read
constexpr uint32_t NS_PICK_THREADS = 1024;
constexpr uint32_t NS_WAVE_ROWS = NS_RANGE_ROWS / (NS_THREADS / 64);
static_assert(NS_WAVE_ROWS % NS_BLOCK_ROWS == 0, "a wave's share of a range is whole blocks");
static_assert(OI_MAX_SEED_TRIALS == 8u && OI_MAX_DIM <= 1024u, "the staged candidates are at most 8 x 1024 floats: 32 KB of LDS");
// a lane adds at most NS_WAVE_ROWS / 64 weights of at most 2^21, a wave NS_WAVE_ROWS of them: both sums fit 32 bits
static_assert((uint64_t)NS_WAVE_ROWS << 21 < (1ull << 32), "the wave's partial sums are 32-bit");

#define NS_NONE 0xFFFFFFFFu

// the state of a call, zeroed by it; the first 24 bytes are the oi_seed_info the caller reads
struct NsState {
    uint32_t found, reserved;
    uint64_t eligible, potential;
    uint32_t done;                          // W == 0 (or no eligible row): every later launch exits at once
    uint32_t t_prev;                        // t* of the last pass when its commit is still to be applied, else NS_NONE
    uint32_t cand_row[OI_MAX_SEED_TRIALS];  // the rows of the staged candidates
};
static_assert(sizeof(NsState) == 64 && sizeof(oi_seed_info) == 24 && sizeof(oi_seed_spec) == 32, "layouts of the header");

// weight(s) = (uint32) rintf(min(max(1.0f - s, 0), 2) * 2^20), weight(NaN) = 0: one rounded subtract, an exact scale
__device__ __forceinline__ uint32_t ns_weight(float s) {
    if (!(s == s)) return 0u;
    const float x = fminf(fmaxf(__fsub_rn(1.0f, s), 0.f), 2.f);
    return (uint32_t)rintf(x * 1048576.f);
}

__device__ __forceinline__ uint64_t ns_splitmix(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// ------------------------------------------------------------------ init
__global__ __launch_bounds__(NS_THREADS) void ns_init_kernel(const uint2 *__restrict__ attrs, uint4 filt, uint32_t has_filt, uint32_t origin,
                                                             uint32_t width, uint32_t n_buckets, uint64_t n, uint64_t n_ranges,
                                                             uint32_t *__restrict__ w, unsigned long long *__restrict__ part) {
    __shared__ uint32_t red[NS_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint64_t range = blockIdx.x; range < n_ranges; range += gridDim.x) {
        uint32_t count = 0;
        for (uint32_t i = tid; i < NS_RANGE_ROWS; i += NS_THREADS) {
            const uint64_t d = range * NS_RANGE_ROWS + i;
            if (d >= n) break;
            bool ok = true;
            if (attrs) {
                const uint2 at = attrs[d];
                uint32_t b = 0;
                ok = (!has_filt || oi_doc_passes(filt, at)) && vo_bucket(at.y, origin, width, n_buckets, &b);
            }
            w[d] = ok ? NS_NONE : 0u;
            count += ok;
        }
        count = oi_wave_sum(count);
        if (lane == 0u) red[wave] = count;
        __syncthreads();
        if (tid == 0u) {
            uint32_t s = 0;
            for (uint32_t k = 0; k < NS_THREADS / 64; ++k) s += red[k];
            part[range] = s;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ the stream
// LT: the candidates the instance has room for (1, 2, 4, 8); L <= LT of them are staged.  FAR: farthest-first (LT == 1).
// CHAIN = false exists in -DOI_ABLATION builds only (OI_NS_NO_CHAIN=1: "timings only, results wrong by construction"): the
// w reads, the row loads and every store stay, the candidate reads, the chains and the wave sums go.
template <int NV, bool BF16, int LT, bool FAR, bool CHAIN>
__global__ __launch_bounds__(NS_THREADS) void ns_score_kernel(const void *__restrict__ rows, uint64_t n, uint32_t dim, uint64_t n_ranges,
                                                              uint32_t L, const NsState *__restrict__ state, const float *__restrict__ cand,
                                                              uint32_t *w, uint32_t *cw, unsigned long long *__restrict__ part,
                                                              unsigned long long *__restrict__ far_key) {
    static_assert(!FAR || LT == 1, "farthest-first scores one vector per pass");
    extern __shared__ float4 ns_cand[]; // [L][dim / 4]
    __shared__ unsigned long long red[NS_THREADS / 64][LT + 1];
    if (state->done != 0u) return; // (uniform over the grid)
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t nvec = dim >> 2;
    for (uint32_t i = tid; i < L * nvec; i += NS_THREADS) ns_cand[i] = reinterpret_cast<const float4 *>(cand)[i];
    uint32_t crow[LT];
#pragma unroll
    for (int t = 0; t < LT; ++t) crow[t] = (uint32_t)t < L ? state->cand_row[t] : NS_NONE;
    const uint32_t t_prev = state->t_prev;
    const size_t row_bytes = (size_t)dim * (BF16 ? 2 : 4);
    __syncthreads();

    for (uint64_t range = blockIdx.x; range < n_ranges; range += gridDim.x) {
        uint32_t acc[LT];
#pragma unroll
        for (int t = 0; t < LT; ++t) acc[t] = 0u;
        unsigned long long key = 0ull;
        for (uint32_t blk = 0; blk < NS_WAVE_ROWS / NS_BLOCK_ROWS; ++blk) {
            const uint64_t base = range * NS_RANGE_ROWS + (uint64_t)wave * NS_WAVE_ROWS + (uint64_t)blk * NS_BLOCK_ROWS;
            if (base >= n) break; // (wave-uniform)
            const uint64_t d = base + lane;
            const bool in = d < n;
            uint32_t wv = in ? w[d] : 0u;
            if (t_prev != NS_NONE && in) { // the commit of the previous pass
                const uint32_t c = cw[(uint64_t)t_prev * n + d];
                wv = wv < c ? wv : c;
            }
            float sim[LT]; // sim(c_t, this lane's row); NaN (weight 0) for a row that is not live
#pragma unroll
            for (int t = 0; t < LT; ++t) sim[t] = __builtin_nanf("");
            unsigned long long m = __ballot(wv != 0u);
            while (m != 0ull) { // (wave-uniform) the next NS_UNROLL live rows of the block
                uint32_t rl[NS_UNROLL];
                float4 x[NS_UNROLL][NV];
#pragma unroll
                for (uint32_t u = 0; u < NS_UNROLL; ++u) {
                    rl[u] = 64u;
                    if (m != 0ull) {
                        rl[u] = (uint32_t)__builtin_ctzll(m);
                        m &= m - 1ull;
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < NS_UNROLL; ++u) {
                    const void *xr = reinterpret_cast<const unsigned char *>(rows) + (base + (rl[u] & 63u)) * row_bytes;
#pragma unroll
                    for (int j = 0; j < NV; ++j) {
                        const uint32_t v = lane + 64u * j;
                        x[u][j] = (rl[u] < 64u && v < nvec) ? vo_load_row4<BF16>(xr, v) : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                }
                float a[NS_UNROLL][LT];
#pragma unroll
                for (uint32_t u = 0; u < NS_UNROLL; ++u)
#pragma unroll
                    for (int t = 0; t < LT; ++t) a[u][t] = 0.f;
                if (!CHAIN) { // (every loaded value is used, so the loads stay)
#pragma unroll
                    for (uint32_t u = 0; u < NS_UNROLL; ++u) {
                        float f = 0.f;
#pragma unroll
                        for (int j = 0; j < NV; ++j) f += (x[u][j].x + x[u][j].y) + (x[u][j].z + x[u][j].w);
#pragma unroll
                        for (int t = 0; t < LT; ++t) a[u][t] = f;
                    }
                }
                if (CHAIN) {
#pragma unroll
                    for (int t = 0; t < LT; ++t) {
                        if ((uint32_t)t >= L) break; // (uniform)
#pragma unroll
                        for (int j = 0; j < NV; ++j) {
                            const uint32_t v = lane + 64u * j;
                            if (v < nvec) {
                                const float4 y = ns_cand[(uint32_t)t * nvec + v];
#pragma unroll
                                for (uint32_t u = 0; u < NS_UNROLL; ++u) a[u][t] = vo_chain4(x[u][j], y, a[u][t]);
                            }
                        }
                    }
                }
#pragma unroll
                for (uint32_t u = 0; u < NS_UNROLL; ++u) {
                    if (rl[u] >= 64u) break; // (wave-uniform)
#pragma unroll
                    for (int t = 0; t < LT; ++t) {
                        if ((uint32_t)t >= L) break;
                        const float s = CHAIN ? oi_wave_sum(a[u][t]) : a[u][t]; // (the same in every lane)
                        if (lane == rl[u]) sim[t] = s;
                    }
                }
            }
            uint32_t mine[LT]; // wc_t of this lane's row, once per lane: wc_t[c_t] = 0
#pragma unroll
            for (int t = 0; t < LT; ++t) mine[t] = d == (uint64_t)crow[t] ? 0u : ns_weight(sim[t]);
            if (LT > 1) {
                if (t_prev != NS_NONE && in) w[d] = wv;
#pragma unroll
                for (int t = 0; t < LT; ++t) {
                    if ((uint32_t)t >= L) break;
                    if (in) cw[(uint64_t)t * n + d] = mine[t];
                    acc[t] += wv < mine[t] ? wv : mine[t];
                }
            } else {
                const uint32_t nw = wv < mine[0] ? wv : mine[0];
                if (in) w[d] = nw;
                acc[0] += nw;
                if (FAR && in) {
                    const unsigned long long k = ((unsigned long long)nw << 32) | (uint32_t)~(uint32_t)d;
                    key = k > key ? k : key;
                }
            }
        }
#pragma unroll
        for (int t = 0; t < LT; ++t) {
            const uint32_t s = oi_wave_sum(acc[t]);
            if (lane == 0u) red[wave][t] = s;
        }
        if (FAR) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long k = __shfl_xor(key, o, OI_WAVE);
                key = k > key ? k : key;
            }
            if (lane == 0u) red[wave][LT] = key;
        }
        __syncthreads();
        if (tid < L) {
            unsigned long long s = 0ull;
            for (uint32_t k = 0; k < NS_THREADS / 64; ++k) s += red[k][tid];
            part[(uint64_t)tid * n_ranges + range] = s;
        }
        if (FAR && tid == 64u) {
            unsigned long long k = 0ull;
            for (uint32_t i = 0; i < NS_THREADS / 64; ++i) k = red[i][LT] > k ? red[i][LT] : k;
            far_key[range] = k;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ the pick
__device__ __forceinline__ unsigned long long ns_block_sum(unsigned long long v, unsigned long long *sh) {
    const uint32_t tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (uint32_t s = NS_PICK_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const unsigned long long r = sh[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ unsigned long long ns_block_max(unsigned long long v, unsigned long long *sh) {
    const uint32_t tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (uint32_t s = NS_PICK_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] = sh[tid + s] > sh[tid] ? sh[tid + s] : sh[tid];
        __syncthreads();
    }
    const unsigned long long r = sh[0];
    __syncthreads();
    return r;
}
// The smallest i < count whose inclusive prefix sum of f exceeds target, and target minus the sum before i.  A thread takes a
// contiguous chunk; the chunk sums are scanned over the workgroup; the one thread whose chunk holds the target walks it.
// (target < the total, by the caller's construction; were it not, the answer is {0, 0}.)
template <class F>
__device__ __forceinline__ void ns_locate(F f, uint64_t count, unsigned long long target, unsigned long long *sh, unsigned long long *res,
                                          uint64_t *index, unsigned long long *rest) {
    const uint32_t tid = threadIdx.x;
    const uint64_t chunk = (count + NS_PICK_THREADS - 1) / NS_PICK_THREADS;
    const uint64_t b = tid * chunk < count ? tid * chunk : count, e = b + chunk < count ? b + chunk : count;
    unsigned long long s = 0ull;
    for (uint64_t i = b; i < e; ++i) s += f(i);
    if (tid == 0u) { res[0] = 0ull; res[1] = 0ull; }
    sh[tid] = s;
    __syncthreads();
    for (uint32_t off = 1; off < NS_PICK_THREADS; off <<= 1) {
        const unsigned long long t = tid >= off ? sh[tid - off] : 0ull;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const unsigned long long incl = sh[tid], excl = incl - s;
    if (target >= excl && target < incl) {
        unsigned long long run = excl;
        for (uint64_t i = b; i < e; ++i) {
            const unsigned long long v = f(i);
            if (target < run + v) { res[0] = i; res[1] = target - run; break; }
            run += v;
        }
    }
    __syncthreads();
    *index = res[0];
    *rest = res[1];
    __syncthreads();
}

// step j = 0: behind ns_init_kernel (part[0] holds the ranges' eligible rows).  j >= 1: behind pass j, which scored L_prev
// vectors.  L_next: the candidates to stage for pass j + 1 (0 behind the last pass).
__global__ __launch_bounds__(NS_PICK_THREADS) void ns_pick_kernel(const void *__restrict__ rows, uint32_t bf16, uint64_t n, uint32_t dim,
                                                                  uint64_t n_ranges, uint32_t step, uint32_t L_prev, uint32_t L_next,
                                                                  uint32_t method, uint64_t rng_seed, NsState *state, const uint32_t *w,
                                                                  const uint32_t *cw, const unsigned long long *__restrict__ part,
                                                                  const unsigned long long *__restrict__ far_key, float *cand,
                                                                  float *seeds_out, uint32_t *rows_out) {
    __shared__ unsigned long long sh[NS_PICK_THREADS];
    __shared__ unsigned long long res[2];
    __shared__ uint32_t gate;
    const uint32_t tid = threadIdx.x;
    if (tid == 0u) gate = state->done;
    __syncthreads();
    if (gate != 0u) return;

    // pot_t of the pass behind us, t* and W
    uint32_t tstar = 0;
    unsigned long long W = 0ull;
    for (uint32_t t = 0; t < (step ? L_prev : 1u); ++t) {
        unsigned long long s = 0ull;
        for (uint64_t r = tid; r < n_ranges; r += NS_PICK_THREADS) s += part[(uint64_t)t * n_ranges + r];
        s = ns_block_sum(s, sh);
        if (t == 0u || s < W) { W = s; tstar = t; } // (ties keep the smallest t)
    }
    if (step >= 1u) { // seed step - 1 is candidate t* of the pass
        const uint32_t p = state->cand_row[tstar];
        for (uint32_t k = tid; k < dim; k += NS_PICK_THREADS) seeds_out[(uint64_t)(step - 1u) * dim + k] = cand[(uint64_t)tstar * dim + k];
        if (tid == 0u && rows_out) rows_out[step - 1u] = p;
    }
    __syncthreads(); // (cand and cand_row are overwritten below)
    if (tid == 0u) {
        state->found = step;
        if (step == 0u) state->eligible = W;
        else state->potential = W;
        state->t_prev = (step && L_prev > 1u) ? tstar : NS_NONE;
        if (L_next != 0u && W == 0ull) state->done = 1u;
    }
    if (L_next == 0u || W == 0ull) return;

    const bool pending = step && L_prev > 1u; // w is still to take min(w, cw[t*])
    for (uint32_t t = 0; t < L_next; ++t) {
        uint64_t row;
        if (method == OI_SEED_FARTHEST && step >= 1u) {
            unsigned long long k = 0ull;
            for (uint64_t r = tid; r < n_ranges; r += NS_PICK_THREADS) k = far_key[r] > k ? far_key[r] : k;
            k = ns_block_max(k, sh);
            row = (uint32_t)~(uint32_t)k;
        } else {
            const unsigned long long u = ns_splitmix(rng_seed + (uint64_t)(8u * (uint64_t)step + t + 1u) * 0x9E3779B97F4A7C15ull);
            const unsigned long long target = __umul64hi(u, W);
            uint64_t range;
            unsigned long long rest;
            ns_locate([&](uint64_t r) -> unsigned long long { return part[(uint64_t)tstar * n_ranges + r]; }, n_ranges, target, sh, res,
                      &range, &rest);
            const uint64_t d0 = range * NS_RANGE_ROWS, cnt = n - d0 < NS_RANGE_ROWS ? n - d0 : NS_RANGE_ROWS;
            uint64_t i;
            unsigned long long rest2;
            ns_locate(
                [&](uint64_t k) -> unsigned long long {
                    const uint32_t wv = w[d0 + k];
                    if (step == 0u) return wv != 0u ? 1ull : 0ull;
                    if (!pending) return wv;
                    const uint32_t c = cw[(uint64_t)tstar * n + d0 + k];
                    return wv < c ? wv : c;
                },
                cnt, rest, sh, res, &i, &rest2);
            row = d0 + i;
        }
        row = row < n ? row : n - 1u; // (never past the corpus, whatever was read)
        if (tid == 0u) state->cand_row[t] = (uint32_t)row;
        for (uint32_t k = tid; k < dim; k += NS_PICK_THREADS) {
            float v;
            if (bf16) v = __uint_as_float((uint32_t)reinterpret_cast<const uint16_t *>(rows)[row * dim + k] << 16);
            else v = reinterpret_cast<const float *>(rows)[row * dim + k];
            cand[(uint64_t)t * dim + k] = v;
        }
    }
}

// ------------------------------------------------------------------ host
template <int NV, bool BF16>
static int ns_launch_score(oi_ctx *ctx, uint32_t grid, const void *rows, uint64_t n, uint32_t dim, uint64_t n_ranges, uint32_t L, bool far,
                           const NsState *state, const float *cand, uint32_t *w, uint32_t *cw, unsigned long long *part,
                           unsigned long long *far_key) {
    const size_t lds = sizeof(float) * (size_t)L * dim;
#define NS_SCORE(LT, FAR, CHAIN)                                                                                                      \
    hipLaunchKernelGGL((ns_score_kernel<NV, BF16, LT, FAR, CHAIN>), dim3(grid), dim3(NS_THREADS), lds, ctx->stream, rows, n, dim, n_ranges, L, \
                       state, cand, w, cw, part, far_key)
#ifdef OI_ABLATION
    const char *no_chain = oi_ablation_env("OI_NS_NO_CHAIN");
    if (no_chain && no_chain[0] == '1') {
        if (far) NS_SCORE(1, true, false);
        else if (L == 1) NS_SCORE(1, false, false);
        else if (L == 2) NS_SCORE(2, false, false);
        else if (L <= 4) NS_SCORE(4, false, false);
        else NS_SCORE(8, false, false);
        OI_HIP_CHECK(hipGetLastError());
        return OI_OK;
    }
#endif
    if (far) NS_SCORE(1, true, true);
    else if (L == 1) NS_SCORE(1, false, true);
    else if (L == 2) NS_SCORE(2, false, true);
    else if (L <= 4) NS_SCORE(4, false, true);
    else NS_SCORE(8, false, true);
#undef NS_SCORE
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}

// Device seeds [K][dim] and rows [K] (may be null) out, both preset here (zeros, 0xFFFFFFFF); *d_info_out: the 24 bytes of
// oi_seed_info in the call's workspace.  Asynchronous on the ctx stream.  The argument and state checks are api.hip's.
int oi_launch_narratives_seed(oi_index *idx, uint32_t K, const oi_seed_spec &sp, const oi_doc_filter *filter, float *d_seeds,
                              uint32_t *d_rows, const void **d_info_out) {
    static_assert(sizeof(oi_doc_filter) == sizeof(uint4), "oi_doc_filter is 16 bytes");
    oi_ctx *ctx = idx->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = idx->n_docs;
    const uint32_t dim = idx->dim, L = sp.trials;
    const bool far = sp.method == OI_SEED_FARTHEST, bf16 = idx->rows_bf16 != nullptr;
    const uint64_t n_ranges = (n + NS_RANGE_ROWS - 1) / NS_RANGE_ROWS;
    // the workspace: state | w | cw (L > 1) | part | far keys (farthest-first) | candidate vectors
    StageLayout lay(256);
    const size_t at_state = lay.add(256), at_w = lay.add(sizeof(uint32_t) * (size_t)n), at_cw = lay.add(L > 1 ? sizeof(uint32_t) * (size_t)L * n : 0),
                 at_part = lay.add(sizeof(uint64_t) * (size_t)L * n_ranges), at_far = lay.add(far ? sizeof(uint64_t) * (size_t)n_ranges : 0),
                 at_cand = lay.add(sizeof(float) * (size_t)L * dim);
    DevBuf &ws = ctx->buf("seeds");
    OI_CHECK(ws.ensure(lay.total()));
    NsState *state = lay.at<NsState>(ws.p, at_state);
    uint32_t *w = lay.at<uint32_t>(ws.p, at_w), *cw = L > 1 ? lay.at<uint32_t>(ws.p, at_cw) : nullptr;
    unsigned long long *part = lay.at<unsigned long long>(ws.p, at_part);
    unsigned long long *far_key = far ? lay.at<unsigned long long>(ws.p, at_far) : nullptr;
    float *cand = lay.at<float>(ws.p, at_cand);
    *d_info_out = state;

    OI_HIP_CHECK(hipMemsetAsync(state, 0, sizeof(NsState), st));
    OI_HIP_CHECK(hipMemsetAsync(d_seeds, 0, sizeof(float) * (size_t)K * dim, st));
    if (d_rows) OI_HIP_CHECK(hipMemsetAsync(d_rows, 0xFF, sizeof(uint32_t) * (size_t)K, st));
    if (n == 0) return OI_OK; // found = 0, eligible = 0
    const void *rows = bf16 ? (const void *)idx->rows_bf16 : (const void *)idx->rows;
    const uint2 *attrs = (filter || sp.bucket_width) ? idx->doc_attrs.as<uint2>() : nullptr;
    const uint4 filt = oi_filter_words(filter);
    // four workgroups of four waves per CU, each with NS_UNROLL rows in flight; a workgroup holds at most 32 KB of LDS
    const uint32_t grid = (uint32_t)std::min<uint64_t>(n_ranges, (uint64_t)ctx->num_cus * 4);
    {
        ProfScope ps(ctx, "seed_init");
        hipLaunchKernelGGL(ns_init_kernel, dim3(grid), dim3(NS_THREADS), 0, st, attrs, filt, filter ? 1u : 0u, sp.stamp_origin, sp.bucket_width,
                           sp.n_buckets, n, n_ranges, w, part);
        OI_HIP_CHECK(hipGetLastError());
    }
    const uint32_t nv = (dim / 4 + 63) / 64; // float4 per lane: 1 .. 4 (OI_MAX_DIM = 1024)
    for (uint32_t j = 0; j <= K; ++j) {
        const uint32_t L_this = j <= 1 ? (j ? 1u : 0u) : L; // pass 1 scores p_0 alone
        const uint32_t L_next = j == K ? 0u : (j == 0 ? 1u : L);
        if (j >= 1) {
            ProfScope ps(ctx, "seed_score");
#define NS_PASS(NV, BF)                                                                                                              \
    OI_CHECK((ns_launch_score<NV, BF>(ctx, grid, rows, n, dim, n_ranges, L_this, far, state, cand, w, L_this > 1 ? cw : nullptr, part, far_key)))
            if (bf16) {
                if (nv <= 1) NS_PASS(1, true); else if (nv == 2) NS_PASS(2, true); else if (nv == 3) NS_PASS(3, true); else NS_PASS(4, true);
            } else {
                if (nv <= 1) NS_PASS(1, false); else if (nv == 2) NS_PASS(2, false); else if (nv == 3) NS_PASS(3, false); else NS_PASS(4, false);
            }
#undef NS_PASS
        }
        ProfScope ps(ctx, "seed_pick");
        hipLaunchKernelGGL(ns_pick_kernel, dim3(1), dim3(NS_PICK_THREADS), 0, st, rows, bf16 ? 1u : 0u, n, dim, n_ranges, j, L_this, L_next,
                           sp.method, sp.seed, state, w, cw, part, far_key, cand, d_seeds, d_rows);
        OI_HIP_CHECK(hipGetLastError());
    }
    return OI_OK;
}
