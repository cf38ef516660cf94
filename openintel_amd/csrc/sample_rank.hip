// sample_rank.hip -- the first speculative threshold of the int8 route, read off the sample pass's dense key array.
#include "oi_internal.h"
#include "oi_select_rank.h"

#define SEL_KPT_MAX 32 // keys a thread holds in registers, as the selects' largest register class (select.hip)

// sample_rank_kernel: the first speculative threshold of the int8 route from the sample pass (cosine_screen_i8.hip,
// i8s_sample_kernel): a query's dense score keys keys[q][0..stride) -- the sample's m rows, 0 where a row takes no part --
// held in registers (stride <= SEL_KPT_MAX * SEL_THREADS), the r-th largest through sel_rth_score_key, the words through
// sel_spec_words.  It is the key the first chunk's margin select found among the keys it carried: the r-th largest of a set is
// unique, and that select carries every key down to the k-th >= r-th.  Fewer than r real keys: the r-th is key 0, a NaN's, which
// sel_spec_words turns into "the proven threshold as it is".
__global__ __launch_bounds__(SEL_THREADS) void sample_rank_kernel(const uint32_t *__restrict__ keys, uint32_t stride, uint32_t m, uint32_t r,
                                                                  const float *__restrict__ eps2, const uint32_t *__restrict__ tau_keys,
                                                                  uint32_t *spec_tau, uint32_t *spec_max) {
    __shared__ SelShared sh;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t *kq = keys + (uint64_t)q * stride;
    const uint32_t kpt = (stride + SEL_THREADS - 1) / SEL_THREADS;
    uint32_t key[SEL_KPT_MAX];
#pragma unroll
    for (int j = 0; j < SEL_KPT_MAX; ++j) {
        const uint32_t i = (uint32_t)j * SEL_THREADS + tid;
        key[j] = (uint32_t)j < kpt && i < stride ? kq[i] : 0u;
    }
    const bool have = m >= r; // (uniform)
    uint32_t rth = 0;
    if (have)
        rth = sel_rth_score_key([&](auto &&f) {
#pragma unroll
            for (int j = 0; j < SEL_KPT_MAX; ++j)
                if ((uint32_t)j < kpt) f((uint32_t)j * SEL_THREADS + tid < stride, (uint64_t)key[j] << 32);
        }, r, sh);
    if (tid == 0) sel_spec_words(have, rth, eps2[q], tau_keys[q], spec_tau + q, spec_max + q);
}

int oi_launch_sample_rank(oi_ctx *ctx, const uint32_t *keys, uint32_t stride, uint32_t m, uint32_t n_queries, uint32_t r, const float *eps2,
                          const uint32_t *tau_keys, uint32_t *spec_tau, uint32_t *spec_max) {
    if (n_queries == 0) return OI_OK;
    OI_REQUIRE(r >= 1 && m <= stride && stride <= SEL_KPT_MAX * SEL_THREADS, "sample rank: %u keys of %u, rank %u", m, stride, r);
    // two spans: "spec" counts the predictions made; "select" goes on counting one span per selection launch of the leg, this one in
    // the place of the first chunk's margin select (the recorded launch schedules and the tools' select share read that tag)
    ProfScope pl(ctx, "select");
    ProfScope ps(ctx, "spec");
    hipLaunchKernelGGL(sample_rank_kernel, dim3(n_queries), dim3(SEL_THREADS), 0, ctx->stream, keys, stride, m, r, eps2, tau_keys, spec_tau, spec_max);
    OI_HIP_CHECK(hipGetLastError());
    return OI_OK;
}
