// oi_select_rank.h -- the pieces of the selects (select.hip) that the sample pass's rank kernel (sample_rank.hip) shares: the
// shared words of one select workgroup, the 2048-bin rank search, the r-th largest score key and the words of a speculative
// threshold.  One workgroup of SEL_THREADS threads owns one query.
#pragma once

#include "oi_device.h"

// (select.hip, whose tuning constants these are, defines both before it includes this header)
#ifndef SEL_THREADS
#define SEL_THREADS 1024
#endif
#ifndef SEL_MAX_SEGS
#define SEL_MAX_SEGS 4096
#endif
static_assert(SEL_THREADS == 1024 && SEL_MAX_SEGS == 4096, "sel_rank_bin2k and SelShared are laid out for 1024 threads and 4096 segments");

// ---------------------------------------------------------------- speculative thresholds of the screen
// The screen's threshold after m of n rows is PROVEN: tau~_m - 2 eps, tau~_m the k'-th best screen score of those m rows.  It is
// weak while m << n (k' of 28 672 rows: 3.5 % of the next chunk pass; the final one passes 0.01 %), and every survivor of a weak
// threshold costs staging, pool traffic and select time.  What the final threshold will be can be PREDICTED from the same m rows:
// if they are a fair sample, the k'-th best of n sits near the (k' m / n)-th best of m.  The prediction takes the r-th best screen
// score so far, r = 3 k' m / n + 12 (three times the expected rank plus twelve: for rows in any exchangeable order the chance
// that fewer than k' of the n rows reach it is < 1e-9 whatever m), lowers it by the same 2 eps, and hands the LARGER of it and the
// proven threshold to the next chunk.  A prediction is not a bound -- so it is CHECKED: pf_rescore_kernel (cosine_prefilter.hip,
// first thing) compares the largest speculative threshold used for a query with the proven one at the end, tau~_n - 2 eps.
// T_spec <= tau~_n - 2 eps means every row the speculation dropped (s~ < T_spec) would have been dropped by the final proven
// threshold as well: the survivor set still holds every row of the exact list, the lists are the proven screen's.  Otherwise (a
// corpus whose first rows are not a fair sample: sorted by time or topic) the gate opens and the exact pipeline rescores the batch
// in the same call, and the host, told through a pinned flag, stops speculating for a while (search.hip: oi_spec_take_failure).
//
// The words of a query's speculative threshold from the r-th largest score key of its carry region (sel_rth_score_key; have: r
// keys were there): the key lowered by the margin, never below the proven threshold tau, and the largest one used is remembered
// for the check.  One thread calls.
__device__ __forceinline__ void sel_spec_words(bool have, uint32_t rth_key, float eps2, uint32_t tau, uint32_t *spec_tau, uint32_t *spec_max) {
    if (!have) { *spec_tau = tau; return; } // too few keys kept: the proven threshold as it is
    const float s = oi_key_f32(rth_key) - eps2; // (a query without a bound has eps2 = +inf: -inf, no speculation)
    const uint32_t T = s == s ? oi_f32_key(s) : 0u;
    const uint32_t st = T > tau ? T : tau;
    *spec_tau = st;
    if (st > tau && st > *spec_max) *spec_max = st;
}

// The words of a radix select (sel_threshold, sel_rank_bin2k): all select_topk_kernel needs of SelShared.
struct SelRadix {
    uint32_t hist[256];
    uint32_t kk, bin_cnt;
    uint64_t prefix;
};
struct SelShared {
    SelRadix rx;
    uint32_t hist2k[2048]; // the margin selects' 11-bit digits (sel_margin_bins, sel_rth_score_key)
    uint32_t seg_off[SEL_MAX_SEGS + 1];
    uint32_t wave_tot[SEL_THREADS / 64];
    uint32_t cnt, n_samples;
    unsigned long long min_key;
};

// hist[digit] += weight for the active lanes; the two most common digits of the wave go in as one atomic each
__device__ __forceinline__ void sel_hist_add_w(uint32_t *hist, bool active, uint32_t digit, uint32_t weight) {
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const unsigned long long m = __ballot(active);
        if (!m) return;
        const uint32_t leader = (uint32_t)__builtin_ctzll(m);
        const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)digit, (int)leader);
        const bool same = active && digit == d0;
        const uint32_t sum = (uint32_t)__builtin_amdgcn_readlane((int)oi_wave_incl_scan(same ? weight : 0u), 63);
        if (lane == leader) atomicAdd(&hist[d0], sum);
        active = active && !same;
    }
    if (active) atomicAdd(&hist[digit], weight);
}

// sh.hist2k holds a histogram of 2048 digits (filled, barrier passed): which digit holds the kk-th key counted from the top?
// -> sh.rx.prefix = the digit, sh.rx.kk = the rank inside it, sh.rx.bin_cnt = 1; fewer than kk keys: sh.rx.bin_cnt = 0xFFFFFFFF.
// All threads call; the words are readable on return (and rewritten by the next call: a barrier before that).
__device__ __forceinline__ void sel_rank_bin2k(SelShared &sh, uint32_t kk, int pass) {
    const uint32_t tid = threadIdx.x;
    { // 64 super-bins of 32 bins: a thread adds two bins, a DPP row (16 lanes) the 32 of a super-bin -- conflict-free reads
        uint32_t v = sh.hist2k[2 * tid] + sh.hist2k[2 * tid + 1];
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false); // row_shr:1
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false); // row_shr:2
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false); // row_shr:4
        v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false); // row_shr:8
        if ((tid & 15u) == 15u) sh.rx.hist[tid >> 4] = v; // super-bin s = bins [32 s, 32 s + 32)
    }
    __syncthreads();
    if (tid < 64) { // wave 0: the super-bin, then the bin, holding the kk-th key counted from the top -- two scans, no walk
        const uint32_t x = sh.rx.hist[63u - tid];
        const uint32_t incl = oi_wave_incl_scan(x);
        const unsigned long long ball = __ballot(incl >= kk);
        if (!ball) {
            if (tid == 0) sh.rx.bin_cnt = 0xFFFFFFFFu; // fewer than kk valid keys
        } else {
            const uint32_t l1 = (uint32_t)__builtin_ctzll(ball), sb = 63u - l1;
            const uint32_t kk2 = kk - (uint32_t)__builtin_amdgcn_readlane((int)(incl - x), (int)l1);
            const uint32_t y = tid < 32u ? sh.hist2k[32u * sb + 31u - tid] : 0u;
            const uint32_t incl2 = oi_wave_incl_scan(y);
            const unsigned long long ball2 = __ballot(incl2 >= kk2); // (non-empty: the super-bin holds >= kk2 keys)
            const uint32_t l2 = ball2 ? (uint32_t)__builtin_ctzll(ball2) : 31u;
            // (read with every lane active: inside the one-lane branch below hipcc computes incl2 - y for that lane only)
            const uint32_t above = (uint32_t)__builtin_amdgcn_readlane((int)(incl2 - y), (int)l2);
            if (tid == 0) {
                sh.rx.prefix = (uint64_t)(32u * sb + 31u - l2);
                sh.rx.kk = kk2 - above;
                sh.rx.bin_cnt = 1u;
#ifdef SEL_RANK_SELFCHECK
                if (sel_dbg_on > 1) { // OI_SELECT_STAMPS=2: self-check against the plain walk from the top
                    uint32_t cum = 0; int dd = 2047;
                    for (; dd >= 0; --dd) { if (cum + sh.hist2k[dd] >= kk) break; cum += sh.hist2k[dd]; }
                    if ((uint32_t)dd != (uint32_t)sh.rx.prefix || kk - cum != sh.rx.kk)
                        printf("MISMATCH q=%u pass=%d kk=%u: walk (%d, %u) super-bin (%u, %u) sb=%u l1=%u kk2=%u l2=%u\n", blockIdx.x, pass, kk, dd, kk - cum,
                               (uint32_t)sh.rx.prefix, sh.rx.kk, sb, l1, kk2, l2);
                }
#endif
            }
        }
    }
    __syncthreads();
}

// One pass of a thread's keys into sh.hist2k by their leading 11 bits (sign, exponent, two bits of mantissa).  A pool of
// near-threshold scores takes a handful of such digits: a thread adds its keys up in runs first, and the wave its threads'
// last runs (one LDS address each).
template <class FE>
__device__ __forceinline__ void sel_hist_leading(FE &&for_each, SelShared &sh) {
    uint32_t run_d = 0, run_c = 0;
    for_each([&](bool valid, uint64_t kv) {
        if (valid) {
            const uint32_t d = (uint32_t)(kv >> 53);
            if (run_c && d != run_d) { atomicAdd(&sh.hist2k[run_d], run_c); run_c = 0; }
            run_d = d;
            ++run_c;
        }
    });
    sel_hist_add_w(sh.hist2k, run_c != 0u, run_d, run_c);
}

// The r-th largest 32-bit score key of the keys `for_each` enumerates (f(valid, key), the same keys on every call; 1 <= r <= their
// number): digits of 11, 11 and 10 bits from the top through the same histogram.  The r-th largest of a set is unique, so
// whichever keys of the carry region the select already holds in registers give the prediction's key.  All threads call; the result is uniform.  sh.hist2k / sh.rx's words are free on entry and on return.
template <class FE>
__device__ __forceinline__ uint32_t sel_rth_score_key(FE &&for_each, uint32_t r, SelShared &sh) {
    const uint32_t tid = threadIdx.x;
    uint32_t kk = r, pfx = 0;
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0, bits = pass == 2 ? 10 : 11;
        sh.hist2k[tid] = 0;
        sh.hist2k[tid + SEL_THREADS] = 0;
        __syncthreads();
        if (pass == 0) {
            sel_hist_leading(for_each, sh);
        } else {
            for_each([&](bool valid, uint64_t kv) {
                const uint32_t sk = (uint32_t)(kv >> 32);
                if (valid && (sk >> (shift + bits)) == pfx) atomicAdd(&sh.hist2k[(sk >> shift) & ((1u << bits) - 1u)], 1u);
            });
        }
        __syncthreads();
        sel_rank_bin2k(sh, kk, 2 + pass);
        const uint32_t d = sh.rx.bin_cnt != 0xFFFFFFFFu ? (uint32_t)sh.rx.prefix : 0u; // (r <= the number of keys: always found)
        kk = sh.rx.kk;
        __syncthreads();
        pfx = (pfx << bits) | d;
    }
    return pfx;
}
