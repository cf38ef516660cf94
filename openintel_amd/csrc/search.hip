// search.hip -- one hybrid search on the device (search_lists_device): the plan of the call, the chunk schedule of the cosine
// leg, the cosine routes and the four BM25 modes.  The entry points that stage the queries and copy the results are in api.hip.
#include <algorithm>
#include <cassert>

#include "oi_internal.h"

namespace {

// ---------------------------------------------------------------- the A/B switches of this path (-DOI_ABLATION builds), read once
int env_int(const char *name, int dflt, int lo) { return oi_ablation_env(name) ? std::max(lo, atoi(oi_ablation_env(name))) : dflt; }
bool env_set(const char *name) { return oi_ablation_env(name) != nullptr; }
struct Knobs {
    uint64_t first_mult = env_int("OI_FIRST_CHUNK_MULT", 1, 1), first_div = env_int("OI_FIRST_CHUNK_DIV", 1, 1);
    uint64_t growth = env_int("OI_CHUNK_GROWTH", 0, 2); // (0: by batch size)
    uint64_t spec_growth = env_int("OI_SPEC_GROWTH", 128, 2), spec_first_div = env_int("OI_SPEC_FIRST_DIV", 4, 1);
    uint32_t bm25_first_div = env_int("OI_BM25_FIRST_DIV", 8, 1);
    bool screen_no_round = env_set("OI_SCREEN_NO_ROUND"), no_spec = env_set("OI_NO_SPEC"), no_overlap = env_set("OI_NO_OVERLAP");
    bool bm25_beside_last = env_set("OI_BM25_BESIDE_LAST"), screen_i8_narrow = env_set("OI_SCREEN_I8_NARROW");
    bool no_sample_pass = env_set("OI_NO_SAMPLE_PASS");
    bool bm25_early = env_set("OI_BM25_EARLY"), small_gemv = env_set("OI_SMALL_BATCH_GEMV"), bm25_two_phase = env_set("OI_BM25_TWO_PHASE");
    // the first-generation cosine / select kernels have no screen in front of them
    bool exact_only = env_set("OI_COSINE_V1") || env_set("OI_SELECT_V1");
};
const Knobs &knobs() { static const Knobs k; return k; }

// ---------------------------------------------------------------- pools
struct Pools { PoolView cos, bm; };
// 1 term-at-a-time per workgroup (bm25.hip), 2 scan of the forward index, 3 one wave per task (bm25_wave.hip), 4 the stream
// kernel (bm25_stream.hip: the default).  The index's own setting wins over the process-wide OI_BM25_MODE.
enum { BM25_TAAT = 1, BM25_SCAN = 2, BM25_WAVE = 3, BM25_STREAM = 4 };
int bm25_mode_of(const oi_index *idx) {
    static const char *mode_env = getenv("OI_BM25_MODE");
    int mode = idx->bm25_mode;
    if (mode == 0 && mode_env)
        mode = strcmp(mode_env, "scan") == 0 ? 2 : strcmp(mode_env, "taat") == 0 ? 1 : strcmp(mode_env, "wave") == 0 ? 3 : 4;
    return mode == 0 ? 4 : mode;
}
// The state words of one pool, carry_cnt[n] tau[n] seg_cnt[n][segs] in memory order: the one place that lays them out.
struct PoolWords {
    uint32_t *carry, *tau, *seg;
    static size_t count(uint32_t n_queries, uint32_t segs) { return (size_t)n_queries * (2 + (size_t)segs); }
    PoolWords(uint32_t *w, uint32_t n_queries) : carry(w), tau(w + n_queries), seg(w + 2 * (size_t)n_queries) {}
};
// State of both pools in one block, zeroed with ONE memset per search: the cosine pool's words (a segment per workgroup), then
// the BM25 pool's (a segment per doc block).
// `extra_words` more zeroed words follow them (*extra): the bf16 screen's state, so that one memset kernel does both.
int prepare_pools(oi_ctx *ctx, uint32_t B, uint64_t cos_alloc_stride, uint64_t cos_stride, uint32_t carry_cap, uint32_t bm_blocks,
                  uint32_t depth, Pools *out, size_t extra_words, uint32_t **extra) {
    DevBuf &flag = ctx->buf("state_flag");
    if (!flag.p) {
        OI_CHECK(flag.ensure(16));
        OI_HIP_CHECK(hipMemsetAsync(flag.p, 0, 16, ctx->stream));
    }
    const uint32_t cos_segs = (uint32_t)ctx->num_cus * (B <= 8 ? 8u : 1u); // one per workgroup: GEMV grids are 8 per CU
    const uint32_t bm_segs = bm_blocks ? bm_blocks : 1;
    const size_t cos_words = PoolWords::count(B, cos_segs), words = cos_words + PoolWords::count(B, bm_segs);
    DevBuf &st = ctx->buf("pool_state");
    OI_CHECK(st.ensure(sizeof(uint32_t) * (words + extra_words)));
    OI_HIP_CHECK(hipMemsetAsync(st.p, 0, sizeof(uint32_t) * (words + extra_words), ctx->stream));
    *extra = st.as<uint32_t>() + words;
    const uint64_t bm_stride = (uint64_t)carry_cap + (uint64_t)bm_segs * depth;
    DevBuf &pc = ctx->buf("pool_cos"), &pb = ctx->buf("pool_bm");
    OI_CHECK(pc.ensure(sizeof(uint64_t) * (size_t)B * cos_alloc_stride)); // (room for the widest view of it: the screen's)
    OI_CHECK(pb.ensure(sizeof(uint64_t) * (size_t)B * bm_stride));
    const PoolWords cw(st.as<uint32_t>(), B), bw(st.as<uint32_t>() + cos_words, B);
    out->cos = PoolView{pc.as<uint64_t>(), cw.carry, cw.seg, cw.tau, cos_stride, carry_cap, 0, 0, cos_segs, flag.as<uint32_t>()};
    out->bm = PoolView{pb.as<uint64_t>(), bw.carry, bw.seg, bw.tau, bm_stride, carry_cap, depth, bm_segs, bm_segs, flag.as<uint32_t>()};
    return OI_OK;
}

// ---------------------------------------------------------------- the chunk schedule of the cosine leg
// Rows of the first corpus chunk (scored with no threshold yet: every row lands in the pool, so it is kept
// small); each later chunk is 8x the one before.  OI_FIRST_CHUNK_MULT scales it (A/B runs).
uint64_t oi_first_chunk_rows(uint32_t depth) {
    return std::max<uint64_t>(std::max<uint64_t>(8192, 32ull * depth) * knobs().first_mult / knobs().first_div, 2ull * depth);
}
// The screen's first chunk (round 4): a whole number of ROUNDS of the persistent grid -- 7/8 of the CUs x 4 waves x 32-row tiles
// (cosine_prefilter.hip: oi_cosine_screen_geometry) -- so that no wave of the two short first launches runs one tile more than
// the others (32000 rows = 1000 tiles on 896 waves: 104 waves with two tiles; 256000 rows: 9.1 per wave, i.e. 10 rounds).
// Chunk k is 8^k times the first and keeps the property.  OI_SCREEN_NO_ROUND=1 (A/B): as before.
// The round stays that of 7/8 of the CUs where the int8 route's chunks take every CU (plan_search, screen_wgs): the first chunk is
// the sample the thresholds come from and must not move, and its 224 quads are one tile per wave at either width.
uint64_t oi_screen_first_chunk_rows(const oi_ctx *ctx, uint32_t depth) {
    uint64_t rows = oi_first_chunk_rows(depth);
    const uint64_t round = 32ull * 4 * std::max<uint64_t>(1, (uint64_t)ctx->num_cus * 7 / 8);
    if (!knobs().screen_no_round && rows >= round) rows -= rows % round;
    return rows;
}
// Measured (tools/growth_ab.sh): 8 is best for the MFMA batch path at 10M and 1.25M rows (more survivors per
// chunk cost more in the epilogue and the select than the launch they save); the GEMV path (B <= 8) gains
// 3 % from 16 (1M rows: 3 launches instead of 4).
uint64_t oi_chunk_growth(uint32_t B) { return knobs().growth ? knobs().growth : (B <= 8 ? 16 : 8); }
// End of the corpus chunk that starts at row r: `chunk` rows, but a tail shorter than a quarter of the chunk is taken along
// (a 2.5M-row shard: 32K, 256K, 2.2M rows instead of 32K, 256K, 2M and a fourth launch + select for 0.2M).
// And when what is left after this chunk would not fit ONE more chunk but fits two, this chunk grows so that the last one is
// exactly the largest the pool takes (10M rows, 6.8M-row pool: 32K, 256K, 2.9M, 6.8M instead of 32K, 256K, 2M, 6.8M, 0.9M).
// (only where the chunk AFTER this one would be cut by the pool anyway -- `next_chunk`, its planned size, reaches max_chunk).
uint64_t oi_chunk_end(uint64_t r, uint64_t chunk, uint64_t n, uint64_t max_chunk, uint64_t next_chunk) {
    uint64_t e = std::min(n, r + chunk);
    if (e < n && (n - e) * 4 <= (e - r) && n - r <= max_chunk) e = n;
    if (e < n && next_chunk >= max_chunk && n - e > max_chunk && n - r <= 2 * max_chunk) e = n - max_chunk;
    return e;
}

struct Chunk { uint64_t r, e; }; // rows [r, e)
// The chunks of n rows: `first` rows, each later chunk `growth` times the one before, none above max_chunk (> 0), the ends
// through oi_chunk_end.  stretch_first = false for a first chunk scored without a threshold (the screen's): it is never stretched.
std::vector<Chunk> chunk_schedule(uint64_t n, uint64_t first, uint64_t growth, uint64_t max_chunk, bool stretch_first) {
    std::vector<Chunk> out;
    uint64_t chunk = first, r = 0;
    while (r < n) {
        if (chunk > max_chunk) chunk = max_chunk;
        const uint64_t e = oi_chunk_end(r, chunk, n, max_chunk, r == 0 && !stretch_first ? 0 : chunk * growth);
        out.push_back(Chunk{r, e});
        r = e;
        chunk *= growth;
    }
    return out;
}

// ---------------------------------------------------------------- the plan of one search
struct Search { // the call's arguments; all pointers device
    oi_index *idx; oi_ctx *ctx;
    const float *qv; const uint32_t *qt, *qo;
    uint32_t B, depth;
    float *cos_s; uint32_t *cos_d, *cos_c;
    float *bm_s; uint32_t *bm_d, *bm_c;
    const uint4 *filt; const uint2 *attrs; // a filtered search: per-query doc filters, the index's {group, stamp} per row
};
// none: no cosine list wanted; bf16: a bf16 corpus (cosine_bf16.hip); exact: f32 GEMV, K-split, split-precision or tile (chosen
// per chunk by oi_launch_cosine_chunk); the bf16 screen, then rescoring and the gated exact pipeline, with bf16(x) converted from the
// f32 rows (screen_f32), read from the index's screening copy (screen_copy) or behind the int8 first tier (screen_i8)
enum class CosRoute { none, bf16, exact, screen_f32, screen_copy, screen_i8 };

struct Plan {
    CosRoute cos = CosRoute::none;
    int bm25 = BM25_STREAM; // the BM25 kernel, after the fallback of a scan without forward tokens (run when the list is wanted)
    uint64_t cos_stride = 0, pf_stride = 0, pf_slack = 0; // the cosine pool and the screen's view of the same buffer
    uint32_t pf_carry = 4096;
    bool spec = false; // speculative screen thresholds
    std::vector<Chunk> screen_chunks; // the screen routes' schedule
    // the int8 route's sample pass: the first speculative threshold comes from the dense score keys of rows [0, sample_rows)
    // (cosine_screen_i8.hip: i8s_sample_kernel, select.hip: sample_rank_kernel) and the first screen chunk, which starts at row 0
    // all the same, runs under it; 0 = the first chunk is pooled without a threshold and its margin select makes the prediction
    uint32_t sample_rows = 0;
    // the BM25 leg on the side stream; late_fork: forked in at the screen's last chunk -- beside it, or (tail_fork, the int8 route)
    // behind it, beside the cosine leg's tail
    bool overlap = false, late_fork = false, tail_fork = false;
    // workgroups of an int8 screen launch: every CU when no other kernel runs beside the chunks, 0 = the screens' 7/8 of the
    // CUs (oi_cosine_screen_geometry).  The bf16 copy, f32-stream and threshold-family kernels are HBM-bound at 7/8 and keep it.
    uint32_t screen_wgs = 0;
    // the int8 route's second tier: the residual plane's rescreen (screen_i8_residual.hip) where the index holds the plane and the
    // ctx allows it (oi_internal_set_rescreen_tier), the bf16 rescreen otherwise
    bool rescreen_residual = false;
};
bool screened(CosRoute c) { return c == CosRoute::screen_f32 || c == CosRoute::screen_copy || c == CosRoute::screen_i8; }

Plan plan_search(const Search &s) {
    oi_index *idx = s.idx; oi_ctx *ctx = s.ctx;
    const Knobs &K = knobs();
    const uint64_t n = idx->n_docs;
    const uint32_t B = s.B, depth = s.depth, carry_cap = OI_MAX_DEPTH;
    Plan p;
    // ---- the cosine route
    // (a view never makes a copy of its own: it streams the source's if that exists, the f32 rows otherwise)
    // OI_COSINE_SCREEN streams the index's bf16 screening copy when there is one (made at finalize, budget permitting);
    // _COPY also makes a missing one now; _STREAM converts the f32 rows on the fly whatever the index holds.
    // B <= 8 (configs[1]: one query): screened only when there is a copy to stream -- half the bytes of the f32 GEMV, which
    // is HBM-bound; the f32-stream screen would read what the GEMV reads.  OI_SMALL_BATCH_GEMV=1 (A/B): as before round 5.
    // The int8 first tier (cosine_screen_i8.hip) when the index holds both screening copies and B > 8.
    const int mode = ctx->cosine_mode;
    const bool want_copy = mode != OI_COSINE_SCREEN_STREAM && (idx->screen_copy.p != nullptr || (mode == OI_COSINE_SCREEN_COPY && !idx->is_view));
    const bool screen = (mode == OI_COSINE_SCREEN || mode == OI_COSINE_SCREEN_COPY || mode == OI_COSINE_SCREEN_STREAM) &&
                        oi_index_screenable(idx) && (B > 8 || (want_copy && !K.small_gemv)) && !K.exact_only;
    if (!s.cos_s) p.cos = CosRoute::none;
    else if (idx->rows_bf16) p.cos = CosRoute::bf16;
    else if (!screen) p.cos = CosRoute::exact;
    else if (!want_copy) p.cos = s.filt ? CosRoute::exact : CosRoute::screen_f32; // (filtered: the f32-stream screen has no filter)
    else if (B > 8 && idx->screen_copy.p && idx->screen_i8.p) p.cos = CosRoute::screen_i8;
    else p.cos = CosRoute::screen_copy;
    p.rescreen_residual = p.cos == CosRoute::screen_i8 && idx->screen_i8r.p != nullptr && ctx->rescreen_residual;
    p.bm25 = bm25_mode_of(idx);
    if (p.bm25 == BM25_SCAN && !(idx->fwd_terms.p && idx->total_tokens > 0)) p.bm25 = BM25_STREAM; // (no forward tokens to scan)
    // A filtered search: every BM25 mode runs the stream kernel (the four give bit-identical lists; only it has the filter)
    if (s.filt) p.bm25 = BM25_STREAM;
    // ---- pool capacities
    // cosine: the corpus is scored in chunks; a chunk can append at most one entry per row and query, so a chunk sized from the
    // pool's free room can never overflow it (no overflow path to handle, no data-dependent sizing).  BM25: every doc block
    // contributes <= depth entries.
    const uint64_t slack = (idx->rows_bf16 ? 128ull : 32ull) * ((uint64_t)ctx->num_cus + 1);
    // Large pools = few launches: at 10M rows the schedule is 32K, 256K, 3.2M, 6.5M rows (4 launches).  The room is worst
    // case (every row of a chunk passes the threshold), only entries that pass are written.  Round 4: an f32 corpus gets
    // 3.25 GiB of pool instead of 8 (the last two chunks are balanced so that the launch count stays), and the screen's pool
    // and the exact fallback's pool are ONE buffer (they are never live together: the gated exact pipeline starts after the
    // rescoring has consumed the screen's survivors).  A bf16 corpus (configs[4]: 256 queries) keeps 8 GiB.
    const uint64_t budget = (idx->rows_bf16 ? (8ull << 30) : (13ull << 28)) / 8 / B;
    p.cos_stride = std::min<uint64_t>(carry_cap + n + slack, std::max<uint64_t>(std::min<uint64_t>(1ull << 24, budget), carry_cap + 4 * slack));
    // the screen's view of the same buffer keeps up to 4096 keys per query between chunks and rounds its segments to 4 tiles; with
    // the int8 first tier up to OI_I8_CARRY
    p.pf_carry = p.cos == CosRoute::screen_i8 ? OI_I8_CARRY : 4096;
    p.pf_slack = 128ull * ((uint64_t)ctx->num_cus + 1);
    p.pf_stride = std::min<uint64_t>(p.pf_carry + n + p.pf_slack, std::max<uint64_t>(std::min<uint64_t>(1ull << 24, budget), p.pf_carry + 4 * p.pf_slack));
    // ---- speculative thresholds of the screen (oi_select_rank.h: sel_spec_words; oi_set_screen_speculation).  Decided here
    // because the chunk schedule depends on it: with a predicted threshold after the first chunk the second can be as large as the
    // pool takes (10M rows 2.64 -> 2.54 ms, a 1.25M-row shard 0.574 -> 0.540 -> 0.523 with the short first chunk;
    // tools/r05_spec_sched.sh), with proven thresholds it must grow slowly (x 8).  Off: oi_set_screen_speculation(ctx, 0); with
    // graph replay (the host decides per call); for batches of <= 8 queries (their survivors cost next to nothing, the extra
    // launches 11 us of 0.34 ms); for spec_skip searches after a failed check.  OI_NO_SPEC=1, OI_SPEC_GROWTH (ablation builds): A/B.
    uint64_t first = oi_screen_first_chunk_rows(ctx, depth), growth = oi_chunk_growth(B);
    const uint64_t pool_max = p.pf_stride - p.pf_carry - p.pf_slack; // rows one screen launch may take (> 0 unless n = 0)
    // No speculation under a filter: the prediction takes the first chunk for a fair sample of the PASSING rows, which a filter
    // on a corpus stored by ticker or time never is; the ctx's back-off is neither consumed nor changed.
    if (screened(p.cos) && B > 8 && !s.filt) {
        oi_spec_take_failure(ctx);
        p.spec = ctx->speculate && !K.no_spec && !ctx->use_graphs;
        if (p.spec && ctx->spec_skip) { --ctx->spec_skip; p.spec = false; }
        if (p.spec && !ctx->spec_fail_host) {
            if (hipHostMalloc(reinterpret_cast<void **>(&ctx->spec_fail_host), 64, hipHostMallocDefault) == hipSuccess) *ctx->spec_fail_host = 0;
            else { (void)hipGetLastError(); ctx->spec_fail_host = nullptr; p.spec = false; } // (no way to hear of a failed check: no speculation)
        }
        if (p.spec && n) { // does the rank after the FIRST chunk qualify (a prediction is made, in the chunk's margin select, when 2 r <= k')?
            // a SHORT first chunk (a quarter of the proven schedule's, >= 8192 rows, >= 8 k': its only job is the sample the
            // prediction is read from) when everything after it fits ONE launch -- a shard: 8 192 rows, then the rest
            // (1.25M rows: 0.540 -> 0.523 ms against 28 672 + the rest); a corpus that needs three launches anyway keeps the
            // regular first chunk and grows x 128 (10M: 28 672, 3.67M, 6.3M rows; a short first chunk measured the same there)
            const uint64_t first_short = std::min<uint64_t>(n, std::max<uint64_t>(std::max<uint64_t>(8192, 8ull * depth), first / K.spec_first_div));
            if (n - first_short <= pool_max && 2 * ((3ull * depth * first_short + n - 1) / n + 12) <= depth) {
                growth = K.spec_growth;
                first = first_short;
            } else if (2 * ((3ull * depth * std::min<uint64_t>(n, first) + n - 1) / n + 12) <= depth) growth = K.spec_growth;
        }
    }
    // (the threshold-less first chunk is never stretched: it is the sample the thresholds come from)
    if (screened(p.cos)) p.screen_chunks = chunk_schedule(n, first, growth, pool_max, /*stretch_first=*/false);
    // ---- the sample pass of the int8 route.  Where a prediction follows the threshold-less first chunk, that prediction is the
    // chunk's only use: T1 = key(r-th largest lower-bound key of its rows) - m2, and the proven threshold of the same select, from
    // rank k' >= 2 r of the same keys less the same m2, is never the larger one.  So the rows of that chunk are scored into a dense
    // key array instead (no pool, no survivor path, no margin select), a small kernel takes the r-th largest, and the second chunk
    // starts at row 0: it screens the sample rows again, under T1 (10M rows: 0.8 % more stream).  The later chunk ends stay, so
    // every later launch is the same launch.  Only where the merged chunk still fits one launch's pool room; otherwise, and
    // without speculation (off, backed off, filtered, graph replay, B <= 8), on the bf16 routes and with OI_NO_SAMPLE_PASS=1
    // (ablation builds), the pooled first chunk as before.
    if (p.cos == CosRoute::screen_i8 && p.spec && !K.no_sample_pass && p.screen_chunks.size() >= 2) {
        const uint64_t m = p.screen_chunks[0].e;
        // (the key array, [B rounded to 32][m rounded to 32] words, lies in the still empty pool buffer: cosine_screen)
        const uint64_t key_words = (uint64_t)((B + 31u) & ~31u) * ((m + 31) & ~31ull);
        if (2 * ((3ull * depth * m + n - 1) / n + 12) <= depth && p.screen_chunks[1].e <= pool_max && m <= (32u << 10) &&
            key_words <= 2 * (uint64_t)B * p.pf_stride) {
            p.sample_rows = (uint32_t)m;
            p.screen_chunks.erase(p.screen_chunks.begin());
            p.screen_chunks[0].r = 0;
        }
    }
    // ---- the two legs of a hybrid query are independent until fusion: the BM25 leg (latency-bound, 128 KB of LDS per workgroup)
    // is issued on a side stream and fills the issue slots the MFMA-bound cosine leg leaves, instead of running after it.
    // OI_NO_OVERLAP=1 serialises them (A/B runs).
    if (s.cos_s && s.bm_s && !ctx->side_stream && !ctx->side_stream_failed && ctx->overlap_legs && !K.no_overlap) {
        // (default priority: at the lowest one the BM25 leg stretched over the whole cosine leg and the step was no shorter)
        if (hipStreamCreateWithFlags(&ctx->side_stream, hipStreamNonBlocking) != hipSuccess) { ctx->side_stream = nullptr; ctx->side_stream_failed = true; }
    }
    p.overlap = s.cos_s && s.bm_s && ctx->side_stream && ctx->ev_fork && ctx->ev_join && ctx->overlap_legs && !K.no_overlap;
    // Round 4: beside the screen the BM25 leg starts with the LAST corpus chunk, not the first.  The screen's persistent
    // workgroups leave 1/8 of the CUs free; the BM25 kernels (enqueued AFTER the last chunk's launch, so that the screen's
    // workgroups are resident first) run there while the long chunk streams -- instead of sharing the CUs with the two short
    // first chunks, whose launches they stretched (10M rows: step 4.998 -> 4.940 ms on one box, -44 .. -58 us on three;
    // tools/r04_epilogue_probe.sh, r04_old_new_ab.sh).  Only when the last chunk is long enough to cover the leg: >= 512K rows.
    // OI_BM25_EARLY=1 (A/B): the round-3 placement.
    p.late_fork = p.overlap && !K.bm25_early && B > 8 && !p.screen_chunks.empty() &&
                  p.screen_chunks.back().e - p.screen_chunks.back().r >= (512u << 10);
    // The int8 screen is not HBM-bound at 7/8 of the CUs and its workgroups claim whole CUs: more waves shorten
    // a chunk (measured: by about half of what they add -- 10M rows, chunk 2 532-546 -> 506 us, chunk 3 799-825 -> 768 us at
    // 256 against 224 workgroups), but only where no other kernel needs a CU meanwhile.  So on this route the late fork moves
    // BEHIND the last chunk: ev_fork is recorded after the chunk's launch, the BM25 kernels start when it ends and run beside
    // the cosine leg's tail -- first on the 192 CUs the 64 workgroups of the chunk's margin select leave idle; the rescreen
    // beside them takes 130 us instead of 104, and the leg ends about 20 us before the cosine leg (profiles/i8_width_ab.json).
    // OI_BM25_BESIDE_LAST=1 (A/B): the fork of the bf16 routes.
    p.tail_fork = p.late_fork && p.cos == CosRoute::screen_i8 && !K.bm25_beside_last;
    // ... and the chunks take every CU when nothing runs beside them: no BM25 leg on the side stream, or one forked behind the
    // last chunk.  A leg forked at the start of the search (a last chunk too short to fork late) runs beside the chunks: 7/8.
    // A search through a VIEW keeps 7/8 as well: a view exists so that a second search can be in flight on the same shard, and
    // every lane of a pipeline (oi_pipeline_*, the sharded pipeline of the Python package) scores through one -- the other
    // lane's selects and rescoring and the fusing stream run on the CUs it leaves free.  The first chunk is NOT
    // re-rounded to the wider grid (oi_screen_first_chunk_rows): it is the sample every threshold comes from, and at 28 672
    // rows it has fewer quads than either width has workgroups.
    // OI_SCREEN_I8_NARROW=1 (A/B): 7/8 throughout.
    if (p.cos == CosRoute::screen_i8 && !idx->is_view && (!p.overlap || p.tail_fork) && !K.screen_i8_narrow)
        p.screen_wgs = (uint32_t)std::max(1, ctx->num_cus);
    return p;
}

// ---------------------------------------------------------------- BM25 leg: one function per mode
// Each runs on ctx->stream (the side stream when the legs overlap).  Their behaviour on an index without postings differs and is
// kept: the stream and wave kernels write empty lists without a launch, the term-at-a-time kernel runs its launches anyway.
// The STREAM kernel (bm25_stream.hip, the default).  Two phases like the cosine chunks: the first eighth of the doc blocks is
// scored with no threshold and fixes tau_q = the depth-th score so far, a lower bound of the final one; the remaining blocks emit
// only scores >= tau_q.  A task's pool segment is SMALL and fixed (4096 keys in the first phase, depth + 256 in the second): a
// segment that would overflow is pruned in place to its top `depth` keys, so nothing can overflow whatever the data, and the pool
// is ~3 MB per query at 10M docs.
int bm25_stream(const Search &s, const PoolView &bm) {
    oi_index *idx = s.idx; oi_ctx *ctx = s.ctx;
    const uint32_t B = s.B, depth = s.depth, carry_cap = OI_MAX_DEPTH, nb = idx->n_blocks;
    if (nb == 0 || idx->n_postings == 0) {
        OI_HIP_CHECK(hipMemsetAsync(s.bm_c, 0, sizeof(uint32_t) * B, ctx->stream));
        return OI_OK;
    }
    // (the share of the blocks scored without a threshold: 1/8 and 1/16 measure the same, 1/32 is 5 % slower)
    // Up to 48 blocks (1.5M docs: a shard of configs[3]) ONE phase: every touched doc is a candidate (~30K keys per query,
    // the select's register path), one launch and one select fewer -- 0.052 vs 0.081 ms of kernels at 1.25M docs.
    // Round 4, second half: NO threshold-less phase at all when the index has its per-term impact floors (bm25.hip): the
    // plan kernel starts every query at max_t fl(idf_t * floor_t) -- at least `depth` docs score that much, so it is a valid
    // lower bound of the depth-th best score before a posting is read -- and ONE launch scores every block against it, with the
    // small pruned segments of the former second phase.  At 10M docs that bound is HIGHER than the first phase's (the 1024th
    // impact of one term over all docs vs the 1000th score over an eighth of them), and a launch, a select and the first
    // phase's 30 K candidates per query go away.  OI_BM25_TWO_PHASE=1 (A/B): the phases as before.
    // (no floors under a doc filter: a floor bounds the depth-th score of ALL docs, not of the passing ones -- DESIGN 4.7)
    const bool floors = idx->impact_floor.p != nullptr && !knobs().bm25_two_phase && !s.filt;
    const uint32_t first = floors ? nb : nb > 48 ? std::max<uint32_t>(8, nb / knobs().bm25_first_div) : nb;
    const uint32_t cap1 = oi_bm25_stream_seg_cap(depth, !floors), cap2 = oi_bm25_stream_seg_cap(depth, false);
    const uint64_t sstride = (uint64_t)carry_cap + std::max<uint64_t>((uint64_t)first * cap1, (uint64_t)nb * cap2);
    uint64_t pass = (2ull << 30) / 8 / sstride; // <= 2 GiB of pool (0.2 GB for 64 queries over 10M docs)
    pass = std::max<uint64_t>(1, std::min<uint64_t>(pass, std::min<uint32_t>(B, oi_bm25_stream_pass_queries())));
    DevBuf &sp = ctx->buf("pool_bm_stream"), &sc = ctx->buf("pool_bm_stream_state");
    OI_CHECK(sp.ensure(sizeof(uint64_t) * (size_t)pass * sstride));
    const size_t swords = PoolWords::count((uint32_t)pass, nb);
    OI_CHECK(sc.ensure(sizeof(uint32_t) * swords));
    for (uint32_t q0 = 0; q0 < B; q0 += (uint32_t)pass) {
        const uint32_t nq = std::min<uint32_t>((uint32_t)pass, B - q0);
        const PoolWords w(sc.as<uint32_t>(), (uint32_t)pass);
        // (the plan launch also zeroes the pass's pool state, and writes the pass's thresholds)
        OI_CHECK(oi_launch_bm25_plan(idx, s.qt, s.qo, q0, nq, w.carry, swords, depth, (uint32_t)(w.tau - w.carry), (uint32_t)pass, floors));
        PoolView W1{sp.as<uint64_t>(), w.carry, w.seg, w.tau, sstride, carry_cap, cap1, first, nb, bm.overflow, s.filt, s.attrs};
        OI_CHECK(oi_launch_bm25_stream(idx, s.qt, s.qo, q0, nq, depth, W1, 0, first));
        PoolView W2 = W1;
        if (first < nb) {
            OI_CHECK(oi_launch_select(ctx, W1, nq, depth, /*compact=*/true, nullptr, nullptr, nullptr, depth));
            W2.seg_cap = cap2; W2.n_segs = nb; // the first phase's segments are empty again: the same memory, cut anew
            OI_CHECK(oi_launch_bm25_stream(idx, s.qt, s.qo, q0, nq, depth, W2, first, nb));
        }
        OI_CHECK(oi_launch_select(ctx, W2, nq, depth, false, s.bm_s + (size_t)q0 * depth, s.bm_d + (size_t)q0 * depth, s.bm_c + q0, depth));
    }
    return OI_OK;
}
// The wave-per-task kernel (bm25_wave.hip).  Two phases like the cosine chunks: the first eighth of the doc blocks is scored with
// no threshold (every touched doc is a candidate) and fixes tau_q = the depth-th score so far, a lower bound of the final one; the
// remaining blocks emit only scores >= tau_q.  A task's pool segment holds a whole block, so nothing can overflow; the room is
// address space, not traffic (only emitted keys are written).  Queries go in passes sized from a 6 GiB pool budget.
int bm25_wave(const Search &s, const PoolView &bm) {
    oi_index *idx = s.idx; oi_ctx *ctx = s.ctx;
    const uint32_t B = s.B, depth = s.depth, carry_cap = OI_MAX_DEPTH, nb = idx->n_blocks;
    if (nb == 0 || idx->n_postings == 0) {
        OI_HIP_CHECK(hipMemsetAsync(s.bm_c, 0, sizeof(uint32_t) * B, ctx->stream));
        return OI_OK;
    }
    const uint64_t wstride = (uint64_t)carry_cap + (uint64_t)nb * OI_BM25_BLOCK_DOCS;
    uint64_t pass = (6ull << 30) / 8 / wstride;
    pass = std::max<uint64_t>(1, std::min<uint64_t>(pass, std::min<uint32_t>(B, oi_bm25_wave_pass_queries())));
    DevBuf &wp = ctx->buf("pool_bm_wave"), &wc = ctx->buf("pool_bm_wave_state");
    OI_CHECK(wp.ensure(sizeof(uint64_t) * (size_t)pass * wstride));
    const size_t wwords = PoolWords::count((uint32_t)pass, nb);
    OI_CHECK(wc.ensure(sizeof(uint32_t) * wwords));
    const uint32_t first = nb > 16 ? std::max<uint32_t>(8, nb / 8) : nb;
    for (uint32_t q0 = 0; q0 < B; q0 += (uint32_t)pass) {
        const uint32_t nq = std::min<uint32_t>((uint32_t)pass, B - q0);
        OI_HIP_CHECK(hipMemsetAsync(wc.p, 0, sizeof(uint32_t) * wwords, ctx->stream));
        const PoolWords w(wc.as<uint32_t>(), (uint32_t)pass);
        PoolView W{wp.as<uint64_t>(), w.carry, w.seg, w.tau, wstride, carry_cap, OI_BM25_BLOCK_DOCS, nb, nb, bm.overflow};
        OI_CHECK(oi_launch_bm25_wave(idx, s.qt, s.qo, q0, nq, W, 0, first));
        if (first < nb) {
            OI_CHECK(oi_launch_select(ctx, W, nq, depth, /*compact=*/true, nullptr, nullptr, nullptr, depth));
            OI_CHECK(oi_launch_bm25_wave(idx, s.qt, s.qo, q0, nq, W, first, nb));
        }
        OI_CHECK(oi_launch_select(ctx, W, nq, depth, false, s.bm_s + (size_t)q0 * depth, s.bm_d + (size_t)q0 * depth, s.bm_c + q0, depth));
    }
    return OI_OK;
}
// Term-at-a-time, one WORKGROUP per doc block (the first-generation kernel, bm25.hip).  Two phases, like the cosine chunks: the
// first eighth of the doc blocks fixes a per-query threshold (the depth-th score seen so far is a lower bound of the final one);
// the remaining blocks then emit only candidates at or above it, so the final selection scans little.  Its segments are the
// depth-sized ones of the search's BM25 pool.
int bm25_taat(const Search &s, const PoolView &bm) {
    const uint32_t nb = s.idx->n_blocks;
    const uint32_t first = nb > 16 ? std::max<uint32_t>(8, nb / 8) : nb;
    OI_CHECK(oi_launch_bm25(s.idx, s.qt, s.qo, s.B, s.depth, bm, 0, first));
    if (first < nb) {
        OI_CHECK(oi_launch_select(s.ctx, bm, s.B, s.depth, /*compact=*/true, nullptr, nullptr, nullptr, s.depth));
        OI_CHECK(oi_launch_bm25(s.idx, s.qt, s.qo, s.B, s.depth, bm, first, nb));
    }
    return oi_launch_select(s.ctx, bm, s.B, s.depth, false, s.bm_s, s.bm_d, s.bm_c, s.depth);
}
// Batch scan of the forward index (bm25_scan.hip): the whole batch in passes of up to 1024 / max_query_terms queries; docs in
// chunks sized from the pool's free room, the first chunk (1/8 of the docs) fixing the thresholds -- a rule of its own, not the
// cosine leg's schedule.  Same worst-case rule as the cosine pools: a chunk can append at most one entry per doc and query.
int bm25_scan(const Search &s, const PoolView &bm) {
    oi_index *idx = s.idx; oi_ctx *ctx = s.ctx;
    const uint64_t n = idx->n_docs;
    const uint32_t B = s.B, depth = s.depth, carry_cap = OI_MAX_DEPTH;
    const uint32_t segs = 2u * (uint32_t)ctx->num_cus;
    const uint64_t sslack = 1024ull * (segs + 1); // oi_bm25_scan_geometry: a workgroup's docs, rounded up by two tiles
    uint64_t sstride = carry_cap + std::min<uint64_t>(n, 1ull << 23) + sslack;
    const uint64_t sbudget = (4ull << 30) / 8 / B;
    if (sstride > sbudget) sstride = std::max<uint64_t>(sbudget, carry_cap + 4 * sslack);
    DevBuf &sp = ctx->buf("pool_bm_scan"), &sc = ctx->buf("pool_bm_scan_state");
    OI_CHECK(sp.ensure(sizeof(uint64_t) * (size_t)B * sstride));
    const size_t swords = PoolWords::count(B, segs);
    OI_CHECK(sc.ensure(sizeof(uint32_t) * swords));
    OI_HIP_CHECK(hipMemsetAsync(sc.p, 0, sizeof(uint32_t) * swords, ctx->stream));
    const PoolWords w(sc.as<uint32_t>(), B);
    PoolView SP{sp.as<uint64_t>(), w.carry, w.seg, w.tau, sstride, carry_cap, 0, 0, segs, bm.overflow};
    const uint64_t max_chunk = sstride - carry_cap - sslack;
    const uint32_t pass = oi_bm25_scan_pass_queries(idx->max_query_terms);
    for (uint32_t q0 = 0; q0 < B; q0 += pass) {
        const uint32_t nq = std::min(pass, B - q0);
        PoolView V = SP;
        V.carry_cnt += q0; V.tau_keys += q0; // keys / seg_cnt are offset inside the kernel by q_begin
        uint64_t r = 0, chunk = std::max<uint64_t>(n / 8, 65536);
        while (r < n) {
            if (chunk > max_chunk) chunk = max_chunk;
            const uint64_t e = std::min(n, r + chunk);
            oi_bm25_scan_geometry(ctx, e - r, &V.n_segs, &V.seg_cap);
            SP.n_segs = V.n_segs; SP.seg_cap = V.seg_cap;
            OI_CHECK(oi_launch_bm25_scan(idx, s.qt, s.qo, q0, nq, r, e, idx->avgdl, /*run_setup=*/r == 0, SP));
            const bool last = e == n;
            PoolView S2 = SP; // select works on this pass's queries only
            S2.keys += (uint64_t)q0 * sstride; S2.carry_cnt += q0; S2.tau_keys += q0; S2.seg_cnt += (uint64_t)q0 * segs;
            OI_CHECK(oi_launch_select(ctx, S2, nq, depth, /*compact=*/!last, last ? s.bm_s + (size_t)q0 * depth : nullptr,
                                      last ? s.bm_d + (size_t)q0 * depth : nullptr, last ? s.bm_c + q0 : nullptr, depth));
            r = e;
            chunk = n; // everything that is left, as far as the pool allows
        }
    }
    return OI_OK;
}
// Which BM25 kernel: the plan's (oi_index_set_bm25_mode, or process-wide OI_BM25_MODE=stream|wave|taat|scan; all four return
// bit-identical lists).  A scan of an index without forward tokens runs the stream kernel.
int bm25_leg(const Search &s, const Plan &p, const PoolView &bm) {
    OI_REQUIRE(s.idx->finalized, "search: index not finalized");
    return p.bm25 == BM25_TAAT ? bm25_taat(s, bm) : p.bm25 == BM25_SCAN ? bm25_scan(s, bm) : p.bm25 == BM25_WAVE ? bm25_wave(s, bm)
                                                                                                               : bm25_stream(s, bm);
}
// The BM25 leg on the side stream, behind ctx->ev_fork (recorded by the caller on the ctx stream), joined through ctx->ev_join.
int fork_bm25(const Search &s, const Plan &p, const PoolView &bm) {
    oi_ctx *ctx = s.ctx;
    hipStream_t st = ctx->stream;
    OI_HIP_CHECK(hipStreamWaitEvent(ctx->side_stream, ctx->ev_fork, 0));
    ctx->stream = ctx->side_stream;
    const int rc = bm25_leg(s, p, bm);
    ctx->stream = st;
    if (rc != OI_OK) { (void)hipStreamSynchronize(ctx->side_stream); return rc; } // nothing of this call stays in flight
    OI_HIP_CHECK(hipEventRecord(ctx->ev_join, ctx->side_stream));
    return OI_OK;
}

// ---------------------------------------------------------------- cosine leg
// bf16 corpus: the same chunk schedule; a workgroup's segment is rounded up to four tiles per wave round
int cosine_bf16(const Search &s, const Plan &p, PoolView C) {
    oi_index *idx = s.idx;
    C.filt = s.filt; C.attrs = s.attrs; // (filtered: oi_launch_cosine_bf16_chunk pins the search to cosine_bf16_filter)
    const uint64_t bslack = 128ull * ((uint64_t)s.ctx->num_cus + 1), room = p.cos_stride - OI_MAX_DEPTH;
    const uint64_t max_chunk = room > bslack ? room - bslack : 0;
    if (max_chunk == 0) { oi_set_error("search: cosine pool too small"); return OI_ERR_STATE; }
    for (const Chunk &c : chunk_schedule(idx->n_docs, oi_first_chunk_rows(s.depth), oi_chunk_growth(s.B), max_chunk, true)) {
        OI_CHECK(oi_launch_cosine_bf16_chunk(s.ctx, idx->rows_bf16, c.r, c.e, idx->dim, s.qv, s.B, idx->doc_id_base, C));
        const bool last = c.e == idx->n_docs;
        OI_CHECK(oi_launch_select(s.ctx, C, s.B, s.depth, /*compact=*/!last, last ? s.cos_s : nullptr,
                                  last ? s.cos_d : nullptr, last ? s.cos_c : nullptr, s.depth));
    }
    return OI_OK;
}
// The exact pipeline over the f32 rows (q: the queries padded to Bp).  With a gate and the screen's thresholds it is the fallback
// behind the bf16 screen: tau~ - 2 eps is a valid lower bound of the exact k'-th score even when the survivors did not fit, so the
// exact kernel takes all rows in ONE launch (as many as the pool holds) -- two launches that exit at once when the gate is shut.
int cosine_exact(const Search &s, PoolView X, const float *q, uint32_t Bp, uint64_t max_chunk, const uint32_t *gate, uint32_t *screen_tau) {
    oi_index *idx = s.idx;
    SelectExtra ex; ex.run_gate = gate;
    if (screen_tau) X.tau_keys = screen_tau;
    X.filt = s.filt; X.attrs = s.attrs;
    const uint64_t first = gate ? max_chunk : oi_first_chunk_rows(s.depth);
    for (const Chunk &c : chunk_schedule(idx->n_docs, first, oi_chunk_growth(s.B), max_chunk, true)) {
        OI_CHECK(oi_launch_cosine_chunk(s.ctx, idx->rows, c.r, c.e, idx->dim, q, s.B, Bp, idx->doc_id_base, X, gate));
        const bool last = c.e == idx->n_docs;
        OI_CHECK(oi_launch_select(s.ctx, X, s.B, s.depth, /*compact=*/!last, last ? s.cos_s : nullptr,
                                  last ? s.cos_d : nullptr, last ? s.cos_c : nullptr, s.depth, gate ? &ex : nullptr));
    }
    return OI_OK;
}

// ---------------------------------------------------------------- the screen routes
// bf16 screen -> margin selects -> exact rescoring -> sorted selection; then the gated exact pipeline (cosine_prefilter.hip).
// Its pool keeps up to 4096 keys per query between chunks (OI_I8_CARRY on the int8 route).

// The screen's state words, zeroed with the pool state (prepare_pools: its extra words), in memory order:
//   carry_cnt[B] tau[B] rs_cnt[B] eps2[B] gate[4] seg_cnt[B][segs] spec_tau[B] spec_max[B]
// search_lists_device sizes them with count(), cosine_screen carves them with the constructor: the one place that lays them out.
uint32_t screen_segs(const oi_ctx *ctx) { return (uint32_t)ctx->num_cus; } // a segment per workgroup of the widest screen launch
struct ScreenWords {
    uint32_t *pf_cnt, *pf_tau, *rs_cnt;
    float *eps2;
    uint32_t *gate, *pf_seg, *spec_tau, *spec_max;
    static size_t count(uint32_t B, uint32_t segs) { return (size_t)B * (6 + (size_t)segs) + 4; }
    ScreenWords(uint32_t *w, uint32_t B, uint32_t segs) {
        uint32_t *const end = w + count(B, segs);
        auto take = [&w](size_t words) { uint32_t *at = w; w += words; return at; };
        pf_cnt = take(B);
        pf_tau = take(B);
        rs_cnt = take(B);
        eps2 = reinterpret_cast<float *>(take(B));
        gate = take(4);
        pf_seg = take((size_t)B * segs);
        spec_tau = take(B);
        spec_max = take(B);
        assert(w == end); // a field added here and not to count() (or the reverse) stops the first search
        (void)end;
    }
};

// What the stages of one screened search share, passed by reference (nothing of it lives on the ctx).
struct ScreenRun {
    ScreenWords w;
    PoolView PF{}, RS{}; // the screen's view of the cosine pool buffer; the rescored survivors
    // the margin selects: mx the bf16 screen's (uniform margin w.eps2: the chunks of the bf16 routes, the final one of the int8
    // route), m8 the chunks' -- the int8 tier's per-row margins on that route, a copy of mx on the others
    SelectExtra mx, m8;
    uint16_t *qb = nullptr; // the staged query blocks: bf16, and the int8 tier's (hi / lo planes, four floats per query)
    int8_t *qi8 = nullptr;
    float *qf8 = nullptr;
    // Speculative thresholds (the plan's spec and schedule): the next chunk is screened against the larger of the proven
    // threshold and a prediction from the rows seen so far, checked at the end (a failed check opens the gate).
    bool spec_next = false, spec_any = false;
    explicit ScreenRun(const ScreenWords &words) : w(words) {}
};

// The staging launch of a route: the bf16 query block, the margins and the gate; the int8 route stages both tiers' blocks in one.
int screen_stage(const Search &s, const Plan &p, ScreenRun &R) {
    oi_index *idx = s.idx;
    const uint32_t *norms = idx->max_row_norm.as<uint32_t>();
    switch (p.cos) {
        case CosRoute::screen_f32:
        case CosRoute::screen_copy:
            return oi_launch_screen_stage(s.ctx, s.qv, s.B, idx->dim, norms, R.qb, R.w.eps2, R.w.gate);
        case CosRoute::screen_i8:
            return oi_launch_screen_stage_i8(s.ctx, s.qv, s.B, idx->dim, norms, idx->screen_i8.as<uint8_t>(), idx->n_docs, R.qi8, R.qf8,
                                             R.w.gate, R.qb, R.w.eps2,
                                             // (the residual tier's margin over the bf16 screen's, which has no reader on that tail)
                                             p.rescreen_residual ? idx->screen_i8r.as<uint8_t>() : nullptr,
                                             p.rescreen_residual ? R.w.eps2 : nullptr);
        default:
            oi_set_error("search: not a screen route");
            return OI_ERR_STATE;
    }
}
// The screen launch of one chunk: the same products, the same bound on the two bf16 routes -- only where bf16(x) comes from differs
// (converted on the fly from the f32 rows, 4 d bytes per row, or read from the copy, 2 d bytes per row); the int8 first tier
// (cosine_screen_i8.hip) streams the int8 copy against per-row bounds.  Sets R.PF's segments for the chunk's select.
int screen_launch_chunk(const Search &s, const Plan &p, ScreenRun &R, const Chunk &c) {
    oi_index *idx = s.idx;
    switch (p.cos) {
        case CosRoute::screen_f32:
            return oi_launch_cosine_screen_chunk(s.ctx, idx->rows, c.r, c.e, idx->dim, R.qb, s.B, idx->doc_id_base, R.PF);
        case CosRoute::screen_copy:
            return oi_launch_cosine_screen_copy_chunk(s.ctx, idx->screen_copy.as<uint16_t>(), c.r, c.e, idx->dim, R.qb, s.B, idx->doc_id_base, R.PF);
        case CosRoute::screen_i8:
            return oi_launch_cosine_screen_i8_chunk(s.ctx, idx->screen_i8.as<uint8_t>(), idx->n_docs, c.r, c.e, idx->dim, R.qi8, R.qf8, s.B,
                                                    idx->doc_id_base, R.PF, p.screen_wgs);
        default:
            oi_set_error("search: not a screen route");
            return OI_ERR_STATE;
    }
}

// Open: the workspace buffers and the pool views, the route's staging launch, a missing bf16 copy, the margin selects' extras.
int screen_open(const Search &s, const Plan &p, const Pools &P, ScreenRun &R) {
    oi_index *idx = s.idx; oi_ctx *ctx = s.ctx;
    const uint64_t n = idx->n_docs;
    const uint32_t B = s.B, dim = idx->dim, segs = screen_segs(ctx), n_padded = (B + 31u) & ~31u;
    const bool i8 = p.cos == CosRoute::screen_i8;
    DevBuf &pk = ctx->buf("pool_cos"), &rk = ctx->buf("screen_rescored"), &qb = ctx->buf("screen_q_bf16");
    const uint32_t rs_cap = p.pf_carry + OI_LONG_ROWS_MAX; // the survivors and the index's long rows (two-class margin)
    OI_CHECK(rk.ensure(sizeof(uint64_t) * (size_t)B * rs_cap));
    OI_CHECK(qb.ensure(sizeof(uint16_t) * (size_t)(n_padded + 64) * dim));
    R.qb = qb.as<uint16_t>();
    R.PF = PoolView{pk.as<uint64_t>(), R.w.pf_cnt, R.w.pf_seg, R.w.pf_tau, p.pf_stride, p.pf_carry, 0, 0, segs, P.cos.overflow, s.filt, s.attrs};
    R.RS = PoolView{rk.as<uint64_t>(), R.w.rs_cnt, R.w.pf_seg, nullptr, rs_cap, rs_cap, 0, 0, segs, P.cos.overflow, s.filt, s.attrs};
    R.mx.eps2 = R.w.eps2; R.mx.margin_gate = R.w.gate;
    if (idx->n_long) { R.mx.skip_bitmap = idx->long_bitmap.as<uint32_t>(); R.mx.skip_base = idx->doc_id_base; }
    R.m8 = R.mx;
    // The int8 first tier (cosine_screen_i8.hip): the chunks stream the int8 copy against per-row bounds, the
    // margin selects keep up to OI_I8_CARRY lower-bound keys per query (an overflow opens the gate), the speculation works on
    // those keys; after the last chunk the survivors get their second-tier keys and the bf16 screen's final margin select,
    // rescoring and gate follow unchanged.
    if (i8) {
        DevBuf &qs = ctx->buf("screen_q_i8"), &cb = ctx->buf("screen_i8_cand");
        const size_t qi8_bytes = ((2 * (size_t)n_padded * dim) + 255) & ~(size_t)255;
        OI_CHECK(qs.ensure(qi8_bytes + sizeof(float) * 4 * (size_t)n_padded));
        OI_CHECK(cb.ensure(sizeof(uint64_t) * (size_t)B * OI_I8_CARRY));
        R.qi8 = reinterpret_cast<int8_t *>(qs.p);
        R.qf8 = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(qs.p) + qi8_bytes);
        R.m8.eps2 = R.qf8 + 3 * (size_t)n_padded; R.m8.row_qn = R.qf8 + (size_t)n_padded; R.m8.row_cq = R.qf8 + 2 * (size_t)n_padded;
        R.m8.cand = cb.as<uint64_t>(); R.m8.cand_cap = OI_I8_CARRY;
        R.m8.row_meta = reinterpret_cast<const float *>(idx->screen_i8.as<uint8_t>() + oi_screen_i8_meta_offset(n, dim));
        R.m8.meta_base = idx->doc_id_base;
    }
    OI_CHECK(screen_stage(s, p, R));
    if (p.cos == CosRoute::screen_copy && !idx->screen_copy.p) { // made once, on the first search that asks for it (n x d x 2 B of HBM)
        OI_CHECK(idx->screen_copy.ensure(sizeof(uint16_t) * (size_t)n * dim + 64));
        OI_CHECK(oi_launch_make_screen_copy(ctx, idx->rows, n, dim, idx->screen_copy.as<uint16_t>()));
    }
    return OI_OK;
}
// The plan's sample pass (int8 route): the first prediction before any chunk is pooled (the proven thresholds are still 0).
int screen_sample(const Search &s, const Plan &p, ScreenRun &R) {
    oi_index *idx = s.idx; oi_ctx *ctx = s.ctx;
    const uint64_t n = idx->n_docs;
    const uint32_t B = s.B, n_padded = (B + 31u) & ~31u;
    // The dense key array lies at the head of the pool buffer (ctx->buf "pool_cos": 7.3 MB of it at 10M x 768, B = 64): the pool
    // holds nothing yet -- no carried key, no segment -- and the first chunk, which writes it, starts behind the rank launch.
    const uint32_t ks = oi_screen_i8_sample_stride(p.sample_rows);
    OI_REQUIRE(sizeof(uint32_t) * (size_t)n_padded * ks <= sizeof(uint64_t) * (size_t)B * p.pf_stride && R.PF.keys,
               "search: the sample pass's keys do not fit the candidate pool");
    uint32_t *sample_keys = reinterpret_cast<uint32_t *>(R.PF.keys);
    OI_CHECK(oi_launch_screen_i8_sample(ctx, idx->screen_i8.as<uint8_t>(), n, p.sample_rows, idx->dim, R.qi8, R.qf8, B,
                                        idx->n_long ? idx->long_bitmap.as<uint32_t>() : nullptr, sample_keys));
    const uint64_t rank = (3ull * s.depth * p.sample_rows + n - 1) / n + 12;
    OI_CHECK(oi_launch_sample_rank(ctx, sample_keys, ks, p.sample_rows, B, (uint32_t)rank, R.m8.eps2, R.w.pf_tau, R.w.spec_tau, R.w.spec_max));
    R.spec_next = R.spec_any = true;
    return OI_OK;
}
// Chunk i of the plan's schedule: its screen launch, the late or tail fork of the BM25 leg, its margin select with the prediction
// for the next chunk.
int screen_chunk(const Search &s, const Plan &p, const Pools &P, ScreenRun &R, size_t i) {
    oi_ctx *ctx = s.ctx;
    const uint64_t n = s.idx->n_docs, e = p.screen_chunks[i].e;
    const bool last = i + 1 == p.screen_chunks.size();
    if (p.late_fork && !p.tail_fork && last) OI_HIP_CHECK(hipEventRecord(ctx->ev_fork, ctx->stream)); // (before the last chunk's launch)
    uint32_t *const proven_tau = R.PF.tau_keys;
    if (R.spec_next) R.PF.tau_keys = R.w.spec_tau; // (this launch only: the selects keep the proven thresholds)
    const int rc_screen = screen_launch_chunk(s, p, R, p.screen_chunks[i]);
    R.PF.tau_keys = proven_tau;
    OI_CHECK(rc_screen);
    ctx->last_screen_wgs = i ? std::max(ctx->last_screen_wgs, R.PF.n_segs) : R.PF.n_segs;
    // ... enqueued after it: the screen's workgroups get their CUs first.  tail_fork: the event is recorded here, behind the
    // launch, so the leg starts when the chunk ends and this chunk's margin select is the first kernel it runs beside.
    if (p.tail_fork && last) OI_HIP_CHECK(hipEventRecord(ctx->ev_fork, ctx->stream));
    if (p.late_fork && last) OI_CHECK(fork_bm25(s, p, P.bm));
    // The prediction for the next chunk rides in this chunk's margin select (select.hip), which holds the carried keys in
    // registers.  expected rank of the final k'-th among the e rows seen: depth e / n; three times that plus twelve
    const uint64_t rank = (3ull * s.depth * e + n - 1) / n + 12;
    const bool spec_here = p.spec && !last && 2 * rank <= s.depth;
    SelectExtra sx = R.m8;
    if (spec_here) { sx.spec_rank = (uint32_t)rank; sx.spec_tau = R.w.spec_tau; sx.spec_max = R.w.spec_max; }
    OI_CHECK(oi_launch_select(ctx, R.PF, s.B, s.depth, /*compact=*/true, nullptr, nullptr, nullptr, s.depth, &sx));
    R.spec_next = spec_here;
    if (spec_here) {
        { ProfScope ps(ctx, "spec"); } // (the profile's "spec" spans count the predictions made: an empty one, the select made it)
        R.spec_any = true;
    }
    return OI_OK;
}
// The int8 route's second tier: the int8 survivors' second-tier keys (in place) -- their two-plane scores from the residual plane,
// or their bf16 screen scores from the bf16 copy -- then the bf16 screen's final margin select over them, with that tier's uniform
// margin (mx.eps2: staging wrote the residual tier's there); the int8 tier's proven thresholds stay (the speculation check and the
// gated exact pipeline read them).
int screen_second_tier(const Search &s, const Plan &p, ScreenRun &R) {
    oi_index *idx = s.idx; oi_ctx *ctx = s.ctx;
    if (p.rescreen_residual) {
        OI_CHECK(oi_launch_rescreen_residual(ctx, idx->screen_i8r.as<uint8_t>(), idx->screen_i8.as<uint8_t>(), idx->n_docs, idx->dim,
                                             idx->doc_id_base, R.qi8, R.qf8, s.B, R.PF));
    } else {
        OI_CHECK(oi_launch_rescreen_bf16(ctx, idx->screen_copy.as<uint16_t>(), idx->n_docs, idx->dim, idx->doc_id_base, R.qb, s.B, R.PF));
    }
    PoolView PB = R.PF; PB.tau_keys = nullptr; PB.n_segs = 0;
    OI_CHECK(oi_launch_select(ctx, PB, s.B, s.depth, /*compact=*/true, nullptr, nullptr, nullptr, s.depth, &R.mx));
    ctx->last_rescreen_cnt = R.w.pf_cnt; ctx->last_rescreen_b = s.B;
    return OI_OK;
}
// Finish: exact rescoring of the survivors, the final sorted select, then the gated exact pipeline over the pool's own view.
int screen_finish(const Search &s, const Plan &p, const Pools &P, ScreenRun &R, const float *q, uint32_t Bp, uint64_t max_chunk) {
    oi_index *idx = s.idx; oi_ctx *ctx = s.ctx;
    PoolView PR = R.PF; // what the rescoring reads: the bf16 screen's final survivors (<= 4096 per query)
    if (p.cos == CosRoute::screen_i8) PR.carry_cap = 4096;
    // (the check of the speculative thresholds against the proven final ones rides in the rescoring launch; the gated exact
    // pipeline is enqueued after it)
    OI_CHECK(oi_launch_rescore(ctx, idx->rows, idx->n_docs, idx->dim, idx->doc_id_base, s.qv, s.B, PR, R.RS,
                               idx->n_long ? idx->long_list.as<uint32_t>() : nullptr, idx->n_long,
                               R.spec_any ? R.w.spec_max : nullptr, R.w.pf_tau, R.w.gate, ctx->spec_fail_host,
                               // behind the residual tier about k' + 7 % survivors per query (10M x 768, k' = 1000: 1 072, at most
                               // 1 094): 72 workgroups take 1 152 in ONE trip, 64 send a few waves on a second (48 -> 40 us)
                               p.rescreen_residual ? 72u : 0u));
    R.RS.n_segs = 0;
    OI_CHECK(oi_launch_select(ctx, R.RS, s.B, s.depth, false, s.cos_s, s.cos_d, s.cos_c, s.depth));
    ctx->last_screen_gate = R.w.gate;
    return cosine_exact(s, P.cos, q, Bp, max_chunk, R.w.gate, R.w.pf_tau);
}
// One screened search, stage by stage; `w`: its zeroed state words (ScreenWords::count of them).
int cosine_screen(const Search &s, const Plan &p, const Pools &P, uint32_t *w, const float *q, uint32_t Bp, uint64_t max_chunk) {
    ScreenRun R(ScreenWords(w, s.B, screen_segs(s.ctx)));
    OI_CHECK(screen_open(s, p, P, R));
    if (p.sample_rows) OI_CHECK(screen_sample(s, p, R));
    for (size_t i = 0; i < p.screen_chunks.size(); ++i) OI_CHECK(screen_chunk(s, p, P, R, i));
    if (R.spec_any) ++s.ctx->spec_searches;
    if (p.cos == CosRoute::screen_i8) OI_CHECK(screen_second_tier(s, p, R));
    return screen_finish(s, p, P, R, q, Bp, max_chunk);
}

int cosine_leg(const Search &s, const Plan &p, const Pools &P, uint32_t *screen_state) {
    if (p.cos == CosRoute::none) return OI_OK;
    if (p.cos == CosRoute::bf16) return cosine_bf16(s, p, P.cos);
    oi_index *idx = s.idx; oi_ctx *ctx = s.ctx;
    OI_REQUIRE(idx->rows, "search: embeddings not set");
    const uint32_t Bp = oi_cosine_query_padding(s.B);
    const float *q = s.qv;
    if (Bp != s.B) {
        DevBuf &qp = ctx->buf("q_padded");
        OI_CHECK(qp.ensure(sizeof(float) * (size_t)Bp * idx->dim));
        OI_HIP_CHECK(hipMemsetAsync(qp.p, 0, sizeof(float) * (size_t)Bp * idx->dim, ctx->stream));
        OI_HIP_CHECK(hipMemcpyAsync(qp.p, s.qv, sizeof(float) * (size_t)s.B * idx->dim, hipMemcpyDeviceToDevice, ctx->stream));
        q = qp.as<float>();
    }
    const uint64_t max_chunk = oi_cosine_max_chunk_rows(ctx, idx->dim, s.B, p.cos_stride, OI_MAX_DEPTH);
    if (max_chunk == 0) { oi_set_error("search: cosine pool too small"); return OI_ERR_STATE; }
    if (p.cos == CosRoute::exact) {
        ctx->last_screen_gate = nullptr; // (profile "screen_gate": -1 = this search was not screened)
        return cosine_exact(s, P.cos, q, Bp, max_chunk, nullptr, nullptr);
    }
    return cosine_screen(s, p, P, screen_state, q, Bp, max_chunk);
}

} // namespace

// A batch since the last look failed its speculation check (the rescoring launch writes *spec_fail_host): the next spec_backoff
// searches do not speculate, and spec_backoff doubles with each failure, from 16 up to 1024.
void oi_spec_take_failure(oi_ctx *ctx) {
    if (!ctx->spec_fail_host || !*ctx->spec_fail_host) return;
    *ctx->spec_fail_host = 0; ++ctx->spec_failures;
    ctx->spec_backoff = ctx->spec_backoff ? std::min(1024u, 2 * ctx->spec_backoff) : 16u;
    ctx->spec_skip = ctx->spec_backoff;
}
// Device-side ranked lists for a batch; all pointers device.
int search_lists_device(oi_index *idx, const float *d_qv, const uint32_t *d_qt, const uint32_t *d_qo, uint32_t B, uint32_t depth,
                        float *cos_s, uint32_t *cos_d, uint32_t *cos_c, float *bm_s, uint32_t *bm_d, uint32_t *bm_c,
                        const uint4 *d_filt, const uint2 *d_attrs) {
    oi_ctx *ctx = idx->ctx;
    const Search s{idx, ctx, d_qv, d_qt, d_qo, B, depth, cos_s, cos_d, cos_c, bm_s, bm_d, bm_c, d_filt, d_attrs};
    const Plan p = plan_search(s);
    ctx->last_sample_rows = p.sample_rows;
    ctx->last_rescreen_tier = p.cos == CosRoute::screen_i8 ? (p.rescreen_residual ? 1 : 0) : -1;
    ctx->last_rescreen_cnt = nullptr;
    Pools P;
    // the bf16 screen's state words (cosine_screen) ride in the same memset; the depth-sized segments of P.bm belong to the
    // workgroup-per-block kernel: no room is set aside for them otherwise
    const size_t screen_words = ScreenWords::count(B, screen_segs(ctx));
    uint32_t *screen_state = nullptr;
    OI_CHECK(prepare_pools(ctx, B, std::max<uint64_t>(p.cos_stride, idx->rows_bf16 ? 0ull : p.pf_stride), p.cos_stride, OI_MAX_DEPTH,
                           p.bm25 == BM25_TAAT ? idx->n_blocks : 0, depth, &P, screen_words, &screen_state));
    if (p.overlap && !p.late_fork) {
        OI_HIP_CHECK(hipEventRecord(ctx->ev_fork, ctx->stream)); // pools are reset, queries staged
        OI_CHECK(fork_bm25(s, p, P.bm));
    }
    const int rc = cosine_leg(s, p, P, screen_state);
    if (rc != OI_OK) { // nothing of this call stays in flight behind an error return
        if (p.overlap) (void)hipStreamSynchronize(ctx->side_stream);
        return rc;
    }
    if (p.overlap) OI_HIP_CHECK(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
    else if (bm_s) OI_CHECK(bm25_leg(s, p, P.bm));
    return OI_OK;
}
