// oi_internal.h -- shared host-side plumbing of libopenintel_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "openintel_hip.h"
#include "oi_stage_layout.h"

// ---------------------------------------------------------------- errors
void oi_set_error(const char *fmt, ...);

#define OI_HIP_CHECK(expr)                                                                   \
    do {                                                                                     \
        hipError_t oi_e_ = (expr);                                                           \
        if (oi_e_ != hipSuccess) {                                                           \
            oi_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(oi_e_), __FILE__, \
                         __LINE__);                                                          \
            return OI_ERR_HIP;                                                               \
        }                                                                                    \
    } while (0)

#define OI_CHECK(expr)              \
    do {                            \
        int oi_rc_ = (expr);        \
        if (oi_rc_ != OI_OK) return oi_rc_; \
    } while (0)

#define OI_REQUIRE(cond, ...)         \
    do {                              \
        if (!(cond)) {                \
            oi_set_error(__VA_ARGS__); \
            return OI_ERR_INVALID_ARG; \
        }                             \
    } while (0)

// ---------------------------------------------------------------- process-wide one-shots and build switches
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE property of a kernel: set once per (kernel, device),
// under a process-wide mutex -- contexts on different devices / host threads all pass through here (api.hip).
struct oi_ctx;
int oi_dyn_lds(oi_ctx *ctx, const void *kernel, size_t bytes);

// A/B switches, ablation builds ("timings only, results wrong by construction") and the first-generation kernels are
// reachable through environment variables ONLY in a -DOI_ABLATION build (tools/build_ablation.sh builds one
// with OI_EXTRA_HIPCC_FLAGS=-DOI_ABLATION).  The product build ignores them: a stray variable cannot change what
// the C ABI returns.  (OI_COSINE_MODE / OI_BM25_MODE select between documented, tested, equivalent modes and stay.)
#ifdef OI_ABLATION
inline const char *oi_ablation_env(const char *name) { return getenv(name); }
#else
inline const char *oi_ablation_env(const char *) { return nullptr; }
#endif

// ---------------------------------------------------------------- buffers
// Grow-only device buffer: the hot path never calls hipMalloc once warmed up.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool borrowed = false; // a view's alias of another index's buffer (oi_index_view): never freed, never resized here
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int ensure(size_t bytes);
    void release();
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// Page-locked host staging of a context (the OI_HOST entry points of the query path): the caller's pageable arrays are
// packed into it and moved with ONE DMA each way -- three pageable copies each way are staged by the runtime one after the
// other.  Every OI_HOST call ends with a stream synchronise inside the ctx mutex, so a buffer is free again at the next call.
#define OI_PINNED_STAGE_MAX ((size_t)1 << 20) // calls moving more than this use the caller's pageable arrays directly (measured: no gain above ~1 MB)
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool pinned = false; // false: hipHostMalloc refused, plain memory stands in (slower copies, same results)
    PinBuf() = default;
    PinBuf(const PinBuf &) = delete;
    PinBuf &operator=(const PinBuf &) = delete;
    int ensure(size_t bytes);
    void release();
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

struct ProfSpan {
    hipEvent_t a, b;
};

// Bumped whenever any DevBuf allocates, grows or is released: a captured launch sequence (below) holds raw workspace
// pointers and is only replayed while no workspace has moved since it was captured.
extern std::atomic<uint64_t> g_oi_ws_epoch;

// One device-buffer call of the query path (oi_search_lists_packed, oi_fuse_packed, oi_search: ~30 launches, memsets and
// event operations; 0.3 ms of host time at a 1.25M-row shard, where the GPU needs 0.7) captured into a hipGraph the second
// time it is made with the same arguments, and replayed with ONE launch call from then on (oi_set_graph_replay).
struct GraphEntry {
    uint64_t key[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t epoch = 0, last_use = 0;
    int state = 0; // 0 = seen once (ran eagerly: every workspace exists now), 1 = captured, 2 = not capturable (stays eager)
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
};

struct oi_ctx {
    // Lifetime: the caller's handle holds one reference and every oi_index created on / viewed through the ctx one more;
    // oi_destroy drops the caller's, the teardown runs when the last one goes (api.hip: ctx_release).  An index can
    // therefore always be destroyed, whatever became of its ctx handle.
    std::atomic<int> refs{1};
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;     // the BM25 leg of a hybrid query runs here, beside the cosine leg (made by the first hybrid search)
    bool side_stream_failed = false;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool overlap_legs = true;              // oi_set_overlap
    // speculative screen thresholds (oi_select_rank.h: sel_spec_words): on by default (oi_set_screen_speculation); a batch whose
    // speculation failed its check (the device writes *spec_fail_host) switches them off for spec_backoff searches, doubling up to 1024
    bool speculate = true;
    uint32_t spec_skip = 0, spec_backoff = 0;
    uint32_t *spec_fail_host = nullptr;    // 4 bytes of pinned host memory, written by pf_rescore_kernel when a check fails
    uint64_t spec_searches = 0, spec_failures = 0; // (diagnostics: profile "spec_state")
    int cosine_mode = 2;                   // oi_set_cosine_mode: 0 exact-f32 MFMA, 1 split-precision products, 2 screen + rescore (default),
                                           // 3 = 2 + make a missing screening copy on first use, 4 = 2 but never read the copy
    std::mutex mu;
    std::map<std::string, DevBuf> ws; // named workspaces
    int prof_enabled = 0; // 0 off, 1 every tagged launch, 2 the cosine scorer only
    const uint32_t *last_screen_gate = nullptr; // the gate word of the last screened search (diagnostics)
    uint32_t last_screen_wgs = 0;               // workgroups of the widest screen launch of the last screened search (diagnostics)
    uint32_t last_sample_rows = 0;              // rows of the last search's sample pass, 0 = it took none (diagnostics: "screen_sample")
    // the int8 route's second tier: the residual plane's rescreen where the index holds the plane (default), or the bf16 rescreen
    // whatever it holds (oi_internal_set_rescreen_tier: A/B runs and tests take both tails over one index)
    bool rescreen_residual = true;
    int last_rescreen_tier = -1;                // the last search's: 0 bf16, 1 residual, -1 no int8 route (diagnostics: "rescreen_tier")
    const uint32_t *last_rescreen_cnt = nullptr; // its survivor counts behind the second margin select, [last_rescreen_b] (diagnostics: "rescreen_survivors")
    uint32_t last_rescreen_b = 0;
    std::map<std::string, std::vector<ProfSpan>> prof;
    std::vector<hipEvent_t> event_pool;
    bool use_graphs = false;          // oi_set_graph_replay
    std::vector<GraphEntry> graphs;   // <= OI_MAX_GRAPHS, least recently used evicted
    uint64_t graph_clock = 0, graph_replays = 0, graph_captures = 0;

    PinBuf pin_in, pin_out;

    DevBuf &buf(const char *name) { return ws[name]; }
    void prof_begin(const char *tag);
    void prof_end(const char *tag);
};

struct ProfScope {
    oi_ctx *c;
    const char *tag;
    bool on;
    ProfScope(oi_ctx *ctx, const char *t) : c(ctx), tag(t) {
        on = c->prof_enabled == 1 || (c->prof_enabled == 2 && strcmp(t, "cosine") == 0);
        if (on) c->prof_begin(tag);
    }
    ~ProfScope() {
        if (on) c->prof_end(tag);
    }
};

#define OI_BM25_FLOOR_RANKS 4
// ---------------------------------------------------------------- index
struct oi_index {
    uint64_t uid = 0;         // process-unique (graph cache keys: an address can be reused, a uid cannot)
    std::atomic<int> refs{1}; // the caller's handle + one per live view (a view borrows this index's buffers)
    oi_index *src = nullptr;  // a view: the index whose buffers it borrows (holds a reference on it)
    oi_ctx *ctx = nullptr;    // holds a reference
    uint64_t n_docs = 0;
    uint32_t dim = 0, vocab = 0, doc_id_base = 0;

    // embeddings
    float *rows = nullptr; // device
    bool rows_owned = false;
    uint16_t *rows_bf16 = nullptr; // device; set instead of `rows` for a bf16 corpus
    bool rows_bf16_owned = false;
    DevBuf max_row_norm; // u32[2]: bits of X = max_r |row r| and E = max_r |bf16(row r) - row r| (f32), taken when the f32 rows
                         // are set; NaN if any norm is
    bool screen_ok = false; // those maxima are finite and < 1e15: the bf16 screen's bound holds for this corpus
    // Two classes of rows (cosine_prefilter.hip): n_long > 0 = the maxima above are those of the rows that are NOT long; the
    // long ones are listed (local row numbers), marked in a bitmap, skipped by the margin selects and always rescored
    uint32_t n_long = 0;
    DevBuf long_list, long_bitmap;
    DevBuf screen_copy;     // the bf16 screening copy: bf16(rows), n_docs x dim x 2 B, made at finalize when the policy allows
    int screen_copy_policy = -1; // oi_index_set_screen_copy; -1 = the process default (OI_SCREEN_COPY, else AUTO)
    // the int8 screening copy (cosine_screen_i8.hip), made and dropped together with the bf16 one: i8 rows (n_docs x dim B,
    // per-row absmax scale) then, 256-B aligned, f32 {scale, e_r} per row (+ 64 rows of zero padding) and bits of max e_r over
    // the rows that are not long
    DevBuf screen_i8;
    // the residual plane of the int8 copy (screen_i8_residual.hip): what the first plane's rounding left over, in the same layout
    // ({t_r, e2_r} per row, the bits of e2_max).  Made, dropped and aliased with the int8 copy; the first of the three copies the
    // AUTO budget leaves out -- an index without it takes the bf16 rescreen
    DevBuf screen_i8r;
    // the doc attributes of filtered searches (oi_index_set_doc_attrs): {group, stamp} per local row, n_docs x 8 B; allocated
    // by the first call, overwritten in place by later ones (never reallocated: views alias it)
    DevBuf doc_attrs;
    // the signal records of oi_similar_summary (oi_index_set_signals): {pol_q30, class + 3 spec + 6 source} per local row,
    // n_docs x 8 B; the same allocation rules as doc_attrs (views alias it)
    DevBuf signals;

    // staged forward index (between set_forward and finalize)
    bool forward_set = false, finalized = false;
    uint64_t total_tokens = 0;  // local
    uint64_t n_postings = 0;    // unique (doc, term) pairs
    uint32_t n_blocks = 0;      // ceil(n_docs / OI_BM25_BLOCK_DOCS)
    uint32_t n_win = 0;         // 2 * n_blocks: windows of OI_BM25_FINE_DOCS docs (the cells of a term's posting list)
    DevBuf uniq_keys;           // u64 (block | term | doc_in_block), sorted
    DevBuf tf;                  // u32 per unique key
    DevBuf doc_len;             // u32 per doc
    DevBuf df_local;            // u32 per term

    // finalized inverted index
    DevBuf postings;   // {u32 doc_in_block, f32 impact} per unique key, (term, doc) order: one contiguous list per term
    DevBuf cell_start; // u32 [vocab * n_win + 1]: start of the (term, window) run; the next entry is its end
    DevBuf idf;        // f32 per term
    // u32 [vocab][OI_BM25_FLOOR_RANKS] (round 4): bits of a lower bound of the term's r-th largest posting impact, r = 16, 64,
    // 256, 1024 (0: fewer than r postings).  A query's first BM25 threshold is read off this table (bm25_stream.hip: the plan).
    DevBuf impact_floor;
    // forward index kept for the batch scan (bm25_scan.hip)
    DevBuf fwd_terms;   // u32 per token
    DevBuf fwd_offsets; // u64 per doc + 1
    float avgdl = 0.f;  // global average doc length fixed at finalize
    uint32_t max_query_terms = 16; // contract for the batch-scan path (oi_index_set_max_query_terms)
    int bm25_mode = 0;             // 0 default (= 4 unless OI_BM25_MODE says otherwise), 1 term-at-a-time per workgroup (bm25.hip),
                                   // 2 scan of the forward index (bm25_scan.hip), 3 term-at-a-time per wave (bm25_wave.hip),
                                   // 4 the stream kernel (bm25_stream.hip)
    bool is_view = false;          // oi_index_view: the data belongs to another index; this handle only searches
};

// search.hip: one hybrid search on the device (the entry points in api.hip stage the queries and copy the results)
// d_filt / d_attrs: a filtered search -- d_filt[B] the queries' {group_mask, group_value, stamp_lo, stamp_hi},
// d_attrs the index's {group, stamp} per local row; both null: the unfiltered search
int search_lists_device(oi_index *idx, const float *d_qv, const uint32_t *d_qt, const uint32_t *d_qo, uint32_t B, uint32_t depth,
                        float *cos_s, uint32_t *cos_d, uint32_t *cos_c, float *bm_s, uint32_t *bm_d, uint32_t *bm_c,
                        const uint4 *d_filt = nullptr, const uint2 *d_attrs = nullptr);
void oi_spec_take_failure(oi_ctx *ctx); // a failed speculation check seen since the last look: back off

// The two layouts the search entry points of api.hip share with pipeline.hip, each written once.
// Staged host queries [vectors | terms | offsets (| filters)], each part 16-byte aligned; nt = the batch's term count (qo[B]).
struct QueryLayout {
    size_t vb, ob, off_t, off_o, off_f, total; // bytes of the vectors / offsets, where the later parts start, bytes in all
    QueryLayout(uint32_t B, uint32_t dim, size_t nt, bool filters) {
        const auto r16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
        vb = sizeof(float) * (size_t)B * dim;
        ob = sizeof(uint32_t) * ((size_t)B + 1);
        off_t = r16(vb);
        off_o = off_t + r16(sizeof(uint32_t) * (nt ? nt : 1));
        off_f = off_o + r16(ob);
        total = filters ? off_f + sizeof(oi_doc_filter) * (size_t)B : off_o + ob;
    }
};
// The fused result block [scores K | docs K | counts B (| dup K)], K = B * k, contiguous in device or page-locked memory.
struct ResultBlock {
    float *scores;
    uint32_t *docs, *counts, *dup; // dup: null without the fourth section
    size_t K;
    uint32_t B, k;
    ResultBlock(void *p, uint32_t B_, uint32_t k_, bool with_dup = false) : scores(static_cast<float *>(p)), K((size_t)B_ * k_), B(B_), k(k_) {
        docs = reinterpret_cast<uint32_t *>(scores + K);
        counts = docs + K;
        dup = with_dup ? counts + B : nullptr;
    }
    ResultBlock at(void *p) const { return ResultBlock(p, B, k, dup != nullptr); } // the same sections over another buffer
    static size_t bytes(uint32_t B, uint32_t k, bool with_dup = false) { return ((with_dup ? 3 : 2) * (size_t)B * k + B) * 4; }
    size_t bytes() const { return ((dup ? 3 : 2) * K + B) * 4; }
    // a block in host memory to the caller's arrays (a null array is skipped)
    void to_arrays(float *scores_out, uint32_t *docs_out, uint32_t *counts_out, uint32_t *dup_out = nullptr) const {
        if (scores_out) memcpy(scores_out, scores, K * 4);
        if (docs_out) memcpy(docs_out, docs, K * 4);
        if (counts_out) memcpy(counts_out, counts, (size_t)B * 4);
        if (dup && dup_out) memcpy(dup_out, dup, K * 4);
    }
};

// a launch's filter argument: the host's filter by value, zeros without one (the kernels' filtered instantiations read it)
inline uint4 oi_filter_words(const oi_doc_filter *f) {
    return f ? make_uint4(f->group_mask, f->group_value, f->stamp_lo, f->stamp_hi) : make_uint4(0u, 0u, 0u, 0u);
}

// ---------------------------------------------------------------- kernels (host launchers)
// lexicon.hip
int oi_launch_lexicon(oi_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets, uint64_t n,
                      uint64_t blob_bytes, double *d_pol, uint8_t *d_spec);
int oi_launch_lexicon_fused(oi_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets, uint64_t n, uint64_t blob_bytes,
                            double *d_pol, uint8_t *d_spec, const uint8_t *d_sources, double tau, oi_social_counters *summary);
int oi_launch_social_summary(oi_ctx *ctx, const uint8_t *d_sources, const double *d_pol,
                             const uint8_t *d_spec, uint64_t n, double tau,
                             oi_social_counters *out_host);
int oi_launch_social_summary_segmented(oi_ctx *ctx, const uint8_t *d_sources, const double *d_pol, const uint8_t *d_spec,
                                       uint64_t n, const uint64_t *d_seg, uint64_t n_seg, double tau,
                                       oi_social_counters *d_out);
// headline.hip
int oi_launch_headline_scan(oi_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets, uint64_t n,
                            uint64_t blob_bytes, const uint8_t *ticker, uint64_t ticker_len,
                            const uint8_t *forms_blob, const uint32_t *form_offsets, uint32_t n_forms,
                            uint16_t *d_mask, uint64_t *d_order, uint8_t *d_about);
size_t oi_headline_params_bytes();
int oi_headline_build_params(void *dst, const uint8_t *ticker, uint64_t ticker_len, const uint8_t *forms_blob,
                             const uint32_t *form_offsets, uint32_t n_forms);
int oi_launch_headline_scan_params(oi_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets, uint64_t n,
                                   uint64_t blob_bytes, uint64_t text_bytes, const void *d_params, uint16_t *d_mask,
                                   uint64_t *d_order, uint8_t *d_about);
// select.hip
// Candidate pools, one per query, never touched by a global atomic in the batch kernels:
//   keys[q*stride + 0 .. carry_cap)                    the top-k carried over from earlier corpus chunks
//   keys[q*stride + carry_cap + s*seg_cap ..)          segment s: written by exactly one producer
//                                                      (cosine: workgroup s; BM25: doc block s)
//   carry_cnt[q], seg_cnt[q*seg_cnt_stride + s]        fill counts
struct PoolView {
    uint64_t *keys;
    uint32_t *carry_cnt;      // [n_queries]
    uint32_t *seg_cnt;        // [n_queries][seg_cnt_stride]
    uint32_t *tau_keys;       // [n_queries] orderable-u32 threshold (0 = accept all); may be null
    uint64_t stride;          // u64 entries between consecutive queries' pools
    uint32_t carry_cap;       // entries reserved for the carried top-k (>= k)
    uint32_t seg_cap;         // entries per segment
    uint32_t n_segs;          // segments in use
    uint32_t seg_cnt_stride;  // allocated segments per query
    uint32_t *overflow;       // single device word, set nonzero if a segment overflowed (bug guard)
    // a filtered search: filt[q] = query q's {group_mask, group_value, stamp_lo, stamp_hi}, offset with tau_keys;
    // attrs[row] = {group, stamp} of local row `row`.  Null: unfiltered (the kernels' unfiltered instantiations).
    const uint4 *filt = nullptr;
    const uint2 *attrs = nullptr;

    // The same pools seen from query q0 on (a launcher's pass over queries q0 .. q0 + 63): every per-query array moves,
    // a null tau_keys / filt stays null, geometry, overflow and attrs (per row) stay.
    PoolView for_queries(uint32_t q0) const {
        PoolView p = *this;
        p.keys += (uint64_t)q0 * stride;
        p.carry_cnt += q0;
        p.seg_cnt += (uint64_t)q0 * seg_cnt_stride;
        if (p.tau_keys) p.tau_keys += q0;
        if (p.filt) p.filt += q0;
        return p;
    }
};
// Optional behaviour of a select launch (cosine_prefilter.hip): eps2 != null = margin mode (keep every key within
// eps2[q] of the k-th score; needs compact, no sorted output, carry_cap >= 4096; an overflowing query sets
// *margin_gate); run_gate != null = the launch exits at once unless *run_gate is nonzero.
struct SelectExtra {
    const float *eps2 = nullptr;
    uint32_t *margin_gate = nullptr;
    const uint32_t *run_gate = nullptr;
    const uint32_t *skip_bitmap = nullptr; // margin mode: keys of docs whose bit (doc - skip_base) is set are left out of the selection
    uint32_t skip_base = 0;
    uint64_t *cand = nullptr; // margin mode: candidates staged here ([n_queries][cand_cap], global) instead of in LDS (4096 keys)
    uint32_t cand_cap = 0;
    // margin mode with per-row margins (the int8 tier): {scale, e_r} per row (row = doc - meta_base), |q^| and c_q per query
    const float *row_meta = nullptr;
    uint32_t meta_base = 0;
    const float *row_qn = nullptr, *row_cq = nullptr;
    // margin mode: the speculative threshold rides in the select (oi_select_rank.h: sel_spec_words, from the r-th largest of the
    // keys the select holds): spec_rank = r > 0 and both pointers set
    uint32_t spec_rank = 0;
    uint32_t *spec_tau = nullptr, *spec_max = nullptr;
};
int oi_launch_select(oi_ctx *ctx, const PoolView &pool, uint32_t n_queries, uint32_t k, bool compact,
                     float *out_scores, uint32_t *out_docs, uint32_t *out_counts, uint32_t out_stride,
                     const SelectExtra *extra = nullptr);
// shard s's lists start at scores + s*shard_stride (same for docs) and counts + s*count_stride
int oi_launch_lists_to_pool(oi_ctx *ctx, const float *scores, const uint32_t *docs,
                            const uint32_t *counts, uint64_t shard_stride, uint64_t count_stride,
                            uint32_t n_shards, uint32_t n_queries, uint32_t depth, const PoolView &pool);
int oi_launch_rrf(oi_ctx *ctx, const uint32_t *docs_a, const uint32_t *counts_a, const uint32_t *docs_b,
                  const uint32_t *counts_b, uint32_t n_queries, uint32_t depth, uint32_t k,
                  float *scores_out, uint32_t *docs_out, uint32_t *counts_out);
// collapse.hip: the near-duplicate collapse of ranked lists -- device lists in and out, asynchronous on the ctx
// stream; d_scores / scores_out and dup_out may be null
int oi_launch_collapse(oi_index *idx, const float *d_scores, const uint32_t *d_docs, const uint32_t *d_counts, uint32_t n_queries,
                       uint32_t depth, float threshold, uint32_t k, float *scores_out, uint32_t *docs_out, uint32_t *counts_out,
                       uint32_t *dup_out);
// cosine_volume.hip: the similarity volume -- device queries / filters in, device counts [n_queries][n_buckets]
// out, asynchronous on the ctx stream; d_filt may be null
int oi_launch_similar_volume(oi_index *idx, const float *d_q, uint32_t n_queries, const oi_volume_spec &spec, const uint4 *d_filt,
                             uint32_t *d_counts);
// the bf16 corpus's rounding of the queries (cb_stage_queries: RNE, inf / NaN truncated), widened back to f32 for the chain
int oi_launch_volume_round_queries(oi_ctx *ctx, const float *d_q, uint64_t total, float *d_out);
// cosine_summary.hip: the similarity summary -- the pack kernel of oi_index_set_signals (device arrays in, the
// index's records out) and the call itself: device queries / thresholds / filters in, device records [n_queries][n_buckets]
// out, asynchronous on the ctx stream; d_thresholds (null: spec.threshold for every query) and d_filt may be null
int oi_launch_pack_signals(oi_ctx *ctx, const double *d_pol, const uint8_t *d_spec, const uint8_t *d_sources, uint64_t n, double tau,
                           uint2 *d_out);
int oi_launch_similar_summary(oi_index *idx, const float *d_q, uint32_t n_queries, const oi_summary_spec &spec, const float *d_thresholds,
                              const uint4 *d_filt, oi_social_counters *d_out);
// cosine_groups.hip: the similarity leaderboard -- device queries / thresholds / filters in; dense (spec.top == 0):
// device records [n_queries][n_keys] out; ranked: records and keys [n_queries][top], counts and (may be null) qualified
// [n_queries] out.  Asynchronous on the ctx stream; d_thresholds and d_filt may be null
int oi_launch_similar_groups(oi_index *idx, const float *d_q, uint32_t n_queries, const oi_groups_spec &spec, const float *d_thresholds,
                             const uint4 *d_filt, oi_social_counters *d_records, uint32_t *d_keys, uint32_t *d_counts,
                             uint32_t *d_qualified);
// cosine_share.hip: the similarity share -- the summary's arguments; device records [n_queries][n_buckets] and
// (may be null) labels [n_docs] by local row out.  Asynchronous on the ctx stream; d_thresholds and d_filt may be null
int oi_launch_similar_share(oi_index *idx, const float *d_q, uint32_t n_queries, const oi_summary_spec &spec, const float *d_thresholds,
                            const uint4 *d_filt, oi_social_counters *d_out, uint32_t *d_labels);
// mention.hip: the mention summary -- device terms / offsets / min_match / filters in, device records
// [n_queries][n_cells] out, asynchronous on the ctx stream; d_min_match (null: ANY) and d_filt may be null
int oi_launch_mention_summary(oi_index *idx, const uint32_t *d_terms, const uint32_t *d_offsets, uint32_t n_queries,
                              const oi_mention_spec &spec, const uint32_t *d_min_match, const uint4 *d_filt, oi_social_counters *d_out);
// centroids.hip: the update step of a clustering over the index, all asynchronous on the ctx stream -- device
// labels [n_docs] in, device sums [n_clusters][dim] and counts [n_clusters] out (zeroed by the launch); sums to unit vectors
// (d_previous may be null or d_out); d_out[0] = rows with d_cur != d_prev, d_out[1] = rows with a label
int oi_launch_label_sums(oi_index *idx, const uint32_t *d_labels, uint32_t n_clusters, int64_t *d_sums, uint64_t *d_counts);
int oi_launch_centroids_from_sums(oi_ctx *ctx, const int64_t *d_sums, const uint64_t *d_counts, const float *d_previous,
                                  uint32_t n_clusters, uint32_t dim, float *d_out);
int oi_launch_fit_moved(oi_ctx *ctx, const uint32_t *d_cur, const uint32_t *d_prev, uint64_t n, uint64_t *d_out);
// seeds.hip: the seeding of that clustering -- device seeds [n_clusters][dim] and rows [n_clusters] (may be null)
// out, both preset by the launch; *d_info_out = the call's oi_seed_info in its workspace.  filter: a host pointer or null.
// Asynchronous on the ctx stream
int oi_launch_narratives_seed(oi_index *idx, uint32_t n_clusters, const oi_seed_spec &spec, const oi_doc_filter *filter, float *d_seeds,
                              uint32_t *d_rows, const void **d_info_out);
// label_terms.hip: the distinguishing terms of each cluster, all asynchronous on the ctx stream -- device labels
// [n_docs] in, device table [vocab][n_clusters] and sizes [n_clusters] out (zeroed by the launch); a device table and the sizes
// (the host's, passed by value, or with sizes_host == null the device's) to device records [n_clusters][top] and n [n_clusters],
// with oi_label_terms_rank_scratch() bytes of the caller's workspace behind `scratch`
int oi_launch_label_term_counts(oi_index *idx, const uint32_t *d_labels, uint32_t n_clusters, uint32_t *d_counts, uint64_t *d_sizes);
size_t oi_label_terms_rank_scratch(uint32_t vocab, uint32_t n_clusters, uint32_t top);
int oi_launch_label_terms_rank(oi_ctx *ctx, const uint32_t *d_counts, const uint64_t *sizes_host, const uint64_t *d_sizes, uint32_t vocab,
                               uint32_t n_clusters, uint32_t top, uint32_t min_df, void *scratch, oi_label_term *d_terms, uint32_t *d_n);
// label_exemplars.hip: the most central posts of each cluster -- device labels [n_docs] and centroids
// [n_clusters][dim] in, device scores / docs [n_clusters][top] and counts [n_clusters] out; `filter` is the host's (by value into
// the launch) or null.  Asynchronous on the ctx stream; its workspace is "exemplars".
int oi_launch_label_exemplars(oi_index *idx, const uint32_t *d_labels, const float *d_centroids, uint32_t n_clusters, uint32_t top,
                              const oi_doc_filter *filter, float *d_scores, uint32_t *d_docs, uint32_t *d_counts);
// cosine_groups.hip: the finish of a key-axis tally -- cells [n_cells / n_keys][n_keys] to dense records (top == 0) or to the
// ranked output (rank_keys: n_cells u64 of the caller's workspace; rank_tag: its profile tag).  Asynchronous on the ctx stream.
int oi_launch_groups_finish(oi_ctx *ctx, const uint32_t *cells, uint64_t n_cells, uint32_t n_keys, uint32_t top, uint32_t rank_by,
                            uint32_t min_total, uint64_t *rank_keys, const char *rank_tag, oi_social_counters *d_records, uint32_t *d_keys,
                            uint32_t *d_counts, uint32_t *d_qualified);
// label_summary.hip: the narrative breakdown -- device labels [n_docs] in; dense (spec.top == 0): device records
// [n_clusters][n_cells] out; ranked: records and keys [n_clusters][top], counts and (may be null) qualified [n_clusters] out;
// `filter` is the host's (by value into the launch) or null.  Asynchronous on the ctx stream; its workspace is "label_summary".
int oi_launch_label_summary(oi_index *idx, const uint32_t *d_labels, uint32_t n_clusters, const oi_label_summary_spec &spec,
                            const oi_doc_filter *filter, oi_social_counters *d_records, uint32_t *d_keys, uint32_t *d_counts,
                            uint32_t *d_qualified);
// cosine.hip
// Sets pool.n_segs / pool.seg_cap for this chunk (the following select must use the same view).
// run_gate != null: a launch of the gated exact pipeline behind a screen (search.hip: cosine_exact) -- the kernel exits at once
// unless *run_gate is nonzero, and the launch is profiled as "cosine_gated"; null: ungated, "cosine".
int oi_launch_cosine_chunk(oi_ctx *ctx, const float *rows, uint64_t row_begin, uint64_t row_end,
                           uint32_t dim, const float *d_queries_padded, uint32_t n_queries,
                           uint32_t n_queries_padded, uint32_t doc_id_base, PoolView &pool, const uint32_t *run_gate);
// Largest chunk (rows) that can never overflow a pool of `stride` entries per query.
uint64_t oi_cosine_max_chunk_rows(const oi_ctx *ctx, uint32_t dim, uint32_t n_queries, uint64_t stride,
                                  uint32_t carry_cap);
int oi_launch_l2_normalize(oi_ctx *ctx, float *rows, uint64_t n, uint32_t dim);
// cosine_split.hip
bool oi_cosine_split_supported(uint32_t dim);
int oi_launch_cosine_split(oi_ctx *ctx, const float *rows, uint64_t row_begin, uint64_t row_end, uint32_t dim,
                           const float *d_queries, uint32_t nq, uint32_t doc_id_base, const PoolView &p);
// cosine_bf16.hip
bool oi_cosine_bf16_supported(uint32_t dim);
int oi_launch_cosine_bf16_chunk(oi_ctx *ctx, const uint16_t *rows, uint64_t row_begin, uint64_t row_end, uint32_t dim,
                                const float *d_queries, uint32_t n_queries, uint32_t doc_id_base, PoolView &pool);
uint32_t oi_cosine_query_padding(uint32_t n_queries);
// cosine_ksplit.hip (the pool geometry of its chunks: oi_cosine_ksplit_geometry, oi_ksplit_tile.h)
bool oi_cosine_ksplit_supported(uint32_t dim);
// cosine_prefilter.hip: the bf16 screen + exact rescoring of an f32 corpus
bool oi_cosine_screen_supported(uint32_t dim);
// The bf16 screen (and the screening copies behind it) applies to this index's corpus: f32 rows of a dim the screen kernels are
// built for, with norms finite and small enough for its bound.
inline bool oi_index_screenable(const oi_index *idx) {
    return idx->rows && !idx->rows_bf16 && idx->screen_ok && oi_cosine_screen_supported(idx->dim);
}
void oi_cosine_screen_geometry(const oi_ctx *ctx, uint64_t n_rows, uint32_t *n_segs, uint32_t *seg_cap);
// ... at a width the caller chooses: at most `wgs` workgroups, 1 <= wgs <= ctx->num_cus (the plan's screen_wgs)
void oi_cosine_screen_geometry(const oi_ctx *ctx, uint64_t n_rows, uint32_t wgs, uint32_t *n_segs, uint32_t *seg_cap);
int oi_launch_row_norm_max(oi_ctx *ctx, const float *rows, uint64_t n, uint32_t dim, uint32_t *max_bits);
int oi_launch_screen_stage(oi_ctx *ctx, const float *d_queries, uint32_t n_queries, uint32_t dim,
                           const uint32_t *max_norm_bits, uint16_t *q_bf16, float *eps2, uint32_t *gate);
int oi_launch_cosine_screen_chunk(oi_ctx *ctx, const float *rows, uint64_t row_begin, uint64_t row_end, uint32_t dim,
                                  const uint16_t *q_bf16, uint32_t n_queries, uint32_t doc_id_base, PoolView &pool);
int oi_launch_make_screen_copy(oi_ctx *ctx, const float *rows, uint64_t n, uint32_t dim, uint16_t *out);
// cosine_screen_i8.hip: the int8 first tier in front of the bf16 screen
#define OI_I8_CARRY 16384u // keys per query the int8 tier carries between chunks (its margin selects' candidate room)
size_t oi_screen_i8_bytes(uint64_t n, uint32_t dim);
size_t oi_screen_i8_meta_offset(uint64_t n, uint32_t dim);
int oi_launch_make_screen_i8(oi_ctx *ctx, const float *rows, uint64_t n, uint32_t dim, const uint32_t *long_bitmap, uint8_t *out);
// per search: i8 hi / lo query blocks (qi8: [2][n_padded][dim]) and four floats per query in qf: qa, qn, cq, eps2 (the tier's margin)
int oi_launch_screen_stage_i8(oi_ctx *ctx, const float *d_queries, uint32_t n_queries, uint32_t dim, const uint32_t *max_norm_bits,
                              const uint8_t *i8_copy, uint64_t n_rows, int8_t *qi8, float *qf, uint32_t *gate,
                              uint16_t *q_bf16, float *eps2, const uint8_t *residual = nullptr, float *eps2_residual = nullptr);
// (q_bf16 / eps2: the same launch also writes what oi_launch_screen_stage writes -- the int8 route stages once;
// residual / eps2_residual set: eps2_residual[q] = 2 eps2'_q, the residual tier's select margin, written last -- it may be eps2)
int oi_launch_cosine_screen_i8_chunk(oi_ctx *ctx, const uint8_t *i8_copy, uint64_t n_rows_total, uint64_t row_begin, uint64_t row_end,
                                     uint32_t dim, const int8_t *qi8, const float *qf, uint32_t n_queries, uint32_t doc_id_base,
                                     PoolView &pool, uint32_t wgs = 0);
// (wgs: the launch's width in workgroups, 0 = the screens' 7/8 of the CUs)
// the sample pass (search.hip, Plan::sample_rows): the dense lower-bound score keys of rows [0, m_rows) against every query,
// keys[padded queries][oi_screen_i8_sample_stride(m_rows)], 0 where a row takes no part (long_bitmap: may be null); then
// (select.hip) the first speculative threshold from the r-th largest of a query's keys -- the words sel_spec_words writes
uint32_t oi_screen_i8_sample_stride(uint32_t m_rows);
int oi_launch_screen_i8_sample(oi_ctx *ctx, const uint8_t *i8_copy, uint64_t n_rows_total, uint32_t m_rows, uint32_t dim, const int8_t *qi8,
                               const float *qf, uint32_t n_queries, const uint32_t *long_bitmap, uint32_t *keys);
int oi_launch_sample_rank(oi_ctx *ctx, const uint32_t *keys, uint32_t stride, uint32_t m, uint32_t n_queries, uint32_t r, const float *eps2,
                          const uint32_t *tau_keys, uint32_t *spec_tau, uint32_t *spec_max);
// the bf16 rescreen: every key of pool's carry (an int8 survivor) becomes its bf16 screen key, in place
int oi_launch_rescreen_bf16(oi_ctx *ctx, const uint16_t *copy_rows, uint64_t n_rows, uint32_t dim, uint32_t doc_id_base,
                            const uint16_t *q_bf16, uint32_t n_queries, const PoolView &pool);
// screen_i8_residual.hip: the residual plane (out: oi_screen_i8_bytes(n, dim) bytes, i8_copy: the finished first plane) and its
// rescreen -- every key of pool's carry (an int8 survivor's lower bound) becomes its two-plane score key, in place
int oi_launch_make_screen_i8_residual(oi_ctx *ctx, const float *rows, uint64_t n, uint32_t dim, const uint32_t *long_bitmap,
                                      const uint8_t *i8_copy, uint8_t *out);
int oi_launch_rescreen_residual(oi_ctx *ctx, const uint8_t *residual, const uint8_t *i8_copy, uint64_t n_rows, uint32_t dim,
                                uint32_t doc_id_base, const int8_t *qi8, const float *qf, uint32_t n_queries, const PoolView &pool);
// cosine_screen_copy.hip
int oi_launch_cosine_screen_copy_chunk(oi_ctx *ctx, const uint16_t *copy_rows, uint64_t row_begin, uint64_t row_end, uint32_t dim,
                                       const uint16_t *q_bf16, uint32_t n_queries, uint32_t doc_id_base, PoolView &pool);
int oi_launch_screen_probe(oi_ctx *ctx, const float *rows, uint64_t row_begin, uint32_t n_rows, uint32_t dim,
                           const uint16_t *q_bf16, uint32_t n_queries, float *d_out);
// speculative thresholds of the screen: the r-th best screen score so far - 2 eps, if above the proven threshold, for the NEXT
// chunk (spec_tau), the largest one used per query (spec_max) -- made inside the margin select that precedes the next chunk
// (SelectExtra::spec_rank, select.hip) or by the sample pass's rank launch; the check against the final one rides in
// oi_launch_rescore (spec_max, tau_final, gate, fail_host)
int oi_launch_rescore(oi_ctx *ctx, const float *rows, uint64_t n_rows, uint32_t dim, uint32_t doc_id_base,
                      const float *d_queries, uint32_t n_queries, const PoolView &in, const PoolView &out,
                      const uint32_t *extra_docs = nullptr, uint32_t n_extra = 0, const uint32_t *spec_max = nullptr,
                      const uint32_t *tau_final = nullptr, uint32_t *gate = nullptr, uint32_t *fail_host = nullptr,
                      uint32_t wgs_per_query = 0);
// (wgs_per_query: the launch's workgroups per query, 16 survivors a trip each; 0 = 64, sized for about 2 200 survivors)
#define OI_LONG_ROWS_MAX 1024u // rows the two-class margin may set aside (more: one class, the corpus maxima, as before)
int oi_launch_row_norm_classes(oi_ctx *ctx, const float *rows, uint64_t n, uint32_t dim, float X0, float E0, uint32_t *cls,
                               uint32_t *bitmap, uint32_t *list, uint32_t cap);
int oi_launch_cosine_ksplit(oi_ctx *ctx, const float *rows, uint64_t row_begin, uint64_t row_end, uint32_t dim,
                            const float *q, uint32_t nq, bool two_tiles, uint32_t doc_id_base, const PoolView &p, const uint32_t *run_gate);
// bm25.hip
int oi_bm25_stage_forward(oi_index *idx, const uint32_t *d_terms, const uint64_t *d_offsets);
int oi_bm25_finalize(oi_index *idx, uint64_t global_n, uint64_t global_tokens, const uint32_t *global_df_host);
// bm25_scan.hip
void oi_bm25_scan_geometry(const oi_ctx *ctx, uint64_t n_docs, uint32_t *n_segs, uint32_t *seg_cap);
uint32_t oi_bm25_scan_pass_queries(uint32_t max_terms_per_query);
int oi_launch_bm25_scan(oi_index *idx, const uint32_t *d_q_terms, const uint32_t *d_q_offsets, uint32_t q_begin,
                        uint32_t nq, uint64_t doc_begin, uint64_t doc_end, float avgdl, bool run_setup,
                        const PoolView &pool);
// bm25_wave.hip: one wave per (block, query) task; `pool` = the view of queries [q_begin, q_begin + nq)
uint32_t oi_bm25_wave_pass_queries(void);
int oi_launch_bm25_wave(oi_index *idx, const uint32_t *d_q_terms, const uint32_t *d_q_offsets, uint32_t q_begin,
                        uint32_t nq, const PoolView &pool, uint32_t block_begin, uint32_t block_end);
// bm25_stream.hip: every wave streams a weight-balanced range of (query, block) tasks through an LDS ring; `pool` = the view
// of queries [q_begin, q_begin + nq) with segments of oi_bm25_stream_seg_cap() keys.  oi_launch_bm25_plan runs once per
// pass, before the first phase: it zeroes the pass's pool state (`state_words` words at `state`) and weighs the queries.
uint32_t oi_bm25_stream_pass_queries(void);
uint32_t oi_bm25_stream_seg_cap(uint32_t depth, bool first_phase);
int oi_launch_bm25_plan(oi_index *idx, const uint32_t *d_q_terms, const uint32_t *d_q_offsets, uint32_t q_begin, uint32_t nq,
                        uint32_t *state, uint64_t state_words, uint32_t depth, uint32_t tau_off, uint32_t tau_words, bool with_floors);
int oi_launch_bm25_stream(oi_index *idx, const uint32_t *d_q_terms, const uint32_t *d_q_offsets, uint32_t q_begin,
                          uint32_t nq, uint32_t depth, const PoolView &pool, uint32_t block_begin, uint32_t block_end);
// Doc blocks [block_begin, block_end); candidates below pool.tau_keys (if set) are dropped.
int oi_launch_bm25(oi_index *idx, const uint32_t *d_q_terms, const uint32_t *d_q_offsets,
                   uint32_t n_queries, uint32_t depth, const PoolView &pool, uint32_t block_begin,
                   uint32_t block_end);

// comm.hip: RCCL through dlopen (no link-time dependency)
struct oi_comm {
    oi_ctx *ctx = nullptr; // holds a reference
    void *nccl = nullptr;  // ncclComm_t
    uint32_t rank = 0, world = 1;
};
int oi_rccl_unique_id(uint8_t *id_out);
int oi_rccl_init(void **comm_out, uint32_t world, const uint8_t *id_bytes, uint32_t rank);
void oi_rccl_destroy(void *comm);
int oi_rccl_all_gather_u32(void *comm, const uint32_t *send, uint32_t *recv, size_t words, hipStream_t st);
int oi_rccl_all_reduce_sum(void *comm, void *buf, size_t count, bool u64, hipStream_t st);
