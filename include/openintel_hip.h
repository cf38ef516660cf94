/*
 * openintel_hip.h -- C ABI of libopenintel_hip.so (MI355X / gfx950, hand-written HIP).
 *
 * This is the drop-in boundary: plain pointers and sizes, int status codes, no
 * exceptions across the ABI, no framework types.  A Rust `extern "C"` block (or
 * ctypes) binds these symbols directly; see INTEGRATION.md for the Rust shim that
 * implements the reference's port trait on top of them.
 *
 * Reference interfaces replaced (paths relative to the openintel repo):
 *
 *   oi_lexicon_analyze*      <- trait PostAnalyzer::analyze
 *                               src/domain/ports/post_analyzer.rs:7-11, implemented by
 *                               LexiconAnalyzer   src/adapters/analyzer/lexicon.rs:53-87
 *                               (called at src/application/analyze.rs:62-63)
 *   oi_social_summary*       <- SpeculationEngine::social_summary
 *                               src/domain/engine/speculation_engine.rs:70-125
 *   oi_social_summary_segmented / oi_lexicon_scan_segments_device
 *                            <- the per-ticker loop of the batch callers run_scan / run_compare
 *                               src/mcp/tools.rs:193-225, :303-352 (each iteration = analyze.rs:61-63 +
 *                               speculation_engine.rs:70-125), as ONE pooled scan + one reduction per ticker
 *   oi_headline_scan*        <- catalyst_hits + headline_mentions_company over the dip
 *                               gate's titles   src/domain/dip.rs:247-272 (loop at :617-626)
 *   oi_index_* / oi_search*  <- NO reference interface exists: the
 *   oi_rrf_fuse / oi_merge_lists  reference has no retrieval port.  New, builder-defined
 *                               API styled after the reference's ports (borrowed inputs,
 *                               caller-owned outputs, DomainError-style failures).
 *
 * Conventions
 *   - Every function returns OI_OK (0) or a negative oi_status.  oi_last_error()
 *     returns a thread-local message for the last failure on the calling thread.
 *     A Rust shim maps nonzero -> DomainError::SourceFailure{name:"hip-analyzer",..}
 *     (src/domain/error.rs:16-17).
 *   - `location` arguments say where the caller's buffers live: OI_HOST or OI_DEVICE
 *     (HBM of the ctx's device).  With OI_DEVICE the call is asynchronous on the ctx
 *     stream (oi_set_stream / oi_synchronize); with OI_HOST it returns after the
 *     results are in the caller's buffers.
 *   - The library never keeps a caller pointer past return, except
 *     oi_index_set_embeddings(OI_DEVICE), which borrows the corpus matrix (30 GB at
 *     10M x 768 is not copied) until oi_index_destroy.
 *   - An oi_ctx serialises calls internally (one mutex): safe to share between host
 *     threads, as the reference's `Send + Sync` port requires.
 */
#ifndef OPENINTEL_HIP_H
#define OPENINTEL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OI_ABI_VERSION 1

typedef enum {
    OI_OK = 0,
    OI_ERR_INVALID_ARG = -1,
    OI_ERR_HIP = -2,           /* a HIP runtime call failed; message has the hipError */
    OI_ERR_ANALYZER_MISMATCH = -3, /* mirrors DomainError::AnalyzerMismatch, error.rs:13-14 */
    OI_ERR_STATE = -5,         /* call order violated (e.g. search before finalize) */
    OI_ERR_NO_DEVICE = -6,     /* no gfx950 device / HIP runtime unusable */
    OI_ERR_UNSUPPORTED = -7,   /* shape outside what the kernels are built for */
    OI_ERR_OVERFLOW = -8,      /* an internal candidate pool overflowed (bug guard) */
    OI_ERR_COMM = -9           /* an RCCL call failed; message has the ncclResult string */
} oi_status;

enum { OI_HOST = 0, OI_DEVICE = 1 };

/* Limits of the kernels in this build. */
#define OI_MAX_DEPTH 1024u      /* per-list depth k' and final k */
#define OI_MAX_DIM 1024u        /* embedding dimension (multiple of 4) */
#define OI_BM25_BLOCK_DOCS 32768u /* docs per BM25 doc block (one pool segment, one seen/multi map) */
#define OI_BM25_FINE_DOCS 16384u  /* docs per (term, window) cell of the inverted index: two windows per block */

typedef struct oi_ctx oi_ctx;
typedef struct oi_index oi_index;
typedef struct oi_comm oi_comm;

int oi_abi_version(void);
const char *oi_last_error(void);

int oi_create(int device_ordinal, oi_ctx **out);
/* A NEW context on `like`'s device with `like`'s settings (cosine mode, overlap of the legs, graph replay) and nothing
 * else of it: its own default stream, its own (still empty) workspaces.  For a host that scores several batches at once
 * through views of one index (oi_index_view): every lane gets a context of its own and the caller's is never rebound. */
int oi_create_like(oi_ctx *like, oi_ctx **out);
/* Lifetime: handles are reference-counted inside the library, so destruction is safe in ANY order.  oi_destroy gives up
 * the caller's handle (which must not be used again); if indexes created on -- or viewed through -- the ctx are still
 * alive, its stream, workspaces and mutex stay until the last of them is destroyed (those indexes remain fully usable
 * and from then on run on the device's default stream: oi_destroy forgets the stream given to oi_set_stream, which may
 * not outlive the caller).  Likewise oi_index_destroy of an index that still has views keeps its buffers until the
 * last view is destroyed.  (The reference shares its long-lived adapters the same way -- `Arc<...>` fields of the MCP
 * server, src/mcp/server.rs:17-20: the last owner frees.) */
void oi_destroy(oi_ctx *ctx);
/* `hip_stream` is a hipStream_t (NULL = the default stream). */
int oi_set_stream(oi_ctx *ctx, void *hip_stream);
int oi_synchronize(oi_ctx *ctx);

/* How the batch cosine scorer works over an f32 corpus (dim 384 / 768; more than 8 queries, or -- since round 5 -- any
 * number of queries when the index holds a screening copy; other shapes always use the exact kernels).  The corpus handed to the library stays f32 in HBM in every mode, and every score the
 * library returns is computed in f32 from those f32 rows.
 *   OI_COSINE_SCREEN (default) a bf16 screen with a proven error bound picks the rows that can reach the list
 *                              (one bf16 MFMA per product: HBM-bound; the bound is built from the MEASURED rounding
 *                              errors of the corpus and of each query), exact f32 scores are then computed for those
 *                              rows only; a query whose survivors do not fit falls back, inside the same call, to the
 *                              exact kernel.  The screen reads the index's bf16 SCREENING COPY of the rows when the
 *                              index holds one (oi_index_set_screen_copy: made at finalize when it fits the budget --
 *                              2 d bytes per row and batch) and converts the f32 rows on the fly otherwise (4 d bytes).
 *                              Same products, same bound, same survivors, same rescoring either way.
 *                              What comes out: the SET of rows of the exact scorer's list up to ties -- two rows whose
 *                              exact f32 scores differ by less than the f32 rounding of two summation orders (measured
 *                              <= 5e-7 at d = 768) may swap neighbouring ranks or, at the list's last rank, places;
 *                              every score within the 1e-5 bar (csrc/cosine_prefilter.hip has the argument).  RRF
 *                              output is bit-exact GIVEN the two lists.
 *   OI_COSINE_EXACT            v_mfma_f32_* on the f32 values for every row: matrix-pipe-bound.
 *   OI_COSINE_SPLIT            every f32 operand is split exactly into three bf16 values and the dot product
 *                              taken as six bf16 MFMAs with f32 accumulation (the three smallest of the nine
 *                              cross terms, <= 2^-23 relative, are dropped): f32-grade scores (measured error
 *                              vs f64 ~4e-8 on unit vectors; the exact kernel's f32 accumulation ~1e-7).
 *   OI_COSINE_SCREEN_COPY      OI_COSINE_SCREEN, and an index without a screening copy gets one on the first search
 *                              whatever its policy (rounds 2-4's opt-in mode; kept for callers that used it).
 *   OI_COSINE_SCREEN_STREAM    OI_COSINE_SCREEN with the screen ALWAYS converting the f32 rows on the fly, copy or not
 *                              (rounds 1-4's default; A/B runs and bench.py's `f32_stream_scorer`).
 * Also selectable with OI_COSINE_MODE=screen|exact|split|screen-copy|screen-stream at oi_create. */
#define OI_COSINE_EXACT 0
#define OI_COSINE_SPLIT 1
#define OI_COSINE_SCREEN 2
#define OI_COSINE_SCREEN_COPY 3
#define OI_COSINE_SCREEN_STREAM 4
int oi_set_cosine_mode(oi_ctx *ctx, int mode);

/* A hybrid query has two independent legs until fusion.  By default the BM25 leg is issued on an
 * internal side stream (forked from and joined back into the ctx stream inside the call) so that it
 * runs beside the MFMA-bound cosine leg; enable = 0 runs them one after the other. */
int oi_set_overlap(oi_ctx *ctx, int enable);

/* Speculative thresholds of the screen (round 5; default on).  Between the corpus chunks of a screened search the threshold is the
 * proven one -- the k'-th best screen score of the rows seen so far, minus the margin -- which is weak while few rows have been seen.
 * With speculation the next chunk is screened against the larger of it and a PREDICTION of the final threshold (the r-th best score
 * so far, r = 3 k' m / n + 12 after m of n rows), and the prediction is checked at the end against the proven final threshold: if it
 * holds, the survivors are a superset of the proven screen's and the lists are the same; if not (a corpus whose first rows are not a
 * fair sample of it), the exact pipeline rescores the batch inside the same call -- the same lists, later -- and the ctx stops
 * speculating for 16, 32, ... 1024 searches.  enable = 0: proven thresholds only (rounds 2-4).  Never used with graph replay. */
int oi_set_screen_speculation(oi_ctx *ctx, int enable);

/* One device-buffer query call is ~30 kernel launches, memsets and event operations: ~0.3 ms of host time, which at a
 * 1.25M-row shard (one of 8 GPUs) is what limits the rate, not the GPU (0.7 ms of work that two batches in flight overlap).
 * enable != 0: oi_search_lists_packed / oi_fuse_packed / oi_search calls with OI_DEVICE buffers are CAPTURED into a
 * hipGraph the second time they are made with the same arguments (index, pointers, sizes, modes) on this ctx and
 * replayed with one launch call from then on.  The launch sequence does not depend on the data (chunk schedules and
 * pool capacities are functions of the sizes alone), so a replay does exactly what the call would have done: same
 * kernels, same buffers, same results.  The caller's part: keep using the SAME buffers (a serving loop copies each batch
 * into per-slot staging buffers -- openintel_amd/sharded.py does).  A call with new arguments runs eagerly once more;
 * profiling (oi_profile_reset) and the default stream disable replay; at most 32 captured calls per ctx are kept.
 * Default off.  (No reference counterpart: the reference makes no device calls, src/adapters/analyzer/lexicon.rs:82-87.) */
int oi_set_graph_replay(oi_ctx *ctx, int enable);

/* ------------------------------------------------------------------------- */
/* PostAnalyzer path (reference-pinned)                                        */
/* ------------------------------------------------------------------------- */

/*
 * One (polarity, speculative) per post, index-aligned with the input
 * (post_analyzer.rs:9).  Post i is text_blob[offsets[i] .. offsets[i+1]), valid
 * UTF-8 (the shim gathers SocialPost.text into one blob: posts are not contiguous
 * in the reference, social_post.rs:25-27).  Infallible in the reference; here it
 * fails only on device errors.
 */
int oi_lexicon_analyze(oi_ctx *ctx, const uint8_t *text_blob, const uint64_t *offsets,
                       uint64_t n_posts, double *polarity_out, uint8_t *speculative_out);

/* Same, buffers already in HBM; asynchronous on the ctx stream. */
int oi_lexicon_analyze_device(oi_ctx *ctx, const uint8_t *d_text_blob, const uint64_t *d_offsets,
                              uint64_t n_posts, uint64_t blob_bytes, double *d_polarity_out,
                              uint8_t *d_speculative_out);

/* Raw sums of SpeculationEngine::social_summary (speculation_engine.rs:76-97).
 * Integer fields are exact.  polarity_sum is a fixed-shape tree sum (bitwise
 * reproducible run to run) and differs from the reference's input-order sum by
 * at most n * 2^-52 * max|partial sum| (the bound tests/ assert). */
typedef struct {
    uint64_t total;
    uint64_t by_source[2]; /* [reddit, bluesky]  source_kind.rs:5-8 */
    uint64_t bullish, bearish, neutral, spec_count;
    double polarity_sum;
} oi_social_counters;

/* sources[i]: 0 = reddit, 1 = bluesky.  n_posts != n_signals ->
 * OI_ERR_ANALYZER_MISMATCH (speculation_engine.rs:29-34). */
int oi_social_summary(oi_ctx *ctx, const uint8_t *sources, uint64_t n_posts,
                      const double *polarity, const uint8_t *speculative, uint64_t n_signals,
                      double bull_bear_threshold, int location, oi_social_counters *out_host);

/* LexiconAnalyzer::analyze and the two loops of social_summary in ONE pass over the text (lexicon.rs:53-87 +
 * speculation_engine.rs:76-97): the per-post signals are reduced where they are computed, so with
 * d_polarity_out == d_speculative_out == NULL nothing per post is written at all ("0 out if fused
 * with the A4 reduction").  Buffers in HBM; d_sources (0 = reddit, 1 = bluesky) may be NULL; the outputs, when
 * given, are exactly oi_lexicon_analyze_device's.  Integer fields exact; polarity_sum a fixed-shape tree sum
 * (bitwise reproducible; same bound as oi_social_summary's).  Synchronises the ctx stream (the sums come back). */
int oi_lexicon_summary_device(oi_ctx *ctx, const uint8_t *d_text_blob, const uint64_t *d_offsets, uint64_t n_posts,
                              uint64_t blob_bytes, const uint8_t *d_sources, double bull_bear_threshold,
                              double *d_polarity_out, uint8_t *d_speculative_out, oi_social_counters *out_host);

/* The batch callers: run_scan (src/mcp/tools.rs:193-225) and run_compare (:303-352) run application::analyze once per
 * ticker.  Here the posts of ALL tickers are pooled into one batch -- one scan -- and every ticker gets its
 * social_summary sums from one reduction: segment s = posts [seg_offsets[s], seg_offsets[s+1]) (non-decreasing,
 * seg_offsets[n_segments] <= n_posts; an empty segment gives zeros), out[s] = that ticker's counters.
 * polarity_sum is the reference's own loop (speculation_engine.rs:82-86): added one signal at a time, in input order, from
 * +0.0 -- BIT-IDENTICAL to the reference's f64 (and so is net_sentiment = polarity_sum / total), unlike the tree of
 * oi_social_summary.  One wave per segment: meant for many segments of a ticker's size (50 posts per source,
 * tools.rs:101); a single segment of 10M posts takes ~50 ms.
 * location OI_HOST: every pointer is host memory, the call returns with `out` filled; seg_offsets[n_segments] > n_posts
 * -> OI_ERR_ANALYZER_MISMATCH (speculation_engine.rs:29-34), decreasing offsets -> OI_ERR_INVALID_ARG.
 * location OI_DEVICE: every pointer (out too: n_segments records) is HBM, asynchronous on the ctx stream; offsets past
 * n_posts are clamped by the kernel.  sources may be NULL (by_source stays 0). */
int oi_social_summary_segmented(oi_ctx *ctx, const uint8_t *sources, const double *polarity, const uint8_t *speculative,
                                uint64_t n_posts, const uint64_t *seg_offsets, uint64_t n_segments,
                                double bull_bear_threshold, int location, oi_social_counters *out);

/* oi_lexicon_analyze_device + oi_social_summary_segmented(OI_DEVICE) as one call on the ctx stream: the pooled posts of
 * n_segments tickers in, one record per ticker out (d_out, HBM).  d_polarity_out / d_speculative_out may be NULL (the
 * signals then live in the ctx's workspace only).  Asynchronous. */
int oi_lexicon_scan_segments_device(oi_ctx *ctx, const uint8_t *d_text_blob, const uint64_t *d_offsets, uint64_t n_posts,
                                    uint64_t blob_bytes, const uint8_t *d_sources, const uint64_t *d_seg_offsets,
                                    uint64_t n_segments, double bull_bear_threshold, double *d_polarity_out,
                                    uint8_t *d_speculative_out, oi_social_counters *d_out);

/* ------------------------------------------------------------------------- */
/* Headline gate (src/domain/dip.rs:204-272)                                   */
/* ------------------------------------------------------------------------- */

/* CATALYST_KEYWORDS (dip.rs:38-55) in declaration order; NULL past the end. */
#define OI_N_CATALYST_KEYWORDS 16
const char *oi_catalyst_keyword(uint32_t index);

/*
 * For each title i = blob[offsets[i] .. offsets[i+1]) (UTF-8, offsets[0] == 0):
 *   mask_out[i]   bit k set iff keyword k occurs as a whole word        catalyst_hits(&[title])
 *   order_out[i]  nibble j = keyword index of the j-th distinct hit,    (dip.rs:261-272; the
 *                 first-occurrence order of the reference's Vec          multi-text call is the
 *                                                                        deduped concatenation)
 *   about_out[i]  headline_mentions_company(title, ticker, name_forms)  dip.rs:247-258
 * ticker is the raw symbol (ticker_len bytes, compared ASCII-lowercased, ignored when
 * shorter than 2 bytes -- dip.rs:250); form i is forms_blob[form_offsets[i] ..
 * form_offsets[i+1]) exactly as company_name_forms returned it (n_forms may be 0; the
 * caller keeps the reference's `name_forms.is_empty() ||` short-circuit, dip.rs:624).
 * At most 32 usable patterns / 1024 pattern bytes per call -> OI_ERR_INVALID_ARG beyond.
 */
int oi_headline_scan(oi_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, uint64_t n_titles,
                     const uint8_t *ticker, uint64_t ticker_len, const uint8_t *forms_blob,
                     const uint32_t *form_offsets, uint32_t n_forms, uint16_t *mask_out,
                     uint64_t *order_out, uint8_t *about_out);

/* Same, titles and outputs already in HBM (blob 16-byte aligned, each title < 4 GiB);
 * ticker/forms stay host pointers.  Asynchronous on the ctx stream. */
int oi_headline_scan_device(oi_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets,
                            uint64_t n_titles, uint64_t blob_bytes, const uint8_t *ticker,
                            uint64_t ticker_len, const uint8_t *forms_blob,
                            const uint32_t *form_offsets, uint32_t n_forms, uint16_t *d_mask_out,
                            uint64_t *d_order_out, uint8_t *d_about_out);

/* The gate over the ROWS of a dip scan (src/application/dip.rs: one `check` per loser -> domain/dip.rs:612-659 on that
 * row's headlines, ticker and name forms).  Row r owns titles [row_offsets[r], row_offsets[r+1]) (row_offsets[0] = 0,
 * row_offsets[n_rows] = n_titles), ticker tickers_blob[ticker_offsets[r] .. ticker_offsets[r+1]) and name forms
 * row_form_offsets[r] .. row_form_offsets[r+1] (indices into form_offsets, which holds total_forms + 1 byte offsets into
 * forms_blob).  Outputs as oi_headline_scan, index-aligned with the titles.  Host buffers; one staging copy, one launch
 * per row back to back, one copy back -- a 25-row scan costs about what four single-row calls do.  At most 4096 rows. */
int oi_headline_scan_rows(oi_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, uint64_t n_titles,
                          const uint64_t *row_offsets, uint32_t n_rows, const uint8_t *tickers_blob,
                          const uint32_t *ticker_offsets, const uint8_t *forms_blob, const uint32_t *form_offsets,
                          const uint32_t *row_form_offsets, uint16_t *mask_out, uint64_t *order_out, uint8_t *about_out);

/* ------------------------------------------------------------------------- */
/* Hybrid retrieval (builder-defined; parity unpinned vs the reference)        */
/* ------------------------------------------------------------------------- */

/* A shard of the corpus: rows [doc_id_base, doc_id_base + n_docs) of the global
 * collection.  Result doc ids are global (doc_id_base + local row). */
int oi_index_create(oi_ctx *ctx, uint64_t n_docs, uint32_t dim, uint32_t vocab,
                    uint32_t doc_id_base, oi_index **out);
void oi_index_destroy(oi_index *idx);

/* A second handle on a FINALIZED index, bound to another context of the same device (its own stream and workspaces), so
 * that two searches over the same shard can be in flight at once -- e.g. batch i+1 scored while the selects and the
 * rescoring of batch i drain.  The view borrows every buffer of `src`: it is read-only (the set_* /
 * finalize calls return OI_ERR_STATE), costs no HBM for the index (its ctx allocates its own search workspaces on
 * first use, see oi_search_lists), may be destroyed before or after `src` (the buffers live until the last handle on them
 * is gone), and is searched with the ordinary
 * oi_search* calls.  Thread-safety is per context as everywhere else: the two handles may be driven from two host threads.
 * (No reference counterpart: the reference's port is synchronous, src/domain/ports/post_analyzer.rs:7-11 is its model.) */
int oi_index_view(oi_index *src, oi_ctx *ctx, oi_index **out);

/* rows: n_docs x dim f32, row-major.  normalize != 0: L2-normalise each row (in
 * place when OI_DEVICE).  OI_DEVICE borrows the pointer; OI_HOST copies to HBM. */
int oi_index_set_embeddings(oi_index *idx, float *rows, int location, int normalize);

/* A bf16 corpus instead (BASELINE configs[4]): rows n_docs x dim of bfloat16 bit patterns, row-major,
 * unit-norm as stored (no normalisation is applied), dim in {384, 768, 1024}.  OI_DEVICE borrows the
 * pointer (16-byte aligned); OI_HOST copies to HBM.  Queries stay f32 at the API and are rounded to
 * bf16 (nearest even) inside: a score is sum_k bf16(q_k) * x_k accumulated in f32.  Replaces any f32
 * matrix set before, and vice versa. */
int oi_index_set_embeddings_bf16(oi_index *idx, const uint16_t *rows, int location);

/* Forward index: doc d owns term_ids[doc_offsets[d] .. doc_offsets[d+1]),
 * every id < vocab.  Stages the postings and computes local statistics. */
int oi_index_set_forward(oi_index *idx, const uint32_t *term_ids, const uint64_t *doc_offsets,
                         int location);
/* Local document frequencies (vocab entries, host) and token count: what a
 * multi-shard caller all-reduces before oi_index_finalize. */
int oi_index_local_stats(oi_index *idx, uint64_t *total_tokens_out, uint32_t *df_out_host);
/* Fix the collection statistics (global N, token count, df; df NULL = local) and
 * build the blocked inverted index with precomputed BM25 impacts. */
int oi_index_finalize(oi_index *idx, uint64_t global_n_docs, uint64_t global_total_tokens,
                      const uint32_t *global_df_host);

/* How many rows the screened cosine scorer sets aside (diagnostics, tests).  When the largest row norms of an f32 corpus
 * stand out from the rest (> 1.5 x the RMS norm, or the same for the norm of bf16(x) - x) and the rows responsible are few
 * (<= 1024), they are left out of the screen's thresholds and rescored exactly for every query; the screen's margin is then
 * built from the other rows' maxima.  0: one class (a normalised corpus, or too many such rows).  Builder-defined like the
 * whole retrieval path (the reference has no embeddings: SURVEY.md section 0). */
int oi_index_long_rows(oi_index *idx, uint32_t *n_out);

/* The bf16 SCREENING COPY of an f32 corpus: a derived index structure like the BM25 impact postings -- bf16(x) of every
 * row, made by the library with the screen's own conversion (so the measured error bound of OI_COSINE_SCREEN is the copy's),
 * n_docs x dim x 2 bytes of HBM on top of the f32 rows.  The screen streams it instead of the f32 rows (half the bytes of
 * an HBM-bound kernel); survivors are still rescored in f32 from the f32 rows, so the lists do not change.
 *   OI_SCREEN_COPY_AUTO (default)  made by oi_index_finalize / oi_index_finalize_sharded (and again by
 *                                  oi_index_set_embeddings on a finalized index) when the corpus can be screened (dim 384 /
 *                                  768, finite norms) and the copy is at most a quarter of the device memory that is FREE at
 *                                  that moment (OI_SCREEN_COPY_MAX_FRAC=0.25 overrides the fraction); otherwise no copy:
 *                                  the screen converts the f32 rows on the fly.
 *   OI_SCREEN_COPY_NEVER           no copy (an existing one is freed).
 *   OI_SCREEN_COPY_ALWAYS          made whatever the budget (OI_ERR_HIP if the allocation fails).
 * Call before finalize (or any time: a finalized index applies the policy at once).  OI_SCREEN_COPY=auto|never|always sets
 * the process-wide default.  Views (oi_index_view) borrow the source's copy.  No reference counterpart (the reference has no
 * embeddings: SURVEY.md section 0). */
#define OI_SCREEN_COPY_AUTO 0
#define OI_SCREEN_COPY_NEVER 1
#define OI_SCREEN_COPY_ALWAYS 2
int oi_index_set_screen_copy(oi_index *idx, int policy);
/* HBM the index itself holds right now (oi_workspace_bytes reports the searching contexts' workspaces): the embedding
 * rows as handed over (0 when the caller's device pointer is borrowed), the screening copy, and the BM25 structures
 * (postings, cell table, idf / floors, doc lengths, the kept forward index).  Any output may be NULL. */
int oi_index_bytes(oi_index *idx, uint64_t *rows_owned_bytes_out, uint64_t *screen_copy_bytes_out, uint64_t *bm25_bytes_out);

/* BM25 kernel choice: 0 = default (= 4), 1 = term-at-a-time with one workgroup per doc block (bm25.hip, the
 * first-generation kernel), 2 = batch scan of the forward index (bm25_scan.hip), 3 = term-at-a-time with one wave
 * per (doc block, query) task (bm25_wave.hip), 4 = term-at-a-time as a stream: every wave walks a weight-balanced
 * range of (query, block) tasks with the postings ahead of it in flight through an LDS ring (bm25_stream.hip).
 * All produce bit-identical lists.  OI_BM25_MODE=stream|wave|taat|scan selects the default process-wide. */
int oi_index_set_bm25_mode(oi_index *idx, int mode);

/* Contract for the batch BM25 scan (mode 2): no query of a batch has more
 * than `max_terms` terms (default 16).  The scan handles 1024 / max_terms queries per pass over the
 * forward index; a longer query sets the ctx's error flag (OI_ERR_OVERFLOW at the next host-visible
 * point).  The term-at-a-time path (smaller batches, or OI_BM25_MODE=taat) has no such limit. */
int oi_index_set_max_query_terms(oi_index *idx, uint32_t max_terms);

/*
 * Per-shard ranked lists for a batch of queries.
 *   query_vecs      n_queries x dim f32 (normalised by the caller if cosine is wanted)
 *   query_terms     concatenated term ids; query q owns [q_term_offsets[q], q_term_offsets[q+1])
 * Outputs, each n_queries x depth, row q sorted by (score desc, doc id asc),
 * first counts[q] entries valid:
 *   cosine list: dot(query, row);  BM25 list: only docs with score > 0.
 * Non-finite rows (OI_COSINE_EXACT): a row whose dot product is NaN under IEEE arithmetic (0 x inf and inf - inf included) is
 * never listed and a +inf or -inf score ranks where IEEE orders it, whatever the batch size.
 */
int oi_search_lists(oi_index *idx, const float *query_vecs, const uint32_t *query_terms,
                    const uint32_t *q_term_offsets, uint32_t n_queries, uint32_t depth,
                    int location, float *cos_scores, uint32_t *cos_docs, uint32_t *cos_counts,
                    float *bm25_scores, uint32_t *bm25_docs, uint32_t *bm25_counts);

/* Merge per-shard lists ([n_shards][n_queries][depth], counts [n_shards][n_queries])
 * into the global top-`depth` per query (the step after the RCCL all-gather). */
int oi_merge_lists(oi_ctx *ctx, const float *scores, const uint32_t *docs, const uint32_t *counts,
                   uint32_t n_shards, uint32_t n_queries, uint32_t depth, int location,
                   float *scores_out, uint32_t *docs_out, uint32_t *counts_out);

/*
 * The multi-GPU exchange format.  A shard's two lists for a batch, packed in ONE buffer of
 * OI_PACKED_WORDS(n_queries, depth) 32-bit words:
 *     float    scores[2][n_queries][depth]     list 0 = cosine, list 1 = BM25
 *     uint32_t docs  [2][n_queries][depth]
 *     uint32_t counts[2][n_queries]
 * oi_search_lists_packed fills it (same contents as oi_search_lists); every rank all-gathers the
 * buffers (RCCL) into [n_shards][OI_PACKED_WORDS] and calls oi_fuse_packed, which merges each list to
 * its global top-`depth` and THEN fuses (global ranks are needed: fusing per shard is not equivalent).
 */
#define OI_PACKED_WORDS(n_queries, depth) (4ull * (n_queries) * (depth) + 2ull * (n_queries))
int oi_search_lists_packed(oi_index *idx, const float *query_vecs, const uint32_t *query_terms,
                           const uint32_t *q_term_offsets, uint32_t n_queries, uint32_t depth,
                           int location, uint32_t *packed_out);
int oi_fuse_packed(oi_ctx *ctx, const uint32_t *packed_all, uint32_t n_shards, uint32_t n_queries,
                   uint32_t depth, uint32_t k, int location, float *scores_out, uint32_t *docs_out,
                   uint32_t *counts_out);

/* Reciprocal-rank fusion of two ranked lists per query (row stride `depth`):
 * rrf(d) = sum over lists containing d of 1/(60 + rank), rank from 1; output top-k
 * by (rrf desc, doc id asc), row stride k. */
int oi_rrf_fuse(oi_ctx *ctx, const uint32_t *docs_a, const uint32_t *counts_a,
                const uint32_t *docs_b, const uint32_t *counts_b, uint32_t n_queries,
                uint32_t depth, uint32_t k, int location, float *scores_out, uint32_t *docs_out,
                uint32_t *counts_out);

/* oi_search_lists + oi_rrf_fuse on one shard: the whole hybrid query. */
int oi_search(oi_index *idx, const float *query_vecs, const uint32_t *query_terms,
              const uint32_t *q_term_offsets, uint32_t n_queries, uint32_t depth, uint32_t k,
              int location, float *scores_out, uint32_t *docs_out, uint32_t *counts_out);

/* ------------------------------------------------------------------------- */
/* The row-sharded query behind the C ABI: one process per GPU, RCCL inside    */
/* ------------------------------------------------------------------------- */
/*
 * A host with no collective library of its own (the Rust composition root, src/main.rs:17-39, has none -- the reference
 * is single-process, src/domain/ports/mod.rs:1-8) gets the whole multi-GPU path from three calls.  RCCL is loaded on
 * first use (dlopen "librccl.so.1", or the library OI_RCCL_LIB names; OI_ERR_UNSUPPORTED with the loader's message if
 * it cannot be loaded -- tests/test_abi.py takes that path).  A Python host that already runs torch.distributed
 * can keep using oi_search_lists_packed + its own all-gather + oi_fuse_packed (openintel_amd/sharded.py): same results.
 *
 *   rank 0:  oi_comm_unique_id(id)  -> ship the OI_COMM_ID_BYTES to every rank over the host's own channel (file, socket, env)
 *   all:     oi_comm_create(ctx, id, rank, world, &comm)          collective: returns when every rank has called it
 *            ... oi_index_create / set_embeddings / set_forward on the rank's row shard (doc_id_base = first global row) ...
 *            oi_index_finalize_sharded(idx, comm)                  collective: all-reduce of (n_docs, tokens) and of the
 *                                                                  df vector, then the impacts from the GLOBAL statistics
 *            oi_search_sharded(idx, comm, queries..., out...)      collective, once per batch, same queries on every rank:
 *                                                                  the shard's two lists -> ONE ncclAllGather of
 *                                                                  OI_PACKED_WORDS words per rank -> merge to the global
 *                                                                  top-depth per list -> RRF.  Identical output on every rank.
 * Collectives run on the ctx stream in call order: every rank must issue them in the same order (one host thread per
 * comm, or external ordering).  With OI_DEVICE buffers oi_search_sharded is asynchronous like oi_search.
 * Executed so far with a communicator of ONE rank only (tests/test_gpu_native_comm.py): the build's GPU lease has one
 * device and RCCL refuses two ranks on one device.  The same choreography over torch.distributed (sharded.py) has run
 * with 2 and 8 gloo ranks; N > 1 through THESE entry points is unexecuted code.
 */
#define OI_COMM_ID_BYTES 128
int oi_comm_unique_id(uint8_t id_out[OI_COMM_ID_BYTES]);
int oi_comm_create(oi_ctx *ctx, const uint8_t id[OI_COMM_ID_BYTES], uint32_t rank, uint32_t world, oi_comm **out);
void oi_comm_destroy(oi_comm *comm);
int oi_index_finalize_sharded(oi_index *idx, oi_comm *comm);
int oi_search_sharded(oi_index *idx, oi_comm *comm, const float *query_vecs, const uint32_t *query_terms,
                      const uint32_t *q_term_offsets, uint32_t n_queries, uint32_t depth, uint32_t k, int location,
                      float *scores_out, uint32_t *docs_out, uint32_t *counts_out);

/* ------------------------------------------------------------------------- */
/* Filtered search: the best rows among the documents that match a predicate    */
/* ------------------------------------------------------------------------- */
/*
 * A document has two caller-defined 32-bit attributes, `group` and `stamp` (e.g. a ticker id and source bits; minutes
 * since an epoch).  A query carries one filter; document d passes when
 *     (group[d] & group_mask) == group_value  &&  stamp_lo <= stamp[d] && stamp[d] <= stamp_hi      (bounds inclusive)
 * {0, 0, 0, 0xFFFFFFFF} passes every document.
 *
 * A filter selects documents; it changes no score.  BM25 idf and average length stay the whole collection's (finalize /
 * finalize_sharded), cosine scores are the f32 values the unfiltered search returns for those rows.  A filtered list is the
 * unfiltered full ranking restricted to the passing documents and cut at `depth`: same order (score desc, doc id asc),
 * the BM25 list holds scores > 0 only, counts[q] is anything from 0 to depth.  RRF fuses the two filtered lists as usual.
 *
 * oi_index_set_doc_attrs: `n_docs` entries each, indexed by LOCAL row; either array may be NULL (zeros).  Allowed before or
 * after finalize.  The index holds one interleaved {group, stamp} pair per row (8 B), allocated by the first call and never
 * reallocated: a later call overwrites it in place, stream-ordered on the index's ctx (retag or "soft-delete" documents
 * without a rebuild).  Views alias it like every other index buffer and see later updates; a view made before any
 * attributes existed has none.  On a view: OI_ERR_STATE.
 *
 * The *_filtered calls take the arguments of their unfiltered twin plus `filters` (n_queries entries, where `location`
 * says).  filters == NULL: exactly the unfiltered call (same kernels, same bytes).  A filtered search on an index without
 * attributes returns OI_ERR_STATE.  oi_search_sharded_filtered: each rank filters its own shard; merge and fusion
 * are unchanged.  Graph replay (oi_set_graph_replay): the capture key includes the filters pointer; a replay reads the
 * filter and attribute CONTENTS at replay time, so changing either between replays is seen by the next one.
 */
typedef struct oi_doc_filter {
    uint32_t group_mask, group_value, stamp_lo, stamp_hi;
} oi_doc_filter;
int oi_index_set_doc_attrs(oi_index *idx, const uint32_t *group, const uint32_t *stamp, int location);
int oi_search_lists_filtered(oi_index *idx, const float *query_vecs, const uint32_t *query_terms,
                             const uint32_t *q_term_offsets, uint32_t n_queries, uint32_t depth,
                             const oi_doc_filter *filters, int location, float *cos_scores, uint32_t *cos_docs,
                             uint32_t *cos_counts, float *bm25_scores, uint32_t *bm25_docs, uint32_t *bm25_counts);
int oi_search_lists_packed_filtered(oi_index *idx, const float *query_vecs, const uint32_t *query_terms,
                                    const uint32_t *q_term_offsets, uint32_t n_queries, uint32_t depth,
                                    const oi_doc_filter *filters, int location, uint32_t *packed_out);
int oi_search_filtered(oi_index *idx, const float *query_vecs, const uint32_t *query_terms,
                       const uint32_t *q_term_offsets, uint32_t n_queries, uint32_t depth, uint32_t k,
                       const oi_doc_filter *filters, int location, float *scores_out, uint32_t *docs_out,
                       uint32_t *counts_out);
int oi_search_sharded_filtered(oi_index *idx, oi_comm *comm, const float *query_vecs, const uint32_t *query_terms,
                               const uint32_t *q_term_offsets, uint32_t n_queries, uint32_t depth, uint32_t k,
                               const oi_doc_filter *filters, int location, float *scores_out, uint32_t *docs_out,
                               uint32_t *counts_out);

/* ------------------------------------------------------------------------- */
/* Near-duplicate collapse of ranked lists                                      */
/* ------------------------------------------------------------------------- */
/*
 * Retweets, cross-posts and copy-pasta fill a ranked list with copies of one post.  These calls collapse them on the GPU (a
 * batched Gram matrix over rows already in HBM) instead of leaving every host to download pool x dim floats per query.
 * Builder-defined like the whole retrieval path; no reference counterpart (the reference has no embeddings, SURVEY.md
 * section 0).
 *
 * sim(a, b) is the dot product of the two STORED rows: for an f32 corpus the f32 rows as the index holds them (the cosine
 * for unit rows -- the convention of oi_search_lists), for a bf16 corpus the bf16 rows widened exactly to f32.  The library's
 * value is accumulated in f32 and is within 1e-5 of the f64 value for rows of norm <= 1.  A NaN similarity is never ">= t".
 *
 * The rule, on a ranked list e_0 .. e_{c-1} (rank order, c = counts[q]) and a threshold t: walk the list in rank order;
 * e_i is KEPT when no kept e_j, j < i, has sim(e_i, e_j) >= t; otherwise it is COLLAPSED INTO ITS REPRESENTATIVE, the
 * best-ranked kept e_j with sim >= t (the first such entry, not the most similar one).  Greedy, not transitive: A~B, B~C,
 * A!~C keeps A and C.  Out come the kept entries in rank order, cut at k, each with its input score bit for bit;
 * dup_counts[r] is 1 + the number of entries of the WHOLE input list collapsed into kept entry r, those ranked after the
 * k-th kept entry included.
 *
 * An entry whose doc id lies outside this handle's shard [doc_id_base, doc_id_base + n_docs) is a SINGLETON: it is kept,
 * nothing collapses into it, and no row is read for it.  This is the rule that keeps the kernels in bounds on any input;
 * there is no error for it.  (The same doc id twice in a list is two entries like any other two.)
 *
 * Pairs whose true similarity is within 1e-5 of t may fall on either side: the result is the greedy collapse under the
 * library's f32 similarities (a k-ordered fused-multiply-add chain), deterministic for a given build and input -- compare
 * the ties of two summation orders under OI_COSINE_SCREEN above.
 *
 * oi_collapse_lists: any ranked list of this index's documents (cosine, BM25 or fused).  Input row stride `depth`
 *   (1 .. OI_MAX_DEPTH), output row stride `k` (1 .. OI_MAX_DEPTH), first counts_out[q] entries of a row valid.  scores may
 *   be NULL: scores_out is then not written and may be NULL too.  dup_counts_out may be NULL.  OI_DEVICE: asynchronous on
 *   the ctx stream, like oi_rrf_fuse.  Works on a view; needs the embeddings only (no forward index, no finalize): an index
 *   without embeddings -> OI_ERR_STATE.  threshold NaN, depth or k out of range, a null required buffer -> OI_ERR_INVALID_ARG.
 * oi_search_collapsed: by definition oi_search_filtered(.., depth, k = pool, filters) followed by
 *   oi_collapse_lists(.., depth = pool, threshold, k) -- the fused pool-list stays on the device between the two.
 *   filters == NULL: the unfiltered search.  pool in [1, OI_MAX_DEPTH], k in [1, pool]; scores out are the RRF scores.
 *   Graph replay (oi_set_graph_replay): the collapse launches are captured with the rest of the call; the key includes
 *   pool, k, the threshold and all four output pointers.
 * Workspace: a pair mask of at most 32 MB per searching context, whatever n_queries (the batch runs in slices of queries).
 *
 * NOT covered: oi_search_sharded* and oi_pipeline_*.  A globally merged list holds rows of other ranks, and collapsing it
 * needs a row exchange.  Until then a sharded host can collapse per shard with oi_collapse_lists, under the singleton rule.
 */
int oi_collapse_lists(oi_index *idx, const float *scores, const uint32_t *docs, const uint32_t *counts,
                      uint32_t n_queries, uint32_t depth, float threshold, uint32_t k, int location,
                      float *scores_out, uint32_t *docs_out, uint32_t *counts_out, uint32_t *dup_counts_out);
int oi_search_collapsed(oi_index *idx, const float *query_vecs, const uint32_t *query_terms,
                        const uint32_t *q_term_offsets, uint32_t n_queries, uint32_t depth, uint32_t pool, uint32_t k,
                        float threshold, const oi_doc_filter *filters, int location,
                        float *scores_out, uint32_t *docs_out, uint32_t *counts_out, uint32_t *dup_counts_out);

/* ------------------------------------------------------------------------- */
/* Similarity volume: posts like a query, counted per time bucket              */
/* ------------------------------------------------------------------------- */
/*
 * Every other retrieval call returns a ranked list of at most OI_MAX_DEPTH posts.  This one keeps a COUNT instead of a list:
 * "how many posts of the index are like this one, and how has that number moved hour by hour?" -- the aggregation
 * counterpart of the filtered search.  Builder-defined like the whole retrieval path; no reference counterpart (the reference
 * counts posts per source in social_summary, it has no embeddings: SURVEY.md section 0).
 *
 * What a count is.  counts_out[q][b] is the number of local documents d of the handle for which all of these hold:
 *   1. d passes filters[q].  filters == NULL means every document passes.
 *   2. bucket_width == 0, or stamp_origin <= stamp[d] and (stamp[d] - stamp_origin) / bucket_width == b.  This is evaluated
 *      in 64 bits, so origin + n * width may exceed 2^32.
 *   3. sim(q, d) >= threshold.
 *
 * What sim is.  sim is the f32 value of the library's rescoring chain: lane l accumulates x_k * q_k over the float4s
 * l, l + 64, .. in k order with single fused multiply-adds, the wave butterfly sum follows.  The result is the score a
 * default (screened) oi_search_lists returns for that row, within 1e-5 of the f64 dot product for rows of norm <= 1.  On a
 * bf16 corpus the row is widened exactly and the query is rounded to bf16 the way that corpus's scorer rounds it.  A NaN
 * similarity is never >= t.
 *
 * Routes.  The value of sim does not depend on the route, so every route returns the same counts bit for bit: the call is
 * deterministic and its result is independent of cosine mode, screening-copy policy and batch composition.  An f32 corpus of
 * dim 384 / 768 with a bf16 screening copy under OI_COSINE_SCREEN / OI_COSINE_SCREEN_COPY is counted by ONE stream of the
 * copy: a pair whose screen score clears the threshold by the query's proven error bound is counted without its f32 row
 * being read, only the pairs inside the bound are rescored.  Everything else (other dims, a bf16 corpus, no copy,
 * OI_COSINE_EXACT / _SPLIT / _SCREEN_STREAM, a query without a bound, more than 4 Mi undecided pairs) takes the exact chain
 * over every row: correct for any input, slower.
 *
 * Rules.  spec is always a host pointer.  location says where the query vectors, the filters and counts_out live.
 * OI_DEVICE is asynchronous on the ctx stream.  The call needs embeddings only: no forward index, no finalize (an index
 * without embeddings -> OI_ERR_STATE), and it works on a view.  bucket_width > 0 or filters != NULL on an index without
 * attributes returns OI_ERR_STATE.  n_queries == 0 is OI_OK; n_queries <= 4096.  The call is not captured by graph replay
 * (oi_set_graph_replay) and always runs eagerly.  Workspace per searching context: the histogram and, on the screen route,
 * a band buffer of 32 MB (oi_workspace_bytes counts both).
 * Profile tags: "volume" (the stream), "volume_band" (the rescoring of the undecided pairs), "volume_exact" (the exact
 * route, and the runs of the fallback inside a screened call that really counted the batch).
 *
 * NOT covered: oi_search_sharded* and oi_pipeline_*.  Counts of shards add, so a sharded host sums the per-rank arrays.
 */
#define OI_MAX_VOLUME_BUCKETS 1024u
typedef struct oi_volume_spec {
    float    threshold;     /* count documents with sim >= threshold.  NaN: OI_ERR_INVALID_ARG; +-inf allowed */
    uint32_t stamp_origin;  /* lower edge of bucket 0 */
    uint32_t bucket_width;  /* > 0: bucket = (stamp - origin) / width.  0: no time axis, n_buckets must be 1 */
    uint32_t n_buckets;     /* 1 .. OI_MAX_VOLUME_BUCKETS */
} oi_volume_spec;
int oi_similar_volume(oi_index *idx, const float *query_vecs, uint32_t n_queries, const oi_volume_spec *spec,
                      const oi_doc_filter *filters, int location, uint32_t *counts_out /* [n_queries][n_buckets] */);

/* ------------------------------------------------------------------------- */
/* Similarity summary: the sentiment of posts like a query, per time bucket    */
/* ------------------------------------------------------------------------- */
/*
 * oi_similar_volume says how many posts are like a query; this call says what they FEEL: the raw sums of social_summary
 * (oi_social_counters: bullish / bearish / neutral, speculative count, posts per source, polarity sum) over exactly the
 * documents oi_similar_volume counts, one record per query and time bucket.  Nothing per post returns to the host.
 * Builder-defined like the whole retrieval path (the reference summarises a list of posts it already holds:
 * speculation_engine.rs:76-97; it has no embeddings).
 *
 * Signals.  oi_index_set_signals gives every local row its signal: `n_docs` entries each, indexed by LOCAL row, exactly
 * the buffers oi_lexicon_analyze[_device] writes and oi_social_summary reads (sources: 0 = reddit, 1 = bluesky; NULL = all
 * reddit).  With OI_DEVICE a host chains oi_lexicon_analyze_device -> oi_index_set_signals over the blob it also hands to
 * oi_index_set_text.  The index keeps one 8-byte record per row:
 *   v        = Polarity::new(polarity[d]): NaN -> 0, clamped to [-1, 1]
 *   pol_q30  = (int32) rint(v * 2^30), f64 round-to-nearest-even (the product is exact in f64)
 *   class    = bullish if v > bull_bear_threshold, bearish if v < -bull_bear_threshold, else neutral: the reference's
 *              comparisons on the f64 value (speculation_engine.rs:87-95)
 *   spec     = speculative[d] != 0,  source = sources[d] != 0
 * The class is fixed at set time with the caller's threshold; the summary call takes none.  The state rules are those of
 * oi_index_set_doc_attrs: the buffer (8 B per row) is allocated by the first call, never reallocated and overwritten in
 * place, stream-ordered on the index's ctx, by later calls; views alias it and see updates; a view made before signals
 * existed has none; on a view: OI_ERR_STATE; allowed before or after finalize.  bull_bear_threshold NaN, a null polarity or
 * speculative -> OI_ERR_INVALID_ARG.
 *
 * What a record is.  out[q][b] holds the social_summary raw sums over the local documents d of the handle for which all of
 * these hold -- word for word the clauses of oi_similar_volume, with the query's own threshold:
 *   1. d passes filters[q].  filters == NULL means every document passes.
 *   2. bucket_width == 0, or stamp_origin <= stamp[d] and (stamp[d] - stamp_origin) / bucket_width == b (evaluated in 64 bits).
 *   3. sim(q, d) >= t_q, where t_q = thresholds[q], or spec->threshold when thresholds == NULL.  sim is oi_similar_volume's
 *      sim.  A NaN thresholds[q] counts nothing for that query, in both locations (no score is >= NaN).
 * total, by_source[2], bullish, bearish, neutral and spec_count are exact integers.
 * polarity_sum = (double)(sum of pol_q30) * 2^-30, the sum taken in 64-bit integers.
 *
 * The contract that follows from it:
 *   - the result is deterministic and independent of the route, the order of the atomics, the cosine mode, the copy policy
 *     and the batch composition;
 *   - polarity_sum is an integer multiple of 2^-30;
 *   - |polarity_sum - sum of Polarity::new(polarity[d])| <= total * 2^-31;
 *   - the sum is exact when every polarity is dyadic, as in the reference's fixture (all of {-1, 0, 1});
 *   - sums of shards add exactly below 2^23 in magnitude;
 *   - total equals oi_similar_volume's count for the same arguments.
 *
 * Rules.  Those of oi_similar_volume: spec is always a host pointer; location says where the query vectors, the thresholds,
 * the filters and out live; OI_DEVICE is asynchronous on the ctx stream; embeddings only (no forward index, no finalize); it
 * works on a view; n_queries == 0 is OI_OK; n_queries <= 4096; not captured by graph replay.  In addition
 * n_queries * n_buckets > OI_MAX_SUMMARY_CELLS -> OI_ERR_INVALID_ARG; an index without signals -> OI_ERR_STATE;
 * bucket_width > 0 or filters != NULL on an index without attributes -> OI_ERR_STATE.  Workspace per searching context: 64 B
 * per cell, and the volume's 32 MB band buffer on the screen route (oi_workspace_bytes counts both).
 * Profile tags: "summary" (the stream), "summary_band" (the rescoring of the undecided pairs), "summary_exact" (the exact
 * route, and the runs of the fallback inside a screened call that really summed the batch).
 *
 * NOT covered: oi_search_sharded* and oi_pipeline_*.  A sharded host adds the records of its ranks.
 */
#define OI_MAX_SUMMARY_CELLS (1u << 18)
typedef struct oi_summary_spec {
    float    threshold;      /* used when thresholds == NULL; NaN then: OI_ERR_INVALID_ARG; +-inf allowed */
    uint32_t stamp_origin;   /* exactly oi_volume_spec's meaning and limits */
    uint32_t bucket_width;
    uint32_t n_buckets;
} oi_summary_spec;
int oi_index_set_signals(oi_index *idx, const double *polarity, const uint8_t *speculative,
                         const uint8_t *sources /* may be NULL: all reddit */, double bull_bear_threshold, int location);
int oi_similar_summary(oi_index *idx, const float *query_vecs, uint32_t n_queries, const oi_summary_spec *spec,
                       const float *thresholds /* [n_queries] where `location` says, or NULL */,
                       const oi_doc_filter *filters, int location, oi_social_counters *out /* [n_queries][n_buckets] */);

/* ------------------------------------------------------------------------- */
/* Similarity leaderboard: posts like a query, summed and ranked per group key */
/* ------------------------------------------------------------------------- */
/*
 * oi_similar_volume and oi_similar_summary break their result down along the time axis (the documents' stamp).  This call
 * breaks it down along the other per-document attribute, the GROUP (oi_index_set_doc_attrs: "a ticker id and source bits"):
 * "which tickers are the posts like this query about, and what do those posts feel?" -- one social_summary record per query
 * and key, all of them (dense) or the best `top` ranked on the device.  One stream of the screening copy decides every
 * (query, document) pair, whatever the number of keys.  Builder-defined like the whole retrieval path; its host counterpart
 * in the reference is the ranking of run_compare (src/mcp/tools.rs:227-349), which analyses a list of tickers one by one.
 *
 * The key.  key(d) = (group[d] & key_mask) >> ctz(key_mask).  key_mask is non-zero and one contiguous run of bits.  A document
 * whose key is >= n_keys belongs to no cell, like a stamp outside every bucket.
 *
 * What a cell is.  Cell (q, key) holds the social_summary raw sums over the local documents d of the handle for which all of
 * these hold -- word for word the clauses of oi_similar_summary, with "bucket" replaced by "key":
 *   1. d passes filters[q].  filters == NULL means every document passes.  A time window is expressed here, through the
 *      filter's stamp_lo / stamp_hi.
 *   2. key(d) == key.
 *   3. sim(q, d) >= t_q, where t_q = thresholds[q], or spec->threshold when thresholds == NULL.  sim is oi_similar_volume's
 *      sim.  A NaN thresholds[q] counts nothing for that query, in both locations (no score is >= NaN).
 * The sums are oi_similar_summary's: total, by_source[2], bullish, bearish, neutral and spec_count are exact integers, and
 * polarity_sum = (double)(sum of pol_q30) * 2^-30, the sum taken in 64-bit integers.  The result is therefore deterministic and
 * independent of the route, the order of the atomics, the cosine mode, the copy policy and the batch composition; summed over
 * the keys it equals oi_similar_summary's one-bucket record for the same arguments when every document has a key.
 *
 * Dense output (top == 0).  records_out[q][key] for key < n_keys; keys_out, counts_out and qualified_out are not written and
 * may be NULL.  This is what a sharded host adds across its ranks.
 *
 * Ranked output (top >= 1).  The rank value v of a cell is its record's total, spec_count, bullish or bearish, chosen by
 * rank_by.  The listed keys of a query are those with total >= max(min_total, 1), ordered by (v descending, key ascending) and
 * cut at top -- the library's usual 64-bit rank key, v << 32 | ~key.  keys_out[q][r] and records_out[q][r] have row stride top;
 * counts_out[q] is the number listed; qualified_out[q] (may be NULL) is the number of keys that qualified before the cut.
 * Entries past counts_out[q] are key 0xFFFFFFFF and an all-zero record.
 *
 * Rules.  Those of oi_similar_summary: spec is always a host pointer; location says where the query vectors, the thresholds,
 * the filters and all four outputs live; OI_DEVICE is asynchronous on the ctx stream; embeddings only (no forward index, no
 * finalize); it works on a view; n_queries == 0 is OI_OK; n_queries <= 4096; not captured by graph replay.  An index without
 * signals, or without doc attributes (the key axis always needs them), -> OI_ERR_STATE.  n_queries * n_keys >
 * OI_MAX_GROUP_CELLS, a bad key_mask, n_keys, top or rank_by, a null required buffer -> OI_ERR_INVALID_ARG with the number in
 * the message; every argument check precedes the first device call.  Workspace per searching context: 64 B per cell, 8 B
 * more per cell for ranked output, and the volume's 32 MB band buffer on the screen route (oi_workspace_bytes counts all).
 * Profile tags: "groups" (the stream), "groups_band" (the rescoring of the undecided pairs), "groups_exact" (the exact
 * route, and the runs of the fallback inside a screened call that really summed the batch), "groups_rank" (the rank keys and
 * the ranking of ranked output).
 *
 * NOT covered: oi_search_sharded* and oi_pipeline_*.  Records of shards add, so a sharded host asks every rank for dense
 * output, adds the records and ranks the sums; ranked lists of shards cannot be merged exactly (a key outside every shard's
 * list may lead the sum).
 */
#define OI_MAX_GROUP_KEYS  65536u
#define OI_MAX_GROUP_CELLS (1u << 20)     /* n_queries * n_keys; 64 MB of cells */
enum { OI_GROUP_RANK_TOTAL = 0, OI_GROUP_RANK_SPEC = 1, OI_GROUP_RANK_BULLISH = 2, OI_GROUP_RANK_BEARISH = 3 };
typedef struct oi_groups_spec {
    float    threshold;   /* used when thresholds == NULL (NaN then: OI_ERR_INVALID_ARG; +-inf allowed) */
    uint32_t key_mask;    /* non-zero, one contiguous run of bits */
    uint32_t n_keys;      /* 1 .. min(2^popcount(key_mask), OI_MAX_GROUP_KEYS) */
    uint32_t top;         /* 0: dense output;  1 .. OI_MAX_DEPTH: ranked output */
    uint32_t rank_by;     /* OI_GROUP_RANK_* */
    uint32_t min_total;   /* ranked output lists a key only when its total >= max(min_total, 1) */
} oi_groups_spec;
int oi_similar_groups(oi_index *idx, const float *query_vecs, uint32_t n_queries, const oi_groups_spec *spec,
                      const float *thresholds /* [n_queries] where `location` says, or NULL */,
                      const oi_doc_filter *filters, int location,
                      oi_social_counters *records_out /* [n_queries][n_keys], or [n_queries][top] */,
                      uint32_t *keys_out /* [n_queries][top] */, uint32_t *counts_out /* [n_queries] */,
                      uint32_t *qualified_out /* [n_queries], may be NULL */);

/* ------------------------------------------------------------------------- */
/* Similarity share: each post counted once, under the query it is most like   */
/* ------------------------------------------------------------------------- */
/*
 * oi_similar_volume, oi_similar_summary and oi_similar_groups decide every (query, document) pair on its own: a post that
 * resembles three queries of a batch is counted three times.  This call is the EXCLUSIVE form, for a batch of narratives
 * ("short squeeze", "earnings beat", "lawsuit", "dilution") among which the posts are to be divided: every post is counted at
 * most once, under the query it is most like.  It is the classification counterpart of the threshold family and the
 * assignment step of any clustering a host may run over the index.  Builder-defined like the whole retrieval path.
 *
 * The definition.  For a local document d, the CANDIDATES are the queries q for which clauses 1 and 3 of oi_similar_summary
 * hold:
 *   - d passes filters[q].  filters == NULL means every document passes.
 *   - sim(q, d) >= t_q, where t_q = thresholds[q], or spec->threshold when thresholds == NULL.  sim is oi_similar_volume's
 *     sim.  A NaN t_q makes q nobody's candidate.  A NaN similarity is never >=.
 * The WINNER of d is the candidate with the largest sim(q, d), compared as the f32 values of the library's chain.  Ties go
 * to the smallest q.
 * d is ASSIGNED when it has a winner and clause 2 holds: bucket_width == 0, or stamp_origin <= stamp[d] and
 * b = (stamp[d] - stamp_origin) / bucket_width < n_buckets (evaluated in 64 bits).
 * out[q][b] holds the social_summary raw sums over the documents assigned to q in bucket b.  The fields and the integer
 * arithmetic are oi_similar_summary's: total, by_source[2], bullish, bearish, neutral and spec_count are exact integers, and
 * polarity_sum = (double)(sum of pol_q30) * 2^-30, the sum taken in 64-bit integers.
 * labels_out[d] is the winner of an assigned document and 0xFFFFFFFF for every other row.  labels_out may be NULL.
 *
 * The contract that follows from it:
 *   - every document is in at most one cell;
 *   - out[q][b].total <= oi_similar_summary's for the same arguments;
 *   - summed over q, the totals equal the number of documents with at least one candidate and a bucket;
 *   - with n_queries == 1 the records are oi_similar_summary's bit for bit;
 *   - so are they with pairwise disjoint filters;
 *   - a query that repeats an earlier one with the same threshold and filter gets all-zero records;
 *   - the result is deterministic and independent of the route, the order of the atomics, the cosine mode and the copy policy;
 *   - unlike its siblings it DOES depend on the batch composition: adding, removing or reordering queries moves posts
 *     between records.  That is the point of the call;
 *   - pairs whose true similarities lie within 1e-5 of each other, or of the threshold, may fall either way under the f32
 *     chain (the same sentence as for the collapse and the screen).
 *
 * Rules.  Those of oi_similar_summary: spec is always a host pointer; location says where the query vectors, the thresholds,
 * the filters, out and labels_out live; OI_DEVICE is asynchronous on the ctx stream; embeddings only (no forward index, no
 * finalize); it works on a view; n_queries == 0 is OI_OK (labels_out, when given, is all 0xFFFFFFFF); n_queries <= 4096;
 * n_queries * n_buckets <= OI_MAX_SUMMARY_CELLS; not captured by graph replay.  An index without signals -> OI_ERR_STATE;
 * bucket_width > 0 or filters != NULL on an index without attributes -> OI_ERR_STATE.  A null spec, index, query or out
 * buffer, a NaN spec->threshold without an array, n_queries or the cell count out of range -> OI_ERR_INVALID_ARG with the
 * number in the message; every argument check precedes the first device call.
 * Routes.  Up to 64 queries on a screened f32 corpus (dim 384 / 768 with a screening copy) take ONE stream of the copy: a row
 * that a single query can reach is decided there, the others are rescored exactly.  More than 64 queries, other corpora and
 * the exact cosine modes take the exact route; the result is the same.
 * Workspace per searching context: 64 B per cell; on the stream route also the volume's 32 MB band buffer, 16.25 MB of keys
 * beside it and `best`, 8 B per local row (oi_workspace_bytes counts all of them); with OI_HOST, 4 B per local row more when
 * labels_out is given.
 * Profile tags: "share" (the stream), "share_band" (rescoring and commit of the undecided rows), "share_exact" (the exact
 * route, and the runs of the fallback inside a screened call that really did the work); "share_state" reads the band fill
 * and the gate / overflow bits of the last call.
 *
 * NOT covered: oi_search_sharded* and oi_pipeline_*.  Winners of shards do not add when the QUERIES are sharded; a host that
 * shards the queries must exchange the per-row best key.  (Shards of the DOCUMENTS hold disjoint rows: their records add.)
 */
int oi_similar_share(oi_index *idx, const float *query_vecs, uint32_t n_queries, const oi_summary_spec *spec,
                     const float *thresholds /* [n_queries] where `location` says, or NULL */,
                     const oi_doc_filter *filters, int location,
                     oi_social_counters *out /* [n_queries][n_buckets] */,
                     uint32_t *labels_out /* [n_docs] by LOCAL row where `location` says, or NULL */);

/* ------------------------------------------------------------------------- */
/* Narrative discovery: centroid sums and a k-means loop over the index        */
/* ------------------------------------------------------------------------- */
/*
 * oi_similar_share is the ASSIGNMENT step of a clustering over the index; these three calls are the rest of it.  With them a
 * host asks not "how many posts are like the narratives I know" but "which narratives are there": seed a few vectors, let
 * assignment and update alternate on the device, and read the moved narratives, their records and the label of every post.
 * Builder-defined like the whole retrieval path.
 *
 * oi_label_sums -- the update step's reduction.  For every local row d with labels[d] < n_clusters: counts[labels[d]] += 1,
 * and for every k: sums[labels[d]][k] += fix(x_dk), where fix(x) = (int64) rint(v * 2^30) and v is x with NaN -> 0, clamped
 * to [-1, 1].  x_dk is the stored row element: the f32 value, or the bf16 value widened exactly.  A label >= n_clusters
 * (0xFFFFFFFF included) is "no cluster": the row is not read, and there is no error for it.  No element of a unit row is
 * clamped, and x * 2^30 is exact in f32.  The sums are 64-bit integers (|sum| <= 2^62 for any shard), so the result is a
 * function of the inputs alone -- independent of grid, order of the atomics, route and run -- and the sums and counts of
 * document shards ADD exactly (the choice of pol_q30 in oi_similar_summary).
 * Rules: location says where labels, sums_out and counts_out live; OI_DEVICE is asynchronous on the ctx stream and needs no
 * workspace; OI_HOST stages 4 B per row + 8 B per sum and count in the ctx workspace.  Embeddings only (no forward index, no
 * finalize, no signals, no attributes); it works on a view; an f32 corpus of any supported dim and a bf16 corpus;
 * n_clusters in [1, OI_MAX_CENTROIDS].  A null index, null buffer or n_clusters out of range -> OI_ERR_INVALID_ARG with the
 * number in the message, before the first device call.  Not captured by graph replay.  Profile tag "label_sums".
 *
 * oi_centroids_from_sums -- sums to unit vectors; a call of its own because a sharded host adds the per-rank integer sums
 * and counts first.  Per cluster c: v_k = (double)sums[c][k] * 2^-30; n2 is accumulated from +0.0 in ascending k as
 * n2 = n2 + v_k * v_k (one rounded f64 multiply, one rounded f64 add, no fma); centroids_out[c][k] = (float)(v_k / sqrt(n2))
 * with IEEE f64 divide and square root and round-to-nearest-even narrowing.  If counts[c] == 0 or n2 == 0 the cluster keeps
 * previous[c] bit for bit (all zeros when previous == NULL).  centroids_out may alias previous.  location says where the four
 * arrays live; n_clusters in [1, OI_MAX_CENTROIDS]; dim a multiple of 4, <= OI_MAX_DIM.  Profile tag "centroids".
 *
 * oi_narratives_fit -- the loop.  c_1 = seeds.  Assignment step i is oi_similar_share with queries c_i, spec's first four
 * fields, no per-query thresholds and `filter` (when given) for every query; it gives labels_i and records_i.  moved_i is the
 * number of rows with labels_i[d] != labels_{i-1}[d]; for i = 1, the number of assigned rows.  If i > 1 and moved_i == 0 the
 * fit has converged; if i == max_iters it stops unconverged; otherwise
 * c_{i+1} = oi_centroids_from_sums(oi_label_sums(labels_i), previous = c_i).  The outputs describe the LAST assignment step:
 * centroids_out = c_i, records_out = records_i, labels_out = labels_i, info = {i, converged, moved_i, assigned rows}.  So
 * oi_similar_share with centroids_out as queries and the same spec and filter returns records_out and labels_out bit for
 * bit.  An empty cluster keeps its vector; a duplicate seed stays empty, by the share's tie rule.
 * Rules: state and argument rules are oi_similar_share's (signals required; attributes required when a filter or a time axis
 * is given; it works on a view); n_clusters in [1, OI_MAX_CENTROIDS], max_iters in [1, 64]; spec, filter and info_host are
 * always host pointers; location covers the seeds and the three outputs; labels_out may be NULL.  The call reads `moved` once
 * per step: it SYNCHRONISES the ctx stream in both locations.  Never captured by graph replay.  Routes: those of the share.
 * Workspace, beside the share's: two label arrays (4 B per local row each), the sums (8 B x n_clusters x dim), the counts,
 * two centroid sets, the replicated filter, and with OI_HOST the records (oi_workspace_bytes counts all of them).
 * Profile tags: "label_sums" and "centroids" as above, "fit_moved" (the moved / assigned count of a step), and the share's.
 *
 * NOT covered: a sharded or pipelined form (shards of the documents add their oi_label_sums outputs and call
 * oi_centroids_from_sums on the total); the seeds come from the caller or from oi_narratives_seed (below); one threshold
 * for all clusters; at most 256 clusters.
 */
#define OI_MAX_CENTROIDS 256u
int oi_label_sums(oi_index *idx, const uint32_t *labels /* [n_docs] by LOCAL row */, uint32_t n_clusters, int location,
                  int64_t *sums_out /* [n_clusters][dim] */, uint64_t *counts_out /* [n_clusters] */);
int oi_centroids_from_sums(oi_ctx *ctx, const int64_t *sums, const uint64_t *counts, const float *previous /* or NULL */,
                           uint32_t n_clusters, uint32_t dim, int location, float *centroids_out /* [n_clusters][dim] */);

typedef struct oi_narrative_spec {
    float    threshold;      /* oi_summary_spec's four fields, same meaning and limits, one threshold for all clusters */
    uint32_t stamp_origin, bucket_width, n_buckets;
    uint32_t max_iters;      /* 1 .. 64 assignment steps */
} oi_narrative_spec;
typedef struct oi_narrative_info { uint32_t iterations, converged; uint64_t moved, assigned; } oi_narrative_info;
int oi_narratives_fit(oi_index *idx, const float *seeds /* [n_clusters][dim] */, uint32_t n_clusters,
                      const oi_narrative_spec *spec, const oi_doc_filter *filter /* ONE, host pointer, or NULL */, int location,
                      float *centroids_out /* [n_clusters][dim] */, oi_social_counters *records_out /* [n_clusters][n_buckets] */,
                      uint32_t *labels_out /* [n_docs] by LOCAL row, or NULL */, oi_narrative_info *info_host);

/* ------------------------------------------------------------------------- */
/* Narrative seeding: greedy k-means++ over the index on the device            */
/* ------------------------------------------------------------------------- */
/*
 * oi_narratives_fit starts from seed vectors; a host that does not know vectors close to the narratives gets them here,
 * without a row leaving the device.  oi_narratives_seed chooses n_clusters STORED ROWS of the index as seeds: greedy
 * k-means++ (D^2 sampling, the best of `trials` candidates per seed) or farthest-first.  Builder-defined like the whole
 * retrieval path.
 *
 * Eligible rows.  A row d is ELIGIBLE when it passes `filter` (if one is given) and bucket_width == 0 or it has a bucket:
 * stamp_origin <= stamp[d] and (stamp[d] - stamp_origin) / bucket_width < n_buckets (evaluated in 64 bits).  This is the set
 * oi_narratives_fit assigns from.  E is the number of eligible rows.
 *
 * sim and weight.  sim(p, d) is oi_similar_volume's sim with the stored row p as the query: the f32 value of the library's
 * chain (on a bf16 corpus both rows are widened exactly, so the query rounding is the identity).
 * weight(s) = (uint32) rintf(min(max(1.0f - s, 0), 2) * 2^20): one rounded f32 subtract, an exact scale; weight(NaN) = 0.
 * For unit rows the weight is proportional to the squared distance.  Weights are integers <= 2^21 and every sum is a 64-bit
 * integer, so the result is a function of the inputs alone.
 *
 * RNG.  u(i, t) = splitmix64(seed + (8 * i + t + 1) * 0x9E3779B97F4A7C15), where splitmix64(z) is z ^= z >> 30;
 * z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31, all mod 2^64.  A target below a total W is
 * r = mulhi64(u, W), the high 64 bits of the 128-bit product (not u mod W: mulhi64 moves continuously with W).
 *
 * Seed 0.  p_0 is the mulhi64(u(0, 0), E)-th eligible row in row order.  w_1[d] = weight(sim(p_0, d)) for eligible d != p_0;
 * w_1[d] = 0 for p_0 and for every ineligible row.
 *
 * Seed i >= 1, OI_SEED_KMEANSPP with trials = L in 1 .. 8.  W = sum of w_i; if W == 0, stop with found = i.  For each
 * t < L: r_t = mulhi64(u(i, t), W), and candidate c_t is the smallest row whose inclusive prefix sum of w_i in row order
 * exceeds r_t (candidates may repeat).  wc_t[d] = weight(sim(c_t, d)) for eligible d, with wc_t[c_t] = 0 and wc_t[d] = 0 for
 * ineligible rows.  pot_t = sum over d of min(w_i[d], wc_t[d]).  The step takes t* = argmin pot_t, ties to the smallest t.
 * p_i = c_t*, w_{i+1} = min(w_i, wc_t*), and the next W is pot_t*.
 *
 * Seed i >= 1, OI_SEED_FARTHEST (trials must be 1).  p_i is the row with the largest w_i, ties to the smallest row; if the
 * maximum is 0, stop with found = i.  The update is the same.  Seed 0 is chosen as above.
 *
 * Outputs.  seeds_out[i] is the stored row p_i as f32, bit for bit (a bf16 row widened exactly); rows_out[i] = p_i, the LOCAL
 * row.  Seeds at and beyond `found` are all-zero vectors with row 0xFFFFFFFF.  info = {found, eligible = E, potential = the
 * sum of w after the last seed}.  A chosen row has weight 0 from then on, so the seeds are distinct rows.
 *
 * Caveats.  Seed 0 is uniform over the eligible rows whatever they hold: if it is a NaN row every weight becomes 0 and
 * found = 1.  On float embeddings the similarities are only within 1e-5 of f64 (the sentence the share carries): the choice
 * is deterministic per build and independent of the cosine mode and the copy policy, but it is not pinned against f64.
 *
 * Rules.  Embeddings only: no signals, no forward index, no finalize; attributes are required only when a filter or
 * bucket_width > 0 is given (without them -> OI_ERR_STATE); it works on a view; an f32 corpus of any supported dim and a
 * bf16 corpus.  n_clusters in [1, OI_MAX_CENTROIDS], trials in [1, OI_MAX_SEED_TRIALS], n_buckets in
 * [1, OI_MAX_VOLUME_BUCKETS] (1 when bucket_width == 0).  An unknown method, OI_SEED_FARTHEST with trials != 1,
 * reserved != 0, a number out of range, a null spec, index or seeds_out -> OI_ERR_INVALID_ARG with the number in the
 * message, before the first device call.  E == 0 is OK with found = 0.  `location` covers seeds_out and rows_out (rows_out
 * may be NULL); spec, filter and info_host are always host pointers.  The seed loop runs without a host synchronise between
 * its steps: two launches per seed, and once W == 0 every later launch of the call exits at once.  With info_host != NULL
 * the call synchronises the ctx stream once at the end to read 24 bytes; with NULL and OI_DEVICE it is fully asynchronous.
 * Never captured by graph replay.
 * Workspace "seeds" per searching context, every part rounded up to 256 B (oi_workspace_bytes counts it): 256 B of state;
 * w, 4 B per local row; cw, 4 * trials B per local row, only when trials > 1; the partial sums, 8 * trials B per range of
 * 2048 rows; with OI_SEED_FARTHEST 8 B more per range; the candidate vectors, 4 * trials * dim B.  With OI_HOST the seeds
 * and rows are staged in "seeds_io".
 * Profile tags: "seed_init" (eligibility), "seed_score" (one stream of the rows per seed), "seed_pick" (one per seed + 1).
 *
 * NOT covered: streaming the bf16 screening copy for the passes; a sharded form; k-means|| or other schemes that take more
 * than one seed per pass.
 */
#define OI_SEED_KMEANSPP 0u
#define OI_SEED_FARTHEST 1u
#define OI_MAX_SEED_TRIALS 8u
typedef struct oi_seed_spec {
    uint32_t method, trials;   /* OI_SEED_*; candidates per seed, 1 .. OI_MAX_SEED_TRIALS (1 with OI_SEED_FARTHEST) */
    uint64_t seed;             /* of the RNG above */
    uint32_t stamp_origin, bucket_width, n_buckets, reserved;   /* oi_narrative_spec's time axis; reserved == 0 */
} oi_seed_spec;
typedef struct oi_seed_info { uint32_t found, reserved; uint64_t eligible, potential; } oi_seed_info;
int oi_narratives_seed(oi_index *idx, uint32_t n_clusters, const oi_seed_spec *spec,
                       const oi_doc_filter *filter /* ONE, host pointer, or NULL */, int location,
                       float *seeds_out /* [n_clusters][dim] */, uint32_t *rows_out /* [n_clusters], or NULL */,
                       oi_seed_info *info_host /* or NULL */);

/* ------------------------------------------------------------------------- */
/* Mention summary: posts containing a query's terms, per bucket or ticker     */
/* ------------------------------------------------------------------------- */
/*
 * The lexical member of the aggregation family, and the one a host WITHOUT embeddings can use: "how many posts mention gme
 * and squeeze, hour by hour, and were they bullish?"  oi_similar_volume / _summary / _groups / _share decide a document by
 * sim(q, d) >= t; this call decides it by the TERMS it contains, read from the postings oi_index_finalize made, and returns
 * the same social_summary records -- per time bucket (OI_MENTION_AXIS_TIME) or per key of the documents' group attribute
 * (OI_MENTION_AXIS_KEY).  Nothing per post returns to the host and no list is cut at OI_MAX_DEPTH.  It is the reference's
 * own question (social_summary over the posts that mention a ticker) asked of the index.
 *
 * The definition.
 *   D_q is the set of DISTINCT term ids in query_terms[q_term_offsets[q] .. q_term_offsets[q+1]).  A repeated term counts
 *     once -- unlike BM25, where it counts each time.  A term id >= vocab occurs in no document, but it is a member of D_q.
 *   m(q, d) is the number of t in D_q with a posting for local document d.
 *   need_q: min_match == NULL gives 1 (ANY); min_match[q] == 0 gives |D_q| (ALL); otherwise it is min_match[q].
 *   d MATCHES q when |D_q| >= 1 and m(q, d) >= need_q.  An empty query matches nothing; need_q > |D_q| matches nothing.
 * out[q][c] holds the social_summary raw sums over the local documents d of the handle that match q, pass filters[q] and
 * fall into cell c:
 *   - the pass clause is oi_similar_summary's clause 1: d passes filters[q]; filters == NULL means every document passes;
 *   - on the TIME axis the cell is oi_similar_summary's clause 2: bucket_width == 0 (one cell, c = 0), or stamp_origin <=
 *     stamp[d] and (stamp[d] - stamp_origin) / bucket_width == c (evaluated in 64 bits);
 *   - on the KEY axis the cell is oi_similar_groups's key clause: (group[d] & key_mask) >> ctz(key_mask) == c, and a key >=
 *     n_cells belongs to no cell.
 * The fields and the integer arithmetic are oi_similar_summary's: total, by_source[2], bullish, bearish, neutral and
 * spec_count are exact integers, and polarity_sum = (double)(sum of pol_q30) * 2^-30, the sum taken in 64-bit integers.
 *
 * The contract that follows from it:
 *   - the result is deterministic and independent of the order of the atomics, the grid and the batch composition;
 *   - with one term, no filter and one cell, total equals the term's local df (oi_index_local_stats);
 *   - with min_match == NULL the matching set of a query equals the set of documents with BM25 score > 0 for it (every idf
 *     is > 0);
 *   - records of document shards add.
 *
 * Limits.  At most OI_MAX_MENTION_TERMS raw terms per query, duplicates included.  With OI_HOST a longer query is
 * OI_ERR_INVALID_ARG, naming the query and the count.  With OI_DEVICE the offsets are not host-visible: such a query gets
 * all-zero records, and nothing is read or written out of bounds for it.  n_queries <= 4096; n_queries * n_cells <=
 * OI_MAX_GROUP_CELLS; n_queries == 0 is OI_OK.
 *
 * Rules.  spec is always a host pointer; location says where the terms, the offsets, min_match, the filters and out live;
 * OI_DEVICE is asynchronous on the ctx stream; not captured by graph replay.  A finalized index is required (the postings),
 * and signals (oi_index_set_signals): otherwise OI_ERR_STATE.  Doc attributes are required when bucket_width > 0, when
 * filters != NULL, or on the KEY axis: otherwise OI_ERR_STATE.  NO embeddings are needed.  It works on a view (views alias
 * the postings, cell_start, the signals and the attributes).  A null spec, a bad axis, n_cells, bucket_width, key_mask,
 * n_queries or cell count out of range, a null terms, offsets or out buffer, a bad location -> OI_ERR_INVALID_ARG with the
 * number in the message; every argument check precedes the first device call.
 * Workspace per searching context: 64 B per cell and the per-query plan, 272 B per query (oi_workspace_bytes counts both);
 * with OI_HOST also the staged inputs and records.  Profile tags: "mention_plan" (the distinct terms and need_q of every
 * query) and "mention" (the match: postings counted in LDS, matches summed).
 *
 * NOT covered: oi_search_sharded* and oi_pipeline_*.  A sharded host adds the records of its ranks.
 */
#define OI_MAX_MENTION_TERMS 64u
enum { OI_MENTION_AXIS_TIME = 0, OI_MENTION_AXIS_KEY = 1 };
typedef struct oi_mention_spec {
    uint32_t axis;          /* OI_MENTION_AXIS_* */
    uint32_t stamp_origin;  /* TIME: oi_summary_spec's meaning.             KEY: key_mask (non-zero, one contiguous run of bits) */
    uint32_t bucket_width;  /* TIME: oi_summary_spec's (0: no axis, 1 cell). KEY: must be 0 */
    uint32_t n_cells;       /* TIME: 1 .. OI_MAX_VOLUME_BUCKETS.             KEY: 1 .. min(2^popcount(mask), OI_MAX_GROUP_KEYS) */
} oi_mention_spec;
int oi_mention_summary(oi_index *idx, const uint32_t *query_terms, const uint32_t *q_term_offsets, uint32_t n_queries,
                       const oi_mention_spec *spec, const uint32_t *min_match /* [n_queries] where `location` says, or NULL */,
                       const oi_doc_filter *filters /* or NULL */, int location,
                       oi_social_counters *out /* [n_queries][n_cells] */);

/* ------------------------------------------------------------------------- */
/* Narrative terms: the distinguishing terms of each cluster of posts          */
/* ------------------------------------------------------------------------- */
/*
 * oi_narratives_fit and oi_similar_share say which narratives there are, how big they are and which post belongs to which;
 * these calls say what a narrative is ABOUT: for every cluster of a labelling, the terms its posts hold more often than the
 * assigned posts at large (the step a host otherwise takes with c-TF-IDF on the CPU, after pulling the labels and the forward
 * index off the device).  They read the postings oi_index_finalize made and the labels where they are.  The lexical
 * counterpart of oi_label_sums, as oi_mention_summary is of oi_similar_summary.  The term ids they return are valid
 * query_terms of oi_mention_summary and of every oi_search* call.  Builder-defined like the whole retrieval path.
 *
 * The table.  labels[d] is a u32 per LOCAL row.  A label >= n_clusters (0xFFFFFFFF included) is "no cluster", as in
 * oi_label_sums: the row counts nowhere, and there is no error for it.
 *   sizes[c]     = the number of local rows with labels[d] == c; it equals the counts of oi_label_sums for the same labels.
 *   counts[t][c] = the number of local documents d with labels[d] == c that have a posting for term t.  A term counts once
 *                  per document, however often it occurs.  The layout is [vocab][n_clusters] u32, term-major like the postings.
 * All of these are exact integers: the table does not depend on the grid, the order of any atomics or the run, and the tables
 * and sizes of document shards ADD.
 *
 * The ranked cut is a function of a table, sizes and a spec only.
 *   A = sum_c sizes[c] and dfA[t] = sum_c counts[t][c], taken in 64 bits.
 *   Term t is ELIGIBLE for cluster c when counts[t][c] >= max(min_df, 1).
 *   excess(c, t) = (int64)counts[t][c] * A - (int64)sizes[c] * dfA[t]: A times (observed minus expected documents of c
 *     holding t).  A term spread evenly over the clusters scores about 0 whatever its frequency, a frequent term concentrated
 *     in c scores high, a rare term scores low even at high lift.
 *   The order within a cluster is excess descending, then counts[t][c] descending, then t ascending: a total order, so the
 *     lists are unique.  With n_clusters == 1 every excess is 0 and the list holds the cluster's most frequent terms.
 *   Cluster c returns n[c] = min(top, number of eligible terms) records {term, df_cluster = counts[t][c], df_assigned =
 *     dfA[t] (its low 32 bits), reserved = 0, excess}; entries at and beyond n[c] are all-zero records with term = 0xFFFFFFFF.
 *   With df_cluster, df_assigned, sizes[c] and A the host has every integer it needs to re-rank by lift, PMI or c-TF-IDF.
 * Overflow is ruled out by a check, not by saturation: A <= 2^31 - 1 is required, and then every product is below 2^62 for a
 * consistent table (dfA[t] <= A).  An inconsistent caller-made table wraps in two's complement; nothing is read or written
 * out of bounds for it.
 *
 * oi_label_term_counts -- labels to the table and the sizes.  oi_label_terms_rank -- a table and sizes to the lists; a call
 * of its own for the reason oi_centroids_from_sums is one: a sharded host adds the per-rank tables and sizes with its own
 * all-reduce and ranks the total.  oi_label_terms -- their composition for a single-GPU host: the table never leaves the ctx
 * workspace; sizes_out may be NULL.
 *
 * Rules.  oi_label_term_counts and oi_label_terms need a FINALIZED index (the postings): otherwise OI_ERR_STATE.  They need
 * NO embeddings, signals or attributes, and they work on a view.  n_clusters in [1, OI_MAX_CENTROIDS]; vocab * n_clusters <=
 * OI_MAX_LABEL_TERM_CELLS; top in [1, OI_MAX_LABEL_TERMS]; reserved == 0; min_df is any value (0 means 1).  oi_label_terms
 * additionally requires n_docs <= 2^31 - 1 (so A is in range without reading the sizes back).  sizes_host and spec are always
 * host pointers (the sizes are at most 2 KB, the A check runs on them, and they are read before the call returns); location
 * covers the labels, the tables, the records, n_out, and sizes_out of oi_label_term_counts and oi_label_terms.  With OI_DEVICE
 * the calls are asynchronous on the ctx stream.  Not captured by graph replay.  A null handle, spec or buffer, a number out of
 * range, A > 2^31 - 1, a bad location -> OI_ERR_INVALID_ARG with the offending number in the message; every argument check
 * precedes the first device call.
 * Workspace per searching context (oi_workspace_bytes counts it): "label_terms" holds the table of the composite call
 * (4 B x vocab x n_clusters), the sizes, and the rank's partial lists (16 B x top x n_clusters per slice of 1024 terms, and
 * 1/64 of that again); "label_terms_plan" holds 4 B per 16384 postings.  With OI_HOST the staged labels, table and records
 * are held in "label_terms_io".
 * Profile tags: "label_term_counts" (the pass over the postings and the pass over the labels) and "label_terms_rank".
 *
 * NOT covered: a time axis (one list per cluster and bucket); a background other than the assigned posts, such as the whole
 * index's df; oi_search_sharded* / oi_pipeline_* forms; mapping ids back to words inside the library (the vocabulary is
 * hashed: a host names the ids by hashing the tokens of a sample of posts with oi_text_terms).
 */
#define OI_MAX_LABEL_TERMS 64u             /* `top` per cluster */
#define OI_MAX_LABEL_TERM_CELLS (1u << 28) /* vocab * n_clusters: 1 GiB of u32 at most */
typedef struct oi_label_terms_spec { uint32_t top, min_df, reserved[2]; } oi_label_terms_spec;
typedef struct oi_label_term { uint32_t term, df_cluster, df_assigned, reserved; int64_t excess; } oi_label_term;
int oi_label_term_counts(oi_index *idx, const uint32_t *labels /* [n_docs] by LOCAL row */, uint32_t n_clusters, int location,
                         uint32_t *counts_out /* [vocab][n_clusters] */, uint64_t *sizes_out /* [n_clusters] */);
int oi_label_terms_rank(oi_ctx *ctx, const uint32_t *counts, const uint64_t *sizes_host, uint32_t vocab, uint32_t n_clusters,
                        const oi_label_terms_spec *spec, int location,
                        oi_label_term *terms_out /* [n_clusters][top] */, uint32_t *n_out /* [n_clusters] */);
int oi_label_terms(oi_index *idx, const uint32_t *labels, uint32_t n_clusters, const oi_label_terms_spec *spec, int location,
                   oi_label_term *terms_out, uint32_t *n_out, uint64_t *sizes_out /* or NULL */);

/* ------------------------------------------------------------------------- */
/* Narrative exemplars: the most central posts of each cluster                */
/* ------------------------------------------------------------------------- */
/*
 * oi_narratives_fit says which narratives there are and which post belongs to which, oi_label_terms what each is about; this
 * call returns THE POSTS TO QUOTE: for every cluster of a labelling, the stored posts closest to the cluster's centroid, among
 * the posts the labelling gave it.  (A search with the centroids as queries returns each centroid's nearest posts in the whole
 * index -- under the share's tie and exclusivity rules a different set -- and a filter tests group and stamp, not a label.)
 * Builder-defined like the whole retrieval path.
 *
 * The lists.  labels[d] is a u32 per LOCAL row.  Row d is a MEMBER of cluster c when
 *   labels[d] == c < n_clusters   (any other label, 0xFFFFFFFF included, is "no cluster", as in oi_label_sums: the row is not
 *                                  read), and
 *   d passes `filter`, when one is given, and
 *   s = sim(centroids[c], d) is not NaN.
 * sim is oi_similar_volume's sim with the centroid as the query: on an f32 corpus the f32 chain; on a bf16 corpus the row is
 * widened exactly and the vector is rounded to bf16 the way that corpus's scorer rounds it.  The list of cluster c is its
 * members in descending order of oi_rank_key(s, doc) -- score descending with -0 and +0 as one key, ties to the smaller doc id:
 * the order of every ranked list of the library -- cut at `top`.  docs_out holds GLOBAL doc ids (doc_id_base + local row),
 * counts_out[c] the number of valid entries; entries beyond it are score 0 and doc 0xFFFFFFFF.  An empty cluster has count 0.
 *
 * The result is a function of the inputs alone: it does not depend on the grid, the order of any atomics, the cosine mode, the
 * screening-copy policy or the run, and ties at the cut are resolved by the rule above, not by arrival.  The score of an entry
 * is bit for bit the sim oi_similar_share compared against the threshold for that pair (a -0 is returned as +0, as by every
 * ranked list).  The lists are valid input of oi_collapse_lists (row stride `top`) -- retweets are what fills the top of a
 * narrative -- and of oi_merge_lists: document shards hold disjoint rows, so a sharded host calls per rank and merges.
 *
 * Rules.  Embeddings only (otherwise OI_ERR_STATE): no signals, no forward index, no finalize; attributes only when a filter
 * is given (otherwise OI_ERR_STATE); it works on a view, on an f32 corpus of any supported dim and on a bf16 corpus.
 * n_clusters in [1, OI_MAX_CENTROIDS]; top in [1, OI_MAX_DEPTH]; reserved == 0.  location covers labels, centroids and the
 * three outputs; spec and filter are host pointers, read before the call returns.  With OI_DEVICE the call is asynchronous on
 * the ctx stream, with no host synchronise anywhere in it.  Not captured by graph replay.  A null index, spec or buffer, top or
 * n_clusters out of range, reserved != 0, a bad location -> OI_ERR_INVALID_ARG with the offending number in the message; every
 * argument check precedes the first device call.
 * Workspace per searching context (oi_workspace_bytes counts it): "exemplars" holds one 4-byte score key per local row, the
 * select's histograms (1 KB per cluster) and states, 8 B x top x n_clusters of list slots and, for a bf16 corpus, the rounded
 * centroids.  With OI_HOST the staged labels, centroids and outputs are held in "exemplars_io".
 * Profile tags: "exemplar_score" (the stream of the member rows), "exemplar_select" (the segmented radix select: at most
 * 4 + ceil(log256 n_docs) passes of 8 B per row), "exemplar_emit" (collect, sort, write).
 *
 * NOT covered: a screened route over the bf16 copy (every member row is read in full); a time axis (one list per cluster and
 * bucket); oi_search_sharded* / oi_pipeline_* forms (a sharded host merges per-rank lists with oi_merge_lists); more than
 * OI_MAX_DEPTH posts per cluster.
 */
typedef struct oi_exemplar_spec { uint32_t top, reserved[3]; } oi_exemplar_spec;   /* top in 1 .. OI_MAX_DEPTH; reserved == 0 */
int oi_label_exemplars(oi_index *idx, const uint32_t *labels /* [n_docs] by LOCAL row */,
                       const float *centroids /* [n_clusters][dim] */, uint32_t n_clusters,
                       const oi_exemplar_spec *spec, const oi_doc_filter *filter /* ONE, host pointer, or NULL */,
                       int location,
                       float *scores_out /* [n_clusters][top] */, uint32_t *docs_out /* [n_clusters][top] */,
                       uint32_t *counts_out /* [n_clusters] */);

/* ------------------------------------------------------------------------- */
/* Narrative breakdown: per-cluster records by time bucket or ticker           */
/* ------------------------------------------------------------------------- */
/*
 * oi_narratives_fit says which narratives there are, oi_label_terms what each is about, oi_label_exemplars which posts to
 * quote; this call answers the two questions the reference's own reports are built around (social_summary per ticker,
 * run_compare across tickers) for a NARRATIVE: how did each cluster develop over time (OI_LABEL_AXIS_TIME), and which tickers
 * is it about and how do its posts feel per ticker (OI_LABEL_AXIS_KEY)?  It is the member of the summing tallies that decides
 * a document by a LABEL: oi_similar_summary / _groups decide it by similarity, oi_mention_summary by terms.  It reads the
 * labels where they are, 4 bytes per row, and the attributes and signals of the labelled rows: no embeddings, no corpus stream,
 * and nothing per post returns to the host.  Builder-defined like the whole retrieval path.
 *
 * The definition.  labels[d] is a u32 per LOCAL row.  Row d is in cell (c, x) when
 *   labels[d] == c < n_clusters   (any other label, 0xFFFFFFFF included, is "no cluster", as in oi_label_sums: it is no error,
 *                                  and the row's attributes and signals are not read), and
 *   d passes `filter`, when one is given, and
 *   on the TIME axis oi_similar_summary's clause 2 gives x: bucket_width == 0 (one cell, x = 0), or stamp_origin <= stamp[d]
 *     and (stamp[d] - stamp_origin) / bucket_width == x < n_cells;
 *   on the KEY axis oi_similar_groups's key clause gives x: (group[d] & key_mask) >> ctz(key_mask) == x, and a key >= n_cells
 *     belongs to no cell.
 * The record of a cell is oi_similar_summary's, word for word: total, by_source[2], bullish, bearish, neutral and spec_count
 * are exact integers, and polarity_sum = (double)(sum of pol_q30) * 2^-30, the sum taken in 64-bit integers.
 *
 * The contract that follows from it:
 *   - the result is a function of the inputs alone: grid, route, order of atomics and run do not matter;
 *   - records of document shards add;
 *   - with no filter, the sum over x of total[c][x] on a one-cell TIME axis equals oi_label_sums' counts[c];
 *   - with labels_out of an oi_similar_share or oi_narratives_fit call, and that call's time axis and filter used for every
 *     query, the dense TIME records equal that call's out bit for bit;
 *   - summed over the keys, a KEY-axis call equals the one-cell TIME call when every document has a key.
 *
 * Dense output (top == 0): records_out[c][x], row stride n_cells; keys_out, counts_out and qualified_out may be NULL and are
 * not written.  Ranked output (top >= 1, KEY axis only) is exactly oi_similar_groups' ranked output with "query" replaced by
 * "cluster": the keys of cluster c with total >= max(min_total, 1) are ordered by the rank key v << 32 | ~key descending (v =
 * the record's total / spec_count / bullish / bearish as rank_by says; ties go to the smaller key) and cut at `top`;
 * records_out and keys_out have row stride `top`; counts_out[c] is the number of listed keys; entries beyond it are key
 * 0xFFFFFFFF and an all-zero record; qualified_out[c], when given, is the number of keys that met the bar before the cut.
 *
 * Rules.  Signals are required (oi_index_set_signals): otherwise OI_ERR_STATE.  Doc attributes are required on the KEY axis,
 * with bucket_width > 0, or with a filter: otherwise OI_ERR_STATE.  NO embeddings, forward index or finalize are needed, and
 * it works on a view.  n_clusters in [1, OI_MAX_CENTROIDS]; n_clusters * n_cells <= OI_MAX_GROUP_CELLS.  spec and filter are
 * host pointers, read before the call returns; location covers the labels and the four outputs.  With OI_DEVICE the call is
 * asynchronous on the ctx stream, with no host synchronise anywhere in it.  Not captured by graph replay.  A null index, spec
 * or required buffer, a bad axis, n_clusters, n_cells or the cell count out of range, top > 0 on the TIME axis, top >
 * OI_MAX_DEPTH, rank_by out of range or non-zero with top == 0, reserved != 0, bucket_width != 0 on the KEY axis, a key_mask
 * that is zero or not one contiguous run of bits, a bad location -> OI_ERR_INVALID_ARG with the offending number in the
 * message; every argument check precedes the first device call.
 * Workspace per searching context (oi_workspace_bytes counts it): "label_summary" holds 64 B per cell and, for ranked output,
 * 8 B more per cell; with OI_HOST the staged labels and outputs are held in "label_summary_io".
 * Profile tags: "label_summary" (the pass over labels, attributes and signals) and "label_summary_rank" (the ranked finish).
 *
 * NOT covered: oi_search_sharded* / oi_pipeline_* forms (a sharded host adds the dense records of its ranks); both axes at
 * once (one record per cluster, bucket and key).
 */
enum { OI_LABEL_AXIS_TIME = 0, OI_LABEL_AXIS_KEY = 1 };
typedef struct oi_label_summary_spec {
    uint32_t axis;          /* OI_LABEL_AXIS_* */
    uint32_t stamp_origin;  /* TIME: oi_summary_spec's meaning.              KEY: key_mask (non-zero, one contiguous run of bits) */
    uint32_t bucket_width;  /* TIME: oi_summary_spec's (0: no axis, 1 cell).  KEY: must be 0 */
    uint32_t n_cells;       /* TIME: 1 .. OI_MAX_VOLUME_BUCKETS (1 when bucket_width == 0).  KEY: 1 .. min(2^popcount(mask), OI_MAX_GROUP_KEYS) */
    uint32_t top;           /* 0: dense output;  1 .. OI_MAX_DEPTH: ranked output, KEY axis only */
    uint32_t rank_by;       /* OI_GROUP_RANK_*; must be 0 when top == 0 */
    uint32_t min_total;     /* ranked output lists a key only when its total >= max(min_total, 1) */
    uint32_t reserved;      /* 0 */
} oi_label_summary_spec;    /* 32 bytes */
int oi_label_summary(oi_index *idx, const uint32_t *labels /* [n_docs] by LOCAL row */, uint32_t n_clusters,
                     const oi_label_summary_spec *spec, const oi_doc_filter *filter /* ONE, host pointer, or NULL */,
                     int location,
                     oi_social_counters *records_out /* [n_clusters][n_cells], or [n_clusters][top] */,
                     uint32_t *keys_out /* [n_clusters][top] */, uint32_t *counts_out /* [n_clusters] */,
                     uint32_t *qualified_out /* [n_clusters], may be NULL */);

/* ------------------------------------------------------------------------- */
/* Text to term ids: the tokeniser and the hashed vocabulary                   */
/* ------------------------------------------------------------------------- */
/*
 * What connects post TEXT to the u32 term ids of oi_index_set_forward and of every oi_search* call.
 *
 * TOKENS of a text are the reference's (src/adapters/analyzer/lexicon.rs:54-58): Unicode lowercase, then the maximal runs
 * of ASCII [0-9a-z].  At byte level: A-Z -> a-z; U+212A (E2 84 AA) -> 'k', joining the token around it; U+0130 (C4 B0) ->
 * 'i' followed by a separator; every other byte >= 0x80 separates.  A text boundary always cuts a token ("abc" | "def" in
 * adjacent texts are two tokens).  The input is valid UTF-8, as for oi_lexicon_analyze.
 *
 * TERM ID of a token whose lowercased bytes are b[0..len) -- the hashing trick, no dictionary to build, ship or all-reduce;
 * a document and a query, and two ranks of a sharded index, agree by construction:
 *     h = 0xcbf29ce484222325;  for i < min(len, OI_TEXT_TOKEN_HASH_BYTES):  h = (h ^ b[i]) * 0x100000001b3    (FNV-1a, mod 2^64)
 *     h ^= h >> 33;  h *= 0xff51afd7ed558ccd;  h ^= h >> 33;  h *= 0xc4ceb9fe1a85ec53;  h ^= h >> 33           (fmix64)
 *     term = (uint32_t)(((h >> 32) * (uint64_t)vocab) >> 32)
 * A token longer than OI_TEXT_TOKEN_HASH_BYTES lowercased bytes hashes by its first 64; it is still ONE token and ends
 * where its run ends.  Collisions merge terms (not an error): about T^2 / 2V colliding pairs for T distinct tokens in a
 * vocabulary of V.  Term ids come out in text order, duplicates kept (a forward index wants tf; a repeated query term
 * counts each time).  The output is a pure function of the input.
 *
 * oi_text_terms: text i = blob[offsets[i] .. offsets[i+1]) (n_texts + 1 offsets, offsets[0] == 0, offsets[n_texts] ==
 *   blob_bytes) -- the buffers of oi_lexicon_analyze[_device], so one blob in HBM serves the analyzer and the index.
 *   Text i's ids are term_ids_out[text_offsets_out[i] .. text_offsets_out[i+1]); *total_out_host (may be NULL) = their
 *   number.  term_ids_out == NULL: count only (offsets and total), so a caller sizes its buffer with one call and fills it
 *   with the next.  Otherwise total > term_capacity -> OI_ERR_OVERFLOW, nothing written past the capacity (the ctx stays
 *   usable); (blob_bytes + 1) / 2 is always enough.  location says where EVERY buffer but total_out_host lives.
 *   OI_DEVICE: asynchronous on the ctx stream when total_out_host == NULL and term_capacity >= (blob_bytes + 1) / 2 (or
 *   count only); otherwise the call synchronises the stream once (the total comes back).  OI_HOST: synchronous.
 * oi_query_terms: the same over a batch of query texts with u32 offsets: its outputs are exactly the `query_terms` /
 *   `q_term_offsets` pair of the oi_search* calls (which are unchanged: a host tokenises, then searches).
 * oi_index_set_text: tokenise with the index's own vocab straight into the forward index and stage it -- bit for bit what
 *   oi_text_terms followed by oi_index_set_forward gives, without the caller ever holding the ids.  offsets: n_docs + 1.
 *   State rules of oi_index_set_forward (a view: OI_ERR_STATE; at most 2^32 - 2 tokens per shard).
 * All three with OI_DEVICE: the offsets cannot be checked by the library.  They must be non-decreasing, start at 0 and end at
 * blob_bytes; otherwise the output offsets (and with them the index oi_index_set_text stages) are unspecified -- the
 * call still writes nothing outside the buffers it was given.
 */
#define OI_TEXT_TOKEN_HASH_BYTES 64u
int oi_text_terms(oi_ctx *ctx, const uint8_t *blob, const uint64_t *offsets, uint64_t n_texts, uint64_t blob_bytes,
                  uint32_t vocab, int location, uint32_t *term_ids_out, uint64_t term_capacity,
                  uint64_t *text_offsets_out, uint64_t *total_out_host);
int oi_query_terms(oi_ctx *ctx, const uint8_t *blob, const uint32_t *offsets, uint32_t n_queries, uint32_t blob_bytes,
                   uint32_t vocab, int location, uint32_t *query_terms_out, uint64_t term_capacity,
                   uint32_t *q_term_offsets_out, uint64_t *total_out_host);
int oi_index_set_text(oi_index *idx, const uint8_t *blob, const uint64_t *offsets, uint64_t blob_bytes, int location);

/* ------------------------------------------------------------------------- */
/* The pipelined query behind the C ABI: several batches in flight             */
/* ------------------------------------------------------------------------- */
/*
 * Throughput mode of oi_search / oi_search_sharded for a host without streams or a collective library of its own (the
 * reference's port is one synchronous call -- src/domain/ports/post_analyzer.rs:7-11, `Send + Sync`, borrowed in / owned
 * out; composition root src/main.rs:17-39 -- so this has no reference counterpart).  Batches are independent: batch n is
 * scored on lane n % lanes (every lane = a context, a stream and a view of the index inside the library), its exchange
 * (ONE RCCL all-gather when `comm` is given, none otherwise) and its fusion run on a further stream, and the next batch's
 * corpus stream overlaps the selects / rescoring / fusion of the previous one.  Per batch: the same kernels on the same
 * data as oi_search (comm == NULL) / oi_search_sharded -- bit-identical results (tests/test_gpu_pipeline.py).
 *
 *   oi_pipeline_create(idx, comm_or_NULL, lanes, max_queries, max_query_terms, depth, k, &p)
 *        idx finalized, not a view; lanes in [1,4] (2 is the measured optimum on one MI355X); every later batch has at most
 *        max_queries queries of at most max_query_terms terms each (sizes of the staging buffers).  HBM: one set of search
 *        workspaces per lane (oi_pipeline_workspace_bytes).
 *   oi_pipeline_submit(p, queries..., n_queries, location, scores_out, docs_out, counts_out, &ticket)
 *        asynchronous in BOTH locations; tickets count from 1.
 *        OI_DEVICE: inputs were produced on the index's context stream (oi_set_stream) and must stay unmodified until the
 *                   batch is waited for; outputs (n_queries x k, k as created) are written by the pipeline's streams.
 *        OI_HOST:   inputs are copied during the call (reusable at return); the host output arrays are filled by
 *                   oi_pipeline_wait(ticket) -- or, if nobody waits, when the slot is reused 2 x lanes (>= 4) submits later
 *                   or at drain -- and must stay valid until then.
 *   oi_pipeline_wait(p, ticket, host_sync)
 *        host_sync != 0: returns when that batch's outputs are complete (host outputs delivered).
 *        host_sync == 0 (OI_DEVICE batches): no host stall -- orders the index's context stream after the batch, so work
 *                   queued there afterwards may read the outputs.
 *   oi_pipeline_drain(p)      everything submitted is complete; a candidate-pool overflow in any lane is reported here.
 *   oi_pipeline_destroy(p)    drains, then frees the lanes (before the index and the communicator).
 * With a communicator every rank must submit the same batches in the same order from ONE host thread (the collectives
 * are issued in submission order on one stream), as with oi_search_sharded.  One submitting thread per pipeline; wait /
 * drain may be called from another.
 */
typedef struct oi_pipeline oi_pipeline;
int oi_pipeline_create(oi_index *idx, oi_comm *comm, uint32_t lanes, uint32_t max_queries, uint32_t max_query_terms,
                       uint32_t depth, uint32_t k, oi_pipeline **out);
void oi_pipeline_destroy(oi_pipeline *p);
int oi_pipeline_submit(oi_pipeline *p, const float *query_vecs, const uint32_t *query_terms, const uint32_t *q_term_offsets,
                       uint32_t n_queries, int location, float *scores_out, uint32_t *docs_out, uint32_t *counts_out,
                       uint64_t *ticket_out);
int oi_pipeline_wait(oi_pipeline *p, uint64_t ticket, int host_sync);
int oi_pipeline_drain(oi_pipeline *p);
int oi_pipeline_workspace_bytes(oi_pipeline *p, uint64_t *device_bytes_out, uint64_t *pinned_host_bytes_out);
/* oi_profile_reset / oi_profile_read (below) over the pipeline's lanes, summed (the lanes' contexts are the library's own).
 * Two lanes' launches overlap in time: the summed durations then exceed the wall time they covered. */
/* oi_pipeline_create MEASURES which of its streams run at the same time (HIP maps streams onto a few hardware queues, and
 * which queue a new stream gets depends on every stream the process already has: two lanes on one queue serialise) and
 * keeps lanes + 1 that do, drawing up to 12 candidates.  This reports how many of the lanes + 1 were pairwise concurrent. */
int oi_pipeline_concurrent_streams(oi_pipeline *p, uint32_t *concurrent_out, uint32_t *streams_out);
int oi_pipeline_profile_reset(oi_pipeline *p, int enable);
int oi_pipeline_profile_read(oi_pipeline *p, const char *kernel_tag, double *total_ms_out, uint64_t *launches_out);

/* Diagnostics of the OI_COSINE_SCREEN mode (tests/test_gpu_prefilter.py; not on the query path).  For host
 * queries [n_queries][dim] against rows [row_begin, row_begin + n_rows) of an f32 index:
 *   screen_scores_out[q * n_rows + r]  the screen's raw score s~ (bf16 operands, the screen's own conversion and
 *                                      matrix instruction);  NULL = skip
 *   eps_out[q]                         the proven bound of that query: |s~ - s| <= eps for EVERY row of the index
 *                                      (infinite when the query has no bound and takes the exact kernel)
 * Both outputs are host buffers; the call is synchronous. */
int oi_screen_probe(oi_index *idx, const float *query_vecs, uint32_t n_queries, uint64_t row_begin,
                    uint32_t n_rows, float *screen_scores_out, float *eps_out);

/* Timing hooks for bench.py: when enabled, HIP events are recorded on the ctx stream
 * around every kernel launch, grouped by tag ("cosine", "bm25", "select", "rrf",
 * "lexicon", "social_summary", "text_count", "text_emit", "groups", "groups_band", "groups_exact", "groups_rank",
 * "volume", "volume_band", "volume_exact",
 * "summary", "summary_band", "summary_exact").  oi_profile_read returns the summed duration (ms) of
 * the launches with that tag and their count since the last reset.  enable: 0 off, 1 every
 * tagged launch, 2 only the "cosine" launches (two event packets per launch cost a few us of
 * stream time each: a timed region that only needs its dominant kernel asks for 2).
 * The screened cosine route also tags "cosine_gated", "rescreen", "rescore" and "spec".  "spec" COUNTS the speculative
 * thresholds computed in a search, one span per prediction; the prediction is computed inside the preceding margin select,
 * whose time is under "select", so the span is empty and its duration reads ~0.
 * The list of tags ends with those of oi_similar_share: "share", "share_band", "share_exact". */
int oi_profile_reset(oi_ctx *ctx, int enable);
int oi_profile_read(oi_ctx *ctx, const char *kernel_tag, double *total_ms_out, uint64_t *launches_out);

/* Memory this context holds right now: HBM of its workspaces (candidate pools, staging, lists -- INTEGRATION.md 5b: the
 * BM25 pool of the wave kernel alone reserves ~5 GB per searching context at 10M docs) and page-locked host memory of
 * its staging buffers.  Index buffers are not counted (oi_index owns them; a view borrows them).  Either output may be
 * NULL.  (No reference counterpart: the reference allocates nothing on a device.) */
int oi_workspace_bytes(oi_ctx *ctx, uint64_t *device_bytes_out, uint64_t *pinned_host_bytes_out);

#ifdef __cplusplus
}
#endif
#endif /* OPENINTEL_HIP_H */
