//! Raw bindings, one-to-one with include/openintel_hip.h (ABI version 1).
//! tests/test_rust_shim_sources.py keeps this list and the header in step.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)]
pub struct OiCtx {
    _p: [u8; 0],
}
#[repr(C)]
pub struct OiIndex {
    _p: [u8; 0],
}
#[repr(C)]
pub struct OiPipeline {
    _p: [u8; 0],
}
#[repr(C)]
pub struct OiComm {
    _p: [u8; 0],
}
pub const OI_COMM_ID_BYTES: usize = 128;

/// `oi_social_counters`: the raw sums of SpeculationEngine::social_summary (speculation_engine.rs:76-97).
#[repr(C)]
#[derive(Default, Debug, Clone, Copy)]
pub struct OiSocialCounters {
    pub total: u64,
    pub by_source: [u64; 2], // [reddit, bluesky]  source_kind.rs:5-8
    pub bullish: u64,
    pub bearish: u64,
    pub neutral: u64,
    pub spec_count: u64,
    pub polarity_sum: f64,
}

/// `oi_doc_filter`: document d passes when (group[d] & group_mask) == group_value && stamp_lo <= stamp[d] <= stamp_hi.
/// `{0, 0, 0, u32::MAX}` passes every document.
#[repr(C)]
#[derive(Debug, Clone, Copy, PartialEq, Eq)]
pub struct OiDocFilter {
    pub group_mask: u32,
    pub group_value: u32,
    pub stamp_lo: u32,
    pub stamp_hi: u32,
}

/// `oi_volume_spec`: count documents with sim >= threshold per bucket (stamp - stamp_origin) / bucket_width;
/// bucket_width == 0 means no time axis (n_buckets must be 1).
#[repr(C)]
#[derive(Debug, Clone, Copy, PartialEq)]
pub struct OiVolumeSpec {
    pub threshold: f32,
    pub stamp_origin: u32,
    pub bucket_width: u32,
    pub n_buckets: u32,
}
pub const OI_MAX_VOLUME_BUCKETS: u32 = 1024;

/// `oi_summary_spec`: `oi_volume_spec`'s time axis; `threshold` is every query's unless the call is given a thresholds array.
#[repr(C)]
#[derive(Debug, Clone, Copy, PartialEq)]
pub struct OiSummarySpec {
    pub threshold: f32,
    pub stamp_origin: u32,
    pub bucket_width: u32,
    pub n_buckets: u32,
}
pub const OI_MAX_SUMMARY_CELLS: u32 = 1 << 18;

/// `oi_narrative_spec`: `oi_summary_spec`'s four fields (one threshold for all clusters), then max_iters (1 ..= 64).
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct OiNarrativeSpec {
    pub threshold: f32,
    pub stamp_origin: u32,
    pub bucket_width: u32,
    pub n_buckets: u32,
    pub max_iters: u32,
}
/// `oi_narrative_info`: assignment steps run, converged (0 / 1), rows moved in the last step, rows it assigned.
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct OiNarrativeInfo {
    pub iterations: u32,
    pub converged: u32,
    pub moved: u64,
    pub assigned: u64,
}
pub const OI_MAX_CENTROIDS: u32 = 256;

/// `oi_label_terms_spec`: records per cluster (1 ..= 64), the smallest df_cluster of an eligible term (0 means 1), reserved (0).
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct OiLabelTermsSpec {
    pub top: u32,
    pub min_df: u32,
    pub reserved: [u32; 2],
}
/// `oi_label_term`: one distinguishing term of a cluster -- the term id (`u32::MAX`: no entry), the cluster's documents that hold
/// it, the assigned documents that hold it, reserved (0), excess = df_cluster * A - sizes[c] * df_assigned.  24 bytes.
#[repr(C)]
#[derive(Debug, Clone, Copy, Default, PartialEq)]
pub struct OiLabelTerm {
    pub term: u32,
    pub df_cluster: u32,
    pub df_assigned: u32,
    pub reserved: u32,
    pub excess: i64,
}
pub const OI_MAX_LABEL_TERMS: u32 = 64;
pub const OI_MAX_LABEL_TERM_CELLS: u32 = 1 << 28;

/// `oi_exemplar_spec`: posts per cluster (1 ..= `OI_MAX_DEPTH`), reserved (0).  16 bytes.
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct OiExemplarSpec {
    pub top: u32,
    pub reserved: [u32; 3],
}

/// `oi_seed_spec`: method (`OI_SEED_*`), trials (candidates per seed, 1 ..= 8; 1 with farthest-first), the RNG seed,
/// `oi_narrative_spec`'s time axis, reserved (0).  32 bytes.
#[repr(C)]
#[derive(Debug, Clone, Copy)]
pub struct OiSeedSpec {
    pub method: u32,
    pub trials: u32,
    pub seed: u64,
    pub stamp_origin: u32,
    pub bucket_width: u32,
    pub n_buckets: u32,
    pub reserved: u32,
}
/// `oi_seed_info`: seeds found, reserved, eligible rows, the sum of the weights after the last seed.  24 bytes.
#[repr(C)]
#[derive(Debug, Clone, Copy, Default)]
pub struct OiSeedInfo {
    pub found: u32,
    pub reserved: u32,
    pub eligible: u64,
    pub potential: u64,
}
pub const OI_SEED_KMEANSPP: u32 = 0;
pub const OI_SEED_FARTHEST: u32 = 1;
pub const OI_MAX_SEED_TRIALS: u32 = 8;

/// `oi_mention_spec`: axis TIME -- `stamp_origin`, `bucket_width` and `n_cells` are `oi_summary_spec`'s time axis; axis KEY --
/// `stamp_origin` carries the key_mask (non-zero, one contiguous run of bits), `bucket_width` is 0, `n_cells` the number of keys.
#[repr(C)]
#[derive(Debug, Clone, Copy, PartialEq)]
pub struct OiMentionSpec {
    pub axis: u32,
    pub stamp_origin: u32,
    pub bucket_width: u32,
    pub n_cells: u32,
}
pub const OI_MAX_MENTION_TERMS: u32 = 64;
pub const OI_MENTION_AXIS_TIME: u32 = 0;
pub const OI_MENTION_AXIS_KEY: u32 = 1;

/// `oi_label_summary_spec`: axis TIME -- `stamp_origin`, `bucket_width` and `n_cells` are `oi_summary_spec`'s time axis and `top`
/// is 0; axis KEY -- `stamp_origin` carries the key_mask, `bucket_width` is 0, `n_cells` the number of keys, and `top` >= 1 asks
/// for the best `top` keys by `rank_by` among those with total >= max(min_total, 1).  `reserved` is 0.  32 bytes.
#[repr(C)]
#[derive(Debug, Clone, Copy, PartialEq)]
pub struct OiLabelSummarySpec {
    pub axis: u32,
    pub stamp_origin: u32,
    pub bucket_width: u32,
    pub n_cells: u32,
    pub top: u32,
    pub rank_by: u32,
    pub min_total: u32,
    pub reserved: u32,
}
pub const OI_LABEL_AXIS_TIME: u32 = 0;
pub const OI_LABEL_AXIS_KEY: u32 = 1;

/// `oi_groups_spec`: the key of a document is (group & key_mask) >> ctz(key_mask); top == 0 asks for dense records, top >= 1 for
/// the best `top` keys by `rank_by` among those with total >= max(min_total, 1).
#[repr(C)]
#[derive(Debug, Clone, Copy, PartialEq)]
pub struct OiGroupsSpec {
    pub threshold: f32,
    pub key_mask: u32,
    pub n_keys: u32,
    pub top: u32,
    pub rank_by: u32,
    pub min_total: u32,
}
pub const OI_MAX_GROUP_KEYS: u32 = 65536;
pub const OI_MAX_GROUP_CELLS: u32 = 1 << 20;
pub const OI_GROUP_RANK_TOTAL: u32 = 0;
pub const OI_GROUP_RANK_SPEC: u32 = 1;
pub const OI_GROUP_RANK_BULLISH: u32 = 2;
pub const OI_GROUP_RANK_BEARISH: u32 = 3;

pub const OI_OK: c_int = 0;
pub const OI_ERR_ANALYZER_MISMATCH: c_int = -3;
pub const OI_ERR_OVERFLOW: c_int = -8;
pub const OI_ERR_COMM: c_int = -9;
pub const OI_HOST: c_int = 0;
pub const OI_DEVICE: c_int = 1;
pub const OI_COSINE_EXACT: c_int = 0;
pub const OI_COSINE_SPLIT: c_int = 1;
pub const OI_COSINE_SCREEN: c_int = 2;
pub const OI_COSINE_SCREEN_COPY: c_int = 3;
pub const OI_COSINE_SCREEN_STREAM: c_int = 4;
pub const OI_SCREEN_COPY_AUTO: c_int = 0;
pub const OI_SCREEN_COPY_NEVER: c_int = 1;
pub const OI_SCREEN_COPY_ALWAYS: c_int = 2;

extern "C" {
    pub fn oi_abi_version() -> c_int;
    pub fn oi_last_error() -> *const c_char; // thread-local
    pub fn oi_create(device_ordinal: c_int, out: *mut *mut OiCtx) -> c_int;
    pub fn oi_create_like(like: *mut OiCtx, out: *mut *mut OiCtx) -> c_int;
    pub fn oi_destroy(ctx: *mut OiCtx);
    pub fn oi_workspace_bytes(ctx: *mut OiCtx, device_bytes_out: *mut u64, pinned_host_bytes_out: *mut u64) -> c_int;
    pub fn oi_set_stream(ctx: *mut OiCtx, hip_stream: *mut c_void) -> c_int;
    pub fn oi_synchronize(ctx: *mut OiCtx) -> c_int;
    pub fn oi_set_cosine_mode(ctx: *mut OiCtx, mode: c_int) -> c_int;
    pub fn oi_set_overlap(ctx: *mut OiCtx, enable: c_int) -> c_int;
    pub fn oi_set_screen_speculation(ctx: *mut OiCtx, enable: c_int) -> c_int;
    pub fn oi_set_graph_replay(ctx: *mut OiCtx, enable: c_int) -> c_int;

    pub fn oi_lexicon_analyze(ctx: *mut OiCtx, text_blob: *const u8, offsets: *const u64, n_posts: u64,
                              polarity_out: *mut f64, speculative_out: *mut u8) -> c_int;
    pub fn oi_lexicon_analyze_device(ctx: *mut OiCtx, d_text_blob: *const u8, d_offsets: *const u64, n_posts: u64,
                                     blob_bytes: u64, d_polarity_out: *mut f64, d_speculative_out: *mut u8) -> c_int;
    pub fn oi_social_summary(ctx: *mut OiCtx, sources: *const u8, n_posts: u64, polarity: *const f64,
                             speculative: *const u8, n_signals: u64, bull_bear_threshold: f64, location: c_int,
                             out_host: *mut OiSocialCounters) -> c_int;
    pub fn oi_lexicon_summary_device(ctx: *mut OiCtx, d_text_blob: *const u8, d_offsets: *const u64, n_posts: u64,
                                     blob_bytes: u64, d_sources: *const u8, bull_bear_threshold: f64,
                                     d_polarity_out: *mut f64, d_speculative_out: *mut u8,
                                     out_host: *mut OiSocialCounters) -> c_int;

    pub fn oi_social_summary_segmented(ctx: *mut OiCtx, sources: *const u8, polarity: *const f64, speculative: *const u8,
                                       n_posts: u64, seg_offsets: *const u64, n_segments: u64, bull_bear_threshold: f64,
                                       location: c_int, out: *mut OiSocialCounters) -> c_int;
    pub fn oi_lexicon_scan_segments_device(ctx: *mut OiCtx, d_text_blob: *const u8, d_offsets: *const u64, n_posts: u64,
                                           blob_bytes: u64, d_sources: *const u8, d_seg_offsets: *const u64,
                                           n_segments: u64, bull_bear_threshold: f64, d_polarity_out: *mut f64,
                                           d_speculative_out: *mut u8, d_out: *mut OiSocialCounters) -> c_int;

    pub fn oi_catalyst_keyword(index: u32) -> *const c_char;
    pub fn oi_headline_scan(ctx: *mut OiCtx, blob: *const u8, offsets: *const u64, n_titles: u64, ticker: *const u8,
                            ticker_len: u64, forms_blob: *const u8, form_offsets: *const u32, n_forms: u32,
                            mask_out: *mut u16, order_out: *mut u64, about_out: *mut u8) -> c_int;
    pub fn oi_headline_scan_rows(ctx: *mut OiCtx, blob: *const u8, offsets: *const u64, n_titles: u64,
                                 row_offsets: *const u64, n_rows: u32, tickers_blob: *const u8,
                                 ticker_offsets: *const u32, forms_blob: *const u8, form_offsets: *const u32,
                                 row_form_offsets: *const u32, mask_out: *mut u16, order_out: *mut u64,
                                 about_out: *mut u8) -> c_int;
    pub fn oi_headline_scan_device(ctx: *mut OiCtx, d_blob: *const u8, d_offsets: *const u64, n_titles: u64,
                                   blob_bytes: u64, ticker: *const u8, ticker_len: u64, forms_blob: *const u8,
                                   form_offsets: *const u32, n_forms: u32, d_mask_out: *mut u16,
                                   d_order_out: *mut u64, d_about_out: *mut u8) -> c_int;

    pub fn oi_index_create(ctx: *mut OiCtx, n_docs: u64, dim: u32, vocab: u32, doc_id_base: u32,
                           out: *mut *mut OiIndex) -> c_int;
    pub fn oi_index_destroy(idx: *mut OiIndex);
    pub fn oi_index_view(src: *mut OiIndex, ctx: *mut OiCtx, out: *mut *mut OiIndex) -> c_int;
    pub fn oi_index_set_embeddings(idx: *mut OiIndex, rows: *mut f32, location: c_int, normalize: c_int) -> c_int;
    pub fn oi_index_set_embeddings_bf16(idx: *mut OiIndex, rows: *const u16, location: c_int) -> c_int;
    pub fn oi_index_set_forward(idx: *mut OiIndex, term_ids: *const u32, doc_offsets: *const u64, location: c_int) -> c_int;
    pub fn oi_index_local_stats(idx: *mut OiIndex, total_tokens_out: *mut u64, df_out_host: *mut u32) -> c_int;
    pub fn oi_index_finalize(idx: *mut OiIndex, global_n_docs: u64, global_total_tokens: u64,
                             global_df_host: *const u32) -> c_int;
    pub fn oi_index_long_rows(idx: *mut OiIndex, n_out: *mut u32) -> c_int;
    pub fn oi_index_set_screen_copy(idx: *mut OiIndex, policy: c_int) -> c_int;
    pub fn oi_index_bytes(idx: *mut OiIndex, rows_owned_bytes_out: *mut u64, screen_copy_bytes_out: *mut u64,
                          bm25_bytes_out: *mut u64) -> c_int;
    pub fn oi_index_set_bm25_mode(idx: *mut OiIndex, mode: c_int) -> c_int;
    pub fn oi_index_set_max_query_terms(idx: *mut OiIndex, max_terms: u32) -> c_int;

    pub fn oi_search_lists(idx: *mut OiIndex, query_vecs: *const f32, query_terms: *const u32,
                           q_term_offsets: *const u32, n_queries: u32, depth: u32, location: c_int,
                           cos_scores: *mut f32, cos_docs: *mut u32, cos_counts: *mut u32, bm25_scores: *mut f32,
                           bm25_docs: *mut u32, bm25_counts: *mut u32) -> c_int;
    pub fn oi_merge_lists(ctx: *mut OiCtx, scores: *const f32, docs: *const u32, counts: *const u32, n_shards: u32,
                          n_queries: u32, depth: u32, location: c_int, scores_out: *mut f32, docs_out: *mut u32,
                          counts_out: *mut u32) -> c_int;
    pub fn oi_search_lists_packed(idx: *mut OiIndex, query_vecs: *const f32, query_terms: *const u32,
                                  q_term_offsets: *const u32, n_queries: u32, depth: u32, location: c_int,
                                  packed_out: *mut u32) -> c_int;
    pub fn oi_fuse_packed(ctx: *mut OiCtx, packed_all: *const u32, n_shards: u32, n_queries: u32, depth: u32, k: u32,
                          location: c_int, scores_out: *mut f32, docs_out: *mut u32, counts_out: *mut u32) -> c_int;
    pub fn oi_rrf_fuse(ctx: *mut OiCtx, docs_a: *const u32, counts_a: *const u32, docs_b: *const u32,
                       counts_b: *const u32, n_queries: u32, depth: u32, k: u32, location: c_int,
                       scores_out: *mut f32, docs_out: *mut u32, counts_out: *mut u32) -> c_int;
    pub fn oi_search(idx: *mut OiIndex, query_vecs: *const f32, query_terms: *const u32, q_term_offsets: *const u32,
                     n_queries: u32, depth: u32, k: u32, location: c_int, scores_out: *mut f32, docs_out: *mut u32,
                     counts_out: *mut u32) -> c_int;

    // the row-sharded query with RCCL inside the library (one process per GPU)
    pub fn oi_comm_unique_id(id_out: *mut u8) -> c_int;
    pub fn oi_comm_create(ctx: *mut OiCtx, id: *const u8, rank: u32, world: u32, out: *mut *mut OiComm) -> c_int;
    pub fn oi_comm_destroy(comm: *mut OiComm);
    pub fn oi_index_finalize_sharded(idx: *mut OiIndex, comm: *mut OiComm) -> c_int;
    pub fn oi_search_sharded(idx: *mut OiIndex, comm: *mut OiComm, query_vecs: *const f32, query_terms: *const u32,
                             q_term_offsets: *const u32, n_queries: u32, depth: u32, k: u32, location: c_int,
                             scores_out: *mut f32, docs_out: *mut u32, counts_out: *mut u32) -> c_int;

    // text -> term ids (the reference's tokens hashed onto [0, vocab); offsets[0] == 0, offsets[n] == blob_bytes)
    pub fn oi_text_terms(ctx: *mut OiCtx, blob: *const u8, offsets: *const u64, n_texts: u64, blob_bytes: u64, vocab: u32,
                         location: c_int, term_ids_out: *mut u32, term_capacity: u64, text_offsets_out: *mut u64,
                         total_out_host: *mut u64) -> c_int;
    pub fn oi_query_terms(ctx: *mut OiCtx, blob: *const u8, offsets: *const u32, n_queries: u32, blob_bytes: u32, vocab: u32,
                          location: c_int, query_terms_out: *mut u32, term_capacity: u64, q_term_offsets_out: *mut u32,
                          total_out_host: *mut u64) -> c_int;
    pub fn oi_index_set_text(idx: *mut OiIndex, blob: *const u8, offsets: *const u64, blob_bytes: u64, location: c_int) -> c_int;

    // filtered search (per-document group / stamp attributes, one oi_doc_filter per query)
    pub fn oi_index_set_doc_attrs(idx: *mut OiIndex, group: *const u32, stamp: *const u32, location: c_int) -> c_int;
    pub fn oi_search_lists_filtered(idx: *mut OiIndex, query_vecs: *const f32, query_terms: *const u32, q_term_offsets: *const u32,
                                    n_queries: u32, depth: u32, filters: *const OiDocFilter, location: c_int,
                                    cos_scores: *mut f32, cos_docs: *mut u32, cos_counts: *mut u32, bm25_scores: *mut f32,
                                    bm25_docs: *mut u32, bm25_counts: *mut u32) -> c_int;
    pub fn oi_search_lists_packed_filtered(idx: *mut OiIndex, query_vecs: *const f32, query_terms: *const u32,
                                           q_term_offsets: *const u32, n_queries: u32, depth: u32, filters: *const OiDocFilter,
                                           location: c_int, packed_out: *mut u32) -> c_int;
    pub fn oi_search_filtered(idx: *mut OiIndex, query_vecs: *const f32, query_terms: *const u32, q_term_offsets: *const u32,
                              n_queries: u32, depth: u32, k: u32, filters: *const OiDocFilter, location: c_int,
                              scores_out: *mut f32, docs_out: *mut u32, counts_out: *mut u32) -> c_int;
    pub fn oi_search_sharded_filtered(idx: *mut OiIndex, comm: *mut OiComm, query_vecs: *const f32, query_terms: *const u32,
                                      q_term_offsets: *const u32, n_queries: u32, depth: u32, k: u32,
                                      filters: *const OiDocFilter, location: c_int, scores_out: *mut f32, docs_out: *mut u32,
                                      counts_out: *mut u32) -> c_int;

    // near-duplicate collapse of ranked lists (scores / scores_out and dup_counts_out may be null)
    pub fn oi_collapse_lists(idx: *mut OiIndex, scores: *const f32, docs: *const u32, counts: *const u32, n_queries: u32,
                             depth: u32, threshold: f32, k: u32, location: c_int, scores_out: *mut f32, docs_out: *mut u32,
                             counts_out: *mut u32, dup_counts_out: *mut u32) -> c_int;
    pub fn oi_search_collapsed(idx: *mut OiIndex, query_vecs: *const f32, query_terms: *const u32, q_term_offsets: *const u32,
                               n_queries: u32, depth: u32, pool: u32, k: u32, threshold: f32, filters: *const OiDocFilter,
                               location: c_int, scores_out: *mut f32, docs_out: *mut u32, counts_out: *mut u32,
                               dup_counts_out: *mut u32) -> c_int;

    // similarity volume: counts_out[n_queries][n_buckets]; spec is a host pointer whatever `location`; filters may be null
    pub fn oi_similar_volume(idx: *mut OiIndex, query_vecs: *const f32, n_queries: u32, spec: *const OiVolumeSpec,
                             filters: *const OiDocFilter, location: c_int, counts_out: *mut u32) -> c_int;

    // similarity summary: one signal record per local row (sources may be null: all reddit), then out[n_queries][n_buckets]
    // records of social_summary sums; spec is a host pointer whatever `location`; thresholds and filters may be null
    pub fn oi_index_set_signals(idx: *mut OiIndex, polarity: *const f64, speculative: *const u8, sources: *const u8,
                                bull_bear_threshold: f64, location: c_int) -> c_int;
    pub fn oi_similar_summary(idx: *mut OiIndex, query_vecs: *const f32, n_queries: u32, spec: *const OiSummarySpec,
                              thresholds: *const f32, filters: *const OiDocFilter, location: c_int,
                              out: *mut OiSocialCounters) -> c_int;

    // similarity leaderboard: records per (query, key) -- dense [n_queries][n_keys] (top == 0; the other outputs may be null), or
    // the best `top` keys ranked: records and keys [n_queries][top], counts and (may be null) qualified [n_queries]
    pub fn oi_similar_groups(idx: *mut OiIndex, query_vecs: *const f32, n_queries: u32, spec: *const OiGroupsSpec,
                             thresholds: *const f32, filters: *const OiDocFilter, location: c_int,
                             records_out: *mut OiSocialCounters, keys_out: *mut u32, counts_out: *mut u32,
                             qualified_out: *mut u32) -> c_int;

    // similarity share: the summary's arguments, every document counted at most once, under the query it is most like;
    // labels_out [n_docs] by local row (0xFFFFFFFF: not assigned) may be null
    pub fn oi_similar_share(idx: *mut OiIndex, query_vecs: *const f32, n_queries: u32, spec: *const OiSummarySpec,
                            thresholds: *const f32, filters: *const OiDocFilter, location: c_int,
                            out: *mut OiSocialCounters, labels_out: *mut u32) -> c_int;

    // mention summary: the social_summary sums of the documents that contain at least need_q of a query's distinct terms, per
    // time bucket or group key; min_match [n_queries] (0: all) and filters may be null; needs postings and signals, no embeddings
    pub fn oi_mention_summary(idx: *mut OiIndex, query_terms: *const u32, q_term_offsets: *const u32, n_queries: u32,
                              spec: *const OiMentionSpec, min_match: *const u32, filters: *const OiDocFilter, location: c_int,
                              out: *mut OiSocialCounters) -> c_int;

    // narrative discovery: the update step of a clustering (integer sums per label: exact, shards add), sums -> unit
    // vectors (previous may be null), and the k-means loop over oi_similar_share (filter: ONE, may be null; labels_out may
    // be null; spec, filter and info_host are host pointers whatever `location`)
    pub fn oi_label_sums(idx: *mut OiIndex, labels: *const u32, n_clusters: u32, location: c_int, sums_out: *mut i64,
                         counts_out: *mut u64) -> c_int;
    pub fn oi_centroids_from_sums(ctx: *mut OiCtx, sums: *const i64, counts: *const u64, previous: *const f32, n_clusters: u32,
                                  dim: u32, location: c_int, centroids_out: *mut f32) -> c_int;
    pub fn oi_narratives_fit(idx: *mut OiIndex, seeds: *const f32, n_clusters: u32, spec: *const OiNarrativeSpec,
                             filter: *const OiDocFilter, location: c_int, centroids_out: *mut f32,
                             records_out: *mut OiSocialCounters, labels_out: *mut u32, info_host: *mut OiNarrativeInfo) -> c_int;
    // the seeds of that loop, chosen on the device among the stored rows (filter: ONE, may be null; rows_out and info_host may
    // be null; spec, filter and info_host are host pointers whatever `location`)
    pub fn oi_narratives_seed(idx: *mut OiIndex, n_clusters: u32, spec: *const OiSeedSpec, filter: *const OiDocFilter,
                              location: c_int, seeds_out: *mut f32, rows_out: *mut u32, info_host: *mut OiSeedInfo) -> c_int;

    // narrative terms: labels -> the [vocab][n_clusters] table of documents per (term, cluster) and the cluster sizes (exact,
    // shards add); a table and sizes -> the ranked lists; their composition (sizes_out may be null; spec and sizes_host are
    // host pointers whatever `location`)
    pub fn oi_label_term_counts(idx: *mut OiIndex, labels: *const u32, n_clusters: u32, location: c_int, counts_out: *mut u32,
                                sizes_out: *mut u64) -> c_int;
    pub fn oi_label_terms_rank(ctx: *mut OiCtx, counts: *const u32, sizes_host: *const u64, vocab: u32, n_clusters: u32,
                               spec: *const OiLabelTermsSpec, location: c_int, terms_out: *mut OiLabelTerm, n_out: *mut u32) -> c_int;
    pub fn oi_label_terms(idx: *mut OiIndex, labels: *const u32, n_clusters: u32, spec: *const OiLabelTermsSpec, location: c_int,
                          terms_out: *mut OiLabelTerm, n_out: *mut u32, sizes_out: *mut u64) -> c_int;

    // narrative exemplars: per cluster of a labelling, its member rows closest to its centroid as ranked lists [n_clusters][top]
    // (global doc ids; score 0 / doc u32::MAX beyond counts_out[c]); spec and filter (one, or null) are host pointers
    pub fn oi_label_exemplars(idx: *mut OiIndex, labels: *const u32, centroids: *const f32, n_clusters: u32, spec: *const OiExemplarSpec,
                              filter: *const OiDocFilter, location: c_int, scores_out: *mut f32, docs_out: *mut u32,
                              counts_out: *mut u32) -> c_int;

    // narrative breakdown: per cluster of a labelling the social_summary records per time bucket or key; dense (spec.top == 0:
    // [n_clusters][n_cells], keys / counts / qualified may be null) or ranked ([n_clusters][top]); spec and filter are host pointers
    pub fn oi_label_summary(idx: *mut OiIndex, labels: *const u32, n_clusters: u32, spec: *const OiLabelSummarySpec,
                            filter: *const OiDocFilter, location: c_int, records_out: *mut OiSocialCounters, keys_out: *mut u32,
                            counts_out: *mut u32, qualified_out: *mut u32) -> c_int;

    pub fn oi_pipeline_create(idx: *mut OiIndex, comm: *mut OiComm, lanes: u32, max_queries: u32, max_query_terms: u32,
                              depth: u32, k: u32, out: *mut *mut OiPipeline) -> c_int;
    pub fn oi_pipeline_destroy(p: *mut OiPipeline);
    pub fn oi_pipeline_submit(p: *mut OiPipeline, query_vecs: *const f32, query_terms: *const u32,
                              q_term_offsets: *const u32, n_queries: u32, location: c_int, scores_out: *mut f32,
                              docs_out: *mut u32, counts_out: *mut u32, ticket_out: *mut u64) -> c_int;
    pub fn oi_pipeline_wait(p: *mut OiPipeline, ticket: u64, host_sync: c_int) -> c_int;
    pub fn oi_pipeline_drain(p: *mut OiPipeline) -> c_int;
    pub fn oi_pipeline_workspace_bytes(p: *mut OiPipeline, device_bytes_out: *mut u64,
                                       pinned_host_bytes_out: *mut u64) -> c_int;
    pub fn oi_pipeline_concurrent_streams(p: *mut OiPipeline, concurrent_out: *mut u32, streams_out: *mut u32) -> c_int;
    pub fn oi_pipeline_profile_reset(p: *mut OiPipeline, enable: c_int) -> c_int;
    pub fn oi_pipeline_profile_read(p: *mut OiPipeline, kernel_tag: *const c_char, total_ms_out: *mut f64,
                                    launches_out: *mut u64) -> c_int;

    pub fn oi_screen_probe(idx: *mut OiIndex, query_vecs: *const f32, n_queries: u32, row_begin: u64, n_rows: u32,
                           screen_scores_out: *mut f32, eps_out: *mut f32) -> c_int;
    pub fn oi_profile_reset(ctx: *mut OiCtx, enable: c_int) -> c_int;
    pub fn oi_profile_read(ctx: *mut OiCtx, kernel_tag: *const c_char, total_ms_out: *mut f64,
                           launches_out: *mut u64) -> c_int;
}
