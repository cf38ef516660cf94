//! Safe wrappers over libopenintel_hip.so and, with feature "reference", the adapter that implements the
//! reference's `PostAnalyzer` port (src/domain/ports/post_analyzer.rs:7-11) on top of them.
//!
//! NOT compile-checked in the build image (no cargo/rustc there); see Cargo.toml.
pub mod ffi;

use std::ffi::CStr;
use std::sync::Arc;

/// A failed library call: the status code and the thread-local message (`oi_last_error`).
#[derive(Debug, Clone)]
pub struct HipError {
    pub code: i32,
    pub message: String,
}
impl std::fmt::Display for HipError {
    fn fmt(&self, f: &mut std::fmt::Formatter<'_>) -> std::fmt::Result {
        write!(f, "libopenintel_hip error {}: {}", self.code, self.message)
    }
}
impl std::error::Error for HipError {}

fn check(rc: i32) -> Result<(), HipError> {
    if rc == 0 {
        return Ok(());
    }
    // never unwind across the ABI: the library reports, the shim converts
    let message = unsafe { CStr::from_ptr(ffi::oi_last_error()) }.to_string_lossy().into_owned();
    Err(HipError { code: rc, message })
}

/// Owns an `oi_ctx`.  The library serialises calls on a ctx with an internal mutex, so the handle may be shared
/// between threads: that is what makes the `Send + Sync` below sound (`PostAnalyzer: Send + Sync`,
/// post_analyzer.rs:7; tests/test_gpu_threads.py drives one ctx from eight host threads).
pub struct HipCtx(*mut ffi::OiCtx);
unsafe impl Send for HipCtx {}
unsafe impl Sync for HipCtx {}
impl Drop for HipCtx {
    fn drop(&mut self) {
        unsafe { ffi::oi_destroy(self.0) }
    }
}
impl HipCtx {
    pub fn new(device: i32) -> Result<Arc<Self>, HipError> {
        let mut p = std::ptr::null_mut();
        check(unsafe { ffi::oi_create(device, &mut p) })?;
        Ok(Arc::new(HipCtx(p)))
    }
    pub fn raw(&self) -> *mut ffi::OiCtx {
        self.0
    }
}

/// Integer sums and counts (`HipIndex::label_sums`, or the total over the shards of the documents) to unit vectors
/// (`oi_centroids_from_sums`): sums / |sums| in f64, rounded once.  A cluster with count 0 or an all-zero sum keeps
/// `previous` (zeros without one).
pub fn centroids_from_sums(ctx: &HipCtx, sums: &[i64], counts: &[u64], previous: Option<&[f32]>, dim: usize) -> Result<Vec<f32>, HipError> {
    assert_eq!(sums.len(), counts.len() * dim);
    if let Some(p) = previous {
        assert_eq!(p.len(), sums.len());
    }
    let mut out = vec![0f32; sums.len()];
    check(unsafe {
        ffi::oi_centroids_from_sums(ctx.raw(), sums.as_ptr(), counts.as_ptr(), previous.map_or(std::ptr::null(), |p| p.as_ptr()),
                                    counts.len() as u32, dim as u32, ffi::OI_HOST, out.as_mut_ptr())
    })?;
    Ok(out)
}

/// A table and sizes (`HipIndex::label_term_counts`, or the total over the shards of the documents) to the ranked lists
/// (`oi_label_terms_rank`): per cluster its eligible terms (df_cluster >= max(min_df, 1)), best first by excess, then
/// df_cluster, then the smaller id.  The sum of the sizes must not exceed 2^31 - 1.
pub fn rank_label_terms(ctx: &HipCtx, counts: &[u32], sizes: &[u64], top: u32, min_df: u32) -> Result<Vec<Vec<ffi::OiLabelTerm>>, HipError> {
    let k = sizes.len();
    assert!(k > 0 && counts.len() % k == 0);
    let spec = ffi::OiLabelTermsSpec { top, min_df, reserved: [0, 0] };
    let width = top.clamp(1, ffi::OI_MAX_LABEL_TERMS) as usize;
    let mut rec = vec![ffi::OiLabelTerm::default(); k * width];
    let mut n = vec![0u32; k];
    check(unsafe {
        ffi::oi_label_terms_rank(ctx.raw(), counts.as_ptr(), sizes.as_ptr(), (counts.len() / k) as u32, k as u32, &spec, ffi::OI_HOST,
                                 rec.as_mut_ptr(), n.as_mut_ptr())
    })?;
    Ok((0..k).map(|c| rec[c * width..c * width + n[c] as usize].to_vec()).collect())
}

/// Gather strings into the FFI layout: one UTF-8 blob + (n + 1) u64 offsets.  In the reference every post owns
/// its text as a separate heap `String` (social_post.rs:25-27).
pub fn gather<'a, I: IntoIterator<Item = &'a str>>(texts: I) -> (Vec<u8>, Vec<u64>) {
    let mut blob = Vec::new();
    let mut offsets = vec![0u64];
    for t in texts {
        blob.extend_from_slice(t.as_bytes());
        offsets.push(blob.len() as u64);
    }
    (blob, offsets)
}

/// Query texts -> the `query_terms` of `HipIndex::search*` (`oi_query_terms`): the tokens of lexicon.rs:54-58 hashed onto
/// [0, vocab), in text order, duplicates kept.  `vocab` is the index's.
pub fn query_terms(ctx: &HipCtx, texts: &[&str], vocab: u32) -> Result<Vec<Vec<u32>>, HipError> {
    let (blob, offsets64) = gather(texts.iter().copied());
    assert!(blob.len() <= u32::MAX as usize && texts.len() < u32::MAX as usize, "a query batch has u32 offsets: under 4 GiB of text");
    let offsets: Vec<u32> = offsets64.iter().map(|&o| o as u32).collect();
    let mut terms = vec![0u32; (blob.len() + 1) / 2 + 1];
    let mut toffs = vec![0u32; texts.len() + 1];
    check(unsafe {
        ffi::oi_query_terms(ctx.raw(), blob.as_ptr(), offsets.as_ptr(), texts.len() as u32, blob.len() as u32, vocab, ffi::OI_HOST,
                            terms.as_mut_ptr(), terms.len() as u64, toffs.as_mut_ptr(), std::ptr::null_mut())
    })?;
    Ok((0..texts.len()).map(|q| terms[toffs[q] as usize..toffs[q + 1] as usize].to_vec()).collect())
}

/// `LexiconAnalyzer::score` for every text (lexicon.rs:53-73): (polarity, speculative), index-aligned.
pub fn analyze_texts(ctx: &HipCtx, texts: &[&str]) -> Result<Vec<(f64, bool)>, HipError> {
    let (blob, offsets) = gather(texts.iter().copied());
    let n = texts.len();
    let (mut pol, mut spec) = (vec![0f64; n], vec![0u8; n]);
    check(unsafe {
        ffi::oi_lexicon_analyze(ctx.raw(), blob.as_ptr(), offsets.as_ptr(), n as u64, pol.as_mut_ptr(), spec.as_mut_ptr())
    })?;
    Ok(pol.into_iter().zip(spec).map(|(p, s)| (p, s != 0)).collect())
}

/// The batch tools' unit of work (mcp/tools.rs:193-225 `run_scan`, :303-352 `run_compare`): the texts of MANY tickers
/// through one scan, and every ticker's `social_summary` sums (speculation_engine.rs:76-97) from one reduction.
/// `segments[s]` = that ticker's (text, source) pairs in fetch order; returns the per-post signals, index-aligned with
/// the flattened input, and one counters record per ticker whose `polarity_sum` is the reference's input-order sum.
pub fn analyze_segments(ctx: &HipCtx, segments: &[Vec<(&str, u8)>], bull_bear_threshold: f64)
    -> Result<(Vec<(f64, bool)>, Vec<ffi::OiSocialCounters>), HipError> {
    let (blob, offsets) = gather(segments.iter().flatten().map(|(t, _)| *t));
    let sources: Vec<u8> = segments.iter().flatten().map(|(_, s)| *s).collect();
    let n = sources.len();
    let mut seg = vec![0u64];
    for s in segments {
        seg.push(seg.last().unwrap() + s.len() as u64);
    }
    let (mut pol, mut spec) = (vec![0f64; n], vec![0u8; n]);
    check(unsafe {
        ffi::oi_lexicon_analyze(ctx.raw(), blob.as_ptr(), offsets.as_ptr(), n as u64, pol.as_mut_ptr(), spec.as_mut_ptr())
    })?;
    let mut out: Vec<ffi::OiSocialCounters> = (0..segments.len()).map(|_| unsafe { std::mem::zeroed() }).collect();
    check(unsafe {
        ffi::oi_social_summary_segmented(ctx.raw(), sources.as_ptr(), pol.as_ptr(), spec.as_ptr(), n as u64, seg.as_ptr(),
                                         segments.len() as u64, bull_bear_threshold, ffi::OI_HOST, out.as_mut_ptr())
    })?;
    Ok((pol.into_iter().zip(spec).map(|(p, s)| (p, s != 0)).collect(), out))
}

/// Per-title result of the headline gate's scan (dip.rs:247-272).
pub struct TitleScan {
    /// indices into CATALYST_KEYWORDS (dip.rs:38-55) in first-occurrence order: `catalyst_hits(&[title])`
    pub hits: Vec<usize>,
    /// `headline_mentions_company(title, ticker, name_forms)`
    pub about_company: bool,
}

pub fn scan_titles(ctx: &HipCtx, titles: &[&str], ticker: &str, name_forms: &[String]) -> Result<Vec<TitleScan>, HipError> {
    let (blob, offsets) = gather(titles.iter().copied());
    let mut fblob = Vec::new();
    let mut foffs = vec![0u32];
    for f in name_forms {
        fblob.extend_from_slice(f.as_bytes());
        foffs.push(fblob.len() as u32);
    }
    let n = titles.len();
    let (mut mask, mut order, mut about) = (vec![0u16; n], vec![0u64; n], vec![0u8; n]);
    check(unsafe {
        ffi::oi_headline_scan(ctx.raw(), blob.as_ptr(), offsets.as_ptr(), n as u64, ticker.as_ptr(), ticker.len() as u64,
                              fblob.as_ptr(), foffs.as_ptr(), name_forms.len() as u32, mask.as_mut_ptr(),
                              order.as_mut_ptr(), about.as_mut_ptr())
    })?;
    Ok((0..n)
        .map(|i| TitleScan {
            hits: (0..mask[i].count_ones()).map(|j| ((order[i] >> (4 * j)) & 15) as usize).collect(),
            about_company: about[i] != 0,
        })
        .collect())
}

/// The gate's scan for every row of a dip scan in one call (application/dip.rs: `check` per loser; `oi_headline_scan_rows`):
/// `rows[r]` = (that loser's headlines, its ticker, its `company_name_forms`).  Per row what `scan_titles` returns.
pub fn scan_title_rows(ctx: &HipCtx, rows: &[(Vec<&str>, &str, Vec<String>)]) -> Result<Vec<Vec<TitleScan>>, HipError> {
    let (blob, offsets) = gather(rows.iter().flat_map(|r| r.0.iter().copied()));
    let (mut row_off, mut tick_off, mut rform_off) = (vec![0u64], vec![0u32], vec![0u32]);
    let (mut tblob, mut fblob, mut foffs) = (Vec::new(), Vec::new(), vec![0u32]);
    for (titles, ticker, forms) in rows {
        row_off.push(row_off.last().unwrap() + titles.len() as u64);
        tblob.extend_from_slice(ticker.as_bytes());
        tick_off.push(tblob.len() as u32);
        for f in forms {
            fblob.extend_from_slice(f.as_bytes());
            foffs.push(fblob.len() as u32);
        }
        rform_off.push(foffs.len() as u32 - 1);
    }
    let n = *row_off.last().unwrap() as usize;
    let (mut mask, mut order, mut about) = (vec![0u16; n], vec![0u64; n], vec![0u8; n]);
    check(unsafe {
        ffi::oi_headline_scan_rows(ctx.raw(), blob.as_ptr(), offsets.as_ptr(), n as u64, row_off.as_ptr(), rows.len() as u32,
                                   tblob.as_ptr(), tick_off.as_ptr(), fblob.as_ptr(), foffs.as_ptr(), rform_off.as_ptr(),
                                   mask.as_mut_ptr(), order.as_mut_ptr(), about.as_mut_ptr())
    })?;
    Ok(rows
        .iter()
        .enumerate()
        .map(|(r, _)| {
            (row_off[r] as usize..row_off[r + 1] as usize)
                .map(|i| TitleScan {
                    hits: (0..mask[i].count_ones()).map(|j| ((order[i] >> (4 * j)) & 15) as usize).collect(),
                    about_company: about[i] != 0,
                })
                .collect()
        })
        .collect())
}

/// One corpus shard in HBM (`oi_index`).  New API: the reference has no retrieval port.
pub struct HipIndex {
    ctx: Arc<HipCtx>,
    idx: *mut ffi::OiIndex,
    dim: usize,
    n_docs: usize, // rows of this shard (the length of every per-document array)
    source: Option<Arc<HipIndex>>, // a view keeps the index it borrows from alive (oi_index_view)
}
unsafe impl Send for HipIndex {}
unsafe impl Sync for HipIndex {}
impl Drop for HipIndex {
    fn drop(&mut self) {
        unsafe { ffi::oi_index_destroy(self.idx) }
    }
}
pub struct RankedPost {
    pub doc_id: u32,
    pub score: f32,
}
/// Concatenated query terms and their offsets (a never-empty term buffer).
fn flatten_terms(query_terms: &[Vec<u32>]) -> (Vec<u32>, Vec<u32>) {
    let mut flat = Vec::new();
    let mut offs = vec![0u32];
    for t in query_terms {
        flat.extend_from_slice(t);
        offs.push(flat.len() as u32);
    }
    if flat.is_empty() {
        flat.push(0);
    }
    (flat, offs)
}
/// The first counts[q] entries of each query's row of stride k.
fn ranked(s: &[f32], d: &[u32], c: &[u32], k: usize) -> Vec<Vec<RankedPost>> {
    (0..c.len())
        .map(|q| (0..c[q] as usize).map(|i| RankedPost { doc_id: d[q * k + i], score: s[q * k + i] }).collect())
        .collect()
}
impl HipIndex {
    /// rows: n_docs x dim f32 (copied to HBM, L2-normalised); forward index: doc d owns terms[offsets[d]..offsets[d+1]].
    pub fn build(ctx: Arc<HipCtx>, rows: &mut [f32], dim: usize, vocab: u32, terms: &[u32], offsets: &[u64]) -> Result<Self, HipError> {
        let n_docs = (rows.len() / dim) as u64;
        let mut idx = std::ptr::null_mut();
        check(unsafe { ffi::oi_index_create(ctx.raw(), n_docs, dim as u32, vocab, 0, &mut idx) })?;
        let me = HipIndex { ctx, idx, dim, n_docs: n_docs as usize, source: None };
        check(unsafe { ffi::oi_index_set_embeddings(me.idx, rows.as_mut_ptr(), ffi::OI_HOST, 1) })?;
        check(unsafe { ffi::oi_index_set_forward(me.idx, terms.as_ptr(), offsets.as_ptr(), ffi::OI_HOST) })?;
        let mut tokens = 0u64;
        check(unsafe { ffi::oi_index_local_stats(me.idx, &mut tokens, std::ptr::null_mut()) })?;
        check(unsafe { ffi::oi_index_finalize(me.idx, n_docs, tokens, std::ptr::null()) })?;
        Ok(me)
    }
    /// `build` from the posts' TEXT (`oi_index_set_text`): the reference's tokens (lexicon.rs:54-58) hashed onto [0, vocab),
    /// so there is no dictionary to keep; queries go through `query_terms` with the same vocab.
    pub fn build_from_texts(ctx: Arc<HipCtx>, rows: &mut [f32], dim: usize, vocab: u32, texts: &[&str]) -> Result<Self, HipError> {
        let n_docs = (rows.len() / dim) as u64;
        assert_eq!(texts.len() as u64, n_docs, "one text per embedding row");
        let (blob, offsets) = gather(texts.iter().copied());
        let mut idx = std::ptr::null_mut();
        check(unsafe { ffi::oi_index_create(ctx.raw(), n_docs, dim as u32, vocab, 0, &mut idx) })?;
        let me = HipIndex { ctx, idx, dim, n_docs: n_docs as usize, source: None };
        check(unsafe { ffi::oi_index_set_embeddings(me.idx, rows.as_mut_ptr(), ffi::OI_HOST, 1) })?;
        check(unsafe { ffi::oi_index_set_text(me.idx, blob.as_ptr(), offsets.as_ptr(), blob.len() as u64, ffi::OI_HOST) })?;
        let mut tokens = 0u64;
        check(unsafe { ffi::oi_index_local_stats(me.idx, &mut tokens, std::ptr::null_mut()) })?;
        check(unsafe { ffi::oi_index_finalize(me.idx, n_docs, tokens, std::ptr::null()) })?;
        Ok(me)
    }
    /// A second, read-only handle on this shard bound to `ctx` (a context of its own: another stream, other workspaces),
    /// so that two searches can be in flight at once; costs no HBM.
    pub fn view(self: &Arc<Self>, ctx: Arc<HipCtx>) -> Result<HipIndex, HipError> {
        let mut idx = std::ptr::null_mut();
        check(unsafe { ffi::oi_index_view(self.idx, ctx.raw(), &mut idx) })?;
        Ok(HipIndex { ctx, idx, dim: self.dim, n_docs: self.n_docs, source: Some(Arc::clone(self)) })
    }
    /// Per-document attributes of filtered searches (`oi_index_set_doc_attrs`): n_docs entries each, local rows; None = zeros.
    /// A later call overwrites them in place (retag or soft-delete posts without a rebuild).
    pub fn set_doc_attrs(&self, group: Option<&[u32]>, stamp: Option<&[u32]>) -> Result<(), HipError> {
        for a in [group, stamp].into_iter().flatten() {
            assert_eq!(a.len(), self.n_docs, "one attribute per document of the shard"); // (the C call reads n_docs of each)
        }
        let p = |a: Option<&[u32]>| a.map_or(std::ptr::null(), |v| v.as_ptr());
        check(unsafe { ffi::oi_index_set_doc_attrs(self.idx, p(group), p(stamp), ffi::OI_HOST) })
    }
    /// `search` restricted to the documents that pass each query's filter (one per query): scores unchanged.
    pub fn search_filtered(&self, query_vecs: &[f32], query_terms: &[Vec<u32>], filters: &[ffi::OiDocFilter], k: usize,
                           depth: usize) -> Result<Vec<Vec<RankedPost>>, HipError> {
        let b = query_terms.len();
        assert_eq!(query_vecs.len(), b * self.dim);
        assert_eq!(filters.len(), b);
        let (flat, offs) = flatten_terms(query_terms);
        let (mut s, mut d, mut c) = (vec![0f32; b * k], vec![0u32; b * k], vec![0u32; b]);
        check(unsafe {
            ffi::oi_search_filtered(self.idx, query_vecs.as_ptr(), flat.as_ptr(), offs.as_ptr(), b as u32, depth as u32,
                                    k as u32, filters.as_ptr(), ffi::OI_HOST, s.as_mut_ptr(), d.as_mut_ptr(), c.as_mut_ptr())
        })?;
        Ok(ranked(&s, &d, &c, k))
    }
    /// `search_filtered` with k = pool, then the near-duplicate collapse of each fused list (`oi_search_collapsed`): an entry
    /// whose stored row has a dot product >= threshold with a better-ranked kept entry is folded into it.  Per query: the
    /// kept posts (<= k, RRF scores) and, index-aligned, how many posts of the pool each one stands for (itself included).
    /// filters: None = unfiltered.
    pub fn search_collapsed(&self, query_vecs: &[f32], query_terms: &[Vec<u32>], filters: Option<&[ffi::OiDocFilter]>, k: usize,
                            depth: usize, pool: usize, threshold: f32) -> Result<Vec<(Vec<RankedPost>, Vec<u32>)>, HipError> {
        let b = query_terms.len();
        assert_eq!(query_vecs.len(), b * self.dim);
        if let Some(f) = filters {
            assert_eq!(f.len(), b);
        }
        let (flat, offs) = flatten_terms(query_terms);
        let (mut s, mut d, mut c, mut n) = (vec![0f32; b * k], vec![0u32; b * k], vec![0u32; b], vec![0u32; b * k]);
        check(unsafe {
            ffi::oi_search_collapsed(self.idx, query_vecs.as_ptr(), flat.as_ptr(), offs.as_ptr(), b as u32, depth as u32,
                                     pool as u32, k as u32, threshold, filters.map_or(std::ptr::null(), |f| f.as_ptr()),
                                     ffi::OI_HOST, s.as_mut_ptr(), d.as_mut_ptr(), c.as_mut_ptr(), n.as_mut_ptr())
        })?;
        let posts = ranked(&s, &d, &c, k);
        Ok(posts.into_iter().enumerate().map(|(q, p)| { let m = p.len(); (p, n[q * k..q * k + m].to_vec()) }).collect())
    }
    /// How many posts of the shard are like each query, per time bucket (`oi_similar_volume`): per query `n_buckets` counts of
    /// the documents that pass its filter, whose stamp falls into bucket (stamp - stamp_origin) / bucket_width and whose
    /// similarity -- the f32 score `search` ranks by -- is >= spec.threshold.  filters: None = every document passes.
    /// Counts of shards add.
    pub fn similar_volume(&self, query_vecs: &[f32], spec: ffi::OiVolumeSpec, filters: Option<&[ffi::OiDocFilter]>)
                          -> Result<Vec<Vec<u32>>, HipError> {
        assert_eq!(query_vecs.len() % self.dim, 0);
        let b = query_vecs.len() / self.dim;
        if let Some(f) = filters {
            assert_eq!(f.len(), b);
        }
        let nb = spec.n_buckets as usize;
        let mut counts = vec![0u32; b * nb];
        check(unsafe {
            ffi::oi_similar_volume(self.idx, query_vecs.as_ptr(), b as u32, &spec, filters.map_or(std::ptr::null(), |f| f.as_ptr()),
                                   ffi::OI_HOST, counts.as_mut_ptr())
        })?;
        Ok(counts.chunks(nb.max(1)).map(|c| c.to_vec()).collect())
    }
    /// The per-post signals the summary sums (`oi_index_set_signals`): what the lexicon analyzer returned for the shard's posts,
    /// n_docs entries each, local rows; sources: 0 = reddit, 1 = bluesky, None = all reddit.  The bullish / bearish class of a
    /// post is fixed here with `bull_bear_threshold`.  A later call overwrites the signals in place.
    pub fn set_signals(&self, polarity: &[f64], speculative: &[u8], sources: Option<&[u8]>, bull_bear_threshold: f64)
                       -> Result<(), HipError> {
        assert_eq!(polarity.len(), self.n_docs, "one signal per document of the shard"); // (the C call reads n_docs of each)
        assert_eq!(speculative.len(), self.n_docs);
        if let Some(s) = sources {
            assert_eq!(s.len(), self.n_docs);
        }
        check(unsafe {
            ffi::oi_index_set_signals(self.idx, polarity.as_ptr(), speculative.as_ptr(), sources.map_or(std::ptr::null(), |s| s.as_ptr()),
                                      bull_bear_threshold, ffi::OI_HOST)
        })
    }
    /// The sentiment of the posts like each query, per time bucket (`oi_similar_summary`): per query `n_buckets` records of the
    /// social_summary sums over exactly the documents `similar_volume` counts.  thresholds: one per query, None = spec.threshold
    /// for all.  Integer fields exact, polarity_sum a 64-bit integer sum of 2^-30 steps: deterministic.  Records of shards add.
    pub fn similar_summary(&self, query_vecs: &[f32], spec: ffi::OiSummarySpec, thresholds: Option<&[f32]>,
                           filters: Option<&[ffi::OiDocFilter]>) -> Result<Vec<Vec<ffi::OiSocialCounters>>, HipError> {
        assert_eq!(query_vecs.len() % self.dim, 0);
        let b = query_vecs.len() / self.dim;
        if let Some(f) = filters {
            assert_eq!(f.len(), b);
        }
        if let Some(t) = thresholds {
            assert_eq!(t.len(), b);
        }
        let nb = spec.n_buckets as usize;
        let mut out = vec![ffi::OiSocialCounters::default(); b * nb];
        check(unsafe {
            ffi::oi_similar_summary(self.idx, query_vecs.as_ptr(), b as u32, &spec, thresholds.map_or(std::ptr::null(), |t| t.as_ptr()),
                                    filters.map_or(std::ptr::null(), |f| f.as_ptr()), ffi::OI_HOST, out.as_mut_ptr())
        })?;
        Ok(out.chunks(nb.max(1)).map(|c| c.to_vec()).collect())
    }
    /// The posts divided among the queries of a batch (`oi_similar_share`): `similar_summary`'s records, but every document is
    /// counted at most once, under the candidate query with the largest similarity (ties to the smallest query).  With
    /// `labels` the second value holds, per local row, the winner of an assigned document and 0xFFFFFFFF for every other row.
    /// Deterministic; unlike its siblings the result depends on the batch composition.
    pub fn similar_share(&self, query_vecs: &[f32], spec: ffi::OiSummarySpec, thresholds: Option<&[f32]>,
                         filters: Option<&[ffi::OiDocFilter]>, labels: bool)
                         -> Result<(Vec<Vec<ffi::OiSocialCounters>>, Option<Vec<u32>>), HipError> {
        assert_eq!(query_vecs.len() % self.dim, 0);
        let b = query_vecs.len() / self.dim;
        if let Some(f) = filters {
            assert_eq!(f.len(), b);
        }
        if let Some(t) = thresholds {
            assert_eq!(t.len(), b);
        }
        let nb = spec.n_buckets as usize;
        let mut out = vec![ffi::OiSocialCounters::default(); b * nb];
        let mut lab = if labels { Some(vec![u32::MAX; self.n_docs]) } else { None };
        check(unsafe {
            ffi::oi_similar_share(self.idx, query_vecs.as_ptr(), b as u32, &spec, thresholds.map_or(std::ptr::null(), |t| t.as_ptr()),
                                  filters.map_or(std::ptr::null(), |f| f.as_ptr()), ffi::OI_HOST, out.as_mut_ptr(),
                                  lab.as_mut().map_or(std::ptr::null_mut(), |l| l.as_mut_ptr()))
        })?;
        Ok((out.chunks(nb.max(1)).map(|c| c.to_vec()).collect(), lab))
    }
    /// The sentiment of the posts that MENTION a query's terms (`oi_mention_summary`): one record per query and cell -- a time
    /// bucket (`OI_MENTION_AXIS_TIME`) or a key of the documents' group (`OI_MENTION_AXIS_KEY`).  A document matches a query
    /// when at least need_q of its DISTINCT terms occur in it: `min_match` None = 1 (any), an entry 0 = all of them.  Reads the
    /// postings of a finalized index and its signals; no embeddings.  At most 64 terms per query.  Records of shards add.
    pub fn mention_summary(&self, query_terms: &[u32], q_term_offsets: &[u32], spec: ffi::OiMentionSpec, min_match: Option<&[u32]>,
                           filters: Option<&[ffi::OiDocFilter]>) -> Result<Vec<Vec<ffi::OiSocialCounters>>, HipError> {
        assert!(!q_term_offsets.is_empty());
        let b = q_term_offsets.len() - 1;
        assert_eq!(*q_term_offsets.last().unwrap() as usize, query_terms.len());
        if let Some(f) = filters {
            assert_eq!(f.len(), b);
        }
        if let Some(m) = min_match {
            assert_eq!(m.len(), b);
        }
        let nc = spec.n_cells as usize;
        let mut out = vec![ffi::OiSocialCounters::default(); b * nc];
        let none = [0u32];
        let terms = if query_terms.is_empty() { &none[..] } else { query_terms };
        check(unsafe {
            ffi::oi_mention_summary(self.idx, terms.as_ptr(), q_term_offsets.as_ptr(), b as u32, &spec,
                                    min_match.map_or(std::ptr::null(), |m| m.as_ptr()), filters.map_or(std::ptr::null(), |f| f.as_ptr()),
                                    ffi::OI_HOST, out.as_mut_ptr())
        })?;
        Ok(out.chunks(nc.max(1)).map(|c| c.to_vec()).collect())
    }
    /// The update step of a clustering over the index (`oi_label_sums`): per label c < n_clusters the number of rows that
    /// carry it and the sum of rint(row * 2^30) over them, as 64-bit integers ([n_clusters * dim], [n_clusters]).  Any other
    /// label (0xFFFFFFFF, as `similar_share` writes for unassigned rows) is "no cluster".  Exact: shards of the documents add.
    pub fn label_sums(&self, labels: &[u32], n_clusters: u32) -> Result<(Vec<i64>, Vec<u64>), HipError> {
        assert_eq!(labels.len(), self.n_docs);
        let k = n_clusters as usize;
        let (mut sums, mut counts) = (vec![0i64; k * self.dim], vec![0u64; k]);
        check(unsafe { ffi::oi_label_sums(self.idx, labels.as_ptr(), n_clusters, ffi::OI_HOST, sums.as_mut_ptr(), counts.as_mut_ptr()) })?;
        Ok((sums, counts))
    }
    /// The documents per (term, cluster) of a labelling (`oi_label_term_counts`): ([vocab * n_clusters] term-major, sizes
    /// [n_clusters]) over the postings of a finalized index; a term counts once per document, any label >= n_clusters is "no
    /// cluster".  Exact: shards of the documents add.  `vocab` is the index's.
    pub fn label_term_counts(&self, labels: &[u32], n_clusters: u32, vocab: u32) -> Result<(Vec<u32>, Vec<u64>), HipError> {
        assert_eq!(labels.len(), self.n_docs);
        let k = n_clusters as usize;
        let (mut counts, mut sizes) = (vec![0u32; k.max(1) * vocab as usize], vec![0u64; k.max(1)]);
        check(unsafe { ffi::oi_label_term_counts(self.idx, labels.as_ptr(), n_clusters, ffi::OI_HOST, counts.as_mut_ptr(), sizes.as_mut_ptr()) })?;
        Ok((counts, sizes))
    }
    /// What each cluster of a labelling is about (`oi_label_terms`): per cluster its distinguishing terms, best first, and the
    /// cluster sizes.  The ids are valid query terms of `mention_summary` and of every search.
    pub fn label_terms(&self, labels: &[u32], n_clusters: u32, top: u32, min_df: u32) -> Result<(Vec<Vec<ffi::OiLabelTerm>>, Vec<u64>), HipError> {
        assert_eq!(labels.len(), self.n_docs);
        let k = n_clusters as usize;
        let spec = ffi::OiLabelTermsSpec { top, min_df, reserved: [0, 0] };
        let width = top.clamp(1, ffi::OI_MAX_LABEL_TERMS) as usize;
        let mut rec = vec![ffi::OiLabelTerm::default(); k.max(1) * width];
        let (mut n, mut sizes) = (vec![0u32; k.max(1)], vec![0u64; k.max(1)]);
        check(unsafe {
            ffi::oi_label_terms(self.idx, labels.as_ptr(), n_clusters, &spec, ffi::OI_HOST, rec.as_mut_ptr(), n.as_mut_ptr(), sizes.as_mut_ptr())
        })?;
        Ok(((0..k).map(|c| rec[c * width..c * width + n[c] as usize].to_vec()).collect(), sizes))
    }
    /// The posts to quote (`oi_label_exemplars`): per cluster of a labelling, its member rows closest to its centroid, best
    /// first, as (global doc id, score) -- score descending, ties to the smaller doc id, at most `top` per cluster.  A member
    /// has `labels[d] == c < n_clusters`, passes `filter` when one is given, and a sim that is not NaN.  `centroids` is
    /// [n_clusters * dim].  The lists of document shards merge with `oi_merge_lists`.
    pub fn label_exemplars(&self, labels: &[u32], centroids: &[f32], n_clusters: u32, top: u32,
                           filter: Option<&ffi::OiDocFilter>) -> Result<Vec<Vec<(u32, f32)>>, HipError> {
        assert_eq!(labels.len(), self.n_docs);
        let k = n_clusters as usize;
        let spec = ffi::OiExemplarSpec { top, reserved: [0, 0, 0] };
        let width = top.clamp(1, 1024) as usize;
        let (mut scores, mut docs, mut counts) = (vec![0f32; k.max(1) * width], vec![0u32; k.max(1) * width], vec![0u32; k.max(1)]);
        check(unsafe {
            ffi::oi_label_exemplars(self.idx, labels.as_ptr(), centroids.as_ptr(), n_clusters, &spec,
                                    filter.map_or(std::ptr::null(), |f| f as *const ffi::OiDocFilter), ffi::OI_HOST, scores.as_mut_ptr(),
                                    docs.as_mut_ptr(), counts.as_mut_ptr())
        })?;
        Ok((0..k).map(|c| (0..counts[c] as usize).map(|i| (docs[c * width + i], scores[c * width + i])).collect()).collect())
    }
    /// The narrative breakdown (`oi_label_summary`): the social_summary sums of the posts of each cluster of a labelling, one
    /// record per cluster and cell -- a time bucket (`OI_LABEL_AXIS_TIME`) or a key of the documents' group
    /// (`OI_LABEL_AXIS_KEY`).  `spec.top == 0`: dense records [n_clusters][n_cells], no keys.  `spec.top >= 1` (KEY axis): per
    /// cluster the listed (key, record) pairs, best first, as `similar_groups` ranks them.  Reads labels, attributes and
    /// signals only; any label >= n_clusters is "no cluster".  Dense records of shards add.
    pub fn label_summary(&self, labels: &[u32], n_clusters: u32, spec: ffi::OiLabelSummarySpec, filter: Option<&ffi::OiDocFilter>)
                         -> Result<Vec<Vec<(u32, ffi::OiSocialCounters)>>, HipError> {
        assert_eq!(labels.len(), self.n_docs);
        let k = (n_clusters as usize).max(1);
        let ranked = spec.top != 0;
        let width = if ranked { spec.top.clamp(1, 1024) as usize } else { (spec.n_cells as usize).clamp(1, (1usize << 20) / k) };
        let mut rec = vec![ffi::OiSocialCounters::default(); k * width];
        let (mut keys, mut counts) = (vec![u32::MAX; if ranked { k * width } else { 0 }], vec![0u32; if ranked { k } else { 0 }]);
        check(unsafe {
            ffi::oi_label_summary(self.idx, labels.as_ptr(), n_clusters, &spec,
                                  filter.map_or(std::ptr::null(), |f| f as *const ffi::OiDocFilter), ffi::OI_HOST, rec.as_mut_ptr(),
                                  if ranked { keys.as_mut_ptr() } else { std::ptr::null_mut() },
                                  if ranked { counts.as_mut_ptr() } else { std::ptr::null_mut() }, std::ptr::null_mut())
        })?;
        Ok((0..n_clusters as usize)
            .map(|c| {
                let n = if ranked { counts[c] as usize } else { width };
                (0..n).map(|i| (if ranked { keys[c * width + i] } else { i as u32 }, rec[c * width + i])).collect()
            })
            .collect())
    }
    /// Which narratives are there (`oi_narratives_fit`): k-means over the index on the device, from `seeds` ([k * dim]).
    /// Returns the centroids, records and (with `labels`) labels of the LAST assignment step and what the loop did;
    /// `similar_share` with the centroids as queries reproduces records and labels bit for bit.
    pub fn fit_narratives(&self, seeds: &[f32], spec: ffi::OiNarrativeSpec, filter: Option<ffi::OiDocFilter>, labels: bool)
                          -> Result<(Vec<f32>, Vec<Vec<ffi::OiSocialCounters>>, Option<Vec<u32>>, ffi::OiNarrativeInfo), HipError> {
        assert_eq!(seeds.len() % self.dim, 0);
        let k = seeds.len() / self.dim;
        let nb = spec.n_buckets as usize;
        let mut cent = vec![0f32; k * self.dim];
        let mut rec = vec![ffi::OiSocialCounters::default(); k * nb];
        let mut lab = if labels { Some(vec![u32::MAX; self.n_docs]) } else { None };
        let mut info = ffi::OiNarrativeInfo::default();
        check(unsafe {
            ffi::oi_narratives_fit(self.idx, seeds.as_ptr(), k as u32, &spec, filter.as_ref().map_or(std::ptr::null(), |f| f as *const _),
                                   ffi::OI_HOST, cent.as_mut_ptr(), rec.as_mut_ptr(),
                                   lab.as_mut().map_or(std::ptr::null_mut(), |l| l.as_mut_ptr()), &mut info)
        })?;
        Ok((cent, rec.chunks(nb.max(1)).map(|c| c.to_vec()).collect(), lab, info))
    }
    /// Seeds for `fit_narratives`, chosen on the device (`oi_narratives_seed`): `n_clusters` stored rows of the index by greedy
    /// k-means++ (the best of `spec.trials` D^2-sampled candidates per seed) or farthest-first, among the rows that pass
    /// `filter` and have a bucket.  Returns the seed vectors ([n_clusters * dim], zeros at and beyond `info.found`), their local
    /// rows (`u32::MAX` there) and {found, eligible, potential}.  A function of the arguments alone.
    pub fn seed_narratives(&self, n_clusters: u32, spec: ffi::OiSeedSpec, filter: Option<ffi::OiDocFilter>)
                           -> Result<(Vec<f32>, Vec<u32>, ffi::OiSeedInfo), HipError> {
        let k = n_clusters as usize;
        let mut seeds = vec![0f32; k.max(1) * self.dim];
        let mut rows = vec![u32::MAX; k.max(1)];
        let mut info = ffi::OiSeedInfo::default();
        check(unsafe {
            ffi::oi_narratives_seed(self.idx, n_clusters, &spec, filter.as_ref().map_or(std::ptr::null(), |f| f as *const _),
                                    ffi::OI_HOST, seeds.as_mut_ptr(), rows.as_mut_ptr(), &mut info)
        })?;
        Ok((seeds, rows, info))
    }
    /// Which group keys (tickers) the posts like each query are about, and what those posts feel (`oi_similar_groups`): the
    /// social_summary sums per key = (group & key_mask) >> ctz(key_mask), under `similar_summary`'s clauses.  spec.top == 0: per
    /// query `n_keys` records, keys implied (entry i is (i, record i)).  spec.top >= 1: per query the listed (key, record) pairs,
    /// best first by spec.rank_by, ties by key; the second value is the number of keys that qualified before the cut.
    pub fn similar_groups(&self, query_vecs: &[f32], spec: ffi::OiGroupsSpec, thresholds: Option<&[f32]>,
                          filters: Option<&[ffi::OiDocFilter]>)
                          -> Result<Vec<(Vec<(u32, ffi::OiSocialCounters)>, u32)>, HipError> {
        assert_eq!(query_vecs.len() % self.dim, 0);
        let b = query_vecs.len() / self.dim;
        if let Some(f) = filters {
            assert_eq!(f.len(), b);
        }
        if let Some(t) = thresholds {
            assert_eq!(t.len(), b);
        }
        let ranked = spec.top > 0;
        let per_q = (if ranked { spec.top } else { spec.n_keys }) as usize;
        let mut records = vec![ffi::OiSocialCounters::default(); b * per_q];
        let (mut keys, mut counts, mut qualified) = (vec![0u32; if ranked { b * per_q } else { 0 }], vec![0u32; b], vec![0u32; b]);
        check(unsafe {
            ffi::oi_similar_groups(self.idx, query_vecs.as_ptr(), b as u32, &spec, thresholds.map_or(std::ptr::null(), |t| t.as_ptr()),
                                   filters.map_or(std::ptr::null(), |f| f.as_ptr()), ffi::OI_HOST, records.as_mut_ptr(),
                                   if ranked { keys.as_mut_ptr() } else { std::ptr::null_mut() },
                                   if ranked { counts.as_mut_ptr() } else { std::ptr::null_mut() },
                                   if ranked { qualified.as_mut_ptr() } else { std::ptr::null_mut() })
        })?;
        Ok((0..b)
            .map(|q| {
                let m = if ranked { counts[q] as usize } else { per_q };
                let list = (0..m).map(|i| (if ranked { keys[q * per_q + i] } else { i as u32 }, records[q * per_q + i])).collect();
                (list, if ranked { qualified[q] } else { per_q as u32 })
            })
            .collect())
    }
    /// Hybrid BM25 + cosine + RRF: one ranked list (<= k) per query, in query order.
    pub fn search(&self, query_vecs: &[f32], query_terms: &[Vec<u32>], k: usize, depth: usize) -> Result<Vec<Vec<RankedPost>>, HipError> {
        let b = query_terms.len();
        assert_eq!(query_vecs.len(), b * self.dim);
        let mut flat = Vec::new();
        let mut offs = vec![0u32];
        for t in query_terms {
            flat.extend_from_slice(t);
            offs.push(flat.len() as u32);
        }
        if flat.is_empty() {
            flat.push(0);
        }
        let (mut s, mut d, mut c) = (vec![0f32; b * k], vec![0u32; b * k], vec![0u32; b]);
        check(unsafe {
            ffi::oi_search(self.idx, query_vecs.as_ptr(), flat.as_ptr(), offs.as_ptr(), b as u32, depth as u32, k as u32,
                           ffi::OI_HOST, s.as_mut_ptr(), d.as_mut_ptr(), c.as_mut_ptr())
        })?;
        let _ = (&self.ctx, &self.source);
        Ok((0..b)
            .map(|q| (0..c[q] as usize).map(|i| RankedPost { doc_id: d[q * k + i], score: s[q * k + i] }).collect())
            .collect())
    }
}

/// An RCCL communicator owned by the library (`oi_comm`): the multi-GPU exchange for a host that brings no collective
/// library of its own -- the reference is single-process (src/domain/ports/mod.rs:1-8), its composition root
/// (src/main.rs:17-39) would start one process per GPU and ship the 128-byte id over any channel it likes.
pub struct HipComm {
    ctx: Arc<HipCtx>,
    comm: *mut ffi::OiComm,
    pub rank: u32,
    pub world: u32,
}
unsafe impl Send for HipComm {}
impl Drop for HipComm {
    fn drop(&mut self) {
        unsafe { ffi::oi_comm_destroy(self.comm) }
    }
}
impl HipComm {
    /// Rank 0 only; every rank passes the same bytes to `create`.
    pub fn unique_id() -> Result<[u8; ffi::OI_COMM_ID_BYTES], HipError> {
        let mut id = [0u8; ffi::OI_COMM_ID_BYTES];
        check(unsafe { ffi::oi_comm_unique_id(id.as_mut_ptr()) })?;
        Ok(id)
    }
    /// Collective: returns when every rank of `world` has called it.
    pub fn create(ctx: Arc<HipCtx>, id: &[u8; ffi::OI_COMM_ID_BYTES], rank: u32, world: u32) -> Result<Self, HipError> {
        let mut comm = std::ptr::null_mut();
        check(unsafe { ffi::oi_comm_create(ctx.raw(), id.as_ptr(), rank, world, &mut comm) })?;
        Ok(HipComm { ctx, comm, rank, world })
    }
}

impl HipIndex {
    /// One rank's row shard of a collection split over `comm.world` GPUs: rows [doc_id_base, doc_id_base + n) of the
    /// global collection.  Collective (the df / N / token all-reduce runs inside `oi_index_finalize_sharded`).
    pub fn build_shard(comm: &HipComm, doc_id_base: u32, rows: &mut [f32], dim: usize, vocab: u32, terms: &[u32],
                       offsets: &[u64]) -> Result<Self, HipError> {
        let n_docs = (rows.len() / dim) as u64;
        let mut idx = std::ptr::null_mut();
        check(unsafe { ffi::oi_index_create(comm.ctx.raw(), n_docs, dim as u32, vocab, doc_id_base, &mut idx) })?;
        let me = HipIndex { ctx: comm.ctx.clone(), idx, dim, n_docs: n_docs as usize, source: None };
        check(unsafe { ffi::oi_index_set_embeddings(me.idx, rows.as_mut_ptr(), ffi::OI_HOST, 1) })?;
        check(unsafe { ffi::oi_index_set_forward(me.idx, terms.as_ptr(), offsets.as_ptr(), ffi::OI_HOST) })?;
        check(unsafe { ffi::oi_index_finalize_sharded(me.idx, comm.comm) })?;
        Ok(me)
    }
    /// `search_sharded` with one doc filter per query: each rank filters its own shard; merge and fusion unchanged.
    pub fn search_sharded_filtered(&self, comm: &HipComm, query_vecs: &[f32], query_terms: &[Vec<u32>],
                                   filters: &[ffi::OiDocFilter], k: usize, depth: usize) -> Result<Vec<Vec<RankedPost>>, HipError> {
        let b = query_terms.len();
        assert_eq!(query_vecs.len(), b * self.dim);
        assert_eq!(filters.len(), b);
        let (flat, offs) = flatten_terms(query_terms);
        let (mut s, mut d, mut c) = (vec![0f32; b * k], vec![0u32; b * k], vec![0u32; b]);
        check(unsafe {
            ffi::oi_search_sharded_filtered(self.idx, comm.comm, query_vecs.as_ptr(), flat.as_ptr(), offs.as_ptr(), b as u32,
                                            depth as u32, k as u32, filters.as_ptr(), ffi::OI_HOST, s.as_mut_ptr(),
                                            d.as_mut_ptr(), c.as_mut_ptr())
        })?;
        Ok(ranked(&s, &d, &c, k))
    }
    /// The hybrid query over ALL shards (collective, same queries on every rank, one ncclAllGather per batch inside):
    /// identical lists on every rank, global doc ids.
    pub fn search_sharded(&self, comm: &HipComm, query_vecs: &[f32], query_terms: &[Vec<u32>], k: usize, depth: usize)
                          -> Result<Vec<Vec<RankedPost>>, HipError> {
        let b = query_terms.len();
        assert_eq!(query_vecs.len(), b * self.dim);
        let mut flat = Vec::new();
        let mut offs = vec![0u32];
        for t in query_terms {
            flat.extend_from_slice(t);
            offs.push(flat.len() as u32);
        }
        if flat.is_empty() {
            flat.push(0);
        }
        let (mut s, mut d, mut c) = (vec![0f32; b * k], vec![0u32; b * k], vec![0u32; b]);
        check(unsafe {
            ffi::oi_search_sharded(self.idx, comm.comm, query_vecs.as_ptr(), flat.as_ptr(), offs.as_ptr(), b as u32,
                                   depth as u32, k as u32, ffi::OI_HOST, s.as_mut_ptr(), d.as_mut_ptr(), c.as_mut_ptr())
        })?;
        Ok((0..b)
            .map(|q| (0..c[q] as usize).map(|i| RankedPost { doc_id: d[q * k + i], score: s[q * k + i] }).collect())
            .collect())
    }
}

/// Several batches in flight through lanes the LIBRARY owns (oi_pipeline_*): the throughput form of `search` /
/// `search_sharded` for a host without streams of its own.  Results are bit-identical to the one-call forms.
pub struct HipPipeline {
    p: *mut ffi::OiPipeline,
    dim: usize,
    k: usize,
    _idx: Arc<HipIndex>,
}
unsafe impl Send for HipPipeline {}
impl Drop for HipPipeline {
    fn drop(&mut self) {
        unsafe { ffi::oi_pipeline_destroy(self.p) } // drains first
    }
}
/// The owned output buffers of one submitted batch; filled when `HipPipeline::wait(ticket)` returns.
pub struct PendingBatch {
    pub ticket: u64,
    n: usize,
    scores: Vec<f32>,
    docs: Vec<u32>,
    counts: Vec<u32>,
}
impl HipPipeline {
    /// `comm`: None = one shard, no exchange; Some = row-sharded, ONE ncclAllGather per batch inside the library.
    pub fn create(idx: Arc<HipIndex>, comm: Option<&HipComm>, lanes: u32, max_queries: u32, max_query_terms: u32, depth: u32, k: u32)
                  -> Result<Self, HipError> {
        let mut p = std::ptr::null_mut();
        let c = comm.map(|c| c.comm).unwrap_or(std::ptr::null_mut());
        check(unsafe { ffi::oi_pipeline_create(idx.idx, c, lanes, max_queries, max_query_terms, depth, k, &mut p) })?;
        Ok(Self { p, dim: idx.dim, k: k as usize, _idx: idx })
    }
    /// Asynchronous: the inputs are copied during the call, the returned buffers are written by `wait`.
    pub fn submit(&self, query_vecs: &[f32], query_terms: &[Vec<u32>]) -> Result<PendingBatch, HipError> {
        let b = query_terms.len();
        assert_eq!(query_vecs.len(), b * self.dim);
        let mut flat = Vec::new();
        let mut offs = vec![0u32];
        for t in query_terms {
            flat.extend_from_slice(t);
            offs.push(flat.len() as u32);
        }
        if flat.is_empty() {
            flat.push(0);
        }
        let mut out = PendingBatch { ticket: 0, n: b, scores: vec![0f32; b * self.k], docs: vec![0u32; b * self.k], counts: vec![0u32; b] };
        check(unsafe {
            ffi::oi_pipeline_submit(self.p, query_vecs.as_ptr(), flat.as_ptr(), offs.as_ptr(), b as u32, ffi::OI_HOST,
                                    out.scores.as_mut_ptr(), out.docs.as_mut_ptr(), out.counts.as_mut_ptr(), &mut out.ticket)
        })?;
        Ok(out) // (the Vecs' heap buffers do not move with the struct: the library's pointers stay valid until wait)
    }
    pub fn wait(&self, batch: PendingBatch) -> Result<Vec<Vec<RankedPost>>, HipError> {
        check(unsafe { ffi::oi_pipeline_wait(self.p, batch.ticket, 1) })?;
        let k = self.k;
        Ok((0..batch.n)
            .map(|q| (0..batch.counts[q] as usize).map(|i| RankedPost { doc_id: batch.docs[q * k + i], score: batch.scores[q * k + i] }).collect())
            .collect())
    }
    pub fn drain(&self) -> Result<(), HipError> {
        check(unsafe { ffi::oi_pipeline_drain(self.p) })
    }
}

/// The adapter for the reference: `impl PostAnalyzer for HipLexiconAnalyzer`.
#[cfg(feature = "reference")]
pub mod adapter {
    use super::*;
    use async_trait::async_trait;
    use openintel::domain::entities::social_post::SocialPost;
    use openintel::domain::error::DomainError;
    use openintel::domain::ports::post_analyzer::PostAnalyzer;
    use openintel::domain::values::{polarity::Polarity, post_signal::PostSignal};

    fn fail(e: HipError) -> DomainError {
        // nonzero status -> DomainError::SourceFailure (src/domain/error.rs:16-17)
        DomainError::SourceFailure { name: "hip-analyzer".into(), message: e.to_string() }
    }

    pub struct HipLexiconAnalyzer {
        ctx: Arc<HipCtx>,
    }
    impl HipLexiconAnalyzer {
        pub fn new(device: i32) -> Result<Self, DomainError> {
            Ok(Self { ctx: HipCtx::new(device).map_err(fail)? })
        }
    }

    #[async_trait]
    impl PostAnalyzer for HipLexiconAnalyzer {
        /// One PostSignal per post, aligned to input order (post_analyzer.rs:9).
        async fn analyze(&self, posts: &[SocialPost]) -> Result<Vec<PostSignal>, DomainError> {
            let (blob, offsets) = gather(posts.iter().map(|p| p.text.as_str()));
            let n = posts.len();
            let ctx = self.ctx.clone();
            // The call blocks (H2D copy, kernel, D2H copy): keep it off the async workers.  The reference impl is an
            // async fn without an await point (lexicon.rs:84-86), so the semantics are unchanged.
            tokio::task::spawn_blocking(move || {
                let (mut pol, mut spec) = (vec![0f64; n], vec![0u8; n]);
                check(unsafe {
                    ffi::oi_lexicon_analyze(ctx.raw(), blob.as_ptr(), offsets.as_ptr(), n as u64, pol.as_mut_ptr(), spec.as_mut_ptr())
                })
                .map_err(fail)?;
                Ok(pol
                    .into_iter()
                    .zip(spec)
                    .map(|(p, s)| PostSignal { polarity: Polarity::new(p), speculative: s != 0 })
                    .collect())
            })
            .await
            .map_err(|e| DomainError::SourceFailure { name: "hip-analyzer".into(), message: e.to_string() })?
        }
    }
}
