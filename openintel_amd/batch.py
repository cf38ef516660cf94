"""The batch callers of the PostAnalyzer path ("the only batch entry").

Host mirror of the reference's batch tools (paths relative to the openintel repo):

    run_list_sources                               src/mcp/tools.rs:23-37
    request_from                                   src/mcp/tools.rs:71-96
    summarize                                      src/mcp/tools.rs:99-108
    AnalyzeOutput / run_analyze (no dip deps)      src/mcp/tools.rs:53-66, 110-162
    ScanArgs / ScanEntry / ScanOutput / run_scan   src/mcp/tools.rs:163-225
    RankBy / CompareArgs / RankedEntry / CompareError / CompareOutput
    rank_metric / sort_ranked / run_compare        src/mcp/tools.rs:227-352
    rank_group_records / compare_index             src/mcp/tools.rs:323-349 over the index's per-ticker sums (oi_similar_groups)
    compare_mentions                               the same over the posts that CONTAIN a text's terms (oi_mention_summary, key axis)
    VoiceShare / share_of_voice                    builder-defined: the records of oi_similar_share as fractions per bucket
    discover_narratives                            builder-defined: oi_narratives_fit and the share of voice of what it found
    SentimentSummary / sentiment_for (per dip row) src/domain/dip.rs:428-431, src/application/dip.rs:175-194

The reference runs `application::analyze` once per ticker (`join_all`, tools.rs:206-220) and never pools posts of
different tickers: each ticker's few dozen posts go through their own `LexiconAnalyzer::analyze`.  On the GPU the batch
IS the unit of work, so here the posts of ALL tickers of a call go through ONE analyzer call (one scan launch), and --
when the analyzer offers it (`HipLexiconAnalyzer.analyze_segments`) -- every ticker's `social_summary` sums come from one
segmented reduction on the device (`oi_social_summary_segmented`: the reference's input-order f64 sum per ticker, bit for
bit).  The reports are the ones `analyze` would have produced ticker by ticker: same posts, same notes, same numbers
(tests/test_batch.py compares them byte for byte); entries keep the input order (join_all keeps positions).

One difference follows from pooling and is deliberate: an analyzer FAILURE (a device error) fails every ticker that had
posts in the pooled call, each with the same message, where the reference would fail them one by one.  The transport
around these functions (the MCP server, JSON-RPC, tool schemas: src/mcp/server.rs) is control plane and out of scope.
"""
from __future__ import annotations

import datetime as _dt
import enum
import functools
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

from .analyzer import PostAnalyzer, counters_record
from .application import (DISCLAIMER, AnalysisRequest, MarketDataSource, SocialDataSource, _debug_name, _json_f64,
                          _pretty, _Raw, gather, report_to_wire)
from .domain import Alignment, AnalyzerMismatch, DomainError, EngineConfig, SourceKind, SpeculationReport, Ticker
from .engine import SpeculationEngine


# ----------------------------------------------------------------------------- shared by the tools
def request_from(ticker: str, enable_reddit: Optional[bool] = None, enable_bluesky: Optional[bool] = None,
                 no_market: Optional[bool] = None, limit: Optional[int] = None) -> AnalysisRequest:
    """tools.rs:71-96: no source flag set -> every source; limit 50; market on unless `no_market`."""
    enabled: List[SourceKind] = []
    if enable_reddit:
        enabled.append(SourceKind.REDDIT)
    if enable_bluesky:
        enabled.append(SourceKind.BLUESKY)
    if not enabled:
        enabled = list(SourceKind.ALL)
    return AnalysisRequest(ticker=ticker, enabled_sources=enabled, market_enabled=not bool(no_market),
                           limit=50 if limit is None else limit, engine=EngineConfig())


def summarize(report: SpeculationReport) -> str:
    """tools.rs:99-108: `{} — {:?} · crowding {:.0}% · {} mentions ({:?})`."""
    return "%s — %s · crowding %.0f%% · %d mentions (%s)" % (
        report.ticker.as_str(), _debug_name(report.fusion.alignment), report.fusion.crowding * 100.0,
        report.social.total_mentions, _debug_name(report.social_confidence))


# ----------------------------------------------------------------------------- list_sources / analyze_ticker
def run_list_sources(social_sources: Sequence[SocialDataSource], market_source: MarketDataSource) -> dict:
    """tools.rs:23-37: the data sources actually wired (`social` reflects the injected list, not SourceKind::ALL)."""
    return {"social": [s.kind().as_str() for s in social_sources], "market": [market_source.name()]}


@dataclass
class AnalyzeOutput:  # tools.rs:53-66; dip_signal / dip_note need the dip dependencies (bars, filings, news: out of scope)
    summary: str
    report: SpeculationReport
    dip_signal: Optional[object] = None
    dip_note: Optional[str] = None
    disclaimer: str = DISCLAIMER


def run_analyze(ticker: str, social_sources: Sequence[SocialDataSource], market_source: MarketDataSource,
                analyzer: PostAnalyzer, enable_reddit: Optional[bool] = None, enable_bluesky: Optional[bool] = None,
                no_market: Optional[bool] = None, limit: Optional[int] = None,
                now: Optional[_dt.datetime] = None) -> AnalyzeOutput:
    """tools.rs:110-162 without the dip attachment (`dip_deps = None`: the reference's own default in its tests, :676-696):
    one ticker, the report and its one-line gloss.  Raises the DomainError the reference returns as Err."""
    from .application import analyze
    req = request_from(ticker, enable_reddit, enable_bluesky, no_market, limit)
    report = analyze(req, social_sources, market_source, analyzer, now=now)
    return AnalyzeOutput(summary=summarize(report), report=report)


# ----------------------------------------------------------------------------- the pooled analysis
def analyze_many(requests: Sequence[AnalysisRequest], social_sources: Sequence[SocialDataSource],
                 market_source: Optional[MarketDataSource], analyzer: PostAnalyzer,
                 now: Optional[_dt.datetime] = None) -> List[object]:
    """`application::analyze` for every request, with ONE analyzer call for the posts of all of them.

    Returns, per request and in order, the SpeculationReport or the DomainError the reference's analyze would have
    returned for it."""
    if now is None:
        now = _dt.datetime.now(_dt.timezone.utc)
    results: List[object] = [None] * len(requests)
    pending = []  # (position, request, ticker, posts, market, notes)
    for i, req in enumerate(requests):
        try:
            ticker, posts, market, notes = gather(req, social_sources, market_source)  # analyze.rs:21-60
        except DomainError as e:
            results[i] = e
            continue
        pending.append((i, req, ticker, posts, market, notes))
    if not pending:
        return results

    segments = [p[3] for p in pending]
    counters = None
    try:
        if hasattr(analyzer, "analyze_segments"):
            # one scan + one reduction per ticker on the device; every request_from config has the same threshold,
            # a caller mixing thresholds gets the host sums below
            taus = {p[1].engine.bull_bear_threshold for p in pending}
            if len(taus) == 1:
                per_segment, counters = analyzer.analyze_segments(segments, tau=taus.pop())
        if counters is None:
            flat = [post for seg in segments for post in seg]
            signals = analyzer.analyze(flat)  # analyze.rs:61-62 -- the hot path, once for the whole batch
            if len(signals) != len(flat):  # speculation_engine.rs:29-34, for the pooled call
                raise AnalyzerMismatch(expected=len(flat), got=len(signals))
            per_segment, at = [], 0
            for seg in segments:
                per_segment.append(signals[at:at + len(seg)])
                at += len(seg)
    except DomainError as e:  # the pooled call failed: every ticker in it fails the same way
        for p in pending:
            results[p[0]] = e
        return results

    for k, (i, req, ticker, posts, market, notes) in enumerate(pending):
        try:
            if counters is not None:
                if int(counters[k]["total"]) != len(posts):
                    raise AnalyzerMismatch(expected=len(posts), got=int(counters[k]["total"]))
                report = SpeculationEngine.aggregate_counters(ticker, counters_record(counters[k]), market, now, req.engine)
            else:
                report = SpeculationEngine.aggregate(ticker, posts, per_segment[k], market, now, req.engine)
            report.fusion.notes = notes + report.fusion.notes  # analyze.rs:68-69 request notes first
            results[i] = report
        except DomainError as e:
            results[i] = e
    return results


# ----------------------------------------------------------------------------- the dip screen's sentiment step
SOCIAL_LIMIT = 50  # application/dip.rs:44


@dataclass
class SentimentSummary:  # domain/dip.rs:428-431
    net_sentiment: float
    mentions: int


def sentiments_for(tickers: Sequence[str], social_sources: Sequence[SocialDataSource], analyzer: PostAnalyzer,
                   now: Optional[_dt.datetime] = None) -> List[Optional[SentimentSummary]]:
    """`sentiment_for` (application/dip.rs:175-194) for every row of a dip scan at once: the social-only analysis the
    screen runs per loser (all sources, no market, limit 50), pooled like run_scan.  Any failure -- no sources, an invalid
    ticker, no posts -- degrades to None, as in the reference (the domain then scores divergence 0 with a note)."""
    if not social_sources:
        return [None] * len(tickers)
    reqs = [AnalysisRequest(ticker=t, enabled_sources=list(SourceKind.ALL), market_enabled=False, limit=SOCIAL_LIMIT,
                            engine=EngineConfig()) for t in tickers]
    out: List[Optional[SentimentSummary]] = []
    for res in analyze_many(reqs, social_sources, None, analyzer, now):
        out.append(None if isinstance(res, DomainError) else
                   SentimentSummary(net_sentiment=float(res.social.net_sentiment), mentions=int(res.social.total_mentions)))
    return out


# ----------------------------------------------------------------------------- scan_watchlist
@dataclass
class ScanArgs:  # tools.rs:163-175
    tickers: List[str]
    enable_reddit: Optional[bool] = None
    enable_bluesky: Optional[bool] = None
    no_market: Optional[bool] = None
    limit: Optional[int] = None


@dataclass
class ScanEntry:  # tools.rs:177-184
    ticker: str
    report: Optional[SpeculationReport] = None
    error: Optional[str] = None


@dataclass
class ScanOutput:  # tools.rs:186-190
    entries: List[ScanEntry]
    disclaimer: str = DISCLAIMER


def run_scan(args: ScanArgs, social_sources: Sequence[SocialDataSource], market_source: MarketDataSource,
             analyzer: PostAnalyzer, now: Optional[_dt.datetime] = None) -> ScanOutput:
    """tools.rs:193-225.  One entry per input ticker, in input order: the report, or the error's Display string."""
    reqs = [request_from(t, args.enable_reddit, args.enable_bluesky, args.no_market, args.limit) for t in args.tickers]
    entries = []
    for t, res in zip(args.tickers, analyze_many(reqs, social_sources, market_source, analyzer, now)):
        if isinstance(res, DomainError):
            entries.append(ScanEntry(ticker=t, error=str(res)))
        else:
            entries.append(ScanEntry(ticker=t, report=res))
    return ScanOutput(entries=entries)


# ----------------------------------------------------------------------------- compare_tickers
class RankBy(enum.Enum):  # tools.rs:227-238, serde snake_case
    CROWDING = "crowding"
    SPECULATION_INDEX = "speculation_index"
    NET_SENTIMENT = "net_sentiment"
    DIVERGENCE = "divergence"


@dataclass
class CompareArgs:  # tools.rs:240-251
    tickers: List[str]
    rank_by: RankBy = RankBy.CROWDING
    enable_reddit: Optional[bool] = None
    enable_bluesky: Optional[bool] = None
    no_market: Optional[bool] = None
    limit: Optional[int] = None


@dataclass
class RankedEntry:  # tools.rs:253-258
    ticker: str
    rank_metric: float
    report: SpeculationReport


@dataclass
class CompareError:  # tools.rs:260-264
    ticker: str
    error: str


@dataclass
class CompareOutput:  # tools.rs:266-272
    rank_by: RankBy
    ranked: List[RankedEntry]
    errors: List[CompareError]
    disclaimer: str = DISCLAIMER


def rank_metric(report: SpeculationReport, rank_by: RankBy) -> float:
    """tools.rs:274-283: `divergence` ranks categorically first, its numeric metric is crowding."""
    if rank_by in (RankBy.CROWDING, RankBy.DIVERGENCE):
        return float(report.fusion.crowding)
    if rank_by is RankBy.SPECULATION_INDEX:
        return float(report.social.speculation_index)
    return float(report.social.net_sentiment)


def _desc_partial(a: float, b: float) -> int:
    # b.partial_cmp(&a).unwrap_or(Equal): descending, an unordered pair (NaN) compares equal
    if math.isnan(a) or math.isnan(b):
        return 0
    return -1 if b < a else (1 if b > a else 0)


def sort_ranked(ranked: List[RankedEntry], rank_by: RankBy) -> None:
    """tools.rs:285-301, in place; `sort_by` is stable and so is this."""
    def cmp(a: RankedEntry, b: RankedEntry) -> int:
        if rank_by is RankBy.DIVERGENCE:
            a_div = a.report.fusion.alignment is Alignment.DIVERGING
            b_div = b.report.fusion.alignment is Alignment.DIVERGING
            if a_div != b_div:  # b_div.cmp(&a_div): diverging first
                return -1 if a_div else 1
        return _desc_partial(a.rank_metric, b.rank_metric)
    ranked.sort(key=functools.cmp_to_key(cmp))


def run_compare(args: CompareArgs, social_sources: Sequence[SocialDataSource], market_source: MarketDataSource,
                analyzer: PostAnalyzer, now: Optional[_dt.datetime] = None) -> CompareOutput:
    """tools.rs:303-352: valid tickers ranked, invalid ones listed, both in input order before the (stable) sort."""
    reqs = [request_from(t, args.enable_reddit, args.enable_bluesky, args.no_market, args.limit) for t in args.tickers]
    ranked: List[RankedEntry] = []
    errors: List[CompareError] = []
    for t, res in zip(args.tickers, analyze_many(reqs, social_sources, market_source, analyzer, now)):
        if isinstance(res, DomainError):
            errors.append(CompareError(ticker=t, error=str(res)))
        else:
            ranked.append(RankedEntry(ticker=t, rank_metric=rank_metric(res, args.rank_by), report=res))
    sort_ranked(ranked, args.rank_by)
    return CompareOutput(rank_by=args.rank_by, ranked=ranked, errors=errors)


# ----------------------------------------------------------------------------- compare over the index (oi_similar_groups)
def rank_group_records(keys, records, count: int, tickers, rank_by: RankBy, market_by_ticker=None,
                       now: Optional[_dt.datetime] = None, cfg: EngineConfig = EngineConfig()) -> CompareOutput:
    """tools.rs:323-349 over the ranked output of one query of `HybridIndex.similar_groups`: the first `count` entries of
    `keys` / `records` (analyzer.COUNTERS_DTYPE) are the tickers' raw social_summary sums, already reduced on the device where
    the reference analyses each ticker's posts.  `tickers` names the keys (a sequence indexed by key, or a mapping); each
    listed key gives `SpeculationEngine.aggregate_counters(ticker, record, market, now, cfg)` with `market_by_ticker`'s
    snapshot for that name (none: a social-only report), then a RankedEntry with `rank_metric`, in the device's order before
    the stable `sort_ranked`.  A key without a name, an invalid name or a mismatching market snapshot goes to `errors`."""
    if now is None:
        now = _dt.datetime.now(_dt.timezone.utc)
    markets = market_by_ticker or {}
    ranked: List[RankedEntry] = []
    errors: List[CompareError] = []
    for r in range(int(count)):
        key = int(keys[r])
        if isinstance(tickers, dict):
            name = tickers.get(key)
        else:
            name = tickers[key] if 0 <= key < len(tickers) else None
        if name is None:
            errors.append(CompareError(ticker="#%d" % key, error="group key %d has no ticker name" % key))
            continue
        try:
            report = SpeculationEngine.aggregate_counters(Ticker.parse(name), counters_record(records[r]), markets.get(name), now, cfg)
        except DomainError as e:
            errors.append(CompareError(ticker=name, error=str(e)))
            continue
        ranked.append(RankedEntry(ticker=name, rank_metric=rank_metric(report, rank_by), report=report))
    sort_ranked(ranked, rank_by)
    return CompareOutput(rank_by=rank_by, ranked=ranked, errors=errors)


def compare_index(index, query_vec, threshold: float, tickers, key_mask: int, rank_by: RankBy = RankBy.CROWDING, top: int = 100,
                  min_total: Optional[int] = None, filters=None, n_keys: Optional[int] = None, market_by_ticker=None,
                  now: Optional[_dt.datetime] = None, cfg: EngineConfig = EngineConfig()) -> CompareOutput:
    """compare_tickers answered from the index: "which tickers are the posts like this query about, and what do they feel?"
    ONE ranked `similar_groups` call by total for the single query `query_vec` (the `top` most-mentioned tickers with at least
    `min_total` posts, default `cfg.min_sample`), then `rank_group_records`.  n_keys defaults to the number of names (a
    mapping: its largest key + 1).  The index's signals must have been set with `cfg.bull_bear_threshold`."""
    import numpy as np
    if n_keys is None:
        n_keys = (max(tickers) + 1) if isinstance(tickers, dict) else len(tickers)
    q = np.ascontiguousarray(np.asarray(query_vec, dtype=np.float32).reshape(1, -1))
    res = index.similar_groups(q, float(threshold), int(key_mask), int(n_keys), top=int(top), rank_by="total",
                               min_total=int(cfg.min_sample if min_total is None else min_total), filters=filters)
    return rank_group_records(res.keys[0], res.records[0], int(res.counts[0]), tickers, rank_by, market_by_ticker, now, cfg)


def compare_mentions(index, text: str, tickers, key_mask: int, rank_by: RankBy = RankBy.CROWDING, top: int = 100,
                     min_total: Optional[int] = None, min_match=None, filters=None, n_keys: Optional[int] = None,
                     market_by_ticker=None, now: Optional[_dt.datetime] = None, cfg: EngineConfig = EngineConfig()) -> CompareOutput:
    """compare_tickers answered from the postings: "which tickers do the posts that MENTION this text belong to, and what do
    they feel?"  ONE dense `mention_groups_text` call for the single query `text` (no embeddings needed); the host keeps the
    keys with total >= max(min_total, 1) (default `cfg.min_sample`), orders them by (total descending, key ascending), cuts
    at `top`, then `rank_group_records` -- compare_index with the lexical match in the similarity's place.  n_keys defaults
    to the number of names (a mapping: its largest key + 1).  The index's signals must have been set with
    `cfg.bull_bear_threshold`."""
    from .analyzer import COUNTERS_DTYPE
    if n_keys is None:
        n_keys = (max(tickers) + 1) if isinstance(tickers, dict) else len(tickers)
    rec = index.mention_groups_text([text], int(key_mask), int(n_keys), min_match=min_match, filters=filters)
    if hasattr(rec, "data_ptr"):
        rec = rec.cpu().numpy().view(COUNTERS_DTYPE).reshape(rec.shape[0], rec.shape[1])
    rec = rec[0]
    bar = max(int(cfg.min_sample if min_total is None else min_total), 1)
    keys = sorted((k for k in range(len(rec)) if int(rec[k]["total"]) >= bar), key=lambda k: (-int(rec[k]["total"]), k))[:int(top)]
    return rank_group_records(keys, [rec[k] for k in keys], len(keys), tickers, rank_by, market_by_ticker, now, cfg)


# ----------------------------------------------------------------------------- share of voice (oi_similar_share)
@dataclass
class VoiceShare:  # builder-defined (the reference divides no posts among narratives)
    total: int                 # posts assigned to the query in the bucket
    fraction: float            # total / the bucket's assigned posts over all queries; 0.0 in a bucket without any
    social: "object"           # SocialSummary of the assigned posts (SpeculationEngine.social_from_counters)


def share_of_voice(records) -> List[List[VoiceShare]]:
    """Each query's share of the posts `HybridIndex.similar_share` assigned, per bucket: `records` is its [B, n_buckets]
    array (analyzer.COUNTERS_DTYPE; every post is in at most one cell, so a bucket's totals add up to its assigned posts).
    Entry [q][b] holds the query's total, its fraction of the bucket's total over all queries, and the SocialSummary of its
    posts.  A bucket no query has a post in gives fraction 0.0 everywhere."""
    B = len(records)
    nb = len(records[0]) if B else 0
    sums = [sum(int(records[q][b]["total"]) for q in range(B)) for b in range(nb)]
    return [[VoiceShare(total=int(records[q][b]["total"]),
                        fraction=(int(records[q][b]["total"]) / sums[b]) if sums[b] else 0.0,
                        social=SpeculationEngine.social_from_counters(records[q][b]))
             for b in range(nb)] for q in range(B)]


def discover_narratives(index, seeds, threshold, **kw):
    """Which narratives are there: `index.fit_narratives(seeds, threshold, **kw)` (k-means over the index on the device,
    oi_narratives_fit) and the share of voice of what it found -> (NarrativeFit, share_of_voice(fit.records)).  Entry
    [c][b] of the second is narrative c's share of the assigned posts in bucket b.  Records that live on the device
    (tensor seeds) are read back for it; the fit itself is returned as it came.
    `seeds` may also be an int: that many seeds are first chosen on the device by `index.seed_narratives` (oi_narratives_seed)
    among the rows the fit assigns from -- with the fit's `filter`, `n_buckets`, `stamp_origin` and `bucket_width`, and with
    `method`, `trials` and `seed` taken from kw (they do not reach the fit).  The seed vectors stay on the device when the
    index's rows were given as device tensors.
    What each narrative is ABOUT -- its distinguishing terms -- comes from `describe_narratives(index, fit)` (fit with labels=True)."""
    from .analyzer import COUNTERS_DTYPE
    import numbers
    if isinstance(seeds, numbers.Integral) and not isinstance(seeds, bool):
        skw = {k: kw.pop(k) for k in ("method", "trials", "seed") if k in kw}
        skw.update({k: kw[k] for k in ("filter", "n_buckets", "stamp_origin", "bucket_width") if k in kw})
        on_device = any(hasattr(t, "data_ptr") for t in getattr(index, "_keep", []))
        seeds = index.seed_narratives(int(seeds), device=on_device, **skw).seeds
    fit = index.fit_narratives(seeds, threshold, **kw)
    rec = fit.records
    if hasattr(rec, "data_ptr"):
        rec = rec.cpu().numpy().view(COUNTERS_DTYPE).reshape(rec.shape[0], rec.shape[1])
    return fit, share_of_voice(rec)


@dataclass
class NarrativeTerm:
    """One distinguishing term of a narrative: the term id (valid in query_terms of mention_summary and every search), the word
    a text sample names it with (None without a sample), df = the narrative's posts that hold it, df_assigned = the assigned
    posts that hold it, lift = (df / size of the narrative) / (df_assigned / assigned posts)."""
    term: int
    word: Optional[str]
    df: int
    df_assigned: int
    lift: float


def _term_words(index, texts):
    """id -> the most frequent token of `texts` that the library's own hash sends to it (ties: the smaller token)."""
    import collections
    import re
    import numpy as np
    from . import retriever
    freq = collections.Counter()
    for t in texts:
        freq.update(re.findall(r"[0-9a-z]+", t.lower()))
    tokens = sorted(freq)
    if not tokens:
        return {}
    ids, offs = retriever.text_terms(index.ctx, tokens, index.vocab)
    ids, offs = np.asarray(ids), np.asarray(offs)
    words = {}
    for i, tok in enumerate(tokens):
        if int(offs[i + 1]) - int(offs[i]) != 1:     # (the tokeniser cut it differently or dropped it: it names no single id)
            continue
        tid = int(ids[int(offs[i])])
        best = words.get(tid)
        if best is None or freq[tok] > freq[best]:   # (a collision is not an error: the more frequent token names the id)
            words[tid] = tok
    return words


def describe_narratives(index, fit_or_labels, n_clusters=None, top=10, min_df=1, texts=None):
    """What every narrative is about: per cluster, the list of its distinguishing terms as NarrativeTerm, best first
    (`index.label_terms`, oi_label_terms: one pass over the BM25 postings on the device, ranked by excess = A * (observed -
    expected posts of the cluster holding the term); the index must be finalized).
    fit_or_labels: a NarrativeFit made with labels=True (n_clusters is then its number of centroids), or a label array
    [n_docs] by local row (numpy or torch CUDA tensor) with n_clusters given.  texts: any sample of posts, or the corpus
    itself, to name the hashed ids with: it is lowercased and split into maximal [0-9a-z] runs, the distinct tokens go through
    retriever.text_terms with the index's vocab, and an id is named by the most frequent token that hashes to it."""
    from . import retriever
    labels = fit_or_labels
    if hasattr(fit_or_labels, "centroids") and hasattr(fit_or_labels, "labels"):
        labels = fit_or_labels.labels
        if labels is None:
            raise ValueError("describe_narratives: the fit carries no labels (fit_narratives(..., labels=True))")
        if n_clusters is None:
            n_clusters = int(fit_or_labels.centroids.shape[0])
    if n_clusters is None:
        raise ValueError("describe_narratives: n_clusters is required with a label array")
    rec, n, sizes = index.label_terms(labels, int(n_clusters), top=top, min_df=min_df)
    rec = retriever.label_term_records(rec)
    if hasattr(n, "data_ptr"):
        n, sizes = n.cpu().numpy(), sizes.cpu().numpy()
    words = _term_words(index, texts) if texts is not None else {}
    assigned = int(sum(int(x) for x in sizes))
    out = []
    for c in range(int(n_clusters)):
        terms = []
        for r in rec[c][:int(n[c])]:
            df, dfa = int(r["df_cluster"]), int(r["df_assigned"])
            lift = (df / int(sizes[c])) / (dfa / assigned) if int(sizes[c]) and dfa and assigned else 0.0
            terms.append(NarrativeTerm(int(r["term"]), words.get(int(r["term"])), df, dfa, lift))
        out.append(terms)
    return out


def narrative_exemplars(index, fit_or_labels, centroids=None, top=5, pool=64, collapse=None, texts=None):
    """The posts to quote for every narrative: per cluster a list of (doc, score, stands_for, text-or-None), best first -- the
    cluster's own posts closest to its centroid (`index.label_exemplars`, oi_label_exemplars).
    fit_or_labels: a NarrativeFit made with labels=True (the centroids are then the fit's), or a label array [n_docs] by local
    row (numpy or torch CUDA tensor) with `centroids` [n_clusters, dim] given.
    collapse=t: by definition label_exemplars(.., top=pool) followed by index.collapse_lists(.., threshold=t, k=top) -- retweets
    and copies of a post fold into its best-ranked copy, and stands_for is how many pool entries the kept post stands for.
    Without collapse: label_exemplars(.., top=top), stands_for = 1.  texts: the corpus's texts by GLOBAL doc id (a sequence
    or a mapping); None leaves the text None."""
    labels = fit_or_labels
    if hasattr(fit_or_labels, "centroids") and hasattr(fit_or_labels, "labels"):
        labels = fit_or_labels.labels
        if labels is None:
            raise ValueError("narrative_exemplars: the fit carries no labels (fit_narratives(..., labels=True))")
        if centroids is None:
            centroids = fit_or_labels.centroids
    if centroids is None:
        raise ValueError("narrative_exemplars: centroids are required with a label array")
    if collapse is None:
        lists = index.label_exemplars(labels, centroids, top=top)
        scores, docs, counts, dups = lists.cos_scores, lists.cos_docs, lists.cos_counts, None
    else:
        lists = index.label_exemplars(labels, centroids, top=pool)
        res = index.collapse_lists(lists.cos_scores, lists.cos_docs, lists.cos_counts, threshold=collapse, k=top)
        scores, docs, counts, dups = res.scores, res.docs, res.counts, res.dup_counts
    if hasattr(docs, "data_ptr"):
        import numpy as np
        scores, docs, counts = scores.cpu().numpy(), docs.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32)
        dups = None if dups is None else dups.cpu().numpy().view(np.uint32)

    def text_of(doc):
        if texts is None:
            return None
        if hasattr(texts, "get"):
            return texts.get(doc)
        return texts[doc] if 0 <= doc < len(texts) else None

    out = []
    for c in range(int(docs.shape[0])):
        out.append([(int(docs[c, i]), float(scores[c, i]), 1 if dups is None else int(dups[c, i]), text_of(int(docs[c, i])))
                    for i in range(int(counts[c]))])
    return out


def _narrative_labels(who, fit_or_labels, n_clusters):
    """(labels, n_clusters) of a NarrativeFit made with labels=True, or of a label array with n_clusters given."""
    labels = fit_or_labels
    if hasattr(fit_or_labels, "centroids") and hasattr(fit_or_labels, "labels"):
        labels = fit_or_labels.labels
        if labels is None:
            raise ValueError("%s: the fit carries no labels (fit_narratives(..., labels=True))" % who)
        if n_clusters is None:
            n_clusters = int(fit_or_labels.centroids.shape[0])
    if n_clusters is None:
        raise ValueError("%s: n_clusters is required with a label array" % who)
    return labels, int(n_clusters)


def _host_records(rec):
    """Records as an analyzer.COUNTERS_DTYPE array [., .] on the host (a torch int64 tensor [., ., 8] is copied off the device)."""
    from .analyzer import COUNTERS_DTYPE
    if hasattr(rec, "data_ptr"):
        rec = rec.cpu().numpy().view(COUNTERS_DTYPE).reshape(rec.shape[0], rec.shape[1])
    return rec


def narrative_timeline(index, fit_or_labels, stamp_origin, bucket_width, n_buckets, n_clusters=None, filter=None):
    """How every narrative developed over time: `share_of_voice` of `index.label_summary` (oi_label_summary on the time axis,
    one pass over labels, stamps and signals -- no corpus stream, whatever the bucket width or window asked for).  Entry [c][b]
    holds narrative c's total in bucket b, its fraction of the bucket's labelled posts and the SocialSummary of its posts.
    fit_or_labels: a NarrativeFit made with labels=True (n_clusters is then its number of centroids), or a label array
    [n_docs] by local row (numpy or torch CUDA tensor) with n_clusters given."""
    labels, K = _narrative_labels("narrative_timeline", fit_or_labels, n_clusters)
    rec = index.label_summary(labels, K, n_buckets=int(n_buckets), stamp_origin=int(stamp_origin), bucket_width=int(bucket_width),
                              filter=filter)
    return share_of_voice(_host_records(rec))


def narrative_tickers(index, fit_or_labels, tickers, key_mask: int, n_clusters=None, top: int = 10, rank_by: RankBy = RankBy.CROWDING,
                      min_total: Optional[int] = None, n_keys: Optional[int] = None, filter=None, market_by_ticker=None,
                      now: Optional[_dt.datetime] = None, cfg: EngineConfig = EngineConfig(), distinctive: bool = False) -> List[CompareOutput]:
    """Which tickers every narrative is about, and what its posts feel per ticker: per cluster a CompareOutput -- compare_index
    with the label in the similarity's place.  ONE ranked `index.label_groups` call by total (oi_label_summary on the key axis:
    per cluster the `top` most-mentioned tickers with at least `min_total` posts, default `cfg.min_sample`), then
    `rank_group_records` per cluster.  n_keys defaults to the number of names (a mapping: its largest key + 1).
    distinctive=True lists instead the tickers a narrative holds MORE of than the labelled posts at large: the dense totals,
    transposed to [n_keys, n_clusters], go through `retriever.rank_label_terms` with the per-cluster sums as the sizes -- its
    order (excess = total[c][k] * A - size[c] * total[.][k] descending, then total descending, then key ascending, among the
    keys with total >= max(min_total, 1)) is the rule wanted; top is then at most 64.
    fit_or_labels as in narrative_timeline.  The index's signals must have been set with `cfg.bull_bear_threshold`."""
    import numpy as np
    from . import retriever
    labels, K = _narrative_labels("narrative_tickers", fit_or_labels, n_clusters)
    if n_keys is None:
        n_keys = (max(tickers) + 1) if isinstance(tickers, dict) else len(tickers)
    bar = int(cfg.min_sample if min_total is None else min_total)
    if not distinctive:
        res = index.label_groups(labels, K, int(key_mask), int(n_keys), top=int(top), rank_by="total", min_total=bar, filter=filter)
        keys, counts, rec = res.keys, res.counts, _host_records(res.records)
        if hasattr(keys, "data_ptr"):
            keys, counts = keys.cpu().numpy().view(np.uint32), counts.cpu().numpy().view(np.uint32)
        return [rank_group_records(keys[c], rec[c], int(counts[c]), tickers, rank_by, market_by_ticker, now, cfg) for c in range(K)]
    rec = _host_records(index.label_groups(labels, K, int(key_mask), int(n_keys), filter=filter))
    totals = np.ascontiguousarray(rec["total"].astype(np.uint32).T)            # [n_keys][n_clusters]
    sizes = rec["total"].sum(axis=1, dtype=np.uint64)
    terms, n = retriever.rank_label_terms(index.ctx, totals, sizes, top=int(top), min_df=max(bar, 1))
    out = []
    for c in range(K):
        keys = [int(t) for t in terms[c]["term"][:int(n[c])]]
        out.append(rank_group_records(keys, [rec[c][k] for k in keys], len(keys), tickers, rank_by, market_by_ticker, now, cfg))
    return out


# ----------------------------------------------------------------------------- wire format (#[derive(Serialize)])
def scan_output_to_json(out: ScanOutput) -> str:
    """serde_json::to_string_pretty(&ScanOutput): `report` / `error` are skipped when None (tools.rs:180-183)."""
    entries = []
    for e in out.entries:
        row = {"ticker": e.ticker}
        if e.report is not None:
            row["report"] = report_to_wire(e.report)
        if e.error is not None:
            row["error"] = e.error
        entries.append(row)
    return _pretty({"entries": entries, "disclaimer": out.disclaimer})


def compare_output_to_json(out: CompareOutput) -> str:
    """serde_json::to_string_pretty(&CompareOutput): field order of the structs, snake_case RankBy."""
    return _pretty({
        "rank_by": out.rank_by.value,
        "ranked": [{"ticker": r.ticker, "rank_metric": _Raw(_json_f64(r.rank_metric)), "report": report_to_wire(r.report)}
                   for r in out.ranked],
        "errors": [{"ticker": e.ticker, "error": e.error} for e in out.errors],
        "disclaimer": out.disclaimer,
    })
