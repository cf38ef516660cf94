"""Hybrid retrieval (cosine + BM25 + reciprocal-rank fusion) on one MI355X.

The reference has no retrieval port, so `PostRetriever` is a NEW port,
styled after the reference's existing ones (borrowed inputs, owned outputs, DomainError-style
failures -- compare src/domain/ports/post_analyzer.rs:7-11).  `HybridIndex` is its
libopenintel_hip.so implementation; `openintel_amd.sharded` scales it over RCCL.
"""
from __future__ import annotations

import abc
import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .context import HipContext

DEFAULT_DEPTH = 1000  # per-list depth k' fed to RRF
DEFAULT_K = 100


@dataclass
class RankedLists:
    """Per-query ranked lists of one shard: rows sorted by (score desc, doc id asc)."""
    cos_scores: object
    cos_docs: object
    cos_counts: object
    bm25_scores: object
    bm25_docs: object
    bm25_counts: object


@dataclass
class SearchResult:
    scores: object   # [B, k] f32 RRF scores
    docs: object     # [B, k] u32 global doc ids
    counts: object   # [B] valid entries per row


@dataclass
class CollapsedResult(SearchResult):
    """A SearchResult whose near-duplicates were collapsed (oi_collapse_lists / oi_search_collapsed)."""
    dup_counts: object = None   # [B, k] u32: entries of the input list each kept entry stands for, itself included


@dataclass
class GroupRanking:
    """Ranked output of HybridIndex.similar_groups (oi_similar_groups with top >= 1); row stride `top`."""
    keys: object        # [B, top] u32 (a torch tensor holds the same bits as int32): 0xFFFFFFFF past counts[q]
    records: object     # [B, top] analyzer.COUNTERS_DTYPE (torch: int64 [B, top, 8]): all zero past counts[q]
    counts: object      # [B] u32: keys listed
    qualified: object   # [B] u32: keys with total >= max(min_total, 1), before the cut at `top`


@dataclass
class NarrativeFit:
    """Result of HybridIndex.fit_narratives (oi_narratives_fit): everything describes the LAST assignment step."""
    centroids: object   # [K, dim] f32: the narratives the last step assigned against
    records: object     # [K, n_buckets] analyzer.COUNTERS_DTYPE (torch: int64 [K, n_buckets, 8])
    labels: object      # [n_docs] u32 by local row (0xFFFFFFFF: unassigned), or None when not asked for
    iterations: int     # assignment steps run
    converged: bool     # a step after the first moved no row
    moved: int          # rows whose label changed in the last step
    assigned: int       # rows the last step assigned


@dataclass
class NarrativeSeeds:
    """Result of HybridIndex.seed_narratives (oi_narratives_seed)."""
    seeds: object       # [K, dim] f32: the chosen stored rows, bit for bit; zero vectors at and beyond `found`
    rows: object        # [K] u32 local rows (0xFFFFFFFF at and beyond `found`)
    found: int          # seeds chosen: K unless the weights ran out (every eligible row coincides with a seed)
    eligible: int       # rows that pass the filter and have a bucket
    potential: int      # sum over the eligible rows of rint((1 - sim to the nearest seed) * 2^20), after the last seed


GROUP_RANKS = {"total": _lib.OI_GROUP_RANK_TOTAL, "spec": _lib.OI_GROUP_RANK_SPEC, "bullish": _lib.OI_GROUP_RANK_BULLISH,
               "bearish": _lib.OI_GROUP_RANK_BEARISH}


class PostRetriever(abc.ABC):
    """New port: rank stored posts for a batch of (embedding, term-id) queries."""

    @abc.abstractmethod
    def search(self, query_vecs, query_terms, q_term_offsets, k: int = DEFAULT_K,
               depth: int = DEFAULT_DEPTH) -> SearchResult:
        ...


def packed_words(n_queries: int, depth: int) -> int:
    """OI_PACKED_WORDS of include/openintel_hip.h."""
    return 4 * n_queries * depth + 2 * n_queries


def unpack_lists(packed, n_queries: int, depth: int) -> "RankedLists":
    """Views into one shard's packed buffer (numpy array or torch tensor of 32-bit words)."""
    L = n_queries * depth
    if hasattr(packed, "data_ptr"):
        import torch
        sc = packed[:2 * L].view(torch.float32).reshape(2, n_queries, depth)
    else:
        sc = packed[:2 * L].view(np.float32).reshape(2, n_queries, depth)
    dc = packed[2 * L:4 * L].reshape(2, n_queries, depth)
    cn = packed[4 * L:].reshape(2, n_queries)
    return RankedLists(sc[0], dc[0], cn[0], sc[1], dc[1], cn[1])


def _is_dev(x) -> bool:
    return hasattr(x, "data_ptr")


def _np(x, dtype):
    return np.ascontiguousarray(x, dtype=dtype)


def pack_query_terms(term_lists: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    offs = np.zeros(len(term_lists) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(t) for t in term_lists])
    flat = np.fromiter((t for ts in term_lists for t in ts), dtype=np.uint32, count=int(offs[-1]))
    return flat, offs


def _packed_texts(texts, off_dtype):
    """texts: a sequence of str (packed here, host) or a (blob, offsets) pair (numpy arrays, or torch CUDA tensors: uint8
    blob + 8-byte / 4-byte integer offsets).  -> (is_device, blob, offsets, n_texts, blob_bytes)."""
    if isinstance(texts, tuple) and len(texts) == 2 and not isinstance(texts[0], str):
        blob, offsets = texts
        if _is_dev(blob):
            assert blob.is_contiguous() and offsets.is_contiguous() and blob.element_size() == 1
            assert offsets.element_size() == np.dtype(off_dtype).itemsize, "offsets: %s wanted" % np.dtype(off_dtype).name
            return True, blob, offsets, int(offsets.numel()) - 1, int(blob.numel())
        blob, offsets = _np(blob, np.uint8), np.asarray(offsets)
    else:
        from .analyzer import pack_posts
        blob, offsets = pack_posts(list(texts))
    if int(offsets[-1]) > np.iinfo(off_dtype).max:  # (a cast would wrap silently)
        raise ValueError("%d bytes of text do not fit %s offsets" % (int(offsets[-1]), np.dtype(off_dtype).name))
    offsets = _np(offsets, off_dtype)
    return False, blob, offsets, int(offsets.size) - 1, int(blob.size)


def _text_terms(ctx: HipContext, texts, vocab: int, off_dtype, count_only: bool):
    lib = ctx.lib
    fn = lib.oi_text_terms if off_dtype is np.uint64 else lib.oi_query_terms
    dev, blob, offsets, n, nbytes = _packed_texts(texts, off_dtype)
    loc = _lib.OI_DEVICE if dev else _lib.OI_HOST
    if dev:
        import torch
        where = blob.device
        out_offs = torch.zeros(n + 1, dtype=torch.int64 if off_dtype is np.uint64 else torch.int32, device=where)
    else:
        out_offs = np.zeros(n + 1, dtype=off_dtype)
    total = C.c_uint64()
    if count_only:
        _lib.check(fn(ctx.handle, _lib.ptr(blob), _lib.ptr(offsets), n, nbytes, int(vocab), loc, None, 0, _lib.ptr(out_offs),
                      C.byref(total)))
        return total.value, out_offs
    if not dev:
        # host text is copied to the GPU by the call: ONE call, into a buffer that is always large enough (two tokens need a
        # separator between them)
        ids = np.zeros(max((nbytes + 1) // 2, 1), dtype=np.uint32)
        _lib.check(fn(ctx.handle, _lib.ptr(blob), _lib.ptr(offsets), n, nbytes, int(vocab), loc, _lib.ptr(ids), ids.size,
                      _lib.ptr(out_offs), C.byref(total)))
        return ids[:total.value].copy() if total.value < ids.size else ids, out_offs
    # text in HBM: nothing is copied, so one call for the size (the count pass, 0.7 ms per 10M posts) and one to fill a
    # buffer of exactly that size rather than holding 2 B of ids per byte of text
    _lib.check(fn(ctx.handle, _lib.ptr(blob), _lib.ptr(offsets), n, nbytes, int(vocab), loc, None, 0, _lib.ptr(out_offs),
                  C.byref(total)))
    ids = torch.zeros(max(total.value, 1), dtype=torch.int32, device=where)
    _lib.check(fn(ctx.handle, _lib.ptr(blob), _lib.ptr(offsets), n, nbytes, int(vocab), loc, _lib.ptr(ids), total.value,
                  _lib.ptr(out_offs), None))
    return ids[:total.value], out_offs


def text_terms(ctx: HipContext, texts, vocab: int, count_only: bool = False):
    """oi_text_terms: the reference's tokens of every text hashed onto [0, vocab), in text order, duplicates kept.
    texts: a sequence of str, or (blob, offsets) as analyzer.pack_posts makes them (numpy, or torch CUDA tensors -- the
    outputs then stay in HBM: int32 ids holding the u32 bits, int64 offsets).  -> (term_ids, text_offsets[n + 1]);
    count_only: (total, text_offsets) without producing the ids."""
    return _text_terms(ctx, texts, vocab, np.uint64, count_only)


class HybridIndex(PostRetriever):
    """One corpus shard resident in HBM: n_docs x dim f32 rows + a blocked BM25 inverted index."""

    def __init__(self, ctx: HipContext, n_docs: int, dim: int, vocab: int, doc_id_base: int = 0):
        self.ctx = ctx
        self.lib = ctx.lib
        self.n_docs, self.dim, self.vocab, self.doc_id_base = int(n_docs), int(dim), int(vocab), int(doc_id_base)
        h = C.c_void_p()
        _lib.check(self.lib.oi_index_create(ctx.handle, self.n_docs, self.dim, self.vocab, self.doc_id_base,
                                            C.byref(h)))
        self.handle = h
        self._keep = []  # device tensors the library borrows

    # ---------------------------------------------------------------- build
    def set_embeddings(self, rows, normalize: bool = True) -> None:
        """rows: [n_docs, dim] f32 numpy array (copied to HBM) or torch CUDA tensor (borrowed;
        normalised in place when normalize=True)."""
        if _is_dev(rows):
            assert tuple(rows.shape) == (self.n_docs, self.dim) and rows.is_contiguous()
            self._keep.append(rows)
            loc = _lib.OI_DEVICE
        else:
            rows = _np(rows, np.float32)
            assert rows.shape == (self.n_docs, self.dim)
            loc = _lib.OI_HOST
        _lib.check(self.lib.oi_index_set_embeddings(self.handle, _lib.ptr(rows), loc, 1 if normalize else 0))

    def set_embeddings_bf16(self, rows) -> None:
        """A bf16 corpus: a torch.bfloat16 CUDA tensor [n_docs, dim] (borrowed, never copied) or a numpy
        uint16 array of bfloat16 bit patterns (copied to HBM).  Rows must be unit-norm as stored."""
        if _is_dev(rows):
            assert rows.is_contiguous() and tuple(rows.shape) == (self.n_docs, self.dim) and rows.element_size() == 2
            self._keep.append(rows)  # keep the borrowed matrix alive
            loc = _lib.OI_DEVICE
        else:
            rows = np.ascontiguousarray(rows, dtype=np.uint16)
            assert rows.shape == (self.n_docs, self.dim)
            loc = _lib.OI_HOST
        _lib.check(self.lib.oi_index_set_embeddings_bf16(self.handle, _lib.ptr(rows), loc))

    def set_forward(self, term_ids, doc_offsets) -> None:
        """Forward index: doc d owns term_ids[doc_offsets[d]:doc_offsets[d+1]] (u32 ids, u64 offsets)."""
        if _is_dev(term_ids):
            loc = _lib.OI_DEVICE
        else:
            term_ids, doc_offsets = _np(term_ids, np.uint32), _np(doc_offsets, np.uint64)
            assert doc_offsets.size == self.n_docs + 1
            loc = _lib.OI_HOST
        _lib.check(self.lib.oi_index_set_forward(self.handle, _lib.ptr(term_ids), _lib.ptr(doc_offsets), loc))

    def set_text(self, texts) -> None:
        """set_forward from the posts' TEXT (oi_index_set_text): tokenised on the GPU with this index's vocab as the hash
        range -- bit for bit text_terms() + set_forward(), without the ids ever reaching the caller.  texts: n_docs str, or
        (blob, offsets) as analyzer.pack_posts makes them (numpy, or torch CUDA tensors: the blob the analyzer reads)."""
        dev, blob, offsets, n, nbytes = _packed_texts(texts, np.uint64)
        assert n == self.n_docs, "one text per document of the shard"
        _lib.check(self.lib.oi_index_set_text(self.handle, _lib.ptr(blob), _lib.ptr(offsets), nbytes,
                                              _lib.OI_DEVICE if dev else _lib.OI_HOST))

    def query_terms(self, texts):
        """Query texts -> (query_terms, q_term_offsets) as every search call takes them (oi_query_terms, this index's
        vocab): sequence of str, or (blob, u32 offsets); device in, device out."""
        return _text_terms(self.ctx, texts, self.vocab, np.uint32, False)

    def search_text(self, query_vecs, query_texts, k: int = DEFAULT_K, depth: int = DEFAULT_DEPTH,
                    out: Optional[SearchResult] = None, filters=None) -> SearchResult:
        """search() with the lexical side given as text: query_terms(query_texts), then search.  Host strings go with
        host vectors; a device (blob, offsets) pair with device vectors."""
        qt, qo = self.query_terms(query_texts)
        assert _is_dev(qt) == _is_dev(query_vecs), "query vectors and query texts must live in the same place"
        if _is_dev(qt) and qt.numel() == 0:
            qt = self._alloc(True, (1,), np.uint32)
        return self.search(query_vecs, qt, qo, k=k, depth=depth, out=out, filters=filters)

    def long_rows(self) -> int:
        """Rows the screened cosine scorer sets aside (always rescored, never part of its thresholds): oi_index_long_rows."""
        n = C.c_uint32()
        _lib.check(self.lib.oi_index_long_rows(self.handle, C.byref(n)))
        return int(n.value)

    def long_list(self) -> np.ndarray:
        """The long rows (local row numbers) in the order the rescoring reads them (internal, for the tests): a filtered search
        packs the passing ones by their position in this list."""
        n = C.c_uint32()
        rows = np.zeros(1024, np.uint32)            # OI_LONG_ROWS_MAX
        _lib.check(self.lib.oi_internal_long_list(self.handle, C.byref(n), _lib.ptr(rows)))
        return rows[:int(n.value)].copy()

    SCREEN_COPY_AUTO,SCREEN_COPY_NEVER, SCREEN_COPY_ALWAYS = _lib.OI_SCREEN_COPY_AUTO, _lib.OI_SCREEN_COPY_NEVER, _lib.OI_SCREEN_COPY_ALWAYS

    def set_screen_copy(self, policy: int) -> None:
        """The bf16 screening copy of an f32 corpus (oi_index_set_screen_copy): SCREEN_COPY_AUTO (default: made at finalize
        when n_docs x dim x 2 B is at most a quarter of the free HBM), _NEVER, _ALWAYS.  The default scorer's screen streams
        it instead of the f32 rows -- half the bytes, the same lists."""
        _lib.check(self.lib.oi_index_set_screen_copy(self.handle, int(policy)))

    def index_bytes(self):
        """(rows owned by the library, screening copy, BM25 structures) in bytes of HBM: oi_index_bytes."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _lib.check(self.lib.oi_index_bytes(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def residual_plane(self, drop: bool = False):
        """The residual plane of the int8 screening copy (internal, for the tests): None when the index holds none, else
        (j: int8 [n_docs, dim], {t_r, e2_r}: float32 [n_docs, 2], e2_max, bytes allocated).  drop=True frees it -- the index is
        then the one the AUTO budget makes when only two copies fit -- and returns None."""
        nb = C.c_uint64()
        _lib.check(self.lib.oi_internal_residual_plane(self.handle, 1 if drop else 0, None, None, None, C.byref(nb)))
        if drop or nb.value == 0:
            return None
        j = np.empty((self.n_docs, self.dim), np.int8)
        meta = np.empty((self.n_docs, 2), np.float32)
        e2max = np.zeros(1, np.float32)
        _lib.check(self.lib.oi_internal_residual_plane(self.handle, 0, _lib.ptr(j), _lib.ptr(meta), _lib.ptr(e2max), C.byref(nb)))
        return j, meta, float(e2max[0]), int(nb.value)

    def residual_rescreen(self, queries, keys, counts, cap: Optional[int] = None):
        """The int8 route's query staging and its residual rescreen over the caller's keys (internal, for the tests): the
        two product launches, in workspaces of their own.  queries: float32 [B, dim]; keys: uint64 [B, stride] rank keys
        (lower-bound score over ~doc); counts: uint32 [B]; cap: the pool's carry_cap (default: stride).  Needs an index (or a
        view of one) that holds both int8 planes.  Returns a dict: keys (the whole block after the launch; the caller's array is
        not written), h and l: int8 [n_padded, dim], qf: float32 [4, n_padded] (a, |q^|, c_q, m2), eps2r: float32 [B] (2 eps2'),
        gate (int) and X, e_max, e2_max (np.float32: the three scalars the staging read)."""
        q = _np(queries, np.float32)
        B = q.shape[0]
        assert q.shape == (B, self.dim)
        k = np.array(keys, dtype=np.uint64, order="C")
        assert k.ndim == 2 and k.shape[0] == B
        stride = k.shape[1]
        cnt = _np(counts, np.uint32)
        assert cnt.shape == (B,)
        n_padded = (B + 31) & ~31
        qi8 = np.empty((2, n_padded, self.dim), np.int8)
        qf = np.empty((4, n_padded), np.float32)
        eps2r = np.empty(B, np.float32)
        gate = np.zeros(1, np.uint32)
        sc = np.zeros(3, np.float32)
        _lib.check(self.lib.oi_internal_residual_rescreen(self.handle, _lib.ptr(q), B, _lib.ptr(k), _lib.ptr(cnt), stride,
                                                          stride if cap is None else int(cap), _lib.ptr(qi8), _lib.ptr(qf),
                                                          _lib.ptr(eps2r), _lib.ptr(gate), _lib.ptr(sc)))
        return dict(keys=k, h=qi8[0], l=qi8[1], qf=qf, eps2r=eps2r, gate=int(gate[0]), X=sc[0], e_max=sc[1], e2_max=sc[2])

    def bm25_index(self):
        """The BM25 structures of a finalized index or of a view of one (internal, for the tests): a dict of n_postings, n_win,
        avgdl (np.float32) and the arrays dib: uint32 [n_postings], impact: float32 [n_postings], cell_start: uint32
        [vocab * n_win + 1], idf: float32 [vocab], floors: uint32 [vocab, 4], doc_len: uint32 [n_docs]."""
        n, w, a = C.c_uint64(), C.c_uint32(), C.c_float()
        _lib.check(self.lib.oi_internal_bm25_index(self.handle, C.byref(n), C.byref(w), C.byref(a), None, None, None, None, None))
        post = np.zeros((n.value, 2), np.uint32)
        cell_start = np.zeros(self.vocab * w.value + 1, np.uint32)
        idf = np.zeros(self.vocab, np.float32)
        floors = np.zeros((self.vocab, 4), np.uint32)
        doc_len = np.zeros(self.n_docs, np.uint32)
        _lib.check(self.lib.oi_internal_bm25_index(self.handle, C.byref(n), C.byref(w), C.byref(a), _lib.ptr(post), _lib.ptr(cell_start),
                                                   _lib.ptr(idf), _lib.ptr(floors), _lib.ptr(doc_len)))
        return dict(n_postings=int(n.value), n_win=int(w.value), avgdl=np.float32(a.value), dib=post[:, 0].copy(),
                    impact=post[:, 1].copy().view(np.float32), cell_start=cell_start, idf=idf, floors=floors, doc_len=doc_len)

    BM25_DEFAULT, BM25_TAAT, BM25_SCAN, BM25_WAVE, BM25_STREAM = 0, 1, 2, 3, 4

    def set_bm25_mode(self, mode: int) -> None:
        """BM25_STREAM (term-at-a-time as a stream through a per-wave LDS ring: the default), BM25_WAVE (one wave per
        (block, query) task), BM25_TAAT (the first-generation workgroup-per-block kernel) or BM25_SCAN (batch scan of
        the forward index).  Bit-identical lists."""
        _lib.check(self.lib.oi_index_set_bm25_mode(self.handle, int(mode)))

    def set_doc_attrs(self, group=None, stamp=None) -> None:
        """Per-document attributes of filtered searches (oi_index_set_doc_attrs): `group` and `stamp`, n_docs uint32 each
        (numpy arrays, or torch CUDA tensors of int32 / uint32), indexed by local row; None = zeros.  The first call allocates
        them, later ones overwrite them in place (retag or soft-delete documents; views see the update)."""
        arrs = []
        dev = _is_dev(group) or _is_dev(stamp)
        for a in (group, stamp):
            if a is None:
                arrs.append(None)
            elif dev:
                assert _is_dev(a) and a.is_contiguous() and a.numel() == self.n_docs and a.element_size() == 4
                arrs.append(a)
            else:
                a = _np(a, np.uint32)
                assert a.size == self.n_docs
                arrs.append(a)
        _lib.check(self.lib.oi_index_set_doc_attrs(self.handle, _lib.ptr(arrs[0]), _lib.ptr(arrs[1]),
                                                   _lib.OI_DEVICE if dev else _lib.OI_HOST))
        if dev:
            self.ctx.synchronize()  # (the strided copies out of the caller's tensors have completed: nothing to keep alive)

    def _filters(self, filters, dev: bool, B: int):
        """(n_queries, 4) uint32 {group_mask, group_value, stamp_lo, stamp_hi} per query, on the queries' side."""
        if dev:
            import torch
            if not _is_dev(filters):
                f = np.ascontiguousarray(np.asarray(filters, dtype=np.uint32).reshape(B, 4))
                filters = torch.from_numpy(f.view(np.int32)).to("cuda:%d" % self.ctx.device)
            assert filters.is_contiguous() and filters.numel() == 4 * B and filters.element_size() == 4
            self._filt_keep = filters  # (an asynchronous call reads it later)
            return filters
        if _is_dev(filters):
            filters = filters.cpu().numpy()
        f = np.ascontiguousarray(np.asarray(filters).astype(np.uint32, copy=False).reshape(B, 4))
        return f

    def set_max_query_terms(self, max_terms: int) -> None:
        """Contract for the batch BM25 scan: no query has more terms than this (default 16)."""
        _lib.check(self.lib.oi_index_set_max_query_terms(self.handle, int(max_terms)))

    def local_stats(self) -> Tuple[int, np.ndarray]:
        tot = C.c_uint64()
        df = np.zeros(self.vocab, dtype=np.uint32)
        _lib.check(self.lib.oi_index_local_stats(self.handle, C.byref(tot), _lib.ptr(df)))
        return tot.value, df

    def finalize(self, global_n_docs: Optional[int] = None, global_total_tokens: Optional[int] = None,
                 global_df: Optional[np.ndarray] = None) -> None:
        if global_n_docs is None:
            tot, _ = self.local_stats()
            global_n_docs, global_total_tokens, global_df = self.n_docs, tot, None
        df = None if global_df is None else _np(global_df, np.uint32)
        _lib.check(self.lib.oi_index_finalize(self.handle, int(global_n_docs), int(global_total_tokens),
                                              _lib.ptr(df)))

    # ---------------------------------------------------------------- query
    def _alloc(self, like_device: bool, shape, dtype):
        if like_device:
            import torch
            tdt = {np.float32: torch.float32, np.uint32: torch.int32}[dtype]
            return torch.zeros(shape, dtype=tdt, device="cuda:%d" % self.ctx.device)
        return np.zeros(shape, dtype=dtype)

    def _queries(self, query_vecs, query_terms, q_term_offsets):
        dev = _is_dev(query_vecs)
        if not dev:
            query_vecs = _np(query_vecs, np.float32)
            query_terms = _np(query_terms, np.uint32)
            q_term_offsets = _np(q_term_offsets, np.uint32)
            if query_terms.size == 0:
                query_terms = np.zeros(1, dtype=np.uint32)
        B = int(query_vecs.shape[0])
        assert int(query_vecs.shape[1]) == self.dim
        return dev, B, query_vecs, query_terms, q_term_offsets

    def search_lists(self, query_vecs, query_terms, q_term_offsets, depth: int = DEFAULT_DEPTH, filters=None) -> RankedLists:
        """filters: None, or (n_queries, 4) uint32 doc filters (oi_doc_filter rows; host array or torch CUDA tensor)."""
        dev, B, qv, qt, qo = self._queries(query_vecs, query_terms, q_term_offsets)
        out = RankedLists(*(self._alloc(dev, s, d) for s, d in (
            ((B, depth), np.float32), ((B, depth), np.uint32), ((B,), np.uint32),
            ((B, depth), np.float32), ((B, depth), np.uint32), ((B,), np.uint32))))
        if filters is not None:
            f = self._filters(filters, dev, B)
            _lib.check(self.lib.oi_search_lists_filtered(
                self.handle, _lib.ptr(qv), _lib.ptr(qt), _lib.ptr(qo), B, int(depth), _lib.ptr(f),
                _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(out.cos_scores), _lib.ptr(out.cos_docs),
                _lib.ptr(out.cos_counts), _lib.ptr(out.bm25_scores), _lib.ptr(out.bm25_docs),
                _lib.ptr(out.bm25_counts)))
            return out
        _lib.check(self.lib.oi_search_lists(
            self.handle, _lib.ptr(qv), _lib.ptr(qt), _lib.ptr(qo), B, int(depth),
            _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(out.cos_scores), _lib.ptr(out.cos_docs),
            _lib.ptr(out.cos_counts), _lib.ptr(out.bm25_scores), _lib.ptr(out.bm25_docs),
            _lib.ptr(out.bm25_counts)))
        return out

    def search_lists_packed(self, query_vecs, query_terms, q_term_offsets, depth: int = DEFAULT_DEPTH, out=None,
                            filters=None):
        """The shard's two lists in the multi-GPU exchange format (include/openintel_hip.h,
        OI_PACKED_WORDS): one flat int32/uint32 buffer, ready for all_gather_into_tensor."""
        dev, B, qv, qt, qo = self._queries(query_vecs, query_terms, q_term_offsets)
        words = packed_words(B, depth)
        if out is None:
            out = self._alloc(dev, (words,), np.uint32)
        if filters is not None:
            f = self._filters(filters, dev, B)
            _lib.check(self.lib.oi_search_lists_packed_filtered(self.handle, _lib.ptr(qv), _lib.ptr(qt), _lib.ptr(qo), B,
                                                                int(depth), _lib.ptr(f), _lib.OI_DEVICE if dev else _lib.OI_HOST,
                                                                _lib.ptr(out)))
            return out
        _lib.check(self.lib.oi_search_lists_packed(self.handle, _lib.ptr(qv), _lib.ptr(qt), _lib.ptr(qo), B,
                                                   int(depth), _lib.OI_DEVICE if dev else _lib.OI_HOST,
                                                   _lib.ptr(out)))
        return out

    def search(self, query_vecs, query_terms, q_term_offsets, k: int = DEFAULT_K,
               depth: int = DEFAULT_DEPTH, out: Optional[SearchResult] = None, filters=None) -> SearchResult:
        dev, B, qv, qt, qo = self._queries(query_vecs, query_terms, q_term_offsets)
        if out is None:
            out = SearchResult(self._alloc(dev, (B, k), np.float32), self._alloc(dev, (B, k), np.uint32),
                               self._alloc(dev, (B,), np.uint32))
        if filters is not None:
            f = self._filters(filters, dev, B)
            _lib.check(self.lib.oi_search_filtered(self.handle, _lib.ptr(qv), _lib.ptr(qt), _lib.ptr(qo), B, int(depth),
                                                   int(k), _lib.ptr(f), _lib.OI_DEVICE if dev else _lib.OI_HOST,
                                                   _lib.ptr(out.scores), _lib.ptr(out.docs), _lib.ptr(out.counts)))
            return out
        _lib.check(self.lib.oi_search(self.handle, _lib.ptr(qv), _lib.ptr(qt), _lib.ptr(qo), B, int(depth), int(k),
                                      _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(out.scores),
                                      _lib.ptr(out.docs), _lib.ptr(out.counts)))
        return out

    # ---------------------------------------------------------------- near-duplicate collapse
    def collapse_lists(self, scores, docs, counts, threshold: float, k: int) -> "CollapsedResult":
        """oi_collapse_lists: ranked lists of this index's documents ([B, depth] docs, [B] counts; scores [B, depth] or None)
        with every entry whose stored row has a dot product >= threshold with a better-ranked kept entry folded into it.
        Host arrays in, host arrays out; torch CUDA tensors in, tensors out (asynchronous on the ctx stream)."""
        dev = _is_dev(docs)
        if not dev:
            docs, counts = _np(docs, np.uint32), _np(counts, np.uint32)
            scores = None if scores is None else _np(scores, np.float32)
        else:
            assert docs.is_contiguous() and counts.is_contiguous() and (scores is None or scores.is_contiguous())
        B, depth = int(docs.shape[0]), int(docs.shape[1])
        out = CollapsedResult(None if scores is None else self._alloc(dev, (B, k), np.float32), self._alloc(dev, (B, k), np.uint32),
                              self._alloc(dev, (B,), np.uint32), self._alloc(dev, (B, k), np.uint32))
        _lib.check(self.lib.oi_collapse_lists(self.handle, _lib.ptr(scores), _lib.ptr(docs), _lib.ptr(counts), B, depth,
                                              float(threshold), int(k), _lib.OI_DEVICE if dev else _lib.OI_HOST,
                                              _lib.ptr(out.scores), _lib.ptr(out.docs), _lib.ptr(out.counts),
                                              _lib.ptr(out.dup_counts)))
        return out

    def search_collapsed(self, query_vecs, query_terms, q_term_offsets, k: int = DEFAULT_K, depth: int = DEFAULT_DEPTH,
                         pool: int = DEFAULT_DEPTH, threshold: float = 0.9, filters=None,
                         out: Optional["CollapsedResult"] = None) -> "CollapsedResult":
        """oi_search_collapsed: search(k=pool, filters) followed by collapse_lists(threshold, k) with the fused pool-list kept
        on the device.  Scores are the RRF scores of the kept documents."""
        dev, B, qv, qt, qo = self._queries(query_vecs, query_terms, q_term_offsets)
        if out is None:
            out = CollapsedResult(self._alloc(dev, (B, k), np.float32), self._alloc(dev, (B, k), np.uint32),
                                  self._alloc(dev, (B,), np.uint32), self._alloc(dev, (B, k), np.uint32))
        f = None if filters is None else self._filters(filters, dev, B)
        _lib.check(self.lib.oi_search_collapsed(self.handle, _lib.ptr(qv), _lib.ptr(qt), _lib.ptr(qo), B, int(depth), int(pool),
                                                int(k), float(threshold), _lib.ptr(f), _lib.OI_DEVICE if dev else _lib.OI_HOST,
                                                _lib.ptr(out.scores), _lib.ptr(out.docs), _lib.ptr(out.counts),
                                                _lib.ptr(out.dup_counts)))
        return out

    # ---------------------------------------------------------------- similarity volume
    def similar_volume(self, query_vecs, threshold: float, n_buckets: int = 1, stamp_origin: int = 0, bucket_width: int = 0,
                       filters=None):
        """oi_similar_volume: [B, n_buckets] uint32 counts of this shard's documents with sim(q, d) >= threshold that pass
        filters[q] and whose stamp falls into bucket (stamp - stamp_origin) // bucket_width (bucket_width = 0: no time axis,
        one bucket).  sim is the f32 score a default search_lists returns for the row.  Host array in, numpy out; torch CUDA
        tensor in, tensor out (asynchronous on the ctx stream).  Counts of shards add."""
        dev = _is_dev(query_vecs)
        if dev:
            assert query_vecs.is_contiguous() and query_vecs.element_size() == 4
        else:
            query_vecs = _np(query_vecs, np.float32)
        B = int(query_vecs.shape[0])
        assert B == 0 or int(query_vecs.shape[1]) == self.dim
        spec = _lib.VolumeSpec(float(threshold), int(stamp_origin), int(bucket_width), int(n_buckets))
        out = self._alloc(dev, (B, max(int(n_buckets), 0)), np.uint32)
        f = None if filters is None else self._filters(filters, dev, B)
        _lib.check(self.lib.oi_similar_volume(self.handle, _lib.ptr(query_vecs), B, C.byref(spec), _lib.ptr(f),
                                              _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(out)))
        return out

    # ---------------------------------------------------------------- similarity summary
    def set_signals(self, polarity, speculative, sources=None, bull_bear_threshold: float = 0.2) -> None:
        """The per-post signals similar_summary sums (oi_index_set_signals): `polarity` float64 and `speculative` uint8 as the
        lexicon analyzer returns them, `sources` uint8 (0 = reddit, 1 = bluesky; None = all reddit), n_docs each, indexed by
        local row -- numpy arrays, or torch CUDA tensors (nothing per post touches the host).  A post's bullish / bearish
        class is fixed here with `bull_bear_threshold`.  The first call allocates 8 B per row, later ones overwrite them in
        place (views see the update)."""
        dev = _is_dev(polarity)
        arrs = []
        for a, dt in ((polarity, np.float64), (speculative, np.uint8), (sources, np.uint8)):
            if a is None:
                arrs.append(None)
            elif dev:
                assert _is_dev(a) and a.is_contiguous() and a.numel() == self.n_docs and a.element_size() == np.dtype(dt).itemsize
                arrs.append(a)
            else:
                a = _np(a, dt)
                assert a.size == self.n_docs
                arrs.append(a)
        _lib.check(self.lib.oi_index_set_signals(self.handle, _lib.ptr(arrs[0]), _lib.ptr(arrs[1]), _lib.ptr(arrs[2]),
                                                 float(bull_bear_threshold), _lib.OI_DEVICE if dev else _lib.OI_HOST))
        if dev:
            self.ctx.synchronize()  # (the pack kernel has read the caller's tensors: nothing to keep alive)

    def set_signals_from_text(self, texts, sources=None, bull_bear_threshold: float = 0.2) -> None:
        """set_signals from the posts' TEXT: the lexicon scan on the device (oi_lexicon_analyze_device), then the pack
        (oi_index_set_signals, OI_DEVICE) -- the two C calls composed, the signals never reach the host.  texts: n_docs
        str, or (blob, offsets) as analyzer.pack_posts makes them (numpy, or torch CUDA tensors: the blob set_text reads)."""
        import torch
        dev, blob, offsets, n, nbytes = _packed_texts(texts, np.uint64)
        assert n == self.n_docs, "one text per document of the shard"
        where = "cuda:%d" % self.ctx.device
        if not dev:
            blob = torch.from_numpy(np.concatenate([blob, np.zeros(8, np.uint8)])).to(where)  # (never an empty tensor)
            offsets = torch.from_numpy(offsets.view(np.int64)).to(where)
        pol = torch.zeros(n, dtype=torch.float64, device=where)
        spec = torch.zeros(n, dtype=torch.uint8, device=where)
        if sources is not None and not _is_dev(sources):
            sources = torch.from_numpy(_np(sources, np.uint8)).to(where)
        _lib.check(self.lib.oi_lexicon_analyze_device(self.ctx.handle, _lib.ptr(blob), _lib.ptr(offsets), n, nbytes,
                                                      _lib.ptr(pol), _lib.ptr(spec)))
        self.set_signals(pol, spec, sources, bull_bear_threshold)

    def similar_summary(self, query_vecs, threshold, n_buckets: int = 1, stamp_origin: int = 0, bucket_width: int = 0,
                        filters=None):
        """oi_similar_summary: [B, n_buckets] records (analyzer.COUNTERS_DTYPE, 64 bytes) of the social_summary sums over the
        documents similar_volume counts -- those with sim(q, d) >= threshold that pass filters[q] and fall into the bucket.
        threshold: a float, or one per query (array; a NaN entry counts nothing).  Integer fields exact; polarity_sum is a
        64-bit integer sum in steps of 2^-30, so the result does not depend on route, order or batch.  Host array in, numpy
        record array out; torch CUDA tensor in, an int64 tensor [B, n_buckets, 8] holding the records' bits out
        (asynchronous on the ctx stream; .cpu().numpy().view(COUNTERS_DTYPE) reads it).  Records of shards add.
        SpeculationEngine.social_from_counters turns a record into a SocialSummary."""
        from .analyzer import COUNTERS_DTYPE
        dev = _is_dev(query_vecs)
        if dev:
            assert query_vecs.is_contiguous() and query_vecs.element_size() == 4
        else:
            query_vecs = _np(query_vecs, np.float32)
        B = int(query_vecs.shape[0])
        assert B == 0 or int(query_vecs.shape[1]) == self.dim
        nb = max(int(n_buckets), 0)
        thr = None
        if not _is_dev(threshold) and np.ndim(threshold) == 0:
            spec = _lib.SummarySpec(float(threshold), int(stamp_origin), int(bucket_width), int(n_buckets))
        else:
            spec = _lib.SummarySpec(0.0, int(stamp_origin), int(bucket_width), int(n_buckets))
            if dev:
                import torch
                if not _is_dev(threshold):
                    threshold = torch.from_numpy(_np(threshold, np.float32)).to("cuda:%d" % self.ctx.device)
                assert threshold.is_contiguous() and threshold.numel() == B and threshold.element_size() == 4
                self._thr_keep = thr = threshold  # (an asynchronous call reads it later)
            else:
                thr = _np(threshold.cpu().numpy() if _is_dev(threshold) else threshold, np.float32)
                assert thr.size == B
        if dev:
            import torch
            out = torch.zeros((B, nb, 8), dtype=torch.int64, device="cuda:%d" % self.ctx.device)
        else:
            out = np.zeros((B, nb), dtype=COUNTERS_DTYPE)
        f = None if filters is None else self._filters(filters, dev, B)
        _lib.check(self.lib.oi_similar_summary(self.handle, _lib.ptr(query_vecs), B, C.byref(spec), _lib.ptr(thr), _lib.ptr(f),
                                               _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(out)))
        return out

    # ---------------------------------------------------------------- similarity leaderboard
    def similar_groups(self, query_vecs, threshold, key_mask: int, n_keys: int, top: int = 0, rank_by="total", min_total: int = 0,
                       filters=None):
        """oi_similar_groups: the social_summary sums of the documents like each query per KEY of their group attribute,
        key = (group & key_mask) >> ctz(key_mask) (a ticker id, say) -- similar_summary's clauses with the key in the bucket's
        place (filters carry a time window), same thresholds (a float, or one per query; a NaN entry counts nothing), same
        deterministic integer sums.  top == 0: [B, n_keys] records (analyzer.COUNTERS_DTYPE), what shards add.  top >= 1: a
        GroupRanking of the best `top` keys per query by rank_by ("total", "spec", "bullish", "bearish", or an
        OI_GROUP_RANK_* value; ties by key ascending) among the keys with total >= max(min_total, 1): keys [B, top] uint32
        (0xFFFFFFFF past the count), records [B, top], counts [B], qualified [B] (keys that qualified before the cut).  Host
        array in, numpy out; torch CUDA tensor in, tensors out (records as int64 [B, ., 8] holding the records' bits;
        asynchronous on the ctx stream)."""
        from .analyzer import COUNTERS_DTYPE
        dev = _is_dev(query_vecs)
        if dev:
            assert query_vecs.is_contiguous() and query_vecs.element_size() == 4
        else:
            query_vecs = _np(query_vecs, np.float32)
        B = int(query_vecs.shape[0])
        assert B == 0 or int(query_vecs.shape[1]) == self.dim
        by = GROUP_RANKS[rank_by] if isinstance(rank_by, str) else int(rank_by)
        top = int(top)
        thr = None
        if not _is_dev(threshold) and np.ndim(threshold) == 0:
            spec = _lib.GroupsSpec(float(threshold), int(key_mask), int(n_keys), top, by, int(min_total))
        else:
            spec = _lib.GroupsSpec(0.0, int(key_mask), int(n_keys), top, by, int(min_total))
            if dev:
                import torch
                if not _is_dev(threshold):
                    threshold = torch.from_numpy(_np(threshold, np.float32)).to("cuda:%d" % self.ctx.device)
                assert threshold.is_contiguous() and threshold.numel() == B and threshold.element_size() == 4
                self._thr_keep = thr = threshold  # (an asynchronous call reads it later)
            else:
                thr = _np(threshold.cpu().numpy() if _is_dev(threshold) else threshold, np.float32)
                assert thr.size == B
        per_q = max(top if top else int(n_keys), 0)
        if dev:
            import torch
            records = torch.zeros((B, per_q, 8), dtype=torch.int64, device="cuda:%d" % self.ctx.device)
        else:
            records = np.zeros((B, per_q), dtype=COUNTERS_DTYPE)
        keys = counts = qualified = None
        if top:
            keys, counts, qualified = (self._alloc(dev, (B, per_q), np.uint32), self._alloc(dev, (B,), np.uint32),
                                       self._alloc(dev, (B,), np.uint32))
        f = None if filters is None else self._filters(filters, dev, B)
        _lib.check(self.lib.oi_similar_groups(self.handle, _lib.ptr(query_vecs), B, C.byref(spec), _lib.ptr(thr), _lib.ptr(f),
                                              _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(records), _lib.ptr(keys),
                                              _lib.ptr(counts), _lib.ptr(qualified)))
        return GroupRanking(keys, records, counts, qualified) if top else records

    # ---------------------------------------------------------------- similarity share
    def similar_share(self, query_vecs, threshold, n_buckets: int = 1, stamp_origin: int = 0, bucket_width: int = 0,
                      filters=None, labels: bool = False):
        """oi_similar_share: similar_summary's [B, n_buckets] records, but every document is counted at most ONCE, under the
        query it is most like: among the queries whose filter it passes and whose threshold its similarity reaches (a float,
        or one per query; a NaN entry is nobody's candidate) the one with the largest similarity wins, ties to the smallest
        query.  Deterministic, and -- unlike similar_summary -- dependent on the batch composition: that is the point.
        labels=True returns (records, labels): labels [n_docs] uint32 by local row, the winner of an assigned document and
        0xFFFFFFFF for every other row.  Host array in, numpy out; torch CUDA tensor in, tensors out (records as int64
        [B, n_buckets, 8] holding the records' bits; asynchronous on the ctx stream).  batch.share_of_voice turns the records
        into each query's fraction of the assigned posts."""
        from .analyzer import COUNTERS_DTYPE
        dev = _is_dev(query_vecs)
        if dev:
            assert query_vecs.is_contiguous() and query_vecs.element_size() == 4
        else:
            query_vecs = _np(query_vecs, np.float32)
        B = int(query_vecs.shape[0])
        assert B == 0 or int(query_vecs.shape[1]) == self.dim
        nb = max(int(n_buckets), 0)
        thr = None
        if not _is_dev(threshold) and np.ndim(threshold) == 0:
            spec = _lib.SummarySpec(float(threshold), int(stamp_origin), int(bucket_width), int(n_buckets))
        else:
            spec = _lib.SummarySpec(0.0, int(stamp_origin), int(bucket_width), int(n_buckets))
            if dev:
                import torch
                if not _is_dev(threshold):
                    threshold = torch.from_numpy(_np(threshold, np.float32)).to("cuda:%d" % self.ctx.device)
                assert threshold.is_contiguous() and threshold.numel() == B and threshold.element_size() == 4
                self._thr_keep = thr = threshold  # (an asynchronous call reads it later)
            else:
                thr = _np(threshold.cpu().numpy() if _is_dev(threshold) else threshold, np.float32)
                assert thr.size == B
        if dev:
            import torch
            out = torch.zeros((B, nb, 8), dtype=torch.int64, device="cuda:%d" % self.ctx.device)
        else:
            out = np.zeros((B, nb), dtype=COUNTERS_DTYPE)
        lab = self._alloc(dev, (self.n_docs,), np.uint32) if labels else None
        f = None if filters is None else self._filters(filters, dev, B)
        _lib.check(self.lib.oi_similar_share(self.handle, _lib.ptr(query_vecs), B, C.byref(spec), _lib.ptr(thr), _lib.ptr(f),
                                             _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(out), _lib.ptr(lab)))
        return (out, lab) if labels else out

    # ---------------------------------------------------------------- mention summary
    def _mention(self, query_terms, q_term_offsets, spec, min_match, filters):
        """One oi_mention_summary call: host arrays in, numpy records out; CUDA tensors in, an int64 [B, n, 8] tensor out."""
        from .analyzer import COUNTERS_DTYPE
        dev = _is_dev(query_terms) or _is_dev(q_term_offsets)
        if dev:
            assert _is_dev(query_terms) and _is_dev(q_term_offsets), "terms and offsets must live in the same place"
            assert query_terms.is_contiguous() and query_terms.element_size() == 4
            assert q_term_offsets.is_contiguous() and q_term_offsets.element_size() == 4
            B = int(q_term_offsets.numel()) - 1
            if query_terms.numel() == 0:
                query_terms = self._alloc(True, (1,), np.uint32)
        else:
            query_terms, q_term_offsets = _np(query_terms, np.uint32), _np(q_term_offsets, np.uint32)
            B = int(q_term_offsets.size) - 1
            if query_terms.size == 0:
                query_terms = np.zeros(1, dtype=np.uint32)
        assert B >= 0, "q_term_offsets has n_queries + 1 entries"
        mm = None
        if isinstance(min_match, str):
            assert min_match in ("any", "all"), min_match
            min_match = None if min_match == "any" else 0
        if min_match is not None:
            if not _is_dev(min_match):
                mm = np.full(B, int(min_match), dtype=np.uint32) if np.ndim(min_match) == 0 else _np(min_match, np.uint32)
                assert mm.size == B
                if dev:
                    import torch
                    mm = torch.from_numpy(mm.view(np.int32)).to("cuda:%d" % self.ctx.device)
            else:
                mm = min_match if dev else _np(min_match.cpu().numpy(), np.uint32)
                assert (mm.numel() if dev else mm.size) == B and (not dev or (mm.is_contiguous() and mm.element_size() == 4))
        nc = max(int(spec.n_cells), 0)
        if dev:
            import torch
            out = torch.zeros((B, nc, 8), dtype=torch.int64, device="cuda:%d" % self.ctx.device)
            self._mention_keep = (query_terms, q_term_offsets, mm)  # (an asynchronous call reads them later)
        else:
            out = np.zeros((B, nc), dtype=COUNTERS_DTYPE)
        f = None if filters is None else self._filters(filters, dev, B)
        _lib.check(self.lib.oi_mention_summary(self.handle, _lib.ptr(query_terms), _lib.ptr(q_term_offsets), B, C.byref(spec),
                                               _lib.ptr(mm), _lib.ptr(f), _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(out)))
        return out

    def mention_summary(self, query_terms, q_term_offsets, min_match=None, n_buckets: int = 1, stamp_origin: int = 0,
                        bucket_width: int = 0, filters=None):
        """oi_mention_summary on the time axis: [B, n_buckets] records (analyzer.COUNTERS_DTYPE) of the social_summary sums
        over this shard's documents that CONTAIN the query's terms, pass filters[q] and fall into bucket
        (stamp - stamp_origin) // bucket_width (bucket_width = 0: one bucket).  A document matches when at least need_q of
        the query's DISTINCT terms occur in it: min_match None or "any" -> 1, "all" or 0 -> all of them, an int, or one per
        query (array).  Needs finalize() and set_signals(); no embeddings.  At most 64 terms per query.  Host arrays in, numpy
        records out; torch CUDA tensors in, an int64 [B, n_buckets, 8] tensor holding the records' bits out (asynchronous on
        the ctx stream).  Records of shards add."""
        spec = _lib.MentionSpec(_lib.OI_MENTION_AXIS_TIME, int(stamp_origin), int(bucket_width), int(n_buckets))
        return self._mention(query_terms, q_term_offsets, spec, min_match, filters)

    def mention_groups(self, query_terms, q_term_offsets, key_mask: int, n_keys: int, min_match=None, filters=None):
        """oi_mention_summary on the key axis: [B, n_keys] records, one per key = (group & key_mask) >> ctz(key_mask) of the
        documents' group attribute (a ticker id, say); a key >= n_keys belongs to no record.  Everything else as
        mention_summary (filters carry a time window)."""
        spec = _lib.MentionSpec(_lib.OI_MENTION_AXIS_KEY, int(key_mask), 0, int(n_keys))
        return self._mention(query_terms, q_term_offsets, spec, min_match, filters)

    def mention_summary_text(self, texts, min_match=None, n_buckets: int = 1, stamp_origin: int = 0, bucket_width: int = 0,
                             filters=None):
        """mention_summary with the queries given as text: query_terms(texts), then the call."""
        qt, qo = self.query_terms(texts)
        return self.mention_summary(qt, qo, min_match=min_match, n_buckets=n_buckets, stamp_origin=stamp_origin,
                                    bucket_width=bucket_width, filters=filters)

    def mention_groups_text(self, texts, key_mask: int, n_keys: int, min_match=None, filters=None):
        """mention_groups with the queries given as text: query_terms(texts), then the call."""
        qt, qo = self.query_terms(texts)
        return self.mention_groups(qt, qo, key_mask, n_keys, min_match=min_match, filters=filters)

    # ---------------------------------------------------------------- narrative discovery
    def label_sums(self, labels, n_clusters: int):
        """oi_label_sums, the update step of a clustering: (sums int64 [n_clusters, dim], counts uint64 [n_clusters]) over the
        rows d with labels[d] < n_clusters -- counts[labels[d]] += 1, sums[labels[d]] += rint(row_d * 2^30) as 64-bit integers
        (NaN -> 0, clamped to [-1, 1]).  Any other label, 0xFFFFFFFF included, is "no cluster".  Exact: the same bits on every
        run, and the sums of document shards add.  labels: [n_docs] uint32 by local row as similar_share(labels=True)
        returns them; numpy in, numpy out; torch CUDA tensor in, tensors out (counts as int64; asynchronous)."""
        K = int(n_clusters)
        dev = _is_dev(labels)
        rows_out = max(min(K, _lib.OI_MAX_CENTROIDS), 1)            # (a count out of range is refused by the library, not here)
        if dev:
            import torch
            assert labels.is_contiguous() and labels.numel() == self.n_docs and labels.element_size() == 4
            sums = torch.zeros((rows_out, self.dim), dtype=torch.int64, device="cuda:%d" % self.ctx.device)
            counts = torch.zeros((rows_out,), dtype=torch.int64, device="cuda:%d" % self.ctx.device)
        else:
            labels = _np(labels, np.uint32)
            assert labels.size == self.n_docs
            sums = np.zeros((rows_out, self.dim), dtype=np.int64)
            counts = np.zeros((rows_out,), dtype=np.uint64)
        _lib.check(self.lib.oi_label_sums(self.handle, _lib.ptr(labels), K, _lib.OI_DEVICE if dev else _lib.OI_HOST,
                                          _lib.ptr(sums), _lib.ptr(counts)))
        return sums, counts

    def label_term_counts(self, labels, n_clusters: int):
        """oi_label_term_counts: (counts uint32 [vocab, n_clusters], sizes uint64 [n_clusters]) -- counts[t, c] = local documents
        with labels[d] == c that hold term t (once per document), sizes[c] = rows with labels[d] == c.  Any label >=
        n_clusters, 0xFFFFFFFF included, is "no cluster".  Exact integers: the same bits on every run, and the tables and sizes
        of document shards add (then rank_label_terms the total).  Needs a finalized index, no embeddings.  labels as in
        label_sums; numpy in, numpy out; torch CUDA tensor in, tensors out (counts int32 holding the u32 bits, sizes int64;
        asynchronous)."""
        K = int(n_clusters)
        dev = _is_dev(labels)
        cols = max(min(K, _lib.OI_MAX_CENTROIDS), 1)                # (a count out of range is refused by the library, not here)
        if dev:
            import torch
            assert labels.is_contiguous() and labels.numel() == self.n_docs and labels.element_size() == 4
            counts = torch.zeros((self.vocab, cols), dtype=torch.int32, device="cuda:%d" % self.ctx.device)
            sizes = torch.zeros((cols,), dtype=torch.int64, device="cuda:%d" % self.ctx.device)
        else:
            labels = _np(labels, np.uint32)
            assert labels.size == self.n_docs
            counts = np.zeros((self.vocab, cols), dtype=np.uint32)
            sizes = np.zeros((cols,), dtype=np.uint64)
        _lib.check(self.lib.oi_label_term_counts(self.handle, _lib.ptr(labels), K, _lib.OI_DEVICE if dev else _lib.OI_HOST,
                                                 _lib.ptr(counts), _lib.ptr(sizes)))
        return counts, sizes

    def label_terms(self, labels, n_clusters: int, top: int = 10, min_df: int = 1):
        """oi_label_terms: the distinguishing terms of every cluster of a labelling -> (records [n_clusters, top], n
        [n_clusters], sizes [n_clusters]).  Per cluster the eligible terms (counts[t, c] >= max(min_df, 1)) in the order
        excess descending, counts descending, term ascending, where excess = counts[t, c] * A - sizes[c] * dfA[t] (A times
        observed minus expected); records beyond n[c] have term 0xFFFFFFFF.  The table stays in the ctx workspace.  numpy
        labels: records as _lib.LABEL_TERM_DTYPE, n uint32, sizes uint64; torch CUDA labels: records as an int64 tensor
        [n_clusters, top, 3] (label_term_records views it), n int32, sizes int64; asynchronous."""
        K = int(n_clusters)
        dev = _is_dev(labels)
        spec = _lib.LabelTermsSpec(int(top), int(min_df), (C.c_uint32 * 2)(0, 0))
        rows, cols = max(min(K, _lib.OI_MAX_CENTROIDS), 1), max(min(int(top), _lib.OI_MAX_LABEL_TERMS), 1)
        if dev:
            import torch
            assert labels.is_contiguous() and labels.numel() == self.n_docs and labels.element_size() == 4
            where = "cuda:%d" % self.ctx.device
            rec = torch.zeros((rows, cols, 3), dtype=torch.int64, device=where)
            n = torch.zeros((rows,), dtype=torch.int32, device=where)
            sizes = torch.zeros((rows,), dtype=torch.int64, device=where)
        else:
            labels = _np(labels, np.uint32)
            assert labels.size == self.n_docs
            rec = np.zeros((rows, cols), dtype=_lib.LABEL_TERM_DTYPE)
            n = np.zeros((rows,), dtype=np.uint32)
            sizes = np.zeros((rows,), dtype=np.uint64)
        _lib.check(self.lib.oi_label_terms(self.handle, _lib.ptr(labels), K, C.byref(spec), _lib.OI_DEVICE if dev else _lib.OI_HOST,
                                           _lib.ptr(rec), _lib.ptr(n), _lib.ptr(sizes)))
        return rec, n, sizes

    def label_exemplars(self, labels, centroids, top: int = 10, filter=None) -> "RankedLists":
        """oi_label_exemplars: the posts to quote -- per cluster of a labelling, its member rows closest to its centroid, as
        ranked lists [n_clusters, top] in cos_scores / cos_docs / cos_counts of a RankedLists (the bm25 fields are None).  A
        member of cluster c has labels[d] == c < n_clusters, passes `filter` (ONE {group_mask, group_value, stamp_lo,
        stamp_hi}, or None) and has a sim to centroids[c] that is not NaN; the order is score descending, then the smaller
        doc id; docs are global ids; entries beyond cos_counts[c] are score 0, doc 0xFFFFFFFF.  The scores are the sims
        similar_share compares, bit for bit.  The lists feed collapse_lists and merge_lists as they are.  labels as in
        label_sums; numpy labels in, numpy out; torch CUDA labels in (centroids are moved to the device if they are not
        there), tensors out, asynchronous."""
        dev = _is_dev(labels)
        K = int(centroids.shape[0])
        assert K == 0 or int(centroids.shape[1]) == self.dim
        spec = _lib.ExemplarSpec(int(top), (C.c_uint32 * 3)(0, 0, 0))
        rows, cols = max(min(K, _lib.OI_MAX_CENTROIDS), 1), max(min(int(top), _lib.OI_MAX_DEPTH), 1)   # (refused by the library, not here)
        if dev:
            import torch
            assert labels.is_contiguous() and labels.numel() == self.n_docs and labels.element_size() == 4
            if not _is_dev(centroids):
                centroids = torch.from_numpy(_np(centroids, np.float32)).to("cuda:%d" % self.ctx.device)
            assert centroids.is_contiguous() and centroids.element_size() == 4
            self._exemplar_keep = centroids  # (an asynchronous call reads it later)
        else:
            labels = _np(labels, np.uint32)
            assert labels.size == self.n_docs
            centroids = _np(centroids.cpu().numpy() if _is_dev(centroids) else centroids, np.float32)
        f = None
        if filter is not None:
            fa = np.ascontiguousarray(np.asarray(filter.cpu().numpy() if _is_dev(filter) else filter).astype(np.uint32, copy=False).reshape(4))
            f = _lib.DocFilter(int(fa[0]), int(fa[1]), int(fa[2]), int(fa[3]))
        out = RankedLists(self._alloc(dev, (rows, cols), np.float32), self._alloc(dev, (rows, cols), np.uint32),
                          self._alloc(dev, (rows,), np.uint32), None, None, None)
        _lib.check(self.lib.oi_label_exemplars(self.handle, _lib.ptr(labels), _lib.ptr(centroids), K, C.byref(spec),
                                               None if f is None else C.byref(f), _lib.OI_DEVICE if dev else _lib.OI_HOST,
                                               _lib.ptr(out.cos_scores), _lib.ptr(out.cos_docs), _lib.ptr(out.cos_counts)))
        return out

    def _label_summary(self, labels, n_clusters, spec, filter):
        """One oi_label_summary call: numpy labels in, numpy out; torch CUDA labels in, tensors out (asynchronous)."""
        from .analyzer import COUNTERS_DTYPE
        K = int(n_clusters)
        dev = _is_dev(labels)
        top = int(spec.top)
        rows = max(min(K, _lib.OI_MAX_CENTROIDS), 1)                # (a count out of range is refused by the library, not here)
        per_c = max(min(top, _lib.OI_MAX_DEPTH) if top else min(int(spec.n_cells), _lib.OI_MAX_GROUP_CELLS // rows), 1)
        if dev:
            import torch
            assert labels.is_contiguous() and labels.numel() == self.n_docs and labels.element_size() == 4
            self._label_summary_keep = labels  # (an asynchronous call reads it later)
            records = torch.zeros((rows, per_c, 8), dtype=torch.int64, device="cuda:%d" % self.ctx.device)
        else:
            labels = _np(labels, np.uint32)
            assert labels.size == self.n_docs
            records = np.zeros((rows, per_c), dtype=COUNTERS_DTYPE)
        f = None
        if filter is not None:
            fa = np.ascontiguousarray(np.asarray(filter.cpu().numpy() if _is_dev(filter) else filter).astype(np.uint32, copy=False).reshape(4))
            f = _lib.DocFilter(int(fa[0]), int(fa[1]), int(fa[2]), int(fa[3]))
        keys = counts = qualified = None
        if top:
            keys, counts, qualified = (self._alloc(dev, (rows, per_c), np.uint32), self._alloc(dev, (rows,), np.uint32),
                                       self._alloc(dev, (rows,), np.uint32))
        _lib.check(self.lib.oi_label_summary(self.handle, _lib.ptr(labels), K, C.byref(spec), None if f is None else C.byref(f),
                                             _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(records), _lib.ptr(keys),
                                             _lib.ptr(counts), _lib.ptr(qualified)))
        return GroupRanking(keys, records, counts, qualified) if top else records

    def label_summary(self, labels, n_clusters: int, n_buckets: int = 1, stamp_origin: int = 0, bucket_width: int = 0, filter=None):
        """oi_label_summary on the time axis: how each cluster of a labelling developed over time -- [n_clusters, n_buckets]
        records (analyzer.COUNTERS_DTYPE) of the social_summary sums over the rows d with labels[d] == c < n_clusters that pass
        `filter` (ONE {group_mask, group_value, stamp_lo, stamp_hi}, or None) and fall into bucket (stamp - stamp_origin) //
        bucket_width (bucket_width = 0: one bucket).  Any other label, 0xFFFFFFFF included, is "no cluster".  Needs
        set_signals(), and set_doc_attrs() with a time axis or a filter; no embeddings.  With the labels, axis and filter of a
        similar_share or fit_narratives call the records are that call's, bit for bit.  Exact integers; records of shards add.
        labels as in label_sums; numpy labels in, numpy out; torch CUDA labels in, an int64 [n_clusters, n_buckets, 8] tensor
        holding the records' bits out (asynchronous on the ctx stream)."""
        spec = _lib.LabelSummarySpec(_lib.OI_LABEL_AXIS_TIME, int(stamp_origin), int(bucket_width), int(n_buckets), 0, 0, 0, 0)
        return self._label_summary(labels, n_clusters, spec, filter)

    def label_groups(self, labels, n_clusters: int, key_mask: int, n_keys: int, top: int = 0, rank_by="total", min_total: int = 0,
                     filter=None):
        """oi_label_summary on the key axis: which tickers each cluster of a labelling is about -- one record per key =
        (group & key_mask) >> ctz(key_mask) of the documents' group attribute; a key >= n_keys belongs to no record.  top == 0:
        [n_clusters, n_keys] records, what shards add.  top >= 1: a GroupRanking as similar_groups returns it, with "query"
        replaced by "cluster": the best `top` keys per cluster by rank_by ("total", "spec", "bullish", "bearish", or an
        OI_GROUP_RANK_* value; ties by key ascending) among the keys with total >= max(min_total, 1).  Everything else as
        label_summary (the filter carries a time window)."""
        by = GROUP_RANKS[rank_by] if isinstance(rank_by, str) else int(rank_by)
        spec = _lib.LabelSummarySpec(_lib.OI_LABEL_AXIS_KEY, int(key_mask), 0, int(n_keys), int(top), by if int(top) else 0,   # (dense: no ranking)
                                     int(min_total), 0)
        return self._label_summary(labels, n_clusters, spec, filter)

    def fit_narratives(self, seeds, threshold: float, max_iters: int = 20, n_buckets: int = 1, stamp_origin: int = 0,
                       bucket_width: int = 0, filter=None, labels: bool = False) -> "NarrativeFit":
        """oi_narratives_fit: k-means over the index on the device.  Starting from seeds [K, dim], similar_share (one
        threshold, `filter` -- ONE {group_mask, group_value, stamp_lo, stamp_hi} -- for every cluster) and the centroid update
        (label_sums + centroids_from_sums) alternate until a step moves no row or max_iters assignment steps ran.  The result
        describes the last assignment step: similar_share(fit.centroids, ...) reproduces fit.records and fit.labels bit for
        bit.  An empty cluster keeps its vector.  numpy seeds in, numpy out; torch CUDA tensor in, tensors out.  The call
        synchronises the ctx stream (it reads the moved count once per step)."""
        from .analyzer import COUNTERS_DTYPE
        dev = _is_dev(seeds)
        if dev:
            import torch
            assert seeds.is_contiguous() and seeds.element_size() == 4
        else:
            seeds = _np(seeds, np.float32)
        K = int(seeds.shape[0])
        assert K == 0 or int(seeds.shape[1]) == self.dim
        nb = max(int(n_buckets), 0)
        spec = _lib.NarrativeSpec(float(threshold), int(stamp_origin), int(bucket_width), int(n_buckets), int(max_iters))
        if dev:
            cent = torch.zeros((K, self.dim), dtype=torch.float32, device="cuda:%d" % self.ctx.device)
            rec = torch.zeros((K, nb, 8), dtype=torch.int64, device="cuda:%d" % self.ctx.device)
        else:
            cent = np.zeros((K, self.dim), dtype=np.float32)
            rec = np.zeros((K, nb), dtype=COUNTERS_DTYPE)
        lab = self._alloc(dev, (self.n_docs,), np.uint32) if labels else None
        f = None
        if filter is not None:
            fa = np.ascontiguousarray(np.asarray(filter.cpu().numpy() if _is_dev(filter) else filter).astype(np.uint32, copy=False).reshape(4))
            f = _lib.DocFilter(int(fa[0]), int(fa[1]), int(fa[2]), int(fa[3]))
        info = _lib.NarrativeInfo()
        _lib.check(self.lib.oi_narratives_fit(self.handle, _lib.ptr(seeds), K, C.byref(spec), None if f is None else C.byref(f),
                                              _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(cent), _lib.ptr(rec), _lib.ptr(lab),
                                              C.byref(info)))
        return NarrativeFit(cent, rec, lab, int(info.iterations), bool(info.converged), int(info.moved), int(info.assigned))

    SEED_METHODS = {"kmeans++": _lib.OI_SEED_KMEANSPP, "farthest": _lib.OI_SEED_FARTHEST}

    def seed_narratives(self, n_clusters: int, method="kmeans++", trials: int = 4, seed: int = 0, n_buckets: int = 1,
                        stamp_origin: int = 0, bucket_width: int = 0, filter=None, device: bool = False) -> "NarrativeSeeds":
        """oi_narratives_seed: n_clusters stored rows of the index chosen as seeds for fit_narratives, on the device -- greedy
        k-means++ (method "kmeans++": D^2 sampling with integer weights rint((1 - sim) * 2^20), the best of `trials` candidates
        per seed) or farthest-first ("farthest", trials = 1).  Only rows that pass `filter` (ONE {group_mask, group_value,
        stamp_lo, stamp_hi}) and have a bucket are eligible: the rows fit_narratives assigns from.  The result is a function
        of the arguments alone (the RNG is splitmix64 of `seed`).  Seeds at and beyond `found` (every eligible row already
        coincides with a seed) are zero vectors with row 0xFFFFFFFF.  numpy out; torch CUDA tensors when device=True."""
        K = int(n_clusters)
        m = self.SEED_METHODS.get(method, method)
        spec = _lib.SeedSpec(int(m), int(trials), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stamp_origin), int(bucket_width), int(n_buckets), 0)
        shape_k = max(min(K, _lib.OI_MAX_CENTROIDS), 1)            # (a count out of range is refused by the library, not here)
        seeds = self._alloc(device, (shape_k, self.dim), np.float32)
        rows = self._alloc(device, (shape_k,), np.uint32)
        f = None
        if filter is not None:
            fa = np.ascontiguousarray(np.asarray(filter.cpu().numpy() if _is_dev(filter) else filter).astype(np.uint32, copy=False).reshape(4))
            f = _lib.DocFilter(int(fa[0]), int(fa[1]), int(fa[2]), int(fa[3]))
        info = _lib.SeedInfo()
        _lib.check(self.lib.oi_narratives_seed(self.handle, K, C.byref(spec), None if f is None else C.byref(f),
                                               _lib.OI_DEVICE if device else _lib.OI_HOST, _lib.ptr(seeds), _lib.ptr(rows), C.byref(info)))
        return NarrativeSeeds(seeds, rows, int(info.found), int(info.eligible), int(info.potential))

    # ---------------------------------------------------------------- the sharded query with RCCL inside the library
    def finalize_sharded(self, comm: "NativeComm") -> None:
        """Collective over `comm`: all-reduce of (n_docs, tokens, df) inside the library, then the impacts from the global
        statistics (oi_index_finalize_sharded) -- what ShardedRetriever.finalize does with torch.distributed."""
        _lib.check(self.lib.oi_index_finalize_sharded(self.handle, comm.handle))

    def search_sharded(self, comm: "NativeComm", query_vecs, query_terms, q_term_offsets, k: int = DEFAULT_K,
                       depth: int = DEFAULT_DEPTH, out: Optional[SearchResult] = None, filters=None) -> SearchResult:
        """Collective over `comm`, same queries on every rank: this shard's lists -> ONE ncclAllGather -> global merge ->
        RRF, in one C call (oi_search_sharded).  Identical result on every rank."""
        dev, B, qv, qt, qo = self._queries(query_vecs, query_terms, q_term_offsets)
        if out is None:
            out = SearchResult(self._alloc(dev, (B, k), np.float32), self._alloc(dev, (B, k), np.uint32),
                               self._alloc(dev, (B,), np.uint32))
        if filters is not None:
            f = self._filters(filters, dev, B)
            _lib.check(self.lib.oi_search_sharded_filtered(self.handle, comm.handle, _lib.ptr(qv), _lib.ptr(qt), _lib.ptr(qo),
                                                           B, int(depth), int(k), _lib.ptr(f),
                                                           _lib.OI_DEVICE if dev else _lib.OI_HOST,
                                                           _lib.ptr(out.scores), _lib.ptr(out.docs), _lib.ptr(out.counts)))
            return out
        _lib.check(self.lib.oi_search_sharded(self.handle, comm.handle, _lib.ptr(qv), _lib.ptr(qt), _lib.ptr(qo), B,
                                              int(depth), int(k), _lib.OI_DEVICE if dev else _lib.OI_HOST,
                                              _lib.ptr(out.scores), _lib.ptr(out.docs), _lib.ptr(out.counts)))
        return out

    def screen_probe(self, query_vecs, row_begin: int = 0, n_rows: int = 0):
        """Diagnostics of the bf16 screen (oi_screen_probe): (s~ [B, n_rows] or None, eps [B]) for host queries --
        the screen's raw scores of rows [row_begin, row_begin + n_rows) and each query's proven bound."""
        qv = _np(query_vecs, np.float32)
        B = int(qv.shape[0])
        assert int(qv.shape[1]) == self.dim
        st = np.zeros((B, n_rows), np.float32) if n_rows else None
        eps = np.zeros(B, np.float32)
        _lib.check(self.lib.oi_screen_probe(self.handle, _lib.ptr(qv), B, int(row_begin), int(n_rows), _lib.ptr(st),
                                            _lib.ptr(eps)))
        return st, eps

    def view(self, ctx: HipContext) -> "HybridIndex":
        """A second handle on this (finalized) shard, bound to `ctx` -- another HipContext of the same device, with its
        own stream and workspaces -- so that two searches can be in flight at once (oi_index_view).  Borrows every
        buffer: read-only, no HBM; close it before this index."""
        v = HybridIndex.__new__(HybridIndex)
        v.ctx, v.lib = ctx, ctx.lib
        v.n_docs, v.dim, v.vocab, v.doc_id_base = self.n_docs, self.dim, self.vocab, self.doc_id_base
        h = C.c_void_p()
        _lib.check(self.lib.oi_index_view(self.handle, ctx.handle, C.byref(h)))
        v.handle = h
        v._keep = [self]  # the source outlives the view
        return v

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.oi_index_destroy(self.handle)
            self.handle = None
            self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativeComm:
    """An RCCL communicator owned by the library (oi_comm_*): the multi-GPU exchange without torch.distributed.

        id = NativeComm.unique_id()            # rank 0; ship the 128 bytes to the other ranks over any host channel
        comm = NativeComm(ctx, id, rank, world)  # collective
        idx.finalize_sharded(comm); idx.search_sharded(comm, qv, qt, qo, k, depth)

    Collectives run on the ctx stream in call order; every rank issues them in the same order."""

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * _lib.OI_COMM_ID_BYTES)()
        _lib.check(_lib.load().oi_comm_unique_id(C.cast(buf, C.c_void_p)))
        return bytes(buf)

    def __init__(self, ctx: HipContext, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == _lib.OI_COMM_ID_BYTES
        self.ctx, self.rank, self.world = ctx, int(rank), int(world)
        buf = (C.c_uint8 * _lib.OI_COMM_ID_BYTES).from_buffer_copy(unique_id)
        h = C.c_void_p()
        _lib.check(ctx.lib.oi_comm_create(ctx.handle, C.cast(buf, C.c_void_p), self.rank, self.world, C.byref(h)))
        self.handle = h

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.ctx.lib.oi_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NativePipeline:
    """Several batches in flight through the library's own lanes (oi_pipeline_*): the pipelined -- and, with a NativeComm,
    row-sharded -- query without torch streams or torch.distributed on the data path.

        pipe = NativePipeline(idx, lanes=2, max_queries=64, max_query_terms=4, depth=1000, k=100)   # comm=NativeComm(...) to shard
        t = pipe.submit(qv, qt, qo, out=result_slot)     # asynchronous (device tensors or numpy arrays)
        pipe.wait(t)                                     # that batch's outputs are complete
        pipe.drain(); pipe.close()

    Device batches: `out` (a SearchResult of device tensors, shape (n_queries, k)) must be a distinct buffer per batch in
    flight; inputs stay unmodified until wait().  Results are bit-identical to HybridIndex.search / search_sharded."""

    def __init__(self, index: "HybridIndex", lanes: int = 2, max_queries: int = 64, max_query_terms: int = 16,
                 depth: int = DEFAULT_DEPTH, k: int = DEFAULT_K, comm: Optional["NativeComm"] = None):
        self.index, self.lib, self.comm = index, index.lib, comm
        self.k, self.depth, self.max_queries = int(k), int(depth), int(max_queries)
        h = C.c_void_p()
        _lib.check(self.lib.oi_pipeline_create(index.handle, comm.handle if comm is not None else None, int(lanes),
                                               int(max_queries), int(max_query_terms), int(depth), int(k), C.byref(h)))
        self.handle = h
        self._keep = {}   # ticket -> (inputs, outputs): host arrays / tensors the library still reads or writes

    def submit(self, query_vecs, query_terms, q_term_offsets, out: Optional[SearchResult] = None):
        dev, B, qv, qt, qo = self.index._queries(query_vecs, query_terms, q_term_offsets)
        if out is None:
            out = SearchResult(self.index._alloc(dev, (B, self.k), np.float32), self.index._alloc(dev, (B, self.k), np.uint32),
                               self.index._alloc(dev, (B,), np.uint32))
        t = C.c_uint64()
        _lib.check(self.lib.oi_pipeline_submit(self.handle, _lib.ptr(qv), _lib.ptr(qt), _lib.ptr(qo), B,
                                               _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(out.scores), _lib.ptr(out.docs),
                                               _lib.ptr(out.counts), C.byref(t)))
        self._keep[int(t.value)] = ((qv, qt, qo), out)
        if len(self._keep) > 64:
            for old in sorted(self._keep)[:-32]:      # (slots that old were reused long ago: the library is done with them)
                del self._keep[old]
        return int(t.value), out

    def wait(self, ticket: int, host_sync: bool = True) -> None:
        _lib.check(self.lib.oi_pipeline_wait(self.handle, int(ticket), 1 if host_sync else 0))
        if host_sync:
            self._keep.pop(int(ticket), None)

    def drain(self) -> None:
        _lib.check(self.lib.oi_pipeline_drain(self.handle))
        self._keep.clear()

    def workspace_bytes(self):
        a, b = C.c_uint64(), C.c_uint64()
        _lib.check(self.lib.oi_pipeline_workspace_bytes(self.handle, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def concurrent_streams(self):
        """(how many of the pipeline's streams were measured to run at the same time, how many it has): oi_pipeline_concurrent_streams."""
        a, b = C.c_uint32(), C.c_uint32()
        _lib.check(self.lib.oi_pipeline_concurrent_streams(self.handle, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def profile_reset(self, enable) -> None:
        _lib.check(self.lib.oi_pipeline_profile_reset(self.handle, int(enable)))

    def profile_read(self, tag: str):
        """(summed ms, launches) of the lanes' launches with that tag since the last reset (oi_pipeline_profile_read)."""
        ms, n = C.c_double(), C.c_uint64()
        _lib.check(self.lib.oi_pipeline_profile_read(self.handle, tag.encode(), C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.oi_pipeline_destroy(self.handle)
            self.handle = None
            self._keep = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------- list-level ops (any ctx)
def centroids_from_sums(ctx: HipContext, sums, counts, previous=None):
    """oi_centroids_from_sums: integer sums [K, dim] and counts [K] (HybridIndex.label_sums's, or the total of several
    shards') -> unit vectors [K, dim] f32: sums / |sums|, computed in f64 and rounded once.  A cluster with count 0 or an
    all-zero sum keeps previous[c] (zeros when previous is None).  numpy in, numpy out; torch CUDA tensors in, tensor out."""
    dev = _is_dev(sums)
    if dev:
        import torch
        assert sums.is_contiguous() and sums.element_size() == 8 and counts.is_contiguous() and counts.element_size() == 8
        if previous is not None:
            assert _is_dev(previous) and previous.is_contiguous() and previous.element_size() == 4 and tuple(previous.shape) == tuple(sums.shape)
        out = torch.zeros(tuple(sums.shape), dtype=torch.float32, device=sums.device)
    else:
        sums, counts = _np(sums, np.int64), _np(counts, np.uint64)
        if previous is not None:
            previous = _np(previous, np.float32)
            assert previous.shape == sums.shape
        out = np.zeros(sums.shape, dtype=np.float32)
    K, dim = int(sums.shape[0]), int(sums.shape[1])
    assert int(counts.shape[0]) == K
    _lib.check(ctx.lib.oi_centroids_from_sums(ctx.handle, _lib.ptr(sums), _lib.ptr(counts), _lib.ptr(previous), K, dim,
                                              _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(out)))
    return out


def rank_label_terms(ctx: HipContext, counts, sizes, top: int = 10, min_df: int = 1):
    """oi_label_terms_rank: a table [vocab, n_clusters] and sizes [n_clusters] (HybridIndex.label_term_counts's, or the total
    of several shards') -> (records [n_clusters, top], n [n_clusters]) as HybridIndex.label_terms returns them.  The sizes go
    to the host (at most 2 KB; their sum A must be <= 2^31 - 1).  numpy table in, numpy out; torch CUDA table in, tensors
    out."""
    dev = _is_dev(counts)
    sizes_h = _np(sizes.cpu().numpy() if _is_dev(sizes) else sizes, np.uint64)
    vocab, K = int(counts.shape[0]), int(counts.shape[1])
    assert sizes_h.size == K
    spec = _lib.LabelTermsSpec(int(top), int(min_df), (C.c_uint32 * 2)(0, 0))
    cols = max(min(int(top), _lib.OI_MAX_LABEL_TERMS), 1)
    if dev:
        import torch
        assert counts.is_contiguous() and counts.element_size() == 4
        rec = torch.zeros((K, cols, 3), dtype=torch.int64, device=counts.device)
        n = torch.zeros((K,), dtype=torch.int32, device=counts.device)
    else:
        counts = _np(counts, np.uint32)
        rec = np.zeros((K, cols), dtype=_lib.LABEL_TERM_DTYPE)
        n = np.zeros((K,), dtype=np.uint32)
    _lib.check(ctx.lib.oi_label_terms_rank(ctx.handle, _lib.ptr(counts), _lib.ptr(sizes_h), vocab, K, C.byref(spec),
                                           _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(rec), _lib.ptr(n)))
    return rec, n


def label_term_records(records) -> np.ndarray:
    """The records of label_terms / rank_label_terms as a _lib.LABEL_TERM_DTYPE array [n_clusters, top] on the host (a torch
    int64 tensor [n_clusters, top, 3] is copied off the device; a numpy array is returned as it is)."""
    if _is_dev(records):
        a = records.cpu().numpy()
        return a.view(_lib.LABEL_TERM_DTYPE).reshape(a.shape[0], a.shape[1])
    return records


def rrf_fuse(ctx: HipContext, docs_a, counts_a, docs_b, counts_b, k: int) -> SearchResult:
    dev = _is_dev(docs_a)
    if not dev:
        docs_a, docs_b = _np(docs_a, np.uint32), _np(docs_b, np.uint32)
        counts_a, counts_b = _np(counts_a, np.uint32), _np(counts_b, np.uint32)
    B, depth = int(docs_a.shape[0]), int(docs_a.shape[1])
    if dev:
        import torch
        mk = lambda shape, dt: torch.zeros(shape, dtype=dt, device=docs_a.device)
        out = SearchResult(mk((B, k), torch.float32), mk((B, k), torch.int32), mk((B,), torch.int32))
    else:
        out = SearchResult(np.zeros((B, k), np.float32), np.zeros((B, k), np.uint32), np.zeros(B, np.uint32))
    _lib.check(ctx.lib.oi_rrf_fuse(ctx.handle, _lib.ptr(docs_a), _lib.ptr(counts_a), _lib.ptr(docs_b),
                                   _lib.ptr(counts_b), B, depth, int(k),
                                   _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(out.scores),
                                   _lib.ptr(out.docs), _lib.ptr(out.counts)))
    return out


def fuse_packed(ctx: HipContext, packed_all, n_shards: int, n_queries: int, depth: int, k: int,
                out: Optional[SearchResult] = None) -> SearchResult:
    """All shards' packed lists ([n_shards * OI_PACKED_WORDS] words) -> global top-depth per list -> RRF top-k."""
    dev = _is_dev(packed_all)
    if not dev:
        packed_all = np.ascontiguousarray(packed_all).view(np.uint32)
    if out is None:
        if dev:
            import torch
            mk = lambda shape, dt: torch.zeros(shape, dtype=dt, device=packed_all.device)
            out = SearchResult(mk((n_queries, k), torch.float32), mk((n_queries, k), torch.int32),
                               mk((n_queries,), torch.int32))
        else:
            out = SearchResult(np.zeros((n_queries, k), np.float32), np.zeros((n_queries, k), np.uint32),
                               np.zeros(n_queries, np.uint32))
    _lib.check(ctx.lib.oi_fuse_packed(ctx.handle, _lib.ptr(packed_all), int(n_shards), int(n_queries), int(depth),
                                      int(k), _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(out.scores),
                                      _lib.ptr(out.docs), _lib.ptr(out.counts)))
    return out


def merge_lists(ctx: HipContext, scores, docs, counts):
    """[S, B, depth] per-shard lists (+ counts [S, B]) -> global top-depth per query."""
    dev = _is_dev(scores)
    if not dev:
        scores, docs, counts = _np(scores, np.float32), _np(docs, np.uint32), _np(counts, np.uint32)
    S, B, depth = (int(x) for x in scores.shape)
    if dev:
        import torch
        mk = lambda shape, dt: torch.zeros(shape, dtype=dt, device=scores.device)
        so, do, co = mk((B, depth), torch.float32), mk((B, depth), torch.int32), mk((B,), torch.int32)
    else:
        so, do, co = np.zeros((B, depth), np.float32), np.zeros((B, depth), np.uint32), np.zeros(B, np.uint32)
    _lib.check(ctx.lib.oi_merge_lists(ctx.handle, _lib.ptr(scores), _lib.ptr(docs), _lib.ptr(counts), S, B, depth,
                                      _lib.OI_DEVICE if dev else _lib.OI_HOST, _lib.ptr(so), _lib.ptr(do),
                                      _lib.ptr(co)))
    return so, do, co
