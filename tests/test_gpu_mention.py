"""Mention summary (oi_mention_summary): out[q][c] = the social_summary raw sums over the documents that hold at
least need_q of query q's DISTINCT terms, pass filters[q] and fall into cell c (a time bucket, or a key of the group).

The reference is numpy in this file, over the test's own forward index: per query the set of distinct terms, per term the
documents that hold it, m(q, d) as a sum of those indicator vectors, then the three clauses and integer sums per cell
(float(int(sum of rint(v * 2^30))) * 2^-30 for the polarity sum).  All eight fields are compared for equality.  Documents have
1 .. 6 tokens (the two documents of the 64-term case aside), the vocabulary is 4096 ids, and no index has embeddings except
where a view or oi_search_lists needs them (dim 16)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
VOCAB = 4096
TAU = 0.2
BLOCK = 32768
ALL_DOCS = (0, 0, 0, 0xFFFFFFFF)
NO_DOCS = (0, 0, 7, 6)
# every class x speculative x source combination occurs; 0 gives pol_q30 = 0, +-1 give +-2^30; 1/3 is not dyadic
VALS = np.array([-1.0, -1.0 / 3.0, 0.0, 0.25, 1.0, 0.0, 1.0, -1.0])
COMMON = np.array([3, 17, 64, 255, 256, 1000, 2047, 2048, 3000, 4095], dtype=np.uint32)   # the terms of the random corpora
EDGE0 = 3500                                                                               # planted terms: EDGE0 + i


def _dtype():
    from openintel_amd.analyzer import COUNTERS_DTYPE
    return COUNTERS_DTYPE


def _ctx():
    import openintel_amd as oi
    return oi.HipContext(0)


class _Sig:
    def __init__(self, pol, spec, src):
        self.pol, self.spec, self.src = pol, spec, src
        v = np.where(np.isnan(pol), 0.0, np.clip(pol, -1.0, 1.0))
        self.q30 = np.rint(v * 2.0 ** 30).astype(np.int64)
        self.bull, self.bear = v > TAU, v < -TAU
        self.neu = ~self.bull & ~self.bear
        self.sp = spec != 0
        self.s1 = src != 0


def _signals(n, seed=0, vals=VALS):
    rng = np.random.default_rng(500 + seed)
    i = np.arange(n)
    # the first 4 * len(vals) documents walk through every (value, spec, source) combination; the rest are random
    pol = np.where(i < 4 * vals.size, vals[i % vals.size], vals[rng.integers(0, vals.size, size=n)])
    spec = np.where(i < 4 * vals.size, (i // vals.size) & 1, rng.integers(0, 2, size=n)).astype(np.uint8)
    src = np.where(i < 4 * vals.size, (i // vals.size) >> 1, rng.integers(0, 2, size=n)).astype(np.uint8)
    return _Sig(pol, spec, src)


class _Fwd:
    """A forward index and, for the reference, the documents of every term."""

    def __init__(self, terms, offs):
        self.terms, self.offs = np.asarray(terms, np.uint32), np.asarray(offs, np.uint64)
        self.n = self.offs.size - 1
        doc_of = np.repeat(np.arange(self.n), np.diff(self.offs.astype(np.int64)))
        order = np.argsort(self.terms, kind="stable")
        self._sorted, self._docs = self.terms[order], doc_of[order]

    def has(self, t):
        """bool [n]: the documents with a posting for term t"""
        lo, hi = np.searchsorted(self._sorted, [t, t + 1])
        out = np.zeros(self.n, bool)
        out[self._docs[lo:hi]] = True
        return out


def _fwd_from_docs(docs):
    offs = np.zeros(len(docs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    return _Fwd(np.array([t for d in docs for t in d], np.uint32), offs)


@functools.lru_cache(maxsize=None)
def _random_fwd(n, seed=0):
    """n documents of 1 .. 6 tokens over COMMON (a document may repeat a term), and one planted term per edge document."""
    rng = np.random.default_rng(seed + n)
    lens = rng.integers(1, 7, size=n)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    terms = COMMON[rng.integers(0, COMMON.size, size=int(offs[-1]))]
    for i, d in enumerate(_edge_docs(n)):
        terms[int(offs[d])] = EDGE0 + i                      # the document's first token (it keeps its other tokens)
    return _Fwd(terms, offs)


def _edge_docs(n):
    """document 0, 16383 | 16384, the last of block 0 | the first of block 1, the last document of the (ragged) last block"""
    return [d for d in dict.fromkeys([0, 16383, 16384, BLOCK - 1, BLOCK, 2 * BLOCK - 1, 2 * BLOCK, n - 1]) if d < n]


def _index(ctx, fwd, sig=None, group=None, stamp=None, finalize=True, dim=4, rows=None):
    import openintel_amd as oi
    idx = oi.HybridIndex(ctx, fwd.n, dim, VOCAB)
    if rows is not None:
        idx.set_embeddings(rows, normalize=True)
    idx.set_forward(fwd.terms if fwd.terms.size else np.zeros(1, np.uint32), fwd.offs)
    if group is not None or stamp is not None:
        idx.set_doc_attrs(group, stamp)
    if sig is not None:
        idx.set_signals(sig.pol, sig.spec, sig.src, TAU)
    if finalize:
        idx.finalize()
    return idx


def _pack(queries):
    offs = np.zeros(len(queries) + 1, np.uint32)
    offs[1:] = np.cumsum([len(q) for q in queries])
    return np.array([t for q in queries for t in q], np.uint32), offs


def _need(min_match, q, nd):
    if min_match is None or (isinstance(min_match, str) and min_match == "any"):
        return 1
    mm = 0 if (isinstance(min_match, str) and min_match == "all") else (int(min_match) if np.ndim(min_match) == 0 else int(min_match[q]))
    return nd if mm == 0 else mm


def _passes(f, group, stamp):
    m, v, lo, hi = (int(x) for x in f)
    return ((group & np.uint32(m)) == np.uint32(v)) & (stamp >= np.uint32(lo)) & (stamp <= np.uint32(hi))


def _ref(fwd, queries, sig, min_match=None, n_cells=1, origin=0, width=0, key_mask=None, group=None, stamp=None, filters=None):
    """The definition, clause by clause -> [B][n_cells] records.  key_mask set: the KEY axis."""
    n = fwd.n
    out = np.zeros((len(queries), n_cells), _dtype())
    if key_mask is not None:
        shift = (key_mask & -key_mask).bit_length() - 1
        cell = ((group.astype(np.int64) & key_mask) >> shift)
        in_cell = cell < n_cells
    elif width:
        s64 = stamp.astype(np.int64)
        cell = (s64 - origin) // width                      # 64-bit: origin + n_cells * width may exceed 2^32
        in_cell = (s64 >= origin) & (cell < n_cells)
    else:
        cell, in_cell = np.zeros(n, np.int64), np.ones(n, bool)
    for q, raw in enumerate(queries):
        if len(raw) > 64:                                    # (the device location's refusal: all-zero records)
            continue
        D = list(dict.fromkeys(int(t) for t in raw))
        m = np.zeros(n, np.int64)
        for t in D:
            if t < VOCAB:                                    # a term outside the vocabulary occurs in no document
                m += fwd.has(t)
        ok = (m >= _need(min_match, q, len(D))) if D else np.zeros(n, bool)
        if filters is not None:
            ok = ok & _passes(filters[q], group, stamp)
        ok = ok & in_cell

        def count(sel):
            return np.bincount(cell[sel], minlength=n_cells)[:n_cells]

        r = out[q]
        r["total"] = count(ok)
        r["by_source"][:, 0], r["by_source"][:, 1] = count(ok & ~sig.s1), count(ok & sig.s1)
        r["bullish"], r["bearish"], r["neutral"] = count(ok & sig.bull), count(ok & sig.bear), count(ok & sig.neu)
        r["spec_count"] = count(ok & sig.sp)
        s = np.zeros(n_cells, np.int64)
        np.add.at(s, cell[ok], sig.q30[ok])
        r["polarity_sum"] = s.astype(np.float64) * 2.0 ** -30
    return out


def _same(got, want):
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype
    if got.tobytes() != want.tobytes():
        bad = [(q, c) for q in range(want.shape[0]) for c in range(want.shape[1]) if got[q, c] != want[q, c]]
        raise AssertionError("%d cells differ, first %s: got %s, want %s" % (len(bad), bad[0], got[bad[0]], want[bad[0]]))


def _host(rec):
    """a device result (int64 [B, n, 8]) as records"""
    return rec.cpu().numpy().view(_dtype()).reshape(rec.shape[0], rec.shape[1])


def _attrs(n, seed=0, n_groups=300, t0=1000, span=5000):
    rng = np.random.default_rng(77 + seed)
    return rng.integers(0, n_groups, size=n).astype(np.uint32), rng.integers(t0, t0 + span, size=n).astype(np.uint32)


# ---------------------------------------------------------------- block and window edges
@pytest.mark.parametrize("n", [1, 16383, 16384, 16385, 32767, 32768, 32769, 65537])
def test_block_and_window_edges(n):
    fwd, sig = _random_fwd(n), _signals(n)
    group, stamp = _attrs(n)
    ctx = _ctx()
    idx = _index(ctx, fwd, sig, group, stamp)
    edges = _edge_docs(n)
    # one query per planted term (its only match is that edge document), then mixed queries over the common terms
    queries = [[EDGE0 + i] for i in range(len(edges))] + [[3], [3, 17], [64, 255, 256], [1000, 2047, 2048, 3000, 4095],
                                                         [EDGE0, 3], [EDGE0 + len(edges) - 1, 17]]
    mm = np.array([1] * len(edges) + [1, 0, 2, 3, 1, 0], np.uint32)
    qt, qo = _pack(queries)
    got = idx.mention_summary(qt, qo, min_match=mm)
    want = _ref(fwd, queries, sig, mm)
    _same(got, want)
    assert [int(r["total"]) for r in want[:len(edges), 0]] == [1] * len(edges)
    _same(idx.mention_summary(qt, qo, min_match=mm, n_buckets=3, stamp_origin=1500, bucket_width=1000),
          _ref(fwd, queries, sig, mm, n_cells=3, origin=1500, width=1000, stamp=stamp))
    _same(idx.mention_groups(qt, qo, 0xFF, 200, min_match=mm), _ref(fwd, queries, sig, mm, n_cells=200, key_mask=0xFF, group=group))


# ---------------------------------------------------------------- packed counters
def test_the_four_byte_counters_of_a_word_are_told_apart():
    a, b, c, other = 100, 200, 300, 400
    docs = []
    for k in range(10):                                      # documents 4k .. 4k+3 hold 0, 1, 2 and 3 of the query's terms
        docs += [[other], [a], [b, c] if k % 2 else [a, c], [a, b, c]]
    fwd, sig = _fwd_from_docs(docs), _signals(len(docs))
    idx = _index(_ctx(), fwd, sig)
    queries = [[a, b, c]] * 5
    mm = np.array([1, 2, 3, 0, 4], np.uint32)
    got = idx.mention_summary(*_pack(queries), min_match=mm)
    _same(got, _ref(fwd, queries, sig, mm))
    assert [int(x) for x in got["total"][:, 0]] == [30, 20, 10, 10, 0]
    # the rotation of the word: the counts 0 .. 3 sit in every byte position
    for rot in range(1, 4):
        f2 = _fwd_from_docs(docs[rot:] + docs[:rot])
        _same(_index(_ctx(), f2, sig).mention_summary(*_pack(queries), min_match=mm), _ref(f2, queries, sig, mm))


def test_a_count_of_64_beside_a_count_of_63():
    q64 = [10 * i + 1 for i in range(64)]
    docs = [[5], q64, q64[:63], [7]]                          # documents 1 and 2 share an LDS word
    fwd, sig = _fwd_from_docs(docs), _signals(4)
    idx = _index(_ctx(), fwd, sig)
    queries = [q64] * 4
    mm = np.array([0, 64, 63, 1], np.uint32)
    got = idx.mention_summary(*_pack(queries), min_match=mm)
    _same(got, _ref(fwd, queries, sig, mm))
    assert [int(x) for x in got["total"][:, 0]] == [1, 1, 2, 2]


# ---------------------------------------------------------------- distinct terms
def test_distinct_terms_vocabulary_and_empty_queries():
    n = 3000
    fwd, sig = _random_fwd(n), _signals(n)
    idx = _index(_ctx(), fwd, sig)
    t, u, unused, outside = 3, 17, 1234, VOCAB + 904         # `unused` has df = 0
    assert not fwd.has(unused).any()

    def run(queries, mm=None):
        got = idx.mention_summary(*_pack(queries), min_match=mm)
        _same(got, _ref(fwd, queries, sig, mm))
        return got

    for mm in (None, "all"):
        g = run([[t, t, u], [t, u]], mm)
        assert g[0].tobytes() == g[1].tobytes()              # a repeated term counts once
    assert run([[t, t]], 2)["total"].sum() == 0               # need 2 > |D| = 1
    g = run([[t, outside], [t]])
    assert g[0].tobytes() == g[1].tobytes() and g["total"][0, 0] > 0     # ANY ignores a term outside the vocabulary
    assert run([[t, outside]], "all")["total"].sum() == 0                # ALL cannot be met with it
    assert run([[t, 0xFFFFFFFF]], "all")["total"].sum() == 0
    assert run([[unused]])["total"].sum() == 0
    g = run([[t, unused], [t]])
    assert g[0].tobytes() == g[1].tobytes()
    assert run([[t, unused]], "all")["total"].sum() == 0
    assert run([[]])["total"].sum() == 0                      # an empty query alone ...
    assert run([[]], "all")["total"].sum() == 0
    g = run([[t], [], [u]])                                   # ... and in the middle of a batch
    assert g["total"][1, 0] == 0 and g["total"][0, 0] > 0 and g["total"][2, 0] > 0
    g = run([[t] * 64, [t]])                                  # 64 raw terms, one distinct term
    assert g[0].tobytes() == g[1].tobytes()
    g = run([[t] * 64, [t]], "all")
    assert g[0].tobytes() == g[1].tobytes() and g["total"][0, 0] > 0
    assert run([[t] * 64], 2)["total"].sum() == 0


def test_total_of_one_term_is_its_local_df():
    n = 40000
    fwd, sig = _random_fwd(n), _signals(n)
    idx = _index(_ctx(), fwd, sig)
    _, df = idx.local_stats()
    terms = [int(t) for t in COMMON] + [EDGE0, 1234]
    got = idx.mention_summary(*_pack([[t] for t in terms]))
    assert [int(x) for x in got["total"][:, 0]] == [int(df[t]) for t in terms]
    assert df[1234] == 0 and df[EDGE0] == 1


# ---------------------------------------------------------------- too many terms, device location
def test_a_65_term_query_on_the_device_gets_zero_records():
    import torch
    n = 3000
    fwd, sig = _random_fwd(n), _signals(n)
    idx = _index(_ctx(), fwd, sig)
    queries = [[3, 17], [int(COMMON[i % COMMON.size]) for i in range(65)], [64]]
    qt, qo = _pack(queries)
    dev = "cuda:0"
    got = _host(idx.mention_summary(torch.from_numpy(qt.view(np.int32)).to(dev), torch.from_numpy(qo.view(np.int32)).to(dev)))
    want = _ref(fwd, queries, sig)
    _same(got, want)
    assert got["total"][1, 0] == 0 and got["total"][0, 0] > 0 and got["total"][2, 0] > 0
    from openintel_amd import _lib
    with pytest.raises(_lib.OiError) as e:                    # the host location sees the offsets and refuses
        idx.mention_summary(qt, qo)
    assert e.value.code == _lib.OI_ERR_INVALID_ARG and "query 1 has 65 terms" in e.value.message


# ---------------------------------------------------------------- a workgroup's second task
def test_counters_are_clean_when_a_workgroup_takes_its_next_task():
    """1024 queries x 3 blocks: more tasks than resident workgroups.  Term A is in EVERY document of the even blocks and in a
    few odd documents of block 1; term B the other way round; the queries alternate [A], [B].  Whether a workgroup's next task
    is the next block of its query or another query of its block, a dense task is followed by a sparse one over other
    documents: counters left behind would be counted."""
    n = 2 * BLOCK + 1
    A, B, pad = 111, 222, 333
    d = np.arange(n)
    blk = d // BLOCK
    sparse = (d % 1021 == 1)
    has_a = np.where(blk % 2 == 0, True, sparse)
    has_b = np.where(blk % 2 == 1, True, (d % 997 == 2))
    docs_t = np.stack([np.where(has_a, A, pad), np.where(has_b, B, pad)], axis=1).astype(np.uint32)
    fwd = _Fwd(docs_t.reshape(-1), np.arange(n + 1, dtype=np.uint64) * 2)
    sig = _signals(n)
    idx = _index(_ctx(), fwd, sig)
    queries = [[A], [B]] * 512
    got = idx.mention_summary(*_pack(queries))
    want2 = _ref(fwd, queries[:2], sig)
    _same(got, np.tile(want2, (512, 1)))
    assert int(want2["total"][0, 0]) == int(has_a.sum()) and int(want2["total"][1, 0]) == int(has_b.sum())


# ---------------------------------------------------------------- a dense and a rare term together
def test_a_term_of_every_document_with_a_term_of_three():
    n = 2 * BLOCK + 1
    dense, rare, pad = 9, 4000, 77
    rare_docs = [5, BLOCK + 7, n - 1]
    second = np.full(n, pad, np.uint32)
    second[rare_docs] = rare
    fwd = _Fwd(np.stack([np.full(n, dense, np.uint32), second], axis=1).reshape(-1), np.arange(n + 1, dtype=np.uint64) * 2)
    pol = np.where(np.arange(n) % 3 == 0, -1.0, 1.0)          # +-2^30 each: the sums pass 2^32 in magnitude
    sig = _Sig(pol, (np.arange(n) % 2).astype(np.uint8), (np.arange(n) % 5 == 0).astype(np.uint8))
    idx = _index(_ctx(), fwd, sig)
    queries = [[dense, rare], [dense, rare], [rare], [dense]]
    mm = np.array([1, 0, 1, 1], np.uint32)
    got = idx.mention_summary(*_pack(queries), min_match=mm)
    _same(got, _ref(fwd, queries, sig, mm))
    assert [int(x) for x in got["total"][:, 0]] == [n, 3, 3, n]
    assert abs(got["polarity_sum"][0, 0]) > 2.0 ** 2 and float(got["polarity_sum"][3, 0]) == float(np.sum(sig.q30)) * 2.0 ** -30


# ---------------------------------------------------------------- clause 2 on both axes, filters, signals
def test_time_axis_edges():
    n = 5000
    fwd, sig = _random_fwd(n), _signals(n)
    rng = np.random.default_rng(9)
    origin, width, nb = 1000, 100, 7
    stamp = rng.integers(origin - 300, origin + (nb + 3) * width, size=n).astype(np.uint32)
    stamp[:6] = [origin - 1, origin, origin + nb * width - 1, origin + nb * width, 0, 0xFFFFFFFF]
    group = np.zeros(n, np.uint32)
    idx = _index(_ctx(), fwd, sig, group, stamp)
    queries = [[3], [17, 64], [255, 256, 1000]]
    queries += [[int(fwd.terms[int(fwd.offs[d])])] for d in range(6)]      # terms of the six planted stamps' documents
    qt, qo = _pack(queries)
    _same(idx.mention_summary(qt, qo, n_buckets=nb, stamp_origin=origin, bucket_width=width),
          _ref(fwd, queries, sig, n_cells=nb, origin=origin, width=width, stamp=stamp))
    _same(idx.mention_summary(qt, qo, n_buckets=1, stamp_origin=123456, bucket_width=0), _ref(fwd, queries, sig))   # no time axis
    # origin + n * width > 2^32
    hi_origin, hi_width = 0xFFFFFF00, 64
    stamp2 = (hi_origin - 64 + rng.integers(0, 320, size=n)).astype(np.uint32)
    idx.set_doc_attrs(group, stamp2)
    _same(idx.mention_summary(qt, qo, n_buckets=8, stamp_origin=hi_origin, bucket_width=hi_width),
          _ref(fwd, queries, sig, n_cells=8, origin=hi_origin, width=hi_width, stamp=stamp2))


@pytest.mark.parametrize("mask", [0xFF, 0xFF00, 0xFFFF0000])
def test_key_axis_masks_and_the_last_key(mask):
    n = 5000
    fwd, sig = _random_fwd(n), _signals(n)
    shift = (mask & -mask).bit_length() - 1
    rng = np.random.default_rng(mask & 0xFFFF)
    n_keys = 50
    key = rng.integers(0, n_keys + 10, size=n)                 # keys n_keys .. n_keys + 9 belong to no cell
    key[:2] = [n_keys - 1, n_keys]
    noise = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64) & np.uint64(~mask & 0xFFFFFFFF)
    group = ((key.astype(np.uint64) << np.uint64(shift)) | noise).astype(np.uint32)
    stamp = np.zeros(n, np.uint32)
    idx = _index(_ctx(), fwd, sig, group, stamp)
    queries = [[3], [17, 64], [int(fwd.terms[int(fwd.offs[0])])], [int(fwd.terms[int(fwd.offs[1])])]]
    mm = np.array([1, 0, 1, 1], np.uint32)
    got = idx.mention_groups(*_pack(queries), mask, n_keys, min_match=mm)
    want = _ref(fwd, queries, sig, mm, n_cells=n_keys, key_mask=mask, group=group)
    _same(got, want)
    assert want["total"][2, n_keys - 1] >= 1 and want["total"].sum() < _ref(fwd, queries, sig, mm)["total"].sum()


def test_per_query_filters():
    n = 20000
    fwd, sig = _random_fwd(n), _signals(n)
    group, stamp = _attrs(n)
    idx = _index(_ctx(), fwd, sig, group, stamp)
    queries = [[3, 17], [3, 17], [3, 17], [64], [255, 256]]
    filters = np.array([ALL_DOCS, NO_DOCS, (0xF, 0x3, 0, 0xFFFFFFFF), (0, 0, 2000, 3000), (0x1, 0x1, 1500, 5500)], np.uint32)
    mm = np.array([1, 1, 0, 1, 2], np.uint32)
    qt, qo = _pack(queries)
    got = idx.mention_summary(qt, qo, min_match=mm, n_buckets=5, stamp_origin=1000, bucket_width=1000, filters=filters)
    _same(got, _ref(fwd, queries, sig, mm, n_cells=5, origin=1000, width=1000, group=group, stamp=stamp, filters=filters))
    assert got["total"][1].sum() == 0 and got["total"][0].sum() > got["total"][2].sum() > 0
    _same(idx.mention_groups(qt, qo, 0x1FF, 300, min_match=mm, filters=filters),
          _ref(fwd, queries, sig, mm, n_cells=300, key_mask=0x1FF, group=group, stamp=stamp, filters=filters))
    _same(idx.mention_summary(qt, qo, min_match=mm, filters=filters),          # a filter without a time axis
          _ref(fwd, queries, sig, mm, group=group, stamp=stamp, filters=filters))


def test_every_flag_combination_and_the_polarity_extremes():
    n = 4 * VALS.size
    sig = _signals(n)
    combos = {(bool(sig.bull[i]), bool(sig.bear[i]), bool(sig.sp[i]), bool(sig.s1[i])) for i in range(n)}
    assert len(combos) == 12 and 0 in sig.q30 and 2 ** 30 in sig.q30 and -2 ** 30 in sig.q30
    fwd = _fwd_from_docs([[50, 1 + i] for i in range(n)])
    idx = _index(_ctx(), fwd, sig, np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32))
    queries = [[50]] + [[1 + i] for i in range(n)]
    _same(idx.mention_summary(*_pack(queries)), _ref(fwd, queries, sig))
    got = idx.mention_groups(*_pack([[50]]), 0xFF, n)            # one document per key: every record on its own
    _same(got, _ref(fwd, [[50]], sig, n_cells=n, key_mask=0xFF, group=np.arange(n, dtype=np.uint32)))


# ---------------------------------------------------------------- cross-check against the BM25 list
def test_any_matches_the_documents_with_a_bm25_score():
    n, dim = 6000, 16
    rng = np.random.default_rng(4)
    lens = rng.integers(1, 7, size=n)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    fwd = _Fwd(rng.integers(0, 400, size=int(offs[-1])).astype(np.uint32), offs)      # ~50 documents per term
    sig = _signals(n)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    idx = _index(_ctx(), fwd, sig, np.arange(n, dtype=np.uint32), np.zeros(n, np.uint32), dim=dim, rows=rows)
    queries = [[5, 9, 300], [17], [17, 17, 200, 399], [1, 2, 3, 4, 5, 6, 7, 8]]
    qt, qo = _pack(queries)
    lists = idx.search_lists(rows[:len(queries)].copy(), qt, qo, depth=1024)
    got = idx.mention_groups(qt, qo, 0xFFFF, n)
    for q in range(len(queries)):
        c = int(lists.bm25_counts[q])
        assert 0 < c < 1024
        assert np.all(got["total"][q] <= 1)
        assert sorted(np.nonzero(got["total"][q])[0].tolist()) == sorted(int(d) for d in lists.bm25_docs[q, :c])


# ---------------------------------------------------------------- routes and state
def test_host_and_device_locations_a_view_and_repeat_calls():
    import torch
    import openintel_amd as oi
    n, dim = 40000, 16
    fwd, sig = _random_fwd(n), _signals(n)
    group, stamp = _attrs(n)
    rows = np.random.default_rng(1).standard_normal((n, dim)).astype(np.float32)
    ctx = _ctx()
    idx = _index(ctx, fwd, sig, group, stamp, dim=dim, rows=rows)
    queries = [[3], [3, 17], [], [64, 255, 256], [EDGE0, EDGE0 + 1, 4095]]
    mm = np.array([1, 0, 1, 2, 1], np.uint32)
    filters = np.array([ALL_DOCS, (0x3, 0x1, 0, 0xFFFFFFFF), ALL_DOCS, (0, 0, 1000, 4000), ALL_DOCS], np.uint32)
    qt, qo = _pack(queries)
    kw = dict(n_buckets=6, stamp_origin=1000, bucket_width=1000)
    want = _ref(fwd, queries, sig, mm, n_cells=6, origin=1000, width=1000, group=group, stamp=stamp, filters=filters)
    host = idx.mention_summary(qt, qo, min_match=mm, filters=filters, **kw)
    _same(host, want)
    assert idx.mention_summary(qt, qo, min_match=mm, filters=filters, **kw).tobytes() == host.tobytes()      # the same call twice
    dev = "cuda:0"
    d_qt, d_qo = torch.from_numpy(qt.view(np.int32)).to(dev), torch.from_numpy(qo.view(np.int32)).to(dev)
    d_mm = torch.from_numpy(mm.view(np.int32)).to(dev)
    d_f = torch.from_numpy(filters.view(np.int32)).to(dev)
    _same(_host(idx.mention_summary(d_qt, d_qo, min_match=d_mm, filters=d_f, **kw)), want)
    _same(_host(idx.mention_groups(d_qt, d_qo, 0xFF, 256, min_match=d_mm, filters=d_f)),
          _ref(fwd, queries, sig, mm, n_cells=256, key_mask=0xFF, group=group, stamp=stamp, filters=filters))
    # a view on a second context sees postings, signals and attributes
    ctx2 = oi.HipContext.like(ctx)
    view = idx.view(ctx2)
    _same(view.mention_summary(qt, qo, min_match=mm, filters=filters, **kw), want)
    # signals overwritten in place between two calls (the view sees the update too)
    sig2 = _signals(n, seed=5)
    idx.set_signals(sig2.pol, sig2.spec, sig2.src, TAU)
    want2 = _ref(fwd, queries, sig2, mm, n_cells=6, origin=1000, width=1000, group=group, stamp=stamp, filters=filters)
    assert want2.tobytes() != want.tobytes()
    _same(idx.mention_summary(qt, qo, min_match=mm, filters=filters, **kw), want2)
    _same(view.mention_summary(qt, qo, min_match=mm, filters=filters, **kw), want2)
    # text in, through the index's own tokeniser: the same call as with its terms
    texts = ["gme squeeze", "moon"]
    t_qt, t_qo = idx.query_terms(texts)
    assert idx.mention_summary_text(texts, min_match="all", **kw).tobytes() == idx.mention_summary(t_qt, t_qo, min_match="all", **kw).tobytes()
    assert idx.mention_groups_text(texts, 0xFF, 9).tobytes() == idx.mention_groups(t_qt, t_qo, 0xFF, 9).tobytes()
    view.close()


def test_state_errors():
    from openintel_amd import _lib
    n = 100
    fwd, sig = _random_fwd(n), _signals(n)
    qt, qo = _pack([[3]])

    def state_error(idx, word, **kw):
        with pytest.raises(_lib.OiError) as e:
            if "key_mask" in kw:
                idx.mention_groups(qt, qo, kw["key_mask"], 4)
            else:
                idx.mention_summary(qt, qo, **kw)
        assert e.value.code == _lib.OI_ERR_STATE and word in e.value.message, e.value.message

    state_error(_index(_ctx(), fwd, sig, finalize=False), "not finalized")
    state_error(_index(_ctx(), fwd, None), "no signals")
    idx = _index(_ctx(), fwd, sig)                                   # no attributes
    assert idx.mention_summary(qt, qo)["total"][0, 0] == fwd.has(3).sum()
    state_error(idx, "doc attributes", n_buckets=2, bucket_width=10)
    state_error(idx, "doc attributes", filters=np.array([ALL_DOCS], np.uint32))
    state_error(idx, "doc attributes", key_mask=0xFF)
    assert idx.mention_summary(np.zeros(0, np.uint32), np.zeros(1, np.uint32)).shape == (0, 1)       # n_queries == 0


def test_workspace_grows_by_64_bytes_per_cell_and_272_per_query():
    import torch
    n = 3000
    fwd, sig = _random_fwd(n), _signals(n)
    _, stamp = _attrs(n)
    ctx = _ctx()
    idx = _index(ctx, fwd, sig, np.zeros(n, np.uint32), stamp)
    B, nb = 64, 24
    qt, qo = _pack([[3, 17]] * B)
    dev = "cuda:0"
    d_qt, d_qo = torch.from_numpy(qt.view(np.int32)).to(dev), torch.from_numpy(qo.view(np.int32)).to(dev)
    before = ctx.workspace_bytes()[0]
    idx.mention_summary(d_qt, d_qo, n_buckets=nb, stamp_origin=1000, bucket_width=250)
    ctx.synchronize()
    assert ctx.workspace_bytes()[0] - before == 64 * B * nb + 272 * B        # (both are multiples of the 256-byte granule)
    idx.mention_summary(d_qt, d_qo, n_buckets=nb, stamp_origin=1000, bucket_width=250)
    assert ctx.workspace_bytes()[0] - before == 64 * B * nb + 272 * B        # and stays
