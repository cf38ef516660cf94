"""Near-duplicate collapse of ranked lists (oi_collapse_lists / oi_search_collapsed).

Small-integer embeddings in [-2, 2] (normalize=False) and thresholds on a half-integer: every dot product is exact in any
order, so docs, counts, dup_counts and score bits are compared BIT FOR BIT with a numpy restatement of the definition
(f64 similarities, a ten-line greedy loop) -- never with anything the library computed.  oi_search / oi_search_filtered,
unchanged and tested elsewhere, produce the input lists of the oi_search_collapsed cases."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
VOCAB = 64
LENS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024)   # every tile (128), mask-word (64) and MFMA-tile (32) edge


# ------------------------------------------------------------------ the definition, in numpy
def np_collapse(rows64, base, scores, docs, count, t, k):
    """-> (kept docs, their scores or None, dup_counts): the header's rule on one list.  rows64: the stored rows as f64."""
    n = rows64.shape[0]
    docs = np.asarray(docs[:count], dtype=np.int64)
    valid = (docs >= base) & (docs < base + n)            # out of the shard: a singleton, no row read
    X = rows64[np.where(valid, docs - base, 0)]
    with np.errstate(invalid="ignore", over="ignore"):
        hit = (X @ X.T >= t) & valid[:, None] & valid[None, :]   # NaN >= t is False
    kept = np.zeros(count, dtype=bool)
    dup = np.zeros(count, dtype=np.int64)
    for i in range(count):
        c = hit[i, :i] & kept[:i]
        if c.any():
            dup[np.argmax(c)] += 1                        # the best-ranked kept entry with sim >= t
        else:
            kept[i], dup[i] = True, 1
    ki = np.nonzero(kept)[0][:k]
    return docs[ki].astype(np.uint32), None if scores is None else np.asarray(scores)[ki], dup[ki].astype(np.uint32)


def check_batch(out, rows64, base, scores, docs, counts, t, k, tag=""):
    for q in range(docs.shape[0]):
        d, s, u = np_collapse(rows64, base, None if scores is None else scores[q], docs[q], int(counts[q]), t, k)
        c = int(out.counts[q])
        assert c == d.size, (tag, q, c, d.size)
        assert np.array_equal(np.asarray(out.docs[q][:c]).view(np.uint32), d), (tag, q)
        assert np.array_equal(np.asarray(out.dup_counts[q][:c]).view(np.uint32), u), (tag, q)
        if scores is not None:
            assert np.array_equal(np.asarray(out.scores[q][:c]).view(np.uint32), s.astype(np.float32).view(np.uint32)), (tag, q)


def _ctx():
    import openintel_amd as oi
    return oi.HipContext(0)


def _emb_index(ctx, rows, base=0, bf16=False):
    """embeddings only: no forward index, no finalize"""
    import openintel_amd as oi
    idx = oi.HybridIndex(ctx, rows.shape[0], rows.shape[1], VOCAB, base)
    if bf16:
        idx.set_embeddings_bf16((np.ascontiguousarray(rows, np.float32).view(np.uint32) >> 16).astype(np.uint16))
    else:
        idx.set_embeddings(rows, normalize=False)
    return idx


# ------------------------------------------------------------------ one small corpus shared by the hand-built lists
N36, D36, T36 = 4500, 36, 60.5
COPY36 = (2000, 2500)   # rows 2500 .. 4499 are exact copies of rows 0 .. 1999


@pytest.fixture(scope="module")
def C36():
    """4500 x 36 small integers, the last 2000 rows copies of the first 2000; `distinct`: 1024 rows below 2000 whose pairwise
    similarities are all < T36 and whose self-similarity is >= T36."""
    rng = np.random.default_rng(7)
    rows = rng.integers(-2, 3, size=(N36, D36)).astype(np.float32)
    rows[2500:] = rows[:2000]
    r64 = rows.astype(np.float64)
    G = r64[:2000] @ r64[:2000].T
    distinct = []
    for i in range(2000):
        if G[i, i] >= T36 and (not distinct or G[i, distinct].max() < T36):
            distinct.append(i)
            if len(distinct) == 1024:
                break
    assert len(distinct) == 1024
    ctx = _ctx()
    idx = _emb_index(ctx, rows)
    yield {"rows": rows, "r64": r64, "distinct": np.array(distinct, dtype=np.uint32), "idx": idx, "ctx": ctx}
    idx.close()
    ctx.close()


def _ragged(B, depth, start, rng, n=N36, base=0, copy_of=COPY36):
    """lengths LENS[start], LENS[start + 1], ... (cut at depth); docs drawn with replacement (the same id twice happens), a
    quarter of them from the copied rows so that exact duplicates of other docs are common"""
    counts = np.array([min(LENS[(start + q) % len(LENS)], depth) for q in range(B)], dtype=np.uint32)
    docs = rng.integers(0, n, size=(B, depth)).astype(np.uint32)
    copy = rng.random((B, depth)) < 0.25
    docs = np.where(copy & (docs < copy_of[0]), docs + copy_of[1], docs).astype(np.uint32) + np.uint32(base)
    scores = -np.sort(-rng.standard_normal((B, depth)).astype(np.float32), axis=1)
    return scores, docs, counts


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("depth", [1, 33, 1024])
def test_every_list_length_in_ragged_batches(C36, B, depth):
    """lengths 0 .. 1024 across every edge, in one ragged batch (B = 65) or in windows of B lists; k = 1, depth and between;
    T = 30.5 makes a few in a thousand random pairs duplicates on top of the exact copies"""
    rng = np.random.default_rng(100 * B + depth)
    idx = C36["idx"]
    for start in range(0, len(LENS) if B < len(LENS) else 1, B):
        scores, docs, counts = _ragged(B, depth, start, rng)
        for k in sorted({1, depth, (depth + 1) // 2}):
            out = idx.collapse_lists(scores, docs, counts, 30.5, k)
            check_batch(out, C36["r64"], 0, scores, docs, counts, 30.5, k, (start, k))


def test_duplicate_pairs_across_tile_and_mask_word_edges(C36):
    """one duplicate pair (i, j) in an otherwise duplicate-free list of 1024: as the same doc id twice and as a copied row"""
    idx, dist = C36["idx"], C36["distinct"]
    pairs = [(1, 0), (32, 31), (33, 0), (64, 63), (64, 0), (1023, 0), (1023, 1022)]
    lists = []
    for (i, j) in pairs:
        for same_id in (True, False):
            d = dist.copy()
            d[i] = d[j] if same_id else d[j] + COPY36[1]
            lists.append(d)
    lists.append(np.where(np.arange(1024) % 2 == 0, dist[0], dist[0] + COPY36[1]).astype(np.uint32))   # all duplicates of entry 0
    lists.append(dist.copy())                                                                          # no duplicates
    docs = np.stack(lists).astype(np.uint32)
    B = docs.shape[0]
    counts = np.full(B, 1024, dtype=np.uint32)
    scores = np.tile(-np.arange(1024, dtype=np.float32), (B, 1))
    for k in (1024, 40):
        out = idx.collapse_lists(scores, docs, counts, T36, k)
        check_batch(out, C36["r64"], 0, scores, docs, counts, T36, k, k)
    out = idx.collapse_lists(scores, docs, counts, T36, 1024)
    # the reference agrees with what the construction says: one collapsed entry per pair list, ...
    for b in range(2 * len(pairs)):
        i, j = pairs[b // 2]
        assert int(out.counts[b]) == 1023 and int(out.dup_counts[b][j]) == 2, (b, i, j)
        assert np.array_equal(out.docs[b][:1023], np.delete(docs[b], i)), b
    assert int(out.counts[B - 2]) == 1 and int(out.dup_counts[B - 2][0]) == 1024          # ... one kept, dup_counts = c ...
    assert int(out.counts[B - 1]) == 1024 and np.array_equal(out.docs[B - 1], docs[B - 1])  # ... and the input unchanged
    assert np.array_equal(out.scores[B - 1].view(np.uint32), scores[B - 1].view(np.uint32)) and (out.dup_counts[B - 1] == 1).all()
    # without scores: scores_out is not written; dup_counts_out may be NULL too
    from openintel_amd import _lib
    o2 = idx.collapse_lists(None, docs, counts, T36, 1024)
    assert o2.scores is None and np.array_equal(o2.docs, out.docs) and np.array_equal(o2.dup_counts, out.dup_counts)
    do, co = np.zeros((B, 1024), np.uint32), np.zeros(B, np.uint32)
    _lib.check(idx.lib.oi_collapse_lists(idx.handle, None, _lib.ptr(docs), _lib.ptr(counts), B, 1024, T36, 1024, _lib.OI_HOST,
                                         None, _lib.ptr(do), _lib.ptr(co), None))
    assert np.array_equal(do, out.docs) and np.array_equal(co, out.counts)


def test_greedy_not_transitive_and_dup_counts_beyond_the_cut():
    ctx = _ctx()
    d = 8
    rows = np.zeros((6, d), np.float32)
    rows[0, 0] = 4                      # A
    rows[1, 0] = rows[1, 1] = 3         # B: A.B = B.C = 12, A.C = 0
    rows[2, 1] = 4                      # C
    rows[4, 2] = 3                      # D, row 5 = its copy; row 3 stays zero (similar to nothing, itself included)
    rows[5, 2] = 3
    A, Bv, Cv, Z, D, D2 = range(6)
    idx = _emb_index(ctx, rows)
    r64 = rows.astype(np.float64)
    depth = 192
    lists = [[A, Bv, Cv], [A, Cv, Bv], [Cv, A, Bv],
             [A] + [Z] * 69 + [Cv] + [Z] * 58 + [Bv],            # A, C and B in three mask words / two tiles
             [D, A, Cv, Z, Z] + [D2, D] * 20 + [Bv]]             # duplicates of D ranked after the k-th kept entry
    docs = np.zeros((len(lists), depth), np.uint32)
    counts = np.array([len(x) for x in lists], np.uint32)
    for q, x in enumerate(lists):
        docs[q, :len(x)] = x
    scores = np.tile(np.linspace(1, 0, depth, dtype=np.float32), (len(lists), 1))
    out = idx.collapse_lists(scores, docs, counts, 8.5, depth)
    check_batch(out, r64, 0, scores, docs, counts, 8.5, depth)
    assert out.docs[0][:2].tolist() == [A, Cv] and out.dup_counts[0][:2].tolist() == [2, 1] and out.counts[0] == 2
    assert out.docs[1][:2].tolist() == [A, Cv] and out.dup_counts[1][:2].tolist() == [2, 1]   # B goes to the better-ranked A
    assert out.docs[2][:2].tolist() == [Cv, A] and out.dup_counts[2][:2].tolist() == [2, 1]
    assert out.counts[3] == 129 and out.dup_counts[3][0] == 2 and out.dup_counts[3][70] == 1
    cut = idx.collapse_lists(scores, docs, counts, 8.5, 2)
    check_batch(cut, r64, 0, scores, docs, counts, 8.5, 2)
    assert cut.counts[4] == 2 and cut.docs[4].tolist() == [D, A] and cut.dup_counts[4].tolist() == [41, 2]
    idx.close()
    ctx.close()


def _k_edge_corpus(dim, rng):
    """pairs that reach t = 3.5 only through coordinate dim - 1 or only through coordinate 0, and pairs that would reach it if
    that product were counted twice; the middle coordinates of the two sides are disjoint (their product is 0)"""
    rows = np.zeros((12, dim), np.float32)
    mid = np.arange(1, dim - 1)
    for r in range(12):
        sel = mid[mid % 2 == r % 2]
        rows[r, sel] = rng.integers(-2, 3, size=sel.size)
    for c, r0 in ((dim - 1, 0), (0, 6)):
        rows[r0 + 0, c], rows[r0 + 1, c] = 2, 2      # 4 >= 3.5 only with the product at c (dropped: 0)
        rows[r0 + 2, c], rows[r0 + 3, c] = 2, 1      # 2 < 3.5 (doubled: 4)
        rows[r0 + 4, c], rows[r0 + 5, c] = -2, -2    # 4
    return rows


@pytest.mark.parametrize("dim,bf16", [(4, False), (20, False), (36, False), (384, False), (768, False), (1024, False),
                                      (384, True), (1024, True)])
def test_k_tail_and_first_coordinate_decide(dim, bf16):
    rng = np.random.default_rng(dim)
    edge = _k_edge_corpus(dim, rng)
    fill = rng.integers(-2, 3, size=(500, dim)).astype(np.float32)
    rows = np.concatenate([edge, fill, fill[:100]])      # random rows and copies of some, for lists with real sums
    ctx = _ctx()
    idx = _emb_index(ctx, rows, bf16=bf16)
    r64 = rows.astype(np.float64)
    depth = 200
    lists = [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11], [1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10]]
    docs = np.zeros((len(lists) + 2, depth), np.uint32)
    counts = np.array([len(x) for x in lists] + [depth, depth], np.uint32)
    for q, x in enumerate(lists):
        docs[q, :len(x)] = x
    out = idx.collapse_lists(None, docs[:len(lists)], counts[:len(lists)], 3.5, depth)
    check_batch(out, r64, 0, None, docs[:len(lists)], counts[:len(lists)], 3.5, depth, dim)
    assert [int(c) for c in out.counts[:6]] == [1, 2, 1, 1, 2, 1]
    # random lists: t at half the mean self-similarity (2 dim), on a half-integer
    docs[len(lists):] = rng.integers(12, rows.shape[0], size=(2, depth))
    t = float(dim) + 0.5
    out = idx.collapse_lists(None, docs, counts, t, 64)
    check_batch(out, r64, 0, None, docs, counts, t, 64, dim)
    idx.close()
    ctx.close()


@pytest.mark.parametrize("bf16", [False, True])
def test_row_and_id_edges_and_thresholds(bf16):
    """local rows 0 and n - 1, doc_id_base = 1000, ids outside the shard (singletons: kept, nothing collapses into them, no
    row read, OI_OK), the same id twice, +inf and -inf thresholds"""
    rng = np.random.default_rng(3 + bf16)
    n, dim, base = 3000, 384, 1000
    rows = rng.integers(-2, 3, size=(n, dim)).astype(np.float32)
    rows[2000:] = rows[:1000]     # (row n - 1 is a copy of row 999, row 2000 of row 0)
    ctx = _ctx()
    idx = _emb_index(ctx, rows, base=base, bf16=bf16)
    r64 = rows.astype(np.float64)
    depth, t = 130, 400.5
    hand = [[base, base + n - 1, base + n, base + n, 999, 999, 0, 0xFFFFFFFF, base + 999, base + 2000, base + 5, base + 5],
            [0xFFFFFFFF, base + n - 1, base, 0, base + n - 1],
            [999, base + n, 5, 7]]
    scores, docs, counts = _ragged(6, depth, 7, rng, n=n, base=base, copy_of=(1000, 2000))
    counts[3] = counts[4] = depth
    for q, x in enumerate(hand):
        docs[q, :len(x)] = x
        counts[q] = len(x)
    docs[3, ::7] = rng.integers(0, base, size=docs[3, ::7].size)            # out-of-shard ids sprinkled into long lists
    docs[4, ::5] = rng.integers(base + n, 1 << 32, size=docs[4, ::5].size)
    for k in (depth, 3):
        out = idx.collapse_lists(scores, docs, counts, t, k)
        check_batch(out, r64, base, scores, docs, counts, t, k, k)
    out = idx.collapse_lists(scores, docs, counts, t, depth)
    assert out.docs[0][:int(out.counts[0])].tolist() == [base, base + n - 1, base + n, base + n, 999, 999, 0, 0xFFFFFFFF, base + 5]
    assert out.dup_counts[0][:int(out.counts[0])].tolist() == [2, 2, 1, 1, 1, 1, 1, 1, 2]
    assert int(out.counts[2]) == 4
    # +inf: the input cut at k; -inf: one entry per non-empty list when every id is in the shard
    scores, docs, counts = _ragged(11, depth, 0, rng, n=n, base=base, copy_of=(1000, 2000))
    out = idx.collapse_lists(scores, docs, counts, float("inf"), 50)
    check_batch(out, r64, base, scores, docs, counts, float("inf"), 50, "+inf")
    for q in range(11):
        c = min(int(counts[q]), 50)
        assert int(out.counts[q]) == c and np.array_equal(out.docs[q][:c], docs[q][:c]) and (out.dup_counts[q][:c] == 1).all()
    out = idx.collapse_lists(scores, docs, counts, float("-inf"), 50)
    check_batch(out, r64, base, scores, docs, counts, float("-inf"), 50, "-inf")
    for q in range(11):
        assert int(out.counts[q]) == min(int(counts[q]), 1)
        if counts[q]:
            assert out.docs[q][0] == docs[q][0] and out.dup_counts[q][0] == counts[q]
    idx.close()
    ctx.close()


def test_nan_row_is_never_a_duplicate_not_even_of_itself():
    rng = np.random.default_rng(11)
    n, dim = 300, 36
    rows = rng.integers(-2, 3, size=(n, dim)).astype(np.float32)
    rows[5, 3] = np.nan
    rows[200] = rows[7]
    ctx = _ctx()
    idx = _emb_index(ctx, rows)
    r64 = rows.astype(np.float64)
    depth = 70
    docs = rng.integers(0, n, size=(3, depth)).astype(np.uint32)
    docs[0, :6] = [5, 5, 7, 5, 200, 7]
    docs[1, ::3] = 5
    counts = np.array([6, depth, depth], np.uint32)
    for t in (float("-inf"), 20.5):
        out = idx.collapse_lists(None, docs, counts, t, depth)
        check_batch(out, r64, 0, None, docs, counts, t, depth, t)
    out = idx.collapse_lists(None, docs, counts, float("-inf"), depth)
    assert out.docs[0][:4].tolist() == [5, 5, 7, 5] and out.dup_counts[0][:4].tolist() == [1, 1, 3, 1] and out.counts[0] == 4
    idx.close()
    ctx.close()


def test_device_lists_a_view_and_an_index_without_embeddings(C36):
    """OI_DEVICE in and out (asynchronous on the ctx stream), the same through an oi_index_view on a second context, and
    OI_ERR_STATE for an index that has no embeddings"""
    import torch
    import openintel_amd as oi
    from openintel_amd import _lib
    rng = np.random.default_rng(5)
    scores, docs, counts = _ragged(11, 1024, 0, rng)
    t32 = lambda x: torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to("cuda:0")
    sd, dd, cd = t32(scores), t32(docs), t32(counts)
    ctx2 = _ctx()
    # (a view needs a finalized source: a finalized twin of the shared corpus)
    src = _emb_index(C36["ctx"], C36["rows"])
    lens = np.ones(N36, dtype=np.uint64)
    src.set_forward(np.zeros(N36, np.uint32), np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64))
    src.finalize()
    view = src.view(ctx2)
    for idx, ctx in ((C36["idx"], C36["ctx"]), (view, ctx2)):
        out = idx.collapse_lists(sd, dd, cd, 30.5, 100)
        ctx.synchronize()
        host = oi.retriever.CollapsedResult(*(x.cpu().numpy() for x in (out.scores, out.docs, out.counts, out.dup_counts)))
        check_batch(host, C36["r64"], 0, scores, docs, counts, 30.5, 100)
    bare = oi.HybridIndex(ctx2, 10, 8, VOCAB)
    with pytest.raises(_lib.OiError) as e:
        bare.collapse_lists(None, docs[:, :4], counts, 1.5, 4)
    assert e.value.code == _lib.OI_ERR_STATE
    for x in (bare, view, src):
        x.close()
    ctx2.close()


# ------------------------------------------------------------------ oi_search_collapsed == collapse(oi_search(k = pool))
def _planted(n, dim, seed):
    """~20 000 small-integer rows; 150 source rows each with a block of 3 .. 30 exact copies scattered over the corpus and a
    few half-zeroed copies whose similarity to the source lies around the threshold (dim + 0.5) on either side"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(-2, 3, size=(n, dim)).astype(np.float32)
    free = rng.permutation(np.arange(1000, n))
    src = np.arange(0, 150)
    at = 0
    for s in src:
        m = int(rng.integers(3, 31))
        rows[free[at:at + m]] = rows[s]
        at += m
        for _ in range(3):
            half = rows[s].copy()
            half[rng.random(dim) < 0.5] = 0
            rows[free[at]] = half
            at += 1
    lens = rng.integers(1, 9, size=n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    terms = rng.integers(0, VOCAB, size=int(offs[-1])).astype(np.uint32)
    group = rng.integers(0, 1 << 16, size=n).astype(np.uint32)
    stamp = (rng.permutation(n) % 2000).astype(np.uint32)
    return rows, terms, offs, group, stamp


@pytest.fixture(scope="module", params=[384, 768])
def planted(request):
    import openintel_amd as oi
    dim, n = request.param, 20000
    rows, terms, offs, group, stamp = _planted(n, dim, seed=dim)
    ctx = _ctx()
    idx = oi.HybridIndex(ctx, n, dim, VOCAB, 0)
    idx.set_embeddings(rows, normalize=False)
    idx.set_forward(terms, offs)
    idx.set_doc_attrs(group, stamp)
    idx.finalize()
    yield {"dim": dim, "n": n, "rows": rows, "r64": rows.astype(np.float64), "group": group, "idx": idx, "ctx": ctx}
    idx.close()
    ctx.close()


def _planted_queries(P, B, seed):
    """query b = a source row (its copies tie at the top of the cosine list) and three random terms"""
    rng = np.random.default_rng(seed)
    q = P["rows"][rng.integers(0, 150, size=B)].copy()
    qt = rng.integers(0, VOCAB, size=3 * B).astype(np.uint32)
    qo = (3 * np.arange(B + 1)).astype(np.uint32)
    return q, qt, qo


def _filter_mix(B, group):
    out = []
    for b in range(B):
        out.append([(0, 0, 0, 0xFFFFFFFF), (1, b & 1, 0, 0xFFFFFFFF), (0, 0, 300, 1500), (0xF, int(group[b]) & 0xF, 0, 0xFFFFFFFF),
                    (0, 0, 7, 6)][b % 5])
    return np.array(out, dtype=np.uint32)


def _check_against_search(P, got, want_pool, t, k, tag):
    """got == numpy-collapse(the trusted pool-list), scores the RRF scores of the kept docs bit for bit"""
    check_batch(got, P["r64"], 0, want_pool.scores, want_pool.docs, want_pool.counts, t, k, tag)


@pytest.mark.parametrize("B", [1, 9, 64])
def test_search_collapsed_is_search_then_collapse(planted, B):
    import torch
    import openintel_amd as oi
    P, idx, ctx = planted, planted["idx"], planted["ctx"]
    depth, pool, k, t = 256, 256, 50, float(P["dim"]) + 0.5
    q, qt, qo = _planted_queries(P, B, seed=B)
    before = idx.search(q, qt, qo, k=k, depth=depth)
    pool_list = idx.search(q, qt, qo, k=pool, depth=depth)
    got = idx.search_collapsed(q, qt, qo, k=k, depth=depth, pool=pool, threshold=t)
    _check_against_search(P, got, pool_list, t, k, "host")
    assert any(int(got.dup_counts[b][:int(got.counts[b])].max()) > 1 for b in range(B)), "the planted copies collapse"
    # a filter mix, against oi_search_filtered
    F = _filter_mix(B, P["group"])
    pool_f = idx.search(q, qt, qo, k=pool, depth=depth, filters=F)
    got_f = idx.search_collapsed(q, qt, qo, k=k, depth=depth, pool=pool, threshold=t, filters=F)
    _check_against_search(P, got_f, pool_f, t, k, "filtered")
    # OI_DEVICE
    t32 = lambda x: torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to("cuda:0")
    qd, qtd, qod = t32(q), t32(qt), t32(qo)
    dev = idx.search_collapsed(qd, qtd, qod, k=k, depth=depth, pool=pool, threshold=t)
    ctx.synchronize()
    to_host = lambda r: oi.retriever.CollapsedResult(*(x.cpu().numpy() for x in (r.scores, r.docs, r.counts, r.dup_counts)))
    _check_against_search(P, to_host(dev), pool_list, t, k, "device")
    # unchanged behaviour: oi_search returns what it did before, byte for byte
    after = idx.search(q, qt, qo, k=k, depth=depth)
    for f in ("scores", "docs", "counts"):
        assert getattr(before, f).tobytes() == getattr(after, f).tobytes(), f


def test_search_collapsed_full_pool_view_and_graph_replay(planted):
    """pool = depth = 1000 (every tile of the triangle), through a view on a second context with its own stream, graph
    replay off and on: replayed results equal unreplayed ones"""
    import torch
    import openintel_amd as oi
    P, idx = planted, planted["idx"]
    B, depth, pool, k, t = 9, 1000, 1000, 100, float(P["dim"]) + 0.5
    q, qt, qo = _planted_queries(P, B, seed=77)
    pool_list = idx.search(q, qt, qo, k=pool, depth=depth)
    ctx2 = _ctx()
    stream = torch.cuda.Stream(device="cuda:0")
    ctx2.set_stream(stream)      # (replay needs a real stream, not the default one)
    view = idx.view(ctx2)
    got = view.search_collapsed(q, qt, qo, k=k, depth=depth, pool=pool, threshold=t)
    _check_against_search(P, got, pool_list, t, k, "view host")
    t32 = lambda x: torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to("cuda:0")
    qd, qtd, qod = t32(q), t32(qt), t32(qo)
    F = _filter_mix(B, P["group"])
    Fd = t32(F)
    pool_f = idx.search(q, qt, qo, k=pool, depth=depth, filters=F)
    to_host = lambda r: oi.retriever.CollapsedResult(*(x.cpu().numpy() for x in (r.scores, r.docs, r.counts, r.dup_counts)))
    torch.cuda.synchronize()
    results = {}
    for replay in (False, True):
        ctx2.set_graph_replay(replay)
        for filt, want in ((None, pool_list), (Fd, pool_f)):
            out = None
            for _ in range(3):       # with replay on: eager, capture, replay
                out = view.search_collapsed(qd, qtd, qod, k=k, depth=depth, pool=pool, threshold=t, filters=filt, out=out)
            ctx2.synchronize()
            h = to_host(out)
            _check_against_search(P, h, want, t, k, ("replay", replay, filt is not None))
            results[(replay, filt is not None)] = h
    assert ctx2.graph_stats()[0] >= 2, "the third call of each kind was a replay"
    for filt in (False, True):
        a, b = results[(False, filt)], results[(True, filt)]
        assert np.array_equal(a.counts, b.counts)
        for x in range(B):
            c = int(a.counts[x])
            for f in ("scores", "docs", "dup_counts"):
                assert getattr(a, f)[x][:c].tobytes() == getattr(b, f)[x][:c].tobytes(), (filt, x, f)
    view.close()
    ctx2.close()
