"""Filtered hybrid search (oi_doc_filter): a filtered list is the unfiltered full ranking restricted to the
passing documents and cut at depth.  Small-integer embeddings make every dot product exact, so each cosine route (the int8
tier, the copy screen, the f32-stream screen's route, exact and split at B = 1, 9, 64, the generic dim, a bf16 corpus) and
every BM25 mode must give exactly that, bit for bit, RRF included.  Larger corpora check the screen's chunk edges and both
phases of the BM25 stream schedule against the CPU oracle.  The chunk, query-group, long-row and gate edges of the filtered
int8, copy-screen and bf16-corpus kernels live in test_gpu_filter_edges.py, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ALL = (0, 0, 0, 0xFFFFFFFF)
VOCAB = 64


@pytest.fixture(scope="module")
def O():
    from oracle import lib
    return lib


def _ctx(mode=None):
    import openintel_amd as oi
    c = oi.HipContext(0)
    if mode is not None:
        c.set_cosine_mode(mode)
    return c


def _corpus(n, dim, seed=0, long_rows=0):
    rng = np.random.default_rng(seed)
    rows = rng.integers(-2, 3, size=(n, dim)).astype(np.float32)
    if long_rows:  # rows far longer than the rest: the screen's two-class margin sets them aside (always rescored)
        rows[rng.choice(n, long_rows, replace=False)] *= 64
    lens = rng.integers(1, 9, size=n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    terms = rng.integers(0, VOCAB, size=int(offs[-1])).astype(np.uint32)
    group = rng.integers(0, 1 << 16, size=n).astype(np.uint32)
    stamp = rng.permutation(n).astype(np.uint32) * 3
    return rows, terms, offs, group, stamp


def _index(ctx, rows, terms, offs, group=None, stamp=None, base=0, bm25_mode=None, attrs=True, finalize=True):
    import openintel_amd as oi
    idx = oi.HybridIndex(ctx, rows.shape[0], rows.shape[1], VOCAB, base)
    idx.set_embeddings(rows, normalize=False)
    idx.set_forward(terms, offs)
    if bm25_mode is not None:
        idx.set_bm25_mode(bm25_mode)
    if attrs:
        idx.set_doc_attrs(group, stamp)
    if finalize:
        idx.finalize()
    return idx


def _queries(B, dim, seed=1):
    rng = np.random.default_rng(seed)
    q = rng.integers(-2, 3, size=(B, dim)).astype(np.float32)
    qt = rng.integers(0, VOCAB, size=3 * B).astype(np.uint32)
    qo = (3 * np.arange(B + 1)).astype(np.uint32)
    return q, qt, qo


def _passes(f, group, stamp):
    m, v, lo, hi = (int(x) for x in f)
    return ((group & np.uint32(m)) == np.uint32(v)) & (stamp >= np.uint32(lo)) & (stamp <= np.uint32(hi))


def _restrict(scores, docs, count, ok, depth, base=0):
    d = docs[:count].astype(np.int64)
    keep = ok[d - base]
    return scores[:count][keep][:depth], docs[:count][keep][:depth]


def _filters(B, group, seed=2):
    """a mix per batch: all-pass, 1/2, 1/16 and 1/4096 of the groups, a stamp window, one that passes nothing"""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        kind = b % 6
        if kind == 0:
            out.append(ALL)
        elif kind == 1:
            out.append((1, int(rng.integers(0, 2)), 0, 0xFFFFFFFF))
        elif kind == 2:
            out.append((0xF, int(rng.integers(0, 16)), 0, 0xFFFFFFFF))
        elif kind == 3:
            out.append((0xFFF, int(group[rng.integers(0, group.size)]) & 0xFFF, 0, 0xFFFFFFFF))
        elif kind == 4:
            out.append((0, 0, 300, 1500))
        else:
            out.append((0xFFFFFFFF, 0xFFFFFFFF, 0, 0xFFFFFFFF) if b % 12 == 5 else (0, 0, 7, 6))  # none pass
    return np.array(out, dtype=np.uint32)


def _check_restricted(idx, q, qt, qo, F, group, stamp, depth, base=0):
    """filtered lists at `depth` == the unfiltered depth = n lists restricted and cut, bit for bit (RRF too)"""
    from oracle import lib as O
    n = group.size
    full = idx.search_lists(q, qt, qo, depth=n)
    L = idx.search_lists(q, qt, qo, depth=depth, filters=F)
    k = min(depth, 50)
    R = idx.search(q, qt, qo, k=k, depth=depth, filters=F)
    for b in range(q.shape[0]):
        ok = _passes(F[b], group, stamp)
        cs, cd = _restrict(full.cos_scores[b], full.cos_docs[b], int(full.cos_counts[b]), ok, depth, base)
        c = int(L.cos_counts[b])
        assert c == cs.size == min(depth, int(ok.sum())), (b, c, cs.size)
        assert np.array_equal(L.cos_docs[b][:c], cd), b
        assert np.array_equal(L.cos_scores[b][:c].view(np.uint32), cs.view(np.uint32)), b
        bs, bd = _restrict(full.bm25_scores[b], full.bm25_docs[b], int(full.bm25_counts[b]), ok, depth, base)
        c = int(L.bm25_counts[b])
        assert c == bs.size, (b, c, bs.size)
        assert np.array_equal(L.bm25_docs[b][:c], bd), b
        assert np.array_equal(L.bm25_scores[b][:c].view(np.uint32), bs.view(np.uint32)), b
        rs, rd = O.rrf_fuse(cd, bd, k)
        c = int(R.counts[b])
        assert c == len(rd) and np.array_equal(R.docs[b][:c], np.asarray(rd, dtype=np.uint32)), b
        assert np.array_equal(R.scores[b][:c], np.asarray(rs, dtype=np.float32)), b
    return L


@pytest.mark.parametrize("mode,B,dim", [
    ("screen", 64, 768),    # the int8 tier
    ("screen", 1, 768),     # the copy screen, one query
    ("screen", 8, 768),     # the copy screen, GEMV-sized batch
    ("stream", 64, 768),    # the f32-stream screen (routed to the exact path under a filter)
    ("exact", 1, 768), ("exact", 9, 768), ("exact", 64, 768),
    ("split", 1, 384), ("split", 9, 384), ("split", 64, 384),
    ("screen", 9, 128),     # the generic dim: the exact tile kernel
])
def test_filtered_lists_are_the_restricted_full_ranking_on_every_cosine_route(mode, B, dim):
    from openintel_amd import _lib
    m = {"screen": _lib.OI_COSINE_SCREEN, "stream": _lib.OI_COSINE_SCREEN_STREAM, "exact": _lib.OI_COSINE_EXACT,
         "split": _lib.OI_COSINE_SPLIT}[mode]
    ctx = _ctx(m)
    n = 1000
    rows, terms, offs, group, stamp = _corpus(n, dim, seed=B + dim)
    idx = _index(ctx, rows, terms, offs, group, stamp)
    q, qt, qo = _queries(B, dim)
    F = _filters(B, group)
    if B == 1:
        F = np.array([(0xF, 3, 0, 0xFFFFFFFF)], np.uint32)
    _check_restricted(idx, q, qt, qo, F, group, stamp, depth=100)
    # the route the case names was the one taken: the last (filtered) search was screened or not, the copies exist
    gate = ctx.profile_read("screen_gate")[0]
    copies = idx.index_bytes()[1]
    if mode == "screen" and dim == 768 and B > 8:
        assert copies > 2 * n * dim and gate != -1.0, "the int8 tier: both screening copies, a screened search"
    elif mode == "screen" and dim == 768:
        assert copies >= 2 * n * dim and gate != -1.0, "the copy screen: the bf16 copy, a screened search"
    else:
        assert gate == -1.0, "an exact-path search (exact, split, the f32-stream screen's route, the generic dim)"
    idx.close()
    ctx.close()


@pytest.mark.parametrize("bm25_mode", [1, 2, 3, 4])
def test_every_bm25_mode_gives_the_restricted_list(bm25_mode):
    ctx = _ctx()
    n, dim, B = 1024, 384, 12
    rows, terms, offs, group, stamp = _corpus(n, dim, seed=7)
    idx = _index(ctx, rows, terms, offs, group, stamp, bm25_mode=bm25_mode)
    q, qt, qo = _queries(B, dim, seed=3)
    _check_restricted(idx, q, qt, qo, _filters(B, group, seed=5), group, stamp, depth=64)
    idx.close()
    ctx.close()


def test_all_pass_filter_returns_the_unfiltered_bytes_and_none_pass_returns_nothing():
    ctx = _ctx()
    n, dim, B = 4000, 768, 64
    rows, terms, offs, group, stamp = _corpus(n, dim, seed=11)
    idx = _index(ctx, rows, terms, offs, group, stamp)
    q, qt, qo = _queries(B, dim, seed=4)
    U = idx.search_lists(q, qt, qo, depth=200)
    A = idx.search_lists(q, qt, qo, depth=200, filters=np.tile(np.array(ALL, np.uint32), (B, 1)))
    for f in ("cos_scores", "cos_docs", "cos_counts", "bm25_scores", "bm25_docs", "bm25_counts"):
        assert np.array_equal(getattr(A, f).view(np.uint32), getattr(U, f).view(np.uint32)), f
    Z = idx.search_lists(q, qt, qo, depth=200, filters=np.tile(np.array((0, 0, 5, 4), np.uint32), (B, 1)))
    assert not Z.cos_counts.any() and not Z.bm25_counts.any()
    R = idx.search(q, qt, qo, k=10, depth=200, filters=np.tile(np.array((0, 0, 5, 4), np.uint32), (B, 1)))
    assert not R.counts.any()
    idx.close()
    ctx.close()


def _oracle_check(L, b, rows, terms, offs, q, qt, qo, ok, depth, O, bm_ref=None):
    ref = O.dot_scores(rows, q[b]).astype(np.float64)
    c = int(L.cos_counts[b])
    npass = int(ok.sum())
    assert c == min(depth, npass), (b, c, npass)
    if c:
        d = L.cos_docs[b][:c].astype(np.int64)
        assert ok[d].all() and np.unique(d).size == c
        s = L.cos_scores[b][:c].astype(np.float64)
        assert np.abs(s - ref[d]).max() <= 1e-5
        pref = np.where(ok, ref, -np.inf)
        kth = np.sort(pref)[::-1][c - 1]
        assert np.isin(np.nonzero(pref > kth + 2e-5)[0], d).all(), "a clearly better passing doc is missing"
    bm = O.bm25_scores(terms, offs, VOCAB, qt[qo[b]:qo[b + 1]]) if bm_ref is None else bm_ref
    bm = np.where(ok, bm, 0).astype(np.float32)
    rs, rd = O.topk(bm, depth, positive_only=True)
    c = int(L.bm25_counts[b])
    assert c == len(rd) == min(depth, int(((bm > 0) & ok).sum())), (b, c, len(rd))
    assert np.array_equal(L.bm25_docs[b][:c], np.asarray(rd, np.uint32))
    assert np.array_equal(L.bm25_scores[b][:c].view(np.uint32), np.asarray(rs, np.float32).view(np.uint32))


def test_chunk_edges_against_the_oracle(O):
    """300 000 rows (three screen chunks at depth 100; its 10 doc blocks are one BM25 phase -- the second phase has a test of
    its own below), the int8 tier (B = 16) and long rows that pass
    and fail; filters: 1/2, 1/100, fewer than depth, only the first / only the last chunk, exact stamp bounds, lo == hi."""
    ctx = _ctx()
    n, dim, B, depth = 300_000, 384, 16, 100
    rng = np.random.default_rng(21)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    long_ids = rng.choice(n, 40, replace=False)
    rows[long_ids] *= 8
    lens = rng.integers(1, 9, size=n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    terms = rng.integers(0, VOCAB, size=int(offs[-1])).astype(np.uint32)
    group = rng.integers(0, 100, size=n).astype(np.uint32)
    group[long_ids[:20]] = 7
    group[long_ids[20:]] = 8
    stamp = np.arange(n, dtype=np.uint32)
    idx = _index(ctx, rows, terms, offs, group, stamp)
    assert idx.long_rows() > 0
    q = rng.standard_normal((B, dim)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    qt = rng.integers(0, VOCAB, size=2 * B).astype(np.uint32)
    qo = (2 * np.arange(B + 1)).astype(np.uint32)
    F = np.array([
        (0x1, 0, 0, 0xFFFFFFFF), (0xFFFFFFFF, 7, 0, 0xFFFFFFFF), (0xFFFFFFFF, 8, 0, 0xFFFFFFFF), (0, 0, 0, 40),
        (0, 0, 0, 20_000), (0, 0, n - 20_000, 0xFFFFFFFF), (0, 0, 1234, 1234), (0, 0, 5000, 5099),
        (0xFFFFFFFF, 42, 100_000, 200_000), ALL, (0, 0, n - 1, n - 1), (0xFFFFFFFF, 7, 0, 60_000),
        (0xFFFFFFFF, 200, 0, 0xFFFFFFFF), (0x3, 1, 0, 0xFFFFFFFF), (0, 0, 28_000, 29_000), (0, 0, 257_000, 259_000),
    ], dtype=np.uint32)
    L = idx.search_lists(q, qt, qo, depth=depth, filters=F)
    for b in range(B):
        _oracle_check(L, b, rows, terms, offs, q, qt, qo, _passes(F[b], group, stamp), depth, O)
    idx.close()
    ctx.close()


def test_shards_views_retagging_and_errors():
    import openintel_amd as oi
    from openintel_amd import _lib
    ctx, ctx2 = _ctx(), _ctx()
    n, dim, B, depth = 6000, 768, 16, 50
    rows, terms, offs, group, stamp = _corpus(n, dim, seed=31)
    q, qt, qo = _queries(B, dim, seed=9)
    F = _filters(B, group, seed=8)
    # an index without attributes, a view of it: OI_ERR_STATE
    bare = _index(ctx, rows, terms, offs, attrs=False)
    with pytest.raises(_lib.OiError) as e:
        bare.search_lists(q, qt, qo, depth=depth, filters=F)
    assert e.value.code == _lib.OI_ERR_STATE
    v0 = bare.view(ctx2)
    with pytest.raises(_lib.OiError):
        v0.set_doc_attrs(group, stamp)
    bare.set_doc_attrs(group, stamp)  # after finalize; the view made before has none
    with pytest.raises(_lib.OiError):
        v0.search_lists(q, qt, qo, depth=depth, filters=F)
    v0.close()
    # one index == two shards through the packed exchange
    full = bare
    Rf = full.search(q, qt, qo, k=20, depth=depth, filters=F)
    h = n // 2
    s0 = _index(ctx, rows[:h], terms[:offs[h]], offs[:h + 1], group[:h], stamp[:h], finalize=False)
    s1 = _index(ctx, rows[h:], terms[offs[h]:], offs[h:] - offs[h], group[h:], stamp[h:], base=h, finalize=False)
    # (the global BM25 statistics: finalize each shard with the whole collection's)
    tot, df = full.local_stats()
    for s in (s0, s1):
        s.finalize(n, tot, df)
    p0 = s0.search_lists_packed(q, qt, qo, depth=depth, filters=F)
    p1 = s1.search_lists_packed(q, qt, qo, depth=depth, filters=F)
    fused = oi.fuse_packed(ctx, np.concatenate([p0, p1]), 2, B, depth, 20)
    assert np.array_equal(fused.counts, Rf.counts)
    for b in range(B):
        c = int(Rf.counts[b])
        assert np.array_equal(fused.docs[b][:c], Rf.docs[b][:c]) and np.array_equal(fused.scores[b][:c], Rf.scores[b][:c])
    # a view sees attributes set before it was made and in-place updates made later (retagging removes docs)
    v = full.view(ctx2)
    L1 = v.search_lists(q, qt, qo, depth=depth, filters=F)
    Lf = full.search_lists(q, qt, qo, depth=depth, filters=F)
    assert np.array_equal(L1.cos_docs, Lf.cos_docs) and np.array_equal(L1.bm25_docs, Lf.bm25_docs)
    gone = np.unique(np.concatenate([Lf.cos_docs[0][:int(Lf.cos_counts[0])], Lf.bm25_docs[0][:int(Lf.bm25_counts[0])]]))
    g2 = group.copy()
    g2[gone] = 0xDEAD0000  # F[0] passes everything: the stamp window removes them instead
    s2 = stamp.copy()
    s2[gone] = 0xFFFFFFF0
    F2 = F.copy()
    F2[0] = (0, 0, 0, 0xFFFFFF00)
    full.set_doc_attrs(g2, s2)
    ctx.synchronize()
    L2 = v.search_lists(q, qt, qo, depth=depth, filters=F2)
    assert not np.isin(L2.cos_docs[0][:int(L2.cos_counts[0])], gone).any()
    assert not np.isin(L2.bm25_docs[0][:int(L2.bm25_counts[0])], gone).any()
    assert int(L2.cos_counts[0]) == depth
    v.close()
    for s in (s0, s1, full):
        s.close()
    ctx.close()
    ctx2.close()


def test_native_world1_sharded_equals_search_filtered():
    import openintel_amd as oi
    from openintel_amd import _lib
    ctx = _ctx()
    n, dim, B, depth = 5000, 384, 9, 64
    rows, terms, offs, group, stamp = _corpus(n, dim, seed=41)
    idx = _index(ctx, rows, terms, offs, group, stamp, finalize=False)
    q, qt, qo = _queries(B, dim, seed=12)
    F = _filters(B, group, seed=13)
    comm = oi.NativeComm(ctx, oi.NativeComm.unique_id(), 0, 1)
    idx.finalize_sharded(comm)
    R = idx.search(q, qt, qo, k=20, depth=depth, filters=F)
    S = idx.search_sharded(comm, q, qt, qo, k=20, depth=depth, filters=F)
    assert np.array_equal(S.counts, R.counts) and np.array_equal(S.docs, R.docs) and np.array_equal(S.scores, R.scores)
    comm.close()
    idx.close()
    ctx.close()


def test_graph_replay_reads_the_filter_contents_at_replay_time():
    import torch
    ctx = _ctx()
    stream = torch.cuda.Stream(device="cuda:0")
    ctx.set_stream(stream)  # (replay needs a real stream, not the default one)
    ctx.set_graph_replay(True)
    n, dim, B, depth = 3000, 768, 16, 40
    rows, terms, offs, group, stamp = _corpus(n, dim, seed=51)
    idx = _index(ctx, rows, terms, offs, group, stamp)
    q, qt, qo = _queries(B, dim, seed=14)
    dev = "cuda:0"
    qd, qtd, qod = (torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to(dev) for x in (q, qt, qo))
    F1, F2 = _filters(B, group, seed=15), _filters(B, group, seed=16)
    Fd = torch.from_numpy(F1.view(np.int32)).to(dev)
    out = None
    for _ in range(3):  # eager, capture, replay
        out = idx.search(qd, qtd, qod, k=10, depth=depth, out=out, filters=Fd)
    ctx.synchronize()
    Fd.copy_(torch.from_numpy(F2.view(np.int32)).to(dev))
    torch.cuda.synchronize()
    out = idx.search(qd, qtd, qod, k=10, depth=depth, out=out, filters=Fd)
    ctx.synchronize()
    want = idx.search(q, qt, qo, k=10, depth=depth, filters=F2)
    assert ctx.profile_read("graph_replays")[1] >= 2, "the last two calls were replays"
    counts, docs = out.counts.cpu().numpy().view(np.uint32), out.docs.cpu().numpy().view(np.uint32)
    assert np.array_equal(counts, want.counts)
    for b in range(B):  # (past counts[b] the reused output holds what an earlier call left there)
        assert np.array_equal(docs[b][:counts[b]], want.docs[b][:counts[b]]), b
    idx.close()
    ctx.close()


@pytest.mark.parametrize("B,dim", [(64, 1024), (9, 1024), (64, 768)])
def test_bf16_corpus_filtered_lists_are_the_restricted_full_ranking(B, dim):
    """a bf16 corpus: a filtered search is pinned to the one-group kernel (cosine_bf16_filter); small integers are exact in
    bf16, so its lists equal the unfiltered ranking (the pair / query-split kernels at these batches) restricted, bit for bit"""
    import openintel_amd as oi
    ctx = _ctx()
    n = 1000
    rows, terms, offs, group, stamp = _corpus(n, dim, seed=61 + B)
    bits = (rows.view(np.uint32) >> 16).astype(np.uint16)  # (small integers: exact in bf16)
    idx = oi.HybridIndex(ctx, n, dim, VOCAB)
    idx.set_embeddings_bf16(bits)
    idx.set_forward(terms, offs)
    idx.set_doc_attrs(group, stamp)
    idx.finalize()
    q, qt, qo = _queries(B, dim, seed=17)
    _check_restricted(idx, q, qt, qo, _filters(B, group, seed=18), group, stamp, depth=100)
    idx.close()
    ctx.close()


def test_bm25_second_phase_against_the_oracle(O):
    """more than 48 doc blocks: under a filter the stream kernel runs its two-phase schedule (no impact floors) -- the first
    phase over the first blocks without a threshold, then the rest against the threshold a select took over the first
    phase's (filtered) candidates.  Lists bit-exact against the oracle restricted to the passing documents."""
    from openintel_amd import _lib
    ctx = _ctx(_lib.OI_COSINE_EXACT)
    n, dim, B, depth = 50 * 32768 + 1000, 4, 8, 200
    rng = np.random.default_rng(71)
    rows = rng.integers(-2, 3, size=(n, dim)).astype(np.float32)
    lens = rng.integers(1, 7, size=n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    terms = rng.integers(0, 512, size=int(offs[-1])).astype(np.uint32)
    group = rng.integers(0, 100, size=n).astype(np.uint32)
    stamp = np.arange(n, dtype=np.uint32)
    import openintel_amd as oi
    idx = oi.HybridIndex(ctx, n, dim, 512)
    idx.set_embeddings(rows, normalize=False)
    idx.set_forward(terms, offs)
    idx.set_doc_attrs(group, stamp)
    idx.finalize()
    qt = rng.integers(0, 512, size=3 * B).astype(np.uint32)
    qo = (3 * np.arange(B + 1)).astype(np.uint32)
    q = rng.integers(-2, 3, size=(B, dim)).astype(np.float32)
    F = np.array([
        (0x1, 0, 0, 0xFFFFFFFF),                 # 1/2
        (0xFFFFFFFF, 42, 0, 0xFFFFFFFF),         # 1/100
        (0, 0, 0, 8 * 32768 - 1),                # only the first phase's blocks
        (0, 0, 8 * 32768, 0xFFFFFFFF),           # only the second phase's
        (0, 0, n - 3000, 0xFFFFFFFF),            # the last 3000 docs: fewer than depth with a score > 0, perhaps
        (0xFFFFFFFF, 7, 1_000_000, 1_000_999),   # a handful
        ALL,
        (0, 0, 5, 4),                            # none
    ], dtype=np.uint32)
    ctx.profile_reset(1)
    L = idx.search_lists(q, qt, qo, depth=depth, filters=F)
    assert ctx.profile_read("bm25")[1] >= 3, "the plan launch and both phases of the stream kernel (one phase: 2)"
    ctx.profile_reset(0)
    for b in range(B):
        ok = _passes(F[b], group, stamp)
        bm = O.bm25_scores(terms, offs, 512, qt[qo[b]:qo[b + 1]])
        bm = np.where(ok, bm, 0).astype(np.float32)
        rs, rd = O.topk(bm, depth, positive_only=True)
        c = int(L.bm25_counts[b])
        assert c == len(rd) == min(depth, int(((bm > 0) & ok).sum())), (b, c, len(rd))
        assert np.array_equal(L.bm25_docs[b][:c], np.asarray(rd, np.uint32)), b
        assert np.array_equal(L.bm25_scores[b][:c].view(np.uint32), np.asarray(rs, np.float32).view(np.uint32)), b
    idx.close()
    ctx.close()


def test_device_attributes_and_the_sharded_retriever():
    """oi_index_set_doc_attrs from device tensors (one array None: zeros) through the strided copies, and the filters of
    ShardedRetriever.search (world 1) equal HybridIndex.search's"""
    import torch
    from openintel_amd import sharded
    ctx = _ctx()
    n, dim, B, depth = 1000, 384, 12, 64
    rows, terms, offs, group, stamp = _corpus(n, dim, seed=81)
    dev = "cuda:0"
    host = _index(ctx, rows, terms, offs, None, stamp)          # group None: zeros
    idx = _index(ctx, rows, terms, offs, attrs=False)
    torch.cuda.synchronize()
    idx.set_doc_attrs(None, torch.from_numpy(stamp.view(np.int32)).to(dev))
    q, qt, qo = _queries(B, dim, seed=19)
    F = np.array([(0xFFFFFFFF, 0, 300, 1800) if b % 2 else (0xFFFFFFFF, 1, 0, 0xFFFFFFFF) for b in range(B)], np.uint32)
    Lh = host.search_lists(q, qt, qo, depth=depth, filters=F)
    Ld = idx.search_lists(q, qt, qo, depth=depth, filters=F)
    for f in ("cos_scores", "cos_docs", "cos_counts", "bm25_scores", "bm25_docs", "bm25_counts"):
        assert np.array_equal(getattr(Ld, f).view(np.uint32), getattr(Lh, f).view(np.uint32)), f
    assert not Ld.cos_counts[0::2].any(), "group 1 never matches: the group array is zeros"
    _check_restricted(idx, q, qt, qo, F, np.zeros(n, np.uint32), stamp, depth=depth)
    # a device group array over the stamps already there (a retag in place)
    idx.set_doc_attrs(torch.from_numpy(group.view(np.int32)).to(dev), torch.from_numpy(stamp.view(np.int32)).to(dev))
    F2 = _filters(B, group, seed=20)
    _check_restricted(idx, q, qt, qo, F2, group, stamp, depth=depth)
    sr = sharded.make_hip_sharded(ctx, idx, torch.device(dev))
    qd, qtd, qod = (torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to(dev) for x in (q, qt, qo))
    s_scores, s_docs, s_counts = sr.search(qd, qtd, qod, 20, depth, filters=F2)
    R = idx.search(q, qt, qo, k=20, depth=depth, filters=F2)
    counts = s_counts.cpu().numpy().view(np.uint32)
    assert np.array_equal(counts, R.counts)
    docs = s_docs.cpu().numpy().view(np.uint32)
    for b in range(B):
        assert np.array_equal(docs[b][:counts[b]], R.docs[b][:counts[b]]), b
    for x in (host, idx):
        x.close()
    ctx.close()
