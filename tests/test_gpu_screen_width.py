"""The width of the int8 screen's launches and the fork point of the BM25 leg (search.hip: plan_search -- screen_wgs, tail_fork;
cosine_prefilter.hip: oi_cosine_screen_geometry at a given width).

The chunks of the int8 route take EVERY CU, one persistent workgroup of four waves each, when no other kernel runs beside them:
a search whose BM25 leg is not on the side stream (set_overlap(False)), or one whose leg is forked behind the last chunk (a last
chunk of >= 512 Ki rows).  Otherwise, through an index view, and on every other route, a screen launch takes 7/8 of the CUs.  The width changes which
segment of the pool a survivor lands in and nothing else, so every list must stay what the f32-stream screen
(OI_COSINE_SCREEN_STREAM, which never reads a copy and keeps 7/8) returns, bit for bit.

The corpus sizes put the edges of the wider grid into the SECOND chunk (depth 100, proven thresholds: 8 192 rows, then the
rest), with W = 4 x CUs waves, CUs read from the context: fewer tiles than waves, exactly one tile per wave and one row either
side of it, a last wave whose only tile is ragged, and two full tiles per wave with every (row, query) pair passing -- every
segment filled to its capacity."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
COS_TOL = 1e-5
VOCAB = 50
FIRST = 8192              # oi_screen_first_chunk_rows at depth 100 (below one round of the grid: not rounded)
DEPTH = 100


@pytest.fixture(scope="module")
def ctxs():
    """(the int8 route with the legs one after the other: full width; the f32-stream screen; the device's CUs)"""
    import openintel_amd as oi
    from openintel_amd import _lib
    a, s = oi.HipContext(0), oi.HipContext(0)
    a.set_cosine_mode(_lib.OI_COSINE_SCREEN)
    a.set_overlap(False)
    s.set_cosine_mode(_lib.OI_COSINE_SCREEN_STREAM)
    cus = a.screen_width()[1]
    assert cus >= 8
    yield a, s, cus
    a.close()
    s.close()


@pytest.fixture(scope="module")
def O():
    from oracle import lib
    return lib


_ROWS = {}


def base_rows(dim, n, cus):
    """Seeded unit rows, made once per dim: room for the first chunk and two tiles per wave of the widest grid."""
    from openintel_amd import synth
    have = _ROWS.get(dim)
    if have is None or have.shape[0] < n:
        _ROWS[dim] = have = synth.embeddings_np(max(n, FIRST + 2 * 4 * 32 * cus + 64), dim, seed=4100 + dim)
    return have[:n]


def _forward(n, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 9, size=n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    return rng.integers(0, VOCAB, size=int(offs[-1])).astype(np.uint32), offs


def _index(ctx, rows, base=0, policy=None):
    import openintel_amd as oi
    idx = oi.HybridIndex(ctx, rows.shape[0], rows.shape[1], VOCAB, base)
    if policy is not None:
        idx.set_screen_copy(policy)
    idx.set_embeddings(rows, normalize=False)
    idx.set_forward(*_forward(rows.shape[0], rows.shape[0]))
    idx.finalize()
    return idx


def _query_terms(B):
    rng = np.random.default_rng(B)
    return rng.integers(0, VOCAB, size=2 * B).astype(np.uint32), np.arange(0, 2 * B + 1, 2, dtype=np.uint32)


def same_lists(L1, L2):
    for f in ("cos_counts", "cos_docs", "bm25_counts", "bm25_docs"):
        assert np.array_equal(getattr(L1, f), getattr(L2, f)), f
    assert np.array_equal(L1.cos_scores.view(np.uint32), L2.cos_scores.view(np.uint32))
    assert np.array_equal(L1.bm25_scores.view(np.uint32), L2.bm25_scores.view(np.uint32))


def check_oracle(L, b, ref, depth, n, base):
    c = int(L.cos_counts[b])
    assert c == min(depth, n)
    d, s = L.cos_docs[b][:c].astype(np.int64) - base, L.cos_scores[b][:c]
    assert np.unique(d).size == c and d.min() >= 0 and d.max() < n
    assert np.abs(s.astype(np.float64) - ref[d]).max() <= COS_TOL
    kth = np.sort(ref)[::-1][c - 1]
    assert np.isin(np.nonzero(ref > kth + 2 * COS_TOL)[0], d).all(), "a clearly better doc is missing"
    assert (ref[d] >= kth - 2 * COS_TOL).all(), "a clearly worse doc is present"


def both(ctxs, rows, q, depth, base=0, width=None):
    """Lists through the int8 route at full width and through the f32-stream screen; the int8 search's widest launch."""
    a, s, cus = ctxs
    qt, qo = _query_terms(q.shape[0])
    ia = _index(a, rows, base)
    assert ia.index_bytes()[1] >= 3 * rows.shape[0] * rows.shape[1], "the index holds both screening copies"
    a.profile_reset(1)
    La = ia.search_lists(q, qt, qo, depth=depth)
    launches = int(a.profile_read("cosine")[1])
    gate = a.profile_read("screen_gate")[0]
    a.profile_reset(0)
    assert a.screen_width() == (cus if width is None else width, cus), "the chunks' width"
    ia.close()
    i_s = _index(s, rows, base)
    Ls = i_s.search_lists(q, qt, qo, depth=depth)
    assert s.screen_width()[0] <= cus * 7 // 8, "the f32-stream screen keeps 7/8 of the CUs"
    i_s.close()
    return La, Ls, launches, gate


def second_chunk_rows(case, cus):
    """Rows of the second chunk: the edges of a grid of W = 4 x cus waves of 32-row tiles."""
    W = 4 * cus
    return {"fewer_tiles_than_waves": 32 * (W - 3),       # the last three waves own no tile
            "one_tile_per_wave_minus_1": 32 * W - 1,      # the last wave's tile is one row short
            "one_tile_per_wave": 32 * W,
            "one_tile_per_wave_plus_1": 32 * W + 1,       # the first wave owns a second tile of one row; seg_cap doubles
            "last_wave_ragged_12": 32 * (W - 1) + 12}[case]


@pytest.mark.parametrize("dim,B", [(768, 64), (768, 33), (384, 64), (384, 33)])
@pytest.mark.parametrize("case", ["fewer_tiles_than_waves", "one_tile_per_wave_minus_1", "one_tile_per_wave",
                                  "one_tile_per_wave_plus_1", "last_wave_ragged_12"])
def test_full_width_second_chunk_edges(ctxs, O, case, dim, B):
    """Each query's two best rows are the last two of the corpus (the last wave's tile, the ragged one where there is one), a third
    sits in the first wave's first tile of the second chunk: a segment offset or a tile count off by one at the wider grid loses them."""
    from openintel_amd import synth
    cus = ctxs[2]
    n = FIRST + second_chunk_rows(case, cus)
    rows = base_rows(dim, n, cus)
    q = synth.embeddings_np(B, dim, seed=4200 + B + dim)
    touched = [FIRST, n - 2, n - 1]
    saved = rows[touched].copy()
    try:
        v = q[0][None, :] + np.array([[0.3], [0.2], [0.1]], np.float32) * rows[touched]
        rows[touched] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
        La, Ls, launches, gate = both(ctxs, rows, q, DEPTH, base=7)
        assert launches == 2 and gate == 0.0
        same_lists(La, Ls)
        for b in sorted({0, 31, 32, B - 1}):
            check_oracle(La, b, O.dot_scores(rows, q[b]).astype(np.float64), DEPTH, n, 7)
        assert La.cos_docs[0][:3].tolist() == [n - 1 + 7, n - 2 + 7, FIRST + 7]
    finally:
        rows[touched] = saved


@pytest.mark.parametrize("dim,B,depth", [(768, 64, 100), (384, 33, 1000)])
def test_every_pair_passes_every_segment_fills(ctxs, dim, B, depth):
    """n copies of one row: no threshold can drop a pair, in the first chunk (8 192 rows at depth 100, 28 672 at depth 1000: every
    one of its segments is filled to its 128 rows) or in the second, whose cus segments each take exactly their capacity of
    2 x 4 x 32 keys per query.  More keys than the tier carries: the gate opens; every list is the first `depth` doc ids.
    (Proven thresholds only: with speculation a corpus this small gets the short first chunk at depth 1000.)"""
    from openintel_amd import synth
    a, s, cus = ctxs
    first = FIRST if depth == 100 else 28_672
    n = first + 2 * 4 * 32 * cus
    rows = np.repeat(synth.embeddings_np(1, dim, seed=4300 + dim), n, axis=0)
    q = synth.embeddings_np(B, dim, seed=4301 + B)
    a.set_screen_speculation(False)
    s.set_screen_speculation(False)
    try:
        La, Ls, launches, gate = both(ctxs, rows, q, depth, base=3, width=cus)
    finally:
        a.set_screen_speculation(True)
        s.set_screen_speculation(True)
    assert launches == 2 and gate != 0.0
    same_lists(La, Ls)
    assert (La.cos_counts == depth).all()
    assert np.array_equal(La.cos_docs, np.tile(np.arange(3, 3 + depth, dtype=np.uint32), (B, 1)))


def test_hybrid_forked_behind_the_last_chunk_equals_serial_legs():
    """Two chunks, the last of 512 Ki rows + 37: with the legs overlapped the BM25 leg is forked behind the last chunk (the chunks
    take every CU, which only that fork point allows); with set_overlap(False) it runs after the cosine leg.  Every output of
    search and of search_lists is the same."""
    import openintel_amd as oi
    from openintel_amd import _lib, synth
    dim, B, k = 384, 64, 10
    n = FIRST + (512 << 10) + 37
    rows = synth.embeddings_np(n, dim, seed=4400)
    q = synth.embeddings_np(B, dim, seed=4401)
    qt, qo = _query_terms(B)
    c = oi.HipContext(0)
    try:
        c.set_cosine_mode(_lib.OI_COSINE_SCREEN)
        cus = c.screen_width()[1]
        idx = _index(c, rows, base=11)
        out = {}
        for overlap in (True, False, True):
            c.set_overlap(overlap)
            c.profile_reset(1)
            L = idx.search_lists(q, qt, qo, depth=DEPTH)
            assert int(c.profile_read("cosine")[1]) == 2, "two chunks"
            c.profile_reset(0)
            assert c.screen_width() == (cus, cus), ("full width: the leg is not beside a chunk", overlap)
            assert c.profile_read("screen_gate")[0] == 0.0
            R = idx.search(q, qt, qo, k=k, depth=DEPTH)
            out.setdefault(overlap, []).append((L, R))
        idx.close()
    finally:
        c.close()
    (L0, R0), (L2, R2) = out[True]
    (L1, R1), = out[False]
    for L, R in ((L1, R1), (L2, R2)):
        same_lists(L0, L)
        assert np.array_equal(R0.counts, R.counts) and np.array_equal(R0.docs, R.docs)
        assert np.array_equal(R0.scores.view(np.uint32), R.scores.view(np.uint32))


def test_overlapped_legs_beside_short_chunks_and_views_keep_seven_eighths(ctxs):
    """A last chunk too short for the late fork: the BM25 leg starts with the search and runs beside the chunks, which keep 7/8
    of the CUs.  A search through a view (a lane of a pipeline: another lane's kernels want the free CUs) keeps 7/8 whatever the
    legs do.  The lists are those of the full-width search."""
    import openintel_amd as oi
    from openintel_amd import _lib, synth
    a, _, cus = ctxs
    dim, B = 768, 33
    n = FIRST + 32 * 4 * cus + 5
    rows = base_rows(dim, n, cus)
    q = synth.embeddings_np(B, dim, seed=4500)
    qt, qo = _query_terms(B)
    idx = _index(a, rows)
    Lw = idx.search_lists(q, qt, qo, depth=DEPTH)
    assert a.screen_width() == (cus, cus)
    c = oi.HipContext(0)
    try:
        c.set_cosine_mode(_lib.OI_COSINE_SCREEN)
        own = _index(c, rows)
        Ln = own.search_lists(q, qt, qo, depth=DEPTH)
        assert c.screen_width() == (cus * 7 // 8, cus), "legs overlapped from the start"
        own.close()
        c.set_overlap(False)
        v = idx.view(c)
        Lv = v.search_lists(q, qt, qo, depth=DEPTH)
        assert c.screen_width() == (cus * 7 // 8, cus), "a view"
        v.close()
    finally:
        c.close()
    idx.close()
    same_lists(Lw, Ln)
    same_lists(Lw, Lv)


def test_width_does_not_leak_between_routes_on_one_context(ctxs):
    """int8, then the bf16 copy route (an index without copies under OI_COSINE_SCREEN_COPY: the bf16 copy is made on first use,
    no int8 one), then int8 again, all on one context: full width, 7/8, full width, and the same lists three times."""
    import openintel_amd as oi
    from openintel_amd import _lib, synth
    a, _, cus = ctxs
    dim, B = 384, 33
    n = FIRST + 2 * 32 * 4 * cus + 5
    rows = base_rows(dim, n, cus)
    q = synth.embeddings_np(B, dim, seed=4600)
    qt, qo = _query_terms(B)
    i8 = _index(a, rows)
    cp = _index(a, rows, policy=oi.HybridIndex.SCREEN_COPY_NEVER)
    assert cp.index_bytes()[1] == 0
    try:
        L1 = i8.search_lists(q, qt, qo, depth=DEPTH)
        assert a.screen_width() == (cus, cus)
        a.set_cosine_mode(_lib.OI_COSINE_SCREEN_COPY)
        L2 = cp.search_lists(q, qt, qo, depth=DEPTH)
        assert a.screen_width() == (cus * 7 // 8, cus)
        assert 0 < cp.index_bytes()[1] < 3 * n * dim, "the bf16 copy alone"
        a.set_cosine_mode(_lib.OI_COSINE_SCREEN)
        L3 = i8.search_lists(q, qt, qo, depth=DEPTH)
        assert a.screen_width() == (cus, cus)
    finally:
        a.set_cosine_mode(_lib.OI_COSINE_SCREEN)
        i8.close()
        cp.close()
    same_lists(L1, L2)
    same_lists(L1, L3)
