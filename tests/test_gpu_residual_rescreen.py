"""The residual rescreen of the int8 route (csrc/screen_i8_residual.hip: i8r_rescreen_kernel; search.hip: Plan::rescreen_residual).

Behind the last chunk the int8 survivors are thinned once more before the exact rescoring: from the residual plane where the index
holds it, from the bf16 copy otherwise.  The lists cannot depend on which: both are the exact rescoring of a superset of the exact
list, or the exact pipeline's behind an open gate.  HipContext.set_rescreen_tier takes both tails over ONE index in one process;
ctx.rescreen_state() tells which tail the last search took and how many keys its second margin select kept.

Every case compares the residual tail's lists bit for bit with the bf16 tail's; the cases that say so also with a context in
OI_COSINE_SCREEN_STREAM (no copy, no int8 tier), with speculation off, and with the f64 oracle at the suite's bar
(test_gpu_prefilter._check).  A list that equals the exact list with the gate shut is the rescoring of the kept set, so that set
held the exact list: the read-back counts then only have to show that the set is there (>= depth per query) and, on i.i.d. rows,
no larger than the bf16 tail's.

Shapes: n 20 000 .. 60 000 (80 000 once: the smallest round size at which a depth-64 search speculates), d 384 / 768, B 9 (one
query tile), 33 (two, the second ragged), 64 (two full), depth 16 .. 64."""
import numpy as np
import pytest

from test_gpu_prefilter import _check, _forward, _index

pytestmark = pytest.mark.gpu
VOCAB = 50
ALL = (0, 0, 0, 0xFFFFFFFF)


@pytest.fixture(scope="module")
def O():
    from oracle import lib
    return lib


@pytest.fixture(scope="module")
def corpus():
    """{dim: (rows[80 000], q[64])}: made once, never written to (the tests copy what they change)."""
    from openintel_amd import synth
    out = {}
    for dim in (384, 768):
        rows = synth.embeddings_np(80_000, dim, seed=1700 + dim)
        q = synth.embeddings_np(64, dim, seed=1800 + dim)
        rows.setflags(write=False)
        q.setflags(write=False)
        out[dim] = rows, q
    return out


@pytest.fixture()
def ctx():
    import openintel_amd as oi
    from openintel_amd import _lib
    c = oi.HipContext(0)
    c.set_cosine_mode(_lib.OI_COSINE_SCREEN)
    yield c
    c.close()


def _terms(B, seed=1):
    rng = np.random.default_rng(seed)
    return rng.integers(0, VOCAB, size=2 * B).astype(np.uint32), np.arange(0, 2 * B + 1, 2, dtype=np.uint32)


def _make(ctx, rows, base=0, plane=True):
    n, d = rows.shape
    terms, offs = _forward(np.random.default_rng(n), n, VOCAB)
    idx = _index(ctx, rows, terms, offs, VOCAB, base=base)
    assert idx.index_bytes()[1] >= 4 * n * d, "the index holds the two screening copies and the residual plane"
    assert idx.residual_plane() is not None
    if not plane:
        idx.residual_plane(drop=True)
    return idx


def _gate(ctx):
    return ctx.profile_read("screen_gate")[0]


def _same(L, R, queries=None):
    sel = slice(None) if queries is None else queries
    assert np.array_equal(L.cos_counts[sel], R.cos_counts[sel])
    assert np.array_equal(L.cos_docs[sel], R.cos_docs[sel])
    assert np.array_equal(L.cos_scores[sel].view(np.uint32), R.cos_scores[sel].view(np.uint32))


def _both_tails(ctx, idx, q, depth, filters=None, want=(1, 0)):
    """((lists, gate, keys kept in all, most for a query) of the residual tail, the same of the bf16 tail).  want: the tier each
    search must report (an index without the plane reports 0 whatever the switch says)."""
    qt, qo = _terms(q.shape[0])
    out = []
    for residual, tier in zip((True, False), want):
        ctx.set_rescreen_tier(residual)
        L = idx.search_lists(q, qt, qo, depth=depth, filters=filters)
        got, total, most = ctx.rescreen_state()
        assert got == tier, (residual, got)
        out.append((L, _gate(ctx), total, most))
    ctx.set_rescreen_tier(True)
    return out


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,B,n,depth", [(384, 9, 20_000, 16), (768, 33, 30_011, 64), (768, 64, 60_000, 64), (384, 64, 25_001, 32),
                                           (384, 33, 80_000, 64)])
def test_lists_are_the_bf16_tails_and_the_stream_screens(ctx, O, corpus, dim, B, n, depth):
    """i.i.d. rows: both tails, speculation on and off, the f32-stream screen and the oracle.  The residual tail keeps no more keys
    than the bf16 tail and at least depth per query."""
    from openintel_amd import _lib
    rows, q64 = corpus[dim]
    rows, q = rows[:n], q64[:B]
    idx = _make(ctx, rows, base=11)
    qt, qo = _terms(B)
    ref = None
    for spec in (True, False):
        ctx.set_screen_speculation(spec)
        s0 = ctx.speculation_state()[1]
        (Lr, gr, tot_r, most_r), (Lb, gb, tot_b, most_b) = _both_tails(ctx, idx, q, depth)
        assert ctx.speculation_state()[1] - s0 == (2 if spec and n == 80_000 else 0), "only the 80 000-row search speculates"
        print("d %d B %d n %d depth %d spec %d: keys kept residual %d (most %d), bf16 %d (most %d)" % (dim, B, n, depth, spec, tot_r, most_r, tot_b, most_b))
        assert gr == 0.0 and gb == 0.0
        _same(Lr, Lb)
        assert B * depth <= tot_r <= tot_b and most_r <= 4096
        if ref is not None:
            _same(Lr, ref)
        ref = Lr
    ctx.set_screen_speculation(True)
    ctx.set_cosine_mode(_lib.OI_COSINE_SCREEN_STREAM)
    Ls = idx.search_lists(q, qt, qo, depth=depth)
    assert ctx.rescreen_state()[0] == -1, "the f32-stream screen is not the int8 route"
    ctx.set_cosine_mode(_lib.OI_COSINE_SCREEN)
    _same(ref, Ls)
    for b in sorted({0, 8, B // 2, B - 1}):
        _check(ref, b, O.dot_scores(rows, q[b]), depth, n, base=11)
    idx.close()


@pytest.mark.parametrize("dim", [384, 768])
def test_more_ties_than_the_cap_open_the_gate(ctx, O, corpus, dim):
    """4 200 copies of one row that is a query's best: every copy ties with the k'-th score, inside any margin, and the second
    select cannot keep them in 4 096 keys.  The gate opens on both tails and the lists are the exact pipeline's."""
    B, n, depth = 33, 30_000, 32
    rows, q64 = corpus[dim]
    rows, q = rows[:n].copy(), q64[:B]
    rows[1000:5200] = q[4]
    idx = _make(ctx, rows)
    (Lr, gr, _, _), (Lb, gb, _, _) = _both_tails(ctx, idx, q, depth)
    assert gr != 0.0 and gb != 0.0, (gr, gb)
    _same(Lr, Lb)
    assert np.array_equal(Lr.cos_docs[4][:depth], np.arange(1000, 1000 + depth)), "equal scores rank by doc id"
    for b in (0, 4, B - 1):
        _check(Lr, b, O.dot_scores(rows, q[b]), depth, n)
    idx.close()


@pytest.mark.parametrize("dim,B", [(768, 33), (384, 64)])
def test_long_rows_are_rescored_whatever_the_tail(ctx, O, corpus, dim, B):
    """Twenty rows three times as long as the rest, near-copies of two queries: set aside as long, outside e2_max and the second
    select, rescored for every query.  They top their queries' lists on both tails and the gate stays shut."""
    n, depth = 40_000, 48
    rows, q64 = corpus[dim]
    rows, q = rows[:n].copy(), q64[:B]
    rng = np.random.default_rng(dim)
    where = {2: np.arange(300, 310), B - 1: 977 * np.arange(10) + 20_001}
    for b, ids in where.items():
        blk = q[b][None, :] + 0.02 * rng.standard_normal((ids.size, dim)).astype(np.float32) / np.sqrt(dim)
        rows[ids] = (3.0 * blk / np.linalg.norm(blk, axis=1, keepdims=True)).astype(np.float32)
    idx = _make(ctx, rows)
    assert idx.long_rows() == 20
    (Lr, gr, tot_r, _), (Lb, gb, tot_b, _) = _both_tails(ctx, idx, q, depth)
    assert gr == 0.0 and gb == 0.0
    _same(Lr, Lb)
    assert tot_r <= tot_b
    for b, ids in where.items():
        assert set(Lr.cos_docs[b][:ids.size].tolist()) == set(ids.tolist()), b
        _check(Lr, b, O.dot_scores(rows, q[b]), depth, n)
    idx.close()


def test_a_query_without_a_bound_opens_the_gate(ctx, O, corpus):
    """A non-finite query beside ordinary ones: its residual margin is +inf like its other margins, the gate opens on both tails,
    and the ordinary queries' lists are the same."""
    dim, B, n, depth = 384, 33, 20_000, 16
    rows, q64 = corpus[dim]
    rows, q = rows[:n], q64[:B].copy()
    q[5, 17] = np.inf
    idx = _make(ctx, rows)
    (Lr, gr, _, _), (Lb, gb, _, _) = _both_tails(ctx, idx, q, depth)
    assert gr != 0.0 and gb != 0.0
    ok = np.array([b for b in range(B) if b != 5])
    _same(Lr, Lb, ok)
    for b in (0, 4, 6, B - 1):
        _check(Lr, b, O.dot_scores(rows, q[b]), depth, n)
    idx.close()


def test_filtered_search_and_few_survivors(ctx, O, corpus):
    """A filtered search on both tails.  Queries 0..4 pass exactly 0, 1, 3, 4 and 5 rows (the rescreen takes four survivors per
    trip: none, a ragged trip, a full one, a full one and a ragged one), query 5 passes one group of sixteen, the rest all rows."""
    dim, B, n, depth = 768, 33, 20_000, 16
    rows, q64 = corpus[dim]
    rows, q = rows[:n], q64[:B]
    idx = _make(ctx, rows, base=5)
    idx.set_doc_attrs(np.arange(n, dtype=np.uint32) % 16, np.arange(n, dtype=np.uint32))
    few = {0: 0, 1: 1, 2: 3, 3: 4, 4: 5}
    F = np.tile(np.array(ALL, np.uint32), (B, 1))
    for b, c in few.items():
        F[b] = (0, 0, 7000 + 100 * b, 7000 + 100 * b + c - 1) if c else (0, 0, 7, 6)
    F[5] = (0xF, 3, 0, 0xFFFFFFFF)
    (Lr, gr, tot_r, _), (Lb, gb, tot_b, _) = _both_tails(ctx, idx, q, depth, filters=F)
    assert gr == 0.0 and gb == 0.0
    _same(Lr, Lb)
    for b, c in few.items():
        assert Lr.cos_counts[b] == c
        want = 5 + 7000 + 100 * b + np.arange(c)
        assert set(Lr.cos_docs[b][:c].tolist()) == set(want.tolist()), b
        ref = O.dot_scores(rows, q[b])
        assert np.abs(Lr.cos_scores[b][:c] - ref[Lr.cos_docs[b][:c].astype(np.int64) - 5]).max(initial=0.0) <= 1e-5
    ref = O.dot_scores(rows, q[5])
    ref[np.arange(n) % 16 != 3] = -np.inf
    d = Lr.cos_docs[5][:depth].astype(np.int64) - 5
    assert Lr.cos_counts[5] == depth and (d % 16 == 3).all()
    kth = np.sort(ref)[::-1][depth - 1]
    assert np.isin(np.nonzero(ref > kth + 2e-5)[0], d).all() and (ref[d] >= kth - 2e-5).all(), "the best sixteen of the group"
    _check(Lr, B - 1, O.dot_scores(rows, q[B - 1]), depth, n, base=5)
    idx.close()


def test_an_index_without_the_plane_takes_the_bf16_tail(ctx, O, corpus):
    """The plane is the first copy the AUTO budget leaves out.  Such an index (here: the plane dropped after finalize) reports
    tier 0 whatever the switch says and returns the lists of an index that holds it."""
    dim, B, n, depth = 384, 64, 25_001, 32
    rows, q64 = corpus[dim]
    rows, q = rows[:n], q64[:B]
    bare, full = _make(ctx, rows, plane=False), _make(ctx, rows)
    assert full.index_bytes()[1] - bare.index_bytes()[1] >= n * (dim + 8)
    (L0, g0, t0, _), (L1, g1, t1, _) = _both_tails(ctx, bare, q, depth, want=(0, 0))
    assert g0 == 0.0 and g1 == 0.0 and t0 == t1
    _same(L0, L1)
    (Lr, gr, _, _), _ = _both_tails(ctx, full, q, depth)
    _same(Lr, L0)
    bare.close()
    full.close()


def test_a_view_and_the_overlapped_legs_return_the_same(ctx, O, corpus):
    """A view (another context: its own switch, the owner's plane) takes the residual tail and returns the owner's lists; the
    hybrid call returns the same fused lists on either tail with the BM25 leg beside the cosine leg's tail and after it."""
    import openintel_amd as oi
    from openintel_amd import _lib
    dim, B, n, depth = 768, 64, 60_000, 64
    rows, q64 = corpus[dim]
    rows, q = rows[:n], q64[:B]
    idx = _make(ctx, rows, base=3)
    qt, qo = _terms(B)
    (Lr, gr, _, _), (Lb, gb, _, _) = _both_tails(ctx, idx, q, depth)
    assert gr == 0.0 and gb == 0.0
    _same(Lr, Lb)
    c2 = oi.HipContext(0)
    try:
        c2.set_cosine_mode(_lib.OI_COSINE_SCREEN)
        v = idx.view(c2)
        (Lv, gv, _, _), (Lw, gw, _, _) = _both_tails(c2, v, q, depth)
        assert gv == 0.0 and gw == 0.0
        _same(Lv, Lr)
        _same(Lw, Lr)
        v.close()
    finally:
        c2.close()
    out = []
    for residual in (True, False):
        ctx.set_rescreen_tier(residual)
        for overlap in (True, False):
            ctx.set_overlap(overlap)
            out.append(idx.search(q, qt, qo, k=10, depth=depth))
            assert ctx.rescreen_state()[0] == (1 if residual else 0) and _gate(ctx) == 0.0, (residual, overlap)
    ctx.set_overlap(True)
    ctx.set_rescreen_tier(True)
    for R in out[1:]:
        assert np.array_equal(out[0].counts, R.counts) and np.array_equal(out[0].docs, R.docs)
        assert np.array_equal(out[0].scores.view(np.uint32), R.scores.view(np.uint32))
    _check(Lr, 0, O.dot_scores(rows, q[0]), depth, n, base=3)
    idx.close()
