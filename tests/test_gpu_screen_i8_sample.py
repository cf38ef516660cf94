"""The sample pass of the int8 route (search.hip: Plan::sample_rows; cosine_screen_i8.hip: i8s_sample_kernel; sample_rank.hip).

Where the plan would predict a threshold right after its threshold-less first chunk, the int8 route scores those rows into a dense
key array instead, takes the r-th largest key per query (r = 3 k' m / n + 12) and screens the first chunk from row 0 under the
predicted threshold.  The lists cannot depend on it: they are the exact rescoring of a superset of the exact list, or the exact
pipeline's behind an open gate.  Every case here is compared, bit for bit, with the same index searched with
set_screen_speculation(False) -- the pooled first chunk and proven thresholds, code the sample pass does not touch -- and with
the f64 oracle at the suite's bar (test_gpu_prefilter._check).

Shapes: depth 100, so the sample is 8 192 rows; N0 = 64 674 rows is the smallest corpus for which the plan speculates after the
first chunk (2 (ceil(3 * 100 * 8192 / n) + 12) <= 100); d 384 and 768; B 9 (one query tile), 33 (two, the second ragged) and 64
(two full).  ctx.profile_read("screen_sample") tells which route a search took."""
import numpy as np
import pytest

from test_gpu_prefilter import _check, _forward, _index

pytestmark = pytest.mark.gpu

DEPTH, SAMPLE, VOCAB = 100, 8192, 50


def _rank(n, depth=DEPTH, m=SAMPLE):
    return (3 * depth * m + n - 1) // n + 12


N0 = next(n for n in range(60_000, 70_000) if 2 * _rank(n) <= DEPTH)
assert N0 == 64_674 and 2 * _rank(N0 - 1) > DEPTH
N1 = N0 + 1531                                      # a little above, off the tile grid


@pytest.fixture(scope="module")
def O():
    from oracle import lib
    return lib


@pytest.fixture(scope="module")
def corpus():
    """{dim: (rows[N1], q[64], forward index)}: made once, never written to (the tests copy what they change)."""
    from openintel_amd import synth
    out = {}
    for dim in (384, 768):
        rows = synth.embeddings_np(N1, dim, seed=700 + dim)
        q = synth.embeddings_np(64, dim, seed=800 + dim)
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


def _make(ctx, rows, base=0):
    terms, offs = _forward(np.random.default_rng(rows.shape[0]), rows.shape[0], VOCAB)
    idx = _index(ctx, rows, terms, offs, VOCAB, base=base)
    assert idx.index_bytes()[1] >= 3 * rows.shape[0] * rows.shape[1], "the index holds both screening copies"
    return idx


def _sample(ctx):
    return int(ctx.profile_read("screen_sample")[0])


def _gate(ctx):
    return ctx.profile_read("screen_gate")[0]


def _same(L, R, queries=None):
    sel = slice(None) if queries is None else queries
    assert np.array_equal(L.cos_counts[sel], R.cos_counts[sel])
    assert np.array_equal(L.cos_docs[sel], R.cos_docs[sel])
    assert np.array_equal(L.cos_scores[sel].view(np.uint32), R.cos_scores[sel].view(np.uint32))


def _on_and_off(ctx, idx, q, depth=DEPTH):
    """(lists with speculation, their route and gate, the reference lists without it and their gate)."""
    qt, qo = _terms(q.shape[0])
    ctx.set_screen_speculation(True)
    L = idx.search_lists(q, qt, qo, depth=depth)
    took, gate = _sample(ctx), _gate(ctx)
    ctx.set_screen_speculation(False)
    R = idx.search_lists(q, qt, qo, depth=depth)
    assert _sample(ctx) == 0, "no sample pass without speculation"
    gate_ref = _gate(ctx)
    ctx.set_screen_speculation(True)
    return L, took, gate, R, gate_ref


def _near_copies(q_row, count, rng, scale=1.0):
    blk = q_row[None, :] + 0.02 * rng.standard_normal((count, q_row.size)).astype(np.float32) / np.sqrt(q_row.size)
    return (scale * blk / np.linalg.norm(blk, axis=1, keepdims=True)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [384, 768])
@pytest.mark.parametrize("n", [N0 - 1, N0, N1])
def test_route_and_lists_at_the_speculating_size(ctx, O, corpus, dim, n):
    """Just below N0 the plan makes no prediction after the first chunk: no sample pass, the parent's route.  At N0 and above the
    sample is the 8 192 rows of the short first chunk.  Either way the lists are the reference's and meet the oracle's bar."""
    rows, q64 = corpus[dim]
    rows = rows[:n]
    idx = _make(ctx, rows, base=7)
    for B in (9, 33, 64):
        q = q64[:B]
        f0, s0 = ctx.speculation_state()
        L, took, gate, R, gate_ref = _on_and_off(ctx, idx, q)
        f1, s1 = ctx.speculation_state()
        assert took == (SAMPLE if n >= N0 else 0), (B, took)
        assert gate == 0.0 and gate_ref == 0.0, (B, gate, gate_ref)
        assert (f1, s1) == (f0, s0 + (1 if n >= N0 else 0)), "a search with a sample pass has speculated, and its check has held"
        _same(L, R)
        for b in sorted({0, 8, B // 2, B - 1}):
            _check(L, b, O.dot_scores(rows, q[b]), DEPTH, n, base=7)
    idx.close()


@pytest.mark.parametrize("dim,B", [(768, 64), (384, 33), (768, 9)])
def test_winners_at_the_sample_edges_are_listed_once(ctx, O, corpus, dim, B):
    """The first chunk screens the sample rows again: a winner at the first and last row of the sample's first tile, at the first
    row of its second, at its last row and at the first row past it is each listed once, at the top of its query's list."""
    rows, q64 = corpus[dim]
    rows, q = rows[:N0].copy(), q64[:B]
    planted = {0: 0, 31: 1, 32: B // 2, SAMPLE - 1: B - 2, SAMPLE: B - 1}  # row -> query
    for r, b in planted.items():
        rows[r] = q[b]
    idx = _make(ctx, rows)
    L, took, gate, R, gate_ref = _on_and_off(ctx, idx, q)
    assert took == SAMPLE and gate == 0.0 and gate_ref == 0.0
    _same(L, R)
    for r, b in planted.items():
        d = L.cos_docs[b][:DEPTH]
        assert d[0] == r and (d == r).sum() == 1, (r, b, d[:4])
    for b in range(B):
        assert np.unique(L.cos_docs[b][:DEPTH]).size == DEPTH, b
    for b in sorted(set(planted.values())):
        _check(L, b, O.dot_scores(rows, q[b]), DEPTH, N0)
    idx.close()


@pytest.mark.parametrize("dim,B", [(768, 33), (384, 64)])
def test_long_rows_in_the_sample_do_not_lift_the_threshold(ctx, O, corpus, dim, B):
    """r + 10 rows three times as long as the rest, near-copies of a query, sit in the sample: their screen scores top the
    batch.  They are set aside as long (always rescored, no part in any threshold): had they entered the r-th largest key, the
    predicted threshold would sit near 3 and the check would fail.  The gate stays shut and the lists are the reference's."""
    rows, q64 = corpus[dim]
    rows, q = rows[:N0].copy(), q64[:B]
    rng = np.random.default_rng(dim + B)
    cnt = _rank(N0) + 10
    where = {0: np.arange(40, 40 + cnt), B - 1: 64 * np.arange(cnt) + 4001}  # contiguous over three tiles; one in every other tile
    for b, ids in where.items():
        rows[ids] = _near_copies(q[b], cnt, rng, scale=3.0)
    idx = _make(ctx, rows)
    assert idx.long_rows() == 2 * cnt
    f0, _ = ctx.speculation_state()
    L, took, gate, R, gate_ref = _on_and_off(ctx, idx, q)
    assert took == SAMPLE and gate == 0.0 and gate_ref == 0.0, (took, gate, gate_ref)
    assert ctx.speculation_state()[0] == f0, "the check held"
    _same(L, R)
    for b, ids in where.items():
        assert set(ids.tolist()) <= set(L.cos_docs[b][:DEPTH].tolist()), b
    idx.close()


@pytest.mark.parametrize("layout", ["two-tiles", "one-per-tile"])
def test_an_unfair_sample_fails_the_check_and_backs_off(ctx, O, corpus, layout):
    """r + 10 near-copies of a query in the sample and none after it: the r-th largest key of the sample sits near 1, which only
    r + 10 rows of the corpus reach.  The r-th largest is taken over every sample key, so it does not matter whether the copies
    share two tiles or sit one per tile: the check fails, the gate opens, the lists are the exact scorer's, and the context backs
    off -- its next searches take the pooled first chunk with proven thresholds."""
    dim, B = 768, 33
    rows, q64 = corpus[dim]
    rows, q = rows[:N0].copy(), q64[:B]
    rng = np.random.default_rng(len(layout))
    cnt = _rank(N0) + 10
    ids = 96 + np.arange(cnt) if layout == "two-tiles" else 32 * np.arange(cnt) + 7
    assert layout != "two-tiles" or (ids[0] // 32 + 1 == ids[-1] // 32), "two tiles"
    victims = (0, B - 1)                                # one query of each query tile; the same rows cannot serve both
    rows[ids] = _near_copies(q[victims[0]], cnt, rng)
    rows[ids + 4096] = _near_copies(q[victims[1]], cnt, rng)
    idx = _make(ctx, rows)
    qt, qo = _terms(B)
    f0, s0 = ctx.speculation_state()
    L = idx.search_lists(q, qt, qo, depth=DEPTH)
    assert _sample(ctx) == SAMPLE
    assert _gate(ctx) != 0.0, "the speculation must have failed its check"
    for b, at in zip(victims, (ids, ids + 4096)):
        _check(L, b, O.dot_scores(rows, q[b]), DEPTH, N0)
        assert set(at.tolist()) <= set(L.cos_docs[b][:DEPTH].tolist()), b
    _check(L, B // 2, O.dot_scores(rows, q[B // 2]), DEPTH, N0)
    assert ctx.speculation_state() == (f0 + 1, s0 + 1), "one failure, one back-off"
    for _ in range(2):                                  # backed off: the pooled route, proven thresholds, no fallback
        L2 = idx.search_lists(q, qt, qo, depth=DEPTH)
        assert _sample(ctx) == 0 and _gate(ctx) == 0.0
        assert np.array_equal(L2.cos_docs, L.cos_docs) or np.abs(L2.cos_scores - L.cos_scores).max() <= 5e-7
    assert ctx.speculation_state() == (f0 + 1, s0 + 1), "no speculation while backed off"
    idx.close()


def test_a_query_without_a_bound_is_gated_as_before(ctx, O, corpus):
    """One query with a non-finite norm beside normal ones: staging opens the gate for the batch with and without speculation, the
    sample pass gives that query no threshold (m2 = +inf), and the normal queries' lists are the reference's."""
    dim, B = 384, 33
    rows, q64 = corpus[dim]
    rows, q = rows[:N0], q64[:B].copy()
    q[5, 17] = np.inf
    idx = _make(ctx, rows)
    L, took, gate, R, gate_ref = _on_and_off(ctx, idx, q)
    assert took == SAMPLE
    assert gate != 0.0 and gate_ref != 0.0, (gate, gate_ref)
    ok = np.array([b for b in range(B) if b != 5])
    _same(L, R, ok)
    for b in (0, 4, 6, B - 1):
        _check(L, b, O.dot_scores(rows, q[b]), DEPTH, N0)
    idx.close()


def test_no_state_is_left_between_searches(O, corpus):
    """One context: a batch of 64, a different batch of 33, then speculation off and on again.  Every result equals that of a fresh
    context that has run nothing else: no threshold, prediction or key of an earlier search is read by a later one."""
    import openintel_amd as oi
    from openintel_amd import _lib
    dim = 384
    rows, q64 = corpus[dim]
    rows = rows[:N1]
    q1, q2 = q64, np.ascontiguousarray(q64[::-1][:33])

    def fresh(q, spec):
        c = oi.HipContext(0)
        try:
            c.set_cosine_mode(_lib.OI_COSINE_SCREEN)
            c.set_screen_speculation(spec)
            i = _make(c, rows)
            L = i.search_lists(q, *_terms(q.shape[0]), depth=DEPTH)
            took = _sample(c)
            i.close()
        finally:
            c.close()
        return L, took

    a = oi.HipContext(0)
    try:
        a.set_cosine_mode(_lib.OI_COSINE_SCREEN)
        ia = _make(a, rows)
        got = []
        for q, spec in ((q1, True), (q2, True), (q1, False), (q1, True), (q2, True)):
            a.set_screen_speculation(spec)
            got.append((ia.search_lists(q, *_terms(q.shape[0]), depth=DEPTH), _sample(a), _gate(a)))
        ia.close()
    finally:
        a.close()
    want = {(1, True): fresh(q1, True), (2, True): fresh(q2, True), (1, False): fresh(q1, False)}
    for (L, took, gate), key in zip(got, ((1, True), (2, True), (1, False), (1, True), (2, True))):
        R, took_ref = want[key]
        assert took == took_ref == (SAMPLE if key[1] else 0) and gate == 0.0, (key, took, took_ref, gate)
        _same(L, R)
    _check(got[0][0], 0, O.dot_scores(rows, q1[0]), DEPTH, N1)
    _check(got[1][0], 32, O.dot_scores(rows, q2[32]), DEPTH, N1)


def test_a_view_and_the_overlapped_legs_return_the_same(ctx, O, corpus):
    """A view of the index (another context; its screen keeps 7/8 of the CUs) takes the sample pass and returns the owner's lists;
    the hybrid call returns the same fused lists with the BM25 leg beside the cosine leg and after it."""
    import openintel_amd as oi
    from openintel_amd import _lib
    dim, B = 768, 64
    rows, q64 = corpus[dim]
    rows, q = rows[:N1], q64[:B]
    idx = _make(ctx, rows, base=3)
    qt, qo = _terms(B)
    L, took, gate, R, gate_ref = _on_and_off(ctx, idx, q)
    assert took == SAMPLE and gate == 0.0
    _same(L, R)
    c2 = oi.HipContext(0)
    try:
        c2.set_cosine_mode(_lib.OI_COSINE_SCREEN)
        v = idx.view(c2)
        Lv = v.search_lists(q, qt, qo, depth=DEPTH)
        cus = c2.screen_width()[1]
        assert _sample(c2) == SAMPLE and _gate(c2) == 0.0 and c2.screen_width()[0] <= max(1, cus * 7 // 8)
        _same(Lv, L)
        v.close()
    finally:
        c2.close()
    out = []
    for overlap in (True, False):
        ctx.set_overlap(overlap)
        out.append(idx.search(q, qt, qo, k=10, depth=DEPTH))
        assert _sample(ctx) == SAMPLE and _gate(ctx) == 0.0, overlap
    ctx.set_overlap(True)
    assert np.array_equal(out[0].counts, out[1].counts) and np.array_equal(out[0].docs, out[1].docs)
    assert np.array_equal(out[0].scores.view(np.uint32), out[1].scores.view(np.uint32))
    _check(L, 0, O.dot_scores(rows, q[0]), DEPTH, N1, base=3)
    idx.close()
