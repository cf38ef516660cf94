"""The int8 first screening tier (csrc/cosine_screen_i8.hip): an index that holds both screening copies screens a
batch of B > 8 queries against the int8 copy with per-row bounds, rescreens the survivors from the bf16 copy and goes on through
the bf16 screen's final select, rescoring and gate.  The lists must be those of the f32-stream screen (OI_COSINE_SCREEN_STREAM,
which never reads a copy) bit for bit, and meet the exact scorer's bar; int8 worst cases, the tier's own carry overflow,
speculation on and off and an index view are covered here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
COS_TOL = 1e-5


@pytest.fixture(scope="module")
def ctxs():
    import openintel_amd as oi
    from openintel_amd import _lib
    a, s = oi.HipContext(0), oi.HipContext(0)
    a.set_cosine_mode(_lib.OI_COSINE_SCREEN)
    s.set_cosine_mode(_lib.OI_COSINE_SCREEN_STREAM)
    yield a, s
    a.close()
    s.close()


@pytest.fixture(scope="module")
def O():
    from oracle import lib
    return lib


def _forward(rng, n, vocab=50):
    lens = rng.integers(1, 9, size=n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    return rng.integers(0, vocab, size=int(offs[-1])).astype(np.uint32), offs


def _index(ctx, rows, base=0, seed=0):
    import openintel_amd as oi
    terms, offs = _forward(np.random.default_rng(seed), rows.shape[0])
    idx = oi.HybridIndex(ctx, rows.shape[0], rows.shape[1], 50, base)
    idx.set_embeddings(rows, normalize=False)
    idx.set_forward(terms, offs)
    idx.finalize()
    return idx


def _check(L, b, ref, depth, n, base=0):
    c = int(L.cos_counts[b])
    assert c == min(depth, n)
    d, s = L.cos_docs[b][:c].astype(np.int64) - base, L.cos_scores[b][:c]
    assert np.unique(d).size == c and d.min() >= 0 and d.max() < n
    assert np.abs(s.astype(np.float64) - ref[d]).max() <= COS_TOL
    kth = np.sort(ref)[::-1][c - 1]
    assert np.isin(np.nonzero(ref > kth + 2 * COS_TOL)[0], d).all(), "a clearly better doc is missing"
    assert (ref[d] >= kth - 2 * COS_TOL).all(), "a clearly worse doc is present"


def _same_lists(L1, L2):
    assert np.array_equal(L1.cos_counts, L2.cos_counts)
    assert np.array_equal(L1.cos_docs, L2.cos_docs)
    assert np.array_equal(L1.cos_scores.view(np.uint32), L2.cos_scores.view(np.uint32))


def _both(ctxs, rows, q, depth, base=0):
    """(lists through the int8 tier, lists of the f32-stream screen, the int8 search's gate)"""
    a, s = ctxs
    B = q.shape[0]
    qt, qo = np.zeros(B, np.uint32), np.arange(B + 1, dtype=np.uint32)
    ia = _index(a, rows, base)
    assert ia.index_bytes()[1] > 2 * rows.shape[0] * rows.shape[1], "the index holds both screening copies"
    La = ia.search_lists(q, qt, qo, depth=depth)
    gate = a.profile_read("screen_gate")[0]
    ia.close()
    i_s = _index(s, rows, base)
    Ls = i_s.search_lists(q, qt, qo, depth=depth)
    i_s.close()
    return La, Ls, gate


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("dim,n,B", [(768, 50_000, 64), (384, 40_001, 33), (768, 9_999, 40), (384, 123_457, 70)])
def test_int8_tier_lists_equal_the_stream_screen(ctxs, O, dim, n, B):
    from openintel_amd import synth
    rows = synth.embeddings_np(n, dim, seed=11 + dim)
    q = synth.embeddings_np(B, dim, seed=12 + B)
    for depth in (10, 1000):
        La, Ls, gate = _both(ctxs, rows, q, depth, base=3)
        assert gate == 0.0, "unit vectors: the int8 tier must hold (no fallback)"
        _same_lists(La, Ls)
        for b in range(0, B, 7):
            _check(La, b, O.dot_scores(rows, q[b]), depth, n, base=3)


@pytest.mark.parametrize("case", ["one_huge_element", "half_steps", "long_rows"])
def test_int8_worst_cases(ctxs, O, case):
    """One element per row far above the rest (the scale is set by it: every other coordinate quantises to a few levels, e_r is
    large); coordinates exactly on half a quantisation step (every rounding a tie); a few rows of norm 50 set aside."""
    from openintel_amd import synth
    n, dim, B, depth = 60_000, 768, 24, 100
    rng = np.random.default_rng(7)
    rows = synth.embeddings_np(n, dim, seed=21)
    q = synth.embeddings_np(B, dim, seed=22)
    if case == "one_huge_element":
        rows[np.arange(n), rng.integers(0, dim, n)] = 0.5
        rows = _unit(rows)
        q = _unit(q + 0.05 * rows[rng.integers(0, n, B)])
    elif case == "half_steps":
        lv = rng.integers(-40, 40, size=(n, dim)).astype(np.float32) + 0.5
        lv[:, 0] = 127.0                                 # absmax 127 steps: step 1, every other coordinate on a half step
        rows = (lv / np.linalg.norm(lv, axis=1, keepdims=True)).astype(np.float32)
        q = _unit(q + rows[rng.integers(0, n, B)])
    else:
        rows[rng.integers(0, n, 5)] *= 50.0
    La, Ls, gate = _both(ctxs, rows, q, depth)
    _same_lists(La, Ls)
    for b in range(0, B, 3):
        _check(La, b, O.dot_scores(rows, q[b]), depth, n)


def test_int8_carry_overflow_opens_the_gate(ctxs, O):
    """20 000 copies of one row close to every query: more keys within the int8 tier's margin than its 16 384-key carry holds --
    the gate opens and the exact pipeline delivers the lists."""
    from openintel_amd import synth
    n, dim, B, depth = 60_000, 768, 16, 100
    rows = synth.embeddings_np(n, dim, seed=31)
    q = synth.embeddings_np(B, dim, seed=32)
    rows[:20_000] = _unit(q[0][None, :] + 0.2 * rows[20_000:20_001])
    a, _ = ctxs
    idx = _index(a, rows)
    qt, qo = np.zeros(B, np.uint32), np.arange(B + 1, dtype=np.uint32)
    L = idx.search_lists(q, qt, qo, depth=depth)
    assert a.profile_read("screen_gate")[0] != 0.0
    for b in (0, 1, 5):
        _check(L, b, O.dot_scores(rows, q[b]), depth, n)
    idx.close()


@pytest.mark.parametrize("spec", [True, False])
def test_speculation_on_and_off(ctxs, spec):
    from openintel_amd import synth
    n, dim, B, depth = 400_000, 768, 64, 1000
    rows = synth.embeddings_np(n, dim, seed=41)
    q = synth.embeddings_np(B, dim, seed=42)
    a, s = ctxs
    a.set_screen_speculation(spec)
    s.set_screen_speculation(spec)
    try:
        La, Ls, gate = _both(ctxs, rows, q, depth)
        assert gate == 0.0
        _same_lists(La, Ls)
    finally:
        a.set_screen_speculation(True)
        s.set_screen_speculation(True)


def test_index_view_returns_the_same_lists(ctxs):
    import openintel_amd as oi
    from openintel_amd import _lib, synth
    n, dim, B, depth = 100_000, 384, 48, 100
    rows = synth.embeddings_np(n, dim, seed=51)
    q = synth.embeddings_np(B, dim, seed=52)
    a, _ = ctxs
    idx = _index(a, rows, base=9)
    qt, qo = np.zeros(B, np.uint32), np.arange(B + 1, dtype=np.uint32)
    L = idx.search_lists(q, qt, qo, depth=depth)
    c2 = oi.HipContext(0)
    c2.set_cosine_mode(_lib.OI_COSINE_SCREEN)
    v = idx.view(c2)
    L2 = v.search_lists(q, qt, qo, depth=depth)
    assert c2.profile_read("screen_gate")[0] == 0.0
    _same_lists(L, L2)
    v.close()
    c2.close()
    idx.close()
