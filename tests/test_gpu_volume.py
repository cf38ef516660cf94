"""Similarity volume (oi_similar_volume): counts[q][b] = documents that pass query q's filter, fall into time
bucket b and have sim(q, d) >= t.  The reference is numpy in this file: an int64 / f64 matmul plus the three clauses of the
definition.  Small-integer corpora make every dot product exact, so both routes (the stream of the bf16 screening copy and the
exact chain) must return the reference bit for bit at every tile, wave and query-group edge; float corpora are built so that
no f64 score lies within the library's 1e-5 of the threshold, and then the counts are the f64 classification exactly -- which
an implementation that counted on screen scores, or dropped the pairs its band buffer cannot hold, does not return."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ALL = (0, 0, 0, 0xFFFFFFFF)
NONE = (0, 0, 7, 6)
TAGS = ("volume", "volume_band", "volume_exact")


def _ctx(mode=None):
    import openintel_amd as oi
    c = oi.HipContext(0)
    if mode is not None:
        c.set_cosine_mode(mode)
    return c


def _index(ctx, rows, group=None, stamp=None, finalize=True, copy=None, bf16=False):
    """finalize=True gives an f32 corpus of dim 384 / 768 its bf16 screening copy (the stream route); copy: a copy policy."""
    import openintel_amd as oi
    n, dim = rows.shape
    idx = oi.HybridIndex(ctx, n, dim, 8)
    if bf16:
        idx.set_embeddings_bf16(rows)
    else:
        idx.set_embeddings(rows, normalize=False)
    if group is not None or stamp is not None:
        idx.set_doc_attrs(group, stamp)
    if copy is not None:
        idx.set_screen_copy(copy)
    if finalize:
        idx.set_forward(np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64))
        idx.finalize()
    return idx


def _ran(ctx, call):
    """(result, the profile tags with at least one launch that did its work) of one call"""
    ctx.profile_reset(True)
    out = call()
    ran = {t for t in TAGS if ctx.profile_read(t)[1] > 0}
    ctx.profile_reset(False)
    return out, ran


def _passes(f, group, stamp):
    m, v, lo, hi = (int(x) for x in f)
    return ((group & np.uint32(m)) == np.uint32(v)) & (stamp >= np.uint32(lo)) & (stamp <= np.uint32(hi))


def _ref(S, t, nb=1, origin=0, width=0, stamp=None, group=None, filters=None):
    """The definition: S [B][n] exact (or f64) similarities -> [B][nb] counts."""
    B, n = S.shape
    with np.errstate(invalid="ignore"):
        hit = S >= t                                    # (a NaN similarity is never >= t)
    if width:
        s64 = stamp.astype(np.int64)
        b = (s64 - origin) // width                     # 64-bit: origin + nb * width may exceed 2^32
        inb = (s64 >= origin) & (b < nb)
    else:
        b, inb = np.zeros(n, np.int64), np.ones(n, bool)
    out = np.zeros((B, nb), np.uint32)
    for q in range(B):
        ok = hit[q] & inb
        if filters is not None:
            ok &= _passes(filters[q], group, stamp)
        out[q] = np.bincount(b[ok], minlength=nb)[:nb]
    return out


def _ints(n, dim, B, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-2, 3, size=(n, dim)).astype(np.float32), rng.integers(-2, 3, size=(B, dim)).astype(np.float32)


def _exact_scores(rows, q):
    return q.astype(np.int64) @ rows.astype(np.int64).T


def _bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def _unit(rng, n, dim):
    x = rng.standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


# ------------------------------------------------------------------ 1. small integers: exact equality on both routes
# n: one row, the 32-row tile's edges, every wave of the 224 x 4 grid with exactly one tile (28 672), one wave with a second
# tile of one row (28 673), three waves with a second tile and a ragged last one (28 773).  B: the 32-query operand tile's and
# the 64-query group's edges.
@pytest.mark.parametrize("dim,n,B", [(384, 1, 1), (384, 31, 32), (768, 32, 33), (768, 33, 64), (384, 28672, 65), (768, 28673, 1),
                                     (768, 28773, 65), (384, 28773, 64), (768, 28672, 32), (384, 33, 65)])
def test_integer_corpus_screen_route_is_exact(dim, n, B):
    ctx = _ctx()
    rows, q = _ints(n, dim, B, seed=n + B)
    idx = _index(ctx, rows)
    S = _exact_scores(rows, q)
    for m in (-3, 20):
        got, ran = _ran(ctx, lambda: idx.similar_volume(q, m + 0.5))
        assert got.dtype == np.uint32 and got.shape == (B, 1)
        assert np.array_equal(got, _ref(S, m + 0.5)), (m, got[:4].ravel(), _ref(S, m + 0.5)[:4].ravel())
        assert "volume" in ran and "volume_exact" not in ran, ran


@pytest.mark.parametrize("kind,dim,n,B", [("f32", 4, 333, 6), ("f32", 20, 8300, 5), ("f32", 1024, 301, 65), ("bf16", 1024, 301, 7),
                                          ("exact_ctx", 768, 1000, 33), ("no_copy", 768, 1000, 64)])
def test_integer_corpus_exact_route_is_exact(kind, dim, n, B):
    from openintel_amd import _lib
    ctx = _ctx(_lib.OI_COSINE_EXACT if kind == "exact_ctx" else None)
    rows, q = _ints(n, dim, B, seed=n + B)
    if kind == "bf16":
        idx = _index(ctx, (rows.view(np.uint32) >> 16).astype(np.uint16), finalize=False, bf16=True)
    elif kind == "no_copy":
        idx = _index(ctx, rows, copy=_lib.OI_SCREEN_COPY_NEVER)
    else:
        idx = _index(ctx, rows, finalize=kind == "exact_ctx")   # (the others: embeddings only, no forward index, no finalize)
    S = _exact_scores(rows, q)
    for m in (-1, 3):
        got, ran = _ran(ctx, lambda: idx.similar_volume(q, m + 0.5))
        assert np.array_equal(got, _ref(S, m + 0.5)), (m, got[:4].ravel())
        assert ran == {"volume_exact"}, ran


def test_bf16_corpus_rounds_the_query_like_its_scorer():
    """rows bf16-exact, queries NOT: sim is the dot product with bf16(q) (round to nearest even), not with q"""
    ctx = _ctx()
    rng = np.random.default_rng(5)
    rows = rng.integers(-2, 3, size=(500, 1024)).astype(np.float32)
    q = (rng.integers(-2, 3, size=(3, 1024)) * (1.0 + 2.0 ** -9) + 2.0 ** -12).astype(np.float32)
    qr = _bf16_round(q)
    assert not np.array_equal(qr, q)
    idx = _index(ctx, (rows.view(np.uint32) >> 16).astype(np.uint16), finalize=False, bf16=True)
    S = qr.astype(np.float64) @ rows.astype(np.float64).T      # exact: small integers times 8-bit significands
    for t in (0.25, 10.25):
        assert np.abs(S - t).min() > 1e-4                        # nothing near the threshold: f32 chain = exact classification
        assert np.array_equal(idx.similar_volume(q, t), _ref(S, t))


# ------------------------------------------------------------------ 2. buckets and filters
def _stamps(n, rng):
    """below the origin, both edges of every bucket of (origin 1000, width 10, up to 1024 buckets), the last bucket's upper
    edge for 1, 2 and 1024 buckets, 0xFFFFFFFF, and the top of the u32 range for the spec whose range passes 2^32"""
    s = [0, 999]
    for b in range(1024):
        s += [1000 + 10 * b, 1000 + 10 * b + 9]
    s += [1010, 1020, 1000 + 10240, 1000 + 10241, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFEFF, 0xFFFFFF00, 0xFFFFFF3F, 0xFFFFFF40,
          0xFFFFFFBF, 0xFFFFFFC0, 0xFFFFFFFE]
    s = np.array(s, dtype=np.uint32)
    rest = rng.integers(900, 1000 + 10300, size=n - s.size).astype(np.uint32)
    return rng.permutation(np.concatenate([s, rest]))


SPECS = [(1000, 10, 1), (1000, 10, 2), (1000, 10, 1024), (0xFFFFFF00, 0x40, 8)]   # (the last: origin + 8 * width > 2^32)


@pytest.mark.parametrize("dim,n", [(384, 28773), (20, 2400)])    # the stream route (second tiles, ragged tile) and the exact route
def test_buckets_and_mixed_filters(dim, n):
    ctx = _ctx()
    rng = np.random.default_rng(11)
    B = 8
    rows, q = _ints(n, dim, B, seed=3)
    stamp = _stamps(n, rng)
    group = rng.integers(0, 1 << 16, size=n).astype(np.uint32)
    idx = _index(ctx, rows, group, stamp, finalize=dim == 384)
    S = _exact_scores(rows, q)
    F = np.array([ALL, (3, 1, 0, 0xFFFFFFFF), (0, 0, 1005, 1014), NONE, (0xF, 2, 1500, 0xFFFFFFFF), ALL, (0, 0, 0xFFFFFF10, 0xFFFFFFFE),
                  (1, 0, 0, 5000)], dtype=np.uint32)
    t = -10.5 if dim == 384 else -2.5
    for origin, width, nb in SPECS:
        for f in (None, F):
            got, ran = _ran(ctx, lambda: idx.similar_volume(q, t, n_buckets=nb, stamp_origin=origin, bucket_width=width, filters=f))
            ref = _ref(S, t, nb, origin, width, stamp, group, f)
            assert got.shape == (B, nb) and np.array_equal(got, ref), (origin, width, nb, f is None, int(got.sum()), int(ref.sum()))
            assert ("volume" in ran) == (dim == 384) and ("volume_exact" in ran) == (dim != 384), ran
        assert ref.sum() > 0 and ref[3].sum() == 0
    # filters without a time axis
    assert np.array_equal(idx.similar_volume(q, t, filters=F), _ref(S, t, stamp=stamp, group=group, filters=F))


@pytest.mark.parametrize("dim", [384, 20])
def test_an_index_without_attributes(dim):
    from openintel_amd import _lib
    ctx = _ctx()
    rows, q = _ints(100, dim, 2, seed=4)
    idx = _index(ctx, rows, finalize=dim == 384)
    assert np.array_equal(idx.similar_volume(q, 0.5), _ref(_exact_scores(rows, q), 0.5))    # bucket_width == 0 works
    with pytest.raises(_lib.OiError) as e:
        idx.similar_volume(q, 0.5, n_buckets=2, stamp_origin=0, bucket_width=5)
    assert e.value.code == _lib.OI_ERR_STATE
    with pytest.raises(_lib.OiError) as e:
        idx.similar_volume(q, 0.5, filters=np.array([ALL, ALL], dtype=np.uint32))
    assert e.value.code == _lib.OI_ERR_STATE


# ------------------------------------------------------------------ 3. the band must be rescored
def _planted(dim, n=28773, B=64, t=0.5, seed=7):
    """random unit rows and queries; per query 40 rows a q + sqrt(1 - a^2) u, u orthogonal to q, with a - t on 32 even steps
    over +-3e-3 and at +-5e-5, +-1e-4, +-2e-4, +-1e-3"""
    rng = np.random.default_rng(seed + dim)
    rows, q = _unit(rng, n, dim), _unit(rng, B, dim)
    offs = np.concatenate([np.linspace(-3e-3, 3e-3, 32), [5e-5, -5e-5, 1e-4, -1e-4, 2e-4, -2e-4, 1e-3, -1e-3]])
    where = rng.permutation(n)[:B * offs.size].reshape(B, offs.size)
    for b in range(B):
        u = rng.standard_normal((offs.size, dim))
        u -= np.outer(u @ q[b], q[b])
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        a = t + offs
        rows[where[b]] = a[:, None] * q[b] + np.sqrt(1.0 - a * a)[:, None] * u
    return rows.astype(np.float32), q.astype(np.float32)


@pytest.mark.parametrize("dim", [384, 768])
def test_the_band_is_rescored_not_counted_on_screen_scores(dim):
    t = 0.5
    rows, q = _planted(dim, t=t)
    S = q.astype(np.float64) @ rows.astype(np.float64).T
    # the test's own preconditions: nothing the f32 chain could put on the other side, and a screen that would
    assert np.abs(S - t).min() > 2e-5
    Sb = _bf16_round(q).astype(np.float64) @ _bf16_round(rows).astype(np.float64).T
    wrong = int(((Sb >= t) != (S >= t)).sum())
    assert wrong >= 20, wrong
    ctx = _ctx()
    idx = _index(ctx, rows)
    got, ran = _ran(ctx, lambda: idx.similar_volume(q, t))
    ref = _ref(S, t)
    print("planted d=%d: bf16-misclassified %d, hits %d, library %d" % (dim, wrong, int(ref.sum()), int(got.sum())))
    assert np.array_equal(got, ref), np.flatnonzero(got.ravel() != ref.ravel())[:8]
    assert "volume" in ran and "volume_band" in ran and "volume_exact" not in ran, ran


# ------------------------------------------------------------------ 4. long rows
def test_long_rows_are_counted_by_the_band_kernel():
    dim, n, B, t = 384, 28773, 64, 0.5
    rng = np.random.default_rng(21)
    rows, q = _unit(rng, n, dim), _unit(rng, B, dim)
    long_at = np.array([0, 31, 4097, 20000, 28671, 28772])
    for i, r in enumerate(long_at):   # norm 50; against query 0 the scores 50 a sit on either side of t, against the others wherever
        a = (0.02, 0.005, 0.0104, 0.0096, -0.02, 0.011)[i]
        u = rng.standard_normal(dim)
        u -= (u @ q[0]) * q[0]
        rows[r] = 50.0 * (a * q[0] + np.sqrt(1 - a * a) * u / np.linalg.norm(u))
    rows, q = rows.astype(np.float32), q.astype(np.float32)
    S = q.astype(np.float64) @ rows.astype(np.float64).T
    is_long = np.zeros(n, bool)
    is_long[long_at] = True
    assert np.abs(S[:, is_long] - t).min() > 1e-3 and np.abs(S[:, ~is_long] - t).min() > 2e-5   # (f32 chain error scales with the norm)
    assert (S[:, is_long] >= t).any() and (S[:, is_long] < t).any()
    ctx = _ctx()
    stamp = (np.arange(n) % 3).astype(np.uint32)
    idx = _index(ctx, rows, None, stamp)
    assert idx.long_rows() == long_at.size
    eps = idx.screen_probe(q)[1]
    assert eps.max() < 0.02, eps.max()                      # the margin is the unit rows': 50 times that with the long rows in it
    F = np.array([ALL if b % 2 == 0 else (0, 0, 1, 2) for b in range(B)], dtype=np.uint32)
    for kw in ({}, dict(n_buckets=3, stamp_origin=0, bucket_width=1, filters=F)):
        got, ran = _ran(ctx, lambda: idx.similar_volume(q, t, **kw))
        ref = _ref(S, t, kw.get("n_buckets", 1), 0, kw.get("bucket_width", 0), stamp, np.zeros(n, np.uint32), kw.get("filters"))
        assert np.array_equal(got, ref), np.flatnonzero(got.ravel() != ref.ravel())[:8]
        assert "volume" in ran and "volume_band" in ran and "volume_exact" not in ran, ran


# ------------------------------------------------------------------ 5. band overflow falls back inside the call
def test_band_overflow_falls_back_inside_the_call():
    dim, n, B = 384, 65632, 64                                   # 64 x 65 632 = 4 200 448 pairs in the band; it holds 4 Mi
    rows = np.zeros((n, dim), np.float32)
    rows[:, 0] = 0.5
    rows[:, 1] = (np.arange(n) % 97) / 256.0                     # bf16-exact: screen score = sim = 0.5 exactly
    q = np.zeros((B, dim), np.float32)
    q[:, 0] = 1.0
    assert B * n > 4 << 20
    ctx = _ctx()
    idx = _index(ctx, rows)
    got, ran = _ran(ctx, lambda: idx.similar_volume(q, 0.5))
    assert np.array_equal(got, np.full((B, 1), n, np.uint32)), (got.min(), got.max())
    assert "volume_exact" in ran, ran
    got, ran = _ran(ctx, lambda: idx.similar_volume(q, 0.75))     # the flags of the first call are gone
    assert not got.any() and "volume" in ran and "volume_exact" not in ran, (int(got.sum()), ran)
    got, ran = _ran(ctx, lambda: idx.similar_volume(q, 0.25))     # proven hits only
    assert np.array_equal(got, np.full((B, 1), n, np.uint32)) and "volume_exact" not in ran, (got.min(), got.max(), ran)


# ------------------------------------------------------------------ 6, 7, 9: one float corpus
class _Float:
    pass


@pytest.fixture(scope="module")
def fl():
    from openintel_amd import _lib
    f = _Float()
    f.dim, f.n, f.B = 768, 28773, 64
    rng = np.random.default_rng(33)
    f.rows, f.q = _unit(rng, f.n, f.dim).astype(np.float32), _unit(rng, f.B, f.dim).astype(np.float32)
    f.stamp = rng.integers(0, 4, size=f.n).astype(np.uint32)
    f.S = f.q.astype(np.float64) @ f.rows.astype(np.float64).T
    f.ctx = _ctx()
    f.idx = _index(f.ctx, f.rows, None, f.stamp)
    f.ctx_exact = _ctx(_lib.OI_COSINE_EXACT)
    f.view_exact = f.idx.view(f.ctx_exact)
    return f


@pytest.mark.parametrize("t", [0.05, 0.1])
def test_routes_agree_bit_for_bit_on_float_data(fl, t):
    from openintel_amd import _lib
    kw = dict(n_buckets=4, stamp_origin=0, bucket_width=1)
    a, ran_a = _ran(fl.ctx, lambda: fl.idx.similar_volume(fl.q, t, **kw))
    b, ran_b = _ran(fl.ctx_exact, lambda: fl.view_exact.similar_volume(fl.q, t, **kw))
    ctx_c = _ctx()
    bare = _index(ctx_c, fl.rows, None, fl.stamp, copy=_lib.OI_SCREEN_COPY_NEVER)
    c, ran_c = _ran(ctx_c, lambda: bare.similar_volume(fl.q, t, **kw))
    assert "volume" in ran_a and "volume_exact" not in ran_a and ran_b == {"volume_exact"} and ran_c == {"volume_exact"}, (ran_a, ran_b, ran_c)
    assert np.array_equal(a, b) and np.array_equal(a, c)
    hi = _ref(fl.S, t - 1e-5, 4, 0, 1, fl.stamp).astype(np.int64)
    lo = _ref(fl.S, t + 1e-5, 4, 0, 1, fl.stamp).astype(np.int64)
    print("t=%g: f64 counts %d .. %d, library %d" % (t, lo.sum(), hi.sum(), a.sum()))
    assert (hi - lo).sum() <= 0.005 * lo.sum(), ((hi - lo).sum(), lo.sum())     # what the two-sided bar can hide
    assert (lo <= a).all() and (a <= hi).all()


@pytest.mark.parametrize("k", [1, 100])
def test_volume_at_the_kth_score_counts_the_list(fl, k):
    qt, qo = np.zeros(1, np.uint32), np.zeros(fl.B + 1, np.uint32)
    L = fl.idx.search_lists(fl.q, qt, qo, depth=k + 1)
    for b in (0, 17, 63):
        s = L.cos_scores[b]
        assert int(L.cos_counts[b]) == k + 1 and (s[:k] > s[k:k + 1]).all() and s[k - 1] > s[k]     # distinct around the cut
        t = float(s[k - 1])
        assert int(fl.idx.similar_volume(fl.q, t)[b].sum()) == k == int((s >= t).sum())
        assert int(fl.idx.similar_volume(fl.q[b:b + 1], t).sum()) == k


def test_device_buffers_streams_views_and_repeats(fl):
    import torch
    t, kw = 0.1, dict(n_buckets=4, stamp_origin=0, bucket_width=1)
    want = fl.idx.similar_volume(fl.q, t, **kw)
    assert np.array_equal(fl.idx.similar_volume(fl.q, t, **kw), want)             # twice: histogram and band counter start over
    assert fl.idx.similar_volume(fl.q[:0], t, **kw).shape == (0, 4)               # n_queries == 0
    ctx2 = _ctx()
    st = torch.cuda.Stream()
    ctx2.set_stream(st)
    v = fl.idx.view(ctx2)
    with torch.cuda.stream(st):
        dq = torch.from_numpy(fl.q).cuda()
        F = np.array([ALL if b % 3 else (0, 0, 1, 2) for b in range(fl.B)], dtype=np.uint32)
        o1 = v.similar_volume(dq, t, **kw)
        o2 = v.similar_volume(dq, t, filters=F, **kw)
        o3 = v.similar_volume(dq[:33], t, **kw)
    st.synchronize()
    assert o1.is_cuda and tuple(o1.shape) == (fl.B, 4)
    assert np.array_equal(o1.cpu().numpy().view(np.uint32), want)
    assert np.array_equal(o3.cpu().numpy().view(np.uint32), want[:33])
    assert np.array_equal(o2.cpu().numpy().view(np.uint32), fl.idx.similar_volume(fl.q, t, filters=F, **kw))
    dev, _ = ctx2.workspace_bytes()
    assert dev >= (32 << 20) + fl.B * 4 * 4                                       # the band buffer and the histogram are counted
    v.close() if hasattr(v, "close") else None


# ------------------------------------------------------------------ 8. odd values
def test_infinite_thresholds_nan_rows_and_queries_without_a_bound(fl):
    n, B = fl.n, fl.B
    F = np.array([ALL if b % 2 == 0 else (0, 0, 1, 2) for b in range(B)], dtype=np.uint32)
    passing = np.array([n if b % 2 == 0 else int(((fl.stamp >= 1) & (fl.stamp <= 2)).sum()) for b in range(B)], np.uint32)
    got, ran = _ran(fl.ctx, lambda: fl.idx.similar_volume(fl.q, float("-inf"), filters=F))
    assert np.array_equal(got.ravel(), passing) and "volume_exact" not in ran, ran
    assert not fl.idx.similar_volume(fl.q, float("inf")).any()
    assert not fl.view_exact.similar_volume(fl.q, float("inf")).any()
    # a query without a bound sends the batch through the exact route; the others' counts do not move
    want = fl.idx.similar_volume(fl.q, 0.1)
    for bad in (float("nan"), 1e30):
        q = fl.q.copy()
        q[5, 3] = bad
        got, ran = _ran(fl.ctx, lambda: fl.idx.similar_volume(q, 0.1))
        assert "volume_exact" in ran, ran
        keep = np.arange(B) != 5
        assert np.array_equal(got[keep], want[keep])
        if bad != bad:
            assert got[5, 0] == 0                                                  # every similarity is NaN
    # a NaN row is never counted, at any threshold (such a corpus is never screened)
    rows = fl.rows[:300].copy()
    rows[7, 100] = np.nan
    ctx = _ctx()
    idx = _index(ctx, rows)
    got, ran = _ran(ctx, lambda: idx.similar_volume(fl.q, float("-inf")))
    assert np.array_equal(got, np.full((B, 1), 299, np.uint32)) and ran == {"volume_exact"}, (got.ravel()[:4], ran)
    S = fl.S[:, :300].copy()
    S[:, 7] = np.nan
    assert np.array_equal(idx.similar_volume(fl.q, 0.05), _ref(S, 0.05))
