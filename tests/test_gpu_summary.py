"""Similarity summary (oi_index_set_signals + oi_similar_summary): out[q][b] = the social_summary raw sums over
the documents that pass query q's filter, fall into time bucket b and have sim(q, d) >= t_q.  The reference is numpy in this
file: an exact (int64) or f64 similarity matrix, the three clauses of the definition, integer counts per cell and
float(int(sum of rint(v * 2^30))) * 2^-30 for the polarity sum.  All eight fields are compared bit for bit.  The corpora are
those of tests/test_gpu_volume.py: small integers make every dot product exact on both routes; float corpora keep every f64
score further than the library's 1e-5 from the threshold."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ALL = (0, 0, 0, 0xFFFFFFFF)
NONE = (0, 0, 7, 6)
TAGS = ("summary", "summary_band", "summary_exact")
TAU = 0.2
INF = float("inf")
# 0.2 is NOT bullish (v > tau), NaN -> 0, 1.5 -> 1, -7 -> -1; 1/3 and 0.2 are not dyadic: their records round
VALS = np.array([-1.0, -0.5, -1.0 / 3.0, -0.2, 0.0, 0.2, 0.25, 1.0 / 3.0, 1.0, np.nan, 1.5, -7.0])


def _dtype():
    from openintel_amd.analyzer import COUNTERS_DTYPE
    return COUNTERS_DTYPE


def _ctx(mode=None):
    import openintel_amd as oi
    c = oi.HipContext(0)
    if mode is not None:
        c.set_cosine_mode(mode)
    return c


class _Sig:
    """per-document signals as the caller gives them, and what the definition makes of them"""

    def __init__(self, pol, spec, src):
        self.pol, self.spec, self.src = pol, spec, src
        v = np.where(np.isnan(pol), 0.0, np.clip(pol, -1.0, 1.0))
        self.q30 = np.rint(v * 2.0 ** 30).astype(np.int64)          # (numpy's rint: round half to even, like the kernel's)
        self.bull, self.bear = v > TAU, v < -TAU
        self.neu = ~self.bull & ~self.bear
        self.sp = spec != 0
        self.s1 = (src != 0) if src is not None else np.zeros(pol.size, bool)

    def without_sources(self):
        return _Sig(self.pol, self.spec, None)


def _signals(n, seed, vals=VALS):
    rng = np.random.default_rng(1000 + seed)
    return _Sig(vals[rng.integers(0, vals.size, size=n)], rng.integers(0, 2, size=n).astype(np.uint8),
                rng.integers(0, 2, size=n).astype(np.uint8))


def _index(ctx, rows, sig=None, group=None, stamp=None, finalize=True, copy=None, bf16=False):
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
    if sig is not None:
        idx.set_signals(sig.pol, sig.spec, sig.src, TAU)
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


def _ref(S, t, sig, nb=1, origin=0, width=0, stamp=None, group=None, filters=None):
    """The definition: S [B][n] exact (or f64) similarities, t a threshold or one per query -> [B][nb] records."""
    B, n = S.shape
    tq = np.broadcast_to(np.asarray(t, dtype=np.float64), (B,))
    with np.errstate(invalid="ignore"):
        hit = S >= tq[:, None]                          # (a NaN similarity, or a NaN threshold, is never a hit)
    if width:
        s64 = stamp.astype(np.int64)
        b = (s64 - origin) // width                     # 64-bit: origin + nb * width may exceed 2^32
        inb = (s64 >= origin) & (b < nb)
    else:
        b, inb = np.zeros(n, np.int64), np.ones(n, bool)
    out = np.zeros((B, nb), _dtype())

    def count(m):
        return np.bincount(b[m], minlength=nb)[:nb]

    for q in range(B):
        ok = hit[q] & inb
        if filters is not None:
            ok &= _passes(filters[q], group, stamp)
        out["total"][q] = count(ok)
        out["by_source"][q, :, 1] = count(ok & sig.s1)
        out["by_source"][q, :, 0] = out["total"][q] - out["by_source"][q, :, 1]
        out["bullish"][q], out["bearish"][q], out["neutral"][q] = count(ok & sig.bull), count(ok & sig.bear), count(ok & sig.neu)
        out["spec_count"][q] = count(ok & sig.sp)
        s = np.zeros(nb, np.int64)
        np.add.at(s, b[ok], sig.q30[ok])
        out["polarity_sum"][q] = [float(int(x)) * 2.0 ** -30 for x in s]
    return out


def _host(x):
    """a result as a numpy record array [B][nb], wherever it lives"""
    if hasattr(x, "data_ptr"):
        B, nb = int(x.shape[0]), int(x.shape[1])
        return x.cpu().numpy().view(_dtype()).reshape(B, nb)
    return x


def _same(got, ref):
    """all eight fields bit for bit (the f64 sum included: compared as its 64 bits)"""
    got = _host(got)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    a, b = got.view(np.uint64).reshape(-1, 8), ref.view(np.uint64).reshape(-1, 8)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, (bad[:4], got.reshape(-1)[bad[:2]], ref.reshape(-1)[bad[:2]])


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


# ------------------------------------------------------------------ 1. the stream route on integer corpora
# the volume tests' tile, wave, grid and query-group edges (tests/test_gpu_volume.py)
@pytest.mark.parametrize("dim,n,B", [(384, 1, 1), (384, 31, 32), (768, 32, 33), (768, 33, 64), (384, 28672, 65), (768, 28673, 1),
                                     (768, 28773, 65), (384, 33, 65)])
def test_integer_corpus_screen_route_is_exact(dim, n, B):
    ctx = _ctx()
    rows, q = _ints(n, dim, B, seed=n + B)
    sig = _signals(n, n + B)
    idx = _index(ctx, rows, sig)
    S = _exact_scores(rows, q)
    for m in (-3, 20):
        got, ran = _ran(ctx, lambda: idx.similar_summary(q, m + 0.5))
        _same(got, _ref(S, m + 0.5, sig))
        assert "summary" in ran and "summary_exact" not in ran, ran
    idx.set_signals(sig.pol, sig.spec, None, TAU)            # sources = NULL: all reddit (and an overwrite in place)
    ref = _ref(S, -2.5, sig.without_sources())
    _same(idx.similar_summary(q, -2.5), ref)
    assert not ref["by_source"][:, :, 1].any() and (n < 31 or ref["total"].sum() > 0)


# ------------------------------------------------------------------ 2. the exact route
@pytest.mark.parametrize("kind,dim,n,B", [("f32", 4, 333, 6), ("f32", 20, 8300, 5), ("f32", 1024, 301, 65), ("bf16", 1024, 301, 7),
                                          ("exact_ctx", 768, 1000, 33), ("no_copy", 768, 1000, 64)])
def test_integer_corpus_exact_route_is_exact(kind, dim, n, B):
    from openintel_amd import _lib
    ctx = _ctx(_lib.OI_COSINE_EXACT if kind == "exact_ctx" else None)
    rows, q = _ints(n, dim, B, seed=n + B)
    sig = _signals(n, n + B)
    if kind == "bf16":
        idx = _index(ctx, (rows.view(np.uint32) >> 16).astype(np.uint16), sig, finalize=False, bf16=True)
    elif kind == "no_copy":
        idx = _index(ctx, rows, sig, copy=_lib.OI_SCREEN_COPY_NEVER)
    else:
        idx = _index(ctx, rows, sig, finalize=kind == "exact_ctx")   # (the others: embeddings only, no forward index, no finalize)
    S = _exact_scores(rows, q)
    for m in (-1, 3):
        got, ran = _ran(ctx, lambda: idx.similar_summary(q, m + 0.5))
        _same(got, _ref(S, m + 0.5, sig))
        assert ran == {"summary_exact"}, ran
    idx.set_signals(sig.pol, sig.spec, None, TAU)
    _same(idx.similar_summary(q, -0.5), _ref(S, -0.5, sig.without_sources()))


# ------------------------------------------------------------------ 3. buckets and filters mixed
def _stamps(n, rng):
    """the stamp set of the volume test: below the origin, both edges of every bucket of (origin 1000, width 10, up to 1024
    buckets), the last bucket's upper edge for 1, 2 and 1024 buckets, 0xFFFFFFFF, and the top of the u32 range"""
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
    sig = _signals(n, 3)
    idx = _index(ctx, rows, sig, group, stamp, finalize=dim == 384)
    S = _exact_scores(rows, q)
    F = np.array([ALL, (3, 1, 0, 0xFFFFFFFF), (0, 0, 1005, 1014), NONE, (0xF, 2, 1500, 0xFFFFFFFF), ALL, (0, 0, 0xFFFFFF10, 0xFFFFFFFE),
                  (1, 0, 0, 5000)], dtype=np.uint32)
    t = -10.5 if dim == 384 else -2.5
    for origin, width, nb in SPECS:
        for f in (None, F):
            got, ran = _ran(ctx, lambda: idx.similar_summary(q, t, n_buckets=nb, stamp_origin=origin, bucket_width=width, filters=f))
            ref = _ref(S, t, sig, nb, origin, width, stamp, group, f)
            _same(got, ref)
            assert ("summary" in ran) == (dim == 384) and ("summary_exact" in ran) == (dim != 384), ran
        assert ref["total"].sum() > 0 and ref["total"][3].sum() == 0
    _same(idx.similar_summary(q, t, filters=F), _ref(S, t, sig, stamp=stamp, group=group, filters=F))   # filters without a time axis


# ------------------------------------------------------------------ 4. per-query thresholds
@pytest.mark.parametrize("dim", [384, 20])                        # the stream route and the exact route
def test_per_query_thresholds_equal_single_query_calls(dim):
    import torch
    ctx = _ctx()
    n, B = 2000, 65
    rows, q = _ints(n, dim, B, seed=44)
    sig = _signals(n, 44)
    idx = _index(ctx, rows, sig, finalize=dim == 384)
    choices = np.array([-INF, -3.5, 0.5, 20.5 if dim == 384 else 2.5, INF, np.nan], dtype=np.float32)
    thr = choices[np.random.default_rng(4).integers(0, choices.size, size=B)]
    thr[:choices.size] = choices                                   # (every one of them is there)
    got, ran = _ran(ctx, lambda: idx.similar_summary(q, thr))
    assert ("summary" in ran) == (dim == 384) and ("summary_exact" in ran) == (dim != 384), ran
    _same(got, _ref(_exact_scores(rows, q), thr, sig))
    for b in range(B):
        if np.isnan(thr[b]):
            assert got[b].tobytes() == bytes(64)                   # a NaN threshold counts nothing: all eight fields zero
        else:
            _same(idx.similar_summary(q[b:b + 1], float(thr[b])), got[b:b + 1])
    assert got["total"][~np.isnan(thr) & (thr < 0)].min() > 0
    # thresholds in HBM, with the queries
    dq = torch.from_numpy(q).cuda()
    _same(idx.similar_summary(dq, torch.from_numpy(thr).cuda()), got)
    _same(idx.similar_summary(dq, thr), got)                       # (a host array beside device queries is moved for the caller)
    ctx.synchronize()


# ------------------------------------------------------------------ 5. the band is rescored
def _planted(dim, n=28773, B=64, t=0.5, seed=7):
    """the planted corpus of the volume test (same generator, same seeds): per query 40 rows a q + sqrt(1 - a^2) u, u
    orthogonal to q, with a - t on 32 even steps over +-3e-3 and at +-5e-5, +-1e-4, +-2e-4, +-1e-3"""
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
def test_the_band_is_rescored_not_summed_on_screen_scores(dim):
    t = 0.5
    rows, q = _planted(dim, t=t)
    S = q.astype(np.float64) @ rows.astype(np.float64).T
    # the test's own preconditions: nothing the f32 chain could put on the other side, and a screen that would
    assert np.abs(S - t).min() > 2e-5
    Sb = _bf16_round(q).astype(np.float64) @ _bf16_round(rows).astype(np.float64).T
    wrong = int(((Sb >= t) != (S >= t)).sum())
    assert wrong >= 20, wrong
    ctx = _ctx()
    sig = _signals(rows.shape[0], dim)
    idx = _index(ctx, rows, sig)
    got, ran = _ran(ctx, lambda: idx.similar_summary(q, t))
    ref = _ref(S, t, sig)
    print("planted d=%d: bf16-misclassified %d, hits %d, library %d" % (dim, wrong, int(ref["total"].sum()), int(got["total"].sum())))
    _same(got, ref)
    assert "summary" in ran and "summary_band" in ran and "summary_exact" not in ran, ran


# ------------------------------------------------------------------ 6. long rows
def test_long_rows_are_summed_by_the_band_kernel():
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
    sig = _signals(n, 21)
    sig.pol[long_at] = (1.0, -1.0 / 3.0, 0.25, -0.5, 1.0 / 3.0, -1.0)   # a long row's record is never a zero
    sig = _Sig(sig.pol, sig.spec, sig.src)
    idx = _index(ctx, rows, sig, None, stamp)
    assert idx.long_rows() == long_at.size
    F = np.array([ALL if b % 2 == 0 else (0, 0, 1, 2) for b in range(B)], dtype=np.uint32)
    for kw in ({}, dict(n_buckets=3, stamp_origin=0, bucket_width=1, filters=F)):
        got, ran = _ran(ctx, lambda: idx.similar_summary(q, t, **kw))
        ref = _ref(S, t, sig, kw.get("n_buckets", 1), 0, kw.get("bucket_width", 0), stamp, np.zeros(n, np.uint32), kw.get("filters"))
        _same(got, ref)
        assert "summary" in ran and "summary_band" in ran and "summary_exact" not in ran, ran


# ------------------------------------------------------------------ 7. band overflow falls back inside the call
def test_band_overflow_falls_back_inside_the_call():
    dim, n, B = 384, 65632, 64                                   # 64 x 65 632 = 4 200 448 pairs in the band; it holds 4 Mi
    rows = np.zeros((n, dim), np.float32)
    rows[:, 0] = 0.5
    rows[:, 1] = (np.arange(n) % 97) / 256.0                     # bf16-exact: screen score = sim = 0.5 exactly
    q = np.zeros((B, dim), np.float32)
    q[:, 0] = 1.0
    assert B * n > 4 << 20
    sig = _signals(n, 7, vals=np.array([-1.0, -1.0 / 3.0, -0.2, 0.0, 0.25]))
    S = np.full((B, n), 0.5)
    full = _ref(S, 0.5, sig)
    assert full["polarity_sum"].max() < -1000.0                   # per-cell sums are NEGATIVE: a stale i64 of the abandoned
    ctx = _ctx()                                                  # stream (only its high word, say) would show
    idx = _index(ctx, rows, sig)
    got, ran = _ran(ctx, lambda: idx.similar_summary(q, 0.5))
    _same(got, full)
    assert "summary_exact" in ran, ran
    got, ran = _ran(ctx, lambda: idx.similar_summary(q, 0.75))    # the flags of the first call are gone
    assert got.tobytes() == bytes(64 * B) and "summary" in ran and "summary_exact" not in ran, (int(got["total"].sum()), ran)
    got, ran = _ran(ctx, lambda: idx.similar_summary(q, 0.25))    # proven hits only
    _same(got, full)
    assert "summary_exact" not in ran, ran


# ------------------------------------------------------------------ 8. the sum is an integer sum
def test_the_polarity_sum_is_deterministic():
    dim, n = 384, 28773
    rows, q = _ints(n, dim, 1, seed=8)
    rng = np.random.default_rng(8)
    pol = np.array([1.0 / 3.0, -1.0 / 3.0, 0.2, -0.2, 1.0, 0.0])[rng.integers(0, 6, size=n)]
    stamp = (np.arange(n) % 2).astype(np.uint32)
    # bucket 1: k rows of +1/3, k rows of -1/3 and one of -0.2, shuffled over the grid: whatever order the atomics take, the
    # running sum is above zero at some point and below it at the end
    odd = np.flatnonzero(stamp == 1)
    k = (odd.size - 1) // 2
    pol[odd] = rng.permutation(np.concatenate([np.full(k, 1.0 / 3.0), np.full(odd.size - 1 - k, -1.0 / 3.0), [-0.2]]))
    sig = _Sig(pol, rng.integers(0, 2, size=n).astype(np.uint8), rng.integers(0, 2, size=n).astype(np.uint8))
    ctx = _ctx()
    idx = _index(ctx, rows, sig, None, stamp)
    S = _exact_scores(rows, q)
    for kw in (dict(), dict(n_buckets=2, stamp_origin=0, bucket_width=1)):      # everything in ONE cell; then the two buckets
        ref = _ref(S, -INF, sig, kw.get("n_buckets", 1), 0, kw.get("bucket_width", 0), stamp)
        a, ran = _ran(ctx, lambda: idx.similar_summary(q, -INF, **kw))
        b = idx.similar_summary(q, -INF, **kw)
        assert "summary" in ran and "summary_exact" not in ran, ran
        _same(a, ref)
        _same(b, a)
        assert int(ref["total"].sum()) == n
    cell = ref["polarity_sum"][0, 1]
    want = (int(np.rint(2.0 ** 30 / 3.0)) * k + int(np.rint(-2.0 ** 30 / 3.0)) * (odd.size - 1 - k) + int(np.rint(-0.2 * 2.0 ** 30))) * 2.0 ** -30
    assert cell == want and cell < 0.0
    assert cell * 2.0 ** 30 == np.rint(cell * 2.0 ** 30)                        # an integer multiple of 2^-30
    exact = float(np.sum(np.clip(pol[odd], -1, 1)))
    assert abs(cell - exact) <= odd.size * 2.0 ** -31 + 1e-12                    # the header's bound (the f64 sum's own error aside)


# ------------------------------------------------------------------ 9. routes agree, and total is the volume
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
    f.sig = _signals(f.n, 33)
    f.ctx = _ctx()
    f.idx = _index(f.ctx, f.rows, f.sig, None, f.stamp)
    f.ctx_exact = _ctx(_lib.OI_COSINE_EXACT)
    f.view_exact = f.idx.view(f.ctx_exact)
    return f


INT_FIELDS = ("total", "by_source", "bullish", "bearish", "neutral", "spec_count")


@pytest.mark.parametrize("t", [0.05, 0.1])
def test_routes_agree_bit_for_bit_and_total_is_the_volume(fl, t):
    from openintel_amd import _lib
    kw = dict(n_buckets=4, stamp_origin=0, bucket_width=1)
    a, ran_a = _ran(fl.ctx, lambda: fl.idx.similar_summary(fl.q, t, **kw))
    b, ran_b = _ran(fl.ctx_exact, lambda: fl.view_exact.similar_summary(fl.q, t, **kw))
    ctx_c = _ctx()
    bare = _index(ctx_c, fl.rows, fl.sig, None, fl.stamp, copy=_lib.OI_SCREEN_COPY_NEVER)
    c, ran_c = _ran(ctx_c, lambda: bare.similar_summary(fl.q, t, **kw))
    assert "summary" in ran_a and "summary_exact" not in ran_a and ran_b == {"summary_exact"} and ran_c == {"summary_exact"}, (ran_a, ran_b, ran_c)
    _same(b, a)
    _same(c, a)
    vol = fl.idx.similar_volume(fl.q, t, **kw)
    assert np.array_equal(a["total"], vol.astype(np.uint64))
    hi = _ref(fl.S, t - 1e-5, fl.sig, 4, 0, 1, fl.stamp)
    lo = _ref(fl.S, t + 1e-5, fl.sig, 4, 0, 1, fl.stamp)
    hidden = int((hi["total"] - lo["total"]).sum())
    print("t=%g: f64 totals %d .. %d, library %d" % (t, lo["total"].sum(), hi["total"].sum(), a["total"].sum()))
    assert hidden <= 0.005 * int(lo["total"].sum()), (hidden, int(lo["total"].sum()))     # what the two-sided bar can hide
    for f in INT_FIELDS:                                                                   # (hits at t + 1e-5 are hits at t - 1e-5)
        assert (lo[f] <= a[f]).all() and (a[f] <= hi[f]).all(), f


# ------------------------------------------------------------------ 10. the reference's own numbers
@pytest.mark.parametrize("dim", [4, 384])                          # the exact route; a finalized index on the stream route
def test_the_reference_fixture_summary(dim):
    from openintel_amd.engine import SpeculationEngine
    here = os.path.dirname(os.path.abspath(__file__))
    golden = json.load(open(os.path.join(here, "golden", "reference_fixture.json")))
    posts = golden["fixture_posts"]
    texts = [p["text"] for p in posts]
    sources = np.array([0 if p["source"] == "reddit" else 1 for p in posts], np.uint8)
    rng = np.random.default_rng(10)
    rows = _unit(rng, len(posts), dim).astype(np.float32)
    q = _unit(rng, 1, dim).astype(np.float32)
    ctx = _ctx()
    idx = _index(ctx, rows, finalize=dim == 384)
    idx.set_signals_from_text(texts, sources, TAU)
    got, ran = _ran(ctx, lambda: idx.similar_summary(q, -INF))
    assert ("summary" in ran and "summary_exact" not in ran) if dim == 384 else ran == {"summary_exact"}, ran
    s = SpeculationEngine.social_from_counters(got[0, 0])
    want = golden["derived"]["summary"]
    assert s.total_mentions == want["total_mentions"] == 10
    assert {k.as_str(): v for k, v in s.mentions_by_source.items()} == want["mentions_by_source"] == {"reddit": 4, "bluesky": 6}
    assert (s.bullish, s.bearish, s.neutral) == (want["bullish"], want["bearish"], want["neutral"]) == (7, 2, 1)
    assert float(s.net_sentiment) == want["net_sentiment"] == 0.5
    assert float(s.speculation_index) == want["speculation_index"] == 0.3
    assert s.bull_bear_ratio == want["bull_bear_ratio"] == 3.5
    assert got["polarity_sum"][0, 0] == 5.0                          # all of {-1, 0, 1}: the sum is exact


def test_everything_hit_equals_oi_social_summary():
    from openintel_amd.domain import EngineConfig
    from openintel_amd.engine import SpeculationEngine
    n, dim = 5000, 20
    ctx = _ctx()
    rows, q = _ints(n, dim, 1, seed=12)
    sig = _signals(n, 12, vals=np.array([-1.0, -0.5, -1.0 / 3.0, -0.2, 0.0, 0.2, 0.25, 1.0 / 3.0, 1.0]))
    idx = _index(ctx, rows, sig, finalize=False)
    got = idx.similar_summary(q, -INF)[0, 0]
    c = SpeculationEngine.social_counters(ctx, sig.src, sig.pol, sig.spec, EngineConfig())
    assert EngineConfig().bull_bear_threshold == TAU
    assert (int(got["total"]), int(got["bullish"]), int(got["bearish"]), int(got["neutral"]), int(got["spec_count"])) == \
        (c.total, c.bullish, c.bearish, c.neutral, c.spec_count) and c.total == n
    assert [int(x) for x in got["by_source"]] == [c.by_source[0], c.by_source[1]]
    assert abs(float(got["polarity_sum"]) - c.polarity_sum) <= n * 2.0 ** -31 + 1e-9


# ------------------------------------------------------------------ 11. state
def test_state_views_device_inputs_and_streams():
    import torch
    from openintel_amd import _lib
    n, B, t, kw = 3000, 64, 10.5, dict(n_buckets=4, stamp_origin=0, bucket_width=1)
    ctx = _ctx()
    rows, q = _ints(n, 384, B, seed=111)
    stamp = np.random.default_rng(111).integers(0, 4, size=n).astype(np.uint32)
    idx = _index(ctx, rows, None, None, stamp)                     # no signals yet
    with pytest.raises(_lib.OiError) as e:
        idx.similar_summary(q, t)
    assert e.value.code == _lib.OI_ERR_STATE and "signals" in e.value.message
    ctx_v0, ctx_v = _ctx(), _ctx()
    early = idx.view(ctx_v0)                                       # a view made before signals existed has none
    sig = _signals(n, 1)
    idx.set_signals(sig.pol, sig.spec, sig.src, TAU)
    with pytest.raises(_lib.OiError) as e:
        early.similar_summary(q, t)
    assert e.value.code == _lib.OI_ERR_STATE
    S = _exact_scores(rows, q)
    want = _ref(S, t, sig, 4, 0, 1, stamp)
    _same(idx.similar_summary(q, t, **kw), want)
    assert idx.similar_summary(q[:0], t, **kw).shape == (0, 4)      # n_queries == 0
    # a view on another ctx and another stream sees the signals set before it was made, and those overwritten after
    st = torch.cuda.Stream()
    ctx_v.set_stream(st)
    v = idx.view(ctx_v)
    with pytest.raises(_lib.OiError) as e:
        v.set_signals(sig.pol, sig.spec, sig.src, TAU)
    assert e.value.code == _lib.OI_ERR_STATE
    F = np.array([ALL if b % 3 else (0, 0, 1, 2) for b in range(B)], dtype=np.uint32)
    with torch.cuda.stream(st):
        dq = torch.from_numpy(q).cuda()
        o1 = v.similar_summary(dq, t, **kw)
        o2 = v.similar_summary(dq, t, filters=F, **kw)
        o3 = v.similar_summary(dq[:33], t, **kw)
    st.synchronize()
    assert o1.is_cuda and tuple(o1.shape) == (B, 4, 8)
    _same(o1, want)
    _same(o3, want[:33])
    _same(o2, _ref(S, t, sig, 4, 0, 1, stamp, np.zeros(n, np.uint32), F))
    dev, _ = ctx_v.workspace_bytes()
    assert dev >= (32 << 20) + B * 4 * 64                           # the band buffer and the 64-byte cells are counted
    # overwritten after the view was made, with device-located inputs: the same records as host-located ones give
    sig2 = _signals(n, 2)
    idx.set_signals(torch.from_numpy(sig2.pol).cuda(), torch.from_numpy(sig2.spec).cuda(), torch.from_numpy(sig2.src).cuda(), TAU)
    want2 = _ref(S, t, sig2, 4, 0, 1, stamp)
    _same(idx.similar_summary(q, t, **kw), want2)
    with torch.cuda.stream(st):
        o4 = v.similar_summary(dq, t, **kw)
    st.synchronize()
    _same(o4, want2)
    assert want2.tobytes() != want.tobytes()
    v.close()
    early.close()


@pytest.mark.parametrize("dim", [384, 20])
def test_buckets_or_filters_without_attributes(dim):
    from openintel_amd import _lib
    ctx = _ctx()
    rows, q = _ints(100, dim, 2, seed=4)
    sig = _signals(100, 4)
    idx = _index(ctx, rows, sig, finalize=dim == 384)
    _same(idx.similar_summary(q, 0.5), _ref(_exact_scores(rows, q), 0.5, sig))    # bucket_width == 0 works
    with pytest.raises(_lib.OiError) as e:
        idx.similar_summary(q, 0.5, n_buckets=2, stamp_origin=0, bucket_width=5)
    assert e.value.code == _lib.OI_ERR_STATE
    with pytest.raises(_lib.OiError) as e:
        idx.similar_summary(q, 0.5, filters=np.array([ALL, ALL], dtype=np.uint32))
    assert e.value.code == _lib.OI_ERR_STATE


# ------------------------------------------------------------------ 12. odd values
def test_infinite_thresholds_nan_rows_and_queries_without_a_bound(fl):
    n, B = fl.n, fl.B
    F = np.array([ALL if b % 2 == 0 else (0, 0, 1, 2) for b in range(B)], dtype=np.uint32)
    S_all = np.zeros((B, n))
    got, ran = _ran(fl.ctx, lambda: fl.idx.similar_summary(fl.q, -INF, filters=F))
    _same(got, _ref(S_all, -INF, fl.sig, stamp=fl.stamp, group=np.zeros(n, np.uint32), filters=F))
    assert "summary_exact" not in ran, ran
    assert fl.idx.similar_summary(fl.q, INF).tobytes() == bytes(64 * B)
    assert fl.view_exact.similar_summary(fl.q, INF).tobytes() == bytes(64 * B)
    # a query without a bound sends the batch through the exact route; the others' records do not move
    want = fl.idx.similar_summary(fl.q, 0.1)
    for bad in (float("nan"), 1e30):
        q = fl.q.copy()
        q[5, 3] = bad
        got, ran = _ran(fl.ctx, lambda: fl.idx.similar_summary(q, 0.1))
        assert "summary_exact" in ran, ran
        keep = np.arange(B) != 5
        _same(got[keep], want[keep])
        if bad != bad:
            assert got[5].tobytes() == bytes(64)                                   # every similarity is NaN
    # a NaN row is never counted, at any threshold (such a corpus is never screened)
    rows = fl.rows[:300].copy()
    rows[7, 100] = np.nan
    ctx = _ctx()
    sig = _signals(300, 5)
    idx = _index(ctx, rows, sig)
    S = fl.S[:, :300].copy()
    S[:, 7] = np.nan
    got, ran = _ran(ctx, lambda: idx.similar_summary(fl.q, -INF))
    _same(got, _ref(S, -INF, sig))
    assert ran == {"summary_exact"} and int(got["total"][0, 0]) == 299, (got["total"][:2], ran)
    _same(idx.similar_summary(fl.q, 0.05), _ref(S, 0.05, sig))
