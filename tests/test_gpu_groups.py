"""Similarity leaderboard (oi_similar_groups): cell (q, key) = the social_summary raw sums over the documents that
pass query q's filter, have key (group & key_mask) >> ctz(key_mask) == key and sim(q, d) >= t_q; dense, or the best `top` keys
ranked on the device.  The reference is numpy in this file, as in tests/test_gpu_summary.py (whose corpora and signal values
these are): an exact (int64) or f64 similarity matrix, the three clauses, bincount per key, float(int(sum of rint(v * 2^30))) *
2^-30 for the polarity sum, and the ranking by Python sort on (-v, key).  All eight record fields, the keys, the counts and
`qualified` are compared bit for bit."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ALL = (0, 0, 0, 0xFFFFFFFF)
NONE = (0, 0, 7, 6)
TAGS = ("groups", "groups_band", "groups_exact", "groups_rank")
RANKS = ("total", "spec", "bullish", "bearish")
RANK_FIELD = {"total": "total", "spec": "spec_count", "bullish": "bullish", "bearish": "bearish"}
TAU = 0.2
INF = float("inf")
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
        self.q30 = np.rint(v * 2.0 ** 30).astype(np.int64)
        self.bull, self.bear = v > TAU, v < -TAU
        self.neu = ~self.bull & ~self.bear
        self.sp = spec != 0
        self.s1 = (src != 0) if src is not None else np.zeros(pol.size, bool)


def _signals(n, seed, vals=VALS):
    rng = np.random.default_rng(1000 + seed)
    return _Sig(vals[rng.integers(0, vals.size, size=n)], rng.integers(0, 2, size=n).astype(np.uint8),
                rng.integers(0, 2, size=n).astype(np.uint8))


def _index(ctx, rows, sig=None, group=None, stamp=None, finalize=True, copy=None, bf16=False):
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


def _keys_of(group, mask):
    shift = (mask & -mask).bit_length() - 1
    return ((group.astype(np.uint64) & mask) >> shift).astype(np.int64)


def _ref(S, t, sig, group, mask, nk, stamp=None, filters=None):
    """The definition, dense: S [B][n] exact (or f64) similarities, t a threshold or one per query -> [B][nk] records."""
    B, n = S.shape
    tq = np.broadcast_to(np.asarray(t, dtype=np.float64), (B,))
    with np.errstate(invalid="ignore"):
        hit = S >= tq[:, None]
    key = _keys_of(group, mask)
    inb = key < nk
    if stamp is None:
        stamp = np.zeros(n, np.uint32)
    out = np.zeros((B, nk), _dtype())

    def count(m):
        return np.bincount(key[m], minlength=nk)[:nk]

    for q in range(B):
        ok = hit[q] & inb
        if filters is not None:
            ok &= _passes(filters[q], group, stamp)
        out["total"][q] = count(ok)
        out["by_source"][q, :, 1] = count(ok & sig.s1)
        out["by_source"][q, :, 0] = out["total"][q] - out["by_source"][q, :, 1]
        out["bullish"][q], out["bearish"][q], out["neutral"][q] = count(ok & sig.bull), count(ok & sig.bear), count(ok & sig.neu)
        out["spec_count"][q] = count(ok & sig.sp)
        s = np.zeros(nk, np.int64)
        np.add.at(s, key[ok], sig.q30[ok])
        out["polarity_sum"][q] = [float(int(x)) * 2.0 ** -30 for x in s]
    return out


def _rank(dense, top, by, min_total):
    """The ranking of dense records [B][nk] by Python sort on (-v, key): (keys, records, counts, qualified)."""
    B, nk = dense.shape
    keys = np.full((B, top), 0xFFFFFFFF, np.uint32)
    recs = np.zeros((B, top), _dtype())
    counts, qual = np.zeros(B, np.uint32), np.zeros(B, np.uint32)
    bar = max(min_total, 1)
    for q in range(B):
        v = dense[RANK_FIELD[by]][q].tolist()
        listed = sorted(np.flatnonzero(dense["total"][q] >= bar).tolist(), key=lambda k: (-v[k], k))
        qual[q] = len(listed)
        listed = listed[:top]
        counts[q] = len(listed)
        keys[q, :len(listed)] = listed
        recs[q, :len(listed)] = dense[q, listed]
    return keys, recs, counts, qual


def _host(x):
    if hasattr(x, "data_ptr"):
        a = x.cpu().numpy()
        if a.dtype == np.int64:
            return a.view(_dtype()).reshape(a.shape[0], a.shape[1])
        return a.view(np.uint32)
    return x


def _same(got, ref):
    """all eight fields bit for bit (the f64 sum included: compared as its 64 bits)"""
    got = _host(got)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    a, b = np.ascontiguousarray(got).view(np.uint64).reshape(-1, 8), np.ascontiguousarray(ref).view(np.uint64).reshape(-1, 8)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, (bad[:4], got.reshape(-1)[bad[:2]], ref.reshape(-1)[bad[:2]])


def _same_ranking(got, dense, top, by, min_total):
    keys, recs, counts, qual = _rank(dense, top, by, min_total)
    assert np.array_equal(_host(got.counts), counts), (by, top, min_total, _host(got.counts)[:4], counts[:4])
    assert np.array_equal(_host(got.qualified), qual), (by, top, min_total)
    assert np.array_equal(_host(got.keys), keys), (by, top, min_total)
    _same(got.records, recs)


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


def _groups(n, nk_drawn, mask, seed):
    """group words whose key under `mask` is uniform in [0, nk_drawn), with random bits everywhere outside the mask"""
    rng = np.random.default_rng(2000 + seed)
    shift = (mask & -mask).bit_length() - 1
    key = rng.integers(0, nk_drawn, size=n).astype(np.uint64)
    noise = rng.integers(0, 1 << 32, size=n, dtype=np.uint64) & np.uint64(~mask & 0xFFFFFFFF)
    return ((key << np.uint64(shift)) | noise).astype(np.uint32)


# ------------------------------------------------------------------ 1. the stream route on integer corpora
@pytest.mark.parametrize("dim,n,B,nk,mask,drawn", [(384, 1, 1, 1, 0x1, 1), (768, 33, 64, 7, 0xF, 7), (384, 28672, 65, 300, 0xFFF0, 300),
                                                   (768, 28773, 65, 300, 0xFFFFFFFF, 400)])
def test_integer_corpus_screen_route_dense_and_ranked(dim, n, B, nk, mask, drawn):
    ctx = _ctx()
    rows, q = _ints(n, dim, B, seed=n + B)
    sig = _signals(n, n + B)
    group = _groups(n, drawn, mask, n)
    idx = _index(ctx, rows, sig, group)
    S = _exact_scores(rows, q)
    for m in (-3, 20):
        t = m + 0.5
        dense = _ref(S, t, sig, group, mask, nk)
        got, ran = _ran(ctx, lambda: idx.similar_groups(q, t, mask, nk))
        _same(got, dense)
        assert "groups" in ran and "groups_exact" not in ran and "groups_rank" not in ran, ran
        for by in RANKS:
            for top in sorted({1, 5, nk, 1024}):
                for min_total in (0, 3):
                    got, ran = _ran(ctx, lambda: idx.similar_groups(q, t, mask, nk, top=top, rank_by=by, min_total=min_total))
                    _same_ranking(got, dense, top, by, min_total)
                    assert "groups" in ran and "groups_rank" in ran and "groups_exact" not in ran, ran
    assert n < 33 or _ref(S, -2.5, sig, group, mask, nk)["total"].sum() > 0
    if drawn > nk:
        assert (_keys_of(group, mask) >= nk).any()                  # some documents have no cell


# ------------------------------------------------------------------ 2. the exact route
@pytest.mark.parametrize("kind,dim,n,B", [("f32", 4, 333, 6), ("f32", 20, 8300, 5), ("f32", 1024, 301, 65), ("bf16", 1024, 301, 7),
                                          ("exact_ctx", 768, 1000, 33), ("no_copy", 768, 1000, 64)])
def test_integer_corpus_exact_route(kind, dim, n, B):
    from openintel_amd import _lib
    ctx = _ctx(_lib.OI_COSINE_EXACT if kind == "exact_ctx" else None)
    rows, q = _ints(n, dim, B, seed=n + B)
    sig = _signals(n, n + B)
    mask, nk = 0x3F00, 50
    group = _groups(n, 64, mask, n)                                 # keys 50 .. 63 have no cell
    if kind == "bf16":
        idx = _index(ctx, (rows.view(np.uint32) >> 16).astype(np.uint16), sig, group, finalize=False, bf16=True)
    elif kind == "no_copy":
        idx = _index(ctx, rows, sig, group, copy=_lib.OI_SCREEN_COPY_NEVER)
    else:
        idx = _index(ctx, rows, sig, group, finalize=kind == "exact_ctx")
    S = _exact_scores(rows, q)
    for m in (-1, 3):
        dense = _ref(S, m + 0.5, sig, group, mask, nk)
        got, ran = _ran(ctx, lambda: idx.similar_groups(q, m + 0.5, mask, nk))
        _same(got, dense)
        assert ran == {"groups_exact"}, ran
        got, ran = _ran(ctx, lambda: idx.similar_groups(q, m + 0.5, mask, nk, top=7, rank_by="bullish", min_total=2))
        _same_ranking(got, dense, 7, "bullish", 2)
        assert ran == {"groups_exact", "groups_rank"}, ran


# ------------------------------------------------------------------ 3. the band is rescored
def _planted(dim, n=28773, B=64, t=0.5, seed=7):
    """the planted corpus of tests/test_gpu_summary.py (same generator, same seeds): per query 40 rows a q + sqrt(1 - a^2) u, u
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
def test_the_band_is_rescored(dim):
    t = 0.5
    rows, q = _planted(dim, t=t)
    S = q.astype(np.float64) @ rows.astype(np.float64).T
    assert np.abs(S - t).min() > 2e-5
    Sb = _bf16_round(q).astype(np.float64) @ _bf16_round(rows).astype(np.float64).T
    wrong = int(((Sb >= t) != (S >= t)).sum())
    assert wrong >= 20, wrong
    ctx = _ctx()
    n = rows.shape[0]
    sig = _signals(n, dim)
    group = (np.arange(n) % 5).astype(np.uint32)
    idx = _index(ctx, rows, sig, group)
    dense = _ref(S, t, sig, group, 0x7, 5)
    got, ran = _ran(ctx, lambda: idx.similar_groups(q, t, 0x7, 5))
    print("planted d=%d: bf16-misclassified %d, hits %d, library %d" % (dim, wrong, int(dense["total"].sum()), int(got["total"].sum())))
    _same(got, dense)
    assert "groups" in ran and "groups_band" in ran and "groups_exact" not in ran, ran
    _same_ranking(idx.similar_groups(q, t, 0x7, 5, top=5, rank_by="spec"), dense, 5, "spec", 0)


# ------------------------------------------------------------------ 4. long rows
def test_long_rows_are_summed_by_the_band_kernel():
    dim, n, B, t = 384, 28773, 64, 0.5
    rng = np.random.default_rng(21)
    rows, q = _unit(rng, n, dim), _unit(rng, B, dim)
    long_at = np.array([0, 31, 4097, 20000, 28671, 28772])
    for i, r in enumerate(long_at):
        a = (0.02, 0.005, 0.0104, 0.0096, -0.02, 0.011)[i]
        u = rng.standard_normal(dim)
        u -= (u @ q[0]) * q[0]
        rows[r] = 50.0 * (a * q[0] + np.sqrt(1 - a * a) * u / np.linalg.norm(u))
    rows, q = rows.astype(np.float32), q.astype(np.float32)
    S = q.astype(np.float64) @ rows.astype(np.float64).T
    is_long = np.zeros(n, bool)
    is_long[long_at] = True
    assert np.abs(S[:, is_long] - t).min() > 1e-3 and np.abs(S[:, ~is_long] - t).min() > 2e-5
    assert (S[:, is_long] >= t).any() and (S[:, is_long] < t).any()
    ctx = _ctx()
    group = (np.arange(n) % 3).astype(np.uint32)
    stamp = (np.arange(n) % 4).astype(np.uint32)
    sig = _signals(n, 21)
    sig.pol[long_at] = (1.0, -1.0 / 3.0, 0.25, -0.5, 1.0 / 3.0, -1.0)
    sig = _Sig(sig.pol, sig.spec, sig.src)
    idx = _index(ctx, rows, sig, group, stamp)
    assert idx.long_rows() == long_at.size
    F = np.array([ALL if b % 2 == 0 else (0, 0, 1, 2) for b in range(B)], dtype=np.uint32)
    for f in (None, F):
        got, ran = _ran(ctx, lambda: idx.similar_groups(q, t, 0x3, 3, filters=f))
        _same(got, _ref(S, t, sig, group, 0x3, 3, stamp, f))
        assert "groups" in ran and "groups_band" in ran and "groups_exact" not in ran, ran


# ------------------------------------------------------------------ 5. band overflow falls back inside the call
def test_band_overflow_falls_back_inside_the_call():
    dim, n, B = 384, 65632, 64
    rows = np.zeros((n, dim), np.float32)
    rows[:, 0] = 0.5
    rows[:, 1] = (np.arange(n) % 97) / 256.0
    q = np.zeros((B, dim), np.float32)
    q[:, 0] = 1.0
    assert B * n > 4 << 20
    sig = _signals(n, 7, vals=np.array([-1.0, -1.0 / 3.0, -0.2, 0.0, 0.25]))
    group = (np.arange(n) % 97).astype(np.uint32)
    S = np.full((B, n), 0.5)
    full = _ref(S, 0.5, sig, group, 0x7F, 97)
    assert full["polarity_sum"].max() < -10.0                       # per-cell sums are NEGATIVE: a stale i64 would show
    ctx = _ctx()
    idx = _index(ctx, rows, sig, group)
    got, ran = _ran(ctx, lambda: idx.similar_groups(q, 0.5, 0x7F, 97))
    _same(got, full)
    assert "groups_exact" in ran, ran
    got, ran = _ran(ctx, lambda: idx.similar_groups(q, 0.75, 0x7F, 97))          # the flags of the first call are gone
    assert got.tobytes() == bytes(64 * B * 97) and "groups" in ran and "groups_exact" not in ran, (int(got["total"].sum()), ran)
    rk = idx.similar_groups(q, 0.75, 0x7F, 97, top=10)
    assert not rk.counts.any() and not rk.qualified.any() and (rk.keys == 0xFFFFFFFF).all() and rk.records.tobytes() == bytes(64 * B * 10)
    got, ran = _ran(ctx, lambda: idx.similar_groups(q, 0.25, 0x7F, 97))          # proven hits only
    _same(got, full)
    assert "groups_exact" not in ran, ran


# ------------------------------------------------------------------ 6. ties
def test_ties_are_broken_by_key_ascending():
    dim, n, B = 384, 4096, 2
    rows = np.zeros((n, dim), np.float32)
    rows[:, 0] = 1.0
    q = np.zeros((B, dim), np.float32)
    q[:, 0] = 1.0
    group = (np.arange(n) % 64).astype(np.uint32)
    sig = _signals(n, 6)
    ctx = _ctx()
    idx = _index(ctx, rows, sig, group)
    S = np.ones((B, n))
    dense = _ref(S, 0.5, sig, group, 0x3F, 64)
    assert (dense["total"] == 64).all()
    for top in (1, 63, 64, 100):
        got = idx.similar_groups(q, 0.5, 0x3F, 64, top=top)
        m = min(top, 64)
        assert (got.counts == m).all() and (got.qualified == 64).all()
        assert np.array_equal(got.keys[:, :m], np.tile(np.arange(m, dtype=np.uint32), (B, 1))), top
        _same_ranking(got, dense, top, "total", 0)
    # three keys get more documents (their neighbours fewer): 17 leads, then 40, then the tie run, cut inside it
    group2 = group.copy()
    group2[np.flatnonzero(group == 3)[:5]] = 17
    group2[np.flatnonzero(group == 5)[:2]] = 40
    group2[np.flatnonzero(group == 9)[:2]] = 40
    idx.set_doc_attrs(group2, None)
    dense = _ref(S, 0.5, sig, group2, 0x3F, 64)
    got = idx.similar_groups(q, 0.5, 0x3F, 64, top=64)
    assert list(got.keys[0, :4]) == [17, 40, 0, 1] and list(got.keys[0, -3:]) == [5, 9, 3]
    for top in (1, 2, 5, 64):
        _same_ranking(idx.similar_groups(q, 0.5, 0x3F, 64, top=top), dense, top, "total", 0)
    _same_ranking(idx.similar_groups(q, 0.5, 0x3F, 64, top=100, min_total=63), dense, 100, "total", 63)


# ------------------------------------------------------------------ 7. a large key space
@pytest.mark.parametrize("nk,mask,B", [(65536, 0xFFFF0000, 16), (8192, 0x1FFF, 3), (8193, 0x3FFF, 3)])
def test_large_key_spaces(nk, mask, B):
    dim, n = 384, 1000
    ctx = _ctx()
    rows, q = _ints(n, dim, B, seed=nk)
    sig = _signals(n, nk)
    group = _groups(n, nk, mask, nk)
    group[:3] = np.uint32(((nk - 1) << ((mask & -mask).bit_length() - 1)) & 0xFFFFFFFF)   # the last key is in use
    idx = _index(ctx, rows, sig, group)
    S = _exact_scores(rows, q)
    t = -2.5
    dense = _ref(S, t, sig, group, mask, nk)
    assert dense["total"][:, nk - 1].sum() > 0
    _same(idx.similar_groups(q, t, mask, nk), dense)
    for by, top, mt in (("total", 1024, 0), ("bearish", 1024, 0), ("total", 100, 2), ("spec", 1, 0)):
        got, ran = _ran(ctx, lambda: idx.similar_groups(q, t, mask, nk, top=top, rank_by=by, min_total=mt))
        _same_ranking(got, dense, top, by, mt)
        assert "groups_rank" in ran, ran
    dev, _ = ctx.workspace_bytes()
    assert dev >= B * nk * (64 + 8)                                  # the cells and the rank keys are counted


# ------------------------------------------------------------------ 8. filters, retagging, views, state
def test_filters_retagging_views_and_state():
    from openintel_amd import _lib
    n, B, t, mask, nk = 3000, 8, -10.5, 0xFF00, 200
    ctx = _ctx()
    rows, q = _ints(n, 384, B, seed=88)
    rng = np.random.default_rng(88)
    stamp = rng.integers(900, 6000, size=n).astype(np.uint32)
    group = _groups(n, 256, mask, 88)
    sig = _signals(n, 88)
    S = _exact_scores(rows, q)
    bare = _index(ctx, rows, sig)                                   # no attributes: the key axis has nothing to read
    with pytest.raises(_lib.OiError) as e:
        bare.similar_groups(q, t, mask, nk)
    assert e.value.code == _lib.OI_ERR_STATE and "attributes" in e.value.message
    nosig = _index(ctx, rows, None, group, stamp)
    with pytest.raises(_lib.OiError) as e:
        nosig.similar_groups(q, t, mask, nk)
    assert e.value.code == _lib.OI_ERR_STATE and "signals" in e.value.message
    idx = _index(ctx, rows, sig, group, stamp)
    ctx_v = _ctx()
    v = idx.view(ctx_v)
    F = np.array([ALL, (3, 1, 0, 0xFFFFFFFF), (0, 0, 1005, 1014), NONE, (0xF, 2, 1500, 0xFFFFFFFF), ALL, (0, 0, 2000, 4000),
                  (1, 0, 0, 5000)], dtype=np.uint32)
    dense = _ref(S, t, sig, group, mask, nk, stamp, F)
    assert dense["total"].sum() > 0 and dense["total"][3].sum() == 0
    for h in (idx, v):
        _same(h.similar_groups(q, t, mask, nk, filters=F), dense)
        _same_ranking(h.similar_groups(q, t, mask, nk, top=9, rank_by="bearish", min_total=2, filters=F), dense, 9, "bearish", 2)
    assert idx.similar_groups(q[:0], t, mask, nk).shape == (0, nk)   # n_queries == 0
    group2 = np.roll(group, 7)                                       # retagged in place: the view sees it
    idx.set_doc_attrs(group2, stamp)
    dense2 = _ref(S, t, sig, group2, mask, nk, stamp, F)
    assert dense2.tobytes() != dense.tobytes()
    _same(v.similar_groups(q, t, mask, nk, filters=F), dense2)
    _same(idx.similar_groups(q, t, mask, nk, filters=F), dense2)
    v.close()


# ------------------------------------------------------------------ 9. consistency with the summary
def test_keys_sum_to_the_summary_and_ranked_records_are_the_dense_ones():
    dim, n, B = 768, 28773, 64
    rng = np.random.default_rng(33)
    rows, q = _unit(rng, n, dim).astype(np.float32), _unit(rng, B, dim).astype(np.float32)
    dyadic = np.array([-1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0])     # polarity sums add exactly
    sig = _signals(n, 33, vals=dyadic)
    group = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    stamp = rng.integers(0, 100, size=n).astype(np.uint32)
    ctx = _ctx()
    idx = _index(ctx, rows, sig, group, stamp)
    F = np.array([ALL if b % 3 else (0, 0, 10, 60) for b in range(B)], dtype=np.uint32)
    mask, nk = 0x00FF0000, 256                                       # every document has a key
    for t in (0.05, 0.1):
        dense = idx.similar_groups(q, t, mask, nk, filters=F)
        one = idx.similar_summary(q, t, filters=F)
        assert one["total"].sum() > 0
        for f in ("total", "by_source", "bullish", "bearish", "neutral", "spec_count", "polarity_sum"):
            assert np.array_equal(dense[f].sum(axis=1), one[f][:, 0]), f
        for by in RANKS:
            got = idx.similar_groups(q, t, mask, nk, top=20, rank_by=by, min_total=2, filters=F)
            _same_ranking(got, dense, 20, by, 2)


# ------------------------------------------------------------------ 10. device location and thresholds
def test_device_location_and_per_query_thresholds():
    import torch
    dim, n, B, mask, nk = 384, 2000, 65, 0xFF, 100
    ctx = _ctx()
    rows, q = _ints(n, dim, B, seed=44)
    sig = _signals(n, 44)
    group = _groups(n, 128, mask, 44)
    idx = _index(ctx, rows, sig, group)
    S = _exact_scores(rows, q)
    choices = np.array([-INF, -3.5, 0.5, 20.5, INF, np.nan], dtype=np.float32)
    thr = choices[np.random.default_rng(4).integers(0, choices.size, size=B)]
    thr[:choices.size] = choices
    dense = _ref(S, thr, sig, group, mask, nk)
    got = idx.similar_groups(q, thr, mask, nk)
    _same(got, dense)
    rk = idx.similar_groups(q, thr, mask, nk, top=12, rank_by="total")
    _same_ranking(rk, dense, 12, "total", 0)
    nan_q, inf_q, minf_q = np.flatnonzero(np.isnan(thr)), np.flatnonzero(thr == INF), np.flatnonzero(thr == -INF)
    assert not rk.counts[nan_q].any() and not rk.counts[inf_q].any() and (rk.qualified[minf_q] == nk).all()
    assert got[nan_q].tobytes() == bytes(64 * nk * nan_q.size)
    dq = torch.from_numpy(q).cuda()
    d_dense = idx.similar_groups(dq, torch.from_numpy(thr).cuda(), mask, nk)
    d_rk = idx.similar_groups(dq, thr, mask, nk, top=12, rank_by="total")      # (a host array beside device queries is moved)
    ctx.synchronize()
    assert d_dense.is_cuda and tuple(d_dense.shape) == (B, nk, 8) and tuple(d_rk.records.shape) == (B, 12, 8)
    _same(d_dense, dense)
    _same_ranking(d_rk, dense, 12, "total", 0)
    for t in (INF, -INF):
        _same(idx.similar_groups(q, t, mask, nk), _ref(S, t, sig, group, mask, nk))


# ------------------------------------------------------------------ 11. the reference's own numbers
@pytest.mark.parametrize("dim", [4, 384])
def test_the_reference_fixture_as_one_ticker_among_others(dim):
    from openintel_amd import batch
    from openintel_amd.engine import SpeculationEngine
    here = os.path.dirname(os.path.abspath(__file__))
    golden = json.load(open(os.path.join(here, "golden", "reference_fixture.json")))
    posts = golden["fixture_posts"]
    filler = ["to the moon", "puts printing", "no opinion", "yolo calls", "bearish crash"] * 4
    texts = [p["text"] for p in posts] + filler
    sources = np.array([0 if p["source"] == "reddit" else 1 for p in posts] + [0, 1] * 10, np.uint8)
    n = len(texts)
    group = np.array([3] * len(posts) + [0, 1, 2, 4, 5] * 4, np.uint32) << np.uint32(4)
    rng = np.random.default_rng(10)
    rows = _unit(rng, n, dim).astype(np.float32)
    q = _unit(rng, 1, dim).astype(np.float32)
    ctx = _ctx()
    idx = _index(ctx, rows, None, group, finalize=dim == 384)
    idx.set_signals_from_text(texts, sources, TAU)
    got, ran = _ran(ctx, lambda: idx.similar_groups(q, -INF, 0xF0, 6))
    assert ("groups" in ran and "groups_exact" not in ran) if dim == 384 else ran == {"groups_exact"}, ran
    assert list(got["total"][0]) == [4, 4, 4, 10, 4, 4]
    s = SpeculationEngine.social_from_counters(got[0, 3])
    want = golden["derived"]["summary"]
    assert s.total_mentions == want["total_mentions"] == 10
    assert {k.as_str(): v for k, v in s.mentions_by_source.items()} == want["mentions_by_source"] == {"reddit": 4, "bluesky": 6}
    assert (s.bullish, s.bearish, s.neutral) == (want["bullish"], want["bearish"], want["neutral"]) == (7, 2, 1)
    assert float(s.net_sentiment) == want["net_sentiment"] == 0.5
    assert float(s.speculation_index) == want["speculation_index"] == 0.3
    assert s.bull_bear_ratio == want["bull_bear_ratio"] == 3.5
    # compare_index: one ranked call, then the host ranking; only the fixture's ticker has min_sample posts
    import openintel_amd as oi
    m = golden["mock_market"]
    snap = oi.MarketSnapshot(oi.Ticker.parse("AAPL"), m["last_price"], m["previous_close"], m["volume"], m["avg_volume"],
                             m["realized_vol"], m["put_call_ratio"], m["iv_rank"])
    names = ["AAA", "BBB", "CCC", "AAPL", "DDD", "EEE"]
    out = batch.compare_index(idx, q[0], -INF, names, 0xF0, market_by_ticker={"AAPL": snap})
    assert [r.ticker for r in out.ranked] == ["AAPL"] and not out.errors and out.rank_by is batch.RankBy.CROWDING
    rep = out.ranked[0].report
    so = rep.social
    assert (so.total_mentions, so.bullish, so.bearish, so.neutral) == (10, 7, 2, 1)
    assert (float(so.net_sentiment), float(so.speculation_index), so.bull_bear_ratio) == (0.5, 0.3, 3.5)
    assert {k.as_str(): v for k, v in so.mentions_by_source.items()} == {"reddit": 4, "bluesky": 6}
    assert rep.fusion.crowding == want["crowding"] == out.ranked[0].rank_metric and rep.fusion.alignment.value == want["alignment"]
    assert rep.market.pct_change == want["pct_change"] and rep.market.rvol == want["rvol"]
    assert rep.social_confidence.value == want["social_confidence"]
    everyone = batch.compare_index(idx, q[0], -INF, names, 0xF0, min_total=1, rank_by=batch.RankBy.NET_SENTIMENT)
    assert sorted(r.ticker for r in everyone.ranked) == sorted(names)
    vals = [r.rank_metric for r in everyone.ranked]
    assert vals == sorted(vals, reverse=True)


# ------------------------------------------------------------------ the host location, dense and ranked, with and without qualified
def test_host_location_is_the_device_location_bit_for_bit_dense_and_ranked():
    """300 rows (a ragged last block of 64), dim 64, 2 queries, 4 keys.  Dense (top == 0: no keys, counts or qualified) and ranked:
    OI_HOST gives OI_DEVICE's bytes; ranked without qualified_out: records, keys and counts are as they were."""
    import ctypes as C
    import torch
    from openintel_amd import _lib
    ctx = _ctx()
    n, dim, B, mask, nk, t, top = 300, 64, 2, 0xFF00, 4, 0.5, 3
    rows, q = _ints(n, dim, B, seed=92)
    sig, group = _signals(n, 92), _groups(n, 6, mask, 92)          # keys 4 and 5 belong to no cell
    idx = _index(ctx, rows, sig, group)
    dq = torch.from_numpy(q).cuda()
    host = idx.similar_groups(q, t, mask, nk)
    dev = idx.similar_groups(dq, t, mask, nk)
    ctx.synchronize()
    _same(host, _ref(_exact_scores(rows, q), t, sig, group, mask, nk))
    assert (host["total"] > 0).all()
    assert np.ascontiguousarray(_host(dev)).tobytes() == host.tobytes()
    ranked = idx.similar_groups(q, t, mask, nk, top=top)
    d_ranked = idx.similar_groups(dq, t, mask, nk, top=top)
    ctx.synchronize()
    _same_ranking(ranked, host, top, "total", 0)
    for f in ("keys", "records", "counts", "qualified"):
        assert np.ascontiguousarray(_host(getattr(d_ranked, f))).tobytes() == getattr(ranked, f).tobytes(), f
    spec = _lib.GroupsSpec(t, mask, nk, top, 0, 0)
    rec, keys, counts = np.zeros((B, top), _dtype()), np.zeros((B, top), np.uint32), np.zeros(B, np.uint32)
    _lib.check(idx.lib.oi_similar_groups(idx.handle, _lib.ptr(q), B, C.byref(spec), None, None, _lib.OI_HOST, _lib.ptr(rec), _lib.ptr(keys),
                                         _lib.ptr(counts), None))
    assert rec.tobytes() == ranked.records.tobytes() and keys.tobytes() == ranked.keys.tobytes() and counts.tobytes() == ranked.counts.tobytes()
