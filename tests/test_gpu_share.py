"""Similarity share (oi_similar_share): every document is counted at most once, under the candidate query with the
largest similarity (ties to the smallest query).  The reference is numpy in this file, in the style of
tests/test_gpu_summary.py: an exact similarity matrix (small-integer corpora: every dot product is an integer, exact in f32 and
in f64, and ties between queries are frequent) or an f64 one (float corpora whose generators keep every decision further from a
tie than the library's 1e-5), the definition of the header, integer counts per cell and float(int(sum of rint(v * 2^30))) *
2^-30 for the polarity sum.  Records are compared as 8 x 64 bits per cell, labels as u32, wherever the result lives."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ALL = (0, 0, 0, 0xFFFFFFFF)
NONE = (0, 0, 7, 6)
TAGS = ("share", "share_band", "share_exact")
TAU = 0.2
INF = float("inf")
NO_LABEL = 0xFFFFFFFF
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
        self.s1 = src != 0


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


def _host(x):
    """records as a numpy record array [B][nb], wherever they live"""
    if hasattr(x, "data_ptr"):
        B, nb = int(x.shape[0]), int(x.shape[1])
        return x.cpu().numpy().view(_dtype()).reshape(B, nb)
    return x


def _host_labels(x):
    if hasattr(x, "data_ptr"):
        return x.cpu().numpy().view(np.uint32)
    return x


def _ran(ctx, call):
    """((records, labels) on the host, the profile tags with at least one launch that did its work, band fill) of one call"""
    ctx.profile_reset(True)
    rec, lab = call()
    ran = {t for t in TAGS if ctx.profile_read(t)[1] > 0}
    fill = int(ctx.profile_read("share_state")[0])
    ctx.profile_reset(False)
    return (_host(rec), _host_labels(lab)), ran, fill


def _passes(f, group, stamp):
    m, v, lo, hi = (int(x) for x in f)
    return ((group & np.uint32(m)) == np.uint32(v)) & (stamp >= np.uint32(lo)) & (stamp <= np.uint32(hi))


def _buckets(n, nb, origin, width, stamp):
    if width:
        s64 = stamp.astype(np.int64)
        b = (s64 - origin) // width                     # 64-bit: origin + nb * width may exceed 2^32
        return b, (s64 >= origin) & (b < nb)
    return np.zeros(n, np.int64), np.ones(n, bool)


def _records_of(labels, B, sig, nb=1, origin=0, width=0, stamp=None):
    """the records that follow from labels (u32 [n], NO_LABEL = not assigned): a row adds its signal to cell (label, bucket)"""
    n = labels.size
    b, _ = _buckets(n, nb, origin, width, stamp)
    out = np.zeros((B, nb), _dtype())

    def count(m):
        return np.bincount(b[m], minlength=nb)[:nb]

    for q in range(B):
        ok = labels == q
        out["total"][q] = count(ok)
        out["by_source"][q, :, 1] = count(ok & sig.s1)
        out["by_source"][q, :, 0] = out["total"][q] - out["by_source"][q, :, 1]
        out["bullish"][q], out["bearish"][q], out["neutral"][q] = count(ok & sig.bull), count(ok & sig.bear), count(ok & sig.neu)
        out["spec_count"][q] = count(ok & sig.sp)
        s = np.zeros(nb, np.int64)
        np.add.at(s, b[ok], sig.q30[ok])
        out["polarity_sum"][q] = [float(int(x)) * 2.0 ** -30 for x in s]
    return out


def _candidates(S, t, stamp=None, group=None, filters=None):
    B, n = S.shape
    tq = np.broadcast_to(np.asarray(t, dtype=np.float64), (B,))
    with np.errstate(invalid="ignore"):
        cand = S >= tq[:, None]                         # (a NaN similarity, or a NaN threshold, is never a candidate)
    if filters is not None:
        for q in range(B):
            cand[q] &= _passes(filters[q], group, stamp)
    return cand


def _ref(S, t, sig, nb=1, origin=0, width=0, stamp=None, group=None, filters=None):
    """The definition: S [B][n] exact (or f64) similarities, t a threshold or one per query -> (records [B][nb], labels [n])."""
    B, n = S.shape
    cand = _candidates(S, t, stamp, group, filters)
    best = np.where(cand, S, -INF)
    win = np.argmax(best, axis=0)                       # the first maximum: ties go to the smallest q
    _, inb = _buckets(n, nb, origin, width, stamp)
    labels = np.where(cand.any(axis=0) & inb, win, NO_LABEL).astype(np.uint32)
    return _records_of(labels, B, sig, nb, origin, width, stamp), labels


def _same(got, ref):
    """all eight fields bit for bit (the f64 sum included: compared as its 64 bits)"""
    got = _host(got)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    a, b = got.view(np.uint64).reshape(-1, 8), ref.view(np.uint64).reshape(-1, 8)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, (bad[:4], got.reshape(-1)[bad[:2]], ref.reshape(-1)[bad[:2]])


def _same_both(got, ref):
    _same(got[0], ref[0])
    lab = _host_labels(got[1])
    assert lab.dtype == np.uint32 and lab.shape == ref[1].shape
    bad = np.flatnonzero(lab != ref[1])
    assert bad.size == 0, (bad[:8], lab[bad[:8]], ref[1][bad[:8]])


def _ints(n, dim, B, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-2, 3, size=(n, dim)).astype(np.float32), rng.integers(-2, 3, size=(B, dim)).astype(np.float32)


def _exact_scores(rows, q):
    return q.astype(np.float64) @ rows.astype(np.float64).T        # small integers: every product and sum is exact


def _tied_rows(S, t):
    """rows with at least two candidates that share the best score"""
    cand = _candidates(S, t)
    best = np.where(cand, S, -INF)
    top = best.max(axis=0)
    return int((((best == top) & cand).sum(axis=0) >= 2).sum())


def _ints_with_a_tie(n, dim, B, seed, t):
    """_ints of the first seed (seed, seed + 1000, ..) whose corpus exercises the tie rule at threshold t (B == 1 cannot)"""
    while True:
        rows, q = _ints(n, dim, B, seed)
        S = _exact_scores(rows, q)
        if B == 1 or _tied_rows(S, t) > 0:
            return rows, q, S
        seed += 1000


def _bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def _unit(rng, n, dim):
    x = rng.standard_normal((n, dim))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


# ------------------------------------------------------------------ 1. the stream route on integer corpora
@pytest.mark.parametrize("dim,n,B", [(384, 1, 1), (384, 31, 32), (768, 32, 33), (768, 33, 64), (768, 28673, 1), (384, 28672, 64),
                                     (768, 28773, 64)])
def test_integer_corpus_stream_route_is_exact(dim, n, B):
    rows, q, S = _ints_with_a_tie(n, dim, B, n + B, -2.5)
    ctx = _ctx()
    sig = _signals(n, n + B)
    idx = _index(ctx, rows, sig)
    for m in (-3, 20):
        t = m + 0.5
        got, ran, fill = _ran(ctx, lambda: idx.similar_share(q, t, labels=True))
        ref = _ref(S, t, sig)
        _same_both(got, ref)
        assert "share" in ran and "share_band" in ran and "share_exact" not in ran, ran
        per_row = _candidates(S, t).sum(axis=0)
        assert fill >= int(per_row[per_row >= 2].sum())             # a row with two or more candidates is always rescored
        if m == -3:
            assert B == 1 or _tied_rows(S, t) > 0
            assert n < 31 or int(ref[0]["total"].sum()) > 0
    _same(idx.similar_share(q, -2.5), _ref(S, -2.5, sig)[0])        # labels_out == NULL


# ------------------------------------------------------------------ 2. more than 64 queries: the exact route
@pytest.mark.parametrize("dim,n", [(384, 33), (768, 1000)])
def test_65_queries_take_the_exact_route(dim, n):
    ctx = _ctx()
    rows, q, S = _ints_with_a_tie(n, dim, 65, n, -2.5)
    sig = _signals(n, n)
    idx = _index(ctx, rows, sig)
    for t in (-2.5, 20.5):
        got, ran, _ = _ran(ctx, lambda: idx.similar_share(q, t, labels=True))
        _same_both(got, _ref(S, t, sig))
        assert ran == {"share_exact"}, ran
    assert _tied_rows(S, -2.5) > 0 and (n < 1000 or (_ref(S, -2.5, sig)[1] == 64).any())    # ties; among 1000 rows the 65th query wins some


# ------------------------------------------------------------------ 3. the exact route, every kind
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
        got, ran, _ = _ran(ctx, lambda: idx.similar_share(q, m + 0.5, labels=True))
        _same_both(got, _ref(S, m + 0.5, sig))
        assert ran == {"share_exact"}, ran
    assert _tied_rows(S, -0.5) > 0


# ------------------------------------------------------------------ 4. reductions
@pytest.mark.parametrize("dim", [384, 20])                        # the stream route and the exact route
def test_reductions_to_the_summary(dim):
    ctx = _ctx()
    rng = np.random.default_rng(40 + dim)
    n, B = 4000, 8
    rows, q = _ints(n, dim, B, seed=40)
    stamp = rng.integers(0, 4, size=n).astype(np.uint32)
    group = rng.integers(0, 1 << 16, size=n).astype(np.uint32)
    sig = _signals(n, 40)
    idx = _index(ctx, rows, sig, group, stamp, finalize=dim == 384)
    S = _exact_scores(rows, q)
    t = -10.5 if dim == 384 else -2.5
    kw = dict(n_buckets=4, stamp_origin=0, bucket_width=1)
    route = "share" if dim == 384 else "share_exact"
    # one query: the summary's records bit for bit
    got, ran, _ = _ran(ctx, lambda: idx.similar_share(q[:1], t, labels=True, **kw))
    _same(got[0], idx.similar_summary(q[:1], t, **kw))
    assert route in ran and (dim != 384 or "share_exact" not in ran), ran
    # pairwise disjoint filters: no document has two candidates
    F = np.array([(7, b, 0, 0xFFFFFFFF) for b in range(B)], dtype=np.uint32)
    got, ran, _ = _ran(ctx, lambda: idx.similar_share(q, t, filters=F, labels=True, **kw))
    want = idx.similar_summary(q, t, filters=F, **kw)
    _same(got[0], want)
    assert int(want["total"].sum()) > 0 and (want["total"].sum(axis=1) > 0).all()
    # a repeated query gets nothing, and no label names it
    q2 = q.copy()
    q2[1] = q2[0]
    got, ran, _ = _ran(ctx, lambda: idx.similar_share(q2, t, labels=True, **kw))
    S2 = _exact_scores(rows, q2)
    _same_both(got, _ref(S2, t, sig, 4, 0, 1, stamp))
    assert got[0][1].tobytes() == bytes(64 * 4) and not (got[1] == 1).any() and (got[1] == 0).any()
    # the records follow from the labels, every document is in at most one cell, and the totals add up to the rows with a candidate
    got, ran, _ = _ran(ctx, lambda: idx.similar_share(q, t, labels=True, **kw))
    _same(got[0], _records_of(got[1], B, sig, 4, 0, 1, stamp))
    has = _candidates(S, t).any(axis=0)
    assert int(got[0]["total"].sum()) == int(has.sum()) == int((got[1] != NO_LABEL).sum())
    assert (got[0]["total"] <= idx.similar_summary(q, t, **kw)["total"]).all()
    assert int(idx.similar_summary(q, t, **kw)["total"].sum()) > int(has.sum())        # (the summary counts such rows more than once)


# ------------------------------------------------------------------ 5. filters, time buckets, per-query thresholds
def _stamps(n, rng):
    """the stamp set of the summary test: below the origin, both edges of every bucket of (origin 1000, width 10, up to 1024
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
FILTERS = np.array([ALL, (3, 1, 0, 0xFFFFFFFF), (0, 0, 1005, 1014), NONE, (0xF, 2, 1500, 0xFFFFFFFF), ALL, (0, 0, 0xFFFFFF10, 0xFFFFFFFE),
                    (1, 0, 0, 5000)], dtype=np.uint32)


@pytest.mark.parametrize("dim,n", [(384, 28773), (20, 2400)])    # the stream route (second tiles, ragged tile) and the exact route
def test_buckets_filters_and_per_query_thresholds(dim, n):
    import torch
    ctx = _ctx()
    rng = np.random.default_rng(11)
    B = 8
    rows, q = _ints(n, dim, B, seed=3)
    stamp = _stamps(n, rng)
    group = rng.integers(0, 1 << 16, size=n).astype(np.uint32)
    sig = _signals(n, 3)
    idx = _index(ctx, rows, sig, group, stamp, finalize=dim == 384)
    S = _exact_scores(rows, q)
    t = -10.5 if dim == 384 else -2.5
    for origin, width, nb in SPECS:
        for f in (None, FILTERS):
            got, ran, _ = _ran(ctx, lambda: idx.similar_share(q, t, n_buckets=nb, stamp_origin=origin, bucket_width=width, filters=f,
                                                               labels=True))
            ref = _ref(S, t, sig, nb, origin, width, stamp, group, f)
            _same_both(got, ref)
            assert ("share" in ran) == (dim == 384) and ("share_exact" in ran) == (dim != 384), ran
        assert ref[0]["total"].sum() > 0 and ref[0]["total"][3].sum() == 0 and not (ref[1] == 3).any()
    _same_both(idx.similar_share(q, t, filters=FILTERS, labels=True), _ref(S, t, sig, stamp=stamp, group=group, filters=FILTERS))
    # per-query thresholds: every kind of value; the -inf query takes every row that no better query takes
    thr = np.array([-INF, -3.5, 0.5, 20.5 if dim == 384 else 2.5, INF, np.nan, -3.5, 0.5], dtype=np.float32)
    kw = dict(n_buckets=1024, stamp_origin=1000, bucket_width=10)
    got, ran, _ = _ran(ctx, lambda: idx.similar_share(q, thr, labels=True, **kw))
    ref = _ref(S, thr, sig, 1024, 1000, 10, stamp)
    _same_both(got, ref)
    assert ("share" in ran) == (dim == 384) and ("share_exact" in ran) == (dim != 384), ran
    inb = _buckets(n, 1024, 1000, 10, stamp)[1]
    assert 100 < int(inb.sum()) < n
    assert ((got[1] != NO_LABEL) == inb).all()                     # every row with a bucket has a winner: query 0 is its candidate
    assert got[0][4].tobytes() == bytes(64 * 1024) and got[0][5].tobytes() == bytes(64 * 1024) and not np.isin(got[1], (4, 5)).any()
    others = np.where(_candidates(S, thr)[1:], S[1:], -INF).max(axis=0)
    assert ((got[1] == 0) == (inb & (S[0] >= others))).all() and (got[1] == 0).any() and (got[1] == 1).any()
    # thresholds, queries and outputs in HBM give the same bytes; a host array beside device queries is moved for the caller
    dq = torch.from_numpy(q).cuda()
    for th in (torch.from_numpy(thr).cuda(), thr):
        rec, lab = idx.similar_share(dq, th, labels=True, **kw)
        assert rec.is_cuda and lab.is_cuda and tuple(rec.shape) == (B, 1024, 8) and tuple(lab.shape) == (n,)
        _same_both((rec, lab), ref)
    dF = torch.from_numpy(FILTERS.view(np.int32)).cuda()
    rec, lab = idx.similar_share(dq, t, filters=dF, labels=True, **kw)
    _same_both((rec, lab), _ref(S, t, sig, 1024, 1000, 10, stamp, group, FILTERS))
    ctx.synchronize()
    if dim == 384:                                                  # a view on another context gives the same bytes
        ctx_v = _ctx()
        v = idx.view(ctx_v)
        _same_both(v.similar_share(q, thr, labels=True, **kw), ref)
        assert v.similar_share(q[:0], 0.5, **kw).shape == (0, 1024)    # n_queries == 0
        dev, _ = ctx_v.workspace_bytes()
        assert dev >= (32 << 20) + 8 * n + B * 1024 * 64               # the band buffer, `best` and the cells are counted
        v.close()


def test_a_nan_query_wins_nothing():
    ctx = _ctx()
    n, dim, B = 2000, 20, 6
    rows, q = _ints(n, dim, B, seed=50)
    sig = _signals(n, 50)
    idx = _index(ctx, rows, sig, finalize=False)
    q[2, 7] = np.nan
    S = _exact_scores(rows, q)
    assert np.isnan(S[2]).all()
    got, ran, _ = _ran(ctx, lambda: idx.similar_share(q, -INF, labels=True))
    _same_both(got, _ref(S, -INF, sig))
    assert got[0][2].tobytes() == bytes(64) and not (got[1] == 2).any() and (got[1] != NO_LABEL).all()


def test_state_errors():
    from openintel_amd import _lib
    ctx = _ctx()
    rows, q = _ints(100, 20, 2, seed=4)
    idx = _index(ctx, rows, None, finalize=False)
    with pytest.raises(_lib.OiError) as e:
        idx.similar_share(q, 0.5)
    assert e.value.code == _lib.OI_ERR_STATE and "signals" in e.value.message
    sig = _signals(100, 4)
    idx.set_signals(sig.pol, sig.spec, sig.src, TAU)
    _same_both(idx.similar_share(q, 0.5, labels=True), _ref(_exact_scores(rows, q), 0.5, sig))
    with pytest.raises(_lib.OiError) as e:
        idx.similar_share(q, 0.5, n_buckets=2, stamp_origin=0, bucket_width=5)
    assert e.value.code == _lib.OI_ERR_STATE
    with pytest.raises(_lib.OiError) as e:
        idx.similar_share(q, 0.5, filters=np.array([ALL, ALL], dtype=np.uint32))
    assert e.value.code == _lib.OI_ERR_STATE
    rec, lab = idx.similar_share(q[:0], 0.5, labels=True)           # no query: no row has a candidate
    assert rec.shape == (0, 1) and (lab == NO_LABEL).all()


# ------------------------------------------------------------------ 6. the band decides, not the screen scores
def _narratives(dim, n, B, seed, t=0.3):
    """B unit queries, each odd one 0.9 x its predecessor + 0.45 x a fresh unit vector (renormalised): overlapping narratives.
    80 % of the rows are 0.6 x a query + 0.8 x unit noise (renormalised), the rest unit noise.  A row with an f64 similarity
    within 3e-5 of t, or whose two best candidate similarities are within 3e-5 of each other, is replaced by a fresh one
    until none is left: nothing the f32 chain could decide the other way stays in the corpus.  Then rows are planted between
    a query and its successor, 100 at a time, with the two similarities 4e-5 .. 2e-4 apart (either way round), until
    assigning by bf16-rounded scores would label at least 20 rows differently.  (The bf16 rounding of unit vectors of these
    dims moves a score by about 1e-4: of 3000 rows planted 3e-4 .. 1e-3 apart it relabelled 0 to 7, measured on the CPU with
    these generators.  The planted gaps therefore sit just above the 3e-5 the preconditions keep clear.)"""
    rng = np.random.default_rng(seed)
    q = _unit(rng, B, dim)
    for b in range(1, B, 2):
        q[b] = 0.9 * q[b - 1] + 0.45 * _unit(rng, 1, dim)[0]
        q[b] /= np.linalg.norm(q[b])
    q = q.astype(np.float32)
    q64 = q.astype(np.float64)

    def fresh(k):
        x = _unit(rng, k, dim)
        c = rng.random(k) < 0.8
        x[c] = 0.6 * q[rng.integers(0, B, size=int(c.sum()))] + 0.8 * x[c]
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        return x.astype(np.float32)

    def close_call():
        """a unit row with sim(q_a) = 0.6 and sim(q_a+1) = 0.6 - d, |d| in 4e-5 .. 2e-4"""
        a = 2 * int(rng.integers(0, B // 2))
        e1 = q64[a] / np.linalg.norm(q64[a])
        c = q64[a + 1] @ e1
        e2 = q64[a + 1] - c * e1
        s = np.linalg.norm(e2)
        e2 /= s
        w = rng.standard_normal(dim)
        w -= (w @ e1) * e1 + (w @ e2) * e2
        w /= np.linalg.norm(w)
        d = rng.uniform(4e-5, 2e-4) * (1 if rng.random() < 0.5 else -1)
        x = 0.6 / np.linalg.norm(q64[a])
        y = ((0.6 - d) / np.linalg.norm(q64[a + 1]) - c * x) / s
        return (x * e1 + y * e2 + np.sqrt(1.0 - x * x - y * y) * w).astype(np.float32)

    def violating(S):
        near_t = (np.abs(S - t) < 3e-5).any(axis=0)
        best = np.sort(np.where(S >= t, S, -INF), axis=0)[-2:]
        with np.errstate(invalid="ignore"):
            return near_t | (np.isfinite(best[0]) & (best[1] - best[0] < 3e-5))

    def settle(rows):
        replaced = 0
        while True:
            S = q64 @ rows.astype(np.float64).T
            bad = np.flatnonzero(violating(S))
            if bad.size == 0:
                return S, replaced
            rows[bad] = fresh(bad.size)
            replaced += bad.size

    rows = fresh(n)
    S, replaced = settle(rows)
    planted = 0
    while planted < n // 2:
        exact = np.where((S >= t).any(axis=0), np.argmax(np.where(S >= t, S, -INF), axis=0), NO_LABEL).astype(np.uint32)
        if int((_bf16_labels(rows, q, t) != exact).sum()) >= 20:
            break
        for r in range(planted, planted + 100):
            rows[r] = close_call()
        planted += 100
        S, more = settle(rows)
        replaced += more
    return rows, q, S, replaced, planted


def _bf16_labels(rows, q, t):
    Sb = _bf16_round(q).astype(np.float64) @ _bf16_round(rows).astype(np.float64).T
    return np.where((Sb >= t).any(axis=0), np.argmax(np.where(Sb >= t, Sb, -INF), axis=0), NO_LABEL).astype(np.uint32)


class _Float:
    pass


_NARR = {}


def _narr(dim, B):
    """one corpus per (dim, B), made once and left unchanged"""
    if (dim, B) not in _NARR:
        f = _Float()
        f.dim, f.n, f.B, f.t = dim, 6000, B, 0.3
        f.rows, f.q, f.S, f.replaced, f.planted = _narratives(dim, f.n, B, seed=7 + (dim == 768) + (B == 64))
        f.sig = _signals(f.n, dim + B)
        f.ref = _ref(f.S, f.t, f.sig)
        _NARR[(dim, B)] = f
    return _NARR[(dim, B)]


@pytest.mark.parametrize("dim,B", [(384, 8), (384, 64), (768, 8), (768, 64)])
def test_the_band_decides_not_the_screen_scores(dim, B):
    f = _narr(dim, B)
    t, S = f.t, f.S
    # the preconditions, on the CPU, before the index is built: NO row is left out of the comparison
    assert np.abs(S - t).min() >= 3e-5
    top2 = np.sort(np.where(S >= t, S, -INF), axis=0)[-2:]
    multi = np.isfinite(top2[0])
    assert (top2[1][multi] - top2[0][multi]).min() >= 3e-5
    wrong = int((_bf16_labels(f.rows, f.q, t) != f.ref[1]).sum())
    print("narratives d=%d B=%d: replaced %d rows, planted %d close calls, %d multi-candidate rows, bf16 scores would label %d rows "
          "differently" % (dim, B, f.replaced, f.planted, int(multi.sum()), wrong))
    assert int(multi.sum()) >= 1000 and wrong >= 20, (int(multi.sum()), wrong)
    ctx = _ctx()
    idx = _index(ctx, f.rows, f.sig)
    got, ran, fill = _ran(ctx, lambda: idx.similar_share(f.q, t, labels=True))
    _same_both(got, f.ref)
    assert ran == {"share", "share_band"}, ran
    assert fill >= int((S >= t).sum(axis=0)[multi].sum())


# ------------------------------------------------------------------ 7. long rows
def test_long_rows_are_assigned_by_the_band_and_the_commit():
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
    top2 = np.sort(np.where(S >= t, S, -INF), axis=0)[-2:]
    multi = np.isfinite(top2[0])
    assert multi[long_at].all() and (top2[1][long_at] - top2[0][long_at]).min() > 1e-3      # every long row has several candidates
    assert not multi[~is_long].any()
    ctx = _ctx()
    stamp = (np.arange(n) % 3).astype(np.uint32)
    sig = _signals(n, 21)
    sig.pol[long_at] = (1.0, -1.0 / 3.0, 0.25, -0.5, 1.0 / 3.0, -1.0)   # a long row's record is never a zero
    sig = _Sig(sig.pol, sig.spec, sig.src)
    idx = _index(ctx, rows, sig, None, stamp)
    assert idx.long_rows() == long_at.size
    F = np.array([ALL if b % 2 == 0 else (0, 0, 1, 2) for b in range(B)], dtype=np.uint32)
    for kw in ({}, dict(n_buckets=3, stamp_origin=0, bucket_width=1, filters=F)):
        got, ran, _ = _ran(ctx, lambda: idx.similar_share(q, t, labels=True, **kw))
        ref = _ref(S, t, sig, kw.get("n_buckets", 1), 0, kw.get("bucket_width", 0), stamp, np.zeros(n, np.uint32), kw.get("filters"))
        _same_both(got, ref)
        assert (ref[1][long_at] != NO_LABEL).all()
        assert ran == {"share", "share_band"}, ran


# ------------------------------------------------------------------ 8. band overflow falls back inside the call
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
    assert (full[1] == 0).all() and full[0][1:].tobytes() == bytes(64 * (B - 1)) and int(full[0]["total"][0, 0]) == n
    assert full[0]["polarity_sum"][0, 0] < -1000.0                # NEGATIVE: a stale i64 of the abandoned stream would show
    ctx = _ctx()
    idx = _index(ctx, rows, sig)
    got, ran, fill = _ran(ctx, lambda: idx.similar_share(q, 0.5, labels=True))
    _same_both(got, full)
    assert "share_exact" in ran and fill == B * n, (ran, fill)
    got, ran, fill = _ran(ctx, lambda: idx.similar_share(q, 0.75, labels=True))    # the flags of the first call are gone
    assert got[0].tobytes() == bytes(64 * B) and (got[1] == NO_LABEL).all(), int(got[0]["total"].sum())
    assert "share" in ran and "share_exact" not in ran and fill == 0, (ran, fill)


# ------------------------------------------------------------------ 9. a query without a bound
@pytest.mark.parametrize("bad", ["nan", "huge"])
def test_a_query_without_a_bound_takes_the_gated_fallback(bad):
    ctx = _ctx()
    dim, n, B = 384, 3000, 40
    rows, q = _ints(n, dim, B, seed=90)
    sig = _signals(n, 90)
    idx = _index(ctx, rows, sig)
    if bad == "nan":
        q[3, 5] = np.nan                                         # every similarity of the query is NaN: it wins nothing
    else:
        q[4] *= np.float32(2.0 ** 60)                            # a norm the screen has no bound for; the scores stay exact
    S = _exact_scores(rows, q)
    t = np.full(B, 10.5, np.float32)
    got, ran, _ = _ran(ctx, lambda: idx.similar_share(q, t, labels=True))
    ref = _ref(S, t, sig)
    _same_both(got, ref)
    assert "share_exact" in ran, ran
    if bad == "nan":
        assert not (got[1] == 3).any()
    else:
        assert int((got[1] == 4).sum()) == int((S[4] >= 10.5).sum()) > 0        # it beats every other candidate of its rows


# ------------------------------------------------------------------ 10. routes agree
def test_routes_agree_bit_for_bit():
    from openintel_amd import _lib
    f = _narr(768, 64)
    rng = np.random.default_rng(5)
    stamp = rng.integers(0, 5, size=f.n).astype(np.uint32)          # bucket 4 does not exist
    kw = dict(n_buckets=4, stamp_origin=0, bucket_width=1)
    ctx = _ctx()
    idx = _index(ctx, f.rows, f.sig, None, stamp)
    a, ran_a, _ = _ran(ctx, lambda: idx.similar_share(f.q, f.t, labels=True, **kw))
    a2, _, _ = _ran(ctx, lambda: idx.similar_share(f.q, f.t, labels=True, **kw))
    ctx_b = _ctx(_lib.OI_COSINE_EXACT)
    view = idx.view(ctx_b)
    b, ran_b, _ = _ran(ctx_b, lambda: view.similar_share(f.q, f.t, labels=True, **kw))
    b2, _, _ = _ran(ctx_b, lambda: view.similar_share(f.q, f.t, labels=True, **kw))
    ctx_c = _ctx()
    bare = _index(ctx_c, f.rows, f.sig, None, stamp, copy=_lib.OI_SCREEN_COPY_NEVER)
    c, ran_c, _ = _ran(ctx_c, lambda: bare.similar_share(f.q, f.t, labels=True, **kw))
    assert ran_a == {"share", "share_band"} and ran_b == {"share_exact"} and ran_c == {"share_exact"}, (ran_a, ran_b, ran_c)
    ref = _ref(f.S, f.t, f.sig, 4, 0, 1, stamp)
    for x in (a, a2, b, b2, c):
        _same_both(x, ref)
        assert x[0].tobytes() == a[0].tobytes() and x[1].tobytes() == a[1].tobytes()
    assert (ref[1][stamp == 4] == NO_LABEL).all() and (ref[1][stamp < 4] != NO_LABEL).any()
    view.close()


# ------------------------------------------------------------------ 11. what the share has in common with the family's other calls
def test_calls_of_the_family_interleave_on_one_context():
    """The band buffer is the family's, the state, best and the pairs' keys are per call: share (labels), summary, share (no
    labels, HIGHER thresholds: a best key left over from the first call would outrank every pair of this one), groups, volume,
    share (labels) on ONE context each give the bytes of the same call on a fresh context."""
    dim, n, B = 384, 2080, 33                                      # two query tiles
    rows, q = _ints(n, dim, B, seed=111)
    S = _exact_scores(rows, q)
    t = ((np.arange(B) % 3) * 20 - 2.5).astype(np.float32)         # -2.5, 17.5, 37.5: most rows have several candidates
    t2 = t + np.float32(20.0)                                      # fewer candidates per row, still several for many
    sig = _signals(n, 111)
    group = (np.arange(n) % 19).astype(np.uint32)                  # keys 16 .. 18 belong to no cell
    stamp = np.zeros(n, np.uint32)
    calls = [("share+", lambda i: i.similar_share(q, t, labels=True)),
             ("summary", lambda i: i.similar_summary(q, t)),
             ("share", lambda i: (i.similar_share(q, t2), np.zeros(0, np.uint32))),
             ("groups", lambda i: i.similar_groups(q, t, 0x1F, 16)),
             ("volume", lambda i: i.similar_volume(q, 17.5)),
             ("share+", lambda i: i.similar_share(q, t, labels=True))]
    ctx = _ctx()
    idx = _index(ctx, rows, sig, group, stamp)
    refs = {"share+": _ref(S, t, sig), "share": _ref(S, t2, sig)}
    moved = (refs["share"][1] != NO_LABEL) & (refs["share"][1] != refs["share+"][1])
    assert moved.any()                         # rows whose winner at t is no candidate at t2, and which another query takes
    for name, call in calls:
        fresh = _ctx()
        view = idx.view(fresh)
        if name.startswith("share"):
            got, ran, fill = _ran(ctx, lambda: call(idx))
            alone, ran_alone, fill_alone = _ran(fresh, lambda: call(view))
            assert ran == ran_alone == {"share", "share_band"} and fill == fill_alone > 0, (name, ran, ran_alone, fill, fill_alone)
            _same(got[0], refs[name][0])
            if name == "share+":
                _same_both(got, refs[name])
            assert got[0].tobytes() == alone[0].tobytes() and got[1].tobytes() == alone[1].tobytes(), name
        else:
            got, alone = call(idx), call(view)
            assert got.dtype == alone.dtype and got.shape == alone.shape and got.tobytes() == alone.tobytes(), name
            assert got.tobytes() != bytes(got.nbytes), name        # (it found something)
        view.close()


def test_the_gated_fallback_without_labels_then_a_screened_call():
    """The fallback's clear has no label array to reset (labels_out == NULL); the next call on the context is screened and right."""
    ctx = _ctx()
    dim, n, B = 384, 3000, 40
    rows, q = _ints(n, dim, B, seed=90)
    sig = _signals(n, 90)
    idx = _index(ctx, rows, sig)
    huge = q.copy()
    huge[4] *= np.float32(2.0 ** 60)                               # a norm the screen has no bound for; the scores stay exact
    t = np.full(B, 10.5, np.float32)
    got, ran, _ = _ran(ctx, lambda: (idx.similar_share(huge, t), np.zeros(0, np.uint32)))
    _same(got[0], _ref(_exact_scores(rows, huge), t, sig)[0])
    assert "share_exact" in ran, ran
    got, ran, _ = _ran(ctx, lambda: idx.similar_share(q, t, labels=True))
    _same_both(got, _ref(_exact_scores(rows, q), t, sig))
    assert "share" in ran and "share_exact" not in ran, ran


# ------------------------------------------------------------------ the host location, with and without its optional output
def test_host_location_with_and_without_labels_is_the_device_location_bit_for_bit():
    """300 rows (a ragged last block of 64), dim 64, 2 queries, 4 buckets: OI_HOST gives OI_DEVICE's bytes, and leaving
    labels_out out leaves the records as they are, in both locations."""
    import torch
    ctx = _ctx()
    n, dim, B, t = 300, 64, 2, 0.5
    rows, q = _ints(n, dim, B, seed=91)
    sig = _signals(n, 91)
    stamp = (1000 + np.arange(n) % 50).astype(np.uint32)           # buckets of 10 from 1000: a fifth of the rows has none
    idx = _index(ctx, rows, sig, np.zeros(n, np.uint32), stamp)
    kw = dict(n_buckets=4, stamp_origin=1000, bucket_width=10)
    dq = torch.from_numpy(q).cuda()
    h_rec, h_lab = idx.similar_share(q, t, labels=True, **kw)
    d_rec, d_lab = idx.similar_share(dq, t, labels=True, **kw)
    ctx.synchronize()
    _same_both((h_rec, h_lab), _ref(_exact_scores(rows, q), t, sig, 4, 1000, 10, stamp))
    assert int(h_rec["total"].sum()) > 0 and (h_lab == NO_LABEL).any()
    assert _host(d_rec).tobytes() == h_rec.tobytes() and _host_labels(d_lab).tobytes() == h_lab.tobytes()
    h_only = idx.similar_share(q, t, **kw)
    d_only = idx.similar_share(dq, t, **kw)
    ctx.synchronize()
    assert h_only.tobytes() == h_rec.tobytes() and _host(d_only).tobytes() == h_rec.tobytes()
