"""The threshold family (oi_volume.h: similar_volume, similar_summary, similar_groups, similar_share) at every band-staging,
band-capacity, query-slice, winner and row-width edge of its kernels.

One construction serves every stream-route test.  Query q is the unit vector e_q; row r holds level(q, r) in coordinate q and
a constant ballast in its last coordinate; every value is bf16-exact.  The MFMA screen score, the f32 chain score and the exact
similarity of a pair are then the same number, level(q, r), and the screen's margin is set by the ballast alone (the rows'
rounding error E is 0, which also keeps the long-row class off).  A pair whose level equals the threshold t sits in the band
and is rescored to a hit, t - 2^-10 sits in the band and is rescored to a miss, 0 is a proven miss and a level far above t a
proven hit; every test asserts these zones against the margin idx.screen_probe reports, never against a constant.  Tiles are
dealt round-robin to waves (wave 4 block + w owns tiles first, first + W, ..; W = 4 x 7/8 of the CUs), so the band pairs of
one wave's consecutive tiles can be planted exactly.

The reference is numpy in this file: the three clauses of the definition (and the winner rule of the share) applied to the
level matrix in f64 / int64, records compared as 8 x 64 bits per cell, labels and counts as u32.  Every stream-route case also
reads the call's state (ctx.profile_read("<family>_state")): the band fill must equal the planted number of undecided pairs,
both flags must be 0, <family>_band ran and <family>_exact did not -- the intended branch ran, not only the right answer came
out.  Every case runs again at nextafter(t), where every band pair is a miss, and on a context in OI_COSINE_EXACT mode."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ALL = (0, 0, 0, 0xFFFFFFFF)
NONE = (0, 0, 7, 6)
TAU = 0.2
INF = float("inf")
NO_LABEL = 0xFFFFFFFF
VALS = np.array([-1.0, -0.5, -1.0 / 3.0, -0.2, 0.0, 0.2, 0.25, 1.0 / 3.0, 1.0, np.nan, 1.5, -7.0])
MISS = 2.0 ** -10                        # a band pair this far below t is rescored to a miss
BALLAST = {384: 16.0, 768: 8.0}          # margin ~ 1.001 dim 2^-22 ballast = 1.47e-3 at both dims: MISS < margin, 2 margin < 1/64
BAND_CAP = 4 << 20
KW3 = dict(n_buckets=3, stamp_origin=1, bucket_width=1)      # stamps 1, 2, 3 have a bucket; 0 and 4 have none
KEY_MASK, KEY_SHIFT, N_KEYS = 0x70, 4, 3                     # keys 0 .. 4 are drawn: 3 and 4 belong to no cell


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


def _index(ctx, rows, sig=None, group=None, stamp=None, finalize=True, bf16=False):
    """finalize=True gives an f32 corpus of dim 384 / 768 its bf16 screening copy (the stream route)"""
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
    if finalize:
        idx.set_forward(np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64))
        idx.finalize()
    return idx


_WAVES = []


def _waves():
    """W: the waves of the stream kernel's persistent grid once the corpus has a tile for each (7/8 of the CUs, 4 waves each)"""
    if not _WAVES:
        ctx = _ctx()
        cus = int(ctx.profile_read("screen_width")[1])
        ctx.close()
        assert cus >= 8, cus
        _WAVES.append(4 * (cus * 7 // 8))
    return _WAVES[0]


# ------------------------------------------------------------------ the calls
def _call(fam, idx, q, thr, filters, nb=3):
    kw = KW3 if nb == 3 else {}
    if fam == "volume":
        return idx.similar_volume(q, thr, filters=filters, **kw)
    if fam == "summary":
        return idx.similar_summary(q, thr, filters=filters, **kw)
    if fam == "groups":
        return idx.similar_groups(q, thr, KEY_MASK, N_KEYS, filters=filters)
    return idx.similar_share(q, thr, filters=filters, labels=True, **kw)


def _ran(ctx, fam, call):
    """(result, the family's profile tags with a launch that did its work, band fill, flags: 1 = gate, 2 = overflow) of a call"""
    ctx.profile_reset(True)
    out = call()
    ran = {t for t in (fam, fam + "_band", fam + "_exact") if ctx.profile_read(t)[1] > 0}
    fill, flags = ctx.profile_read(fam + "_state")
    ctx.profile_reset(False)
    return out, ran, int(fill), int(flags)


# ------------------------------------------------------------------ the definition, in numpy
def _fpass(B, n, filters, group, stamp):
    """clause 1: [B][n], row r passes filters[q]"""
    out = np.ones((B, n), bool)
    if filters is not None:
        for q in range(B):
            m, v, lo, hi = (int(x) for x in filters[q])
            out[q] = ((group & np.uint32(m)) == np.uint32(v)) & (stamp >= np.uint32(lo)) & (stamp <= np.uint32(hi))
    return out


def _axis(fam, nb, group, stamp):
    """clause 2: (the cell of a row on the family's second axis, whether it has one, cells per query)"""
    n = stamp.size
    if fam == "groups":
        key = ((group.astype(np.int64) & KEY_MASK) >> KEY_SHIFT)
        return key, key < N_KEYS, N_KEYS
    if nb == 1:
        return np.zeros(n, np.int64), np.ones(n, bool), 1
    s64 = stamp.astype(np.int64)
    b = (s64 - KW3["stamp_origin"]) // KW3["bucket_width"]
    return b, (s64 >= KW3["stamp_origin"]) & (b < KW3["n_buckets"]), KW3["n_buckets"]


def _thr(t, B):
    return np.broadcast_to(np.asarray(t, dtype=np.float64), (B,))


def _records(qs, rs, cell, B, nc, sig):
    """records [B][nc]: pair i adds the signals of row rs[i] to cell (qs[i], cell[rs[i]])"""
    out = np.zeros((B, nc), _dtype())
    flat = qs.astype(np.int64) * nc + cell[rs]

    def count(m):
        return np.bincount(flat[m], minlength=B * nc).reshape(B, nc)

    out["total"] = count(np.ones(flat.size, bool))
    out["by_source"][:, :, 1] = count(sig.s1[rs])
    out["by_source"][:, :, 0] = out["total"] - out["by_source"][:, :, 1]
    out["bullish"], out["bearish"], out["neutral"] = count(sig.bull[rs]), count(sig.bear[rs]), count(sig.neu[rs])
    out["spec_count"] = count(sig.sp[rs])
    s = np.zeros(B * nc, np.int64)
    np.add.at(s, flat, sig.q30[rs])
    out["polarity_sum"] = s.reshape(B, nc).astype(np.float64) * 2.0 ** -30       # |s| < 2^53: the conversion is exact
    return out


def _expect(fam, L, t, fpass, cell, inc, nc, sig):
    """The definition on the level matrix L [B][n] (f32 values, compared in f64): counts u32 [B][nc] (volume), records
    [B][nc] (summary, groups) or (records, labels u32 [n]) (share: the largest level wins, ties to the smallest query)."""
    B, n = L.shape
    with np.errstate(invalid="ignore"):
        cand = (L >= _thr(t, B)[:, None]) & fpass                # (a NaN threshold is nobody's)
    if fam == "share":
        win = np.argmax(np.where(cand, L, -INF), axis=0)         # the first maximum: ties go to the smallest q
        labels = np.where(cand.any(axis=0) & inc, win, NO_LABEL).astype(np.uint32)
        rs = np.flatnonzero(labels != NO_LABEL)
        return _records(labels[rs], rs, cell, B, nc, sig), labels
    qs, rs = np.nonzero(cand & inc[None, :])
    if fam == "volume":
        return np.bincount(qs * nc + cell[rs], minlength=B * nc).reshape(B, nc).astype(np.uint32)
    return _records(qs, rs, cell, B, nc, sig)


def _same(got, ref):
    """all eight fields bit for bit (the f64 sum included: compared as its 64 bits)"""
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    a = np.ascontiguousarray(got).view(np.uint64).reshape(-1, 8)
    b = np.ascontiguousarray(ref).view(np.uint64).reshape(-1, 8)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, (bad[:4], got.reshape(-1)[bad[:2]], ref.reshape(-1)[bad[:2]])


def _check(fam, got, ref, what):
    if fam == "volume":
        assert got.dtype == np.uint32 and got.shape == ref.shape, (what, got.dtype, got.shape)
        bad = np.flatnonzero(got.ravel() != ref.ravel())
        assert bad.size == 0, (what, bad[:8], got.ravel()[bad[:8]], ref.ravel()[bad[:8]])
    elif fam == "share":
        _same(got[0], ref[0])
        assert got[1].dtype == np.uint32 and got[1].shape == ref[1].shape, what
        bad = np.flatnonzero(got[1] != ref[1])
        assert bad.size == 0, (what, bad[:8], got[1][bad[:8]], ref[1][bad[:8]])
    else:
        _same(got, ref)


# ------------------------------------------------------------------ the construction
class _Built:
    """An index over a level matrix, its queries, the margin the screen reports and an OI_COSINE_EXACT view of it."""

    def __init__(self, L, dim, stamp, group, seed):
        from openintel_amd import _lib
        B, n = L.shape
        assert B < dim - 1 and L.dtype == np.float32
        rows = np.zeros((n, dim), np.float32)
        rows[:, :B] = L.T
        rows[:, dim - 1] = BALLAST[dim]
        assert not (rows.view(np.uint32) & 0xFFFF).any()          # every value is bf16-exact
        self.q = np.zeros((B, dim), np.float32)
        self.q[np.arange(B), np.arange(B)] = 1.0
        self.L, self.B, self.n, self.dim, self.stamp, self.group = L, B, n, dim, stamp, group
        self.sig = _signals(n, seed)
        self.ctx = _ctx()
        self.idx = _index(self.ctx, rows, self.sig, group, stamp)
        assert self.idx.long_rows() == 0
        self.eps = self.idx.screen_probe(self.q)[1].astype(np.float64)
        assert (self.eps > 0).all() and np.isfinite(self.eps).all()
        self.ctx_x = _ctx(_lib.OI_COSINE_EXACT)
        self.view = self.idx.view(self.ctx_x)

    def close(self):
        self.view.close()
        self.idx.close()
        self.ctx_x.close()
        self.ctx.close()

    def zones(self, t):
        """(band, proven hit) [B][n] at thresholds t, from the margin the library reports.  The test's own precondition: every
        level is either inside the margin of its query's threshold (undecided by the screen) or more than twice the margin
        away (proven), so neither depends on how the margin is rounded."""
        tq = _thr(t, self.B)
        with np.errstate(invalid="ignore"):
            d = self.L.astype(np.float64) - tq[:, None]
            e = self.eps[:, None]
            band, hit, miss = np.abs(d) < e, d > 2 * e, d < -2 * e
        assert (band | hit | miss | np.isnan(tq)[:, None]).all()
        return band, hit

    def to_band(self, fam, t, fpass, inc):
        """[B][n]: the pairs the stream leaves undecided.  A non-exclusive tally: lo <= s < hi behind filter, cell and long-row
        test.  The share: every bit (s >= lo, behind the filter) of a row that is not a proven sole candidate."""
        band, hit = self.zones(t)
        if fam != "share":
            return band & fpass & inc[None, :]
        bits = (band | hit) & fpass
        sole = (bits.sum(axis=0) == 1) & ((hit & fpass).sum(axis=0) == 1)
        return bits & ~sole[None, :]


_SLOT = {}


def _cached(key, make):
    """one construction alive at a time: built at the first case that needs it, shared by the cases that follow, never changed"""
    if key not in _SLOT:
        for old in list(_SLOT.values()):
            old.close()
        _SLOT.clear()
        _SLOT[key] = make()
    return _SLOT[key]


def _per_tile(m):
    """band pairs per 32-row tile of a [B][n] mask"""
    per_row = m.sum(axis=0)
    pad = (-per_row.size) % 32
    return np.concatenate([per_row, np.zeros(pad, per_row.dtype)]).reshape(-1, 32).sum(axis=1)


def _attrs(rng, n):
    """stamps 0 .. 4 and groups {key 0 .. 4 in bits 4 .. 6, three low bits for the filters}, different from row to row"""
    stamp = rng.integers(0, 5, size=n).astype(np.uint32)
    group = (rng.integers(0, 8, size=n) | (rng.integers(0, 5, size=n) << KEY_SHIFT)).astype(np.uint32)
    return stamp, group


def _up(t):
    return float(np.nextafter(np.float32(t), np.float32(INF)))


def _stream_and_exact(b, fam, t, filters, fpass, nb, what, per_query=False):
    """The three runs of a stream-route case: at t (fill, flags, route), at nextafter(t) and on the exact route."""
    cell, inc, nc = _axis(fam, nb, b.group, b.stamp)
    runs = [t] if per_query else [t, _up(t)]
    for thr in runs:
        want_fill = int(b.to_band(fam, thr, fpass, inc).sum())
        got, ran, fill, flags = _ran(b.ctx, fam, lambda: _call(fam, b.idx, b.q, thr, filters, nb))
        print("%s thr=%r: band fill %d (planted %d), flags %d, ran %s" % (what, thr if not per_query else "per query", fill,
                                                                          want_fill, flags, sorted(ran)))
        _check(fam, got, _expect(fam, b.L, thr, fpass, cell, inc, nc, b.sig), (what, "stream"))
        assert fill == want_fill and flags == 0, (what, fill, want_fill, flags)
        assert fam in ran and fam + "_band" in ran and fam + "_exact" not in ran, (what, ran)
    got, ran, _, _ = _ran(b.ctx_x, fam, lambda: _call(fam, b.view, b.q, t, filters, nb))
    _check(fam, got, _expect(fam, b.L, t, fpass, cell, inc, nc, b.sig), (what, "exact"))
    assert ran == {fam + "_exact"}, (what, ran)


# ------------------------------------------------------------------ 1. band staging classes
# Band pairs per tile of ONE wave, over its consecutive tiles.  Class c is planted at level (c + 1) / 64 into the tiles of wave c
# (c, c + W, c + 2 W): the threshold selects the class, every other class is then a cluster of proven hits or proven misses in
# other waves' tiles.  OI_STAGE = 256 staged pairs per wave, a flush at 64, the sparse path up to 192 pairs per tile.
CLASSES = [(1,), (2,), (3,), (5,),            # the band kernel's c % 4 tail (no background: the band holds exactly these)
           (192, 192),                        # three flushes, then staging from st_head = 192 across the wrap at 256
           (191, 130),                        # a wrap with a remainder
           (63, 0),                           # no flush until the end
           (64, 0),                           # one exact flush, nothing left
           (65, 0),                           # a flush and one pair left for the final flush
           (192,), (193,),                    # the last sparse tile and the first dense one
           (2048,),                           # a full tile (dense): every pair of the tile (32 rows x B)
           (63, 193, 1),                      # a dense tile while 63 pairs sit staged, then sparse again
           (193, 64),                         # a dense tile followed by a sparse one
           ()]                                # nothing at this level: a call whose band stays empty
NO_BACKGROUND = (0, 1, 2, 3, 14)
FILT1 = np.array([(ALL, (0, 0, 1, 2), (1, 0, 0, 0xFFFFFFFF))[q % 3] for q in range(64)], dtype=np.uint32)


def _spread(rng, ok, k):
    """k cells (q, slot) of ok [B][32], dealt round-robin over the 32 row slots (= 16 registers x 2 half-waves), the query
    drawn at random within the slot"""
    lists = [list(rng.permutation(np.flatnonzero(ok[:, s]))) for s in range(32)]
    assert sum(len(x) for x in lists) >= k, (sum(len(x) for x in lists), k)
    order, out, i = rng.permutation(32), [], 0
    while len(out) < k:
        s = int(order[i % 32])
        i += 1
        if lists[s]:
            out.append((int(lists[s].pop()), s))
    return out


def _stage_levels(fam, B, W, n, stamp, group, filters, rng):
    n_tiles = (n + 31) // 32
    full = CLASSES.index((2048,))
    for c in range(len(CLASSES)):                                # the classes' tiles: every row has a bucket and a key, so that
        for j in range(3):                                       # every row slot can carry band pairs; the filters still differ
            r = np.arange(32 * (c + j * W), 32 * (c + j * W) + 32)
            stamp[r] = 1 + rng.integers(0, 3, size=32)
            group[r] = rng.integers(0, 8, size=32) | (rng.integers(0, 3, size=32) << KEY_SHIFT)
    r = np.arange(32 * full, 32 * full + 32)                     # the full tile: rows that every filter keeps as well
    stamp[r] = 1 + r % 2
    group[r] = (2 * (r % 4)) | ((r % 3) << KEY_SHIFT)
    fpass = _fpass(B, n, filters, group, stamp)
    _, inc, _ = _axis(fam, 3, group, stamp)
    counted = fpass if fam == "share" else fpass & inc[None, :]  # (the stream evaluates the share's clause 2 at the assignment)
    L = np.zeros((B, n), np.float32)
    class_tile = np.zeros(n_tiles, bool)
    for c, seq in enumerate(CLASSES):
        lvl = (c + 1) / 64.0
        for j in range(3):
            T = c + j * W
            class_tile[T] = True
            k = min(seq[j], 32 * B) if j < len(seq) else 0
            ok = counted[:, 32 * T:32 * T + 32]
            for q, s in _spread(rng, ok, k):
                L[q, 32 * T + s] = lvl - (MISS if k < 32 * B and rng.random() < 0.33 else 0.0)
            if 0 < k < 32 * B:
                # band levels on pairs the filter or the axis rejects: never part of the fill.  Proven hits beside them (not
                # for the share, whose rows would then have a second candidate and go to the band whole)
                for q, s in np.argwhere(~ok)[rng.permutation(int((~ok).sum()))[:3]]:
                    L[q, 32 * T + s] = lvl
                if fam != "share":
                    free = np.argwhere(L[:, 32 * T:32 * T + 32] == 0)
                    for q, s in free[rng.permutation(len(free))[:24]]:
                        L[q, 32 * T + s] = 1.0
    # the other waves: 0 .. 3 band pairs per tile and class, so that the global claims interleave; proven hits everywhere
    others = np.flatnonzero((np.arange(n_tiles) % W >= 16) & ~class_tile)
    for c in range(len(CLASSES)):
        if c in NO_BACKGROUND:
            continue
        cnt = rng.integers(0, 4, size=others.size)
        for i in range(3):
            T = others[cnt > i]
            q, rr = rng.integers(0, B, size=T.size), 32 * T + rng.integers(0, 32, size=T.size)
            q, rr = q[rr < n], rr[rr < n]
            ok = L[q, rr] == 0                                   # (wherever: a pair the filter or the axis rejects is not in the fill)
            L[q[ok], rr[ok]] = (c + 1) / 64.0 - MISS * (rng.random(int(ok.sum())) < 0.33)
    T = others[rng.integers(0, others.size, size=3000)]
    q, rr = rng.integers(0, B, size=T.size), 32 * T + rng.integers(0, 32, size=T.size)
    ok = rr < n
    ok[ok] = L[q[ok], rr[ok]] == 0
    L[q[ok], rr[ok]] = np.where(rng.random(int(ok.sum())) < 0.5, 1.0, 0.5)
    return L.astype(np.float32), fpass


class _Stage:
    pass


def _stage(fam, dim, B, filt):
    def make():
        W = _waves()
        n = 32 * (2 * W + 16) + 7                                # every wave below 16 owns three tiles; a ragged last tile
        rng = np.random.default_rng(dim + B + 7 * filt + len(fam))
        stamp, group = _attrs(rng, n)
        filters = FILT1[:B] if filt else None
        L, fpass = _stage_levels(fam, B, W, n, stamp, group, filters, rng)
        s = _Built(L, dim, stamp, group, seed=dim + B)
        s.W, s.filters, s.fpass = W, filters, fpass
        return s
    return _cached(("stage", fam, dim, B, filt), make)


STAGE_CONFIGS = [("volume", dim, B, filt) for dim in (384, 768) for B in (32, 64) for filt in (0, 1)] + \
                [("summary", 768, 64, 1), ("groups", 384, 64, 1), ("share", 384, 64, 1)]


@pytest.mark.parametrize("fam,dim,B,filt,c", [cfg + (c,) for cfg in STAGE_CONFIGS for c in range(len(CLASSES))])
def test_band_staging_classes(fam, dim, B, filt, c):
    s = _stage(fam, dim, B, filt)
    seq, t, W = CLASSES[c], (c + 1) / 64.0, s.W
    _, inc, _ = _axis(fam, 3, s.group, s.stamp)
    tb = s.to_band(fam, t, s.fpass, inc)
    per_tile = _per_tile(tb)
    # the class reaches its branch: the pairs the wave's consecutive tiles send to the band, against 64 / 192 / 256
    want = [min(seq[j], 32 * B) if j < len(seq) else 0 for j in range(3)]
    assert [int(per_tile[c + j * W]) for j in range(3)] == want, (seq, [int(per_tile[c + j * W]) for j in range(3)])
    if c in NO_BACKGROUND:
        # the band kernel sees exactly this many pairs (the share's band also holds the rows with two proven candidates)
        assert int(tb.sum()) == sum(seq) or fam == "share"
    else:
        rest = np.delete(per_tile, [c + j * W for j in range(3)])
        assert rest.max() <= 3 or fam == "share", rest.max()      # (the share sends rows with two proven candidates too)
        assert int((rest > 0).sum()) > 300
    for j in range(3):
        if 63 <= want[j] < 32 * B:                                # every register, both half-waves, both query tiles
            m = tb[:, 32 * (c + j * W):32 * (c + j * W) + 32]
            assert m.any(axis=0).all() and m[:32].any() and (B == 32 or m[32:].any())
    assert s.zones(t)[1].any()                                    # proven hits beside the band
    _stream_and_exact(s, fam, t, s.filters, s.fpass, 3, "%s d=%d B=%d filt=%d class %r" % (fam, dim, B, filt, seq))


# ------------------------------------------------------------------ 2. the band at its capacity
def _cap(n):
    def make():
        dim, B = 384, 64
        rows = np.zeros((n, dim), np.float32)
        rows[:, 0] = 0.5
        rows[:, 1] = (np.arange(n) % 97) / 256.0                  # bf16-exact: screen score = sim = 0.5 exactly
        s = _Stage()
        s.q = np.zeros((B, dim), np.float32)
        s.q[:, 0] = 1.0
        s.sig = _signals(n, 7, vals=np.array([-1.0, -1.0 / 3.0, -0.2, 0.0, 0.25]))
        s.ctx = _ctx()
        s.idx = _index(s.ctx, rows, s.sig)
        assert s.idx.long_rows() == 0
        s.close = lambda: (s.idx.close(), s.ctx.close())
        return s
    return _cached(("cap", n), make)


@pytest.mark.parametrize("n,fam", [(65536, "volume"), (65536, "share"), (65537, "volume"), (65537, "share")])
def test_the_band_exactly_full_and_one_row_over(n, fam):
    """64 copies of e_0 against rows[:, 0] = 0.5: every pair is undecided at t = 0.5.  65 536 rows fill the 4 Mi pairs of the
    band exactly (no overflow, no fallback); one row more is cap + 64 pairs, the overflow flag and the gated fallback.  For
    the share all 64 queries tie, so every row goes to query 0: the commit kernel's own clamp and the fallback's label clear."""
    B = 64
    s = _cap(n)
    assert B * 65536 == BAND_CAP
    zeros, ones = np.zeros(n, np.int64), np.ones(n, bool)

    def ref(t):
        return _expect(fam, np.full((B, n), 0.5, np.float32), t, np.ones((B, n), bool), zeros, ones, 1, s.sig)

    full = ref(0.5)
    if fam == "volume":
        assert (full == n).all()
    else:
        assert (full[1] == 0).all() and int(full[0]["total"][0, 0]) == n and full[0]["polarity_sum"][0, 0] < -1000.0
    got, ran, fill, flags = _ran(s.ctx, fam, lambda: _call(fam, s.idx, s.q, 0.5, None, 1))
    print("%s n=%d t=0.5: band fill %d, flags %d, ran %s" % (fam, n, fill, flags, sorted(ran)))
    _check(fam, got, full, (fam, n, 0.5))
    assert fill == B * n and fam in ran and fam + "_band" in ran, (fill, ran)
    if n == 65536:
        assert fill == BAND_CAP and flags == 0 and fam + "_exact" not in ran, (fill, flags, ran)
        got, ran, fill, flags = _ran(s.ctx, fam, lambda: _call(fam, s.idx, s.q, _up(0.5), None, 1))
        _check(fam, got, ref(_up(0.5)), (fam, n, "nextafter"))
        assert not (got if fam == "volume" else got[0]["total"]).any()
        assert fill == BAND_CAP and flags == 0 and fam + "_exact" not in ran, (fill, flags, ran)
    else:
        assert fill == BAND_CAP + 64 and flags == 2 and fam + "_exact" in ran, (fill, flags, ran)
    got, ran, fill, flags = _ran(s.ctx, fam, lambda: _call(fam, s.idx, s.q, 0.75, None, 1))      # a following call sees clean state
    _check(fam, got, ref(0.75), (fam, n, 0.75))
    assert not (got if fam == "volume" else got[0]["total"]).any() and (fam == "volume" or (got[1] == NO_LABEL).all())
    assert fill == 0 and flags == 0 and fam in ran and fam + "_exact" not in ran, (fill, flags, ran)


# ------------------------------------------------------------------ 3. the exclusive epilogue, slot by slot
# The candidate sets a row slot can hold, and the pairs each sends to the band (filters on, filters off).
KINDS = ["sole proven", "sole at t", "sole at t - 2^-10", "q and q + 32 proven, different levels", "q and q + 32 proven, equal levels",
         "two lanes of one tile", "proven + band miss", "the better candidate's filter rejects the row", "a winner without a bucket"]
KIND_PAIRS = {1: (0, 1, 1, 2, 2, 2, 2, 0, 0), 0: (0, 1, 1, 2, 2, 2, 2, 2, 0)}
T3 = 0.25
FILT3 = np.array([(0, 0, 1, 2) if q % 2 else (ALL if q % 4 == 0 else (1, 0, 0, 0xFFFFFFFF)) for q in range(64)], dtype=np.uint32)


def _slots(B, v):
    def make():
        W = _waves()
        n = 32 * (W + 1) + 17                                     # wave 0 has a second tile (W); the last tile is ragged
        rng = np.random.default_rng(300 + B + v)
        stamp, group = _attrs(rng, n)
        L = np.zeros((B, n), np.float32)
        kinds = {}
        for T in (0, W):
            for slot in range(32):
                r = 32 * T + slot
                kind = (slot + v + (4 if T else 0)) % 9
                if B == 32 and kind in (3, 4):
                    kind = 5                                      # (no second query tile)
                kinds[r] = kind
                qa = (5 * slot + 3 * v + (T > 0)) % 32
                up = 32 if B == 64 and slot % 2 else 0            # the set sits in the second query tile at every other slot
                stamp[r], group[r] = 1 + slot % 2, 2 * (slot % 4) | ((slot % 5) << KEY_SHIFT)      # passes every filter
                if kind == 0:
                    L[qa + up, r] = 0.5 if slot % 4 < 2 else 1.0
                elif kind == 1:
                    L[qa + up, r] = T3
                elif kind == 2:
                    L[qa + up, r] = T3 - MISS
                elif kind == 3:
                    L[qa, r], L[qa + 32, r] = (0.5, 1.0) if slot % 4 < 2 else (1.0, 0.5)
                elif kind == 4:
                    L[qa, r] = L[qa + 32, r] = 0.75
                elif kind == 5:
                    L[qa + up, r], L[(qa + 7) % 32 + up, r] = (0.5, 1.0) if slot % 4 < 2 else (1.0, 0.5)
                elif kind == 6:
                    L[qa + up, r], L[(qa + 11) % 32 + (32 - up if B == 64 else 0), r] = 1.0, T3 - MISS
                elif kind == 7:
                    L[(qa | 1) + up, r], L[(qa & ~3) + (32 - up if B == 64 else 0), r] = 1.0, 0.5     # an odd query: stamps 1 .. 2 only
                    stamp[r] = 3
                else:
                    L[(qa & ~3) + up, r] = 1.0                    # (a query that takes every row)
                    stamp[r] = 4 if slot % 2 else 0
        rest = np.setdiff1d(np.arange(n), np.concatenate([np.arange(32), np.arange(32 * W, 32 * W + 32)]))
        rr = rest[rng.integers(0, rest.size, size=2500)]          # the other tiles: every kind of level, wherever
        L[rng.integers(0, B, size=rr.size), rr] = rng.choice(np.array([T3, T3 - MISS, 0.5, 0.75, 1.0], np.float32), size=rr.size)
        L[3, n - 1], L[B - 1, n - 1], L[5, n - 17], L[B - 2, n - 2] = T3, 1.0, 0.5, T3 - MISS       # the ragged tile's ends
        s = _Stage()
        s.L, s.stamp, s.group, s.W, s.kinds, s.built = L, stamp, group, W, kinds, {}
        s.close = lambda: [b.close() for b in s.built.values()]
        return s
    return _cached(("slots", B, v), make)


@pytest.mark.parametrize("B,v", [(B, v) for B in (64, 32) for v in range(9)])
def test_exclusive_epilogue_slot_by_slot(B, v):
    """similar_share(labels=True): every one of the 32 row slots of tiles 0 and W (both wave 0's) holds each candidate set of
    KINDS in turn (v rotates them), at both dims, filters off and on, 1 and 3 buckets."""
    s = _slots(B, v)
    W, n = s.W, s.L.shape[1]
    mine = np.concatenate([np.arange(32), np.arange(32 * W, 32 * W + 32)])
    assert {s.kinds[r] for r in mine} == (set(range(9)) - {3, 4} if B == 32 else set(range(9)))
    for dim in (384, 768):
        b = s.built[dim] = _Built(s.L, dim, s.stamp, s.group, seed=v)
        for filt in (0, 1):
            filters = FILT3[:B] if filt else None
            fpass = _fpass(B, n, filters, s.group, s.stamp)
            for nb in (1, 3):
                cell, inc, nc = _axis("share", nb, s.group, s.stamp)
                tb = b.to_band("share", T3, fpass, inc)
                assert int(tb[:, mine].sum()) == sum(KIND_PAIRS[filt][s.kinds[r]] for r in mine)    # the sum of pairs over the sets
                ref = _expect("share", s.L, T3, fpass, cell, inc, nc, b.sig)
                for r in mine:                                    # the sets decide what the definition says they decide
                    k, lab = s.kinds[r], int(ref[1][r])
                    if k in (2,) or (k == 8 and nb == 3):
                        assert lab == NO_LABEL, (k, lab)
                    elif k in (3, 5, 6) or (k == 7 and not filt):
                        assert lab == int(np.argmax(s.L[:, r])) and s.L[lab, r] == 1.0, (k, lab)
                    elif k == 4:
                        assert lab < 32 and s.L[lab, r] == s.L[lab + 32, r] == 0.75, (k, lab)
                    elif k == 7:
                        assert s.L[lab, r] == 0.5, (k, lab)
                    else:
                        assert lab != NO_LABEL, (k, lab)
                _stream_and_exact(b, "share", T3, filters, fpass, nb, "share slots B=%d v=%d d=%d filt=%d nb=%d" % (B, v, dim, filt, nb))
        b.close()
        del s.built[dim]


# ------------------------------------------------------------------ 4. query slices
FILT4 = np.array([(ALL, (0, 0, 1, 2), NONE, (1, 0, 0, 0xFFFFFFFF), (0, 0, 2, 3))[q % 5] for q in range(129)], dtype=np.uint32)


def _slices(dim, B):
    def make():
        W = _waves()
        n = 32 * (W + 1) + 5
        rng = np.random.default_rng(400 + dim + B)
        stamp, group = _attrs(rng, n)
        L = np.zeros((B, n), np.float32)
        for q in range(B):                                        # every query its own pattern, over all the tiles
            rr = rng.permutation(n)[:30]
            L[q, rr[:12]] = T3
            L[q, rr[12:18]] = T3 - MISS
            L[q, rr[18:]] = np.where(rng.random(12) < 0.5, 0.5, 1.0)
        s = _Built(L, dim, stamp, group, seed=dim + B)
        s.filters = FILT4[:B]
        return s
    return _cached(("slices", dim, B), make)


@pytest.mark.parametrize("dim,B", [(384, 64), (384, 65), (384, 96), (384, 97), (384, 128), (384, 129), (768, 129)])
def test_query_slices(dim, B):
    """More than 64 queries run as slices of 64 (the last one with one or two query tiles): band pairs carry q_base + 32 t + li,
    every per-query argument and the cells are sliced.  Volume takes one threshold, summary and groups one per query."""
    s = _slices(dim, B)
    choices = np.array([T3, -INF, _up(T3), T3, INF, np.nan], np.float32)
    thr = choices[(np.arange(B) + 4) % 6]                         # (the single query of a third slice, 128, has t)
    band, hit = s.zones(thr)
    for q0 in range(0, B, 64):
        assert band[q0:q0 + 64].any() and hit[q0:q0 + 64].any()   # every slice carries band pairs and proven hits
    for filt in (0, 1):
        filters = s.filters if filt else None
        fpass = _fpass(B, s.n, filters, s.group, s.stamp)
        _stream_and_exact(s, "volume", T3, filters, fpass, 3, "volume slices d=%d B=%d filt=%d" % (dim, B, filt))
        _stream_and_exact(s, "summary", thr, filters, fpass, 3, "summary slices d=%d B=%d filt=%d" % (dim, B, filt), per_query=True)
    if B == 129:
        fpass = _fpass(B, s.n, s.filters, s.group, s.stamp)
        key, inc, _ = _axis("groups", 3, s.group, s.stamp)
        assert (~inc).any() and inc.any()                         # some rows have keys >= n_keys
        _stream_and_exact(s, "groups", thr, s.filters, fpass, 3, "groups slices d=%d B=%d" % (dim, B), per_query=True)


# ------------------------------------------------------------------ 5. exact route widths
# vo_exact_kernel holds a row in NV = ceil(dim / 256) float4 per lane and guards the last with v < nvec: dims on either side of
# every NV boundary.  The planted coordinate and the query's coordinate lie in the row's LAST float4; coordinate 0 of every row
# and every query is set too, so a float4 read past the row's end (the next row's, the next query's first) changes the score.
@pytest.mark.parametrize("kind,dim", [("f32", d) for d in (252, 256, 260, 508, 512, 516, 764, 772, 1020, 1024)] +
                         [("bf16", d) for d in (384, 768, 1024)])      # (a bf16 corpus has dim 384, 768 or 1024)
def test_exact_route_row_widths(kind, dim):
    levels = np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32)
    ctx = _ctx()
    for B in (1, 3, 4, 5):
        for n in (1, 3, 4, 5, 333):
            qi, ri = np.arange(B)[:, None], np.arange(n)[None, :]
            L = levels[(3 * qi + 5 * ri + qi * ri + dim) % 5]
            coord = [dim - 1 - q if q < 4 else dim - 5 for q in range(B)]       # query 4: the last lane of the float4 before
            rows = np.zeros((n, dim), np.float32)
            q = np.zeros((B, dim), np.float32)
            rows[:, 0], q[:, 0] = 2.0, 1.0
            for b in range(B):
                rows[:, coord[b]] = L[b]
                q[b, coord[b]] = 1.0
            S = (q.astype(np.float64) @ rows.astype(np.float64).T).astype(np.float32)         # 2 + level: exact
            assert np.array_equal(S, 2.0 + L)
            stamp = (np.arange(n) % 5).astype(np.uint32)
            group = np.zeros(n, np.uint32)
            sig = _signals(n, dim + B)
            data = (rows.view(np.uint32) >> 16).astype(np.uint16) if kind == "bf16" else rows
            idx = _index(ctx, data, sig, group, stamp, finalize=False, bf16=kind == "bf16")
            fpass = np.ones((B, n), bool)
            for fam in ("volume", "share"):
                cell, inc, nc = _axis(fam, 3, group, stamp)
                for t in (2.5, _up(2.5)):
                    got, ran, _, _ = _ran(ctx, fam, lambda: _call(fam, idx, q, t, None, 3))
                    _check(fam, got, _expect(fam, S, t, fpass, cell, inc, nc, sig), (kind, dim, B, n, fam, t))
                    assert ran == {fam + "_exact"}, ran
            idx.close()
    ctx.close()
