"""The shard contract of the analytics family: every analytics entry point of include/openintel_hip.h ends its
contract with a sentence that tells a sharded host how to get the single-index answer from per-rank calls -- counts of shards
add, records of shards add, labels of shards concatenate, integer sums and counts add before oi_centroids_from_sums, exemplar
lists merge with oi_merge_lists, and a k-means loop over shards is the recipe of oi_narratives_fit's last paragraph.  This
module holds those sentences: the same rows are indexed once as a WHOLE and once as three SHARDS with their own local row 0,
doc_id_base, tile, block, range and window phase, and each test compares three things, with no tolerance anywhere:

    the numpy definition on the whole corpus  ==  the call on the whole index  ==  the host-side composition of the shards.

Records are compared as 8 x 64 bits per cell, counts, labels and doc ids as u32, scores and centroids as their 32 bits.

Corpora (built once per module, see _corpus / _m_corpus):
  E384  f32, dim 384, n = 20 011, finalized (screening copy: the stream route).  Rows and queries are integers in [-8, 8] times
        2^-8: every product is a multiple of 2^-16, every dot product at most 3/8, so each similarity is exact in f32 in any
        order and the f64 restatement of the definition is unambiguous.  The thresholds sit on a half step, (m + 1/2) 2^-16.
        (The recipe of tests/test_gpu_seed.py with the integers four times as large: the screen's margin d 2^-22 |x| |q| is
        then 2.25 steps, so pairs within two steps of the threshold go through the BAND -- with integers up to 2 the margin is
        below the half step and the band stays empty.  The scale 2^-8 keeps a stored row, norm 0.6, below a unit centroid: a
        duplicate seed then loses every row to the centroid that left it.)  Cuts at rows 1 and 16 386: a one-row shard, a shard
        of 16 385 rows and one of 3 625 rows, whose local row 0 lies at phase 1 resp. 2 of the whole's 32-row tiles, 64-row
        blocks, 2 048-row ranges and 16 384-document windows.  A second set of handles puts the whole at doc_id_base
        2^32 - 1 - n.
  F384  the same n and cuts, planted unit-norm float rows and float queries: no numpy oracle, whole and shards are compared with
        each other only -- sim is defined per pair and does not depend on route, batch or grid.
  B384  a bf16 corpus of the E384 recipe, n = 5 003, cuts at 1 and 2 049.
  M     forward index, attributes and signals only, n = 40 001, cuts at 1 and 32 769: the middle shard is exactly one
        32 768-document block, shifted by one row against the whole's block grid.  The shards are finalized as ranks are: with
        the summed n, tokens and df.

The CPU tests (not marked gpu) hold the facts these docstrings claim about the corpora, and show that every comparer fails when
one boundary row's contribution is dropped, doubled or moved to the neighbouring cell."""
import functools
import os
import re

import numpy as np
import pytest

import test_gpu_exemplars as EX
import test_gpu_groups as GR
import test_gpu_label_summary as LS
import test_gpu_mention as MN
import test_gpu_narratives as NV
import test_gpu_seed as SD
import test_gpu_threshold_edges as TE
from test_centroids_abi import SHAPE as CENTROID_SHAPE
from test_exemplars_abi import SHAPE as EXEMPLAR_SHAPE
from test_label_summary_abi import SHAPE as LABEL_SUMMARY_SHAPE

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO = 0xFFFFFFFF
TILE = 32                                   # rows per tile of the threshold family's stream (tests/test_gpu_threshold_edges.py)
DIM, INT_MAX, STEP = 384, 8, 2.0 ** -16     # integers in [-8, 8] times 2^-8; similarities are multiples of STEP
SCALE = np.float32(2.0 ** -8)
T_E = (19 * 1024 + 0.5) * STEP              # the threshold family's threshold on the exact corpora: a half step
T_F = 0.91                                  # ... and on the float corpus: inside the clouds, thousands of pairs within the margin
T_FIT_F = 0.35                              # the fit's on the float corpus (tests/test_gpu_narratives.py's)
T_FIT_E = (5376 + 0.5) * STEP               # the fit's, 0.082: stored rows as seeds reach 0.30, unit centroids 0.52, strangers 0.03 sigma
CUTS = {"E384": (20011, 1, 16386), "F384": (20011, 1, 16386), "B384": (5003, 1, 2049), "M": (40001, 1, 32769)}
C_PLANTED = 5                               # planted centres; the last one has members in the last shard only
K_LAB = 6                                   # clusters of the label tests: 0 .. 4 planted, 5 three rows of the middle shard
FILTERS = TE.FILT1                          # per query: everything | stamps 1 .. 2 | even groups
ONE_FILTER = (1, 0, 0, 3)                   # of the label calls and the fit: even groups, stamps up to 3
COMBOS = [(1, 0), (3, 0), (1, 1), (3, 1)]   # (time buckets, per-query filters): none, buckets, filters, both
FIT_ITERS = 8
SEED_KW = dict(trials=4, seed=11)
ROUTES = {}                                 # (corpus, family, mode, B, handle) -> (profile tags that ran, band fill, flags): printed


def _bounds(name):
    n, c1, c2 = CUTS[name]
    return [(0, c1), (c1, c2), (c2, n)]


# ------------------------------------------------------------------ corpora (CPU)
class _Corpus:
    def sig(self, lo=0, hi=None):
        return TE._Sig(self.sigs.pol[lo:hi], self.sigs.spec[lo:hi], self.sigs.src[lo:hi])


@functools.lru_cache(maxsize=None)
def _corpus(name):
    """-> rows f32 [n, 384], q f32 [64, 384], S: the similarities f32 [64, n] (None on F384), signals, attributes, labels"""
    n, c1, c2 = CUTS[name]
    c = _Corpus()
    c.name, c.n, c.bf16, c.exact = name, n, name == "B384", name != "F384"
    rng = np.random.default_rng({"E384": 384, "F384": 3840, "B384": 16}[name])
    which = np.where(np.arange(n) < c2, rng.integers(0, C_PLANTED - 1, size=n), rng.integers(0, C_PLANTED, size=n))
    c.copies = np.array([0, 1, 2, c2 - 1, c2, c2 + 1, n - 1])       # bit-identical rows on both sides of both cuts
    which[c.copies] = 1
    if c.exact:
        centres = rng.choice(np.array([-INT_MAX, INT_MAX]), size=(C_PLANTED, DIM))
        rows = centres[which].astype(np.int64)
        f = rng.random((n, DIM)) < 0.1
        rows[f] = rng.integers(-INT_MAX, INT_MAX + 1, size=int(f.sum()))
        nz = rng.random(n) < 0.1
        nz[c.copies] = False
        rows[nz] = rng.integers(-INT_MAX, INT_MAX + 1, size=(int(nz.sum()), DIM))
        rows[c.copies] = centres[1]
        q = centres[np.arange(64) % C_PLANTED].astype(np.int64)    # queries: the centres, then centres with 4 .. 12 % redrawn
        f = rng.random((64, DIM)) < (0.04 + 0.08 * rng.random(64))[:, None]
        f[:C_PLANTED] = False
        q[f] = rng.integers(-INT_MAX, INT_MAX + 1, size=int(f.sum()))
        q[63] = q[1]                                               # a repeated query
        S = (q.astype(np.float64) @ rows.astype(np.float64).T) * STEP        # integers below 2^53: exact
        c.S = S.astype(np.float32)
        assert np.array_equal(c.S.astype(np.float64), S) and np.abs(S).max() <= 0.375
        c.rows, c.q, c.centres = rows.astype(np.float32) * SCALE, q.astype(np.float32) * SCALE, centres.astype(np.float32) * SCALE
        assert not (c.rows.view(np.uint32) & 0xFFFF).any() and not (c.q.view(np.uint32) & 0xFFFF).any()      # bf16 values too
    else:
        centres = EX._unit(rng.standard_normal((C_PLANTED, DIM)))
        rows = centres[which] + rng.standard_normal((n, DIM)) * (0.45 / np.sqrt(DIM))
        nz = rng.random(n) < 0.2
        nz[c.copies] = False
        rows[nz] = rng.standard_normal((int(nz.sum()), DIM))
        rows[c.copies] = centres[1]
        q = centres[np.arange(64) % C_PLANTED] + rng.standard_normal((64, DIM)) * (0.3 / np.sqrt(DIM)) * (np.arange(64) >= C_PLANTED)[:, None]
        q[63] = q[1]
        c.rows, c.q, c.centres, c.S = EX._unit(rows).astype(np.float32), EX._unit(q).astype(np.float32), centres.astype(np.float32), None
    c.which = which
    c.sigs = TE._signals(n, len(name) + n)
    c.stamp, c.group = TE._attrs(rng, n)
    c.stamp[c.copies] = 1 + np.arange(c.copies.size) % 3           # the boundary rows have a bucket, a key and pass every filter
    c.group[c.copies] = (2 * (np.arange(c.copies.size) % 4)) | ((np.arange(c.copies.size) % 3) << TE.KEY_SHIFT)
    if c.exact:
        # the leaderboard's trap: the rows query 0 reaches carry keys 0, 2, 0, 2, .. in the middle shard and 1, 2, 1, 2, .. in
        # the last one.  Key 0 leads the one, key 1 the other, and key 2, second in both, leads their sum.
        for (lo, hi), first in zip(_bounds(name)[1:], (0, 1)):
            hit = lo + np.flatnonzero(c.S[0, lo:hi].astype(np.float64) >= T_E)
            key = np.where(np.arange(hit.size) % 2 == 0, first, 2)
            c.group[hit] = (c.group[hit] & ~np.uint32(TE.KEY_MASK)) | (key << TE.KEY_SHIFT).astype(np.uint32)
    # labels of the label calls: the planted cluster; a twentieth each K and 0xFFFFFFFF; cluster 5 is three rows of the middle
    # shard; the copies belong to cluster 1 (so the one-row shard holds cluster 1 alone, and cluster 4 lives in the last shard)
    lab = which.astype(np.uint32)
    r = rng.random(n)
    lab[r < 0.05] = K_LAB
    lab[(r >= 0.05) & (r < 0.10)] = NO
    lab[[c1 + 5, c1 + 700, c2 - 3]] = 5
    lab[c.copies] = 1
    c.lab = lab
    c.cents = np.ascontiguousarray(c.centres[np.arange(K_LAB) % C_PLANTED])
    return c


def _qi(B):
    """the queries of a batch: 3 = (centre 0, centre 4 -- rows of the last shard only --, centre 0 again), 64 = all of them"""
    return np.array([0, 4, 0]) if B == 3 else np.arange(64)


@functools.lru_cache(maxsize=None)
def _m_corpus():
    """M: 2 .. 7 tokens per document.  The first is EVERY (a term of every document), document 0's second is ONLY0 (a term of the
    one-row shard alone), the rest come from tests/test_gpu_mention.py's COMMON."""
    n = CUTS["M"][0]
    rng = np.random.default_rng(40001)
    c = _Corpus()
    c.n, c.EVERY, c.ONLY0 = n, 9, 3777
    lens = rng.integers(2, 8, size=n)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    terms = MN.COMMON[rng.integers(0, MN.COMMON.size, size=int(offs[-1]))]
    terms[offs[:-1].astype(np.int64)] = c.EVERY
    terms[1] = c.ONLY0
    c.fwd = MN._Fwd(terms, offs)
    c.sigs = MN._signals(n, seed=3)
    c.group, c.stamp = MN._attrs(n, seed=3)
    c.queries = [[c.EVERY], [c.ONLY0], [3], [3, 17], [64, 255, 256], [c.EVERY, 3], [c.ONLY0, 17], [1000, 2047, 2048, 3000, 4095],
                 [c.EVERY, c.ONLY0, 3, 3]]
    c.filters = np.array([MN.ALL_DOCS, MN.ALL_DOCS, (0xF, 0x3, 0, 0xFFFFFFFF), (0, 0, 2000, 3000), (0x1, 0x1, 1500, 5500), MN.NO_DOCS,
                          MN.ALL_DOCS, (0, 0, 1000, 1000 + 4999), (0x1, 0x0, 0, 0xFFFFFFFF)], np.uint32)
    return c


def _m_shard(c, lo, hi):
    o = c.fwd.offs.astype(np.int64)
    return MN._Fwd(c.fwd.terms[o[lo]:o[hi]], (o[lo:hi + 1] - o[lo]).astype(np.uint64))


def _m_sig(c, lo, hi):
    return MN._Sig(c.sigs.pol[lo:hi], c.sigs.spec[lo:hi], c.sigs.src[lo:hi])


# ------------------------------------------------------------------ composition and comparison
def _records(x):
    """a result of records on the host: numpy records as they are, an int64 [.., .., 8] tensor as records"""
    if hasattr(x, "data_ptr"):
        a = x.cpu().numpy()
        return a.view(TE._dtype()).reshape(a.shape[0], a.shape[1])
    return x


def _u32(x):
    if hasattr(x, "data_ptr"):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint32)


def _add_records(parts):
    """what a sharded host does with the records of its ranks: the seven integers add as u64, the polarity sums as f64 (each
    is a multiple of 2^-30 below 2^23 in magnitude, so is every partial sum: the f64 addition is exact in any order)"""
    recs = [np.ascontiguousarray(_records(p)) for p in parts]
    words = np.stack([r.view(np.uint64).reshape(r.shape + (8,)) for r in recs])
    out = words.sum(axis=0, dtype=np.uint64)
    pol = np.ascontiguousarray(words[..., 7]).view(np.float64)
    assert (np.abs(pol) < 2.0 ** 23).all()
    out[..., 7] = pol.sum(axis=0).view(np.uint64)
    return np.ascontiguousarray(out).view(TE._dtype()).reshape(recs[0].shape)


def _compose(fam, parts):
    if fam == "volume":
        return np.stack(parts).sum(axis=0, dtype=np.uint64).astype(np.uint32)
    if fam == "share":
        return _add_records([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    return _add_records(parts)


def _same_records(got, ref, what=""):
    TE._same(_records(got), _records(ref))


def _same_u32(got, ref, what=""):
    got, ref = _u32(got), _u32(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = np.flatnonzero(got.ravel() != ref.ravel())
    assert bad.size == 0, (what, bad[:8], got.ravel()[bad[:8]], ref.ravel()[bad[:8]])


def _same_lists(got, ref, what=""):
    """ranked lists (scores, docs, counts): the valid entries of every list, bit for bit"""
    (gs, gd, gc), (rs, rd, rc) = got, ref
    _same_u32(gc, rc, what)
    for q in range(len(rc)):
        m = int(rc[q])
        _same_u32(gd[q, :m], rd[q, :m], (what, q, "docs"))
        _same_u32(gs[q, :m], rs[q, :m], (what, q, "scores"))


def _definition(c, fam, B, nb, filt, lo=0, hi=None, t=T_E):
    """the numpy definition of tests/test_gpu_threshold_edges.py on rows [lo, hi) of an exact corpus"""
    hi = c.n if hi is None else hi
    L = c.S[_qi(B)][:, lo:hi]
    group, stamp = c.group[lo:hi], c.stamp[lo:hi]
    fpass = TE._fpass(B, hi - lo, FILTERS[:B] if filt else None, group, stamp)
    cell, inc, nc = TE._axis(fam, nb, group, stamp)
    return TE._expect(fam, L, t, fpass, cell, inc, nc, c.sig(lo, hi))


def _fam_combos(fam):
    return [(3, 0), (3, 1)] if fam == "groups" else COMBOS        # (the leaderboard's axis is the key: no time buckets)


# ------------------------------------------------------------------ CPU: the facts the docstrings claim
def _header_constant(name):
    with open(os.path.join(ROOT, "include", "openintel_hip.h")) as f:
        return int(re.search(r"#define\s+%s\s+(\d+)u" % name, f.read()).group(1))


def test_every_cut_lies_off_the_tile_block_range_window_and_block_grids():
    from openintel_amd import _lib
    block = {EXEMPLAR_SHAPE["LE_BLOCK_ROWS"], LABEL_SUMMARY_SHAPE["LS_BLOCK_ROWS"], CENTROID_SHAPE["LS_BLOCK_ROWS"], EX.BLOCK}
    rng_rows = {EXEMPLAR_SHAPE["LE_RANGE_ROWS"], LABEL_SUMMARY_SHAPE["LS_RANGE_ROWS"], EX.RANGE, SD.RANGE}
    assert block == {64} and rng_rows == {2048}
    window, docs = _header_constant("OI_BM25_FINE_DOCS"), _header_constant("OI_BM25_BLOCK_DOCS")
    assert (window, docs) == (16384, 32768) and docs == _lib.OI_BM25_BLOCK_DOCS == MN.BLOCK
    for name in ("E384", "F384"):
        n, c1, c2 = CUTS[name]
        assert (c1, c2 - c1, n - c2) == (1, window + 1, 3625)
        for cut, phase in ((c1, 1), (c2, 2)):                       # local row 0 of a shard is row `phase` of the whole's every grid
            assert [cut % g for g in (TILE, 64, 2048, window)] == [phase] * 4
        assert (c2 - c1) % TILE == 1 and (n - c2) % TILE != 0 and (n - c2) % 64 != 0     # ragged last tiles and blocks
    n, c1, c2 = CUTS["B384"]
    assert (c1, c2 - c1) == (1, 2048) and c2 % 2048 == 1 and (n - c2) % 64 != 0
    n, c1, c2 = CUTS["M"]
    assert (c1, c2 - c1) == (1, docs) and c2 % docs == 1 and c2 % window == 1 and n - c2 < docs
    base = 2 ** 32 - 1 - CUTS["E384"][0]
    assert base + CUTS["E384"][0] - 1 == 0xFFFFFFFE                # the last doc id of the high-base pass: one below "no doc"


@pytest.mark.parametrize("name", ["E384", "F384", "B384"])
def test_every_cell_class_is_populated_in_two_shards_and_the_sums_stay_below_2_to_23(name):
    c = _corpus(name)
    (_, _), (a, b), (_, e) = _bounds(name)
    for lo, hi in ((a, b), (b, e)):
        key = (c.group[lo:hi] & TE.KEY_MASK) >> TE.KEY_SHIFT
        assert set(c.stamp[lo:hi].tolist()) == {0, 1, 2, 3, 4}      # stamps 1 .. 3 have a bucket, 0 and 4 have none
        assert set(key.tolist()) == {0, 1, 2, 3, 4}                 # keys 3 and 4 lie at and above n_keys
        assert set((c.group[lo:hi] & 7).tolist()) == set(range(8))  # the filters' bits
        s = c.sig(lo, hi)
        assert len({(bool(x), bool(y), bool(z), bool(w)) for x, y, z, w in zip(s.bull, s.bear, s.sp, s.s1)}) == 12
        assert np.isnan(s.pol).any() and (s.pol == 1.5).any() and (s.pol == -7.0).any()
        lab = c.lab[lo:hi]
        assert (lab == K_LAB).any() and (lab == NO).any()
    assert float(np.abs(c.sigs.q30).sum()) * 2.0 ** -30 < 2.0 ** 23  # no sum of any subset of the rows reaches 2^23
    assert c.lab[0] == 1 and not (c.lab[:b] == 4).any() and (c.lab[b:] == 4).any()       # cluster 4: the last shard only
    assert not (c.lab[:a] == 5).any() and not (c.lab[b:] == 5).any() and int((c.lab == 5).sum()) == 3
    assert c.q[63].tobytes() == c.q[1].tobytes()
    for r in c.copies:
        assert c.rows[r].tobytes() == c.centres[1].tobytes()
    if not c.exact:
        # the float corpus: hundreds of pairs within 1e-3 of the threshold in both large shards, for both batches -- the pairs
        # whose side depends on the f32 chain's value, which no route may change
        s64 = c.q.astype(np.float64) @ c.rows.astype(np.float64).T
        for B in (3, 64):
            for lo, hi in ((a, b), (b, e)):
                assert int((np.abs(s64[_qi(B)][:, lo:hi] - T_F) < 1e-3).sum()) > 100
    if c.exact:
        for B in (3, 64):
            rec, lab = _definition(c, "share", B, 1, 0)
            assert not rec["total"][-1].any()                       # the repeat of an earlier query gets nothing
            hits = c.S[_qi(B)].astype(np.float64) >= T_E
            assert hits[:, a:b].any() and hits[:, b:].any() and (B == 3 or hits[:, :a].any())   # (row 0 is a copy of centre 1)
        rec, lab = _definition(c, "share", 3, 1, 0)
        assert not (lab[:b] == 1).any() and (lab[b:] == 1).sum() > 50      # query 1 of the batch of 3 wins rows in the last shard only
        # the band is not empty by construction: pairs within two steps of the threshold, on both sides, in both large shards
        d = (c.S.astype(np.float64) - T_E) / STEP
        for lo, hi in ((a, b), (b, e)):
            assert ((d[:, lo:hi] > 0) & (d[:, lo:hi] < 2)).any() and ((d[:, lo:hi] < 0) & (d[:, lo:hi] > -2)).any()
        assert np.abs(d - np.rint(d)).min() == 0.5                  # every similarity is half a step or more away from T_E


@pytest.mark.parametrize("name", ["E384", "B384"])
def test_a_key_that_leads_no_shard_leads_the_sum(name):
    c = _corpus(name)
    parts = [_definition(c, "groups", 3, 3, 0, lo, hi) for lo, hi in _bounds(name)]
    leaders = [GR._rank(p, 1, "total", 0)[0][0, 0] for p in parts]
    assert leaders == [NO, 0, 1], leaders                           # (the one-row shard has nothing for query 0)
    assert GR._rank(_compose("groups", parts), 1, "total", 0)[0][0, 0] == 2
    assert GR._rank(_definition(c, "groups", 3, 3, 0), 1, "total", 0)[0][0, 0] == 2


@pytest.mark.parametrize("name", ["E384", "B384"])
@pytest.mark.parametrize("fam", ["volume", "summary", "groups", "share"])
def test_the_definition_composes_and_the_comparers_notice_one_boundary_row(name, fam):
    """On the CPU: the numpy definition of the shards composes to the definition of the whole, and a composition with the
    contribution of the first row of the middle shard dropped, doubled or moved to the neighbouring cell is refused."""
    c = _corpus(name)
    (_, _), (a, b), _ = _bounds(name)
    for nb, filt in _fam_combos(fam):
        whole = _definition(c, fam, 64, nb, filt)
        parts = [_definition(c, fam, 64, nb, filt, lo, hi) for lo, hi in _bounds(name)]
        TE._check(fam, _compose(fam, parts), whole, "composition")
        one = _definition(c, fam, 64, nb, filt, a, a + 1)           # what row `a` alone contributes (a copy of centre 1)
        tot = one if fam == "volume" else (one[0] if fam == "share" else one)["total"]
        assert tot.sum() >= 1, (fam, nb, filt)
        zero = _definition(c, fam, 64, nb, filt, a, a + 1, t=1.0)    # (nothing reaches 1: the same shapes, all zero)
        moved = (np.roll(one[0], 1, axis=0), one[1]) if fam == "share" else np.roll(one, 1, axis=0)     # to the next query's cell
        rest = _definition(c, fam, 64, nb, filt, a + 1, b)

        def middle(extra):
            """the middle shard as the contributions `extra` of its first row and the rest of its rows (the labels stay right)"""
            if fam == "share":
                return _add_records([x[0] for x in extra] + [rest[0]]), np.concatenate([one[1], rest[1]])
            return _compose(fam, extra + [rest])

        TE._check(fam, _compose(fam, [parts[0], middle([one]), parts[2]]), whole, "row by row")
        for what, extra in (("dropped", [zero]), ("doubled", [one, one]), ("moved", [moved])):
            with pytest.raises(AssertionError):
                TE._check(fam, _compose(fam, [parts[0], middle(extra), parts[2]]), whole, what)
        if fam == "share":                                          # and a label moved across the cut
            lab = _compose(fam, parts)[1].copy()
            lab[a] = whole[1][a + 1] if whole[1][a + 1] != whole[1][a] else NO
            with pytest.raises(AssertionError):
                TE._check(fam, (whole[0], lab), whole, "label")


def test_the_other_comparers_notice_one_changed_entry():
    c = _corpus("B384")
    rec = _definition(c, "summary", 3, 3, 0)
    for field in ("total", "spec_count", "polarity_sum"):
        bad = rec.copy()
        bad[field][0, 1] += 1
        with pytest.raises(AssertionError):
            _same_records(bad, rec)
    bad = rec.copy()
    bad["polarity_sum"][0, 0] = -0.0 if rec["polarity_sum"][0, 0] == 0 else np.nextafter(rec["polarity_sum"][0, 0], 9e9)
    with pytest.raises(AssertionError):
        _same_records(bad, rec)                                     # one bit of the f64
    with pytest.raises(AssertionError):
        _same_u32(np.array([1, 2, 3], np.uint32), np.array([1, 2, 4], np.uint32))
    with pytest.raises(AssertionError):
        _same_u32(np.array([0.0], np.float32), np.array([-0.0], np.float32))
    ref = EX._reference(c.rows, c.lab, c.cents, 9)
    _same_lists(ref, ref)
    for i, delta in ((0, np.float32(STEP)), (1, 1), (2, 1)):
        bad = [x.copy() for x in ref]
        bad[i][(1, 3) if i < 2 else 1] += delta
        with pytest.raises(AssertionError):
            _same_lists(bad, ref)
    # the ranking: the whole's list against the sum of two of the three shards (another key leads it)
    from openintel_amd.retriever import GroupRanking
    dense = [_definition(c, "groups", 3, 3, 0, lo, hi) for lo, hi in _bounds("B384")]
    for mod in (GR, LS):
        ranked = GroupRanking(*mod._rank(_compose("groups", dense), 1, "total", 0))
        mod._same_ranking(ranked, _compose("groups", dense), 1, "total", 0)
        with pytest.raises(AssertionError):
            mod._same_ranking(ranked, _compose("groups", dense[:2]), 1, "total", 0)
    # the sums of label_sums: dropping the boundary row of the middle shard changes a sum and a count
    (_, _), (a, b), _ = _bounds("B384")
    sums, counts = NV._label_sums(c.rows, c.lab, K_LAB)
    parts = [NV._label_sums(c.rows[lo:hi], c.lab[lo:hi], K_LAB) for lo, hi in ((0, a), (a + 1, b), (b, c.n))]
    assert not np.array_equal(sum(p[0] for p in parts), sums) and not np.array_equal(sum(p[1] for p in parts), counts)
    parts[1] = NV._label_sums(c.rows[a:b], c.lab[a:b], K_LAB)
    assert np.array_equal(sum(p[0] for p in parts), sums) and np.array_equal(sum(p[1] for p in parts), counts)


def test_mention_corpus_facts_and_composition_on_the_cpu():
    c = _m_corpus()
    (_, a), (_, b), (_, e) = _bounds("M")
    assert c.fwd.has(c.EVERY).all() and np.flatnonzero(c.fwd.has(c.ONLY0)).tolist() == [0]
    assert float(np.abs(c.sigs.q30).sum()) * 2.0 ** -30 < 2.0 ** 23
    mm = np.array([1, 1, 1, 0, 2, 1, 0, 3, 0], np.uint32)
    kw = dict(n_cells=5, origin=1000, width=1000)
    whole = MN._ref(c.fwd, c.queries, c.sigs, mm, group=c.group, stamp=c.stamp, filters=c.filters, **kw)
    parts = [MN._ref(_m_shard(c, lo, hi), c.queries, _m_sig(c, lo, hi), mm, group=c.group[lo:hi], stamp=c.stamp[lo:hi],
                     filters=c.filters, **kw) for lo, hi in _bounds("M")]
    _same_records(_add_records(parts), whole)
    assert int(whole["total"][1].sum()) == 1 and int(parts[0]["total"][1].sum()) == 1     # ONLY0: the one-row shard's
    short = MN._ref(_m_shard(c, a + 1, b), c.queries, _m_sig(c, a + 1, b), mm, group=c.group[a + 1:b], stamp=c.stamp[a + 1:b],
                    filters=c.filters, **kw)
    with pytest.raises(AssertionError):
        _same_records(_add_records([parts[0], short, parts[2]]), whole)                   # the block's first document dropped


def _emulated_seeds(c):
    ref = SD._emulate(c.rows, 5, **SEED_KW)
    assert ref["found"] == 5
    return np.concatenate([ref["seeds"], ref["seeds"][1:2]])          # plus one duplicate seed


@pytest.mark.parametrize("filtered", [False, True])
def test_the_fit_on_the_exact_corpus_has_no_decision_near_a_tie(filtered):
    """What makes the f64 emulation of tests/test_gpu_narratives.py a reference for E384: after step 1 (exact) no similarity
    comes within 1e-4 of the threshold or of the runner-up, and the loop moves rows, converges and stops before max_iters."""
    c = _corpus("E384")
    elig = NV._eligible(c.group, c.stamp, ONE_FILTER, 3, 1, 1) if filtered else None
    ref = NV._emulate(c.rows, _emulated_seeds(c), T_FIT_E, FIT_ITERS, eligible=elig)
    assert not ref["risky"].any(), int(ref["risky"].sum())
    assert 3 <= ref["iterations"] < FIT_ITERS and ref["converged"], (ref["iterations"], ref["converged"])
    assert 0 < ref["assigned"] < c.n and not (ref["labels"] == 5).any()      # the duplicate seed stays empty
    _, a, b = CUTS["E384"]
    assert len(set(ref["labels"][a:b].tolist())) >= 4 and len(set(ref["labels"][b:].tolist())) >= 4


# ------------------------------------------------------------------ GPU: the handles
class _Handles:
    pass


def _build(ctx, c, lo, hi, base, plain=False):
    import openintel_amd as oi
    n = hi - lo
    idx = oi.HybridIndex(ctx, n, DIM, 8, doc_id_base=base)
    if c.bf16:
        idx.set_embeddings_bf16((c.rows[lo:hi].view(np.uint32) >> 16).astype(np.uint16))
    else:
        idx.set_embeddings(c.rows[lo:hi], normalize=False)
    if plain:                                                       # (the exemplars need nothing else)
        return idx
    idx.set_doc_attrs(c.group[lo:hi], c.stamp[lo:hi])
    idx.set_signals(c.sigs.pol[lo:hi], c.sigs.spec[lo:hi], c.sigs.src[lo:hi], TE.TAU)
    idx.set_forward(np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64))
    idx.finalize()
    return idx


@pytest.fixture(scope="module")
def handles():
    """name -> the whole index and its three shards (doc_id_base = first global row) on a default context, their views on an
    OI_COSINE_EXACT context, and a second set at the high base.  Built at first use, shared, never changed, closed at the end."""
    from openintel_amd import _lib
    made = {}

    def get(name):
        if name not in made:
            c = _corpus(name)
            h = _Handles()
            h.c, h.ctx, h.ctx_x = c, TE._ctx(), TE._ctx(_lib.OI_COSINE_EXACT)
            h.whole = _build(h.ctx, c, 0, c.n, 0)
            h.shards = [_build(h.ctx, c, lo, hi, lo) for lo, hi in _bounds(name)]
            h.whole_x = h.whole.view(h.ctx_x)
            h.shards_x = [s.view(h.ctx_x) for s in h.shards]
            h.base = 2 ** 32 - 1 - c.n
            h.whole_hi = _build(h.ctx, c, 0, c.n, h.base, plain=True)
            h.shards_hi = [_build(h.ctx, c, lo, hi, h.base + lo, plain=True) for lo, hi in _bounds(name)]
            made[name] = h
        return made[name]

    yield get
    for h in made.values():
        for idx in h.shards_x + [h.whole_x] + h.shards + [h.whole] + h.shards_hi + [h.whole_hi]:
            idx.close()
        h.ctx_x.close()
        h.ctx.close()


def _slices(name, x):
    return [x[lo:hi] for lo, hi in _bounds(name)]


# ------------------------------------------------------------------ 1. volume, summary, groups, share
@gpu
@pytest.mark.parametrize("fam", ["volume", "summary", "groups", "share"])
@pytest.mark.parametrize("name", ["E384", "F384", "B384"])
def test_threshold_family_shards_add_to_the_whole(handles, name, fam):
    h = handles(name)
    c = h.c
    t = T_E if c.exact else T_F
    for B in (3, 64):
        q = np.ascontiguousarray(c.q[_qi(B)])
        for mode, ctx, whole, shards in (("default", h.ctx, h.whole, h.shards), ("exact", h.ctx_x, h.whole_x, h.shards_x)):
            for nb, filt in _fam_combos(fam):
                filters = FILTERS[:B] if filt else None
                what = "%s %s B=%d %s nb=%d filt=%d" % (name, fam, B, mode, nb, filt)
                got, ran, fill, flags = TE._ran(ctx, fam, lambda: TE._call(fam, whole, q, t, filters, nb))
                ROUTES[(name, fam, mode, B, "whole")] = (sorted(ran), fill, flags)
                parts = []
                for i, s in enumerate(shards):
                    p, ran_s, fill_s, flags_s = TE._ran(ctx, fam, lambda: TE._call(fam, s, q, t, filters, nb))
                    ROUTES[(name, fam, mode, B, "shard %d" % i)] = (sorted(ran_s), fill_s, flags_s)
                    parts.append(p)
                sums = _compose(fam, parts)
                TE._check(fam, sums, got, what + ": shards against whole")
                if c.exact:
                    TE._check(fam, got, _definition(c, fam, B, nb, filt), what + ": whole against numpy")
                if fam == "share":
                    assert [p[1].size for p in parts] == [hi - lo for lo, hi in _bounds(name)]
                    assert filt or not got[0]["total"][-1].any(), what     # the repeated query (same threshold, same filter)
                    if c.exact and B == 3:
                        assert not (sums[1][:_bounds(name)[2][0]] == 1).any() and (parts[2][1] == 1).any(), what
                if fam == "groups":
                    for top, by, min_total in ((1, "total", 0), (2, "spec", 0), (3, "bullish", 2), (2, "bearish", 0), (3, "total", 40)):
                        ranked = whole.similar_groups(q, t, TE.KEY_MASK, TE.N_KEYS, top=top, rank_by=by, min_total=min_total, filters=filters)
                        GR._same_ranking(ranked, sums, top, by, min_total)
                    if c.exact and not filt:
                        own = [int(s.similar_groups(q, t, TE.KEY_MASK, TE.N_KEYS, top=1).keys[0, 0]) for s in shards]
                        assert own == [NO, 0, 1] and int(whole.similar_groups(q, t, TE.KEY_MASK, TE.N_KEYS, top=1).keys[0, 0]) == 2, own
                if mode == "exact":
                    assert ran == {fam + "_exact"}, (what, ran)
                elif not c.bf16 and B == 64:
                    # the whole and the 16 385-row shard took the stream, and their bands were not empty
                    for who in ("whole", "shard 1"):
                        tags, fill_w, flags_w = ROUTES[(name, fam, mode, B, who)]
                        assert fam in tags and fam + "_band" in tags and fam + "_exact" not in tags and fill_w > 0 and flags_w == 0, (what, who, tags, fill_w, flags_w)
    for k in sorted(k for k in ROUTES if k[:2] == (name, fam)):
        print("route", k, ROUTES[k])


# ------------------------------------------------------------------ 2. mention
@gpu
def test_mention_records_of_document_shards_add():
    import openintel_amd as oi
    c = _m_corpus()
    ctx = TE._ctx()

    def build(lo, hi):
        idx = oi.HybridIndex(ctx, hi - lo, 8, MN.VOCAB, doc_id_base=lo)
        f = _m_shard(c, lo, hi)
        idx.set_forward(f.terms, f.offs)
        idx.set_doc_attrs(c.group[lo:hi], c.stamp[lo:hi])
        idx.set_signals(c.sigs.pol[lo:hi], c.sigs.spec[lo:hi], c.sigs.src[lo:hi], MN.TAU)
        return idx

    whole = build(0, c.n)
    whole.finalize()
    shards = [build(lo, hi) for lo, hi in _bounds("M")]
    stats = [s.local_stats() for s in shards]                       # the all-reduce of a sharded host
    tokens, df = sum(s[0] for s in stats), np.stack([s[1] for s in stats]).sum(axis=0, dtype=np.uint64).astype(np.uint32)
    assert (tokens, df.tolist()) == (whole.local_stats()[0], whole.local_stats()[1].tolist())
    for s in shards:
        s.finalize(c.n, tokens, df)
    qt, qo = MN._pack(c.queries)
    time_kw = dict(n_buckets=5, stamp_origin=1000, bucket_width=1000)
    ref_kw = dict(n_cells=5, origin=1000, width=1000)
    for mm in (None, "all", np.array([1, 1, 1, 0, 2, 1, 0, 3, 0], np.uint32), 2):
        for filters in (None, c.filters):
            f_kw = dict(group=c.group, stamp=c.stamp, filters=filters)
            for call, ref in ((lambda i: i.mention_summary(qt, qo, min_match=mm, filters=filters, **time_kw),
                               lambda: MN._ref(c.fwd, c.queries, c.sigs, mm, **ref_kw, **f_kw)),
                              (lambda i: i.mention_summary(qt, qo, min_match=mm, filters=filters),
                               lambda: MN._ref(c.fwd, c.queries, c.sigs, mm, **f_kw)),
                              (lambda i: i.mention_groups(qt, qo, 0x1FF, 300, min_match=mm, filters=filters),
                               lambda: MN._ref(c.fwd, c.queries, c.sigs, mm, n_cells=300, key_mask=0x1FF, **f_kw))):
                got = call(whole)
                parts = [call(s) for s in shards]
                _same_records(_add_records(parts), got)
                _same_records(got, ref())
                if mm is None and filters is None:
                    assert int(got["total"][0].sum()) <= c.n and int(parts[0]["total"][1].sum()) == 1       # ONLY0: the one-row shard's
                    assert int(parts[1]["total"][1].sum()) == 0 and int(parts[2]["total"][1].sum()) == 0
    assert int(whole.mention_summary(qt, qo)["total"][0, 0]) == c.n  # EVERY: every document, once
    for idx in shards + [whole]:
        idx.close()
    ctx.close()


# ------------------------------------------------------------------ 3. label_sums -> centroids
@gpu
@pytest.mark.parametrize("name", ["E384", "F384", "B384"])
def test_label_sums_of_shards_add_and_the_centroids_of_the_total_are_the_whole_s(handles, name):
    from openintel_amd.retriever import centroids_from_sums
    h = handles(name)
    c = h.c
    sums, counts = h.whole.label_sums(c.lab, K_LAB)
    parts = [s.label_sums(lab, K_LAB) for s, lab in zip(h.shards, _slices(name, c.lab))]
    tot_s = np.stack([p[0] for p in parts]).sum(axis=0, dtype=np.int64)
    tot_c = np.stack([p[1] for p in parts]).sum(axis=0, dtype=np.uint64)
    assert tot_s.tobytes() == sums.tobytes() and tot_c.tobytes() == counts.tobytes()
    assert [int(p[1][4]) for p in parts[:2]] == [0, 0] and int(parts[2][1][4]) > 0 and parts[0][1].tolist() == [0, 1, 0, 0, 0, 0]
    assert int(counts[5]) == 3 and int(counts.sum()) == int((c.lab < K_LAB).sum())
    ref_s, ref_c = NV._label_sums(c.rows, c.lab, K_LAB)              # (fix() is exact integer arithmetic on any f32 value)
    if c.exact:
        assert sums.tobytes() == ref_s.tobytes() and counts.tobytes() == ref_c.tobytes()
    previous = np.random.default_rng(5).standard_normal((K_LAB + 1, DIM)).astype(np.float32)
    # (a seventh cluster that nobody belongs to: it keeps `previous`)
    s7, c7 = h.whole.label_sums(c.lab, K_LAB + 1)
    p7 = [s.label_sums(lab, K_LAB + 1) for s, lab in zip(h.shards, _slices(name, c.lab))]
    t7_s, t7_c = np.stack([p[0] for p in p7]).sum(axis=0, dtype=np.int64), np.stack([p[1] for p in p7]).sum(axis=0, dtype=np.uint64)
    assert int(c7[K_LAB]) == int((c.lab == K_LAB).sum()) > 0         # (label K is a cluster now, K + 1 .. and 0xFFFFFFFF are not)
    a = centroids_from_sums(h.ctx, t7_s, t7_c, previous)
    b = centroids_from_sums(h.ctx, s7, c7, previous)
    assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
    lab8 = np.where(c.lab == K_LAB, NO, c.lab).astype(np.uint32)     # and with an empty cluster in the middle of the table
    s8, c8 = h.whole.label_sums(lab8, K_LAB + 1)
    p8 = [s.label_sums(lab, K_LAB + 1) for s, lab in zip(h.shards, _slices(name, lab8))]
    t8_s, t8_c = np.stack([p[0] for p in p8]).sum(axis=0, dtype=np.int64), np.stack([p[1] for p in p8]).sum(axis=0, dtype=np.uint64)
    a, b = centroids_from_sums(h.ctx, t8_s, t8_c, previous), centroids_from_sums(h.ctx, s8, c8, previous)
    assert a.tobytes() == b.tobytes() and a[K_LAB].tobytes() == previous[K_LAB].tobytes() and int(c8[K_LAB]) == 0
    if c.exact:
        assert a.tobytes() == NV._centroids(*NV._label_sums(c.rows, lab8, K_LAB + 1), previous).tobytes()


# ------------------------------------------------------------------ 4. label_summary / label_groups
@gpu
def test_label_summary_records_of_shards_add_and_the_rank_of_the_sum_is_the_whole_s(handles):
    h = handles("E384")
    c = h.c
    sig = c.sig()
    labs = _slices("E384", c.lab)
    for filt in (None, ONE_FILTER):
        for kw, ref in ((dict(n_buckets=3, stamp_origin=1, bucket_width=1), LS._ref_time(c.lab, K_LAB, sig, c.stamp, 1, 1, 3, filt, c.group)),
                        (dict(), LS._ref_time(c.lab, K_LAB, sig, c.stamp, 0, 0, 1, filt, c.group))):
            got = h.whole.label_summary(c.lab, K_LAB, filter=filt, **kw)
            parts = [s.label_summary(lab, K_LAB, filter=filt, **kw) for s, lab in zip(h.shards, labs)]
            _same_records(_add_records(parts), got)
            _same_records(got, ref)
        dense = h.whole.label_groups(c.lab, K_LAB, TE.KEY_MASK, TE.N_KEYS, filter=filt)
        parts = [s.label_groups(lab, K_LAB, TE.KEY_MASK, TE.N_KEYS, filter=filt) for s, lab in zip(h.shards, labs)]
        sums = _add_records(parts)
        _same_records(sums, dense)
        _same_records(dense, LS._ref_key(c.lab, K_LAB, sig, c.group, TE.KEY_MASK, TE.N_KEYS, filt, c.stamp))
        assert not parts[0]["total"][[0, 2, 3, 4, 5]].any() and int(parts[0]["total"][1].sum()) == 1
        assert not parts[1]["total"][4].any() and parts[2]["total"][4].any() and not parts[2]["total"][5].any()
        for top, by, min_total in ((1, "total", 0), (2, "spec", 0), (3, "bullish", 0), (2, "bearish", 3), (3, "total", 1200)):
            LS._same_ranking(h.whole.label_groups(c.lab, K_LAB, TE.KEY_MASK, TE.N_KEYS, top=top, rank_by=by, min_total=min_total, filter=filt),
                             sums, top, by, min_total)


# ------------------------------------------------------------------ 5. label_exemplars
@gpu
@pytest.mark.parametrize("name", ["E384", "B384"])
def test_exemplar_lists_of_three_shards_merge_to_the_whole_s_at_both_bases(handles, name):
    from openintel_amd import retriever
    h = handles(name)
    c = h.c
    labs = _slices(name, c.lab)
    for base, whole, shards in ((0, h.whole, h.shards), (h.base, h.whole_hi, h.shards_hi)):
        for top in (3, 12, 200):
            ref = EX._reference(c.rows, c.lab, c.cents, top, base=base)
            got = EX._got(whole.label_exemplars(c.lab, c.cents, top=top))
            EX._same(got, ref, "%s whole base %d top %d" % (name, base, top))
            parts = [EX._got(s.label_exemplars(lab, c.cents, top=top)) for s, lab in zip(shards, labs)]
            assert parts[0][2].tolist() == [0, 1, 0, 0, 0, 0]        # the one-row shard: one list of one entry
            assert parts[1][2][4] == 0 and parts[2][2][5] == 0 and parts[2][2][4] == min(top, int((c.lab == 4).sum()))
            merged = retriever.merge_lists(h.ctx, np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]),
                                           np.stack([p[2] for p in parts]))
            _same_lists(merged, got, "%s merged base %d top %d" % (name, base, top))
            _same_lists(merged, ref)
            # ties across both cuts: the copies of centre 1 share the best score and are listed by global doc id
            want = (c.copies[:min(top, c.copies.size)] + base).tolist()
            assert merged[1][1, :len(want)].tolist() == want and len(set(merged[0][1, :len(want)].tolist())) == 1
            assert int(merged[1].max()) <= 0xFFFFFFFF and (base == 0 or int(merged[1][1, 0]) == base)
    assert c.copies[-1] + h.base == 0xFFFFFFFE


# ------------------------------------------------------------------ 6. the sharded fit
def _sharded_fit(ctx, shards, seeds, t, max_iters, filt=None, dev=False, **axis):
    """oi_narratives_fit's loop built from the public calls over document shards, as its header paragraph prescribes:
    similar_share per shard (labels concatenate, records add), label_sums per shard (sums and counts add),
    centroids_from_sums(previous = c_i), `moved` counted by the host.  dev: every array stays on the device, added with torch."""
    from openintel_amd.retriever import centroids_from_sums
    K = seeds.shape[0]
    kw = dict(axis)
    if filt is not None:
        kw["filters"] = np.array([filt] * K, np.uint32)
    if dev:
        import torch
        c = torch.from_numpy(np.ascontiguousarray(seeds)).cuda()
        torch.cuda.synchronize()
    else:
        c = np.ascontiguousarray(seeds)
    prev, i = None, 0
    while True:
        i += 1
        out = [s.similar_share(c, t, labels=True, **kw) for s in shards]
        if dev:
            ctx.synchronize()
            lab = torch.cat([o[1] for o in out])
            words = torch.stack([o[0] for o in out])
            rec = torch.cat([words[..., :7].sum(dim=0), words[..., 7].contiguous().view(torch.float64).sum(dim=0).view(torch.int64).unsqueeze(-1)], dim=-1)
            assigned = int((lab != -1).sum().item())
            moved = assigned if prev is None else int((lab != prev).sum().item())
        else:
            lab = np.concatenate([o[1] for o in out])
            rec = _add_records([o[0] for o in out])
            assigned = int((lab != NO).sum())
            moved = assigned if prev is None else int((lab != prev).sum())
        converged = i > 1 and moved == 0
        if converged or i == max_iters:
            break
        parts = [s.label_sums(o[1], K) for s, o in zip(shards, out)]
        if dev:
            ctx.synchronize()
            sums, counts = torch.stack([p[0] for p in parts]).sum(dim=0), torch.stack([p[1] for p in parts]).sum(dim=0)
            torch.cuda.synchronize()
        else:
            sums = np.stack([p[0] for p in parts]).sum(axis=0, dtype=np.int64)
            counts = np.stack([p[1] for p in parts]).sum(axis=0, dtype=np.uint64)
        c = centroids_from_sums(ctx, sums, counts, c)
        prev = lab
    if dev:
        ctx.synchronize()
    return dict(centroids=c, records=rec, labels=lab, iterations=i, converged=converged, moved=moved, assigned=assigned)


def _same_fit(got, fit, what):
    assert (got["iterations"], got["converged"], got["moved"], got["assigned"]) == (fit.iterations, fit.converged, fit.moved, fit.assigned), \
        (what, got["iterations"], got["converged"], got["moved"], got["assigned"], fit.iterations, fit.converged, fit.moved, fit.assigned)
    _same_u32(got["labels"], fit.labels, what + " labels")
    _same_u32(got["centroids"], fit.centroids, what + " centroids")
    _same_records(got["records"], fit.records, what + " records")


@gpu
@pytest.mark.parametrize("name", ["E384", "F384"])
def test_a_fit_looped_over_shards_with_the_public_calls_is_fit_narratives_on_the_whole(handles, name):
    import torch
    h = handles(name)
    c = h.c
    t = T_FIT_E if c.exact else T_FIT_F
    found = h.whole.seed_narratives(5, **SEED_KW)
    assert found.found == 5
    seeds = np.concatenate([found.seeds, found.seeds[1:2]])          # the seeds of the whole, and one duplicate
    if c.exact:
        assert seeds.tobytes() == _emulated_seeds(c).tobytes()
    buckets = dict(n_buckets=3, stamp_origin=1, bucket_width=1)
    for what, filt, axis in (("plain", None, {}), ("filter and buckets", ONE_FILTER, buckets)):
        fit = h.whole.fit_narratives(seeds, t, max_iters=FIT_ITERS, filter=filt, labels=True, **axis)
        got = _sharded_fit(h.ctx, h.shards, seeds, t, FIT_ITERS, filt=filt, **axis)
        print(name, what, "iterations", fit.iterations, "converged", fit.converged, "moved", fit.moved, "assigned", fit.assigned)
        _same_fit(got, fit, "%s %s" % (name, what))
        assert fit.iterations >= 2 and not (fit.records["total"][5].any() and c.exact)      # E384: the duplicate seed stays empty
        # (on unit rows the copy competes from step 2 on as the vector seed 1 was, and may win rows: in whole and shards alike)
        if c.exact:
            elig = NV._eligible(c.group, c.stamp, filt, 3, 1, 1) if filt else None
            ref = NV._emulate(c.rows, seeds, t, FIT_ITERS, eligible=elig)
            assert not ref["risky"].any()
            assert (fit.iterations, fit.converged, fit.moved, fit.assigned) == (ref["iterations"], ref["converged"], ref["moved"], ref["assigned"])
            _same_u32(fit.labels, ref["labels"], "emulation labels")
            _same_u32(fit.centroids, ref["centroids"], "emulation centroids")
            nb = axis.get("n_buckets", 1)
            _same_records(fit.records, LS._ref_time(ref["labels"], 6, c.sig(), c.stamp, axis.get("stamp_origin", 0), axis.get("bucket_width", 0), nb))
    # once in the device location: queries, records, labels, sums and centroids stay on the device and are added with torch
    fit = h.whole.fit_narratives(seeds, t, max_iters=FIT_ITERS, labels=True)
    got = _sharded_fit(h.ctx, h.shards, seeds, t, FIT_ITERS, dev=True)
    assert got["centroids"].is_cuda and got["labels"].is_cuda and got["records"].is_cuda
    _same_fit(got, fit, "%s device" % name)
    dfit = h.whole.fit_narratives(torch.from_numpy(seeds).cuda(), t, max_iters=FIT_ITERS, labels=True)
    _same_fit(got, dfit, "%s device against device" % name)
