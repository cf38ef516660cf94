"""The int8 screen appends a tile's survivors from what the tile test kept (csrc/cosine_screen_i8.hip): the edges.

A lane of cosine_i8_screen holds, per tile, 16 rows x NQT queries: query 32 t + li and the rows (r & 3) + 8 (r >> 2) + 4 lh of the
tile, lane = li + 32 lh.  A test that passes leaves its s~ and e_r in two registers of the lane; when NO lane of the wave tested
more than one pair in (before the ragged mask and the filter take bits away) the survivors are staged from those registers, one
pair per lane, at the lane's rank among the lanes that have one.  Every other tile (a lane with two pairs, and so every dense
tile) takes the path that reads the sums and the metadata again.  What this can get wrong is silent: a key made from a pair the
mask dropped or from the tile before, a lane's second pair lost, staging positions that collide, a flush in the middle of an
append that loses what was behind it.  Each case plants the winners of some queries where such a defect changes the lists and
compares the int8 route with the f32-stream screen (bit for bit) and with the f64 oracle, gate shut, as
tests/test_gpu_screen_i8_deferred.py does; geometry, background and runner are that module's.

A plant is a list of (row of the tile, queries): the row is put near the mean of those queries and made orthogonal to every
other query of the batch, so it passes for exactly those (score ~ 0.95 / sqrt(len(queries)), every other query's ~ 0 against
thresholds of 0.1 and more).  `lane_pairs` gives the pairs each lane then holds; the host-side test below checks the table of
plants against the capacities it is meant to straddle.  (Which path a tile took is not observable from outside the kernel: the
plants are what puts a tile on one side of an edge, the lists are what a wrong path changes.)"""
from collections import Counter

import numpy as np
import pytest

from test_gpu_screen_i8_deferred import (STAGE_DIRECT, Case, O, background, geometry, near, num_cus, queries, run,  # noqa: F401
                                         stream_ctx)
from test_gpu_screen_i8_edges import MI355X_CUS, TILE, VOCAB, _forward, _index, check_oracle, listed, plan, wave_tiles

STAGE_FLUSH = 64            # oi_lds_dma.h: OI_STAGE_FLUSH, the staged pairs that leave for the pool at once

CASES = {c.name: c for c in [
    Case("pairs-d384", 384, 33, 10, 5, 0, True),
    Case("pairs-d768", 768, 33, 10, 5, 0, False),
    Case("pairs-nqt1", 768, 9, 10, 5, 0, True),
    Case("consecutive-d384", 384, 33, 10, 5, 0, True),
    Case("consecutive-d768", 768, 9, 10, 5, 0, False),
    Case("last-tiles-12", 384, 9, 10, 3, 0, True),
    Case("last-tiles-23", 768, 33, 10, 5, 0, False),
    Case("direct-d384", 384, 33, 10, 5, 0, True),
    Case("direct-d768", 768, 33, 10, 5, 0, False),
    Case("ring-d384", 384, 33, 10, 5, 0, True),
    Case("ring-d768", 768, 33, 10, 5, 0, False),
    Case("ragged-12", 384, 33, 10, 5, 12, True),
    Case("ragged-31", 768, 9, 10, 5, 31, False),
    Case("filtered", 384, 33, 10, 5, 0, True),
]}

G6 = [list(range(1 + 6 * i, 7 + 6 * i)) for i in range(4)]     # four groups of six queries, none 32 apart from another

# ---- the plants, per tile: (row of the tile, queries)
ONE_PAIR = [(2, [3])]                                   # one lane, one pair
TWO_QUERIES_ONE_LANE = [(2, [0, 32])]                   # queries 32 apart share a lane: query tiles 0 and 1 of one register row
TWO_ROWS_ONE_LANE = [(2, [5]), (3, [5])]                # two rows of one register half (lh = 0)
TWO_ROWS_TWO_LANES = [(2, [6]), (6, [6])]               # the same query in both halves: two lanes, a pair each
ONE_AND_TWO = [(9, [7]), (12, [8]), (13, [8])]          # a lane at one beside a lane at two
TWO_ROWS_ONE_LANE_NQT1 = [(17, [4]), (19, [4])]
FULL_192 = [(r, list(range(6))) for r in range(TILE)]   # 32 rows x 6 queries: exactly what a wave stages
OVER_193 = [(0, list(range(7)))] + FULL_192[1:]         # one pair more, in a lane of its own: straight to the pool
OVER_194 = [(0, list(range(7))), (1, list(range(7)))] + FULL_192[2:]    # that lane at two
RING_48 = [(r, G6[r]) for r in range(4)] + [(4 + r, G6[r]) for r in range(4)]   # 48 lanes, a pair each


def lane_pairs(plant):
    """{(li, lh): pairs} of a tile holding the plant."""
    c = Counter()
    for rit, qs in plant:
        for b in qs:
            c[(b % 32, (rit >> 2) & 1)] += 1
    return c


def test_plants_reach_both_sides_of_every_capacity_edge():
    """The lanes of every plant hold what its name says; on 256 CUs the cases have waves of 1, 2 and 3 tiles under thresholds,
    both query-tile counts and both dims, a ragged tile, a filter, speculation on and off."""
    def counts(p):
        return sorted(lane_pairs(p).values())
    assert counts(ONE_PAIR) == [1]
    assert counts(TWO_QUERIES_ONE_LANE) == [2] and counts(TWO_ROWS_ONE_LANE) == [2] and counts(TWO_ROWS_ONE_LANE_NQT1) == [2]
    assert counts(TWO_ROWS_TWO_LANES) == [1, 1] and counts(ONE_AND_TWO) == [1, 2]
    assert sum(counts(FULL_192)) == STAGE_DIRECT and sum(counts(OVER_193)) == STAGE_DIRECT + 1
    assert counts(OVER_193)[0] == 1 and sum(counts(OVER_194)) == STAGE_DIRECT + 2 and counts(OVER_194)[0] == 2
    ring = counts(RING_48)
    assert set(ring) == {1} and len(ring) < STAGE_FLUSH < 2 * len(ring) and 2 * len(ring) - STAGE_FLUSH + len(ring) > STAGE_FLUSH
    tiles, dim_nqt = set(), set()
    for c in CASES.values():
        g = geometry(c, MI355X_CUS)
        p = plan(g.n, c.B, c.depth, MI355X_CUS, c.spec)
        last = wave_tiles(g.n - g.r, MI355X_CUS)
        assert last == ({1, 2} if c.half_rounds == 3 else {2, 3}), (c.name, last)
        assert wave_tiles(p.chunks[0][1], MI355X_CUS) == {1}, c.name
        tiles |= last
        dim_nqt.add((c.dim, 2 if c.B > 32 else 1))
        assert 30_000 <= g.n <= 200_000, (c.name, g.n)
    assert tiles == {1, 2, 3} and dim_nqt == {(384, 1), (384, 2), (768, 1), (768, 2)}
    assert any(c.ragged for c in CASES.values()) and {c.spec for c in CASES.values()} == {True, False}


# ==================================================================== GPU
def put(rows, q, g, tile, plant, won, w=0.1):
    """Writes the plant into a tile of the last chunk; `won` collects query -> planted rows."""
    B = q.shape[0]
    tr = g.rows(tile)
    for rit, qs in plant:
        row = tr[rit]
        others = [b for b in range(B) if b not in qs]
        basis, _ = np.linalg.qr(q[others].astype(np.float64).T)
        v = q[qs].astype(np.float64).sum(axis=0)
        x = v / np.linalg.norm(v) + w * rows[row].astype(np.float64)
        x -= basis @ (basis.T @ x)
        rows[row] = (x / np.linalg.norm(x)).astype(np.float32)
        for b in qs:
            won.setdefault(b, []).append(row)


def winners(won, depth):
    """The queries whose planted rows all fit the list (each scores far over the background)."""
    return {b: np.array(w) for b, w in won.items() if len(w) <= depth}


def waves(g, k):
    """First tiles of the last chunk's waves of k tiles."""
    out = [f for f in range(g.stride) if g.count(f) == k]
    assert out, k
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["pairs-d384", "pairs-d768"])
def test_one_and_two_pairs_in_a_lane(stream_ctx, O, num_cus, name):
    """Exactly one pair in a lane, and exactly two: two queries 32 apart on one row, two rows of one register half, the same two
    rows' worth split over both halves (two lanes at one), and a lane at two beside a lane at one.  First, middle and last tiles
    of three-tile waves."""
    c = CASES[name]
    g = geometry(c, num_cus)
    rows, q = background(c.dim, g.n), queries(c.dim, c.B, 51)
    three = waves(g, 3)
    f = [three[i * (len(three) - 1) // 4] for i in range(5)]
    assert len(set(f)) == 5
    won = {}
    put(rows, q, g, f[0], ONE_PAIR, won)
    put(rows, q, g, f[1] + g.stride, TWO_QUERIES_ONE_LANE, won)
    put(rows, q, g, f[2] + 2 * g.stride, TWO_ROWS_ONE_LANE, won)
    put(rows, q, g, f[3] + g.stride, TWO_ROWS_TWO_LANES, won)
    put(rows, q, g, f[4], ONE_AND_TWO, won)
    put(rows, q, g, f[4] + g.stride, [(9, [7])], won)          # the lane that was at one beside a two, at one alone
    run(stream_ctx, O, c, rows, q, winners(won, c.depth))


@pytest.mark.gpu
def test_two_rows_in_a_lane_with_one_query_tile(stream_ctx, O, num_cus):
    """NQT = 1: a lane at one and a lane at two, in a two-tile wave's tiles."""
    c = CASES["pairs-nqt1"]
    g = geometry(c, num_cus)
    rows, q = background(c.dim, g.n), queries(c.dim, c.B, 52)
    f = waves(g, 2)[1]
    won = {}
    put(rows, q, g, f, [(30, [2])], won)
    put(rows, q, g, f + g.stride, TWO_ROWS_ONE_LANE_NQT1, won)
    run(stream_ctx, O, c, rows, q, winners(won, c.depth))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["consecutive-d384", "consecutive-d768"])
def test_one_survivor_in_every_tile_of_a_wave(stream_ctx, O, num_cus, name):
    """Every tile of a three-tile and of a two-tile wave has one survivor: the same lane three times with another register row
    each time (a key made from the tile before would be another row's), then another lane each time."""
    c = CASES[name]
    g = geometry(c, num_cus)
    rows, q = background(c.dim, g.n), queries(c.dim, c.B, 53)
    three, two = waves(g, 3), waves(g, 2)
    won = {}
    for i, rit in enumerate([1, 10, 27]):                      # lane (0, lh = 0), rows of three register quarters
        put(rows, q, g, three[1] + i * g.stride, [(rit, [0])], won)
    for i, (rit, b) in enumerate([(5, 1), (16, 2), (31, 3)]):
        put(rows, q, g, three[-2] + i * g.stride, [(rit, [b])], won)
    for i, (rit, b) in enumerate([(0, 4), (4, 4)]):
        put(rows, q, g, two[0] + i * g.stride, [(rit, [b])], won)
    run(stream_ctx, O, c, rows, q, winners(won, c.depth))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["last-tiles-12", "last-tiles-23"])
def test_last_and_last_but_one_tile(stream_ctx, O, num_cus, name):
    """A survivor in the last tile of a wave (tested after the loop, in the iteration without a span) and in its last but one,
    for every length of wave the chunk has; the last tile once with a lane at two."""
    c = CASES[name]
    g = geometry(c, num_cus)
    rows, q = background(c.dim, g.n), queries(c.dim, c.B, 54)
    won, b = {}, 0
    for k in sorted({g.count(f) for f in range(g.stride)}):
        fs = waves(g, k)
        put(rows, q, g, fs[0] + (k - 1) * g.stride, [(7 + k, [b])], won)
        if k > 1:
            put(rows, q, g, fs[0] + (k - 2) * g.stride, [(20 + k, [b + 1])], won)
        put(rows, q, g, fs[-1] + (k - 1) * g.stride, [(12, [b + 2]), (14, [b + 2])], won)
        b += 3
    assert b <= c.B
    run(stream_ctx, O, c, rows, q, winners(won, c.depth))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["direct-d384", "direct-d768"])
def test_direct_limit(stream_ctx, O, num_cus, name):
    """A tile of exactly OI_STAGE - OI_STAGE_FLUSH pairs (staged), of one more in a lane of its own and of two more in that lane
    (both straight to the pool), each followed in its wave by a tile with one survivor."""
    c = CASES[name]
    g = geometry(c, num_cus)
    rows, q = background(c.dim, g.n), queries(c.dim, c.B, 55)
    three = waves(g, 3)
    won = {}
    for i, plant in enumerate([FULL_192, OVER_193, OVER_194]):
        f = three[i * (len(three) - 1) // 2]
        put(rows, q, g, f + g.stride, plant, won, w=0.05)
        put(rows, q, g, f + 2 * g.stride, [(3 + i, [10 + i])], won)
    run(stream_ctx, O, c, rows, q, winners(won, c.depth))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ring-d384", "ring-d768"])
def test_staging_ring_crosses_a_flush_inside_an_append(stream_ctx, O, num_cus, name):
    """48 lanes with a pair each in all three tiles of a wave: the second append takes the staged pairs from 48 to 96, over the
    64 that leave at once, the third from 32 to 80; the last 16 leave at the end."""
    c = CASES[name]
    g = geometry(c, num_cus)
    rows, q = background(c.dim, g.n), queries(c.dim, c.B, 56)
    f = waves(g, 3)[2]
    won = {}
    for i in range(3):
        put(rows, q, g, f + i * g.stride, RING_48, won)
    run(stream_ctx, O, c, rows, q, winners(won, c.depth))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged-12", "ragged-31"])
def test_ragged_last_tile(stream_ctx, O, num_cus, name):
    """The corpus ends 12 or 31 rows into its last tile and the survivor is the last real row.  Every row scores below 0 for
    query 2, so the padding rows (zeros: score 0) pass its test and would head its list without the mask: with 12 rows its lanes
    keep many of them (the tile is appended from the sums), with 31 rows one lane keeps exactly one, which the mask then drops
    (the tile is appended from what the tests kept, that lane left out).  The wave's tile two before the last one -- the same
    metadata slot -- has winners of query 1 at the positions the last tile does not have."""
    c = CASES[name]
    g = geometry(c, num_cus)
    rng = np.random.default_rng(57)
    u = rng.standard_normal(c.dim)
    u /= np.linalg.norm(u)
    x = background(c.dim, g.n).astype(np.float64) + 0.5 * u       # x . u > 0 for every row
    rows = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    q = queries(c.dim, c.B, 57)
    v = -u + 0.3 * q[2]
    q[2] = (v / np.linalg.norm(v)).astype(np.float32)
    last_tile = g.n_tiles - 1
    last = g.rows(last_tile)
    assert last.size == c.ragged and last[-1] == g.n - 1 and last_tile // g.stride == 2
    before = g.rows(last_tile - 2 * g.stride)[c.ragged:][:3]
    rows[before] = near(q[1], rows[before])
    w = last[-1:]
    rows[w] = near(q[0], rows[w])
    assert O.dot_scores(rows, q[2]).max() < 0
    R = run(stream_ctx, O, c, rows, q, {0: w, 1: before})
    assert listed(R.La, 2, 0).max() < g.n


@pytest.mark.gpu
def test_filtered_search(O, num_cus):
    """Under a filter (the FILT instantiation): a row that passes it and a row that fails it, both over the threshold, in one
    tile -- in two lanes (the failing lane's pair is dropped after the test kept it) and in one lane (at two before the filter,
    at one after it).  Under a filter the f32-stream mode takes the exact kernels (tests/test_gpu_filter.py), whose sums run in
    another order, so the bit-for-bit reference here is that module's: the same index's unfiltered lists, two entries deeper,
    restricted to the rows that pass and cut."""
    import openintel_amd as oi
    from openintel_amd import _lib
    c = CASES["filtered"]
    g = geometry(c, num_cus)
    rows, q = background(c.dim, g.n), queries(c.dim, c.B, 58)
    three = waves(g, 3)
    won = {}
    put(rows, q, g, three[0] + g.stride, [(2, [0]), (6, [0])], won)
    put(rows, q, g, three[-1] + 2 * g.stride, [(9, [1]), (11, [1])], won)
    put(rows, q, g, three[1], [(3, [0])], won)
    group = np.zeros(g.n, dtype=np.uint32)
    fail = np.array([won[0][1], won[1][0]])
    group[fail] = 1
    group[np.arange(0, g.n, 7)] |= 2                                            # (a bit the filter does not look at)
    F = np.tile(np.array([1, 0, 0, 0xFFFFFFFF], dtype=np.uint32), (c.B, 1))     # group & 1 == 0, any stamp

    n, B = g.n, c.B
    rng = np.random.default_rng(n + B)
    fwd = _forward(rng, n)
    qo = np.arange(0, 2 * B + 1, 2, dtype=np.uint32)
    qt = rng.integers(0, VOCAB, size=2 * B).astype(np.uint32)
    a = oi.HipContext(0)
    try:
        a.set_cosine_mode(_lib.OI_COSINE_SCREEN)
        a.set_screen_speculation(c.spec)
        ia = _index(a, rows, 0, fwd)
        ia.set_doc_attrs(group=group)
        a.profile_reset(1)
        La = ia.search_lists(q, qt, qo, depth=c.depth, filters=F)
        launches = int(a.profile_read("cosine")[1])
        gate = float(a.profile_read("screen_gate")[0])
        a.profile_reset(0)
        U = ia.search_lists(q, qt, qo, depth=c.depth + fail.size)
        ia.close()
    finally:
        a.close()
    assert launches >= 2 and gate == 0.0, (launches, gate)
    for b in range(B):
        cu = int(U.cos_counts[b])
        keep = ~np.isin(U.cos_docs[b][:cu], fail)
        assert int(La.cos_counts[b]) == c.depth and np.array_equal(La.cos_docs[b], U.cos_docs[b][:cu][keep][:c.depth]), b
        assert np.array_equal(La.cos_scores[b].view(np.uint32), U.cos_scores[b][:cu][keep][:c.depth].view(np.uint32)), b
    passes = (group & 1) == 0
    for b in range(B):
        ref = O.dot_scores(rows, q[b]).astype(np.float64)
        ref[~passes] = -np.inf
        check_oracle(La, b, ref, c.depth, n, 0)
    for b in (0, 1):
        got = set(listed(La, b, 0).tolist())
        assert set(won[b]) - set(fail.tolist()) <= got and not set(fail.tolist()) & got, b
