"""The int8 screen's tile test runs one tile late (csrc/cosine_screen_i8.hip): what that can get wrong.

cosine_i8_screen keeps a tile's sums S = 128 S_h + S_l in registers and tests them inside the NEXT tile's matrix span, against the
tile's {scale, e_r} pairs in a two-slot ring; the survivors are appended after that span, only the (query tile, register row)
bits some lane kept being visited; the last tile of a wave is tested after the loop, and the first span of a wave tests a
"tile -1" whose mask is dropped.  The defects this invites are silent: a wave's last tile never drained, a tile tested against its
neighbour's metadata, survivors staged in another order or twice, a "tile -1" that passes something.  Each case below plants the
winners of some queries where such a defect changes the lists, and compares the int8 route with the f32-stream screen (bit for
bit) and with the f64 oracle, as tests/test_gpu_screen_i8_edges.py does; the geometry comes from that module's mirrors.

A wave takes the chunk's 32-row tiles f, f + stride, f + 2 stride, ... (stride = 4 waves x workgroups).  Every case has a first
chunk of one tile per wave (no threshold yet: every pair passes, straight to the pool) and a last chunk under the first chunk's
thresholds whose waves hold `half_rounds / 2` rounds of tiles: {1, 2} or {2, 3} tiles per wave."""
from typing import NamedTuple

import numpy as np
import pytest

from test_gpu_screen_i8_edges import MI355X_CUS, TILE, check_all, listed, plan, run_both, screen_geometry, wave_tiles

STAGE_DIRECT = 256 - 64   # oi_lds_dma.h: OI_STAGE - OI_STAGE_FLUSH, the most pairs of one tile a wave stages


class Case(NamedTuple):
    name: str
    dim: int
    B: int
    depth: int
    half_rounds: int      # tiles of the last chunk, in half rounds of `stride` tiles: 3 -> waves of 1 and 2 tiles, 5 -> 2 and 3
    ragged: int           # rows of the last tile (0: a whole tile)
    spec: bool


CASES = {c.name: c for c in [
    Case("one-tile-wave", 384, 9, 10, 3, 0, True),
    Case("ragged-last-tile", 384, 33, 10, 5, 12, True),
    Case("adjacent-d384", 384, 33, 10, 5, 0, False),
    Case("adjacent-d768", 768, 9, 10, 5, 7, True),
    Case("every-tile-spec", 384, 33, 10, 5, 0, True),
    Case("every-tile-proven", 384, 33, 10, 5, 0, False),
    Case("direct-spec", 384, 33, 10, 5, 0, True),
    Case("direct-proven", 384, 9, 10, 5, 0, False),
]}


class Geo(NamedTuple):
    n: int
    r: int                # the last chunk's first row
    n_tiles: int          # its tiles
    stride: int           # tiles between two tiles of one wave

    def count(self, f):   # tiles of the wave whose first tile is f
        return (self.n_tiles - f + self.stride - 1) // self.stride if f < self.n_tiles else 0

    def rows(self, tile):  # the rows of a tile of the last chunk
        a = self.r + TILE * tile
        return np.arange(a, min(a + TILE, self.n))


def geometry(c: Case, num_cus: int) -> Geo:
    """n such that the last chunk of the case's schedule has half_rounds / 2 rounds of tiles, the last one of `ragged` rows."""
    stride = 4 * max(1, num_cus * 7 // 8)
    rows_last = c.half_rounds * stride // 2 * TILE - ((TILE - c.ragged) if c.ragged else 0)
    n = 8192 + rows_last
    for _ in range(4):
        p = plan(n, c.B, c.depth, num_cus, c.spec)
        n = p.chunks[-1][0] + rows_last
    p = plan(n, c.B, c.depth, num_cus, c.spec)
    r, e = p.chunks[-1]
    assert e == n and e - r == rows_last and len(p.chunks) >= 2, (c.name, p.chunks)
    assert screen_geometry(e - r, num_cus)[0] * 4 == stride, c.name
    return Geo(n, r, (e - r + TILE - 1) // TILE, stride)


def test_case_table_reaches_every_deferred_edge():
    """On 256 CUs the table has waves of exactly 1, 2 and 3 tiles in a chunk under thresholds, one tile per wave in the first
    chunk, both query-tile counts, both dims, a ragged last tile, speculation on and off."""
    tiles, dim_nqt, first = set(), set(), set()
    for c in CASES.values():
        g = geometry(c, MI355X_CUS)
        p = plan(g.n, c.B, c.depth, MI355X_CUS, c.spec)
        last = wave_tiles(g.n - g.r, MI355X_CUS)
        assert last == ({1, 2} if c.half_rounds == 3 else {2, 3}), (c.name, last)
        assert last == {g.count(f) for f in range(g.stride)}, c.name
        tiles |= last
        first |= wave_tiles(p.chunks[0][1], MI355X_CUS)
        dim_nqt.add((c.dim, 2 if c.B > 32 else 1))
        assert 30_000 <= g.n <= 200_000, (c.name, g.n)
    assert tiles == {1, 2, 3} and first == {1}
    assert {(384, 1), (384, 2), (768, 1)} <= dim_nqt and {d for d, _ in dim_nqt} == {384, 768}
    assert any(c.ragged for c in CASES.values()) and {c.spec for c in CASES.values()} == {True, False}


# ==================================================================== GPU
@pytest.fixture(scope="module")
def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def O():
    from oracle import lib
    return lib


@pytest.fixture(scope="module")
def stream_ctx():
    import openintel_amd as oi
    from openintel_amd import _lib
    s = oi.HipContext(0)
    s.set_cosine_mode(_lib.OI_COSINE_SCREEN_STREAM)
    yield s
    s.close()


_ROWS = {}


def background(dim, n):
    """Seeded unit rows, built once per dim (a copy: the cases write into it)."""
    from openintel_amd import synth
    if dim not in _ROWS:
        _ROWS[dim] = synth.embeddings_np(200_000, dim, seed=9101 + dim)
    return _ROWS[dim][:n].copy()


def queries(dim, B, seed):
    from openintel_amd import synth
    return synth.embeddings_np(B, dim, seed=seed)


def near(v, rows, w=0.3):
    """Unit rows close to v (score ~ 0.95 with w = 0.3), each with its own noise: no ties."""
    x = v[None, :].astype(np.float64) + w * rows.astype(np.float64)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def run(stream_ctx, O, c, rows, q, winners, short_rows_only=True):
    """Both routes, the gate shut, every list the oracle's, every planted winner listed."""
    R = run_both(stream_ctx, rows, q, c.depth, 0, c.spec, short_rows_only=short_rows_only)
    assert R.launches["cosine"] >= 2 and R.gate == 0.0, (R.launches, R.gate)
    check_all(O, R, rows, q, c.depth, 0)
    for b, w in winners.items():
        assert set(np.asarray(w).tolist()) <= set(listed(R.La, b, 0).tolist()), (c.name, b)
    return R


@pytest.mark.gpu
def test_last_tile_of_a_one_tile_wave(stream_ctx, O, num_cus):
    """The whole top-k of two queries sits in the only tile of a wave (tested and drained after the loop, with no span at all),
    and that of a third in the last tile of a two-tile wave."""
    c = CASES["one-tile-wave"]
    g = geometry(c, num_cus)
    rows, q = background(c.dim, g.n), queries(c.dim, c.B, 31)
    one = [f for f in range(g.stride) if g.count(f) == 1]
    two = [f for f in range(g.stride) if g.count(f) == 2]
    assert one and two
    tiles = {0: one[0], 1: one[-1], 2: two[len(two) // 2] + g.stride}
    winners = {}
    for b, t in tiles.items():
        w = g.rows(t)[[0, 1, 5, 8, 13, 16, 21, 27, 30, 31]]
        rows[w] = near(q[b], rows[w])
        winners[b] = w
    run(stream_ctx, O, c, rows, q, winners)


@pytest.mark.gpu
def test_last_tile_ragged(stream_ctx, O, num_cus):
    """The last tile of the corpus has 12 rows: the top-k of query 0 is its last ten, the last real row among them.  Every row
    scores below 0 for query 2, so the tile's padding (zeros: score 0) would head its list if the late test lost the mask."""
    c = CASES["ragged-last-tile"]
    g = geometry(c, num_cus)
    rng = np.random.default_rng(5)
    u = rng.standard_normal(c.dim)
    u /= np.linalg.norm(u)
    x = background(c.dim, g.n).astype(np.float64) + 0.5 * u       # x . u > 0 for every row
    rows = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    q = queries(c.dim, c.B, 32)
    v = -u + 0.3 * q[2]
    q[2] = (v / np.linalg.norm(v)).astype(np.float32)
    last = g.rows(g.n_tiles - 1)
    assert last.size == c.ragged and last[-1] == g.n - 1 and g.count((g.n_tiles - 1) % g.stride) == (g.n_tiles - 1) // g.stride + 1
    w = last[-c.depth:]
    rows[w] = near(q[0], rows[w])
    assert O.dot_scores(rows, q[2]).max() < 0
    R = run(stream_ctx, O, c, rows, q, {0: w})
    assert listed(R.La, 2, 0).max() < g.n


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["adjacent-d384", "adjacent-d768"])
def test_adjacent_tiles_keep_their_own_metadata(stream_ctx, O, num_cus, name):
    """Two consecutive tiles of one wave whose row scales (and e_r) differ by 2^10.  Wave f: the winners of query 0 (unit rows),
    then a tile of rows near query 3 scaled by 2^-10 (true scores ~ 1e-3, far from the list).  Wave f2: the other way round with
    queries 4 and 1.  The winners' sums under the small tile's metadata fall below the threshold and are dropped; the small
    rows' sums under the winners' metadata pass with keys ~ 0.95 and lift the threshold of queries 3 / 4 over their true lists."""
    c = CASES[name]
    g = geometry(c, num_cus)
    rows, q = background(c.dim, g.n), queries(c.dim, c.B, 33 + c.dim)
    three = [f for f in range(g.stride) if g.count(f) == 3]
    assert len(three) >= 2
    f, f2 = three[0], three[-1]
    small = np.float32(2.0 ** -10)
    w0, w1 = g.rows(f)[3:3 + c.depth], g.rows(f2 + g.stride)[20:20 + c.depth]
    rows[w0] = near(q[0], rows[w0])
    rows[w1] = near(q[1], rows[w1])
    s3, s4 = g.rows(f + g.stride), g.rows(f2)
    rows[s3] = near(q[3], rows[s3]) * small
    rows[s4] = near(q[4], rows[s4]) * small
    R = run(stream_ctx, O, c, rows, q, {0: w0, 1: w1})
    for b, s in ((3, s3), (4, s4)):
        assert not set(s.tolist()) & set(listed(R.La, b, 0).tolist()), b


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["every-tile-spec", "every-tile-proven"])
def test_survivors_in_every_tile_of_a_wave(stream_ctx, O, num_cus, name):
    """The top-k of queries 0, 1 and 32 spread over all three tiles of one wave (4 + 3 + 3 rows), seven winners of query 5 over
    both tiles of a two-tile wave: the staged survivors of consecutive late tests (the last one drained after the loop) all
    reach the pool, once."""
    c = CASES[name]
    g = geometry(c, num_cus)
    rows, q = background(c.dim, g.n), queries(c.dim, c.B, 34)
    three = [f for f in range(g.stride) if g.count(f) == 3]
    two = [f for f in range(g.stride) if g.count(f) == 2]
    f3, f2 = three[len(three) // 2], two[0]
    winners = {}
    for o, (b, f, k) in enumerate([(0, f3, 3), (1, f3, 3), (32, f3, 3), (5, f2, 2)]):
        w = np.concatenate([g.rows(f + i * g.stride)[[o, 8 + o, 16 + o, 28 + o][:4 if i == 0 else 3]] for i in range(k)])
        rows[w] = near(q[b], rows[w])
        winners[b] = w
    run(stream_ctx, O, c, rows, q, winners)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["direct-spec", "direct-proven"])
def test_direct_to_pool_tile_and_silent_first_tiles(stream_ctx, O, num_cus, name):
    """The first tile of EVERY wave of the last chunk holds rows of norm 2^-20 (nothing of it can pass: a "tile -1" test that
    passed anything, or a first tile tested against leftovers, would flood the pool and open the gate).  The middle tile of a
    three-tile wave holds 32 rows near the mean of seven queries: 224 pairs of one tile, over the 192 a wave stages, so they go
    straight to the pool; the wave's last tile holds the winners of another query, staged after them.  (A third of the corpus
    being tiny lowers the RMS the long-row classes are cut at, and a couple of unit rows land in them: they are rescored
    whatever the screen does, the other rows of the tile still go through it.)"""
    c = CASES[name]
    g = geometry(c, num_cus)
    rows, q = background(c.dim, g.n), queries(c.dim, c.B, 35)
    first = np.arange(g.r, g.r + g.stride * TILE)
    rows[first] *= np.float32(2.0 ** -20)
    three = [f for f in range(g.stride) if g.count(f) == 3]
    f = three[len(three) // 3]
    nq = 7
    assert TILE * nq > STAGE_DIRECT
    mid = g.rows(f + g.stride)
    mean = q[:nq].astype(np.float64).sum(axis=0)
    rows[mid] = near((mean / np.linalg.norm(mean)).astype(np.float32), rows[mid], w=0.2)
    w8 = g.rows(f + 2 * g.stride)[2:2 + c.depth]
    rows[w8] = near(q[8], rows[w8])
    R = run(stream_ctx, O, c, rows, q, {8: w8}, short_rows_only=False)
    for b in range(nq):
        assert set(listed(R.La, b, 0).tolist()) <= set(mid.tolist()), b     # ten of the 32: which ones, the oracle says
    assert not set(first.tolist()) & set(np.concatenate([listed(R.La, b, 0) for b in range(c.B)]).tolist())
