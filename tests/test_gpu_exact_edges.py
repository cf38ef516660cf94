"""The exact f32 cosine kernels (csrc/cosine.hip, csrc/cosine_ksplit.hip, csrc/cosine_split.hip) at every query-group, tile,
chunk and pool edge, bit for bit against the oracle.

The exact scorer is what every other cosine tier is judged against (OI_COSINE_EXACT, every batch of <= 8 queries without a
screening copy, every dim other than 384 / 768, every filtered search on the f32-stream route, the gated fallback behind the
screens).  One search can run four kernels (oi_launch_cosine_chunk): the GEMV (cosine_gemv_filter<NQ>, B <= 8), the K-split
(cosine_ksplit16_filter<D, NQT> at d = 384 / 768 / 1024, one launch per group of 64 queries), the v1 tile kernel
(cosine_mfma_filter<NQT>, every other dim) and, in OI_COSINE_SPLIT at 384 / 768, the split-precision kernel
(cosine_split_filter<D, NQT>).  The search cuts the corpus into chunks (search.hip: cosine_exact through chunk_schedule and
oi_chunk_end, the pool budget of plan_search, oi_cosine_max_chunk_rows); a later chunk is filtered against the thresholds the
selects carried out of the earlier ones.  A wrong group offset, tile mask, epilogue guard or carried threshold drops a true
top-k row on some data only: nothing crashes and nothing slows down.

CASES below is the table of what this module runs.  A pure-Python mirror of the dispatch (exact_pool, exact_schedule, kernel_of,
the two pool geometries) computes each case's chunks and kernels; CPU tests check the table against the mirror at 256 CUs and
that it reaches every kernel variant, every rule of oi_chunk_end, a chunk cut by the pool and every per-workgroup load.  On the
GPU every case checks its chunk count through the profiler (one "cosine" span per chunk) and its lists against the oracle.

Data: rows and queries are integers in [-3, 3], so every product and partial sum is exact in f32 in any order (|dot| <=
9 x 1024 < 2^24): cosine, BM25 and fused lists must equal the oracle's bit for bit, ties broken towards the lower doc id.
Cosine reference scores come from one float64 matmul (test_gpu_bf16_edges.test_int_matmul_equals_oracle_dot_scores).  The split
kernel takes small integers exactly too (each is its own bf16 high plane); it turns an infinity into NaN by construction
(inf - bf16(inf) in the lower planes), so the non-finite test below leaves split mode out."""
from typing import NamedTuple, Union

import numpy as np
import pytest

from test_gpu_bf16_edges import (VOCAB, _assert_lists, _forward, _oracle_lists, _pool, _query_terms, _scores_f64, chunk_end,
                                 chunk_growth, first_chunk_rows)

MI355X_CUS = 256          # what the table's declared chunk counts assume (the GPU tests read the real count)
OI_MAX_DEPTH = 1024       # also the keys per query the exact pools carry between chunks
EXACT, SPLIT, SCREEN = 0, 1, 2        # _lib.OI_COSINE_*
MAXB = -1                 # doc_id_base = 2^32 - 1 - n: the last doc id is 2^32 - 2
KSPLIT_DIMS = (384, 768, 1024)
SPLIT_DIMS = (384, 768)


# ==================================================================== mirror of the exact route's dispatch
def exact_pool(n: int, B: int, num_cus: int):
    """search.hip, plan_search + cosine.hip, oi_cosine_max_chunk_rows: (cos_stride, max_chunk) of an f32 corpus."""
    carry, slack = OI_MAX_DEPTH, 32 * (num_cus + 1)
    budget = (13 << 28) // 8 // B
    stride = min(carry + n + slack, max(min(1 << 24, budget), carry + 4 * slack))
    return stride, stride - carry - slack


class Chunk(NamedTuple):
    begin: int
    end: int
    rule: str             # the rule of oi_chunk_end that ended it: "plain", "stretch" or "n-max"
    cut: bool             # the planned size was above max_chunk: the pool cut it

    @property
    def rows(self) -> int:
        return self.end - self.begin


def exact_schedule(n: int, B: int, depth: int, num_cus: int, first=None):
    """search.hip: cosine_exact -- chunk_schedule(n, oi_first_chunk_rows(depth), oi_chunk_growth(B), max_chunk, stretch_first =
    true).  first: the gated fallback's first chunk (max_chunk)."""
    _, max_chunk = exact_pool(n, B, num_cus)
    assert max_chunk > 0
    out, chunk, r, growth = [], (first_chunk_rows(depth) if first is None else first), 0, chunk_growth(B)
    while r < n:
        cut = chunk > max_chunk and max_chunk < n          # (max_chunk = n: the whole corpus fits, nothing is cut)
        chunk = min(chunk, max_chunk)
        e = chunk_end(r, chunk, n, max_chunk, chunk * growth)
        e0 = min(n, r + chunk)
        out.append(Chunk(r, e, "plain" if e == e0 else "stretch" if e == n else "n-max", cut and e - r == max_chunk))
        r = e
        chunk *= growth
    return out


def kernel_of(dim: int, B: int, mode: int = EXACT, filtered: bool = False):
    """cosine.hip: oi_launch_cosine_chunk -- the kernel of every launch of one chunk, in launch order."""
    if B <= 8:
        return ("gemv<%d>" % B,)
    Bp = (B + 31) & ~31
    out = []
    for q0 in range(0, Bp, 64):
        nqt = 2 if Bp - q0 >= 64 else 1
        if dim in KSPLIT_DIMS:
            split = mode == SPLIT and dim in SPLIT_DIMS and not filtered
            out.append(("split<%d,%d>" if split else "ksplit16<%d,%d>") % (dim, nqt))
        else:
            out.append("tile<%d>" % nqt)
        if q0 + 64 >= B:
            break
    return tuple(out)


def ksplit_geometry(rows: int, num_cus: int):
    """cosine_ksplit.hip: oi_cosine_ksplit_geometry -> (segments, segment capacity)."""
    tiles = (rows + 31) // 32
    segs = min(tiles, num_cus)
    return segs, (tiles + segs - 1) // segs * 32


def gemv_geometry(rows: int, num_cus: int):
    """cosine.hip: oi_cosine_gemv_geometry -> (segments, segment capacity)."""
    blocks = min((rows + 3) // 4, 8 * num_cus) or 1
    return blocks, 4 * ((rows + 4 * blocks - 1) // (4 * blocks))


def pool_use(dim: int, B: int, rows: int, stride: int, num_cus: int):
    """(segments, segment capacity, segment counters per query) of one chunk: what oi_launch_cosine_chunk requires to fit."""
    if B <= 8:
        return gemv_geometry(rows, num_cus) + (8 * num_cus,)
    if dim in KSPLIT_DIMS:
        return ksplit_geometry(rows, num_cus) + (num_cus,)
    return 1, stride - OI_MAX_DEPTH, num_cus          # the v1 tile kernel: one global counter per query


def work_counts(dim: int, B: int, rows: int, num_cus: int) -> set:
    """The distinct loads of one chunk: 32-row tiles per K-split workgroup (tile b, b + grid, ...), rows per GEMV wave (row w,
    w + waves, ...; 0 when the chunk has fewer rows than waves), 128-row tiles per workgroup of the tile kernel."""
    if B <= 8:
        units, grid = rows, gemv_geometry(rows, num_cus)[0] * 4
    elif dim in KSPLIT_DIMS:
        units, grid = (rows + 31) // 32, ksplit_geometry(rows, num_cus)[0]
    else:
        units = (rows + 127) // 128
        grid = min(units, 4 * num_cus)
    return {(units - f + grid - 1) // grid if f < units else 0 for f in range(grid)}


VARIANTS = ({"gemv<%d>" % b for b in range(1, 9)} | {"ksplit16<%d,%d>" % (d, t) for d in KSPLIT_DIMS for t in (1, 2)} |
            {"tile<1>", "tile<2>"} | {"split<%d,%d>" % (d, t) for d in SPLIT_DIMS for t in (1, 2)})


# ==================================================================== the case table
class CURows(NamedTuple):
    """Rows relative to one K-split round, 32 x num_cus: mult x 32 x num_cus + add."""
    mult: int
    add: int


class Case(NamedTuple):
    name: str
    dim: int
    B: int
    n: Union[int, CURows]
    depth: int
    k: int
    base: int             # doc_id_base (MAXB: 2^32 - 1 - n)
    data: str             # "rand": i.i.d. integers; "ties": a few distinct rows repeated (many ties at every cut)
    mode: int             # EXACT or SPLIT
    kernels: frozenset    # every kernel the case runs (the mirror, checked on the CPU)
    chunks: int           # corpus chunks on an MI355X (the mirror on the CPU, the profiler on the GPU)

    def n_rows(self, num_cus: int) -> int:
        return self.n if isinstance(self.n, int) else self.n.mult * 32 * num_cus + self.n.add

    def doc_base(self, num_cus: int) -> int:
        return 2 ** 32 - 1 - self.n_rows(num_cus) if self.base == MAXB else self.base


def _k(*names):
    return frozenset(names)


def _ks(d, *nqt):
    return frozenset("ksplit16<%d,%d>" % (d, t) for t in nqt)


def _sp(d, *nqt):
    return frozenset("split<%d,%d>" % (d, t) for t in nqt)


def _tl(*nqt):
    return frozenset("tile<%d>" % t for t in nqt)


N2 = 8192 + 3000               # depth <= 256: a first chunk of 8192 rows, then a 3000-row tail longer than a quarter of it
N_STRETCH = 8192 + 2048        # the tail is exactly a quarter of the first chunk: taken along, one chunk
N_NOSTRETCH = N_STRETCH + 1    # one row more: two chunks
N_TWO_TILES = 8192 + 1         # one chunk of 257 tiles on 256 CUs: workgroup 0 owns two tiles, the second holding one row
N3_GEMV = 8192 + 131072 + 40000   # B <= 8 (growth x 16): three chunks
N3 = 8192 + 65536 + 20000      # B > 8 (growth x 8): three chunks, 1, 8 and 2..3 tiles per workgroup
N2D = 32768 + 9000             # depth 1024: a first chunk of 32 768 rows
N_NMAX = 202_688               # B = 4096 (max_chunk 97 248): 8192, then up to n - max_chunk (the n-max rule), then max_chunk
N_CUT = N_NMAX + 1             # one row more: 8192, 65 536, a chunk cut to max_chunk, the rest
N_2048 = 450_000               # B = 2048 (max_chunk 203 744): 8192, 65 536, a chunk cut to max_chunk, the rest

CASES = [
    # ---- GEMV: every NQ, dims on both sides of nvec = 64 c (ncol 1..4), one and two rows per wave, n < waves, 1..3 chunks
    Case("gemv-B1-d768", 768, 1, N2, 1, 1, 0, "rand", EXACT, _k("gemv<1>"), 2),
    Case("gemv-B2-d100", 100, 2, N2, 2, 2, 7, "ties", EXACT, _k("gemv<2>"), 2),
    Case("gemv-B3-d4-3chunks", 4, 3, N3_GEMV, 100, 10, MAXB, "rand", EXACT, _k("gemv<3>"), 3),
    Case("gemv-B4-d252-stretch", 252, 4, N_STRETCH, 100, 100, 0, "ties", EXACT, _k("gemv<4>"), 1),
    Case("gemv-B5-d256", 256, 5, N_NOSTRETCH, 10, 10, 1000, "rand", EXACT, _k("gemv<5>"), 2),
    Case("gemv-B6-d260-depth1024", 260, 6, N2, 1024, 1024, 0, "rand", EXACT, _k("gemv<6>"), 1),
    Case("gemv-B7-d1020", 1020, 7, N2, 100, 50, 5, "rand", EXACT, _k("gemv<7>"), 2),
    Case("gemv-B8-d1024", 1024, 8, N2, 100, 100, MAXB, "ties", EXACT, _k("gemv<8>"), 2),
    Case("gemv-B8-d384-depth1024", 384, 8, N2D, 1024, 100, 0, "rand", EXACT, _k("gemv<8>"), 2),
    Case("gemv-B8-d100-3chunks", 100, 8, N3_GEMV, 100, 100, 0, "ties", EXACT, _k("gemv<8>"), 3),
    Case("gemv-B3-n1", 384, 3, 1, 1024, 1024, 7, "rand", EXACT, _k("gemv<3>"), 1),
    Case("gemv-B8-n3", 100, 8, 3, 2, 2, 0, "rand", EXACT, _k("gemv<8>"), 1),
    Case("gemv-B4-d768-split-mode", 768, 4, N2, 100, 10, 0, "rand", SPLIT, _k("gemv<4>"), 2),
    # ---- K-split, d = 384: B at every group edge (the 2-chunk corpora run the second chunk against carried thresholds)
    Case("ks-d384-B9", 384, 9, N2, 1, 1, 0, "rand", EXACT, _ks(384, 1), 2),
    Case("ks-d384-B32", 384, 32, N2, 2, 2, 7, "ties", EXACT, _ks(384, 1), 2),
    Case("ks-d384-B33-stretch", 384, 33, N_STRETCH, 100, 10, 1000, "rand", EXACT, _ks(384, 2), 1),
    Case("ks-d384-B64-nostretch", 384, 64, N_NOSTRETCH, 100, 100, 0, "rand", EXACT, _ks(384, 2), 2),
    Case("ks-d384-B65", 384, 65, N2, 100, 100, MAXB, "ties", EXACT, _ks(384, 2, 1), 2),
    Case("ks-d384-B96", 384, 96, N2, 10, 10, 0, "rand", EXACT, _ks(384, 2, 1), 2),
    Case("ks-d384-B97-depth1024", 384, 97, N2D, 1024, 1024, 0, "rand", EXACT, _ks(384, 2), 2),
    Case("ks-d384-B128", 384, 128, N2, 100, 50, 123_456_789, "ties", EXACT, _ks(384, 2), 2),
    Case("ks-d384-B129", 384, 129, N2, 100, 100, 0, "rand", EXACT, _ks(384, 2, 1), 2),
    Case("ks-d384-B200", 384, 200, N2, 10, 100, 5, "rand", EXACT, _ks(384, 2, 1), 2),
    # ---- K-split, d = 768: the CU-relative sizes, the two-tile workgroup, three chunks
    Case("ks-d768-B9-two-tiles", 768, 9, N_TWO_TILES, 100, 10, 0, "ties", EXACT, _ks(768, 1), 1),
    Case("ks-d768-B32-round", 768, 32, CURows(1, 0), 100, 100, 0, "rand", EXACT, _ks(768, 1), 1),
    Case("ks-d768-B33-round+1", 768, 33, CURows(1, 1), 10, 10, MAXB, "rand", EXACT, _ks(768, 2), 1),
    Case("ks-d768-B64-round+32", 768, 64, CURows(1, 32), 1000, 100, 0, "ties", EXACT, _ks(768, 2), 1),
    Case("ks-d768-B65", 768, 65, N2, 2, 2, 7, "rand", EXACT, _ks(768, 2, 1), 2),
    Case("ks-d768-B96", 768, 96, N2, 100, 1024, 0, "ties", EXACT, _ks(768, 2, 1), 2),
    Case("ks-d768-B97-3chunks", 768, 97, N3, 100, 100, MAXB, "rand", EXACT, _ks(768, 2), 3),
    Case("ks-d768-B128-depth1000", 768, 128, 32000 + 9000, 1000, 1000, 0, "rand", EXACT, _ks(768, 2), 2),
    Case("ks-d768-B129", 768, 129, N2, 10, 10, 1000, "ties", EXACT, _ks(768, 2, 1), 2),
    Case("ks-d768-B200", 768, 200, N2, 100, 100, 0, "rand", EXACT, _ks(768, 2, 1), 2),
    # ---- K-split, d = 1024: ragged tiles (n = 1, 20, 31, 32, 33), depth > n, every group edge
    Case("ks-d1024-B9-n1", 1024, 9, 1, 1024, 1024, MAXB, "rand", EXACT, _ks(1024, 1), 1),
    Case("ks-d1024-B32", 1024, 32, N_NOSTRETCH, 1, 1, 0, "rand", EXACT, _ks(1024, 1), 2),
    Case("ks-d1024-B33-n20", 1024, 33, 20, 100, 100, 0, "rand", EXACT, _ks(1024, 2), 1),
    Case("ks-d1024-B64-n31", 1024, 64, 31, 2, 1, 7, "ties", EXACT, _ks(1024, 2), 1),
    Case("ks-d1024-B65-n32", 1024, 65, 32, 1000, 10, 0, "rand", EXACT, _ks(1024, 2, 1), 1),
    Case("ks-d1024-B96-n33", 1024, 96, 33, 10, 10, MAXB, "rand", EXACT, _ks(1024, 2, 1), 1),
    Case("ks-d1024-B97", 1024, 97, N2, 100, 100, 0, "ties", EXACT, _ks(1024, 2), 2),
    Case("ks-d1024-B128-3chunks", 1024, 128, N3, 100, 10, 5, "ties", EXACT, _ks(1024, 2), 3),
    Case("ks-d1024-B129", 1024, 129, N2, 100, 100, 0, "rand", EXACT, _ks(1024, 2, 1), 2),
    Case("ks-d1024-B200", 1024, 200, N2, 2, 2, MAXB, "ties", EXACT, _ks(1024, 2, 1), 2),
    Case("ks-d1024-B65-split-mode", 1024, 65, N2, 100, 10, 0, "rand", SPLIT, _ks(1024, 2, 1), 2),   # (no split kernel at 1024)
    # ---- the K-split under a pool cut: B = 4096, 64 groups over four chunks
    Case("ks-d384-B4096-pool-cut", 384, 4096, N_CUT, 100, 10, 0, "rand", EXACT, _ks(384, 2), 4),
    # ---- v1 tile kernel: dims 4, 32, 100, 1020; B at its group edges; n around one 128-row tile; two chunks; the pool cuts
    Case("tile-d4-B9-n1", 4, 9, 1, 100, 100, 0, "rand", EXACT, _tl(1), 1),
    Case("tile-d32-B33-n127", 32, 33, 127, 1024, 1024, MAXB, "rand", EXACT, _tl(2), 1),
    Case("tile-d100-B64-n128", 100, 64, 128, 10, 10, 7, "ties", EXACT, _tl(2), 1),
    Case("tile-d1020-B65-n129", 1020, 65, 129, 100, 100, 0, "rand", EXACT, _tl(2, 1), 1),
    Case("tile-d100-B97", 100, 97, N2, 100, 100, 0, "rand", EXACT, _tl(2), 2),
    Case("tile-d1020-B9", 1020, 9, N2, 2, 2, 1000, "ties", EXACT, _tl(1), 2),
    Case("tile-d32-B65-depth1024", 32, 65, N2D, 1024, 100, MAXB, "rand", EXACT, _tl(2, 1), 2),
    Case("tile-d4-B97-3chunks", 4, 97, N3, 100, 100, 0, "rand", EXACT, _tl(2), 3),
    Case("tile-d32-B4096-n-max", 32, 4096, N_NMAX, 100, 10, 0, "rand", EXACT, _tl(2), 3),
    Case("tile-d32-B4096-pool-cut", 32, 4096, N_CUT, 100, 10, MAXB, "ties", EXACT, _tl(2), 4),
    Case("tile-d32-B2048-pool-cut", 32, 2048, N_2048, 100, 10, 0, "rand", EXACT, _tl(2), 4),
    # ---- split mode at 384 / 768: the group-edge cases again
    Case("split-d384-B9", 384, 9, N2, 1, 1, 0, "rand", SPLIT, _sp(384, 1), 2),
    Case("split-d384-B33", 384, 33, N_STRETCH, 100, 10, 1000, "rand", SPLIT, _sp(384, 2), 1),
    Case("split-d384-B65", 384, 65, N2, 100, 100, MAXB, "ties", SPLIT, _sp(384, 2, 1), 2),
    Case("split-d384-B97-depth1024", 384, 97, N2D, 1024, 1024, 0, "rand", SPLIT, _sp(384, 2), 2),
    Case("split-d384-B129", 384, 129, N2, 100, 100, 0, "rand", SPLIT, _sp(384, 2, 1), 2),
    Case("split-d768-B32-round+1", 768, 32, CURows(1, 1), 100, 100, 0, "rand", SPLIT, _sp(768, 1), 1),
    Case("split-d768-B64-two-tiles", 768, 64, N_TWO_TILES, 10, 10, 0, "ties", SPLIT, _sp(768, 2), 1),
    Case("split-d768-B65", 768, 65, N2, 2, 2, 7, "rand", SPLIT, _sp(768, 2, 1), 2),
    Case("split-d768-B97-3chunks", 768, 97, N3, 100, 100, MAXB, "rand", SPLIT, _sp(768, 2), 3),
    Case("split-d768-B129", 768, 129, N2, 10, 10, 1000, "ties", SPLIT, _sp(768, 2, 1), 2),
]
BY_NAME = {c.name: c for c in CASES}

# the filtered pass (exact mode): one case per FILT instantiation family, and B = 97 over two chunks (carried thresholds)
FILTERED = ["gemv-B1-d768", "gemv-B4-d252-stretch", "gemv-B8-d1024", "ks-d384-B9", "ks-d384-B64-nostretch", "ks-d768-B32-round",
            "ks-d768-B65", "ks-d1024-B32", "ks-d1024-B97", "tile-d1020-B9", "tile-d100-B97", "ks-d384-B97-depth1024"]
BIG_B = 2048              # from here on: cosine lists only, empty term lists, the reference in blocks of queries


def case_chunks(c: Case, num_cus: int):
    return exact_schedule(c.n_rows(num_cus), c.B, c.depth, num_cus)


# ==================================================================== CPU: the mirror and the table
def test_mirror_reproduces_known_schedules():
    """The one recorded exact schedule (test_gpu_search_plan.RECORDED["exact"]: 300 000 x 768, B = 64, 3 "cosine" launches) and
    the schedules and geometries the table is built on, at 256 CUs."""
    cus = MI355X_CUS
    assert len(exact_schedule(300_000, 64, 100, cus)) == 3
    assert [(c.rows, c.rule) for c in exact_schedule(N2, 64, 100, cus)] == [(8192, "plain"), (3000, "plain")]
    assert [ksplit_geometry(c.rows, cus) for c in exact_schedule(N2, 64, 100, cus)] == [(256, 32), (94, 32)]
    assert [gemv_geometry(c.rows, cus) for c in exact_schedule(N2, 8, 100, cus)] == [(2048, 4), (750, 4)]
    assert [c.rule for c in exact_schedule(N_STRETCH, 9, 256, cus)] == ["stretch"]
    assert [c.rows for c in exact_schedule(N_NOSTRETCH, 9, 256, cus)] == [8192, 2049]
    assert [c.rule for c in exact_schedule(N_TWO_TILES, 9, 100, cus)] == ["stretch"] and ksplit_geometry(N_TWO_TILES, cus) == (256, 64)
    assert [c.rows for c in exact_schedule(N3_GEMV, 8, 100, cus)] == [8192, 131072, 40000]
    assert [c.rows for c in exact_schedule(N3, 9, 100, cus)] == [8192, 65536, 20000]
    assert [work_counts(768, 9, c.rows, cus) for c in exact_schedule(N3, 9, 100, cus)] == [{1}, {8}, {2, 3}]
    assert [c.rows for c in exact_schedule(N2D, 9, 1024, cus)] == [32768, 9000]
    assert exact_pool(N_NMAX, 4096, cus) == (106_496, 97_248) and exact_pool(N_2048, 2048, cus)[1] == 203_744
    s = exact_schedule(N_NMAX, 4096, 100, cus)
    assert [(c.rows, c.rule, c.cut) for c in s] == [(8192, "plain", False), (N_NMAX - 97_248 - 8192, "n-max", False), (97_248, "plain", True)]
    s = exact_schedule(N_CUT, 4096, 100, cus)
    assert [(c.rows, c.rule, c.cut) for c in s] == [(8192, "plain", False), (65536, "plain", False), (97_248, "plain", True),
                                                    (N_CUT - 8192 - 65536 - 97_248, "plain", False)]
    s = exact_schedule(N_2048, 2048, 100, cus)
    assert [c.rows for c in s] == [8192, 65536, 203_744, N_2048 - 8192 - 65536 - 203_744] and s[2].cut
    assert kernel_of(384, 8) == ("gemv<8>",) and kernel_of(768, 9) == ("ksplit16<768,1>",)
    assert kernel_of(768, 33) == ("ksplit16<768,2>",) and kernel_of(1024, 65) == ("ksplit16<1024,2>", "ksplit16<1024,1>")
    assert kernel_of(384, 97) == ("ksplit16<384,2>",) * 2 and kernel_of(384, 129, SPLIT) == ("split<384,2>", "split<384,2>", "split<384,1>")
    assert kernel_of(384, 200) == ("ksplit16<384,2>",) * 3 + ("ksplit16<384,1>",)
    assert kernel_of(100, 65) == ("tile<2>", "tile<1>") and kernel_of(1024, 64, SPLIT) == ("ksplit16<1024,2>",)
    assert kernel_of(768, 64, SPLIT, filtered=True) == ("ksplit16<768,2>",) and len(kernel_of(32, 4096)) == 64
    # the gated fallback takes as many rows as the pool holds in its first launch
    assert len(exact_schedule(20_011, 129, 100, cus, first=exact_pool(20_011, 129, cus)[1])) == 1


def test_case_table_reaches_every_variant_with_its_declared_schedule():
    """On an MI355X (256 CUs) every case runs the chunks and kernels it names, every chunk fits the candidate pool the search
    allocates (the library refuses a chunk that does not), and the table reaches every kernel variant, every rule of
    oi_chunk_end, a chunk cut by the pool, and 0, 1, 2 and more units of work per workgroup (GEMV: per wave)."""
    cus = MI355X_CUS
    seen, rules, loads, names, cut = set(), set(), {"gemv": set(), "ksplit": set()}, set(), set()
    gemv_dims, gemv_chunks, ks_chunks = set(), set(), set()
    for c in CASES:
        assert c.name not in names, c.name
        names.add(c.name)
        n, base = c.n_rows(cus), c.doc_base(cus)
        assert 0 < n and 0 <= base and base + n <= 2 ** 32 - 1, c.name
        assert 1 <= c.depth <= OI_MAX_DEPTH and 1 <= c.k <= OI_MAX_DEPTH and c.mode in (EXACT, SPLIT), c.name
        s = case_chunks(c, cus)
        assert s[0].begin == 0 and s[-1].end == n and all(a.end == b.begin for a, b in zip(s, s[1:])), c.name
        assert len(s) == c.chunks, (c.name, [(ch.begin, ch.end) for ch in s])
        ks = set(kernel_of(c.dim, c.B, c.mode))
        assert ks == set(c.kernels), (c.name, sorted(ks))
        seen |= ks
        stride, max_chunk = exact_pool(n, c.B, cus)
        for ch in s:
            segs, cap, counters = pool_use(c.dim, c.B, ch.rows, stride, cus)
            assert ch.rows <= max_chunk and segs <= counters and OI_MAX_DEPTH + segs * cap <= stride, (c.name, ch)
            assert ch.rows <= segs * cap, (c.name, ch)               # room for every row of the chunk
            rules.add(ch.rule)
            if ch.cut:
                cut.add("ksplit" if c.dim in KSPLIT_DIMS else "tile")
            if c.B <= 8:
                loads["gemv"] |= work_counts(c.dim, c.B, ch.rows, cus)
            elif c.dim in KSPLIT_DIMS:
                loads["ksplit"] |= work_counts(c.dim, c.B, ch.rows, cus)
        if c.B <= 8:
            gemv_dims.add(c.dim)
            gemv_chunks.add(len(s))
        elif c.dim in KSPLIT_DIMS:
            ks_chunks.add(len(s))
    assert seen == VARIANTS, sorted(VARIANTS ^ seen)
    assert sum(v.startswith("gemv") for v in seen) == 8 and sum(v.startswith("ksplit16") for v in seen) == 6
    assert sum(v.startswith("tile") for v in seen) == 2 and sum(v.startswith("split") for v in seen) == 4
    assert rules == {"plain", "stretch", "n-max"} and cut == {"ksplit", "tile"}
    # a K-split workgroup always owns a tile (grid = min(tiles, CUs)); a GEMV wave of a short chunk may own no row
    assert {1, 2} <= loads["ksplit"] and max(loads["ksplit"]) > 2 and 0 not in loads["ksplit"], loads["ksplit"]
    assert {0, 1, 2} <= loads["gemv"] and max(loads["gemv"]) > 2, loads["gemv"]
    assert any(x % 2 for x in loads["gemv"] if x > 2) and any(x % 2 == 0 for x in loads["gemv"] if x > 2)   # loop + tail, loop alone
    # the edges the table is there for
    assert {4, 100, 252, 256, 260, 384, 768, 1020, 1024} <= gemv_dims and {1, 2, 3} <= gemv_chunks and {1, 2, 3, 4} <= ks_chunks
    for d in KSPLIT_DIMS:
        assert {9, 32, 33, 64, 65, 96, 97, 128, 129, 200} <= {c.B for c in CASES if c.dim == d and c.mode == EXACT}, d
    ks_n = {c.n for c in CASES if c.dim in KSPLIT_DIMS and c.B > 8}
    assert {1, 20, 31, 32, 33, CURows(1, 0), CURows(1, 1), CURows(1, 32)} <= ks_n
    ks_depth = {c.depth for c in CASES if c.dim in KSPLIT_DIMS and c.B > 8}
    assert {1, 2, 1000, 1024} <= ks_depth and any(c.depth > c.n_rows(cus) for c in CASES if c.dim in KSPLIT_DIMS and c.B > 8)
    tile = [c for c in CASES if c.dim not in KSPLIT_DIMS and c.B > 8]
    assert {4, 32, 100, 1020} <= {c.dim for c in tile} and {9, 33, 64, 65, 97} <= {c.B for c in tile}
    assert {1, 127, 128, 129} <= {c.n for c in tile} and any(c.chunks == 2 for c in tile)
    assert {(32, 4096, N_NMAX), (32, 4096, N_CUT)} <= {(c.dim, c.B, c.n) for c in tile}
    assert (384, 4096, N_CUT) in {(c.dim, c.B, c.n) for c in CASES}
    for d in SPLIT_DIMS:
        assert {65, 97, 129} <= {c.B for c in CASES if c.dim == d and c.mode == SPLIT}, d      # (B <= 64: one group, by VARIANTS)
    assert {0, MAXB} <= {c.base for c in CASES} and {"rand", "ties"} <= {c.data for c in CASES}


def test_filtered_cases_reach_every_filt_family():
    """The filtered pass runs the GEMV at NQ 1, 4 and 8, the K-split at every dim x NQT, the tile kernel at both NQT, and a
    B = 97 search over two chunks (a filtered chunk against carried thresholds)."""
    seen = set()
    for name in FILTERED:
        c = BY_NAME[name]
        assert c.mode == EXACT and c.B < BIG_B, name
        seen |= set(kernel_of(c.dim, c.B, c.mode, filtered=True))
    want = {"gemv<1>", "gemv<4>", "gemv<8>", "tile<1>", "tile<2>"} | {"ksplit16<%d,%d>" % (d, t) for d in KSPLIT_DIMS for t in (1, 2)}
    assert want <= seen, sorted(want - seen)
    assert any(BY_NAME[x].B == 97 and BY_NAME[x].chunks == 2 for x in FILTERED)


# ==================================================================== GPU helpers
@pytest.fixture(scope="module")
def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def ctx():
    """One context per cosine mode, made on first use."""
    import openintel_amd as oi
    made = {}

    def get(mode):
        if mode not in made:
            made[mode] = oi.HipContext(0)
            made[mode].set_cosine_mode(mode)
        return made[mode]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import lib
    return lib


def _int_data(case: Case, n: int, chunks, seed: int):
    """Integer rows (int8) and queries (f32) of a case, with the adversaries of test_gpu_bf16_edges._int_data:
    * "ties": 7 distinct rows, repeated with skewed frequencies, the rarest one at both ends of every chunk -- many rows tie at the
      k-th score, copies of one row sit in every chunk and every segment, and the list must hold the lowest doc ids;
    * the queries of every second 64-query group in [-1, 1]: their thresholds sit well below the first group's, so a group
      filtered with another group's thresholds (a lost pool.for_queries offset) loses rows of their lists;
    * a zero query inside the batch (B >= 3): every row ties at 0;
    * a query whose top rows all sit in the LAST chunk (B >= 3, two chunks or more): the threshold carried from the earlier
      chunks has to give way."""
    rng = np.random.default_rng(seed)
    dim, B = case.dim, case.B
    if case.data == "ties":
        distinct = rng.integers(-3, 4, size=(7, dim)).astype(np.int8)
        pick = rng.choice(7, size=n, p=[0.002, 0.008, 0.04, 0.1, 0.2, 0.25, 0.4])
        for c in chunks:
            pick[c.begin] = 0
            pick[c.end - 1] = 0
        rows = distinct[pick]
        q = rng.integers(-3, 4, size=(B, dim)).astype(np.float32)
        q[1::3] = distinct[rng.integers(0, 7, size=q[1::3].shape[0])]      # queries equal to corpus rows
    else:
        rows = rng.integers(-3, 4, size=(n, dim)).astype(np.int8)
        q = rng.integers(-3, 4, size=(B, dim)).astype(np.float32)
    second = (np.arange(B) % 128) >= 64
    q[second] = rng.integers(-1, 2, size=(int(second.sum()), dim))
    if B >= 3:
        q[B // 2 + (1 if B >= 8 else 0)] = 0.0
    if B >= 3 and len(chunks) >= 2:
        last = chunks[-1]
        m = min(case.depth + 20, last.rows // 7)
        rows[last.end - 1 - 7 * np.arange(m)] = 3                           # score 3 x dim with the all-ones query: the top
        q[B - 1] = 1.0
    return rows, q


def _index(ctx, rows, terms, offs, base, attrs=None, screen_copy=None):
    import openintel_amd as oi
    idx = oi.HybridIndex(ctx, rows.shape[0], rows.shape[1], VOCAB, base)
    idx.set_embeddings(np.ascontiguousarray(rows, dtype=np.float32), normalize=False)
    if screen_copy is not None:
        idx.set_screen_copy(screen_copy)
    idx.set_forward(terms, offs)
    if attrs is not None:
        idx.set_doc_attrs(*attrs)
    idx.finalize()
    return idx


def _cos_lists_equal(O, L, rows, q, depth, base, tag, ok=None, block=256):
    """The cosine lists against the float64 reference, in blocks of queries (no B x n matrix for B = 4096); ok: [B, n] pass masks
    of a filtered search -- the reference ranking restricted to the passing rows, cut at depth."""
    for b0 in range(0, q.shape[0], block):
        with np.errstate(invalid="ignore"):
            S = _scores_f64(rows, q[b0:b0 + block])

        def one(i):
            if ok is None:
                return O.topk(S[i], depth, False, base)
            keep = np.nonzero(ok(b0 + i))[0]
            s, j = O.topk(S[i][keep], depth, False, 0)
            return s, (keep[j.astype(np.int64)] + base).astype(np.uint32)
        with _pool() as ex:
            ref = list(ex.map(one, range(S.shape[0])))
        for i, (cs, cd) in enumerate(ref):
            t = (tag, b0 + i)
            assert int(L.cos_counts[b0 + i]) == cd.size, t + (int(L.cos_counts[b0 + i]), cd.size)
            assert np.array_equal(L.cos_docs[b0 + i][:cd.size], cd), t
            assert np.array_equal(L.cos_scores[b0 + i][:cd.size].view(np.uint32), cs.view(np.uint32)), t


def _profiled_search(c, idx, q, qt, qo, depth, filters=None):
    """(lists, "cosine" spans, the gate word) of one search."""
    c.profile_reset(2)
    L = idx.search_lists(q, qt, qo, depth=depth, filters=filters)
    launches = int(c.profile_read("cosine")[1])
    gate = float(c.profile_read("screen_gate")[0])
    c.profile_reset(0)
    return L, launches, gate


def _case_inputs(case: Case, num_cus: int):
    n, base = case.n_rows(num_cus), case.doc_base(num_cus)
    chunks = case_chunks(case, num_cus)
    seed = 1013 * case.dim + 37 * case.B + n + case.mode
    rows, q = _int_data(case, n, chunks, seed)
    rng = np.random.default_rng(seed + 1)
    if case.B >= BIG_B:   # cosine only: no forward tokens, empty term lists
        terms, offs = np.zeros(1, dtype=np.uint32), np.zeros(n + 1, dtype=np.uint64)
        qt, qo = np.zeros(1, dtype=np.uint32), np.zeros(case.B + 1, dtype=np.uint32)
    else:
        terms, offs = _forward(rng, n)
        qt, qo = _query_terms(rng, case.B)
    return n, base, chunks, rows, q, terms, offs, qt, qo, rng


# ==================================================================== GPU: the table, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_exact_case_bit_exact(ctx, O, num_cus, case):
    c = ctx(case.mode)
    n, base, chunks, rows, q, terms, offs, qt, qo, _ = _case_inputs(case, num_cus)
    idx = _index(c, rows, terms, offs, base)
    L, launches, gate = _profiled_search(c, idx, q, qt, qo, case.depth)
    print(case.name, "cosine spans", launches, "chunks", [(ch.begin, ch.end, ch.rule, ch.cut) for ch in chunks], "gate", gate)
    assert launches == len(chunks), (case.name, launches, [(ch.begin, ch.end) for ch in chunks])
    if num_cus == MI355X_CUS:
        assert launches == case.chunks, (case.name, launches)
    assert gate == -1.0, "an exact-path search is not screened"
    if case.B >= BIG_B:
        idx.close()
        assert not L.bm25_counts.any()
        _cos_lists_equal(O, L, rows, q, case.depth, base, case.name)
        return
    R = idx.search(q, qt, qo, k=case.k, depth=case.depth)
    idx.close()
    ref = _oracle_lists(O, _scores_f64(rows, q), terms, offs, qt, qo, case.depth, case.k, base)
    _assert_lists(L, R, ref, case.name)


# ==================================================================== GPU: the FILT instantiations
@pytest.mark.gpu
@pytest.mark.parametrize("name", FILTERED)
def test_exact_case_filtered(ctx, O, num_cus, name):
    """The filter mix of test_gpu_filter._filters over a table case: cosine, BM25 and fused lists equal the reference ranking
    (float64 scores, the oracle's BM25) restricted to the passing rows and cut at depth."""
    from test_gpu_filter import _filters, _passes
    case = BY_NAME[name]
    c = ctx(EXACT)
    n, base, chunks, rows, q, terms, offs, qt, qo, rng = _case_inputs(case, num_cus)
    group = rng.integers(0, 1 << 16, size=n).astype(np.uint32)
    stamp = rng.permutation(n).astype(np.uint32) * 3
    F = _filters(case.B, group, seed=case.B + case.dim)
    idx = _index(c, rows, terms, offs, base, attrs=(group, stamp))
    L, launches, gate = _profiled_search(c, idx, q, qt, qo, case.depth, filters=F)
    assert launches == len(chunks) and gate == -1.0, (name, launches, gate)
    R = idx.search(q, qt, qo, k=case.k, depth=case.depth, filters=F)
    idx.close()

    def ok(b):
        return _passes(F[b], group, stamp)
    _cos_lists_equal(O, L, rows, q, case.depth, base, name, ok=ok)
    for b in range(case.B):
        keep = np.nonzero(ok(b))[0]
        bm = O.bm25_scores(terms, offs, VOCAB, qt[qo[b]:qo[b + 1]])
        bs, j = O.topk(bm[keep], case.depth, True, 0)
        bd = (keep[j.astype(np.int64)] + base).astype(np.uint32)
        assert int(L.bm25_counts[b]) == bd.size and np.array_equal(L.bm25_docs[b][:bd.size], bd), (name, b)
        assert np.array_equal(L.bm25_scores[b][:bd.size].view(np.uint32), bs.view(np.uint32)), (name, b)
        fs, fd = O.rrf_fuse(L.cos_docs[b][:int(L.cos_counts[b])], bd, case.k)
        assert int(R.counts[b]) == fd.size and np.array_equal(R.docs[b][:fd.size], fd), (name, b)
        assert np.array_equal(R.scores[b][:fd.size].view(np.uint32), fs.view(np.uint32)), (name, b)


# ==================================================================== GPU: the gated fallback with more than one group
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [384, 768])
@pytest.mark.parametrize("B", [65, 97, 129])
def test_gated_fallback_groups(ctx, O, num_cus, dim, B):
    """OI_COSINE_SCREEN with a zero query in the last 64-query group: that query has no bound, the gate opens, and the exact
    pipeline (run_gate, first = max_chunk, the screen's thresholds as tau_keys) rescores the whole batch: every list is the
    oracle's bit for bit."""
    c = ctx(SCREEN)
    n, depth, k, base = 20_011, 100, 20, 5
    case = Case("gated", dim, B, n, depth, k, base, "rand", SCREEN, frozenset(), 1)
    chunks = exact_schedule(n, B, depth, num_cus, first=exact_pool(n, B, num_cus)[1])
    rows, q = _int_data(case, n, chunks, 7 * dim + B)
    q[B // 2 + 1] = rows[3]                               # (the zero query of _int_data moves to the last group)
    q[B - 1] = 0.0
    rng = np.random.default_rng(dim + B)
    terms, offs = _forward(rng, n)
    qt, qo = _query_terms(rng, B)
    idx = _index(c, rows, terms, offs, base)
    assert idx.index_bytes()[1] >= 2 * n * dim, "the index holds a screening copy: the search is screened"
    c.profile_reset(1)
    L = idx.search_lists(q, qt, qo, depth=depth)
    gated = int(c.profile_read("cosine_gated")[1])
    gate = float(c.profile_read("screen_gate")[0])
    c.profile_reset(0)
    R = idx.search(q, qt, qo, k=k, depth=depth)
    idx.close()
    assert gate not in (0.0, -1.0), gate
    assert gated == len(chunks) >= 1, (gated, chunks)
    _assert_lists(L, R, _oracle_lists(O, _scores_f64(rows, q), terms, offs, qt, qo, depth, k, base), ("gated", dim, B))


# ==================================================================== GPU: non-finite rows
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [384, 100, 1024, 4])
def test_non_finite_rows_rank_as_ieee_orders_them(ctx, O, dim):
    """Exact mode.  A few rows hold one +inf, -inf or NaN coordinate (first, middle and last positions of the row -- the last four
    included -- in the first, middle and last rows of the corpus).  The rule (openintel_hip.h, oi_search_lists): a row whose score
    is NaN is never listed, +-inf ranks as IEEE orders it.  The reference is the float64 matmul (inf x 0 = NaN there too).  The
    same batch runs at B = 8 (the GEMV, whose lanes past the row's end re-read the row's last float4: dim / 4 is not a multiple
    of 64 at d = 384, 100 and 4) and at B = 9 (the K-split at 384 / 1024, the tile kernel at 100 / 4); depth > n lists every row
    that has a score."""
    c = ctx(EXACT)
    n, depth = 900, 1024
    rng = np.random.default_rng(dim)
    rows = rng.integers(-3, 4, size=(n, dim)).astype(np.float32)
    coords = [0, dim // 2, dim - 4, dim - 3, dim - 2, dim - 1]
    special = [0, 1, 2, 3, 4, 5, n // 2 - 1, n // 2, n // 2 + 1, n // 2 + 2, n - 6, n - 5, n - 4, n - 3, n - 2, n - 1]
    vals = [np.inf, -np.inf, np.nan]
    for i, r in enumerate(special):
        rows[r, coords[i % len(coords)]] = vals[(i // 2) % 3]
    q = rng.integers(-3, 4, size=(9, dim)).astype(np.float32)
    q[0] = rng.choice(np.array([-3, -2, -1, 1, 2, 3], dtype=np.float32), size=dim)      # no zero: every inf row has a score
    q[1, coords] = 0.0                                                                  # every special row scores NaN
    q[2] = np.abs(q[0])
    q[3, coords[2:]] = 0.0
    q[8] = -q[0]
    terms, offs = _forward(rng, n)
    idx = _index(c, rows, terms, offs, 0, screen_copy=1)     # (_lib.OI_SCREEN_COPY_NEVER: no quantised copy of these rows)
    qo = np.zeros(10, dtype=np.uint32)
    with np.errstate(invalid="ignore"):
        S = _scores_f64(rows, q)
    assert np.isinf(S[0]).any() and np.isnan(S[1][special]).all()
    try:
        for B in (8, 9):
            L = idx.search_lists(q[:B], np.zeros(1, dtype=np.uint32), qo[:B + 1], depth=depth)
            _cos_lists_equal(O, L, rows, q[:B], depth, 0, ("non-finite", dim, B))
    finally:
        idx.close()
