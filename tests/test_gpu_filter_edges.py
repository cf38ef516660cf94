"""Filtered search (oi_search*_filtered) bit for bit at every screen-route, chunk, group, long-row and gate edge.

A filtered search does not run the unfiltered code with one more test: every route is compiled a second time with FILT = true
(cosine_i8_screen, cosine_copy_screen, cosine_bf16_filter, the exact kernels, bm25_stream_kernel, a branch of pf_rescore_kernel),
and the filter changes the plan -- no speculation and no sample pass (the proven x 8 schedule, the first chunk never grown),
a bf16 corpus pinned to the solo kernel in passes of 64 queries (32 at d = 1024), BM25 through the stream kernel without floors.
The exact kernels and the BM25 stream kernel run their filtered forms in their own edge modules; this one holds the three
screened / bf16 routes, the rescoring of long rows and the gated exact pipeline under a filter.

CASES_* below are the tables of what this module runs.  A pure-Python mirror of the rules that decide chunks and kernels under a
filter (`filtered_bf16_schedule`, `filtered_screen_chunks`; the unfiltered mirrors are imported from the sibling modules) gives
each case's chunks, passes and kernels; CPU tests hold the tables to the mirror at 256 CUs and to reaching every FILT
instantiation with two chunks or more, and hold the filters to the conditions the cases rely on.  On the GPU every case proves
its route through the profiler (one "cosine" span per chunk and search, the "screen_gate" it declares, the planted long rows,
the screening copies the index holds).

Data: rows are integers in {-1, 0, 1} (never all zero), queries integers in [-2, 2]: exact in int8, bf16 and f32 in any order.
The cosine reference is ONE float64 matmul (test_int_matmul_equals_oracle_dot_scores), restricted to the rows that pass the
query's filter, cut at depth with ties to the lower doc id and cast to f32; BM25 is the oracle's bm25_scores restricted the same
way, the fused lists its rrf_fuse.  Cosine docs and scores, BM25 docs and scores, counts and fused lists are compared bit for
bit: no tolerance appears in this module.  Every query of every case has a filter of its own, drawn from KINDS.

Two departures from "small integers" that the library's rules force, both exact all the same:
  * an index looks for long rows only where bf16 rounds (api.hip: E0 > 0), so the long-row cases scale every row by 1 + 2^-9 and
    the long ones by 64 more: every product is a multiple of 2^-9 and every partial sum stays far below 2^24 of those;
  * the carry cases plant rows with one coordinate of 254: their int8 scale is 2, so their +-1 coordinates round away and the
    int8 tier cannot tell them apart while both second tiers can (test_gpu_select_i8_margin's recipe on integers)."""
from typing import NamedTuple

import numpy as np
import pytest

from test_gpu_bf16_edges import (_bf16_index, _int_bits, _pool, _query_terms, _scores_f64, bf16_geometry, bf16_pool, chunk_end,  # noqa: F401
                                 chunk_growth, first_chunk_rows, schedule)
from test_gpu_filter import _filters, _passes
from test_gpu_screen_i8_edges import (OI_I8_CARRY, VOCAB, _forward, _index, chunk_schedule, listed, plan, query_groups,
                                      screen_first_chunk_rows, screen_geometry, screen_pool)

MI355X_CUS = 256          # what the tables' declared schedules assume (the GPU tests read the real count)
OI_LONG_ROWS_MAX = 1024   # oi_internal.h
PF_CARRY_COPY = 4096      # search.hip, plan_search: keys per query the copy screen carries between chunks
TILE = 32
MAXB = -1                 # doc_id_base = 2^32 - 1 - n: the last doc id is 2^32 - 2
K_FUSED = 10


# ==================================================================== mirror: what a filter changes in the plan
def solo_group(dim: int) -> int:
    """cosine_bf16.hip, oi_launch_cosine_bf16_chunk (`filtered`): queries of one pass of a filtered search."""
    return 32 if dim == 1024 else 64


def filtered_bf16_passes(dim: int, B: int):
    """The passes of one chunk of a filtered search over a bf16 corpus: [(kernel, q0, queries)] in launch order.  Every pass is
    the solo kernel (the only one with the doc filter), its pool view moved by q0 (PoolView::for_queries: keys, counters,
    thresholds and `filt`)."""
    out, q0 = [], 0
    while q0 < B:
        nq = min(solo_group(dim), B - q0)
        out.append(("solo<%d,%d>" % (dim, (nq + TILE - 1) // TILE), q0, nq))
        q0 += nq
    return out


def filtered_bf16_schedule(n: int, dim: int, B: int, depth: int, num_cus: int):
    """[(begin, end, kernels)]: the chunks are the unfiltered search's (search.hip, cosine_bf16: a function of the sizes alone,
    chunk_schedule with stretch_first = true), the kernels of each are filtered_bf16_passes', never siblings."""
    kernels = tuple(k for k, _, _ in filtered_bf16_passes(dim, B))
    return [(ch.begin, ch.end, kernels) for ch in schedule(n, dim, B, depth, num_cus)]


def filtered_screen_chunks(n: int, B: int, depth: int, num_cus: int, pf_carry: int):
    """search.hip, plan_search under a filter: no speculation and no sample pass whatever B, so the proven schedule -- the
    rounded first chunk, then x 8 (x 16 for B <= 8).  stretch_first = false: the threshold-less first chunk is never GROWN so
    that the last chunk is the largest the pool takes (oi_chunk_end's second rule); a tail of at most a quarter of it is taken
    along all the same (its first rule), so 8 193 rows are ONE chunk and 10 241 the smallest corpus with two."""
    _, pool_max = screen_pool(n, B, num_cus, pf_carry)
    return tuple(chunk_schedule(n, screen_first_chunk_rows(depth, num_cus), chunk_growth(B), pool_max, stretch_first=False))


def screen_route(B: int) -> str:
    """plan_search on an f32 index that holds both screening copies, default mode."""
    return "i8" if B > 8 else "copy"


# ==================================================================== filters
KINDS = ("all", "sparse-chunk-1", "half", "last-chunk", "sixteenth", "last-tile", "one-in-4096", "none", "window", "lo==hi")


def make_attrs(n: int, stamps: str, seed: int):
    """group: random 16-bit; stamp: arange ("arange": a stamp window is a row range) or a permutation times 3 ("perm")."""
    rng = np.random.default_rng(seed)
    group = rng.integers(0, 1 << 16, size=n).astype(np.uint32)
    stamp = np.arange(n, dtype=np.uint32) if stamps == "arange" else rng.permutation(n).astype(np.uint32) * 3
    return group, stamp


def make_filters(B: int, group, stamps: str, depth: int, chunks, seed: int) -> np.ndarray:
    """Query b gets kind KINDS[b % 10], with values of its own:
    all; FEWER than depth rows of chunk 1 and everything after it ("sparse-chunk-1": with more than depth rows after chunk 1 the
    query reaches chunk 2 with an open threshold); 1/2 of the groups; only the last chunk; 1/16; only the rows of the last
    32-row tile; 1/4096; none; a stamp window; lo == hi.  (Row ranges are stamp windows: exact under "arange" stamps.)"""
    rng = np.random.default_rng(seed)
    n = group.size
    u = 1 if stamps == "arange" else 3
    c1, last = chunks[0][1], chunks[-1][0]
    r0 = int(rng.integers(0, n))
    out = []
    for b in range(B):
        kind, j = KINDS[b % len(KINDS)], b // len(KINDS)
        top = 0xFFFFFFFF - b          # (an upper stamp bound above every stamp, every query with one of its own)
        if kind == "all":
            f = (0, 0, 0, top)
        elif kind == "sparse-chunk-1":
            m = min(c1, max(1, depth // 2) + j)
            f = (0, 0, (c1 - m) * u, top)
        elif kind == "half":
            f = (1, int(rng.integers(0, 2)), 0, top)
        elif kind == "last-chunk":
            f = (0, 0, last * u, top)
        elif kind == "sixteenth":
            f = (0xF, int(rng.integers(0, 16)), 0, top)
        elif kind == "last-tile":
            f = (0, 0, TILE * ((n - 1) // TILE) * u, top)
        elif kind == "one-in-4096":
            f = (0xFFF, int(group[rng.integers(0, n)]) & 0xFFF, 0, top)
        elif kind == "none":
            f = (0xFFFFFFFF, 0xFFFFFFFF - j, 0, top) if j % 2 else (0, 0, 7 + j, 6 + j)
        elif kind == "window":
            lo = int(rng.integers(0, max(1, n // 2)))
            f = (0, 0, lo * u, (lo + max(1, n // 4) + j) * u)
        else:
            r = (r0 + 7 * j) % n * u
            f = (0, 0, r, r)
        out.append(f)
    return np.array(out, dtype=np.uint32)


# ==================================================================== the case tables
class Case(NamedTuple):
    name: str
    route: str            # "bf16", "i8" or "copy"
    dim: int
    B: int
    n: int
    depth: int
    base: int             # doc_id_base (MAXB: 2^32 - 1 - n)
    stamps: str           # "arange" or "perm"
    chunks: int           # declared for 256 CUs (the mirror, checked on the CPU; the profiler on the GPU)
    kernels: tuple        # bf16: the kernel of every pass; i8: the NQT of every 64-query group; copy: ()
    hybrid: bool = False  # also search(..., filters=F): the fused lists

    def doc_base(self) -> int:
        return 2 ** 32 - 1 - self.n if self.base == MAXB else self.base


N1, N2 = 10_240, 10_241                # depth 10, chunk_schedule(stretch_first = true): the largest one-chunk and smallest two-chunk n
N3 = 8192 + 65_536 + 16_385            # three chunks; one row fewer and the third is taken along with the second
S1, S2 = 8192, 8193                    # the screens' first chunk alone, and with a one-row tail (taken along: still ONE chunk)
S3 = N2                                # ... and the smallest corpus with a second screen chunk: a tail longer than a quarter


def _s(dim, *nqt):
    return tuple("solo<%d,%d>" % (dim, t) for t in nqt)


CASES_BF16 = [
    Case("bf16-d384-B9-2chunks", "bf16", 384, 9, N2, 10, 0, "arange", 2, _s(384, 1), hybrid=True),
    Case("bf16-d384-B33-2chunks", "bf16", 384, 33, N2, 10, 7, "arange", 2, _s(384, 2)),
    Case("bf16-d384-B64-1chunk", "bf16", 384, 64, N1, 10, 0, "arange", 1, _s(384, 2)),
    Case("bf16-d384-B65-3chunks", "bf16", 384, 65, N3, 10, 1000, "arange", 3, _s(384, 2, 1)),
    Case("bf16-d768-B32-2chunks", "bf16", 768, 32, N2, 10, 0, "arange", 2, _s(768, 1)),
    Case("bf16-d768-B64-2chunks-maxbase", "bf16", 768, 64, N2, 10, MAXB, "arange", 2, _s(768, 2)),
    Case("bf16-d768-B65-2chunks", "bf16", 768, 65, N2, 10, 5, "arange", 2, _s(768, 2, 1)),
    Case("bf16-d1024-B9-2chunks", "bf16", 1024, 9, N2, 10, 0, "arange", 2, _s(1024, 1)),
    Case("bf16-d1024-B33-2chunks", "bf16", 1024, 33, N2, 10, 3, "arange", 2, _s(1024, 1, 1)),
    Case("bf16-d1024-B97-2chunks", "bf16", 1024, 97, N2, 10, 0, "arange", 2, _s(1024, 1, 1, 1, 1), hybrid=True),
    Case("bf16-d1024-B32-1chunk", "bf16", 1024, 32, N1, 10, 0, "perm", 1, _s(1024, 1)),
    # ---- a ragged single tile, depth > n
    Case("bf16-d384-B9-n1", "bf16", 384, 9, 1, 100, MAXB, "arange", 1, _s(384, 1)),
    Case("bf16-d1024-B33-n31", "bf16", 1024, 33, 31, 100, 0, "arange", 1, _s(1024, 1, 1)),
    Case("bf16-d384-B33-n32", "bf16", 384, 33, 32, 100, 0, "perm", 1, _s(384, 2)),
    Case("bf16-d768-B65-n33", "bf16", 768, 65, 33, 100, 9, "arange", 1, _s(768, 2, 1)),
]
CASES_I8 = [
    Case("i8-d384-B9-2chunks", "i8", 384, 9, S3, 10, 0, "arange", 2, (1,), hybrid=True),
    Case("i8-d384-B64-tail-of-one-row", "i8", 384, 64, S2, 10, 0, "arange", 1, (2,)),
    Case("i8-d384-B33-3chunks", "i8", 384, 33, N3, 10, 7, "arange", 3, (2,)),
    Case("i8-d384-B65-1chunk", "i8", 384, 65, S1, 10, 0, "perm", 1, (2, 1)),
    Case("i8-d384-B129-2chunks-maxbase", "i8", 384, 129, S3, 100, MAXB, "arange", 2, (2, 2, 1)),
    Case("i8-d768-B9-third-taken-along", "i8", 768, 9, N3 - 1, 10, 0, "arange", 2, (1,)),
    Case("i8-d768-B33-2chunks", "i8", 768, 33, S3, 10, 11, "arange", 2, (2,)),
    Case("i8-d768-B64-2chunks", "i8", 768, 64, S3, 100, 0, "arange", 2, (2,)),
    Case("i8-d768-B129-3chunks", "i8", 768, 129, N3, 10, 5, "arange", 3, (2, 2, 1)),
]
# the copy screen (B <= 8): growth x 16, two chunks; test_gpu_copy_screen_edges.py has the rest of the route
CASES_COPY = [
    Case("copy-d384-B1", "copy", 384, 1, S3 + 32, 10, 0, "arange", 2, ()),
    Case("copy-d384-B8", "copy", 384, 8, S3 + 32, 10, 3, "arange", 2, (), hybrid=True),
    Case("copy-d768-B1", "copy", 768, 1, S3 + 32, 10, MAXB, "arange", 2, ()),
    Case("copy-d768-B8", "copy", 768, 8, S3 + 32, 10, 0, "arange", 2, ()),
]
CASES = CASES_BF16 + CASES_I8 + CASES_COPY


def case_chunks(c: Case, num_cus: int):
    """((begin, end), ...) of the case's filtered search."""
    if c.route == "bf16":
        return tuple((r, e) for r, e, _ in filtered_bf16_schedule(c.n, c.dim, c.B, c.depth, num_cus))
    return filtered_screen_chunks(c.n, c.B, c.depth, num_cus, OI_I8_CARRY if c.route == "i8" else PF_CARRY_COPY)


def case_seed(c: Case) -> int:
    return 7919 * c.dim + 131 * c.B + c.n


def case_attrs_filters(c: Case, num_cus: int):
    group, stamp = make_attrs(c.n, c.stamps, case_seed(c) + 1)
    F = make_filters(c.B, group, c.stamps, c.depth, case_chunks(c, num_cus), case_seed(c) + 2)
    return group, stamp, F


# ---- long rows under a filter (pf_rescore_kernel): (name, B, planted long rows, doc_id_base)
class LongCase(NamedTuple):
    name: str
    B: int
    n_long: int
    base: int


N_LONG_CORPUS, LONG_DIM, LONG_DEPTH = 4200, 384, 100     # an index sets rows aside only when it has more than 4096
LONG_CASES = [
    LongCase("long1-B9", 9, 1, 0), LongCase("long63-B33", 33, 63, 7), LongCase("long64-B9", 9, 64, 1000),
    LongCase("long65-B33", 33, 65, 0), LongCase("long129-B9", 9, 129, MAXB), LongCase("long129-B33", 33, 129, 0),
    LongCase("long1024-B9", 9, OI_LONG_ROWS_MAX, 0), LongCase("long1024-B33", 33, OI_LONG_ROWS_MAX, 12_345),
]
# pass / fail patterns over the long rows IN THE ORDER OF long_list, which pf_rescore_kernel's long_passing(j) counts in ballots of
# 64: name -> (group mask, group value, does the long row at position i pass).  A long row's group carries bit 4 (it is long),
# bit 0 = i odd, bit 1 = (i == 63), bit 2 = (i == 64), bit 3 = (i >= 64); the other rows' groups are random, bit 4 included, so
# every pattern also passes a share of the ordinary rows and the long rows have to take their places among them.
LONG_PATTERNS = {
    "none": (0x10, 0x00, lambda i: False),
    "all": (0x10, 0x10, lambda i: True),
    "only-63": (0x12, 0x12, lambda i: i == 63),
    "only-64": (0x14, 0x14, lambda i: i == 64),
    "alternating": (0x11, 0x11, lambda i: i % 2 == 1),
    "first-64-fail": (0x18, 0x18, lambda i: i >= 64),
}


def long_attrs(n: int, long_list, seed: int):
    """group and stamp of a long-row case, given the index's long_list (local rows, in its order)."""
    rng = np.random.default_rng(seed)
    group = rng.integers(0, 1 << 16, size=n).astype(np.uint32)
    stamp = rng.permutation(n).astype(np.uint32) * 3
    i = np.arange(len(long_list), dtype=np.uint32)
    bits = np.uint32(0x10) | (i & 1) | ((i == 63).astype(np.uint32) << 1) | ((i == 64).astype(np.uint32) << 2) | ((i >= 64).astype(np.uint32) << 3)
    group[np.asarray(long_list, dtype=np.int64)] = (group[np.asarray(long_list, dtype=np.int64)] & np.uint32(0xFFE0)) | bits
    return group, stamp


def long_filters(B: int, group, seed: int) -> np.ndarray:
    """The six patterns first (every case has B >= 9), then test_gpu_filter's mix for the other queries."""
    F = _filters(B, group, seed=seed)
    for b, (mask, value, _) in enumerate(LONG_PATTERNS.values()):
        for bb in range(b, B, 11):
            F[bb] = (mask, value, 0, 0xFFFFFFFF)
    return F


# ==================================================================== data
_ROWS = {}


def int_rows(n: int, dim: int) -> np.ndarray:
    """Seeded int8 rows of {-1, 0, 1}, never all zero, generated once per dim (the largest corpus of that dim) and cut."""
    have = _ROWS.get(dim)
    if have is None or have.shape[0] < n:
        want = max([c.n for c in CASES if c.dim == dim] + [n])
        have = np.random.default_rng(6100 + dim).integers(-1, 2, size=(want, dim)).astype(np.int8)
        have[:, 0] = np.where(np.abs(have).sum(axis=1) == 0, 1, have[:, 0])
        have.setflags(write=False)
        _ROWS[dim] = have
    return have[:n]


def int_queries(B: int, dim: int, seed: int) -> np.ndarray:
    q = np.random.default_rng(6200 + seed).integers(-2, 3, size=(B, dim)).astype(np.float32)
    q[:, 0] = np.where(np.abs(q).sum(axis=1) == 0, 1.0, q[:, 0])
    return q


def ref_cosine(s_b, ok, depth: int, base: int):
    """(scores, doc ids) of the passing rows' top `depth`, ties to the lower doc id."""
    rows = np.flatnonzero(ok)
    order = np.argsort(-s_b[rows].astype(np.float64), kind="stable")[:depth]
    return s_b[rows][order].astype(np.float32), (rows[order].astype(np.int64) + base).astype(np.uint32)


def ref_lists(O, S, fwd, qt, qo, F, group, stamp, depth, k, base, queries):
    """{b: (cos scores, cos docs, bm25 scores, bm25 docs, fused scores, fused docs)}.  (The oracle's C calls release the GIL.)"""
    terms, offs = fwd

    def one(b):
        ok = _passes(F[b], group, stamp)
        cs, cd = ref_cosine(S[b], ok, depth, base)
        bm = np.where(ok, O.bm25_scores(terms, offs, VOCAB, qt[qo[b]:qo[b + 1]]), 0).astype(np.float32)
        bs, bd = O.topk(bm, depth, True, base)
        fs, fd = O.rrf_fuse(cd, bd, k)
        return b, (cs, cd, bs, bd, fs, fd)
    with _pool() as ex:
        return dict(ex.map(one, queries))


def assert_lists(L, R, ref, tag):
    for b, (cs, cd, bs, bd, fs, fd) in ref.items():
        t = (tag, b)
        assert int(L.cos_counts[b]) == cd.size, t + (int(L.cos_counts[b]), cd.size)
        assert np.array_equal(L.cos_docs[b][:cd.size], cd), t
        assert np.array_equal(L.cos_scores[b][:cd.size].view(np.uint32), cs.view(np.uint32)), t
        assert int(L.bm25_counts[b]) == bd.size, t
        assert np.array_equal(L.bm25_docs[b][:bd.size], bd), t
        assert np.array_equal(L.bm25_scores[b][:bd.size].view(np.uint32), bs.view(np.uint32)), t
        if R is not None:
            assert int(R.counts[b]) == fd.size and np.array_equal(R.docs[b][:fd.size], fd), t
            assert np.array_equal(R.scores[b][:fd.size].view(np.uint32), fs.view(np.uint32)), t


# ==================================================================== CPU: the tables against the mirrors
def test_case_table_reaches_every_filtered_instantiation():
    """At 256 CUs every case runs the chunks and kernels it declares; the tables reach every FILT instantiation of the three
    routes with two chunks or more, and hold every B and n edge."""
    names, two = set(), {"bf16": set(), "i8": set(), "copy": set()}
    for c in CASES:
        assert c.name not in names, c.name
        names.add(c.name)
        assert 1 <= c.depth <= 1024 and 0 <= c.doc_base() and c.doc_base() + c.n <= 2 ** 32 - 1, c.name
        ch = case_chunks(c, MI355X_CUS)
        assert ch[0][0] == 0 and ch[-1][1] == c.n and all(a[1] == b[0] for a, b in zip(ch, ch[1:])), c.name
        assert len(ch) == c.chunks, (c.name, ch)
        if c.route == "bf16":
            sched = filtered_bf16_schedule(c.n, c.dim, c.B, c.depth, MI355X_CUS)
            assert all(k == c.kernels for _, _, k in sched), (c.name, sched[0][2])
            passes = filtered_bf16_passes(c.dim, c.B)
            assert [q0 for _, q0, _ in passes] == list(range(0, c.B, solo_group(c.dim))) and sum(nq for _, _, nq in passes) == c.B
            stride, max_chunk = bf16_pool(c.n, c.B, MI355X_CUS)
            for r, e in ch:     # the launcher's OI_REQUIRE: a filtered chunk takes the solo geometry, never the siblings'
                segs, cap = bf16_geometry(e - r, MI355X_CUS, False)
                assert e - r <= max_chunk and 1024 + segs * cap <= stride, (c.name, r, e)
            kinds = set(c.kernels)
        else:
            assert screen_route(c.B) == c.route, c.name
            carry = OI_I8_CARRY if c.route == "i8" else PF_CARRY_COPY
            # the filtered plan IS the unfiltered proven plan: plan_search takes the speculation away and nothing else
            assert ch == plan(c.n, c.B, c.depth, MI355X_CUS, spec=False, pf_carry=carry).chunks, c.name
            stride, pool_max = screen_pool(c.n, c.B, MI355X_CUS, carry)
            for r, e in ch:
                segs, cap = screen_geometry(e - r, MI355X_CUS)
                assert e - r <= pool_max and carry + segs * cap <= stride, (c.name, r, e)
            if c.route == "i8":
                assert query_groups(c.B) == c.kernels, (c.name, query_groups(c.B))
                kinds = {"i8<%d,%d>" % (c.dim, t) for t in c.kernels}
            else:
                assert c.kernels == ()
                kinds = {"copy<%d,B%d>" % (c.dim, c.B)}
        if len(ch) >= 2:
            two[c.route] |= kinds
    assert two["bf16"] >= {"solo<384,1>", "solo<384,2>", "solo<768,1>", "solo<768,2>", "solo<1024,1>"}, two["bf16"]
    assert two["i8"] >= {"i8<384,1>", "i8<384,2>", "i8<768,1>", "i8<768,2>"}, two["i8"]
    assert two["copy"] >= {"copy<384,B1>", "copy<384,B8>", "copy<768,B1>", "copy<768,B8>"}, two["copy"]
    # ---- bf16: the B and n edges; two passes at 384 / 768 (64 + 1), two and four at 1024 (32 + 1, 32 + 32 + 32 + 1)
    bf = CASES_BF16
    assert {9, 32, 33, 64, 65} <= {c.B for c in bf} and {33, 97} <= {c.B for c in bf if c.dim == 1024}
    assert all(any(c.B == 65 and c.dim == d and c.chunks >= 2 for c in bf) for d in (384, 768))
    assert {1, 31, 32, 33, N1, N2} <= {c.n for c in bf} and all(c.depth > c.n for c in bf if c.n <= 33)
    assert any(c.dim == 384 and c.chunks == 3 for c in bf) and any(c.base == MAXB for c in bf)
    assert len(schedule(N1, 384, 9, 10, MI355X_CUS)) == 1 and len(schedule(N2, 384, 9, 10, MI355X_CUS)) == 2
    # ---- int8: B, n; the corpus of one row fewer than the three-chunk one has two chunks
    i8 = CASES_I8
    assert {9, 33, 64, 65, 129} <= {c.B for c in i8} and {S1, S2, S3, N3, N3 - 1} <= {c.n for c in i8}
    assert {c.chunks for c in i8 if c.n == N3} == {3} and {c.chunks for c in i8 if c.n == N3 - 1} == {2}
    assert {c.chunks for c in i8 if c.n in (S1, S2)} == {1} and {c.chunks for c in i8 if c.n == S3} == {2}
    assert any(c.base == MAXB for c in i8) and any(len(c.kernels) >= 3 for c in i8)
    # the proven schedule's "first chunk never grown" changes a schedule only where the pool is smaller than the second chunk:
    # no corpus of this module's sizes, so the mirror is held to it at a shape no case runs (2 048 queries, depth 1000: the pool
    # takes 163 712 rows, less than 8 x 28 672; a first chunk under the rule for later chunks would end at n - 163 712)
    wide = filtered_screen_chunks(300_000, 2048, 1000, MI355X_CUS, OI_I8_CARRY)
    assert screen_pool(300_000, 2048, MI355X_CUS, OI_I8_CARRY)[1] == 163_712 and wide[0] == (0, 28_672), wide
    assert wide == plan(300_000, 2048, 1000, MI355X_CUS, spec=False).chunks
    # ---- one hybrid check per route
    assert all(any(c.hybrid for c in t) for t in (CASES_BF16, CASES_I8, CASES_COPY))
    # ---- long rows and the carry cases
    assert {c.n_long for c in LONG_CASES} == {1, 63, 64, 65, 129, OI_LONG_ROWS_MAX} and {c.B for c in LONG_CASES} == {9, 33}
    assert any(c.base == 0 for c in LONG_CASES) and any(c.base != 0 for c in LONG_CASES)
    assert N_LONG_CORPUS > 4 * OI_LONG_ROWS_MAX and len(filtered_screen_chunks(N_LONG_CORPUS, 9, LONG_DEPTH, MI355X_CUS, OI_I8_CARRY)) == 1
    first = filtered_screen_chunks(CARRY_N, CARRY_B, CARRY_DEPTH, MI355X_CUS, OI_I8_CARRY)
    assert len(first) == 2 and first[0][1] >= OI_I8_CARRY + 1 + CARRY_FAIL, "the planted rows all fit the first chunk"


def test_filters_meet_the_conditions_the_cases_rely_on():
    """From the data alone.  Every multi-chunk case under "arange" stamps: at least two queries with FEWER than depth passing
    rows inside chunk 1 and MORE than depth overall (they reach chunk 2 with an open threshold, the others with a carried one),
    and a query that passes more than depth rows inside chunk 1.  Every case: a "last-tile" query passes only rows of the last
    32-row tile (so its reference list lies entirely there) and passes at least one; a none-pass query passes nothing; every
    query's filter differs from every other's."""
    for c in CASES:
        group, stamp, F = case_attrs_filters(c, MI355X_CUS)
        ch = case_chunks(c, MI355X_CUS)
        assert len({tuple(f) for f in F.tolist()}) == c.B, c.name
        ok = np.stack([_passes(F[b], group, stamp) for b in range(c.B)])
        in1, total = ok[:, :ch[0][1]].sum(axis=1), ok.sum(axis=1)
        if len(ch) >= 2 and c.stamps == "arange" and c.n - ch[0][1] > c.depth:
            opened = int(((in1 < c.depth) & (total > c.depth)).sum())
            assert opened >= min(2, c.B // 2), (c.name, opened)         # (B = 1: the copy screen's one query passes everything)
            assert (in1 > c.depth).any(), c.name
        assert c.route != "bf16" or len(ch) < 2 or c.n - ch[0][1] > c.depth, (c.name, "a bf16 multi-chunk case must open thresholds")
        for b in range(c.B):
            kind = KINDS[b % len(KINDS)]
            if kind == "none":
                assert total[b] == 0, (c.name, b)
            if kind == "all":
                assert total[b] == c.n, (c.name, b)
            if kind == "last-tile" and c.stamps == "arange":
                rows = np.flatnonzero(ok[b])
                assert rows.size == c.n - TILE * ((c.n - 1) // TILE) and rows.min() >= TILE * ((c.n - 1) // TILE), (c.name, b)
                _, cd = ref_cosine(np.zeros(c.n, np.float32), ok[b], c.depth, 0)
                assert cd.size and cd.min() >= TILE * ((c.n - 1) // TILE), (c.name, b)


def test_long_row_patterns_are_present():
    """Whatever order the index lists its long rows in (here: a seeded permutation), long_attrs and long_filters give every named
    pattern over the long rows in that order -- none, all, only position 63, only position 64, alternating, the first 64 fail and
    the rest pass -- and each pattern also passes ordinary rows."""
    for c in LONG_CASES:
        rng = np.random.default_rng(c.n_long)
        long_list = rng.permutation(N_LONG_CORPUS)[:c.n_long]
        group, stamp = long_attrs(N_LONG_CORPUS, long_list, 1)
        F = long_filters(c.B, group, 2)
        is_long = np.zeros(N_LONG_CORPUS, bool)
        is_long[long_list] = True
        for b, (name, (_, _, want)) in enumerate(LONG_PATTERNS.items()):
            ok = _passes(F[b], group, stamp)
            assert np.array_equal(ok[long_list], np.array([want(i) for i in range(c.n_long)])), (c.name, name)
            assert ok[~is_long].sum() > LONG_DEPTH, (c.name, name)
    # the positions the ballots of long_passing turn on exist where the count allows them
    assert LONG_PATTERNS["only-63"][2](63) and not LONG_PATTERNS["only-63"][2](64) and LONG_PATTERNS["only-64"][2](64)


def test_int_matmul_equals_oracle_dot_scores():
    """The module's cosine reference (a float64 matmul) is the oracle's dot_scores bit for bit on each kind of row it uses:
    {-1, 0, 1}, those scaled by 1 + 2^-9 with long rows 64 times that, and a carry case's planted rows."""
    from oracle import lib as O
    q = int_queries(4, 384, 1)
    plain = int_rows(3000, 384).astype(np.float32)
    scaled = long_rows_matrix(3000, np.arange(0, 3000, 7))
    planted = plain.copy()
    planted[:50] = carry_row(q[0], 8)
    planted[50:90] = carry_row(q[0], 4)
    for rows in (plain, scaled, planted):
        S = _scores_f64(rows, q)
        for b in range(q.shape[0]):
            assert np.array_equal(S[b].view(np.uint32), O.dot_scores(rows, q[b]).view(np.uint32))


# ==================================================================== GPU helpers
@pytest.fixture(scope="module")
def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def O():
    from oracle import lib
    return lib


@pytest.fixture(scope="module")
def bf16_ctx():
    """A ctx that only ever searches bf16 corpora: its "screen_gate" stays -1 (no search of it was screened)."""
    import openintel_amd as oi
    c = oi.HipContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def screen_ctx():
    import openintel_amd as oi
    from openintel_amd import _lib
    c = oi.HipContext(0)
    c.set_cosine_mode(_lib.OI_COSINE_SCREEN)
    yield c
    c.set_rescreen_tier(True)
    c.close()


def profiled_lists(ctx, idx, q, qt, qo, depth, F):
    """One filtered search_lists: (lists, launches per tag, the gate)."""
    ctx.profile_reset(1)
    L = idx.search_lists(q, qt, qo, depth=depth, filters=F)
    launches = {t: int(ctx.profile_read(t)[1]) for t in ("cosine", "spec", "rescreen")}
    gate = float(ctx.profile_read("screen_gate")[0])
    ctx.profile_reset(0)
    assert launches["spec"] == 0 and int(ctx.profile_read("screen_sample")[0]) == 0, "a filtered search never speculates"
    return L, launches, gate


def same_bits(A, Bl):
    """Two searches' lists, bit for bit up to each list's count (a filtered list can be shorter than depth)."""
    for leg in ("cos", "bm25"):
        ca, cb = getattr(A, leg + "_counts"), getattr(Bl, leg + "_counts")
        assert np.array_equal(ca, cb), leg
        for b, c in enumerate(ca.tolist()):
            for f in ("_docs", "_scores"):
                assert np.array_equal(getattr(A, leg + f)[b][:c].view(np.uint32), getattr(Bl, leg + f)[b][:c].view(np.uint32)), (leg, f, b)


# ==================================================================== GPU: the bf16 corpus, solo FILT
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES_BF16, ids=[c.name for c in CASES_BF16])
def test_bf16_filtered_case(bf16_ctx, O, num_cus, case):
    n, base, depth = case.n, case.doc_base(), case.depth
    chunks = case_chunks(case, num_cus)
    rows = int_rows(n, case.dim)
    q = int_queries(case.B, case.dim, case_seed(case))
    group, stamp, F = case_attrs_filters(case, num_cus)
    rng = np.random.default_rng(case_seed(case) + 3)
    fwd = _forward(rng, n)
    qt, qo = _query_terms(rng, case.B)
    idx = _bf16_index(bf16_ctx, _int_bits(rows), fwd[0], fwd[1], base, vocab=VOCAB)
    idx.set_doc_attrs(group, stamp)
    L, launches, gate = profiled_lists(bf16_ctx, idx, q, qt, qo, depth, F)
    assert launches["cosine"] == len(chunks), (case.name, launches, chunks)
    assert launches["rescreen"] == 0 and gate == -1.0 and idx.index_bytes()[1] == 0, "a bf16 corpus: no screen, no copy"
    assert idx.long_rows() == 0
    R = idx.search(q, qt, qo, k=K_FUSED, depth=depth, filters=F) if case.hybrid else None
    idx.close()
    ref = ref_lists(O, _scores_f64(rows, q), fwd, qt, qo, F, group, stamp, depth, K_FUSED, base, range(case.B))
    assert_lists(L, R, ref, case.name)


# ==================================================================== GPU: the int8 tier and the copy screen, FILT
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES_I8 + CASES_COPY, ids=[c.name for c in CASES_I8 + CASES_COPY])
def test_screen_filtered_case(screen_ctx, O, num_cus, case):
    """The int8 cases run with the residual tier on and off: the same lists, both the reference's."""
    n, base, depth = case.n, case.doc_base(), case.depth
    chunks = case_chunks(case, num_cus)
    rows = int_rows(n, case.dim).astype(np.float32)
    q = int_queries(case.B, case.dim, case_seed(case))
    group, stamp, F = case_attrs_filters(case, num_cus)
    rng = np.random.default_rng(case_seed(case) + 3)
    fwd = _forward(rng, n)
    qt, qo = _query_terms(rng, case.B)
    idx = _index(screen_ctx, rows, base, fwd)
    idx.set_doc_attrs(group, stamp)
    assert idx.index_bytes()[1] >= 3 * n * case.dim, "the index holds both screening copies"
    assert idx.long_rows() == 0
    got = []
    for residual in ((True, False) if case.route == "i8" else (True,)):
        screen_ctx.set_rescreen_tier(residual)
        L, launches, gate = profiled_lists(screen_ctx, idx, q, qt, qo, depth, F)
        assert launches["cosine"] == len(chunks), (case.name, launches, chunks)
        assert launches["rescreen"] == (1 if case.route == "i8" else 0), (case.name, launches)
        assert gate == 0.0, (case.name, gate)
        if case.route == "i8":
            assert screen_ctx.rescreen_state()[0] == (1 if residual else 0), "the second tier the case names"
        got.append(L)
    screen_ctx.set_rescreen_tier(True)
    R = idx.search(q, qt, qo, k=K_FUSED, depth=depth, filters=F) if case.hybrid else None
    idx.close()
    if len(got) == 2:
        same_bits(got[0], got[1])
    ref = ref_lists(O, _scores_f64(rows, q), fwd, qt, qo, F, group, stamp, depth, K_FUSED, base, range(case.B))
    for L in got:
        assert_lists(L, R, ref, case.name)


# ==================================================================== GPU: long rows under a filter (pf_rescore_kernel)
def long_rows_matrix(n: int, long_at) -> np.ndarray:
    """{-1, 0, 1} x (1 + 2^-9) -- not exact in bf16, which is where an index looks for long rows -- the planted rows 64 times that."""
    rows = int_rows(n, LONG_DIM).astype(np.float32) * np.float32(1 + 2.0 ** -9)
    rows[np.asarray(long_at, dtype=np.int64)] *= np.float32(64)
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("case", LONG_CASES, ids=[c.name for c in LONG_CASES])
def test_long_rows_under_a_filter(screen_ctx, O, num_cus, case):
    """The passing long rows are packed behind the survivors by their rank among the passing ones in long_list order
    (long_passing: ballots of 64, so positions 63 and 64 sit on either side of its second trip); attributes are read by LOCAL
    row (attrs[extra_docs[k]]) while the key carries the doc id.  Long rows score 64 times the others': the ones that pass head
    the list with their exact scores, the ones that fail never appear."""
    n, depth = N_LONG_CORPUS, LONG_DEPTH
    base = 2 ** 32 - 1 - n if case.base == MAXB else case.base
    rng = np.random.default_rng(900 + case.n_long + case.B)
    long_at = np.sort(rng.choice(n, size=case.n_long, replace=False))
    rows = long_rows_matrix(n, long_at)
    q = int_queries(case.B, LONG_DIM, case.n_long)
    fwd = _forward(rng, n)
    qt, qo = _query_terms(rng, case.B)
    idx = _index(screen_ctx, rows, base, fwd)
    assert idx.long_rows() == case.n_long and idx.index_bytes()[1] >= 3 * n * LONG_DIM
    long_list = idx.long_list()
    assert np.array_equal(np.sort(long_list), long_at), "the index lists the planted rows, in an order of its own"
    group, stamp = long_attrs(n, long_list, case.n_long + 1)
    F = long_filters(case.B, group, case.n_long + 2)
    idx.set_doc_attrs(group, stamp)
    screen_ctx.set_rescreen_tier(True)
    L, launches, gate = profiled_lists(screen_ctx, idx, q, qt, qo, depth, F)
    assert launches["cosine"] == 1 and launches["rescreen"] == 1 and gate == 0.0, (launches, gate)
    idx.close()
    S = _scores_f64(rows, q)
    ref = ref_lists(O, S, fwd, qt, qo, F, group, stamp, depth, K_FUSED, base, range(case.B))
    assert_lists(L, None, ref, case.name)
    is_long = np.zeros(n, bool)
    is_long[long_at] = True
    for b, (name, (_, _, want)) in enumerate(LONG_PATTERNS.items()):      # (what the equality above means for the long rows)
        ok = _passes(F[b], group, stamp)
        assert np.array_equal(ok[long_list], np.array([want(i) for i in range(case.n_long)])), (case.name, name)
        d = listed(L, b, base)
        assert not (is_long[d] & ~ok[d]).any(), (case.name, name, "a long row that fails the filter is listed")
        best = long_list[ok[long_list]]
        if best.size and S[b][best].max() > np.abs(S[b][~is_long]).max():
            assert int(d[0]) in set(best.tolist()), (case.name, name, "the best passing long row heads the list")


# ==================================================================== GPU: the gate open under a filter
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [384, 768])
def test_gate_open_by_a_query_without_a_bound(screen_ctx, O, num_cus, dim):
    """One query of the batch has an infinite coordinate: staging opens the gate, the gated exact pipeline runs with the filters
    (cosine_exact: X.filt = s.filt) from the screen's filtered thresholds.  Every other query's list is the reference's bit for
    bit; the unbounded query is held to nothing, as in test_a_query_without_a_bound_is_gated_as_before."""
    n, B, depth, base, bad = S3, 33, 10, 7, 5
    case = Case("gate-inf-d%d" % dim, "i8", dim, B, n, depth, base, "arange", 2, (2,))
    chunks = case_chunks(case, num_cus)
    rows = int_rows(n, dim).astype(np.float32)
    q = int_queries(B, dim, 77 + dim)
    q[bad, 17] = np.inf
    group, stamp, F = case_attrs_filters(case, num_cus)
    rng = np.random.default_rng(dim)
    fwd = _forward(rng, n)
    qt, qo = _query_terms(rng, B)
    idx = _index(screen_ctx, rows, base, fwd)
    idx.set_doc_attrs(group, stamp)
    assert idx.index_bytes()[1] >= 3 * n * dim and idx.long_rows() == 0
    L, launches, gate = profiled_lists(screen_ctx, idx, q, qt, qo, depth, F)
    idx.close()
    assert launches["cosine"] == len(chunks) == 2 and launches["rescreen"] == 1, (launches, chunks)
    assert gate == 1.0, gate
    good = [b for b in range(B) if b != bad]
    qs = q.copy()
    qs[bad] = 0.0
    assert_lists(L, None, ref_lists(O, _scores_f64(rows, qs), fwd, qt, qo, F, group, stamp, depth, K_FUSED, base, good), case.name)


CARRY_N, CARRY_B, CARRY_DEPTH, CARRY_FAIL = 36_000, 16, 1000, 100


def carry_row(q0, keep: int) -> np.ndarray:
    """254 at coordinate 0 and sign(q0) at the first `keep` coordinates where |q0| = 2, zero elsewhere.  Its int8 scale is 2: the
    +-1 coordinates round away (the tier sees 254 e_0 with a row error of sqrt(keep)), bf16 and the residual plane hold them."""
    x = np.zeros(q0.size, np.float32)
    at = np.flatnonzero(np.abs(q0[1:]) == 2)[:keep] + 1
    assert at.size == keep
    x[at] = np.sign(q0[at])
    x[0] = 254.0
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [384, 768])
@pytest.mark.parametrize("K,want_gate", [(OI_I8_CARRY, 0.0), (OI_I8_CARRY + 1, 1.0)])
def test_carry_capacity_counts_passing_rows_only(screen_ctx, O, num_cus, dim, K, want_gate):
    """test_carry_region_full_and_overflowing's recipe on integers, inside the first chunk (depth 1000: 28 672 rows at 256 CUs).
    Query 0 has q[0] = 2, every other query -2.  W = 254 e_0 + sign(q0) on 8 coordinates (score 524), D the same on 4 (516): the
    int8 tier sees both as 254 e_0 (score 508, bounds wider than their difference, lower bounds above every ordinary row's
    upper bound), so its margin selects carry every planted row that was appended; the second tier tells W from D.  `depth`
    copies of W and K - depth of D are in a group query 0's filter passes, CARRY_FAIL more copies of W in one it fails.
    K = OI_I8_CARRY: the carry is full to its last slot and the gate stays shut -- it would open if failing rows were appended or
    counted.  K = OI_I8_CARRY + 1: it overflows and the gate opens.  Lists exact either way: query 0's is the passing W rows."""
    n, B, depth, base = CARRY_N, CARRY_B, CARRY_DEPTH, 3
    case = Case("carry-d%d-K%d" % (dim, K), "i8", dim, B, n, depth, base, "arange", 2, (1,))
    chunks = case_chunks(case, num_cus)
    assert len(chunks) >= 2 and chunks[0][1] >= K + CARRY_FAIL
    rng = np.random.default_rng(K + dim)
    rows = int_rows(n, dim).astype(np.float32)
    q = int_queries(B, dim, 88 + dim)
    q[:, 0] = -2.0
    q[0, 0] = 2.0
    at = rng.choice(chunks[0][1], size=K + CARRY_FAIL, replace=False)
    w_pass, d_pass, w_fail = np.sort(at[:depth]), at[depth:K], at[K:]
    rows[w_pass] = rows[w_fail] = carry_row(q[0], 8)
    rows[d_pass] = carry_row(q[0], 4)
    group, stamp, F = case_attrs_filters(case, num_cus)
    group[at[:K]] = (group[at[:K]] & np.uint32(0xFFFC)) | np.uint32(1)
    group[w_fail] = (group[w_fail] & np.uint32(0xFFFC)) | np.uint32(2)
    F[0] = (0x3, 0x1, 0, 0xFFFFFFFF)
    fwd = _forward(rng, n)
    qt, qo = _query_terms(rng, B)
    idx = _index(screen_ctx, rows, base, fwd)
    idx.set_doc_attrs(group, stamp)
    assert idx.index_bytes()[1] >= 3 * n * dim and idx.long_rows() == 0
    S = _scores_f64(rows, q)
    assert S[0][w_pass].min() == S[0][w_fail].min() == 524.0 and S[0][d_pass].max() == 516.0
    ordinary = np.ones(n, bool)
    ordinary[at] = False
    assert S[0][ordinary].max() < 300.0 and S[1:, at].max() < 0.0
    ref = ref_lists(O, S, fwd, qt, qo, F, group, stamp, depth, K_FUSED, base, range(B))
    got = []
    for residual in (True, False):
        screen_ctx.set_rescreen_tier(residual)
        L, launches, gate = profiled_lists(screen_ctx, idx, q, qt, qo, depth, F)
        print("%s residual=%s: launches %s gate %g" % (case.name, residual, launches, gate))
        got.append((L, launches, gate))
    screen_ctx.set_rescreen_tier(True)
    idx.close()
    for L, launches, gate in got:
        assert launches["cosine"] == len(chunks) and launches["rescreen"] == 1, (launches, chunks)
        assert_lists(L, None, ref, case.name)
        assert np.array_equal(listed(L, 0, base), w_pass)
        assert gate == want_gate, (K, gate)
