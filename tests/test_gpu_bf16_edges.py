"""bf16 corpus scorer (configs[4]; csrc/cosine_bf16.hip) at every kernel and chunk edge, bit for bit against the oracle.

One search over a bf16 corpus can run four kernels, chosen per corpus chunk and per group of queries (oi_launch_cosine_bf16_chunk):
the solo kernel (cosine_bf16_filter<D, 1 | 2>), the pair kernel (cosine_bf16_pair<D, 2 | 3>), the query-split kernel
(cosine_bf16_qsplit<0>: 97-128 queries at d = 1024) and its sibling form (cosine_bf16_qsplit<2>: 256 queries at d = 1024 as two
workgroups per tile, only when B % 256 == 0 and the chunk has >= 32 x num_cus rows).  The search cuts the corpus into chunks
(search.hip: oi_first_chunk_rows, oi_chunk_growth, chunk_schedule, the pool budget of plan_search), so one search can run
siblings on one chunk and qsplit<0> on the next, both carrying into the same pools.

CASES below is the table of what this module runs.  A pure-Python mirror of the dispatch rules (`schedule`) computes each case's
chunks and kernels; a CPU test checks that the table reaches every kernel variant at every dim where it exists, and that each
case names the chunk count and kernels the mirror predicts on an MI355X.  On the GPU every case checks its chunk count through
the profiler (one "cosine" span per chunk), so a change to the schedule fails here instead of quietly turning a boundary case
into a one-chunk case.

Data: rows and queries are integers in [-3, 3], so every product and partial sum is exact in f32 in any order (|dot| <=
9 x 1024 < 2^24): cosine, BM25 and fused lists must equal the oracle's bit for bit, ties broken towards the lower doc id.
Cosine reference scores come from one float64 matmul (exact for these integers; test_int_matmul_equals_oracle_dot_scores).

Data "order": exact in any order means blind to the order.  The "order" cases carry products of +-2^24 beside small integers, at
most one non-zero product per (row, query) and 16-wide k-step (one MFMA adds one exact product to its accumulator), so a score
depends on the order of its sum: 2^24 + 1 = 2^24 in f32.  Their reference is an f32 chain in numpy, per query the one of the kernel
the mirror names for it: ascending K for the solo and query-split kernels, two ascending half chains summed as (half 0) +
(half 1) for the pair kernel.  A CPU test holds every such case to telling the two apart in at least one query's list."""
import os
from concurrent.futures import ThreadPoolExecutor
from typing import NamedTuple, Tuple, Union

import numpy as np
import pytest

COS_TOL = 1e-5
VOCAB = 300
MI355X_CUS = 256          # what the table's declared chunk counts and kernels assume (the GPU tests read the real count)
OI_MAX_DEPTH = 1024


# ==================================================================== mirror of the dispatch rules
def cb_group(dim: int, left: int) -> int:
    """cosine_bf16.hip: cb_group -- queries of the next corpus pass."""
    solo = 32 if dim == 1024 else 64
    if left <= solo:
        return solo
    if dim == 1024:
        return 128 if left > 96 else 96
    return 96 if (left + 95) // 96 < (left + 63) // 64 else 64


def first_chunk_rows(depth: int) -> int:
    """search.hip: oi_first_chunk_rows."""
    return max(max(8192, 32 * depth), 2 * depth)


def chunk_growth(B: int) -> int:
    """search.hip: oi_chunk_growth."""
    return 16 if B <= 8 else 8


def chunk_end(r: int, chunk: int, n: int, max_chunk: int, next_chunk: int) -> int:
    """search.hip: oi_chunk_end."""
    e = min(n, r + chunk)
    if e < n and (n - e) * 4 <= (e - r) and n - r <= max_chunk:
        e = n
    if e < n and next_chunk >= max_chunk and n - e > max_chunk and n - r <= 2 * max_chunk:
        e = n - max_chunk
    return e


def bf16_pool(n: int, B: int, num_cus: int) -> Tuple[int, int]:
    """search.hip, plan_search and cosine_bf16: (cos_stride, max_chunk) of a bf16 corpus."""
    carry_cap = OI_MAX_DEPTH
    slack = 128 * (num_cus + 1)
    cos_stride = 1 << 24
    budget = (8 << 30) // 8 // B
    cos_stride = min(cos_stride, budget)
    cos_stride = max(cos_stride, carry_cap + 4 * slack)
    cos_stride = min(cos_stride, carry_cap + n + slack)
    room = cos_stride - carry_cap
    return cos_stride, (room - slack if room > slack else 0)


def bf16_geometry(n_rows: int, num_cus: int, siblings: bool) -> Tuple[int, int]:
    """cosine_bf16.hip: oi_cosine_bf16_geometry -> (segments, rows per segment)."""
    n_tiles = (n_rows + 31) // 32
    quads = (n_tiles + 3) // 4
    cus = max(8, (num_cus // 16) * 8) if siblings else num_cus
    grid = quads if quads < cus else cus
    grid = grid if grid else 1
    if siblings and grid >= 8:
        grid -= grid % 8
    return grid, (quads + grid - 1) // grid * 4 * 32


def chunk_kernels(dim: int, B: int, n_rows: int, siblings: bool):
    """cosine_bf16.hip: oi_launch_cosine_bf16_chunk -- the kernel of every group of queries, in launch order."""
    return [k for k, _ in chunk_groups(dim, B, n_rows, siblings)]


def chunk_groups(dim: int, B: int, n_rows: int, siblings: bool):
    """The same, with each group's size: [(kernel, queries)] in launch order."""
    out, q0 = [], 0
    while q0 < B:
        left = B - q0
        group = 256 if siblings else cb_group(dim, left)
        nq = min(group, left)
        nqt = (nq + 31) // 32
        if dim == 1024:
            if nq > 128:
                kernel = "qsplit<2>"
            elif nq > 96:
                kernel = "qsplit<0>"
            elif nq <= 32:
                kernel = "solo<1024,1>"
            else:
                kernel = "pair<1024,%d>" % nqt
        elif nq > 64:
            kernel = "pair<%d,3>" % dim
        else:
            kernel = "solo<%d,%d>" % (dim, nqt)
        out.append((kernel, nq))
        q0 += nq
    return out


class Chunk(NamedTuple):
    begin: int
    end: int
    siblings: bool
    n_segs: int
    seg_cap: int
    kernels: tuple

    @property
    def rows(self) -> int:
        return self.end - self.begin


def schedule(n: int, dim: int, B: int, depth: int, num_cus: int):
    """The chunks of one search over an n-row bf16 corpus (search.hip: cosine_bf16, through chunk_schedule)."""
    _, max_chunk = bf16_pool(n, B, num_cus)
    assert max_chunk > 0
    chunks, chunk, r = [], first_chunk_rows(depth), 0
    while r < n:
        chunk = min(chunk, max_chunk)
        e = chunk_end(r, chunk, n, max_chunk, chunk * chunk_growth(B))
        sib = dim == 1024 and B >= 256 and B % 256 == 0 and e - r >= 32 * num_cus
        segs, cap = bf16_geometry(e - r, num_cus, sib)
        chunks.append(Chunk(r, e, sib, segs, cap, tuple(chunk_kernels(dim, B, e - r, sib))))
        r = e
        chunk *= chunk_growth(B)
    return chunks


VARIANTS = {384: {"solo<384,1>", "solo<384,2>", "pair<384,3>"},
            768: {"solo<768,1>", "solo<768,2>", "pair<768,3>"},
            1024: {"solo<1024,1>", "pair<1024,2>", "pair<1024,3>", "qsplit<0>", "qsplit<2>"}}


# ==================================================================== the case table
class TRows(NamedTuple):
    """Rows relative to the sibling threshold T = 32 x num_cus: mult x T + add."""
    mult: int
    add: int


MAX_BASE = -1             # doc_id_base = 4e9 - n: the largest ids the uint32 lists hold in this test


class Case(NamedTuple):
    name: str
    dim: int
    B: int
    n: Union[int, TRows]
    depth: int
    k: int
    base: int
    data: str             # "rand": i.i.d. integers; "ties": a few distinct rows repeated (many ties at every cut); "order": see above
    kernels: frozenset    # every kernel the case runs on an MI355X (the mirror, checked on the CPU)
    chunks: int           # corpus chunks on an MI355X (the mirror on the CPU, the profiler on the GPU)

    def n_rows(self, num_cus: int) -> int:
        return self.n if isinstance(self.n, int) else self.n.mult * 32 * num_cus + self.n.add

    def doc_base(self, num_cus: int) -> int:
        return 4_000_000_000 - self.n_rows(num_cus) if self.base == MAX_BASE else self.base


def _k(*names):
    return frozenset(names)


N2 = 8192 + 3000          # depth <= 256: a first chunk of 8192 rows, then a 3000-row tail longer than a quarter of it
N2D = 32000 + 9000        # depth 1000: a first chunk of 32 000 rows, then a 9000-row tail
N3 = 8192 + 65536 + 20000  # depth <= 256: three chunks (the last longer than a quarter of the second)

CASES = [
    # ---- B at every group edge, every dim (the 2-chunk corpora run the second chunk against carried thresholds)
    Case("d384-B1", 384, 1, N2, 1, 1, 0, "rand", _k("solo<384,1>"), 2),
    Case("d384-B32", 384, 32, N2, 2, 2, 7, "ties", _k("solo<384,1>"), 2),
    Case("d384-B33", 384, 33, N2, 100, 10, 1000, "rand", _k("solo<384,2>"), 2),
    Case("d384-B64", 384, 64, N2D, 1000, 100, MAX_BASE, "rand", _k("solo<384,2>"), 2),
    Case("d384-B65", 384, 65, N2D, 1024, 1024, 0, "rand", _k("pair<384,3>"), 2),
    Case("d384-B96", 384, 96, N2, 100, 50, 123_456_789, "ties", _k("pair<384,3>"), 2),
    Case("d384-B97", 384, 97, N2, 10, 10, 5, "rand", _k("solo<384,2>"), 2),   # 64 + 33: two passes of 96 are no fewer than two of 64
    Case("d768-B1", 768, 1, N2, 100, 10, MAX_BASE, "rand", _k("solo<768,1>"), 2),
    Case("d768-B32", 768, 32, N2, 1, 1, 0, "rand", _k("solo<768,1>"), 2),
    Case("d768-B33", 768, 33, N2D, 1000, 1000, 1000, "ties", _k("solo<768,2>"), 2),
    Case("d768-B64", 768, 64, N2, 2, 2, 7, "rand", _k("solo<768,2>"), 2),
    Case("d768-B65", 768, 65, N2, 100, 100, 0, "rand", _k("pair<768,3>"), 2),
    Case("d768-B96", 768, 96, N2D, 1024, 100, MAX_BASE, "rand", _k("pair<768,3>"), 2),
    Case("d768-B97", 768, 97, N2, 10, 1024, 0, "ties", _k("solo<768,2>"), 2),
    Case("d1024-B1", 1024, 1, N2, 2, 2, 0, "rand", _k("solo<1024,1>"), 2),
    Case("d1024-B32", 1024, 32, N2D, 1000, 100, 5, "rand", _k("solo<1024,1>"), 2),
    Case("d1024-B33", 1024, 33, N2, 1, 1, MAX_BASE, "rand", _k("pair<1024,2>"), 2),
    Case("d1024-B64", 1024, 64, N2, 100, 10, 0, "ties", _k("pair<1024,2>"), 2),
    Case("d1024-B65", 1024, 65, N2, 10, 10, 1000, "rand", _k("pair<1024,3>"), 2),
    Case("d1024-B96", 1024, 96, N2D, 1024, 1024, 0, "rand", _k("pair<1024,3>"), 2),
    Case("d1024-B97", 1024, 97, N2, 100, 100, MAX_BASE, "rand", _k("qsplit<0>"), 2),
    # ---- d = 1024: 128-query groups, the non-multiples of 256 (qsplit<0> + solo / pair tails) and the sibling batches
    Case("d1024-B128", 1024, 128, N2, 100, 100, 0, "rand", _k("qsplit<0>"), 2),
    Case("d1024-B129", 1024, 129, N2, 10, 10, 7, "ties", _k("qsplit<0>", "solo<1024,1>"), 2),
    Case("d1024-B200", 1024, 200, N2D, 1000, 100, 0, "rand", _k("qsplit<0>", "pair<1024,3>"), 2),
    Case("d1024-B225", 1024, 225, N2, 2, 2, MAX_BASE, "rand", _k("qsplit<0>"), 2),
    Case("d1024-B255", 1024, 255, N2, 100, 50, 0, "rand", _k("qsplit<0>"), 2),
    Case("d1024-B256", 1024, 256, N2, 100, 100, 1000, "rand", _k("qsplit<2>", "qsplit<0>"), 2),
    Case("d1024-B257", 1024, 257, N2, 100, 10, 0, "rand", _k("qsplit<0>", "solo<1024,1>"), 2),
    Case("d1024-B300", 1024, 300, N2, 10, 100, MAX_BASE, "rand", _k("qsplit<0>", "pair<1024,2>"), 2),
    Case("d1024-B384", 1024, 384, N2, 100, 100, 0, "ties", _k("qsplit<0>"), 2),
    Case("d1024-B512", 1024, 512, N2, 100, 100, 5, "rand", _k("qsplit<2>", "qsplit<0>"), 2),
    # ---- the pair kernel's larger batches at 384 / 768
    Case("d384-B128", 384, 128, N2, 100, 100, 0, "rand", _k("solo<384,2>"), 2),
    Case("d384-B200", 384, 200, N2, 10, 10, MAX_BASE, "ties", _k("pair<384,3>", "solo<384,2>"), 2),
    Case("d384-B256", 384, 256, N2D, 1000, 100, 0, "rand", _k("pair<384,3>", "solo<384,2>"), 2),
    Case("d768-B128", 768, 128, N2, 100, 100, 1000, "rand", _k("solo<768,2>"), 2),
    Case("d768-B200", 768, 200, N2, 2, 2, 0, "rand", _k("pair<768,3>", "solo<768,2>"), 2),
    Case("d768-B256", 768, 256, N2, 100, 1024, MAX_BASE, "ties", _k("pair<768,3>", "solo<768,2>"), 2),
    # ---- rows at the sibling threshold T = 32 x num_cus (d = 1024, B = 256)
    Case("sib-T", 1024, 256, TRows(1, 0), 100, 100, 0, "rand", _k("qsplit<2>"), 1),
    Case("sib-T-32", 1024, 256, TRows(1, -32), 100, 100, 1000, "rand", _k("qsplit<0>"), 1),
    Case("sib-T-1", 1024, 256, TRows(1, -1), 100, 10, 0, "ties", _k("qsplit<0>"), 1),
    Case("sib-T+1", 1024, 256, TRows(1, 1), 100, 100, MAX_BASE, "rand", _k("qsplit<2>"), 1),
    Case("sib-T+385", 1024, 256, TRows(1, 32 * 4 * 3 + 1), 10, 10, 0, "rand", _k("qsplit<2>"), 1),
    Case("sib-2T+1", 1024, 256, TRows(2, 1), 100, 100, 7, "rand", _k("qsplit<2>"), 2),
    Case("sib-2T+1-ties", 1024, 256, TRows(2, 1), 1024, 1024, 0, "ties", _k("qsplit<2>"), 1),
    # ---- mixed chunks: siblings on one chunk, qsplit<0> on the next
    Case("mixed-ties", 1024, 256, N2, 10, 10, 0, "ties", _k("qsplit<2>", "qsplit<0>"), 2),
    Case("mixed-depth1000", 1024, 256, 32000 + 8100, 1000, 100, 1000, "rand", _k("qsplit<2>", "qsplit<0>"), 2),
    Case("mixed-B512-depth1000", 1024, 512, 32000 + 8100, 1000, 1000, MAX_BASE, "ties", _k("qsplit<2>", "qsplit<0>"), 2),
    Case("B512-3chunks", 1024, 512, N3, 100, 100, 0, "rand", _k("qsplit<2>"), 3),
    # ---- ragged tiles: n not a multiple of 32, n < 32, a single row under a deeper list
    Case("ragged-n20", 768, 33, 20, 10, 10, 0, "rand", _k("solo<768,2>"), 1),
    Case("ragged-n1-d1024", 1024, 256, 1, 100, 100, MAX_BASE, "rand", _k("qsplit<0>"), 1),
    Case("ragged-n1-d384", 384, 5, 1, 1024, 1024, 7, "rand", _k("solo<384,1>"), 1),
    Case("ragged-n31-d1024", 1024, 97, 31, 2, 1, 0, "ties", _k("qsplit<0>"), 1),
    # ---- the order of a score's sum, one case per tile loop and K split (scores that depend on it: "order" data)
    Case("order-d384-B64", 384, 64, N2, 100, 10, 0, "order", _k("solo<384,2>"), 2),
    Case("order-d768-B96", 768, 96, N2, 100, 100, 7, "order", _k("pair<768,3>"), 2),
    Case("order-d1024-B32", 1024, 32, N2, 100, 10, 1000, "order", _k("solo<1024,1>"), 2),
    Case("order-d1024-B64", 1024, 64, N2, 100, 100, 0, "order", _k("pair<1024,2>"), 2),
    Case("order-d1024-B96", 1024, 96, N2, 100, 10, MAX_BASE, "order", _k("pair<1024,3>"), 2),
    Case("order-d1024-B128", 1024, 128, N2, 100, 100, 0, "order", _k("qsplit<0>"), 2),
    Case("order-d1024-B256-sib", 1024, 256, TRows(1, 0), 100, 10, 5, "order", _k("qsplit<2>"), 1),
]
ORDER_CASES = [c for c in CASES if c.data == "order"]


@pytest.fixture(scope="module")
def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def ctx():
    import openintel_amd as oi
    c = oi.HipContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import lib
    return lib


# ==================================================================== helpers
def to_bf16_bits(x):
    """f32 -> bfloat16 bit patterns, round to nearest even."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bf16_bits(b):
    return (np.asarray(b).astype(np.uint32) << 16).view(np.float32)


def _forward(rng, n, vocab=VOCAB):
    lens = rng.integers(1, 9, size=n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    return rng.integers(0, vocab, size=int(offs[-1])).astype(np.uint32), offs


def _query_terms(rng, B):
    return rng.integers(0, 12, size=B * 4).astype(np.uint32), (np.arange(B + 1) * 4).astype(np.uint32)


def _bf16_index(ctx, bits, terms, offs, base, vocab=VOCAB, stats=None):
    import openintel_amd as oi
    idx = oi.HybridIndex(ctx, bits.shape[0], bits.shape[1], vocab, base)
    idx.set_embeddings_bf16(bits)
    idx.set_forward(terms, offs)
    if stats is None:
        idx.finalize()
    else:
        idx.finalize(*stats)
    return idx


def _scores_f64(rows, q):
    """[B, n] f32 scores of every query against every row through a float64 matmul (rows in blocks: int8 rows stay small)."""
    qd = np.asarray(q, dtype=np.float64)
    out = np.empty((qd.shape[0], rows.shape[0]), dtype=np.float32)
    for r in range(0, rows.shape[0], 8192):
        out[:, r:r + 8192] = qd @ rows[r:r + 8192].astype(np.float64).T
    return out


def _pool():
    return ThreadPoolExecutor(max_workers=max(1, min(16, os.cpu_count() or 1)))


def _oracle_lists(O, S, terms, offs, qt, qo, depth, k, base, vocab=VOCAB, stats=None):
    """Per query: the oracle's (cosine scores, docs, BM25 scores, docs, fused scores, docs).  The oracle's C calls release the
    GIL: queries run on a thread pool."""
    df, n_glob, tot_glob = stats if stats is not None else (None, None, None)

    def one(b):
        cs, cd = O.topk(S[b], depth, False, base)
        bm = O.bm25_scores(terms, offs, vocab, qt[qo[b]:qo[b + 1]], df, n_glob, tot_glob)
        bs, bd = O.topk(bm, depth, True, base)
        fs, fd = O.rrf_fuse(cd, bd, k)
        return cs, cd, bs, bd, fs, fd
    with _pool() as ex:
        return list(ex.map(one, range(S.shape[0])))


def _assert_lists(L, R, ref, tag):
    for b, (cs, cd, bs, bd, fs, fd) in enumerate(ref):
        t = (tag, b)
        assert int(L.cos_counts[b]) == cd.size, t
        assert np.array_equal(L.cos_docs[b][:cd.size], cd), t
        assert np.array_equal(L.cos_scores[b][:cd.size].view(np.uint32), cs.view(np.uint32)), t
        assert int(L.bm25_counts[b]) == bd.size and np.array_equal(L.bm25_docs[b][:bd.size], bd), t
        if R is not None:
            assert int(R.counts[b]) == fd.size and np.array_equal(R.docs[b][:fd.size], fd), t
            assert np.array_equal(R.scores[b][:fd.size].view(np.uint32), fs.view(np.uint32)), t


def _int_data(case: Case, n: int, chunks, seed: int):
    """Integer rows (int8) and queries (f32) of a case, with its adversaries:
    * "ties": 7 distinct rows, repeated with skewed frequencies, the rarest one at both ends of every chunk -- many rows tie at the
      k-th score, copies of one row sit in every chunk and every segment, and the list must hold the lowest doc ids;
    * queries 128..255 of every 256 (the second sibling half) in [-1, 1]: their thresholds sit well below the first half's, so
      a chunk filtered with the other half's thresholds loses rows of their lists;
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
    second = (np.arange(B) % 256) >= 128
    q[second] = rng.integers(-1, 2, size=(int(second.sum()), dim))        # weaker queries: a threshold of the other half is too high
    if B >= 3:
        q[B // 2 + (1 if B >= 8 else 0)] = 0.0
    if B >= 3 and len(chunks) >= 2:
        last = chunks[-1]
        m = min(case.depth + 20, last.rows // 7)
        rows[last.end - 1 - 7 * np.arange(m)] = 3                           # score 3 x dim with the all-ones query: the top
        q[B - 1] = 1.0
    return rows, q


def _int_bits(rows):
    """bf16 bit patterns of small integers and of +-2^24 (exact)."""
    return (rows.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


BIG = np.float32(2.0 ** 24)


def _order_data(case: Case, n: int, seed: int):
    """Rows and queries (f32, every value exact in bf16) whose scores depend on the order of the sum, and what the reference needs:
    * one seeded position in every 16-wide k-step; rows are zero elsewhere, queries are 1 or 0 there: a (row, query) pair has at
      most one non-zero product per k-step, the row's value;
    * the values vals[row, step]: half of them zero, the rest integers in [-3, 3]; three rows in four also carry +2^24 at one
      step and -2^24 at another, in either order;
    * sel[query, step]: every second query takes every step, the others drop one step in ten (a dropped +-2^24 leaves its
      partner standing: scores near +-2^24 as well as near 0)."""
    rng = np.random.default_rng(seed)
    dim, B, ks = case.dim, case.B, case.dim // 16
    pos = 16 * np.arange(ks) + rng.integers(0, 16, size=ks)
    vals = rng.integers(-3, 4, size=(n, ks)).astype(np.float32)
    vals[rng.random((n, ks)) < 0.5] = 0.0
    big = np.nonzero(rng.random(n) < 0.75)[0]
    a = rng.integers(0, ks, size=big.size)
    b = (a + rng.integers(1, ks, size=big.size)) % ks
    sign = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=big.size)
    vals[big, a] = sign * BIG
    vals[big, b] = -sign * BIG
    sel = rng.random((B, ks)) < 0.9
    sel[::2] = True
    rows = np.zeros((n, dim), dtype=np.float32)
    rows[:, pos] = vals
    q = np.zeros((B, dim), dtype=np.float32)
    q[:, pos] = sel
    return rows, q, vals, sel


def _f32_chain(M):
    """((0 + M[:, 0]) + M[:, 1]) + ... in f32, round to nearest even: an MFMA accumulation chain with one product per step."""
    acc = np.zeros(M.shape[0], dtype=np.float32)
    for s in range(M.shape[1]):
        acc = acc + M[:, s]
    return acc


def _order_scores(vals, sel):
    """([B, n] f32 scores as ONE chain in ascending K, the same as TWO half chains summed as (half 0) + (half 1))."""
    B, (n, ks) = sel.shape[0], vals.shape
    one, two = np.empty((B, n), dtype=np.float32), np.empty((B, n), dtype=np.float32)
    for b in range(B):
        M = vals * sel[b].astype(np.float32)
        one[b] = _f32_chain(M)
        two[b] = _f32_chain(M[:, :ks // 2]) + _f32_chain(M[:, ks // 2:])
    return one, two


def _order_reference(case: Case, chunks, vals, sel):
    """[B, n] f32 scores of an "order" case: per chunk and query, the sum order of the kernel the mirror names for them."""
    one, two = _order_scores(vals, sel)
    S = one.copy()
    for ch in chunks:
        q0 = 0
        for kernel, nq in chunk_groups(case.dim, case.B, ch.rows, ch.siblings):
            if kernel.startswith("pair<"):
                S[q0:q0 + nq, ch.begin:ch.end] = two[q0:q0 + nq, ch.begin:ch.end]
            else:
                assert kernel.startswith(("solo<", "qsplit<")), kernel
            q0 += nq
        assert q0 == case.B
    return S, one, two


# ==================================================================== CPU: the table and the oracle shortcut
def test_case_table_reaches_every_variant_with_its_declared_schedule():
    """On an MI355X (256 CUs) every case runs the chunks and kernels it names, every chunk fits the candidate pool the search
    allocates (the library refuses a chunk that does not), and the table reaches every kernel variant at every dim."""
    seen = {d: set() for d in VARIANTS}
    names = set()
    for c in CASES:
        assert c.name not in names, c.name
        names.add(c.name)
        n = c.n_rows(MI355X_CUS)
        assert 0 < n and 0 <= c.doc_base(MI355X_CUS) and c.doc_base(MI355X_CUS) + n <= 4_000_000_000, c.name
        assert 1 <= c.depth <= OI_MAX_DEPTH and 1 <= c.k <= OI_MAX_DEPTH, c.name
        s = schedule(n, c.dim, c.B, c.depth, MI355X_CUS)
        assert s[0].begin == 0 and s[-1].end == n and all(a.end == b.begin for a, b in zip(s, s[1:])), c.name
        assert len(s) == c.chunks, (c.name, len(s))
        ks = {k for ch in s for k in ch.kernels}
        assert ks == set(c.kernels), (c.name, sorted(ks))
        seen[c.dim] |= ks
        stride, _ = bf16_pool(n, c.B, MI355X_CUS)
        for ch in s:
            assert ch.n_segs <= MI355X_CUS * (8 if c.B <= 8 else 1), c.name
            assert OI_MAX_DEPTH + ch.n_segs * ch.seg_cap <= stride, c.name
            if ch.siblings:
                assert ch.n_segs % 8 == 0, c.name        # the same-XCD pairing addresses workgroups in groups of 16
    for d, want in VARIANTS.items():
        assert seen[d] == want, (d, sorted(want - seen[d]))
    # the edges the table is there for
    for d in VARIANTS:
        assert {1, 32, 33, 64, 65, 96, 97} <= {c.B for c in CASES if c.dim == d}, d
    assert {128, 200, 256} <= {c.B for c in CASES if c.dim == 384} & {c.B for c in CASES if c.dim == 768}
    assert {128, 129, 200, 225, 255, 256, 257, 300, 384, 512} <= {c.B for c in CASES if c.dim == 1024}
    assert {1, 2, 100, 1000, 1024} <= {c.depth for c in CASES} and {1, 2, 100, 1000, 1024} <= {c.k for c in CASES}
    sib = {c.n for c in CASES if c.dim == 1024 and c.B == 256 and isinstance(c.n, TRows)}
    assert {TRows(1, 0), TRows(1, -32), TRows(1, -1), TRows(1, 1), TRows(1, 385), TRows(2, 1)} <= sib
    # the geometry those cases are meant to hit: T + 1 trims the grid to a multiple of 8, T + 385 puts two quads in a segment
    T = 32 * MI355X_CUS
    assert bf16_geometry(T, MI355X_CUS, True) == (64, 128)
    assert bf16_geometry(T + 1, MI355X_CUS, True) == (64, 256) and bf16_geometry(T + 1, MI355X_CUS, False)[0] == 65
    assert bf16_geometry(T + 385, MI355X_CUS, True) == (64, 256)
    # mixed chunks: siblings on the first chunk, not on the tail, in one search; and >= 3 chunks with B = 512
    mixed = [c for c in CASES if c.chunks >= 2 and c.B % 256 == 0 and c.dim == 1024]
    assert any(not schedule(c.n_rows(MI355X_CUS), 1024, c.B, c.depth, MI355X_CUS)[-1].siblings and c.depth >= 1000 for c in mixed)
    assert any(c.B == 512 and c.chunks >= 3 for c in CASES)
    assert any(c.n_rows(MI355X_CUS) < 32 for c in CASES) and any(c.n_rows(MI355X_CUS) == 1 and c.depth > 1 for c in CASES)


def test_int_matmul_equals_oracle_dot_scores():
    """The module's cosine reference (a float64 matmul of integer rows and queries) is the oracle's dot_scores, bit for bit."""
    from oracle import lib as O
    rng = np.random.default_rng(3)
    rows = rng.integers(-3, 4, size=(3000, 1024)).astype(np.int8)
    q = rng.integers(-3, 4, size=(4, 1024)).astype(np.float32)
    q[1] = 0.0
    q[2] = 3.0
    S = _scores_f64(rows, q)
    for b in range(q.shape[0]):
        assert np.array_equal(S[b].view(np.uint32), O.dot_scores(rows.astype(np.float32), q[b]).view(np.uint32))


def test_order_cases_tell_one_chain_from_two_half_chains():
    """Every "order" case: its data is what the reference assumes (exact in bf16, at most one non-zero product per k-step and
    (row, query) pair), and the case can see what it is there for -- the lists of at least one of its queries differ between
    the two sum orders, so a tile loop that sums a score in the other kernel's order fails the case."""
    from oracle import lib as O
    assert [(c.dim, c.B) for c in ORDER_CASES] == [(384, 64), (768, 96), (1024, 32), (1024, 64), (1024, 96), (1024, 128), (1024, 256)]
    assert ORDER_CASES[-1].n == TRows(1, 0)
    for c in ORDER_CASES:
        n, base = c.n_rows(MI355X_CUS), c.doc_base(MI355X_CUS)
        chunks = schedule(n, c.dim, c.B, c.depth, MI355X_CUS)
        rows, q, vals, sel = _order_data(c, n, 1009 * c.dim + 31 * c.B + n)
        assert np.array_equal(from_bf16_bits(_int_bits(rows)), rows) and np.array_equal(from_bf16_bits(to_bf16_bits(q)), q), c.name
        assert (np.count_nonzero(rows.reshape(n, -1, 16), axis=2) <= 1).all() and np.isin(q, (0.0, 1.0)).all(), c.name
        assert np.array_equal(rows[:, np.nonzero(q.any(axis=0))[0]] != 0, vals != 0), c.name     # the products ARE vals x sel
        S, one, two = _order_reference(c, chunks, vals, sel)
        pair = all(k.startswith("pair<") for k in c.kernels)
        assert np.array_equal(S.view(np.uint32), (two if pair else one).view(np.uint32)), c.name
        differ = 0
        for b in range(c.B):
            (s1, d1), (s2, d2) = O.topk(one[b], c.depth, False, base), O.topk(two[b], c.depth, False, base)
            differ += not (np.array_equal(d1, d2) and np.array_equal(s1.view(np.uint32), s2.view(np.uint32)))
        print("%s: the lists of %d of %d queries differ between the two sum orders" % (c.name, differ, c.B))
        assert differ >= 1, c.name


# ==================================================================== GPU: the table, bit for bit
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_bf16_case_bit_exact(ctx, O, num_cus, case):
    n, base = case.n_rows(num_cus), case.doc_base(num_cus)
    chunks = schedule(n, case.dim, case.B, case.depth, num_cus)
    seed = 1009 * case.dim + 31 * case.B + n
    if case.data == "order":
        rows, q, vals, sel = _order_data(case, n, seed)
        S = _order_reference(case, chunks, vals, sel)[0]
    else:
        rows, q = _int_data(case, n, chunks, seed)
        S = _scores_f64(rows, q)
    rng = np.random.default_rng(seed + 1)
    terms, offs = _forward(rng, n)
    qt, qo = _query_terms(rng, case.B)
    idx = _bf16_index(ctx, _int_bits(rows), terms, offs, base)
    ctx.profile_reset(2)
    L = idx.search_lists(q, qt, qo, depth=case.depth)
    launches = ctx.profile_read("cosine")[1]
    ctx.profile_reset(0)
    assert launches == len(chunks), (case.name, launches, [(c.begin, c.end) for c in chunks])
    R = idx.search(q, qt, qo, k=case.k, depth=case.depth)
    idx.close()
    ref = _oracle_lists(O, S, terms, offs, qt, qo, case.depth, case.k, base)
    _assert_lists(L, R, ref, case.name)


# ==================================================================== GPU: float data
def _halfway_queries(rng, B, dim):
    """Coordinates exactly halfway between two bf16 values, 1 + (2m + 1) 2^-8 for m in 0..63, both signs: round to nearest even
    goes up for odd m and down for even m, so truncation and rounding half away from zero each get half of them wrong."""
    m = rng.integers(0, 64, size=(B, dim))
    sign = rng.choice(np.array([-1.0, 1.0]), size=(B, dim))
    return (sign * (1.0 + (2 * m + 1) / 256.0)).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("dim,B,n", [(384, 9, 3000), (768, 100, 5000), (1024, 65, 4001), (1024, 256, TRows(1, 0))],
                         ids=["d384-solo", "d768-pair", "d1024-pair", "d1024-siblings"])
def test_query_staging_rounds_to_nearest_even(ctx, O, num_cus, dim, B, n):
    """cb_stage_queries rounds f32 queries to bf16 with round-to-nearest-even.  With halfway coordinates and small-integer rows
    the score of bf16(q) . x is exact in f32 (8 significant bits times |x| <= 3, 1024 terms: well under 2^24 units of 2^-7),
    so the lists must equal the float64 reference of the RNE-rounded queries bit for bit."""
    n = n if isinstance(n, int) else n.mult * 32 * num_cus + n.add
    rng = np.random.default_rng(dim + B)
    rows = rng.integers(-3, 4, size=(n, dim)).astype(np.int8)
    q = _halfway_queries(rng, B, dim)
    qr = from_bf16_bits(to_bf16_bits(q))
    assert not np.array_equal(qr, q)
    terms, offs = _forward(rng, n)
    idx = _bf16_index(ctx, _int_bits(rows), terms, offs, 0)
    depth = 100
    L = idx.search_lists(q, np.zeros(B, np.uint32), np.arange(B + 1, dtype=np.uint32), depth=depth)
    idx.close()
    S = _scores_f64(rows, qr)
    trunc = from_bf16_bits((q.view(np.uint32) >> 16).astype(np.uint16))                       # round toward zero
    away = from_bf16_bits(((q.view(np.uint32) + 0x8000) >> 16).astype(np.uint16))             # half away from zero
    for b in range(B):
        cs, cd = O.topk(S[b], depth, False, 0)
        assert int(L.cos_counts[b]) == cd.size and np.array_equal(L.cos_docs[b][:cd.size], cd), b
        assert np.array_equal(L.cos_scores[b][:cd.size].view(np.uint32), cs.view(np.uint32)), b
        # (the test can see the difference: either wrong rounding changes the scores of this query's list)
        x = rows[cd.astype(np.int64)].astype(np.float64)
        assert (x @ trunc[b].astype(np.float64) != cs).any() and (x @ away[b].astype(np.float64) != cs).any(), b


@pytest.mark.gpu
@pytest.mark.parametrize("B,n,depths", [(256, TRows(1, 0), (10, 1000)), (256, TRows(2, 1), (10, 1000)),
                                        (512, N2, (10, 100)), (256, 32000 + 8100, (10, 1000))],
                         ids=["siblings-T", "siblings-2T+1", "mixed-B512", "mixed-depth1000"])
def test_bf16_unit_rows_within_tolerance_at_sibling_shapes(ctx, num_cus, B, n, depths):
    """Random unit-norm bf16 rows at the sibling and mixed-chunk shapes: the bar of test_gpu_bf16.py's tolerance test (scores
    within 1e-5 of the float64 dot of the rows as stored with bf16-rounded queries, every row clearly above the k-th score in
    the list, nothing clearly below it)."""
    from openintel_amd import synth
    dim = 1024
    n = n if isinstance(n, int) else n.mult * 32 * num_cus + n.add
    bits = to_bf16_bits(synth.embeddings_np(n, dim, seed=11 + B))
    rows = from_bf16_bits(bits)
    q = synth.embeddings_np(B, dim, seed=91 + B)
    qr = from_bf16_bits(to_bf16_bits(q))
    rng = np.random.default_rng(B)
    terms, offs = _forward(rng, n, 50)
    idx = _bf16_index(ctx, bits, terms, offs, 0, vocab=50)
    qt, qo = np.zeros(B, np.uint32), np.arange(B + 1, dtype=np.uint32)
    ref_all = _scores_f64(rows, qr).astype(np.float64)
    for depth in depths:
        L = idx.search_lists(q, qt, qo, depth=depth)
        for b in range(B):
            ref = ref_all[b]
            c = int(L.cos_counts[b])
            assert c == min(depth, n)
            d, s = L.cos_docs[b][:c], L.cos_scores[b][:c]
            assert np.unique(d).size == c and np.abs(s - ref[d]).max() <= COS_TOL, (depth, b)
            assert (np.diff(s) <= 0).all()
            kth = np.sort(ref)[::-1][c - 1]
            assert np.isin(np.nonzero(ref > kth + 2 * COS_TOL)[0], d).all() and (ref[d] >= kth - 2 * COS_TOL).all(), (depth, b)
    idx.close()


# ==================================================================== GPU: composition and reuse
@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(9000, 15000), (8000, 8192, 7808)], ids=["2-shards", "3-shards"])
def test_bf16_shards_merge_to_the_single_index(ctx, O, num_cus, sizes):
    """A bf16 corpus as one index and as 2 or 3 shards with doc_id_base (how configs[4] runs on 8 GPUs), BM25 finalised with the
    global statistics: merge_lists of the shards' lists and RRF of the merged lists equal the single index's lists and the
    oracle bit for bit.  The sizes give the shards schedules and kernels of their own (the single index: siblings on both
    chunks; a 9000-row shard: siblings then qsplit<0>; shards below T rows: qsplit<0> only)."""
    import openintel_amd as oi
    dim, B, depth, k, base = 1024, 256, 100, 50, 3_000_000_000
    n = sum(sizes)
    rng = np.random.default_rng(n)
    case = Case("shards", dim, B, n, depth, k, base, "ties", frozenset(), 0)
    chunks = schedule(n, dim, B, depth, num_cus)
    rows, q = _int_data(case, n, chunks, n + 1)
    terms, offs = _forward(rng, n)
    qt, qo = _query_terms(rng, B)
    bits = _int_bits(rows)
    df, tot = O.bm25_df(terms, offs, VOCAB)
    single = _bf16_index(ctx, bits, terms, offs, base)
    Ls = single.search_lists(q, qt, qo, depth=depth)
    Rs = single.search(q, qt, qo, k=k, depth=depth)
    single.close()
    scheds = {len(chunks)}
    parts, r0 = [], 0
    for m in sizes:
        tt, oo = terms[int(offs[r0]):int(offs[r0 + m])], offs[r0:r0 + m + 1] - offs[r0]
        scheds.add(tuple(ch.kernels for ch in schedule(m, dim, B, depth, num_cus)))
        sh = _bf16_index(ctx, bits[r0:r0 + m], tt, oo, base + r0, stats=(n, tot, df))
        parts.append(sh.search_lists(q, qt, qo, depth=depth))
        sh.close()
        r0 += m
    assert len(scheds) >= 3                              # (the shards do not all run the single index's schedule)
    cs, cd, cc = oi.merge_lists(ctx, np.stack([p.cos_scores for p in parts]), np.stack([p.cos_docs for p in parts]),
                                np.stack([p.cos_counts for p in parts]))
    bs, bd, bc = oi.merge_lists(ctx, np.stack([p.bm25_scores for p in parts]), np.stack([p.bm25_docs for p in parts]),
                                np.stack([p.bm25_counts for p in parts]))
    F = oi.rrf_fuse(ctx, cd, cc, bd, bc, k)
    for got, want in ((cs, Ls.cos_scores), (cd, Ls.cos_docs), (cc, Ls.cos_counts), (bs, Ls.bm25_scores),
                      (bd, Ls.bm25_docs), (bc, Ls.bm25_counts), (F.scores, Rs.scores), (F.docs, Rs.docs), (F.counts, Rs.counts)):
        assert np.array_equal(np.asarray(got).view(np.uint32), np.asarray(want).view(np.uint32))
    ref = _oracle_lists(O, _scores_f64(rows, q), terms, offs, qt, qo, depth, k, base)
    _assert_lists(Ls, Rs, ref, "single")


@pytest.mark.gpu
def test_one_ctx_many_shapes(O, num_cus):
    """One ctx, a sequence of searches of different shapes (q_bf16, pool_cos and the pool state words are reused buffers of the
    ctx): each must equal the oracle bit for bit."""
    import openintel_amd as oi
    c = oi.HipContext(0)
    rng = np.random.default_rng(77)
    nA, baseA = 32000 + 8100, 11

    def int_index(n, dim, base, bf16=True):
        rows = rng.integers(-3, 4, size=(n, dim)).astype(np.int8)
        terms, offs = _forward(rng, n)
        if bf16:
            return rows, terms, offs, _bf16_index(c, _int_bits(rows), terms, offs, base)
        idx = oi.HybridIndex(c, n, dim, VOCAB, base)
        idx.set_embeddings(rows.astype(np.float32), normalize=False)
        idx.set_forward(terms, offs)
        idx.finalize()
        return rows, terms, offs, idx

    A = int_index(nA, 1024, baseA)
    D768 = int_index(N2, 768, 0)
    F32 = int_index(20_011, 384, 5, bf16=False)
    steps = [("B512-d1024-depth1000", A, baseA, 512, 1000, 100), ("B97-depth10", A, baseA, 97, 10, 10),
             ("B256-d768", D768, 0, 256, 100, 100), ("f32-screen-B64", F32, 5, 64, 100, 20), ("B1-again", A, baseA, 1, 100, 10)]
    for name, (rows, terms, offs, idx), base, B, depth, k in steps:
        q = rng.integers(-3, 4, size=(B, rows.shape[1])).astype(np.float32)
        if B >= 3:
            q[B // 2] = 0.0
        qt, qo = _query_terms(rng, B)
        L = idx.search_lists(q, qt, qo, depth=depth)
        R = idx.search(q, qt, qo, k=k, depth=depth)
        _assert_lists(L, R, _oracle_lists(O, _scores_f64(rows, q), terms, offs, qt, qo, depth, k, base), name)
    for _, _, _, idx in (A, D768, F32):
        idx.close()
    c.close()
