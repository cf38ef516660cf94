"""The int8 first screening tier (csrc/cosine_screen_i8.hip) at every query-group, tile, chunk and carry edge.

An f32 batch of B > 8 queries over an index that holds both screening copies streams the int8 copy first: one launch of
cosine_i8_screen per 64 queries (NQT = 1 or 2 query tiles by the group's size), one persistent workgroup of four waves per segment,
wave w of workgroup b taking the 32-row tiles b x 4 + w, stepping by grid x 4.  Keys are per-row lower bounds l_r = s~ - m_r, a row
is kept when u_r = s~ + m_r reaches the threshold.  A wrong term of that bound, or a wrong tile, chunk or group offset, drops a true
top-k row on some data only: nothing crashes and nothing slows down.

CASES below is the table of what this module runs.  A pure-Python mirror of the route's dispatch (search.hip: plan_search,
oi_screen_first_chunk_rows, the speculation decision, chunk_schedule; cosine_prefilter.hip: oi_cosine_screen_geometry; the
64-query groups of oi_launch_cosine_screen_i8_chunk) computes each case's chunks, speculative launches and groups; a CPU test
checks each case's declared schedule against it and that the table reaches every edge.  On the GPU every case runs through the
int8 route (OI_COSINE_SCREEN) and through the f32-stream screen (OI_COSINE_SCREEN_STREAM, which never reads a copy): the profiled
schedule must be the mirror's, both lists must be the same bit for bit, and they must meet the f64 oracle's bar.  The stream screen
shares the selects and the rescoring with the int8 route, so the oracle bar is checked as well.

Named adversaries (test_adversary_*) build data where a wrong term of the bound, a missing tile mask or a wrong group offset
changes the lists; test_isa_* pins the packed-f32 claim of DESIGN 4.1a / 7 on the compiled assembly."""
import os
import re
import subprocess
import tempfile
from typing import NamedTuple, Tuple

import numpy as np
import pytest

from test_gpu_bf16_edges import chunk_end, chunk_growth, first_chunk_rows

MI355X_CUS = 256          # what the table's declared schedules assume (the GPU tests read the real count)
OI_MAX_DEPTH = 1024
OI_I8_CARRY = 16384       # oi_internal.h: keys per query the int8 tier carries between chunks
TILE = 32
COS_TOL = 1e-5
VOCAB = 50
MAXB = -1                 # doc_id_base = 2^32 - 1 - n: the last doc id is 2^32 - 2


# ==================================================================== mirror of the int8 route's dispatch
def route(B: int, mode: str, copy: bool = True, i8: bool = True) -> str:
    """search.hip: plan_search, the cosine route of a screenable f32 index (mode: "screen" or "stream")."""
    want_copy = mode != "stream" and copy
    if not (B > 8 or want_copy):
        return "exact"
    if not want_copy:
        return "screen_f32"
    return "screen_i8" if B > 8 and i8 else "screen_copy"


def screen_first_chunk_rows(depth: int, num_cus: int) -> int:
    """search.hip: oi_screen_first_chunk_rows -- a whole number of rounds of 32 x 4 x floor(7 CUs / 8) rows."""
    rows = first_chunk_rows(depth)
    rnd = TILE * 4 * max(1, num_cus * 7 // 8)
    return rows - rows % rnd if rows >= rnd else rows


def screen_pool(n: int, B: int, num_cus: int, pf_carry: int = OI_I8_CARRY) -> Tuple[int, int]:
    """search.hip, plan_search: (pf_stride, pool_max) of the screen's view of the cosine pool."""
    budget = (13 << 28) // 8 // B
    slack = 128 * (num_cus + 1)
    stride = min(pf_carry + n + slack, max(min(1 << 24, budget), pf_carry + 4 * slack))
    return stride, stride - pf_carry - slack


def chunk_schedule(n: int, first: int, growth: int, max_chunk: int, stretch_first: bool, branches=None):
    """search.hip: chunk_schedule -> [(r, e)].  branches (a list): which rule of oi_chunk_end ended each chunk -- "plain",
    "stretch" (a tail of <= a quarter of the chunk taken along) or "n-max" (grown so that the last chunk is max_chunk)."""
    out, chunk, r = [], first, 0
    while r < n:
        chunk = min(chunk, max_chunk)
        e = chunk_end(r, chunk, n, max_chunk, 0 if (r == 0 and not stretch_first) else chunk * growth)
        if branches is not None:
            e0 = min(n, r + chunk)
            branches.append("plain" if e == e0 else "stretch" if e == n else "n-max")
        out.append((r, e))
        r = e
        chunk *= growth
    return out


def _rank(depth: int, e: int, n: int) -> int:
    return (3 * depth * e + n - 1) // n + 12


class Plan(NamedTuple):
    kind: str             # "proven", "short" (short first chunk, x 128) or "regular" (regular first chunk, x 128)
    chunks: tuple         # ((r, e), ...)
    branches: tuple       # the oi_chunk_end rule of each chunk
    spec_launches: int
    pool_max: int
    pf_stride: int


def plan(n: int, B: int, depth: int, num_cus: int, spec: bool = True, pf_carry: int = OI_I8_CARRY) -> Plan:
    """The screen's schedule (search.hip: plan_search + the spec launches of cosine_screen), B > 8."""
    stride, pool_max = screen_pool(n, B, num_cus, pf_carry)
    first, growth, kind = screen_first_chunk_rows(depth, num_cus), chunk_growth(B), "proven"
    if spec and n and B > 8:
        first_short = min(n, max(max(8192, 8 * depth), first // 4))
        if n - first_short <= pool_max and 2 * _rank(depth, first_short, n) <= depth:
            growth, first, kind = 128, first_short, "short"
        elif 2 * _rank(depth, min(n, first), n) <= depth:
            growth, kind = 128, "regular"
    branches = []
    chunks = chunk_schedule(n, first, growth, pool_max, stretch_first=False, branches=branches)
    ns = sum(1 for (_, e) in chunks[:-1] if spec and B > 8 and 2 * _rank(depth, e, n) <= depth)
    return Plan(kind, tuple(chunks), tuple(branches), ns, pool_max, stride)


def screen_geometry(n_rows: int, num_cus: int) -> Tuple[int, int]:
    """cosine_prefilter.hip: oi_cosine_screen_geometry -> (segments, segment capacity)."""
    n_tiles = (n_rows + TILE - 1) // TILE
    quads = (n_tiles + 3) // 4
    cus = max(1, num_cus * 7 // 8)
    grid = (quads if quads else 1) if quads < cus else cus
    return grid, (quads + grid - 1) // grid * 4 * TILE


def wave_tiles(n_rows: int, num_cus: int) -> set:
    """The distinct per-wave tile counts of one chunk (cosine_i8_screen: first = block x 4 + w, stride = grid x 4)."""
    n_tiles = (n_rows + TILE - 1) // TILE
    stride = screen_geometry(n_rows, num_cus)[0] * 4
    return {(n_tiles - f + stride - 1) // stride if f < n_tiles else 0 for f in range(stride)}


def query_groups(B: int) -> tuple:
    """oi_launch_cosine_screen_i8_chunk: the NQT of each 64-query group."""
    return tuple(2 if min(64, B - q0) > 32 else 1 for q0 in range(0, B, 64))


# ==================================================================== the case table
class Case(NamedTuple):
    name: str
    dim: int
    B: int
    n: int
    depth: int
    base: int             # doc_id_base (MAXB: 2^32 - 1 - n)
    spec: bool            # speculation on
    chunks: int           # declared for 256 CUs (the mirror, checked on the CPU)
    nqt: tuple            # declared NQT per 64-query group
    hybrid: bool = False  # also a hybrid search, fused outputs compared between the two routes

    def doc_base(self) -> int:
        return 2 ** 32 - 1 - self.n if self.base == MAXB else self.base


N_STRETCH = 8192 + 65536 + 12000    # proven x 8: the third chunk would be 12 000 rows, <= a quarter: taken along
N_BIG = 3_300_001                   # B = 256, d = 384: 8192, then n - max_chunk (off the 32-row grid), then max_chunk

CASES = [
    Case("d384-B9-depth10", 384, 9, 40_001, 10, 0, True, 2, (1,)),
    Case("d768-B31-maxbase", 768, 31, 100_003, 100, MAXB, True, 2, (1,), hybrid=True),
    Case("d384-B32-one-chunk", 384, 32, 5_000, 1, 0, True, 1, (1,)),
    Case("d768-B33-depth1000", 768, 33, 123_457, 1000, 5, True, 2, (2,)),
    Case("d384-B63-short-spec", 384, 63, 300_001, 100, 7, True, 2, (2,)),
    Case("d768-B64-proven", 768, 64, 300_000, 100, 0, False, 3, (2,)),
    Case("d384-B65-stretch", 384, 65, N_STRETCH, 100, MAXB, False, 2, (2, 1), hybrid=True),
    Case("d768-B96-depth1024", 768, 96, 90_017, 1024, 0, True, 2, (2, 1)),
    Case("d384-B97-ragged", 384, 97, 1_000, 100, 3, True, 1, (2, 2)),
    Case("d768-B97-spec", 768, 97, 200_011, 100, 0, True, 2, (2, 2)),
    Case("d384-B128-depth1", 384, 128, 70_001, 1, MAXB, True, 2, (2, 2)),
    Case("d768-B129-depth10", 768, 129, 81_920, 10, 0, True, 2, (2, 2, 1), hybrid=True),
    Case("d384-B129-proven", 384, 129, 150_000, 100, 11, False, 3, (2, 2, 1)),
    Case("d768-B256-depth1000", 768, 256, 160_001, 1000, 0, True, 2, (2, 2, 2, 2)),
    Case("d384-B256-offgrid", 384, 256, N_BIG, 100, 0, True, 3, (2, 2, 2, 2)),
    Case("d768-B9-tiny", 768, 9, 33, 10, MAXB, True, 1, (1,)),
]


def case_plan(c: Case, num_cus: int) -> Plan:
    return plan(c.n, c.B, c.depth, num_cus, c.spec)


# ==================================================================== CPU: the mirror against known schedules, the table
def test_mirror_reproduces_the_recorded_int8_schedules():
    """The mirror gives the "cosine" and "spec" launch counts test_gpu_search_plan.py recorded on an MI355X for its int8 cases
    (d = 768, B = 64 unless named)."""
    recorded = {(300_000, 64, 100, True): (2, 1), (300_000, 64, 100, False): (3, 0), (300_000, 128, 1000, True): (2, 1),
                (300_000, 9, 100, True): (2, 1), (1_250_000, 64, 100, True): (2, 1), (2_000_000, 64, 100, False): (4, 0)}
    for (n, B, depth, spec), (cos, sp) in recorded.items():
        p = plan(n, B, depth, MI355X_CUS, spec)
        assert (len(p.chunks), p.spec_launches) == (cos, sp), (n, B, depth, spec, p)
    assert plan(1_250_000, 64, 100, MI355X_CUS).kind == "short"
    # the f32 screen's rounded first chunk: 28 672 rows = one round of 224 workgroups x 4 waves x 32 rows
    assert screen_first_chunk_rows(1000, MI355X_CUS) == 28_672 and screen_first_chunk_rows(100, MI355X_CUS) == 8192
    assert screen_pool(10**9, 256, MI355X_CUS) == (1_703_936, 1_654_656)
    assert screen_geometry(8192, MI355X_CUS) == (64, 128) and screen_geometry(10**6, MI355X_CUS)[0] == 224
    assert route(9, "screen") == "screen_i8" and route(8, "screen") == "screen_copy" and route(64, "stream") == "screen_f32"
    assert route(8, "stream") == "exact" and route(64, "screen", i8=False) == "screen_copy"
    assert query_groups(129) == (2, 2, 1) and query_groups(97) == (2, 2) and query_groups(96) == (2, 1)


def test_case_table_reaches_every_edge():
    """Every case runs the schedule and groups it declares on an MI355X (256 CUs), every chunk fits the pool the search
    allocates, and the table as a whole reaches every edge the int8 tier has."""
    names, seen = set(), {"kinds": set(), "tiles": set(), "dim_nqt": set()}
    offgrid = stretch = ragged = False
    for c in CASES:
        assert c.name not in names, c.name
        names.add(c.name)
        assert route(c.B, "screen") == "screen_i8" and route(c.B, "stream") == "screen_f32", c.name
        assert 1 <= c.depth <= OI_MAX_DEPTH and 0 <= c.doc_base() and c.doc_base() + c.n <= 2 ** 32 - 1, c.name
        p = case_plan(c, MI355X_CUS)
        ch = p.chunks
        assert ch[0][0] == 0 and ch[-1][1] == c.n and all(a[1] == b[0] for a, b in zip(ch, ch[1:])), c.name
        assert len(ch) == c.chunks, (c.name, ch)
        assert query_groups(c.B) == c.nqt, (c.name, query_groups(c.B))
        seen["kinds"].add("one" if len(ch) == 1 else p.kind)
        seen["dim_nqt"] |= {(c.dim, t) for t in c.nqt}
        for (r, e) in ch:
            segs, cap = screen_geometry(e - r, MI355X_CUS)
            assert segs <= MI355X_CUS and OI_I8_CARRY + segs * cap <= p.pf_stride, (c.name, r, e)   # the launcher's OI_REQUIRE
            assert e - r <= p.pool_max, c.name
            seen["tiles"] |= wave_tiles(e - r, MI355X_CUS)
            offgrid |= e < c.n and e % TILE != 0
        ragged |= c.n % TILE != 0
        stretch |= "stretch" in p.branches
    assert {"one", "proven", "short", "regular"} <= seen["kinds"], seen["kinds"]
    assert {(384, 1), (384, 2), (768, 1), (768, 2)} <= seen["dim_nqt"]
    Bs = {c.B for c in CASES}
    assert {9, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 256} <= Bs
    assert {1, 2, 3, 4} <= {len(c.nqt) for c in CASES}
    lasts = {c.B - 64 * (len(c.nqt) - 1) for c in CASES if len(c.nqt) > 1}
    assert 1 in lasts and 33 in lasts                                   # a last group of 1 query, and one of 33
    assert {0, 1, 2, 3} <= seen["tiles"] and max(seen["tiles"]) > 3, seen["tiles"]
    assert offgrid and stretch and ragged
    assert {1, 10, 100, 1000, 1024} <= {c.depth for c in CASES}
    assert {0, MAXB} <= {c.base for c in CASES}
    big = next(c for c in CASES if c.n == N_BIG)
    pb = case_plan(big, MI355X_CUS)
    assert pb.kind == "regular" and pb.branches[1] == "n-max" and pb.chunks[1][1] == N_BIG - pb.pool_max
    assert pb.chunks[1][1] % TILE != 0                                  # the next chunk starts mid-tile


# ==================================================================== CPU: no packed-f32 forms where DESIGN 4.1a / 7 says so
def _kernel_asm(src: str):
    """{mangled kernel name: its assembly} of one source compiled to gfx950 assembly with the library's flags."""
    from openintel_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        r = subprocess.run([b.HIPCC, *b.FLAGS, "--cuda-device-only", "-S", os.path.join(b.CSRC, src), "-o", out],
                           capture_output=True, text=True, cwd=tmp)
        assert r.returncode == 0, r.stderr[-4000:]
        with open(out) as f:
            text = f.read()
    kernels, name, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
        elif name and line.startswith(".Lfunc_end"):
            kernels[name] = "\n".join(body)
            name = None
        elif name:
            body.append(line)
    return kernels


def _find(kernels, base):
    hits = [k for k in kernels if base in k]
    assert len(hits) == 1, (base, hits)
    return kernels[hits[0]]


PK_F32 = re.compile(r"^\s*v_pk_(fma|mul|add)_f32\b.*$", re.M)


@pytest.mark.skipif(not os.path.exists(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")), reason="no hipcc")
def test_isa_rescreen_and_rescore_have_no_packed_f32():
    """pf_rescreen_kernel and pf_rescore_kernel (the non-MFMA kernels the screen runs beside another lane's MFMA stream) hold no
    v_pk_{fma,mul,add}_f32 at all; i8s_stage_both_kernel (both staging bodies) and pf_stage_queries_kernel hold none with an
    op_sel:[...] operand (the documented failing form; op_sel_hi alone is not it)."""
    i8 = _kernel_asm("cosine_screen_i8.hip")
    pf = _kernel_asm("cosine_prefilter.hip")
    for k in (_find(i8, "pf_rescreen_kernel"), _find(pf, "pf_rescore_kernel")):
        assert not PK_F32.findall(k), [m.group(0) for m in PK_F32.finditer(k)]
    for k in (_find(i8, "i8s_stage_both_kernel"), _find(pf, "pf_stage_queries_kernel")):
        bad = [m.group(0).strip() for m in PK_F32.finditer(k) if re.search(r"\bop_sel:\[", m.group(0))]
        assert not bad, bad


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
def stream_ctx():
    import openintel_amd as oi
    from openintel_amd import _lib
    s = oi.HipContext(0)
    s.set_cosine_mode(_lib.OI_COSINE_SCREEN_STREAM)
    yield s
    s.close()


_BASE = {}


def base_rows(dim: int, n: int) -> np.ndarray:
    """Seeded unit rows, built once per module and dim (in blocks: no float64 copy of the whole matrix)."""
    from openintel_amd import synth
    have = _BASE.get(dim)
    if have is None or have.shape[0] < n:
        want = max([c.n for c in CASES if c.dim == dim] + [n])
        out = np.empty((want, dim), dtype=np.float32)
        blk = 1 << 19
        for i, r in enumerate(range(0, want, blk)):
            out[r:r + blk] = synth.embeddings_np(min(blk, want - r), dim, seed=7001 + 17 * dim + i)
        _BASE[dim] = have = out
    return have[:n]


def _forward(rng, n):
    lens = rng.integers(1, 9, size=n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    return rng.integers(0, VOCAB, size=int(offs[-1])).astype(np.uint32), offs


def _index(ctx, rows, base, fwd):
    import openintel_amd as oi
    idx = oi.HybridIndex(ctx, rows.shape[0], rows.shape[1], VOCAB, base)
    idx.set_embeddings(rows, normalize=False)
    idx.set_forward(*fwd)
    idx.finalize()
    return idx


class Run(NamedTuple):
    La: object
    Ls: object
    Ra: object
    Rs: object
    launches: dict
    gate: float
    gate_s: float


def run_both(stream_ctx, rows, q, depth, base=0, spec=True, hybrid=False, k=10, short_rows_only=True):
    """One search through the int8 route (a fresh ctx: its speculation back-off state is its own) and one through the f32-stream
    screen; the int8 search's launches per tag and both gates."""
    import openintel_amd as oi
    from openintel_amd import _lib
    n, dim = rows.shape
    B = q.shape[0]
    rng = np.random.default_rng(n + B)
    fwd = _forward(rng, n)
    qo = np.arange(0, 2 * B + 1, 2, dtype=np.uint32)
    qt = rng.integers(0, VOCAB, size=2 * B).astype(np.uint32)
    a = oi.HipContext(0)
    try:
        a.set_cosine_mode(_lib.OI_COSINE_SCREEN)
        a.set_screen_speculation(spec)
        ia = _index(a, rows, base, fwd)
        assert ia.index_bytes()[1] >= 3 * n * dim, "the index holds both screening copies"
        if short_rows_only:
            assert ia.long_rows() == 0, "no row is set aside as long: every row goes through the int8 bound"
        a.profile_reset(1)
        La = ia.search_lists(q, qt, qo, depth=depth)
        launches = {t: int(a.profile_read(t)[1]) for t in ("cosine", "spec", "rescreen")}
        gate = float(a.profile_read("screen_gate")[0])
        a.profile_reset(0)
        Ra = ia.search(q, qt, qo, k=k, depth=depth) if hybrid else None
        ia.close()
    finally:
        a.close()
    stream_ctx.set_screen_speculation(spec)
    i_s = _index(stream_ctx, rows, base, fwd)
    Ls = i_s.search_lists(q, qt, qo, depth=depth)
    gate_s = float(stream_ctx.profile_read("screen_gate")[0])
    Rs = i_s.search(q, qt, qo, k=k, depth=depth) if hybrid else None
    i_s.close()
    stream_ctx.set_screen_speculation(True)
    return Run(La, Ls, Ra, Rs, launches, gate, gate_s)


def same_lists(R: Run):
    assert np.array_equal(R.La.cos_counts, R.Ls.cos_counts)
    assert np.array_equal(R.La.cos_docs, R.Ls.cos_docs)
    assert np.array_equal(R.La.cos_scores.view(np.uint32), R.Ls.cos_scores.view(np.uint32))
    if R.Ra is not None:
        assert np.array_equal(R.Ra.counts, R.Rs.counts) and np.array_equal(R.Ra.docs, R.Rs.docs)
        assert np.array_equal(R.Ra.scores.view(np.uint32), R.Rs.scores.view(np.uint32))


def check_oracle(L, b, ref, depth, n, base):
    """test_gpu_screen_i8.py's bar against the f64 reference, and exact ties in doc-id order."""
    c = int(L.cos_counts[b])
    assert c == min(depth, n), b
    d, s = L.cos_docs[b][:c].astype(np.int64) - base, L.cos_scores[b][:c]
    assert np.unique(d).size == c and d.min() >= 0 and d.max() < n, b
    assert np.abs(s.astype(np.float64) - ref[d]).max() <= COS_TOL, b
    assert (np.diff(s.astype(np.float64)) <= 0).all(), b
    tied = s[1:].view(np.uint32) == s[:-1].view(np.uint32)
    assert (d[1:][tied] > d[:-1][tied]).all(), ("exact ties out of doc-id order", b)
    kth = np.sort(ref)[::-1][c - 1]
    assert np.isin(np.nonzero(ref > kth + 2 * COS_TOL)[0], d).all(), ("a clearly better doc is missing", b)
    assert (ref[d] >= kth - 2 * COS_TOL).all(), ("a clearly worse doc is present", b)


def check_all(O, R: Run, rows, q, depth, base, queries=None):
    same_lists(R)
    n = rows.shape[0]
    for b in (range(q.shape[0]) if queries is None else queries):
        check_oracle(R.La, b, O.dot_scores(rows, q[b]).astype(np.float64), depth, n, base)


def listed(L, b, base):
    c = int(L.cos_counts[b])
    return L.cos_docs[b][:c].astype(np.int64) - base


# ==================================================================== GPU: the table
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_int8_case(stream_ctx, O, num_cus, case):
    """Schedule, lists against the stream screen and the oracle; identical rows at both sides of every chunk boundary the mirror
    predicts (including the one off the tile grid), each pair the top of one query: both listed, in doc-id order."""
    from openintel_amd import synth
    p = case_plan(case, num_cus)
    n, base = case.n, case.doc_base()
    rows = base_rows(case.dim, n)
    q = synth.embeddings_np(case.B, case.dim, seed=90 + case.B + case.dim)
    bounds = [r for (r, _) in p.chunks[1:]]
    tie_q = {}
    saved = {r: rows[r - 1:r + 1].copy() for r in bounds}
    try:
        for i, r in enumerate(bounds):
            b = (5 * i + 1) % case.B
            rows[r - 1] = rows[r] = q[b]
            tie_q[b] = r
        R = run_both(stream_ctx, rows, q, case.depth, base, case.spec, case.hybrid)
        assert R.launches["cosine"] == len(p.chunks), (R.launches, p.chunks)
        assert R.launches["spec"] == p.spec_launches, (R.launches, p)
        assert R.launches["rescreen"] == 1, R.launches
        assert R.gate == 0.0, "the int8 tier holds on unit rows"
        # every query of a small case; of a large one every 7th, both sides of every group edge and the tie queries
        edges = {0, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 191, 192, 255, case.B - 1}
        checked = range(case.B) if n * case.B <= 10_000_000 else sorted((set(range(0, case.B, 7)) | edges | set(tie_q)) & set(range(case.B)))
        check_all(O, R, rows, q, case.depth, base, checked)
        for b, r in tie_q.items():
            d = listed(R.La, b, base)
            assert r - 1 in d and (case.depth == 1 or r in d), (b, r)
            if case.depth > 1:
                i = int(np.nonzero(d == r - 1)[0][0])
                assert d[i + 1] == r and R.La.cos_scores[b][i] == R.La.cos_scores[b][i + 1], (b, r)
    finally:
        for r, v in saved.items():
            rows[r - 1:r + 1] = v


# ==================================================================== GPU: named adversaries
def _scaled_background(dim, n, norm, zero_first=False):
    x = base_rows(dim, n).copy()
    if zero_first:
        x[:, 0] = 0.0
        x /= np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True).astype(np.float32)
    return (x * np.float32(norm)).astype(np.float32)


def _queries(dim, B, seed):
    from openintel_amd import synth
    return synth.embeddings_np(B, dim, seed=seed)


def _i8_estimate(x, q):
    """Host model of the int8 tier for rows x and query q (a query int8 staging leaves exact): (s~, e_r) in f64."""
    s = (np.abs(x).max(axis=1) / np.float32(127)).astype(np.float64)
    i = np.clip(np.rint(x / np.where(s > 0, s, 1)[:, None]), -127, 127)
    xh = s[:, None] * i
    return xh @ q.astype(np.float64), np.linalg.norm(xh - x.astype(np.float64), axis=1)


def _winners_and_decoys(R, win, depth):
    d = listed(R.La, 0, 0)
    assert set(win) <= set(d.tolist()), "a winner the int8 estimate ranks below the decoys is missing"
    assert np.array_equal(d[len(win):], np.arange(depth - len(win))), "the decoys fill the list in doc-id order"


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [384, 768])
def test_adversary_a_bound_tight_winners(stream_ctx, O, dim):
    """Winners x = s (i + 0.49 sign(q)), i in +-[40, 80], with the absmax pinned at 127 s: the quantisation error points straight at the sign
    query, s~ sits ~ e_r |q^| BELOW the true score.  Decoys (200 identical rows in the first chunk) round the other way: their s~
    is above the winners' s~ + e_r while their true score is below the winners'.  Keys that were s~ instead of the lower bound
    s~ - m_r (or a bound without e_r |q^|) put the carried threshold above the winners' upper bounds: the last chunk (whose last,
    ragged tile holds winners) drops them.  Speculation off: the proven thresholds alone."""
    rng = np.random.default_rng(dim)
    n, B, depth, n_dec, n_win = 50_001, 16, 100, 200, 40
    sg = rng.choice(np.array([-1.0, 1.0]), size=dim)
    q = _queries(dim, B, 11 + dim)
    q[0] = (sg / np.sqrt(dim)).astype(np.float32)
    I = rng.integers(40, 81, size=dim) * sg        # (varied magnitudes: bf16 errors like a random row's, no long rows)
    I[0] = 127.0 * sg[0]
    P, Rr = float(I @ q[0]), float(sg[1:] @ q[0, 1:].astype(np.float64))
    s_w = 0.9 / (P + 0.49 * Rr)
    s_d = (0.9 - 0.2 * Rr * s_w) / (P + 0.51 * Rr)

    def row(s, frac):
        x = s * (I + frac * sg)
        x[0] = s * I[0]
        return x.astype(np.float32)
    xw, xd = row(s_w, 0.49), row(s_d, 0.51)
    rows = _scaled_background(dim, n, float(np.linalg.norm(xw)))
    win = np.arange(n - n_win, n)
    rows[:n_dec] = xd
    rows[win] = xw
    est, er = _i8_estimate(np.stack([xw, xd]), q[0])
    true = np.stack([xw, xd]).astype(np.float64) @ q[0].astype(np.float64)
    assert true[0] > true[1] + 1e-3, "winners are truly above the decoys"
    assert est[0] + er[0] < est[1] - 1e-3, "s~ + e_r of a winner is below the decoys' s~: a bound missing a term drops it"
    R = run_both(stream_ctx, rows, q, depth, 0, spec=False)
    assert R.gate == 0.0, "the int8 tier holds (the exact pipeline would hide a dropped row)"
    assert R.launches["cosine"] == 2
    check_all(O, R, rows, q, depth, 0)
    _winners_and_decoys(R, win, depth)


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [384, 768])
def test_adversary_a_query_residual_needs_c_q(stream_ctx, O, dim):
    """Rows exact in int8 (e_r = 0) and a query whose int8 staging rounds every coordinate but the first to zero: the only error
    of s~ is x . (q^ - q), which the bound carries in c_q (X |e_q|).  Winners lean against e_q (s~ below the truth), decoys with
    it (s~ above): without c_q the decoys' keys exceed every winner's upper bound and the last chunk drops the winners."""
    rng = np.random.default_rng(dim + 1)
    n, B, depth, n_dec, n_win = 50_001, 16, 100, 200, 40
    sg = rng.choice(np.array([-1.0, 1.0]), size=dim)
    a = np.float32(1.0) / np.float32(127.0)
    q = _queries(dim, B, 12 + dim)
    q[0] = (0.4 * (a / 128.0) * sg).astype(np.float32)
    q[0, 0] = 1.0
    t = q[0] / a
    h = np.rint(t)
    assert (h[1:] == 0).all() and (np.rint((t - h) * 128)[1:] == 0).all(), "every coordinate but the first stages to zero"
    iw, idc = 100.0 * sg, -100.0 * sg
    iw[0] = idc[0] = 127.0
    s_w = 2.0 ** -7
    xw, xd = (s_w * iw).astype(np.float32), (s_w * 129 / 128 * idc).astype(np.float32)
    rows = _scaled_background(dim, n, float(np.linalg.norm(xw)), zero_first=True)
    win = np.arange(n - n_win, n)
    rows[:n_dec] = xd
    rows[win] = xw
    est, er = _i8_estimate(np.stack([xw, xd]), np.where(np.arange(dim) == 0, q[0], 0.0))
    true = np.stack([xw, xd]).astype(np.float64) @ q[0].astype(np.float64)
    assert er.max() == 0.0 and true[0] > true[1] + 1e-3 and est[0] < est[1] - 1e-3
    R = run_both(stream_ctx, rows, q, depth, 0, spec=False)
    assert R.gate == 0.0
    check_all(O, R, rows, q, depth, 0)
    _winners_and_decoys(R, win, depth)


def _negative_rows(dim, n, seed):
    """Unit rows with a common direction u (x . u > 0 for every row) and u."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(dim)
    u /= np.linalg.norm(u)
    x = base_rows(dim, n).astype(np.float64) + 0.5 * u
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    assert (x @ u).min() > 0
    return x.astype(np.float32), u


@pytest.mark.gpu
@pytest.mark.parametrize("dim,n,depth", [(768, 100_003, 100), (384, 77_777, 1000), (384, 8_191, 10)])
def test_adversary_b_negative_thresholds_ragged(stream_ctx, O, dim, n, depth):
    """Every score of half the queries is below 0 and n % 32 != 0: the padding rows of the ragged last tile score 0 and only
    the tile mask keeps them out -- no doc id at or past n may ever be listed."""
    rows, u = _negative_rows(dim, n, dim + n)
    B = 24
    q = _queries(dim, B, 13 + n)
    for b in range(0, B, 2):
        v = -u + 0.3 * q[b]
        q[b] = (v / np.linalg.norm(v)).astype(np.float32)
    for b in range(0, B, 2):
        assert O.dot_scores(rows, q[b]).max() < 0
    R = run_both(stream_ctx, rows, q, depth, 0)
    assert R.gate == 0.0
    check_all(O, R, rows, q, depth, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("K,gate", [(4_000, 0.0), (5_000, 1.0), (12_000, 1.0), (16_385, 1.0)])
def test_adversary_c_carry_edges(stream_ctx, O, K, gate):
    """K exact copies of a row close to query 0.  4 000 fit both the int8 carry (16 384) and the bf16 rescreen's final select
    (4 096): the tier holds.  5 000 and 12 000 fit the int8 carry but not the final select: its margin overflow writes gate = 1
    (select.hip: select_flat_kernel).  16 385 overflow the int8 carry itself: gate = 1.  The lists are the oracle's in every
    case, the copies listed in doc-id order."""
    n, dim, B, depth = 60_000, 768, 16, 100
    rng = np.random.default_rng(K)
    rows = _scaled_background(dim, n, 1.0)
    q = _queries(dim, B, 14)
    v = q[0] + 0.2 * rows[1]
    dup = np.sort(rng.choice(n, size=K, replace=False))
    rows[dup] = (v / np.linalg.norm(v)).astype(np.float32)
    R = run_both(stream_ctx, rows, q, depth, 0)
    assert R.gate == gate, (K, R.gate)
    check_all(O, R, rows, q, depth, 0, queries=range(0, B, 3))
    assert np.array_equal(listed(R.La, 0, 0), dup[:depth])


@pytest.mark.gpu
@pytest.mark.parametrize("B", [97, 129])
def test_adversary_d_distinct_query_groups(stream_ctx, O, B):
    """Queries 64..96 are the negations (B = 97) or coordinate permutations (B = 129) of queries 0..32, each query with rows of
    its own near it: a group's pool, carry, threshold or query offset taken from another group returns that group's lists."""
    n, dim, depth = 100_000, 768, 100
    rng = np.random.default_rng(B)
    q = _queries(dim, B, 15 + B)
    q[64:97] = -q[0:33] if B == 97 else q[0:33][:, rng.permutation(dim)]
    rows = _scaled_background(dim, n, 1.0)
    near = rng.permutation(n)[:B * 20].reshape(B, 20)
    for b in range(B):
        v = q[b][None, :] + 0.3 * rows[near[b]]
        rows[near[b]] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    R = run_both(stream_ctx, rows, q, depth, 0, hybrid=True)
    assert R.gate == 0.0
    check_all(O, R, rows, q, depth, 0)
    for b in range(B):
        assert set(near[b]) <= set(listed(R.La, b, 0).tolist()), b


@pytest.mark.gpu
def test_adversary_e_degenerate_queries(stream_ctx, O):
    """A zero query and a query of norm 1e-13 in a batch of 40: both get m2 = inf (no bound), the gate opens, every list is right
    and the zero query's is the first `depth` doc ids."""
    n, dim, B, depth = 50_000, 384, 40, 100
    rows = _scaled_background(dim, n, 1.0)
    q = _queries(dim, B, 16)
    q[7] = 0.0
    q[23] *= np.float32(1e-13)
    R = run_both(stream_ctx, rows, q, depth, 0)
    assert R.gate == 1.0
    check_all(O, R, rows, q, depth, 0)
    assert np.array_equal(listed(R.La, 7, 0), np.arange(depth))


@pytest.mark.gpu
def test_adversary_g_top_of_the_doc_id_range(stream_ctx, O):
    """doc_id_base = 2^32 - 1 - n with every query's best rows among the last ones: doc ids up to 2^32 - 2 (rows are recovered as
    doc - doc_id_base in u32 by the rescreen and the rescoring)."""
    n, dim, B, depth = 70_001, 768, 33, 100
    base = 2 ** 32 - 1 - n
    rows = _scaled_background(dim, n, 1.0)
    q = _queries(dim, B, 17)
    for b in range(B):
        v = q[b] + 0.1 * rows[b]
        rows[n - 1 - 3 * b] = (v / np.linalg.norm(v)).astype(np.float32)
    R = run_both(stream_ctx, rows, q, depth, base, hybrid=True)
    assert R.gate == 0.0
    check_all(O, R, rows, q, depth, base)
    for b in range(B):
        assert listed(R.La, b, base)[0] == n - 1 - 3 * b


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [384, 768])
def test_adversary_h_tiny_and_zero_rows(stream_ctx, O, dim):
    """Rows of absmax ~1e-39 (a denormal int8 scale) and all-zero rows (scale 0) among unit rows; half the queries score every
    unit row below 0, so the zero and tiny rows are their lists."""
    n, B, depth = 40_009, 24, 100
    rows, u = _negative_rows(dim, n, dim)
    rng = np.random.default_rng(dim + 5)
    pick = rng.choice(n, size=60, replace=False)
    tiny, zero = pick[:30], pick[30:]
    rows[tiny] = (rows[tiny] * np.float32(1e-39)).astype(np.float32)
    rows[zero] = 0.0
    q = _queries(dim, B, 18 + dim)
    for b in range(0, B, 2):
        v = -u + 0.3 * q[b]
        q[b] = (v / np.linalg.norm(v)).astype(np.float32)
    R = run_both(stream_ctx, rows, q, depth, 0)
    check_all(O, R, rows, q, depth, 0)
    for b in range(0, B, 2):
        assert set(pick) <= set(listed(R.La, b, 0).tolist()), b
