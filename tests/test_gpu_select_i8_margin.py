"""The margin selects of the int8 route (csrc/select.hip: sel_flat_select's fast margin path with row margins) at the edges of what
they keep in registers, and the speculative threshold they compute on the way (SelectExtra::spec_rank).

With the pool's keys in registers (KPT = 4, 8, 16, 32 keys per thread: pools of up to 4 096, 8 192, 16 384, 32 768 keys) a margin
select tests every key ONCE -- the global threshold, then the row's own bound from the int8 copy's metadata, the verdicts kept in a
bit mask -- writes the survivors straight into the pool's carry region, and, after the first chunk of a speculating search, finds
the r-th largest score key among them: the words pf_spec_kernel used to compute in a launch of its own.  A wrong mask bit, slot or
rank drops or adds a row on some data only, so every case here runs through the public search path on an index with both
screening copies, default mode (B > 8: the int8 route), and is compared BIT FOR BIT with OI_COSINE_EXACT on embeddings of small
integers, where every dot product is exact in f32, bf16 and int8 alike; unit rows are checked against the f64 oracle.

The first chunk has no threshold, so its select sees exactly its rows as keys, per query: 8 192 rows at depth <= 256, 16 384 at
depth 512, 28 672 (the rounded first chunk, 256 CUs) at depth 1000, and up to a quarter more where that is all that is left.
Rows reach the pool in 128-row segments whose inner order is the screen's (atomics); with 8 192 rows a wave of the select owns
512 consecutive rows, four whole segments."""
import numpy as np
import pytest

from test_gpu_screen_i8_edges import (OI_I8_CARRY, O, _forward, _index, _queries, check_oracle, listed, num_cus, plan,  # noqa: F401
                                      screen_first_chunk_rows, screen_geometry)

# Two cases the selects handle cannot be reached through oi_search, and have no test here:
#  * fewer than r carried keys (sel_spec_words' `have == false`: the proven threshold is handed on as it is).  A prediction is asked
#    for only when 2 r <= k' (search.hip: screen_chunk); the first chunk holds at least max(8 192, 8 k') rows and no threshold, so all
#    its rows are keys; at most 1 024 of them are set aside as long rows and a filtered search, which could pass fewer, never
#    speculates (plan_search).  So the select sees >= 7 168 valid keys, keeps at least the k' best, and k' >= 2 r > r.
#  * fewer than k' keys in play because of long rows: an index sets rows aside only when it has more than 4 096 and at most 1 024
#    of them, so more than 3 072 >= k' stay in play (test_long_rows_set_aside runs the dead-slot mask at its limit of 1 000 rows).
pytestmark = pytest.mark.gpu
DIM, B33 = 384, 33


@pytest.fixture(scope="module")
def exact_ctx():
    import openintel_amd as oi
    from openintel_amd import _lib
    e = oi.HipContext(0)
    e.set_cosine_mode(_lib.OI_COSINE_EXACT)
    yield e
    e.close()


_ROWS = {}


def int_rows(n, dim=DIM):
    """Seeded rows of {-1, 0, 1} (never all zero), generated once per dim and cut: exact in int8 (absmax scale 1 / 127) and bf16."""
    have = _ROWS.get(dim)
    if have is None or have.shape[0] < n:
        rng = np.random.default_rng(4100 + dim)
        have = rng.integers(-1, 2, size=(max(n, 90_000 if dim == DIM else 9_000), dim)).astype(np.float32)
        have[:, 0] = np.where(np.abs(have).sum(axis=1) == 0, 1.0, have[:, 0])
        _ROWS[dim] = have
    return have[:n].copy()


def int_queries(B, dim=DIM, seed=1):
    q = np.random.default_rng(4200 + seed).integers(-2, 3, size=(B, dim)).astype(np.float32)
    q[:, 0] = np.where(np.abs(q).sum(axis=1) == 0, 1.0, q[:, 0])
    return q


def winner(qb, zeros=0):
    """The best ternary row for query qb, less `zeros` of its nonzero coordinates (score = sum |q| less those entries)."""
    w = np.sign(qb).astype(np.float32)
    nz = np.nonzero(w)[0][:zeros]
    w[nz] = 0.0
    return w


class Got:
    def __init__(self, La, Le, gate, launches, failures, searches):
        self.La, self.Le, self.gate, self.launches, self.failures, self.searches = La, Le, gate, launches, failures, searches


def run_pair(exact_ctx, rows, q, depth, spec=True, base=0):
    """One search through the default mode (a fresh ctx: its speculation state is its own) and one through the exact scorer."""
    import openintel_amd as oi
    from openintel_amd import _lib
    n, dim = rows.shape
    B = q.shape[0]
    rng = np.random.default_rng(n + B)
    fwd = _forward(rng, n)
    qo = np.arange(0, 2 * B + 1, 2, dtype=np.uint32)
    qt = rng.integers(0, 50, size=2 * B).astype(np.uint32)
    a = oi.HipContext(0)
    try:
        a.set_cosine_mode(_lib.OI_COSINE_SCREEN)
        a.set_screen_speculation(spec)
        ia = _index(a, rows, base, fwd)
        assert ia.index_bytes()[1] >= 3 * n * dim, "the index holds both screening copies"
        f0, s0 = a.speculation_state()
        a.profile_reset(1)
        La = ia.search_lists(q, qt, qo, depth=depth)
        launches = {t: int(a.profile_read(t)[1]) for t in ("cosine", "spec", "rescreen")}
        gate = float(a.profile_read("screen_gate")[0])
        a.profile_reset(0)
        assert launches["rescreen"] == (1 if B > 8 else 0), "B > 8 takes the int8 route (one rescreen), B <= 8 the bf16 copy screen"
        f1, s1 = a.speculation_state()
        ia.close()
    finally:
        a.close()
    ie = _index(exact_ctx, rows, base, fwd)
    Le = ie.search_lists(q, qt, qo, depth=depth)
    ie.close()
    return Got(La, Le, gate, launches, f1 - f0, s1 - s0)


def same_bits(G, queries=None):
    qs = slice(None) if queries is None else list(queries)
    assert np.array_equal(G.La.cos_counts[qs], G.Le.cos_counts[qs])
    assert np.array_equal(G.La.cos_docs[qs], G.Le.cos_docs[qs])
    assert np.array_equal(G.La.cos_scores[qs].view(np.uint32), G.Le.cos_scores[qs].view(np.uint32))


# ==================================================================== the register paths of the first select
# (n_docs, depth, keys the first select sees, chunks) at 256 CUs.  A tail of at most a quarter of a chunk is taken along with it
# (search.hip: oi_chunk_end), so one row more than the first chunk's length is still ONE chunk, of one key more -- the first pool of
# the next KPT -- and a second chunk, with a threshold and a carry, follows from a quarter more: 10 241 and 35 841 rows.
FIRST = [(4095, 100, 4095, 1), (4096, 100, 4096, 1), (4097, 100, 4097, 1), (8191, 100, 8191, 1), (8192, 100, 8192, 1),
         (8193, 100, 8193, 1), (10241, 100, 8192, 2), (16384, 512, 16384, 1), (28672, 1000, 28672, 1), (28673, 1000, 28673, 1),
         (35840, 1000, 35840, 1), (35841, 1000, 28672, 2)]


@pytest.mark.parametrize("n,depth,keys,chunks", FIRST, ids=["n%d" % f[0] for f in FIRST])
def test_first_select_at_the_register_path_boundaries(exact_ctx, num_cus, n, depth, keys, chunks):
    """4 095 / 4 096 | 4 097 / 8 191 / 8 192 | 8 193 / 16 384 | 28 672 / 28 673 keys: the last pool of KPT = 4, both ends of 8, both
    ends of 16, and 32; 35 840 keys: the re-loading path (KPT = 0), which keeps the candidate buffer; 10 241 and 35 841 rows: the
    smallest corpora with a second chunk behind a first one of 8 192 and 28 672 rows.  33 queries: the second query tile is ragged."""
    p = plan(n, B33, depth, num_cus)
    if num_cus == 256:
        assert p.chunks[0][1] == keys and len(p.chunks) == chunks
    G = run_pair(exact_ctx, int_rows(n), int_queries(B33), depth)
    assert G.launches["cosine"] == len(p.chunks) and G.launches["spec"] == p.spec_launches
    assert G.gate == 0.0
    same_bits(G)


def test_first_select_unit_rows_against_the_oracle(exact_ctx, O):
    """The same boundary (8 192 keys, then a second chunk) on unit rows: the f64 oracle's bar."""
    from openintel_amd import synth
    n, depth = 10241, 100
    rows, q = synth.embeddings_np(n, DIM, seed=4301), _queries(DIM, B33, 4302)
    G = run_pair(exact_ctx, rows, q, depth)
    assert G.gate == 0.0
    for b in range(0, B33, 4):
        check_oracle(G.La, b, O.dot_scores(rows, q[b]).astype(np.float64), depth, n, 0)


# ==================================================================== fewer valid keys than k'
@pytest.mark.parametrize("n,depth", [(700, 1000), (1000, 1000), (1001, 1000)])
def test_pool_no_larger_than_the_depth(exact_ctx, n, depth):
    """n_docs < k', = k' and k' + 1: the selects that keep everything, and the smallest one that selects."""
    G = run_pair(exact_ctx, int_rows(n), int_queries(B33), depth)
    same_bits(G)
    assert (G.La.cos_counts == min(n, depth)).all()


def test_long_rows_set_aside(exact_ctx):
    """1 000 rows of three times the norm among 5 000: they are set aside as long (skipped by the margin selects: dead slots under the
    verdict mask, rescored whatever happens) and, being long, hold most places of every list of depth 1000.  (An index sets aside
    at most 1 024 rows and only when it has more than 4 096, so the keys in play never fall below k' this way.)"""
    import openintel_amd as oi
    n, depth = 5000, 1000
    rows = int_rows(n) * np.float32(1 + 2.0 ** -9)     # (not exact in bf16: the index looks for long rows only where bf16 rounds;
    rows[np.arange(3, n, 5)] *= 3.0                     # the f32 sums of 10-bit values times small integers stay exact)
    a = oi.HipContext(0)
    ia = _index(a, rows, 0, _forward(np.random.default_rng(1), n))
    n_long = ia.long_rows()
    ia.close()
    a.close()
    assert n_long == 1000
    G = run_pair(exact_ctx, rows, int_queries(B33), depth)
    assert G.gate == 0.0
    same_bits(G)


# ==================================================================== the verdict mask
def test_single_survivors_in_every_slot(exact_ctx, num_cus):
    """depth 8, eight planted rows per query, far above everything else and one score apart: the eight are the only survivors of
    the select, each alone in its thread.  Over the 33 queries they sit at the first and the last rows of the 128-row segments that
    begin and end a wave's 512 rows (slots 0 / 1 and kpt - 2 / kpt - 1, whatever order the screen wrote a segment in) and in
    between: a survivor in a thread's first slot only, in its last only, anywhere (the row-to-slot mapping: _one_quad_per_segment;
    test_only_survivor_pinned_to_a_slot pins the first and the last slot exactly)."""
    n, depth = 8192, 8
    assert _one_quad_per_segment(n, num_cus) == 8
    rows, q = int_rows(n), int_queries(B33, seed=2)
    planted = {}
    for b in range(B33):
        w0 = (b % 16) * 512
        at = [w0, w0 + 127, w0 + 384 + (b % 128), w0 + 511, (w0 + 512 * 5 + 64 * (b % 8)) % n, (w0 + 512 * 9 + 64 * (b % 8) + 63) % n,
              (w0 + 512 * 11 + 200 + b) % n, (w0 + 512 * 13 + 300 + b) % n]
        planted[b] = at
    used = set()
    for b, at in planted.items():
        for i, r in enumerate(at):
            while r in used:
                r = (r + 1) % n
            used.add(r)
            at[i] = r
            rows[r] = winner(q[b], zeros=i)
    G = run_pair(exact_ctx, rows, q, depth)
    assert G.gate == 0.0
    same_bits(G)
    for b, at in planted.items():
        assert np.array_equal(listed(G.La, b, 0), np.array(at)), b


def _one_quad_per_segment(n, num_cus):
    """Where a row's key sits in the first select's flat view.  A chunk of at most 7/8 of the CUs x 128 rows gets one workgroup and
    one pool segment per QUAD of four 32-row tiles (cosine_prefilter.hip: oi_cosine_screen_geometry -- grid = quads, seg_cap = 128;
    cosine_screen_i8.hip: wave w of workgroup b takes tile 4 b + w), so segment b holds rows 128 b .. 128 b + 127 in the order the four
    waves' atomics gave them.  select_flat_kernel scans the segment counts into offsets (carry empty: flat index = offset + position),
    wave w owns the flat range [w kpt 64, (w + 1) kpt 64), kpt = ceil(n / 1024), and thread (w, lane)'s slot j is flat index
    w kpt 64 + 64 j + lane.  A row's slot is therefore known up to the order inside its segment: exactly when the segment's rows
    fill one 64-key slot -- the ragged last segment of a corpus of 128 s + 64 rows."""
    grid, cap = screen_geometry(n, num_cus)
    assert cap == 128 and grid == (n + 127) // 128, (grid, cap)
    return (n + 1023) // 1024


@pytest.mark.parametrize("n,slot", [(4800, "last"), (4544, "first")])
def test_only_survivor_pinned_to_a_slot(exact_ctx, num_cus, n, slot):
    """kpt = 5.  4 800 = 15 x 5 x 64 rows: the last segment's 64 rows (4 736 ..) are wave 14's slot 4 = kpt - 1, whatever their order;
    4 544 = 14 x 5 x 64 + 64 rows: the last segment's 64 rows (4 480 ..) are wave 14's slot 0, its other slots past the end.  Eight
    queries' eight winners each fill those 64 rows (depth 8: nothing else survives), so every surviving key is its thread's only
    one and sits in the last, or the first, slot."""
    kpt = _one_quad_per_segment(n, num_cus)
    start = n - 64
    assert kpt == 5 and start % 128 == 0 and start - 14 * kpt * 64 == (4 * 64 if slot == "last" else 0)
    depth = 8
    rows, q = int_rows(n), int_queries(B33, seed=4)
    for b in range(8):
        for i in range(8):
            rows[start + 8 * i + b] = winner(q[b], zeros=i)
    G = run_pair(exact_ctx, rows, q, depth)
    assert G.gate == 0.0
    same_bits(G)
    for b in range(8):
        assert np.array_equal(listed(G.La, b, 0), start + 8 * np.arange(8) + b), b


def test_full_waves_around_an_empty_one(exact_ctx):
    """Query 0's best row 512 times in rows 0 .. 511 and 512 times in rows 1 024 .. 1 535, all tied: every slot of every thread of
    waves 0 and 2 survives, wave 1 (rows 512 .. 1 023) keeps nothing.  Ties list in doc-id order."""
    n, depth = 8192, 100
    rows, q = int_rows(n), int_queries(B33, seed=3)
    rows[0:512] = winner(q[0])
    rows[1024:1536] = winner(q[0])
    G = run_pair(exact_ctx, rows, q, depth)
    assert G.gate == 0.0
    same_bits(G)
    assert np.array_equal(listed(G.La, 0, 0), np.arange(depth))


# ==================================================================== the carry region, written directly, at its capacity
def _row_with_score(q0, r1, target):
    """normalise(q0 + a r1) whose f64 score against q0 is `target` (bisection over a; f32 row)."""
    lo, hi = 0.0, 4.0
    for _ in range(60):
        a = 0.5 * (lo + hi)
        v = q0.astype(np.float64) + a * r1.astype(np.float64)
        v = (v / np.linalg.norm(v)).astype(np.float32)
        if float(v.astype(np.float64) @ q0.astype(np.float64)) > target:
            lo = a
        else:
            hi = a
    return v


@pytest.mark.parametrize("K,gate", [(OI_I8_CARRY, 0.0), (OI_I8_CARRY + 1, 1.0)])
def test_carry_region_full_and_overflowing(exact_ctx, O, K, gate):
    """test_adversary_c_carry_edges' construction with survivors the int8 tier cannot tell from the winners and the bf16 tier can:
    100 copies of a row W close to query 0 and K - 100 copies of a row D scoring 0.0105 less -- inside the int8 rows' margin
    (the two rows' widths, 0.0148 for these unit rows of 768 dims by the host model of the tier), outside the bf16 screen's
    (2 eps = 0.0074).  The last int8 margin select keeps
    exactly K keys of query 0: 16 384 fill the carry region to its last slot (gate shut, the bf16 select keeps the 100), 16 385
    overflow it (gate open).  The lists are the oracle's either way, the copies of W in doc-id order."""
    from openintel_amd import synth
    n, dim, B, depth = 60_000, 768, 16, 100
    rng = np.random.default_rng(K)
    rows = synth.embeddings_np(n, dim, seed=4401)
    q = _queries(dim, B, 14)
    W = _row_with_score(q[0], rows[1], 0.975)
    D = _row_with_score(q[0], rows[1], 0.975 - 0.0105)
    dup = np.sort(rng.choice(n, size=K, replace=False))
    wins = np.sort(rng.choice(dup, size=depth, replace=False))
    rows[dup] = D
    rows[wins] = W
    G = run_pair(exact_ctx, rows, q, depth)
    for b in range(0, B, 3):
        check_oracle(G.La, b, O.dot_scores(rows, q[b]).astype(np.float64), depth, n, 0)
    assert np.array_equal(listed(G.La, 0, 0), wins)
    assert G.gate == gate, (K, G.gate)


# ==================================================================== the prediction computed in the select
def test_speculation_on_a_fair_sample(exact_ctx, num_cus):
    """Three first-chunk lengths of i.i.d. rows at depth 1000: the search takes the short first chunk, its select predicts the
    threshold of the rest (rank 3 k' m / n + 12), the check at the end passes."""
    depth = 1000
    n = 3 * screen_first_chunk_rows(depth, num_cus)
    p = plan(n, B33, depth, num_cus)
    assert p.spec_launches == 1
    G = run_pair(exact_ctx, int_rows(n), int_queries(B33, seed=5), depth)
    assert G.launches["spec"] == 1 and G.launches["cosine"] == len(p.chunks)
    assert G.gate == 0.0 and G.failures == 0 and G.searches == 1
    same_bits(G)


def test_speculation_fails_on_planted_first_rows(exact_ctx, num_cus):
    """test_a_failed_speculation_opens_the_gate_and_backs_off at the smallest size that speculates at depth 100 (2 (300 x 8 192 / n
    + 12) <= 100: n >= 64 674): 60 near-copies of every query among the first 8 192 rows and none after.  The 48th best of the first
    chunk is a copy, the prediction sits far above the final threshold, the check fails, the gate opens; the lists are exact."""
    n, depth, B = 70_000, 100, 16
    assert plan(n, B, depth, num_cus).spec_launches == 1
    rows, q = int_rows(n), int_queries(B, seed=6)
    for b in range(B):
        for i in range(60):
            rows[100 + 60 * b + i] = winner(q[b], zeros=i % 7)
    G = run_pair(exact_ctx, rows, q, depth)
    assert G.launches["spec"] == 1
    assert G.gate != 0.0 and G.failures == 1 and G.searches == 1
    same_bits(G)
    for b in range(B):
        assert set(range(100 + 60 * b, 160 + 60 * b)) <= set(listed(G.La, b, 0).tolist())


def test_no_prediction_for_a_query_without_a_bound(exact_ctx, num_cus):
    """A zero query in a speculating batch has eps2 = +inf: its proven threshold stays at key 0 and what the prediction hands to the
    next chunk for it is key(score - inf) = key(-inf) = 0x007FFFFF, below every row: nothing is dropped on a prediction.  That word
    is above the proven key 0 all the same, so it is recorded in spec_max, and the check in the rescoring launch (spec_max > final
    threshold) counts ONE failed speculation for the batch -- what pf_spec_kernel's arithmetic did and the issue keeps ("behave as
    today"); the gate is open anyway, the query has no bound.  The select must write exactly those words: no failure counted means
    it skipped the query, and the fifteen bounded queries on i.i.d. rows fail no check (test_speculation_on_a_fair_sample).  Every
    list is exact; the zero query's is the first `depth` doc ids."""
    n, depth, B = 70_000, 100, 16
    rows, q = int_rows(n), int_queries(B, seed=7)
    q[5] = 0.0
    G = run_pair(exact_ctx, rows, q, depth)
    print("zero query in a speculating batch: spec launches %d gate %g failures %d searches %d" % (G.launches["spec"], G.gate, G.failures, G.searches))
    assert G.launches["spec"] == 1 and G.gate == 1.0
    assert G.searches == 1 and G.failures == 1
    same_bits(G)
    assert np.array_equal(listed(G.La, 5, 0), np.arange(depth))


# ==================================================================== staging
@pytest.mark.parametrize("dim", [384, 768])
@pytest.mark.parametrize("B", [1, 31, 32, 33, 64, 97])
def test_staged_queries_at_every_tile_edge(exact_ctx, B, dim):
    """The staged blocks (bf16 queries, margins and gate; int8 hi / lo and the four floats per query) at one query, both sides of a
    32-query tile and of a 64-query group.  (One query takes the bf16 copy screen: no int8 blocks.)"""
    n, depth = 9000, 50
    G = run_pair(exact_ctx, int_rows(n, dim), int_queries(B, dim, seed=8 + B), depth)
    assert G.gate == 0.0
    same_bits(G)


def test_staged_zero_and_nan_queries_open_the_gate(exact_ctx):
    """An all-zero query and one with a NaN among 33: neither has a bound, the gate opens, the other lists are exact."""
    n, depth = 9000, 50
    q = int_queries(B33, seed=9)
    q[3] = 0.0
    q[32, 17] = np.nan
    G = run_pair(exact_ctx, int_rows(n), q, depth)
    assert G.gate == 1.0
    same_bits(G, queries=[b for b in range(B33) if b != 32])
    assert np.array_equal(listed(G.La, 3, 0), np.arange(depth))
