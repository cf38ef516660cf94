"""The bf16 copy screen (csrc/cosine_screen_copy.hip: cosine_copy_screen over csrc/oi_screen_tile.h) at every tile, wave, chunk
and query-group edge.

An index told never to keep screening copies (set_screen_copy(NEVER)), searched in OI_COSINE_SCREEN_COPY: the first search makes
the bf16 copy and no int8 tier, so plan_search takes the copy screen for EVERY batch size -- NQT = 1 and 2 query tiles, one launch
per 64 queries and chunk.  Wave w of workgroup b owns the 32-row tiles b x 4 + w, stepping by grid x 4, and streams them through a
ring whose refills reach up to two tiles ahead and, past the wave's last tile, read an empty descriptor; the first chunk has no
threshold (dense tiles, straight to the pool), the later ones stage their survivors.  A wrong ring offset, descriptor, tile mask
or pool slot drops or adds a row on some shapes only.

Judges.  B > 8: the same rows through the f32-stream screen (OI_COSINE_SCREEN_STREAM, which never reads a copy) -- the two
screens make the same products, margins and survivors, so the lists are the same BIT FOR BIT -- and the f64 oracle's
bar.  B <= 8: the oracle's bar alone (the stream mode runs the f32 GEMV there, which sums in another order).  The filtered case:
test_gpu_filter's reference, the oracle's full ranking restricted to the passing documents.

Speculation is off (at depth 10 no prediction qualifies anyway: 2 r <= k' fails); one case repeats with the switch on."""
import numpy as np
import pytest

from test_gpu_screen_i8_edges import MI355X_CUS, O, check_oracle, listed, num_cus, plan, wave_tiles  # noqa: F401

VOCAB = 50
DEPTH = 10
N_BIG = 159_777           # 8 192 + 65 536 + 86 049 rows at B > 8; the last tile holds ONE row
B_MAX = 65
PF_CARRY = 4096           # search.hip, plan_search: keys per query the copy screen carries between chunks
SMALL_N = (1, 31, 32, 33, 129)


def big_plan(B, cus, spec=False):
    return plan(N_BIG, B, DEPTH, cus, spec=spec, pf_carry=PF_CARRY)


# ==================================================================== CPU: what the shapes reach, from the mirror at 256 CUs
def test_big_shape_reaches_every_tile_count_and_both_epilogues():
    """B > 8: chunks of 8 192 / 65 536 / 86 049 rows = at most 1, 3 and 4 tiles per wave (so my_nt = 1..4, refills two tiles ahead
    and the empty descriptor of tile ti + 3 are all run), a dense first chunk and staged later ones, a one-row last tile.  B = 8
    grows x 16: two chunks, more tiles per wave.  The switch for speculation changes nothing at depth 10."""
    for B in (9, 33, 64, 65):
        p = big_plan(B, MI355X_CUS)
        assert p.chunks == ((0, 8192), (8192, 73_728), (73_728, N_BIG)) and p.kind == "proven", p
        assert [e - r for r, e in p.chunks] == [8192, 65_536, 86_049]
        assert [max(wave_tiles(e - r, MI355X_CUS)) for r, e in p.chunks] == [1, 3, 4]
        assert set().union(*(wave_tiles(e - r, MI355X_CUS) for r, e in p.chunks)) >= {1, 2, 3, 4}
        assert big_plan(B, MI355X_CUS, spec=True) == p
    assert N_BIG % 32 == 1
    p8 = big_plan(8, MI355X_CUS)
    assert p8.chunks == ((0, 8192), (8192, N_BIG)) and max(wave_tiles(N_BIG - 8192, MI355X_CUS)) > 4, p8
    for n in SMALL_N:   # one chunk; waves without a tile beside waves with their only one
        assert plan(n, 64, DEPTH, MI355X_CUS, spec=False, pf_carry=PF_CARRY).chunks == ((0, n),)
        assert wave_tiles(n, MI355X_CUS) == {0, 1}


# ==================================================================== GPU
_ROWS, _QUERIES, _REF = {}, {}, {}


def rows_of(dim):
    from openintel_amd import synth
    if dim not in _ROWS:
        _ROWS[dim] = synth.embeddings_np(N_BIG, dim, seed=5200 + dim)
    return _ROWS[dim]


def queries_of(dim):
    """B_MAX unit queries per dim; a case of B queries takes the first B, so the oracle's scores are computed once per query."""
    from openintel_amd import synth
    if dim not in _QUERIES:
        _QUERIES[dim] = synth.embeddings_np(B_MAX, dim, seed=5300 + dim)
    return _QUERIES[dim]


def reference(O, dim, n, b):
    """f64 oracle scores of query b over the first n rows: computed once over all rows of the large shape, and once over the
    129 rows the small shapes are cut from."""
    key = (dim, b, n > max(SMALL_N))
    if key not in _REF:
        _REF[key] = O.dot_scores(rows_of(dim)[:N_BIG if key[2] else max(SMALL_N)], queries_of(dim)[b]).astype(np.float64)
    return _REF[key][:n]


def _terms(n, B):
    rng = np.random.default_rng(n + B)
    lens = rng.integers(1, 9, size=n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    fwd = (rng.integers(0, VOCAB, size=int(offs[-1])).astype(np.uint32), offs)
    return fwd, rng.integers(0, VOCAB, size=2 * B).astype(np.uint32), np.arange(0, 2 * B + 1, 2, dtype=np.uint32)


def _index(ctx, rows, fwd, attrs=None):
    import openintel_amd as oi
    from openintel_amd import _lib
    idx = oi.HybridIndex(ctx, rows.shape[0], rows.shape[1], VOCAB, 0)
    idx.set_embeddings(rows, normalize=False)
    idx.set_forward(*fwd)
    if attrs is not None:
        idx.set_doc_attrs(*attrs)
    idx.set_screen_copy(_lib.OI_SCREEN_COPY_NEVER)
    idx.finalize()
    return idx


def _ctx(mode, spec=False):
    import openintel_amd as oi
    c = oi.HipContext(0)
    c.set_cosine_mode(mode)
    c.set_screen_speculation(spec)
    return c


@pytest.fixture(scope="module")
def ctxs():
    """(copy-mode ctx, stream-mode ctx), speculation off."""
    from openintel_amd import _lib
    c, s = _ctx(_lib.OI_COSINE_SCREEN_COPY), _ctx(_lib.OI_COSINE_SCREEN_STREAM)
    yield c, s
    c.close()
    s.close()


def group_of(n):
    return np.random.default_rng(5400).integers(0, 7, size=n).astype(np.uint32)


@pytest.fixture(scope="module")
def big(ctxs):
    """{dim: (copy-mode index, stream-mode index)} over the N_BIG rows, built on first use and shared by the cases of a dim."""
    made = {}

    def get(dim):
        if dim not in made:
            fwd, _, _ = _terms(N_BIG, B_MAX)
            attrs = (group_of(N_BIG), np.arange(N_BIG, dtype=np.uint32))
            made[dim] = (_index(ctxs[0], rows_of(dim), fwd, attrs), _index(ctxs[1], rows_of(dim), fwd))
        return made[dim]
    yield get
    for pair in made.values():
        for i in pair:
            i.close()


def search_copy(ctx, idx, n, dim, q, qt, qo, filters=None):
    """One search on the copy route: the lists and the launches per tag."""
    ctx.profile_reset(1)
    L = idx.search_lists(q, qt, qo, depth=DEPTH) if filters is None else idx.search_lists(q, qt, qo, depth=DEPTH, filters=filters)
    launches = {t: int(ctx.profile_read(t)[1]) for t in ("cosine", "spec", "rescreen")}
    gate = float(ctx.profile_read("screen_gate")[0])
    ctx.profile_reset(0)
    assert 2 * n * dim <= idx.index_bytes()[1] < 3 * n * dim, "the index holds the bf16 copy (made by the search) and no int8 tier"
    assert launches["rescreen"] == 0 and launches["spec"] == 0, launches
    assert gate == 0.0, "the screen holds on unit rows (the exact pipeline would hide a dropped row)"
    return L, launches


def same_bits(La, Ls):
    assert np.array_equal(La.cos_counts, Ls.cos_counts)
    assert np.array_equal(La.cos_docs, Ls.cos_docs)
    assert np.array_equal(La.cos_scores.view(np.uint32), Ls.cos_scores.view(np.uint32))


def run_case(O, ctxs, ic, istream, dim, n, B, cus, checked):
    q = queries_of(dim)[:B]
    _, qt, qo = _terms(n, B)
    L, launches = search_copy(ctxs[0], ic, n, dim, q, qt, qo)
    p = plan(n, B, DEPTH, cus, spec=False, pf_carry=PF_CARRY)
    assert launches["cosine"] == len(p.chunks), (launches, p.chunks)
    if B > 8:
        same_bits(L, istream.search_lists(q, qt, qo, depth=DEPTH))
    for b in checked:
        check_oracle(L, b, reference(O, dim, n, b), DEPTH, n, 0)
    return L


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 33, 64])
@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("dim", [384, 768])
def test_small_corpus(O, ctxs, num_cus, dim, n, B):
    """A wave's only tile, ragged tiles, waves with no tile at all, count = min(depth, n)."""
    fwd, _, _ = _terms(n, B)
    rows = rows_of(dim)[:n]
    ic, istream = _index(ctxs[0], rows, fwd), (_index(ctxs[1], rows, fwd) if B > 8 else None)
    try:
        L = run_case(O, ctxs, ic, istream, dim, n, B, num_cus, range(B))
        assert (L.cos_counts[:B] == min(DEPTH, n)).all()
    finally:
        ic.close()
        if istream is not None:
            istream.close()


def _checked(B):
    """Of a large case: both sides of every query-tile and group edge, the last query, every 7th."""
    return sorted((set(range(0, B, 7)) | {0, 7, 8, 31, 32, 33, 63, 64, B - 1}) & set(range(B)))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [8, 9, 33, 64, 65])
@pytest.mark.parametrize("dim", [384, 768])
def test_big_corpus(O, ctxs, big, num_cus, dim, B):
    """my_nt = 1 .. 4 (B = 8: more), the dense first chunk and the staged later ones, refills two tiles ahead, the empty descriptor,
    a one-row last tile, both sides of NQT = 1 / 2 and of a 64-query group."""
    ic, istream = big(dim)
    L = run_case(O, ctxs, ic, istream, dim, N_BIG, B, num_cus, _checked(B))
    for b in _checked(B):   # the one-row last tile is somebody's best row or nobody's: never a row past the end
        assert listed(L, b, 0).max() < N_BIG


@pytest.mark.gpu
def test_big_corpus_with_the_speculation_switch_on(O, big, num_cus):
    """d = 768, B = 64 again on a ctx of its own with speculation on: at depth 10 no prediction qualifies, so the schedule, the
    launches and the lists are those of the proven thresholds -- bit for bit the stream screen's."""
    from openintel_amd import _lib
    dim, B = 768, 64
    _, istream = big(dim)
    c = _ctx(_lib.OI_COSINE_SCREEN_COPY, spec=True)
    try:
        fwd, qt, qo = _terms(N_BIG, B)
        ic = _index(c, rows_of(dim), fwd)
        q = queries_of(dim)[:B]
        L, launches = search_copy(c, ic, N_BIG, dim, q, qt, qo)
        assert launches["cosine"] == len(big_plan(B, num_cus, spec=True).chunks)
        same_bits(L, istream.search_lists(q, qt, qo, depth=DEPTH))
        for b in _checked(B):
            check_oracle(L, b, reference(O, dim, N_BIG, b), DEPTH, N_BIG, 0)
        ic.close()
    finally:
        c.close()


@pytest.mark.gpu
def test_big_corpus_filtered(O, ctxs, big, num_cus):
    """cosine_copy_screen<.., FILT = true>: d = 768, B = 64, every query with a group filter that passes about one row in seven.
    The lists are the oracle's full ranking restricted to the passing documents (test_gpu_filter's reference)."""
    from test_gpu_filter import _passes
    dim, B = 768, 64
    ic, _ = big(dim)
    group, stamp = group_of(N_BIG), np.arange(N_BIG, dtype=np.uint32)
    F = np.array([(0xFFFFFFFF, b % 7, 0, 0xFFFFFFFF) for b in range(B)], dtype=np.uint32)
    q = queries_of(dim)[:B]
    _, qt, qo = _terms(N_BIG, B)
    L, launches = search_copy(ctxs[0], ic, N_BIG, dim, q, qt, qo, filters=F)
    assert launches["cosine"] == len(big_plan(B, num_cus).chunks)
    for b in _checked(B):
        ok = _passes(F[b], group, stamp)
        assert 0.13 < ok.mean() < 0.16
        d = listed(L, b, 0)
        assert ok[d].all(), ("a document that fails the filter is listed", b)
        check_oracle(L, b, np.where(ok, reference(O, dim, N_BIG, b), -np.inf), DEPTH, N_BIG, 0)
