"""GPU tokeniser (csrc/text_terms.hip) against the Python restatement of its contract (tests/test_text_terms_abi.py):
oi_text_terms / oi_query_terms / oi_index_set_text.  Every comparison is exact: the outputs are integers."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from test_text_terms_abi import ref_text_terms, term_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KSIGN, IDOT = "\u212a", "\u0130"          # E2 84 AA -> 'k' (joins);  C4 B0 -> 'i' + separator
LOOKALIKES = "\u00aa\u00b0\u20aa\u00c4"   # C2 AA, C2 B0, E2 82 AA, C3 84: bytes of the two mappings without being them


@pytest.fixture(scope="module")
def ctx():
    import openintel_amd as oi
    c = oi.HipContext(0)
    yield c
    c.close()


def _edges():
    """the kernel's own constants: bytes per lane window and per workgroup tile (one launch covers every tile)"""
    import re
    src = open(os.path.join(ROOT, "openintel_amd", "csrc", "text_terms.hip")).read()
    lane, tile = (int(re.search(r"^#define\s+" + name + r"\s+(\d+)u\b", src, flags=re.M).group(1)) for name in ("TT_LANE", "TT_TILE"))
    assert 0 < lane < tile
    return lane, tile


def _dev(blob, offs, off_dtype=np.uint64, skew=0):
    """the packed texts as torch CUDA tensors; skew > 0: the blob starts `skew` bytes into a 16-byte-aligned buffer"""
    import torch
    dev = torch.device("cuda:0")
    buf = torch.zeros(skew + max(blob.size, 1), dtype=torch.uint8, device=dev)
    buf[skew:skew + blob.size] = torch.from_numpy(np.ascontiguousarray(blob)).to(dev)
    signed = np.int64 if off_dtype is np.uint64 else np.int32
    return buf[skew:skew + blob.size], torch.from_numpy(offs.astype(off_dtype).view(signed)).to(dev)


def _check(ctx, texts, vocab, skews=(0,), what=""):
    """host and device locations, count-only == full offsets, all equal to the restatement"""
    import openintel_amd as oi
    want_ids, want_offs = ref_text_terms(texts, vocab)
    ids, offs = oi.text_terms(ctx, texts, vocab)
    assert ids.dtype == np.uint32 and offs.dtype == np.uint64
    assert np.array_equal(offs, want_offs), (what, "host offsets")
    assert np.array_equal(ids, want_ids), (what, "host ids")
    total, offs_c = oi.text_terms(ctx, texts, vocab, count_only=True)
    assert total == want_ids.size and np.array_equal(offs_c, want_offs), (what, "host count-only")
    blob, boffs = oi.pack_posts(texts)
    for skew in skews:
        d_blob, d_offs = _dev(blob, boffs, skew=skew)
        d_ids, d_to = oi.text_terms(ctx, (d_blob, d_offs), vocab)
        assert np.array_equal(d_to.cpu().numpy().view(np.uint64), want_offs), (what, skew, "device offsets")
        assert np.array_equal(d_ids.cpu().numpy().view(np.uint32), want_ids), (what, skew, "device ids")
        total, d_tc = oi.text_terms(ctx, (d_blob, d_offs), vocab, count_only=True)
        assert total == want_ids.size and np.array_equal(d_tc.cpu().numpy().view(np.uint64), want_offs), (what, skew, "device count-only")
    return want_ids, want_offs


# ---------------------------------------------------------------- 3. oi_text_terms == restatement
def test_fixture_posts_and_fixed_vectors(ctx, golden):
    texts = [p["text"] for p in golden["fixture_posts"]]
    assert len(texts) == 10
    _check(ctx, texts, 131072, skews=(0, 1, 15))
    ids, offs = _check(ctx, ["a", "moon", "x" * 64, "x" * 65, "x" * 64 + "y"], 131072)
    assert ids.tolist() == [66885, 24944, 54459, 54459, 54459] and offs.tolist() == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("vocab", [1000, 131072, 3_000_000, (1 << 32) - 1])
def test_synthetic_posts_at_four_vocab_sizes(ctx, vocab):
    from openintel_amd import synth
    ids, _ = _check(ctx, synth.posts_np(20000), vocab, skews=(0, 7))
    assert int(ids.max()) < vocab


def test_degenerate_batches(ctx):
    import openintel_amd as oi
    V = 131072
    _check(ctx, [], V, what="n = 0")
    _check(ctx, [""], V, what="n = 1, empty blob")
    _check(ctx, ["moon"], V, what="n = 1")
    _check(ctx, ["", "", ""], V, what="empty blob")
    _check(ctx, ["", "abc", "", "", "def", ""], V, what="empty posts")
    _check(ctx, [" ,.;", "\t\n", "--", "\u00e9\u00e9", "abc"], V, what="separators only")
    _check(ctx, ["first"] + [""] * 10000 + ["last one"] + [""] * 10000, V, what="10 000 consecutive empty posts")
    _check(ctx, ["abc", "def"], V, what="adjacent posts cut a token")
    _check(ctx, ["MiXeD CaSe 0dTe", "mixed case 0DTE"], V, what="mixed case")
    _check(ctx, ["hello wor", "ld", "x" * 13 + " tail-tok"], V, skews=(0, 3), what="blob not a multiple of 16, ends mid-token")
    # n = 0 with nothing at all: the one offset is zero
    total, offs = oi.text_terms(ctx, (np.zeros(0, np.uint8), np.zeros(1, np.uint64)), V, count_only=True)
    assert total == 0 and offs.tolist() == [0]


@pytest.mark.parametrize("length", [1, 63, 64, 65, 100_000])
def test_one_token_of_n_bytes(ctx, length):
    ids, offs = _check(ctx, ["q" * length], 131072, skews=(0, 9))
    assert offs.tolist() == [0, 1] and ids[0] == term_of("q" * min(length, 64), 131072)
    _check(ctx, ["ab " + "Q" * length + " cd", "q" * length, "z"], 131072)


def test_long_tokens_of_mapped_code_points_across_the_tile_edge(ctx):
    """64 hashed bytes are up to 192 raw bytes: the halo behind a tile must hold them wherever the token starts"""
    lane, tile = _edges()
    V = 131072
    for back in (1, 2, 3, 15, 16, 17, lane - 1, lane, lane + 1, 189, 190, 191, 192, 193, 194, 250):
        for n_k in (63, 64, 65, 70):
            t = " " * (tile - back) + KSIGN * n_k + " z"
            ids, _ = _check(ctx, [t], V, what=(back, n_k))
            assert ids[0] == term_of("k" * min(n_k, 64), V)
        _check(ctx, [" " * (tile - back) + "a" + KSIGN * 62 + IDOT + "b"], V, what=(back, "k...i|b"))


def _edge_unit():
    """posts whose boundaries, token starts, token ends, U+212A and U+0130 each sit at a fixed byte of an ODD-length unit:
    repeated, every one of them visits every residue of every power-of-two edge"""
    unit = ["abc", "def", "x" + KSIGN + "y", KSIGN, IDOT + "stanbul a" + IDOT + "b", "9 Zq-", "",
            "a\u00aab\u00b0c\u20aad\u00c4e", KSIGN + KSIGN + " " + IDOT + IDOT, "k" + IDOT, "tail"]
    if sum(len(p.encode()) for p in unit) % 2 == 0:
        unit.append("_")
    return unit


def test_every_case_at_every_offset_across_lane_and_tile_edges(ctx):
    lane, tile = _edges()
    unit = _edge_unit()
    L = sum(len(p.encode()) for p in unit)
    assert L % 2 == 1 and tile % lane == 0 and tile & (tile - 1) == 0
    # gcd(L, tile) = 1: over 2 * tile repetitions each byte of the unit is placed at every offset modulo the tile (and so
    # modulo the lane window) twice -- two tiles' worth of offsets for each case, in one blob spanning 2 L tiles
    texts = unit * (2 * tile)
    _check(ctx, texts, 131072, skews=(0, 5), what="edge unit")
    # the same bytes as ONE post and as one post per unit: the post boundary moves, the tokens inside do not
    _check(ctx, ["".join(unit)] * 3000 + ["".join(unit * 3000)], 1000, what="edge unit, long posts")


def test_lookalikes_and_the_golden_lowercase_table(ctx):
    entries = json.load(open(os.path.join(ROOT, "tests", "golden", "unicode_lower_ascii.json")))["entries"]
    mapped = [bytes(e["utf8"]).decode("utf-8") for e in entries]
    assert sorted(mapped) == sorted([KSIGN, IDOT])
    for e in entries:  # the table is the lowercase Python applies, so the restatement and the table agree
        assert [ord(c) for c in bytes(e["utf8"]).decode("utf-8").lower()] == e["lower"]
    texts = []
    for ch in mapped + list(LOOKALIKES):
        texts += ["ab" + ch + "cd", ch + "cd", "ab" + ch, ch, "ab" + ch + ch + "cd", "AB " + ch + " CD"]
    for a in mapped + list(LOOKALIKES):
        for b in mapped + list(LOOKALIKES):
            texts.append("p" + a + b + "q")
    _check(ctx, texts, 131072, skews=(0, 1, 2, 3))
    ids, _ = _check(ctx, ["ab" + KSIGN + "cd", "ab" + IDOT + "cd", "ab\u20aacd"], 131072)
    assert ids.tolist() == [term_of(t, 131072) for t in ("abkcd", "abi", "cd", "ab", "cd")]


# ---------------------------------------------------------------- 4. capacity
def test_capacity_one_short_is_overflow_and_the_ctx_stays_usable(ctx):
    import torch
    import openintel_amd as oi
    from openintel_amd import _lib, synth
    texts = synth.posts_np(300)
    want_ids, want_offs = ref_text_terms(texts, 4096)
    blob, offs = oi.pack_posts(texts)
    total = C.c_uint64()
    for loc, (b, o) in ((_lib.OI_HOST, (blob, offs)), (_lib.OI_DEVICE, _dev(blob, offs))):
        dev = loc == _lib.OI_DEVICE
        cap = want_ids.size - 1
        ids = torch.full((want_ids.size,), -1, dtype=torch.int32, device="cuda:0") if dev else np.full(want_ids.size, 0xFFFFFFFF, np.uint32)
        to = torch.zeros(len(texts) + 1, dtype=torch.int64, device="cuda:0") if dev else np.zeros(len(texts) + 1, np.uint64)
        rc = ctx.lib.oi_text_terms(ctx.handle, _lib.ptr(b), _lib.ptr(o), len(texts), blob.size, 4096, loc, _lib.ptr(ids), cap,
                                   _lib.ptr(to), C.byref(total))
        assert rc == _lib.OI_ERR_OVERFLOW and b"term_capacity" in ctx.lib.oi_last_error()
        assert total.value == want_ids.size
        ctx.synchronize()
        last = ids.cpu().numpy().view(np.uint32)[-1] if dev else ids[-1]
        assert last == 0xFFFFFFFF  # nothing written past the capacity
        rc = ctx.lib.oi_text_terms(ctx.handle, _lib.ptr(b), _lib.ptr(o), len(texts), blob.size, 4096, loc, _lib.ptr(ids), cap + 1,
                                   _lib.ptr(to), None)
        assert rc == 0
        ctx.synchronize()
        got = ids.cpu().numpy().view(np.uint32) if dev else ids
        assert np.array_equal(got, want_ids)
    _check(ctx, texts, 4096)


def test_a_corpus_sized_host_call_gives_its_staging_back():
    """OI_HOST staging lives in the ctx's workspace only while it is query-sized (<= 16 MiB per buffer)"""
    import openintel_amd as oi
    c = oi.HipContext(0)
    n_tok = 8_000_000
    blob = np.tile(np.frombuffer(b"ab ", dtype=np.uint8), n_tok)            # 24 MB of text, one post
    offs = np.array([0, blob.size], dtype=np.uint64)
    ids, toffs = oi.text_terms(c, (blob, offs), 4096)
    assert ids.size == n_tok and toffs.tolist() == [0, n_tok] and bool((ids == term_of("ab", 4096)).all())
    held_large = c.workspace_bytes()[0]
    oi.text_terms(c, ["a small one"], 4096)
    assert held_large < (1 << 20), held_large                                # tile counts and bases only
    assert c.workspace_bytes()[0] < (1 << 20)
    c.close()


# ---------------------------------------------------------------- 5. queries
def test_query_terms_with_u32_offsets(ctx):
    import openintel_amd as oi
    from openintel_amd import synth
    words, _ = synth.word_list()
    rng = np.random.default_rng(5)
    long_q = " ".join(words[i] for i in rng.integers(0, len(words), 300))
    texts = ["AAPL to the moon", "", long_q, "puts PUTS puts", KSIGN + "elvin " + IDOT + "x", "0dte"]
    V = 50_000
    want_ids, want_offs = ref_text_terms(texts, V, np.uint32)
    assert want_offs[3] - want_offs[2] == 300 and want_offs[2] == want_offs[1]
    idx = oi.HybridIndex(ctx, 4, 8, V)
    qt, qo = idx.query_terms(texts)
    assert qt.dtype == np.uint32 and qo.dtype == np.uint32
    assert np.array_equal(qt, want_ids) and np.array_equal(qo, want_offs)
    blob, offs = oi.pack_posts(texts)
    d_qt, d_qo = idx.query_terms(_dev(blob, offs, np.uint32, skew=4))
    assert np.array_equal(d_qt.cpu().numpy().view(np.uint32), want_ids)
    assert np.array_equal(d_qo.cpu().numpy().view(np.uint32), want_offs)
    e_qt, e_qo = idx.query_terms([""])
    assert e_qt.size == 0 and e_qo.tolist() == [0, 0]
    idx.close()


# ---------------------------------------------------------------- 6. - 8. the index built from text
N_IDX, DIM, VOCAB, B, DEPTH, K = 50_000, 384, 131072, 12, 100, 20


@pytest.fixture(scope="module")
def built(ctx):
    import openintel_amd as oi
    from openintel_amd import synth
    texts = synth.posts_np(N_IDX)
    texts[17] = ""                      # a document without tokens
    texts[18] = "Kelvin " + KSIGN + "elvin " + IDOT + "stanbul"
    rows = synth.embeddings_np(N_IDX, DIM)
    terms, offs = ref_text_terms(texts, VOCAB)
    rng = np.random.default_rng(11)
    group = rng.integers(0, 8, size=N_IDX).astype(np.uint32)
    stamp = rng.permutation(N_IDX).astype(np.uint32)
    A = oi.HybridIndex(ctx, N_IDX, DIM, VOCAB)
    A.set_embeddings(rows, normalize=False)
    A.set_text(texts)
    Bx = oi.HybridIndex(ctx, N_IDX, DIM, VOCAB)
    Bx.set_embeddings(rows, normalize=False)
    Bx.set_forward(terms, offs)
    stats = {}
    for name, ix in (("A", A), ("B", Bx)):
        ix.set_doc_attrs(group, stamp)
        stats[name] = ix.local_stats()   # as staged, before finalize
        ix.finalize()                    # here, so that every test below can search whichever runs first
    words, _ = synth.word_list()
    q_texts = [" ".join(words[i] for i in rng.integers(0, len(words), 4)) for _ in range(B - 2)] + ["moon MOON calls", "kelvin"]
    q = synth.embeddings_np(B, DIM, seed=synth.SEED_QUERY)
    yield dict(A=A, B=Bx, stats=stats, texts=texts, rows=rows, terms=terms, offs=offs, q=q, q_texts=q_texts, group=group, stamp=stamp)
    A.close()
    Bx.close()


def _same_lists(x, y):
    return all(np.array_equal(np.asarray(getattr(x, f)).view(np.uint32), np.asarray(getattr(y, f)).view(np.uint32))
               for f in ("cos_scores", "cos_docs", "cos_counts", "bm25_scores", "bm25_docs", "bm25_counts"))


def _same_result(x, y):
    return all(np.array_equal(np.asarray(getattr(x, f)).view(np.uint32), np.asarray(getattr(y, f)).view(np.uint32))
               for f in ("scores", "docs", "counts"))


def test_set_text_equals_text_terms_plus_set_forward(ctx, built):
    from oracle import lib as O
    A, Bx = built["A"], built["B"]
    (ta, dfa), (tb, dfb) = built["stats"]["A"], built["stats"]["B"]
    assert ta == tb == built["terms"].size and np.array_equal(dfa, dfb)
    q = built["q"]
    qt, qo = A.query_terms(built["q_texts"])
    want_qt, want_qo = ref_text_terms(built["q_texts"], VOCAB, np.uint32)
    assert np.array_equal(qt, want_qt) and np.array_equal(qo, want_qo)
    F = np.array([[0, 0, 0, 0xFFFFFFFF], [7, 3, 0, 0xFFFFFFFF], [0, 0, 1000, 30000]] * (B // 3), dtype=np.uint32)
    for mode in (1, 2, 3, 4):  # the four BM25 kernels (oi_index_set_bm25_mode)
        A.set_bm25_mode(mode)
        Bx.set_bm25_mode(mode)
        La, Lb = A.search_lists(q, qt, qo, depth=DEPTH), Bx.search_lists(q, qt, qo, depth=DEPTH)
        assert _same_lists(La, Lb), mode
        assert _same_result(A.search(q, qt, qo, k=K, depth=DEPTH), Bx.search(q, qt, qo, k=K, depth=DEPTH)), mode
        assert _same_result(A.search(q, qt, qo, k=K, depth=DEPTH, filters=F), Bx.search(q, qt, qo, k=K, depth=DEPTH, filters=F)), mode
        for b in range(B):  # and the list is the oracle's on the restatement's ids
            bs, bd = O.topk(O.bm25_scores(built["terms"], built["offs"], VOCAB, want_qt[want_qo[b]:want_qo[b + 1]]), DEPTH, True)
            assert int(La.bm25_counts[b]) == bd.size, (mode, b)
            assert np.array_equal(La.bm25_docs[b][:bd.size], bd) and np.array_equal(La.bm25_scores[b][:bd.size].view(np.uint32), bs.view(np.uint32)), (mode, b)
    A.set_bm25_mode(0)
    Bx.set_bm25_mode(0)
    # search_text == search: host strings, and a device blob with device vectors
    import torch
    import openintel_amd as oi
    want = Bx.search(q, qt, qo, k=K, depth=DEPTH)
    assert _same_result(A.search_text(q, built["q_texts"], k=K, depth=DEPTH), want)
    assert _same_result(A.search_text(q, built["q_texts"], k=K, depth=DEPTH, filters=F), Bx.search(q, qt, qo, k=K, depth=DEPTH, filters=F))
    blob, offs = oi.pack_posts(built["q_texts"])
    got = A.search_text(torch.from_numpy(q).to("cuda:0"), _dev(blob, offs, np.uint32), k=K, depth=DEPTH)
    ctx.synchronize()
    assert _same_result(SimpleResult(got), want)
    # a device blob builds the same index
    import openintel_amd as oi
    D = oi.HybridIndex(ctx, N_IDX, DIM, VOCAB)
    D.set_embeddings(built["rows"], normalize=False)
    D.set_text(_dev(*oi.pack_posts(built["texts"]), skew=8))
    td, dfd = D.local_stats()
    assert td == ta and np.array_equal(dfd, dfa)
    D.finalize()
    assert _same_lists(D.search_lists(q, qt, qo, depth=DEPTH), Lb)
    D.close()


class SimpleResult:
    def __init__(self, r):
        self.scores, self.docs, self.counts = (x.cpu().numpy() for x in (r.scores, r.docs, r.counts))


def test_two_shards_need_no_shared_dictionary(ctx, built):
    import openintel_amd as oi
    A = built["A"]
    q = built["q"]
    qt, qo = A.query_terms(built["q_texts"])
    want = A.search(q, qt, qo, k=K, depth=DEPTH)
    h = N_IDX // 2 + 77
    shards = []
    for lo, hi in ((0, h), (h, N_IDX)):
        s = oi.HybridIndex(ctx, hi - lo, DIM, VOCAB, doc_id_base=lo)
        s.set_embeddings(built["rows"][lo:hi], normalize=False)
        s.set_text(built["texts"][lo:hi])          # each shard on its own: no ids, no dictionary exchanged
        shards.append(s)
    stats = [s.local_stats() for s in shards]
    tot, df = sum(t for t, _ in stats), stats[0][1] + stats[1][1]
    assert (tot, df.tolist()) == (built["stats"]["A"][0], built["stats"]["A"][1].tolist())
    for s in shards:
        s.finalize(N_IDX, tot, df)
    packed = [s.search_lists_packed(q, *s.query_terms(built["q_texts"]), depth=DEPTH) for s in shards]
    fused = oi.fuse_packed(ctx, np.concatenate(packed), 2, B, DEPTH, K)
    assert _same_result(fused, want)
    for s in shards:
        s.close()


def test_view_is_read_only_and_a_pipeline_serves_the_text_index(ctx, built):
    import openintel_amd as oi
    from openintel_amd import _lib
    A, Bx = built["A"], built["B"]
    ctx2 = oi.HipContext(0)
    v = A.view(ctx2)
    with pytest.raises(_lib.OiError) as e:
        v.set_text(built["texts"])
    assert e.value.code == _lib.OI_ERR_STATE
    v.close()
    ctx2.close()
    q = built["q"]
    qt, qo = A.query_terms(built["q_texts"])
    want = Bx.search(q, qt, qo, k=K, depth=DEPTH)
    pipe = oi.NativePipeline(A, lanes=2, max_queries=B, max_query_terms=8, depth=DEPTH, k=K)
    sub = [pipe.submit(q, qt, qo) for _ in range(3)]
    pipe.drain()
    for _, out in sub:
        assert _same_result(out, want)
    pipe.close()


# ---------------------------------------------------------------- 9. full size
def test_ten_million_posts(ctx):
    import torch
    import openintel_amd as oi
    from openintel_amd import synth
    n, V = 10_000_000, 131072
    dev = torch.device("cuda:0")
    blob, offs = synth.posts_torch(n, dev)
    torch.cuda.synchronize()
    ids, toffs = oi.text_terms(ctx, (blob, offs), V)
    ctx.synchronize()
    # token starts of an ASCII corpus: an alnum byte after a non-alnum byte or at a post start
    assert int(blob.max()) < 0x80
    al = ((blob >= 48) & (blob <= 57)) | ((blob >= 65) & (blob <= 90)) | ((blob >= 97) & (blob <= 122))
    prev_ok = torch.ones_like(al)
    prev_ok[1:] = ~al[:-1]
    starts_at = offs[:-1][offs[:-1] < blob.numel()]
    prev_ok[starts_at] = True
    n_starts = int((al & prev_ok).sum())
    del al, prev_ok
    assert ids.numel() == n_starts
    assert int(toffs[0]) == 0 and int(toffs[-1]) == n_starts and bool((toffs[1:] >= toffs[:-1]).all())
    assert int(ids.view(torch.int32).min()) >= 0 and int(ids.max()) < V
    # 2 000 posts across the whole range, first and last included
    rng = np.random.default_rng(3)
    sample = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, 1998)]))
    h_offs = offs.cpu().numpy()
    h_toffs = toffs.cpu().numpy()
    for i in sample:
        text = bytes(blob[h_offs[i]:h_offs[i + 1]].cpu().numpy()).decode("ascii")
        want, _ = ref_text_terms([text], V)
        got = ids[h_toffs[i]:h_toffs[i + 1]].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want), i
    # a pure function of the input: a second run gives the same bytes
    ids2, toffs2 = oi.text_terms(ctx, (blob, offs), V)
    ctx.synchronize()
    assert torch.equal(ids, ids2) and torch.equal(toffs, toffs2)
