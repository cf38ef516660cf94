"""Narrative terms (oi_label_term_counts, oi_label_terms_rank, oi_label_terms): counts[t][c] = the documents of
cluster c that hold term t, sizes[c] = the rows of cluster c, and per cluster the eligible terms in the order excess
descending, counts descending, term ascending, excess = counts[t][c] * A - sizes[c] * dfA[t].

The references are numpy and Python integers in this file, from the test's own forward index: the distinct (term, document)
pairs, the label of every document, Python big-int excess values and `sorted` with the three-part key.  Everything is
compared bit for bit; there is no tolerance anywhere.  Documents have 1 .. 6 tokens (duplicates within a document on purpose),
a few are empty, and no index has embeddings except where a view or oi_label_sums needs them (dim 16)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BLOCK, WINDOW = 32768, 16384
THREADS, SPLIT, SLICE, FAN = 256, 16384, 1024, 64     # label_terms.hip's (tests/test_label_terms_abi.py asserts them)
NONE = 0xFFFFFFFF
COMMON = np.array([3, 17, 64, 255, 256, 1000, 2047, 2048, 3000, 4095], dtype=np.int64)
EVERY, W0, W1, LAST, GAP, TAIL0, N_TAIL, UNUSED = 7, 3500, 3501, 3502, 3503, 3600, 200, 3599


@functools.lru_cache(maxsize=None)
def _ctx():
    import openintel_amd as oi
    return oi.HipContext(0)


def _dtype():
    from openintel_amd import _lib
    return _lib.LABEL_TERM_DTYPE


class _Corpus:
    def __init__(self, n, vocab, docs, terms):
        """(docs[i], terms[i]): token i; any order, duplicates allowed"""
        order = np.argsort(docs, kind="stable")
        self.n, self.vocab = n, vocab
        self.terms = (terms[order] % vocab).astype(np.uint32)
        self.offs = np.zeros(n + 1, np.uint64)
        self.offs[1:] = np.cumsum(np.bincount(docs, minlength=n))
        pairs = np.unique((self.terms.astype(np.int64) << 32) | docs[order])   # a term counts once per document
        self.pair_term, self.pair_doc = pairs >> 32, pairs & 0xFFFFFFFF

    def part(self, lo, hi):
        a, b = int(self.offs[lo]), int(self.offs[hi])
        docs = np.repeat(np.arange(hi - lo), np.diff(self.offs[lo:hi + 1].astype(np.int64)))
        return _Corpus(hi - lo, self.vocab, docs, self.terms[a:b].astype(np.int64))


@functools.lru_cache(maxsize=None)
def _corpus(n, vocab, every=False, seed=0):
    """n documents of 1 .. 6 random tokens over COMMON (every 7th repeats its first token; every 997th is empty), and planted:
    W0 in exactly the documents of window 1 (its run starts at a window and ends at a block boundary), W1 in those of window 2
    (starts at a block, ends at a window boundary), LAST in every 3rd document of the last block only, GAP in every 5th
    document of the even blocks (the odd ones are empty for it), N_TAIL terms with one posting each, UNUSED with none; with
    `every`, EVERY in every document (then no document is empty)."""
    rng = np.random.default_rng(100 * seed + n + vocab)
    d = np.arange(n)
    lens = rng.integers(1, 7, size=n)
    lens[d % 997 == 5] = 0
    docs = np.repeat(d, lens)
    terms = COMMON[rng.integers(0, COMMON.size, size=docs.size)]
    first = np.concatenate([[0], np.cumsum(lens)[:-1]])
    rep = d[(d % 7 == 0) & (lens >= 2)]
    terms[first[rep] + 1] = terms[first[rep]]
    last0 = (n - 1) // BLOCK * BLOCK
    planted = [(d[(d >= WINDOW) & (d < BLOCK)], W0), (d[(d >= BLOCK) & (d < BLOCK + WINDOW)], W1), (d[(d >= last0) & (d % 3 == 0)], LAST),
               (d[((d // BLOCK) % 2 == 0) & (d % 5 == 0)], GAP)]
    planted += [(np.array([(i * 331 + 11) % n]), TAIL0 + i) for i in range(N_TAIL)]
    if every:
        planted.append((d, EVERY))
    docs = np.concatenate([docs] + [p for p, _ in planted])
    terms = np.concatenate([terms] + [np.full(p.size, t, np.int64) for p, t in planted])
    return _Corpus(n, vocab, docs, terms)


def _labels(n, K, seed=0, assigned=0.8):
    """random labels over [0, K) with a share unassigned; the first rows carry K - 1, K, 0xFFFFFFFF, 0 exactly"""
    rng = np.random.default_rng(7000 + seed + n + K)
    lab = rng.integers(0, K, size=n).astype(np.uint32)
    lab[rng.random(n) >= assigned] = NONE
    edge = np.array([K - 1, K, NONE, 0, K + 1], np.uint32)
    lab[:min(n, edge.size)] = edge[:min(n, edge.size)]
    return lab


def _index(corp, finalize=True, rows=None, dim=4):
    import openintel_amd as oi
    idx = oi.HybridIndex(_ctx(), corp.n, dim, corp.vocab)
    if rows is not None:
        idx.set_embeddings(rows, normalize=True)
    idx.set_forward(corp.terms if corp.terms.size else np.zeros(1, np.uint32), corp.offs)
    if finalize:
        idx.finalize()
    return idx


@functools.lru_cache(maxsize=None)
def _built(n, vocab, every=False, seed=0):
    corp = _corpus(n, vocab, every, seed)
    return corp, _index(corp)


def _ref_table(corp, labels, K):
    lab = labels[corp.pair_doc]
    m = lab < K
    counts = np.zeros((corp.vocab, K), np.uint32)
    np.add.at(counts, (corp.pair_term[m], lab[m].astype(np.int64)), 1)
    sizes = np.bincount(labels[labels < K].astype(np.int64), minlength=K).astype(np.uint64)
    return counts, sizes


def _ref_rank(counts, sizes, top, min_df):
    """the definition in Python integers -> (records [K][top], n [K])"""
    K = counts.shape[1]
    A = sum(int(s) for s in sizes)
    dfa = [int(x) for x in counts.astype(np.uint64).sum(axis=1)]
    rec = np.zeros((K, top), _dtype())
    rec["term"] = NONE
    n = np.zeros(K, np.uint32)
    for c in range(K):
        col = counts[:, c]
        cand = [(-(int(col[t]) * A - int(sizes[c]) * dfa[t]), -int(col[t]), int(t)) for t in np.nonzero(col >= max(min_df, 1))[0]]
        cand.sort()
        n[c] = min(top, len(cand))
        for r, (neg_excess, neg_cnt, t) in enumerate(cand[:top]):
            rec[c, r] = (t, -neg_cnt, dfa[t] & 0xFFFFFFFF, 0, -neg_excess)
    return rec, n


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    view = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(view).copy()).to("cuda:0")


def _host_counts(t, sizes):
    return t.cpu().numpy().view(np.uint32), sizes.cpu().numpy().view(np.uint64)


def _host_terms(rec, n, sizes):
    from openintel_amd import retriever
    return retriever.label_term_records(rec), n.cpu().numpy().view(np.uint32), sizes.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------ the table and the lists at every block, vocabulary and cluster edge
CASES = [(1, 97, 2, False), (32767, 4096, 7, False), (32768, 4096, 64, True), (32769, 97, 255, False), (32769, 4096, 1, True),
         (65537, 4096, 256, True), (65537, 4096, 2, False), (65537, 1, 1, False), (65537, 97, 7, True), (32769, 1, 256, False)]


@pytest.mark.parametrize("n,vocab,K,every", CASES)
def test_table_and_lists_match_the_definition_in_both_locations(n, vocab, K, every):
    corp, idx = _built(n, vocab, every)
    lab = _labels(n, K)
    ref_counts, ref_sizes = _ref_table(corp, lab, K)
    if vocab == 4096:
        assert ref_counts[UNUSED % vocab].sum() == 0                           # a term id with no posting
        if every and n > SPLIT:
            assert int(np.count_nonzero(corp.pair_term == EVERY)) == n > SPLIT  # one term in every document: split across tasks
    counts, sizes = idx.label_term_counts(lab, K)
    assert _same(counts, ref_counts) and _same(sizes, ref_sizes)
    d_counts, d_sizes = _host_counts(*idx.label_term_counts(_dev(lab), K))
    assert _same(d_counts, ref_counts) and _same(d_sizes, ref_sizes)
    ref_rec, ref_n = _ref_rank(ref_counts, ref_sizes, 10, 1)
    rec, cnt, sizes2 = idx.label_terms(lab, K)
    assert _same(rec, ref_rec) and _same(cnt, ref_n) and _same(sizes2, ref_sizes)
    d_rec, d_cnt, d_sizes2 = _host_terms(*idx.label_terms(_dev(lab), K))
    assert _same(d_rec, ref_rec) and _same(d_cnt, ref_n) and _same(d_sizes2, ref_sizes)
    again = idx.label_terms(lab, K)                                            # two runs give the same bytes
    assert _same(again[0], rec) and _same(again[1], cnt)


@pytest.mark.parametrize("top,min_df", [(1, 0), (1, 3), (10, 0), (10, 3), (64, 1), (64, 3), (64, 1 << 30)])
def test_top_and_min_df(top, min_df):
    corp, idx = _built(65537, 4096, True)
    K = 7
    lab = _labels(65537, K, seed=3)
    ref_rec, ref_n = _ref_rank(*_ref_table(corp, lab, K), top, min_df)
    rec, cnt, _ = idx.label_terms(lab, K, top=top, min_df=min_df)
    assert _same(rec, ref_rec) and _same(cnt, ref_n)
    if min_df == 1 << 30:                                                      # larger than any count: nothing is eligible
        assert not cnt.any() and (rec["term"] == NONE).all() and not rec["excess"].any() and not rec["df_cluster"].any()
    if (top, min_df) == (64, 1):
        assert (rec["excess"] < 0).any()                                       # lists long enough to reach negative entries


def test_all_rows_unlabelled_and_one_cluster_holding_every_row():
    corp, idx = _built(32769, 4096, True)
    for fill in (NONE, 5):                                                     # 5 == n_clusters: "no cluster" too
        lab = np.full(corp.n, fill, np.uint32)
        counts, sizes = idx.label_term_counts(lab, 5)
        assert not counts.any() and not sizes.any()
        rec, cnt, sizes = idx.label_terms(lab, 5, top=10)
        assert not cnt.any() and (rec["term"] == NONE).all() and not sizes.any()
        assert not rec["excess"].any() and not rec["df_cluster"].any() and not rec["df_assigned"].any() and not rec["reserved"].any()
    lab = np.full(corp.n, 2, np.uint32)                                        # cluster 2 holds every row
    counts, sizes = idx.label_term_counts(lab, 4)
    ref_counts, ref_sizes = _ref_table(corp, lab, 4)
    assert _same(counts, ref_counts) and _same(sizes, ref_sizes) and int(sizes[2]) == corp.n
    rec, cnt, _ = idx.label_terms(lab, 4, top=10)
    ref_rec, ref_n = _ref_rank(ref_counts, ref_sizes, 10, 1)
    assert _same(rec, ref_rec) and _same(cnt, ref_n) and list(cnt) == [0, 0, 10, 0]
    assert not rec["excess"].any() and rec["term"][2, 0] == EVERY              # every excess is 0: the most frequent terms


@pytest.mark.parametrize("postings", [SPLIT - 1, SPLIT, SPLIT + 1])
@pytest.mark.parametrize("lead", [0, 7, SPLIT - 3])
def test_terms_around_the_split_constant(postings, lead):
    """Term 50 with SPLIT - 1, SPLIT or SPLIT + 1 postings, behind `lead` postings of light terms (so that it starts at a
    cut, just behind one, or just before the next) and in front of light terms with one posting each."""
    n = SPLIT + 40
    d = np.arange(n)
    per = max(lead // 3, 1)
    parts = [(d[:postings], 50)]
    parts += [(d[i * per:min((i + 1) * per, lead)] if i < 2 else d[2 * per:lead], 10 + i) for i in range(3) if lead]
    parts += [(np.array([(i * 37) % n]), 60 + i) for i in range(70)]
    docs = np.concatenate([p for p, _ in parts])
    terms = np.concatenate([np.full(p.size, t, np.int64) for p, t in parts])
    corp = _Corpus(n, 200, docs, terms)
    assert int(np.count_nonzero(corp.pair_term == 50)) == postings and int(np.count_nonzero(corp.pair_term < 50)) == lead
    idx = _index(corp)
    for K in (3, 256):
        lab = _labels(n, K, seed=postings + lead)
        ref_counts, ref_sizes = _ref_table(corp, lab, K)
        counts, sizes = idx.label_term_counts(lab, K)
        assert _same(counts, ref_counts) and _same(sizes, ref_sizes)
    idx.close()


# ------------------------------------------------------------------ contracts
def test_all_labels_zero_give_the_local_df():
    corp, idx = _built(65537, 4096, True)
    counts, sizes = idx.label_term_counts(np.zeros(corp.n, np.uint32), 1)
    _, df = idx.local_stats()
    assert _same(counts[:, 0], df) and int(sizes[0]) == corp.n


def test_sizes_equal_label_sums_counts_and_a_view_gives_the_same_bytes():
    import openintel_amd as oi
    corp = _corpus(32769, 4096, True)
    rows = np.random.default_rng(5).standard_normal((corp.n, 16)).astype(np.float32)
    idx = _index(corp, rows=rows, dim=16)
    K = 9
    lab = _labels(corp.n, K, seed=1)
    counts, sizes = idx.label_term_counts(lab, K)
    _, ls_counts = idx.label_sums(lab, K)
    assert _same(sizes, ls_counts)
    rec, cnt, _ = idx.label_terms(lab, K, top=12, min_df=2)
    ctx2 = oi.HipContext(0)
    view = idx.view(ctx2)
    v_counts, v_sizes = view.label_term_counts(lab, K)
    v_rec, v_cnt, _ = view.label_terms(lab, K, top=12, min_df=2)
    assert _same(v_counts, counts) and _same(v_sizes, sizes) and _same(v_rec, rec) and _same(v_cnt, cnt)
    view.close()
    idx.close()


def test_tables_of_two_halves_add_and_rank_of_the_sum_is_the_whole():
    from openintel_amd import retriever
    corp, idx = _built(65537, 4096, True)
    K, h = 6, 30001
    lab = _labels(corp.n, K, seed=2)
    whole_counts, whole_sizes = idx.label_term_counts(lab, K)
    a, b = _index(corp.part(0, h)), _index(corp.part(h, corp.n))
    ca, sa = a.label_term_counts(lab[:h], K)
    cb, sb = b.label_term_counts(lab[h:], K)
    assert _same(ca + cb, whole_counts) and _same(sa + sb, whole_sizes)
    rec, cnt, _ = idx.label_terms(lab, K, top=16, min_df=2)
    r_rec, r_cnt = retriever.rank_label_terms(_ctx(), ca + cb, sa + sb, top=16, min_df=2)
    assert _same(r_rec, rec) and _same(r_cnt, cnt)
    d_rec, d_cnt = retriever.rank_label_terms(_ctx(), _dev(ca + cb), sa + sb, top=16, min_df=2)
    assert _same(retriever.label_term_records(d_rec), rec) and _same(d_cnt.cpu().numpy().view(np.uint32), cnt)
    a.close()
    b.close()


# ------------------------------------------------------------------ the ranked cut on planted tables
def _rank(counts, sizes, top, min_df):
    from openintel_amd import retriever
    return retriever.rank_label_terms(_ctx(), counts, np.asarray(sizes, np.uint64), top=top, min_df=min_df)


def _check_rank(counts, sizes, top, min_df):
    ref_rec, ref_n = _ref_rank(counts, np.asarray(sizes, np.uint64), top, min_df)
    rec, n = _rank(counts, sizes, top, min_df)
    assert _same(rec, ref_rec) and _same(n, ref_n)
    return rec, n


def test_ties_on_excess_and_on_count():
    counts = np.zeros((2 * SLICE + 52, 2), np.uint32)
    sizes = [10, 10]                                                           # A = 20: excess(0, t) = 20 c0 - 10 (c0 + c1)
    counts[5] = (5, 1)                                                         # 40
    counts[SLICE + 1] = (6, 2)                                                 # 40, the larger count: first
    counts[9] = (5, 1)                                                         # 40, count 5, the larger id: behind term 5
    counts[2 * SLICE + 51] = (5, 1)                                            # ... and the last term of the last slice behind both
    counts[700] = (9, 1)                                                       # 80
    counts[3] = (1, 9)                                                         # -80 for cluster 0, +80 for cluster 1
    rec, n = _check_rank(counts, sizes, 10, 1)
    assert list(rec["term"][0, :6]) == [700, SLICE + 1, 5, 9, 2 * SLICE + 51, 3] and list(n) == [6, 6]
    assert list(rec["excess"][0, :6]) == [80, 40, 40, 40, 40, -80]
    _check_rank(counts, sizes, 3, 1)                                           # the cut falls inside the tie
    _check_rank(counts, sizes, 4, 5)
    _check_rank(counts, sizes, 1, 0)


@pytest.mark.parametrize("where", ["last", "two", "many"])
def test_eligible_terms_by_slice(where):
    rng = np.random.default_rng(11)
    vocab = {"last": 3 * SLICE + 5, "two": 3 * SLICE + 5, "many": FAN * SLICE + 3 * SLICE + 1}[where]   # "many": two merge rounds
    K = 3
    counts = np.zeros((vocab, K), np.uint32)
    if where == "last":
        t = np.arange(3 * SLICE, vocab)
    elif where == "two":
        t = np.concatenate([np.arange(SLICE - 40, SLICE), np.arange(3 * SLICE, vocab)])
    else:
        t = rng.choice(vocab, size=5000, replace=False)
        t[:3] = (0, vocab - 1, FAN * SLICE)
    counts[t] = rng.integers(0, 6, size=(t.size, K))
    sizes = [50, 60, 70]
    for top, min_df in ((64, 1), (10, 3), (64, 5)):                            # (64, 5): fewer eligible terms than top where == "last"
        _check_rank(counts, sizes, top, min_df)


def test_assigned_rows_at_the_limit_do_not_overflow():
    A = (1 << 31) - 1
    sizes = [A - 1000, 1000]
    counts = np.zeros((SLICE + 9, 2), np.uint32)
    counts[0] = (A - 1000, 1000)                                               # in every assigned post: excess 0
    counts[1] = (A - 1000, 0)                                                  # the whole of cluster 0 and nothing else: the largest products
    counts[2] = (0, 1000)
    counts[SLICE + 8] = (1, 999)
    counts[77] = (12345678, 3)
    rec, n = _check_rank(counts, sizes, 10, 1)
    assert int(rec["excess"][0, 0]) == (A - 1000) * A - (A - 1000) * (A - 1000) and rec["term"][0, 0] == 1
    assert int(rec["excess"][1, 0]) == 1000 * A - 1000 * 1000 and rec["term"][1, 0] == 2
    _check_rank(counts, sizes, 64, 0)


def test_rank_edges_of_vocabulary_and_clusters():
    rng = np.random.default_rng(12)
    for vocab, K in ((1, 1), (1, 256), (97, 255), (SLICE, 64), (SLICE + 1, 65)):
        counts = rng.integers(0, 4, size=(vocab, K)).astype(np.uint32)
        sizes = rng.integers(3, 50, size=K)
        for top, min_df in ((1, 1), (10, 0), (64, 3)):
            _check_rank(counts, sizes, top, min_df)


# ------------------------------------------------------------------ batch.describe_narratives
def test_describe_narratives_names_the_planted_words():
    import openintel_amd as oi
    from openintel_amd import batch
    planted = ["squeeze", "earnings", "dividend"]
    filler = ["the", "stock", "today", "market", "moves", "again"]
    rng = np.random.default_rng(21)
    texts, lab = [], []
    for i in range(300):
        c = i % 3
        words = [filler[j] for j in rng.integers(0, len(filler), size=4)] + [planted[c]] + ([planted[c]] if i % 5 == 0 else [])
        texts.append(" ".join(words).upper() if i % 11 == 0 else " ".join(words))
        lab.append(c)
    lab = np.array(lab, np.uint32)
    idx = oi.HybridIndex(_ctx(), len(texts), 4, 1 << 16)
    idx.set_text(texts)
    idx.set_signals(np.zeros(len(texts)), np.zeros(len(texts), np.uint8), np.zeros(len(texts), np.uint8))
    idx.finalize()
    out = batch.describe_narratives(idx, lab, n_clusters=3, top=5, texts=texts[:90])
    assert len(out) == 3
    for c in range(3):
        first = out[c][0]
        assert first.word == planted[c] and first.df == 100 and first.df_assigned == 100 and first.lift == (100 / 100) / (100 / 300)
        ids, offs = np.array([t.term for t in out[c]], np.uint32), np.arange(len(out[c]) + 1, dtype=np.uint32)
        totals = idx.mention_summary(ids, offs)["total"][:, 0]                 # every returned id as a one-term query: all posts are assigned
        assert [int(x) for x in totals] == [t.df_assigned for t in out[c]]
    no_words = batch.describe_narratives(idx, lab, n_clusters=3, top=5)
    assert all(t.word is None for terms in no_words for t in terms)
    assert [[t.term for t in terms] for terms in no_words] == [[t.term for t in terms] for terms in out]
    idx.close()


# ------------------------------------------------------------------ state errors
def test_an_unfinalized_index_is_a_state_error_and_the_ctx_stays_usable():
    from openintel_amd import _lib
    corp = _corpus(32767, 4096)
    idx = _index(corp, finalize=False)
    lab = _labels(corp.n, 4)
    for call in (lambda: idx.label_term_counts(lab, 4), lambda: idx.label_terms(lab, 4)):
        with pytest.raises(_lib.OiError) as e:
            call()
        assert e.value.code == _lib.OI_ERR_STATE and "not finalized" in e.value.message
    idx.finalize()
    ref_counts, ref_sizes = _ref_table(corp, lab, 4)
    counts, sizes = idx.label_term_counts(lab, 4)
    assert _same(counts, ref_counts) and _same(sizes, ref_sizes)
    idx.close()


def test_host_location_without_sizes_out_is_the_device_location_bit_for_bit():
    """300 documents, vocab 50, 3 clusters: OI_HOST gives OI_DEVICE's bytes, and with sizes_out NULL the records and n are as
    they were."""
    import ctypes as C
    from openintel_amd import _lib
    n, vocab, K, top = 300, 50, 3, 10
    corp, idx = _built(n, vocab)
    lab = _labels(n, K, seed=9)
    rec, cnt, sizes = idx.label_terms(lab, K, top=top)
    d_rec, d_cnt, d_sizes = _host_terms(*idx.label_terms(_dev(lab), K, top=top))
    ref_counts, ref_sizes = _ref_table(corp, lab, K)
    ref_rec, ref_n = _ref_rank(ref_counts, ref_sizes, top, 1)
    assert _same(rec, ref_rec) and _same(cnt, ref_n) and _same(sizes, ref_sizes) and int(cnt.sum()) > 0
    assert _same(d_rec, rec) and _same(d_cnt, cnt) and _same(d_sizes, sizes)
    spec = _lib.LabelTermsSpec(top, 1, (C.c_uint32 * 2)(0, 0))
    rec2, cnt2 = np.zeros((K, top), _dtype()), np.zeros(K, np.uint32)
    _lib.check(idx.lib.oi_label_terms(idx.handle, _lib.ptr(lab), K, C.byref(spec), _lib.OI_HOST, _lib.ptr(rec2), _lib.ptr(cnt2), None))
    assert _same(rec2, rec) and _same(cnt2, cnt)
