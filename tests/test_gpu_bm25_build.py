"""The BM25 index BUILD (csrc/bm25.hip: oi_bm25_stage_forward + oi_bm25_finalize -- bm_make_keys_kernel, bm_count_kernel,
bm_df_kernel, bm_impact_kernel, bm_term_floor_kernel around a radix sort, a run-length encode and a scan) bit for bit at every
wave, cell and floor edge.

The search tests see the index through the lists of the terms they query.  Here the whole index is read back
(HybridIndex.bm25_index, an internal export) and every array -- postings, cell_start, idf, impact floors, doc_len -- is
compared for equality with a plain numpy build of the same corpus, np_build below.  All outputs are integers or f32 bit
patterns: there is no tolerance anywhere.  A floor that is too LOW, a row of floors left at zero or a wrong bound of a cell
nobody queries changes no search result; it changes these arrays.

The reference is pinned first, without a GPU: np_impact equals the oracle's oio_bm25_doc_norm / oio_bm25_impact over a grid, and
the scores summed from np_build's postings equal oracle.lib.bm25_scores.  Two mirrors of kernel geometry (fold_trace:
bm_count_kernel's ballot fold of a wave's runs; floor_trace: bm_floor_find's lanes of 32 bins) are used only to ASSERT that a
case reaches the edge it is there for; what the arrays must be is np_build's alone (np.unique, np.sort)."""
import functools
import os
import re
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
BLOCK, FINE, FINE_LOG2 = 32768, 16384, 14
RANKS = (16, 64, 256, 1024)
K1, B = F32(1.2), F32(0.75)
K1P1, ONE_MINUS_B = K1 + F32(1.0), F32(1.0) - B
M64 = (1 << 64) - 1


# ==================================================================== the reference
def np_impact(tf, dl, avgdl):
    """w = (tf * (k1 + 1)) / (tf + k1 * ((1 - b) + b * (dl / avgdl))), one float32 operation at a time."""
    tf, dl = np.asarray(tf).astype(F32), np.asarray(dl).astype(F32)
    kd = K1 * (ONE_MINUS_B + B * (dl / F32(avgdl)))
    return (tf * K1P1) / (tf + kd)


def np_avgdl(tokens, n):
    return F32(np.float64(int(tokens)) / np.float64(int(n)))


def _idf(O, n, df):
    u, inv = np.unique(np.asarray(df, np.int64), return_inverse=True)
    return np.array([O.bm25_idf(int(n), int(d)) for d in u], F32)[inv.reshape(-1)]


def _floors(impact, starts):
    """[vocab][4]: bits(r-th largest impact of the term) & 0xFFFFFC00 (the lower edge of its 22-bit bin) when df >= r, else 0."""
    vocab = starts.size - 1
    out = np.zeros((vocab, len(RANKS)), np.uint32)
    bits = impact.view(np.uint32)                                     # impacts are > 0: the bits order like the values
    for t in np.flatnonzero(np.diff(starts.astype(np.int64)) >= RANKS[0]):
        seg = np.sort(bits[starts[t]:starts[t + 1]])[::-1]
        for j, r in enumerate(RANKS):
            if seg.size >= r:
                out[t, j] = seg[r - 1] & np.uint32(0xFFFFFC00)
    return out


def np_build(terms, offs, vocab, global_n=None, global_tokens=None, global_df=None):
    """The index of a forward index (doc d owns terms[offs[d]:offs[d + 1]]) as HybridIndex.bm25_index() returns it, plus `term`,
    `doc` and `tf` per posting.  No global statistics: the local ones."""
    from oracle import lib as O
    terms, offs = np.asarray(terms, np.uint32), np.asarray(offs, np.uint64)
    n = offs.size - 1
    doc_len = np.diff(offs.astype(np.int64)).astype(np.uint32)
    doc_of = np.repeat(np.arange(n, dtype=np.uint64), doc_len)
    keys, tf = np.unique((terms[:int(offs[-1])].astype(np.uint64) << np.uint64(32)) | doc_of, return_counts=True)
    term, doc = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    n_win = 2 * ((n + BLOCK - 1) // BLOCK)
    cell_start = np.zeros(vocab * n_win + 1, np.uint32)
    cell_start[1:] = np.cumsum(np.bincount(term * n_win + (doc >> FINE_LOG2), minlength=vocab * n_win))
    df_local = np.bincount(term, minlength=vocab)
    if global_n is None:
        global_n, global_tokens = n, int(offs[-1])
    if global_df is None:
        global_df = df_local
    avgdl = np_avgdl(global_tokens, global_n)
    impact = np_impact(tf, doc_len[doc], avgdl) if keys.size else np.zeros(0, F32)
    starts = cell_start[::n_win]
    return dict(n_postings=int(keys.size), n_win=n_win, avgdl=avgdl, dib=(doc & (BLOCK - 1)).astype(np.uint32), impact=impact,
                cell_start=cell_start, idf=_idf(O, global_n, global_df), floors=_floors(impact, starts), doc_len=doc_len,
                term=term, doc=doc, tf=tf, starts=starts, df_local=df_local)


def np_scores(bld, n, idf, query):
    """score(d) = sum over the query's terms, in query order, of idf_t * impact(t, d): float32 adds from +0."""
    s = np.zeros(n, F32)
    for t in query:
        lo, hi = int(bld["starts"][t]), int(bld["starts"][t + 1])
        d = bld["doc"][lo:hi]
        s[d] = s[d] + idf[t] * bld["impact"][lo:hi]
    return s


# ==================================================================== corpus helpers
def fwd_from_pairs(n, docs, terms):
    """(terms, offs) of n documents from (doc, term) token pairs, in any order (a pair given twice: tf 2)."""
    docs = np.asarray(docs, np.int64)
    order = np.argsort(docs, kind="stable")
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(np.bincount(docs, minlength=n))
    return np.asarray(terms, np.uint32)[order], offs


def fwd_from_docs(docs):
    offs = np.zeros(len(docs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in docs])
    return np.array([t for d in docs for t in d], np.uint32), offs


def fwd_subject_docs(n, where, subj, tf, dl, filler):
    """Document where[i] holds tf[i] tokens of term subj[i] and dl[i] - tf[i] of the filler term; every other document is empty."""
    where, subj, tf, dl = (np.asarray(a, np.int64) for a in (where, subj, tf, dl))
    assert np.all(dl >= tf) and np.all(tf >= 1) and np.unique(where).size == where.size
    lens = np.zeros(n, np.int64)
    lens[where] = dl
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    terms = np.full(int(offs[-1]), filler, np.uint32)
    first = offs[:-1].astype(np.int64)[where]
    k = np.arange(int(tf.sum())) - np.repeat(np.cumsum(tf) - tf, tf)
    terms[np.repeat(first, tf) + k] = np.repeat(subj, tf)
    return terms, offs


# ==================================================================== mirror 1: bm_count_kernel's fold of a wave
def fold_trace(cell):
    """cell: the (term, window) cell of every sorted unique key.  -> (counts per cell as the kernel adds them up, the set of
    (head lane, run) additions per wave).  Wave w holds keys 64 w .. 64 w + 63; a head lane adds its run = the lanes up to the
    next head or the first invalid lane; lane 63 adds 1."""
    cell = np.asarray(cell, np.int64)
    counts, adds = {}, []
    for w0 in range(0, cell.size, 64):
        c = cell[w0:w0 + 64]
        heads = sum(1 << l for l in range(c.size) if l == 0 or c[l - 1] != c[l])
        valids = (1 << c.size) - 1
        for lane in range(c.size):
            if not (heads >> lane) & 1:
                continue
            above = 0 if lane == 63 else (((heads | (~valids & M64)) & M64) >> (lane + 1))
            run = ((above & -above).bit_length() - 1) + 1 if above else 64 - lane
            counts[int(c[lane])] = counts.get(int(c[lane]), 0) + run
            adds.append((w0 // 64, lane, run))
    return counts, adds


def run_features(runs):
    """runs: the lengths of consecutive cell runs of a key array -> what the layout reaches."""
    f, s, total = set(), 0, sum(runs)
    for r in runs:
        if r == 0:
            continue
        e = s + r
        f.add("head%d" % (s & 63))
        waves = (e - 1) // 64 - s // 64 + 1
        f.add("spans%d" % waves)
        if (e - 1) & 63 == 63 and waves == 1 and e < total:
            f.add("ends_at_63")
        if r == 1 and s & 63 == 63:
            f.add("len1_at_63")
        s = e
    f.add("last_wave_%d" % (((total - 1) & 63) + 1))
    return f


# name -> run lengths (one-token documents; run k is term 2 k + 1, so term 0, every even term and the last term are unused)
WAVE_CASES = {
    "t1": [1],
    "t63": [1, 61, 1],                    # heads on lanes 0, 1, 62; 63 valid lanes
    "t64": [1, 61, 1, 1],                 # a run of length 1 on lane 63
    "t65": [62, 3],                       # head on lane 62, two waves; a last wave of 1 lane
    "t255": [63, 66, 126],                # head on lane 63 over three waves; head on lane 1 over two; 63 valid lanes at the end
    "t256": [1, 63, 64, 62, 2, 64],       # a run ending exactly on lane 63 with the next head on lane 0; whole-wave runs
    "t257": [127, 130],                   # the second workgroup; head on lane 63 over four waves; a last wave of 1 lane
}
WAVE_TOTALS = {1, 63, 64, 65, 255, 256, 257}


def wave_corpus(name):
    runs = WAVE_CASES[name]
    vocab, n = 2 * len(runs) + 2, sum(runs)
    of_pos = np.repeat(2 * np.arange(len(runs)) + 1, runs)
    terms = of_pos[np.random.default_rng(n).permutation(n)]          # the sort has work to do; the runs keep their lengths
    return terms.astype(np.uint32), np.arange(n + 1, dtype=np.uint64), vocab


# ==================================================================== mirror 2: bm_floor_find
def floor_find(hist, kk):
    """The bin of hist[0 .. 2048) holding the kk-th entry from the top: lane l owns bins 2047 - 32 l - (0 .. 31).
    -> (bin, entries above it, owner lane, i at the exit)."""
    mine = hist[::-1].reshape(64, 32).sum(axis=1)
    incl = np.cumsum(mine)
    hit = np.flatnonzero(incl >= kk)
    owner = int(hit[0]) if hit.size else 63
    cum, b = int(incl[owner] - mine[owner]), 2047 - 32 * owner
    for i in range(32):
        c = int(hist[b])
        if cum + c >= kk or i == 31:
            break
        cum += c
        b -= 1
    return b, cum, owner, i


def floor_trace(impact, r):
    """The two passes of bm_term_floor_kernel for rank r over one term's impacts."""
    bits = np.asarray(impact, F32).view(np.uint32).astype(np.int64)
    assert bits.size >= r
    b1, above1, lane1, i1 = floor_find(np.bincount(bits >> 21, minlength=2048), r)
    inbin = bits[(bits >> 21) == b1]
    kk = r - above1
    b2, above2, lane2, i2 = floor_find(np.bincount((inbin >> 10) & 2047, minlength=2048), kk)
    return dict(floor=(b1 << 21) | (b2 << 10), bin1=b1, lane1=lane1, i1=i1, kk=kk, in_bin1=int(inbin.size), bin2=b2, lane2=lane2, i2=i2)


# ==================================================================== the floors corpora
FLOOR_AVGDL = 64           # pinned through the global statistics: a document's (tf, dl) alone decides its impact
FLOOR_GLOBAL_N = 1 << 20
EDGES = (1.0, 1.25, 1.5, 1.75, 2.0)     # leading-11-bit bin edges: bins 508 .. 512; 512 is lane 47's last bin, 511 lane 48's first
DF_CLASSES = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 5000)


@functools.lru_cache(maxsize=None)
def impact_table():
    """Every (tf, dl) with tf 1 .. 12, dl tf .. 128, sorted by impact at avgdl = 64: (tf, dl, impact bits)."""
    tf, dl = np.meshgrid(np.arange(1, 13), np.arange(1, 129), indexing="ij")
    ok = dl >= tf
    tf, dl = tf[ok], dl[ok]
    bits = np_impact(tf, dl, np_avgdl(FLOOR_AVGDL * FLOOR_GLOBAL_N, FLOOR_GLOBAL_N)).view(np.uint32).astype(np.int64)
    o = np.argsort(bits, kind="stable")
    return tf[o], dl[o], bits[o]


def _lane2(bits):
    return (2047 - ((bits >> 10) & 2047)) // 32


def _pairs_in_one_leading_bin():
    """Indices (hi, lo) of neighbouring table values in one leading bin but different 22-bit bins: one pair inside a lane of the
    second pass, one across a lane edge -- with the upper value in its lane's LAST bin (the i == 31 exit) where the table has one."""
    _, _, bits = impact_table()
    u = np.flatnonzero(np.diff(bits) > 0)                          # bits[u] < bits[u + 1]
    same_lead = (bits[u] >> 21) == (bits[u + 1] >> 21)
    other22 = (bits[u] >> 10) != (bits[u + 1] >> 10)
    lane_lo, lane_hi = _lane2(bits[u]), _lane2(bits[u + 1])
    inside = u[same_lead & other22 & (lane_lo == lane_hi)]
    across = u[same_lead & other22 & (lane_lo != lane_hi)]
    last = across[((bits[across + 1] >> 10) & 31) == 0]
    assert inside.size and across.size
    a = last[0] if last.size else across[0]
    return (int(inside[0]) + 1, int(inside[0])), (int(a) + 1, int(a))


def _top_of_a_leading_bin():
    """Index of a table value that is the largest of its leading bin, with a smaller one in another 22-bit bin of that bin, and
    with at least 1023 table values above it (for the kk = 1 shape)."""
    _, _, bits = impact_table()
    lead = bits >> 21
    for i in range(bits.size - 1024, 0, -1):
        if lead[i + 1] != lead[i] and lead[i - 1] == lead[i] and (bits[i - 1] >> 10) != (bits[i] >> 10):
            return i
    raise AssertionError("no such table value")


@functools.lru_cache(maxsize=None)
def shape_specs():
    """[(name, rank, n_hi, hi index, lo index, hi pool, lo pool)]: a term whose n_hi largest impacts are table[hi] and values of
    the hi pool (all >= table[hi]); the others are table[lo] and values of the lo pool (all <= table[lo])."""
    _, _, bits = impact_table()
    N = bits.size
    specs = []
    inside, across = _pairs_in_one_leading_bin()
    top = _top_of_a_leading_bin()
    for r in RANKS:
        one = int(np.searchsorted(bits, F32(1.0).view(np.uint32)))
        specs.append(("equal", r, r, one, one, (one, one + 1), (one, one + 1)))
        for E in EDGES:
            hi = int(np.searchsorted(bits, int(F32(E).view(np.uint32))))          # the smallest value >= E
            assert 0 < hi < N and bits[hi - 1] < int(F32(E).view(np.uint32)) <= bits[hi]
            specs.append(("above%g" % E, r, r, hi, hi - 1, (hi, N), (0, hi)))         # the r-th is just above the edge
            specs.append(("below%g" % E, r, r - 1, hi, hi - 1, (hi, N), (0, hi)))     # the r-th is just below it
        specs.append(("bin22", r, r, inside[0], inside[1], (inside[0], N), (0, inside[1] + 1)))
        specs.append(("lane2", r, r, across[0], across[1], (across[0], N), (0, across[1] + 1)))
        first_above = int(np.searchsorted(bits >> 21, (bits[top] >> 21) + 1))   # the values of the higher leading bins
        specs.append(("kk1", r, r, top, top - 1, (first_above, N), (0, top)))
    return tuple(specs)


SHAPE_EXTRA = 6            # postings below the n_hi largest


@functools.lru_cache(maxsize=None)
def shapes_corpus():
    """One term per (shape, rank) + the filler term: -> (terms, offs, vocab, n, [table indices of each term's documents])."""
    specs = shape_specs()
    rng = np.random.default_rng(1024)
    ttf, tdl, _ = impact_table()
    subj, pick = [], []
    for t, (name, r, n_hi, hi, lo, hp, lp) in enumerate(specs):
        n_lo = r + SHAPE_EXTRA - n_hi
        idx = np.concatenate([rng.integers(hp[0], hp[1], size=n_hi - 1), [hi], [lo], rng.integers(lp[0], lp[1], size=n_lo - 1)])
        subj.append(np.full(idx.size, t))
        pick.append(idx)
    subj, allpick = np.concatenate(subj), np.concatenate(pick)
    n = subj.size + 100                                                         # some documents stay empty
    where = rng.permutation(n)[:subj.size]
    vocab = len(specs) + 1
    terms, offs = fwd_subject_docs(n, where, subj, ttf[allpick], tdl[allpick], vocab - 1)
    return terms, offs, vocab, n, pick


@functools.lru_cache(maxsize=None)
def df_classes_corpus():
    """Term i has DF_CLASSES[i] postings, impacts drawn from the table; the documents are spread over three windows."""
    rng = np.random.default_rng(5000)
    ttf, tdl, _ = impact_table()
    subj = np.repeat(np.arange(len(DF_CLASSES)), DF_CLASSES)
    pick = rng.integers(0, ttf.size, size=subj.size)
    n = 40000
    where = rng.permutation(n)[:subj.size]
    vocab = len(DF_CLASSES) + 1
    terms, offs = fwd_subject_docs(n, where, subj, ttf[pick], tdl[pick], vocab - 1)
    return terms, offs, vocab, n


FLOOR_STATS = (FLOOR_GLOBAL_N, FLOOR_AVGDL * FLOOR_GLOBAL_N, None)


# ==================================================================== the window corpora
WIN_N = (1, 16383, 16384, 16385, 32767, 32768, 32769, 65537)
T_LO, T_EDGE, T_NOFIRST, T_NOMID, T_NOLAST, T_NEVER, T_FILL, T_HI = range(8)


@functools.lru_cache(maxsize=None)
def window_corpus(n, ends_used):
    """vocab 8.  T_EDGE: the first and the last document of every window, nothing else.  T_NOFIRST / T_NOMID / T_NOLAST: random
    documents, none in the first / a middle / the last window that holds documents.  T_NEVER (between two used terms): unused.
    Term 0 and term 7: both used, or both unused."""
    rng = np.random.default_rng(2 * n + ends_used)
    m = 2 * n + 8
    docs = rng.integers(0, n, size=m)
    pool = [T_NOFIRST, T_NOMID, T_NOLAST, T_FILL] + ([T_LO, T_HI] if ends_used else [])
    tt = np.array(pool)[rng.integers(0, len(pool), size=m)]
    used_win = (n + FINE - 1) // FINE
    win = docs >> FINE_LOG2
    drop = ((tt == T_NOFIRST) & (win == 0)) | ((tt == T_NOMID) & (win == used_win // 2)) | ((tt == T_NOLAST) & (win == used_win - 1))
    edge = sorted({w * FINE for w in range(used_win)} | {min((w + 1) * FINE, n) - 1 for w in range(used_win)})
    docs = np.concatenate([docs[~drop], edge])
    tt = np.concatenate([tt[~drop], np.full(len(edge), T_EDGE)])
    terms, offs = fwd_from_pairs(n, docs, tt)
    return terms, offs, 8


# ==================================================================== CPU tests: the reference and the mirrors are pinned first
def test_constants_equal_the_source():
    src = open(os.path.join(ROOT, "openintel_amd", "csrc", "bm25.hip")).read()
    assert re.search(r"ranks\[OI_BM25_FLOOR_RANKS\] = \{16u, 64u, 256u, 1024u\}", src)
    assert "#define BM_K1 1.2f" in src and "#define BM_B 0.75f" in src and "#define BM_F_LOG2 14" in src
    assert "hist[2047u - (lane * 32u + i)]" in src and "(d1 << 21) | (s_bin2 << 10)" in src
    assert K1P1 == F32(2.2) and ONE_MINUS_B == F32(0.25)


def test_np_impact_equals_the_oracle_bit_for_bit():
    from oracle import lib as O
    rng = np.random.default_rng(11)
    grid = [(dl, tf, av) for dl in (0, 1, 2, 3, 7, 64, 255, 1000, 100000) for tf in (1, 2, 3, 255, 70000)
            for av in (F32(1.0), F32(64.0), np_avgdl(3001, 1000), np_avgdl(1, 3), np_avgdl(12345678, 1000), F32(1e-3))]
    grid += [(int(rng.integers(0, 5000)), int(rng.integers(1, 300)), F32(rng.uniform(0.5, 400.0))) for _ in range(2000)]
    dl, tf, av = (np.array(x) for x in zip(*grid))
    for a in np.unique(av):
        m = av == a
        got = np_impact(tf[m], dl[m], a)
        want = np.array([O.bm25_impact(t, O.bm25_doc_norm(d, a)) for d, t in zip(dl[m], tf[m])], F32)
        assert got.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), float(a)
    kd = K1 * (ONE_MINUS_B + B * (dl.astype(F32)[:50] / F32(64.0)))
    assert np.array_equal(kd.view(np.uint32), np.array([O.bm25_doc_norm(d, 64.0) for d in dl[:50]], F32).view(np.uint32))


@pytest.mark.parametrize("seed", range(4))
def test_np_build_scores_equal_the_oracle_bit_for_bit(seed):
    """local statistics (even seeds) and global ones (odd seeds); queries repeat terms and name unused ones"""
    from oracle import lib as O
    rng = np.random.default_rng(seed)
    n, vocab = 70, 12
    lens = rng.integers(0, 9, size=n)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    terms = rng.integers(0, vocab - 1, size=int(offs[-1])).astype(np.uint32)           # term 11 is unused
    stats = (None, None, None) if seed % 2 == 0 else (1000 + seed, 4321, rng.integers(0, 1000, size=vocab).astype(np.uint32))
    bld = np_build(terms, offs, vocab, *stats)
    assert stats[0] is None or bld["avgdl"] == np_avgdl(4321, 1000 + seed)
    for q in ([0], [3, 3], [11], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 0, 11], list(rng.integers(0, vocab, size=5))):
        want = O.bm25_scores(terms, offs, vocab, np.array(q, np.uint32), df=stats[2], n_docs_global=stats[0], total_tokens_global=stats[1])
        got = np_scores(bld, n, bld["idf"], q)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), q


def test_wave_cases_reach_their_lanes():
    feats = set()
    for name, runs in WAVE_CASES.items():
        terms, offs, vocab = wave_corpus(name)
        bld = np_build(terms, offs, vocab)
        assert bld["n_win"] == 2 and np.array_equal(np.diff(bld["starts"].astype(np.int64))[1::2][:len(runs)], runs)   # the layout is the declared one
        cell = bld["term"] * 2 + (bld["doc"] >> FINE_LOG2)
        counts, adds = fold_trace(cell)
        assert counts == {int(c): int(k) for c, k in zip(*np.unique(cell, return_counts=True))}                      # the fold is a histogram
        f = run_features(runs)
        assert {"head%d" % l for _, l, _ in adds} >= {x for x in f if x.startswith("head")}
        feats |= f
    assert {sum(r) for r in WAVE_CASES.values()} == WAVE_TOTALS
    assert feats >= {"head0", "head1", "head62", "head63", "ends_at_63", "len1_at_63", "spans2", "spans3", "last_wave_1", "last_wave_63"}, feats
    assert (0, 63, 1) in fold_trace(np.repeat([1, 3, 5, 7], WAVE_CASES["t64"]))[1]
    assert "ends_at_63" in run_features(WAVE_CASES["t256"]) and "spans3" in run_features(WAVE_CASES["t255"])


def test_window_corpora_have_the_cells_they_declare():
    for n in WIN_N:
        for ends in (False, True):
            terms, offs, vocab = window_corpus(n, ends)
            bld = np_build(terms, offs, vocab)
            used_win, nw = (n + FINE - 1) // FINE, bld["n_win"]
            cnt = np.diff(bld["cell_start"].astype(np.int64)).reshape(vocab, nw)
            assert nw == 2 * ((n + BLOCK - 1) // BLOCK) and not cnt[:, used_win:].any()
            edge_docs = bld["doc"][bld["starts"][T_EDGE]:bld["starts"][T_EDGE + 1]]
            assert set(edge_docs) == {w * FINE for w in range(used_win)} | {min((w + 1) * FINE, n) - 1 for w in range(used_win)}
            assert cnt[T_NOFIRST, 0] == 0 and cnt[T_NOMID, used_win // 2] == 0 and cnt[T_NOLAST, used_win - 1] == 0 and not cnt[T_NEVER].any()
            assert (cnt[T_LO].any() and cnt[T_HI].any()) if ends else not (cnt[T_LO].any() or cnt[T_HI].any())
    cnt = np.diff(np_build(*window_corpus(65537, True))["cell_start"].astype(np.int64)).reshape(8, 6)
    assert cnt[T_NOFIRST, 1] and cnt[T_NOMID, 1] and cnt[T_NOMID, 3] and cnt[T_NOLAST, 3] and cnt[T_EDGE].tolist() == [2, 2, 2, 2, 1, 0]


def test_floor_shapes_reach_what_they_claim():
    terms, offs, vocab, n, pick = shapes_corpus()
    bld = np_build(terms, offs, vocab, *FLOOR_STATS)
    assert bld["avgdl"] == F32(FLOOR_AVGDL)
    _, _, tbits = impact_table()
    seen = set()
    for t, (name, r, n_hi, hi, lo, _, _) in enumerate(shape_specs()):
        imp = bld["impact"][bld["starts"][t]:bld["starts"][t + 1]]
        assert np.array_equal(np.sort(imp.view(np.uint32)), np.sort(tbits[pick[t]]).astype(np.uint32))      # the table decides the impacts
        j = RANKS.index(r)
        for jj, rr in enumerate(RANKS):                                                                      # the mirror is the reference's floor
            if imp.size >= rr:
                assert floor_trace(imp, rr)["floor"] == int(bld["floors"][t, jj]), (name, r, rr)
            else:
                assert bld["floors"][t, jj] == 0
        tr = floor_trace(imp, r)
        want_rth = tbits[hi] if n_hi == r else tbits[lo]
        assert int(bld["floors"][t, j]) == int(want_rth) & 0xFFFFFC00, (name, r)
        if name == "equal":
            assert tr["kk"] == r and tr["in_bin1"] == imp.size
        elif name.startswith("above"):
            E = float(name[5:])
            assert tr["bin1"] == int(F32(E).view(np.uint32)) >> 21 and tr["kk"] == tr["in_bin1"], (name, r, tr)        # kk = the whole leading bin
            assert E != 2.0 or (tr["lane1"], tr["i1"]) == (47, 31)
        elif name.startswith("below"):
            E = float(name[5:])
            assert tr["bin1"] < int(F32(E).view(np.uint32)) >> 21 and tr["kk"] == 1, (name, r, tr)
            assert E != 2.0 or (tr["bin1"], tr["lane1"], tr["i1"]) == (511, 48, 0)
        elif name == "bin22":
            assert tbits[hi] >> 21 == tbits[lo] >> 21 and tbits[hi] >> 10 != tbits[lo] >> 10 and _lane2(tbits[hi]) == _lane2(tbits[lo])
            assert tr["bin2"] == (tbits[hi] >> 10) & 2047
        elif name == "lane2":
            assert tbits[hi] >> 21 == tbits[lo] >> 21 and _lane2(tbits[hi]) + 1 <= _lane2(tbits[lo]) and tr["lane2"] == _lane2(tbits[hi])
            seen.add("i2=%d" % tr["i2"])
        elif name == "kk1":
            assert tr["kk"] == 1 and tr["in_bin1"] >= 2 and tr["bin1"] == tbits[hi] >> 21
        seen.add(name)
    assert seen >= {"equal", "bin22", "lane2", "kk1", "i2=31"} | {"%s%g" % (s, E) for s in ("above", "below") for E in EDGES}
    assert [int(F32(E).view(np.uint32)) >> 21 for E in EDGES] == [508, 509, 510, 511, 512]


def test_df_classes_corpus_has_the_declared_dfs():
    terms, offs, vocab, n = df_classes_corpus()
    bld = np_build(terms, offs, vocab, *FLOOR_STATS)
    assert bld["df_local"][:-1].tolist() == list(DF_CLASSES) and bld["n_win"] == 4
    assert all(np.diff(bld["cell_start"].astype(np.int64)).reshape(vocab, 4)[t, :3].all() for t in (9, 12, 14))  # large terms span the windows
    nz = bld["floors"] != 0
    assert [int(nz[t].sum()) for t in range(len(DF_CLASSES))] == [sum(d >= r for r in RANKS) for d in DF_CLASSES]
    for t in (3, 6, 9, 12, 14):
        imp = bld["impact"][bld["starts"][t]:bld["starts"][t + 1]]
        for j, r in enumerate(RANKS):
            if imp.size >= r:
                assert floor_trace(imp, r)["floor"] == int(bld["floors"][t, j])


# ==================================================================== GPU
@pytest.fixture(scope="module")
def ctx():
    import openintel_amd as oi
    c = oi.HipContext(0)
    yield c
    c.close()


def _first(a, b):
    d = np.flatnonzero(np.asarray(a).reshape(-1) != np.asarray(b).reshape(-1))
    return int(d[0]) if d.size else None


def diff_index(got, want, vocab):
    """Every array of bm25_index() against the reference: -> a list of differences, each naming the first place."""
    bad = []
    nw = want["n_win"]
    for k in ("n_postings", "n_win"):
        if got[k] != want[k]:
            bad.append("%s: %d, expected %d" % (k, got[k], want[k]))
    if F32(got["avgdl"]).view(np.uint32) != F32(want["avgdl"]).view(np.uint32):
        bad.append("avgdl: %r, expected %r" % (got["avgdl"], want["avgdl"]))
    if got["cell_start"].shape != want["cell_start"].shape:
        bad.append("cell_start: %d entries, expected %d" % (got["cell_start"].size, want["cell_start"].size))
    else:
        i = _first(got["cell_start"], want["cell_start"])
        if i is not None:
            bad.append("cell_start[term %d][window %d]: %d, expected %d" % (i // nw, i % nw, got["cell_start"][i], want["cell_start"][i]))
    if got["dib"].size == want["dib"].size:
        for k, view in (("dib", np.uint32), ("impact", np.uint32)):
            i = _first(got[k].view(view), want[k].view(view))
            if i is not None:
                t = int(np.searchsorted(want["cell_start"][::nw], i, side="right")) - 1
                bad.append("posting %d (term %d) %s: %r, expected %r" % (i, t, k, got[k][i], want[k][i]))
    for k in ("idf", "doc_len"):
        i = _first(got[k].view(np.uint32), want[k].view(np.uint32))
        if i is not None:
            bad.append("%s[%d]: %r, expected %r" % (k, i, got[k][i], want[k][i]))
    i = _first(got["floors"], want["floors"])
    if i is not None:
        t, j = divmod(i, len(RANKS))
        bad.append("floors[term %d][rank %d]: %#x, expected %#x (df %d)" % (t, RANKS[j], got["floors"][t, j], want["floors"][t, j],
                                                                         int(want["cell_start"][(t + 1) * nw]) - int(want["cell_start"][t * nw])))
    return bad


def _index(ctx, terms, offs, vocab, stats=(None, None, None), rows=None, dim=4):
    import openintel_amd as oi
    idx = oi.HybridIndex(ctx, offs.size - 1, dim, vocab)
    if rows is not None:
        idx.set_embeddings(rows, normalize=True)
    idx.set_forward(terms if terms.size else np.zeros(1, np.uint32), offs)
    idx.finalize(*stats)
    return idx


def _check(ctx, terms, offs, vocab, stats=(None, None, None)):
    want = np_build(terms, offs, vocab, *stats)
    idx = _index(ctx, terms, offs, vocab, stats)
    got = idx.bm25_index()
    idx.close()
    bad = diff_index(got, want, vocab)
    assert not bad, bad
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(WAVE_CASES))
def test_build_wave_folding(ctx, name):
    _check(ctx, *wave_corpus(name))


@pytest.mark.gpu
@pytest.mark.parametrize("ends_used", (False, True))
@pytest.mark.parametrize("n", WIN_N)
def test_build_windows_blocks_vocabulary(ctx, n, ends_used):
    _check(ctx, *window_corpus(n, ends_used))


@pytest.mark.gpu
def test_build_vocab_of_one(ctx):
    rng = np.random.default_rng(1)
    lens = rng.integers(0, 6, size=100)
    offs = np.zeros(101, np.uint64)
    offs[1:] = np.cumsum(lens)
    got, _ = _check(ctx, np.zeros(int(offs[-1]), np.uint32), offs, 1)
    assert got["cell_start"].tolist() == [0, int((lens > 0).sum()), int((lens > 0).sum())]


@pytest.mark.gpu
def test_build_tf_and_lengths(ctx):
    """tf 1, 2, 3, 255 and 70 000 (in a document of 100 000 tokens: the long per-thread loop of bm_make_keys_kernel); empty
    documents inside and at the end"""
    long_doc = [5] * 70000 + [6] * 10000 + [7] * 10000 + [1] * 10000
    docs = [[1], [], [1, 1, 2], [1, 2, 1, 1], [1] * 255 + [3], [], long_doc, [2, 3, 2], [5, 1], [], []]
    rng = np.random.default_rng(7)
    docs[6] = list(rng.permutation(long_doc))
    terms, offs = fwd_from_docs(docs)
    got, want = _check(ctx, terms, offs, 9)
    assert set(want["tf"].tolist()) == {1, 2, 3, 255, 10000, 70000} and want["n_postings"] == 15
    assert got["doc_len"].tolist() == [1, 0, 3, 4, 256, 0, 100000, 3, 2, 0, 0]


@pytest.mark.gpu
def test_build_no_tokens_at_all(ctx):
    got, _ = _check(ctx, np.zeros(0, np.uint32), np.zeros(6, np.uint64), 5)
    assert got["n_postings"] == 0 and not got["floors"].any() and not got["doc_len"].any() and not got["cell_start"].any()
    assert got["dib"].size == 0 and got["avgdl"] == 0


def _small_corpus(n, vocab, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 7, size=n)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    return rng.integers(0, vocab, size=int(offs[-1])).astype(np.uint32), offs


@pytest.mark.gpu
def test_build_global_statistics(ctx):
    """global n, tokens and df all differ from the local ones; avgdl = 3.001 is not representable; df of 0, 1 and global_n"""
    n, vocab = 300, 8
    terms, offs = _small_corpus(n, vocab, 3)
    df_a = np.array([0, 1, 1000, 17, 999, 500, 2, 0], np.uint32)
    got_a, want_a = _check(ctx, terms, offs, vocab, (1000, 3001, df_a))
    assert want_a["avgdl"] != np_avgdl(offs[-1], n) and np.all(df_a != want_a["df_local"]) and float(want_a["avgdl"]) != 3.001
    # only the df changes: the idf follows it, the postings do not move
    df_b = np.array([1000, 0, 1, 1, 0, 1000, 999, 3], np.uint32)
    got_b, _ = _check(ctx, terms, offs, vocab, (1000, 3001, df_b))
    assert np.array_equal(got_a["impact"].view(np.uint32), got_b["impact"].view(np.uint32)) and np.array_equal(got_a["dib"], got_b["dib"])
    assert np.all(got_a["idf"].view(np.uint32) != got_b["idf"].view(np.uint32))
    # the local statistics (no global ones given)
    _check(ctx, terms, offs, vocab)


@pytest.mark.gpu
def test_build_global_n_and_tokens_of_one(ctx):
    terms, offs = fwd_from_docs([[2, 0, 2, 2, 1]])
    for df in ([0, 1, 1], [1, 0, 0]):
        got, _ = _check(ctx, terms, offs, 3, (1, 1, np.array(df, np.uint32)))
        assert got["avgdl"] == 1 and got["doc_len"].tolist() == [5]


@pytest.mark.gpu
def test_build_floors_df_classes(ctx):
    terms, offs, vocab, n = df_classes_corpus()
    _check(ctx, terms, offs, vocab, FLOOR_STATS)


@pytest.mark.gpu
def test_build_floors_shapes(ctx):
    """every (shape, rank) term of shape_specs(): the expected floors are np_build's; test_floor_shapes_reach_what_they_claim
    shows what each one reaches"""
    terms, offs, vocab, n, _ = shapes_corpus()
    _check(ctx, terms, offs, vocab, FLOOR_STATS)


@pytest.mark.gpu
def test_rebuild_replaces_every_array(ctx):
    """term 0: 1100 postings in the first corpus (four floors), 10 in the second (none); the dump needs a finalized index"""
    import openintel_amd as oi
    from openintel_amd import _lib
    n, vocab = 1200, 4
    rng = np.random.default_rng(9)
    t1, o1 = fwd_subject_docs(n, np.arange(1100), np.zeros(1100), rng.integers(1, 4, size=1100), rng.integers(3, 40, size=1100), 1)
    t2, o2 = fwd_subject_docs(n, rng.permutation(n)[:900], np.repeat([0, 2], [10, 890]), rng.integers(1, 3, size=900), rng.integers(2, 9, size=900), 3)
    w1, w2 = np_build(t1, o1, vocab), np_build(t2, o2, vocab)
    assert w1["floors"][0].all() and not w2["floors"][0].any() and w2["floors"][2].any() and w2["df_local"][0] == 10
    idx = oi.HybridIndex(ctx, n, 4, vocab)
    idx.set_forward(t1, o1)
    with pytest.raises(_lib.OiError) as e:
        idx.bm25_index()
    assert e.value.code == _lib.OI_ERR_STATE
    idx.finalize()
    bad = diff_index(idx.bm25_index(), w1, vocab)
    idx.set_forward(t2, o2)
    with pytest.raises(_lib.OiError) as e:
        idx.bm25_index()
    assert e.value.code == _lib.OI_ERR_STATE
    idx.finalize()
    got = idx.bm25_index()
    idx.close()
    bad += diff_index(got, w2, vocab)
    assert not bad, bad
    assert not got["floors"][0].any()


@pytest.mark.gpu
def test_view_dumps_the_sources_arrays(ctx):
    import openintel_amd as oi
    n, vocab = 500, 16
    terms, offs = _small_corpus(n, vocab, 5)
    stats = (900, 2500, None)
    idx = _index(ctx, terms, offs, vocab, stats, rows=np.random.default_rng(2).standard_normal((n, 4)).astype(F32))
    ctx2 = oi.HipContext(0)
    v = idx.view(ctx2)
    got, src = v.bm25_index(), idx.bm25_index()
    v.close()
    idx.close()
    ctx2.close()
    bad = diff_index(got, np_build(terms, offs, vocab, *stats), vocab) + diff_index(got, src, vocab)
    assert not bad, bad


@pytest.mark.gpu
def test_set_text_builds_the_index_of_the_reference_tokens(ctx):
    import openintel_amd as oi
    from openintel_amd import synth
    from test_text_terms_abi import ref_text_terms
    vocab = 512
    texts = synth.posts_np(300) + ["", "AAPL aapl AAPL to the moon", ""]
    terms, offs = ref_text_terms(texts, vocab)
    want = np_build(terms, offs, vocab)
    a = oi.HybridIndex(ctx, len(texts), 4, vocab)
    a.set_text(texts)
    a.finalize()
    b = _index(ctx, terms, offs, vocab)
    got_a, got_b = a.bm25_index(), b.bm25_index()
    a.close()
    b.close()
    bad = diff_index(got_a, want, vocab) + diff_index(got_b, want, vocab)
    assert not bad, bad


BIG_N = 65535 * 256 + 300


@pytest.mark.gpu
def test_build_grid_stride_second_trip(ctx):
    """65535 * 256 + 300 one-token documents, term = doc mod 3: the only shape at which a workgroup of bm_make_keys_kernel,
    bm_count_kernel and bm_impact_kernel (grids capped at 65535 blocks of 256) takes a second trip.  Every document has dl = 1
    and tf = 1, so the expected arrays follow from counting residues."""
    from oracle import lib as O
    t0 = time.perf_counter()
    n, vocab = BIG_N, 3
    assert (n + 255) // 256 > 65535
    terms = (np.arange(n, dtype=np.uint32) % np.uint32(3))
    offs = np.arange(n + 1, dtype=np.uint64)
    n_win = 2 * ((n + BLOCK - 1) // BLOCK)
    lo = np.minimum(np.arange(n_win, dtype=np.int64) * FINE, n)
    hi = np.minimum(lo + FINE, n)
    t = np.arange(3, dtype=np.int64)[:, None]
    cnt = (hi[None, :] - t + 2) // 3 - (lo[None, :] - t + 2) // 3              # docs of [lo, hi) with doc mod 3 == t
    cell_start = np.zeros(vocab * n_win + 1, np.uint32)
    cell_start[1:] = np.cumsum(cnt.reshape(-1))
    df = cnt.sum(axis=1)
    assert int(cell_start[-1]) == n and cnt[:, 0].tolist() == [5462, 5461, 5461]
    w = np_impact([1], [1], np_avgdl(n, n))[0]
    want = dict(n_postings=n, n_win=n_win, avgdl=F32(1.0), cell_start=cell_start, idf=_idf(O, n, df),
                dib=np.concatenate([np.arange(r, n, 3, dtype=np.uint32) & np.uint32(BLOCK - 1) for r in range(3)]),
                impact=np.full(n, w, F32), doc_len=np.ones(n, np.uint32),
                floors=np.full((3, 4), int(w.view(np.uint32)) & 0xFFFFFC00, np.uint32))
    t1 = time.perf_counter()
    idx = _index(ctx, terms, offs, vocab)
    got = idx.bm25_index()
    idx.close()
    t2 = time.perf_counter()
    bad = diff_index(got, want, vocab)
    print("grid-stride case: reference %.2f s, build + read-back %.2f s, compare %.2f s" % (t1 - t0, t2 - t1, time.perf_counter() - t2))
    assert not bad, bad
