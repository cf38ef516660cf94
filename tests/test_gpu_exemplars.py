"""Narrative exemplars (oi_label_exemplars): per cluster of a labelling, its member rows closest to its centroid.
The reference is the numpy restatement of the header's definition in this file: members by label, filter and non-NaN; sorted by
(-key(s), doc); cut at `top`.

EXACT corpora follow tests/test_gpu_seed.py: entries are small integers in [-2, 2] times 2^-k with 4^k >= dim, loaded with
normalize=False, and the centroids are planted centres from the same set of values.  Every product is a multiple of 4^-k and
every dot product at most 4, so each sum is exact in f32 in any order: scores, docs, counts and padding must equal the
reference BIT FOR BIT.  These corpora are full of tied scores by construction (test_exact_corpora_are_full_of_ties counts them
on the CPU side of a run).  Float corpora are checked against f64 within the library's 1e-5 contract."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BLOCK, RANGE, RADIX_BITS, THREADS = 64, 2048, 8, 256       # LE_* of label_exemplars.hip (tests/test_exemplars_abi.py compares)
NO_DOC = 0xFFFFFFFF


def _ctx(mode=None):
    import openintel_amd as oi
    c = oi.HipContext(0)
    if mode is not None:
        c.set_cosine_mode(mode)
    return c


# ------------------------------------------------------------------ the definition, in numpy
def _key(s):
    """oi_f32_key of f32 values that are not NaN: -0 folded into +0, then the order-preserving map"""
    b = (np.asarray(s, np.float32) + np.float32(0.0)).view(np.uint32).astype(np.uint64)
    return np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000)


def _sims(rows, cent):
    """sim(cent, row) of every row as f32 (exact corpora: the f32 chain's value in any order; inf and NaN as IEEE has them)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (rows.astype(np.float64) * cent.astype(np.float64)[None, :]).sum(axis=1).astype(np.float32)


def _passes(filt, group, stamp):
    gm, gv, lo, hi = (int(x) for x in filt)
    return ((group & gm) == gv) & (stamp >= lo) & (stamp <= hi)


def _reference(rows, labels, cents, top, base=0, filt=None, attrs=None, sims=None):
    """-> (scores f32 [K, top], docs u32 [K, top], counts u32 [K]).  sims: the f32 sims per cluster when the caller has them."""
    K = cents.shape[0]
    scores, docs, counts = np.zeros((K, top), np.float32), np.full((K, top), NO_DOC, np.uint32), np.zeros(K, np.uint32)
    ok = np.ones(len(labels), bool) if filt is None else _passes(filt, attrs[0], attrs[1])
    for c in range(K):
        d = np.flatnonzero((labels == c) & ok)
        if d.size == 0:
            continue
        s = _sims(rows[d], cents[c]) if sims is None else sims[c][d]
        keep = ~np.isnan(s)
        d, s = d[keep], s[keep]
        order = np.lexsort((d, -_key(s).astype(np.int64)))[:top]
        m = order.size
        scores[c, :m], docs[c, :m], counts[c] = s[order] + np.float32(0.0), d[order] + base, m
    return scores, docs, counts


# ------------------------------------------------------------------ data
def _k_of(dim):
    k = 0
    while 4 ** k < dim:
        k += 1
    return k


@functools.lru_cache(maxsize=None)
def _exact(dim, n, C=4, rs=0, noise=0.1, flip=0.1):
    """Planted clusters of small integers times 2^-k (the recipe of tests/test_gpu_seed.py): centres in {-2, 2}^dim, a member
    re-draws a tenth of its entries from [-2, 2], `noise` of the rows are uniform in [-2, 2].
    -> (rows f32 [n, dim], centres f32 [C, dim], which: the planted cluster per row)"""
    k = _k_of(dim)
    rng = np.random.default_rng(500 + rs)
    centres = rng.choice(np.array([-2, 2]), size=(C, dim))
    which = rng.integers(0, C, size=n)
    rows = centres[which].astype(np.int64)
    f = rng.random((n, dim)) < flip
    rows[f] = rng.integers(-2, 3, size=int(f.sum()))
    nz = rng.random(n) < noise
    rows[nz] = rng.integers(-2, 3, size=(int(nz.sum()), dim))
    scale = np.float32(2.0 ** -k)
    return (rows.astype(np.float32) * scale), (centres.astype(np.float32) * scale), which


def _labels(which, K, rs=0, stray=0.1):
    """the planted cluster modulo K, with `stray` of the rows given a random other label, K itself or 0xFFFFFFFF"""
    rng = np.random.default_rng(900 + rs)
    lab = (which % K).astype(np.uint32)
    r = rng.random(len(lab))
    lab[r < stray / 2] = rng.integers(0, K, size=int((r < stray / 2).sum()))
    lab[(r >= stray / 2) & (r < 3 * stray / 4)] = K
    lab[(r >= 3 * stray / 4) & (r < stray)] = NO_DOC
    return lab


def _cents(centres, K):
    return np.ascontiguousarray(centres[np.arange(K) % centres.shape[0]])


def _index(ctx, rows, bf16=False, attrs=None, finalize=False, copy_policy=None, base=0):
    import openintel_amd as oi
    n, dim = rows.shape
    idx = oi.HybridIndex(ctx, n, dim, 8, doc_id_base=base)
    if copy_policy is not None:
        idx.set_screen_copy(copy_policy)
    if bf16:
        bits = rows.view(np.uint32)
        assert not (bits & 0xFFFF).any()                              # the values are bf16 values
        idx.set_embeddings_bf16((bits >> 16).astype(np.uint16))
    else:
        idx.set_embeddings(rows, normalize=False)
    if attrs is not None:
        idx.set_doc_attrs(*attrs)
    if finalize:
        idx.set_forward(np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64))
        idx.finalize()
    return idx


def _host(x, dtype):
    if hasattr(x, "data_ptr"):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).view(dtype)


def _got(lists):
    return _host(lists.cos_scores, np.float32), _host(lists.cos_docs, np.uint32), _host(lists.cos_counts, np.uint32)


def _same(got, ref, what=""):
    """scores, docs, counts and padding, bit for bit"""
    gs, gd, gc = got
    rs, rd, rc = ref
    print(what, "counts", gc[:8], rc[:8], "docs", gd[0, :6], rd[0, :6])
    assert gc.tolist() == rc.tolist(), what
    assert gd.shape == rd.shape and gd.tobytes() == rd.tobytes(), what
    assert gs.shape == rs.shape and gs.tobytes() == rs.tobytes(), what


def _run(rows, labels, cents, top, ctx=None, idx=None, bf16=False, what="", **ref_kw):
    ctx = ctx or _ctx()
    idx = idx or _index(ctx, rows, bf16=bf16)
    got = _got(idx.label_exemplars(labels, cents, top=top))
    ref = _reference(rows, labels, cents, top, **ref_kw)
    _same(got, ref, what or "n=%d dim=%d K=%d top=%d" % (rows.shape + (cents.shape[0], top)))
    return idx, got


def _tied(got):
    """entries of the lists whose score equals their predecessor's"""
    s, _, c = got
    return sum(int((s[q, 1:c[q]] == s[q, :c[q] - 1]).sum()) for q in range(len(c)) if c[q] > 1)


# ------------------------------------------------------------------ the row walk
@pytest.mark.parametrize("n", [1, BLOCK - 1, BLOCK, BLOCK + 1, RANGE - 1, RANGE, RANGE + 1])
def test_sizes_around_the_block_and_range_edges(n):
    rows, centres, which = _exact(64, n, rs=n)
    for K, top in ((1, 10), (3, 7)):
        _run(rows, _labels(which, K, rs=n), _cents(centres, K), top)


def test_exact_corpora_are_full_of_ties():
    rows, centres, which = _exact(64, 3000, rs=1)
    _, got = _run(rows, _labels(which, 4), _cents(centres, 4), 200)
    s = _sims(rows, centres[0])
    assert len(np.unique(s)) <= 150                                   # the CPU side: 3000 rows, about a hundred distinct scores
    assert _tied(got) > 400                                           # and the lists are mostly runs of equal scores


def test_members_only_in_the_last_partial_block_and_a_range_without_members():
    n = 3 * RANGE + BLOCK + 6
    rows, centres, which = _exact(64, n, rs=2)
    lab = np.full(n, NO_DOC, np.uint32)
    lab[3 * RANGE + BLOCK:] = (which[3 * RANGE + BLOCK:] % 2).astype(np.uint32)          # the last, partial block only
    idx, got = _run(rows, lab, _cents(centres, 2), 4)
    assert int(got[2].sum()) == sum(min(4, int((lab == c).sum())) for c in range(2)) >= 4
    lab = _labels(which, 3, rs=2)
    lab[RANGE:2 * RANGE] = 3                                                           # the second range: no member at all
    _run(rows, lab, _cents(centres, 3), 12, idx=idx)


def test_all_rows_members_of_one_cluster_and_more_ranges_than_workgroups():
    rows, centres, which = _exact(64, 5000, rs=3)
    _run(rows, np.zeros(5000, np.uint32), _cents(centres, 1), 50)
    _run(rows, np.full(5000, 2, np.uint32), _cents(centres, 3), 50)
    # the score pass launches at most 4 workgroups per CU, a range at a time each: 1024 on 256 CUs -- these rows are 1030 ranges
    n = RANGE * 1029 + 77
    rows, centres, which = _exact(8, n, rs=4)
    _run(rows, _labels(which, 5, rs=4), _cents(centres, 5), 9)


# ------------------------------------------------------------------ dims
@pytest.mark.parametrize("dim", [8, 256, 260, 384, 768, 1024])
def test_dims_one_per_register_class_of_the_chain(dim):
    rows, centres, which = _exact(dim, 2500, rs=dim)
    _run(rows, _labels(which, 4, rs=dim), _cents(centres, 4), 20)


@pytest.mark.parametrize("dim", [384, 768, 1024])
def test_bf16_corpus(dim):
    rows, centres, which = _exact(dim, 2500, rs=dim + 1)
    _run(rows, _labels(which, 4, rs=dim), _cents(centres, 4), 20, bf16=True)


def test_bf16_corpus_rounds_the_centroid_the_way_its_scorer_does():
    """a centroid that is no bf16 value is rounded to nearest even before the chain; the stored rows are widened exactly"""
    rows, centres, which = _exact(384, 1500, rs=5)
    cents = _cents(centres, 3) * np.float32(1.0 + 2.0 ** -8 + 2.0 ** -9)             # not bf16 values any more: they round UP
    b = cents.view(np.uint32).astype(np.uint64)
    rounded = (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)
    assert (rounded != cents).all() and (np.abs(rounded) > np.abs(cents)).all()
    lab = _labels(which, 3, rs=5)
    ctx = _ctx()
    idx = _index(ctx, rows, bf16=True)
    # (rounded centroid entries are +-(1 + 2^-7) 2^-4: 9 significant bits times the rows' 2, sums below 2^10 terms -- still exact)
    _same(_got(idx.label_exemplars(lab, cents, top=15)), _reference(rows, lab, rounded, 15), "bf16 rounding")


# ------------------------------------------------------------------ clusters and tops
@pytest.mark.parametrize("K", [1, 2, 64, 65, 255, 256])             # (64 | 65: the select's histogram in LDS | in global memory)
def test_cluster_counts(K):
    rows, centres, which = _exact(64, 3000, C=8, rs=6)
    rng = np.random.default_rng(K)
    lab = rng.integers(0, K, size=3000).astype(np.uint32)
    _run(rows, lab, _cents(centres, K), 6)


def test_empty_short_and_exactly_full_clusters_and_labels_out_of_range():
    rows, centres, which = _exact(64, 2500, rs=7)
    top, K = 8, 5
    lab = _labels(which, K, rs=7, stray=0.2)                          # (holds labels == K and 0xFFFFFFFF)
    assert (lab == K).any() and (lab == NO_DOC).any()
    lab[lab == 2] = NO_DOC                                            # an empty cluster in the middle
    three = np.flatnonzero(lab == 3)
    lab[three[top - 3:]] = K                                          # fewer than `top` members
    four = np.flatnonzero(lab == 4)
    lab[four[top:]] = 0xFFFFFFFE                                      # exactly `top` members
    _, (s, d, c) = _run(rows, lab, _cents(centres, K), top)
    assert c.tolist()[2:] == [0, top - 3, top] and c[0] == top
    assert (d[2] == NO_DOC).all() and not s[2].any() and (d[3, top - 3:] == NO_DOC).all()


@pytest.mark.parametrize("top", [1, 2, 1023, 1024])
def test_tops(top):
    rows, centres, which = _exact(64, 4000, rs=8)
    lab = _labels(which, 3, rs=8)
    _, (s, d, c) = _run(rows, lab, _cents(centres, 3), top)
    assert c.tolist() == [min(top, int((lab == q).sum())) for q in range(3)] and c.max() == top


# ------------------------------------------------------------------ ties at the cut, digits, special values
def test_three_thousand_identical_rows_return_the_ten_smallest_doc_ids():
    rows, centres, which = _exact(64, 4500, rs=9)
    rows = rows.copy()
    rng = np.random.default_rng(9)
    dup = np.sort(rng.choice(4500, size=3000, replace=False))
    rows[dup] = centres[1]                                            # retweets of the post at the centre: one score, the best
    lab = _labels(which, 3, rs=9, stray=0.0)
    lab[dup] = 1
    _, (s, d, c) = _run(rows, lab, _cents(centres, 3), 10)
    assert d[1].tolist() == dup[:10].tolist() and len(set(s[1].tolist())) == 1
    # and a cut inside the tie below a few better rows: 4 rows above the 3000
    rows[dup[-4:]] = centres[1] * np.float32(2.0)
    _, (s, d, c) = _run(rows, lab, _cents(centres, 3), 10)
    assert d[1].tolist() == dup[-4:].tolist() + dup[:6].tolist()


def _axis_corpus(values, dim=8):
    """row i = values[i] on axis 0, zeros elsewhere; the centroid is the unit axis: sim = values[i] exactly"""
    rows = np.zeros((len(values), dim), np.float32)
    rows[:, 0] = values
    cent = np.zeros((1, dim), np.float32)
    cent[0, 0] = 1.0
    return rows, cent


def test_keys_that_differ_in_one_radix_digit_only():
    rng = np.random.default_rng(10)
    # the last digit: 1 + i 2^-23, i < 256 -- and every value twice, so that the cut also falls inside a tie
    last = (np.float32(1.0) + np.arange(256, dtype=np.float32) * np.float32(2.0 ** -23)).astype(np.float32)
    assert len(set((_key(last) >> 8).tolist())) == 1 and len(set(_key(last).tolist())) == 256
    values = rng.permutation(np.concatenate([last, last]))
    rows, cent = _axis_corpus(values)
    lab = np.zeros(len(values), np.uint32)
    idx = _index(_ctx(), rows)
    for top in (1, 5, 255, 256, 257, 511, 512):
        _run(rows, lab, cent, top, idx=idx, sims=[values.astype(np.float32)])
    # the first digit: powers of two with exponents of one parity, both signs -- digits 2 to 4 agree within a sign
    first = np.array([2.0 ** e for e in (-60, -30, -2, 20, 64)] + [-(2.0 ** e) for e in (-60, -30, -2, 20, 64)], np.float32)
    k = _key(first)
    assert len(set((k >> 24).tolist())) == 10 and len(set((k[:5] & 0xFFFFFF).tolist())) == 1
    values = rng.permutation(np.repeat(first, 3))
    rows, cent = _axis_corpus(values)
    idx = _index(_ctx(), rows)
    for top in (1, 3, 4, 16, 30):
        _run(rows, np.zeros(len(values), np.uint32), cent, top, idx=idx, sims=[values.astype(np.float32)])


def test_negative_zero_and_infinite_scores_rank_as_ieee_orders_them_and_nan_is_never_listed():
    rows, centres, which = _exact(64, 600, C=2, rs=11)
    rows, cents = rows.copy(), _cents(centres, 3).copy()
    lab = (np.arange(600) % 3).astype(np.uint32)
    rows[0:6] = 0.0                                                   # +0 scores ...
    rows[6:12] = -0.0                                                 # ... against -0 products: one key, ties by doc id
    pos = int(np.flatnonzero(cents[0] > 0)[0])
    rows[30, pos] = np.inf                                            # +inf for cluster 0 (no entry of a centre is 0: no inf * 0)
    rows[33, pos] = -np.inf                                           # -inf
    rows[36, pos], rows[36, (pos + 1) % 64] = np.inf, np.nan          # NaN: never listed
    rows[39, 0], rows[39, 1] = np.inf, -np.inf
    rows[39] *= np.sign(cents[0])                                     # inf - inf = NaN
    cents[2, 5] = np.nan                                              # a NaN centroid: cluster 2 lists nobody
    members0 = int((lab == 0).sum())
    _, (s, d, c) = _run(rows, lab, cents, 300)
    assert c.tolist() == [members0 - 2, int((lab == 1).sum()), 0]
    assert d[0, 0] == 30 and s[0, 0] == np.inf and d[0, c[0] - 1] == 33 and s[0, c[0] - 1] == -np.inf
    z = np.flatnonzero(s[0, :c[0]] == 0.0)
    zd = d[0, z].tolist()
    assert {0, 3, 6, 9} <= set(zd) and zd == sorted(zd) and not np.signbit(s[0, z]).any()  # -0 and +0 tie by doc id; +0 comes back
    assert (s[0, :c[0]] < 0).any()                                    # negative scores below them
    _run(rows, lab, cents, 3)                                         # and a short cut over the same values


# ------------------------------------------------------------------ filter
def test_filter_removes_the_best_member_passes_nothing_and_needs_attributes():
    from openintel_amd import _lib
    n = RANGE + 300
    rows, centres, which = _exact(64, n, rs=12)
    lab = _labels(which, 3, rs=12)
    cents = _cents(centres, 3)
    group = (np.arange(n) % 4).astype(np.uint32)
    stamp = (1000 + np.arange(n)).astype(np.uint32)
    ctx = _ctx()
    idx = _index(ctx, rows, attrs=(group, stamp))
    _, plain = _run(rows, lab, cents, 10, idx=idx)
    best = int(plain[1][1, 0])
    stamp[best] = 5                                                   # the best member of cluster 1 falls out of the window
    idx.set_doc_attrs(group, stamp)
    filt = (0, 0, 1000, 1000 + n)
    got = _got(idx.label_exemplars(lab, cents, top=10, filter=filt))
    _same(got, _reference(rows, lab, cents, 10, filt=filt, attrs=(group, stamp)), "window")
    assert best not in got[1][1].tolist() and got[1][1, 0] == plain[1][1, 1]
    filt = (0x3, 0x2, 1100, 1000 + RANGE + 10)                        # a group of four and a window across the range edge
    got = _got(idx.label_exemplars(lab, cents, top=10, filter=filt))
    _same(got, _reference(rows, lab, cents, 10, filt=filt, attrs=(group, stamp)), "group and window")
    assert (group[got[1][got[1] != NO_DOC]] == 2).all()
    none = _got(idx.label_exemplars(lab, cents, top=10, filter=(0xFFFFFFFF, 0xDEAD, 0, 0xFFFFFFFF)))
    assert not none[2].any() and (none[1] == NO_DOC).all() and not none[0].any()
    no_attrs = _index(ctx, rows)
    with pytest.raises(_lib.OiError) as e:
        no_attrs.label_exemplars(lab, cents, top=10, filter=filt)
    assert e.value.code == _lib.OI_ERR_STATE
    _run(rows, lab, cents, 10, idx=no_attrs)                          # no attributes needed without a filter


# ------------------------------------------------------------------ placement and mode
def test_device_location_a_view_two_runs_and_a_doc_id_base():
    import torch
    rows, centres, which = _exact(64, 2 * RANGE + 100, rs=13)
    lab = _labels(which, 4, rs=13)
    cents = _cents(centres, 4)
    ref = _reference(rows, lab, cents, 25)
    ctx = _ctx()
    idx = _index(ctx, rows, finalize=True)
    host = _got(idx.label_exemplars(lab, cents, top=25))
    _same(host, ref, "host")
    dev = idx.label_exemplars(torch.from_numpy(lab.view(np.int32)).cuda(), torch.from_numpy(cents).cuda(), top=25)
    assert dev.cos_scores.is_cuda and dev.cos_docs.is_cuda and dev.cos_counts.is_cuda
    ctx.synchronize()
    _same(_got(dev), ref, "device")
    _same(_got(idx.label_exemplars(lab, cents, top=25)), ref, "again")
    ctx_v = _ctx()
    view = idx.view(ctx_v)
    _same(_got(view.label_exemplars(lab, cents, top=25)), ref, "view")
    view.close()
    based = _index(ctx, rows, base=70000)
    gs, gd, gc = _got(based.label_exemplars(lab, cents, top=25))
    assert gs.tobytes() == ref[0].tobytes() and gc.tolist() == ref[2].tolist()
    assert gd.tolist() == np.where(ref[1] == NO_DOC, NO_DOC, ref[1].astype(np.int64) + 70000).tolist()


def test_cosine_mode_and_copy_policy_change_nothing():
    from openintel_amd import _lib
    import openintel_amd as oi
    rows, centres, which = _exact(384, 3000, rs=14)
    lab = _labels(which, 4, rs=14)
    cents = _cents(centres, 4)
    ref = _reference(rows, lab, cents, 30)
    for mode, policy in ((None, None), (_lib.OI_COSINE_EXACT, None), (_lib.OI_COSINE_SPLIT, None), (_lib.OI_COSINE_SCREEN, None),
                         (None, oi.HybridIndex.SCREEN_COPY_NEVER), (_lib.OI_COSINE_SCREEN_COPY, oi.HybridIndex.SCREEN_COPY_ALWAYS),
                         (_lib.OI_COSINE_SCREEN_STREAM, None)):
        ctx = _ctx(mode)
        idx = _index(ctx, rows, finalize=True, copy_policy=policy)
        _same(_got(idx.label_exemplars(lab, cents, top=30)), ref, "mode %r policy %r" % (mode, policy))


def test_workspace_is_counted():
    rows, centres, which = _exact(64, 5000, rs=15)
    ctx = _ctx()
    idx = _index(ctx, rows)
    before = ctx.workspace_bytes()[0]
    idx.label_exemplars(_labels(which, 4), _cents(centres, 4), top=16)
    assert ctx.workspace_bytes()[0] - before >= 4 * 5000 + 4 * 1024 + 8 * 16 * 4


# ------------------------------------------------------------------ agreement with the rest of the library
def test_one_cluster_of_everything_is_the_exact_cosine_list():
    from openintel_amd import _lib, retriever
    rows, centres, which = _exact(384, 3000, rs=16)
    ctx = _ctx(_lib.OI_COSINE_EXACT)
    idx = _index(ctx, rows, finalize=True)
    qt, qo = retriever.pack_query_terms([[0]])
    for depth in (10, 300):
        want = idx.search_lists(centres[:1], qt, qo, depth=depth)
        got = _got(idx.label_exemplars(np.zeros(3000, np.uint32), centres[:1], top=depth))
        assert depth < 300 or _tied(got) > depth // 2                 # the tie rule is what is compared
        _same(got, (_host(want.cos_scores, np.float32), _host(want.cos_docs, np.uint32), _host(want.cos_counts, np.uint32)), "cosine list")


def _unit(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _planted(dim, C, n, seed, copies=False):
    """planted unit centres, noise sigma * sqrt(dim) = 0.45, a fifth of the rows pure noise (tests/test_gpu_narratives.py's
    data); copies: every row is followed by 0 to 3 bit-identical copies of itself, cut at n rows.
    -> (rows f32, centres f32, which: the planted direction per row, -1 for noise)"""
    rng = np.random.default_rng(seed)
    centres = _unit(rng.standard_normal((C, dim)))
    which = rng.integers(0, C, size=n)
    rows = centres[which] + rng.standard_normal((n, dim)) * (0.45 / np.sqrt(dim))
    noise = rng.random(n) < 0.2
    rows[noise] = rng.standard_normal((int(noise.sum()), dim))
    which = np.where(noise, -1, which)
    rows = _unit(rows).astype(np.float32)
    if copies:
        rep = np.repeat(np.arange(n), rng.integers(1, 5, size=n))[:n]
        rows, which = rows[rep], which[rep]
    return rows, centres.astype(np.float32), which


def _with_signals(idx, n):
    idx.set_signals(np.zeros(n), np.zeros(n, np.uint8), np.zeros(n, np.uint8), 0.2)
    return idx


@pytest.mark.parametrize("dim", [64, 768])
def test_labels_of_similar_share_and_the_f64_oracle(dim):
    n, K, t, top = 3000, 6, 0.35, 40
    rows, centres, _ = _planted(dim, K, n, 21)
    ctx = _ctx()
    idx = _with_signals(_index(ctx, rows), n)
    _, lab = idx.similar_share(centres, t, labels=True)
    s, d, c = _got(idx.label_exemplars(lab, centres, top=top))
    s64 = rows.astype(np.float64) @ centres.astype(np.float64).T
    assert c.min() >= 1
    for q in range(K):
        m = int(c[q])
        docs = d[q, :m].astype(np.int64)
        members = np.flatnonzero(lab == q)
        assert m == min(top, members.size) and len(set(docs.tolist())) == m
        assert (lab[docs] == q).all()                                 # every listed doc carries the cluster's label
        assert (s[q, :m] >= np.float32(t)).all()                      # the sim the share compared against t, so >= t
        err = np.abs(s[q, :m].astype(np.float64) - s64[docs, q]).max()
        cut = np.sort(s64[members, q])[::-1][m - 1]
        print(dim, q, "members", members.size, "max err", err, "lowest listed f64", s64[docs, q].min(), "cut", cut)
        assert err <= 1e-5                                            # the library's contract
        assert (np.diff(s[q, :m]) <= 0).all()                         # descending
        assert (s64[docs, q] >= cut - 2e-5).all()                     # two of its 1e-5 bounds
        assert (d[q, m:] == NO_DOC).all() and not s[q, m:].any()


# ------------------------------------------------------------------ composition
def test_narrative_exemplars_with_collapse_is_the_two_calls():
    from openintel_amd import batch
    n, K, t = 2400, 4, 0.95
    rows, centres, which = _planted(64, K, n, 22, copies=True)
    ctx = _ctx()
    idx = _with_signals(_index(ctx, rows), n)
    _, lab = idx.similar_share(centres, 0.35, labels=True)
    texts = ["post %d" % i for i in range(n)]
    pool = 48
    lists = idx.label_exemplars(lab, centres, top=pool)
    for top in (5, pool):
        res = idx.collapse_lists(lists.cos_scores, lists.cos_docs, lists.cos_counts, threshold=t, k=top)
        got = batch.narrative_exemplars(idx, lab, centroids=centres, top=top, pool=pool, collapse=t, texts=texts)
        assert len(got) == K
        for q in range(K):
            m = int(res.counts[q])
            assert [(g[0], np.float32(g[1]).tobytes(), g[2], g[3]) for g in got[q]] == \
                   [(int(res.docs[q, i]), res.scores[q, i].tobytes(), int(res.dup_counts[q, i]), texts[int(res.docs[q, i])]) for i in range(m)]
            kept = np.array([g[0] for g in got[q]])
            gram = rows[kept].astype(np.float64) @ rows[kept].astype(np.float64).T
            np.fill_diagonal(gram, 0.0)
            assert (gram < t).all()                                   # the kept docs are pairwise below t
            if top == pool:
                assert sum(g[2] for g in got[q]) == int(lists.cos_counts[q]) == pool       # stands_for sums to the pool count
                assert max(g[2] for g in got[q]) > 1                  # copies were folded
    plain = batch.narrative_exemplars(idx, lab, centroids=centres, top=5)
    five = _got(idx.label_exemplars(lab, centres, top=5))
    for q in range(K):
        assert [(g[0], np.float32(g[1]).tobytes(), g[2], g[3]) for g in plain[q]] == \
               [(int(five[1][q, i]), five[0][q, i].tobytes(), 1, None) for i in range(int(five[2][q]))]


def test_two_shards_merge_to_the_whole_index():
    from openintel_amd import retriever
    n = 2 * RANGE + 600
    rows, centres, which = _exact(64, n, rs=17)
    lab = _labels(which, 5, rs=17)
    cents = _cents(centres, 5)
    ctx = _ctx()
    whole = _got(_index(ctx, rows).label_exemplars(lab, cents, top=40))
    h = n // 2
    a = _got(_index(ctx, rows[:h]).label_exemplars(lab[:h], cents, top=40))
    b = _got(_index(ctx, rows[h:], base=h).label_exemplars(lab[h:], cents, top=40))
    so, do, co = retriever.merge_lists(ctx, np.stack([a[0], b[0]]), np.stack([a[1], b[1]]), np.stack([a[2], b[2]]))
    assert co.tolist() == whole[2].tolist()
    for q in range(5):
        m = int(co[q])
        assert do[q, :m].tolist() == whole[1][q, :m].tolist() and so[q, :m].tobytes() == whole[0][q, :m].tobytes()


# ------------------------------------------------------------------ end to end
def test_discover_then_quote_four_planted_directions():
    from openintel_amd import batch
    n, dim, K, t = 4096, 64, 4, 0.35
    rows, centres, which = _planted(dim, K, n, 23)
    ctx = _ctx()
    idx = _with_signals(_index(ctx, rows), n)
    fit, _ = batch.discover_narratives(idx, K, t, max_iters=8, trials=4, seed=2, labels=True)
    ex = batch.narrative_exemplars(idx, fit, top=5)
    lab = _host(fit.labels, np.uint32)
    cent = _host(fit.centroids, np.float32).reshape(K, dim)
    nearest = np.argmax(cent.astype(np.float64) @ centres.astype(np.float64).T, axis=1)
    assert sorted(nearest.tolist()) == [0, 1, 2, 3]                   # one narrative per planted direction
    for q in range(K):
        assert len(ex[q]) == 5
        for doc, score, stands_for, text in ex[q]:
            assert lab[doc] == q and which[doc] == nearest[q] and stands_for == 1 and text is None
