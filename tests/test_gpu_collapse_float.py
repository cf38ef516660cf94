"""oi_search_collapsed on unit-norm float rows (d = 768): planted near-copies normalise(x + sigma * noise) at a few sigma.

The library's similarities are f32 (within 1e-5 of f64 for unit rows), so a pair within 1e-5 of the threshold may fall on
either side.  The test therefore first ASSERTS, on the CPU, that no pair of any query's pooled candidates has an f64
similarity within 1e-4 of t = 0.9 -- i.i.d. unit rows at d = 768 have similarities of sigma ~ 0.036, the planted copies sit
at >= 0.95 (sigma <= 0.2) or <= 0.86 (sigma = 0.6): the band is empty by construction -- and only then compares, bit for bit
and with no pair excluded, against the numpy greedy on those f64 values."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
VOCAB = 64
T, BAND = 0.9, 1e-4
SIGMAS = (0.05, 0.1, 0.2, 0.6)


def _corpus(n=20000, dim=768, families=40, per_sigma=6, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    free = rng.permutation(np.arange(families, n))
    at = 0
    for s in range(families):
        for sigma in SIGMAS:
            for _ in range(per_sigma):
                noise = rng.standard_normal(dim)
                noise -= (noise @ x[s]) * x[s]
                noise /= np.linalg.norm(noise)
                c = x[s] + sigma * noise
                x[free[at]] = c / np.linalg.norm(c)
                at += 1
    rows = x.astype(np.float32)     # the rows as the index stores them (normalize=False below)
    lens = rng.integers(1, 9, size=n)
    offs = np.zeros(n + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lens)
    terms = rng.integers(0, VOCAB, size=int(offs[-1])).astype(np.uint32)
    return rows, terms, offs


def _greedy(G, t, k):
    """the header's rule on one list, from its f64 similarity matrix -> (kept positions cut at k, their dup_counts)"""
    c = G.shape[0]
    hit = G >= t
    kept = np.zeros(c, dtype=bool)
    dup = np.zeros(c, dtype=np.int64)
    for i in range(c):
        m = hit[i, :i] & kept[:i]
        if m.any():
            dup[np.argmax(m)] += 1
        else:
            kept[i], dup[i] = True, 1
    ki = np.nonzero(kept)[0][:k]
    return ki, dup[ki]


def test_float_rows_collapse_bit_for_bit_when_no_pair_is_near_the_threshold():
    import openintel_amd as oi
    n, dim, B, depth, pool, k = 20000, 768, 8, 1000, 1000, 100
    rows, terms, offs = _corpus(n, dim)
    ctx = oi.HipContext(0)
    idx = oi.HybridIndex(ctx, n, dim, VOCAB, 0)
    idx.set_embeddings(rows, normalize=False)
    idx.set_forward(terms, offs)
    idx.finalize()
    rng = np.random.default_rng(6)
    q = rows[:B].copy()                                  # the sources of the first B families
    qt = rng.integers(0, VOCAB, size=3 * B).astype(np.uint32)
    qo = (3 * np.arange(B + 1)).astype(np.uint32)
    pooled = idx.search(q, qt, qo, k=pool, depth=depth)  # the trusted producer of the input lists
    got = idx.search_collapsed(q, qt, qo, k=k, depth=depth, pool=pool, threshold=T)
    r64 = rows.astype(np.float64)
    collapsed_any = False
    for b in range(B):
        c = int(pooled.counts[b])
        docs = pooled.docs[b][:c].astype(np.int64)
        G = r64[docs] @ r64[docs].T
        gap = np.abs(G - T).min()
        print("query %d: pool %d, closest pair to t: %.6f away" % (b, c, gap))
        assert gap > BAND, "the inputs are wrong: a pair of pooled candidates lies within %g of t" % BAND
        ki, dup = _greedy(G, T, k)
        m = int(got.counts[b])
        assert m == ki.size, (b, m, ki.size)
        assert np.array_equal(got.docs[b][:m], pooled.docs[b][ki]), b
        assert np.array_equal(got.dup_counts[b][:m], dup.astype(np.uint32)), b
        assert np.array_equal(got.scores[b][:m].view(np.uint32), pooled.scores[b][ki].view(np.uint32)), b
        collapsed_any |= bool((dup > 1).any())
        assert dup.sum() == c if ki.size < k else dup.sum() <= c
    assert collapsed_any, "the planted near-copies were in the pools and collapsed"
    idx.close()
    ctx.close()
