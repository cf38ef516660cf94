"""Narrative seeding (oi_narratives_seed): greedy k-means++ / farthest-first over the index on the device.  The
reference is the numpy emulation of the header's definition in this file: Python ints for the 128-bit product and every sum,
np.float32 for the one rounded subtract of the weight.

EXACT corpora: entries are small integers in [-2, 2] (one row in [-4, 4]) times 2^-k with 4^k >= dim, loaded with
normalize=False.  Every product is a multiple of 4^-k, every dot product at most 8, so each sum is exact in f32 in any order,
1 - s is exact, and the weight is an integer without rounding: rows, seeds, found, eligible and potential must equal the
emulation BIT FOR BIT.  Float corpora are checked by their properties and against f64 within the library's 1e-5 contract."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RANGE = 2048                      # NS_RANGE_ROWS of seeds.hip (tests/test_seed_abi.py compares)
NO_ROW = 0xFFFFFFFF
M64 = (1 << 64) - 1
KMEANSPP, FARTHEST = "kmeans++", "farthest"


def _ctx(mode=None):
    import openintel_amd as oi
    c = oi.HipContext(0)
    if mode is not None:
        c.set_cosine_mode(mode)
    return c


# ------------------------------------------------------------------ the definition, in numpy
def _splitmix(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def _u(seed, i, t):
    return _splitmix((seed + (8 * i + t + 1) * 0x9E3779B97F4A7C15) & M64)


def _mulhi(u, w):
    return (u * w) >> 64


def _weight(s):
    """s: f32 similarities -> integer weights (int64)"""
    s = np.asarray(s, np.float32)
    with np.errstate(invalid="ignore"):
        x = np.float32(1.0) - s                                      # one rounded f32 subtract
        x = np.minimum(np.maximum(x, np.float32(0.0)), np.float32(2.0))
        w = np.rint(x * np.float32(2.0 ** 20))
    w[np.isnan(s)] = 0.0
    return w.astype(np.int64)


def _sims(rows64, p):
    with np.errstate(invalid="ignore", over="ignore"):
        return (rows64 @ rows64[p]).astype(np.float32)               # (exact corpora: the f32 chain's value in any order)


def _emulate(rows, K, method=KMEANSPP, trials=4, seed=0, elig=None):
    """rows: the stored values as f32.  -> dict(rows, seeds, found, eligible, potential, cands: the candidates of every step)"""
    n, dim = rows.shape
    rows64 = rows.astype(np.float64)
    elig = np.ones(n, bool) if elig is None else elig
    out_rows = np.full(K, NO_ROW, np.uint32)
    out_seeds = np.zeros((K, dim), np.float32)
    E = int(elig.sum())
    res = dict(rows=out_rows, seeds=out_seeds, found=0, eligible=E, potential=0, cands=[])
    if E == 0:
        return res

    def wc_of(c):
        wc = _weight(_sims(rows64, c))
        wc[~elig] = 0
        wc[c] = 0
        return wc

    p = int(np.flatnonzero(elig)[_mulhi(_u(seed, 0, 0), E)])
    w = wc_of(p)
    out_rows[0], out_seeds[0] = p, rows[p]
    res["cands"].append([p])
    found = 1
    W = int(w.sum())
    for i in range(1, K):
        if W == 0:
            break
        if method == FARTHEST:
            cands = [int(np.argmax(w))]                               # the largest w, ties to the smallest row
        else:
            cs = np.cumsum(w.astype(np.uint64))
            cands = [int(np.searchsorted(cs, np.uint64(_mulhi(_u(seed, i, t), W)), side="right")) for t in range(trials)]
        res["cands"].append(cands)
        best = None
        for c in cands:
            nw = np.minimum(w, wc_of(c))
            pot = int(nw.sum())
            if best is None or pot < best[0]:                         # ties to the smallest t
                best = (pot, c, nw)
        W, p, w = best
        out_rows[i], out_seeds[i] = p, rows[p]
        found = i + 1
    res.update(found=found, potential=W)
    return res


# ------------------------------------------------------------------ data
def _k_of(dim):
    k = 0
    while 4 ** k < dim:
        k += 1
    return k


@functools.lru_cache(maxsize=None)
def _exact(dim, n, C=4, rs=0, k=None, noise=0.1, specials=True, flip=0.1):
    """Planted clusters of small integers times 2^-k: centres in {-2, 2}^dim, a member re-draws a tenth of its entries from
    [-2, 2], `noise` of the rows are uniform in [-2, 2].  specials (n >= 8): one row times 2 (its similarities to its cluster
    reach 1 and more: the weight clamps at 0), one times -2 (1 - s >= 2: the clamp at 2^21), one NaN row.
    -> (rows f32, which: the planted cluster per row, -1 for noise and the special rows)"""
    k = _k_of(dim) if k is None else k
    assert 4 ** k >= dim
    rng = np.random.default_rng(100 + rs)
    centres = rng.choice(np.array([-2, 2]), size=(C, dim))
    which = rng.integers(0, C, size=n)
    rows = centres[which].astype(np.int64)
    f = rng.random((n, dim)) < flip
    rows[f] = rng.integers(-2, 3, size=int(f.sum()))
    nz = rng.random(n) < noise
    rows[nz] = rng.integers(-2, 3, size=(int(nz.sum()), dim))
    which = np.where(nz, -1, which)
    rows = rows.astype(np.float32)
    if specials and n >= 8:
        a, b, c = (int(x) for x in rng.choice(n, size=3, replace=False))
        rows[a] *= 2.0
        rows[b] *= -2.0
        rows[c, :] = 0.0
        rows[c, int(rng.integers(0, dim))] = np.nan
        which[[a, b, c]] = -1
    return (rows * np.float32(2.0 ** -k)).astype(np.float32), which


def _index(ctx, rows, bf16=False, attrs=None, finalize=False, copy_policy=None, device=False):
    import openintel_amd as oi
    n, dim = rows.shape
    idx = oi.HybridIndex(ctx, n, dim, 8)
    if copy_policy is not None:
        idx.set_screen_copy(copy_policy)
    if bf16:
        bits = rows.view(np.uint32)
        assert not (bits & 0xFFFF).any()                              # the values are bf16 values
        idx.set_embeddings_bf16((bits >> 16).astype(np.uint16))
    elif device:
        import torch
        idx.set_embeddings(torch.from_numpy(rows).cuda(), normalize=False)
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


def _check(got, ref, what=""):
    """every output against the emulation, bit for bit"""
    rows, seeds = _host(got.rows, np.uint32), _host(got.seeds, np.float32)
    print(what, "found", got.found, ref["found"], "eligible", got.eligible, ref["eligible"], "potential", got.potential, ref["potential"],
          "rows", rows[:8], ref["rows"][:8])
    assert (got.found, got.eligible, got.potential) == (ref["found"], ref["eligible"], ref["potential"]), what
    assert rows.tolist() == ref["rows"].tolist(), what
    assert seeds.shape == ref["seeds"].shape and seeds.tobytes() == ref["seeds"].tobytes(), what


def _run(rows, K, ctx=None, bf16=False, **kw):
    ctx = ctx or _ctx()
    idx = _index(ctx, rows, bf16=bf16)
    got = idx.seed_narratives(K, **kw)
    ref = _emulate(rows, K, kw.get("method", KMEANSPP), kw.get("trials", 4), kw.get("seed", 0))
    _check(got, ref, "n=%d dim=%d K=%d %r" % (rows.shape + (K, kw)))
    return idx, got, ref


# ------------------------------------------------------------------ exact corpora: sizes, dims, trials, cluster counts
@pytest.mark.parametrize("n", [1, 63, 2047, 2048, 2049, 4097])
def test_sizes_around_the_block_and_range_edges(n):
    rows, _ = _exact(64, n)
    for trials in (1, 2):
        _run(rows, 2 if n == 1 else 5, trials=trials, seed=n)


def test_more_ranges_than_workgroups():
    """the score pass launches at most 4 workgroups per CU, one range at a time each: 1024 on 256 CUs -- these rows are 1030 ranges"""
    n = RANGE * 1029 + 77
    rows, _ = _exact(16, n, rs=3)
    _run(rows, 3, trials=2, seed=5)


@pytest.mark.parametrize("dim", [16, 64, 384, 768, 1024])
def test_dims_one_per_row_width(dim):
    rows, _ = _exact(dim, 2500, rs=dim)
    for trials in (1, 8):
        _run(rows, 6, trials=trials, seed=dim)
    _run(rows, 6, method=FARTHEST, trials=1, seed=1)


def test_bf16_corpus():
    rows, _ = _exact(384, 3000, rs=1)
    for trials in (1, 2, 8):
        _run(rows, 6, bf16=True, trials=trials, seed=3)
    _run(rows, 4, bf16=True, method=FARTHEST, trials=1)


@pytest.mark.parametrize("trials", [1, 2, 3, 4, 5, 8])
def test_trials(trials):
    rows, _ = _exact(64, 4097, C=6, rs=2)
    _, got, ref = _run(rows, 8, trials=trials, seed=11)
    assert got.found == 8 and len(set(_host(got.rows, np.uint32).tolist())) == 8          # distinct rows
    if trials > 1:
        assert any(len(set(c)) > 1 for c in ref["cands"][1:])                              # the argmin had a choice


@pytest.mark.parametrize("K", [1, 2, 65, 256])
def test_cluster_counts(K):
    rows, _ = _exact(64, 3000, C=8, rs=4)
    _, got, _ = _run(rows, K, trials=2, seed=K)
    assert got.found == K


def test_farthest_first_with_many_tied_maxima():
    """twelve distinct vectors, 40 copies each: after every seed the largest weight is shared by whole groups of rows"""
    rng = np.random.default_rng(9)
    base = (rng.integers(-2, 3, size=(12, 64)) * 2.0 ** -3).astype(np.float32)
    rows = np.repeat(base, 40, axis=0)[rng.permutation(480)]
    _, got, ref = _run(rows, 6, method=FARTHEST, trials=1, seed=2)
    w = _weight(_sims(rows.astype(np.float64), int(ref["rows"][0])))
    assert int((w == w.max()).sum()) >= 40
    assert got.found == 6


def test_three_distinct_vectors_run_out_of_weight():
    """self-similarity >= 1: a copy of a seed has weight 0, so after three seeds nothing is left"""
    base = (np.array([[2, 2, 2, 2] * 4, [2, -2, 2, -2] * 4, [-2, -2, 2, 2] * 4]) * 2.0 ** -2).astype(np.float32)
    assert ((base.astype(np.float64) ** 2).sum(axis=1) >= 1.0).all()
    rows = np.repeat(base, 20, axis=0)[np.random.default_rng(1).permutation(60)]
    for kw in (dict(trials=4), dict(trials=1), dict(method=FARTHEST, trials=1)):
        _, got, ref = _run(rows, 8, seed=6, **kw)
        assert (ref["found"], ref["potential"]) == (3, 0)
        assert (_host(got.rows, np.uint32)[3:] == NO_ROW).all() and not _host(got.seeds, np.float32)[3:].any()


def test_a_nan_seed_0_ends_the_call_with_one_seed():
    rows, _ = _exact(64, 100, specials=False)
    rows = rows.copy()
    rng_seed = 0
    p0 = _mulhi(_u(rng_seed, 0, 0), 100)
    rows[p0, 5] = np.nan
    _, got, ref = _run(rows, 4, trials=2, seed=rng_seed)
    assert (got.found, got.potential, int(_host(got.rows, np.uint32)[0])) == (1, 0, p0)


# ------------------------------------------------------------------ eligibility
def _time_axis(n, lo, hi):
    """stamp = 1000 + row and buckets of 97 stamps from row lo on: the time axis keeps rows [lo, hi'), hi' the end of the last bucket"""
    stamp = (1000 + np.arange(n)).astype(np.uint32)
    nb = -(-(hi - lo) // 97)
    return stamp, dict(stamp_origin=1000 + lo, bucket_width=97, n_buckets=nb), min(n, lo + nb * 97)


def test_filter_and_buckets_with_an_eligible_span_inside_the_ranges():
    n = 3 * RANGE + 500
    rows, _ = _exact(64, n, C=5, rs=6)
    lo = 1000
    stamp, axis, hi = _time_axis(n, lo, 5500)
    group = (np.arange(n) % 4).astype(np.uint32)
    filt = (0x3, 0x1, 1000 + 1100, 1000 + 5400)                       # group 1 of 4, and a stamp window inside the buckets
    elig = (np.arange(n) >= 1100) & (np.arange(n) <= 5400) & (np.arange(n) >= lo) & (np.arange(n) < hi) & (group == 1)
    ctx = _ctx()
    idx = _index(ctx, rows, attrs=(group, stamp))
    for kw in (dict(trials=1), dict(trials=4), dict(method=FARTHEST, trials=1)):
        got = idx.seed_narratives(5, seed=8, filter=filt, **axis, **kw)
        ref = _emulate(rows, 5, kw.get("method", KMEANSPP), kw["trials"], 8, elig)
        _check(got, ref, repr(kw))
        assert elig[_host(got.rows, np.uint32)[:got.found]].all() and got.eligible == int(elig.sum()) < n // 3
    # buckets alone: the span starts and ends mid-range
    elig = (np.arange(n) >= lo) & (np.arange(n) < hi)
    _check(idx.seed_narratives(4, trials=2, seed=1, **axis), _emulate(rows, 4, KMEANSPP, 2, 1, elig), "buckets")
    # a filter alone
    elig = group == 1
    _check(idx.seed_narratives(4, trials=2, seed=1, filter=(0x3, 0x1, 0, 0xFFFFFFFF)), _emulate(rows, 4, KMEANSPP, 2, 1, elig), "filter")


def test_a_whole_range_ineligible_and_no_eligible_row():
    n = 3 * RANGE + 9
    rows, _ = _exact(64, n, rs=7)
    stamp = np.arange(n).astype(np.uint32)
    stamp[RANGE:2 * RANGE] = 0xFFFFFFF0                               # the second range has no bucket
    elig = stamp < 3 * RANGE + 9
    ctx = _ctx()
    idx = _index(ctx, rows, attrs=(None, stamp))
    axis = dict(stamp_origin=0, bucket_width=RANGE, n_buckets=4)
    for trials in (1, 3):
        _check(idx.seed_narratives(6, trials=trials, seed=4, **axis), _emulate(rows, 6, KMEANSPP, trials, 4, elig), "range")
    none = idx.seed_narratives(3, trials=2, filter=(0xFFFFFFFF, 0xDEAD, 0, 0xFFFFFFFF))
    assert (none.found, none.eligible, none.potential) == (0, 0, 0)
    assert (none.rows == NO_ROW).all() and not none.seeds.any()
    # rows with a stamp below the origin have no bucket either
    elig = (stamp >= 100) & ((stamp.astype(np.int64) - 100) // 50 < 7)
    _check(idx.seed_narratives(3, trials=2, stamp_origin=100, bucket_width=50, n_buckets=7), _emulate(rows, 3, KMEANSPP, 2, 0, elig), "origin")
    no_attrs = _index(ctx, rows)
    from openintel_amd import _lib
    with pytest.raises(_lib.OiError) as e:
        no_attrs.seed_narratives(3, **axis)
    assert e.value.code == _lib.OI_ERR_STATE
    _check(no_attrs.seed_narratives(3, trials=2), _emulate(rows, 3, KMEANSPP, 2, 0), "no attributes needed")


# ------------------------------------------------------------------ locations, views, determinism, workspace, modes
def test_device_location_without_info_a_view_and_determinism():
    import ctypes as C
    import torch
    from openintel_amd import _lib
    rows, _ = _exact(64, 4097, C=5, rs=8)
    ref = _emulate(rows, 5, KMEANSPP, 4, 3)
    ctx = _ctx()
    idx = _index(ctx, rows, finalize=True)
    dev = idx.seed_narratives(5, trials=4, seed=3, device=True)
    assert dev.seeds.is_cuda and dev.rows.is_cuda
    _check(dev, ref, "device")
    # info_host = NULL: fully asynchronous; the outputs are there after a synchronise
    seeds = torch.full((5, 64), 7.0, dtype=torch.float32, device="cuda")
    out_rows = torch.zeros(5, dtype=torch.int32, device="cuda")
    spec = _lib.SeedSpec(_lib.OI_SEED_KMEANSPP, 4, 3, 0, 0, 1, 0)
    _lib.check(idx.lib.oi_narratives_seed(idx.handle, 5, C.byref(spec), None, _lib.OI_DEVICE, _lib.ptr(seeds), _lib.ptr(out_rows), None))
    ctx.synchronize()
    assert _host(out_rows, np.uint32).tolist() == ref["rows"].tolist() and _host(seeds, np.float32).tobytes() == ref["seeds"].tobytes()
    # rows_out = NULL
    seeds2 = np.zeros((5, 64), np.float32)
    info = _lib.SeedInfo()
    _lib.check(idx.lib.oi_narratives_seed(idx.handle, 5, C.byref(spec), None, _lib.OI_HOST, _lib.ptr(seeds2), None, C.byref(info)))
    assert seeds2.tobytes() == ref["seeds"].tobytes() and (info.found, info.reserved, info.eligible, info.potential) == (5, 0, 4097, ref["potential"])
    # the same call twice: the same bytes; another RNG seed: other rows
    again = idx.seed_narratives(5, trials=4, seed=3)
    assert again.rows.tobytes() == _host(dev.rows, np.uint32).tobytes() and again.seeds.tobytes() == ref["seeds"].tobytes()
    other = idx.seed_narratives(5, trials=4, seed=4)
    _check(other, _emulate(rows, 5, KMEANSPP, 4, 4), "seed 4")
    assert other.rows.tolist() != again.rows.tolist()
    # a view, on a context of its own
    ctx_v = _ctx()
    view = idx.view(ctx_v)
    _check(view.seed_narratives(5, trials=4, seed=3), ref, "view")
    view.close()


@pytest.mark.parametrize("method,trials", [(KMEANSPP, 1), (KMEANSPP, 4), (FARTHEST, 1)])
def test_workspace_bytes_grow_by_the_documented_amount(method, trials):
    n, dim = 5000, 64
    rows, _ = _exact(dim, n, rs=9)
    ctx = _ctx()
    idx = _index(ctx, rows)
    before = ctx.workspace_bytes()[0]
    idx.seed_narratives(3, method=method, trials=trials, device=True)
    ctx.synchronize()

    def up(b):
        return (b + 255) & ~255

    n_ranges = -(-n // RANGE)
    want = 256 + up(4 * n) + (up(4 * trials * n) if trials > 1 else 0) + up(8 * trials * n_ranges) + up(4 * trials * dim)
    if method == FARTHEST:
        want += up(8 * n_ranges)
    assert ctx.workspace_bytes()[0] - before == want


def test_cosine_mode_and_copy_policy_change_nothing():
    from openintel_amd import _lib
    import openintel_amd as oi
    rows, _ = _exact(384, 3000, rs=10)
    ref = _emulate(rows, 5, KMEANSPP, 4, 2)
    for mode, policy in ((None, None), (_lib.OI_COSINE_EXACT, None), (None, oi.HybridIndex.SCREEN_COPY_NEVER),
                         (_lib.OI_COSINE_SCREEN_COPY, oi.HybridIndex.SCREEN_COPY_ALWAYS)):
        ctx = _ctx(mode)
        idx = _index(ctx, rows, finalize=True, copy_policy=policy)
        _check(idx.seed_narratives(5, trials=4, seed=2), ref, "mode %r policy %r" % (mode, policy))


# ------------------------------------------------------------------ quality: a condition on the reference, then equality
@pytest.mark.parametrize("dim,C,n,k", [(64, 5, 2100, 4), (768, 6, 2049, 6)])
def test_greedy_seeding_lands_one_seed_in_every_planted_cluster(dim, C, n, k):
    rows, which = _exact(dim, n, C=C, rs=21, k=k, specials=False)
    ctx = _ctx()
    idx = _index(ctx, rows)
    for trials in (4, 8):
        ref = _emulate(rows, C, KMEANSPP, trials, 0)
        hit = which[ref["rows"]]
        print(dim, trials, "clusters of the seeds", hit)
        assert sorted(hit.tolist()) == list(range(C)), (trials, hit)      # of the emulation alone
        _check(idx.seed_narratives(C, trials=trials, seed=0), ref, "quality")


# ------------------------------------------------------------------ float planted data: properties and the 1e-5 contract
def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def _planted(dim, C, n, seed):
    """planted unit centres, noise sigma * sqrt(dim) = 0.45, a fifth of the rows pure noise (tests/test_gpu_narratives.py's data)"""
    rng = np.random.default_rng(seed)
    centres = _unit(rng.standard_normal((C, dim)))
    which = rng.integers(0, C, size=n)
    rows = centres[which] + rng.standard_normal((n, dim)) * (0.45 / np.sqrt(dim))
    noise = rng.random(n) < 0.2
    rows[noise] = rng.standard_normal((int(noise.sum()), dim))
    return _unit(rows).astype(np.float32)


@pytest.mark.parametrize("dim", [64, 768])
def test_float_rows_properties_and_the_potential_within_the_contract(dim):
    n, K = 3000, 6
    rows = _planted(dim, 6, n, 5)
    group = (np.arange(n) % 3).astype(np.uint32)
    elig = group != 2
    ctx = _ctx()
    idx = _index(ctx, rows, attrs=(group, None))
    # (group & 2) == 0 keeps groups 0 and 1
    got = idx.seed_narratives(K, trials=4, seed=1, filter=(0x2, 0x0, 0, 0xFFFFFFFF))
    r = got.rows.astype(np.int64)
    E = int(elig.sum())
    assert got.found == K and got.eligible == E
    assert len(set(r.tolist())) == K and elig[r].all()                                   # distinct eligible rows
    assert got.seeds.tobytes() == rows[r].tobytes()                                      # the stored rows, bit for bit
    s = rows.astype(np.float64) @ rows[r].astype(np.float64).T                           # f64, from the GPU's own rows
    w64 = np.rint(np.clip(1.0 - s, 0.0, 2.0) * 2.0 ** 20)
    w64[r, np.arange(K)] = 0.0
    pot64 = int(w64.min(axis=1)[elig].sum())
    bound = E * (2.0 ** 20 * 1e-5 + 1)
    print(dim, "potential", got.potential, "f64", pot64, "diff", got.potential - pot64, "bound", bound)
    assert abs(got.potential - pot64) <= bound


@pytest.mark.parametrize("dim,device_rows", [(64, False), (768, False), (64, True)])
def test_discover_narratives_with_a_seed_count(dim, device_rows):
    from openintel_amd import batch
    n, K, t = 3000, 6, 0.35
    rows = _planted(dim, 6, n, 6)
    rng = np.random.default_rng(3)
    ctx = _ctx()
    idx = _index(ctx, rows, device=device_rows)
    idx.set_signals(rng.uniform(-1, 1, n), rng.integers(0, 2, n).astype(np.uint8), rng.integers(0, 2, n).astype(np.uint8), 0.2)
    kw = dict(trials=4, seed=2)
    fit, sov = batch.discover_narratives(idx, K, t, max_iters=8, **kw)
    seeds = idx.seed_narratives(K, device=device_rows, **kw)
    assert seeds.found == K
    want = idx.fit_narratives(seeds.seeds, t, max_iters=8)
    from openintel_amd.analyzer import COUNTERS_DTYPE
    if device_rows:
        assert fit.centroids.is_cuda                                                     # the seeds never left the device
    assert _host(fit.centroids, np.float32).tobytes() == _host(want.centroids, np.float32).tobytes()
    assert _host(fit.records, np.uint8).tobytes() == _host(want.records, np.uint8).tobytes()
    assert (fit.iterations, fit.converged, fit.moved, fit.assigned) == (want.iterations, want.converged, want.moved, want.assigned)
    assert len(sov) == K and fit.assigned > n // 2                                       # seeds in the clusters: most rows are assigned
    # the share with the fitted centroids reproduces the fit
    rec, _ = idx.similar_share(fit.centroids, t, labels=True)
    ctx.synchronize()
    assert _host(rec, np.uint8).tobytes() == _host(fit.records, np.uint8).tobytes()
    # the array form is unchanged
    fit2, _ = batch.discover_narratives(idx, seeds.seeds, t, max_iters=8)
    assert _host(fit2.centroids, np.float32).tobytes() == _host(want.centroids, np.float32).tobytes()


# ------------------------------------------------------------------ argument errors: refused before any device call
def test_argument_errors_name_the_number_and_launch_nothing():
    import ctypes as C
    from openintel_amd import _lib
    rows, _ = _exact(64, 300)
    ctx = _ctx()
    idx = _index(ctx, rows)
    seeds = np.zeros((256, 64), np.float32)
    ctx.profile_reset(True)

    def call(K=4, method=0, trials=2, nb=1, width=0, reserved=0, spec=True, out=seeds, handle=idx.handle):
        sp = C.byref(_lib.SeedSpec(method, trials, 0, 0, width, nb, reserved)) if spec else None
        return idx.lib.oi_narratives_seed(handle, K, sp, None, _lib.OI_HOST, _lib.ptr(out), None, None)

    for kw, word in ((dict(K=0), b"n_clusters=0"), (dict(K=257), b"n_clusters=257"), (dict(method=2), b"method=2"),
                     (dict(trials=0), b"trials=0"), (dict(trials=9), b"trials=9"), (dict(method=1, trials=2), b"trials=2"),
                     (dict(reserved=5), b"reserved=5"), (dict(nb=0), b"n_buckets=0"), (dict(nb=1025, width=1), b"n_buckets=1025"),
                     (dict(nb=2), b"n_buckets=2"), (dict(spec=False), b"null spec"), (dict(out=None), b"null buffer"),
                     (dict(handle=None), b"null index")):
        rc = call(**kw)
        msg = idx.lib.oi_last_error()
        assert rc == _lib.OI_ERR_INVALID_ARG and word in msg, (kw, rc, msg)
    for tag in ("seed_init", "seed_score", "seed_pick"):
        assert ctx.profile_read(tag)[1] == 0, tag
    assert call() == 0                                                                   # and a good call records all three
    ran = {t: ctx.profile_read(t)[1] for t in ("seed_init", "seed_score", "seed_pick")}
    ctx.profile_reset(False)
    assert ran == {"seed_init": 1, "seed_score": 4, "seed_pick": 5}, ran


def test_host_location_without_rows_and_info_is_the_device_location_bit_for_bit():
    """300 rows (a ragged last block of 64), dim 64, 3 clusters: OI_HOST gives OI_DEVICE's bytes, and with rows_out and
    info_host both NULL the seeds are as they were."""
    import ctypes as C
    from openintel_amd import _lib
    rows, _ = _exact(64, 300, C=3, rs=12)
    ctx = _ctx()
    idx = _index(ctx, rows)
    full = idx.seed_narratives(3, trials=2, seed=5)
    dev = idx.seed_narratives(3, trials=2, seed=5, device=True)
    ctx.synchronize()
    _check(full, _emulate(rows, 3, KMEANSPP, 2, 5), "host")
    assert _host(dev.seeds, np.float32).tobytes() == full.seeds.tobytes() and _host(dev.rows, np.uint32).tobytes() == full.rows.tobytes()
    assert (dev.found, dev.eligible, dev.potential) == (full.found, full.eligible, full.potential) and full.found == 3
    spec = _lib.SeedSpec(_lib.OI_SEED_KMEANSPP, 2, 5, 0, 0, 1, 0)
    seeds = np.full((3, 64), 7.0, np.float32)
    _lib.check(idx.lib.oi_narratives_seed(idx.handle, 3, C.byref(spec), None, _lib.OI_HOST, _lib.ptr(seeds), None, None))
    assert seeds.tobytes() == full.seeds.tobytes()
