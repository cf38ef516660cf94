"""Narrative discovery (oi_narratives_fit): k-means over the index on the device.  The reference is an f64
emulation of the loop in this file: per step s = rows @ centroids^T in f64 (on a bf16 corpus the centroids are first rounded
to bf16 the way that corpus's scorer rounds its queries), candidates s >= t, the winner the largest with ties to the smallest
cluster, then the integer sums and the sequential f64 centroid loop of the header.  The library's similarities are within 1e-5
of f64, so the generator keeps every decision of every step away from a tie: it drops each row for which any |s - t|, or the
gap between the best and the second-best candidate, is below 1e-4 in any step, and repeats until no row is dropped.  On such
data the labels must be EQUAL, and with them the sums, centroids, records, iterations, converged, moved and assigned: bit
for bit."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NO_LABEL = 0xFFFFFFFF
TAU = 0.2
T = 0.35
MAX_ITERS = 12
MARGIN = 1e-4
VALS = np.array([-1.0, -0.5, -1.0 / 3.0, -0.2, 0.0, 0.2, 0.25, 1.0 / 3.0, 1.0, np.nan, 1.5, -7.0])
FILTER = (0x3, 0x1, 100, 5000)
BUCKETS = dict(n_buckets=6, stamp_origin=500, bucket_width=700)


def _dtype():
    from openintel_amd.analyzer import COUNTERS_DTYPE
    return COUNTERS_DTYPE


def _ctx(mode=None):
    import openintel_amd as oi
    c = oi.HipContext(0)
    if mode is not None:
        c.set_cosine_mode(mode)
    return c


# ------------------------------------------------------------------ the definition, in numpy
def _bf16_round(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def _fix(x):
    v = np.clip(np.where(np.isnan(x), 0.0, x), -1.0, 1.0).astype(np.float64)
    return np.rint(v * 2.0 ** 30).astype(np.int64)


def _label_sums(rows, labels, K):
    sums = np.zeros((K, rows.shape[1]), np.int64)
    ok = labels < K
    np.add.at(sums, labels[ok], _fix(rows[ok]))
    return sums, np.bincount(labels[ok], minlength=K).astype(np.uint64)


def _centroids(sums, counts, previous):
    v = sums.astype(np.float64) * 2.0 ** -30
    acc = np.zeros(sums.shape[0], np.float64)
    for k in range(sums.shape[1]):
        acc = acc + v[:, k] * v[:, k]
    keep = (counts == 0) | (acc == 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (v / np.sqrt(acc)[:, None]).astype(np.float32)
    out[keep] = previous[keep]
    return out


def _emulate(rows, seeds, t, max_iters, bf16=False, eligible=None):
    """rows: the stored values as f32 (a bf16 corpus widened).  eligible: rows that pass the filter and have a bucket (None:
    all).  -> dict of the last step's centroids / labels / iterations / converged / moved / assigned, `risky` (rows with a
    decision closer than MARGIN to a tie in any step) and `history` (the centroids and labels of every step)."""
    n, K = rows.shape[0], seeds.shape[0]
    rows64 = rows.astype(np.float64)
    elig = np.ones(n, bool) if eligible is None else eligible
    c = np.ascontiguousarray(seeds, np.float32).copy()
    prev = np.full(n, NO_LABEL, np.uint32)
    risky = np.zeros(n, bool)
    history = []
    i = 0
    while True:
        i += 1
        cq = _bf16_round(c) if bf16 else c
        s = rows64 @ cq.astype(np.float64).T
        cand = s >= t
        for j in range(1, K):                                        # a repeat of an earlier vector never wins: ties go to the smallest
            if any(c[j].tobytes() == c[e].tobytes() for e in range(j)):
                cand[:, j] = False
        best = np.where(cand, s, -np.inf)
        labels = np.where(cand.any(axis=1) & elig, np.argmax(best, axis=1), NO_LABEL).astype(np.uint32)
        close = np.abs(s - t).min(axis=1) < MARGIN
        if K > 1:
            top = np.sort(best, axis=1)[:, -2:]
            with np.errstate(invalid="ignore"):
                close |= (top[:, 1] - top[:, 0]) < MARGIN            # (-inf second: inf or NaN, never below)
        risky |= close & elig
        moved = int((labels != prev).sum())
        history.append((c.copy(), labels))
        converged = i > 1 and moved == 0
        if converged or i == max_iters:
            break
        c = _centroids(*_label_sums(rows, labels, K), c)
        prev = labels
    return dict(centroids=c, labels=labels, iterations=i, converged=converged, moved=moved, assigned=int((labels != NO_LABEL).sum()),
                risky=risky, history=history)


# ------------------------------------------------------------------ data
def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _planted(dim, K, n, seed, spread=0.45, extra_seeds=0, duplicate=False):
    """Planted unit centres, noise sigma * sqrt(dim) = spread, a fifth of the rows pure noise; deliberately bad seeds: two near
    centre 0 (the second leaning towards centre 1, whose cloud it takes), the others between centres, and the last one so far
    from its centre that only half of its cloud reaches the threshold in the first step -- the rest joins in the second, and
    the third finds nothing left to move.  extra_seeds: vectors far from every cloud (they stay empty); duplicate: one more
    seed, a copy of seed 1."""
    rng = np.random.default_rng(seed)
    centres = _unit(rng.standard_normal((K, dim)))
    which = rng.integers(0, K, size=n)
    rows = centres[which] + rng.standard_normal((n, dim)) * (spread / np.sqrt(dim))
    noise = rng.random(n) < 0.2
    rows[noise] = rng.standard_normal((int(noise.sum()), dim))
    rows = _unit(rows).astype(np.float32)
    seeds = [centres[0] + 0.25 * _unit(rng.standard_normal(dim)), centres[0] + 0.7 * centres[1]]
    for j in range(2, K - 1):
        seeds.append(0.5 * centres[j - 1] + centres[j])
    c, w = centres[K - 1], rng.standard_normal(dim)
    w = _unit(w - (w @ c) * c)
    cloud = rows[(which == K - 1) & ~noise].astype(np.float64)
    lo, hi = 0.0, 2.0                                                # bisection: half of the cloud reaches T in the first step
    for _ in range(30):
        a = 0.5 * (lo + hi)
        if ((cloud @ _unit(a * c + w)) >= T).mean() < 0.5:
            lo = a
        else:
            hi = a
    seeds.append(hi * c + w)
    for _ in range(extra_seeds):
        seeds.append(-centres[rng.integers(0, K)] + 0.3 * _unit(rng.standard_normal(dim)))
    seeds = _unit(np.array(seeds)).astype(np.float32)
    if duplicate:
        seeds = np.concatenate([seeds, seeds[1:2]])
    return rows, seeds


def _attrs(n, seed):
    rng = np.random.default_rng(7000 + seed)
    return rng.integers(0, 8, size=n).astype(np.uint32), rng.integers(0, 6000, size=n).astype(np.uint32)


def _eligible(group, stamp, filt, nb, origin, width):
    m, v, lo, hi = filt
    ok = ((group & np.uint32(m)) == np.uint32(v)) & (stamp >= lo) & (stamp <= hi)
    s64 = stamp.astype(np.int64)
    return ok & (s64 >= origin) & ((s64 - origin) // width < nb)


class _Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(dim, K, n, seed=0, bf16=False, extra_seeds=0, duplicate=False, filtered=False):
    """The generator: drop the rows whose decisions are too close to call, emulate again, until none is dropped."""
    rows, seeds = _planted(dim, K, n, seed, extra_seeds=extra_seeds, duplicate=duplicate)
    if bf16:
        rows = ((rows.view(np.uint32) >> 16) << 16).view(np.float32)    # the stored bf16 values, widened exactly
    group, stamp = _attrs(n, seed)
    rounds = 0
    while True:
        elig = _eligible(group, stamp, FILTER, BUCKETS["n_buckets"], BUCKETS["stamp_origin"], BUCKETS["bucket_width"]) if filtered else None
        ref = _emulate(rows, seeds, T, MAX_ITERS, bf16, elig)
        if not ref["risky"].any():
            break
        keep = ~ref["risky"]
        rows, group, stamp = rows[keep], group[keep], stamp[keep]
        rounds += 1
    c = _Case()
    c.rows, c.seeds, c.group, c.stamp, c.elig, c.ref, c.bf16, c.dropped, c.rounds = rows, seeds, group, stamp, elig, ref, bf16, n - rows.shape[0], rounds
    assert c.dropped <= 0.02 * n, (c.dropped, n)
    assert 3 <= ref["iterations"] < MAX_ITERS and ref["converged"], (ref["iterations"], ref["converged"])
    rng = np.random.default_rng(1000 + seed)
    m = rows.shape[0]
    c.pol = VALS[rng.integers(0, VALS.size, size=m)]
    c.spec, c.src = rng.integers(0, 2, size=m).astype(np.uint8), rng.integers(0, 2, size=m).astype(np.uint8)
    return c


def _records_of(case, labels, K, nb=1, origin=0, width=0):
    """the records that follow from labels: a row adds its signal to cell (label, bucket)"""
    v = np.where(np.isnan(case.pol), 0.0, np.clip(case.pol, -1.0, 1.0))
    q30 = np.rint(v * 2.0 ** 30).astype(np.int64)
    bull, bear = v > TAU, v < -TAU
    b = (case.stamp.astype(np.int64) - origin) // width if width else np.zeros(labels.size, np.int64)
    out = np.zeros((K, nb), _dtype())

    def count(m):
        return np.bincount(b[m], minlength=nb)[:nb]

    for q in range(K):
        ok = labels == q
        out["total"][q] = count(ok)
        out["by_source"][q, :, 1] = count(ok & (case.src != 0))
        out["by_source"][q, :, 0] = out["total"][q] - out["by_source"][q, :, 1]
        out["bullish"][q], out["bearish"][q], out["neutral"][q] = count(ok & bull), count(ok & bear), count(ok & ~bull & ~bear)
        out["spec_count"][q] = count(ok & (case.spec != 0))
        s = np.zeros(nb, np.int64)
        np.add.at(s, b[ok], q30[ok])
        out["polarity_sum"][q] = [float(int(x)) * 2.0 ** -30 for x in s]
    return out


def _index(ctx, case, finalize=False, attrs=False):
    import openintel_amd as oi
    n, dim = case.rows.shape
    idx = oi.HybridIndex(ctx, n, dim, 8)
    if case.bf16:
        idx.set_embeddings_bf16((case.rows.view(np.uint32) >> 16).astype(np.uint16))
    else:
        idx.set_embeddings(case.rows, normalize=False)
    if attrs:
        idx.set_doc_attrs(case.group, case.stamp)
    idx.set_signals(case.pol, case.spec, case.src, TAU)
    if finalize:
        idx.set_forward(np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64))
        idx.finalize()
    return idx


def _host(x, dtype=None):
    if hasattr(x, "data_ptr"):
        x = x.cpu().numpy()
        if dtype is not None:
            x = x.view(dtype).reshape(x.shape[0], x.shape[1]) if dtype is _dtype() else x.view(dtype)
    return x


def _check_fit(fit, ref, case, K, **axis):
    """every field of the fit against the emulation, bit for bit"""
    lab = _host(fit.labels, np.uint32)
    bad = np.flatnonzero(lab != ref["labels"])
    assert bad.size == 0, (bad[:8], lab[bad[:8]], ref["labels"][bad[:8]])
    assert (fit.iterations, fit.converged, fit.moved, fit.assigned) == (ref["iterations"], ref["converged"], ref["moved"], ref["assigned"])
    cent = _host(fit.centroids)
    assert cent.dtype == np.float32 and cent.tobytes() == ref["centroids"].tobytes()
    rec = _host(fit.records, _dtype())
    want = _records_of(case, ref["labels"], K, axis.get("n_buckets", 1), axis.get("stamp_origin", 0), axis.get("bucket_width", 0))
    assert rec.shape == want.shape and rec.tobytes() == want.tobytes()


def _check_share_reproduces(idx, fit, **kw):
    """the contract a host relies on: the share with the fitted centroids gives the fit's records and labels"""
    K = int(fit.centroids.shape[0])
    if "filter" in kw:
        kw["filters"] = np.array([kw.pop("filter")] * K, np.uint32)
    rec, lab = idx.similar_share(fit.centroids, T, labels=True, **kw)
    idx.ctx.synchronize()
    assert _host(rec, _dtype()).tobytes() == _host(fit.records, _dtype()).tobytes()
    assert _host(lab, np.uint32).tobytes() == _host(fit.labels, np.uint32).tobytes()


def _check_update_step(idx, seeds, i, **kw):
    """centroids_from_sums(label_sums(labels_i), previous = c_i) is c_{i+1}: max_iters = i against i + 1"""
    from openintel_amd.retriever import centroids_from_sums
    K = seeds.shape[0]
    a = idx.fit_narratives(seeds, T, max_iters=i, labels=True, **kw)
    b = idx.fit_narratives(seeds, T, max_iters=i + 1, **kw)
    assert a.iterations == i and b.iterations == i + 1
    nxt = centroids_from_sums(idx.ctx, *idx.label_sums(a.labels, K), a.centroids)
    assert nxt.tobytes() == b.centroids.tobytes()


def _fit_and_check(ctx, case, finalize=False, attrs=False, **kw):
    idx = _index(ctx, case, finalize, attrs)
    K = case.seeds.shape[0]
    ctx.profile_reset(True)
    fit = idx.fit_narratives(case.seeds, T, max_iters=MAX_ITERS, labels=True, **kw)
    ran = {t: ctx.profile_read(t)[1] for t in ("share", "share_exact", "label_sums", "centroids", "fit_moved")}
    ctx.profile_reset(False)
    axis = {k: v for k, v in kw.items() if k != "filter"}
    _check_fit(fit, case.ref, case, K, **axis)
    assert ran["fit_moved"] == fit.iterations and ran["label_sums"] == ran["centroids"] == fit.iterations - 1, ran
    _check_share_reproduces(idx, fit, **dict(kw))
    return idx, fit, ran


# ------------------------------------------------------------------ the cases
@pytest.mark.parametrize("dim,K,n", [(384, 4, 3000), (768, 3, 1500)])
def test_screened_corpus_stream_route_and_exact_route_agree(dim, K, n):
    from openintel_amd import _lib
    case = _case(dim, K, n)
    ctx = _ctx()
    idx, fit, ran = _fit_and_check(ctx, case, finalize=True)
    assert ran["share"] == fit.iterations and ran["share_exact"] == 0, ran          # <= 64 clusters on a screened corpus: the stream
    _check_update_step(idx, case.seeds, 1)
    _check_update_step(idx, case.seeds, 2)
    ctx_e = _ctx(_lib.OI_COSINE_EXACT)
    idx_e, fit_e, ran_e = _fit_and_check(ctx_e, case, finalize=True)
    assert ran_e["share"] == 0 and ran_e["share_exact"] == fit_e.iterations, ran_e
    assert fit_e.centroids.tobytes() == fit.centroids.tobytes() and fit_e.records.tobytes() == fit.records.tobytes()
    assert fit_e.labels.tobytes() == fit.labels.tobytes()


@pytest.mark.parametrize("dim,K,n", [(16, 5, 1000), (64, 4, 1500)])
def test_exact_route_dims(dim, K, n):
    case = _case(dim, K, n)
    ctx = _ctx()
    idx, fit, ran = _fit_and_check(ctx, case)
    assert ran["share"] == 0 and ran["share_exact"] == fit.iterations, ran
    _check_update_step(idx, case.seeds, 1)
    _check_update_step(idx, case.seeds, 2)


def test_bf16_corpus():
    case = _case(384, 4, 3000, bf16=True)
    ctx = _ctx()
    idx, fit, _ = _fit_and_check(ctx, case)
    _check_update_step(idx, case.seeds, 1)


def test_65_clusters():
    case = _case(128, 4, 2000, extra_seeds=61)
    assert case.seeds.shape[0] == 65
    ctx = _ctx()
    idx, fit, ran = _fit_and_check(ctx, case)
    assert ran["share_exact"] == fit.iterations, ran
    empty = np.flatnonzero(fit.records["total"][:, 0] == 0)
    assert empty.size >= 50 and fit.centroids[empty].tobytes() == case.seeds[empty].tobytes()     # an empty cluster keeps its vector


def test_max_iters_1_and_2():
    case = _case(64, 4, 1500)
    ctx = _ctx()
    idx = _index(ctx, case)
    for iters in (1, 2):
        ref = _emulate(case.rows, case.seeds, T, iters)
        fit = idx.fit_narratives(case.seeds, T, max_iters=iters, labels=True)
        _check_fit(fit, ref, case, 4)
        assert fit.iterations == iters and not fit.converged and fit.moved > 0
        _check_share_reproduces(idx, fit)
    one = idx.fit_narratives(case.seeds, T, max_iters=1)
    assert one.centroids.tobytes() == case.seeds.tobytes() and one.labels is None and one.moved == one.assigned


def test_a_duplicate_seed_stays_empty():
    case = _case(128, 4, 2000, duplicate=True)
    K = case.seeds.shape[0]
    assert K == 5 and case.seeds[4].tobytes() == case.seeds[1].tobytes()
    # (in the first step the tie rule keeps the copy empty; from the second on it competes, as the vector seed 1 was, with the
    # centroid that left it -- and on this data loses every row to it: the emulation says so before the device is asked)
    assert all(not (lab == 4).any() for _, lab in case.ref["history"])
    ctx = _ctx()
    idx, fit, _ = _fit_and_check(ctx, case)
    assert fit.records[4].tobytes() == bytes(64) and not (fit.labels == 4).any()
    assert fit.centroids[4].tobytes() == case.seeds[4].tobytes() and fit.centroids[1].tobytes() != case.seeds[1].tobytes()


def test_a_filter_together_with_time_buckets():
    case = _case(64, 4, 3000, filtered=True)
    ctx = _ctx()
    idx, fit, _ = _fit_and_check(ctx, case, attrs=True, filter=FILTER, **BUCKETS)
    assert 0 < fit.assigned < int(case.elig.sum()) + 1 and int(case.elig.sum()) < case.rows.shape[0] // 2
    assert (fit.records["total"].sum(axis=0) > 0).all()                                # every bucket is in play
    _check_update_step(idx, case.seeds, 1, filter=FILTER, **BUCKETS)


def test_device_location_and_a_view():
    import torch
    case = _case(64, 4, 1500)
    ctx = _ctx()
    idx = _index(ctx, case, finalize=True)
    dseeds = torch.from_numpy(case.seeds).cuda()
    fit = idx.fit_narratives(dseeds, T, max_iters=MAX_ITERS, labels=True)
    assert fit.centroids.is_cuda and fit.records.is_cuda and fit.labels.is_cuda and tuple(fit.records.shape) == (4, 1, 8)
    _check_fit(fit, case.ref, case, 4)
    _check_share_reproduces(idx, fit)
    before = ctx.workspace_bytes()[0]
    n, dim = case.rows.shape
    assert before >= 2 * 4 * n + 8 * 4 * dim + 2 * 4 * 4 * dim                        # label arrays, sums and centroid sets are counted
    ctx_v = _ctx()
    view = idx.view(ctx_v)
    _check_fit(view.fit_narratives(case.seeds, T, max_iters=MAX_ITERS, labels=True), case.ref, case, 4)
    view.close()


def test_discover_narratives_adds_the_share_of_voice():
    from openintel_amd import batch
    case = _case(64, 4, 1500)
    ctx = _ctx()
    idx = _index(ctx, case)
    fit, sov = batch.discover_narratives(idx, case.seeds, T, max_iters=MAX_ITERS)
    assert fit.converged and len(sov) == 4 and len(sov[0]) == 1
    assert [r[0].total for r in sov] == [int(x) for x in fit.records["total"][:, 0]]
    assert abs(sum(r[0].fraction for r in sov) - 1.0) < 1e-12
