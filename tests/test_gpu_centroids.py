"""The update step of narrative discovery (oi_label_sums, oi_centroids_from_sums).  The references are numpy in
this file: np.add.at over rint(clip(x with NaN -> 0, -1, 1) * 2^30) as int64 for the sums -- compared as exact integers -- and
the sequential f64 loop of the header for the centroids, compared as the 32 bits of every f32.  Shapes are the smallest at
which the kernel can go wrong: one below, at and one above a wave step, a wave block, a workgroup trip, a row range and a dim
slice."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
# centroids.hip's shape constants (tests/test_centroids_abi.py holds them against the file): floats per dim slice, rows per wave
# step, rows per wave block, rows per workgroup trip, rows per range
SLICE, STEP, BLOCK, WG_STEP, RANGE = 64, 4, 64, 1024, 2048
NO_LABEL = 0xFFFFFFFF


def _ctx():
    import openintel_amd as oi
    return oi.HipContext(0)


def _index(ctx, rows, bf16=False, finalize=False):
    import openintel_amd as oi
    n, dim = rows.shape
    idx = oi.HybridIndex(ctx, n, dim, 8)
    if bf16:
        idx.set_embeddings_bf16(rows)
    else:
        idx.set_embeddings(rows, normalize=False)
    if finalize:
        idx.set_forward(np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64))
        idx.finalize()
    return idx


def _unit_rows(n, dim, seed):
    x = np.random.default_rng(seed).standard_normal((n, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _labels(n, K, seed, unlabelled=0.25):
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, K, size=n).astype(np.uint32)
    lab[rng.random(n) < unlabelled] = NO_LABEL
    return lab


def _fix(x):
    v = np.clip(np.where(np.isnan(x), 0.0, x), -1.0, 1.0).astype(np.float64)
    return np.rint(v * 2.0 ** 30).astype(np.int64)


def _ref(rows, labels, K):
    sums = np.zeros((K, rows.shape[1]), np.int64)
    ok = labels < K
    np.add.at(sums, labels[ok], _fix(rows[ok]))
    return sums, np.bincount(labels[ok], minlength=K).astype(np.uint64)


def _same(got, ref):
    sums, counts = got
    if hasattr(sums, "data_ptr"):
        sums, counts = sums.cpu().numpy(), counts.cpu().numpy().view(np.uint64)
    assert sums.dtype == np.int64 and counts.dtype == np.uint64 and sums.shape == ref[0].shape and counts.shape == ref[1].shape
    bad = np.argwhere(sums != ref[0])
    assert bad.size == 0, (bad[:4], sums[tuple(bad[0])], ref[0][tuple(bad[0])])
    assert (counts == ref[1]).all(), (counts, ref[1])


@pytest.mark.parametrize("n", [1, STEP - 1, STEP, STEP + 1, 4 * STEP - 1, 4 * STEP, 4 * STEP + 1, BLOCK - 1, BLOCK, BLOCK + 1, WG_STEP - 1, WG_STEP, WG_STEP + 1, RANGE - 1, RANGE, RANGE + 1, 2 * RANGE + 1])
def test_row_count_edges(n):
    ctx = _ctx()
    dim, K = SLICE + 4, 5
    rows, lab = _unit_rows(n, dim, n), _labels(n, K, n)
    lab[n - 1] = n % K                                              # the last row always counts
    idx = _index(ctx, rows)
    _same(idx.label_sums(lab, K), _ref(rows, lab, K))


@pytest.mark.parametrize("dim", [4, SLICE - 4, SLICE, SLICE + 4, 384, 768, 1024])
def test_dim_edges(dim):
    ctx = _ctx()
    n, K = WG_STEP + 45, 3
    rows, lab = _unit_rows(n, dim, dim), _labels(n, K, dim)
    idx = _index(ctx, rows)
    ref = _ref(rows, lab, K)
    assert (ref[0][:, dim - 1] != 0).all()                          # the last element of the last slice is in play
    _same(idx.label_sums(lab, K), ref)


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 157, 158, 255, 256])
def test_cluster_count_edges(K):
    """(157 / 158: the last count at which two workgroups share a CU's LDS, and the first at which one has it alone)"""
    ctx = _ctx()
    n, dim = 3 * WG_STEP + 7, SLICE + 4
    rows, lab = _unit_rows(n, dim, K), _labels(n, K, K)
    lab[:2] = (K - 1, 0)                                            # the first and the last cluster are in play
    idx = _index(ctx, rows)
    ref = _ref(rows, lab, K)
    assert ref[1][0] > 0 and ref[1][K - 1] > 0
    _same(idx.label_sums(lab, K), ref)


def test_nobody_labelled_everybody_under_one_label_and_labels_that_mean_no_cluster():
    ctx = _ctx()
    n, dim, K = RANGE + WG_STEP + 3, 2 * SLICE + 4, 7
    rows = _unit_rows(n, dim, 1)
    idx = _index(ctx, rows)
    sums, counts = idx.label_sums(np.full(n, NO_LABEL, np.uint32), K)
    assert not sums.any() and not counts.any() and sums.shape == (K, dim) and counts.shape == (K,)
    one = np.full(n, 4, np.uint32)                                  # maximum contention: every add lands on one accumulator row
    ref = _ref(rows, one, K)
    assert ref[1][4] == n
    _same(idx.label_sums(one, K), ref)
    lab = _labels(n, K, 2, unlabelled=0.0)
    lab[0::3] = K
    lab[1::7] = K + 1
    lab[2::11] = 0xFFFFFFFE
    ref = _ref(rows, lab, K)
    assert 0 < int(ref[1].sum()) < n - n // 3
    _same(idx.label_sums(lab, K), ref)


def test_the_four_rows_of_a_wave_step():
    """A step is four LABELLED rows of a 64-row block, in row order: four different labels, four equal ones (added in registers
    first), pairs, equal runs with a hole or a foreign label inside, and blocks with fewer than four labelled rows."""
    ctx = _ctx()
    dim, K = SLICE + 4, 6
    steps = [(0, 1, 2, 3), (5, 5, 5, 5), (2, 2, 4, 4), (3, NO_LABEL, 3, 3), (NO_LABEL,) * 4, (1, 1, 1, K), (4, 4, 4, 4), (0, 5, 0, 5)]
    lab = np.array([l for s in steps * 36 for l in s], np.uint32)   # 1152 rows: more than one workgroup trip
    lab[BLOCK:2 * BLOCK] = NO_LABEL                                  # a block with nobody, then blocks with 1, 3 and 5 labelled rows
    lab[2 * BLOCK + 7] = 2
    lab[3 * BLOCK:4 * BLOCK] = NO_LABEL
    lab[3 * BLOCK + np.array([0, 31, 63])] = (1, 1, 4)
    lab[4 * BLOCK:5 * BLOCK] = NO_LABEL
    lab[4 * BLOCK + np.array([5, 6, 7, 8, 60])] = 3
    lab[5 * BLOCK:6 * BLOCK] = 5                                     # a block under one label: sixteen equal steps
    n = lab.size
    rows = _unit_rows(n, dim, 3)
    idx = _index(ctx, rows)
    _same(idx.label_sums(lab, K), _ref(rows, lab, K))


def test_values_at_the_edges_of_fix():
    ctx = _ctx()
    inf = np.inf
    vals = np.array([-1.0, 1.0, 2.0 ** -31, -2.0 ** -31, 3 * 2.0 ** -31, 1.5, -1.5, inf, -inf, np.nan, -0.0, 0.0, 0.3, -0.7,
                     1.0 - 2.0 ** -24, 2.0 ** -30], np.float32)
    n, dim, K = WG_STEP + 9, SLICE + 4, 3
    rng = np.random.default_rng(4)
    rows = vals[rng.integers(0, vals.size, size=(n, dim))]
    rows[0, :vals.size] = vals                                       # every value at least once
    lab = _labels(n, K, 4)
    lab[0] = 1
    idx = _index(ctx, rows)
    assert _fix(vals).tolist()[:12] == [-2 ** 30, 2 ** 30, 0, 0, 2, 2 ** 30, -2 ** 30, 2 ** 30, -2 ** 30, 0, 0, 0]
    _same(idx.label_sums(lab, K), _ref(rows, lab, K))


def test_a_sum_that_crosses_2_to_the_32():
    ctx = _ctx()
    n, dim, K = 2 * RANGE + 9, 8, 2
    rows = np.ones((n, dim), np.float32)
    lab = (np.arange(n) % 2).astype(np.uint32)
    rows[lab == 1] = -1.0
    idx = _index(ctx, rows)
    sums, counts = idx.label_sums(lab, K)
    ref = _ref(rows, lab, K)
    assert ref[0][0, 0] == (n + 1) // 2 * 2 ** 30 > 2 ** 40 and ref[0][1, 0] == -(n // 2) * 2 ** 30
    _same((sums, counts), ref)


@pytest.mark.parametrize("dim", [384, 1024])
def test_bf16_corpus(dim):
    ctx = _ctx()
    n, K = WG_STEP + 77, 4
    bits = (_unit_rows(n, dim, dim + 1).view(np.uint32) >> 16).astype(np.uint16)
    wide = (bits.astype(np.uint32) << 16).view(np.float32)
    lab = _labels(n, K, dim + 1)
    idx = _index(ctx, bits, bf16=True)
    _same(idx.label_sums(lab, K), _ref(wide, lab, K))


def test_more_ranges_than_workgroups():
    """dim 4 is one slice: every resident workgroup walks several ranges before it flushes"""
    ctx = _ctx()
    n, dim, K = 1100 * RANGE + 1, 4, 3
    rows, lab = _unit_rows(n, dim, 5), _labels(n, K, 5)
    idx = _index(ctx, rows)
    _same(idx.label_sums(lab, K), _ref(rows, lab, K))


def test_locations_a_view_repeat_calls_and_the_workspace():
    import torch
    ctx = _ctx()
    n, dim, K = RANGE + 100, 384, 9
    rows, lab = _unit_rows(n, dim, 6), _labels(n, K, 6)
    idx = _index(ctx, rows, finalize=True)
    ref = _ref(rows, lab, K)
    dlab = torch.from_numpy(lab.view(np.int32)).cuda()
    before = ctx.workspace_bytes()[0]
    dev = idx.label_sums(dlab, K)
    ctx.synchronize()
    assert dev[0].is_cuda and dev[1].is_cuda and dev[0].dtype == torch.int64
    assert ctx.workspace_bytes()[0] == before                       # the device location needs no workspace
    _same(dev, ref)
    again = idx.label_sums(dlab, K)
    ctx.synchronize()
    assert torch.equal(dev[0], again[0]) and torch.equal(dev[1], again[1])
    host = idx.label_sums(lab, K)
    _same(host, ref)
    after = ctx.workspace_bytes()[0]
    assert before + 4 * n + 8 * K * dim + 8 * K <= after <= before + 4 * n + 8 * K * dim + 8 * K + 512   # the host location's staging
    assert host[0].tobytes() == idx.label_sums(lab, K)[0].tobytes()
    ctx_v = _ctx()
    view = idx.view(ctx_v)
    _same(view.label_sums(lab, K), ref)
    ctx.profile_reset(True)
    idx.label_sums(lab, K)
    assert ctx.profile_read("label_sums")[1] == 1
    ctx.profile_reset(False)
    view.close()


# ------------------------------------------------------------------ sums -> unit vectors
def _centroids_ref(sums, counts, previous):
    v = sums.astype(np.float64) * 2.0 ** -30
    acc = np.zeros(sums.shape[0], np.float64)
    for k in range(sums.shape[1]):                                  # ascending k, one rounded multiply and one rounded add each
        acc = acc + v[:, k] * v[:, k]
    keep = (counts == 0) | (acc == 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = (v / np.sqrt(acc)[:, None]).astype(np.float32)
    out[keep] = previous[keep] if previous is not None else 0.0
    return out


def _same_bits(got, ref):
    if hasattr(got, "data_ptr"):
        got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:4], got[tuple(bad[0])], ref[tuple(bad[0])])


def _sums_case(K, dim, seed):
    rng = np.random.default_rng(seed)
    sums = np.rint(rng.standard_normal((K, dim)) * rng.integers(1, 2 ** 34, size=(K, 1))).astype(np.int64)
    counts = rng.integers(1, 1000, size=K).astype(np.uint64)
    return sums, counts


@pytest.mark.parametrize("K,dim", [(1, 4), (5, 68), (64, 384), (256, 1024), (7, 768)])
def test_centroids_are_the_f64_loop_bit_for_bit(K, dim):
    from openintel_amd.retriever import centroids_from_sums
    ctx = _ctx()
    sums, counts = _sums_case(K, dim, K + dim)
    _same_bits(centroids_from_sums(ctx, sums, counts), _centroids_ref(sums, counts, None))


def test_centroids_of_real_label_sums():
    from openintel_amd.retriever import centroids_from_sums
    ctx = _ctx()
    n, dim, K = 3000, 384, 6
    rows, lab = _unit_rows(n, dim, 8), _labels(n, K, 8)
    idx = _index(ctx, rows)
    sums, counts = idx.label_sums(lab, K)
    got = centroids_from_sums(ctx, sums, counts)
    _same_bits(got, _centroids_ref(sums, counts, None))
    assert np.allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_empty_clusters_zero_sums_large_sums_and_the_aliasing_form():
    import torch
    from openintel_amd import _lib
    from openintel_amd.retriever import centroids_from_sums
    ctx = _ctx()
    K, dim = 9, 68
    sums, counts = _sums_case(K, dim, 9)
    counts[2] = 0                                                   # empty, with sums that must not be looked at
    sums[4] = 0                                                     # a non-zero count whose sum cancelled
    counts[6] = 0
    sums[6] = 0
    sums[7] = (2 ** 60 + 12345) * np.where(np.arange(dim) % 2 == 0, 1, -1) + np.arange(dim)    # |sum| above 2^53: the conversion rounds
    sums[8, :] = 0
    sums[8, 5] = -(2 ** 30)                                          # one element: the centroid is -e_5 exactly
    prev = _unit_rows(K, dim, 10)
    ref0, ref1 = _centroids_ref(sums, counts, None), _centroids_ref(sums, counts, prev)
    assert not ref0[[2, 4, 6]].any() and (ref1[[2, 4, 6]] == prev[[2, 4, 6]]).all() and ref0[8, 5] == -1.0
    _same_bits(centroids_from_sums(ctx, sums, counts), ref0)
    _same_bits(centroids_from_sums(ctx, sums, counts, prev), ref1)
    ds, dc, dp = torch.from_numpy(sums).cuda(), torch.from_numpy(counts.view(np.int64)).cuda(), torch.from_numpy(prev).cuda()
    got = centroids_from_sums(ctx, ds, dc, dp)
    ctx.synchronize()
    assert got.is_cuda
    _same_bits(got, ref1)
    _same_bits(centroids_from_sums(ctx, ds, dc), ref0)
    # centroids_out == previous, on the device
    _lib.check(ctx.lib.oi_centroids_from_sums(ctx.handle, _lib.ptr(ds), _lib.ptr(dc), _lib.ptr(dp), K, dim, _lib.OI_DEVICE, _lib.ptr(dp)))
    ctx.synchronize()
    _same_bits(dp, ref1)
    # ... and on the host
    alias = prev.copy()
    _lib.check(ctx.lib.oi_centroids_from_sums(ctx.handle, _lib.ptr(sums), _lib.ptr(counts), _lib.ptr(alias), K, dim, _lib.OI_HOST, _lib.ptr(alias)))
    _same_bits(alias, ref1)
