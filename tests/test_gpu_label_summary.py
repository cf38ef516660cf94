"""Narrative breakdown (oi_label_summary): cell (c, x) = the social_summary raw sums over the local rows d with
labels[d] == c < n_clusters that pass the filter and whose stamp (TIME axis) or group key (KEY axis) gives x; dense, or the best
`top` keys per cluster ranked on the device.  The reference is the header's definition restated in numpy in this file:
np.add.at per counter, Python integers for the polarity sum (float(int(sum of rint(v * 2^30))) * 2^-30), the ranking by Python
sort on (-v, key).  All eight record fields, the keys, the counts and `qualified` are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
BLOCK, RANGE, THREADS, LOCAL_CELLS = 64, 2048, 256, 1024       # LS_* of label_summary.hip (tests/test_label_summary_abi.py compares)
GRID_PER_CU = 4                                                # the launch uses at most this many workgroups per CU
NO = 0xFFFFFFFF
TAU = 0.2
VALS = np.array([-1.0, -0.5, -1.0 / 3.0, -0.2, 0.0, 0.2, 0.25, 1.0 / 3.0, 1.0, np.nan, 1.5, -7.0])
RANKS = ("total", "spec", "bullish", "bearish")
RANK_FIELD = {"total": "total", "spec": "spec_count", "bullish": "bullish", "bearish": "bearish"}


def _dtype():
    from openintel_amd.analyzer import COUNTERS_DTYPE
    return COUNTERS_DTYPE


def _ctx():
    import openintel_amd as oi
    return oi.HipContext(0)


class _Sig:
    """per-document signals as the caller gives them, and what the definition makes of them"""

    def __init__(self, pol, spec, src):
        self.pol, self.spec, self.src = pol, spec, src
        v = np.where(np.isnan(pol), 0.0, np.clip(pol, -1.0, 1.0))
        self.q30 = np.rint(v * 2.0 ** 30).astype(np.int64)
        self.bull, self.bear = v > TAU, v < -TAU
        self.neu = ~self.bull & ~self.bear
        self.sp = spec != 0
        self.s1 = src != 0


def _signals(n, seed, vals=VALS):
    rng = np.random.default_rng(1000 + seed)
    return _Sig(vals[rng.integers(0, vals.size, size=n)], rng.integers(0, 2, size=n).astype(np.uint8),
                rng.integers(0, 2, size=n).astype(np.uint8))


def _index(ctx, n, sig=None, group=None, stamp=None, rows=None, finalize=False):
    """attributes and signals only, unless rows are given"""
    import openintel_amd as oi
    idx = oi.HybridIndex(ctx, n, 16 if rows is None else rows.shape[1], 8)
    if rows is not None:
        idx.set_embeddings(rows, normalize=False)
    if group is not None or stamp is not None:
        idx.set_doc_attrs(group, stamp)
    if sig is not None:
        idx.set_signals(sig.pol, sig.spec, sig.src, TAU)
    if finalize:
        idx.set_forward(np.zeros(n, np.uint32), np.arange(n + 1, dtype=np.uint64))
        idx.finalize()
    return idx


def _labels(n, K, seed, p_none=0.2):
    """labels uniform in [0, K), a share of them "no cluster" in its several spellings"""
    rng = np.random.default_rng(3000 + seed)
    lab = rng.integers(0, K, size=n).astype(np.uint32)
    none = rng.random(n) < p_none
    lab[none] = np.array([NO, K, K + 1, 0x80000000], np.uint32)[rng.integers(0, 4, size=int(none.sum()))]
    return lab


def _passes(f, group, stamp):
    m, v, lo, hi = (int(x) for x in f)
    return ((group & np.uint32(m)) == np.uint32(v)) & (stamp >= np.uint32(lo)) & (stamp <= np.uint32(hi))


def _time_x(stamp, origin, width, nc):
    """clause 2 on the TIME axis, in 64 bits: (cell, has one)"""
    if width == 0:
        return np.zeros(stamp.size, np.int64), np.ones(stamp.size, bool)
    s = stamp.astype(np.int64)
    x = (s - origin) // width
    return x, (s >= origin) & (x < nc)


def _key_x(group, mask, nc):
    shift = (mask & -mask).bit_length() - 1
    x = ((group.astype(np.uint64) & np.uint64(mask)) >> np.uint64(shift)).astype(np.int64)
    return x, x < nc


def _ref(lab, K, sig, nc, x, ok, filt=None, group=None, stamp=None):
    """The definition, dense: [K][nc] records.  x / ok: the row's cell on the axis and whether it has one."""
    n = lab.size
    hit = (lab < K) & ok
    if filt is not None:
        hit &= _passes(filt, group, stamp)
    cell = lab[hit].astype(np.int64) * nc + x[hit]
    out = np.zeros(K * nc, _dtype())

    def count(m):
        c = np.zeros(K * nc, np.uint64)
        np.add.at(c, cell[m[hit]], 1)
        return c

    every = np.ones(n, bool)
    out["total"] = count(every)
    out["by_source"][:, 1] = count(sig.s1)
    out["by_source"][:, 0] = count(~sig.s1)
    out["bullish"], out["bearish"], out["neutral"] = count(sig.bull), count(sig.bear), count(sig.neu)
    out["spec_count"] = count(sig.sp)
    s = np.zeros(K * nc, np.int64)          # (|sum| <= n * 2^30: far inside 64 bits)
    np.add.at(s, cell, sig.q30[hit])
    out["polarity_sum"] = [float(int(v)) * 2.0 ** -30 for v in s]
    return out.reshape(K, nc)


def _ref_time(lab, K, sig, stamp, origin, width, nc, filt=None, group=None):
    st = stamp if stamp is not None else np.zeros(lab.size, np.uint32)
    x, ok = _time_x(st, origin, width, nc)
    return _ref(lab, K, sig, nc, x, ok, filt, group if group is not None else np.zeros(lab.size, np.uint32), st)


def _ref_key(lab, K, sig, group, mask, nc, filt=None, stamp=None):
    x, ok = _key_x(group, mask, nc)
    return _ref(lab, K, sig, nc, x, ok, filt, group, stamp if stamp is not None else np.zeros(lab.size, np.uint32))


def _rank(dense, top, by, min_total):
    """The ranking of dense records [K][nk] by Python sort on (-v, key): (keys, records, counts, qualified)."""
    K, nk = dense.shape
    keys = np.full((K, top), NO, np.uint32)
    recs = np.zeros((K, top), _dtype())
    counts, qual = np.zeros(K, np.uint32), np.zeros(K, np.uint32)
    bar = max(min_total, 1)
    for c in range(K):
        v = dense[RANK_FIELD[by]][c].tolist()
        listed = sorted(np.flatnonzero(dense["total"][c] >= bar).tolist(), key=lambda k: (-v[k], k))
        qual[c] = len(listed)
        listed = listed[:top]
        counts[c] = len(listed)
        keys[c, :len(listed)] = listed
        recs[c, :len(listed)] = dense[c, listed]
    return keys, recs, counts, qual


def _host(x):
    if hasattr(x, "data_ptr"):
        a = x.cpu().numpy()
        if a.dtype == np.int64:
            return a.view(_dtype()).reshape(a.shape[0], a.shape[1])
        return a.view(np.uint32)
    return x


def _same(got, ref):
    """all eight fields bit for bit (the f64 sum included: compared as its 64 bits)"""
    got = _host(got)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, got.shape, ref.shape)
    a, b = np.ascontiguousarray(got).view(np.uint64).reshape(-1, 8), np.ascontiguousarray(ref).view(np.uint64).reshape(-1, 8)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, (bad[:4], got.reshape(-1)[bad[:2]], ref.reshape(-1)[bad[:2]])


def _same_ranking(got, dense, top, by, min_total):
    keys, recs, counts, qual = _rank(dense, top, by, min_total)
    assert np.array_equal(_host(got.counts), counts), (by, top, min_total, _host(got.counts)[:4], counts[:4])
    assert np.array_equal(_host(got.qualified), qual), (by, top, min_total)
    assert np.array_equal(_host(got.keys), keys), (by, top, min_total)
    _same(got.records, recs)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")


def _groups(n, nk_drawn, mask, seed):
    """group words whose key under `mask` is uniform in [0, nk_drawn), with random bits everywhere outside the mask"""
    rng = np.random.default_rng(2000 + seed)
    shift = (mask & -mask).bit_length() - 1
    key = rng.integers(0, nk_drawn, size=n).astype(np.uint64)
    noise = rng.integers(0, 1 << 32, size=n, dtype=np.uint64) & np.uint64(~mask & 0xFFFFFFFF)
    return ((key << np.uint64(shift)) | noise).astype(np.uint32)


def _stamps(n, lo, hi, seed):
    return np.random.default_rng(4000 + seed).integers(lo, hi, size=n).astype(np.uint32)


# ------------------------------------------------------------------ 1. the row walk
@pytest.mark.parametrize("n", [1, BLOCK - 1, BLOCK, BLOCK + 1, RANGE - 1, RANGE, RANGE + 1, 3 * RANGE + 17])
def test_row_walk_edges_on_both_axes(n):
    K = 5
    sig, lab = _signals(n, n), _labels(n, K, n)
    lab[-1] = K - 1                                                  # the last row of the last, partial block counts
    group, stamp = _groups(n, 9, 0xFFF0, n), _stamps(n, 90, 100 + 3 * 50 + 20, n)
    idx = _index(_ctx(), n, sig, group, stamp)
    _same(idx.label_summary(lab, K, n_buckets=3, stamp_origin=100, bucket_width=50), _ref_time(lab, K, sig, stamp, 100, 50, 3))
    _same(idx.label_groups(lab, K, 0xFFF0, 8), _ref_key(lab, K, sig, group, 0xFFF0, 8))
    _same(idx.label_groups(lab, K, 0xFFF0, 300), _ref_key(lab, K, sig, group, 0xFFF0, 300))       # 1500 cells: the global route


def test_more_ranges_than_the_grid_so_the_stride_loop_turns():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = RANGE * (GRID_PER_CU * cus + 1) + 77                         # one range more than the largest grid, and a partial one
    K = 3
    rng = np.random.default_rng(5)
    sig = _signals(n, 5)
    lab = rng.integers(0, K + 1, size=n).astype(np.uint32)
    stamp = rng.integers(0, 4 * 10, size=n).astype(np.uint32)
    group = rng.integers(0, 700, size=n).astype(np.uint32)
    idx = _index(_ctx(), n, sig, group, stamp)
    _same(idx.label_summary(lab, K, n_buckets=4, stamp_origin=0, bucket_width=10), _ref_time(lab, K, sig, stamp, 0, 10, 4))
    _same(idx.label_groups(lab, K, 0xFFFF, 600), _ref_key(lab, K, sig, group, 0xFFFF, 600))     # the global route


# ------------------------------------------------------------------ 2. labels
@pytest.mark.parametrize("K", [1, 7, 256])
def test_label_edges_first_rows_and_cluster_counts(K):
    n = RANGE + 300
    sig, lab = _signals(n, K), _labels(n, K, K)
    lab[:5] = [K - 1, K, NO, 0, K + 1]
    stamp = _stamps(n, 0, 60, K)
    group = _groups(n, 6, 0x7, K)
    idx = _index(_ctx(), n, sig, group, stamp)
    ref = _ref_time(lab, K, sig, stamp, 0, 20, 3)
    _same(idx.label_summary(lab, K, n_buckets=3, stamp_origin=0, bucket_width=20), ref)
    assert ref["total"][K - 1].sum() >= 1 and ref["total"][0].sum() >= 1
    _same(idx.label_groups(lab, K, 0x7, 6), _ref_key(lab, K, sig, group, 0x7, 6))


def test_every_row_unassigned_gives_all_zero_records():
    n = 2 * RANGE + 5
    sig = _signals(n, 1)
    lab = np.array([NO, 4, 5, 0x80000000], np.uint32)[np.arange(n) % 4]
    group, stamp = _groups(n, 5, 0xF, 1), _stamps(n, 0, 100, 1)
    idx = _index(_ctx(), n, sig, group, stamp)
    for got in (idx.label_summary(lab, 4, n_buckets=10, stamp_origin=0, bucket_width=10), idx.label_groups(lab, 4, 0xF, 5),
                idx.label_groups(lab, 4, 0xFFFF, 500)):
        assert not np.ascontiguousarray(got).view(np.uint64).any()
    r = idx.label_groups(lab, 4, 0xF, 5, top=3)
    assert not r.counts.any() and not r.qualified.any() and (r.keys == NO).all() and not np.ascontiguousarray(r.records).view(np.uint64).any()


@pytest.mark.parametrize("K,nk", [(4, 3), (2, LOCAL_CELLS)])         # 12 cells: local; 2048 cells: global
def test_every_row_in_one_cluster_and_one_cell(K, nk):
    n = 3 * RANGE + 100
    sig = _signals(n, nk, vals=np.array([1.0, -1.0, 0.5, 0.0, np.nan]))
    lab = np.full(n, K - 1, np.uint32)
    group = np.full(n, (nk - 1) << 4 | 0x3, np.uint32)
    stamp = np.full(n, 77, np.uint32)
    idx = _index(_ctx(), n, sig, group, stamp)
    mask = (1 << 16) - 16
    ref = _ref_key(lab, K, sig, group, mask, nk)
    assert int(ref["total"][K - 1, nk - 1]) == n and int(ref["total"].sum()) == n
    _same(idx.label_groups(lab, K, mask, nk), ref)
    if K * nk <= LOCAL_CELLS:
        refs = _ref_time(lab, K, sig, stamp, 70, 5, nk)
        assert int(refs["total"][K - 1, 1]) == n
        _same(idx.label_summary(lab, K, n_buckets=nk, stamp_origin=70, bucket_width=5), refs)
    else:                                                            # the time axis on the global route: 256 x 8 cells
        refs = _ref_time(np.full(n, 255, np.uint32), 256, sig, stamp, 70, 1, 8)
        assert int(refs["total"][255, 7]) == n
        _same(idx.label_summary(np.full(n, 255, np.uint32), 256, n_buckets=8, stamp_origin=70, bucket_width=1), refs)


# ------------------------------------------------------------------ 3. the two routes
def test_route_edge_local_cells_and_one_more_agree():
    n = 2 * RANGE + 999
    K = 1
    sig, lab = _signals(n, 31), _labels(n, K, 31)
    group = _groups(n, LOCAL_CELLS + 1, 0x7FF, 31)
    group[:3] = [LOCAL_CELLS - 1, LOCAL_CELLS, LOCAL_CELLS + 1]
    lab[:3] = 0
    idx = _index(_ctx(), n, sig, group)
    local = idx.label_groups(lab, K, 0x7FF, LOCAL_CELLS)
    glob = idx.label_groups(lab, K, 0x7FF, LOCAL_CELLS + 1)
    _same(local, _ref_key(lab, K, sig, group, 0x7FF, LOCAL_CELLS))
    _same(glob, _ref_key(lab, K, sig, group, 0x7FF, LOCAL_CELLS + 1))
    _same(np.ascontiguousarray(glob[:, :LOCAL_CELLS]), np.ascontiguousarray(local))
    assert int(glob["total"][0, LOCAL_CELLS]) >= 1
    # the same edge with more than one cluster: 4 x 256 and 4 x 257 cells
    lab4 = _labels(n, 4, 32)
    _same(idx.label_groups(lab4, 4, 0x7FF, 256), _ref_key(lab4, 4, sig, group, 0x7FF, 256))
    _same(idx.label_groups(lab4, 4, 0x7FF, 257), _ref_key(lab4, 4, sig, group, 0x7FF, 257))


def test_the_cell_limit_sixteen_clusters_by_65536_keys():
    n = 20000
    K, nk = 16, 65536
    sig, lab = _signals(n, 41), _labels(n, K, 41)
    rng = np.random.default_rng(41)
    group = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    group[:4] = [0, 0xFFFF, 0xFFFF0000, 0xFFFFFFFF]
    group[4:2004] = 0x12345678                                        # a hot key: runs of one (cell, flag word)
    lab[4:2004] = 9
    idx = _index(_ctx(), n, sig, group)
    _same(idx.label_groups(lab, K, 0xFFFF, nk), _ref_key(lab, K, sig, group, 0xFFFF, nk))


# ------------------------------------------------------------------ 4. cell arithmetic
@pytest.mark.parametrize("nk", [8, LOCAL_CELLS + 8])                 # local and global route
def test_cell_arithmetic_flags_carries_signs_and_cancellation(nk):
    K = 2
    pol, spec, src, key, lab = [], [], [], [], []

    def rows(c, k, pols, sp=0, sr=0):
        for p in pols:
            pol.append(p), spec.append(sp), src.append(sr), key.append(k), lab.append(c)

    for sp in (0, 1):                                                 # all 12 flag combinations, in cell (0, 0)
        for sr in (0, 1):
            for p in (0.9, -0.9, 0.1):
                rows(0, 0, [p], sp, sr)
    rows(1, 1, [1.0] * 12)                                            # sum = 12 * 2^30 > 2^32
    rows(1, 2, [-1.0] * 9, sp=1)                                      # sum = -9 * 2^30: the sign through the flush
    rows(0, 3, [0.5, -0.5, 0.25, -0.25, 1.0, -1.0], sr=1)            # cancels to 0 with total 6
    rows(1, nk - 1, [0.0, np.nan, 0.0, -0.0])                         # only polarity-0 rows
    n = len(pol)
    sig = _Sig(np.array(pol), np.array(spec, np.uint8), np.array(src, np.uint8))
    lab = np.array(lab, np.uint32)
    group = (np.array(key, np.uint32) << np.uint32(8)) | np.uint32(0xAB)
    idx = _index(_ctx(), n, sig, group)
    ref = _ref_key(lab, K, sig, group, 0xFFFF00, nk)
    flags = {(bool(s), bool(r), int(b) - int(e)) for s, r, b, e in zip(sig.sp[:12], sig.s1[:12], sig.bull[:12], sig.bear[:12])}
    assert len(flags) == 12
    assert ref["polarity_sum"][1, 1] == 12.0 and ref["polarity_sum"][1, 2] == -9.0
    assert ref["polarity_sum"][0, 3] == 0.0 and int(ref["total"][0, 3]) == 6
    assert ref["polarity_sum"][1, nk - 1] == 0.0 and int(ref["neutral"][1, nk - 1]) == 4
    _same(idx.label_groups(lab, K, 0xFFFF00, nk), ref)


# ------------------------------------------------------------------ 5. the clauses
def test_time_axis_origin_last_bucket_and_wide_differences():
    n = RANGE + 77
    K = 3
    sig, lab = _signals(n, 51), _labels(n, K, 51)
    origin, width, nb = 1000, 7, 5
    stamp = _stamps(n, origin - 20, origin + width * nb + 20, 51)
    stamp[:6] = [origin - 1, origin, origin + width * nb - 1, origin + width * nb, 0, 0xFFFFFFFF]
    lab[:6] = [0, 1, 2, 0, 1, 2]
    idx = _index(_ctx(), n, sig, None, stamp)
    ref = _ref_time(lab, K, sig, stamp, origin, width, nb)
    assert int(ref["total"][2, nb - 1]) >= 1 and int(ref["total"].sum()) < int((lab < K).sum())
    _same(idx.label_summary(lab, K, n_buckets=nb, stamp_origin=origin, bucket_width=width), ref)
    # stamp - origin near 2^32 with width 1: far past the last bucket, or exactly the last bucket
    _same(idx.label_summary(lab, K, n_buckets=1024, stamp_origin=5, bucket_width=1), _ref_time(lab, K, sig, stamp, 5, 1, 1024))
    ref = _ref_time(lab, K, sig, stamp, 0xFFFFFC00, 1, 1024)
    assert int(ref["total"][2, 1023]) == 1
    _same(idx.label_summary(lab, K, n_buckets=1024, stamp_origin=0xFFFFFC00, bucket_width=1), ref)
    ref = _ref_time(lab, K, sig, stamp, 0, 0xFFFFFFFF, 2)             # the widest bucket: 0xFFFFFFFF is the first stamp of bucket 1
    assert int(ref["total"][2, 1]) == 1
    _same(idx.label_summary(lab, K, n_buckets=2, stamp_origin=0, bucket_width=0xFFFFFFFF), ref)


def test_no_time_axis_needs_no_attributes():
    n = RANGE + 5
    K = 6
    sig, lab = _signals(n, 52), _labels(n, K, 52)
    idx = _index(_ctx(), n, sig)                                      # signals only
    ref = _ref_time(lab, K, sig, None, 0, 0, 1)
    _same(idx.label_summary(lab, K), ref)
    _same(idx.label_summary(lab, K, stamp_origin=123), ref)           # (the origin means nothing without a width)


def test_key_axis_shifted_mask_and_the_last_key():
    n = RANGE + 9
    K, mask, nk = 4, 0x00FFFF00, 50
    sig, lab = _signals(n, 53), _labels(n, K, 53)
    group = _groups(n, nk + 3, mask, 53)
    group[:3] = [(nk - 1) << 8 | 0xFF0000FF, nk << 8 | 0x11, 0xFFFF << 8]
    lab[:3] = [1, 1, 1]
    idx = _index(_ctx(), n, sig, group)
    ref = _ref_key(lab, K, sig, group, mask, nk)
    assert int(ref["total"][1, nk - 1]) >= 1 and int(ref["total"].sum()) < int((lab < K).sum())
    _same(idx.label_groups(lab, K, mask, nk), ref)
    _same(idx.label_groups(lab, K, 0x80000000, 2), _ref_key(lab, K, sig, group, 0x80000000, 2))
    _same(idx.label_groups(lab, K, 0x1, 1), _ref_key(lab, K, sig, group, 0x1, 1))


@pytest.mark.parametrize("filt", [(0x3, 0x2, 0, NO), (0, 0, 1100, 1180), (0x3, 0x1, 1050, 1200), (0, 0, 7, 6), (0xF, 0xF0, 0, NO)])
def test_filter_alone_and_with_each_axis(filt):
    n = RANGE + 321
    K = 5
    sig, lab = _signals(n, 54), _labels(n, K, 54)
    group, stamp = _groups(n, 40, 0xFF0, 54), _stamps(n, 1000, 1300, 54)
    idx = _index(_ctx(), n, sig, group, stamp)
    ref = _ref_time(lab, K, sig, stamp, 0, 0, 1, filt, group)         # the filter alone: one cell
    if filt in ((0, 0, 7, 6), (0xF, 0xF0, 0, NO)):                    # a filter that passes nothing
        assert not ref["total"].any()
    else:
        assert 0 < int(ref["total"].sum()) < int((lab < K).sum())
    _same(idx.label_summary(lab, K, filter=filt), ref)
    _same(idx.label_summary(lab, K, n_buckets=6, stamp_origin=1010, bucket_width=40, filter=filt),
          _ref_time(lab, K, sig, stamp, 1010, 40, 6, filt, group))
    _same(idx.label_groups(lab, K, 0xFF0, 37, filter=np.array(filt, np.uint32)), _ref_key(lab, K, sig, group, 0xFF0, 37, filt, stamp))
    _same(idx.label_groups(lab, K, 0xFF0, 37, top=4, filter=filt).records, _rank(_ref_key(lab, K, sig, group, 0xFF0, 37, filt, stamp), 4, "total", 0)[1])


# ------------------------------------------------------------------ 6. ranked output
@pytest.fixture(scope="module")
def ranked_case():
    n = 3 * RANGE + 11
    K, mask, nk = 3, 0xFFF0, 40
    sig, lab = _signals(n, 61), _labels(n, K, 61)
    group = _groups(n, 30, mask, 61)                                  # keys 30 .. 39 stay empty
    group[:400] = (np.arange(400, dtype=np.uint32) % 4 + 30) << 4     # keys 30 .. 33 of cluster 0: 100 rows each, ties in total
    lab[:400] = 0
    idx = _index(_ctx(), n, sig, group)
    return idx, lab, K, mask, nk, _ref_key(lab, K, sig, group, mask, nk)


@pytest.mark.parametrize("by", RANKS)
@pytest.mark.parametrize("top,min_total", [(1, 0), (5, 0), (5, 60), (64, 60), (1024, 0)])
def test_ranked_output_orders_cuts_pads_and_counts(ranked_case, by, top, min_total):
    idx, lab, K, mask, nk, dense = ranked_case
    assert len({int(dense["total"][0, k]) for k in range(30, 34)}) == 1          # the ties
    got = idx.label_groups(lab, K, mask, nk, top=top, rank_by=by, min_total=min_total)
    _same_ranking(got, dense, top, by, min_total)
    if top >= nk:
        assert int(got.counts.max()) < top and (got.keys[:, -1] == NO).all()     # padded
    if min_total == 60 and top == 5:                                             # the bar is above some totals
        assert (got.qualified < nk).all() and int(got.qualified.min()) >= 1


def test_ranked_records_are_the_dense_records_at_the_listed_keys(ranked_case):
    idx, lab, K, mask, nk, ref = ranked_case
    dense = idx.label_groups(lab, K, mask, nk)
    _same(dense, ref)
    got = idx.label_groups(lab, K, mask, nk, top=7, rank_by="bearish", min_total=3)
    for c in range(K):
        m = int(got.counts[c])
        assert m == 7
        _same(np.ascontiguousarray(got.records[c:c + 1, :m]), np.ascontiguousarray(dense[c:c + 1, got.keys[c, :m].astype(np.int64)]))
    dev = idx.label_groups(_dev(lab), K, mask, nk, top=7, rank_by="bearish", min_total=3)          # the device location
    idx.ctx.synchronize()
    for a, b in ((dev.keys, got.keys), (dev.counts, got.counts), (dev.qualified, got.qualified)):
        assert np.array_equal(_host(a), b)
    _same(dev.records, got.records)


def test_ranked_output_out_of_lds_with_8193_keys_and_without_qualified():
    from openintel_amd import _lib
    n = 2 * RANGE + 50
    K, mask, nk, top = 3, 0xFFFF, 8193, 20
    sig, lab = _signals(n, 62), _labels(n, K, 62)
    rng = np.random.default_rng(62)
    group = (rng.integers(0, 90, size=n) ** 2 + rng.integers(0, 2, size=n) * 8192).astype(np.uint32)   # some keys hot, key 8192 the last, larger ones in no cell
    group[:3] = 8192
    lab[:3] = [0, 1, 2]
    idx = _index(_ctx(), n, sig, group)
    dense = _ref_key(lab, K, sig, group, mask, nk)
    assert int(dense["total"][:, 8192].min()) >= 1
    for by in ("total", "spec"):
        _same_ranking(idx.label_groups(lab, K, mask, nk, top=top, rank_by=by, min_total=2), dense, top, by, 2)
    # qualified_out = NULL, through the C entry point
    keys, recs, counts, _ = _rank(dense, top, "total", 0)
    spec = _lib.LabelSummarySpec(_lib.OI_LABEL_AXIS_KEY, mask, 0, nk, top, 0, 0, 0)
    g_rec, g_keys, g_counts = np.zeros((K, top), _dtype()), np.zeros((K, top), np.uint32), np.zeros(K, np.uint32)
    for loc in ("host", "device"):
        if loc == "host":
            args = (_lib.ptr(lab), _lib.OI_HOST, _lib.ptr(g_rec), _lib.ptr(g_keys), _lib.ptr(g_counts))
        else:
            import torch
            d_lab = _dev(lab)
            d_rec = torch.zeros((K, top, 8), dtype=torch.int64, device="cuda:0")
            d_keys, d_counts = torch.zeros((K, top), dtype=torch.int32, device="cuda:0"), torch.zeros((K,), dtype=torch.int32, device="cuda:0")
            args = (_lib.ptr(d_lab), _lib.OI_DEVICE, _lib.ptr(d_rec), _lib.ptr(d_keys), _lib.ptr(d_counts))
        _lib.check(idx.lib.oi_label_summary(idx.handle, args[0], K, C.byref(spec), None, args[1], args[2], args[3], args[4], None))
        if loc == "device":
            idx.ctx.synchronize()
            g_rec, g_keys, g_counts = _host(d_rec), _host(d_keys), _host(d_counts)
        assert np.array_equal(g_keys, keys) and np.array_equal(g_counts, counts)
        _same(g_rec, recs)


# ------------------------------------------------------------------ 7. identities
def _ints(n, dim, B, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-2, 3, size=(n, dim)).astype(np.float32), rng.integers(-2, 3, size=(B, dim)).astype(np.float32)


def test_totals_equal_label_sums_counts_and_keys_sum_to_the_one_cell_record():
    n = 2 * RANGE + 123
    K = 9
    rows, _ = _ints(n, 16, 1, 71)
    sig, lab = _signals(n, 71), _labels(n, K, 71)
    group, stamp = _groups(n, 33, 0x3F, 71), _stamps(n, 0, 50, 71)
    idx = _index(_ctx(), n, sig, group, stamp, rows=rows)
    one = idx.label_summary(lab, K)
    _, counts = idx.label_sums(lab, K)
    assert np.array_equal(one["total"][:, 0], counts)
    assert np.array_equal(idx.label_summary(lab, K, n_buckets=5, stamp_origin=0, bucket_width=10)["total"].sum(axis=1), counts)
    per_key = idx.label_groups(lab, K, 0x3F, 64)                     # every document has a key
    for f in ("total", "bullish", "bearish", "neutral", "spec_count"):
        assert np.array_equal(per_key[f].sum(axis=1), one[f][:, 0]), f
    assert np.array_equal(per_key["by_source"].sum(axis=1), one["by_source"][:, 0])
    q30 = np.rint(per_key["polarity_sum"] * 2.0 ** 30).astype(np.int64).sum(axis=1)       # (each cell's sum is an exact integer here)
    assert [float(int(v)) * 2.0 ** -30 for v in q30] == one["polarity_sum"][:, 0].tolist()


def test_share_and_fit_records_are_reproduced_from_their_labels():
    n = 2 * RANGE + 300
    B = 6
    rows, q = _ints(n, 16, B, 72)
    sig = _signals(n, 72)
    group, stamp = _groups(n, 8, 0x7, 72), _stamps(n, 480, 1100, 72)
    idx = _index(_ctx(), n, sig, group, stamp, rows=rows, finalize=True)
    filt = (0x1, 0x1, 500, 1050)
    axis = dict(n_buckets=5, stamp_origin=500, bucket_width=100)
    rec, lab = idx.similar_share(q, 3.0, filters=np.tile(np.array(filt, np.uint32), (B, 1)), labels=True, **axis)
    assert 0 < int(rec["total"].sum()) < n and int((lab < B).sum()) >= int(rec["total"].sum())
    _same(idx.label_summary(lab, B, filter=filt, **axis), rec)
    qn = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1.0)
    fit = idx.fit_narratives(qn.astype(np.float32), 0.5, max_iters=4, filter=filt, labels=True, **axis)
    assert int(fit.records["total"].sum()) > 0
    _same(idx.label_summary(fit.labels, B, filter=filt, **axis), fit.records)


# ------------------------------------------------------------------ 8. plumbing
def test_host_and_device_locations_views_updates_and_repeat_calls():
    import openintel_amd as oi
    n = RANGE + 200
    K = 4
    rows, _ = _ints(n, 16, 1, 81)
    sig, lab = _signals(n, 81), _labels(n, K, 81)
    group, stamp = _groups(n, 20, 0xFFFF, 81), _stamps(n, 0, 100, 81)
    idx = _index(_ctx(), n, sig, group, stamp, rows=rows, finalize=True)
    ref_t, ref_k = _ref_time(lab, K, sig, stamp, 0, 25, 4), _ref_key(lab, K, sig, group, 0xFFFF, 1500)
    d_lab = _dev(lab)
    for _ in range(2):                                                # twice: the workspace cells are cleared by every call
        _same(idx.label_summary(lab, K, n_buckets=4, bucket_width=25), ref_t)
        _same(idx.label_groups(lab, K, 0xFFFF, 1500), ref_k)
        got_t, got_k = idx.label_summary(d_lab, K, n_buckets=4, bucket_width=25), idx.label_groups(d_lab, K, 0xFFFF, 1500)
        idx.ctx.synchronize()
        _same(got_t, ref_t)
        _same(got_k, ref_k)
    ws = idx.ctx.workspace_bytes()[0]
    assert ws >= 64 * K * 1500 + 4 * n                                # "label_summary" and "label_summary_io" are counted
    view = idx.view(oi.HipContext(0))
    _same(view.label_summary(lab, K, n_buckets=4, bucket_width=25), ref_t)
    sig2 = _signals(n, 82)
    idx.set_signals(sig2.pol, sig2.spec, sig2.src, TAU)               # through the parent: the view sees it
    _same(view.label_groups(lab, K, 0xFFFF, 1500), _ref_key(lab, K, sig2, group, 0xFFFF, 1500))
    view.close()


def test_profile_tags_of_the_pass_and_the_ranked_finish():
    n = RANGE
    sig, lab = _signals(n, 83), _labels(n, 2, 83)
    idx = _index(_ctx(), n, sig, _groups(n, 5, 0xF, 83))
    ctx = idx.ctx
    ctx.profile_reset(True)
    idx.label_groups(lab, 2, 0xF, 5)
    assert ctx.profile_read("label_summary")[1] == 1 and ctx.profile_read("label_summary_rank")[1] == 0
    idx.label_groups(lab, 2, 0xF, 5, top=2)
    assert ctx.profile_read("label_summary")[1] == 2 and ctx.profile_read("label_summary_rank")[1] == 1
    ctx.profile_reset(False)


def test_state_errors():
    from openintel_amd import _lib
    n = 100
    sig, lab = _signals(n, 84), _labels(n, 3, 84)
    group = _groups(n, 5, 0xF, 84)

    def state_error(call, word):
        with pytest.raises(_lib.OiError) as e:
            call()
        assert e.value.code == _lib.OI_ERR_STATE and word in e.value.message, e.value.message

    bare = _index(_ctx(), n, None, group)
    state_error(lambda: bare.label_summary(lab, 3), "no signals")
    plain = _index(_ctx(), n, sig)
    plain.label_summary(lab, 3)                                       # one cell, no filter: fine
    state_error(lambda: plain.label_groups(lab, 3, 0xF, 5), "doc attributes")
    state_error(lambda: plain.label_summary(lab, 3, n_buckets=2, bucket_width=10), "doc attributes")
    state_error(lambda: plain.label_summary(lab, 3, filter=(0, 0, 0, NO)), "doc attributes")


# ------------------------------------------------------------------ 9. the batch helpers
@pytest.fixture(scope="module")
def narrative_case():
    n = 2 * RANGE + 40
    K, nk = 4, 12
    sig, lab = _signals(n, 91), _labels(n, K, 91)
    rng = np.random.default_rng(91)
    key = np.where(rng.random(n) < 0.5, lab % K * 3, rng.integers(0, nk, size=n)).astype(np.uint32) % nk   # each cluster leans to one ticker
    group, stamp = key << np.uint32(4), _stamps(n, 0, 60, 91)
    tickers = ["TK%s" % chr(65 + k) for k in range(nk)]
    return _index(_ctx(), n, sig, group, stamp), lab, K, nk, sig, group, stamp, tickers


def test_narrative_timeline_fractions(narrative_case):
    from fractions import Fraction
    from openintel_amd import batch
    idx, lab, K, nk, sig, group, stamp, _ = narrative_case
    ref = _ref_time(lab, K, sig, stamp, 0, 10, 8)                     # buckets 6 and 7 are empty
    for labels in (lab, _dev(lab)):
        tl = batch.narrative_timeline(idx, labels, 0, 10, 8, n_clusters=K)
        assert len(tl) == K and len(tl[0]) == 8
        for b in range(8):
            tot = int(ref["total"][:, b].sum())
            assert [tl[c][b].total for c in range(K)] == ref["total"][:, b].tolist()
            fr = [tl[c][b].fraction for c in range(K)]
            assert fr == ([int(ref["total"][c, b]) / tot for c in range(K)] if tot else [0.0] * K)
            # each fraction is the correctly rounded total / bucket total, and as exact rationals they sum to 1 where there is a post
            assert sum(Fraction(tl[c][b].total, tot) for c in range(K)) == 1 if tot else not any(fr)
    with pytest.raises(ValueError):
        batch.narrative_timeline(idx, lab, 0, 10, 8)


def test_narrative_tickers_against_a_host_restatement(narrative_case):
    import datetime
    from openintel_amd import batch
    idx, lab, K, nk, sig, group, stamp, tickers = narrative_case
    now = datetime.datetime(2024, 1, 1, tzinfo=datetime.timezone.utc)
    dense = _ref_key(lab, K, sig, group, 0xF0, nk)
    cfg = batch.EngineConfig()
    for kw in (dict(top=5), dict(top=3, min_total=50, rank_by=batch.RankBy.SPECULATION_INDEX)):
        min_total = kw.get("min_total", cfg.min_sample)
        rank_by = kw.get("rank_by", batch.RankBy.CROWDING)
        keys, recs, counts, _ = _rank(dense, kw["top"], "total", int(min_total))
        got = batch.narrative_tickers(idx, lab, tickers, 0xF0, n_clusters=K, now=now, **kw)
        assert len(got) == K
        for c in range(K):
            want = batch.rank_group_records(keys[c], recs[c], int(counts[c]), tickers, rank_by, None, now, cfg)
            assert batch.compare_output_to_json(got[c]) == batch.compare_output_to_json(want)
            assert len(want.ranked) == int(counts[c]) >= 1


def test_narrative_tickers_distinctive_is_the_big_int_excess_order(narrative_case):
    import datetime
    from openintel_amd import batch
    idx, lab, K, nk, sig, group, stamp, tickers = narrative_case
    now = datetime.datetime(2024, 1, 1, tzinfo=datetime.timezone.utc)
    dense = _ref_key(lab, K, sig, group, 0xF0, nk)
    tot = [[int(v) for v in row] for row in dense["total"]]
    size = [sum(row) for row in tot]
    A = sum(size)
    per_key = [sum(tot[c][k] for c in range(K)) for k in range(nk)]
    top, bar = 4, 20
    cfg = batch.EngineConfig()
    for labels in (lab, _dev(lab)):
        got = batch.narrative_tickers(idx, labels, tickers, 0xF0, n_clusters=K, top=top, min_total=bar, now=now, distinctive=True)
        for c in range(K):
            order = sorted((k for k in range(nk) if tot[c][k] >= bar),
                           key=lambda k: (-(tot[c][k] * A - size[c] * per_key[k]), -tot[c][k], k))[:top]
            want = batch.rank_group_records(order, [dense[c, k] for k in order], len(order), tickers, batch.RankBy.CROWDING, None, now, cfg)
            assert batch.compare_output_to_json(got[c]) == batch.compare_output_to_json(want)
            assert order
    lean = [max(range(nk), key=lambda k: tot[c][k] * A - size[c] * per_key[k]) for c in range(K)]
    assert lean == [c * 3 for c in range(K)]                          # the ticker each cluster was built to lean to comes first
