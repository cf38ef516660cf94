"""The residual plane of the int8 screening copy as oi_index_finalize makes it (csrc/screen_i8_residual.hip: i8r_make_kernel).

The plane and its {t_r, e2_r} table are read back (HybridIndex.residual_plane, an internal export) and compared with the numpy
construction of tests/test_residual_plane_bound.py: the bytes and the scales bit for bit, e2_r not short of the true error (f64)
and no looser than its (1 + 2^-20) rounding, e2_max the largest e2_r over the rows that are not long.

Shapes: d 384 and 768 (one and a half, and three float4 sweeps of a wave); n 1, 31, 32, 33 (both sides of a tile of the copy's
layout), 4 097 (the smallest corpus that sets a long row aside, and the planted huge row is one) and 8 200 (more rows than the
launch has waves on a 256-CU device, 8 192: some waves take a second row).  The planted rows of the bound test ride at the end of
every corpus that has room for them."""
import numpy as np
import pytest

from test_gpu_prefilter import _forward, _index
from test_residual_plane_bound import F32, F64, plane1, plane2, planted_rows, unit_rows, _true_error

pytestmark = pytest.mark.gpu
VOCAB = 50


@pytest.fixture()
def ctx():
    import openintel_amd as oi
    from openintel_amd import _lib
    c = oi.HipContext(0)
    c.set_cosine_mode(_lib.OI_COSINE_SCREEN)
    yield c
    c.close()


def _rows(n, d, seed=0):
    x = unit_rows(n, d, 1000 + n + d + seed)
    # (scaled by powers of two, which moves no rounding: every planted row but the huge one then has a norm below 1, so the
    # huge one is the only row a corpus of more than 4 096 rows sets aside as long)
    planted = [p * F32(f) for p, f in zip(planted_rows(d).values(), (1.0, 0.5, 0.5, 0.25, 0.25))]
    if n >= len(planted) + 1:
        x[n - len(planted):] = np.stack(planted)
    return x


def _make(ctx, x):
    n = x.shape[0]
    terms, offs = _forward(np.random.default_rng(n), n, VOCAB)
    return _index(ctx, x, terms, offs, VOCAB)


def _plane_bytes(n, d):
    """oi_screen_i8_bytes, in the 256-byte units of an allocation: n d bytes, {t_r, e2_r} per row, 64 padding rows, e2_max."""
    return (((n * d + 255) & ~255) + 8 * (n + 64) + 256 + 255) & ~255


def _check_plane(idx, x, long_rows=()):
    n, d = x.shape
    got = idx.residual_plane()
    assert got is not None, "the index holds no residual plane"
    j, meta, e2max, nbytes = got
    i, s, er = plane1(x)
    jr, tr, e2r, _ = plane2(x, i, s)
    assert np.array_equal(j, jr), "residual bytes differ from the numpy construction at rows %s" % np.nonzero((j != jr).any(axis=1))[0][:8]
    assert np.array_equal(meta[:, 0].view(np.uint32), tr.view(np.uint32)), "t_r differs"
    true = _true_error(x, i, s, jr, tr)
    assert (meta[:, 1].astype(F64) >= true).all(), "e2_r is short"
    assert (meta[:, 1].astype(F64) <= true * (1 + 4e-6) + 1e-45).all(), "e2_r is looser than its rounding"
    keep = np.ones(n, bool)
    keep[list(long_rows)] = False
    assert F32(e2max) == meta[keep, 1].max(), (e2max, meta[keep, 1].max())
    assert nbytes == _plane_bytes(n, d)
    assert n * (d + 8) <= nbytes <= n * (d + 8) + 255 + 8 * 64 + 256 + 255
    return nbytes


@pytest.mark.parametrize("d", [384, 768])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 4097, 8200])
def test_plane_equals_the_numpy_construction(ctx, d, n):
    x = _rows(n, d)
    idx = _make(ctx, x)
    huge = [n - 5] if n >= 4097 else []        # planted_rows' first: norm 50 among unit rows, the one long row
    assert idx.long_rows() == len(huge)
    with_plane = idx.index_bytes()[1]
    nbytes = _check_plane(idx, x, huge)
    assert idx.residual_plane(drop=True) is None and idx.residual_plane() is None
    assert with_plane - idx.index_bytes()[1] == nbytes, "index_bytes counts the plane in the screening-copy figure"
    assert idx.index_bytes()[1] >= 3 * n * d, "the other two copies stay"
    idx.close()


@pytest.mark.parametrize("d", [384, 768])
def test_plane_follows_the_int8_copy(ctx, d):
    """Remade on re-ingest under a finalized index, gone with NEVER, back with AUTO, gone for a bf16 corpus; a view aliases it."""
    import openintel_amd as oi
    from openintel_amd import _lib
    n = 33
    x, y = _rows(n, d), _rows(n, d, seed=7)
    idx = _make(ctx, x)
    _check_plane(idx, x)
    full = idx.index_bytes()[1]
    c2 = oi.HipContext(0)
    try:
        v = idx.view(c2)
        _check_plane(v, x)
        assert v.index_bytes()[1] == 0, "a view owns none of the copies"
        v.close()
    finally:
        c2.close()
    idx.set_embeddings(y, normalize=False)          # new rows under a finalized index: every copy anew
    _check_plane(idx, y)
    assert idx.index_bytes()[1] == full
    idx.set_screen_copy(_lib.OI_SCREEN_COPY_NEVER)
    assert idx.residual_plane() is None and idx.index_bytes()[1] == 0
    idx.set_screen_copy(_lib.OI_SCREEN_COPY_AUTO)
    _check_plane(idx, y)
    assert idx.index_bytes()[1] == full
    import torch
    yb = torch.from_numpy(y).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    idx.set_embeddings_bf16(yb)                       # a switch of corpus type: no f32 rows, no copies
    assert idx.residual_plane() is None and idx.index_bytes()[1] == 0
    idx.close()
