"""Embedding ingest (oi_index_set_embeddings, oi_index_finalize, oi_index_set_screen_copy) at every normalise, norm-class and copy edge.

Every cosine route trusts what ingest leaves behind: the normalised rows (cosine.hip: l2_normalize_kernel), the corpus maxima X
and E and the long-row class (cosine_prefilter.hip: pf_row_norm_max_kernel, pf_row_norm_class_kernel), the bf16 screening copy
(pf_make_copy_kernel), the int8 copy with its per-row {scale, e_r} and e_max (cosine_screen_i8.hip: i8s_make_kernel), the per-query
staging words (oi_screen_stage.h: pf_stage_query_row; cosine_screen_i8.hip: i8s_stage_query_row) and the host logic around them
(api.hip).  A maximum that loses one row, a class pass that ignores E, a copy whose tail is stale: nothing crashes, nothing slows
down, a true top row is dropped on some data only.

References are numpy float64 in this file.  What is observed: the borrowed device tensor after normalize=True; idx.long_rows();
idx.screen_probe(q)[1], which is pf_eps(X, E, ...) and so shows the maxima the index holds; profile "screen_gate" (-1: the search
was never screened, 0: the screen held, 1: the exact pipeline took over); idx.index_bytes()[1]; and the lists, against
OI_COSINE_EXACT's on the same index.  Integer corpora make every f32 sum exact, so "the same lists" is bit for bit there.

Every "one sweep" is read from the launcher in the source (wave_sweep_rows, copy_wrap_vec8) and the device's CU count, as
tests/test_gpu_search_plan.py reads it: at 256 CUs one sweep of the wave-per-row kernels is 8192 rows."""
import os
import re

import numpy as np
import pytest

from test_gpu_screen_i8_edges import O, _i8_estimate, _winners_and_decoys, check_all, num_cus, run_both, stream_ctx  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openintel_amd", "csrc")
MI355X_CUS = 256
COS_TOL = 1e-5
VOCAB = 50
LONG_ROWS_MAX = 1024          # oi_internal.h: OI_LONG_ROWS_MAX; api.hip splits the classes only when n > 4 x this
NORM_LIMIT, QNORM_MIN = 1.0e15, 1.0e-12   # oi_screen_stage.h: PF_NORM_LIMIT, PF_QNORM_MIN (cosine_screen_i8.hip: the same two)
EPS_RTOL = 2e-4               # five f32 norms of <= 1024 squares, each within 3.1e-5; pf_eps's own comment budgets 1e-4
NORM_DIMS = (4, 60, 64, 68, 252, 256, 260, 384, 768, 1024)


# ==================================================================== the launchers, read from the source
def _function(path, name):
    with open(os.path.join(CSRC, path)) as f:
        m = re.search(r"^int %s\(.*?^}" % name, f.read(), re.S | re.M)
    assert m, (path, name)
    return m.group(0)


def wave_sweep_rows(path, launcher, cus):
    """Rows one sweep of a wave-per-row kernel covers: blocks of 256 threads = 4 waves = 4 rows, capped at num_cus x K blocks."""
    body = _function(path, launcher)
    assert "blocks = (n + 3) / 4;" in body and "dim3(256)" in body, launcher
    return cus * int(re.search(r"ctx->num_cus \* (\d+)", body).group(1)) * (256 // 64)


def copy_wrap_vec8(cus):
    """The vec8 index at which pf_make_copy_kernel's grid-stride loop wraps: one vec8 per thread, num_cus x K blocks of 256."""
    body = _function("cosine_prefilter.hip", "oi_launch_make_screen_copy")
    assert "(n_vec8 + 255) / 256" in body and "dim3(256)" in body
    return cus * int(re.search(r"ctx->num_cus \* (\d+)", body).group(1)) * 256


def sweeps(cus):
    return {"normalize": wave_sweep_rows("cosine.hip", "oi_launch_l2_normalize", cus),
            "max": wave_sweep_rows("cosine_prefilter.hip", "oi_launch_row_norm_max", cus),
            "class": wave_sweep_rows("cosine_prefilter.hip", "oi_launch_row_norm_classes", cus),
            "i8": wave_sweep_rows("cosine_screen_i8.hip", "oi_launch_make_screen_i8", cus)}


def wrap_rows(dim, cus):
    """(n, planted rows) of the copies' wrap test: the last row of the int8 copy's first sweep, the first of its second, the rows that
    hold the vec8s at which the bf16 copy wraps, and n - 1; n is just past the later wrap."""
    s, w = sweeps(cus)["i8"], copy_wrap_vec8(cus)
    at = [s - 1, s] + [(v * 8) // dim for v in (w - 1, w, w + 1)]
    n = max(at) + 150
    return n, sorted(set(at + [n - 1]))


# ==================================================================== f64 references
def bf16(x):
    """Round to nearest even onto bf16 (finite values), as v_cvt_pk_bf16_f32 and the query staging do."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32)).view(np.float32)


def norms64(x):
    """(|x_r|, |bf16(x_r) - x_r|) per row in f64."""
    x64 = np.asarray(x, dtype=np.float64)
    return np.sqrt((x64 * x64).sum(axis=-1)), np.sqrt(((bf16(x).astype(np.float64) - x64) ** 2).sum(axis=-1))


def classes64(rows):
    """api.hip, oi_index_set_embeddings restated in f64: (long rows set aside, X, E over the rows the margin is built from, every
    row's norm and error norm as multiples of the corpus RMS).  E0 > 0 and X0 > 0 are the guard of that function."""
    nx, ne = norms64(rows)
    n = rows.shape[0]
    rx, re_ = np.sqrt((nx * nx).mean()), np.sqrt((ne * ne).mean())
    long_ = (nx > 1.5 * rx) | (ne > 1.5 * re_)
    on = n > 4 * LONG_ROWS_MAX and rx > 0 and re_ > 0 and 1 <= int(long_.sum()) <= LONG_ROWS_MAX
    keep = ~long_ if on else np.ones(n, bool)
    return (int(long_.sum()) if on else 0), nx[keep].max(), ne[keep].max(), nx / rx, ne / (re_ if re_ > 0 else 1.0)


def eps_model(X, E, q, dim):
    """oi_screen_stage.h: pf_eps, in f64, with the query's three norms in f64."""
    qn, en = norms64(q)
    qtn = norms64(bf16(q))[0]
    tiny, d = 4.0e-18, float(dim)
    Xs, Es, qts, ens = X + tiny, E + tiny, qtn + tiny, en + tiny
    acc = d * 2.0 ** -22
    return 1.001 * (Es * qts + Xs * ens + acc * (Xs + Es) * qts) + d * 7.5231638452626401e-37 * (Xs + qn) + 1.0e-30


def norm_tol(dim):
    """Relative error per element of a normalised row.  Derived for an f32 kernel: a lane's fma chain of dim/64 squares plus a
    six-level wave sum is about half of (dim/64 + 6) ulp after the square root; one ulp for the root, 2.5 for the reciprocal, one
    for the product.  The kernel now sums the squares in f64 (error 2^-53 dim, nothing at this scale), rounds 1/sqrt to f32 once
    (half an ulp) and multiplies in f32 (half an ulp): re-derived, 2^-23 -- inside this bound at every dim, so the bound stays."""
    return (dim / 128.0 + 8.0) * 2.0 ** -24


def normalize64(x):
    """Rows / |row| in f64; a zero row stays, a NaN makes its row NaN, an inf gives NaN there and 0 elsewhere (1 / inf = 0): the
    results of the oracle's oio_l2_normalize_rows."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        ss = (x * x).sum(axis=1, keepdims=True)
        return np.where(ss == 0.0, x, x * (1.0 / np.sqrt(ss)))


# ==================================================================== constructions
def raw_rows(n, dim, seed):
    """Gaussian rows with scales over 1e-3 .. 1e3."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(-3, 3, size=(n, 1))).astype(np.float32)


SPECIAL = ("zero", "negzero", "nan", "inf", "big", "tiny")


def plant_special(rows, kind, at, seed=0):
    rng = np.random.default_rng(seed)
    dim = rows.shape[1]
    for i, r in enumerate(at):
        k = (0, dim - 1, 1)[i % 3]
        if kind == "zero":
            rows[r] = 0.0
        elif kind == "negzero":
            rows[r] = -0.0
        elif kind == "nan":
            rows[r, k] = np.nan
        elif kind == "inf":
            rows[r, k] = np.inf if i % 2 == 0 else -np.inf
        else:
            mag = 1e20 if kind == "big" else 1e-25
            rows[r] = (rng.choice([-1.0, 1.0], size=dim) * mag * (1.0 + 0.5 * rng.random(dim))).astype(np.float32)
    return rows


def grid_rows(n, dim, rng, f_lo, f_hi, e_cols):
    """+-(1 + (m + f) / 128) 2^e: e per column, m random in [0, 128), f = j / 65536 in [f_lo, f_hi).  Exact in f32; the bf16 error
    of an element is min(f, 1 - f) / 128 x 2^e whatever m is, so a row's error norm is set by its f alone."""
    m = rng.integers(0, 128, size=(n, dim), dtype=np.uint32)
    j = rng.integers(int(f_lo * 65536), int(f_hi * 65536), size=(n, dim), dtype=np.uint32)
    sg = rng.integers(0, 2, size=(n, dim), dtype=np.uint32)
    u = (sg << np.uint32(31)) | ((127 + e_cols).astype(np.uint32)[None, :] << np.uint32(23)) | (m << np.uint32(16)) | j
    return u.view(np.float32)


def set_f(rows, r, f):
    u = rows.view(np.uint32)
    u[r] = (u[r] & np.uint32(0xFFFF0000)) | np.uint32(int(f * 65536))


def set_m(rows, r, m):
    u = rows.view(np.uint32)
    u[r] = (u[r] & np.uint32(0xFF80FFFF)) | np.uint32(m << 16)


def maxima_rows(n, dim, which, at, seed=0):
    """Ordinary rows (f in [0.2, 0.3), e in {-3, -2}) and ONE row that owns X (m = 127 everywhere: 1.3 x the RMS norm) or E
    (f = 0.35: 1.39 x the RMS error norm) -- below the 1.5 x at which a row is set aside, above every other row."""
    rng = np.random.default_rng(seed + 7 * dim)
    rows = grid_rows(n, dim, rng, 0.2, 0.3, rng.integers(-3, -1, size=dim)).copy()
    if which == "X":
        set_m(rows, at, 127)
    else:
        set_f(rows, at, 0.35)
    return rows


def class_rows(n, n_long, seed=0):
    """Unit rows of dim 384, n_long of them three times as long; ids of the long rows."""
    from openintel_amd import synth
    rows = synth.embeddings_np(n, 384, seed=8100 + n_long)
    ids = np.sort(np.random.default_rng(seed + n_long).choice(n, size=n_long, replace=False))
    rows[ids] *= np.float32(3.0)
    return rows, ids


CLASS_CASES = [(4096, 10, 0), (4097, 1, 1), (4097, 1023, 1023), (4097, 1024, 1024), (4097, 1025, 0)]   # n, planted, set aside


def clear_queries(rows, targets, B, depth, seed):
    """B unit queries, query b leaning on row targets[b % len] (that row is its best by far), kept only when the f64 scores of
    its top depth + 1 rows are further apart than 1e-6 x the largest: two f32 orders of summation of 384 products (an MFMA's, a
    lane chain's) differ by a few 1e-8 x |x||q|, so no route decides a rank that the reference does not."""
    rng = np.random.default_rng(seed)
    x64 = rows.astype(np.float64)
    out, ref, b = [], [], 0
    while len(out) < B:
        t = x64[targets[b % len(targets)]]
        g = rng.standard_normal(rows.shape[1])
        v = t / np.linalg.norm(t) + 0.5 * g / np.linalg.norm(g)
        q = (v / np.linalg.norm(v)).astype(np.float32)
        s = x64 @ q.astype(np.float64)
        top = np.sort(s)[::-1][:depth + 1]
        if (-np.diff(top)).min() > 1e-6 * max(1.0, top[0]):
            out.append(q)
            ref.append(s)
            b += 1
    return np.stack(out), np.stack(ref)


def e_alone_rows(n=4097, dim=384, n_planted=10, seed=3):
    rng = np.random.default_rng(seed)
    rows = grid_rows(n, dim, rng, 0.0, 1.0, rng.integers(-4, 0, size=dim)).copy()
    ids = np.sort(rng.choice(n, size=n_planted, replace=False))
    for r in ids:
        set_f(rows, r, 0.499)
    return rows, ids


def int_rows(n, dim, seed):
    return np.random.default_rng(seed).integers(-2, 3, size=(n, dim)).astype(np.float32)


def planted_winners(rows, at, B, seed):
    """Row at[p] becomes 2 sign(z_p), z_p in {+-1, +-2}; query b is z_p (p = b mod len(at)) with 8 coordinates of its own zeroed, so
    the planted row reaches the largest score any row in [-2, 2] can have against it: the unique best by a wide margin."""
    rng = np.random.default_rng(seed)
    dim = rows.shape[1]
    z = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], dtype=np.float32), size=(len(at), dim))
    rows[at] = 2.0 * np.sign(z)
    q = z[np.arange(B) % len(at)].copy()
    for b in range(B):
        q[b, rng.choice(dim, size=8, replace=False)] = 0.0
    return q, np.asarray(at)[np.arange(B) % len(at)]


def sparse_signs(B, dim, seed):
    """B vectors with 256 entries of +-1: norm 16, exact in bf16."""
    rng = np.random.default_rng(seed)
    z = np.zeros((B, dim), dtype=np.float32)
    for b in range(B):
        z[b, rng.choice(dim, size=256, replace=False)] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=256)
    return z


def with_norm(z, norm):
    """z (norm 16) x a scale of 8 significant bits: exact in bf16, and every score against integer rows stays an exact f32."""
    m, e = np.frexp(norm / 16.0)
    return (z * np.float32(np.ldexp(np.round(m * 256.0) / 256.0, e))).astype(np.float32)


# kind -> has the screen a bound for it?
QUERY_KINDS = {"ordinary": True, "zero": False, "0.9e-12": False, "1.1e-12": True, "0.9e15": True, "1.1e15": False,
               "nan": False, "inf": False}


def special_query(kind, z):
    if kind == "ordinary":
        return z.copy()
    if kind == "zero":
        return np.zeros_like(z)
    if kind in ("nan", "inf"):
        q = z.copy()
        q[np.flatnonzero(z)[3]] = np.nan if kind == "nan" else np.inf
        return q
    return with_norm(z, float(kind))


# ==================================================================== CPU: the constructions themselves
def test_sweeps_come_from_the_launchers():
    assert sweeps(MI355X_CUS) == {"normalize": 8192, "max": 8192, "class": 8192, "i8": 8192}
    assert sweeps(304)["i8"] == 304 * 32
    assert copy_wrap_vec8(MI355X_CUS) == 1 << 20
    n, at = wrap_rows(384, MI355X_CUS)
    assert at == [8191, 8192, 21845, n - 1] and 21_900 < n < 22_100      # 2^20 vec8 = 21 845 rows and 16 vec8 of the next
    n, at = wrap_rows(768, MI355X_CUS)
    assert at == [8191, 8192, 10922, n - 1] and n > 8200


def test_tolerance_arithmetic():
    assert norm_tol(4) == (8 + 1 / 32) * 2.0 ** -24 and norm_tol(1024) == 2.0 ** -20
    assert all(2.0 ** -23 + 1024 * 2.0 ** -53 < norm_tol(d) for d in NORM_DIMS)      # the f64-sum kernel's own error is inside it
    x = np.array([[3.0, 4.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [1e20, 1e20, 1e20, 1e20], [np.inf, 1.0, -1.0, 0.0]], dtype=np.float32)
    r = normalize64(x)
    assert np.allclose(r[0], [0.6, 0.8, 0.0, 0.0], rtol=1e-15) and not r[1].any() and np.allclose(r[2], 0.5, rtol=1e-15)
    assert np.isnan(r[3, 0]) and not r[3, 1:].any()
    with np.errstate(all="ignore"):   # what the f32 sum of squares did: overflow above 1.8e19, underflow below 3e-23
        assert np.isinf(np.float32(1e20) * np.float32(1e20)) and np.float32(1e-25) * np.float32(1e-25) == 0.0


def test_eps_model_against_hand_values():
    def e0(d):
        return np.array([1.0] + [0.0] * (d - 1), dtype=np.float32)
    z = np.zeros(16, dtype=np.float32)
    # X = |q| = 1, E = e_q = 0 at d = 1024: 1.001 x 2^-12, and the three terms of 1e-18 and less
    assert abs(eps_model(1.0, 0.0, e0(1024), 1024) / (1.001 * 2.0 ** -12) - 1) < 1e-12
    # everything zero: the floor
    assert abs(eps_model(0.0, 0.0, z, 16) / 1.0e-30 - 1) < 1e-4
    # d = 256: E |q~| + acc (X + E) |q~| with acc = 2^-14
    want = 1.001 * (2.0 ** -9 + 2.0 ** -14 * (1 + 2.0 ** -9))
    assert abs(eps_model(1.0, 2.0 ** -9, e0(256), 256) / want - 1) < 1e-12
    # a query half-way between two bf16 values: 1 + 2^-8 rounds to even (1), e_q = 2^-8, |q~| = 1
    q = np.array([1.0 + 2.0 ** -8] + [0.0] * 15, dtype=np.float32)
    assert bf16(q)[0] == 1.0 and bf16(np.float32([1.0 + 3 * 2.0 ** -8]))[0] == 1.0 + 2.0 ** -6
    want = 1.001 * (0.5 * 1.0 + 2.0 * 2.0 ** -8 + 16 * 2.0 ** -22 * 2.5 * 1.0)
    assert abs(eps_model(2.0, 0.5, q, 16) / want - 1) < 1e-12


@pytest.mark.parametrize("n,n_long,aside", CLASS_CASES)
def test_class_edge_constructions_have_f64_margins(n, n_long, aside):
    """No planted norm inside [1.45, 1.55] x the RMS (long rows included): the reference never decides a near-tie."""
    rows, ids = class_rows(n, n_long)
    got, X, E, rx, re_ = classes64(rows)
    is_long = np.zeros(n, bool)
    is_long[ids] = True
    # (a planted row is long by its norm whatever its error norm; the others must be short by both)
    assert (rx[is_long] > 1.55).all() and (rx[~is_long] < 1.45).all() and (re_[~is_long] < 1.45).all()
    assert got == aside
    assert (X > 2.9) == (aside == 0), "eps comes from the corpus maxima exactly when nothing is set aside"


def test_long_by_E_alone_construction():
    rows, ids = e_alone_rows()
    got, X, E, rx, re_ = classes64(rows)
    planted = np.zeros(rows.shape[0], bool)
    planted[ids] = True
    assert (re_[planted] >= 1.55).all() and (re_[~planted] <= 1.45).all() and (rx <= 1.45).all()
    assert got == 10 and E == norms64(rows[~planted])[1].max()


@pytest.mark.parametrize("dim", [16, 768])
def test_maxima_constructions_own_their_maximum(dim):
    n = sweeps(MI355X_CUS)["max"] + 1
    for which in "XE":
        rows = maxima_rows(n, dim, which, n - 1)
        got, X, E, rx, re_ = classes64(rows)
        own, rest = (rx, re_)[which == "E"][n - 1], (rx, re_)[which == "E"][:n - 1].max()
        assert got == 0 and rx.max() < 1.45 and re_.max() < 1.45, "nothing is set aside: the maxima are the corpus's"
        assert own > 1.05 * rest, "losing the planted row moves X or E, and eps with it, by far more than the model's 2e-4"
        other = (re_, rx)[which == "E"]
        assert other[n - 1] < other[:n - 1].max(), "the planted row owns one maximum only"


def test_planted_winners_and_special_queries():
    n, at = wrap_rows(384, MI355X_CUS)
    rows = int_rows(n, 384, 1)
    q, win = planted_winners(rows, at, 64, 2)
    s = rows.astype(np.float64) @ q.T.astype(np.float64)
    assert np.array_equal(s.argmax(axis=0), win) and (np.sort(s, axis=0)[-1] > 2 * np.sort(s, axis=0)[-2]).all()
    assert classes64(rows)[0] == 0 and set(win.tolist()) == set(at)
    z = sparse_signs(4, 384, 5)
    for kind, bound in QUERY_KINDS.items():
        if kind in ("nan", "inf"):
            assert (~np.isfinite(special_query(kind, z[0]))).sum() == 1
            continue
        qn = norms64(special_query(kind, z[0]))[0]
        assert (QNORM_MIN * 1.05 < qn < NORM_LIMIT * 0.95) == bound, (kind, qn)
        assert kind in ("ordinary", "zero") or abs(qn / float(kind) - 1) < 0.01
        assert np.array_equal(bf16(special_query(kind, z[0])), special_query(kind, z[0])), "exact in bf16: e_q = 0, |q~| = |q|"


# ==================================================================== GPU helpers
@pytest.fixture(scope="module")
def ctx():
    import openintel_amd as oi
    c = oi.HipContext(0)
    c.set_screen_speculation(False)      # proven thresholds only: a failed speculation opens the gate by itself
    yield c
    c.close()


def modes():
    from openintel_amd import _lib
    return _lib


def make_index(ctx, rows, normalize=False, policy=None, finalize=True):
    import openintel_amd as oi
    n, dim = int(rows.shape[0]), int(rows.shape[1])
    idx = oi.HybridIndex(ctx, n, dim, VOCAB, 0)
    idx.set_embeddings(rows, normalize=normalize)
    if finalize:
        idx.set_forward(np.zeros(n, dtype=np.uint32), np.arange(n + 1, dtype=np.uint64))
        if policy is not None:
            idx.set_screen_copy(policy)
        idx.finalize()
    return idx


def search(ctx, idx, q, depth, mode):
    """(lists, screen_gate) of one search in the given cosine mode."""
    B = q.shape[0]
    ctx.set_cosine_mode(mode)
    L = idx.search_lists(q, np.zeros(B, dtype=np.uint32), np.arange(B + 1, dtype=np.uint32), depth=depth)
    gate = float(ctx.profile_read("screen_gate")[0])
    ctx.set_cosine_mode(modes().OI_COSINE_SCREEN)
    return L, gate


def same_lists(La, Lb):
    assert np.array_equal(La.cos_counts, Lb.cos_counts)
    for b, c in enumerate(La.cos_counts):
        assert np.array_equal(La.cos_docs[b][:c], Lb.cos_docs[b][:c]), b
        assert np.array_equal(La.cos_scores[b][:c].view(np.uint32), Lb.cos_scores[b][:c].view(np.uint32)), b


def check_cos_list(L, b, ref, depth, n, tol=COS_TOL):
    c = int(L.cos_counts[b])
    assert c == min(depth, n), b
    d, s = L.cos_docs[b][:c].astype(np.int64), L.cos_scores[b][:c]
    assert np.unique(d).size == c and d.min() >= 0 and d.max() < n, b
    assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (d[:-1] < d[1:]))).all(), ("not sorted by (score desc, doc asc)", b)
    assert np.abs(s.astype(np.float64) - ref[d]).max() <= tol, b
    kth = np.sort(ref)[::-1][c - 1]
    assert np.isin(np.nonzero(ref > kth + 2 * tol)[0], d).all(), ("a clearly better doc is missing", b)
    assert (ref[d] >= kth - 2 * tol).all(), ("a clearly worse doc is present", b)


def check_eps(idx, q, X, E, dim):
    eps = idx.screen_probe(q)[1].astype(np.float64)
    for b in range(q.shape[0]):
        want = eps_model(X, E, q[b], dim)
        assert abs(eps[b] / want - 1) <= EPS_RTOL, (b, eps[b], want)


def device_normalize(ctx, rows):
    """The borrowed device tensor after set_embeddings(normalize=True)."""
    import torch
    import openintel_amd as oi
    t = torch.from_numpy(rows).to("cuda:0")
    torch.cuda.synchronize()
    idx = oi.HybridIndex(ctx, rows.shape[0], rows.shape[1], VOCAB, 0)
    try:
        idx.set_embeddings(t, normalize=True)
        return t.cpu().numpy()
    finally:
        idx.close()


def check_normalized(got, raw):
    dim = raw.shape[1]
    ref, tol = normalize64(raw), norm_tol(dim)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaNs exactly where the reference has them (and in no neighbour)"
    fin = ~np.isnan(ref)
    g64 = got.astype(np.float64)
    err = np.abs(g64[fin] - ref[fin])
    bad = err > tol * np.abs(ref[fin])
    assert not bad.any(), (int(bad.sum()), float((err / np.maximum(np.abs(ref[fin]), 1e-300))[bad].max()), tol)
    unit = fin.all(axis=1) & (ref != 0).any(axis=1) & (np.abs(np.sqrt((ref * ref).sum(axis=1)) - 1) < 1e-9)
    assert (np.abs(np.sqrt((g64[unit] ** 2).sum(axis=1)) - 1.0) <= tol).all()
    return unit


# ==================================================================== 1. normalisation
@pytest.mark.gpu
@pytest.mark.parametrize("dim", NORM_DIMS)
def test_normalize_matches_f64(ctx, num_cus, dim):
    """Every lane count of a row (fewer than 64 elements, one past a multiple of 64), row counts around one block of four
    waves, and at dim 4 around one and two sweeps of the grid."""
    s = sweeps(num_cus)["normalize"]
    for n in (1, 3, 4, 5) + ((s - 1, s, s + 1, 2 * s + 3) if dim == 4 else ()):
        raw = raw_rows(n, dim, seed=dim + n)
        unit = check_normalized(device_normalize(ctx, raw), raw)
        assert unit.all()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", SPECIAL)
def test_normalize_special_rows(ctx, num_cus, kind):
    """At row 0, row n - 1 and the first row of the second sweep.  zero / -0.0: untouched, bit for bit.  One NaN: the row becomes
    NaN, its neighbours are as without it.  One inf: NaN there, 0 elsewhere.  Rows of 1e20s and of 1e-25s (the squared norm
    overflows f32, every square underflows it): unit rows like any other -- the f32 sum zeroed the first and left the second."""
    s = sweeps(num_cus)["normalize"]
    for dim, n in ((4, 2 * s + 3), (260, s + 2), (768, s + 2)):
        at = (0, n - 1, s)
        raw = plant_special(raw_rows(n, dim, seed=dim), kind, at, seed=dim)
        got = device_normalize(ctx, raw)
        unit = check_normalized(got, raw)
        if kind in ("zero", "negzero"):
            assert np.array_equal(got[list(at)].view(np.uint32), raw[list(at)].view(np.uint32)) and not unit[list(at)].any()
            assert (got[list(at)].view(np.uint32) == (0x80000000 if kind == "negzero" else 0)).all()
        elif kind == "nan":
            assert np.isnan(got[list(at)]).all() and int(np.isnan(got).any(axis=1).sum()) == 3
        elif kind == "inf":
            assert (np.isnan(got[list(at)]).sum(axis=1) == 1).all() and (np.nan_to_num(got[list(at)]) == 0).all()
        else:
            assert unit.all(), "the over / underflowing rows are unit rows now"


@pytest.mark.gpu
def test_normalize_host_rows_leaves_the_callers_array_and_stores_the_same_rows(ctx):
    """Host location: the caller's numpy array is unchanged byte for byte; the stored rows are the device-normalised ones --
    exact-mode lists at depth = n equal those of an index built with normalize=False from the device-normalised tensor."""
    n, dim, B = 1000, 260, 4
    raw = raw_rows(n, dim, seed=77)
    keep = raw.copy()
    q = raw_rows(B, dim, seed=78)
    a = make_index(ctx, raw, normalize=True)
    assert np.array_equal(raw.view(np.uint32), keep.view(np.uint32))
    b = make_index(ctx, device_normalize(ctx, raw), normalize=False)
    try:
        La, _ = search(ctx, a, q, n, modes().OI_COSINE_EXACT)
        Lb, _ = search(ctx, b, q, n, modes().OI_COSINE_EXACT)
        assert (La.cos_counts == n).all()
        same_lists(La, Lb)
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [384, 768, 128])
def test_normalized_corpus_on_every_route(ctx, O, dim):
    """3000 raw rows (scales 1e-3 .. 1e3) ingested with normalize=True: int8 tier (B = 64), copy screen (B = 8), exact, split;
    dim 128 takes the generic kernels whatever the mode."""
    from openintel_amd import synth
    M = modes()
    n, depth = 3000, 100
    raw = raw_rows(n, dim, seed=900 + dim)
    q = synth.embeddings_np(64, dim, seed=901 + dim)
    unit = O.l2_normalize_rows(raw)
    ref = [O.dot_scores(unit, q[b]).astype(np.float64) for b in range(64)]
    idx = make_index(ctx, raw, normalize=True)
    try:
        assert idx.long_rows() == 0
        screened = dim in (384, 768)
        assert (idx.index_bytes()[1] >= 3 * n * dim) if screened else (idx.index_bytes()[1] == 0)
        for mode, B in ((M.OI_COSINE_SCREEN, 64), (M.OI_COSINE_SCREEN, 8), (M.OI_COSINE_EXACT, 64), (M.OI_COSINE_EXACT, 8),
                        (M.OI_COSINE_SPLIT, 64), (M.OI_COSINE_SPLIT, 8)):
            L, gate = search(ctx, idx, q[:B], depth, mode)
            for b in range(B):
                check_cos_list(L, b, ref[b], depth, n)
            assert gate == (0.0 if screened and mode == M.OI_COSINE_SCREEN else -1.0), (mode, B, gate)
    finally:
        idx.close()


# ==================================================================== 2. corpus maxima and the two classes
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [16, 768])
def test_eps_sees_the_row_that_owns_a_maximum_wherever_it_sits(ctx, num_cus, dim):
    """The one row that owns X, and separately the one that owns E, at row 0, n - 1, the last row of the first sweep and the
    first of the second, for n = 1, 5, one sweep + 1: pf_eps of the index follows the f64 model over ALL rows every time."""
    s = sweeps(num_cus)["max"]
    assert sweeps(num_cus)["class"] == s
    q = np.random.default_rng(dim).standard_normal((3, dim)).astype(np.float32)
    for n in (1, 5, s + 1):
        for which in "XE":
            for at in sorted({0, n - 1, s - 1, s} & set(range(n))):
                rows = maxima_rows(n, dim, which, at)
                got, X, E, rx, re_ = classes64(rows)
                r = (rx, re_)[which == "E"]
                assert got == 0 and (n == 1 or r[at] > 1.05 * np.delete(r, at).max())
                idx = make_index(ctx, rows, finalize=False)
                try:
                    assert idx.long_rows() == 0
                    check_eps(idx, q, X, E, dim)
                finally:
                    idx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,n_long,aside", CLASS_CASES)
def test_class_edges(ctx, n, n_long, aside):
    """n = 4096: no classes whatever the rows.  n = 4097: 1, 1023, 1024 long rows are set aside and eps comes from the others;
    1025 are too many: one class, the corpus maxima.  Lists at depth 100 on the int8 route and the copy screen are the exact
    mode's; every query's own long row is its rank 0; with classes on the screen holds."""
    M = modes()
    dim, depth = 384, 100
    rows, ids = class_rows(n, n_long)
    got, X, E, _, _ = classes64(rows)
    assert got == aside
    q, ref = clear_queries(rows, ids, 64, depth, seed=n_long)
    idx = make_index(ctx, rows)
    try:
        assert idx.long_rows() == aside
        check_eps(idx, q[:8], X, E, dim)
        assert idx.index_bytes()[1] >= 3 * n * dim
        Le, _ = search(ctx, idx, q, depth, M.OI_COSINE_EXACT)
        for B in (64, 8):     # the int8 route, the copy screen
            L, gate = search(ctx, idx, q[:B], depth, M.OI_COSINE_SCREEN)
            assert gate != -1.0 and (gate == 0.0 or not aside), gate
            for b in range(B):
                assert int(L.cos_counts[b]) == depth and L.cos_docs[b][0] == ids[b % n_long], b
                assert np.array_equal(L.cos_docs[b][:depth], Le.cos_docs[b][:depth]), b
                assert np.array_equal(L.cos_docs[b][:depth], np.argsort(-ref[b], kind="stable")[:depth]), b
                tol = COS_TOL * float(Le.cos_scores[b][0])
                assert np.abs(L.cos_scores[b][:depth] - Le.cos_scores[b][:depth]).max() <= tol, b
                assert np.abs(L.cos_scores[b][:depth] - ref[b][L.cos_docs[b][:depth]]).max() <= tol, b
    finally:
        idx.close()


@pytest.mark.gpu
def test_rows_long_by_their_error_norm_alone(ctx):
    """10 of 4097 rows sit a hair from a bf16 tie in every element: an ordinary norm, 1.7 x the RMS error norm.  A class pass that
    looks at |x_r| only sets nothing aside."""
    rows, ids = e_alone_rows()
    got, X, E, _, _ = classes64(rows)
    q = np.random.default_rng(5).standard_normal((4, 384)).astype(np.float32)
    idx = make_index(ctx, rows, finalize=False)
    try:
        assert got == 10 and idx.long_rows() == 10
        check_eps(idx, q, X, E, 384)
    finally:
        idx.close()


@pytest.mark.gpu
def test_bf16_exact_corpus_is_one_class(ctx):
    """Small integers: E = 0.  Ten rows 64 x as long would be set aside by their norms, but api.hip (oi_index_set_embeddings:
    `(mx.X > X0 || mx.E > E0) && X0 > 0.f && E0 > 0.f`) asks for E0 > 0 and leaves the corpus in one class.  Pinned: a change of
    that policy edits the first assert knowingly."""
    M = modes()
    n, dim, depth = 4100, 384, 100
    rows = int_rows(n, dim, 11)
    rows[np.arange(10) * 400 + 7] *= 64.0
    assert (norms64(rows)[1] == 0).all() and (classes64(rows)[3] > 1.55).sum() == 10
    q = int_rows(64, dim, 12)
    idx = make_index(ctx, rows)
    try:
        assert idx.long_rows() == 0
        Le, _ = search(ctx, idx, q, depth, M.OI_COSINE_EXACT)
        for B in (64, 8):
            L, gate = search(ctx, idx, q[:B], depth, M.OI_COSINE_SCREEN)
            assert gate != -1.0
            same_lists(L, search(ctx, idx, q[:B], depth, M.OI_COSINE_EXACT)[0] if B == 8 else Le)
    finally:
        idx.close()


NO_BOUND = ("nan_first", "nan_last", "nan_second_sweep", "inf", "1e20", "1.1e15", "9e14")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", NO_BOUND)
def test_corpus_without_a_bound_is_never_screened(ctx, num_cus, kind):
    """A NaN at (0, 0), at (n - 1, dim - 1) or in the second sweep, an inf, a row of 1e20s (its norm overflows f32), a row of norm
    1.1e15: no search of that index is screened and no copy is kept.  A row of norm 9e14 alone still is."""
    M = modes()
    dim, depth, B = 384, 10, 16
    s = sweeps(num_cus)["max"]
    n = s + 1
    rows = int_rows(n, dim, 21)
    z = sparse_signs(1, dim, 22)[0]
    if kind.startswith("nan"):
        r, k = {"nan_first": (0, 0), "nan_last": (n - 1, dim - 1), "nan_second_sweep": (s, 5)}[kind]
        rows[r, k] = np.nan
    elif kind == "inf":
        rows[s - 1, 100] = -np.inf
    elif kind == "1e20":
        rows[s] = 1e20
    else:
        rows[n - 1] = with_norm(z, float(kind))
    q = int_rows(B, dim, 23)
    idx = make_index(ctx, rows)
    try:
        screened = kind == "9e14"
        L, gate = search(ctx, idx, q, depth, M.OI_COSINE_SCREEN)
        assert (gate != -1.0) if screened else (gate == -1.0), gate
        assert (idx.index_bytes()[1] > 0) == screened and idx.long_rows() == 0
        same_lists(L, search(ctx, idx, q, depth, M.OI_COSINE_EXACT)[0])
    finally:
        idx.close()


# ==================================================================== 3. the screening copies and the copy policy
@pytest.mark.gpu
@pytest.mark.parametrize("dim", [384, 768])
def test_copies_hold_the_rows_at_the_grid_stride_wrap(ctx, num_cus, dim):
    """Each query's unique best row sits at the last row of i8s_make_kernel's first sweep, the first of its second, the rows holding
    the vec8s at which pf_make_copy_kernel wraps, or n - 1.  A row a copy never got has scale 0 (or stale bytes) there: its screen
    score is not the winner's and the list loses its rank 0."""
    M = modes()
    n, at = wrap_rows(dim, num_cus)
    rows = int_rows(n, dim, 31 + dim)
    q, win = planted_winners(rows, at, 64, 32 + dim)
    idx = make_index(ctx, rows)
    try:
        assert idx.index_bytes()[1] >= 3 * n * dim and idx.long_rows() == 0, "both copies"
        for B in (64, 8):     # the int8 route, the copy screen
            L, gate = search(ctx, idx, q[:B], 10, M.OI_COSINE_SCREEN)
            assert gate == 0.0
            assert np.array_equal(L.cos_docs[:B, 0], win[:B])
            same_lists(L, search(ctx, idx, q[:B], 10, M.OI_COSINE_EXACT)[0])
    finally:
        idx.close()


@pytest.mark.gpu
def test_int8_copy_error_norms_are_not_short(stream_ctx, O):
    """e_r as i8s_make_kernel stores it.  test_gpu_screen_i8_edges' bound-tight construction, with more room: winners whose
    quantisation error points straight at the query (s~ sits e_r below the true score) in the last rows of the copy, decoys in the
    first chunk that round the other way.  With e_r at half its size the decoys' lower bounds pass the winners' upper bounds and the
    last chunk drops true top rows."""
    dim, n, B, depth, n_dec, n_win = 384, 50_001, 16, 100, 200, 40
    from openintel_amd import synth
    rng = np.random.default_rng(dim)
    sg = rng.choice(np.array([-1.0, 1.0]), size=dim)
    q = synth.embeddings_np(B, dim, seed=11 + dim)
    q[0] = (sg / np.sqrt(dim)).astype(np.float32)
    I = rng.integers(40, 81, size=dim) * sg
    I[0] = 127.0 * sg[0]
    P, Rr = float(I @ q[0]), float(sg[1:] @ q[0, 1:].astype(np.float64))
    s_w = 0.9 / (P + 0.49 * Rr)
    s_d = (0.9 - 0.2 * Rr * s_w) / (P + 0.51 * Rr)

    def row(s, frac):
        x = s * (I + frac * sg)
        x[0] = s * I[0]
        return x.astype(np.float32)
    xw, xd = row(s_w, 0.49), row(s_d, 0.51)
    rows = synth.embeddings_np(n, dim, seed=7001) * np.float32(np.linalg.norm(xw))   # background of the winners' norm: no long rows
    win = np.arange(n - n_win, n)
    rows[:n_dec] = xd
    rows[win] = xw
    est, er = _i8_estimate(np.stack([xw, xd]), q[0])
    true = np.stack([xw, xd]).astype(np.float64) @ q[0].astype(np.float64)
    assert true[0] > true[1] + 1e-3, "winners are truly above the decoys"
    assert est[0] + er[0] < est[1] - 1e-3, "full e_r: the winner's upper bound s~ + e_r + c_q still reaches the decoys' lower bound"
    assert est[0] + 0.5 * er[0] + 2e-3 < est[1] - 0.5 * er[1], "half e_r: it does not, by 2e-3 (c_q is 1e-4 here)"
    R = run_both(stream_ctx, rows, q, depth, 0, spec=False)
    assert R.gate == 0.0, "the int8 tier holds (the exact pipeline would hide a dropped row)"
    check_all(O, R, rows, q, depth, 0, queries=[0, 1, B - 1])
    _winners_and_decoys(R, win, depth)


def _unit_corpus(n, dim, seed, n_long=0):
    from openintel_amd import synth
    rows = synth.embeddings_np(n, dim, seed=seed)
    rows[np.arange(n_long) * 401 + 3] *= np.float32(3.0)
    return rows


def _own_queries(rows, B, seed):
    """Query b is row w_b of THESE rows, normalised: its rank 0 here and (almost surely) in no other corpus."""
    w = np.random.default_rng(seed).choice(rows.shape[0], size=B, replace=False)
    q = rows[w].astype(np.float64)
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32), w


@pytest.mark.gpu
def test_copy_policy_transitions_on_a_finalized_index(ctx):
    """NEVER -> ALWAYS -> NEVER -> AUTO: the copies go and come, the lists are the same bytes at every step."""
    M = modes()
    n, dim = 5000, 384
    rows = int_rows(n, dim, 41)
    q, win = planted_winners(rows, [0, 2500, n - 1], 64, 42)
    idx = make_index(ctx, rows, policy=M.OI_SCREEN_COPY_NEVER)
    try:
        seen = []
        for policy, want in ((None, "zero"), (M.OI_SCREEN_COPY_ALWAYS, "both"), (M.OI_SCREEN_COPY_NEVER, "zero"), (M.OI_SCREEN_COPY_AUTO, "some")):
            if policy is not None:
                idx.set_screen_copy(policy)
            b = idx.index_bytes()[1]
            assert {"zero": b == 0, "both": b >= 3 * n * dim, "some": b >= 2 * n * dim}[want], (policy, b)
            for B in (64, 8):
                L, gate = search(ctx, idx, q[:B], 10, M.OI_COSINE_SCREEN)
                assert gate == (-1.0 if B == 8 and b == 0 else 0.0) and np.array_equal(L.cos_docs[:B, 0], win[:B])
                assert idx.index_bytes()[1] == b, "a search in OI_COSINE_SCREEN makes no copy"
                seen.append((B, L))
        for B, L in seen[2:]:
            same_lists(L, seen[0 if B == 64 else 1][1])
        same_lists(seen[0][1], search(ctx, idx, q, 10, M.OI_COSINE_EXACT)[0])
    finally:
        idx.close()


@pytest.mark.gpu
def test_reingest_under_a_finalized_index(ctx):
    """set_embeddings with other rows (other winners, ten long rows; then others again) under a finalized index, from the host and
    from a device tensor: the copies are remade NOW (as many bytes as a fresh index holds) from the new rows, long_rows() follows
    them, and the lists are a fresh index's -- a stale copy, or none, fails."""
    import torch
    M = modes()
    n, dim, B, depth = 4200, 384, 64, 10
    corpora = [_unit_corpus(n, dim, 51), _unit_corpus(n, dim, 52, n_long=10), _unit_corpus(n, dim, 53)]
    idx = make_index(ctx, corpora[0])
    try:
        for step, rows in enumerate(corpora):
            if step == 1:
                idx.set_embeddings(rows, normalize=False)
            elif step == 2:
                t = torch.from_numpy(rows).to("cuda:0")
                torch.cuda.synchronize()
                idx.set_embeddings(t, normalize=False)
            q, w = _own_queries(rows, B, 60 + step)
            fresh = make_index(ctx, rows)
            try:
                assert idx.long_rows() == fresh.long_rows() == (10 if step == 1 else 0)
                assert idx.index_bytes()[1] == fresh.index_bytes()[1] >= 3 * n * dim
                assert np.array_equal(idx.screen_probe(q[:4])[1], fresh.screen_probe(q[:4])[1])
                for Bq in (64, 8):
                    L, gate = search(ctx, idx, q[:Bq], depth, M.OI_COSINE_SCREEN)
                    Lf, gate_f = search(ctx, fresh, q[:Bq], depth, M.OI_COSINE_SCREEN)
                    assert gate == gate_f == 0.0 and np.array_equal(L.cos_docs[:Bq, 0], w[:Bq])
                    same_lists(L, Lf)
            finally:
                fresh.close()
    finally:
        idx.close()


@pytest.mark.gpu
def test_switching_corpus_type(ctx):
    """f32 -> set_embeddings_bf16 -> f32 on one finalized index: the derived copies go with the f32 rows and come back with them;
    the lists are a fresh index's at each step."""
    import openintel_amd as oi
    M = modes()
    n, dim, B, depth = 3000, 384, 64, 10
    rows = [_unit_corpus(n, dim, 71), _unit_corpus(n, dim, 72), _unit_corpus(n, dim, 73)]
    as_bf16 = (bf16(rows[1]).view(np.uint32) >> 16).astype(np.uint16)
    idx = make_index(ctx, rows[0])
    try:
        for step in range(3):
            if step == 1:
                idx.set_embeddings_bf16(as_bf16)
                fresh = oi.HybridIndex(ctx, n, dim, VOCAB, 0)
                fresh.set_embeddings_bf16(as_bf16)
                fresh.set_forward(np.zeros(n, dtype=np.uint32), np.arange(n + 1, dtype=np.uint64))
                fresh.finalize()
            else:
                if step == 2:
                    idx.set_embeddings(rows[2], normalize=False)
                fresh = make_index(ctx, rows[step])
            try:
                b = idx.index_bytes()[1]
                assert b == fresh.index_bytes()[1] and ((b == 0) if step == 1 else (b >= 3 * n * dim)), (step, b)
                q, w = _own_queries(bf16(rows[1]) if step == 1 else rows[step], B, 80 + step)
                L, _ = search(ctx, idx, q, depth, M.OI_COSINE_SCREEN)
                assert np.array_equal(L.cos_docs[:B, 0], w)
                same_lists(L, search(ctx, fresh, q, depth, M.OI_COSINE_SCREEN)[0])
            finally:
                fresh.close()
    finally:
        idx.close()


# ==================================================================== 4. query staging
@pytest.fixture(scope="module")
def staged(ctx):
    """Integer rows in [-2, 2] (every score an exact f32) under an index with both copies and one that the copy-screen mode gives
    the bf16 copy alone; (rows' X in f64, the two indexes)."""
    made = {}

    def get(dim):
        if dim not in made:
            rows = int_rows(3000, dim, 90 + dim)
            made[dim] = (norms64(rows)[0].max(), make_index(ctx, rows), make_index(ctx, rows, policy=modes().OI_SCREEN_COPY_NEVER))
        return made[dim]
    yield get
    for _, a, b in made.values():
        a.close()
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dim,B", [(384, 1), (384, 31), (384, 32), (384, 33), (384, 64), (384, 65), (768, 33)])
def test_query_staging(ctx, staged, dim, B):
    """Each kind of query at slot 0, 31, 32 and B - 1 of a batch of ordinary ones (both sides of the 32-row padding): eps is inf
    exactly for the kinds without a bound and the model's for the others; the int8 route (B <= 8: the copy screen) and the copy
    screen return the exact mode's lists; the gate opens exactly when the batch holds a query without a bound."""
    M = modes()
    X, both, copy_only = staged(dim)
    n, depth = 3000, 10
    z = sparse_signs(B + 1, dim, 100 + B)
    for kind, bound in QUERY_KINDS.items():
        for slot in sorted({0, 31, 32, B - 1} & set(range(B))):
            q = z[:B].copy()
            q[slot] = special_query(kind, z[B])
            eps = both.screen_probe(q)[1].astype(np.float64)
            for b in range(B):
                if b == slot and not bound:
                    assert np.isposinf(eps[b]), (kind, slot, eps[b])
                else:
                    assert abs(eps[b] / eps_model(X, 0.0, q[b], dim) - 1) <= EPS_RTOL, (kind, slot, b, eps[b])
            Le, _ = search(ctx, both, q, depth, M.OI_COSINE_EXACT)
            for idx, mode in ((both, M.OI_COSINE_SCREEN), (copy_only, M.OI_COSINE_SCREEN_COPY)):
                L, gate = search(ctx, idx, q, depth, mode)
                assert (gate == 0.0) if bound else (gate > 0.0), (kind, slot, mode, gate)
                same_lists(L, Le)
            assert both.index_bytes()[1] >= 3 * n * dim and 2 * n * dim <= copy_only.index_bytes()[1] < 3 * n * dim
