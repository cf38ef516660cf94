"""The residual plane of the int8 screening copy and the bound of its rescreen, restated in numpy (csrc/screen_i8_residual.hip,
DESIGN 4.1a "Bound of the residual tier").  No GPU: the f32 steps of the kernels are taken in numpy f32, every reference in f64.

  first plane   s_r = max |x| / 127, i = rint(x / s_r), e_r >= |s_r i - x|                       (i8s_make_kernel)
  second plane  rho = x - s_r i (f64, exact), t_r = max |f32(rho)| / 127, j = rint(f32(rho) / t_r),
                e2_r >= |s_r i + t_r j - x| measured in f64, times (1 + 2^-20)                     (i8r_make_kernel)
  query         q^ = a (h + l / 128); |q^|, |e_q| in f64 rounded up; c_q; the two margins          (i8s_stage_query_row)
  rescreen      s' = f32(l_r + m_r) with l_r = f32(s~ - m_r), m_r = fma(e_r, |q^|, c_q);
                s~2 = f32(s' + f32(f32(S2) f32(t_r a / 128))), S2 = 128 sum j h + sum j l          (i8r_rescreen_kernel)
  claim         e2_r >= the true error, and |s~2 - s^| <= eps2'_q for every row, s^ the rescoring's f32 fma chain
                (pf_rescore_kernel: per lane the float4 at lane, lane + 64, ..., then the butterfly sum)

The same functions are the reference of tests/test_gpu_residual_plane.py, which compares the device's plane with them bit for bit."""
import numpy as np
import pytest

F32, F64 = np.float32, np.float64
UP = F32(1.00000095367431640625)   # 1 + 2^-20


# ------------------------------------------------------------------------------------------------ the construction
def plane1(x):
    """(i int8 [n, d], s f32 [n], e_r f32 [n]) of f32 rows x."""
    s = (np.abs(x).max(axis=1) / F32(127.0)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(s[:, None] > 0, np.rint(x / s[:, None]), F32(0.0)).astype(F32)
    i = np.clip(t, -127.0, 127.0).astype(np.int8)
    e = s.astype(F64)[:, None] * i.astype(F64) - x.astype(F64)
    er = np.sqrt((e * e).sum(axis=1)).astype(F32) * UP
    return i, s, er


def plane2(x, i, s):
    """(j int8 [n, d], t f32 [n], e2_r f32 [n], e2 in f64 before rounding) of the rows and their first plane."""
    rho = x.astype(F64) - s.astype(F64)[:, None] * i.astype(F64)
    rf = rho.astype(F32)
    t = (np.abs(rf).max(axis=1) / F32(127.0)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(t[:, None] > 0, np.rint(rf / t[:, None]), F32(0.0)).astype(F32)
    j = np.clip(f, -127.0, 127.0).astype(np.int8)
    e = t.astype(F64)[:, None] * j.astype(F64) - rho
    e2 = np.sqrt((e * e).sum(axis=1))
    return j, t, e2.astype(F32) * UP, e2


def stage(q, X, e_max, e2_max):
    """The staged words of f32 queries q: h, l (int8), a, |q^|, c_q, the int8 tier's m2 and the residual tier's 2 eps2' (f32)."""
    d = q.shape[1]
    a = (np.abs(q).max(axis=1) / F32(127.0)).astype(F32)
    t = (q / a[:, None]).astype(F32)
    h = np.clip(np.rint(t), -127, 127).astype(F32)
    l = np.clip(np.rint(((t - h).astype(F32) * F32(128.0)).astype(F32)), -127, 127).astype(F32)
    qh = a.astype(F64)[:, None] * (h.astype(F64) + l.astype(F64) * 0.0078125)
    qn = np.sqrt((qh * qh).sum(axis=1)).astype(F32) * UP
    en = np.sqrt(((qh - q.astype(F64)) ** 2).sum(axis=1)).astype(F32) * UP
    X, em, e2m = F32(X), F32(e_max), F32(e2_max)
    rnd = F32(3.814697265625e-06) + F32(d) * F32(2.384185791015625e-07)
    cq = F32(1.001) * (X * en + rnd * (X + em) * (qn + en)) + F32(1.0e-27)
    m2 = F32(2.002) * (em * qn + cq)
    rec = F32(4.76837158203125e-07) * ((X + em) * qn + (em * qn + cq))
    m2r = F32(2.002) * (e2m * qn + cq + rec)
    return h.astype(np.int8), l.astype(np.int8), a, qn.astype(F32), cq.astype(F32), m2.astype(F32), m2r.astype(F32)


def fma32(x, y, z):
    """f32(x y + z) with ONE rounding, as v_fma_f32 gives it (finite operands).  x y is exact in f64; the f64 sum is taken with
    its exact error (two-sum) and rounded to odd, so that the rounding to f32 behind it cannot land on a tie the exact sum is not
    on -- a plain f64 sum rounds twice and is off by an f32 ulp about once in 2^30 operations, which a bit-for-bit comparison
    with the device over millions of products meets (tests/test_gpu_residual_rescreen_edges.py)."""
    p, z = x.astype(F64) * y.astype(F64), np.asarray(z).astype(F64)
    s = p + z
    v = s - p
    e = (p - (s - v)) + (z - v)          # s + e = p + z exactly
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    odd = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return odd.astype(F32)


def rescreen(i, s, er, j, t, h, l, a, qn, cq):
    """(s~, l_r, s', s~2) [n, B] as the screen and the residual rescreen compute them."""
    hi, lo = h.astype(np.int64), l.astype(np.int64)
    S = 128 * (i.astype(np.int64) @ hi.T) + i.astype(np.int64) @ lo.T
    S2 = 128 * (j.astype(np.int64) @ hi.T) + j.astype(np.int64) @ lo.T
    assert np.abs(S).max() < 2 ** 31 and np.abs(S2).max() < 2 ** 31
    qa = (a * F32(0.0078125)).astype(F32)
    sc = S.astype(F32) * (s[:, None] * qa[None, :]).astype(F32)
    m = fma32(np.broadcast_to(er[:, None], sc.shape), np.broadcast_to(qn[None, :], sc.shape), np.broadcast_to(cq[None, :], sc.shape))
    lb = (sc - m).astype(F32)
    s1 = (lb + m).astype(F32)
    s2 = (s1 + (S2.astype(F32) * (t[:, None] * qa[None, :]).astype(F32)).astype(F32)).astype(F32)
    return sc, lb, s1, s2, m


def rescore(x, q):
    """pf_rescore_kernel's f32 score of every (row, query): lane L chains the float4 at L, L + 64, ... then the butterfly sum."""
    n, d = x.shape
    nvec = d // 4
    out = np.empty((n, q.shape[0]), F32)
    for b in range(q.shape[0]):
        acc = np.zeros((n, 64), F32)
        for v0 in range(0, nvec, 64):
            lanes = np.arange(min(64, nvec - v0))
            for c in range(4):
                k = 4 * (v0 + lanes) + c
                acc[:, lanes] = fma32(x[:, k], np.broadcast_to(q[b, k][None, :], (n, lanes.size)), acc[:, lanes])
        for o in (32, 16, 8, 4, 2, 1):
            acc = (acc + acc[:, np.arange(64) ^ o]).astype(F32)
        out[:, b] = acc[:, 0]
    return out


# ------------------------------------------------------------------------------------------------ the rows
def unit_rows(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(F32)


def planted_rows(d, seed=5):
    """{name: f32 row}: the rows the rounding of either plane can go wrong on."""
    rng = np.random.default_rng(seed)
    base = unit_rows(1, d, seed + 1)[0]
    out = {}
    huge = base.copy()
    huge[5] = F32(50.0)
    out["one huge element"] = huge
    s = F32(2.0 ** -10)
    k = rng.integers(-100, 101, size=d).astype(F32)
    k[0] = 127.0
    half1 = (s * (k + F32(0.5))).astype(F32)
    half1[0] = s * F32(127.0)
    out["half steps of the first plane"] = half1
    t = F32(s / F32(254.0))
    m = rng.integers(-126, 126, size=d).astype(F32)
    half2 = (s * k + t * (m + F32(0.5))).astype(F32)
    half2[0], half2[1] = s * F32(127.0), s * k[1] + s * F32(0.5)      # the scale's own element; one residual of s / 2 = 127 t
    out["half steps of the second plane"] = half2
    out["exactly representable in the first plane"] = (F32(2.0 ** -9) * k).astype(F32)
    single = (F32(2.0 ** -9) * k).astype(F32)
    single[7] += F32(2.0 ** -11)
    out["a single non-zero in the residual"] = single
    return out


@pytest.fixture(scope="module", params=[384, 768])
def corpus(request):
    d = request.param
    planted = planted_rows(d)
    x = np.concatenate([unit_rows(1500, d, 40 + d), np.stack(list(planted.values()))]).astype(F32)
    q = unit_rows(12, d, 90 + d)
    q[1] = x[3]                                    # a query that is a row
    q[2] = planted["half steps of the second plane"] / np.linalg.norm(planted["half steps of the second plane"])
    q[3] = np.sign(x[-1]) / np.sqrt(d)             # every coordinate at the query's absmax: l = 0 throughout
    return d, x, q.astype(F32), list(planted)


def _true_error(x, i, s, j, t):
    y = s.astype(np.longdouble)[:, None] * i.astype(np.longdouble) + t.astype(np.longdouble)[:, None] * j.astype(np.longdouble)
    return np.sqrt(((y - x.astype(np.longdouble)) ** 2).sum(axis=1)).astype(F64)


# ------------------------------------------------------------------------------------------------ the claims
@pytest.mark.parametrize("rows", ["unit", "all"])
def test_error_norm_and_score_bound_hold_for_every_row(corpus, rows):
    """e2_r >= the true two-plane error and |s~2 - s^| <= eps2'_q, over i.i.d. unit rows alone (the margin the workload sees) and
    with the planted rows among them (X, e_max and e2_max are then the huge row's: a loose margin, but the planted rows' own
    roundings are in it)."""
    d, x, q, names = corpus
    if rows == "unit":
        x = x[:1500]
    i, s, er = plane1(x)
    j, t, e2r, e2_f64 = plane2(x, i, s)
    true = _true_error(x, i, s, j, t)
    assert (e2r.astype(F64) >= true).all(), "e2_r is short"
    assert (e2r.astype(F64) <= true * (1 + 4e-6) + 1e-45).all(), "e2_r is the measured error rounded up, not a looser figure"
    assert (e2r <= F32(0.12) * er + F32(1e-30)).all(), "the residual's error is a ninth of the first plane's at d <= 768"
    X = np.linalg.norm(x.astype(F64), axis=1).max()
    h, l, a, qn, cq, m2, m2r = stage(q, np.nextafter(F32(X), F32(np.inf)), er.max(), e2r.max())
    sc, lb, s1, s2, m = rescreen(i, s, er, j, t, h, l, a, qn, cq)
    sr = rescore(x, q)
    eps2p = m2r.astype(F64) / 2.0
    off = np.abs(s2.astype(F64) - sr.astype(F64))
    print("d %d rows %s: e2_max %.3e  eps2' %.3e .. %.3e  worst |s~2 - s^| %.3e (%.1f %% of eps2')"
          % (d, rows, e2r.max(), eps2p.min(), eps2p.max(), off.max(), 100 * (off / eps2p[None, :]).max()))
    assert (off <= eps2p[None, :]).all(), "a pair outside the residual tier's margin"
    # ... and the first tier's own claim, on the way: s^ in [l_r, l_r + 2 m_r]
    assert (sr >= lb).all() and (sr.astype(F64) <= lb.astype(F64) + 2.0 * m.astype(F64)).all()
    if rows == "unit":
        # the tier is worth having: its uniform margin is far inside the first tier's per-row margins and the bf16 screen's
        assert (m2r < F32(0.12) * m2).all() and eps2p.max() < 4.0e-4


def test_planted_rows_round_as_described(corpus):
    d, x, q, names = corpus
    i, s, er = plane1(x)
    j, t, e2r, _ = plane2(x, i, s)
    at = {name: 1500 + k for k, name in enumerate(names)}
    r = at["exactly representable in the first plane"]
    assert er[r] == 0 and t[r] == 0 and not j[r].any() and e2r[r] == 0, "degenerate row: t_r = 0, j = 0, e2_r = 0"
    r = at["a single non-zero in the residual"]
    assert np.count_nonzero(j[r]) == 1 and abs(int(j[r, 7])) == 127
    assert e2r[r] <= 2.0 ** -22 * 2.0 ** -11, "127 f32(rho / 127) is rho to an ulp or two, and e2_r says so"
    r = at["one huge element"]
    assert np.count_nonzero(i[r]) == 1 and i[r, 5] == 127, "the first plane holds the huge element alone"
    assert np.count_nonzero(j[r]) > d // 2, "the second plane holds the rest of the row"
    r = at["half steps of the first plane"]
    assert (np.abs(np.abs(x[r, 1:].astype(F64) / s[r] - i[r, 1:]) - 0.5) < 1e-6).all(), "every coordinate but the scale's sits on a half step"
    assert np.abs(j[r, 1:]).min() == 127, "... so every residual is +- s / 2: the second plane's end of range"
    r = at["half steps of the second plane"]
    frac = np.abs((x[r].astype(F64) - F64(s[r]) * i[r]) / F64(t[r]))
    assert (np.abs(frac[2:] - np.floor(frac[2:]) - 0.5) < 2e-2).all(), "the residuals sit on the second plane's half steps"


def test_recovery_of_the_first_score_from_its_key():
    """s' = f32(f32(s~ - m) + m) against s~: within 2^-23 (|s~| + m), the term eps2' carries; hand values at both ends."""
    rng = np.random.default_rng(3)
    sc = np.concatenate([rng.standard_normal(200000).astype(F32), (rng.standard_normal(200000) * 1e-3).astype(F32)])
    m = np.abs(np.concatenate([rng.standard_normal(200000) * 1e-2, rng.standard_normal(200000)])).astype(F32)
    s1 = ((sc - m).astype(F32) + m).astype(F32)
    slack = 2.0 ** -23 * (np.abs(sc.astype(F64)) + m.astype(F64))
    assert (np.abs(s1.astype(F64) - sc.astype(F64)) <= slack).all()
    # m of s~'s size or smaller: the subtraction is exact or nearly so and the key gives s~ back (the workload: |s~| 0.13, m 0.008)
    a, b = F32(0.1328125), F32(0.0078125)
    assert F32(F32(a - b) + b) == a
    # m >> |s~|: the key keeps m's ulps only.  s~ = 3 2^-26, m = 1: l = -1 + 2^-24, s' = 2^-24, off by 2^-26 <= 2^-23 (1 + 3 2^-26)
    a, b = F32(3 * 2.0 ** -26), F32(1.0)
    lb = F32(a - b)
    assert lb == F32(-1.0 + 2.0 ** -24) and F32(lb + b) == F32(2.0 ** -24)
    assert abs(F64(F32(lb + b)) - F64(a)) == 2.0 ** -26
    # a tie on the way down and on the way up (round to even both times): s~ = 1 + 2^-23, m = 2^-24
    a, b = F32(1.0 + 2.0 ** -23), F32(2.0 ** -24)
    lb = F32(a - b)
    assert lb == F32(1.0) and F32(lb + b) == F32(1.0), "1 + 2^-24 ties down to 1: off by one ulp of 1"
    assert abs(F64(F32(lb + b)) - F64(a)) == 2.0 ** -23 <= 2.0 ** -23 * (F64(a) + F64(b))


def test_integer_sums_fit_i32():
    """S2 = 128 sum j h + sum j l is exact in i32: d 127^2 129 < 2^31 at the largest d instantiated."""
    assert 768 * 127 * 127 * 129 < 2 ** 31
