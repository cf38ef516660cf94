"""The residual tier of the int8 route on the device, step by step, against the numpy models its bound is proven on
(tests/test_residual_plane_bound.py; DESIGN 4.1a "Bound of the residual tier").

HybridIndex.residual_rescreen (an internal export: oi_internal_residual_rescreen) runs the two product launchers -- the int8
staging (cosine_screen_i8.hip: i8s_stage_query_row) and the residual rescreen (screen_i8_residual.hip: i8r_rescreen_kernel) -- over
keys and counts the test chooses and copies back what they wrote:

  a. the staged words against `stage`: a, h, l bit for bit; |q^|, c_q, m2 and 2 eps2' not short of their f64 values recomputed from
     the device's own a, h, l, X, e_max and e2_max, and within 1e-5 of numpy's; queries without a bound; padding rows;
  b. the rescreened keys bit for bit against `rescreen`'s chain (single f32 operations on the device: equality is the bar; a
     differing element is re-derived in exact rational arithmetic for the failure message), every slot at or past a count untouched;
  c. the claim itself on the device's numbers: |s~2 - s^| <= eps2', s^ in [l_r, l_r + 2 m_r], s^ = `rescore`; and `rescore`
     against the scores a screened search lists, bit for bit;
  d. the probe: repeatable, the same through a view, no workspace of a search, refused without the plane.

Corpus: n = 4 200 (test_gpu_residual_plane._rows: unit rows, the bound test's planted rows at the end, the huge one long) and a zero
row; d 384 and 768 (24 and 48 active lanes).  COUNTS is the table of survivor counts around the kernel's step of 1 024; the test
without a GPU at the top runs a mirror of the kernel's two-deep loop over it and asserts that it reaches every branch outcome.

Seen on an MI355X (the tests print the figures): |q^|, c_q, m2 and 2 eps2' equal numpy's `stage` bit for bit (relative gap 0); the
worst |s~2 - s^| is 9.1 % of eps2' at d = 384 and 6.4 % at d = 768, over 62 000 pairs each."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from test_gpu_prefilter import _forward, _index
from test_gpu_residual_plane import _rows
from test_gpu_search_tail_edges import key_f32_bits, rank_keys
from test_residual_plane_bound import F32, F64, fma32, plane1, plane2, rescore, rescreen, stage, unit_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
VOCAB = 50
N = 4200
ZERO_ROW = 7
STRIDE = 16384                       # OI_I8_CARRY: the int8 route's carry, 16 trips of every wave
# survivors per query: both sides of every multiple of the step the waves' trip counts change at, a ragged and a full last trip on
# either register set, the whole carry and a count past it (clamped)
COUNTS = [0, 1, 3, 4, 5, 1023, 1024, 1025, 1028, 1029, 2047, 2048, 2049, 3071, 3072, 3073, 4097, 5121, STRIDE, STRIDE + 3616]
BASES = [0, 1000, 2 ** 32 - 1 - N]


# ==================================================================================================== the loop, without a GPU
def launch_waves():
    """Waves per query of oi_launch_rescreen_residual, read off the launch."""
    src = open(os.path.join(ROOT, "openintel_amd", "csrc", "screen_i8_residual.hip")).read()
    m = re.search(r"hipLaunchKernelGGL\(i8r_rescreen_kernel, dim3\((\d+), n_queries\), dim3\((\d+)\)", src)
    assert m, "the launch of i8r_rescreen_kernel is no longer written as this test reads it"
    return int(m.group(1)) * int(m.group(2)) // 64


def loop_trace(wave, count, n_waves, cap=STRIDE):
    """i8r_rescreen_kernel's pipelined loop for one wave: (events, break taken), None for a wave that returns at once.
    Events: ("keys", at), ("stage", set, at), ("finish", set, at, slots written)."""
    c = min(count, cap)
    step, i0 = 4 * n_waves, 4 * wave
    if i0 >= c:
        return None
    ev, kn = [], [None]

    def keys(at):
        kn[0] = at
        ev.append(("keys", at))

    def stage_(reg, at):
        assert kn[0] == at, "a trip is staged from keys read for another"
        ev.append(("stage", reg, at))

    def finish(reg, at):
        staged = [e for e in ev if e[0] == "stage" and e[1] == reg]
        assert staged and staged[-1][2] == at, "a trip is finished from a register set staged for another"
        ev.append(("finish", reg, at, tuple(at + u for u in range(4) if at + u < c)))

    keys(i0)
    stage_("A", i0)
    more = i0 + step < c
    if more:
        keys(i0 + step)
    while True:
        if more:
            stage_("B", i0 + step)
        more2 = more and i0 + 2 * step < c
        if more2:
            keys(i0 + 2 * step)
        finish("A", i0)
        if not more:
            return ev, 1
        i0 += step
        if more2:
            stage_("A", i0 + step)
        more = more2 and i0 + 2 * step < c
        if more:
            keys(i0 + 2 * step)
        finish("B", i0)
        if not more2:
            return ev, 2
        i0 += step


def test_count_table_reaches_every_outcome_of_the_pipelined_loop():
    n_waves = launch_waves()
    assert STRIDE == int(re.search(r"#define OI_I8_CARRY (\d+)u", open(os.path.join(ROOT, "openintel_amd", "csrc", "oi_internal.h")).read()).group(1))
    breaks, trips, ragged = set(), set(), set()
    for count in COUNTS:
        written = []
        for wave in range(n_waves):
            t = loop_trace(wave, count, n_waves)
            if t is None:
                assert 4 * wave >= min(count, STRIDE)
                continue
            ev, brk = t
            fin = [e for e in ev if e[0] == "finish"]
            assert [e[1] for e in fin] == ["A", "B"] * (len(fin) // 2) + ["A"] * (len(fin) % 2), "the register sets take turns"
            assert all(len(e[3]) == 4 for e in fin[:-1]), "only a wave's last trip is ragged"
            assert len([e for e in ev if e[0] == "stage"]) == len(fin) and len([e for e in ev if e[0] == "keys"]) == len(fin)
            breaks.add(brk)
            trips.add(len(fin))
            if len(fin[-1][3]) < 4:
                ragged.add(fin[-1][1])
            for e in fin:
                written += e[3]
        assert sorted(written) == list(range(min(count, STRIDE))), "count %d: every survivor's slot once, no other" % count
    assert breaks == {1, 2}, "a wave stops at each of the two breaks"
    assert {1, 2, 3, 4, 5, 16} <= trips, trips
    assert ragged == {"A", "B"}, "a ragged final trip on either register set"


# ==================================================================================================== exact arithmetic
def round_f32(v: Fraction) -> Fraction:
    """The f32 nearest to v, ties to even (normal range)."""
    if v == 0:
        return v
    sign, v = (-1 if v < 0 else 1), abs(v)
    e = v.numerator.bit_length() - v.denominator.bit_length() - 24
    while v >= Fraction(2) ** (e + 24):
        e += 1
    while v < Fraction(2) ** (e + 23):
        e -= 1
    assert -149 < e < 104
    s = v / Fraction(2) ** e                       # in [2^23, 2^24)
    n, r = divmod(s.numerator, s.denominator)
    half = Fraction(r, s.denominator)
    if half > Fraction(1, 2) or (half == Fraction(1, 2) and n & 1):
        n += 1
    return sign * n * Fraction(2) ** e


def exact_s2(lb, er, qn, cq, S2, t, qa):
    """The rescreen's chain for one survivor with every step rounded once, in rational arithmetic: (m, s', s~2) as floats."""
    fr = lambda v: Fraction(float(v))
    m = round_f32(fr(er) * fr(qn) + fr(cq))
    s1 = round_f32(fr(lb) + m)
    prod = round_f32(round_f32(Fraction(int(S2))) * round_f32(fr(t) * fr(qa)))
    return float(m), float(s1), float(round_f32(s1 + prod))


def test_fma32_rounds_once():
    """The model's fma against rational arithmetic: random operands, and a sum an f64 addition would carry onto an f32 tie."""
    rng = np.random.default_rng(11)
    x, y = rng.standard_normal(4000).astype(F32), rng.standard_normal(4000).astype(F32)
    z = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 3, 4000)).astype(F32)
    x[0], y[0], z[0] = F32(1 + 2.0 ** -23), F32(1 - 2.0 ** -23), F32(2.0 ** 24 + 2)     # 2^24 + 3 - 2^-46: just below the tie
    x[1], y[1], z[1] = x[0], -y[0], -z[0]
    got = fma32(x, y, z)
    want = np.array([float(round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))) for a, b, c in zip(x, y, z)], F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got[0] == F32(2.0 ** 24 + 2) and got[1] == -got[0]
    assert F32(F64(x[0]) * F64(y[0]) + F64(z[0])) == F32(2.0 ** 24 + 4), "(the twice-rounded sum this replaces is an ulp off here)"


# ==================================================================================================== the corpus and the queries
def corpus_rows(d):
    x = _rows(N, d)
    x[ZERO_ROW] = 0.0
    return x


KINDS = ["unit", "S2 max +", "S2 max -", "S2 large, rounded", "a row", "half steps", "at absmax", "largest negative", "unit 2",
         "zero", "inf", "nan", "tiny"]
BAD = {"zero", "inf", "nan", "tiny"}
GOOD = [k for k in KINDS if k not in BAD]


def query_kinds(d, x, j):
    """{kind: f32 query}: the bound test's queries, the pair that drives |S2| to its largest value, and queries without a bound."""
    from test_residual_plane_bound import planted_rows
    u = unit_rows(4, d, 90 + d)
    half2 = planted_rows(d)["half steps of the second plane"]
    sj = np.where(j[N - 4] >= 0, 1.0, -1.0).astype(F32)      # the first-plane half-step row: |j| = 127 but at the scale's element
    neg = u[2].copy()
    neg[5] = -0.5
    bad_inf, bad_nan = u[3].copy(), u[3].copy()
    bad_inf[17], bad_nan[d - 1] = np.inf, np.nan
    # ... and beside that pair (l = 0 throughout: S2 a multiple of 128, its conversion exact) one with h = +-127 still and l in
    # [-58, 0]: |S2| stays above 2^30 and its low bits are set, so f32(S2) IS a rounding of a 31-bit integer
    delta = np.random.default_rng(d).uniform(0.0, 0.45, size=d)
    delta[0] = 0.0
    near = (sj.astype(F64) * (127.0 - delta) / 127.0 / np.sqrt(d)).astype(F32)
    out = {"unit": u[0], "S2 max +": sj / F32(np.sqrt(d)), "S2 max -": -sj / F32(np.sqrt(d)), "S2 large, rounded": near, "a row": x[3].copy(),
           "half steps": (half2 / np.linalg.norm(half2)).astype(F32), "at absmax": (np.sign(x[-1]) / np.sqrt(d)).astype(F32),
           "largest negative": neg, "unit 2": u[1], "zero": np.zeros(d, F32), "inf": bad_inf, "nan": bad_nan,
           "tiny": (u[3] * F32(1e-13)).astype(F32)}
    assert list(out) == KINDS
    return {k: np.ascontiguousarray(v, dtype=F32) for k, v in out.items()}


class Case:
    """One dim: the rows and their planes (numpy), a context and an index at base 0, the queries' models from the device's own
    staged words.  Made once per module and dim; nothing in it is written after that."""

    def __init__(self, d):
        import openintel_amd as oi
        from openintel_amd import _lib
        self.d = d
        self.x = corpus_rows(d)
        self.i, self.s, self.er = plane1(self.x)
        self.j, self.t, self.e2r, _ = plane2(self.x, self.i, self.s)
        self.ctx = oi.HipContext(0)
        self.ctx.set_cosine_mode(_lib.OI_COSINE_SCREEN)
        self.idx = self.make(0)
        assert self.idx.long_rows() == 1, "the planted huge row is the one long row"
        self.long = N - 5
        self.kinds = query_kinds(d, self.x, self.j)
        # the batch of b and c: one query per count, the good kinds in turn, and a query without a bound at the end
        self.names = [GOOD[b % len(GOOD)] for b in range(len(COUNTS))] + ["inf"]
        self.counts = np.array(COUNTS + [5], np.uint32)
        self.q = np.stack([self.kinds[k] for k in self.names])
        self.good = np.array([k not in BAD for k in self.names])
        B = self.q.shape[0]
        st = self.idx.residual_rescreen(self.q, np.zeros((B, 1), U64), np.zeros(B, np.uint32))
        self.staged = st
        qf = st["qf"][:, :B]
        h, l, a, qn, cq = st["h"][:B], st["l"][:B], qf[0], qf[1], qf[2]
        # the model of every (row, query) from the DEVICE's words (a tells on them): s~, l_r, s', s~2, m_r and the second product
        self.sc, self.lb, self.s1, self.s2, self.m = rescreen(self.i, self.s, self.er, self.j, self.t, h, l, a, qn, cq)
        self.S2 = 128 * (self.j.astype(np.int64) @ h.astype(np.int64).T) + self.j.astype(np.int64) @ l.astype(np.int64).T
        self.qa = (a * F32(0.0078125)).astype(F32)
        self.prod = (self.S2.astype(F32) * (self.t[:, None] * self.qa[None, :]).astype(F32)).astype(F32)
        assert np.array_equal(self.expect(self.lb).view(np.uint32), self.s2.view(np.uint32)), "this file's chain is rescreen's"
        # s^ of the distinct good queries, once
        uniq = sorted({k for k in self.names if k not in BAD}, key=KINDS.index)
        sr = rescore(self.x, np.stack([self.kinds[k] for k in uniq]))
        self.sr = np.stack([sr[:, uniq.index(k)] if k in uniq else np.full(N, np.nan, F32) for k in self.names], axis=1)

    def make(self, base):
        terms, offs = _forward(np.random.default_rng(N), N, VOCAB)
        idx = _index(self.ctx, self.x, terms, offs, VOCAB, base=base)
        assert idx.residual_plane() is not None
        return idx

    def expect(self, lb, rows=None, b=None):
        """s~2 from a key's score lb: f32(f32(lb + m) + prod).  lb [n, B], or lb [k] with rows [k] of query b."""
        m, prod = (self.m, self.prod) if rows is None else (self.m[rows, b], self.prod[rows, b])
        return ((lb + m).astype(F32) + prod).astype(F32)

    def close(self):
        self.idx.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(d):
        if d not in made:
            made[d] = Case(d)
        return made[d]
    yield get
    for c in made.values():
        c.close()


# ==================================================================================================== a. the staged words
def _check_staged(C, names, out, gaps):
    d, B = C.d, len(names)
    q = np.stack([C.kinds[k] for k in names])
    n_padded = (B + 31) & ~31
    h, l, qf, eps2r = out["h"], out["l"], out["qf"], out["eps2r"]
    assert h.shape == (n_padded, d) and l.shape == (n_padded, d) and qf.shape == (4, n_padded) and eps2r.shape == (B,)
    X, em, e2m = F64(out["X"]), F64(out["e_max"]), F64(out["e2_max"])
    bad = np.array([k in BAD for k in names])
    assert (out["gate"] != 0) == bool(bad.any()), "the gate word opens for a query without a bound, and only then"
    # padding rows: zeros, a finite margin
    assert not h[B:].any() and not l[B:].any() and not qf[:3, B:].any() and np.isfinite(qf[3, B:]).all()
    # queries without a bound
    assert not qf[:3, :B][:, bad].any() and np.isposinf(qf[3, :B][bad]).all() and np.isposinf(eps2r[bad]).all()
    nofin = np.array([k in ("zero", "inf", "nan") for k in names])
    assert not h[:B][nofin].any() and not l[:B][nofin].any(), "a = 0: both planes of the query are zeros"
    # h and l of every query with a scale (the tiny one too: it is staged, then refused on its norm), a of the good ones
    sel = np.nonzero(~nofin)[0]
    if sel.size == 0:
        return
    hm, lm, am, qnm, cqm, m2m, m2rm = stage(q[sel], out["X"], out["e_max"], out["e2_max"])
    assert np.array_equal(h[sel], hm), "h differs from the model at queries %s" % [names[b] for b in sel[(h[sel] != hm).any(axis=1)]]
    assert np.array_equal(l[sel], lm), "l differs from the model at queries %s" % [names[b] for b in sel[(l[sel] != lm).any(axis=1)]]
    ok = ~bad[sel]
    g, mg = sel[ok], np.nonzero(ok)[0]
    if g.size == 0:
        return
    a, qn, cq, m2, m2r = qf[0, g], qf[1, g].astype(F64), qf[2, g].astype(F64), qf[3, g].astype(F64), eps2r[g].astype(F64)
    assert np.array_equal(a.view(np.uint32), am[mg].view(np.uint32)), "a differs from the model"
    qh = a.astype(F64)[:, None] * (h[g].astype(F64) + l[g].astype(F64) * 0.0078125)
    qn_true = np.sqrt((qh * qh).sum(axis=1))
    en_true = np.sqrt(((qh - q[g].astype(F64)) ** 2).sum(axis=1))
    assert (qn >= qn_true).all() and (qn <= qn_true * (1 + 4e-6)).all(), "|q^| is its f64 norm rounded up, and no more"
    rnd = 2.0 ** -18 + d * 2.0 ** -22
    assert (cq >= X * en_true + rnd * (X + em) * (qn_true + en_true)).all(), "c_q is short"
    assert (m2 >= 2.0 * (em * qn + cq)).all(), "the int8 tier's margin is short"
    rec = 2.0 ** -21 * ((X + em) * qn + (em * qn + cq))
    assert (m2r >= 2.0 * (e2m * qn + cq + rec)).all(), "the residual tier's margin is short"
    for name, dev, model in (("qn", qn, qnm[mg]), ("cq", cq, cqm[mg]), ("m2", m2, m2m[mg]), ("eps2r", m2r, m2rm[mg])):
        rel = np.abs(dev - model.astype(F64)) / model.astype(F64)
        gaps[name] = max(gaps.get(name, 0.0), float(rel.max()))
        assert (rel <= 1e-5).all(), "%s is off numpy's by %.3e" % (name, rel.max())


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 32, 33, 64])
@pytest.mark.parametrize("d", [384, 768])
def test_staged_words_equal_the_model(cases, d, B):
    C = cases(d)
    gaps = {}
    if B == 1:
        batches = [[k] for k in KINDS]
    else:
        # every kind, the bad ones apart from each other, the rest unit queries; one batch of good queries alone (gate shut)
        mixed = (KINDS + ["unit", "unit 2"] * 32)[:B]
        mixed[-1] = "nan"
        batches = [mixed, (GOOD * 8)[:B]]
    for names in batches:
        q = np.stack([C.kinds[k] for k in names])
        out = C.idx.residual_rescreen(q, np.zeros((len(names), 1), U64), np.zeros(len(names), np.uint32))
        assert np.array_equal(out["keys"], np.zeros((len(names), 1), U64)), "a count of 0: no key is written"
        _check_staged(C, names, out, gaps)
    print("d %d B %d: worst relative gap to numpy's stage: %s" % (d, B, ", ".join("%s %.2e" % kv for kv in sorted(gaps.items()))))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [384, 768])
def test_scalars_the_staging_read(cases, d):
    """X is the largest norm of the rows that are not long (the device's f32 figure: within a few ulps of numpy's f64 one), e_max
    and e2_max the largest error norms of those rows as the planes' models have them."""
    C = cases(d)
    st = C.staged
    keep = np.ones(N, bool)
    keep[C.long] = False
    X = np.linalg.norm(C.x[keep].astype(F64), axis=1).max()
    assert abs(F64(st["X"]) - X) <= 1e-5 * X
    assert st["e_max"] == C.er[keep].max() and st["e2_max"] == C.e2r[keep].max()
    if d == 768:
        b = C.names.index("S2 max +")
        assert abs(int(C.S2[N - 4, b])) == 128 * 127 * 127 * (d - 1) > 2 ** 30, "the pair drives |S2| to 31 bits"
        assert C.S2[N - 4, b] == -C.S2[N - 4, C.names.index("S2 max -")]
        r = int(C.S2[N - 4, C.names.index("S2 large, rounded")])
        assert 2 ** 30 <= r < 2 ** 31 and r % 128 and int(F32(r)) != r, "... and its neighbour's f32(S2) is a rounding"


# ==================================================================================================== b. the keys
SPECIAL_LB = [("-0.0", None), ("+0.0", F32(0.0)), ("negative", F32(-0.375)), ("1e30", F32(1e30))]


def _batch_keys(C, base, seed):
    """(keys [B, STRIDE], expected keys, per query: local rows [c], plain mask [c]) of the batch.  Slots below a count name rows
    with the model's lower bound as the score -- the rows every corpus edge sits at first, then random ones -- but for a doc on
    either side of the shard and four scores that are not the screen's; slots at and past a count hold a pattern."""
    rng = np.random.default_rng(seed)
    B = C.q.shape[0]
    first = [N - 4, 0, N - 1, C.long, N - 3, N - 2, ZERO_ROW]
    keys = rng.integers(1, 2 ** 63, size=(B, STRIDE), dtype=np.int64).astype(U64) | U64(1 << 63)
    want = keys.copy()
    rows_of, plain_of = [], []
    for b in range(B):
        c = int(min(C.counts[b], STRIDE))
        rows = np.concatenate([np.array(first, np.int64), rng.integers(0, N, size=max(0, c - len(first)))])[:c]
        docs = ((rows + base) & 0xFFFFFFFF).astype(np.uint32)
        lb = C.lb[rows, b].copy()
        plain = np.ones(c, bool)
        k_in = None
        if c >= 1023:
            at = 16
            outside = [base + N] + ([base - 1] if base else [])
            for doc in outside:                               # a doc past the shard's end, one below its base: score 0, the doc kept
                docs[at], lb[at], plain[at] = doc, F32(0.25), False
                at += 1
            k_in = rank_keys(lb, docs)
            for name, v in SPECIAL_LB:
                if v is None:                                 # (rank_keys makes +0.0 of it: the bits of -0.0 by hand)
                    k_in[at] = (U64(0x7FFFFFFF) << U64(32)) | U64(~docs[at] & np.uint32(0xFFFFFFFF))
                    lb[at] = F32(-0.0)
                else:
                    lb[at] = v
                    k_in[at] = rank_keys(lb[at:at + 1], docs[at:at + 1])[0]
                plain[at] = False
                at += 1
            s2 = C.expect(lb, rows, b)
            s2[16:16 + len(outside)] = F32(0.0)
        else:
            k_in = rank_keys(lb, docs)
            s2 = C.expect(lb, rows, b)
        keys[b, :c] = k_in
        want[b, :c] = rank_keys(s2, docs)
        plain &= rows != C.long
        rows_of.append((rows, docs, lb))
        plain_of.append(plain)
    return keys, want, rows_of, plain_of


def _explain(C, b, slot, rows_of, got_key, want_key, base):
    """A differing slot, decided in rational arithmetic."""
    rows, docs, lb = rows_of[b]
    if slot >= rows.size:
        return "query %d slot %d (past the count %d): written" % (b, slot, rows.size)
    r = int(rows[slot])
    qf = C.staged["qf"]
    m, s1, s2 = exact_s2(lb[slot], C.er[r], qf[1, b], qf[2, b], C.S2[r, b], C.t[r], C.qa[b])
    got = key_f32_bits(np.array([got_key >> U64(32)], np.uint64).astype(np.uint32)).view(F32)[0]
    want = key_f32_bits(np.array([want_key >> U64(32)], np.uint64).astype(np.uint32)).view(F32)[0]
    side = "the DEVICE holds the exact chain's value: the model is off" if F32(s2) == got else \
           "the MODEL holds the exact chain's value: the device is off" if F32(s2) == want else "neither holds the exact chain's value"
    return "query %d (%s, count %d) slot %d row %d doc %d: device %r (doc %d), model %r, exact chain m %r s' %r s~2 %r -- %s" % (
        b, C.names[b], C.counts[b], slot, r, docs[slot], got, ~np.uint32(got_key & U64(0xFFFFFFFF)), want, m, s1, s2, side)


@pytest.mark.gpu
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("d", [384, 768])
def test_rescreened_keys_equal_the_model_and_the_claim_holds(cases, d, base):
    """b and c over one ragged batch: every key below a count is rank_key(s~2, doc) of the model's chain bit for bit, every slot
    at or past it is untouched; then, on the device's own s~2 and margins, the claim the select behind this launch rests on."""
    C = cases(d)
    idx = C.idx if base == 0 else C.make(base)
    try:
        keys, want, rows_of, plain_of = _batch_keys(C, base, seed=d + base % 1000)
        out = idx.residual_rescreen(C.q, keys, C.counts)
    finally:
        if base:
            idx.close()
    got = out["keys"]
    assert out["gate"] != 0, "the batch holds a query without a bound"
    for name in ("h", "l", "qf", "eps2r"):
        assert np.array_equal(out[name].view(np.uint8), C.staged[name].view(np.uint8)), "staging does not depend on the keys or the base"
    diff = np.argwhere(got != want)
    assert diff.size == 0, "%d keys differ; the first:\n%s" % (
        len(diff), "\n".join(_explain(C, int(b), int(s), rows_of, got[b, s], want[b, s], base) for b, s in diff[:6]))
    # c. the claim, on what the device wrote
    worst, pairs = 0.0, 0
    for b in np.nonzero(C.good)[0]:
        rows, docs, lb = rows_of[b]
        p = plain_of[b]
        if not p.any():
            continue
        r = rows[p]
        s2 = key_f32_bits((got[b, :rows.size][p] >> U64(32)).astype(np.uint32)).view(F32).astype(F64)
        sr, eps = C.sr[r, b].astype(F64), F64(out["eps2r"][b]) / 2.0
        off = np.abs(s2 - sr)
        worst, pairs = max(worst, float((off / eps).max())), pairs + r.size
        assert (off <= eps).all(), "query %d (%s): a pair outside the residual tier's margin, %.3e against %.3e" % (b, C.names[b], off.max(), eps)
        assert (sr >= lb[p].astype(F64)).all() and (sr <= lb[p].astype(F64) + 2.0 * C.m[r, b].astype(F64)).all(), \
            "query %d (%s): s^ outside the first tier's [l_r, l_r + 2 m_r]" % (b, C.names[b])
    print("d %d base %d: worst |s~2_dev - s^| / (eps2r_dev / 2) = %.4f over %d pairs" % (d, base, worst, pairs))


@pytest.mark.gpu
@pytest.mark.parametrize("d,B", [(384, 9), (384, 33), (768, 9), (768, 33)])
def test_listed_scores_are_rescores(d, B):
    """`rescore` is the device's: a screened search over 1 000 rows at depth 1 000 lists every row, with the gate shut the scores
    are pf_rescore_kernel's, and they equal the model's f32 fma chain bit for bit."""
    import openintel_amd as oi
    from openintel_amd import _lib
    n = 1000
    x, q = unit_rows(n, d, 300 + d), unit_rows(B, d, 400 + d + B)
    ctx = oi.HipContext(0)
    try:
        ctx.set_cosine_mode(_lib.OI_COSINE_SCREEN)
        terms, offs = _forward(np.random.default_rng(n), n, VOCAB)
        idx = _index(ctx, x, terms, offs, VOCAB)
        rng = np.random.default_rng(B)
        qt, qo = rng.integers(0, VOCAB, size=2 * B).astype(np.uint32), np.arange(0, 2 * B + 1, 2, dtype=np.uint32)
        L = idx.search_lists(q, qt, qo, depth=n)
        assert ctx.profile_read("screen_gate")[0] == 0.0, "the search was screened and the gate stayed shut"
        sr = rescore(x, q)
        for b in range(B):
            assert L.cos_counts[b] == n
            docs = L.cos_docs[b][:n].astype(np.int64)
            assert np.array_equal(np.sort(docs), np.arange(n))
            assert np.array_equal(L.cos_scores[b][:n].view(np.uint32), sr[docs, b].view(np.uint32)), "query %d: a listed score is not rescore's" % b
        idx.close()
    finally:
        ctx.close()


# ==================================================================================================== d. the probe itself
def _same_bytes(a, b):
    for name in ("keys", "h", "l", "qf", "eps2r", "X", "e_max", "e2_max"):
        assert np.array_equal(np.atleast_1d(a[name]).view(np.uint8), np.atleast_1d(b[name]).view(np.uint8)), name
    assert a["gate"] == b["gate"]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [384, 768])
def test_probe_repeats_and_borrows_nothing(cases, d):
    import openintel_amd as oi
    from openintel_amd import _lib
    C = cases(d)
    keys, want, _, _ = _batch_keys(C, 0, seed=5)
    Bq = 33
    q = unit_rows(Bq, d, 77 + d)
    rng = np.random.default_rng(d)
    qt, qo = rng.integers(0, VOCAB, size=2 * Bq).astype(np.uint32), np.arange(0, 2 * Bq + 1, 2, dtype=np.uint32)
    before = C.idx.search_lists(q, qt, qo, depth=64)
    first = C.idx.residual_rescreen(C.q, keys, C.counts)
    after = C.idx.search_lists(q, qt, qo, depth=64)
    assert C.ctx.rescreen_state()[0] == 1, "the searches take the residual tail"
    for leg in ("cos", "bm25"):
        cb, ca = getattr(before, leg + "_counts"), getattr(after, leg + "_counts")
        assert np.array_equal(cb, ca) and cb.min() > 0
        for name in (leg + "_docs", leg + "_scores"):
            for b in range(Bq):
                assert np.array_equal(getattr(before, name)[b][:cb[b]].view(np.uint32), getattr(after, name)[b][:cb[b]].view(np.uint32)), (name, b)
    _same_bytes(first, C.idx.residual_rescreen(C.q, keys, C.counts))
    assert np.array_equal(first["keys"], want)
    c2 = oi.HipContext(0)
    try:
        c2.set_cosine_mode(_lib.OI_COSINE_SCREEN)
        v = C.idx.view(c2)
        _same_bytes(first, v.residual_rescreen(C.q, keys, C.counts))
        v.close()
    finally:
        c2.close()


@pytest.mark.gpu
def test_probe_is_refused_without_the_plane(cases):
    from openintel_amd import _lib
    C = cases(384)
    idx = C.make(0)
    try:
        assert idx.residual_plane(drop=True) is None
        keys, _, _, _ = _batch_keys(C, 0, seed=5)
        with pytest.raises(_lib.OiError, match="both int8 planes"):
            idx.residual_rescreen(C.q, keys, C.counts)
        with pytest.raises(_lib.OiError):
            idx.residual_rescreen(C.q, keys, C.counts, cap=STRIDE + 1)
    finally:
        idx.close()
    with pytest.raises(_lib.OiError, match="cap"):
        C.idx.residual_rescreen(C.q, keys, C.counts, cap=STRIDE + 1)
