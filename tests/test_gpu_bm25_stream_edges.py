"""The BM25 stream kernel (csrc/bm25_stream.hip: bm25_stream_kernel, the default BM25 kernel and the only one a filtered search
runs) at every chunk, ring, table and segment edge, bit for bit against the oracle.

The kernel is a per-wave state machine: a chunk table built with a lane scatter and a DPP max-scan, LDS-DMA chunks of 128
posting slots in a 4-slot ring ordered by counted waits, a seen / multi bitmap pair with a perfect-hash rank for the docs of
several runs, extra rounds from global memory past BS_CAP such docs, and small pool segments pruned in place by a radix
select.  A wrong guard at any of these drops or invents one document on some data only: nothing crashes, nothing slows down.

This module holds a pure-Python MIRROR of the kernel's geometry (Layout, window, ring_trace, plan / ranges, prune_trace), a
declared table of cases (GROUP_MAKERS: groups of one index each -> batches searched together -> Q rows, each row naming the
edges it is there for) and a CHECKLIST of every edge.
CPU tests prove through the mirror that every row reaches what it declares and that the table leaves no checklist item
without a case; GPU tests run every row against the oracle.

Construction rules (what makes a wrong kernel visible):
  * real f32 impacts: document lengths run from 1 to about 12 tokens and tf from 1 to 3, so a multi document's score is a
    non-associative f32 sum in query order.  The "ties" corpora are the exception: there equal lengths are the point;
  * planted victims: for a run under test, its first and its last document, and every document of the two neighbouring terms
    in id order (which no query of that run holds), are documents of length 1 holding that one token -- the highest impact of
    the block, so they pass every threshold and rank at the top.  A posting read one past the run's end (the next term's first
    posting) is then an extra document at the head of the list, a dropped first or last posting a missing one, a misaligned
    odd start either.  Neighbour terms have postings in every block, at block offsets no run under test uses, so the
    neighbour's posting names a document that does not hold the query term;
  * complete lists: every batch is also searched at depth 1024, which is the whole match set wherever at most 1024 docs match;
  * the reference is oracle.lib.bm25_scores + oracle.lib.topk(positive_only) (pinned to a numpy evaluation of the formula in
    test_oracle_retrieval.py); under a filter, the oracle's full score vector with the failing docs zeroed, then topk;
  * counts, doc ids and score bits are compared for equality.  Unfiltered batches also run BM25_WAVE and BM25_TAAT on the same
    index: the three lists must be byte-identical (a filtered search runs the stream kernel in every mode).

Not reachable, asserted in the mirror instead of a case: a run with e - cs = 1 and an odd start (e > s makes e - cs >= 2), and
a first-phase segment cap above 4096 (depth + 256 > 4096 needs a depth above OI_MAX_DEPTH)."""
import os
import re
from typing import NamedTuple

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openintel_amd", "csrc")

# ==================================================================== constants of the kernel (checked against the source below)
BS_BLOCK, BS_FINE = 32768, 16384
BS_WPB, BS_RING, BS_CAP, BS_STAGE, BS_MAX_Q = 2, 4, 256, 128, 128
BS_RUN_COST, BS_TASK_COST = 64, 384
OI_MAX_DEPTH = 1024
OI_BM25_FLOOR_RANKS = 4
FLOOR_RANKS = (16, 64, 256, 1024)
LDS_PER_CU = 160 * 1024
MI355X_CUS = 256
MAXB = -1                 # doc_id_base = 2^32 - 1 - n: the key holds ~doc
STREAM, WAVE, TAAT = 4, 3, 1          # HybridIndex.BM25_*


def lds_total(W: int = BS_BLOCK) -> int:
    """BsLds<W>::TOTAL."""
    words = W // 32
    off_acc = words * 10
    off_accdoc = off_acc + BS_CAP * 4
    off_stage = off_accdoc + BS_CAP * 4
    off_desc = off_stage + BS_STAGE * 8
    off_ring = (off_desc + 2 * 3 * 256 + 1023) & ~1023
    wave = off_ring + BS_RING * 1024
    return BS_WPB * wave + (BS_MAX_Q + 2) * 8 + BS_MAX_Q * 4


PER_CU = LDS_PER_CU // lds_total()


# ==================================================================== mirror: the index layout
class Layout:
    """bm25.hip: postings sorted by (term, doc), a doc holding a term twice is one posting; run(t, blk) = [s, e)."""

    def __init__(self, terms, offs, vocab):
        n = offs.size - 1
        self.n, self.vocab, self.nb = n, vocab, (n + BS_BLOCK - 1) // BS_BLOCK
        span = self.nb * BS_BLOCK
        doc = np.repeat(np.arange(n, dtype=np.int64), np.diff(offs.astype(np.int64)))
        key = np.unique(terms.astype(np.int64) * span + doc)
        self.pdoc = key % span
        cell = (key // span) * self.nb + (self.pdoc >> 15)
        cnt = np.bincount(cell, minlength=vocab * self.nb)
        self.start = np.concatenate([[0], np.cumsum(cnt)])
        self.n_postings = int(key.size)

    def run(self, t, blk):
        return int(self.start[t * self.nb + blk]), int(self.start[t * self.nb + blk + 1])

    def df(self, t):
        return int(self.start[(t + 1) * self.nb] - self.start[t * self.nb])

    def docs(self, t, blk):
        s, e = self.run(t, blk)
        return self.pdoc[s:e]


class Run(NamedTuple):
    pos: int      # position of the term in the query (the lane of the run, when < 64)
    term: int
    s: int
    e: int
    n: int        # chunks
    lane: int     # lane of its first chunk: the exclusive prefix of n


class Win(NamedTuple):
    runs: tuple
    T: int
    C: int
    slow: bool
    M: int
    rounds: int   # extra rounds from global memory
    multi: np.ndarray   # block offsets of the multi docs, ascending = rank order


def window(L: Layout, q, blk) -> Win:
    """build_table + the sweep of one (query, block): product build, one window per block."""
    runs, C, docs = [], 0, []
    for pos, t in enumerate(q):
        if t >= L.vocab:
            continue
        s, e = L.run(t, blk)
        n = (e - (s & ~1) + 127) >> 7 if e > s else 0
        runs.append(Run(pos, t, s, e, n, C))
        C += n
        docs.append(L.pdoc[s:e])
    T = len(q)
    if docs:
        u, c = np.unique(np.concatenate(docs), return_counts=True)
        multi = (u[c >= 2] & (BS_BLOCK - 1)).astype(np.int64)
    else:
        multi = np.zeros(0, np.int64)
    M = int(multi.size)
    return Win(tuple(runs), T, C, T > 64 or C > 64, M, max(0, -(-M // BS_CAP) - 1), multi)


def ring_trace(wins):
    """The ring over the consecutive windows a wave walks for ONE query (wins: [(C, slow)]): what `ahead` is at every
    wait_oldest, and whether chunks of the next window were issued under the current one.  -> (branches, ran_ahead)"""
    R, ahead, branches, ran_ahead = BS_RING, 0, set(), []
    icur = 0
    for w, (C, slow) in enumerate(wins):
        nC = 0
        if w + 1 < len(wins) and not wins[w + 1][1]:
            nC = wins[w + 1][0]
        inxt = 0
        if slow:
            assert ahead == 0 and icur == 0
        elif C:
            V = 2 * C
            while ahead < R and icur < V:
                icur += 1; ahead += 1
            for _ in range(V):
                assert ahead >= 1
                branches.add("full" if ahead >= R else "half" if ahead >= R // 2 else "drain")
                ahead -= 1
                if icur < V:
                    icur += 1; ahead += 1
                elif inxt < 2 * nC:
                    inxt += 1; ahead += 1
        ran_ahead.append(inxt)
        icur = inxt
    assert ahead == 0
    return branches, ran_ahead


# ==================================================================== mirror: passes, plan and ranges
def seg_cap(depth: int, first_phase: bool) -> int:
    """oi_bm25_stream_seg_cap."""
    c = depth + 256
    return max(c, 4096) if first_phase else c


class Plan(NamedTuple):
    floors: bool
    first: int         # blocks of the first launch
    phases: int
    cap1: int
    cap2: int
    pass_q: int
    q_begins: tuple


def plan(nb: int, B: int, depth: int, filtered: bool) -> Plan:
    """search.hip: bm25_stream (default knobs: one phase with floors, a first phase of nb / 8 blocks past 48 without)."""
    floors = not filtered
    first = nb if floors else (max(8, nb // 8) if nb > 48 else nb)
    cap1, cap2 = seg_cap(depth, not floors), seg_cap(depth, False)
    sstride = OI_MAX_DEPTH + max(first * cap1, nb * cap2)
    p = max(1, min((2 << 30) // 8 // sstride, min(B, BS_MAX_Q)))
    return Plan(floors, first, 1 if first == nb else 2, cap1, cap2, p, tuple(range(0, B, p)))


def launch_geometry(nbh: int, nq: int, num_cus: int):
    """oi_launch_bm25_stream -> (n_tasks, workgroups, waves = ranges)."""
    n_tasks = nbh * nq
    wgs = min((n_tasks + BS_WPB - 1) // BS_WPB, PER_CU * num_cus)
    return n_tasks, wgs, max(wgs * BS_WPB, min(n_tasks, wgs * BS_WPB))


def units(L: Layout, queries):
    """bm25_plan_kernel: the weight of one block of each query."""
    out = []
    for q in queries:
        wsum = sum(L.df(t) for t in q if t < L.vocab)
        runs = sum(1 for t in q if t < L.vocab and L.df(t))
        out.append(min(wsum // max(L.nb, 1) + BS_RUN_COST * runs + BS_TASK_COST, 1 << 24))
    return out


def ranges(unit, nbh: int, G: int):
    """The kernel's cut + locate: the tasks [(query, block)] of each of the G ranges, in the order a wave walks them."""
    nq = len(unit)
    cum = np.concatenate([[0], np.cumsum(unit)]).astype(object)
    total = int(cum[nq]) * nbh

    def locate(P):
        if P >= total:
            return nq, 0
        lo = max(i for i in range(nq) if int(cum[i]) * nbh <= P)
        u, off = int(cum[lo + 1] - cum[lo]), P - int(cum[lo]) * nbh
        b = (off + u - 1) // u
        return (lo + 1, 0) if b >= nbh else (lo, b)

    def cut(c):
        return total // G * c + total % G * c // G

    out = []
    for ch in range(G):
        r0, b0 = locate(cut(ch))
        r1, b1 = (nq, 0) if ch + 1 == G else locate(cut(ch + 1))
        tasks = []
        for r in range(r0, min(r1, nq - 1) + 1):
            bA, bB = (b0 if r == r0 else 0), (b1 if r == r1 else nbh)
            tasks += [(r, b) for b in range(bA, bB)]
        out.append(tasks)
    return out


def prune_trace(K: int, cap: int, depth: int):
    """A segment that is handed K keys, none held back by a threshold (true up to the first prune whatever the scores; true
    throughout when every score ties, since a prune then raises the threshold to exactly that score): the prunes, as
    ("flush" | "end", out_n when it ran)."""
    out_n, prunes = 0, []
    for _ in range(K // 64):
        if out_n + 64 > cap:
            prunes.append(("flush", out_n)); out_n = min(depth, out_n)
        out_n += 64
    rem = K % 64
    if rem and out_n + rem > cap:
        prunes.append(("end", out_n)); out_n = min(depth, out_n)
    assert out_n + rem <= cap
    return prunes


# ==================================================================== corpus builder
class Corpus:
    """A forward index built from posting sets.  Block offsets ("dibs") are handed out once for ALL blocks: a dib a term took
    is free in no block, so the same offsets can be reused block after block and a posting of another block or term, read by
    mistake, names a document that does not hold the term under test."""

    def __init__(self, n, vocab, seed, filler=0):
        self.n, self.vocab, self.filler = n, vocab, filler
        self.nb = (n + BS_BLOCK - 1) // BS_BLOCK
        self.D, self.T, self.F = [], [], []
        self.victim = np.zeros(n, bool)
        self.length = np.zeros(n, np.int64)          # 0: 1..12 tokens from the hash
        self.free = np.ones(BS_BLOCK, bool)
        self.hash = np.random.default_rng(seed).integers(0, 1 << 30, size=n)
        self.parity = []

    def take(self, k, stride=1):
        f = np.flatnonzero(self.free)[:k * stride:stride]
        assert f.size == k, "out of block offsets"
        self.free[f] = False
        return f

    def reserve(self, dibs):
        self.free[np.asarray(dibs)] = False

    def put(self, term, blk, dibs, victims=None, tf=None):
        docs = blk * BS_BLOCK + np.asarray(dibs, dtype=np.int64)
        docs = docs[docs < self.n]
        if docs.size == 0:
            return docs
        f = 1 + ((self.hash[docs] >> 3) + term) % 3 if tf is None else np.full(docs.size, tf, np.int64)
        if victims == "ends":
            self.victim[[docs.min(), docs.max()]] = True
        elif victims == "all":
            self.victim[docs] = True
        self.D.append(docs); self.T.append(np.full(docs.size, term, np.int64)); self.F.append(f)
        return docs

    def want_parity(self, term, blk, odd, spare_term):
        """finish() gives `spare_term` (< term, never queried) one more posting if run (term, blk) would start on the other parity"""
        self.parity.append((term, blk, odd, spare_term))

    def finish(self):
        D, T, F = np.concatenate(self.D), np.concatenate(self.T), np.concatenate(self.F)
        assert np.unique(T * self.n + D).size == D.size, "a (term, doc) pair put twice"
        assert (T != self.filler).all()
        F = np.where(self.victim[D], 1, F)
        held = np.bincount(D, minlength=self.n)
        assert (held[self.victim] == 1).all(), "a victim holds one token"
        c = np.bincount(D, weights=F, minlength=self.n).astype(np.int64)
        fill = self.hash % 7
        fill = np.where((c == 0) & (fill == 0), 1, fill)
        fixed = self.length > 0
        assert (self.length[fixed] >= c[fixed]).all()
        fill = np.where(fixed, self.length - c, fill)
        fill = np.where(self.victim, 0, fill)
        fd = np.flatnonzero(fill)
        D, T, F = np.concatenate([D, fd]), np.concatenate([T, np.full(fd.size, self.filler, np.int64)]), np.concatenate([F, fill[fd]])
        # run-start parities, in term order: one more posting of a lower, never-queried term moves every later run by one
        cnt = np.bincount(T * self.nb + (D >> 15), minlength=self.vocab * self.nb)
        start = np.concatenate([[0], np.cumsum(cnt)])
        added, last = 0, -1
        for term, blk, odd, spare in sorted(self.parity):
            assert last < spare < term
            last = term
            if (int(start[term * self.nb + blk]) + added) % 2 != odd:
                d = int(self.take(1)[0])          # block 0: a doc of filler tokens so far
                assert fill[d] > 0 and not fixed[d]
                D, T, F = np.append(D, d), np.append(T, spare), np.append(F, 1)
                added += 1
        order = np.argsort(D, kind="stable")
        D, T, F = D[order], T[order], F[order]
        terms = np.repeat(T, F).astype(np.uint32)
        offs = np.zeros(self.n + 1, np.uint64)
        offs[1:] = np.cumsum(np.bincount(D, weights=F, minlength=self.n).astype(np.int64))
        assert int(offs[-1]) == terms.size and (np.diff(offs.astype(np.int64)) >= 1).all()
        return terms, offs


# ==================================================================== the case table
class Q(NamedTuple):
    name: str
    terms: tuple
    edges: tuple          # the checklist items this row is in the table for
    filt: tuple = None    # the query's doc filter (filtered batches)


class Batch(NamedTuple):
    name: str
    rows: tuple           # Q rows, searched together (one query each, in this order)
    depths: tuple
    filtered: bool = False
    edges: tuple = ()     # checklist items of the batch as a whole (passes, ranges, the ring across tasks)


class Group(NamedTuple):
    name: str
    n: int
    vocab: int
    base: int
    terms: np.ndarray
    offs: np.ndarray
    batches: tuple
    group: np.ndarray = None   # doc attributes (filtered batches)
    stamp: np.ndarray = None
    max_terms: int = 16

    def doc_base(self):
        return 2 ** 32 - 1 - self.n if self.base == MAXB else self.base


RUN_LENS = (1, 2, 127, 128, 129, 255, 256, 257)
PARTIALS = (1, 16383, 16384, 16385, 32767)
TABLE_C, SLOW_C = (1, 2, 3, 4, 5, 63, 64), (65, 66, 256)
LONG_T = (63, 64, 65, 66)
LANES = (15, 16, 17, 31, 32, 33, 47, 48, 49)
MULTI_M = (0, 1, 255, 256, 257, 512, 513)
TIE_DEPTHS = (1, 16, 17, 64, 256, 1000, 1024)
FILT_K = (4032, 4033, 4095, 4096, 4097, 4160, 8192)
FILT_DEPTHS = (1, 1024)
PASS_B = (127, 128, 129, 130)
DF_EDGES = (15, 16, 17, 1023, 1024, 1025)
SPECIAL_DIBS = (15 * 32, 15 * 32 + 31, 16 * 32, 16 * 32 + 31, 32736, 32767)

CHECKLIST = (
    ["run:%d:even" % x for x in RUN_LENS] + ["run:%d:odd" % x for x in RUN_LENS if x > 1] +
    ["run:last-of-array", "run:empty-middle"] + ["partial:%d" % r for r in PARTIALS] +
    ["C:%d:table" % c for c in TABLE_C] + ["C:%d:slow" % c for c in SLOW_C] +
    ["T:%d" % t for t in LONG_T] + ["T:oov", "T:repeat", "T:df0"] + ["lane:%d" % x for x in LANES] +
    ["wait:full", "wait:half", "wait:drain", "ring:C1", "ring:C2", "ring:C3", "ring:table-slow-table", "ring:table-empty-table",
     "ring:C64-every-block", "ring:ahead-across-task"] +
    ["multi:%d:table" % m for m in MULTI_M] + ["multi:%d:slow" % m for m in MULTI_M] +
    ["multi:%d:3terms" % m for m in MULTI_M] +
    ["multi:repeat2", "multi:repeat3", "multi:bit0", "multi:bit31", "multi:word15", "multi:word16", "multi:pref-even",
     "multi:pref-odd", "multi:last-word", "multi:5runs", "multi:rank-crosses-lane-slice"] +
    ["ties:depth%d" % d for d in TIE_DEPTHS] + ["ties:two-values", "ties:doc-id-bytes"] +
    ["filt:K%d:depth%d" % (k, d) for k in FILT_K for d in FILT_DEPTHS] +
    ["filt:full-no-prune", "filt:prune-at-flush-exact", "filt:prune-at-end", "filt:none-then-all", "filt:all-pass", "filt:cap-is-4096"] +
    ["pass:B%d:%s" % (b, k) for b in PASS_B for k in ("plain", "filtered")] +
    ["pass:q_begin128", "pass:filters-differ-127-128-129", "range:empty", "range:tasks-of-two-queries", "range:several-tasks",
     "range:B1-one-task-two-waves", "range:tasks-exceed-waves", "query:no-terms", "query:all-oov"] +
    ["floor:rank%d:%+d" % (r, o) for r in FLOOR_RANKS for o in (-1, 0, 1) if r + o <= OI_MAX_DEPTH] +
    ["df:%d" % d for d in DF_EDGES] + ["base:max"])

ALLF = (0, 0, 0, 0xFFFFFFFF)
_GROUPS = {}


def _runs_group(r):
    """Single-term runs of every chunk length from an even and an odd start, the last run of the array, an empty run between two
    others, a partial last block of r docs."""
    n = 3 * BS_BLOCK + r
    tests = [(L, odd) for L in RUN_LENS for odd in (0, 1) if L - odd >= 1]
    vocab = 10 + 4 * len(tests) + 4
    c = Corpus(n, vocab, seed=100 + r)
    c.reserve([0])
    rows = []
    for i, (L, odd) in enumerate(tests):
        par, before, t, after = 10 + 4 * i, 11 + 4 * i, 12 + 4 * i, 13 + 4 * i
        for nbr in (before, after):
            d = c.take(3)
            for blk in range(c.nb):
                c.put(nbr, blk, d, "all")
        c.put(t, 1, c.take(L - odd), "ends")
        c.want_parity(t, 1, odd, par)
        rows.append(Q("run-%d-%s" % (L, "odd" if odd else "even"), (t,), ("run:%d:%s" % (L, "odd" if odd else "even"),)))
    em, d = 5, c.take(40)
    for nbr in (4, 6):
        dn = c.take(3)
        for blk in range(c.nb):
            c.put(nbr, blk, dn, "all")
    c.put(em, 0, d, "ends"); c.put(em, 2, d, "ends")
    rows.append(Q("empty-middle", (em,), ("run:empty-middle",)))
    hi, dn = vocab - 1, c.take(3)
    for blk in range(c.nb):
        c.put(hi - 1, blk, dn, "all")
    c.put(hi, c.nb - 1, [0], "all")
    rows.append(Q("last-of-array", (hi,), ("run:last-of-array",)))
    terms, offs = c.finish()
    base = MAXB if r == 1 else 1000 + r
    return Group("runs-%d" % r, n, vocab, base, terms, offs,
                 (Batch("runs", tuple(rows), (1024, 3), edges=("partial:%d" % r,) + (("base:max",) if base == MAXB else ())),))


def _table_group():
    """Chunk tables of 1..64 chunks, windows past the table (65, 66, 256 chunks; 65 and 66 terms), run starts on both sides of
    every DPP row, and the ring across windows: table / slow / table, table / empty / table, 64 chunks in every block."""
    n, vocab = 3 * BS_BLOCK, 120
    c = Corpus(n, vocab, seed=7)
    S = list(range(10, 80))                      # one chunk per block each
    for t in S:
        d = c.take(3)
        for blk in range(3):
            c.put(t, blk, d, "ends" if blk != 1 else None)      # (block 1: every doc holds DN too)
    M2 = [82, 84, 86]                            # two chunks, block 0 only (so that their queries match <= 1024 docs)
    for t in M2:
        c.put(t, 0, c.take(131), "ends")
    DF0, OOV = 88, vocab + 7
    RG, E, DN = 92, 94, 98
    d = c.take(50)
    c.put(RG, 0, d); c.put(RG, 2, d); c.put(RG, 1, c.take(8400))       # > 64 chunks in block 1 only
    d = c.take(40)
    c.put(E, 0, d, "ends"); c.put(E, 2, d, "ends")
    c.put(DN, 1, np.arange(BS_BLOCK))            # every doc of block 1: 256 chunks from an even start
    c.want_parity(DN, 1, 0, 96)
    terms, offs = c.finish()
    rows = [Q("C-%d" % k, tuple(S[:k]), ("C:%d:table" % k,) + (("ring:C%d" % k,) if k <= 3 else ())) for k in (1, 2, 3, 4, 5, 63)]
    rows += [Q("C-65", tuple(S[:63] + M2[:1]), ("C:65:slow",)), Q("C-66", tuple(S[:62] + M2[:2]), ("C:66:slow",)),
             Q("C-256", (DN,), ("C:256:slow",))]
    for T in LONG_T:
        rows.append(Q("T-%d" % T, tuple([S[0], OOV, DF0, S[0]] + S[1:T - 3]), ("T:%d" % T, "T:oov", "T:repeat", "T:df0")))
    qa = S[:15] + [M2[0]] + S[15:29] + [M2[1]] + S[29:43] + [M2[2]] + S[43:44]
    qb = S[:16] + [M2[0]] + S[16:30] + [M2[1]] + S[30:44] + [M2[2]] + S[44:45]
    rows += [Q("lanes-a", tuple(qa), tuple("lane:%d" % x for x in (15, 17, 31, 33, 47, 49))),
             Q("lanes-b", tuple(qb), tuple("lane:%d" % x for x in (16, 32, 48)))]
    heavy = [Q("heavy-%d" % i, (DN, S[i]), ()) for i in range(6)]
    ring = [Q("table-slow-table", (RG, S[0]), ("ring:table-slow-table",)), Q("table-empty-table", (E,), ("ring:table-empty-table",)),
            Q("C-64", tuple(S[:64]), ("C:64:table", "ring:C64-every-block", "ring:ahead-across-task"))] + heavy
    return Group("table", n, vocab, 77, terms, offs,
                 (Batch("tables", tuple(rows), (1024, 10), edges=("wait:full", "wait:half", "wait:drain")),
                  Batch("ring", tuple(ring), (1024, 10))), max_terms=128)


def _multi_group():
    """Docs of several runs: 0..513 of them in a window on the table path and on the direct path, repeated terms, the corners of
    the map words, the halves of a pref word, a lane's slice of the sweep, the last word of the block, one doc in five runs."""
    n, vocab = BS_BLOCK + 5000, 80
    c = Corpus(n, vocab, seed=11)
    c.reserve(SPECIAL_DIBS)
    U, X, Y, DN = 10, 40, 42, 60
    u = c.take(700, stride=5)                    # spread over 110 map words = 7 lanes of the sweep
    c.put(U, 0, u)
    P = {}
    for i, M in enumerate(MULTI_M):
        P[M] = 12 + 2 * i
        if M:
            c.put(P[M], 0, u[:M])
        c.put(P[M], 0, c.take(20), "all")
    c.put(X, 0, u[:1]); c.put(X, 0, c.take(10), "all")
    c.put(Y, 0, c.take(10), "all")
    c.put(DN, 0, c.take(8400))                   # > 64 chunks, shares no doc
    G1, G2 = 44, 46
    for t in (G1, G2):
        c.put(t, 0, SPECIAL_DIBS); c.put(t, 0, c.take(10), "all")
    F5 = [48, 50, 52, 54, 56]
    x = c.take(1)
    for t in F5:
        c.put(t, 0, x); c.put(t, 0, c.take(8), "all")
    terms, offs = c.finish()
    rows = []
    for M in MULTI_M:
        rows.append(Q("M-%d-table" % M, (U, P[M]), ("multi:%d:table" % M,) + (("multi:rank-crosses-lane-slice",) if M == 513 else ())))
        rows.append(Q("M-%d-3terms" % M, (P[M], U, X if M else Y), ("multi:%d:3terms" % M,)))
        rows.append(Q("M-%d-slow" % M, (U, P[M], DN), ("multi:%d:slow" % M,)))
    rows += [Q("repeat-2", (U, U), ("multi:repeat2",)), Q("repeat-3", (U, P[1], U), ("multi:repeat3",)),
             Q("corners", (G1, G2), ("multi:bit0", "multi:bit31", "multi:word15", "multi:word16", "multi:pref-even", "multi:pref-odd",
                                     "multi:last-word")),
             Q("five-runs", tuple(F5), ("multi:5runs",))]
    return Group("multi", n, vocab, 123456, terms, offs, (Batch("multi", tuple(rows), (1024, 100)),))


def _ties_group():
    """Unfiltered segments (floors on, cap = depth + 256) pruned again and again: a term in every doc of a block with every
    impact equal, and one with two impact values whose higher one is held by exactly 256 docs."""
    n, vocab = 2 * BS_BLOCK, 8
    c = Corpus(n, vocab, seed=13)
    V, TT = 3, 5
    c.put(V, 0, np.arange(BS_BLOCK), tf=1)
    c.put(TT, 1, np.arange(BS_BLOCK), tf=1)
    c.length[:BS_BLOCK] = np.where(np.arange(BS_BLOCK) % 128 == 77, 1, 2)
    c.length[BS_BLOCK:] = 1
    terms, offs = c.finish()
    rows = (Q("all-tie", (TT,), tuple("ties:depth%d" % d for d in TIE_DEPTHS) + ("ties:doc-id-bytes",)),
            Q("two-values", (V,), ("ties:two-values",)))
    return Group("ties", n, vocab, 5, terms, offs, (Batch("ties", rows, tuple(sorted(set(TIE_DEPTHS) | {255, 257}))),))


FILT_STAMP1 = 100_000


def _filt_group():
    """Filtered segments (no floors, cap = 4096, one phase): a term in every doc; the stamp window of a filter passes exactly K
    docs of block 0 (real impacts) or of block 1 (every impact equal: the prunes of the mirror are exact)."""
    n, vocab = 2 * BS_BLOCK, 8
    c = Corpus(n, vocab, seed=17)
    A = 3
    c.put(A, 0, np.arange(BS_BLOCK))
    c.put(A, 1, np.arange(BS_BLOCK), tf=1)
    c.length[BS_BLOCK:] = 2
    terms, offs = c.finish()
    rng = np.random.default_rng(18)
    stamp = np.concatenate([rng.permutation(BS_BLOCK), FILT_STAMP1 + rng.permutation(BS_BLOCK)]).astype(np.uint32)
    group = (np.arange(n) >> 15).astype(np.uint32)
    batches = []
    for depth in FILT_DEPTHS:
        rows = []
        for K in FILT_K:
            rows.append(Q("real-K%d" % K, (A,), (), (0, 0, 0, K - 1)))
            extra = {4096: ("filt:full-no-prune",), 4097: ("filt:prune-at-end",), 4160: ("filt:prune-at-flush-exact",)}.get(K, ())
            rows.append(Q("ties-K%d" % K, (A,), ("filt:K%d:depth%d" % (K, depth),) + extra, (0, 0, FILT_STAMP1, FILT_STAMP1 + K - 1)))
        rows.append(Q("none-then-all", (A,), ("filt:none-then-all",), (0xFFFFFFFF, 1, 0, 0xFFFFFFFF)))
        rows.append(Q("all-pass", (A,), ("filt:all-pass",), ALLF))
        batches.append(Batch("filt-depth%d" % depth, tuple(rows), (depth,), True, ("filt:cap-is-4096",)))
    return Group("filt", n, vocab, 9, terms, offs, tuple(batches), group, stamp)


def _pass_queries(vocab, df):
    order = np.argsort(-df, kind="stable")
    heavy, rare = [int(t) for t in order[:8]], [int(t) for t in order if df[t] > 0][-30:]
    out = []
    for b in range(max(PASS_B)):
        kind = 3 if b >= 127 else b % 4          # (127, 128, 129: heavy, so that the second pass's lists show a wrong offset)
        out.append(() if kind == 0 else (vocab + 3, vocab + 9) if kind == 1 else (rare[b % len(rare)],) if kind == 2 else
                   tuple(heavy[(b + i) % 8] for i in range(8)))
    return out


def _pass_group():
    """Two passes (B = 129, 130) beside one (127, 128) on two blocks, with and without filters; zero-term, out-of-vocabulary, rare
    and heavy queries side by side, so that the equal-weight ranges are empty here and hold several tasks there."""
    from test_gpu_parity import _small_forward
    n, vocab = 2 * BS_BLOCK, 300
    rng = np.random.default_rng(19)
    terms, offs = _small_forward(rng, n, vocab, max_len=10, zipf=True)
    df = np.array([Layout(terms, offs, vocab).df(t) for t in range(vocab)])
    qs = _pass_queries(vocab, df)
    group = rng.integers(0, 4, size=n).astype(np.uint32)
    stamp = np.arange(n, dtype=np.uint32)
    batches = []
    for B in PASS_B:
        for filtered in (False, True):
            rows = []
            for b in range(B):
                f = None
                if filtered:
                    f = {127: (1, 0, 0, 0xFFFFFFFF), 128: (1, 1, 0, 0xFFFFFFFF), 129: (3, 2, 0, 0xFFFFFFFF)}.get(
                        b, (3, b % 4, 0, 0xFFFFFFFF) if b % 3 else (0, 0, 1000, n - 1000))
                e = ("query:no-terms",) if b == 0 else ("query:all-oov",) if b == 1 else ()
                rows.append(Q("q%d" % b, qs[b], e, f))
            e = ["pass:B%d:%s" % (B, "filtered" if filtered else "plain")]
            if B > 128:
                e.append("pass:q_begin128")
            if B == 130 and filtered:
                e.append("pass:filters-differ-127-128-129")
            if B == 128 and not filtered:
                e += ["range:empty", "range:tasks-of-two-queries", "range:several-tasks"]
            batches.append(Batch("B%d-%s" % (B, "filtered" if filtered else "plain"), tuple(rows), (50,), filtered, tuple(e)))
    return Group("pass", n, vocab, 31, terms, offs, tuple(batches), group, stamp)


def _b1_group():
    """B = 1 on a single block: one task, one workgroup of two waves, one of them with an empty range."""
    from test_gpu_parity import _small_forward
    n, vocab = 5000, 40
    terms, offs = _small_forward(np.random.default_rng(23), n, vocab, max_len=10, zipf=True)
    return Group("b1", n, vocab, 3, terms, offs,
                 (Batch("B1", (Q("one", (0, 5, 7), ()),), (1024, 10), edges=("range:B1-one-task-two-waves",)),))


FLOOR_GROUP_DOCS = 200


def _floors_group():
    """The first threshold (bm25.hip: the per-term impact floors): a term whose 16th / 64th, 256th and 1024th largest impacts each
    tie with 199 others (docs of one length per 200), and terms with df on both sides of every floor rank."""
    n, vocab = BS_BLOCK + 7232, 40
    c = Corpus(n, vocab, seed=29)
    FL = 10
    for g in range(7):                           # impact ranks 200 g + 1 .. 200 (g + 1): docs of g + 1 tokens
        blk = g % 2
        d = c.take(FLOOR_GROUP_DOCS)
        d = d[d < n - blk * BS_BLOCK]
        assert d.size == FLOOR_GROUP_DOCS
        docs = c.put(FL, blk, d, tf=1)
        c.length[docs] = g + 1
    rows = [Q("tied-ranks", (FL,), tuple("floor:rank%d:%+d" % (r, o) for r in FLOOR_RANKS for o in (-1, 0, 1) if r + o <= OI_MAX_DEPTH))]
    for i, df in enumerate(DF_EDGES):
        t = 12 + 2 * i
        d = c.take(df)
        c.put(t, 0, d[: df // 2], "ends"); c.put(t, 1, d[df // 2:][d[df // 2:] < 7232], "ends")
        rows.append(Q("df-%d" % df, (t,), ("df:%d" % df,)))
    terms, offs = c.finish()
    depths = sorted({r + o for r in FLOOR_RANKS for o in (-1, 0, 1) if r + o <= OI_MAX_DEPTH} | {1, 1000})
    return Group("floors", n, vocab, 2000, terms, offs, (Batch("floors", tuple(rows), tuple(depths)),))


GROUP_MAKERS = dict([("runs-%d" % r, (lambda r=r: _runs_group(r))) for r in PARTIALS] +
                    [("table", _table_group), ("multi", _multi_group), ("ties", _ties_group), ("filt", _filt_group),
                     ("pass", _pass_group), ("b1", _b1_group), ("floors", _floors_group)])
GROUP_NAMES = tuple(GROUP_MAKERS)
LARGE_EDGES = ("range:tasks-exceed-waves",)       # the larger range case is a test of its own (sized from the CU count)


def get_group(name) -> Group:
    if name not in _GROUPS:
        _GROUPS[name] = GROUP_MAKERS[name]()
    return _GROUPS[name]


def large_blocks(num_cus: int, B: int = BS_MAX_Q) -> int:
    """The fewest blocks at which the tasks of B queries exceed the waves of a full launch: 17 at 256 CUs."""
    return BS_WPB * PER_CU * num_cus // B + 1


# ==================================================================== what the mirror says a row reaches
def _passes(f, group, stamp):
    m, v, lo, hi = (int(x) for x in f)
    return ((group & np.uint32(m)) == np.uint32(v)) & (stamp >= np.uint32(lo)) & (stamp <= np.uint32(hi))


def _waves(g: Group, L: Layout, b: Batch, num_cus: int):
    """Per pass: the task list of every wave's range (queries numbered inside the pass)."""
    p = plan(L.nb, len(b.rows), max(b.depths), b.filtered)
    assert p.phases == 1 and p.first == L.nb
    out = []
    for q0 in p.q_begins:
        qs = [r.terms for r in b.rows[q0:q0 + p.pass_q]]
        n_tasks, wgs, G = launch_geometry(L.nb, len(qs), num_cus)
        out.append((q0, n_tasks, wgs, G, ranges(units(L, qs), L.nb, G)))
    return p, out


def reached_row(g: Group, L: Layout, b: Batch, row: Q) -> set:
    out = set()
    wins = [window(L, row.terms, blk) for blk in range(L.nb)]
    T = len(row.terms)
    inv = [t for t in row.terms if t < L.vocab]
    if T == 0:
        out.add("query:no-terms")
    elif not inv:
        out.add("query:all-oov")
    if T in LONG_T:
        out.add("T:%d" % T)
        first = row.terms[:64]
        if any(t >= L.vocab for t in first):
            out.add("T:oov")
        if len(set(first)) < len(first):
            out.add("T:repeat")
        if any(t < L.vocab and L.df(t) == 0 for t in first):
            out.add("T:df0")
    for blk, w in enumerate(wins):
        for r in w.runs:
            if r.e > r.s:
                assert r.e - (r.s & ~1) >= 1 + (r.s & 1)          # an odd start: never a single slot
                if T == 1:
                    out.add("run:%d:%s" % (r.e - (r.s & ~1), "odd" if r.s & 1 else "even"))
                    if r.e == L.n_postings and r.e - r.s == 1 and blk == L.nb - 1 and r.term == L.vocab - 1:
                        out.add("run:last-of-array")
                if not w.slow and T <= 64:
                    out.add("lane:%d" % r.lane)
        if w.C:
            out.add("C:%d:%s" % (w.C, "slow" if w.slow else "table"))
            if not w.slow and w.C <= 3:
                out.add("ring:C%d" % w.C)
        if len(inv) == 2 and len(set(inv)) == 2 and not w.slow:
            out.add("multi:%d:table" % w.M)
        if len(inv) == 3 and len(set(inv)) == 3:
            out.add("multi:%d:%s" % (w.M, "slow" if w.slow else "3terms"))
        if w.M and not w.slow:
            if len(inv) == 2 and inv[0] == inv[1] and w.M == len(L.docs(inv[0], blk)):
                out.add("multi:repeat2")
            if len(inv) == 3 and inv[0] == inv[2] != inv[1] and w.M == len(L.docs(inv[0], blk)):
                out.add("multi:repeat3")
            word, bit = w.multi >> 5, w.multi & 31
            for name, hit in (("bit0", bit == 0), ("bit31", bit == 31), ("word15", word % 16 == 15), ("word16", (word % 16 == 0) & (word > 0)),
                              ("pref-even", word % 2 == 0), ("pref-odd", word % 2 == 1), ("last-word", word == BS_BLOCK // 32 - 1)):
                if hit.any():
                    out.add("multi:" + name)
            if np.unique(word // 16).size >= 3 and w.M > 2 * BS_CAP:
                out.add("multi:rank-crosses-lane-slice")
            if len(set(inv)) == 5:
                cat = np.concatenate([L.docs(t, blk) for t in inv])
                if (np.unique(cat, return_counts=True)[1] == 5).any():
                    out.add("multi:5runs")
    if len(wins) == 3:
        sig = tuple("slow" if w.slow else "table" if w.C else "empty" for w in wins)
        if sig == ("table", "slow", "table"):
            out.add("ring:table-slow-table")
        if sig == ("table", "empty", "table"):
            out.add("ring:table-empty-table")
        if all(w.C == 64 and not w.slow for w in wins):
            out.add("ring:C64-every-block")
    if len(wins) >= 3 and T == 1 and wins[0].C and not wins[1].C and wins[2].C:
        out.add("run:empty-middle")
    # ---- segments
    if T == 1 and inv and not b.filtered:
        t = inv[0]
        for blk in range(L.nb):
            docs = L.docs(t, blk)
            if docs.size == BS_BLOCK:             # a term in every doc of the block
                lens = np.diff(g.offs.astype(np.int64))[docs]
                vals, cnts = np.unique(lens, return_counts=True)
                for depth in b.depths:
                    pr = prune_trace(BS_BLOCK, seg_cap(depth, False), depth)
                    if vals.size == 1 and len(pr) > 8:      # every impact ties: each prune ends in the doc-id bytes
                        out.add("ties:depth%d" % depth)
                        out.add("ties:doc-id-bytes")
                    if vals.size == 2 and cnts[0] == depth and len(pr) > 8:   # vals[0]: the shorter docs, the higher impact
                        out.add("ties:two-values")
        if L.df(t) in DF_EDGES:
            out.add("df:%d" % L.df(t))
        # floors: the docs of the term in groups of one length; rank r and its neighbours searched
        lens = np.sort(np.diff(g.offs.astype(np.int64))[np.concatenate([L.docs(t, blk) for blk in range(L.nb)])])
        for r in FLOOR_RANKS:
            if lens.size >= r + 100 and (lens == lens[r - 1]).sum() >= 200 and len(set(inv)) == 1:
                first = int(np.searchsorted(lens, lens[r - 1]))       # ranks first + 1 .. first + ties hold that impact
                if first + 1 < r < first + (lens == lens[r - 1]).sum():
                    for o in (-1, 0, 1):
                        if r + o in b.depths:
                            out.add("floor:rank%d:%+d" % (r, o))
    if b.filtered and T == 1 and inv:
        ok = _passes(row.filt, g.group, g.stamp)
        per_blk = [int(ok[L.docs(inv[0], blk)].sum()) for blk in range(L.nb)]
        if row.filt == ALLF:
            out.add("filt:all-pass")
        if L.nb == 2 and per_blk[0] == 0 and per_blk[1] == BS_BLOCK == len(L.docs(inv[0], 1)):
            out.add("filt:none-then-all")
        for depth in b.depths:
            cap = plan(L.nb, len(b.rows), depth, True).cap1
            for blk, K in enumerate(per_blk):
                lens = np.diff(g.offs.astype(np.int64))[L.docs(inv[0], blk)]
                if K in FILT_K and (lens == lens[0]).all():
                    out.add("filt:K%d:depth%d" % (K, depth))
                    pr = prune_trace(K, cap, depth)
                    if K == cap and not pr:
                        out.add("filt:full-no-prune")
                    if pr == [("flush", cap)]:
                        out.add("filt:prune-at-flush-exact")
                    if pr == [("end", cap)]:
                        out.add("filt:prune-at-end")
    return out


def reached_batch(g: Group, L: Layout, b: Batch, num_cus: int = MI355X_CUS) -> set:
    out = set()
    B = len(b.rows)
    p, passes = _waves(g, L, b, num_cus)
    kind = "filtered" if b.filtered else "plain"
    if g.name == "pass":
        out.add("pass:B%d:%s" % (B, kind))
    if 128 in p.q_begins:
        out.add("pass:q_begin128")
        if b.filtered and B >= 130 and len({b.rows[i].filt for i in (127, 128, 129)}) == 3:
            out.add("pass:filters-differ-127-128-129")
    if b.filtered:
        assert all(seg_cap(d, True) == 4096 for d in range(1, OI_MAX_DEPTH + 1))   # depth + 256 > 4096: past OI_MAX_DEPTH
        if all(plan(L.nb, B, d, True).cap1 == 4096 for d in b.depths):
            out.add("filt:cap-is-4096")
    if g.n % BS_BLOCK in PARTIALS:
        out.add("partial:%d" % (g.n % BS_BLOCK))
    if g.base == MAXB:
        out.add("base:max")
    for q0, n_tasks, wgs, G, rng in passes:
        if B == 1 and L.nb == 1 and (n_tasks, wgs, G) == (1, 1, 2) and sorted(len(t) for t in rng) == [0, 1]:
            out.add("range:B1-one-task-two-waves")
        if n_tasks > G:
            out.add("range:tasks-exceed-waves")
        for tasks in rng:
            if not tasks and n_tasks >= G:
                out.add("range:empty")
            if len(tasks) >= 3:
                out.add("range:several-tasks")
            if len(tasks) >= 3 and len({r for r, _ in tasks}) >= 2:
                out.add("range:tasks-of-two-queries")
            # the ring over the windows the wave walks for each query of its range
            for r in sorted({r for r, _ in tasks}):
                blks = [blk for rr, blk in tasks if rr == r]
                wins = [window(L, b.rows[q0 + r].terms, blk) for blk in blks]
                br, ahead = ring_trace([(w.C, w.slow) for w in wins])
                out |= {"wait:" + x for x in br}
                sig = tuple("slow" if w.slow else "table" if w.C else "empty" for w in wins)
                if any(ahead):
                    out.add("ring:ahead-across-task")
                for i in range(len(sig) - 2):
                    if sig[i:i + 3] == ("table", "slow", "table"):
                        out.add("walk:table-slow-table:%d" % (q0 + r))
                    if sig[i:i + 3] == ("table", "empty", "table"):
                        out.add("walk:table-empty-table:%d" % (q0 + r))
                for i in range(len(sig) - 1):
                    if wins[i].C == 64 and wins[i + 1].C == 64 and not wins[i].slow and ahead[i] == BS_RING:
                        out.add("walk:C64-ring-full:%d" % (q0 + r))
    return out


# ==================================================================== CPU tests
def _defines(path):
    out = {}
    for m in re.finditer(r"^\s*#\s*define\s+(\w+)\s+(\S+)", open(path).read(), re.M):
        out.setdefault(m.group(1), m.group(2))
    return out


def test_mirror_constants_equal_the_sources():
    """A retune of the kernel breaks the table loudly: every mirrored constant is read from the #define lines."""
    d = _defines(os.path.join(CSRC, "bm25_stream.hip"))
    num = lambda s: int(s.rstrip("uU"))
    assert d["BS_BLOCK"] == "OI_BM25_BLOCK_DOCS" and d["BS_FINE"] == "OI_BM25_FINE_DOCS"
    for name, want in (("BS_WPB", BS_WPB), ("BS_RING", BS_RING), ("BS_CAP", BS_CAP), ("BS_STAGE", BS_STAGE), ("BS_MAX_Q", BS_MAX_Q),
                       ("BS_RUN_COST", BS_RUN_COST), ("BS_TASK_COST", BS_TASK_COST)):
        assert num(d[name]) == want, name
    internal = _defines(os.path.join(CSRC, "oi_internal.h"))
    assert num(internal["OI_BM25_FLOOR_RANKS"]) == OI_BM25_FLOOR_RANKS == len(FLOOR_RANKS)
    public = _defines(os.path.join(ROOT, "include", "openintel_hip.h"))      # (oi_internal.h takes the block sizes from here)
    assert num(public["OI_BM25_BLOCK_DOCS"]) == BS_BLOCK and num(public["OI_BM25_FINE_DOCS"]) == BS_FINE
    assert num(public["OI_MAX_DEPTH"]) == OI_MAX_DEPTH
    src = open(os.path.join(CSRC, "bm25_stream.hip")).read()
    assert "(160u * 1024u) / lds_total" in src and "const uint32_t c = depth + 256u;" in src and "std::max(c, 4096u)" in src
    assert "{16u, 64u, 256u, 1024u}" in open(os.path.join(CSRC, "bm25.hip")).read()
    assert lds_total() == 40464 and PER_CU == 4 and large_blocks(MI355X_CUS) == 17


@pytest.mark.parametrize("name", GROUP_NAMES)
def test_every_row_reaches_the_edges_it_declares(name):
    g = get_group(name)
    L = Layout(g.terms, g.offs, g.vocab)
    lens = np.diff(g.offs.astype(np.int64))
    assert lens.min() >= 1 and (name in ("ties",) or lens.max() >= 8), "documents of 1 to about 12 tokens"
    for b in g.batches:
        whole = reached_batch(g, L, b)
        assert set(b.edges) <= whole, (b.name, sorted(set(b.edges) - whole))
        for i, row in enumerate(b.rows):
            got = reached_row(g, L, b, row)
            assert set(row.edges) <= got | whole, (b.name, row.name, sorted(set(row.edges) - got - whole))
            # a wave walks the three windows of the ring rows one after the other (the ranges of this batch, at 256 CUs)
            for e in row.edges:
                if e in ("ring:table-slow-table", "ring:table-empty-table"):
                    assert "walk:%s:%d" % (e[5:], i) in whole, (row.name, e)
                if e == "ring:ahead-across-task":
                    assert "walk:C64-ring-full:%d" % i in whole, row.name
            # complete lists: a row there for a run, a table or the multi docs of a table window is searched at a depth that
            # returns every matching doc
            if any(e.startswith("run:") or e.startswith("lane:") or e.startswith("T:") or e.endswith(":table") or e.endswith(":3terms")
                   for e in row.edges):
                matches = sum(np.unique(np.concatenate([L.docs(t, blk) for t in row.terms if t < L.vocab])).size for blk in range(L.nb))
                assert matches <= OI_MAX_DEPTH == max(b.depths), (row.name, matches)


def test_the_table_covers_the_whole_checklist():
    declared = set(LARGE_EDGES)
    for name in GROUP_NAMES:
        for b in get_group(name).batches:
            declared |= set(b.edges)
            for row in b.rows:
                declared |= set(row.edges)
    assert len(set(CHECKLIST)) == len(CHECKLIST)
    assert set(CHECKLIST) <= declared, sorted(set(CHECKLIST) - declared)
    assert declared <= set(CHECKLIST), sorted(declared - set(CHECKLIST))
    # the larger case at 256 CUs: more tasks than waves, so a wave walks several whole tasks
    nbk = large_blocks(MI355X_CUS)
    n_tasks, wgs, G = launch_geometry(nbk, BS_MAX_Q, MI355X_CUS)
    assert n_tasks > G == BS_WPB * PER_CU * MI355X_CUS and plan(nbk, BS_MAX_Q, 10, False).pass_q == BS_MAX_Q
    rng = ranges([BS_TASK_COST + (BS_RUN_COST + 163) * (1 + b % 3) for b in range(BS_MAX_Q)], nbk, G)   # queries of 1..3 terms
    assert sum(len(t) for t in rng) == n_tasks and max(len(t) for t in rng) >= 2
    assert any(len({r for r, _ in t}) == 2 for t in rng), "a wave ends one query and starts the next"


def test_victims_are_the_shortest_docs_of_their_runs():
    """runs-*: the first and last doc of every run under test, and every doc of its neighbour terms, hold one token."""
    g = get_group("runs-16384")
    L = Layout(g.terms, g.offs, g.vocab)
    lens = np.diff(g.offs.astype(np.int64))
    for row in g.batches[0].rows:
        t = row.terms[0]
        for blk in range(L.nb):
            d = L.docs(t, blk)
            if d.size:
                assert lens[d[0]] == 1 and lens[d[-1]] == 1, row.name
            for nbr in (t - 1, t + 1):
                if nbr < L.vocab and row.name.startswith("run-"):
                    dn = L.docs(nbr, blk)
                    assert dn.size and (lens[dn] == 1).all(), (row.name, nbr, blk)
                    assert not np.isin(dn & (BS_BLOCK - 1), L.docs(t, 1) & (BS_BLOCK - 1)).any()


def test_mirror_layout_against_a_brute_force_sort():
    rng = np.random.default_rng(5)
    for n, vocab in ((70, 5), (40000, 7), (66000, 3)):
        lens = rng.integers(1, 5, size=n)
        offs = np.zeros(n + 1, np.uint64)
        offs[1:] = np.cumsum(lens)
        terms = rng.integers(0, vocab, size=int(offs[-1])).astype(np.uint32)
        L = Layout(terms, offs, vocab)
        doc = np.repeat(np.arange(n), lens)
        keys = sorted(set(zip(terms.tolist(), doc.tolist())))
        assert L.n_postings == len(keys)
        q = [int(x) for x in rng.integers(0, vocab + 1, size=3)] + [0]
        q[3] = q[0]                               # a repeated term counts as two runs
        for blk in range(L.nb):
            seen = {}
            for t in q:
                if t >= vocab:
                    continue
                idx = [i for i, (tt, d) in enumerate(keys) if tt == t and d // BS_BLOCK == blk]
                s = idx[0] if idx else sum(1 for tt, d in keys if (tt, d // BS_BLOCK) < (t, blk))
                assert L.run(t, blk) == (s, s + len(idx)), (n, t, blk)
                for i in idx:
                    seen[keys[i][1]] = seen.get(keys[i][1], 0) + 1
            w = window(L, q, blk)
            assert w.M == sum(1 for v in seen.values() if v >= 2), (n, blk)
            assert w.C == sum(r.n for r in w.runs) and [r.lane for r in w.runs] == list(np.cumsum([0] + [r.n for r in w.runs])[:-1])


def test_ring_and_prune_mirrors_on_known_shapes():
    assert ring_trace([(1, False)]) == ({"half", "drain"}, [0])
    assert ring_trace([(2, False)])[0] == {"full", "half", "drain"}
    assert ring_trace([(3, False), (0, True), (2, False)])[1] == [0, 0, 0]
    assert ring_trace([(64, False), (64, False)])[1] == [BS_RING, 0]
    assert prune_trace(4096, 4096, 1) == [] and prune_trace(4097, 4096, 1) == [("end", 4096)]
    assert prune_trace(4160, 4096, 1024) == [("flush", 4096)] and prune_trace(4095, 4096, 1) == []
    assert prune_trace(4096 - 63, 4096, 1) == [] and len(prune_trace(BS_BLOCK, seg_cap(1, False), 1)) == 127


# ==================================================================== GPU tests
@pytest.fixture(scope="module")
def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.fixture(scope="module")
def ctx():
    import openintel_amd as oi
    from openintel_amd import _lib
    c = oi.HipContext(0)
    c.set_cosine_mode(_lib.OI_COSINE_EXACT)
    yield c
    c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import lib
    return lib


def _make_index(ctx, g_n, vocab, base, terms, offs, group=None, stamp=None, max_terms=16, seed=1):
    import openintel_amd as oi
    rows = np.random.default_rng(seed).integers(-2, 3, size=(g_n, 8)).astype(np.float32)      # as _small_forward's users
    idx = oi.HybridIndex(ctx, g_n, 8, vocab, base)
    idx.set_embeddings(rows, normalize=False)
    idx.set_forward(terms, offs)
    if group is not None:
        idx.set_doc_attrs(group, stamp)
    idx.finalize()
    idx.set_max_query_terms(max_terms)
    return idx


def _compare(L, b, rs, rd, tag, bad):
    c = int(L.bm25_counts[b])
    if c != rd.size:
        bad.append(tag + ("count %d, oracle %d" % (c, rd.size),))
    elif not np.array_equal(L.bm25_docs[b][:c], rd):
        i = int(np.flatnonzero(L.bm25_docs[b][:c] != rd)[0])
        bad.append(tag + ("doc ids differ from rank %d: %d, oracle %d" % (i, L.bm25_docs[b][i], rd[i]),))
    elif not np.array_equal(L.bm25_scores[b][:c].view(np.uint32), rs.view(np.uint32)):
        bad.append(tag + ("score bits differ",))


def _run_batch(idx, O, g, b, full, bad, modes=(STREAM, WAVE, TAAT)):
    from openintel_amd import pack_query_terms
    base = g.doc_base()
    B = len(b.rows)
    qt, qo = pack_query_terms([list(r.terms) for r in b.rows])
    q = np.random.default_rng(B).integers(-2, 3, size=(B, 8)).astype(np.float32)
    F = np.array([r.filt for r in b.rows], np.uint32) if b.filtered else None
    for depth in b.depths:
        lists = {}
        for mode in ((STREAM,) if b.filtered else modes):
            idx.set_bm25_mode(mode)
            lists[mode] = idx.search_lists(q, qt, qo, depth=depth, filters=F)
        idx.set_bm25_mode(STREAM)
        S = lists[STREAM]
        for i, row in enumerate(b.rows):
            sc = full[row.terms]
            if b.filtered:
                sc = np.where(_passes(row.filt, g.group, g.stamp), sc, 0).astype(np.float32)
            rs, rd = O.topk(sc, depth, True, base)
            _compare(S, i, rs, rd, (g.name, b.name, row.name, depth), bad)
        for mode, Lm in lists.items():
            if mode != STREAM:
                for f in ("bm25_counts", "bm25_docs", "bm25_scores"):
                    if not np.array_equal(getattr(Lm, f).view(np.uint32), getattr(S, f).view(np.uint32)):
                        bad.append((g.name, b.name, "mode %d" % mode, depth, f + " differ from the stream kernel's"))
        if b.filtered and any(r.filt == ALLF for r in b.rows):       # the all-pass filter: the unfiltered list
            U = idx.search_lists(q, qt, qo, depth=depth)
            for i, row in enumerate(b.rows):
                if row.filt == ALLF and not all(np.array_equal(getattr(U, f)[i].view(np.uint32), getattr(S, f)[i].view(np.uint32))
                                                for f in ("bm25_counts", "bm25_docs", "bm25_scores")):
                    bad.append((g.name, b.name, row.name, depth, "the all-pass list differs from the unfiltered one"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", GROUP_NAMES)
def test_stream_group_bit_exact(ctx, O, name):
    """Every row of the group's batches: counts, doc ids and score bits equal the oracle's at every depth of the batch; the wave
    and the workgroup-per-block kernels return the same bytes."""
    g = get_group(name)
    idx = _make_index(ctx, g.n, g.vocab, g.doc_base(), g.terms, g.offs, g.group, g.stamp, g.max_terms)
    full, bad = {}, []
    for b in g.batches:
        for row in b.rows:
            if row.terms not in full:
                tv = np.array([t for t in row.terms if t < g.vocab], np.uint32)
                full[row.terms] = O.bm25_scores(g.terms, g.offs, g.vocab, tv)
    for b in g.batches:
        _run_batch(idx, O, g, b, full, bad)
    idx.close()
    assert not bad, "%d mismatches, the first: %r" % (len(bad), bad[:8])


@pytest.mark.gpu
def test_stream_more_tasks_than_waves(ctx, O, num_cus):
    """Enough blocks that the tasks of a 128-query pass exceed the waves of a full launch (17 blocks at 256 CUs): a wave walks
    several whole tasks of one query and then the next query's.  Docs of 1 to 3 tokens keep the oracle's share to seconds."""
    from openintel_amd import pack_query_terms
    B, depth, vocab, base = BS_MAX_Q, 10, 400, 4242
    nbk = large_blocks(num_cus, B)
    n = nbk * BS_BLOCK - 5
    n_tasks, wgs, G = launch_geometry(nbk, B, num_cus)
    assert n_tasks > G and plan(nbk, B, depth, False).pass_q == B
    rng = np.random.default_rng(37)
    lens = rng.integers(1, 4, size=n)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    terms = rng.integers(0, vocab, size=int(offs[-1])).astype(np.uint32)
    queries = [tuple(int(t) for t in rng.integers(0, vocab, size=1 + b % 3)) for b in range(B)]
    g = Group("large", n, vocab, base, terms, offs, (Batch("large", tuple(Q("q%d" % i, t, ()) for i, t in enumerate(queries)), (depth,)),))
    rng = ranges(units(Layout(terms, offs, vocab), queries), nbk, G)
    assert max(len(t) for t in rng) >= 2 and any(len({r for r, _ in t}) == 2 for t in rng), "a wave ends one query, starts the next"
    idx = _make_index(ctx, n, vocab, base, terms, offs)
    full = {t: O.bm25_scores(terms, offs, vocab, np.array(t, np.uint32)) for t in set(queries)}
    bad = []
    _run_batch(idx, O, g, g.batches[0], full, bad)
    idx.close()
    assert not bad, "%d mismatches, the first: %r" % (len(bad), bad[:8])
