"""The search tail (csrc/select.hip: select_flat_kernel, lists_to_pool_kernel, rrf_kernel, and oi_fuse_packed on top of them) at
every size class, sample and hash edge, bit for bit against a numpy statement of the contract.

Every ranked list this library returns leaves through these kernels.  The select is a tree of paths chosen by the pool size
alone (keys in registers at 4, 8, 16, 32 per thread, then the re-loading path), a sampled cut with three fallbacks whose
outcome depends on WHERE in the pool the good keys sit, and a radix select whose wave-0 digit walk has four positions per
lane; the fusion is a linear-probe LDS hash.  A wrong guard in any of these drops or doubles one document on some data
only, and the branch it sits in is not visible in the output: "the RESULT never depends on the sample".

This module holds a pure-Python MIRROR of the kernels' geometry (select_trace: size class, keys per thread, idle waves, the
sample set, r, the sampled threshold, c, the branch taken, every radix pass with its digit, lane and position; rrf_trace:
the probe table, its clusters and the walk of every lookup), a declared table of cases (MERGE_ROWS, RRF_ROWS, PACKED_ROWS:
each row names the edges it is there for) and a CHECKLIST of every edge.  CPU tests prove through the mirror that every
row reaches what it declares, that the table leaves no checklist item without a case, and that the mirror's selected set is
the brute-force top k; GPU tests run every row through merge_lists / rrf_fuse / fuse_packed, from host arrays and from
device tensors, and compare counts, doc ids and score bits for equality.  No tolerance, no skipped row.

The reference is numpy: key = orderable(score) << 32 | ~doc as uint64 (orderable adds +0.0f first: -0.0 ties with +0.0 and
comes back as +0.0), top k of the union in descending key order; RRF = 1/(60+i) + 1/(60+j) with 1-based ranks, f32
divisions added A-then-B in f32, ranked by the same key.  Where a row holds no -0.0 the C oracle (oracle.lib.merge_ranked,
rrf_fuse) must agree as well, which pins the numpy reference to the project's oracle.  NaN scores are not part of the
contract (the producers filter them before pooling) and appear nowhere.

Construction rules:
  * lists are sorted within a shard, docs are distinct within a query's pool (keys of distinct docs are distinct);
  * the slots of a shard's list past its count hold a score of 3e38 and doc ids of their own: a key read past a count lands
    at the top of the output;
  * planted cuts: the sampled flat indices are made the FIRST keys of their segments (one segment per sample) to put the
    pool's best keys under the sample, and the LAST keys of their segments to put its worst there; the c == k case keeps
    k - 1 keys at 2.x, the r-th largest sample alone at 1.0 and everything else at or below 0.5, so the sample's radix stops
    at the second byte on a prefix that exactly k keys reach;
  * hash sets are found by scanning doc ids on the CPU with the kernel's hash.

Beyond the sizes and values, two things the output cannot show are pinned through the mirror: how many candidate keys per thread
the cut hands to the exact select (1 to 4 registers of 1024 keys: planted cuts of 900, 1500, 2500, 3500 and 4096 keys), and which
thread owns the slot just past the pool's end (the last keys of the flat order are the pool's best: a slot at index n taken for
a key doubles one of them).

Not reachable, asserted in the mirror instead of a case:
  * whole waves without a key in the 32-key register class and in the re-loading class: kpt = ceil(n / 1024) >= 16 there, and
    the last wave's first index 15 * 64 * kpt is below 1024 * (kpt - 1) + 1 <= n (test_mirror_select_on_known_shapes).  Those
    two classes have a ragged last wave only;
  * "300 keys of one score whose doc ids differ only in the low byte": 256 ids at most share their upper 24 bits.  The
    shift == 0 rows hold 400 keys of one score with CONSECUTIVE doc ids, k cutting through a full block of 256;
  * a pool of more than 4096 segments (select_topk_kernel) through these three calls: n_shards <= 1024."""
import os
import re
from typing import NamedTuple

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openintel_amd", "csrc")

# ==================================================================== constants of the kernels (checked against the source below)
SEL_THREADS, SEL_MAX, SEL_CAND, SEL_KPT_MAX, SEL_MAX_SEGS = 1024, 1024, 4096, 32, 4096
SEL_CLASSES = (4, 8, 16, 32)           # keys per thread in registers; 0 = the re-loading path
RRF_HASH, RRF_HASH_BITS, RRF_MULT, RRF_K = 4096, 12, 2654435761, 60.0
OI_MAX_DEPTH, MAX_SHARDS = 1024, 1024
PAD_SCORE = np.float32(3e38)
U64 = np.uint64


# ==================================================================== the reference: keys, merge, RRF
def f32_key(scores):
    """oi_f32_key: +0.0f first, then the order-preserving map of the bits."""
    s = np.ascontiguousarray(scores, dtype=np.float32) + np.float32(0.0)
    b = s.view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_f32_bits(k):
    """oi_key_f32, as bits."""
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k).astype(np.uint32)


def rank_keys(scores, docs):
    d = np.ascontiguousarray(docs, dtype=np.uint32)
    return (f32_key(scores).astype(U64) << U64(32)) | (~d).astype(U64)


def decode(keys):
    """-> (score bits, doc ids)"""
    keys = np.asarray(keys, dtype=U64)
    return key_f32_bits((keys >> U64(32)).astype(np.uint32)), ~(keys & U64(0xFFFFFFFF)).astype(np.uint32)


def pool_keys(scores, docs, counts):
    """One query's pool in the flat order of select_flat_kernel: scores / docs [S, depth], counts [S] (clamped to depth)."""
    S, depth = scores.shape
    c = np.minimum(np.asarray(counts, dtype=np.int64), depth)
    keep = np.arange(depth)[None, :] < c[:, None]
    return rank_keys(scores[keep], docs[keep]), c


def ref_merge(scores, docs, counts, k):
    keys, _ = pool_keys(scores, docs, counts)
    return decode(np.sort(keys)[::-1][:k])


def ref_rrf(da, db, k):
    """-> (score bits, doc ids, m = size of the union)"""
    da, db = np.asarray(da, np.uint32), np.asarray(db, np.uint32)
    ra = np.float32(1.0) / (np.float32(RRF_K) + np.arange(1, da.size + 1).astype(np.float32))
    rb = np.float32(1.0) / (np.float32(RRF_K) + np.arange(1, db.size + 1).astype(np.float32))
    where = {int(d): i for i, d in enumerate(da)}
    s, xs, xd = ra.copy(), [], []
    for j, d in enumerate(db):
        i = where.get(int(d))
        if i is None:
            xs.append(rb[j]); xd.append(d)
        else:
            s[i] = ra[i] + rb[j]                  # A, then B, in f32
    keys = rank_keys(np.concatenate([s, np.array(xs, np.float32)]), np.concatenate([da, np.array(xd, np.uint32)]))
    bits, docs = decode(np.sort(keys)[::-1][:k])
    return bits, docs, int(keys.size)


# ==================================================================== mirror: the select
class Pass(NamedTuple):
    shift: int
    digit: int
    lane: int      # wave-0 lane whose four bins hold the digit
    pos: int       # 0..3 inside that lane's bins, counted from the top
    bin_cnt: int


class Radix(NamedTuple):
    passes: tuple
    shift: int
    prefix: int
    stop: str      # "alone" (bin_cnt == 1 above the last byte) | "shift0" (the walk went down to the last byte of the doc id)


def radix_threshold(keys, kk) -> Radix:
    """sel_threshold: 8-bit digits from the top; the wave-0 scan over lanes of four bins, then the walk inside the owner."""
    assert 1 <= kk <= keys.size
    cur, prefix, passes = keys, 0, []
    for shift in range(56, -8, -8):
        dig = ((cur >> U64(shift)) & U64(255)).astype(np.int64)
        hist = np.bincount(dig, minlength=256)
        mine = hist[::-1].reshape(64, 4).sum(axis=1)          # lane l: bins 255 - 4 l - i
        incl = np.cumsum(mine)
        own = np.flatnonzero(incl >= kk)
        owner = int(own[0]) if own.size else 63
        cum, d, pos = int(incl[owner] - mine[owner]), 255 - 4 * owner, 0
        for _ in range(3):
            if cum + hist[d] >= kk:
                break
            cum += int(hist[d]); d -= 1; pos += 1
        prefix, kk = (prefix << 8) | d, kk - cum
        passes.append(Pass(shift, d, owner, pos, int(hist[d])))
        if hist[d] == 1 or shift == 0:
            return Radix(tuple(passes), shift, prefix, "shift0" if shift == 0 else "alone")
        cur = cur[dig == d]


def reaching(keys, rx: Radix):
    return keys[(keys >> U64(rx.shift)) >= U64(rx.prefix)]


def size_class(n):
    for c in SEL_CLASSES:
        if n <= c * SEL_THREADS:
            return c
    return 0


def sample_positions(n):
    """The flat indices the sampled cut reads: thread (wv, lane) samples wv*kpt*64 + lane + 64*(lane % kpt) when < n."""
    kpt = -(-n // SEL_THREADS)
    tid = np.arange(SEL_THREADS)
    wv, lane = tid >> 6, tid & 63
    i = wv * kpt * 64 + lane + 64 * (lane % kpt)
    return np.sort(i[i < n])


class Sel(NamedTuple):
    n: int
    k: int
    KPT: int
    kpt: int
    waves: int           # waves that own a key
    ragged: bool         # the last owning wave owns fewer than kpt * 64 keys
    sampled: bool
    ns: int
    r: int
    sample: Radix        # the sampled threshold (None when not sampled)
    c: int
    outcome: str         # "all" (n <= k) | "exact" (no cut) | "cut" | "c==k" | "c<k" | "c>cand"
    exact: Radix         # the exact select: over the pool, or over the cut ("cut"); None for "all" / "c==k"
    m: int
    P: int
    selected: np.ndarray


def select_trace(keys, k) -> Sel:
    n = int(keys.size)
    KPT, kpt = size_class(n), -(-n // SEL_THREADS)
    waves = -(-n // (kpt * 64)) if n else 0
    ragged = bool(n) and n % (kpt * 64) != 0
    m = min(n, k)
    P = 2
    while P < m:
        P <<= 1
    if n <= k:
        return Sel(n, k, KPT, kpt, waves, ragged, False, 0, 0, None, 0, "all", None, m, P, keys)
    if KPT != 4 and n > SEL_CAND:
        sk = keys[sample_positions(n)]
        ns = int(sk.size)
        r = min(ns, (ns * 2 * k + n - 1) // n + 1)
        srx = radix_threshold(sk, r)
        cut = reaching(keys, srx)
        c = int(cut.size)
        if c == k:
            return Sel(n, k, KPT, kpt, waves, ragged, True, ns, r, srx, c, "c==k", None, m, P, cut)
        if k < c <= SEL_CAND:
            rx = radix_threshold(cut, k)
            return Sel(n, k, KPT, kpt, waves, ragged, True, ns, r, srx, c, "cut", rx, m, P, reaching(cut, rx))
        rx = radix_threshold(keys, k)
        return Sel(n, k, KPT, kpt, waves, ragged, True, ns, r, srx, c, "c<k" if c < k else "c>cand", rx, m, P, reaching(keys, rx))
    rx = radix_threshold(keys, k)
    return Sel(n, k, KPT, kpt, waves, ragged, False, 0, 0, None, 0, "exact", rx, m, P, reaching(keys, rx))


# ==================================================================== mirror: the RRF hash
def rrf_hash(d):
    return ((np.asarray(d, dtype=np.uint64) * U64(RRF_MULT)) & U64(0xFFFFFFFF)) >> U64(32 - RRF_HASH_BITS)


class Rrf(NamedTuple):
    na: int
    nb: int
    m: int
    P: int
    occupied: np.ndarray     # [RRF_HASH] bool: the set of taken slots (independent of the insertion order)
    clusters: tuple          # (start, length) of every maximal run of taken slots, wrapping runs joined
    miss_walk: int           # the longest walk of a B id that is not in A
    wraps: bool              # a cluster starts at a slot >= 4090 and runs through slot 0


def rrf_trace(da, db) -> Rrf:
    da, db = np.asarray(da, np.uint32), np.asarray(db, np.uint32)
    occ = np.zeros(RRF_HASH, bool)
    for h in rrf_hash(da):
        h = int(h)
        while occ[h]:
            h = (h + 1) & (RRF_HASH - 1)
        occ[h] = True
    assert not occ.all()
    clusters = []
    first_free = int(np.flatnonzero(~occ)[0])
    s = first_free
    while True:                                   # walk the ring once from a free slot
        s = (s + 1) % RRF_HASH
        if s == first_free:
            break
        if occ[s] and not occ[s - 1]:
            ln = 0
            while occ[(s + ln) % RRF_HASH]:
                ln += 1
            clusters.append((s, ln))
    inA = set(int(d) for d in da)
    miss = 0
    for d, h in zip(db, rrf_hash(db)):
        if int(d) in inA:
            continue
        h, w = int(h), 0
        while occ[h]:
            h, w = (h + 1) & (RRF_HASH - 1), w + 1
        miss = max(miss, w)
    m = da.size + sum(1 for d in db if int(d) not in inA)
    P = 2
    while P < m:
        P <<= 1
    wraps = any(s >= 4090 and s + ln > RRF_HASH for s, ln in clusters)
    return Rrf(int(da.size), int(db.size), int(m), P, occ, tuple(clusters), miss, wraps)


_SCAN = {}


def ids_hashing_to(slot, count, skip=0):
    """The first `count` doc ids >= 1 (after `skip` of them) that the kernel's hash sends to `slot`."""
    if "h" not in _SCAN:
        _SCAN["h"] = rrf_hash(np.arange(1 << 23, dtype=np.uint32)).astype(np.uint16)
    ids = np.flatnonzero(_SCAN["h"] == slot)
    ids = ids[ids > 0][skip:skip + count].astype(np.uint32)
    assert ids.size == count
    return ids


# ==================================================================== builders
def ragged_counts(n, S, depth, rng):
    assert 0 <= n <= S * depth
    c = np.minimum(rng.multinomial(n, np.full(S, 1.0 / S)), depth).astype(np.int64)
    while c.sum() < n:
        room = np.flatnonzero(c < depth)
        c[rng.choice(room, size=min(int(n - c.sum()), room.size), replace=False)] += 1
    return c


def distinct_docs(n, rng, span=None):
    span = max(4 * n, 16) if span is None else span
    return (rng.permutation(span)[:n] + 3).astype(np.uint32)


def lists_from_flat(scores, docs, counts, depth, pad_base=0xE0000000):
    """A query's pool given in flat order (shard s takes the next counts[s] keys) -> [S, depth] lists, each shard sorted by
    descending key, the slots past a count holding the pad key."""
    counts = np.asarray(counts, dtype=np.int64)
    S, n = counts.size, int(counts.sum())
    assert n == scores.size == docs.size and counts.max(initial=0) <= depth
    seg = np.repeat(np.arange(S), counts)
    keys = rank_keys(scores, docs)
    assert np.unique(keys).size == n, "docs of a pool are distinct"
    o = np.lexsort((~keys, seg))
    rank = np.arange(n) - np.repeat(np.cumsum(counts) - counts, counts)
    out_s = np.full((S, depth), PAD_SCORE, np.float32)
    out_d = (pad_base + np.arange(S * depth, dtype=np.int64)).astype(np.uint32).reshape(S, depth)
    out_s[seg, rank], out_d[seg, rank] = np.asarray(scores, np.float32)[o], np.asarray(docs, np.uint32)[o]
    return out_s, out_d


class Call(NamedTuple):
    scores: np.ndarray   # [S, B, depth]
    docs: np.ndarray
    counts: np.ndarray   # [S, B]; may exceed depth (the kernel clamps)


def call_of(queries, depth, raw_counts=None):
    """queries: [(scores, docs, counts)] in flat order, one per query of the call, all of S shards."""
    ls = [lists_from_flat(s, d, c, depth, 0xE0000000 + (b << 24)) for b, (s, d, c) in enumerate(queries)]
    counts = np.stack([np.asarray(c, np.uint32) for _, _, c in queries], axis=1)
    if raw_counts is not None:
        counts = raw_counts
    return Call(np.ascontiguousarray(np.stack([l[0] for l in ls], axis=1)), np.ascontiguousarray(np.stack([l[1] for l in ls], axis=1)),
                np.ascontiguousarray(counts.astype(np.uint32)))


def rand_query(n, S, depth, rng, kind="normal", counts=None):
    counts = ragged_counts(n, S, depth, rng) if counts is None else np.asarray(counts, np.int64)
    n = int(counts.sum())
    x = rng.standard_normal(n)
    sc = {"normal": x * 0.05, "negative": -np.abs(x) - 0.1, "straddle": x, "ties": np.round(x, 1)}[kind].astype(np.float32)
    return sc, distinct_docs(n, rng), counts


# ---- planted cuts
def _segments_first(n):
    """one segment per sample, the sample its first key"""
    p = sample_positions(n)
    return p, np.diff(np.append(p, n))


def _segments_last(n):
    """one segment per sample, the sample its last key (the keys after the last sample join the last segment)"""
    p = sample_positions(n)
    c = np.diff(np.concatenate([[-1], p]))
    c[-1] += n - 1 - p[-1]
    return p, c


def _sample_r(n, k):
    ns = sample_positions(n).size
    return min(ns, (ns * 2 * k + n - 1) // n + 1)


def planted(n, k, what, seed):
    rng = np.random.default_rng(seed)
    low = rng.uniform(0.01, 0.5, size=n).astype(np.float32)
    docs = distinct_docs(n, rng)
    if what == "c<k":            # every sample above every other key
        p, counts = _segments_first(n)
        low[p] = (2.9 - np.arange(p.size) * 5e-4).astype(np.float32)
    elif what == "c>cand":       # every sample below every key before it
        p, counts = _segments_last(n)
        hi = np.ones(n, bool); hi[p] = False; hi[p[-1]:] = False
        low[hi] = (2.0 + rng.uniform(0, 0.9, size=int(hi.sum()))).astype(np.float32)
        low[p[-1] + 1:] *= np.float32(0.001)
    elif what == "c==k":         # k - 1 keys at 2.x (r - 1 of them samples), the r-th sample alone at 1.0
        p, counts = _segments_first(n)
        r = _sample_r(n, k)
        others = np.setdiff1d(np.arange(p[r - 1]), p)[:k - r]
        assert others.size == k - r, "room for the top keys behind the first r - 1 samples"
        top = np.sort(np.concatenate([p[:r - 1], others]))
        low[top] = (2.9 - np.arange(top.size) * 5e-4).astype(np.float32)
        low[p[r - 1]] = np.float32(1.0)
    elif what[0] == "c":         # exactly what[1] keys reach the sampled threshold: the first r - 1 segments whole and the keys
        p, counts = _segments_last(n)             # before the r-th sample at 2.x, that sample alone at 1.0, then keys of later
        r = _sample_r(n, k)                       # segments (never their samples) until the count is right
        hi = np.zeros(n, bool)
        hi[:p[r - 1]] = True
        later = np.setdiff1d(np.arange(p[r - 1] + 1, p[-1]), p)
        extra = what[1] - 1 - int(hi.sum())
        assert 0 <= extra <= later.size
        hi[rng.permutation(later)[:extra]] = True
        low[hi] = (2.0 + rng.permutation(int(hi.sum())) * 1e-4).astype(np.float32)
        low[p[r - 1]] = np.float32(1.0)
    else:
        raise KeyError(what)
    assert counts.max() <= k and counts.size <= MAX_SHARDS
    return low, docs, counts


# ==================================================================== the merge / select table
class M(NamedTuple):
    name: str
    depth: int
    make: object          # () -> [(scores, docs, counts)] per query, flat order
    edges: tuple
    device: bool = False  # also run from device tensors
    over: bool = False    # counts of full segments are reported above depth


BOUNDARY_N = (4096, 4097, 8192, 8193, 16384, 16385, 32768, 32769)
K_AND_P = ((1, 2), (2, 2), (3, 4), (64, 64), (1000, 1024), (1023, 1024), (1024, 1024))
S_VALUES = (1, 2, 300, 1023, 1024)
CLS = {4: "KPT4", 8: "KPT8", 16: "KPT16", 32: "KPT32", 0: "reload"}
CUTS = ("cut", "c==k", "c<k", "c>cand")

SPECIALS = np.array([np.inf, 3.4028234663852886e38, 1.0, 0.5, 1.1754943508222875e-38, 1e-40, 1.401298464324817e-45, 0.0,
                     -0.0, -1.401298464324817e-45, -1e-40, -1.1754943508222875e-38, -0.5, -1.0, -3.4028234663852886e38, -np.inf],
                    dtype=np.float32)

MERGE_CHECKLIST = (
    ["n:%s:k%d" % (x, k) for k, _ in K_AND_P for x in ("0", "1", "k-1", "k", "k+1")] + ["P:k%d" % k for k, _ in K_AND_P] +
    ["class:n%d" % n for n in BOUNDARY_N] + ["ragged:%s" % CLS[c] for c in (4, 8, 16, 32, 0)] +
    ["idle-waves:%s" % CLS[c] for c in (4, 8, 16)] + ["n:max"] +
    ["S:%d" % s for s in S_VALUES] + ["empty:start", "empty:middle", "empty:end", "walk:over-empty-run:regs", "walk:over-empty-run:reload",
                                      "seg:all-in-last", "seg:one-key-each", "count:above-depth"] +
    ["%s:%s" % (c, w) for c in CUTS for w in ("regs", "reload")] + ["cand:%d-per-thread" % i for i in (1, 2, 3, 4)] +
    ["radix:first-pass", "radix:shift0", "radix:digit0", "radix:digit255", "radix:pos0", "radix:pos1", "radix:pos2", "radix:pos3",
     "radix:lane0", "radix:lane63", "pool:all-negative", "pool:straddles-zero", "own:last-keys-are-best:KPT4", "own:last-keys-are-best:KPT8"] +
    ["val:+inf", "val:-inf", "val:max-normal", "val:min-normal", "val:denormal", "val:+0-beside--0", "val:cut-in-denormals", "val:cut-in-zeros",
     "doc:0-highest", "doc:0-lowest", "doc:max-highest", "doc:max-lowest"] +
    ["multi:classes-in-one-launch", "multi:large-then-small", "abi:ranges"])


def _nk_row(k):
    def make():
        rng = np.random.default_rng(1000 + k)
        return [rand_query(n, 3, k, rng) for n in sorted({0, 1, max(k - 1, 0), k, k + 1})]
    return M("nk-%d" % k, k, make, tuple("n:%s:k%d" % (x, k) for x in ("0", "1", "k-1", "k", "k+1")) + ("P:k%d" % k,))


def _boundary_row(lo, S):
    def make():
        rng = np.random.default_rng(lo)
        return [rand_query(lo, S, 512, rng), rand_query(lo + 1, S, 512, rng)]
    return M("boundary-%d" % lo, 512, make, ("class:n%d" % lo, "class:n%d" % (lo + 1)), device=True)


def _ragged_row(n, S, KPT, idle):
    def make():
        return [rand_query(n, S, 512, np.random.default_rng(n))]
    return M("ragged-%d" % n, 512, make, ("ragged:%s" % CLS[KPT],) + (("idle-waves:%s" % CLS[KPT],) if idle else ()))


def _max_row():
    def make():
        rng = np.random.default_rng(77)
        n = 1 << 20
        return [((rng.standard_normal(n) * 0.05).astype(np.float32), rng.permutation(n).astype(np.uint32) + np.uint32(5), np.full(1024, 1024))]
    return M("max-pool", 1024, make, ("n:max", "S:1024"))


def _geometry_rows():
    def s1():
        rng = np.random.default_rng(31)
        return [rand_query(n, 1, 1024, rng) for n in (0, 500, 1024)]

    def s2():
        rng = np.random.default_rng(32)
        return [rand_query(0, 2, 700, rng, counts=[700, 700]), rand_query(0, 2, 700, rng, counts=[0, 700]), rand_query(0, 2, 700, rng, counts=[700, 1])]

    def s300():
        rng = np.random.default_rng(33)
        c = rng.integers(1, 11, size=300)
        c[:100] = 0; c[150:250] = 0
        return [rand_query(0, 300, 10, rng, counts=c)]

    def s1023():
        rng = np.random.default_rng(34)
        c = rng.integers(1, 65, size=1023)
        c[500:] = 0
        return [rand_query(0, 1023, 64, rng, counts=c)]

    def runs(full):
        def make():
            rng = np.random.default_rng(35 + full)
            c = np.full(1024, 64) if full else rng.integers(1, 17, size=1024)
            c[:100] = 0; c[400:700] = 0; c[924:] = 0
            if not full:
                c[399] = 64; c[700] = 64          # a thread's next key, 64 further on, lies beyond the empty run
            return [rand_query(0, 1024, 64, rng, counts=c)]
        return make

    def one_each():
        return [rand_query(0, 1024, 64, np.random.default_rng(37), counts=np.ones(1024, np.int64))]

    def all_in_last():
        c = np.zeros(1024, np.int64); c[-1] = 64
        return [rand_query(0, 1024, 64, np.random.default_rng(38), counts=c)]

    def over():
        rng = np.random.default_rng(39)
        return [rand_query(0, 5, 100, rng, counts=[100, 37, 100, 0, 100]), rand_query(0, 5, 100, rng, counts=[100, 100, 100, 100, 100])]

    return [M("S1", 1024, s1, ("S:1",)), M("S2", 700, s2, ("S:2",)), M("S300-empty-runs", 10, s300, ("S:300", "empty:start", "empty:middle")),
            M("S1023-empty-end", 64, s1023, ("S:1023", "empty:end")),
            M("empty-runs-regs", 64, runs(False), ("S:1024", "empty:start", "empty:middle", "empty:end", "walk:over-empty-run:regs")),
            M("empty-runs-reload", 64, runs(True), ("walk:over-empty-run:reload",)),
            M("one-key-each", 64, one_each, ("seg:one-key-each",)), M("all-in-last", 64, all_in_last, ("seg:all-in-last",)),
            M("count-above-depth", 100, over, ("count:above-depth",), over=True)]


def _cut_rows():
    rows = []
    for w, n, k, S in (("regs", 8192, 64, 0), ("reload", 33792, 128, 0)):
        for what in ("c==k", "c<k", "c>cand"):
            rows.append(M("planted-%s-%s" % (what, w), k, (lambda n=n, k=k, what=what: [planted(n, k, what, n + k)]), ("%s:%s" % (what, w),), device=True))
    for per, target in ((1, 900), (2, 1500), (3, 2500), (4, 3500)):
        rows.append(M("cand-%d-per-thread" % per, 64, (lambda target=target: [planted(8192, 64, ("c", target), target)]), ("cand:%d-per-thread" % per,)))
    rows.append(M("cand-4-per-thread-reload", 128, lambda: [planted(33792, 128, ("c", 4096), 5)], ("cand:4-per-thread", "cut:reload"), device=True))
    rows.append(M("cut-ok-regs", 512, lambda: [rand_query(8192, 17, 512, np.random.default_rng(81))], ("cut:regs",), device=True))
    rows.append(M("cut-ok-reload", 512, lambda: [rand_query(33000, 65, 512, np.random.default_rng(82))], ("cut:reload", "ragged:reload"), device=True))
    return rows


def _radix_rows():
    def first_pass():
        sc, dd, c = rand_query(0, 1024, 1, np.random.default_rng(91), counts=np.ones(1024, np.int64))
        sc[333] = np.float32(1e30)
        return [(sc, dd, c)]

    def shift0(extra):
        def make():
            rng = np.random.default_rng(92 + extra)
            tie_docs = (0x10000 + np.arange(400)).astype(np.uint32)
            sc = np.concatenate([np.full(400, 0.25, np.float32), rng.uniform(-1, 0.2, size=extra).astype(np.float32)])
            dd = np.concatenate([tie_docs, (0x900000 + rng.permutation(4 * extra + 4)[:extra]).astype(np.uint32)])
            o = rng.permutation(sc.size)
            S = 4 if extra < 1000 else 40
            return [(sc[o], dd[o], ragged_counts(sc.size, S, 200, rng))]
        return make

    def infs():
        rng = np.random.default_rng(94)
        a = rng.standard_normal(64).astype(np.float32); a[:30] = np.inf       # the 8th key is a +inf: digits 255, 128, 0, 0
        b = rng.standard_normal(40).astype(np.float32); b[:36] = -np.inf      # the 8th key is a -inf: digits 0, 127, 255, 255
        return [(a, distinct_docs(64, rng), ragged_counts(64, 8, 8, rng)), (b, distinct_docs(40, rng), ragged_counts(40, 8, 8, rng))]

    def signs(n, S):
        def make():
            rng = np.random.default_rng(95 + n)
            return [rand_query(n, S, 512, rng, "negative"), rand_query(n, S, 512, rng, "straddle"), rand_query(n, S, 512, rng, "ties")]
        return make

    def last_best(n, S):
        def make():                               # the last 100 keys of the flat order are the pool's best 100
            rng = np.random.default_rng(97 + n)
            c = ragged_counts(n - 100, S - 1, 512, rng)
            sc, dd, _ = rand_query(0, S - 1, 512, rng, counts=c)
            return [(np.concatenate([sc, (5.0 + rng.uniform(0, 1, 100)).astype(np.float32)]),
                     np.concatenate([dd, (0x7000000 + np.arange(100)).astype(np.uint32)]), np.append(c, 100))]
        return make

    return [M("radix-first-pass", 1, first_pass, ("radix:first-pass",)),
            M("radix-shift0", 200, shift0(100), ("radix:shift0",), device=True),
            M("radix-shift0-cut", 200, shift0(6000), ("radix:shift0",)),
            M("radix-infs", 8, infs, ("radix:digit0", "radix:digit255", "radix:pos0", "radix:pos3", "radix:lane0", "radix:lane63", "val:+inf", "val:-inf")),
            M("signs-3000", 512, signs(3000, 9), ("pool:all-negative", "pool:straddles-zero", "radix:pos1", "radix:pos2")),
            M("signs-9000", 512, signs(9000, 33), ("pool:all-negative", "pool:straddles-zero")),
            M("last-best-KPT4", 512, last_best(3003, 9), ("own:last-keys-are-best:KPT4",)),
            M("last-best-KPT8", 512, last_best(6021, 17), ("own:last-keys-are-best:KPT8",))]


def _value_rows():
    def make():
        rng = np.random.default_rng(99)
        v = SPECIALS
        d0 = distinct_docs(16, rng); d0[0], d0[15] = 0, 0xFFFFFFFF             # doc 0: +inf, doc 2^32 - 1: -inf
        d1 = distinct_docs(16, rng); d1[0], d1[15] = 0xFFFFFFFF, 0
        v3 = np.repeat(v, 3)                                                   # the 16th of 48 is a 1.4e-45
        neg = np.repeat(v[7:], 3)                                              # zeros first: the 16th of 27 is a -min normal ...
        zer = np.concatenate([np.tile(np.float32([0.0, -0.0]), 12), v[9:]])    # ... and here the 16th is one of 24 zeros
        q = [(v, d0, ragged_counts(16, 8, 16, rng)), (v, d1, ragged_counts(16, 8, 16, rng)),
             (v3, distinct_docs(48, rng), ragged_counts(48, 8, 16, rng)), (neg, distinct_docs(neg.size, rng), ragged_counts(neg.size, 8, 16, rng)),
             (zer, distinct_docs(zer.size, rng), ragged_counts(zer.size, 8, 16, rng))]
        return q
    return [M("special-values", 16, make, ("val:+inf", "val:-inf", "val:max-normal", "val:min-normal", "val:denormal", "val:+0-beside--0",
                                           "val:cut-in-denormals", "val:cut-in-zeros", "doc:0-highest", "doc:0-lowest", "doc:max-highest",
                                           "doc:max-lowest"), device=True)]


MULTI_N = (0, 5, 4097, 8193, 16385, 32769)


def _multi_row():
    def make():
        rng = np.random.default_rng(111)
        return [rand_query(n, 33, 1024, rng) for n in MULTI_N]
    return M("classes-in-one-launch", 1024, make, ("multi:classes-in-one-launch",), device=True)


MERGE_ROWS = ([_nk_row(k) for k, _ in K_AND_P] + [_boundary_row(4096, 9), _boundary_row(8192, 17), _boundary_row(16384, 33), _boundary_row(32768, 65)] +
              [_ragged_row(2100, 5, 4, True), _ragged_row(5130, 11, 8, True), _ragged_row(8500, 17, 16, True), _ragged_row(17000, 34, 32, False)] +
              [_max_row()] + _geometry_rows() + _cut_rows() + _radix_rows() + _value_rows() + [_multi_row()])
MERGE_BY_NAME = {r.name: r for r in MERGE_ROWS}
MERGE_TESTS_OF_THEIR_OWN = ("multi:large-then-small", "abi:ranges")
_CALLS = {}


def merge_call(name) -> Call:
    if name not in _CALLS:
        row = MERGE_BY_NAME[name]
        qs = row.make()
        raw = None
        if row.over:
            raw = np.stack([np.where(np.asarray(c) == row.depth, row.depth + 7 + 1000 * np.arange(len(c)), c) for _, _, c in qs], axis=1)
        _CALLS[name] = call_of(qs, row.depth, raw)
    return _CALLS[name]


def _zero_runs(c):
    """(start, length) of the runs of empty segments"""
    z = np.concatenate([[0], (np.asarray(c) == 0).astype(np.int64), [0]])
    d = np.diff(z)
    return list(zip(np.flatnonzero(d == 1), np.flatnonzero(d == -1) - np.flatnonzero(d == 1)))


def reached_merge(call: Call):
    """-> (edges the call reaches, [Sel] per query)"""
    S, B, depth = call.scores.shape
    k, out, traces = depth, set(), []
    if S in S_VALUES:
        out.add("S:%d" % S)
    if (call.counts > depth).any():
        out.add("count:above-depth")
    for b in range(B):
        keys, c = pool_keys(call.scores[:, b], call.docs[:, b], call.counts[:, b])
        t = select_trace(keys, k)
        traces.append(t)
        n = t.n
        for x, v in (("0", 0), ("1", 1), ("k-1", k - 1), ("k", k), ("k+1", k + 1)):
            if n == v:
                out.add("n:%s:k%d" % (x, k))
        if n >= k and (k, t.P) in K_AND_P:
            out.add("P:k%d" % k)
        if n in BOUNDARY_N:
            out.add("class:n%d" % n)
        if n == MAX_SHARDS * OI_MAX_DEPTH:
            out.add("n:max")
        if n > k and n % SEL_THREADS and t.ragged:
            out.add("ragged:%s" % CLS[t.KPT])
            if t.waves < SEL_THREADS // 64:
                out.add("idle-waves:%s" % CLS[t.KPT])
        # segment geometry
        runs = [(s, ln) for s, ln in _zero_runs(c) if ln >= 50] if n else []
        seg_of = np.repeat(np.arange(S), c)
        for s, ln in runs:
            out.add("empty:start" if s == 0 else "empty:end" if s + ln == S else "empty:middle")
            if 0 < s and s + ln < S and n > k and t.kpt >= 2:      # a thread's consecutive keys i, i + 64 on the two sides of the run
                i = np.arange(n - 64)
                same_wave = i // (t.kpt * 64) == (i + 64) // (t.kpt * 64)
                if (same_wave & (seg_of[i] < s) & (seg_of[i + 64] >= s + ln)).any():
                    out.add("walk:over-empty-run:%s" % ("regs" if t.KPT else "reload"))
        if n and (c == 1).all():
            out.add("seg:one-key-each")
        if n and c[-1] == n and S > 1:
            out.add("seg:all-in-last")
        # the cut and the radix
        if t.sampled:
            out.add("%s:%s" % (t.outcome, "regs" if t.KPT else "reload"))
            if t.outcome == "cut":                # the cut's keys go back into registers, c / 1024 of them per thread
                out.add("cand:%d-per-thread" % -(-t.c // SEL_THREADS))
        rxs = [r for r in (t.sample, t.exact) if r is not None]
        if t.exact is not None and len(t.exact.passes) == 1 and t.exact.stop == "alone" and k == 1:
            out.add("radix:first-pass")
        if t.exact is not None and t.exact.stop == "shift0":
            bits, docs = decode(keys)
            kth = np.sort(keys)[::-1][k - 1]
            tied = docs[bits == decode(np.array([kth]))[0][0]]
            if tied.size >= 300 and (tied >> 8 == (decode(np.array([kth]))[1][0] >> 8)).sum() == 256:
                out.add("radix:shift0")
        for r in rxs:
            for p in r.passes:
                if p.digit in (0, 255):
                    out.add("radix:digit%d" % p.digit)
                out.add("radix:pos%d" % p.pos)
                if p.lane in (0, 63):
                    out.add("radix:lane%d" % p.lane)
        if n > k:
            bits, docs = decode(keys)
            fl = bits.view(np.float32)
            if (fl < 0).all():
                out.add("pool:all-negative")
            if (fl < 0).any() and (fl > 0).any() and np.isfinite(fl).all():
                out.add("pool:straddles-zero")
            top = np.sort(keys)[::-1][:k]
            if n % SEL_THREADS and n > SEL_THREADS and np.isin(keys[[n - 64, n - 1]], top).all() and t.KPT in (4, 8):
                out.add("own:last-keys-are-best:%s" % CLS[t.KPT])
        # values (of the inputs: -0.0 is gone from the keys)
        keep = np.arange(depth)[None, :] < c[:, None]
        raw, rd = call.scores[:, b][keep], call.docs[:, b][keep]
        rb = raw.view(np.uint32)
        if n:
            hi, lo = raw.max(), raw.min()
            for name, bit in (("+inf", 0x7F800000), ("-inf", 0xFF800000)):
                if (rb == bit).any():
                    out.add("val:" + name)
            if (np.abs(raw) == SPECIALS[1]).any():
                out.add("val:max-normal")
            if (np.abs(raw) == SPECIALS[4]).any():
                out.add("val:min-normal")
            if ((rb & 0x7F800000) == 0).any() and ((rb & 0x007FFFFF) != 0)[(rb & 0x7F800000) == 0].any():
                out.add("val:denormal")
            if (rb == 0).any() and (rb == 0x80000000).any():
                out.add("val:+0-beside--0")
            if n > k:
                kb = int(decode(np.sort(keys)[::-1][k - 1:k])[0][0])
                if kb & 0x7F800000 == 0:
                    out.add("val:cut-in-zeros" if kb & 0x7FFFFFFF == 0 else "val:cut-in-denormals")
            for d, dn in ((0, "0"), (0xFFFFFFFF, "max")):
                w = np.flatnonzero(rd == d)
                if w.size and raw[w[0]] == hi:
                    out.add("doc:%s-highest" % dn)
                if w.size and raw[w[0]] == lo:
                    out.add("doc:%s-lowest" % dn)
    if B >= 4 and any(t.n == 0 for t in traces) and len({t.KPT for t in traces if t.n}) >= 4:
        out.add("multi:classes-in-one-launch")
    return out, traces


# ==================================================================== the RRF table
class R(NamedTuple):
    name: str
    depth: int
    make: object          # () -> (docs_a [B, depth], counts_a [B], docs_b, counts_b); a count may exceed depth
    ks: tuple             # () = 1, 1024 and m - 1, m, m + 1 of every query
    edges: tuple


RRF_DEPTHS = (1, 7, 1024)
RRF_CHECKLIST = (
    ["len:%d,%d:depth%d" % (a, b, d) for d in RRF_DEPTHS for a in sorted({0, 1, d}) for b in sorted({0, 1, d})] +
    ["k:%s:depth%d" % (x, d) for d in RRF_DEPTHS for x in ("1", "m-1", "m", "m+1", "1024")] +
    ["rrf:identical", "rrf:disjoint-2048", "rrf:count-above-depth", "hash:one-slot-1024", "hash:wrap", "hash:miss-walks-cluster",
     "hash:hit-at-cluster-end", "id:0:A", "id:0:B", "id:0:both", "id:max:A", "id:max:B", "id:max:both", "tie:single-ranks", "tie:swapped-pairs",
     "abi:rrf-ranges"])


def _pad_ids(B, depth, base):
    return (base + np.arange(B * depth, dtype=np.int64)).astype(np.uint32).reshape(B, depth)


def _rrf_pack(pairs, depth, over=0):
    """pairs: [(ids_a, ids_b)] -> the four arrays; the slots past a count hold ids that are in no list (and ids of list A in
    list B's, so that a lookup past the count would be a hit)."""
    B = len(pairs)
    da, db = _pad_ids(B, depth, 0xA0000000), _pad_ids(B, depth, 0xB0000000)
    ca, cb = np.zeros(B, np.uint32), np.zeros(B, np.uint32)
    for b, (a, bb) in enumerate(pairs):
        a, bb = np.asarray(a, np.uint32), np.asarray(bb, np.uint32)
        assert np.unique(a).size == a.size and np.unique(bb).size == bb.size
        da[b, :a.size], db[b, :bb.size] = a, bb
        if a.size and bb.size < depth:
            db[b, bb.size:] = np.resize(a, depth - bb.size)
        ca[b], cb[b] = a.size + (over if a.size == depth else 0), bb.size + (over if bb.size == depth else 0)
    return da, ca, db, cb


def _lengths_row(depth):
    def make():
        rng = np.random.default_rng(200 + depth)
        pool = rng.permutation(50000)[:2 * depth].astype(np.uint32) + 1
        a_full, fresh = pool[:depth], pool[depth:]
        pairs = []
        for na in sorted({0, 1, depth}):
            for nb in sorted({0, 1, depth}):
                b_full = np.where(np.arange(depth) % 2 == 0, a_full[::-1], fresh)     # every other B id is in A, at another rank
                pairs.append((a_full[:na], b_full[:nb]))
        pairs.append((a_full[:1], fresh[:1]))     # m = 2 at every depth: k = m - 1 exists at depth 1 too
        return _rrf_pack(pairs, depth)
    e = ["len:%d,%d:depth%d" % (a, b, depth) for a in sorted({0, 1, depth}) for b in sorted({0, 1, depth})]
    return R("lengths-%d" % depth, depth, make, (), tuple(e) + tuple("k:%s:depth%d" % (x, depth) for x in ("1", "m-1", "m", "m+1", "1024")))


def _rrf_rows():
    def identical():
        rng = np.random.default_rng(210)
        a = rng.permutation(1 << 20)[:1024].astype(np.uint32)
        return _rrf_pack([(a, a), (a, a[::-1]), (a[:7], a[:7])], 1024)

    def disjoint():
        rng = np.random.default_rng(211)
        a = rng.permutation(1 << 20)[:2048].astype(np.uint32)
        return _rrf_pack([(a[:1024], a[1024:]), (a[1024:], a[:1024])], 1024)

    def above(depth):
        def make():
            rng = np.random.default_rng(212 + depth)
            a = rng.permutation(1 << 20)[:2 * depth].astype(np.uint32)
            return _rrf_pack([(a[:depth], a[depth // 2:depth // 2 + depth]), (a[:depth], a[:depth // 2])], depth, over=5)
        return make

    def one_slot():
        a = ids_hashing_to(77, 1024)
        absent = ids_hashing_to(77, 512, skip=1024)
        rng = np.random.default_rng(213)
        return _rrf_pack([(a, np.concatenate([rng.permutation(a)[:512], absent])), (a, rng.permutation(a))], 1024)

    def wrap():
        rng = np.random.default_rng(214)
        a = np.concatenate([ids_hashing_to(4090, 40), ids_hashing_to(1000, 30)])
        miss = np.concatenate([ids_hashing_to(4090, 10, skip=40), ids_hashing_to(4092, 10), ids_hashing_to(0, 10)])
        return _rrf_pack([(rng.permutation(a), rng.permutation(np.concatenate([a[:40], miss])))], 1024)

    def zero_max():
        rng = np.random.default_rng(215)
        f = rng.permutation(1 << 20)[:40].astype(np.uint32) + 7
        Z, X = np.uint32(0), np.uint32(0xFFFFFFFF)
        with_ = lambda ids, at, v: np.concatenate([ids[:at], [v], ids[at:]]).astype(np.uint32)
        return _rrf_pack([(with_(with_(f[:10], 3, Z), 7, X), f[5:20]),                         # A only
                          (f[:10], with_(with_(f[5:20], 0, X), 9, Z)),                         # B only
                          (with_(with_(f[:10], 10, Z), 0, X), with_(with_(f[5:20], 2, Z), 16, X)),   # both, at other ranks
                          (np.array([Z], np.uint32), np.array([Z], np.uint32)), (np.array([X], np.uint32), np.array([], np.uint32))], 32)

    def ties():
        # single ranks: a_i and b_i tie at every rank, the lower id first (a_i < b_i at odd i, a_i > b_i at even i);
        # swapped pairs: x at (1, 2) with y at (2, 1), p at (5, 8) with q at (8, 5)
        a = np.array([100 + 10 * i + (0 if i % 2 else 5) for i in range(8)], np.uint32)
        b = np.array([100 + 10 * i + (5 if i % 2 else 0) for i in range(8)], np.uint32)
        x, y, p, q = 900, 800, 700, 701
        A = np.array([x, y, 11, 12, p, 13, 14, q], np.uint32)
        Bq = np.array([y, x, 21, 22, q, 23, 24, p], np.uint32)
        return _rrf_pack([(a, b), (A, Bq)], 8)

    return [R("identical", 1024, identical, (1, 7, 1023, 1024), ("rrf:identical",)),
            R("disjoint-2048", 1024, disjoint, (1, 1000, 1024), ("rrf:disjoint-2048",)),
            R("count-above-depth-7", 7, above(7), (1, 5, 1024), ("rrf:count-above-depth",)),
            R("count-above-depth-1024", 1024, above(1024), (1024,), ("rrf:count-above-depth",)),
            R("one-slot", 1024, one_slot, (1024, 100), ("hash:one-slot-1024", "hash:miss-walks-cluster", "hash:hit-at-cluster-end")),
            R("wrap", 1024, wrap, (1024, 10), ("hash:wrap", "hash:miss-walks-cluster", "hash:hit-at-cluster-end")),
            R("ids-0-and-max", 32, zero_max, (1, 64), ("id:0:A", "id:0:B", "id:0:both", "id:max:A", "id:max:B", "id:max:both")),
            R("ties", 8, ties, (16, 3), ("tie:single-ranks", "tie:swapped-pairs"))]


RRF_ROWS = [_lengths_row(d) for d in RRF_DEPTHS] + _rrf_rows()
RRF_BY_NAME = {r.name: r for r in RRF_ROWS}
RRF_TESTS_OF_THEIR_OWN = ("abi:rrf-ranges",)
_RRF_CALLS = {}


def rrf_call(name):
    if name not in _RRF_CALLS:
        _RRF_CALLS[name] = RRF_BY_NAME[name].make()
    return _RRF_CALLS[name]


def rrf_lists(call, b):
    da, ca, db, cb = call
    depth = da.shape[1]
    return da[b, :min(int(ca[b]), depth)], db[b, :min(int(cb[b]), depth)]


def rrf_ks(row: R, call):
    if row.ks:
        return row.ks
    ks = {1, 1024}
    for b in range(call[0].shape[0]):
        m = ref_rrf(*rrf_lists(call, b), 1)[2]
        ks |= {m - 1, m, m + 1}
    return tuple(sorted(k for k in ks if 1 <= k <= OI_MAX_DEPTH))


def reached_rrf(row: R, call):
    out = set()
    da, ca, db, cb = call
    depth, ks = da.shape[1], rrf_ks(row, call)
    if (ca > depth).any() and (cb > depth).any():
        out.add("rrf:count-above-depth")
    for b in range(da.shape[0]):
        a, bb = rrf_lists(call, b)
        t = rrf_trace(a, bb)
        if depth in RRF_DEPTHS and t.na in (0, 1, depth) and t.nb in (0, 1, depth):
            out.add("len:%d,%d:depth%d" % (t.na, t.nb, depth))
        if depth in RRF_DEPTHS:
            for k in ks:
                for x, v in (("1", 1), ("m-1", t.m - 1), ("m", t.m), ("m+1", t.m + 1), ("1024", 1024)):
                    if k == v:
                        out.add("k:%s:depth%d" % (x, depth))
        if t.na == 1024 and t.m == t.na and t.nb == t.na:
            out.add("rrf:identical")
        if t.m == 2048 and t.P == 2048:
            out.add("rrf:disjoint-2048")
        ha = rrf_hash(a)
        if t.na == 1024 and np.unique(ha).size == 1:
            out.add("hash:one-slot-1024")
        if t.wraps:
            out.add("hash:wrap")
        for s, ln in t.clusters:
            members = a[(ha.astype(np.int64) - s) % RRF_HASH < ln]
            if ln >= 16 and t.miss_walk >= ln:
                out.add("hash:miss-walks-cluster")
            # every id of the cluster has the cluster's first slot as its home, so ANY of them may sit at its end, and all are in B
            if ln >= 16 and (rrf_hash(members) == s).all() and members.size == ln and np.isin(members, bb).all():
                out.add("hash:hit-at-cluster-end")
        for d, dn in ((0, "0"), (0xFFFFFFFF, "max")):
            ia, ib = (a == d).any(), (bb == d).any()
            if ia or ib:
                out.add("id:%s:%s" % (dn, "both" if ia and ib else "A" if ia else "B"))
        # ties, read off the reference's own output
        bits, docs, m = ref_rrf(a, bb, 2048)
        pa, pb = {int(d): i for i, d in enumerate(a)}, {int(d): i for i, d in enumerate(bb)}
        for i in range(m - 1):
            if bits[i] == bits[i + 1]:
                assert docs[i] < docs[i + 1]
                u, v = int(docs[i]), int(docs[i + 1])
                if (u in pa) != (u in pb) and (v in pa) != (v in pb) and (u in pa) != (v in pa):
                    out.add("tie:single-ranks")
                if u in pa and u in pb and v in pa and v in pb and pa[u] != pb[u] and (pa[u], pb[u]) == (pb[v], pa[v]):
                    out.add("tie:swapped-pairs")
    return out


# ==================================================================== the packed table
class Pk(NamedTuple):
    name: str
    S: int
    depth: int
    sizes: tuple          # per query: (cosine pool size, BM25 pool size)
    ks: tuple
    edges: tuple


PACKED_ROWS = [Pk("packed-S1", 1, 1024, ((0, 1024), (700, 0), (1024, 3)), (10, 1024), ("packed:S1", "packed:empty-cosine", "packed:empty-bm25")),
               Pk("packed-S2", 2, 700, ((0, 1400), (900, 0), (1400, 20)), (10, 1024), ("packed:S2", "packed:empty-cosine", "packed:empty-bm25")),
               Pk("packed-S1024", 1024, 40, ((0, 3000), (9000, 0), (40960, 5000)), (10, 1024),
                  ("packed:S1024", "packed:empty-cosine", "packed:empty-bm25", "packed:two-classes-in-one-query"))]
PACKED_BY_NAME = {r.name: r for r in PACKED_ROWS}
PACKED_CHECKLIST = ["packed:S1", "packed:S2", "packed:S1024", "packed:empty-cosine", "packed:empty-bm25", "packed:two-classes-in-one-query",
                    "packed:device-replay-follows-contents"]
PACKED_TESTS_OF_THEIR_OWN = ("packed:device-replay-follows-contents",)
_PACKED = {}


def packed_lists(row: Pk, seed=0):
    """-> (cos Call, bm25 Call) of B = 3 queries: shard s holds the docs s + S j, the two lists of a query share docs."""
    key = (row.name, seed)
    if key not in _PACKED:
        rng = np.random.default_rng(300 + row.S + seed)
        calls = []
        for which in (0, 1):
            qs = []
            for sizes in row.sizes:
                n = sizes[which]
                c = ragged_counts(n, row.S, row.depth, rng)
                seg = np.repeat(np.arange(row.S), c)
                j = np.concatenate([rng.permutation(2 * row.depth)[:x] for x in c]) if n else np.zeros(0, np.int64)
                docs = (seg + row.S * j + 11).astype(np.uint32)
                sc = (rng.standard_normal(n) * (0.05 if which == 0 else 3.0) + (0 if which == 0 else 9.0)).astype(np.float32)
                qs.append((sc, docs, c))
            calls.append(call_of(qs, row.depth))
        _PACKED[key] = tuple(calls)
    return _PACKED[key]


def pack(cos: Call, bm: Call):
    """The OI_PACKED_WORDS layout, shard after shard: scores [2][B][depth], docs [2][B][depth], counts [2][B]."""
    S = cos.scores.shape[0]
    out = []
    for s in range(S):
        out += [cos.scores[s].ravel().view(np.uint32), bm.scores[s].ravel().view(np.uint32), cos.docs[s].ravel(), bm.docs[s].ravel(),
                cos.counts[s], bm.counts[s]]
    return np.ascontiguousarray(np.concatenate(out).astype(np.uint32))


def ref_packed(cos: Call, bm: Call, k):
    S, B, depth = cos.scores.shape
    out = []
    for b in range(B):
        _, cd = ref_merge(cos.scores[:, b], cos.docs[:, b], cos.counts[:, b], depth)
        _, bd = ref_merge(bm.scores[:, b], bm.docs[:, b], bm.counts[:, b], depth)
        out.append(ref_rrf(cd, bd, k)[:2])
    return out


def reached_packed(row: Pk):
    cos, bm = packed_lists(row)
    out = {"packed:S%d" % row.S}
    for b in range(3):
        nc, nb = int(np.minimum(cos.counts[:, b], row.depth).sum()), int(np.minimum(bm.counts[:, b], row.depth).sum())
        assert (nc, nb) == row.sizes[b]
        if nc == 0 and nb:
            out.add("packed:empty-cosine")
        if nb == 0 and nc:
            out.add("packed:empty-bm25")
        if nc > row.depth and nb > row.depth and size_class(nc) != size_class(nb):
            out.add("packed:two-classes-in-one-query")
    return out


CHECKLIST = MERGE_CHECKLIST + RRF_CHECKLIST + PACKED_CHECKLIST


# ==================================================================== CPU tests
def _defines(path):
    out = {}
    for m in re.finditer(r"^\s*#\s*define\s+(\w+)\s+(\S+)", open(path).read(), re.M):
        out.setdefault(m.group(1), m.group(2))
    return out


def test_mirror_constants_equal_the_sources():
    """A retune of the kernels breaks the table loudly: every mirrored constant is read from select.hip."""
    path = os.path.join(CSRC, "select.hip")
    d, src = _defines(path), open(path).read()
    num = lambda s: int(s.rstrip("uU"))
    for name, want in (("SEL_THREADS", SEL_THREADS), ("SEL_MAX", SEL_MAX), ("SEL_CAND", SEL_CAND), ("SEL_KPT_MAX", SEL_KPT_MAX),
                       ("SEL_MAX_SEGS", SEL_MAX_SEGS), ("RRF_HASH", RRF_HASH)):
        assert num(d[name]) == want, name
    assert RRF_HASH == 1 << RRF_HASH_BITS
    assert src.count("(d * %du) >> %d" % (RRF_MULT, 32 - RRF_HASH_BITS)) == 2            # insert and lookup
    assert src.count("1.0f / (%.1ff + (float)" % RRF_K) == 3
    for c in SEL_CLASSES[:3]:
        assert "if (n <= %d * SEL_THREADS) return f(SelClass<%d>{});" % (c, c) in src
    assert "if (n <= SEL_KPT_MAX * SEL_THREADS) return f(SelClass<SEL_KPT_MAX>{});" in src and SEL_CLASSES[3] == SEL_KPT_MAX
    assert "if (KPT != 4 && n > SEL_CAND)" in src and "if (c >= k && c <= SEL_CAND)" in src and "if (c == k)" in src
    assert "const uint32_t js = lane % kpt, is = first + js * 64;" in src
    assert "uint32_t r = (uint32_t)(((uint64_t)ns * (2 * k) + n - 1) / n) + 1;" in src
    assert "const uint32_t first = wv * kpt * 64 + lane, last = n - 1;" in src
    public = _defines(os.path.join(ROOT, "include", "openintel_hip.h"))
    assert num(public["OI_MAX_DEPTH"]) == OI_MAX_DEPTH == SEL_MAX
    api = open(os.path.join(CSRC, "api.hip")).read()
    assert api.count("n_shards >= 1 && n_shards <= %d" % MAX_SHARDS) == 2                 # merge_lists and fuse_packed
    assert "return s + 0.0f" in src or "s += 0.0f;" in open(os.path.join(CSRC, "oi_device.h")).read()


@pytest.mark.parametrize("name", [r.name for r in MERGE_ROWS])
def test_every_merge_row_reaches_the_edges_it_declares(name):
    """... and the mirror's selected set is the brute-force top k of the pool, for every query of the row."""
    row, call = MERGE_BY_NAME[name], merge_call(name)
    S, B, depth = call.scores.shape
    assert 1 <= S <= MAX_SHARDS and 1 <= depth <= OI_MAX_DEPTH and depth == row.depth
    got, traces = reached_merge(call)
    assert set(row.edges) <= got, (name, sorted(set(row.edges) - got))
    for b, t in enumerate(traces):
        keys, c = pool_keys(call.scores[:, b], call.docs[:, b], call.counts[:, b])
        assert np.unique(keys).size == keys.size
        for s in range(S):                        # sorted within a shard
            assert (np.diff(rank_keys(call.scores[s, b, :c[s]], call.docs[s, b, :c[s]]).astype(object)) < 0).all() if c[s] > 1 else True
        want = np.sort(keys)[::-1][:depth]
        assert t.m == want.size and np.array_equal(np.sort(t.selected)[::-1], want), (name, b, t.outcome)
        if t.sampled:
            assert t.c >= t.r >= 1 and t.ns <= SEL_THREADS
        assert t.KPT == 0 or t.kpt <= t.KPT
        if t.kpt >= 16:
            assert t.waves == 16                  # (the module's docstring: no idle wave in these classes)


@pytest.mark.parametrize("name", [r.name for r in RRF_ROWS])
def test_every_rrf_row_reaches_the_edges_it_declares(name):
    row, call = RRF_BY_NAME[name], rrf_call(name)
    got = reached_rrf(row, call)
    assert set(row.edges) <= got, (name, sorted(set(row.edges) - got))
    assert 1 <= row.depth <= OI_MAX_DEPTH and all(1 <= k <= OI_MAX_DEPTH for k in rrf_ks(row, call))


def test_the_table_covers_the_whole_checklist():
    declared = set(MERGE_TESTS_OF_THEIR_OWN) | set(RRF_TESTS_OF_THEIR_OWN) | set(PACKED_TESTS_OF_THEIR_OWN)
    for r in MERGE_ROWS + RRF_ROWS + PACKED_ROWS:
        declared |= set(r.edges)
    for r in PACKED_ROWS:
        assert set(r.edges) <= reached_packed(r), r.name
    assert len(set(CHECKLIST)) == len(CHECKLIST)
    assert set(CHECKLIST) <= declared, sorted(set(CHECKLIST) - declared)
    assert declared <= set(CHECKLIST), sorted(declared - set(CHECKLIST))
    # the device subset: one row per size class, the four outcomes of the cut in both kinds of class, the shift == 0 row
    dev = [r for r in MERGE_ROWS if r.device]
    classes, cuts, shift0 = set(), set(), False
    for r in dev:
        for t in reached_merge(merge_call(r.name))[1]:
            classes.add(t.KPT)
            if t.sampled:
                cuts.add((t.outcome, bool(t.KPT)))
            shift0 |= t.exact is not None and t.exact.stop == "shift0"
    assert classes == {4, 8, 16, 32, 0} and cuts == {(c, w) for c in CUTS for w in (True, False)} and shift0


def test_mirror_select_on_known_shapes():
    assert [size_class(n) for n in (1, 4096, 4097, 8192, 8193, 16384, 16385, 32768, 32769, 1 << 20)] == [4, 4, 8, 8, 16, 16, 32, 32, 0, 0]
    # no idle wave from kpt = 16 on: the last wave's first index is below n
    for kpt in range(16, 1025):
        assert 15 * 64 * kpt < 1024 * (kpt - 1) + 1
    assert any(15 * 64 * kpt >= 1024 * (kpt - 1) + 1 for kpt in range(2, 16))
    # the sample: one index per thread, all distinct, inside the thread's wave
    for n in (4097, 8192, 8500, 33000, 1 << 20):
        p = sample_positions(n)
        kpt = -(-n // 1024)
        assert np.unique(p).size == p.size <= 1024 and p[0] == 0 and p.max() < n
        assert p.size == 1024 or n % (kpt * 64) or n < 1024 * kpt
    assert sample_positions(8192).size == 1024 and sample_positions(8192)[-1] == 8191
    # the radix: a hand-made pool
    keys = np.array([0xFF00000000000000, 0x0100000000000005, 0x0100000000000004, 0x0100000000000003, 0x00000000000000FF], dtype=U64)
    r = radix_threshold(keys, 1)
    assert (r.stop, r.shift, r.prefix, len(r.passes)) == ("alone", 56, 0xFF, 1) and r.passes[0][1:4] == (255, 0, 0)
    r = radix_threshold(keys, 3)
    assert (r.stop, r.shift, r.prefix) == ("shift0", 0, 0x0100000000000004) and r.passes[0][1:4] == (1, 63, 2) and reaching(keys, r).size == 3
    r = radix_threshold(keys, 5)
    assert r.passes[0][1:4] == (0, 63, 3) and r.stop == "alone" and reaching(keys, r).size == 5
    rng = np.random.default_rng(3)
    for n, k in ((10, 3), (5000, 17), (40000, 1024)):
        keys = np.unique(rng.integers(0, 1 << 62, size=n, dtype=np.uint64) >> U64(int(rng.integers(0, 40))))
        t = select_trace(keys, k)
        assert np.array_equal(np.sort(t.selected)[::-1], np.sort(keys)[::-1][:k])
    # the keys: order, the two zeros, the round trip
    v = SPECIALS
    k32 = f32_key(v)
    assert (np.diff(k32.astype(np.int64)) <= 0).all() and k32[7] == k32[8] == 0x80000000 and (np.diff(k32.astype(np.int64)) == 0).sum() == 1
    assert np.array_equal(key_f32_bits(k32), (v + np.float32(0)).view(np.uint32))
    assert k32[0] == 0xFF800000 and k32[-1] == 0x007FFFFF


def test_mirror_rrf_on_known_shapes():
    assert int(rrf_hash(np.uint32(0))) == 0 and int(rrf_hash(np.uint32(0xFFFFFFFF))) == ((1 << 32) - RRF_MULT) >> 20
    assert int(rrf_hash(np.uint32(1))) == RRF_MULT >> 20
    a = ids_hashing_to(4094, 5)
    t = rrf_trace(a, np.concatenate([a[:2], ids_hashing_to(4094, 1, skip=5), ids_hashing_to(4095, 1)]))
    assert t.clusters == ((4094, 5),) and t.wraps and t.miss_walk == 5 and (t.m, t.P) == (7, 8)
    assert np.flatnonzero(t.occupied).tolist() == [0, 1, 2, 4094, 4095]
    bits, docs, m = ref_rrf([5, 9], [9, 7], 4)
    f = np.float32
    want = [(f(1) / f(62) + f(1) / f(61), 9), (f(1) / f(61), 5), (f(1) / f(62), 7)]
    assert m == 3 and docs.tolist() == [9, 5, 7] and bits.tolist() == [int(np.float32(s).view(np.uint32)) for s, _ in want]


# ==================================================================== GPU tests
@pytest.fixture(scope="module")
def ctx():
    import openintel_amd as oi
    c = oi.HipContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def O():
    from oracle import lib
    return lib


def _to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def _to_host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _check_merge(call: Call, so, do, co, O, tag, bad):
    S, B, depth = call.scores.shape
    has_neg_zero = (call.scores.view(np.uint32) == 0x80000000).any()
    for b in range(B):
        bits, docs = ref_merge(call.scores[:, b], call.docs[:, b], call.counts[:, b], depth)
        if not has_neg_zero:                      # the numpy reference itself, pinned to the project's oracle
            c = np.minimum(call.counts[:, b], depth)
            ms, md = O.merge_ranked([call.scores[s, b, :c[s]] for s in range(S)], [call.docs[s, b, :c[s]] for s in range(S)], depth)
            assert np.array_equal(md, docs) and np.array_equal(ms.view(np.uint32), bits), tag + (b, "numpy reference != C oracle")
        m = int(co[b])
        if m != docs.size:
            bad.append(tag + (b, "count %d, reference %d" % (m, docs.size)))
        elif not np.array_equal(do[b, :m], docs):
            i = int(np.flatnonzero(do[b, :m] != docs)[0])
            bad.append(tag + (b, "doc ids differ from rank %d: %d, reference %d" % (i, do[b, i], docs[i])))
        elif not np.array_equal(so[b, :m].view(np.uint32), bits):
            i = int(np.flatnonzero(so[b, :m].view(np.uint32) != bits)[0])
            bad.append(tag + (b, "score bits differ from rank %d: %08x, reference %08x" % (i, so[b, i:i + 1].view(np.uint32)[0], bits[i])))


def _merge(ctx, call: Call, device):
    from openintel_amd import merge_lists
    if not device:
        return merge_lists(ctx, call.scores, call.docs, call.counts)
    import torch
    args = [_to_dev(call.scores), _to_dev(call.docs), _to_dev(call.counts)]
    torch.cuda.synchronize()
    so, do, co = merge_lists(ctx, *args)
    ctx.synchronize()
    return _to_host(so, np.float32), _to_host(do, np.uint32), _to_host(co, np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r.name for r in MERGE_ROWS])
def test_merge_row_bit_exact(ctx, O, name):
    """merge_lists from host arrays: counts, doc ids and score bits of every query of the row equal the reference's."""
    call, bad = merge_call(name), []
    _check_merge(call, *_merge(ctx, call, False), O, (name, "host"), bad)
    assert not bad, "%d mismatches, the first: %r" % (len(bad), bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r.name for r in MERGE_ROWS if r.device])
def test_merge_row_bit_exact_from_device_tensors(ctx, O, name):
    call, bad = merge_call(name), []
    _check_merge(call, *_merge(ctx, call, True), O, (name, "device"), bad)
    assert not bad, "%d mismatches, the first: %r" % (len(bad), bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True])
def test_merge_large_call_then_small_call(O, device):
    """The grow-only pool buffer of a context: after a call of 32769-key pools, a small call's pools lie over their keys."""
    import openintel_amd as oi
    c = oi.HipContext(0)
    rng = np.random.default_rng(120)
    large = call_of([rand_query(32769, 33, 1024, rng, "straddle"), rand_query(30000, 33, 1024, rng, "straddle")], 1024)
    small = [call_of([rand_query(n, S, d, rng) for n in ns], d) for S, d, ns in ((2, 5, (7, 0, 3)), (40, 30, (1100, 35)), (33, 1024, (9, 4100)))]
    bad = []
    _check_merge(large, *_merge(c, large, device), O, ("large",), bad)
    for i, call in enumerate(small):
        _check_merge(call, *_merge(c, call, device), O, ("small", i), bad)
    c.close()
    assert not bad, "%d mismatches, the first: %r" % (len(bad), bad[:8])


def _check_rrf(call, k, R, O, tag, bad):
    da = call[0]
    sc, dc, cn = R
    for b in range(da.shape[0]):
        a, bb = rrf_lists(call, b)
        bits, docs, _ = ref_rrf(a, bb, k)
        fs, fd = O.rrf_fuse(a, bb, k)
        assert np.array_equal(fd, docs) and np.array_equal(fs.view(np.uint32), bits), tag + (b, "numpy reference != C oracle")
        m = int(cn[b])
        if m != docs.size:
            bad.append(tag + (b, "count %d, reference %d" % (m, docs.size)))
        elif not np.array_equal(dc[b, :m], docs):
            i = int(np.flatnonzero(dc[b, :m] != docs)[0])
            bad.append(tag + (b, "doc ids differ from rank %d: %d, reference %d" % (i, dc[b, i], docs[i])))
        elif not np.array_equal(sc[b, :m].view(np.uint32), bits):
            bad.append(tag + (b, "score bits differ"))


def _rrf(ctx, call, k, device):
    from openintel_amd import rrf_fuse
    if not device:
        R = rrf_fuse(ctx, *call, k)
        return R.scores, R.docs, R.counts
    import torch
    args = [_to_dev(x) for x in call]
    torch.cuda.synchronize()
    R = rrf_fuse(ctx, *args, k)
    ctx.synchronize()
    return _to_host(R.scores, np.float32), _to_host(R.docs, np.uint32), _to_host(R.counts, np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", [r.name for r in RRF_ROWS])
def test_rrf_row_bit_exact(ctx, O, name, device):
    row, call, bad = RRF_BY_NAME[name], rrf_call(name), []
    for k in rrf_ks(row, call):
        _check_rrf(call, k, _rrf(ctx, call, k, device), O, (name, k), bad)
    assert not bad, "%d mismatches, the first: %r" % (len(bad), bad[:8])


def _check_packed(cos, bm, k, got, tag, bad):
    sc, dc, cn = got
    for b, (bits, docs) in enumerate(ref_packed(cos, bm, k)):
        m = int(cn[b])
        if m != docs.size:
            bad.append(tag + (b, "count %d, reference %d" % (m, docs.size)))
        elif not np.array_equal(dc[b, :m], docs):
            i = int(np.flatnonzero(dc[b, :m] != docs)[0])
            bad.append(tag + (b, "doc ids differ from rank %d: %d, reference %d" % (i, dc[b, i], docs[i])))
        elif not np.array_equal(sc[b, :m].view(np.uint32), bits):
            bad.append(tag + (b, "score bits differ"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [r.name for r in PACKED_ROWS])
def test_fuse_packed_row_bit_exact(ctx, name):
    """fuse_packed == rrf_fuse(merge_lists(cosine), merge_lists(BM25)) == the reference, from host and from device buffers."""
    import torch
    from openintel_amd import fuse_packed, merge_lists, rrf_fuse
    row = PACKED_BY_NAME[name]
    cos, bm = packed_lists(row)
    flat, bad = pack(cos, bm), []
    assert flat.size == row.S * (4 * 3 * row.depth + 6)
    _, cd, cc = merge_lists(ctx, cos.scores, cos.docs, cos.counts)
    _, bd, bc = merge_lists(ctx, bm.scores, bm.docs, bm.counts)
    for k in row.ks:
        F = fuse_packed(ctx, flat, row.S, 3, row.depth, k)
        _check_packed(cos, bm, k, (F.scores, F.docs, F.counts), (name, k, "host"), bad)
        two = rrf_fuse(ctx, cd, cc, bd, bc, k)
        for f in ("scores", "docs", "counts"):
            x, y = getattr(F, f).view(np.uint32), getattr(two, f).view(np.uint32)
            if f != "counts":
                keep = np.arange(k)[None, :] < F.counts[:, None]
                x, y = x[keep], y[keep]
            if not np.array_equal(x, y):
                bad.append((name, k, f + " differ from rrf_fuse(merge_lists, merge_lists)"))
        d_flat = _to_dev(flat)
        torch.cuda.synchronize()
        D = fuse_packed(ctx, d_flat, row.S, 3, row.depth, k)
        ctx.synchronize()
        _check_packed(cos, bm, k, (_to_host(D.scores, np.float32), _to_host(D.docs, np.uint32), _to_host(D.counts, np.uint32)), (name, k, "device"), bad)
    assert not bad, "%d mismatches, the first: %r" % (len(bad), bad[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("replay", [False, True], ids=["eager", "graph-replay"])
def test_fuse_packed_device_calls_follow_the_buffer_contents(replay):
    """The same device tensors, rewritten between calls: every result follows the contents.  With graph replay on, the third
    call on is a replay of a graph captured under the same pointers."""
    import torch
    import openintel_amd as oi
    dev = torch.device("cuda:0")
    c = oi.HipContext(0)
    if replay:
        c.set_stream(torch.cuda.Stream(device=dev))
        c.set_graph_replay(True)
    row, k, bad = PACKED_BY_NAME["packed-S2"], 50, []
    first = pack(*packed_lists(row))
    d_flat = torch.zeros(first.size, dtype=torch.int32, device=dev)
    out = oi.SearchResult(torch.zeros((3, k), dtype=torch.float32, device=dev), torch.zeros((3, k), dtype=torch.int32, device=dev),
                          torch.zeros(3, dtype=torch.int32, device=dev))
    for it in range(5):
        cos, bm = packed_lists(row, seed=it)
        d_flat.copy_(_to_dev(pack(cos, bm)))
        out.scores.zero_(); out.docs.zero_(); out.counts.zero_()
        torch.cuda.synchronize()
        oi.fuse_packed(c, d_flat, row.S, 3, row.depth, k, out=out)
        c.synchronize()
        _check_packed(cos, bm, k, (_to_host(out.scores, np.float32), _to_host(out.docs, np.uint32), _to_host(out.counts, np.uint32)), ("call", it), bad)
    replays = c.graph_stats()[0]
    c.close()
    assert not bad, "%d mismatches, the first: %r" % (len(bad), bad[:8])
    assert (replays >= 2) if replay else (replays == 0)


@pytest.mark.gpu
def test_out_of_range_arguments_are_refused_before_any_launch(ctx):
    """n_shards, depth and k outside the ABI's ranges: the host-side check returns an error; the context still works."""
    from openintel_amd import _lib, fuse_packed, merge_lists, rrf_fuse
    z = lambda *shape: np.zeros(shape, np.uint32)
    with pytest.raises(_lib.OiError):
        merge_lists(ctx, np.zeros((MAX_SHARDS + 1, 1, 1), np.float32), z(MAX_SHARDS + 1, 1, 1), z(MAX_SHARDS + 1, 1))
    with pytest.raises(_lib.OiError):
        merge_lists(ctx, np.zeros((1, 1, OI_MAX_DEPTH + 1), np.float32), z(1, 1, OI_MAX_DEPTH + 1), z(1, 1))
    for depth, k in ((OI_MAX_DEPTH + 1, 1), (4, 0), (4, OI_MAX_DEPTH + 1)):
        with pytest.raises(_lib.OiError):
            rrf_fuse(ctx, z(1, depth), z(1), z(1, depth), z(1), k)
    for S, depth, k in ((0, 4, 4), (MAX_SHARDS + 1, 4, 4), (1, OI_MAX_DEPTH + 1, 4), (1, 4, 0), (1, 4, OI_MAX_DEPTH + 1)):
        with pytest.raises(_lib.OiError):
            fuse_packed(ctx, z(max(S, 1) * (4 * depth + 2)), S, 1, depth, k)
    so, do, co = merge_lists(ctx, np.float32([[[2.0, 1.0]]]), np.uint32([[[5, 6]]]), np.uint32([[2]]))
    assert co[0] == 2 and do[0].tolist() == [5, 6] and so[0].tolist() == [2.0, 1.0]
