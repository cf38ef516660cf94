"""The search family's entry points (api.hip: oi_search_lists[_filtered], oi_search[_filtered], oi_search_collapsed,
oi_search_lists_packed[_filtered], oi_fuse_packed, oi_search_sharded[_filtered], oi_rrf_fuse, oi_merge_lists) share one call
frame, one view of the two list layouts, one result block and one graph-key builder.  Three things tie them together:
  * agreement -- every entry point gives the same bits for host arrays and device tensors, oi_search equals oi_rrf_fuse over
    oi_search_lists and oi_fuse_packed over one shard of oi_search_lists_packed, an all-pass filter changes nothing: the lists
    block, the packed layout and the result block describe the same data;
  * check order -- a call with two faults reports the one its checks reach first (the table below is copied from the source of
    the commit before the shared call frame, not from the code under test);
  * graph keys -- a captured call is replayed only while everything its key names is unchanged.
One index of 40 000 x 384 rows; B = 16 (the batch route) and B = 1; depth 64, k 10, pool 32."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, DIM, VOCAB, DEPTH, K, POOL, THR = 40_000, 384, 400, 64, 10, 32, 0.9
N_DUP = 2_000                     # the last N_DUP rows repeat the first N_DUP: near-duplicates for the collapse
ALL_PASS = (0, 0, 0, 0xFFFFFFFF)
MAX_DEPTH = 1024                  # OI_MAX_DEPTH


class Env:
    pass


@pytest.fixture(scope="module")
def env():
    import torch
    import openintel_amd as oi
    e = Env()
    e.dev = torch.device("cuda:0")
    rng = np.random.default_rng(41)
    rows = rng.standard_normal((N, DIM)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows[N - N_DUP:] = rows[:N_DUP]
    lens = rng.integers(1, 12, size=N)
    offs = np.zeros(N + 1, np.uint64)
    offs[1:] = np.cumsum(lens)
    terms = rng.integers(0, VOCAB, size=int(offs[-1])).astype(np.uint32)
    e.rows = rows
    e.ctx = oi.HipContext(0)
    e.idx = oi.HybridIndex(e.ctx, N, DIM, VOCAB, doc_id_base=100)
    e.idx.set_embeddings(torch.from_numpy(rows).to(e.dev), normalize=False)
    e.idx.set_forward(terms, offs)
    e.idx.set_doc_attrs(group=rng.integers(0, 16, size=N).astype(np.uint32), stamp=np.arange(N, dtype=np.uint32))
    e.idx.finalize()
    # a small index WITHOUT doc attributes: a filtered call on it fails the state check, the last one of every call
    e.bare = oi.HybridIndex(e.ctx, 512, DIM, VOCAB)
    e.bare.set_embeddings(rows[:512].copy(), normalize=False)
    e.bare.set_forward(terms[:int(offs[512])], offs[:513])
    e.bare.finalize()
    yield e
    e.bare.close(); e.idx.close(); e.ctx.close()


def batch(e, B, seed=5):
    """Queries next to duplicated rows (both copies rank at the top of the cosine list), a few terms each; host and device."""
    import torch
    rng = np.random.default_rng(seed + B)
    q = e.rows[rng.integers(0, N_DUP, size=B)] + 0.02 * rng.standard_normal((B, DIM)).astype(np.float32)
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    qo = np.zeros(B + 1, np.uint32)
    qo[1:] = np.cumsum(rng.integers(1, 5, size=B))
    qt = rng.integers(0, VOCAB, size=int(qo[-1])).astype(np.uint32)
    f = np.tile(np.array(ALL_PASS, np.uint32), (B, 1))
    host = (q, qt, qo)
    devq = tuple(torch.from_numpy(x.view(np.int32) if x.dtype == np.uint32 else x).to(e.dev) for x in host)
    torch.cuda.synchronize()
    return host, devq, f, torch.from_numpy(f.view(np.int32)).to(e.dev)


def bits(x):
    """host bytes of a numpy array or a tensor, as uint32"""
    a = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    return np.ascontiguousarray(a).view(np.uint32)


def same_rows(got, want, counts, what):
    """[B, width] arrays equal bit for bit over each row's valid prefix"""
    g, w, c = bits(got), bits(want), bits(counts).reshape(-1)
    for b in range(c.size):
        assert np.array_equal(g[b, :c[b]], w[b, :c[b]]), (what, b)


def same_lists(a, b, what):
    assert np.array_equal(bits(a.cos_counts), bits(b.cos_counts)) and np.array_equal(bits(a.bm25_counts), bits(b.bm25_counts)), what
    same_rows(a.cos_scores, b.cos_scores, a.cos_counts, what + " cos scores")
    same_rows(a.cos_docs, b.cos_docs, a.cos_counts, what + " cos docs")
    same_rows(a.bm25_scores, b.bm25_scores, a.bm25_counts, what + " bm25 scores")
    same_rows(a.bm25_docs, b.bm25_docs, a.bm25_counts, what + " bm25 docs")


def same_result(a, b, what):
    assert np.array_equal(bits(a.counts), bits(b.counts)), what
    same_rows(a.scores, b.scores, a.counts, what + " scores")
    same_rows(a.docs, b.docs, a.counts, what + " docs")
    if hasattr(a, "dup_counts") and hasattr(b, "dup_counts"):
        same_rows(a.dup_counts, b.dup_counts, a.counts, what + " dup counts")


@pytest.mark.parametrize("B", [16, 1])
def test_entry_points_agree_across_locations_layouts_and_an_all_pass_filter(env, B):
    import openintel_amd as oi
    e, ix, ctx = env, env.idx, env.ctx
    host, devq, f_h, f_d = batch(e, B)

    def both(call):          # the call with host arrays and with device tensors
        h, d = call(host, f_h), call(devq, f_d)
        ctx.synchronize()
        return h, d

    lists_h, lists_d = both(lambda q, f: ix.search_lists(*q, depth=DEPTH))
    same_lists(lists_d, lists_h, "search_lists device / host")
    assert int(bits(lists_h.cos_counts).min()) == DEPTH and int(bits(lists_h.bm25_counts).min()) > 0
    want, want_d = both(lambda q, f: ix.search(*q, k=K, depth=DEPTH))
    same_result(want_d, want, "search device / host")
    assert int(bits(want.counts).min()) == K and int(bits(want.docs).min()) >= 100

    # the lists block and the result block: RRF over the lists is the search
    for lists, name in ((lists_h, "host"), (lists_d, "device")):
        fused = oi.rrf_fuse(ctx, lists.cos_docs, lists.cos_counts, lists.bm25_docs, lists.bm25_counts, K)
        ctx.synchronize()
        same_result(fused, want, "rrf_fuse over search_lists, " + name)
    # the packed layout: the same lists, and fused as one shard the same search
    for packed, name in zip(both(lambda q, f: ix.search_lists_packed(*q, depth=DEPTH)), ("host", "device")):
        same_lists(oi.unpack_lists(packed, B, DEPTH), lists_h, "search_lists_packed, " + name)
        fused = oi.fuse_packed(ctx, packed, 1, B, DEPTH, K)
        ctx.synchronize()
        same_result(fused, want, "fuse_packed over one shard, " + name)
    # one shard merged is that shard's list
    for lists, name in ((lists_h, "host"), (lists_d, "device")):
        so, do, co = oi.merge_lists(ctx, lists.cos_scores[None], lists.cos_docs[None], lists.cos_counts[None])
        ctx.synchronize()
        assert np.array_equal(bits(co), bits(lists_h.cos_counts)), name
        same_rows(so, lists_h.cos_scores, co, "merge_lists scores, " + name)
        same_rows(do, lists_h.cos_docs, co, "merge_lists docs, " + name)
    # the collapse over the fused pool-list, kept on the device or passed by the caller
    col_h, col_d = both(lambda q, f: ix.search_collapsed(*q, k=K, depth=DEPTH, pool=POOL, threshold=THR))
    same_result(col_d, col_h, "search_collapsed device / host")
    assert int(bits(col_h.dup_counts).max()) >= 2         # (a planted duplicate was folded into its better-ranked copy)
    pool_list = ix.search(*host, k=POOL, depth=DEPTH)
    same_result(ix.collapse_lists(pool_list.scores, pool_list.docs, pool_list.counts, THR, K), col_h, "collapse_lists over search(k = pool)")

    # an all-pass filter: the unfiltered bits, through every filtered form
    fl_h, fl_d = both(lambda q, f: ix.search_lists(*q, depth=DEPTH, filters=f))
    same_lists(fl_h, lists_h, "search_lists_filtered host"); same_lists(fl_d, lists_h, "search_lists_filtered device")
    for got, name in zip(both(lambda q, f: ix.search(*q, k=K, depth=DEPTH, filters=f)), ("host", "device")):
        same_result(got, want, "search_filtered, " + name)
    for got, name in zip(both(lambda q, f: ix.search_lists_packed(*q, depth=DEPTH, filters=f)), ("host", "device")):
        same_lists(oi.unpack_lists(got, B, DEPTH), lists_h, "search_lists_packed_filtered, " + name)
    for got, name in zip(both(lambda q, f: ix.search_collapsed(*q, k=K, depth=DEPTH, pool=POOL, threshold=THR, filters=f)), ("host", "device")):
        same_result(got, col_h, "search_collapsed with a filter, " + name)

    # the sharded call over a communicator of one rank: the packed lists, gathered and fused
    comm = oi.NativeComm(ctx, oi.NativeComm.unique_id(), 0, 1)
    try:
        for got, name in zip(both(lambda q, f: ix.search_sharded(comm, *q, k=K, depth=DEPTH)), ("host", "device")):
            same_result(got, want, "search_sharded, " + name)
        for got, name in zip(both(lambda q, f: ix.search_sharded(comm, *q, k=K, depth=DEPTH, filters=f)), ("host", "device")):
            same_result(got, want, "search_sharded_filtered, " + name)
    finally:
        comm.close()


# ---- check order: (entry point, the two faults, return code, oi_last_error) -- the first check the call's code reaches wins.
# Every call: check_search_args (null index, null query buffer, n_queries, depth), the call's own checks, then the state check
# of a filtered search; oi_search_collapsed: its collapse checks (threshold, pool, k, k <= pool, outputs) BEFORE the search checks.
INVALID, STATE = -1, -5
NO_ATTRS = "filtered search: the index has no doc attributes (oi_index_set_doc_attrs)"
CHECK_ORDER = [
    ("lists", "depth = 0 + null output", dict(depth=0, out=False), INVALID, "search: depth=0 outside [1,%u]" % MAX_DEPTH),
    ("lists", "null output + filter without attributes", dict(out=False, filt=True), INVALID, "search_lists: null output buffer"),
    ("lists", "null query buffer + n_queries = 0", dict(qv=False, B=0), INVALID, "search: null query buffer"),
    ("search", "depth = 0 + k = 0", dict(depth=0, k=0), INVALID, "search: depth=0 outside [1,%u]" % MAX_DEPTH),
    ("search", "k = 0 + filter without attributes", dict(k=0, filt=True), INVALID, "search: k=0 outside [1,%u]" % MAX_DEPTH),
    ("search", "k = 0 + null output", dict(k=0, out=False), INVALID, "search: k=0 outside [1,%u]" % MAX_DEPTH),
    ("search", "null output + filter without attributes", dict(out=False, filt=True), INVALID, "search: null output buffer"),
    ("collapsed", "NaN threshold + depth = 0", dict(thr=float("nan"), depth=0), INVALID, "search_collapsed: threshold is NaN"),
    ("collapsed", "pool = 0 + null query buffer", dict(pool=0, qv=False), INVALID, "search_collapsed: depth / pool = 0 outside [1,%u]" % MAX_DEPTH),
    ("collapsed", "k > pool + n_queries = 0", dict(k=POOL + 1, B=0), INVALID, "search_collapsed: k=%u exceeds pool=%u" % (POOL + 1, POOL)),
    ("collapsed", "null output + depth = 0", dict(out=False, depth=0), INVALID, "search_collapsed: null output buffer"),
    ("collapsed", "depth = 0 + filter without attributes", dict(depth=0, filt=True), INVALID, "search: depth=0 outside [1,%u]" % MAX_DEPTH),
    ("packed", "n_queries = 0 + null output", dict(B=0, out=False), INVALID, "search: n_queries=0 outside [1,4096]"),
    ("packed", "null output + filter without attributes", dict(out=False, filt=True), INVALID, "search_lists_packed: null output buffer"),
    ("sharded", "depth = 0 + null communicator", dict(depth=0), INVALID, "search: depth=0 outside [1,%u]" % MAX_DEPTH),
    ("sharded", "null communicator + k = 0", dict(k=0), INVALID, "null communicator"),
    ("sharded", "null communicator + filter without attributes", dict(filt=True), INVALID, "null communicator"),
    # (and the last check alone, for each call that can reach it without a communicator)
    ("lists", "filter without attributes", dict(filt=True), STATE, NO_ATTRS),
    ("search", "filter without attributes", dict(filt=True), STATE, NO_ATTRS),
    ("collapsed", "filter without attributes", dict(filt=True), STATE, NO_ATTRS),
    ("packed", "filter without attributes", dict(filt=True), STATE, NO_ATTRS),
]


@pytest.mark.parametrize("row", CHECK_ORDER, ids=["%s: %s" % r[:2] for r in CHECK_ORDER])
def test_a_call_with_two_faults_reports_the_check_that_comes_first(env, row):
    from openintel_amd import _lib
    entry, _, fault, want_rc, want_msg = row
    lib, B = env.ctx.lib, fault.get("B", 2)
    (q, qt, qo), _, f, _ = batch(env, 2)
    depth, k, pool, thr = fault.get("depth", 8), fault.get("k", 4), fault.get("pool", POOL), fault.get("thr", THR)
    ix = env.bare.handle                                  # no doc attributes: `filt` is a fault here
    qv = _lib.ptr(q) if fault.get("qv", True) else None
    filt = _lib.ptr(f) if fault.get("filt") else None
    keep = [np.zeros(4096, np.uint32) for _ in range(6)]
    o = [_lib.ptr(a) if fault.get("out", True) else None for a in keep]
    H = _lib.OI_HOST
    if entry == "lists":
        rc = lib.oi_search_lists_filtered(ix, qv, _lib.ptr(qt), _lib.ptr(qo), B, depth, filt, H, *o)
    elif entry == "search":
        rc = lib.oi_search_filtered(ix, qv, _lib.ptr(qt), _lib.ptr(qo), B, depth, k, filt, H, *o[:3])
    elif entry == "collapsed":
        rc = lib.oi_search_collapsed(ix, qv, _lib.ptr(qt), _lib.ptr(qo), B, depth, pool, k, C.c_float(thr), filt, H, *o[:4])
    elif entry == "packed":
        rc = lib.oi_search_lists_packed_filtered(ix, qv, _lib.ptr(qt), _lib.ptr(qo), B, depth, filt, H, o[0])
    else:
        rc = lib.oi_search_sharded_filtered(ix, None, qv, _lib.ptr(qt), _lib.ptr(qo), B, depth, k, filt, H, *o[:3])
    assert (rc, lib.oi_last_error().decode()) == (want_rc, want_msg)


def test_a_captured_call_is_replayed_only_while_everything_its_key_names_is_unchanged(env):
    """oi_search, oi_search_filtered, oi_search_collapsed, oi_search_lists_packed, three calls each with the same device buffers:
    eager, captured, replayed.  Then one keyed thing changes at a time -- k, depth, the collapse threshold, set_overlap, the
    filters pointer, one output tensor: the next call is not a replay, and gives the eager context's bits."""
    import torch
    import openintel_amd as oi
    e, B = env, 16
    cg = oi.HipContext(0)
    cg.set_stream(torch.cuda.Stream(device=e.dev))         # replay needs a real stream (not the default one)
    cg.set_graph_replay(True)
    ig = e.idx.view(cg)
    _, (qv, qt, qo), _, filt = batch(e, B)
    zeros = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=e.dev)
    s_buf, d_buf, c_buf, u_buf, p_buf = zeros(B * K, torch.float32), zeros(B * K), zeros(B), zeros(B * K), zeros(oi.packed_words(B, DEPTH))
    c_other, u_other, p_other, filt_other = zeros(B), zeros(B * K).view(B, K), zeros(oi.packed_words(B, DEPTH)), filt.clone()
    torch.cuda.synchronize()                               # (the tensors are filled on torch's stream, the calls run on cg's)

    def result(k=K, counts=c_buf, dup=None):      # views of the SAME storage whatever k is: only what the test changes moves in the key
        return oi.CollapsedResult(s_buf[:B * k].view(B, k), d_buf[:B * k].view(B, k), counts, u_buf[:B * k].view(B, k) if dup is None else dup)

    def search(ix, out, k=K, depth=DEPTH, filters=None):
        return ix.search(qv, qt, qo, k=k, depth=depth, out=out, filters=filters)

    def collapsed(ix, out, thr=THR):
        return ix.search_collapsed(qv, qt, qo, k=K, depth=DEPTH, pool=POOL, threshold=thr, out=out)

    def packed(ix, out):
        return ix.search_lists_packed(qv, qt, qo, depth=DEPTH, out=out)

    kinds = {"search": lambda: search(ig, result()), "search_filtered": lambda: search(ig, result(), filters=filt),
             "search_collapsed": lambda: collapsed(ig, result()), "search_lists_packed": lambda: packed(ig, p_buf)}
    for name, call in kinds.items():
        r0, c0 = cg.graph_stats()
        for _ in range(3):
            call()
        cg.synchronize()
        r1, c1 = cg.graph_stats()
        assert c1 - c0 >= 1 and r1 - r0 >= 1, (name, r1 - r0, c1 - c0)

    def not_a_replay(what, call, eager, compare):
        r0 = cg.graph_stats()[0]
        got = call()
        cg.synchronize()
        assert cg.graph_stats()[0] == r0, what
        want = eager()
        e.ctx.synchronize()
        compare(got, want, what)

    same_packed = lambda a, b, what: same_lists(oi.unpack_lists(a, B, DEPTH), oi.unpack_lists(b, B, DEPTH), what)
    not_a_replay("k", lambda: search(ig, result(K - 1), k=K - 1), lambda: search(e.idx, None, k=K - 1), same_result)
    not_a_replay("depth", lambda: search(ig, result(), depth=DEPTH - 1), lambda: search(e.idx, None, depth=DEPTH - 1), same_result)
    not_a_replay("threshold", lambda: collapsed(ig, result(), thr=0.5), lambda: collapsed(e.idx, None, thr=0.5), same_result)
    cg.set_overlap(False)
    not_a_replay("set_overlap: search", lambda: search(ig, result()), lambda: search(e.idx, None), same_result)
    not_a_replay("set_overlap: packed", lambda: packed(ig, p_buf), lambda: packed(e.idx, None), same_packed)
    cg.set_overlap(True)
    not_a_replay("filters pointer", lambda: search(ig, result(), filters=filt_other), lambda: search(e.idx, None, filters=filt), same_result)
    not_a_replay("counts tensor", lambda: search(ig, result(counts=c_other)), lambda: search(e.idx, None), same_result)
    not_a_replay("dup-counts tensor", lambda: collapsed(ig, result(dup=u_other)), lambda: collapsed(e.idx, None), same_result)
    not_a_replay("packed output", lambda: packed(ig, p_other), lambda: packed(e.idx, None), same_packed)
    # ... and the unchanged calls are replayed again (three rounds: a workspace the eager context grew in between restarts a capture)
    r0 = cg.graph_stats()[0]
    for _ in range(3):
        for call in kinds.values():
            call()
    cg.synchronize()
    assert cg.graph_stats()[0] >= r0 + len(kinds)
    ig.close(); cg.close()
