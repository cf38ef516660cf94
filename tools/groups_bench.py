"""Similarity leaderboard at the flagship size (10M x 768 i.i.d. unit rows, B = 64, 8192 keys with Zipf-distributed group ids):
ms per call of oi_similar_groups ranked with top = 100 at t in {0.5, 0.2, 0.1}, ALTERNATED with oi_similar_summary with one
bucket and the same filters on the same index in one process, with rotating query batches as in bench.py.  The yardstick is
the summary call itself (the parent's code): both stream the same bytes, and a filtered summary stream already loads the
attribute the key is read from.  Per threshold: the two calls' mean, min and max over the alternated repeats (the summary's
own spread is the bar a difference has to clear), the route taken, the undecided pairs, the event times per profile tag of
one profiled call each ("groups" is the stream; "groups_rank" the rank keys and the ranking), the bytes of cells the call
zeroes, the keys that qualified, and whether the dense records summed over the keys equal the summary's record.  Prints one
JSON line (kept as profiles/groups_bench.json).

    python tools/groups_bench.py [--docs N] [--keys 8192] [--top 100] [--steps K] [--warmup W] [--thresholds 0.5,0.2,0.1]
                                 [--zipf 1.1] [--nonzero 0.03] [--no-filters]

Signals as in tools/summary_bench.py: a share --nonzero of the posts has polarity +1 or -1, half each, the rest 0; 30 %
speculative; sources a coin flip.  Group ids: key k with probability ~ 1 / (k + 1)^zipf, in bits 8..23 of the group word
(the low byte holds source bits, as the header's example has it).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_STREAM_TBPS = 7.0   # the copy screen's measured rate
KEY_SHIFT = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--keys", type=int, default=8192)
    ap.add_argument("--top", type=int, default=100)
    ap.add_argument("--zipf", type=float, default=1.1)
    ap.add_argument("--thresholds", default="0.5,0.2,0.1")
    ap.add_argument("--nonzero", type=float, default=0.03, help="share of posts with a non-zero polarity")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--query-batches", type=int, default=8)
    ap.add_argument("--no-filters", action="store_true", help="no filters on either call (the summary stream then loads no attribute)")
    args = ap.parse_args()

    import torch
    import openintel_amd as oi
    from openintel_amd import synth
    from openintel_amd.analyzer import COUNTERS_DTYPE

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = oi.HipContext(0)
    ctx.use_torch_current_stream()
    n, nk = args.docs, args.keys
    rows = synth.embeddings_torch(n, args.dim, dev, seed=synth.SEED_EMB)
    idx = oi.HybridIndex(ctx, n, args.dim, synth.VOCAB)
    idx.set_embeddings(rows, normalize=False)
    terms, offs = synth.forward_index_torch(n, dev, seed=synth.SEED_TEXT)   # (finalize, which makes the screening copy, wants one)
    idx.set_forward(terms, offs)
    del terms, offs
    g = torch.Generator(device=dev)
    g.manual_seed(20261)
    p = 1.0 / torch.arange(1, nk + 1, device=dev, dtype=torch.float64) ** args.zipf
    cdf = torch.cumsum(p / p.sum(), 0)
    key = torch.searchsorted(cdf, torch.rand(n, device=dev, generator=g, dtype=torch.float64)).clamp_(max=nk - 1)
    top_key_share = float((key == 0).double().mean().item())
    group = ((key << KEY_SHIFT) | torch.randint(0, 256, (n,), device=dev, generator=g)).to(torch.int32)
    idx.set_doc_attrs(group, None)
    u = torch.rand(n, device=dev, generator=g)
    pol = torch.where(u < args.nonzero / 2, 1.0, torch.where(u < args.nonzero, -1.0, 0.0)).to(torch.float64)
    spec = (torch.rand(n, device=dev, generator=g) < 0.3).to(torch.uint8)
    src = (torch.rand(n, device=dev, generator=g) < 0.5).to(torch.uint8)
    nonzero_share = float((pol != 0).double().mean().item())
    idx.set_signals(pol, spec, src, 0.2)
    del u, pol, spec, src, key, group, cdf, p
    idx.finalize()                       # (the bf16 screening copy: the stream route)
    torch.cuda.empty_cache()
    batches = [synth.query_batch_torch(args.batch, args.dim, dev, seed=synth.SEED_QUERY + 7919 * i)[0]
               for i in range(args.query_batches)]
    ths = [float(t) for t in args.thresholds.split(",") if t]
    filters = None                       # or: everything passes, resident like the queries
    if not args.no_filters:
        filters = torch.from_numpy(np.tile(np.array([[0, 0, 0, 0xFFFFFFFF]], np.uint32), (args.batch, 1)).view(np.int32)).to(dev)
    mask = ((1 << max(1, (nk - 1).bit_length())) - 1) << KEY_SHIFT
    calls = {"groups": lambda q, t: idx.similar_groups(q, t, mask, nk, top=args.top, rank_by="total", filters=filters),
             "summary": lambda q, t: idx.similar_summary(q, t, filters=filters)}
    tags = {"groups": ("groups", "groups_band", "groups_exact", "groups_rank"), "summary": ("summary", "summary_band", "summary_exact")}
    last = {}

    def run(call, t, i):
        last[call, t] = calls[call](batches[i % len(batches)], t)

    for i in range(args.warmup):
        for t in ths:
            for call in calls:
                run(call, t, i)
    torch.cuda.synchronize()
    times = {(call, t): [] for t in ths for call in calls}
    for i in range(args.steps):          # alternating: both calls see the same clocks and the same neighbours
        for t in ths:
            for call in calls:
                t0 = time.perf_counter()
                run(call, t, i)
                torch.cuda.synchronize()
                times[call, t].append((time.perf_counter() - t0) * 1e3)
    res = {}
    for t in ths:
        case = {}
        for call in calls:
            x = np.array(times[call, t])
            case[call] = {"ms_per_call": round(float(x.mean()), 4), "min_ms": round(float(x.min()), 4), "max_ms": round(float(x.max()), 4),
                          "std_ms": round(float(x.std()), 4)}
            ctx.profile_reset(True)      # one more profiled call: the route, the band, the event times
            run(call, t, 0)
            prof = {tag: ctx.profile_read(tag) for tag in tags[call]}
            band, flags = ctx.profile_read(call + "_state")
            ctx.profile_reset(False)
            ran = [tag for tag, (_, launches) in prof.items() if launches > 0]
            case[call].update(route="exact (fallback)" if tags[call][2] in ran else "screen", band_pairs=int(band),
                              band_overflow=bool(int(flags) & 2),
                              event_ms={tag: round(ms, 4) for tag, (ms, launches) in prof.items() if launches > 0})
        rk = last["groups", t]
        one = last["summary", t].cpu().numpy().view(COUNTERS_DTYPE).reshape(args.batch, 1)
        dense = idx.similar_groups(batches[0], t, mask, nk, filters=filters)     # (the profiled calls above ran batch 0)
        dense = dense.cpu().numpy().view(COUNTERS_DTYPE).reshape(args.batch, nk)
        sums_equal = all(np.array_equal(dense[f].sum(axis=1), one[f][:, 0])
                         for f in ("total", "by_source", "bullish", "bearish", "neutral", "spec_count", "polarity_sum"))
        lo, hi = case["summary"]["min_ms"], case["summary"]["max_ms"]
        case.update(hits=int(one["total"].sum()), keys_qualified_mean=round(float(rk.qualified.cpu().numpy().view(np.uint32).mean()), 1),
                    keys_listed_mean=round(float(rk.counts.cpu().numpy().view(np.uint32).mean()), 1),
                    dense_sums_equal_summary=bool(sums_equal),
                    groups_minus_summary_ms=round(case["groups"]["ms_per_call"] - case["summary"]["ms_per_call"], 4),
                    groups_stream_event_inside_summary_call_spread=bool(case["groups"]["event_ms"].get("groups", 0.0) <= hi),
                    summary_call_spread_ms=[lo, hi])
        res["t=%g" % t] = case
    floor_ms = 2.0 * n * args.dim / (COPY_STREAM_TBPS * 1e12) * 1e3
    print(json.dumps({"tool": "groups_bench", "docs": n, "dim": args.dim, "batch": args.batch, "keys": nk, "top": args.top,
                      "zipf": args.zipf, "top_key_share": round(top_key_share, 5), "filters": not args.no_filters,
                      "steps": args.steps, "warmup": args.warmup, "nonzero_polarity_share": round(nonzero_share, 5),
                      "cells_zeroed_bytes_per_call": 64 * args.batch * nk, "rank_keys_bytes": 8 * args.batch * nk,
                      "stream_floor_ms": round(floor_ms, 3), "cases": res}))


if __name__ == "__main__":
    main()
