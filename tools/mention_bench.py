#!/usr/bin/env python3
"""Mention summary at the flagship size: the synth.py corpus text at 10M documents, B = 64 queries of 4 terms
(synth.query_batch_torch), 24 hourly buckets.  oi_mention_summary with ANY and with ALL ALTERNATES in one process with
oi_search_lists over the same terms, whose BM25 leg (bm25_stream_kernel and its plan, profile tag "bm25") reads the same
posting runs and is the yardstick: per repeat one profiled call of each, so the three see the same clocks and neighbours.

    python tools/mention_bench.py [--docs N] [--repeats R] [--batch B] [--buckets K]

Prints one JSON line (kept as profiles/mention_bench.json): per call the mean / min / max of the kernel's event time over the
repeats, the postings read (the df of every distinct query term), the matches tallied (the sum of the records' totals), and
for the BM25 leg its max - min, the spread a difference has to clear.  With OI_LIB=ablation and OI_MENTION_ABLATE=1 (no tally)
or 2 (no LDS adds) the same run times a -DOI_ABLATION build's variants of the match kernel (results wrong by construction).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(x):
    x = np.array(x)
    return {"mean_ms": round(float(x.mean()), 4), "min_ms": round(float(x.min()), 4), "max_ms": round(float(x.max()), 4),
            "max_minus_min_ms": round(float(x.max() - x.min()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--buckets", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch
    import openintel_amd as oi
    import _ablation  # noqa: F401  (OI_LIB=ablation: tools only)
    from openintel_amd import synth
    from openintel_amd.analyzer import COUNTERS_DTYPE

    DIM, DEPTH = 32, 1000                 # a narrow embedding keeps the cosine leg of oi_search_lists out of the way
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = oi.HipContext(0)
    ctx.use_torch_current_stream()
    ctx.set_overlap(False)                # the BM25 kernels alone, not beside the cosine leg
    n, B = args.docs, args.batch
    idx = oi.HybridIndex(ctx, n, DIM, synth.VOCAB)
    idx.set_embeddings(synth.embeddings_torch(n, DIM, dev), normalize=False)
    terms, offs = synth.forward_index_torch(n, dev)
    idx.set_forward(terms, offs)
    del terms, offs
    idx.set_max_query_terms(4)
    width = 3600                          # a day of posts in row order: 24 hourly buckets
    idx.set_doc_attrs(None, (torch.arange(n, device=dev, dtype=torch.int64) * (args.buckets * width) // n).to(torch.int32))
    g = torch.Generator(device=dev)
    g.manual_seed(20260)
    u = torch.rand(n, device=dev, generator=g)
    pol = torch.where(u < 0.015, 1.0, torch.where(u < 0.03, -1.0, 0.0)).to(torch.float64)     # 3 % of the posts hit the lexicon
    idx.set_signals(pol, (torch.rand(n, device=dev, generator=g) < 0.3).to(torch.uint8),
                    (torch.rand(n, device=dev, generator=g) < 0.5).to(torch.uint8), 0.2)
    del u, pol
    idx.finalize()
    torch.cuda.empty_cache()
    qv, qt, qo = synth.query_batch_torch(B, DIM, dev)
    kw = dict(n_buckets=args.buckets, stamp_origin=0, bucket_width=width)
    calls = {"mention_any": lambda: idx.mention_summary(qt, qo, min_match=None, **kw),
             "mention_all": lambda: idx.mention_summary(qt, qo, min_match="all", **kw),
             "search_lists": lambda: idx.search_lists(qv, qt, qo, depth=DEPTH)}
    tags = {"mention_any": ("mention", "mention_plan"), "mention_all": ("mention", "mention_plan"), "search_lists": ("bm25",)}
    last = {}
    for _ in range(args.warmup):
        for name, call in calls.items():
            last[name] = call()
    torch.cuda.synchronize()
    times = {(name, tag): [] for name in calls for tag in tags[name]}
    for _ in range(args.repeats):         # alternating, one profiled call each
        for name, call in calls.items():
            ctx.profile_reset(True)
            last[name] = call()
            torch.cuda.synchronize()
            for tag in tags[name]:
                times[name, tag].append(ctx.profile_read(tag)[0])
            ctx.profile_reset(False)
    df = idx.local_stats()[1].astype(np.int64)
    qt_h, qo_h = qt.cpu().numpy().view(np.uint32), qo.cpu().numpy().view(np.uint32)
    postings = int(sum(df[np.unique(qt_h[qo_h[q]:qo_h[q + 1]])].sum() for q in range(B)))
    res = {"tool": "mention_bench", "docs": n, "batch": B, "buckets": args.buckets, "repeats": args.repeats,
           "lib": os.environ.get("OI_LIB", "product"), "ablate": int(os.environ.get("OI_MENTION_ABLATE", "0") or 0),
           "terms_per_query": float(qt_h.size) / B, "postings_read": postings, "posting_bytes": 8 * postings,
           "tasks": B * ((n + 32767) // 32768)}
    for name in ("mention_any", "mention_all"):
        rec = last[name].cpu().numpy().view(COUNTERS_DTYPE).reshape(B, args.buckets)
        res[name] = {"kernel": stats(times[name, "mention"]), "plan": stats(times[name, "mention_plan"]),
                     "matches_tallied": int(rec["total"].sum())}
    res["bm25"] = stats(times["search_lists", "bm25"])
    for name in ("mention_any", "mention_all"):
        d = res[name]["kernel"]["mean_ms"] - res["bm25"]["mean_ms"]
        res[name]["minus_bm25_ms"] = round(d, 4)
        res[name]["slower_than_bm25_by_more_than_its_spread"] = bool(d > res["bm25"]["max_minus_min_ms"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
