"""Filtered hybrid search at the flagship size (10M x 768, B = 64, depth 1000, k 100): ms per step of the unfiltered search
(with and without speculative screen thresholds -- a filtered search never speculates), an all-pass filter, random groups
of selectivity 1/2, 1/100 and 1/10 000, a clustered 1/100 (the passing posts are contiguous rows, like one ticker's posts
stored together) and a stamp window over the newest 5 % of rows -- all in one
process on one index, with the same rotating query batches as bench.py.  Prints one JSON line.

    python tools/filter_bench.py [--docs N] [--steps K] [--warmup W] [--only CASE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL = (0, 0, 0, 0xFFFFFFFF)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--depth", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--vocab", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--query-batches", type=int, default=8)
    ap.add_argument("--only", default="", help="comma-separated case names (default: all)")
    ap.add_argument("--no-speculation", action="store_true")
    args = ap.parse_args()

    import torch
    import openintel_amd as oi
    from openintel_amd import synth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = oi.HipContext(0)
    ctx.use_torch_current_stream()
    if args.no_speculation:
        ctx.set_screen_speculation(False)
    n = args.docs
    idx = oi.HybridIndex(ctx, n, args.dim, args.vocab)
    rows = synth.embeddings_torch(n, args.dim, dev, seed=synth.SEED_EMB)
    idx.set_embeddings(rows, normalize=False)
    terms, offs = synth.forward_index_torch(n, dev, vocab=args.vocab, seed=synth.SEED_TEXT)
    idx.set_forward(terms, offs)
    idx.set_max_query_terms(4)
    del terms, offs
    torch.cuda.empty_cache()
    # group: bit 0 = a random half; bits 8..15 = one of 100 random "tickers"; bits 16..29 = one of 10 000; bit 30 = the
    # clustered 1/100 (rows [n/2, n/2 + n/100)).  stamp: the row number (rows are stored oldest first).
    rng = np.random.default_rng(12345)
    group = (rng.integers(0, 2, n, dtype=np.uint32) | (rng.integers(0, 100, n, dtype=np.uint32) << 8)
             | (rng.integers(0, 10_000, n, dtype=np.uint32) << 16))
    group[n // 2: n // 2 + n // 100] |= np.uint32(1 << 30)
    stamp = np.arange(n, dtype=np.uint32)
    idx.set_doc_attrs(group, stamp)
    del group, stamp
    idx.finalize()
    batches = [synth.query_batch_torch(args.batch, args.dim, dev, vocab=args.vocab, seed=synth.SEED_QUERY + 7919 * i)
               for i in range(args.query_batches)]

    def filt(row):
        return torch.tensor(np.tile(np.array(row, np.uint32), (args.batch, 1)).view(np.int32), device=dev)

    cases = {
        "unfiltered": None,
        "unfiltered_no_speculation": None,
        "all_pass": filt(ALL),
        "random_1_2": filt((0x1, 1, 0, 0xFFFFFFFF)),
        "random_1_100": filt((0xFF << 8, 42 << 8, 0, 0xFFFFFFFF)),
        "random_1_10000": filt((0x3FFF << 16, 4321 << 16, 0, 0xFFFFFFFF)),
        "clustered_1_100": filt((1 << 30, 1 << 30, 0, 0xFFFFFFFF)),
        "newest_5pct": filt((0, 0, n - n // 20, 0xFFFFFFFF)),
    }
    only = [c for c in args.only.split(",") if c]
    out = oi.SearchResult(torch.zeros((args.batch, args.k), dtype=torch.float32, device=dev),
                          torch.zeros((args.batch, args.k), dtype=torch.int32, device=dev),
                          torch.zeros((args.batch,), dtype=torch.int32, device=dev))
    res = {}
    for name, F in cases.items():
        if only and name not in only:
            continue
        ctx.set_screen_speculation(not args.no_speculation and name != "unfiltered_no_speculation")

        def step(i):
            qv, qt, qo = batches[i % len(batches)]
            idx.search(qv, qt, qo, k=args.k, depth=args.depth, out=out, filters=F)

        for i in range(args.warmup):
            step(i)
        ctx.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            step(i)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / args.steps
        res[name] = {"ms_per_step": round(ms, 4), "mean_count": float(out.counts.float().mean().item())}
    print(json.dumps({"tool": "filter_bench", "docs": n, "dim": args.dim, "batch": args.batch, "depth": args.depth,
                      "k": args.k, "steps": args.steps, "warmup": args.warmup, "speculation": not args.no_speculation,
                      "cases": res}))


if __name__ == "__main__":
    main()
