#!/usr/bin/env python3
"""Narrative breakdown at the flagship size: the synth.py corpus (10M x 768 i.i.d. unit rows) with attributes and signals,
labelled by oi_similar_share at t = 0 with 8 and with 256 query vectors (the exemplar bench's setup).  Per labelling three runs of
oi_label_summary, device location, one profiled call per repeat, event ms per profile tag ("label_summary": the pass;
"label_summary_rank": the ranked finish):

    time        TIME axis, 24 buckets
    key_dense   KEY axis, 4096 keys, dense
    key_ranked  KEY axis, 4096 keys, top = 10

and next to the times the rate over the algorithmic bytes: 4 B of label per row, 8 B of attributes and 8 B of signals per
labelled row.  The gate: in the same session, ALTERNATED with the `time` run, the only route a host had for the timeline before
this call -- oi_similar_share with the same vectors and the same 24-bucket axis (torch event ms around the call).  The new call, also as
event ms around the whole call ("call_event": the memset of the cells and the finish are under no profile tag), must be below it
in every run against every run ("time_below_share_every_run").

    python tools/label_summary_bench.py [--docs N] [--dim 768] [--clusters 8,256] [--repeats R]

Prints one JSON line (kept as profiles/label_summary_bench.json).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAGS = ("label_summary", "label_summary_rank")
N_BUCKETS, BUCKET_WIDTH, N_KEYS, KEY_MASK, TOP = 24, 3600, 4096, 0xFFF, 10


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return {"mean_ms": round(float(x.mean()), 4), "min_ms": round(float(x.min()), 4), "max_ms": round(float(x.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--clusters", default="8,256")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch
    import openintel_amd as oi
    from openintel_amd import synth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = oi.HipContext(0)
    ctx.use_torch_current_stream()
    n, dim = args.docs, args.dim
    rows = synth.embeddings_torch(n, dim, dev, seed=synth.SEED_EMB)
    idx = oi.HybridIndex(ctx, n, dim, synth.VOCAB)
    idx.set_embeddings(rows, normalize=False)
    g = torch.Generator(device=dev)
    g.manual_seed(20240)
    # a day of stamps, uniform; tickers skewed towards the small ids (a few hot ones), one per post
    stamp = torch.randint(0, N_BUCKETS * BUCKET_WIDTH, (n,), device=dev, generator=g, dtype=torch.int32)
    u = torch.rand((n,), device=dev, generator=g, dtype=torch.float32)
    group = (u * u * u * N_KEYS).to(torch.int32).clamp_(0, N_KEYS - 1)
    idx.set_doc_attrs(group, stamp)
    pol = torch.rand((n,), device=dev, generator=g, dtype=torch.float64) * 2.0 - 1.0
    spec = (torch.rand((n,), device=dev, generator=g) < 0.3).to(torch.uint8)
    src = (torch.rand((n,), device=dev, generator=g) < 0.5).to(torch.uint8)
    idx.set_signals(pol, spec, src, 0.2)
    del u, pol, spec, src

    runs = {
        "time": lambda lab, K: idx.label_summary(lab, K, n_buckets=N_BUCKETS, stamp_origin=0, bucket_width=BUCKET_WIDTH),
        "key_dense": lambda lab, K: idx.label_groups(lab, K, KEY_MASK, N_KEYS),
        "key_ranked": lambda lab, K: idx.label_groups(lab, K, KEY_MASK, N_KEYS, top=TOP),
    }
    res = {"tool": "label_summary_bench", "docs": n, "dim": dim, "n_buckets": N_BUCKETS, "n_keys": N_KEYS, "top": TOP,
           "repeats": args.repeats, "cases": []}
    for K in [int(k) for k in args.clusters.split(",") if k]:
        cent = synth.query_batch_torch(K, dim, dev, seed=synth.SEED_QUERY + K)[0]
        share = lambda: idx.similar_share(cent, 0.0, n_buckets=N_BUCKETS, stamp_origin=0, bucket_width=BUCKET_WIDTH, labels=True)
        share_rec, lab = share()
        torch.cuda.synchronize()
        assigned = int((lab >= 0).sum().item())
        algo_bytes = 4 * n + 16 * assigned
        case = {"n_clusters": K, "assigned_rows": assigned, "algorithmic_bytes": algo_bytes, "cells": {"time": K * N_BUCKETS, "key": K * N_KEYS}}
        for name, run in runs.items():
            for _ in range(args.warmup):
                run(lab, K)
                if name == "time":
                    share()
            torch.cuda.synchronize()
            per_tag = {t: [] for t in TAGS}
            share_ms, call_ms = [], []
            for _ in range(args.repeats):                              # alternating: both see the same clocks
                ctx.profile_reset(True)
                c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                c0.record()
                out = run(lab, K)
                c1.record()
                torch.cuda.synchronize()
                call_ms.append(c0.elapsed_time(c1))                    # the whole call: the cells' memset, the pass, the finish
                for t in TAGS:
                    per_tag[t].append(ctx.profile_read(t)[0])
                ctx.profile_reset(False)
                if name == "time":
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    share()
                    b.record()
                    torch.cuda.synchronize()
                    share_ms.append(a.elapsed_time(b))
            p = stats(per_tag["label_summary"])
            entry = {"label_summary": p, "TBps_at_mean": round(algo_bytes / (p["mean_ms"] * 1e-3) / 1e12, 3), "call_event": stats(call_ms)}
            if name == "key_ranked":
                entry["label_summary_rank"] = stats(per_tag["label_summary_rank"])
            if name == "time":
                entry["records_equal_share"] = bool(torch.equal(out, share_rec))
                entry["similar_share_event"] = stats(share_ms)
                entry["time_below_share_every_run"] = bool(max(call_ms) < min(share_ms))
                entry["share_over_call_mean"] = round(float(np.mean(share_ms)) / float(np.mean(call_ms)), 1)
            case[name] = entry
        res["cases"].append(case)
        del lab, cent, share_rec
    res["workspace_bytes"] = ctx.workspace_bytes()[0]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
