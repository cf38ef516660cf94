#!/usr/bin/env python3
"""Narrative exemplars at the flagship size: the synth.py corpus (10M x 768 i.i.d. unit rows), labelled by oi_similar_share with
8 and with 256 query vectors as centroids.  Per case: oi_label_exemplars, one profiled call per repeat, with the event time per
profile tag ("exemplar_score": the stream of the member rows; "exemplar_select": the segmented radix select; "exemplar_emit":
collect, sort, write), ALTERNATED with oi_label_sums (tag "label_sums") on the same labels in the same session: that pass reads
the same member rows, so it is the yardstick.  Next to the times: the bytes the score pass had to move (assigned rows x 4 dim,
a label in and a key out per row) and the rate it reached.  No pass/fail bar.

    python tools/exemplar_bench.py [--docs N] [--dim 768] [--clusters 8,256] [--threshold 0.0] [--top 10] [--repeats R]

Prints one JSON line (kept as profiles/exemplar_bench.json).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAGS = ("exemplar_score", "exemplar_select", "exemplar_emit")


def stats(x):
    x = np.asarray(x, dtype=np.float64)
    return {"mean_ms": round(float(x.mean()), 4), "min_ms": round(float(x.min()), 4), "max_ms": round(float(x.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--clusters", default="8,256")
    ap.add_argument("--threshold", type=float, default=0.0)
    ap.add_argument("--top", type=int, default=10)
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
    idx.set_signals(torch.zeros(n, device=dev, dtype=torch.float64), torch.zeros(n, device=dev, dtype=torch.uint8),
                    torch.zeros(n, device=dev, dtype=torch.uint8), 0.2)     # (the share that makes the labels wants them)

    res = {"tool": "exemplar_bench", "docs": n, "dim": dim, "top": args.top, "threshold": args.threshold, "repeats": args.repeats,
           "cases": []}
    for K in [int(k) for k in args.clusters.split(",") if k]:
        cent = synth.query_batch_torch(K, dim, dev, seed=synth.SEED_QUERY + K)[0]
        _, lab = idx.similar_share(cent, args.threshold, labels=True)
        torch.cuda.synchronize()
        assigned = int((lab >= 0).sum().item())
        for _ in range(args.warmup):
            idx.label_exemplars(lab, cent, top=args.top)
            idx.label_sums(lab, K)
        torch.cuda.synchronize()
        per_tag = {t: [] for t in TAGS}
        total, sums_ms, wall = [], [], []
        for _ in range(args.repeats):                                  # alternating: both see the same clocks
            ctx.profile_reset(True)
            t0 = time.perf_counter()
            lists = idx.label_exemplars(lab, cent, top=args.top)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms = [ctx.profile_read(t)[0] for t in TAGS]
            for t, v in zip(TAGS, ms):
                per_tag[t].append(v)
            total.append(sum(ms))
            ctx.profile_reset(True)
            idx.label_sums(lab, K)
            torch.cuda.synchronize()
            sums_ms.append(ctx.profile_read("label_sums")[0])
        ctx.profile_reset(False)
        listed = int(lists.cos_counts.sum().item())
        row_bytes = assigned * 4 * dim
        score_bytes = row_bytes + 8 * n                                # a label in and a key out per row
        sc, ls = stats(per_tag["exemplar_score"]), stats(sums_ms)
        res["cases"].append({
            "n_clusters": K, "assigned_rows": assigned, "listed": listed,
            "label_exemplars_ms": stats(total), "wall_ms": stats(wall),
            "exemplar_score": sc, "exemplar_select": stats(per_tag["exemplar_select"]), "exemplar_emit": stats(per_tag["exemplar_emit"]),
            "label_sums": ls, "score_vs_label_sums_mean": round(sc["mean_ms"] / ls["mean_ms"], 3),
            "score_bytes": score_bytes, "score_TBps_at_mean": round(score_bytes / (sc["mean_ms"] * 1e-3) / 1e12, 3),
            "label_sums_bytes": row_bytes + 4 * n, "label_sums_TBps_at_mean": round((row_bytes + 4 * n) / (ls["mean_ms"] * 1e-3) / 1e12, 3),
            "select_bytes_per_pass": 8 * n})
        del lab, cent, lists
    res["workspace_bytes"] = ctx.workspace_bytes()[0]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
