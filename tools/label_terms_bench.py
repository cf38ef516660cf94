#!/usr/bin/env python3
"""Narrative terms at the flagship size: the text side of the synth.py corpus at 10M documents, labels from 8 and 256 clusters
with 100 % and 50 % of the rows assigned.  Per case: oi_label_term_counts (profile tag "label_term_counts": the pass over the
postings, the pass over the labels and the zeroing of the table) and oi_label_terms_rank (tag "label_terms_rank"), one profiled
call per repeat, and the count pass's bytes per second against its own byte model.  The yardstick is bm_impact_kernel (tag
"bm25_impact"), which oi_index_finalize runs over the same number of 8-byte records: the index is staged and finalized
`--builds` times in the same process and every finalize gives one sample.

    python tools/label_terms_bench.py [--docs N] [--repeats R] [--builds M]

Prints one JSON line (kept as profiles/label_terms_bench.json).  With OI_LIB=ablation and OI_LT_ABLATE=gather (no label
gather), walk (no block search in cell_start) or adds (the split terms' pieces stored, not added) the same run times a
-DOI_ABLATION build's variants of the count kernel (results wrong by construction).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SPLIT_POSTINGS = 16384   # label_terms.hip: LT_SPLIT_POSTINGS


def stats(x):
    x = np.array(x)
    return {"mean_ms": round(float(x.mean()), 4), "min_ms": round(float(x.min()), 4), "max_ms": round(float(x.max()), 4),
            "max_minus_min_ms": round(float(x.max() - x.min()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--builds", type=int, default=3)
    ap.add_argument("--top", type=int, default=10)
    args = ap.parse_args()

    import torch
    import openintel_amd as oi
    import _ablation  # noqa: F401  (OI_LIB=ablation: tools only)
    from openintel_amd import retriever, synth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = oi.HipContext(0)
    ctx.use_torch_current_stream()
    n = args.docs
    idx = oi.HybridIndex(ctx, n, 4, synth.VOCAB)                 # no embeddings: the calls need the postings only
    terms, offs = synth.forward_index_torch(n, dev)
    impact = []
    for _ in range(max(args.builds, 1)):                         # every finalize runs bm_impact_kernel once
        idx.set_forward(terms, offs)
        ctx.profile_reset(True)
        idx.finalize()
        torch.cuda.synchronize()
        impact.append(ctx.profile_read("bm25_impact")[0])
        ctx.profile_reset(False)
    del terms, offs
    torch.cuda.empty_cache()
    df = idx.local_stats()[1].astype(np.int64)
    n_postings, vocab = int(df.sum()), synth.VOCAB

    g = torch.Generator(device=dev)
    g.manual_seed(20261)
    res = {"tool": "label_terms_bench", "docs": n, "vocab": vocab, "postings": n_postings, "posting_bytes": 8 * n_postings,
           "tasks": n_postings // SPLIT_POSTINGS + 1, "split_terms": int((df >= SPLIT_POSTINGS).sum()),
           "postings_of_split_terms": int(df[df >= SPLIT_POSTINGS].sum()), "repeats": args.repeats, "top": args.top,
           "lib": os.environ.get("OI_LIB", "product"), "ablate": os.environ.get("OI_LT_ABLATE", ""),
           "bm_impact_kernel": stats(impact), "cases": []}
    res["bm_impact_kernel"]["bytes"] = n_postings * (8 + 4 + 8) + 4 * n       # key and tf in, posting out, one doc_len per document
    for K in (8, 256):
        for share in (1.0, 0.5):
            lab = torch.randint(0, K, (n,), device=dev, generator=g, dtype=torch.int32)
            if share < 1.0:
                lab = torch.where(torch.rand(n, device=dev, generator=g) < share, lab, torch.full_like(lab, -1))
            for _ in range(args.warmup):
                counts, sizes = idx.label_term_counts(lab, K)
                retriever.rank_label_terms(ctx, counts, sizes, top=args.top)
            torch.cuda.synchronize()
            t_count, t_rank = [], []
            for _ in range(args.repeats):
                ctx.profile_reset(True)
                counts, sizes = idx.label_term_counts(lab, K)
                torch.cuda.synchronize()
                t_count.append(ctx.profile_read("label_term_counts")[0])
                ctx.profile_reset(False)
                ctx.profile_reset(True)
                retriever.rank_label_terms(ctx, counts, sizes, top=args.top)
                torch.cuda.synchronize()
                t_rank.append(ctx.profile_read("label_terms_rank")[0])
                ctx.profile_reset(False)
            # the count pass's byte model: every posting once, two bounds of cell_start per term (the block search reads more of
            # a term's row, from L2), every label once from HBM (the gathers of a block's 128 KB hit L2), the table zeroed and
            # written once each, the labels once more for the sizes
            model = 8 * n_postings + 8 * vocab + 4 * n + 2 * 4 * vocab * K + 4 * n
            c = stats(t_count)
            res["cases"].append({"n_clusters": K, "assigned_share": share, "assigned_rows": int(sizes.sum().item()),
                                 "label_term_counts": c, "label_terms_rank": stats(t_rank), "model_bytes": model,
                                 "model_GBps_at_mean": round(model / c["mean_ms"] / 1e6, 1),
                                 "vs_bm_impact_mean": round(c["mean_ms"] / res["bm_impact_kernel"]["mean_ms"], 3)})
            del lab, counts, sizes
    print(json.dumps(res))


if __name__ == "__main__":
    main()
