"""The update step of narrative discovery at the flagship size (10M x 768 i.i.d. unit rows): oi_label_sums with 100 %, 50 % and
5 % of the rows assigned over 8 / 64 / 256 clusters (labels drawn uniformly, device location), ALTERNATED with the share's
stream (oi_similar_share, B = 8, t = 0.5: every row screened, almost none assigned) on the same index in one process.  Per
case the tool reports the "label_sums" event time per call (mean / min / max / std over the repeats), the bytes the call had
to read (assigned rows x 4 dim + 4 B per row), their time at 7 TB/s and the fraction of that floor the call reaches; next to
it the "share" stream's time of the same session.  Then ONE oi_narratives_fit run (--fit-clusters seeds drawn like queries,
--fit-threshold, --fit-iters steps) with the event time per profile tag and per step.  Prints one JSON line (kept as
profiles/centroids_bench.json).

    python tools/centroid_bench.py [--docs N] [--dim 768] [--shares 1,0.5,0.05] [--clusters 8,64,256] [--steps K] [--warmup W]
                                   [--fit-clusters 8] [--fit-threshold 0.1] [--fit-iters 5]

OI_LIB=ablation OI_LS_NO_ADDS=1 times the variant without the LDS atomics (tools/build_ablation.sh; sums wrong by
construction): what the labels, the row loads and the conversion cost alone.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_TBPS = 7.0   # the copy screen's measured rate
FIT_TAGS = ("share", "share_band", "share_exact", "fit_moved", "label_sums", "centroids")


def _stats(x):
    x = np.asarray(x, dtype=np.float64)
    return {"mean": round(float(x.mean()), 4), "min": round(float(x.min()), 4), "max": round(float(x.max()), 4),
            "std": round(float(x.std()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--shares", default="1,0.5,0.05")
    ap.add_argument("--clusters", default="8,64,256")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--fit-clusters", type=int, default=8)
    ap.add_argument("--fit-threshold", type=float, default=0.1)
    ap.add_argument("--fit-iters", type=int, default=5)
    args = ap.parse_args()

    import torch
    import openintel_amd as oi
    import _ablation  # noqa: F401  (OI_LIB=ablation: the timing variants)
    from openintel_amd import synth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = oi.HipContext(0)
    ctx.use_torch_current_stream()
    n, dim = args.docs, args.dim
    rows = synth.embeddings_torch(n, dim, dev, seed=synth.SEED_EMB)
    idx = oi.HybridIndex(ctx, n, dim, synth.VOCAB)
    idx.set_embeddings(rows, normalize=False)
    terms, offs = synth.forward_index_torch(n, dev, seed=synth.SEED_TEXT)   # (finalize, which makes the screening copy, wants one)
    idx.set_forward(terms, offs)
    del terms, offs
    g = torch.Generator(device=dev)
    g.manual_seed(20263)
    pol = torch.zeros(n, device=dev, dtype=torch.float64)
    spec = (torch.rand(n, device=dev, generator=g) < 0.3).to(torch.uint8)
    src = (torch.rand(n, device=dev, generator=g) < 0.5).to(torch.uint8)
    idx.set_signals(pol, spec, src, 0.2)
    del pol, spec, src
    idx.finalize()
    torch.cuda.empty_cache()

    no_adds = os.environ.get("OI_LS_NO_ADDS", "") == "1"        # (the timing variant: sums and counts wrong by construction)
    q_share = synth.query_batch_torch(8, dim, dev, seed=synth.SEED_QUERY)[0]
    res = {}
    share_ms = []
    for share in [float(s) for s in args.shares.split(",") if s]:
        for K in [int(k) for k in args.clusters.split(",") if k]:
            lab = torch.randint(0, K, (n,), device=dev, generator=g, dtype=torch.int32)
            if share < 1.0:
                lab[torch.rand(n, device=dev, generator=g) >= share] = -1          # 0xFFFFFFFF: no cluster
            assigned = int((lab >= 0).sum().item())
            for _ in range(args.warmup):
                idx.label_sums(lab, K)
                idx.similar_share(q_share, 0.5)
            torch.cuda.synchronize()
            ev, wall = [], []
            for _ in range(args.steps):                                           # alternating: both see the same clocks
                ctx.profile_reset(True)
                t0 = time.perf_counter()
                sums, counts = idx.label_sums(lab, K)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                ev.append(ctx.profile_read("label_sums")[0])
                ctx.profile_reset(True)
                idx.similar_share(q_share, 0.5)
                torch.cuda.synchronize()
                ms, launches = ctx.profile_read("share")
                if launches:
                    share_ms.append(ms)
            ctx.profile_reset(False)
            assert no_adds or int(counts.sum().item()) == assigned
            nbytes = assigned * 4 * dim + 4 * n
            floor_ms = nbytes / (STREAM_TBPS * 1e12) * 1e3
            st = _stats(ev)
            res["assigned=%g K=%d" % (share, K)] = {
                "assigned_rows": assigned, "bytes_to_read": nbytes, "floor_ms_at_7TBps": round(floor_ms, 4), "label_sums_ms": st,
                "fraction_of_floor": round(floor_ms / st["mean"], 4), "achieved_TBps": round(nbytes / (st["mean"] * 1e-3) / 1e12, 3),
                "wall_ms": _stats(wall)}
            del lab, sums, counts

    # one fit: seeds drawn like queries, per-tag event times
    seeds = synth.query_batch_torch(args.fit_clusters, dim, dev, seed=synth.SEED_QUERY + 7919)[0]
    idx.fit_narratives(seeds, args.fit_threshold, max_iters=2)                    # warm-up: every workspace exists
    torch.cuda.synchronize()
    ctx.profile_reset(True)
    t0 = time.perf_counter()
    fit = idx.fit_narratives(seeds, args.fit_threshold, max_iters=args.fit_iters, labels=True)
    torch.cuda.synchronize()
    fit_wall = (time.perf_counter() - t0) * 1e3
    tags = {}
    for tag in FIT_TAGS:
        ms, launches = ctx.profile_read(tag)
        if launches:
            tags[tag] = {"total_ms": round(ms, 4), "launches": int(launches), "ms_per_launch": round(ms / launches, 4)}
    ctx.profile_reset(False)
    ws = ctx.workspace_bytes()[0]
    fit_res = {"clusters": args.fit_clusters, "threshold": args.fit_threshold, "iterations": fit.iterations, "converged": fit.converged,
               "moved": fit.moved, "assigned": fit.assigned, "wall_ms": round(fit_wall, 3),
               "wall_ms_per_step": round(fit_wall / fit.iterations, 3), "event_ms": tags, "workspace_bytes": ws}
    print(json.dumps({"tool": "centroid_bench", "docs": n, "dim": dim, "steps": args.steps, "warmup": args.warmup,
                      "lib": os.environ.get("OI_LIB", "product"), "no_adds_variant": no_adds,
                      "share_stream_ms_same_session": _stats(share_ms) if share_ms else None,
                      "share_stream_floor_ms": round(2.0 * n * dim / (STREAM_TBPS * 1e12) * 1e3, 3),
                      "cases": res, "fit": fit_res}))


if __name__ == "__main__":
    main()
