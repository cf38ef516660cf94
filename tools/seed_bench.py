"""Narrative seeding at the flagship size (10M x 768 i.i.d. unit rows, device location): oi_narratives_seed with trials 1, 4 and
8, ALTERNATED in one process with oi_label_sums at 100 % assigned -- the call that reads the same bytes.  Per trials value the
tool reports the "seed_score" event time per pass (a call of n_clusters seeds runs one pass that scores seed 0 alone and
n_clusters - 1 passes that score `trials` candidates; the time of the first, taken from the trials = 1 runs of the same session,
is subtracted), the "seed_pick" time per launch and the "seed_init" time; the bytes a pass moves (rows, and the per-row w / cw
traffic), their time at 7 TB/s and the fraction of that floor the pass reaches.  Then the whole call at --call-clusters seeds
(wall and event times), and ONE batch.discover_narratives(index, --fit-clusters, --fit-threshold) wall time.  Prints one JSON
line (kept as profiles/seed_bench.json).

    python tools/seed_bench.py [--docs N] [--dim 768] [--trials 1,4,8] [--clusters 5] [--steps K] [--warmup W]
                               [--call-clusters 16] [--fit-clusters 8] [--fit-threshold 0.1]

OI_LIB=ablation OI_NS_NO_CHAIN=1 times the variant without the candidate reads, the chains and the wave sums
(tools/build_ablation.sh; seeds wrong by construction): what the w reads, the row loads and the stores cost alone.
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
TAGS = ("seed_init", "seed_score", "seed_pick")


def _stats(x):
    x = np.asarray(x, dtype=np.float64)
    return {"mean": round(float(x.mean()), 4), "min": round(float(x.min()), 4), "max": round(float(x.max()), 4),
            "std": round(float(x.std()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--trials", default="1,4,8")
    ap.add_argument("--clusters", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--call-clusters", type=int, default=16)
    ap.add_argument("--fit-clusters", type=int, default=8)
    ap.add_argument("--fit-threshold", type=float, default=0.1)
    args = ap.parse_args()

    import torch
    import openintel_amd as oi
    import _ablation  # noqa: F401  (OI_LIB=ablation: the timing variants)
    from openintel_amd import batch, synth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = oi.HipContext(0)
    ctx.use_torch_current_stream()
    n, dim, K = args.docs, args.dim, args.clusters
    rows = synth.embeddings_torch(n, dim, dev, seed=synth.SEED_EMB)
    idx = oi.HybridIndex(ctx, n, dim, synth.VOCAB)
    idx.set_embeddings(rows, normalize=False)
    no_chain = os.environ.get("OI_NS_NO_CHAIN", "") == "1"      # (the timing variant: seeds wrong by construction)
    with_fit = not no_chain and args.fit_clusters > 0
    if with_fit:                                                # the fit wants signals, its stream route a finalized index
        terms, offs = synth.forward_index_torch(n, dev, seed=synth.SEED_TEXT)
        idx.set_forward(terms, offs)
        del terms, offs
        g = torch.Generator(device=dev)
        g.manual_seed(20263)
        idx.set_signals(torch.zeros(n, device=dev, dtype=torch.float64), (torch.rand(n, device=dev, generator=g) < 0.3).to(torch.uint8),
                        (torch.rand(n, device=dev, generator=g) < 0.5).to(torch.uint8), 0.2)
        idx.finalize()
        torch.cuda.empty_cache()
    lab = torch.zeros(n, device=dev, dtype=torch.int32)         # label_sums with every row assigned (8 clusters, round robin)
    lab[:] = torch.arange(n, device=dev, dtype=torch.int32) % 8

    res = {}
    sums_ms = []
    first_pass_ms = None
    for L in [int(t) for t in args.trials.split(",") if t]:
        for _ in range(args.warmup):
            idx.seed_narratives(K, trials=L, seed=1, device=True)
            idx.label_sums(lab, 8)
        torch.cuda.synchronize()
        score, pick, init, wall = [], [], [], []
        for r in range(args.steps):                             # alternating: both see the same clocks
            ctx.profile_reset(True)
            t0 = time.perf_counter()
            s = idx.seed_narratives(K, trials=L, seed=r, device=True)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms, launches = ctx.profile_read("seed_score")
            assert launches == K and (no_chain or s.found == K)
            score.append(ms)
            pick.append(ctx.profile_read("seed_pick")[0] / (K + 1))
            init.append(ctx.profile_read("seed_init")[0])
            ctx.profile_reset(True)
            idx.label_sums(lab, 8)
            torch.cuda.synchronize()
            sums_ms.append(ctx.profile_read("label_sums")[0])
        ctx.profile_reset(False)
        score = np.asarray(score)
        if L == 1:
            per_pass = score / K
            first_pass_ms = float(per_pass.mean())
            nbytes = n * (4 * dim + 4 + 4)                      # rows, w read, w written
        else:
            assert first_pass_ms is not None, "--trials must begin with 1: the first pass of every call scores one vector"
            per_pass = (score - first_pass_ms) / (K - 1)
            nbytes = n * (4 * dim + 4 + 4 * L + 4 + 4)          # rows, w read, cw written; then (all but the first) cw[t*] read, w written
        floor_ms = nbytes / (STREAM_TBPS * 1e12) * 1e3
        st = _stats(per_pass)
        res["trials=%d" % L] = {"seed_score_ms_per_pass": st, "bytes_per_pass": nbytes, "floor_ms_at_7TBps": round(floor_ms, 4),
                                "fraction_of_floor": round(floor_ms / st["mean"], 4),
                                "achieved_TBps": round(nbytes / (st["mean"] * 1e-3) / 1e12, 3), "seed_pick_ms_per_launch": _stats(pick),
                                "seed_init_ms": _stats(init), "call_wall_ms_at_%d_clusters" % K: _stats(wall)}

    # the whole call
    Kc = args.call_clusters
    idx.seed_narratives(Kc, trials=4, seed=0, device=True)
    torch.cuda.synchronize()
    ctx.profile_reset(True)
    t0 = time.perf_counter()
    s = idx.seed_narratives(Kc, trials=4, seed=0, device=True)
    torch.cuda.synchronize()
    call_wall = (time.perf_counter() - t0) * 1e3
    tags = {}
    for tag in TAGS:
        ms, launches = ctx.profile_read(tag)
        tags[tag] = {"total_ms": round(ms, 4), "launches": int(launches)}
    ctx.profile_reset(False)
    call = {"clusters": Kc, "trials": 4, "found": s.found, "eligible": s.eligible, "potential": s.potential, "wall_ms": round(call_wall, 3),
            "event_ms": tags, "workspace_bytes": ctx.workspace_bytes()[0]}

    fit_res = None
    if with_fit:
        batch.discover_narratives(idx, args.fit_clusters, args.fit_threshold, max_iters=2)     # warm-up: every workspace exists
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fit, _ = batch.discover_narratives(idx, args.fit_clusters, args.fit_threshold, max_iters=5)
        torch.cuda.synchronize()
        fit_res = {"clusters": args.fit_clusters, "threshold": args.fit_threshold, "wall_ms": round((time.perf_counter() - t0) * 1e3, 3),
                   "iterations": fit.iterations, "converged": fit.converged, "assigned": fit.assigned}
    print(json.dumps({"tool": "seed_bench", "docs": n, "dim": dim, "clusters": K, "steps": args.steps, "warmup": args.warmup,
                      "lib": os.environ.get("OI_LIB", "product"), "no_chain_variant": no_chain,
                      "label_sums_ms_same_session": _stats(sums_ms), "label_sums_bytes": n * (4 * dim + 4),
                      "cases": res, "call": call, "discover_narratives": fit_res}))


if __name__ == "__main__":
    main()
