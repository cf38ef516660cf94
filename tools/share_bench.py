"""Similarity share at the flagship size (10M x 768 i.i.d. unit rows, B = 8 and 64): oi_similar_share at t in {0.5, 0.2, 0.1},
ALTERNATED with oi_similar_summary for the same arguments (one bucket, no filters) on the same index in one process, with
rotating query batches as in bench.py.  The yardstick is the summary's "summary" stream in that same run: the two kernels move
the same bytes through the same tile loop, and the share's extra per-row work sits behind the ballot.  Every repeat is
profiled, so per (B, t) and call the tool reports the event time per profile tag as mean / min / max / std over the repeats
("share" and "summary" are the streams; "share_band" holds the rescoring AND the commit), the wall time per call, the route,
the band fill, the assigned posts against the summary's hits, the ratio of the two streams' means and whether the share
stream's mean lies inside the spread of the summary stream's repeats.  Prints one JSON line (kept as
profiles/share_bench.json).

    python tools/share_bench.py [--docs N] [--dim 768] [--batches 8,64] [--thresholds 0.5,0.2,0.1] [--steps K] [--warmup W]
                                [--nonzero 0.03] [--labels]

Signals as in tools/summary_bench.py: a share --nonzero of the posts has polarity +1 or -1, half each, the rest 0; 30 %
speculative; sources a coin flip.  --labels also asks for the per-row labels (4 B per row more to preset and, for a winner,
to write).
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
TAGS = {"share": ("share", "share_band", "share_exact"), "summary": ("summary", "summary_band", "summary_exact")}


def _stats(x):
    x = np.asarray(x, dtype=np.float64)
    return {"mean": round(float(x.mean()), 4), "min": round(float(x.min()), 4), "max": round(float(x.max()), 4),
            "std": round(float(x.std()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batches", default="8,64")
    ap.add_argument("--thresholds", default="0.5,0.2,0.1")
    ap.add_argument("--nonzero", type=float, default=0.03, help="share of posts with a non-zero polarity")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--query-batches", type=int, default=8)
    ap.add_argument("--labels", action="store_true", help="ask the share call for the per-row labels as well")
    args = ap.parse_args()

    import torch
    import openintel_amd as oi
    from openintel_amd import synth
    from openintel_amd.analyzer import COUNTERS_DTYPE

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = oi.HipContext(0)
    ctx.use_torch_current_stream()
    n = args.docs
    rows = synth.embeddings_torch(n, args.dim, dev, seed=synth.SEED_EMB)
    idx = oi.HybridIndex(ctx, n, args.dim, synth.VOCAB)
    idx.set_embeddings(rows, normalize=False)
    terms, offs = synth.forward_index_torch(n, dev, seed=synth.SEED_TEXT)   # (finalize, which makes the screening copy, wants one)
    idx.set_forward(terms, offs)
    del terms, offs
    g = torch.Generator(device=dev)
    g.manual_seed(20262)
    u = torch.rand(n, device=dev, generator=g)
    pol = torch.where(u < args.nonzero / 2, 1.0, torch.where(u < args.nonzero, -1.0, 0.0)).to(torch.float64)
    spec = (torch.rand(n, device=dev, generator=g) < 0.3).to(torch.uint8)
    src = (torch.rand(n, device=dev, generator=g) < 0.5).to(torch.uint8)
    nonzero_share = float((pol != 0).double().mean().item())
    idx.set_signals(pol, spec, src, 0.2)
    del u, pol, spec, src
    idx.finalize()                       # (the bf16 screening copy: the stream route)
    torch.cuda.empty_cache()
    ths = [float(t) for t in args.thresholds.split(",") if t]
    calls = {"share": lambda q, t: idx.similar_share(q, t, labels=args.labels),
             "summary": lambda q, t: idx.similar_summary(q, t)}
    res = {}
    for B in [int(b) for b in args.batches.split(",") if b]:
        batches = [synth.query_batch_torch(B, args.dim, dev, seed=synth.SEED_QUERY + 7919 * i)[0] for i in range(args.query_batches)]
        last = {}

        def run(call, t, i):
            last[call, t] = calls[call](batches[i % len(batches)], t)

        for i in range(args.warmup):
            for t in ths:
                for call in calls:
                    run(call, t, i)
        torch.cuda.synchronize()
        wall = {(call, t): [] for t in ths for call in calls}
        ev = {(call, t, tag): [] for t in ths for call in calls for tag in TAGS[call]}
        state = {}
        for i in range(args.steps):      # alternating: both calls see the same clocks and the same neighbours
            for t in ths:
                for call in calls:
                    ctx.profile_reset(True)
                    t0 = time.perf_counter()
                    run(call, t, i)
                    torch.cuda.synchronize()
                    wall[call, t].append((time.perf_counter() - t0) * 1e3)
                    for tag in TAGS[call]:
                        ms, launches = ctx.profile_read(tag)
                        if launches > 0:
                            ev[call, t, tag].append(ms)
                    if i == 0:           # (batch 0: the one the results below come from)
                        state[call, t] = ctx.profile_read(call + "_state")
                        state[call, t, "out"] = last[call, t]
        ctx.profile_reset(False)
        for t in ths:
            case = {}
            for call in calls:
                band, flags = state[call, t]
                ran = [tag for tag in TAGS[call] if ev[call, t, tag]]
                case[call] = {"wall_ms": _stats(wall[call, t]), "route": "exact (fallback)" if TAGS[call][2] in ran else "screen",
                              "band_pairs": int(band), "band_overflow": bool(int(flags) & 2),
                              "event_ms": {tag: _stats(ev[call, t, tag]) for tag in ran}}
            out = state["share", t, "out"]
            rec = (out[0] if args.labels else out).cpu().numpy().view(COUNTERS_DTYPE).reshape(B, 1)
            one = state["summary", t, "out"].cpu().numpy().view(COUNTERS_DTYPE).reshape(B, 1)
            sh, sm = case["share"]["event_ms"].get("share"), case["summary"]["event_ms"].get("summary")
            if sh and sm:
                case.update(stream_ratio_share_over_summary=round(sh["mean"] / sm["mean"], 4),
                            share_stream_mean_inside_summary_stream_spread=bool(sm["min"] <= sh["mean"] <= sm["max"]),
                            summary_stream_spread_ms=[sm["min"], sm["max"]])
            case.update(assigned_posts=int(rec["total"].sum()), summary_hits=int(one["total"].sum()),
                        totals_at_most_the_summarys=bool((rec["total"] <= one["total"]).all()))
            res["B=%d t=%g" % (B, t)] = case
    floor_ms = 2.0 * n * args.dim / (COPY_STREAM_TBPS * 1e12) * 1e3
    print(json.dumps({"tool": "share_bench", "docs": n, "dim": args.dim, "labels": bool(args.labels), "steps": args.steps,
                      "warmup": args.warmup, "nonzero_polarity_share": round(nonzero_share, 5), "best_bytes_zeroed_per_call": 8 * n,
                      "stream_floor_ms": round(floor_ms, 3), "cases": res}))


if __name__ == "__main__":
    main()
