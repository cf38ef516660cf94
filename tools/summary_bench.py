"""Similarity summary at the flagship size (10M x 768 i.i.d. unit rows, B = 64, 24 hourly buckets): ms per call of
oi_similar_summary at t in {0.5, 0.2, 0.1}, ALTERNATED with oi_similar_volume for the same arguments on the same index in one
process, with rotating query batches as in bench.py.  The yardstick is the volume call itself: per threshold the two calls'
mean, min and max over the alternated repeats (the volume's own spread is the bar a difference has to clear), the route taken,
the undecided pairs the stream sent to the band, the stream / band / fallback event times of one profiled call each, the hits,
and the share of hits that needed the second (64-bit) atomic.  Prints one JSON line (kept as profiles/summary_bench.json).

    python tools/summary_bench.py [--docs N] [--steps K] [--warmup W] [--thresholds 0.5,0.2,0.1] [--nonzero 0.03]

Signals: a share --nonzero of the posts (default 3 %, the share actually drawn is reported) has polarity +1 or -1, half
each, the rest 0; 30 % speculative; sources a coin flip.  A non-zero polarity is then exactly a bullish or bearish post, so
the second-atomic share of a call is (bullish + bearish) / total of its records.

The kernels' own durations come from a rocprofv3 run of their own (kernel tracing perturbs the step times):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/summary_bench.py --steps 5 --warmup 2
    python tools/summary_bench.py --merge TIMING.json --stats-csv DIR/.../*kernel_stats.csv > profiles/summary_bench.json

--merge needs no GPU.
"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_STREAM_TBPS = 7.0   # the copy screen's measured rate
# the kernels of the two tallies: label -> what its name in the trace matches (the family's templates carry the tally as their
# last argument)
KERNELS = {"vo_stream_kernel<SmSum>": r"vo_stream_kernel<[^>]*SmSum>", "vo_band_kernel<SmSum>": r"vo_band_kernel<SmSum>",
           "vo_exact_kernel<SmSum>": r"vo_exact_kernel<[^>]*SmSum>", "summary_finish_kernel": r"summary_finish_kernel",
           "vo_stream_kernel<VoCount>": r"vo_stream_kernel<[^>]*VoCount>", "vo_band_kernel<VoCount>": r"vo_band_kernel<VoCount>",
           "vo_exact_kernel<VoCount>": r"vo_exact_kernel<[^>]*VoCount>"}


def merge(timing_path, stats_csv):
    res = json.loads(open(timing_path).read().strip().splitlines()[-1])
    kern = {}
    with open(stats_csv, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for tag, pattern in KERNELS.items():
                if re.search(pattern, name):
                    k = kern.setdefault(tag, {"calls": 0, "total_ns": 0.0})
                    k["calls"] += int(row["Calls"])
                    k["total_ns"] += float(row["TotalDurationNs"])
    for k in kern.values():
        k["avg_us"] = round(k["total_ns"] / max(k["calls"], 1) / 1e3, 2)
    res["kernels"] = kern
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--buckets", type=int, default=24)
    ap.add_argument("--thresholds", default="0.5,0.2,0.1")
    ap.add_argument("--nonzero", type=float, default=0.03, help="share of posts with a non-zero polarity")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--query-batches", type=int, default=8)
    ap.add_argument("--merge", default="", help="a timing line written earlier: add --stats-csv to it and print (no GPU)")
    ap.add_argument("--stats-csv", default="")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.stats_csv)

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
    # a day of posts, one stamp per second of it in row order: 24 hourly buckets
    width = 3600
    stamp = (torch.arange(n, device=dev, dtype=torch.int64) * (args.buckets * width) // n).to(torch.int32)
    idx.set_doc_attrs(None, stamp)
    g = torch.Generator(device=dev)
    g.manual_seed(20260)
    u = torch.rand(n, device=dev, generator=g)
    pol = torch.where(u < args.nonzero / 2, 1.0, torch.where(u < args.nonzero, -1.0, 0.0)).to(torch.float64)
    spec = (torch.rand(n, device=dev, generator=g) < 0.3).to(torch.uint8)
    src = (torch.rand(n, device=dev, generator=g) < 0.5).to(torch.uint8)
    nonzero_share = float((pol != 0).double().mean().item())
    idx.set_signals(pol, spec, src, 0.2)
    del u, pol, spec, src
    idx.finalize()                       # (the bf16 screening copy: the stream route)
    torch.cuda.empty_cache()
    batches = [synth.query_batch_torch(args.batch, args.dim, dev, seed=synth.SEED_QUERY + 7919 * i)[0]
               for i in range(args.query_batches)]
    ths = [float(t) for t in args.thresholds.split(",") if t]
    kw = dict(n_buckets=args.buckets, stamp_origin=0, bucket_width=width)
    calls = {"summary": idx.similar_summary, "volume": idx.similar_volume}
    last = {}

    def run(call, t, i):
        last[call, t] = calls[call](batches[i % len(batches)], t, **kw)

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
            tags = ("summary", "summary_band", "summary_exact") if call == "summary" else ("volume", "volume_band", "volume_exact")
            ctx.profile_reset(True)      # one more profiled call: the route, the band, the event times
            run(call, t, 0)
            prof = {tag: ctx.profile_read(tag) for tag in tags}
            band, flags = ctx.profile_read(call + "_state")
            ctx.profile_reset(False)
            ran = [tag for tag, (_, launches) in prof.items() if launches > 0]
            case[call].update(route="exact (fallback)" if tags[2] in ran else "screen", band_pairs=int(band),
                              band_overflow=bool(int(flags) & 2),
                              event_ms={tag: round(ms, 4) for tag, (ms, launches) in prof.items() if launches > 0})
        rec = last["summary", t].cpu().numpy().view(COUNTERS_DTYPE).reshape(args.batch, args.buckets)
        vol = last["volume", t].cpu().numpy().view(np.uint32).astype(np.uint64)
        hits = int(rec["total"].sum())
        second = int(rec["bullish"].sum() + rec["bearish"].sum())
        case.update(hits=hits, total_equals_volume=bool(np.array_equal(rec["total"], vol)), second_atomic_hits=second,
                    second_atomic_share=round(second / hits, 5) if hits else None,
                    summary_minus_volume_ms=round(case["summary"]["ms_per_call"] - case["volume"]["ms_per_call"], 4))
        res["t=%g" % t] = case
    floor_ms = 2.0 * n * args.dim / (COPY_STREAM_TBPS * 1e12) * 1e3
    print(json.dumps({"tool": "summary_bench", "docs": n, "dim": args.dim, "batch": args.batch, "buckets": args.buckets,
                      "steps": args.steps, "warmup": args.warmup, "nonzero_polarity_share": round(nonzero_share, 5),
                      "stream_floor_ms": round(floor_ms, 3), "cases": res}))


if __name__ == "__main__":
    main()
