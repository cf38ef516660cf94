"""Similarity volume at the flagship size (10M x 768, B = 64, 24 hourly buckets): ms per call of oi_similar_volume at
t in {0.05, 0.1, 0.2, 0.5}, alternating with oi_search on the same index in one process, with rotating query batches as in
bench.py.  Per threshold: the route taken, the undecided pairs the stream sent to the band, the hits counted.  Prints one
JSON line (kept as profiles/volume_bench.json).

    python tools/volume_bench.py [--docs N] [--steps K] [--warmup W] [--thresholds 0.05,0.1,0.2,0.5]

The three kernels' own durations come from a rocprofv3 run of their own (kernel tracing perturbs the step times):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/volume_bench.py --steps 5 --warmup 2 --no-search
    python tools/volume_bench.py --merge TIMING.json --stats-csv DIR/.../*kernel_stats.csv > profiles/volume_bench.json

--merge needs no GPU.  The stream floor is the bf16 screening copy (2 N d bytes) at the copy screen's measured rate
(7.0 TB/s).
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

COPY_STREAM_TBPS = 7.0
# the kernels of a tally: label -> what its name in the trace matches (the family's templates carry the tally as their last argument)
KERNELS = {"vo_stream_kernel<VoCount>": r"vo_stream_kernel<[^>]*VoCount>", "vo_band_kernel<VoCount>": r"vo_band_kernel<VoCount>",
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
    ap.add_argument("--thresholds", default="0.05,0.1,0.2,0.5")
    ap.add_argument("--vocab", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--query-batches", type=int, default=8)
    ap.add_argument("--no-search", action="store_true", help="do not alternate with oi_search (kernel-trace runs)")
    ap.add_argument("--merge", default="", help="a timing line written earlier: add --stats-csv to it and print (no GPU)")
    ap.add_argument("--stats-csv", default="")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge, args.stats_csv)

    import torch
    import openintel_amd as oi
    from openintel_amd import synth

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ctx = oi.HipContext(0)
    ctx.use_torch_current_stream()
    n = args.docs
    rows = synth.embeddings_torch(n, args.dim, dev, seed=synth.SEED_EMB)
    idx = oi.HybridIndex(ctx, n, args.dim, args.vocab)
    idx.set_embeddings(rows, normalize=False)
    terms, offs = synth.forward_index_torch(n, dev, vocab=args.vocab, seed=synth.SEED_TEXT)
    idx.set_forward(terms, offs)
    idx.set_max_query_terms(4)
    del terms, offs
    torch.cuda.empty_cache()
    # a day of posts, one stamp per second of it in row order: 24 hourly buckets
    width = 3600
    stamp = (torch.arange(n, device=dev, dtype=torch.int64) * (args.buckets * width) // n).to(torch.int32)
    idx.set_doc_attrs(None, stamp)
    idx.finalize()
    batches = [synth.query_batch_torch(args.batch, args.dim, dev, vocab=args.vocab, seed=synth.SEED_QUERY + 7919 * i)
               for i in range(args.query_batches)]
    out = oi.SearchResult(torch.zeros((args.batch, 100), dtype=torch.float32, device=dev),
                          torch.zeros((args.batch, 100), dtype=torch.int32, device=dev),
                          torch.zeros((args.batch,), dtype=torch.int32, device=dev))
    ths = [float(t) for t in args.thresholds.split(",") if t]
    names = ([] if args.no_search else ["search"]) + ["t=%g" % t for t in ths]
    last = {}

    def run(name, i):
        qv, qt, qo = batches[i % len(batches)]
        if name == "search":
            idx.search(qv, qt, qo, k=100, depth=1000, out=out)
        else:
            last[name] = idx.similar_volume(qv, float(name[2:]), n_buckets=args.buckets, stamp_origin=0, bucket_width=width)

    for i in range(args.warmup):
        for name in names:
            run(name, i)
    torch.cuda.synchronize()
    total = {name: 0.0 for name in names}
    for i in range(args.steps):          # alternating: every case sees the same clocks and the same neighbours
        for name in names:
            t0 = time.perf_counter()
            run(name, i)
            torch.cuda.synchronize()
            total[name] += time.perf_counter() - t0
    res = {name: {"ms_per_call": round(total[name] * 1e3 / args.steps, 4)} for name in names}
    for name in names:                   # one more profiled call each: the route, the band, the hits
        if name == "search":
            continue
        ctx.profile_reset(True)
        run(name, 0)
        prof = {t: ctx.profile_read(t) for t in ("volume", "volume_band", "volume_exact")}
        ran = [t for t, (_, launches) in prof.items() if launches > 0]
        band, flags = ctx.profile_read("volume_state")
        ctx.profile_reset(False)
        hits = int(last[name].cpu().numpy().view(np.uint32).astype(np.int64).sum())
        res[name].update(route="exact (fallback)" if "volume_exact" in ran else "screen", band_pairs=int(band),
                         band_overflow=bool(int(flags) & 2), hits=hits,
                         proven_hits_at_least=max(hits - int(band), 0) if "volume_exact" not in ran else None,
                         event_ms={t: round(ms, 4) for t, (ms, launches) in prof.items() if launches > 0})
    floor_ms = 2.0 * n * args.dim / (COPY_STREAM_TBPS * 1e12) * 1e3
    print(json.dumps({"tool": "volume_bench", "docs": n, "dim": args.dim, "batch": args.batch, "buckets": args.buckets,
                      "steps": args.steps, "warmup": args.warmup, "stream_floor_ms": round(floor_ms, 3), "cases": res}))


if __name__ == "__main__":
    main()
