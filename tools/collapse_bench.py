"""Near-duplicate collapse at the flagship size (10M x 768, B = 64, depth 1000, pool 1000, k 100, t = 0.9, 1 % planted
copies): ms per step of (a) oi_search with k = 100, (b) oi_search with k = 1000 and (c) oi_search_collapsed, alternating in
one process on one index, with rotating query batches as in bench.py.  Prints one JSON line.

    python tools/collapse_bench.py [--docs N] [--steps K] [--warmup W] [--only a,b,c]

The two collapse kernels' own durations come from a rocprofv3 run of their own (kernel tracing perturbs the step times):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/collapse_bench.py --only c --steps 5 --warmup 2
    python tools/collapse_bench.py --merge TIMING.json --stats-csv DIR/.../*kernel_stats.csv > profiles/collapse_bench.json

--merge needs no GPU: it adds the kernels' average microseconds and the Gram kernel's fraction of the 157.3 TFLOP/s f32
matrix peak on its lower-triangle FLOPs to the timing line.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MATRIX_PEAK_TFLOPS = 157.3
TILE = 128  # collapse.hip: CG_TILE


def gram_flops(batch, pool, dim):
    """multiply-adds x 2 of the 64 x 64 wave blocks the Gram kernel computes for full lists: the lower-triangle 128 x 128
    tiles, less the strictly upper quarter of each diagonal tile"""
    ntr = (pool + TILE - 1) // TILE
    tiles = ntr * (ntr + 1) / 2 - ntr * 0.25
    return 2.0 * batch * tiles * TILE * TILE * dim


def merge(timing_path, stats_csv):
    res = json.loads(open(timing_path).read().strip().splitlines()[-1])
    kern = {}
    with open(stats_csv, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for tag in ("collapse_gram_kernel", "collapse_sweep_kernel"):
                if tag in name:
                    k = kern.setdefault(tag, {"calls": 0, "total_ns": 0.0})
                    k["calls"] += int(row["Calls"])
                    k["total_ns"] += float(row["TotalDurationNs"])
    for tag, k in kern.items():
        k["avg_us"] = round(k["total_ns"] / max(k["calls"], 1) / 1e3, 2)
    res["kernels"] = kern
    if "collapse_gram_kernel" in kern:
        fl = gram_flops(res["batch"], res["pool"], res["dim"])
        tf = fl / (kern["collapse_gram_kernel"]["avg_us"] * 1e-6) / 1e12
        res["gram"] = {"flop_per_batch": fl, "tflops": round(tf, 1), "fraction_of_f32_matrix_peak": round(tf / F32_MATRIX_PEAK_TFLOPS, 3)}
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--depth", type=int, default=1000)
    ap.add_argument("--pool", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--copies", type=float, default=0.01, help="fraction of the rows that are planted copies")
    ap.add_argument("--vocab", type=int, default=131072)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--query-batches", type=int, default=8)
    ap.add_argument("--only", default="", help="comma-separated among a,b,c (default: all, alternating)")
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
    # planted copies: blocks of 100 copies of the first sources, scattered over the second half of the corpus
    n_copies = int(n * args.copies)
    n_src = max(n_copies // 100, 1)
    g = torch.Generator(device="cpu").manual_seed(4242)
    targets = (n // 2 + torch.randperm(n - n // 2, generator=g)[:n_copies]).to(dev)
    rows[targets] = rows[torch.arange(n_copies, device=dev) % n_src]
    idx = oi.HybridIndex(ctx, n, args.dim, args.vocab)
    idx.set_embeddings(rows, normalize=False)
    terms, offs = synth.forward_index_torch(n, dev, vocab=args.vocab, seed=synth.SEED_TEXT)
    idx.set_forward(terms, offs)
    idx.set_max_query_terms(4)
    del terms, offs
    torch.cuda.empty_cache()
    idx.finalize()
    batches = []
    for i in range(args.query_batches):
        qv, qt, qo = synth.query_batch_torch(args.batch, args.dim, dev, vocab=args.vocab, seed=synth.SEED_QUERY + 7919 * i)
        # every other query asks for a copied post: its pool holds the whole block of copies
        src = (torch.arange(0, args.batch, 2, device=dev) * 7 + 13 * i) % n_src
        qv[0::2] = rows[src]
        batches.append((qv, qt, qo))

    def result(k, cls):
        mk = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        r = [mk((args.batch, k), torch.float32), mk((args.batch, k), torch.int32), mk((args.batch,), torch.int32)]
        return cls(*r) if cls is oi.SearchResult else cls(*r, mk((args.batch, k), torch.int32))

    from openintel_amd.retriever import CollapsedResult
    out_a, out_b, out_c = result(args.k, oi.SearchResult), result(args.pool, oi.SearchResult), result(args.k, CollapsedResult)

    def run(name, i):
        qv, qt, qo = batches[i % len(batches)]
        if name == "a":
            idx.search(qv, qt, qo, k=args.k, depth=args.depth, out=out_a)
        elif name == "b":
            idx.search(qv, qt, qo, k=args.pool, depth=args.depth, out=out_b)
        else:
            idx.search_collapsed(qv, qt, qo, k=args.k, depth=args.depth, pool=args.pool, threshold=args.threshold, out=out_c)

    names = [c for c in (args.only.split(",") if args.only else ["a", "b", "c"]) if c]
    for i in range(args.warmup):
        for name in names:
            run(name, i)
    ctx.synchronize()
    torch.cuda.synchronize()
    total = {name: 0.0 for name in names}
    for i in range(args.steps):          # alternating: every case sees the same clocks and the same neighbours
        for name in names:
            t0 = time.perf_counter()
            run(name, i)
            torch.cuda.synchronize()
            total[name] += time.perf_counter() - t0
    label = {"a": "search_k%d" % args.k, "b": "search_k%d" % args.pool, "c": "search_collapsed"}
    res = {label[name]: {"ms_per_step": round(total[name] * 1e3 / args.steps, 4)} for name in names}
    if "c" in names:
        cnt = out_c.counts.cpu().numpy().astype(np.int64)
        dup = out_c.dup_counts.cpu().numpy().astype(np.int64)
        res[label["c"]]["mean_kept"] = float(cnt.mean())
        res[label["c"]]["mean_pool_entries_per_kept"] = float(np.mean([dup[b][:cnt[b]].mean() for b in range(args.batch) if cnt[b]]))
    print(json.dumps({"tool": "collapse_bench", "docs": n, "dim": args.dim, "batch": args.batch, "depth": args.depth,
                      "pool": args.pool, "k": args.k, "threshold": args.threshold, "copies": args.copies, "steps": args.steps,
                      "warmup": args.warmup, "cases": res}))


if __name__ == "__main__":
    main()
