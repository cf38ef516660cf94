#!/usr/bin/env python3
"""The GPU tokeniser (oi_text_terms / oi_index_set_text) at full size: N synth.posts_torch posts resident in HBM.
In one process: ms of the count pass (count kernel + scan of the tile counts) and of the emit pass, of set_text end to
end, of set_forward alone on the same ids, and of lexicon_scan_kernel on the same blob; algorithmic bytes, GB/s and the
share of 8 TB/s; and the SINGLE-THREAD HOST rate of the same tokens + hash in Python (oracle.pyref.tokens) on a sample,
labelled as such.  Prints one JSON line.  (The host restatement is the tests' -- tests/test_text_terms_abi.py, imported
from there: it is deliberately not part of the product, so this tool needs the repository's tests/ beside it.)

    python tools/text_terms_bench.py [--posts N] [--reps R] [--vocab V] [--host-sample S]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--posts", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--vocab", type=int, default=131072)
    ap.add_argument("--host-sample", type=int, default=200_000)
    args = ap.parse_args()

    import numpy as np
    import torch
    import openintel_amd as oi
    from openintel_amd import _lib, synth

    n, V = args.posts, args.vocab
    dev = torch.device("cuda:0")
    ctx = oi.HipContext(0)
    ctx.use_torch_current_stream()
    blob, offs = synth.posts_torch(n, dev)
    text_bytes = blob.numel()
    cap = (text_bytes + 1) // 2                        # always enough: the call below is asynchronous
    ids = torch.zeros(cap, dtype=torch.int32, device=dev)
    toffs = torch.zeros(n + 1, dtype=torch.int64, device=dev)

    def tokenise():
        _lib.check(ctx.lib.oi_text_terms(ctx.handle, _lib.ptr(blob), _lib.ptr(offs), n, text_bytes, V, _lib.OI_DEVICE,
                                         _lib.ptr(ids), cap, _lib.ptr(toffs), None))

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    tokenise()
    torch.cuda.synchronize()
    tokens = int(toffs[-1].item())
    ctx.profile_reset(True)
    call_ms = timed(tokenise, args.reps)
    c_ms, c_n = ctx.profile_read("text_count")
    e_ms, e_n = ctx.profile_read("text_emit")
    ctx.profile_reset(False)
    count_ms, emit_ms = c_ms / c_n, e_ms / e_n
    unprofiled_call_ms = timed(tokenise, args.reps)

    # lexicon_scan_kernel on the same blob, same process
    pol = torch.zeros(n, dtype=torch.float64, device=dev)
    spec = torch.zeros(n, dtype=torch.uint8, device=dev)
    an = oi.HipLexiconAnalyzer(ctx)
    an.analyze_device(blob, offs, pol, spec)
    torch.cuda.synchronize()
    ctx.profile_reset(True)
    timed(lambda: an.analyze_device(blob, offs, pol, spec), args.reps)
    l_ms, l_n = ctx.profile_read("lexicon")
    ctx.profile_reset(False)
    lexicon_ms = l_ms / l_n
    del pol, spec

    # the index build: set_text end to end, set_forward alone on the same ids
    idx = oi.HybridIndex(ctx, n, 4, V)
    reps_build = max(1, min(3, args.reps))
    set_text_ms = timed(lambda: idx.set_text((blob, offs)), reps_build)
    tot_text, _ = idx.local_stats()
    exact = ids[:tokens]
    set_forward_ms = timed(lambda: idx.set_forward(exact, toffs), reps_build)
    tot_fwd, _ = idx.local_stats()
    idx.close()

    # single-thread host rate: the same tokens and the same hash in Python (the restatement the tests use)
    from test_text_terms_abi import ref_text_terms
    ns = min(n, args.host_sample)
    h_offs = offs[:ns + 1].cpu().numpy()
    h_blob = blob[:int(h_offs[-1])].cpu().numpy().tobytes()
    texts = [h_blob[h_offs[i]:h_offs[i + 1]].decode("ascii") for i in range(ns)]
    t0 = time.perf_counter()
    want, want_offs = ref_text_terms(texts, V)
    host_s = time.perf_counter() - t0
    sample_equal = bool(np.array_equal(ids[:want.size].cpu().numpy().view(np.uint32), want)
                        and np.array_equal(toffs[:ns + 1].cpu().numpy().view(np.uint64), want_offs))

    passes = 2
    alg = passes * text_bytes + 16 * (n + 1) + 4 * tokens   # text read by both passes, offsets in and out, ids out
    tok_ms = count_ms + emit_ms
    print(json.dumps({
        "tool": "text_terms_bench", "posts": n, "vocab": V, "text_bytes": text_bytes, "tokens": tokens, "reps": args.reps,
        "count_pass_ms": round(count_ms, 4), "emit_pass_ms": round(emit_ms, 4), "tokeniser_kernels_ms": round(tok_ms, 4),
        "tokeniser_call_ms": round(unprofiled_call_ms, 4), "tokeniser_call_ms_profiled": round(call_ms, 4),
        "passes_over_text": passes, "algorithmic_bytes": alg, "algorithmic_GBs": round(alg / (tok_ms / 1e3) / 1e9, 1),
        "frac_of_8TBs": round(alg / (tok_ms / 1e3) / 8e12, 4),
        "posts_per_s": round(n / (tok_ms / 1e3)), "tokens_per_s": round(tokens / (tok_ms / 1e3)),
        "lexicon_scan_kernel_ms": round(lexicon_ms, 4), "tokeniser_over_lexicon_scan": round(tok_ms / lexicon_ms, 2),
        "set_text_ms": round(set_text_ms, 2), "set_forward_ms_same_ids": round(set_forward_ms, 2),
        "tokeniser_share_of_set_text": round(tok_ms / set_text_ms, 4),
        "set_text_tokens_equal_set_forward": tot_text == tot_fwd == tokens,
        "host_single_thread_python": {"what": "oracle.pyref.tokens + FNV-1a/fmix64 in Python, ONE host thread", "sample_posts": ns,
                                      "seconds": round(host_s, 3), "posts_per_s": round(ns / host_s),
                                      "gpu_equals_host_on_sample": sample_equal},
    }))


if __name__ == "__main__":
    main()
