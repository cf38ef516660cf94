#!/usr/bin/env python3
"""OI_LIB=ablation OI_SELECT_STAMPS=1 python tools/sel_debug.py : the small screened search of tests/test_gpu_prefilter.py through the
ablation build (select_flat's self-check prints a MISMATCH line when the super-bin search and the plain walk disagree).

OI_LIB=ablation OI_SELECT_V1=1 python tools/sel_debug.py merge : every MERGE_ROWS row of tests/test_gpu_search_tail_edges.py through
merge_lists, from host arrays and from device tensors, against ref_merge (counts, doc ids, score bits).  With OI_SELECT_V1 the plain
selects take select_topk_kernel, which no product run reaches.  Exit status 1 on any mismatch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import openintel_amd as oi
import _ablation  # noqa: F401
from openintel_amd import synth


def merge_rows(ctx):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_search_tail_edges as T
    bad = 0
    for row in T.MERGE_ROWS:
        call = T.merge_call(row.name)
        depth = call.scores.shape[2]
        for device in (False, True):
            so, do, co = T._merge(ctx, call, device)
            for b in range(call.scores.shape[1]):
                bits, docs = T.ref_merge(call.scores[:, b], call.docs[:, b], call.counts[:, b], depth)
                m = int(co[b])
                if m != docs.size or not np.array_equal(do[b, :m], docs) or not np.array_equal(so[b, :m].view(np.uint32), bits):
                    bad += 1
                    print("MISMATCH %s %s query %d: count %d, reference %d" % (row.name, "device" if device else "host", b, m, docs.size))
        print("%-40s %d queries, host and device" % (row.name, call.scores.shape[1]), flush=True)
    print("merge rows: %d rows, %d mismatches (OI_SELECT_V1=%s)" % (len(T.MERGE_ROWS), bad, os.environ.get("OI_SELECT_V1", "")))
    return 1 if bad else 0


if sys.argv[1:2] == ["merge"]:
    sys.exit(merge_rows(oi.HipContext(0)))

B, dim, n = 9, 768, 5000
ctx = oi.HipContext(0)
rows = synth.embeddings_np(n, dim, seed=3 + B)
q = synth.embeddings_np(B, dim, seed=55 + B)
rng = np.random.default_rng(B)
lens = rng.integers(1, 8, size=n)
offs = np.zeros(n + 1, np.uint64)
offs[1:] = np.cumsum(lens)
terms = rng.integers(0, 50, size=int(offs[-1])).astype(np.uint32)
idx = oi.HybridIndex(ctx, n, dim, 50, doc_id_base=77)
idx.set_embeddings(rows, normalize=False)
idx.set_forward(terms, offs)
idx.finalize()
qt, qo = np.zeros(B, np.uint32), np.arange(B + 1, dtype=np.uint32)
for depth in (10, 1000):
    L = idx.search_lists(q, qt, qo, depth=depth)
    print(depth, L.cos_counts)
