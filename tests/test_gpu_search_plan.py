"""The launch schedule of every route through one hybrid search (csrc/search.hip: search_lists_device), pinned.

The f32 cosine routes return the same lists whatever their chunk schedule is, and the BM25 modes return bit-identical lists, so a
changed schedule, a lost speculation launch or a BM25 leg that quietly takes another kernel would only show up as a change in
speed.  Each case here runs hybrid searches on a fresh context with every launch profiled and compares, per search, the launch
count of each tagged kernel family, the context's workspace bytes and the screen's gate word with a table recorded on an MI355X.

Routes: the int8 tier (speculation on and off), the bf16 copy screen without the int8 tier (the copy is made by the first
search), the f32-stream screen (by mode and by an index without a copy), the exact and split scorers, one and eight queries with
a copy (screened) and without (GEMV), an unsupported dim, a bf16 corpus, a shard-sized corpus whose speculation takes the short
first chunk and one long launch, a corpus whose last screen chunk forks the BM25 leg in late, graph replay, and the four BM25
modes, also on an index without forward tokens (the scan mode falls back to the stream kernel there)."""
from typing import NamedTuple

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MI355X_CUS = 256          # what the recorded table assumes
VOCAB = 50
TAGS = ("cosine", "cosine_gated", "select", "spec", "rescreen", "rescore", "bm25", "rrf")
EXACT, SPLIT, SCREEN, SCREEN_COPY, SCREEN_STREAM = 0, 1, 2, 3, 4          # _lib.OI_COSINE_*
AUTO, NEVER = 0, 1                                                        # _lib.OI_SCREEN_COPY_*
STREAM, WAVE, TAAT, SCAN = 4, 3, 1, 2                                     # oi_index_set_bm25_mode


class Case(NamedTuple):
    name: str
    n: int
    dim: int = 768
    B: int = 64
    depth: int = 100
    mode: int = SCREEN
    policy: int = AUTO
    spec: bool = True
    graphs: bool = False
    bm25: int = 0             # 0: the index's default
    bf16: bool = False
    searches: int = 1
    empty_fwd: bool = False


CASES = [
    Case("i8-spec", 300_000),
    Case("i8-nospec", 300_000, spec=False),
    Case("i8-d384-depth1000", 300_000, dim=384, B=128, depth=1000),
    Case("i8-B9", 300_000, B=9),
    Case("copy-made-by-search", 300_000, mode=SCREEN_COPY, policy=NEVER, searches=2),
    Case("stream-mode", 300_000, mode=SCREEN_STREAM),
    Case("stream-no-copy", 300_000, policy=NEVER),
    Case("exact", 300_000, mode=EXACT),
    Case("split", 300_000, mode=SPLIT),
    Case("B1-copy", 300_000, B=1),
    Case("B8-copy", 300_000, B=8),
    Case("B1-gemv", 300_000, B=1, policy=NEVER),
    Case("B8-gemv", 300_000, B=8, policy=NEVER),
    Case("d1024-f32", 300_000, dim=1024),
    Case("bf16-corpus", 300_000, bf16=True),
    Case("shard-spec", 1_250_000),
    Case("late-fork-nospec", 2_000_000, spec=False),
    Case("graph-replay", 300_000, graphs=True, searches=2),
    Case("bm25-stream", 100_000, bm25=STREAM),
    Case("bm25-wave", 100_000, bm25=WAVE),
    Case("bm25-taat", 100_000, bm25=TAAT),
    Case("bm25-scan", 100_000, bm25=SCAN),
    Case("bm25-scan-no-tokens", 100_000, bm25=SCAN, empty_fwd=True),
    Case("bm25-wave-no-tokens", 100_000, bm25=WAVE, empty_fwd=True),
    Case("bm25-taat-no-tokens", 100_000, bm25=TAAT, empty_fwd=True),
]

# per case, per search: (launches of each of TAGS), (workspace bytes: device, host), screen_gate (-1: not screened) -- recorded on
# an MI355X
RECORDED = {
    "i8-spec": [((2, 1, 6, 1, 1, 1, 2, 1), (199862528, 208896), 0.0)],
    "i8-nospec": [((3, 1, 7, 0, 1, 1, 2, 1), (199862528, 208896), 0.0)],
    "i8-d384-depth1000": [((2, 1, 6, 1, 1, 1, 2, 1), (411096576, 212992), 0.0)],
    "i8-B9": [((2, 1, 6, 1, 1, 1, 2, 1), (28418560, 32768), 0.0)],
    "copy-made-by-search": [((2, 1, 5, 1, 0, 1, 2, 1), (178791680, 208896), 0.0), ((2, 1, 5, 1, 0, 1, 2, 1), (178791680, 208896), 0.0)],
    "stream-mode": [((2, 1, 5, 1, 0, 1, 2, 1), (178791680, 208896), 0.0)],
    "stream-no-copy": [((2, 1, 5, 1, 0, 1, 2, 1), (178791680, 208896), 0.0)],
    "exact": [((3, 0, 4, 0, 0, 0, 2, 1), (175973632, 208896), -1.0)],
    "split": [((3, 0, 4, 0, 0, 0, 2, 1), (176366848, 208896), -1.0)],
    "B1-copy": [((3, 1, 6, 0, 0, 1, 2, 1), (3013120, 8192), 0.0)],
    "B8-copy": [((3, 1, 6, 0, 0, 1, 2, 1), (22588928, 32768), 0.0)],
    "B1-gemv": [((3, 0, 4, 0, 0, 0, 2, 1), (2824704, 8192), -1.0)],
    "B8-gemv": [((3, 0, 4, 0, 0, 0, 2, 1), (22113792, 32768), -1.0)],
    "d1024-f32": [((3, 0, 4, 0, 0, 0, 2, 1), (176039168, 274432), -1.0)],
    "bf16-corpus": [((3, 0, 4, 0, 0, 0, 2, 1), (174695680, 208896), -1.0)],
    "shard-spec": [((2, 1, 6, 1, 1, 1, 2, 1), (691555840, 208896), 0.0)],
    "late-fork-nospec": [((4, 1, 8, 0, 1, 1, 2, 1), (1079753984, 208896), 0.0)],
    "graph-replay": [((3, 1, 7, 0, 1, 1, 2, 1), (199862528, 208896), 0.0), ((3, 1, 7, 0, 1, 1, 2, 1), (199862528, 208896), 0.0)],
    "bm25-stream": [((2, 1, 6, 1, 1, 1, 2, 1), (96367360, 208896), 0.0)],
    "bm25-wave": [((2, 1, 6, 1, 1, 1, 1, 1), (162679808, 208896), 0.0)],
    "bm25-taat": [((2, 1, 6, 1, 1, 1, 1, 1), (95199488, 208896), 0.0)],
    "bm25-scan": [((2, 1, 7, 1, 1, 1, 2, 1), (415913216, 208896), 0.0)],
    "bm25-scan-no-tokens": [((2, 1, 5, 1, 1, 1, 0, 1), (95045120, 208896), 0.0)],
    "bm25-wave-no-tokens": [((2, 1, 5, 1, 1, 1, 0, 1), (95045120, 208896), 0.0)],
    "bm25-taat-no-tokens": [((2, 1, 6, 1, 1, 1, 0, 1), (95199488, 208896), 0.0)],
}


def _data(case: Case):
    import torch
    g = torch.Generator(device="cuda").manual_seed(1000 + case.n % 997 + case.dim + case.B)
    rows = torch.randn(case.n, case.dim, device="cuda", generator=g, dtype=torch.float32)
    q = torch.randn(case.B, case.dim, device="cuda", generator=g, dtype=torch.float32)
    q = (q / q.norm(dim=1, keepdim=True)).cpu().numpy()
    rng = np.random.default_rng(case.n + case.B)
    if case.empty_fwd:
        terms, offs = np.zeros(1, dtype=np.uint32), np.zeros(case.n + 1, dtype=np.uint64)
    else:
        lens = rng.integers(1, 9, size=case.n)
        offs = np.zeros(case.n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(lens)
        terms = rng.integers(0, VOCAB, size=int(offs[-1])).astype(np.uint32)
    qo = np.arange(0, 2 * case.B + 1, 2, dtype=np.uint32)
    qt = rng.integers(0, VOCAB, size=2 * case.B).astype(np.uint32)
    return rows, q, terms, offs, qt, qo


def run_case(case: Case):
    """[(launches per tag, workspace_bytes, screen_gate) for each search] of one case on a fresh context."""
    import torch
    import openintel_amd as oi
    rows, q, terms, offs, qt, qo = _data(case)
    ctx = oi.HipContext(0)
    ctx.set_cosine_mode(case.mode)
    ctx.set_screen_speculation(case.spec)
    ctx.set_graph_replay(case.graphs)
    idx = oi.HybridIndex(ctx, case.n, case.dim, VOCAB)
    if case.bf16:
        rows = (rows / rows.norm(dim=1, keepdim=True)).to(torch.bfloat16).contiguous()
        idx.set_embeddings_bf16(rows)
    else:
        idx.set_embeddings(rows, normalize=True)
    idx.set_screen_copy(case.policy)
    if case.bm25:
        idx.set_bm25_mode(case.bm25)
    idx.set_forward(terms, offs)
    idx.finalize()
    out = []
    for _ in range(case.searches):
        ctx.profile_reset(True)
        idx.search(q, qt, qo, k=10, depth=case.depth)
        launches = tuple(int(ctx.profile_read(t)[1]) for t in TAGS)
        out.append((launches, tuple(ctx.workspace_bytes()), float(ctx.profile_read("screen_gate")[0])))
    ctx.profile_reset(False)
    idx.close()
    ctx.close()
    del rows
    torch.cuda.empty_cache()
    return out


@pytest.fixture(scope="module")
def num_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_search_launch_schedule(num_cus, case):
    if num_cus != MI355X_CUS:
        pytest.skip("the table was recorded on a %d-CU MI355X" % MI355X_CUS)
    got = run_case(case)
    want = RECORDED[case.name]
    assert len(got) == len(want)
    for i, ((launches, ws, gate), (w_launches, w_ws, w_gate)) in enumerate(zip(got, want)):
        assert dict(zip(TAGS, launches)) == dict(zip(TAGS, w_launches)), (case.name, i)
        assert ws == w_ws, (case.name, i)
        assert gate == w_gate, (case.name, i)
