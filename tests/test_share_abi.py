"""CPU-side checks of the similarity-share boundary (oi_similar_share): the header, the Python table, the Rust binding, the
argument checks that run before any device call, and batch.share_of_voice on hand-made records."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ARGS = 9


def _header_code():
    hdr = open(os.path.join(ROOT, "include", "openintel_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_function_and_states_the_contract():
    hdr, code = _header_code()
    m = re.search(r"\bint\s+oi_similar_share\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m and m.group(1).count(",") + 1 == N_ARGS
    args = " ".join(m.group(1).split())
    assert "const oi_summary_spec *spec" in args and "oi_social_counters *out" in args and "uint32_t *labels_out" in args
    assert not re.search(r"struct\s+\w*share\w*", code)                 # oi_summary_spec is reused: no new struct
    assert re.search(r"#define\s+OI_ABI_VERSION\s+1\b", code)

    def flat(t):
        return " ".join(t.replace(" *", " ").split())

    text = flat(hdr)
    for phrase in ("the CANDIDATES are the queries q for which clauses 1 and 3 of oi_similar_summary hold",
                   "d passes filters[q]. filters == NULL means every document passes.",
                   "sim(q, d) >= t_q, where t_q = thresholds[q], or spec->threshold when thresholds == NULL",
                   "A NaN t_q makes q nobody's candidate",
                   "A NaN similarity is never >=",
                   "The WINNER of d is the candidate with the largest sim(q, d), compared as the f32 values of the library's chain",
                   "Ties go to the smallest q",
                   "d is ASSIGNED when it has a winner and clause 2 holds",
                   "(evaluated in 64 bits)",
                   "out[q][b] holds the social_summary raw sums over the documents assigned to q in bucket b",
                   "polarity_sum = (double)(sum of pol_q30) * 2^-30",
                   "labels_out[d] is the winner of an assigned document and 0xFFFFFFFF for every other row",
                   "every document is in at most one cell",
                   "out[q][b].total <= oi_similar_summary's for the same arguments",
                   "summed over q, the totals equal the number of documents with at least one candidate and a bucket",
                   "with n_queries == 1 the records are oi_similar_summary's bit for bit",
                   "so are they with pairwise disjoint filters",
                   "a query that repeats an earlier one with the same threshold and filter gets all-zero records",
                   "deterministic and independent of the route, the order of the atomics, the cosine mode and the copy policy",
                   "unlike its siblings it DOES depend on the batch composition",
                   "within 1e-5 of each other, or of the threshold, may fall either way under the f32 chain",
                   "spec is always a host pointer",
                   "the filters, out and labels_out live",
                   "OI_DEVICE is asynchronous on the ctx stream",
                   "embeddings only",
                   "works on a view",
                   "n_queries == 0 is OI_OK",
                   "n_queries <= 4096",
                   "n_queries * n_buckets <= OI_MAX_SUMMARY_CELLS",
                   "not captured by graph replay",
                   "An index without signals -> OI_ERR_STATE",
                   "on an index without attributes -> OI_ERR_STATE",
                   "every argument check precedes the first device call",
                   "`best`, 8 B per local row (oi_workspace_bytes counts all of them)",
                   '"share" (the stream), "share_band" (rescoring and commit of the undecided rows), "share_exact"',
                   '"share_state" reads the band fill',
                   "NOT covered: oi_search_sharded* and oi_pipeline_*",
                   "exchange the per-row best key",
                   'The list of tags ends with those of oi_similar_share: "share", "share_band", "share_exact". /'):
        # (the END of the comment above oi_profile_reset: tests/test_summary_abi.py pins the bracket after "summary_exact")
        assert flat(phrase) in text, phrase


def test_python_table_and_rust_binding_match_the_header():
    from openintel_amd import _lib
    assert len(_lib.SIGNATURES["oi_similar_share"][1]) == N_ARGS
    assert _lib.SIGNATURES["oi_similar_share"][1][:8] == _lib.SIGNATURES["oi_similar_summary"][1]     # the summary's, then the labels
    src = re.sub(r"//.*", "", open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read())
    m = re.search(r"pub fn oi_similar_share\s*\(([^)]*)\)", src, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == N_ARGS
    assert "spec: *const OiSummarySpec" in m.group(1) and "labels_out: *mut u32" in m.group(1)
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    assert "fn similar_share" in lib_rs and "ffi::oi_similar_share" in lib_rs


def test_the_new_kernel_file_is_part_of_the_build():
    from openintel_amd import build
    assert "cosine_share.hip" in build.sources()


def test_python_wrappers_exist_with_the_documented_defaults():
    import inspect
    from openintel_amd import batch, retriever
    sig = inspect.signature(retriever.HybridIndex.similar_share)
    assert list(sig.parameters) == ["self", "query_vecs", "threshold", "n_buckets", "stamp_origin", "bucket_width", "filters", "labels"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["n_buckets"], d["stamp_origin"], d["bucket_width"], d["filters"], d["labels"]) == (1, 0, 0, None, False)
    assert list(inspect.signature(batch.share_of_voice).parameters) == ["records"]


def test_bad_arguments_are_refused_without_touching_a_device():
    import ctypes as C
    import numpy as np
    from openintel_amd import build, _lib
    build.build()
    lib = _lib.load()
    INVALID, HOST = _lib.OI_ERR_INVALID_ARG, _lib.OI_HOST
    none = C.c_void_p(None)
    buf = np.zeros(16, dtype=np.uint64)     # a real host buffer wherever one is required
    p = _lib.ptr(buf)
    nan = float("nan")

    def spec(t=0.5, origin=0, width=0, nb=1):
        return C.byref(_lib.SummarySpec(t, origin, width, nb))

    def refused(rc, word):
        msg = lib.oi_last_error()
        assert rc == INVALID and msg and word in msg, (rc, msg, word)

    # oi_similar_share(idx, query_vecs, n_queries, spec, thresholds, filters, location, out, labels_out)
    def call(n=1, sp=None, thr=none, qv=p, out=p, labels=p):
        return lib.oi_similar_share(none, qv, n, spec() if sp is None else sp, thr, none, HOST, out, labels)

    refused(call(), b"null index")
    refused(call(n=0), b"null index")
    refused(call(sp=none), b"null spec")
    refused(call(sp=spec(t=nan)), b"NaN")
    refused(call(sp=spec(t=nan), thr=p), b"null index")                     # a NaN spec with an array gets as far as the handle
    refused(call(sp=spec(t=float("inf"))), b"null index")
    refused(call(sp=spec(t=float("-inf"))), b"null index")
    refused(call(n=4097), b"n_queries=4097")
    refused(call(n=4096, sp=spec(width=1, nb=64)), b"null index")            # = 2^18 cells: allowed
    refused(call(n=4096, sp=spec(width=1, nb=65)), b"266240 cells")
    refused(call(sp=spec(nb=0)), b"n_buckets=0")
    refused(call(sp=spec(nb=2)), b"bucket_width=0")
    refused(call(out=none), b"null buffer")
    refused(call(qv=none), b"null buffer")
    refused(call(labels=none), b"null index")                               # labels_out may be NULL: on to the handle


def _records(rows):
    import numpy as np
    from openintel_amd.analyzer import COUNTERS_DTYPE
    rec = np.zeros((len(rows), len(rows[0])), dtype=COUNTERS_DTYPE)
    for q, row in enumerate(rows):
        for b, r in enumerate(row):
            rec[q, b] = r
    return rec


def test_share_of_voice_on_hand_made_records():
    from openintel_amd import batch
    from openintel_amd.engine import SpeculationEngine
    zero = (0, (0, 0), 0, 0, 0, 0, 0.0)
    # (total, by_source, bullish, bearish, neutral, spec_count, polarity_sum); bucket 1 is empty for every query
    rec = _records([[(6, (4, 2), 3, 1, 2, 3, 1.5), zero, (1, (1, 0), 0, 1, 0, 0, -1.0)],
                    [(2, (0, 2), 0, 2, 0, 1, -2.0), zero, (3, (3, 0), 3, 0, 0, 3, 3.0)],
                    [zero, zero, zero]])
    sov = batch.share_of_voice(rec)
    assert len(sov) == 3 and all(len(r) == 3 for r in sov)
    assert [[c.total for c in r] for r in sov] == [[6, 0, 1], [2, 0, 3], [0, 0, 0]]
    assert [[c.fraction for c in r] for r in sov] == [[0.75, 0.0, 0.25], [0.25, 0.0, 0.75], [0.0, 0.0, 0.0]]
    for b in (0, 2):
        assert sum(sov[q][b].fraction for q in range(3)) == 1.0
    for q in range(3):
        for b in range(3):
            assert sov[q][b].social == SpeculationEngine.social_from_counters(rec[q, b])
    s = sov[0][0].social
    assert (s.total_mentions, s.bullish, s.bearish, s.neutral) == (6, 3, 1, 2)
    assert float(s.net_sentiment) == 0.25 and float(s.speculation_index) == 0.5 and s.bull_bear_ratio == 3.0
    e = sov[2][1].social
    assert e.total_mentions == 0 and float(e.net_sentiment) == 0.0 and e.bull_bear_ratio is None
    assert batch.share_of_voice(rec[:0]) == []
