"""CPU-side checks of the similarity-summary boundary (oi_index_set_signals, oi_similar_summary): the header, the Python
table, the Rust binding, and the argument checks that run before any device call."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"oi_similar_summary": 8, "oi_index_set_signals": 6}


def _header_code():
    hdr = open(os.path.join(ROOT, "include", "openintel_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_functions_and_states_the_contract():
    hdr, code = _header_code()
    for name, n_args in CALLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n_args, name
    assert re.search(r"#define\s+OI_MAX_SUMMARY_CELLS\s+\(1u\s*<<\s*18\)", code)
    m = re.search(r"typedef\s+struct\s+oi_summary_spec\s*\{(.*?)\}\s*oi_summary_spec\s*;", code, flags=re.S)
    assert m, "oi_summary_spec"
    fields = re.findall(r"\b(float|uint32_t)\s+(\w+)\s*;", m.group(1))
    assert fields == [("float", "threshold"), ("uint32_t", "stamp_origin"), ("uint32_t", "bucket_width"), ("uint32_t", "n_buckets")]
    assert re.search(r"#define\s+OI_ABI_VERSION\s+1\b", code)

    def flat(t):                                    # (the comment's line starts go, and with them every " *" of a formula)
        return " ".join(t.replace(" *", " ").split())

    text = flat(hdr)
    for phrase in ("NaN -> 0, clamped to [-1, 1]",
                   "pol_q30 = (int32) rint(v * 2^30), f64 round-to-nearest-even (the product is exact in f64)",
                   "bullish if v > bull_bear_threshold, bearish if v < -bull_bear_threshold, else neutral",
                   "The class is fixed at set time",
                   "allocated by the first call, never reallocated and overwritten in place",
                   "views alias it and see updates; a view made before signals existed has none; on a view: OI_ERR_STATE",
                   "8 B per row",
                   "out[q][b] holds the social_summary raw sums over the local documents d of the handle",
                   "d passes filters[q]. filters == NULL means every document passes.",
                   "bucket_width == 0, or stamp_origin <= stamp[d] and (stamp[d] - stamp_origin) / bucket_width == b",
                   "sim(q, d) >= t_q, where t_q = thresholds[q], or spec->threshold when thresholds == NULL",
                   "A NaN thresholds[q] counts nothing for that query, in both locations",
                   "total, by_source[2], bullish, bearish, neutral and spec_count are exact integers",
                   "polarity_sum = (double)(sum of pol_q30) * 2^-30, the sum taken in 64-bit integers",
                   "deterministic and independent of the route, the order of the atomics, the cosine mode, the copy policy and the batch composition",
                   "polarity_sum is an integer multiple of 2^-30",
                   "|polarity_sum - sum of Polarity::new(polarity[d])| <= total * 2^-31",
                   "the sum is exact when every polarity is dyadic",
                   "sums of shards add exactly below 2^23 in magnitude",
                   "spec is always a host pointer",
                   "OI_DEVICE is asynchronous on the ctx stream",
                   "works on a view",
                   "n_queries == 0 is OI_OK",
                   "not captured by graph replay",
                   "n_queries * n_buckets > OI_MAX_SUMMARY_CELLS -> OI_ERR_INVALID_ARG",
                   "an index without signals -> OI_ERR_STATE",
                   "oi_search_sharded* and oi_pipeline_*",
                   "A sharded host adds the records",
                   '"summary", "summary_band", "summary_exact"). oi_profile_read'):
        assert flat(phrase) in text, phrase


def test_python_table_and_rust_binding_have_matching_argument_counts():
    import ctypes as C
    from openintel_amd import _lib
    assert _lib.OI_MAX_SUMMARY_CELLS == 1 << 18
    assert C.sizeof(_lib.SummarySpec) == 16
    assert [f[0] for f in _lib.SummarySpec._fields_] == ["threshold", "stamp_origin", "bucket_width", "n_buckets"]
    assert C.sizeof(_lib.SocialCounters) == 64
    src = open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read()
    src = re.sub(r"//.*", "", src)
    for name, n_args in CALLS.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
        m = re.search(r"pub fn " + name + r"\s*\(([^)]*)\)", src, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args, name
    m = re.search(r"pub struct OiSummarySpec\s*\{(.*?)\}", src, flags=re.S)
    assert m and re.findall(r"pub (\w+): (\w+)", m.group(1)) == [("threshold", "f32"), ("stamp_origin", "u32"),
                                                                  ("bucket_width", "u32"), ("n_buckets", "u32")]
    assert re.search(r"pub const OI_MAX_SUMMARY_CELLS: u32 = 1 << 18;", src)
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    assert "fn similar_summary" in lib_rs and "ffi::oi_similar_summary" in lib_rs
    assert "fn set_signals" in lib_rs and "ffi::oi_index_set_signals" in lib_rs


def test_python_wrappers_exist_with_the_documented_defaults():
    import inspect
    from openintel_amd import engine, retriever
    H = retriever.HybridIndex
    sig = inspect.signature(H.similar_summary)
    assert list(sig.parameters) == ["self", "query_vecs", "threshold", "n_buckets", "stamp_origin", "bucket_width", "filters"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["n_buckets"], d["stamp_origin"], d["bucket_width"], d["filters"]) == (1, 0, 0, None)
    sig = inspect.signature(H.set_signals)
    assert list(sig.parameters) == ["self", "polarity", "speculative", "sources", "bull_bear_threshold"]
    assert (sig.parameters["sources"].default, sig.parameters["bull_bear_threshold"].default) == (None, 0.2)
    sig = inspect.signature(H.set_signals_from_text)
    assert list(sig.parameters) == ["self", "texts", "sources", "bull_bear_threshold"]
    assert (sig.parameters["sources"].default, sig.parameters["bull_bear_threshold"].default) == (None, 0.2)
    assert list(inspect.signature(engine.SpeculationEngine.social_from_counters).parameters) == ["record"]


def test_social_from_counters_finishes_a_record_like_the_reference():
    import numpy as np
    from openintel_amd.analyzer import COUNTERS_DTYPE
    from openintel_amd.domain import SourceKind
    from openintel_amd.engine import SpeculationEngine
    rec = np.zeros(2, dtype=COUNTERS_DTYPE)
    rec[0] = (10, (4, 6), 7, 2, 1, 3, 5.0)
    s = SpeculationEngine.social_from_counters(rec[0])
    assert (s.total_mentions, s.bullish, s.bearish, s.neutral) == (10, 7, 2, 1)
    assert {int(k): v for k, v in s.mentions_by_source.items()} == {int(SourceKind.ALL[0]): 4, int(SourceKind.ALL[1]): 6}
    assert (float(s.net_sentiment), float(s.speculation_index), s.bull_bear_ratio) == (0.5, 0.3, 3.5)
    e = SpeculationEngine.social_from_counters(rec[1])              # an empty cell: the reference's zero-post summary
    assert (e.total_mentions, float(e.net_sentiment), float(e.speculation_index), e.bull_bear_ratio) == (0, 0.0, 0.0, None)
    assert e.mentions_by_source == {}


def test_the_new_kernel_file_is_part_of_the_build():
    from openintel_amd import build
    assert "cosine_summary.hip" in build.sources()


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

    # oi_similar_summary(idx, query_vecs, n_queries, spec, thresholds, filters, location, out)
    refused(lib.oi_similar_summary(none, p, 1, spec(), none, none, HOST, p), b"null index")
    refused(lib.oi_similar_summary(none, p, 0, spec(), none, none, HOST, p), b"null index")
    refused(lib.oi_similar_summary(none, p, 1, none, none, none, HOST, p), b"null spec")
    refused(lib.oi_similar_summary(none, p, 1, spec(t=nan), none, none, HOST, p), b"NaN")
    refused(lib.oi_similar_summary(none, p, 1, spec(width=1, nb=0), none, none, HOST, p), b"n_buckets=0")
    refused(lib.oi_similar_summary(none, p, 1, spec(width=1, nb=1025), none, none, HOST, p), b"n_buckets=1025")
    refused(lib.oi_similar_summary(none, p, 1, spec(width=0, nb=2), none, none, HOST, p), b"bucket_width=0")
    refused(lib.oi_similar_summary(none, p, 4097, spec(), none, none, HOST, p), b"n_queries=4097")
    refused(lib.oi_similar_summary(none, p, 4096, spec(width=1, nb=65), none, none, HOST, p), b"266240 cells")   # > 2^18
    refused(lib.oi_similar_summary(none, p, 4096, spec(width=1, nb=64), none, none, HOST, p), b"null index")     # = 2^18: allowed
    refused(lib.oi_similar_summary(none, p, 1, spec(), none, none, HOST, none), b"null buffer")
    refused(lib.oi_similar_summary(none, none, 1, spec(), none, none, HOST, p), b"null buffer")
    # +-inf are thresholds like any other, and a NaN spec.threshold is not read when the call brings a thresholds array: with
    # them the call gets as far as the handle
    refused(lib.oi_similar_summary(none, p, 1, spec(t=float("inf")), none, none, HOST, p), b"null index")
    refused(lib.oi_similar_summary(none, p, 1, spec(t=float("-inf"), width=3600, nb=1024), none, none, HOST, p), b"null index")
    refused(lib.oi_similar_summary(none, p, 1, spec(t=nan), p, none, HOST, p), b"null index")

    # oi_index_set_signals(idx, polarity, speculative, sources, bull_bear_threshold, location)
    refused(lib.oi_index_set_signals(none, p, p, none, 0.2, HOST), b"null index")
    refused(lib.oi_index_set_signals(none, p, p, p, nan, HOST), b"bull_bear_threshold is NaN")
    refused(lib.oi_index_set_signals(none, none, p, p, 0.2, HOST), b"null buffer (polarity)")
    refused(lib.oi_index_set_signals(none, p, none, p, 0.2, HOST), b"null buffer (speculative)")
    refused(lib.oi_index_set_signals(none, p, p, none, 0.2, 7), b"bad location 7")
