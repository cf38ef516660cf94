"""CPU-side checks of the mention-summary boundary (oi_mention_summary): the header, the Python table, the Rust binding, the
wrappers, the build, the argument checks that run before any device call, and compare_mentions' host ranking."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"oi_mention_summary": 9}
SPEC_FIELDS = ["axis", "stamp_origin", "bucket_width", "n_cells"]


def _header_code():
    hdr = open(os.path.join(ROOT, "include", "openintel_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_function_and_states_the_contract():
    hdr, code = _header_code()
    for name, n_args in CALLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n_args, name
    assert re.search(r"#define\s+OI_MAX_MENTION_TERMS\s+64u", code)
    assert re.search(r"enum\s*\{\s*OI_MENTION_AXIS_TIME\s*=\s*0\s*,\s*OI_MENTION_AXIS_KEY\s*=\s*1\s*\}", code)
    m = re.search(r"typedef\s+struct\s+oi_mention_spec\s*\{(.*?)\}\s*oi_mention_spec\s*;", code, flags=re.S)
    assert m, "oi_mention_spec"
    assert re.findall(r"\b(uint32_t)\s+(\w+)\s*;", m.group(1)) == [("uint32_t", f) for f in SPEC_FIELDS]
    assert re.search(r"#define\s+OI_ABI_VERSION\s+1\b", code)

    def flat(t):                                    # (the comment's line starts go, and with them every " *" of a formula)
        return " ".join(t.replace(" *", " ").split())

    text = flat(hdr)
    for phrase in ("D_q is the set of DISTINCT term ids in query_terms[q_term_offsets[q] .. q_term_offsets[q+1])",
                   "A repeated term counts once -- unlike BM25, where it counts each time",
                   "A term id >= vocab occurs in no document, but it is a member of D_q",
                   "m(q, d) is the number of t in D_q with a posting for local document d",
                   "min_match == NULL gives 1 (ANY); min_match[q] == 0 gives |D_q| (ALL); otherwise it is min_match[q]",
                   "d MATCHES q when |D_q| >= 1 and m(q, d) >= need_q",
                   "An empty query matches nothing; need_q > |D_q| matches nothing",
                   "out[q][c] holds the social_summary raw sums over the local documents d of the handle that match q, pass filters[q] and fall into cell c",
                   "the pass clause is oi_similar_summary's clause 1",
                   "on the TIME axis the cell is oi_similar_summary's clause 2",
                   "on the KEY axis the cell is oi_similar_groups's key clause: (group[d] & key_mask) >> ctz(key_mask) == c, and a key >= n_cells belongs to no cell",
                   "total, by_source[2], bullish, bearish, neutral and spec_count are exact integers",
                   "polarity_sum = (double)(sum of pol_q30) * 2^-30, the sum taken in 64-bit integers",
                   "deterministic and independent of the order of the atomics, the grid and the batch composition",
                   "with one term, no filter and one cell, total equals the term's local df (oi_index_local_stats)",
                   "with min_match == NULL the matching set of a query equals the set of documents with BM25 score > 0 for it (every idf is > 0)",
                   "records of document shards add",
                   "At most OI_MAX_MENTION_TERMS raw terms per query, duplicates included",
                   "With OI_HOST a longer query is OI_ERR_INVALID_ARG, naming the query and the count",
                   "With OI_DEVICE the offsets are not host-visible: such a query gets all-zero records, and nothing is read or written out of bounds",
                   "n_queries <= 4096; n_queries * n_cells <= OI_MAX_GROUP_CELLS; n_queries == 0 is OI_OK",
                   "spec is always a host pointer",
                   "OI_DEVICE is asynchronous on the ctx stream; not captured by graph replay",
                   "A finalized index is required (the postings), and signals (oi_index_set_signals): otherwise OI_ERR_STATE",
                   "Doc attributes are required when bucket_width > 0, when filters != NULL, or on the KEY axis: otherwise OI_ERR_STATE",
                   "NO embeddings are needed",
                   "It works on a view",
                   "every argument check precedes the first device call",
                   "64 B per cell and the per-query plan, 272 B per query (oi_workspace_bytes counts both)",
                   '"mention_plan"', '"mention"',
                   "oi_search_sharded* and oi_pipeline_*",
                   "A sharded host adds the records"):
        assert flat(phrase) in text, phrase


def test_python_table_and_rust_binding_have_matching_argument_counts():
    import ctypes as C
    from openintel_amd import _lib
    assert _lib.OI_MAX_MENTION_TERMS == 64
    assert (_lib.OI_MENTION_AXIS_TIME, _lib.OI_MENTION_AXIS_KEY) == (0, 1)
    assert C.sizeof(_lib.MentionSpec) == 16
    assert [f[0] for f in _lib.MentionSpec._fields_] == SPEC_FIELDS
    src = open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read()
    src = re.sub(r"//.*", "", src)
    for name, n_args in CALLS.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
        m = re.search(r"pub fn " + name + r"\s*\(([^)]*)\)", src, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args, name
    m = re.search(r"pub struct OiMentionSpec\s*\{(.*?)\}", src, flags=re.S)
    assert m and re.findall(r"pub (\w+): (\w+)", m.group(1)) == [(f, "u32") for f in SPEC_FIELDS]
    assert re.search(r"pub const OI_MAX_MENTION_TERMS: u32 = 64;", src)
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    assert "fn mention_summary" in lib_rs and "ffi::oi_mention_summary" in lib_rs
    assert "oi_mention_summary(" in open(os.path.join(ROOT, "integration", "c", "abi_check.c")).read()


def test_python_wrappers_exist_with_the_documented_defaults():
    import inspect
    from openintel_amd import batch, retriever
    H = retriever.HybridIndex
    sig = inspect.signature(H.mention_summary)
    assert list(sig.parameters) == ["self", "query_terms", "q_term_offsets", "min_match", "n_buckets", "stamp_origin", "bucket_width",
                                    "filters"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["min_match"], d["n_buckets"], d["stamp_origin"], d["bucket_width"], d["filters"]) == (None, 1, 0, 0, None)
    sig = inspect.signature(H.mention_groups)
    assert list(sig.parameters) == ["self", "query_terms", "q_term_offsets", "key_mask", "n_keys", "min_match", "filters"]
    assert (sig.parameters["min_match"].default, sig.parameters["filters"].default) == (None, None)
    sig = inspect.signature(H.mention_summary_text)
    assert list(sig.parameters) == ["self", "texts", "min_match", "n_buckets", "stamp_origin", "bucket_width", "filters"]
    sig = inspect.signature(H.mention_groups_text)
    assert list(sig.parameters) == ["self", "texts", "key_mask", "n_keys", "min_match", "filters"]
    sig = inspect.signature(batch.compare_mentions)
    assert list(sig.parameters)[:9] == ["index", "text", "tickers", "key_mask", "rank_by", "top", "min_total", "min_match", "filters"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["rank_by"], d["top"], d["min_total"], d["min_match"], d["filters"]) == (batch.RankBy.CROWDING, 100, None, None, None)


def test_the_new_kernel_file_is_part_of_the_build():
    from openintel_amd import build
    assert "mention.hip" in build.sources()


def test_bad_arguments_are_refused_without_touching_a_device():
    import ctypes as C
    import numpy as np
    from openintel_amd import build, _lib
    build.build()
    lib = _lib.load()
    INVALID, HOST, DEVICE = _lib.OI_ERR_INVALID_ARG, _lib.OI_HOST, _lib.OI_DEVICE
    TIME, KEY = _lib.OI_MENTION_AXIS_TIME, _lib.OI_MENTION_AXIS_KEY
    none = C.c_void_p(None)
    offs = np.zeros(4098, dtype=np.uint32)          # real host buffers wherever one is required: 4097 empty queries at the most
    terms = np.zeros(128, dtype=np.uint32)
    p, po = _lib.ptr(terms), _lib.ptr(offs)

    def spec(axis=TIME, origin=0, width=0, n=1):
        return C.byref(_lib.MentionSpec(axis, origin, width, n))

    def refused(rc, word):
        msg = lib.oi_last_error()
        assert rc == INVALID and msg and word in msg, (rc, msg, word)

    # oi_mention_summary(idx, query_terms, q_term_offsets, n_queries, spec, min_match, filters, location, out)
    def call(sp, nq=1, qt=p, qo=po, loc=HOST, out=p):
        return lib.oi_mention_summary(none, qt, qo, nq, sp, none, none, loc, out)

    refused(call(spec()), b"null index")
    refused(call(spec(), nq=0), b"null index")
    refused(call(none), b"null spec")
    refused(call(spec(axis=2)), b"axis=2")
    refused(call(spec(width=1, n=0)), b"n_cells=0")
    refused(call(spec(width=1, n=1025)), b"n_cells=1025")
    refused(call(spec(width=1, n=1024)), b"null index")                       # the largest time axis: allowed
    refused(call(spec(width=0, n=2)), b"bucket_width=0")
    refused(call(spec(axis=KEY, origin=0, n=1)), b"key_mask=0x0")
    refused(call(spec(axis=KEY, origin=0xF0F, n=1)), b"key_mask=0xf0f")
    refused(call(spec(axis=KEY, origin=0xFF, width=3600, n=1)), b"bucket_width=3600")
    refused(call(spec(axis=KEY, origin=0xFF, n=0)), b"n_cells=0")
    refused(call(spec(axis=KEY, origin=0xFF, n=257)), b"n_cells=257")           # more keys than the mask has values
    refused(call(spec(axis=KEY, origin=0xFFFFF, n=65537)), b"n_cells=65537")    # more than OI_MAX_GROUP_KEYS
    refused(call(spec(axis=KEY, origin=0xFF00, n=256)), b"null index")
    refused(call(spec(), nq=4097), b"n_queries=4097")
    refused(call(spec(axis=KEY, origin=0xFFFF, n=257), nq=4096), b"1052672 cells")   # > 2^20
    refused(call(spec(axis=KEY, origin=0xFFFF, n=256), nq=4096), b"null index")      # = 2^20: allowed
    refused(call(spec(), qt=none), b"null buffer")
    refused(call(spec(), qo=none), b"null buffer")
    refused(call(spec(), out=none), b"null buffer")
    refused(call(spec(), loc=7), b"bad location 7")
    long_offs = np.array([0, 3, 68, 70], dtype=np.uint32)                        # query 1 has 65 raw terms
    refused(call(spec(), nq=3, qo=_lib.ptr(long_offs)), b"query 1 has 65 terms")
    long_offs[2] = 67                                                            # 64: allowed
    refused(call(spec(), nq=3, qo=_lib.ptr(long_offs)), b"null index")
    refused(call(spec(), nq=3, qo=_lib.ptr(long_offs), loc=DEVICE), b"null index")   # (device offsets are never read by the host)


class _Stub:
    """An index whose one dense mention_groups_text call returns hand-made records."""

    def __init__(self, totals):
        import numpy as np
        from openintel_amd.analyzer import COUNTERS_DTYPE
        self.rec = np.zeros((1, len(totals)), dtype=COUNTERS_DTYPE)
        for k, t in enumerate(totals):
            self.rec[0, k] = (t, (t, 0), t, 0, 0, 0, 0.5 * t)
        self.calls = []

    def mention_groups_text(self, texts, key_mask, n_keys, min_match=None, filters=None):
        self.calls.append((list(texts), key_mask, n_keys, min_match, filters))
        return self.rec[:, :n_keys]


def test_compare_mentions_ranks_the_dense_records_on_the_host(monkeypatch):
    from openintel_amd import batch
    names = ["AAA", "BBB", "CCC", "DDD", "EEE", "FFF"]
    seen = {}

    def fake_rank(keys, records, count, tickers, rank_by, market_by_ticker=None, now=None, cfg=None):
        seen["keys"], seen["totals"], seen["count"] = list(keys), [int(r["total"]) for r in records], count
        return "ranked"

    monkeypatch.setattr(batch, "rank_group_records", fake_rank)
    stub = _Stub([5, 9, 0, 9, 1, 30])
    assert batch.compare_mentions(stub, "gme squeeze", names, 0xFF, min_total=1, min_match="all") == "ranked"
    assert stub.calls == [(["gme squeeze"], 0xFF, 6, "all", None)]                # one call, n_keys = the number of names
    assert (seen["keys"], seen["totals"], seen["count"]) == ([5, 1, 3, 0, 4], [30, 9, 9, 5, 1], 5)   # total desc, key asc; 0 left out
    batch.compare_mentions(stub, "gme", names, 0xFF, min_total=9)
    assert seen["keys"] == [5, 1, 3]
    batch.compare_mentions(stub, "gme", names, 0xFF, min_total=0, top=2)          # the bar is max(min_total, 1); cut at top
    assert seen["keys"] == [5, 1]
    batch.compare_mentions(stub, "gme", names, 0xFF)                              # default bar: cfg.min_sample
    assert seen["keys"] == [k for k in [5, 1, 3, 0, 4] if stub.rec[0, k]["total"] >= batch.EngineConfig().min_sample]


def test_compare_mentions_gives_a_compare_output():
    from openintel_amd import batch
    out = batch.compare_mentions(_Stub([5, 9, 0, 9]), "gme", ["AAA", "BBB", "CCC", "DDD"], 0xFF, min_total=1)
    assert isinstance(out, batch.CompareOutput) and not out.errors and out.rank_by == batch.RankBy.CROWDING
    assert sorted(e.ticker for e in out.ranked) == ["AAA", "BBB", "DDD"]                       # CCC has no post
    assert {e.ticker: e.report.social.total_mentions for e in out.ranked} == {"AAA": 5, "BBB": 9, "DDD": 9}
