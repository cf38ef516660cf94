"""CPU-side checks of the similarity-leaderboard boundary (oi_similar_groups): the header, the Python table, the Rust binding,
the argument checks that run before any device call, and the host ranking of batch.rank_group_records."""
import datetime as dt
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ARGS = 11
FIELDS = ["threshold", "key_mask", "n_keys", "top", "rank_by", "min_total"]


def _header_code():
    hdr = open(os.path.join(ROOT, "include", "openintel_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_function_and_states_the_contract():
    hdr, code = _header_code()
    m = re.search(r"\bint\s+oi_similar_groups\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m and m.group(1).count(",") + 1 == N_ARGS
    assert re.search(r"#define\s+OI_MAX_GROUP_KEYS\s+65536u", code)
    assert re.search(r"#define\s+OI_MAX_GROUP_CELLS\s+\(1u\s*<<\s*20\)", code)
    assert re.search(r"enum\s*\{\s*OI_GROUP_RANK_TOTAL\s*=\s*0,\s*OI_GROUP_RANK_SPEC\s*=\s*1,\s*OI_GROUP_RANK_BULLISH\s*=\s*2,\s*"
                     r"OI_GROUP_RANK_BEARISH\s*=\s*3\s*\}", code)
    m = re.search(r"typedef\s+struct\s+oi_groups_spec\s*\{(.*?)\}\s*oi_groups_spec\s*;", code, flags=re.S)
    assert m, "oi_groups_spec"
    assert re.findall(r"\b(float|uint32_t)\s+(\w+)\s*;", m.group(1)) == [("float", FIELDS[0])] + [("uint32_t", f) for f in FIELDS[1:]]
    assert re.search(r"#define\s+OI_ABI_VERSION\s+1\b", code)

    def flat(t):
        return " ".join(t.replace(" *", " ").split())

    text = flat(hdr)
    for phrase in ("key(d) = (group[d] & key_mask) >> ctz(key_mask)",
                   "key_mask is non-zero and one contiguous run of bits",
                   "whose key is >= n_keys belongs to no cell, like a stamp outside every bucket",
                   'word for word the clauses of oi_similar_summary, with "bucket" replaced by "key"',
                   "d passes filters[q]. filters == NULL means every document passes. A time window is expressed here",
                   "key(d) == key.",
                   "sim(q, d) >= t_q, where t_q = thresholds[q], or spec->threshold when thresholds == NULL",
                   "polarity_sum = (double)(sum of pol_q30) * 2^-30, the sum taken in 64-bit integers",
                   "deterministic and independent of the route, the order of the atomics, the cosine mode, the copy policy and the batch composition",
                   "Dense output (top == 0). records_out[q][key] for key < n_keys; keys_out, counts_out and qualified_out are not written and may be NULL",
                   "is its record's total, spec_count, bullish or bearish, chosen by rank_by",
                   "those with total >= max(min_total, 1), ordered by (v descending, key ascending) and cut at top",
                   "v << 32 | ~key",
                   "keys_out[q][r] and records_out[q][r] have row stride top",
                   "counts_out[q] is the number listed; qualified_out[q] (may be NULL) is the number of keys that qualified before the cut",
                   "Entries past counts_out[q] are key 0xFFFFFFFF and an all-zero record",
                   "spec is always a host pointer",
                   "OI_DEVICE is asynchronous on the ctx stream",
                   "works on a view",
                   "n_queries == 0 is OI_OK",
                   "not captured by graph replay",
                   "An index without signals, or without doc attributes (the key axis always needs them), -> OI_ERR_STATE",
                   "OI_MAX_GROUP_CELLS, a bad key_mask, n_keys, top or rank_by, a null required buffer -> OI_ERR_INVALID_ARG",
                   "every argument check precedes the first device call",
                   "NOT covered: oi_search_sharded* and oi_pipeline_*. Records of shards add",
                   "ranked lists of shards cannot be merged exactly",
                   '"text_emit", "groups", "groups_band", "groups_exact", "groups_rank", "volume"'):     # the list at oi_profile_reset
        assert flat(phrase) in text, phrase


def test_python_table_and_rust_binding_match_the_header():
    import ctypes as C
    from openintel_amd import _lib
    assert (_lib.OI_MAX_GROUP_KEYS, _lib.OI_MAX_GROUP_CELLS) == (65536, 1 << 20)
    assert (_lib.OI_GROUP_RANK_TOTAL, _lib.OI_GROUP_RANK_SPEC, _lib.OI_GROUP_RANK_BULLISH, _lib.OI_GROUP_RANK_BEARISH) == (0, 1, 2, 3)
    assert C.sizeof(_lib.GroupsSpec) == 24
    assert [f[0] for f in _lib.GroupsSpec._fields_] == FIELDS
    assert [getattr(_lib.GroupsSpec, f).offset for f in FIELDS] == [0, 4, 8, 12, 16, 20]
    assert len(_lib.SIGNATURES["oi_similar_groups"][1]) == N_ARGS
    src = re.sub(r"//.*", "", open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read())
    m = re.search(r"pub fn oi_similar_groups\s*\(([^)]*)\)", src, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == N_ARGS
    m = re.search(r"pub struct OiGroupsSpec\s*\{(.*?)\}", src, flags=re.S)
    assert m and re.findall(r"pub (\w+): (\w+)", m.group(1)) == [(FIELDS[0], "f32")] + [(f, "u32") for f in FIELDS[1:]]
    assert re.search(r"pub const OI_MAX_GROUP_KEYS: u32 = 65536;", src) and re.search(r"pub const OI_MAX_GROUP_CELLS: u32 = 1 << 20;", src)
    for i, name in enumerate(("TOTAL", "SPEC", "BULLISH", "BEARISH")):
        assert re.search(r"pub const OI_GROUP_RANK_%s: u32 = %d;" % (name, i), src)
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    assert "fn similar_groups" in lib_rs and "ffi::oi_similar_groups" in lib_rs
    abi_c = open(os.path.join(ROOT, "integration", "c", "abi_check.c")).read()
    assert "sizeof(oi_groups_spec) != 24" in abi_c and all("offsetof(oi_groups_spec, %s)" % f in abi_c for f in FIELDS)


def test_the_new_kernel_file_is_part_of_the_build():
    from openintel_amd import build
    assert "cosine_groups.hip" in build.sources()


def test_python_wrappers_exist_with_the_documented_defaults():
    import inspect
    from openintel_amd import batch, retriever
    from openintel_amd.domain import EngineConfig
    sig = inspect.signature(retriever.HybridIndex.similar_groups)
    assert list(sig.parameters) == ["self", "query_vecs", "threshold", "key_mask", "n_keys", "top", "rank_by", "min_total", "filters"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["top"], d["rank_by"], d["min_total"], d["filters"]) == (0, "total", 0, None)
    assert [f.name for f in retriever.GroupRanking.__dataclass_fields__.values()] == ["keys", "records", "counts", "qualified"]
    sig = inspect.signature(batch.rank_group_records)
    assert list(sig.parameters) == ["keys", "records", "count", "tickers", "rank_by", "market_by_ticker", "now", "cfg"]
    assert sig.parameters["market_by_ticker"].default is None and sig.parameters["now"].default is None
    assert sig.parameters["cfg"].default == EngineConfig()
    sig = inspect.signature(batch.compare_index)
    assert list(sig.parameters)[:9] == ["index", "query_vec", "threshold", "tickers", "key_mask", "rank_by", "top", "min_total", "filters"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["rank_by"], d["top"], d["min_total"], d["filters"]) == (batch.RankBy.CROWDING, 100, None, None)


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

    def spec(t=0.5, mask=0xFF, nk=4, top=0, by=0, mt=0):
        return C.byref(_lib.GroupsSpec(t, mask, nk, top, by, mt))

    def refused(rc, word):
        msg = lib.oi_last_error()
        assert rc == INVALID and msg and word in msg, (rc, msg, word)

    # oi_similar_groups(idx, query_vecs, n_queries, spec, thresholds, filters, location, records_out, keys_out, counts_out, qualified_out)
    def call(n=1, sp=None, thr=none, qv=p, rec=p, keys=p, counts=p, qual=p):
        return lib.oi_similar_groups(none, qv, n, spec() if sp is None else sp, thr, none, HOST, rec, keys, counts, qual)

    refused(call(), b"null index")
    refused(call(n=0), b"null index")
    refused(call(sp=none), b"null spec")
    refused(call(sp=spec(t=nan)), b"NaN")
    refused(call(sp=spec(t=nan), thr=p), b"null index")                     # a NaN spec with an array gets as far as the handle
    refused(call(sp=spec(t=float("inf"))), b"null index")
    refused(call(sp=spec(t=float("-inf"), top=1024, by=3, mt=7)), b"null index")
    refused(call(sp=spec(mask=0)), b"key_mask=0x0")
    refused(call(sp=spec(mask=0x5)), b"key_mask=0x5")
    refused(call(sp=spec(mask=0xFFFFFFFF, nk=65536)), b"null index")          # the full word is one run
    refused(call(sp=spec(mask=0x80000000, nk=2)), b"null index")
    refused(call(sp=spec(nk=0)), b"n_keys=0")
    refused(call(sp=spec(mask=0x7, nk=9)), b"n_keys=9")
    refused(call(sp=spec(mask=0x7, nk=8)), b"null index")
    refused(call(sp=spec(mask=0xFFFFFFFF, nk=65537)), b"n_keys=65537")
    refused(call(sp=spec(top=1025)), b"top=1025")
    refused(call(sp=spec(by=4)), b"rank_by=4")
    refused(call(n=4097), b"n_queries=4097")
    refused(call(n=17, sp=spec(mask=0xFFFF0000, nk=65536)), b"1114112 cells")
    refused(call(n=16, sp=spec(mask=0xFFFF0000, nk=65536)), b"null index")    # = 2^20: allowed
    refused(call(rec=none), b"null buffer")
    refused(call(qv=none), b"null buffer")
    refused(call(sp=spec(top=1), keys=none), b"null buffer")
    refused(call(sp=spec(top=1), counts=none), b"null buffer")
    refused(call(sp=spec(top=1), qual=none), b"null index")                   # qualified_out may be NULL
    refused(call(keys=none, counts=none, qual=none), b"null index")          # dense: only the records are required


# ------------------------------------------------------------------ the host ranking
def _golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "reference_fixture.json")))


def _records(rows):
    import numpy as np
    from openintel_amd.analyzer import COUNTERS_DTYPE
    rec = np.zeros(len(rows), dtype=COUNTERS_DTYPE)
    for i, r in enumerate(rows):
        rec[i] = r
    return rec


def test_rank_group_records_reproduces_the_reference_fixture():
    import numpy as np
    from openintel_amd import batch
    from openintel_amd.domain import MarketSnapshot, Ticker
    g = _golden()
    m = g["mock_market"]
    snap = MarketSnapshot(Ticker.parse("AAPL"), m["last_price"], m["previous_close"], m["volume"], m["avg_volume"],
                          m["realized_vol"], m["put_call_ratio"], m["iv_rank"])
    rec = _records([(10, (4, 6), 7, 2, 1, 3, 5.0)])
    now = dt.datetime(2026, 6, 24, 20, 0, 0, tzinfo=dt.timezone.utc)
    out = batch.rank_group_records(np.array([3], np.uint32), rec, 1, ["A", "B", "C", "AAPL"], batch.RankBy.CROWDING,
                                   market_by_ticker={"AAPL": snap}, now=now)
    assert not out.errors and [r.ticker for r in out.ranked] == ["AAPL"] and "Not financial advice" in out.disclaimer
    rep, d = out.ranked[0].report, g["derived"]["summary"]
    so = rep.social
    assert so.total_mentions == d["total_mentions"] and (so.bullish, so.bearish, so.neutral) == (d["bullish"], d["bearish"], d["neutral"])
    assert {k.as_str(): v for k, v in so.mentions_by_source.items()} == d["mentions_by_source"]
    assert float(so.net_sentiment) == d["net_sentiment"] and float(so.speculation_index) == d["speculation_index"]
    assert so.bull_bear_ratio == d["bull_bear_ratio"]
    assert rep.market.pct_change == d["pct_change"] and rep.market.rvol == d["rvol"]
    assert rep.fusion.crowding == d["crowding"] == out.ranked[0].rank_metric
    assert rep.fusion.alignment.value == d["alignment"] and rep.social_confidence.value == d["social_confidence"]
    assert batch.summarize(rep) == "AAPL — ConfirmingBullish · crowding 50% · 10 mentions (Medium)"
    json.loads(batch.compare_output_to_json(out))                              # the wire format takes it


def test_rank_group_records_orders_like_sort_ranked_and_lists_unnamed_keys():
    import numpy as np
    from openintel_amd import batch
    from openintel_amd.domain import MarketSnapshot, Ticker
    from openintel_amd.engine import SpeculationEngine
    # device order: by total.  (total, by_source, bullish, bearish, neutral, spec_count, polarity_sum)
    rows = [(40, (40, 0), 10, 20, 10, 4, -10.0),     # key 5  BEAR: net -0.25, spec 0.1
            (30, (10, 20), 24, 3, 3, 15, 21.0),       # key 2  BULL: net 0.7, spec 0.5
            (20, (20, 0), 5, 5, 10, 20, 0.0),         # key 9  (no name)
            (12, (6, 6), 6, 0, 6, 12, 6.0),           # key 0  SPEC: net 0.5, spec 1.0
            (11, (11, 0), 0, 0, 11, 0, 0.0)]          # key 7  FLAT: net 0, spec 0
    keys = np.array([5, 2, 9, 0, 7, 0xFFFFFFFF], np.uint32)
    rec = _records(rows + [(0, (0, 0), 0, 0, 0, 0, 0.0)])
    names = {5: "BEAR", 2: "BULL", 0: "SPEC", 7: "FLAT", 8: "$$$"}
    down = MarketSnapshot(Ticker.parse("BULL"), 90.0, 100.0, 1, 1, None, None, None)     # sentiment up, price down: diverging
    for by in batch.RankBy:
        out = batch.rank_group_records(keys, rec, 5, names, by, market_by_ticker={"BULL": down})
        assert out.rank_by is by
        assert [(e.ticker, e.error) for e in out.errors] == [("#9", "group key 9 has no ticker name")]
        want = []
        for k, r in zip(keys[:5], rec[:5]):
            if int(k) in names:
                rep = SpeculationEngine.aggregate_counters(Ticker.parse(names[int(k)]), batch.counters_record(r),
                                                           down if names[int(k)] == "BULL" else None, None, batch.EngineConfig())
                want.append(batch.RankedEntry(names[int(k)], batch.rank_metric(rep, by), rep))
        batch.sort_ranked(want, by)
        assert [r.ticker for r in out.ranked] == [w.ticker for w in want]
        assert [r.rank_metric for r in out.ranked] == [w.rank_metric for w in want]
    order = {by: [r.ticker for r in batch.rank_group_records(keys, rec, 5, names, by, market_by_ticker={"BULL": down}).ranked]
             for by in batch.RankBy}
    assert order[batch.RankBy.NET_SENTIMENT] == ["BULL", "SPEC", "FLAT", "BEAR"]
    assert order[batch.RankBy.SPECULATION_INDEX] == ["SPEC", "BULL", "BEAR", "FLAT"]
    assert order[batch.RankBy.DIVERGENCE][0] == "BULL"                          # diverging first, whatever its crowding
    # a sequence names keys by position; a key past its end, an invalid name and a foreign market snapshot are errors
    out = batch.rank_group_records(np.array([1, 4, 0], np.uint32), rec[:3], 3, ["$$$", "OK"], batch.RankBy.CROWDING,
                                   market_by_ticker={"OK": down})
    assert [r.ticker for r in out.ranked] == [] and [e.ticker for e in out.errors] == ["OK", "#4", "$$$"]
    assert out.errors[2].error == "invalid ticker: $$$" and "BULL" in out.errors[0].error
    assert batch.rank_group_records(keys, rec, 0, names, batch.RankBy.CROWDING).ranked == []
