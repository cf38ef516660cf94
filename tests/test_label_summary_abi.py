"""CPU-side checks of the narrative-breakdown boundary (oi_label_summary): the header, the Python table, the Rust binding, the
argument checks that run before any device call, and the shape constants of label_summary.hip that
tests/test_gpu_label_summary.py hard-codes."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the shapes tests/test_gpu_label_summary.py builds its edge cases from: rows a wave labels at once, rows per range of the
# pass, threads per workgroup, cells up to which a workgroup sums in LDS
SHAPE = {"LS_BLOCK_ROWS": 64, "LS_RANGE_ROWS": 2048, "LS_THREADS": 256, "LS_LOCAL_CELLS": 1024}
FIELDS = ["axis", "stamp_origin", "bucket_width", "n_cells", "top", "rank_by", "min_total", "reserved"]


def _header_code():
    hdr = open(os.path.join(ROOT, "include", "openintel_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_call_the_struct_and_the_limits():
    hdr, code = _header_code()
    m = re.search(r"\bint\s+oi_label_summary\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m and m.group(1).count(",") + 1 == 10
    assert re.search(r"#define\s+OI_MAX_DEPTH\s+1024u", code)
    assert re.search(r"#define\s+OI_MAX_CENTROIDS\s+256u", code)
    assert re.search(r"#define\s+OI_MAX_VOLUME_BUCKETS\s+1024u", code)
    assert re.search(r"#define\s+OI_MAX_GROUP_KEYS\s+65536u", code)
    assert re.search(r"#define\s+OI_MAX_GROUP_CELLS\s+\(1u << 20\)", code)
    assert re.search(r"#define\s+OI_ABI_VERSION\s+1\b", code)
    assert re.search(r"enum\s*\{\s*OI_LABEL_AXIS_TIME\s*=\s*0\s*,\s*OI_LABEL_AXIS_KEY\s*=\s*1\s*\}\s*;", code)
    m = re.search(r"typedef\s+struct\s+oi_label_summary_spec\s*\{(.*?)\}\s*oi_label_summary_spec\s*;", code, flags=re.S)
    assert m and " ".join(m.group(1).split()) == " ".join("uint32_t %s;" % f for f in FIELDS)

    def flat(t):
        return " ".join(t.replace(" *", " ").split())

    text = flat(hdr)
    for phrase in ("labels[d] == c < n_clusters", "is \"no cluster\", as in oi_label_sums: it is no error",
                   "the row's attributes and signals are not read", "d passes `filter`, when one is given",
                   "on the TIME axis oi_similar_summary's clause 2 gives x", "on the KEY axis oi_similar_groups's key clause gives x",
                   "a key >= n_cells belongs to no cell", "The record of a cell is oi_similar_summary's, word for word",
                   "polarity_sum = (double)(sum of pol_q30) * 2^-30, the sum taken in 64-bit integers",
                   "the result is a function of the inputs alone: grid, route, order of atomics and run do not matter",
                   "records of document shards add",
                   "the sum over x of total[c][x] on a one-cell TIME axis equals oi_label_sums' counts[c]",
                   "the dense TIME records equal that call's out bit for bit",
                   "summed over the keys, a KEY-axis call equals the one-cell TIME call when every document has a key",
                   "exactly oi_similar_groups' ranked output with \"query\" replaced by \"cluster\"",
                   "v << 32 | ~key", "total >= max(min_total, 1)", "row stride `top`", "0xFFFFFFFF and an all-zero record",
                   "keys_out, counts_out and qualified_out may be NULL and are not written",
                   "Signals are required", "NO embeddings, forward index or finalize are needed", "it works on a view",
                   "no host synchronise anywhere", "Not captured by graph replay", "every argument check precedes the first device call",
                   '"label_summary" holds 64 B per cell', "8 B more per cell", '"label_summary_io"',
                   'Profile tags: "label_summary"', '"label_summary_rank"', "both axes at once"):
        assert flat(phrase) in text, phrase


def test_python_table_struct_and_rust_binding_match_the_header():
    import ctypes as C
    from openintel_amd import _lib
    assert _lib.OI_MAX_DEPTH == 1024 and _lib.OI_MAX_CENTROIDS == 256
    assert (_lib.OI_LABEL_AXIS_TIME, _lib.OI_LABEL_AXIS_KEY) == (0, 1)
    assert len(_lib.SIGNATURES["oi_label_summary"][1]) == 10
    assert [f[0] for f in _lib.LabelSummarySpec._fields_] == FIELDS
    assert C.sizeof(_lib.LabelSummarySpec) == 32
    src = re.sub(r"//.*", "", open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read())
    m = re.search(r"pub fn oi_label_summary\s*\(([^)]*)\)", src, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 10
    m = re.search(r"pub struct OiLabelSummarySpec\s*\{(.*?)\}", src, flags=re.S)
    assert m and " ".join(m.group(1).split()) == " ".join("pub %s: u32," % f for f in FIELDS)
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    assert "pub fn label_summary" in lib_rs and "ffi::oi_label_summary" in lib_rs
    check = open(os.path.join(ROOT, "integration", "c", "abi_check.c")).read()
    assert "sizeof(oi_label_summary_spec) != 32" in check


def test_the_new_kernel_file_is_part_of_the_build():
    from openintel_amd import build
    assert "label_summary.hip" in build.sources()


def test_shape_constants_are_the_ones_the_gpu_tests_hard_code():
    src = open(os.path.join(ROOT, "openintel_amd", "csrc", "label_summary.hip")).read()
    for name, value in SHAPE.items():
        m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert m and int(m.group(1)) == value, name
    import importlib.util
    spec = importlib.util.spec_from_file_location("_gpu_label_summary", os.path.join(ROOT, "tests", "test_gpu_label_summary.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert (mod.BLOCK, mod.RANGE, mod.THREADS, mod.LOCAL_CELLS) == (SHAPE["LS_BLOCK_ROWS"], SHAPE["LS_RANGE_ROWS"], SHAPE["LS_THREADS"],
                                                                   SHAPE["LS_LOCAL_CELLS"])
    m = re.search(r"constexpr\s+uint32_t\s+LS_GRID_PER_CU\s*=\s*(\d+)\s*;", src)    # (the size of the grid-stride case follows it)
    assert m and int(m.group(1)) == mod.GRID_PER_CU


def test_python_wrappers_exist_with_the_documented_defaults():
    import inspect
    from openintel_amd import batch, retriever
    sig = inspect.signature(retriever.HybridIndex.label_summary)
    assert list(sig.parameters) == ["self", "labels", "n_clusters", "n_buckets", "stamp_origin", "bucket_width", "filter"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["n_buckets"], d["stamp_origin"], d["bucket_width"], d["filter"]) == (1, 0, 0, None)
    sig = inspect.signature(retriever.HybridIndex.label_groups)
    assert list(sig.parameters) == ["self", "labels", "n_clusters", "key_mask", "n_keys", "top", "rank_by", "min_total", "filter"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["top"], d["rank_by"], d["min_total"], d["filter"]) == (0, "total", 0, None)
    sig = inspect.signature(batch.narrative_timeline)
    assert list(sig.parameters) == ["index", "fit_or_labels", "stamp_origin", "bucket_width", "n_buckets", "n_clusters", "filter"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["n_clusters"], d["filter"]) == (None, None)
    sig = inspect.signature(batch.narrative_tickers)
    assert list(sig.parameters) == ["index", "fit_or_labels", "tickers", "key_mask", "n_clusters", "top", "rank_by", "min_total", "n_keys",
                                    "filter", "market_by_ticker", "now", "cfg", "distinctive"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["n_clusters"], d["top"], d["min_total"], d["n_keys"], d["filter"], d["market_by_ticker"], d["now"], d["distinctive"]) == (
        None, 10, None, None, None, None, None, False)
    assert isinstance(d["rank_by"], batch.RankBy) and isinstance(d["cfg"], batch.EngineConfig)
    sig = inspect.signature(batch.describe_narratives)                      # (left unchanged)
    assert list(sig.parameters) == ["index", "fit_or_labels", "n_clusters", "top", "min_df", "texts"]


def test_bad_arguments_are_refused_without_touching_a_device():
    import ctypes as C
    import numpy as np
    from openintel_amd import build, _lib
    build.build()
    lib = _lib.load()
    INVALID, HOST, DEVICE = _lib.OI_ERR_INVALID_ARG, _lib.OI_HOST, _lib.OI_DEVICE
    TIME, KEY = _lib.OI_LABEL_AXIS_TIME, _lib.OI_LABEL_AXIS_KEY
    none = C.c_void_p(None)
    buf = np.zeros(512, dtype=np.uint64)    # a real host buffer wherever one is required
    p = _lib.ptr(buf)

    def refused(rc, word):
        msg = lib.oi_last_error()
        assert rc == INVALID and msg and word in msg, (rc, msg, word)

    def spec(axis=TIME, origin=0, width=60, cells=24, top=0, by=0, min_total=0, reserved=0):
        return C.byref(_lib.LabelSummarySpec(axis, origin, width, cells, top, by, min_total, reserved))

    def key(mask=0xFFFF, cells=4096, **kw):
        return spec(axis=KEY, origin=mask, width=0, cells=cells, **kw)

    filt = C.byref(_lib.DocFilter(0, 0, 0, 0xFFFFFFFF))

    # oi_label_summary(idx, labels, n_clusters, spec, filter, location, records_out, keys_out, counts_out, qualified_out)
    def call(labels=p, k=8, sp=None, f=none, loc=HOST, r=p, ks=p, c=p, q=p):
        return lib.oi_label_summary(none, labels, k, spec() if sp is None else sp, f, loc, r, ks, c, q)

    # every argument in range: on to the handle
    refused(call(), b"null index")
    refused(call(sp=spec(width=0, cells=1)), b"null index")
    refused(call(sp=spec(cells=1024), k=256), b"null index")
    refused(call(sp=spec(origin=0xFFFFFFFF, width=1, cells=1)), b"null index")
    refused(call(ks=none, c=none, q=none), b"null index")                      # dense: the three may be NULL
    refused(call(sp=key(), f=filt, loc=DEVICE), b"null index")
    refused(call(sp=key(mask=0xFFFFFFFF, cells=65536), k=16), b"null index")   # the cell limit itself
    refused(call(sp=key(mask=0x00FFFF00, cells=65536, top=1024, by=3, min_total=7), k=16, q=none), b"null index")
    refused(call(sp=key(mask=0x80000000, cells=2, top=1, by=1), k=1), b"null index")
    refused(call(sp=key(cells=1, top=1)), b"null index")

    refused(call(sp=none), b"null spec")
    refused(call(labels=none), b"null buffer")
    refused(call(r=none), b"null buffer")
    refused(call(sp=key(top=5), ks=none), b"null buffer")
    refused(call(sp=key(top=5), c=none), b"null buffer")
    refused(call(k=0), b"n_clusters=0")
    refused(call(k=257), b"n_clusters=257")
    refused(call(sp=spec(cells=0)), b"n_cells=0")
    refused(call(sp=key(cells=0)), b"n_cells=0")
    refused(call(sp=spec(cells=1025)), b"n_cells=1025")
    refused(call(sp=spec(width=0, cells=2)), b"n_cells=2")
    refused(call(sp=key(mask=0xFFFFFFFF, cells=65537), k=1), b"n_cells=65537")
    refused(call(sp=key(mask=0xF, cells=17)), b"n_cells=17")
    refused(call(sp=key(mask=0xFFFFFFFF, cells=61681), k=17), b"1048577 cells")   # 17 * 61681 = 2^20 + 1
    refused(call(sp=spec(top=1)), b"top=1")
    refused(call(sp=key(top=1025)), b"top=1025")
    refused(call(sp=key(top=5, by=4)), b"rank_by=4")
    refused(call(sp=key(top=0, by=2)), b"rank_by=2")
    refused(call(sp=spec(reserved=9)), b"reserved=9")
    refused(call(sp=key(reserved=1)), b"reserved=1")
    refused(call(sp=spec(axis=KEY, origin=0xFF, width=60, cells=4)), b"bucket_width=60")
    refused(call(sp=key(mask=0)), b"key_mask=0x0")
    refused(call(sp=key(mask=0x5, cells=2)), b"key_mask=0x5")
    refused(call(sp=spec(axis=2)), b"axis=2")
    refused(call(loc=7), b"bad location 7")
    refused(call(loc=-1), b"bad location -1")
