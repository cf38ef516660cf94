"""CPU-side checks of the near-duplicate collapse boundary (oi_collapse_lists, oi_search_collapsed): the header, the Python
table, the Rust binding, and the argument checks that run before any device call."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLLAPSE = {"oi_collapse_lists": 13, "oi_search_collapsed": 15}   # name -> number of arguments


def _header_code():
    hdr = open(os.path.join(ROOT, "include", "openintel_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_both_functions_and_states_the_rules():
    hdr, code = _header_code()
    for name, n_args in COLLAPSE.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == n_args, name
    assert re.search(r"#define\s+OI_ABI_VERSION\s+1\b", code)
    text = " ".join(hdr.split())
    for phrase in ("SINGLETON", "oi_search_sharded* and oi_pipeline_*", "within 1e-5 of t"):
        assert phrase in text, phrase


def test_python_table_and_rust_binding_have_matching_argument_counts():
    from openintel_amd import _lib
    src = open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read()
    src = re.sub(r"//.*", "", src)
    for name, n_args in COLLAPSE.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == n_args, name
        m = re.search(r"pub fn " + name + r"\s*\(([^)]*)\)", src, flags=re.S)
        assert m, name
        assert len([a for a in m.group(1).split(",") if a.strip()]) == n_args, name
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    assert "fn search_collapsed" in lib_rs and "ffi::oi_search_collapsed" in lib_rs


def test_python_wrappers_exist_and_existing_constructors_keep_working():
    from openintel_amd import retriever
    assert callable(retriever.HybridIndex.collapse_lists) and callable(retriever.HybridIndex.search_collapsed)
    r = retriever.SearchResult(1, 2, 3)
    assert (r.scores, r.docs, r.counts) == (1, 2, 3)
    c = retriever.CollapsedResult(1, 2, 3)
    assert isinstance(c, retriever.SearchResult) and c.dup_counts is None
    assert retriever.CollapsedResult(1, 2, 3, 4).dup_counts == 4


def test_bad_arguments_are_refused_without_touching_a_device():
    import ctypes as C
    import numpy as np
    from openintel_amd import build, _lib
    build.build()
    lib = _lib.load()
    INVALID, HOST = _lib.OI_ERR_INVALID_ARG, _lib.OI_HOST
    none = C.c_void_p(None)
    buf = np.zeros(8, dtype=np.uint32)     # a real host buffer wherever one is required
    p = _lib.ptr(buf)
    nan = float("nan")
    MAXD = _lib.OI_MAX_DEPTH

    def refused(rc, word):
        msg = lib.oi_last_error()
        assert rc == INVALID and msg and word in msg, (rc, msg)

    # oi_collapse_lists(idx, scores, docs, counts, B, depth, threshold, k, location, scores_out, docs_out, counts_out, dup_out)
    refused(lib.oi_collapse_lists(none, p, p, p, 1, 1, 0.5, 1, HOST, p, p, p, p), b"null index")
    refused(lib.oi_collapse_lists(none, p, p, p, 1, 1, nan, 1, HOST, p, p, p, p), b"NaN")
    refused(lib.oi_collapse_lists(none, p, p, p, 1, 1, 0.5, 0, HOST, p, p, p, p), b"k=0")
    refused(lib.oi_collapse_lists(none, p, p, p, 1, 1, 0.5, MAXD + 1, HOST, p, p, p, p), b"k=%d" % (MAXD + 1))
    refused(lib.oi_collapse_lists(none, p, p, p, 1, 0, 0.5, 1, HOST, p, p, p, p), b"depth")
    refused(lib.oi_collapse_lists(none, p, p, p, 1, MAXD + 1, 0.5, 1, HOST, p, p, p, p), b"depth")
    refused(lib.oi_collapse_lists(none, p, p, p, 1, 1, 0.5, 1, HOST, p, none, p, p), b"null buffer")
    refused(lib.oi_collapse_lists(none, p, p, p, 1, 1, 0.5, 1, HOST, p, p, none, p), b"null buffer")
    refused(lib.oi_collapse_lists(none, p, none, p, 1, 1, 0.5, 1, HOST, p, p, p, p), b"null buffer")
    refused(lib.oi_collapse_lists(none, p, p, p, 1, 1, 0.5, 1, HOST, none, p, p, p), b"without scores_out")
    # oi_search_collapsed(idx, qv, qt, qo, B, depth, pool, k, threshold, filters, location, scores_out, docs_out, counts_out, dup_out)
    refused(lib.oi_search_collapsed(none, p, p, p, 1, 1, 4, 2, 0.5, none, HOST, p, p, p, p), b"null index")
    refused(lib.oi_search_collapsed(none, p, p, p, 1, 1, 4, 2, nan, none, HOST, p, p, p, p), b"NaN")
    refused(lib.oi_search_collapsed(none, p, p, p, 1, 1, 4, 0, 0.5, none, HOST, p, p, p, p), b"k=0")
    refused(lib.oi_search_collapsed(none, p, p, p, 1, 1, 4, 5, 0.5, none, HOST, p, p, p, p), b"exceeds pool")
    refused(lib.oi_search_collapsed(none, p, p, p, 1, 1, MAXD + 1, 5, 0.5, none, HOST, p, p, p, p), b"pool")
    refused(lib.oi_search_collapsed(none, p, p, p, 1, 1, 0, 1, 0.5, none, HOST, p, p, p, p), b"pool")
    refused(lib.oi_search_collapsed(none, p, p, p, 1, 1, 4, 2, 0.5, none, HOST, none, p, p, p), b"null output")
    refused(lib.oi_search_collapsed(none, p, p, p, 1, 1, 4, 2, 0.5, none, HOST, p, none, p, p), b"null output")
    refused(lib.oi_search_collapsed(none, p, p, p, 1, 1, 4, 2, 0.5, none, HOST, p, p, none, p), b"null output")
