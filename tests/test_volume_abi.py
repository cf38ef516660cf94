"""CPU-side checks of the similarity-volume boundary (oi_similar_volume): the header, the Python table, the Rust binding, and
the argument checks that run before any device call."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, N_ARGS = "oi_similar_volume", 7


def _header_code():
    hdr = open(os.path.join(ROOT, "include", "openintel_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_function_and_states_the_definition():
    hdr, code = _header_code()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m, NAME
    assert m.group(1).count(",") + 1 == N_ARGS
    assert re.search(r"#define\s+OI_MAX_VOLUME_BUCKETS\s+1024u\b", code)
    m = re.search(r"typedef\s+struct\s+oi_volume_spec\s*\{(.*?)\}\s*oi_volume_spec\s*;", code, flags=re.S)
    assert m, "oi_volume_spec"
    fields = re.findall(r"\b(float|uint32_t)\s+(\w+)\s*;", m.group(1))
    assert fields == [("float", "threshold"), ("uint32_t", "stamp_origin"), ("uint32_t", "bucket_width"), ("uint32_t", "n_buckets")]
    assert re.search(r"#define\s+OI_ABI_VERSION\s+1\b", code)
    text = " ".join(hdr.replace(" *", " ").split())
    for phrase in ("counts_out[q][b] is the number of local documents d of the handle",
                   "d passes filters[q]. filters == NULL means every document passes.",
                   "bucket_width == 0, or stamp_origin <= stamp[d] and (stamp[d] - stamp_origin) / bucket_width == b",
                   "evaluated in 64 bits",
                   "sim(q, d) >= threshold",
                   "in k order with single fused multiply-adds",
                   "within 1e-5 of the f64 dot product for rows of norm <= 1",
                   "A NaN similarity is never >= t",
                   "every route returns the same counts bit for bit",
                   "spec is always a host pointer",
                   "OI_DEVICE is asynchronous on the ctx stream",
                   "it works on a view",
                   "n_queries == 0 is OI_OK",
                   "not captured by graph replay",
                   "oi_search_sharded* and oi_pipeline_*",
                   "a sharded host sums the per-rank arrays"):
        assert phrase in text, phrase


def test_python_table_and_rust_binding_have_matching_argument_counts():
    import ctypes as C
    from openintel_amd import _lib
    assert _lib.OI_MAX_VOLUME_BUCKETS == 1024
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == N_ARGS
    assert C.sizeof(_lib.VolumeSpec) == 16
    assert [f[0] for f in _lib.VolumeSpec._fields_] == ["threshold", "stamp_origin", "bucket_width", "n_buckets"]
    src = open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read()
    src = re.sub(r"//.*", "", src)
    m = re.search(r"pub fn " + NAME + r"\s*\(([^)]*)\)", src, flags=re.S)
    assert m, NAME
    assert len([a for a in m.group(1).split(",") if a.strip()]) == N_ARGS
    m = re.search(r"pub struct OiVolumeSpec\s*\{(.*?)\}", src, flags=re.S)
    assert m and re.findall(r"pub (\w+): (\w+)", m.group(1)) == [("threshold", "f32"), ("stamp_origin", "u32"),
                                                                  ("bucket_width", "u32"), ("n_buckets", "u32")]
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    assert "fn similar_volume" in lib_rs and "ffi::oi_similar_volume" in lib_rs


def test_python_wrapper_exists_with_the_documented_defaults():
    import inspect
    from openintel_amd import retriever
    sig = inspect.signature(retriever.HybridIndex.similar_volume)
    assert list(sig.parameters) == ["self", "query_vecs", "threshold", "n_buckets", "stamp_origin", "bucket_width", "filters"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["n_buckets"], d["stamp_origin"], d["bucket_width"], d["filters"]) == (1, 0, 0, None)


def test_the_new_kernel_file_is_part_of_the_build():
    from openintel_amd import build
    assert "cosine_volume.hip" in build.sources()


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

    def spec(t=0.5, origin=0, width=0, nb=1):
        return C.byref(_lib.VolumeSpec(t, origin, width, nb))

    def refused(rc, word):
        msg = lib.oi_last_error()
        assert rc == INVALID and msg and word in msg, (rc, msg)

    # oi_similar_volume(idx, query_vecs, n_queries, spec, filters, location, counts_out)
    refused(lib.oi_similar_volume(none, p, 1, spec(), none, HOST, p), b"null index")
    refused(lib.oi_similar_volume(none, p, 0, spec(), none, HOST, p), b"null index")
    refused(lib.oi_similar_volume(none, p, 1, none, none, HOST, p), b"null spec")
    refused(lib.oi_similar_volume(none, p, 1, spec(t=float("nan")), none, HOST, p), b"NaN")
    refused(lib.oi_similar_volume(none, p, 1, spec(width=1, nb=0), none, HOST, p), b"n_buckets=0")
    refused(lib.oi_similar_volume(none, p, 1, spec(width=1, nb=1025), none, HOST, p), b"n_buckets=1025")
    refused(lib.oi_similar_volume(none, p, 1, spec(width=0, nb=2), none, HOST, p), b"bucket_width=0")
    refused(lib.oi_similar_volume(none, p, 1, spec(), none, HOST, none), b"null buffer")
    refused(lib.oi_similar_volume(none, none, 1, spec(), none, HOST, p), b"null buffer")
    # +-inf are thresholds like any other: with them the call gets as far as the handle
    refused(lib.oi_similar_volume(none, p, 1, spec(t=float("inf")), none, HOST, p), b"null index")
    refused(lib.oi_similar_volume(none, p, 1, spec(t=float("-inf"), width=3600, nb=1024), none, HOST, p), b"null index")
