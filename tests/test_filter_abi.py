"""CPU-side checks of the filtered-search boundary (oi_doc_filter): the header, the Python structure, the Rust binding and
the argument checks that run before any device call."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERED = ("oi_index_set_doc_attrs", "oi_search_lists_filtered", "oi_search_lists_packed_filtered",
            "oi_search_filtered", "oi_search_sharded_filtered")


def test_header_declares_the_filter_and_the_five_entry_points():
    hdr = open(os.path.join(ROOT, "include", "openintel_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"typedef\s+struct\s+oi_doc_filter\s*\{([^}]*)\}\s*oi_doc_filter\s*;", code)
    assert m, "oi_doc_filter is not declared"
    assert re.findall(r"\w+", m.group(1)) == ["uint32_t", "group_mask", "group_value", "stamp_lo", "stamp_hi"]
    for name in FILTERED:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name


def test_python_doc_filter_is_16_bytes_in_header_order():
    import ctypes as C
    from openintel_amd import _lib
    assert C.sizeof(_lib.DocFilter) == 16
    assert [f[0] for f in _lib.DocFilter._fields_] == ["group_mask", "group_value", "stamp_lo", "stamp_hi"]
    assert [f[1] for f in _lib.DocFilter._fields_] == [C.c_uint32] * 4
    for name, off in (("group_mask", 0), ("group_value", 4), ("stamp_lo", 8), ("stamp_hi", 12)):
        assert getattr(_lib.DocFilter, name).offset == off
    for name in FILTERED:
        assert name in _lib.SIGNATURES


def test_rust_binding_has_the_filter_struct_and_the_functions():
    src = open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read()
    m = re.search(r"#\[repr\(C\)\][^{]*?pub struct OiDocFilter\s*\{([^}]*)\}", src, flags=re.S)
    assert m, "no #[repr(C)] OiDocFilter"
    fields = re.findall(r"pub\s+(\w+)\s*:\s*(\w+)", m.group(1))
    assert fields == [("group_mask", "u32"), ("group_value", "u32"), ("stamp_lo", "u32"), ("stamp_hi", "u32")]
    for name in FILTERED:
        assert re.search(r"pub fn " + name + r"\s*\(", src), name
    lib = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    for name in ("fn set_doc_attrs", "fn search_filtered", "fn search_sharded_filtered"):
        assert name in lib, name


def test_null_handles_and_arguments_are_refused_without_touching_a_device():
    import ctypes as C
    from openintel_amd import build, _lib
    build.build()
    lib = _lib.load()
    INVALID = _lib.OI_ERR_INVALID_ARG
    none = C.c_void_p(None)
    assert lib.oi_index_set_doc_attrs(none, none, none, _lib.OI_HOST) == INVALID and lib.oi_last_error()
    assert lib.oi_search_lists_filtered(none, none, none, none, 1, 1, none, _lib.OI_HOST,
                                        none, none, none, none, none, none) == INVALID
    assert lib.oi_search_lists_packed_filtered(none, none, none, none, 1, 1, none, _lib.OI_HOST, none) == INVALID
    assert lib.oi_search_filtered(none, none, none, none, 1, 1, 1, none, _lib.OI_HOST, none, none, none) == INVALID
    assert lib.oi_search_sharded_filtered(none, none, none, none, none, 1, 1, 1, none, _lib.OI_HOST,
                                          none, none, none) == INVALID
    assert b"null" in lib.oi_last_error()
