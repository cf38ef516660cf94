"""CPU-side checks of the narrative-exemplars boundary (oi_label_exemplars): the header, the Python table, the Rust binding, the
argument checks that run before any device call, and the shape constants of label_exemplars.hip that
tests/test_gpu_exemplars.py hard-codes."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the shapes tests/test_gpu_exemplars.py builds its edge cases from: rows a wave labels at once, rows per range of the score
# pass, bits per pass of the select, threads per workgroup
SHAPE = {"LE_BLOCK_ROWS": 64, "LE_RANGE_ROWS": 2048, "LE_RADIX_BITS": 8, "LE_THREADS": 256}


def _header_code():
    hdr = open(os.path.join(ROOT, "include", "openintel_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_call_the_struct_and_the_limits():
    hdr, code = _header_code()
    m = re.search(r"\bint\s+oi_label_exemplars\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m and m.group(1).count(",") + 1 == 10
    assert re.search(r"#define\s+OI_MAX_DEPTH\s+1024u", code)
    assert re.search(r"#define\s+OI_MAX_CENTROIDS\s+256u", code)
    assert re.search(r"#define\s+OI_ABI_VERSION\s+1\b", code)
    m = re.search(r"typedef\s+struct\s+oi_exemplar_spec\s*\{(.*?)\}\s*oi_exemplar_spec\s*;", code, flags=re.S)
    assert m and " ".join(m.group(1).split()) == "uint32_t top, reserved[3];"

    def flat(t):
        return " ".join(t.replace(" *", " ").split())

    text = flat(hdr)
    for phrase in ("labels[d] == c < n_clusters", "is \"no cluster\", as in oi_label_sums", "s = sim(centroids[c], d) is not NaN",
                   "descending order of oi_rank_key(s, doc)", "ties to the smaller doc id", "GLOBAL doc ids (doc_id_base + local row)",
                   "entries beyond it are score 0 and doc 0xFFFFFFFF", "An empty cluster has count 0",
                   "bit for bit the sim oi_similar_share compared against the threshold",
                   "valid input of oi_collapse_lists (row stride `top`)", "oi_merge_lists",
                   "no host synchronise anywhere", "Not captured by graph replay",
                   'Profile tags: "exemplar_score"', '"exemplar_select"', '"exemplar_emit"', '"exemplars" holds one 4-byte score key',
                   "NOT covered: a screened route over the bf16 copy"):
        assert flat(phrase) in text, phrase


def test_python_table_struct_and_rust_binding_match_the_header():
    import ctypes as C
    from openintel_amd import _lib
    assert _lib.OI_MAX_DEPTH == 1024 and _lib.OI_MAX_CENTROIDS == 256
    assert len(_lib.SIGNATURES["oi_label_exemplars"][1]) == 10
    assert [f[0] for f in _lib.ExemplarSpec._fields_] == ["top", "reserved"]
    assert C.sizeof(_lib.ExemplarSpec) == 16
    src = re.sub(r"//.*", "", open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read())
    m = re.search(r"pub fn oi_label_exemplars\s*\(([^)]*)\)", src, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 10
    m = re.search(r"pub struct OiExemplarSpec\s*\{(.*?)\}", src, flags=re.S)
    assert m and " ".join(m.group(1).split()) == "pub top: u32, pub reserved: [u32; 3],"
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    assert "pub fn label_exemplars" in lib_rs and "ffi::oi_label_exemplars" in lib_rs
    check = open(os.path.join(ROOT, "integration", "c", "abi_check.c")).read()
    assert "sizeof(oi_exemplar_spec) != 16" in check


def test_the_new_kernel_file_is_part_of_the_build():
    from openintel_amd import build
    assert "label_exemplars.hip" in build.sources()


def test_shape_constants_are_the_ones_the_gpu_tests_hard_code():
    src = open(os.path.join(ROOT, "openintel_amd", "csrc", "label_exemplars.hip")).read()
    for name, value in SHAPE.items():
        m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert m and int(m.group(1)) == value, name
    import importlib.util
    spec = importlib.util.spec_from_file_location("_gpu_exemplars", os.path.join(ROOT, "tests", "test_gpu_exemplars.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert (mod.BLOCK, mod.RANGE, mod.RADIX_BITS, mod.THREADS) == (SHAPE["LE_BLOCK_ROWS"], SHAPE["LE_RANGE_ROWS"], SHAPE["LE_RADIX_BITS"],
                                                                   SHAPE["LE_THREADS"])


def test_python_wrappers_exist_with_the_documented_defaults():
    import inspect
    from openintel_amd import batch, retriever
    sig = inspect.signature(retriever.HybridIndex.label_exemplars)
    assert list(sig.parameters) == ["self", "labels", "centroids", "top", "filter"]
    assert (sig.parameters["top"].default, sig.parameters["filter"].default) == (10, None)
    sig = inspect.signature(batch.narrative_exemplars)
    assert list(sig.parameters) == ["index", "fit_or_labels", "centroids", "top", "pool", "collapse", "texts"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["centroids"], d["top"], d["pool"], d["collapse"], d["texts"]) == (None, 5, 64, None, None)
    sig = inspect.signature(batch.describe_narratives)                      # (left unchanged)
    assert list(sig.parameters) == ["index", "fit_or_labels", "n_clusters", "top", "min_df", "texts"]


def test_bad_arguments_are_refused_without_touching_a_device():
    import ctypes as C
    import numpy as np
    from openintel_amd import build, _lib
    build.build()
    lib = _lib.load()
    INVALID, HOST, DEVICE = _lib.OI_ERR_INVALID_ARG, _lib.OI_HOST, _lib.OI_DEVICE
    none = C.c_void_p(None)
    buf = np.zeros(512, dtype=np.uint64)    # a real host buffer wherever one is required
    p = _lib.ptr(buf)

    def refused(rc, word):
        msg = lib.oi_last_error()
        assert rc == INVALID and msg and word in msg, (rc, msg, word)

    def spec(top=10, r=(0, 0, 0)):
        return C.byref(_lib.ExemplarSpec(top, (C.c_uint32 * 3)(*r)))

    filt = C.byref(_lib.DocFilter(0, 0, 0, 0xFFFFFFFF))

    # oi_label_exemplars(idx, labels, centroids, n_clusters, spec, filter, location, scores_out, docs_out, counts_out)
    def call(labels=p, cent=p, k=4, sp=None, f=none, loc=HOST, s=p, d=p, c=p):
        return lib.oi_label_exemplars(none, labels, cent, k, spec() if sp is None else sp, f, loc, s, d, c)

    refused(call(), b"null index")                                         # every other argument is in range: on to the handle
    refused(call(sp=spec(top=1)), b"null index")
    refused(call(sp=spec(top=1024), k=256), b"null index")
    refused(call(f=filt, loc=DEVICE), b"null index")
    refused(call(sp=none), b"null spec")
    refused(call(sp=spec(top=0)), b"top=0")
    refused(call(sp=spec(top=1025)), b"top=1025")
    refused(call(sp=spec(r=(5, 0, 0))), b"reserved=5")
    refused(call(sp=spec(r=(0, 9, 0))), b"reserved=9")
    refused(call(sp=spec(r=(0, 0, 3))), b"reserved=3")
    refused(call(k=0), b"n_clusters=0")
    refused(call(k=257), b"n_clusters=257")
    refused(call(labels=none), b"null buffer")
    refused(call(cent=none), b"null buffer")
    refused(call(s=none), b"null buffer")
    refused(call(d=none), b"null buffer")
    refused(call(c=none), b"null buffer")
    refused(call(loc=7), b"bad location 7")
    refused(call(loc=-1), b"bad location -1")
