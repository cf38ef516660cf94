"""CPU-side checks of the narrative-terms boundary (oi_label_term_counts, oi_label_terms_rank, oi_label_terms): the header, the
Python table, the Rust binding, the argument checks that run before any device call, and the shape constants of
label_terms.hip that tests/test_gpu_label_terms.py hard-codes."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ARGS = {"oi_label_term_counts": 6, "oi_label_terms_rank": 9, "oi_label_terms": 8}
# the shapes tests/test_gpu_label_terms.py builds its edge cases from: threads per workgroup of the count pass, the posting
# count at which a term is split (and the width of a task's cut), the slice width and the merge fan of the rank
SHAPE = {"LT_THREADS": 256, "LT_SPLIT_POSTINGS": 16384, "LT_RANK_SLICE": 1024, "LT_MERGE_FAN": 64}


def _header_code():
    hdr = open(os.path.join(ROOT, "include", "openintel_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_calls_the_structs_and_the_limits():
    hdr, code = _header_code()
    for name, n in N_ARGS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, code, flags=re.S)
        assert m and m.group(1).count(",") + 1 == n, name
    assert re.search(r"#define\s+OI_MAX_LABEL_TERMS\s+64u", code)
    assert re.search(r"#define\s+OI_MAX_LABEL_TERM_CELLS\s+\(1u\s*<<\s*28\)", code)
    assert re.search(r"#define\s+OI_ABI_VERSION\s+1\b", code)
    m = re.search(r"typedef\s+struct\s+oi_label_terms_spec\s*\{(.*?)\}\s*oi_label_terms_spec\s*;", code, flags=re.S)
    assert m and " ".join(m.group(1).split()) == "uint32_t top, min_df, reserved[2];"
    m = re.search(r"typedef\s+struct\s+oi_label_term\s*\{(.*?)\}\s*oi_label_term\s*;", code, flags=re.S)
    assert m and " ".join(m.group(1).split()) == "uint32_t term, df_cluster, df_assigned, reserved; int64_t excess;"

    def flat(t):
        return " ".join(t.replace(" *", " ").split())

    text = flat(hdr)
    for phrase in ("excess(c, t) = (int64)counts[t][c] * A - (int64)sizes[c] * dfA[t]",
                   "excess descending, then counts[t][c] descending, then t ascending",
                   "A label >= n_clusters (0xFFFFFFFF included) is \"no cluster\", as in oi_label_sums",
                   "and sizes of document shards ADD",
                   "Term t is ELIGIBLE for cluster c when counts[t][c] >= max(min_df, 1)",
                   "A <= 2^31 - 1 is required", "wraps in two's complement",
                   'Profile tags: "label_term_counts"', '"label_terms_rank"', '"label_terms" holds the table of the composite call'):
        assert flat(phrase) in text, phrase


def test_python_table_structs_and_rust_binding_match_the_header():
    import ctypes as C
    from openintel_amd import _lib
    assert _lib.OI_MAX_LABEL_TERMS == 64 and _lib.OI_MAX_LABEL_TERM_CELLS == 1 << 28
    for name, n in N_ARGS.items():
        assert len(_lib.SIGNATURES[name][1]) == n, name
    assert [f[0] for f in _lib.LabelTermsSpec._fields_] == ["top", "min_df", "reserved"]
    assert C.sizeof(_lib.LabelTermsSpec) == 16
    assert _lib.LABEL_TERM_DTYPE.names == ("term", "df_cluster", "df_assigned", "reserved", "excess")
    assert _lib.LABEL_TERM_DTYPE.itemsize == 24 and _lib.LABEL_TERM_DTYPE.fields["excess"][1] == 16
    src = re.sub(r"//.*", "", open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read())
    for name, n in N_ARGS.items():
        m = re.search(r"pub fn %s\s*\(([^)]*)\)" % name, src, flags=re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == n, name
    assert "pub struct OiLabelTermsSpec" in src and "pub struct OiLabelTerm" in src
    assert "OI_MAX_LABEL_TERMS: u32 = 64" in src and "OI_MAX_LABEL_TERM_CELLS: u32 = 1 << 28" in src
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    for fn, sym in (("label_term_counts", "oi_label_term_counts"), ("rank_label_terms", "oi_label_terms_rank"), ("label_terms", "oi_label_terms")):
        assert "pub fn %s" % fn in lib_rs and "ffi::%s" % sym in lib_rs


def test_the_new_kernel_file_is_part_of_the_build():
    from openintel_amd import build
    assert "label_terms.hip" in build.sources()


def test_shape_constants_are_the_ones_the_gpu_tests_hard_code():
    src = open(os.path.join(ROOT, "openintel_amd", "csrc", "label_terms.hip")).read()
    for name, value in SHAPE.items():
        m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert m and int(m.group(1)) == value, name
    import importlib.util
    spec = importlib.util.spec_from_file_location("_gpu_label_terms", os.path.join(ROOT, "tests", "test_gpu_label_terms.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert (mod.THREADS, mod.SPLIT, mod.SLICE, mod.FAN) == (SHAPE["LT_THREADS"], SHAPE["LT_SPLIT_POSTINGS"], SHAPE["LT_RANK_SLICE"],
                                                            SHAPE["LT_MERGE_FAN"])


def test_python_wrappers_exist_with_the_documented_defaults():
    import dataclasses
    import inspect
    from openintel_amd import batch, retriever
    assert list(inspect.signature(retriever.HybridIndex.label_term_counts).parameters) == ["self", "labels", "n_clusters"]
    sig = inspect.signature(retriever.HybridIndex.label_terms)
    assert list(sig.parameters) == ["self", "labels", "n_clusters", "top", "min_df"]
    assert (sig.parameters["top"].default, sig.parameters["min_df"].default) == (10, 1)
    sig = inspect.signature(retriever.rank_label_terms)
    assert list(sig.parameters) == ["ctx", "counts", "sizes", "top", "min_df"]
    sig = inspect.signature(batch.describe_narratives)
    assert list(sig.parameters) == ["index", "fit_or_labels", "n_clusters", "top", "min_df", "texts"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["n_clusters"], d["top"], d["min_df"], d["texts"]) == (None, 10, 1, None)
    assert [f.name for f in dataclasses.fields(batch.NarrativeTerm)] == ["term", "word", "df", "df_assigned", "lift"]
    assert "describe_narratives" in batch.discover_narratives.__doc__
    sig = inspect.signature(batch.discover_narratives)                      # (its signature and return value are unchanged)
    assert list(sig.parameters) == ["index", "seeds", "threshold", "kw"]


def test_bad_arguments_are_refused_without_touching_a_device():
    import ctypes as C
    import numpy as np
    from openintel_amd import build, _lib
    build.build()
    lib = _lib.load()
    INVALID, HOST = _lib.OI_ERR_INVALID_ARG, _lib.OI_HOST
    none = C.c_void_p(None)
    buf = np.zeros(512, dtype=np.uint64)    # a real host buffer wherever one is required
    p = _lib.ptr(buf)

    def refused(rc, word):
        msg = lib.oi_last_error()
        assert rc == INVALID and msg and word in msg, (rc, msg, word)

    def spec(top=10, min_df=1, r0=0, r1=0):
        return C.byref(_lib.LabelTermsSpec(top, min_df, (C.c_uint32 * 2)(r0, r1)))

    # oi_label_term_counts(idx, labels, n_clusters, location, counts_out, sizes_out)
    def counts(k=4, labels=p, loc=HOST, c=p, s=p):
        return lib.oi_label_term_counts(none, labels, k, loc, c, s)

    refused(counts(), b"null index")
    refused(counts(k=256), b"null index")
    refused(counts(k=0), b"n_clusters=0")
    refused(counts(k=257), b"n_clusters=257")
    refused(counts(labels=none), b"null buffer")
    refused(counts(c=none), b"null buffer")
    refused(counts(s=none), b"null buffer")
    refused(counts(loc=7), b"bad location 7")

    # oi_label_terms_rank(ctx, counts, sizes_host, vocab, n_clusters, spec, location, terms_out, n_out)
    sizes = np.array([5, 7, 0, 1], dtype=np.uint64)

    def rank(table=p, sz=None, vocab=97, k=4, sp=None, loc=HOST, out=p, n=p):
        return lib.oi_label_terms_rank(none, table, _lib.ptr(sizes) if sz is None else sz, vocab, k, spec() if sp is None else sp, loc, out, n)

    refused(rank(), b"null ctx")
    refused(rank(sp=spec(top=1, min_df=0)), b"null ctx")
    refused(rank(sp=spec(top=64, min_df=0xFFFFFFFF)), b"null ctx")
    refused(rank(sp=none), b"null spec")
    refused(rank(sp=spec(top=0)), b"top=0")
    refused(rank(sp=spec(top=65)), b"top=65")
    refused(rank(sp=spec(r0=5)), b"reserved=5")
    refused(rank(sp=spec(r1=9)), b"reserved=9")
    refused(rank(k=0), b"n_clusters=0")
    refused(rank(k=257), b"n_clusters=257")
    refused(rank(vocab=0), b"vocab=0")
    refused(rank(vocab=(1 << 26) + 1), b"268435460 cells")                    # (2^26 + 1) * 4, four over the limit
    refused(rank(vocab=1 << 26), b"null ctx")                                 # exactly the limit passes this check
    refused(rank(table=none), b"null buffer")
    refused(rank(sz=none), b"null buffer")
    refused(rank(out=none), b"null buffer")
    refused(rank(n=none), b"null buffer")
    big = np.array([1 << 30, 1 << 30, 0, 0], dtype=np.uint64)                 # A = 2^31
    refused(rank(sz=_lib.ptr(big)), b"A = 2147483648")
    big[1] -= 1                                                               # A = 2^31 - 1: in range
    refused(rank(sz=_lib.ptr(big)), b"null ctx")
    huge = np.full(4, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)                    # a sum that wraps in 64 bits is still refused
    refused(rank(sz=_lib.ptr(huge)), b"A = 18446744073709551615")
    refused(rank(loc=2), b"bad location 2")

    # oi_label_terms(idx, labels, n_clusters, spec, location, terms_out, n_out, sizes_out)
    def terms(labels=p, k=4, sp=None, loc=HOST, out=p, n=p, s=p):
        return lib.oi_label_terms(none, labels, k, spec() if sp is None else sp, loc, out, n, s)

    refused(terms(), b"null index")
    refused(terms(s=none), b"null index")                                    # sizes_out may be NULL: on to the handle
    refused(terms(sp=none), b"null spec")
    refused(terms(sp=spec(top=0)), b"top=0")
    refused(terms(sp=spec(top=65)), b"top=65")
    refused(terms(sp=spec(r0=1)), b"reserved=1")
    refused(terms(k=0), b"n_clusters=0")
    refused(terms(k=257), b"n_clusters=257")
    refused(terms(labels=none), b"null buffer")
    refused(terms(out=none), b"null buffer")
    refused(terms(n=none), b"null buffer")
    refused(terms(loc=-1), b"bad location -1")
