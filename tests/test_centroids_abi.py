"""CPU-side checks of the narrative-discovery boundary (oi_label_sums, oi_centroids_from_sums, oi_narratives_fit): the header,
the Python table, the Rust binding, the argument checks that run before any device call, and the shape constants of
centroids.hip that tests/test_gpu_centroids.py hard-codes."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ARGS = {"oi_label_sums": 6, "oi_centroids_from_sums": 8, "oi_narratives_fit": 10}
# the shapes tests/test_gpu_centroids.py builds its edge cases from
SHAPE = {"LS_SLICE": 64, "LS_STEP_ROWS": 4, "LS_UNROLL": 4, "LS_THREADS": 1024, "LS_BLOCK_ROWS": 64, "LS_WG_STEP_ROWS": 1024,
         "LS_RANGE_ROWS": 2048}


def _header_code():
    hdr = open(os.path.join(ROOT, "include", "openintel_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_calls_the_structs_and_the_limit():
    hdr, code = _header_code()
    for name, n in N_ARGS.items():
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, code, flags=re.S)
        assert m and m.group(1).count(",") + 1 == n, name
    assert re.search(r"#define\s+OI_MAX_CENTROIDS\s+256u\b", code)
    assert re.search(r"#define\s+OI_ABI_VERSION\s+1\b", code)
    m = re.search(r"typedef\s+struct\s+oi_narrative_spec\s*\{(.*?)\}\s*oi_narrative_spec\s*;", code, flags=re.S)
    assert m and [w for w in re.findall(r"\b(threshold|stamp_origin|bucket_width|n_buckets|max_iters)\b", m.group(1))] == \
        ["threshold", "stamp_origin", "bucket_width", "n_buckets", "max_iters"]
    m = re.search(r"typedef\s+struct\s+oi_narrative_info\s*\{(.*?)\}\s*oi_narrative_info\s*;", code, flags=re.S)
    assert m and " ".join(m.group(1).split()) == "uint32_t iterations, converged; uint64_t moved, assigned;"

    def flat(t):
        return " ".join(t.replace(" *", " ").split())

    text = flat(hdr)
    for phrase in ("fix(x) = (int64) rint(v * 2^30)", "A label >= n_clusters (0xFFFFFFFF included) is \"no cluster\"",
                   "n2 = n2 + v_k * v_k (one rounded f64 multiply, one rounded f64 add, no fma)",
                   "centroids_out may alias previous", "it SYNCHRONISES the ctx stream in both locations",
                   'Profile tag "label_sums"', 'Profile tag "centroids"', '"fit_moved"'):
        assert flat(phrase) in text, phrase


def test_python_table_structs_and_rust_binding_match_the_header():
    import ctypes as C
    from openintel_amd import _lib
    assert _lib.OI_MAX_CENTROIDS == 256
    for name, n in N_ARGS.items():
        assert len(_lib.SIGNATURES[name][1]) == n, name
    assert [f[0] for f in _lib.NarrativeSpec._fields_] == ["threshold", "stamp_origin", "bucket_width", "n_buckets", "max_iters"]
    assert C.sizeof(_lib.NarrativeSpec) == 20
    assert [f[0] for f in _lib.NarrativeInfo._fields_] == ["iterations", "converged", "moved", "assigned"]
    assert C.sizeof(_lib.NarrativeInfo) == 24
    src = re.sub(r"//.*", "", open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read())
    for name, n in N_ARGS.items():
        m = re.search(r"pub fn %s\s*\(([^)]*)\)" % name, src, flags=re.S)
        assert m and len([a for a in m.group(1).split(",") if a.strip()]) == n, name
    assert "pub struct OiNarrativeSpec" in src and "pub struct OiNarrativeInfo" in src and "OI_MAX_CENTROIDS: u32 = 256" in src
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    for fn, sym in (("label_sums", "oi_label_sums"), ("centroids_from_sums", "oi_centroids_from_sums"), ("fit_narratives", "oi_narratives_fit")):
        assert "pub fn %s" % fn in lib_rs and "ffi::%s" % sym in lib_rs


def test_the_new_kernel_file_is_part_of_the_build():
    from openintel_amd import build
    assert "centroids.hip" in build.sources()


def test_shape_constants_are_the_ones_the_gpu_tests_hard_code():
    src = open(os.path.join(ROOT, "openintel_amd", "csrc", "centroids.hip")).read()
    for name, value in SHAPE.items():
        m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert m and int(m.group(1)) == value, name
    import importlib.util
    spec = importlib.util.spec_from_file_location("_gpu_centroids", os.path.join(ROOT, "tests", "test_gpu_centroids.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert (mod.SLICE, mod.STEP, mod.BLOCK, mod.WG_STEP, mod.RANGE) == (SHAPE["LS_SLICE"], SHAPE["LS_STEP_ROWS"], SHAPE["LS_BLOCK_ROWS"],
                                                                        SHAPE["LS_WG_STEP_ROWS"], SHAPE["LS_RANGE_ROWS"])


def test_python_wrappers_exist_with_the_documented_defaults():
    import dataclasses
    import inspect
    from openintel_amd import batch, retriever
    assert list(inspect.signature(retriever.HybridIndex.label_sums).parameters) == ["self", "labels", "n_clusters"]
    sig = inspect.signature(retriever.centroids_from_sums)
    assert list(sig.parameters) == ["ctx", "sums", "counts", "previous"] and sig.parameters["previous"].default is None
    sig = inspect.signature(retriever.HybridIndex.fit_narratives)
    assert list(sig.parameters) == ["self", "seeds", "threshold", "max_iters", "n_buckets", "stamp_origin", "bucket_width", "filter", "labels"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["max_iters"], d["n_buckets"], d["stamp_origin"], d["bucket_width"], d["filter"], d["labels"]) == (20, 1, 0, 0, None, False)
    assert [f.name for f in dataclasses.fields(retriever.NarrativeFit)] == ["centroids", "records", "labels", "iterations", "converged",
                                                                           "moved", "assigned"]
    sig = inspect.signature(batch.discover_narratives)
    assert list(sig.parameters) == ["index", "seeds", "threshold", "kw"] and sig.parameters["kw"].kind is inspect.Parameter.VAR_KEYWORD


def test_bad_arguments_are_refused_without_touching_a_device():
    import ctypes as C
    import numpy as np
    from openintel_amd import build, _lib
    build.build()
    lib = _lib.load()
    INVALID, HOST = _lib.OI_ERR_INVALID_ARG, _lib.OI_HOST
    none = C.c_void_p(None)
    buf = np.zeros(64, dtype=np.uint64)     # a real host buffer wherever one is required
    p = _lib.ptr(buf)
    nan = float("nan")

    def refused(rc, word):
        msg = lib.oi_last_error()
        assert rc == INVALID and msg and word in msg, (rc, msg, word)

    # oi_label_sums(idx, labels, n_clusters, location, sums_out, counts_out)
    def sums(k=4, labels=p, s=p, c=p):
        return lib.oi_label_sums(none, labels, k, HOST, s, c)

    refused(sums(), b"null index")
    refused(sums(k=256), b"null index")
    refused(sums(k=0), b"n_clusters=0")
    refused(sums(k=257), b"n_clusters=257")
    refused(sums(labels=none), b"null buffer")
    refused(sums(s=none), b"null buffer")
    refused(sums(c=none), b"null buffer")

    # oi_centroids_from_sums(ctx, sums, counts, previous, n_clusters, dim, location, centroids_out)
    def cent(k=4, dim=8, s=p, c=p, prev=none, out=p):
        return lib.oi_centroids_from_sums(none, s, c, prev, k, dim, HOST, out)

    refused(cent(), b"null ctx")
    refused(cent(prev=p), b"null ctx")
    refused(cent(k=0), b"n_clusters=0")
    refused(cent(k=257), b"n_clusters=257")
    refused(cent(dim=0), b"dim=0")
    refused(cent(dim=6), b"dim=6")
    refused(cent(dim=1028), b"dim=1028")
    refused(cent(s=none), b"null buffer")
    refused(cent(c=none), b"null buffer")
    refused(cent(out=none), b"null buffer")

    # oi_narratives_fit(idx, seeds, n_clusters, spec, filter, location, centroids_out, records_out, labels_out, info_host)
    def spec(t=0.5, origin=0, width=0, nb=1, iters=5):
        return C.byref(_lib.NarrativeSpec(t, origin, width, nb, iters))

    def fit(k=4, sp=None, seeds=p, cent_out=p, rec=p, labels=p, info=p):
        return lib.oi_narratives_fit(none, seeds, k, spec() if sp is None else sp, none, HOST, cent_out, rec, labels, info)

    refused(fit(), b"null index")
    refused(fit(sp=none), b"null spec")
    refused(fit(k=0), b"n_clusters=0")
    refused(fit(k=257), b"n_clusters=257")
    refused(fit(k=256, sp=spec(iters=1)), b"null index")
    refused(fit(sp=spec(iters=64)), b"null index")
    refused(fit(sp=spec(iters=0)), b"max_iters=0")
    refused(fit(sp=spec(iters=65)), b"max_iters=65")
    refused(fit(sp=spec(t=nan)), b"NaN")
    refused(fit(sp=spec(nb=0)), b"n_buckets=0")
    refused(fit(sp=spec(nb=2)), b"bucket_width=0")
    refused(fit(seeds=none), b"null buffer")
    refused(fit(cent_out=none), b"null buffer")
    refused(fit(rec=none), b"null buffer")
    refused(fit(info=none), b"null buffer")
    refused(fit(labels=none), b"null index")                                # labels_out may be NULL: on to the handle
