"""CPU-side checks of the narrative-seeding boundary (oi_narratives_seed): the header, the struct layouts, the Python table, the
Rust binding, the build, the shape constant tests/test_gpu_seed.py hard-codes, and the argument checks that run before any
device call."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_code():
    hdr = open(os.path.join(ROOT, "include", "openintel_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_call_the_structs_and_the_constants():
    hdr, code = _header_code()
    m = re.search(r"\bint\s+oi_narratives_seed\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
    assert m and m.group(1).count(",") + 1 == 8
    for name, value in (("OI_SEED_KMEANSPP", "0u"), ("OI_SEED_FARTHEST", "1u"), ("OI_MAX_SEED_TRIALS", "8u"), ("OI_MAX_CENTROIDS", "256u"),
                        ("OI_ABI_VERSION", "1")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), code), name
    m = re.search(r"typedef\s+struct\s+oi_seed_spec\s*\{(.*?)\}\s*oi_seed_spec\s*;", code, flags=re.S)
    assert m and re.findall(r"\b(uint32_t|uint64_t|method|trials|seed|stamp_origin|bucket_width|n_buckets|reserved)\b", m.group(1)) == \
        ["uint32_t", "method", "trials", "uint64_t", "seed", "uint32_t", "stamp_origin", "bucket_width", "n_buckets", "reserved"]
    m = re.search(r"typedef\s+struct\s+oi_seed_info\s*\{(.*?)\}\s*oi_seed_info\s*;", code, flags=re.S)
    assert m and " ".join(m.group(1).split()) == "uint32_t found, reserved; uint64_t eligible, potential;"

    def flat(t):
        return " ".join(t.replace(" *", " ").split())

    text = flat(hdr)
    for phrase in ("weight(s) = (uint32) rintf(min(max(1.0f - s, 0), 2) * 2^20)", "weight(NaN) = 0", "r = mulhi64(u, W)",
                   "u(i, t) = splitmix64(seed + (8 * i + t + 1) * 0x9E3779B97F4A7C15)", "ties to the smallest t", "ties to the smallest row",
                   "p_0 is the mulhi64(u(0, 0), E)-th eligible row in row order", "Seeds at and beyond `found` are all-zero vectors with row 0xFFFFFFFF",
                   "without a host synchronise between", '"seed_init"', '"seed_score"', '"seed_pick"', "Never captured by graph replay"):
        assert flat(phrase) in text, phrase
    assert "seeding is the caller's" not in text


def test_python_table_structs_and_rust_binding_match_the_header():
    import ctypes as C
    from openintel_amd import _lib
    assert (_lib.OI_SEED_KMEANSPP, _lib.OI_SEED_FARTHEST, _lib.OI_MAX_SEED_TRIALS) == (0, 1, 8)
    assert len(_lib.SIGNATURES["oi_narratives_seed"][1]) == 8
    assert [f[0] for f in _lib.SeedSpec._fields_] == ["method", "trials", "seed", "stamp_origin", "bucket_width", "n_buckets", "reserved"]
    assert C.sizeof(_lib.SeedSpec) == 32 and _lib.SeedSpec.seed.offset == 8 and _lib.SeedSpec.reserved.offset == 28
    assert [f[0] for f in _lib.SeedInfo._fields_] == ["found", "reserved", "eligible", "potential"]
    assert C.sizeof(_lib.SeedInfo) == 24 and _lib.SeedInfo.eligible.offset == 8
    src = re.sub(r"//.*", "", open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read())
    m = re.search(r"pub fn oi_narratives_seed\s*\(([^)]*)\)", src, flags=re.S)
    assert m and len([a for a in m.group(1).split(",") if a.strip()]) == 8
    assert "pub struct OiSeedSpec" in src and "pub struct OiSeedInfo" in src
    for c in ("OI_SEED_KMEANSPP: u32 = 0", "OI_SEED_FARTHEST: u32 = 1", "OI_MAX_SEED_TRIALS: u32 = 8"):
        assert c in src, c
    lib_rs = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    assert "pub fn seed_narratives" in lib_rs and "ffi::oi_narratives_seed" in lib_rs


def test_the_new_kernel_file_is_part_of_the_build_and_its_range_is_the_gpu_tests():
    from openintel_amd import build
    assert "seeds.hip" in build.sources()
    src = open(os.path.join(ROOT, "openintel_amd", "csrc", "seeds.hip")).read()
    m = re.search(r"constexpr\s+uint32_t\s+NS_RANGE_ROWS\s*=\s*(\d+)\s*;", src)
    assert m and int(m.group(1)) == 2048
    import importlib.util
    spec = importlib.util.spec_from_file_location("_gpu_seed", os.path.join(ROOT, "tests", "test_gpu_seed.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.RANGE == int(m.group(1))
    for kernel in ("ns_init_kernel", "ns_score_kernel", "ns_pick_kernel", "vo_load_row4", "vo_chain4", "oi_wave_sum"):
        assert kernel in src, kernel


def test_the_emulation_of_the_gpu_tests_is_self_consistent():
    """the RNG against splitmix64's published first outputs for seed 0, and a hand-checked weight table"""
    import importlib.util
    import numpy as np
    spec = importlib.util.spec_from_file_location("_gpu_seed", os.path.join(ROOT, "tests", "test_gpu_seed.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    # splitmix64 from state 0: the first two outputs of the reference generator (Vigna) -- u(0, 0), u(0, 1) with seed 0
    assert mod._u(0, 0, 0) == 0xE220A8397B1DCDAF and mod._u(0, 0, 1) == 0x6E789E6AA1B965F4
    assert mod._mulhi((1 << 64) - 1, 10) == 9 and mod._mulhi(1 << 63, 7) == 3
    w = mod._weight(np.array([1.0, 0.0, -1.0, 2.0, -3.0, 0.5, np.nan, 1.0 - 2.0 ** -21], np.float32))
    assert w.tolist() == [0, 1 << 20, 1 << 21, 0, 1 << 21, 1 << 19, 0, 0]              # (0.5 rounds to even: 0)


def test_python_wrappers_exist_with_the_documented_defaults():
    import dataclasses
    import inspect
    from openintel_amd import batch, retriever
    sig = inspect.signature(retriever.HybridIndex.seed_narratives)
    assert list(sig.parameters) == ["self", "n_clusters", "method", "trials", "seed", "n_buckets", "stamp_origin", "bucket_width", "filter", "device"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["method"], d["trials"], d["seed"], d["n_buckets"], d["stamp_origin"], d["bucket_width"], d["filter"], d["device"]) == \
        ("kmeans++", 4, 0, 1, 0, 0, None, False)
    assert [f.name for f in dataclasses.fields(retriever.NarrativeSeeds)] == ["seeds", "rows", "found", "eligible", "potential"]
    assert list(inspect.signature(batch.discover_narratives).parameters) == ["index", "seeds", "threshold", "kw"]


def test_bad_arguments_are_refused_without_touching_a_device():
    import ctypes as C
    import numpy as np
    from openintel_amd import build, _lib
    build.build()
    lib = _lib.load()
    none = C.c_void_p(None)
    buf = np.zeros(64, dtype=np.uint64)
    p = _lib.ptr(buf)

    def call(k=4, method=0, trials=2, nb=1, width=0, reserved=0, spec=True, out=p, loc=_lib.OI_HOST):
        sp = C.byref(_lib.SeedSpec(method, trials, 0, 0, width, nb, reserved)) if spec else none
        return lib.oi_narratives_seed(none, k, sp, none, loc, out, none, none)

    def refused(rc, word):
        msg = lib.oi_last_error()
        assert rc == _lib.OI_ERR_INVALID_ARG and msg and word in msg, (rc, msg, word)

    refused(call(), b"null index")
    refused(call(k=256, trials=8), b"null index")
    refused(call(method=1, trials=1), b"null index")
    refused(call(nb=1024, width=1), b"null index")
    refused(call(spec=False), b"null spec")
    refused(call(k=0), b"n_clusters=0")
    refused(call(k=257), b"n_clusters=257")
    refused(call(method=2), b"method=2")
    refused(call(trials=0), b"trials=0")
    refused(call(trials=9), b"trials=9")
    refused(call(method=1, trials=2), b"trials=2")
    refused(call(reserved=7), b"reserved=7")
    refused(call(nb=0), b"n_buckets=0")
    refused(call(nb=1025, width=1), b"n_buckets=1025")
    refused(call(nb=3), b"n_buckets=3")
    refused(call(out=none), b"null buffer")
    refused(call(loc=5), b"location 5")
