"""CPU-side checks of the text -> term-id boundary (oi_text_terms, oi_query_terms, oi_index_set_text): the Python
restatement of the contract in include/openintel_hip.h -- pinned by fixed vectors before it judges anything -- the header,
the Python and Rust bindings, and the argument checks that run before any device call.  tests/test_gpu_text_terms.py
imports the restatement from here."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEXT_FUNCS = {"oi_text_terms": 11, "oi_query_terms": 11, "oi_index_set_text": 5}
HASH_BYTES = 64
M64 = (1 << 64) - 1


# ---------------------------------------------------------------- the restatement (header: "Text to term ids")
def fnv1a64(b: bytes) -> int:
    h = 0xcbf29ce484222325
    for c in b:
        h = ((h ^ c) * 0x100000001b3) & M64
    return h


def term_of(token, vocab: int) -> int:
    b = token.encode("ascii") if isinstance(token, str) else bytes(token)
    h = fnv1a64(b[:HASH_BYTES])
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & M64
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & M64
    h ^= h >> 33
    return ((h >> 32) * vocab) >> 32


def ref_text_terms(texts, vocab: int, off_dtype=np.uint64):
    """(term ids u32 in text order, offsets[n + 1]) of a list of str: oracle.pyref.tokens + the hash."""
    from oracle import pyref
    ids, offs, memo = [], [0], {}
    for t in texts:
        for tok in pyref.tokens(t):
            if tok not in memo:
                memo[tok] = term_of(tok, vocab)
            ids.append(memo[tok])
        offs.append(len(ids))
    return np.array(ids, dtype=np.uint32), np.array(offs, dtype=off_dtype)


# ---------------------------------------------------------------- 1. the yardstick is pinned first
def test_restatement_reproduces_the_fixed_vectors():
    assert fnv1a64(b"") == 0xcbf29ce484222325
    assert fnv1a64(b"a") == 0xaf63dc4c8601ec8c
    assert fnv1a64(b"foobar") == 0x85944171f73967e8
    V = 131072
    assert term_of("a", V) == 66885
    assert term_of("moon", V) == 24944
    assert term_of("x" * 64, V) == term_of("x" * 65, V) == term_of("x" * 64 + "y", V) == 54459
    assert term_of("x" * 63, V) != term_of("x" * 64, V)


def test_restatement_tokens_and_spread():
    ids, offs = ref_text_terms(["AAPL to the MOON", "", "abc", "def", "Kelvin İx aªb"], 1 << 20)
    assert offs.tolist() == [0, 4, 4, 5, 6, 11]
    V = 1 << 20
    assert ids.tolist() == [term_of(w, V) for w in ("aapl", "to", "the", "moon", "abc", "def", "kelvin", "i", "x", "a", "b")]
    # the finaliser does its job: 4096 distinct words land in about as many buckets as a uniform hash would give
    from openintel_amd import synth
    words, _ = synth.word_list()
    for vocab, lo in ((1000, 960), (4096, 2500), (131072, 3990), (1 << 20, 4070)):
        assert len({term_of(w, vocab) for w in words}) >= lo, vocab
    assert all(0 <= term_of(w, 7) < 7 for w in words[:200])
    assert term_of("moon", (1 << 32) - 1) < (1 << 32) - 1


# ---------------------------------------------------------------- 2. header, bindings, argument checks
def _header_code():
    hdr = open(os.path.join(ROOT, "include", "openintel_hip.h")).read()
    return hdr, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_declares_the_three_functions_and_the_constants():
    hdr, code = _header_code()
    for name, arity in TEXT_FUNCS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
        assert m, name
        assert m.group(1).count(",") + 1 == arity, name
    assert re.search(r"#define\s+OI_TEXT_TOKEN_HASH_BYTES\s+64u?\b", code)
    assert re.search(r"#define\s+OI_ABI_VERSION\s+1\b", code)
    # the contract is in the header word for word
    for needle in ("0xcbf29ce484222325", "0x100000001b3", "0xff51afd7ed558ccd", "0xc4ceb9fe1a85ec53", "E2 84 AA", "C4 B0"):
        assert needle in hdr, needle


def test_python_binding_and_the_hash_length():
    from openintel_amd import _lib
    import openintel_amd as oi
    for name, arity in TEXT_FUNCS.items():
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == arity, name
    _, code = _header_code()
    m = re.search(r"#define\s+OI_TEXT_TOKEN_HASH_BYTES\s+(\d+)u?\b", code)
    assert m and int(m.group(1)) == _lib.OI_TEXT_TOKEN_HASH_BYTES == HASH_BYTES
    for name in ("set_text", "query_terms", "search_text"):
        assert callable(getattr(oi.HybridIndex, name)), name
    assert callable(oi.text_terms)


def test_rust_binding_has_the_functions():
    src = open(os.path.join(ROOT, "integration", "rust", "src", "ffi.rs")).read()
    for name in TEXT_FUNCS:
        assert re.search(r"pub fn " + name + r"\s*\(", src), name
    lib = open(os.path.join(ROOT, "integration", "rust", "src", "lib.rs")).read()
    for name in ("fn build_from_texts", "fn query_terms"):
        assert name in lib, name


def test_bad_arguments_are_refused_without_touching_a_device():
    from openintel_amd import build, _lib
    build.build()
    lib = _lib.load()
    INVALID = _lib.OI_ERR_INVALID_ARG
    none = C.c_void_p(None)
    # every argument check comes before the handle is looked at, so a handle that is merely non-null gets that far
    page = C.create_string_buffer(4096)
    fake = C.cast(page, C.c_void_p)
    offs64 = np.zeros(2, dtype=np.uint64)
    offs32 = np.zeros(2, dtype=np.uint32)
    out = np.zeros(2, dtype=np.uint64)
    for fn, offs in ((lib.oi_text_terms, offs64), (lib.oi_query_terms, offs32)):
        o, r = _lib.ptr(offs), _lib.ptr(out)
        assert fn(none, none, o, 1, 0, 16, _lib.OI_HOST, none, 0, r, None) == INVALID and b"null ctx" in lib.oi_last_error()
        assert fn(fake, none, none, 1, 0, 16, _lib.OI_HOST, none, 0, r, None) == INVALID and b"null offsets" in lib.oi_last_error()
        assert fn(fake, none, o, 1, 0, 16, _lib.OI_HOST, none, 0, none, None) == INVALID and b"null offsets" in lib.oi_last_error()
        assert fn(fake, none, o, 1, 0, 0, _lib.OI_HOST, none, 0, r, None) == INVALID and b"vocab" in lib.oi_last_error()
        assert fn(fake, none, o, 1, 0, 16, 2, none, 0, r, None) == INVALID and b"location" in lib.oi_last_error()
        assert fn(fake, none, o, 1, 5, 16, _lib.OI_HOST, none, 0, r, None) == INVALID and b"null text blob" in lib.oi_last_error()
    o = _lib.ptr(offs64)
    assert lib.oi_index_set_text(none, none, o, 0, _lib.OI_HOST) == INVALID and b"null" in lib.oi_last_error()
    assert lib.oi_index_set_text(fake, none, none, 0, _lib.OI_HOST) == INVALID and b"null" in lib.oi_last_error()
    assert lib.oi_index_set_text(fake, none, o, 0, 7) == INVALID and b"location" in lib.oi_last_error()
    assert lib.oi_index_set_text(fake, none, o, 9, _lib.OI_HOST) == INVALID and b"null text blob" in lib.oi_last_error()


def test_offsets_that_do_not_fit_u32_are_refused_not_wrapped():
    import pytest
    from openintel_amd.retriever import _packed_texts
    blob = np.zeros(4, dtype=np.uint8)
    with pytest.raises(ValueError):
        _packed_texts((blob, np.array([0, 1 << 32], dtype=np.uint64)), np.uint32)
    dev, b, o, n, nbytes = _packed_texts((blob, np.array([0, 4], dtype=np.uint64)), np.uint32)
    assert (dev, o.dtype, o.tolist(), n, nbytes) == (False, np.uint32, [0, 4], 1, 4)
