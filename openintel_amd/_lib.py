"""ctypes binding of libopenintel_hip.so (include/openintel_hip.h).

There is no CPU fallback: if the library is missing or no gfx950 device is visible the
calls raise.  `python -m openintel_amd.build` (or `__graft_entry__.build()`) compiles it.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libopenintel_hip.so")
# (No environment override here: tests/ and bench.py always load THIS file.  The tools that time -DOI_ABLATION builds set
# LIB_PATH explicitly before first use -- tools/_ablation.py.)

OI_HOST, OI_DEVICE = 0, 1
OI_MAX_DEPTH = 1024
OI_MAX_DIM = 1024
OI_MAX_VOLUME_BUCKETS = 1024
OI_MAX_SUMMARY_CELLS = 1 << 18
OI_MAX_GROUP_KEYS = 65536
OI_MAX_GROUP_CELLS = 1 << 20
OI_MAX_CENTROIDS = 256
OI_SEED_KMEANSPP, OI_SEED_FARTHEST = 0, 1
OI_MAX_SEED_TRIALS = 8
OI_MAX_MENTION_TERMS = 64
OI_MAX_LABEL_TERMS = 64
OI_MAX_LABEL_TERM_CELLS = 1 << 28
OI_MENTION_AXIS_TIME, OI_MENTION_AXIS_KEY = 0, 1
OI_LABEL_AXIS_TIME, OI_LABEL_AXIS_KEY = 0, 1
OI_GROUP_RANK_TOTAL, OI_GROUP_RANK_SPEC, OI_GROUP_RANK_BULLISH, OI_GROUP_RANK_BEARISH = 0, 1, 2, 3
OI_BM25_BLOCK_DOCS = 32768
OI_N_CATALYST_KEYWORDS = 16
OI_TEXT_TOKEN_HASH_BYTES = 64
OI_COSINE_EXACT, OI_COSINE_SPLIT, OI_COSINE_SCREEN, OI_COSINE_SCREEN_COPY, OI_COSINE_SCREEN_STREAM = 0, 1, 2, 3, 4
OI_SCREEN_COPY_AUTO, OI_SCREEN_COPY_NEVER, OI_SCREEN_COPY_ALWAYS = 0, 1, 2

OI_ERR_INVALID_ARG = -1
OI_ERR_HIP = -2
OI_ERR_ANALYZER_MISMATCH = -3
OI_ERR_STATE = -5
OI_ERR_NO_DEVICE = -6
OI_ERR_UNSUPPORTED = -7
OI_ERR_OVERFLOW = -8
OI_ERR_COMM = -9
OI_COMM_ID_BYTES = 128


class OiError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__("libopenintel_hip error %d: %s" % (code, message))
        self.code = code
        self.message = message


class SocialCounters(C.Structure):
    _fields_ = [
        ("total", C.c_uint64),
        ("by_source", C.c_uint64 * 2),
        ("bullish", C.c_uint64),
        ("bearish", C.c_uint64),
        ("neutral", C.c_uint64),
        ("spec_count", C.c_uint64),
        ("polarity_sum", C.c_double),
    ]


class DocFilter(C.Structure):
    """oi_doc_filter: a document passes when (group & group_mask) == group_value and stamp_lo <= stamp <= stamp_hi."""
    _fields_ = [
        ("group_mask", C.c_uint32),
        ("group_value", C.c_uint32),
        ("stamp_lo", C.c_uint32),
        ("stamp_hi", C.c_uint32),
    ]


class VolumeSpec(C.Structure):
    """oi_volume_spec: count documents with sim >= threshold, per bucket (stamp - stamp_origin) // bucket_width."""
    _fields_ = [
        ("threshold", C.c_float),
        ("stamp_origin", C.c_uint32),
        ("bucket_width", C.c_uint32),
        ("n_buckets", C.c_uint32),
    ]


class SummarySpec(C.Structure):
    """oi_summary_spec: oi_volume_spec's time axis; threshold is every query's unless the call is given a thresholds array."""
    _fields_ = [
        ("threshold", C.c_float),
        ("stamp_origin", C.c_uint32),
        ("bucket_width", C.c_uint32),
        ("n_buckets", C.c_uint32),
    ]


class NarrativeSpec(C.Structure):
    """oi_narrative_spec: oi_summary_spec's four fields (one threshold for all clusters), then max_iters (1 .. 64)."""
    _fields_ = [
        ("threshold", C.c_float),
        ("stamp_origin", C.c_uint32),
        ("bucket_width", C.c_uint32),
        ("n_buckets", C.c_uint32),
        ("max_iters", C.c_uint32),
    ]


class NarrativeInfo(C.Structure):
    """oi_narrative_info: assignment steps run, converged (0 / 1), rows moved in the last step, rows assigned by it."""
    _fields_ = [
        ("iterations", C.c_uint32),
        ("converged", C.c_uint32),
        ("moved", C.c_uint64),
        ("assigned", C.c_uint64),
    ]


class SeedSpec(C.Structure):
    """oi_seed_spec: method (OI_SEED_*), trials (candidates per seed, 1 .. 8), the RNG seed, oi_narrative_spec's time axis,
    reserved (0).  32 bytes."""
    _fields_ = [
        ("method", C.c_uint32),
        ("trials", C.c_uint32),
        ("seed", C.c_uint64),
        ("stamp_origin", C.c_uint32),
        ("bucket_width", C.c_uint32),
        ("n_buckets", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class SeedInfo(C.Structure):
    """oi_seed_info: seeds found, reserved, eligible rows, the potential (sum of the weights) after the last seed.  24 bytes."""
    _fields_ = [
        ("found", C.c_uint32),
        ("reserved", C.c_uint32),
        ("eligible", C.c_uint64),
        ("potential", C.c_uint64),
    ]


class GroupsSpec(C.Structure):
    """oi_groups_spec: the key of a document is (group & key_mask) >> ctz(key_mask); top == 0 asks for dense records, top >= 1
    for the best `top` keys by rank_by among those with total >= max(min_total, 1)."""
    _fields_ = [
        ("threshold", C.c_float),
        ("key_mask", C.c_uint32),
        ("n_keys", C.c_uint32),
        ("top", C.c_uint32),
        ("rank_by", C.c_uint32),
        ("min_total", C.c_uint32),
    ]


class MentionSpec(C.Structure):
    """oi_mention_spec: axis TIME -- {stamp_origin, bucket_width, n_cells} are oi_summary_spec's time axis; axis KEY -- stamp_origin
    carries the key_mask, bucket_width is 0 and n_cells the number of keys."""
    _fields_ = [
        ("axis", C.c_uint32),
        ("stamp_origin", C.c_uint32),
        ("bucket_width", C.c_uint32),
        ("n_cells", C.c_uint32),
    ]


class LabelTermsSpec(C.Structure):
    """oi_label_terms_spec: records per cluster (1 .. OI_MAX_LABEL_TERMS), the smallest counts[t][c] of an eligible term (0 means
    1), reserved (0).  16 bytes."""
    _fields_ = [
        ("top", C.c_uint32),
        ("min_df", C.c_uint32),
        ("reserved", C.c_uint32 * 2),
    ]


class ExemplarSpec(C.Structure):
    """oi_exemplar_spec: posts per cluster (1 .. OI_MAX_DEPTH), reserved (0).  16 bytes."""
    _fields_ = [
        ("top", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
    ]


class LabelSummarySpec(C.Structure):
    """oi_label_summary_spec: axis TIME -- {stamp_origin, bucket_width, n_cells} are oi_summary_spec's time axis, top is 0; axis
    KEY -- stamp_origin carries the key_mask, bucket_width is 0, n_cells the number of keys, and top >= 1 asks for the best `top`
    keys by rank_by among those with total >= max(min_total, 1).  reserved is 0.  32 bytes."""
    _fields_ = [
        ("axis", C.c_uint32),
        ("stamp_origin", C.c_uint32),
        ("bucket_width", C.c_uint32),
        ("n_cells", C.c_uint32),
        ("top", C.c_uint32),
        ("rank_by", C.c_uint32),
        ("min_total", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


# oi_label_term: 24 bytes
LABEL_TERM_DTYPE = np.dtype([("term", "<u4"), ("df_cluster", "<u4"), ("df_assigned", "<u4"), ("reserved", "<u4"), ("excess", "<i8")])
assert LABEL_TERM_DTYPE.itemsize == 24


_P = C.c_void_p
_U32, _U64, _I = C.c_uint32, C.c_uint64, C.c_int

# name -> (restype, argtypes); every symbol include/openintel_hip.h declares
SIGNATURES = {
    "oi_abi_version": (_I, []),
    "oi_last_error": (C.c_char_p, []),
    "oi_create": (_I, [_I, C.POINTER(_P)]),
    "oi_create_like": (_I, [_P, C.POINTER(_P)]),
    "oi_destroy": (None, [_P]),
    "oi_set_stream": (_I, [_P, _P]),
    "oi_synchronize": (_I, [_P]),
    "oi_lexicon_analyze": (_I, [_P, _P, _P, _U64, _P, _P]),
    "oi_lexicon_analyze_device": (_I, [_P, _P, _P, _U64, _U64, _P, _P]),
    "oi_lexicon_summary_device": (_I, [_P, _P, _P, _U64, _U64, _P, C.c_double, _P, _P, C.POINTER(SocialCounters)]),
    "oi_workspace_bytes": (_I, [_P, C.POINTER(_U64), C.POINTER(_U64)]),
    "oi_set_overlap": (_I, [_P, _I]),
    "oi_set_screen_speculation": (_I, [_P, _I]),
    "oi_set_graph_replay": (_I, [_P, _I]),
    "oi_set_cosine_mode": (_I, [_P, _I]),
    "oi_catalyst_keyword": (C.c_char_p, [_U32]),
    "oi_headline_scan": (_I, [_P, _P, _P, _U64, _P, _U64, _P, _P, _U32, _P, _P, _P]),
    "oi_headline_scan_device": (_I, [_P, _P, _P, _U64, _U64, _P, _U64, _P, _P, _U32, _P, _P, _P]),
    "oi_headline_scan_rows": (_I, [_P, _P, _P, _U64, _P, _U32, _P, _P, _P, _P, _P, _P, _P, _P]),
    "oi_social_summary": (_I, [_P, _P, _U64, _P, _P, _U64, C.c_double, _I, C.POINTER(SocialCounters)]),
    "oi_social_summary_segmented": (_I, [_P, _P, _P, _P, _U64, _P, _U64, C.c_double, _I, _P]),
    "oi_lexicon_scan_segments_device": (_I, [_P, _P, _P, _U64, _U64, _P, _P, _U64, C.c_double, _P, _P, _P]),
    "oi_index_create": (_I, [_P, _U64, _U32, _U32, _U32, C.POINTER(_P)]),
    "oi_index_destroy": (None, [_P]),
    "oi_index_view": (_I, [_P, _P, C.POINTER(_P)]),
    "oi_index_set_embeddings": (_I, [_P, _P, _I, _I]),
    "oi_index_set_embeddings_bf16": (_I, [_P, _P, _I]),
    "oi_index_set_forward": (_I, [_P, _P, _P, _I]),
    "oi_index_local_stats": (_I, [_P, C.POINTER(_U64), _P]),
    "oi_index_set_max_query_terms": (_I, [_P, _U32]),
    "oi_index_set_bm25_mode": (_I, [_P, _I]),
    "oi_index_long_rows": (_I, [_P, C.POINTER(C.c_uint32)]),
    "oi_index_set_screen_copy": (_I, [_P, _I]),
    "oi_index_bytes": (_I, [_P, C.POINTER(_U64), C.POINTER(_U64), C.POINTER(_U64)]),
    "oi_index_finalize": (_I, [_P, _U64, _U64, _P]),
    "oi_search_lists": (_I, [_P, _P, _P, _P, _U32, _U32, _I, _P, _P, _P, _P, _P, _P]),
    "oi_search_lists_packed": (_I, [_P, _P, _P, _P, _U32, _U32, _I, _P]),
    "oi_fuse_packed": (_I, [_P, _P, _U32, _U32, _U32, _U32, _I, _P, _P, _P]),
    "oi_merge_lists": (_I, [_P, _P, _P, _P, _U32, _U32, _U32, _I, _P, _P, _P]),
    "oi_rrf_fuse": (_I, [_P, _P, _P, _P, _P, _U32, _U32, _U32, _I, _P, _P, _P]),
    "oi_search": (_I, [_P, _P, _P, _P, _U32, _U32, _U32, _I, _P, _P, _P]),
    "oi_comm_unique_id": (_I, [_P]),
    "oi_comm_create": (_I, [_P, _P, _U32, _U32, C.POINTER(_P)]),
    "oi_comm_destroy": (None, [_P]),
    "oi_index_finalize_sharded": (_I, [_P, _P]),
    "oi_search_sharded": (_I, [_P, _P, _P, _P, _P, _U32, _U32, _U32, _I, _P, _P, _P]),
    "oi_index_set_doc_attrs": (_I, [_P, _P, _P, _I]),
    "oi_search_lists_filtered": (_I, [_P, _P, _P, _P, _U32, _U32, _P, _I, _P, _P, _P, _P, _P, _P]),
    "oi_search_lists_packed_filtered": (_I, [_P, _P, _P, _P, _U32, _U32, _P, _I, _P]),
    "oi_search_filtered": (_I, [_P, _P, _P, _P, _U32, _U32, _U32, _P, _I, _P, _P, _P]),
    "oi_search_sharded_filtered": (_I, [_P, _P, _P, _P, _P, _U32, _U32, _U32, _P, _I, _P, _P, _P]),
    "oi_collapse_lists": (_I, [_P, _P, _P, _P, _U32, _U32, C.c_float, _U32, _I, _P, _P, _P, _P]),
    "oi_search_collapsed": (_I, [_P, _P, _P, _P, _U32, _U32, _U32, _U32, C.c_float, _P, _I, _P, _P, _P, _P]),
    "oi_similar_volume": (_I, [_P, _P, _U32, _P, _P, _I, _P]),
    "oi_index_set_signals": (_I, [_P, _P, _P, _P, C.c_double, _I]),
    "oi_similar_summary": (_I, [_P, _P, _U32, _P, _P, _P, _I, _P]),
    "oi_similar_groups": (_I, [_P, _P, _U32, _P, _P, _P, _I, _P, _P, _P, _P]),
    "oi_similar_share": (_I, [_P, _P, _U32, _P, _P, _P, _I, _P, _P]),
    "oi_mention_summary": (_I, [_P, _P, _P, _U32, _P, _P, _P, _I, _P]),
    "oi_label_sums": (_I, [_P, _P, _U32, _I, _P, _P]),
    "oi_centroids_from_sums": (_I, [_P, _P, _P, _P, _U32, _U32, _I, _P]),
    "oi_narratives_fit": (_I, [_P, _P, _U32, _P, _P, _I, _P, _P, _P, _P]),
    "oi_narratives_seed": (_I, [_P, _U32, _P, _P, _I, _P, _P, _P]),
    "oi_label_term_counts": (_I, [_P, _P, _U32, _I, _P, _P]),
    "oi_label_terms_rank": (_I, [_P, _P, _P, _U32, _U32, _P, _I, _P, _P]),
    "oi_label_terms": (_I, [_P, _P, _U32, _P, _I, _P, _P, _P]),
    "oi_label_exemplars": (_I, [_P, _P, _P, _U32, _P, _P, _I, _P, _P, _P]),
    "oi_label_summary": (_I, [_P, _P, _U32, _P, _P, _I, _P, _P, _P, _P]),
    "oi_text_terms": (_I, [_P, _P, _P, _U64, _U64, _U32, _I, _P, _U64, _P, C.POINTER(_U64)]),
    "oi_query_terms": (_I, [_P, _P, _P, _U32, _U32, _U32, _I, _P, _U64, _P, C.POINTER(_U64)]),
    "oi_index_set_text": (_I, [_P, _P, _P, _U64, _I]),
    "oi_pipeline_create": (_I, [_P, _P, _U32, _U32, _U32, _U32, _U32, C.POINTER(_P)]),
    "oi_pipeline_destroy": (None, [_P]),
    "oi_pipeline_submit": (_I, [_P, _P, _P, _P, _U32, _I, _P, _P, _P, C.POINTER(_U64)]),
    "oi_pipeline_wait": (_I, [_P, _U64, _I]),
    "oi_pipeline_drain": (_I, [_P]),
    "oi_pipeline_workspace_bytes": (_I, [_P, C.POINTER(_U64), C.POINTER(_U64)]),
    "oi_pipeline_concurrent_streams": (_I, [_P, C.POINTER(_U32), C.POINTER(_U32)]),
    "oi_pipeline_profile_reset": (_I, [_P, _I]),
    "oi_pipeline_profile_read": (_I, [_P, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_U64)]),
    "oi_screen_probe": (_I, [_P, _P, _U32, _U64, _U32, _P, _P]),
    "oi_profile_reset": (_I, [_P, _I]),
    "oi_profile_read": (_I, [_P, C.c_char_p, C.POINTER(C.c_double), C.POINTER(_U64)]),
}

# exports that are NOT part of the C ABI (no declaration in the header): the switch between the int8 route's two second tiers
# (A/B runs, tests) and the tests' views of an index's residual plane, of its BM25 structures, of its long rows in the order the
# rescoring reads them, and of the residual tier's staging and rescreen launches
INTERNAL = {
    "oi_internal_residual_rescreen": (_I, [_P, _P, _U32, _P, _P, _U64, _U32, _P, _P, _P, _P, _P]),
    "oi_internal_set_rescreen_tier": (_I, [_P, _I]),
    "oi_internal_residual_plane": (_I, [_P, _I, _P, _P, _P, C.POINTER(_U64)]),
    "oi_internal_bm25_index": (_I, [_P, C.POINTER(_U64), C.POINTER(_U32), C.POINTER(C.c_float), _P, _P, _P, _P, _P]),
    "oi_internal_long_list": (_I, [_P, C.POINTER(_U32), _P]),
}

_lib = None


def load() -> C.CDLL:
    """Load the shared library and bind every declared symbol.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libopenintel_hip.so is not built (%s). Run `python -m openintel_amd.build`. "
            "openintel_amd has no CPU fallback." % LIB_PATH)
    # torch bundles its own HIP runtime (same soname, libamdhip64.so.7).  Two HIP runtimes in one
    # process cannot share a GPU, so when torch is present it must be loaded FIRST: the dynamic
    # linker then resolves this library's libamdhip64.so.7 to the copy torch already mapped, and
    # torch tensors / streams are valid arguments.  A host without torch (the Rust shim of
    # INTEGRATION.md) simply gets the system ROCm runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(SIGNATURES.items()) + list(INTERNAL.items()):
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().oi_last_error()
        raise OiError(rc, msg.decode("utf-8", "replace") if msg else "")


def ptr(x):
    """Device or host address of a torch tensor / numpy array / None."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(x.ctypes.data)
