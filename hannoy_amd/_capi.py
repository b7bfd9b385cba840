"""ctypes binding of the C ABI in include/hannoy_amd.h (hannoy_amd/libhannoy_amd.so).

The shared library is the product: there is no Python or CPU fallback.  Importing works without a
GPU (so that symbol/ABI checks can run anywhere); every computing call needs a gfx950 device and
raises HannoyError otherwise.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HNY_LIB") or os.path.join(HERE, "libhannoy_amd.so")

COSINE, EUCLIDEAN, MANHATTAN, HAMMING, BQ_COSINE, BQ_EUCLIDEAN, BQ_MANHATTAN = range(7)
METRIC_NAMES = ["cosine", "euclidean", "manhattan", "hamming", "binary quantized cosine",
                "binary quantized euclidean", "binary quantized manhattan"]

OK, ERR_INVALID_ARG, ERR_CANCELLED, ERR_MISSING_KEY, ERR_INVALID_DIM = 0, -1, -2, -3, -4
ERR_UNSUPPORTED, ERR_NO_DEVICE, ERR_DEVICE, ERR_OOM = -5, -6, -7, -8

EXPORTED = [
    "hny_build", "hny_graph_free", "hny_builder_create", "hny_builder_reset",
    "hny_builder_next_batch", "hny_builder_search", "hny_builder_apply", "hny_builder_sync",
    "hny_builder_finish", "hny_builder_destroy", "hny_builder_set_profiling", "hny_batch_size", "hny_builder_distances",
    "hny_builder_search_knn", "hny_vector_bytes", "hny_header_bytes", "hny_encode_vectors",
    "hny_encode_kv", "hny_last_error", "hny_version", "hny_draw_levels", "hny_build_incremental",
    "hny_builder_create_incremental", "hny_builder_fill_gaps", "hny_encode_vectors_gpu",
    "hny_builder_nns", "hny_draw_levels_from_seed", "hny_builder_load",
    "hny_builder_apply_begin", "hny_builder_apply_deferred", "hny_builder_apply_merge",
    "hny_builder_exch_stride_u64", "hny_builder_stream", "hny_default_batch_max", "hny_selftest_lane_ops",
    "hny_lmdb_writer_open", "hny_lmdb_writer_put", "hny_lmdb_writer_finish", "hny_lmdb_writer_abort",
    "hny_lmdb_open", "hny_lmdb_stat_get", "hny_lmdb_get", "hny_lmdb_scan", "hny_lmdb_close",
    "hny_multi_builder_create", "hny_multi_builder_run", "hny_multi_builder_set_profiling",
    "hny_multi_builder_world", "hny_multi_builder_collectives", "hny_multi_builder_replica",
    "hny_multi_builder_destroy", "hny_abi_sizes", "hny_set_graph_cache",
    "hny_build_f32", "hny_build_incremental_f32", "hny_builder_create_f32", "hny_builder_load_f32",
    "hny_builder_export_items", "hny_builder_search_knn_f32", "hny_builder_nns_f32",
    "hny_builder_create_update", "hny_builder_update", "hny_builder_finish_delta", "hny_graph_delta_free",
    "hny_builder_exact_knn", "hny_builder_exact_knn_f32",
    "hny_builder_nns_filtered", "hny_builder_nns_filtered_f32",
    "hny_builder_exact_knn_filtered", "hny_builder_exact_knn_filtered_f32", "hny_builder_exact_rows_read",
    "hny_distance_keeps_links", "hny_builder_create_changed_distance", "hny_builder_recode_items",
    "hny_builder_nns_bitsets", "hny_builder_nns_bitsets_f32",
    "hny_builder_exact_knn_bitsets", "hny_builder_exact_knn_bitsets_f32",
    "hny_builder_exact_range", "hny_builder_exact_range_f32", "hny_builder_exact_range_count",
    "hny_builder_exact_range_count_f32", "hny_range_result_free",
    "hny_builder_exact_range_filtered", "hny_builder_exact_range_filtered_f32",
    "hny_builder_exact_range_count_filtered", "hny_builder_exact_range_count_filtered_f32",
    "hny_builder_exact_range_bitsets", "hny_builder_exact_range_bitsets_f32",
    "hny_builder_exact_range_count_bitsets", "hny_builder_exact_range_count_bitsets_f32",
    "hny_builder_finish_encoded", "hny_encoded_links_free", "hny_encode_kv_encoded",
    "hny_builder_finish_delta_encoded", "hny_encoded_delta_free",
    "hny_builder_load_encoded", "hny_builder_load_encoded_f32", "hny_builder_create_incremental_encoded",
    "hny_build_incremental_encoded", "hny_encoded_links_measure", "hny_lmdb_read_links",
]
ERR_IO = -9
NNS_NONE = 0xFFFFFFFF  # by_item: the reference returns None
NNS_FILTER_NONE = 0xFFFFFFFF  # hny_query_filters.filter_of: no .candidates() for this query
RANGE_NONE = 0xFFFFFFFFFFFFFFFF  # exact_range_count by_item: the reference returns None


CANCEL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)


class QueryOpts(C.Structure):
    _fields_ = [("k", C.c_uint32), ("ef_search", C.c_uint32), ("has_candidates", C.c_int32),
                ("candidates", C.c_void_p), ("n_candidates", C.c_uint64), ("linear_below", C.c_uint32),
                ("linear_below_ratio", C.c_float), ("cancel", CANCEL_FN), ("cancel_ctx", C.c_void_p),
                ("did_cancel", C.POINTER(C.c_int32))]


class QueryFilters(C.Structure):
    """hny_query_filters; struct_size is the guard (the struct is not part of hny_abi_sizes)"""
    _fields_ = [("struct_size", C.c_uint32), ("n_filters", C.c_uint32), ("offsets", C.c_void_p),
                ("ids", C.c_void_p), ("filter_of", C.c_void_p)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(QueryFilters)

    @classmethod
    def pack(cls, filters, filter_of):
        """`filters`: a list of id arrays; `filter_of`: one int per query, -1 or NNS_FILTER_NONE = none.
        Returns (struct, arrays the struct points into)"""
        arrs = [u32_ids(f).ravel() for f in filters]
        offsets = np.zeros(len(arrs) + 1, np.uint64)
        if arrs:
            offsets[1:] = np.cumsum([len(a) for a in arrs], dtype=np.uint64)
        ids = np.concatenate(arrs) if arrs else np.zeros(0, np.uint32)
        ids = np.ascontiguousarray(ids, np.uint32)
        fo = np.asarray(filter_of, np.int64).ravel()
        fo = np.ascontiguousarray(np.where(fo < 0, NNS_FILTER_NONE, fo), np.uint32)
        s = cls()
        s.n_filters, s.offsets, s.filter_of = len(arrs), _p(offsets).value, _p(fo).value
        s.ids = _p(ids).value if len(ids) else None
        return s, (offsets, ids, fo)


def pack_id_bits(masks, n_bits=None):
    """filters as bitsets over item ids: a bool array [n_filters, n_bits] packed little-endian (item id i is bit
    i & 31 of word i >> 5), or an already packed uint32 array [n_filters, words] with `n_bits`.  Returns (uint32
    [n_filters, words], n_bits)"""
    m = np.asarray(masks)
    if m.ndim != 2:
        raise ValueError("filter bitsets are a 2-d array, one row per filter")
    if m.dtype == np.bool_:
        if n_bits is not None and int(n_bits) != m.shape[1]:
            raise ValueError(f"n_bits {n_bits} for bool masks of {m.shape[1]} columns")
        nb = m.shape[1]
        if nb % 32:
            m = np.pad(m, ((0, 0), (0, -nb % 32)))
        bits = np.packbits(m, axis=1, bitorder="little").view("<u4") if nb else np.zeros((len(m), 0), np.uint32)
        return np.ascontiguousarray(bits, np.uint32), nb
    if m.dtype != np.uint32:
        raise ValueError(f"filter bitsets are bool or packed uint32, not {m.dtype}")
    if n_bits is None:
        raise ValueError("packed filter bitsets need n_bits")
    return np.ascontiguousarray(m), int(n_bits)


class QueryBitsets(C.Structure):
    """hny_query_bitsets; struct_size is the guard (the struct is not part of hny_abi_sizes)"""
    _fields_ = [("struct_size", C.c_uint32), ("n_filters", C.c_uint32), ("n_bits", C.c_uint64),
                ("stride_words", C.c_uint64), ("bits", C.c_void_p), ("filter_of", C.c_void_p)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(QueryBitsets)

    @classmethod
    def pack(cls, bits, n_bits, filter_of):
        """`bits`: uint32 [n_filters, words] (rows may be longer than ceil(n_bits / 32): the row length is the
        stride); `filter_of`: one int per query, -1 or NNS_FILTER_NONE = none.  Returns (struct, arrays the struct
        points into), filter_of last as in QueryFilters.pack"""
        bits, n_bits = pack_id_bits(bits, n_bits)
        fo = np.asarray(filter_of, np.int64).ravel()
        fo = np.ascontiguousarray(np.where(fo < 0, NNS_FILTER_NONE, fo), np.uint32)
        s = cls()
        s.n_filters, s.n_bits, s.stride_words = bits.shape[0], n_bits, bits.shape[1]
        s.bits = _p(bits).value if bits.size else None
        s.filter_of = _p(fo).value
        return s, (bits, n_bits, fo)


class RangeOpts(C.Structure):
    """hny_range_opts; struct_size is the guard (the struct is not part of hny_abi_sizes)"""
    _fields_ = [("struct_size", C.c_uint32), ("has_candidates", C.c_int32), ("candidates", C.c_void_p),
                ("n_candidates", C.c_uint64), ("radius", C.c_void_p), ("max_total", C.c_uint64),
                ("cancel", CANCEL_FN), ("cancel_ctx", C.c_void_p), ("did_cancel", C.POINTER(C.c_int32))]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(RangeOpts)


class RangeResult(C.Structure):
    """hny_range_result: owned by the library (hny_range_result_free)"""
    _fields_ = [("n_queries", C.c_uint64), ("offsets", C.POINTER(C.c_uint64)), ("ids", C.POINTER(C.c_uint32)),
                ("dists", C.POINTER(C.c_float)), ("is_none", C.POINTER(C.c_uint8))]


class HannoyError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"hannoy_amd error {code}: {msg}")
        self.code = code


class BuildCancelled(HannoyError):
    """Error::BuildCancelled (/root/reference/src/error.rs:58-59)"""


PROGRESS_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_uint64, C.c_uint64)
KV_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8),
                      C.c_size_t)


class LmdbStat(C.Structure):
    _fields_ = [("page_size", C.c_uint32), ("depth", C.c_uint32), ("branch_pages", C.c_uint64),
                ("leaf_pages", C.c_uint64), ("overflow_pages", C.c_uint64), ("entries", C.c_uint64),
                ("last_pgno", C.c_uint64), ("txnid", C.c_uint64), ("map_size", C.c_uint64)]


class BuildOpts(C.Structure):
    _fields_ = [("metric", C.c_int32), ("dim", C.c_uint32), ("M", C.c_uint32), ("M0", C.c_uint32),
                ("ef_construction", C.c_uint32), ("alpha", C.c_float), ("seed", C.c_uint64),
                ("cancel", CANCEL_FN), ("cancel_ctx", C.c_void_p),
                ("progress", PROGRESS_FN), ("progress_ctx", C.c_void_p),
                ("batch_frac", C.c_double), ("batch_max", C.c_uint32), ("device", C.c_int32),
                ("x86_order", C.c_int32), ("n_gpus", C.c_int32), ("devices", C.POINTER(C.c_int32)),
                ("schedule", C.c_uint32), ("reserved_", C.c_uint32)]


SCHED_NO_SHUFFLE, SCHED_LEVEL_ORDER_ID, SCHED_UPDATE_NO_RAMP = 1, 2, 4  # hny_build_opts.schedule (HNY_SCHED_*)


class Items(C.Structure):
    _fields_ = [("n", C.c_uint64), ("ids", C.c_void_p), ("vectors", C.c_void_p),
                ("stride", C.c_size_t), ("headers", C.c_void_p), ("header_size", C.c_size_t),
                ("levels", C.c_void_p)]


class GraphStruct(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("rec_item", C.POINTER(C.c_uint32)),
                ("rec_layer", C.POINTER(C.c_uint8)), ("rec_offset", C.POINTER(C.c_uint64)),
                ("neighbours", C.POINTER(C.c_uint32)), ("entry_points", C.POINTER(C.c_uint32)),
                ("n_entry_points", C.c_uint32), ("max_level", C.c_uint32),
                ("n_links_added", C.c_uint64), ("n_distance_evals", C.c_uint64),
                ("n_evals_walk", C.c_uint64), ("n_evals_prune", C.c_uint64),
                ("n_evals_apply", C.c_uint64), ("n_batches", C.c_uint64),
                ("t_upload_s", C.c_double), ("t_build_s", C.c_double), ("t_export_s", C.c_double),
                ("n_tie_pool_overflow", C.c_uint64),
                ("t_walk_kernels_s", C.c_double), ("t_prune_kernels_s", C.c_double),
                ("t_sort_kernels_s", C.c_double), ("t_apply_kernels_s", C.c_double),
                ("n_walk_launches", C.c_uint64)]


class PrevGraph(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("rec_item", C.c_void_p), ("rec_layer", C.c_void_p),
                ("rec_offset", C.c_void_p), ("neighbours", C.c_void_p), ("entry_points", C.c_void_p),
                ("n_entry_points", C.c_uint32), ("max_level", C.c_uint32)]


class Update(C.Structure):
    """hny_update; struct_size is the guard (the struct is not part of hny_abi_sizes)"""
    _fields_ = [("struct_size", C.c_uint32), ("vectors_are_f32", C.c_int32), ("n_upsert", C.c_uint64),
                ("upsert_ids", C.c_void_p), ("vectors", C.c_void_p), ("stride", C.c_size_t),
                ("headers", C.c_void_p), ("header_size", C.c_size_t), ("levels", C.c_void_p),
                ("seed", C.c_uint64), ("n_delete", C.c_uint64), ("delete_ids", C.c_void_p)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(Update)


class ChangeDistance(C.Structure):
    """hny_change_distance; struct_size is the guard (the struct is not part of hny_abi_sizes)"""
    _fields_ = [("struct_size", C.c_uint32), ("new_metric", C.c_int32), ("levels", C.c_void_p),
                ("seed", C.c_uint64), ("update", C.POINTER(Update))]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(ChangeDistance)


class GraphDeltaStruct(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("rec_item", C.POINTER(C.c_uint32)),
                ("rec_layer", C.POINTER(C.c_uint8)), ("rec_offset", C.POINTER(C.c_uint64)),
                ("neighbours", C.POINTER(C.c_uint32)), ("n_removed", C.c_uint64),
                ("removed_item", C.POINTER(C.c_uint32)), ("removed_layer", C.POINTER(C.c_uint8)),
                ("entry_points", C.POINTER(C.c_uint32)), ("n_entry_points", C.c_uint32),
                ("max_level", C.c_uint32), ("n_records_total", C.c_uint64), ("t_export_s", C.c_double)]


class EncodedLinksStruct(C.Structure):
    """hny_encoded_links: library-owned and read-only here, not part of hny_abi_sizes"""
    _fields_ = [("n_records", C.c_uint64), ("rec_item", C.POINTER(C.c_uint32)),
                ("rec_layer", C.POINTER(C.c_uint8)), ("val_offset", C.POINTER(C.c_uint64)),
                ("values", C.POINTER(C.c_uint8)), ("entry_points", C.POINTER(C.c_uint32)),
                ("n_entry_points", C.c_uint32), ("max_level", C.c_uint32),
                ("n_links_added", C.c_uint64), ("n_evals_walk", C.c_uint64), ("n_batches", C.c_uint64),
                ("t_export_s", C.c_double), ("t_device_s", C.c_double), ("t_download_s", C.c_double),
                ("bytes_downloaded", C.c_uint64)]


class EncodedDeltaStruct(C.Structure):
    """hny_encoded_delta: library-owned and read-only here, not part of hny_abi_sizes"""
    _fields_ = [("links", EncodedLinksStruct), ("n_removed", C.c_uint64),
                ("removed_item", C.POINTER(C.c_uint32)), ("removed_layer", C.POINTER(C.c_uint8)),
                ("n_records_total", C.c_uint64)]


class Batch(C.Structure):
    _fields_ = [("first", C.c_uint64), ("count", C.c_uint32), ("level", C.c_uint32),
                ("n_layers", C.c_uint32), ("sel_stride_u64", C.c_uint32)]


_lib = None


def load_library():
    """Loads the HIP extension; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch wheels bundle their own libamdhip64.  If this library were
    # loaded first it would register its kernels with /opt/rocm's runtime and later calls could bind
    # to torch's (global scope) — "no HIP device" / invalid device function.  Importing torch first
    # (when it is installed) makes every HIP symbol resolve to the one runtime torch also uses, which
    # the multi-GPU driver needs anyway (torch tensors are handed to the C ABI as device pointers).
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    # HNY_LIB: another build of this same library (python -m hannoy_amd.buildlib --out PATH), for A/B
    # measurements of two kernel variants on one box (scripts/r2_ab_lib.sh); still no CPU fallback
    lib_path = os.environ.get("HNY_LIB") or LIB_PATH
    if not os.path.exists(lib_path):
        raise ImportError(
            f"{lib_path} is missing: build it with `python -m hannoy_amd.buildlib` "
            "(hipcc --offload-arch=gfx950). hannoy_amd has no CPU fallback.")
    L = C.CDLL(lib_path)
    vp = C.c_void_p
    L.hny_build.restype = C.c_int
    L.hny_build.argtypes = [C.POINTER(BuildOpts), C.POINTER(Items), C.POINTER(C.POINTER(GraphStruct))]
    L.hny_graph_free.argtypes = [C.POINTER(GraphStruct)]
    L.hny_build_incremental.restype = C.c_int
    L.hny_build_incremental.argtypes = [C.POINTER(BuildOpts), C.POINTER(Items), vp, C.c_uint64, vp,
                                        C.c_uint64, C.POINTER(PrevGraph),
                                        C.POINTER(C.POINTER(GraphStruct))]
    L.hny_builder_create_incremental.restype = C.c_int
    L.hny_builder_create_incremental.argtypes = [C.POINTER(BuildOpts), C.POINTER(Items), vp, C.c_uint64,
                                                 vp, C.c_uint64, C.POINTER(PrevGraph), C.POINTER(vp)]
    L.hny_builder_load.restype = C.c_int
    L.hny_builder_load.argtypes = [C.POINTER(BuildOpts), C.POINTER(Items), C.POINTER(PrevGraph), C.POINTER(vp)]
    L.hny_builder_fill_gaps.restype = C.c_int
    L.hny_builder_fill_gaps.argtypes = [vp]
    L.hny_builder_create.restype = C.c_int
    L.hny_builder_create.argtypes = [C.POINTER(BuildOpts), C.POINTER(Items), C.POINTER(vp)]
    for name in ("hny_builder_reset", "hny_builder_sync"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [vp]
    L.hny_builder_set_profiling.restype = C.c_int
    L.hny_builder_set_profiling.argtypes = [vp, C.c_int]
    L.hny_builder_next_batch.restype = C.c_int
    L.hny_builder_next_batch.argtypes = [vp, C.POINTER(Batch)]
    L.hny_builder_search.restype = C.c_int
    L.hny_builder_search.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    L.hny_builder_apply.restype = C.c_int
    L.hny_builder_apply.argtypes = [vp, vp]
    L.hny_builder_apply_begin.restype = C.c_int
    L.hny_builder_apply_begin.argtypes = [vp, vp, C.POINTER(C.c_uint32)]
    L.hny_builder_apply_deferred.restype = C.c_int
    L.hny_builder_apply_deferred.argtypes = [vp, C.c_uint32, C.c_uint32, vp]
    L.hny_builder_apply_merge.restype = C.c_int
    L.hny_builder_apply_merge.argtypes = [vp, vp, C.c_uint32, C.c_uint32]
    L.hny_builder_exch_stride_u64.restype = C.c_uint32
    L.hny_builder_exch_stride_u64.argtypes = [vp]
    L.hny_builder_finish.restype = C.c_int
    L.hny_builder_finish.argtypes = [vp, C.POINTER(C.POINTER(GraphStruct))]
    L.hny_builder_destroy.argtypes = [vp]
    L.hny_draw_levels.restype = C.c_int
    L.hny_draw_levels.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, vp]
    L.hny_batch_size.restype = C.c_uint32
    L.hny_batch_size.argtypes = [C.c_double, C.c_uint32, C.c_uint64]
    L.hny_builder_distances.restype = C.c_int
    L.hny_builder_distances.argtypes = [vp, C.c_uint64, vp, vp, vp]
    L.hny_builder_search_knn.restype = C.c_int
    L.hny_builder_search_knn.argtypes = [vp, C.c_uint64, vp, C.c_size_t, vp, C.c_uint32, C.c_uint32,
                                         vp, vp, vp]
    L.hny_builder_nns.restype = C.c_int
    L.hny_builder_nns.argtypes = [vp, C.POINTER(QueryOpts), C.c_uint64, vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.hny_draw_levels_from_seed.restype = C.c_int
    L.hny_draw_levels_from_seed.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint64, vp]
    L.hny_vector_bytes.restype = C.c_size_t
    L.hny_vector_bytes.argtypes = [C.c_int32, C.c_uint32]
    L.hny_header_bytes.restype = C.c_size_t
    L.hny_header_bytes.argtypes = [C.c_int32]
    L.hny_encode_vectors.restype = C.c_int
    L.hny_encode_vectors.argtypes = [C.c_int32, C.c_uint32, C.c_uint64, vp, vp, vp]
    L.hny_encode_vectors_gpu.restype = C.c_int
    L.hny_encode_vectors_gpu.argtypes = [C.c_int32, C.c_uint32, C.c_uint64, vp, vp, vp, C.c_int32]
    L.hny_encode_kv.restype = C.c_int
    L.hny_encode_kv.argtypes = [C.POINTER(GraphStruct), C.POINTER(BuildOpts), C.POINTER(Items),
                                C.c_uint16, C.c_int, KV_SINK, vp]
    L.hny_lmdb_writer_open.restype = C.c_int
    L.hny_lmdb_writer_open.argtypes = [C.c_char_p, C.c_uint32, C.c_uint64, C.c_char_p, C.POINTER(vp)]
    L.hny_lmdb_writer_put.restype = C.c_int
    L.hny_lmdb_writer_put.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.hny_lmdb_writer_finish.restype = C.c_int
    L.hny_lmdb_writer_finish.argtypes = [vp]
    L.hny_lmdb_writer_abort.argtypes = [vp]
    L.hny_lmdb_open.restype = C.c_int
    L.hny_lmdb_open.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(vp)]
    L.hny_lmdb_stat_get.restype = C.c_int
    L.hny_lmdb_stat_get.argtypes = [vp, C.POINTER(LmdbStat)]
    L.hny_lmdb_get.restype = C.c_int
    L.hny_lmdb_get.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
    L.hny_lmdb_scan.restype = C.c_int
    L.hny_lmdb_scan.argtypes = [vp, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, KV_SINK, vp]
    L.hny_lmdb_close.argtypes = [vp]
    L.hny_last_error.restype = C.c_char_p
    L.hny_version.restype = C.c_char_p
    L.hny_multi_builder_create.restype = C.c_int
    L.hny_multi_builder_create.argtypes = [C.POINTER(BuildOpts), C.POINTER(Items), C.POINTER(vp)]
    L.hny_multi_builder_run.restype = C.c_int
    L.hny_multi_builder_run.argtypes = [vp, C.POINTER(C.POINTER(GraphStruct))]
    L.hny_multi_builder_set_profiling.restype = C.c_int
    L.hny_multi_builder_set_profiling.argtypes = [vp, C.c_int]
    L.hny_multi_builder_world.restype = C.c_uint32
    L.hny_multi_builder_world.argtypes = [vp]
    L.hny_multi_builder_collectives.restype = C.c_uint64
    L.hny_multi_builder_collectives.argtypes = [vp]
    L.hny_multi_builder_replica.restype = vp
    L.hny_multi_builder_replica.argtypes = [vp, C.c_uint32]
    L.hny_multi_builder_destroy.argtypes = [vp]
    for name, base in (("hny_build_f32", "hny_build"), ("hny_build_incremental_f32", "hny_build_incremental"),
                       ("hny_builder_create_f32", "hny_builder_create"), ("hny_builder_load_f32", "hny_builder_load")):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = getattr(L, base).argtypes
    el = C.POINTER(EncodedLinksStruct)
    for name in ("hny_builder_load_encoded", "hny_builder_load_encoded_f32"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.POINTER(BuildOpts), C.POINTER(Items), el, C.POINTER(vp)]
    L.hny_builder_create_incremental_encoded.restype = C.c_int
    L.hny_builder_create_incremental_encoded.argtypes = [C.POINTER(BuildOpts), C.POINTER(Items), vp, C.c_uint64, vp,
                                                         C.c_uint64, el, C.POINTER(vp)]
    L.hny_build_incremental_encoded.restype = C.c_int
    L.hny_build_incremental_encoded.argtypes = [C.POINTER(BuildOpts), C.POINTER(Items), vp, C.c_uint64, vp, C.c_uint64,
                                                el, C.POINTER(C.POINTER(GraphStruct))]
    L.hny_encoded_links_measure.restype = C.c_int
    L.hny_encoded_links_measure.argtypes = [el, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                            C.POINTER(C.c_uint64)]
    L.hny_lmdb_read_links.restype = C.c_int
    L.hny_lmdb_read_links.argtypes = [vp, C.c_uint16, C.POINTER(el)]
    L.hny_builder_export_items.restype = C.c_int
    L.hny_builder_export_items.argtypes = [vp, vp, vp]
    L.hny_builder_search_knn_f32.restype = C.c_int
    L.hny_builder_search_knn_f32.argtypes = [vp, C.c_uint64, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp, vp, vp]
    L.hny_builder_nns_f32.restype = C.c_int
    L.hny_builder_nns_f32.argtypes = [vp, C.POINTER(QueryOpts), C.c_uint64, vp, C.c_size_t, vp, vp, vp]
    L.hny_builder_exact_knn.restype = C.c_int
    L.hny_builder_exact_knn.argtypes = [vp, C.POINTER(QueryOpts), C.c_uint64, vp, C.c_size_t, vp, vp, vp, vp, vp]
    L.hny_builder_exact_knn_f32.restype = C.c_int
    L.hny_builder_exact_knn_f32.argtypes = [vp, C.POINTER(QueryOpts), C.c_uint64, vp, C.c_size_t, vp, vp, vp]
    L.hny_builder_nns_filtered.restype = C.c_int
    L.hny_builder_nns_filtered.argtypes = [vp, C.POINTER(QueryOpts), C.POINTER(QueryFilters), C.c_uint64, vp, C.c_size_t,
                                           vp, vp, vp, vp, vp]
    L.hny_builder_nns_filtered_f32.restype = C.c_int
    L.hny_builder_nns_filtered_f32.argtypes = [vp, C.POINTER(QueryOpts), C.POINTER(QueryFilters), C.c_uint64, vp,
                                               C.c_size_t, vp, vp, vp]
    L.hny_builder_exact_knn_filtered.restype = C.c_int
    L.hny_builder_exact_knn_filtered.argtypes = L.hny_builder_nns_filtered.argtypes
    L.hny_builder_exact_knn_filtered_f32.restype = C.c_int
    L.hny_builder_exact_knn_filtered_f32.argtypes = L.hny_builder_nns_filtered_f32.argtypes
    for name in ("hny_builder_nns_bitsets", "hny_builder_exact_knn_bitsets"):
        fn, f32 = getattr(L, name), getattr(L, name + "_f32")
        fn.restype = f32.restype = C.c_int
        fn.argtypes = [vp, C.POINTER(QueryOpts), C.POINTER(QueryBitsets)] + L.hny_builder_nns_filtered.argtypes[3:]
        f32.argtypes = [vp, C.POINTER(QueryOpts), C.POINTER(QueryBitsets)] + L.hny_builder_nns_filtered_f32.argtypes[3:]
    L.hny_builder_exact_range.restype = C.c_int
    L.hny_builder_exact_range.argtypes = [vp, C.POINTER(RangeOpts), C.c_uint64, vp, C.c_size_t, vp, vp,
                                          C.POINTER(C.POINTER(RangeResult))]
    L.hny_builder_exact_range_f32.restype = C.c_int
    L.hny_builder_exact_range_f32.argtypes = [vp, C.POINTER(RangeOpts), C.c_uint64, vp, C.c_size_t,
                                              C.POINTER(C.POINTER(RangeResult))]
    L.hny_builder_exact_range_count.restype = C.c_int
    L.hny_builder_exact_range_count.argtypes = [vp, C.POINTER(RangeOpts), C.c_uint64, vp, C.c_size_t, vp, vp, vp]
    L.hny_builder_exact_range_count_f32.restype = C.c_int
    L.hny_builder_exact_range_count_f32.argtypes = [vp, C.POINTER(RangeOpts), C.c_uint64, vp, C.c_size_t, vp]
    for kind, struct in (("filtered", QueryFilters), ("bitsets", QueryBitsets)):
        for count in ("", "_count"):
            plain = "hny_builder_exact_range" + count
            fn, f32 = getattr(L, f"{plain}_{kind}"), getattr(L, f"{plain}_{kind}_f32")
            fn.restype = f32.restype = C.c_int
            fn.argtypes = getattr(L, plain).argtypes[:2] + [C.POINTER(struct)] + getattr(L, plain).argtypes[2:]
            f32.argtypes = (getattr(L, plain + "_f32").argtypes[:2] + [C.POINTER(struct)] +
                            getattr(L, plain + "_f32").argtypes[2:])
    L.hny_range_result_free.restype = None
    L.hny_range_result_free.argtypes = [C.POINTER(RangeResult)]
    L.hny_builder_exact_rows_read.restype = C.c_uint64
    L.hny_builder_exact_rows_read.argtypes = [vp]
    L.hny_builder_create_update.restype = C.c_int
    L.hny_builder_create_update.argtypes = [vp, C.POINTER(Update), C.POINTER(vp)]
    L.hny_builder_update.restype = C.c_int
    L.hny_builder_update.argtypes = [C.POINTER(vp), C.POINTER(Update), C.POINTER(C.POINTER(GraphStruct)),
                                     C.POINTER(C.POINTER(GraphDeltaStruct))]
    L.hny_builder_finish_delta.restype = C.c_int
    L.hny_builder_finish_delta.argtypes = [vp, C.POINTER(C.POINTER(GraphDeltaStruct))]
    L.hny_graph_delta_free.restype = None
    L.hny_graph_delta_free.argtypes = [C.POINTER(GraphDeltaStruct)]
    L.hny_distance_keeps_links.restype = C.c_int
    L.hny_distance_keeps_links.argtypes = [C.c_int32, C.c_int32]
    L.hny_builder_create_changed_distance.restype = C.c_int
    L.hny_builder_create_changed_distance.argtypes = [vp, C.POINTER(ChangeDistance), C.POINTER(vp)]
    L.hny_builder_recode_items.restype = C.c_int
    L.hny_builder_recode_items.argtypes = [vp, C.c_int32, vp, vp]
    L.hny_builder_finish_encoded.restype = C.c_int
    L.hny_builder_finish_encoded.argtypes = [vp, C.POINTER(C.POINTER(EncodedLinksStruct))]
    L.hny_encoded_links_free.restype = None
    L.hny_encoded_links_free.argtypes = [C.POINTER(EncodedLinksStruct)]
    L.hny_encode_kv_encoded.restype = C.c_int
    L.hny_encode_kv_encoded.argtypes = [C.POINTER(EncodedLinksStruct), C.POINTER(BuildOpts), C.POINTER(Items),
                                        C.c_uint16, C.c_int, KV_SINK, vp]
    L.hny_builder_finish_delta_encoded.restype = C.c_int
    L.hny_builder_finish_delta_encoded.argtypes = [vp, C.POINTER(C.POINTER(EncodedDeltaStruct))]
    L.hny_encoded_delta_free.restype = None
    L.hny_encoded_delta_free.argtypes = [C.POINTER(EncodedDeltaStruct)]
    L.hny_abi_sizes.restype = C.c_uint32
    L.hny_abi_sizes.argtypes = [C.POINTER(C.c_uint32), C.c_uint32]
    _check_abi(L)
    _lib = L
    return L


# the order of hny_abi_sizes (HNY_ABI_* in include/hannoy_amd.h)
ABI_STRUCTS = None


def _check_abi(L):
    """sizeof of every struct declared here against the library's own (hny_abi_sizes): a field added
    to the header and not to this binding fails the import instead of corrupting a call"""
    global ABI_STRUCTS
    ABI_STRUCTS = [("hny_build_opts", BuildOpts), ("hny_items", Items), ("hny_graph", GraphStruct),
                   ("hny_prev_graph", PrevGraph), ("hny_batch", Batch), ("hny_query_opts", QueryOpts),
                   ("hny_lmdb_stat", LmdbStat)]
    out = (C.c_uint32 * len(ABI_STRUCTS))()
    n = L.hny_abi_sizes(out, len(ABI_STRUCTS))
    if n != len(ABI_STRUCTS):
        raise ImportError(f"hannoy_amd ABI mismatch: the library knows {n} public structs, this binding {len(ABI_STRUCTS)}")
    for (name, cls), size in zip(ABI_STRUCTS, out):
        if C.sizeof(cls) != size:
            raise ImportError(f"hannoy_amd ABI mismatch: sizeof({name}) is {size} in the library, "
                              f"{C.sizeof(cls)} in hannoy_amd/_capi.py")


def abi_sizes():
    """{struct name: sizeof in the loaded library}"""
    L = load_library()
    out = (C.c_uint32 * len(ABI_STRUCTS))()
    L.hny_abi_sizes(out, len(ABI_STRUCTS))
    return {name: int(v) for (name, _), v in zip(ABI_STRUCTS, out)}


def _check(rc):
    if rc != OK:
        msg = load_library().hny_last_error().decode("utf-8", "replace")
        raise (BuildCancelled if rc == ERR_CANCELLED else HannoyError)(rc, msg)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def u32_ids(a):
    """item ids (hny_items.ids, candidates, query_items, to_insert, to_delete ...) as a contiguous uint32 array.  An
    ItemId is a full u32: 0 .. 2^32 - 1 are all legal, 2^32 - 1 included.  Anything else is refused here — a negative
    value, one >= 2^32, a fraction, NaN — because a numpy cast to uint32 would wrap it into some other item's id"""
    if isinstance(a, np.ndarray) and a.dtype == np.uint32:
        return np.ascontiguousarray(a)
    arr = np.asarray(a if isinstance(a, np.ndarray) else list(a))
    if arr.size == 0:
        return np.zeros(arr.shape, np.uint32)
    if arr.dtype.kind == "f":
        if not np.isfinite(arr).all() or (arr != np.floor(arr)).any():
            raise ValueError("item ids must be integers")
    elif arr.dtype.kind not in "iu":
        raise TypeError(f"item ids must be integers, not {arr.dtype}")
    if arr.min() < 0 or arr.max() > 0xFFFFFFFF:
        bad = arr[(arr < 0) | (arr > 0xFFFFFFFF)].ravel()[0]
        raise OverflowError(f"item id {bad} is outside 0 .. 2^32 - 1")
    return np.ascontiguousarray(arr, np.uint32)


def set_graph_cache(max_bytes):
    """hny_set_graph_cache: opt-in recycling of released export arrays (0 = off, the default)"""
    L = load_library()
    L.hny_set_graph_cache.restype = None
    L.hny_set_graph_cache.argtypes = [C.c_size_t]
    L.hny_set_graph_cache(int(max_bytes))


def default_batch_max(n_items):
    """what batch_max = 0 selects for an index of n_items (hny_default_batch_max)"""
    L = load_library()
    L.hny_default_batch_max.restype = C.c_uint32
    L.hny_default_batch_max.argtypes = [C.c_uint64]
    return int(L.hny_default_batch_max(int(n_items)))


def selftest_lane_ops(device=-1):
    """hny_selftest_lane_ops: per-lane mismatch masks (all zero = the cross-lane primitives agree with
    __shfl_xor); raises HannoyError if they do not"""
    L = load_library()
    L.hny_selftest_lane_ops.restype = C.c_int
    L.hny_selftest_lane_ops.argtypes = [C.c_int32, C.POINTER(C.c_uint32)]
    out = (C.c_uint32 * 64)()
    _check(L.hny_selftest_lane_ops(int(device), out))
    return list(out)


def draw_levels(seed, M, n):
    out = np.zeros(n, np.uint8)
    _check(load_library().hny_draw_levels(seed, M, n, _p(out)))
    return out


class StdRng:
    """rand 0.8.5 `StdRng` as far as a build uses it: the 32-byte seed plus how many levels were
    drawn so far (get_random_level costs one u32 each, hnsw.rs:113-119), so that one generator can
    be carried across builds like `writer.builder(&mut rng)` does."""

    def __init__(self, seed32, drawn=0):
        self.seed = bytes(seed32)
        assert len(self.seed) == 32
        self.drawn = drawn

    @classmethod
    def from_seed(cls, seed32):
        """SeedableRng::from_seed (the reference's test rng: [42; 32], src/tests/mod.rs:145-147)"""
        return cls(seed32)

    @classmethod
    def seed_from_u64(cls, state):
        """SeedableRng::seed_from_u64 (rand_core 0.6): PCG32 expansion (python.rs:261 uses 42)"""
        out = b""
        for _ in range(8):
            state = (state * 6364136223846793005 + 11634580027462260723) & 0xFFFFFFFFFFFFFFFF
            xs = (((state >> 18) ^ state) >> 27) & 0xFFFFFFFF
            rot = state >> 59
            out += (((xs >> rot) | (xs << ((32 - rot) & 31))) & 0xFFFFFFFF).to_bytes(4, "little")
        return cls(out)

    def draw_levels(self, M, n):
        out = np.zeros(n, np.uint8)
        seed = (C.c_uint8 * 32).from_buffer_copy(self.seed)
        _check(load_library().hny_draw_levels_from_seed(seed, self.drawn, M, n, _p(out)))
        self.drawn += n
        return out


def distance_keeps_links(old_metric, new_metric):
    """hny_distance_keeps_links: Writer::prepare_changing_distance keeps links and Metadata for this pair"""
    return bool(load_library().hny_distance_keeps_links(int(old_metric), int(new_metric)))


def vector_bytes(metric, dim):
    return load_library().hny_vector_bytes(metric, dim)


def header_bytes(metric):
    return load_library().hny_header_bytes(metric)


def encode_vectors(metric, vecs, gpu=False, device=-1):
    """UnalignedVectorCodec::from_slice + Distance::new_header for a [n, dim] f32 matrix
    (gpu=True: hny_encode_vectors_gpu, byte-identical)."""
    vecs = np.ascontiguousarray(vecs, dtype=np.float32)
    n, dim = vecs.shape
    codes = np.zeros((n, vector_bytes(metric, dim)), np.uint8)
    headers = np.zeros((n, header_bytes(metric)), np.uint8)
    if gpu:
        _check(load_library().hny_encode_vectors_gpu(metric, dim, n, _p(vecs), _p(codes), _p(headers),
                                                     device))
    else:
        _check(load_library().hny_encode_vectors(metric, dim, n, _p(vecs), _p(codes), _p(headers)))
    return codes, headers


class ItemSet:
    """What FrozenReader hands to the builder (/root/reference/src/parallel.rs:33-45)."""

    def __init__(self, metric, dim, ids, codes, headers, levels=None):
        self.metric, self.dim = int(metric), int(dim)
        self.ids = u32_ids(ids)
        self.codes = np.ascontiguousarray(codes, dtype=np.uint8)
        self.headers = np.ascontiguousarray(headers, dtype=np.uint8)
        self.levels = None if levels is None else np.ascontiguousarray(levels, dtype=np.uint8)
        self.n = len(self.ids)

    f32 = False  # codec bytes + headers (F32ItemSet: f32 rows, encoded on the device)

    def encoded(self):
        return self

    @classmethod
    def from_f32(cls, metric, vecs, ids=None, levels=None, device=False):
        """device=True: keep the f32 matrix and let the device encode it while it is uploaded (F32ItemSet)"""
        if device:
            return F32ItemSet(metric, vecs, ids, levels)
        vecs = np.ascontiguousarray(vecs, dtype=np.float32)
        codes, headers = encode_vectors(metric, vecs)
        ids = np.arange(len(vecs), dtype=np.uint32) if ids is None else ids
        return cls(metric, vecs.shape[1], ids, codes, headers, levels)

    def struct(self):
        return Items(self.n, _p(self.ids).value, _p(self.codes).value,
                     self.codes.shape[1] if self.codes.ndim == 2 else 0, _p(self.headers).value,
                     self.headers.shape[1] if self.headers.ndim == 2 else 0,
                     None if self.levels is None else _p(self.levels).value)


def _f32_rows(a):
    """a [n, dim] f32 matrix whose rows are contiguous (the row stride may be larger than dim * 4)"""
    a = np.asarray(a, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError("expected a [n, dim] matrix")
    if a.shape[1] > 1 and a.strides[1] != 4 or a.shape[0] > 1 and a.strides[0] < a.shape[1] * 4:
        a = np.ascontiguousarray(a)
    return a


def _query_opts(k, ef_search=0, linear_below=0, linear_below_ratio=0.0, candidates=None, cancel=None):
    """hny_query_opts of one search call.  cancel: a closure without arguments, true = stop.
    Returns (struct, what it points into, the int32 did_cancel points at: stays 0 without a closure)"""
    qo = QueryOpts()
    qo.k, qo.ef_search = k, ef_search
    qo.linear_below, qo.linear_below_ratio = linear_below, linear_below_ratio
    flag = C.c_int32(0)
    keep = [flag]
    if cancel is not None:
        fn = CANCEL_FN(lambda _ctx: 1 if cancel() else 0)
        qo.cancel, qo.did_cancel = fn, C.pointer(flag)
        keep.append(fn)
    if candidates is not None:
        cand = u32_ids(candidates)
        qo.has_candidates, qo.candidates, qo.n_candidates = 1, cand.ctypes.data, len(cand)
        keep.append(cand)
    return qo, keep, flag


def _query_source(query_items=None, qf32=None, qcodes=None, qheaders=None):
    """The queries of one search call, by item, as f32 rows (see _f32_rows) or as codes + headers.
    Returns ((nq, qvectors, qstride, qheaders, query_items) as the entry points take them, the arrays behind them)"""
    if query_items is not None:
        items = u32_ids(query_items)
        return (len(items), None, 0, None, _p(items)), (items,)
    if qf32 is not None:
        nq = qf32.shape[0]  # (numpy gives a one-row view whatever stride it likes)
        return (nq, _p(qf32), qf32.strides[0] if nq > 1 else qf32.shape[1] * 4, None, None), (qf32,)
    qcodes = np.ascontiguousarray(qcodes, np.uint8)
    qheaders = np.ascontiguousarray(qheaders, np.uint8)
    return (qcodes.shape[0], _p(qcodes), qcodes.shape[1], _p(qheaders), None), (qcodes, qheaders)


def _range_opts(radius, nq, candidates=None, cancel=None, max_total=0):
    """hny_range_opts of one range call.  radius: a scalar or one value per query.
    Returns (struct, what it points into, the int32 did_cancel points at)"""
    ro = RangeOpts()
    r = np.asarray(radius, np.float32)
    r = np.full(nq, r, np.float32) if r.ndim == 0 else np.ascontiguousarray(r.ravel())
    if len(r) != nq:
        raise ValueError(f"radius has {len(r)} entries for {nq} queries")
    flag = C.c_int32(0)
    keep = [flag, r]
    ro.radius, ro.max_total = r.ctypes.data, int(max_total)
    if cancel is not None:
        fn = CANCEL_FN(lambda _ctx: 1 if cancel() else 0)
        ro.cancel, ro.did_cancel = fn, C.pointer(flag)
        keep.append(fn)
    if candidates is not None:
        cand = u32_ids(candidates)
        ro.has_candidates, ro.candidates, ro.n_candidates = 1, cand.ctypes.data, len(cand)
        keep.append(cand)
    return ro, keep, flag


def _result_arrays(nq, k):
    """(ids, dists, counts) for nq queries of k hits"""
    return np.zeros((nq, k), np.uint32), np.zeros((nq, k), np.float32), np.zeros(nq, np.uint32)


class F32ItemSet:
    """The items as the f32 vectors Writer::add_item takes (src/writer.rs:462-480): build(),
    build_incremental() and Builder hand them to the hny_*_f32 entry points, which encode them on the device
    while they are uploaded.  Codes and headers exist on the host only once something asks for them
    (Graph.encode_kv(with_items=True)): encoded() runs hny_encode_vectors then."""
    f32 = True

    def __init__(self, metric, vecs, ids=None, levels=None):
        self.vecs = _f32_rows(vecs)
        self.metric, self.dim = int(metric), int(self.vecs.shape[1])
        self.n = len(self.vecs)
        self.ids = u32_ids(np.arange(self.n) if ids is None else ids)
        self.levels = None if levels is None else np.ascontiguousarray(levels, dtype=np.uint8)
        self._encoded = None

    def struct(self):
        stride = self.vecs.strides[0] if self.n > 1 else self.dim * 4
        return Items(self.n, _p(self.ids).value, _p(self.vecs).value, stride, None, 0,
                     None if self.levels is None else _p(self.levels).value)

    def encoded(self):
        if self._encoded is None:
            codes, headers = encode_vectors(self.metric, self.vecs)
            self._encoded = ItemSet(self.metric, self.dim, self.ids, codes, headers, self.levels)
        return self._encoded

    @property
    def codes(self):
        return self.encoded().codes

    @property
    def headers(self):
        return self.encoded().headers


class _IdsOnly:
    """the items of a successor Builder as far as the host knows them: ids (rows and codes live in HBM;
    Builder.export_items reads them back)"""
    f32 = False

    def __init__(self, metric, dim, ids):
        self.metric, self.dim, self.ids, self.n, self.levels = int(metric), int(dim), ids, len(ids), None

    def encoded(self):
        raise HannoyError(ERR_UNSUPPORTED, "the items of an updated builder live on the device: Builder.export_items()")


def make_opts(metric, dim, M=16, M0=32, ef_construction=100, alpha=1.0, seed=42, batch_frac=0.0,
              batch_max=0, device=-1, cancel=None, progress=None, x86_order=False, n_gpus=0, devices=None,
              schedule=0):
    o = BuildOpts()
    o.schedule = int(schedule)
    o.metric, o.dim, o.M, o.M0 = metric, dim, M, M0
    o.ef_construction, o.alpha, o.seed = ef_construction, alpha, seed
    o.batch_frac, o.batch_max, o.device = batch_frac, batch_max, device
    o.x86_order = int(bool(x86_order))
    keep = []
    o.n_gpus = int(n_gpus)
    if devices is not None:  # one replica per listed GPU, RCCL all-gathers between them (hny_multi.cpp)
        arr = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        o.devices = C.cast(arr, C.POINTER(C.c_int32))
        o.n_gpus = int(n_gpus) or len(devices)
        keep.append(arr)
    if cancel is not None:
        fn = CANCEL_FN(lambda _ctx: 1 if cancel() else 0)
        o.cancel = fn
        keep.append(fn)
    if progress is not None:
        fn = PROGRESS_FN(lambda _ctx, done, total: progress(done, total))
        o.progress = fn
        keep.append(fn)
    o._keep = keep
    return o


class Graph:
    """Host copy of hny_graph (records the write loop of hnsw.rs:195-213 consumes)."""

    _ARRAYS = ("rec_item", "rec_layer", "offsets", "nbrs", "entry_points")

    def __init__(self, gp, opts=None, items=None):
        g = gp.contents
        self.max_level = g.max_level
        for f in ("n_links_added", "n_distance_evals", "n_evals_walk", "n_evals_prune",
                  "n_evals_apply", "n_batches", "t_upload_s", "t_build_s", "t_export_s",
                  "n_tie_pool_overflow", "t_walk_kernels_s", "t_prune_kernels_s",
                  "t_sort_kernels_s", "t_apply_kernels_s", "n_walk_launches"):
            setattr(self, f, getattr(g, f))
        self._gp, self._opts, self._items = gp, opts, items

    def __getattr__(self, name):
        # numpy copies of the library-owned arrays, made on first use (a 1M x 768 index has 125 MB
        # of them; the product is the hny_graph itself, these are for tests and scripts)
        if name not in Graph._ARRAYS or self.__dict__.get("_gp") is None:
            raise AttributeError(name)
        g = self._gp.contents
        nrec = g.n_records
        if name == "rec_item":
            v = np.ctypeslib.as_array(g.rec_item, (max(nrec, 1),))[:nrec].copy()
        elif name == "rec_layer":
            v = np.ctypeslib.as_array(g.rec_layer, (max(nrec, 1),))[:nrec].copy()
        elif name == "offsets":
            v = np.ctypeslib.as_array(g.rec_offset, (nrec + 1,)).copy()
        elif name == "nbrs":
            nl = int(self.offsets[-1])
            v = np.ctypeslib.as_array(g.neighbours, (max(nl, 1),))[:nl].copy()
        else:
            ne = g.n_entry_points
            v = np.ctypeslib.as_array(g.entry_points, (max(ne, 1),))[:ne].copy()
        self.__dict__[name] = v
        return v

    def __del__(self):
        try:
            if getattr(self, "_gp", None) is not None:
                load_library().hny_graph_free(self._gp)
                self._gp = None
        except Exception:  # interpreter shutdown
            pass

    def as_dict(self):
        return {(int(self.rec_item[r]), int(self.rec_layer[r])):
                self.nbrs[int(self.offsets[r]):int(self.offsets[r + 1])].tolist()
                for r in range(len(self.rec_item))}

    def encode_kv(self, index=0, with_items=False):
        """Byte-exact (key, value) records in LMDB key order (hny_encode_kv)."""
        out = []

        def sink(_ctx, k, kl, v, vl):
            out.append((bytes(k[:kl]), bytes(v[:vl])))
            return 0
        cb = KV_SINK(sink)
        it, _keep = _kv_items(self._items, with_items)
        _check(load_library().hny_encode_kv(self._gp, C.byref(self._opts), C.byref(it), index,
                                            int(with_items), cb, None))
        return out

    def write_lmdb(self, path, index=0, with_items=True, name=None, page_size=0, map_size=0):
        """The records of a fresh index straight into an LMDB `data.mdb`: hny_encode_kv with
        hny_lmdb_writer_put as its sink (no Python in the record loop)."""
        L = load_library()
        w = LmdbWriter(path, name, page_size, map_size)
        it = self._items.encoded().struct()
        sink = C.cast(L.hny_lmdb_writer_put, KV_SINK)
        try:
            _check(L.hny_encode_kv(self._gp, C.byref(self._opts), C.byref(it), index, int(with_items), sink, w.handle))
        except Exception:
            w.abort()
            raise
        w.finish()


def _kv_items(items, with_items):
    """(hny_items for hny_encode_kv[_encoded], what keeps its arrays alive)"""
    if isinstance(items, _IdsOnly) and not with_items:  # a successor's items live on the device
        ids = np.ascontiguousarray(items.ids, np.uint32)
        return Items(len(ids), _p(ids).value, None, 0, None, 0, None), ids
    enc = items.encoded()  # an F32ItemSet encodes on the host here, once
    return enc.struct(), enc


class EncodedLinks:
    """hny_encoded_links (Builder.finish_encoded): the Links records of a finished builder, their values serialised
    on the device.  `rec_item`, `rec_layer`, `val_offset`, `values` are numpy views of the library's arrays (valid
    while this object lives, which frees them); the value of record r is values[val_offset[r]:val_offset[r + 1]]."""

    _VIEWS = ("rec_item", "rec_layer", "val_offset", "values")

    def __init__(self, ep, opts=None, items=None, owner=None):
        """owner: `ep` points into a struct that another object frees (EncodedDelta): this view frees nothing"""
        e = ep.contents
        self._owner = owner
        for f in ("max_level", "n_links_added", "n_evals_walk", "n_batches", "t_export_s", "t_device_s",
                  "t_download_s", "bytes_downloaded"):
            setattr(self, f, getattr(e, f))
        ne = e.n_entry_points
        self.entry_points = np.ctypeslib.as_array(e.entry_points, (max(ne, 1),))[:ne].copy()
        self._ep, self._opts, self._items = ep, opts, items

    @classmethod
    def from_records(cls, rec_item, rec_layer, values_list, entry_points, max_level):
        """A struct filled in here, for Builder(stored=...), build_incremental(stored=...), encoded_links_measure and
        encode_kv: the Links records (item, layer) in key order with their values as they lie on disk (bytes-like
        each: tag 0x01 | roaring bytes).  Nothing is decoded or checked here."""
        lens = np.fromiter((len(v) for v in values_list), np.uint64, len(values_list))
        keep = [np.ascontiguousarray(rec_item, np.uint32), np.ascontiguousarray(rec_layer, np.uint8),
                np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)]),
                np.frombuffer(b"".join(values_list) or b"\0", np.uint8),
                np.ascontiguousarray(entry_points if len(entry_points) else np.zeros(1), np.uint32)]
        if not len(keep[0]) == len(keep[1]) == len(lens):
            raise ValueError("rec_item, rec_layer and values_list differ in length")
        st = EncodedLinksStruct()
        st.n_records = len(lens)
        for f, a, t in zip(("rec_item", "rec_layer", "val_offset", "values", "entry_points"), keep,
                           (C.c_uint32, C.c_uint8, C.c_uint64, C.c_uint8, C.c_uint32)):
            if not len(a):  # (no NULL arrays: the views of an empty struct are empty arrays)
                a = np.zeros(1, a.dtype)
                keep.append(a)
            setattr(st, f, C.cast(a.ctypes.data, C.POINTER(t)))
        st.n_entry_points, st.max_level = len(entry_points), int(max_level)
        return cls(C.pointer(st), owner=keep)

    @property
    def ptr(self):
        """POINTER(hny_encoded_links) for the calls that take the struct as input"""
        return self._ep

    def __getattr__(self, name):
        if name not in EncodedLinks._VIEWS or self.__dict__.get("_ep") is None:
            raise AttributeError(name)
        e = self._ep.contents
        nrec = e.n_records
        if name == "val_offset":
            v = np.ctypeslib.as_array(e.val_offset, (nrec + 1,))
        elif name == "values":
            nb = int(self.val_offset[-1])
            v = np.ctypeslib.as_array(e.values, (max(nb, 1),))[:nb]
        else:
            v = np.ctypeslib.as_array(getattr(e, name), (max(nrec, 1),))[:nrec]
        self.__dict__[name] = v
        return v

    def __del__(self):
        try:
            if getattr(self, "_ep", None) is not None:
                for name in EncodedLinks._VIEWS:  # (the views die with the arrays)
                    self.__dict__.pop(name, None)
                if getattr(self, "_owner", None) is None:
                    load_library().hny_encoded_links_free(self._ep)
                self._ep = self._owner = None
        except Exception:  # interpreter shutdown
            pass

    def encode_kv(self, index=0, with_items=False):
        """Byte-exact (key, value) records in LMDB key order (hny_encode_kv_encoded): what Graph.encode_kv gives for
        the Graph of the same builder."""
        out = []

        def sink(_ctx, k, kl, v, vl):
            out.append((bytes(k[:kl]), bytes(v[:vl])))
            return 0
        cb = KV_SINK(sink)
        it, _keep = _kv_items(self._items, with_items)
        _check(load_library().hny_encode_kv_encoded(self._ep, C.byref(self._opts), C.byref(it), index,
                                                    int(with_items), cb, None))
        return out

    def write_lmdb(self, path, index=0, with_items=True, name=None, page_size=0, map_size=0):
        """The records straight into an LMDB `data.mdb`: hny_encode_kv_encoded with hny_lmdb_writer_put as its sink
        (the Links values go from the downloaded buffer into the pages, no Python in the record loop)."""
        L = load_library()
        w = LmdbWriter(path, name, page_size, map_size)
        it, _keep = _kv_items(self._items, with_items)
        sink = C.cast(L.hny_lmdb_writer_put, KV_SINK)
        try:
            _check(L.hny_encode_kv_encoded(self._ep, C.byref(self._opts), C.byref(it), index, int(with_items), sink,
                                           w.handle))
        except Exception:
            w.abort()
            raise
        w.finish()


class GraphDelta:
    """Host view of hny_graph_delta: what the write loop has to put (`rec_item` / `rec_layer` / `offsets` / `nbrs`:
    records that are new or whose list changed) and to delete (`removed_item` / `removed_layer`) after an update.
    The arrays are numpy views of library-owned memory, freed with the object."""

    def __init__(self, dp, opts=None):
        d = dp.contents
        self._dp, self._opts = dp, opts
        nr, nm, ne = d.n_records, d.n_removed, d.n_entry_points
        self.max_level, self.n_records_total, self.t_export_s = d.max_level, d.n_records_total, d.t_export_s
        self.rec_item = np.ctypeslib.as_array(d.rec_item, (max(nr, 1),))[:nr]
        self.rec_layer = np.ctypeslib.as_array(d.rec_layer, (max(nr, 1),))[:nr]
        self.offsets = np.ctypeslib.as_array(d.rec_offset, (nr + 1,))
        nl = int(self.offsets[-1])
        self.nbrs = np.ctypeslib.as_array(d.neighbours, (max(nl, 1),))[:nl]
        self.removed_item = np.ctypeslib.as_array(d.removed_item, (max(nm, 1),))[:nm]
        self.removed_layer = np.ctypeslib.as_array(d.removed_layer, (max(nm, 1),))[:nm]
        self.entry_points = np.ctypeslib.as_array(d.entry_points, (max(ne, 1),))[:ne]

    def __del__(self):
        try:
            if getattr(self, "_dp", None) is not None:
                for f in ("rec_item", "rec_layer", "offsets", "nbrs", "removed_item", "removed_layer", "entry_points"):
                    self.__dict__.pop(f, None)  # the views die with the memory
                load_library().hny_graph_delta_free(self._dp)
                self._dp = None
        except Exception:  # interpreter shutdown
            pass

    def as_dict(self):
        return {(int(self.rec_item[r]), int(self.rec_layer[r])):
                self.nbrs[int(self.offsets[r]):int(self.offsets[r + 1])].tolist()
                for r in range(len(self.rec_item))}

    def removed_keys(self):
        return [(int(i), int(l)) for i, l in zip(self.removed_item, self.removed_layer)]

    def encode_kv(self, item_ids, index=0):
        """Metadata, Version and the Links records of the delta as byte-exact (key, value) pairs (hny_encode_kv on the
        delta's records); `item_ids`: every item of the index after the update, ascending (Metadata.items)"""
        d = self._dp.contents
        g = GraphStruct()
        g.n_records, g.rec_item, g.rec_layer, g.rec_offset = d.n_records, d.rec_item, d.rec_layer, d.rec_offset
        g.neighbours, g.entry_points, g.n_entry_points, g.max_level = d.neighbours, d.entry_points, d.n_entry_points, d.max_level
        ids = u32_ids(item_ids)
        it = Items(len(ids), _p(ids).value, None, 0, None, 0, None)
        out = []

        def sink(_ctx, k, kl, v, vl):
            out.append((bytes(k[:kl]), bytes(v[:vl])))
            return 0
        cb = KV_SINK(sink)
        _check(load_library().hny_encode_kv(C.byref(g), C.byref(self._opts), C.byref(it), index, 0, cb, None))
        return out


class EncodedDelta:
    """hny_encoded_delta (Builder.finish_delta_encoded): GraphDelta's records with their values serialised on the
    device.  `links` is an EncodedLinks view of the new / changed records (it frees nothing); its `rec_item`,
    `rec_layer`, `val_offset`, `values`, `entry_points`, `max_level`, counters and timings are attributes of this
    object too.  `removed_item` / `removed_layer` are the keys to delete.  All valid while this object lives."""

    _LINKS = EncodedLinks._VIEWS + ("entry_points", "max_level", "n_links_added", "n_evals_walk", "n_batches",
                                    "t_export_s", "t_device_s", "t_download_s", "bytes_downloaded")

    def __init__(self, dp, opts=None):
        self._dp = dp  # first: whatever fails below, __del__ frees the struct
        d = dp.contents
        nm = d.n_removed
        self.n_records_total = d.n_records_total
        self.removed_item = np.ctypeslib.as_array(d.removed_item, (max(nm, 1),))[:nm]
        self.removed_layer = np.ctypeslib.as_array(d.removed_layer, (max(nm, 1),))[:nm]
        self.links = EncodedLinks(C.pointer(d.links), opts, None, owner=True)

    def __getattr__(self, name):
        if name not in EncodedDelta._LINKS or self.__dict__.get("links") is None:
            raise AttributeError(name)
        return getattr(self.links, name)

    def __del__(self):
        try:
            if getattr(self, "_dp", None) is not None:
                for name in ("removed_item", "removed_layer"):  # (the views die with the arrays)
                    self.__dict__.pop(name, None)
                links = self.__dict__.pop("links", None)
                if links is not None:
                    links.__del__()  # drops its views and its pointer into the struct
                load_library().hny_encoded_delta_free(self._dp)
                self._dp = None
        except Exception:  # interpreter shutdown
            pass

    def removed_keys(self):
        return [(int(i), int(l)) for i, l in zip(self.removed_item, self.removed_layer)]

    def encode_kv(self, item_ids, index=0):
        """What GraphDelta.encode_kv gives for the delta of the same builder (hny_encode_kv_encoded on `links`);
        `item_ids`: every item of the index after the update, ascending (Metadata.items)"""
        if np.ndim(item_ids) != 1:
            raise HannoyError(ERR_INVALID_ARG, "EncodedDelta.encode_kv(item_ids, index): item_ids is a sequence of ids")
        ids = u32_ids(item_ids)
        it = Items(len(ids), _p(ids).value, None, 0, None, 0, None)
        out = []

        def sink(_ctx, k, kl, v, vl):
            out.append((bytes(k[:kl]), bytes(v[:vl])))
            return 0
        cb = KV_SINK(sink)
        _check(load_library().hny_encode_kv_encoded(self.links._ep, C.byref(self.links._opts), C.byref(it), index, 0,
                                                    cb, None))
        return out


class LmdbWriter:
    """hny_lmdb_writer_*: bulk loader of an LMDB `data.mdb` (keys strictly ascending)."""

    def __init__(self, path, name=None, page_size=0, map_size=0):
        self._w = C.c_void_p()
        _check(load_library().hny_lmdb_writer_open(os.fsencode(path), page_size, map_size,
                                                   None if name is None else name.encode(), C.byref(self._w)))

    @property
    def handle(self):
        return self._w

    def put(self, k, v):
        _check(load_library().hny_lmdb_writer_put(self._w, k, len(k), v, len(v)))

    def finish(self):
        w, self._w = self._w, None
        _check(load_library().hny_lmdb_writer_finish(w))

    def abort(self):
        if self._w is not None:
            load_library().hny_lmdb_writer_abort(self._w)
            self._w = None

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.finish()
        else:
            self.abort()
        return False


class LmdbEnv:
    """hny_lmdb_open / get / scan: read side of a `data.mdb` (RoTxn + Database::get / iter)."""

    def __init__(self, path, name=None):
        self._e = C.c_void_p()
        _check(load_library().hny_lmdb_open(os.fsencode(path), None if name is None else name.encode(),
                                            C.byref(self._e)))

    def stat(self):
        st = LmdbStat()
        _check(load_library().hny_lmdb_stat_get(self._e, C.byref(st)))
        return {f: getattr(st, f) for f, _ in LmdbStat._fields_}

    def get(self, k):
        val, n = C.POINTER(C.c_uint8)(), C.c_size_t()
        rc = load_library().hny_lmdb_get(self._e, k, len(k), C.byref(val), C.byref(n))
        if rc < 0:
            _check(rc)
        return C.string_at(val, n.value) if rc == 1 else None

    def items(self, lo=None, hi=None):
        """(key, value) pairs with lo <= key <= hi in key order; a full scan also verifies the
        page counts of the MDB_db record"""
        out = []

        def sink(_ctx, k, kl, v, vl):
            out.append((C.string_at(k, kl), C.string_at(v, vl)))
            return 0
        cb = KV_SINK(sink)
        _check(load_library().hny_lmdb_scan(self._e, lo, len(lo) if lo else 0, hi, len(hi) if hi else 0, cb, None))
        return out

    def verify(self):
        _check(load_library().hny_lmdb_scan(self._e, None, 0, None, 0, KV_SINK(), None))

    def read_links(self, index=0):
        """hny_lmdb_read_links: every Links record of `index` with its value as it lies in the file, plus the entry
        points and max_level of the Metadata record, as an EncodedLinks (no Python in the record loop)"""
        ep = C.POINTER(EncodedLinksStruct)()
        _check(load_library().hny_lmdb_read_links(self._e, index, C.byref(ep)))
        return EncodedLinks(ep)

    def close(self):
        if self._e is not None:
            load_library().hny_lmdb_close(self._e)
            self._e = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False


def build(items, **kw):
    """hny_build: the drop-in for HnswBuilder::build (/root/reference/src/hnsw.rs:122-216)."""
    o = make_opts(items.metric, items.dim, **kw)
    it = items.struct()
    gp = C.POINTER(GraphStruct)()
    L = load_library()
    _check((L.hny_build_f32 if items.f32 else L.hny_build)(C.byref(o), C.byref(it), C.byref(gp)))
    return Graph(gp, o, items)


def _prev_struct(prev):
    keep = [np.ascontiguousarray(prev.rec_item, np.uint32), np.ascontiguousarray(prev.rec_layer, np.uint8),
            np.ascontiguousarray(prev.offsets, np.uint64),
            np.ascontiguousarray(prev.nbrs if len(prev.nbrs) else np.zeros(1), np.uint32),
            np.ascontiguousarray(prev.entry_points, np.uint32)]
    pg = PrevGraph(len(keep[0]), _p(keep[0]).value, _p(keep[1]).value, _p(keep[2]).value,
                   _p(keep[3]).value, _p(keep[4]).value, len(keep[4]), int(prev.max_level))
    return pg, keep


def encoded_links_measure(stored, device=-1):
    """hny_encoded_links_measure: (longest layer-0 list, longest upper list, links) of an EncodedLinks, from the
    container headers alone, on the device"""
    m0, mu, nl = C.c_uint32(), C.c_uint32(), C.c_uint64()
    _check(load_library().hny_encoded_links_measure(stored.ptr, device, C.byref(m0), C.byref(mu), C.byref(nl)))
    return m0.value, mu.value, nl.value


def build_incremental(items, prev=None, to_insert=(), to_delete=(), stored=None, **kw):
    """hny_build_incremental: `items` = every item present after the update (levels, if any: one per
    to_insert id); `prev` = graph of the previous build (anything with rec_item/rec_layer/offsets/
    nbrs/entry_points/max_level), or `stored` = its Links records undecoded (an EncodedLinks:
    hny_build_incremental_encoded)."""
    o = make_opts(items.metric, items.dim, **kw)
    it = items.struct()
    ins = u32_ids(to_insert)
    dl = u32_ids(to_delete)
    if (prev is None) == (stored is None):
        raise ValueError("build_incremental takes either prev or stored")
    if stored is not None:
        if items.f32:
            raise HannoyError(ERR_UNSUPPORTED, "build_incremental(stored=...) takes codec bytes")
        gp = C.POINTER(GraphStruct)()
        _check(load_library().hny_build_incremental_encoded(C.byref(o), C.byref(it), _p(ins), len(ins), _p(dl), len(dl),
                                                            stored.ptr, C.byref(gp)))
        return Graph(gp, o, items)
    keep = [np.ascontiguousarray(prev.rec_item, np.uint32), np.ascontiguousarray(prev.rec_layer, np.uint8),
            np.ascontiguousarray(prev.offsets, np.uint64),
            np.ascontiguousarray(prev.nbrs if len(prev.nbrs) else np.zeros(1), np.uint32),
            np.ascontiguousarray(prev.entry_points, np.uint32)]
    pg = PrevGraph(len(keep[0]), _p(keep[0]).value, _p(keep[1]).value, _p(keep[2]).value,
                   _p(keep[3]).value, _p(keep[4]).value, len(keep[4]), int(prev.max_level))
    gp = C.POINTER(GraphStruct)()
    L = load_library()
    _check((L.hny_build_incremental_f32 if items.f32 else L.hny_build_incremental)(
        C.byref(o), C.byref(it), _p(ins), len(ins), _p(dl), len(dl), C.byref(pg), C.byref(gp)))
    return Graph(gp, o, items)


class MultiBuilder:
    """hny_multi_builder_*: one resident replica per GPU of this node in ONE process (one host thread
    per GPU, RCCL all-gathers on the builders' streams, hny_multi.cpp); every run() is a complete fresh
    build whose records equal the one-GPU build's."""

    def __init__(self, items, devices=None, n_gpus=0, **kw):
        self.items = items
        self.opts = make_opts(items.metric, items.dim, n_gpus=n_gpus, devices=devices, **kw)
        self._h = C.c_void_p()
        self._replicas = []
        it = items.struct()
        _check(load_library().hny_multi_builder_create(C.byref(self.opts), C.byref(it), C.byref(self._h)))

    @property
    def world(self):
        return int(load_library().hny_multi_builder_world(self._h))

    @property
    def n_collectives(self):
        return int(load_library().hny_multi_builder_collectives(self._h))

    def set_profiling(self, on=True):
        _check(load_library().hny_multi_builder_set_profiling(self._h, int(on)))

    def run(self):
        gp = C.POINTER(GraphStruct)()
        _check(load_library().hny_multi_builder_run(self._h, C.byref(gp)))
        return Graph(gp, self.opts, self.items)

    def replica(self, rank=0):
        """the resident builder of `rank` as a Builder (library-owned: close() on it is a no-op)"""
        h = load_library().hny_multi_builder_replica(self._h, rank)
        if not h:
            raise IndexError(rank)
        b = Builder.__new__(Builder)
        b.items, b.opts, b.incremental = self.items, self.opts, False
        b._h, b._borrowed = C.c_void_p(h), True
        b._mb = self  # the borrowed handle lives exactly as long as this multi-builder: keep it alive ...
        self._replicas.append(b)
        return b

    def close(self):
        if self._h:
            for b in self._replicas:  # ... and make a replica handle unusable once it is gone
                b._h = C.c_void_p()
            self._replicas = []
            load_library().hny_multi_builder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Builder:
    """Stepwise builder (hny_builder_*): vectors stay resident in HBM across reset()/rebuilds."""
    _borrowed = False

    def __init__(self, items, prev=None, to_insert=(), to_delete=(), load=False, stored=None, **kw):
        """prev given -> incremental builder on top of a stored graph (hny_builder_create_incremental);
        with load=True the stored graph is only loaded for searching (hny_builder_load).  stored (an EncodedLinks)
        in place of prev: the same from the Links records as they lie on disk, decoded on the device
        (hny_builder_create_incremental_encoded / hny_builder_load_encoded)"""
        if prev is not None and stored is not None:
            raise ValueError("Builder takes either prev or stored")
        self.items = items
        self.opts = make_opts(items.metric, items.dim, **kw)
        self._h = C.c_void_p()
        self.incremental = prev is not None or stored is not None
        it = items.struct()
        L, f32 = load_library(), items.f32
        if stored is not None:
            if load:
                _check((L.hny_builder_load_encoded_f32 if f32 else L.hny_builder_load_encoded)(
                    C.byref(self.opts), C.byref(it), stored.ptr, C.byref(self._h)))
            else:
                if f32:
                    raise HannoyError(ERR_UNSUPPORTED, "a stepwise incremental builder takes codec bytes")
                ins = u32_ids(to_insert)
                dl = u32_ids(to_delete)
                _check(L.hny_builder_create_incremental_encoded(
                    C.byref(self.opts), C.byref(it), _p(ins), len(ins), _p(dl), len(dl), stored.ptr, C.byref(self._h)))
        elif prev is None:
            _check((L.hny_builder_create_f32 if f32 else L.hny_builder_create)(C.byref(self.opts), C.byref(it), C.byref(self._h)))
        elif load:
            pg, _keep = _prev_struct(prev)
            _check((L.hny_builder_load_f32 if f32 else L.hny_builder_load)(C.byref(self.opts), C.byref(it), C.byref(pg), C.byref(self._h)))
        else:
            if f32:
                raise HannoyError(ERR_UNSUPPORTED, "a stepwise incremental builder takes codec bytes: use build_incremental() "
                                                   "for f32 items")
            ins = u32_ids(to_insert)
            dl = u32_ids(to_delete)
            pg, _keep = _prev_struct(prev)
            _check(load_library().hny_builder_create_incremental(
                C.byref(self.opts), C.byref(it), _p(ins), len(ins), _p(dl), len(dl), C.byref(pg),
                C.byref(self._h)))

    def close(self):
        if self._h and not self._borrowed:
            load_library().hny_builder_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self):
        _check(load_library().hny_builder_reset(self._h))

    def set_profiling(self, on=True):
        _check(load_library().hny_builder_set_profiling(self._h, int(on)))

    def next_batch(self):
        b = Batch()
        _check(load_library().hny_builder_next_batch(self._h, C.byref(b)))
        return b

    def search(self, lo, hi, sel_ptr=None):
        _check(load_library().hny_builder_search(self._h, lo, hi, sel_ptr))

    def apply(self, sel_ptr=None):
        _check(load_library().hny_builder_apply(self._h, sel_ptr))

    def apply_begin(self, sel_ptr=None):
        """emit / sort / append links; returns the number of targets whose list must be re-pruned"""
        n = C.c_uint32()
        _check(load_library().hny_builder_apply_begin(self._h, sel_ptr, C.byref(n)))
        return n.value

    def apply_deferred(self, rank=0, world=1, exch_ptr=None):
        _check(load_library().hny_builder_apply_deferred(self._h, rank, world, exch_ptr))

    def apply_merge(self, exch_ptr=None, rank=0, world=1):
        _check(load_library().hny_builder_apply_merge(self._h, exch_ptr, rank, world))

    @property
    def exch_stride_u64(self):
        return load_library().hny_builder_exch_stride_u64(self._h)

    def sync(self):
        _check(load_library().hny_builder_sync(self._h))

    @property
    def stream_ptr(self):
        """hipStream_t every step is enqueued on (for collectives ordered on the same stream)"""
        L = load_library()
        L.hny_builder_stream.restype = C.c_void_p
        L.hny_builder_stream.argtypes = [C.c_void_p]
        return L.hny_builder_stream(self._h) or 0

    def run(self):
        """All batches on this GPU (what hny_build loops over)."""
        n = 0
        while True:
            b = self.next_batch()
            if b.count == 0:
                break
            self.search(0, b.count)
            self.apply()
            n += 1
        if self.incremental:
            self.fill_gaps()
        return n

    def fill_gaps(self):
        _check(load_library().hny_builder_fill_gaps(self._h))

    def finish(self):
        gp = C.POINTER(GraphStruct)()
        _check(load_library().hny_builder_finish(self._h, C.byref(gp)))
        return Graph(gp, self.opts, self.items)

    def finish_encoded(self):
        """hny_builder_finish_encoded: the Links records with their values serialised on the device"""
        ep = C.POINTER(EncodedLinksStruct)()
        _check(load_library().hny_builder_finish_encoded(self._h, C.byref(ep)))
        return EncodedLinks(ep, self.opts, self.items)

    # -- resident updates (hny_builder_create_update / hny_builder_update) --------------
    def _update_struct(self, upsert_ids, vectors, codes, headers, delete_ids, levels, seed):
        u = Update()
        keep = [u32_ids(upsert_ids), u32_ids(delete_ids)]
        u.n_upsert, u.upsert_ids = len(keep[0]), _p(keep[0]).value
        u.n_delete, u.delete_ids = len(keep[1]), _p(keep[1]).value
        u.seed = int(seed)
        if vectors is not None:
            v = _f32_rows(vectors) if len(keep[0]) else np.zeros((0, self.items.dim), np.float32)
            u.vectors_are_f32, u.vectors = 1, _p(v).value
            u.stride = v.strides[0] if len(v) > 1 else v.shape[1] * 4
            keep.append(v)
        else:
            c = np.ascontiguousarray(codes if codes is not None else np.zeros((0, 1)), np.uint8)
            h = np.ascontiguousarray(headers if headers is not None else np.zeros((0, 1)), np.uint8)
            u.vectors, u.stride = _p(c).value, c.shape[1] if c.ndim == 2 else 0
            u.headers, u.header_size = _p(h).value, h.shape[1] if h.ndim == 2 else 0
            keep += [c, h]
        if levels is not None:
            lv = np.ascontiguousarray(levels, np.uint8)
            u.levels = _p(lv).value
            keep.append(lv)
        return u, keep

    def _successor(self, handle, keep):
        ids = np.union1d(np.setdiff1d(self.items.ids, keep[1]), keep[0]).astype(np.uint32)
        b = Builder.__new__(Builder)
        b.items = _IdsOnly(self.items.metric, self.items.dim, ids)
        b.opts, b.incremental, b._h = self.opts, True, handle
        return b

    def create_update(self, upsert_ids=(), vectors=None, codes=None, headers=None, delete_ids=(), levels=None, seed=42):
        """hny_builder_create_update: an incremental Builder made from this (finished or loaded) builder device to
        device; `vectors` = f32 rows of the upserts, or `codes` + `headers`.  This builder stays usable."""
        u, keep = self._update_struct(upsert_ids, vectors, codes, headers, delete_ids, levels, seed)
        h = C.c_void_p()
        _check(load_library().hny_builder_create_update(self._h, C.byref(u), C.byref(h)))
        return self._successor(h, keep)

    def update(self, upsert_ids=(), vectors=None, codes=None, headers=None, delete_ids=(), levels=None, seed=42,
               full=True, delta=False):
        """hny_builder_update: this Builder becomes its successor (every batch + fill_gaps run); returns the complete
        Graph, the GraphDelta, or (Graph, GraphDelta) as asked.  delta="encoded": the delta is an EncodedDelta
        (finish_delta_encoded on the successor, after hny_builder_update has returned: if that second call fails,
        this Builder is the successor already and finish() / finish_delta() on it give what the update made)"""
        u, keep = self._update_struct(upsert_ids, vectors, codes, headers, delete_ids, levels, seed)
        gp, dp = C.POINTER(GraphStruct)(), C.POINTER(GraphDeltaStruct)()
        if self._borrowed:
            raise HannoyError(ERR_INVALID_ARG, "a borrowed replica cannot be replaced: use create_update()")
        encoded = isinstance(delta, str)
        if encoded and delta != "encoded":
            raise HannoyError(ERR_INVALID_ARG, f"delta={delta!r}: True, False or \"encoded\"")
        _check(load_library().hny_builder_update(C.byref(self._h), C.byref(u), C.byref(gp) if full else None,
                                                 C.byref(dp) if delta and not encoded else None))
        succ = self._successor(self._h, keep)
        self.items, self.incremental = succ.items, True
        succ._h = C.c_void_p()  # (the handle stays with this object)
        g = Graph(gp, self.opts, self.items) if full else None
        d = self.finish_delta_encoded() if encoded else GraphDelta(dp, self.opts) if delta else None
        return (g, d) if full and delta else g if full else d

    # -- resident change of distance (hny_builder_create_changed_distance) ----------
    def create_changed_distance(self, new_metric, levels=None, seed=42, upsert_ids=(), vectors=None, codes=None,
                                headers=None, delete_ids=()):
        """hny_builder_create_changed_distance: a Builder of `new_metric` whose rows are encoded on the device from
        the f32 rows of this (finished or loaded) builder.  `levels`: one per item that exists after the change.
        Upserts are f32 `vectors`, or `codes` + `headers` of the NEW codec.  Kept-links pairs (distance_keeps_links)
        give an incremental Builder on this builder's graph, the others a fresh one.  This builder stays usable."""
        new_metric = int(new_metric)
        u, keep = self._update_struct(upsert_ids, vectors, codes, headers, delete_ids, None, seed)
        c = ChangeDistance()
        c.new_metric, c.seed = new_metric, int(seed)
        if len(keep[0]) or len(keep[1]):
            c.update = C.pointer(u)
        if levels is not None:
            lv = np.ascontiguousarray(levels, np.uint8)
            c.levels = _p(lv).value
            keep.append(lv)
        h = C.c_void_p()
        _check(load_library().hny_builder_create_changed_distance(self._h, C.byref(c), C.byref(h)))
        b = self._successor(h, keep)
        b.items = _IdsOnly(new_metric, self.items.dim, b.items.ids)
        b.opts = BuildOpts.from_buffer_copy(self.opts)
        b.opts.metric, b.opts.seed = new_metric, int(seed)
        b._opts_keep = self.opts  # (the callbacks the copied pointers refer to)
        b.incremental = distance_keeps_links(self.items.metric, new_metric)
        return b

    def recode_items(self, new_metric):
        """hny_builder_recode_items: (codes, headers) of this builder's items as `new_metric` stores them, encoded on
        the device from the resident f32 rows; ascending id order"""
        n = self.items.n
        codes = np.zeros((n, vector_bytes(new_metric, self.items.dim)), np.uint8)
        headers = np.zeros((n, header_bytes(new_metric)), np.uint8)
        _check(load_library().hny_builder_recode_items(self._h, int(new_metric), _p(codes), _p(headers)))
        return codes, headers

    def finish_delta(self):
        dp = C.POINTER(GraphDeltaStruct)()
        _check(load_library().hny_builder_finish_delta(self._h, C.byref(dp)))
        return GraphDelta(dp, self.opts)

    def finish_delta_encoded(self):
        """hny_builder_finish_delta_encoded: finish_delta's records with their values serialised on the device"""
        dp = C.POINTER(EncodedDeltaStruct)()
        _check(load_library().hny_builder_finish_delta_encoded(self._h, C.byref(dp)))
        return EncodedDelta(dp, self.opts)

    def distances(self, slot_a, slot_b):
        a = np.ascontiguousarray(slot_a, np.uint32)
        b = np.ascontiguousarray(slot_b, np.uint32)
        out = np.zeros(len(a), np.float32)
        _check(load_library().hny_builder_distances(self._h, len(a), _p(a), _p(b), _p(out)))
        return out

    def search_knn(self, qcodes, qheaders, k=10, ef_search=100):
        """Reader::nns(k).by_vector (/root/reference/src/reader.rs:132-148) on the built graph."""
        (nq, qc, qs, qh, _), _keep = _query_source(qcodes=qcodes, qheaders=qheaders)
        out = _result_arrays(nq, k)
        _check(load_library().hny_builder_search_knn(self._h, nq, qc, qs, qh, k, ef_search, *map(_p, out)))
        return out

    def export_items(self):
        """hny_builder_export_items: (codes [n, vector_bytes], headers [n, header_bytes]) of the builder's items in
        ascending id order, read back from HBM"""
        n = self.items.n
        codes = np.zeros((n, vector_bytes(self.items.metric, self.items.dim)), np.uint8)
        headers = np.zeros((n, header_bytes(self.items.metric)), np.uint8)
        _check(load_library().hny_builder_export_items(self._h, _p(codes), _p(headers)))
        return codes, headers

    def search_knn_f32(self, queries, k=10, ef_search=100):
        """search_knn with the &[f32] queries the reference takes, encoded on the device"""
        (nq, qc, qs, _, _), _keep = _query_source(qf32=_f32_rows(queries))
        out = _result_arrays(nq, k)
        _check(load_library().hny_builder_search_knn_f32(self._h, nq, qc, qs, k, ef_search, *map(_p, out)))
        return out

    def _search(self, name, opts, source, f32, filters=None):
        """One call of the entry point `name` that takes hny_query_opts, of its _f32 form for f32 queries: `opts`
        from _query_opts, `source` from _query_source, `filters` from QueryFilters.pack.  Returns (ids, dists,
        counts) and sets did_cancel."""
        qo, _keep, flag = opts
        (nq, qc, qs, qh, qi), _arrays = source
        if filters is not None and len(filters[1][2]) != nq:
            raise ValueError(f"filter_of has {len(filters[1][2])} entries for {nq} queries")
        self._cancel_flag = flag
        out = _result_arrays(nq, qo.k)
        head = (self._h, C.byref(qo)) + (() if filters is None else (C.byref(filters[0]),))
        if f32:
            _check(getattr(load_library(), name + "_f32")(*head, nq, qc, qs, *map(_p, out)))
        else:
            _check(getattr(load_library(), name)(*head, nq, qc, qs, qh, qi, *map(_p, out)))
        self.did_cancel = bool(flag.value)
        return out

    def nns_f32(self, queries, **kw):
        """nns(by_vector) with f32 queries, encoded on the device"""
        return self.nns(qf32=_f32_rows(queries), **kw)

    def nns(self, qcodes=None, qheaders=None, k=10, ef_search=100, candidates=None, query_items=None,
            linear_below=1000, linear_below_ratio=1.0, cancel=None, qf32=None):
        """Reader::nns(k).ef_search(..).candidates(..).linear_below(..).by_vector / .by_item
        (/root/reference/src/reader.rs:60-262).  counts == NNS_NONE where by_item returns None.
        cancel: the closure of the *_with_cancellation variants; self.did_cancel tells whether it fired."""
        opts = _query_opts(k, ef_search, linear_below, linear_below_ratio, candidates, cancel)
        return self._search("hny_builder_nns", opts, _query_source(query_items, qf32, qcodes, qheaders),
                            qf32 is not None)

    def nns_filtered_f32(self, queries, filters, filter_of, **kw):
        """nns_filtered(by_vector) with f32 queries, encoded on the device"""
        return self.nns_filtered(filters, filter_of, qf32=_f32_rows(queries), **kw)

    def nns_filtered(self, filters, filter_of, qcodes=None, qheaders=None, k=10, ef_search=100, query_items=None,
                     linear_below=1000, linear_below_ratio=1.0, cancel=None, qf32=None):
        """hny_builder_nns_filtered: nns with one .candidates() filter per query.  `filters` is a list of id arrays,
        `filter_of[i]` the filter of query i (-1 or NNS_FILTER_NONE: none).  The rows of the queries of one filter
        equal nns(candidates=that filter) on those queries alone."""
        opts = _query_opts(k, ef_search, linear_below, linear_below_ratio, cancel=cancel)
        qf = QueryFilters.pack(filters, filter_of)
        return self._search("hny_builder_nns_filtered", opts, _query_source(query_items, qf32, qcodes, qheaders),
                            qf32 is not None, qf)

    def exact_knn_f32(self, queries, **kw):
        """exact_knn(by_vector) with f32 queries, encoded on the device"""
        return self.exact_knn(qf32=_f32_rows(queries), **kw)

    def exact_knn(self, qcodes=None, qheaders=None, k=10, candidates=None, query_items=None, cancel=None, qf32=None):
        """hny_builder_exact_knn: the k nearest of the live items (or of `candidates` among them) by a flat scan —
        brute_force_search's result, the ground truth of the index's own distances.  Returns (ids, dists, counts)
        like nns; counts == NNS_NONE where by_item names an unknown item."""
        opts = _query_opts(k, candidates=candidates, cancel=cancel)
        return self._search("hny_builder_exact_knn", opts, _query_source(query_items, qf32, qcodes, qheaders),
                            qf32 is not None)

    def _range(self, radius, count_only, qcodes, qheaders, candidates, query_items, cancel, qf32, max_total,
               filters=None):
        """One call of hny_builder_exact_range in the form the arguments name; `filters`: ("filtered" | "bitsets",
        QueryFilters.pack's / QueryBitsets.pack's result) for the calls with a filter per query"""
        (nq, qc, qs, qh, qi), _arrays = _query_source(query_items, qf32, qcodes, qheaders)
        ro, _keep, flag = _range_opts(radius, nq, candidates, cancel, max_total)
        if filters is not None and len(filters[1][1][2]) != nq:
            raise ValueError(f"filter_of has {len(filters[1][1][2])} entries for {nq} queries")
        self._cancel_flag = flag
        L = load_library()
        name = ("hny_builder_exact_range" + ("_count" if count_only else "") +
                ("" if filters is None else "_" + filters[0]) + ("_f32" if qf32 is not None else ""))
        head = (self._h, C.byref(ro)) + (() if filters is None else (C.byref(filters[1][0]),))
        src = (nq, qc, qs) if qf32 is not None else (nq, qc, qs, qh, qi)
        if count_only:
            counts = np.zeros(nq, np.uint64)
            _check(getattr(L, name)(*head, *src, _p(counts)))
            self.did_cancel = bool(flag.value)
            return counts
        res = C.POINTER(RangeResult)()
        _check(getattr(L, name)(*head, *src, C.byref(res)))
        try:
            r = res.contents
            offsets = np.ctypeslib.as_array(r.offsets, (nq + 1,)).copy()
            total = int(offsets[-1])
            ids = np.ctypeslib.as_array(r.ids, (total,)).copy() if total else np.zeros(0, np.uint32)
            dists = np.ctypeslib.as_array(r.dists, (total,)).copy() if total else np.zeros(0, np.float32)
            is_none = np.ctypeslib.as_array(r.is_none, (nq,)).copy() if nq else np.zeros(0, np.uint8)
        finally:
            L.hny_range_result_free(res)
        self.did_cancel = bool(flag.value)
        return offsets, ids, dists, is_none

    def exact_range(self, radius, qcodes=None, qheaders=None, candidates=None, query_items=None, cancel=None,
                    qf32=None, max_total=0):
        """hny_builder_exact_range: every live item (or every one of `candidates` among them) whose distance to query
        i is <= radius[i] (a scalar holds for every query), ordered by (distance bits, item id).  Returns (offsets
        [nq + 1], ids, dists, is_none): the hits of query i are ids / dists[offsets[i]:offsets[i + 1]]; is_none is 1
        where by_item names an unknown item.  max_total != 0: more hits than that in all are refused."""
        return self._range(radius, False, qcodes, qheaders, candidates, query_items, cancel, qf32, max_total)

    def exact_range_f32(self, queries, radius, **kw):
        """exact_range(by_vector) with f32 queries, encoded on the device"""
        return self.exact_range(radius, qf32=_f32_rows(queries), **kw)

    def exact_range_count(self, radius, qcodes=None, qheaders=None, candidates=None, query_items=None, cancel=None,
                          qf32=None):
        """hny_builder_exact_range_count: the sizes of exact_range's rows alone (uint64), RANGE_NONE where by_item
        names an unknown item; one scan, nothing is emitted or sorted"""
        return self._range(radius, True, qcodes, qheaders, candidates, query_items, cancel, qf32, 0)

    def exact_range_count_f32(self, queries, radius, **kw):
        """exact_range_count(by_vector) with f32 queries, encoded on the device"""
        return self.exact_range_count(radius, qf32=_f32_rows(queries), **kw)

    def exact_range_filtered(self, radius, filters, filter_of, qcodes=None, qheaders=None, query_items=None,
                             cancel=None, qf32=None, max_total=0):
        """hny_builder_exact_range_filtered: exact_range with one .candidates() filter per query, `filters` and
        `filter_of` as in nns_filtered.  The rows of the queries of one filter equal exact_range(candidates=that
        filter) on those queries alone; the result is in call order."""
        qf = ("filtered", QueryFilters.pack(filters, filter_of))
        return self._range(radius, False, qcodes, qheaders, None, query_items, cancel, qf32, max_total, qf)

    def exact_range_filtered_f32(self, queries, radius, filters, filter_of, **kw):
        """exact_range_filtered(by_vector) with f32 queries, encoded on the device"""
        return self.exact_range_filtered(radius, filters, filter_of, qf32=_f32_rows(queries), **kw)

    def exact_range_count_filtered(self, radius, filters, filter_of, qcodes=None, qheaders=None, query_items=None,
                                   cancel=None, qf32=None):
        """hny_builder_exact_range_count_filtered: the sizes of exact_range_filtered's rows alone, one scan"""
        qf = ("filtered", QueryFilters.pack(filters, filter_of))
        return self._range(radius, True, qcodes, qheaders, None, query_items, cancel, qf32, 0, qf)

    def exact_range_count_filtered_f32(self, queries, radius, filters, filter_of, **kw):
        """exact_range_count_filtered(by_vector) with f32 queries, encoded on the device"""
        return self.exact_range_count_filtered(radius, filters, filter_of, qf32=_f32_rows(queries), **kw)

    def exact_range_bitsets(self, radius, bits, n_bits, filter_of, qcodes=None, qheaders=None, query_items=None,
                            cancel=None, qf32=None, max_total=0):
        """hny_builder_exact_range_bitsets: exact_range_filtered with the filters as bitsets over item ids, `bits`,
        `n_bits` and `filter_of` as in nns_bitsets.  Equal to exact_range_filtered on the set bits of each filter."""
        qb = ("bitsets", QueryBitsets.pack(bits, n_bits, filter_of))
        return self._range(radius, False, qcodes, qheaders, None, query_items, cancel, qf32, max_total, qb)

    def exact_range_bitsets_f32(self, queries, radius, bits, n_bits, filter_of, **kw):
        """exact_range_bitsets(by_vector) with f32 queries, encoded on the device"""
        return self.exact_range_bitsets(radius, bits, n_bits, filter_of, qf32=_f32_rows(queries), **kw)

    def exact_range_count_bitsets(self, radius, bits, n_bits, filter_of, qcodes=None, qheaders=None, query_items=None,
                                  cancel=None, qf32=None):
        """hny_builder_exact_range_count_bitsets: the sizes of exact_range_bitsets' rows alone, one scan"""
        qb = ("bitsets", QueryBitsets.pack(bits, n_bits, filter_of))
        return self._range(radius, True, qcodes, qheaders, None, query_items, cancel, qf32, 0, qb)

    def exact_range_count_bitsets_f32(self, queries, radius, bits, n_bits, filter_of, **kw):
        """exact_range_count_bitsets(by_vector) with f32 queries, encoded on the device"""
        return self.exact_range_count_bitsets(radius, bits, n_bits, filter_of, qf32=_f32_rows(queries), **kw)

    def exact_knn_filtered_f32(self, queries, filters, filter_of, **kw):
        """exact_knn_filtered(by_vector) with f32 queries, encoded on the device"""
        return self.exact_knn_filtered(filters, filter_of, qf32=_f32_rows(queries), **kw)

    def exact_knn_filtered(self, filters, filter_of, qcodes=None, qheaders=None, k=10, query_items=None, cancel=None,
                           qf32=None):
        """hny_builder_exact_knn_filtered: exact_knn with one .candidates() filter per query, `filters` and
        `filter_of` as in nns_filtered.  The rows of the queries of one filter equal exact_knn(candidates=that
        filter) on those queries alone: counts[i] = min(k, live candidates of query i's filter)."""
        opts = _query_opts(k, cancel=cancel)
        qf = QueryFilters.pack(filters, filter_of)
        return self._search("hny_builder_exact_knn_filtered", opts,
                            _query_source(query_items, qf32, qcodes, qheaders), qf32 is not None, qf)

    def nns_bitsets_f32(self, queries, bits, n_bits, filter_of, **kw):
        """nns_bitsets(by_vector) with f32 queries, encoded on the device"""
        return self.nns_bitsets(bits, n_bits, filter_of, qf32=_f32_rows(queries), **kw)

    def nns_bitsets(self, bits, n_bits, filter_of, qcodes=None, qheaders=None, k=10, ef_search=100, query_items=None,
                    linear_below=1000, linear_below_ratio=1.0, cancel=None, qf32=None):
        """hny_builder_nns_bitsets: nns_filtered with the filters as bitsets over item ids, `bits` a uint32
        [n_filters, words] array (np.packbits(mask, bitorder="little").view("<u4")) that covers ids 0 .. n_bits-1.
        Equal to nns_filtered on the set bits of each filter."""
        opts = _query_opts(k, ef_search, linear_below, linear_below_ratio, cancel=cancel)
        qb = QueryBitsets.pack(bits, n_bits, filter_of)
        return self._search("hny_builder_nns_bitsets", opts, _query_source(query_items, qf32, qcodes, qheaders),
                            qf32 is not None, qb)

    def exact_knn_bitsets_f32(self, queries, bits, n_bits, filter_of, **kw):
        """exact_knn_bitsets(by_vector) with f32 queries, encoded on the device"""
        return self.exact_knn_bitsets(bits, n_bits, filter_of, qf32=_f32_rows(queries), **kw)

    def exact_knn_bitsets(self, bits, n_bits, filter_of, qcodes=None, qheaders=None, k=10, query_items=None,
                          cancel=None, qf32=None):
        """hny_builder_exact_knn_bitsets: exact_knn_filtered with the filters as bitsets over item ids, `bits`,
        `n_bits` and `filter_of` as in nns_bitsets.  Equal to exact_knn_filtered on the set bits of each filter."""
        opts = _query_opts(k, cancel=cancel)
        qb = QueryBitsets.pack(bits, n_bits, filter_of)
        return self._search("hny_builder_exact_knn_bitsets", opts,
                            _query_source(query_items, qf32, qcodes, qheaders), qf32 is not None, qb)

    def exact_rows_read(self):
        """(tile, row) loads of the dense scan in the last exact_knn_filtered / exact_range_filtered call (or their
        bitsets forms) on this builder, both passes of a range call; 0 if none ran"""
        return int(load_library().hny_builder_exact_rows_read(self._h))
