"""ctypes binding of libgcnspmm.so (the C ABI declared in include/gcn_spmm.h).

The product path has NO CPU fallback: if the library is missing or a call returns a
non-zero status, a GcnAmdError is raised.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (GCN_AMD_LIB: load a private copy — long-running host tools that must survive a rebuild of the in-tree library)
LIB_PATH = os.environ.get("GCN_AMD_LIB") or os.path.join(_HERE, "lib", "libgcnspmm.so")
DROPIN_DIR = os.path.join(_HERE, "dropin")


class GcnAmdError(RuntimeError):
    status = None            # the C-ABI status code when the error came from a call (include/gcn_spmm.h), else None


ERR_NOT_FACTORED = 6         # GCN_ERR_NOT_FACTORED
ERR_INTERNAL = 7             # GCN_ERR_INTERNAL (a consistency guard tripped: gcn_order_rabbit_device)
DTYPE_F32, DTYPE_BF16 = 0, 1 # GCN_DTYPE_F32 / GCN_DTYPE_BF16 (gcn_spmm_csr_bf16_epilogue)
REDUCE_MAX, REDUCE_MIN = 0, 1 # GCN_REDUCE_MAX / GCN_REDUCE_MIN (gcn_aggregate_csr)
REDUCE_SUM = 2               # GCN_REDUCE_SUM (gcn_edge_aggregate_csr_f32)
EDGE_OP_ADD, EDGE_OP_MUL = 0, 1      # GCN_EDGE_OP_*: how a node row and an entry's row of features meet
EDGE_ACT_NONE, EDGE_ACT_RELU = 0, 1  # GCN_EDGE_ACT_*
SAMPLE_LONG_ROW = 2048       # GCN_SAMPLE_LONG_ROW: longer rows get a workgroup, not a wave (gcn_sample_neighbors_csr)
SAMPLE_WS_BYTES = 16         # GCN_SAMPLE_WS_BYTES
SUBGRAPH_WS_BYTES = 16       # GCN_SUBGRAPH_WS_BYTES (gcn_induced_subgraph_count_csr / _fill_csr)
BUCKET_WAVE_MAX = 256        # GCN_BUCKET_WAVE_MAX: longer buckets are ordered by a workgroup in LDS, not a wave (gcn_bucket_fill_i32)
BUCKET_BLOCK_MAX = 8192      # GCN_BUCKET_BLOCK_MAX: longer buckets are ordered in place in global memory
COALESCE_WS_BYTES = 16       # GCN_COALESCE_WS_BYTES (gcn_csr_coalesce_count / _fill)
COALESCE_SUM, COALESCE_MAX, COALESCE_MIN, COALESCE_FIRST = 0, 1, 2, 3   # GCN_COALESCE_*: the value of a merged run
DIAG_KEEP, DIAG_DROP, DIAG_FILL, DIAG_ADD = 0, 1, 2, 3                   # GCN_DIAG_*: what the merge does to the diagonal
NORM_SYM, NORM_ROW = 0, 1    # GCN_NORM_SYM / GCN_NORM_ROW (gcn_csr_normalize_f32)
SPGEMM_WAVE_MAX = 512        # GCN_SPGEMM_WAVE_MAX: rows of at most this many possible columns are taken by a wave (gcn_spgemm_*_csr)
SPGEMM_BLOCK_MAX = 8192      # GCN_SPGEMM_BLOCK_MAX: ... by a workgroup with a table in LDS; above, a dense accumulator
SPGEMM_DENSE_BLOCKS = 16     # GCN_SPGEMM_DENSE_BLOCKS: the workgroups (and accumulators in the workspace) of the dense rows
SAMPLED_DOT_WS_BYTES = 16    # GCN_SAMPLED_DOT_WS_BYTES (gcn_csr_sampled_dot_f32)
KNN_K_MAX = 64               # GCN_KNN_K_MAX: the most neighbours gcn_knn_f32 returns per query
KNN_TILE_Q = 64              # GCN_KNN_TILE_Q: queries of a workgroup
KNN_TILE_C = 64              # GCN_KNN_TILE_C: candidates of a tile; the candidate range is split in whole tiles


def bucket_ws_bytes(count, nbuckets):
    """bytes of device scratch gcn_bucket_fill_i32 needs (the rule written out in include/gcn_spmm.h): four counters, a
    cursor per bucket, and a list for each ordering tier as long as the number of buckets that can reach the tier"""
    count, nbuckets = int(count), int(nbuckets)
    ints = 4 + nbuckets + sum(min(nbuckets, count // (above + 1)) for above in (1, BUCKET_WAVE_MAX, BUCKET_BLOCK_MAX))
    return (ints * 4 + 15) // 16 * 16


def spgemm_ws_bytes(m, n):
    """bytes of device scratch gcn_spgemm_count_csr / _fill_csr need (gcn_spgemm_ws_bytes, written out in
    include/gcn_spmm.h): two flags, a product count per row, and per dense-row workgroup n stamps and n floats"""
    return 16 + (4 * int(m) + 15) // 16 * 16 + 8 * int(n) * SPGEMM_DENSE_BLOCKS


def knn_splits(q, n, splits, cus=256):
    """parts of the candidate range gcn_knn_f32 works with (gcn_knn_splits, the rule written out in include/gcn_spmm.h):
    splits >= 1 as given, 0 = two workgroups per CU but at least 8 tiles per part (not measured); then within [1, tiles]"""
    q, n, splits, cus = int(q), int(n), int(splits), int(cus)
    blocks, tiles = -(-q // KNN_TILE_Q), -(-n // KNN_TILE_C)
    if splits <= 0:
        splits = min(-(-2 * (cus if cus > 0 else 256) // blocks), tiles // 8) if blocks > 0 else 1
    return max(1, min(splits, tiles))


def knn_ws_bytes(q, n, k, splits, cus=256):
    """bytes of device scratch gcn_knn_f32 needs (gcn_knn_ws_bytes, written out in include/gcn_spmm.h): k keys of 8 bytes
    and one fp64 partial sum for every (query, part)"""
    return 16 + (8 * int(q) * knn_splits(q, n, splits, cus) * (int(k) + 1) + 15) // 16 * 16


def spgemm_slots(k):
    """slots of the hash table of a row with K = k possible columns: the power of two >= 2 k, at least 64"""
    s = 64
    while s < 2 * int(k):
        s *= 2
    return s


_c_i32 = ctypes.c_int32
_c_p = ctypes.c_void_p

# name -> (restype, argtypes)  — one entry per symbol declared in include/gcn_spmm.h
SIGNATURES = {
    "gcn_status_string": (ctypes.c_char_p, [ctypes.c_int]),
    "gcn_version": (ctypes.c_char_p, []),
    "gcn_device_cu_count": (ctypes.c_int, []),
    "gcn_spmm_plan_create": (ctypes.c_int, [ctypes.POINTER(_c_p), _c_p, _c_i32, _c_i32, _c_i32, _c_i32, _c_p]),
    "gcn_spmm_plan_destroy": (ctypes.c_int, [_c_p]),
    "gcn_spmm_plan_num_chunks": (_c_i32, [_c_p]),
    "gcn_spmm_plan_chunk_nnz": (_c_i32, [_c_p]),
    "gcn_spmm_plan_workspace_bytes": (ctypes.c_size_t, [_c_p, _c_i32]),
    "gcn_spmm_csr_f32": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i32, _c_p]),
    "gcn_spmm_csr_f32_bias_relu": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i32, _c_i32, _c_p]),
    "gcn_spmm_csr_f32_epilogue": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i32, ctypes.c_float,
                                                 ctypes.c_uint64, ctypes.c_uint64, _c_i32, _c_p]),
    "gcn_dropout_f32": (ctypes.c_int, [_c_p, _c_p, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64, _c_p]),
    "gcn_spmm_csr_bf16_epilogue": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i32, _c_p, _c_i32, ctypes.c_float,
                                                  ctypes.c_uint64, ctypes.c_uint64, _c_i32, _c_p]),
    "gcn_spmm_csr_bf16": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i32, _c_i32, _c_p]),
    "gcn_dropout_bf16": (ctypes.c_int, [_c_p, _c_p, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint64, _c_p]),
    "gcn_spmm_plan_set_tile_cols": (ctypes.c_int, [_c_p, _c_i32]),
    "gcn_spmm_plan_set_blocks_per_cu": (ctypes.c_int, [_c_p, _c_i32]),
    "gcn_spmm_plan_set_gather_width": (ctypes.c_int, [_c_p, _c_i32]),
    "gcn_exchange_flags_create": (ctypes.c_int, [_c_i32, _c_p, _c_p]),
    "gcn_exchange_flags_open": (ctypes.c_int, [_c_p, _c_p]),
    "gcn_exchange_flags_close": (ctypes.c_int, [_c_p]),
    "gcn_exchange_flags_destroy": (ctypes.c_int, [_c_p]),
    "gcn_exchange_push": (ctypes.c_int, [_c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_exchange_signal": (ctypes.c_int, [_c_p, _c_p, _c_p]),
    "gcn_exchange_wait": (ctypes.c_int, [_c_p, _c_i32, _c_i32, _c_i32, _c_p, ctypes.c_double, _c_p]),
    "gcn_spmm_plan_num_passes": (_c_i32, [_c_p, _c_i32]),
    "gcn_spmm_plan_main_kernel": (ctypes.c_int, [_c_p, _c_i32, _c_i32, ctypes.c_char_p, _c_i32]),
    "gcn_spmm_plan_main_kernel_bf16": (ctypes.c_int, [_c_p, _c_i32, _c_i32, ctypes.c_char_p, _c_i32]),
    "gcn_spmm_plan_enable_slicing": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_p, _c_i32, _c_p]),
    "gcn_spmm_plan_num_slices": (_c_i32, [_c_p]),
    "gcn_spmm_plan_narrow_slices": (_c_i32, [_c_p, _c_i32]),
    "gcn_spmm_plan_prepare_width": (_c_i32, [_c_p, _c_p, _c_p, _c_p, _c_i32, _c_p]),
    "gcn_spmm_plan_set_value_factors": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "gcn_spmm_plan_has_value_factors": (_c_i32, [_c_p]),
    "gcn_spmm_plan_set_values_mutable": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_p, _c_p]),
    "gcn_spmm_plan_values_mutable": (_c_i32, [_c_p]),
    "gcn_spmm_plan_update_values": (ctypes.c_int, [_c_p, _c_p, _c_p]),
    "gcn_sddmm_csr_f32": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i32, _c_p]),
    "gcn_edge_softmax_csr_f32": (ctypes.c_int, [_c_p, _c_i32, _c_i32, _c_p, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_edge_softmax_backward_csr_f32": (ctypes.c_int, [_c_p, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_gat_edge_softmax_csr_f32": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_p, _c_p, ctypes.c_float, _c_p, _c_p,
                                                    ctypes.c_size_t, _c_p]),
    "gcn_gat_edge_softmax_backward_csr_f32": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_p, _c_p, ctypes.c_float, _c_p, _c_p,
                                                             _c_p, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_segment_sum_csr_f32": (ctypes.c_int, [_c_p, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_heads_ws_bytes": (ctypes.c_int, [_c_i32, _c_i32, _c_i32, _c_i32, ctypes.POINTER(ctypes.c_size_t)]),
    "gcn_edge_softmax_heads_csr_f32": (ctypes.c_int, [_c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_edge_softmax_heads_backward_csr_f32": (ctypes.c_int, [_c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_p, ctypes.c_size_t,
                                                               _c_p]),
    "gcn_gat_edge_softmax_heads_csr_f32": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_p, ctypes.c_float, _c_p, _c_p,
                                                          ctypes.c_size_t, _c_p]),
    "gcn_gat_edge_softmax_heads_backward_csr_f32": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_p, ctypes.c_float,
                                                                   _c_p, _c_p, _c_p, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_segment_sum_heads_csr_f32": (ctypes.c_int, [_c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_spmm_heads_csr_f32": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_p,
                                              ctypes.c_size_t, _c_p]),
    "gcn_sddmm_heads_csr_f32": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_p, ctypes.c_size_t,
                                               _c_p]),
    "gcn_gatv2_ws_bytes": (ctypes.c_int, [_c_i32, _c_i32, _c_i32, _c_i32, ctypes.POINTER(ctypes.c_size_t)]),
    "gcn_gatv2_scores_csr_f32": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_p, ctypes.c_float, _c_p,
                                                _c_p, ctypes.c_size_t, _c_p]),
    "gcn_gatv2_scores_backward_csr_f32": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_p,
                                                         ctypes.c_float, _c_p, _c_p, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_aggregate_csr": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_p,
                                         ctypes.c_size_t, _c_p]),
    "gcn_aggregate_backward_csr": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_i32, _c_p, _c_i32, _c_p, _c_p,
                                                  ctypes.c_size_t, _c_p]),
    "gcn_edge_aggregate_csr_f32": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_i32,
                                                  _c_p, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_edge_aggregate_backward_x_csr_f32": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_i32,
                                                             _c_i32, _c_i32, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_edge_aggregate_backward_e_csr_f32": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_i32,
                                                             _c_i32, _c_i32, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_sample_neighbors_csr": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_p, _c_i32, _c_i32, ctypes.c_uint64, ctypes.c_uint64,
                                                _c_p, _c_p, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_induced_subgraph_count_csr": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_p, _c_i32, _c_p, _c_p, _c_p, ctypes.c_size_t,
                                                      _c_p]),
    "gcn_induced_subgraph_fill_csr": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_p, _c_i32, _c_p, _c_p, _c_p, _c_p, _c_p,
                                                     ctypes.c_size_t, _c_p]),
    "gcn_random_walk_csr": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_p, _c_i32, _c_i32, ctypes.c_uint64, ctypes.c_uint64, _c_p,
                                           _c_p]),
    "gcn_csr_find_entries": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_p, _c_p, _c_i32, _c_p, _c_p]),
    "gcn_negative_sample_csr": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_i32, _c_i32, _c_i32, _c_i32,
                                               ctypes.c_uint64, ctypes.c_uint64, _c_p, _c_p]),
    "gcn_bucket_count_i32": (ctypes.c_int, [_c_p, _c_i32, _c_i32, _c_p, _c_p]),
    "gcn_bucket_fill_i32": (ctypes.c_int, [_c_p, _c_i32, _c_i32, _c_p, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_csr_transpose_gather": (ctypes.c_int, [_c_p, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "gcn_csr_coalesce_count": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_i32, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_csr_coalesce_fill": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, ctypes.c_float, _c_p, _c_p,
                                             _c_p, _c_p, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_csr_degree_f64": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_p, _c_p]),
    "gcn_csr_normalize_f32": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_i32, _c_p, _c_p]),
    "gcn_spgemm_ws_bytes": (ctypes.c_int, [_c_i32, _c_i32, ctypes.POINTER(ctypes.c_size_t)]),
    "gcn_spgemm_count_csr": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_i32, _c_i32, _c_p, _c_p,
                                            ctypes.c_size_t, _c_p]),
    "gcn_spgemm_fill_csr": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_i32, _c_i32, _c_p, _c_p,
                                           _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_csr_sampled_dot_f32": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_i32, _c_p, _c_p, _c_p, _c_i32,
                                               _c_i32, _c_i32, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_knn_splits": (ctypes.c_int, [_c_i32, _c_i32, _c_i32]),
    "gcn_knn_ws_bytes": (ctypes.c_int, [_c_i32, _c_i32, _c_i32, _c_i32, ctypes.POINTER(ctypes.c_size_t)]),
    "gcn_knn_f32": (ctypes.c_int, [_c_p, ctypes.c_int64, _c_p, ctypes.c_int64, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32, _c_i32,
                                   _c_p, _c_p, _c_p, _c_p, ctypes.c_size_t, _c_p]),
    "gcn_spmm_plan_sddmm_kernel":(ctypes.c_int, [_c_p, _c_i32, ctypes.c_char_p, _c_i32]),
    "gcn_spmm_plan_enable_panels": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_p, _c_i32, _c_p]),
    "gcn_spmm_plan_panel_rows": (_c_i32, [_c_p]),
    "gcn_spmm_plan_panel_coverage": (ctypes.c_double, [_c_p]),
    "gcn_spmm_plan_dense_panels": (_c_i32, [_c_p]),
    "gcn_spmm_profile_begin": (ctypes.c_int, [_c_p, _c_i32]),
    "gcn_spmm_profile_end": (ctypes.c_int, [_c_p, _c_p, _c_p]),
    "gcn_spmm_csr_f32_oneshot": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_i32, _c_p]),
    "gcn_spmm_plan_prelaid_layout": (ctypes.c_int, [_c_p, _c_i32, _c_p, _c_p, _c_p, _c_p]),
    "gcn_spmm_csr_f32_prelaid": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i32, _c_i32, _c_p]),
    "gcn_spmm_auto_slices": (_c_i32, [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, _c_i32]),
    "gcn_spmm_group_addressing": (_c_i32, [ctypes.c_int64, _c_i32]),
    "gcn_gather_rows_f32": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_i32, _c_i32, _c_p]),
    "gcn_order_deg_device": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_i32, _c_p, _c_p]),
    "gcn_order_rcm_device": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_p, _c_p, _c_p]),
    "gcn_csr_apply_rank_device": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_p, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_p, _c_p]),
    "gcn_order_rabbit_device": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_p]),
    "gcn_order_rabbit": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_p, _c_p]),
    "gcn_order_deg": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_i32, _c_p]),
    "gcn_order_rcm": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_p]),
    "gcn_order_gorder": (ctypes.c_int, [_c_p, _c_p, _c_i32, _c_i32, _c_i32, _c_p]),
    "gcn_csr_apply_rank": (ctypes.c_int, [_c_p, _c_p, _c_p, _c_i32, _c_i32, _c_p, _c_p]),
    # drop-in symbols (reference signatures; void)
    "dfs": (None, [_c_p, _c_p, _c_p, _c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "gorder": (None, [_c_p, _c_p, _c_p, _c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "perm_apply": (None, [_c_p, _c_p, _c_p, _c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "rabbit": (None, [_c_p, _c_p, _c_p, _c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "csr2seg_Cmajor": (None, [ctypes.c_int, _c_p, _c_p, _c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_p, _c_p, _c_p, _c_p,
                              ctypes.c_int, _c_p]),
    "csr2tile": (None, [_c_p, _c_p, _c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_p, _c_p, _c_p,
                        _c_p, _c_p, _c_p, ctypes.c_int, _c_p]),
    "flexspmm": (None, [_c_p, _c_p, _c_p, _c_p, _c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                        ctypes.c_int, _c_p, _c_p]),
    "permutate": (None, [_c_p, _c_p, _c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "cuspmm": (None, [_c_p, _c_p, _c_p, _c_p, _c_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
}

_lib = None


def load(path=None):
    """Load (once) and return the ctypes handle; raises GcnAmdError if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise GcnAmdError(
            f"{p} not found: the HIP library is not built. Run `python -m gcn_amd.build` "
            "(there is no CPU fallback for the SpMM path).")
    try:
        lib = ctypes.CDLL(p)
    except OSError as e:  # pragma: no cover - environment dependent
        raise GcnAmdError(f"cannot load {p}: {e}") from e
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise GcnAmdError(f"{p} does not export `{name}` declared in include/gcn_spmm.h") from e
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def check(status, what):
    if status != 0:
        msg = load().gcn_status_string(status).decode()
        err = GcnAmdError(f"{what}: {msg} (status {status})")
        err.status = int(status)
        raise err


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream_ptr(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_Tensor = torch.Tensor
_calls = {}                  # name -> (function, number of arguments): resolved once per name


def call(name, *args, device=None):
    """One call of the status-returning C-ABI function `name`: a torch.Tensor argument goes as its address, None as a null
    pointer, everything else as it is.  With `device` the call runs under ``torch.cuda.device(device)`` and that device's
    current stream is appended as the last argument.  A non-zero status raises GcnAmdError under `name`, `.status` set.
    Nothing else: no ``.contiguous()``, no dtype or shape checks.  TypeError for a wrong number of arguments (before the
    library is entered: ctypes lets surplus arguments through), GcnAmdError for a name include/gcn_spmm.h does not declare."""
    try:
        fn, nargs = _calls[name]
    except KeyError:
        if name not in SIGNATURES:
            raise GcnAmdError(f"`{name}` is not a function declared in include/gcn_spmm.h") from None
        fn, nargs = _calls[name] = getattr(load(), name), len(SIGNATURES[name][1])
    if len(args) + (device is not None) != nargs:
        raise TypeError(f"{name} takes {nargs} arguments ({len(args) + (device is not None)} given)")
    args = [a.data_ptr() if isinstance(a, _Tensor) else a for a in args]    # (an int under a void* argtype is the address)
    if device is None:
        status = fn(*args)
    else:
        with torch.cuda.device(device):
            status = fn(*args, torch.cuda.current_stream(device).cuda_stream)
    if status != 0:
        check(status, name)
