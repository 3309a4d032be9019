"""ctypes binding of the C ABI in include/alpgpu.h (libalpgpu.so) — Python-side plumbing only.

The codec runs entirely in hand-written HIP kernels behind the C ABI; this module passes raw device
pointers (from torch tensors, which are used purely as an HBM allocator + stream provider) and sizes.
There is no CPU fallback: importing works anywhere (the .so links only the HIP runtime), but creating a
Context without a gfx950 device raises, and a missing libalpgpu.so raises at import.
"""
from __future__ import annotations

import ctypes as C
import os
from functools import partialmethod

import numpy as np
# torch ships its own libamdhip64.so (same SONAME as /opt/rocm's).  It MUST be loaded first so that
# libalpgpu.so binds to the same HIP runtime instance as the tensors/streams it is handed; two runtimes in
# one process do not see each other's streams (and the second one may not see the device at all).
import torch  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ALPGPU_LIB", os.path.join(HERE, "libalpgpu.so"))  # ALPGPU_LIB: A/B builds of the same ABI

VECTOR_SIZE = 1024
ROWGROUP_VECTORS = 100
SCHEME_ALP_RD = 1
SCHEME_ALP = 2

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950).  alp_amd has no CPU fallback.")

lib = C.CDLL(LIB_PATH)

# numpy mirrors of the two HBM record types (include/alpgpu.h)
ROWGROUP_DTYPE = np.dtype([
    ("scheme", np.uint8), ("k", np.uint8), ("combos", np.uint8, (10,)), ("rd_rbw", np.uint8), ("rd_lbw", np.uint8),
    ("rd_dict_size", np.uint8), ("pad", np.uint8), ("rd_dict", np.uint16, (8,)),
], align=False)
VECTOR_DTYPE = np.dtype([
    ("packed_off", np.uint64), ("exc_off", np.uint64), ("base", np.int64), ("bw", np.uint8), ("e", np.uint8),
    ("f", np.uint8), ("lbw", np.uint8), ("exc_cnt", np.uint16), ("scheme", np.uint16),
], align=False)
assert ROWGROUP_DTYPE.itemsize == 32 and VECTOR_DTYPE.itemsize == 32


class CColumn(C.Structure):
    _fields_ = [
        ("n_vectors", C.c_uint64), ("n_rowgroups", C.c_uint64), ("d_rowgroups", C.c_void_p), ("d_vectors", C.c_void_p),
        ("d_packed", C.c_void_p), ("packed_capacity", C.c_uint64), ("d_exc", C.c_void_p), ("exc_capacity", C.c_uint64),
        ("d_totals", C.c_void_p), ("packed_bytes_hint", C.c_uint64), ("exc_bytes_hint", C.c_uint64), ("d_rd_order", C.c_void_p), ("alp_rd_rowgroups_hint", C.c_uint64),
    ]


RD_ORDER_STRIDE = 296  # ALPGPU_RD_ORDER_STRIDE


def _sig(name, restype, *argtypes):
    f = getattr(lib, name)
    f.restype = restype
    f.argtypes = list(argtypes)
    return f


_vp, _u64, _sz, _int = C.c_void_p, C.c_uint64, C.c_size_t, C.c_int
_sig("alpgpu_abi_version", _int)
_sig("alpgpu_last_error", C.c_char_p)
_sig("alpgpu_ctx_create", _int, _int, C.POINTER(_vp))
_sig("alpgpu_ctx_destroy", None, _vp)
_sig("alpgpu_set_stream", _int, _vp, _vp)
_sig("alpgpu_synchronize", _int, _vp)
_sig("alpgpu_set_option", _int, _vp, _int, C.c_int64)
OPT_DECODE_VECTORS_PER_WG, OPT_DECODE_PLAIN_STORES, OPT_ENCODE_TWO_PASS, OPT_DEBUG_FORCE_STALL, OPT_CONSUMER_PIPELINED, OPT_ENCODE_ASYNC_INIT, OPT_ENCODE_KERNEL, OPT_DECODE_PAIRING = 1, 2, 3, 4, 5, 6, 7, 8
OPT_DECODE_PATCH_AFTER, OPT_ENCODE_UNORDERED, OPT_DECODE_RESIDENCY_PAD = 9, 10, 11
OPT_DECODE_READ_AHEAD, OPT_DECODE_READ_AHEAD_US, OPT_DECODE_SEGMENTS, OPT_DECODE_UNHINTED = 12, 13, 14, 15
ENCODE_KERNEL_LEAN, ENCODE_KERNEL_CLASSIC = 0, 1
_sig("alpgpu_device_info", _int, _vp, C.c_char_p, _sz, C.POINTER(_int), C.POINTER(_u64))
_sig("alpgpu_decode_vectors_per_wg", _int, _vp, C.POINTER(CColumn), _int)
_sig("alpgpu_decode_reads_ahead", _int, _vp, C.POINTER(CColumn), _int)
_sig("alpgpu_decode_runs", _int, _vp, C.POINTER(CColumn))
try:  # (round 6; an A/B library of an earlier round selected with ALPGPU_LIB does not have them)
    _sig("alpgpu_decode_runs_f32", _int, _vp, C.POINTER(CColumn))
    _sig("alpgpu_debug_read_ahead_batches", _int, _vp, C.POINTER(_u64))
    _sig("alpgpu_debug_unhinted_plan", _int, _vp, C.POINTER(_u64 * 6))
    _sig("alpgpu_debug_forget_column", _int, _vp, C.POINTER(CColumn))
    _sig("alpgpu_debug_decode_plan", _int, _vp, C.POINTER(CColumn), _int, C.POINTER(_u64 * 4))
except AttributeError:
    pass
_sig("alpgpu_debug_traffic_probe", _int, _vp, _vp, _vp, _u64, C.c_uint32)
try:
    _sig("alpgpu_debug_traffic_probe_with_search", _int, _vp, _vp, _vp, _u64, C.c_uint32, C.POINTER(CColumn))
except AttributeError:  # (an A/B library from before round 5, selected with ALPGPU_LIB: a measurement aid it does not have)
    pass
_sig("alpgpu_malloc_host", _int, _vp, C.POINTER(_vp), _sz)
for _t in ("f64", "f32"):
    _sig("alpgpu_compress_host_" + _t, _int, _vp, _vp, _u64, _vp, _u64, C.POINTER(_u64))
    _sig("alpgpu_decompress_host_" + _t, _int, _vp, _vp, _u64, _vp, _u64, C.POINTER(_u64))
for _t in ("f64", "f32"):
    _sig("alpgpu_compress_host_multi_" + _t, _int, C.POINTER(_vp), _int, _vp, _u64, _vp, _u64, C.POINTER(_u64))
    _sig("alpgpu_decompress_host_multi_" + _t, _int, C.POINTER(_vp), _int, _vp, _u64, _vp, _u64, C.POINTER(_u64))
_sig("alpgpu_free_host", _int, _vp, _vp)
_sig("alpgpu_memcpy_h2d_async", _int, _vp, _vp, _vp, _sz)
_sig("alpgpu_debug_decode_probe_f64", _int, _vp, C.POINTER(CColumn), _vp)
_sig("alpgpu_packed_capacity", _u64, _u64)
_sig("alpgpu_exc_capacity", _u64, _u64)
_sig("alpgpu_use_own_stream", _int, _vp)
_sig("alpgpu_decode_f64", _int, _vp, C.POINTER(CColumn), _vp)
_sig("alpgpu_decode_sum_f64", _int, _vp, C.POINTER(CColumn), _vp)
_sig("alpgpu_decode_count_range_f64", _int, _vp, C.POINTER(CColumn), C.c_double, C.c_double, _vp)
_sig("alpgpu_column_sum_f64", _int, _vp, C.POINTER(CColumn), _vp)
_sig("alpgpu_column_sum_f32", _int, _vp, C.POINTER(CColumn), _vp)
_sig("alpgpu_tree_sum_f64", _int, _vp, _vp, _u64, _vp)
_sig("alpgpu_gather_f64", _int, _vp, C.POINTER(CColumn), _vp, _u64, _vp)
_sig("alpgpu_gather_f32", _int, _vp, C.POINTER(CColumn), _vp, _u64, _vp)
_sig("alpgpu_decode_slice_f64", _int, _vp, C.POINTER(CColumn), _u64, _u64, _vp)
_sig("alpgpu_decode_slice_f32", _int, _vp, C.POINTER(CColumn), _u64, _u64, _vp)
_sig("alpgpu_select_scratch_bytes", _u64, _u64)
_sig("alpgpu_select_range_f64", _int, _vp, C.POINTER(CColumn), _u64, _u64, C.c_double, C.c_double, _vp, _vp, _u64, _vp, _vp)
_sig("alpgpu_select_range_f32", _int, _vp, C.POINTER(CColumn), _u64, _u64, C.c_float, C.c_float, _vp, _vp, _u64, _vp, _vp)
_sig("alpgpu_debug_select_scan", _int, _vp, _vp, _u64, _vp, _vp, _vp)
for _t, _ft in (("f64", C.c_double), ("f32", C.c_float)):
    _sig("alpgpu_zone_map_" + _t, _int, _vp, C.POINTER(CColumn), _vp)
    _sig("alpgpu_zone_map_of_values_" + _t, _int, _vp, _vp, _u64, _vp)
    _sig("alpgpu_zones_minmax_" + _t, _int, _vp, _vp, _u64, _vp)
    _sig("alpgpu_select_range_zoned_" + _t, _int, _vp, C.POINTER(CColumn), _vp, _u64, _u64, _ft, _ft, _vp, _vp, _u64, _vp, _vp)
MASK_SET, MASK_AND, MASK_OR = 0, 1, 2  # ALPGPU_MASK_*
for _t, _ft in (("f64", C.c_double), ("f32", C.c_float)):
    _sig("alpgpu_select_mask_" + _t, _int, _vp, C.POINTER(CColumn), _u64, _u64, _ft, _ft, _int, _vp)
    _sig("alpgpu_decode_sum_masked_" + _t, _int, _vp, C.POINTER(CColumn), _vp, _vp, _vp)
    _sig("alpgpu_decode_masked_" + _t, _int, _vp, C.POINTER(CColumn), _vp, _vp, _vp, _u64, _vp, _vp)
_sig("alpgpu_mask_to_indices", _int, _vp, _vp, _u64, _vp, _u64, _vp, _vp)
CMP_LT, CMP_LE, CMP_GT, CMP_GE, CMP_EQ, CMP_NE = 0, 1, 2, 3, 4, 5  # ALPGPU_CMP_*
for _t in ("f64", "f32"):
    _sig("alpgpu_compare_mask_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _u64, _u64, _int, _int, _vp)
    _sig("alpgpu_decode_dot_masked_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp)
GROUP_MAX = 16  # ALPGPU_GROUP_MAX
for _t in ("f64", "f32"):
    _sig("alpgpu_decode_group_sum_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _vp, _vp)
_sig("alpgpu_group_totals_scratch_bytes", C.c_size_t, _u64, C.c_uint32)
_sig("alpgpu_group_totals", _int, _vp, _vp, _vp, _u64, C.c_uint32, _vp, _vp, _vp)
for _t in ("f64", "f32"):
    _sig("alpgpu_decode_minmax_masked_" + _t, _int, _vp, C.POINTER(CColumn), _vp, _vp, _vp)
    _sig("alpgpu_decode_group_minmax_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _vp, _vp)
    _sig("alpgpu_group_minmax_totals_" + _t, _int, _vp, _vp, _u64, C.c_uint32, _vp)
for _t in ("f64", "f32"):
    _sig("alpgpu_select_in_mask_" + _t, _int, _vp, C.POINTER(CColumn), _u64, _u64, _vp, _u64, _int, _vp, _int, _vp)
_sig("alpgpu_in_list_lds_max", C.c_size_t, _int)
TOP_K_MAX = 1024  # ALPGPU_TOP_K_MAX
_sig("alpgpu_top_k_scratch_bytes", _u64, _u64, _u64)
for _t in ("f64", "f32"):
    _sig("alpgpu_top_k_" + _t, _int, _vp, C.POINTER(CColumn), _vp, _vp, _u64, _int, _vp, _vp, _vp, _vp)
RANK_MAX, QUANTILE_MAX = 32, 16  # ALPGPU_RANK_MAX, ALPGPU_QUANTILE_MAX


class QuantileTuning(C.Structure):  # alpgpu_quantile_tuning
    _fields_ = [("capacity", C.c_uint64), ("max_workgroups", C.c_uint32), ("flush_every", C.c_uint32)]


class QuantileTrace(C.Structure):  # alpgpu_quantile_trace
    _fields_ = [("compact_pass", C.c_uint32), ("wide_grid", C.c_uint32), ("waves_per_wg", C.c_uint32), ("reserved", C.c_uint32), ("candidates", C.c_uint64), ("n", C.c_uint64),
                ("zero_skips", C.c_uint64), ("zone_skips", C.c_uint64 * 8)]


_sig("alpgpu_quantile_scratch_bytes", _u64, _u64)
for _t in ("f64", "f32"):
    _sig("alpgpu_select_rank_" + _t, _int, _vp, C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _int, _vp, _vp, _vp)
    _sig("alpgpu_quantile_" + _t, _int, _vp, C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp)
    _sig("alpgpu_debug_quantile_" + _t, _int, _vp, C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _int, _vp, _vp, _vp, C.POINTER(QuantileTuning))
_sig("alpgpu_debug_quantile_trace", _int, _vp, _vp, C.POINTER(QuantileTrace))
JOIN_NO_MATCH = -1  # ALPGPU_JOIN_NO_MATCH
for _t in ("f64", "f32"):
    _sig("alpgpu_join_probe_" + _t, _int, _vp, C.POINTER(CColumn), _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _vp, _vp)
HISTOGRAM_EDGES_MAX = 4095  # ALPGPU_HISTOGRAM_EDGES_MAX


class HistogramTuning(C.Structure):  # alpgpu_histogram_tuning
    _fields_ = [("grid", C.c_uint32), ("flush_every", C.c_uint32)]


for _t in ("f64", "f32"):
    _sig("alpgpu_histogram_" + _t, _int, _vp, C.POINTER(CColumn), _u64, _u64, _vp, _vp, _vp, C.c_uint32, _int, _int, _vp)
    _sig("alpgpu_debug_histogram_" + _t, _int, _vp, C.POINTER(CColumn), _u64, _u64, _vp, _vp, _vp, C.c_uint32, _int, _int, _vp, C.POINTER(HistogramTuning), _vp)
DISTINCT_MAX = 1 << 20  # ALPGPU_DISTINCT_MAX


class DistinctTuning(C.Structure):  # alpgpu_distinct_tuning
    _fields_ = [("grid", C.c_uint32), ("flush_every", C.c_uint32), ("lds_slots", C.c_uint32), ("table_slots", C.c_uint32), ("sort_tile", C.c_uint32), ("reserved", C.c_uint32)]


_sig("alpgpu_distinct_scratch_bytes", _u64, _u64)
for _t in ("f64", "f32"):
    _sig("alpgpu_distinct_" + _t, _int, _vp, C.POINTER(CColumn), _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp)
    _sig("alpgpu_debug_distinct_" + _t, _int, _vp, C.POINTER(CColumn), _u64, _u64, _vp, _vp, _u64, _vp, _vp, _vp, _vp, C.POINTER(DistinctTuning), _vp)
KEYED_KEYS_MAX, KEYED_STRIPES_MAX = 1024, 4096  # ALPGPU_KEYED_KEYS_MAX, ALPGPU_KEYED_STRIPES_MAX


class KeyedTuning(C.Structure):  # alpgpu_keyed_tuning
    _fields_ = [("grid", C.c_uint32), ("reserved", C.c_uint32)]


_sig("alpgpu_keyed_stripe_vectors", _u64, _u64)
_sig("alpgpu_keyed_sum_scratch_bytes", _u64, _u64, C.c_uint32)
for _t in ("f64",):  # (double columns only: the float entry points are not built yet, include/alpgpu.h says why)
    _sig("alpgpu_decode_keyed_sum_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp)
    _sig("alpgpu_debug_decode_keyed_sum_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, C.POINTER(KeyedTuning), _vp)
for _t in ("f64", "f32"):  # keyed MIN / MAX: both precisions, no scratch
    _sig("alpgpu_decode_keyed_minmax_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _vp, _vp)
    _sig("alpgpu_debug_decode_keyed_minmax_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _vp, _vp, C.POINTER(KeyedTuning), _vp)
KEYED_MANY_KEYS_MAX = 1 << 20  # ALPGPU_KEYED_MANY_KEYS_MAX == ALPGPU_DISTINCT_MAX
BUCKET_EDGES_MAX = 1023  # ALPGPU_BUCKET_EDGES_MAX: n_edges + 1 buckets <= KEYED_KEYS_MAX table entries
for _t in ("f64", "f32"):  # keyed MIN / MAX beyond KEYED_KEYS_MAX keys: the table in device memory
    _sig("alpgpu_decode_keyed_minmax_many_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _vp, _vp)
    _sig("alpgpu_debug_decode_keyed_minmax_many_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _vp, _vp, C.POINTER(KeyedTuning), _vp)
KEYED_EXACT_VECTORS_MAX = 1 << 21  # ALPGPU_KEYED_EXACT_VECTORS_MAX: 2^31 rows, what a limb of the exact sums' table holds
_sig("alpgpu_keyed_exact_sum_table_bytes", _u64, C.c_uint32)
for _t in ("f64", "f32"):  # the exact keyed SUM: (ctx, val, key, mask, zones, keys, n_keys, sums, counts, table, accumulate)
    _sig("alpgpu_decode_keyed_exact_sum_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _int)
    _sig("alpgpu_debug_decode_keyed_exact_sum_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _int, C.POINTER(KeyedTuning), _vp)
_sig("alpgpu_bucket_sum_scratch_bytes", _u64, _u64, C.c_uint32)
for _t in ("f64", "f32"):  # bucketed aggregation: the key column's buckets by sorted edges; (ctx, val, key, mask, zones, edges, n_edges, right, ...)
    _sig("alpgpu_decode_bucket_sum_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _int, _vp, _vp, _vp)
    _sig("alpgpu_debug_decode_bucket_sum_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _int, _vp, _vp, _vp, C.POINTER(KeyedTuning), _vp)
    _sig("alpgpu_decode_bucket_minmax_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _int, _vp, _vp)
    _sig("alpgpu_debug_decode_bucket_minmax_" + _t, _int, _vp, C.POINTER(CColumn), C.POINTER(CColumn), _vp, _vp, _vp, C.c_uint32, _int, _vp, _vp, C.POINTER(KeyedTuning), _vp)
_sig("alpgpu_column_validate", _int, _vp, C.POINTER(CColumn), _int, C.POINTER(_u64))
_sig("alpgpu_rowgroup_init_f64", _int, _vp, _vp, _u64, C.POINTER(CColumn))
_sig("alpgpu_encode_vectors_f64", _int, _vp, _vp, _u64, C.POINTER(CColumn))
_sig("alpgpu_encode_f64", _int, _vp, _vp, _u64, C.POINTER(CColumn))
_sig("alpgpu_column_totals", _int, _vp, C.POINTER(CColumn), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_int))
_sig("alpgpu_pad_tail_f64", _int, _vp, _vp, _u64)
_sig("alpgpu_blob_size", _u64, _u64, _u64, _u64)
_sig("alpgpu_column_to_blob", _int, _vp, C.POINTER(CColumn), _u64, _vp, _u64, C.POINTER(_u64))
_sig("alpgpu_column_from_blob", _int, _vp, _vp, _u64, C.POINTER(CColumn), C.POINTER(_u64))
_sig("alpgpu_ffor_i64", _int, _vp, _vp, _vp, _sz, _vp, _vp, _u64)
_sig("alpgpu_unffor_i64", _int, _vp, _vp, _sz, _vp, _vp, _vp, _u64)
_sig("alpgpu_ffor_u16", _int, _vp, _vp, _vp, _sz, _vp, _vp, _u64)
_sig("alpgpu_unffor_u16", _int, _vp, _vp, _sz, _vp, _vp, _vp, _u64)
_sig("alpgpu_ffor_u8", _int, _vp, _vp, _vp, _sz, _vp, _vp, _u64)
_sig("alpgpu_unffor_u8", _int, _vp, _vp, _sz, _vp, _vp, _vp, _u64)
_sig("alpgpu_falp_f64", _int, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _u64)
_sig("alpgpu_decode_values_f64", _int, _vp, _vp, _vp, _vp, _vp, _u64)
_sig("alpgpu_patch_f64", _int, _vp, _vp, _vp, _vp, _sz, _vp, _u64)
_sig("alpgpu_encode_simdized_f64", _int, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _u64)
_sig("alpgpu_encode_values_f64", _int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _u64)
_sig("alpgpu_analyze_ffor_i64", _int, _vp, _vp, _vp, _vp, _u64)
_sig("alpgpu_encode_value_f64", _int, _vp, _vp, _vp, C.c_uint8, C.c_uint8, _int, _u64)
_sig("alpgpu_encode_value_f32", _int, _vp, _vp, _vp, C.c_uint8, C.c_uint8, _int, _u64)
_sig("alpgpu_rd_encode_vectors_f64", _int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _u64)
_sig("alpgpu_rd_decode_vectors_f64", _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _u64)
# single precision (same argument shapes; 32-bit words)
_sig("alpgpu_packed_capacity_f32", _u64, _u64)
_sig("alpgpu_exc_capacity_f32", _u64, _u64)
_sig("alpgpu_decode_f32", _int, _vp, C.POINTER(CColumn), _vp)
_sig("alpgpu_decode_sum_f32", _int, _vp, C.POINTER(CColumn), _vp)
_sig("alpgpu_decode_count_range_f32", _int, _vp, C.POINTER(CColumn), C.c_float, C.c_float, _vp)
_sig("alpgpu_rowgroup_init_f32", _int, _vp, _vp, _u64, C.POINTER(CColumn))
_sig("alpgpu_encode_vectors_f32", _int, _vp, _vp, _u64, C.POINTER(CColumn))
_sig("alpgpu_encode_f32", _int, _vp, _vp, _u64, C.POINTER(CColumn))
_sig("alpgpu_state_from_samples_f32", _int, _vp, _vp, C.c_uint32, _vp)
_sig("alpgpu_rd_state_from_samples_f32", _int, _vp, _vp, C.c_uint32, _vp)
_sig("alpgpu_state_from_samples_f64", _int, _vp, _vp, C.c_uint32, _vp)
_sig("alpgpu_rd_state_from_samples_f64", _int, _vp, _vp, C.c_uint32, _vp)
_sig("alpgpu_rd_dictionary_for_cut_f64", _int, _vp, _vp, C.c_uint32, C.c_uint8, _vp, _vp)
_sig("alpgpu_rd_dictionary_for_cut_f32", _int, _vp, _vp, C.c_uint32, C.c_uint8, _vp, _vp)
_sig("alpgpu_pad_tail_f32", _int, _vp, _vp, _u64)
_sig("alpgpu_column_to_blob_f32", _int, _vp, C.POINTER(CColumn), _u64, _vp, _u64, C.POINTER(_u64))
_sig("alpgpu_column_from_blob_f32", _int, _vp, _vp, _u64, C.POINTER(CColumn), C.POINTER(_u64))
_sig("alpgpu_ffor_i32", _int, _vp, _vp, _vp, _sz, _vp, _vp, _u64)
_sig("alpgpu_unffor_i32", _int, _vp, _vp, _sz, _vp, _vp, _vp, _u64)
_sig("alpgpu_falp_f32", _int, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _u64)
_sig("alpgpu_decode_values_f32", _int, _vp, _vp, _vp, _vp, _vp, _u64)
_sig("alpgpu_patch_f32", _int, _vp, _vp, _vp, _vp, _sz, _vp, _u64)
_sig("alpgpu_encode_simdized_f32", _int, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _u64)
_sig("alpgpu_encode_values_f32", _int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _u64)
_sig("alpgpu_analyze_ffor_i32", _int, _vp, _vp, _vp, _vp, _u64)
_sig("alpgpu_rd_encode_vectors_f32", _int, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _u64)
_sig("alpgpu_rd_decode_vectors_f32", _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _u64)


class AlpGpuError(RuntimeError):
    pass


def _check(rc: int, what: str):
    if rc != 0:
        raise AlpGpuError(f"{what} failed ({rc}): {lib.alpgpu_last_error().decode()}")


_TORCH_TYPE = {"f64": torch.float64, "f32": torch.float32}  # a column's dtype -> its value type
_NUMPY_TYPE = {"f64": np.float64, "f32": np.float32}


def _ptr(t):
    """an optional argument's address: NULL for None and for a tensor without elements (whose data_ptr() is 0 already)"""
    return _vp(t.data_ptr()) if t is not None and t.numel() else None


class Context:
    """One per device / process.  With use_torch_stream (default) every call is enqueued on torch's CURRENT stream of the
    device at the time of the call (so `with torch.cuda.stream(s):` works as for torch's own ops); set_stream() pins a
    stream instead."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        h = _vp()
        _check(lib.alpgpu_ctx_create(device, C.byref(h)), "alpgpu_ctx_create")
        self._h = h
        self.device = device
        self._follow_torch = bool(use_torch_stream)
        self._last_stream = None

    @property
    def h(self):
        """the context handle; re-points the context at torch's current stream first when it follows torch"""
        if self._follow_torch and self._h:
            cur = torch.cuda.current_stream(self.device).cuda_stream
            if cur != self._last_stream:
                _check(lib.alpgpu_set_stream(self._h, _vp(cur)), "alpgpu_set_stream")
                self._last_stream = cur
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            lib.alpgpu_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle: int):
        """pin the context to this hipStream_t handle (it stops following torch's current stream)"""
        self._follow_torch = False
        _check(lib.alpgpu_set_stream(self._h, _vp(stream_handle)), "alpgpu_set_stream")

    def set_option(self, option: int, value: int):
        _check(lib.alpgpu_set_option(self.h, option, value), "alpgpu_set_option")

    def synchronize(self):
        _check(lib.alpgpu_synchronize(self.h), "alpgpu_synchronize")

    def compress_host(self, x_host, blob_host=None):
        """host tensor (CPU, float64 / float32, any length; page-locked for speed) -> uint8 CPU tensor holding the serialized column
        (include/alpgpu.h: alpgpu_compress_host_*).  blob_host: a CPU uint8 tensor to write into (e.g. page-locked), else one is made."""
        t = self._sfx(x_host)
        n = (x_host.numel() + VECTOR_SIZE - 1) // VECTOR_SIZE
        if blob_host is None:
            cap = int(lib.alpgpu_blob_size(n, lib.alpgpu_packed_capacity(n), lib.alpgpu_exc_capacity(n)))
            blob_host = torch.empty(cap, dtype=torch.uint8)
        w = _u64()
        _check(getattr(lib, "alpgpu_compress_host_" + t)(self.h, _vp(x_host.data_ptr()), x_host.numel(), _vp(blob_host.data_ptr()), blob_host.numel(), C.byref(w)),
               "alpgpu_compress_host_" + t)
        return blob_host[: w.value]

    def decompress_host(self, blob_host, out_host):
        """serialized column (CPU uint8 tensor) -> out_host (CPU tensor of the column's type, at least as long as the column); returns the value count"""
        t = self._sfx(out_host)
        nv = _u64()
        _check(getattr(lib, "alpgpu_decompress_host_" + t)(self.h, _vp(blob_host.data_ptr()), blob_host.numel(), _vp(out_host.data_ptr()), out_host.numel(), C.byref(nv)),
               "alpgpu_decompress_host_" + t)
        return int(nv.value)

    @staticmethod
    def compress_host_multi(ctxs, x_host, blob_host=None):
        """alpgpu_compress_host_multi_*: the host column cut into whole-rowgroup shards over the contexts (one per GPU, normally), one blob"""
        t = "f64" if x_host.dtype == torch.float64 else "f32"
        n = (x_host.numel() + 1023) // 1024
        if blob_host is None:
            cap = int(lib.alpgpu_blob_size(n, getattr(lib, "alpgpu_packed_capacity" + ("" if t == "f64" else "_f32"))(n), getattr(lib, "alpgpu_exc_capacity" + ("" if t == "f64" else "_f32"))(n)))
            blob_host = torch.empty(cap, dtype=torch.uint8)
        arr = (_vp * len(ctxs))(*[c.h for c in ctxs])
        w = _u64()
        _check(getattr(lib, "alpgpu_compress_host_multi_" + t)(arr, len(ctxs), _vp(x_host.data_ptr()), x_host.numel(), _vp(blob_host.data_ptr()), blob_host.numel(), C.byref(w)),
               "alpgpu_compress_host_multi_" + t)
        return blob_host[: w.value]

    @staticmethod
    def decompress_host_multi(ctxs, blob_host, out_host):
        t = "f64" if out_host.dtype == torch.float64 else "f32"
        arr = (_vp * len(ctxs))(*[c.h for c in ctxs])
        nv = _u64()
        _check(getattr(lib, "alpgpu_decompress_host_multi_" + t)(arr, len(ctxs), _vp(blob_host.data_ptr()), blob_host.numel(), _vp(out_host.data_ptr()), out_host.numel(), C.byref(nv)),
               "alpgpu_decompress_host_multi_" + t)
        return nv.value

    def decode_probe(self, col: "DeviceColumn", out):
        """decode_sum without the unpack arithmetic (include/alpgpu.h: alpgpu_debug_decode_probe_f64)"""
        _check(lib.alpgpu_debug_decode_probe_f64(self.h, C.byref(col.c), _vp(out.data_ptr())), "alpgpu_debug_decode_probe_f64")

    def traffic_probe(self, x, out, n_vectors: int, write_bytes_per_vector: int):
        """the single-pass encode's loads and stores without its arithmetic (include/alpgpu.h: alpgpu_debug_traffic_probe)"""
        _check(lib.alpgpu_debug_traffic_probe(self.h, _vp(x.data_ptr()), _vp(out.data_ptr()), n_vectors, write_bytes_per_vector), "alpgpu_debug_traffic_probe")

    def traffic_probe_with_search(self, x, out, n_vectors: int, write_bytes_per_vector: int, scratch: "DeviceColumn"):
        """the same probe with the encode's rowgroup search (over x, a double column) running beside it as beside alpgpu_encode_f64"""
        _check(lib.alpgpu_debug_traffic_probe_with_search(self.h, _vp(x.data_ptr()), _vp(out.data_ptr()), n_vectors, write_bytes_per_vector, C.byref(scratch.c)),
               "alpgpu_debug_traffic_probe_with_search")

    def decode_vectors_per_wg(self, col: "DeviceColumn") -> int:
        """the launch shape decode() would use for this column now (vectors per decode workgroup)"""
        return int(lib.alpgpu_decode_vectors_per_wg(self.h, C.byref(col.c), 1 if col.dtype == "f32" else 0))

    def decode_runs(self, col: "DeviceColumn") -> int:
        """launches decode() of this column would make now: 1, or the runs of regions of different kinds (OPT_DECODE_SEGMENTS; after column_totals / from_blob)"""
        return int((lib.alpgpu_decode_runs_f32 if col.dtype == "f32" else lib.alpgpu_decode_runs)(self.h, C.byref(col.c)))

    def read_ahead_batches(self) -> int:
        """batches of 64 vectors this context's read-aheads have read since it was created (debug counter; waits for the streams)"""
        n = _u64()
        _check(lib.alpgpu_debug_read_ahead_batches(self.h, C.byref(n)), "alpgpu_debug_read_ahead_batches")
        return n.value

    def forget(self, col: "DeviceColumn"):
        """what the context remembers about this column (segments, learned sizes) is dropped, as an encode into it would"""
        _check(lib.alpgpu_debug_forget_column(self.h, C.byref(col.c)), "alpgpu_debug_forget_column")

    def unhinted_plan(self) -> dict:
        """the device-side plan of this context's last unhinted decode (include/alpgpu.h: alpgpu_debug_unhinted_plan)"""
        w = (_u64 * 6)()
        _check(lib.alpgpu_debug_unhinted_plan(self.h, C.byref(w)), "alpgpu_debug_unhinted_plan")
        return {"shape": int(w[0]), "lead_min": int(w[1] & 0xFFFFFFFF), "lead_max": int(w[1] >> 32), "ps_per_vector": int(w[2] & 0xFFFFFFFF), "max_bits": int(w[2] >> 32),
                "packed_bytes": int(w[3]), "exceptions": int(w[4]), "rd_vectors": int(w[5])}

    def decode_plan(self, col: "DeviceColumn"):
        """the launch decode() of this column would make now, as a whole (include/alpgpu.h: alpgpu_debug_decode_plan): None for an unhinted decode planned on the device,
        else {"word", "vectors_per_wg", "many_exc", "pad_kib", "packed_bytes", "exc_bytes", "rd_rowgroups_hint"} (float: vectors_per_wg is the shape, pad_kib None = none)"""
        w = (_u64 * 4)()
        rc = int(lib.alpgpu_debug_decode_plan(self.h, C.byref(col.c), 1 if col.dtype == "f32" else 0, C.byref(w)))
        if rc < 0:
            _check(rc, "alpgpu_debug_decode_plan")
        if rc == 0:
            return None
        word = int(w[0])
        if col.dtype == "f32":
            vpw, many, pad = word & 0xFF, False, (None if (word >> 8) == 0xFF else word >> 8)
        else:
            vpw, many, pad = (1 if word & 1 else 2), bool(word & 64), word >> 8
        return {"word": word, "vectors_per_wg": vpw, "many_exc": many, "pad_kib": pad, "packed_bytes": int(w[1]), "exc_bytes": int(w[2]), "rd_rowgroups_hint": int(w[3])}

    def decode_reads_ahead(self, col: "DeviceColumn") -> bool:
        """decode() of this column would start the read-ahead beside the decode kernel (OPT_DECODE_READ_AHEAD)"""
        return int(lib.alpgpu_decode_reads_ahead(self.h, C.byref(col.c), 1 if col.dtype == "f32" else 0)) == 1

    def device_info(self) -> dict:
        name = C.create_string_buffer(128)
        cus, hbm = _int(), _u64()
        _check(lib.alpgpu_device_info(self.h, name, 128, C.byref(cus), C.byref(hbm)), "alpgpu_device_info")
        return {"name": name.value.decode(), "cu_count": cus.value, "hbm_bytes": hbm.value}

    # ---- whole-column path ------------------------------------------------------------------------
    # Every whole-column call dispatches on the value type: float64 tensors / DeviceColumn(dtype="f64") -> *_f64 entry
    # points, float32 / "f32" -> *_f32.
    @staticmethod
    def _sfx(x):
        assert x.dtype in (torch.float64, torch.float32)
        return "f64" if x.dtype == torch.float64 else "f32"

    def _check_input(self, x, col):
        assert x.is_contiguous() and x.is_cuda and self._sfx(x) == col.dtype, "input tensor and column must have the same value type"
        assert x.numel() == col.n_vectors * VECTOR_SIZE, "input must hold exactly n_vectors * 1024 values"

    def _call(self, stem, sfx, *args):
        name = f"alpgpu_{stem}_{sfx}"
        _check(getattr(lib, name)(self.h, *args), name)

    def rowgroup_init(self, x, col: "DeviceColumn"):
        self._check_input(x, col)
        self._call("rowgroup_init", col.dtype, _vp(x.data_ptr()), col.n_vectors, C.byref(col.c))

    def encode_vectors(self, x, col: "DeviceColumn"):
        self._check_input(x, col)
        self._call("encode_vectors", col.dtype, _vp(x.data_ptr()), col.n_vectors, C.byref(col.c))

    def encode(self, x, col: "DeviceColumn" = None):
        """rowgroup init + vector encode of a device tensor of n_vectors*1024 doubles (or floats)"""
        if col is None:
            col = DeviceColumn(x.numel() // VECTOR_SIZE, self.device, dtype=self._sfx(x))
        self._check_input(x, col)
        self._call("encode", col.dtype, _vp(x.data_ptr()), col.n_vectors, C.byref(col.c))
        return col

    def state_from_samples(self, samples, state, rd_only: bool = False):
        """samples: device tensor of 1..288 first-level samples; state: 32-byte uint8 device tensor"""
        self._call("rd_state_from_samples" if rd_only else "state_from_samples", self._sfx(samples), _vp(samples.data_ptr()), samples.numel(),
                   _vp(state.data_ptr()))

    def rd_dictionary_for_cut(self, samples, right_bit_width: int, state, estimate):
        """rd_encoder::build_left_parts_dictionary for one cut: state (32-byte uint8 device tensor) and estimate (1 float64, device) are written"""
        self._call("rd_dictionary_for_cut", self._sfx(samples), _vp(samples.data_ptr()), samples.numel(), right_bit_width, _vp(state.data_ptr()), _vp(estimate.data_ptr()))

    # ---- tail padding + serialized container ------------------------------------------------------
    def pad_tail(self, x, n_values: int):
        """x: device tensor with room for ceil(n_values/1024)*1024 doubles; fills the incomplete last vector"""
        assert x.numel() >= (n_values + 1023) // 1024 * 1024
        self._call("pad_tail", self._sfx(x), _vp(x.data_ptr()), n_values)

    def to_blob(self, col: "DeviceColumn", n_values: int) -> np.ndarray:
        pb, eb, ov = self.column_totals(col)
        size = int(lib.alpgpu_blob_size(col.n_vectors, pb, eb))
        blob = np.zeros(size, np.uint8)
        w = _u64()
        fn = lib.alpgpu_column_to_blob if col.dtype == "f64" else lib.alpgpu_column_to_blob_f32
        _check(fn(self.h, C.byref(col.c), n_values, blob.ctypes.data_as(_vp), size, C.byref(w)), "alpgpu_column_to_blob")
        assert w.value == size
        return blob

    def from_blob(self, blob: np.ndarray):
        """-> (DeviceColumn, n_values); raises AlpGpuError on a malformed blob"""
        if blob.size < 64:
            raise AlpGpuError("blob shorter than its 64-byte header")
        hdr = np.frombuffer(blob[:64].tobytes(), dtype=np.uint64)
        n_vectors, packed_bytes, exc_bytes = int(hdr[3]), int(hdr[5]), int(hdr[6])
        if n_vectors > (1 << 40) or packed_bytes > (1 << 50) or exc_bytes > (1 << 50):
            raise AlpGpuError("blob header is implausible")
        dtype = "f32" if int(hdr[7]) == 4 else "f64"
        col = DeviceColumn(n_vectors, self.device, packed_capacity=packed_bytes + 1024, exc_capacity=exc_bytes + 64, dtype=dtype)
        nv = _u64()
        fn = lib.alpgpu_column_from_blob if dtype == "f64" else lib.alpgpu_column_from_blob_f32
        _check(fn(self.h, blob.ctypes.data_as(_vp), blob.size, C.byref(col.c), C.byref(nv)), "alpgpu_column_from_blob")
        return col, nv.value

    def column_totals(self, col: "DeviceColumn"):
        pb, eb, ov = _u64(), _u64(), _int()
        _check(lib.alpgpu_column_totals(self.h, C.byref(col.c), C.byref(pb), C.byref(eb), C.byref(ov)), "alpgpu_column_totals")
        return pb.value, eb.value, ov.value

    # ---- batch primitives (torch tensors on this device; shapes [n, 1024] unless noted) ---------------
    # One body per primitive takes the entry point's suffix; the public names are the double codec's (i64 / f64 words), its ALP_RD streams'
    # (u16 / u8) and, with _i32 / _f32, the float codec's (32-bit words, the same argument shapes).
    def _ffor(self, sfx, vals, packed, bw, base):
        self._call("ffor", sfx, _ptr(vals), _ptr(packed), packed.shape[1], _ptr(bw), _ptr(base), vals.shape[0])

    def _unffor(self, sfx, packed, out, bw, base):
        self._call("unffor", sfx, _ptr(packed), packed.shape[1], _ptr(out), _ptr(bw), _ptr(base), out.shape[0])

    def _falp(self, sfx, packed, out, bw, base, fac, exp):
        self._call("falp", sfx, _ptr(packed), packed.shape[1], _ptr(out), _ptr(bw), _ptr(base), _ptr(fac), _ptr(exp), out.shape[0])

    def _decode_values(self, sfx, enc, out, fac, exp):
        self._call("decode_values", sfx, _ptr(enc), _ptr(out), _ptr(fac), _ptr(exp), out.shape[0])

    def _patch(self, sfx, out, exc, pos, cnt):
        self._call("patch", sfx, _ptr(out), _ptr(exc), _ptr(pos), exc.shape[1], _ptr(cnt), out.shape[0])

    def _encode_simdized(self, sfx, x, exc, pos, cnt, enc, fac, exp):
        self._call("encode_simdized", sfx, _ptr(x), _ptr(exc), _ptr(pos), exc.shape[1], _ptr(cnt), _ptr(enc), _ptr(fac), _ptr(exp), x.shape[0])

    def _encode_values(self, sfx, x, states, state_idx, exc, pos, cnt, enc, fac, exp):
        self._call("encode_values", sfx, _ptr(x), _ptr(states), _ptr(state_idx), _ptr(exc), _ptr(pos), exc.shape[1], _ptr(cnt), _ptr(enc), _ptr(fac), _ptr(exp),
                   x.shape[0])

    def _analyze_ffor(self, sfx, enc, bw, base):
        self._call("analyze_ffor", sfx, _ptr(enc), _ptr(bw), _ptr(base), enc.shape[0])

    def _rd_encode_vectors(self, sfx, x, states, state_idx, exc, pos, cnt, right, left):
        self._call("rd_encode_vectors", sfx, _ptr(x), _ptr(states), _ptr(state_idx), _ptr(exc), _ptr(pos), exc.shape[1], _ptr(cnt), _ptr(right), _ptr(left),
                   x.shape[0])

    def _rd_decode_vectors(self, sfx, out, right, left, states, state_idx, exc, pos, cnt):
        self._call("rd_decode_vectors", sfx, _ptr(out), _ptr(right), _ptr(left), _ptr(states), _ptr(state_idx), _ptr(exc), _ptr(pos), exc.shape[1], _ptr(cnt),
                   out.shape[0])

    ffor_i64, ffor_i32 = partialmethod(_ffor, "i64"), partialmethod(_ffor, "i32")
    unffor_i64, unffor_i32 = partialmethod(_unffor, "i64"), partialmethod(_unffor, "i32")
    falp, falp_f32 = partialmethod(_falp, "f64"), partialmethod(_falp, "f32")
    decode_values, decode_values_f32 = partialmethod(_decode_values, "f64"), partialmethod(_decode_values, "f32")
    patch, patch_f32 = partialmethod(_patch, "f64"), partialmethod(_patch, "f32")
    encode_simdized, encode_simdized_f32 = partialmethod(_encode_simdized, "f64"), partialmethod(_encode_simdized, "f32")
    encode_values, encode_values_f32 = partialmethod(_encode_values, "f64"), partialmethod(_encode_values, "f32")
    analyze_ffor, analyze_ffor_i32 = partialmethod(_analyze_ffor, "i64"), partialmethod(_analyze_ffor, "i32")
    rd_encode_vectors, rd_encode_vectors_f32 = partialmethod(_rd_encode_vectors, "f64"), partialmethod(_rd_encode_vectors, "f32")
    rd_decode_vectors, rd_decode_vectors_f32 = partialmethod(_rd_decode_vectors, "f64"), partialmethod(_rd_decode_vectors, "f32")

    def ffor_u16(self, vals, packed, bw, base=None):  # (the ALP_RD streams pack without a base)
        self._ffor("u16", vals, packed, bw, base)

    def unffor_u16(self, packed, out, bw, base=None):
        self._unffor("u16", packed, out, bw, base)

    def ffor_u8(self, vals, packed, bw, base=None):
        self._ffor("u8", vals, packed, bw, base)

    def unffor_u8(self, packed, out, bw, base=None):
        self._unffor("u8", packed, out, bw, base)

    def encode_value(self, x, fac: int, exp: int, safe: bool = True):
        """alpgpu_encode_value_f64 / _f32 on a 1-d device tensor: the encoded integers (int64 / int32)"""
        f64 = x.dtype == torch.float64
        out = torch.empty(x.numel(), dtype=torch.int64 if f64 else torch.int32, device=x.device)
        self._call("encode_value", "f64" if f64 else "f32", _ptr(x), _ptr(out), fac, exp, 1 if safe else 0, x.numel())
        return out

    def decode_count_range(self, col: "DeviceColumn", lo: float, hi: float, out=None):
        """per-vector count of decoded values in [lo, hi] without materialising them (alpgpu_decode_count_range_f64 / _f32)"""
        if out is None:
            out = torch.empty(col.n_vectors, dtype=torch.int32, device=f"cuda:{self.device}")
        self._call("decode_count_range", col.dtype, C.byref(col.c), lo, hi, _vp(out.data_ptr()))
        return out

    def column_sum(self, col: "DeviceColumn", out=None):
        """the whole column's total in the documented tree order (alpgpu_column_sum_f64 / _f32): a 1-element float64 tensor"""
        if out is None:
            out = torch.empty(1, dtype=torch.float64, device=col.vectors.device)
        self._call("column_sum", col.dtype, C.byref(col.c), _vp(out.data_ptr()))
        return out

    def tree_sum(self, x, out=None):
        """alpgpu_tree_sum_f64 over a float64 device tensor"""
        if out is None:
            out = torch.empty(1, dtype=torch.float64, device=x.device)
        _check(lib.alpgpu_tree_sum_f64(self.h, _vp(x.data_ptr()), x.numel(), _vp(out.data_ptr())), "alpgpu_tree_sum_f64")
        return out

    def column_validate(self, col: "DeviceColumn"):
        """alpgpu_column_validate: None when every descriptor is well-formed, else the index of the first bad vector"""
        bad = _u64(0)
        rc = lib.alpgpu_column_validate(self.h, C.byref(col.c), 8 if col.dtype == "f64" else 4, C.byref(bad))
        if rc == 0:
            return None
        if rc != -2:
            _check(rc, "alpgpu_column_validate")
        return int(bad.value)

    def decode_sum(self, col: "DeviceColumn", out=None):
        """per-vector sums (float64) of the decoded values without materialising them (alpgpu_decode_sum_f64 / _f32)"""
        if out is None:
            out = torch.empty(col.n_vectors, dtype=torch.float64, device=f"cuda:{self.device}")
        self._call("decode_sum", col.dtype, C.byref(col.c), _vp(out.data_ptr()))
        return out

    def decode(self, col: "DeviceColumn", out=None):
        tdt = _TORCH_TYPE[col.dtype]
        if out is None:
            out = torch.empty(col.n_vectors * VECTOR_SIZE, dtype=tdt, device=f"cuda:{self.device}")
        assert out.is_contiguous() and out.numel() >= col.n_vectors * VECTOR_SIZE and out.dtype == tdt
        self._call("decode", col.dtype, C.byref(col.c), _vp(out.data_ptr()))
        return out

    # ---- random access (include/alpgpu.h: alpgpu_gather_*, alpgpu_decode_slice_*) -----------------------------------
    def gather(self, col: "DeviceColumn", idx, out=None):
        """the values at the value indices idx (a contiguous int64 tensor on this context's device; any order, repeats allowed) as a float64 /
        float32 tensor; an index outside [0, n_vectors * 1024) gives the canonical quiet NaN"""
        self._check_tensor(idx, torch.int64, "idx")
        tdt = _TORCH_TYPE[col.dtype]
        if out is None:
            out = torch.empty(idx.numel(), dtype=tdt, device=self._dev)
        assert out.is_contiguous() and out.numel() >= idx.numel() and out.dtype == tdt
        self._call("gather", col.dtype, C.byref(col.c), _vp(idx.data_ptr()), idx.numel(), _vp(out.data_ptr()))
        return out

    def decode_slice(self, col: "DeviceColumn", first: int, n: int, out=None):
        """values first .. first + n - 1 of the column (any first); AlpGpuError if the slice reaches past the column's n_vectors * 1024 values"""
        tdt = _TORCH_TYPE[col.dtype]
        if out is None:
            out = torch.empty(max(0, int(n)), dtype=tdt, device=self._dev)
        assert out.is_contiguous() and out.numel() >= n and out.dtype == tdt
        self._call("decode_slice", col.dtype, C.byref(col.c), first, n, _vp(out.data_ptr()))
        return out

    # ---- the argument rules the query wrappers share: each refuses with ValueError, and nothing here touches the device but _scratch and the
    # last lines of _list_to_device ---------------------------------------------------------------------------------------
    @property
    def _dev(self):
        return f"cuda:{self.device}"

    def _check_tensor(self, t, dtype, name):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or t.device.index != self.device or not t.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor on cuda:%d" % (name, str(dtype).replace("torch.", ""), self.device))

    def _check_shape(self, t, dtype, name, shape, what, records=False):
        """an output of exactly this shape (what: the shape in the caller's words); records: rows {min, max}, aligned to them"""
        self._check_tensor(t, dtype, name)
        if tuple(t.shape) != tuple(shape) or (records and t.data_ptr() % (2 * t.element_size())):
            raise ValueError("%s must be a contiguous %s tensor of shape %s%s" % (name, str(dtype).replace("torch.", ""), what, ", aligned to its records" if records else ""))

    def _check_at_least(self, t, dtype, name, n, what):
        """an output of at least n elements (what: that number in the caller's words)"""
        self._check_tensor(t, dtype, name)
        if t.numel() < n:
            raise ValueError("%s must hold %s" % (name, what))

    @staticmethod
    def _range(col, first, n):
        """(first, n) of a call over the value indices [first, first + n): n None is the rest of the column"""
        first = int(first)
        n = col.n_vectors * VECTOR_SIZE - first if n is None else int(n)
        if first < 0 or n < 0:
            raise ValueError("first and n must not be negative")
        return first, n

    def _check_mask_zones(self, mask, zones, col):
        """the optional bitmap and the optional records of a column's vectors (of two paired columns: of either)"""
        if mask is not None:
            self._check_mask(mask, col.n_vectors)
        if zones is not None:
            self._check_zones(zones, _TORCH_TYPE[col.dtype], col.n_vectors)

    def _check_trace(self, trace, words=4):
        if trace is not None:
            self._check_tensor(trace, torch.int64, "trace")
            if trace.numel() != words:
                raise ValueError("trace must hold %d int64 words" % words)

    def _scratch(self, scratch, need, what):
        """the scratch of a call that needs `need` bytes (what: that number in the caller's words): a new one for None, else the caller's, checked"""
        if scratch is None:
            return torch.empty(need, dtype=torch.uint8, device=self._dev)
        self._check_tensor(scratch, torch.uint8, "scratch")
        if scratch.numel() < need or scratch.data_ptr() % 16:
            raise ValueError("scratch must hold %s bytes, 16-byte aligned" % what)
        return scratch

    @staticmethod
    def _check_len(t, what, lo, hi):
        if t.dim() != 1 or t.numel() < lo or (hi is not None and t.numel() > hi):
            raise ValueError("%s must be one-dimensional and hold %s elements" % (what, "any number of" if hi is None else "%d .. %d" % (lo, hi)))

    def _check_list(self, t, what, col, lo=0, hi=None):
        """the raw forms' list (keys, edges): a contiguous one-dimensional tensor of the column's type on this device, lo .. hi long; returns its length"""
        if not isinstance(t, torch.Tensor) or t.dtype != _TORCH_TYPE[col.dtype]:
            raise ValueError("%s must be a tensor of the column's type (%s)" % (what, col.dtype))
        self._check_len(t, what, lo, hi)
        if not t.is_cuda or t.device.index != self.device or not t.is_contiguous():
            raise ValueError("%s must be contiguous on cuda:%d" % (what, self.device))
        return t.numel()

    def _list_to_device(self, values, what, col, lo=0, hi=None, sorted=False, want_perm=False):
        """the allocating wrappers' list: a device tensor, host tensor, numpy array (of the column's type: none is converted) or sequence (converted
        to it), one-dimensional and lo .. hi long, as the contiguous device tensor the raw form wants, in order by torch.sort on the device unless
        sorted.  want_perm: (list, the sort's permutation or None).  Every refusal comes before anything is moved to or allocated on the device."""
        if isinstance(values, np.ndarray):
            if values.dtype != _NUMPY_TYPE[col.dtype]:
                raise ValueError("%s must be of the column's type (%s)" % (what, col.dtype))
            values = torch.from_numpy(np.ascontiguousarray(values))
        elif not isinstance(values, torch.Tensor):
            values = torch.tensor(list(values), dtype=_TORCH_TYPE[col.dtype])
        if values.dtype != _TORCH_TYPE[col.dtype]:
            raise ValueError("%s must be of the column's type (%s)" % (what, col.dtype))
        self._check_len(values, what, lo, hi)
        if values.is_cuda and values.device.index != self.device:
            raise ValueError("%s must be on the host or on cuda:%d" % (what, self.device))
        lst = values if values.is_cuda else values.to(self._dev)
        lst, perm = (lst.contiguous(), None) if sorted else torch.sort(lst)
        return (lst, perm) if want_perm else lst

    def _call_tuned(self, stem, sfx, args, tuning, trace, record, fields):
        """the plain entry, or with a tuning dict or a trace tensor given debug_<stem>: the same arguments, then the tuning record (a field the
        dict leaves out is 0: the library's choice) and the trace"""
        if tuning is None and trace is None:
            return self._call(stem, sfx, *args)
        tuning = {} if tuning is None else tuning
        if set(tuning) - set(fields):
            raise ValueError("tuning takes " + ", ".join(fields))
        t = record(*[int(tuning.get(k, 0)) for k in fields])
        self._call("debug_" + stem, sfx, *args, C.byref(t), _ptr(trace))

    # ---- selection (include/alpgpu.h: alpgpu_select_range_*) --------------------------------------------------------
    def select_scratch(self, col: "DeviceColumn"):
        """a scratch tensor for select_range_into on this column (alpgpu_select_scratch_bytes; torch allocations are at least 16-byte aligned)"""
        return torch.empty(lib.alpgpu_select_scratch_bytes(col.n_vectors), dtype=torch.uint8, device=f"cuda:{self.device}")

    def select_range_into(self, col: "DeviceColumn", lo: float, hi: float, idx_out, count_out, vals_out=None, first: int = 0, n: int = None, scratch=None, zones=None):
        """the raw form of alpgpu_select_range_*: the ascending value indices r of [first, first + n) (n None: to the column's end) whose value x
        has lo <= x <= hi go to idx_out (int64; its numel() is the capacity, None or empty: a count), their values to vals_out (optional, at
        least as long), their number to count_out (one int64, the full count also beyond the capacity).  Nothing is synchronised and nothing
        read back; with a scratch given (select_scratch) nothing is allocated either, so the call can be captured into a graph.
        zones (zone_map(col)): alpgpu_select_range_zoned_* — the same result, vectors whose record excludes or contains them are not decoded."""
        tdt = _TORCH_TYPE[col.dtype]
        self._check_at_least(count_out, torch.int64, "count_out", 1, "one int64")
        capacity = 0
        if idx_out is not None:
            self._check_tensor(idx_out, torch.int64, "idx_out")
            capacity = idx_out.numel()
        if vals_out is not None:
            self._check_at_least(vals_out, tdt, "vals_out", capacity, "as many values as idx_out")
        first, n = self._range(col, first, n)
        scratch = self._scratch(scratch, lib.alpgpu_select_scratch_bytes(col.n_vectors), "alpgpu_select_scratch_bytes(n_vectors)")
        outs = (_ptr(idx_out), _ptr(vals_out) if capacity else None, capacity, _vp(count_out.data_ptr()), _vp(scratch.data_ptr()))
        if zones is None:
            self._call("select_range", col.dtype, C.byref(col.c), first, n, lo, hi, *outs)
        else:
            self._check_zones(zones, tdt, col.n_vectors)
            self._call("select_range_zoned", col.dtype, C.byref(col.c), _vp(zones.data_ptr()), first, n, lo, hi, *outs)

    def select_range(self, col: "DeviceColumn", lo: float, hi: float, first: int = 0, n: int = None, values: bool = False, capacity: int = None, zones=None):
        """the ascending value indices of [first, first + n) whose value lies in [lo, hi] as an int64 tensor, or (indices, values) with
        values=True.  capacity None: the call counts first (one device-to-host read of the count, which synchronises the stream), allocates
        exactly and selects; with a capacity given there is no read-back before the selection, one after it to trim the result to
        min(count, capacity)."""
        count = torch.empty(1, dtype=torch.int64, device=self._dev)
        scratch = self.select_scratch(col)
        if capacity is None:
            self.select_range_into(col, lo, hi, None, count, first=first, n=n, scratch=scratch, zones=zones)
            capacity = int(count.item())
        idx = torch.empty(int(capacity), dtype=torch.int64, device=self._dev)
        vals = torch.empty(int(capacity), dtype=_TORCH_TYPE[col.dtype], device=self._dev) if values else None
        self.select_range_into(col, lo, hi, idx, count, vals, first=first, n=n, scratch=scratch, zones=zones)
        k = min(int(count.item()), int(capacity))
        return (idx[:k], vals[:k]) if values else idx[:k]

    # ---- selection bitmaps (include/alpgpu.h: alpgpu_select_mask_*, alpgpu_mask_to_indices, alpgpu_decode_sum_masked_*, alpgpu_decode_masked_*) ---
    _MASK_OPS = {"set": MASK_SET, "and": MASK_AND, "or": MASK_OR}

    def _check_mask(self, mask, n_vectors=None):
        self._check_tensor(mask, torch.int64, "mask")
        if mask.dim() != 1 or mask.numel() % 16 or (n_vectors is not None and mask.numel() != 16 * n_vectors):
            raise ValueError("mask must be a one-dimensional int64 tensor of 16 words per vector" + ("" if n_vectors is None else " (%d)" % (16 * n_vectors)))

    def _check_op(self, op, mask, n_vectors):
        """ALPGPU_MASK_* of op, which without a mask to combine into can only be "set" (the caller then makes one, after its other checks)"""
        if op not in self._MASK_OPS:
            raise ValueError('op must be "set", "and" or "or"')
        if mask is not None:
            self._check_mask(mask, n_vectors)
        elif op != "set":
            raise ValueError('op "%s" combines into a mask: pass one' % op)
        return self._MASK_OPS[op]

    def select_mask(self, col: "DeviceColumn", lo: float, hi: float, first: int = 0, n: int = None, op: str = "set", mask=None):
        """the qualify mask of lo <= x <= hi over the value indices [first, first + n) (n None: to the column's end) as a selection bitmap: an int64
        tensor of 16 words per vector, bit r & 63 of word r >> 6 = value index r.  op "set" writes it (mask None: a new tensor), "and" / "or"
        combine it into the mask given: "and" clears the bits outside the range, "or" leaves them.  Returns the mask.  Nothing is
        synchronised; with a mask given nothing is allocated either (alpgpu_select_mask_f64 / _f32)."""
        op = self._check_op(op, mask, col.n_vectors)
        first, n = self._range(col, first, n)
        if mask is None:
            mask = torch.empty(16 * col.n_vectors, dtype=torch.int64, device=self._dev)
        self._call("select_mask", col.dtype, C.byref(col.c), first, n, lo, hi, op, _vp(mask.data_ptr()))
        return mask

    def mask_to_indices_into(self, mask, idx_out, count_out, scratch=None):
        """the raw form of alpgpu_mask_to_indices: the set bits of the mask as ascending value indices into idx_out (int64; its numel() is the
        capacity, None or empty: a count), their number into count_out (one int64, the full count also beyond the capacity).  Nothing is
        synchronised; with a scratch given (alpgpu_select_scratch_bytes(mask.numel() // 16) bytes of uint8) nothing is allocated."""
        self._check_mask(mask)
        n_vectors = mask.numel() // 16
        self._check_at_least(count_out, torch.int64, "count_out", 1, "one int64")
        if idx_out is not None:
            self._check_tensor(idx_out, torch.int64, "idx_out")
        scratch = self._scratch(scratch, lib.alpgpu_select_scratch_bytes(n_vectors), "alpgpu_select_scratch_bytes(n_vectors)")
        _check(lib.alpgpu_mask_to_indices(self.h, _vp(mask.data_ptr()), n_vectors, _ptr(idx_out), 0 if idx_out is None else idx_out.numel(), _vp(count_out.data_ptr()),
                                          _vp(scratch.data_ptr())), "alpgpu_mask_to_indices")

    def mask_to_indices(self, mask, capacity: int = None):
        """the set bits of a selection bitmap as an ascending int64 tensor of value indices.  capacity None: the call counts first (one read of
        the count, which synchronises the stream) and allocates exactly; with a capacity the result is trimmed to min(count, capacity)."""
        self._check_mask(mask)
        count = torch.empty(1, dtype=torch.int64, device=self._dev)
        scratch = torch.empty(lib.alpgpu_select_scratch_bytes(mask.numel() // 16), dtype=torch.uint8, device=self._dev)
        if capacity is None:
            self.mask_to_indices_into(mask, None, count, scratch)
            capacity = int(count.item())
        idx = torch.empty(int(capacity), dtype=torch.int64, device=self._dev)
        self.mask_to_indices_into(mask, idx, count, scratch)
        return idx[:min(int(count.item()), int(capacity))]

    def _per_vector_out(self, out, counts, n_vectors):
        """the masked sums' outputs: one float64 per vector (a new tensor for None) and, optionally, one int32 count per vector"""
        if out is None:
            out = torch.empty(n_vectors, dtype=torch.float64, device=self._dev)
        else:
            self._check_at_least(out, torch.float64, "out", n_vectors, "one float64 per vector")
        if counts is not None:
            self._check_at_least(counts, torch.int32, "counts", n_vectors, "one int32 per vector")
        return out

    def decode_sum_masked(self, col: "DeviceColumn", mask, out=None, counts=None):
        """per-vector sums (float64) of the decoded values whose bit is set in the mask, in the order include/alpgpu.h documents for
        alpgpu_decode_sum_masked_f64 / _f32; counts (optional, int32, one per vector) receives each vector's number of set bits.  The column's
        total is tree_sum(out)."""
        self._check_mask(mask, col.n_vectors)
        out = self._per_vector_out(out, counts, col.n_vectors)
        self._call("decode_sum_masked", col.dtype, C.byref(col.c), _vp(mask.data_ptr()), _vp(out.data_ptr()), _ptr(counts))
        return out

    def decode_masked_into(self, col: "DeviceColumn", mask, vals_out, count_out, idx_out=None, scratch=None):
        """the raw form of alpgpu_decode_masked_f64 / _f32: the column's values at the set bits of the mask, in ascending index order, into
        vals_out (the column's value type; its numel() is the capacity, None or empty: a count), their value indices into idx_out (optional,
        int64, at least as long), their number into count_out (one int64, the full count also beyond the capacity).  Nothing is
        synchronised and nothing read back; with a scratch given (select_scratch) nothing is allocated either, so the call can be captured
        into a graph.  The mask is only read."""
        self._check_mask(mask, col.n_vectors)
        self._check_at_least(count_out, torch.int64, "count_out", 1, "one int64")
        capacity = 0
        if vals_out is not None:
            self._check_tensor(vals_out, _TORCH_TYPE[col.dtype], "vals_out")
            capacity = vals_out.numel()
        if idx_out is not None:
            self._check_at_least(idx_out, torch.int64, "idx_out", capacity, "as many indices as vals_out")
        scratch = self._scratch(scratch, lib.alpgpu_select_scratch_bytes(col.n_vectors), "alpgpu_select_scratch_bytes(n_vectors)")
        self._call("decode_masked", col.dtype, C.byref(col.c), _vp(mask.data_ptr()), _ptr(vals_out), _ptr(idx_out) if capacity else None, capacity,
                   _vp(count_out.data_ptr()), _vp(scratch.data_ptr()))

    def decode_masked(self, col: "DeviceColumn", mask, indices: bool = False, capacity: int = None):
        """the column's values at the set bits of a selection bitmap as a tensor of the column's value type, ascending by index, or
        (indices, values) with indices=True.  capacity None: the call counts first (one read of the count, which synchronises the stream) and
        allocates exactly; with a capacity there is no read-back before the projection, one after it to trim the result to
        min(count, capacity)."""
        count = torch.empty(1, dtype=torch.int64, device=self._dev)
        scratch = self.select_scratch(col)
        if capacity is None:
            self.decode_masked_into(col, mask, None, count, scratch=scratch)
            capacity = int(count.item())
        vals = torch.empty(int(capacity), dtype=_TORCH_TYPE[col.dtype], device=self._dev)
        idx = torch.empty(int(capacity), dtype=torch.int64, device=self._dev) if indices else None
        self.decode_masked_into(col, mask, vals, count, idx, scratch=scratch)
        k = min(int(count.item()), int(capacity))
        return (idx[:k], vals[:k]) if indices else vals[:k]

    # ---- two-column consumers (include/alpgpu.h: alpgpu_compare_mask_*, alpgpu_decode_dot_masked_*) -------------------------
    _CMP_OPS = {"lt": CMP_LT, "le": CMP_LE, "gt": CMP_GT, "ge": CMP_GE, "eq": CMP_EQ, "ne": CMP_NE}

    @staticmethod
    def _check_pair(a, b):
        if a.dtype != b.dtype or a.n_vectors != b.n_vectors:
            raise ValueError("the two columns must have the same dtype and the same number of vectors")

    def compare_mask(self, a: "DeviceColumn", b: "DeviceColumn", cmp: str = "lt", first: int = 0, n: int = None, op: str = "set", mask=None):
        """the qualify mask of a_r CMP b_r between two columns of equal length and dtype over the value indices [first, first + n) (n None: to the
        columns' end) as a selection bitmap.  cmp is "lt", "le", "gt", "ge", "eq" or "ne" with C's meaning (a NaN on either side: only "ne"
        holds); op and mask as in select_mask.  Returns the mask.  Nothing is synchronised; with a mask given nothing is allocated either
        (alpgpu_compare_mask_f64 / _f32)."""
        self._check_pair(a, b)
        if cmp not in self._CMP_OPS:
            raise ValueError('cmp must be "lt", "le", "gt", "ge", "eq" or "ne"')
        op = self._check_op(op, mask, a.n_vectors)
        first, n = self._range(a, first, n)
        if mask is None:
            mask = torch.empty(16 * a.n_vectors, dtype=torch.int64, device=self._dev)
        self._call("compare_mask", a.dtype, C.byref(a.c), C.byref(b.c), first, n, self._CMP_OPS[cmp], op, _vp(mask.data_ptr()))
        return mask

    def decode_dot_masked(self, a: "DeviceColumn", b: "DeviceColumn", mask, out=None, counts=None):
        """per-vector sums (float64) of a_r * b_r over the set bits of the mask, product and sum rounded separately in the order
        include/alpgpu.h documents for alpgpu_decode_dot_masked_f64 / _f32; counts (optional, int32, one per vector) receives each vector's
        number of set bits.  The total is tree_sum(out)."""
        self._check_pair(a, b)
        self._check_mask(mask, a.n_vectors)
        out = self._per_vector_out(out, counts, a.n_vectors)
        self._call("decode_dot_masked", a.dtype, C.byref(a.c), C.byref(b.c), _vp(mask.data_ptr()), _vp(out.data_ptr()), _ptr(counts))
        return out

    # ---- grouped aggregation (include/alpgpu.h: alpgpu_decode_group_sum_*, alpgpu_group_totals) -----------------------------------
    @staticmethod
    def _group_bounds(lo, hi, dtype):
        """(n_groups, lo, hi) with the bounds as C arrays of the columns' type"""
        try:
            lo, hi = [float(t) for t in lo], [float(t) for t in hi]
        except TypeError:
            raise ValueError("lo and hi must be sequences of numbers") from None
        if len(hi) != len(lo) or not 1 <= len(lo) <= GROUP_MAX:
            raise ValueError("lo and hi must hold the same number of bounds, 1 .. %d" % GROUP_MAX)
        ft = (C.c_double if dtype == "f64" else C.c_float) * len(lo)
        return len(lo), ft(*lo), ft(*hi)

    def decode_group_sum(self, val: "DeviceColumn", key: "DeviceColumn", mask, lo, hi, out=None, counts=None):
        """per-group, per-vector sums of val over the set bits of the mask whose key lies in the closed range lo[g] <= k <= hi[g] (select_mask's
        predicate), every group settled in one pass over the two columns: a [n_groups, n_vectors] float64 tensor, row g bit for bit what
        decode_sum_masked(val) gives under the mask ANDed with select_mask(key, lo[g], hi[g]).  lo, hi: sequences of 1 .. GROUP_MAX floats of
        equal length; counts (optional, int32, the same shape) receives the number of values each sum adds.  Every group's total is
        group_totals(out, counts).  Nothing is synchronised (alpgpu_decode_group_sum_f64 / _f32)."""
        self._check_pair(val, key)
        self._check_mask(mask, val.n_vectors)
        n_groups, lo, hi = self._group_bounds(lo, hi, val.dtype)
        if out is None:
            out = torch.empty((n_groups, val.n_vectors), dtype=torch.float64, device=self._dev)
        else:
            self._check_shape(out, torch.float64, "out", (n_groups, val.n_vectors), "[n_groups, n_vectors]")
        if counts is not None:
            self._check_shape(counts, torch.int32, "counts", (n_groups, val.n_vectors), "[n_groups, n_vectors]")
        self._call("decode_group_sum", val.dtype, C.byref(val.c), C.byref(key.c), _vp(mask.data_ptr()), lo, hi, n_groups, _vp(out.data_ptr()), _ptr(counts))
        return out

    def group_totals_scratch(self, n_vectors: int, n_groups: int):
        """a scratch tensor for group_totals (alpgpu_group_totals_scratch_bytes; torch allocations are at least 16-byte aligned)"""
        return torch.empty(lib.alpgpu_group_totals_scratch_bytes(int(n_vectors), int(n_groups)), dtype=torch.uint8, device=f"cuda:{self.device}")

    def group_totals(self, sums, counts=None, scratch=None, out=None, counts_out=None):
        """every group's total of a [n_groups, n_vectors] float64 tensor of per-vector sums, row by row the tree of tree_sum, and (with counts,
        int32 of the same shape) every group's exact count: (float64[n_groups], int64[n_groups] or None).  With scratch (group_totals_scratch),
        out and counts_out given nothing is allocated (alpgpu_group_totals)."""
        self._check_tensor(sums, torch.float64, "sums")
        if sums.dim() != 2 or not 1 <= sums.shape[0] <= GROUP_MAX:
            raise ValueError("sums must be a [n_groups, n_vectors] float64 tensor of 1 .. %d groups" % GROUP_MAX)
        n_groups, n_vectors = int(sums.shape[0]), int(sums.shape[1])
        if counts is not None:
            self._check_shape(counts, torch.int32, "counts", (n_groups, n_vectors), "[n_groups, n_vectors]")
        elif counts_out is not None:
            raise ValueError("counts_out without counts")
        scratch = self._scratch(scratch, lib.alpgpu_group_totals_scratch_bytes(n_vectors, n_groups), "group_totals_scratch(n_vectors, n_groups)")
        if out is None:
            out = torch.empty(n_groups, dtype=torch.float64, device=self._dev)
        else:
            self._check_tensor(out, torch.float64, "out")
            if out.numel() != n_groups:
                raise ValueError("out must hold one float64 per group")
        if counts is not None:
            if counts_out is None:
                counts_out = torch.empty(n_groups, dtype=torch.int64, device=self._dev)
            else:
                self._check_tensor(counts_out, torch.int64, "counts_out")
                if counts_out.numel() != n_groups:
                    raise ValueError("counts_out must hold one int64 per group")
        _check(lib.alpgpu_group_totals(self.h, _vp(sums.data_ptr()), _ptr(counts), n_vectors, n_groups, _vp(out.data_ptr()), _ptr(counts_out) if counts is not None else None,
                                       _vp(scratch.data_ptr())), "alpgpu_group_totals")
        return out, counts_out

    # ---- masked and grouped MIN / MAX (include/alpgpu.h: alpgpu_decode_minmax_masked_*, alpgpu_decode_group_minmax_*, alpgpu_group_minmax_totals_*) ---
    def decode_minmax_masked(self, col: "DeviceColumn", mask, out=None, counts=None):
        """per-vector records {min, max} over the decoded values whose bit is set in the mask: a [n_vectors, 2] tensor of the column's value type
        with the rules of zone_map (NaNs ignored, -0.0 < +0.0, {+inf, -inf} when nothing selected is a number); counts (optional, int32, one per
        vector) receives each vector's number of set bits.  The column's MIN / MAX is column_minmax(out).  The records are narrower than the
        vectors' intervals: not a zone map for select_range.  Nothing is synchronised (alpgpu_decode_minmax_masked_f64 / _f32)."""
        self._check_mask(mask, col.n_vectors)
        if out is None:
            out = torch.empty((col.n_vectors, 2), dtype=_TORCH_TYPE[col.dtype], device=self._dev)
        else:
            self._check_zones(out, _TORCH_TYPE[col.dtype], col.n_vectors)
        if counts is not None:
            self._check_at_least(counts, torch.int32, "counts", col.n_vectors, "one int32 per vector")
        self._call("decode_minmax_masked", col.dtype, C.byref(col.c), _vp(mask.data_ptr()), _vp(out.data_ptr()), _ptr(counts))
        return out

    def decode_group_minmax(self, val: "DeviceColumn", key: "DeviceColumn", mask, lo, hi, out=None, counts=None):
        """per-group, per-vector records {min, max} of val over the set bits of the mask whose key lies in the closed range lo[g] <= k <= hi[g]
        (select_mask's predicate), every group settled in one pass over the two columns: a [n_groups, n_vectors, 2] tensor of the columns' value
        type, row g bit for bit what decode_minmax_masked(val) gives under the mask ANDed with select_mask(key, lo[g], hi[g]).  lo, hi: sequences
        of 1 .. GROUP_MAX floats of equal length; counts (optional, int32 [n_groups, n_vectors]) receives what decode_group_sum counts.  Every
        group's MIN / MAX is group_minmax_totals(out).  Nothing is synchronised (alpgpu_decode_group_minmax_f64 / _f32)."""
        self._check_pair(val, key)
        self._check_mask(mask, val.n_vectors)
        n_groups, lo, hi = self._group_bounds(lo, hi, val.dtype)
        if out is None:
            out = torch.empty((n_groups, val.n_vectors, 2), dtype=_TORCH_TYPE[val.dtype], device=self._dev)
        else:
            self._check_shape(out, _TORCH_TYPE[val.dtype], "out", (n_groups, val.n_vectors, 2), "[n_groups, n_vectors, 2]", records=True)
        if counts is not None:
            self._check_shape(counts, torch.int32, "counts", (n_groups, val.n_vectors), "[n_groups, n_vectors]")
        self._call("decode_group_minmax", val.dtype, C.byref(val.c), C.byref(key.c), _vp(mask.data_ptr()), lo, hi, n_groups, _vp(out.data_ptr()), _ptr(counts))
        return out

    def group_minmax_totals(self, zones, out=None):
        """every group's {min, max} of a [n_groups, n_vectors, 2] tensor of records: a [n_groups, 2] tensor, row g what column_minmax(zones[g])
        gives; {+inf, -inf} for n_vectors == 0.  No scratch (alpgpu_group_minmax_totals_f64 / _f32)."""
        if not isinstance(zones, torch.Tensor) or zones.dtype not in (torch.float64, torch.float32):
            raise ValueError("zones must be a float64 or float32 tensor")
        self._check_tensor(zones, zones.dtype, "zones")
        if zones.dim() != 3 or zones.shape[2] != 2 or not 1 <= zones.shape[0] <= GROUP_MAX or zones.data_ptr() % (2 * zones.element_size()):
            raise ValueError("zones must be a [n_groups, n_vectors, 2] tensor of 1 .. %d groups, aligned to its records" % GROUP_MAX)
        n_groups, n_vectors = int(zones.shape[0]), int(zones.shape[1])
        if out is None:
            out = torch.empty((n_groups, 2), dtype=zones.dtype, device=zones.device)
        else:
            self._check_shape(out, zones.dtype, "out", (n_groups, 2), "[n_groups, 2]")
        self._call("group_minmax_totals", self._sfx(zones), _ptr(zones), n_vectors, n_groups, _vp(out.data_ptr()))
        return out

    # ---- set membership (include/alpgpu.h: alpgpu_select_in_mask_*, alpgpu_in_list_lds_max) ---------------------------------
    @staticmethod
    def in_list_lds_max(dtype) -> int:
        """the longest list select_in_mask holds whole in LDS: dtype is "f64" / "f32", a torch or numpy float64 / float32 type; 0 for anything else"""
        name = str(dtype).replace("torch.", "").replace("<class 'numpy.", "").replace("'>", "")
        return int(lib.alpgpu_in_list_lds_max({"f64": 8, "float64": 8, "f32": 4, "float32": 4}.get(name, 0)))

    def select_in_mask(self, col: "DeviceColumn", values, first: int = 0, n: int = None, negate: bool = False, zones=None, op: str = "set", mask=None, sorted: bool = False):
        """the qualify mask of `x IN (values)` — negate: `x NOT IN (values)`, which a NaN satisfies — over the value indices [first, first + n) as a
        selection bitmap, set or combined as select_mask does it.  A value is a member iff some element == it: -0.0 matches +0.0, a NaN never
        matches.  values: a device tensor, host tensor, sequence or numpy array of the column's type; it is brought into list form by torch.sort on
        the device (nothing dropped or deduplicated: NaNs sort last and are inert); sorted=True skips that for a caller who guarantees the
        order.  zones (zone_map(col)): the same bytes, vectors whose record holds no element are not decoded.  Returns the mask.  Nothing is
        synchronised; with a mask and a sorted device tensor given nothing is allocated either (alpgpu_select_in_mask_f64 / _f32)."""
        op = self._check_op(op, mask, col.n_vectors)
        if zones is not None:
            self._check_zones(zones, _TORCH_TYPE[col.dtype], col.n_vectors)
        first, n = self._range(col, first, n)
        lst = self._list_to_device(values, "values", col, sorted=sorted)
        if mask is None:
            mask = torch.empty(16 * col.n_vectors, dtype=torch.int64, device=self._dev)
        self._call("select_in_mask", col.dtype, C.byref(col.c), first, n, _ptr(lst), lst.numel(), 1 if negate else 0, _ptr(zones), op, _vp(mask.data_ptr()))
        return mask

    # ---- top-k (include/alpgpu.h: alpgpu_top_k_scratch_bytes, alpgpu_top_k_*) ---------------------------------------------
    @staticmethod
    def _check_k(k):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) <= TOP_K_MAX:
            raise ValueError("k must be an integer in 0 .. %d" % TOP_K_MAX)
        return int(k)

    def top_k_scratch(self, col: "DeviceColumn", k: int):
        """a scratch tensor for top_k_into on this column with this k or a smaller one (alpgpu_top_k_scratch_bytes; torch allocations are at least
        16-byte aligned)"""
        return torch.empty(lib.alpgpu_top_k_scratch_bytes(col.n_vectors, self._check_k(k)), dtype=torch.uint8, device=f"cuda:{self.device}")

    def top_k_into(self, col: "DeviceColumn", mask, k: int, vals_out, count_out, idx_out=None, largest: bool = True, records=None, scratch=None):
        """the raw form of alpgpu_top_k_f64 / _f32: the k largest (largest=False: smallest) values among the set bits of the mask that are no NaNs,
        in the order include/alpgpu.h defines (-0.0 below +0.0, equal bit patterns by ascending index), into vals_out (the column's value type, at
        least k long), their value indices into idx_out (optional, int64, at least k long), their number min(k, selected values that are no
        NaNs) into count_out (one int64).  Nothing is written behind the count.  records: the EXACT masked records of the column under this mask
        (decode_minmax_masked, or zone_map under a mask of every real value): the first decode pass is skipped; anything else there gives an
        unspecified selection.  Nothing is synchronised and nothing read back; with a scratch given (top_k_scratch) nothing is allocated
        either, so the call can be captured into a graph.  The mask is only read."""
        tdt = _TORCH_TYPE[col.dtype]
        k = self._check_k(k)
        self._check_mask(mask, col.n_vectors)
        self._check_at_least(count_out, torch.int64, "count_out", 1, "one int64")
        self._check_at_least(vals_out, tdt, "vals_out", k, "k values")
        if idx_out is not None:
            self._check_at_least(idx_out, torch.int64, "idx_out", k, "k indices")
        if records is not None:
            self._check_zones(records, tdt, col.n_vectors)
            if records.data_ptr() % 16:
                raise ValueError("records must be 16-byte aligned")
        scratch = self._scratch(scratch, lib.alpgpu_top_k_scratch_bytes(col.n_vectors, k), "alpgpu_top_k_scratch_bytes(n_vectors, k)")
        nowhere = _vp(scratch.data_ptr())  # (a tensor without elements has no address: the library wants one even where it writes nothing)
        self._call("top_k", col.dtype, C.byref(col.c), _ptr(mask) or nowhere, _ptr(records), k, 1 if largest else 0, _ptr(vals_out) or nowhere, _ptr(idx_out),
                   _vp(count_out.data_ptr()), nowhere)

    def top_k(self, col: "DeviceColumn", mask, k: int, largest: bool = True, records=None, indices: bool = True):
        """(values, indices) — values alone with indices=False — of the k largest (largest=False: smallest) values among the set bits of the mask,
        NaNs left out, largest (smallest) first, equal bit patterns by ascending index; trimmed to min(k, how many there are).  One read of the
        count, which synchronises the stream."""
        k = self._check_k(k)
        vals = torch.empty(k, dtype=_TORCH_TYPE[col.dtype], device=self._dev)
        idx = torch.empty(k, dtype=torch.int64, device=self._dev) if indices else None
        count = torch.empty(1, dtype=torch.int64, device=self._dev)
        self.top_k_into(col, mask, k, vals, count, idx, largest=largest, records=records)
        n = min(int(count.item()), k)
        return (vals[:n], idx[:n]) if indices else vals[:n]

    # ---- quantiles (include/alpgpu.h: alpgpu_quantile_scratch_bytes, alpgpu_select_rank_*, alpgpu_quantile_*) ------------
    @staticmethod
    def _check_ranks(ranks):
        if isinstance(ranks, (str, bytes)) or not hasattr(ranks, "__len__") or not 1 <= len(ranks) <= RANK_MAX:
            raise ValueError("ranks must be a sequence of 1 .. %d integers" % RANK_MAX)
        out = []
        for r in ranks:
            if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 0 <= int(r) < 2**64:
                raise ValueError("a rank must be an integer in 0 .. 2^64 - 1")
            out.append(int(r))
        return out

    @staticmethod
    def _check_q(q):
        if isinstance(q, (str, bytes)) or not hasattr(q, "__len__") or not 1 <= len(q) <= QUANTILE_MAX:
            raise ValueError("q must be a sequence of 1 .. %d numbers" % QUANTILE_MAX)
        out = []
        for x in q:
            if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not 0.0 <= float(x) <= 1.0:
                raise ValueError("a quantile must be a number in [0, 1]")
            out.append(float(x))
        return out

    def quantile_scratch(self, col: "DeviceColumn"):
        """a scratch tensor for select_rank_into / quantile_into on this column (alpgpu_quantile_scratch_bytes; torch allocations are at least 16-byte
        aligned)"""
        return torch.empty(lib.alpgpu_quantile_scratch_bytes(col.n_vectors), dtype=torch.uint8, device=f"cuda:{self.device}")

    def _check_quantile_args(self, col, mask, vals_out, n_vals, count_out, zones, scratch):
        self._check_mask(mask, col.n_vectors)
        self._check_at_least(count_out, torch.int64, "count_out", 1, "one int64")
        self._check_at_least(vals_out, _TORCH_TYPE[col.dtype], "vals_out", n_vals, "%d values" % n_vals)
        if zones is not None:
            self._check_zones(zones, _TORCH_TYPE[col.dtype], col.n_vectors)
        return self._scratch(scratch, lib.alpgpu_quantile_scratch_bytes(col.n_vectors), "alpgpu_quantile_scratch_bytes(n_vectors)")

    def select_rank_into(self, col: "DeviceColumn", mask, ranks, vals_out, count_out, from_top: bool = False, zones=None, scratch=None, tuning=None):
        """the raw form of alpgpu_select_rank_f64 / _f32: with S the values at the set bits of the mask that are no NaNs, sorted in the order
        include/alpgpu.h defines (-0.0 below +0.0), N = |S| goes to count_out (one int64) and S[min(ranks[i], N - 1)] — from_top: counted from the
        largest — to vals_out[i] (the column's value type, at least len(ranks) long).  N == 0 writes the count alone.  ranks: 1 .. 32 integers on the
        host, in any order, repeats allowed.  zones: any records that contain the vectors' masked intervals (zone_map, decode_minmax_masked,
        widened ones): the same bytes, vectors are skipped by them.  tuning: {"capacity", "max_workgroups", "flush_every"} for the debug entry
        (alpgpu_debug_quantile_*; the same bytes).  Nothing is synchronised and nothing read back; with a scratch given (quantile_scratch)
        nothing is allocated either, so the call can be captured into a graph.  The mask is only read."""
        ranks = self._check_ranks(ranks)
        scratch = self._check_quantile_args(col, mask, vals_out, len(ranks), count_out, zones, scratch)
        args = [C.byref(col.c), _ptr(mask) or _vp(scratch.data_ptr()), _ptr(zones), (_u64 * len(ranks))(*ranks), len(ranks), 1 if from_top else 0, _vp(vals_out.data_ptr()),
                _vp(count_out.data_ptr()), _vp(scratch.data_ptr())]
        if tuning is None:  # (not _call_tuned: the debug entry is named for the family, not for select_rank, and takes no trace)
            self._call("select_rank", col.dtype, *args)
        else:
            if set(tuning) - {"capacity", "max_workgroups", "flush_every"}:
                raise ValueError("tuning takes capacity, max_workgroups, flush_every")
            t = QuantileTuning(int(tuning.get("capacity", 0)), int(tuning.get("max_workgroups", 0)), int(tuning.get("flush_every", 0)))
            self._call("debug_quantile", col.dtype, *args, C.byref(t))

    def quantile_into(self, col: "DeviceColumn", mask, q, vals_out, count_out, ranks_out=None, zones=None, scratch=None):
        """the raw form of alpgpu_quantile_f64 / _f32: for each q[i] (1 .. 16 numbers in [0, 1] on the host) the rank r = min(N - 1, floor(q[i] * (N - 1)))
        (numpy's method="lower") goes to ranks_out[i] (optional, int64), S[r] to vals_out[2 i] and S[min(r + 1, N - 1)] to vals_out[2 i + 1] (the
        column's value type, at least 2 len(q) long), N to count_out; S, zones, scratch and the promises as for select_rank_into."""
        q = self._check_q(q)
        if ranks_out is not None:
            self._check_at_least(ranks_out, torch.int64, "ranks_out", len(q), "len(q) ranks")
        scratch = self._check_quantile_args(col, mask, vals_out, 2 * len(q), count_out, zones, scratch)
        self._call("quantile", col.dtype, C.byref(col.c), _ptr(mask) or _vp(scratch.data_ptr()), _ptr(zones), (C.c_double * len(q))(*q), len(q), _vp(vals_out.data_ptr()),
                   _ptr(ranks_out), _vp(count_out.data_ptr()), _vp(scratch.data_ptr()))

    def quantile_trace(self, scratch):
        """what the last select_rank / quantile call on this scratch did (include/alpgpu.h: alpgpu_debug_quantile_trace); synchronises the stream"""
        self._check_tensor(scratch, torch.uint8, "scratch")
        t = QuantileTrace()
        _check(lib.alpgpu_debug_quantile_trace(self.h, _vp(scratch.data_ptr()), C.byref(t)), "alpgpu_debug_quantile_trace")
        return {"compact_pass": int(t.compact_pass), "wide_grid": int(t.wide_grid), "waves_per_wg": int(t.waves_per_wg), "candidates": int(t.candidates), "n": int(t.n),
                "zero_skips": int(t.zero_skips), "zone_skips": [int(x) for x in t.zone_skips]}

    def select_rank(self, col: "DeviceColumn", mask, ranks, from_top: bool = False, zones=None):
        """(values, N): values[i] the ranks[i]-th smallest (from_top: largest) of the values at the set bits of the mask that are no NaNs, ranks
        beyond the last clamped to it; an empty tensor for N == 0.  One read of the count, which synchronises the stream."""
        ranks = self._check_ranks(ranks)
        vals = torch.empty(len(ranks), dtype=_TORCH_TYPE[col.dtype], device=self._dev)
        count = torch.empty(1, dtype=torch.int64, device=self._dev)
        self.select_rank_into(col, mask, ranks, vals, count, from_top=from_top, zones=zones)
        n = int(count.item())
        return (vals if n else vals[:0]), n

    def quantile(self, col: "DeviceColumn", mask, q, interpolation: str = "linear", zones=None):
        """the quantiles q (a number or 1 .. 16 of them, in [0, 1]) of the values at the set bits of the mask that are no NaNs, as a device tensor:
        interpolation "lower" / "higher": the neighbour below / above q * (N - 1), of the column's type and bit for bit a value of the column (numpy's
        method="lower" / "higher"); "linear": lo + (hi - lo) * (q * (N - 1) - r) in double, by torch ops on the device tensors.  NaN where nothing
        is selected.  Nothing is synchronised."""
        if interpolation not in ("linear", "lower", "higher"):
            raise ValueError('interpolation must be "linear", "lower" or "higher"')
        scalar = isinstance(q, (int, float, np.integer, np.floating)) and not isinstance(q, bool)
        q = self._check_q([q] if scalar else q)
        dev = f"cuda:{self.device}"
        vals = torch.full((len(q), 2), float("nan"), dtype=_TORCH_TYPE[col.dtype], device=dev)
        ranks = torch.zeros(len(q), dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        self.quantile_into(col, mask, q, vals, count, ranks, zones=zones)
        if interpolation == "linear":
            pos = torch.tensor(q, dtype=torch.float64, device=dev) * (count - 1).clamp(min=0).to(torch.float64)
            lo, hi = vals[:, 0].to(torch.float64), vals[:, 1].to(torch.float64)
            frac = pos - ranks.to(torch.float64)
            out = torch.where((frac == 0) | (hi == lo), lo, lo + (hi - lo) * frac)  # (an infinite neighbour at weight 0, or twice, is no NaN)
        else:
            out = vals[:, 0 if interpolation == "lower" else 1]
        return out[0] if scalar else out

    # ---- histograms (include/alpgpu.h: alpgpu_histogram_*) ---------------------------------------------------------------
    def histogram_into(self, col: "DeviceColumn", edges, counts_out, mask=None, first: int = 0, n: int = None, right: bool = False, zones=None, accumulate: bool = False,
                       tuning=None, trace=None):
        """the raw form of alpgpu_histogram_f64 / _f32: counts_out (int64, exactly len(edges) + 2 words) takes — accumulate: is added — the bucket counts
        of the values at the indices [first, first + n) whose bit is set in the mask (None: every index of the range).  Bucket b = the number of
        edges <= x (right: < x), so 0 lies below the first edge and len(edges) at or above the last; the last word counts the NaNs.  edges: a SORTED
        contiguous device tensor of the column's type, at most HISTOGRAM_EDGES_MAX long (NaNs last are inert, duplicates give empty buckets).  zones:
        any records that contain the vectors' intervals (zone_map, decode_minmax_masked, widened ones): the same counts, vectors are settled or their
        search narrowed by them.  tuning: {"grid", "flush_every"}, trace: an int64 device tensor of 4 words that is ADDED to (vectors settled without
        the column, from their record, by the few-bucket route (always 0), decoded); either sends the call through the debug entry
        (alpgpu_debug_histogram_*; the same counts).  Nothing is synchronised, allocated or read back, so the call can be captured into a graph."""
        n_edges = self._check_list(edges, "edges", col, 0, HISTOGRAM_EDGES_MAX)
        self._check_shape(counts_out, torch.int64, "counts_out", (n_edges + 2,), "[len(edges) + 2]")
        self._check_mask_zones(mask, zones, col)
        first, n = self._range(col, first, n)
        self._check_trace(trace)
        args = [C.byref(col.c), first, n, _ptr(mask), _ptr(zones), _ptr(edges), n_edges, 1 if right else 0, 1 if accumulate else 0, _vp(counts_out.data_ptr())]
        self._call_tuned("histogram", col.dtype, args, tuning, trace, HistogramTuning, ("grid", "flush_every"))

    def histogram(self, col: "DeviceColumn", edges, mask=None, first: int = 0, n: int = None, right: bool = False, zones=None, out=None, accumulate: bool = False,
                  sorted: bool = False):
        """the histogram of the column's values at the indices [first, first + n) whose bit is set in the mask (None: all of them) as an int64 device
        tensor of len(edges) + 2 words: word b counts the values with b edges <= x (right: < x) — numpy.searchsorted(edges, x, side="right") /
        torch.bucketize(x, edges, right=True); right=True: side="left" — and the last word the NaNs.  -0.0 == +0.0; +-inf are ordinary values and
        edges.  edges: a device tensor, host tensor, sequence or numpy array of the column's type, at most HISTOGRAM_EDGES_MAX long; it is brought
        into order by torch.sort on the device (NaNs sort last and are inert); sorted=True skips that for a caller who guarantees the order.
        out: the tensor to write or, with accumulate, to add to (shards, successive ranges, several columns).  zones (zone_map(col) or any records
        that contain the vectors' intervals): the same counts.  Nothing is synchronised; with out and a sorted device tensor given nothing is
        allocated either (alpgpu_histogram_f64 / _f32)."""
        if out is None and accumulate:
            raise ValueError("accumulate adds to a tensor: pass out")
        first, n = self._range(col, first, n)
        lst = self._list_to_device(edges, "edges", col, 0, HISTOGRAM_EDGES_MAX, sorted=sorted)
        if out is None:
            out = torch.zeros(lst.numel() + 2, dtype=torch.int64, device=self._dev)  # (zeroed, where the others are empty: a column of no vectors writes nothing)
        else:
            self._check_shape(out, torch.int64, "out", (lst.numel() + 2,), "[len(edges) + 2]")
        self.histogram_into(col, lst, out, mask=mask, first=first, n=n, right=right, zones=zones, accumulate=accumulate)
        return out

    # ---- distinct values (include/alpgpu.h: alpgpu_distinct_*) ----------------------------------------------------------
    _DISTINCT_TUNING = ("grid", "flush_every", "lds_slots", "table_slots", "sort_tile")

    def distinct_scratch(self, capacity: int):
        """a scratch tensor for distinct_into with this capacity (alpgpu_distinct_scratch_bytes; torch allocations are at least 16-byte aligned)"""
        capacity = int(capacity)
        if not 1 <= capacity <= DISTINCT_MAX:
            raise ValueError("capacity must be in 1 .. %d" % DISTINCT_MAX)
        return torch.empty(lib.alpgpu_distinct_scratch_bytes(capacity), dtype=torch.uint8, device=f"cuda:{self.device}")

    def distinct_into(self, col: "DeviceColumn", vals_out, state_out, counts_out=None, mask=None, first: int = 0, n: int = None, zones=None, scratch=None, tuning=None, trace=None):
        """the raw form of alpgpu_distinct_f64 / _f32: the distinct values, ascending, of the values at the indices [first, first + n) whose bit is set
        in the mask (None: every index of the range) go to vals_out (the column's type; its numel() is the capacity, 1 .. DISTINCT_MAX), how often
        each occurs to counts_out (optional, int64, at least as long).  -0.0 and +0.0 are one value, reported as +0.0; NaNs are no values, only
        counted.  state_out (int64, 4 words): the entries written, the selected NaNs, the selected values that are no NaNs, 1 if there are more
        distinct values than the capacity (then the entries are unspecified; nothing is written beyond the capacity).  zones: any records that
        contain the vectors' intervals: the same bytes, constant ALP vectors are settled from their record.  tuning: {"grid", "flush_every",
        "lds_slots", "table_slots", "sort_tile"}, trace: an int64 device tensor of 6 words that is ADDED to; either sends the call through the
        debug entry (alpgpu_debug_distinct_*; the same bytes).  Nothing is synchronised and nothing read back; with a scratch given
        (distinct_scratch) nothing is allocated either, so the call can be captured into a graph."""
        self._check_tensor(vals_out, _TORCH_TYPE[col.dtype], "vals_out")
        capacity = vals_out.numel()
        if vals_out.dim() != 1 or not 1 <= capacity <= DISTINCT_MAX:
            raise ValueError("vals_out must be one-dimensional and hold 1 .. %d values" % DISTINCT_MAX)
        self._check_tensor(state_out, torch.int64, "state_out")
        if state_out.numel() != 4:
            raise ValueError("state_out must hold 4 int64 words")
        if counts_out is not None:
            self._check_at_least(counts_out, torch.int64, "counts_out", capacity, "as many counts as vals_out")
        self._check_mask_zones(mask, zones, col)
        first, n = self._range(col, first, n)
        self._check_trace(trace, 6)  # (6 words where the other families' traces have 4)
        scratch = self._scratch(scratch, lib.alpgpu_distinct_scratch_bytes(capacity), "alpgpu_distinct_scratch_bytes(capacity)")
        args = [C.byref(col.c), first, n, _ptr(mask), _ptr(zones), capacity, _vp(vals_out.data_ptr()), _ptr(counts_out), _vp(state_out.data_ptr()), _vp(scratch.data_ptr())]
        self._call_tuned("distinct", col.dtype, args, tuning, trace, DistinctTuning, self._DISTINCT_TUNING)

    def distinct(self, col: "DeviceColumn", mask=None, first: int = 0, n: int = None, zones=None, capacity: int = 65536, counts: bool = True):
        """(values, counts, n_nan, overflow): the distinct values, ascending, of the column's values at the indices [first, first + n) whose bit is set in
        the mask (None: all of them) as a device tensor of the column's type, how often each occurs as an int64 device tensor (None with
        counts=False), the number of selected NaNs (which are no values) and whether there are more than `capacity` distinct values: then
        values and counts are unspecified and the call wants a larger capacity (at most DISTINCT_MAX).  -0.0 == +0.0, one value, reported as +0.0.
        The values are a valid sorted list for select_in_mask, edge array for histogram and key array for join_probe.  One read of the state,
        which synchronises the stream (alpgpu_distinct_f64 / _f32)."""
        dev = f"cuda:{self.device}"
        capacity = int(capacity)
        if not 1 <= capacity <= DISTINCT_MAX:
            raise ValueError("capacity must be in 1 .. %d" % DISTINCT_MAX)
        vals = torch.empty(capacity, dtype=_TORCH_TYPE[col.dtype], device=dev)
        cnt = torch.empty(capacity, dtype=torch.int64, device=dev) if counts else None
        state = torch.empty(4, dtype=torch.int64, device=dev)
        self.distinct_into(col, vals, state, counts_out=cnt, mask=mask, first=first, n=n, zones=zones)
        d, n_nan, _, overflow = state.tolist()
        return vals[:d], (cnt[:d] if counts else None), n_nan, bool(overflow)

    # ---- keyed aggregation (include/alpgpu.h: alpgpu_decode_keyed_sum_*) ------------------------------------------------
    def keyed_sum_scratch(self, n_vectors: int, n_keys: int):
        """a scratch tensor for keyed_sum_into (alpgpu_keyed_sum_scratch_bytes; torch allocations are at least 16-byte aligned)"""
        n_vectors, n_keys = int(n_vectors), int(n_keys)
        if n_vectors < 0 or not 1 <= n_keys <= KEYED_KEYS_MAX:
            raise ValueError("n_vectors must not be negative and n_keys must be in 1 .. %d" % KEYED_KEYS_MAX)
        return torch.empty(lib.alpgpu_keyed_sum_scratch_bytes(n_vectors, n_keys), dtype=torch.uint8, device=f"cuda:{self.device}")

    def keyed_sum_into(self, val: "DeviceColumn", key: "DeviceColumn", keys, sums_out, counts_out=None, mask=None, zones=None, scratch=None, tuning=None, trace=None):
        """the raw form of alpgpu_decode_keyed_sum_f64 (double columns only): sums_out (float64, exactly len(keys)) takes, per key, the sum of val over the rows whose
        bit is set in the mask (None: every row) and whose value of the key column == that key (the first of equal keys; -0.0 == +0.0; a NaN
        matches nothing), in the order include/alpgpu.h documents; counts_out (optional, int64, exactly len(keys) + 1) their exact numbers and, in
        its last word, the selected rows that match no key.  keys: a SORTED contiguous device tensor of the columns' type, 1 .. KEYED_KEYS_MAX long.
        zones: any records that contain the KEY vectors' intervals (zone_map(key), widened ones): the same bits.  tuning: {"grid"}, trace: an int64
        device tensor of 4 words that is ADDED to (vectors settled without either column, by the constant-key shortcut, with a record that admits
        no key, decoded); either sends the call through the debug entry (the same bits).  Nothing is synchronised or read back; with a scratch
        given (keyed_sum_scratch) nothing is allocated either, so the call can be captured into a graph."""
        self._check_pair(val, key)
        if val.dtype != "f64":
            raise ValueError("keyed_sum is built for double columns only")
        n_keys = self._check_list(keys, "keys", val, 1, KEYED_KEYS_MAX)
        self._check_shape(sums_out, torch.float64, "sums_out", (n_keys,), "[len(keys)]")
        if counts_out is not None:
            self._check_shape(counts_out, torch.int64, "counts_out", (n_keys + 1,), "[len(keys) + 1]")
        self._check_mask_zones(mask, zones, key)
        self._check_trace(trace)
        scratch = self._scratch(scratch, lib.alpgpu_keyed_sum_scratch_bytes(val.n_vectors, n_keys), "keyed_sum_scratch(n_vectors, n_keys)")
        args = [C.byref(val.c), C.byref(key.c), _ptr(mask), _ptr(zones), _vp(keys.data_ptr()), n_keys, _vp(sums_out.data_ptr()), _ptr(counts_out), _vp(scratch.data_ptr())]
        self._call_tuned("decode_keyed_sum", val.dtype, args, tuning, trace, KeyedTuning, ("grid",))

    def keyed_sum(self, val: "DeviceColumn", key: "DeviceColumn", keys, mask=None, zones=None, counts: bool = True, sorted: bool = False):
        """SUM(val), COUNT(*) GROUP BY key for the given keys in one pass over the two columns: (float64[K] sums, int64[K] counts or None with
        counts=False, unmatched), K = len(keys) in 1 .. KEYED_KEYS_MAX, in the order of the SORTED keys.  keys: a device tensor, host tensor,
        sequence or numpy array of the columns' type; it is brought into order by torch.sort on the device (NaNs sort last and never match);
        sorted=True skips that for a caller who guarantees the order (what distinct returns is in order).  A row belongs to the first key equal to
        its value of the key column; later duplicates get +0.0 and 0.  unmatched: the selected rows that match no key, an int64 device scalar
        (None with counts=False).  zones (zone_map(key) or any records that contain the key vectors' intervals): the same bits.  Nothing is
        synchronised (alpgpu_decode_keyed_sum_f64; double columns only)."""
        self._check_pair(val, key)
        if val.dtype != "f64":
            raise ValueError("keyed_sum is built for double columns only")  # (the float entry points are not built: include/alpgpu.h says why)
        lst = self._list_to_device(keys, "keys", val, 1, KEYED_KEYS_MAX, sorted=sorted)
        sums = torch.empty(lst.numel(), dtype=torch.float64, device=self._dev)
        cnt = torch.empty(lst.numel() + 1, dtype=torch.int64, device=self._dev) if counts else None
        self.keyed_sum_into(val, key, lst, sums, counts_out=cnt, mask=mask, zones=zones)
        return sums, (cnt[:-1] if counts else None), (cnt[-1] if counts else None)

    # ---- keyed MIN / MAX (include/alpgpu.h: alpgpu_decode_keyed_minmax_*) ----------------------------------------------
    def keyed_minmax_into(self, val: "DeviceColumn", key: "DeviceColumn", keys, out, counts_out=None, mask=None, zones=None, tuning=None, trace=None):
        """the raw form of alpgpu_decode_keyed_minmax_f64 / _f32: out ([len(keys), 2] of the columns' type) takes, per key, the record {min, max} of
        val over the rows whose bit is set in the mask (None: every row) and whose value of the key column == that key (the first of equal keys;
        -0.0 == +0.0; a NaN matches nothing): NaN values ignored, -0.0 < +0.0, {+inf, -inf} for a key without a number; counts_out (optional,
        int64, exactly len(keys) + 1) the rows of each key, NaN values included, and, in its last word, the selected rows that match no key.
        keys: a SORTED contiguous device tensor of the columns' type, 1 .. KEYED_KEYS_MAX long.  zones: any records that contain the KEY vectors'
        intervals: the same bytes.  tuning: {"grid"}, trace: an int64 device tensor of 4 words that is ADDED to (keyed_sum_into's); either sends
        the call through the debug entry (the same bytes).  Nothing is synchronised, read back or allocated, so the call can be captured."""
        self._keyed_minmax_into("decode_keyed_minmax", KEYED_KEYS_MAX, val, key, keys, out, counts_out, mask, zones, tuning, trace)

    def _keyed_minmax_into(self, stem, keys_max, val, key, keys, out, counts_out, mask, zones, tuning, trace):
        """keyed_minmax_into and keyed_minmax_many_into: the same arguments and checks, up to keys_max keys, into the entry points of this stem"""
        self._check_pair(val, key)
        n_keys = self._check_list(keys, "keys", val, 1, keys_max)
        self._check_shape(out, _TORCH_TYPE[val.dtype], "out", (n_keys, 2), "[len(keys), 2]", records=True)
        if counts_out is not None:
            self._check_shape(counts_out, torch.int64, "counts_out", (n_keys + 1,), "[len(keys) + 1]")
        self._check_mask_zones(mask, zones, key)
        self._check_trace(trace)
        args = [C.byref(val.c), C.byref(key.c), _ptr(mask), _ptr(zones), _vp(keys.data_ptr()), n_keys, _vp(out.data_ptr()), _ptr(counts_out)]
        self._call_tuned(stem, val.dtype, args, tuning, trace, KeyedTuning, ("grid",))

    def _keyed_minmax(self, into, keys_max, val, key, keys, mask, zones, counts, sorted):
        """keyed_minmax and keyed_minmax_many: the keys onto the device and into order, the outputs made, the raw form called"""
        self._check_pair(val, key)
        lst = self._list_to_device(keys, "keys", val, 1, keys_max, sorted=sorted)
        out = torch.empty((lst.numel(), 2), dtype=lst.dtype, device=self._dev)
        cnt = torch.empty(lst.numel() + 1, dtype=torch.int64, device=self._dev) if counts else None
        into(val, key, lst, out, counts_out=cnt, mask=mask, zones=zones)
        return out, (cnt[:-1] if counts else None), (cnt[-1] if counts else None)

    def keyed_minmax(self, val: "DeviceColumn", key: "DeviceColumn", keys, mask=None, zones=None, counts: bool = True, sorted: bool = False):
        """MIN(val), MAX(val), COUNT(*) GROUP BY key for the given keys in one pass over the two columns: ([K, 2] records {min, max} of the
        columns' type, int64[K] counts or None with counts=False, unmatched), K = len(keys) in 1 .. KEYED_KEYS_MAX, in the order of the SORTED
        keys.  keys: a device tensor, host tensor, sequence or numpy array of the columns' type; brought into order by torch.sort on the device
        (NaNs sort last and never match); sorted=True skips that.  A row belongs to the first key equal to its value of the key column; a key
        without a number, and every later duplicate, gets {+inf, -inf}.  NaN values are counted and ignored.  unmatched: the selected rows that
        match no key, an int64 device scalar (None with counts=False).  Nothing is synchronised (alpgpu_decode_keyed_minmax_f64 / _f32)."""
        return self._keyed_minmax(self.keyed_minmax_into, KEYED_KEYS_MAX, val, key, keys, mask, zones, counts, sorted)

    # ---- keyed MIN / MAX, many keys (include/alpgpu.h: alpgpu_decode_keyed_minmax_many_*) -----------------------------
    def keyed_minmax_many_into(self, val: "DeviceColumn", key: "DeviceColumn", keys, out, counts_out=None, mask=None, zones=None, tuning=None, trace=None):
        """the raw form of alpgpu_decode_keyed_minmax_many_f64 / _f32: keyed_minmax_into's arguments, records and counts (the same bytes up to
        KEYED_KEYS_MAX keys) with keys 1 .. KEYED_MANY_KEYS_MAX long: the keys beyond what LDS holds are searched through pivots, and the table is
        out and counts_out themselves, updated by integer atomics in device memory.  counts_out=None issues no count atomic at all: the usual call
        behind distinct(), whose counts on the same selection are these.  Nothing is synchronised, read back or allocated, so the call can be
        captured."""
        self._keyed_minmax_into("decode_keyed_minmax_many", KEYED_MANY_KEYS_MAX, val, key, keys, out, counts_out, mask, zones, tuning, trace)

    def keyed_minmax_many(self, val: "DeviceColumn", key: "DeviceColumn", keys, mask=None, zones=None, counts: bool = True):
        """MIN(val), MAX(val), COUNT(*) GROUP BY key for up to KEYED_MANY_KEYS_MAX keys in one pass over the two columns: keyed_minmax's argument
        forms and result, ([K, 2] records {min, max} of the columns' type, int64[K] counts or None with counts=False, unmatched), in the order
        of the SORTED keys (torch.sort on the device: NaNs last, where they match nothing).  counts=False keeps no counts at all, which is the
        cheaper call where distinct() has already counted.  Nothing is synchronised (alpgpu_decode_keyed_minmax_many_f64 / _f32)."""
        return self._keyed_minmax(self.keyed_minmax_many_into, KEYED_MANY_KEYS_MAX, val, key, keys, mask, zones, counts, sorted=False)  # (always sorts)

    # ---- exact keyed SUM (include/alpgpu.h: alpgpu_decode_keyed_exact_sum_*) ---------------------------------------------
    def keyed_sum_exact_table(self, n_keys: int):
        """a table for keyed_sum_exact_into with this many keys (alpgpu_keyed_exact_sum_table_bytes; torch allocations are at least 16-byte
        aligned).  Its contents are irrelevant before a call without accumulate; calls with accumulate add to it."""
        n_keys = int(n_keys)
        if not 1 <= n_keys <= KEYED_MANY_KEYS_MAX:
            raise ValueError("n_keys must be in 1 .. %d" % KEYED_MANY_KEYS_MAX)
        return torch.empty(lib.alpgpu_keyed_exact_sum_table_bytes(n_keys), dtype=torch.uint8, device=self._dev)

    def keyed_sum_exact_into(self, val: "DeviceColumn", key: "DeviceColumn", keys, sums_out, counts_out=None, mask=None, zones=None, table=None, accumulate: bool = False,
                             tuning=None, trace=None):
        """the raw form of alpgpu_decode_keyed_exact_sum_f64 / _f32: keyed_minmax_many_into's columns, keys (SORTED, on the device, 1 ..
        KEYED_MANY_KEYS_MAX long), match, counts, bitmap and zones; sums_out (float64 for both precisions, exactly len(keys)) takes, per key, the
        CORRECTLY ROUNDED real sum of val over its selected rows: a NaN if a NaN or both infinities are among them, an infinity if it is, +-inf
        where the sum rounds beyond the largest double, +0.0 for no row; the same bytes on every grid, device and row order.  table
        (keyed_sum_exact_table(len(keys)); None: a new one) holds the sums as integers.  accumulate: the table and counts_out are added to and
        not zeroed first, and sums_out is written from the table as it then stands, so calls over shards, ranges of a bitmap or further columns
        extend the sums exactly; it needs the table of the earlier call.  A table takes at most 2^31 rows in all; one call at most
        KEYED_EXACT_VECTORS_MAX vectors.  tuning: {"grid"}, trace: an int64 device tensor of 6 words that is ADDED to (keyed_sum_into's four,
        the steps summed in registers, the steps sent lane by lane); either sends the call through the debug entry (the same bytes).  Nothing
        is synchronised or read back; with a table given nothing is allocated either, so the call can be captured into a graph."""
        self._check_pair(val, key)
        n_keys = self._check_list(keys, "keys", val, 1, KEYED_MANY_KEYS_MAX)
        if val.n_vectors > KEYED_EXACT_VECTORS_MAX:
            raise ValueError("one call takes at most %d vectors" % KEYED_EXACT_VECTORS_MAX)
        self._check_shape(sums_out, torch.float64, "sums_out", (n_keys,), "[len(keys)]")
        if counts_out is not None:
            self._check_shape(counts_out, torch.int64, "counts_out", (n_keys + 1,), "[len(keys) + 1]")
        self._check_mask_zones(mask, zones, key)
        self._check_trace(trace, 6)  # (6 words where the family's other traces have 4)
        if accumulate and table is None:
            raise ValueError("accumulate adds to a table: pass the one of the earlier call")
        table = self._scratch(table, lib.alpgpu_keyed_exact_sum_table_bytes(n_keys), "keyed_sum_exact_table(len(keys))")
        args = [C.byref(val.c), C.byref(key.c), _ptr(mask), _ptr(zones), _vp(keys.data_ptr()), n_keys, _vp(sums_out.data_ptr()), _ptr(counts_out), _vp(table.data_ptr()),
                1 if accumulate else 0]
        self._call_tuned("decode_keyed_exact_sum", val.dtype, args, tuning, trace, KeyedTuning, ("grid",))

    def keyed_sum_exact(self, val: "DeviceColumn", key: "DeviceColumn", keys, mask=None, zones=None, counts: bool = True, sorted: bool = False):
        """SUM(val), COUNT(*) GROUP BY key for up to KEYED_MANY_KEYS_MAX keys in one pass over the two columns, every sum correctly rounded:
        (float64[K] sums, int64[K] counts or None with counts=False, unmatched), in the order of the SORTED keys.  keys: keyed_sum's forms,
        brought into order by torch.sort on the device unless sorted.  Double and float columns; the sums are float64 for both.  To extend
        sums over further calls use keyed_sum_exact_into with a table and accumulate.  Nothing is synchronised
        (alpgpu_decode_keyed_exact_sum_f64 / _f32)."""
        self._check_pair(val, key)
        lst = self._list_to_device(keys, "keys", val, 1, KEYED_MANY_KEYS_MAX, sorted=sorted)
        if val.n_vectors > KEYED_EXACT_VECTORS_MAX:
            raise ValueError("one call takes at most %d vectors" % KEYED_EXACT_VECTORS_MAX)
        sums = torch.empty(lst.numel(), dtype=torch.float64, device=self._dev)
        cnt = torch.empty(lst.numel() + 1, dtype=torch.int64, device=self._dev) if counts else None
        self.keyed_sum_exact_into(val, key, lst, sums, counts_out=cnt, mask=mask, zones=zones)
        return sums, (cnt[:-1] if counts else None), (cnt[-1] if counts else None)

    # ---- bucketed aggregation (include/alpgpu.h: alpgpu_decode_bucket_sum_* / alpgpu_decode_bucket_minmax_*) -----------
    def bucket_sum_scratch(self, n_vectors: int, n_edges: int):
        """a scratch tensor for bucket_sum_into (alpgpu_bucket_sum_scratch_bytes = keyed_sum_scratch's for n_edges + 1 keys)"""
        n_vectors, n_edges = int(n_vectors), int(n_edges)
        if n_vectors < 0 or not 0 <= n_edges <= BUCKET_EDGES_MAX:
            raise ValueError("n_vectors must not be negative and n_edges must be in 0 .. %d" % BUCKET_EDGES_MAX)
        return torch.empty(lib.alpgpu_bucket_sum_scratch_bytes(n_vectors, n_edges), dtype=torch.uint8, device=f"cuda:{self.device}")

    def bucket_sum_into(self, val: "DeviceColumn", key: "DeviceColumn", edges, sums_out, counts_out=None, right: bool = False, mask=None, zones=None, scratch=None,
                        tuning=None, trace=None):
        """the raw form of alpgpu_decode_bucket_sum_f64 / _f32: sums_out (float64, exactly len(edges) + 1) takes, per bucket of the KEY column, the sum
        of val over the rows whose bit is set in the mask (None: every row), in keyed_sum_into's documented order; counts_out (optional, int64,
        exactly len(edges) + 2) what histogram_into writes for key: the buckets' rows and, last, the rows whose key is a NaN (they enter no sum).
        Bucket b = the number of edges <= key (right: < key).  edges: a SORTED contiguous device tensor of the columns' type, 0 .. BUCKET_EDGES_MAX
        long (NaNs last are inert, duplicates give empty buckets).  zones: any records that contain the KEY vectors' intervals: the same bits; a
        vector whose record lies in one bucket is settled without its key values.  tuning: {"grid"}, trace: an int64 device tensor of 4 words that
        is ADDED to (vectors settled without either column, by the one-bucket shortcut, always 0, decoded); either sends the call through the
        debug entry (the same bits).  Nothing is synchronised or read back; with a scratch given (bucket_sum_scratch) nothing is allocated either,
        so the call can be captured into a graph."""
        self._check_pair(val, key)
        n_edges = self._check_list(edges, "edges", val, 0, BUCKET_EDGES_MAX)
        self._check_shape(sums_out, torch.float64, "sums_out", (n_edges + 1,), "[len(edges) + 1]")
        if counts_out is not None:
            self._check_shape(counts_out, torch.int64, "counts_out", (n_edges + 2,), "[len(edges) + 2]")  # (histogram's words; the keyed forms have len + 1)
        self._check_mask_zones(mask, zones, key)
        self._check_trace(trace)
        scratch = self._scratch(scratch, lib.alpgpu_bucket_sum_scratch_bytes(val.n_vectors, n_edges), "bucket_sum_scratch(n_vectors, n_edges)")
        args = [C.byref(val.c), C.byref(key.c), _ptr(mask), _ptr(zones), _ptr(edges), n_edges, 1 if right else 0, _vp(sums_out.data_ptr()), _ptr(counts_out),
                _vp(scratch.data_ptr())]
        self._call_tuned("decode_bucket_sum", val.dtype, args, tuning, trace, KeyedTuning, ("grid",))

    def bucket_minmax_into(self, val: "DeviceColumn", key: "DeviceColumn", edges, out, counts_out=None, right: bool = False, mask=None, zones=None, tuning=None, trace=None):
        """the raw form of alpgpu_decode_bucket_minmax_f64 / _f32: out ([len(edges) + 1, 2] of the columns' type) takes, per bucket of the KEY column,
        the record {min, max} of val over the selected rows: NaN values ignored but counted, -0.0 < +0.0, {+inf, -inf} for a bucket without a
        number; counts_out, right, edges, zones, tuning and trace are bucket_sum_into's.  counts_out=None keeps no count at all.  Nothing is
        synchronised, read back or allocated, so the call can be captured."""
        self._check_pair(val, key)
        n_edges = self._check_list(edges, "edges", val, 0, BUCKET_EDGES_MAX)
        self._check_shape(out, _TORCH_TYPE[val.dtype], "out", (n_edges + 1, 2), "[len(edges) + 1, 2]", records=True)
        if counts_out is not None:
            self._check_shape(counts_out, torch.int64, "counts_out", (n_edges + 2,), "[len(edges) + 2]")
        self._check_mask_zones(mask, zones, key)
        self._check_trace(trace)
        args = [C.byref(val.c), C.byref(key.c), _ptr(mask), _ptr(zones), _ptr(edges), n_edges, 1 if right else 0, _vp(out.data_ptr()), _ptr(counts_out)]
        self._call_tuned("decode_bucket_minmax", val.dtype, args, tuning, trace, KeyedTuning, ("grid",))

    def bucket_sum(self, val: "DeviceColumn", key: "DeviceColumn", edges, right: bool = False, mask=None, zones=None, counts: bool = True, sorted: bool = False):
        """SUM(val), COUNT(*) GROUP BY bucket(key) in one pass over the two columns: (float64[B] sums, int64[B + 1] counts or None with
        counts=False), B = len(edges) + 1 buckets, so len(edges) + 2 count words.  Bucket b holds the rows with b edges <= key (right: < key) — numpy.searchsorted(edges, key,
        side="right") / side="left" —; counts are histogram(key, edges)'s words: counts[:B] the buckets' rows, counts[-1] the rows whose key is a NaN.  AVG is
        sums / counts[:B].  edges: a device tensor, host tensor, sequence or numpy array of the columns' type, at most BUCKET_EDGES_MAX long,
        brought into order by torch.sort on the device (NaNs sort last and are inert); sorted=True skips that.  zones (zone_map(key) or any
        records that contain the key vectors' intervals): the same bits.  Nothing is synchronised (alpgpu_decode_bucket_sum_f64 / _f32)."""
        self._check_pair(val, key)
        lst = self._list_to_device(edges, "edges", val, 0, BUCKET_EDGES_MAX, sorted=sorted)
        sums = torch.empty(lst.numel() + 1, dtype=torch.float64, device=self._dev)
        cnt = torch.empty(lst.numel() + 2, dtype=torch.int64, device=self._dev) if counts else None
        self.bucket_sum_into(val, key, lst, sums, counts_out=cnt, right=right, mask=mask, zones=zones)
        return sums, cnt

    def bucket_minmax(self, val: "DeviceColumn", key: "DeviceColumn", edges, right: bool = False, mask=None, zones=None, counts: bool = True, sorted: bool = False):
        """MIN(val), MAX(val), COUNT(*) GROUP BY bucket(key) in one pass over the two columns: ([B, 2] records {min, max} of the columns' type,
        int64[B + 1] counts or None with counts=False), B = len(edges) + 1; bucket_sum's buckets, edges and counts.  NaN values are counted and
        ignored; a bucket without a number gets {+inf, -inf}.  Nothing is synchronised (alpgpu_decode_bucket_minmax_f64 / _f32)."""
        self._check_pair(val, key)
        lst = self._list_to_device(edges, "edges", val, 0, BUCKET_EDGES_MAX, sorted=sorted)
        out = torch.empty((lst.numel() + 1, 2), dtype=lst.dtype, device=self._dev)
        cnt = torch.empty(lst.numel() + 2, dtype=torch.int64, device=self._dev) if counts else None
        self.bucket_minmax_into(val, key, lst, out, counts_out=cnt, right=right, mask=mask, zones=zones)
        return out, cnt

    # ---- join probe (include/alpgpu.h: alpgpu_join_probe_*) -----------------------------------------------------------
    def join_probe_into(self, col: "DeviceColumn", keys, pos_out, count_out, mask=None, rows=None, span_out=None, idx_out=None, zones=None, scratch=None):
        """the raw form of alpgpu_join_probe_f64 / _f32: one row per set bit of the mask (None: every index), ascending.  keys: a SORTED contiguous
        device tensor of the column's type (numpy.sort's order, NaNs last).  pos_out (int64; its numel() is the capacity, None or empty: a count)
        takes the position of the first key == the value, rows[that position] with rows (int64, one per key) given, or JOIN_NO_MATCH; span_out
        (optional, int32, at least as long) the number of equal keys; idx_out (optional, int64, at least as long) the value index; count_out (one
        int64) the number of set bits, also beyond the capacity.  zones (zone_map(col)): the same bytes, vectors whose record admits no key are
        not decoded.  Nothing is synchronised and nothing read back; without a mask, or with a scratch given (select_scratch), nothing is
        allocated either, so the call can be captured into a graph."""
        n_keys = self._check_list(keys, "keys", col)
        self._check_at_least(count_out, torch.int64, "count_out", 1, "one int64")
        capacity = 0
        if pos_out is not None:
            self._check_tensor(pos_out, torch.int64, "pos_out")
            capacity = pos_out.numel()
        if span_out is not None:
            self._check_at_least(span_out, torch.int32, "span_out", capacity, "as many spans as pos_out")
        if idx_out is not None:
            self._check_at_least(idx_out, torch.int64, "idx_out", capacity, "as many indices as pos_out")
        if rows is not None:
            self._check_at_least(rows, torch.int64, "rows", n_keys, "one int64 per key")
        self._check_mask_zones(mask, zones, col)
        if mask is not None:  # (the scratch serves the mask's scan alone)
            scratch = self._scratch(scratch, lib.alpgpu_select_scratch_bytes(col.n_vectors), "alpgpu_select_scratch_bytes(n_vectors)")
        self._call("join_probe", col.dtype, C.byref(col.c), _ptr(mask), _ptr(zones), _ptr(keys), n_keys, _ptr(rows) if n_keys else None, _ptr(pos_out),
                   _ptr(span_out) if capacity else None, _ptr(idx_out) if capacity else None, capacity, _vp(count_out.data_ptr()),
                   _vp(scratch.data_ptr()) if mask is not None else None)

    def join_probe(self, col: "DeviceColumn", keys, mask=None, rows=None, span: bool = False, indices: bool = False, zones=None, capacity: int = None, sorted: bool = False):
        """for every set bit of the mask (None: every value of the column), ascending by index, which key the value equals: an int64 tensor pos
        of positions in the SORTED keys (or rows[position] with rows given), JOIN_NO_MATCH (-1) where no key == the value: -0.0 matches +0.0, a
        NaN never matches.  Returns pos, or a tuple (pos[, span][, idx]) with span=True (int32: the number of equal keys, the run
        [pos, pos + span) of the sorted keys) and indices=True (the value indices).  keys: a device tensor, host tensor, sequence or numpy array
        of the column's type; sorted=True promises numpy.sort's order, else the keys are sorted by torch.sort on the device and, unless rows is
        given, rows is that sort's permutation: pos then indexes the keys AS PASSED (among equal keys, one of them), which is what
        gather(dim_col, pos) wants.  rows given with unsorted keys is permuted alongside them.  capacity None: the mask's bits are counted
        first (one read of the count, which synchronises the stream); without a mask the count is the column's length and nothing is read
        back."""
        dev = self._dev
        lst, perm = self._list_to_device(keys, "keys", col, sorted=sorted, want_perm=True)
        if rows is not None:
            if not isinstance(rows, torch.Tensor):
                rows = torch.as_tensor(np.asarray(rows, dtype=np.int64))
            rows = rows.to(dev).contiguous()
            if rows.dtype != torch.int64 or rows.dim() != 1 or rows.numel() != lst.numel():
                raise ValueError("rows must hold one int64 per key")
        if perm is not None:  # (the keys were sorted: rows goes alongside, and without rows the positions are those of the keys as passed)
            rows = perm if rows is None else rows[perm]
        count = torch.empty(1, dtype=torch.int64, device=dev)
        scratch = self.select_scratch(col) if mask is not None else None
        if capacity is None:
            if mask is None:
                capacity = col.n_vectors * VECTOR_SIZE
            else:
                self.join_probe_into(col, lst, None, count, mask=mask, scratch=scratch)
                capacity = int(count.item())
        capacity = int(capacity)
        pos = torch.empty(capacity, dtype=torch.int64, device=dev)
        spn = torch.empty(capacity, dtype=torch.int32, device=dev) if span else None
        idx = torch.empty(capacity, dtype=torch.int64, device=dev) if indices else None
        self.join_probe_into(col, lst, pos, count, mask=mask, rows=rows, span_out=spn, idx_out=idx, zones=zones, scratch=scratch)
        k = capacity if mask is None and capacity <= col.n_vectors * VECTOR_SIZE else min(int(count.item()), capacity)
        out = [pos[:k]] + ([spn[:k]] if span else []) + ([idx[:k]] if indices else [])
        return out[0] if len(out) == 1 else tuple(out)

    # ---- zone maps (include/alpgpu.h: alpgpu_zone_map_*, alpgpu_zones_minmax_*) ---------------------------------------
    def _check_zones(self, zones, dtype, n_vectors):
        self._check_tensor(zones, dtype, "zones")
        if zones.dim() != 2 or zones.shape[1] != 2 or zones.shape[0] < n_vectors or zones.data_ptr() % (2 * zones.element_size()):
            raise ValueError("zones must be a [n_vectors, 2] tensor {min, max}, aligned to its records (16 bytes for float64, 8 for float32)")

    def zone_map(self, col: "DeviceColumn", out=None):
        """the zone map of an encoded column, a [n_vectors, 2] tensor of the column's value type: row v = {min, max} of vector v's decoded
        values, NaNs ignored, -0.0 < +0.0, {+inf, -inf} for a vector of NaNs only (alpgpu_zone_map_f64 / _f32)"""
        if out is None:
            out = torch.empty((col.n_vectors, 2), dtype=_TORCH_TYPE[col.dtype], device=self._dev)
        else:
            self._check_zones(out, _TORCH_TYPE[col.dtype], col.n_vectors)
        self._call("zone_map", col.dtype, C.byref(col.c), _vp(out.data_ptr()))
        return out

    def zone_map_of_values(self, x, out=None):
        """the same records from the raw values: x is a contiguous float64 / float32 tensor of whole vectors on this context's device"""
        if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float64, torch.float32):
            raise ValueError("x must be a float64 or float32 tensor")
        self._check_tensor(x, x.dtype, "x")
        if x.numel() % VECTOR_SIZE or x.data_ptr() % 16:
            raise ValueError("x must hold whole vectors of 1024 values, 16-byte aligned")
        nv = x.numel() // VECTOR_SIZE
        if out is None:
            out = torch.empty((nv, 2), dtype=x.dtype, device=x.device)
        else:
            self._check_zones(out, x.dtype, nv)
        self._call("zone_map_of_values", self._sfx(x), _vp(x.data_ptr()), nv, _vp(out.data_ptr()))
        return out

    def column_minmax(self, zones, out=None):
        """the column's {min, max} as a 2-element tensor: the reduction of a zone map (alpgpu_zones_minmax_f64 / _f32); {+inf, -inf} for no records"""
        if not isinstance(zones, torch.Tensor) or zones.dtype not in (torch.float64, torch.float32):
            raise ValueError("zones must be a float64 or float32 tensor")
        self._check_zones(zones, zones.dtype, 0)
        if out is None:
            out = torch.empty(2, dtype=zones.dtype, device=zones.device)
        else:
            self._check_tensor(out, zones.dtype, "out")
            if out.numel() < 2:
                raise ValueError("out must hold two values")
        self._call("zones_minmax", self._sfx(zones), _vp(zones.data_ptr()), zones.shape[0], _vp(out.data_ptr()))
        return out


class DeviceColumn:
    """A compressed column in HBM (struct alpgpu_column) whose buffers are torch uint8 tensors."""

    def __init__(self, n_vectors: int, device: int = 0, packed_capacity: int | None = None,
                 exc_capacity: int | None = None, dtype: str = "f64", rd_order: bool = True):
        import torch
        assert dtype in ("f64", "f32")
        dev = f"cuda:{device}"
        self.dtype = dtype
        self.n_vectors = int(n_vectors)
        self.n_rowgroups = (self.n_vectors + ROWGROUP_VECTORS - 1) // ROWGROUP_VECTORS
        pcap = lib.alpgpu_packed_capacity if dtype == "f64" else lib.alpgpu_packed_capacity_f32
        ecap = lib.alpgpu_exc_capacity if dtype == "f64" else lib.alpgpu_exc_capacity_f32
        pc = int(pcap(self.n_vectors)) if packed_capacity is None else int(packed_capacity)
        ec = int(ecap(self.n_vectors)) if exc_capacity is None else int(exc_capacity)
        self.rowgroups = torch.zeros(max(1, self.n_rowgroups) * 32, dtype=torch.uint8, device=dev)
        self.vectors = torch.zeros(max(1, self.n_vectors) * 32, dtype=torch.uint8, device=dev)
        self.packed = torch.zeros(pc, dtype=torch.uint8, device=dev)
        self.exc = torch.zeros(ec, dtype=torch.uint8, device=dev)
        self.totals = torch.zeros(8, dtype=torch.int64, device=dev)
        # optional ALP_RD sorted-order table (exception-slot indices identical to the reference's); rd_order=False leaves it out
        self.rd_order = torch.zeros(max(1, self.n_rowgroups) * RD_ORDER_STRIDE, dtype=torch.int16, device=dev) if rd_order else None
        self.c = CColumn(self.n_vectors, self.n_rowgroups, self.rowgroups.data_ptr(), self.vectors.data_ptr(),
                         self.packed.data_ptr(), pc, self.exc.data_ptr(), ec, self.totals.data_ptr(), 0, 0,
                         self.rd_order.data_ptr() if rd_order else None)

    @classmethod
    def from_host(cls, rowgroups: np.ndarray, vectors: np.ndarray, packed: np.ndarray, exc: np.ndarray, device: int = 0, dtype: str = "f64"):
        """Upload host-side records/streams (numpy; see ROWGROUP_DTYPE / VECTOR_DTYPE)."""
        import torch
        n = vectors.size
        col = cls(n, device, packed_capacity=packed.size + 1024, exc_capacity=exc.size + 64, dtype=dtype)
        col.rowgroups[: rowgroups.size * 32] = torch.from_numpy(rowgroups.view(np.uint8).reshape(-1)).to(col.rowgroups.device)
        col.vectors[: n * 32] = torch.from_numpy(vectors.view(np.uint8).reshape(-1)).to(col.vectors.device)
        col.packed[: packed.size] = torch.from_numpy(packed).to(col.packed.device)
        col.exc[: exc.size] = torch.from_numpy(exc).to(col.exc.device)
        col.totals[0] = packed.size
        col.totals[1] = exc.size
        col.c.packed_bytes_hint, col.c.exc_bytes_hint = packed.size, exc.size
        col.c.alp_rd_rowgroups_hint = 1 + int((rowgroups["scheme"] == SCHEME_ALP_RD).sum())
        return col

    def to_host(self):
        rg = self.rowgroups.cpu().numpy().view(ROWGROUP_DTYPE)[: self.n_rowgroups]
        vec = self.vectors.cpu().numpy().view(VECTOR_DTYPE)[: self.n_vectors]
        tot = self.totals.cpu().numpy()
        packed = self.packed[: int(tot[0])].cpu().numpy()
        exc = self.exc[: int(tot[1])].cpu().numpy()
        return rg, vec, packed, exc
