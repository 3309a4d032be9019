"""Host replica of bucketed aggregation (include/alpgpu.h, "bucketed aggregation": alpgpu_decode_bucket_sum_* / alpgpu_decode_bucket_minmax_*), numpy
only.  The bucket is numpy.searchsorted over the edges that are no NaNs, NaN keys apart; sums, records and counts are the keyed replicas' fed the bucket
index as the "key" against np.arange(B), with a NaN index for a NaN key: the documented order is reused, not restated.  tests/test_bucket_cpu.py pins
it; the GPU suites hold the kernels to it bit for bit.  It is fed the values that were encoded or the oracle's decode, never a result of the call
under test."""
import numpy as np

from keyed_minmax_replica import host_keyed_minmax
from keyed_replica import host_keyed_sum, host_keyed_sum_dense

EDGES_MAX = 1023


def bucket_of(key, edges, right=False):
    """per row, as float64: b = #{i : edges[i] <= key} (right: < key) under C's comparisons, NaN for a NaN key.  edges: sorted as numpy.sort sorts,
    NaNs (inert) last"""
    key = np.asarray(key).reshape(-1)
    edges = np.asarray(edges, dtype=key.dtype).reshape(-1)
    assert edges.size <= EDGES_MAX
    real = edges[~np.isnan(edges)]
    assert np.all(np.isnan(edges[real.size:])) and np.all(real[:-1] <= real[1:]), "edges must be sorted with their NaNs last"
    nan = np.isnan(key)
    b = np.full(key.size, np.nan)
    b[~nan] = np.searchsorted(real, key[~nan], side="left" if right else "right")
    return b


def host_bucket_sum(val, key, bits, edges, right=False, dense=False):
    """(sums [B] float64, counts [B + 1] int64), B = len(edges) + 1: counts[:B] the buckets' selected rows, counts[B] the selected rows whose key is a NaN"""
    B = np.asarray(edges).size + 1
    fn = host_keyed_sum_dense if dense else host_keyed_sum
    return fn(np.ascontiguousarray(val).reshape(-1), bucket_of(key, edges, right), bits, np.arange(B, dtype=np.float64))


def host_bucket_minmax(val, key, bits, edges, right=False):
    """(records [B, 2] of val's type, counts [B + 1] int64): NaN values counted and ignored, {+inf, -inf} for a bucket without a number"""
    B = np.asarray(edges).size + 1
    return host_keyed_minmax(np.ascontiguousarray(val).reshape(-1), bucket_of(key, edges, right), bits, np.arange(B, dtype=np.float64))
