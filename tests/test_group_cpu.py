"""CPU: grouped aggregation (include/alpgpu.h, "grouped aggregation") is exported, the header's constant is what the Python side uses, a NULL context
is refused with ALPGPU_ERR_INVALID before the HIP runtime is touched (ALPGPU_CHECK_CTX), so this runs without a device, and the host replica of the
documented order (tests/group_replica.py) is pinned on a hand-made case and against the replicas the masked sum and the dot are held to."""
import ctypes
import os
import subprocess

import numpy as np

from group_replica import adjacent_tree, host_group_sums, host_group_totals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_decode_group_sum_f64", "alpgpu_decode_group_sum_f32", "alpgpu_group_totals_scratch_bytes", "alpgpu_group_totals")
NAN, INF = float("nan"), float("inf")


def test_library_exports_the_group_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols
    assert capi.GROUP_MAX == 16
    for m in ("decode_group_sum", "group_totals", "group_totals_scratch"):
        assert callable(getattr(capi.Context, m))


def test_the_header_declares_them_and_the_group_limit(tmp_path):
    src = tmp_path / "group_decls.c"
    src.write_text('#include "alpgpu.h"\n'
                   '_Static_assert(ALPGPU_GROUP_MAX == 16, "group max");\n'
                   '_Static_assert(sizeof(alpgpu_column) == 104, "alpgpu_column keeps its layout");\n'
                   'int (*f0)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, const uint64_t*, const double*, const double*, uint32_t, double*, uint32_t*) = alpgpu_decode_group_sum_f64;\n'
                   'int (*f1)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, const uint64_t*, const float*, const float*, uint32_t, double*, uint32_t*) = alpgpu_decode_group_sum_f32;\n'
                   'size_t (*f2)(uint64_t, uint32_t) = alpgpu_group_totals_scratch_bytes;\n'
                   'int (*f3)(alpgpu_ctx*, const double*, const uint32_t*, uint64_t, uint32_t, double*, uint64_t*, void*) = alpgpu_group_totals;\n')
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_without_a_context_every_call_is_an_error_and_writes_nothing():
    from alp_amd import capi
    lib = capi.lib
    a, b = capi.CColumn(), capi.CColumn()
    a.n_vectors = b.n_vectors = 1
    mask = (ctypes.c_uint64 * 16)(*([7] * 16))
    sums = (ctypes.c_double * 2)(7.0, 7.0)
    counts = (ctypes.c_uint32 * 2)(7, 7)
    totals = (ctypes.c_double * 2)(7.0, 7.0)
    tcounts = (ctypes.c_uint64 * 2)(7, 7)
    lo, hi = (ctypes.c_double * 2)(0.0, 1.0), (ctypes.c_double * 2)(1.0, 2.0)
    flo, fhi = (ctypes.c_float * 2)(0.0, 1.0), (ctypes.c_float * 2)(1.0, 2.0)
    p = lambda t: ctypes.cast(t, ctypes.c_void_p)
    calls = [
        lambda: lib.alpgpu_decode_group_sum_f64(None, ctypes.byref(a), ctypes.byref(b), p(mask), p(lo), p(hi), 2, p(sums), p(counts)),
        lambda: lib.alpgpu_decode_group_sum_f32(None, ctypes.byref(a), ctypes.byref(b), p(mask), p(flo), p(fhi), 2, p(sums), p(counts)),
        lambda: lib.alpgpu_group_totals(None, p(sums), p(counts), 1, 2, p(totals), p(tcounts), None),
    ]
    for call in calls:
        assert call() == -2
        assert b"null context" in lib.alpgpu_last_error()
    assert list(mask) == [7] * 16 and list(sums) == [7.0, 7.0] and list(counts) == [7, 7] and list(totals) == [7.0, 7.0] and list(tcounts) == [7, 7]
    # the scratch size needs no device: two buffers of sums and two of counts, 8 bytes per group and block of 1024, a multiple of 16
    size = lib.alpgpu_group_totals_scratch_bytes
    assert size(0, 16) == 0 and size(1, 1) == 32 and size(1024, 16) == 512 and size(1025, 16) == 1024 and size(2**20, 3) == 3 * 32 * 1024


def hand_made():
    """two vectors of value = 1, 2, 3, ... (exact in double, every partial sum too) and hand-placed keys; everything else has key 100"""
    val = np.arange(1, 2049, dtype=np.float64).reshape(2, 1024)
    key = np.full((2, 1024), 100.0)
    bits = np.ones((2, 1024), dtype=bool)
    # vector 0: lane 0 holds positions 0, 64, 128; lane 3 holds 3 and 67
    key[0, 0], key[0, 64], key[0, 128] = 1.0, 2.0, 3.0   # values 1, 65, 129
    key[0, 3], key[0, 67] = 2.0, NAN                     # values 4, 68
    key[0, 5], key[0, 6] = 0.0, -0.0                     # values 6, 7
    key[0, 7] = 2.0                                      # value 8, its bit is cleared below
    bits[0, 7] = False
    # vector 1: one key on the shared boundary, one -inf
    key[1, 1023], key[1, 10] = 2.0, -INF                 # values 2048, 1035
    lo = [1.0, 2.0, 3.0, NAN, 0.0, -INF, 100.0]
    hi = [2.0, 3.0, 1.0, 5.0, 0.0, -INF, 100.0]
    return val, key, bits, lo, hi


def test_the_replica_on_a_hand_made_case():
    val, key, bits, lo, hi = hand_made()
    sums, counts = host_group_sums(val, key, bits, lo, hi)
    assert sums.shape == counts.shape == (7, 2) and sums.dtype == np.float64
    # group 0, [1, 2]: keys 1 and 2; the key 2.0 at value 65 and value 4 is on the boundary shared with group 1 and counts in both; value 8's bit is clear
    assert sums[0].tolist() == [1.0 + 65.0 + 4.0, 2048.0] and counts[0].tolist() == [3, 1]
    # group 1, [2, 3]
    assert sums[1].tolist() == [65.0 + 129.0 + 4.0, 2048.0] and counts[1].tolist() == [3, 1]
    # group 2, lo > hi, and group 3, a NaN bound: nothing, and +0.0 with the sign bit clear; the NaN key (value 68) is in no group at all
    assert sums[2:4].view(np.int64).tolist() == [[0, 0], [0, 0]] and counts[2:4].tolist() == [[0, 0], [0, 0]]
    # group 4, the point 0.0: -0.0 == 0.0
    assert sums[4].tolist() == [6.0 + 7.0, 0.0] and counts[4].tolist() == [2, 0]
    # group 5, the point -inf: an ordinary value
    assert sums[5].tolist() == [0.0, 1035.0] and counts[5].tolist() == [0, 1]
    # group 6: everything left at key 100
    rest0 = sum(range(1, 1025)) - (1 + 65 + 129 + 4 + 68 + 6 + 7 + 8)
    rest1 = sum(range(1025, 2049)) - (2048 + 1035)
    assert sums[6].tolist() == [float(rest0), float(rest1)] and counts[6].tolist() == [1024 - 8, 1024 - 2]
    assert int(counts.sum()) == 2048 - 2 + 3  # every value once, but for the NaN key and the clear bit; the three on the shared boundary twice
    totals, tcounts = host_group_totals(sums, counts)
    assert totals.tolist() == [70.0 + 2048.0, 198.0 + 2048.0, 0.0, 0.0, 13.0, 1035.0, float(rest0 + rest1)] and tcounts.tolist() == [4, 4, 0, 0, 2, 1, 2038]
    # float keys compare as floats: a bound that is no float rounds to one first, as the float entry point's bounds are floats
    kf = key.astype(np.float32)
    kf[0, 9] = np.float32(0.1)
    s32, c32 = host_group_sums(val.astype(np.float32), kf, bits, [0.1], [0.1])
    assert c32.tolist() == [[1, 0]] and s32.tolist() == [[10.0, 0.0]]
    # a selected NaN value makes the sum NaN, an unselected one does not
    val2 = val.copy()
    val2[0, 7] = NAN
    assert np.array_equal(host_group_sums(val2, key, bits, lo, hi)[0], sums)
    val2[0, 64] = NAN
    got = host_group_sums(val2, key, bits, lo, hi)[0]
    assert np.isnan(got[0, 0]) and np.isnan(got[1, 0]) and got[4, 0] == 13.0


def test_the_order_is_m_ascending_within_a_lane_then_the_adjacent_tree():
    val = np.zeros((1, 1024))
    key = np.zeros((1, 1024))
    bits = np.ones((1, 1024), dtype=bool)
    val[0, 5], val[0, 64 + 5], val[0, 128 + 5] = 1e16, 1.0, -1e16  # lane 5: (1e16 + 1) - 1e16 = 0, not 1
    val[0, 6] = 3.0                                                # lane 6 joins lane 7 first, then lanes 4..5
    key[0, 64 + 5] = 1.0
    sums, counts = host_group_sums(val, key, bits, [-1.0, 0.0, 1.0], [2.0, 0.0, 1.0])
    assert sums[:, 0].tolist() == [3.0, 3.0, 1.0] and counts[:, 0].tolist() == [1024, 1023, 1]  # group 1 skips the 1.0: 1e16 - 1e16 + 3


def test_the_replica_agrees_with_the_masked_sum_and_pair_replicas():
    from pair_replica import pairwise_tree
    from test_mask_gpu import host_column_total, host_sums_masked
    rng = np.random.default_rng(17)
    n = 7
    val = rng.normal(0, 1e6, (n, 1024)) * rng.choice([1e-9, 1.0, 1e9], (n, 1024))
    key = np.round(rng.uniform(0, 10, (n, 1024)), 1)
    key[rng.random((n, 1024)) < 0.01] = NAN
    val[rng.random((n, 1024)) < 0.001] = NAN
    bits = rng.random((n, 1024)) < 0.6
    bits[3] = False
    lo = [-INF, 0.0, 2.5, 2.5, 7.0, 9.0, NAN]
    hi = [INF, 2.5, 5.0, 2.5, 3.0, 9.0, 1.0]
    sums, counts = host_group_sums(val, key, bits, lo, hi)
    for g in range(len(lo)):
        both = bits & (key >= lo[g]) & (key <= hi[g])
        want = host_sums_masked(val, both)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(sums[g]), nan) and np.array_equal(sums[g].view(np.int64)[~nan], want.view(np.int64)[~nan]), g
        assert np.array_equal(counts[g], both.sum(axis=1))
    assert nan.sum() == 0 and np.isnan(sums[0]).any()  # (the NaN-bound group selects nothing; the open group meets NaN values)
    p = rng.normal(0, 1, (5, 64))
    assert np.array_equal(adjacent_tree(p), pairwise_tree(p))
    for width in (1, 1023, 1024, 1025, 2049):
        rows = rng.normal(0, 1e3, (3, width))
        totals, none = host_group_totals(rows)
        assert none is None and [t.view(np.int64) for t in totals] == [np.float64(host_column_total(r)).view(np.int64) for r in rows]
    totals, tcounts = host_group_totals(np.zeros((2, 0)), np.zeros((2, 0), dtype=np.uint32))
    assert totals.view(np.int64).tolist() == [0, 0] and tcounts.tolist() == [0, 0]
    big = np.full((1, 3), 2**32 - 1, dtype=np.uint32)
    assert host_group_totals(np.zeros((1, 3)), big)[1].tolist() == [3 * (2**32 - 1)]
