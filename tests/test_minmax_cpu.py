"""CPU: masked and grouped MIN / MAX (include/alpgpu.h, "masked and grouped MIN / MAX") is exported and declared, a NULL context is refused with
ALPGPU_ERR_INVALID before the HIP runtime is touched (ALPGPU_CHECK_CTX), so this runs without a device, and the host replica of the records
(tests/minmax_replica.py) is pinned on a hand-made case and against the grouped sum's replica."""
import ctypes
import os
import subprocess

import numpy as np

from group_replica import host_group_sums
from minmax_replica import host_group_minmax, host_minmax_masked, host_minmax_totals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_decode_minmax_masked_f64", "alpgpu_decode_minmax_masked_f32", "alpgpu_decode_group_minmax_f64", "alpgpu_decode_group_minmax_f32",
         "alpgpu_group_minmax_totals_f64", "alpgpu_group_minmax_totals_f32")
NAN, INF = float("nan"), float("inf")


def test_library_exports_the_minmax_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols
    for m in ("decode_minmax_masked", "decode_group_minmax", "group_minmax_totals"):
        assert callable(getattr(capi.Context, m))


def test_the_header_declares_them(tmp_path):
    src = tmp_path / "minmax_decls.c"
    src.write_text('#include "alpgpu.h"\n'
                   '_Static_assert(sizeof(alpgpu_zone_f64) == 16 && sizeof(alpgpu_zone_f32) == 8, "the records are those of the zone maps");\n'
                   '_Static_assert(sizeof(alpgpu_column) == 104, "alpgpu_column keeps its layout");\n'
                   'int (*f0)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, alpgpu_zone_f64*, uint32_t*) = alpgpu_decode_minmax_masked_f64;\n'
                   'int (*f1)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, alpgpu_zone_f32*, uint32_t*) = alpgpu_decode_minmax_masked_f32;\n'
                   'int (*f2)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, const uint64_t*, const double*, const double*, uint32_t, alpgpu_zone_f64*, uint32_t*) = alpgpu_decode_group_minmax_f64;\n'
                   'int (*f3)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, const uint64_t*, const float*, const float*, uint32_t, alpgpu_zone_f32*, uint32_t*) = alpgpu_decode_group_minmax_f32;\n'
                   'int (*f4)(alpgpu_ctx*, const alpgpu_zone_f64*, uint64_t, uint32_t, double*) = alpgpu_group_minmax_totals_f64;\n'
                   'int (*f5)(alpgpu_ctx*, const alpgpu_zone_f32*, uint64_t, uint32_t, float*) = alpgpu_group_minmax_totals_f32;\n')
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_without_a_context_every_call_is_an_error_and_writes_nothing():
    from alp_amd import capi
    lib = capi.lib
    a, b = capi.CColumn(), capi.CColumn()
    a.n_vectors = b.n_vectors = 1
    mask = (ctypes.c_uint64 * 16)(*([7] * 16))
    zones = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    counts = (ctypes.c_uint32 * 2)(7, 7)
    totals = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    lo, hi = (ctypes.c_double * 2)(0.0, 1.0), (ctypes.c_double * 2)(1.0, 2.0)
    flo, fhi = (ctypes.c_float * 2)(0.0, 1.0), (ctypes.c_float * 2)(1.0, 2.0)
    p = lambda t: ctypes.cast(t, ctypes.c_void_p)
    calls = [
        lambda: lib.alpgpu_decode_minmax_masked_f64(None, ctypes.byref(a), p(mask), p(zones), p(counts)),
        lambda: lib.alpgpu_decode_minmax_masked_f32(None, ctypes.byref(a), p(mask), p(zones), p(counts)),
        lambda: lib.alpgpu_decode_group_minmax_f64(None, ctypes.byref(a), ctypes.byref(b), p(mask), p(lo), p(hi), 2, p(zones), p(counts)),
        lambda: lib.alpgpu_decode_group_minmax_f32(None, ctypes.byref(a), ctypes.byref(b), p(mask), p(flo), p(fhi), 2, p(zones), p(counts)),
        lambda: lib.alpgpu_group_minmax_totals_f64(None, p(zones), 1, 2, p(totals)),
        lambda: lib.alpgpu_group_minmax_totals_f32(None, p(zones), 1, 2, p(totals)),
    ]
    for call in calls:
        assert call() == -2
        assert b"null context" in lib.alpgpu_last_error()
    assert list(mask) == [7] * 16 and list(zones) == [7.0] * 4 and list(counts) == [7, 7] and list(totals) == [7.0] * 4


def bits_of(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64 if x.dtype == np.float64 else np.int32).tolist()


def rec(mn, mx, dtype=np.float64):
    return bits_of(np.array([mn, mx], dtype=dtype))


def hand_made():
    """two vectors of value = 1, 2, 3, ... with hand-placed specials and keys; every other key is 100"""
    val = np.arange(1, 2049, dtype=np.float64).reshape(2, 1024)
    key = np.full((2, 1024), 100.0)
    bits = np.ones((2, 1024), dtype=bool)
    # vector 0.  Lane 5 holds both zeros (positions 5 and 64 + 5), in different groups
    val[0, 5], val[0, 69] = -0.0, 0.0
    key[0, 5], key[0, 69] = 1.0, 2.0
    val[0, 9], key[0, 9] = NAN, 2.0      # a selected NaN beside ordinary values
    val[0, 20], key[0, 20] = -5.0, 1.0   # the true minimum: its bit is cleared
    bits[0, 20] = False
    val[0, 30], key[0, 30] = INF, 3.0
    key[0, 0] = 2.0                      # value 1.0, on the boundary groups 0 and 1 share
    key[0, 1] = NAN                      # value 2.0: in no group
    key[0, 2], key[0, 3] = -0.0, 0.0     # values 3.0 and 4.0: the point 0.0 takes both
    # vector 1: the only selected values are NaN
    bits[1] = False
    bits[1, 3] = bits[1, 4] = True
    val[1, 3] = val[1, 4] = NAN
    val[1, 100] = -INF
    lo = [1.0, 2.0, 3.0, NAN, 0.0, 100.0, -INF]
    hi = [2.0, 3.0, 1.0, 5.0, 0.0, 100.0, INF]
    return val, key, bits, lo, hi


def test_the_replica_on_a_hand_made_case():
    val, key, bits, lo, hi = hand_made()
    empty = rec(INF, -INF)
    zones, counts = host_minmax_masked(val, bits)
    assert zones.shape == (2, 2) and zones.dtype == np.float64 and counts.tolist() == [1023, 2]
    # vector 0: -5.0 is not selected, so the minimum is -0.0 (sign bit set, below the +0.0 of the same lane); the NaN is counted and ignored
    assert bits_of(zones[0]) == rec(-0.0, INF) and bits_of(zones[0])[0] < 0
    # vector 1: two selected values, both NaN
    assert bits_of(zones[1]) == empty
    full, cfull = host_minmax_masked(val, np.ones_like(bits))
    assert bits_of(full[0]) == rec(-5.0, INF) and bits_of(full[1]) == rec(-INF, 2048.0) and cfull.tolist() == [1024, 1024]
    gz, gc = host_group_minmax(val, key, bits, lo, hi)
    assert gz.shape == (7, 2, 2) and gc.shape == (7, 2) and gz.dtype == np.float64
    # group 0, [1, 2]: -0.0, +0.0, the NaN and 1.0 (on the shared boundary); -5.0 has key 1.0 but a clear bit
    assert bits_of(gz[0, 0]) == rec(-0.0, 1.0) and gc[0].tolist() == [4, 0]
    # group 1, [2, 3]: +0.0 selected while -0.0 is not: the minimum is +0.0, sign bit clear
    assert bits_of(gz[1, 0]) == rec(0.0, INF) and bits_of(gz[1, 0])[0] == 0 and gc[1].tolist() == [4, 0]
    # group 2, lo > hi, and group 3, a NaN bound: nothing
    assert [bits_of(gz[g, v]) for g in (2, 3) for v in (0, 1)] == [empty] * 4 and gc[2:4].tolist() == [[0, 0], [0, 0]]
    # group 4, the point 0.0: the keys -0.0 and 0.0
    assert bits_of(gz[4, 0]) == rec(3.0, 4.0) and gc[4].tolist() == [2, 0]
    # group 5: everything left at key 100; vector 1 selects two NaNs there
    assert bits_of(gz[5, 0]) == rec(5.0, 1024.0) and bits_of(gz[5, 1]) == empty and gc[5].tolist() == [1024 - 9, 2]
    # group 6, everything: but for the NaN key and the clear bit
    assert bits_of(gz[6, 0]) == rec(-0.0, INF) and gc[6].tolist() == [1022, 2]
    assert [bits_of(gz[g, 1]) for g in range(7)] == [empty] * 7
    totals = host_minmax_totals(gz)
    assert totals.shape == (7, 2)
    assert [bits_of(t) for t in totals] == [rec(-0.0, 1.0), rec(0.0, INF), empty, empty, rec(3.0, 4.0), rec(5.0, 1024.0), rec(-0.0, INF)]
    assert [bits_of(t) for t in host_minmax_totals(np.empty((3, 0, 2)))] == [empty] * 3
    # floats stay floats, and a float key compares as a float
    kf = key.astype(np.float32)
    kf[0, 11] = np.float32(0.1)
    z32, c32 = host_group_minmax(val.astype(np.float32), kf, bits, [0.1], [0.1])
    assert z32.dtype == np.float32 and bits_of(z32[0, 0]) == rec(12.0, 12.0, np.float32) and c32.tolist() == [[1, 0]]
    assert bits_of(host_minmax_totals(z32)[0]) == rec(12.0, 12.0, np.float32)
    # a signalling NaN is a NaN
    snan = np.array([0x7FF0000000000001], dtype=np.int64).view(np.float64)[0]
    val2 = val.copy()
    val2[0, 40] = snan
    assert bits_of(host_minmax_masked(val2, bits)[0]) == bits_of(zones)


def test_every_row_is_the_masked_replica_under_the_anded_bitmap_and_counts_are_the_group_sums():
    rng = np.random.default_rng(19)
    n = 6
    for dtype in (np.float64, np.float32):
        val = (rng.normal(0, 1e6, (n, 1024)) * rng.choice([1e-9, 1.0, 1e9], (n, 1024))).astype(dtype)
        key = np.round(rng.uniform(0, 10, (n, 1024)), 1).astype(dtype)
        key[rng.random((n, 1024)) < 0.01] = NAN
        val[rng.random((n, 1024)) < 0.01] = NAN
        val[rng.random((n, 1024)) < 0.01] = -0.0
        bits = rng.random((n, 1024)) < 0.6
        bits[3] = False
        lo = [-INF, 0.0, 2.5, 2.5, 7.0, 9.0, NAN]
        hi = [INF, 2.5, 5.0, 2.5, 3.0, 9.0, 1.0]
        zones, counts = host_group_minmax(val, key, bits, lo, hi)
        want_counts = host_group_sums(val, key, bits, lo, hi)[1]
        assert np.array_equal(counts, want_counts)
        with np.errstate(invalid="ignore"):
            for g in range(len(lo)):
                both = bits & (key >= dtype(lo[g])) & (key <= dtype(hi[g]))
                want, c = host_minmax_masked(val, both)
                assert bits_of(zones[g]) == bits_of(want) and np.array_equal(counts[g], c), g
        assert counts[4].sum() == 0 and counts[6].sum() == 0 and 0 < counts[2].sum() < counts[0].sum()
        # against numpy's own NaN-ignoring reductions where the zeros' signs cannot matter
        sel = np.where(bits & ~np.isnan(key), val, NAN)[[0, 1, 2, 4, 5]]
        with np.errstate(all="ignore"):
            assert np.array_equal(zones[0][[0, 1, 2, 4, 5], 0], np.nanmin(sel, axis=1)) and np.array_equal(zones[0][[0, 1, 2, 4, 5], 1], np.nanmax(sel, axis=1))
