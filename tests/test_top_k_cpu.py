"""CPU: top-k (include/alpgpu.h, "top-k") is exported and declared, a NULL context is refused with ALPGPU_ERR_INVALID before the HIP runtime is touched
(ALPGPU_CHECK_CTX), so this runs without a device, alpgpu_top_k_scratch_bytes behaves as documented, and the host replica of the order
(tests/top_k_replica.py) is pinned on a hand-made vector."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from top_k_replica import host_top_k, is_nan_bits, okey

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_top_k_scratch_bytes", "alpgpu_top_k_f64", "alpgpu_top_k_f32")
NAN, INF = float("nan"), float("inf")
UINT64_MAX = 2**64 - 1


def test_library_exports_the_top_k_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols
    for m in ("top_k_scratch", "top_k_into", "top_k"):
        assert callable(getattr(capi.Context, m))
    assert capi.TOP_K_MAX == 1024


def test_the_header_declares_them(tmp_path):
    src = tmp_path / "top_k_decls.c"
    src.write_text('#include "alpgpu.h"\n'
                   '_Static_assert(ALPGPU_TOP_K_MAX == 1024, "the documented bound");\n'
                   '_Static_assert(sizeof(alpgpu_zone_f64) == 16 && sizeof(alpgpu_zone_f32) == 8, "the records are those of the zone maps");\n'
                   '_Static_assert(sizeof(alpgpu_column) == 104, "alpgpu_column keeps its layout");\n'
                   'uint64_t (*f0)(uint64_t, uint64_t) = alpgpu_top_k_scratch_bytes;\n'
                   'int (*f1)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_f64*, uint64_t, int, double*, int64_t*, uint64_t*, void*) = alpgpu_top_k_f64;\n'
                   'int (*f2)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_f32*, uint64_t, int, float*, int64_t*, uint64_t*, void*) = alpgpu_top_k_f32;\n')
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_without_a_context_every_call_is_an_error_and_writes_nothing():
    from alp_amd import capi
    lib = capi.lib
    a = capi.CColumn()
    a.n_vectors = 1
    mask = (ctypes.c_uint64 * 16)(*([7] * 16))
    vals = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    idx = (ctypes.c_int64 * 4)(7, 7, 7, 7)
    count = (ctypes.c_uint64 * 1)(7)
    scratch = (ctypes.c_uint64 * 64)(*([7] * 64))
    p = lambda t: ctypes.cast(t, ctypes.c_void_p)
    for name in ("alpgpu_top_k_f64", "alpgpu_top_k_f32"):
        assert getattr(lib, name)(None, ctypes.byref(a), p(mask), None, 4, 1, p(vals), p(idx), p(count), p(scratch)) == -2
        assert b"null context" in lib.alpgpu_last_error()
    assert list(mask) == [7] * 16 and list(vals) == [7.0] * 4 and list(idx) == [7] * 4 and list(count) == [7] and list(scratch) == [7] * 64


def test_scratch_bytes_is_monotone_never_zero_and_refuses_what_the_call_refuses():
    from alp_amd import capi
    sb = capi.lib.alpgpu_top_k_scratch_bytes
    ns = (0, 1, 2, 5, 1023, 1024, 1025, 4096, 1 << 20, (1 << 32) - 1)
    ks = (0, 1, 2, 63, 64, 65, 1000, 1023, 1024)
    table = [[sb(n, k) for k in ks] for n in ns]
    for row in table:
        assert all(0 < b < UINT64_MAX and b % 16 == 0 for b in row)
        assert all(a <= b for a, b in zip(row, row[1:])), "monotone in k"
    for r0, r1 in zip(table, table[1:]):
        assert all(a <= b for a, b in zip(r0, r1)), "monotone in n_vectors"
    assert sb(0, 0) > 0
    # what it covers: 20 bytes per vector of records and counts, min(k, n_vectors) * 1024 candidates of 16 bytes, and the fixed part
    fixed = sb(0, 0)
    assert sb(4096, 100) >= fixed + 20 * 4096 + 100 * 1024 * 16
    assert sb(5, 1024) >= fixed + 20 * 5 + 5 * 1024 * 16 and sb(5, 1024) < fixed + 20 * 5 + 6 * 1024 * 16
    assert sb(1 << 20, 1024) < fixed + 32 * (1 << 20) + 1024 * 1024 * 16
    for n in (0, 1, 1 << 20):
        assert sb(n, 1025) == UINT64_MAX and sb(n, UINT64_MAX) == UINT64_MAX
    for n in (1 << 32, 1 << 60, UINT64_MAX):  # more vectors than the call accepts, and sizes that would overflow
        assert sb(n, 1) == UINT64_MAX


def special_vector(dtype):
    """a hand-made vector: both zeros, NaNs of both kinds and both signs, +-inf, 1-ulp neighbours, three equal values at scattered indices"""
    u = np.uint64 if dtype == np.float64 else np.uint32
    qnan, snan = (0x7FF8000000000000, 0x7FF0000000000001) if dtype == np.float64 else (0x7FC00000, 0x7F800001)
    sign = 1 << (63 if dtype == np.float64 else 31)
    x = np.linspace(-500.0, 500.0, 1024).astype(dtype)  # distinct, ascending, no zero among them
    assert not (x == 0).any() and np.unique(x).size == 1024
    x[10], x[700] = 0.0, -0.0
    x[20], x[21] = np.array([qnan, snan], dtype=u).view(dtype)
    x[22], x[23] = np.array([qnan | sign, snan | sign], dtype=u).view(dtype)
    x[30], x[31] = INF, -INF
    x[40] = dtype(1000.0)
    x[41], x[42] = np.nextafter(dtype(1000.0), dtype(INF)), np.nextafter(dtype(1000.0), dtype(-INF))
    x[900] = x[50] = x[333] = dtype(777.25)  # three equal values at scattered indices
    x[60] = dtype(-1000.0)
    x[61], x[62] = np.nextafter(dtype(-1000.0), dtype(INF)), np.nextafter(dtype(-1000.0), dtype(-INF))
    return x


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_replica_on_a_hand_made_vector(dtype):
    x = special_vector(dtype)
    full = np.ones(1024, bool)
    assert is_nan_bits(x).sum() == 4 and np.array_equal(is_nan_bits(x), np.isnan(x))
    # okey is monotone on what is no NaN: sorting by it is sorting by value, the zeros apart
    ok = ~np.isnan(x)
    by_key = x[ok][np.argsort(okey(x[ok]), kind="stable")]
    assert np.array_equal(by_key, np.sort(x[ok])) and okey(np.array([-0.0], dtype))[0] < okey(np.array([0.0], dtype))[0]
    assert okey(x).dtype.itemsize == x.dtype.itemsize
    # the largest: +inf, the three neighbours of 1000 in order, then 777.25 three times by ascending index
    v, i = host_top_k(x, full, 7, largest=True)
    assert i.tolist() == [30, 41, 40, 42, 50, 333, 900] and v.dtype == dtype
    assert v.tolist() == [INF, float(x[41]), 1000.0, float(x[42]), 777.25, 777.25, 777.25]
    # the smallest: -inf, the neighbours of -1000, then the ramp
    v, i = host_top_k(x, full, 5, largest=False)
    assert i.tolist() == [31, 62, 60, 61, 0] and v[0] == -INF and v[1] < v[2] < v[3] < v[4]
    # the zeros: -0.0 lies below +0.0, whatever their indices, and each keeps its sign
    zeros = np.zeros(1024, bool)
    zeros[[10, 700]] = True
    v, i = host_top_k(x, zeros, 2, largest=True)
    assert i.tolist() == [10, 700] and np.signbit(v).tolist() == [False, True]
    v, i = host_top_k(x, zeros, 2, largest=False)
    assert i.tolist() == [700, 10] and np.signbit(v).tolist() == [True, False]
    # NaNs are never returned: a selection of nothing else is empty, and k beyond what there is gives what there is
    nans = np.zeros(1024, bool)
    nans[[20, 21, 22, 23]] = True
    for largest in (True, False):
        v, i = host_top_k(x, nans, 10, largest)
        assert v.size == 0 and i.size == 0
        v, i = host_top_k(x, full, 2000, largest)
        assert v.size == 1020 and not np.isnan(v).any() and np.unique(i).size == 1020
        assert (np.diff(okey(v).astype(object)) <= 0).all() if largest else (np.diff(okey(v).astype(object)) >= 0).all()
        assert host_top_k(x, full, 0, largest)[0].size == 0
    # the three equal values alone, both directions: ascending index either way
    same = np.zeros(1024, bool)
    same[[900, 50, 333]] = True
    for largest in (True, False):
        assert host_top_k(x, same, 3, largest)[1].tolist() == [50, 333, 900]
        assert host_top_k(x, same, 2, largest)[1].tolist() == [50, 333]
    # an unselected value does not appear: without +inf's bit the neighbour above 1000 leads
    no_inf = full.copy()
    no_inf[30] = False
    assert host_top_k(x, no_inf, 1)[1].tolist() == [41]
