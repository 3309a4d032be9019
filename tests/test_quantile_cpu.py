"""CPU: the quantiles (include/alpgpu.h, "quantiles") are exported and declared, a NULL context is refused with ALPGPU_ERR_INVALID before the HIP
runtime is touched (ALPGPU_CHECK_CTX), so this runs without a device, alpgpu_quantile_scratch_bytes behaves as documented, and the host replica
(tests/quantile_replica.py) is pinned on a hand-made vector and against numpy's method="lower"."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from quantile_replica import host_quantile, host_select_rank, quantile_ranks, sorted_selection

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_quantile_scratch_bytes", "alpgpu_select_rank_f64", "alpgpu_select_rank_f32", "alpgpu_quantile_f64", "alpgpu_quantile_f32", "alpgpu_debug_quantile_f64",
         "alpgpu_debug_quantile_f32", "alpgpu_debug_quantile_trace")
NAN, INF = float("nan"), float("inf")
UINT64_MAX = 2**64 - 1


def test_library_exports_the_quantile_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols
    for m in ("quantile_scratch", "select_rank_into", "quantile_into", "select_rank", "quantile", "quantile_trace"):
        assert callable(getattr(capi.Context, m))
    assert capi.RANK_MAX == 32 and capi.QUANTILE_MAX == 16
    assert ctypes.sizeof(capi.QuantileTuning) == 16 and ctypes.sizeof(capi.QuantileTrace) == 104


def test_the_header_declares_them(tmp_path):
    src = tmp_path / "quantile_decls.c"
    src.write_text('#include "alpgpu.h"\n'
                   '_Static_assert(ALPGPU_RANK_MAX == 32 && ALPGPU_QUANTILE_MAX == 16, "the documented bounds");\n'
                   '_Static_assert(sizeof(alpgpu_quantile_tuning) == 16 && sizeof(alpgpu_quantile_trace) == 104, "the debug records");\n'
                   '_Static_assert(sizeof(alpgpu_column) == 104, "alpgpu_column keeps its layout");\n'
                   'uint64_t (*f0)(uint64_t) = alpgpu_quantile_scratch_bytes;\n'
                   'int (*f1)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_f64*, const uint64_t*, uint32_t, int, double*, uint64_t*, void*) = alpgpu_select_rank_f64;\n'
                   'int (*f2)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_f32*, const uint64_t*, uint32_t, int, float*, uint64_t*, void*) = alpgpu_select_rank_f32;\n'
                   'int (*f3)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_f64*, const double*, uint32_t, double*, uint64_t*, uint64_t*, void*) = alpgpu_quantile_f64;\n'
                   'int (*f4)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_f32*, const double*, uint32_t, float*, uint64_t*, uint64_t*, void*) = alpgpu_quantile_f32;\n'
                   'int (*f5)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_f64*, const uint64_t*, uint32_t, int, double*, uint64_t*, void*,\n'
                   '          const alpgpu_quantile_tuning*) = alpgpu_debug_quantile_f64;\n'
                   'int (*f6)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_f32*, const uint64_t*, uint32_t, int, float*, uint64_t*, void*,\n'
                   '          const alpgpu_quantile_tuning*) = alpgpu_debug_quantile_f32;\n'
                   'int (*f7)(alpgpu_ctx*, const void*, alpgpu_quantile_trace*) = alpgpu_debug_quantile_trace;\n')
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_without_a_context_every_call_is_an_error_and_writes_nothing():
    from alp_amd import capi
    lib = capi.lib
    a = capi.CColumn()
    a.n_vectors = 1
    mask = (ctypes.c_uint64 * 16)(*([7] * 16))
    vals = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    out_ranks = (ctypes.c_uint64 * 2)(7, 7)
    count = (ctypes.c_uint64 * 1)(7)
    scratch = (ctypes.c_uint64 * 64)(*([7] * 64))
    ranks = (ctypes.c_uint64 * 2)(0, 1)
    q = (ctypes.c_double * 2)(0.25, 0.5)
    trace = capi.QuantileTrace()
    p = lambda t: ctypes.cast(t, ctypes.c_void_p)
    for t in ("f64", "f32"):
        assert getattr(lib, "alpgpu_select_rank_" + t)(None, ctypes.byref(a), p(mask), None, p(ranks), 2, 0, p(vals), p(count), p(scratch)) == -2
        assert b"null context" in lib.alpgpu_last_error()
        assert getattr(lib, "alpgpu_quantile_" + t)(None, ctypes.byref(a), p(mask), None, p(q), 2, p(vals), p(out_ranks), p(count), p(scratch)) == -2
        assert b"null context" in lib.alpgpu_last_error()
        assert getattr(lib, "alpgpu_debug_quantile_" + t)(None, ctypes.byref(a), p(mask), None, p(ranks), 2, 0, p(vals), p(count), p(scratch), None) == -2
        assert b"null context" in lib.alpgpu_last_error()
    assert lib.alpgpu_debug_quantile_trace(None, p(scratch), ctypes.byref(trace)) == -2
    assert list(mask) == [7] * 16 and list(vals) == [7.0] * 4 and list(out_ranks) == [7, 7] and list(count) == [7] and list(scratch) == [7] * 64
    assert list(ranks) == [0, 1] and list(q) == [0.25, 0.5] and trace.n == 0 and trace.compact_pass == 0


def test_scratch_bytes_is_monotone_never_zero_and_refuses_what_the_call_refuses():
    from alp_amd import capi
    sb = capi.lib.alpgpu_quantile_scratch_bytes
    ns = (0, 1, 2, 5, 1023, 1024, 1025, 4095, 4096, 4097, 1 << 20, (1 << 32) - 1)
    row = [sb(n) for n in ns]
    assert all(0 < b < UINT64_MAX and b % 16 == 0 for b in row)
    assert all(a <= b for a, b in zip(row, row[1:])), "monotone in n_vectors"
    # what it covers: max(65536, 16 * n_vectors) candidate keys of 8 bytes and the fixed part (the state, 8 passes of 32 x 256 64-bit bins)
    fixed = sb(0) - 8 * 65536
    assert fixed >= 8 * 32 * 256 * 8
    assert sb(4096) == sb(0) and sb(4097) == fixed + 8 * 16 * 4097 and sb(1 << 20) == fixed + 8 * 16 * (1 << 20)
    for n in (1 << 32, 1 << 60, UINT64_MAX):  # more vectors than the call accepts, and sizes that would overflow
        assert sb(n) == UINT64_MAX


def bits_of(v):
    v = np.ascontiguousarray(v)
    return v.view(np.uint64 if v.dtype == np.float64 else np.uint32).tolist()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_replica_on_a_hand_made_vector(dtype):
    """+-0.0, +-inf, denormals of both signs, NaNs quiet and signalling of both signs: rank -> bits, spelled out"""
    f64 = dtype == np.float64
    u = np.uint64 if f64 else np.uint32
    sign = 1 << (63 if f64 else 31)
    qnan, snan = (0x7FF8000000000000, 0x7FF0000000000001) if f64 else (0x7FC00000, 0x7F800001)
    pinf = 0x7FF0000000000000 if f64 else 0x7F800000
    one, two = (0x3FF0000000000000, 0x4000000000000000) if f64 else (0x3F800000, 0x40000000)
    pattern = [one, qnan, 0, sign, pinf, snan, pinf | sign, 1, 1 | sign, qnan | sign, two | sign, 3, snan | sign, one, one | sign]
    x = np.array(pattern, dtype=u).view(dtype)
    full = np.ones(x.size, bool)
    s = sorted_selection(x, full)
    # ascending: -inf, -2.0, -1.0, the negative denormal, -0.0, +0.0, the denormals 1 and 3 ulp, 1.0 twice, +inf
    want = [pinf | sign, two | sign, one | sign, 1 | sign, sign, 0, 1, 3, one, one, pinf]
    assert bits_of(s) == want and s.dtype == dtype
    v, n = host_select_rank(s, [0, 4, 5, 10, 11, 2**63, 8, 8])
    assert n == 11 and bits_of(v) == [want[0], sign, 0, pinf, pinf, pinf, one, one]  # ranks at and beyond N clamp to the last; repeats repeat
    v, n = host_select_rank(s, [0, 1, 10, 500], from_top=True)
    assert n == 11 and bits_of(v) == [pinf, one, pinf | sign, pinf | sign]
    pairs, r, n = host_quantile(s, [0.0, 0.5, 1.0, 0.45, 0.99])
    assert n == 11 and r.tolist() == [0, 5, 10, 4, 9]
    assert bits_of(pairs.reshape(-1)) == [want[0], want[1], 0, 1, pinf, pinf, sign, 0, one, pinf]  # the median is +0.0, its lower neighbour at 0.45 is -0.0
    # an unselected value does not count, NaNs never do
    sel = full.copy()
    sel[[4, 6]] = False  # without the infinities
    s2 = sorted_selection(x, sel)
    assert bits_of(s2) == want[1:-1]
    nans = np.zeros(x.size, bool)
    nans[[1, 5, 9, 12]] = True
    s3 = sorted_selection(x, nans)
    assert s3.size == 0 and host_select_rank(s3, [0, 1])[1] == 0 and host_select_rank(s3, [0])[0].size == 0
    pairs, r, n = host_quantile(s3, [0.5])
    assert n == 0 and pairs.shape == (0, 2) and r.size == 0
    nans[[0, 10]] = True  # NaNs and two numbers
    v, n = host_select_rank(sorted_selection(x, nans), [0, 1, 2])
    assert n == 2 and bits_of(v) == [two | sign, one, one]


def test_the_rank_rule_is_numpys_method_lower():
    rng = np.random.default_rng(2006)
    for trial in range(600):
        n = int(rng.integers(1, 5000))
        x = rng.normal(0, 100, n)
        q = np.concatenate([rng.random(3), rng.integers(0, 101, 3) / 100.0, [0.0, 1.0]])
        s = sorted_selection(x, np.ones(n, bool))
        pairs, r, cnt = host_quantile(s, q)
        assert cnt == n and np.array_equal(r, quantile_ranks(q, n))
        assert np.array_equal(pairs[:, 0], np.quantile(x, q, method="lower")), (n, q)
        assert np.array_equal(pairs[:, 1], s[np.minimum(r + 1, n - 1)])
