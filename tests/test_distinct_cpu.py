"""CPU: the distinct values (include/alpgpu.h, "distinct values") are exported and declared, a NULL context is refused with ALPGPU_ERR_INVALID before
the HIP runtime is touched (ALPGPU_CHECK_CTX), so this runs without a device, the scratch formula keeps its promises, and the host replica
(tests/distinct_replica.py) is pinned on a hand-made case, spelled out.  The first four tests need the feature (the symbols, the header's section,
the wrappers); the replica's test needs only numpy: it pins the yardstick every GPU expectation goes through."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from distinct_replica import host_distinct, is_nan_bits, unpack_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_distinct_f64", "alpgpu_distinct_f32", "alpgpu_debug_distinct_f64", "alpgpu_debug_distinct_f32", "alpgpu_distinct_scratch_bytes")
NAN, INF = float("nan"), float("inf")
U64_MAX = 2**64 - 1


def test_library_exports_the_distinct_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols
    for m in ("distinct", "distinct_into", "distinct_scratch"):
        assert callable(getattr(capi.Context, m))
    assert capi.DISTINCT_MAX == 1 << 20
    assert ctypes.sizeof(capi.DistinctTuning) == 24
    assert [f[0] for f in capi.DistinctTuning._fields_] == ["grid", "flush_every", "lds_slots", "table_slots", "sort_tile", "reserved"]


def test_the_header_declares_them(tmp_path):
    src = tmp_path / "distinct_decls.c"
    src.write_text('#include "alpgpu.h"\n'
                   '_Static_assert(ALPGPU_DISTINCT_MAX == (1u << 20), "the documented bound");\n'
                   '_Static_assert(sizeof(alpgpu_distinct_tuning) == 24, "the debug record");\n'
                   '_Static_assert(sizeof(alpgpu_column) == 104, "alpgpu_column keeps its layout");\n'
                   'uint64_t (*s0)(uint64_t) = alpgpu_distinct_scratch_bytes;\n'
                   'int (*f0)(alpgpu_ctx*, const alpgpu_column*, uint64_t, uint64_t, const uint64_t*, const alpgpu_zone_f64*, uint64_t, double*, uint64_t*, uint64_t*, void*) = alpgpu_distinct_f64;\n'
                   'int (*f1)(alpgpu_ctx*, const alpgpu_column*, uint64_t, uint64_t, const uint64_t*, const alpgpu_zone_f32*, uint64_t, float*, uint64_t*, uint64_t*, void*) = alpgpu_distinct_f32;\n'
                   'int (*f2)(alpgpu_ctx*, const alpgpu_column*, uint64_t, uint64_t, const uint64_t*, const alpgpu_zone_f64*, uint64_t, double*, uint64_t*, uint64_t*, void*,\n'
                   '          const alpgpu_distinct_tuning*, uint64_t*) = alpgpu_debug_distinct_f64;\n'
                   'int (*f3)(alpgpu_ctx*, const alpgpu_column*, uint64_t, uint64_t, const uint64_t*, const alpgpu_zone_f32*, uint64_t, float*, uint64_t*, uint64_t*, void*,\n'
                   '          const alpgpu_distinct_tuning*, uint64_t*) = alpgpu_debug_distinct_f32;\n')
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_without_a_context_every_call_is_an_error_and_writes_nothing():
    from alp_amd import capi
    lib = capi.lib
    a = capi.CColumn()
    a.n_vectors = 1
    mask = (ctypes.c_uint64 * 16)(*([7] * 16))
    vals = (ctypes.c_double * 8)(*([7.0] * 8))
    counts = (ctypes.c_uint64 * 8)(*([7] * 8))
    state = (ctypes.c_uint64 * 4)(*([7] * 4))
    scratch = (ctypes.c_uint64 * 64)(*([7] * 64))
    trace = (ctypes.c_uint64 * 6)(*([7] * 6))
    tuning = capi.DistinctTuning(1, 1, 64, 8, 64, 0)
    p = lambda t: ctypes.cast(t, ctypes.c_void_p)
    for t in ("f64", "f32"):
        assert getattr(lib, "alpgpu_distinct_" + t)(None, ctypes.byref(a), 0, 1024, p(mask), None, 8, p(vals), p(counts), p(state), p(scratch)) == -2
        assert b"null context" in lib.alpgpu_last_error()
        assert getattr(lib, "alpgpu_debug_distinct_" + t)(None, ctypes.byref(a), 0, 1024, p(mask), None, 8, p(vals), p(counts), p(state), p(scratch), ctypes.byref(tuning), p(trace)) == -2
        assert b"null context" in lib.alpgpu_last_error()
    assert list(mask) == [7] * 16 and list(vals) == [7.0] * 8 and list(counts) == [7] * 8 and list(state) == [7] * 4 and list(scratch) == [7] * 64 and list(trace) == [7] * 6


def test_the_scratch_formula():
    from alp_amd import capi
    f = capi.lib.alpgpu_distinct_scratch_bytes
    assert f(0) == U64_MAX and f(capi.DISTINCT_MAX + 1) == U64_MAX and f(2**32) == U64_MAX and f(U64_MAX) == U64_MAX
    last = 0
    for c in list(range(1, 300)) + [2**k + d for k in range(9, 21) for d in (-1, 0, 1) if 2**k + d <= capi.DISTINCT_MAX]:
        b = f(c)
        assert 0 < b < U64_MAX and b % 16 == 0 and b >= last, c
        p = 1
        while p < c:
            p *= 2
        assert b == 64 + 16 * (2 * p) + 16 * p, "the documented formula: the state, T = 2 P keys and counts, P pairs"
        last = b
    assert f(capi.DISTINCT_MAX) == 64 + 48 * 2**20


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_replica_on_a_hand_made_case(dtype):
    """a dozen values: both zeros, +-inf, a NaN, repeats; then a selection and an empty selection"""
    x = np.array([2.5, -0.0, INF, 0.0, NAN, -INF, 2.5, -1.5, 2.5, INF, 7.0, -0.0], dtype=dtype)
    assert x.size == 12 and np.signbit(x[1]) and not np.signbit(x[3])
    values, counts, n_nan, n_numbers = host_distinct(x)
    assert values.dtype == dtype and counts.dtype == np.uint64
    assert values.tolist() == [-INF, -1.5, 0.0, 2.5, 7.0, INF] and not np.signbit(values[2]), "the zeros are one value, +0.0; the infinities are ordinary"
    assert counts.tolist() == [1, 1, 3, 3, 1, 2]
    assert (n_nan, n_numbers) == (1, 11) and int(counts.sum()) == n_numbers
    # a selection: without the first 2.5, the +0.0, the NaN and the last value
    sel = np.ones(12, bool)
    sel[[0, 3, 4, 11]] = False
    values, counts, n_nan, n_numbers = host_distinct(x, sel)
    assert values.tolist() == [-INF, -1.5, 0.0, 2.5, 7.0, INF] and not np.signbit(values[2]), "the one zero left is -0.0 and is reported as +0.0"
    assert counts.tolist() == [1, 1, 1, 2, 1, 2] and (n_nan, n_numbers) == (0, 8)
    # only the NaN; nothing
    only = np.zeros(12, bool)
    only[4] = True
    values, counts, n_nan, n_numbers = host_distinct(x, only)
    assert values.size == 0 and counts.size == 0 and (n_nan, n_numbers) == (1, 0)
    values, counts, n_nan, n_numbers = host_distinct(x, np.zeros(12, bool))
    assert values.size == 0 and values.dtype == dtype and counts.size == 0 and (n_nan, n_numbers) == (0, 0)
    # a signalling NaN and a negative NaN are NaNs by their bits
    u = np.uint64 if dtype == np.float64 else np.uint32
    odd = np.array([0x7FF0000000000001, 0xFFF8000000000000] if dtype == np.float64 else [0x7F800001, 0xFFC00000], dtype=u).view(dtype)
    assert is_nan_bits(odd).all() and not is_nan_bits(np.array([INF, -INF, 0.0, 1.0], dtype)).any()
    assert host_distinct(np.concatenate([odd, x]))[2] == 3


def test_unpack_mask_is_bit_r_of_word_r_over_64():
    words = np.array([1 | (1 << 63), 0, 2], dtype=np.uint64)
    bits = unpack_mask(words, 190)
    assert bits.size == 190 and np.flatnonzero(bits).tolist() == [0, 63, 129]
