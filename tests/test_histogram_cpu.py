"""CPU: the histograms (include/alpgpu.h, "histograms") are exported and declared, a NULL context is refused with ALPGPU_ERR_INVALID before the HIP
runtime is touched (ALPGPU_CHECK_CTX), so this runs without a device, and the host replica (tests/histogram_replica.py) is pinned on a hand-made
case, spelled out.  The first three tests need the feature (the symbols, the header's section, the wrappers); the replica's tests need only numpy:
they pin the yardstick every GPU expectation goes through and hold with or without the library."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from histogram_replica import host_histogram, sorted_edges, unpack_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_histogram_f64", "alpgpu_histogram_f32", "alpgpu_debug_histogram_f64", "alpgpu_debug_histogram_f32")
NAN, INF = float("nan"), float("inf")


def test_library_exports_the_histogram_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols
    for m in ("histogram", "histogram_into"):
        assert callable(getattr(capi.Context, m))
    assert capi.HISTOGRAM_EDGES_MAX == 4095
    assert ctypes.sizeof(capi.HistogramTuning) == 8


def test_the_header_declares_them(tmp_path):
    src = tmp_path / "histogram_decls.c"
    src.write_text('#include "alpgpu.h"\n'
                   '_Static_assert(ALPGPU_HISTOGRAM_EDGES_MAX == 4095, "the documented bound");\n'
                   '_Static_assert(sizeof(alpgpu_histogram_tuning) == 8, "the debug record");\n'
                   '_Static_assert(sizeof(alpgpu_column) == 104, "alpgpu_column keeps its layout");\n'
                   'int (*f0)(alpgpu_ctx*, const alpgpu_column*, uint64_t, uint64_t, const uint64_t*, const alpgpu_zone_f64*, const double*, uint32_t, int, int, uint64_t*) = alpgpu_histogram_f64;\n'
                   'int (*f1)(alpgpu_ctx*, const alpgpu_column*, uint64_t, uint64_t, const uint64_t*, const alpgpu_zone_f32*, const float*, uint32_t, int, int, uint64_t*) = alpgpu_histogram_f32;\n'
                   'int (*f2)(alpgpu_ctx*, const alpgpu_column*, uint64_t, uint64_t, const uint64_t*, const alpgpu_zone_f64*, const double*, uint32_t, int, int, uint64_t*,\n'
                   '          const alpgpu_histogram_tuning*, uint64_t*) = alpgpu_debug_histogram_f64;\n'
                   'int (*f3)(alpgpu_ctx*, const alpgpu_column*, uint64_t, uint64_t, const uint64_t*, const alpgpu_zone_f32*, const float*, uint32_t, int, int, uint64_t*,\n'
                   '          const alpgpu_histogram_tuning*, uint64_t*) = alpgpu_debug_histogram_f32;\n')
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_without_a_context_every_call_is_an_error_and_writes_nothing():
    from alp_amd import capi
    lib = capi.lib
    a = capi.CColumn()
    a.n_vectors = 1
    mask = (ctypes.c_uint64 * 16)(*([7] * 16))
    edges = (ctypes.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    counts = (ctypes.c_uint64 * 6)(*([7] * 6))
    trace = (ctypes.c_uint64 * 4)(*([7] * 4))
    tuning = capi.HistogramTuning(1, 1)
    p = lambda t: ctypes.cast(t, ctypes.c_void_p)
    for t in ("f64", "f32"):
        for accumulate in (0, 1):
            assert getattr(lib, "alpgpu_histogram_" + t)(None, ctypes.byref(a), 0, 1024, p(mask), None, p(edges), 4, 0, accumulate, p(counts)) == -2
            assert b"null context" in lib.alpgpu_last_error()
            assert getattr(lib, "alpgpu_debug_histogram_" + t)(None, ctypes.byref(a), 0, 1024, p(mask), None, p(edges), 4, 1, accumulate, p(counts), ctypes.byref(tuning), p(trace)) == -2
            assert b"null context" in lib.alpgpu_last_error()
    assert list(mask) == [7] * 16 and list(edges) == [1.0, 2.0, 3.0, 4.0] and list(counts) == [7] * 6 and list(trace) == [7] * 4


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_replica_on_a_hand_made_case(dtype):
    """a dozen values: both zeros with an edge at 0.0, values on edges under both rules, +-inf as values and as edges, a NaN value, a NaN edge at the
    end, duplicate edges; then no edges at all"""
    x = np.array([-INF, -1.5, -0.0, 0.0, 1.0, 2.0, 2.0, 3.0, 5.0, INF, NAN, 2.5], dtype=dtype)
    assert x.size == 12 and np.signbit(x[2]) and not np.signbit(x[3])
    edges = sorted_edges(np.array([2.0, NAN, INF, 0.0, -INF, 3.0, 2.0], dtype=dtype))
    assert np.array_equal(edges[:6], np.array([-INF, 0.0, 2.0, 2.0, 3.0, INF], dtype=dtype)) and np.isnan(edges[6]) and edges.dtype == dtype
    # right = False: bucket = #{e <= x}, the buckets [e[b-1], e[b]).  -inf sits on the first edge: bucket 1; both zeros on the edge 0.0: bucket 2; 2.0 on
    # the doubled edge: bucket 4, bucket 3 between the twins stays empty; +inf on the last real edge: bucket 6; nothing passes the NaN edge
    left_closed = host_histogram(x, edges)
    assert left_closed.dtype == np.uint64 and left_closed.tolist() == [0, 2, 3, 0, 3, 2, 1, 0, 1]
    # right = True: bucket = #{e < x}, the buckets (e[b-1], e[b]].  -inf: bucket 0; the zeros: bucket 1; 2.0: bucket 2; 3.0: bucket 4; +inf: bucket 5
    right_closed = host_histogram(x, edges, right=True)
    assert right_closed.tolist() == [1, 3, 3, 0, 2, 2, 0, 0, 1]
    assert int(left_closed.sum()) == int(right_closed.sum()) == 12
    # -0.0 as the edge: the same buckets
    neg = edges.copy()
    neg[1] = -0.0
    assert host_histogram(x, neg).tolist() == left_closed.tolist() and host_histogram(x, neg, right=True).tolist() == right_closed.tolist()
    # a selection: without the infinities and the NaN
    sel = np.ones(12, bool)
    sel[[0, 9, 10]] = False
    assert host_histogram(x, edges, sel).tolist() == [0, 1, 3, 0, 3, 2, 0, 0, 0]
    assert host_histogram(x, edges, np.zeros(12, bool)).tolist() == [0] * 9
    # no edges: one bucket, COUNT of the values that are no NaNs, and the NaN counter
    none = np.zeros(0, dtype)
    assert host_histogram(x, none).tolist() == [11, 1] and host_histogram(x, none, right=True).tolist() == [11, 1]
    assert host_histogram(x, none, sel).tolist() == [9, 0]
    # only NaN edges: everything in bucket 0
    assert host_histogram(x, np.array([NAN, NAN], dtype)).tolist() == [11, 0, 0, 1]


def test_the_replica_agrees_with_a_loop_over_the_definition():
    rng = np.random.default_rng(2107)
    for trial in range(50):
        x = np.round(rng.normal(0, 3, 400), 1)
        x[rng.integers(0, 400, 5)] = NAN
        edges = sorted_edges(np.concatenate([rng.choice(x[~np.isnan(x)], int(rng.integers(0, 30))), [NAN] * int(rng.integers(0, 3))]))
        sel = rng.random(400) < 0.7
        for right in (False, True):
            want = [0] * (edges.size + 2)
            for v in x[sel]:
                if v != v:
                    want[-1] += 1
                else:
                    want[sum(1 for e in edges if (e < v if right else e <= v))] += 1
            assert host_histogram(x, edges, sel, right).tolist() == want


def test_unpack_mask_is_bit_r_of_word_r_over_64():
    words = np.array([1 | (1 << 63), 0, 2], dtype=np.uint64)
    bits = unpack_mask(words, 190)
    assert bits.size == 190 and np.flatnonzero(bits).tolist() == [0, 63, 129]
    assert np.array_equal(unpack_mask(words.view(np.int64), 192), unpack_mask(words, 192))
