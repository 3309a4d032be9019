"""CPU: the join probe (include/alpgpu.h, "join probe") is exported and declared, a NULL context is refused with ALPGPU_ERR_INVALID before the HIP
runtime is touched (ALPGPU_CHECK_CTX), so this runs without a device, and the host replica (tests/join_replica.py) is pinned on a hand-made case and
checked against a plain loop over the definition."""
import ctypes
import os
import subprocess

import numpy as np

from join_replica import NO_MATCH, host_bounds, host_join, host_probe, unpack_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_join_probe_f64", "alpgpu_join_probe_f32")
NAN, INF = float("nan"), float("inf")


def test_library_exports_the_join_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols
    assert capi.JOIN_NO_MATCH == -1 == NO_MATCH


def test_the_wrappers_exist():
    from alp_amd import capi
    for m in ("join_probe", "join_probe_into"):
        assert callable(getattr(capi.Context, m))
    with open(os.path.join(ROOT, "include", "alp", "batch.hpp")) as f:
        assert "join_probe(" in f.read()


def test_the_header_declares_them(tmp_path):
    src = tmp_path / "join_decls.c"
    src.write_text('#include "alpgpu.h"\n'
                   '_Static_assert(sizeof(alpgpu_column) == 104, "alpgpu_column keeps its layout");\n'
                   '_Static_assert(ALPGPU_JOIN_NO_MATCH == -1, "no match is -1, the index alpgpu_gather_* turns into a NaN");\n'
                   'int (*f0)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_f64*, const double*, uint64_t, const int64_t*, int64_t*, uint32_t*, int64_t*,\n'
                   '          uint64_t, uint64_t*, void*) = alpgpu_join_probe_f64;\n'
                   'int (*f1)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_f32*, const float*, uint64_t, const int64_t*, int64_t*, uint32_t*, int64_t*,\n'
                   '          uint64_t, uint64_t*, void*) = alpgpu_join_probe_f32;\n')
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_without_a_context_the_call_is_an_error_and_writes_nothing():
    from alp_amd import capi
    lib = capi.lib
    a = capi.CColumn()
    a.n_vectors = 1
    mask = (ctypes.c_uint64 * 16)(*([7] * 16))
    keys = (ctypes.c_double * 2)(1.0, 2.0)
    fkeys = (ctypes.c_float * 2)(1.0, 2.0)
    rows = (ctypes.c_int64 * 2)(5, 6)
    pos = (ctypes.c_int64 * 8)(*([11] * 8))
    span = (ctypes.c_uint32 * 8)(*([12] * 8))
    idx = (ctypes.c_int64 * 8)(*([13] * 8))
    count = (ctypes.c_uint64 * 1)(14)
    scratch = (ctypes.c_uint64 * 64)(*([15] * 64))
    p = lambda t: ctypes.cast(t, ctypes.c_void_p)
    for m in (None, p(mask)):
        for cap in (0, 8):
            assert lib.alpgpu_join_probe_f64(None, ctypes.byref(a), m, None, p(keys), 2, p(rows), p(pos), p(span), p(idx), cap, p(count), p(scratch)) == -2
            assert b"null context" in lib.alpgpu_last_error()
            assert lib.alpgpu_join_probe_f32(None, ctypes.byref(a), m, None, p(fkeys), 2, p(rows), p(pos), p(span), p(idx), cap, p(count), p(scratch)) == -2
            assert b"null context" in lib.alpgpu_last_error()
    assert list(mask) == [7] * 16 and list(keys) == [1.0, 2.0] and list(rows) == [5, 6]
    assert list(pos) == [11] * 8 and list(span) == [12] * 8 and list(idx) == [13] * 8 and list(count) == [14] and list(scratch) == [15] * 64


def test_the_replica_on_a_hand_made_case():
    for dtype in (np.float64, np.float32):
        up = lambda v: np.nextafter(dtype(v), dtype(INF))
        down = lambda v: np.nextafter(dtype(v), dtype(-INF))
        #                 0     1    2    3    4     5    6        7          8    9    10    11
        x = np.array([-0.0, 0.0, 1.5, NAN, INF, -INF, up(1.5), down(1.5), 7.0, 8.0, 99.0, -3.0], dtype=dtype)
        # sorted as numpy.sort sorts: both zeros (in the order -0.0, +0.0 here), 7.0 three times, NaNs last
        keys = np.array([-INF, -0.0, 0.0, 1.5, 7.0, 7.0, 7.0, 99.0, INF, NAN, NAN], dtype=dtype)
        assert np.array_equal(np.sort(keys)[:9], keys[:9]) and np.isnan(np.sort(keys)[9:]).all()  # (by ==: the zeros' order is free)
        lb, ub = host_bounds(x, keys)
        assert lb.dtype == np.int64 and ub.dtype == np.int64
        assert lb.tolist() == [1, 1, 3, 0, 8, 0, 4, 3, 4, 7, 7, 1]
        assert ub.tolist() == [3, 3, 4, 0, 9, 1, 4, 3, 7, 7, 8, 1]
        pos, span = host_probe(x, keys)
        assert pos.dtype == np.int64 and span.dtype == np.uint32
        assert span.tolist() == [2, 2, 1, 0, 1, 1, 0, 0, 3, 0, 1, 0]  # each zero matches both zeros; 7.0 its run of three; the NaN value nothing
        assert pos.tolist() == [1, 1, 3, -1, 8, 0, -1, -1, 4, -1, 7, -1]  # the run's first element
        # the zeros in the other order: the same positions
        swapped = keys.copy()
        swapped[1], swapped[2] = 0.0, -0.0
        p2, s2 = host_probe(x, swapped)
        assert np.array_equal(p2, pos) and np.array_equal(s2, span)
        # rows: the payload at the run's first element, read nowhere else
        rows = np.array([100, 101, 102, 103, 104, 105, 106, 107, 108, 109, 110], dtype=np.int64)
        p3, s3 = host_probe(x, keys, rows)
        assert p3.tolist() == [101, 101, 103, -1, 108, 100, -1, -1, 104, -1, 107, -1] and np.array_equal(s3, span)
        # NaN keys alone and an empty list match nothing, the NaN value included
        for none in (np.array([NAN, NAN], dtype=dtype), np.zeros(0, dtype=dtype)):
            pn, sn = host_probe(x, none, rows[:none.size])
            assert (pn == NO_MATCH).all() and not sn.any()
        # the rows of a bitmap: set bits ascending
        vec = np.full(1024, 5.0, dtype=dtype)
        vec[:x.size] = x
        words = np.zeros(16, dtype=np.uint64)
        words[0] = (1 << 0) | (1 << 3) | (1 << 8)
        words[15] = 1 << 63
        assert np.nonzero(unpack_bits(words))[0].tolist() == [0, 3, 8, 1023]
        idx, pj, sj = host_join(vec, keys, words, rows)
        assert idx.tolist() == [0, 3, 8, 1023] and pj.tolist() == [101, -1, 104, -1] and sj.tolist() == [2, 0, 3, 0]
        idx, pj, sj = host_join(vec, keys)
        assert idx.size == 1024 and np.array_equal(idx, np.arange(1024)) and pj[:12].tolist() == pos.tolist() and (pj[12:] == -1).all()


def test_the_replica_against_a_loop_over_the_definition():
    rng = np.random.default_rng(22)
    for case in range(50):
        dtype = (np.float64, np.float32)[case % 2]
        n_keys = int(rng.integers(0, 40))
        pool = np.concatenate([rng.integers(-5, 6, 12).astype(dtype), np.array([0.0, -0.0, INF, -INF, NAN], dtype=dtype)])
        keys = np.sort(rng.choice(pool, n_keys))  # duplicates, both zeros, NaNs last
        x = rng.choice(np.concatenate([pool, pool + dtype(0.5)]), 64)
        rows = rng.permutation(n_keys).astype(np.int64) + 1000
        pos, span = host_probe(x, keys, rows)
        for i, v in enumerate(x):
            with np.errstate(invalid="ignore"):
                lb = sum(1 for k in keys if k < v)
                ub = sum(1 for k in keys if k <= v)
                eq = sum(1 for k in keys if k == v)
            assert ub - lb == eq == int(span[i]), (case, i)
            assert int(pos[i]) == (int(rows[lb]) if eq else NO_MATCH), (case, i)
            if eq:
                assert all(k == v for k in keys[lb:lb + eq])
