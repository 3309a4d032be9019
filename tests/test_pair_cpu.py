"""CPU: the two-column consumers (include/alpgpu.h, "two-column consumers") are exported, the header's constants are what the Python side uses, a
NULL context is refused with ALPGPU_ERR_INVALID before the HIP runtime is touched (ALPGPU_CHECK_CTX), so this runs without a device, and the
host replica of the documented summation order (tests/pair_replica.py) is pinned on a hand-made case that a fused multiply-add gets wrong."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np

from pair_replica import host_dots_masked

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_compare_mask_f64", "alpgpu_compare_mask_f32", "alpgpu_decode_dot_masked_f64", "alpgpu_decode_dot_masked_f32")


def test_library_exports_the_pair_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols


def test_the_header_declares_them_and_the_cmp_constants(tmp_path):
    src = tmp_path / "pair_decls.c"
    src.write_text('#include "alpgpu.h"\n'
                   '_Static_assert(ALPGPU_CMP_LT == 0 && ALPGPU_CMP_LE == 1 && ALPGPU_CMP_GT == 2 && ALPGPU_CMP_GE == 3 && ALPGPU_CMP_EQ == 4 && ALPGPU_CMP_NE == 5, "cmp");\n'
                   '_Static_assert(sizeof(alpgpu_column) == 104, "alpgpu_column keeps its layout");\n'
                   'int (*f0)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, uint64_t, uint64_t, int, int, uint64_t*) = alpgpu_compare_mask_f64;\n'
                   'int (*f1)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, uint64_t, uint64_t, int, int, uint64_t*) = alpgpu_compare_mask_f32;\n'
                   'int (*f2)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, const uint64_t*, double*, uint32_t*) = alpgpu_decode_dot_masked_f64;\n'
                   'int (*f3)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, const uint64_t*, double*, uint32_t*) = alpgpu_decode_dot_masked_f32;\n')
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    from alp_amd import capi
    assert (capi.CMP_LT, capi.CMP_LE, capi.CMP_GT, capi.CMP_GE, capi.CMP_EQ, capi.CMP_NE) == (0, 1, 2, 3, 4, 5)
    assert capi.Context._CMP_OPS == {"lt": 0, "le": 1, "gt": 2, "ge": 3, "eq": 4, "ne": 5}


def test_a_null_context_is_refused():
    from alp_amd import capi
    lib = capi.lib
    a, b = capi.CColumn(), capi.CColumn()
    a.n_vectors = b.n_vectors = 1
    mask = (ctypes.c_uint64 * 16)(*([7] * 16))
    sums = (ctypes.c_double * 1)(7.0)
    counts = (ctypes.c_uint32 * 1)(7)
    p = lambda t: ctypes.cast(t, ctypes.c_void_p)
    calls = [
        lambda: lib.alpgpu_compare_mask_f64(None, ctypes.byref(a), ctypes.byref(b), 0, 16, 0, 0, p(mask)),
        lambda: lib.alpgpu_compare_mask_f32(None, ctypes.byref(a), ctypes.byref(b), 0, 16, 5, 1, p(mask)),
        lambda: lib.alpgpu_decode_dot_masked_f64(None, ctypes.byref(a), ctypes.byref(b), p(mask), p(sums), p(counts)),
        lambda: lib.alpgpu_decode_dot_masked_f32(None, ctypes.byref(a), ctypes.byref(b), p(mask), p(sums), p(counts)),
    ]
    assert len(calls) == len(NAMES)
    for call in calls:
        assert call() == -2
        assert b"null context" in lib.alpgpu_last_error()
    assert list(mask) == [7] * 16 and sums[0] == 7.0 and counts[0] == 7


def fused(acc, a, b):
    """acc + a * b rounded ONCE: what a fused multiply-add returns (exact rational arithmetic, one conversion)"""
    return float(Fraction(acc) + Fraction(a) * Fraction(b))


def test_the_replica_multiplies_then_adds_in_the_documented_order():
    """two hand-made vectors.  Vector 0 holds one lane whose two products cancel when each is rounded before it is added and leave 2^-60 when
    the second is fused into the sum: the documented result is +0.0, so a kernel whose multiply and add contract cannot agree with this replica.
    Vector 1 pins the order: m ascending within a lane (1e16 + 1 - 1e16 is 0, not 1), clear bits skipped, adjacent-lane tree."""
    a, b = np.zeros((2, 1024)), np.zeros((2, 1024))
    bits = np.zeros((2, 1024), dtype=bool)
    x = 1.0 + 2.0 ** -30
    a[0, 0], b[0, 0] = -1.0, 1.0 + 2.0 ** -29  # lane 0, m = 0: exact
    a[0, 64], b[0, 64] = x, x                  # lane 0, m = 1: x * x = 1 + 2^-29 + 2^-60, the last term is rounded away
    bits[0, 0] = bits[0, 64] = True
    assert x * x == 1.0 + 2.0 ** -29 and fused(-(1.0 + 2.0 ** -29), x, x) == 2.0 ** -60
    # vector 1: lane 1: 3 * 0.5 at m = 0, 0.1 * 0.3 at m = 2 (rounds); lane 2: a value at m = 5 whose bit is clear; lane 5: 1e16, 1, -1e16 at m = 0, 1, 2;
    # lane 63: 2 * 4 at m = 15
    for lane, m, va, vb, on in ((1, 0, 3.0, 0.5, True), (1, 2, 0.1, 0.3, True), (2, 5, 1e300, 1e300, False), (5, 0, 1e16, 1.0, True), (5, 1, 1.0, 1.0, True),
                                (5, 2, -1e16, 1.0, True), (63, 15, 2.0, 4.0, True)):
        a[1, 64 * m + lane], b[1, 64 * m + lane], bits[1, 64 * m + lane] = va, vb, on
    got = host_dots_masked(a, b, bits)
    lane1 = 1.5 + 0.1 * 0.3  # (Python rounds the product, then the sum)
    assert got.view(np.int64)[0] == 0, "vector 0: product and sum are rounded separately, the result is +0.0 with the sign bit clear"
    assert got[1] == lane1 + 8.0 and got.dtype == np.float64  # lane 5 adds 0.0, lane 2 nothing; lanes 0..31 and 32..63 meet at the tree's top
    # floats widen first and their product is then exact in double
    af, bf = np.full((1, 1024), np.float32(0.1)), np.full((1, 1024), np.float32(0.3))
    one = np.zeros((1, 1024), dtype=bool)
    one[0, 7] = True
    assert host_dots_masked(af, bf, one)[0] == float(Fraction(float(np.float32(0.1))) * Fraction(float(np.float32(0.3))))
    # a selected NaN, and inf * 0, make the sum NaN; unselected ones do not
    a[1, 9], b[1, 9] = np.inf, 0.0
    assert host_dots_masked(a, b, bits)[1] == got[1]
    bits[1, 9] = True
    assert np.isnan(host_dots_masked(a, b, bits)[1])
