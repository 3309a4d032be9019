"""CPU: the selection entry points (include/alpgpu.h, "selection") are exported, the scratch size is monotone and inside its documented bound, and
a NULL context is refused with ALPGPU_ERR_INVALID before the HIP runtime is touched (ALPGPU_CHECK_CTX), so this runs without a device."""
import ctypes

NAMES = ("alpgpu_select_scratch_bytes", "alpgpu_select_range_f64", "alpgpu_select_range_f32")


def test_library_exports_the_selection_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n


def test_scratch_size_is_monotone_and_within_its_documented_bound():
    """include/alpgpu.h: at most 12 * n_vectors + n_vectors / 100 + 256 bytes, never 0, a multiple of 16; at least the 12 bytes per vector it keeps"""
    from alp_amd import capi
    f = capi.lib.alpgpu_select_scratch_bytes
    sizes = sorted(set([0, 1, 2, 3, 4, 5, 100, 1023, 1024, 1025, 2048, 2049, 70000, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1 << 30, (1 << 30) + 1, (1 << 40) + 12345,
                        1 << 54] + [7 ** k for k in range(1, 19)] + [1024 ** k + d for k in range(1, 6) for d in (-1, 0, 1)]))
    last = 0
    for n in sizes:
        b = f(n)
        assert b >= last, n
        assert b > 0 and b % 16 == 0, n
        assert 12 * n <= b <= 12 * n + n // 100 + 256, (n, b)
        last = b
    assert f((1 << 54) + 1) == 2**64 - 1 and f(2**64 - 1) == 2**64 - 1


def test_a_null_context_is_refused():
    from alp_amd import capi
    col = capi.CColumn()
    col.n_vectors = 1
    idx = (ctypes.c_int64 * 16)(*([7] * 16))
    vals = (ctypes.c_double * 16)(*([7.0] * 16))
    fvals = (ctypes.c_float * 16)(*([7.0] * 16))
    count = (ctypes.c_uint64 * 1)(7)
    scratch = (ctypes.c_uint8 * 64)(*([7] * 64))
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    assert capi.lib.alpgpu_select_range_f64(None, ctypes.byref(col), 0, 16, 0.0, 1.0, p(idx), p(vals), 16, p(count), p(scratch)) == -2
    assert b"null context" in capi.lib.alpgpu_last_error()
    assert capi.lib.alpgpu_select_range_f32(None, ctypes.byref(col), 0, 16, 0.0, 1.0, p(idx), p(fvals), 16, p(count), p(scratch)) == -2
    assert b"null context" in capi.lib.alpgpu_last_error()
    assert list(idx) == [7] * 16 and list(vals) == [7.0] * 16 and list(fvals) == [7.0] * 16 and count[0] == 7 and list(scratch) == [7] * 64
