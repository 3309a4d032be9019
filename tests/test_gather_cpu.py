"""CPU: the random-access entry points (include/alpgpu.h, "random access") are exported, and each refuses a NULL context with ALPGPU_ERR_INVALID
before it touches the HIP runtime (ALPGPU_CHECK_CTX), so this runs without a device."""
import ctypes

NAMES = ("alpgpu_gather_f64", "alpgpu_gather_f32", "alpgpu_decode_slice_f64", "alpgpu_decode_slice_f32")


def test_library_exports_the_random_access_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n


def test_a_null_context_is_refused():
    from alp_amd import capi
    col = capi.CColumn()
    col.n_vectors = 1
    buf = (ctypes.c_double * 16)()
    idx = (ctypes.c_int64 * 16)()
    assert capi.lib.alpgpu_gather_f64(None, ctypes.byref(col), ctypes.cast(idx, ctypes.c_void_p), 16, ctypes.cast(buf, ctypes.c_void_p)) == -2
    assert capi.lib.alpgpu_gather_f32(None, ctypes.byref(col), ctypes.cast(idx, ctypes.c_void_p), 16, ctypes.cast(buf, ctypes.c_void_p)) == -2
    assert capi.lib.alpgpu_decode_slice_f64(None, ctypes.byref(col), 0, 16, ctypes.cast(buf, ctypes.c_void_p)) == -2
    assert capi.lib.alpgpu_decode_slice_f32(None, ctypes.byref(col), 0, 16, ctypes.cast(buf, ctypes.c_void_p)) == -2
    assert b"null context" in capi.lib.alpgpu_last_error()
    assert list(buf) == [0.0] * 16
