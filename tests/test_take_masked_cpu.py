"""CPU: the masked-projection entry points (include/alpgpu.h, "masked projection": alpgpu_decode_masked_f64 / _f32) are exported, the header
declares them with the documented signatures without touching the ABI version or alpgpu_column, and a NULL context is refused with
ALPGPU_ERR_INVALID before the HIP runtime is touched (ALPGPU_CHECK_CTX), so this runs without a device: no buffer passed in is modified."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_decode_masked_f64", "alpgpu_decode_masked_f32")


def test_library_exports_the_masked_projection():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols
    assert callable(capi.Context.decode_masked) and callable(capi.Context.decode_masked_into)


def test_the_header_declares_them(tmp_path):
    src = tmp_path / "take_masked_decls.c"
    src.write_text('#include "alpgpu.h"\n'
                   '_Static_assert(sizeof(alpgpu_column) == 104, "alpgpu_column keeps its layout");\n'
                   'int (*f0)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, double*, int64_t*, uint64_t, uint64_t*, void*) = alpgpu_decode_masked_f64;\n'
                   'int (*f1)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, float*, int64_t*, uint64_t, uint64_t*, void*) = alpgpu_decode_masked_f32;\n')
    p = subprocess.run(["gcc", "-std=c11", "-Werror", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_a_null_context_is_refused():
    from alp_amd import capi
    lib = capi.lib
    col = capi.CColumn()
    col.n_vectors = 1
    mask = (ctypes.c_uint64 * 16)(*([7] * 16))
    idx = (ctypes.c_int64 * 16)(*([7] * 16))
    vals64 = (ctypes.c_double * 16)(*([7.0] * 16))
    vals32 = (ctypes.c_float * 16)(*([7.0] * 16))
    count = (ctypes.c_uint64 * 1)(7)
    scratch = (ctypes.c_uint8 * 64)(*([7] * 64))
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    calls = [
        lambda: lib.alpgpu_decode_masked_f64(None, ctypes.byref(col), p(mask), p(vals64), p(idx), 16, p(count), p(scratch)),
        lambda: lib.alpgpu_decode_masked_f32(None, ctypes.byref(col), p(mask), p(vals32), p(idx), 16, p(count), p(scratch)),
        lambda: lib.alpgpu_decode_masked_f64(None, ctypes.byref(col), p(mask), None, None, 0, p(count), p(scratch)),
        lambda: lib.alpgpu_decode_masked_f32(None, None, None, None, None, 0, None, None),
    ]
    for call in calls:
        assert call() == -2
        assert b"null context" in lib.alpgpu_last_error()
    assert list(mask) == [7] * 16 and list(idx) == [7] * 16 and count[0] == 7 and list(scratch) == [7] * 64
    assert list(vals64) == [7.0] * 16 and list(vals32) == [7.0] * 16
