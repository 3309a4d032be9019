"""CPU: the selection-bitmap entry points (include/alpgpu.h, "selection bitmaps") are exported, the header's constants are what the Python side
uses, and a NULL context is refused with ALPGPU_ERR_INVALID before the HIP runtime is touched (ALPGPU_CHECK_CTX), so this runs without a
device: no buffer passed in is modified."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_select_mask_f64", "alpgpu_select_mask_f32", "alpgpu_mask_to_indices", "alpgpu_decode_sum_masked_f64", "alpgpu_decode_sum_masked_f32")


def test_library_exports_the_mask_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols


def test_the_header_declares_them_and_the_op_constants(tmp_path):
    src = tmp_path / "mask_decls.c"
    src.write_text('#include "alpgpu.h"\n'
                   '_Static_assert(ALPGPU_MASK_SET == 0 && ALPGPU_MASK_AND == 1 && ALPGPU_MASK_OR == 2, "ops");\n'
                   '_Static_assert(sizeof(alpgpu_column) == 104, "alpgpu_column keeps its layout");\n'
                   'int (*f0)(alpgpu_ctx*, const alpgpu_column*, uint64_t, uint64_t, double, double, int, uint64_t*) = alpgpu_select_mask_f64;\n'
                   'int (*f1)(alpgpu_ctx*, const alpgpu_column*, uint64_t, uint64_t, float, float, int, uint64_t*) = alpgpu_select_mask_f32;\n'
                   'int (*f2)(alpgpu_ctx*, const uint64_t*, uint64_t, int64_t*, uint64_t, uint64_t*, void*) = alpgpu_mask_to_indices;\n'
                   'int (*f3)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, double*, uint32_t*) = alpgpu_decode_sum_masked_f64;\n'
                   'int (*f4)(alpgpu_ctx*, const alpgpu_column*, const uint64_t*, double*, uint32_t*) = alpgpu_decode_sum_masked_f32;\n')
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    from alp_amd import capi
    assert (capi.MASK_SET, capi.MASK_AND, capi.MASK_OR) == (0, 1, 2)


def test_a_null_context_is_refused():
    from alp_amd import capi
    lib = capi.lib
    col = capi.CColumn()
    col.n_vectors = 1
    mask = (ctypes.c_uint64 * 16)(*([7] * 16))
    idx = (ctypes.c_int64 * 16)(*([7] * 16))
    count = (ctypes.c_uint64 * 1)(7)
    scratch = (ctypes.c_uint8 * 64)(*([7] * 64))
    sums = (ctypes.c_double * 1)(7.0)
    counts = (ctypes.c_uint32 * 1)(7)
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    calls = [
        lambda: lib.alpgpu_select_mask_f64(None, ctypes.byref(col), 0, 16, 0.0, 1.0, 0, p(mask)),
        lambda: lib.alpgpu_select_mask_f32(None, ctypes.byref(col), 0, 16, 0.0, 1.0, 1, p(mask)),
        lambda: lib.alpgpu_mask_to_indices(None, p(mask), 1, p(idx), 16, p(count), p(scratch)),
        lambda: lib.alpgpu_decode_sum_masked_f64(None, ctypes.byref(col), p(mask), p(sums), p(counts)),
        lambda: lib.alpgpu_decode_sum_masked_f32(None, ctypes.byref(col), p(mask), p(sums), p(counts)),
    ]
    assert len(calls) == len(NAMES)
    for call in calls:
        assert call() == -2
        assert b"null context" in lib.alpgpu_last_error()
    assert list(mask) == [7] * 16 and list(idx) == [7] * 16 and count[0] == 7 and list(scratch) == [7] * 64 and sums[0] == 7.0 and counts[0] == 7
