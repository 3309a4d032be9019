"""CPU: the zone-map entry points (include/alpgpu.h, "zone maps") are exported, the records have the sizes the header documents, and a NULL
context is refused with ALPGPU_ERR_INVALID before the HIP runtime is touched (ALPGPU_CHECK_CTX), so this runs without a device."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_zone_map_f64", "alpgpu_zone_map_f32", "alpgpu_zone_map_of_values_f64", "alpgpu_zone_map_of_values_f32", "alpgpu_zones_minmax_f64",
         "alpgpu_zones_minmax_f32", "alpgpu_select_range_zoned_f64", "alpgpu_select_range_zoned_f32")


def test_library_exports_the_zone_map_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n


def test_record_sizes(tmp_path):
    """alpgpu_zone_f64 is {double min, max} = 16 bytes, alpgpu_zone_f32 {float min, max} = 8, as a C compiler lays the header's types out"""
    src = tmp_path / "zone_sizes.c"
    src.write_text('#include <stddef.h>\n#include "alpgpu.h"\n'
                   '_Static_assert(sizeof(alpgpu_zone_f64) == 16 && offsetof(alpgpu_zone_f64, min) == 0 && offsetof(alpgpu_zone_f64, max) == 8, "alpgpu_zone_f64");\n'
                   '_Static_assert(sizeof(alpgpu_zone_f32) == 8 && offsetof(alpgpu_zone_f32, min) == 0 && offsetof(alpgpu_zone_f32, max) == 4, "alpgpu_zone_f32");\n'
                   '_Static_assert(sizeof(alpgpu_column) == 104, "alpgpu_column keeps its layout");\n')
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    from alp_amd import capi
    assert capi.lib.alpgpu_abi_version() == 3


def test_a_null_context_is_refused():
    from alp_amd import capi
    lib = capi.lib
    col = capi.CColumn()
    col.n_vectors = 1
    zones = (ctypes.c_double * 8)(*([7.0] * 8))
    fzones = (ctypes.c_float * 8)(*([7.0] * 8))
    x = (ctypes.c_double * 1024)(*([1.0] * 1024))
    fx = (ctypes.c_float * 1024)(*([1.0] * 1024))
    mm = (ctypes.c_double * 2)(7.0, 7.0)
    fmm = (ctypes.c_float * 2)(7.0, 7.0)
    idx = (ctypes.c_int64 * 16)(*([7] * 16))
    vals = (ctypes.c_double * 16)(*([7.0] * 16))
    fvals = (ctypes.c_float * 16)(*([7.0] * 16))
    count = (ctypes.c_uint64 * 1)(7)
    scratch = (ctypes.c_uint8 * 64)(*([7] * 64))
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    calls = [
        lambda: lib.alpgpu_zone_map_f64(None, ctypes.byref(col), p(zones)),
        lambda: lib.alpgpu_zone_map_f32(None, ctypes.byref(col), p(fzones)),
        lambda: lib.alpgpu_zone_map_of_values_f64(None, p(x), 1, p(zones)),
        lambda: lib.alpgpu_zone_map_of_values_f32(None, p(fx), 1, p(fzones)),
        lambda: lib.alpgpu_zones_minmax_f64(None, p(zones), 4, p(mm)),
        lambda: lib.alpgpu_zones_minmax_f32(None, p(fzones), 4, p(fmm)),
        lambda: lib.alpgpu_select_range_zoned_f64(None, ctypes.byref(col), p(zones), 0, 16, 0.0, 1.0, p(idx), p(vals), 16, p(count), p(scratch)),
        lambda: lib.alpgpu_select_range_zoned_f32(None, ctypes.byref(col), p(fzones), 0, 16, 0.0, 1.0, p(idx), p(fvals), 16, p(count), p(scratch)),
    ]
    assert len(calls) == len(NAMES)
    for call in calls:
        assert call() == -2
        assert b"null context" in lib.alpgpu_last_error()
    assert list(zones) == [7.0] * 8 and list(fzones) == [7.0] * 8 and list(mm) == [7.0, 7.0] and list(fmm) == [7.0, 7.0]
    assert list(idx) == [7] * 16 and list(vals) == [7.0] * 16 and list(fvals) == [7.0] * 16 and count[0] == 7 and list(scratch) == [7] * 64
