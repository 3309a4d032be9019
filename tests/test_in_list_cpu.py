"""CPU: set membership (include/alpgpu.h, "set membership") is exported and declared, a NULL context is refused with ALPGPU_ERR_INVALID before the
HIP runtime is touched (ALPGPU_CHECK_CTX), so this runs without a device, and the host replica of the predicate (tests/in_list_replica.py) is
pinned on a hand-made case."""
import ctypes
import os
import subprocess

import numpy as np

from in_list_replica import host_in_mask, host_member, pack_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_select_in_mask_f64", "alpgpu_select_in_mask_f32", "alpgpu_in_list_lds_max")
NAN, INF = float("nan"), float("inf")


def test_library_exports_the_in_list_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols
    for m in ("select_in_mask", "in_list_lds_max"):
        assert callable(getattr(capi.Context, m))


def test_the_header_declares_them(tmp_path):
    src = tmp_path / "in_list_decls.c"
    src.write_text('#include "alpgpu.h"\n'
                   '_Static_assert(sizeof(alpgpu_column) == 104, "alpgpu_column keeps its layout");\n'
                   'int (*f0)(alpgpu_ctx*, const alpgpu_column*, uint64_t, uint64_t, const double*, uint64_t, int, const alpgpu_zone_f64*, int, uint64_t*) = alpgpu_select_in_mask_f64;\n'
                   'int (*f1)(alpgpu_ctx*, const alpgpu_column*, uint64_t, uint64_t, const float*, uint64_t, int, const alpgpu_zone_f32*, int, uint64_t*) = alpgpu_select_in_mask_f32;\n'
                   'size_t (*f2)(int) = alpgpu_in_list_lds_max;\n')
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_the_lds_tier_holds_a_list_of_both_types_and_of_nothing_else():
    from alp_amd import capi
    f = capi.lib.alpgpu_in_list_lds_max
    assert f(8) > 0 and f(4) > 0 and f(2) == 0 and f(0) == 0 and f(16) == 0 and f(-8) == 0
    assert f(4) == 2 * f(8)  # the same bytes of LDS
    assert capi.Context.in_list_lds_max("f64") == f(8) and capi.Context.in_list_lds_max(np.float32) == f(4) and capi.Context.in_list_lds_max("i16") == 0


def test_without_a_context_the_call_is_an_error_and_writes_nothing():
    from alp_amd import capi
    lib = capi.lib
    a = capi.CColumn()
    a.n_vectors = 1
    mask = (ctypes.c_uint64 * 16)(*([7] * 16))
    lst = (ctypes.c_double * 2)(1.0, 2.0)
    flst = (ctypes.c_float * 2)(1.0, 2.0)
    p = lambda t: ctypes.cast(t, ctypes.c_void_p)
    for op in (0, 1, 2):
        for negate in (0, 1):
            assert lib.alpgpu_select_in_mask_f64(None, ctypes.byref(a), 0, 1024, p(lst), 2, negate, None, op, p(mask)) == -2
            assert b"null context" in lib.alpgpu_last_error()
            assert lib.alpgpu_select_in_mask_f32(None, ctypes.byref(a), 0, 1024, p(flst), 2, negate, None, op, p(mask)) == -2
            assert b"null context" in lib.alpgpu_last_error()
    assert list(mask) == [7] * 16 and list(lst) == [1.0, 2.0]


def test_the_replica_on_a_hand_made_case():
    for dtype in (np.float64, np.float32):
        up = lambda v: np.nextafter(dtype(v), dtype(INF))
        down = lambda v: np.nextafter(dtype(v), dtype(-INF))
        #                  0     1    2    3     4     5    6        7          8    9     10   11           12
        vals = np.array([-0.0, 0.0, 1.5, NAN, INF, -INF, up(1.5), down(1.5), 7.0, 7.0, 8.0, up(0.0), down(-0.0)], dtype=dtype)
        x = np.full(1024, 100.0, dtype=dtype)
        x[:vals.size] = vals
        # +0.0 alone matches both zeros; duplicates and a NaN in the list change nothing; 1-ulp neighbours of 1.5 and of zero miss
        lst = np.array([NAN, 7.0, 0.0, 1.5, 7.0, INF, NAN, -INF, 7.0], dtype=dtype)
        m = host_member(x, lst)
        assert m.dtype == bool and m.shape == x.shape
        assert np.nonzero(m)[0].tolist() == [0, 1, 2, 4, 5, 8, 9]
        assert np.nonzero(host_member(x, np.array([-0.0], dtype=dtype)))[0].tolist() == [0, 1]  # and -0.0 alone as well
        assert not host_member(x, np.array([NAN], dtype=dtype)).any()  # a NaN element matches nothing, the NaN value included
        assert not host_member(x, np.zeros(0, dtype=dtype)).any()
        assert np.nonzero(host_member(x, np.array([up(1.5)], dtype=dtype)))[0].tolist() == [6]
        # the list's order does not matter to the replica (it sorts), nor does its length
        rng = np.random.default_rng(4)
        assert np.array_equal(host_member(x, rng.permutation(lst)), m)
        long = np.concatenate([lst, np.arange(200, 5000, dtype=dtype)])
        assert np.array_equal(host_member(x, long), m)
        # against the definition: a broadcast ==
        with np.errstate(invalid="ignore"):
            assert np.array_equal(m, (x[:, None] == lst[None, :]).any(axis=1))
        # negate: the NaN value qualifies (it is not a member); the range cuts both ways
        q = host_in_mask(x, lst, first=1, n=10)
        assert np.nonzero(q)[0].tolist() == [1, 2, 4, 5, 8, 9]
        nq = host_in_mask(x, lst, first=1, n=10, negate=True)
        assert np.nonzero(nq)[0].tolist() == [3, 6, 7, 10]
        assert not host_in_mask(x, lst, first=5, n=0).any() and not host_in_mask(x, lst, first=5, n=0, negate=True).any()
        words = pack_bits(q)
        assert words.dtype == np.uint64 and words.size == 16
        assert int(words[0]) == sum(1 << r for r in (1, 2, 4, 5, 8, 9)) and not words[1:].any()
        assert int(pack_bits(np.ones(1024, dtype=bool))[15]) == 2**64 - 1
