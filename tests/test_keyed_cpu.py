"""CPU: keyed aggregation (include/alpgpu.h, "keyed aggregation") is exported and declared, a NULL context is refused with ALPGPU_ERR_INVALID before the
HIP runtime is touched (ALPGPU_CHECK_CTX), so this runs without a device; the two host formulas are pinned; the host replica
(tests/keyed_replica.py) is pinned on a hand-made case, spelled out, and its two forms are held to each other; the Python wrappers refuse what does
not fit before any launch.  The tests of the symbols, the header, the NULL context, the two formulas and the wrappers need the feature and fail
without it; the four tests of the replica (the hand-made case, the two forms, match_keys) need only numpy: they pin the yardstick every GPU
expectation goes through and hold with or without the library, as tests/test_histogram_cpu.py's do."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from keyed_replica import host_keyed_sum, host_keyed_sum_dense, match_keys, same_sums, stripe_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_decode_keyed_sum_f64", "alpgpu_debug_decode_keyed_sum_f64", "alpgpu_keyed_stripe_vectors", "alpgpu_keyed_sum_scratch_bytes")  # (double columns only)
NAN, INF = float("nan"), float("inf")


def test_library_exports_the_keyed_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols
    for m in ("keyed_sum", "keyed_sum_into", "keyed_sum_scratch"):
        assert callable(getattr(capi.Context, m))
    assert capi.KEYED_KEYS_MAX == 1024
    assert ctypes.sizeof(capi.KeyedTuning) == 8


def test_the_header_declares_them(tmp_path):
    src = tmp_path / "keyed_decls.c"
    src.write_text('#include "alpgpu.h"\n'
                   '_Static_assert(ALPGPU_KEYED_KEYS_MAX == 1024 && ALPGPU_KEYED_STRIPES_MAX == 4096, "the documented bounds");\n'
                   '_Static_assert(sizeof(alpgpu_keyed_tuning) == 8, "the debug record");\n'
                   '_Static_assert(sizeof(alpgpu_column) == 104, "alpgpu_column keeps its layout");\n'
                   'uint64_t (*g0)(uint64_t) = alpgpu_keyed_stripe_vectors;\n'
                   'uint64_t (*g1)(uint64_t, uint32_t) = alpgpu_keyed_sum_scratch_bytes;\n'
                   'int (*f0)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_f64*, const double*, uint32_t, double*, uint64_t*, void*)\n'
                   '    = alpgpu_decode_keyed_sum_f64;\n'
                   'int (*f2)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_f64*, const double*, uint32_t, double*, uint64_t*, void*,\n'
                   '          const alpgpu_keyed_tuning*, uint64_t*) = alpgpu_debug_decode_keyed_sum_f64;\n')
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_without_a_context_every_call_is_an_error_and_writes_nothing():
    from alp_amd import capi
    lib = capi.lib
    a = capi.CColumn()
    a.n_vectors = 1
    mask = (ctypes.c_uint64 * 16)(*([7] * 16))
    keys = (ctypes.c_double * 4)(1.0, 2.0, 3.0, 4.0)
    sums = (ctypes.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    counts = (ctypes.c_uint64 * 5)(*([7] * 5))
    scratch = (ctypes.c_uint64 * 16)(*([7] * 16))
    trace = (ctypes.c_uint64 * 4)(*([7] * 4))
    tuning = capi.KeyedTuning(1, 0)
    p = lambda t: ctypes.cast(t, ctypes.c_void_p)
    for t in ("f64",):
        assert getattr(lib, "alpgpu_decode_keyed_sum_" + t)(None, ctypes.byref(a), ctypes.byref(a), p(mask), None, p(keys), 4, p(sums), p(counts), p(scratch)) == -2
        assert b"null context" in lib.alpgpu_last_error()
        assert getattr(lib, "alpgpu_debug_decode_keyed_sum_" + t)(None, ctypes.byref(a), ctypes.byref(a), p(mask), None, p(keys), 4, p(sums), p(counts), p(scratch),
                                                                   ctypes.byref(tuning), p(trace)) == -2
        assert b"null context" in lib.alpgpu_last_error()
    assert list(mask) == [7] * 16 and list(sums) == [7.0] * 4 and list(counts) == [7] * 5 and list(scratch) == [7] * 16 and list(trace) == [7] * 4


def test_the_stripe_length():
    from alp_amd import capi
    want = {0: 1, 1: 1, 4096: 1, 4097: 2, 8192: 2, 8193: 3, 2**30: 2**18}
    for n, L in want.items():
        assert capi.lib.alpgpu_keyed_stripe_vectors(n) == L == stripe_vectors(n), n
    for n in (4097, 8193, 12289, 2**30 + 1):  # never more than 4096 stripes
        L = capi.lib.alpgpu_keyed_stripe_vectors(n)
        assert -(-n // L) <= 4096


def test_the_scratch_formula():
    from alp_amd import capi
    f = capi.lib.alpgpu_keyed_sum_scratch_bytes
    up16 = lambda b: (b + 15) & ~15
    for n in (0, 1, 2, 3, 4095, 4096, 4097, 8192, 8193, 10**6, 2**30):
        for k in (1, 2, 63, 64, 65, 1023, 1024):
            got = f(n, k)
            assert got == up16(64 + 8 * k * min(n, 4096)), (n, k)
            L = stripe_vectors(n)
            assert got >= 64 + 8 * k * -(-n // L), "the S rows of partials fit"
            assert got <= 64 + 8 * k * 4096 and got % 16 == 0
    ns = [0, 1, 2, 100, 4095, 4096, 4097, 5000, 8192, 8193, 2**20, 2**30]
    for k in (1, 64, 1024):  # monotone in n_vectors, also where the number of stripes is not (4096 vectors: 4096 stripes; 4097: 2049)
        sizes = [f(n, k) for n in ns]
        assert sizes == sorted(sizes)
    for n in (1, 4096, 4097):
        sizes = [f(n, k) for k in range(1, 1025)]
        assert sizes == sorted(sizes)
    assert f(2**30, 1024) == 64 + 8 * 1024 * 4096
    for k in (0, 1025, 2**32 - 1):
        assert f(100, k) == 2**64 - 1


def test_the_replica_on_a_hand_made_case():
    """Two vectors (L = 1: two stripes), three keys.  Selected are only the rows named here.
    vector 0, step 0: all 64 lanes on key 2.0, values 1 .. 64: one tree, 2080.
    vector 0, step 1: key 3.0 in lanes 0 and 63 only (0.5 and 0.25: the tree's two ends meet at its root, 0.75); the 62 lanes between hold the key 7.0,
                      which is not in the list: 62 rows without a key.
    vector 0, step 2: lane 5 on key 1.0, value -3.0.
    vector 1, step 5: key 1.0 in lanes 0 .. 3 with 1e16, 1, 1, 1.  The adjacent tree adds (1e16 + 1) + (1 + 1) = 1e16 + 2 (1e16 + 1 is a tie and
                      rounds to the even 1e16); lane after lane would give 1e16.
    vector 1, step 6: lane 10 on key 1.0, value 1: the stripe's accumulator (1e16 + 2) + 1 is a tie and rounds to the even 1e16 + 4.
    vector 1, step 7: lane 3 on key 1.0, value 1: (1e16 + 4) + 1 is a tie and stays 1e16 + 4.
    key 1.0: stripes -3 and 1e16 + 4; their tree, -3 + (1e16 + 4) = 1e16 + 1, is a tie and rounds to the even 1e16."""
    val = np.zeros(2048)
    key = np.full(2048, 9.0)
    bits = np.zeros(2048, bool)
    val[0:64], key[0:64], bits[0:64] = np.arange(1, 65), 2.0, True
    val[64:128], key[64:128], bits[64:128] = 100.0, 7.0, True
    val[64], key[64], val[127], key[127] = 0.5, 3.0, 0.25, 3.0
    val[128 + 5], key[128 + 5], bits[128 + 5] = -3.0, 1.0, True
    s5 = 1024 + 5 * 64
    val[s5: s5 + 4], key[s5: s5 + 4], bits[s5: s5 + 4] = [1e16, 1.0, 1.0, 1.0], 1.0, True
    val[1024 + 6 * 64 + 10], key[1024 + 6 * 64 + 10], bits[1024 + 6 * 64 + 10] = 1.0, 1.0, True
    val[1024 + 7 * 64 + 3], key[1024 + 7 * 64 + 3], bits[1024 + 7 * 64 + 3] = 1.0, 1.0, True
    key[500] = 1.0  # an unselected row of key 1.0: nothing
    keys = np.array([1.0, 2.0, 3.0])
    for f in (host_keyed_sum_dense, host_keyed_sum):
        sums, counts = f(val, key, bits, keys)
        assert sums.dtype == np.float64 and counts.dtype == np.int64
        assert sums.tolist() == [1e16, 2080.0, 0.75], f.__name__
        assert counts.tolist() == [7, 64, 2, 62] and int(counts.sum()) == int(bits.sum())
    assert 1e16 + 2.0 != 1e16 and (1e16 + 1.0) + 1.0 == 1e16, "the tree's order shows in the case"
    # a duplicate key gets +0.0 and 0; a NaN key at the end matches nothing; -0.0 in the list matches a +0.0 row
    key[500], bits[500], val[500] = 0.0, True, 4.5
    keys = np.array([-0.0, 1.0, 2.0, 2.0, 3.0, NAN])
    for f in (host_keyed_sum_dense, host_keyed_sum):
        sums, counts = f(val, key, bits, keys)
        assert sums.tolist()[:5] == [4.5, 1e16, 2080.0, 0.0, 0.75] and sums[5] == 0.0 and not np.signbit(sums[3])
        assert counts.tolist() == [1, 7, 64, 0, 2, 0, 62]
    # a selected NaN value makes its key's sum a NaN; a NaN in the key column is a row without a key
    val[3], key[700], bits[700] = NAN, NAN, True
    for f in (host_keyed_sum_dense, host_keyed_sum):
        sums, counts = f(val, key, bits, keys)
        assert np.isnan(sums[2]) and sums[1] == 1e16 and counts.tolist() == [1, 7, 64, 0, 2, 0, 63]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_two_forms_of_the_replica_agree(dtype):
    rng = np.random.default_rng(2501)
    for trial in range(6):
        n = int(rng.integers(1, 4))
        K = int(rng.choice([1, 2, 5, 70]))
        pool = np.unique(np.round(rng.normal(0, 50, 2 * K), 1).astype(dtype))
        keys = np.sort(np.concatenate([pool[:K], pool[:1], np.array([NAN], dtype)]))[: min(K + 2, 1024)]
        key = rng.choice(np.concatenate([pool, np.array([NAN, -0.0, 0.0], dtype)]), n * 1024).astype(dtype)
        if trial % 2:
            key[:1024] = np.repeat(rng.choice(pool, 16), 64)  # steps whose lanes agree
        val = (rng.normal(0, 1, n * 1024) * 10.0 ** rng.integers(-8, 12, n * 1024)).astype(dtype)
        val[rng.integers(0, n * 1024, 3)] = [NAN, -0.0, INF]
        bits = rng.random(n * 1024) < (0.1, 0.6, 1.0)[trial % 3]
        a, ca = host_keyed_sum_dense(val, key, bits, keys)
        b, cb = host_keyed_sum(val, key, bits, keys)
        assert same_sums(a, b) and np.array_equal(ca, cb) and int(ca.sum()) == int(bits.sum())
    # several vectors to a stripe: 4097 vectors are stripes of two, the last of one
    n, K = 4097, 3
    keys = np.array([1.0, 2.0, 3.0], dtype)
    key = rng.choice(np.array([1.0, 2.0, 3.0, 4.0], dtype), n * 1024)
    val = (rng.normal(0, 1, n * 1024) * 10.0 ** rng.integers(-3, 6, n * 1024)).astype(dtype)
    bits = rng.random(n * 1024) < 0.02
    a, ca = host_keyed_sum_dense(val, key, bits, keys)
    b, cb = host_keyed_sum(val, key, bits, keys)
    assert same_sums(a, b) and np.array_equal(ca, cb)


def test_match_keys_is_the_first_equal_key():
    keys = np.array([-INF, -0.0, 0.0, 1.0, 1.0, INF, NAN])
    at, ok = match_keys(np.array([0.0, -0.0, 1.0, INF, -INF, NAN, 0.5, 2.0]), keys)
    assert ok.tolist() == [True, True, True, True, True, False, False, False]
    assert at[:5].tolist() == [1, 1, 3, 5, 0] and bool((at < keys.size).all())


def test_python_rejects_arguments_that_do_not_fit_before_any_launch(monkeypatch):
    """no device: the columns are bare descriptors and every check below fails before the library is called"""
    import torch
    from alp_amd import capi

    def unreachable(*a, **k):
        raise AssertionError("the library was called")
    for t in ("f64",):
        monkeypatch.setattr(capi.lib, "alpgpu_decode_keyed_sum_" + t, unreachable)
        monkeypatch.setattr(capi.lib, "alpgpu_debug_decode_keyed_sum_" + t, unreachable)

    class Col:  # what the wrappers look at before they reach the library
        def __init__(self, dtype, n_vectors):
            self.dtype, self.n_vectors, self.c = dtype, n_vectors, capi.CColumn()
    ctx = capi.Context.__new__(capi.Context)
    ctx.device = 0
    a, b, f, short = Col("f64", 4), Col("f64", 4), Col("f32", 4), Col("f64", 3)
    good = np.array([1.0, 2.0, 3.0])
    for val, key in ((a, f), (a, short)):  # the columns' types and lengths agree
        with pytest.raises(ValueError):
            ctx.keyed_sum(val, key, good)
        with pytest.raises(ValueError):
            ctx.keyed_sum_into(val, key, torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    for bad in (good.astype(np.float32), torch.zeros(3, dtype=torch.float32), torch.zeros(3, dtype=torch.int64), np.zeros((2, 2)), [], np.zeros(0), np.zeros(1025),
                torch.zeros(1025, dtype=torch.float64)):  # the columns' type, one dimension, 1 .. 1024 keys
        with pytest.raises(ValueError):
            ctx.keyed_sum(a, b, bad)
    with pytest.raises(ValueError):
        ctx.keyed_sum(f, f, good.astype(np.float32))  # float columns: not built
    for bad in (good, good.tolist(), torch.from_numpy(good), torch.zeros(3, dtype=torch.float32)):  # the raw form: a device tensor of the columns' type
        with pytest.raises(ValueError):
            ctx.keyed_sum_into(a, b, bad, torch.zeros(3, dtype=torch.float64))
    for n, k in ((-1, 4), (10, 0), (10, 1025)):
        with pytest.raises(ValueError):
            ctx.keyed_sum_scratch(n, k)
