"""CPU: keyed MIN / MAX for up to 2^20 keys (include/alpgpu.h, "keyed MIN / MAX, many keys") is exported and declared, a NULL context is refused with
ALPGPU_ERR_INVALID before the HIP runtime is touched (ALPGPU_CHECK_CTX), so this runs without a device; the Python wrappers refuse what does not fit
before any launch and pass 1025 and 2^20 keys through; the host replica (tests/keyed_many_replica.py) equals keyed_minmax_replica.host_keyed_minmax bit
for bit up to 1024 keys and is pinned on a hand-made case of 1030 keys.  The tests of the symbols, the header, the NULL context and the wrappers need
the feature and fail without it; the tests of the replica need only numpy: they pin the yardstick every GPU expectation goes through."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from keyed_many_replica import host_keyed_minmax_many, match_many
from keyed_minmax_replica import host_keyed_minmax, same_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_decode_keyed_minmax_many_f64", "alpgpu_decode_keyed_minmax_many_f32", "alpgpu_debug_decode_keyed_minmax_many_f64",
         "alpgpu_debug_decode_keyed_minmax_many_f32")
NAN, INF = float("nan"), float("inf")
EMPTY = [INF, -INF]


def test_library_exports_the_keyed_minmax_many_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols
    assert capi.KEYED_MANY_KEYS_MAX == 1 << 20 and capi.KEYED_KEYS_MAX == 1024
    for m in ("keyed_minmax_many", "keyed_minmax_many_into"):
        assert callable(getattr(capi.Context, m))


def test_the_header_declares_them(tmp_path):
    src = tmp_path / "keyed_minmax_many_decls.c"
    text = ('#include "alpgpu.h"\n_Static_assert(ALPGPU_KEYED_MANY_KEYS_MAX == ALPGPU_DISTINCT_MAX && ALPGPU_KEYED_KEYS_MAX == 1024, "the two bounds");\n'
            '_Static_assert(ALPGPU_KEYED_MANY_KEYS_MAX == 1048576u, "2^20");\n')
    for i, (sfx, t) in enumerate((("f64", "double"), ("f32", "float"))):
        text += ('int (*f%d)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_%s*, const %s*, uint32_t, alpgpu_zone_%s*, uint64_t*)\n'
                 '    = alpgpu_decode_keyed_minmax_many_%s;\n' % (i, sfx, t, sfx, sfx))
        text += ('int (*d%d)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_%s*, const %s*, uint32_t, alpgpu_zone_%s*, uint64_t*,\n'
                 '          const alpgpu_keyed_tuning*, uint64_t*) = alpgpu_debug_decode_keyed_minmax_many_%s;\n' % (i, sfx, t, sfx, sfx))
    src.write_text(text)
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_the_three_lists_name_the_new_call_and_keyed_sum_stays_not_built():
    for name in ("README.md", "DESIGN.md", "include/alpgpu.h"):
        with open(os.path.join(ROOT, name)) as f:
            text = f.read()
        assert "keyed_minmax_many" in text, name
        assert "keyed SUM beyond 1024 keys" in text, name


def test_without_a_context_every_call_is_an_error_and_writes_nothing():
    from alp_amd import capi
    lib = capi.lib
    a = capi.CColumn()
    a.n_vectors = 1
    mask = (ctypes.c_uint64 * 16)(*([7] * 16))
    trace = (ctypes.c_uint64 * 4)(*([7] * 4))
    counts = (ctypes.c_uint64 * 5)(*([7] * 5))
    tuning = capi.KeyedTuning(1, 0)
    p = lambda t: ctypes.cast(t, ctypes.c_void_p)
    for t, ct in (("f64", ctypes.c_double), ("f32", ctypes.c_float)):
        keys = (ct * 4)(1.0, 2.0, 3.0, 4.0)
        out = (ct * 8)(*([7.0] * 8))
        assert getattr(lib, "alpgpu_decode_keyed_minmax_many_" + t)(None, ctypes.byref(a), ctypes.byref(a), p(mask), None, p(keys), 4, p(out), p(counts)) == -2
        assert b"null context" in lib.alpgpu_last_error()
        assert getattr(lib, "alpgpu_debug_decode_keyed_minmax_many_" + t)(None, ctypes.byref(a), ctypes.byref(a), p(mask), None, p(keys), 4, p(out), p(counts),
                                                                           ctypes.byref(tuning), p(trace)) == -2
        assert b"null context" in lib.alpgpu_last_error()
        assert list(out) == [7.0] * 8
    assert list(mask) == [7] * 16 and list(counts) == [7] * 5 and list(trace) == [7] * 4


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------------------------------------
class Col:  # what the wrappers look at before they reach the library
    def __init__(self, dtype, n_vectors):
        from alp_amd import capi
        self.dtype, self.n_vectors, self.c = dtype, n_vectors, capi.CColumn()


def bare_context():
    from alp_amd import capi
    ctx = capi.Context.__new__(capi.Context)
    ctx.device, ctx._h, ctx._follow_torch = 0, None, False
    return ctx


def test_python_rejects_arguments_that_do_not_fit_before_any_launch(monkeypatch):
    """no device: the columns are bare descriptors and every check below fails before the library is called"""
    import torch
    from alp_amd import capi

    def unreachable(*a, **k):
        raise AssertionError("the library was called")
    for t in ("f64", "f32"):
        monkeypatch.setattr(capi.lib, "alpgpu_decode_keyed_minmax_many_" + t, unreachable)
        monkeypatch.setattr(capi.lib, "alpgpu_debug_decode_keyed_minmax_many_" + t, unreachable)
    ctx = bare_context()
    a, b, f, g, short = Col("f64", 4), Col("f64", 4), Col("f32", 4), Col("f32", 4), Col("f64", 3)
    good = np.array([1.0, 2.0, 3.0])
    over = capi.KEYED_MANY_KEYS_MAX + 1
    for val, key in ((a, f), (a, short), (f, a)):  # the columns' types and lengths agree
        with pytest.raises(ValueError):
            ctx.keyed_minmax_many(val, key, good)
        with pytest.raises(ValueError):
            ctx.keyed_minmax_many_into(val, key, torch.zeros(3, dtype=torch.float64), torch.zeros((3, 2), dtype=torch.float64))
    for bad in (good.astype(np.float32), torch.zeros(3, dtype=torch.float32), torch.zeros(3, dtype=torch.int64), np.zeros((2, 2)), [], np.zeros(0), np.zeros(over),
                torch.zeros(over, dtype=torch.float64)):  # the columns' type, one dimension, 1 .. 2^20 keys
        with pytest.raises(ValueError):
            ctx.keyed_minmax_many(a, b, bad)
    for bad in (good, torch.zeros(3, dtype=torch.float64), np.zeros(0, np.float32), np.zeros(over, np.float32)):  # float columns take float keys
        with pytest.raises(ValueError):
            ctx.keyed_minmax_many(f, g, bad)
    for bad in (good, good.tolist(), torch.from_numpy(good), torch.zeros(3, dtype=torch.float32), torch.zeros(1025, dtype=torch.float64)):
        with pytest.raises(ValueError):  # the raw form: a DEVICE tensor of the columns' type; host keys are refused
            ctx.keyed_minmax_many_into(a, b, bad, torch.zeros((bad.numel() if isinstance(bad, torch.Tensor) else 3, 2), dtype=torch.float64))


def test_the_raw_wrapper_passes_1025_and_2_to_the_20_keys_through_and_refuses_one_more(monkeypatch):
    """no device: host tensors that answer as tensors on cuda:0 reach the (replaced) library with their n_keys; the bound is checked in front of it"""
    import torch
    from alp_amd import capi

    class OnDevice(torch.Tensor):  # a host tensor that says it lives on cuda:0: nothing dereferences it here
        is_cuda = property(lambda self: True)
        device = property(lambda self: torch.device("cuda", 0))
    seen = []

    def record(h, val, key, mask, zones, keys, n_keys, out, counts, *debug):
        seen.append((int(n_keys), counts is not None and counts.value is not None, len(debug)))
        return 0
    ctx = bare_context()
    for t, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        monkeypatch.setattr(capi.lib, "alpgpu_decode_keyed_minmax_many_" + t, record)
        monkeypatch.setattr(capi.lib, "alpgpu_debug_decode_keyed_minmax_many_" + t, record)
        a, b = Col(t, 4), Col(t, 4)
        for K in (1, 1024, 1025, capi.KEYED_MANY_KEYS_MAX):
            keys = torch.zeros(K, dtype=tdt).as_subclass(OnDevice)
            out = torch.zeros((K, 2), dtype=tdt).as_subclass(OnDevice)
            cnt = torch.zeros(K + 1, dtype=torch.int64).as_subclass(OnDevice)
            del seen[:]
            ctx.keyed_minmax_many_into(a, b, keys, out)
            ctx.keyed_minmax_many_into(a, b, keys, out, counts_out=cnt)
            ctx.keyed_minmax_many_into(a, b, keys, out, counts_out=cnt, tuning={"grid": 3})
            assert seen == [(K, False, 0), (K, True, 0), (K, True, 2)], (t, K, seen)
        K = capi.KEYED_MANY_KEYS_MAX + 1
        del seen[:]
        with pytest.raises(ValueError):
            ctx.keyed_minmax_many_into(a, b, torch.zeros(K, dtype=tdt).as_subclass(OnDevice), torch.zeros((K, 2), dtype=tdt).as_subclass(OnDevice))
        with pytest.raises(ValueError):  # ... and the old wrapper still stops at 1024
            ctx.keyed_minmax_into(a, b, torch.zeros(1025, dtype=tdt).as_subclass(OnDevice), torch.zeros((1025, 2), dtype=tdt).as_subclass(OnDevice))
        with pytest.raises(ValueError):  # counts of the wrong length
            ctx.keyed_minmax_many_into(a, b, torch.zeros(5, dtype=tdt).as_subclass(OnDevice), torch.zeros((5, 2), dtype=tdt).as_subclass(OnDevice),
                                       counts_out=torch.zeros(5, dtype=torch.int64).as_subclass(OnDevice))
        assert seen == []


# ---- the replica ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_replica_equals_host_keyed_minmax_up_to_1024_keys(dtype):
    rng = np.random.default_rng(2701)
    for trial in range(8):
        n = int(rng.integers(1, 4))
        K = int(rng.choice([1, 2, 5, 70, 1000]))
        pool = np.unique(np.round(rng.normal(0, 50, 2 * K), 1).astype(dtype))
        keys = np.sort(np.concatenate([pool[:K], pool[:1], np.array([NAN], dtype)]))[:1024]
        key = rng.choice(np.concatenate([pool, np.array([NAN, -0.0, 0.0], dtype)]), n * 1024).astype(dtype)
        if trial % 2:
            key[:1024] = np.repeat(rng.choice(pool, 16), 64)  # steps whose lanes agree
        val = (rng.normal(0, 1, n * 1024) * 10.0 ** rng.integers(-8, 12, n * 1024)).astype(dtype)
        val[rng.integers(0, n * 1024, 6)] = [NAN, -0.0, 0.0, INF, -INF, NAN]
        bits = rng.random(n * 1024) < (0.1, 0.6, 1.0)[trial % 3]
        rec, counts = host_keyed_minmax_many(val, key, bits, keys)
        want_r, want_c = host_keyed_minmax(val, key, bits, keys)
        assert rec.dtype == dtype and counts.dtype == np.int64
        assert same_records(rec, want_r) and np.array_equal(counts, want_c) and int(counts.sum()) == int(bits.sum())
    rec, counts = host_keyed_minmax_many(np.zeros(0, dtype), np.zeros(0, dtype), np.zeros(0, bool), keys)  # no vectors at all
    assert rec.tolist() == [EMPTY] * keys.size and counts.tolist() == [0] * (keys.size + 1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_replica_on_a_hand_made_case_of_1030_keys(dtype):
    """keys: -0.0 (position 0), 1 .. 1026 (positions 1 .. 1026), 1026 again (1027), 2000 (1028), NaN (1029).  Selected are only the rows named here.
    key 0 (-0.0 in the list): a +0.0 row of the key column matches it; its values are +0.0 and, in another vector, -0.0: {-0.0, +0.0} BY THEIR BITS.
    key 1026 (position 1026, past the old bound): 5.5 and a NaN value: {5.5, 5.5}, count 2; its duplicate at 1027 gets nothing.
    key 2000 (position 1028): one row, -inf.   key 700: 64 rows 1 .. 64.
    a NaN in the key column and 62 rows of key 0.5 (not in the list): rows without a key."""
    keys = np.concatenate([[-0.0], np.arange(1, 1027), [1026.0, 2000.0, NAN]]).astype(dtype)
    assert keys.size == 1030 and np.array_equal(np.sort(keys)[:-1], keys[:-1])
    val = np.zeros(3072, dtype)
    key = np.full(3072, 9999.0, dtype)
    bits = np.zeros(3072, bool)
    val[0:64], key[0:64], bits[0:64] = np.arange(1, 65), 700.0, True
    val[64:126], key[64:126], bits[64:126] = 100.0, 0.5, True
    val[130], key[130], bits[130] = 0.0, 0.0, True
    val[2048 + 9], key[2048 + 9], bits[2048 + 9] = -0.0, -0.0, True
    val[300], key[300], bits[300] = 5.5, 1026.0, True
    val[1024 + 5], key[1024 + 5], bits[1024 + 5] = NAN, 1026.0, True
    val[1500], key[1500], bits[1500] = -INF, 2000.0, True
    val[1600], key[1600], bits[1600] = 3.0, NAN, True
    key[1700], val[1700] = 1026.0, -1e30  # an unselected row of key 1026: nothing
    idx, matched = match_many(key, keys)
    assert idx[300] == 1026 and matched[300] and idx[1500] == 1028 and idx[130] == 0 and matched[130] and not matched[1600] and not matched[64]
    rec, counts = host_keyed_minmax_many(val, key, bits, keys)
    assert rec.dtype == dtype and rec.shape == (1030, 2) and counts.shape == (1031,)
    assert rec[0].tolist() == [0.0, 0.0] and np.signbit(rec[0, 0]) and not np.signbit(rec[0, 1]), "-0.0 < +0.0 by the bits"
    assert rec[700].tolist() == [1.0, 64.0] and rec[1026].tolist() == [5.5, 5.5] and rec[1027].tolist() == EMPTY and rec[1028].tolist() == [-INF, -INF]
    assert rec[1029].tolist() == EMPTY
    named = np.zeros(1030, bool)
    named[[0, 700, 1026, 1028]] = True
    assert rec[~named].tolist() == [EMPTY] * 1026
    assert counts[[0, 700, 1026, 1027, 1028, 1029, 1030]].tolist() == [2, 64, 2, 0, 1, 0, 63] and int(counts.sum()) == int(bits.sum()) == 132
