"""CPU: keyed MIN / MAX (include/alpgpu.h, "keyed MIN / MAX") is exported and declared, a NULL context is refused with ALPGPU_ERR_INVALID before the HIP
runtime is touched (ALPGPU_CHECK_CTX), so this runs without a device; the host replica (tests/keyed_minmax_replica.py) is pinned on a hand-made case and
held to minmax_replica's host_group_minmax + host_minmax_totals with point groups and to _reduce key by key; the Python wrappers refuse what does not fit
before any launch.  The tests of the symbols, the header, the NULL context and the wrappers need the feature and fail without it; the tests of the replica
need only numpy: they pin the yardstick every GPU expectation goes through."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from keyed_minmax_replica import host_keyed_minmax, same_records
from keyed_replica import match_keys
from minmax_replica import _reduce, host_group_minmax, host_minmax_totals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_decode_keyed_minmax_f64", "alpgpu_decode_keyed_minmax_f32", "alpgpu_debug_decode_keyed_minmax_f64", "alpgpu_debug_decode_keyed_minmax_f32")
NAN, INF = float("nan"), float("inf")


def test_library_exports_the_keyed_minmax_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols
    for m in ("keyed_minmax", "keyed_minmax_into"):
        assert callable(getattr(capi.Context, m))


def test_the_header_declares_them(tmp_path):
    src = tmp_path / "keyed_minmax_decls.c"
    text = '#include "alpgpu.h"\n_Static_assert(sizeof(alpgpu_zone_f64) == 16 && sizeof(alpgpu_zone_f32) == 8, "the records");\n'
    for i, (sfx, t) in enumerate((("f64", "double"), ("f32", "float"))):
        text += ('int (*f%d)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_%s*, const %s*, uint32_t, alpgpu_zone_%s*, uint64_t*)\n'
                 '    = alpgpu_decode_keyed_minmax_%s;\n' % (i, sfx, t, sfx, sfx))
        text += ('int (*d%d)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_%s*, const %s*, uint32_t, alpgpu_zone_%s*, uint64_t*,\n'
                 '          const alpgpu_keyed_tuning*, uint64_t*) = alpgpu_debug_decode_keyed_minmax_%s;\n' % (i, sfx, t, sfx, sfx))
    src.write_text(text)
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_the_three_lists_of_what_is_not_built_no_longer_name_it():
    for name in ("README.md", "DESIGN.md", "include/alpgpu.h"):
        with open(os.path.join(ROOT, name)) as f:
            assert "MIN / MAX per key" not in f.read(), name


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
        assert getattr(lib, "alpgpu_decode_keyed_minmax_" + t)(None, ctypes.byref(a), ctypes.byref(a), p(mask), None, p(keys), 4, p(out), p(counts)) == -2
        assert b"null context" in lib.alpgpu_last_error()
        assert getattr(lib, "alpgpu_debug_decode_keyed_minmax_" + t)(None, ctypes.byref(a), ctypes.byref(a), p(mask), None, p(keys), 4, p(out), p(counts), ctypes.byref(tuning),
                                                                      p(trace)) == -2
        assert b"null context" in lib.alpgpu_last_error()
        assert list(out) == [7.0] * 8
    assert list(mask) == [7] * 16 and list(counts) == [7] * 5 and list(trace) == [7] * 4


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_replica_on_a_hand_made_case(dtype):
    """Two vectors, keys 1, 2, 3 (and 9 and 7 in the key column, which are not in the list).  Selected are only the rows named here.
    key 1: -3.0, +0.0 and then -0.0 in another vector: min is -3, max is +0.0; with -3 taken out, min is -0.0 and max +0.0 BY THEIR BITS.
    key 2: 64 rows 1 .. 64 and one +inf: {1, +inf}.
    key 3: two rows, both NaN: {+inf, -inf}, count 2.
    62 selected rows of key 7: without a key."""
    val = np.zeros(2048, dtype)
    key = np.full(2048, 9.0, dtype)
    bits = np.zeros(2048, bool)
    val[0:64], key[0:64], bits[0:64] = np.arange(1, 65), 2.0, True
    val[64:128], key[64:128], bits[64:128] = 100.0, 7.0, True
    val[64], key[64], val[127], key[127] = NAN, 3.0, NAN, 3.0
    val[133], key[133], bits[133] = -3.0, 1.0, True
    val[200], key[200], bits[200] = 0.0, 1.0, True
    val[1024 + 70], key[1024 + 70], bits[1024 + 70] = -0.0, 1.0, True
    val[1500], key[1500], bits[1500] = INF, 2.0, True
    key[500], val[500] = 1.0, -1e30  # an unselected row of key 1.0: nothing
    keys = np.array([1.0, 2.0, 3.0], dtype)
    rec, counts = host_keyed_minmax(val, key, bits, keys)
    assert rec.dtype == dtype and rec.shape == (3, 2) and counts.dtype == np.int64
    assert rec.tolist() == [[-3.0, 0.0], [1.0, INF], [INF, -INF]] and not np.signbit(rec[0, 1])
    assert counts.tolist() == [3, 65, 2, 62] and int(counts.sum()) == int(bits.sum())
    bits[133] = False
    rec, counts = host_keyed_minmax(val, key, bits, keys)
    assert rec[0].tolist() == [0.0, 0.0] and np.signbit(rec[0, 0]) and not np.signbit(rec[0, 1]), "-0.0 < +0.0 by the bits, whichever comes first"
    # a duplicate key gets the empty record and 0; a NaN key at the end matches nothing; -0.0 in the list matches a +0.0 row; a NaN in the key column is a row without a key
    key[500], bits[500], val[500] = 0.0, True, 4.5
    key[700], bits[700] = NAN, True
    keys = np.array([-0.0, 1.0, 2.0, 2.0, 3.0, NAN], dtype)
    rec, counts = host_keyed_minmax(val, key, bits, keys)
    assert rec.tolist() == [[4.5, 4.5], [-0.0, 0.0], [1.0, INF], [INF, -INF], [INF, -INF], [INF, -INF]]
    assert counts.tolist() == [1, 2, 65, 0, 2, 0, 63]
    # no vectors at all
    rec, counts = host_keyed_minmax(np.zeros(0, dtype), np.zeros(0, dtype), np.zeros(0, bool), keys)
    assert rec.tolist() == [[INF, -INF]] * 6 and counts.tolist() == [0] * 7


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_replica_is_group_minmax_and_totals_with_point_groups(dtype):
    rng = np.random.default_rng(2601)
    for trial in range(6):
        n = int(rng.integers(1, 4))
        K = int(rng.choice([1, 2, 5, 70]))
        pool = np.unique(np.round(rng.normal(0, 50, 2 * K), 1).astype(dtype))
        keys = np.sort(np.concatenate([pool[:K], pool[:1], np.array([NAN], dtype)]))
        key = rng.choice(np.concatenate([pool, np.array([NAN, -0.0, 0.0], dtype)]), n * 1024).astype(dtype)
        if trial % 2:
            key[:1024] = np.repeat(rng.choice(pool, 16), 64)  # steps whose lanes agree
        val = (rng.normal(0, 1, n * 1024) * 10.0 ** rng.integers(-8, 12, n * 1024)).astype(dtype)
        val[rng.integers(0, n * 1024, 6)] = [NAN, -0.0, 0.0, INF, -INF, NAN]
        bits = rng.random(n * 1024) < (0.1, 0.6, 1.0)[trial % 3]
        rec, counts = host_keyed_minmax(val, key, bits, keys)
        assert int(counts.sum()) == int(bits.sum())
        first = np.concatenate([[True], keys[1:] != keys[:-1]]) & ~np.isnan(keys)  # the first of its equals
        zones, c = host_group_minmax(val, key, bits, keys.tolist(), keys.tolist())  # group g: lo = hi = keys[g]
        tot = host_minmax_totals(zones)
        assert same_records(rec[first], tot[first]) and np.array_equal(counts[:-1][first], c.sum(axis=1)[first])
        assert same_records(rec[~first], np.tile(np.array([INF, -INF], dtype), (int((~first).sum()), 1))) and not counts[:-1][~first].any()
        idx, matched = match_keys(key, keys)  # ... and _reduce itself, key by key
        for i in range(keys.size):
            assert same_records(rec[i], _reduce(val, bits & matched & (idx == i)))


def test_python_rejects_arguments_that_do_not_fit_before_any_launch(monkeypatch):
    """no device: the columns are bare descriptors and every check below fails before the library is called"""
    import torch
    from alp_amd import capi

    def unreachable(*a, **k):
        raise AssertionError("the library was called")
    for t in ("f64", "f32"):
        monkeypatch.setattr(capi.lib, "alpgpu_decode_keyed_minmax_" + t, unreachable)
        monkeypatch.setattr(capi.lib, "alpgpu_debug_decode_keyed_minmax_" + t, unreachable)

    class Col:  # what the wrappers look at before they reach the library
        def __init__(self, dtype, n_vectors):
            self.dtype, self.n_vectors, self.c = dtype, n_vectors, capi.CColumn()
    ctx = capi.Context.__new__(capi.Context)
    ctx.device = 0
    a, b, f, g, short = Col("f64", 4), Col("f64", 4), Col("f32", 4), Col("f32", 4), Col("f64", 3)
    good = np.array([1.0, 2.0, 3.0])
    for val, key in ((a, f), (a, short), (f, a)):  # the columns' types and lengths agree
        with pytest.raises(ValueError):
            ctx.keyed_minmax(val, key, good)
        with pytest.raises(ValueError):
            ctx.keyed_minmax_into(val, key, torch.zeros(3, dtype=torch.float64), torch.zeros((3, 2), dtype=torch.float64))
    for bad in (good.astype(np.float32), torch.zeros(3, dtype=torch.float32), torch.zeros(3, dtype=torch.int64), np.zeros((2, 2)), [], np.zeros(0), np.zeros(1025),
                torch.zeros(1025, dtype=torch.float64)):  # the columns' type, one dimension, 1 .. 1024 keys
        with pytest.raises(ValueError):
            ctx.keyed_minmax(a, b, bad)
    for bad in (good, torch.zeros(3, dtype=torch.float64), np.zeros(0, np.float32), np.zeros(1025, np.float32)):  # float columns take float keys
        with pytest.raises(ValueError):
            ctx.keyed_minmax(f, g, bad)
    for bad in (good, good.tolist(), torch.from_numpy(good), torch.zeros(3, dtype=torch.float32)):  # the raw form: a device tensor of the columns' type
        with pytest.raises(ValueError):
            ctx.keyed_minmax_into(a, b, bad, torch.zeros((3, 2), dtype=torch.float64))
