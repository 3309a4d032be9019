"""GPU: keyed MIN / MAX for up to 2^20 keys (include/alpgpu.h, "keyed MIN / MAX, many keys": alpgpu_decode_keyed_minmax_many_*), double and float.  No
expectation comes from the code under test: the columns' values are the arrays that were encoded (the store decode is held to them bit for bit where
they are encoded, and to the oracle by other suites) or the oracle's decode of hand-built vectors; records and counts come from
tests/keyed_many_replica.py (its own searchsorted, clamp and ==; integer order keys).  Records compare as bytes, counts as integers; every output is
poisoned before the call.  Columns, key patterns, key lists and bitmaps are tests/test_keyed_gpu.py's.

The tiers: a double list up to 4096 keys (float: 8192) sits in LDS whole; a longer one leaves every stride-th key there (stride = ceil(K / 4096) or
ceil(K / 8192)) and ends its search in the list itself."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from alp_amd import capi
from keyed_many_replica import host_keyed_minmax_many
from keyed_minmax_replica import same_records
from test_keyed_gpu import PATTERNS, POISON, encoded, key_column, key_list, key_pool, masks_of, random_mask, unpack_np, vectors_cleared, widened
from test_keyed_minmax_gpu import value_column

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF, NAN = math.inf, math.nan
DTYPES = {"f64": np.float64, "f32": np.float32}
EMPTY = [INF, -INF]
LDS_MAX = {"f64": 4096, "f32": 8192}  # the longest list that is staged whole
GLOBAL_K = {"f64": 4097, "f32": 8193}  # the shortest list of the pivot tier: stride 2


def bitmaps(n, seed):
    m = masks_of(n, seed)
    return {"none": None, "random": m["random"], "vectors zero": m["vectors zero"], "all zero": torch.zeros(16 * n, dtype=torch.int64, device=DEV)}


def run(ctx, val, key, keys, mask=None, zones=None, tuning=None, trace=None, counts=True, old=False):
    """keyed_minmax_many_into (old: keyed_minmax_into) on poisoned outputs: (records [K, 2] as numpy, counts int64[K + 1] as numpy or None)"""
    kd = torch.from_numpy(np.ascontiguousarray(keys)).to(DEV)
    out = torch.full((kd.numel(), 2), NAN, dtype=kd.dtype, device=DEV)
    cnt = torch.full((kd.numel() + 1,), POISON, dtype=torch.int64, device=DEV) if counts else None
    (ctx.keyed_minmax_into if old else ctx.keyed_minmax_many_into)(val, key, kd, out, counts_out=cnt, mask=mask, zones=zones, tuning=tuning, trace=trace)
    return out.cpu().numpy(), (cnt.cpu().numpy() if counts else None)


def bits_of(mask, total):
    return np.ones(total, bool) if mask is None else unpack_np(mask, total)


def check(ctx, val, xv, key, xk, keys, mask, what, **kw):
    bits = bits_of(mask, xv.size)
    want_r, want_c = host_keyed_minmax_many(xv, xk, bits, keys)
    got_r, got_c = run(ctx, val, key, keys, mask=mask, **kw)
    assert np.array_equal(got_c, want_c), f"{what}: counts differ from the replica in {int((got_c != want_c).sum())} words"
    assert same_records(got_r, want_r), f"{what}: records differ from the replica in {int((got_r.view(np.uint8) != want_r.view(np.uint8)).reshape(len(keys), -1).any(axis=1).sum())} keys"
    assert int(got_c.sum()) == int(bits.sum())
    return got_r, got_c


def stride_of(dtype, K):
    return -(-K // LDS_MAX[dtype]) if K > LDS_MAX[dtype] else 1


# ---- 1. the old range: the replica's records and the bytes of keyed_minmax_into ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 64, 1024])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_old_range_equals_the_replica_and_keyed_minmax_into_byte_for_byte(ctx, dtype, K):
    n = 3
    val, xv = value_column(ctx, dtype, "mixed", n)
    keys = key_list(K, xv.dtype)
    for pattern in PATTERNS:
        key, xk = key_column(ctx, pattern, n, K, xv.dtype)
        for mname, mask in bitmaps(n, 21 + K).items():
            what = f"{dtype}, {n} vectors, {K} keys, {pattern}, bitmap {mname}"
            trace, old_trace = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
            r, c = check(ctx, val, xv, key, xk, keys, mask, what, trace=trace)
            o_r, o_c = run(ctx, val, key, keys, mask=mask, trace=old_trace, old=True)
            assert r.tobytes() == o_r.tobytes() and c.tobytes() == o_c.tobytes() and trace.tolist() == old_trace.tolist(), f"{what}: not keyed_minmax_into's bytes"
            if mname == "all zero":
                assert r.tolist() == [EMPTY] * K and not c.any() and trace.tolist() == [n, 0, 0, 0], "nothing selected: every vector is skipped"
    zones = ctx.zone_map(key)  # (the last pattern's) ... and with the key column's zone map
    r, c = run(ctx, val, key, keys, mask=mask, zones=zones)
    o_r, o_c = run(ctx, val, key, keys, mask=mask, zones=zones, old=True)
    assert r.tobytes() == o_r.tobytes() and c.tobytes() == o_c.tobytes()


# ---- 2. tier boundaries and strides -----------------------------------------------------------------------------------------------------------------------------
TIER_KEYS = [("f64", 1025), ("f64", 4096), ("f64", 4097), ("f64", 12289), ("f32", 1025), ("f32", 8192), ("f32", 8193), ("f32", 24577)]


@pytest.mark.parametrize("dtype,K", TIER_KEYS)
def test_tier_boundaries_and_strides_every_pattern_and_bitmap(ctx, dtype, K):
    """strides 1, 1, 2 and 4; with stride 4 the last slice of the list is not full ((K - 1) % 4 == 0: the last pivot is the last key)"""
    assert stride_of(dtype, K) == {("f64", 1025): 1, ("f64", 4096): 1, ("f64", 4097): 2, ("f64", 12289): 4, ("f32", 1025): 1, ("f32", 8192): 1, ("f32", 8193): 2,
                                   ("f32", 24577): 4}[(dtype, K)]
    n = 32
    val, xv = value_column(ctx, dtype, "mixed", n)
    keys = key_list(K, xv.dtype)
    for pattern in PATTERNS:
        key, xk = key_column(ctx, pattern, n, K, xv.dtype)
        for mname, mask in bitmaps(n, 21 + K).items():
            trace = torch.zeros(4, dtype=torch.int64, device=DEV)
            r, c = check(ctx, val, xv, key, xk, keys, mask, f"{dtype}, {n} vectors, {K} keys, {pattern}, bitmap {mname}", trace=trace)
            if mname == "all zero":
                assert not c.any() and (r == np.array(EMPTY, xv.dtype)).all() and trace.tolist() == [n, 0, 0, 0], "nothing selected: every vector is skipped"
            elif mname == "none":
                assert trace.tolist() == [0, 0, 0, n]


@pytest.mark.parametrize("dtype,K", TIER_KEYS)
def test_every_key_of_the_list_is_matched_once(ctx, dtype, K):
    """the pool tiled over ceil((K + 3) / 1024) vectors: every key of the list has a row, so every position of every slice of the pivot search is
    reached; a key the search missed would keep the empty record"""
    dt = DTYPES[dtype]
    n = -(-(K + 3) // 1024)
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = encoded(ctx, ("every key once", dtype, K), lambda: key_pool(K, dt)[np.arange(n * 1024) % (K + 3)])
    keys = key_list(K, dt)
    for mname, mask in bitmaps(n, 33 + K).items():
        trace = torch.zeros(4, dtype=torch.int64, device=DEV)
        r, c = check(ctx, val, xv, key, xk, keys, mask, f"{dtype}, every key once, {K} keys, bitmap {mname}", trace=trace)
        want_r, _ = host_keyed_minmax_many(xv, xk, bits_of(mask, xv.size), keys)
        empty_got, empty_want = (r == np.array(EMPTY, dt)).all(axis=1), (want_r == np.array(EMPTY, dt)).all(axis=1)
        assert np.array_equal(empty_got, empty_want), f"bitmap {mname}: {int((empty_got & ~empty_want).sum())} keys kept the empty record against the replica"
        if mname == "none":
            assert (c[:K] >= 1).all() and int(c[K]) == xv.size - int(c[:K].sum()) and int(c[K]) > 0, "every key has a row, and the three keys left out have theirs"
        if mname == "all zero":
            assert trace.tolist() == [n, 0, 0, 0] and empty_got.all()


# ---- 3. the bound -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_two_to_the_twenty_keys_with_and_without_the_zone_map(ctx, dtype):
    K, n = capi.KEYED_MANY_KEYS_MAX, 64
    assert K == 1 << 20
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    keys = key_list(K, xv.dtype)
    assert keys.size == K and np.unique(keys).size == K, "the float pool is exact up to 2^18: 2^20 distinct keys"
    mask = random_mask(n, 77)
    plain = check(ctx, val, xv, key, xk, keys, mask, f"{dtype}, 2^20 keys")
    r, c = check(ctx, val, xv, key, xk, keys, mask, f"{dtype}, 2^20 keys, the zone map", zones=ctx.zone_map(key))
    assert r.tobytes() == plain[0].tobytes() and c.tobytes() == plain[1].tobytes()
    assert int((c[:K] > 0).sum()) > 1024 and int(c[K]) >= 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_one_key_more_and_no_key_are_invalid_and_write_nothing(ctx, dtype):
    n = 3
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = key_column(ctx, "random", n, 64, xv.dtype)
    K = capi.KEYED_MANY_KEYS_MAX + 1
    tdt = torch.float64 if dtype == "f64" else torch.float32
    keys = torch.zeros(K, dtype=tdt, device=DEV)
    out = torch.full((K, 2), 7.5, dtype=tdt, device=DEV)
    cnt = torch.full((K + 1,), POISON, dtype=torch.int64, device=DEV)
    trace = torch.full((4,), POISON, dtype=torch.int64, device=DEV)
    fn, dbg = getattr(capi.lib, "alpgpu_decode_keyed_minmax_many_" + dtype), getattr(capi.lib, "alpgpu_debug_decode_keyed_minmax_many_" + dtype)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    v, k = ctypes.byref(val.c), ctypes.byref(key.c)
    for bad in (0, K, 2**32 - 1):
        assert fn(ctx.h, v, k, None, None, p(keys), bad, p(out), p(cnt)) == -2, f"n_keys = {bad} must be refused"
        assert dbg(ctx.h, v, k, None, None, p(keys), bad, p(out), p(cnt), None, p(trace)) == -2, f"n_keys = {bad} must be refused by the debug entry"
    ctx.synchronize()
    assert bool((out == 7.5).all()) and bool((cnt == POISON).all()) and bool((trace == POISON).all()), "a refused call wrote"
    with pytest.raises(ValueError):
        ctx.keyed_minmax_many_into(val, key, keys, out, counts_out=cnt)
    with pytest.raises(ValueError):
        ctx.keyed_minmax_many(val, key, keys)
    with pytest.raises(ValueError):  # 1025 keys are still refused by the existing call
        ctx.keyed_minmax_into(val, key, keys[:1025], out[:1025], counts_out=cnt[:1026])
    assert getattr(capi.lib, "alpgpu_decode_keyed_minmax_" + dtype)(ctx.h, v, k, None, None, p(keys), 1025, p(out), p(cnt)) == -2
    ctx.synchronize()
    assert bool((out == 7.5).all()) and bool((cnt == POISON).all())
    # the accepted call at K - 1 = 2^20 fills exactly its records and counts (a column of no vectors: the init kernel alone)
    empty = capi.CColumn()
    assert fn(ctx.h, ctypes.byref(empty), ctypes.byref(empty), None, None, p(keys), K - 1, p(out), p(cnt)) == 0
    ctx.synchronize()
    assert bool((out[: K - 1, 0] == INF).all()) and bool((out[: K - 1, 1] == -INF).all()) and out[K - 1].tolist() == [7.5, 7.5]
    assert not bool(cnt[:K].any()) and int(cnt[K]) == POISON


# ---- 4. the grid does not enter the result ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,kind", [("f64", "mixed"), ("f64", "rd"), ("f32", "mixed"), ("f32", "rd")])
def test_grids_of_1_7_the_default_and_1000_give_the_same_bytes(ctx, dtype, kind):
    n, K = 250, GLOBAL_K[dtype]
    val, xv = value_column(ctx, dtype, kind, n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    keys = key_list(K, xv.dtype)
    mask = random_mask(n, 71)
    want_r, want_c = host_keyed_minmax_many(xv, xk, unpack_np(mask, xv.size), keys)
    runs = []
    for tuning in ({"grid": 1}, {"grid": 7}, None, {"grid": 1000}):  # one workgroup: 32 trips per wavefront; more workgroups than there is work for
        trace = torch.zeros(4, dtype=torch.int64, device=DEV)
        r, c = run(ctx, val, key, keys, mask=mask, tuning=tuning, trace=trace)
        assert same_records(r, want_r) and np.array_equal(c, want_c), f"tuning {tuning}"
        assert trace.tolist() == [0, 0, 0, n]
        runs.append(r.tobytes() + c.tobytes())
    assert len(set(runs)) == 1
    r, c = run(ctx, val, key, keys, mask=mask, counts=False)  # without counts: the same records
    assert c is None and same_records(r, want_r)


# ---- 5. a second trip at the default grid -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_second_trip_at_the_default_grid(ctx, dtype):
    """8193 vectors are more than 2 x 256 workgroups of 8 wavefronts hold at once: wavefronts make a second trip at the default grid.  A sparse
    bitmap keeps the replica quick."""
    n, K = 8193, GLOBAL_K[dtype]
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    mask = vectors_cleared(random_mask(n, 31, ands=3), 3)
    check(ctx, val, xv, key, xk, key_list(K, xv.dtype), mask, f"{dtype}, {n} vectors, {K} keys")


# ---- 6. zone records in the pivot tier --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,kind", [("f64", "mixed"), ("f32", "rd")])
def test_truthful_and_widened_records_change_no_byte_and_constant_keys_are_settled(ctx, dtype, kind):
    n, K = 250, GLOBAL_K[dtype]
    val, xv = value_column(ctx, dtype, kind, n)
    for pattern in ("constant per vector", "random", "two keys by lane"):
        key, xk = key_column(ctx, pattern, n, K, xv.dtype)
        _, vec, _, _ = key.to_host()
        keys = key_list(K, xv.dtype)
        zones = ctx.zone_map(key)
        holes = zones.clone()
        holes[::3, 0] = NAN  # a NaN bound prunes nothing
        for mname, mask in (("none", None), ("vectors zero", vectors_cleared(random_mask(n, 81), 3))):
            sel_any = bits_of(mask, xv.size).reshape(n, 1024).any(axis=1)
            plain = check(ctx, val, xv, key, xk, keys, mask, f"{dtype} {kind}, {pattern}: without zones")
            for zname, z in (("the zone map", zones), ("widened", widened(zones)), ("NaN bounds", holes)):
                trace = torch.zeros(4, dtype=torch.int64, device=DEV)
                r, c = run(ctx, val, key, keys, mask=mask, zones=z, trace=trace)
                assert same_records(r, plain[0]) and c.tobytes() == plain[1].tobytes(), f"{dtype} {kind}, {pattern}, bitmap {mname}: {zname} changed the result"
                zz = z.cpu().numpy()
                ok = ~np.isnan(zz).any(axis=1)
                j0 = np.searchsorted(keys, np.where(ok, zz[:, 0], 0), side="left")
                j1 = np.searchsorted(keys, np.where(ok, zz[:, 1], 0), side="right")
                no_key = sel_any & ok & (j1 <= j0)
                const = sel_any & ok & (j1 > j0) & (zz[:, 0] == zz[:, 1]) & (vec["scheme"] == capi.SCHEME_ALP) & (vec["exc_cnt"] == 0)
                t = trace.tolist()
                assert t == [n - int(sel_any.sum()), int(const.sum()), int(no_key.sum()), int(sel_any.sum()) - int(const.sum()) - int(no_key.sum())], f"{pattern}, {zname}: trace {t}"
                if pattern == "constant per vector" and zname == "the zone map":
                    per_vector = xk.reshape(n, 1024)
                    constant = (per_vector == per_vector[:, :1]).all(axis=1) & np.isin(per_vector[:, 0], keys)  # (from the values, not from the records)
                    plain_alp = (vec["scheme"] == capi.SCHEME_ALP) & (vec["exc_cnt"] == 0)  # what the shortcut asks of the descriptor: no NaN can hide
                    assert t[1] == int((constant & plain_alp & sel_any).sum()) > int(sel_any.sum()) // 2, "every constant ALP vector with a selected row and a key is settled by the shortcut"
                    # (3 of the pool's K + 3 values are no keys: at this K no constant vector draws one; the no-key class has the test below)
                if pattern == "constant per vector" and zname == "widened":
                    assert t[1] == 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_column_whose_records_admit_no_key_is_rows_without_a_key(ctx, dtype):
    dt = DTYPES[dtype]
    n, K = 250, GLOBAL_K[dtype]
    val, xv = value_column(ctx, dtype, "mixed", n)
    pool = key_pool(K, dt)
    key, xk = encoded(ctx, ("no key", dtype, K), lambda: np.where(np.arange(n * 1024) % 2 == 0, pool[0], pool[K + 2]))
    keys = key_list(K, dt)
    outside = np.concatenate([keys[keys < pool[0]], keys[keys > pool[K + 2]]])
    assert outside.size == 0 and pool[0] < keys[0] and pool[K + 2] > keys[-1], "both values of the key column lie outside the list"
    # every record is {pool[0], pool[K + 2]}: it admits EVERY key, nothing is pruned; only the search finds that no row has one
    mask = vectors_cleared(random_mask(n, 83), 3)
    sel_any = bits_of(mask, xv.size).reshape(n, 1024).any(axis=1)
    trace = torch.zeros(4, dtype=torch.int64, device=DEV)
    r, c = check(ctx, val, xv, key, xk, keys, mask, "a record that admits every key", zones=ctx.zone_map(key), trace=trace)
    assert trace.tolist() == [n - int(sel_any.sum()), 0, 0, int(sel_any.sum())] and int(c[K]) == int(bits_of(mask, xv.size).sum())
    # the same rows under records that admit no key: one constant below the list per vector
    low, xl = encoded(ctx, ("below the list", dtype, K), lambda: np.full(n * 1024, pool[0], dt))
    trace = torch.zeros(4, dtype=torch.int64, device=DEV)
    r, c = check(ctx, val, xv, low, xl, keys, mask, "records that admit no key", zones=ctx.zone_map(low), trace=trace)
    assert trace.tolist() == [n - int(sel_any.sum()), 0, int(sel_any.sum()), 0], "neither column is read"
    assert int(c[K]) == int(bits_of(mask, xv.size).sum()) > 0 and not c[:K].any() and (r == np.array(EMPTY, dt)).all()
    r2, c2 = run(ctx, val, low, keys, mask=mask, zones=ctx.zone_map(low), counts=False)
    assert c2 is None and r2.tobytes() == r.tobytes()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_lying_records_and_unsorted_keys_keep_the_total_and_stay_inside_the_outputs(ctx, dtype):
    n = 250
    val, xv = value_column(ctx, dtype, "mixed", n)
    mask = random_mask(n, 91)
    n_sel = int(unpack_np(mask, xv.size).sum())
    guard = 64
    G = GLOBAL_K[dtype]
    for K, pattern in ((G, "constant per vector"), (G, "random"), (3 * LDS_MAX[dtype] + 1, "random"), (1025, "two keys by lane")):
        key, xk = key_column(ctx, pattern, n, K, xv.dtype)
        in_order = key_list(K, xv.dtype)
        unsorted = np.random.default_rng(92).permutation(in_order)
        zones = ctx.zone_map(key)
        lies = {"swapped": zones.flip(1).contiguous(), "shifted": torch.roll(zones, 7, 0).contiguous(), "a point": torch.full_like(zones, 0.25),
                "infinite": torch.stack([torch.full((n,), INF, dtype=zones.dtype, device=DEV), torch.full((n,), -INF, dtype=zones.dtype, device=DEV)], dim=1).contiguous()}
        cases = [("unsorted keys", unsorted, None), ("unsorted keys with the zone map", unsorted, zones)] + [("records: " + k, in_order, z) for k, z in lies.items()]
        for what, keys, z in cases:
            kd = torch.from_numpy(np.ascontiguousarray(keys)).to(DEV)
            rbuf = torch.full((guard + K + guard, 2), -12345.5, dtype=kd.dtype, device=DEV)
            cbuf = torch.full((guard + K + 1 + guard,), POISON, dtype=torch.int64, device=DEV)
            ctx.keyed_minmax_many_into(val, key, kd, rbuf[guard: guard + K], counts_out=cbuf[guard: guard + K + 1], mask=mask, zones=z)
            ctx.synchronize()
            assert bool((rbuf[:guard] == -12345.5).all()) and bool((rbuf[guard + K:] == -12345.5).all()), f"{what}, {K} keys: words beside the records changed"
            assert bool((cbuf[:guard] == POISON).all()) and bool((cbuf[guard + K + 1:] == POISON).all()), f"{what}, {K} keys: words beside the counts changed"
            counts = cbuf[guard: guard + K + 1]
            assert bool((counts >= 0).all()) and int(counts.sum()) == n_sel, f"{what}, {K} keys: the total is the selected count"
            assert not bool(torch.isnan(rbuf).any())


# ---- 7. values and keys -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_duplicates_both_zeros_and_nans_in_the_key_list(ctx, dtype):
    dt = DTYPES[dtype]
    n, K = 32, GLOBAL_K[dtype] - 7
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = key_column(ctx, "random", n, K, dt)
    assert (xk == 0).any()
    base = key_list(K, dt)
    keys = np.sort(np.concatenate([base, base[10:14], base[K - 3: K - 1], np.array([-0.0], dt)]))  # duplicates, and -0.0 beside +0.0 (numpy.sort keeps either order)
    keys = np.concatenate([keys, np.array([NAN, NAN], dt)])  # NaNs last: never matched
    assert keys.size > GLOBAL_K[dtype]
    r, c = check(ctx, val, xv, key, xk, keys, random_mask(n, 51), "duplicates, zeros, NaNs in the list")
    first_zero = int(np.flatnonzero(keys == 0)[0])
    assert c[first_zero] > 0 and c[first_zero + 1] == 0 and r[first_zero + 1].tolist() == EMPTY
    assert c[-3] == 0 and c[-2] == 0 and r[-1].tolist() == EMPTY and r[-2].tolist() == EMPTY
    dup = np.flatnonzero(keys[1:] == keys[:-1]) + 1
    assert dup.size >= 7 and not c[dup].any() and r[dup].tolist() == [EMPTY] * dup.size, "later duplicates receive nothing"
    assert (c[dup - 1] > 0).any()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_nan_keys_and_nan_values_in_the_columns(ctx, dtype):
    dt = DTYPES[dtype]
    n, K = 32, GLOBAL_K[dtype]
    pool = key_pool(K, dt)

    def make_key():
        k = pool[np.random.default_rng(61).integers(0, K + 3, n * 1024)].copy()
        k[::7] = NAN  # exceptions of ALP vectors
        return k

    def make_rd_key():
        k = np.random.default_rng(62).random(n * 1024).astype(dt)
        k[::3] = NAN  # an ALP_RD vector holds them in its packed words
        return k
    keys = key_list(K, dt)
    lonely = keys[K // 2]  # a key whose rows all hold NaN values

    def make_val():
        x = np.round(np.random.default_rng(63).normal(0, 100, n * 1024), 2).astype(dt)
        x[5::64] = NAN
        x[6::64] = INF
        x[7::64] = -INF
        x[make_key() == lonely] = NAN
        return x
    key, xk = encoded(ctx, ("kmany nan key", dtype), make_key)
    val, xv = encoded(ctx, ("kmany nan val", dtype), make_val)
    assert (xk == lonely).any()
    r, c = check(ctx, val, xv, key, xk, keys, None, "NaN keys, NaN values")
    assert r[K // 2].tolist() == EMPTY and c[K // 2] > 0, "a key whose rows are all NaN: the empty record, counted"
    assert int(c[-1]) >= int(np.isnan(xk).sum()) and (r[:, 1] == INF).any() and (r[:, 0] == -INF).any()
    check(ctx, val, xv, key, xk, keys, vectors_cleared(random_mask(n, 64), 2), "NaN keys, NaN values, a bitmap")
    rdk, xrk = encoded(ctx, ("kmany rd nan key", dtype), make_rd_key)
    _, vec, _, _ = rdk.to_host()
    assert (vec["scheme"] == capi.SCHEME_ALP_RD).all()
    real = np.unique(xrk[~np.isnan(xrk)])
    assert real.size > GLOBAL_K[dtype]
    r, c = check(ctx, val, xv, rdk, xrk, real[: 2 * GLOBAL_K[dtype]: 2].copy(), None, "an ALP_RD key column with NaNs")
    assert int(c[-1]) >= int(np.isnan(xrk).sum()) and int(c[:-1].sum()) >= GLOBAL_K[dtype]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_both_zeros_under_one_key_in_vectors_of_different_workgroups(ctx, dtype):
    """key 1.0 meets +0.0 in vector 0 and -0.0 in vector 240, key 2.0 the opposite order; every other row has a key that is not in the list.  The
    record is {-0.0, +0.0} by its bits: a guard that compared with C's < would drop the zero that arrives second."""
    dt = DTYPES[dtype]
    n = 250
    second = 240 * 1024 + 9

    def make_val():
        x = np.full(n * 1024, 7.25, dt)
        x[3], x[second] = 0.0, -0.0  # key 1.0
        x[4], x[second + 1] = -0.0, 0.0  # key 2.0
        return x

    def make_key():
        k = np.full(n * 1024, -7.0, dt)
        k[[3, second]] = 1.0
        k[[4, second + 1]] = 2.0
        return k
    val, xv = encoded(ctx, ("many zeros val", dtype), make_val)
    key, xk = encoded(ctx, ("many zeros key", dtype), make_key)
    keys = np.arange(1, GLOBAL_K[dtype] + 1).astype(dt)  # 1.0, 2.0, ...: the pivot tier
    for zones in (None, ctx.zone_map(key)):
        for tuning in (None, {"grid": 1}):
            r, c = check(ctx, val, xv, key, xk, keys, None, f"{dtype}, zones {zones is not None}, tuning {tuning}", zones=zones, tuning=tuning)
            for i in (0, 1):
                assert r[i].tolist() == [0.0, 0.0] and np.signbit(r[i, 0]) and not np.signbit(r[i, 1]), f"key {keys[i]}: min is -0.0 and max is +0.0"
            assert r[2].tolist() == EMPTY and c[:3].tolist() == [2, 2, 0] and int(c[-1]) == n * 1024 - 4


@pytest.mark.parametrize("dtype,kind", [("f64", "mixed"), ("f64", "rd"), ("f32", "mixed"), ("f32", "rd")])
def test_a_column_as_its_own_key_with_its_distinct_values_as_the_list(ctx, dtype, kind):
    n = 32
    val, xv = value_column(ctx, dtype, kind, n)
    real = np.unique(xv[~np.isnan(xv)])  # (numpy's: -0.0 and +0.0 are one value here too)
    assert real.size > 1024
    for mname, mask in masks_of(n, 41).items():
        sel = xv[bits_of(mask, xv.size)]
        want_keys = np.unique(sel[~np.isnan(sel)])
        vals, cnts, n_nan, overflow = ctx.distinct(val, mask=mask, capacity=capi.KEYED_MANY_KEYS_MAX)
        keys = vals.cpu().numpy()
        assert not overflow and np.array_equal(keys, want_keys) and keys.size > 1024, "the list is the column's distinct selected values (held to numpy's here)"
        r, c = check(ctx, val, xv, val, xv, keys, mask, f"{dtype} {kind} as its own key, bitmap {mname}")
        assert int(c[-1]) == n_nan == int(np.isnan(sel).sum()), "only the NaNs have no key"
        assert np.array_equal(c[:-1], cnts.cpu().numpy()), "distinct's counts on the same selection are these counts: d_counts == NULL is the usual call"
        zero = keys == 0
        assert (r[~zero, 0] == keys[~zero]).all() and (r[~zero, 1] == keys[~zero]).all(), "a key's record is the key itself"
        r2, c2 = run(ctx, val, val, keys, mask=mask, counts=False)
        assert c2 is None and r2.tobytes() == r.tobytes()


# ---- 8. hand-built vectors --------------------------------------------------------------------------------------------------------------------------------------
class Columns:
    """the rows of double_rows.py / float_rows.py as value and key columns, in vector order (A) and with their records shuffled in the streams (S).
    The rows hold several million distinct values, more than one call takes, so the vectors are dealt into G = ceil(nv / 1024) groups (v % G): a
    group's list is EVERY distinct non-NaN value of its at most 2^20 key rows, and its bitmap selects its vectors alone.  The G calls together read
    every vector, each against all of its own values."""

    def __init__(self, ctx, dtype):
        from oracle.pyoracle import Oracle, OracleF32
        import test_histogram_rows_gpu as hr
        import double_rows as dr
        import float_rows as fr
        rows, oracle = (dr, Oracle()) if dtype == "f64" else (fr, OracleF32())
        self.dtype = dtype
        enc = fr.concat_encodings([rows.alp_rows(), rows.rd_rows()])
        self.A = hr.Built(ctx, oracle, enc, dtype)
        self.S = hr.Built(ctx, oracle, enc, dtype, shuffle_seed=31)
        self.nv = self.A.nv
        self.G = -(-self.nv // 1024)
        rnd = hr.random_mask(self.nv, 53)
        every = torch.full((16 * self.nv,), -1, dtype=torch.int64, device=DEV)
        self.masks = {"none": every, "random": rnd, "cleared": hr.vectors_cleared(rnd, 3)}
        self.unpack = hr.unpack
        self.keys = {}

    def group(self, g, mname):
        """(the group's keys, its bitmap on the device, the bitmap's bits [nv, 1024])"""
        mine = (torch.arange(self.nv, device=DEV) % self.G) == g
        mask = (self.masks[mname].reshape(-1, 16) * mine[:, None].to(torch.int64)).reshape(-1).contiguous()
        if g not in self.keys:
            flat = self.A.values[g:: self.G].reshape(-1)
            self.keys[g] = np.unique(flat[~np.isnan(flat)])  # (+-inf and one of the zeros among them, if the rows hold them)
        return self.keys[g], mask, self.unpack(mask.cpu().numpy(), self.nv)


@pytest.fixture(scope="module", params=["f64", "f32"])
def cols(ctx, request):
    return Columns(ctx, request.param)


@pytest.mark.parametrize("mname", ["none", "random", "cleared"])
def test_keyed_minmax_many_of_the_hand_built_rows_by_all_their_own_values(ctx, cols, mname):
    matched = without = 0
    for g in range(cols.G):
        keys, mask, bits = cols.group(g, mname)
        assert 1024 < keys.size <= capi.KEYED_MANY_KEYS_MAX, "the list is longer than keyed_minmax_into takes"
        want_r, want_c = host_keyed_minmax_many(cols.A.want, cols.A.want, bits.reshape(-1), keys)
        selected = int(bits.any(axis=1).sum())
        for name, val, key in (("A by A", cols.A, cols.A), ("A by S", cols.A, cols.S), ("S by A", cols.S, cols.A)):
            trace = torch.zeros(4, dtype=torch.int64, device=DEV)
            got_r, got_c = run(ctx, val.col, key.col, keys, mask=mask, trace=trace)
            what = f"{cols.dtype} {name}, group {g} of {cols.G}, {keys.size} keys, bitmap {mname}"
            assert np.array_equal(got_c, want_c), f"{what}: counts are not the oracle's decode through the replica"
            assert same_records(got_r, want_r), f"{what}: records are not the oracle's decode through the replica"
            assert trace.tolist() == [cols.nv - selected, 0, 0, selected], "every vector with a selected bit is decoded, both columns"
        assert int(want_c[-1]) == int(np.isnan(cols.A.want[bits.reshape(-1)]).sum()), "only the NaNs have no key"
        matched, without = matched + int(want_c[:-1].sum()), without + int(want_c[-1])
    assert matched > 0 and without > 0, "rows with and without a key are selected"


# ---- 9. capture -------------------------------------------------------------------------------------------------------------------------------------------------
CAPTURE = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
import datagen
from alp_amd import capi
from keyed_many_replica import host_keyed_minmax_many
from keyed_minmax_replica import same_records
ctx = capi.Context(0)
side = torch.cuda.Stream()
ok = True
nv = 230
def bitmap(seed):
    return np.random.default_rng(seed).integers(0, 2**64, 16 * nv, dtype=np.uint64)
def bits_of(words):
    return ((words[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)
for dt, make, K in ((np.float64, datagen.mixed_column, 4097), (np.float32, datagen.mixed_column_f32, 8193)):
    rng = np.random.default_rng(5)
    xv = make(nv, seed=81)
    pool = ((np.arange(K + 3) - 5) * 0.25).astype(dt)
    xk = pool[rng.integers(0, K + 3, nv * 1024)]
    keys = np.sort(np.delete(pool, [0, 30, K + 2]))
    other = np.sort(np.delete(pool, [1, 2, 3]))               # the keys' contents after the capture: the same length, other values
    val, key = ctx.encode(torch.from_numpy(xv).cuda()), ctx.encode(torch.from_numpy(xk).cuda())
    kd = torch.from_numpy(keys).cuda()
    words = bitmap(6)
    mask = torch.from_numpy(words.view(np.int64)).cuda()
    out = torch.zeros((K, 2), dtype=kd.dtype, device="cuda:0")
    cnt = torch.zeros(K + 1, dtype=torch.int64, device="cuda:0")
    def calls():
        ctx.keyed_minmax_many_into(val, key, kd, out, counts_out=cnt, mask=mask)
    with torch.cuda.stream(side):
        calls()                                                 # warm-up on the capture stream
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            calls()
    for rep in range(4):
        if rep == 2:
            words = bitmap(7)                                   # the third replay after the bitmap changed
            mask.copy_(torch.from_numpy(words.view(np.int64)).cuda())
        if rep == 3:
            keys = other                                        # the fourth after the keys' contents changed
            kd.copy_(torch.from_numpy(keys).cuda())
        torch.cuda.synchronize()
        out.fill_(float(rep) - 1.0); cnt.fill_(rep - 1)
        g.replay()
        torch.cuda.synchronize()
        wr, wc = host_keyed_minmax_many(xv, xk, bits_of(words), keys)
        ok = ok and same_records(out.cpu().numpy(), wr) and np.array_equal(cnt.cpu().numpy(), wc) and int(wc.sum()) > 0
        print(dt.__name__, rep, int(wc.sum()), int(wc[-1]), ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_keys_and_the_bitmap_changed():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 10. the allocating wrapper and the C++ surface -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_allocating_wrapper_sorts_its_keys(ctx, dtype):
    n, K = 32, GLOBAL_K[dtype]
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    keys = key_list(K, xv.dtype)
    mask = random_mask(n, 5)
    want_r, want_c = host_keyed_minmax_many(xv, xk, unpack_np(mask, xv.size), keys)
    shuffled = np.random.default_rng(1).permutation(keys)
    tdt = torch.float64 if dtype == "f64" else torch.float32
    for form in (shuffled, torch.from_numpy(shuffled), torch.from_numpy(shuffled).to(DEV), [float(t) for t in shuffled]):
        r, c, u = ctx.keyed_minmax_many(val, key, form, mask=mask, zones=ctx.zone_map(key))
        assert r.dtype == tdt and c.dtype == torch.int64 and tuple(r.shape) == (K, 2) and c.numel() == K
        assert same_records(r.cpu().numpy(), want_r) and np.array_equal(c.cpu().numpy(), want_c[:K]) and int(u) == int(want_c[K])
    r, c, u = ctx.keyed_minmax_many(val, key, torch.from_numpy(keys).to(DEV), mask=mask, counts=False)
    assert c is None and u is None and same_records(r.cpu().numpy(), want_r)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cpp_column_minmax_by_key_many_against_decompress_and_a_host_loop(ctx, tmp_path, dtype):
    """include/alp/batch.hpp: alp::gpu::column<PT>::minmax_by_key_many of two serialized columns against column::decompress and a host loop
    (tests/cpp/keyed_minmax_many_test.cpp)"""
    exe = tmp_path / "keyed_minmax_many_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/keyed_minmax_many_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    n, K = 250, GLOBAL_K[dtype]
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    ctx.to_blob(val, xv.size).tofile(str(tmp_path / "val.blob"))
    ctx.to_blob(key, xk.size).tofile(str(tmp_path / "key.blob"))
    keys = key_list(K, xk.dtype)
    np.random.default_rng(2).permutation(keys).tofile(str(tmp_path / "keys.bin"))  # (the wrapper sorts)
    mask = vectors_cleared(random_mask(n, 53), 3)
    mask[16:32] = -1
    mask.cpu().numpy().tofile(str(tmp_path / "in.mask"))
    p = subprocess.run([str(exe), dtype] + [str(tmp_path / f) for f in ("val.blob", "key.blob", "keys.bin", "in.mask")], capture_output=True, text=True, timeout=600)
    line = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("ok ")]
    assert p.returncode == 0 and len(line) == 1, p.stdout[-3000:] + p.stderr[-2000:]
    k = int(unpack_np(mask, xv.size).sum())
    assert int(line[0][1]) == n and int(line[0][2]) == k and 0 < k < xv.size and int(line[0][3]) == K and int(line[0][4]) > 1024
