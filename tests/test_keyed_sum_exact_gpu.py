"""GPU: the exact keyed SUM (include/alpgpu.h, "exact keyed SUM": alpgpu_decode_keyed_exact_sum_*), double and float.  No expectation comes from the code
under test: the columns' values are the arrays that were encoded (the store decode is held to them bit for bit where they are encoded), the sums come
from tests/keyed_exact_replica.py (keyed_many_replica's match; Python integers rounded once by int / int), the trace's two arms from a host count of
the steps that meet the documented condition.  Sums compare as bytes, counts as integers; every output is poisoned before the call and the table is
filled with ones, so a call that did not zero it would be wrong.  Columns, key patterns, key lists and bitmaps are tests/test_keyed_gpu.py's."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from alp_amd import capi
from keyed_exact_replica import host_keyed_sum_exact
from keyed_many_replica import match_many
from test_keyed_gpu import PATTERNS, POISON, encoded, key_column, key_list, key_pool, masks_of, random_mask, unpack_np, vectors_cleared
from test_keyed_minmax_gpu import value_column

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF, NAN = math.inf, math.nan
DTYPES = {"f64": np.float64, "f32": np.float32}
DBL_MAX, FLT_MAX = 1.7976931348623157e308, 3.4028234663852886e38
GLOBAL_K = {"f64": 4097, "f32": 8193}  # the shortest list of the pivot tier
_wanted = {}


def bitmaps(n, seed):
    m = masks_of(n, seed)
    return {"none": None, "random": m["random"], "vectors zero": m["vectors zero"], "all zero": torch.zeros(16 * n, dtype=torch.int64, device=DEV)}


def bits_of(mask, total):
    return np.ones(total, bool) if mask is None else unpack_np(mask, total)


def new_table(ctx, K):
    t = ctx.keyed_sum_exact_table(K)
    t.fill_(1)  # (a table is scratch: whatever it holds, a call without accumulate starts from zero)
    return t


def run(ctx, val, key, keys, mask=None, zones=None, tuning=None, trace=None, counts=True, table=None, accumulate=False, outs=None):
    """keyed_sum_exact_into on poisoned outputs (or, accumulating, on outs = (sums, counts) of the earlier call): (sums float64[K] as numpy,
    counts int64[K + 1] as numpy or None)"""
    kd = torch.from_numpy(np.ascontiguousarray(keys)).to(DEV)
    if outs is None:
        sums = torch.full((kd.numel(),), -12345.5, dtype=torch.float64, device=DEV)
        cnt = torch.full((kd.numel() + 1,), POISON, dtype=torch.int64, device=DEV) if counts else None
    else:
        sums, cnt = outs
    ctx.keyed_sum_exact_into(val, key, kd, sums, counts_out=cnt, mask=mask, zones=zones, tuning=tuning, trace=trace, accumulate=accumulate,
                             table=new_table(ctx, kd.numel()) if table is None else table)
    return sums.cpu().numpy(), (cnt.cpu().numpy() if cnt is not None else None)


def wanted(tag, xv, xk, bits, keys):
    """the replica's (sums, counts), computed once per tag and left unchanged"""
    if tag not in _wanted:
        _wanted[tag] = host_keyed_sum_exact(xv, xk, bits, keys)
    return _wanted[tag]


def check(ctx, val, xv, key, xk, keys, mask, what, tag=None, **kw):
    bits = bits_of(mask, xv.size)
    want_s, want_c = host_keyed_sum_exact(xv, xk, bits, keys) if tag is None else wanted(tag, xv, xk, bits, keys)
    got_s, got_c = run(ctx, val, key, keys, mask=mask, **kw)
    assert np.array_equal(got_c, want_c), f"{what}: counts differ from the replica in {int((got_c != want_c).sum())} words"
    diff = got_s.view(np.uint64) != want_s.view(np.uint64)
    assert not diff.any(), f"{what}: sums differ from the replica in {int(diff.sum())} keys, first {int(np.flatnonzero(diff)[0])}: {got_s[diff][:3]} against {want_s[diff][:3]}"
    assert int(got_c.sum()) == int(bits.sum())
    return got_s, got_c


# ---- 1. values ------------------------------------------------------------------------------------------------------------------------------------------------
def hard_values(dtype, n, seed):
    """magnitudes from both ends of the exponent range beside ones, the smallest subnormal, the largest number, -0.0, decimals, a few infinities
    and NaNs: ALP takes them as exceptions or the rowgroup goes to ALP_RD"""
    dt = DTYPES[dtype]
    rng = np.random.default_rng(seed)
    big, tiny, top = (1e300, 2.0 ** -1074, DBL_MAX) if dtype == "f64" else (1e30, 2.0 ** -149, FLT_MAX)
    pool = np.array([big, -big, 1.0, -1.0, tiny, -tiny, top, -top, -0.0, 0.0, 0.1, 123.45, -7.25, 1e-5, 65536.5, -3.0e10, big / 3, -tiny * 5], dt)
    x = pool[rng.integers(0, pool.size, n * 1024)].copy()
    decimal = rng.random(n * 1024) < 0.4
    x[decimal] = np.round(rng.normal(0, 1000, int(decimal.sum())), 2).astype(dt)
    odd = rng.choice(n * 1024, 9, replace=False)
    x[odd] = np.array([INF, -INF, NAN, INF, NAN, -INF, INF, INF, -INF], dt)
    return x


@pytest.mark.parametrize("K", [1, 64, 1024])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_hard_values_every_pattern_and_bitmap(ctx, dtype, K):
    n = 3
    dt = DTYPES[dtype]
    val, xv = encoded(ctx, ("exact hard", dtype, n), lambda: hard_values(dtype, n, 17))
    _, vec, _, _ = val.to_host()
    assert (vec["exc_cnt"] > 0).any() or (vec["scheme"] == capi.SCHEME_ALP_RD).any(), "the values are stored as exceptions or as ALP_RD"
    keys = key_list(K, dt)
    seen_nan = seen_inf = seen_number = False
    for pattern in PATTERNS:
        key, xk = key_column(ctx, pattern, n, K, dt)
        for mname, mask in bitmaps(n, 21 + K).items():
            trace = torch.zeros(6, dtype=torch.int64, device=DEV)
            s, c = check(ctx, val, xv, key, xk, keys, mask, f"{dtype}, {n} vectors, {K} keys, {pattern}, bitmap {mname}", trace=trace)
            seen_nan, seen_inf, seen_number = seen_nan or bool(np.isnan(s).any()), seen_inf or bool(np.isinf(s).any()), seen_number or bool((np.isfinite(s) & (s != 0)).any())
            assert not np.signbit(s[s == 0]).any(), "no sum is -0.0"
            if mname == "all zero":
                assert s.view(np.uint64).tolist() == [0] * K and not c.any() and trace.tolist() == [n, 0, 0, 0, 0, 0], "nothing selected: every vector is skipped, every sum +0.0"
            elif mname == "none":
                assert trace.tolist()[:4] == [0, 0, 0, n]
    assert seen_number and (seen_nan or seen_inf)
    zones = ctx.zone_map(key)  # (the last pattern's) ... and with the key column's zone map
    plain = run(ctx, val, key, keys, mask=mask)
    zoned = run(ctx, val, key, keys, mask=mask, zones=zones)
    assert plain[0].tobytes() == zoned[0].tobytes() and plain[1].tobytes() == zoned[1].tobytes()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_single_keys_that_cancel_overflow_and_see_nans_and_infinities(ctx, dtype):
    """nine keys of the list receive exactly the rows named here, spread over vectors and lanes; every other row has another key"""
    dt = DTYPES[dtype]
    n, K = 3, 64
    keys = key_list(K, dt)
    big, top = (1e300, DBL_MAX) if dtype == "f64" else (1e30, FLT_MAX)
    tiny = 2.0 ** -1074 if dtype == "f64" else 2.0 ** -149
    cases = [([big, 1.0, -big], 1.0), ([top, top], INF if dtype == "f64" else 2.0 * FLT_MAX), ([top, top, -top], top), ([-0.0, -0.0], 0.0), ([5.0, INF, -3.0], INF),
             ([INF, 1.0, -INF], NAN), ([2.5, NAN, INF], NAN), ([tiny, tiny, tiny, 1.0, -1.0], 3 * tiny), ([-INF, -INF], -INF)]
    special = keys[3: 3 + len(cases)]

    def make_key():
        rng = np.random.default_rng(5)
        rest = np.setdiff1d(key_pool(K, dt), special)
        return rest[rng.integers(0, rest.size, n * 1024)]

    def place(base, what):
        rng = np.random.default_rng(6)
        rows = rng.choice(n * 1024, sum(len(v) for v, _ in cases), replace=False)
        out, at = base.copy(), 0
        for i, (values, _) in enumerate(cases):
            for v in values:
                out[rows[at]] = special[i] if what == "key" else v
                at += 1
        return out
    key, xk = encoded(ctx, ("exact placed key", dtype), lambda: place(make_key(), "key"))
    val, xv = encoded(ctx, ("exact placed val", dtype), lambda: place(hard_values(dtype, n, 18), "val"))
    for tuning in (None, {"grid": 1}):
        s, c = check(ctx, val, xv, key, xk, keys, None, f"{dtype}, placed rows, tuning {tuning}", tuning=tuning)
        for i, (values, want) in enumerate(cases):
            got = s[3 + i]
            assert c[3 + i] == len(values) and ((np.isnan(got) and np.isnan(want)) or (got == want and not (got == 0 and np.signbit(got)))), f"key {special[i]}: {values} sum to {got}, not {want}"


# ---- 2. tier boundaries and strides -----------------------------------------------------------------------------------------------------------------------------
TIER_KEYS = [("f64", 1025), ("f64", 4096), ("f64", 4097), ("f64", 12289), ("f32", 1025), ("f32", 8192), ("f32", 8193), ("f32", 24577)]


@pytest.mark.parametrize("dtype,K", TIER_KEYS)
def test_tier_boundaries_and_strides_every_pattern_and_bitmap(ctx, dtype, K):
    """the list whole in LDS (strides 1, 1) and its pivots there (strides 2 and 4; with stride 4 the last slice of the list is not full)"""
    n = 32
    val, xv = value_column(ctx, dtype, "mixed", n)
    keys = key_list(K, xv.dtype)
    for pattern in PATTERNS:
        key, xk = key_column(ctx, pattern, n, K, xv.dtype)
        for mname, mask in bitmaps(n, 21 + K).items():
            trace = torch.zeros(6, dtype=torch.int64, device=DEV)
            s, c = check(ctx, val, xv, key, xk, keys, mask, f"{dtype}, {n} vectors, {K} keys, {pattern}, bitmap {mname}", trace=trace)
            if mname == "all zero":
                assert not c.any() and not s.view(np.uint64).any() and trace.tolist() == [n, 0, 0, 0, 0, 0]
            elif mname == "none":
                assert trace.tolist()[:4] == [0, 0, 0, n] and trace[4] + trace[5] > 0


@pytest.mark.parametrize("dtype,K", TIER_KEYS)
def test_every_key_of_the_list_is_matched_once(ctx, dtype, K):
    """the pool tiled over ceil((K + 3) / 1024) vectors: every key of the list has a row, so every position of every slice of the pivot search is reached"""
    dt = DTYPES[dtype]
    n = -(-(K + 3) // 1024)
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = encoded(ctx, ("every key once", dtype, K), lambda: key_pool(K, dt)[np.arange(n * 1024) % (K + 3)])
    keys = key_list(K, dt)
    for mname, mask in bitmaps(n, 33 + K).items():
        s, c = check(ctx, val, xv, key, xk, keys, mask, f"{dtype}, every key once, {K} keys, bitmap {mname}")
        if mname == "none":
            assert (c[:K] >= 1).all() and int(c[K]) == xv.size - int(c[:K].sum()) and int(c[K]) > 0, "every key has a row, and the three keys left out have theirs"


# ---- 3. the bound -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_two_to_the_twenty_keys_with_and_without_the_zone_map(ctx, dtype):
    K, n = capi.KEYED_MANY_KEYS_MAX, 64
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    keys = key_list(K, xv.dtype)
    assert keys.size == K == 1 << 20 and np.unique(keys).size == K
    mask = random_mask(n, 77)
    table = new_table(ctx, K)
    plain = check(ctx, val, xv, key, xk, keys, mask, f"{dtype}, 2^20 keys", tag=("bound", dtype), table=table)
    table.fill_(255)
    s, c = check(ctx, val, xv, key, xk, keys, mask, f"{dtype}, 2^20 keys, the zone map", tag=("bound", dtype), zones=ctx.zone_map(key), table=table)
    assert s.tobytes() == plain[0].tobytes() and c.tobytes() == plain[1].tobytes()
    assert int((c[:K] > 0).sum()) > 1024


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_one_key_more_no_key_and_one_vector_more_are_invalid_and_write_nothing(ctx, dtype):
    n = 3
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = key_column(ctx, "random", n, 64, xv.dtype)
    K = capi.KEYED_MANY_KEYS_MAX + 1
    tdt = torch.float64 if dtype == "f64" else torch.float32
    keys = torch.zeros(K, dtype=tdt, device=DEV)
    sums = torch.full((K,), 7.5, dtype=torch.float64, device=DEV)
    cnt = torch.full((K + 1,), POISON, dtype=torch.int64, device=DEV)
    trace = torch.full((6,), POISON, dtype=torch.int64, device=DEV)
    table = torch.full((4096,), 9, dtype=torch.int64, device=DEV)
    fn, dbg = getattr(capi.lib, "alpgpu_decode_keyed_exact_sum_" + dtype), getattr(capi.lib, "alpgpu_debug_decode_keyed_exact_sum_" + dtype)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    v, k = ctypes.byref(val.c), ctypes.byref(key.c)
    for acc in (0, 1):
        for bad in (0, K, 2**32 - 1):
            assert fn(ctx.h, v, k, None, None, p(keys), bad, p(sums), p(cnt), p(table), acc) == -2, f"n_keys = {bad} must be refused"
            assert dbg(ctx.h, v, k, None, None, p(keys), bad, p(sums), p(cnt), p(table), acc, None, p(trace)) == -2, f"n_keys = {bad} must be refused by the debug entry"
        long = capi.CColumn()
        ctypes.memmove(ctypes.byref(long), ctypes.byref(val.c), ctypes.sizeof(capi.CColumn))
        long.n_vectors = capi.KEYED_EXACT_VECTORS_MAX + 1  # (refused before any descriptor is followed)
        assert fn(ctx.h, ctypes.byref(long), ctypes.byref(long), None, None, p(keys), 4, p(sums), p(cnt), p(table), acc) == -2, "2^21 + 1 vectors must be refused"
        assert b"ALPGPU_KEYED_EXACT_VECTORS_MAX" in capi.lib.alpgpu_last_error()
        assert dbg(ctx.h, ctypes.byref(long), ctypes.byref(long), None, None, p(keys), 4, p(sums), p(cnt), p(table), acc, None, p(trace)) == -2
        assert fn(ctx.h, v, k, None, None, p(keys), 4, p(sums), p(cnt), ctypes.c_void_p(table.data_ptr() + 8), acc) == -2, "a table that is not 16-byte aligned"
        assert fn(ctx.h, v, k, None, None, p(keys), 4, p(sums), p(cnt), None, acc) == -2, "no table"
    ctx.synchronize()
    assert bool((sums == 7.5).all()) and bool((cnt == POISON).all()) and bool((trace == POISON).all()) and bool((table == 9).all()), "a refused call wrote"
    with pytest.raises(ValueError):
        ctx.keyed_sum_exact_into(val, key, keys, sums, counts_out=cnt)
    with pytest.raises(ValueError):
        ctx.keyed_sum_exact(val, key, keys)
    # the accepted call at 2^20 keys on a column of no vectors: the zero kernel and the rounding kernel alone write exactly the sums and counts
    empty = capi.CColumn()
    big = ctx.keyed_sum_exact_table(K - 1)
    big.fill_(3)
    assert fn(ctx.h, ctypes.byref(empty), ctypes.byref(empty), None, None, p(keys), K - 1, p(sums), p(cnt), p(big), 0) == 0
    ctx.synchronize()
    assert not bool(sums[: K - 1].view(torch.int64).any()) and float(sums[K - 1]) == 7.5 and not bool(cnt[:K].any()) and int(cnt[K]) == POISON and not bool(big.any())


# ---- 4. both arms, by the trace -----------------------------------------------------------------------------------------------------------------------------------
def expected_arms(xv, xk, bits, keys):
    """(steps summed in registers, steps sent lane by lane) of a call without zone records, from the documented condition: a step of 64 rows with a
    selected, matched row goes through registers if those rows agree on their key and the first limbs of their non-zero finite values span at most 3"""
    idx, matched = match_many(xk, keys)
    m = (bits & matched).reshape(-1, 64)
    idx = idx.reshape(-1, 64)
    x = xv.astype(np.float64).view(np.uint64).reshape(-1, 64)
    e = ((x >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64)
    live = m & (e != 0x7FF) & ((x << np.uint64(1)) != 0)
    limb = (np.maximum(e, 1) - 1) >> 5
    in_registers = by_lane = 0
    for s in np.flatnonzero(m.any(axis=1)):
        agree = np.unique(idx[s][m[s]]).size == 1
        span_ok = not live[s].any() or int(limb[s][live[s]].max()) - int(limb[s][live[s]].min()) <= 2
        if agree and span_ok:
            in_registers += 1
        else:
            by_lane += 1
    return in_registers, by_lane


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_both_arms_by_the_trace(ctx, dtype):
    dt = DTYPES[dtype]
    n, K = 8, 64
    keys = key_list(K, dt)
    rng = np.random.default_rng(41)
    sorted_key, xs = encoded(ctx, ("exact sorted key", dtype), lambda: np.sort(keys[rng.integers(0, K, n * 16)]).repeat(64))  # runs of whole steps
    random_key, xr = key_column(ctx, "random", n, K, dt)
    one_magnitude, x1 = encoded(ctx, ("exact one magnitude", dtype), lambda: (1.0 + np.random.default_rng(42).random(n * 1024)).astype(dt))
    apart, x2 = encoded(ctx, ("exact apart", dtype), lambda: np.where(np.arange(n * 1024) % 2 == 0, 1.0, 2.0 ** (200 if dtype == "f64" else 100)).astype(dt) * x1)
    steps = n * 16
    for what, val, xv, key, xk, want in (("a sorted key column, one magnitude", one_magnitude, x1, sorted_key, xs, (steps, 0)),
                                         ("the same keys, values 2^200 (float: 2^100) apart inside a step", apart, x2, sorted_key, xs, (0, steps)),
                                         ("a random key column", one_magnitude, x1, random_key, xr, (0, steps))):
        for mname, mask in (("none", None), ("random", random_mask(n, 43))):
            trace = torch.zeros(6, dtype=torch.int64, device=DEV)
            check(ctx, val, xv, key, xk, keys, mask, f"{dtype}, {what}, bitmap {mname}", trace=trace)
            arms = expected_arms(xv, xk, bits_of(mask, xv.size), keys)
            assert tuple(trace.tolist()[4:]) == arms, f"{what}, bitmap {mname}: the trace counts {trace.tolist()[4:]} steps, the condition {arms}"
            if mask is None:
                assert arms == want, f"{what}: {arms}"
    # with the key column's zone map the search is narrowed and nothing else changes: the runs are steps long, not vectors, so every vector is still
    # decoded or, where 16 runs happen to share a key, settled by the shortcut; either way every step goes through registers (the shortcut and the
    # record that admits no key have their own test below)
    zones = ctx.zone_map(sorted_key)
    trace = torch.zeros(6, dtype=torch.int64, device=DEV)
    check(ctx, one_magnitude, x1, sorted_key, xs, keys, None, f"{dtype}, the sorted key column with its zone map", zones=zones, trace=trace)
    t = trace.tolist()
    assert t[0] == 0 and t[1] + t[3] == n and t[4] == steps and t[5] == 0


# ---- 4b. the zone records: the constant-key shortcut and the record that admits no key ------------------------------------------------------------------------
def expected_classes(keys, zones, vec, sel_any):
    """the trace's first four words from the documented zone rules: vectors without a selected row, settled by the constant-key shortcut, with a record
    that admits no key, decoded"""
    zz = zones.cpu().numpy()
    ok = ~np.isnan(zz).any(axis=1)
    j0 = np.searchsorted(keys, np.where(ok, zz[:, 0], 0), side="left")
    j1 = np.searchsorted(keys, np.where(ok, zz[:, 1], 0), side="right")
    no_key = sel_any & ok & (j1 <= j0)
    const = sel_any & ok & (j1 > j0) & (zz[:, 0] == zz[:, 1]) & (vec["scheme"] == capi.SCHEME_ALP) & (vec["exc_cnt"] == 0)
    n_sel = int(sel_any.sum())
    return [sel_any.size - n_sel, int(const.sum()), int(no_key.sum()), n_sel - int(const.sum()) - int(no_key.sum())]


@pytest.mark.parametrize("K", [1, 64, 1024, 4097, 8193])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_zone_records_every_pattern_and_bitmap_the_shortcut_and_the_record_without_a_key(ctx, dtype, K):
    """the hard values beside every key pattern WITH the key column's zone map, its widened form and one with NaN bounds, under every bitmap: the
    replica's sums and counts, and the trace's classes from the rules.  The constant pattern sends vectors through the shortcut (the value vector
    alone decoded, 16 steps in registers under a NULL bitmap) and, where its key is one of the three left out of the list, through the record
    that admits no key (the rows counted in the last word, neither column read)."""
    from test_keyed_gpu import widened
    n = 32
    dt = DTYPES[dtype]
    val, xv = encoded(ctx, ("exact hard", dtype, n), lambda: hard_values(dtype, n, 19))
    keys = key_list(K, dt)
    for pattern in PATTERNS:
        key, xk = key_column(ctx, pattern, n, K, dt)
        _, vec, _, _ = key.to_host()
        zones = ctx.zone_map(key)
        holes = zones.clone()
        holes[::3, 0] = NAN  # a NaN bound prunes nothing
        for mname, mask in bitmaps(n, 57 + K).items():
            bits = bits_of(mask, xv.size)
            sel_any = bits.reshape(n, 1024).any(axis=1)
            tag = ("zones", dtype, K, pattern, mname)
            plain = check(ctx, val, xv, key, xk, keys, mask, f"{dtype}, {K} keys, {pattern}, bitmap {mname}: without zones", tag=tag)
            for zname, z in (("the zone map", zones), ("widened", widened(zones)), ("NaN bounds", holes)):
                what = f"{dtype}, {K} keys, {pattern}, bitmap {mname}, {zname}"
                trace = torch.zeros(6, dtype=torch.int64, device=DEV)
                s, c = check(ctx, val, xv, key, xk, keys, mask, what, tag=tag, zones=z, trace=trace)
                assert s.tobytes() == plain[0].tobytes() and c.tobytes() == plain[1].tobytes(), f"{what}: the records changed a byte"
                t = trace.tolist()
                assert t[:4] == expected_classes(keys, z, vec, sel_any), f"{what}: trace {t}"
                if pattern == "constant per vector" and zname == "the zone map":
                    per_vector = xk.reshape(n, 1024)
                    in_list = np.isin(per_vector[:, 0], keys)  # (from the values, not from the records)
                    plain_alp = (vec["scheme"] == capi.SCHEME_ALP) & (vec["exc_cnt"] == 0)  # what the shortcut asks of the descriptor: no NaN can hide
                    assert (per_vector == per_vector[:, :1]).all()
                    assert t[1] == int((in_list & plain_alp & sel_any).sum()) and t[2] == int((~in_list & sel_any).sum()), f"{what}: trace {t}"
                    assert int(c[K]) == int(bits.reshape(n, 1024)[~in_list].sum()), "the rows of a vector without a key are counted in the last word"
                    assert (t[4], t[5]) == expected_arms(xv, xk, bits, keys), "the shortcut's steps meet the same condition as a decoded vector's"
                    if mname == "none":
                        assert t[1] > 0 and (t[2] > 0 or K > 1), "the column reaches the shortcut and, with 3 of the pool's 4 values left out, the record without a key"
                        assert t[4] + t[5] == 16 * (t[1] + t[3]), "a constant-key vector is 16 agreeing steps, a vector without a key none"
                    if mname == "all zero":
                        assert t == [n, 0, 0, 0, 0, 0]
                if pattern == "constant per vector" and zname == "widened":
                    assert t[1] == 0, "a widened record is no point: no shortcut"
    s2, c2 = run(ctx, val, key, keys, mask=mask, zones=zones, counts=False)  # (the last pattern and bitmap) without counts: the same sums
    assert c2 is None and s2.tobytes() == plain[0].tobytes()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_column_settled_by_the_shortcut_alone_and_one_whose_records_admit_no_key(ctx, dtype):
    """every vector constant with a key of the list: the shortcut alone, 16 steps in registers each under a NULL bitmap, also where the values of a
    step lie too far apart for the frame (then 16 steps lane by lane).  Every vector constant below the list: rows without a key, neither column read."""
    dt = DTYPES[dtype]
    n, K = 32, GLOBAL_K[dtype]
    keys = key_list(K, dt)
    val, xv = encoded(ctx, ("exact hard", dtype, n), lambda: hard_values(dtype, n, 19))
    near, xn = encoded(ctx, ("exact one magnitude", dtype, n), lambda: (1.0 + np.random.default_rng(44).random(n * 1024)).astype(dt))
    key, xk = encoded(ctx, ("exact all shortcut", dtype), lambda: np.repeat(keys[np.random.default_rng(45).integers(0, K, n)], 1024))
    zones = ctx.zone_map(key)
    _, vec, _, _ = key.to_host()
    plain_alp = (vec["scheme"] == capi.SCHEME_ALP) & (vec["exc_cnt"] == 0)
    for mname, mask in bitmaps(n, 91).items():
        bits = bits_of(mask, xv.size)
        sel_any = bits.reshape(n, 1024).any(axis=1)
        n_sel, n_short = int(sel_any.sum()), int((sel_any & plain_alp).sum())  # (a constant vector the encoder stored as exceptions is decoded)
        for vname, v, x in (("hard values", val, xv), ("one magnitude", near, xn)):
            trace = torch.zeros(6, dtype=torch.int64, device=DEV)
            check(ctx, v, x, key, xk, keys, mask, f"{dtype}, all shortcut, {vname}, bitmap {mname}", zones=zones, trace=trace)
            t = trace.tolist()
            assert t[:4] == [n - n_sel, n_short, 0, n_sel - n_short], f"{vname}, bitmap {mname}: trace {t}"
            assert (t[4], t[5]) == expected_arms(x, xk, bits, keys), "the shortcut's steps meet the same condition as a decoded vector's"
            if mask is None:
                assert t[1] > n // 2 and t[4] + t[5] == 16 * n
                if vname == "one magnitude":
                    assert t[4] == 16 * n and t[5] == 0, "a constant-key vector is 16 steps in registers"
                else:
                    assert t[5] > 0, "steps whose values lie further apart than the frame go lane by lane in the shortcut too"
    low, xl = encoded(ctx, ("exact below the list", dtype), lambda: np.full(n * 1024, key_pool(K, dt)[0], dt))
    assert xl[0] < keys[0]
    mask = vectors_cleared(random_mask(n, 92), 3)
    sel = bits_of(mask, xv.size)
    n_sel = int(sel.reshape(n, 1024).any(axis=1).sum())
    trace = torch.zeros(6, dtype=torch.int64, device=DEV)
    s, c = check(ctx, val, xv, low, xl, keys, mask, f"{dtype}, records that admit no key", zones=ctx.zone_map(low), trace=trace)
    assert trace.tolist() == [n - n_sel, 0, n_sel, 0, 0, 0] and int(c[K]) == int(sel.sum()) > 0 and not c[:K].any() and not s.view(np.uint64).any()
    s2, c2 = run(ctx, val, low, keys, mask=mask, zones=ctx.zone_map(low), counts=False)
    assert c2 is None and s2.tobytes() == s.tobytes()


# ---- 5. what "exact" buys -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,kind", [("f64", "mixed"), ("f64", "rd"), ("f32", "mixed"), ("f32", "rd")])
def test_grids_of_1_7_and_the_default_give_the_same_bytes(ctx, dtype, kind):
    n, K = 250, GLOBAL_K[dtype]
    val, xv = value_column(ctx, dtype, kind, n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    keys = key_list(K, xv.dtype)
    mask = random_mask(n, 71)
    want_s, want_c = host_keyed_sum_exact(xv, xk, unpack_np(mask, xv.size), keys)
    runs = []
    for tuning in ({"grid": 1}, {"grid": 7}, None):
        s, c = run(ctx, val, key, keys, mask=mask, tuning=tuning)
        assert s.tobytes() == want_s.tobytes() and np.array_equal(c, want_c), f"tuning {tuning}"
        runs.append(s.tobytes() + c.tobytes())
    assert len(set(runs)) == 1
    s, c = run(ctx, val, key, keys, mask=mask, counts=False)  # without counts: the same sums
    assert c is None and s.tobytes() == want_s.tobytes()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_permuted_rows_give_the_same_sums_byte_for_byte(ctx, dtype):
    n, K = 32, 1024
    val, xv = encoded(ctx, ("exact hard", dtype, n), lambda: hard_values(dtype, n, 19))
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    keys = key_list(K, xv.dtype)
    perm = np.random.default_rng(73).permutation(xv.size)
    pval, pxv = encoded(ctx, ("exact hard permuted", dtype, n), lambda: xv[perm])
    pkey, pxk = encoded(ctx, ("exact key permuted", dtype, n), lambda: xk[perm])
    s, c = check(ctx, val, xv, key, xk, keys, None, f"{dtype}, the rows in order")
    ps, pc = run(ctx, pval, pkey, keys)
    assert ps.tobytes() == s.tobytes() and pc.tobytes() == c.tobytes(), "the order of the rows entered a sum"
    assert np.isfinite(s).sum() > K // 2


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_accumulate_over_two_halves_of_a_bitmap_and_over_two_shards_equals_one_call(ctx, dtype):
    n, K = 32, GLOBAL_K[dtype]
    val, xv = encoded(ctx, ("exact hard", dtype, n), lambda: hard_values(dtype, n, 19))
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    keys = key_list(K, xv.dtype)
    kd = torch.from_numpy(keys).to(DEV)
    mask = random_mask(n, 75)
    whole_s, whole_c = check(ctx, val, xv, key, xk, keys, mask, f"{dtype}, one call")
    # two halves of the bitmap
    half = random_mask(n, 76)
    table = new_table(ctx, K)
    s1, c1 = run(ctx, val, key, keys, mask=mask & half, table=table)
    outs = (torch.from_numpy(s1).to(DEV), torch.from_numpy(c1).to(DEV))
    s2, c2 = run(ctx, val, key, keys, mask=mask & ~half, table=table, accumulate=True, outs=outs)
    assert s2.tobytes() == whole_s.tobytes() and np.array_equal(c2, whole_c), "two halves of the bitmap, the second call accumulating"
    assert s1.tobytes() != whole_s.tobytes()
    # two shards of the columns, encoded separately
    cut = 13 * 1024
    shards = [(encoded(ctx, ("exact shard val", dtype, i), lambda: xv[a:b].copy())[0], encoded(ctx, ("exact shard key", dtype, i), lambda: xk[a:b].copy())[0],
               mask[a // 64: b // 64].contiguous()) for i, (a, b) in enumerate(((0, cut), (cut, xv.size)))]
    table = new_table(ctx, K)
    sums = torch.full((K,), NAN, dtype=torch.float64, device=DEV)
    cnt = torch.full((K + 1,), POISON, dtype=torch.int64, device=DEV)
    for i, (sv, sk, sm) in enumerate(shards):
        ctx.keyed_sum_exact_into(sv, sk, kd, sums, counts_out=cnt, mask=sm, table=table, accumulate=i > 0)
    assert sums.cpu().numpy().tobytes() == whole_s.tobytes() and np.array_equal(cnt.cpu().numpy(), whole_c), "two shards, the second call accumulating"


@pytest.mark.parametrize("K", [1, 65, 1024])
def test_multiples_of_a_quarter_equal_keyed_sum_into_byte_for_byte(ctx, K):
    """a column whose every partial sum is exact in any order: the striped keyed SUM and the exact one give the same bytes and the same counts"""
    n = 250
    val, xv = encoded(ctx, ("exact quarters", n), lambda: np.random.default_rng(79).integers(-(2**20), 2**20 + 1, n * 1024).astype(np.float64) * 0.25)
    key, xk = key_column(ctx, "random", n, K, np.float64)
    keys = key_list(K, np.float64)
    kd = torch.from_numpy(keys).to(DEV)
    for mask in (None, random_mask(n, 80)):
        s, c = run(ctx, val, key, keys, mask=mask)
        old_s = torch.full((K,), NAN, dtype=torch.float64, device=DEV)
        old_c = torch.full((K + 1,), POISON, dtype=torch.int64, device=DEV)
        ctx.keyed_sum_into(val, key, kd, old_s, counts_out=old_c, mask=mask)
        assert s.tobytes() == old_s.cpu().numpy().tobytes() and np.array_equal(c, old_c.cpu().numpy())
        assert np.abs(s).max() > 0


# ---- 6. capture ---------------------------------------------------------------------------------------------------------------------------------------------------
CAPTURE = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
import datagen
from alp_amd import capi
from keyed_exact_replica import host_keyed_sum_exact
ctx = capi.Context(0)
side = torch.cuda.Stream()
ok = True
nv = 60
def bits_of(words):
    return ((words[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)
for dt, make, K in ((np.float64, datagen.mixed_column, 4097), (np.float32, datagen.mixed_column_f32, 8193)):
    rng = np.random.default_rng(5)
    xv = make(nv, seed=81)
    pool = ((np.arange(K + 3) - 5) * 0.25).astype(dt)
    xk = pool[rng.integers(0, K + 3, nv * 1024)]
    keys = np.sort(np.delete(pool, [0, 30, K + 2]))
    other = np.sort(np.delete(pool, [1, 2, 3]))               # the keys' contents after the first replay: the same length, other values
    val, key = ctx.encode(torch.from_numpy(xv).cuda()), ctx.encode(torch.from_numpy(xk).cuda())
    kd = torch.from_numpy(keys).cuda()
    words = np.random.default_rng(6).integers(0, 2**64, 16 * nv, dtype=np.uint64)
    mask = torch.from_numpy(words.view(np.int64)).cuda()
    sums = torch.zeros(K, dtype=torch.float64, device="cuda:0")
    cnt = torch.zeros(K + 1, dtype=torch.int64, device="cuda:0")
    table = ctx.keyed_sum_exact_table(K)
    def calls():
        ctx.keyed_sum_exact_into(val, key, kd, sums, counts_out=cnt, mask=mask, table=table)
    with torch.cuda.stream(side):
        calls()                                                 # warm-up on the capture stream
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            calls()
    for rep in range(2):
        if rep == 1:
            keys = other
            kd.copy_(torch.from_numpy(keys).cuda())
        torch.cuda.synchronize()
        sums.fill_(float(rep) - 1.0); cnt.fill_(rep - 1); table.fill_(rep + 1)
        g.replay()
        torch.cuda.synchronize()
        ws, wc = host_keyed_sum_exact(xv, xk, bits_of(words), keys)
        ok = ok and sums.cpu().numpy().tobytes() == ws.tobytes() and np.array_equal(cnt.cpu().numpy(), wc) and int(wc.sum()) > 0
        print(dt.__name__, rep, int(wc.sum()), int(wc[-1]), ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_twice_with_the_keys_changed_between():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 7. the allocating wrapper and the C++ surface ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_allocating_wrapper_sorts_its_keys(ctx, dtype):
    n, K = 32, GLOBAL_K[dtype]
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    keys = key_list(K, xv.dtype)
    mask = random_mask(n, 5)
    want_s, want_c = host_keyed_sum_exact(xv, xk, unpack_np(mask, xv.size), keys)
    shuffled = np.random.default_rng(1).permutation(keys)
    for form in (shuffled, torch.from_numpy(shuffled), torch.from_numpy(shuffled).to(DEV), [float(t) for t in shuffled]):
        s, c, u = ctx.keyed_sum_exact(val, key, form, mask=mask, zones=ctx.zone_map(key))
        assert s.dtype == torch.float64 and c.dtype == torch.int64 and tuple(s.shape) == (K,) and c.numel() == K
        assert s.cpu().numpy().tobytes() == want_s.tobytes() and np.array_equal(c.cpu().numpy(), want_c[:K]) and int(u) == int(want_c[K])
    s, c, u = ctx.keyed_sum_exact(val, key, torch.from_numpy(keys).to(DEV), mask=mask, counts=False, sorted=True)
    assert c is None and u is None and s.cpu().numpy().tobytes() == want_s.tobytes()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cpp_column_sum_by_key_exact_against_the_replica(ctx, tmp_path, dtype):
    """include/alp/batch.hpp: alp::gpu::column<PT>::sum_by_key_exact of two serialized columns; the counts against column::decompress and a host
    loop, the sums against the replica's bytes (tests/cpp/keyed_sum_exact_test.cpp)"""
    exe = tmp_path / "keyed_sum_exact_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/keyed_sum_exact_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    n, K = 60, GLOBAL_K[dtype]
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    ctx.to_blob(val, xv.size).tofile(str(tmp_path / "val.blob"))
    ctx.to_blob(key, xk.size).tofile(str(tmp_path / "key.blob"))
    keys = key_list(K, xk.dtype)
    np.random.default_rng(2).permutation(keys).tofile(str(tmp_path / "keys.bin"))  # (the wrapper sorts)
    mask = vectors_cleared(random_mask(n, 53), 3)
    mask[16:32] = -1
    mask.cpu().numpy().tofile(str(tmp_path / "in.mask"))
    want_s, want_c = host_keyed_sum_exact(xv, xk, unpack_np(mask, xv.size), keys)
    with open(tmp_path / "want.bin", "wb") as f:
        f.write(want_s.tobytes() + want_c.astype(np.uint64).tobytes())
    p = subprocess.run([str(exe), dtype] + [str(tmp_path / f) for f in ("val.blob", "key.blob", "keys.bin", "in.mask", "want.bin")], capture_output=True, text=True, timeout=600)
    line = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("ok ")]
    assert p.returncode == 0 and len(line) == 1, p.stdout[-3000:] + p.stderr[-2000:]
    k = int(unpack_np(mask, xv.size).sum())
    assert int(line[0][1]) == n and int(line[0][2]) == k and 0 < k < xv.size and int(line[0][3]) == K
