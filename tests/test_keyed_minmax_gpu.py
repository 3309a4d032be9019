"""GPU: keyed MIN / MAX (include/alpgpu.h, "keyed MIN / MAX": alpgpu_decode_keyed_minmax_*), double and float.  No expectation comes from the code under
test: the columns' values are the arrays that were encoded (the store decode is held to them bit for bit here and to the oracle by other suites), the
records and counts come from tests/keyed_minmax_replica.py (integer order keys on the host).  Records compare bit for bit, counts as integers.  The
columns, key patterns, key lists and bitmaps are tests/test_keyed_gpu.py's."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import datagen
from alp_amd import capi
from keyed_minmax_replica import host_keyed_minmax, same_records
from test_keyed_gpu import KEY_COUNTS, PATTERNS, POISON, encoded, key_column, key_list, key_pool, masks_of, random_mask, unpack_np, vectors_cleared, widened

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF, NAN = math.inf, math.nan
DTYPES = {"f64": np.float64, "f32": np.float32}
EMPTY = [INF, -INF]


def value_column(ctx, dtype, kind, n):
    make = {("f64", "mixed"): lambda: datagen.mixed_column(n, seed=5 + n), ("f64", "rd"): lambda: datagen.rd_column(n, seed=6 + n),
            ("f32", "mixed"): lambda: datagen.mixed_column_f32(n, seed=5 + n), ("f32", "rd"): lambda: datagen.rd_column_f32(n, seed=6 + n)}[(dtype, kind)]
    col, xs = encoded(ctx, ("kmm val", dtype, kind, n), make)
    assert xs.dtype == DTYPES[dtype]
    return col, xs


def bitmaps(n, seed):
    m = masks_of(n, seed)
    return {"none": None, "random": m["random"], "vectors zero": m["vectors zero"], "all zero": torch.zeros(16 * n, dtype=torch.int64, device=DEV)}


def run(ctx, val, key, keys, mask=None, zones=None, tuning=None, trace=None, counts=True):
    """keyed_minmax_into on poisoned outputs: (records [K, 2] as numpy, counts int64[K + 1] as numpy or None)"""
    kd = torch.from_numpy(np.ascontiguousarray(keys)).to(DEV)
    out = torch.full((kd.numel(), 2), NAN, dtype=kd.dtype, device=DEV)
    cnt = torch.full((kd.numel() + 1,), POISON, dtype=torch.int64, device=DEV) if counts else None
    ctx.keyed_minmax_into(val, key, kd, out, counts_out=cnt, mask=mask, zones=zones, tuning=tuning, trace=trace)
    return out.cpu().numpy(), (cnt.cpu().numpy() if counts else None)


def bits_of(mask, total):
    return np.ones(total, bool) if mask is None else unpack_np(mask, total)


def check(ctx, val, xv, key, xk, keys, mask, what, **kw):
    bits = bits_of(mask, xv.size)
    want_r, want_c = host_keyed_minmax(xv, xk, bits, keys)
    got_r, got_c = run(ctx, val, key, keys, mask=mask, **kw)
    assert np.array_equal(got_c, want_c), f"{what}: counts differ from the replica"
    assert same_records(got_r, want_r), f"{what}: records differ from the replica in {int((got_r.view(np.uint8) != want_r.view(np.uint8)).reshape(len(keys), -1).any(axis=1).sum())} keys"
    assert int(got_c.sum()) == int(bits.sum())
    return got_r, got_c


# ---- 1. small columns: fewer vectors than wavefronts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "rd"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_small_columns_every_key_count_pattern_and_bitmap(ctx, dtype, kind, n):
    """n < 8: idle wavefronts still pass the barrier and the flush; 1024 keys: more keys than the workgroup has threads, the staging loop strides"""
    val, xv = value_column(ctx, dtype, kind, n)
    for K in KEY_COUNTS:
        keys = key_list(K, xv.dtype)
        for pattern in PATTERNS:
            key, xk = key_column(ctx, pattern, n, K, xv.dtype)
            for mname, mask in bitmaps(n, 21 + K).items():
                trace = torch.zeros(4, dtype=torch.int64, device=DEV)
                r, c = check(ctx, val, xv, key, xk, keys, mask, f"{dtype} {kind}, {n} vectors, {K} keys, {pattern}, bitmap {mname}", trace=trace)
                if mname == "all zero":
                    assert r.tolist() == [EMPTY] * K and not c.any() and trace.tolist() == [n, 0, 0, 0], "nothing selected: every vector is skipped"
    assert K == capi.KEYED_KEYS_MAX


# ---- 2. the grid does not enter the result ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,kind,K", [("f64", "mixed", 65), ("f64", "rd", 1024), ("f32", "mixed", 1024), ("f32", "rd", 64)])
def test_grids_of_1_7_and_the_default_give_the_same_bytes(ctx, dtype, kind, K):
    n = 250
    val, xv = value_column(ctx, dtype, kind, n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    keys = key_list(K, xv.dtype)
    mask = random_mask(n, 71)
    want_r, want_c = host_keyed_minmax(xv, xk, unpack_np(mask, xv.size), keys)
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


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_second_trip_at_the_default_grid(ctx, dtype):
    """8193 vectors are more than 2 x 256 workgroups of 8 wavefronts hold at once: wavefronts make a second trip at the default grid"""
    n, K = 8193, 65
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    mask = vectors_cleared(random_mask(n, 31, ands=3), 3)
    check(ctx, val, xv, key, xk, key_list(K, xv.dtype), mask, f"{dtype}, {n} vectors")


# ---- 3. today's route and the counts of keyed SUM ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,kind", [("f64", "mixed"), ("f32", "rd")])
def test_equal_to_rounds_of_decode_group_minmax_and_group_minmax_totals(ctx, dtype, kind):
    n, K = 250, 65
    val, xv = value_column(ctx, dtype, kind, n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    keys = key_list(K, xv.dtype)
    mask = random_mask(n, 12)
    got_r, got_c = check(ctx, val, xv, key, xk, keys, mask, "against the replica first")
    recs, counts = [], []
    for r in range(0, K, 16):  # ceil(K / 16) rounds, each key a closed range [k, k]
        part = keys[r: r + 16].astype(np.float64).tolist()
        c = torch.zeros((len(part), n), dtype=torch.int32, device=DEV)
        z = ctx.decode_group_minmax(val, key, mask, part, part, counts=c)
        recs.append(ctx.group_minmax_totals(z))
        counts.append(c.sum(dim=1, dtype=torch.int64))
    assert same_records(got_r, torch.cat(recs).cpu().numpy())
    assert np.array_equal(got_c[:K], torch.cat(counts).cpu().numpy())
    if dtype == "f64":  # the counts are keyed SUM's
        kd = torch.from_numpy(keys).to(DEV)
        sums = torch.empty(K, dtype=torch.float64, device=DEV)
        cnt = torch.full((K + 1,), POISON, dtype=torch.int64, device=DEV)
        ctx.keyed_sum_into(val, key, kd, sums, counts_out=cnt, mask=mask)
        assert np.array_equal(got_c, cnt.cpu().numpy())


# ---- 4. both zeros ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("where", ["one step", "two steps", "two wavefronts", "two workgroups"])
def test_both_zeros_in_either_order_of_arrival(ctx, dtype, where):
    """key 1.0 meets +0.0 and then -0.0, key 2.0 the opposite order; every other row has a key that is not in the list.  The record is {-0.0, +0.0} by
    its bits: a guard that compared with C's < would drop the zero that arrives second."""
    dt = DTYPES[dtype]
    n = 10
    second = {"one step": 9, "two steps": 5 * 64 + 9, "two wavefronts": 1024 + 9, "two workgroups": 9 * 1024 + 9}[where]

    def make_val():
        x = np.full(n * 1024, 7.25, dt)
        x[3], x[second] = 0.0, -0.0  # key 1.0
        x[4], x[second + 1] = -0.0, 0.0  # key 2.0
        return x

    def make_key():
        k = np.full(n * 1024, 5.0, dt)
        k[[3, second]] = 1.0
        k[[4, second + 1]] = 2.0
        return k
    val, xv = encoded(ctx, ("zeros val", dtype, where), make_val)
    key, xk = encoded(ctx, ("zeros key", dtype, where), make_key)
    keys = np.array([1.0, 2.0, 3.0], dt)
    for zones in (None, ctx.zone_map(key)):
        r, c = check(ctx, val, xv, key, xk, keys, None, f"{dtype}, {where}", zones=zones)
        for i in (0, 1):
            assert r[i].tolist() == [0.0, 0.0] and np.signbit(r[i, 0]) and not np.signbit(r[i, 1]), f"key {keys[i]}: min is -0.0 and max is +0.0"
        assert r[2].tolist() == EMPTY and c.tolist() == [2, 2, 0, n * 1024 - 4]


# ---- 5. NaNs, lists, a column as its own key ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_nan_keys_and_nan_values_in_the_columns(ctx, dtype):
    dt = DTYPES[dtype]

    def make_key():
        k = key_pool(16, dt)[np.random.default_rng(61).integers(0, 19, 3 * 1024)].copy()
        k[::7] = NAN  # exceptions of ALP vectors
        return k

    def make_rd_key():
        k = np.random.default_rng(62).random(3 * 1024).astype(dt)
        k[::3] = NAN  # an ALP_RD vector holds them in its packed words
        return k

    def make_val():
        x = np.round(np.random.default_rng(63).normal(0, 100, 3 * 1024), 2).astype(dt)
        x[5::64] = NAN
        x[6::64] = INF
        x[7::64] = -INF
        return x
    key, xk = encoded(ctx, ("kmm nan key", dtype), make_key)
    keys = key_list(16, dt)
    lonely = keys[4]  # a key whose rows all hold NaN values

    def make_val_lonely():
        x = make_val()
        x[make_key() == lonely] = NAN
        return x
    val, xv = encoded(ctx, ("kmm nan val", dtype), make_val_lonely)
    r, c = check(ctx, val, xv, key, xk, keys, None, "NaN keys, NaN values")
    assert r[4].tolist() == EMPTY and c[4] > 0, "a key whose rows are all NaN: the empty record, counted"
    assert int(c[-1]) >= int(np.isnan(xk).sum()) and (r[:, 1] == INF).any() and (r[:, 0] == -INF).any()
    check(ctx, val, xv, key, xk, keys, vectors_cleared(random_mask(3, 64), 2), "NaN keys, NaN values, a bitmap")
    rdk, xrk = encoded(ctx, ("kmm rd nan key", dtype), make_rd_key)
    _, vec, _, _ = rdk.to_host()
    assert (vec["scheme"] == capi.SCHEME_ALP_RD).all()
    real = np.unique(xrk[~np.isnan(xrk)])
    r, c = check(ctx, val, xv, rdk, xrk, np.sort(real[:1024]), None, "an ALP_RD key column with NaNs")
    assert int(c[-1]) >= 1024


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_duplicates_both_zeros_and_nans_in_the_key_list(ctx, dtype):
    dt = DTYPES[dtype]
    val, xv = value_column(ctx, dtype, "mixed", 3)
    key, xk = key_column(ctx, "random", 3, 63, dt)
    assert (xk == 0).any()
    base = key_list(63, dt)
    keys = np.sort(np.concatenate([base, base[10:14], np.array([-0.0], dt)]))  # duplicates, and -0.0 beside +0.0 (numpy.sort keeps either order)
    keys = np.concatenate([keys, np.array([NAN, NAN], dt)])  # NaNs last: never matched
    r, c = check(ctx, val, xv, key, xk, keys, random_mask(3, 51), "duplicates, zeros, NaNs in the list")
    first_zero = int(np.flatnonzero(keys == 0)[0])
    assert c[first_zero] > 0 and c[first_zero + 1] == 0 and r[first_zero + 1].tolist() == EMPTY
    assert c[-3] == 0 and c[-2] == 0 and r[-1].tolist() == EMPTY and r[-2].tolist() == EMPTY
    dup = np.flatnonzero(keys[1:] == keys[:-1]) + 1
    assert dup.size >= 5 and not c[dup].any() and r[dup].tolist() == [EMPTY] * dup.size, "later duplicates receive nothing"


@pytest.mark.parametrize("dtype,kind", [("f64", "mixed"), ("f64", "rd"), ("f32", "mixed"), ("f32", "rd")])
def test_a_column_as_its_own_key(ctx, dtype, kind):
    val, xv = value_column(ctx, dtype, kind, 3)
    real = np.unique(xv[~np.isnan(xv)])
    keys = np.sort(np.random.default_rng(3).choice(real, min(1024, real.size), replace=False))
    for mname, mask in masks_of(3, 41).items():
        r, c = check(ctx, val, xv, val, xv, keys, mask, f"{dtype} {kind} as its own key, bitmap {mname}")
    hit = c[:-1] > 0
    assert int(c[-1]) > 0 and hit.any() and (r[hit, 0] == keys[hit]).all() and (r[hit, 1] == keys[hit]).all(), "a key's record is the key itself"


# ---- 6. zone records --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,kind", [("f64", "mixed"), ("f32", "rd")])
def test_truthful_and_widened_records_change_no_byte_and_constant_keys_are_settled(ctx, dtype, kind):
    n, K = 250, 65
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
                    assert t[1] > 0 and t[2] > 0, "the constant-key and the no-key class must show in the trace"
                if pattern == "constant per vector" and zname == "widened":
                    assert t[1] == 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_lying_records_and_unsorted_keys_keep_the_total_and_stay_inside_the_outputs(ctx, dtype):
    n = 250
    val, xv = value_column(ctx, dtype, "mixed", n)
    mask = random_mask(n, 91)
    n_sel = int(unpack_np(mask, xv.size).sum())
    guard = 64
    for K, pattern in ((65, "constant per vector"), (65, "random"), (1024, "random"), (1, "two keys by lane")):
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
            ctx.keyed_minmax_into(val, key, kd, rbuf[guard: guard + K], counts_out=cbuf[guard: guard + K + 1], mask=mask, zones=z)
            ctx.synchronize()
            assert bool((rbuf[:guard] == -12345.5).all()) and bool((rbuf[guard + K:] == -12345.5).all()), f"{what}, {K} keys: words beside the records changed"
            assert bool((cbuf[:guard] == POISON).all()) and bool((cbuf[guard + K + 1:] == POISON).all()), f"{what}, {K} keys: words beside the counts changed"
            counts = cbuf[guard: guard + K + 1]
            assert bool((counts >= 0).all()) and int(counts.sum()) == n_sel, f"{what}, {K} keys: the total is the selected count"
            assert not bool(torch.isnan(rbuf).any())


# ---- 7. capture -------------------------------------------------------------------------------------------------------------------------------------------------
CAPTURE = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
import datagen
from alp_amd import capi
from keyed_minmax_replica import host_keyed_minmax, same_records
ctx = capi.Context(0)
side = torch.cuda.Stream()
ok = True
nv, K = 230, 65
def bitmap(seed):
    return np.random.default_rng(seed).integers(0, 2**64, 16 * nv, dtype=np.uint64)
def bits_of(words):
    return ((words[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)
for dt, make in ((np.float64, datagen.mixed_column), (np.float32, datagen.mixed_column_f32)):
    rng = np.random.default_rng(5)
    xv = make(nv, seed=81)
    pool = ((np.arange(K + 3) - 5) * 0.25).astype(dt)
    xk = pool[rng.integers(0, K + 3, nv * 1024)]
    keys = np.sort(np.delete(pool, [0, 30, K + 2]))
    val, key = ctx.encode(torch.from_numpy(xv).cuda()), ctx.encode(torch.from_numpy(xk).cuda())
    kd = torch.from_numpy(keys).cuda()
    words = bitmap(6)
    mask = torch.from_numpy(words.view(np.int64)).cuda()
    out = torch.zeros((K, 2), dtype=kd.dtype, device="cuda:0")
    cnt = torch.zeros(K + 1, dtype=torch.int64, device="cuda:0")
    def calls():
        ctx.keyed_minmax_into(val, key, kd, out, counts_out=cnt, mask=mask)
    with torch.cuda.stream(side):
        calls()                                                 # warm-up on the capture stream
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            calls()
    for rep in range(3):
        if rep == 2:
            words = bitmap(7)                                   # the second replay after the bitmap changed
            mask.copy_(torch.from_numpy(words.view(np.int64)).cuda())
        torch.cuda.synchronize()
        out.fill_(float(rep) - 1.0); cnt.fill_(rep - 1)
        g.replay()
        torch.cuda.synchronize()
        wr, wc = host_keyed_minmax(xv, xk, bits_of(words), keys)
        ok = ok and same_records(out.cpu().numpy(), wr) and np.array_equal(cnt.cpu().numpy(), wc) and int(wc.sum()) > 0
        print(dt.__name__, rep, int(wc.sum()), ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_bitmap_changed():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 8. argument checks, an empty column, the allocating wrapper ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c_argument_checks(ctx, dtype):
    n, K = 3, 65
    vb = 8 if dtype == "f64" else 4
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    other, _ = value_column(ctx, dtype, "mixed", 1)
    keys = torch.from_numpy(key_list(K, xv.dtype)).to(DEV)
    zones = ctx.zone_map(key)
    mask = random_mask(n, 10)
    out = torch.full((K + 8, 2), 7.5, dtype=keys.dtype, device=DEV)
    cnt = torch.full((K + 9,), POISON, dtype=torch.int64, device=DEV)
    trace = torch.full((5,), POISON, dtype=torch.int64, device=DEV)
    fn, dbg = getattr(capi.lib, "alpgpu_decode_keyed_minmax_" + dtype), getattr(capi.lib, "alpgpu_debug_decode_keyed_minmax_" + dtype)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    v, k, o = ctypes.byref(val.c), ctypes.byref(key.c), ctypes.byref(other.c)
    assert fn(None, v, k, p(mask), None, p(keys), K, p(out), p(cnt)) == -2, "a NULL context must be refused"
    assert fn(ctx.h, None, k, p(mask), None, p(keys), K, p(out), p(cnt)) == -2, "a NULL value column must be refused"
    assert fn(ctx.h, v, None, p(mask), None, p(keys), K, p(out), p(cnt)) == -2, "a NULL key column must be refused"
    assert fn(ctx.h, v, k, p(mask), None, None, K, p(out), p(cnt)) == -2, "NULL keys must be refused"
    assert fn(ctx.h, v, k, p(mask), None, p(keys), K, None, p(cnt)) == -2, "NULL records must be refused"
    for bad in (0, 1025, 2**32 - 1):
        assert fn(ctx.h, v, k, p(mask), None, p(keys), bad, p(out), p(cnt)) == -2, "n_keys outside 1 .. 1024 must be refused"
    assert fn(ctx.h, v, o, p(mask), None, p(keys), K, p(out), p(cnt)) == -2, "columns of unequal length must be refused"
    assert fn(ctx.h, v, k, p(mask), None, p(keys), K, p(out, vb), p(cnt)) == -2, "records that are not aligned to their size must be refused"
    assert fn(ctx.h, v, k, p(mask), None, p(keys), K, p(out), p(cnt, 4)) == -2, "misaligned counts must be refused"
    assert fn(ctx.h, v, k, p(mask, 4), None, p(keys), K, p(out), p(cnt)) == -2, "a misaligned bitmap must be refused"
    assert fn(ctx.h, v, k, p(mask), None, p(keys, vb // 2), K, p(out), p(cnt)) == -2, "misaligned keys must be refused"
    assert fn(ctx.h, v, k, p(mask), p(zones, vb), p(keys), K, p(out), p(cnt)) == -2, "misaligned zones must be refused"
    assert dbg(ctx.h, v, k, p(mask), None, p(keys), K, p(out), p(cnt), None, p(trace, 4)) == -2, "a misaligned trace must be refused"
    ctx.synchronize()
    assert bool((out == 7.5).all()) and bool((cnt == POISON).all()) and bool((trace == POISON).all()), "a refused call wrote"
    # the accepted call fills exactly its K records and K + 1 counts
    assert fn(ctx.h, v, k, p(mask), p(zones), p(keys), K, p(out), p(cnt)) == 0
    ctx.synchronize()
    want_r, want_c = host_keyed_minmax(xv, xk, unpack_np(mask, xv.size), keys.cpu().numpy())
    assert same_records(out[:K].cpu().numpy(), want_r) and np.array_equal(cnt[: K + 1].cpu().numpy(), want_c)
    assert bool((out[K:] == 7.5).all()) and bool((cnt[K + 1:] == POISON).all())


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_column_of_no_vectors_gives_the_empty_record_and_zero_everywhere(ctx, dtype):
    empty = capi.CColumn()
    fn = getattr(capi.lib, "alpgpu_decode_keyed_minmax_" + dtype)
    tdt = torch.float64 if dtype == "f64" else torch.float32
    keys = torch.arange(5, dtype=tdt, device=DEV)
    out = torch.full((7, 2), -1.0, dtype=tdt, device=DEV)
    cnt = torch.full((8,), POISON, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert fn(ctx.h, ctypes.byref(empty), ctypes.byref(empty), None, None, p(keys), 5, p(out), p(cnt)) == 0
    ctx.synchronize()
    assert out[:5].tolist() == [EMPTY] * 5 and out[5:].tolist() == [[-1.0, -1.0]] * 2, "{+inf, -inf}, and nothing behind the records"
    assert cnt[:6].tolist() == [0] * 6 and cnt[6:].tolist() == [POISON] * 2
    out.fill_(-1.0)
    assert fn(ctx.h, ctypes.byref(empty), ctypes.byref(empty), None, None, p(keys), 5, p(out), None) == 0  # without counts
    ctx.synchronize()
    assert out[:5].tolist() == [EMPTY] * 5 and out[5:].tolist() == [[-1.0, -1.0]] * 2


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_allocating_wrapper_sorts_its_keys(ctx, dtype):
    n, K = 3, 63
    val, xv = value_column(ctx, dtype, "mixed", n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    keys = key_list(K, xv.dtype)
    mask = random_mask(n, 5)
    want_r, want_c = host_keyed_minmax(xv, xk, unpack_np(mask, xv.size), keys)
    shuffled = np.random.default_rng(1).permutation(keys)
    forms = [shuffled, torch.from_numpy(shuffled), torch.from_numpy(shuffled).to(DEV)] + ([shuffled.tolist()] if dtype == "f64" else [[float(t) for t in shuffled]])
    for form in forms:
        r, c, u = ctx.keyed_minmax(val, key, form, mask=mask, zones=ctx.zone_map(key))
        assert r.dtype == val_dtype(dtype) and c.dtype == torch.int64 and tuple(r.shape) == (K, 2) and c.numel() == K
        assert same_records(r.cpu().numpy(), want_r) and np.array_equal(c.cpu().numpy(), want_c[:K]) and int(u) == int(want_c[K])
    r, c, u = ctx.keyed_minmax(val, key, torch.from_numpy(keys).to(DEV), mask=mask, counts=False, sorted=True)
    assert c is None and u is None and same_records(r.cpu().numpy(), want_r)


def val_dtype(dtype):
    return torch.float64 if dtype == "f64" else torch.float32


# ---- 9. the C++ wrapper -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cpp_column_minmax_by_key_against_decompress_and_a_host_loop(ctx, tmp_path, dtype):
    """include/alp/batch.hpp: alp::gpu::column<PT>::minmax_by_key of two serialized columns against column::decompress and a host loop
    (tests/cpp/keyed_minmax_test.cpp)"""
    exe = tmp_path / "keyed_minmax_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/keyed_minmax_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    n, K = 250, 65
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
    assert int(line[0][1]) == n and int(line[0][2]) == k and 0 < k < xv.size
