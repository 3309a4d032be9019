"""GPU: bucketed aggregation (include/alpgpu.h, "bucketed aggregation": alpgpu_decode_bucket_sum_* / alpgpu_decode_bucket_minmax_*).  No expectation comes
from the code under test: the columns' values are the arrays that were encoded (the store decode is held to them bit for bit here and to the oracle by
other suites), sums, records and counts come from tests/bucket_replica.py (numpy.searchsorted in front of the keyed replicas' documented order), and,
where the contract names existing calls, from Context.histogram, keyed_sum and keyed_minmax.  Sums compare bit for bit (NaNs as NaNs), records byte for
byte, counts as integers."""
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
from bucket_replica import bucket_of, host_bucket_minmax, host_bucket_sum
from keyed_minmax_replica import same_records
from keyed_replica import same_sums, stripe_vectors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF, NAN = math.inf, math.nan
EDGE_COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 1023)  # 255: the last of the small tier (256 buckets), 256 the first of the large
PATTERNS = ("constant per vector", "two buckets by lane", "64 distinct per step", "random")
KINDS = ("mixed", "rd", "float")
POISON = 0x5A5A5A5A5A5A5A5A
_cache = {}


def ibits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def unpack_np(mask, total):
    w = mask.cpu().numpy().view(np.uint64)
    return ((w[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)[:total]


def random_mask(n_vectors, seed, ands=1):
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 2**64, 16 * n_vectors, dtype=np.uint64)
    for _ in range(ands - 1):  # density 2^-ands
        words &= rng.integers(0, 2**64, 16 * n_vectors, dtype=np.uint64)
    return torch.from_numpy(words.view(np.int64)).to(DEV)


def vectors_cleared(mask, keep_every):
    m = mask.clone().reshape(-1, 16)
    v = torch.arange(m.shape[0], device=mask.device)
    m[(v % keep_every) != 1] = 0
    return m.reshape(-1)


def masks_of(n_vectors, seed, ands=1):
    rnd = random_mask(n_vectors, seed, ands)
    return {"none": None, "full": torch.full((16 * n_vectors,), -1, dtype=torch.int64, device=DEV), "random": rnd, "vectors zero": vectors_cleared(rnd, 3)}


def bits_of(mask, total):
    return np.ones(total, bool) if mask is None else unpack_np(mask, total)


def encoded(ctx, tag, make):
    """(DeviceColumn, the values that were encoded), encoded once per session and left unchanged"""
    if tag not in _cache:
        xs = np.ascontiguousarray(make())
        xd = torch.from_numpy(xs).to(DEV)
        col = ctx.encode(xd)
        assert torch.equal(ibits(ctx.decode(col)), ibits(xd)), f"{tag}: decode(encode(x)) != x"
        _cache[tag] = (col, xs)
    return _cache[tag]


def value_column(ctx, kind, n):
    make = {"mixed": lambda: datagen.mixed_column(n, seed=5 + n), "rd": lambda: datagen.rd_column(n, seed=6 + n), "float": lambda: datagen.mixed_column_f32(n, seed=7 + n)}[kind]
    return encoded(ctx, ("val", kind, n), make)


def key_pool(E, dtype):
    """2 E + 6 distinct keys an eighth apart around zero (decimal: ALP vectors without exceptions), +0.0 among them"""
    return ((np.arange(2 * E + 6) - 5) * 0.125).astype(dtype)


def edge_list(E, dtype):
    """E sorted edges, every second value of the pool from its fourth on: keys lie on edges, between them, below the first and above the last"""
    return key_pool(E, dtype)[3::2][:E].copy()


def key_column(ctx, pattern, n, E, dtype, seed=0):
    def make():
        rng = np.random.default_rng(1000 * n + E + seed)
        pool = key_pool(E, dtype)
        P = pool.size
        lane = np.arange(1024) % 64
        if pattern == "constant per vector":
            k = np.repeat(pool[rng.integers(0, P, n)], 1024)
        elif pattern == "two buckets by lane":
            pair = rng.integers(0, P, (n, 2))
            k = pool[np.where((lane % 2 == 0)[None, :], pair[:, :1], pair[:, 1:])].reshape(-1)
        elif pattern == "64 distinct per step":
            off = rng.integers(0, P, (n, 16))
            k = pool[(np.repeat(off, 64, axis=1) + 2 * lane[None, :]) % P].reshape(-1)
        else:
            k = pool[rng.integers(0, P, n * 1024)]
        return k.astype(dtype)
    return encoded(ctx, ("key", pattern, n, E, np.dtype(dtype).name, seed), make)


def run_sum(ctx, val, key, edges, right=False, mask=None, zones=None, tuning=None, trace=None, counts=True, scratch=None):
    """bucket_sum_into on poisoned outputs: (sums float64[B], counts int64[B + 1] or None) as numpy"""
    ed = torch.from_numpy(np.ascontiguousarray(edges)).to(DEV)
    sums = torch.full((ed.numel() + 1,), NAN, dtype=torch.float64, device=DEV)
    cnt = torch.full((ed.numel() + 2,), POISON, dtype=torch.int64, device=DEV) if counts else None
    ctx.bucket_sum_into(val, key, ed, sums, counts_out=cnt, right=right, mask=mask, zones=zones, tuning=tuning, trace=trace, scratch=scratch)
    return sums.cpu().numpy(), (cnt.cpu().numpy() if counts else None)


def run_minmax(ctx, val, key, edges, right=False, mask=None, zones=None, tuning=None, trace=None, counts=True):
    """bucket_minmax_into on poisoned outputs: (records [B, 2], counts int64[B + 1] or None) as numpy"""
    ed = torch.from_numpy(np.ascontiguousarray(edges)).to(DEV)
    out = torch.full((ed.numel() + 1, 2), NAN, dtype=ed.dtype, device=DEV)
    cnt = torch.full((ed.numel() + 2,), POISON, dtype=torch.int64, device=DEV) if counts else None
    ctx.bucket_minmax_into(val, key, ed, out, counts_out=cnt, right=right, mask=mask, zones=zones, tuning=tuning, trace=trace)
    return out.cpu().numpy(), (cnt.cpu().numpy() if counts else None)


def check(ctx, val, xv, key, xk, edges, right, mask, what, **kw):
    bits = bits_of(mask, xv.size)
    want_s, want_c = host_bucket_sum(xv, xk, bits, edges, right)
    want_r, want_cr = host_bucket_minmax(xv, xk, bits, edges, right)
    assert np.array_equal(want_c, want_cr)
    got_s, got_c = run_sum(ctx, val, key, edges, right=right, mask=mask, **kw)
    got_r, got_cr = run_minmax(ctx, val, key, edges, right=right, mask=mask, **kw)
    assert np.array_equal(got_c, want_c), f"{what}: SUM's counts differ from the replica"
    assert np.array_equal(got_cr, want_c), f"{what}: MIN / MAX's counts differ from the replica"
    assert same_sums(got_s, want_s), f"{what}: sums differ from the documented order in {int((got_s.view(np.uint64) != want_s.view(np.uint64)).sum())} buckets"
    assert same_records(got_r, want_r), f"{what}: records differ from the replica"
    assert int(got_c.sum()) == int(bits.sum())
    return got_s, got_r, got_c


# ---- 1. every tier edge and ballot shape ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("right", [False, True])
@pytest.mark.parametrize("n", [1, 3, 9])
@pytest.mark.parametrize("kind", KINDS)
def test_every_tier_edge_pattern_and_bitmap(ctx, kind, n, right):
    val, xv = value_column(ctx, kind, n)
    for E in EDGE_COUNTS:
        edges = edge_list(E, xv.dtype)
        assert edges.size == E
        for pattern in PATTERNS:
            key, xk = key_column(ctx, pattern, n, E, xv.dtype)
            for mname, mask in masks_of(n, 21 + E).items():
                check(ctx, val, xv, key, xk, edges, right, mask, f"{kind}, {n} vectors, {E} edges, right {right}, {pattern}, bitmap {mname}")
    assert E == capi.BUCKET_EDGES_MAX


@pytest.mark.parametrize("kind,E,pattern,right", [("mixed", 63, "random", False), ("float", 256, "64 distinct per step", True)])
def test_several_vectors_to_a_stripe_and_a_short_last_stripe(ctx, kind, E, pattern, right):
    """4097 vectors: L = 2, 2049 stripes, the last of one vector.  Sparse bitmaps keep the replica quick."""
    n = 4097
    val, xv = value_column(ctx, kind, n)
    key, xk = key_column(ctx, pattern, n, E, xv.dtype)
    L = stripe_vectors(n)
    assert (L, n % L, -(-n // L)) == (2, 1, 2049)
    rnd = random_mask(n, 31, ands=5)
    for mname, mask in (("random", rnd), ("vectors zero", vectors_cleared(rnd, 3))):
        check(ctx, val, xv, key, xk, edge_list(E, xv.dtype), right, mask, f"{kind}, {n} vectors, {E} edges, {pattern}, bitmap {mname}")


# ---- 2. against existing code -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_counts_are_byte_for_byte_the_histogram_of_the_key_column(ctx, kind):
    n = 9
    val, xv = value_column(ctx, kind, n)
    for E in (0, 2, 65, 255, 1023):
        edges = edge_list(E, xv.dtype)
        key, xk = key_column(ctx, "random", n, E, xv.dtype)
        for mname, mask in masks_of(n, 33).items():
            for right in (False, True):
                want = ctx.histogram(key, edges, mask=mask, right=right, sorted=True).cpu().numpy()
                _, c = run_sum(ctx, val, key, edges, right=right, mask=mask)
                _, cr = run_minmax(ctx, val, key, edges, right=right, mask=mask)
                assert c.tobytes() == want.tobytes() == cr.tobytes(), f"{kind}, {E} edges, right {right}, bitmap {mname}"
    other, xo = value_column(ctx, kind, 3)  # a key column with NaNs, exceptions and ALP_RD vectors: the value column of another test as the key
    real = np.unique(xo[~np.isnan(xo)])
    edges = real[:: max(1, real.size // 100)][:100]
    val3, _ = value_column(ctx, kind, 3)
    want = ctx.histogram(other, edges, sorted=True).cpu().numpy()
    assert run_sum(ctx, val3, other, edges)[1].tobytes() == want.tobytes() == run_minmax(ctx, val3, other, edges)[1].tobytes()


@pytest.mark.parametrize("kind", KINDS)
def test_edges_that_are_the_keys_give_keyed_sums_and_keyed_records(ctx, kind):
    """d_edges distinct keys without NaNs, right == 0, every selected key value one of them or below the first: sums[1:] and records[1:] are the keyed calls'"""
    n = 9
    val, xv = value_column(ctx, kind, n)
    for E in (1, 64, 255, 256, 1023):
        keys = (np.arange(E) * 0.25).astype(xv.dtype)
        rng = np.random.default_rng(E)
        xk = np.concatenate([keys, [-1.0, -0.25]]).astype(xv.dtype)[rng.integers(0, E + 2, n * 1024)]
        key, xk = encoded(ctx, ("keyed premise", kind, E), lambda: xk)
        kd = torch.from_numpy(keys).to(DEV)
        for mname, mask in (("none", None), ("random", random_mask(n, 44))):
            s, c = run_sum(ctx, val, key, keys, mask=mask)
            r, _ = run_minmax(ctx, val, key, keys, mask=mask)
            kr, kc, ku = ctx.keyed_minmax(val, key, kd, mask=mask, sorted=True)
            assert r[1:].tobytes() == kr.cpu().numpy().tobytes(), f"{kind}, {E} keys, bitmap {mname}: records"
            assert np.array_equal(c[1: E + 1], kc.cpu().numpy()) and int(c[0]) == int(ku) > 0 and int(c[E + 1]) == 0
            if kind != "float":  # (alpgpu_decode_keyed_sum_f32 is not built)
                ks, _, _ = ctx.keyed_sum(val, key, kd, mask=mask, sorted=True)
                assert same_sums(s[1:], ks.cpu().numpy()), f"{kind}, {E} keys, bitmap {mname}: sums"


# ---- 3. special values ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_column_as_its_own_key(ctx, kind):
    val, xv = value_column(ctx, kind, 3)
    real = np.unique(xv[~np.isnan(xv)])
    edges = np.sort(np.random.default_rng(3).choice(real, min(1023, real.size), replace=False))
    for right in (False, True):
        for mname, mask in masks_of(3, 41).items():
            s, r, c = check(ctx, val, xv, val, xv, edges, right, mask, f"{kind} as its own key, right {right}, bitmap {mname}")
    assert int(c[:-1].sum()) > 0


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_nan_keys_nan_values_both_zeros_and_infinities(ctx, dt):
    def make_key():
        k = key_pool(16, dt)[np.random.default_rng(61).integers(0, 38, 3 * 1024)].copy()
        k[::7] = NAN  # exceptions of ALP vectors
        k[1::11] = -0.0
        k[2::13] = INF
        k[3::17] = -INF
        return k

    def make_rd_key():
        k = np.random.default_rng(62).random(3 * 1024).astype(dt)
        k[::3] = NAN  # an ALP_RD vector holds them in its packed words
        return k

    def make_val():
        x = np.round(np.random.default_rng(63).normal(0, 100, 3 * 1024), 2).astype(dt)
        x[5::64] = NAN
        x[6::64] = INF
        x[7::64] = -0.0
        x[8::64] = 0.0
        return x
    name = np.dtype(dt).name
    val, xv = encoded(ctx, ("special val", name), make_val)
    key, xk = encoded(ctx, ("special key", name), make_key)
    assert np.signbit(xk[xk == 0]).any() and not np.signbit(xk[xk == 0]).all()
    lists = {"an edge of 0.0": np.array([0.0], dt), "an edge of -0.0": np.array([-0.0], dt), "infinite edges": np.array([-INF, -1.0, -0.0, 0.5, INF], dt),
             "duplicates and NaN edges": np.array([-1.0, 0.0, 0.0, 0.0, 0.5, 0.5, NAN, NAN], dt), "the pool": edge_list(16, dt)}
    for what, edges in lists.items():
        for right in (False, True):
            for mask in (None, vectors_cleared(random_mask(3, 64), 2)):
                s, r, c = check(ctx, val, xv, key, xk, edges, right, mask, f"{name}, {what}, right {right}")
                if mask is None:
                    assert int(c[-1]) == int(np.isnan(xk).sum()) > 0 and np.isnan(s).any()
                    if edges.size == 1:  # -0.0 == +0.0: both zeros on the same side of the edge
                        zeros = int((xk == 0).sum())
                        below = int((xk < 0).sum())
                        assert c[0] == below + (zeros if right else 0)
    rdk, xrk = encoded(ctx, ("special rd key", name), make_rd_key)
    _, vec, _, _ = rdk.to_host()
    assert (vec["scheme"] == capi.SCHEME_ALP_RD).all()
    real = np.unique(xrk[~np.isnan(xrk)])
    s, r, c = check(ctx, val, xv, rdk, xrk, np.sort(real[:1023]), False, None, "an ALP_RD key column with NaNs")
    assert int(c[-1]) >= 1024


# ---- 4. the grid does not enter the result ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,E", [("mixed", 65), ("rd", 1023), ("rd", 255), ("float", 256)])
def test_grids_of_1_7_and_the_default_give_the_same_bytes(ctx, kind, E):
    n = 250
    val, xv = value_column(ctx, kind, n)
    key, xk = key_column(ctx, "random", n, E, xv.dtype)
    edges = edge_list(E, xv.dtype)
    mask = random_mask(n, 71)
    bits = unpack_np(mask, xv.size)
    want_s, want_c = host_bucket_sum(xv, xk, bits, edges)
    want_r, _ = host_bucket_minmax(xv, xk, bits, edges)
    runs = []
    for tuning in ({"grid": 1}, {"grid": 7}, None, {"grid": 1000}):  # one workgroup: every wavefront takes many stripes; more than there is work for
        ts, tm = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
        s, c = run_sum(ctx, val, key, edges, mask=mask, tuning=tuning, trace=ts)
        r, cr = run_minmax(ctx, val, key, edges, mask=mask, tuning=tuning, trace=tm)
        assert same_sums(s, want_s) and np.array_equal(c, want_c) and same_records(r, want_r) and np.array_equal(cr, want_c), f"tuning {tuning}"
        assert ts.tolist() == [0, 0, 0, n] == tm.tolist()
        runs.append(np.where(np.isnan(s), NAN, s).tobytes() + c.tobytes() + r.tobytes())  # (a NaN sum: any payload)
    assert len(set(runs)) == 1
    s, c = run_sum(ctx, val, key, edges, mask=mask, counts=False)  # without counts: the same sums and records
    r, cr = run_minmax(ctx, val, key, edges, mask=mask, counts=False)
    assert c is None and cr is None and same_sums(s, want_s) and same_records(r, want_r)


# ---- 5. zone records ----------------------------------------------------------------------------------------------------------------------------------------------
def widened(zones):
    z = zones.cpu().numpy().copy()
    dt = z.dtype.type
    z[:, 0] = np.nextafter(z[:, 0], dt(-INF))
    z[:, 1] = np.nextafter(z[:, 1], dt(INF))
    return torch.from_numpy(z).to(DEV)


def expected_trace(z, vec, edges, right, sel_any):
    """the four trace words from the records, the key vectors' descriptors and the bitmap: histogram's rule on the host"""
    zz = z.cpu().numpy()
    ok = ~np.isnan(zz).any(axis=1)
    a = bucket_of(np.where(ok, zz[:, 0], 0), edges, right)
    b = bucket_of(np.where(ok, zz[:, 1], 0), edges, right)
    one = sel_any & ok & (a == b) & (vec["scheme"] == capi.SCHEME_ALP) & (vec["exc_cnt"] == 0)
    n = sel_any.size
    return [n - int(sel_any.sum()), int(one.sum()), 0, int(sel_any.sum()) - int(one.sum())]


@pytest.mark.parametrize("kind", KINDS)
def test_truthful_and_widened_records_change_no_byte(ctx, kind):
    n, E = 120, 65
    val, xv = value_column(ctx, kind, n)
    edges = edge_list(E, xv.dtype)
    for pattern in ("constant per vector", "random", "two buckets by lane"):
        key, xk = key_column(ctx, pattern, n, E, xv.dtype)
        _, vec, _, _ = key.to_host()
        zones = ctx.zone_map(key)
        holes = zones.clone()
        holes[::3, 0] = NAN  # a NaN bound prunes nothing
        for right in (False, True):
            for mname, mask in (("none", None), ("vectors zero", vectors_cleared(random_mask(n, 81), 3))):
                sel_any = bits_of(mask, xv.size).reshape(n, 1024).any(axis=1)
                plain = check(ctx, val, xv, key, xk, edges, right, mask, f"{kind}, {pattern}: without zones")
                for zname, z in (("the zone map", zones), ("widened", widened(zones)), ("NaN bounds", holes)):
                    ts, tm = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
                    s, c = run_sum(ctx, val, key, edges, right=right, mask=mask, zones=z, trace=ts)
                    r, cr = run_minmax(ctx, val, key, edges, right=right, mask=mask, zones=z, trace=tm)
                    what = f"{kind}, {pattern}, right {right}, bitmap {mname}: {zname}"
                    assert same_sums(s, plain[0]) and r.tobytes() == plain[1].tobytes() and c.tobytes() == plain[2].tobytes() == cr.tobytes(), what + " changed the result"
                    want_t = expected_trace(z, vec, edges, right, sel_any)
                    assert ts.tolist() == want_t == tm.tolist(), f"{what}: trace {ts.tolist()} {tm.tolist()}, expected {want_t}"
                    assert sum(want_t) == n and want_t[2] == 0
                    if pattern == "constant per vector" and zname != "NaN bounds":
                        assert want_t[1] > 0, "the one-bucket shortcut must show in the trace (widened records stay inside a bucket here)"


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_a_sorted_key_column_with_bins_wider_than_a_vector_takes_the_one_bucket_route(ctx, dt):
    n = 60
    name = np.dtype(dt).name
    t0, rows = (1.7e9, 1) if dt == np.float64 else (0.0, 64)  # timestamps in whole seconds, one row each; the float column 64 rows to a second, so that
    key, xk = encoded(ctx, ("sorted key", name), lambda: (t0 + np.arange(n * 1024) // rows).astype(dt))  # its values stay below 1024, where the float encoder takes them without exceptions; min != max in every vector
    val, xv = value_column(ctx, "mixed" if dt == np.float64 else "float", n)
    _, vec, _, _ = key.to_host()
    assert (vec["scheme"] == capi.SCHEME_ALP).all() and (vec["exc_cnt"] == 0).all()
    edges = (t0 + np.arange(1, 25) * (2500.0 / rows)).astype(dt)  # 2500 rows to a bin: about 2.4 vectors
    zones = ctx.zone_map(key)
    for right in (False, True):
        for mask in (None, random_mask(n, 83)):
            plain = check(ctx, val, xv, key, xk, edges, right, mask, f"{name}: sorted keys without zones")
            ts, tm = torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
            s, c = run_sum(ctx, val, key, edges, right=right, mask=mask, zones=zones, trace=ts)
            r, cr = run_minmax(ctx, val, key, edges, right=right, mask=mask, zones=zones, trace=tm)
            assert same_sums(s, plain[0]) and r.tobytes() == plain[1].tobytes() and c.tobytes() == plain[2].tobytes() == cr.tobytes()
            zz = zones.cpu().numpy()
            one = int((bucket_of(zz[:, 0], edges, right) == bucket_of(zz[:, 1], edges, right)).sum())  # the host's count of one-bucket vectors (all ALP without exceptions)
            assert 0 < one < n and ts.tolist() == [0, one, 0, n - one] == tm.tolist()


def test_lying_records_and_unsorted_edges_keep_the_total_and_stay_inside_the_outputs(ctx):
    n = 120
    guard = 64
    for kind, E, pattern in (("mixed", 65, "constant per vector"), ("mixed", 65, "random"), ("float", 1023, "random"), ("rd", 255, "random"), ("float", 1, "two buckets by lane")):
        val, xv = value_column(ctx, kind, n)
        tdt = torch.float64 if xv.dtype == np.float64 else torch.float32
        mask = random_mask(n, 91)
        n_sel = int(unpack_np(mask, xv.size).sum())
        key, xk = key_column(ctx, pattern, n, E, xv.dtype)
        in_order = edge_list(E, xv.dtype)
        unsorted = np.random.default_rng(92).permutation(in_order)
        zones = ctx.zone_map(key)
        lies = {"swapped": zones.flip(1).contiguous(), "shifted": torch.roll(zones, 7, 0).contiguous(), "a point": torch.full_like(zones, 0.25),
                "far above": torch.full_like(zones, 1e30), "infinite": torch.stack([torch.full((n,), INF, dtype=tdt, device=DEV), torch.full((n,), -INF, dtype=tdt, device=DEV)], dim=1).contiguous()}
        cases = [("unsorted edges", unsorted, None), ("unsorted edges with the zone map", unsorted, zones)] + [("records: " + k, in_order, z) for k, z in lies.items()]
        B = E + 1
        for what, edges, z in cases:
            ed = torch.from_numpy(np.ascontiguousarray(edges)).to(DEV)
            for right in (False, True):
                sbuf = torch.full((guard + B + guard,), -12345.5, dtype=torch.float64, device=DEV)
                rbuf = torch.full((guard + B + guard, 2), -12345.5, dtype=tdt, device=DEV)
                cs = torch.full((guard + B + 1 + guard,), POISON, dtype=torch.int64, device=DEV)
                cm = torch.full((guard + B + 1 + guard,), POISON, dtype=torch.int64, device=DEV)
                ctx.bucket_sum_into(val, key, ed, sbuf[guard: guard + B], counts_out=cs[guard: guard + B + 1], right=right, mask=mask, zones=z)
                ctx.bucket_minmax_into(val, key, ed, rbuf[guard: guard + B], counts_out=cm[guard: guard + B + 1], right=right, mask=mask, zones=z)
                ctx.synchronize()
                tag = f"{what}, {kind}, {E} edges, right {right}"
                assert bool((sbuf[:guard] == -12345.5).all()) and bool((sbuf[guard + B:] == -12345.5).all()), f"{tag}: words beside the sums changed"
                assert bool((rbuf[:guard] == -12345.5).all()) and bool((rbuf[guard + B:] == -12345.5).all()), f"{tag}: words beside the records changed"
                for cbuf in (cs, cm):
                    assert bool((cbuf[:guard] == POISON).all()) and bool((cbuf[guard + B + 1:] == POISON).all()), f"{tag}: words beside the counts changed"
                    counts = cbuf[guard: guard + B + 1]
                    assert bool((counts >= 0).all()) and int(counts.sum()) == n_sel, f"{tag}: the total is the selected count"


# ---- 6. capture -----------------------------------------------------------------------------------------------------------------------------------------------------
CAPTURE = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
import datagen
from alp_amd import capi
from bucket_replica import host_bucket_sum, host_bucket_minmax
from keyed_replica import same_sums
ctx = capi.Context(0)
side = torch.cuda.Stream()
ok = True
nv, E = 230, 65
rng = np.random.default_rng(5)
for dt, xv in ((np.float64, datagen.mixed_column(nv, seed=81)), (np.float32, datagen.mixed_column_f32(nv, seed=82))):
    pool = ((np.arange(2 * E + 6) - 5) * 0.125).astype(dt)
    xk = pool[rng.integers(0, pool.size, nv * 1024)]
    edges = pool[3::2][:E].copy()
    val, key = ctx.encode(torch.from_numpy(xv).cuda()), ctx.encode(torch.from_numpy(xk).cuda())
    ed = torch.from_numpy(edges).cuda()
    def bitmap(seed):
        return np.random.default_rng(seed).integers(0, 2**64, 16 * nv, dtype=np.uint64)
    def bits_of(words):
        return ((words[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)
    words = bitmap(6)
    mask = torch.from_numpy(words.view(np.int64)).cuda()
    sums = torch.zeros(E + 1, dtype=torch.float64, device="cuda:0")
    recs = torch.zeros((E + 1, 2), dtype=ed.dtype, device="cuda:0")
    cs = torch.zeros(E + 2, dtype=torch.int64, device="cuda:0")
    cm = torch.zeros(E + 2, dtype=torch.int64, device="cuda:0")
    scratch = ctx.bucket_sum_scratch(nv, E)
    def calls():
        ctx.bucket_sum_into(val, key, ed, sums, counts_out=cs, mask=mask, scratch=scratch, right=True)
        ctx.bucket_minmax_into(val, key, ed, recs, counts_out=cm, mask=mask, right=True)
    with torch.cuda.stream(side):
        calls()                                                 # warm-up on the capture stream
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            calls()
    for rep in range(3):
        if rep == 2:
            words = bitmap(7)                                   # the third replay after the bitmap AND the edges' contents changed
            mask.copy_(torch.from_numpy(words.view(np.int64)).cuda())
            edges = (edges + dt(0.625)).astype(dt)
            ed.copy_(torch.from_numpy(edges).cuda())
        torch.cuda.synchronize()
        sums.fill_(float(rep) - 1.0); recs.fill_(float(rep) - 1.0); cs.fill_(rep - 1); cm.fill_(rep - 1); scratch.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        ws, wc = host_bucket_sum(xv, xk, bits_of(words), edges, True)
        wr, _ = host_bucket_minmax(xv, xk, bits_of(words), edges, True)
        ok = ok and same_sums(sums.cpu().numpy(), ws) and np.array_equal(cs.cpu().numpy(), wc) and np.array_equal(cm.cpu().numpy(), wc) and int(wc.sum()) > 0
        ok = ok and recs.cpu().numpy().tobytes() == wr.tobytes()
        print(np.dtype(dt).name, rep, int(wc.sum()), ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_bitmap_and_the_edges_changed():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 7. argument checks, an empty column, the allocating wrappers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "float"])
def test_c_argument_checks(ctx, kind):
    n, E = 3, 65
    val, xv = value_column(ctx, kind, n)
    key, xk = key_column(ctx, "random", n, E, xv.dtype)
    other, _ = value_column(ctx, kind, 1)
    dtype, vb, tdt = ("f64", 8, torch.float64) if kind == "mixed" else ("f32", 4, torch.float32)
    edges = torch.from_numpy(edge_list(E, xv.dtype)).to(DEV)
    zones = ctx.zone_map(key)
    mask = random_mask(n, 10)
    B = E + 1
    sums = torch.full((B + 8,), 7.5, dtype=torch.float64, device=DEV)
    recs = torch.full((B + 8, 2), 7.5, dtype=tdt, device=DEV)
    cnt = torch.full((B + 9,), POISON, dtype=torch.int64, device=DEV)
    trace = torch.full((5,), POISON, dtype=torch.int64, device=DEV)
    scratch = ctx.bucket_sum_scratch(n, E)
    before = scratch.clone()
    lib = capi.lib
    fs, ds = getattr(lib, "alpgpu_decode_bucket_sum_" + dtype), getattr(lib, "alpgpu_debug_decode_bucket_sum_" + dtype)
    fm, dm = getattr(lib, "alpgpu_decode_bucket_minmax_" + dtype), getattr(lib, "alpgpu_debug_decode_bucket_minmax_" + dtype)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    v, k, o = ctypes.byref(val.c), ctypes.byref(key.c), ctypes.byref(other.c)
    huge_v, huge_k = capi.CColumn.from_buffer_copy(val.c), capi.CColumn.from_buffer_copy(key.c)
    huge_v.n_vectors = huge_k.n_vectors = 2**32
    bare = capi.CColumn()
    bare.n_vectors = n
    hv, hk, bv = ctypes.byref(huge_v), ctypes.byref(huge_k), ctypes.byref(bare)

    def both(why, V=v, K=k, M=None, Z=None, Ed=None, ne=E, S=None, R=None, Cn=None, Sc=None, ctxh=ctx.h, sum_only=False, minmax_only=False):
        M = p(mask) if M is None else M
        Ed = p(edges) if Ed is None else Ed
        Cn = p(cnt) if Cn is None else Cn
        if not minmax_only:
            assert fs(ctxh, V, K, M, Z, Ed, ne, 0, p(sums) if S is None else S, Cn, p(scratch) if Sc is None else Sc) == -2, why + " (SUM)"
        if not sum_only:
            assert fm(ctxh, V, K, M, Z, Ed, ne, 1, p(recs) if R is None else R, Cn) == -2, why + " (MIN / MAX)"
    null = ctypes.c_void_p(None)
    both("a NULL context must be refused", ctxh=None)
    both("a NULL value column must be refused", V=None)
    both("a NULL key column must be refused", K=None)
    both("NULL sums or records must be refused", S=null, R=null)
    both("a NULL scratch must be refused", Sc=null, sum_only=True)
    both("NULL edges with n_edges > 0 must be refused", Ed=null)
    for bad in (1024, 2**32 - 1):
        both("n_edges beyond ALPGPU_BUCKET_EDGES_MAX must be refused", ne=bad)
    both("columns of unequal length must be refused", K=o)
    both("n_vectors beyond 2^32 - 1 must be refused", V=hv, K=hk)
    both("a column without descriptors must be refused", V=bv, K=bv)
    both("a scratch that is not 16-byte aligned must be refused", Sc=p(scratch, 8), sum_only=True)
    both("misaligned sums must be refused", S=p(sums, 4), sum_only=True)
    both("misaligned records must be refused", R=p(recs, vb), minmax_only=True)
    both("misaligned counts must be refused", Cn=p(cnt, 4))
    both("a misaligned bitmap must be refused", M=p(mask, 4))
    both("misaligned edges must be refused", Ed=p(edges, vb // 2))
    both("misaligned zones must be refused", Z=p(zones, vb))
    assert ds(ctx.h, v, k, p(mask), None, p(edges), E, 0, p(sums), p(cnt), p(scratch), None, p(trace, 4)) == -2, "a misaligned trace must be refused"
    assert dm(ctx.h, v, k, p(mask), None, p(edges), E, 0, p(recs), p(cnt), None, p(trace, 4)) == -2, "a misaligned trace must be refused"
    ctx.synchronize()
    assert bool((sums == 7.5).all()) and bool((recs == 7.5).all()) and bool((cnt == POISON).all()) and bool((trace == POISON).all()) and torch.equal(scratch, before), "a refused call wrote"
    # the accepted calls fill exactly their B sums / records and B + 1 counts
    bits = unpack_np(mask, xv.size)
    want_s, want_c = host_bucket_sum(xv, xk, bits, edges.cpu().numpy())
    want_r, _ = host_bucket_minmax(xv, xk, bits, edges.cpu().numpy())
    assert fs(ctx.h, v, k, p(mask), p(zones), p(edges), E, 0, p(sums), p(cnt), p(scratch)) == 0
    ctx.synchronize()
    assert same_sums(sums[:B].cpu().numpy(), want_s) and np.array_equal(cnt[: B + 1].cpu().numpy(), want_c)
    assert bool((sums[B:] == 7.5).all()) and bool((cnt[B + 1:] == POISON).all())
    cnt.fill_(POISON)
    assert fm(ctx.h, v, k, p(mask), p(zones), p(edges), E, 0, p(recs), p(cnt)) == 0
    ctx.synchronize()
    assert same_records(recs[:B].cpu().numpy(), want_r) and np.array_equal(cnt[: B + 1].cpu().numpy(), want_c)
    assert bool((recs[B:] == 7.5).all()) and bool((cnt[B + 1:] == POISON).all())
    # no edges and NULL d_edges: one bucket
    assert fs(ctx.h, v, k, p(mask), None, None, 0, 0, p(sums), p(cnt), p(scratch)) == 0 and fm(ctx.h, v, k, p(mask), None, None, 0, 0, p(recs), p(cnt)) == 0
    ctx.synchronize()
    w1s, w1c = host_bucket_sum(xv, xk, bits, np.zeros(0, xv.dtype))
    assert same_sums(sums[:1].cpu().numpy(), w1s) and cnt[:2].tolist() == w1c.tolist() and same_records(recs[:1].cpu().numpy(), host_bucket_minmax(xv, xk, bits, np.zeros(0, xv.dtype))[0])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_column_of_no_vectors_gives_the_empty_result_everywhere(ctx, dtype):
    empty = capi.CColumn()
    tdt = torch.float64 if dtype == "f64" else torch.float32
    edges = torch.arange(5, dtype=tdt, device=DEV)
    sums = torch.full((8,), -1.0, dtype=torch.float64, device=DEV)
    recs = torch.full((8, 2), -1.0, dtype=tdt, device=DEV)
    cnt = torch.full((9,), POISON, dtype=torch.int64, device=DEV)
    scratch = torch.zeros(64, dtype=torch.uint8, device=DEV)
    assert capi.lib.alpgpu_bucket_sum_scratch_bytes(0, 5) == 64
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    e = ctypes.byref(empty)
    assert getattr(capi.lib, "alpgpu_decode_bucket_sum_" + dtype)(ctx.h, e, e, None, None, p(edges), 5, 0, p(sums), p(cnt), p(scratch)) == 0
    ctx.synchronize()
    assert ibits(sums[:6]).tolist() == [0] * 6 and sums[6:].tolist() == [-1.0, -1.0], "+0.0, and nothing behind the sums"
    assert cnt[:7].tolist() == [0] * 7 and cnt[7:].tolist() == [POISON] * 2
    cnt.fill_(POISON)
    assert getattr(capi.lib, "alpgpu_decode_bucket_minmax_" + dtype)(ctx.h, e, e, None, None, p(edges), 5, 1, p(recs), p(cnt)) == 0
    ctx.synchronize()
    assert recs[:6].tolist() == [[INF, -INF]] * 6 and recs[6:].tolist() == [[-1.0, -1.0]] * 2
    assert cnt[:7].tolist() == [0] * 7 and cnt[7:].tolist() == [POISON] * 2


def test_the_scratch_formula_is_keyed_sums_for_one_more_entry():
    f, g = capi.lib.alpgpu_bucket_sum_scratch_bytes, capi.lib.alpgpu_keyed_sum_scratch_bytes
    for nv in (0, 1, 3, 4096, 4097, 10**6, 2**32 - 1):
        for E in (0, 1, 255, 256, 1023):
            assert f(nv, E) == g(nv, E + 1) == (64 + 8 * (E + 1) * min(nv, 4096) + 15) // 16 * 16
        assert f(nv, 1024) == f(nv, 2**32 - 1) == 2**64 - 1


@pytest.mark.parametrize("kind", ["mixed", "float"])
def test_the_allocating_wrappers_sort_their_edges(ctx, kind):
    n, E = 3, 63
    val, xv = value_column(ctx, kind, n)
    key, xk = key_column(ctx, "random", n, E, xv.dtype)
    edges = edge_list(E, xv.dtype)
    mask = random_mask(n, 5)
    bits = unpack_np(mask, xv.size)
    tdt = torch.float64 if kind == "mixed" else torch.float32
    shuffled = np.random.default_rng(1).permutation(edges)
    for right in (False, True):
        want_s, want_c = host_bucket_sum(xv, xk, bits, edges, right)
        want_r, _ = host_bucket_minmax(xv, xk, bits, edges, right)
        for form in (shuffled, shuffled.tolist(), torch.from_numpy(shuffled), torch.from_numpy(shuffled).to(DEV)):
            s, c = ctx.bucket_sum(val, key, form, right=right, mask=mask, zones=ctx.zone_map(key))
            r, cr = ctx.bucket_minmax(val, key, form, right=right, mask=mask, zones=ctx.zone_map(key))
            assert s.dtype == torch.float64 and r.dtype == tdt and c.dtype == torch.int64 and s.numel() == E + 1 and tuple(r.shape) == (E + 1, 2) and c.numel() == E + 2 == cr.numel()
            assert same_sums(s.cpu().numpy(), want_s) and same_records(r.cpu().numpy(), want_r) and np.array_equal(c.cpu().numpy(), want_c) and np.array_equal(cr.cpu().numpy(), want_c)
    s, c = ctx.bucket_sum(val, key, torch.from_numpy(edges).to(DEV), right=True, mask=mask, counts=False, sorted=True)
    r, cr = ctx.bucket_minmax(val, key, torch.from_numpy(edges).to(DEV), right=True, mask=mask, counts=False, sorted=True)
    assert c is None and cr is None and same_sums(s.cpu().numpy(), want_s) and same_records(r.cpu().numpy(), want_r)
    s, c = ctx.bucket_sum(val, key, [], mask=mask)  # no edges: one bucket
    assert s.numel() == 1 and c.tolist() == [int(bits.sum()), 0]


# ---- 8. the C++ wrappers ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cpp_column_sum_by_bucket_and_minmax_by_bucket_against_decompress_and_a_host_loop(ctx, tmp_path, dtype):
    """include/alp/batch.hpp: alp::gpu::column<PT>::sum_by_bucket and ::minmax_by_bucket of two serialized columns against column::decompress and a host
    loop over integer-valued values, whose sums no order changes (tests/cpp/bucket_test.cpp)"""
    exe = tmp_path / "bucket_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/bucket_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    n, E = 40, 33
    dt = np.float64 if dtype == "f64" else np.float32
    rng = np.random.default_rng(77)
    val, xv = encoded(ctx, ("exact val", dtype), lambda: rng.integers(-(2**20), 2**20 + 1, n * 1024).astype(dt))
    key, xk = key_column(ctx, "random", n, E, dt, seed=3)
    ctx.to_blob(val, xv.size).tofile(str(tmp_path / "val.blob"))
    ctx.to_blob(key, xk.size).tofile(str(tmp_path / "key.blob"))
    edge_list(E, dt).tofile(str(tmp_path / "edges.bin"))
    mask = vectors_cleared(random_mask(n, 53), 3)
    mask[16:32] = -1
    mask.cpu().numpy().tofile(str(tmp_path / "in.mask"))
    p = subprocess.run([str(exe), dtype] + [str(tmp_path / f) for f in ("val.blob", "key.blob", "edges.bin", "in.mask")], capture_output=True, text=True, timeout=600)
    line = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("ok ")]
    assert p.returncode == 0 and len(line) == 1, p.stdout[-3000:] + p.stderr[-2000:]
    k = int(unpack_np(mask, xv.size).sum())
    assert int(line[0][1]) == n and int(line[0][2]) == k and 0 < k < xv.size
