"""GPU: keyed aggregation (include/alpgpu.h, "keyed aggregation": alpgpu_decode_keyed_sum_*).  No expectation comes from the code under test: the
columns' values are the arrays that were encoded (the store decode is held to them bit for bit here and to the oracle by other suites), the sums come
from tests/keyed_replica.py, the documented order on the host, or, for integer-valued columns whose every partial sum is exact, from numpy's integer
sums.  Sums compare bit for bit (NaNs as NaNs), counts as integers."""
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
from keyed_replica import host_keyed_sum, same_sums, stripe_vectors

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF, NAN = math.inf, math.nan
KEY_COUNTS = (1, 2, 63, 64, 65, 1024)
PATTERNS = ("constant per vector", "two keys by lane", "64 distinct per step", "random")
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
    make = {"mixed": lambda: datagen.mixed_column(n, seed=5 + n), "rd": lambda: datagen.rd_column(n, seed=6 + n)}[kind]
    return encoded(ctx, ("val", kind, n), make)


def key_pool(K, dtype):
    """K + 3 distinct keys a quarter apart around zero (decimal: ALP vectors without exceptions), +0.0 among them"""
    return ((np.arange(K + 3) - 5) * 0.25).astype(dtype)


def key_column(ctx, pattern, n, K, dtype, seed=0):
    """a key column over key_pool(K): the list will hold K of the pool's K + 3 values, so that some rows match no key (where the pattern reaches them)"""
    def make():
        rng = np.random.default_rng(1000 * n + K + seed)
        pool = key_pool(K, dtype)
        lane = np.arange(1024) % 64
        if pattern == "constant per vector":
            k = np.repeat(pool[rng.integers(0, K + 3, n)], 1024)
        elif pattern == "two keys by lane":
            pair = rng.integers(0, K + 3, (n, 2))
            k = pool[np.where((lane % 2 == 0)[None, :], pair[:, :1], pair[:, 1:])].reshape(-1)
        elif pattern == "64 distinct per step":
            off = rng.integers(0, K + 3, (n, 16))
            k = pool[(np.repeat(off, 64, axis=1) + lane[None, :]) % (K + 3)].reshape(-1)
        else:
            k = pool[rng.integers(0, K + 3, n * 1024)]
        return k.astype(dtype)
    return encoded(ctx, ("key", pattern, n, K, np.dtype(dtype).name, seed), make)


def key_list(K, dtype):
    """K sorted keys of the pool: its first, its last and one in the middle are left out"""
    pool = key_pool(K, dtype)
    return np.sort(np.delete(pool, [0, (K + 3) // 2, K + 2]))


def run(ctx, val, key, keys, mask=None, zones=None, tuning=None, trace=None, counts=True, scratch=None):
    """keyed_sum_into on poisoned outputs: (sums float64[K] as numpy, counts int64[K + 1] as numpy or None)"""
    kd = torch.from_numpy(np.ascontiguousarray(keys)).to(DEV)
    sums = torch.full((kd.numel(),), NAN, dtype=torch.float64, device=DEV)
    cnt = torch.full((kd.numel() + 1,), POISON, dtype=torch.int64, device=DEV) if counts else None
    ctx.keyed_sum_into(val, key, kd, sums, counts_out=cnt, mask=mask, zones=zones, tuning=tuning, trace=trace, scratch=scratch)
    return sums.cpu().numpy(), (cnt.cpu().numpy() if counts else None)


def check(ctx, val, xv, key, xk, keys, mask, what, **kw):
    total = xv.size
    bits = np.ones(total, bool) if mask is None else unpack_np(mask, total)
    want_s, want_c = host_keyed_sum(xv, xk, bits, keys)
    got_s, got_c = run(ctx, val, key, keys, mask=mask, **kw)
    assert np.array_equal(got_c, want_c), f"{what}: counts differ from the replica"
    assert same_sums(got_s, want_s), f"{what}: sums differ from the documented order in {int((got_s.view(np.uint64) != want_s.view(np.uint64)).sum())} keys"
    assert int(got_c.sum()) == int(bits.sum())
    return got_s, got_c


# ---- 1. exact columns: an expectation that no order enters --------------------------------------------------------------------------------------------------
def exact_columns(ctx, n, K):
    dt = np.float64
    rng = np.random.default_rng(77 + n + K)
    val = encoded(ctx, ("exact val", n), lambda: rng.integers(-(2**20), 2**20 + 1, n * 1024).astype(dt))
    key = key_column(ctx, "random", n, K, dt, seed=3)
    return val, key


@pytest.mark.parametrize("n,K", [(3, 65), (250, 16), (4097, 64), (8193, 1024)])
def test_integer_valued_columns_equal_numpys_integer_sums(ctx, n, K):
    (val, xv), (key, xk) = exact_columns(ctx, n, K)
    keys = key_list(K, xk.dtype)
    assert stripe_vectors(n) == {3: 1, 250: 1, 4097: 2, 8193: 3}[n]
    pos = np.minimum(np.searchsorted(keys, xk), K - 1)
    match = keys[pos] == xk
    xi = xv.astype(np.float64)  # whole numbers of at most 21 bits: every sum of at most 2^23 of them is a whole number below 2^53, exact in any order
    masks = masks_of(n, 11)
    for mname in (masks if n < 4097 else ("none", "vectors zero")):  # (the large columns under two bitmaps: the test stays quick)
        mask = masks[mname]
        bits = np.ones(xv.size, bool) if mask is None else unpack_np(mask, xv.size)
        hit = bits & match
        want_s = np.bincount(pos[hit], weights=xi[hit], minlength=K)
        want_c = np.append(np.bincount(pos[hit], minlength=K), int((bits & ~hit).sum()))
        got_s, got_c = run(ctx, val, key, keys, mask=mask)
        assert np.array_equal(got_c, want_c), f"bitmap {mname}"
        assert np.array_equal(got_s.view(np.uint64), (want_s + 0.0).view(np.uint64)), f"bitmap {mname}: sums differ from numpy's"
        assert int(got_c[K]) > 0 and int(got_c.sum()) == int(bits.sum())


def test_integer_valued_columns_equal_rounds_of_decode_group_sum_and_group_totals(ctx):
    n, K = 250, 65
    (val, xv), (key, xk) = exact_columns(ctx, n, K)
    keys = key_list(K, xk.dtype)
    mask = random_mask(n, 12)
    got_s, got_c = run(ctx, val, key, keys, mask=mask)
    sums, counts = [], []
    for r in range(0, K, 16):  # today's route: ceil(K / 16) rounds, each key a closed range [k, k]
        part = keys[r: r + 16].astype(np.float64).tolist()
        c = torch.zeros((len(part), n), dtype=torch.int32, device=DEV)
        s = ctx.decode_group_sum(val, key, mask, part, part, counts=c)
        ts, tc = ctx.group_totals(s, c)
        sums.append(ts)
        counts.append(tc)
    assert np.array_equal(got_s.view(np.uint64), torch.cat(sums).cpu().numpy().view(np.uint64))
    assert np.array_equal(got_c[:K], torch.cat(counts).cpu().numpy())


# ---- 2. general columns, bit for bit against the replica ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mixed", "rd"])
@pytest.mark.parametrize("n", [1, 3])
def test_small_columns_every_key_count_pattern_and_bitmap(ctx, kind, n):
    val, xv = value_column(ctx, kind, n)
    for K in KEY_COUNTS:
        keys = key_list(K, xv.dtype)
        for pattern in PATTERNS:
            key, xk = key_column(ctx, pattern, n, K, xv.dtype)
            for mname, mask in masks_of(n, 21 + K).items():
                check(ctx, val, xv, key, xk, keys, mask, f"{kind}, {n} vectors, {K} keys, {pattern}, bitmap {mname}")
    assert K == capi.KEYED_KEYS_MAX


@pytest.mark.parametrize("kind,n,K,pattern", [("mixed", 4097, 63, "random"), ("mixed", 4097, 1024, "64 distinct per step"), ("rd", 4097, 2, "two keys by lane"),
                                              ("mixed", 8193, 65, "constant per vector"), ("rd", 8193, 64, "random"), ("rd", 8193, 1024, "random"), ("mixed", 8194, 65, "random")])
def test_several_vectors_to_a_stripe_and_a_short_last_stripe(ctx, kind, n, K, pattern):
    """4097 vectors: L = 2, 2049 stripes, the last of one vector; 8193: L = 3, 2731 whole stripes; 8194: L = 3 and a last stripe of one.  Sparse bitmaps keep the replica quick."""
    val, xv = value_column(ctx, kind, n)
    key, xk = key_column(ctx, pattern, n, K, xv.dtype)
    keys = key_list(K, xv.dtype)
    L = stripe_vectors(n)
    assert (L, n % L) == {4097: (2, 1), 8193: (3, 0), 8194: (3, 1)}[n]
    rnd = random_mask(n, 31, ands=5)
    for mname, mask in (("random", rnd), ("vectors zero", vectors_cleared(rnd, 3))):
        check(ctx, val, xv, key, xk, keys, mask, f"{kind}, {n} vectors, {K} keys, {pattern}, bitmap {mname}")


@pytest.mark.parametrize("kind", ["mixed", "rd"])
def test_a_column_as_its_own_key(ctx, kind):
    val, xv = value_column(ctx, kind, 3)
    real = np.unique(xv[~np.isnan(xv)])
    keys = np.sort(np.random.default_rng(3).choice(real, min(1024, real.size), replace=False))
    for mname, mask in masks_of(3, 41).items():
        s, c = check(ctx, val, xv, val, xv, keys, mask, f"{kind} as its own key, bitmap {mname}")
    assert int(c[-1]) > 0 and int(c[:-1].sum()) > 0


def test_duplicates_both_zeros_and_nans_in_the_key_list(ctx):
    dt = np.float64
    val, xv = value_column(ctx, "mixed", 3)
    key, xk = key_column(ctx, "random", 3, 63, dt)
    assert (xk == 0).any()
    base = key_list(63, dt)
    keys = np.sort(np.concatenate([base, base[10:14], np.array([-0.0], dt)]))  # duplicates, and -0.0 beside +0.0 (numpy.sort keeps either order)
    keys = np.concatenate([keys, np.array([NAN, NAN], dt)])  # NaNs last: never matched
    s, c = check(ctx, val, xv, key, xk, keys, random_mask(3, 51), "duplicates, zeros, NaNs in the list")
    first_zero = int(np.flatnonzero(keys == 0)[0])
    assert c[first_zero] > 0 and c[first_zero + 1] == 0 and s[first_zero + 1] == 0 and not np.signbit(s[first_zero + 1])
    assert c[-3] == 0 and c[-2] == 0 and s[-1] == 0 and s[-2] == 0
    dup = np.flatnonzero(keys[1:] == keys[:-1]) + 1
    assert dup.size >= 5 and not c[dup].any() and not s[dup].any(), "later duplicates receive +0.0 and 0"
    tail = np.sort(np.array([-0.0, 0.0, 0.25, 0.5], dt))  # a NaN-free list whose first two are the zeros
    check(ctx, val, xv, key, xk, tail, None, "a short NaN-free list")


def test_nan_keys_and_nan_values_in_the_columns(ctx):
    dt = np.float64

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
        return x
    val, xv = encoded(ctx, ("nan val",), make_val)
    key, xk = encoded(ctx, ("nan key",), make_key)
    keys = key_list(16, dt)
    s, c = check(ctx, val, xv, key, xk, keys, None, "NaN keys, NaN values")
    assert np.isnan(s).any() and int(c[-1]) >= int(np.isnan(xk).sum())
    s, c = check(ctx, val, xv, key, xk, keys, vectors_cleared(random_mask(3, 64), 2), "NaN keys, NaN values, a bitmap")
    rdk, xrk = encoded(ctx, ("rd nan key",), make_rd_key)
    _, vec, _, _ = rdk.to_host()
    assert (vec["scheme"] == capi.SCHEME_ALP_RD).all()
    real = np.unique(xrk[~np.isnan(xrk)])
    s, c = check(ctx, val, xv, rdk, xrk, np.sort(real[:1024]), None, "an ALP_RD key column with NaNs")
    assert int(c[-1]) >= 1024


# ---- 3. the grid does not enter the result --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,K", [("mixed", 65), ("rd", 1024), ("rd", 256), ("mixed", 257)])
def test_grids_of_1_7_and_the_default_give_the_same_bits(ctx, kind, K):
    n = 250
    val, xv = value_column(ctx, kind, n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    keys = key_list(K, xv.dtype)
    mask = random_mask(n, 71)
    want_s, want_c = host_keyed_sum(xv, xk, unpack_np(mask, xv.size), keys)
    runs = []
    for tuning in ({"grid": 1}, {"grid": 7}, None, {"grid": 1000}):  # one workgroup: every wavefront takes many stripes; more than there is work for
        trace = torch.zeros(4, dtype=torch.int64, device=DEV)
        s, c = run(ctx, val, key, keys, mask=mask, tuning=tuning, trace=trace)
        assert same_sums(s, want_s) and np.array_equal(c, want_c), f"tuning {tuning}"
        assert trace.tolist() == [0, 0, 0, n]
        runs.append(np.where(np.isnan(s), NAN, s).tobytes() + c.tobytes())  # (a NaN sum: any payload)
    assert len(set(runs)) == 1
    s, c = run(ctx, val, key, keys, mask=mask, counts=False)  # without counts: the same sums
    assert c is None and np.where(np.isnan(s), NAN, s).tobytes() == runs[0][: 8 * K]


# ---- 4. zone records ----------------------------------------------------------------------------------------------------------------------------------------------
def widened(zones):
    z = zones.cpu().numpy().copy()
    dt = z.dtype.type
    z[:, 0] = np.nextafter(z[:, 0], dt(-INF))
    z[:, 1] = np.nextafter(z[:, 1], dt(INF))
    return torch.from_numpy(z).to(DEV)


@pytest.mark.parametrize("kind", ["mixed", "rd"])
def test_truthful_and_widened_records_change_no_bit_and_constant_keys_are_settled(ctx, kind):
    n, K = 250, 65
    val, xv = value_column(ctx, kind, n)
    for pattern in ("constant per vector", "random", "two keys by lane"):
        key, xk = key_column(ctx, pattern, n, K, xv.dtype)
        _, vec, _, _ = key.to_host()
        keys = key_list(K, xv.dtype)
        zones = ctx.zone_map(key)
        holes = zones.clone()
        holes[::3, 0] = NAN  # a NaN bound prunes nothing
        for mname, mask in (("none", None), ("vectors zero", vectors_cleared(random_mask(n, 81), 3))):
            bits = np.ones(xv.size, bool) if mask is None else unpack_np(mask, xv.size)
            sel_any = bits.reshape(n, 1024).any(axis=1)
            plain = check(ctx, val, xv, key, xk, keys, mask, f"{kind}, {pattern}: without zones")
            for zname, z in (("the zone map", zones), ("widened", widened(zones)), ("NaN bounds", holes)):
                trace = torch.zeros(4, dtype=torch.int64, device=DEV)
                s, c = run(ctx, val, key, keys, mask=mask, zones=z, trace=trace)
                assert same_sums(s, plain[0]) and c.tobytes() == plain[1].tobytes(), f"{kind}, {pattern}, bitmap {mname}: {zname} changed the result"  # (a NaN sum: any payload)
                zz = z.cpu().numpy()
                ok = ~np.isnan(zz).any(axis=1)
                j0 = np.searchsorted(keys, np.where(ok, zz[:, 0], 0), side="left")
                j1 = np.searchsorted(keys, np.where(ok, zz[:, 1], 0), side="right")
                no_key = sel_any & ok & (j1 <= j0)
                const = sel_any & ok & (j1 > j0) & (zz[:, 0] == zz[:, 1]) & (vec["scheme"] == capi.SCHEME_ALP) & (vec["exc_cnt"] == 0)
                t = trace.tolist()
                assert t == [n - int(sel_any.sum()), int(const.sum()), int(no_key.sum()), int(sel_any.sum()) - int(const.sum()) - int(no_key.sum())], f"{pattern}, {zname}: trace {t}"
                if pattern == "constant per vector" and zname == "the zone map":
                    assert t[1] > 0 and t[2] > 0, "the constant-key shortcut must show in the trace"
                if pattern == "constant per vector" and zname == "widened":
                    assert t[1] == 0


def test_lying_records_and_unsorted_keys_keep_the_total_and_stay_inside_the_outputs(ctx):
    n = 250
    val, xv = value_column(ctx, "mixed", n)
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
            sbuf = torch.full((guard + K + guard,), -12345.5, dtype=torch.float64, device=DEV)
            cbuf = torch.full((guard + K + 1 + guard,), POISON, dtype=torch.int64, device=DEV)
            ctx.keyed_sum_into(val, key, kd, sbuf[guard: guard + K], counts_out=cbuf[guard: guard + K + 1], mask=mask, zones=z)
            ctx.synchronize()
            assert bool((sbuf[:guard] == -12345.5).all()) and bool((sbuf[guard + K:] == -12345.5).all()), f"{what}, {K} keys: words beside the sums changed"
            assert bool((cbuf[:guard] == POISON).all()) and bool((cbuf[guard + K + 1:] == POISON).all()), f"{what}, {K} keys: words beside the counts changed"
            counts = cbuf[guard: guard + K + 1]
            assert bool((counts >= 0).all()) and int(counts.sum()) == n_sel, f"{what}, {K} keys: the total is the selected count"


# ---- 5. capture -----------------------------------------------------------------------------------------------------------------------------------------------------
CAPTURE = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
import datagen
from alp_amd import capi
from keyed_replica import host_keyed_sum, same_sums
ctx = capi.Context(0)
side = torch.cuda.Stream()
ok = True
nv, K = 230, 65
rng = np.random.default_rng(5)
xv = datagen.mixed_column(nv, seed=81)
pool = (np.arange(K + 3) - 5) * 0.25
xk = pool[rng.integers(0, K + 3, nv * 1024)]
keys = np.sort(np.delete(pool, [0, 30, K + 2]))
val, key = ctx.encode(torch.from_numpy(xv).cuda()), ctx.encode(torch.from_numpy(xk).cuda())
kd = torch.from_numpy(keys).cuda()
def bitmap(seed):
    return np.random.default_rng(seed).integers(0, 2**64, 16 * nv, dtype=np.uint64)
def bits_of(words):
    return ((words[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(-1)
words = bitmap(6)
mask = torch.from_numpy(words.view(np.int64)).cuda()
sums = torch.zeros(K, dtype=torch.float64, device="cuda:0")
cnt = torch.zeros(K + 1, dtype=torch.int64, device="cuda:0")
scratch = ctx.keyed_sum_scratch(nv, K)
def calls():
    ctx.keyed_sum_into(val, key, kd, sums, counts_out=cnt, mask=mask, scratch=scratch)
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
    sums.fill_(float(rep) - 1.0); cnt.fill_(rep - 1); scratch.fill_(0xA5)
    g.replay()
    torch.cuda.synchronize()
    ws, wc = host_keyed_sum(xv, xk, bits_of(words), keys)
    ok = ok and same_sums(sums.cpu().numpy(), ws) and np.array_equal(cnt.cpu().numpy(), wc) and int(wc.sum()) > 0
    print(rep, int(wc.sum()), ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_bitmap_changed():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 6. argument checks, an empty column, the allocating wrapper ------------------------------------------------------------------------------------------------
def test_c_argument_checks(ctx):
    n, K = 3, 65
    val, xv = value_column(ctx, "mixed", n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    other, _ = value_column(ctx, "mixed", 1)
    dtype, vb = "f64", 8
    keys = torch.from_numpy(key_list(K, xv.dtype)).to(DEV)
    zones = ctx.zone_map(key)
    mask = random_mask(n, 10)
    sums = torch.full((K + 8,), 7.5, dtype=torch.float64, device=DEV)
    cnt = torch.full((K + 9,), POISON, dtype=torch.int64, device=DEV)
    trace = torch.full((5,), POISON, dtype=torch.int64, device=DEV)
    scratch = ctx.keyed_sum_scratch(n, K)
    before = scratch.clone()
    fn, dbg = getattr(capi.lib, "alpgpu_decode_keyed_sum_" + dtype), getattr(capi.lib, "alpgpu_debug_decode_keyed_sum_" + dtype)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    v, k, o = ctypes.byref(val.c), ctypes.byref(key.c), ctypes.byref(other.c)
    assert fn(None, v, k, p(mask), None, p(keys), K, p(sums), p(cnt), p(scratch)) == -2, "a NULL context must be refused"
    assert fn(ctx.h, None, k, p(mask), None, p(keys), K, p(sums), p(cnt), p(scratch)) == -2, "a NULL value column must be refused"
    assert fn(ctx.h, v, None, p(mask), None, p(keys), K, p(sums), p(cnt), p(scratch)) == -2, "a NULL key column must be refused"
    assert fn(ctx.h, v, k, p(mask), None, None, K, p(sums), p(cnt), p(scratch)) == -2, "NULL keys must be refused"
    assert fn(ctx.h, v, k, p(mask), None, p(keys), K, None, p(cnt), p(scratch)) == -2, "NULL sums must be refused"
    assert fn(ctx.h, v, k, p(mask), None, p(keys), K, p(sums), p(cnt), None) == -2, "a NULL scratch must be refused"
    for bad in (0, 1025, 2**32 - 1):
        assert fn(ctx.h, v, k, p(mask), None, p(keys), bad, p(sums), p(cnt), p(scratch)) == -2, "n_keys outside 1 .. 1024 must be refused"
    assert fn(ctx.h, v, o, p(mask), None, p(keys), K, p(sums), p(cnt), p(scratch)) == -2, "columns of unequal length must be refused"
    assert fn(ctx.h, v, k, p(mask), None, p(keys), K, p(sums), p(cnt), p(scratch, 8)) == -2, "a scratch that is not 16-byte aligned must be refused"
    assert fn(ctx.h, v, k, p(mask), None, p(keys), K, p(sums, 4), p(cnt), p(scratch)) == -2, "misaligned sums must be refused"
    assert fn(ctx.h, v, k, p(mask), None, p(keys), K, p(sums), p(cnt, 4), p(scratch)) == -2, "misaligned counts must be refused"
    assert fn(ctx.h, v, k, p(mask, 4), None, p(keys), K, p(sums), p(cnt), p(scratch)) == -2, "a misaligned bitmap must be refused"
    assert fn(ctx.h, v, k, p(mask), None, p(keys, vb // 2), K, p(sums), p(cnt), p(scratch)) == -2, "misaligned keys must be refused"
    assert fn(ctx.h, v, k, p(mask), p(zones, vb), p(keys), K, p(sums), p(cnt), p(scratch)) == -2, "misaligned zones must be refused"
    assert dbg(ctx.h, v, k, p(mask), None, p(keys), K, p(sums), p(cnt), p(scratch), None, p(trace, 4)) == -2, "a misaligned trace must be refused"
    ctx.synchronize()
    assert bool((sums == 7.5).all()) and bool((cnt == POISON).all()) and bool((trace == POISON).all()) and torch.equal(scratch, before), "a refused call wrote"
    # the accepted call fills exactly its K sums and K + 1 counts
    assert fn(ctx.h, v, k, p(mask), p(zones), p(keys), K, p(sums), p(cnt), p(scratch)) == 0
    ctx.synchronize()
    want_s, want_c = host_keyed_sum(xv, xk, unpack_np(mask, xv.size), keys.cpu().numpy())
    assert same_sums(sums[:K].cpu().numpy(), want_s) and np.array_equal(cnt[: K + 1].cpu().numpy(), want_c)
    assert bool((sums[K:] == 7.5).all()) and bool((cnt[K + 1:] == POISON).all())


def test_a_column_of_no_vectors_gives_plus_zero_and_zero_everywhere(ctx):
    empty = capi.CColumn()
    fn = capi.lib.alpgpu_decode_keyed_sum_f64
    keys = torch.arange(5, dtype=torch.float64, device=DEV)
    sums = torch.full((7,), -1.0, dtype=torch.float64, device=DEV)
    cnt = torch.full((8,), POISON, dtype=torch.int64, device=DEV)
    scratch = torch.zeros(64, dtype=torch.uint8, device=DEV)
    assert capi.lib.alpgpu_keyed_sum_scratch_bytes(0, 5) == 64
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert fn(ctx.h, ctypes.byref(empty), ctypes.byref(empty), None, None, p(keys), 5, p(sums), p(cnt), p(scratch)) == 0
    ctx.synchronize()
    assert ibits(sums[:5]).tolist() == [0] * 5 and sums[5:].tolist() == [-1.0, -1.0], "+0.0, and nothing behind the sums"
    assert cnt[:6].tolist() == [0] * 6 and cnt[6:].tolist() == [POISON] * 2


def test_the_allocating_wrapper_sorts_its_keys(ctx):
    n, K = 3, 63
    val, xv = value_column(ctx, "mixed", n)
    key, xk = key_column(ctx, "random", n, K, xv.dtype)
    keys = key_list(K, xv.dtype)
    mask = random_mask(n, 5)
    want_s, want_c = host_keyed_sum(xv, xk, unpack_np(mask, xv.size), keys)
    shuffled = np.random.default_rng(1).permutation(keys)
    for form in (shuffled, shuffled.tolist(), torch.from_numpy(shuffled), torch.from_numpy(shuffled).to(DEV)):
        s, c, u = ctx.keyed_sum(val, key, form, mask=mask, zones=ctx.zone_map(key))
        assert s.dtype == torch.float64 and c.dtype == torch.int64 and s.numel() == K == c.numel()
        assert same_sums(s.cpu().numpy(), want_s) and np.array_equal(c.cpu().numpy(), want_c[:K]) and int(u) == int(want_c[K])
    s, c, u = ctx.keyed_sum(val, key, torch.from_numpy(keys).to(DEV), mask=mask, counts=False, sorted=True)
    assert c is None and u is None and same_sums(s.cpu().numpy(), want_s)


# ---- 7. the C++ wrapper ---------------------------------------------------------------------------------------------------------------------------------------------
def test_cpp_column_sum_by_key_against_decompress_and_a_host_loop(ctx, tmp_path):
    """include/alp/batch.hpp: alp::gpu::column<double>::sum_by_key of two serialized columns against column::decompress and a host loop over
    integer-valued values, whose sums no order changes (tests/cpp/keyed_test.cpp)"""
    exe = tmp_path / "keyed_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/keyed_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    dtype = "f64"
    n, K = 250, 65
    (val, xv), (key, xk) = exact_columns(ctx, n, K)
    ctx.to_blob(val, xv.size).tofile(str(tmp_path / "val.blob"))
    ctx.to_blob(key, xk.size).tofile(str(tmp_path / "key.blob"))
    keys = key_list(K, xk.dtype)
    keys.tofile(str(tmp_path / "keys.bin"))
    mask = vectors_cleared(random_mask(n, 53), 3)
    mask[16:32] = -1
    mask.cpu().numpy().tofile(str(tmp_path / "in.mask"))
    p = subprocess.run([str(exe), dtype] + [str(tmp_path / f) for f in ("val.blob", "key.blob", "keys.bin", "in.mask")], capture_output=True, text=True, timeout=600)
    line = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("ok ")]
    assert p.returncode == 0 and len(line) == 1, p.stdout[-3000:] + p.stderr[-2000:]
    k = int(unpack_np(mask, xv.size).sum())
    assert int(line[0][1]) == n and int(line[0][2]) == k and 0 < k < xv.size
