"""GPU: distinct values (include/alpgpu.h, "distinct values": alpgpu_distinct_*).  The expected values and counts never come from the code under test:
x = ctx.decode(col) (pinned to the oracle and the reference by other suites) goes through the host replica (tests/distinct_replica.py: numpy.unique).
Values compare by their bytes, counts and state words as integers.  Every output buffer is poisoned and has guard words behind `capacity` that must
survive; without overflow nothing is written behind the D entries either."""
import ctypes
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from alp_amd import capi
from distinct_replica import host_distinct, is_nan_bits, unpack_mask

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF, NAN = math.inf, math.nan
POISON = 0x5A5A5A5A5A5A5A5A
GUARD = 32


def np_dtype(dtype):
    return np.float64 if dtype == "f64" else np.float32


def random_mask(n_vectors, seed):
    words = np.random.default_rng(seed).integers(0, 2**64, 16 * n_vectors, dtype=np.uint64)
    return torch.from_numpy(words.view(np.int64)).to(DEV)


def vectors_cleared(mask, keep_every):
    """the mask with every keep_every-th vector zeroed in all 16 words: skipped vectors beside decoded ones"""
    m = mask.clone().reshape(-1, 16)
    v = torch.arange(m.shape[0], device=mask.device)
    m[(v % keep_every) == 1] = 0
    return m.reshape(-1)


def selection(total, mask, first, n):
    r = np.arange(total)
    sel = (r >= first) & (r < first + n)
    return sel if mask is None else sel & unpack_mask(mask.cpu().numpy(), total)


_cache = {}


def encoded(ctx, key, make):
    """(DeviceColumn, the store decode on the host), encoded once per session and left unchanged"""
    if key not in _cache:
        xd = torch.from_numpy(np.ascontiguousarray(make())).to(DEV)
        col = ctx.encode(xd)
        dec = ctx.decode(col)
        assert torch.equal(dec.view(torch.uint8), xd.view(torch.uint8)), f"{key}: decode(encode(x)) != x"
        _cache[key] = (col, dec.cpu().numpy())
    return _cache[key]


KEYS16 = [-INF, -1234.5, -7.25, -1.5, -0.0, 0.0, 0.5, 1.5, 2.25, 3.0, 17.75, 100.5, 4096.0, 65000.25, 99999.5, INF]  # 15 distinct values: the zeros are one


def keys_column(ctx, dtype, nv):
    """16 keys with both zeros and +-inf, and NaNs: in these ALP vectors the NaNs, the zeros' -0.0 and the infinities are exceptions"""
    def make():
        rng = np.random.default_rng(100 + nv)
        x = rng.choice(np.array(KEYS16, np_dtype(dtype)), 1024 * nv)
        x[rng.integers(0, x.size, 5 * nv)] = NAN
        return x
    return encoded(ctx, ("keys", dtype, nv), make)


def constant_column(ctx, dtype, nv):
    return encoded(ctx, ("const", dtype, nv), lambda: np.full(1024 * nv, 5.25, np_dtype(dtype)))


def nan_column(ctx, dtype, nv):
    return encoded(ctx, ("nan", dtype, nv), lambda: np.full(1024 * nv, NAN, np_dtype(dtype)))


def all_distinct_column(ctx, dtype):
    """8 vectors, 8192 distinct values (halves: exact in both types), in no order; one of them is 0.0"""
    return encoded(ctx, ("distinct", dtype), lambda: ((np.random.default_rng(8).permutation(8192) - 4096) * 0.5).astype(np_dtype(dtype)))


def sorted_keys_column(ctx, dtype):
    """12 vectors of 7 keys in ascending order: most vectors hold one value, the others two"""
    def make():
        rng = np.random.default_rng(12)
        return np.sort(rng.choice(np.array([1.5, 2.5, 3.5, 7.0, 8.5, 100.0, 250.5], np_dtype(dtype)), 12 * 1024))
    return encoded(ctx, ("sorted", dtype), make)


class Out:
    """the poisoned buffers of one call with their guard words; run() makes the call and checks what may never be written"""

    def __init__(self, dtype, capacity, counts=True):
        it = torch.int64 if dtype == "f64" else torch.int32
        self.capacity = capacity
        self.vals_raw = torch.full((capacity + GUARD,), POISON if dtype == "f64" else 0x5A5A5A5A, dtype=it, device=DEV)
        self.vals = self.vals_raw[:capacity].view(torch.float64 if dtype == "f64" else torch.float32)
        self.counts_raw = torch.full((capacity + GUARD,), POISON, dtype=torch.int64, device=DEV) if counts else None
        self.counts = self.counts_raw[:capacity] if counts else None
        self.state_raw = torch.full((4 + GUARD,), POISON, dtype=torch.int64, device=DEV)
        self.state = self.state_raw[:4]

    def run(self, ctx, col, **kw):
        ctx.distinct_into(col, self.vals, self.state, counts_out=self.counts, **kw)
        ctx.synchronize()
        poison_v = POISON if self.vals_raw.dtype == torch.int64 else 0x5A5A5A5A
        assert bool((self.vals_raw[self.capacity:] == poison_v).all()), "guard words behind the values changed"
        assert self.counts_raw is None or bool((self.counts_raw[self.capacity:] == POISON).all()), "guard words behind the counts changed"
        assert bool((self.state_raw[4:] == POISON).all()), "guard words behind the state changed"
        d, n_nan, n_num, overflow = self.state.tolist()
        assert 0 <= d <= self.capacity and overflow in (0, 1)
        if not overflow:
            assert bool((self.vals_raw[d:] == poison_v).all()), "values were written behind the D entries"
            assert self.counts_raw is None or bool((self.counts_raw[d:] == POISON).all()), "counts were written behind the D entries"
        return d, n_nan, n_num, overflow

    def bytes(self):
        return self.vals_raw.cpu().numpy().tobytes() + (b"" if self.counts_raw is None else self.counts_raw.cpu().numpy().tobytes()) + self.state_raw.cpu().numpy().tobytes()


def check(out, state, want, what):
    """the call's entries and state against the replica's (values, counts, n_nan, n_numbers)"""
    values, counts, n_nan, n_num = want
    d = values.size
    assert list(state) == [d, n_nan, n_num, 0], f"{what}: state {list(state)}, want {[d, n_nan, n_num, 0]}"
    got = out.vals[:d].cpu().numpy()
    assert got.tobytes() == values.tobytes(), f"{what}: the values differ from the replica's"
    if out.counts is not None:
        assert np.array_equal(out.counts[:d].cpu().numpy().view(np.uint64), counts), f"{what}: the counts differ from the replica's"
        assert int(out.counts[:d].sum()) == n_num, "the counts add up to state word 2"


# ---- 1. columns encoded by the context, of 1, 3 and 9 vectors: values, ranges, bitmaps, both precisions ----------------------------------------------------
@pytest.mark.parametrize("nv", [1, 3, 9])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_keys_constant_and_nan_columns_over_ranges_and_bitmaps(ctx, dtype, nv):
    total = 1024 * nv
    rnd = random_mask(nv, 20 + nv)
    masks = {"none": None, "random": rnd, "all zero": torch.zeros_like(rnd), "every third vector cleared": vectors_cleared(rnd, 3)}
    ranges = [(0, 1), (0, 63), (1000, 100) if nv > 1 else (1000, 24), (0, total)]
    seen_nan = seen_zero = False
    for cname, (col, xs) in (("keys", keys_column(ctx, dtype, nv)), ("constant", constant_column(ctx, dtype, nv)), ("all NaN", nan_column(ctx, dtype, nv))):
        for mname, mask in masks.items():
            for first, n in ranges:
                want = host_distinct(xs, selection(total, mask, first, n))
                out = Out(dtype, 40)
                state = out.run(ctx, col, mask=mask, first=first, n=n)
                check(out, state, want, f"{dtype} {cname} of {nv} vectors, bitmap {mname}, first={first} n={n}")
                seen_nan = seen_nan or (cname == "keys" and want[2] > 0)
                seen_zero = seen_zero or bool((want[0] == 0).any())
        # the allocating form
        values, counts, n_nan, overflow = ctx.distinct(col, mask=rnd)
        want = host_distinct(xs, selection(total, rnd, 0, total))
        assert values.cpu().numpy().tobytes() == want[0].tobytes() and np.array_equal(counts.cpu().numpy().view(np.uint64), want[1]) and (n_nan, overflow) == (want[2], False)
        assert ctx.distinct(col, counts=False)[1] is None
    assert seen_nan and seen_zero
    _, xs = keys_column(ctx, dtype, nv)
    both = xs[xs == 0]
    assert np.signbit(both).any() and not np.signbit(both).all(), "the keys column holds both zeros"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_nans_of_every_kind_are_counted_and_never_values(ctx, dtype):
    """quiet, signalling and negative NaNs, as exceptions of ALP vectors and as packed values of an ALP_RD vector"""
    dt = np_dtype(dtype)
    u = np.uint64 if dtype == "f64" else np.uint32
    odd = np.array([0x7FF0000000000001, 0xFFF8000000000000, 0x7FF8000000000000] if dtype == "f64" else [0x7F800001, 0xFFC00000, 0x7FC00000], dtype=u).view(dt)

    def alp():
        x = np.random.default_rng(3).choice(np.array([1.5, 2.5, -0.0], dt), 2048)
        x[5:2048:97] = np.resize(odd, x[5:2048:97].size)
        return x

    def rd():
        x = np.random.default_rng(4).random(2048).astype(dt)
        x[::3] = np.resize(odd, x[::3].size)
        return x
    for name, make in (("alp", alp), ("rd", rd)):
        col, xs = encoded(ctx, ("nans", name, dtype), make)
        want = host_distinct(xs)
        assert want[2] == int(is_nan_bits(xs).sum()) > 0
        out = Out(dtype, 2048)
        check(out, out.run(ctx, col), want, f"{dtype} {name}")


# ---- 2. every value distinct: capacities, overflow, the sort's sizes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_value_distinct_at_and_beyond_the_capacity(ctx, dtype):
    col, xs = all_distinct_column(ctx, dtype)
    D = 8192
    want = host_distinct(xs)
    assert want[0].size == D and int(want[1].max()) == 1
    out = Out(dtype, D)
    check(out, out.run(ctx, col), want, f"{dtype}, capacity == D")
    mask = random_mask(8, 81)
    sel = selection(D, mask, 0, D)
    n_sel = int(sel.sum())  # (every value is distinct: as many distinct values as selected ones)
    assert 1 < n_sel < 5000
    for capacity in (D - 1, 1, 5000, n_sel - 1, n_sel):
        for m, n_distinct in ((None, D), (mask, n_sel)):
            out = Out(dtype, capacity)
            state = out.run(ctx, col, mask=m)
            if n_distinct > capacity:  # the flag, the entries written = the capacity, the totals right (the guards: run())
                assert state == (capacity, 0, n_distinct, 1), f"{dtype}, capacity {capacity}, {n_distinct} distinct values: state {state}"
            else:
                check(out, state, host_distinct(xs, None if m is None else sel), f"{dtype}, capacity {capacity}, {n_distinct} distinct values")
    values, counts, n_nan, overflow = ctx.distinct(col, capacity=100)
    assert overflow and n_nan == 0


@pytest.mark.parametrize("D", [1, 2, 64, 65, 4096, 4097])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_sort_at_its_sizes(ctx, dtype, D):
    """D distinct values (the first D of the all-distinct column) against a tile of 64 and the default, with the capacity D and one well above it"""
    col, xs = all_distinct_column(ctx, dtype)
    want = host_distinct(xs[:D])
    assert want[0].size == D
    runs = []
    for capacity in (D, 8192):
        for tuning in (None, {"sort_tile": 64}, {"sort_tile": 1}, {"sort_tile": 100}):
            out = Out(dtype, capacity)
            check(out, out.run(ctx, col, first=0, n=D, tuning=tuning), want, f"{dtype}, D {D}, capacity {capacity}, tuning {tuning}")
            runs.append(out.vals[:D].cpu().numpy().tobytes() + out.counts[:D].cpu().numpy().tobytes())
    assert len(set(runs)) == 1


# ---- 3. tuning: no field changes a byte; the trace shows the paths ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_tuning_changes_no_byte(ctx, dtype):
    col, xs = keys_column(ctx, dtype, 9)
    mask = random_mask(9, 31)
    want = host_distinct(xs, selection(xs.size, mask, 0, xs.size))
    runs = []
    # one workgroup of 8 wavefronts makes 2 trips over 9 vectors: flush_every = 1 flushes in the loop after each
    for tuning in (None, {"grid": 1}, {"grid": 1000}, {"flush_every": 1}, {"grid": 1, "flush_every": 1}, {"lds_slots": 64}, {"lds_slots": 1}, {"table_slots": 64}, {"table_slots": 1},
                   {"sort_tile": 64}, {"grid": 2, "flush_every": 1, "lds_slots": 64, "table_slots": 64, "sort_tile": 64}):
        out = Out(dtype, 40)
        trace = torch.zeros(6, dtype=torch.int64, device=DEV)
        check(out, out.run(ctx, col, mask=mask, tuning=tuning, trace=trace), want, f"{dtype}, tuning {tuning}")
        t = trace.tolist()
        assert t[:3] == [0, 0, 9] and t[4] >= t[3] and t[5] >= want[0].size, f"tuning {tuning}: trace {t}"
        runs.append(out.bytes())
    assert len(set(runs)) == 1


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_tiny_lds_table_sends_values_straight_to_the_global_table(ctx, dtype):
    """300 distinct values in one vector against 64 LDS slots: most find no place within the probe bound"""
    def make():
        rng = np.random.default_rng(300)
        x = rng.choice((np.arange(300) * 0.25 - 20).astype(np_dtype(dtype)), 1024)
        x[:300] = (np.arange(300) * 0.25 - 20).astype(np_dtype(dtype))
        return x
    col, xs = encoded(ctx, ("300", dtype), make)
    want = host_distinct(xs)
    assert want[0].size == 300
    ref_bytes, made = None, {}
    for tuning in (None, {"lds_slots": 64}):
        out = Out(dtype, 300)
        trace = torch.zeros(6, dtype=torch.int64, device=DEV)
        check(out, out.run(ctx, col, tuning=tuning, trace=trace), want, f"{dtype}, tuning {tuning}")
        t = trace.tolist()
        assert t[:3] == [0, 0, 1] and t[5] >= 300, f"tuning {tuning}: trace {t}"
        made[tuning is None] = t[5]
        ref_bytes = ref_bytes or out.bytes()
        assert out.bytes() == ref_bytes
    assert made[False] > 300 and made[False] > made[True], f"the tiny table sends values straight to the global table: {made}"
    assert made[True] < 330, "the default table holds (nearly) all 300 values: one flushed entry each"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_full_global_table_with_wrapped_probes_is_exact(ctx, dtype):
    col, xs = all_distinct_column(ctx, dtype)
    for D in (64, 4096):
        want = host_distinct(xs[:D])
        out = Out(dtype, D)
        trace = torch.zeros(6, dtype=torch.int64, device=DEV)
        check(out, out.run(ctx, col, first=0, n=D, tuning={"table_slots": D, "grid": 3}, trace=trace), want, f"{dtype}: {D} values in {D} slots")
        assert trace[5] >= D
        # one value more than the table has slots: the flag, the totals right
        out = Out(dtype, D)
        assert out.run(ctx, col, first=0, n=D + 1, tuning={"table_slots": D}) == (D, 0, D + 1, 1)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_steps_that_agree_are_one_insert(ctx, dtype):
    for nv in (1, 9):
        col, xs = constant_column(ctx, dtype, nv)
        out = Out(dtype, 4)
        trace = torch.zeros(6, dtype=torch.int64, device=DEV)
        check(out, out.run(ctx, col, trace=trace), host_distinct(xs), f"{dtype} constant")
        t = trace.tolist()
        assert t[:5] == [0, 0, nv, 16 * nv, 16 * nv], f"every step of the constant column is settled by agreement: trace {t}"
        assert 1 <= t[5] <= nv, "one flushed entry per workgroup that had a vector"
    # alternating values: no step agrees
    col, xs = encoded(ctx, ("alt", dtype), lambda: np.where(np.arange(2048) % 2 == 0, 1.5, 3.5).astype(np_dtype(dtype)))
    out = Out(dtype, 4)
    trace = torch.zeros(6, dtype=torch.int64, device=DEV)
    check(out, out.run(ctx, col, trace=trace), host_distinct(xs), f"{dtype} alternating")
    assert trace.tolist()[:5] == [0, 0, 2, 0, 2048]


# ---- 4. zone maps ------------------------------------------------------------------------------------------------------------------------------------------------
def widened(zones):
    z = zones.cpu().numpy().copy()
    dt = z.dtype.type
    with np.errstate(over="ignore"):
        z[:, 0] = np.nextafter(z[:, 0], dt(-INF))
        z[:, 1] = np.nextafter(z[:, 1], dt(INF))
    return torch.from_numpy(z).to(DEV)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_truthful_records_change_no_byte(ctx, dtype):
    settled_some = False
    for cname, (col, xs) in (("keys", keys_column(ctx, dtype, 9)), ("sorted", sorted_keys_column(ctx, dtype)), ("constant", constant_column(ctx, dtype, 9))):
        nv, total = col.n_vectors, xs.size
        _, vec, _, _ = col.to_host()
        zones = ctx.zone_map(col)
        mask = vectors_cleared(random_mask(nv, 41), 3)
        masked = ctx.decode_minmax_masked(col, mask)
        first, n = 100, total - 600  # the first and the last vector cut by the range
        for m, records in ((None, {"the zone map": zones, "widened": widened(zones)}),
                           (mask, {"the zone map": zones, "widened": widened(zones), "masked": masked, "masked widened": widened(masked)})):
            sel = selection(total, m, first, n)
            want = host_distinct(xs, sel)
            plain = Out(dtype, 64)
            check(plain, plain.run(ctx, col, mask=m, first=first, n=n), want, f"{dtype} {cname}: without zones")
            for zname, z in records.items():
                out = Out(dtype, 64)
                trace = torch.zeros(6, dtype=torch.int64, device=DEV)
                out.run(ctx, col, mask=m, first=first, n=n, zones=z, trace=trace)
                assert out.bytes() == plain.bytes(), f"{dtype} {cname}: {zname} changed the output"
                zh = z.cpu().numpy()
                sel_any = sel.reshape(nv, 1024).any(axis=1)
                by_record = sel_any & (zh[:, 0] == zh[:, 1]) & (vec["scheme"] == capi.SCHEME_ALP) & (vec["exc_cnt"] == 0)
                t = trace.tolist()
                assert t[:3] == [nv - int(sel_any.sum()), int(by_record.sum()), int(sel_any.sum()) - int(by_record.sum())], f"{dtype} {cname}, {zname}: trace {t}"
                settled_some = settled_some or (cname == "sorted" and zname == "the zone map" and 0 < t[1] and 0 < t[2])
    assert settled_some, "the sorted key column settled no vector from its record, or every one"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_lying_records_keep_the_totals_and_stay_inside_the_buffers(ctx, dtype):
    for col, xs in (keys_column(ctx, dtype, 9), sorted_keys_column(ctx, dtype)):
        nv = col.n_vectors
        mask = random_mask(nv, 43)
        n_sel = int(unpack_mask(mask.cpu().numpy(), xs.size).sum())
        zones = ctx.zone_map(col)
        tdt = zones.dtype
        lies = {"swapped": zones.flip(1).contiguous(), "shifted": torch.roll(zones, 5, 0).contiguous(), "a point": torch.full_like(zones, 12.5),
                "another point per vector": torch.arange(nv, dtype=tdt, device=DEV).reshape(nv, 1).repeat(1, 2).contiguous(),
                "infinite": torch.stack([torch.full((nv,), INF, dtype=tdt, device=DEV), torch.full((nv,), -INF, dtype=tdt, device=DEV)], dim=1).contiguous(),
                "NaN": torch.full_like(zones, NAN)}
        for what, z in lies.items():
            for capacity in (64, 3):
                out = Out(dtype, capacity)
                d, n_nan, n_num, overflow = out.run(ctx, col, mask=mask, zones=z)  # (returns, and the guards are checked)
                assert n_nan + n_num == n_sel, f"{dtype}, records {what}: the totals"


# ---- 5. cross-checks against the shipped calls ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_values_feed_histogram_and_select_in_mask(ctx, dtype):
    for col, xs in (keys_column(ctx, dtype, 9), sorted_keys_column(ctx, dtype), all_distinct_column(ctx, dtype)):
        nv = col.n_vectors
        mask = random_mask(nv, 51)
        first, n = 0, min(xs.size, 3000)  # (at most 3000 distinct values: a histogram takes 4095 edges)
        values, counts, n_nan, overflow = ctx.distinct(col, mask=mask, first=first, n=n)
        d = values.numel()
        assert not overflow and d > 0
        hist = ctx.histogram(col, values, mask=mask, first=first, n=n, sorted=True)
        assert torch.equal(hist[1:d + 1], counts) and int(hist[0]) == 0 and int(hist[d + 1]) == n_nan, "point buckets: bucket i + 1 counts value i"
        member = ctx.select_in_mask(col, values, first=first, n=n, sorted=True)
        sel = selection(xs.size, mask, first, n)
        want = sel & ~is_nan_bits(xs)
        got = unpack_mask((member & mask).cpu().numpy(), xs.size)
        assert np.array_equal(got, want), "x IN (the distinct values) under the bitmap is the selected values that are no NaNs"


# ---- 6. run to run, statelessness ------------------------------------------------------------------------------------------------------------------------------------
def test_the_same_call_gives_the_same_bytes(ctx):
    col, xs = all_distinct_column(ctx, "f64")
    keys, _ = keys_column(ctx, "f64", 9)
    mask = random_mask(8, 61)
    runs = []
    for rep in range(3):
        torch.empty(1 << (20 + rep), dtype=torch.uint8, device=DEV).fill_(rep)  # (a different allocation history each time)
        a, b = Out("f64", 8192), Out("f64", 100)
        a.run(ctx, col, mask=mask)
        b.run(ctx, keys, first=999, n=5000)
        runs.append(a.bytes() + b.bytes())
    assert runs[0] == runs[1] == runs[2]


def test_distinct_calls_leave_the_decode_plan_alone(ctx):
    import datagen
    for hinted in (True, False):
        col = ctx.encode(torch.from_numpy(datagen.mixed_column(150, seed=91)).to(DEV))
        if hinted:
            ctx.column_totals(col)
        ctx.decode(col)
        ctx.synchronize()
        before = ctx.decode_plan(col)
        ctx.distinct(col, capacity=1 << 18)
        ctx.distinct(col, mask=random_mask(150, 92), zones=ctx.zone_map(col), first=5, n=9999)
        ctx.synchronize()
        assert ctx.decode_plan(col) == before


# ---- 7. capture ----------------------------------------------------------------------------------------------------------------------------------------------------------
CAPTURE = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
from alp_amd import capi
from distinct_replica import host_distinct, unpack_mask
ctx = capi.Context(0)
side = torch.cuda.Stream()
ok = True
def bitmap(nv, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2**64, 16 * nv, dtype=np.uint64).view(np.int64)).cuda()
def data(seed, dt):
    rng = np.random.default_rng(seed)
    x = rng.choice((rng.permutation(5000)[:700] * 0.25 - 300).astype(dt), 40 * 1024)
    x[rng.integers(0, x.size, 50)] = np.nan
    x[rng.integers(0, x.size, 50)] = -0.0
    return x
nv = 40
a, b = [data(s, np.float64) for s in (1, 2)], [data(s, np.float32) for s in (3, 4)]
ad, bd = [torch.from_numpy(t).cuda() for t in a], [torch.from_numpy(t).cuda() for t in b]
cola, colb = ctx.encode(ad[0]), ctx.encode(bd[0])
mask = bitmap(nv, 5)
cap = 1000
va, vb = torch.zeros(cap, dtype=torch.float64, device="cuda:0"), torch.zeros(cap, dtype=torch.float32, device="cuda:0")
ca, cb = torch.zeros(cap, dtype=torch.int64, device="cuda:0"), torch.zeros(cap, dtype=torch.int64, device="cuda:0")
sa, sb = torch.zeros(4, dtype=torch.int64, device="cuda:0"), torch.zeros(4, dtype=torch.int64, device="cuda:0")
scr_a, scr_b = ctx.distinct_scratch(cap), ctx.distinct_scratch(cap)
def calls():
    ctx.distinct_into(cola, va, sa, counts_out=ca, mask=mask, first=1000, n=30 * 1024, scratch=scr_a)
    ctx.distinct_into(colb, vb, sb, counts_out=cb, mask=mask, scratch=scr_b)
with torch.cuda.stream(side):
    calls()                                                 # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        calls()
for rep in range(3):
    if rep == 1:
        ctx.encode(ad[1], cola); ctx.encode(bd[1], colb)    # other data encoded into the same buffers and another bitmap written into the same tensor
        mask.copy_(bitmap(nv, 6))
    torch.cuda.synchronize()
    for t in (va, vb, ca, cb, sa, sb):
        t.fill_(rep - 1)
    scr_a.fill_(rep); scr_b.fill_(255 - rep)
    g.replay()
    torch.cuda.synchronize()
    sel = unpack_mask(mask.cpu().numpy(), nv * 1024)
    r = np.arange(nv * 1024)
    for col, vals, cnts, state, s in ((cola, va, ca, sa, sel & (r >= 1000) & (r < 1000 + 30 * 1024)), (colb, vb, cb, sb, sel)):
        v, c, n_nan, n_num = host_distinct(ctx.decode(col).cpu().numpy(), s)
        d = v.size
        ok = ok and state.tolist() == [d, n_nan, n_num, 0] and vals[:d].cpu().numpy().tobytes() == v.tobytes() and np.array_equal(cnts[:d].cpu().numpy().view(np.uint64), c)
        ok = ok and d > 100 and n_nan > 0 and bool((vals[d:] == rep - 1).all()) and bool((cnts[d:] == rep - 1).all())
    print(rep, sa.tolist(), sb.tolist(), ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_bitmap_and_the_columns_change():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 8. several contexts -----------------------------------------------------------------------------------------------------------------------------------------------
def test_host_threads_with_one_context_each(ctx):
    cols = [keys_column(ctx, "f64", 9), all_distinct_column(ctx, "f64"), keys_column(ctx, "f32", 9), sorted_keys_column(ctx, "f32")]
    wants = [host_distinct(xs) for _, xs in cols]
    got, errors = [None] * len(cols), []

    def thread_main(i):
        try:
            own = capi.Context(0)
            with torch.cuda.stream(torch.cuda.Stream()):
                res = []
                for _ in range(3):
                    values, counts, n_nan, overflow = own.distinct(cols[i][0], capacity=8192)
                    res.append((values.cpu().numpy().tobytes(), counts.cpu().numpy().view(np.uint64).copy(), n_nan, overflow))
                got[i] = res
            own.close()
        except Exception as exc:  # noqa: BLE001 (reported below)
            errors.append((i, repr(exc)))

    torch.cuda.synchronize()
    threads = [threading.Thread(target=thread_main, args=(i,)) for i in range(len(cols))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i, res in enumerate(got):
        for values, counts, n_nan, overflow in res:
            assert values == wants[i][0].tobytes() and np.array_equal(counts, wants[i][1]) and (n_nan, overflow) == (wants[i][2], False), i


# ---- 9. argument checks ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c_argument_checks(ctx, dtype):
    col, xs = keys_column(ctx, dtype, 9)
    nv, vb = col.n_vectors, 8 if dtype == "f64" else 4
    zones = ctx.zone_map(col)
    mask = random_mask(nv, 10)
    cap = 64
    out = Out(dtype, cap)
    trace = torch.full((7,), POISON, dtype=torch.int64, device=DEV)
    scratch = torch.full((capi.lib.alpgpu_distinct_scratch_bytes(cap) + 16,), 0x5A, dtype=torch.uint8, device=DEV)
    fn, dbg = getattr(capi.lib, "alpgpu_distinct_" + dtype), getattr(capi.lib, "alpgpu_debug_distinct_" + dtype)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    c = ctypes.byref(col.c)
    V, C_, S, X, M = p(out.vals), p(out.counts), p(out.state), p(scratch), p(mask)
    assert fn(None, c, 0, 1024, M, None, cap, V, C_, S, X) == -2, "a NULL context must be refused"
    assert fn(ctx.h, None, 0, 1024, M, None, cap, V, C_, S, X) == -2, "a NULL column must be refused"
    assert fn(ctx.h, c, 0, 1024, M, None, cap, None, C_, S, X) == -2, "NULL values must be refused"
    assert fn(ctx.h, c, 0, 1024, M, None, cap, V, C_, None, X) == -2, "a NULL state must be refused"
    assert fn(ctx.h, c, 0, 1024, M, None, cap, V, C_, S, None) == -2, "a NULL scratch must be refused"
    for bad in (0, capi.DISTINCT_MAX + 1, 2**32, 2**64 - 1):
        assert fn(ctx.h, c, 0, 1024, M, None, bad, V, C_, S, X) == -2, f"capacity {bad} must be refused"
    assert fn(ctx.h, c, 0, 1024, p(mask, 4), None, cap, V, C_, S, X) == -2, "a misaligned bitmap must be refused"
    assert fn(ctx.h, c, 0, 1024, M, p(zones, vb), cap, V, C_, S, X) == -2, "misaligned zones must be refused"
    assert fn(ctx.h, c, 0, 1024, M, None, cap, p(out.vals, vb // 2), C_, S, X) == -2, "misaligned values must be refused"
    assert fn(ctx.h, c, 0, 1024, M, None, cap, V, p(out.counts, 4), S, X) == -2, "misaligned counts must be refused"
    assert fn(ctx.h, c, 0, 1024, M, None, cap, V, C_, p(out.state, 4), X) == -2, "a misaligned state must be refused"
    assert fn(ctx.h, c, 0, 1024, M, None, cap, V, C_, S, p(scratch, 8)) == -2, "a scratch that is not 16-byte aligned must be refused"
    assert dbg(ctx.h, c, 0, 1024, M, None, cap, V, C_, S, X, None, p(trace, 4)) == -2, "a misaligned trace must be refused"
    total = nv * 1024
    for first, n in ((1, total), (total - 100, 101), (total + 1, 0), (2**64 - 1, 2), (2, 2**64 - 1), (2**63, 2**63)):
        assert fn(ctx.h, c, first, n, M, None, cap, V, C_, S, X) == -2, f"range ({first}, {n}) must be refused"
    bare = capi.CColumn()
    bare.n_vectors = 1
    assert fn(ctx.h, ctypes.byref(bare), 0, 1024, None, None, cap, V, C_, S, X) == -2, "a column without descriptors must be refused"
    ctx.synchronize()
    assert out.bytes() == Out(dtype, cap).bytes() and bool((trace == POISON).all()) and bool((scratch == 0x5A).all()), "a refused call wrote"
    # n == 0 and a column of no vectors: the zero state and nothing else
    empty = capi.CColumn()
    for column, first in ((c, 777), (c, total), (ctypes.byref(empty), 0), (ctypes.byref(bare), 0)):
        out = Out(dtype, cap)
        assert fn(ctx.h, column, first, 0, None, None, cap, p(out.vals), p(out.counts), p(out.state), X) == 0
        ctx.synchronize()
        assert out.state.tolist() == [0, 0, 0, 0] and bool((out.state_raw[4:] == POISON).all())
        assert out.vals_raw.cpu().numpy().tobytes() == Out(dtype, cap).vals_raw.cpu().numpy().tobytes() and bool((out.counts_raw == POISON).all())
    assert bool((scratch == 0x5A).all()), "a call without work touches no scratch"
    assert fn(ctx.h, ctypes.byref(empty), 0, 1, None, None, cap, V, C_, S, X) == -2
    # counts may be NULL; the full call fills exactly its entries
    out = Out(dtype, cap, counts=False)
    assert fn(ctx.h, c, 0, total, M, p(zones), cap, p(out.vals), None, p(out.state), X) == 0
    ctx.synchronize()
    want = host_distinct(xs, unpack_mask(mask.cpu().numpy(), total))
    check(out, out.state.tolist(), want, "NULL counts")


def test_python_rejects_arguments_that_do_not_fit(ctx, monkeypatch):
    col, xs = keys_column(ctx, "f64", 9)
    cf, _ = keys_column(ctx, "f32", 9)
    nv = col.n_vectors
    vals = torch.zeros(64, dtype=torch.float64, device=DEV)
    counts = torch.zeros(64, dtype=torch.int64, device=DEV)
    state = torch.full((4,), 7, dtype=torch.int64, device=DEV)
    mask = random_mask(nv, 3)
    zones = ctx.zone_map(col)

    def unreachable(*a, **k):
        raise AssertionError("the library was called")
    for t in ("f64", "f32"):
        monkeypatch.setattr(capi.lib, "alpgpu_distinct_" + t, unreachable)
        monkeypatch.setattr(capi.lib, "alpgpu_debug_distinct_" + t, unreachable)
    for bad in (vals.to(torch.float32), vals.cpu(), vals[:0], vals.reshape(8, 8), torch.zeros(128, dtype=torch.float64, device=DEV)[::2], [0.0] * 64):
        with pytest.raises(ValueError):
            ctx.distinct_into(col, bad, state)
    with pytest.raises(ValueError):
        ctx.distinct_into(cf, vals, state)  # a float column takes float values
    for bad in (state.to(torch.int32), state.cpu(), torch.zeros(5, dtype=torch.int64, device=DEV), [0] * 4):
        with pytest.raises(ValueError):
            ctx.distinct_into(col, vals, bad)
    for bad in (counts.to(torch.int32), counts.cpu(), counts[:-1]):
        with pytest.raises(ValueError):
            ctx.distinct_into(col, vals, state, counts_out=bad)
    for bad in (mask.to(torch.int32), mask.cpu(), mask[:-16], mask.reshape(nv, 16)):
        with pytest.raises(ValueError):
            ctx.distinct_into(col, vals, state, mask=bad)
    for bad in (zones.to(torch.float32), zones.cpu(), zones[:-1], zones.reshape(-1)):
        with pytest.raises(ValueError):
            ctx.distinct_into(col, vals, state, zones=bad)
    for kw in ({"first": -1}, {"n": -1}, {"tuning": {"grid": 1, "capacity": 5}}, {"trace": torch.zeros(4, dtype=torch.int64, device=DEV)},
               {"scratch": torch.zeros(100, dtype=torch.uint8, device=DEV)}):
        with pytest.raises(ValueError):
            ctx.distinct_into(col, vals, state, **kw)
    for bad in (0, capi.DISTINCT_MAX + 1):
        with pytest.raises(ValueError):
            ctx.distinct(col, capacity=bad)
        with pytest.raises(ValueError):
            ctx.distinct_scratch(bad)
    ctx.synchronize()
    assert bool((state == 7).all()), "a refused call launched"


# ---- 10. the C++ wrapper ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cpp_column_distinct_against_decompress_and_a_host_map(ctx, tmp_path, dtype):
    """include/alp/batch.hpp: alp::gpu::column<double / float>::distinct of a serialized column against column::decompress and an ordered map on the host
    (tests/cpp/distinct_test.cpp)"""
    exe = tmp_path / "distinct_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/distinct_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])

    def make():  # the keys with their zeros, infinities and NaNs, then a few hundred more values, then sorted keys: constant vectors
        rng = np.random.default_rng(77)
        dt = np_dtype(dtype)
        head = rng.choice(np.array(KEYS16, dt), 3 * 1024)
        head[rng.integers(0, head.size, 20)] = NAN
        body = rng.choice((np.arange(700) * 0.5 - 100).astype(dt), 3 * 1024)
        tail = np.sort(rng.choice(np.array([1.5, 2.5, 9.75], dt), 4 * 1024))
        return np.concatenate([head, body, tail])
    col, xs = encoded(ctx, ("cpp", dtype), make)
    ctx.to_blob(col, xs.size).tofile(str(tmp_path / "col.blob"))
    mask = vectors_cleared(random_mask(col.n_vectors, 53), 3)
    mask.cpu().numpy().tofile(str(tmp_path / "in.mask"))
    p = subprocess.run([str(exe), dtype] + [str(tmp_path / f) for f in ("col.blob", "in.mask")], capture_output=True, text=True, timeout=600)
    line = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("ok ")]
    assert p.returncode == 0 and len(line) == 1, p.stdout[-3000:] + p.stderr[-2000:]
    want = host_distinct(xs, unpack_mask(mask.cpu().numpy(), xs.size))
    assert int(line[0][1]) == col.n_vectors and int(line[0][2]) == want[0].size > 300
