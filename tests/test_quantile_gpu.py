"""GPU: the quantiles (include/alpgpu.h, "quantiles": alpgpu_select_rank_*, alpgpu_quantile_*).  The expected result never comes from the code under
test: x = ctx.decode(col) on the host (pinned to the oracle and the reference by other suites) or the oracle's decode of a hand-built encoding, and
tests/quantile_replica.py, the definition by numpy on integer views.  Values compare as integers.  Every call goes through `run_rank` / `run_q`, which
put canaries behind both outputs and behind alpgpu_quantile_scratch_bytes of scratch and check that none of them changed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import datagen
from alp_amd import capi
from quantile_replica import host_quantile, host_select_rank, okey, sorted_selection, unpack_mask
from test_in_list_gpu import COLUMNS, column, random_mask, vectors_cleared

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF, NAN = float("inf"), float("nan")
CANARY = 0xA5


def ints(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def run_rank(ctx, col, mask, ranks, from_top=False, zones=None, tuning=None, trace=False):
    """select_rank_into with canaries: (values as integers, none for N == 0; N[; the trace])"""
    tdt = torch.float64 if col.dtype == "f64" else torch.float32
    k = len(ranks)
    vals = torch.full((k + 8,), 7.0, dtype=tdt, device=DEV)
    count = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    need = capi.lib.alpgpu_quantile_scratch_bytes(col.n_vectors)
    scratch = torch.full((need + 256,), CANARY, dtype=torch.uint8, device=DEV)
    ctx.select_rank_into(col, mask, ranks, vals, count, from_top=from_top, zones=zones, scratch=scratch, tuning=tuning)
    n = int(count[0].item())
    assert n >= 0 and int(count[1].item()) == -7
    assert bool((scratch[need:] == CANARY).all()), "the call wrote behind alpgpu_quantile_scratch_bytes"
    assert bool((vals[k if n else 0:] == 7.0).all()), "values were written behind the ranks (or, with N == 0, at all)"
    out = ints(vals[:k if n else 0])
    return (out, n, ctx.quantile_trace(scratch)) if trace else (out, n)


def run_q(ctx, col, mask, q, zones=None, with_ranks=True):
    """quantile_into with canaries: (the neighbour pairs as integers [len(q), 2], the ranks, N); nothing for N == 0"""
    tdt = torch.float64 if col.dtype == "f64" else torch.float32
    k = len(q)
    vals = torch.full((2 * k + 8,), 7.0, dtype=tdt, device=DEV)
    ranks = torch.full((k + 8,), -7, dtype=torch.int64, device=DEV)
    count = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    need = capi.lib.alpgpu_quantile_scratch_bytes(col.n_vectors)
    scratch = torch.full((need + 256,), CANARY, dtype=torch.uint8, device=DEV)
    ctx.quantile_into(col, mask, q, vals, count, ranks if with_ranks else None, zones=zones, scratch=scratch)
    n = int(count[0].item())
    assert n >= 0 and int(count[1].item()) == -7
    assert bool((scratch[need:] == CANARY).all()), "the call wrote behind alpgpu_quantile_scratch_bytes"
    assert bool((vals[2 * k if n else 0:] == 7.0).all()), "values were written behind the quantiles (or, with N == 0, at all)"
    assert bool((ranks[k if n and with_ranks else 0:] == -7).all()), "ranks were written where none belong"
    return ints(vals[:2 * k if n else 0]).reshape(-1, 2), ranks[:k if n else 0].cpu().numpy(), n


def check_rank(ctx, col, s, mask, ranks, what, from_top=False, zones=None, tuning=None, trace=False):
    want_v, want_n = host_select_rank(s, ranks, from_top)
    got = run_rank(ctx, col, mask, ranks, from_top, zones, tuning, trace)
    assert got[1] == want_n, f"{what}: N {got[1]}, expected {want_n}"
    assert np.array_equal(got[0], ints(want_v)), f"{what}: values differ at {np.nonzero(got[0] != ints(want_v))[0][:4]}"
    return got


def check_q(ctx, col, s, mask, q, what, zones=None, with_ranks=True):
    want_p, want_r, want_n = host_quantile(s, q)
    got_p, got_r, got_n = run_q(ctx, col, mask, q, zones, with_ranks)
    assert got_n == want_n, f"{what}: N {got_n}, expected {want_n}"
    assert np.array_equal(got_p, ints(want_p).reshape(-1, 2)), f"{what}: neighbours differ"
    if with_ranks:
        assert np.array_equal(got_r, want_r), f"{what}: ranks differ"
    return got_p, got_r, got_n


def encode(ctx, x):
    """(DeviceColumn, its decode on the host) of whole vectors of values"""
    x = np.ascontiguousarray(x)
    assert x.size % 1024 == 0
    it = torch.int64 if x.dtype == np.float64 else torch.int32
    xd = torch.from_numpy(x).to(DEV)
    col = ctx.encode(xd)
    assert torch.equal(ctx.decode(col).view(it), xd.view(it))
    return col, x


def full_mask(nv):
    return torch.full((16 * nv,), -1, dtype=torch.int64, device=DEV)


def one_bit(nv, r):
    m = torch.zeros(16 * nv, dtype=torch.int64, device=DEV)
    m[r >> 6] = 1 << (r & 63) if (r & 63) < 63 else -(1 << 63)
    return m


def spread(n, k=32):
    """k ranks spread over [0, n)"""
    return [int(i) for i in np.linspace(0, max(n - 1, 0), k).astype(np.int64)]


def from_keys(keys, dtype):
    """values of this type from their okeys (the inverse of okey)"""
    u = np.uint64 if dtype == np.float64 else np.uint32
    keys = np.asarray(keys, dtype=u)
    sign = u(1) << u(8 * keys.dtype.itemsize - 1)
    return np.where(keys & sign != 0, keys ^ sign, ~keys).astype(u).view(dtype)


def key_of(v, dtype):
    return int(okey(np.array([v], dtype=dtype))[0])


# ---- 1. every column kind against the replica ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_every_column_kind_against_the_host_replica(ctx, name):
    col, _, xs, _ = column(ctx, name)
    nv = col.n_vectors
    rnd = random_mask(nv, 71)
    masks = {"full": full_mask(nv), "random": rnd, "cleared": vectors_cleared(rnd, 7, 0), "one bit": one_bit(nv, 1024 * (nv // 2) + 321),
             "zero": torch.zeros(16 * nv, dtype=torch.int64, device=DEV)}
    rng = np.random.default_rng(72)
    for mname, mask in masks.items():
        s = sorted_selection(xs, unpack_mask(mask.cpu().numpy()))
        n = s.size
        what = f"{name}, {mname} bitmap"
        sp = spread(n)
        shuffled = [sp[i] for i in rng.permutation(32)][:24] + sp[:8]  # any order, with repeats
        for ranks in ([0], [max(n - 1, 0)], [n // 2], sp, shuffled, [n, n + 1, 2**40, 2**64 - 1, 0]):
            check_rank(ctx, col, s, mask, ranks, f"{what}, ranks {ranks[:4]}")
        check_rank(ctx, col, s, mask, sp, what + ", from the top", from_top=True)
        check_rank(ctx, col, s, mask, [0, 1, n + 5], what + ", from the top", from_top=True)
        desc = sorted(rng.random(12).tolist() + [0.5, 0.5, 1.0, 0.0], reverse=True)  # 16 values with repeats, descending
        for q in ([0.0, 0.5, 1.0], [0.25, 0.5, 0.75], desc):
            check_q(ctx, col, s, mask, q, f"{what}, q {q[:3]}")
        check_q(ctx, col, s, mask, [0.5, 0.9], what + ", no ranks", with_ranks=False)
        if mname == "zero":
            assert n == 0
        if mname == "one bit":
            assert n == (0 if np.isnan(xs[1024 * (nv // 2) + 321]) else 1)
    assert not np.isnan(xs).all()


# ---- 2. small shapes ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_one_vector_and_a_ragged_last_workgroup(ctx, dtype):
    gen = datagen.mixed_column if dtype == "f64" else datagen.mixed_column_f32
    for nv in (1, 5):
        col, xs = encode(ctx, gen(nv, seed=73 + nv))
        for mask in (full_mask(nv), random_mask(nv, 74)):
            s = sorted_selection(xs, unpack_mask(mask.cpu().numpy()))
            check_rank(ctx, col, s, mask, spread(s.size), f"{dtype}, {nv} vectors")
            check_rank(ctx, col, s, mask, [0, s.size - 1, s.size // 2], f"{dtype}, {nv} vectors, from the top", from_top=True)
            check_q(ctx, col, s, mask, [0.0, 0.01, 0.5, 0.99, 1.0], f"{dtype}, {nv} vectors")


# ---- 3. every path, by the debug entry ------------------------------------------------------------------------------------------------------------------
def staircase(dtype, nv=19):
    """Bit patterns chosen so that the number of values that still match a rank's prefix after pass d is known.  Around A = 1.5: 935 values that leave
    at byte 1, then (double) 1, 1, 61, 1 at bytes 2 .. 5, (float) 1 and 63 at bytes 2 and 3: with A itself 1000, 65, 64, 63, 2, 1 (double) or 1000, 65, 64
    (float) match after passes 0, 1, 2 ...  B: 70 equal values.  C: one value and two that leave at the last byte but one.  The rest is decimal fill
    with other top bytes.  Returns (values, {name: key})"""
    vb = 8 if dtype == np.float64 else 4
    a, b, c = key_of(1.5, dtype), key_of(1.5 * 2.0**20, dtype), key_of(1.5 * 2.0**-40, dtype)
    leave = {1: 935, 2: 1, 3: 1, 4: 61, 5: 1} if vb == 8 else {1: 935, 2: 1, 3: 63}
    keys = [a] + [a ^ (1 << (8 * (vb - 1 - j))) for j, n in leave.items() for _ in range(n)] + [b] * 70 + [c, c ^ (1 << 8), c ^ (1 << 8)]
    special = from_keys(keys, dtype)
    assert not np.isnan(special).any()
    rng = np.random.default_rng(75)
    x = -np.round(rng.uniform(1.0, 1000.0, nv * 1024), 2).astype(dtype)  # negative: no top byte of A, B or C
    x[rng.permutation(x.size)[:special.size]] = special
    return x, {"A": a, "B": b, "C": c}


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_path_by_the_debug_entry_gives_the_default_calls_bytes(ctx, dtype):
    vb = 8 if dtype == np.float64 else 4
    x, keys = staircase(dtype)
    col, xs = encode(ctx, x)
    nv = col.n_vectors
    mask = full_mask(nv)
    s = sorted_selection(xs, np.ones(xs.size, bool))
    sk = okey(s)
    rank_of = {k: int(np.searchsorted(sk, v)) for k, v in keys.items()}
    queries = {"A": [rank_of["A"]], "B": [rank_of["B"] + 35], "C": [rank_of["C"]], "many": spread(s.size)}
    default = {k: check_rank(ctx, col, s, mask, r, f"default, {k}", trace=True) for k, r in queries.items()}
    assert all(d[2]["compact_pass"] == 0 and d[2]["candidates"] == s.size for d in default.values())  # every value fits the default capacity
    stairs = {1000: 1, 65: 2, 64: 3, **({63: 4, 2: 5, 1: 6} if vb == 8 else {})}
    compacted, trips, exact = set(), set(), False
    for cap in (1, 2, 63, 64, 65, 1000, s.size, 0):
        for wgs in (1, 2, 3, 0):
            for flush in (1, 3, 0):
                for k, r in queries.items():
                    if k in ("B", "C") and (wgs, flush) != (0, 0):
                        continue  # (their paths differ from A's in the capacity alone)
                    tuning = {"capacity": cap, "max_workgroups": wgs, "flush_every": flush}
                    got_v, got_n, tr = run_rank(ctx, col, mask, r, tuning=tuning, trace=True)
                    assert got_n == default[k][1] and np.array_equal(got_v, default[k][0]), f"{k} under {tuning}"
                    assert tr["n"] == s.size and tr["waves_per_wg"] == 8 and tr["wide_grid"] == (min(wgs, 3) if wgs else 3)
                    compacted.add(tr["compact_pass"])
                    trips.add(-(-nv // (tr["wide_grid"] * tr["waves_per_wg"])))
                    if tr["compact_pass"] < vb:
                        assert tr["candidates"] <= (cap or 65536)
                        exact = exact or (cap != 0 and tr["candidates"] == cap)
                    if k == "A" and cap in stairs:  # the staircase: exactly `cap` values match A's prefix after pass stairs[cap] - 1
                        assert tr["compact_pass"] == stairs[cap] and tr["candidates"] == cap, (tuning, tr)
    # the closing guard: every pass compacted once, "never" occurred, a workgroup made more than one trip, a candidate count met its capacity exactly
    assert compacted == set(range(vb + 1)), compacted
    assert max(trips) > 1 and min(trips) == 1, trips
    assert exact


# ---- 4. digits ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_byte_of_the_key_decides_a_rank(ctx, dtype):
    vb = 8 if dtype == np.float64 else 4
    base = key_of(-123.456, dtype)
    rng = np.random.default_rng(76)
    for p in range(vb):
        keys = np.where(rng.random(3 * 1024) < 0.5, base, base ^ (1 << (8 * p)))
        x = from_keys(keys, dtype)
        assert not np.isnan(x).any() and np.unique(x).size == 2
        col, xs = encode(ctx, x)
        mask = random_mask(3, 77 + p)
        s = sorted_selection(xs, unpack_mask(mask.cpu().numpy()))
        lower = int((okey(s) == okey(s)[0]).sum())  # the values of the lower group
        assert 0 < lower < s.size
        got, _ = check_rank(ctx, col, s, mask, [lower - 1, lower, 0, s.size - 1], f"byte {p}")
        assert got[0] != got[1] and got[0] == got[2] and got[1] == got[3]
        # the two groups part in pass VB - 1 - p; with one candidate allowed every pass is a decode pass (either group holds more than one value)
        got1, _, tr = run_rank(ctx, col, mask, [lower - 1, lower, 0, s.size - 1], tuning={"capacity": 1}, trace=True)
        assert tr["compact_pass"] == vb and np.array_equal(got1, got)
    # values that differ only in the sign
    x = np.where(rng.random(2 * 1024) < 0.5, dtype(17.25), dtype(-17.25)).astype(dtype)
    col, xs = encode(ctx, x)
    s = sorted_selection(xs, np.ones(xs.size, bool))
    neg = int((xs < 0).sum())
    got, _ = check_rank(ctx, col, s, full_mask(2), [neg - 1, neg], "sign")
    assert got[0] < 0 <= got[1]
    # 33 distinct values with distinct top bytes and 32 ranks, one on each of the first 32: 32 live slots
    step = 16 if vb == 8 else 2
    vals33 = np.array([2.0 ** (step * (k - 16)) for k in range(33)], dtype=dtype)
    assert np.unique(okey(vals33) >> (8 * (vb - 1))).size == 33
    x = vals33[rng.integers(0, 33, 3 * 1024)]
    col, xs = encode(ctx, x)
    s = sorted_selection(xs, np.ones(xs.size, bool))
    starts = np.searchsorted(okey(s), okey(vals33))
    ranks = [int(starts[k]) for k in range(32)]
    got, _, tr = check_rank(ctx, col, s, full_mask(3), ranks, "32 live slots", tuning={"capacity": 1}, trace=True)
    assert np.unique(got).size == 32 and tr["compact_pass"] == vb


# ---- 5. ties and special values -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ties_zeros_infinities_and_nans(ctx, dtype):
    vb = 8 if dtype == np.float64 else 4
    # a constant column with a capacity below N: all VB passes wide, every add wave-uniform
    col, xs = encode(ctx, np.full(40 * 1024, 3.5, dtype=dtype))
    s = sorted_selection(xs, np.ones(xs.size, bool))
    got, n, tr = check_rank(ctx, col, s, full_mask(40), [0, 12345, 40 * 1024 - 1, 2**50], "constant column", tuning={"capacity": 1000}, trace=True)
    assert n == 40 * 1024 and tr["compact_pass"] == vb and tr["candidates"] == 0
    check_q(ctx, col, s, full_mask(40), [0.0, 0.5, 1.0], "constant column")
    # two values
    x = np.full(6 * 1024, 1.25, dtype=dtype)
    x[::3] = 2.5
    col, xs = encode(ctx, x)
    s = sorted_selection(xs, np.ones(xs.size, bool))
    lows = int((xs == 1.25).sum())
    check_rank(ctx, col, s, full_mask(6), [0, lows - 1, lows, xs.size - 1], "two values")
    check_rank(ctx, col, s, full_mask(6), [0, lows - 1, lows, xs.size - 1], "two values, capacity 100", tuning={"capacity": 100})
    # +0.0 / -0.0 alternating: the ranks N/2 - 1 and N/2 keep their signs
    z = np.zeros(3 * 1024, dtype=dtype)
    z[1::2] = -0.0
    col, xs = encode(ctx, z)
    s = sorted_selection(xs, np.ones(xs.size, bool))
    got, n = check_rank(ctx, col, s, full_mask(3), [3 * 512 - 1, 3 * 512], "alternating zeros")
    assert got[0] < 0 and got[1] == 0  # as integers: -0.0 has the sign bit, +0.0 is 0
    got_p, _, _ = check_q(ctx, col, s, full_mask(3), [0.5], "alternating zeros")
    assert got_p[0, 0] < 0 and got_p[0, 1] == 0
    # +-inf among ordinary values, NaN exceptions (quiet and signalling) that a selection skips
    rng = np.random.default_rng(78)
    x = np.round(rng.normal(0, 1000, 6 * 1024), 2).astype(dtype)
    u = np.uint64 if dtype == np.float64 else np.uint32
    snan = np.array([0x7FF0000000000001 if dtype == np.float64 else 0x7F800001], dtype=u).view(dtype)[0]
    x[[7, 1500, 4000]] = INF
    x[[8, 2500]] = -INF
    x[[9, 100, 1024, 5000]] = NAN
    x[[10, 3000]] = snan
    col, xs = encode(ctx, x)
    s = sorted_selection(xs, np.ones(xs.size, bool))
    got, n = check_rank(ctx, col, s, full_mask(6), [0, 1, 2, s.size - 4, s.size - 3, s.size - 1], "infinities and NaNs")
    assert n == 6 * 1024 - 6 and np.isinf(s[[0, 1, -3, -1]]).all() and not np.isinf(s[[2, -4]]).any()
    check_q(ctx, col, s, full_mask(6), [0.0, 0.0001, 0.5, 0.9999, 1.0], "infinities and NaNs")
    # a selection of NaNs alone: count 0 and nothing else; NaNs and two numbers
    mask = torch.zeros(16 * 6, dtype=torch.int64, device=DEV)
    for r in (9, 10, 100, 1024, 3000, 5000):
        mask[r >> 6] |= one_bit(1, r & 63)[0]
    s = sorted_selection(xs, unpack_mask(mask.cpu().numpy()))
    assert check_rank(ctx, col, s, mask, [0, 5], "NaNs alone")[1] == 0
    assert check_q(ctx, col, s, mask, [0.5], "NaNs alone")[2] == 0
    for r in (11, 4001):
        mask[r >> 6] |= one_bit(1, r & 63)[0]
    s = sorted_selection(xs, unpack_mask(mask.cpu().numpy()))
    assert check_rank(ctx, col, s, mask, [0, 1, 2], "NaNs and two numbers")[1] == 2
    assert check_q(ctx, col, s, mask, [0.0, 0.5, 1.0], "NaNs and two numbers")[2] == 2


# ---- 6. zones -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "adversarial", "rd_unit_f32", "adversarial_f32"])
def test_zones_that_contain_the_truth_change_no_byte(ctx, name):
    col, _, xs, _ = column(ctx, name)
    nv = col.n_vectors
    tdt = torch.float64 if col.dtype == "f64" else torch.float32
    rnd = vectors_cleared(random_mask(nv, 79), 2, 0)
    s = sorted_selection(xs, unpack_mask(rnd.cpu().numpy()))
    ranks = spread(s.size)
    q = [0.1, 0.5, 0.9]
    anything = torch.tensor([[-INF, INF]], dtype=tdt, device=DEV).repeat(nv, 1).contiguous()
    with_nan = ctx.decode_minmax_masked(col, rnd).clone()
    with_nan[::2, 0] = NAN
    with_nan[1::4, 1] = NAN
    for tuning in (None, {"capacity": 500}):  # (with the default capacity these columns compact in the first pass, which no record prunes)
        want = check_rank(ctx, col, s, rnd, ranks, f"{name}, no zones", tuning=tuning)
        for zname, zones in (("decode_minmax_masked", ctx.decode_minmax_masked(col, rnd)), ("zone_map (widened)", ctx.zone_map(col)), ("-inf .. +inf", anything), ("NaN bounds", with_nan)):
            got = run_rank(ctx, col, rnd, ranks, zones=zones, tuning=tuning, trace=True)
            assert got[1] == want[1] and np.array_equal(got[0], want[0]), f"{name}: {zname}, {tuning}"
            if zname == "-inf .. +inf":
                assert sum(got[2]["zone_skips"]) == 0
    check_q(ctx, col, s, rnd, q, f"{name}, zone_map", zones=ctx.zone_map(col))
    # a record with a NaN bound skips nothing
    all_nan = torch.full((nv, 2), NAN, dtype=tdt, device=DEV)
    _, _, tr = run_rank(ctx, col, rnd, ranks, zones=all_nan, tuning={"capacity": 500}, trace=True)
    assert sum(tr["zone_skips"]) == 0
    # records that say "empty" everywhere: the call returns, the canaries are intact (run_rank checks them); the values are unspecified
    nothing = torch.tensor([[INF, -INF]], dtype=tdt, device=DEV).repeat(nv, 1).contiguous()
    for tuning in (None, {"capacity": 500}):
        _, n = run_rank(ctx, col, rnd, ranks, zones=nothing, tuning=tuning)
        assert n == s.size  # (the first pass reads no record)
        run_q(ctx, col, rnd, q, zones=nothing)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_sorted_column_is_skipped_by_its_zone_map_in_every_pass_but_the_first(ctx, dtype):
    vb = 8 if dtype == np.float64 else 4
    nv = 300
    # sorted over 60 decades and both signs, so that the vectors differ in every byte of the key; every value twice: a capacity of 1 never compacts
    pos = 10.0 ** np.linspace(-30.0, 30.0, nv * 256)
    x = np.repeat(np.concatenate([-pos[::-1], pos]), 2).astype(dtype)
    assert np.unique(x).size == nv * 512 and (np.diff(x) >= 0).all()
    col, xs = encode(ctx, x)
    s = sorted_selection(xs, np.ones(xs.size, bool))
    mask = full_mask(nv)
    zones = ctx.zone_map(col)
    ranks = [s.size // 2, s.size // 3, 5]
    want = check_rank(ctx, col, s, mask, ranks, "sorted, no zones")
    got_v, got_n, tr = run_rank(ctx, col, mask, ranks, zones=zones, tuning={"capacity": 1}, trace=True)
    assert got_n == want[1] and np.array_equal(got_v, want[0])
    assert tr["compact_pass"] == vb and tr["zone_skips"][0] == 0 and all(k > 0 for k in tr["zone_skips"][1:vb]), tr
    assert tr["zone_skips"][vb - 1] >= nv - 2 * len(ranks) and tr["zero_skips"] == 0
    # vectors without a set bit are counted as such
    _, _, tr = run_rank(ctx, col, vectors_cleared(mask, 3, 0), ranks, trace=True)
    assert tr["zero_skips"] == nv - (nv + 2) // 3


# ---- 7. every width of the register decode --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["f64", "f32"])
def built(ctx, request):
    import test_register_decode_rows_gpu as rows
    return rows.Columns(ctx, request.param)


def test_every_width_cut_and_exception_class_holds_a_selected_number(ctx, built):
    """the hand-built columns of tests/test_register_decode_rows_gpu.py under its random bitmap, 32 spread ranks, with the default capacity and with one
    that keeps every pass wide"""
    rnd, rnd_bits = built.masks["random"], built.mask_bits["random"]
    for name, b in (("A", built.A), ("B", built.B)):
        s = sorted_selection(b.want, rnd_bits)
        for tuning in (None, {"capacity": 1}):
            check_rank(ctx, b.col, s, rnd, spread(s.size), f"{built.dtype} {name}, {tuning}", tuning=tuning)
        check_q(ctx, b.col, s, rnd, [0.0, 0.1, 0.5, 0.9, 1.0], f"{built.dtype} {name}")
        with np.errstate(invalid="ignore"):
            kept = (rnd_bits.reshape(built.nv, 1024) & ~np.isnan(b.values)).any(axis=1)
        e = b.enc
        assert sorted(set(e["bw"][b.alp & kept].tolist())) == list(range(built.value_bits + 1))
        assert sorted(set(zip(e["bw"][~b.alp & kept].tolist(), e["lbw"][~b.alp & kept].tolist()))) == sorted(built.rows.rd_cuts())
        assert sorted(set(e["exc_cnt"][b.alp & kept].tolist())) == sorted(built.rows.ALP_EXC_COUNTS)


# ---- 8. longer than one trip of the default grid ----------------------------------------------------------------------------------------------------------
def test_a_float_column_longer_than_one_trip_of_the_default_grid(ctx):
    nv = 8200
    col, xs = encode(ctx, datagen.mixed_column_f32(nv, seed=80))
    mask = random_mask(nv, 81)
    s = sorted_selection(xs, unpack_mask(mask.cpu().numpy()))
    _, _, tr = check_rank(ctx, col, s, mask, spread(s.size), "long float column", trace=True)
    assert nv > tr["wide_grid"] * tr["waves_per_wg"], "the column no longer exceeds one trip of the default grid: lengthen it"
    check_q(ctx, col, s, mask, [0.5], "long float column")


# ---- 9. determinism and statelessness -------------------------------------------------------------------------------------------------------------------
def test_the_same_call_gives_the_same_bytes(ctx):
    col, _, xs, _ = column(ctx, "mixed")
    mask = random_mask(col.n_vectors, 82)
    n = int(unpack_mask(mask.cpu().numpy()).sum())
    runs = []
    for rep in range(2):
        torch.empty(1 << (20 + rep), dtype=torch.uint8, device=DEV).fill_(rep)  # (a different allocation history each time)
        runs.append(tuple(a.tobytes() for t in (None, {"capacity": 300}) for a in (run_rank(ctx, col, mask, spread(n), tuning=t)[0], run_q(ctx, col, mask, [0.3, 0.5])[0])))
    assert runs[0] == runs[1]


def test_quantiles_leave_the_decode_plan_alone(ctx):
    cols = [ctx.encode(torch.from_numpy(datagen.mixed_column(150, seed=s)).to(DEV)) for s in (96, 97)]
    ctx.column_totals(cols[0])  # one hinted, one not
    for col in cols:
        ctx.decode(col)
    ctx.synchronize()  # (what an unhinted decode learns about the column is in by now)
    before = [ctx.decode_plan(col) for col in cols]
    mask = random_mask(150, 52)
    for col in cols:
        ctx.select_rank(col, mask, [5, 50000])
        ctx.quantile(col, mask, [0.5], zones=ctx.zone_map(col))
    ctx.synchronize()
    assert [ctx.decode_plan(col) for col in cols] == before


CAPTURE = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
import datagen
from alp_amd import capi
from quantile_replica import host_quantile, host_select_rank, sorted_selection, unpack_mask
ctx = capi.Context(0)
side = torch.cuda.Stream()
ok = True
nv = 230
x = datagen.mixed_column(nv, seed=81)
col = ctx.encode(torch.from_numpy(x).cuda())
prior = torch.from_numpy(np.random.default_rng(85).integers(0, 2**64, 16 * nv, dtype=np.uint64).view(np.int64)).cuda()
mask = torch.zeros(16 * nv, dtype=torch.int64, device="cuda:0")
ranks = [100000, 3, 50000]
q = [0.5, 0.01]
rv = torch.zeros(3, dtype=torch.float64, device="cuda:0")
qv = torch.zeros(4, dtype=torch.float64, device="cuda:0")
qr = torch.zeros(2, dtype=torch.int64, device="cuda:0")
count = torch.zeros(2, dtype=torch.int64, device="cuda:0")
scratch = ctx.quantile_scratch(col)
def calls():
    ctx.select_rank_into(col, mask, ranks, rv, count[0:1], scratch=scratch)   # everything on the one stream: the graph is a chain
    ctx.quantile_into(col, mask, q, qv, count[1:2], qr, scratch=scratch)
with torch.cuda.stream(side):
    mask.copy_(prior)
    calls()          # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        calls()
ranks[0], q[0] = 0, 1.0   # the host arrays travelled as kernel arguments: the graph keeps what they held
for rep in range(2):
    if rep == 1:
        prior = ~prior
        prior[16 * 5:16 * 9] = 0
    torch.cuda.synchronize()
    mask.copy_(prior); rv.fill_(7.0); qv.fill_(7.0); qr.fill_(-7); count.fill_(-7); scratch.fill_(rep)
    g.replay()
    torch.cuda.synchronize()
    s = sorted_selection(x, unpack_mask(prior.cpu().numpy()))
    want_v, n = host_select_rank(s, [100000, 3, 50000])
    want_p, want_r, _ = host_quantile(s, [0.5, 0.01])
    ok = ok and torch.equal(mask, prior) and count.tolist() == [n, n]
    ok = ok and np.array_equal(rv.cpu().numpy().view(np.int64), want_v.view(np.int64)) and np.array_equal(qv.cpu().numpy().view(np.int64), want_p.reshape(-1).view(np.int64))
    ok = ok and np.array_equal(qr.cpu().numpy(), want_r)
    print(rep, n, want_r.tolist(), ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_bitmap_changes():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 10. argument checks --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c_argument_checks(ctx, dtype):
    col, _, xs, _ = column(ctx, "mixed" if dtype == "f64" else "mixed_f32")
    nv = col.n_vectors
    sr = getattr(capi.lib, "alpgpu_select_rank_" + dtype)
    qt = getattr(capi.lib, "alpgpu_quantile_" + dtype)
    dbg = getattr(capi.lib, "alpgpu_debug_quantile_" + dtype)
    tdt = torch.float32 if dtype == "f32" else torch.float64
    mask = torch.full((16 * nv + 16,), -1, dtype=torch.int64, device=DEV)
    vals = torch.full((80,), 7.0, dtype=tdt, device=DEV)
    out_r = torch.full((40,), -7, dtype=torch.int64, device=DEV)
    count = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    zones = torch.full((nv + 1, 2), 7.0, dtype=tdt, device=DEV)
    scratch = torch.full((capi.lib.alpgpu_quantile_scratch_bytes(nv) + 64,), CANARY, dtype=torch.uint8, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    V, M, Z, X, R, N, S = ctypes.byref(col.c), p(mask), p(zones), p(vals), p(out_r), p(count), p(scratch)
    ranks = (ctypes.c_uint64 * 33)(*range(33))
    q = (ctypes.c_double * 17)(*([0.5] * 17))
    bad_q = [(ctypes.c_double * 2)(0.5, v) for v in (-0.001, 1.0000001, NAN, INF, -INF)]
    bare = capi.CColumn()
    bare.n_vectors = nv  # a column without descriptors
    huge = capi.CColumn()
    huge.n_vectors = 2**32
    rec = 16 if dtype == "f64" else 8
    refused = [
        sr(None, V, M, Z, ranks, 4, 0, X, N, S), sr(ctx.h, None, M, Z, ranks, 4, 0, X, N, S), sr(ctx.h, V, None, Z, ranks, 4, 0, X, N, S), sr(ctx.h, V, M, Z, None, 4, 0, X, N, S),
        sr(ctx.h, V, M, Z, ranks, 4, 0, None, N, S), sr(ctx.h, V, M, Z, ranks, 4, 0, X, None, S), sr(ctx.h, V, M, Z, ranks, 4, 0, X, N, None),
        sr(ctx.h, V, M, Z, ranks, 0, 0, X, N, S), sr(ctx.h, V, M, Z, ranks, 33, 0, X, N, S), sr(ctx.h, V, M, Z, ranks, 2**32 - 1, 0, X, N, S),
        sr(ctx.h, V, M, p(zones, rec // 2), ranks, 4, 0, X, N, S), sr(ctx.h, V, M, Z, ranks, 4, 0, X, N, p(scratch, 8)), sr(ctx.h, V, p(mask, 4), Z, ranks, 4, 0, X, N, S),
        sr(ctx.h, V, M, Z, ranks, 4, 0, p(vals, rec // 4), N, S), sr(ctx.h, V, M, Z, ranks, 4, 0, X, p(count, 4), S),
        sr(ctx.h, ctypes.byref(bare), M, Z, ranks, 4, 0, X, N, S), sr(ctx.h, ctypes.byref(huge), M, Z, ranks, 4, 0, X, N, S),
        qt(None, V, M, Z, q, 4, X, R, N, S), qt(ctx.h, None, M, Z, q, 4, X, R, N, S), qt(ctx.h, V, None, Z, q, 4, X, R, N, S), qt(ctx.h, V, M, Z, None, 4, X, R, N, S),
        qt(ctx.h, V, M, Z, q, 4, None, R, N, S), qt(ctx.h, V, M, Z, q, 4, X, R, None, S), qt(ctx.h, V, M, Z, q, 4, X, R, N, None),
        qt(ctx.h, V, M, Z, q, 0, X, R, N, S), qt(ctx.h, V, M, Z, q, 17, X, R, N, S), qt(ctx.h, V, M, Z, q, 4, X, p(out_r, 4), N, S),
        qt(ctx.h, V, M, Z, q, 4, X, R, N, p(scratch, 4)), qt(ctx.h, ctypes.byref(bare), M, Z, q, 4, X, R, N, S), qt(ctx.h, ctypes.byref(huge), M, Z, q, 4, X, R, N, S),
        *[qt(ctx.h, V, M, Z, b, 2, X, R, N, S) for b in bad_q],
        dbg(None, V, M, Z, ranks, 4, 0, X, N, S, None), dbg(ctx.h, V, M, Z, ranks, 33, 0, X, N, S, None),
        # the errors come before the early exit: an empty column still needs its pointers and its bounds
        sr(ctx.h, ctypes.byref(capi.CColumn()), M, Z, ranks, 4, 0, X, None, S), qt(ctx.h, ctypes.byref(capi.CColumn()), M, Z, q, 17, X, R, N, S),
        capi.lib.alpgpu_debug_quantile_trace(ctx.h, None, ctypes.byref(capi.QuantileTrace())), capi.lib.alpgpu_debug_quantile_trace(ctx.h, S, None),
    ]
    assert refused == [-2] * len(refused), refused
    ctx.synchronize()
    untouched = lambda: (bool((mask == -1).all()) and bool((vals == 7.0).all()) and bool((out_r == -7).all()) and bool((zones == 7.0).all()) and bool((scratch == CANARY).all()))
    assert untouched() and bool((count == -7).all()), "a refused call wrote"
    # an empty column: ALPGPU_OK, the count alone is written
    empty = capi.CColumn()
    for call in (lambda: sr(ctx.h, ctypes.byref(empty), M, None, ranks, 4, 1, X, N, S), lambda: qt(ctx.h, ctypes.byref(empty), M, None, q, 4, X, R, N, S),
                 lambda: qt(ctx.h, ctypes.byref(empty), M, Z, q, 16, X, None, N, S)):
        count.fill_(-7)
        assert call() == 0
        ctx.synchronize()
        assert count.tolist() == [0, -7] and untouched()
    # the bounds themselves are accepted, d_ranks and d_zones are optional, q = 0 and 1 are quantiles
    s = sorted_selection(xs, np.ones(xs.size, bool))
    count.fill_(-7)
    assert sr(ctx.h, V, M, None, ranks, 32, 0, X, N, S) == 0
    ctx.synchronize()
    assert count.tolist() == [xs.size - int(np.isnan(xs).sum()), -7] and bool((vals[32:] == 7.0).all()) and bool((scratch[-64:] == CANARY).all())
    assert np.array_equal(ints(vals[:32]), ints(host_select_rank(s, range(32))[0]))
    q16 = (ctypes.c_double * 16)(*[i / 15 for i in range(16)])
    vals.fill_(7.0)
    assert qt(ctx.h, V, M, None, q16, 16, X, None, N, S) == 0
    ctx.synchronize()
    assert bool((vals[32:] == 7.0).all()) and bool((out_r == -7).all()) and bool((scratch[-64:] == CANARY).all())
    assert np.array_equal(ints(vals[:32]), ints(host_quantile(s, [i / 15 for i in range(16)])[0]).reshape(-1))


def test_python_rejects_arguments_that_do_not_fit(ctx, monkeypatch):
    col, _, _, _ = column(ctx, "mixed")
    cf, _, _, _ = column(ctx, "mixed_f32")
    nv = col.n_vectors
    mask = torch.full((16 * nv,), 7, dtype=torch.int64, device=DEV)
    vals = torch.full((8,), 7.0, dtype=torch.float64, device=DEV)
    out_r = torch.full((4,), 7, dtype=torch.int64, device=DEV)
    count = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    zones = torch.full((nv, 2), 7.0, dtype=torch.float64, device=DEV)
    scratch = ctx.quantile_scratch(col)

    def unreachable(*a, **k):
        raise AssertionError("the library was called")
    for t in ("f64", "f32"):
        for stem in ("alpgpu_select_rank_", "alpgpu_quantile_", "alpgpu_debug_quantile_"):
            monkeypatch.setattr(capi.lib, stem + t, unreachable)
    ok_r = dict(col=col, mask=mask, ranks=[1, 2, 3, 4], vals_out=vals, count_out=count, zones=zones, scratch=scratch)
    ok_q = dict(col=col, mask=mask, q=[0.1, 0.2, 0.3, 0.4], vals_out=vals, count_out=count, ranks_out=out_r, zones=zones, scratch=scratch)

    def rejected(**change):
        if "q" not in change and "ranks_out" not in change:
            with pytest.raises(ValueError):
                ctx.select_rank_into(**{**ok_r, **change})
        if "ranks" not in change and "tuning" not in change:
            with pytest.raises(ValueError):
                ctx.quantile_into(**{**ok_q, **change})
    wide = torch.full((32 * nv,), 7, dtype=torch.int64, device=DEV)
    for bad in (mask.to(torch.int32), mask.cpu(), mask[:-16], wide, wide[::2], mask.reshape(nv, 16), [1, 2, 3], np.zeros(16 * nv, np.int64)):
        rejected(mask=bad)
    for bad in ([], list(range(33)), [-1], [2**64], [1.5], ["3"], [None], [True], 5, None, "12"):
        rejected(ranks=bad)
        with pytest.raises(ValueError):
            ctx.select_rank(col, mask, bad)
    for bad in ([], [0.5] * 17, [-0.1], [1.1], [NAN], [INF], ["0.5"], [None], [True], None, "0.5"):
        rejected(q=bad)
        with pytest.raises(ValueError):
            ctx.quantile(col, mask, bad)
    for bad in (vals.to(torch.float32), vals.cpu(), vals[:3], vals[::2], None, [1.0]):
        rejected(vals_out=bad)
    rejected(q=[0.1] * 5)  # ten values into eight
    for bad in (out_r.to(torch.int32), out_r.cpu(), out_r[:3], out_r[::2]):
        rejected(ranks_out=bad)
    for bad in (count.to(torch.int32), count.cpu(), count[:0], None):
        rejected(count_out=bad)
    unaligned = torch.zeros(2 * nv + 1, dtype=torch.float64, device=DEV)[1:].reshape(nv, 2)
    for bad in (zones.to(torch.float32), zones.cpu(), zones[:-1], zones.reshape(-1), zones.t(), unaligned):
        rejected(zones=bad)
    for bad in (scratch.to(torch.int8), scratch.cpu(), scratch[:-1], torch.zeros(scratch.numel() + 16, dtype=torch.uint8, device=DEV)[8:]):
        rejected(scratch=bad)
    rejected(col=cf)  # a float column's values and records are floats
    rejected(tuning={"capacity": 1, "grid": 2})
    for bad in ("nearest", None, 1):
        with pytest.raises(ValueError):
            ctx.quantile(col, mask, [0.5], interpolation=bad)
    ctx.synchronize()
    assert bool((mask == 7).all()) and bool((vals == 7.0).all()) and bool((out_r == 7).all()) and bool((count == 7).all()) and bool((zones == 7.0).all())


@pytest.mark.parametrize("name", ["mixed", "mixed_f32"])
def test_interpolation_of_each_kind_against_the_replicas_neighbours(ctx, name):
    col, _, xs, _ = column(ctx, name)
    mask = random_mask(col.n_vectors, 83)
    s = sorted_selection(xs, unpack_mask(mask.cpu().numpy()))
    q = [0.0, 0.123, 0.5, 0.77777, 1.0]
    pairs, r, n = host_quantile(s, q)
    lower, higher, linear = (ctx.quantile(col, mask, q, interpolation=k) for k in ("lower", "higher", "linear"))
    assert lower.dtype == higher.dtype == (torch.float64 if col.dtype == "f64" else torch.float32) and linear.dtype == torch.float64
    assert np.array_equal(ints(lower), ints(pairs[:, 0])) and np.array_equal(ints(higher), ints(pairs[:, 1]))
    lo, hi = pairs[:, 0].astype(np.float64), pairs[:, 1].astype(np.float64)
    frac = np.asarray(q, np.float64) * np.float64(n - 1) - r.astype(np.float64)
    with np.errstate(invalid="ignore"):  # (inf - inf where both neighbours are one infinity: that arm is not taken)
        want = np.where((frac == 0) | (hi == lo), lo, lo + (hi - lo) * frac)
    assert np.array_equal(linear.cpu().numpy().view(np.int64), want.view(np.int64))
    assert np.array_equal(lower.cpu().numpy().astype(np.float64), np.quantile(s.astype(np.float64), q, method="lower"))
    # a number gives a number; nothing selected gives NaN
    assert ints(ctx.quantile(col, mask, 0.5, interpolation="lower").reshape(1))[0] == ints(pairs[2:3, 0])[0]
    zero = torch.zeros_like(mask)
    assert bool(torch.isnan(ctx.quantile(col, zero, [0.5, 0.9])).all()) and bool(torch.isnan(ctx.quantile(col, zero, 0.5, interpolation="higher")))
    v, cnt = ctx.select_rank(col, mask, [0, n - 1, n // 2], from_top=True)
    assert cnt == n and np.array_equal(ints(v), ints(host_select_rank(s, [0, n - 1, n // 2], True)[0]))
    v, cnt = ctx.select_rank(col, zero, [0])
    assert cnt == 0 and v.numel() == 0


# ---- 11. the C++ wrapper ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cpp_column_quantile_and_select_rank_against_decompress_and_a_sort(ctx, tmp_path, dtype):
    """include/alp/batch.hpp: alp::gpu::column<double / float>::quantile and ::select_rank of a serialized column against column::decompress and a host
    std::sort with the same comparator (tests/cpp/quantile_test.cpp)"""
    exe = tmp_path / "quantile_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/quantile_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    col, x, _, _ = column(ctx, "adversarial" if dtype == "f64" else "adversarial_f32")  # NaN, +-inf and -0.0 among the values
    ctx.to_blob(col, x.numel()).tofile(str(tmp_path / "col.blob"))
    mask = vectors_cleared(random_mask(col.n_vectors, 84), 3, -1)
    mask[16:32] = 0
    mask.cpu().numpy().tofile(str(tmp_path / "in.mask"))
    p = subprocess.run([str(exe), dtype, str(tmp_path / "col.blob"), str(tmp_path / "in.mask")], capture_output=True, text=True, timeout=600)
    line = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("ok ")]
    assert p.returncode == 0 and len(line) == 1, p.stdout[-3000:] + p.stderr[-2000:]
    assert int(line[0][1]) == col.n_vectors and int(line[0][2]) > 0
