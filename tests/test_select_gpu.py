"""GPU: range selection on compressed columns (include/alpgpu.h, "selection": alpgpu_select_range_*).  The expected result never comes from the code
under test: it is computed from the store decode, which other suites pin to the oracle and the reference — x = ctx.decode(col),
m = (x >= lo) & (x <= hi) restricted to [first, first + n), indices = nonzero(m), values = x[indices] — and compared on int64 / int32 views, so
that -0.0 and NaN payloads count.  Column kinds x predicates, index ranges, capacities, other column sources, long columns (the prefix sum's
upper levels), determinism, late materialisation with gather, statelessness and stream capture, the Python argument checks, the C++ wrapper and
a speed sanity check."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import datagen
import golden_io
import layout
from alp_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF, NAN = math.inf, math.nan


def ibits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def encoded(ctx, x):
    """(DeviceColumn, x on the device) for a host column of whole vectors"""
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return ctx.encode(xd), xd


def exception_indices(col):
    """value indices of every exception position of every vector, read from the column's own streams"""
    rg, vec, packed, exc = col.to_host()
    W = 8 if col.dtype == "f64" else 4
    out = []
    for v in range(vec.size):
        c = int(vec["exc_cnt"][v])
        if c == 0:
            continue
        e0 = int(vec["exc_off"][v])
        vb = W if vec["scheme"][v] == capi.SCHEME_ALP else 2
        pos = exc[e0 + vb * c:e0 + (vb + 2) * c].view(np.uint16).astype(np.int64)
        assert np.all(np.diff(pos) > 0), "exception positions must ascend (the encoders write them so)"
        out.append(v * 1024 + pos)
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def expected(x, lo, hi, first=0, n=None):
    """(indices, value bits) of the decoded column x inside [lo, hi] and [first, first + n)"""
    n = x.numel() - first if n is None else n
    m = (x >= lo) & (x <= hi)
    m[:first] = False
    m[first + n:] = False
    idx = torch.nonzero(m).reshape(-1)
    return idx, ibits(x)[idx]


def check_select(ctx, col, x, lo, hi, first=0, n=None, what=""):
    """select_range (indices + values, and indices alone) against the decoded column x; -> the selected indices"""
    want_idx, want_bits = expected(x, lo, hi, first, n)
    tag = f"{what} [{lo!r}, {hi!r}] first={first} n={n}"
    idx, vals = ctx.select_range(col, lo, hi, first=first, n=n, values=True)
    assert idx.dtype == torch.int64 and idx.numel() == want_idx.numel(), f"{tag}: {idx.numel()} selected, expected {want_idx.numel()}"
    assert torch.equal(idx, want_idx), f"{tag}: indices differ"
    assert torch.equal(ibits(vals), want_bits), f"{tag}: values differ from the store decode"
    only = ctx.select_range(col, lo, hi, first=first, n=n)
    assert torch.equal(only, want_idx), f"{tag}: indices without values differ"
    return idx


def battery(x, specials):
    """predicates from the column's own finite decoded values (bounds are values that occur, so they are exact in the column's type)"""
    xs = x.cpu().numpy()
    s = np.sort(xs[np.isfinite(xs)])
    q = lambda f: float(s[min(s.size - 1, int(f * s.size))])
    preds = [("everything", -INF, INF), ("middle band", q(0.3), q(0.7)), ("narrow band", q(0.5), q(0.502)), ("point", q(0.41), q(0.41)),
             ("lo > hi", q(0.7), q(0.3)), ("nan lo", NAN, q(0.7)), ("nan hi", q(0.3), NAN), ("low tail", -INF, q(0.1)), ("high tail", q(0.9), INF)]
    if specials:
        preds += [("zero", 0.0, 0.0), ("negative zero", -0.0, -0.0), ("+inf", INF, INF), ("-inf", -INF, -INF)]
    return preds


def check_battery(ctx, col, x, what, specials=False):
    """every predicate of the battery (+ one aimed at an exception, where the column has any): indices, values, count, the per-vector tie to
    decode_count_range; and the battery is not vacuous"""
    total = x.numel()
    exc_idx = exception_indices(col)
    preds = battery(x, specials)
    if exc_idx.size:  # a point predicate on a value that sits at an exception position (a finite one if there is one, else whatever is there but NaN)
        ev = x[torch.from_numpy(exc_idx).to(DEV)].cpu().numpy()
        cand = ev[np.isfinite(ev)] if np.isfinite(ev).any() else ev[~np.isnan(ev)]
        if cand.size:
            v = float(np.sort(cand)[cand.size // 2])
            preds.append(("exception value", v, v))
    exc_set = torch.zeros(total, dtype=torch.bool, device=DEV)
    exc_set[torch.from_numpy(exc_idx).to(DEV)] = True
    partial, hit_exception = False, False
    for name, lo, hi in preds:
        idx = check_select(ctx, col, x, lo, hi, what=f"{what}/{name}")
        per_vector = torch.bincount(idx >> 10, minlength=col.n_vectors).to(torch.int32)
        counts = ctx.decode_count_range(col, lo, hi)
        assert torch.equal(per_vector, counts.view(torch.int32)), f"{what}/{name}: selected per vector != decode_count_range"
        partial = partial or 0 < idx.numel() < total
        hit_exception = hit_exception or bool(exc_set[idx].any())
    assert partial, f"{what}: no predicate of the battery selects some but not all values"
    # (a kind without exceptions, every_width for one, has nothing to hit: the second condition does not apply to it)
    assert hit_exception or exc_idx.size == 0, f"{what}: the column has exceptions and no predicate selected one"


def adversarial_column(cases):
    return np.concatenate([cases[k] for k in sorted(cases)])


DOUBLE_COLUMNS = {
    "mixed": lambda: datagen.mixed_column(250, seed=5),
    "rd_unit": lambda: datagen.rd_column(250, seed=6),
    "rd_latlon": lambda: datagen.rd_column(250, seed=7, kind="latlon"),
    "drifting": lambda: datagen.drifting_column(250, seed=8),
    "every_width_exc": lambda: datagen.every_bit_width_column(208, seed=9, exceptions=True),
    "every_width": lambda: datagen.every_bit_width_column(208, seed=10, exceptions=False),
    "adversarial": lambda: adversarial_column(datagen.adversarial_vectors()),
}
FLOAT_COLUMNS = {
    "mixed_f32": lambda: datagen.mixed_column_f32(250, seed=5),
    "rd_unit_f32": lambda: datagen.rd_column_f32(250, seed=6),
    "rd_latlon_f32": lambda: datagen.rd_column_f32(250, seed=7, kind="latlon"),
    "drifting_f32": lambda: datagen.drifting_column_f32(250, seed=8),
    "adversarial_f32": lambda: adversarial_column(datagen.adversarial_vectors_f32()),
    **{f"decimal_f32_{d}": (lambda d=d: datagen.decimal_column_f32(130, decimals=d, hi=10.0 ** (7 - d), seed=20 + d)) for d in (0, 1, 2, 3, 4, 6)},
}
WITH_SPECIALS = ("mixed", "mixed_f32", "adversarial", "adversarial_f32")  # NaN, +-inf and -0.0 are planted in these


@pytest.mark.parametrize("name", sorted(DOUBLE_COLUMNS) + sorted(FLOAT_COLUMNS))
def test_every_column_kind_against_the_store_decode(ctx, name):
    x = (DOUBLE_COLUMNS.get(name) or FLOAT_COLUMNS[name])()
    col, xd = encoded(ctx, x)
    dec = ctx.decode(col)
    assert torch.equal(ibits(dec), ibits(xd)), f"{name}: decode(encode(x)) != x"
    check_battery(ctx, col, dec, name, specials=name in WITH_SPECIALS)
    if name in WITH_SPECIALS:  # what the special predicates are there for
        zeros = check_select(ctx, col, dec, 0.0, 0.0, what=name)
        zb = ibits(dec)[zeros]
        assert bool((zb != 0).any()), f"{name}: [0, 0] must select -0.0, with its sign kept"
        assert bool((zb == 0).any()) or not name.startswith("adversarial"), f"{name}: [0, 0] must select +0.0 (the all_zero vector)"
        infs = check_select(ctx, col, dec, INF, INF, what=name)
        exc = set(exception_indices(col).tolist())
        scheme = col.to_host()[1]["scheme"]
        in_alp = [i for i in infs.tolist() if scheme[i >> 10] == capi.SCHEME_ALP]
        # (the adversarial vectors share one rowgroup, which the search may give to ALP_RD: +inf is then a left / right part like any value)
        assert infs.numel() > 0 and all(i in exc for i in in_alp), f"{name}: in an ALP vector +inf is an exception, and only exceptions qualify"
        assert len(in_alp) > 0 or not name.startswith("mixed"), f"{name}: the mixed columns are ALP and hold +inf"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_first_and_n(ctx, dtype):
    x = datagen.mixed_column(250, seed=101) if dtype == "f64" else datagen.mixed_column_f32(250, seed=101)
    col, _ = encoded(ctx, x)
    dec = ctx.decode(col)
    total = dec.numel()
    s = np.sort(x[np.isfinite(x)])
    lo, hi = float(s[s.size // 5]), float(s[4 * s.size // 5])
    ranges = [(3 * 1024 + 17, 500), (3 * 1024 + 17, 1), (5 * 1024 - 100, 300), (5 * 1024, 1024), (5 * 1024 - 1, 1026), (100 * 1024 - 700, 5000), (99 * 1024 + 1000, 101 * 1024),
              (1, total - 1), (total - 1, 1), (0, total), (0, 0), (777, 0), (total, 0), (0, total - 1), (1023, 2)]
    for first, n in ranges:
        idx = check_select(ctx, col, dec, lo, hi, first, n, what=dtype)
        check_select(ctx, col, dec, -INF, INF, first, n, what=dtype)
        assert n < 2000 or idx.numel() > 0
    # ranges past the end, and a first + n that overflows, are refused on the host: nothing is written
    fn = getattr(capi.lib, "alpgpu_select_range_" + dtype)
    idx = torch.full((4096,), 7, dtype=torch.int64, device=DEV)
    vals = torch.full((4096,), 7, dtype=dec.dtype, device=DEV)
    count = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    scratch = ctx.select_scratch(col)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for first, n in ((total - 100, 101), (0, total + 1), (total + 1, 0), (2**64 - 1, 2), (2, 2**64 - 1), (2**63, 2**63)):
        assert fn(ctx.h, ctypes.byref(col.c), first, n, lo, hi, p(idx), p(vals), 4096, p(count), p(scratch)) == -2, f"range ({first}, {n}) must be refused"
    ctx.synchronize()
    assert bool((idx == 7).all()) and bool((vals == 7).all()) and int(count) == 7, "a refused select wrote"
    # the other argument checks of the C entry point
    assert fn(ctx.h, None, 0, 10, lo, hi, p(idx), p(vals), 4096, p(count), p(scratch)) == -2
    assert fn(ctx.h, ctypes.byref(col.c), 0, 10, lo, hi, p(idx), p(vals), 4096, None, p(scratch)) == -2
    assert fn(ctx.h, ctypes.byref(col.c), 0, 10, lo, hi, p(idx), p(vals), 4096, p(count), None) == -2
    assert fn(ctx.h, ctypes.byref(col.c), 0, 10, lo, hi, None, p(vals), 4096, p(count), p(scratch)) == -2
    ctx.synchronize()
    assert bool((idx == 7).all()) and bool((vals == 7).all()) and int(count) == 7, "a refused select wrote"
    assert fn(ctx.h, ctypes.byref(col.c), 0, 0, lo, hi, None, None, 0, p(count), None) == 0  # n == 0 needs neither outputs nor scratch
    ctx.synchronize()
    assert int(count) == 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_capacity(ctx, dtype):
    x = datagen.mixed_column(130, seed=111) if dtype == "f64" else datagen.mixed_column_f32(130, seed=111)
    col, _ = encoded(ctx, x)
    dec = ctx.decode(col)
    s = np.sort(x[np.isfinite(x)])
    lo, hi = float(s[s.size // 3]), float(s[s.size // 3 + 5000])
    want_idx, want_bits = expected(dec, lo, hi)
    full = want_idx.numel()
    assert 5000 <= full < dec.numel() // 2
    CANARY, PAD = 0x5A5A5A5A, 96
    scratch = ctx.select_scratch(col)
    for cap in (0, 1, full - 1, full, full + 7):
        for with_vals in (True, False):
            idx = torch.full((cap + PAD,), CANARY, dtype=torch.int64, device=DEV)
            vals = torch.empty(cap + PAD, dtype=dec.dtype, device=DEV)
            ibits(vals).fill_(CANARY)
            count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
            ctx.select_range_into(col, lo, hi, idx[:cap] if cap else None, count, vals[:cap] if with_vals and cap else None, scratch=scratch)
            ctx.synchronize()
            k = min(cap, full)
            tag = f"{dtype} capacity {cap} values {with_vals}"
            assert int(count) == full, f"{tag}: the count is the full count whatever the capacity"
            assert torch.equal(idx[:k], want_idx[:k]), f"{tag}: prefix of the indices"
            assert bool((idx[k:] == CANARY).all()), f"{tag}: indices written behind min(count, capacity)"
            if with_vals:
                assert torch.equal(ibits(vals)[:k], want_bits[:k]), f"{tag}: prefix of the values"
                assert bool((ibits(vals)[k:] == CANARY).all()), f"{tag}: values written behind min(count, capacity)"
            else:
                assert bool((ibits(vals) == CANARY).all()), f"{tag}: values written without a value buffer"
    # the convenience form with a capacity trims to it
    idx, vals = ctx.select_range(col, lo, hi, values=True, capacity=100)
    assert torch.equal(idx, want_idx[:100]) and torch.equal(ibits(vals), want_bits[:100])
    idx = ctx.select_range(col, lo, hi, capacity=full + 50)
    assert torch.equal(idx, want_idx)


def test_golden_vectors_encoded_by_the_oracle(ctx, oracle):
    from oracle.pyoracle import OracleF32
    for name, x, _, _ in golden_io.first_vectors():
        col = capi.DeviceColumn.from_host(*layout.compact(oracle.encode_column(x)))
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(torch.from_numpy(x.copy()).to(DEV))), name
        for pname, lo, hi in battery(dec, False):
            check_select(ctx, col, dec, lo, hi, what=f"{name}/{pname}")
    of = OracleF32()
    for name, x, _, _ in golden_io.float_vectors():
        col = capi.DeviceColumn.from_host(*layout.compact(of.encode_column(x), 4), dtype="f32")
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(torch.from_numpy(x.copy()).to(DEV))), name
        for pname, lo, hi in battery(dec, False):
            check_select(ctx, col, dec, lo, hi, what=f"{name}/{pname}")


def test_columns_encoded_unordered_and_loaded_from_a_blob(ctx):
    x = np.concatenate([datagen.mixed_column(150, seed=31), datagen.rd_column(120, seed=32)])
    ctx.set_option(10, 1)  # ALPGPU_OPT_ENCODE_UNORDERED: records out of vector order
    try:
        col, xd = encoded(ctx, x)
        ctx.synchronize()
    finally:
        ctx.set_option(10, 0)
    check_battery(ctx, col, ctx.decode(col), "unordered", specials=True)
    for dt, xx in (("f64", x), ("f32", datagen.mixed_column_f32(170, seed=33))):
        c0, xd = encoded(ctx, xx)
        bcol, nv = ctx.from_blob(ctx.to_blob(c0, xx.size))
        assert nv == xx.size and bcol.dtype == dt
        check_battery(ctx, bcol, ctx.decode(bcol), "from_blob " + dt, specials=True)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_single_vectors_and_an_empty_column(ctx, dtype):
    cases = datagen.adversarial_vectors() if dtype == "f64" else datagen.adversarial_vectors_f32()
    widths = set()
    for name in ("plain", "all_exceptions", "exceptions_0_to_1022", "all_zero", "constant", "half_negzero", "inf_ends", "prefix_nan"):
        col, xd = encoded(ctx, cases[name])
        assert col.n_vectors == 1
        vec = col.to_host()[1]
        if name == "all_exceptions":
            assert int(vec["exc_cnt"][0]) == 1024 or int(vec["scheme"][0]) == capi.SCHEME_ALP_RD
        widths.add(int(vec["bw"][0]))
        dec = ctx.decode(col)
        for pname, lo, hi in battery(dec, True):
            check_select(ctx, col, dec, lo, hi, what=f"{name}/{pname}")
        v = float(dec[517])
        if not math.isnan(v):
            idx = check_select(ctx, col, dec, v, v, what=name)
            assert 517 in idx.tolist()
        for first, n in ((0, 1), (1023, 1), (63, 2), (64, 64), (100, 900)):
            check_select(ctx, col, dec, -INF, INF, first, n, what=name)
    assert 0 in widths, "none of the single vectors is a 0-bit vector (no packed words)"
    # a vector of 1024 exceptions, whatever the encoder makes of the adversarial one: the plain vector's descriptor with every position listed
    src, _ = encoded(ctx, cases["plain"])
    rg, vec, packed, exc = src.to_host()
    assert int(vec["scheme"][0]) == capi.SCHEME_ALP
    W = 8 if dtype == "f64" else 4
    vals = (np.arange(1024) * 0.37 - 100.0).astype(np.float64 if dtype == "f64" else np.float32)
    rec = np.concatenate([vals.view(np.uint8), np.arange(1024, dtype=np.uint16).view(np.uint8)])
    vec = vec.copy()
    vec["exc_cnt"][0], vec["exc_off"][0] = 1024, 0
    col = capi.DeviceColumn.from_host(rg, vec, packed, rec, dtype=dtype)
    dec = ctx.decode(col)
    assert torch.equal(ibits(dec), ibits(torch.from_numpy(vals).to(DEV)))
    for pname, lo, hi in battery(dec, False):
        check_select(ctx, col, dec, lo, hi, what=f"1024 exceptions/{pname}")
    # an empty column: nothing to select from, the count is written
    empty = capi.CColumn()
    count = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    fn = getattr(capi.lib, "alpgpu_select_range_" + dtype)
    assert fn(ctx.h, ctypes.byref(empty), 0, 0, -INF, INF, None, None, 0, ctypes.c_void_p(count.data_ptr()), None) == 0
    ctx.synchronize()
    assert int(count) == 0
    assert fn(ctx.h, ctypes.byref(empty), 0, 1, -INF, INF, None, None, 0, ctypes.c_void_p(count.data_ptr()), None) == -2


def tiled_column(ctx, x, k):
    """the column encoded from x (a multiple of 100 vectors, so that rowgroups tile too) repeated k times in HBM: descriptors and states tiled, every
    copy pointing at its own copy of the streams"""
    src, _ = encoded(ctx, x)
    ctx.synchronize()
    rg, vec, packed, exc = src.to_host()
    assert vec.size % 100 == 0
    d = vec.size
    tv = np.tile(vec, k)
    rep = np.repeat(np.arange(k, dtype=np.uint64), d)
    tv["packed_off"] += rep * np.uint64(packed.size)
    tv["exc_off"] += rep * np.uint64(exc.size)
    return capi.DeviceColumn.from_host(np.tile(rg, k), tv, np.tile(packed, k), np.tile(exc, k), dtype=src.dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_column_long_enough_for_the_second_scan_level(ctx, dtype):
    """more than 1024 x 64 vectors: the prefix sum over the per-vector counts takes block sums and a level above them"""
    if dtype == "f64":
        x = np.concatenate([datagen.mixed_column(200, seed=121), datagen.rd_column(100, seed=122), datagen.every_bit_width_column(100, seed=123, exceptions=True)])
    else:
        x = np.concatenate([datagen.mixed_column_f32(300, seed=121), datagen.rd_column_f32(100, seed=122)])
    col = tiled_column(ctx, x, 176)
    assert col.n_vectors >= 70000
    dec = ctx.decode(col)
    assert torch.equal(ibits(dec[:x.size]), ibits(torch.from_numpy(x).to(DEV)))
    s = np.sort(x[np.isfinite(x)])
    q = lambda f: float(s[int(f * s.size)])
    total = dec.numel()
    for lo, hi in ((q(0.2), q(0.8)), (q(0.5), q(0.501)), (-INF, INF), (q(0.9), q(0.1))):
        idx = check_select(ctx, col, dec, lo, hi, what=f"tiled {dtype}")
        per_vector = torch.bincount(idx >> 10, minlength=col.n_vectors).to(torch.int32)
        assert torch.equal(per_vector, ctx.decode_count_range(col, lo, hi).view(torch.int32))
    check_select(ctx, col, dec, q(0.2), q(0.8), 1024 * 1500 + 7, total - 1024 * 3000, what=f"tiled {dtype}")
    # a predicate only one far-away vector meets: everything in front of it has a zero count
    one = float(dec[total - 2000])
    if not math.isnan(one):
        idx = check_select(ctx, col, dec, one, one, total - 2048, 2048, what=f"tiled {dtype}")
        assert idx.numel() >= 1


def test_the_scan_alone_at_every_depth(ctx):
    """alpgpu_debug_select_scan over synthetic counts: one block, the block edge, two levels, and three levels (more than 2^20 counts, which a column
    would need 8 GiB of decoded values to reach).  A fourth level takes more than 2^30 counts (12 GB of counts and offsets) and is not run: it is
    the third level's code again — the in-place scan of u64 block sums with block offsets from the level above — which 3 * 2^20 + 5 counts reach."""
    rng = np.random.default_rng(7)
    for n in (1, 2, 63, 64, 1023, 1024, 1025, 4096, 70001, 1 << 20, (1 << 20) + 1, (1 << 20) + 4097, 3 * (1 << 20) + 5):
        counts_np = rng.integers(0, 1025, n).astype(np.uint32)
        if n > 5000:
            counts_np[rng.integers(0, n, n // 3)] = 0
        counts = torch.from_numpy(counts_np.view(np.int32)).to(DEV)
        offsets = torch.full((n + 8,), -1, dtype=torch.int64, device=DEV)
        total = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        scratch = torch.empty(capi.lib.alpgpu_select_scratch_bytes(n), dtype=torch.uint8, device=DEV)
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        assert capi.lib.alpgpu_debug_select_scan(ctx.h, p(counts), n, p(offsets), p(total), p(scratch)) == 0
        ctx.synchronize()
        want = np.concatenate([[0], np.cumsum(counts_np.astype(np.int64))])
        assert int(total) == int(want[-1]), n
        assert np.array_equal(offsets[:n].cpu().numpy(), want[:-1]), n
        assert bool((offsets[n:] == -1).all()), n


def test_the_same_call_gives_the_same_bytes(ctx):
    x = np.concatenate([datagen.mixed_column(300, seed=131), datagen.rd_column(100, seed=132)])
    col, _ = encoded(ctx, x)
    s = np.sort(x[np.isfinite(x)])
    lo, hi = float(s[s.size // 4]), float(s[s.size // 2])
    runs = []
    for rep in range(3):
        cap = 300 * 1024
        idx = torch.full((cap,), -3, dtype=torch.int64, device=DEV)
        vals = torch.full((cap,), -3.0, dtype=torch.float64, device=DEV)
        count = torch.zeros(1, dtype=torch.int64, device=DEV)
        torch.empty(1 << (20 + rep), dtype=torch.uint8, device=DEV).fill_(rep)  # (a different allocation history each time)
        ctx.select_range_into(col, lo, hi, idx, count, vals)
        ctx.synchronize()
        runs.append((idx.cpu().numpy().tobytes(), vals.cpu().numpy().tobytes(), int(count)))
    assert runs[0] == runs[1] == runs[2]
    assert 0 < runs[0][2] < 300 * 1024


def test_late_materialisation_select_on_one_column_gather_from_another(ctx):
    a = datagen.mixed_column(260, seed=141)
    b = np.concatenate([datagen.rd_column(130, seed=142), datagen.drifting_column(130, seed=143)])
    cola, _ = encoded(ctx, a)
    colb, _ = encoded(ctx, b)
    da, db = ctx.decode(cola), ctx.decode(colb)
    s = np.sort(a[np.isfinite(a)])
    lo, hi = float(s[s.size // 10]), float(s[s.size // 5])
    idx = ctx.select_range(cola, lo, hi)
    got = ctx.gather(colb, idx)
    m = (da >= lo) & (da <= hi)
    assert 0 < idx.numel() < da.numel()
    assert torch.equal(ibits(got), ibits(db)[m])
    f32 = datagen.mixed_column_f32(260, seed=144)  # a float column read through a selection on a double column
    colf, _ = encoded(ctx, f32)
    assert torch.equal(ibits(ctx.gather(colf, idx)), ibits(ctx.decode(colf))[m])


def test_a_select_leaves_the_decode_plan_alone(ctx):
    for hinted in (True, False):
        col, _ = encoded(ctx, datagen.mixed_column(150, seed=91))
        if hinted:
            ctx.column_totals(col)
        ctx.decode(col)
        ctx.synchronize()  # (what an unhinted decode learns about the column is in by now)
        before = ctx.decode_plan(col)
        ctx.select_range(col, -5.0, 5.0, values=True)
        ctx.select_range(col, -INF, INF, first=5, n=9999)
        ctx.synchronize()
        assert ctx.decode_plan(col) == before


CAPTURE = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
import datagen
from alp_amd import capi
ctx = capi.Context(0)
side = torch.cuda.Stream()
ok = True
for dtype, x, y in (("f64", datagen.mixed_column(230, seed=81), datagen.mixed_column(230, seed=83)),
                    ("f32", datagen.mixed_column_f32(230, seed=82), datagen.mixed_column_f32(230, seed=84))):
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    col = ctx.encode(xd)
    ctx.column_totals(col)               # hinted: a planned decode
    plan0 = ctx.decode_plan(col)
    s = np.sort(x[np.isfinite(x)])
    lo, hi = float(s[s.size // 4]), float(s[s.size // 2])
    cap = 200 * 1024
    idx = torch.zeros(cap, dtype=torch.int64, device="cuda:0")
    vals = torch.zeros(cap, dtype=xd.dtype, device="cuda:0")
    count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    scratch = ctx.select_scratch(col)
    with torch.cuda.stream(side):
        ctx.select_range_into(col, lo, hi, idx, count, vals, first=1000, n=220 * 1024, scratch=scratch)      # warm-up on the capture stream
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ctx.select_range_into(col, lo, hi, idx, count, vals, first=1000, n=220 * 1024, scratch=scratch)
    iv = torch.int64 if dtype == "f64" else torch.int32
    for rep in range(3):
        if rep == 1:
            ctx.encode(yd, col)          # other data encoded into the same buffers; rep 2 changes nothing
        torch.cuda.synchronize()
        idx.fill_(-1); vals.zero_(); count.zero_(); scratch.fill_(rep)
        g.replay()
        torch.cuda.synchronize()
        got = (idx.clone(), vals.clone(), int(count))
        e_idx, e_vals = ctx.select_range(col, lo, hi, first=1000, n=220 * 1024, values=True)
        dec = ctx.decode(col)
        m = (dec >= lo) & (dec <= hi); m[:1000] = False; m[1000 + 220 * 1024:] = False
        w_idx = torch.nonzero(m).reshape(-1)
        torch.cuda.synchronize()
        k = got[2]
        ok = ok and 0 < k <= cap and k == e_idx.numel() == w_idx.numel() and torch.equal(got[0][:k], e_idx) and torch.equal(e_idx, w_idx)
        ok = ok and torch.equal(got[1][:k].view(iv), e_vals.view(iv)) and torch.equal(e_vals.view(iv), dec[w_idx].view(iv)) and bool((got[0][k:] == -1).all())
        print(dtype, rep, k, ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_column_changes():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


def test_python_rejects_tensors_that_do_not_fit(ctx):
    col, _ = encoded(ctx, datagen.mixed_column(3, seed=95))
    idx = torch.full((64,), 7, dtype=torch.int64, device=DEV)
    vals = torch.full((64,), 7.0, dtype=torch.float64, device=DEV)
    count = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    wide = torch.full((128,), 7, dtype=torch.int64, device=DEV)
    for bad in (idx.to(torch.int32), idx.cpu(), wide[::2], [1, 2, 3], np.arange(64)):
        with pytest.raises(ValueError):
            ctx.select_range_into(col, -INF, INF, bad, count, vals)
    for bad in (vals.to(torch.float32), vals.cpu(), vals[:10], torch.full((128,), 7.0, dtype=torch.float64, device=DEV)[::2]):
        with pytest.raises(ValueError):
            ctx.select_range_into(col, -INF, INF, idx, count, bad)
    for bad in (count.to(torch.int32), count.cpu(), count[:0], None):
        with pytest.raises(ValueError):
            ctx.select_range_into(col, -INF, INF, idx, bad, vals)
    for bad in (torch.zeros(8, dtype=torch.uint8, device=DEV), torch.zeros(4096, dtype=torch.int64, device=DEV), torch.zeros(4096, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ctx.select_range_into(col, -INF, INF, idx, count, vals, scratch=bad)
    with pytest.raises(ValueError):
        ctx.select_range_into(col, -INF, INF, idx, count, vals, first=-1)
    with pytest.raises(ValueError):
        ctx.select_range_into(col, -INF, INF, idx, count, vals, n=-1)
    ctx.synchronize()
    assert bool((idx == 7).all()) and bool((vals == 7).all()) and int(count) == 7, "a refused select launched"


def test_cpp_column_select_range_matches_decompress(tmp_path):
    """include/alp/batch.hpp: alp::gpu::column<double / float>::select_range of a serialized column == a host scan of decompress (tests/cpp/select_test.cpp)"""
    exe = tmp_path / "select_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/select_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0 and "select_test: 0 failures" in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]


def test_a_one_percent_select_is_faster_than_decode_then_filter(ctx):
    """about 1 % of the benchmark's 1 Mi-vector mixed column, indices only, against what the API offered before: a store decode of the column, a
    compare and torch.nonzero on the device.  Alternating, medians of five, same process."""
    sys.path.insert(0, ROOT)
    import bench
    nv = 1 << 20
    x = bench.synthetic_input("mixed", nv, torch.device(DEV), seed=1)
    col = ctx.encode(x)
    sample = x[::251].cpu().numpy()
    del x
    s = np.sort(sample[np.isfinite(sample)])
    lo, hi = float(s[int(0.50 * s.size)]), float(s[int(0.51 * s.size)])
    ctx.column_totals(col)
    out = torch.empty(nv * 1024, dtype=torch.float64, device=DEV)
    cap = nv * 1024 // 20
    idx = torch.empty(cap, dtype=torch.int64, device=DEV)
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    scratch = ctx.select_scratch(col)
    base = {}

    def baseline():
        ctx.decode(col, out)
        base["idx"] = torch.nonzero((out >= lo) & (out <= hi))

    def select():
        ctx.select_range_into(col, lo, hi, idx, count, scratch=scratch)

    ts = {"baseline": [], "select": []}
    for rep in range(7):
        for name, fn in (("baseline", baseline), ("select", select)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b))
    t_base, t_sel = float(np.median(ts["baseline"][2:])), float(np.median(ts["select"][2:]))
    k = int(count)
    print(f"select of {k} values ({k / (nv * 1024):.4f} of the column) {t_sel:.3f} ms, decode + compare + nonzero {t_base:.3f} ms")
    assert 0 < k <= cap and 0.002 < k / (nv * 1024) < 0.05
    assert torch.equal(idx[:k], base["idx"].reshape(-1))
    assert t_sel < t_base
