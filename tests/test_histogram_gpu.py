"""GPU: histograms (include/alpgpu.h, "histograms": alpgpu_histogram_*).  The expected counts never come from the code under test: x = ctx.decode(col)
(pinned to the oracle and the reference by other suites), torch.isnan, torch.bucketize into the NaN-free sorted edges, torch.bincount of the selected
values; tests/histogram_replica.py does the same on the host with numpy.  Counts compare as integers and must be equal."""
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
from histogram_replica import host_histogram, unpack_mask

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF, NAN = math.inf, math.nan
EDGE_COUNTS = (0, 1, 2, 63, 64, 65, 4094, 4095)
POISON = 0x5A5A5A5A5A5A5A5A


def ibits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def unpack(mask):
    s = torch.arange(64, dtype=torch.int64, device=mask.device)
    return (((mask.reshape(-1, 1) >> s) & 1) != 0).reshape(-1)


def random_mask(n_vectors, seed):
    words = np.random.default_rng(seed).integers(0, 2**64, 16 * n_vectors, dtype=np.uint64)
    return torch.from_numpy(words.view(np.int64)).to(DEV)


def vectors_cleared(mask, keep_every):
    """the mask with every vector but each keep_every-th zeroed in all 16 words: skipped vectors beside decoded ones"""
    m = mask.clone().reshape(-1, 16)
    v = torch.arange(m.shape[0], device=mask.device)
    m[(v % keep_every) != 1] = 0
    return m.reshape(-1)


def in_range(total, first, n):
    r = torch.arange(total, device=DEV)
    return (r >= first) & (r < first + n)


def expect(x, edges, sel=None, right=False):
    """the definition on the device, by torch: edges in any order, NaNs among them inert"""
    s = torch.sort(edges).values
    real = s[~torch.isnan(s)]
    xs = x if sel is None else x[sel]
    nan = torch.isnan(xs)
    out = torch.zeros(edges.numel() + 2, dtype=torch.int64, device=x.device)
    b = torch.bucketize(xs[~nan], real, right=not right)  # (torch's right=True is "edges <= x", the call's right == 0)
    out[: edges.numel() + 1] = torch.bincount(b, minlength=edges.numel() + 1)
    out[-1] = nan.sum()
    return out


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
        out.append(v * 1024 + exc[e0 + vb * c:e0 + (vb + 2) * c].view(np.uint16).astype(np.int64))
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def make_edges(xs, size, seed):
    """`size` edges in no order: +-inf and both zeros first, then values of the column itself (values sit on edges), padded with noise the column does
    not hold where it has too few distinct values"""
    rng = np.random.default_rng(seed)
    present = np.unique(xs[~np.isnan(xs)])
    must = np.array([INF, -INF, 0.0, -0.0], dtype=xs.dtype)[: min(size, 4)]
    k = min(size - must.size, max(0, present.size // 2))
    own = rng.choice(present, k, replace=False) if k else present[:0]
    pad = (rng.standard_normal(size - must.size - k) * 12345.678).astype(xs.dtype)
    e = np.concatenate([must, own, pad]).astype(xs.dtype)
    assert e.size == size and e.dtype == xs.dtype
    return rng.permutation(e)


def adversarial_column(cases):
    return np.concatenate([cases[k] for k in sorted(cases)])


COLUMNS = {
    "mixed": lambda: datagen.mixed_column(250, seed=5),
    "rd_unit": lambda: datagen.rd_column(250, seed=6),
    "every_width_exc": lambda: datagen.every_bit_width_column(208, seed=9, exceptions=True),
    "adversarial": lambda: adversarial_column(datagen.adversarial_vectors()),
    "mixed_f32": lambda: datagen.mixed_column_f32(250, seed=5),
    "rd_unit_f32": lambda: datagen.rd_column_f32(250, seed=6),
    "every_width_exc_f32": lambda: datagen.every_bit_width_column_f32(200, seed=9, exceptions=True),
    "adversarial_f32": lambda: adversarial_column(datagen.adversarial_vectors_f32()),
}
_cache = {}


def column(ctx, name):
    """(DeviceColumn, its store decode, the decode on the host), encoded once per session and left unchanged"""
    if name not in _cache:
        xd = torch.from_numpy(np.ascontiguousarray(COLUMNS[name]())).to(DEV)
        col = ctx.encode(xd)
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(xd)), f"{name}: decode(encode(x)) != x"
        _cache[name] = (col, dec, dec.cpu().numpy())
    return _cache[name]


def raw_column(ctx, key, make):
    if key not in _cache:
        xd = torch.from_numpy(np.ascontiguousarray(make())).to(DEV)
        col = ctx.encode(xd)
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(xd))
        _cache[key] = (col, dec, dec.cpu().numpy())
    return _cache[key]


def sorted_column(ctx, f32):
    def make():
        # (whole numbers for float: vectors without an exception, which a record can settle)
        raw = datagen.decimal_column_f32(120, decimals=0, hi=100000.0, seed=31) if f32 else datagen.decimal_column(120, seed=31)
        return np.sort(raw)
    return raw_column(ctx, "sorted_f32" if f32 else "sorted", make)


def masks_of(col, seed):
    rnd = random_mask(col.n_vectors, seed)
    return {"none": None, "random": rnd, "vectors zero": vectors_cleared(rnd, 3)}


def debug_call(ctx, col, edges, counts, mask=None, first=0, n=None, right=0, zones=None, accumulate=0, tuning=None, trace=None, n_edges=None):
    """alpgpu_debug_histogram_* by ctypes: the return code"""
    fn = getattr(capi.lib, "alpgpu_debug_histogram_" + col.dtype)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr() if isinstance(t, torch.Tensor) else t)
    n = col.n_vectors * 1024 - first if n is None else n
    t = capi.HistogramTuning(*tuning) if tuning is not None else None
    return fn(ctx.h, ctypes.byref(col.c), first, n, p(mask), p(zones), p(edges), edges.numel() if n_edges is None else n_edges, right, accumulate, p(counts),
              ctypes.byref(t) if t is not None else None, p(trace))


# ---- 1. every edge count on every kind of column, both rules, three bitmaps ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_edge_counts_on_every_column_against_the_store_decode(ctx, name):
    col, x, xs = column(ctx, name)
    total = x.numel()
    out = {n: torch.full((n + 2,), POISON, dtype=torch.int64, device=DEV) for n in EDGE_COUNTS}  # overwritten: what they held does not matter
    on_edge = False
    for mname, mask in masks_of(col, 1).items():
        sel = None if mask is None else unpack(mask)
        for size in EDGE_COUNTS:
            edges = torch.from_numpy(make_edges(xs, size, 100 + size)).to(DEV)
            assert edges.numel() == size
            on_edge = on_edge or bool(torch.isin(x, edges[torch.isfinite(edges)]).any())
            for right in (False, True):
                want = expect(x, edges, sel, right)
                got = ctx.histogram(col, edges, mask=mask, right=right, out=out[size])
                assert got is out[size] and torch.equal(got, want), f"{name}, {size} edges, right={right}, bitmap {mname}: counts differ from bucketize + bincount on the store decode"
                assert int(want.sum()) == (total if sel is None else int(sel.sum()))
            if size in (2, 65):  # the host replica, fed the store decode, says the same
                s = np.sort(edges.cpu().numpy())
                host = host_histogram(xs, s, None if mask is None else unpack_mask(mask.cpu().numpy(), total), right=True)
                assert np.array_equal(got.cpu().numpy().view(np.uint64), host)
    assert on_edge, "no value of the column sat on an edge"
    fresh = ctx.histogram(col, torch.from_numpy(make_edges(xs, 65, 165)).to(DEV))  # the allocating form
    assert fresh.dtype == torch.int64 and fresh.numel() == 67 and torch.equal(fresh, expect(x, torch.from_numpy(make_edges(xs, 65, 165)).to(DEV)))
    assert size == 4095 == capi.HISTOGRAM_EDGES_MAX


def test_zeros_infinities_and_values_on_edges(ctx):
    for name in ("mixed", "mixed_f32"):
        col, x, xs = column(ctx, name)
        assert np.any((xs == 0) & np.signbit(xs)) and np.any(np.isinf(xs)) and np.any(np.isnan(xs))
        v = xs[np.isfinite(xs) & (xs != 0)][7]
        n_v, n_zero, n_nan = int((xs == v).sum()), int((xs == 0).sum()), int(np.isnan(xs).sum())
        n_below = int((xs < v).sum())
        for zero in (0.0, -0.0):
            e = torch.tensor([zero], dtype=x.dtype, device=DEV)
            assert ctx.histogram(col, e).tolist() == [int((xs < 0).sum()), int((xs >= 0).sum()), n_nan]  # -0.0 == +0.0: both zeros at or above the edge
            assert ctx.histogram(col, e, right=True).tolist() == [int((xs <= 0).sum()), int((xs > 0).sum()), n_nan]
        e = torch.tensor([v], dtype=x.dtype, device=DEV)
        assert ctx.histogram(col, e).tolist() == [n_below, xs.size - n_nan - n_below, n_nan]
        assert ctx.histogram(col, e, right=True).tolist() == [n_below + n_v, xs.size - n_nan - n_below - n_v, n_nan]
        e = torch.tensor([-INF, INF], dtype=x.dtype, device=DEV)
        n_pinf, n_ninf = int((xs == INF).sum()), int((xs == -INF).sum())
        assert ctx.histogram(col, e).tolist() == [0, xs.size - n_nan - n_pinf, n_pinf, n_nan]
        assert ctx.histogram(col, e, right=True).tolist() == [n_ninf, xs.size - n_nan - n_ninf, 0, n_nan]
        assert n_v > 0 and n_zero > 0 and n_pinf > 0 and n_ninf > 0


# ---- 2. ranges ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "mixed_f32"])
def test_first_and_n(ctx, name):
    col, x, xs = column(ctx, name)
    total = x.numel()
    edges = torch.sort(torch.from_numpy(make_edges(xs, 65, 7)).to(DEV)).values
    rnd = random_mask(col.n_vectors, 2)
    ranges = [(3 * 1024 + 17, 500), (3 * 1024 + 17, 1), (63, 1), (63, 2), (64, 64), (1024 + 63, 66), (5 * 1024 - 100, 300), (5 * 1024, 1024), (5 * 1024 - 1, 1026),
              (99 * 1024 + 1000, 101 * 1024), (total - 1, 1), (0, total), (0, total - 500), (0, 0), (777, 0), (total, 0), (1023, 2)]
    out = torch.empty(67, dtype=torch.int64, device=DEV)
    for first, n in ranges:
        r = in_range(total, first, n)
        for mask in (None, rnd):
            sel = r if mask is None else r & unpack(mask)
            for right in (False, True):
                out.fill_(POISON)
                ctx.histogram(col, edges, mask=mask, first=first, n=n, right=right, out=out, sorted=True)
                assert torch.equal(out, expect(x, edges, sel, right)), f"{name} first={first} n={n} right={right} mask={mask is not None}"
                assert int(out.sum()) == int(sel.sum())
    # n == 0 under accumulate: nothing changes
    out.fill_(5)
    ctx.histogram(col, edges, first=777, n=0, out=out, accumulate=True, sorted=True)
    assert bool((out == 5).all())
    # ranges past the end, and a first + n that overflows, are refused on the host: the counts are unchanged
    out.fill_(POISON)
    for first, n in ((total - 100, 101), (0, total + 1), (total + 1, 0), (2**64 - 1, 2), (2, 2**64 - 1), (2**63, 2**63)):
        assert debug_call(ctx, col, edges, out, first=first, n=n) == -2, f"range ({first}, {n}) must be refused"
    ctx.synchronize()
    assert bool((out == POISON).all()), "a refused histogram wrote"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_single_vector_and_an_empty_column(ctx, dtype):
    cases = datagen.adversarial_vectors() if dtype == "f64" else datagen.adversarial_vectors_f32()
    for name in ("plain", "all_exceptions", "all_zero", "half_negzero", "inf_ends", "prefix_nan"):
        col = ctx.encode(torch.from_numpy(cases[name]).to(DEV))
        assert col.n_vectors == 1
        x = ctx.decode(col)
        xs = x.cpu().numpy()
        mask = random_mask(1, 3)
        for size in (0, 1, 3, 65, 4095):
            edges = torch.from_numpy(make_edges(xs, size, 7 + size)).to(DEV)
            for right in (False, True):
                for first, n in ((0, 1024), (1023, 1), (63, 2), (100, 900)):
                    sel = in_range(1024, first, n)
                    assert torch.equal(ctx.histogram(col, edges, first=first, n=n, right=right), expect(x, edges, sel, right)), f"{name}, {size} edges, first={first} n={n}"
                    assert torch.equal(ctx.histogram(col, edges, mask=mask, first=first, n=n, right=right), expect(x, edges, sel & unpack(mask), right))
    empty = capi.CColumn()
    fn = getattr(capi.lib, "alpgpu_histogram_" + dtype)
    edges = torch.zeros(4, dtype=torch.float64 if dtype == "f64" else torch.float32, device=DEV)
    out = torch.full((6,), POISON, dtype=torch.int64, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for accumulate in (0, 1):
        assert fn(ctx.h, ctypes.byref(empty), 0, 0, None, None, p(edges), 4, 0, accumulate, p(out)) == 0
        assert fn(ctx.h, ctypes.byref(empty), 0, 0, None, None, None, 0, 1, accumulate, p(out)) == 0
        assert fn(ctx.h, ctypes.byref(empty), 0, 1, None, None, p(edges), 4, 0, accumulate, p(out)) == -2
    ctx.synchronize()
    assert bool((out == POISON).all()), "a column of no vectors writes nothing"


# ---- 3. NaNs: values, edges; duplicates --------------------------------------------------------------------------------------------------------------------
def nan_columns(ctx, f32):
    """(an ALP column whose NaNs are exceptions, an ALP_RD column a third of whose values are NaNs: their left part is a dictionary entry)"""
    def rd():
        r = np.random.default_rng(44).random(3 * 1024)
        r[::3] = NAN
        return r.astype(np.float32) if f32 else r
    return column(ctx, "adversarial_f32" if f32 else "adversarial"), raw_column(ctx, "rd_nan_f32" if f32 else "rd_nan", rd)


@pytest.mark.parametrize("f32", [False, True])
def test_selected_nans_land_in_the_last_word_and_nowhere_else(ctx, f32):
    (alp, xa, xsa), (rd, xr, xsr) = nan_columns(ctx, f32)
    exc_a, exc_r = np.zeros(xsa.size, bool), np.zeros(xsr.size, bool)
    exc_a[exception_indices(alp)] = True
    exc_r[exception_indices(rd)] = True
    assert (np.isnan(xsa) & exc_a).any(), "a NaN that is an exception"
    rg, vec, _, _ = rd.to_host()
    assert (vec["scheme"] == capi.SCHEME_ALP_RD).all() and (np.isnan(xsr) & ~exc_r).any(), "a NaN in an ALP_RD vector that is no exception"
    for col, x, xs in ((alp, xa, xsa), (rd, xr, xsr)):
        n_nan = int(np.isnan(xs).sum())
        mask = random_mask(col.n_vectors, 8)
        sel = unpack(mask)
        for size in (0, 5, 65):
            edges = torch.from_numpy(make_edges(xs, size, 30 + size)).to(DEV)
            for right in (False, True):
                got = ctx.histogram(col, edges, right=right)
                assert torch.equal(got, expect(x, edges, None, right)) and int(got[-1]) == n_nan and int(got[:-1].sum()) == xs.size - n_nan
                got = ctx.histogram(col, edges, mask=mask, right=right)
                assert torch.equal(got, expect(x, edges, sel, right)) and int(got[-1]) == int((torch.isnan(x) & sel).sum()) > 0
        nan_mask = torch.zeros(16 * col.n_vectors, dtype=torch.int64, device=DEV)
        w = torch.ones(64, dtype=torch.int64, device=DEV) << torch.arange(64, dtype=torch.int64, device=DEV)
        nan_mask.copy_((torch.isnan(x).reshape(-1, 64).to(torch.int64) * w).sum(dim=1))
        got = ctx.histogram(col, torch.tensor([0.5], dtype=x.dtype, device=DEV), mask=nan_mask)
        assert got.tolist() == [0, 0, n_nan], "a selection of NaNs alone"


@pytest.mark.parametrize("name", ["mixed", "mixed_f32"])
def test_nan_edges_at_the_end_and_duplicates_add_empty_buckets(ctx, name):
    col, x, xs = column(ctx, name)
    for size in (5, 64, 2000):  # (doubled below: at most 4095)
        edges = torch.sort(torch.from_numpy(np.unique(make_edges(xs, size, 50 + size))).to(DEV)).values  # distinct (the two zeros are one)
        n = edges.numel()
        for right in (False, True):
            base = ctx.histogram(col, edges, right=right, sorted=True)
            assert torch.equal(base, expect(x, edges, None, right))
            nans = torch.full((3,), NAN, dtype=x.dtype, device=DEV)
            got = ctx.histogram(col, torch.cat([nans, edges]), right=right)  # the wrapper sorts: NaNs last
            assert torch.equal(got[: n + 1], base[: n + 1]) and got[n + 1: n + 4].tolist() == [0, 0, 0] and got[-1] == base[-1]
            by_hand = torch.cat([edges, nans])
            assert torch.equal(ctx.histogram(col, by_hand, right=right, sorted=True), got)
            twice = torch.sort(torch.cat([edges, edges])).values  # every edge doubled: an empty bucket between the twins
            got = ctx.histogram(col, twice, right=right, sorted=True)
            assert torch.equal(got, expect(x, twice, None, right))
            assert torch.equal(got[0:-1:2], base[:-1]) and bool((got[1:-2:2] == 0).all()) and got[-1] == base[-1]
    only_nans = torch.full((9,), NAN, dtype=x.dtype, device=DEV)
    n_nan = int(np.isnan(xs).sum())
    assert ctx.histogram(col, only_nans).tolist() == [xs.size - n_nan] + [0] * 9 + [n_nan]


# ---- 4. accumulate -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "rd_unit_f32"])
def test_accumulate_adds_and_a_plain_call_overwrites(ctx, name):
    col, x, xs = column(ctx, name)
    total = x.numel()
    edges = torch.from_numpy(make_edges(xs, 300, 3)).to(DEV)
    mask = random_mask(col.n_vectors, 21)
    whole = ctx.histogram(col, edges, mask=mask)
    assert torch.equal(whole, expect(x, edges, unpack(mask)))
    cut = 117 * 1024 + 333  # inside a vector
    out = torch.full((302,), POISON, dtype=torch.int64, device=DEV)
    ctx.histogram(col, edges, mask=mask, first=0, n=cut, out=out)  # overwrites the poison
    ctx.histogram(col, edges, mask=mask, first=cut, n=total - cut, out=out, accumulate=True)
    assert torch.equal(out, whole), "two half ranges added are the whole range"
    ctx.histogram(col, edges, mask=mask, out=out, accumulate=True)
    assert torch.equal(out, 2 * whole)
    start = torch.arange(302, dtype=torch.int64, device=DEV) * 1000003
    out.copy_(start)
    ctx.histogram(col, edges, mask=mask, out=out, accumulate=True)
    assert torch.equal(out, start + whole)


# ---- 5. zone maps --------------------------------------------------------------------------------------------------------------------------------------------
def widened(zones):
    z = zones.cpu().numpy().copy()
    dt = z.dtype.type
    with np.errstate(over="ignore"):
        z[:, 0] = np.nextafter(z[:, 0], dt(-INF))
        z[:, 1] = np.nextafter(z[:, 1], dt(INF))
    return torch.from_numpy(z).to(DEV)


def settled_by_record(vec, zones, edges_sorted, sel_any, right):
    """vectors the kernel settles from their record, by the rule: selected, both bounds no NaNs, one bucket, ALP without exceptions (vec: the descriptors)"""
    z = zones.cpu().numpy()
    e = edges_sorted.cpu().numpy()
    e = e[~np.isnan(e)]
    side = "left" if right else "right"
    ok = ~np.isnan(z).any(axis=1)
    z = np.where(np.isnan(z), 0, z)
    j0, j1 = np.searchsorted(e, z[:, 0], side=side), np.searchsorted(e, z[:, 1], side=side)
    return sel_any & ok & (j0 == j1) & (vec["scheme"] == capi.SCHEME_ALP) & (vec["exc_cnt"] == 0)


def some_exceptions_column(ctx, f32):
    """40 vectors of whole numbers, all ALP: the first 20 without an exception, the others with a few (one of them a NaN)"""
    def make():
        raw = datagen.decimal_column_f32(40, decimals=0, hi=100000.0, seed=77) if f32 else datagen.decimal_column(40, decimals=0, seed=77)
        for v in range(20, 40):
            raw[v * 1024 + 5: v * 1024 + 8] = raw.dtype.type(np.pi) * raw[v * 1024 + 5: v * 1024 + 8]
        raw[33 * 1024 + 100] = NAN
        return raw
    return raw_column(ctx, "some_exc_f32" if f32 else "some_exc", make)


@pytest.mark.parametrize("f32", [False, True])
def test_zone_maps_change_no_count(ctx, f32):
    settled_some = False
    for cname, (col, x, xs) in (("random", column(ctx, "mixed_f32" if f32 else "mixed")), ("sorted", sorted_column(ctx, f32))):
        nv, total = col.n_vectors, x.numel()
        _, vec, _, _ = col.to_host()
        zones = ctx.zone_map(col)
        holes = zones.clone()
        holes[::3, 0] = NAN  # a NaN bound: prunes nothing
        holes[1::3, 1] = NAN
        mask = vectors_cleared(random_mask(nv, 12), 3)
        masked = ctx.decode_minmax_masked(col, mask)  # the records of the selected values alone
        first, n = 1024 + 100, total - 2048  # vectors outside the range, two cut by it, the rest whole
        for size in (0, 1, 7, 65, 4095):
            edges = torch.sort(torch.from_numpy(make_edges(xs, size, 70 + size)).to(DEV)).values
            for right in (False, True):
                for m, records in ((None, {"the zone map": zones, "widened": widened(zones), "NaN bounds": holes}),
                                   (mask, {"the zone map": zones, "widened": widened(zones), "masked": masked, "masked widened": widened(masked)})):
                    sel = in_range(total, first, n) if m is None else in_range(total, first, n) & unpack(m)
                    plain = ctx.histogram(col, edges, mask=m, first=first, n=n, right=right, sorted=True)
                    assert torch.equal(plain, expect(x, edges, sel, right)), f"{cname}, {size} edges: without zones"
                    for zname, z in records.items():
                        trace = torch.zeros(4, dtype=torch.int64, device=DEV)
                        got = torch.full_like(plain, POISON)
                        ctx.histogram_into(col, edges, got, mask=m, first=first, n=n, right=right, zones=z, trace=trace)
                        assert got.cpu().numpy().tobytes() == plain.cpu().numpy().tobytes(), f"{cname}, {size} edges, right={right}: {zname} changed the counts"
                        t = trace.tolist()
                        sel_any = sel.reshape(nv, 1024).any(dim=1).cpu().numpy()
                        want1 = int(settled_by_record(vec, z, edges, sel_any, right).sum())
                        assert t == [nv - int(sel_any.sum()), want1, 0, int(sel_any.sum()) - want1], f"{cname}, {size} edges, {zname}: trace {t}"
                        settled_some = settled_some or (cname == "sorted" and size == 65 and t[1] > 0)
    assert settled_some, "the sorted ALP column settled no vector from its record"


@pytest.mark.parametrize("f32", [False, True])
def test_zone_records_settle_alp_vectors_without_exceptions_only(ctx, f32):
    # an all-ALP_RD column: never settled from a record, whatever it says
    col, x, xs = column(ctx, "rd_unit_f32" if f32 else "rd_unit")
    _, vec, _, _ = col.to_host()
    assert (vec["scheme"] == capi.SCHEME_ALP_RD).all()
    zones = ctx.zone_map(col)
    edges = torch.tensor([-1.0, 2.0], dtype=x.dtype, device=DEV)  # every record of values in [0, 1) lies in bucket 1
    trace = torch.zeros(4, dtype=torch.int64, device=DEV)
    got = torch.empty(4, dtype=torch.int64, device=DEV)
    ctx.histogram_into(col, edges, got, zones=zones, trace=trace)
    assert got.tolist() == [0, x.numel(), 0, 0] and trace.tolist() == [0, 0, 0, col.n_vectors]
    # a column with exceptions in some vectors: with no edge at all every record lies in the one bucket, and exactly the ALP vectors without exceptions are settled
    col, x, xs = some_exceptions_column(ctx, f32)
    _, vec, _, _ = col.to_host()
    zones = ctx.zone_map(col)
    clean = (vec["scheme"] == capi.SCHEME_ALP) & (vec["exc_cnt"] == 0) & ~np.isnan(zones.cpu().numpy()).any(axis=1)
    assert 0 < int(clean.sum()) < col.n_vectors and ((vec["scheme"] == capi.SCHEME_ALP) & (vec["exc_cnt"] > 0)).any()
    trace.zero_()
    got = torch.empty(2, dtype=torch.int64, device=DEV)
    none = torch.zeros(0, dtype=x.dtype, device=DEV)
    ctx.histogram_into(col, none, got, zones=zones, trace=trace)
    n_nan = int(np.isnan(xs).sum())
    assert got.tolist() == [xs.size - n_nan, n_nan] and n_nan > 0
    assert trace.tolist() == [0, int(clean.sum()), 0, col.n_vectors - int(clean.sum())], "a vector with exceptions is decoded, not settled from its record"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_lying_records_and_unsorted_edges_keep_the_total_and_stay_inside_the_counts(ctx, dtype):
    for col, x, xs in (column(ctx, "mixed" if dtype == "f64" else "mixed_f32"), sorted_column(ctx, dtype == "f32")):
        lying_records_and_unsorted_edges(ctx, col, x, xs)


def lying_records_and_unsorted_edges(ctx, col, x, xs):
    nv = col.n_vectors
    mask = random_mask(nv, 33)
    n_sel = int(unpack(mask).sum())
    zones = ctx.zone_map(col)
    lies = {"swapped": zones.flip(1).contiguous(), "shifted": torch.roll(zones, 7, 0).contiguous(), "a point": torch.full_like(zones, 12.5),
            "infinite": torch.stack([torch.full((nv,), INF, dtype=x.dtype, device=DEV), torch.full((nv,), -INF, dtype=x.dtype, device=DEV)], dim=1).contiguous()}
    guard = 64
    for size in (1, 65, 4095):
        unsorted = torch.from_numpy(make_edges(xs, size, 5 + size)).to(DEV)
        in_order = torch.sort(unsorted).values
        cases = [("unsorted edges", unsorted, None), ("unsorted edges with the zone map", unsorted, zones)] + [("records: " + k, in_order, z) for k, z in lies.items()]
        for what, edges, z in cases:
            for right in (0, 1):
                buf = torch.full((guard + size + 2 + guard,), POISON, dtype=torch.int64, device=DEV)
                counts = buf[guard: guard + size + 2]
                assert debug_call(ctx, col, edges, counts, mask=mask, right=right, zones=z) == 0
                ctx.synchronize()
                assert bool((buf[:guard] == POISON).all()) and bool((buf[guard + size + 2:] == POISON).all()), f"{what}, {size} edges: guard words changed"
                assert bool((counts >= 0).all()) and int(counts.sum()) == n_sel, f"{what}, {size} edges: the total is the selected count"


# ---- 6. tuning: the flush, the grid; determinism -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
def test_tuning_changes_no_count(ctx, f32):
    col, x, xs = raw_column(ctx, "small_f32" if f32 else "small", lambda: datagen.mixed_column_f32(24, seed=61) if f32 else datagen.mixed_column(24, seed=61))
    assert col.n_vectors == 24
    mask = random_mask(24, 62)
    for size in (3, 65, 4095):
        edges = torch.sort(torch.from_numpy(make_edges(xs, size, 63 + size)).to(DEV)).values
        want = expect(x, edges, unpack(mask))
        runs = []
        # one workgroup of 8 wavefronts makes 3 trips over 24 vectors: flush_every = 1 flushes in the loop after each; then the default, one workgroup,
        # more workgroups than the column has work for, and a flush every second trip
        for tuning in ({"grid": 1, "flush_every": 1}, None, {"grid": 1}, {"grid": 1000}, {"grid": 2, "flush_every": 2}, {"flush_every": 1}):
            got = torch.full_like(want, POISON)
            trace = torch.zeros(4, dtype=torch.int64, device=DEV)
            ctx.histogram_into(col, edges, got, mask=mask, tuning=tuning, trace=trace)
            assert torch.equal(got, want), f"{size} edges, tuning {tuning}"
            assert trace.tolist() == [0, 0, 0, 24]
            runs.append(got.cpu().numpy().tobytes())
        assert len(set(runs)) == 1


def test_the_same_call_gives_the_same_bytes(ctx):
    col, x, xs = column(ctx, "mixed")
    zones = ctx.zone_map(col)
    edges = torch.from_numpy(make_edges(xs, 1000, 4)).to(DEV)
    mask = random_mask(col.n_vectors, 5)
    runs = []
    for rep in range(3):
        torch.empty(1 << (20 + rep), dtype=torch.uint8, device=DEV).fill_(rep)  # (a different allocation history each time)
        out = ctx.histogram(col, edges, mask=mask)
        ctx.histogram(col, edges, first=999, n=100000, zones=zones, right=True, out=out, accumulate=True)
        runs.append(out.cpu().numpy().tobytes())
    assert runs[0] == runs[1] == runs[2]
    assert torch.equal(out, expect(x, edges, unpack(mask)) + expect(x, edges, in_range(x.numel(), 999, 100000), True))


# ---- 7. the two ways of adding: a step whose lanes agree, a step whose lanes differ ----------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True])
def test_one_bucket_and_alternating_buckets(ctx, f32):
    dt = np.float32 if f32 else np.float64
    n = 20 * 1024
    const = raw_column(ctx, ("const", f32), lambda: np.full(n, 5.25, dt))
    alt = raw_column(ctx, ("alt", f32), lambda: np.where(np.arange(n) % 2 == 0, 1.5, 3.5).astype(dt))
    wide = torch.from_numpy(np.sort(np.concatenate([np.linspace(-100, 100, 2000), [2.5]])).astype(dt)).to(DEV)
    mask = random_mask(20, 71)
    for edges in (torch.tensor([2.5], dtype=const[1].dtype, device=DEV), wide):
        for col, x, xs in (const, alt):
            for m in (None, mask):
                sel = None if m is None else unpack(m)
                for right in (False, True):
                    got = ctx.histogram(col, edges, mask=m, right=right, sorted=True)
                    assert torch.equal(got, expect(x, edges, sel, right))
                    assert int((got != 0).sum()) == (1 if col is const[0] else 2)
    got = ctx.histogram(alt[0], torch.tensor([2.5], dtype=alt[1].dtype, device=DEV))
    assert got.tolist() == [n // 2, n // 2, 0]


# ---- 8. statelessness, capture ---------------------------------------------------------------------------------------------------------------------------------
def test_histogram_calls_leave_the_decode_plan_alone(ctx):
    for hinted in (True, False):
        raw = datagen.mixed_column(150, seed=91)
        col = ctx.encode(torch.from_numpy(raw).to(DEV))
        if hinted:
            ctx.column_totals(col)
        ctx.decode(col)
        ctx.synchronize()  # (what an unhinted decode learns about the column is in by now)
        before = ctx.decode_plan(col)
        vals = raw[~np.isnan(raw)][:300]
        out = ctx.histogram(col, vals)
        ctx.histogram(col, vals[:5], first=5, n=9999, right=True)
        ctx.histogram(col, vals, mask=random_mask(150, 92), zones=ctx.zone_map(col), out=out, accumulate=True)
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
def expect(x, edges, sel, right):
    real = edges[~torch.isnan(edges)]
    xs = x[sel]
    nan = torch.isnan(xs)
    out = torch.zeros(edges.numel() + 2, dtype=torch.int64, device=x.device)
    out[: edges.numel() + 1] = torch.bincount(torch.bucketize(xs[~nan], real, right=not right), minlength=edges.numel() + 1)
    out[-1] = nan.sum()
    return out
def unpack(mask):
    s = torch.arange(64, dtype=torch.int64, device=mask.device)
    return (((mask.reshape(-1, 1) >> s) & 1) != 0).reshape(-1)
def draw(x, size, seed):
    rng = np.random.default_rng(seed)
    u = np.unique(x[np.isfinite(x)])
    return torch.sort(torch.from_numpy(rng.choice(u, size, replace=False)).cuda()).values
def bitmap(nv, seed):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 2**64, 16 * nv, dtype=np.uint64).view(np.int64)).cuda()
nv = 230
a0, a1 = datagen.mixed_column(nv, seed=81), datagen.mixed_column(nv, seed=83)
b0, b1 = datagen.mixed_column_f32(nv, seed=82), datagen.mixed_column_f32(nv, seed=84)
ad, bd = [torch.from_numpy(t).cuda() for t in (a0, a1)], [torch.from_numpy(t).cuda() for t in (b0, b1)]
cola, colb = ctx.encode(ad[0]), ctx.encode(bd[0])
na, nb = 65, 4095
ea, eb = draw(a0, na, 1), draw(b0, nb, 2)
mask = bitmap(nv, 5)
outa = torch.zeros(na + 2, dtype=torch.int64, device="cuda:0")
outb = torch.zeros(nb + 2, dtype=torch.int64, device="cuda:0")
def calls():
    ctx.histogram(cola, ea, mask=mask, first=1000, n=220 * 1024, out=outa, sorted=True)
    ctx.histogram(colb, eb, right=True, out=outb, sorted=True)
    ctx.histogram(colb, eb, mask=mask, right=True, out=outb, accumulate=True, sorted=True)
with torch.cuda.stream(side):
    calls()                                                 # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        calls()
for rep in range(3):
    if rep == 1:
        ctx.encode(ad[1], cola); ctx.encode(bd[1], colb)    # other data encoded into the same buffers, other edges and another bitmap written into the same tensors
        ea.copy_(draw(a1, na, 3)); eb.copy_(draw(b1, nb, 4)); mask.copy_(bitmap(nv, 6))
    torch.cuda.synchronize()
    outa.fill_(rep - 1); outb.fill_(rep - 1)
    g.replay()
    torch.cuda.synchronize()
    da, db = ctx.decode(cola), ctx.decode(colb)
    sel = unpack(mask)
    r = torch.arange(da.numel(), device="cuda:0")
    wa = expect(da, ea, sel & (r >= 1000) & (r < 1000 + 220 * 1024), False)
    wb = expect(db, eb, torch.ones_like(sel), True) + expect(db, eb, sel, True)
    ok = ok and torch.equal(outa, wa) and torch.equal(outb, wb) and int(wa.sum()) > 0
    print(rep, int(wa.sum()), int(wb.sum()), ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_edges_the_bitmap_and_the_columns_change():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 9. argument checks ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c_argument_checks(ctx, dtype):
    name = "mixed" if dtype == "f64" else "mixed_f32"
    col, x, xs = column(ctx, name)
    nv, vb = col.n_vectors, 8 if dtype == "f64" else 4
    edges = torch.sort(torch.from_numpy(make_edges(xs, 4095, 9)).to(DEV)).values
    zones = ctx.zone_map(col)
    mask = random_mask(nv, 10)
    out = torch.full((4097 + 8,), POISON, dtype=torch.int64, device=DEV)
    trace = torch.full((5,), POISON, dtype=torch.int64, device=DEV)
    fn, dbg = getattr(capi.lib, "alpgpu_histogram_" + dtype), getattr(capi.lib, "alpgpu_debug_histogram_" + dtype)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    c = ctypes.byref(col.c)
    for right in (0, 1):
        for acc in (0, 1):
            assert fn(None, c, 0, 1024, p(mask), None, p(edges), 65, right, acc, p(out)) == -2, "a NULL context must be refused"
            assert fn(ctx.h, None, 0, 1024, p(mask), None, p(edges), 65, right, acc, p(out)) == -2, "a NULL column must be refused"
            assert fn(ctx.h, c, 0, 1024, p(mask), None, p(edges), 65, right, acc, None) == -2, "NULL counts must be refused"
            assert fn(ctx.h, c, 0, 1024, p(mask), None, None, 65, right, acc, p(out)) == -2, "NULL edges with n_edges > 0 must be refused"
            assert fn(ctx.h, c, 0, 1024, p(mask), None, p(edges), 4096, right, acc, p(out)) == -2, "n_edges beyond ALPGPU_HISTOGRAM_EDGES_MAX must be refused"
            assert fn(ctx.h, c, 0, 1024, p(mask), None, p(edges), 2**32 - 1, right, acc, p(out)) == -2
            assert fn(ctx.h, c, 0, 1024, p(mask, 4), None, p(edges), 65, right, acc, p(out)) == -2, "a misaligned bitmap must be refused"
            assert fn(ctx.h, c, 0, 1024, p(mask), None, p(edges, vb // 2), 65, right, acc, p(out)) == -2, "misaligned edges must be refused"
            assert fn(ctx.h, c, 0, 1024, p(mask), p(zones, vb), p(edges), 65, right, acc, p(out)) == -2, "misaligned zones must be refused"
            assert fn(ctx.h, c, 0, 1024, p(mask), None, p(edges), 65, right, acc, p(out, 4)) == -2, "misaligned counts must be refused"
            assert dbg(ctx.h, c, 0, 1024, p(mask), None, p(edges), 65, right, acc, p(out), None, p(trace, 4)) == -2, "a misaligned trace must be refused"
            assert fn(ctx.h, c, 1, nv * 1024, p(mask), None, p(edges), 65, right, acc, p(out)) == -2, "a range past the end must be refused"
    ctx.synchronize()
    assert bool((out == POISON).all()) and bool((trace == POISON).all()), "a refused call wrote"
    # n == 0: the counts (and nothing behind them) are zeroed unless the call accumulates
    assert fn(ctx.h, c, 5, 0, p(mask), None, p(edges), 65, 0, 1, p(out)) == 0
    ctx.synchronize()
    assert bool((out == POISON).all())
    assert fn(ctx.h, c, 5, 0, p(mask), None, p(edges), 65, 0, 0, p(out)) == 0
    ctx.synchronize()
    assert bool((out[:67] == 0).all()) and bool((out[67:] == POISON).all())
    # no edges with a NULL pointer is valid: one bucket and the NaN counter; the full 4095 edges fill exactly their 4097 words
    out.fill_(POISON)
    assert fn(ctx.h, c, 0, x.numel(), None, None, None, 0, 0, 0, p(out)) == 0
    ctx.synchronize()
    n_nan = int(np.isnan(xs).sum())
    assert out[:2].tolist() == [xs.size - n_nan, n_nan] and bool((out[2:] == POISON).all())
    assert fn(ctx.h, c, 0, x.numel(), p(mask), p(zones), p(edges), 4095, 1, 0, p(out)) == 0
    ctx.synchronize()
    assert torch.equal(out[:4097], expect(x, edges, unpack(mask), True)) and bool((out[4097:] == POISON).all())


def test_python_rejects_arguments_that_do_not_fit(ctx, monkeypatch):
    col, x, xs = column(ctx, "mixed")
    cf = column(ctx, "mixed_f32")[0]
    nv = col.n_vectors
    edges = torch.sort(torch.from_numpy(make_edges(xs, 65, 1)).to(DEV)).values
    out = torch.full((67,), 7, dtype=torch.int64, device=DEV)
    mask = random_mask(nv, 3)
    zones = ctx.zone_map(col)

    def unreachable(*a, **k):
        raise AssertionError("the library was called")
    for t in ("f64", "f32"):
        monkeypatch.setattr(capi.lib, "alpgpu_histogram_" + t, unreachable)
        monkeypatch.setattr(capi.lib, "alpgpu_debug_histogram_" + t, unreachable)
    for bad in (edges.to(torch.float32), edges.cpu().numpy().astype(np.float32), edges.to(torch.int64), edges[:64].reshape(8, 8), np.arange(5),
                torch.zeros(4096, dtype=torch.float64, device=DEV), np.zeros(5000)):  # the column's type, one dimension, at most 4095
        with pytest.raises(ValueError):
            ctx.histogram(col, bad, out=None)
    with pytest.raises(ValueError):
        ctx.histogram(cf, edges)  # a float column takes float edges
    for bad in (out.to(torch.int32), out.cpu(), out[:-1], torch.zeros(68, dtype=torch.int64, device=DEV), torch.zeros(134, dtype=torch.int64, device=DEV)[::2], out.reshape(1, 67),
                [0] * 67, np.zeros(67, np.int64)):
        with pytest.raises(ValueError):
            ctx.histogram(col, edges, out=bad)
    with pytest.raises(ValueError):
        ctx.histogram(col, edges, accumulate=True)  # adds to a tensor: which?
    wide = torch.full((32 * nv,), 7, dtype=torch.int64, device=DEV)
    for bad in (mask.to(torch.int32), mask.cpu(), mask[:-16], wide, wide[::2], mask.reshape(nv, 16), [1, 2, 3]):
        with pytest.raises(ValueError):
            ctx.histogram(col, edges, mask=bad, out=out)
    for kw in ({"first": -1}, {"n": -1}):
        with pytest.raises(ValueError):
            ctx.histogram(col, edges, out=out, **kw)
    unaligned = torch.zeros(2 * nv + 1, dtype=torch.float64, device=DEV)[1:].reshape(nv, 2)
    for bad in (zones.to(torch.float32), zones.cpu(), zones[:-1], zones.reshape(-1), zones.t(), unaligned, [[0.0, 1.0]] * nv):
        with pytest.raises(ValueError):
            ctx.histogram(col, edges, zones=bad, out=out)
    # the raw form: sorted device edges only, a trace of 4 words, the tuning's two names
    for bad in (edges.cpu(), edges.cpu().numpy(), edges.tolist(), torch.zeros(130, dtype=torch.float64, device=DEV)[::2]):
        with pytest.raises(ValueError):
            ctx.histogram_into(col, bad, out)
    for bad in (torch.zeros(3, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int64)):
        with pytest.raises(ValueError):
            ctx.histogram_into(col, edges, out, trace=bad)
    with pytest.raises(ValueError):
        ctx.histogram_into(col, edges, out, tuning={"grid": 1, "capacity": 5})
    ctx.synchronize()
    assert bool((out == 7).all()), "a refused call launched"


def test_edges_in_every_form_the_wrapper_takes(ctx):
    col, x, xs = column(ctx, "mixed")
    edges = torch.from_numpy(make_edges(xs, 65, 2)).to(DEV)
    want = expect(x, edges)
    host = edges.cpu()
    for e in (edges, host, host.numpy(), host.tolist(), tuple(host.tolist())):
        assert torch.equal(ctx.histogram(col, e), want)
    n_nan = int(np.isnan(xs).sum())
    assert ctx.histogram(col, []).tolist() == [xs.size - n_nan, n_nan]
    assert torch.equal(ctx.histogram(col, torch.sort(edges).values, sorted=True), want)


# ---- 10. the C++ wrapper ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cpp_column_histogram_against_decompress_and_a_host_loop(ctx, tmp_path, dtype):
    """include/alp/batch.hpp: alp::gpu::column<double / float>::histogram of a serialized column against column::decompress and a host loop over the
    definition of a bucket (tests/cpp/histogram_test.cpp)"""
    exe = tmp_path / "histogram_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/histogram_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    name = "adversarial" if dtype == "f64" else "adversarial_f32"  # NaN, +-inf and -0.0 among the values
    col, x, xs = column(ctx, name)
    ctx.to_blob(col, x.numel()).tofile(str(tmp_path / "col.blob"))
    edges = np.concatenate([make_edges(xs, 40, 5), np.array([NAN, NAN], dtype=xs.dtype)])
    edges.tofile(str(tmp_path / "edges.bin"))
    mask = vectors_cleared(random_mask(col.n_vectors, 53), 3)
    mask[16:32] = -1
    mask.cpu().numpy().tofile(str(tmp_path / "in.mask"))
    p = subprocess.run([str(exe), dtype] + [str(tmp_path / f) for f in ("col.blob", "edges.bin", "in.mask")], capture_output=True, text=True, timeout=600)
    line = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("ok ")]
    assert p.returncode == 0 and len(line) == 1, p.stdout[-3000:] + p.stderr[-2000:]
    k = int(unpack(mask).sum())
    assert int(line[0][1]) == col.n_vectors and int(line[0][2]) == k and 0 < k < x.numel()


# ---- 11. the route it replaces -----------------------------------------------------------------------------------------------------------------------------------
def test_sixteen_buckets_are_group_totals_of_decode_group_sum(ctx):
    """INTEGRATION.md 2i's workaround: decode_group_sum(col, col, mask, edges[:-1], edges[1:] nudged down by one ulp, counts=...) + group_totals"""
    col, x, xs = column(ctx, "mixed")
    finite = np.sort(xs[np.isfinite(xs)])
    edges_np = np.unique(finite[np.linspace(0, finite.size - 1, 17).astype(np.int64)])
    assert edges_np.size == 17
    lo, hi = edges_np[:-1], np.nextafter(edges_np[1:], -INF)  # closed ranges made disjoint
    for mask in (torch.full((16 * col.n_vectors,), -1, dtype=torch.int64, device=DEV), random_mask(col.n_vectors, 15)):
        counts = torch.zeros((16, col.n_vectors), dtype=torch.int32, device=DEV)
        sums = ctx.decode_group_sum(col, col, mask, lo.tolist(), hi.tolist(), counts=counts)
        total_counts = torch.zeros(16, dtype=torch.int64, device=DEV)
        ctx.group_totals(sums, counts, counts_out=total_counts)
        got = ctx.histogram(col, edges_np, mask=mask)
        assert got.numel() == 19 and torch.equal(got[1:17], total_counts), "buckets 1 .. 16 are the 16 groups"
        assert torch.equal(got, expect(x, torch.from_numpy(edges_np).to(DEV), unpack(mask)))
        assert int(got[0]) > 0 and int(got[17]) > 0 and int(got[18]) > 0  # below the first edge (-inf), at or above the last (the maximum, +inf), the NaNs
