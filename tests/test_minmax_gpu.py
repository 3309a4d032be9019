"""GPU: masked and grouped MIN / MAX (include/alpgpu.h, "masked and grouped MIN / MAX": alpgpu_decode_minmax_masked_*, alpgpu_decode_group_minmax_*,
alpgpu_group_minmax_totals_*).  The expected result never comes from the code under test: val = ctx.decode(col_val), key = ctx.decode(col_key)
(pinned to the oracle and the reference by other suites), the predicate evaluated on the host, the records by the definition of a record,
tests/minmax_replica.py.  Minimum and maximum are exact, so everything compares on integer views of the bits; there is no tolerance anywhere."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import datagen
from alp_amd import capi
from minmax_replica import host_group_minmax, host_minmax_masked, host_minmax_totals
from test_group_gpu import quantile_groups
from test_mask_gpu import COLUMNS, bounds, column, exception_indices, pack, random_mask, unpack, vectors_cleared
from test_pair_gpu import PAIRS, pair
from test_zone_gpu import expected_zones, reduce_keys

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF, NAN = float("inf"), float("nan")


def ib(a):
    """the integer view of a float array or tensor, as numpy"""
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same(got, want):
    return ib(got).shape == ib(want).shape and np.array_equal(ib(got), ib(want))


def host(t, nv):
    return t.cpu().numpy().reshape(nv, 1024)


def empty_record(dtype):
    return ib(np.array([INF, -INF], dtype=dtype)).tolist()


def sentinel(shape, dtype):
    return torch.full(shape, 7.0, dtype=dtype, device=DEV)


def run_masked(ctx, col, mask):
    nv = col.n_vectors
    tdt = torch.float64 if col.dtype == "f64" else torch.float32
    zones, counts = sentinel((nv, 2), tdt), torch.full((nv,), 7, dtype=torch.int32, device=DEV)
    assert ctx.decode_minmax_masked(col, mask, out=zones, counts=counts) is zones
    return zones, counts


def run_group(ctx, cv, ck, mask, lo, hi):
    nv = cv.n_vectors
    tdt = torch.float64 if cv.dtype == "f64" else torch.float32
    zones, counts = sentinel((len(lo), nv, 2), tdt), torch.full((len(lo), nv), 7, dtype=torch.int32, device=DEV)
    assert ctx.decode_group_minmax(cv, ck, mask, lo, hi, out=zones, counts=counts) is zones
    return zones, counts


def one_bit_per_vector(col):
    """a bitmap with one set bit in every vector: on the vector's first exception position where it has one"""
    nv = col.n_vectors
    pos = (np.arange(nv) * 37 + 11) % 1024
    exc = np.sort(exception_indices(col))
    vs, first = np.unique(exc >> 10, return_index=True)
    pos[vs] = exc[first] & 1023
    bits = np.zeros((nv, 1024), dtype=bool)
    bits[np.arange(nv), pos] = True
    return pack(torch.from_numpy(bits.reshape(-1)).to(DEV)), vs.size


# ---- 1. every column kind -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_every_column_kind_against_the_host_replica(ctx, name):
    col, x = column(ctx, name)
    nv = col.n_vectors
    xn = host(x, nv)
    rnd = random_mask(nv, 41)
    single, with_exc = one_bit_per_vector(col)
    assert with_exc > 0 or exception_indices(col).size == 0
    unmasked = None
    for mname, mask in (("full", torch.full_like(rnd, -1)), ("random", rnd), ("vectors zero", vectors_cleared(rnd, 3, 0)), ("one bit", single)):
        tag = f"{name}, mask {mname}"
        bits = host(unpack(mask), nv)
        want_z, want_c = host_minmax_masked(xn, bits)
        kept = mask.clone()
        zones, counts = run_masked(ctx, col, mask)
        bad = np.nonzero((ib(zones) != ib(want_z)).any(axis=1))[0]
        assert bad.size == 0, f"{tag}: {bad.size} records differ, first vector {bad[0]}: got {zones[int(bad[0])].tolist()}, expected {want_z[bad[0]].tolist()}"
        assert np.array_equal(counts.cpu().numpy(), want_c.astype(np.int32)), f"{tag}: counts are not the popcounts"
        assert torch.equal(mask, kept), f"{tag}: the bitmap was written"
        without = ctx.decode_minmax_masked(col, mask)  # counts=None, out allocated
        assert without.shape == (nv, 2) and without.dtype == x.dtype and same(without, want_z), f"{tag}: without counts"
        if mname == "full":
            unmasked = want_z
            assert same(zones, ctx.zone_map(col)), f"{tag}: not the records of zone_map"
            assert np.array_equal(ib(want_z), expected_zones(x).cpu().numpy()), "the replica is not the zone suite's expectation"
        if mname == "random" and nv >= 200:  # the bitmap really moves the records: a kernel that ignored it would fail
            share = float((ib(want_z)[:, 0] != ib(unmasked)[:, 0]).mean())
            assert share >= 0.25, f"{tag}: the masked minimum differs from the vector's in only {share:.2f} of the vectors"
        if mname == "vectors zero":
            cleared = np.nonzero(~bits.any(axis=1))[0]
            assert cleared.size > nv // 2 and ib(zones)[cleared].tolist() == [empty_record(xn.dtype)] * cleared.size and not counts.cpu().numpy()[cleared].any()
        if mname == "one bit":
            assert want_c.tolist() == [1] * nv
        # the column's MIN / MAX is zones_minmax over the records
        lo, hi = reduce_keys(torch.from_numpy(want_z[:, 0].copy()), torch.from_numpy(want_z[:, 1].copy()))
        assert ib(ctx.column_minmax(zones)).tolist() == [int(lo), int(hi)], f"{tag}: column_minmax of the records"


# ---- 2. hand-made vectors -----------------------------------------------------------------------------------------------------------------------------
def snan(dtype):
    return np.array([0x7FF0000000000001], dtype=np.int64).view(np.float64)[0] if dtype == np.float64 else np.array([0x7F800001], dtype=np.int32).view(np.float32)[0]


@pytest.mark.parametrize("scheme", ["alp", "alp_rd"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_hand_made_vectors(ctx, dtype, scheme):
    dt = np.float64 if dtype == "f64" else np.float32
    rng = np.random.default_rng(61)
    if scheme == "alp":
        x = np.round(rng.uniform(1.0, 900.0, 8 * 1024), 2).astype(dt).reshape(8, 1024)
        small, large = dt(0.25), dt(950.5)
    else:
        x = (rng.random(8 * 1024) * 0.5 + 0.25).astype(dt).reshape(8, 1024)  # full precision in [0.25, 0.75)
        small, large = dt(0.2500001), dt(0.7500001)
    bits = np.zeros((8, 1024), dtype=bool)
    x[0, 5], x[0, 69] = -0.0, 0.0          # vector 0: both zeros selected, in one lane, and nothing else
    bits[0, [5, 69]] = True
    x[1, 5], x[1, 69] = -0.0, 0.0          # vector 1: +0.0 selected, -0.0 not
    bits[1, [69, 70, 200]] = True
    x[2, 7] = snan(dt)                     # vector 2: a signalling NaN beside numbers
    bits[2, [7, 8, 9, 1000]] = True
    x[3, 3], x[3, 4] = NAN, snan(dt)       # vector 3: only NaNs selected
    bits[3, [3, 4]] = True
    x[4, 10], x[4, 11] = INF, -INF         # vector 4: +-inf are values
    bits[4, [10, 11, 12]] = True
    x[5, 0] = small                        # vector 5: the minimum at value 0
    bits[5] = True
    x[6, 1023] = large                     # vector 6: the maximum at value 1023
    bits[6] = True
    # vector 7: the maximum in an exception record.  Twenty values far above the others, no two-decimal numbers and each with an exponent of its
    # own, four apart: an ALP vector encodes those beyond its integer range as exceptions, and an ALP_RD dictionary holds eight left parts at the most
    x[7, 400:420] = (np.pi * 1e3 * 16.0 ** np.arange(20)).astype(dt)
    xd = torch.from_numpy(x.reshape(-1)).to(DEV)
    col = ctx.encode(xd)
    dec = ctx.decode(col)
    assert same(dec, xd), "decode(encode(x)) != x"
    schemes = col.to_host()[1]["scheme"]
    assert (schemes == (capi.SCHEME_ALP if scheme == "alp" else capi.SCHEME_ALP_RD)).all(), schemes
    exc7 = exception_indices(col)
    exc7 = exc7[(exc7 >> 10) == 7] & 1023
    assert exc7.size > 0, "vector 7 has no exception"
    top = int(exc7[np.argmax(x[7, exc7])])
    assert 400 <= top < 420, "none of the planted values is an exception"
    odd = x[7, top]
    bits[7] = x[7] <= odd                  # everything up to the largest exception: the maximum is in the exception record
    bits[7, 3] = False
    mask = pack(torch.from_numpy(bits.reshape(-1)).to(DEV))
    zones, counts = run_masked(ctx, col, mask)
    z = ib(zones).tolist()
    rec = lambda mn, mx: ib(np.array([mn, mx], dtype=dt)).tolist()
    assert z[0] == rec(-0.0, 0.0) and z[0][0] < 0 and z[0][1] == 0
    assert z[1] == rec(0.0, max(x[1, 70], x[1, 200])) and z[1][0] == 0, "an unselected -0.0 is not the minimum"
    assert z[2] == rec(min(x[2, 8], x[2, 9], x[2, 1000]), max(x[2, 8], x[2, 9], x[2, 1000]))
    assert z[3] == empty_record(dt)
    assert z[4] == rec(-INF, INF)
    assert z[5] == rec(small, x[5].max()) and z[6] == rec(x[6].min(), large)
    assert z[7] == rec(np.delete(x[7], 3).min(), odd) and int(bits[7].sum()) > 1000
    assert counts.tolist() == [2, 3, 4, 2, 3, 1024, 1024, int(bits[7].sum())]
    want_z, want_c = host_minmax_masked(x, bits)
    assert same(zones, want_z) and np.array_equal(counts.cpu().numpy(), want_c)
    # the same through the grouped call with the column as its own key: the open group, and a band that holds the zeros alone
    gz, gc = run_group(ctx, col, col, mask, [-INF, -0.0], [INF, 0.0])
    want_gz, want_gc = host_group_minmax(x, x, bits, [-INF, -0.0], [INF, 0.0])
    assert same(gz, want_gz) and np.array_equal(gc.cpu().numpy(), want_gc)
    g = ib(gz).tolist()
    assert g[1][0] == rec(-0.0, 0.0) and g[1][1] == rec(0.0, 0.0) and g[1][2] == empty_record(dt) and gc[1].tolist() == [2, 1, 0, 0, 0, 0, 0, 0]
    assert g[0][3] == empty_record(dt) and gc[0].tolist() == [2, 3, 3, 0, 3, 1024, 1024, int(bits[7].sum())], "a NaN is in no group of its own column"


def test_no_shared_double_column_has_a_vector_with_both_zeros(ctx):
    """... which is why the hand-made vectors carry that case"""
    for name in sorted(COLUMNS):
        if not name.endswith("_f32"):
            xn = host(column(ctx, name)[1], column(ctx, name)[0].n_vectors)
            neg, pos = (xn == 0) & np.signbit(xn), (xn == 0) & ~np.signbit(xn)
            assert not (neg.any(axis=1) & pos.any(axis=1)).any(), name


# ---- 3. grouped ---------------------------------------------------------------------------------------------------------------------------------------
_grouped = {}


def grouped(ctx, pname):
    """the records and counts of a pair under the random mask and its quantile groups: ((zones, counts) of the device, (zones, counts) of the replica)"""
    if pname not in _grouped:
        cv, val, ck, key = pair(ctx, pname)
        nv = cv.n_vectors
        lo, hi = quantile_groups(key)
        mask = random_mask(nv, 41)
        _grouped[pname] = (run_group(ctx, cv, ck, mask, lo, hi), host_group_minmax(host(val, nv), host(key, nv), host(unpack(mask), nv), lo, hi))
    return _grouped[pname]


@pytest.mark.parametrize("pname", sorted(PAIRS))
def test_grouped_on_every_scheme_pairing(ctx, pname):
    cv, val, ck, key = pair(ctx, pname)
    nv = cv.n_vectors
    vn, kn = host(val, nv), host(key, nv)
    lo, hi = quantile_groups(key)
    assert 8 < len(lo) <= capi.GROUP_MAX
    rnd = random_mask(nv, 41)
    exc_v, exc_k = exception_indices(cv), exception_indices(ck)
    for mname, mask in (("full", torch.full_like(rnd, -1)), ("random", rnd), ("vectors zero", vectors_cleared(rnd, 3, 0))):
        tag = f"{pname}, mask {mname}"
        bits = host(unpack(mask), nv)
        kept = mask.clone()
        if mname == "random":
            (zones, counts), (want_z, want_c) = grouped(ctx, pname)
        else:
            want_z, want_c = host_group_minmax(vn, kn, bits, lo, hi)
            zones, counts = run_group(ctx, cv, ck, mask, lo, hi)
        assert same(zones, want_z), f"{tag}: records differ from the replica"
        assert np.array_equal(counts.cpu().numpy(), want_c.astype(np.int32)), f"{tag}: counts"
        assert torch.equal(mask, kept), f"{tag}: the bitmap was written"
        # counts are decode_group_sum's
        sum_counts = torch.empty((len(lo), nv), dtype=torch.int32, device=DEV)
        ctx.decode_group_sum(cv, ck, mask, lo, hi, counts=sum_counts)
        assert torch.equal(counts, sum_counts), f"{tag}: counts are not decode_group_sum's"
        # every row is select_mask and then decode_minmax_masked, through the existing entry points
        for g in range(len(lo)):
            m = mask.clone()
            ctx.select_mask(ck, lo[g], hi[g], op="and", mask=m)
            row_z, row_c = run_masked(ctx, cv, m)
            assert torch.equal(zones[g].view(torch.uint8), row_z.view(torch.uint8)) and torch.equal(counts[g], row_c), f"{tag}, group {g}: not decode_minmax_masked under the ANDed bitmap"
        without = ctx.decode_group_minmax(cv, ck, mask, lo, hi)  # counts=None, out allocated
        assert without.shape == (len(lo), nv, 2) and without.dtype == val.dtype and same(without, want_z), f"{tag}: without counts"
        e = empty_record(vn.dtype)
        assert int(want_c[7].sum()) == 0 and int(want_c[8].sum()) == 0 and ib(zones[7:9]).reshape(-1, 2).tolist() == [e] * (2 * nv), "lo > hi and a NaN bound select nothing"
        if mname == "full":
            assert 0 < int(want_c[2].sum()) < bits.sum(), f"{tag}: a band selects some but not all"
            sel = (bits & (kn >= -INF) & (kn <= INF)).reshape(-1)
            for exc in (exc_v, exc_k):
                assert exc.size == 0 or sel[exc].any(), f"{tag}: the pair has exceptions and none is selected"


# ---- 4. tier edges ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_groups", [1, 3, 4, 5, 8, 9, 16])
def test_tier_edges_write_their_rows_and_nothing_behind(ctx, n_groups):
    cv, val, ck, key = pair(ctx, "alp_rd")
    nv = cv.n_vectors
    xs = np.sort(key.cpu().numpy())
    cuts = [float(xs[int(f * (xs.size - 1))]) for f in np.linspace(0.0, 1.0, n_groups + 1)]
    lo, hi = cuts[:-1], cuts[1:]  # touching bands
    mask = random_mask(nv, 42)
    bits = host(unpack(mask), nv)
    want_z, want_c = host_group_minmax(host(val, nv), host(key, nv), bits, lo, hi)
    zones = sentinel((n_groups + 2, nv, 2), torch.float64)
    counts = torch.full((n_groups + 2, nv), 7, dtype=torch.int32, device=DEV)
    ctx.decode_group_minmax(cv, ck, mask, lo, hi, out=zones[:n_groups], counts=counts[:n_groups])
    assert same(zones[:n_groups], want_z) and np.array_equal(counts[:n_groups].cpu().numpy(), want_c.astype(np.int32))
    assert bool((zones[n_groups:] == 7.0).all()) and bool((counts[n_groups:] == 7).all()), "written behind the last group's row"
    assert int(want_c.sum()) >= int(bits.sum())  # the bands cover every value; the shared boundaries count twice
    counts.fill_(7)
    zones.fill_(7.0)
    ctx.decode_group_minmax(cv, ck, mask, lo, hi, out=zones[:n_groups])
    assert same(zones[:n_groups], want_z) and bool((counts == 7).all()) and bool((zones[n_groups:] == 7.0).all()), "counts=None writes no counts"


# ---- 5. ragged launches -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_one_vector_and_a_ragged_last_workgroup(ctx, dtype):
    f32 = dtype == "f32"
    cases = datagen.adversarial_vectors_f32() if f32 else datagen.adversarial_vectors()
    five_v = datagen.mixed_column_f32(5, seed=31) if f32 else datagen.mixed_column(5, seed=31)
    five_k = datagen.drifting_column_f32(5, seed=32) if f32 else datagen.drifting_column(5, seed=32)
    for xv, xk in ((cases["prefix_nan"], cases["inf_ends"]), (cases["plain"], cases["half_negzero"]), (cases["all_exceptions"], cases["plain"]), (five_v, five_k)):
        cv, ck = ctx.encode(torch.from_numpy(xv).to(DEV)), ctx.encode(torch.from_numpy(xk).to(DEV))
        val, key = ctx.decode(cv), ctx.decode(ck)
        nv = cv.n_vectors
        assert nv in (1, 5)
        lo, hi = quantile_groups(key)
        mask = random_mask(nv, 49)
        if nv == 5:
            mask[16:32] = 0  # a skipped vector inside the first workgroup
        bits = host(unpack(mask), nv)
        vn, kn = host(val, nv), host(key, nv)
        want_z, want_c = host_minmax_masked(vn, bits)
        zones, counts = run_masked(ctx, cv, mask)
        assert same(zones, want_z) and np.array_equal(counts.cpu().numpy(), want_c), f"{dtype}, {nv} vectors: masked"
        want_gz, want_gc = host_group_minmax(vn, kn, bits, lo, hi)
        gz, gc = run_group(ctx, cv, ck, mask, lo, hi)
        assert same(gz, want_gz) and np.array_equal(gc.cpu().numpy(), want_gc), f"{dtype}, {nv} vectors: grouped"
        if nv == 5:
            e = empty_record(vn.dtype)
            assert ib(zones)[1].tolist() == e and int(counts[1]) == 0 and ib(gz)[:, 1].tolist() == [e] * len(lo) and not bool(gc[:, 1].any()), "a vector without a set bit"


# ---- 6. totals ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["alp_rd", "adversarial_rolled", "widths_f32", "adversarial_rolled_f32"])
def test_totals_of_the_grouped_records(ctx, pname):
    (zones, counts), (want_z, want_c) = grouped(ctx, pname)
    totals = ctx.group_minmax_totals(zones)
    assert totals.shape == (zones.shape[0], 2) and totals.dtype == zones.dtype
    assert same(totals, host_minmax_totals(want_z)), "totals differ from the replica"
    for g in range(zones.shape[0]):
        assert same(totals[g], ctx.column_minmax(zones[g])), f"group {g}: not alpgpu_zones_minmax of the row"
    out = sentinel((zones.shape[0], 2), zones.dtype)
    assert ctx.group_minmax_totals(zones, out=out) is out and same(out, totals)
    e = empty_record(want_z.dtype)
    assert ib(totals)[7].tolist() == e and ib(totals)[8].tolist() == e and ib(totals)[0].tolist() != e


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_totals_of_synthetic_records_and_of_none(ctx, dtype):
    dt = np.float64 if dtype == "f64" else np.float32
    n = 300_000
    rng = np.random.default_rng(62)
    mins = rng.uniform(-1000.0, 0.0, (3, n)).astype(dt)
    z = np.stack([mins, (mins + rng.uniform(0.0, 1000.0, (3, n))).astype(dt)], axis=-1)
    z[0, 0, 0], z[0, n - 1, 1] = -5000.0, 5000.0       # the extremes in the first and in the last record
    z[1, n // 2] = [-INF, 6000.0]                       # ... in a middle one
    z[2] = [INF, -INF]                                  # an all-empty row
    z[0, 7] = [INF, -INF]                               # an empty record among others
    z[1, 9, 1] = -0.0
    zones = torch.from_numpy(z).to(DEV)
    kept = zones.clone()
    totals = ctx.group_minmax_totals(zones)
    assert ib(totals).tolist() == [ib(np.array(r, dtype=dt)).tolist() for r in ([-5000.0, 5000.0], [-INF, 6000.0], [INF, -INF])]
    assert same(totals, host_minmax_totals(z)) and torch.equal(zones.view(torch.uint8), kept.view(torch.uint8))
    for g in range(3):
        assert same(totals[g], ctx.column_minmax(zones[g]))
    # zeros keep their order through the atomics: a row of +0.0 with one -0.0
    zz = np.zeros((2, 5000, 2), dtype=dt)
    zz[0, 4321, 0], zz[1, 17, 1] = -0.0, -0.0
    tz = ib(ctx.group_minmax_totals(torch.from_numpy(zz).to(DEV))).tolist()
    assert tz[0][0] < 0 and tz[0][1] == 0 and tz[1] == [0, 0] and same(np.array(tz, dtype=ib(zz).dtype).view(dt), host_minmax_totals(zz))
    none = ctx.group_minmax_totals(torch.empty((3, 0, 2), dtype=zones.dtype, device=DEV))
    assert ib(none).tolist() == [empty_record(dt)] * 3, "n_vectors == 0: {+inf, -inf} for every group"


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_select_key_min_max_count_where_group_by_key(ctx, dtype):
    """SELECT key, MIN(x), MAX(x), COUNT(*) WHERE lo <= a <= hi GROUP BY key"""
    f32 = dtype == "f32"
    nv = 230
    rng = np.random.default_rng(43)
    flags = rng.integers(0, 6, nv * 1024).astype(np.float32 if f32 else np.float64)
    flags[rng.random(flags.size) < 0.002] = NAN
    flags[rng.random(flags.size) < 0.002] = -0.0
    vals = datagen.mixed_column_f32(nv, seed=44) if f32 else datagen.mixed_column(nv, seed=44)
    other = datagen.drifting_column_f32(nv, seed=45) if f32 else datagen.drifting_column(nv, seed=45)
    ck, cv, ca = (ctx.encode(torch.from_numpy(t).to(DEV)) for t in (flags, vals, other))
    key, val, a = ctx.decode(ck), ctx.decode(cv), ctx.decode(ca)
    kn, vn, an = key.cpu().numpy(), val.cpu().numpy(), a.cpu().numpy()
    assert np.isnan(kn).any() and (np.signbit(kn) & (kn == 0)).any() and np.isnan(vn).any()
    a_lo, a_hi = bounds(a, 0.2, 0.7)
    keys = [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    mask = ctx.select_mask(ca, a_lo, a_hi)                                                     # WHERE
    counts = torch.empty((6, nv), dtype=torch.int32, device=DEV)
    zones = ctx.decode_group_minmax(cv, ck, mask, keys, keys, counts=counts)                   # GROUP BY key
    totals = ctx.group_minmax_totals(zones).cpu().numpy()                                      # MIN(x), MAX(x)
    n_rows = counts.sum(dim=1, dtype=torch.int64).cpu().numpy()                                # COUNT(*)
    where = (an >= a_lo) & (an <= a_hi)
    with np.errstate(invalid="ignore"):
        for g, k in enumerate(keys):
            sel = where & (kn == k)
            x = vn[sel]
            assert n_rows[g] == sel.sum() and 0 < n_rows[g] < where.sum()
            assert np.nanmin(x) != 0 and np.nanmax(x) != 0  # (the zeros' order cannot matter to numpy here)
            assert ib(totals[g]).tolist() == ib(np.array([np.nanmin(x), np.nanmax(x)])).tolist(), f"group {g}"
        assert n_rows.sum() == (where & ~np.isnan(kn)).sum(), "every selected row with a key that is a number falls in exactly one flag"


# ---- 8. determinism and statelessness -----------------------------------------------------------------------------------------------------------------
def test_the_same_calls_give_the_same_bytes(ctx):
    cv, val, ck, key = pair(ctx, "alp_rd")
    lo, hi = quantile_groups(key)
    mask = random_mask(cv.n_vectors, 51)
    runs = []
    for rep in range(2):
        torch.empty(1 << (20 + rep), dtype=torch.uint8, device=DEV).fill_(rep)  # (a different allocation history each time)
        zones, counts = run_masked(ctx, cv, mask)
        gz, gc = run_group(ctx, cv, ck, mask, lo, hi)
        totals = ctx.group_minmax_totals(gz)
        runs.append(tuple(t.cpu().numpy().tobytes() for t in (zones, counts, gz, gc, totals)))
    assert runs[0] == runs[1]


def test_minmax_calls_leave_the_decode_plan_alone(ctx):
    cols = [ctx.encode(torch.from_numpy(datagen.mixed_column(150, seed=s)).to(DEV)) for s in (96, 97)]
    ctx.column_totals(cols[0])  # one hinted, one not
    for col in cols:
        ctx.decode(col)
    ctx.synchronize()  # (what an unhinted decode learns about the column is in by now)
    before = [ctx.decode_plan(col) for col in cols]
    mask = random_mask(150, 52)
    ctx.decode_minmax_masked(cols[0], mask)
    ctx.decode_minmax_masked(cols[1], mask)
    zones = ctx.decode_group_minmax(cols[0], cols[1], mask, [0.0, 10.0], [10.0, 1e9])
    ctx.decode_group_minmax(cols[1], cols[1], mask, [0.0], [1e9])
    ctx.group_minmax_totals(zones)
    ctx.synchronize()
    assert [ctx.decode_plan(col) for col in cols] == before


# ---- 9. graph capture ---------------------------------------------------------------------------------------------------------------------------------
CAPTURE = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
import datagen
from alp_amd import capi
from minmax_replica import host_group_minmax, host_minmax_masked, host_minmax_totals
ctx = capi.Context(0)
side = torch.cuda.Stream()
ok = True
nv = 230
v0, v1 = datagen.mixed_column(nv, seed=81), datagen.rd_column(nv, seed=83, kind="latlon")
k0, k1 = datagen.drifting_column(nv, seed=82), datagen.mixed_column(nv, seed=84)
vd, kd = [torch.from_numpy(t).cuda() for t in (v0, v1)], [torch.from_numpy(t).cuda() for t in (k0, k1)]
colv, colk = ctx.encode(vd[0]), ctx.encode(kd[0])
s = np.sort(np.concatenate([k0, k1])[np.isfinite(np.concatenate([k0, k1]))])
q = lambda f: float(s[int(f * (s.size - 1))])
lo, hi = [q(0.0), q(0.2), q(0.5), q(0.5), q(0.9)], [q(0.2), q(0.5), q(1.0), q(0.5), q(0.1)]
lo0, hi0 = list(lo), list(hi)
G = len(lo)
prior = torch.from_numpy(np.random.default_rng(85).integers(0, 2**64, 16 * nv, dtype=np.uint64).view(np.int64)).cuda()
mask = torch.zeros(16 * nv, dtype=torch.int64, device="cuda:0")
zones = torch.zeros((nv, 2), dtype=torch.float64, device="cuda:0")
counts = torch.zeros(nv, dtype=torch.int32, device="cuda:0")
gz = torch.zeros((G, nv, 2), dtype=torch.float64, device="cuda:0")
gc = torch.zeros((G, nv), dtype=torch.int32, device="cuda:0")
totals = torch.zeros((G, 2), dtype=torch.float64, device="cuda:0")
def calls():
    # everything on the one stream: the graph is a chain, no parallel branches
    ctx.decode_minmax_masked(colv, mask, out=zones, counts=counts)
    ctx.decode_group_minmax(colv, colk, mask, lo, hi, out=gz, counts=gc)
    ctx.group_minmax_totals(gz, out=totals)
with torch.cuda.stream(side):
    mask.copy_(prior)
    calls()          # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        calls()
for i in range(G):   # the graph keeps the bounds it was captured with
    lo[i], hi[i] = -1e300, 1e300
def same(a, b):
    a = a.cpu().numpy()
    return a.shape == b.shape and np.array_equal(a.view(np.int64), np.ascontiguousarray(b).view(np.int64))
for rep in range(2):
    if rep == 1:
        ctx.encode(vd[1], colv); ctx.encode(kd[1], colk)    # other data encoded into the same buffers
        prior = ~prior
        prior[16 * 5:16 * 9] = 0
    torch.cuda.synchronize()
    mask.copy_(prior); zones.fill_(7.0); counts.fill_(7); gz.fill_(7.0); gc.fill_(7); totals.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    dv, dk = ctx.decode(colv), ctx.decode(colk)
    torch.cuda.synchronize()
    sh = torch.arange(64, dtype=torch.int64, device="cuda:0")
    bits = (((prior.reshape(-1, 1) >> sh) & 1) != 0).reshape(nv, 1024).cpu().numpy()
    vn, kn = dv.cpu().numpy().reshape(nv, 1024), dk.cpu().numpy().reshape(nv, 1024)
    want_z, want_c = host_minmax_masked(vn, bits)
    want_gz, want_gc = host_group_minmax(vn, kn, bits, lo0, hi0)
    ok = ok and torch.equal(mask, prior)
    ok = ok and same(zones, want_z) and np.array_equal(counts.cpu().numpy(), want_c)
    ok = ok and same(gz, want_gz) and np.array_equal(gc.cpu().numpy(), want_gc)
    ok = ok and same(totals, host_minmax_totals(want_gz))
    ok = ok and 0 < int(want_gc[1].sum()) < bits.sum() and int(want_gc[4].sum()) == 0
    print(rep, want_gc.sum(axis=1).tolist(), ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_inputs_change():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 10. argument checks ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c_argument_checks(ctx, dtype):
    cv, val, ck, key = pair(ctx, "alp_alp" if dtype == "f64" else "alp_alp_f32")
    short, _ = column(ctx, "every_width" if dtype == "f64" else "every_width_f32")  # another length
    nv = cv.n_vectors
    assert short.n_vectors != nv
    mm = getattr(capi.lib, "alpgpu_decode_minmax_masked_" + dtype)
    gm = getattr(capi.lib, "alpgpu_decode_group_minmax_" + dtype)
    tot = getattr(capi.lib, "alpgpu_group_minmax_totals_" + dtype)
    ft = ctypes.c_float if dtype == "f32" else ctypes.c_double
    tdt = torch.float32 if dtype == "f32" else torch.float64
    W = 4 if dtype == "f32" else 8
    lo, hi = (ft * 17)(*([0.0] * 17)), (ft * 17)(*([1e30] * 17))
    mask = torch.full((16 * nv + 16,), -1, dtype=torch.int64, device=DEV)
    zones = sentinel((17, nv + 1, 2), tdt)
    counts = torch.full((17, nv), 7, dtype=torch.int32, device=DEV)
    totals = sentinel((18, 2), tdt)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    V, K, S = ctypes.byref(cv.c), ctypes.byref(ck.c), ctypes.byref(short.c)
    M, Z, CO, T = p(mask), p(zones), p(counts), p(totals)
    bare = capi.CColumn()
    bare.n_vectors = nv  # a column without descriptors
    huge = capi.CColumn()
    huge.n_vectors = 2**60
    refused = [
        mm(None, V, M, Z, CO), mm(ctx.h, None, M, Z, CO), mm(ctx.h, V, None, Z, CO), mm(ctx.h, V, M, None, CO),
        mm(ctx.h, V, p(mask, 4), Z, CO), mm(ctx.h, V, M, p(zones, W), CO), mm(ctx.h, ctypes.byref(bare), M, Z, CO), mm(ctx.h, ctypes.byref(huge), M, Z, CO),
        gm(None, V, K, M, lo, hi, 2, Z, CO), gm(ctx.h, None, K, M, lo, hi, 2, Z, CO), gm(ctx.h, V, None, M, lo, hi, 2, Z, CO),
        gm(ctx.h, V, K, M, None, hi, 2, Z, CO), gm(ctx.h, V, K, M, lo, None, 2, Z, CO),
        gm(ctx.h, V, K, M, lo, hi, 0, Z, CO), gm(ctx.h, V, K, M, lo, hi, 17, Z, CO), gm(ctx.h, V, K, M, lo, hi, 2**32 - 1, Z, CO),
        gm(ctx.h, V, S, M, lo, hi, 2, Z, CO), gm(ctx.h, S, K, M, lo, hi, 2, Z, CO),
        gm(ctx.h, ctypes.byref(huge), ctypes.byref(huge), M, lo, hi, 2, Z, CO),
        gm(ctx.h, V, K, None, lo, hi, 2, Z, CO), gm(ctx.h, V, K, M, lo, hi, 2, None, CO), gm(ctx.h, V, K, p(mask, 4), lo, hi, 2, Z, CO),
        gm(ctx.h, V, K, M, lo, hi, 2, p(zones, W), CO),
        gm(ctx.h, ctypes.byref(bare), K, M, lo, hi, 2, Z, CO), gm(ctx.h, V, ctypes.byref(bare), M, lo, hi, 2, Z, CO),
        tot(None, Z, nv, 2, T), tot(ctx.h, None, nv, 2, T), tot(ctx.h, Z, nv, 2, None), tot(ctx.h, Z, nv, 0, T), tot(ctx.h, Z, nv, 17, T),
        tot(ctx.h, p(zones, W), nv, 2, T), tot(ctx.h, Z, nv, 2, p(totals, W // 2)), tot(ctx.h, Z, 2**60, 2, T), tot(ctx.h, None, 0, 0, T),
    ]
    assert refused == [-2] * len(refused), refused
    ctx.synchronize()
    assert bool((mask == -1).all()) and bool((zones == 7.0).all()) and bool((counts == 7).all()) and bool((totals == 7.0).all()), "a refused call wrote"
    # an empty column is fine and launches nothing; counts are optional; 16 groups are accepted; no vectors still reset the totals
    empty = capi.CColumn()
    assert mm(ctx.h, ctypes.byref(empty), None, None, None) == 0
    assert gm(ctx.h, ctypes.byref(empty), ctypes.byref(empty), None, lo, hi, 2, None, None) == 0
    assert gm(ctx.h, ctypes.byref(empty), ctypes.byref(empty), None, lo, hi, 0, None, None) == -2
    ctx.synchronize()
    assert bool((zones == 7.0).all()) and bool((counts == 7).all())
    assert mm(ctx.h, V, M, Z, None) == 0
    ctx.synchronize()
    flat = zones.reshape(-1, 2)
    assert bool((counts == 7).all()) and not bool((flat[:nv] == 7.0).any()) and bool((flat[nv:] == 7.0).all())
    zones.fill_(7.0)
    assert gm(ctx.h, V, K, M, lo, hi, 16, Z, None) == 0
    ctx.synchronize()
    flat = zones.reshape(-1, 2)
    assert bool((counts == 7).all()) and not bool((flat[:16 * nv] == 7.0).any()) and bool((flat[16 * nv:] == 7.0).all())
    assert tot(ctx.h, None, 0, 16, T) == 0
    ctx.synchronize()
    assert ib(totals[:16]).tolist() == [empty_record(np.float32 if dtype == "f32" else np.float64)] * 16 and bool((totals[16:] == 7.0).all())


def test_python_rejects_arguments_that_do_not_fit(ctx, monkeypatch):
    cv, val, ck, key = pair(ctx, "alp_alp")
    cf, _ = column(ctx, "mixed_f32")
    short, _ = column(ctx, "every_width")
    nv = cv.n_vectors
    mask = torch.full((16 * nv,), 7, dtype=torch.int64, device=DEV)
    zones = sentinel((nv, 2), torch.float64)
    gz = sentinel((2, nv, 2), torch.float64)
    counts = torch.full((nv,), 7, dtype=torch.int32, device=DEV)
    gc = torch.full((2, nv), 7, dtype=torch.int32, device=DEV)
    lo, hi = [0.0, 1.0], [1.0, 2.0]

    def unreachable(*a, **k):
        raise AssertionError("the library was called")
    for t in ("f64", "f32"):
        for stem in ("alpgpu_decode_minmax_masked_", "alpgpu_decode_group_minmax_", "alpgpu_group_minmax_totals_"):
            monkeypatch.setattr(capi.lib, stem + t, unreachable)
    wide = torch.full((32 * nv,), 7, dtype=torch.int64, device=DEV)
    bad_masks = (mask.to(torch.int32), mask.cpu(), mask[:-16], wide, wide[::2], mask.reshape(nv, 16), [1, 2, 3], np.zeros(16 * nv, np.int64))
    for bad in bad_masks:
        with pytest.raises(ValueError):
            ctx.decode_minmax_masked(cv, bad, out=zones, counts=counts)
        with pytest.raises(ValueError):
            ctx.decode_group_minmax(cv, ck, bad, lo, hi, out=gz, counts=gc)
    unaligned = torch.zeros(2 * nv + 1, dtype=torch.float64, device=DEV)[1:].reshape(nv, 2)
    for bad in (zones.to(torch.float32), zones.cpu(), zones[:-1], zones.reshape(-1), zones.t(), torch.zeros((nv, 3), dtype=torch.float64, device=DEV), unaligned):
        with pytest.raises(ValueError):
            ctx.decode_minmax_masked(cv, mask, out=bad)
    for bad in (counts.to(torch.int64), counts.cpu(), counts[:-1]):
        with pytest.raises(ValueError):
            ctx.decode_minmax_masked(cv, mask, out=zones, counts=bad)
    with pytest.raises(ValueError):
        ctx.decode_minmax_masked(cf, mask, out=zones)  # a float column's records are floats
    for other in (cf, short):  # another dtype, another length
        with pytest.raises(ValueError):
            ctx.decode_group_minmax(cv, other, mask, lo, hi)
        with pytest.raises(ValueError):
            ctx.decode_group_minmax(other, cv, mask, lo, hi)
    for blo, bhi in (([0.0], [1.0, 2.0]), ([], []), ([0.0] * 17, [1.0] * 17), (0.0, 1.0), (None, None)):
        with pytest.raises(ValueError):
            ctx.decode_group_minmax(cv, ck, mask, blo, bhi)
    unaligned3 = torch.zeros(4 * nv + 1, dtype=torch.float64, device=DEV)[1:].reshape(2, nv, 2)
    for bad in (gz.to(torch.float32), gz.cpu(), gz[:1], gz.reshape(-1, 2), sentinel((3, nv, 2), torch.float64), gz.transpose(0, 1), gz[:, ::2], unaligned3):
        with pytest.raises(ValueError):
            ctx.decode_group_minmax(cv, ck, mask, lo, hi, out=bad)
    for bad in (gc.to(torch.int64), gc.cpu(), gc[:1], gc.reshape(-1)):
        with pytest.raises(ValueError):
            ctx.decode_group_minmax(cv, ck, mask, lo, hi, out=gz, counts=bad)
    for bad in (gz.to(torch.int64), gz.cpu(), gz.reshape(-1, 2), sentinel((17, 4, 2), torch.float64), sentinel((0, 4, 2), torch.float64), sentinel((2, 4, 3), torch.float64), gz.transpose(0, 1),
                unaligned3, [1.0, 2.0]):
        with pytest.raises(ValueError):
            ctx.group_minmax_totals(bad)
    for bad in (sentinel((3, 2), torch.float64), sentinel((2, 2), torch.float32), sentinel((2, 2), torch.float64).cpu(), sentinel((4,), torch.float64)):
        with pytest.raises(ValueError):
            ctx.group_minmax_totals(gz, out=bad)
    ctx.synchronize()
    assert bool((mask == 7).all()) and bool((zones == 7.0).all()) and bool((gz == 7.0).all()) and bool((counts == 7).all()) and bool((gc == 7).all())


# ---- 11. the C++ wrapper ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cpp_column_minmax_against_decompress_and_a_host_loop(ctx, tmp_path, dtype):
    """include/alp/batch.hpp: alp::gpu::column<double / float>::minmax_masked, group_minmax_masked and group_minmax_totals of two serialized
    columns against column::decompress and a host loop over the definition of a record (tests/cpp/minmax_test.cpp)"""
    exe = tmp_path / "minmax_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/minmax_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    cv, val, ck, key = pair(ctx, "adversarial_rolled" if dtype == "f64" else "adversarial_rolled_f32")  # NaN, +-inf and -0.0 among the values and the keys
    n_values = val.numel()
    for name, col in (("val.blob", cv), ("key.blob", ck)):
        ctx.to_blob(col, n_values).tofile(str(tmp_path / name))
    mask = vectors_cleared(random_mask(cv.n_vectors, 53), 3, -1)
    mask[16:32] = 0
    mask.cpu().numpy().tofile(str(tmp_path / "in.mask"))
    lo, hi = quantile_groups(key)
    np.asarray(lo + hi, dtype=np.float32 if dtype == "f32" else np.float64).tofile(str(tmp_path / "bounds.bin"))
    p = subprocess.run([str(exe), dtype] + [str(tmp_path / f) for f in ("val.blob", "key.blob", "in.mask", "bounds.bin")], capture_output=True, text=True, timeout=600)
    line = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("ok ")]
    assert p.returncode == 0 and len(line) == 1, p.stdout[-3000:] + p.stderr[-2000:]
    assert int(line[0][1]) == cv.n_vectors and int(line[0][2]) == len(lo) and int(line[0][3]) > cv.n_vectors
