"""GPU: zone maps (include/alpgpu.h, "zone maps": alpgpu_zone_map_*, alpgpu_zone_map_of_values_*, alpgpu_zones_minmax_*,
alpgpu_select_range_zoned_*).  As in test_select_gpu.py the expected result never comes from the code under test: it is computed from the store
decode x = ctx.decode(col), which other suites pin to the oracle and the reference.  Expected record of a vector = minimum / maximum of the
order-preserving integer key (b if b >= 0 else b ^ INT_MAX on the int64 / int32 view) over the values of its 1024-block that are not NaN, mapped
back to bits, {+inf, -inf} where there is none; compared on integer views, so that -0.0 and +0.0 differ.  The expected selection is
nonzero((x >= lo) & (x <= hi)) on the decoded column, and the zoned call is compared with the plain call as well."""
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


def fbits(b):
    return b.view(torch.float64 if b.dtype == torch.int64 else torch.float32)


def int_max(dtype):
    return torch.iinfo(dtype).max


def key(b):
    """the order-preserving key of value bits: ascending keys = ascending values, -0.0 below +0.0; its own inverse"""
    return torch.where(b >= 0, b, b ^ int_max(b.dtype))


def reduce_keys(x_min, x_max):
    """(min bits, max bits) along the last axis over the entries that are not NaN; {+inf, -inf} where there is none"""
    bmin, bmax = ibits(x_min), ibits(x_max)
    top = int_max(bmin.dtype)
    kmin = torch.where(torch.isnan(x_min), torch.full_like(bmin, top), key(bmin)).min(dim=-1).values
    kmax = torch.where(torch.isnan(x_max), torch.full_like(bmax, -top - 1), key(bmax)).max(dim=-1).values
    pinf = ibits(torch.tensor([INF], dtype=x_min.dtype, device=x_min.device))[0]
    ninf = ibits(torch.tensor([-INF], dtype=x_min.dtype, device=x_min.device))[0]
    lo = torch.where(kmin == top, pinf, key(kmin))
    hi = torch.where(kmax == -top - 1, ninf, key(kmax))
    return lo, hi


def expected_zones(dec):
    """[n_vectors, 2] record bits of a decoded column"""
    blocks = dec.reshape(-1, 1024)
    lo, hi = reduce_keys(blocks, blocks)
    return torch.stack([lo, hi], dim=1)


def expected_minmax(zones):
    """[2] bits: the reduction of a zone map"""
    if zones.shape[0] == 0:
        return ibits(torch.tensor([INF, -INF], dtype=zones.dtype, device=zones.device))
    lo, hi = reduce_keys(zones[:, 0].contiguous(), zones[:, 1].contiguous())
    return torch.stack([lo, hi])


def encoded(ctx, x):
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return ctx.encode(xd), xd


def check_zones(ctx, col, dec, what, raw=None):
    """zone_map(col) against the decoded column; zone_map_of_values(raw) the same bytes; column_minmax the reduction; -> the zone map"""
    want = expected_zones(dec)
    z = ctx.zone_map(col)
    ctx.synchronize()
    assert z.shape == (col.n_vectors, 2) and z.dtype == dec.dtype
    bad = torch.nonzero((ibits(z) != want).any(dim=1)).reshape(-1)
    assert bad.numel() == 0, f"{what}: {bad.numel()} records differ, first vector {int(bad[0])}: got {z[bad[0]].tolist()} bits {ibits(z)[bad[0]].tolist()}, expected {fbits(want)[bad[0]].tolist()} bits {want[bad[0]].tolist()}"
    if raw is not None:
        zv = ctx.zone_map_of_values(raw)
        assert torch.equal(ibits(zv), want), f"{what}: zone_map_of_values differs from zone_map of the encoded column"
    mm = ctx.column_minmax(z)
    assert torch.equal(ibits(mm), expected_minmax(z)), f"{what}: column_minmax {mm.tolist()}"
    return z


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
    **{f"decimal_f32_{d}": (lambda d=d: datagen.decimal_column_f32(130, decimals=d, hi=10.0 ** (7 - d), seed=20 + d)) for d in (0, 2, 4)},
}


# ---- column generators for the zoned selection (sorted / clustered data is where a zone map excludes vectors) ---------------------------------
def sorted_column(n_vectors, seed, dtype=np.float64):
    """ascending decimals: every vector covers its own narrow interval"""
    rng = np.random.default_rng(seed)
    if dtype == np.float64:
        return np.sort(np.round(rng.uniform(-1e5, 1e5, n_vectors * 1024), 2))
    return np.sort(np.round(rng.uniform(0.0, 1e4, n_vectors * 1024), 1).astype(np.float32))


def clustered_column(n_vectors, seed, dtype=np.float64):
    """each rowgroup of 100 vectors around a level of its own, the levels in random order; a few exceptions and specials"""
    rng = np.random.default_rng(seed)
    n_rg = (n_vectors + 99) // 100
    levels = rng.permutation(n_rg).astype(np.float64) * 50.0
    x = np.round(rng.uniform(0.0, 40.0, n_vectors * 1024), 2) + np.repeat(levels, 100 * 1024)[:n_vectors * 1024]
    x = np.round(x, 2)
    m = rng.random(x.size) < 0.002
    x[m] = x[m] * np.pi / 3.0
    x[rng.integers(0, x.size, 40)] = np.nan
    x[rng.integers(0, x.size, 10)] = -0.0
    return x.astype(dtype)


def sorted_rd_column(n_vectors, seed):
    """ascending full-precision doubles: ALP_RD vectors with narrow intervals"""
    return np.sort(np.random.default_rng(seed).random(n_vectors * 1024))


def battery(x, specials):
    """test_select_gpu.py's predicates, from the column's own finite decoded values"""
    xs = x.cpu().numpy()
    s = np.sort(xs[np.isfinite(xs)])
    q = lambda f: float(s[min(s.size - 1, int(f * s.size))])
    preds = [("everything", -INF, INF), ("middle band", q(0.3), q(0.7)), ("narrow band", q(0.5), q(0.502)), ("point", q(0.41), q(0.41)),
             ("lo > hi", q(0.7), q(0.3)), ("nan lo", NAN, q(0.7)), ("nan hi", q(0.3), NAN), ("low tail", -INF, q(0.1)), ("high tail", q(0.9), INF)]
    if specials:
        preds += [("zero", 0.0, 0.0), ("negative zero", -0.0, -0.0), ("+inf", INF, INF), ("-inf", -INF, -INF)]
    return preds


def expected(x, lo, hi, first=0, n=None):
    n = x.numel() - first if n is None else n
    m = (x >= lo) & (x <= hi)
    m[:first] = False
    m[first + n:] = False
    idx = torch.nonzero(m).reshape(-1)
    return idx, ibits(x)[idx]


CANARY, PAD = 0x5A5A5A5A, 64


def check_zoned_select(ctx, col, x, zones, lo, hi, first=0, n=None, what="", plain_col=None):
    """the zoned selection against the decoded column x AND against the plain selection (of plain_col, default col): indices + values, indices alone,
    count only (capacity 0) and a truncating capacity; -> the number selected"""
    want_idx, want_bits = expected(x, lo, hi, first, n)
    tag = f"{what} [{lo!r}, {hi!r}] first={first} n={n}"
    p_idx, p_vals = ctx.select_range(col if plain_col is None else plain_col, lo, hi, first=first, n=n, values=True)
    idx, vals = ctx.select_range(col, lo, hi, first=first, n=n, values=True, zones=zones)
    assert idx.numel() == want_idx.numel() == p_idx.numel(), f"{tag}: {idx.numel()} selected, expected {want_idx.numel()}, plain {p_idx.numel()}"
    assert torch.equal(idx, want_idx) and torch.equal(idx, p_idx), f"{tag}: indices differ"
    assert torch.equal(ibits(vals), want_bits) and torch.equal(ibits(vals), ibits(p_vals)), f"{tag}: values differ"
    only = ctx.select_range(col, lo, hi, first=first, n=n, zones=zones)
    assert torch.equal(only, want_idx), f"{tag}: indices without values differ"
    full = want_idx.numel()
    count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    ctx.select_range_into(col, lo, hi, None, count, first=first, n=n, zones=zones)
    assert int(count) == full, f"{tag}: count-only {int(count)} != {full}"
    if full > 1:
        cap = full // 2
        tidx = torch.full((cap + PAD,), CANARY, dtype=torch.int64, device=DEV)
        tvals = torch.empty(cap + PAD, dtype=x.dtype, device=DEV)
        ibits(tvals).fill_(CANARY)
        ctx.select_range_into(col, lo, hi, tidx[:cap], count, tvals[:cap], first=first, n=n, zones=zones)
        assert int(count) == full and torch.equal(tidx[:cap], want_idx[:cap]) and torch.equal(ibits(tvals)[:cap], want_bits[:cap]), f"{tag}: truncated to {cap}"
        assert bool((tidx[cap:] == CANARY).all()) and bool((ibits(tvals)[cap:] == CANARY).all()), f"{tag}: written behind the capacity {cap}"
    return full


def zone_variants(zones, seed):
    """exact records, records widened by random amounts, and {-inf, +inf} everywhere: each contains every vector's true interval"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    span = float(torch.nan_to_num(zones, nan=0.0, posinf=0.0, neginf=0.0).abs().max()) + 1.0
    grow = torch.rand(zones.shape, generator=g, device=DEV, dtype=torch.float64) * torch.tensor([0.0, 1e-6, 1e-3, 1.0], device=DEV, dtype=torch.float64)[
        torch.randint(0, 4, (zones.shape[0], 1), generator=g, device=DEV)] * span
    wide = torch.stack([(zones[:, 0].double() - grow[:, 0]), (zones[:, 1].double() + grow[:, 1])], dim=1)
    if zones.dtype == torch.float32:  # round outwards
        lo32, hi32 = wide[:, 0].float(), wide[:, 1].float()
        lo32 = torch.where(lo32.double() > wide[:, 0], torch.nextafter(lo32, torch.full_like(lo32, -INF)), lo32)
        hi32 = torch.where(hi32.double() < wide[:, 1], torch.nextafter(hi32, torch.full_like(hi32, INF)), hi32)
        wide = torch.stack([lo32, hi32], dim=1)
    wide = wide.to(zones.dtype).contiguous()
    # an empty record {+inf, -inf} stays as it is (inf - r = inf), every other one only grew
    assert bool(((wide[:, 0] <= zones[:, 0]) & (wide[:, 1] >= zones[:, 1]))[zones[:, 0] <= zones[:, 1]].all())
    everything = torch.empty_like(zones)
    everything[:, 0], everything[:, 1] = -INF, INF
    return (("exact", zones), ("widened", wide), ("everything", everything))


RANGES = lambda total: [(3 * 1024 + 17, 500), (5 * 1024 - 100, 300), (1, total - 1), (1023, 2), (total - 1, 1), (777, 0), (40 * 1024 + 5, 61 * 1024 + 900)]


def check_zoned_battery(ctx, col, x, what, specials=False, seed=1):
    zones = check_zones(ctx, col, x, what)
    total = x.numel()
    preds = battery(x, specials)
    some = False
    for zname, z in zone_variants(zones, seed):
        for name, lo, hi in preds:
            k = check_zoned_select(ctx, col, x, z, lo, hi, what=f"{what}/{zname}/{name}")
            some = some or 0 < k < total
        for first, n in RANGES(total):
            for name, lo, hi in (preds[1], preds[2], preds[0]):
                check_zoned_select(ctx, col, x, z, lo, hi, first, n, what=f"{what}/{zname}/{name}")
    assert some, f"{what}: no predicate selects some but not all values"
    return zones


# ---- 1, 2: the zone map against the store decode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(DOUBLE_COLUMNS) + sorted(FLOAT_COLUMNS))
def test_zone_map_of_every_column_kind_against_the_store_decode(ctx, name):
    x = (DOUBLE_COLUMNS.get(name) or FLOAT_COLUMNS[name])()
    col, xd = encoded(ctx, x)
    dec = ctx.decode(col)
    assert torch.equal(ibits(dec), ibits(xd)), f"{name}: decode(encode(x)) != x"
    z = check_zones(ctx, col, dec, name, raw=xd)
    schemes = set(col.to_host()[1]["scheme"].tolist())
    if name.startswith("rd_"):
        assert capi.SCHEME_ALP_RD in schemes
    if name.startswith("mixed"):
        assert capi.SCHEME_ALP in schemes and bool(torch.isnan(dec).any()) and bool(torch.isinf(z).any())


def test_golden_vectors_and_rowgroups_encoded_by_the_oracle(ctx, oracle):
    from oracle.pyoracle import OracleF32
    for name, x, _, _ in golden_io.first_vectors():
        col = capi.DeviceColumn.from_host(*layout.compact(oracle.encode_column(x)))
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(torch.from_numpy(x.copy()).to(DEV))), name
        check_zones(ctx, col, dec, name, raw=torch.from_numpy(x.copy()).to(DEV))
    for name, x, _ in golden_io.rowgroup_samples():
        col = capi.DeviceColumn.from_host(*layout.compact(oracle.encode_column(x)))
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(torch.from_numpy(x.copy()).to(DEV))), name
        check_zones(ctx, col, dec, "rowgroup " + name, raw=torch.from_numpy(x.copy()).to(DEV))
    of = OracleF32()
    for name, x, _, _ in golden_io.float_vectors():
        col = capi.DeviceColumn.from_host(*layout.compact(of.encode_column(x), 4), dtype="f32")
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(torch.from_numpy(x.copy()).to(DEV))), name
        check_zones(ctx, col, dec, name, raw=torch.from_numpy(x.copy()).to(DEV))


def test_columns_encoded_unordered_and_loaded_from_a_blob(ctx):
    x = np.concatenate([datagen.mixed_column(150, seed=31), datagen.rd_column(120, seed=32)])
    ctx.set_option(10, 1)  # ALPGPU_OPT_ENCODE_UNORDERED: records out of vector order
    try:
        col, xd = encoded(ctx, x)
        ctx.synchronize()
    finally:
        ctx.set_option(10, 0)
    check_zones(ctx, col, ctx.decode(col), "unordered", raw=xd)
    for dt, xx in (("f64", x), ("f32", np.concatenate([datagen.mixed_column_f32(170, seed=33), datagen.rd_column_f32(100, seed=34)]))):
        c0, xd = encoded(ctx, xx)
        bcol, nv = ctx.from_blob(ctx.to_blob(c0, xx.size))
        assert nv == xx.size and bcol.dtype == dt
        check_zones(ctx, bcol, ctx.decode(bcol), "from_blob " + dt, raw=xd)


def _types(dtype):
    return (np.float64, np.uint64, np.int64) if dtype == "f64" else (np.float32, np.uint32, np.int32)


def nan_patterns(dtype):
    """quiet and SIGNALLING NaNs with non-zero payloads, both signs, as bit patterns"""
    if dtype == "f64":
        return {"quiet": 0x7FF8000000000123, "quiet negative": 0xFFF8000000000456, "signalling": 0x7FF0000000000001, "signalling negative": 0xFFF4000000000ABC,
                "signalling wide": 0x7FF7FFFFFFFFFFFF}
    return {"quiet": 0x7FC00123, "quiet negative": 0xFFC00456, "signalling": 0x7F800001, "signalling negative": 0xFFA00ABC, "signalling wide": 0x7FBFFFFF}


def is_signalling(bits, dtype):
    quiet_bit = 1 << (51 if dtype == "f64" else 22)
    return not bits & quiet_bit


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_hand_made_vectors(ctx, dtype):
    F, U, I = _types(dtype)
    base = np.round(np.random.default_rng(3).uniform(1, 100, 1024), 2).astype(F)
    one = lambda a: (float(a[0]), float(a[1]))
    sign = lambda v: math.copysign(1.0, v)

    def zone_of(x, what, want_scheme=None):
        col, xd = encoded(ctx, x)
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(xd)), f"{what}: decode(encode(x)) != x"
        vec = col.to_host()[1]
        if want_scheme is not None:
            assert set(vec["scheme"].tolist()) == {want_scheme}, f"{what}: scheme {set(vec['scheme'].tolist())}"
        return check_zones(ctx, col, dec, what, raw=xd).cpu().numpy(), vec

    # both zeros as the minimum: min = -0.0 (sign bit set); as the maximum: max = +0.0
    a = base.copy(); a[17] = 0.0; a[400] = -0.0; a[900] = 0.0
    z, _ = zone_of(a, "zeros as minimum")
    assert z[0, 0] == 0.0 and sign(z[0, 0]) == -1.0 and z[0, 1] == a.max()
    a = -base.copy(); a[17] = -0.0; a[400] = 0.0; a[900] = -0.0
    z, _ = zone_of(a, "zeros as maximum")
    assert z[0, 1] == 0.0 and sign(z[0, 1]) == 1.0 and z[0, 0] == a.min()
    a = base.copy(); a[5] = -0.0  # -0.0 alone: it is the minimum, and +0.0 is not invented
    z, _ = zone_of(a, "negative zero alone")
    assert z[0, 0] == 0.0 and sign(z[0, 0]) == -1.0
    a = np.zeros(1024, F); a[::3] = -0.0
    z, _ = zone_of(a, "only zeros")
    assert sign(z[0, 0]) == -1.0 and sign(z[0, 1]) == 1.0 and z[0, 0] == 0.0 and z[0, 1] == 0.0
    # +-inf are ordinary values
    a = base.copy(); a[1023] = np.inf; a[0] = -np.inf
    z, _ = zone_of(a, "inf ends")
    assert one(z[0]) == (-INF, INF)
    a = base.copy(); a[77] = np.inf
    z, _ = zone_of(a, "+inf only")
    assert one(z[0]) == (float(base[np.arange(1024) != 77].min()), INF)
    # quiet and signalling NaNs with payloads in an ALP exception record next to finite values: the zone is the finite values'
    pats = nan_patterns(dtype)
    a = base.copy()
    bits = a.view(U)
    where = {}
    for j, (pname, pat) in enumerate(pats.items()):
        for p in (3 + 64 * j, 1023 - 5 * j):
            bits[p] = pat
            where[p] = pat
    finite = np.ones(1024, bool); finite[list(where)] = False
    col, xd = encoded(ctx, a)
    dec = ctx.decode(col)
    vec = col.to_host()[1]
    assert int(vec["scheme"][0]) == capi.SCHEME_ALP and int(vec["exc_cnt"][0]) >= len(where), "the NaNs must sit in an ALP exception record"
    got = dec.cpu().numpy().view(U)
    assert all(int(got[p]) == pat for p, pat in where.items()), "a NaN payload (signalling ones included) did not survive encode + decode"
    assert any(is_signalling(pat, dtype) for pat in where.values())
    z = check_zones(ctx, col, dec, "NaNs in an ALP exception record", raw=xd).cpu().numpy()
    assert one(z[0]) == (float(base[finite].min()), float(base[finite].max()))
    # the same in ALP_RD vectors (the NaN lies in the packed words / the left dictionary's exceptions)
    rd = (datagen.rd_column(100, seed=41) if dtype == "f64" else datagen.rd_column_f32(100, seed=41)).astype(F)
    rb = rd.view(U)
    planted = {}
    for j, (pname, pat) in enumerate(pats.items()):
        for p in (7 * 1024 + 11 + j, 8 * 1024 + 1000 - j, (20 + j) * 1024 + 512):
            rb[p] = pat
            planted[p] = pat
    col, xd = encoded(ctx, rd)
    dec = ctx.decode(col)
    vec = col.to_host()[1]
    assert all(int(vec["scheme"][p >> 10]) == capi.SCHEME_ALP_RD for p in planted), "the vectors holding the NaNs must be ALP_RD"
    got = dec.cpu().numpy().view(U)
    assert all(int(got[p]) == pat for p, pat in planted.items()), "a NaN payload did not survive the ALP_RD encode + decode"
    z = check_zones(ctx, col, dec, "NaNs in ALP_RD vectors", raw=xd).cpu().numpy()
    for v in sorted({p >> 10 for p in planted}):
        blk = rd[v * 1024:(v + 1) * 1024]
        ok = ~np.isnan(blk)
        assert ok.sum() >= 1019 and one(z[v]) == (float(blk[ok].min()), float(blk[ok].max())), f"ALP_RD vector {v}"
    # crafted records on the plain vector's descriptor: 1024 exceptions (finite), and 1024 NaN exceptions of every pattern = a vector of NaNs only
    src, _ = encoded(ctx, base)
    rg, vec, packed, _ = src.to_host()
    assert int(vec["scheme"][0]) == capi.SCHEME_ALP
    vec = vec.copy()
    vec["exc_cnt"][0], vec["exc_off"][0] = 1024, 0
    vals = (np.arange(1024) * 0.37 - 100.0).astype(F)
    vals[300], vals[301] = 0.0, -0.0
    nans = np.array([list(pats.values())[i % len(pats)] for i in range(1024)], dtype=U).view(F)
    for what, v, want in (("1024 exceptions", vals, (float(vals.min()), float(vals.max()))), ("1024 NaN exceptions", nans, (INF, -INF))):
        rec = np.concatenate([v.view(np.uint8), np.arange(1024, dtype=np.uint16).view(np.uint8)])
        col = capi.DeviceColumn.from_host(rg, vec, packed, rec, dtype=dtype)
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(torch.from_numpy(v).to(DEV))), what
        z = check_zones(ctx, col, dec, what, raw=dec).cpu().numpy()
        assert one(z[0]) == want, what
    # an all-NaN vector through the encoder, between ordinary vectors
    a = np.concatenate([base, np.full(1024, np.nan, F), base + 1])
    col, xd = encoded(ctx, a)
    dec = ctx.decode(col)
    assert bool(torch.isnan(dec[1024:2048]).all())
    z = check_zones(ctx, col, dec, "a vector of NaNs", raw=xd).cpu().numpy()
    assert one(z[1]) == (INF, -INF) and one(z[0]) == (float(base.min()), float(base.max()))
    mm = ctx.column_minmax(ctx.zone_map(col)).cpu().numpy()
    assert one(mm) == (float(base.min()), float(base.max() + 1))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_column_minmax_of_two_million_records_and_of_none(ctx, dtype):
    """the reduction alone: more records than one pass of workgroups covers at a stride of one; zeros of both signs, infinities, empty records"""
    g = torch.Generator(device=DEV).manual_seed(5)
    n = (1 << 21) + 5
    a = (torch.rand((n, 2), generator=g, device=DEV, dtype=torch.float64) - 0.5) * 2e6
    z = torch.stack([a.min(dim=1).values, a.max(dim=1).values], dim=1).to(dtype).contiguous()
    mm = ctx.column_minmax(z)
    assert torch.equal(ibits(mm), expected_minmax(z)) and float(mm[0]) == float(z[:, 0].min()) and float(mm[1]) == float(z[:, 1].max())
    z[12345, 0], z[12345, 1] = INF, -INF  # an empty record changes nothing
    z[n - 1, 0], z[n - 1, 1] = -INF, INF
    mm = ctx.column_minmax(z)
    assert mm.tolist() == [-INF, INF]
    zz = torch.zeros((5000, 2), dtype=dtype, device=DEV)
    zz[:, 0] = 0.0
    zz[4000, 0] = -0.0
    zz[:, 1] = -0.0
    zz[77, 1] = 0.0
    mm = ctx.column_minmax(zz)
    assert torch.equal(ibits(mm), expected_minmax(zz)) and math.copysign(1, float(mm[0])) == -1.0 and math.copysign(1, float(mm[1])) == 1.0
    neg = -torch.rand((3000, 2), generator=g, device=DEV, dtype=torch.float64).to(dtype) - 1.0  # negative values only: the other atomic of each pair
    neg = torch.stack([neg.min(dim=1).values, neg.max(dim=1).values], dim=1).contiguous()
    assert torch.equal(ibits(ctx.column_minmax(neg)), expected_minmax(neg))
    empty = torch.empty((0, 2), dtype=dtype, device=DEV)
    assert ctx.column_minmax(empty).tolist() == [INF, -INF]
    allnan = torch.empty((300, 2), dtype=dtype, device=DEV)
    allnan[:, 0], allnan[:, 1] = INF, -INF
    assert ctx.column_minmax(allnan).tolist() == [INF, -INF]
    out = torch.full((4,), 7.0, dtype=dtype, device=DEV)
    ctx.column_minmax(z[:1000], out=out)
    assert out[2:].tolist() == [7.0, 7.0]


# ---- 3: zoned select == plain select == the decoded column -----------------------------------------------------------------------------------
ZONED_COLUMNS = {
    "mixed": (lambda: datagen.mixed_column(250, seed=5), True),
    "rd_unit": (lambda: datagen.rd_column(250, seed=6), False),
    "every_width_exc": (lambda: datagen.every_bit_width_column(208, seed=9, exceptions=True), False),
    "adversarial": (lambda: np.tile(adversarial_column(datagen.adversarial_vectors()), 11), True),
    "mixed_f32": (lambda: datagen.mixed_column_f32(250, seed=5), True),
    "rd_unit_f32": (lambda: datagen.rd_column_f32(250, seed=6), False),
    "sorted": (lambda: sorted_column(1200, seed=51), False),
    "clustered": (lambda: clustered_column(1200, seed=52), True),
    "sorted_rd": (lambda: sorted_rd_column(300, seed=53), False),
    "sorted_f32": (lambda: sorted_column(300, seed=54, dtype=np.float32), False),
    "clustered_f32": (lambda: clustered_column(300, seed=55, dtype=np.float32), True),
}


@pytest.mark.parametrize("name", sorted(ZONED_COLUMNS))
def test_zoned_select_equals_plain_select(ctx, name):
    make, specials = ZONED_COLUMNS[name]
    x = make()
    col, xd = encoded(ctx, x)
    dec = ctx.decode(col)
    assert torch.equal(ibits(dec), ibits(xd)), f"{name}: decode(encode(x)) != x"
    assert col.n_vectors >= 102
    zones = check_zoned_battery(ctx, col, dec, name, specials=specials, seed=len(name))
    vec = col.to_host()[1]
    if name == "sorted_rd":
        assert set(vec["scheme"].tolist()) == {capi.SCHEME_ALP_RD}
    if name.startswith("sorted"):  # the zones of a sorted column do exclude: for the narrow band nearly every vector
        s = np.sort(x)
        lo, hi = float(s[int(0.5 * s.size)]), float(s[int(0.502 * s.size)])
        out = ~((zones[:, 1] >= lo) & (zones[:, 0] <= hi))
        assert int(out.sum()) >= col.n_vectors - 5, f"{name}: {int(out.sum())} of {col.n_vectors} vectors excluded"


# ---- 4: the skipping is real -----------------------------------------------------------------------------------------------------------------
def scrambled_copy(col, which):
    """a copy of the column in buffers of its own with the packed words of the vectors `which` (bool per vector) overwritten — inside each vector's own
    extent of the stream; descriptors, offsets and exception records untouched, so every access of a decode stays in bounds"""
    rg, vec, packed, exc = col.to_host()
    packed = packed.copy()
    rng = np.random.default_rng(9)
    touched = 0
    for v in np.nonzero(which)[0]:
        off = int(vec["packed_off"][v])
        size = 128 * int(vec["bw"][v]) + (128 * int(vec["lbw"][v]) if vec["scheme"][v] == capi.SCHEME_ALP_RD else 0)
        end = int(vec["packed_off"][v + 1]) if v + 1 < vec.size else packed.size
        assert 0 <= off and off + size <= min(end, packed.size) or size == 0
        packed[off:off + size] = rng.integers(0, 256, size, dtype=np.uint8)
        touched += size > 0
    return capi.DeviceColumn.from_host(rg.copy(), vec.copy(), packed, exc.copy(), dtype=col.dtype), touched


def test_excluded_and_contained_vectors_are_not_decoded(ctx):
    V = 1200
    x = sorted_column(V, seed=61)
    col, xd = encoded(ctx, x)
    ctx.synchronize()
    dec = ctx.decode(col)
    assert torch.equal(ibits(dec), ibits(xd))
    zones = check_zones(ctx, col, dec, "sorted")
    vec = col.to_host()[1]
    # excluded: a predicate spanning values of two adjacent vectors; in a sorted column only their neighbours can share a bound
    lo, hi = float(dec[600 * 1024 + 1000]), float(dec[601 * 1024 + 20])
    out = (~((zones[:, 1] >= lo) & (zones[:, 0] <= hi))).cpu().numpy()
    assert V >= 1000 and int(out.sum()) >= V - 3, f"{int(out.sum())} of {V} vectors excluded"
    scr, touched = scrambled_copy(col, out)
    assert touched >= V - 3
    sdec = ctx.decode(scr)
    changed = (ibits(sdec).reshape(V, 1024) != ibits(dec).reshape(V, 1024)).any(dim=1).cpu().numpy()
    assert changed[out].sum() >= V - 3 and not changed[~out].any(), "the overwritten words must change what a decode of those vectors gives, and nothing else"
    assert ctx.select_range(scr, lo, hi).numel() == expected(sdec, lo, hi)[0].numel()  # (the plain call does read them)
    k = check_zoned_select(ctx, scr, dec, zones, lo, hi, what="excluded vectors overwritten", plain_col=col)
    assert 45 <= k <= 3 * 1024  # (positions 1000 .. 1023 of vector 600 and 0 .. 20 of vector 601, plus equal values beside them)
    check_zoned_select(ctx, scr, dec, zones, lo, hi, 600 * 1024 + 1010, 900, what="excluded vectors overwritten", plain_col=col)
    # contained: exception-free ALP vectors wholly inside a wide predicate are counted, and their indices written, without their words
    lo, hi = float(dec[100 * 1024]), float(dec[1100 * 1024 + 1023])
    inside = ((zones[:, 0] >= lo) & (zones[:, 1] <= hi)).cpu().numpy() & (vec["scheme"] == capi.SCHEME_ALP) & (vec["exc_cnt"] == 0)
    assert int(inside.sum()) >= 900, f"{int(inside.sum())} contained exception-free ALP vectors"
    scr, touched = scrambled_copy(col, inside)
    assert touched >= 900
    sdec = ctx.decode(scr)
    assert int((ibits(sdec).reshape(V, 1024) != ibits(dec).reshape(V, 1024)).any(dim=1).sum()) >= 900
    # (overwritten digits stay within the vector's bit width, so most of them still decode to values inside [lo, hi]: what shows that the words are
    #  not read is that the INDICES-ONLY emit and the count need no decode, while every decode of these vectors now gives other values — above)
    for first, n in ((0, None), (150 * 1024 + 3, 700 * 1024 + 100)):
        w_idx, _ = expected(dec, lo, hi, first, n)
        count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
        ctx.select_range_into(scr, lo, hi, None, count, first=first, n=n, zones=zones)
        assert int(count) == w_idx.numel(), "count-only over contained vectors"
        assert torch.equal(ctx.select_range(scr, lo, hi, first=first, n=n, zones=zones), w_idx), "indices-only over contained vectors"


# ---- 5: stateless and capturable --------------------------------------------------------------------------------------------------------------
def test_zone_calls_leave_the_decode_plan_alone(ctx):
    for hinted in (True, False):
        col, _ = encoded(ctx, datagen.mixed_column(150, seed=91))
        if hinted:
            ctx.column_totals(col)
        ctx.decode(col)
        ctx.synchronize()  # (what an unhinted decode learns about the column is in by now)
        before = ctx.decode_plan(col)
        z = ctx.zone_map(col)
        ctx.column_minmax(z)
        ctx.select_range(col, -5.0, 5.0, values=True, zones=z)
        ctx.select_range(col, -INF, INF, first=5, n=9999, zones=z)
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
for dtype, x, y in (("f64", np.sort(datagen.mixed_column(230, seed=81)), datagen.mixed_column(230, seed=83)),
                    ("f32", np.sort(datagen.mixed_column_f32(230, seed=82)), datagen.mixed_column_f32(230, seed=84))):
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    col = ctx.encode(xd)
    other = ctx.encode(yd)
    s = x[np.isfinite(x)]
    t = x[~np.isnan(x)]
    lo, hi = float(s[s.size // 4]), float(s[s.size // 2])
    cap = 200 * 1024
    idx = torch.zeros(cap, dtype=torch.int64, device="cuda:0")
    vals = torch.zeros(cap, dtype=xd.dtype, device="cuda:0")
    fetched = torch.zeros(cap, dtype=xd.dtype, device="cuda:0")
    count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    zones = torch.zeros((col.n_vectors, 2), dtype=xd.dtype, device="cuda:0")
    mm = torch.zeros(2, dtype=xd.dtype, device="cuda:0")
    scratch = ctx.select_scratch(col)
    def work():
        ctx.zone_map(col, out=zones)
        ctx.column_minmax(zones, out=mm)
        ctx.select_range_into(col, lo, hi, idx, count, vals, first=1000, n=220 * 1024, scratch=scratch, zones=zones)
        ctx.gather(other, idx, out=fetched)
    with torch.cuda.stream(side):
        work()                            # warm-up on the capture stream
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            work()
    iv = torch.int64 if dtype == "f64" else torch.int32
    dec, dother = ctx.decode(col), ctx.decode(other)
    m = (dec >= lo) & (dec <= hi); m[:1000] = False; m[1000 + 220 * 1024:] = False
    w_idx = torch.nonzero(m).reshape(-1)
    e_zones = ctx.zone_map(col)
    e_idx, e_vals = ctx.select_range(col, lo, hi, first=1000, n=220 * 1024, values=True, zones=e_zones)
    torch.cuda.synchronize()
    for rep in range(2):
        idx.zero_(); vals.zero_(); fetched.zero_(); count.zero_(); zones.zero_(); mm.zero_(); scratch.fill_(rep)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        k = int(count)
        ok = ok and 0 < k <= cap and k == e_idx.numel() == w_idx.numel() and torch.equal(idx[:k], e_idx) and torch.equal(e_idx, w_idx)
        ok = ok and torch.equal(vals[:k].view(iv), e_vals.view(iv)) and torch.equal(e_vals.view(iv), dec[w_idx].view(iv)) and bool((idx[k:] == 0).all())
        ok = ok and torch.equal(zones.view(iv), e_zones.view(iv)) and torch.equal(fetched[:k].view(iv), dother[w_idx].view(iv))
        ok = ok and float(mm[0]) == float(t.min()) and float(mm[1]) == float(t.max())
        print(dtype, rep, k, ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_zone_map_zoned_select_and_gather_captured_into_one_graph():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 6: argument checks -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_argument_checks_of_the_c_entry_points(ctx, dtype):
    x = datagen.mixed_column(40, seed=71) if dtype == "f64" else datagen.mixed_column_f32(40, seed=71)
    col, xd = encoded(ctx, x)
    dec = ctx.decode(col)
    lib = capi.lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    zones = torch.full((col.n_vectors, 2), 7.0, dtype=dec.dtype, device=DEV)
    mm = torch.full((2,), 7.0, dtype=dec.dtype, device=DEV)
    zm, zv, red, sel = (getattr(lib, f"alpgpu_{n}_{dtype}") for n in ("zone_map", "zone_map_of_values", "zones_minmax", "select_range_zoned"))
    assert zm(ctx.h, None, p(zones)) == -2 and zm(ctx.h, ctypes.byref(col.c), None) == -2
    assert zv(ctx.h, None, col.n_vectors, p(zones)) == -2 and zv(ctx.h, p(xd), col.n_vectors, None) == -2
    assert red(ctx.h, None, col.n_vectors, p(mm)) == -2 and red(ctx.h, p(zones), col.n_vectors, None) == -2
    idx = torch.full((4096,), 7, dtype=torch.int64, device=DEV)
    vals = torch.full((4096,), 7.0, dtype=dec.dtype, device=DEV)
    count = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    scratch = ctx.select_scratch(col)
    total = dec.numel()
    good = (ctypes.byref(col.c), p(zones), 0, 10, -1.0, 1.0, p(idx), p(vals), 4096, p(count), p(scratch))
    for at, bad in ((0, None), (1, None), (6, None), (9, None), (10, None)):  # NULL column, zones, indices (with a capacity), count, scratch
        args = list(good)
        args[at] = bad
        assert sel(ctx.h, *args) == -2, f"argument {at}"
    for first, n in ((total - 100, 101), (0, total + 1), (total + 1, 0), (2**64 - 1, 2), (2**63, 2**63)):
        assert sel(ctx.h, ctypes.byref(col.c), p(zones), first, n, -1.0, 1.0, p(idx), p(vals), 4096, p(count), p(scratch)) == -2, f"range ({first}, {n}) must be refused"
    # a zone array that is not aligned to its records (16 / 8 bytes), raw values that are not 16-byte aligned: refused like a misaligned scratch
    vb = dec.element_size()
    off = lambda t, nbytes: ctypes.c_void_p(t.data_ptr() + nbytes)
    assert zm(ctx.h, ctypes.byref(col.c), off(zones, vb)) == -2 and zv(ctx.h, p(xd), col.n_vectors - 1, off(zones, vb)) == -2
    assert zv(ctx.h, off(xd, vb), col.n_vectors - 1, p(zones)) == -2
    assert red(ctx.h, off(zones, vb), col.n_vectors - 1, p(mm)) == -2
    assert sel(ctx.h, ctypes.byref(col.c), off(zones, vb), 0, 10, -1.0, 1.0, p(idx), p(vals), 4096, p(count), p(scratch)) == -2
    ctx.synchronize()
    assert bool((zones == 7).all()) and bool((mm == 7).all()) and bool((idx == 7).all()) and bool((vals == 7).all()) and int(count) == 7, "a refused call wrote"
    # nothing to do is not an error and launches nothing (the reduction still resets its result)
    empty = capi.CColumn()
    assert zm(ctx.h, ctypes.byref(empty), None) == 0 and zv(ctx.h, None, 0, None) == 0
    assert sel(ctx.h, ctypes.byref(col.c), None, 0, 0, -1.0, 1.0, None, None, 0, p(count), None) == 0  # n == 0 needs neither zones nor scratch
    assert red(ctx.h, None, 0, p(mm)) == 0
    ctx.synchronize()
    assert int(count) == 0 and mm.tolist() == [INF, -INF] and bool((zones == 7).all())


def test_python_rejects_tensors_that_do_not_fit(ctx):
    col, xd = encoded(ctx, datagen.mixed_column(6, seed=95))
    good = ctx.zone_map(col)
    idx = torch.full((64,), 7, dtype=torch.int64, device=DEV)
    count = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    bads = (good.to(torch.float32), good.cpu(), good[:5], good.reshape(-1), torch.zeros((6, 3), dtype=torch.float64, device=DEV)[:, :2], [[0.0, 1.0]] * 6, good.cpu().numpy())
    for bad in bads:
        with pytest.raises(ValueError):
            ctx.select_range_into(col, -INF, INF, idx, count, zones=bad)
        with pytest.raises(ValueError):
            ctx.zone_map(col, out=bad)
        with pytest.raises(ValueError):
            ctx.zone_map_of_values(xd, out=bad)
    for bad in (good.cpu(), good.reshape(-1), good.to(torch.int64), [[0.0, 1.0]], torch.zeros((6, 3), dtype=torch.float64, device=DEV)[:, :2]):
        with pytest.raises(ValueError):
            ctx.column_minmax(bad)
    for bad in (xd.cpu(), xd[:1000], xd[::2], xd.to(torch.int64), xd[1:1025], None):
        with pytest.raises(ValueError):
            ctx.zone_map_of_values(bad)
    for bad in (torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(2, dtype=torch.float32, device=DEV), torch.zeros(2, dtype=torch.float64)):
        with pytest.raises(ValueError):
            ctx.column_minmax(good, out=bad)
    zf = torch.stack([torch.arange(9.0), torch.arange(9.0) + 1], dim=1).to(torch.float32).to(DEV).contiguous()
    assert ctx.column_minmax(zf[1:]).tolist() == [1.0, 9.0]  # float records are 8 bytes: a map that starts at an odd record is aligned
    with pytest.raises(ValueError):
        ctx.column_minmax(good[1:].view(torch.float64).reshape(-1)[1:-1].reshape(-1, 2))  # double records shifted by 8 bytes
    ctx.synchronize()
    assert bool((idx == 7).all()) and int(count) == 7, "a refused select launched"
    assert torch.equal(ibits(ctx.zone_map(col, out=torch.empty((9, 2), dtype=torch.float64, device=DEV))[:6]), ibits(good))  # a larger buffer is fine


def test_cpp_column_zone_map_and_zoned_select_range(tmp_path):
    """include/alp/batch.hpp: alp::gpu::column<double / float>::zone_map, min_max and select_range with zones (tests/cpp/zone_test.cpp)"""
    exe = tmp_path / "zone_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/zone_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0 and "zone_test: 0 failures" in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]


# ---- 7: a speed sanity check ------------------------------------------------------------------------------------------------------------------
def test_a_narrow_zoned_select_of_a_sorted_column_is_faster_than_the_plain_one(ctx):
    """a sorted double column of 64 Ki vectors, a predicate a few vectors wide: the zoned call reads 16 bytes of nearly every vector where the plain
    one decodes it, so it must be faster; by how much is not asserted.  Median of 7 device-event timings, arms alternating."""
    nv = 1 << 16
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.sort(torch.round((torch.rand(nv * 1024, generator=g, device=DEV, dtype=torch.float64) * 2e5 - 1e5) * 100.0) / 100.0).values
    col = ctx.encode(x)
    lo, hi = float(x[nv * 512]), float(x[nv * 512 + 3000])
    del x
    zones = ctx.zone_map(col)
    idx = torch.empty(1 << 20, dtype=torch.int64, device=DEV)
    pidx = torch.empty(1 << 20, dtype=torch.int64, device=DEV)
    count, pcount = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    scratch = ctx.select_scratch(col)
    arms = {"plain": lambda: ctx.select_range_into(col, lo, hi, pidx, pcount, scratch=scratch),
            "zoned": lambda: ctx.select_range_into(col, lo, hi, idx, count, scratch=scratch, zones=zones)}
    ts = {k: [] for k in arms}
    for rep in range(9):
        for name, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts[name].append(a.elapsed_time(b))
    t_plain, t_zoned = float(np.median(ts["plain"][2:])), float(np.median(ts["zoned"][2:]))
    k = int(count)
    print(f"select of {k} values from {nv} sorted vectors: zoned {t_zoned:.3f} ms, plain {t_plain:.3f} ms")
    assert 3000 <= k == int(pcount) <= 1 << 20 and torch.equal(idx[:k], pidx[:k])
    assert t_zoned < t_plain
