"""GPU: set membership (include/alpgpu.h, "set membership": alpgpu_select_in_mask_*).  The expected bitmap never comes from the code under test:
x = ctx.decode(col) (pinned to the oracle and the reference by other suites), membership by == (a broadcast compare for short lists, a
searchsorted into the NaN-free sorted list and one == for long ones), bits packed 64 to a word in index order.  Bitmaps compare as integers."""
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

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF, NAN = math.inf, math.nan
OPS = {"set": 0, "and": 1, "or": 2}


def ibits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def pack(bits):
    """bool tensor of whole vectors -> the bitmap: bit r & 63 of int64 word r >> 6 = bits[r]"""
    w = torch.ones(64, dtype=torch.int64, device=bits.device) << torch.arange(64, dtype=torch.int64, device=bits.device)
    return (bits.reshape(-1, 64).to(torch.int64) * w).sum(dim=1)


def unpack(mask):
    s = torch.arange(64, dtype=torch.int64, device=mask.device)
    return (((mask.reshape(-1, 1) >> s) & 1) != 0).reshape(-1)


def random_mask(n_vectors, seed):
    words = np.random.default_rng(seed).integers(0, 2**64, 16 * n_vectors, dtype=np.uint64)
    return torch.from_numpy(words.view(np.int64)).to(DEV)


def vectors_cleared(mask, keep_every, fill):
    """the mask with every vector but each keep_every-th set to `fill` (0 or -1) in all 16 words: skipped vectors beside decoded ones"""
    m = mask.clone().reshape(-1, 16)
    v = torch.arange(m.shape[0], device=mask.device)
    m[(v % keep_every) != 1] = fill
    return m.reshape(-1)


def in_range(total, first, n):
    r = torch.arange(total, device=DEV)
    return (r >= first) & (r < first + n)


def member(x, lst):
    """the definition on the device, by torch: some element of lst == the value (-0.0 == 0.0; a NaN, value or element, never)"""
    l = lst[~torch.isnan(lst)]
    if l.numel() == 0:
        return torch.zeros(x.numel(), dtype=torch.bool, device=x.device)
    if l.numel() <= 80:
        return (x[:, None] == l[None, :]).any(dim=1)
    s = torch.sort(l).values
    at = torch.searchsorted(s, x).clamp(max=s.numel() - 1)
    return s[at] == x


def qualify(x, lst, first=0, n=None, negate=False):
    n = x.numel() - first if n is None else n
    return (member(x, lst) != negate) & in_range(x.numel(), first, n)


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


def make_list(xs, size, seed, extra=()):
    """a list of `size` elements in no order, drawn from the column's own decoded values xs so that hits exist: one value of the column first, then
    a 1-ulp neighbour of it that the column does not hold, then `extra` (exception values), the zero of the other sign where the column holds one,
    +-inf, then more values of the column (at most half of its distinct ones: never everything) and more neighbours; padded with absent values"""
    dt = xs.dtype.type
    rng = np.random.default_rng(seed)
    if size == 0:
        return np.zeros(0, xs.dtype)
    present = np.unique(xs[~np.isnan(xs)])
    n_hit = min(present.size, max(1, min(size, present.size // 2)))
    hits = rng.choice(present, n_hit, replace=False) if n_hit else present[:0]
    with np.errstate(over="ignore"):
        near = np.stack([np.nextafter(hits, dt(INF)), np.nextafter(hits, dt(-INF))], axis=1).reshape(-1)
    near = near[~np.isin(near, present) & ~np.isnan(near)]
    must = [dt(e) for e in extra]
    if np.any((xs == 0) & np.signbit(xs)):
        must.append(dt(0.0))
    if np.any((xs == 0) & ~np.signbit(xs)):
        must.append(dt(-0.0))
    must += [dt(INF), dt(-INF)]
    head = np.concatenate([hits[:1], near[:1], np.asarray(must, dtype=xs.dtype)])[:size]
    rest = size - head.size
    more_hits = hits[1:1 + rest - rest // 3]
    more_near = near[1:1 + rest - more_hits.size]
    lst = np.concatenate([head, more_hits, more_near])
    while lst.size < size:  # absent values: full-precision noise that the column does not hold
        c = (rng.standard_normal(2 * (size - lst.size) + 64) * 12345.678).astype(xs.dtype)
        c = c[~np.isin(c, present)]
        lst = np.concatenate([lst, c[:size - lst.size]])
    return rng.permutation(lst).astype(xs.dtype)


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
    """(DeviceColumn, its store decode, the decode on the host, a few exception values), encoded once per session and left unchanged"""
    if name not in _cache:
        xd = torch.from_numpy(np.ascontiguousarray(COLUMNS[name]())).to(DEV)
        col = ctx.encode(xd)
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(xd)), f"{name}: decode(encode(x)) != x"
        xs = dec.cpu().numpy()
        ev = xs[exception_indices(col)]
        ev = ev[~np.isnan(ev)]
        _cache[name] = (col, dec, xs, tuple(ev[:: max(1, ev.size // 3)][:3]))
    return _cache[name]


_lists = {}


def device_list(ctx, name, size, seed=0):
    """the list of this size for this column, made once and shared: (device tensor in no order, its members among the column's values)"""
    key = (name, size, seed)
    if key not in _lists:
        col, x, xs, ev = column(ctx, name)
        lst = torch.from_numpy(make_list(xs, size, 1000 * seed + size, ev)).to(DEV)
        _lists[key] = (lst, member(x, lst))
    return _lists[key]


def lds_max(col):
    return capi.Context.in_list_lds_max(col.dtype)


# ---- 1. every list size on every kind of column, both polarities -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_lists_of_every_size_against_the_store_decode(ctx, name):
    col, x, xs, ev = column(ctx, name)
    total = x.numel()
    L = lds_max(col)
    assert L > 0
    exc_set = torch.zeros(total, dtype=torch.bool, device=DEV)
    exc_set[torch.from_numpy(exception_indices(col)).to(DEV)] = True
    mask = random_mask(col.n_vectors, 1)  # SET writes every word: what the bitmap held does not matter
    hit_exception = False
    for size in (0, 1, 2, 3, 63, 64, 65, L - 1, L, L + 1, 2 * L + 7, 100000):
        lst, m = device_list(ctx, name, size)
        assert lst.numel() == size
        k = int(m.sum())
        assert (size == 0 and k == 0) or 0 < k < total, f"{name}, {size} elements: the list must select some but not all values ({k} of {total})"
        hit_exception = hit_exception or bool(exc_set[m].any())
        for negate in (False, True):
            got = ctx.select_in_mask(col, lst, negate=negate, mask=mask)
            assert got is mask and torch.equal(mask, pack(m != negate)), f"{name}, {size} elements, negate={negate}: bitmap differs from == on the store decode"
    assert hit_exception or not bool(exc_set.any()), f"{name}: the column has exceptions and no list selected one"
    lst, m = device_list(ctx, name, 65)
    fresh = ctx.select_in_mask(col, lst)  # the allocating form
    assert fresh.dtype == torch.int64 and fresh.numel() == 16 * col.n_vectors and torch.equal(fresh, pack(m))


def test_neighbours_zeros_and_infinities(ctx):
    """what make_list promises: 1-ulp neighbours of present values are in the lists and miss, the zero of the other sign hits"""
    for name in ("mixed", "mixed_f32"):
        col, x, xs, ev = column(ctx, name)
        dt = xs.dtype.type
        assert np.any((xs == 0) & np.signbit(xs)) and np.any(np.isinf(xs)) and np.any(np.isnan(xs))
        v = xs[np.isfinite(xs) & (xs != 0)][7]
        for lst_np, want in (([0.0], xs == 0), ([-0.0], xs == 0), ([INF], xs == INF), ([-INF], xs == -INF), ([NAN], np.zeros(xs.size, bool)),
                             ([np.nextafter(v, dt(INF)), np.nextafter(v, dt(-INF))], np.zeros(xs.size, bool)), ([v], xs == v)):
            lst = torch.tensor(lst_np, dtype=x.dtype, device=DEV)
            w = torch.from_numpy(want).to(DEV)
            assert torch.equal(ctx.select_in_mask(col, lst), pack(w)), f"{name}: IN {lst_np}"
            assert torch.equal(ctx.select_in_mask(col, lst, negate=True), pack(~w)), f"{name}: NOT IN {lst_np}"
        assert bool((xs == v).any()) and bool((xs == 0).any())


# ---- 2. every op against prior bitmaps: the skip rules -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "rd_unit", "every_width_exc", "adversarial", "mixed_f32", "rd_unit_f32"])
def test_every_op_against_prior_bitmaps(ctx, name):
    col, x, xs, ev = column(ctx, name)
    nv, total = col.n_vectors, x.numel()
    rnd = random_mask(nv, 4)
    priors = {"zeros": torch.zeros_like(rnd), "ones": torch.full_like(rnd, -1), "random": rnd, "vectors zero": vectors_cleared(rnd, 3, 0),
              "vectors ones": vectors_cleared(rnd, 3, -1)}
    for size in (3, 65, lds_max(col) + 1):
        lst, m = device_list(ctx, name, size)
        assert 0 < int(m.sum()) < total
        for negate in (False, True):
            for first, n in ((0, total), (1024 + 100, total - 2048)):
                q = (m != negate) & in_range(total, first, n)
                for pname, prior in priors.items():
                    pb = unpack(prior)
                    for op, want in (("set", q), ("and", pb & q), ("or", pb | q)):
                        mask = prior.clone()
                        ctx.select_in_mask(col, lst, first=first, n=n, negate=negate, op=op, mask=mask)
                        assert torch.equal(mask, pack(want)), f"{name}, {size} elements, negate={negate}: {op} into {pname}, first={first} n={n}"


# ---- 3. ranges -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "mixed_f32"])
def test_first_and_n_under_every_op(ctx, name):
    col, x, xs, ev = column(ctx, name)
    total = x.numel()
    lst, m = device_list(ctx, name, 65)
    assert 0 < int(m.sum()) < total
    slist = torch.sort(lst).values
    prior = random_mask(col.n_vectors, 2)
    pb = unpack(prior)
    ranges = [(3 * 1024 + 17, 500), (3 * 1024 + 17, 1), (63, 1), (63, 2), (64, 64), (65, 63), (1024 + 63, 66), (5 * 1024 - 100, 300), (5 * 1024, 1024), (5 * 1024 - 1, 1026),
              (99 * 1024 + 1000, 101 * 1024), (total - 1, 1), (0, total), (0, total - 500), (0, 0), (777, 0), (total, 0), (1023, 2)]
    for first, n in ranges:
        for negate in (False, True):
            q = (m != negate) & in_range(total, first, n)
            want = {"set": q, "and": pb & q, "or": pb | q}
            for op in OPS:
                mask = prior.clone()
                ctx.select_in_mask(col, slist, first=first, n=n, negate=negate, op=op, mask=mask, sorted=True)
                assert torch.equal(mask, pack(want[op])), f"{name} first={first} n={n} negate={negate} op={op}"
            assert n < 2000 or bool(q.any())
    # ranges past the end, and a first + n that overflows, are refused on the host: the bitmap is unchanged
    fn = getattr(capi.lib, "alpgpu_select_in_mask_" + col.dtype)
    mask = prior.clone()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for first, n in ((total - 100, 101), (0, total + 1), (total + 1, 0), (2**64 - 1, 2), (2, 2**64 - 1), (2**63, 2**63)):
        for op in OPS.values():
            for negate in (0, 1):
                assert fn(ctx.h, ctypes.byref(col.c), first, n, p(slist), slist.numel(), negate, None, op, p(mask)) == -2, f"range ({first}, {n}) must be refused"
    ctx.synchronize()
    assert torch.equal(mask, prior), "a refused select_in_mask wrote"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_single_vector_and_an_empty_column(ctx, dtype):
    cases = datagen.adversarial_vectors() if dtype == "f64" else datagen.adversarial_vectors_f32()
    selective = False
    for name in ("plain", "all_exceptions", "all_zero", "half_negzero", "inf_ends", "prefix_nan"):
        col = ctx.encode(torch.from_numpy(cases[name]).to(DEV))
        assert col.n_vectors == 1
        x = ctx.decode(col)
        xs = x.cpu().numpy()
        prior = random_mask(1, 3)
        for size in (0, 1, 3, 65, lds_max(col) + 1):
            lst = torch.from_numpy(make_list(xs, size, 7 + size)).to(DEV)
            m = member(x, lst)
            selective = selective or 0 < int(m.sum()) < 1024
            for negate in (False, True):
                for first, n in ((0, 1024), (1023, 1), (63, 2), (100, 900)):
                    q = (m != negate) & in_range(1024, first, n)
                    for op, want in (("set", q), ("and", unpack(prior) & q), ("or", unpack(prior) | q)):
                        mask = prior.clone()
                        ctx.select_in_mask(col, lst, first=first, n=n, negate=negate, op=op, mask=mask)
                        assert torch.equal(mask, pack(want)), f"{name}, {size} elements, negate={negate} first={first} n={n} op={op}"
    assert selective, "no list selected some but not all values of a vector"
    empty = capi.CColumn()
    fn = getattr(capi.lib, "alpgpu_select_in_mask_" + dtype)
    lst = torch.zeros(4, dtype=torch.float64 if dtype == "f64" else torch.float32, device=DEV)
    for op in OPS.values():
        assert fn(ctx.h, ctypes.byref(empty), 0, 0, ctypes.c_void_p(lst.data_ptr()), 4, 0, None, op, None) == 0
        assert fn(ctx.h, ctypes.byref(empty), 0, 0, None, 0, 1, None, op, None) == 0
        assert fn(ctx.h, ctypes.byref(empty), 0, 1, ctypes.c_void_p(lst.data_ptr()), 4, 0, None, op, None) == -2


# ---- 4. NaNs and duplicates in the list; the equivalence with rounds of select_mask -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "mixed_f32"])
def test_nans_at_the_end_and_duplicates_change_nothing(ctx, name):
    col, x, xs, ev = column(ctx, name)
    L = lds_max(col)
    for size in (5, 64, L - 3, L + 1):
        lst, m = device_list(ctx, name, size)
        assert 0 < int(m.sum()) < x.numel()
        want = ctx.select_in_mask(col, lst)
        assert torch.equal(want, pack(m))
        nans = torch.full((3,), NAN, dtype=x.dtype, device=DEV)
        noisy = torch.cat([lst, nans, lst[: max(1, size // 2)], lst[:1], lst[:1]])  # NaNs sort last; every second element twice, one four times
        assert torch.equal(ctx.select_in_mask(col, noisy), want), f"{name}, {size} elements with NaNs and duplicates"
        assert torch.equal(ctx.select_in_mask(col, noisy, negate=True), pack(~m))
        by_hand = torch.cat([torch.sort(torch.cat([lst, lst[:1]])).values, nans])  # sorted by the caller, NaNs at its end
        assert torch.equal(ctx.select_in_mask(col, by_hand, sorted=True), want)
    only_nans = torch.full((9,), NAN, dtype=x.dtype, device=DEV)
    assert not bool(ctx.select_in_mask(col, only_nans).any()) and bool((ctx.select_in_mask(col, only_nans, negate=True) == -1).all())


@pytest.mark.parametrize("name", ["mixed", "rd_unit", "every_width_exc_f32"])
def test_a_short_list_is_rounds_of_select_mask(ctx, name):
    col, x, xs, ev = column(ctx, name)
    for r in (1, 2, 8):
        vals = np.unique(make_list(xs, 3 * r, 40 + r, ev))
        vals = vals[~np.isnan(vals)]
        pick = np.concatenate([vals[np.isin(vals, xs)][: r - r // 3], vals[~np.isin(vals, xs)]])[:r]
        assert pick.size == r and np.unique(pick).size == r
        rounds = torch.zeros(16 * col.n_vectors, dtype=torch.int64, device=DEV)
        for v in pick:
            ctx.select_mask(col, float(v), float(v), op="or", mask=rounds)
        got = ctx.select_in_mask(col, pick)
        assert torch.equal(got, rounds), f"{name}: {r} values"
        assert 0 < int(unpack(got).sum()) < x.numel()


# ---- 5. zone maps --------------------------------------------------------------------------------------------------------------------------------------
def sorted_column(ctx, f32):
    key = "sorted_f32" if f32 else "sorted"
    if key not in _cache:
        raw = datagen.mixed_column_f32(120, seed=31) if f32 else datagen.mixed_column(120, seed=31)
        s = np.sort(raw[~np.isnan(raw)])
        s = np.ascontiguousarray(s[: s.size // 1024 * 1024])
        xd = torch.from_numpy(s).to(DEV)
        col = ctx.encode(xd)
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(xd))
        _cache[key] = (col, dec, dec.cpu().numpy(), ())
    return _cache[key]


def excluded_vectors(zones, lst):
    """vectors whose record holds no element of the list, by the definition"""
    z = zones.cpu().numpy()
    l = lst.cpu().numpy()
    l = np.sort(l[~np.isnan(l)])
    if l.size == 0:
        return np.ones(z.shape[0], dtype=bool)
    at = np.searchsorted(l, z[:, 0], side="left")
    with np.errstate(invalid="ignore"):
        return (at >= l.size) | (l[np.minimum(at, l.size - 1)] > z[:, 1])


@pytest.mark.parametrize("f32", [False, True])
def test_zone_maps_change_no_byte(ctx, f32):
    random_name = "mixed_f32" if f32 else "mixed"
    most_excluded = {False: False, True: False}
    for cname, (col, x, xs, ev) in (("random", column(ctx, random_name)), ("sorted", sorted_column(ctx, f32))):
        nv, total = col.n_vectors, x.numel()
        L = lds_max(col)
        zones = ctx.zone_map(col)
        wide = torch.empty_like(zones)
        wide[:, 0], wide[:, 1] = -INF, INF
        holes = zones.clone()
        holes[::3, 0] = NAN  # a NaN bound: decode the vector
        holes[1::3, 1] = NAN
        prior = vectors_cleared(random_mask(nv, 12), 3, 0)
        lists = [("drawn %d" % size, torch.from_numpy(make_list(xs, size, 70 + size, ev)).to(DEV)) for size in (0, 1, 5, 65, L, L + 1, 2 * L + 7)]
        if cname == "sorted":
            lo_v = xs[np.isfinite(xs)]
            lists.append(("clustered", torch.from_numpy(np.ascontiguousarray(np.unique(lo_v)[100:140])).to(DEV)))  # neighbours in value: a few vectors
            lists.append(("clustered long", torch.from_numpy(np.ascontiguousarray(np.unique(lo_v)[: L + 50])).to(DEV)))
        for lname, lst in lists:
            m = member(x, lst)
            assert lst.numel() == 0 or 0 < int(m.sum()) < total, f"{cname}, {lname}"
            excl = excluded_vectors(zones, lst)
            for negate in (False, True):
                if cname == "sorted" and excl.mean() > 0.5:
                    most_excluded[negate] = True
                for first, n in ((1024 + 100, total - 2048),):  # vectors outside the range, two cut by it, the rest whole
                    q = (m != negate) & in_range(total, first, n)
                    for op, want in (("set", q), ("and", unpack(prior) & q), ("or", unpack(prior) | q)):
                        plain = prior.clone()
                        ctx.select_in_mask(col, lst, first=first, n=n, negate=negate, op=op, mask=plain)
                        assert torch.equal(plain, pack(want)), f"{cname}, {lname}, negate={negate}, {op}: without zones"
                        for zname, z in (("the zone map", zones), ("widened", wide), ("NaN bounds", holes)):
                            mask = prior.clone()
                            ctx.select_in_mask(col, lst, first=first, n=n, negate=negate, zones=z, op=op, mask=mask)
                            assert torch.equal(mask, plain), f"{cname}, {lname}, negate={negate}, {op}: {zname} changed the bytes"
    assert most_excluded[False] and most_excluded[True], "no list excluded most vectors of the sorted column"


# ---- 6. robustness: an unsorted list ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_an_unsorted_list_stays_inside_the_bitmap(ctx, dtype):
    name = "mixed" if dtype == "f64" else "mixed_f32"
    col, x, xs, ev = column(ctx, name)
    nv = col.n_vectors
    lst, _ = device_list(ctx, name, 2 * lds_max(col) + 7)  # in no order; the global tier, which reads the list itself
    guard = 64
    buf = torch.full((guard + 16 * nv + guard,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    fn = getattr(capi.lib, "alpgpu_select_in_mask_" + dtype)
    rc = fn(ctx.h, ctypes.byref(col.c), 0, x.numel(), ctypes.c_void_p(lst.data_ptr()), lst.numel(), 0, None, 0, ctypes.c_void_p(buf.data_ptr() + 8 * guard))
    ctx.synchronize()
    assert rc == 0
    assert bool((buf[:guard] == 0x5A5A5A5A5A5A5A5A).all()) and bool((buf[guard + 16 * nv:] == 0x5A5A5A5A5A5A5A5A).all()), "guard words changed"


# ---- 7. determinism, statelessness, capture ----------------------------------------------------------------------------------------------------------------
def test_the_same_call_gives_the_same_bytes(ctx):
    col, x, xs, ev = column(ctx, "mixed")
    zones = ctx.zone_map(col)
    for size in (65, lds_max(col) + 1):
        lst, m = device_list(ctx, "mixed", size)
        runs = []
        for rep in range(3):
            torch.empty(1 << (20 + rep), dtype=torch.uint8, device=DEV).fill_(rep)  # (a different allocation history each time)
            mask = ctx.select_in_mask(col, lst)
            ctx.select_in_mask(col, lst, negate=True, zones=zones, first=999, n=100000, op="or", mask=mask)
            runs.append(mask.cpu().numpy().tobytes())
        assert runs[0] == runs[1] == runs[2]
        assert torch.equal(mask, pack(m | (~m & in_range(x.numel(), 999, 100000))))


def test_in_list_calls_leave_the_decode_plan_alone(ctx):
    for hinted in (True, False):
        raw = datagen.mixed_column(150, seed=91)
        col = ctx.encode(torch.from_numpy(raw).to(DEV))
        if hinted:
            ctx.column_totals(col)
        ctx.decode(col)
        ctx.synchronize()  # (what an unhinted decode learns about the column is in by now)
        before = ctx.decode_plan(col)
        vals = raw[~np.isnan(raw)][:300]
        mask = ctx.select_in_mask(col, vals)
        ctx.select_in_mask(col, vals[:5], first=5, n=9999, negate=True, op="or", mask=mask)
        ctx.select_in_mask(col, np.concatenate([vals, np.arange(10000.0)]), zones=ctx.zone_map(col), op="and", mask=mask)
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
def member(x, lst):
    s = torch.sort(lst[~torch.isnan(lst)]).values
    return s[torch.searchsorted(s, x).clamp(max=s.numel() - 1)] == x
def draw(x, size, seed):
    rng = np.random.default_rng(seed)
    u = np.unique(x[np.isfinite(x)])
    hits = rng.choice(u, min(size // 2, u.size // 2), replace=False)
    pad = (rng.standard_normal(size - hits.size) * 4321.0).astype(x.dtype)
    return torch.sort(torch.from_numpy(np.concatenate([hits, pad])).cuda()).values
a0, a1 = datagen.mixed_column(230, seed=81), datagen.mixed_column(230, seed=83)
b0, b1 = datagen.mixed_column_f32(230, seed=82), datagen.mixed_column_f32(230, seed=84)
ad, bd = [torch.from_numpy(t).cuda() for t in (a0, a1)], [torch.from_numpy(t).cuda() for t in (b0, b1)]
cola, colb = ctx.encode(ad[0]), ctx.encode(bd[0])
na, nb = 65, ctx.in_list_lds_max("f32") + 9                 # the LDS tier and the global tier
la, lb = draw(a0, na, 1), draw(b0, nb, 2)
nv = 230
mask = torch.zeros(16 * nv, dtype=torch.int64, device="cuda:0")
def calls(mask):
    ctx.select_in_mask(cola, la, first=1000, n=220 * 1024, mask=mask, sorted=True)
    ctx.select_in_mask(colb, lb, negate=True, op="and", mask=mask, sorted=True)
with torch.cuda.stream(side):
    calls(mask)                                             # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        calls(mask)
for rep in range(3):
    if rep == 1:
        ctx.encode(ad[1], cola); ctx.encode(bd[1], colb)    # other data encoded into the same buffers, other lists written into the same tensors
        la.copy_(draw(a1, na, 3)); lb.copy_(draw(b1, nb, 4))
    torch.cuda.synchronize()
    mask.fill_(rep - 1)
    g.replay()
    torch.cuda.synchronize()
    da, db = ctx.decode(cola), ctx.decode(colb)
    m = member(da, la) & ~member(db, lb); m[:1000] = False; m[1000 + 220 * 1024:] = False
    w = torch.ones(64, dtype=torch.int64, device="cuda:0") << torch.arange(64, dtype=torch.int64, device="cuda:0")
    want = (m.reshape(-1, 64).to(torch.int64) * w).sum(dim=1)
    k = int(m.sum())
    ok = ok and 0 < k < m.numel() and torch.equal(mask, want)
    print(rep, k, ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_list_and_the_columns_change():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 8. argument checks ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c_argument_checks(ctx, dtype):
    name = "mixed" if dtype == "f64" else "mixed_f32"
    col, x, xs, ev = column(ctx, name)
    nv, vb = col.n_vectors, 8 if dtype == "f64" else 4
    fn = getattr(capi.lib, "alpgpu_select_in_mask_" + dtype)
    lst = torch.sort(device_list(ctx, name, 65)[0]).values
    zones = ctx.zone_map(col)
    prior = random_mask(nv + 1, 10)
    mask = prior.clone()
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    c = ctypes.byref(col.c)
    for op in (-1, 3, 17):
        assert fn(ctx.h, c, 0, 1024, p(lst), 65, 0, None, op, p(mask)) == -2, "a bad op must be refused"
    for op in OPS.values():
        for negate in (0, 1):
            assert fn(ctx.h, c, 0, 1024, p(lst), 65, negate, None, op, p(mask, 4)) == -2, "a misaligned bitmap must be refused"
            assert fn(ctx.h, c, 0, 1024, p(lst), 65, negate, None, op, None) == -2, "a NULL bitmap must be refused"
            assert fn(ctx.h, None, 0, 1024, p(lst), 65, negate, None, op, p(mask)) == -2, "a NULL column must be refused"
            assert fn(ctx.h, c, 0, 1024, None, 65, negate, None, op, p(mask)) == -2, "a NULL list with n_list > 0 must be refused"
            assert fn(ctx.h, c, 0, 1024, p(lst, vb // 2), 64, negate, None, op, p(mask)) == -2, "a misaligned list must be refused"
            assert fn(ctx.h, c, 0, 1024, p(lst), 65, negate, p(zones, vb), op, p(mask)) == -2, "misaligned zones must be refused"
            assert fn(ctx.h, c, 0, 1024, p(lst), 2**31, negate, None, op, p(mask)) == -2, "n_list beyond 2^31 - 1 must be refused"
            assert fn(ctx.h, c, 0, 1024, p(lst), 2**40, negate, None, op, p(mask)) == -2
            assert fn(None, c, 0, 1024, p(lst), 65, negate, None, op, p(mask)) == -2, "a NULL context must be refused"
    ctx.synchronize()
    assert torch.equal(mask, prior), "a refused call wrote"
    # n == 0: SET and AND clear the bitmap (and nothing behind it), OR enqueues nothing; negated or not
    for negate in (0, 1):
        for op, cleared in ((0, True), (1, True), (2, False)):
            mask = prior.clone()
            assert fn(ctx.h, c, 0, 0, p(lst), 65, negate, None, op, p(mask)) == 0
            ctx.synchronize()
            assert torch.equal(mask[16 * nv:], prior[16 * nv:])
            assert bool((mask[:16 * nv] == 0).all()) if cleared else torch.equal(mask, prior)
    # an empty list with a NULL pointer is valid: nothing is a member, and under negate everything in the range qualifies
    mask = prior.clone()
    assert fn(ctx.h, c, 0, x.numel(), None, 0, 0, None, 0, p(mask)) == 0
    ctx.synchronize()
    assert bool((mask[:16 * nv] == 0).all()) and torch.equal(mask[16 * nv:], prior[16 * nv:])
    assert fn(ctx.h, c, 70, 2000, None, 0, 1, p(zones), 0, p(mask)) == 0
    ctx.synchronize()
    assert torch.equal(mask[:16 * nv], pack(in_range(x.numel(), 70, 2000))) and torch.equal(mask[16 * nv:], prior[16 * nv:])


def test_python_rejects_arguments_that_do_not_fit(ctx, monkeypatch):
    col, x, xs, ev = column(ctx, "mixed")
    cf = column(ctx, "mixed_f32")[0]
    nv = col.n_vectors
    lst = device_list(ctx, "mixed", 65)[0]
    mask = torch.full((16 * nv,), 7, dtype=torch.int64, device=DEV)
    zones = ctx.zone_map(col)

    def unreachable(*a, **k):
        raise AssertionError("the library was called")
    for t in ("f64", "f32"):
        monkeypatch.setattr(capi.lib, "alpgpu_select_in_mask_" + t, unreachable)
    wide = torch.full((32 * nv,), 7, dtype=torch.int64, device=DEV)
    for bad in (mask.to(torch.int32), mask.cpu(), mask[:-16], wide, wide[::2], mask.reshape(nv, 16), [1, 2, 3], np.zeros(16 * nv, np.int64)):
        for op in OPS:
            with pytest.raises(ValueError):
                ctx.select_in_mask(col, lst, op=op, mask=bad)
    for op in ("xor", "SET", 0, None):
        with pytest.raises(ValueError):
            ctx.select_in_mask(col, lst, op=op, mask=mask)
    for op in ("and", "or"):
        with pytest.raises(ValueError):
            ctx.select_in_mask(col, lst, op=op)
    for kw in ({"first": -1}, {"n": -1}):
        with pytest.raises(ValueError):
            ctx.select_in_mask(col, lst, mask=mask, **kw)
    for bad in (lst.to(torch.float32), lst.cpu().numpy().astype(np.float32), lst.to(torch.int64), lst.reshape(5, 13), np.arange(5)):  # the column's type, one dimension
        with pytest.raises(ValueError):
            ctx.select_in_mask(col, bad, mask=mask)
    with pytest.raises(ValueError):
        ctx.select_in_mask(cf, lst, mask=mask)  # a float column takes a float list
    unaligned = torch.zeros(2 * nv + 1, dtype=torch.float64, device=DEV)[1:].reshape(nv, 2)
    for bad in (zones.to(torch.float32), zones.cpu(), zones[:-1], zones.reshape(-1), zones.t(), torch.zeros((nv, 3), dtype=torch.float64, device=DEV), unaligned, [[0.0, 1.0]] * nv):
        with pytest.raises(ValueError):
            ctx.select_in_mask(col, lst, zones=bad, mask=mask)
    ctx.synchronize()
    assert bool((mask == 7).all()), "a refused call launched"


def test_values_in_every_form_the_wrapper_takes(ctx):
    col, x, xs, ev = column(ctx, "mixed")
    lst, m = device_list(ctx, "mixed", 65)
    want = pack(m)
    host = lst.cpu()
    for values in (lst, host, host.numpy(), host.tolist(), tuple(host.tolist())):
        assert torch.equal(ctx.select_in_mask(col, values), want)
    assert not bool(ctx.select_in_mask(col, []).any())


# ---- 9. the C++ wrapper ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cpp_column_select_in_mask_against_decompress_and_a_host_loop(ctx, tmp_path, dtype):
    """include/alp/batch.hpp: alp::gpu::column<double / float>::select_in_mask of a serialized column against column::decompress and a host loop
    over the definition of a member (tests/cpp/in_list_test.cpp)"""
    exe = tmp_path / "in_list_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/in_list_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    name = "adversarial" if dtype == "f64" else "adversarial_f32"  # NaN, +-inf and -0.0 among the values
    col, x, xs, ev = column(ctx, name)
    ctx.to_blob(col, x.numel()).tofile(str(tmp_path / "col.blob"))
    lst = np.concatenate([make_list(xs, 40, 5, ev), np.array([NAN, NAN], dtype=xs.dtype)])
    lst.tofile(str(tmp_path / "values.bin"))
    mask = vectors_cleared(random_mask(col.n_vectors, 53), 3, -1)
    mask[16:32] = 0
    mask.cpu().numpy().tofile(str(tmp_path / "in.mask"))
    p = subprocess.run([str(exe), dtype] + [str(tmp_path / f) for f in ("col.blob", "values.bin", "in.mask")], capture_output=True, text=True, timeout=600)
    line = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("ok ")]
    assert p.returncode == 0 and len(line) == 1, p.stdout[-3000:] + p.stderr[-2000:]
    k = int(member(x, torch.from_numpy(lst).to(DEV)).sum())
    assert int(line[0][1]) == col.n_vectors and int(line[0][2]) == k and 0 < k < x.numel()


# ---- 10. a semi-join end to end ----------------------------------------------------------------------------------------------------------------------------
def test_a_semi_join_of_two_columns_against_torch(ctx):
    """SELECT ... FROM t WHERE t.key IN (SELECT o.key FROM o WHERE lo <= o.val <= hi) AND t.flag IN (1, 3)"""
    rng = np.random.default_rng(77)
    nv_t, nv_o = 60, 20
    t_key = rng.integers(0, 50000, nv_t * 1024).astype(np.float64)
    t_flag = rng.integers(0, 5, nv_t * 1024).astype(np.float64)
    o_key = rng.integers(0, 50000, nv_o * 1024).astype(np.float64)
    o_val = np.round(rng.uniform(0, 100, nv_o * 1024), 2)
    dev = lambda a: torch.from_numpy(a).to(DEV)
    ct_key, ct_flag, co_key, co_val = (ctx.encode(dev(a)) for a in (t_key, t_flag, o_key, o_val))
    build_mask = ctx.select_mask(co_val, 10.0, 35.0)
    build = ctx.decode_masked(co_key, build_mask)
    assert build.numel() > lds_max(ct_key)  # thousands of keys: the global tier
    keys = torch.sort(build).values
    mask = ctx.select_in_mask(ct_flag, [1.0, 3.0])
    ctx.select_in_mask(ct_key, keys, op="and", mask=mask, sorted=True, zones=ctx.zone_map(ct_key))
    got = ctx.mask_to_indices(mask)
    tk, tf, ok, ov = dev(t_key), dev(t_flag), dev(o_key), dev(o_val)
    want = torch.isin(tk, ok[(ov >= 10.0) & (ov <= 35.0)]) & ((tf == 1.0) | (tf == 3.0))
    assert torch.equal(got, torch.nonzero(want).reshape(-1)) and 0 < got.numel() < tk.numel()
    anti = ctx.select_in_mask(ct_key, keys, negate=True, sorted=True)  # the anti-join: NOT IN
    assert torch.equal(ctx.mask_to_indices(anti), torch.nonzero(~torch.isin(tk, keys)).reshape(-1))
