"""GPU: the join probe (include/alpgpu.h, "join probe": alpgpu_join_probe_*).  EVERY expectation comes from the host replica (tests/join_replica.py:
numpy.searchsorted "left" / "right" on the NaN-free prefix of the sorted keys) fed with ctx.decode(col), which other suites pin to the oracle and the
reference; never with the call under test.  Positions, spans, indices and counts compare as integers.  Columns have at most 64 vectors."""
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
from in_list_replica import pack_bits
from join_replica import NO_MATCH, host_join, unpack_bits
from test_in_list_gpu import exception_indices, ibits, make_list, random_mask, vectors_cleared

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF, NAN = math.inf, math.nan
CANARY64, CANARY32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
GUARD = 64
ROW_BASE = 1000000  # payloads are ROW_BASE + a permutation: never a position

COLUMNS = {
    "mixed": lambda: datagen.mixed_column(64, seed=5),        # ALP with exceptions, NaN, +-inf, -0.0
    "rd_unit": lambda: datagen.rd_column(60, seed=6),         # ALP_RD rowgroups
    "mixed_f32": lambda: datagen.mixed_column_f32(64, seed=5),
    "rd_unit_f32": lambda: datagen.rd_column_f32(60, seed=6),
}
_cache = {}


def column(ctx, name):
    """(DeviceColumn, the store decode on the host, a few exception values), encoded once per session and left unchanged"""
    if name not in _cache:
        xd = torch.from_numpy(np.ascontiguousarray(COLUMNS[name]())).to(DEV)
        col = ctx.encode(xd)
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(xd)), f"{name}: decode(encode(x)) != x"
        assert col.n_vectors <= 64
        xs = dec.cpu().numpy()
        ev = xs[exception_indices(col)]
        ev = ev[~np.isnan(ev)]
        _cache[name] = (col, xs, tuple(ev[:: max(1, ev.size // 3)][:3]))
    return _cache[name]


def lds_max(col):
    return capi.Context.in_list_lds_max(col.dtype)


_keys = {}


def make_keys(ctx, name, size, seed=0):
    """`size` sorted keys for this column, made once and shared: test_in_list_gpu.make_list's elements (hits, 1-ulp near-misses, exception values, the
    other zero, +-inf), a quarter of them twice"""
    key = (name, size, seed)
    if key not in _keys:
        col, xs, ev = column(ctx, name)
        dup = size // 4
        base = make_list(xs, size - dup, 1000 * seed + size, ev)
        _keys[key] = np.sort(np.concatenate([base, base[:dup]]))
        assert _keys[key].size == size
    return _keys[key]


def payload(n_keys, seed=3):
    return ROW_BASE + np.random.default_rng(seed).permutation(n_keys).astype(np.int64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def probe(ctx, col, keys, mask=None, rows=None, span=True, idx=True, zones=None, capacity=None, room=None):
    """one call of the raw form into poisoned buffers of `room` rows (default: the capacity) + GUARD: (count, pos, span, idx) as numpy, whole buffers"""
    total = col.n_vectors * 1024
    capacity = total if capacity is None else capacity
    room = capacity if room is None else room
    pos = torch.full((room + GUARD,), CANARY64, dtype=torch.int64, device=DEV)
    spn = torch.full((room + GUARD,), CANARY32, dtype=torch.int32, device=DEV) if span else None
    ix = torch.full((room + GUARD,), CANARY64, dtype=torch.int64, device=DEV) if idx else None
    count = torch.full((1,), CANARY64, dtype=torch.int64, device=DEV)
    ctx.join_probe_into(col, keys if isinstance(keys, torch.Tensor) else dev(keys), pos[:capacity] if capacity else None, count, mask=mask,
                        rows=None if rows is None else (rows if isinstance(rows, torch.Tensor) else dev(rows)), span_out=spn[:capacity] if span and capacity else None,
                        idx_out=ix[:capacity] if idx and capacity else None, zones=zones)
    ctx.synchronize()
    return int(count.item()), pos.cpu().numpy(), None if spn is None else spn.cpu().numpy().view(np.uint32), None if ix is None else ix.cpu().numpy()


def check(got, want, capacity, what):
    """got: probe()'s tuple; want: host_join()'s (idx, pos, span).  The first min(count, capacity) rows equal the replica's, everything behind is canary."""
    count, pos, spn, ix = got
    widx, wpos, wspan = want
    assert count == widx.size, f"{what}: count {count}, expected {widx.size}"
    k = min(count, capacity)
    assert np.array_equal(pos[:k], wpos[:k]), f"{what}: positions differ from the replica"
    assert (pos[k:] == CANARY64).all(), f"{what}: a position was written behind row {k}"
    if spn is not None:
        assert np.array_equal(spn[:k], wspan[:k]), f"{what}: spans differ from the replica"
        assert (spn[k:] == CANARY32).all(), f"{what}: a span was written behind row {k}"
    if ix is not None:
        assert np.array_equal(ix[:k], widx[:k]), f"{what}: indices differ from the set bits"
        assert (ix[k:] == CANARY64).all(), f"{what}: an index was written behind row {k}"


# ---- 1. every key-list size on every kind of column ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_key_lists_of_every_size_against_the_replica(ctx, name):
    col, xs, ev = column(ctx, name)
    L = lds_max(col)
    mask = random_mask(col.n_vectors, 1)
    words = mask.cpu().numpy()
    hit_exception = False
    exc = exception_indices(col)
    for size in (0, 1, 2, 3, 63, 64, 65, L - 1, L, L + 1, 2 * L + 1, 3 * L - 1):  # the last three: strides 2, 3 and 3
        keys = make_keys(ctx, name, size)
        rows = payload(size)
        for m, w in ((None, None), (mask, words)):
            want = host_join(xs, keys, w, rows)
            check(probe(ctx, col, keys, mask=m, rows=rows), want, xs.size, f"{name}, {size} keys, bitmap {m is not None}")
        full = host_join(xs, keys)
        matched = int((full[1] != NO_MATCH).sum())
        assert (size == 0 and matched == 0) or 0 < matched < xs.size, f"{name}, {size} keys: the keys must match some but not all values"
        hit_exception = hit_exception or bool((full[1][exc] != NO_MATCH).any())
        if size >= 8:
            assert int(full[2].max()) >= 2, "a value sits on a duplicated key"
    assert hit_exception or exc.size == 0, f"{name}: the column has exceptions and no key matched one"


@pytest.mark.parametrize("name", ["mixed", "mixed_f32"])
def test_zeros_infinities_nans_and_neighbours(ctx, name):
    col, xs, ev = column(ctx, name)
    dt = xs.dtype.type
    assert np.any((xs == 0) & np.signbit(xs)) and np.any(np.isinf(xs)) and np.any(np.isnan(xs))
    v = xs[np.isfinite(xs) & (xs != 0)][7]
    keys = np.sort(np.array([0.0, -0.0, INF, -INF, v, np.nextafter(v, dt(INF)), np.nextafter(v, dt(-INF)), NAN, NAN], dtype=xs.dtype))
    want = host_join(xs, keys)
    check(probe(ctx, col, keys), want, xs.size, name)
    zero = xs == 0
    assert (want[2][zero] == 2).all() and len(set(want[1][zero].tolist())) == 1, "both zeros match both zero keys, at the first of them"
    assert (want[1][np.isnan(xs)] == NO_MATCH).all() and (want[2][np.isnan(xs)] == 0).all()
    assert (want[1][np.isinf(xs)] != NO_MATCH).all() and (want[2][xs == v] == 1).all()
    swapped = keys.copy()
    z = np.nonzero(keys == 0)[0]
    swapped[z[0]], swapped[z[1]] = keys[z[1]], keys[z[0]]  # the zeros in the other order: the same rows
    assert not np.array_equal(np.signbit(swapped), np.signbit(keys))
    check(probe(ctx, col, swapped), want, xs.size, name + ", zeros swapped")
    only_nans = np.full(5, NAN, dtype=xs.dtype)
    check(probe(ctx, col, only_nans), host_join(xs, only_nans), xs.size, name + ", NaN keys only")


# ---- 2. equal runs in the pivot tier -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "mixed_f32"])
def test_equal_runs_that_straddle_pivots(ctx, name):
    col, xs, ev = column(ctx, name)
    L = lds_max(col)
    finite = np.unique(xs[np.isfinite(xs)])
    for n_keys in (2 * L + 1, 3 * L - 1):
        stride = -(-n_keys // L)
        run = 3 * stride + 1
        others = make_keys(ctx, name, n_keys)
        others = others[np.isfinite(others)]
        for where, v in (("start", finite[0]), ("middle", finite[finite.size // 2]), ("end", finite[-1])):
            rest = others[others != v]
            rest = rest[rest > v] if where == "start" else rest[rest < v] if where == "end" else rest
            rest = rest[: n_keys - run] if where != "end" else rest[rest.size - min(rest.size, n_keys - run):]
            keys = np.sort(np.concatenate([rest, np.full(run, v, dtype=xs.dtype)]))
            assert -(-keys.size // L) == stride, "the run straddles several pivots of this stride"
            first = int(np.nonzero(keys == v)[0][0])
            assert (where != "start" or first == 0) and (where != "end" or first + run == keys.size)
            rows = payload(keys.size)
            want = host_join(xs, keys, None, rows)
            at = xs == v
            assert at.any() and (want[1][at] == rows[first]).all() and (want[2][at] == run).all()
            check(probe(ctx, col, keys, rows=rows), want, xs.size, f"{name}, {keys.size} keys, a run of {run} at the {where}")
            check(probe(ctx, col, keys), host_join(xs, keys), xs.size, f"{name}, {keys.size} keys, a run of {run} at the {where}, positions")
        assert stride in (2, 3)


# ---- 3. bitmaps ---------------------------------------------------------------------------------------------------------------------------------------
def bitmaps(col, xs):
    nv = col.n_vectors
    rnd = random_mask(nv, 4)
    upper = rnd.clone().reshape(-1, 16)
    upper[:, :8] = 0
    last = torch.zeros_like(rnd)
    last[-1] = -(2**63)  # bit 63 of the last word of the last vector
    nan_exc = np.zeros(xs.size, dtype=bool)
    e = exception_indices(col)
    nan_exc[e[np.isnan(xs[e])]] = True
    return {"none": None, "full": torch.full_like(rnd, -1), "empty": torch.zeros_like(rnd), "random": rnd, "every third vector": vectors_cleared(rnd, 3, 0),
            "upper halves": upper.reshape(-1), "the last bit": last, "NaN exceptions": dev(pack_bits(nan_exc).view(np.int64))}


@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_every_shape_of_bitmap(ctx, name):
    col, xs, ev = column(ctx, name)
    L = lds_max(col)
    for size in (65, L + 1):
        keys = make_keys(ctx, name, size)
        rows = payload(size)
        for bname, m in bitmaps(col, xs).items():
            w = None if m is None else m.cpu().numpy()
            want = host_join(xs, keys, w, rows)
            if bname == "NaN exceptions":
                assert (want[0].size > 0 or "rd" in name) and (want[1] == NO_MATCH).all()
            if bname == "the last bit":
                assert want[0].tolist() == [xs.size - 1]
            if bname == "upper halves":
                assert ((want[0] % 1024) >= 512).all() and want[0].size > 0
            check(probe(ctx, col, keys, mask=m, rows=rows), want, xs.size, f"{name}, {size} keys, bitmap: {bname}")


# ---- 4. capacity -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "rd_unit_f32"])
def test_every_capacity_and_the_canaries_behind_it(ctx, name):
    col, xs, ev = column(ctx, name)
    keys = make_keys(ctx, name, lds_max(col) + 1)
    rows = payload(keys.size)
    rnd = random_mask(col.n_vectors, 8)
    for bname, m in (("none", None), ("random", rnd), ("every third vector", vectors_cleared(rnd, 3, 0))):
        w = None if m is None else m.cpu().numpy()
        want = host_join(xs, keys, w, rows)
        count = want[0].size
        per_vector = np.ones(col.n_vectors, int) * 1024 if w is None else unpack_bits(w).reshape(-1, 1024).sum(axis=1)
        v_cut = int(np.nonzero(per_vector)[0][2])  # inside the third vector that holds a bit, and inside a word of it
        inside = int(per_vector[:v_cut].sum()) + int(per_vector[v_cut]) // 2 + 1
        assert per_vector[:v_cut].sum() < inside < per_vector[:v_cut + 1].sum()
        for cap in (0, 1, count - 1, count, inside):
            check(probe(ctx, col, keys, mask=m, rows=rows, capacity=cap), want, cap, f"{name}, bitmap {bname}, capacity {cap} of {count}")
        if count < xs.size:  # room behind the count: nothing is written at j >= count
            check(probe(ctx, col, keys, mask=m, rows=rows, capacity=count + 50), want, count + 50, f"{name}, bitmap {bname}, capacity above the count")
        # capacity 0 with NULL outputs: a count
        cnt = torch.full((1,), CANARY64, dtype=torch.int64, device=DEV)
        ctx.join_probe_into(col, dev(keys), None, cnt, mask=m)
        assert int(cnt.item()) == count


# ---- 5. which outputs are asked for ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_every_combination_of_span_idx_and_rows(ctx, name):
    col, xs, ev = column(ctx, name)
    rnd = random_mask(col.n_vectors, 9)
    for size in (65, lds_max(col) + 1):
        keys = make_keys(ctx, name, size)
        rows = payload(size)
        for m in (None, rnd):
            w = None if m is None else m.cpu().numpy()
            for with_rows in (False, True):
                want = host_join(xs, keys, w, rows if with_rows else None)
                if with_rows:
                    assert (want[1][want[1] != NO_MATCH] >= ROW_BASE).all()
                for span in (False, True):
                    for idx in (False, True):
                        check(probe(ctx, col, keys, mask=m, rows=rows if with_rows else None, span=span, idx=idx), want, xs.size,
                              f"{name}, {size} keys, bitmap {m is not None}, rows {with_rows}, span {span}, idx {idx}")


# ---- 6. zone maps ------------------------------------------------------------------------------------------------------------------------------------------
def sorted_column(ctx, f32):
    key = "sorted_f32" if f32 else "sorted"
    if key not in _cache:
        raw = datagen.mixed_column_f32(64, seed=31) if f32 else datagen.mixed_column(64, seed=31)
        s = np.sort(raw[~np.isnan(raw)])
        s = np.ascontiguousarray(s[: s.size // 1024 * 1024])
        col = ctx.encode(dev(s))
        xs = ctx.decode(col).cpu().numpy()
        assert np.array_equal(xs.view(np.uint8), s.view(np.uint8))
        _cache[key] = (col, xs, ())
    return _cache[key]


@pytest.mark.parametrize("f32", [False, True])
def test_zone_maps_change_no_byte(ctx, f32):
    most_settled = False
    for cname, (col, xs, ev) in (("random", column(ctx, "mixed_f32" if f32 else "mixed")), ("sorted", sorted_column(ctx, f32))):
        nv = col.n_vectors
        L = lds_max(col)
        zones = ctx.zone_map(col)
        wide = zones.clone()
        wide[:, 0] -= 1.0
        wide[:, 1] += 1.0
        everything = torch.empty_like(zones)
        everything[:, 0], everything[:, 1] = -INF, INF
        holes = zones.clone()
        holes[::3, 0] = NAN  # a NaN bound: decode the vector
        holes[1::3, 1] = NAN
        lists = [("drawn %d" % size, np.sort(make_list(xs, size, 70 + size, ev))) for size in (0, 1, 5, 65, L, L + 1, 2 * L + 1)]
        if cname == "sorted":
            u = np.unique(xs[np.isfinite(xs)])
            lists.append(("clustered", np.ascontiguousarray(u[100:140])))  # neighbours in value: a few vectors
        rnd = vectors_cleared(random_mask(nv, 12), 3, 0)
        for lname, keys in lists:
            rows = payload(keys.size)
            for m in (None, rnd):
                w = None if m is None else m.cpu().numpy()
                want = host_join(xs, keys, w, rows)
                plain = probe(ctx, col, keys, mask=m, rows=rows)
                check(plain, want, xs.size, f"{cname}, {lname}: without zones")
                for zname, z in (("the zone map", zones), ("widened", wide), ("all-admitting", everything), ("NaN bounds", holes)):
                    got = probe(ctx, col, keys, mask=m, rows=rows, zones=z)
                    assert got[0] == plain[0] and all(np.array_equal(a, b) for a, b in zip(got[1:], plain[1:])), f"{cname}, {lname}: {zname} changed the bytes"
            if cname == "sorted" and keys.size:
                zn = zones.cpu().numpy()
                real = keys[~np.isnan(keys)]
                at = np.searchsorted(real, zn[:, 0], side="left")
                settled = (at >= real.size) | (real[np.minimum(at, real.size - 1)] > zn[:, 1])  # no key in [min, max], by the definition
                most_settled = most_settled or settled.mean() > 0.5
    assert most_settled, "no short list left most vectors of the sorted column to their records"


# ---- 7. robustness: unsorted keys, lying zones -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "mixed_f32"])
def test_unsorted_keys_and_lying_zones_stay_in_bounds(ctx, name):
    col, xs, ev = column(ctx, name)
    L = lds_max(col)
    zones = ctx.zone_map(col)
    rnd = random_mask(col.n_vectors, 14)
    for size in (65, L, 2 * L + 1):
        sorted_keys = make_keys(ctx, name, size)
        shuffled = np.random.default_rng(size).permutation(sorted_keys)
        assert not np.array_equal(np.sort(shuffled)[:8], shuffled[:8])
        rows = payload(size)
        lies = {"shifted": torch.roll(zones, 5, dims=0), "inverted": zones.flip(1).contiguous(), "all one point": torch.zeros_like(zones)}
        for kname, keys, z in [("unsorted", shuffled, None), ("unsorted with zones", shuffled, zones)] + [("lying zones: " + k, sorted_keys, v) for k, v in lies.items()]:
            for m in (None, rnd):
                w = None if m is None else m.cpu().numpy()
                widx = host_join(xs, sorted_keys, w)[0]
                for with_rows in (False, True):
                    what = f"{name}, {size} keys, {kname}, bitmap {m is not None}, rows {with_rows}"
                    count, pos, spn, ix = probe(ctx, col, keys, mask=m, rows=rows if with_rows else None, zones=z)
                    assert count == widx.size and np.array_equal(ix[:count], widx), what + ": count and indices are exact"
                    p, s = pos[:count], spn[:count]
                    lo = ROW_BASE if with_rows else 0
                    assert (((p >= lo) & (p < lo + size)) | (p == NO_MATCH)).all(), what + ": a position outside the keys"
                    assert (s <= size).all(), what + ": a span above n_keys"
                    assert (pos[count:] == CANARY64).all() and (spn[count:] == CANARY32).all() and (ix[count:] == CANARY64).all(), what + ": written behind the rows"


# ---- 8. an empty column and the argument checks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_no_vectors_and_every_refused_call(ctx, dtype):
    name = "mixed" if dtype == "f64" else "mixed_f32"
    col, xs, ev = column(ctx, name)
    vb = 8 if dtype == "f64" else 4
    fn = getattr(capi.lib, "alpgpu_join_probe_" + dtype)
    keys = dev(make_keys(ctx, name, 65))
    rows = dev(payload(65))
    zones = ctx.zone_map(col)
    mask = random_mask(col.n_vectors, 10)
    scratch = ctx.select_scratch(col)
    cap = 256
    pos = torch.full((cap + 1,), CANARY64, dtype=torch.int64, device=DEV)
    spn = torch.full((cap + 1,), CANARY32, dtype=torch.int32, device=DEV)
    ix = torch.full((cap + 1,), CANARY64, dtype=torch.int64, device=DEV)
    count = torch.full((2,), CANARY64, dtype=torch.int64, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    c = ctypes.byref(col.c)
    # a column without vectors: the count alone is written, with or without a bitmap pointer, scratch or outputs
    empty = capi.CColumn()
    for args in ((None, None, p(keys), 65, p(rows), p(pos), p(spn), p(ix), cap, p(count), None), (None, None, None, 0, None, None, None, None, 0, p(count), None),
                 (p(mask), None, p(keys), 65, None, p(pos), None, None, cap, p(count), None)):
        count.fill_(CANARY64)
        assert fn(ctx.h, ctypes.byref(empty), *args) == 0
        ctx.synchronize()
        assert count.tolist() == [0, CANARY64]
    count.fill_(CANARY64)
    refused = {
        "a NULL context": (None, c, p(mask), None, p(keys), 65, p(rows), p(pos), p(spn), p(ix), cap, p(count), p(scratch)),
        "a NULL column": (ctx.h, None, p(mask), None, p(keys), 65, p(rows), p(pos), p(spn), p(ix), cap, p(count), p(scratch)),
        "a NULL count": (ctx.h, c, p(mask), None, p(keys), 65, p(rows), p(pos), p(spn), p(ix), cap, None, p(scratch)),
        "a NULL d_pos with a capacity": (ctx.h, c, p(mask), None, p(keys), 65, p(rows), None, p(spn), p(ix), cap, p(count), p(scratch)),
        "a NULL scratch with a bitmap": (ctx.h, c, p(mask), None, p(keys), 65, p(rows), p(pos), p(spn), p(ix), cap, p(count), None),
        "a NULL scratch with a bitmap, counting": (ctx.h, c, p(mask), None, p(keys), 65, None, None, None, None, 0, p(count), None),
        "a misaligned scratch": (ctx.h, c, p(mask), None, p(keys), 65, p(rows), p(pos), p(spn), p(ix), cap, p(count), p(scratch, 8)),
        "NULL keys with n_keys > 0": (ctx.h, c, None, None, None, 65, p(rows), p(pos), p(spn), p(ix), cap, p(count), None),
        "n_keys of 2^31": (ctx.h, c, None, None, p(keys), 2**31, p(rows), p(pos), p(spn), p(ix), cap, p(count), None),
        "n_keys of 2^40": (ctx.h, c, None, None, p(keys), 2**40, None, p(pos), None, None, cap, p(count), None),
        "a misaligned bitmap": (ctx.h, c, p(mask, 4), None, p(keys), 65, p(rows), p(pos), p(spn), p(ix), cap, p(count), p(scratch)),
        "misaligned zones": (ctx.h, c, None, p(zones, vb), p(keys), 65, p(rows), p(pos), p(spn), p(ix), cap, p(count), None),
        "misaligned keys": (ctx.h, c, None, None, p(keys, vb // 2), 64, p(rows), p(pos), p(spn), p(ix), cap, p(count), None),
        "misaligned rows": (ctx.h, c, None, None, p(keys), 65, p(rows, 4), p(pos), p(spn), p(ix), cap, p(count), None),
    }
    for what, args in refused.items():
        assert fn(*args) == -2, what + " must be refused"
    ctx.synchronize()
    assert (pos == CANARY64).all() and (spn == CANARY32).all() and (ix == CANARY64).all() and (count == CANARY64).all(), "a refused call wrote"
    # and the same arguments, put right, are accepted: without a bitmap no scratch is needed
    assert fn(ctx.h, c, None, None, p(keys), 65, p(rows), p(pos), p(spn), p(ix), cap, p(count), None) == 0
    ctx.synchronize()
    assert count.tolist() == [xs.size, CANARY64] and int(pos[cap]) == CANARY64
    # NULL keys with n_keys == 0 are valid: nothing matches
    assert fn(ctx.h, c, p(mask), p(zones), None, 0, None, p(pos), p(spn), None, cap, p(count), p(scratch)) == 0
    ctx.synchronize()
    assert (pos[:cap] == NO_MATCH).all() and (spn[:cap] == 0).all() and int(pos[cap]) == CANARY64 and int(spn[cap]) == CANARY32


def test_python_rejects_arguments_that_do_not_fit(ctx, monkeypatch):
    col, xs, ev = column(ctx, "mixed")
    cf = column(ctx, "mixed_f32")[0]
    keys = dev(make_keys(ctx, "mixed", 65))
    count = torch.zeros(1, dtype=torch.int64, device=DEV)
    pos = torch.full((100,), 7, dtype=torch.int64, device=DEV)

    def unreachable(*a, **k):
        raise AssertionError("the library was called")
    for t in ("f64", "f32"):
        monkeypatch.setattr(capi.lib, "alpgpu_join_probe_" + t, unreachable)
    for bad in (keys.to(torch.float32), keys.cpu(), keys.reshape(5, 13), [1.0, 2.0]):
        with pytest.raises(ValueError):
            ctx.join_probe_into(col, bad, pos, count)
    with pytest.raises(ValueError):
        ctx.join_probe_into(cf, keys, pos, count)  # a float column takes float keys
    for kw in ({"span_out": torch.zeros(99, dtype=torch.int32, device=DEV)}, {"span_out": torch.zeros(100, dtype=torch.int64, device=DEV)},
               {"idx_out": torch.zeros(99, dtype=torch.int64, device=DEV)}, {"rows": torch.zeros(64, dtype=torch.int64, device=DEV)},
               {"rows": torch.zeros(65, dtype=torch.int32, device=DEV)}, {"mask": torch.zeros(16 * col.n_vectors - 16, dtype=torch.int64, device=DEV)},
               {"zones": torch.zeros((col.n_vectors, 2), dtype=torch.float32, device=DEV)},
               {"mask": random_mask(col.n_vectors, 1), "scratch": torch.zeros(8, dtype=torch.uint8, device=DEV)}):
        with pytest.raises(ValueError):
            ctx.join_probe_into(col, keys, pos, count, **kw)
    for bad_count in (count.to(torch.int32), count.cpu(), count[:0]):
        with pytest.raises(ValueError):
            ctx.join_probe_into(col, keys, pos, bad_count)
    with pytest.raises(ValueError):
        ctx.join_probe(col, keys.to(torch.float32))
    with pytest.raises(ValueError):
        ctx.join_probe(col, keys, rows=torch.zeros(3, dtype=torch.int64, device=DEV), sorted=True)
    ctx.synchronize()
    assert bool((pos == 7).all()), "a refused call launched"


def test_the_allocating_form_sorts_and_maps_back(ctx):
    """join_probe with keys in no order: pos indexes the keys as passed (rows = the sort's permutation), in every form the wrapper takes"""
    col, xs, ev = column(ctx, "mixed")
    keys_sorted = make_keys(ctx, "mixed", 300)
    uniq = np.unique(keys_sorted[~np.isnan(keys_sorted) & (keys_sorted != 0)])  # distinct: "one of the equal keys" is then the key
    shuffled = np.random.default_rng(5).permutation(uniq)
    want_idx, want_pos, want_span = host_join(xs, uniq)
    for values in (dev(shuffled), torch.from_numpy(shuffled), shuffled, shuffled.tolist()):
        pos, span, idx = ctx.join_probe(col, values, span=True, indices=True)
        pos, span, idx = pos.cpu().numpy(), span.cpu().numpy().view(np.uint32), idx.cpu().numpy()
        assert np.array_equal(idx, want_idx) and np.array_equal(span, want_span) and np.array_equal(pos != NO_MATCH, want_pos != NO_MATCH)
        hit = pos != NO_MATCH
        assert hit.any() and np.array_equal(shuffled[pos[hit]], xs[hit]), "pos indexes the keys as they were passed"
    m = random_mask(col.n_vectors, 21)
    w = m.cpu().numpy()
    pos = ctx.join_probe(col, dev(uniq), mask=m, sorted=True)
    assert np.array_equal(pos.cpu().numpy(), host_join(xs, uniq, w)[1])
    pos, idx = ctx.join_probe(col, dev(uniq), mask=m, sorted=True, indices=True, capacity=100)
    assert pos.numel() == 100 and np.array_equal(pos.cpu().numpy(), host_join(xs, uniq, w)[1][:100]) and np.array_equal(idx.cpu().numpy(), host_join(xs, uniq, w)[0][:100])
    caller_rows = torch.arange(5000, 5000 + uniq.size, dtype=torch.int64)
    pos = ctx.join_probe(col, dev(shuffled), rows=caller_rows).cpu().numpy()  # the caller's payloads follow the sort
    hit = pos != NO_MATCH
    assert np.array_equal(shuffled[pos[hit] - 5000], xs[hit])


# ---- 9. composition: the two routes of the header ------------------------------------------------------------------------------------------------------------
def test_inner_and_left_outer_join_against_the_host(ctx):
    """SELECT l.*, d.val FROM l JOIN d ON l.fk = d.key WHERE d.flag  — and the same as a LEFT JOIN"""
    rng = np.random.default_rng(77)
    nv_l, nv_d = 48, 8
    n_d = nv_d * 1024
    d_key = rng.permutation(3 * n_d)[:n_d].astype(np.float64)  # unique keys in no order
    d_val = np.round(rng.uniform(0, 100, n_d), 2)
    d_flag = rng.random(n_d) < 0.6
    l_fk = rng.integers(0, 3 * n_d, nv_l * 1024).astype(np.float64)
    c_fk, c_val = ctx.encode(dev(l_fk)), ctx.encode(dev(d_val))
    build_rows = np.nonzero(d_flag)[0].astype(np.int64)  # the filtered dimension: its keys and their row ids
    build_keys = d_key[build_rows]
    assert build_keys.size > lds_max(c_fk)
    # the host join
    order = np.argsort(build_keys, kind="stable")
    idx_h, pos_h, span_h = host_join(l_fk, build_keys[order], None, build_rows[order])
    assert (span_h <= 1).all() and 0 < int((pos_h != NO_MATCH).sum()) < l_fk.size
    want_val = np.where(pos_h != NO_MATCH, d_val[np.maximum(pos_h, 0)], NAN)
    # left outer join: join_probe alone, rows = the caller's row ids permuted by the wrapper's sort; gather turns -1 into the canonical NaN
    pos = ctx.join_probe(c_fk, dev(build_keys), rows=dev(build_rows))
    assert np.array_equal(pos.cpu().numpy(), pos_h)
    got = ctx.gather(c_val, pos).cpu().numpy()
    assert np.array_equal(got.view(np.uint64)[pos_h != NO_MATCH], want_val.view(np.uint64)[pos_h != NO_MATCH])
    assert (got.view(np.uint64)[pos_h == NO_MATCH] == 0x7FF8000000000000).all(), "no match gathers the canonical NaN"
    # inner join: the semi-join's bitmap first, then the probe under it leaves no NO_MATCH
    keys_sorted = torch.sort(dev(build_keys))
    mask = ctx.select_in_mask(c_fk, keys_sorted.values, sorted=True)
    pos, idx = ctx.join_probe(c_fk, keys_sorted.values, mask=mask, rows=dev(build_rows)[keys_sorted.indices], indices=True, sorted=True)
    hit = pos_h != NO_MATCH
    assert not bool((pos == NO_MATCH).any()) and np.array_equal(idx.cpu().numpy(), idx_h[hit]) and np.array_equal(pos.cpu().numpy(), pos_h[hit])
    assert np.array_equal(ctx.gather(c_val, pos).cpu().numpy().view(np.uint64), want_val[hit].view(np.uint64))


# ---- 10. statelessness, capture ------------------------------------------------------------------------------------------------------------------------------
def test_join_calls_leave_the_decode_plan_alone(ctx):
    for hinted in (True, False):
        raw = datagen.mixed_column(64, seed=91)
        col = ctx.encode(dev(raw))
        if hinted:
            ctx.column_totals(col)
        ctx.decode(col)
        ctx.synchronize()
        before = ctx.decode_plan(col)
        vals = raw[~np.isnan(raw)][:300]
        ctx.join_probe(col, vals, span=True)
        ctx.join_probe(col, np.concatenate([vals, np.arange(10000.0)]), mask=random_mask(64, 3), zones=ctx.zone_map(col), indices=True)
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
from join_replica import host_join
ctx = capi.Context(0)
side = torch.cuda.Stream()
ok = True
nv = 48
def draw(x, size, seed):
    rng = np.random.default_rng(seed)
    u = np.unique(x[np.isfinite(x)])
    hits = rng.choice(u, min(size // 2, u.size // 2), replace=False)
    pad = (rng.standard_normal(size - hits.size) * 4321.0).astype(x.dtype)
    return np.sort(np.concatenate([hits, pad]))
a0, b0 = datagen.mixed_column(nv, seed=81), datagen.mixed_column_f32(nv, seed=82)
cola, colb = ctx.encode(torch.from_numpy(a0).cuda()), ctx.encode(torch.from_numpy(b0).cuda())
na, nb = 65, ctx.in_list_lds_max("f32") + 9                 # the LDS tier and the global tier
ka, kb = torch.from_numpy(draw(a0, na, 1)).cuda(), torch.from_numpy(draw(b0, nb, 2)).cuda()
rows = torch.from_numpy(np.random.default_rng(9).permutation(nb).astype(np.int64) + 1000000).cuda()
mask = torch.from_numpy(np.random.default_rng(5).integers(0, 2**64, 16 * nv, dtype=np.uint64).view(np.int64)).cuda()
total = nv * 1024
out = {k: (torch.zeros(total, dtype=torch.int64, device="cuda:0"), torch.zeros(total, dtype=torch.int32, device="cuda:0"), torch.zeros(total, dtype=torch.int64, device="cuda:0"),
           torch.zeros(1, dtype=torch.int64, device="cuda:0")) for k in ("a", "b")}
scratch = ctx.select_scratch(colb)
def calls():
    pos, spn, idx, cnt = out["a"]
    ctx.join_probe_into(cola, ka, pos, cnt, span_out=spn, idx_out=idx)                                        # without a bitmap: no scratch, the count by a kernel
    pos, spn, idx, cnt = out["b"]
    ctx.join_probe_into(colb, kb, pos, cnt, mask=mask, rows=rows, span_out=spn, idx_out=idx, scratch=scratch)  # with one
with torch.cuda.stream(side):
    calls()                                                 # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        calls()
xa, xb = ctx.decode(cola).cpu().numpy(), ctx.decode(colb).cpu().numpy()
for rep in range(3):
    if rep > 0:                                             # other keys written into the same tensors, another bitmap into the same words
        ka.copy_(torch.from_numpy(draw(a0, na, 10 + rep))); kb.copy_(torch.from_numpy(draw(b0, nb, 20 + rep)))
        mask.copy_(torch.from_numpy(np.random.default_rng(30 + rep).integers(0, 2**64, 16 * nv, dtype=np.uint64).view(np.int64)))
        if rep == 2:
            mask.reshape(-1, 16)[::2] = 0
    torch.cuda.synchronize()
    for t in out.values():
        for u in t:
            u.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    for name, x, keys, m, r in (("a", xa, ka, None, None), ("b", xb, kb, mask.cpu().numpy(), rows.cpu().numpy())):
        widx, wpos, wspan = host_join(x, keys.cpu().numpy(), m, r)
        pos, spn, idx, cnt = [t.cpu().numpy() for t in out[name]]
        k = widx.size
        good = int(cnt[0]) == k and np.array_equal(pos[:k], wpos) and np.array_equal(spn[:k].view(np.uint32), wspan) and np.array_equal(idx[:k], widx)
        good = good and (pos[k:] == -7).all() and 0 < int((wpos >= 0).sum()) < k
        ok = ok and bool(good)
        print(rep, name, k, bool(good))
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_keys_and_the_bitmap_change():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 11. the C++ wrapper ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cpp_column_join_probe_against_decompress_and_a_host_loop(ctx, tmp_path, dtype):
    """include/alp/batch.hpp: alp::gpu::column<double / float>::join_probe of a serialized column against column::decompress and a host loop over the
    definition (tests/cpp/join_test.cpp)"""
    exe = tmp_path / "join_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/join_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    cases = datagen.adversarial_vectors() if dtype == "f64" else datagen.adversarial_vectors_f32()  # NaN, +-inf and -0.0 among the values
    raw = np.concatenate([cases[k] for k in sorted(cases)])
    col = ctx.encode(dev(raw))
    assert col.n_vectors <= 64
    xs = ctx.decode(col).cpu().numpy()
    ctx.to_blob(col, xs.size).tofile(str(tmp_path / "col.blob"))
    base = make_list(xs, 40, 5)
    keys = np.concatenate([base, base[:7], np.array([NAN, NAN], dtype=xs.dtype)])  # in no order, duplicates, NaNs
    keys.tofile(str(tmp_path / "keys.bin"))
    mask = vectors_cleared(random_mask(col.n_vectors, 53), 3, -1)
    mask[16:32] = 0
    mask.cpu().numpy().tofile(str(tmp_path / "in.mask"))
    p = subprocess.run([str(exe), dtype] + [str(tmp_path / f) for f in ("col.blob", "keys.bin", "in.mask")], capture_output=True, text=True, timeout=600)
    line = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("ok ")]
    assert p.returncode == 0 and len(line) == 1, p.stdout[-3000:] + p.stderr[-2000:]
    widx, wpos, wspan = host_join(xs, np.sort(keys), mask.cpu().numpy())
    assert [int(t) for t in line[0][1:]] == [col.n_vectors, widx.size, int((wspan > 0).sum())] and 0 < int((wspan > 0).sum()) < widx.size
