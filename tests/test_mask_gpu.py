"""GPU: selection bitmaps (include/alpgpu.h, "selection bitmaps": alpgpu_select_mask_*, alpgpu_mask_to_indices, alpgpu_decode_sum_masked_*).  The
expected result never comes from the code under test: x = ctx.decode(col) (pinned to the oracle and the reference by other suites), the
predicate in torch, bits packed 64 to a word in index order.  Bitmaps compare as integers, sums on their int64 views against a host replica of
the documented summation order (host_sums_masked below)."""
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
    """bool tensor of whole vectors -> the bitmap: bit r & 63 of int64 word r >> 6 = bits[r] (the 64 terms of a word are disjoint powers of two,
    so the wrapping int64 sum is their OR)"""
    w = torch.ones(64, dtype=torch.int64, device=bits.device) << torch.arange(64, dtype=torch.int64, device=bits.device)
    return (bits.reshape(-1, 64).to(torch.int64) * w).sum(dim=1)


def unpack(mask):
    s = torch.arange(64, dtype=torch.int64, device=mask.device)
    return (((mask.reshape(-1, 1) >> s) & 1) != 0).reshape(-1)


def random_mask(n_vectors, seed):
    words = np.random.default_rng(seed).integers(0, 2**64, 16 * n_vectors, dtype=np.uint64)
    return torch.from_numpy(words.view(np.int64)).to(DEV)


def vectors_cleared(mask, keep_every, fill):
    """the mask with every vector but each keep_every-th set to `fill` (0 or -1) in all 16 words: skipped vectors beside decoded ones, also
    inside one workgroup of four wavefronts"""
    m = mask.clone().reshape(-1, 16)
    v = torch.arange(m.shape[0], device=mask.device)
    m[(v % keep_every) != 1] = fill
    return m.reshape(-1)


def in_range(total, first, n):
    r = torch.arange(total, device=DEV)
    return (r >= first) & (r < first + n)


def qualify(x, lo, hi, first=0, n=None):
    n = x.numel() - first if n is None else n
    return (x >= lo) & (x <= hi) & in_range(x.numel(), first, n)


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


def adversarial_column(cases):
    return np.concatenate([cases[k] for k in sorted(cases)])


COLUMNS = {
    "mixed": lambda: datagen.mixed_column(250, seed=5),
    "rd_unit": lambda: datagen.rd_column(250, seed=6),
    "rd_latlon": lambda: datagen.rd_column(250, seed=7, kind="latlon"),
    "drifting": lambda: datagen.drifting_column(250, seed=8),
    "every_width_exc": lambda: datagen.every_bit_width_column(208, seed=9, exceptions=True),
    "every_width": lambda: datagen.every_bit_width_column(208, seed=10, exceptions=False),
    "adversarial": lambda: adversarial_column(datagen.adversarial_vectors()),
    "mixed_f32": lambda: datagen.mixed_column_f32(250, seed=5),
    "rd_unit_f32": lambda: datagen.rd_column_f32(250, seed=6),
    "rd_latlon_f32": lambda: datagen.rd_column_f32(250, seed=7, kind="latlon"),
    "drifting_f32": lambda: datagen.drifting_column_f32(250, seed=8),
    "every_width_exc_f32": lambda: datagen.every_bit_width_column_f32(200, seed=9, exceptions=True),
    "every_width_f32": lambda: datagen.every_bit_width_column_f32(200, seed=10, exceptions=False),
    "adversarial_f32": lambda: adversarial_column(datagen.adversarial_vectors_f32()),
}
WITH_SPECIALS = ("mixed", "mixed_f32", "adversarial", "adversarial_f32")  # NaN, +-inf and -0.0 are planted in these
_cache = {}


def column(ctx, name):
    """(DeviceColumn, its store decode), encoded once per session and left unchanged"""
    if name not in _cache:
        xd = torch.from_numpy(np.ascontiguousarray(COLUMNS[name]())).to(DEV)
        col = ctx.encode(xd)
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(xd)), f"{name}: decode(encode(x)) != x"
        _cache[name] = (col, dec)
    return _cache[name]


def bounds(dec, f_lo, f_hi):
    xs = dec.cpu().numpy()
    s = np.sort(xs[np.isfinite(xs)])
    return float(s[int(f_lo * s.size)]), float(s[min(s.size - 1, int(f_hi * s.size))])


# ---- 1. SET against the decode ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_set_on_every_column_kind_against_the_store_decode(ctx, name):
    col, x = column(ctx, name)
    total = x.numel()
    exc_idx = exception_indices(col)
    preds = battery(x, name in WITH_SPECIALS)
    if exc_idx.size:
        ev = x[torch.from_numpy(exc_idx).to(DEV)].cpu().numpy()
        cand = ev[np.isfinite(ev)] if np.isfinite(ev).any() else ev[~np.isnan(ev)]
        if cand.size:
            v = float(np.sort(cand)[cand.size // 2])
            preds.append(("exception value", v, v))
    exc_set = torch.zeros(total, dtype=torch.bool, device=DEV)
    exc_set[torch.from_numpy(exc_idx).to(DEV)] = True
    partial, hit_exception = False, False
    mask = random_mask(col.n_vectors, 1)  # SET writes every word: what the bitmap held does not matter
    for pname, lo, hi in preds:
        tag = f"{name}/{pname}"
        q = (x >= lo) & (x <= hi)
        got = ctx.select_mask(col, lo, hi, mask=mask)
        assert got is mask and torch.equal(mask, pack(q)), f"{tag}: bitmap differs from (x >= lo) & (x <= hi) of the store decode"
        per_vector = unpack(mask).reshape(-1, 1024).sum(dim=1).to(torch.int32)
        assert torch.equal(per_vector, ctx.decode_count_range(col, lo, hi).view(torch.int32)), f"{tag}: popcounts != decode_count_range"
        idx = ctx.mask_to_indices(mask)
        assert torch.equal(idx, ctx.select_range(col, lo, hi)), f"{tag}: mask_to_indices != select_range"
        assert torch.equal(idx, torch.nonzero(q).reshape(-1)), f"{tag}: mask_to_indices != nonzero of the predicate"
        partial = partial or 0 < idx.numel() < total
        hit_exception = hit_exception or bool(exc_set[idx].any())
    assert partial, f"{name}: no predicate of the battery selects some but not all values"
    assert hit_exception or exc_idx.size == 0, f"{name}: the column has exceptions and no predicate selected one"
    fresh = ctx.select_mask(col, *bounds(x, 0.3, 0.7))  # the allocating form
    assert fresh.dtype == torch.int64 and fresh.numel() == 16 * col.n_vectors and torch.equal(fresh, pack(qualify(x, *bounds(x, 0.3, 0.7))))


# ---- 2. ranges ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "mixed_f32"])
def test_first_and_n_under_every_op(ctx, name):
    col, x = column(ctx, name)
    total = x.numel()
    lo, hi = bounds(x, 0.2, 0.8)
    prior = random_mask(col.n_vectors, 2)
    pb = unpack(prior)
    ranges = [(3 * 1024 + 17, 500), (3 * 1024 + 17, 1), (63, 1), (63, 2), (64, 64), (65, 63), (1024 + 63, 66), (5 * 1024 - 100, 300), (5 * 1024, 1024), (5 * 1024 - 1, 1026),
              (99 * 1024 + 1000, 101 * 1024), (total - 1, 1), (0, total), (0, total - 500), (0, 0), (777, 0), (total, 0), (1023, 2)]
    for first, n in ranges:
        q = qualify(x, lo, hi, first, n)
        want = {"set": q, "and": pb & q, "or": pb | q}
        for op in OPS:
            mask = prior.clone()
            ctx.select_mask(col, lo, hi, first=first, n=n, op=op, mask=mask)
            assert torch.equal(mask, pack(want[op])), f"{name} first={first} n={n} op={op}"
        assert n < 2000 or bool(q.any())
    # ranges past the end, and a first + n that overflows, are refused on the host: the bitmap is unchanged
    fn = getattr(capi.lib, "alpgpu_select_mask_" + col.dtype)
    mask = prior.clone()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for first, n in ((total - 100, 101), (0, total + 1), (total + 1, 0), (2**64 - 1, 2), (2, 2**64 - 1), (2**63, 2**63)):
        for op in OPS.values():
            assert fn(ctx.h, ctypes.byref(col.c), first, n, lo, hi, op, p(mask)) == -2, f"range ({first}, {n}) must be refused"
    ctx.synchronize()
    assert torch.equal(mask, prior), "a refused select_mask wrote"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_single_vector_and_an_empty_column(ctx, dtype):
    cases = datagen.adversarial_vectors() if dtype == "f64" else datagen.adversarial_vectors_f32()
    for name in ("plain", "all_exceptions", "all_zero", "half_negzero", "inf_ends", "prefix_nan"):
        col = ctx.encode(torch.from_numpy(cases[name]).to(DEV))
        assert col.n_vectors == 1
        x = ctx.decode(col)
        prior = random_mask(1, 3)
        for pname, lo, hi in battery(x, True):
            for first, n in ((0, 1024), (1023, 1), (63, 2), (100, 900)):
                q = qualify(x, lo, hi, first, n)
                for op, want in (("set", q), ("and", unpack(prior) & q), ("or", unpack(prior) | q)):
                    mask = prior.clone()
                    ctx.select_mask(col, lo, hi, first=first, n=n, op=op, mask=mask)
                    assert torch.equal(mask, pack(want)), f"{name}/{pname} first={first} n={n} op={op}"
    empty = capi.CColumn()
    fn = getattr(capi.lib, "alpgpu_select_mask_" + dtype)
    for op in OPS.values():
        assert fn(ctx.h, ctypes.byref(empty), 0, 0, -INF, INF, op, None) == 0
        assert fn(ctx.h, ctypes.byref(empty), 0, 1, -INF, INF, op, None) == -2
    count = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    assert capi.lib.alpgpu_mask_to_indices(ctx.h, None, 0, None, 0, ctypes.c_void_p(count.data_ptr()), None) == 0
    ctx.synchronize()
    assert int(count) == 0
    assert getattr(capi.lib, "alpgpu_decode_sum_masked_" + dtype)(ctx.h, ctypes.byref(empty), None, None, None) == 0


# ---- 3. AND and OR against a prior bitmap ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "rd_unit", "every_width_exc", "adversarial", "mixed_f32", "rd_latlon_f32"])
def test_and_or_against_prior_bitmaps(ctx, name):
    col, x = column(ctx, name)
    nv, total = col.n_vectors, x.numel()
    lo, hi = bounds(x, 0.25, 0.6)
    rnd = random_mask(nv, 4)
    priors = {"zeros": torch.zeros_like(rnd), "ones": torch.full_like(rnd, -1), "random": rnd, "vectors zero": vectors_cleared(rnd, 3, 0),
              "vectors ones": vectors_cleared(rnd, 3, -1), "most vectors zero": vectors_cleared(rnd, 7, 0)}
    for pname, prior in priors.items():
        pb = unpack(prior)
        for first, n in ((0, total), (1024 + 100, total - 2048)):
            q = qualify(x, lo, hi, first, n)
            assert 0 < int(q.sum()) < n
            for op, want in (("and", pb & q), ("or", pb | q)):
                mask = prior.clone()
                ctx.select_mask(col, lo, hi, first=first, n=n, op=op, mask=mask)
                assert torch.equal(mask, pack(want)), f"{name}: {op} into {pname}, first={first} n={n}"


# ---- 4. two and three columns end to end ----------------------------------------------------------------------------------------------------------
def test_three_columns_end_to_end(ctx):
    (ca, a), (cb, b), (cc, c) = column(ctx, "mixed"), column(ctx, "rd_unit_f32"), column(ctx, "drifting")
    assert a.numel() == b.numel() == c.numel()
    (lo1, hi1), (lo2, hi2), (lo3, hi3) = bounds(a, 0.1, 0.6), bounds(b, 0.3, 0.9), bounds(c, 0.45, 0.5)
    mask = ctx.select_mask(ca, lo1, hi1)
    ctx.select_mask(cb, lo2, hi2, op="and", mask=mask)
    two = ctx.mask_to_indices(mask)
    want_two = ((a >= lo1) & (a <= hi1)) & ((b >= lo2) & (b <= hi2))
    assert torch.equal(two, torch.nonzero(want_two).reshape(-1)) and 0 < two.numel() < a.numel()
    ctx.select_mask(cc, lo3, hi3, op="or", mask=mask)
    idx = ctx.mask_to_indices(mask)
    want = want_two | ((c >= lo3) & (c <= hi3))
    assert torch.equal(idx, torch.nonzero(want).reshape(-1)) and two.numel() < idx.numel() < a.numel()
    for col, dec in (column(ctx, "rd_latlon"), (cc, c), column(ctx, "mixed_f32")):
        assert torch.equal(ibits(ctx.gather(col, idx)), ibits(dec)[idx])


# ---- 5. mask_to_indices on hand-made bitmaps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_vectors", [1, 1024, 1025, 2049])
def test_mask_to_indices_on_hand_made_bitmaps(ctx, n_vectors):
    total = 1024 * n_vectors
    singles = torch.zeros(total, dtype=torch.bool, device=DEV)
    singles[torch.tensor([r for r in (0, 63, 64, 1023, 1024, total - 1) if r < total], device=DEV)] = True
    alternating = torch.zeros(16 * n_vectors, dtype=torch.int64, device=DEV)
    alternating[::2] = -1
    masks = {"single bits": pack(singles), "all ones": torch.full((16 * n_vectors,), -1, dtype=torch.int64, device=DEV), "alternating words": alternating,
             "random": random_mask(n_vectors, 5), "nothing": torch.zeros(16 * n_vectors, dtype=torch.int64, device=DEV)}
    for name, mask in masks.items():
        want = torch.nonzero(unpack(mask)).reshape(-1)
        full = want.numel()
        assert torch.equal(ctx.mask_to_indices(mask), want), f"{n_vectors} vectors, {name}"
        for cap in sorted({0, 1, max(full - 1, 0), full, full + 1}):
            idx = torch.full((cap + 64,), -1, dtype=torch.int64, device=DEV)
            count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
            ctx.mask_to_indices_into(mask, idx[:cap] if cap else None, count)
            k = min(cap, full)
            assert int(count) == full, f"{n_vectors} vectors, {name}, capacity {cap}: the count is the full count whatever the capacity"
            assert torch.equal(idx[:k], want[:k]) and bool((idx[k:] == -1).all()), f"{n_vectors} vectors, {name}, capacity {cap}"
        assert torch.equal(ctx.mask_to_indices(mask, capacity=full + 9), want)


# ---- 6. decode_sum_masked ---------------------------------------------------------------------------------------------------------------------------
def pairwise_tree(p):
    """[n, 2^k] -> [n]: adjacent pairs, pairs of pairs, ..."""
    while p.shape[1] > 1:
        p = p[:, 0::2] + p[:, 1::2]
    return p[:, 0]


def host_sums_masked(values, bits):
    """the order include/alpgpu.h documents for alpgpu_decode_sum_masked_*: lane L of 64 starts from +0.0 and for m = 0..15 adds value 64 m + L
    (widened to double) if its bit is set, else does nothing; adjacent-lane tree over the 64 partials.  values, bits: [n, 1024]"""
    v = values.astype(np.float64).reshape(-1, 16, 64)
    b = bits.reshape(-1, 16, 64)
    p = np.zeros((v.shape[0], 64))
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(16):
            p = np.where(b[:, m], p + v[:, m], p)
        return pairwise_tree(p)


def host_column_total(sums):
    """alpgpu_tree_sum_f64: levels of 1024-element blocks (padded with +0.0), each reduced by the adjacent-pair tree"""
    s = np.asarray(sums, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            blocks = (s.size + 1023) // 1024
            pad = np.zeros(blocks * 1024)
            pad[: s.size] = s
            s = pairwise_tree(pad.reshape(blocks, 1024))
            if blocks == 1:
                return s[0]


def test_the_host_replica_is_a_sum():
    """on a well-conditioned column (positive decimals) the replica agrees with a plain float64 sum of the selected values to a relative 1e-9: a
    replica wrong in the same way as the kernel cannot pass the tests below"""
    rng = np.random.default_rng(3)
    x = np.round(rng.uniform(1.0, 1000.0, 40 * 1024), 2)
    bits = rng.random(x.size) < 0.37
    got = host_column_total(host_sums_masked(x.reshape(-1, 1024), bits.reshape(-1, 1024)))
    want = float(np.sum(x[bits]))
    assert abs(got - want) <= 1e-9 * abs(want)
    assert host_column_total(host_sums_masked(x.reshape(-1, 1024), np.zeros_like(bits).reshape(-1, 1024))) == 0.0


@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_decode_sum_masked_against_the_host_replica(ctx, name):
    col, x = column(ctx, name)
    nv = col.n_vectors
    xs = x.cpu().numpy().reshape(nv, 1024)
    rnd = random_mask(nv, 6)
    sparse = rnd & random_mask(nv, 7) & random_mask(nv, 8) & random_mask(nv, 9)
    masks = {"all ones": torch.full_like(rnd, -1), "all zeros": torch.zeros_like(rnd), "random": rnd, "sparse": sparse,
             "from select_mask": ctx.select_mask(col, *bounds(x, 0.2, 0.7)), "vectors zero": vectors_cleared(rnd, 3, 0)}
    for mname, mask in masks.items():
        bits = unpack(mask).cpu().numpy().reshape(nv, 1024)
        want = host_sums_masked(xs, bits)
        sums = torch.full((nv,), 7.0, dtype=torch.float64, device=DEV)
        counts = torch.full((nv,), 7, dtype=torch.int32, device=DEV)
        assert ctx.decode_sum_masked(col, mask, out=sums, counts=counts) is sums
        got = sums.cpu().numpy()
        nan = np.isnan(want)
        tag = f"{name}, mask {mname}"
        assert np.array_equal(np.isnan(got), nan), f"{tag}: NaN sums where the replica has none, or the reverse"
        assert np.array_equal(got.view(np.int64)[~nan], want.view(np.int64)[~nan]), f"{tag}: sums differ from the documented order"
        assert np.array_equal(counts.cpu().numpy(), bits.sum(axis=1).astype(np.int32)), f"{tag}: counts != popcounts"
        total, want_total = float(ctx.tree_sum(sums)), host_column_total(want)
        assert (math.isnan(total) and math.isnan(want_total)) or np.float64(total).view(np.int64) == np.float64(want_total).view(np.int64), f"{tag}: column total"
        assert torch.equal(ctx.decode_sum_masked(col, mask), sums) or bool(nan.any()), f"{tag}: without counts"
    if name in ("mixed", "mixed_f32"):  # the sum means what it says: the selected values, added up
        mask = masks["from select_mask"]
        chosen = x[unpack(mask)].to(torch.float64)
        assert abs(float(ctx.tree_sum(ctx.decode_sum_masked(col, mask))) - float(chosen.sum())) <= 1e-9 * float(chosen.abs().sum())


# ---- 7. determinism, statelessness, capture -----------------------------------------------------------------------------------------------------
def test_the_same_calls_give_the_same_bytes(ctx):
    (ca, a), (cb, b) = column(ctx, "mixed"), column(ctx, "rd_latlon")
    runs = []
    for rep in range(3):
        torch.empty(1 << (20 + rep), dtype=torch.uint8, device=DEV).fill_(rep)  # (a different allocation history each time)
        mask = ctx.select_mask(ca, *bounds(a, 0.1, 0.7))
        ctx.select_mask(cb, *bounds(b, 0.2, 0.9), op="and", mask=mask)
        idx = ctx.mask_to_indices(mask)
        counts = torch.empty(ca.n_vectors, dtype=torch.int32, device=DEV)
        sums = ctx.decode_sum_masked(ca, mask, counts=counts)
        runs.append(tuple(t.cpu().numpy().tobytes() for t in (mask, idx, sums, counts)))
    assert runs[0] == runs[1] == runs[2]
    assert 0 < len(runs[0][1]) < 8 * a.numel()


def test_mask_calls_leave_the_decode_plan_alone(ctx):
    for hinted in (True, False):
        col = ctx.encode(torch.from_numpy(datagen.mixed_column(150, seed=91)).to(DEV))
        if hinted:
            ctx.column_totals(col)
        ctx.decode(col)
        ctx.synchronize()  # (what an unhinted decode learns about the column is in by now)
        before = ctx.decode_plan(col)
        mask = ctx.select_mask(col, -5.0, 5.0)
        ctx.select_mask(col, -INF, 0.0, first=5, n=9999, op="or", mask=mask)
        ctx.select_mask(col, -100.0, 100.0, op="and", mask=mask)
        ctx.mask_to_indices(mask)
        ctx.decode_sum_masked(col, mask)
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
def q(x, f):
    s = np.sort(x[np.isfinite(x)])
    return float(s[int(f * s.size)])
a0, a1 = datagen.mixed_column(230, seed=81), datagen.mixed_column(230, seed=83)
b0, b1 = datagen.mixed_column_f32(230, seed=82), datagen.mixed_column_f32(230, seed=84)
ad, bd = [torch.from_numpy(t).cuda() for t in (a0, a1)], [torch.from_numpy(t).cuda() for t in (b0, b1)]
cola, colb = ctx.encode(ad[0]), ctx.encode(bd[0])
lo1, hi1, lo2, hi2 = q(a0, 0.2), q(a0, 0.7), q(b0, 0.1), q(b0, 0.8)
nv, cap = 230, 120 * 1024
mask = torch.zeros(16 * nv, dtype=torch.int64, device="cuda:0")
idx = torch.zeros(cap, dtype=torch.int64, device="cuda:0")
count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
sums = torch.zeros(nv, dtype=torch.float64, device="cuda:0")
counts = torch.zeros(nv, dtype=torch.int32, device="cuda:0")
scratch = ctx.select_scratch(cola)
def calls(mask, idx, count, sums, counts, scratch):
    ctx.select_mask(cola, lo1, hi1, first=1000, n=220 * 1024, mask=mask)
    ctx.select_mask(colb, lo2, hi2, op="and", mask=mask)
    ctx.mask_to_indices_into(mask, idx, count, scratch)
    ctx.decode_sum_masked(cola, mask, out=sums, counts=counts)
with torch.cuda.stream(side):
    calls(mask, idx, count, sums, counts, scratch)          # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        calls(mask, idx, count, sums, counts, scratch)
for rep in range(3):
    if rep == 1:
        ctx.encode(ad[1], cola); ctx.encode(bd[1], colb)    # other data encoded into the same buffers; rep 2 changes nothing
    torch.cuda.synchronize()
    mask.fill_(rep - 1); idx.fill_(-1); count.zero_(); sums.fill_(7.0); counts.fill_(7); scratch.fill_(rep)
    g.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in (mask, idx, count, sums, counts)]
    e = [torch.zeros_like(t) for t in got]
    e[1].fill_(-1)
    calls(*e, ctx.select_scratch(cola))
    da, db = ctx.decode(cola), ctx.decode(colb)
    m = (da >= lo1) & (da <= hi1) & (db >= lo2) & (db <= hi2); m[:1000] = False; m[1000 + 220 * 1024:] = False
    w_idx = torch.nonzero(m).reshape(-1)
    torch.cuda.synchronize()
    k = int(got[2])
    ok = ok and 0 < k <= cap and k == w_idx.numel() and torch.equal(got[1][:k], w_idx) and bool((got[1][k:] == -1).all())
    ok = ok and all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y) for x, y in zip(got, e))
    ok = ok and torch.equal(got[4].to(torch.int64), m.reshape(nv, 1024).sum(dim=1))
    ok = ok and abs(float(ctx.tree_sum(got[3])) - float(da[m].sum())) <= 1e-9 * float(da[m].abs().sum())
    print(rep, k, ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_columns_change():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 8. argument checks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c_argument_checks(ctx, dtype):
    col, x = column(ctx, "mixed" if dtype == "f64" else "mixed_f32")
    nv = col.n_vectors
    sel = getattr(capi.lib, "alpgpu_select_mask_" + dtype)
    msum = getattr(capi.lib, "alpgpu_decode_sum_masked_" + dtype)
    prior = random_mask(nv + 1, 10)
    mask = prior.clone()
    idx = torch.full((4096,), 7, dtype=torch.int64, device=DEV)
    count = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    sums = torch.full((nv,), 7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((nv,), 7, dtype=torch.int32, device=DEV)
    scratch = ctx.select_scratch(col)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    c = ctypes.byref(col.c)
    for op in (-1, 3, 17):
        assert sel(ctx.h, c, 0, 1024, -INF, INF, op, p(mask)) == -2, "a bad op must be refused"
    for op in OPS.values():
        assert sel(ctx.h, c, 0, 1024, -INF, INF, op, p(mask, 4)) == -2, "a misaligned bitmap must be refused"
        assert sel(ctx.h, c, 0, 1024, -INF, INF, op, None) == -2
        assert sel(ctx.h, None, 0, 1024, -INF, INF, op, p(mask)) == -2
    assert capi.lib.alpgpu_mask_to_indices(ctx.h, p(mask, 4), nv, p(idx), 4096, p(count), p(scratch)) == -2
    assert capi.lib.alpgpu_mask_to_indices(ctx.h, None, nv, p(idx), 4096, p(count), p(scratch)) == -2
    assert capi.lib.alpgpu_mask_to_indices(ctx.h, p(mask), nv, None, 4096, p(count), p(scratch)) == -2
    assert capi.lib.alpgpu_mask_to_indices(ctx.h, p(mask), nv, p(idx), 4096, None, p(scratch)) == -2
    assert capi.lib.alpgpu_mask_to_indices(ctx.h, p(mask), nv, p(idx), 4096, p(count), None) == -2
    assert capi.lib.alpgpu_mask_to_indices(ctx.h, p(mask), nv, p(idx), 4096, p(count), p(scratch, 8)) == -2
    assert msum(ctx.h, c, p(mask, 4), p(sums), p(counts)) == -2
    assert msum(ctx.h, c, None, p(sums), p(counts)) == -2
    assert msum(ctx.h, c, p(mask), None, p(counts)) == -2
    assert msum(ctx.h, None, p(mask), p(sums), p(counts)) == -2
    ctx.synchronize()
    assert torch.equal(mask, prior) and bool((idx == 7).all()) and int(count) == 7 and bool((sums == 7.0).all()) and bool((counts == 7).all()), "a refused call wrote"
    # n == 0: SET and AND clear the bitmap (and nothing behind it), OR enqueues nothing
    for op, cleared in ((0, True), (1, True), (2, False)):
        mask = prior.clone()
        assert sel(ctx.h, c, 0, 0, -INF, INF, op, p(mask)) == 0
        ctx.synchronize()
        assert torch.equal(mask[16 * nv:], prior[16 * nv:])
        assert bool((mask[:16 * nv] == 0).all()) if cleared else torch.equal(mask, prior)
    # counts are optional
    assert msum(ctx.h, c, p(prior), p(sums), None) == 0
    ctx.synchronize()
    assert bool((counts == 7).all())


def test_python_rejects_arguments_that_do_not_fit(ctx):
    col, x = column(ctx, "mixed")
    nv = col.n_vectors
    mask = torch.full((16 * nv,), 7, dtype=torch.int64, device=DEV)
    idx = torch.full((64,), 7, dtype=torch.int64, device=DEV)
    count = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    sums = torch.full((nv,), 7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((nv,), 7, dtype=torch.int32, device=DEV)
    wide = torch.full((32 * nv,), 7, dtype=torch.int64, device=DEV)
    bad_masks = (mask.to(torch.int32), mask.cpu(), mask[:-16], wide, wide[::2], mask.reshape(nv, 16), [1, 2, 3], np.zeros(16 * nv, np.int64))
    for bad in bad_masks:
        for op in OPS:
            with pytest.raises(ValueError):
                ctx.select_mask(col, -INF, INF, op=op, mask=bad)
        with pytest.raises(ValueError):
            ctx.decode_sum_masked(col, bad, out=sums, counts=counts)
    for bad in (mask.to(torch.int32), mask.cpu(), mask[:-3], wide[::2], [1, 2, 3]):
        with pytest.raises(ValueError):
            ctx.mask_to_indices_into(bad, idx, count)
        with pytest.raises(ValueError):
            ctx.mask_to_indices(bad)
    for op in ("xor", "SET", 0, None):
        with pytest.raises(ValueError):
            ctx.select_mask(col, -INF, INF, op=op, mask=mask)
    for op in ("and", "or"):
        with pytest.raises(ValueError):
            ctx.select_mask(col, -INF, INF, op=op)
    for kw in ({"first": -1}, {"n": -1}):
        with pytest.raises(ValueError):
            ctx.select_mask(col, -INF, INF, mask=mask, **kw)
    for bad in (idx.to(torch.int32), idx.cpu(), torch.full((128,), 7, dtype=torch.int64, device=DEV)[::2]):
        with pytest.raises(ValueError):
            ctx.mask_to_indices_into(mask, bad, count)
    for bad in (count.to(torch.int32), count.cpu(), count[:0], None):
        with pytest.raises(ValueError):
            ctx.mask_to_indices_into(mask, idx, bad)
    for bad in (torch.zeros(8, dtype=torch.uint8, device=DEV), torch.zeros(4096, dtype=torch.int64, device=DEV), torch.zeros(1 << 16, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ctx.mask_to_indices_into(mask, idx, count, scratch=bad)
    for bad in (sums.to(torch.float32), sums.cpu(), sums[:-1], torch.full((2 * nv,), 7.0, dtype=torch.float64, device=DEV)[::2]):
        with pytest.raises(ValueError):
            ctx.decode_sum_masked(col, mask, out=bad)
    for bad in (counts.to(torch.int64), counts.cpu(), counts[:-1]):
        with pytest.raises(ValueError):
            ctx.decode_sum_masked(col, mask, out=sums, counts=bad)
    ctx.synchronize()
    assert bool((mask == 7).all()) and bool((idx == 7).all()) and int(count) == 7 and bool((sums == 7.0).all()) and bool((counts == 7).all()), "a refused call launched"


# ---- 9. the C++ wrapper -------------------------------------------------------------------------------------------------------------------------
def test_cpp_column_masks_match_decompress(tmp_path):
    """include/alp/batch.hpp: alp::gpu::column<double / float>::select_mask, mask_indices and sum_masked of serialized columns == a host scan of
    decompress (tests/cpp/mask_test.cpp)"""
    exe = tmp_path / "mask_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/mask_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0 and "mask_test: 0 failures" in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]
