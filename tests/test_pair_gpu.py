"""GPU: two-column consumers (include/alpgpu.h, "two-column consumers": alpgpu_compare_mask_*, alpgpu_decode_dot_masked_*).  The expected result
never comes from the code under test: a = ctx.decode(col_a), b = ctx.decode(col_b) (pinned to the oracle and the reference by other suites), the
operator in torch, bits packed as tests/test_mask_gpu.py packs them.  Sums compare on their int64 views (and as "both NaN") against the host
replica of the documented order, tests/pair_replica.py: host_sums_masked with the value replaced by a product that numpy rounds on its own."""
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
from pair_replica import host_dots_masked
from test_mask_gpu import COLUMNS, bounds, column, exception_indices, host_column_total, ibits, in_range, pack, random_mask, unpack, vectors_cleared

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
OPS = {"set": 0, "and": 1, "or": 2}
CMPS = {"lt": torch.lt, "le": torch.le, "gt": torch.gt, "ge": torch.ge, "eq": torch.eq, "ne": torch.ne}  # IEEE comparisons, as C's
CMP_CODE = {"lt": 0, "le": 1, "gt": 2, "ge": 3, "eq": 4, "ne": 5}

# every scheme pairing: ALP x ALP, RD x RD, ALP x RD both ways, every packed width with and without exceptions, and the adversarial vectors
# against themselves and against themselves rolled by one vector (NaN, +-inf and -0.0 meet ordinary values and each other)
PAIRS = {
    "alp_alp": ("mixed", "drifting"),
    "rd_rd": ("rd_unit", "rd_latlon"),
    "alp_rd": ("mixed", "rd_unit"),
    "rd_alp": ("rd_unit", "mixed"),
    "widths": ("every_width_exc", "every_width"),
    "adversarial_self": ("adversarial", "adversarial"),
    "adversarial_rolled": ("adversarial", "adversarial+1"),
}
PAIRS.update({k + "_f32": (a + "_f32", b.replace("+1", "") + "_f32" + ("+1" if b.endswith("+1") else "")) for k, (a, b) in list(PAIRS.items())})
_rolled = {}


def pcolumn(ctx, name):
    """(DeviceColumn, its store decode), encoded once per session and left unchanged; "name+1": the column rolled by one vector"""
    if not name.endswith("+1"):
        return column(ctx, name)
    if name not in _rolled:
        xd = torch.from_numpy(np.ascontiguousarray(np.roll(COLUMNS[name[:-2]](), 1024))).to(DEV)
        col = ctx.encode(xd)
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(xd)), f"{name}: decode(encode(x)) != x"
        _rolled[name] = (col, dec)
    return _rolled[name]


def pair(ctx, pname):
    (ca, a), (cb, b) = pcolumn(ctx, PAIRS[pname][0]), pcolumn(ctx, PAIRS[pname][1])
    assert ca.n_vectors == cb.n_vectors and a.dtype == b.dtype
    return ca, a, cb, b


def same_sums(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int64)[~nan], want.view(np.int64)[~nan])


def same_total(got, want):
    return (math.isnan(got) and math.isnan(want)) or np.float64(got).view(np.int64) == np.float64(want).view(np.int64)


# ---- 1. every scheme pairing, six comparisons under SET ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", sorted(PAIRS))
def test_six_comparisons_on_every_scheme_pairing(ctx, pname):
    ca, a, cb, b = pair(ctx, pname)
    total = a.numel()
    exc = np.union1d(exception_indices(ca), exception_indices(cb))
    exc_set = torch.zeros(total, dtype=torch.bool, device=DEV)
    exc_set[torch.from_numpy(exc).to(DEV)] = True
    partial, hit_exception = False, False
    mask = random_mask(ca.n_vectors, 21)  # SET writes every word: what the bitmap held does not matter
    for cmp, fn in CMPS.items():
        q = fn(a, b)
        got = ctx.compare_mask(ca, cb, cmp, mask=mask)
        assert got is mask and torch.equal(mask, pack(q)), f"{pname}/{cmp}: bitmap differs from the comparison of the two store decodes"
        k = int(q.sum())
        partial = partial or 0 < k < total
        hit_exception = hit_exception or bool((q & exc_set).any())
    assert partial, f"{pname}: no comparison selects some but not all values"
    assert hit_exception or exc.size == 0, f"{pname}: the pair has exceptions and no comparison selected one"
    fresh = ctx.compare_mask(ca, cb)  # the allocating form; cmp defaults to "lt"
    assert fresh.dtype == torch.int64 and fresh.numel() == 16 * ca.n_vectors and torch.equal(fresh, pack(a < b))


def test_the_pairs_cover_what_they_are_named_for(ctx):
    """the ALP / ALP_RD pairings really pair those schemes, the rolled adversarial pair really has NaN and +-inf meeting ordinary values (-0.0 meets
    +0.0 in test_one_vector_and_a_ragged_last_workgroup: half_negzero against all_zero)"""
    scheme = lambda col: col.to_host()[1]["scheme"]
    for pname, sa, sb in (("alp_alp", True, True), ("rd_rd", False, False), ("alp_rd", True, False), ("rd_alp", False, True), ("alp_rd_f32", True, False)):
        ca, a, cb, b = pair(ctx, pname)
        both = (scheme(ca) == capi.SCHEME_ALP) == sa
        both &= (scheme(cb) == capi.SCHEME_ALP) == sb
        assert both.any(), pname
    for pname in ("adversarial_rolled", "adversarial_rolled_f32"):
        ca, a, cb, b = pair(ctx, pname)
        assert bool((torch.isnan(a) & ~torch.isnan(b)).any()) and bool((~torch.isnan(a) & torch.isnan(b)).any())
        assert bool((torch.isinf(a) & torch.isfinite(b)).any()) and bool((torch.isfinite(a) & torch.isinf(b)).any())


# ---- 2. a column against itself -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "adversarial", "rd_latlon", "mixed_f32", "adversarial_f32", "every_width_exc_f32"])
def test_a_column_against_itself(ctx, name):
    col, x = column(ctx, name)
    nan = torch.isnan(x)
    assert name.startswith("rd") or bool(nan.any())
    zero = torch.zeros(16 * col.n_vectors, dtype=torch.int64, device=DEV)
    for cmp, want in (("eq", pack(~nan)), ("ne", pack(nan)), ("lt", zero), ("gt", zero), ("le", pack(~nan)), ("ge", pack(~nan))):
        assert torch.equal(ctx.compare_mask(col, col, cmp), want), f"{name} {cmp} itself"


# ---- 3. ops and ranges --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["alp_alp", "alp_rd_f32"])
def test_first_and_n_under_every_op(ctx, pname):
    ca, a, cb, b = pair(ctx, pname)
    total = a.numel()
    prior = random_mask(ca.n_vectors, 22)
    pb = unpack(prior)
    cmp_all = a < b
    ranges = [(3 * 1024 + 17, 500), (3 * 1024 + 17, 1), (63, 1), (63, 2), (64, 64), (65, 63), (1024 + 63, 66), (5 * 1024 - 100, 300), (5 * 1024, 1024), (5 * 1024 - 1, 1026),
              (99 * 1024 + 1000, 101 * 1024), (total - 1, 1), (0, total), (0, total - 500), (0, 0), (777, 0), (total, 0), (1023, 2)]
    for first, n in ranges:
        q = cmp_all & in_range(total, first, n)
        want = {"set": q, "and": pb & q, "or": pb | q}
        for op in OPS:
            mask = prior.clone()
            ctx.compare_mask(ca, cb, "lt", first=first, n=n, op=op, mask=mask)
            assert torch.equal(mask, pack(want[op])), f"{pname} first={first} n={n} op={op}"
        assert n < 2000 or bool(q.any())
    # ranges past the end, and a first + n that overflows, are refused on the host: the bitmap is unchanged
    fn = getattr(capi.lib, "alpgpu_compare_mask_" + ca.dtype)
    mask = prior.clone()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for first, n in ((total - 100, 101), (0, total + 1), (total + 1, 0), (2**64 - 1, 2), (2, 2**64 - 1), (2**63, 2**63)):
        for op in OPS.values():
            assert fn(ctx.h, ctypes.byref(ca.c), ctypes.byref(cb.c), first, n, 0, op, p(mask)) == -2, f"range ({first}, {n}) must be refused"
    ctx.synchronize()
    assert torch.equal(mask, prior), "a refused compare_mask wrote"


# ---- 4. skip rules ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["alp_alp", "rd_rd", "widths", "adversarial_rolled", "rd_alp_f32", "widths_f32"])
def test_and_or_against_prior_bitmaps(ctx, pname):
    ca, a, cb, b = pair(ctx, pname)
    nv, total = ca.n_vectors, a.numel()
    rnd = random_mask(nv, 23)
    priors = {"zeros": torch.zeros_like(rnd), "ones": torch.full_like(rnd, -1), "random": rnd, "vectors zero": vectors_cleared(rnd, 3, 0),
              "vectors ones": vectors_cleared(rnd, 3, -1), "most vectors zero": vectors_cleared(rnd, 7, 0)}
    for cmp in ("le", "ne"):
        full = CMPS[cmp](a, b)
        for prname, prior in priors.items():
            pb = unpack(prior)
            for first, n in ((0, total), (1024 + 100, total - 2048)):
                q = full & in_range(total, first, n)
                for op, want in (("and", pb & q), ("or", pb | q)):
                    mask = prior.clone()
                    ctx.compare_mask(ca, cb, cmp, first=first, n=n, op=op, mask=mask)
                    assert torch.equal(mask, pack(want)), f"{pname} {cmp}: {op} into {prname}, first={first} n={n}"


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_one_vector_and_a_ragged_last_workgroup(ctx, dtype):
    """n_vectors == 1 (three of a workgroup's four wavefronts have nothing to do) and 5 (the second workgroup holds one vector)"""
    f32 = dtype == "f32"
    cases = datagen.adversarial_vectors_f32() if f32 else datagen.adversarial_vectors()
    five_a = datagen.mixed_column_f32(5, seed=31) if f32 else datagen.mixed_column(5, seed=31)
    five_b = datagen.drifting_column_f32(5, seed=32) if f32 else datagen.drifting_column(5, seed=32)
    for xa, xb in ((cases["prefix_nan"], cases["inf_ends"]), (cases["half_negzero"], cases["all_zero"]), (cases["all_exceptions"], cases["plain"]), (five_a, five_b)):
        ca, cb = ctx.encode(torch.from_numpy(xa).to(DEV)), ctx.encode(torch.from_numpy(xb).to(DEV))
        a, b = ctx.decode(ca), ctx.decode(cb)
        nv, total = ca.n_vectors, a.numel()
        assert nv in (1, 5)
        prior = random_mask(nv, 24)
        if nv == 5:
            prior[:16] = 0       # vector 0 all-zero: skipped under AND
            prior[16 * 4:] = -1  # the lone vector of the last workgroup all-ones: skipped under OR
        pb = unpack(prior)
        for cmp, fn in CMPS.items():
            for first, n in ((0, total), (63, 2), (100, total - 200)):
                q = fn(a, b) & in_range(total, first, n)
                for op, want in (("set", q), ("and", pb & q), ("or", pb | q)):
                    mask = prior.clone()
                    ctx.compare_mask(ca, cb, cmp, first=first, n=n, op=op, mask=mask)
                    assert torch.equal(mask, pack(want)), f"{dtype} {nv} vectors, {cmp} first={first} n={n} op={op}"
        bits = pb.cpu().numpy().reshape(nv, 1024)
        sums = ctx.decode_dot_masked(ca, cb, prior)
        assert same_sums(sums.cpu().numpy(), host_dots_masked(a.cpu().numpy().reshape(nv, 1024), b.cpu().numpy().reshape(nv, 1024), bits)), f"{dtype} {nv} vectors: dot"
    empty = capi.CColumn()
    for op in OPS.values():
        assert getattr(capi.lib, "alpgpu_compare_mask_" + dtype)(ctx.h, ctypes.byref(empty), ctypes.byref(empty), 0, 0, 0, op, None) == 0
        assert getattr(capi.lib, "alpgpu_compare_mask_" + dtype)(ctx.h, ctypes.byref(empty), ctypes.byref(empty), 0, 1, 0, op, None) == -2
    assert getattr(capi.lib, "alpgpu_decode_dot_masked_" + dtype)(ctx.h, ctypes.byref(empty), ctypes.byref(empty), None, None, None) == 0


# ---- 5. decode_dot_masked -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", sorted(PAIRS))
def test_decode_dot_masked_against_the_host_replica(ctx, pname):
    ca, a, cb, b = pair(ctx, pname)
    nv = ca.n_vectors
    an, bn = a.cpu().numpy().reshape(nv, 1024), b.cpu().numpy().reshape(nv, 1024)
    rnd = random_mask(nv, 25)
    one = torch.zeros(nv * 1024, dtype=torch.bool, device=DEV)
    one[torch.arange(nv, device=DEV) * 1024 + torch.from_numpy(np.random.default_rng(26).integers(0, 1024, nv)).to(DEV)] = True
    masks = {"all ones": torch.full_like(rnd, -1), "random": rnd, "from select_mask": ctx.select_mask(ca, *bounds(a, 0.2, 0.7)), "all zeros": torch.zeros_like(rnd),
             "one value per vector": pack(one), "vectors zero": vectors_cleared(rnd, 3, 0)}
    for mname, mask in masks.items():
        bits = unpack(mask).cpu().numpy().reshape(nv, 1024)
        want = host_dots_masked(an, bn, bits)
        sums = torch.full((nv,), 7.0, dtype=torch.float64, device=DEV)
        counts = torch.full((nv,), 7, dtype=torch.int32, device=DEV)
        kept = mask.clone()
        assert ctx.decode_dot_masked(ca, cb, mask, out=sums, counts=counts) is sums
        got = sums.cpu().numpy()
        tag = f"{pname}, mask {mname}"
        assert same_sums(got, want), f"{tag}: sums differ from the documented order"
        assert np.array_equal(counts.cpu().numpy(), bits.sum(axis=1).astype(np.int32)), f"{tag}: counts != popcounts"
        assert torch.equal(mask, kept), f"{tag}: the bitmap was written"
        assert same_total(float(ctx.tree_sum(sums)), host_column_total(want)), f"{tag}: column total"
        without = ctx.decode_dot_masked(ca, cb, mask)  # counts=None
        assert same_sums(without.cpu().numpy(), want), f"{tag}: without counts"
        if mname == "all zeros":
            assert bool((ibits(sums) == 0).all()) and bool((counts == 0).all()), f"{tag}: +0.0 with the sign bit clear, and 0"
        if mname == "one value per vector":
            assert bool((counts == 1).all())
            sel = np.nonzero(bits)
            prod = an[sel].astype(np.float64) * bn[sel].astype(np.float64)
            assert same_sums(got, 0.0 + prod), f"{tag}: one selected value: the sum is its product"


@pytest.mark.parametrize("name", ["mixed", "drifting", "rd_latlon_f32"])
def test_a_column_dotted_with_itself_is_the_sum_of_squares(ctx, name):
    col, x = column(ctx, name)
    nv = col.n_vectors
    xn = x.cpu().numpy().reshape(nv, 1024)
    mask = ctx.select_mask(col, *bounds(x, 0.1, 0.9))  # (a range predicate never selects a NaN)
    bits = unpack(mask).cpu().numpy().reshape(nv, 1024)
    sums = ctx.decode_dot_masked(col, col, mask)
    assert same_sums(sums.cpu().numpy(), host_dots_masked(xn, xn, bits))
    chosen = x[unpack(mask)].to(torch.float64)
    want = float((chosen * chosen).sum())
    assert want > 0 and abs(float(ctx.tree_sum(sums)) - want) <= 1e-9 * want  # the sum means what it says


# ---- 6. TPC-H Q6 end to end ---------------------------------------------------------------------------------------------------------------------------
def test_q6_end_to_end(ctx):
    """SUM(price * discount) WHERE lo1 <= shipdate <= hi1 AND lo2 <= discount <= hi2 AND lo3 <= quantity <= hi3: three predicates and the aggregate
    on compressed columns, nothing decoded to HBM"""
    (c_ship, ship), (c_disc, disc), (c_qty, qty), (c_price, price) = column(ctx, "mixed"), column(ctx, "drifting"), column(ctx, "rd_unit"), column(ctx, "rd_latlon")
    nv = c_ship.n_vectors
    assert nv == c_disc.n_vectors == c_qty.n_vectors == c_price.n_vectors == 250
    (lo1, hi1), (lo2, hi2), (lo3, hi3) = bounds(ship, 0.2, 0.8), bounds(disc, 0.3, 0.9), bounds(qty, 0.0, 0.5)
    mask = ctx.select_mask(c_ship, lo1, hi1)
    ctx.select_mask(c_disc, lo2, hi2, op="and", mask=mask)
    ctx.select_mask(c_qty, lo3, hi3, op="and", mask=mask)
    sums = ctx.decode_dot_masked(c_price, c_disc, mask)
    total = float(ctx.tree_sum(sums))
    q = (ship >= lo1) & (ship <= hi1) & (disc >= lo2) & (disc <= hi2) & (qty >= lo3) & (qty <= hi3)
    assert 0 < int(q.sum()) < q.numel() and torch.equal(mask, pack(q))
    want = host_dots_masked(price.cpu().numpy().reshape(nv, 1024), disc.cpu().numpy().reshape(nv, 1024), q.cpu().numpy().reshape(nv, 1024))
    assert same_sums(sums.cpu().numpy(), want) and same_total(total, host_column_total(want))
    plain = price[q] * disc[q]
    assert abs(total - float(plain.sum())) <= 1e-9 * float(plain.abs().sum())


# ---- 7. argument checks -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c_argument_checks(ctx, dtype):
    ca, a, cb, b = pair(ctx, "alp_alp" if dtype == "f64" else "alp_alp_f32")
    short, _ = column(ctx, "every_width" if dtype == "f64" else "every_width_f32")  # another length
    nv = ca.n_vectors
    assert short.n_vectors != nv
    cmpf = getattr(capi.lib, "alpgpu_compare_mask_" + dtype)
    dot = getattr(capi.lib, "alpgpu_decode_dot_masked_" + dtype)
    prior = random_mask(nv + 1, 27)
    mask = prior.clone()
    sums = torch.full((nv,), 7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((nv,), 7, dtype=torch.int32, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    A, B, S = ctypes.byref(ca.c), ctypes.byref(cb.c), ctypes.byref(short.c)
    for cmp in (-1, 6, 17):
        assert cmpf(ctx.h, A, B, 0, 1024, cmp, 0, p(mask)) == -2, "a bad cmp must be refused"
    for op in (-1, 3, 17):
        assert cmpf(ctx.h, A, B, 0, 1024, 0, op, p(mask)) == -2, "a bad op must be refused"
    for op in OPS.values():
        assert cmpf(ctx.h, A, S, 0, 1024, 0, op, p(mask)) == -2 and cmpf(ctx.h, S, B, 0, 1024, 0, op, p(mask)) == -2, "unequal n_vectors must be refused"
        assert cmpf(ctx.h, A, B, 0, 1024, 0, op, p(mask, 4)) == -2, "a misaligned bitmap must be refused"
        assert cmpf(ctx.h, A, B, 0, 1024, 0, op, None) == -2
        assert cmpf(ctx.h, None, B, 0, 1024, 0, op, p(mask)) == -2 and cmpf(ctx.h, A, None, 0, 1024, 0, op, p(mask)) == -2
    assert dot(ctx.h, A, S, p(mask), p(sums), p(counts)) == -2 and dot(ctx.h, S, B, p(mask), p(sums), p(counts)) == -2
    assert dot(ctx.h, A, B, p(mask, 4), p(sums), p(counts)) == -2
    assert dot(ctx.h, A, B, None, p(sums), p(counts)) == -2
    assert dot(ctx.h, A, B, p(mask), None, p(counts)) == -2
    assert dot(ctx.h, None, B, p(mask), p(sums), p(counts)) == -2 and dot(ctx.h, A, None, p(mask), p(sums), p(counts)) == -2
    ctx.synchronize()
    assert torch.equal(mask, prior) and bool((sums == 7.0).all()) and bool((counts == 7).all()), "a refused call wrote"
    # n == 0: SET and AND clear the bitmap (and nothing behind it), OR enqueues nothing
    for op, cleared in ((0, True), (1, True), (2, False)):
        mask = prior.clone()
        assert cmpf(ctx.h, A, B, 0, 0, 0, op, p(mask)) == 0
        ctx.synchronize()
        assert torch.equal(mask[16 * nv:], prior[16 * nv:])
        assert bool((mask[:16 * nv] == 0).all()) if cleared else torch.equal(mask, prior)
    # counts are optional
    assert dot(ctx.h, A, B, p(prior), p(sums), None) == 0
    ctx.synchronize()
    assert bool((counts == 7).all()) and not bool((sums == 7.0).all())


def test_python_rejects_arguments_that_do_not_fit(ctx):
    ca, a, cb, b = pair(ctx, "alp_alp")
    cf, _ = column(ctx, "mixed_f32")
    short, _ = column(ctx, "every_width")
    nv = ca.n_vectors
    mask = torch.full((16 * nv,), 7, dtype=torch.int64, device=DEV)
    sums = torch.full((nv,), 7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((nv,), 7, dtype=torch.int32, device=DEV)
    wide = torch.full((32 * nv,), 7, dtype=torch.int64, device=DEV)
    for other in (cf, short):  # another dtype, another length
        with pytest.raises(ValueError):
            ctx.compare_mask(ca, other, mask=mask)
        with pytest.raises(ValueError):
            ctx.compare_mask(other, ca, mask=mask)
        with pytest.raises(ValueError):
            ctx.decode_dot_masked(ca, other, mask, out=sums)
    for bad in (mask.to(torch.int32), mask.cpu(), mask[:-16], wide, wide[::2], mask.reshape(nv, 16), [1, 2, 3], np.zeros(16 * nv, np.int64)):
        for op in OPS:
            with pytest.raises(ValueError):
                ctx.compare_mask(ca, cb, op=op, mask=bad)
        with pytest.raises(ValueError):
            ctx.decode_dot_masked(ca, cb, bad, out=sums, counts=counts)
    for cmp in ("<", "LT", 0, None):
        with pytest.raises(ValueError):
            ctx.compare_mask(ca, cb, cmp, mask=mask)
    for op in ("xor", "SET", 0, None):
        with pytest.raises(ValueError):
            ctx.compare_mask(ca, cb, op=op, mask=mask)
    for op in ("and", "or"):
        with pytest.raises(ValueError):
            ctx.compare_mask(ca, cb, op=op)
    for kw in ({"first": -1}, {"n": -1}):
        with pytest.raises(ValueError):
            ctx.compare_mask(ca, cb, mask=mask, **kw)
    for bad in (sums.to(torch.float32), sums.cpu(), sums[:-1], torch.full((2 * nv,), 7.0, dtype=torch.float64, device=DEV)[::2]):
        with pytest.raises(ValueError):
            ctx.decode_dot_masked(ca, cb, mask, out=bad)
    for bad in (counts.to(torch.int64), counts.cpu(), counts[:-1]):
        with pytest.raises(ValueError):
            ctx.decode_dot_masked(ca, cb, mask, out=sums, counts=bad)
    ctx.synchronize()
    assert bool((mask == 7).all()) and bool((sums == 7.0).all()) and bool((counts == 7).all()), "a refused call launched"


# ---- 8. determinism, statelessness, capture -----------------------------------------------------------------------------------------------------------
def test_the_same_calls_give_the_same_bytes(ctx):
    ca, a, cb, b = pair(ctx, "alp_rd")
    runs = []
    for rep in range(2):
        torch.empty(1 << (20 + rep), dtype=torch.uint8, device=DEV).fill_(rep)  # (a different allocation history each time)
        mask = ctx.compare_mask(ca, cb, "ge")
        counts = torch.empty(ca.n_vectors, dtype=torch.int32, device=DEV)
        sums = ctx.decode_dot_masked(ca, cb, mask, counts=counts)
        runs.append(tuple(t.cpu().numpy().tobytes() for t in (mask, sums, counts)))
    assert runs[0] == runs[1]
    assert 0 < int(np.frombuffer(runs[0][2], np.int32).sum()) < a.numel()


def test_pair_calls_leave_the_decode_plan_alone(ctx):
    cols = [ctx.encode(torch.from_numpy(datagen.mixed_column(150, seed=s)).to(DEV)) for s in (92, 93)]
    ctx.column_totals(cols[0])  # one hinted, one not
    for col in cols:
        ctx.decode(col)
    ctx.synchronize()  # (what an unhinted decode learns about the column is in by now)
    before = [ctx.decode_plan(col) for col in cols]
    mask = ctx.compare_mask(cols[0], cols[1], "lt")
    ctx.compare_mask(cols[1], cols[0], "eq", first=5, n=9999, op="or", mask=mask)
    ctx.decode_dot_masked(cols[0], cols[1], mask)
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
from pair_replica import host_dots_masked
ctx = capi.Context(0)
side = torch.cuda.Stream()
ok = True
nv = 230
a0, a1 = datagen.mixed_column(nv, seed=81), datagen.mixed_column(nv, seed=83)
b0, b1 = datagen.drifting_column(nv, seed=82), datagen.rd_column(nv, seed=84, kind="latlon")
ad, bd = [torch.from_numpy(t).cuda() for t in (a0, a1)], [torch.from_numpy(t).cuda() for t in (b0, b1)]
cola, colb = ctx.encode(ad[0]), ctx.encode(bd[0])
prior = torch.from_numpy(np.random.default_rng(85).integers(0, 2**64, 16 * nv, dtype=np.uint64).view(np.int64)).cuda()
mask = torch.zeros(16 * nv, dtype=torch.int64, device="cuda:0")
sums = torch.zeros(nv, dtype=torch.float64, device="cuda:0")
counts = torch.zeros(nv, dtype=torch.int32, device="cuda:0")
total = torch.zeros(1, dtype=torch.float64, device="cuda:0")
def calls(mask, sums, counts, total):
    # everything on the one stream: the graph is a chain, no parallel branches
    ctx.compare_mask(cola, colb, "gt", first=1000, n=220 * 1024, op="and", mask=mask)
    ctx.decode_dot_masked(cola, colb, mask, out=sums, counts=counts)
    ctx.tree_sum(sums, out=total)
with torch.cuda.stream(side):
    mask.copy_(prior)
    calls(mask, sums, counts, total)          # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        calls(mask, sums, counts, total)
for rep in range(2):
    if rep == 1:
        ctx.encode(ad[1], cola); ctx.encode(bd[1], colb)    # other data encoded into the same buffers
        prior = ~prior
    torch.cuda.synchronize()
    mask.copy_(prior); sums.fill_(7.0); counts.fill_(7); total.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in (mask, sums, counts, total)]
    e = [prior.clone(), torch.zeros_like(sums), torch.zeros_like(counts), torch.zeros_like(total)]
    calls(*e)
    da, db = ctx.decode(cola), ctx.decode(colb)
    torch.cuda.synchronize()
    m = (da > db); m[:1000] = False; m[1000 + 220 * 1024:] = False
    s = torch.arange(64, dtype=torch.int64, device="cuda:0")
    pb = (((prior.reshape(-1, 1) >> s) & 1) != 0).reshape(-1)
    m = m & pb
    want = host_dots_masked(da.cpu().numpy().reshape(nv, 1024), db.cpu().numpy().reshape(nv, 1024), m.cpu().numpy().reshape(nv, 1024))
    w = got[1].cpu().numpy()
    nan = np.isnan(want)
    ok = ok and 0 < int(m.sum()) < m.numel()
    ok = ok and np.array_equal(np.isnan(w), nan) and np.array_equal(w.view(np.int64)[~nan], want.view(np.int64)[~nan])
    ok = ok and torch.equal(got[2].to(torch.int64), m.reshape(nv, 1024).sum(dim=1))
    ok = ok and torch.equal(got[0], e[0]) and torch.equal(got[2], e[2])
    ok = ok and all(np.array_equal(np.isnan(x.cpu().numpy()), np.isnan(y.cpu().numpy())) and torch.equal(x.view(torch.int64)[~torch.isnan(x)], y.view(torch.int64)[~torch.isnan(y)]) for x, y in ((got[1], e[1]), (got[3], e[3])))
    print(rep, int(m.sum()), ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_inputs_change():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 9. the C++ wrapper -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cpp_column_pair_matches_the_python_route(ctx, tmp_path, dtype):
    """include/alp/batch.hpp: alp::gpu::column<double / float>::compare_mask and dot_masked of two serialized columns give the bytes
    Context.compare_mask / decode_dot_masked + tree_sum give for the same blobs (tests/cpp/pair_test.cpp)"""
    exe = tmp_path / "pair_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/pair_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    ca, a, cb, b = pair(ctx, "alp_rd" if dtype == "f64" else "alp_rd_f32")
    n_values = a.numel() - 333  # an incomplete last vector: its padding must come out clear
    for name, col in (("a.blob", ca), ("b.blob", cb)):
        ctx.to_blob(col, n_values).tofile(str(tmp_path / name))
    prior = ctx.select_mask(ca, *bounds(a, 0.1, 0.8), n=n_values)
    prior.cpu().numpy().tofile(str(tmp_path / "prior.mask"))
    p = subprocess.run([str(exe), dtype, str(tmp_path / "a.blob"), str(tmp_path / "b.blob"), str(tmp_path / "prior.mask"), str(tmp_path / "set.mask"), str(tmp_path / "and.mask")],
                       capture_output=True, text=True, timeout=600)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("dot ")]
    assert p.returncode == 0 and len(line) == 1, p.stdout[-3000:] + p.stderr[-2000:]
    want_set = ctx.compare_mask(ca, cb, "le", n=n_values)
    want_and = ctx.compare_mask(ca, cb, "gt", n=n_values, op="and", mask=prior.clone())
    assert 0 < int(unpack(want_and).sum()) < n_values
    assert np.array_equal(np.fromfile(str(tmp_path / "set.mask"), np.int64), want_set.cpu().numpy()), "column::compare_mask (fresh) != Context.compare_mask"
    assert np.array_equal(np.fromfile(str(tmp_path / "and.mask"), np.int64), want_and.cpu().numpy()), "column::compare_mask (mask_and) != Context.compare_mask"
    counts = torch.empty(ca.n_vectors, dtype=torch.int32, device=DEV)
    total = ctx.tree_sum(ctx.decode_dot_masked(ca, cb, want_and, counts=counts))
    _, bits_hex, count = line[0].split()
    assert int(bits_hex, 16) == int(total.view(torch.int64).item()) & (2**64 - 1) and int(count) == int(counts.sum()), "column::dot_masked != decode_dot_masked + tree_sum"
