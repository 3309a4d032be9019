"""GPU: grouped aggregation (include/alpgpu.h, "grouped aggregation": alpgpu_decode_group_sum_*, alpgpu_group_totals).  The expected result never
comes from the code under test: val = ctx.decode(col_val), key = ctx.decode(col_key) (pinned to the oracle and the reference by other suites), the
predicate evaluated on them, the sums by the host replica of the documented order, tests/group_replica.py.  Everything compares on int64 views,
NaN being equal to NaN; there is no tolerance anywhere."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import datagen
from alp_amd import capi
from group_replica import host_group_sums, host_group_totals
from test_mask_gpu import bounds, column, exception_indices, random_mask, unpack, vectors_cleared
from test_pair_gpu import PAIRS, pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF, NAN = float("inf"), float("nan")


def same(got, want):
    """float64 arrays: NaN where NaN is wanted, the same bits elsewhere"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int64)[~nan], want.view(np.int64)[~nan])


def host(t, nv):
    return t.cpu().numpy().reshape(nv, 1024)


def quantile_groups(key):
    """13 groups from the key's own finite decoded values (bounds are values that occur, so they are exact in the key's type): everything; three
    touching bands that share their boundary values; two overlapping bands; a point; lo > hi; a NaN lo; the points 0.0 and -0.0; the points +inf and
    -inf.  More than 8: the 16-tier."""
    xs = key.cpu().numpy()
    s = np.sort(xs[np.isfinite(xs)])
    q = lambda f: float(s[min(s.size - 1, int(f * s.size))])
    above, below = (q(0.7), q(0.3)) if q(0.7) > q(0.3) else (INF, -INF)  # (a column of mostly one value: still lo > hi)
    g = [(-INF, INF), (q(0.1), q(0.3)), (q(0.3), q(0.5)), (q(0.5), q(0.7)), (q(0.2), q(0.6)), (q(0.4), q(0.8)), (q(0.41), q(0.41)), (above, below), (NAN, q(0.7)),
         (0.0, 0.0), (-0.0, -0.0), (INF, INF), (-INF, -INF)]
    return [a for a, _ in g], [b for _, b in g]


def run(ctx, cv, ck, mask, lo, hi):
    nv = cv.n_vectors
    sums = torch.full((len(lo), nv), 7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((len(lo), nv), 7, dtype=torch.int32, device=DEV)
    assert ctx.decode_group_sum(cv, ck, mask, lo, hi, out=sums, counts=counts) is sums
    return sums.cpu().numpy(), counts.cpu().numpy()


# ---- 1. every scheme pairing --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", sorted(PAIRS))
def test_every_scheme_pairing_against_the_host_replica(ctx, pname):
    cv, val, ck, key = pair(ctx, pname)
    nv = cv.n_vectors
    vn, kn = host(val, nv), host(key, nv)
    lo, hi = quantile_groups(key)
    assert 8 < len(lo) <= capi.GROUP_MAX
    rnd = random_mask(nv, 41)
    exc_v, exc_k = exception_indices(cv), exception_indices(ck)
    for mname, mask in (("full", torch.full_like(rnd, -1)), ("random", rnd), ("vectors zero", vectors_cleared(rnd, 3, 0))):
        bits = host(unpack(mask), nv)
        want_s, want_c = host_group_sums(vn, kn, bits, lo, hi)
        kept = mask.clone()
        got_s, got_c = run(ctx, cv, ck, mask, lo, hi)
        tag = f"{pname}, mask {mname}"
        assert same(got_s, want_s), f"{tag}: sums differ from the documented order"
        assert np.array_equal(got_c, want_c.astype(np.int32)), f"{tag}: counts"
        assert torch.equal(mask, kept), f"{tag}: the bitmap was written"
        without = ctx.decode_group_sum(cv, ck, mask, lo, hi)  # counts=None, out allocated
        assert without.shape == (len(lo), nv) and same(without.cpu().numpy(), want_s), f"{tag}: without counts"
        assert int(want_c[7].sum()) == 0 and int(want_c[8].sum()) == 0, "lo > hi and a NaN bound select nothing"
        if mname == "full":
            assert 0 < int(want_c[2].sum()) < bits.sum(), f"{tag}: a band selects some but not all"
            # exceptions of both columns are among what the open group selects
            sel = (bits & (kn >= -INF) & (kn <= INF)).reshape(-1)
            for exc in (exc_v, exc_k):
                assert exc.size == 0 or sel[exc].any(), f"{tag}: the pair has exceptions and none is selected"


# ---- 2. tier edges ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_groups", [1, 3, 4, 5, 8, 9, 16])
def test_tier_edges_write_their_rows_and_nothing_behind(ctx, n_groups):
    cv, val, ck, key = pair(ctx, "alp_rd")
    nv = cv.n_vectors
    xs = np.sort(key.cpu().numpy())
    cuts = [float(xs[int(f * (xs.size - 1))]) for f in np.linspace(0.0, 1.0, n_groups + 1)]
    lo, hi = cuts[:-1], cuts[1:]  # touching bands
    mask = random_mask(nv, 42)
    bits = host(unpack(mask), nv)
    want_s, want_c = host_group_sums(host(val, nv), host(key, nv), bits, lo, hi)
    rows = n_groups + 2
    sums = torch.full((rows, nv), 7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((rows, nv), 7, dtype=torch.int32, device=DEV)
    ctx.decode_group_sum(cv, ck, mask, lo, hi, out=sums[:n_groups], counts=counts[:n_groups])
    assert same(sums[:n_groups].cpu().numpy(), want_s) and np.array_equal(counts[:n_groups].cpu().numpy(), want_c.astype(np.int32))
    assert bool((sums[n_groups:] == 7.0).all()) and bool((counts[n_groups:] == 7).all()), "written behind the last group's row"
    assert int(want_c.sum()) >= int(bits.sum())  # the bands cover every value; the shared boundaries count twice
    counts.fill_(7)
    sums.fill_(7.0)
    ctx.decode_group_sum(cv, ck, mask, lo, hi, out=sums[:n_groups])
    assert same(sums[:n_groups].cpu().numpy(), want_s) and bool((counts == 7).all()) and bool((sums[n_groups:] == 7.0).all()), "counts=None writes no counts"


# ---- 3. flag keys -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_flag_keys_with_point_groups_and_their_totals(ctx, dtype):
    f32 = dtype == "f32"
    nv = 230
    rng = np.random.default_rng(43)
    flags = rng.integers(0, 6, nv * 1024).astype(np.float32 if f32 else np.float64)
    flags[rng.random(flags.size) < 0.002] = NAN
    flags[rng.random(flags.size) < 0.002] = -0.0
    vals = datagen.mixed_column_f32(nv, seed=44) if f32 else datagen.mixed_column(nv, seed=44)
    ck, cv = ctx.encode(torch.from_numpy(flags).to(DEV)), ctx.encode(torch.from_numpy(vals).to(DEV))
    key, val = ctx.decode(ck), ctx.decode(cv)
    kn, vn = host(key, nv), host(val, nv)
    assert np.isnan(kn).any() and (np.signbit(kn) & (kn == 0)).any()
    lo = hi = [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    mask = random_mask(nv, 45)
    bits = host(unpack(mask), nv)
    want_s, want_c = host_group_sums(vn, kn, bits, lo, hi)
    got_s, got_c = run(ctx, cv, ck, mask, lo, hi)
    assert same(got_s, want_s) and np.array_equal(got_c, want_c.astype(np.int32))
    sums, counts = torch.from_numpy(got_s).to(DEV), torch.from_numpy(got_c).to(DEV)
    totals, tcounts = ctx.group_totals(sums, counts)
    want_t, want_tc = host_group_totals(want_s, want_c)
    assert totals.dtype == torch.float64 and tcounts.dtype == torch.int64
    assert same(totals.cpu().numpy(), want_t) and np.array_equal(tcounts.cpu().numpy(), want_tc)
    assert int(tcounts.sum()) == int((bits & ~np.isnan(kn)).sum()), "every set bit with a key that is a number falls in exactly one flag"
    only, none = ctx.group_totals(sums)
    assert none is None and same(only.cpu().numpy(), want_t)


# ---- 4. the defining identity on the device -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pname", ["alp_rd", "adversarial_rolled", "widths", "rd_alp_f32", "adversarial_rolled_f32"])
def test_every_row_is_select_mask_and_then_decode_sum_masked(ctx, pname):
    cv, val, ck, key = pair(ctx, pname)
    nv = cv.n_vectors
    lo, hi = quantile_groups(key)
    for mask in (random_mask(nv, 46), vectors_cleared(random_mask(nv, 47), 3, 0)):
        got_s, got_c = run(ctx, cv, ck, mask, lo, hi)
        for g in range(len(lo)):
            m = mask.clone()
            ctx.select_mask(ck, lo[g], hi[g], op="and", mask=m)
            counts = torch.empty(nv, dtype=torch.int32, device=DEV)
            sums = ctx.decode_sum_masked(cv, m, counts=counts)
            assert same(got_s[g], sums.cpu().numpy()), f"{pname} group {g}: the row is not decode_sum_masked under the ANDed bitmap"
            assert np.array_equal(got_c[g], counts.cpu().numpy()), f"{pname} group {g}: counts"


# ---- 5. a column as its own key -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "adversarial", "rd_latlon", "mixed_f32", "every_width_exc_f32"])
def test_a_column_as_its_own_key(ctx, name):
    col, x = column(ctx, name)
    nv = col.n_vectors
    xn = host(x, nv)
    lo, hi = quantile_groups(x)
    mask = random_mask(nv, 48)
    bits = host(unpack(mask), nv)
    want_s, want_c = host_group_sums(xn, xn, bits, lo, hi)
    got_s, got_c = run(ctx, col, col, mask, lo, hi)
    assert same(got_s, want_s) and np.array_equal(got_c, want_c.astype(np.int32))
    assert not np.isnan(want_s[1:]).any(), "a NaN is in no band of its own column"


# ---- 6. shapes ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_one_vector_a_ragged_last_workgroup_and_an_empty_column(ctx, dtype):
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
        want_s, want_c = host_group_sums(host(val, nv), host(key, nv), bits, lo, hi)
        got_s, got_c = run(ctx, cv, ck, mask, lo, hi)
        assert same(got_s, want_s) and np.array_equal(got_c, want_c.astype(np.int32)), f"{dtype}, {nv} vectors"
        if nv == 5:
            assert (got_s[:, 1].view(np.int64) == 0).all() and (got_c[:, 1] == 0).all(), "a vector without a set bit: +0.0 and 0 in every group"
    empty = capi.CColumn()
    fn = getattr(capi.lib, "alpgpu_decode_group_sum_" + dtype)
    ft = ctypes.c_float if f32 else ctypes.c_double
    b = (ft * 2)(0.0, 1.0)
    assert fn(ctx.h, ctypes.byref(empty), ctypes.byref(empty), None, b, b, 2, None, None) == 0
    assert fn(ctx.h, ctypes.byref(empty), ctypes.byref(empty), None, b, b, 0, None, None) == -2
    totals, tcounts = ctx.group_totals(torch.empty((3, 0), dtype=torch.float64, device=DEV), torch.empty((3, 0), dtype=torch.int32, device=DEV))
    assert totals.view(torch.int64).tolist() == [0, 0, 0] and tcounts.tolist() == [0, 0, 0], "no vector: +0.0 and 0"


# ---- 7. group_totals alone ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_groups", [1, 16])
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_group_totals_is_the_tree_sum_of_every_row(ctx, n, n_groups):
    rng = np.random.default_rng(50 + n)
    rows = rng.normal(0, 1e6, (n_groups, n)) * rng.choice([1e-12, 1.0, 1e12], (n_groups, n))
    raw = rng.integers(2**31, 2**32, (n_groups, n), dtype=np.uint64).astype(np.uint32)  # every count near 2^32: any row of two or more overflows 32 bits
    sums, counts = torch.from_numpy(rows).to(DEV), torch.from_numpy(raw.view(np.int32)).to(DEV)
    scratch = ctx.group_totals_scratch(n, n_groups)
    assert scratch.numel() == 32 * n_groups * ((n + 1023) // 1024)
    scratch.fill_(0x5A)
    totals, tcounts = ctx.group_totals(sums, counts, scratch=scratch)
    want_t, want_c = host_group_totals(rows, raw)
    assert same(totals.cpu().numpy(), want_t), "totals differ from the documented tree"
    assert np.array_equal(tcounts.cpu().numpy(), want_c) and (n == 1 or int(want_c.min()) >= 2**32)
    for g in range(n_groups):
        assert int(ctx.tree_sum(sums[g]).view(torch.int64).item()) == int(totals[g].view(torch.int64).item()), f"row {g}: not alpgpu_tree_sum_f64 of the row"
    assert torch.equal(sums, torch.from_numpy(rows).to(DEV)) and torch.equal(counts, torch.from_numpy(raw.view(np.int32)).to(DEV)), "the inputs were written"
    # preallocated outputs: nothing else is needed
    out, cout = torch.full((n_groups,), 7.0, dtype=torch.float64, device=DEV), torch.full((n_groups,), 7, dtype=torch.int64, device=DEV)
    a, b = ctx.group_totals(sums, counts, scratch=scratch, out=out, counts_out=cout)
    assert a is out and b is cout and torch.equal(out.view(torch.int64), totals.view(torch.int64)) and torch.equal(cout, tcounts)


# ---- 8. C argument checks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c_argument_checks(ctx, dtype):
    cv, val, ck, key = pair(ctx, "alp_alp" if dtype == "f64" else "alp_alp_f32")
    short, _ = column(ctx, "every_width" if dtype == "f64" else "every_width_f32")  # another length
    nv = cv.n_vectors
    assert short.n_vectors != nv
    fn = getattr(capi.lib, "alpgpu_decode_group_sum_" + dtype)
    tot = capi.lib.alpgpu_group_totals
    ft = ctypes.c_float if dtype == "f32" else ctypes.c_double
    lo, hi = (ft * 17)(*([0.0] * 17)), (ft * 17)(*([1e30] * 17))
    mask = torch.full((16 * nv + 16,), -1, dtype=torch.int64, device=DEV)
    sums = torch.full((17, nv), 7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((17, nv), 7, dtype=torch.int32, device=DEV)
    totals = torch.full((17,), 7.0, dtype=torch.float64, device=DEV)
    tcounts = torch.full((17,), 7, dtype=torch.int64, device=DEV)
    scratch = ctx.group_totals_scratch(2049, 16)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    V, K, S = ctypes.byref(cv.c), ctypes.byref(ck.c), ctypes.byref(short.c)
    M, SU, CO = p(mask), p(sums), p(counts)
    bare = capi.CColumn()
    bare.n_vectors = nv  # a column without descriptors
    huge = capi.CColumn()
    huge.n_vectors = 2**60
    refused = [
        fn(None, V, K, M, lo, hi, 2, SU, CO), fn(ctx.h, None, K, M, lo, hi, 2, SU, CO), fn(ctx.h, V, None, M, lo, hi, 2, SU, CO),
        fn(ctx.h, V, K, M, None, hi, 2, SU, CO), fn(ctx.h, V, K, M, lo, None, 2, SU, CO),
        fn(ctx.h, V, K, M, lo, hi, 0, SU, CO), fn(ctx.h, V, K, M, lo, hi, 17, SU, CO), fn(ctx.h, V, K, M, lo, hi, 2**32 - 1, SU, CO),
        fn(ctx.h, V, S, M, lo, hi, 2, SU, CO), fn(ctx.h, S, K, M, lo, hi, 2, SU, CO),
        fn(ctx.h, ctypes.byref(huge), ctypes.byref(huge), M, lo, hi, 2, SU, CO),
        fn(ctx.h, V, K, None, lo, hi, 2, SU, CO), fn(ctx.h, V, K, M, lo, hi, 2, None, CO), fn(ctx.h, V, K, p(mask, 4), lo, hi, 2, SU, CO),
        fn(ctx.h, ctypes.byref(bare), K, M, lo, hi, 2, SU, CO), fn(ctx.h, V, ctypes.byref(bare), M, lo, hi, 2, SU, CO),
        tot(None, SU, CO, nv, 2, p(totals), p(tcounts), p(scratch)), tot(ctx.h, None, CO, nv, 2, p(totals), p(tcounts), p(scratch)),
        tot(ctx.h, SU, CO, nv, 2, None, p(tcounts), p(scratch)), tot(ctx.h, SU, CO, nv, 0, p(totals), p(tcounts), p(scratch)),
        tot(ctx.h, SU, CO, nv, 17, p(totals), p(tcounts), p(scratch)), tot(ctx.h, SU, None, nv, 2, p(totals), p(tcounts), p(scratch)),
        tot(ctx.h, SU, CO, nv, 2, p(totals), None, p(scratch)), tot(ctx.h, SU, CO, 2049, 2, p(totals), p(tcounts), None),
        tot(ctx.h, SU, CO, 2049, 2, p(totals), p(tcounts), p(scratch, 8)), tot(ctx.h, SU, CO, 2**60, 2, p(totals), p(tcounts), p(scratch)),
    ]
    assert refused == [-2] * len(refused), refused
    ctx.synchronize()
    assert bool((mask == -1).all()) and bool((sums == 7.0).all()) and bool((counts == 7).all()) and bool((totals == 7.0).all()) and bool((tcounts == 7).all()), "a refused call wrote"
    # counts are optional, and 16 groups are accepted
    assert fn(ctx.h, V, K, M, lo, hi, 16, SU, None) == 0
    ctx.synchronize()
    assert bool((counts == 7).all()) and not bool((sums[:16] == 7.0).any()) and bool((sums[16] == 7.0).all())


# ---- 9. Python checks ---------------------------------------------------------------------------------------------------------------------------------
def test_python_rejects_arguments_that_do_not_fit(ctx, monkeypatch):
    cv, val, ck, key = pair(ctx, "alp_alp")
    cf, _ = column(ctx, "mixed_f32")
    short, _ = column(ctx, "every_width")
    nv = cv.n_vectors
    mask = torch.full((16 * nv,), 7, dtype=torch.int64, device=DEV)
    sums = torch.full((2, nv), 7.0, dtype=torch.float64, device=DEV)
    counts = torch.full((2, nv), 7, dtype=torch.int32, device=DEV)
    lo, hi = [0.0, 1.0], [1.0, 2.0]

    def unreachable(*a, **k):
        raise AssertionError("the library was called")
    for t in ("f64", "f32"):
        monkeypatch.setattr(capi.lib, "alpgpu_decode_group_sum_" + t, unreachable)
    monkeypatch.setattr(capi.lib, "alpgpu_group_totals", unreachable)
    for other in (cf, short):  # another dtype, another length
        with pytest.raises(ValueError):
            ctx.decode_group_sum(cv, other, mask, lo, hi)
        with pytest.raises(ValueError):
            ctx.decode_group_sum(other, cv, mask, lo, hi)
    wide = torch.full((32 * nv,), 7, dtype=torch.int64, device=DEV)
    for bad in (mask.to(torch.int32), mask.cpu(), mask[:-16], wide, wide[::2], mask.reshape(nv, 16), [1, 2, 3], np.zeros(16 * nv, np.int64)):
        with pytest.raises(ValueError):
            ctx.decode_group_sum(cv, ck, bad, lo, hi, out=sums, counts=counts)
    for blo, bhi in (([0.0], [1.0, 2.0]), ([], []), ([0.0] * 17, [1.0] * 17), (0.0, 1.0), (None, None)):
        with pytest.raises(ValueError):
            ctx.decode_group_sum(cv, ck, mask, blo, bhi)
    for bad in (sums.to(torch.float32), sums.cpu(), sums[:1], sums.reshape(-1), torch.full((3, nv), 7.0, dtype=torch.float64, device=DEV), sums.t(), sums[:, ::2]):
        with pytest.raises(ValueError):
            ctx.decode_group_sum(cv, ck, mask, lo, hi, out=bad)
    for bad in (counts.to(torch.int64), counts.cpu(), counts[:1], counts.reshape(-1)):
        with pytest.raises(ValueError):
            ctx.decode_group_sum(cv, ck, mask, lo, hi, out=sums, counts=bad)
    scratch = ctx.group_totals_scratch(nv, 2)
    for bad in (sums.to(torch.float32), sums.cpu(), sums.reshape(-1), torch.zeros((17, 4), dtype=torch.float64, device=DEV), torch.zeros((0, 4), dtype=torch.float64, device=DEV), sums.t()):
        with pytest.raises(ValueError):
            ctx.group_totals(bad)
    for bad in (counts.to(torch.int64), counts.cpu(), counts[:1], counts.reshape(-1)):
        with pytest.raises(ValueError):
            ctx.group_totals(sums, bad)
    for kw in ({"scratch": scratch[:-1]}, {"scratch": scratch.cpu()}, {"scratch": torch.zeros(scratch.numel() + 16, dtype=torch.uint8, device=DEV)[8:]},
               {"out": torch.zeros(3, dtype=torch.float64, device=DEV)}, {"out": torch.zeros(2, dtype=torch.float32, device=DEV)},
               {"counts_out": torch.zeros(3, dtype=torch.int64, device=DEV)}, {"counts_out": torch.zeros(2, dtype=torch.int32, device=DEV)}):
        with pytest.raises(ValueError):
            ctx.group_totals(sums, counts, **kw)
    with pytest.raises(ValueError):
        ctx.group_totals(sums, counts_out=torch.zeros(2, dtype=torch.int64, device=DEV))
    ctx.synchronize()
    assert bool((mask == 7).all()) and bool((sums == 7.0).all()) and bool((counts == 7).all())


# ---- 10. determinism, statelessness, capture ----------------------------------------------------------------------------------------------------------
def test_the_same_calls_give_the_same_bytes(ctx):
    cv, val, ck, key = pair(ctx, "alp_rd")
    lo, hi = quantile_groups(key)
    mask = random_mask(cv.n_vectors, 51)
    runs = []
    for rep in range(2):
        torch.empty(1 << (20 + rep), dtype=torch.uint8, device=DEV).fill_(rep)  # (a different allocation history each time)
        counts = torch.empty((len(lo), cv.n_vectors), dtype=torch.int32, device=DEV)
        sums = ctx.decode_group_sum(cv, ck, mask, lo, hi, counts=counts)
        totals, tcounts = ctx.group_totals(sums, counts)
        runs.append(tuple(t.cpu().numpy().tobytes() for t in (sums, counts, totals, tcounts)))
    assert runs[0] == runs[1]
    assert 0 < int(np.frombuffer(runs[0][3], np.int64)[1]) < val.numel()


def test_group_calls_leave_the_decode_plan_alone(ctx):
    cols = [ctx.encode(torch.from_numpy(datagen.mixed_column(150, seed=s)).to(DEV)) for s in (94, 95)]
    ctx.column_totals(cols[0])  # one hinted, one not
    for col in cols:
        ctx.decode(col)
    ctx.synchronize()  # (what an unhinted decode learns about the column is in by now)
    before = [ctx.decode_plan(col) for col in cols]
    mask = random_mask(150, 52)
    sums = ctx.decode_group_sum(cols[0], cols[1], mask, [0.0, 10.0], [10.0, 1e9])
    ctx.decode_group_sum(cols[1], cols[1], mask, [0.0], [1e9])
    ctx.group_totals(sums)
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
from group_replica import host_group_sums, host_group_totals
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
where = (q(0.05), q(0.95))
lo, hi = [q(0.0), q(0.2), q(0.5), q(0.5), q(0.9)], [q(0.2), q(0.5), q(1.0), q(0.5), q(0.1)]
lo0, hi0 = list(lo), list(hi)
G = len(lo)
mask = torch.zeros(16 * nv, dtype=torch.int64, device="cuda:0")
sums = torch.zeros((G, nv), dtype=torch.float64, device="cuda:0")
counts = torch.zeros((G, nv), dtype=torch.int32, device="cuda:0")
totals = torch.zeros(G, dtype=torch.float64, device="cuda:0")
tcounts = torch.zeros(G, dtype=torch.int64, device="cuda:0")
scratch = ctx.group_totals_scratch(nv, G)
def calls():
    # everything on the one stream: the graph is a chain, no parallel branches
    ctx.select_mask(colk, where[0], where[1], first=1000, n=220 * 1024, mask=mask)
    ctx.decode_group_sum(colv, colk, mask, lo, hi, out=sums, counts=counts)
    ctx.group_totals(sums, counts, scratch=scratch, out=totals, counts_out=tcounts)
with torch.cuda.stream(side):
    calls()          # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        calls()
for i in range(G):   # the graph keeps the bounds it was captured with
    lo[i], hi[i] = -1e300, 1e300
def same(a, b):
    nan = np.isnan(b)
    return np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.int64)[~nan], b.view(np.int64)[~nan])
for rep in range(2):
    if rep == 1:
        ctx.encode(vd[1], colv); ctx.encode(kd[1], colk)    # other data encoded into the same buffers
    torch.cuda.synchronize()
    mask.fill_(7); sums.fill_(7.0); counts.fill_(7); totals.fill_(7.0); tcounts.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    dv, dk = ctx.decode(colv), ctx.decode(colk)
    torch.cuda.synchronize()
    kn, vn = dk.cpu().numpy(), dv.cpu().numpy()
    r = np.arange(kn.size)
    bits = (kn >= where[0]) & (kn <= where[1]) & (r >= 1000) & (r < 1000 + 220 * 1024)
    want_s, want_c = host_group_sums(vn.reshape(nv, 1024), kn.reshape(nv, 1024), bits.reshape(nv, 1024), lo0, hi0)
    want_t, want_tc = host_group_totals(want_s, want_c)
    ok = ok and 0 < int(want_tc[1]) < bits.sum() and int(want_tc[4]) == 0
    ok = ok and same(sums.cpu().numpy(), want_s) and np.array_equal(counts.cpu().numpy(), want_c.astype(np.int32))
    ok = ok and same(totals.cpu().numpy(), want_t) and np.array_equal(tcounts.cpu().numpy(), want_tc)
    print(rep, want_tc.tolist(), ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_columns_change():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 11. the C++ wrapper ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cpp_column_group_sum_matches_the_python_route(ctx, tmp_path, dtype):
    """include/alp/batch.hpp: alp::gpu::column<double / float>::group_sum_masked and group_totals of two serialized columns give the bytes
    Context.decode_group_sum / group_totals give for the same blobs (tests/cpp/group_test.cpp)"""
    exe = tmp_path / "group_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/group_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    cv, val, ck, key = pair(ctx, "alp_rd" if dtype == "f64" else "alp_rd_f32")
    n_values = val.numel()
    for name, col in (("val.blob", cv), ("key.blob", ck)):
        ctx.to_blob(col, n_values).tofile(str(tmp_path / name))
    mask = ctx.select_mask(cv, *bounds(val, 0.1, 0.8))
    mask.cpu().numpy().tofile(str(tmp_path / "in.mask"))
    lo, hi = quantile_groups(key)
    np.asarray(lo + hi, dtype=np.float32 if dtype == "f32" else np.float64).tofile(str(tmp_path / "bounds.bin"))
    p = subprocess.run([str(exe), dtype] + [str(tmp_path / f) for f in ("val.blob", "key.blob", "in.mask", "bounds.bin", "sums.bin", "counts.bin")],
                       capture_output=True, text=True, timeout=600)
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("total ")]
    assert p.returncode == 0 and len(lines) == len(lo), p.stdout[-3000:] + p.stderr[-2000:]
    counts = torch.empty((len(lo), cv.n_vectors), dtype=torch.int32, device=DEV)
    sums = ctx.decode_group_sum(cv, ck, mask, lo, hi, counts=counts)
    totals, tcounts = ctx.group_totals(sums, counts)
    assert same(np.fromfile(str(tmp_path / "sums.bin"), np.float64).reshape(len(lo), -1), sums.cpu().numpy()), "column::group_sum_masked != Context.decode_group_sum"
    assert np.array_equal(np.fromfile(str(tmp_path / "counts.bin"), np.int32).reshape(len(lo), -1), counts.cpu().numpy())
    assert 0 < int(tcounts[2]) < int(tcounts[0])
    for g, (_, gi, bits_hex, count) in enumerate(lines):
        got = np.array([int(bits_hex, 16)], dtype=np.uint64).view(np.float64)
        assert int(gi) == g and same(got, totals[g:g + 1].cpu().numpy()) and int(count) == int(tcounts[g]), f"column::group_totals, group {g}"
