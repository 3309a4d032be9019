"""GPU: masked projection (include/alpgpu.h, "masked projection": alpgpu_decode_masked_f64 / _f32; Context.decode_masked / decode_masked_into;
alp::gpu::column<PT>::take_masked).  The expected result never comes from the code under test: x = ctx.decode(col) (pinned to the oracle and
the reference by other suites) indexed by the unpacked bitmap, compared as integer bit patterns, and torch.nonzero of the bitmap for the
indices.  Columns are those of test_mask_gpu.py, encoded once per session and shared with it."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import datagen
from alp_amd import capi
from test_mask_gpu import COLUMNS, WITH_SPECIALS, battery, bounds, column, exception_indices, ibits, pack, unpack

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
DENSITIES = (1e-3, 0.1, 0.5, 1.0)
I64_MIN = -2**63  # bit 63 alone


def density_mask(n_vectors, density, seed):
    """a bitmap of n_vectors whose bits are set independently with the given probability (1.0: all of them); made on the host by numpy alone, so
    that what it selects can be worked out without a device"""
    bits = np.random.default_rng(seed).random(n_vectors * 1024) < density
    return torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int64).copy()).to(DEV)


def words(n_vectors, fill=0):
    return torch.full((n_vectors, 16), fill, dtype=torch.int64, device=DEV)


def expected(x, mask):
    sel = unpack(mask)
    return torch.nonzero(sel).reshape(-1), ibits(x)[sel]


def check(ctx, col, x, mask, tag):
    """decode_masked in both forms against the store decode under the bitmap; the bitmap is only read.  Returns the selected indices."""
    before = mask.clone()
    w_idx, w_bits = expected(x, mask)
    idx, vals = ctx.decode_masked(col, mask, indices=True)
    assert vals.dtype == x.dtype and idx.dtype == torch.int64 and idx.numel() == vals.numel() == w_idx.numel(), f"{tag}: {vals.numel()} values, the bitmap has {w_idx.numel()} bits"
    assert torch.equal(idx, w_idx), f"{tag}: indices differ from nonzero of the bitmap"
    assert torch.equal(ibits(vals), w_bits), f"{tag}: values differ in bits from the store decode at the set bits"
    assert torch.equal(ibits(ctx.decode_masked(col, mask)), w_bits), f"{tag}: the form without indices differs"
    assert torch.equal(mask, before), f"{tag}: the bitmap was written"
    return w_idx


def exception_set(col, total):
    exc_idx = exception_indices(col)
    s = torch.zeros(total, dtype=torch.bool, device=DEV)
    s[torch.from_numpy(exc_idx).to(DEV)] = True
    return exc_idx, s


# ---- 1. every column kind against the store decode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_every_column_kind_against_the_store_decode(ctx, name):
    col, x = column(ctx, name)
    total = x.numel()
    exc_idx, exc_set = exception_set(col, total)
    preds = battery(x, name in WITH_SPECIALS)
    if exc_idx.size:
        ev = x[torch.from_numpy(exc_idx).to(DEV)].cpu().numpy()
        cand = ev[np.isfinite(ev)] if np.isfinite(ev).any() else ev[~np.isnan(ev)]
        if cand.size:
            v = float(np.sort(cand)[cand.size // 2])
            preds.append(("exception value", v, v))
    partial = hit_exception = False
    mask = torch.empty(16 * col.n_vectors, dtype=torch.int64, device=DEV)
    for pname, lo, hi in preds:
        ctx.select_mask(col, lo, hi, mask=mask)
        idx = check(ctx, col, x, mask, f"{name}/{pname}")
        partial = partial or 0 < idx.numel() < total
        hit_exception = hit_exception or bool(exc_set[idx].any())
    for i, density in enumerate(DENSITIES):
        idx = check(ctx, col, x, density_mask(col.n_vectors, density, 100 + i), f"{name}/density {density}")
        assert (idx.numel() == total) == (density == 1.0)
        partial = partial or 0 < idx.numel() < total
        hit_exception = hit_exception or bool(exc_set[idx].any())
    assert partial, f"{name}: no bitmap selects some but not all values"
    assert hit_exception or exc_idx.size == 0, f"{name}: the column has exceptions and no bitmap selected one"


# ---- 2. hand-made bitmaps on columns with exceptions in every step ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["every_width_exc", "adversarial", "every_width_exc_f32", "adversarial_f32"])
def test_hand_made_bitmaps(ctx, name):
    col, x = column(ctx, name)
    nv, total = col.n_vectors, x.numel()
    exc_idx, exc_set = exception_set(col, total)
    ev, ep = exc_idx // 1024, exc_idx % 1024
    # from the column's streams: every step of some vector holds an exception, and some vector has exceptions in its first eight steps AND in its
    # last eight (under "words 8..15" the kernel passes over the first batch and must still rank the exceptions behind it correctly)
    steps = np.zeros((nv, 16), dtype=bool)
    steps[ev, ep >> 6] = True
    assert steps.any(axis=0).all(), f"{name}: a step without an exception in every vector"
    both_halves = steps[:, :8].any(axis=1) & steps[:, 8:].any(axis=1)
    assert both_halves.any(), f"{name}: no vector with exceptions in steps 0..7 and in steps 8..15"

    def only(cols, value=-1):
        m = words(nv)
        m[:, cols] = value
        return m.reshape(-1)

    alternating = words(nv)
    alternating[0::2] = -1
    masks = {"bit 0": only(0, 1), "bit 1023": only(15, I64_MIN), "word 0": only(0), "word 15": only(15), "words 8..15": only(slice(8, 16)), "words 0..7": only(slice(0, 8)),
             "on the exceptions": pack(exc_set), "off the exceptions": pack(~exc_set), "alternating vectors": alternating.reshape(-1),
             "nothing": words(nv).reshape(-1), "everything": words(nv, -1).reshape(-1)}
    for mname, mask in masks.items():
        idx = check(ctx, col, x, mask, f"{name}/{mname}")
        if mname == "words 8..15":
            chosen = exc_set[idx].cpu().numpy()
            v_of = (idx >> 10).cpu().numpy()
            assert np.isin(np.flatnonzero(both_halves), v_of[chosen]).all(), f"{name}: the exceptions of steps 8..15 are not all selected"
        if mname == "on the exceptions":
            assert idx.numel() == exc_idx.size > 0
        if mname == "off the exceptions":
            assert idx.numel() == total - exc_idx.size and not bool(exc_set[idx].any())
    assert check(ctx, col, x, masks["nothing"], name).numel() == 0 and check(ctx, col, x, masks["everything"], name).numel() == total


# ---- 3. sizes -----------------------------------------------------------------------------------------------------------------------------------
_sized = {}


def sized_column(ctx, dtype, n_vectors):
    key = (dtype, n_vectors)
    if key not in _sized:
        gen = datagen.mixed_column if dtype == "f64" else datagen.mixed_column_f32
        xd = torch.from_numpy(np.ascontiguousarray(gen(n_vectors, seed=40 + n_vectors % 7))).to(DEV)
        col = ctx.encode(xd)
        dec = ctx.decode(col)
        assert torch.equal(ibits(dec), ibits(xd))
        _sized[key] = (col, dec)
    return _sized[key]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n_vectors", [1, 4, 5, 1024, 1025, 2049])
def test_sizes(ctx, dtype, n_vectors):
    """one wavefront, one workgroup, one more workgroup, one scan block, a second scan level"""
    col, x = sized_column(ctx, dtype, n_vectors)
    assert col.n_vectors == n_vectors
    last_bit = words(n_vectors)
    last_bit[-1, 15] = I64_MIN
    sparse_vectors = density_mask(n_vectors, 0.4, 7).reshape(-1, 16).clone()
    sparse_vectors[torch.arange(n_vectors, device=DEV) % 3 != 1] = 0
    masks = {"random": density_mask(n_vectors, 0.3, 6), "everything": words(n_vectors, -1).reshape(-1), "the last bit": last_bit.reshape(-1),
             "every third vector": sparse_vectors.reshape(-1)}
    for mname, mask in masks.items():
        check(ctx, col, x, mask, f"{dtype}, {n_vectors} vectors, {mname}")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_an_empty_column(ctx, dtype):
    fn = getattr(capi.lib, "alpgpu_decode_masked_" + dtype)
    empty = capi.CColumn()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    mask = torch.full((16,), -1, dtype=torch.int64, device=DEV)
    vals = torch.full((8,), 7.0, dtype=torch.float64 if dtype == "f64" else torch.float32, device=DEV)
    idx = torch.full((8,), 7, dtype=torch.int64, device=DEV)
    for args in ((p(vals), p(idx), 8), (None, None, 0)):
        count = torch.full((1,), 7, dtype=torch.int64, device=DEV)
        assert fn(ctx.h, ctypes.byref(empty), p(mask), *args, p(count), None) == 0
        ctx.synchronize()
        assert int(count) == 0 and bool((vals == 7.0).all()) and bool((idx == 7).all()) and bool((mask == -1).all())


# ---- 4. capacity --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "every_width_exc_f32"])
def test_capacity(ctx, name):
    col, x = column(ctx, name)
    mask = density_mask(col.n_vectors, 0.5, 11)
    sel = unpack(mask)
    w_idx, w_bits = expected(x, mask)
    full = w_idx.numel()
    r = 3 * 1024 + 5 * 64 + 17  # a capacity that ends inside word 5 of vector 3, with selected values on both sides of it in that word
    mid = int(sel[:r].sum())
    assert int(sel[r - 17:r].sum()) > 0 and int(sel[r:r - 17 + 64].sum()) > 0 and 0 < mid < full
    scratch = ctx.select_scratch(col)
    for cap in (0, 1, full - 1, full, full + 7, mid):
        for with_idx in (True, False):
            vals = torch.full((cap + 64,), 7.0, dtype=x.dtype, device=DEV)
            idx = torch.full((cap + 64,), -7, dtype=torch.int64, device=DEV)
            count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
            ctx.decode_masked_into(col, mask, vals[:cap], count, idx[:cap] if with_idx else None, scratch)
            k = min(cap, full)
            tag = f"{name}, capacity {cap}, indices {with_idx}"
            assert int(count) == full, f"{tag}: the count is the full count whatever the capacity"
            assert torch.equal(ibits(vals[:k]), w_bits[:k]) and bool((vals[k:] == 7.0).all()), f"{tag}: values"
            assert (torch.equal(idx[:k], w_idx[:k]) if with_idx else bool((idx[:k] == -7).all())) and bool((idx[k:] == -7).all()), f"{tag}: indices"
    count = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    ctx.decode_masked_into(col, mask, None, count)  # a count: no outputs at all, and a scratch of the call's own
    assert int(count) == full
    idx, vals = ctx.decode_masked(col, mask, indices=True, capacity=full + 9)
    assert torch.equal(idx, w_idx) and torch.equal(ibits(vals), w_bits)
    assert torch.equal(ibits(ctx.decode_masked(col, mask, capacity=mid)), w_bits[:mid])


# ---- 5. agreement within the family -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "rd_latlon", "adversarial", "mixed_f32", "rd_unit_f32", "every_width_exc_f32"])
def test_agreement_within_the_family(ctx, name):
    col, x = column(ctx, name)
    lo, hi = bounds(x, 0.2, 0.7)
    mask = ctx.select_mask(col, lo, hi)
    idx, vals = ctx.decode_masked(col, mask, indices=True)
    s_idx, s_vals = ctx.select_range(col, lo, hi, values=True)
    assert 0 < idx.numel() < x.numel()
    assert torch.equal(idx, s_idx) and torch.equal(ibits(vals), ibits(s_vals)), f"{name}: a SET bitmap's projection differs from select_range(values=True)"
    for tag, m in (("select_mask", mask), ("random", density_mask(col.n_vectors, 0.05, 12))):
        idx, vals = ctx.decode_masked(col, m, indices=True)
        assert torch.equal(idx, ctx.mask_to_indices(m)), f"{name}, {tag}: indices differ from mask_to_indices"
        assert torch.equal(ibits(vals), ibits(ctx.gather(col, idx))), f"{name}, {tag}: values differ in bits from gather at the same indices"


# ---- 6. repeatability -----------------------------------------------------------------------------------------------------------------------------
def test_the_same_call_gives_the_same_bytes_and_leaves_the_decode_plan_alone(ctx):
    for hinted in (True, False):
        col = ctx.encode(torch.from_numpy(datagen.mixed_column(150, seed=91)).to(DEV))
        if hinted:
            ctx.column_totals(col)
        ctx.decode(col)
        ctx.synchronize()  # (what an unhinted decode learns about the column is in by now)
        before = ctx.decode_plan(col)
        mask = density_mask(150, 0.3, 13)
        kept = mask.clone()
        runs = []
        for rep in range(3):
            torch.empty(1 << (20 + rep), dtype=torch.uint8, device=DEV).fill_(rep)  # (a different allocation history each time)
            idx, vals = ctx.decode_masked(col, mask, indices=True)
            runs.append((idx.cpu().numpy().tobytes(), vals.cpu().numpy().tobytes()))
        ctx.synchronize()
        assert runs[0] == runs[1] == runs[2] and len(runs[0][0]) > 0
        assert ctx.decode_plan(col) == before
        assert torch.equal(mask, kept)


# ---- 7. graph capture -----------------------------------------------------------------------------------------------------------------------------
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
nv = 230
a0, a1 = datagen.mixed_column(nv, seed=81), datagen.mixed_column(nv, seed=83)
b0, b1 = datagen.mixed_column_f32(nv, seed=82), datagen.mixed_column_f32(nv, seed=84)
c0, c1 = datagen.rd_column(nv, seed=85), datagen.mixed_column(nv, seed=86)
ad, bd, cd = [[torch.from_numpy(t).cuda() for t in pair] for pair in ((a0, a1), (b0, b1), (c0, c1))]
cola, colb, colc = ctx.encode(ad[0]), ctx.encode(bd[0]), ctx.encode(cd[0])
lo1, hi1, lo2, hi2 = q(a0, 0.2), q(a0, 0.7), q(b0, 0.1), q(b0, 0.8)
cap = nv * 1024
mask = torch.zeros(16 * nv, dtype=torch.int64, device="cuda:0")
vals = torch.zeros(cap, dtype=torch.float64, device="cuda:0")
idx = torch.zeros(cap, dtype=torch.int64, device="cuda:0")
count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
scratch = ctx.select_scratch(colc)
def calls():
    ctx.select_mask(cola, lo1, hi1, mask=mask)
    ctx.select_mask(colb, lo2, hi2, op="and", mask=mask)
    ctx.decode_masked_into(colc, mask, vals, count, idx, scratch)
with torch.cuda.stream(side):
    calls()                                                   # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        calls()
counts = []
for rep in range(3):
    if rep == 1:                                              # other data encoded into the same buffers; rep 2 changes nothing
        ctx.encode(ad[1], cola); ctx.encode(bd[1], colb); ctx.encode(cd[1], colc)
    torch.cuda.synchronize()
    mask.fill_(rep - 1); vals.fill_(7.0); idx.fill_(-1); count.zero_(); scratch.fill_(rep)
    g.replay()
    torch.cuda.synchronize()
    da, db, dc = ctx.decode(cola), ctx.decode(colb), ctx.decode(colc)
    m = (da >= lo1) & (da <= hi1) & (db >= lo2) & (db <= hi2)
    w_idx = torch.nonzero(m).reshape(-1)
    torch.cuda.synchronize()
    k = int(count)
    ok = ok and 0 < k < cap and k == w_idx.numel() and torch.equal(idx[:k], w_idx) and bool((idx[k:] == -1).all())
    ok = ok and torch.equal(vals[:k].view(torch.int64), dc.view(torch.int64)[m]) and bool((vals[k:] == 7.0).all())
    counts.append(k)
    print(rep, k, ok)
ok = ok and counts[0] != counts[1] and counts[1] == counts[2]
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_columns_change():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 8. argument checks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c_argument_checks(ctx, dtype):
    col, x = column(ctx, "mixed" if dtype == "f64" else "mixed_f32")
    nv = col.n_vectors
    fn = getattr(capi.lib, "alpgpu_decode_masked_" + dtype)
    prior = density_mask(nv + 1, 0.5, 14)
    mask = prior.clone()
    vals = torch.full((4096,), 7.0, dtype=x.dtype, device=DEV)
    idx = torch.full((4096,), 7, dtype=torch.int64, device=DEV)
    count = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    scratch = ctx.select_scratch(col)
    scratch.fill_(7)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    c = ctypes.byref(col.c)
    refused = {
        "null column": (ctx.h, None, p(mask), p(vals), p(idx), 4096, p(count), p(scratch)),
        "null bitmap": (ctx.h, c, None, p(vals), p(idx), 4096, p(count), p(scratch)),
        "null bitmap of a count": (ctx.h, c, None, None, None, 0, p(count), p(scratch)),
        "null count": (ctx.h, c, p(mask), p(vals), p(idx), 4096, None, p(scratch)),
        "misaligned bitmap": (ctx.h, c, p(mask, 4), p(vals), p(idx), 4096, p(count), p(scratch)),
        "null scratch": (ctx.h, c, p(mask), p(vals), p(idx), 4096, p(count), None),
        "null scratch of a count": (ctx.h, c, p(mask), None, None, 0, p(count), None),
        "null values with a capacity": (ctx.h, c, p(mask), None, p(idx), 4096, p(count), p(scratch)),
        "null context": (None, c, p(mask), p(vals), p(idx), 4096, p(count), p(scratch)),
    }
    for what, args in refused.items():
        assert fn(*args) == -2, f"{what} must be refused"
        assert capi.lib.alpgpu_last_error() != b""
    ctx.synchronize()
    assert torch.equal(mask, prior) and bool((vals == 7.0).all()) and bool((idx == 7).all()) and int(count) == 7 and bool((scratch == 7).all()), "a refused call wrote"
    # what is allowed: no index output, and no output at all when the capacity is zero
    w_idx, w_bits = expected(x, mask[:16 * nv])
    assert fn(ctx.h, c, p(mask), p(vals), None, 4096, p(count), p(scratch)) == 0
    ctx.synchronize()
    assert int(count) == w_idx.numel() > 4096 and torch.equal(ibits(vals), w_bits[:4096]) and bool((idx == 7).all())
    count.fill_(7)
    assert fn(ctx.h, c, p(mask), None, None, 0, p(count), p(scratch)) == 0
    ctx.synchronize()
    assert int(count) == w_idx.numel() and torch.equal(mask, prior)


def test_python_rejects_arguments_that_do_not_fit(ctx):
    col, x = column(ctx, "mixed")
    nv = col.n_vectors
    mask = torch.full((16 * nv,), 7, dtype=torch.int64, device=DEV)
    vals = torch.full((64,), 7.0, dtype=torch.float64, device=DEV)
    idx = torch.full((64,), 7, dtype=torch.int64, device=DEV)
    count = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    wide = torch.full((32 * nv,), 7, dtype=torch.int64, device=DEV)
    need = capi.lib.alpgpu_select_scratch_bytes(nv)
    for bad in (mask.to(torch.int32), mask.cpu(), mask[:-16], wide, wide[::2], mask.reshape(nv, 16), [1, 2, 3], np.zeros(16 * nv, np.int64)):
        with pytest.raises(ValueError):
            ctx.decode_masked_into(col, bad, vals, count, idx)
        with pytest.raises(ValueError):
            ctx.decode_masked(col, bad)
    for bad in (vals.to(torch.float32), vals.cpu(), torch.full((128,), 7.0, dtype=torch.float64, device=DEV)[::2], [1.0, 2.0]):
        with pytest.raises(ValueError):
            ctx.decode_masked_into(col, mask, bad, count, idx)
    for bad in (idx.to(torch.int32), idx.cpu(), idx[:-1], torch.full((128,), 7, dtype=torch.int64, device=DEV)[::2]):
        with pytest.raises(ValueError):
            ctx.decode_masked_into(col, mask, vals, count, bad)
    for bad in (count.to(torch.int32), count.cpu(), count[:0], None):
        with pytest.raises(ValueError):
            ctx.decode_masked_into(col, mask, vals, bad, idx)
    for bad in (torch.zeros(need - 1, dtype=torch.uint8, device=DEV), torch.zeros(need + 16, dtype=torch.uint8, device=DEV)[1:], torch.zeros(need, dtype=torch.int64, device=DEV),
                torch.zeros(need, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ctx.decode_masked_into(col, mask, vals, count, idx, scratch=bad)
    colf, _ = column(ctx, "mixed_f32")
    with pytest.raises(ValueError):
        ctx.decode_masked_into(colf, mask, vals, count, idx)  # a float column's values are float32
    ctx.synchronize()
    assert bool((mask == 7).all()) and bool((vals == 7.0).all()) and bool((idx == 7).all()) and int(count) == 7, "a refused call launched"


# ---- 9. the C++ wrapper -------------------------------------------------------------------------------------------------------------------------
def test_cpp_take_masked_matches_decompress(tmp_path):
    """include/alp/batch.hpp: alp::gpu::column<double / float>::take_masked under select_mask + mask_and == a host filter of decompress
    (tests/cpp/take_masked_test.cpp)"""
    exe = tmp_path / "take_masked_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/take_masked_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0 and "take_masked_test: 0 failures" in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]
