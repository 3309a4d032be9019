"""GPU: random access (include/alpgpu.h, "random access": alpgpu_gather_*, alpgpu_decode_slice_*).  Every value read where it lies must be, bit for
bit, what the store decode writes at that index (ctx.decode, pinned against the oracle and the reference elsewhere) and, for columns encoded from x,
x itself: the comparisons are on int64 / int32 views, so that NaN payloads and -0.0 count.  Column kinds, index sets, other column sources, bounds,
sizes, 64-bit indices, slices, stream capture and the context's planning state, the Python argument check and a speed sanity check."""
import ctypes
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
NAN_BITS = {"f64": 0x7FF8000000000000, "f32": 0x7FC00000}


def ibits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def encoded(ctx, x):
    """(DeviceColumn, x on the device) for a host column of whole vectors"""
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return ctx.encode(xd), xd


def exception_neighbourhood(col):
    """value indices of every exception position of every vector and of its two neighbours (inside the column)"""
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
        for d in (-1, 0, 1):
            out.append(v * 1024 + pos + d)
    n = col.n_vectors * 1024
    a = np.concatenate(out) if out else np.zeros(0, np.int64)
    return a[(a >= 0) & (a < n)]


def index_sets(col, seed=0):
    n = col.n_vectors * 1024
    rng = np.random.default_rng(seed)
    ends = np.arange(col.n_vectors, dtype=np.int64) * 1024
    return {
        "in order": np.arange(n, dtype=np.int64),
        "permutation": rng.permutation(n).astype(np.int64),
        "duplicates": rng.integers(0, n, n // 2 + 17).astype(np.int64),
        "exceptions": exception_neighbourhood(col),
        "vector ends": np.concatenate([ends, ends + 1023]),
    }


def check_column(ctx, col, x=None, what=""):
    """every index set: gather == decode at those indices (and == x); plus a few slices"""
    ref = ibits(ctx.decode(col))
    if x is not None:
        assert torch.equal(ref, ibits(x)), f"{what}: decode(encode(x)) != x"
    for name, idx_np in index_sets(col).items():
        idx = torch.from_numpy(idx_np).to(DEV)
        got = ibits(ctx.gather(col, idx))
        assert torch.equal(got, ref[idx]), f"{what}: gather of {name} differs from the store decode"
    n = col.n_vectors * 1024
    for first, m in ((0, n), (1, n - 1), (1023, 2), (n // 2 + 333, n // 4), (n - 1, 1)):
        if first + m > n:  # (one-vector columns)
            continue
        got = ibits(ctx.decode_slice(col, first, m))
        assert torch.equal(got, ref[first:first + m]), f"{what}: slice ({first}, {m}) differs from the store decode"


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


@pytest.mark.parametrize("name", sorted(DOUBLE_COLUMNS) + sorted(FLOAT_COLUMNS))
def test_gather_and_slices_match_the_store_decode(ctx, name):
    x = (DOUBLE_COLUMNS.get(name) or FLOAT_COLUMNS[name])()
    col, xd = encoded(ctx, x)
    check_column(ctx, col, xd, name)


def test_golden_vectors_encoded_by_the_oracle(ctx, oracle):
    from oracle.pyoracle import OracleF32
    for name, x, _, _ in golden_io.first_vectors():
        col = capi.DeviceColumn.from_host(*layout.compact(oracle.encode_column(x)))
        check_column(ctx, col, torch.from_numpy(x.copy()).to(DEV), name)
    of = OracleF32()
    for name, x, _, _ in golden_io.float_vectors():
        col = capi.DeviceColumn.from_host(*layout.compact(of.encode_column(x), 4), dtype="f32")
        check_column(ctx, col, torch.from_numpy(x.copy()).to(DEV), name)


def test_columns_encoded_unordered_and_loaded_from_a_blob(ctx):
    x = np.concatenate([datagen.mixed_column(150, seed=31), datagen.rd_column(120, seed=32)])
    ctx.set_option(10, 1)  # ALPGPU_OPT_ENCODE_UNORDERED: records out of vector order
    try:
        col, xd = encoded(ctx, x)
        ctx.synchronize()
    finally:
        ctx.set_option(10, 0)
    check_column(ctx, col, xd, "unordered")
    for dt, xx in (("f64", x), ("f32", datagen.mixed_column_f32(170, seed=33))):
        c0, xd = encoded(ctx, xx)
        bcol, nv = ctx.from_blob(ctx.to_blob(c0, xx.size))
        assert nv == xx.size and bcol.dtype == dt
        check_column(ctx, bcol, xd, "from_blob " + dt)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_out_of_range_indices_give_the_canonical_nan(ctx, dtype):
    x = datagen.mixed_column(130, seed=41) if dtype == "f64" else datagen.mixed_column_f32(130, seed=41)
    col, xd = encoded(ctx, x)
    n = col.n_vectors * 1024
    bad = np.array([-1, np.iinfo(np.int64).min, n, np.iinfo(np.int64).max, n + 1, -1024], np.int64)
    good = np.random.default_rng(1).integers(0, n, 300).astype(np.int64)
    idx_np = np.concatenate([good, bad, good[::-1], bad[::-1]])
    np.random.default_rng(2).shuffle(idx_np)
    got = ibits(ctx.gather(col, torch.from_numpy(idx_np).to(DEV))).cpu().numpy()
    is_bad = (idx_np < 0) | (idx_np >= n)
    assert np.all(got[is_bad] == NAN_BITS[dtype])
    assert np.array_equal(got[~is_bad], ibits(xd).cpu().numpy()[idx_np[~is_bad]])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_sizes_write_exactly_n_values_and_leave_the_column_alone(ctx, dtype):
    x = datagen.mixed_column(250, seed=51) if dtype == "f64" else datagen.mixed_column_f32(250, seed=51)
    col, xd = encoded(ctx, x)
    ref = ibits(xd)
    before = [t.clone() for t in (col.rowgroups, col.vectors, col.packed, col.exc, col.totals)]
    tdt = torch.float64 if dtype == "f64" else torch.float32
    sentinel = 0x5A5A5A5A
    rng = np.random.default_rng(3)
    for n in (0, 1, 63, 65, 257, (1 << 25) + 17):
        idx = torch.from_numpy(rng.integers(0, col.n_vectors * 1024, n).astype(np.int64)).to(DEV)
        out = torch.empty(n + 64, dtype=tdt, device=DEV)
        ibits(out).fill_(sentinel)
        ctx.gather(col, idx, out)
        assert torch.equal(ibits(out)[:n], ref[idx]), f"gather of {n}"
        assert bool((ibits(out)[n:] == sentinel).all()), f"gather of {n} wrote past d_out[n]"
        m = min(n, col.n_vectors * 1024 - 77)
        ibits(out).fill_(sentinel)
        ctx.decode_slice(col, 77, m, out)
        assert torch.equal(ibits(out)[:m], ref[77:77 + m]), f"slice of {m}"
        assert bool((ibits(out)[m:] == sentinel).all()), f"slice of {m} wrote past d_out[n]"
        del idx, out
    ctx.synchronize()
    for a, b in zip(before, (col.rowgroups, col.vectors, col.packed, col.exc, col.totals)):
        assert torch.equal(a, b), "a gather or slice changed the column's buffers"


def one_vector_column(ctx, n_vectors, x):
    """a column of n_vectors vectors whose descriptors all point at the packed words and the exception record of the one encoded vector x (the
    store decode follows descriptors as found, so this is a valid column for it) -> (column, that vector decoded)"""
    src, _ = encoded(ctx, x)
    one = ctx.decode(src)
    rgs = src.rowgroups[:32]
    desc = src.vectors[:32]
    pb, eb = int(src.totals[0]), int(src.totals[1])
    col = capi.DeviceColumn(n_vectors, 0, packed_capacity=pb + 1024, exc_capacity=eb + 64, dtype=src.dtype, rd_order=False)
    col.rowgroups.view(-1, 32)[:] = rgs
    col.vectors.view(-1, 32)[:] = desc
    col.packed[:pb] = src.packed[:pb]
    col.exc[:eb] = src.exc[:eb]
    col.c.packed_bytes_hint, col.c.exc_bytes_hint = pb, eb
    return col, ibits(one)


@pytest.mark.parametrize("kind", ["alp", "rd"])
def test_indices_beyond_two_to_the_32(ctx, kind):
    x = datagen.mixed_column(1, seed=61) if kind == "alp" else datagen.rd_column(1, seed=62)
    nv = (1 << 22) + 3
    col, one = one_vector_column(ctx, nv, x)
    vec = col.vectors[:32].cpu().numpy().view(capi.VECTOR_DTYPE)
    assert int(vec["scheme"][0]) == (capi.SCHEME_ALP if kind == "alp" else capi.SCHEME_ALP_RD)
    assert kind == "rd" or int(vec["exc_cnt"][0]) > 0
    n = nv * 1024
    assert n > 1 << 32
    rng = np.random.default_rng(4)
    idx_np = np.concatenate([np.arange((1 << 32) - 1500, n, dtype=np.int64), rng.integers(1 << 32, n, 5000), rng.integers(0, n, 5000), [n, n + (1 << 32)]])
    got = ibits(ctx.gather(col, torch.from_numpy(idx_np).to(DEV))).cpu().numpy()
    want = one.cpu().numpy()[idx_np & 1023]
    want[idx_np >= n] = NAN_BITS["f64"]
    assert np.array_equal(got, want)
    first, m = (1 << 32) - 700, 2000
    got = ibits(ctx.decode_slice(col, first, m)).cpu().numpy()
    assert np.array_equal(got, one.cpu().numpy()[(np.arange(first, first + m) & 1023)])
    got = ibits(ctx.decode_slice(col, n - 3000, 3000)).cpu().numpy()
    assert np.array_equal(got, one.cpu().numpy()[(np.arange(n - 3000, n) & 1023)])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_slices(ctx, dtype):
    x = datagen.rd_column(250, seed=71) if dtype == "f64" else datagen.rd_column_f32(250, seed=71)
    col, xd = encoded(ctx, x)
    rg = col.to_host()[0]
    assert np.all(rg["scheme"] == capi.SCHEME_ALP_RD)
    ref = ibits(xd)
    n = col.n_vectors * 1024
    for first, m in ((0, n), (0, 1), (1, 1023), (1023, 2), (99 * 1024 + 5, 2000), (n - 1, 1), (149 * 1024 + 1000, 60 * 1024)):
        assert torch.equal(ibits(ctx.decode_slice(col, first, m)), ref[first:first + m]), f"slice ({first}, {m})"
    assert ctx.decode_slice(col, 0, 0).numel() == 0 and ctx.decode_slice(col, n, 0).numel() == 0
    tdt = torch.float64 if dtype == "f64" else torch.float32
    fn = getattr(capi.lib, "alpgpu_decode_slice_" + dtype)
    out = torch.zeros(4096, dtype=tdt, device=DEV)
    for first, m in ((n - 100, 101), (0, n + 1), (n + 1, 0), (2**64 - 1, 2), (2, 2**64 - 1)):
        assert fn(ctx.h, ctypes.byref(col.c), first, m, ctypes.c_void_p(out.data_ptr())) == -2, f"slice ({first}, {m}) must be refused"
    ctx.synchronize()
    assert bool((ibits(out) == 0).all()), "a refused slice wrote"


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
for dtype, x in (("f64", datagen.mixed_column(230, seed=81)), ("f32", datagen.mixed_column_f32(230, seed=82))):
    xd = torch.from_numpy(x).cuda()
    col = ctx.encode(xd)
    ctx.column_totals(col)               # hinted: a planned decode
    plan0 = ctx.decode_plan(col)
    n = col.n_vectors * 1024
    rng = np.random.default_rng(5)
    idx = torch.from_numpy(rng.integers(-5, n + 5, 70000).astype(np.int64)).cuda()
    tdt = xd.dtype
    out_g = torch.zeros(idx.numel(), dtype=tdt, device="cuda:0")
    out_s = torch.zeros(50000, dtype=tdt, device="cuda:0")
    with torch.cuda.stream(side):
        ctx.gather(col, idx, out_g)      # warm-up on the capture stream
        ctx.decode_slice(col, 12345, 50000, out_s)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ctx.gather(col, idx, out_g)
            ctx.decode_slice(col, 12345, 50000, out_s)
    for rep in range(3):
        idx.copy_(torch.from_numpy(rng.integers(-5, n + 5, idx.numel()).astype(np.int64)).cuda())  # rewritten in place
        torch.cuda.synchronize()
        out_g.zero_(); out_s.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager_g = ctx.gather(col, idx)
        eager_s = ctx.decode_slice(col, 12345, 50000)
        torch.cuda.synchronize()
        iv = torch.int64 if dtype == "f64" else torch.int32
        ok = ok and torch.equal(out_g.view(iv), eager_g.view(iv)) and torch.equal(out_s.view(iv), eager_s.view(iv))
    ok = ok and ctx.decode_plan(col) == plan0 and plan0 is not None
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_indices_change():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


def test_a_gather_leaves_the_decode_plan_alone(ctx):
    for hinted in (True, False):
        col, _ = encoded(ctx, datagen.mixed_column(150, seed=91))
        if hinted:
            ctx.column_totals(col)
        ctx.decode(col)
        ctx.synchronize()  # (what an unhinted decode learns about the column is in by now)
        before = ctx.decode_plan(col)
        ctx.gather(col, torch.arange(0, col.n_vectors * 1024, 7, dtype=torch.int64, device=DEV))
        ctx.decode_slice(col, 5, 9999)
        ctx.synchronize()
        assert ctx.decode_plan(col) == before


def test_python_rejects_index_tensors_that_are_not_contiguous_int64_on_the_device(ctx):
    col, _ = encoded(ctx, datagen.mixed_column(3, seed=95))
    out = torch.zeros(64, dtype=torch.float64, device=DEV)
    base = torch.arange(128, dtype=torch.int64, device=DEV)
    for bad in (base[:64].to(torch.int32), base[:64].cpu(), base[::2], [1, 2, 3], np.arange(64)):
        with pytest.raises(ValueError):
            ctx.gather(col, bad, out)
    ctx.synchronize()
    assert bool((out == 0).all()), "a refused gather launched"


def test_a_sparse_gather_is_faster_than_a_full_decode(ctx):
    """2^20 uniformly random indices (0.1 % of the values) of the benchmark's 1 Mi-vector mixed column against one store decode of it: medians
    of five, same process"""
    sys.path.insert(0, ROOT)
    import bench
    nv = 1 << 20
    x = bench.synthetic_input("mixed", nv, torch.device(DEV), seed=1)
    col = ctx.encode(x)
    del x
    ctx.column_totals(col)
    out = torch.empty(nv * 1024, dtype=torch.float64, device=DEV)
    idx = torch.randint(0, nv * 1024, (1 << 20,), dtype=torch.int64, device=DEV)
    gout = torch.empty(idx.numel(), dtype=torch.float64, device=DEV)

    def timed(fn):
        ts = []
        for _ in range(7):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts[2:]))

    t_decode = timed(lambda: ctx.decode(col, out))
    t_gather = timed(lambda: ctx.gather(col, idx, gout))
    print(f"gather of 2^20 random indices {t_gather:.3f} ms, decode of the column {t_decode:.3f} ms")
    assert torch.equal(ibits(gout), ibits(out)[idx])
    assert t_gather < t_decode


def test_cpp_column_take_matches_decompress(tmp_path):
    """include/alp/batch.hpp: alp::gpu::column<double / float>::take of a serialized column == decompress at those indices (tests/cpp/take_test.cpp)"""
    exe = tmp_path / "take_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/take_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", f"-Wl,-rpath,{ROOT}/alp_amd"])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(p.stdout)
    assert p.returncode == 0 and "take_test: 0 failures" in p.stdout, p.stdout[-3000:] + p.stderr[-2000:]
