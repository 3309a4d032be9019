"""GPU: every stream reader at stream offsets of 2^31, 2^32 and above.  A small column (about 500 vectors: narrow decimals, exception-heavy ALP rowgroups, ALP_RD
rowgroups) is encoded by the GPU, decoded at offset 0 and compared bit for bit with its INPUT; its records are then placed high in two streams of 2^32 + 64 MiB
(tests/high_offsets.py: a record boundary on 2^31, on 2^32, 2^32 inside an ALP vector's words and between an exception record's values and positions, 2^32 on an
ALP_RD vector's left block and inside its exception positions, everything at and above 2^32) and every reader runs on it: the store decodes of both precisions in
their launch shapes, the read-ahead, the unhinted decode, the sinks, gather / slices / selection / zone maps, the in-register consumers and the validator.

EVERY expectation is the input, directly or through the host replicas the feature suites share; no result of a GPU call is the expectation of another.  The buffers
are real allocations, zero outside the column's window: an offset that lost its upper half reads zeros of the same allocation and gives a wrong answer, not a fault.
tests/test_high_offsets_cpu.py checks, without a GPU, that the placements put their seams where they say."""
import contextlib

import numpy as np
import pytest
import torch

import high_offsets as ho
import layout
from bucket_replica import host_bucket_minmax, host_bucket_sum
from distinct_replica import host_distinct
from group_replica import host_group_sums
from histogram_replica import host_histogram
from in_list_replica import host_in_mask, pack_bits
from join_replica import host_join
from keyed_many_replica import host_keyed_minmax_many
from keyed_minmax_replica import host_keyed_minmax
from keyed_replica import host_keyed_sum
from keyed_replica import same_sums as same_keyed_sums
from minmax_replica import host_group_minmax, host_minmax_masked
from pair_replica import host_dots_masked
from quantile_replica import host_quantile, host_select_rank, sorted_selection
from test_decode_sum_gpu import host_column_total, host_sums, host_sums_f32, host_sums_pipelined
from test_float_widths_gpu import STREAMED
from test_mask_gpu import host_sums_masked, random_mask
from top_k_replica import host_top_k

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
SMALL_CASES = [f"{t}-{p}" for t in ("f64", "f32") for p in ho.PLACEMENTS]
LONG_F32_CASES = [f"f32-{p}" for p in ho.LONG_PLACEMENTS]
READ_AHEAD_CASES = [f"{t}-{p}" for t in ("f64", "f32") for p in ("seam_2_32", "all_above")]


# =====================================================================================================================================================
# the columns
# =====================================================================================================================================================
class World:
    """per value type: the high buffers, the two sources (encoded by the GPU from their inputs, checked at offset 0), the bitmaps and a memo of expectations"""

    def __init__(self, ctx, dtype):
        self.ctx, self.dtype = ctx, dtype
        self.W = 8 if dtype == "f64" else 4
        self.it = torch.int64 if dtype == "f64" else torch.int32
        self.sources, self.device_x, self.memo = {}, {}, {}
        self.high = ho.HighColumn(ctx, dtype, ho.LONG_VECTORS)

    def source(self, name):
        if name not in self.sources:
            x = ho.small_input(self.dtype) if name == "small" else ho.long_input(self.dtype)
            xd = torch.from_numpy(x).to(DEV)
            col = self.ctx.encode(xd)
            out = self.ctx.decode(col)
            self.ctx.synchronize()
            # before anything else: the column decoded at offset 0 is its input, bit for bit
            assert torch.equal(out.view(self.it), xd.view(self.it)), f"{name} {self.dtype}: decode(encode(x)) at offset 0 differs from x"
            pb, eb, ov = self.ctx.column_totals(col)
            assert ov == 0
            rg, vec, packed, exc = col.to_host()
            assert packed.size == pb and exc.size == eb
            src = ho.Source(name, self.dtype, x, rg.copy(), vec.copy(), packed, exc, ho.PLACEMENTS if name == "small" else ho.LONG_PLACEMENTS)
            psz, esz = ho.sizes(vec, self.W)
            assert np.array_equal(vec["packed_off"].astype(np.int64), np.concatenate([[0], np.cumsum(psz)[:-1]])), "records contiguous and in vector order"
            assert np.array_equal(vec["exc_off"].astype(np.int64), np.concatenate([[0], np.cumsum(esz)[:-1]]))
            self.sources[name], self.device_x[name] = src, xd
            if name == "small":
                rnd = random_mask(src.nv, 51)
                self.masks = {"full": torch.full_like(rnd, -1), "random": rnd}
                self.mask_bits = {k: np.unpackbits(m.cpu().numpy().view(np.uint8), bitorder="little").astype(bool).reshape(src.nv, 1024) for k, m in self.masks.items()}
                self.enc = layout.expand(src.rg, src.vec, src.packed, src.exc, self.W)  # (the float sums' replica wants the exception records)
                s = np.sort(x[np.isfinite(x)])
                self.q = lambda f: float(s[min(s.size - 1, int(f * s.size))])
        return self.sources[name]

    def once(self, key, fn):
        if key not in self.memo:
            self.memo[key] = fn()
        return self.memo[key]


_worlds = {}


@pytest.fixture(scope="module")
def worlds(ctx):
    def world(dtype):
        if dtype not in _worlds:
            _worlds[dtype] = World(ctx, dtype)
        return _worlds[dtype]
    yield world
    _worlds.clear()
    torch.cuda.empty_cache()


class Placed:
    def __init__(self, w, src, name, col, twin=None):
        self.w, self.src, self.name, self.col, self.twin = w, src, name, col, twin
        self.pl = src.placements[name]
        self.what = f"{src.name} {w.dtype} under {name}"


@pytest.fixture(params=SMALL_CASES)
def small(request, ctx, worlds):
    """the small column under one placement (and its twin at high_offsets.twin_shift in the same streams); validated.  (HighColumn.put does nothing when the placement is in place.)"""
    dtype, name = request.param.split("-")
    w = worlds(dtype)
    src = w.source("small")
    col = w.high.put(src, name, twin=True)
    assert ctx.column_validate(col) is None and ctx.column_validate(w.high.twin) is None, f"{request.param}: column_validate refuses the placement"
    return Placed(w, src, name, col, w.high.twin)


def put_long(ctx, worlds, case):
    dtype, name = case.split("-")
    w = worlds(dtype)
    src = w.source("long")
    col = w.high.put(src, name)
    assert ctx.column_validate(col) is None
    return Placed(w, src, name, col)


@contextlib.contextmanager
def options(ctx, **values):
    from alp_amd import capi
    ids = {"vpw": (capi.OPT_DECODE_VECTORS_PER_WG, 0), "plain": (capi.OPT_DECODE_PLAIN_STORES, 0), "sink": (capi.OPT_CONSUMER_PIPELINED, 0),
           "read_ahead": (capi.OPT_DECODE_READ_AHEAD, -1)}
    try:
        for k, v in values.items():
            ctx.set_option(ids[k][0], v)
        yield
    finally:
        for k in values:
            ctx.set_option(*ids[k])


@contextlib.contextmanager
def hints(col, packed, exc, rd):
    c = col.c
    truth = (int(c.packed_bytes_hint), int(c.exc_bytes_hint), int(c.alp_rd_rowgroups_hint))
    try:
        c.packed_bytes_hint, c.exc_bytes_hint, c.alp_rd_rowgroups_hint = packed, exc, rd
        yield
    finally:
        c.packed_bytes_hint, c.exc_bytes_hint, c.alp_rd_rowgroups_hint = truth


# ---- comparisons ----------------------------------------------------------------------------------------------------------------------------------
def describe(p, bad_vectors):
    v, pl = p.src.vec, p.pl
    rows = [(int(i), int(v["scheme"][i]), int(v["bw"][i]), int(v["lbw"][i]), int(v["exc_cnt"][i]), hex(int(v["packed_off"][i]) + pl.p_shift), hex(int(v["exc_off"][i]) + pl.e_shift))
            for i in bad_vectors[:6]]
    return f"{p.what}: {len(bad_vectors)} vectors differ; (vector, scheme, bw, lbw, exc_cnt, packed_off, exc_off): {rows}; seam vectors {pl.p_vector} (packed), {pl.e_vector} (exceptions)"


def assert_decoded(p, out, what):
    x = p.w.device_x[p.src.name]
    same = (out.view(p.w.it) == x.view(p.w.it)).view(-1, 1024).all(dim=1)
    if not bool(same.all()):
        pytest.fail(f"{what}: " + describe(p, torch.nonzero(~same).reshape(-1).cpu().numpy()))


def assert_per_vector(p, same, what):
    same = np.asarray(same)
    if not same.all():
        pytest.fail(f"{what}: " + describe(p, np.nonzero(~same.reshape(-1, p.src.nv).all(axis=0))[0]))


def assert_values(p, got, idx_np, what):
    g = got.cpu().numpy().view(p.src.bits.dtype)
    same = g == p.src.bits[idx_np]
    if not same.all():
        pytest.fail(f"{what}: " + describe(p, np.unique(np.asarray(idx_np)[~same] >> 10)))


def assert_bitmap(p, got, want_bits, what):
    g = got.cpu().numpy().view(np.uint64)
    w = pack_bits(want_bits)
    if not np.array_equal(g, w):
        pytest.fail(f"{what}: " + describe(p, np.nonzero((g ^ w).reshape(-1, 16).any(axis=1))[0]))


def same_sums(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))


def ints(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def band(p):
    """a closed range whose bounds are values of the column: the middle half of its finite values"""
    return p.w.q(0.25), p.w.q(0.75)


def qualifies(p, lo, hi):
    t = p.src.x.dtype.type
    with np.errstate(invalid="ignore"):
        return (p.src.values >= t(lo)) & (p.src.values <= t(hi))


# =====================================================================================================================================================
# the store decode
# =====================================================================================================================================================
def test_store_decode(ctx, small):
    """k_decode_column: one and two vectors per workgroup, non-temporal and plain stores, and the 256-entry exception stage; the variant word says which ran"""
    p = small
    if p.w.dtype != "f64":
        return float_store_decode(ctx, p)
    for vpw in (1, 2):
        for plain in (0, 1):
            with options(ctx, vpw=vpw, plain=plain):
                plan = ctx.decode_plan(p.col)
                assert plan is not None and (plan["word"] & 1) == (vpw == 1) and bool(plan["word"] & 2) == bool(plain) and not plan["many_exc"], plan
                out = ctx.decode(p.col)
                ctx.synchronize()
            assert_decoded(p, out, f"{vpw} vectors per workgroup, {'plain' if plain else 'non-temporal'} stores")
    # the hints steer the launch, never the bytes: those of an exception-heavy wide ALP column select the 256-entry stage
    with hints(p.col, 23 * 128 * p.src.nv, 1280 * p.src.nv, 1):
        plan = ctx.decode_plan(p.col)
        assert plan is not None and plan["many_exc"] and plan["vectors_per_wg"] == 1 and plan["word"] & 64, plan
        out = ctx.decode(p.col)
        ctx.synchronize()
    assert_decoded(p, out, "the 256-entry exception stage")
    out = ctx.decode(p.col)
    ctx.synchronize()
    assert_decoded(p, out, "the rule's own shape")


def float_store_decode(ctx, p):
    """shapes 1, 2, 4 (staged), 8 (one wavefront per vector) and every streamed shape"""
    for shape in [1, 2, 4, 8] + STREAMED:
        with options(ctx, vpw=shape):
            plan = ctx.decode_plan(p.col)
            assert plan is not None and plan["vectors_per_wg"] == shape, (shape, plan)
            out = ctx.decode(p.col)
            ctx.synchronize()
        assert_decoded(p, out, f"float shape {shape}")
    out = ctx.decode(p.col)
    ctx.synchronize()
    assert_decoded(p, out, "the rule's own shape")


@pytest.mark.parametrize("case", LONG_F32_CASES)
def test_streamed_float_decode_of_the_long_column(ctx, worlds, case):
    """chunks of 12 (and of every other streamed shape's size) straddle the seam in the flat arm: 33 068 contiguous narrow records"""
    p = put_long(ctx, worlds, case)
    for shape in STREAMED:
        with options(ctx, vpw=shape):
            assert ctx.decode_vectors_per_wg(p.col) == shape
            out = ctx.decode(p.col)
            ctx.synchronize()
        assert_decoded(p, out, f"streamed shape {shape}")
        del out


READ_AHEAD_REPEAT = 32


@pytest.mark.parametrize("case", READ_AHEAD_CASES)
def test_read_ahead_beside_the_decode(ctx, worlds, case):
    """ALPGPU_OPT_DECODE_READ_AHEAD = 1 on the long column: the read-ahead's wave reductions and shuffles of offsets at and above 2^32.  The decode of 33 068 narrow
    vectors is over (some 20 us) before a kernel launched behind it on a second stream reads its first progress word, and a read-ahead that finds the decode past its
    batches reads none; so the long column's whole rowgroups are described 32 times over — 1 056 000 vectors through the same high records, as
    tests/test_gather_gpu.py: one_vector_column does with one record — a decode of a millisecond or more.  The first decode of the two loads the kernels' code
    and writes a fresh output, after which a read-ahead may find the decode gone; the batches are counted over the second, into the same output.
    A float column of this width is streamed by the rule, without a read-ahead: two vectors per workgroup are forced for it, as that suite does."""
    dtype, name = case.split("-")
    w = worlds(dtype)
    src = w.source("long")
    col = w.high.put(src, name, repeat=READ_AHEAD_REPEAT)
    assert ctx.column_validate(col) is None
    p = Placed(w, src, name, col)
    whole = src.nv // 100 * 100
    assert col.n_vectors == READ_AHEAD_REPEAT * whole
    forced = {"vpw": 2} if dtype == "f32" else {}
    with options(ctx, read_ahead=1, **forced):
        assert ctx.decode_reads_ahead(col)
        first = ctx.read_ahead_batches()
        out = ctx.decode(col)
        before = ctx.read_ahead_batches()
        ctx.decode(col, out.zero_())
        ctx.synchronize()
    grown = ctx.read_ahead_batches() - before
    print(f"{p.what}: the read-ahead read {before - first}, then {grown} batches of 64 vectors of {col.n_vectors // 64}")
    assert grown > 0, "the read-ahead did not run"
    x = w.device_x["long"][:whole * 1024]
    same = (out.view(w.it).view(READ_AHEAD_REPEAT, whole, 1024) == x.view(w.it).view(1, whole, 1024)).all(dim=2)
    if not bool(same.all()):
        pytest.fail("decode with the read-ahead beside it: " + describe(p, np.unique(torch.nonzero(~same)[:, 1].cpu().numpy())))


def test_unhinted_decode(ctx, small):
    """both size hints 0 and fewer than 65 536 vectors: the one-vector shape (float: two), planned without the column's sizes"""
    p = small
    with hints(p.col, 0, 0, 0):
        ctx.forget(p.col)
        plan = ctx.decode_plan(p.col)
        assert plan is not None and (plan["packed_bytes"], plan["exc_bytes"]) == (0, 0), plan
        assert plan["vectors_per_wg"] == (1 if p.w.dtype == "f64" else 2), plan
        out = ctx.decode(p.col)
        ctx.synchronize()
    ctx.forget(p.col)
    assert_decoded(p, out, "no hints")


# =====================================================================================================================================================
# the sinks
# =====================================================================================================================================================
@pytest.mark.parametrize("sink", [0, 1, 3])
def test_sinks(ctx, small, sink):
    """decode_sum, decode_count_range and column_sum under ALPGPU_OPT_CONSUMER_PIPELINED 0 (the per-column choice), 1 (double: the ring kernel, whose order is its
    own; float: the staged kernel) and 3 (four wavefronts per vector)"""
    p, w = small, small.w
    if w.dtype == "f64":
        order = host_sums_pipelined if sink == 1 else host_sums
        want = w.once(("sums", order.__name__), lambda: order(p.src.values))
    else:
        want = w.once("sums", lambda: host_sums_f32(p.src.values, w.enc))
    lo, hi = band(p)
    with options(ctx, sink=sink):
        got = ctx.decode_sum(p.col)
        total = ctx.column_sum(p.col)
        cnt = ctx.decode_count_range(p.col, lo, hi)
        ctx.synchronize()
    assert np.isfinite(want).sum() * 2 >= want.size
    assert_per_vector(p, same_sums(got.cpu().numpy(), want), f"decode_sum, sink option {sink}")
    assert same_sums(total.cpu().numpy(), np.array([host_column_total(want)])).all(), f"{p.what}: column_sum, sink option {sink}"
    want_cnt = qualifies(p, lo, hi).sum(axis=1)
    assert 0 < want_cnt.sum() < p.src.x.size
    assert_per_vector(p, cnt.cpu().numpy().astype(np.int64) == want_cnt, f"decode_count_range, sink option {sink}")


# =====================================================================================================================================================
# random access and selection
# =====================================================================================================================================================
def seam_vectors(p):
    return sorted({p.pl.p_vector, p.pl.e_vector})


def test_gather_and_slices(ctx, small):
    p = small
    n = p.src.x.size
    sets = {"a permutation of everything": np.random.default_rng(17).permutation(n)}
    for v in seam_vectors(p):
        lo = max(0, v - 1) * 1024
        sets[f"the 2048 indices around vector {v}"] = np.arange(lo, lo + 2048)
    for name, idx_np in sets.items():
        idx_np = np.ascontiguousarray(idx_np, dtype=np.int64)
        assert_values(p, ctx.gather(p.col, torch.from_numpy(idx_np).to(DEV)), idx_np, f"gather of {name}")
    for v in seam_vectors(p):  # slices that start and end inside the seam vector
        for first, m in ((v * 1024 + 5, 1000), (v * 1024 + 1023, 1), (max(0, v * 1024 - 300), 700), (v * 1024 + 700, min(2000, n - v * 1024 - 700)), (v * 1024, 1024)):
            assert_values(p, ctx.decode_slice(p.col, first, m), np.arange(first, first + m), f"slice ({first}, {m}) at vector {v}")
    assert_values(p, ctx.decode_slice(p.col, 1, n - 2), np.arange(1, n - 1), "the slice of nearly everything")


def test_selection_and_zone_maps(ctx, small):
    """select_range, zone_map, and select_range_zoned with the column's own zone map"""
    p, w = small, small.w
    lo, hi = band(p)
    want_idx = w.once("select", lambda: np.nonzero(qualifies(p, lo, hi).reshape(-1))[0])
    idx, vals = ctx.select_range(p.col, lo, hi, values=True)
    got = idx.cpu().numpy()
    if not np.array_equal(got, want_idx):
        pytest.fail("select_range: " + describe(p, np.unique(np.setxor1d(got, want_idx) >> 10)))
    assert_values(p, vals, want_idx, "select_range values")
    zones = ctx.zone_map(p.col)
    want_z = w.once("zones", lambda: host_minmax_masked(p.src.values, np.ones((p.src.nv, 1024), bool))[0])
    assert_per_vector(p, (ints(zones) == ints(want_z)).all(axis=1), "zone_map")
    # the zoned selection against the host's records: a narrow band that lets the records skip some vectors and not all
    lo2, hi2 = w.q(0.02), w.q(0.10)
    with np.errstate(invalid="ignore"):
        skipped = ~((want_z[:, 1] >= lo2) & (want_z[:, 0] <= hi2))
    assert 0 < skipped.sum() < p.src.nv
    want2 = w.once("select2", lambda: np.nonzero(qualifies(p, lo2, hi2).reshape(-1))[0])
    for a, b, want in ((lo, hi, want_idx), (lo2, hi2, want2)):
        idx, vals = ctx.select_range(p.col, a, b, values=True, zones=zones)
        got = idx.cpu().numpy()
        if not np.array_equal(got, want):
            pytest.fail("select_range_zoned: " + describe(p, np.unique(np.setxor1d(got, want) >> 10)))
        assert_values(p, vals, want, "select_range_zoned values")


# =====================================================================================================================================================
# the in-register consumers
# =====================================================================================================================================================
def test_select_mask_sum_masked_and_decode_masked(ctx, small):
    p, w = small, small.w
    lo, hi = band(p)
    q = qualifies(p, lo, hi)
    assert_bitmap(p, ctx.select_mask(p.col, lo, hi), q, "select_mask SET")
    mask = w.masks["random"].clone()
    ctx.select_mask(p.col, lo, hi, op="and", mask=mask)
    assert_bitmap(p, mask, w.mask_bits["random"] & q, "select_mask AND")
    for mname in ("full", "random"):
        bits = w.mask_bits[mname]
        want = w.once(("sum_masked", mname), lambda: host_sums_masked(p.src.values, bits))
        counts = torch.full((p.src.nv,), 7, dtype=torch.int32, device=DEV)
        got = ctx.decode_sum_masked(p.col, w.masks[mname], counts=counts).cpu().numpy()
        assert_per_vector(p, same_sums(got, want), f"decode_sum_masked under the {mname} bitmap")
        assert np.array_equal(counts.cpu().numpy(), bits.sum(axis=1).astype(np.int32))
        idx, vals = ctx.decode_masked(p.col, w.masks[mname], indices=True)
        want_idx = np.nonzero(bits.reshape(-1))[0]
        assert np.array_equal(idx.cpu().numpy(), want_idx)
        assert_values(p, vals, want_idx, f"decode_masked under the {mname} bitmap")


def test_two_column_kernels(ctx, small):
    """compare_mask and decode_dot_masked: the second operand is the same column under another placement (its twin, high_offsets.twin_shift), so both carry high offsets
    that differ"""
    p, w = small, small.w
    assert ho.twin_shift(p.name) not in (p.pl.p_shift, p.pl.e_shift)
    nan = np.isnan(p.src.values)
    assert_bitmap(p, ctx.compare_mask(p.col, p.twin, "eq"), ~nan, "compare_mask(col, twin, eq)")
    assert_bitmap(p, ctx.compare_mask(p.twin, p.col, "lt"), np.zeros_like(nan), "compare_mask(twin, col, lt)")
    for mname in ("full", "random"):
        want = w.once(("dot", mname), lambda: host_dots_masked(p.src.values, p.src.values, w.mask_bits[mname]))
        got = ctx.decode_dot_masked(p.col, p.twin, w.masks[mname]).cpu().numpy()
        assert_per_vector(p, same_sums(got, want), f"decode_dot_masked(col, twin) under the {mname} bitmap")


def groups(w):
    cuts = [w.q(f) for f in (0.0, 0.3, 0.6, 1.0)]
    g = list(zip(cuts[:-1], cuts[1:])) + [(w.q(0.2), w.q(0.8))]
    return [a for a, _ in g], [b for _, b in g]


def test_grouped_and_masked_aggregates(ctx, small):
    """decode_group_sum, decode_minmax_masked, decode_group_minmax: the value column is the column, the key column its twin"""
    p, w = small, small.w
    lo, hi = groups(w)
    for mname in ("full", "random"):
        bits, mask = w.mask_bits[mname], w.masks[mname]
        want_s, want_c = w.once(("group_sum", mname), lambda: host_group_sums(p.src.values, p.src.values, bits, lo, hi))
        counts = torch.full((len(lo), p.src.nv), 7, dtype=torch.int32, device=DEV)
        got = ctx.decode_group_sum(p.col, p.twin, mask, lo, hi, counts=counts).cpu().numpy()
        assert_per_vector(p, same_sums(got, want_s), f"decode_group_sum under the {mname} bitmap")
        assert_per_vector(p, counts.cpu().numpy() == want_c.astype(np.int32), f"decode_group_sum counts under the {mname} bitmap")
        want_z, want_c = w.once(("minmax", mname), lambda: host_minmax_masked(p.src.values, bits))
        got = ctx.decode_minmax_masked(p.col, mask, counts=(counts1 := torch.full((p.src.nv,), 7, dtype=torch.int32, device=DEV)))
        assert_per_vector(p, (ints(got) == ints(want_z)).all(axis=1), f"decode_minmax_masked under the {mname} bitmap")
        assert np.array_equal(counts1.cpu().numpy(), want_c.astype(np.int32))
        want_z, want_c = w.once(("group_minmax", mname), lambda: host_group_minmax(p.src.values, p.src.values, bits, lo, hi))
        got = ctx.decode_group_minmax(p.twin, p.col, mask, lo, hi)
        assert_per_vector(p, (ints(got) == ints(want_z)).all(axis=2), f"decode_group_minmax under the {mname} bitmap")


def test_select_in_mask_on_both_arms(ctx, small):
    """the whole list in LDS (50 elements) and pivots in LDS with the list in device memory (lds_max + 1 elements)"""
    p, w = small, small.w
    lds_max = ctx.in_list_lds_max(w.dtype)
    for size in (50, lds_max + 1):
        def make():
            rng = np.random.default_rng(70 + size)
            lst = p.src.x[rng.choice(p.src.x.size, size, replace=False)].copy()
            lst[np.isnan(lst)] = 12345.678
            return lst, host_in_mask(p.src.x, lst).reshape(p.src.nv, 1024)
        lst, member = w.once(("in_list", size), make)
        assert 0 < member.sum() < member.size
        assert_bitmap(p, ctx.select_in_mask(p.col, torch.from_numpy(lst).to(DEV)), member, f"select_in_mask, list of {size}")


def test_top_k_ranks_and_quantiles(ctx, small):
    p, w = small, small.w
    for mname in ("full", "random"):
        bits, mask = w.mask_bits[mname].reshape(-1), w.masks[mname]
        for largest in (True, False):
            want_v, want_i = w.once(("top_k", mname, largest), lambda: host_top_k(p.src.x, bits, 1024, largest))
            vals, idx = ctx.top_k(p.col, mask, 1024, largest=largest)
            assert np.array_equal(ints(vals), ints(want_v)) and np.array_equal(idx.cpu().numpy(), want_i), f"{p.what}: top_k {mname} largest={largest}"
        s = w.once(("sorted", mname), lambda: sorted_selection(p.src.x, bits))
        ranks = [int(r) for r in np.linspace(0, s.size - 1, 32).astype(np.int64)]
        want_v, want_n = host_select_rank(s, ranks)
        vals, n = ctx.select_rank(p.col, mask, ranks)
        assert n == want_n and np.array_equal(ints(vals), ints(want_v)), f"{p.what}: select_rank {mname}"
        qs = [0.0, 0.1, 0.5, 0.77, 1.0]
        pairs, _, _ = host_quantile(s, qs)
        for side, method in enumerate(("lower", "higher")):
            got = ctx.quantile(p.col, mask, qs, interpolation=method)
            assert np.array_equal(ints(got), ints(np.ascontiguousarray(pairs[:, side]))), f"{p.what}: quantile {method} {mname}"


def edges_of(w, n):
    return np.unique(np.array([w.q(f) for f in np.linspace(0.02, 0.98, n)], dtype=np.float64 if w.dtype == "f64" else np.float32))


def test_histogram_join_probe_and_distinct(ctx, small):
    from alp_amd import capi
    p, w = small, small.w
    edges = edges_of(w, 40)
    keys = w.once("join_keys", lambda: np.unique(p.src.x[:100 * 1024]))  # the narrow rowgroup's values: a few hundred sorted keys
    assert not np.isnan(keys).any() and 50 < keys.size < 2000
    for mname in ("full", "random"):
        bits, mask = w.mask_bits[mname].reshape(-1), w.masks[mname]
        want = w.once(("histogram", mname), lambda: host_histogram(p.src.x, edges, bits))
        got = ctx.histogram(p.col, edges, mask=mask, sorted=True)
        assert np.array_equal(got.cpu().numpy().astype(np.uint64), want.astype(np.uint64)), f"{p.what}: histogram {mname}"
        want_idx, want_pos, want_span = w.once(("join", mname), lambda: host_join(p.src.x, keys, mask.cpu().numpy()))
        pos, span, idx = ctx.join_probe(p.col, keys, mask=mask, span=True, indices=True, sorted=True)
        assert np.array_equal(idx.cpu().numpy(), want_idx)
        bad = (pos.cpu().numpy() != want_pos) | (span.cpu().numpy().astype(np.int64) != np.asarray(want_span).astype(np.int64))
        if bad.any():
            pytest.fail(f"join_probe {mname}: " + describe(p, np.unique(want_idx[bad] >> 10)))
        assert (want_pos != capi.JOIN_NO_MATCH).any() and (want_pos == capi.JOIN_NO_MATCH).any()
        want_v, want_c, want_nan, _ = w.once(("distinct", mname), lambda: host_distinct(p.src.x, bits))
        vals, cnt, n_nan, overflow = ctx.distinct(p.col, mask=mask, capacity=capi.DISTINCT_MAX)
        assert not overflow and n_nan == want_nan, f"{p.what}: distinct {mname}"
        assert np.array_equal(ints(vals), ints(want_v)) and np.array_equal(cnt.cpu().numpy().astype(np.uint64), np.asarray(want_c).astype(np.uint64)), f"{p.what}: distinct {mname}"


def test_keyed_and_bucketed_aggregates(ctx, small):
    """decode_keyed_sum (double only), decode_keyed_minmax, decode_keyed_minmax_many, decode_bucket_sum, decode_bucket_minmax: values from the column, keys from its twin"""
    p, w = small, small.w
    x = p.src.x
    keys = w.once("keys", lambda: np.unique(x[:100 * 1024])[:1024])
    many = w.once("many_keys", lambda: np.unique(x[np.isfinite(x)])[::37][:6000])
    assert keys.size > 50 and many.size > 1024
    edges = edges_of(w, 15)
    for mname in ("full", "random"):
        bits, mask = w.mask_bits[mname].reshape(-1), w.masks[mname]
        if w.dtype == "f64":
            want_s, want_c = w.once(("keyed_sum", mname), lambda: host_keyed_sum(x, x, bits, keys))
            sums, cnt, unmatched = ctx.keyed_sum(p.col, p.twin, keys, mask=mask, sorted=True)
            assert same_keyed_sums(sums.cpu().numpy(), want_s), f"{p.what}: keyed_sum {mname}"
            assert np.array_equal(cnt.cpu().numpy(), want_c[:-1]) and int(unmatched) == int(want_c[-1]), f"{p.what}: keyed_sum counts {mname}"
        want_r, want_c = w.once(("keyed_minmax", mname), lambda: host_keyed_minmax(x, x, bits, keys))
        rec, cnt, unmatched = ctx.keyed_minmax(p.twin, p.col, keys, mask=mask, sorted=True)
        assert np.array_equal(ints(rec), ints(want_r)) and np.array_equal(cnt.cpu().numpy(), want_c[:-1]) and int(unmatched) == int(want_c[-1]), f"{p.what}: keyed_minmax {mname}"
        want_r, want_c = w.once(("keyed_minmax_many", mname), lambda: host_keyed_minmax_many(x, x, bits, many))
        rec, cnt, unmatched = ctx.keyed_minmax_many(p.col, p.twin, many, mask=mask)
        assert np.array_equal(ints(rec), ints(want_r)) and np.array_equal(cnt.cpu().numpy(), want_c[:-1]) and int(unmatched) == int(want_c[-1]), f"{p.what}: keyed_minmax_many {mname}"
        want_s, want_c = w.once(("bucket_sum", mname), lambda: host_bucket_sum(x, x, bits, edges))
        sums, cnt = ctx.bucket_sum(p.col, p.twin, edges, mask=mask, sorted=True)
        assert same_keyed_sums(sums.cpu().numpy(), want_s) and np.array_equal(cnt.cpu().numpy(), want_c), f"{p.what}: bucket_sum {mname}"
        want_r, want_c = w.once(("bucket_minmax", mname), lambda: host_bucket_minmax(x, x, bits, edges))
        rec, cnt = ctx.bucket_minmax(p.twin, p.col, edges, mask=mask, sorted=True)
        assert np.array_equal(ints(rec), ints(want_r)) and np.array_equal(cnt.cpu().numpy(), want_c), f"{p.what}: bucket_minmax {mname}"


# =====================================================================================================================================================
# validation
# =====================================================================================================================================================
def test_the_validator_reads_the_seam_record(ctx, small):
    """column_validate accepts the placement; with one exception position of the seam record set to 1024 it reports that vector (the only edit of a record)"""
    from alp_amd import capi
    p = small
    v = p.src.vec
    m = p.pl.e_vector if v["exc_cnt"][p.pl.e_vector] > 0 else int(np.nonzero(v["exc_cnt"])[0][0])
    c = int(v["exc_cnt"][m])
    value_bytes = p.w.W if v["scheme"][m] == capi.SCHEME_ALP else 2
    at = int(v["exc_off"][m]) + p.pl.e_shift + value_bytes * c + 2 * (c - 1)  # the record's last position
    exc = p.w.high.col.exc
    assert ctx.column_validate(p.col) is None
    saved = exc[at:at + 2].clone()
    try:
        exc[at:at + 2] = torch.tensor([0x00, 0x04], dtype=torch.uint8, device=exc.device)  # 1024, little-endian
        assert ctx.column_validate(p.col) == m, f"{p.what}: the bad position of vector {m} at byte {at:#x} of the exception stream"
    finally:
        exc[at:at + 2] = saved
    assert ctx.column_validate(p.col) is None
