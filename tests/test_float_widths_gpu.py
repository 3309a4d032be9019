"""GPU: every float kernel at every packed width 0..32, bit for bit against the float oracle (oracle/pyoracle.py: OracleF32, itself pinned to the reference by
tests/test_oracle_f32.py).  No result of the GPU is ever the expectation of another; everything is compared on uint32 views (-0.0, NaN payloads).

  1. datagen.every_bit_width_column_f32 (ALP vectors of every width 0..32 the reference's own search arrives at) through every encode route, alone and between
     ALP_RD and decimal rowgroups: the oracle's streams byte for byte, and the input bits back.
  2. hand-built vectors (float_rows.py) — every width x every factor with bases on the bounds of the conversion shortcut, exception records of every staging
     class, every ALP_RD cut — through every launch shape of the store decode (staged 1 / 2 / 4, wave-direct 8, streamed 16..30), in vector order and with
     their records shuffled in the streams; chunks that straddle every streamed arena; and long exception-free columns on which the rule itself streams.
  3. the other float read paths on the same columns: SUM, COUNT, zone maps, gather, slices, plain and zoned selection.
tests/test_float_widths_cpu.py checks, without a GPU, that these inputs are what they claim to be."""
import contextlib

import numpy as np
import pytest
import torch

import datagen
import float_rows as fr
import layout
import test_float_gpu as tf
import test_select_gpu as ts
import test_zone_gpu as tz
from test_decode_sum_gpu import host_sums_f32, kernel_f32  # noqa: F401  (kernel_f32: the fixture over the three consumer kernels)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STAGED_AND_DIRECT = [0, 1, 2, 4, 8]
STREAMED = list(range(16, 31))


@pytest.fixture(scope="module")
def of32():
    from oracle.pyoracle import OracleF32
    return OracleF32()


def upload(enc):
    from alp_amd import capi
    return capi.DeviceColumn.from_host(*layout.compact(enc, 4), dtype="f32")


def decode_bits(ctx, col):
    out = ctx.decode(col)
    ctx.synchronize()
    return out.cpu().numpy().view(np.uint32)


def describe_bad_rows(enc, got, want, limit=6):
    """the first vectors whose bits differ, as (vector, bw, f, e, base, exc_cnt) and their first bad value index"""
    bad = np.nonzero((got.reshape(-1, 1024) != want.reshape(-1, 1024)).any(axis=1))[0]
    rows = [(int(v), int(enc["bw"][v]), int(enc["f"][v]), int(enc["e"][v]), int(enc["base"][v]), int(enc["exc_cnt"][v]),
             "scheme %d lbw %d" % (int(enc["scheme"][v]), int(enc["lbw"][v])), "first bad value %d" % int(np.nonzero(got.reshape(-1, 1024)[v] != want.reshape(-1, 1024)[v])[0][0]))
            for v in bad[:limit]]
    return f"{bad.size} vectors differ; (vector, bw, f, e, base, exc_cnt): {rows}"


class Built:
    """a hand-built encoding, the oracle's decode of it, and the column in HBM"""

    def __init__(self, ctx, of32, enc):
        self.enc = enc
        self.want = of32.decode_column(enc)
        self.bits = self.want.view(np.uint32)
        self.col = upload(enc)
        assert ctx.column_validate(self.col) is None, "the hand-built descriptors are ones the kernels are specified for"
        self.x = torch.from_numpy(self.want).to(DEV)


@pytest.fixture(scope="module")
def rows(ctx, of32):
    """the ALP rows (3200 vectors) followed by the ALP_RD rows (one rowgroup per cut)"""
    return Built(ctx, of32, fr.concat_encodings([fr.alp_rows(), fr.rd_rows()]))


@pytest.fixture(scope="module")
def arena(ctx, of32):
    enc, where, skewed = fr.arena_column()
    b = Built(ctx, of32, enc)
    b.where, b.skewed = where, skewed
    return b


@pytest.fixture(scope="module")
def generated(ctx, of32):
    """the every-width column as the ORACLE encodes it (section 3 reads it; section 1 compares the GPU's encode with it)"""
    col = datagen.every_bit_width_column_f32(233, seed=10, exceptions=True)
    b = Built(ctx, of32, of32.encode_column(col))
    assert np.array_equal(b.bits, col.view(np.uint32))
    return b


@contextlib.contextmanager
def forced_shape(ctx, shape):
    from alp_amd import capi
    ctx.set_option(capi.OPT_DECODE_VECTORS_PER_WG, shape)
    try:
        yield
    finally:
        ctx.set_option(capi.OPT_DECODE_VECTORS_PER_WG, 0)


# =====================================================================================================================================================
# 1. a float column of every width through the encoder
# =====================================================================================================================================================
ENCODE_COLUMNS = {
    "every_width_exc": lambda: datagen.every_bit_width_column_f32(200, seed=77, exceptions=True),
    "every_width_clean": lambda: datagen.every_bit_width_column_f32(200, seed=77, exceptions=False),
    "between_rd_and_mixed": lambda: np.concatenate([datagen.every_bit_width_column_f32(200, seed=9, exceptions=True), datagen.rd_column_f32(100, seed=41),
                                                    datagen.mixed_column_f32(100, seed=42, exc_rate=0.02), datagen.every_bit_width_column_f32(133, seed=10, exceptions=True)]),
}


def assert_streams_are_the_oracles(dcol, want, what):
    """what test_synthetic_float_columns_encode_bit_exact compares: states, descriptors (offsets included) and both streams, byte for byte"""
    for a, b, part in zip(dcol.to_host(), layout.compact(want, 4), ("rowgroup states", "descriptors", "packed stream", "exception stream")):
        assert a.size == b.size and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: {part} differ from the oracle's"


@pytest.mark.parametrize("route", ["single_pass", "two_pass"])
@pytest.mark.parametrize("name", list(ENCODE_COLUMNS))
def test_every_width_column_encodes_to_the_oracles_bytes(ctx, of32, name, route):
    from alp_amd import capi
    col_np = ENCODE_COLUMNS[name]()
    want = of32.encode_column(col_np)
    assert set(range(33)) <= set(want["bw"][want["scheme"] == 2].tolist())
    ctx.set_option(capi.OPT_ENCODE_TWO_PASS, 1 if route == "two_pass" else 0)
    try:
        dcol, x = tf.gpu_encode(ctx, col_np)
    finally:
        ctx.set_option(capi.OPT_ENCODE_TWO_PASS, 0)
    assert_streams_are_the_oracles(dcol, want, f"{name} {route}")
    got = layout.expand(*dcol.to_host(), 4)
    tf.assert_parts_equal(got, want, name)
    out = ctx.decode(dcol)
    ctx.synchronize()
    assert torch.equal(out.view(torch.int32), x.view(torch.int32)), f"{name} {route}: decode(encode(x)) differs from the input bits"


@pytest.mark.parametrize("name", list(ENCODE_COLUMNS))
def test_every_width_column_encoded_unordered(ctx, of32, name):
    """as test_unordered_float_encode_writes_the_same_records_somewhere_else: every record is the oracle's, the records tile the streams"""
    from alp_amd import capi
    import test_encode_gpu
    col_np = ENCODE_COLUMNS[name]()
    want = of32.encode_column(col_np)
    try:
        ctx.set_option(capi.OPT_ENCODE_UNORDERED, 1)
        dcol, x = tf.gpu_encode(ctx, col_np)
    finally:
        ctx.set_option(capi.OPT_ENCODE_UNORDERED, 0)
    rg, vec, packed, exc = dcol.to_host()
    got = layout.expand(rg, vec, packed, exc, 4)
    tf.assert_parts_equal(got, want, name)
    assert np.array_equal(got["packed_left"], want["packed_left"])
    pb, eb, ov = ctx.column_totals(dcol)
    test_encode_gpu._assert_records_tile_the_streams(vec, pb, eb, value_bytes=4)
    for shape in (0, 2, 8, 27):  # (records out of vector order: the streamed decode copies them vector by vector)
        with forced_shape(ctx, shape):
            out = ctx.decode(dcol)
            ctx.synchronize()
        assert torch.equal(out.view(torch.int32), x.view(torch.int32)), (name, shape)


@pytest.mark.parametrize("async_mode", [1, 2])
def test_every_width_column_with_the_search_beside_the_encode(ctx, of32, async_mode):
    """ALPGPU_OPT_ENCODE_ASYNC_INIT 1 and 2 (tests/test_async_init_gpu.py) take effect from 1024 rowgroups on: the 400-vector column `between_rd_and_mixed`
    (every-width ALP, ALP_RD, decimals with exceptions) repeated 262 times in HBM.  The rowgroups repeat, so the expectation is the oracle's encoding of
    one period, tiled: states and descriptor fields as they are, offsets advanced by the period's stream sizes, streams repeated.
    The two standalone every-width columns are left out on purpose: the period's first 200 vectors are such a column (every width 0..32, with exceptions), and
    a thousand rowgroups of each further column would only repeat it."""
    from alp_amd import capi
    period = ENCODE_COLUMNS["between_rd_and_mixed"]()[: 400 * 1024]
    reps = 262
    want = of32.encode_column(period)
    assert set(range(33)) <= set(want["bw"][want["scheme"] == 2].tolist()) and (want["scheme"] == 1).any()
    w_rg, w_vec, w_packed, w_exc = layout.compact(want, 4)
    x = torch.from_numpy(period).to(DEV).repeat(reps).contiguous()
    n = 400 * reps
    assert n // 100 >= 1024
    ctx.set_option(capi.OPT_ENCODE_ASYNC_INIT, async_mode)
    try:
        col = capi.DeviceColumn(n, 0, dtype="f32")
        col.rowgroups.fill_(0x5A)
        col.vectors.fill_(0x5A)
        ctx.encode(x, col)
        ctx.synchronize()
        pb, eb, ov = ctx.column_totals(col)
    finally:
        ctx.set_option(capi.OPT_ENCODE_ASYNC_INIT, 1)
    assert ov == 0 and pb == reps * w_packed.size and eb == reps * w_exc.size
    rg = col.rowgroups.cpu().numpy().view(capi.ROWGROUP_DTYPE)[: n // 100]
    assert np.array_equal(rg.view(np.uint8), np.tile(w_rg, reps).view(np.uint8)), "rowgroup states"
    vec = col.vectors.cpu().numpy().view(capi.VECTOR_DTYPE)[:n]
    tv = np.tile(w_vec, reps)
    rep = np.repeat(np.arange(reps, dtype=np.uint64), 400)
    tv["packed_off"] += rep * np.uint64(w_packed.size)
    tv["exc_off"] += rep * np.uint64(w_exc.size)
    assert np.array_equal(vec.view(np.uint8), tv.view(np.uint8)), "descriptors"
    assert bool((col.packed[:pb].view(reps, -1) == torch.from_numpy(w_packed).to(DEV)).all()), "packed stream"
    assert bool((col.exc[:eb].view(reps, -1) == torch.from_numpy(w_exc).to(DEV)).all()), "exception stream"
    out = ctx.decode(col)
    ctx.synchronize()
    assert torch.equal(out.view(torch.int32), x.view(torch.int32))


# =====================================================================================================================================================
# 2. hand-built vectors through every decode shape
# =====================================================================================================================================================
@pytest.mark.parametrize("shape", STAGED_AND_DIRECT + STREAMED)
def test_hand_built_rows_in_every_launch_shape(ctx, rows, shape):
    with forced_shape(ctx, shape):
        got = decode_bits(ctx, rows.col)
    assert np.array_equal(got, rows.bits), f"shape {shape}: {describe_bad_rows(rows.enc, got, rows.bits)}"


@pytest.mark.parametrize("shape", [0, 2, 8, 19, 27, 29])  # staged, wave-direct, streamed with D = 1 (19), D = 2 (27), D = 4 (29)
def test_hand_built_rows_with_records_out_of_vector_order(ctx, rows, shape):
    from alp_amd import capi
    enc = rows.enc
    n = enc["scheme"].size
    order = np.random.default_rng(31).permutation(n)
    rg, in_order, _, _ = layout.compact(enc, 4)
    _, placed, packed, exc = layout.compact(fr.take_vectors(enc, order), 4)  # placement i holds the records of vector order[i]
    vec = in_order.copy()
    vec["packed_off"][order] = placed["packed_off"]
    vec["exc_off"][order] = placed["exc_off"]
    for k in ("bw", "lbw", "exc_cnt", "base", "e", "f", "scheme"):
        assert np.array_equal(vec[k][order], placed[k])
    assert (np.diff(vec["packed_off"].astype(np.int64)) < 0).any()
    col = capi.DeviceColumn.from_host(rg, vec, packed, exc, dtype="f32")
    assert ctx.column_validate(col) is None
    with forced_shape(ctx, shape):
        got = decode_bits(ctx, col)
    assert np.array_equal(got, rows.bits), f"shape {shape}, shuffled records: {describe_bad_rows(enc, got, rows.bits)}"


@pytest.mark.parametrize("shape", [0, 2, 8] + STREAMED)
def test_chunks_that_straddle_the_arena(ctx, arena, shape):
    """runs of vectors that fill a streamed shape's arena to within 8 bytes (copied flat), overflow it by 8 (copied vector by vector, the last decoded from
    HBM directly), once as narrow vectors with large exception records and once as wide ones without; one run's records start 8 modulo 16"""
    with forced_shape(ctx, shape):
        got = decode_bits(ctx, arena.col)
    if not np.array_equal(got, arena.bits):
        bad = np.nonzero((got.reshape(-1, 1024) != arena.bits.reshape(-1, 1024)).any(axis=1))[0]
        runs = [(s, c, a, kind, over) for s, c, a, kind, over in arena.where if ((bad >= s) & (bad < s + 16)).any()]
        pytest.fail(f"shape {shape}: {describe_bad_rows(arena.enc, got, arena.bits)}; runs hit (start, chunk, arena, kind, over): {runs[:6]}; skewed run at {arena.skewed}")


def tiled(enc, k):
    """the encoding's column repeated k times in HBM (tests/test_select_gpu.py: tiled_column, from an oracle-layout encoding instead of a GPU encode)"""
    from alp_amd import capi
    rg, vec, packed, exc = layout.compact(enc, 4)
    tv = np.tile(vec, k)
    rep = np.repeat(np.arange(k, dtype=np.uint64), vec.size)
    tv["packed_off"] += rep * np.uint64(packed.size)
    tv["exc_off"] += rep * np.uint64(exc.size)
    return capi.DeviceColumn.from_host(np.tile(rg, k), tv, np.tile(packed, k), np.tile(exc, k), dtype="f32")


RULE_BLOCKS = {**{f"width_{bw}": (lambda bw=bw: fr.uniform_block(bw), 27 if 2 <= bw <= 8 else None) for bw in range(1, 10)},
               "width_3_with_20_exceptions": (lambda: fr.uniform_block(3, exc_cnt=20), None),
               "mostly_narrow_with_32_bit_runs": (lambda: fr.mixed_width_block(), 27)}


@pytest.mark.parametrize("name", list(RULE_BLOCKS))
def test_the_rules_own_choice_on_long_columns(ctx, of32, name):
    """no option set: a long exception-free column of 2..8 packed bits is streamed (shape 27, decode_policy.hpp: policy_stream_f32), one of 1 or 9 bits or one
    with exceptions is not; either way every tile of the column decodes to the oracle's decode of the block"""
    make, streamed = RULE_BLOCKS[name]
    enc = make()
    n_block = enc["scheme"].size
    k = (32768 + n_block - 1) // n_block
    col = tiled(enc, k)
    assert col.n_vectors >= 32768
    shape = ctx.decode_vectors_per_wg(col)
    if streamed is None:
        assert shape < 16, f"{name}: the rule must not stream this column (shape {shape})"
    else:
        assert shape == streamed, f"{name}: the rule chose shape {shape}"
    want = torch.from_numpy(of32.decode_column(enc)).to(DEV).view(torch.int32)
    out = ctx.decode(col)
    ctx.synchronize()
    same = (out.view(torch.int32).view(k, -1) == want).view(k, n_block, 1024).all(dim=2)
    if not bool(same.all()):
        tile, v = [int(t) for t in torch.nonzero(~same)[0]]
        got = out.view(torch.int32).view(k, -1)[tile].cpu().numpy().view(np.uint32)
        pytest.fail(f"{name} (shape {shape}): {int((~same).sum())} vectors differ, first in tile {tile}; within it {describe_bad_rows(enc, got, want.cpu().numpy().view(np.uint32))}")


# =====================================================================================================================================================
# 3. the other float read paths on the same columns
# =====================================================================================================================================================
def same_sums(got, want):
    return (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))


@pytest.fixture(scope="module")
def sums(rows, generated):
    """host_sums_f32 (the documented order) of the oracle's decode, once per module"""
    return {id(b): host_sums_f32(b.want.reshape(-1, 1024), b.enc) for b in (rows, generated)}


@pytest.mark.parametrize("which", ["rows", "generated"])
def test_decode_sum_of_every_width(ctx, rows, generated, sums, kernel_f32, which):
    b = rows if which == "rows" else generated
    if which == "rows":  # the branch past the 256-entry stage of exception values: ALP vectors with 257 and 1024 exceptions
        alp = b.enc["scheme"] == 2
        assert ((b.enc["exc_cnt"] == 257) & alp).any() and ((b.enc["exc_cnt"] == 1024) & alp).any()
    want = sums[id(b)]
    got = ctx.decode_sum(b.col)
    ctx.synchronize()
    got = got.cpu().numpy()
    same = same_sums(got, want)
    assert np.isfinite(want).sum() * 2 >= want.size, "at least half of the sums say something"
    bad = np.nonzero(~same)[0]
    assert same.all(), (f"{which} {kernel_f32}: {bad.size} sums differ; (vector, bw, f, e, base, exc_cnt, scheme): "
                        f"{[(int(v), int(b.enc['bw'][v]), int(b.enc['f'][v]), int(b.enc['e'][v]), int(b.enc['base'][v]), int(b.enc['exc_cnt'][v]), int(b.enc['scheme'][v])) for v in bad[:6]]} "
                        f"got {got[bad[:3]]} want {want[bad[:3]]}")


def some_bounds(want):
    """(lo, hi) pairs as np.float32: quantiles of the finite values, a point, zero, everything, nothing, and midpoints between two adjacent distinct values
    (bounds that are no value of the column), rounded to float"""
    s = np.unique(want[np.isfinite(want)])
    q = lambda f: s[min(s.size - 1, int(f * s.size))]
    mid = lambda f: np.float32((np.float64(q(f)) + np.float64(s[min(s.size - 1, int(f * s.size) + 1)])) / 2.0)
    inf = np.float32(np.inf)
    return [(q(0.25), q(0.75)), (q(0.5), q(0.5)), (np.float32(0.0), np.float32(0.0)), (-inf, inf), (np.float32(1.0), np.float32(-1.0)), (s[-1], s[-1]),
            (mid(0.3), q(0.7)), (q(0.3), mid(0.7)), (mid(0.45), mid(0.55)), (np.float32(-1000.0), np.float32(1000.0))]


@pytest.mark.parametrize("which", ["rows", "generated"])
def test_decode_count_range_of_every_width(ctx, rows, generated, kernel_f32, which):
    b = rows if which == "rows" else generated
    v = b.want.reshape(-1, 1024)
    partial = False
    for lo32, hi32 in some_bounds(b.want):
        got = ctx.decode_count_range(b.col, float(lo32), float(hi32))
        ctx.synchronize()
        with np.errstate(invalid="ignore"):
            want = ((v >= lo32) & (v <= hi32)).sum(axis=1)
        got = got.cpu().numpy().astype(np.int64)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f"{which} {kernel_f32} [{lo32!r}, {hi32!r}]: {bad.size} counts differ; (vector, bw, f, base, exc_cnt, got, want): "
                               f"{[(int(i), int(b.enc['bw'][i]), int(b.enc['f'][i]), int(b.enc['base'][i]), int(b.enc['exc_cnt'][i]), int(got[i]), int(want[i])) for i in bad[:6]]}")
        partial = partial or 0 < int(want.sum()) < v.size
    assert partial


@pytest.mark.parametrize("which", ["rows", "generated", "arena"])
def test_zone_maps_of_every_width(ctx, rows, generated, arena, which):
    """zone_map / column_minmax against tests/test_zone_gpu.py's key reduction of the ORACLE's decode"""
    b = {"rows": rows, "generated": generated, "arena": arena}[which]
    tz.check_zones(ctx, b.col, b.x, which)


@pytest.mark.parametrize("which", ["rows", "generated"])
def test_gather_and_slices_of_every_width(ctx, rows, generated, which):
    b = rows if which == "rows" else generated
    n = b.want.size
    rng = np.random.default_rng(17)
    ref = torch.from_numpy(b.bits.view(np.int32)).to(DEV)
    widths = [int(w) for w in (0, 1, 31, 32)]
    alp = b.enc["scheme"] == 2
    picked = [int(np.nonzero(alp & (b.enc["bw"] == w))[0][j]) for w in widths for j in (0, -1)]  # first and last vector of each of these widths
    sets = {"random": rng.integers(0, n, 200_000), "duplicates": rng.integers(0, n, 64)[rng.integers(0, 64, 100_000)], "permutation of everything": rng.permutation(n),
            **{f"every index of vector {v}": np.arange(v * 1024, v * 1024 + 1024) for v in picked},
            **{f"vector {v} backwards, twice": np.concatenate([np.arange(v * 1024 + 1023, v * 1024 - 1, -1)] * 2) for v in picked[:2]}}
    for name, idx_np in sets.items():
        idx = torch.from_numpy(np.ascontiguousarray(idx_np, dtype=np.int64)).to(DEV)
        got = ctx.gather(b.col, idx).view(torch.int32)
        assert torch.equal(got, ref[idx]), f"{which}: gather of {name} differs from the oracle's decode"
    for v in picked:  # slices that start and end inside a vector of width 0, 1, 31 or 32
        for first, m in ((v * 1024 + 5, 1000), (v * 1024 + 1023, 1), (v * 1024 + 511, 2), (max(0, v * 1024 - 300), 700), (v * 1024 + 700, min(2000, n - v * 1024 - 700)), (v * 1024, 1024)):
            got = ctx.decode_slice(b.col, first, m).view(torch.int32)
            assert torch.equal(got, ref[first:first + m]), f"{which}: slice ({first}, {m}) at vector {v} (width {int(b.enc['bw'][v])}) differs from the oracle's decode"
    got = ctx.decode_slice(b.col, 1, n - 2).view(torch.int32)
    assert torch.equal(got, ref[1:n - 1]), f"{which}: the slice of nearly everything"


@pytest.mark.parametrize("which", ["rows", "generated", "arena"])
def test_selection_of_every_width_plain_and_zoned(ctx, rows, generated, arena, which):
    """tests/test_select_gpu.py's battery (indices, values, counts, the tie to decode_count_range) and tests/test_zone_gpu.py's zoned form of it, plus bounds
    that are no values of the column; `x` is the oracle's decode, so indices and values are checked against nonzero / fancy indexing of it"""
    b = {"rows": rows, "generated": generated, "arena": arena}[which]
    ts.check_battery(ctx, b.col, b.x, which, specials=True)
    zones = tz.check_zones(ctx, b.col, b.x, which)
    preds = ts.battery(b.x, True) + [(f"off-value bounds {i}", float(lo), float(hi)) for i, (lo, hi) in enumerate(some_bounds(b.want)[6:])]
    hit = 0
    for name, lo, hi in preds:
        hit += tz.check_zoned_select(ctx, b.col, b.x, zones, lo, hi, what=f"{which}/{name}")
    n = b.want.size
    tz.check_zoned_select(ctx, b.col, b.x, zones, *[float(t) for t in some_bounds(b.want)[6]], first=1024 * 3 + 7, n=n - 1024 * 9, what=f"{which}/window")
    assert hit > 0
