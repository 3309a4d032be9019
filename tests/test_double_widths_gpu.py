"""GPU: every double (64-bit) read path on the hand-built vectors of every packed width — the sibling of sections 2 and 3 of tests/test_float_widths_gpu.py for the
kernels the project is measured by: the store decode k_decode_column in each of its five instances, the three sink kernels behind decode_sum / decode_count_range /
column_sum (k_sink_direct, k_consume_column, the four-wavefront k_decode_column), zone_map, gather and decode_slice, and select_range plain and zoned.

The columns are double_rows.py's alp_rows (widths 0..64 under factors across the table, bases on the shortcut's bounds and at both ends of int64), arm_rows (every
(arithmetic arm, exception arm) pair of decode_kernels.hip and consume_kernels.hip at the widths where an arm begins or ends) and rd_rows (every ALP_RD cut 48..63 with
a dictionary of its own): in vector order (`rows`), the ALP part alone (`alp_only`: the rule launches the 256-entry-stage instance for it), with narrow and wide vectors
side by side (`mixed`) and with the records permuted in the streams (`shuffled`).  tests/test_double_widths_cpu.py checks, without a GPU, that these inputs are what they
claim to be, and states the kernels' per-vector rules the coverage guard at the end of this file counts by.

EVERY expectation is the oracle's decode of the hand-built encoding (oracle/pyoracle.py: Oracle.decode_column), directly or through the host replicas of the
documented summation orders and numpy's IEEE comparisons.  No result of a GPU call is the expectation of another; everything compares on integer views (-0.0, NaN
payloads), sums also as "both NaN"."""
import contextlib

import numpy as np
import pytest
import torch

import double_rows as dr
import float_rows as fr
import layout
import test_double_widths_cpu as tc
import test_select_gpu as ts
import test_zone_gpu as tz
from test_decode_sum_gpu import host_column_total, host_sums, host_sums_pipelined, shape  # noqa: F401  (shape: the fixture over the three sink kernels)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
EDGE_WIDTHS = (0, 1, 28, 29, 32, 33, 50, 51, 63, 64)
SHAPES = [(1, "<1,nt>"), (2, "<2,nt>"), (4, "<2,nt>"), (8, "<1,nt>")]  # ALPGPU_OPT_DECODE_VECTORS_PER_WG: double columns run 4 as 2 and 8 as 1
PADS = (0, 3, 6, 11, 14)                                               # the residency pads the rule knows (decode_policy.hpp), forced


# =====================================================================================================================================================
# the columns
# =====================================================================================================================================================
class Built:
    """a hand-built encoding, the oracle's decode of it, and the column in HBM; source[i]: the row of `rows` that vector i is"""

    def __init__(self, ctx, oracle, name, enc, source=None, shuffle_seed=None):
        from alp_amd import capi
        self.name, self.enc = name, enc
        self.nv = enc["scheme"].size
        self.source = np.arange(self.nv) if source is None else source
        self.want = oracle.decode_column(enc)
        assert self.want.dtype == np.float64 and self.want.size == 1024 * self.nv
        self.bits = self.want.view(np.uint64)
        self.values = self.want.reshape(self.nv, 1024)
        self.alp = enc["scheme"] == fr.SCHEME_ALP
        rg, vec, packed, exc = layout.compact(enc)
        if shuffle_seed is not None:
            # the same vectors, their records somewhere else in the streams (test_float_widths_gpu.py: test_hand_built_rows_with_records_out_of_vector_order)
            order = np.random.default_rng(shuffle_seed).permutation(self.nv)
            _, placed, packed, exc = layout.compact(fr.take_vectors(enc, order))  # placement i holds the records of vector order[i]
            vec = vec.copy()
            vec["packed_off"][order] = placed["packed_off"]
            vec["exc_off"][order] = placed["exc_off"]
            for k in ("bw", "lbw", "exc_cnt", "base", "e", "f", "scheme"):
                assert np.array_equal(vec[k][order], placed[k])
            assert (np.diff(vec["packed_off"].astype(np.int64)) < 0).any() and (np.diff(vec["exc_off"].astype(np.int64)) < 0).any()
        self.col = capi.DeviceColumn.from_host(rg, vec, packed, exc)
        assert ctx.column_validate(self.col) is None, "the hand-built descriptors are ones the kernels are specified for"
        self.x = torch.from_numpy(self.want).to(DEV)
        self.memo = {}

    def once(self, key, fn):
        """an expectation computed once from the oracle's decode and left unchanged"""
        if key not in self.memo:
            self.memo[key] = fn()
        return self.memo[key]


@pytest.fixture(scope="module")
def encodings():
    return tc.column_encodings()


@pytest.fixture(scope="module")
def rows(ctx, oracle, encodings):
    """[alp_rows, arm_rows, rd_rows] in vector order"""
    return Built(ctx, oracle, "rows", encodings[0]["rows"])


@pytest.fixture(scope="module")
def alp_only(ctx, oracle, encodings):
    """[alp_rows, arm_rows]: exception-heavy ALP vectors and no ALP_RD rowgroup"""
    return Built(ctx, oracle, "alp_only", encodings[0]["alp_only"])


@pytest.fixture(scope="module")
def mixed(ctx, oracle, encodings):
    """interleave(rows): narrow and wide vectors side by side, ALP_RD rowgroups between ALP rowgroups"""
    return Built(ctx, oracle, "mixed", encodings[0]["mixed"], source=encodings[1])


@pytest.fixture(scope="module")
def shuffled(ctx, oracle, encodings):
    """`rows` with its records permuted in the streams: descriptor offsets not ascending"""
    return Built(ctx, oracle, "shuffled", encodings[0]["rows"], shuffle_seed=31)


@pytest.fixture
def columns(rows, mixed, shuffled):
    return {"rows": rows, "mixed": mixed, "shuffled": shuffled}


# ---- what a failure prints ------------------------------------------------------------------------------------------------------------------------
def describe(b, bad_vectors, first_bad=None, limit=6):
    """(vector, source row, scheme, bw, lbw, f, e, base, exc_cnt, first bad value index) of the first vectors that differ"""
    e = b.enc
    found = [(int(v), int(b.source[v]), "ALP" if e["scheme"][v] == fr.SCHEME_ALP else "ALP_RD", int(e["bw"][v]), int(e["lbw"][v]), int(e["f"][v]), int(e["e"][v]), int(e["base"][v]),
              int(e["exc_cnt"][v]), None if first_bad is None else int(first_bad(int(v)))) for v in bad_vectors[:limit]]
    return f"{b.name}: {len(bad_vectors)} vectors differ; (vector, source row, scheme, bw, lbw, f, e, base, exc_cnt, first bad value index): {found}"


def assert_decoded(b, out, what):
    """out: the device tensor a store decode wrote"""
    if not torch.equal(out.view(torch.int64), b.x.view(torch.int64)):
        got = out.cpu().numpy().view(np.uint64).reshape(b.nv, 1024)
        diff = got != b.bits.reshape(b.nv, 1024)
        pytest.fail(f"{what}: " + describe(b, np.nonzero(diff.any(axis=1))[0], lambda v: np.nonzero(diff[v])[0][0]))


def assert_values(b, got, idx_np, what):
    """got: device values that must be the oracle's at the value indices idx_np"""
    g = got.cpu().numpy().view(np.uint64)
    same = g == b.bits[idx_np]
    if not same.all():
        first = np.asarray(idx_np)[np.nonzero(~same)[0]]
        vectors = np.unique(first >> 10)
        pytest.fail(f"{what}: " + describe(b, vectors, lambda v: first[first >> 10 == v][0] & 1023))


def assert_per_vector(b, same, what, extra=""):
    same = np.asarray(same)
    if not same.all():
        pytest.fail(f"{what}: {describe(b, np.nonzero(~same)[0])} {extra}")


def same_sums(got, want):
    return (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))


@contextlib.contextmanager
def options(ctx, **values):
    """decode options set for one block: vpw (ALPGPU_OPT_DECODE_VECTORS_PER_WG), plain (.._PLAIN_STORES), pad (.._RESIDENCY_PAD)"""
    from alp_amd import capi
    ids = {"vpw": (capi.OPT_DECODE_VECTORS_PER_WG, 0), "plain": (capi.OPT_DECODE_PLAIN_STORES, 0), "pad": (capi.OPT_DECODE_RESIDENCY_PAD, -1)}
    try:
        for k, v in values.items():
            ctx.set_option(ids[k][0], v)
        yield
    finally:
        for k in values:
            ctx.set_option(*ids[k])


def decode(ctx, b):
    out = ctx.decode(b.col)
    ctx.synchronize()
    return out


# =====================================================================================================================================================
# the store decode: forced launch shapes
# =====================================================================================================================================================
@pytest.mark.parametrize("plain", [0, 1], ids=["nt_stores", "plain_stores"])
@pytest.mark.parametrize("vpw", [s for s, _ in SHAPES])
@pytest.mark.parametrize("which", ["rows", "mixed", "shuffled"])
def test_store_decode_in_every_forced_shape(ctx, columns, which, vpw, plain):
    b = columns[which]
    with options(ctx, vpw=vpw, plain=plain):
        assert ctx.decode_vectors_per_wg(b.col) == (2 if vpw in (2, 4) else 1)
        plan = ctx.decode_plan(b.col)
        assert plan is not None and not plan["many_exc"], "a forced shape never takes the 256-entry-stage instance"
        out = decode(ctx, b)
    assert_decoded(b, out, f"{vpw} vectors per workgroup, {'plain' if plain else 'non-temporal'} stores")


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("which", ["rows", "mixed", "shuffled"])
def test_store_decode_under_every_residency_pad(ctx, columns, which, pad):
    b = columns[which]
    with options(ctx, pad=pad):
        plan = ctx.decode_plan(b.col)
        assert plan is not None and plan["pad_kib"] == pad and plan["vectors_per_wg"] == 1
        out = decode(ctx, b)
    assert_decoded(b, out, f"the rule's shape under a residency pad of {pad} KiB")


# =====================================================================================================================================================
# the store decode: the rule's own choice
# =====================================================================================================================================================
def test_the_rule_decodes_the_rows_as_an_alp_rd_column(ctx, rows, mixed):
    """decode_policy.hpp, policy_shape_f64: more than half of the vectors belong to ALP_RD rowgroups -> one vector per workgroup, seven workgroups per CU (an 11 KiB pad),
    and never the 256-entry stage"""
    for b in (rows, mixed):
        assert 2 * int((~b.alp).sum()) > b.nv
        plan = ctx.decode_plan(b.col)
        assert plan is not None and (plan["vectors_per_wg"], plan["many_exc"], plan["pad_kib"]) == (1, False, 11), (b.name, plan)
        assert plan["rd_rowgroups_hint"] == 1 + int((~b.alp).sum()) // 100
        assert_decoded(b, decode(ctx, b), "no option set")


def test_the_rule_decodes_the_alp_column_with_the_256_entry_stage(ctx, alp_only):
    """decode_policy.hpp: exc_bytes >= 10 * 128 * n_vectors, more than 22 packed bits per value, no ALP_RD -> DecodeShape::many_exc: k_decode_column<1, true, kSinkStore,
    DecodeLdsManyExc> on 255 / 256 / 257 / 1024 exceptions at every arithmetic arm.  (tests/test_double_widths_cpu.py holds the two numbers.)"""
    b = alp_only
    plan = ctx.decode_plan(b.col)
    assert plan is not None and plan["many_exc"] and plan["vectors_per_wg"] == 1, plan
    assert plan["exc_bytes"] >= 1280 * b.nv and plan["packed_bytes"] > 22 * 128 * b.nv and plan["rd_rowgroups_hint"] == 1
    for c in (255, 256, 257, 1024):
        assert (b.enc["exc_cnt"] == c).any()
    assert_decoded(b, decode(ctx, b), "no option set: the 256-entry exception stage")
    with options(ctx, plain=1):  # ... which has no instance with plain stores
        assert not ctx.decode_plan(b.col)["many_exc"]
        assert_decoded(b, decode(ctx, b), "plain stores")


def test_the_256_entry_stage_on_every_alp_rd_cut(ctx, rows):
    """the same instance over the ALP_RD rowgroups (a stage of 1024 left parts): `rows` under a hint that says it has no ALP_RD rowgroup, as a column whose rowgroups
    were never counted has (tests/test_decode_planning_gpu.py: the hints steer the launch, never the bytes)"""
    b = rows
    c = b.col.c
    truth = int(c.alp_rd_rowgroups_hint)
    try:
        c.alp_rd_rowgroups_hint = 1
        plan = ctx.decode_plan(b.col)
        assert plan is not None and plan["many_exc"] and plan["vectors_per_wg"] == 1, plan
        out = decode(ctx, b)
    finally:
        c.alp_rd_rowgroups_hint = truth
    assert_decoded(b, out, "the 256-entry exception stage on ALP_RD rowgroups")
    assert not ctx.decode_plan(b.col)["many_exc"]


def test_the_alp_column_without_hints(ctx, alp_only):
    """size hints zero and fewer than 65 536 vectors: no device-side plan, the shape a column without hints always got (one vector per workgroup, no pad, the
    128-entry stage)"""
    b = alp_only
    c = b.col.c
    truth = (int(c.packed_bytes_hint), int(c.exc_bytes_hint), int(c.alp_rd_rowgroups_hint))
    assert b.nv < 65536
    try:
        c.packed_bytes_hint = c.exc_bytes_hint = c.alp_rd_rowgroups_hint = 0
        ctx.forget(b.col)
        plan = ctx.decode_plan(b.col)
        assert plan is not None and (plan["vectors_per_wg"], plan["many_exc"], plan["pad_kib"], plan["packed_bytes"], plan["exc_bytes"]) == (1, False, 0, 0, 0), plan
        out = decode(ctx, b)
    finally:
        c.packed_bytes_hint, c.exc_bytes_hint, c.alp_rd_rowgroups_hint = truth
        ctx.forget(b.col)
    assert_decoded(b, out, "no hints")
    assert ctx.decode_plan(b.col)["many_exc"]


# =====================================================================================================================================================
# SUM, the column total, COUNT: the three sink kernels (the `shape` fixture)
# =====================================================================================================================================================
@pytest.mark.parametrize("which", ["rows", "mixed"])
def test_decode_sum_and_column_sum(ctx, columns, shape, which, request):
    b = columns[which]
    kernel = request.node.callspec.params["shape"]
    want = b.once(("sums", shape.__name__), lambda: shape(b.values))
    assert np.isfinite(want).sum() * 2 >= want.size, "at least half of the sums say something"
    got = ctx.decode_sum(b.col)
    total = ctx.column_sum(b.col)
    ctx.synchronize()
    got = got.cpu().numpy()
    same = same_sums(got, want)
    bad = np.nonzero(~same)[0]
    assert_per_vector(b, same, f"decode_sum, {kernel} kernel, in the order of {shape.__name__}", f"got {got[bad[:3]]} want {want[bad[:3]]}")
    want_total = np.float64(host_column_total(want))
    got_total = total.cpu().numpy()
    assert same_sums(got_total, np.array([want_total])).all(), f"{which}: column_sum {got_total} != {want_total!r} (the documented tree over the per-vector sums)"


def some_bounds(want):
    """tests/test_float_widths_gpu.py's some_bounds in float64: quantiles of the finite values, a point, zero, everything, the empty range, the maximum, and midpoints
    between two adjacent distinct values (bounds that are no value of the column)"""
    s = np.unique(want[np.isfinite(want)])
    q = lambda f: s[min(s.size - 1, int(f * s.size))]

    def mid(f):
        a, c = q(f), s[min(s.size - 1, int(f * s.size) + 1)]
        m = a / 2.0 + c / 2.0
        return m if a < m < c else a  # (adjacent doubles have no midpoint)

    return [(q(0.25), q(0.75)), (q(0.5), q(0.5)), (0.0, 0.0), (-INF, INF), (1.0, -1.0), (s[-1], s[-1]),
            (mid(0.3), q(0.7)), (q(0.3), mid(0.7)), (mid(0.45), mid(0.55)), (-1000.0, 1000.0)]


def bounds_of(b):
    def make():
        bounds = some_bounds(b.want)
        off = np.array([bounds[6][0], bounds[7][1], bounds[8][0], bounds[8][1]])
        assert not np.isin(off, b.want).all(), "some bound is no value of the column"
        # ... and a band for each pair of edge widths, from the values of their vectors with a base of 0 or -1: quantiles of the whole column lie far from values
        # of a few dozen bits, and a digit that lost its top bit would cross none of them
        bw, base = b.enc["bw"].astype(int), b.enc["base"]
        for w in (28, 32, 50, 56, 63):
            v = b.values[b.alp & ((bw == w) | (bw == w + 1)) & ((base == 0) | (base == -1))]
            s = np.sort(v[np.isfinite(v)])
            assert s.size >= 2048, w
            bounds.append((s[s.size // 4], s[3 * s.size // 4]))
        return bounds
    return b.once("bounds", make)


@pytest.mark.parametrize("which", ["rows", "mixed"])
def test_decode_count_range(ctx, columns, shape, which, request):
    b = columns[which]
    kernel = request.node.callspec.params["shape"]
    partial = False
    for i, (lo, hi) in enumerate(bounds_of(b)):
        lo, hi = float(lo), float(hi)

        def count():
            with np.errstate(invalid="ignore"):
                return ((b.values >= lo) & (b.values <= hi)).sum(axis=1)
        want = b.once(("count", i), count)
        got = ctx.decode_count_range(b.col, lo, hi)
        ctx.synchronize()
        got = got.cpu().numpy().astype(np.int64)
        bad = np.nonzero(got != want)[0]
        assert_per_vector(b, got == want, f"decode_count_range [{lo!r}, {hi!r}], {kernel} kernel", f"(got, want): {[(int(got[v]), int(want[v])) for v in bad[:6]]}")
        partial = partial or 0 < int(want.sum()) < b.want.size
    assert partial, "some bound selects part of the column"


# =====================================================================================================================================================
# zone maps
# =====================================================================================================================================================
@pytest.mark.parametrize("which", ["rows", "mixed", "shuffled"])
def test_zone_maps(ctx, columns, which):
    """zone_map / column_minmax against the key reduction of the ORACLE's decode (tests/test_zone_gpu.py: check_zones), and byte for byte zone_map_of_values of it"""
    b = columns[which]
    try:
        z = tz.check_zones(ctx, b.col, b.x, which, raw=b.x)
    except AssertionError:
        z = ctx.zone_map(b.col)
        want = tz.expected_zones(b.x)
        bad = torch.nonzero((tz.ibits(z) != want).any(dim=1)).reshape(-1).cpu().numpy()
        print(describe(b, bad))
        raise
    assert z.cpu().numpy().tobytes() == ctx.zone_map_of_values(b.x).cpu().numpy().tobytes()
    assert bool(torch.isinf(z).any()), "some vector holds an infinity, or nothing but NaNs"


# =====================================================================================================================================================
# gather and slices
# =====================================================================================================================================================
def picked_vectors(b):
    """the first and last vector of each edge width and of three ALP_RD cuts"""
    e = b.enc
    cuts = dr.rd_cuts()
    picks = [np.nonzero(b.alp & (e["bw"] == w))[0] for w in EDGE_WIDTHS]
    picks += [np.nonzero(~b.alp & (e["bw"] == rbw) & (e["lbw"] == lbw))[0] for rbw, lbw in (cuts[0], cuts[len(cuts) // 2], cuts[-1])]
    return [int(p[j]) for p in picks for j in (0, -1)]


@pytest.mark.parametrize("which", ["rows", "shuffled"])
def test_gather_and_slices(ctx, columns, which):
    b = columns[which]
    n = b.want.size
    rng = np.random.default_rng(17)
    picked = picked_vectors(b)
    assert len(picked) == 26 and len(set(picked)) == 26
    sets = {"random": rng.integers(0, n, 200_000), "duplicates": rng.integers(0, n, 64)[rng.integers(0, 64, 100_000)], "permutation of everything": rng.permutation(n),
            **{f"every index of vector {v}": np.arange(v * 1024, v * 1024 + 1024) for v in picked},
            **{f"vector {v} backwards, twice": np.concatenate([np.arange(v * 1024 + 1023, v * 1024 - 1, -1)] * 2) for v in picked}}
    for name, idx_np in sets.items():
        idx_np = np.ascontiguousarray(idx_np, dtype=np.int64)
        got = ctx.gather(b.col, torch.from_numpy(idx_np).to(DEV))
        assert_values(b, got, idx_np, f"gather of {name}")
    for v in picked:  # slices that start and end inside these vectors
        for first, m in ((v * 1024 + 5, 1000), (v * 1024 + 1023, 1), (v * 1024 + 511, 2), (max(0, v * 1024 - 300), 700), (v * 1024 + 700, min(2000, n - v * 1024 - 700)), (v * 1024, 1024)):
            got = ctx.decode_slice(b.col, first, m)
            assert_values(b, got, np.arange(first, first + m), f"slice ({first}, {m}) at vector {v}")
    assert_values(b, ctx.decode_slice(b.col, 1, n - 2), np.arange(1, n - 1), "the slice of nearly everything")


# =====================================================================================================================================================
# selection, plain and zoned
# =====================================================================================================================================================
def zoned_predicates(b):
    return ts.battery(b.x, True) + [(f"off-value bounds {i}", float(lo), float(hi)) for i, (lo, hi) in enumerate(bounds_of(b)[6:])]


def skipped_by_record(b, lo, hi):
    """vectors whose record {min, max} (of the oracle's decode) lies outside [lo, hi]: what the zoned selection does not decode"""
    zones = b.once("zones", lambda: tz.fbits(tz.expected_zones(b.x)).cpu().numpy())
    with np.errstate(invalid="ignore"):
        return ~((zones[:, 1] >= lo) & (zones[:, 0] <= hi))


@pytest.mark.parametrize("which", ["rows", "mixed", "shuffled"])
def test_selection_plain_and_zoned(ctx, columns, which):
    """tests/test_select_gpu.py's battery (indices, values, counts, the tie to decode_count_range) and tests/test_zone_gpu.py's zoned form of it with the column's own
    zone map, plus bounds that are no values of the column and a window that starts and ends inside vectors; `x` is the oracle's decode, so indices and values are checked
    against nonzero / fancy indexing of it"""
    b = columns[which]
    ts.check_battery(ctx, b.col, b.x, which, specials=True)
    zones = tz.check_zones(ctx, b.col, b.x, which)
    hit, skipping = 0, 0
    for name, lo, hi in zoned_predicates(b):
        hit += tz.check_zoned_select(ctx, b.col, b.x, zones, lo, hi, what=f"{which}/{name}")
        skipped = int(skipped_by_record(b, lo, hi).sum())
        skipping += 0 < skipped < b.nv
    lo, hi = (float(t) for t in bounds_of(b)[6])
    tz.check_zoned_select(ctx, b.col, b.x, zones, lo, hi, first=1024 * 3 + 7, n=b.want.size - 1024 * 9, what=f"{which}/window")
    assert hit > 0 and skipping > 0, "some predicate skips some vectors by their records and not all"


# =====================================================================================================================================================
# the coverage guard
# =====================================================================================================================================================
STORE_CALLS = {  # instance of k_decode_column -> the columns the tests above decode with it
    "<2,nt>": ("rows", "mixed", "shuffled"), "<2,plain>": ("rows", "mixed", "shuffled"), "<1,nt>": ("rows", "mixed", "shuffled", "alp_only"),
    "<1,plain>": ("rows", "mixed", "shuffled", "alp_only"), "<1,nt,DecodeLdsManyExc>": ("alp_only", "rows")}
FAMILIES = {**{"k_decode_column" + k: v for k, v in STORE_CALLS.items()},
            "k_sink_direct (decode_sum, decode_count_range, column_sum)": ("rows", "mixed"), "k_consume_column": ("rows", "mixed"),
            "k_decode_column<2,plain,sink>": ("rows", "mixed"), "zone_map": ("rows", "mixed", "shuffled"), "gather": ("rows", "shuffled"), "decode_slice": ("rows", "shuffled"),
            "select_range": ("rows", "mixed", "shuffled")}


def test_every_family_decoded_every_width_cut_and_cell(ctx, rows, alp_only, mixed, shuffled):
    """what each family's calls above decode: a store decode, a sink, zone_map, the gather of a permutation of everything, the slice of nearly everything and the
    plain selection decode every vector of their columns; the zoned selection those its records do not skip (reported, and asserted to reach every class as well under
    the predicate `everything`)"""
    by_name = {"rows": rows, "alp_only": alp_only, "mixed": mixed, "shuffled": shuffled}
    widths, cuts = set(range(65)), set(dr.rd_cuts())
    for family, names in FAMILIES.items():
        got_w, got_c, got_cells, vectors = set(), set(), set(), 0
        for name in names:
            e, b = by_name[name].enc, by_name[name]
            got_w |= set(e["bw"][b.alp].tolist())
            got_c |= set(zip(e["bw"][~b.alp].tolist(), e["lbw"][~b.alp].tolist()))
            got_cells |= b.once("cells", lambda: tc.cells(e))
            vectors += b.nv
        print(f"coverage {family}: {vectors} vectors decoded in {len(names)} columns; ALP widths {min(got_w)}..{max(got_w)} ({len(got_w)}), ALP_RD cuts {len(got_c)} of {len(cuts)}, "
              f"cells {len(got_cells & tc.REQUIRED_CELLS)} of {len(tc.REQUIRED_CELLS)} required ({len(got_cells)} in all)")
        assert got_w == widths and got_c == cuts and tc.REQUIRED_CELLS <= got_cells, (family, sorted(tc.REQUIRED_CELLS - got_cells))
    for b in (rows, mixed, shuffled):  # the zoned selection: what the records leave to decode, per predicate
        reached, fewest = np.zeros(b.nv, bool), b.nv
        for name, lo, hi in zoned_predicates(b):
            decoded = ~skipped_by_record(b, lo, hi)
            reached |= decoded
            fewest = min(fewest, int(decoded.sum()) or fewest)
        got = tc.cells(b.enc, reached)
        print(f"coverage select_range_zoned {b.name}: {int(reached.sum())} of {b.nv} vectors decoded under some predicate, as few as {fewest} (and not none) under one; "
              f"cells {len(got & tc.REQUIRED_CELLS)} of {len(tc.REQUIRED_CELLS)} required")
        assert reached.all() and tc.REQUIRED_CELLS <= got
