"""GPU: the one in-register decode of a vector (register_decode.hpp: DecodeVec / step_request / step_value) under each of its seven kernels, on the
hand-built vectors of every packed width — k_select's kSelMask, kSelSum and kSelTake arms (select_device.hpp: alpgpu_select_mask_*,
alpgpu_decode_sum_masked_*, alpgpu_decode_masked_*), k_pair (compare, dot), k_group (three tiers), k_minmax_masked, k_group_minmax (three tiers) and k_in_list
(the LDS and the global arm).  The suites of those features read columns the encoder produces from datagen; here the columns are float_rows.py (widths 0..32,
cuts 16..31) and double_rows.py (widths 0..64, cuts 48..63): every width under every factor, bases on the bounds of the conversion shortcut and at the ends
of the integer range, exception records on both sides of every lane count and stage, every ALP_RD cut with a dictionary of its own.

EVERY expectation is the oracle's decode of the hand-built encoding (oracle/pyoracle.py: Oracle / OracleF32 decode_column), fed through the host replicas
the feature suites share (host_sums_masked, host_dots_masked, host_group_sums, host_minmax_masked, host_group_minmax, host_in_mask) or through numpy's own
IEEE comparisons.  No result of a GPU call is the expectation of another; everything compares bit for bit on integer views, sums also as "both NaN".
tests/test_double_rows_cpu.py and tests/test_float_widths_cpu.py check, without a GPU, that the rows are what they claim to be."""
import numpy as np
import pytest
import torch

import double_rows as dr
import float_rows as fr
import layout
from group_replica import host_group_sums
from in_list_replica import host_in_mask, pack_bits
from minmax_replica import host_group_minmax, host_minmax_masked
from pair_replica import host_dots_masked
from test_mask_gpu import host_sums_masked, random_mask, vectors_cleared

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
PER_VECTOR = ("scheme", "e", "f", "bw", "lbw", "base", "exc_cnt", "packed", "packed_left", "exc", "pos")
PER_ROWGROUP = ("dict", "dict_size", "k", "combos")
CMPS = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal, "ne": np.not_equal}  # IEEE comparisons, as C's
GROUP_COUNTS = (1, 4, 5, 16)  # the accumulator tiers of 4, 8 and 16 groups, and the first one's two ends
PAIR_FAMILIES = ("compare_mask", "decode_dot_masked", "decode_group_sum", "decode_group_minmax")
FAMILIES = ("select_mask", "decode_sum_masked", "decode_masked", "decode_minmax_masked", "select_in_mask") + PAIR_FAMILIES


# =====================================================================================================================================================
# the columns
# =====================================================================================================================================================
def rowgroups(enc, r0, r1):
    """rowgroups [r0, r1) of an encoding, with their per-rowgroup arrays"""
    out = {k: enc[k][100 * r0:100 * r1] for k in PER_VECTOR}
    out.update({k: enc[k][r0:r1] for k in PER_ROWGROUP})
    return out


def second_column(alp, rd):
    """the rows of [alp, rd] as a second column of the same length in which every scheme pairing occurs: the first half of the ALP_RD rowgroups, the ALP
    part backwards, the remaining ALP_RD rowgroups.  Against [alp, rd]: ALP x ALP_RD, ALP x ALP, ALP_RD x ALP, ALP_RD x ALP_RD, in this order"""
    n_alp, n_rd = alp["bw"].size // 100, rd["bw"].size // 100
    k = min(n_alp, n_rd) // 2
    return fr.concat_encodings([rowgroups(rd, 0, k), fr.take_vectors(alp, np.arange(100 * n_alp)[::-1].copy()), rowgroups(rd, k, n_rd)])


class Built:
    """a hand-built encoding, the oracle's decode of it, and the column in HBM"""

    def __init__(self, ctx, oracle, enc, dtype, shuffle_seed=None):
        from alp_amd import capi
        W = 8 if dtype == "f64" else 4
        self.enc, self.dtype = enc, dtype
        self.nv = enc["scheme"].size
        self.want = oracle.decode_column(enc)
        assert self.want.dtype == (np.float64 if W == 8 else np.float32) and self.want.size == 1024 * self.nv
        self.bits = self.want.view(np.uint64 if W == 8 else np.uint32)
        self.values = self.want.reshape(self.nv, 1024)
        rg, vec, packed, exc = layout.compact(enc, W)
        if shuffle_seed is not None:
            # the same vectors, their records somewhere else in the streams (test_float_widths_gpu.py: test_hand_built_rows_with_records_out_of_vector_order)
            order = np.random.default_rng(shuffle_seed).permutation(self.nv)
            _, placed, packed, exc = layout.compact(fr.take_vectors(enc, order), W)  # placement i holds the records of vector order[i]
            vec = vec.copy()
            vec["packed_off"][order] = placed["packed_off"]
            vec["exc_off"][order] = placed["exc_off"]
            for k in ("bw", "lbw", "exc_cnt", "base", "e", "f", "scheme"):
                assert np.array_equal(vec[k][order], placed[k])
            assert (np.diff(vec["packed_off"].astype(np.int64)) < 0).any()
        self.col = capi.DeviceColumn.from_host(rg, vec, packed, exc, dtype=dtype)
        assert ctx.column_validate(self.col) is None, "the hand-built descriptors are ones the kernels are specified for"
        self.alp = enc["scheme"] == fr.SCHEME_ALP
        # value indices of every exception position, from the descriptors
        self.exc_at = np.zeros((self.nv, 1024), bool)
        for v in np.nonzero(enc["exc_cnt"])[0]:
            self.exc_at[v, enc["pos"][v, : int(enc["exc_cnt"][v])]] = True


class Columns:
    """A = [alp_rows, rd_rows], B = the same rows as second_column lays them out, S = A with its records shuffled in the streams; the bitmaps and bounds
    every test shares, and a memo of the expectations (each computed once from the oracle's decode and left unchanged)"""

    def __init__(self, ctx, dtype):
        from oracle.pyoracle import Oracle, OracleF32
        rows, oracle = (dr, Oracle()) if dtype == "f64" else (fr, OracleF32())
        alp, rd = rows.alp_rows(), rows.rd_rows()
        self.dtype, self.rows = dtype, rows
        self.value_bits = 64 if dtype == "f64" else 32
        self.A = Built(ctx, oracle, fr.concat_encodings([alp, rd]), dtype)
        self.B = Built(ctx, oracle, second_column(alp, rd), dtype)
        self.S = Built(ctx, oracle, self.A.enc, dtype, shuffle_seed=31)
        self.nv = self.A.nv
        assert self.B.nv == self.nv < 10000
        rnd = random_mask(self.nv, 51)
        self.masks = {"full": torch.full_like(rnd, -1), "random": rnd, "cleared": vectors_cleared(rnd, 3, 0)}
        self.mask_bits = {k: unpack(m.cpu().numpy(), self.nv) for k, m in self.masks.items()}
        self.memo = {}

    def once(self, key, fn):
        if key not in self.memo:
            self.memo[key] = fn()
        return self.memo[key]

    def quantile(self, b, f):
        s = self.once(("sorted", id(b)), lambda: np.sort(b.want[np.isfinite(b.want)]))
        return float(s[min(s.size - 1, int(f * s.size))])

    def predicates(self, b):
        """three closed ranges whose bounds are values of the column (exact in its type): two quantile bands and everything"""
        q = lambda f: self.quantile(b, f)
        return [(q(0.25), q(0.75)), (q(0.45), q(0.55)), (-INF, INF)]

    def groups(self, n_groups):
        """(lo, hi) of n_groups closed ranges on B's finite values: touching quantile bands, then one point group and one overlapping pair"""
        q = lambda f: self.quantile(self.B, f)
        # the point: a finite key under a bit that all three bitmaps have set, so that the point group selects something under each
        at = np.nonzero(self.mask_bits["cleared"].reshape(-1) & np.isfinite(self.B.want))[0][1000]
        point = float(self.B.want[at])
        if n_groups < 4:
            g = [(q(0.2), q(0.8))] * n_groups
        else:
            cuts = [q(f) for f in np.linspace(0.0, 1.0, n_groups - 2)]
            g = list(zip(cuts[:-1], cuts[1:])) + [(point, point), (q(0.2), q(0.6)), (q(0.4), q(0.8))]
        assert len(g) == n_groups
        return [a for a, _ in g], [b for _, b in g]


def unpack(words, nv):
    """a bitmap's int64 words on the host -> bool [nv, 1024]"""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little").astype(bool).reshape(nv, 1024)


@pytest.fixture(scope="module", params=["f64", "f32"])
def cols(ctx, request):
    return Columns(ctx, request.param)


# ---- what a failure prints ------------------------------------------------------------------------------------------------------------------------
def describe(b, bad_vectors, first_bad=None, limit=6):
    """(vector, scheme, bw, lbw, f, e, base, exc_cnt, first bad value) of the first vectors that differ"""
    e = b.enc
    rows = [(int(v), "ALP" if e["scheme"][v] == fr.SCHEME_ALP else "ALP_RD", int(e["bw"][v]), int(e["lbw"][v]), int(e["f"][v]), int(e["e"][v]), int(e["base"][v]),
             int(e["exc_cnt"][v]), None if first_bad is None else int(first_bad(int(v)))) for v in bad_vectors[:limit]]
    return f"{len(bad_vectors)} vectors differ; (vector, scheme, bw, lbw, f, e, base, exc_cnt, first bad value): {rows}"


def assert_bitmap(b, got, want_bits, what, other=None):
    """got: the device bitmap; want_bits: bool [nv, 1024]"""
    g = got.cpu().numpy().view(np.uint64)
    w = pack_bits(want_bits)
    if not np.array_equal(g, w):
        diff = unpack(g ^ w, b.nv)
        bad = np.nonzero(diff.any(axis=1))[0]
        text = f"{what}: {describe(b, bad, lambda v: np.nonzero(diff[v])[0][0])}"
        pytest.fail(text if other is None else text + f"; the other column there: {describe(other, bad)}")


def same_sums(got, want):
    return (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))


def assert_per_vector(b, same, what, other=None):
    """same: bool [nv] (or [G, nv]: a vector is bad if any group's entry is)"""
    same = np.asarray(same)
    if not same.all():
        bad = np.nonzero(~same.reshape(-1, b.nv).all(axis=0))[0]
        text = f"{what}: {describe(b, bad)}"
        pytest.fail(text if other is None else text + f"; the other column there: {describe(other, bad)}")


def ints(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


# =====================================================================================================================================================
# the columns are what the tests below need them to be
# =====================================================================================================================================================
def test_the_second_column_pairs_every_scheme_and_narrow_with_wide(cols):
    a, b = cols.A.enc, cols.B.enc
    pairs = set(zip((a["scheme"] == fr.SCHEME_ALP).tolist(), (b["scheme"] == fr.SCHEME_ALP).tolist()))
    assert pairs == {(True, True), (True, False), (False, True), (False, False)}, "ALP x ALP, ALP x ALP_RD, ALP_RD x ALP and ALP_RD x ALP_RD vector pairs"
    wide = a["bw"].astype(int) + b["bw"].astype(int)
    assert (wide >= cols.value_bits).any() and (wide < cols.value_bits).any(), "narrow meets wide: some pair's widths add up to the value width or more, some pair's do not"
    both = (a["exc_cnt"] > 0) & (b["exc_cnt"] > 0)
    assert both.any() and ((a["exc_cnt"] > 0) & (b["exc_cnt"] == 0)).any() and ((a["exc_cnt"] == 0) & (b["exc_cnt"] > 0)).any()
    assert (a["exc_cnt"][both] != b["exc_cnt"][both]).any(), "exception masks of different sizes side by side"
    # the same multiset of vectors: B's decode is a permutation of A's, vector by vector
    assert sorted(hash(r.tobytes()) for r in cols.A.bits.reshape(-1, 1024)) == sorted(hash(r.tobytes()) for r in cols.B.bits.reshape(-1, 1024))
    assert np.array_equal(cols.S.bits, cols.A.bits)


# =====================================================================================================================================================
# k_select: the kSelMask, kSelSum and kSelTake arms
# =====================================================================================================================================================
def test_select_mask(ctx, cols):
    for name, b in (("A", cols.A), ("B", cols.B)):
        preds = cols.predicates(b)
        q = []
        for lo, hi in preds:
            with np.errstate(invalid="ignore"):
                q.append((b.values >= b.want.dtype.type(lo)) & (b.values <= b.want.dtype.type(hi)))
            got = ctx.select_mask(b.col, lo, hi)
            assert_bitmap(b, got, q[-1], f"{cols.dtype} {name} select_mask SET [{lo!r}, {hi!r}]")
        assert 0 < q[0].sum() < q[0].size and (q[0] & b.exc_at).any() and (~q[0] & b.exc_at).any()
        prior = cols.masks["random"]
        mask = prior.clone()
        ctx.select_mask(b.col, *preds[0], op="and", mask=mask)
        assert_bitmap(b, mask, cols.mask_bits["random"] & q[0], f"{cols.dtype} {name} select_mask AND")
        mask = prior.clone()
        ctx.select_mask(b.col, *preds[1], op="or", mask=mask)
        assert_bitmap(b, mask, cols.mask_bits["random"] | q[1], f"{cols.dtype} {name} select_mask OR")
        if name == "A":  # mask_to_indices under one of those bitmaps
            idx = ctx.mask_to_indices(ctx.select_mask(b.col, *preds[0]))
            assert np.array_equal(idx.cpu().numpy(), np.nonzero(q[0].reshape(-1))[0])


@pytest.mark.parametrize("mname", ["full", "random", "cleared"])
def test_decode_sum_masked(ctx, cols, mname):
    for name, b in (("A", cols.A), ("B", cols.B)):
        want = cols.once(("sum", name, mname), lambda: host_sums_masked(b.values, cols.mask_bits[mname]))
        counts = torch.full((b.nv,), 7, dtype=torch.int32, device=DEV)
        got = ctx.decode_sum_masked(b.col, cols.masks[mname], counts=counts).cpu().numpy()
        assert_per_vector(b, same_sums(got, want), f"{cols.dtype} {name} decode_sum_masked under the {mname} bitmap")
        assert np.array_equal(counts.cpu().numpy(), cols.mask_bits[mname].sum(axis=1).astype(np.int32)), "counts are the popcounts"
        assert np.isfinite(want).sum() * 2 >= want.size, "at least half of the sums say something"


@pytest.mark.parametrize("mname", ["full", "random", "cleared"])
def test_decode_masked(ctx, cols, mname):
    for name, b in (("A", cols.A), ("B", cols.B)):
        bits = cols.mask_bits[mname]
        idx, vals = ctx.decode_masked(b.col, cols.masks[mname], indices=True)
        want_idx = np.nonzero(bits.reshape(-1))[0]
        got_idx = idx.cpu().numpy()
        assert got_idx.size == want_idx.size and (np.diff(got_idx) > 0).all() and np.array_equal(got_idx, want_idx), f"{cols.dtype} {name} {mname}: the indices are the set bits, ascending"
        same = ints(vals) == ints(b.want)[want_idx]
        if not same.all():
            first = want_idx[np.nonzero(~same)[0]]
            bad = np.unique(first >> 10)
            pytest.fail(f"{cols.dtype} {name} decode_masked under the {mname} bitmap: " + describe(b, bad, lambda v: first[first >> 10 == v][0] & 1023))


# =====================================================================================================================================================
# the decode under k_pair
# =====================================================================================================================================================
@pytest.mark.parametrize("cmp", sorted(CMPS))
def test_compare_mask(ctx, cols, cmp):
    a, b = cols.A, cols.B
    with np.errstate(invalid="ignore"):
        want = CMPS[cmp](a.values, b.values)
    assert 0 < want.sum() < want.size
    assert_bitmap(a, ctx.compare_mask(a.col, b.col, cmp), want, f"{cols.dtype} compare_mask(A, B, {cmp})", other=b)


def test_a_column_equals_itself_but_for_its_nans(ctx, cols):
    for name, b in (("A", cols.A), ("B", cols.B)):
        nan = np.isnan(b.values)
        assert nan.any() and (nan & b.exc_at).any()
        assert_bitmap(b, ctx.compare_mask(b.col, b.col, "eq"), ~nan, f"{cols.dtype} compare_mask({name}, {name}, eq)")


@pytest.mark.parametrize("mname", ["full", "random"])
def test_decode_dot_masked(ctx, cols, mname):
    a, b = cols.A, cols.B
    want = cols.once(("dot", mname), lambda: host_dots_masked(a.values, b.values, cols.mask_bits[mname]))
    counts = torch.full((a.nv,), 7, dtype=torch.int32, device=DEV)
    got = ctx.decode_dot_masked(a.col, b.col, cols.masks[mname], counts=counts).cpu().numpy()
    assert_per_vector(a, same_sums(got, want), f"{cols.dtype} decode_dot_masked(A, B) under the {mname} bitmap", other=b)
    assert np.array_equal(counts.cpu().numpy(), cols.mask_bits[mname].sum(axis=1).astype(np.int32))
    assert np.isfinite(want).sum() * 3 >= want.size, "a third of the dots say something"


# =====================================================================================================================================================
# the decode under k_group and k_group_minmax: the value column is A, the key column is B
# =====================================================================================================================================================
GROUP_MASK = {1: "full", 4: "random", 5: "cleared", 16: "random"}


@pytest.mark.parametrize("n_groups", GROUP_COUNTS)
def test_decode_group_sum(ctx, cols, n_groups):
    a, b, mname = cols.A, cols.B, GROUP_MASK[n_groups]
    lo, hi = cols.groups(n_groups)
    want_s, want_c = cols.once(("group_sum", n_groups), lambda: host_group_sums(a.values, b.values, cols.mask_bits[mname], lo, hi))
    counts = torch.full((n_groups, a.nv), 7, dtype=torch.int32, device=DEV)
    got = ctx.decode_group_sum(a.col, b.col, cols.masks[mname], lo, hi, counts=counts).cpu().numpy()
    what = f"{cols.dtype} decode_group_sum(A by B), {n_groups} groups under the {mname} bitmap"
    assert_per_vector(a, same_sums(got, want_s), what, other=b)
    assert_per_vector(a, counts.cpu().numpy() == want_c.astype(np.int32), what + " (counts)", other=b)
    assert all(0 < int(want_c[g].sum()) < cols.mask_bits[mname].sum() for g in range(n_groups)), "every group selects some but not all"


@pytest.mark.parametrize("n_groups", GROUP_COUNTS)
def test_decode_group_minmax(ctx, cols, n_groups):
    a, b, mname = cols.A, cols.B, GROUP_MASK[n_groups]
    lo, hi = cols.groups(n_groups)
    want_z, want_c = cols.once(("group_minmax", n_groups), lambda: host_group_minmax(a.values, b.values, cols.mask_bits[mname], lo, hi))
    counts = torch.full((n_groups, a.nv), 7, dtype=torch.int32, device=DEV)
    got = ctx.decode_group_minmax(a.col, b.col, cols.masks[mname], lo, hi, counts=counts)
    what = f"{cols.dtype} decode_group_minmax(A by B), {n_groups} groups under the {mname} bitmap"
    assert_per_vector(a, (ints(got) == ints(want_z)).all(axis=2), what, other=b)
    assert_per_vector(a, counts.cpu().numpy() == want_c.astype(np.int32), what + " (counts)", other=b)


# =====================================================================================================================================================
# the decode under k_minmax_masked
# =====================================================================================================================================================
@pytest.mark.parametrize("mname", ["full", "random"])
def test_decode_minmax_masked(ctx, cols, mname):
    for name, b in (("A", cols.A), ("B", cols.B)):
        want_z, want_c = cols.once(("minmax", name, mname), lambda: host_minmax_masked(b.values, cols.mask_bits[mname]))
        counts = torch.full((b.nv,), 7, dtype=torch.int32, device=DEV)
        got = ctx.decode_minmax_masked(b.col, cols.masks[mname], counts=counts)
        assert_per_vector(b, (ints(got) == ints(want_z)).all(axis=1), f"{cols.dtype} {name} decode_minmax_masked under the {mname} bitmap")
        assert np.array_equal(counts.cpu().numpy(), want_c.astype(np.int32))
        if mname == "full":
            # the records of the oracle's decode uploaded as a raw column: a route that shares no decode kernel with the call under test
            raw = ctx.zone_map_of_values(torch.from_numpy(b.want).to(DEV))
            assert got.cpu().numpy().tobytes() == raw.cpu().numpy().tobytes(), f"{cols.dtype} {name}: not the bytes of zone_map_of_values of the oracle's decode"


# =====================================================================================================================================================
# the decode under k_in_list: the whole list in LDS, its edge, and pivots in LDS with the list in L2
# =====================================================================================================================================================
IN_LISTS = ("about 50", "lds_max", "lds_max + 1")


def in_list_size(ctx, cols, which):
    lds_max = ctx.in_list_lds_max(cols.dtype)
    assert lds_max == 32768 // (cols.value_bits // 8)
    return {"about 50": 50, "lds_max": lds_max, "lds_max + 1": lds_max + 1}[which]


def make_list(b, size, seed):
    """`size` elements in no order: values of the oracle's decode that are not NaN — at exception positions of vectors with one exception and with many, at
    positions that read the upper half of an 8-entry dictionary, and anywhere — then 1-ulp neighbours of a fifth of them, and both zeros"""
    rng = np.random.default_rng(seed)
    dt = b.want.dtype.type
    e = b.enc
    n_near = size // 5
    n_hit = size - n_near - 2
    flat = b.want
    ok = ~np.isnan(b.values)
    exc = np.nonzero((b.exc_at & ok).reshape(-1))[0]
    few = exc[np.isin(exc >> 10, np.nonzero(e["exc_cnt"] <= 5)[0])]
    upper = np.nonzero((e["lbw"] == 3) & ~b.alp)[0]  # (a random position of such a vector reads entries 4..7 of an 8-entry dictionary half of the time)
    at = np.concatenate([rng.choice(exc, n_hit // 4, replace=False), rng.choice(few, min(few.size, n_hit // 8), replace=False),
                         1024 * rng.choice(upper, n_hit // 4) + rng.integers(0, 1024, n_hit // 4)])
    at = np.concatenate([at, rng.choice(np.nonzero(ok.reshape(-1))[0], n_hit - at.size, replace=False)])
    hits = flat[at]
    hits = hits[~np.isnan(hits)]
    with np.errstate(over="ignore"):
        near = np.nextafter(hits[:n_near], np.where(rng.random(min(n_near, hits.size)) < 0.5, dt(INF), dt(-INF)).astype(flat.dtype))
    near = near[~np.isnan(near)]
    lst = np.concatenate([hits, near, np.array([0.0, -0.0], flat.dtype)])
    while lst.size < size:  # (a drawn position was an ALP_RD exception that decodes to a NaN: top up with absent values)
        lst = np.concatenate([lst, (rng.standard_normal(size - lst.size) * 12345.678).astype(flat.dtype)])
    assert lst.size == size and not np.isnan(lst).any()
    return rng.permutation(lst)


def excluded_by_zone(zones, lst):
    """vectors whose record {min, max} holds no element of the list, by the definition"""
    s = np.sort(lst)
    at = np.searchsorted(s, zones[:, 0], side="left")
    with np.errstate(invalid="ignore"):
        return ~np.isnan(zones).any(axis=1) & ((at >= s.size) | (s[np.minimum(at, s.size - 1)] > zones[:, 1]))


def in_list_case(ctx, cols, b, name, which):
    size = in_list_size(ctx, cols, which)
    lst = cols.once(("list", name, which), lambda: make_list(b, size, 70 + size))
    member = cols.once(("member", name, which), lambda: host_in_mask(b.want, lst).reshape(b.nv, 1024))
    zones = cols.once(("zones", name), lambda: host_minmax_masked(b.values, np.ones((b.nv, 1024), bool))[0])
    return lst, member, zones


@pytest.mark.parametrize("which", IN_LISTS)
def test_select_in_mask(ctx, cols, which):
    for name, b in (("A", cols.A), ("B", cols.B)):
        lst, member, zones_host = in_list_case(ctx, cols, b, name, which)
        what = f"{cols.dtype} {name} select_in_mask, list of {lst.size}"
        assert 0 < member.sum() < member.size and (member & b.exc_at).any(), "some matched value sits at an exception position"
        assert (member & ~b.alp[:, None]).any() and (member & b.alp[:, None] & ~b.exc_at).any()
        dev_list = torch.from_numpy(lst).to(DEV)
        assert_bitmap(b, ctx.select_in_mask(b.col, dev_list), member, what)
        not_in = host_in_mask(b.want, lst, negate=True).reshape(b.nv, 1024)
        assert np.array_equal(not_in, ~member) and not_in[np.isnan(b.values)].all()
        assert_bitmap(b, ctx.select_in_mask(b.col, dev_list, negate=True), not_in, what + ", negate")
        zones = ctx.zone_map_of_values(torch.from_numpy(b.want).to(DEV))
        assert zones.cpu().numpy().tobytes() == zones_host.tobytes(), "zone_map_of_values of the oracle's decode is the replica's records"
        skipped = excluded_by_zone(zones_host, lst)
        assert skipped.any() and not skipped.all(), "some vector is skipped by its zone record"
        assert not member[skipped].any()
        assert_bitmap(b, ctx.select_in_mask(b.col, dev_list, zones=zones), member, what + ", with zones")


# =====================================================================================================================================================
# records out of vector order: one call of each family on the shuffled column, the expectation of the ordered one
# =====================================================================================================================================================
def test_every_family_on_the_column_with_shuffled_records(ctx, cols):
    a, s, b = cols.A, cols.S, cols.B
    bits, mask = cols.mask_bits["random"], cols.masks["random"]
    lo, hi = cols.predicates(a)[0]
    with np.errstate(invalid="ignore"):
        assert_bitmap(a, ctx.select_mask(s.col, lo, hi), (a.values >= a.want.dtype.type(lo)) & (a.values <= a.want.dtype.type(hi)), "select_mask")
        assert_bitmap(a, ctx.compare_mask(s.col, b.col, "lt"), a.values < b.values, "compare_mask", other=b)
    want = cols.once(("sum", "A", "random"), lambda: host_sums_masked(a.values, bits))
    assert_per_vector(a, same_sums(ctx.decode_sum_masked(s.col, mask).cpu().numpy(), want), "decode_sum_masked")
    vals = ctx.decode_masked(s.col, mask)
    assert np.array_equal(ints(vals), ints(a.want)[bits.reshape(-1)]), "decode_masked"
    want = cols.once(("dot", "random"), lambda: host_dots_masked(a.values, b.values, bits))
    assert_per_vector(a, same_sums(ctx.decode_dot_masked(s.col, b.col, mask).cpu().numpy(), want), "decode_dot_masked", other=b)
    glo, ghi = cols.groups(4)
    want_s, want_c = cols.once(("group_sum", 4), lambda: host_group_sums(a.values, b.values, bits, glo, ghi))
    assert GROUP_MASK[4] == "random"
    assert_per_vector(a, same_sums(ctx.decode_group_sum(s.col, b.col, mask, glo, ghi).cpu().numpy(), want_s), "decode_group_sum", other=b)
    want_z, _ = cols.once(("group_minmax", 4), lambda: host_group_minmax(a.values, b.values, bits, glo, ghi))
    assert_per_vector(a, (ints(ctx.decode_group_minmax(s.col, b.col, mask, glo, ghi)) == ints(want_z)).all(axis=2), "decode_group_minmax", other=b)
    want_z, _ = cols.once(("minmax", "A", "random"), lambda: host_minmax_masked(a.values, bits))
    assert_per_vector(a, (ints(ctx.decode_minmax_masked(s.col, mask)) == ints(want_z)).all(axis=1), "decode_minmax_masked")
    lst, member, _ = in_list_case(ctx, cols, a, "A", "about 50")
    assert_bitmap(a, ctx.select_in_mask(s.col, torch.from_numpy(lst).to(DEV)), member, "select_in_mask")


# =====================================================================================================================================================
# the coverage guard
# =====================================================================================================================================================
def decoded_vectors(ctx, cols):
    """{family: {column name: bool [nv]}}: the vectors each family's calls above decode, by the skip rules of the kernels — SET over the whole column decodes
    every vector, AND skips a vector whose words are all zero and OR one whose words are all ones, the masked consumers skip a vector without a set bit, and
    select_in_mask with zones one whose record holds no element of the list"""
    any_bit = {k: m.any(axis=1) for k, m in cols.mask_bits.items()}
    every = np.ones(cols.nv, bool)
    masked = any_bit["full"] | any_bit["random"] | any_bit["cleared"]
    group = np.zeros(cols.nv, bool)
    for g in GROUP_COUNTS:
        group |= any_bit[GROUP_MASK[g]]
    out = {"select_mask": {"A": every, "B": every}, "decode_sum_masked": {"A": masked, "B": masked}, "decode_masked": {"A": masked, "B": masked},
           "decode_minmax_masked": {"A": any_bit["full"] | any_bit["random"], "B": any_bit["full"] | any_bit["random"]},
           "compare_mask": {"A": every, "B": every}, "decode_dot_masked": {"A": any_bit["full"] | any_bit["random"], "B": any_bit["full"] | any_bit["random"]},
           "decode_group_sum": {"A": group, "B": group}, "decode_group_minmax": {"A": group, "B": group}, "select_in_mask": {}}
    for name, b in (("A", cols.A), ("B", cols.B)):
        zoned = np.zeros(cols.nv, bool)
        for which in IN_LISTS:
            lst, _, zones = in_list_case(ctx, cols, b, name, which)
            zoned |= ~excluded_by_zone(zones, lst)
        out["select_in_mask"][name] = every  # (the plain and the negated call decode every vector; the zoned one those below)
        out.setdefault("select_in_mask with zones", {})[name] = zoned
    return out


def classes(b, decoded):
    e = b.enc
    alp, rd = b.alp & decoded, ~b.alp & decoded
    return dict(widths=sorted(set(e["bw"][alp].tolist())), cuts=sorted(set(zip(e["bw"][rd].tolist(), e["lbw"][rd].tolist()))),
                alp_exc=sorted(set(e["exc_cnt"][alp].tolist())), rd_exc=sorted(set(e["exc_cnt"][rd].tolist())),
                width_by_exc=len(set(zip(e["bw"][alp].tolist(), e["exc_cnt"][alp].tolist()))))


def test_every_family_decoded_every_width_cut_and_exception_class(ctx, cols):
    rows = cols.rows
    widths, cuts = list(range(cols.value_bits + 1)), sorted(rows.rd_cuts())
    for family, per_column in decoded_vectors(ctx, cols).items():
        for name, decoded in per_column.items():
            got = classes(cols.A if name == "A" else cols.B, decoded)
            print(f"coverage {cols.dtype} {family} column {name}: {int(decoded.sum())} of {cols.nv} vectors decoded; ALP widths {got['widths'][0]}..{got['widths'][-1]} "
                  f"({len(got['widths'])}), ALP_RD cuts {len(got['cuts'])} of {len(cuts)}, ALP exception counts {got['alp_exc']}, ALP_RD exception counts {got['rd_exc']}, "
                  f"(width, exception count) pairs {got['width_by_exc']}")
            if family in FAMILIES:  # (the zoned calls of select_in_mask are reported only: the family's plain calls are what has to reach everything)
                assert got["widths"] == widths, (family, name)
                assert got["cuts"] == cuts, (family, name)
                assert got["alp_exc"] == sorted(rows.ALP_EXC_COUNTS) and got["rd_exc"] == sorted(rows.RD_EXC_COUNTS), (family, name)
    assert set(FAMILIES) <= set(decoded_vectors(ctx, cols))
    # ... and under the bitmap that clears two vectors of three, decoded and skipped vectors lie side by side in every class
    kept = cols.mask_bits["cleared"].any(axis=1)
    for b in (cols.A, cols.B):
        for decoded in (kept, ~kept):
            got = classes(b, decoded)
            assert got["widths"] == widths and got["cuts"] == cuts and got["alp_exc"] == sorted(rows.ALP_EXC_COUNTS) and got["rd_exc"] == sorted(rows.RD_EXC_COUNTS)
