"""The batch primitives (alpgpu_ffor_*, unffor_*, falp_*, decode_values_*, patch_*, encode_simdized_*, encode_values_*, encode_value_*, analyze_ffor_*,
rd_encode_vectors_* / rd_decode_vectors_*, both precisions) where tests/test_primitives_gpu.py does not reach:
  a. batches past one grid, so that wavefronts take a second trip of their grid-stride loop with another width, (e,f), state or exception count than on the first;
  b. packed and exception strides other than 1024, every output filled with a sentinel beforehand and compared whole, unused tails included;
  c. widths above the lane width, which are a no-op;
  d. every double (e,f) pair: falp, decode_values, encode_simdized + analyze_ffor + decode_values + patch, encode_value; the float encode_simdized under all 66;
  e. analyze_ffor with the extremes at chosen positions and ranges on the width boundaries;
  f. exception lists and exception placements aimed at the ballot ranks (counts around 64 and 128, a whole step, a whole lane, every second value);
  g. the ALP_RD primitives on every cut with a dictionary of its own, fed hand-built arrays;
  h. a closing guard that states what ran.
Every comparison is bit for bit on integer views against the oracle or a numpy restatement of a few lines (tests/primitive_inputs.py, kept honest by
tests/test_primitives_cpu.py); no GPU result serves as another's expectation.  The tests run in file order; the guard at the end counts what they covered."""
import numpy as np
import pytest
import torch

import primitive_inputs as pi
from primitive_inputs import F32, F64, VEC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 4096  # vectors compared at a time: bounds the gathered expectation at 32 MiB
SIGNED = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}
TORCH = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
RAN = {}  # entry point -> what it was run on, for the closing guard


def ran(name):
    return RAN.setdefault(name, dict(vectors=0, second_trip=0, widths=set(), pairs=set(), cuts=set(), dict_sizes=set(), packed_strides=set(), exc_strides=set(),
                                     state_idx=set(), counts=set()))


def note(name, n, first=None, **sets):
    r = ran(name)
    r["vectors"] += n
    if first is not None:
        r["second_trip"] += max(0, n - first)
    for k, v in sets.items():
        r[k] |= set(v)


@pytest.fixture(scope="module")
def oracles(oracle):
    from oracle.pyoracle import OracleF32
    return {64: oracle, 32: OracleF32(), 16: oracle, 8: oracle}


@pytest.fixture(scope="module")
def grid(ctx):
    """(vectors of one trip, the batch that reaches a second one)"""
    cus = ctx.device_info()["cu_count"]
    return 64 * cus, pi.second_trip_batch(cus)


def cu(a):
    """the array's bits on the device (torch has no unsigned 16 / 32 / 64-bit tensors: signed views throughout)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(SIGNED[a.dtype.itemsize])).to(DEV)


def filled(rows, cols, itemsize):
    """[rows, cols] of the sentinel"""
    t = torch.full((rows, cols * itemsize), pi.SENTINEL_BYTE, dtype=torch.uint8, device=DEV)
    return t if itemsize == 1 else t.view(TORCH[itemsize])


def filled1(n, itemsize):
    return filled(1, n, itemsize)[0]


def take(t, index):
    return t if index is None else t.index_select(0, index)


def assert_rows(got, want, index, what, info=None):
    """got[v] == want[index[v]] for every vector, compared on the device a chunk at a time; reports the first vector that differs"""
    if got.dim() == 1:
        got, want = got.unsqueeze(1), want.unsqueeze(1)
    assert got.dtype == want.dtype and got.shape[1] == want.shape[1], (what, got.dtype, want.dtype, got.shape, want.shape)
    for a in range(0, got.shape[0], CHUNK):
        b = min(got.shape[0], a + CHUNK)
        w = take(want[a:b] if index is None else want, None if index is None else index[a:b])
        ne = got[a:b] != w
        if bool(ne.any()):
            r, c = (int(q) for q in ne.nonzero()[0])
            v = a + r
            pytest.fail(f"{what}: vector {v} {info(v) if info else ''} differs first at element {c} (got {int(got[v, c])}, want {int(w[r, c])}); "
                        f"{int(ne.any(dim=1).sum())} of the vectors {a}..{b - 1} differ")


def trip_info(P, first):
    return lambda v: f"(pattern {v % P}, trip {v // first})"


def pattern_index(n, P):
    return torch.arange(n, device=DEV) % P


class Api:
    """the entry points of one precision under common names"""

    def __init__(self, ctx, prec):
        self.ctx, self.prec, self.sfx = ctx, prec, prec.name
        s = "" if prec.bits == 64 else "_f32"
        for name in ("falp", "decode_values", "patch", "encode_simdized", "encode_values", "rd_encode_vectors", "rd_decode_vectors"):
            setattr(self, name, getattr(ctx, name + s))
        self.analyze_ffor = ctx.analyze_ffor if prec.bits == 64 else ctx.analyze_ffor_i32
        self.isz = prec.bits // 8


FFOR = {64: ("ffor_i64", "unffor_i64"), 32: ("ffor_i32", "unffor_i32"), 16: ("ffor_u16", "unffor_u16"), 8: ("ffor_u8", "unffor_u8")}


# =====================================================================================================================================================
# runners shared by the sections: expectations per pattern, the batch is the patterns taken through `index` (None = one vector per pattern)
# =====================================================================================================================================================
def run_ffor_family(ctx, b, index, stride, label, first=None):
    """ffor and unffor (and falp; decode_values and analyze_ffor if every width is valid) of one lane width at one packed stride"""
    bits, words, P = b["bits"], b["words"], b["P"]
    dt, isz = pi.LANE[bits][0], bits // 8
    valid = b["bw"] <= bits
    sent = pi.sentinel(dt)
    want_packed = np.full((P, stride), sent)
    for i in range(P):
        if valid[i]:
            w = words * int(b["bw"][i])
            assert w <= stride and (stride * isz) % 16 == 0, "a packed row must fit its stride and stay 16-byte aligned"
            want_packed[i, :w] = b["packed"][i, :w]
    in_packed = pi.restride(b["packed"], stride, sent)
    want_vals = np.where(valid[:, None], b["vals"], sent)
    info = trip_info(P, first) if first else None
    bw, base = take(cu(b["bw"]), index), take(cu(b["base"]), index)
    n = bw.shape[0]
    ffor, unffor = FFOR[bits]
    sets = dict(widths=b["bw"].tolist(), packed_strides=[stride])
    d_vals = take(cu(b["vals"]), index)
    out = filled(n, stride, isz)
    getattr(ctx, ffor)(d_vals, out, bw, base)
    ctx.synchronize()
    assert_rows(out, cu(want_packed), index, f"{label}: {ffor} at stride {stride}", info)
    note(ffor, n, first, **sets)
    del out
    d_in = take(cu(in_packed), index)
    out = filled(n, VEC, isz)
    getattr(ctx, unffor)(d_in, out, bw, base)
    ctx.synchronize()
    assert_rows(out, cu(want_vals), index, f"{label}: {unffor} at stride {stride}", info)
    note(unffor, n, first, **sets)
    if bits not in (64, 32):
        return
    api = Api(ctx, F64 if bits == 64 else F32)
    fac, exp = take(cu(b["fac"]), index), take(cu(b["exp"]), index)
    want_falp = cu(np.where(valid[:, None], b["falp"], pi.sentinel(b["falp"].dtype)))
    pairs = set(zip(b["exp"].tolist(), b["fac"].tolist()))
    out = filled(n, VEC, isz)
    api.falp(d_in, out, bw, base, fac, exp)
    ctx.synchronize()
    assert_rows(out, want_falp, index, f"{label}: falp_{api.sfx} at stride {stride}", info)
    note(f"falp_{api.sfx}", n, first, pairs=pairs, **sets)
    del d_in
    if valid.all():
        out = filled(n, VEC, isz)
        api.decode_values(d_vals, out, fac, exp)
        ctx.synchronize()
        assert_rows(out, want_falp, index, f"{label}: decode_values_{api.sfx}", info)
        note(f"decode_values_{api.sfx}", n, first, pairs=pairs)
        del out
        geom = [pi.analyze_ffor_np(row) for row in b["vals"].view(api.prec.idt)]
        g_bw, g_base = filled1(n, 1), filled1(n, isz)
        api.analyze_ffor(d_vals, g_bw, g_base)
        ctx.synchronize()
        assert_rows(g_bw, cu(np.array([g[0] for g in geom], np.uint8)), index, f"{label}: analyze_ffor_{api.sfx} width", info)
        assert_rows(g_base, cu(np.array([g[1] for g in geom], api.prec.idt)), index, f"{label}: analyze_ffor_{api.sfx} base", info)
        note(f"analyze_ffor_{api.sfx}", n, first, widths=[g[0] for g in geom])


def check_encoded(api, got, w, index, stride, label, info, with_ef):
    d_exc, d_pos, d_cnt, d_enc, d_fac, d_exp = got
    assert_rows(d_cnt, cu(w["cnt"]), index, f"{label}: cnt", info)
    assert_rows(d_enc, cu(w["enc"]), index, f"{label}: enc", info)
    assert_rows(d_pos, cu(pi.restride(w["pos"], stride, pi.sentinel(np.uint16))), index, f"{label}: pos (tail beyond cnt included)", info)
    assert_rows(d_exc, cu(pi.restride(w["exc"], stride, pi.sentinel(api.prec.udt))), index, f"{label}: exc (tail beyond cnt included)", info)
    if with_ef:
        assert_rows(d_fac, cu(w["fac"]), index, f"{label}: fac", info)
        assert_rows(d_exp, cu(w["exp"]), index, f"{label}: exp", info)


def run_encode_simdized(api, w, index, stride, label, first=None):
    """encode_simdized of the expectation table's own vectors and (e,f)"""
    P = w["cnt"].size
    info = trip_info(P, first) if first else None
    assert int(w["cnt"].max()) <= stride
    x, fac, exp = take(cu(w["x"]), index), take(cu(w["fac"]), index), take(cu(w["exp"]), index)
    n = x.shape[0]
    got = (filled(n, stride, api.isz), filled(n, stride, 2), filled1(n, 2), filled(n, VEC, api.isz), fac, exp)
    api.encode_simdized(x, *got)
    api.ctx.synchronize()
    check_encoded(api, got, w, index, stride, f"{label}: encode_simdized_{api.sfx} at exception stride {stride}", info, False)
    note(f"encode_simdized_{api.sfx}", n, first, pairs=set(zip(w["exp"].tolist(), w["fac"].tolist())), exc_strides=[stride], counts=w["cnt"].tolist())


def run_encode_values(api, w, x_rows, states, S, pattern, state_of, state_idx, stride, label, first=None):
    """encode_values: vector v holds pattern pattern[v] and runs under states[state_of[v]] (through state_idx, or v / 100 when that is None); the table w has
    row p * S + s for pattern p under distinct state s % S"""
    P = x_rows.shape[0]
    info = (lambda v: f"(pattern {v % P}, trip {v // first}, state {int(state_of[v])})") if first else None
    n = pattern.shape[0]
    assert int(w["cnt"].max()) <= stride
    x = cu(x_rows).index_select(0, pattern)
    index = pattern * S + torch.from_numpy(state_of % S).to(DEV)
    got = (filled(n, stride, api.isz), filled(n, stride, 2), filled1(n, 2), filled(n, VEC, api.isz), filled1(n, 1), filled1(n, 1))
    api.encode_values(x, cu(states.view(np.uint8)), None if state_idx is None else cu(state_idx.astype(np.uint32)), *got)
    api.ctx.synchronize()
    mode = "v / 100" if state_idx is None else "state_idx"
    check_encoded(api, got, w, index, stride, f"{label}: encode_values_{api.sfx} ({mode}) at exception stride {stride}", info, True)
    note(f"encode_values_{api.sfx}", n, first, pairs=set(zip(w["exp"].tolist(), w["fac"].tolist())), exc_strides=[stride], state_idx=[mode], counts=w["cnt"].tolist())


def rd_decode_inputs(b, stride, left_at_exceptions=None):
    """the hand-built arrays rd_decode_vectors reads: slots beyond cnt hold a valid position and another left part, which a kernel that ran past cnt would apply"""
    N = b["cnt"].size
    live = np.arange(stride)[None, :] < b["cnt"][:, None]
    pos = np.where(live, pi.restride(b["pos"], stride, 0), 7).astype(np.uint16)
    exc = np.where(live, pi.restride(b["exc"], stride, 0), 0x1234).astype(np.uint16)
    left = b["left"].copy()
    if left_at_exceptions is not None:
        for i in range(N):
            left[i, b["pos"][i, :b["cnt"][i]]] = left_at_exceptions
    return left, exc, pos


def run_rd(api, b, states, index, state_idx, stride, label, first=None):
    """rd_encode_vectors against the numpy restatement; rd_decode_vectors fed the hand-built arrays (and with the left index at exception slots set to 8 and to
    0xFFFF) against the input bits.  state_idx: per pattern (taken through index like everything else), or None = v / 100"""
    prec = api.prec
    P = b["cnt"].size
    info = trip_info(P, first) if first else None
    assert int(b["cnt"].max()) <= stride
    d_states = cu(states.view(np.uint8))
    sidx = None if state_idx is None else take(cu(np.asarray(state_idx, np.uint32)), index)
    mode = "v / 100" if state_idx is None else "state_idx"
    x = take(cu(b["bits"]), index)
    n = x.shape[0]
    used = states[np.unique(b["state_idx"])]
    sets = dict(cuts=used["rd_rbw"].tolist(), dict_sizes=used["rd_dict_size"].tolist(), exc_strides=[stride], state_idx=[mode], counts=b["cnt"].tolist())
    d_exc, d_pos, d_cnt, d_right, d_left = filled(n, stride, 2), filled(n, stride, 2), filled1(n, 2), filled(n, VEC, api.isz), filled(n, VEC, 2)
    api.rd_encode_vectors(x, d_states, sidx, d_exc, d_pos, d_cnt, d_right, d_left)
    api.ctx.synchronize()
    what = f"{label}: rd_encode_vectors_{api.sfx} ({mode}) at exception stride {stride}"
    assert_rows(d_cnt, cu(b["cnt"]), index, what + ": cnt", info)
    assert_rows(d_right, cu(b["right"]), index, what + ": right", info)
    assert_rows(d_left, cu(b["left"]), index, what + ": left (dict_size at exception slots)", info)
    assert_rows(d_pos, cu(pi.restride(b["pos"], stride, pi.sentinel(np.uint16))), index, what + ": pos (tail beyond cnt included)", info)
    assert_rows(d_exc, cu(pi.restride(b["exc"], stride, pi.sentinel(np.uint16))), index, what + ": exc (tail beyond cnt included)", info)
    note(f"rd_encode_vectors_{api.sfx}", n, first, **sets)
    del d_exc, d_pos, d_right, d_left
    right, cnt, want = take(cu(b["right"]), index), take(cu(b["cnt"]), index), cu(b["bits"])
    for at_exc in (None, 8, 0xFFFF):
        left, exc, pos = rd_decode_inputs(b, stride, at_exc)
        out = filled(n, VEC, api.isz)
        api.rd_decode_vectors(out, right, take(cu(left), index), d_states, sidx, take(cu(exc), index), take(cu(pos), index), cnt)
        api.ctx.synchronize()
        assert_rows(out, want, index, f"{label}: rd_decode_vectors_{api.sfx} ({mode}) at exception stride {stride}, left index at exception slots "
                    f"{'dict_size' if at_exc is None else at_exc}", info)
        del out
        if first:
            break  # the big batch runs the plain form only
    note(f"rd_decode_vectors_{api.sfx}", n, first, **sets)


def run_patch(api, c, index, stride, label, first=None):
    P = c["cnt"].size
    info = trip_info(P, first) if first else None
    assert int(c["cnt"].max()) <= stride
    out = take(cu(c["out"]), index)
    n = out.shape[0]
    api.patch(out, take(cu(pi.restride(c["exc"], stride, 0)), index), take(cu(pi.restride(c["pos"], stride, 0)), index), take(cu(c["cnt"]), index))
    api.ctx.synchronize()
    assert_rows(out, cu(c["want"]), index, f"{label}: patch_{api.sfx} at exception stride {stride}", info)
    note(f"patch_{api.sfx}", n, first, exc_strides=[stride], counts=c["cnt"].tolist())


def subset(d, keep, keys):
    out = dict(d)
    for k in keys:
        out[k] = d[k][keep]
    return out


# =====================================================================================================================================================
# a. past one grid
# =====================================================================================================================================================
@pytest.mark.parametrize("bits", [64, 32, 16, 8])
def test_a_ffor_family_past_one_grid(ctx, oracles, grid, bits):
    """ffor / unffor of every lane width (with bases), falp, decode_values and analyze_ffor: a wavefront's second vector has another width, base and (e,f)"""
    first, n = grid
    prec = {64: F64, 32: F32}.get(bits)
    b = pi.ffor_patterns(oracles[bits], bits, pi.big_ffor_widths(bits), seed=100 + bits, ef=prec.ef if prec else None)
    assert b["P"] % 2 == 1 and 33 <= b["P"] <= 70
    run_ffor_family(ctx, b, pattern_index(n, b["P"]), VEC, "past one grid", first)


@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
def test_a_patch_past_one_grid(ctx, grid, prec):
    first, n = grid
    c = pi.patch_cases(prec, seed=21, counts=tuple(range(0, 65, 4)) + (1, 63, 64, 3))
    keep = np.nonzero(c["cnt"] <= pi.BIG_EXC_STRIDE)[0]
    keep = keep[:keep.size - (keep.size + 1) % 2]  # an odd period
    c = subset(c, keep, ("out", "exc", "pos", "cnt", "want"))
    assert keep.size % 2 == 1 and 33 <= keep.size <= 70
    run_patch(Api(ctx, prec), c, pattern_index(n, keep.size), pi.BIG_EXC_STRIDE, "past one grid", first)


@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
def test_a_alp_encoders_past_one_grid(ctx, oracles, grid, prec):
    """encode_simdized, and encode_values with states that alternate k > 1 and k = 1 from one trip to the next, through v / 100 and through a state_idx that is
    not monotone"""
    first, n = grid
    o, api = oracles[prec.bits], Api(ctx, prec)
    x, distinct = pi.alp_patterns(prec), pi.alternating_states(o, prec)
    P, S = x.shape[0], distinct.size
    w = pi.encode_values_expectations(o, prec, x, distinct, pi.BIG_EXC_STRIDE)
    own = np.arange(P) * S + np.arange(P) % S  # encode_simdized: pattern p under the (e,f) its state p % S chose
    run_encode_simdized(api, subset(w, own, ("x", "exp", "fac", "cnt", "enc", "exc", "pos")), pattern_index(n, P), pi.BIG_EXC_STRIDE, "past one grid", first)
    pattern = pattern_index(n, P)
    # v / 100: rowgroup r runs under distinct[r % S], shifted by one from the second trip's first rowgroup on if that is what makes the two trips differ in k
    r = np.arange(n) // pi.ROWGROUP
    r2 = first // pi.ROWGROUP
    rg_state = (np.arange(r.max() + 1) + (np.arange(r.max() + 1) >= r2) * (r2 % 2 == 0)) % S
    state_of = rg_state[r]
    assert state_of.size >= 201 and all(int(distinct[state_of[v]]["k"] > 1) != int(distinct[state_of[v - first]]["k"] > 1) for v in range(first, n))
    run_encode_values(api, w, x, distinct[rg_state], S, pattern, state_of, None, pi.BIG_EXC_STRIDE, "past one grid", first)
    state_of = (7 * np.arange(n) + 3) % S
    state_of[first:] = (state_of[:n - first] + 1) % S
    assert (np.diff(state_of) < 0).any() and all(int(distinct[state_of[v]]["k"] > 1) != int(distinct[state_of[v - first]]["k"] > 1) for v in range(first, n))
    run_encode_values(api, w, x, distinct, S, pattern, state_of, state_of, pi.BIG_EXC_STRIDE, "past one grid", first)


def rd_big_batch(prec):
    states = pi.rd_states(prec)
    pl = [p for _, p in pi.placements(prec, seed=22, counts=(0, 1, 63, 64, 2, 33)) if p.size <= pi.BIG_EXC_STRIDE]
    lists = [pl[i % len(pl)] for i in range(33)]
    sidx = [i % len(prec.cuts) for i in range(33)]
    return states, pi.rd_batch(prec, states, sidx, lists, seed=23)


@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
def test_a_alp_rd_primitives_past_one_grid(ctx, grid, prec):
    first, n = grid
    states, b = rd_big_batch(prec)
    run_rd(Api(ctx, prec), b, states, pattern_index(n, 33), b["state_idx"], pi.BIG_EXC_STRIDE, "past one grid", first)


# =====================================================================================================================================================
# b. strides and sentinels, c. no-op widths
# =====================================================================================================================================================
@pytest.mark.parametrize("bits", [64, 32, 16, 8])
def test_b_packed_strides(ctx, oracles, bits):
    """the tight stride of the batch's largest width (bw = 0 included: ffor writes nothing, unffor gives the base) and 1024 + 16"""
    prec = {64: F64, 32: F32}.get(bits)
    words = pi.LANE[bits][1]
    for top, stride in ((bits * 5 // 8, words * (bits * 5 // 8)), (bits // 8, words * (bits // 8)), (bits, VEC), (bits, VEC + 16)):
        b = pi.ffor_patterns(oracles[bits], bits, list(range(top + 1)) * 2, seed=200 + bits + top, ef=prec.ef if prec else None)
        run_ffor_family(ctx, b, None, stride, f"widths 0..{top}")


@pytest.mark.parametrize("bits", [64, 32, 16, 8])
def test_c_widths_above_the_lane_width_are_a_no_op(ctx, oracles, bits):
    """bw = lane width + 1 and 255 between valid widths: their outputs keep the sentinel, their neighbours are exact"""
    prec = {64: F64, 32: F32}.get(bits)
    b = pi.ffor_patterns(oracles[bits], bits, pi.noop_mix_widths(bits), seed=300 + bits, ef=prec.ef if prec else None)
    assert set(pi.NOOP_WIDTHS[bits]) <= set(b["bw"].tolist())
    run_ffor_family(ctx, b, None, VEC, "no-op widths mixed in")
    run_ffor_family(ctx, b, None, VEC + 16, "no-op widths mixed in")


@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
def test_b_f_exception_strides_lists_and_placements(ctx, oracles, prec):
    """patch_* on hand-built lists (ascending and descending; counts around one and two ballots; both ends) and encode_simdized_* on vectors whose exceptions
    fill one step, one lane, every second value: at the batch's largest count as stride, at 1024 and at 1024 + 8; order, count and untouched tail"""
    o, api = oracles[prec.bits], Api(ctx, prec)
    c = pi.patch_cases(prec)
    small = np.nonzero(c["cnt"] <= 129)[0]
    run_patch(api, c, None, VEC, "hand-built lists")
    run_patch(api, c, None, VEC + 8, "hand-built lists")
    run_patch(api, subset(c, small, ("out", "exc", "pos", "cnt", "want")), None, 129, "hand-built lists up to 129")
    x, pl = pi.alp_placed_vectors(prec)
    e, f = pi.ALP_PLACED_EF[prec.bits]
    w = pi.simdized_expectations(o, prec, x, [e] * len(pl), [f] * len(pl))
    assert [int(q) for q in w["cnt"]] == [p.size for _, p in pl]
    keys = ("x", "exp", "fac", "cnt", "enc", "exc", "pos")
    run_encode_simdized(api, w, None, VEC, "placed exceptions")
    run_encode_simdized(api, w, None, VEC + 8, "placed exceptions")
    small = np.nonzero(w["cnt"] <= 129)[0]
    run_encode_simdized(api, subset(w, small, keys), None, 129, "placed exceptions up to 129")
    # encode_values at a second stride: every pattern of the big batch under every state
    xs, distinct = pi.alp_patterns(prec), pi.alternating_states(o, prec)
    P, S = xs.shape[0], distinct.size
    wv = pi.encode_values_expectations(o, prec, xs, distinct, VEC + 8)
    pattern = torch.arange(P * S, device=DEV) // S
    state_of = np.arange(P * S) % S
    run_encode_values(api, wv, xs, distinct, S, pattern, state_of, state_of, VEC + 8, "every pattern under every state")
    tight = int(wv["cnt"].max())
    run_encode_values(api, pi.encode_values_expectations(o, prec, xs, distinct, tight), xs, distinct, S, pattern, state_of, state_of, tight,
                      "every pattern under every state")


# =====================================================================================================================================================
# d. every (e,f)
# =====================================================================================================================================================
def test_d_falp_and_decode_values_under_every_double_pair(ctx, oracle):
    """integers on the edges of the decoder's arithmetic (the int64 product wraps), one vector per pair, packed at width 64 under a base of their own"""
    rows = pi.edge_integer_rows(F64)
    n = rows.shape[0]
    assert n == 190
    rng = np.random.default_rng(31)
    base = rng.integers(F64.imin, F64.imax, n, dtype=np.int64)
    bw = np.full(n, 64, np.uint8)
    exp, fac = np.array([e for e, f in F64.ef], np.uint8), np.array([f for e, f in F64.ef], np.uint8)
    packed = np.stack([oracle.ffor_u64(rows[i], 64, int(base[i])) for i in range(n)])
    want = cu(np.stack([oracle.falp(packed[i], 64, int(base[i]), int(fac[i]), int(exp[i])) for i in range(n)]))
    info = lambda v: f"(e, f) = {F64.ef[v]}"
    out = filled(n, VEC, 8)
    ctx.falp(cu(packed), out, cu(bw), cu(base), cu(fac), cu(exp))
    ctx.synchronize()
    assert_rows(out, want, None, "falp_f64 under every pair", info)
    out = filled(n, VEC, 8)
    ctx.decode_values(cu(rows), out, cu(fac), cu(exp))
    ctx.synchronize()
    assert_rows(out, want, None, "decode_values_f64 under every pair", info)
    note("falp_f64", n, pairs=F64.ef, widths=[64], packed_strides=[VEC])
    note("decode_values_f64", n, pairs=F64.ef)


@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
def test_d_encode_simdized_analyze_decode_patch_under_every_pair(ctx, oracles, prec):
    """the adversarial vectors and vectors of the search's boundary values under all 190 / 66 pairs: encode_simdized and analyze_ffor against the oracle;
    decode_values + patch of the oracle's encoding must give the input bits back"""
    o, api = oracles[prec.bits], Api(ctx, prec)
    vecs = pi.boundary_vectors(prec)
    V, E = vecs.shape[0], len(prec.ef)
    x = np.tile(vecs, (E, 1))
    exp, fac = np.repeat([e for e, f in prec.ef], V), np.repeat([f for e, f in prec.ef], V)
    w = pi.simdized_expectations(o, prec, x, exp, fac)
    run_encode_simdized(api, w, None, VEC, "every pair")
    n = x.shape[0]
    info = lambda v: f"(vector {v % V}, (e, f) = {prec.ef[v // V]})"
    geom = [o.analyze_ffor(row) for row in w["enc"]]
    d_enc, g_bw, g_base = cu(w["enc"]), filled1(n, 1), filled1(n, api.isz)
    api.analyze_ffor(d_enc, g_bw, g_base)
    out = filled(n, VEC, api.isz)
    api.decode_values(d_enc, out, cu(w["fac"]), cu(w["exp"]))
    api.patch(out, cu(pi.restride(w["exc"], VEC, 0)), cu(np.where(np.arange(VEC)[None, :] < w["cnt"][:, None], w["pos"], 0).astype(np.uint16)), cu(w["cnt"]))
    ctx.synchronize()
    assert_rows(g_bw, cu(np.array([g[0] for g in geom], np.uint8)), None, f"analyze_ffor_{api.sfx} width under every pair", info)
    assert_rows(g_base, cu(np.array([g[1] for g in geom], prec.idt)), None, f"analyze_ffor_{api.sfx} base under every pair", info)
    assert_rows(out, cu(w["x"]), None, f"decode_values_{api.sfx} + patch_{api.sfx} must reproduce the input bits", info)
    pairs = set(zip(w["exp"].tolist(), w["fac"].tolist()))
    note(f"analyze_ffor_{api.sfx}", n, widths=[g[0] for g in geom], pairs=pairs)
    note(f"decode_values_{api.sfx}", n, pairs=pairs)
    note(f"patch_{api.sfx}", n, pairs=pairs, exc_strides=[VEC], counts=w["cnt"].tolist())


def test_d_encode_value_of_every_boundary_value_under_every_double_pair(ctx, oracle):
    """alpgpu_encode_value_f64, the sampling form (sentinel for what cannot be encoded) and the plain one (the conversion as x86 executes it)"""
    values = pi.unique_boundary_values()
    x = torch.from_numpy(values).to(DEV)
    got = {(e, f, safe): ctx.encode_value(x, f, e, safe=safe) for e, f in F64.ef for safe in (True, False)}
    ctx.synchronize()
    for (e, f, safe), g in got.items():
        want = pi.oracle_encode_value_f64(oracle, values, e, f, safe)
        g = g.cpu().numpy()
        bad = np.nonzero(g != want)[0]
        assert bad.size == 0, (f"encode_value_f64(e={e}, f={f}, safe={safe}): {bad.size} values differ from the oracle; (value, got, want): "
                               f"{[(float(values[i]).hex(), int(g[i]), int(want[i])) for i in bad[:6]]}")
    note("encode_value_f64", values.size * len(got), pairs=F64.ef)


# =====================================================================================================================================================
# e. analyze_ffor
# =====================================================================================================================================================
@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
def test_e_analyze_ffor_extremes_at_every_position_and_ranges_on_every_width_boundary(ctx, prec):
    api = Api(ctx, prec)
    rows, names = pi.analyze_cases(prec)
    n = rows.shape[0]
    geom = [pi.analyze_ffor_np(r) for r in rows]
    g_bw, g_base = filled1(n, 1), filled1(n, api.isz)
    api.analyze_ffor(cu(rows), g_bw, g_base)
    ctx.synchronize()
    info = lambda v: f"({names[v][0]})"
    assert_rows(g_bw, cu(np.array([g[0] for g in geom], np.uint8)), None, f"analyze_ffor_{api.sfx} width", info)
    assert_rows(g_base, cu(np.array([g[1] for g in geom], prec.idt)), None, f"analyze_ffor_{api.sfx} base", info)
    note(f"analyze_ffor_{api.sfx}", n, widths=[g[0] for g in geom])


# =====================================================================================================================================================
# g. ALP_RD primitives
# =====================================================================================================================================================
@pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
def test_g_alp_rd_primitives_on_every_cut(ctx, prec):
    """every cut with its own dictionary (sizes 1..8) under every exception placement: through a shuffled state_idx at three exception strides, and through
    v / 100 with three states"""
    api = Api(ctx, prec)
    states = pi.rd_states(prec)
    pl = [p for _, p in pi.placements(prec, seed=41, counts=(0, 1, 63, 64, 65, 1024))]
    rng = np.random.default_rng(42)
    order = rng.permutation(len(pl) * len(prec.cuts))
    b = pi.rd_batch(prec, states, (order % len(prec.cuts)), [pl[i // len(prec.cuts)] for i in order], seed=43)
    assert (np.diff(b["state_idx"].astype(np.int64)) < 0).any()
    run_rd(api, b, states, None, b["state_idx"], VEC, "every cut")
    run_rd(api, b, states, None, b["state_idx"], VEC + 8, "every cut")
    small = np.nonzero(b["cnt"] <= 65)[0]
    run_rd(api, subset(b, small, ("bits", "right", "left", "exc", "pos", "cnt", "state_idx")), states, None, b["state_idx"][small], 65, "every cut, up to 65 exceptions")
    three = states[[5, 12, 0]]
    n = 2 * pi.ROWGROUP + 37
    b = pi.rd_batch(prec, three, np.arange(n) // pi.ROWGROUP, [pl[i % len(pl)] for i in range(n)], seed=44)
    run_rd(api, b, three, None, None, VEC, "three rowgroups")


# =====================================================================================================================================================
# h. closing guard
# =====================================================================================================================================================
def test_h_every_kernel_ran_past_one_grid_on_every_width_pair_cut_and_stride(grid):
    first, n = grid
    for name in sorted(RAN):
        r = RAN[name]
        print(f"coverage {name}: {r['vectors']} vectors, {r['second_trip']} on a second trip; widths {len(r['widths'])}, (e,f) pairs {len(r['pairs'])}, cuts "
              f"{len(r['cuts'])}, dictionary sizes {sorted(r['dict_sizes'])}, packed strides {sorted(r['packed_strides'])}, exception strides "
              f"{sorted(r['exc_strides'])}, state index {sorted(r['state_idx'])}, exception counts {len(r['counts'])} distinct")
    both = lambda stem: [f"{stem}_f64", f"{stem}_f32"]
    batch = (["ffor_i64", "unffor_i64", "ffor_i32", "unffor_i32", "ffor_u16", "unffor_u16", "ffor_u8", "unffor_u8"] + both("falp") + both("decode_values") +
             both("analyze_ffor") + both("patch") + both("encode_simdized") + both("encode_values") + both("rd_encode_vectors") + both("rd_decode_vectors"))
    for name in batch:
        assert name in RAN and RAN[name]["second_trip"] >= n - first > 0, f"{name} never took a second trip"
    for bits, (a, b) in FFOR.items():
        for name in (a, b) + ((f"falp_f{bits}",) if bits >= 32 else ()):
            assert set(range(bits + 1)) | set(pi.NOOP_WIDTHS[bits]) <= RAN[name]["widths"], name
            assert len(RAN[name]["packed_strides"]) >= 4 and VEC + 16 in RAN[name]["packed_strides"], name
    for name in both("patch") + both("encode_simdized") + both("encode_values") + both("rd_encode_vectors") + both("rd_decode_vectors"):
        assert len(RAN[name]["exc_strides"]) >= 2 and VEC + 8 in RAN[name]["exc_strides"], name
    for name in ("falp", "decode_values", "encode_simdized", "analyze_ffor", "patch"):
        assert set(F64.ef) <= RAN[name + "_f64"]["pairs"] and len(F64.ef) == 190, name
    assert set(F64.ef) <= RAN["encode_value_f64"]["pairs"]
    assert set(F32.ef) <= RAN["encode_simdized_f32"]["pairs"] and len(F32.ef) == 66
    for prec in (F64, F32):
        for stem in ("rd_encode_vectors", "rd_decode_vectors"):
            r = RAN[f"{stem}_{prec.name}"]
            assert r["cuts"] == set(prec.cuts) and len(r["cuts"]) == 16 and r["dict_sizes"] == set(range(1, 9)), (stem, prec.name)
            assert r["state_idx"] == {"v / 100", "state_idx"} and {0, 1, 63, 64, 65, 1024} <= r["counts"], (stem, prec.name)
        assert RAN[f"encode_values_{prec.name}"]["state_idx"] == {"v / 100", "state_idx"}
        for stem in ("patch", "encode_simdized"):
            assert set(pi.EXC_COUNTS) <= RAN[f"{stem}_{prec.name}"]["counts"], (stem, prec.name)
        assert set(range(prec.bits + 1)) <= RAN[f"analyze_ffor_{prec.name}"]["widths"]
