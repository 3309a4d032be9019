"""CPU: keeps the inputs of tests/test_primitive_batches_gpu.py honest (tests/primitive_inputs.py).  What the GPU file's closing guard claims to have run really
occurs in the inputs; the numpy restatements equal the oracle wherever the oracle has the function; where oracle/_ref is built, the oracle equals the reference on
exactly these inputs; and every batch the GPU file passes with a tight exception stride has no vector with more exceptions than that stride."""
import ctypes as C

import numpy as np
import pytest

import primitive_inputs as pi
from primitive_inputs import F32, F64, VEC

PRECS = pytest.mark.parametrize("prec", [F64, F32], ids=["f64", "f32"])
LANES = pytest.mark.parametrize("bits", [64, 32, 16, 8])


@pytest.fixture(scope="module")
def oracles(oracle):
    from oracle.pyoracle import OracleF32
    return {64: oracle, 32: OracleF32(), 16: oracle, 8: oracle}


@pytest.fixture(scope="module")
def refs():
    from oracle.pyoracle import Reference, ReferenceF32
    if not (Reference.available() and ReferenceF32.available()):
        pytest.skip("oracle/_ref is not built")
    return {64: Reference(), 32: ReferenceF32(), 16: Reference(), 8: Reference()}


def ffor_batches(o, bits):
    """every FFOR batch the GPU file builds for this lane width"""
    prec = {64: F64, 32: F32}.get(bits)
    ef = prec.ef if prec else None
    out = [pi.ffor_patterns(o, bits, pi.big_ffor_widths(bits), seed=100 + bits, ef=ef), pi.ffor_patterns(o, bits, pi.noop_mix_widths(bits), seed=300 + bits, ef=ef)]
    for top in (bits * 5 // 8, bits // 8, bits):
        out.append(pi.ffor_patterns(o, bits, list(range(top + 1)) * 2, seed=200 + bits + top, ef=ef))
    return out


def test_the_state_record_is_the_librarys():
    from alp_amd import capi
    assert pi.STATE_DTYPE == capi.ROWGROUP_DTYPE and pi.STATE_DTYPE.itemsize == 32
    assert (pi.SCHEME_ALP, pi.SCHEME_ALP_RD, pi.ROWGROUP) == (capi.SCHEME_ALP, capi.SCHEME_ALP_RD, capi.ROWGROUP_VECTORS)


def test_the_second_trip_batch_is_the_smallest_with_a_part_filled_workgroup():
    for cus in (1, 64, 256, 304):
        n, first = pi.second_trip_batch(cus), 64 * cus
        grid = cus * 16                           # prim_grid's cap, 4 wavefronts each
        assert grid * 4 == first and n > first    # vector `first` is wavefront 0's second
        assert (n - first) // 4 == 1 and (n - first) % 4 == 3  # one whole workgroup on a second trip, then three wavefronts of the next


@LANES
def test_ffor_patterns_hold_every_width_and_an_odd_period(oracles, bits):
    big = pi.big_ffor_widths(bits)
    assert len(big) % 2 == 1 and 33 <= len(big) <= 70 and set(big) == set(range(bits + 1))
    for cus in (64, 256, 304):  # a wavefront's two trips see different patterns
        assert all(pi.pattern_of(v, len(big)) != pi.pattern_of(v + 64 * cus, len(big)) for v in range(7))
    mix = pi.noop_mix_widths(bits)
    assert set(mix) == set(range(bits + 1)) | set(pi.NOOP_WIDTHS[bits]) and min(pi.NOOP_WIDTHS[bits]) == bits + 1
    for b in ffor_batches(oracles[bits], bits):
        dt, words = pi.LANE[bits]
        span = (b["vals"] - b["base"][:, None]).astype(dt)  # wraps
        for i, bw in enumerate(b["bw"]):
            if bw < bits:
                assert int(span[i].max()) < 2**int(bw)
            if 1 <= bw <= bits:
                assert np.any(b["packed"][i, :words * int(bw)]) and not np.any(b["packed"][i, words * int(bw):])
        if "falp" in b:
            assert len(set(zip(b["exp"].tolist(), b["fac"].tolist()))) >= min(b["P"], 30) and (b["fac"] <= b["exp"]).all()


@LANES
def test_the_oracle_equals_the_reference_on_the_ffor_patterns(oracles, refs, bits):
    o, r = oracles[bits], refs[bits]
    for b in ffor_batches(o, bits):
        for i, bw in enumerate(int(w) for w in b["bw"]):
            if bw > bits:
                continue
            base = int(b["base"][i])
            words = b["words"] * bw
            assert np.array_equal(getattr(r, f"ffor_u{bits}")(b["vals"][i], bw, base)[:words], b["packed"][i, :words]), (bits, bw)
            assert np.array_equal(getattr(r, f"unffor_u{bits}")(b["packed"][i], bw, base), b["vals"][i]), (bits, bw)
            if "falp" in b and not (bits == 32 and b["fac"][i] == 10):  # the reference reads past its table at the float f = 10
                e, f = int(b["exp"][i]), int(b["fac"][i])
                assert np.array_equal(r.unffor_decode(b["packed"][i], bw, base, f, e).view(b["falp"].dtype), b["falp"][i]), (bits, bw, e, f)
                if bw < bits:  # the reference's fused kernel is broken at the full width
                    assert np.array_equal(r.falp(b["packed"][i], bw, base, f, e).view(b["falp"].dtype), b["falp"][i]), (bits, bw, e, f)


@PRECS
def test_analyze_cases_and_the_restatement(oracles, prec):
    o = oracles[prec.bits]
    rows, names = pi.analyze_cases(prec)
    got = [pi.analyze_ffor_np(r) for r in rows]
    assert got == [o.analyze_ffor(r) for r in rows]
    for p in range(VEC):
        assert int(rows[p].argmin()) == p and int(rows[p].argmax()) == VEC - 1 - p and np.count_nonzero(rows[p] == rows[p].min()) == 1
    for (w, _), (name, aimed) in zip(got, names):
        assert aimed is None or w == aimed, name
    aimed = [a for _, a in names if a is not None]
    assert all(aimed.count(bw) == 2 for bw in range(1, prec.bits)) and aimed.count(0) == 1 and aimed.count(prec.bits) == 3
    assert rows[-1].min() == prec.imin and rows[-1].max() == prec.imax and np.unique(rows[-2]).size == 1
    from oracle.pyoracle import Reference, ReferenceF32
    R = Reference if prec.bits == 64 else ReferenceF32
    if R.available():
        r = R()
        assert got == [r.analyze_ffor(row) for row in rows]


@PRECS
def test_placements_aim_at_the_ballot_ranks(prec):
    pl = dict(pi.placements(prec))
    assert [pl[f"{c} random"].size for c in pi.EXC_COUNTS] == list(pi.EXC_COUNTS) == [0, 1, 63, 64, 65, 127, 128, 129, 1024]
    for name, p in pl.items():
        assert np.array_equal(p, np.unique(p)) and (p.size == 0 or (0 <= p.min() and p.max() < VEC)), name
    # position = 128 m + 2 lane + j (double), 256 m + 4 lane + j (float): a step is one (m, j) in all 64 lanes, a lane all (m, j) of one lane
    per = prec.per_lane
    for name in ("first step", "last step", "a middle step"):
        p = pl[name]
        assert p.size == 64 and np.unique(p // (64 * per)).size == 1 and np.unique(p % per).size == 1 and np.array_equal(np.unique(p % (64 * per) // per), np.arange(64))
    for name, lane in (("lane 0", 0), ("lane 63", 63), ("lane 37", 37)):
        p = pl[name]
        assert p.size == 16 and (p % (64 * per) // per == lane).all()
    assert pl["both ends"].tolist() == [0, VEC - 1] and pl["every second value"].size == 512
    c = pi.patch_cases(prec)
    assert set(pi.EXC_COUNTS) <= set(c["cnt"].tolist())
    assert sum("descending" in n for n in c["names"]) >= 10
    for i, name in enumerate(c["names"]):
        k = int(c["cnt"][i])
        d = np.diff(c["pos"][i, :k].astype(np.int64))
        assert np.unique(c["pos"][i, :k]).size == k and ((d < 0).all() if "descending" in name else (d > 0).all()), name
        assert c["pos"][i].max() < VEC  # the slots beyond cnt too: a kernel that read them would stay inside the vector


@PRECS
def test_patch_restatement_is_the_oracles(oracles, prec):
    o = oracles[prec.bits]
    c = pi.patch_cases(prec)
    for i in range(c["cnt"].size):
        out = c["out"][i].copy()
        o.fn("patch")(pi._p(out), pi._p(c["exc"][i]), pi._p(c["pos"][i]), C.c_uint16(int(c["cnt"][i])))
        assert np.array_equal(out, c["want"][i]), c["names"][i]


@PRECS
def test_placed_alp_vectors_have_their_exceptions_where_aimed(oracles, prec):
    o = oracles[prec.bits]
    x, pl = pi.alp_placed_vectors(prec)
    e, f = pi.ALP_PLACED_EF[prec.bits]
    w = pi.simdized_expectations(o, prec, x, [e] * len(pl), [f] * len(pl))
    for i, (name, p) in enumerate(pl):
        assert int(w["cnt"][i]) == p.size and np.array_equal(w["pos"][i, :p.size], p), name
        assert (w["pos"][i, p.size:] == pi.sentinel(np.uint16)).all() and (w["exc"][i, p.size:] == pi.sentinel(prec.udt)).all()


@PRECS
def test_big_batches_fit_their_tight_exception_stride(oracles, prec):
    """a condition on the inputs, checked here and not on the device: no vector of a batch passed with exc_stride = 64 has more than 64 exceptions, under any
    state it is run with"""
    o = oracles[prec.bits]
    x, states = pi.alp_patterns(prec), pi.alternating_states(o, prec)
    assert x.shape[0] % 2 == 1 and 33 <= x.shape[0] <= 70
    assert [int(s["k"] > 1) for s in states] == [1, 0, 1, 0, 1, 0] and all(s["scheme"] == pi.SCHEME_ALP for s in states)
    w = pi.encode_values_expectations(o, prec, x, states, pi.BIG_EXC_STRIDE)
    assert int(w["cnt"].max()) <= pi.BIG_EXC_STRIDE and np.unique(w["cnt"]).size >= 10
    assert len(set(zip(w["exp"].tolist(), w["fac"].tolist()))) >= 5
    per_pattern = w["fac"].reshape(x.shape[0], states.size)
    assert any(np.unique(per_pattern[:, s]).size > 1 for s in (0, 2, 4)), "the second-level sampling must choose differently for different patterns"


@PRECS
def test_the_oracle_equals_the_reference_on_the_alp_inputs(oracles, refs, prec):
    o, r = oracles[prec.bits], refs[prec.bits]
    x, pl = pi.alp_placed_vectors(prec)
    e, f = pi.ALP_PLACED_EF[prec.bits]
    rows = [(v, e, f) for v in x]
    vecs = pi.boundary_vectors(prec)
    pairs = [q for q in prec.ef if not (prec.bits == 32 and q[1] == 10)]  # the reference reads past its table at the float f = 10
    rows += [(v, *pairs[(7 * i + j) % len(pairs)]) for i, v in enumerate(vecs) for j in range(12)]
    for v, e, f in rows:
        a, b = o.encode_simdized(v, f, e), r.encode_simdized(v, f, e)
        assert a[3] == b[3] and np.array_equal(a[0], b[0]) and np.array_equal(a[2][:a[3]], b[2][:a[3]]), (e, f)
        assert np.array_equal(a[1][:a[3]].view(prec.udt), b[1][:a[3]].view(prec.udt)), (e, f)
        assert o.analyze_ffor(a[0]) == r.analyze_ffor(a[0]), (e, f)
    rows = pi.edge_integer_rows(prec)
    for i, (e, f) in enumerate(prec.ef):
        if prec.bits == 32 and f == 10:
            continue
        packed = pi.oracle_ffor(o, prec.bits, rows[i], prec.bits, 12345)
        assert np.array_equal(o.falp(packed, prec.bits, 12345, f, e).view(prec.udt), r.unffor_decode(packed, prec.bits, 12345, f, e).view(prec.udt)), (e, f)


@PRECS
def test_every_pair_inputs(oracles, prec):
    o = oracles[prec.bits]
    assert len(prec.ef) == (190 if prec.bits == 64 else 66) and len(set(prec.ef)) == len(prec.ef) and all(f <= e <= prec.max_e for e, f in prec.ef)
    rows = pi.edge_integer_rows(prec)
    assert rows.shape == (len(prec.ef), VEC)
    mant = 53 if prec.bits == 64 else 24
    for i, (e, f) in enumerate(prec.ef):
        have = set(int(q) for q in rows[i])
        wrap = (1 << (prec.bits - 1)) // 10**f
        need = {0, 1, -1, prec.imin, prec.imax, 2**mant, 2**mant + 1, 2**mant - 1, -(2**mant), 1 - 2**mant, -1 - 2**mant}
        need |= {q for d in (-1, 0, 1) for q in (wrap + d, -(wrap + d)) if prec.imin <= q <= prec.imax}
        need |= {s * 10**k for k in range(19 if prec.bits == 64 else 10) for s in (1, -1)}
        assert need <= have, (e, f, sorted(need - have)[:4])
    vecs = pi.boundary_vectors(prec)
    assert vecs.shape[0] >= 14 and vecs.dtype == prec.fdt
    # decode + patch of the oracle's encoding gives the input bits back: what the GPU test asserts of the kernels holds of the inputs
    for v in vecs:
        for e, f in prec.ef[::7]:
            enc, exc, pos, cnt = o.encode_simdized(v, f, e)
            out = np.zeros(VEC, prec.fdt)
            o.fn("decode")(pi._p(enc), C.c_int(f), C.c_int(e), pi._p(out))
            o.fn("patch")(pi._p(out), pi._p(exc), pi._p(pos), C.c_uint16(cnt))
            assert np.array_equal(out.view(prec.udt), v.view(prec.udt)), (e, f)
    if prec.bits == 64:
        vals = pi.unique_boundary_values()
        assert vals.size > 1500 and np.unique(vals.view(np.uint64)).size == vals.size


@PRECS
def test_rd_states_cover_every_cut_and_dictionary_size(prec):
    st = pi.rd_states(prec)
    assert tuple(st["rd_rbw"].tolist()) == prec.cuts and len(prec.cuts) == 16 and set(st["rd_dict_size"].tolist()) == set(range(1, 9))
    for s in st:
        ds, lbits = int(s["rd_dict_size"]), prec.bits - int(s["rd_rbw"])
        assert np.unique(s["rd_dict"][:ds]).size == ds and (s["rd_dict"][:ds] < 2**lbits).all() and ds < 2**lbits and not s["rd_dict"][ds:].any()
        assert s["scheme"] == pi.SCHEME_ALP_RD and s["rd_lbw"] == max(1, int(np.ceil(np.log2(ds))))
    assert len({tuple(s["rd_dict"]) for s in st}) == 16


def rd_gpu_batches(prec):
    """the ALP_RD batches of the GPU file, built the same way"""
    states = pi.rd_states(prec)
    pl = [p for _, p in pi.placements(prec, seed=41, counts=(0, 1, 63, 64, 65, 1024))]
    order = np.random.default_rng(42).permutation(len(pl) * len(prec.cuts))
    every = pi.rd_batch(prec, states, order % len(prec.cuts), [pl[i // len(prec.cuts)] for i in order], seed=43)
    big_pl = [p for _, p in pi.placements(prec, seed=22, counts=(0, 1, 63, 64, 2, 33)) if p.size <= pi.BIG_EXC_STRIDE]
    big = pi.rd_batch(prec, states, [i % len(prec.cuts) for i in range(33)], [big_pl[i % len(big_pl)] for i in range(33)], seed=23)
    return states, every, big, pl


@PRECS
def test_rd_restatements_are_the_oracles_on_the_gpu_batches(oracles, prec):
    o = oracles[prec.bits]
    states, every, big, pl = rd_gpu_batches(prec)
    assert int(big["cnt"].max()) <= pi.BIG_EXC_STRIDE and set(big["state_idx"].tolist()) == set(range(16))
    seen = set()
    for b in (every, big):
        for i in range(b["cnt"].size):
            rec, c = states[int(b["state_idx"][i])], int(b["cnt"][i])
            right, left, exc, pos, cnt = pi.oracle_rd_encode(o, prec, rec, b["bits"][i].view(prec.fdt))
            assert cnt == c and np.array_equal(right, b["right"][i]) and np.array_equal(left, b["left"][i])
            assert np.array_equal(exc[:c], b["exc"][i, :c]) and np.array_equal(pos[:c], b["pos"][i, :c])
            assert (b["left"][i, b["pos"][i, :c]] == rec["rd_dict_size"]).all() and (np.delete(b["left"][i], b["pos"][i, :c]) < rec["rd_dict_size"]).all()
            for at_exc in (None, 8, 0xFFFF):
                l = b["left"][i].copy()
                if at_exc is not None:
                    l[b["pos"][i, :c]] = at_exc
                assert np.array_equal(pi.rd_decode_np(prec, rec, b["right"][i], l, b["exc"][i], b["pos"][i], c), b["bits"][i])
                if at_exc is None:
                    assert np.array_equal(pi.oracle_rd_decode(o, prec, rec, right, l, exc, pos, c).view(prec.udt), b["bits"][i])
            seen.add((int(rec["rd_rbw"]), c))
    for cut in prec.cuts:
        assert {c for r, c in seen if r == cut} >= {0, 1, 63, 64, 65, 1024, 16, 512}, cut
    assert sorted(p.size for p in pl) == sorted([0, 1, 63, 64, 65, 1024, 2, 64, 64, 64, 16, 16, 16, 512, 512])


@PRECS
def test_rd_restatements_on_columns_the_oracle_encodes_itself(oracles, prec):
    """columns of vectors built under four of the states, encoded by the oracle's own search: whatever cut and dictionary it chooses, the restatement under that
    state gives the oracle's right parts and exception lists, and the oracle's decode gives the column back"""
    o = oracles[prec.bits]
    states = pi.rd_states(prec)
    rng = np.random.default_rng(51)
    pl = [p for _, p in pi.placements(prec, seed=52, counts=(0, 1, 5, 64))]
    unffor = o.unffor_u64 if prec.bits == 64 else o.unffor_u32
    checked = 0
    for si in (0, 5, 9, 13):
        col = np.stack([pi.rd_vector(prec, states[si], pl[v % len(pl)] if pl[v % len(pl)].size <= 64 else pl[0], rng) for v in range(24)])
        enc = o.encode_column(col.view(prec.fdt).reshape(-1))
        assert np.array_equal(o.decode_column(enc).view(prec.udt), col.reshape(-1))
        if enc["scheme"][0] != pi.SCHEME_ALP_RD:
            continue
        rec = np.zeros(1, pi.STATE_DTYPE)[0]
        rec["scheme"], rec["rd_rbw"], rec["rd_lbw"], rec["rd_dict_size"], rec["rd_dict"] = pi.SCHEME_ALP_RD, enc["bw"][0], enc["lbw"][0], enc["dict_size"][0], enc["dict"][0]
        for v in range(col.shape[0]):
            right, left, exc, pos, cnt = pi.rd_encode_np(prec, col[v], rec)
            assert cnt == enc["exc_cnt"][v] and np.array_equal(pos, enc["pos"][v, :cnt]) and np.array_equal(exc, enc["exc"][v].view(np.uint16)[:cnt])
            assert np.array_equal(right, unffor(enc["packed"][v], int(enc["bw"][v]), 0))
            got_left = oracles[16].unffor_u16(enc["packed_left"][v], int(enc["lbw"][v]), 0)
            keep = np.setdiff1d(np.arange(VEC), pos)
            assert np.array_equal(got_left[keep], left[keep])
            assert np.array_equal(pi.rd_decode_np(prec, rec, right, got_left, exc, pos, cnt), col[v])
            checked += 1
    assert checked >= 24, "at least one of the columns must come out as ALP_RD"
