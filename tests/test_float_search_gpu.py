"""GPU: the float (e,f) search and encode on their decision boundaries, bit for bit against the float oracle (oracle/pyoracle.py: OracleF32; pinned to the
reference on exactly these inputs by tests/test_float_search_cpu.py, which also checks that the inputs are what they claim to be).  Everything goes through
the C ABI, no result of the GPU is ever the expectation of another, and everything is compared on uint32 / int32 views (-0.0, NaN payloads, INT32_MIN).

The float arithmetic restates what one Clang build of the reference does where C++ leaves it undefined (alp_device_f32.hpp, U1..U4): the conversion's range
test and its INT32_MIN, four separately rounded operations around 1.5 * 2^23, a 32-bit product that wraps, 10^10 mod 2^32 for the (10,10) candidate.
datagen.search_boundary_values_f32 puts values on each of these; search_boundary_mixtures_f32 mixes them into vectors so that exception counts and
ranges decide.

  1. encode_value of every value under all 66 (e,f); decode_values_f32 and falp_f32 of integers on the product's wrap under all 66, f = 10 included
  2. the search: one constant sample set per value (the first candidate that fits, or ALP_RD), which reaches 65 of the 66 candidates — among them (0,0)
     and (1,0), the two that k_rowgroup_init<PrecF32> evaluates "on their side" (init_kernels.hip)
  3. the mixtures as whole streams through every encode route, their decode in every staged and direct launch shape, and the per-vector route
     (second_level_select_f32)"""
import ctypes as C

import numpy as np
import pytest
import torch

import datagen
import layout
import test_encode_gpu as te
import test_float_gpu as tf
from test_float_search_cpu import ALL_EF, column_of_samples, describe, tail_threshold_sample_sets, unique_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEEDS = list(range(60))
PARTS = ("rowgroup states", "descriptors", "packed stream", "exception stream")


@pytest.fixture(scope="module")
def of32():
    from oracle.pyoracle import OracleF32
    return OracleF32()


@pytest.fixture(scope="module")
def values():
    return unique_bits(datagen.search_boundary_values_f32())


@pytest.fixture(scope="module")
def mixtures(of32):
    """(column, the oracle's encoding of it) per seed, computed once"""
    cols = [datagen.search_boundary_mixtures_f32(seed) for seed in SEEDS]
    return [(c, of32.encode_column(c)) for c in cols]


def show_state(s):
    if s["scheme"] == 2:
        return f"ALP k={int(s['k'])} combos={s['combos'][:2 * int(s['k'])].tolist()}"
    return f"ALP_RD rbw={int(s['rd_rbw'])} lbw={int(s['rd_lbw'])} dict={s['rd_dict'][:int(s['rd_dict_size'])].tolist()}"


# =====================================================================================================================================================
# 1. the scalar arithmetic
# =====================================================================================================================================================
def test_encode_value_of_every_boundary_value_under_every_candidate(ctx, of32, values):
    """alpgpu_encode_value_f32: (v * 10^e) * 10^-f, + magic, - magic, each rounded to float, then the conversion as x86 executes it.  The SAFE form does not
    exist for float as the reference is built (U1), so `safe` changes nothing"""
    x = torch.from_numpy(values).to(DEV)
    got = {(e, f, safe): ctx.encode_value(x, f, e, safe=safe) for e, f in ALL_EF for safe in (True, False)}
    ctx.synchronize()
    enc = of32.fn("encode_value", C.c_int32)
    cv = [C.c_float(float(v)) for v in values]
    for e, f in ALL_EF:
        want = np.array([enc(c, C.c_int(f), C.c_int(e)) for c in cv], np.int32)
        for safe in (True, False):
            g = got[(e, f, safe)].cpu().numpy()
            bad = np.nonzero(g != want)[0]
            assert bad.size == 0, (f"encode_value(e={e}, f={f}, safe={safe}): {bad.size} values differ from the oracle; (value, got, want): "
                                   f"{[(describe(values[i]), int(g[i]), int(want[i])) for i in bad[:6]]}")
        assert torch.equal(got[(e, f, True)], got[(e, f, False)])


def wrap_rows():
    """one row of 1024 int32 per (e,f): 0, +-1, the int32 ends, the integers around 2^31 / 10^f and 2^32 / 10^f (times 10^f they sit on the wrap of the 32-bit
    product), then a seeded fill: half of it anywhere in int32, half within twice 2^32 / 10^f"""
    rng = np.random.default_rng(2024)
    rows = np.empty((len(ALL_EF), 1024), np.int32)
    for i, (e, f) in enumerate(ALL_EF):
        head = [0, 1, -1, -2**31, 2**31 - 1]
        for lim in (2**31, 2**32):
            for d in (-1, 0, 1):
                r = lim // 10**f + d
                head += [r, -r]
        head = np.array(head, np.int64)
        near = rng.integers(-2 * (2**32 // 10**f) - 2, 2 * (2**32 // 10**f) + 3, 512)
        far = rng.integers(-2**31, 2**31, 1024 - 512 - head.size)
        rows[i] = np.concatenate([head, near, far]).astype(np.uint32).view(np.int32)  # wrapped to int32
    return rows


def test_decode_values_and_falp_at_every_candidate(ctx, of32):
    """alpgpu_decode_values_f32 and alpgpu_falp_f32: float(int32(uint32(enc) * 10^f)) * 10^-e with the product wrapping modulo 2^32, and 10^10 mod 2^32 as the
    multiplier of f = 10 (the reference reads past its table there, U4: both sides use the same number)"""
    rows = wrap_rows()
    n = rows.shape[0]
    exp = np.array([e for e, f in ALL_EF], np.uint8)
    fac = np.array([f for e, f in ALL_EF], np.uint8)
    assert fac.max() == 10 and len(set(ALL_EF)) == 66
    dec = of32.fn("decode_value", C.c_float)
    want = np.array([[dec(C.c_int32(int(q)), C.c_int(int(f)), C.c_int(int(e))) for q in row] for row, (e, f) in zip(rows, ALL_EF)], np.float32).view(np.uint32)
    d_enc, d_fac, d_exp = tf.cu(rows), tf.cu(fac), tf.cu(exp)
    d_out = torch.zeros((n, 1024), dtype=torch.float32, device=DEV)
    ctx.decode_values_f32(d_enc, d_out, d_fac, d_exp)
    geom = [of32.analyze_ffor(row) for row in rows]
    bws, bases = np.array([g[0] for g in geom], np.uint8), np.array([g[1] for g in geom], np.int32)
    packed = np.stack([of32.ffor_u32(row, int(bw), int(base)) for row, bw, base in zip(rows, bws, bases)])
    d_out2 = torch.zeros((n, 1024), dtype=torch.float32, device=DEV)
    ctx.falp_f32(tf.cu(packed.view(np.int32)), d_out2, tf.cu(bws), tf.cu(bases), d_fac, d_exp)
    ctx.synchronize()
    for what, out in (("decode_values_f32", d_out), ("falp_f32", d_out2)):
        got = out.cpu().numpy().view(np.uint32)
        r, c = np.nonzero(got != want)
        assert r.size == 0, (f"{what}: {r.size} values differ from the oracle; (e, f, enc, got bits, want bits): "
                             f"{[(*ALL_EF[i], int(rows[i, j]), hex(int(got[i, j])), hex(int(want[i, j]))) for i, j in list(zip(r, c))[:6]]}")


# =====================================================================================================================================================
# 2. the search
# =====================================================================================================================================================
def test_constant_samples_name_the_first_fitting_candidate(ctx, of32, values):
    """alpgpu_state_from_samples_f32 on 32 copies of each value against the state of the oracle's encoding of a constant vector: the first candidate (in the
    reference's order) that round-trips the value, or the ALP_RD cut and dictionary when none does"""
    from alp_amd import capi
    states = torch.zeros((values.size, 32), dtype=torch.uint8, device=DEV)
    smp = torch.from_numpy(np.repeat(values, 32)).to(DEV)
    for i in range(values.size):
        ctx.state_from_samples(smp[32 * i: 32 * i + 32], states[i])
    ctx.synchronize()
    got = states.cpu().numpy().reshape(-1).view(capi.ROWGROUP_DTYPE)
    chosen = set()
    for i, v in enumerate(values):
        w = layout.compact(of32.encode_column(np.full(1024, v, np.float32)), 4)[0][0]
        g = got[i]
        msg = f"value {describe(v)}: GPU {show_state(g)}, oracle {show_state(w)}"
        assert g["scheme"] == w["scheme"], msg
        if w["scheme"] == 2:
            assert g["k"] == w["k"] and np.array_equal(g["combos"], w["combos"]), msg
            chosen.add((int(w["combos"][0]), int(w["combos"][1])))
        else:
            assert g["rd_rbw"] == w["rd_rbw"] and g["rd_lbw"] == w["rd_lbw"] and g["rd_dict_size"] == w["rd_dict_size"], msg
            assert np.array_equal(g["rd_dict"], w["rd_dict"]), msg
    assert {(10, 10), (0, 0), (1, 0)} <= chosen  # (what tests/test_float_search_cpu.py asserts of the inputs; here: that this comparison saw them)


def test_the_sideways_tail_counts_and_ranges_at_the_scheme_threshold(ctx, of32):
    """candidates 64 and 65, (1,0) and (0,0), are evaluated one sample per lane: a ballot counts, a DPP min / max spans (init_kernels.hip).  A constant
    sample set cannot tell a wrong reduction, so: 32 different samples that only the candidate round-trips, 20 / 21 / 22 bits wide with 0 / 1 / 2
    exceptions — on the threshold between ALP and ALP_RD, where one bit or one exception too few changes the scheme —, the minimum at every lane in turn
    (tests/test_float_search_cpu.py: tail_threshold_sample_sets, where the oracle's answers are checked to be the threshold's)"""
    from alp_amd import capi
    sets = tail_threshold_sample_sets(of32)
    states = torch.zeros((len(sets), 32), dtype=torch.uint8, device=DEV)
    smp = torch.from_numpy(np.concatenate([s for *_, s in sets])).to(DEV)
    for i in range(len(sets)):
        ctx.state_from_samples(smp[32 * i: 32 * i + 32], states[i])
    ctx.synchronize()
    got = states.cpu().numpy().reshape(-1).view(capi.ROWGROUP_DTYPE)
    seen = set()
    for g, (cand, bits, n_exc, p, s) in zip(got, sets):
        w = layout.compact(of32.encode_column(column_of_samples(s)), 4)[0][0]
        msg = f"candidate {cand}, {bits} bits, {n_exc} exceptions, minimum at sample {p}: GPU {show_state(g)}, oracle {show_state(w)}"
        assert g["scheme"] == w["scheme"], msg
        if w["scheme"] == 2:
            assert g["k"] == w["k"] and np.array_equal(g["combos"], w["combos"]), msg
        else:
            assert g["rd_rbw"] == w["rd_rbw"] and g["rd_lbw"] == w["rd_lbw"] and g["rd_dict_size"] == w["rd_dict_size"] and np.array_equal(g["rd_dict"], w["rd_dict"]), msg
        seen.add((cand, int(w["scheme"])))
    assert seen == {((0, 0), 1), ((0, 0), 2), ((1, 0), 1), ((1, 0), 2)}


# =====================================================================================================================================================
# 3. the mixtures
# =====================================================================================================================================================
ROUTES = [("single pass", None, 0), ("two pass", "OPT_ENCODE_TWO_PASS", 1), ("async init 1", "OPT_ENCODE_ASYNC_INIT", 1), ("async init 2", "OPT_ENCODE_ASYNC_INIT", 2)]
RESET = {"OPT_ENCODE_TWO_PASS": 0, "OPT_ENCODE_ASYNC_INIT": 1, "OPT_ENCODE_UNORDERED": 0}


def encode_by(ctx, col_np, option, value):
    from alp_amd import capi
    if option is None:
        return tf.gpu_encode(ctx, col_np)
    try:
        ctx.set_option(getattr(capi, option), value)
        return tf.gpu_encode(ctx, col_np)  # (asserts column_totals(...)[2] == 0)
    finally:
        ctx.set_option(getattr(capi, option), RESET[option])


@pytest.mark.parametrize("seed", SEEDS)
def test_mixtures_whole_streams_by_every_route(ctx, mixtures, seed):
    col_np, want = mixtures[seed]
    w_parts = layout.compact(want, 4)
    for route, option, value in ROUTES:
        dcol, x = encode_by(ctx, col_np, option, value)
        assert ctx.column_totals(dcol)[2] == 0
        for a, b, part in zip(dcol.to_host(), w_parts, PARTS):
            if a.size != b.size or not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
                got = layout.expand(*dcol.to_host(), 4)
                tf.assert_parts_equal(got, want, f"seed {seed}, {route}")  # names the field and the vector
                pytest.fail(f"seed {seed}, {route}: {part} differ from the oracle's; rowgroup state GPU {show_state(dcol.to_host()[0][0])}, oracle {show_state(w_parts[0][0])}")
        out = ctx.decode(dcol)
        ctx.synchronize()
        assert torch.equal(out.view(torch.int32), x.view(torch.int32)), f"seed {seed}, {route}: decode(encode(x)) differs from the input bits"


@pytest.mark.parametrize("seed", SEEDS[:10])
def test_mixtures_encoded_unordered(ctx, mixtures, seed):
    """as test_unordered_float_encode_writes_the_same_records_somewhere_else: every record is the oracle's, the records tile the streams"""
    col_np, want = mixtures[seed]
    dcol, x = encode_by(ctx, col_np, "OPT_ENCODE_UNORDERED", 1)
    rg, vec, packed, exc = dcol.to_host()
    got = layout.expand(rg, vec, packed, exc, 4)
    assert np.array_equal(rg.view(np.uint8), layout.compact(want, 4)[0].view(np.uint8)), f"seed {seed}: rowgroup states"
    tf.assert_parts_equal(got, want, f"seed {seed}")
    assert np.array_equal(got["packed_left"], want["packed_left"])
    pb, eb, ov = ctx.column_totals(dcol)
    assert ov == 0
    te._assert_records_tile_the_streams(vec, pb, eb, value_bytes=4)
    out = ctx.decode(dcol)
    ctx.synchronize()
    assert torch.equal(out.view(torch.int32), x.view(torch.int32))


def test_full_rowgroups_of_mixtures_with_the_search_beside_the_encode(ctx, of32):
    """ALPGPU_OPT_ENCODE_ASYNC_INIT = 2 takes effect from 1024 rowgroups on (tests/test_async_init_gpu.py), so the 25-vector columns above never reach the
    persistent search.  Here: four full rowgroups of mixtures (100 vectors each, nine sampled vectors with a decimal exponent of their own, so the
    search keeps k = 5 candidates), repeated 262 times in HBM; the expectation is the oracle's encoding of the period, tiled (as
    tests/test_float_widths_gpu.py: test_every_width_column_with_the_search_beside_the_encode)"""
    from alp_amd import capi
    period = np.concatenate([datagen.search_boundary_mixtures_f32(seed, n_vectors=100) for seed in range(4)])
    reps = 262
    want = of32.encode_column(period)
    assert (want["scheme"] == 2).all() and (want["k"] == 5).all() and len({tuple(c) for c in want["combos"].tolist()}) == 4
    w_rg, w_vec, w_packed, w_exc = layout.compact(want, 4)
    x = torch.from_numpy(period).to(DEV).repeat(reps).contiguous()
    n = 400 * reps
    assert n // 100 >= 1024
    ctx.set_option(capi.OPT_ENCODE_ASYNC_INIT, 2)
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
    bad = np.nonzero((rg.view(np.uint8).reshape(-1, 32) != np.tile(w_rg, reps).view(np.uint8).reshape(-1, 32)).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} rowgroup states differ, first {int(bad[0])}: GPU {show_state(rg[bad[0]])}, oracle {show_state(w_rg[bad[0] % 4])}"
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


@pytest.mark.parametrize("vpw", [0, 1, 2, 4, 8])
def test_decode_of_the_oracles_mixtures_in_every_launch_shape(ctx, mixtures, vpw):
    """encoder-made vectors with f up to 10, bases at the int32 ends and 1024 exceptions, which the hand-built rows of tests/float_rows.py do not combine"""
    from alp_amd import capi
    cols = [capi.DeviceColumn.from_host(*layout.compact(want, 4), dtype="f32") for _, want in mixtures[:10]]
    try:
        ctx.set_option(capi.OPT_DECODE_VECTORS_PER_WG, vpw)
        outs = [ctx.decode(c) for c in cols]
        ctx.synchronize()
    finally:
        ctx.set_option(capi.OPT_DECODE_VECTORS_PER_WG, 0)
    for seed, ((col_np, want), out) in enumerate(zip(mixtures[:10], outs)):
        got = out.cpu().numpy().view(np.uint32)
        bad = np.nonzero(got != col_np.view(np.uint32))[0]
        assert bad.size == 0, (f"seed {seed}, shape {vpw}: {bad.size} values differ; (vector, position, e, f, bw, base, exc_cnt, got, want): "
                               f"{[(int(i) // 1024, int(i) % 1024, *(int(want[k][i // 1024]) for k in ('e', 'f', 'bw', 'base', 'exc_cnt')), describe(got[i:i + 1].view(np.float32)[0]), describe(col_np[i])) for i in bad[:4]]}")


def test_per_vector_route_chooses_the_oracles_candidate(ctx, of32, mixtures):
    """alpgpu_encode_values_f32 with the oracle's rowgroup states on the ALP vectors of seeds 0..9: the second-level sampling (second_level_select_f32)
    must arrive at the oracle's (e,f) per vector, and the encoding under it at the oracle's integers and exceptions"""
    from alp_amd import capi
    picked = [(col_np, want) for col_np, want in mixtures[:10] if want["scheme"][0] == 2]
    assert len(picked) >= 5 and all(int(want["k"][0]) > 1 for _, want in picked)
    x = np.concatenate([col_np for col_np, _ in picked]).reshape(-1, 1024)
    states = np.concatenate([layout.compact(want, 4)[0] for _, want in picked])
    idx = np.repeat(np.arange(len(picked), dtype=np.uint32), 25)
    w = {k: np.concatenate([want[k] for _, want in picked]) for k in ("e", "f", "exc_cnt")}
    m = x.shape[0]
    d_exc = torch.zeros((m, 1024), dtype=torch.float32, device=DEV)
    d_pos = torch.zeros((m, 1024), dtype=torch.int16, device=DEV)
    d_cnt = torch.zeros(m, dtype=torch.int16, device=DEV)
    d_enc = torch.zeros((m, 1024), dtype=torch.int32, device=DEV)
    d_fac = torch.zeros(m, dtype=torch.uint8, device=DEV)
    d_exp = torch.zeros(m, dtype=torch.uint8, device=DEV)
    ctx.encode_values_f32(tf.cu(x), tf.cu(states.view(np.uint8)), tf.cu(idx.view(np.int32)), d_exc, d_pos, d_cnt, d_enc, d_fac, d_exp)
    ctx.synchronize()
    fac, exp, cnt = d_fac.cpu().numpy(), d_exp.cpu().numpy(), d_cnt.cpu().numpy().view(np.uint16)
    bad = np.nonzero((fac != w["f"]) | (exp != w["e"]) | (cnt != w["exc_cnt"]))[0]
    assert bad.size == 0, (f"{bad.size} vectors differ; (vector, GPU e f exceptions, oracle e f exceptions, state): "
                           f"{[(int(v), int(exp[v]), int(fac[v]), int(cnt[v]), int(w['e'][v]), int(w['f'][v]), int(w['exc_cnt'][v]), show_state(states[idx[v]])) for v in bad[:6]]}")
    assert len(set(zip(exp.tolist(), fac.tolist()))) >= 8, "the vectors choose among several candidates"
    enc, exc, pos = d_enc.cpu().numpy(), d_exc.cpu().numpy(), d_pos.cpu().numpy().view(np.uint16)
    for v in range(m):
        we, wx, wp, wc = of32.encode_simdized(x[v], int(w["f"][v]), int(w["e"][v]))
        assert wc == cnt[v] and np.array_equal(enc[v], we), f"vector {v} (e={int(exp[v])}, f={int(fac[v])}): encoded integers"
        assert np.array_equal(pos[v, :wc], wp[:wc]) and np.array_equal(exc[v, :wc].view(np.uint32), wx[:wc].view(np.uint32)), f"vector {v}: exceptions"
