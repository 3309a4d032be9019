"""GPU: the ALP_RD half of the rowgroup search (k_rowgroup_init: cut choice, dictionary, the replay of libstdc++'s containers in
rd_dictionary_order.hpp) and the encoders' dictionary and map-position lookups, bit for bit against the oracle and the recorded answers of the real
reference (tests/golden/rd_search_samples.npz), on the inputs of rd_search_inputs.py.  tests/test_rd_search_cpu.py shows what those inputs reach
(every cut, dictionary size and left width; up to 288 distinct left parts, every rehash of the node list, both forms of the sort; ties across the
dictionary's 8th place) and pins the oracle to the reference on them.  No result of the GPU is ever the expectation of another.

  1. the search on sample sets handed in directly: the chosen state and all 16 forced cuts, state bytes and estimates
  2. rowgroup init through columns: states, the d_rd_order tables, ALP rowgroups' rows
  3. every encode route on those columns, whole streams; a column without the table; decode
  4. many rowgroups of different cuts and sizes in one launch, and 1024 of them (the search runs beside the encode)"""
import functools

import numpy as np
import pytest
import torch

import datagen
import layout
import rd_search_golden
import rd_search_inputs as inputs
import test_encode_gpu as te

pytestmark = pytest.mark.gpu
BITS = [64, 32]
PARTS = ("rowgroup states", "descriptors", "packed stream", "exception stream")
ROUTES = ["single_pass", "two_pass", "classic_kernel", "unordered", "given_states"]
STRIDE = 296  # ALPGPU_RD_ORDER_STRIDE


def _oracle(bits):
    from oracle.pyoracle import Oracle, OracleF32
    return Oracle() if bits == 64 else OracleF32()


def _dtype(bits):
    return "f64" if bits == 64 else "f32"


def _int_view(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _state_record(ans):
    """the 32-byte rowgroup state of an ALP_RD answer (rd_state_from_samples): scheme, widths, size, dictionary, zeros everywhere else"""
    from alp_amd import capi
    st = np.zeros(1, capi.ROWGROUP_DTYPE)
    st["scheme"], st["rd_rbw"], st["rd_lbw"], st["rd_dict_size"], st["rd_dict"] = capi.SCHEME_ALP_RD, ans["rbw"], ans["lbw"], ans["dict_size"], ans["dict"]
    return st.view(np.uint8)


# ---- expectations, computed once ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _columns(bits):
    """{name: column}: all 100-vector cases as the rowgroups of one column, the shorter columns of (c), and ALP rowgroups between ALP_RD ones"""
    cols = inputs.columns(bits)
    out = {"joined": inputs.joined_column(bits)}
    out.update({nm: a for nm, a in cols.items() if a.size != 100 * 1024})
    alp = datagen.decimal_column(200, 2, seed=41) if bits == 64 else datagen.decimal_column_f32(200, 2, seed=41)
    out["alp_between"] = np.concatenate([alp[:102400], cols["distinct_k21_rnd"], alp[102400:], cols["ladder_k3_m300"], cols["ties_t12_c1_v25"]])
    return out


@functools.lru_cache(maxsize=None)
def expected(bits, name):
    """(compact column of the oracle's encoding, the d_rd_order rows the search must write: count, entries, zeros)"""
    orc = _oracle(bits)
    col = _columns(bits)[name]
    enc = orc.encode_column(col)
    want = layout.compact(enc, bits // 8)
    rows = np.zeros((want[0].size, STRIDE), np.uint16)
    for r in np.nonzero(want[0]["scheme"] == 1)[0]:
        srt = orc.rd_state_from_samples(inputs.samples_of(col, r))["sorted"]
        rows[r, 0], rows[r, 1:1 + srt.size] = srt.size, srt
    return want, rows


def _upload(bits, name):
    return torch.from_numpy(_columns(bits)[name].copy()).cuda()  # (the shared arrays are read-only)


def _assert_column(dcol, want, what):
    for a, b, part in zip(dcol.to_host(), want, PARTS):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: {part} differ from the oracle's"


def _table(dcol):
    return dcol.rd_order.cpu().numpy().view(np.uint16).reshape(-1, STRIDE)


# =====================================================================================================================================================
# 1. the search on sample sets handed in directly
# =====================================================================================================================================================
@pytest.mark.parametrize("bits", BITS)
def test_search_on_direct_samples_every_cut(ctx, bits):
    """alpgpu_rd_state_from_samples_* and alpgpu_rd_dictionary_for_cut_* at each of the 16 cuts on every sample set of (d): the whole 32-byte state
    (scheme, widths, size, the dictionary entry by entry, zeros behind it) and the estimate (== on the double) are the oracle's and, for the built
    families, the recorded reference's; the chosen cut is the first strictly smallest of the 16 estimates."""
    from alp_amd import capi
    orc = _oracle(bits)
    sets = inputs.sample_sets(bits)
    fixture = rd_search_golden.cases(bits)
    names = list(sets)
    offs = np.concatenate([[0], np.cumsum([sets[nm].size for nm in names])])
    d_smp = torch.from_numpy(np.concatenate([sets[nm] for nm in names])).cuda()
    states = torch.zeros((len(names), 17, 32), dtype=torch.uint8, device="cuda")
    ests = torch.zeros((len(names), 17), dtype=torch.float64, device="cuda")
    for i in range(len(names)):
        smp = d_smp[offs[i]:offs[i + 1]]
        ctx.state_from_samples(smp, states[i, 0], rd_only=True)
        for cut in range(1, 17):
            ctx.rd_dictionary_for_cut(smp, bits - cut, states[i, cut], ests[i, cut:cut + 1])
    ctx.synchronize()
    states, ests = states.cpu().numpy(), ests.cpu().numpy()
    for i, nm in enumerate(names):
        for cut in range(17):
            want = orc.rd_state_from_samples(sets[nm], cut)
            if nm in fixture:
                assert rd_search_golden.same_answer(want, fixture[nm][1][cut]), (nm, cut)
            assert np.array_equal(states[i, cut], _state_record(want)), (f"{nm}, cut {cut or 'chosen'}: state {states[i, cut].tolist()} != "
                                                                         f"rbw {want['rbw']} lbw {want['lbw']} size {want['dict_size']} dict {want['dict']}")
            if cut:
                assert ests[i, cut] == want["estimate"], (nm, cut, ests[i, cut], want["estimate"])
        first_smallest = 1 + int(np.argmin(ests[i, 1:]))
        assert int(states[i, 0].view(capi.ROWGROUP_DTYPE)["rd_rbw"][0]) == bits - first_smallest, f"{nm}: chosen right width against the first strictly smallest estimate (cut {first_smallest})"


# =====================================================================================================================================================
# 2. rowgroup init through a column
# =====================================================================================================================================================
@pytest.mark.parametrize("bits", BITS)
def test_rowgroup_init_states_and_sorted_order_tables(ctx, bits):
    """alpgpu_rowgroup_init_* on every column of (a) to (c): rowgroup states byte for byte; d_rd_order holds, per ALP_RD rowgroup, the count and the
    distinct sampled left parts in the reference's sorted order and nothing behind them; an ALP rowgroup's row gets a zero count and is otherwise
    left as it was"""
    from alp_amd import capi
    for name, col_np in _columns(bits).items():
        want, rows = expected(bits, name)
        x = _upload(bits, name)
        dcol = capi.DeviceColumn(col_np.size // 1024, dtype=_dtype(bits))
        dcol.rd_order.fill_(0x5A5A)
        ctx.rowgroup_init(x, dcol)
        ctx.synchronize()
        got_rg = dcol.rowgroups.cpu().numpy()[: want[0].size * 32]
        assert np.array_equal(got_rg, want[0].view(np.uint8)), f"{name}: rowgroup states differ in rowgroups {np.nonzero((got_rg.reshape(-1, 32) != want[0].view(np.uint8).reshape(-1, 32)).any(axis=1))[0][:8]}"
        tab = _table(dcol)
        for r in range(want[0].size):
            n = int(rows[r, 0])
            assert tab[r, 0] == n and np.array_equal(tab[r, 1:1 + n], rows[r, 1:1 + n]), f"{name}: sorted order of rowgroup {r} (D = {n})"
            assert (tab[r, 1 + n:] == 0x5A5A).all(), f"{name}: rowgroup {r}: words behind the table's entries were written"
    assert (expected(bits, "alp_between")[0][0]["scheme"] == [2, 1, 2, 1, 1]).all()


# =====================================================================================================================================================
# 3. every encode route
# =====================================================================================================================================================
def _encode(ctx, bits, route, x, want, rows):
    from alp_amd import capi
    dcol = capi.DeviceColumn(x.numel() // 1024, dtype=_dtype(bits))
    option = {"two_pass": (capi.OPT_ENCODE_TWO_PASS, 1), "classic_kernel": (capi.OPT_ENCODE_KERNEL, 1), "unordered": (capi.OPT_ENCODE_UNORDERED, 1)}.get(route)
    try:
        if option:
            ctx.set_option(*option)
        if route == "given_states":  # the oracle's states and its sorted-order table, as a caller may supply them
            dcol.rowgroups[: want[0].size * 32] = torch.from_numpy(want[0].view(np.uint8).reshape(-1)).cuda()
            dcol.rd_order[: rows.size] = torch.from_numpy(rows.view(np.int16).reshape(-1)).cuda()
            ctx.encode_vectors(x, dcol)
        else:
            ctx.encode(x, dcol)
        ctx.synchronize()
    finally:
        if option:
            ctx.set_option(option[0], 0)
    return dcol


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("bits", BITS)
def test_every_encode_route_writes_the_oracles_streams(ctx, bits, route):
    """every column of (a) to (c) through every route the library has: rowgroup states, descriptors, packed stream (right parts and left indices,
    the map positions at exception slots included) and exception stream equal layout.compact(oracle) byte for byte; the unordered route writes the
    same records elsewhere (compared per vector, and the records tile the streams); the decode of each is the input, bit for bit"""
    W = bits // 8
    for name in _columns(bits):
        want, rows = expected(bits, name)
        x = _upload(bits, name)
        dcol = _encode(ctx, bits, route, x, want, rows)
        pb, eb, ov = ctx.column_totals(dcol)
        assert ov == 0
        if route == "unordered":
            rg, vec, packed, exc = dcol.to_host()
            assert np.array_equal(rg.view(np.uint8), want[0].view(np.uint8)), f"{name}: rowgroup states"
            got, exp = layout.expand(rg, vec, packed, exc, W), layout.expand(*want, W)
            for k in ("scheme", "e", "f", "bw", "lbw", "base", "exc_cnt", "packed", "packed_left", "pos"):
                assert np.array_equal(got[k], exp[k]), f"{name}: {k} differ from the oracle's"
            assert np.array_equal(got["exc"].view(np.uint8), exp["exc"].view(np.uint8)), f"{name}: exception values"
            te._assert_records_tile_the_streams(vec, pb, eb, W)
        else:
            _assert_column(dcol, want, f"{name}, {route}")
            assert (pb, eb) == (want[2].size, want[3].size)
        out = ctx.decode(dcol)
        ctx.synchronize()
        assert torch.equal(_int_view(out), _int_view(x)), f"{name}, {route}: decode(encode(x)) differs from the input bits"


@pytest.mark.parametrize("bits", BITS)
def test_column_without_the_sorted_order_table(ctx, bits):
    """DeviceColumn(rd_order=False): d_rd_order is absent.  DESIGN.md 3.3: rowgroup states, descriptors, right parts, exception records and every
    left index a decoder reads are the same; the exception slots' left indices (which no decoder reads) carry the dictionary size instead of the
    reference's map position — as FFOR packs it, its low left-width bits."""
    from alp_amd import capi
    orc, u16 = _oracle(bits), _oracle(64)  # (the 16-bit FFOR of the left indices is the same code for both precisions)
    W = bits // 8
    cols = inputs.columns(bits)
    names = [nm for nm in inputs.rowgroup_cases(bits) if not nm.startswith("ladder_") or nm.split("_")[1] in ("k0", "k5", "k11")]
    col_np = np.concatenate([cols[nm] for nm in names])
    enc = orc.encode_column(col_np)
    slots_changed = 0
    for v in range(enc["scheme"].size):  # the expectation: the oracle's left indices with the dictionary size at every exception slot
        c, lbw, ds = int(enc["exc_cnt"][v]), int(enc["lbw"][v]), int(enc["dict_size"][v // 100])
        if c:
            left = u16.unffor_u16(enc["packed_left"][v], lbw)
            slots_changed += int((left[enc["pos"][v, :c]] != (ds & ((1 << lbw) - 1))).sum())
            left[enc["pos"][v, :c]] = ds
            enc["packed_left"][v] = 0
            enc["packed_left"][v, :64 * lbw] = u16.ffor_u16(left, lbw)[:64 * lbw]
    assert slots_changed > 1000, "the columns must hold exception slots whose map position differs from the dictionary size"
    want = layout.compact(enc, W)
    x = torch.from_numpy(col_np).cuda()
    dcol = capi.DeviceColumn(col_np.size // 1024, dtype=_dtype(bits), rd_order=False)
    ctx.encode(x, dcol)
    ctx.synchronize()
    _assert_column(dcol, want, "no d_rd_order")
    out = ctx.decode(dcol)
    ctx.synchronize()
    assert torch.equal(_int_view(out), _int_view(x))


# =====================================================================================================================================================
# 4. 1024 rowgroups: the search runs beside the encode
# =====================================================================================================================================================
def _tiled(want, rows, n_rowgroups):
    """the compact column and table of a column whose rowgroup r is rowgroup r % len(rows) of the column `want` describes"""
    rg, vec, packed, exc = want
    base, reps, tail = rg.size, n_rowgroups // rg.size, n_rowgroups % rg.size
    p_tail = int(vec["packed_off"][tail * 100]) if tail else 0
    e_tail = int(vec["exc_off"][tail * 100]) if tail else 0
    vs = []
    for i in range(reps + (1 if tail else 0)):
        v = vec[: tail * 100].copy() if i == reps else vec.copy()
        v["packed_off"] += np.uint64(i * packed.size)
        v["exc_off"] += np.uint64(i * exc.size)
        vs.append(v)
    assert base * 100 == vec.size, "whole rowgroups only"
    return (np.concatenate([rg] * reps + [rg[:tail]]), np.concatenate(vs), np.concatenate([packed] * reps + [packed[:p_tail]]),
            np.concatenate([exc] * reps + [exc[:e_tail]])), np.concatenate([rows] * reps + [rows[:tail]])


@pytest.mark.parametrize("bits", BITS)
def test_1024_rowgroups_of_every_cut_and_size_search_beside_the_encode(ctx, bits):
    """the 100-vector cases repeated to 1024 rowgroups: from that length on alpgpu_encode_f64 runs the search as a persistent kernel beside the
    vector encode (alpgpu.h, ALPGPU_OPT_ENCODE_ASYNC_INIT; float columns with the option at 2), whose workgroups walk rowgroups of different cuts
    and dictionary sizes one after the other over the same LDS.  States, tables and streams are the oracle's rowgroups repeated."""
    from alp_amd import capi
    want1, rows1 = expected(bits, "joined")
    n_rg = 1024
    want, rows = _tiled(want1, rows1, n_rg)
    x1 = _upload(bits, "joined")
    base = want1[0].size
    x = torch.cat([x1] * (n_rg // base) + [x1[: (n_rg % base) * 102400]])
    del x1
    assert x.numel() == n_rg * 102400
    try:
        if bits == 32:
            ctx.set_option(capi.OPT_ENCODE_ASYNC_INIT, 2)
        dcol = capi.DeviceColumn(n_rg * 100, dtype=_dtype(bits))
        ctx.encode(x, dcol)
        ctx.synchronize()
    finally:
        ctx.set_option(capi.OPT_ENCODE_ASYNC_INIT, 1)
    _assert_column(dcol, want, "1024 rowgroups")
    assert np.array_equal(_table(dcol), rows), "sorted-order tables"
    out = ctx.decode(dcol)
    ctx.synchronize()
    assert torch.equal(_int_view(out), _int_view(x))
