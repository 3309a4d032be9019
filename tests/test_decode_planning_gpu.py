"""GPU: the layer that chooses which store-decode kernel runs.  Every launch of alpgpu_decode_f64 / _f32 is planned on the host from state no kernel checks —
the caller-writable size hints of alpgpu_column, the per-segment tables alpgpu_column_totals / alpgpu_column_from_blob leave in the context, the sizes an unhinted
decode learns — and api_decode.hip holds that this state picks launch shapes only: the bytes cannot differ.  These tests hold it to that.

1. A content battery — ALP vectors of every bit width with 0 .. 1024 exceptions (sorted positions that include the first and the last slot, arbitrary bit patterns,
   NaN payloads among them), ALP_RD vectors with 0 .. 1024 exceptions, runs of 0-bit vectors, all of it mixed inside rowgroups — built by hand in the oracle's layout,
   tiled past two plan segments (>= 65 600 vectors), with its records in vector order and out of it.
2. The lie matrix (decode_lies.py): hints that drive every arm of the launch rule (decode_policy.hpp: policy_decode_plan) over that content, with the read-ahead left
   to the library, off and forced on.  Each arm is shown to be the one launched (alpgpu_debug_decode_plan) and writes the oracle's bytes.
3. Stale plans: a region plan or learned sizes applied to other content in the same buffers (a D2D copy, another context's encode).
Everything is compared bit for bit, NaNs included."""
import numpy as np
import pytest
import torch

import layout
from decode_lies import LIES_F32, LIES_F64, TILED_VECTORS, lie_hints

pytestmark = pytest.mark.gpu

EXC_COUNTS = [0, 1, 127, 128, 129, 255, 256, 257, 1023, 1024]
RD_EXC_COUNTS = [0, 511, 512, 513, 1024]  # (2-byte ALP_RD exceptions: staged four times as deep as 8-byte ALP ones)
NAN_PATTERNS = {8: [0x7FF0000000000001, 0x7FF8000000000000, 0xFFF8000000000123, 0x7FFFFFFFFFFFFFFF, 0x8000000000000000, 0x7FF0000000000000],
                4: [0x7F800001, 0x7FC00000, 0xFFC00123, 0x7FFFFFFF, 0x80000000, 0x7F800000]}


@pytest.fixture(scope="module")
def of32():
    from oracle.pyoracle import OracleF32
    return OracleF32()


def _empty(n, vb):
    nrg = (n + 99) // 100
    return dict(scheme=np.full(n, 2, np.uint8), e=np.zeros(n, np.uint8), f=np.zeros(n, np.uint8), bw=np.zeros(n, np.uint8), lbw=np.zeros(n, np.uint8),
                base=np.zeros(n, np.int64), exc_cnt=np.zeros(n, np.uint16),
                packed=np.zeros((n, 1024), np.int64 if vb == 8 else np.int32), packed_left=np.zeros((n, 1024), np.uint16),
                exc=np.zeros((n, 1024), np.float64 if vb == 8 else np.float32), pos=np.zeros((n, 1024), np.uint16),
                dict=np.zeros((nrg, 8), np.uint16), dict_size=np.zeros(nrg, np.uint8), k=np.ones(nrg, np.uint8), combos=np.zeros((nrg, 10), np.int32))


def _positions(rng, c, v):
    """c sorted exception positions; from two on they include slots 0 and 1023 (one alone: either)"""
    if c == 0:
        return np.zeros(0, np.uint16)
    if c == 1:
        return np.array([0 if v % 2 else 1023], np.uint16)
    inner = rng.choice(np.arange(1, 1023), c - 2, replace=False)
    return np.sort(np.concatenate([[0, 1023], inner])).astype(np.uint16)


def _alp_vector(enc, rng, v, bw, c, vb):
    if vb == 8:
        e = int(rng.integers(0, 19)); f = int(rng.integers(0, e + 1))
        enc["base"][v] = int(rng.integers(-2**62, 2**62))
        enc["packed"][v, :16 * bw] = rng.integers(-2**63, 2**63 - 1, 16 * bw, dtype=np.int64)
    else:
        e = int(rng.integers(0, 11)); f = int(rng.integers(0, e + 1))
        enc["base"][v] = int(rng.integers(-2**30, 2**30))
        enc["packed"][v, :32 * bw] = rng.integers(-2**31, 2**31 - 1, 32 * bw, dtype=np.int32)
    enc["scheme"][v], enc["bw"][v], enc["e"][v], enc["f"][v], enc["exc_cnt"][v] = 2, bw, e, f, c
    enc["pos"][v, :c] = _positions(rng, c, v)
    ut = np.uint64 if vb == 8 else np.uint32
    bits = rng.integers(0, 2**(8 * vb), c, dtype=ut)
    nans = np.array(NAN_PATTERNS[vb], ut)
    if v % 2:  # NaN payloads, an infinity and -0.0 among the exception values of every other vector (the even ones keep sums that are numbers)
        bits[: min(c, nans.size)] = nans[: min(c, nans.size)]
    enc["exc"][v, :c] = bits.view(enc["exc"].dtype)


def _rd_rowgroup(enc, rng, r, rbw, lbw, counts, vb):
    """one ALP_RD rowgroup: right words of rbw bits, left indices of lbw bits into a full dictionary of left parts, exceptions that replace left parts"""
    left_bits = 8 * vb - rbw
    enc["dict"][r] = rng.integers(0, 2**left_bits, 8).astype(np.uint16)
    enc["dict_size"][r] = 8
    for i in range(100):
        v = 100 * r + i
        c = counts[i % len(counts)]
        enc["scheme"][v], enc["bw"][v], enc["lbw"][v], enc["exc_cnt"][v] = 1, rbw, lbw, c
        if vb == 8:
            enc["packed"][v, :16 * rbw] = rng.integers(-2**63, 2**63 - 1, 16 * rbw, dtype=np.int64)
        else:
            enc["packed"][v, :32 * rbw] = rng.integers(-2**31, 2**31 - 1, 32 * rbw, dtype=np.int32)
        enc["packed_left"][v, :64 * lbw] = rng.integers(0, 2**16, 64 * lbw).astype(np.uint16)
        enc["pos"][v, :c] = _positions(rng, c, v)
        enc["exc"][v].view(np.uint16)[:c] = rng.integers(0, 2**left_bits, c).astype(np.uint16)


def battery(vb, seed=1):
    """500 distinct vectors in five rowgroups (oracle layout): [0] every ALP width with every exception count, a run of 0-bit vectors and more of both, mixed;
    [1] the widths the other way round with the counts shifted; [2] ALP_RD, narrow left parts; [3] a rowgroup of 0-bit vectors; [4] ALP_RD, wide right parts"""
    rng = np.random.default_rng(seed + vb)
    enc = _empty(500, vb)
    top = 8 * vb
    rg0 = [(bw, EXC_COUNTS[bw % 10]) for bw in range(top + 1)] + [(0, 0)] * 20
    rg0 += [(int(rng.integers(0, top + 1)), EXC_COUNTS[i % 10]) for i in range(100 - len(rg0))]
    rg1 = [(bw, EXC_COUNTS[(bw + 5) % 10]) for bw in range(top, -1, -1)] + [(0, 0)] * 15 + [(0, EXC_COUNTS[i % 10]) for i in range(10)]
    rg1 += [(int(rng.integers(0, top + 1)), EXC_COUNTS[(3 * i) % 10]) for i in range(100 - len(rg1))]
    for r, rows in ((0, rg0), (1, rg1), (3, [(0, 0)] * 100)):
        for i, (bw, c) in enumerate(rows):
            _alp_vector(enc, rng, 100 * r + i, bw, c, vb)
    _rd_rowgroup(enc, rng, 2, 50 if vb == 8 else 22, 3, RD_EXC_COUNTS, vb)
    _rd_rowgroup(enc, rng, 4, 62 if vb == 8 else 30, 1, RD_EXC_COUNTS[::-1], vb)
    return enc


def _reordered(vec, packed, exc, vb, perm):
    """the same column with its records laid into the streams in the order perm (descriptors point to them where they now are)"""
    psz, esz = layout.record_sizes(vec["scheme"], vec["bw"], vec["lbw"], vec["exc_cnt"], vb)
    vec = vec.copy()
    p_parts, e_parts, po, eo = [], [], 0, 0
    for v in perm:
        p0, e0 = int(vec["packed_off"][v]), int(vec["exc_off"][v])
        p_parts.append(packed[p0:p0 + int(psz[v])]); e_parts.append(exc[e0:e0 + int(esz[v])])
        vec["packed_off"][v], vec["exc_off"][v] = po, eo
        po += int(psz[v]); eo += int(esz[v])
    return vec, np.concatenate(p_parts), np.concatenate(e_parts)


class Tiled:
    """a battery tiled to TILED_VECTORS vectors in HBM (the streams repeated on the device), with the oracle's decode of it tiled the same way"""

    def __init__(self, enc, vb, want, ordered=True):
        from alp_amd import capi
        rg, vec, packed, exc = layout.compact(enc, vb)
        if not ordered:  # records out of vector order: rowgroups back to front, within each the odd vectors' records before the even ones'
            perm = [100 * r + i for r in range(rg.size - 1, -1, -1) for i in list(range(1, 100, 2)) + list(range(0, 100, 2))]
            vec, packed, exc = _reordered(vec, packed, exc, vb, perm)
        d = vec.size
        self.k = k = -(-TILED_VECTORS // d)
        self.n = n = d * k
        self.vb, self.enc, self.distinct = vb, enc, d
        tv = np.tile(vec, k)
        rep = np.repeat(np.arange(k, dtype=np.uint64), d)
        tv["packed_off"] += rep * np.uint64(packed.size)
        tv["exc_off"] += rep * np.uint64(exc.size)
        self.packed_bytes, self.exc_bytes = k * packed.size, k * exc.size
        trg = np.tile(rg, k)
        self.rd_rowgroups = int((trg["scheme"] == capi.SCHEME_ALP_RD).sum())
        # capacities with room for every lie below (a real column of this length could carry any of them)
        col = capi.DeviceColumn(n, packed_capacity=max(self.packed_bytes + 1024, 64 * 128 * n), exc_capacity=max(self.exc_bytes + 64, 1536 * n),
                                dtype="f64" if vb == 8 else "f32")
        col.rowgroups[: trg.size * 32] = torch.from_numpy(trg.view(np.uint8).reshape(-1)).cuda()
        col.vectors[: n * 32] = torch.from_numpy(tv.view(np.uint8).reshape(-1)).cuda()
        col.packed[: self.packed_bytes] = torch.from_numpy(packed).cuda().repeat(k)
        col.exc[: self.exc_bytes] = torch.from_numpy(exc).cuda().repeat(k)
        col.totals[0], col.totals[1] = self.packed_bytes, self.exc_bytes
        self.col = col
        self.want_distinct = want
        self.want = torch.from_numpy(want.view(np.int64 if vb == 8 else np.int32)).cuda().repeat(k)
        self.truth()

    def truth(self):
        c = self.col.c
        c.packed_bytes_hint, c.exc_bytes_hint, c.alp_rd_rowgroups_hint = self.packed_bytes, self.exc_bytes, 1 + self.rd_rowgroups

    def lie(self, packed_bits, exc_bytes_per_vector, rd):
        c = self.col.c
        c.packed_bytes_hint, c.exc_bytes_hint, c.alp_rd_rowgroups_hint = lie_hints(self.n, packed_bits, exc_bytes_per_vector, rd)
        assert 1 <= c.packed_bytes_hint <= c.packed_capacity and c.exc_bytes_hint <= c.exc_capacity

    def check(self, ctx, what):
        out = ctx.decode(self.col)
        ctx.synchronize()
        it = torch.int64 if self.vb == 8 else torch.int32
        if not torch.equal(out.view(it), self.want):
            bad = torch.nonzero((out.view(it) != self.want).view(self.n, 1024).any(dim=1)).flatten()[:8].cpu().numpy()
            raise AssertionError((what, "vectors differ", bad.tolist(), [int(b) % self.distinct for b in bad]))


_BATTERIES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_batteries():
    yield
    _BATTERIES.clear()


def tiled(oracle, of32, vb, ordered):
    key = (vb, ordered)
    if key not in _BATTERIES:
        enc = battery(vb)
        want = oracle.decode_column(enc) if vb == 8 else of32.decode_column(enc)
        _BATTERIES[key] = Tiled(enc, vb, want, ordered)
    return _BATTERIES[key]


def _stream_direct_vectors(col_np_vec, n, chunk=12, arena=24576):
    """vectors the streamed float shape 27 (chunks of 12 vectors, a 24 KiB arena: decode_stream_f32_kernels.hip) decodes from HBM because their records do not fit what
    is left of the chunk's arena (kPlanDirect) — the kernel's own placement rule restated (a chunk whose records overflow the arena is laid out record by record)"""
    words = col_np_vec["bw"].astype(np.int64) + np.where(col_np_vec["scheme"] == 2, 0, col_np_vec["lbw"].astype(np.int64))
    cnt = col_np_vec["exc_cnt"].astype(np.int64)
    rec = (cnt * np.where(col_np_vec["scheme"] == 2, 6, 4) + 7) // 8 * 8
    slot = (128 * words + (rec + 15) // 16 * 16)[: n // chunk * chunk].reshape(-1, chunk)
    excl = np.cumsum(slot, axis=1) - slot
    return int(((excl + slot) > arena).sum())


@pytest.mark.parametrize("ordered", [True, False], ids=["vector_order", "out_of_order"])
@pytest.mark.parametrize("lie", list(LIES_F64))
def test_every_arm_of_the_double_rule_decodes_any_content(ctx, oracle, of32, lie, ordered):
    from alp_amd import capi
    t = tiled(oracle, of32, 8, ordered)
    (bits, exc_pv, rd), (vpw, many, pad) = LIES_F64[lie]
    try:
        for ra in (-1, 0, 1):
            ctx.set_option(capi.OPT_DECODE_READ_AHEAD, ra)
            t.lie(bits, exc_pv, rd)
            plan = ctx.decode_plan(t.col)
            assert plan is not None and (plan["vectors_per_wg"], plan["many_exc"], plan["pad_kib"]) == (vpw, many, pad), (lie, ra, plan)
            assert ctx.decode_vectors_per_wg(t.col) == vpw and ctx.decode_runs(t.col) == 1
            assert ctx.decode_reads_ahead(t.col) == (ra == 1), (lie, ra)  # (65 600 vectors: too short for the library's own read-ahead)
            t.check(ctx, (lie, ra))
    finally:
        ctx.set_option(capi.OPT_DECODE_READ_AHEAD, -1)
        t.truth()


@pytest.mark.parametrize("ordered", [True, False], ids=["vector_order", "out_of_order"])
@pytest.mark.parametrize("lie", list(LIES_F32))
def test_every_arm_of_the_float_rule_decodes_any_content(ctx, oracle, of32, lie, ordered):
    from alp_amd import capi
    t = tiled(oracle, of32, 4, ordered)
    (bits, exc_pv, rd), shape = LIES_F32[lie]
    if shape == 27:  # the streamed shape meets records that do not fit its arena and decodes them from HBM
        assert _stream_direct_vectors(layout.compact(t.enc, 4)[1], t.distinct) > 0
    try:
        for ra in (-1, 0, 1):
            ctx.set_option(capi.OPT_DECODE_READ_AHEAD, ra)
            t.lie(bits, exc_pv, rd)
            plan = ctx.decode_plan(t.col)
            assert plan is not None and plan["vectors_per_wg"] == shape and plan["pad_kib"] is None, (lie, ra, plan)
            assert ctx.decode_vectors_per_wg(t.col) == shape and ctx.decode_runs(t.col) == 1
            assert ctx.decode_reads_ahead(t.col) == (ra == 1 and shape < 16), (lie, ra)
            t.check(ctx, (lie, ra))
    finally:
        ctx.set_option(capi.OPT_DECODE_READ_AHEAD, -1)
        t.truth()


def test_the_truthful_hints_and_the_unhinted_decode_agree(ctx, oracle, of32):
    """the battery under its real sizes, and with no hints at all (device-side plan, then the learned sizes, which are the column's totals)"""
    for vb in (8, 4):
        t = tiled(oracle, of32, vb, True)
        try:
            t.truth()
            t.check(ctx, ("truth", vb))
            c = t.col.c
            c.packed_bytes_hint = c.exc_bytes_hint = c.alp_rd_rowgroups_hint = 0
            ctx.forget(t.col)
            assert ctx.decode_plan(t.col) is None
            t.check(ctx, ("unhinted", vb))
            learned = ctx.decode_plan(t.col)  # (the stream has drained: the sizes have landed)
            assert learned is not None and learned["packed_bytes"] == t.packed_bytes, (vb, learned)
            assert learned["rd_rowgroups_hint"] == 1 + t.rd_rowgroups
            t.check(ctx, ("learned", vb))
        finally:
            ctx.forget(t.col)
            t.truth()


def test_consumers_do_not_read_hints(ctx, oracle, of32):
    """decode_sum, decode_count_range and column_sum under a lie: their kernels do not read hints, so they match the documented-order host replicas"""
    import test_decode_sum_gpu as ds
    for vb, lie in ((8, (40, 1300, False)), (4, (6, 0, False))):
        t = tiled(oracle, of32, vb, False)
        try:
            t.lie(*lie)
            vals = t.want_distinct.reshape(t.distinct, 1024)
            sums = ds.host_sums(vals) if vb == 8 else ds.host_sums_f32(vals, t.enc)
            want = np.tile(sums, t.k)
            got = ctx.decode_sum(t.col).cpu().numpy()
            assert ds._same_bits(got, want).all(), vb
            total = ctx.column_sum(t.col).cpu().numpy()
            assert ds._same_bits(total, np.array([ds.host_column_total(want)])).all(), vb
            lo, hi = -1.0e3, 1.0e3
            with np.errstate(invalid="ignore"):
                cnt = ((vals >= lo) & (vals <= hi)).sum(axis=1)
            got_cnt = ctx.decode_count_range(t.col, lo, hi).cpu().numpy().astype(np.int64)
            assert np.array_equal(got_cnt, np.tile(cnt, t.k)), vb
        finally:
            t.truth()


# ---- stale plans ----------------------------------------------------------------------------------------------------------------------------------------------

def _halves(n, vb, swapped, seed):
    """double: a column whose first half is 6-bit vectors with 20 exceptions each (two vectors per workgroup) and whose second half is 44-bit vectors without (one per
    workgroup, six workgroups per CU); float: 4-bit vectors without exceptions (the streamed shape) and 20-bit ones with 20 each.  swapped: the other way round.  Both
    have the same length, stream sizes and capacities."""
    import bench
    idx = np.arange(n)
    first = idx < n // 2
    if swapped:
        first = ~first
    if vb == 8:
        bw, exc = np.where(first, 6, 44), np.where(first, 20, 0)
    else:
        bw, exc = np.where(first, 4, 20), np.where(first, 0, 20)
    col, vec, _ = bench.build_decode_column(n, 0, seed=seed, bw_of_rowgroup=bw, exc_per_vec=exc, value_bytes=vb)
    return col, vec


def _oracle_sample(oracle, col, vec, sel, vb):
    """the oracle's decode of the vectors sel of a bench-built column (ALP, one exception count)"""
    m = sel.size
    sub = {k: vec[k][sel].copy() for k in ("bw", "e", "f", "base", "exc_cnt", "lbw")}
    sub["scheme"] = vec["scheme"][sel].astype(np.uint8)
    sub["packed"] = np.zeros((m, 1024), np.int64 if vb == 8 else np.int32)
    sub["exc"] = np.zeros((m, 1024), np.float64 if vb == 8 else np.float32)
    sub["pos"] = np.zeros((m, 1024), np.uint16)
    sub["packed_left"] = np.zeros((m, 1024), np.uint16)
    sub["dict"] = np.zeros(((m + 99) // 100, 8), np.uint16)
    sub["dict_size"] = np.zeros((m + 99) // 100, np.uint8)
    p8 = sub["packed"].view(np.uint8).reshape(m, 1024 * vb)
    packed, excs = col.packed.cpu().numpy(), col.exc.cpu().numpy()
    for i, v in enumerate(sel):
        o, w, c = int(vec["packed_off"][v]), int(vec["bw"][v]), int(vec["exc_cnt"][v])
        p8[i, : 128 * w] = packed[o:o + 128 * w]
        if c:
            e = int(vec["exc_off"][v])
            r = excs[e: e + (vb + 2) * c]
            sub["exc"][i, :c] = r[: vb * c].view(sub["exc"].dtype)
            sub["pos"][i, :c] = r[vb * c:].view(np.uint16)
    return oracle.decode_column(sub)


def _copy_into(dst, src):
    """src's streams, descriptors and totals D2D into dst's buffers (what a caller's copy, or a caching allocator's next tenant, does behind the context's back)"""
    for a in ("rowgroups", "vectors", "packed", "exc", "totals"):
        getattr(dst, a).copy_(getattr(src, a))
    dst.c.packed_bytes_hint, dst.c.exc_bytes_hint, dst.c.alp_rd_rowgroups_hint = src.c.packed_bytes_hint, src.c.exc_bytes_hint, src.c.alp_rd_rowgroups_hint


@pytest.mark.parametrize("vb", [8, 4], ids=["f64", "f32"])
def test_a_stale_region_plan_decodes_the_new_content(ctx, oracle, of32, vb):
    from alp_amd import capi
    n = 4 * 32800  # four plan segments; the halves meet on a segment border
    x, _ = _halves(n, vb, False, seed=7)
    y, yvec = _halves(n, vb, True, seed=7)
    assert (x.c.packed_bytes_hint, x.c.exc_bytes_hint, x.c.packed_capacity, x.c.exc_capacity) == (y.c.packed_bytes_hint, y.c.exc_bytes_hint, y.c.packed_capacity, y.c.exc_capacity)
    want = ctx.decode(y).clone()  # (y has no plan: one launch)
    ctx.synchronize()
    runs_of = ctx.decode_runs
    assert runs_of(y) == 1
    o = oracle if vb == 8 else of32
    for lo in (0, n // 2 - 100, n - 100):
        sel = np.arange(lo, lo + 200) if lo + 200 <= n else np.arange(lo, n)
        got = want.view(-1, 1024)[torch.from_numpy(sel).cuda()].cpu().numpy().reshape(-1)
        assert np.array_equal(got.view(np.uint8), _oracle_sample(o, y, yvec, sel, vb).view(np.uint8)), lo
    try:
        ctx.column_totals(x)
        runs = runs_of(x)
        assert runs >= 2, runs
        if vb == 4:  # the plan's first run is the streamed shape (27), which now meets 20-bit vectors with exceptions
            first = capi.DeviceColumn(1, dtype="f32")  # (the rule reads the length and the hints only)
            first.c.n_vectors, first.c.packed_bytes_hint, first.c.exc_bytes_hint = n // 2, n // 2 * 4 * 128, 0
            assert ctx.decode_vectors_per_wg(first) == 27
        _copy_into(x, y)
        assert runs_of(x) == runs  # the key still matches: x's runs are applied to y's content
        out = torch.zeros_like(want)
        ctx.decode(x, out)
        ctx.synchronize()
        assert torch.equal(out.view(torch.uint8), want.view(torch.uint8))
    finally:
        ctx.forget(x)


def test_stale_learned_sizes_decode_the_new_content(ctx):
    n = 4 * 32800
    x, _ = _halves(n, 8, False, seed=9)
    y, _ = _halves(n, 8, True, seed=9)
    want = ctx.decode(y).clone()
    ctx.synchronize()
    pb, eb = int(x.c.packed_bytes_hint), int(x.c.exc_bytes_hint)
    try:
        x.c.packed_bytes_hint = x.c.exc_bytes_hint = x.c.alp_rd_rowgroups_hint = 0
        ctx.forget(x)
        assert ctx.decode_plan(x) is None
        ctx.decode(x)  # unhinted: the sizes travel to the host behind the decode ...
        ctx.synchronize()  # ... and have landed
        learned = ctx.decode_plan(x)
        assert learned is not None and (learned["packed_bytes"], learned["exc_bytes"]) == (pb, eb), learned
        for a in ("rowgroups", "vectors", "packed", "exc", "totals"):
            getattr(x, a).copy_(getattr(y, a))
        assert ctx.decode_plan(x) == learned  # the stale learned shape is what the next decode uses
        out = torch.zeros_like(want)
        ctx.decode(x, out)
        ctx.synchronize()
        assert torch.equal(out.view(torch.int64), want.view(torch.int64))
    finally:
        ctx.forget(x)


def test_another_context_encodes_into_the_column(ctx):
    """a column encoded through this context and planned region by region (column_totals), then encoded again with other content of the same sizes through a SECOND
    context: this context's plan is stale, and its decode still gives the new input's bits"""
    from alp_amd import capi
    n = 2 * 32800
    g = torch.Generator(device="cuda:0")
    g.manual_seed(21)
    narrow = torch.round(torch.rand(n // 2 * 1024, dtype=torch.float64, device="cuda:0", generator=g) * 100, decimals=1)
    narrow[::53] = torch.rand(narrow[::53].shape, dtype=torch.float64, device="cuda:0", generator=g)  # exceptions
    wide = torch.rand(n // 2 * 1024, dtype=torch.float64, device="cuda:0", generator=g)  # full-precision values: ALP_RD rowgroups
    a = torch.cat([narrow, wide])
    b = torch.cat([wide, narrow])
    col = capi.DeviceColumn(n)
    other = capi.Context(0)
    try:
        ctx.encode(a, col)
        totals = ctx.column_totals(col)
        runs = ctx.decode_runs(col)
        assert runs >= 2, runs
        other.encode(b, col)
        assert other.column_totals(col) == totals  # the same sizes: this context's key still matches
        assert ctx.decode_runs(col) == runs
        out = ctx.decode(col)
        ctx.synchronize()
        assert torch.equal(out.view(torch.int64), b.view(torch.int64))
    finally:
        ctx.forget(col)
        other.close()
