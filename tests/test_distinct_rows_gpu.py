"""GPU: k_distinct_insert (distinct_kernels.hip) decodes in registers (register_decode.hpp), so it reads the hand-built vectors of float_rows.py (widths
0..32, cuts 16..31) and double_rows.py (widths 0..64, cuts 48..63): every width under every factor, bases on the bounds of the conversion shortcut,
exception records on both sides of every lane count and stage, every ALP_RD cut with a dictionary of its own.  The columns are built as
tests/test_histogram_rows_gpu.py builds them: in vector order, and with their records shuffled in the streams.

EVERY expectation is the oracle's decode of the hand-built encoding (oracle/pyoracle.py: Oracle / OracleF32 decode_column) fed through the host replica
(tests/distinct_replica.py).  The columns have thousands of vectors of mostly distinct values, so a call covers a range of 512 vectors with a capacity
of 2^19, which cannot overflow.  Values compare by their bytes, counts as integers."""
import numpy as np
import pytest
import torch

import double_rows as dr
import float_rows as fr
import layout
from distinct_replica import host_distinct

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0x5A5A5A5A5A5A5A5A
RANGE_VECTORS = 512
CAPACITY = 1 << 19
GUARD = 32


def random_mask(n_vectors, seed):
    words = np.random.default_rng(seed).integers(0, 2**64, 16 * n_vectors, dtype=np.uint64)
    return torch.from_numpy(words.view(np.int64)).to(DEV)


def vectors_cleared(mask, keep_every):
    m = mask.clone().reshape(-1, 16)
    v = torch.arange(m.shape[0], device=mask.device)
    m[(v % keep_every) != 1] = 0
    return m.reshape(-1)


def unpack(words, nv):
    """a bitmap's int64 words on the host -> bool [nv, 1024]"""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little").astype(bool).reshape(nv, 1024)


class Built:
    """a hand-built encoding, the oracle's decode of it, and the column in HBM"""

    def __init__(self, ctx, oracle, enc, dtype, shuffle_seed=None):
        from alp_amd import capi
        W = 8 if dtype == "f64" else 4
        self.enc, self.dtype = enc, dtype
        self.nv = enc["scheme"].size
        self.want = oracle.decode_column(enc)
        assert self.want.dtype == (np.float64 if W == 8 else np.float32) and self.want.size == 1024 * self.nv
        rg, vec, packed, exc = layout.compact(enc, W)
        if shuffle_seed is not None:  # the same vectors, their records somewhere else in the streams
            order = np.random.default_rng(shuffle_seed).permutation(self.nv)
            _, placed, packed, exc = layout.compact(fr.take_vectors(enc, order), W)  # placement i holds the records of vector order[i]
            vec = vec.copy()
            vec["packed_off"][order] = placed["packed_off"]
            vec["exc_off"][order] = placed["exc_off"]
            assert (np.diff(vec["packed_off"].astype(np.int64)) < 0).any()
        self.col = capi.DeviceColumn.from_host(rg, vec, packed, exc, dtype=dtype)
        assert ctx.column_validate(self.col) is None, "the hand-built descriptors are ones the kernels are specified for"
        self.alp = enc["scheme"] == fr.SCHEME_ALP


class Columns:
    def __init__(self, ctx, dtype):
        from oracle.pyoracle import Oracle, OracleF32
        rows, oracle = (dr, Oracle()) if dtype == "f64" else (fr, OracleF32())
        self.dtype, self.rows = dtype, rows
        self.value_bits = 64 if dtype == "f64" else 32
        enc = fr.concat_encodings([rows.alp_rows(), rows.rd_rows()])
        self.A = Built(ctx, oracle, enc, dtype)
        self.S = Built(ctx, oracle, enc, dtype, shuffle_seed=31)
        self.nv = self.A.nv
        assert np.array_equal(self.A.want.view(np.uint8), self.S.want.view(np.uint8))
        rnd = random_mask(self.nv, 51)
        self.masks = {"none": None, "random": rnd, "cleared": vectors_cleared(rnd, 3)}
        self.mask_bits = {k: np.ones((self.nv, 1024), bool) if m is None else unpack(m.cpu().numpy(), self.nv) for k, m in self.masks.items()}
        self.ranges = [(v0, min(RANGE_VECTORS, self.nv - v0)) for v0 in range(0, self.nv, RANGE_VECTORS)]
        it = torch.int64 if dtype == "f64" else torch.int32
        self.vals_raw = torch.empty(CAPACITY + GUARD, dtype=it, device=DEV)
        self.vals = self.vals_raw[:CAPACITY].view(torch.float64 if dtype == "f64" else torch.float32)
        self.counts_raw = torch.empty(CAPACITY + GUARD, dtype=torch.int64, device=DEV)
        self.state = torch.empty(4, dtype=torch.int64, device=DEV)
        self.scratch = ctx.distinct_scratch(CAPACITY)
        self.memo = {}

    def expect(self, v0, n_vec, mname):
        """the replica on the oracle's decode of the range's vectors: computed once, shared by both placements"""
        key = (v0, mname)
        if key not in self.memo:
            self.memo[key] = host_distinct(self.A.want[1024 * v0: 1024 * (v0 + n_vec)], self.mask_bits[mname][v0: v0 + n_vec].reshape(-1))
        return self.memo[key]

    def call(self, ctx, b, v0, n_vec, mname, trace=None):
        self.vals_raw.fill_(0x5A5A5A5A5A5A5A5A if self.dtype == "f64" else 0x5A5A5A5A)
        self.counts_raw.fill_(POISON)
        self.state.fill_(POISON)
        ctx.distinct_into(b.col, self.vals, self.state, counts_out=self.counts_raw[:CAPACITY], mask=self.masks[mname], first=1024 * v0, n=1024 * n_vec, scratch=self.scratch, trace=trace)
        return self.state.tolist()


@pytest.fixture(scope="module", params=["f64", "f32"])
def cols(ctx, request):
    return Columns(ctx, request.param)


@pytest.mark.parametrize("mname", ["none", "random", "cleared"])
def test_distinct_of_the_hand_built_rows(ctx, cols, mname):
    poison_v = POISON if cols.dtype == "f64" else 0x5A5A5A5A
    nans = numbers = 0
    for name, b in (("A", cols.A), ("S", cols.S)):
        for v0, n_vec in cols.ranges:
            values, counts, n_nan, n_num = cols.expect(v0, n_vec, mname)
            d = values.size
            assert d <= CAPACITY
            state = cols.call(ctx, b, v0, n_vec, mname)
            what = f"{cols.dtype} {name}, vectors [{v0}, {v0 + n_vec}), bitmap {mname}"
            assert state == [d, n_nan, n_num, 0], f"{what}: state {state}, want {[d, n_nan, n_num, 0]}"
            assert cols.vals[:d].cpu().numpy().tobytes() == values.tobytes(), f"{what}: the values are not the oracle's decode through the replica"
            assert np.array_equal(cols.counts_raw[:d].cpu().numpy().view(np.uint64), counts), f"{what}: the counts are not the oracle's decode through the replica"
            assert bool((cols.vals_raw[d:] == poison_v).all()) and bool((cols.counts_raw[d:] == POISON).all()), f"{what}: written behind the D entries"
            nans += n_nan
            numbers += n_num
    assert nans > 0 and numbers > 0, "NaNs and numbers are selected"


def test_the_call_decoded_every_width_cut_and_exception_class(ctx, cols):
    """what the kernel decoded, from its own trace: per bitmap, trace word 2 (decoded) summed over the ranges must be exactly the vectors with a
    selected bit and word 1 zero (no zones), so the classes of those vectors are classes the kernel read: without a bitmap and under the random one
    every vector, under the cleared one every third — all classes on both sides"""
    rows, e = cols.rows, cols.A.enc
    for mname in cols.masks:
        decoded = cols.mask_bits[mname].any(axis=1)
        trace = torch.zeros(6, dtype=torch.int64, device=DEV)
        for v0, n_vec in cols.ranges:
            cols.call(ctx, cols.A, v0, n_vec, mname, trace=trace)
        t = trace.tolist()
        assert t[:3] == [cols.nv - int(decoded.sum()), 0, int(decoded.sum())], f"bitmap {mname}: the trace {t} is not the vectors with a selected bit"
    widths, cuts = list(range(cols.value_bits + 1)), sorted(rows.rd_cuts())

    def classes(decoded):
        alp, rd = cols.A.alp & decoded, ~cols.A.alp & decoded
        return dict(widths=sorted(set(e["bw"][alp].tolist())), cuts=sorted(set(zip(e["bw"][rd].tolist(), e["lbw"][rd].tolist()))),
                    alp_exc=sorted(set(e["exc_cnt"][alp].tolist())), rd_exc=sorted(set(e["exc_cnt"][rd].tolist())))
    kept = cols.mask_bits["cleared"].any(axis=1)
    for what, decoded in (("every vector", np.ones(cols.nv, bool)), ("the kept third", kept), ("the cleared two thirds", ~kept)):
        got = classes(decoded)
        print(f"coverage {cols.dtype} distinct, {what}: {int(decoded.sum())} of {cols.nv} vectors; ALP widths {got['widths'][0]}..{got['widths'][-1]} ({len(got['widths'])}), "
              f"ALP_RD cuts {len(got['cuts'])} of {len(cuts)}, ALP exception counts {got['alp_exc']}, ALP_RD exception counts {got['rd_exc']}")
        assert got["widths"] == widths, what
        assert got["cuts"] == cuts, what
        assert got["alp_exc"] == sorted(rows.ALP_EXC_COUNTS) and got["rd_exc"] == sorted(rows.RD_EXC_COUNTS), what
