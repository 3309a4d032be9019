"""GPU: k_histogram (histogram_kernels.hip) decodes in registers (register_decode.hpp), so it reads the hand-built vectors of float_rows.py (widths 0..32,
cuts 16..31) and double_rows.py (widths 0..64, cuts 48..63): every width under every factor, bases on the bounds of the conversion shortcut, exception
records on both sides of every lane count and stage, every ALP_RD cut with a dictionary of its own.  The columns are built as
tests/test_register_decode_rows_gpu.py builds them: in vector order, and with their records shuffled in the streams.

EVERY expectation is the oracle's decode of the hand-built encoding (oracle/pyoracle.py: Oracle / OracleF32 decode_column) fed through the host replica
(tests/histogram_replica.py).  Counts compare as integers."""
import numpy as np
import pytest
import torch

import double_rows as dr
import float_rows as fr
import layout
from histogram_replica import host_histogram

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
POISON = 0x5A5A5A5A5A5A5A5A
EDGE_COUNTS = (7, 300, 4095)


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
        self.values = self.want.reshape(self.nv, 1024)
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
        rng = np.random.default_rng(77)
        flat = self.A.want
        present = np.unique(flat[np.isfinite(flat)])
        self.edges = {}
        for size in EDGE_COUNTS:  # values of the oracle's decode (values sit on edges), +-inf and both zeros; sorted, as the call wants them
            e = np.concatenate([np.array([INF, -INF, 0.0, -0.0], flat.dtype), rng.choice(present, size - 4, replace=False)])
            self.edges[size] = np.sort(e)
        self.memo = {}

    def expect(self, size, mname, right):
        key = (size, mname, right)
        if key not in self.memo:
            self.memo[key] = host_histogram(self.A.want, self.edges[size], self.mask_bits[mname].reshape(-1), right)
        return self.memo[key]


@pytest.fixture(scope="module", params=["f64", "f32"])
def cols(ctx, request):
    return Columns(ctx, request.param)


def describe(b, bad_vectors, limit=6):
    e = b.enc
    rows = [(int(v), "ALP" if e["scheme"][v] == fr.SCHEME_ALP else "ALP_RD", int(e["bw"][v]), int(e["lbw"][v]), int(e["f"][v]), int(e["e"][v]), int(e["base"][v]), int(e["exc_cnt"][v]))
            for v in bad_vectors[:limit]]
    return f"{len(bad_vectors)} vectors differ; (vector, scheme, bw, lbw, f, e, base, exc_cnt): {rows}"


@pytest.mark.parametrize("mname", ["none", "random", "cleared"])
def test_histogram_of_the_hand_built_rows(ctx, cols, mname):
    for name, b in (("A", cols.A), ("S", cols.S)):
        for size in EDGE_COUNTS:
            edges = torch.from_numpy(cols.edges[size]).to(DEV)
            for right in (False, True):
                want = cols.expect(size, mname, right)
                got = torch.full((size + 2,), POISON, dtype=torch.int64, device=DEV)
                trace = torch.zeros(4, dtype=torch.int64, device=DEV)
                ctx.histogram_into(b.col, edges, got, mask=cols.masks[mname], right=right, trace=trace)
                assert np.array_equal(got.cpu().numpy().view(np.uint64), want), f"{cols.dtype} {name}, {size} edges, right={right}, bitmap {mname}: not the oracle's decode through the replica"
                selected = int(cols.mask_bits[mname].any(axis=1).sum())
                assert trace.tolist() == [cols.nv - selected, 0, 0, selected], "every vector with a selected bit is decoded"
        assert int(want[-1]) > 0 and int(want[:-1].sum()) > 0, "NaNs and numbers are selected"


def test_histogram_vector_by_vector(ctx, cols):
    """one call per vector over its 1024 values: a difference names the vector and its descriptor"""
    size = EDGE_COUNTS[0]
    e = cols.edges[size]
    real = e[~np.isnan(e)]
    for name, b in (("A", cols.A), ("S", cols.S)):
        edges = torch.from_numpy(e).to(DEV)
        got = torch.full((b.nv, size + 2), POISON, dtype=torch.int64, device=DEV)
        for v in range(b.nv):
            ctx.histogram_into(b.col, edges, got[v], first=1024 * v, n=1024)
        nan = np.isnan(b.values)
        bucket = np.where(nan, size + 1, np.searchsorted(real, np.where(nan, 0, b.values), side="right"))
        want = np.zeros((b.nv, size + 2), np.int64)
        np.add.at(want, (np.repeat(np.arange(b.nv), 1024), bucket.reshape(-1)), 1)
        assert np.array_equal(want.sum(axis=0).astype(np.uint64), cols.expect(size, "none", False)), "the per-vector expectation adds up to the replica's"
        same = (got.cpu().numpy() == want).all(axis=1)
        if not same.all():
            pytest.fail(f"{cols.dtype} {name} histogram of single vectors: " + describe(b, np.nonzero(~same)[0]))


def test_the_histogram_decoded_every_width_cut_and_exception_class(ctx, cols):
    """what the kernel decoded, from its own trace: one call per bitmap here, trace word 3 (decoded by the general route) must be exactly the vectors with a
    selected bit and words 1 and 2 zero (no zones, no other route), so the classes of those vectors are classes the kernel read: without a bitmap and
    under the random one every vector, under the cleared one every third — all classes on both sides"""
    rows, e = cols.rows, cols.A.enc
    size = EDGE_COUNTS[0]
    edges = torch.from_numpy(cols.edges[size]).to(DEV)
    for mname, m in cols.masks.items():
        decoded = cols.mask_bits[mname].any(axis=1)
        trace = torch.zeros(4, dtype=torch.int64, device=DEV)
        ctx.histogram_into(cols.A.col, edges, torch.empty(size + 2, dtype=torch.int64, device=DEV), mask=m, trace=trace)
        assert trace.tolist() == [cols.nv - int(decoded.sum()), 0, 0, int(decoded.sum())], f"bitmap {mname}: the trace is not the vectors with a selected bit"
    widths, cuts = list(range(cols.value_bits + 1)), sorted(rows.rd_cuts())

    def classes(decoded):
        alp, rd = cols.A.alp & decoded, ~cols.A.alp & decoded
        return dict(widths=sorted(set(e["bw"][alp].tolist())), cuts=sorted(set(zip(e["bw"][rd].tolist(), e["lbw"][rd].tolist()))),
                    alp_exc=sorted(set(e["exc_cnt"][alp].tolist())), rd_exc=sorted(set(e["exc_cnt"][rd].tolist())))
    kept = cols.mask_bits["cleared"].any(axis=1)
    for what, decoded in (("every vector", np.ones(cols.nv, bool)), ("the kept third", kept), ("the cleared two thirds", ~kept)):
        got = classes(decoded)
        print(f"coverage {cols.dtype} histogram, {what}: {int(decoded.sum())} of {cols.nv} vectors; ALP widths {got['widths'][0]}..{got['widths'][-1]} ({len(got['widths'])}), "
              f"ALP_RD cuts {len(got['cuts'])} of {len(cuts)}, ALP exception counts {got['alp_exc']}, ALP_RD exception counts {got['rd_exc']}")
        assert got["widths"] == widths, what
        assert got["cuts"] == cuts, what
        assert got["alp_exc"] == sorted(rows.ALP_EXC_COUNTS) and got["rd_exc"] == sorted(rows.RD_EXC_COUNTS), what
