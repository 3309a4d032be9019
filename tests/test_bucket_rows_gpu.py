"""GPU: k_bucket_sum and k_bucket_minmax (bucket_kernels.hip) decode two vectors side by side in registers (register_decode.hpp), so they read the
hand-built vectors of double_rows.py (widths 0..64, cuts 48..63) AND float_rows.py (widths 0..32, cuts 16..31) as BOTH their value and their key column:
every width under every factor, the bases on the shortcut's bounds, exception records on both sides of every lane count and stage (around 64, 128 and
512 exceptions), every ALP_RD cut with a dictionary of its own.  The columns are built as tests/test_histogram_rows_gpu.py builds them: in vector
order (A), and with their records shuffled in the streams (S).

EVERY expectation is the oracle's decode of the hand-built encoding (oracle/pyoracle.py) fed through the host replica (tests/bucket_replica.py).  The
edges are quantiles of the rows' own values.  Sums compare bit for bit (NaNs as NaNs), records byte for byte, counts as integers."""
import numpy as np
import pytest
import torch

from bucket_replica import host_bucket_minmax, host_bucket_sum
from keyed_minmax_replica import same_records
from keyed_replica import same_sums
from test_histogram_rows_gpu import Built, random_mask, unpack, vectors_cleared
import double_rows as dr
import float_rows as fr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
POISON = 0x5A5A5A5A5A5A5A5A
EDGE_COUNTS = (7, 255, 1023)


class Columns:
    def __init__(self, ctx, dtype):
        from oracle.pyoracle import Oracle, OracleF32
        rows, oracle = (dr, Oracle()) if dtype == "f64" else (fr, OracleF32())
        self.dtype, self.rows = dtype, rows
        self.tdt = torch.float64 if dtype == "f64" else torch.float32
        enc = fr.concat_encodings([rows.alp_rows(), rows.rd_rows()])
        self.A = Built(ctx, oracle, enc, dtype)
        self.S = Built(ctx, oracle, enc, dtype, shuffle_seed=31)
        self.nv = self.A.nv
        rnd = random_mask(self.nv, 54)
        self.masks = {"none": None, "random": rnd, "cleared": vectors_cleared(rnd, 3)}
        self.mask_bits = {k: np.ones((self.nv, 1024), bool) if m is None else unpack(m.cpu().numpy(), self.nv) for k, m in self.masks.items()}
        flat = self.A.want
        real = np.sort(flat[~np.isnan(flat)])  # (+-inf and both zeros among them, if the rows hold them)
        self.edges = {size: real[((np.arange(size) + 0.5) * real.size / size).astype(np.int64)] for size in EDGE_COUNTS}  # quantiles: duplicates where a value is frequent
        self.memo = {}

    def expect(self, size, right, mname):
        if (size, right, mname) not in self.memo:
            bits = self.mask_bits[mname].reshape(-1)
            s, c = host_bucket_sum(self.A.want, self.A.want, bits, self.edges[size], right)
            r, cr = host_bucket_minmax(self.A.want, self.A.want, bits, self.edges[size], right)
            assert np.array_equal(c, cr)
            self.memo[(size, right, mname)] = (s, r, c)
        return self.memo[(size, right, mname)]

    def call(self, ctx, val, key, edges, right, mask, traces=(None, None)):
        ed = torch.from_numpy(np.ascontiguousarray(edges)).to(DEV)
        B = edges.size + 1
        sums = torch.full((B,), NAN, dtype=torch.float64, device=DEV)
        out = torch.full((B, 2), NAN, dtype=self.tdt, device=DEV)
        cs = torch.full((B + 1,), POISON, dtype=torch.int64, device=DEV)
        cm = torch.full((B + 1,), POISON, dtype=torch.int64, device=DEV)
        ctx.bucket_sum_into(val.col, key.col, ed, sums, counts_out=cs, right=right, mask=mask, trace=traces[0])
        ctx.bucket_minmax_into(val.col, key.col, ed, out, counts_out=cm, right=right, mask=mask, trace=traces[1])
        return sums.cpu().numpy(), out.cpu().numpy(), cs.cpu().numpy(), cm.cpu().numpy()


@pytest.fixture(scope="module", params=["f64", "f32"])
def cols(ctx, request):
    return Columns(ctx, request.param)


@pytest.mark.parametrize("size,right", [(7, False), (255, True), (1023, False), (1023, True)])  # both tiers, both rules; one case stays a few seconds
@pytest.mark.parametrize("mname", ["none", "random", "cleared"])
def test_buckets_of_the_hand_built_rows_by_quantiles_of_their_own_values(ctx, cols, mname, size, right):
    want_s, want_r, want_c = cols.expect(size, right, mname)
    for name, val, key in (("A by A", cols.A, cols.A), ("A by S", cols.A, cols.S), ("S by A", cols.S, cols.A)):
        traces = (torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV))
        s, r, cs, cm = cols.call(ctx, val, key, cols.edges[size], right, cols.masks[mname], traces)
        what = f"{cols.dtype} {name}, {size} edges, right {right}, bitmap {mname}"
        assert np.array_equal(cs, want_c) and np.array_equal(cm, want_c), f"{what}: counts are not the oracle's decode through the replica"
        assert same_sums(s, want_s), f"{what}: sums are not the oracle's decode through the replica"
        assert same_records(r, want_r), f"{what}: records are not the oracle's decode through the replica"
        selected = int(cols.mask_bits[mname].any(axis=1).sum())
        assert traces[0].tolist() == [cols.nv - selected, 0, 0, selected] == traces[1].tolist(), "every vector with a selected bit is decoded, both columns"
    assert int(want_c[:-1].sum()) > 0 and int(want_c.sum()) == int(cols.mask_bits[mname].sum())


def test_buckets_vector_by_vector(ctx, cols):
    """a bitmap that selects one vector at a time: a difference names the vector"""
    edges = cols.edges[EDGE_COUNTS[1]]
    bad = []
    # the column's sums under such a bitmap are the selected vector's own: its stripe's other vectors, and the other stripes, add +0.0
    step = max(1, cols.nv // 150)  # every step-th vector: the test stays quick; the whole-column test above reads all of them
    every = np.ones(1024, bool)
    for v in range(0, cols.nv, step):
        mask = torch.zeros(16 * cols.nv, dtype=torch.int64, device=DEV)
        mask[16 * v: 16 * v + 16] = -1
        right = bool((v // step) & 1)
        want_s, want_c = host_bucket_sum(cols.A.values[v], cols.A.values[v], every, edges, right)
        want_r, _ = host_bucket_minmax(cols.A.values[v], cols.A.values[v], every, edges, right)
        s, r, cs, cm = cols.call(ctx, cols.A, cols.S, edges, right, mask)
        if not (np.array_equal(cs, want_c) and np.array_equal(cm, want_c) and same_sums(s, want_s) and same_records(r, want_r)):
            bad.append(v)
    e = cols.A.enc
    assert not bad, f"{cols.dtype}: vectors {bad[:8]} differ; (scheme, bw, lbw, exc_cnt) of the first: {[(int(e[k][bad[0]])) for k in ('scheme', 'bw', 'lbw', 'exc_cnt')]}"
