"""GPU: k_keyed_minmax (keyed_minmax_kernels.hip) decodes two vectors side by side in registers (register_decode.hpp), so it reads the hand-built vectors
of double_rows.py (widths 0..64, cuts 48..63) AND float_rows.py (widths 0..32, cuts 16..31) as BOTH its value and its key column: every width under
every factor, exception records on both sides of every lane count and stage, every ALP_RD cut with a dictionary of its own.  The columns are built as
tests/test_histogram_rows_gpu.py builds them: in vector order (A), and with their records shuffled in the streams (S).

EVERY expectation is the oracle's decode of the hand-built encoding (oracle/pyoracle.py) fed through the host replica (tests/keyed_minmax_replica.py).
The keys are the rows' own distinct values.  Records compare bit for bit, counts as integers."""
import numpy as np
import pytest
import torch

from keyed_minmax_replica import host_keyed_minmax, same_records
from test_histogram_rows_gpu import Built, random_mask, unpack, vectors_cleared
import double_rows as dr
import float_rows as fr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0x5A5A5A5A5A5A5A5A
KEY_COUNTS = (7, 256, 1024)


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
        rnd = random_mask(self.nv, 53)
        self.masks = {"none": None, "random": rnd, "cleared": vectors_cleared(rnd, 3)}
        self.mask_bits = {k: np.ones((self.nv, 1024), bool) if m is None else unpack(m.cpu().numpy(), self.nv) for k, m in self.masks.items()}
        flat = self.A.want
        present = np.unique(flat[~np.isnan(flat)])  # (+-inf and one of the zeros among them, if the rows hold them)
        rng = np.random.default_rng(79)
        self.keys = {size: np.sort(rng.choice(present, min(size, present.size), replace=False)) for size in KEY_COUNTS}
        self.memo = {}

    def expect(self, size, mname):
        if (size, mname) not in self.memo:
            self.memo[(size, mname)] = host_keyed_minmax(self.A.want, self.A.want, self.mask_bits[mname].reshape(-1), self.keys[size])
        return self.memo[(size, mname)]

    def call(self, ctx, val, key, keys, mask, trace=None):
        kd = torch.from_numpy(keys).to(DEV)
        out = torch.full((keys.size, 2), float("nan"), dtype=self.tdt, device=DEV)
        cnt = torch.full((keys.size + 1,), POISON, dtype=torch.int64, device=DEV)
        ctx.keyed_minmax_into(val.col, key.col, kd, out, counts_out=cnt, mask=mask, trace=trace)
        return out.cpu().numpy(), cnt.cpu().numpy()


@pytest.fixture(scope="module", params=["f64", "f32"])
def cols(ctx, request):
    return Columns(ctx, request.param)


@pytest.mark.parametrize("mname", ["none", "random", "cleared"])
def test_keyed_minmax_of_the_hand_built_rows_by_their_own_values(ctx, cols, mname):
    for name, val, key in (("A by A", cols.A, cols.A), ("A by S", cols.A, cols.S), ("S by A", cols.S, cols.A)):
        for size in KEY_COUNTS:
            keys = cols.keys[size]
            want_r, want_c = cols.expect(size, mname)
            trace = torch.zeros(4, dtype=torch.int64, device=DEV)
            got_r, got_c = cols.call(ctx, val, key, keys, cols.masks[mname], trace=trace)
            assert np.array_equal(got_c, want_c), f"{cols.dtype} {name}, {keys.size} keys, bitmap {mname}: counts are not the oracle's decode through the replica"
            assert same_records(got_r, want_r), f"{cols.dtype} {name}, {keys.size} keys, bitmap {mname}: records are not the oracle's decode through the replica"
            selected = int(cols.mask_bits[mname].any(axis=1).sum())
            assert trace.tolist() == [cols.nv - selected, 0, 0, selected], "every vector with a selected bit is decoded, both columns"
    assert int(want_c[-1]) > 0 and int(want_c[:-1].sum()) > 0, "rows with and without a key are selected"


def test_keyed_minmax_vector_by_vector(ctx, cols):
    """a bitmap that selects one vector at a time: a difference names the vector"""
    keys = cols.keys[KEY_COUNTS[1]]
    bad = []
    step = max(1, cols.nv // 150)  # every step-th vector: the test stays quick; the whole-column test above reads all of them
    every = np.ones(1024, bool)
    for v in range(0, cols.nv, step):
        mask = torch.zeros(16 * cols.nv, dtype=torch.int64, device=DEV)
        mask[16 * v: 16 * v + 16] = -1
        want_r, want_c = host_keyed_minmax(cols.A.values[v], cols.A.values[v], every, keys)
        got_r, got_c = cols.call(ctx, cols.A, cols.S, keys, mask)
        if not (np.array_equal(got_c, want_c) and same_records(got_r, want_r)):
            bad.append(v)
    e = cols.A.enc
    assert not bad, f"{cols.dtype}: vectors {bad[:8]} differ; (scheme, bw, lbw, exc_cnt) of the first: {[(int(e[k][bad[0]])) for k in ('scheme', 'bw', 'lbw', 'exc_cnt')]}"
