"""GPU: k_join_probe (join_kernels.hip) decodes in registers (register_decode.hpp), so it reads the hand-built vectors of float_rows.py (widths 0..32,
cuts 16..31) and double_rows.py (widths 0..64, cuts 48..63): every width under every factor, bases on the bounds of the conversion shortcut, exception
records on both sides of every lane count and stage, every ALP_RD cut with a dictionary of its own.  The columns are built as
tests/test_histogram_rows_gpu.py builds them: in vector order, and with their records shuffled in the streams.

EVERY expectation is the oracle's decode of the hand-built encoding (oracle/pyoracle.py: Oracle / OracleF32 decode_column) fed through the host replica
(tests/join_replica.py).  Positions, spans and indices compare as integers."""
import numpy as np
import pytest
import torch

import double_rows as dr
import float_rows as fr
from alp_amd import capi
from join_replica import NO_MATCH, host_join
from test_histogram_rows_gpu import Built, describe, random_mask, vectors_cleared

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
POISON = 0x5A5A5A5A5A5A5A5A
ROW_BASE = 1000000


class Columns:
    def __init__(self, ctx, dtype):
        from oracle.pyoracle import Oracle, OracleF32
        rows, oracle = (dr, Oracle()) if dtype == "f64" else (fr, OracleF32())
        self.dtype = dtype
        enc = fr.concat_encodings([rows.alp_rows(), rows.rd_rows()])
        self.A = Built(ctx, oracle, enc, dtype)
        self.S = Built(ctx, oracle, enc, dtype, shuffle_seed=31)
        self.nv = self.A.nv
        assert np.array_equal(self.A.want.view(np.uint8), self.S.want.view(np.uint8))
        rnd = random_mask(self.nv, 51)
        self.masks = {"none": None, "random": rnd, "cleared": vectors_cleared(rnd, 3)}
        rng = np.random.default_rng(77)
        flat = self.A.want
        present = np.unique(flat[np.isfinite(flat)])
        self.keys, self.rows = {}, {}
        for size in (7, 300, capi.Context.in_list_lds_max(dtype) + 1):  # values of the oracle's decode, +-inf and both zeros, some twice; sorted, as the call wants them
            drawn = rng.choice(present, min(present.size, size - 4 - size // 5), replace=False)
            e = np.concatenate([np.array([INF, -INF, 0.0, -0.0], flat.dtype), drawn, drawn[: size - 4 - drawn.size]])
            assert e.size == size, "the decoded values hold enough distinct numbers for the longest list"
            self.keys[size] = np.sort(e)
            self.rows[size] = ROW_BASE + rng.permutation(size).astype(np.int64)
        self.memo = {}

    def expect(self, size, mname):
        if (size, mname) not in self.memo:
            m = self.masks[mname]
            self.memo[(size, mname)] = host_join(self.A.want, self.keys[size], None if m is None else m.cpu().numpy(), self.rows[size])
        return self.memo[(size, mname)]


@pytest.fixture(scope="module", params=["f64", "f32"])
def cols(ctx, request):
    return Columns(ctx, request.param)


@pytest.mark.parametrize("mname", ["none", "random", "cleared"])
def test_join_probe_of_the_hand_built_rows(ctx, cols, mname):
    total = 1024 * cols.nv
    for name, b in (("A", cols.A), ("S", cols.S)):
        for size in cols.keys:
            widx, wpos, wspan = cols.expect(size, mname)
            keys, rows = torch.from_numpy(cols.keys[size]).to(DEV), torch.from_numpy(cols.rows[size]).to(DEV)
            pos = torch.full((total,), POISON, dtype=torch.int64, device=DEV)
            spn = torch.full((total,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
            idx = torch.full((total,), POISON, dtype=torch.int64, device=DEV)
            count = torch.full((1,), POISON, dtype=torch.int64, device=DEV)
            ctx.join_probe_into(b.col, keys, pos, count, mask=cols.masks[mname], rows=rows, span_out=spn, idx_out=idx)
            k = int(count.item())
            what = f"{cols.dtype} {name}, {size} keys, bitmap {mname}"
            assert k == widx.size, what
            pos, spn, idx = pos.cpu().numpy(), spn.cpu().numpy().view(np.uint32), idx.cpu().numpy()
            assert np.array_equal(idx[:k], widx), what + ": indices"
            bad = (pos[:k] != wpos) | (spn[:k] != wspan)
            if bad.any():
                pytest.fail(what + ": not the oracle's decode through the replica; " + describe(b, np.unique(widx[bad] >> 10)))
            assert (pos[k:] == POISON).all() and (idx[k:] == POISON).all() and (spn[k:] == 0x5A5A5A5A).all(), what + ": written behind the rows"
            matched = int((wpos != NO_MATCH).sum())
            assert 0 < matched < k and int(wspan.max()) >= 2, "matches, misses and a duplicated key are among the rows"
