"""GPU: top-k (include/alpgpu.h, "top-k": alpgpu_top_k_*).  The expected result never comes from the code under test: x = ctx.decode(col) on the host
(pinned to the oracle and the reference by other suites) or the oracle's decode of a hand-built encoding, and tests/top_k_replica.py, the definition by
numpy's lexsort on integer views.  Values and indices compare as integers.  Every call goes through `run`, which puts canaries behind the k entries of
both outputs and behind alpgpu_top_k_scratch_bytes of scratch and checks that nothing behind the count and none of them changed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import datagen
from alp_amd import capi
from test_in_list_gpu import COLUMNS, column, random_mask, vectors_cleared
from top_k_replica import host_top_k, unpack_mask

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
INF, NAN = float("inf"), float("nan")
KS = (1, 2, 63, 64, 65, 1000, 1024)
CANARY = 0xA5


def ints(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def run(ctx, col, mask, k, largest, records=None, indices=True):
    """top_k_into with canaries: (values as integers, indices) trimmed to the count"""
    tdt = torch.float64 if col.dtype == "f64" else torch.float32
    vals = torch.full((k + 8,), 7.0, dtype=tdt, device=DEV)
    idx = torch.full((k + 8,), -7, dtype=torch.int64, device=DEV)
    count = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    need = capi.lib.alpgpu_top_k_scratch_bytes(col.n_vectors, k)
    scratch = torch.full((need + 256,), CANARY, dtype=torch.uint8, device=DEV)
    ctx.top_k_into(col, mask, k, vals, count, idx if indices else None, largest=largest, records=records, scratch=scratch)
    n = int(count[0].item())
    assert 0 <= n <= k and int(count[1].item()) == -7
    assert bool((scratch[need:] == CANARY).all()), "the call wrote behind alpgpu_top_k_scratch_bytes"
    assert bool((vals[n:] == 7.0).all()), "values were written at or behind the count"
    assert bool((idx[n:] == -7).all()) and (indices or bool((idx == -7).all())), "indices were written at or behind the count"
    return ints(vals[:n]), idx[:n].cpu().numpy()


def check(ctx, col, xs, mask, k, largest, what, records=None, want=None):
    want_v, want_i = host_top_k(xs, unpack_mask(mask.cpu().numpy()), k, largest) if want is None else want
    got_v, got_i = run(ctx, col, mask, k, largest, records)
    assert got_i.size == want_i.size, f"{what}: count {got_i.size}, expected {want_i.size}"
    assert np.array_equal(got_i, want_i), f"{what}: indices differ first at {np.nonzero(got_i != want_i)[0][:4]}: {got_i[got_i != want_i][:4]} for {want_i[got_i != want_i][:4]}"
    assert np.array_equal(got_v, ints(want_v)), f"{what}: values differ"
    return got_v, got_i


def encode(ctx, x):
    """(DeviceColumn, its decode on the host) of whole vectors of values"""
    x = np.ascontiguousarray(x)
    assert x.size % 1024 == 0
    xd = torch.from_numpy(x).to(DEV)
    col = ctx.encode(xd)
    dec = ctx.decode(col)
    assert torch.equal(dec.view(torch.int64 if x.dtype == np.float64 else torch.int32), xd.view(torch.int64 if x.dtype == np.float64 else torch.int32))
    return col, x


def full_mask(nv):
    return torch.full((16 * nv,), -1, dtype=torch.int64, device=DEV)


def one_bit(nv, r):
    m = torch.zeros(16 * nv, dtype=torch.int64, device=DEV)
    m[r >> 6] = 1 << (r & 63) if (r & 63) < 63 else -(1 << 63)
    return m


# ---- 1. every column kind against the replica ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(COLUMNS))
def test_every_column_kind_against_the_host_replica(ctx, name):
    col, _, xs, _ = column(ctx, name)
    nv = col.n_vectors
    rnd = random_mask(nv, 61)
    masks = {"full": full_mask(nv), "random": rnd, "cleared": vectors_cleared(rnd, 7, 0), "one bit": one_bit(nv, 1024 * (nv // 2) + 321),
             "zero": torch.zeros(16 * nv, dtype=torch.int64, device=DEV)}
    for mname, mask in masks.items():
        bits = unpack_mask(mask.cpu().numpy())
        for largest in (True, False):
            all_v, all_i = host_top_k(xs, bits, 1024, largest)  # the first k of the order are a prefix of its first 1024
            for k in KS:
                got_v, got_i = check(ctx, col, xs, mask, k, largest, f"{name}, {mname} bitmap, k={k}, largest={largest}", want=(all_v[:k], all_i[:k]))
                if mname == "zero":
                    assert got_i.size == 0
                if mname == "one bit":
                    assert got_i.size == (0 if np.isnan(xs[1024 * (nv // 2) + 321]) else 1)
    assert not np.isnan(xs).all()


# ---- 2. ties --------------------------------------------------------------------------------------------------------------------------------------------
def test_a_constant_column_gives_the_lowest_indices(ctx):
    col, xs = encode(ctx, np.full(40 * 1024, 3.5))
    for k in (33, 1024):
        for largest in (True, False):
            _, got_i = check(ctx, col, xs, full_mask(40), k, largest, f"constant column, k={k}, largest={largest}")
            assert got_i.tolist() == list(range(k))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_tie_at_the_vector_threshold_and_more_winners_than_tie_vectors(ctx, dtype):
    """two values; the larger (for smallest: the smaller) occurs once per vector, at a position that moves: with k = 30 the vector level keeps 30 of 40
    tied vectors; with k = 50 all 40 vectors are kept and 10 winners come from the other value, by ascending index"""
    for largest in (True, False):
        x = np.full((40, 1024), 1.25, dtype=dtype)
        for v in range(40):
            x[v, (37 * v + 5) % 1024] = 2.5 if largest else 0.5
        col, xs = encode(ctx, x.reshape(-1))
        for k in (30, 50):
            _, got_i = check(ctx, col, xs, full_mask(40), k, largest, f"two values, k={k}, largest={largest}")
            assert got_i[:min(k, 40)].tolist() == [1024 * v + (37 * v + 5) % 1024 for v in range(min(k, 40))]
        # ... and under a bitmap that clears the single value of every third vector: those vectors' records tie with nothing
        mask = full_mask(40)
        for v in range(0, 40, 3):
            r = 1024 * v + (37 * v + 5) % 1024
            mask[r >> 6] &= ~one_bit(1, r & 63)[0]
        check(ctx, col, xs, mask, 30, largest, f"two values, some singles cleared, largest={largest}")


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zeros_infinities_nans_and_fewer_values_than_k(ctx, dtype):
    # +0.0 / -0.0 alternating: all +0.0 first by ascending index (largest), all -0.0 first (smallest); each keeps its sign
    z = np.zeros(3 * 1024, dtype=dtype)
    z[1::2] = -0.0
    col, xs = encode(ctx, z)
    for k in (5, 1024):
        got_v, got_i = check(ctx, col, xs, full_mask(3), k, True, "alternating zeros, largest")
        assert got_i.tolist() == list(range(0, 2 * k, 2)) and (got_v == 0).all()
        got_v, got_i = check(ctx, col, xs, full_mask(3), k, False, "alternating zeros, smallest")
        assert got_i.tolist() == list(range(1, 2 * k, 2)) and (got_v < 0).all()
    # +-inf among ordinary values, NaN exceptions (quiet and signalling) that a selection skips
    rng = np.random.default_rng(62)
    x = np.round(rng.normal(0, 1000, 6 * 1024), 2).astype(dtype)
    u = np.uint64 if dtype == np.float64 else np.uint32
    snan = np.array([0x7FF0000000000001 if dtype == np.float64 else 0x7F800001], dtype=u).view(dtype)[0]
    x[[7, 1500, 4000]] = INF
    x[[8, 2500]] = -INF
    x[[9, 100, 1024, 5000]] = NAN
    x[[10, 3000]] = snan
    col, xs = encode(ctx, x)
    for largest in (True, False):
        got_v, got_i = check(ctx, col, xs, full_mask(6), 64, largest, f"infinities and NaNs, largest={largest}")
        assert got_i[:2].tolist() == ([7, 1500] if largest else [8, 2500])
    # a selection of NaNs alone gives nothing; NaNs and two numbers give the two numbers (count < k)
    mask = torch.zeros(16 * 6, dtype=torch.int64, device=DEV)
    for r in (9, 10, 100, 1024, 3000, 5000):
        mask[r >> 6] |= one_bit(1, r & 63)[0]
    for largest in (True, False):
        assert check(ctx, col, xs, mask, 10, largest, "NaNs alone")[1].size == 0
    for r in (11, 4001):
        mask[r >> 6] |= one_bit(1, r & 63)[0]
    for largest in (True, False):
        assert check(ctx, col, xs, mask, 10, largest, "NaNs and two numbers")[1].size == 2
    # two non-empty vectors with k = 1024: fewer kept vectors than k, 2048 candidates
    mask = torch.zeros(16 * 6, dtype=torch.int64, device=DEV)
    mask[16:32] = -1
    mask[64:80] = -1
    for largest in (True, False):
        assert check(ctx, col, xs, mask, 1024, largest, "two vectors, k = 1024")[1].size == 1024


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_one_vector_and_a_ragged_last_workgroup(ctx, dtype):
    gen = datagen.mixed_column if dtype == "f64" else datagen.mixed_column_f32
    for nv in (1, 5):
        col, xs = encode(ctx, gen(nv, seed=63 + nv))
        for mask in (full_mask(nv), random_mask(nv, 64)):
            for k in (1, 100, 1024):
                for largest in (True, False):
                    check(ctx, col, xs, mask, k, largest, f"{dtype}, {nv} vectors, k={k}, largest={largest}")


# ---- 3. the candidate bound reached -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["strictly ascending", "one value per vector"])
def test_a_sorted_column_fills_the_candidate_array(ctx, shape):
    """1026 vectors, k = 1024: every vector's record lies above its predecessor's, so 1024 vectors are kept and nearly all of their values (with one value
    per vector: all of them, k * 1024) reach the value part of the vector threshold"""
    nv = 1026
    x = np.arange(nv * 1024, dtype=np.float64) * 0.25 if shape == "strictly ascending" else np.repeat(np.arange(nv, dtype=np.float64) - 500.0, 1024)
    col, xs = encode(ctx, x)
    mask = full_mask(nv)
    _, got_i = check(ctx, col, xs, mask, 1024, True, f"{shape}, largest")
    assert got_i[0] == (nv * 1024 - 1 if shape == "strictly ascending" else (nv - 1) * 1024)
    _, got_i = check(ctx, col, xs, mask, 1024, False, f"{shape}, smallest")
    assert got_i.tolist() == list(range(1024))


# ---- 4. records given ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "adversarial", "rd_unit_f32", "adversarial_f32"])
def test_records_given_are_the_bytes_of_the_call_without(ctx, name):
    col, _, xs, _ = column(ctx, name)
    nv = col.n_vectors
    rnd = vectors_cleared(random_mask(nv, 65), 2, 0)
    full = full_mask(nv)
    tdt = torch.float64 if col.dtype == "f64" else torch.float32
    for k in (1, 100, 1024):
        for largest in (True, False):
            want = check(ctx, col, xs, rnd, k, largest, f"{name}, no records")
            got = run(ctx, col, rnd, k, largest, records=ctx.decode_minmax_masked(col, rnd))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{name}: records of decode_minmax_masked, k={k}, largest={largest}"
            want = check(ctx, col, xs, full, k, largest, f"{name}, full bitmap, no records")
            got = run(ctx, col, full, k, largest, records=ctx.zone_map(col))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{name}: records of zone_map, k={k}, largest={largest}"
            # records that lie: {-inf, +inf} everywhere.  The call returns, writes at most k entries and leaves the canaries alone (run checks that)
            lying = torch.tensor([[-INF, INF]], dtype=tdt, device=DEV).repeat(nv, 1).contiguous()
            got = run(ctx, col, rnd, k, largest, records=lying)
            assert got[1].size <= k
    # ... and records that say "empty" everywhere select nothing
    nothing = torch.tensor([[INF, -INF]], dtype=tdt, device=DEV).repeat(nv, 1).contiguous()
    assert run(ctx, col, full, 100, True, records=nothing)[1].size == 0
    # without indices the values are the same
    want = run(ctx, col, rnd, 100, True)
    got = run(ctx, col, rnd, 100, True, indices=False)
    assert np.array_equal(got[0], want[0])


# ---- 5. every width of the register decode --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["f64", "f32"])
def built(ctx, request):
    import test_register_decode_rows_gpu as rows
    return rows.Columns(ctx, request.param)


def test_every_width_cut_and_exception_class_in_windows_of_kept_vectors(ctx, built):
    """the hand-built columns of tests/test_register_decode_rows_gpu.py; k = 1024 under bitmaps that open at most 1024 consecutive vectors, so every
    vector of a window that holds a selected number is kept and decoded by k_top_k_candidates"""
    rnd = built.masks["random"]
    rnd_bits = built.mask_bits["random"]
    nv = built.nv
    for name, b in (("A", built.A), ("B", built.B)):
        covered = np.zeros(nv, bool)
        for v0 in range(0, nv, 1024):
            v1 = min(nv, v0 + 1024)
            mask = torch.zeros_like(rnd)
            mask[16 * v0:16 * v1] = rnd[16 * v0:16 * v1]
            covered[v0:v1] = True
            for largest in (True, False):
                want_v, want_i = host_top_k(b.want[1024 * v0:1024 * v1], rnd_bits[v0:v1], 1024, largest)
                got_v, got_i = run(ctx, b.col, mask, 1024, largest)
                what = f"{built.dtype} {name}, vectors [{v0}, {v1}), largest={largest}"
                assert np.array_equal(got_i, want_i + 1024 * v0), what + ": indices"
                assert np.array_equal(got_v, ints(want_v)), what + ": values"
        assert covered.all(), "the windows together cover every vector"
        # what the windows kept: every vector with a selected number, which is every class of the rows
        with np.errstate(invalid="ignore"):
            kept = (rnd_bits & ~np.isnan(b.values)).any(axis=1)
        e = b.enc
        assert sorted(set(e["bw"][b.alp & kept].tolist())) == list(range(built.value_bits + 1))
        assert sorted(set(zip(e["bw"][~b.alp & kept].tolist(), e["lbw"][~b.alp & kept].tolist()))) == sorted(built.rows.rd_cuts())
        assert sorted(set(e["exc_cnt"][b.alp & kept].tolist())) == sorted(built.rows.ALP_EXC_COUNTS)


# ---- 6. determinism and statelessness -------------------------------------------------------------------------------------------------------------------
def test_the_same_call_gives_the_same_bytes(ctx):
    col, _, xs, _ = column(ctx, "mixed")
    mask = random_mask(col.n_vectors, 66)
    runs = []
    for rep in range(2):
        torch.empty(1 << (20 + rep), dtype=torch.uint8, device=DEV).fill_(rep)  # (a different allocation history each time)
        runs.append(tuple(a.tobytes() for k in (1, 100, 1024) for largest in (True, False) for a in run(ctx, col, mask, k, largest)))
    assert runs[0] == runs[1]


def test_top_k_leaves_the_decode_plan_alone(ctx):
    cols = [ctx.encode(torch.from_numpy(datagen.mixed_column(150, seed=s)).to(DEV)) for s in (96, 97)]
    ctx.column_totals(cols[0])  # one hinted, one not
    for col in cols:
        ctx.decode(col)
    ctx.synchronize()  # (what an unhinted decode learns about the column is in by now)
    before = [ctx.decode_plan(col) for col in cols]
    mask = random_mask(150, 52)
    for col in cols:
        ctx.top_k(col, mask, 100)
        ctx.top_k(col, mask, 1024, largest=False, records=ctx.decode_minmax_masked(col, mask))
    ctx.synchronize()
    assert [ctx.decode_plan(col) for col in cols] == before


# ---- 7. graph capture -----------------------------------------------------------------------------------------------------------------------------------
CAPTURE = r"""
import sys
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
import datagen
from alp_amd import capi
from top_k_replica import host_top_k, unpack_mask
ctx = capi.Context(0)
side = torch.cuda.Stream()
ok = True
nv, k = 230, 100
x = datagen.mixed_column(nv, seed=81)
col = ctx.encode(torch.from_numpy(x).cuda())
prior = torch.from_numpy(np.random.default_rng(85).integers(0, 2**64, 16 * nv, dtype=np.uint64).view(np.int64)).cuda()
mask = torch.zeros(16 * nv, dtype=torch.int64, device="cuda:0")
vals = torch.zeros(k, dtype=torch.float64, device="cuda:0")
idx = torch.zeros(k, dtype=torch.int64, device="cuda:0")
count = torch.zeros(1, dtype=torch.int64, device="cuda:0")
scratch = ctx.top_k_scratch(col, k)
def calls():
    ctx.top_k_into(col, mask, k, vals, count, idx, largest=False, scratch=scratch)   # everything on the one stream: the graph is a chain
with torch.cuda.stream(side):
    mask.copy_(prior)
    calls()          # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        calls()
for rep in range(2):
    if rep == 1:
        prior = ~prior
        prior[16 * 5:16 * 9] = 0
    torch.cuda.synchronize()
    mask.copy_(prior); vals.fill_(7.0); idx.fill_(-7); count.fill_(-7); scratch.fill_(rep)
    g.replay()
    torch.cuda.synchronize()
    want_v, want_i = host_top_k(x, unpack_mask(prior.cpu().numpy()), k, False)
    n = int(count.item())
    ok = ok and torch.equal(mask, prior) and n == want_i.size == k
    ok = ok and np.array_equal(idx.cpu().numpy()[:n], want_i) and np.array_equal(vals.cpu().numpy()[:n].view(np.int64), want_v.view(np.int64))
    print(rep, n, want_i[:4].tolist(), ok)
print("RESULT", ok)
""" % (ROOT, os.path.join(ROOT, "tests"))


def test_captured_into_a_graph_and_replayed_after_the_bitmap_changes():
    p = subprocess.run([sys.executable, "-c", CAPTURE], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert p.returncode == 0 and line == ["RESULT True"], p.stdout[-2000:] + p.stderr[-3000:]


# ---- 8. argument checks ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_c_argument_checks(ctx, dtype):
    col, _, xs, _ = column(ctx, "mixed" if dtype == "f64" else "mixed_f32")
    nv = col.n_vectors
    tk = getattr(capi.lib, "alpgpu_top_k_" + dtype)
    tdt = torch.float32 if dtype == "f32" else torch.float64
    mask = torch.full((16 * nv + 16,), -1, dtype=torch.int64, device=DEV)
    vals = torch.full((1100,), 7.0, dtype=tdt, device=DEV)
    idx = torch.full((1100,), -7, dtype=torch.int64, device=DEV)
    count = torch.full((2,), -7, dtype=torch.int64, device=DEV)
    records = torch.full((nv + 1, 2), 7.0, dtype=tdt, device=DEV)
    scratch = torch.full((capi.lib.alpgpu_top_k_scratch_bytes(nv, 1024) + 64,), CANARY, dtype=torch.uint8, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    V, M, R, X, I, N, S = ctypes.byref(col.c), p(mask), p(records), p(vals), p(idx), p(count), p(scratch)
    bare = capi.CColumn()
    bare.n_vectors = nv  # a column without descriptors
    huge = capi.CColumn()
    huge.n_vectors = 2**32
    refused = [
        tk(None, V, M, R, 10, 1, X, I, N, S), tk(ctx.h, None, M, R, 10, 1, X, I, N, S), tk(ctx.h, V, None, R, 10, 1, X, I, N, S),
        tk(ctx.h, V, M, R, 10, 1, None, I, N, S), tk(ctx.h, V, M, R, 10, 1, X, I, None, S), tk(ctx.h, V, M, R, 10, 1, X, I, N, None),
        tk(ctx.h, V, M, R, 1025, 1, X, I, N, S), tk(ctx.h, V, M, R, 2**64 - 1, 1, X, I, N, S),
        tk(ctx.h, V, M, p(records, 8), 10, 1, X, I, N, S), tk(ctx.h, V, M, R, 10, 1, X, I, N, p(scratch, 8)), tk(ctx.h, V, M, None, 10, 1, X, I, N, p(scratch, 4)),
        tk(ctx.h, V, p(mask, 4), R, 10, 1, X, I, N, S), tk(ctx.h, ctypes.byref(bare), M, R, 10, 1, X, I, N, S), tk(ctx.h, ctypes.byref(huge), M, R, 10, 1, X, I, N, S),
        # the errors come before the early exits: k == 0 and an empty column still need their pointers
        tk(ctx.h, V, M, R, 0, 1, None, I, N, S), tk(ctx.h, V, M, R, 0, 1, X, I, None, S), tk(None, V, M, R, 0, 1, X, I, N, S),
    ]
    assert refused == [-2] * len(refused), refused
    ctx.synchronize()
    untouched = lambda: bool((mask == -1).all()) and bool((vals == 7.0).all()) and bool((idx == -7).all()) and bool((records == 7.0).all()) and bool((scratch == CANARY).all())
    assert untouched() and bool((count == -7).all()), "a refused call wrote"
    # k == 0 and an empty column: ALPGPU_OK, the count alone is written
    empty = capi.CColumn()
    for c_, k_ in ((V, 0), (ctypes.byref(empty), 10), (ctypes.byref(empty), 0)):
        count.fill_(-7)
        assert tk(ctx.h, c_, M, None, k_, 1, X, I, N, S) == 0
        ctx.synchronize()
        assert count.tolist() == [0, -7] and untouched()
    # d_idx is optional; the bound itself is accepted
    count.fill_(-7)
    assert tk(ctx.h, V, M, None, 1024, 0, X, None, N, S) == 0
    ctx.synchronize()
    assert count.tolist() == [1024, -7] and bool((idx == -7).all()) and bool((vals[1024:] == 7.0).all())
    assert bool((scratch[-64:] == CANARY).all())
    want_v, _ = host_top_k(xs, np.ones(xs.size, bool), 1024, False)
    assert np.array_equal(ints(vals[:1024]), ints(want_v))


def test_python_rejects_arguments_that_do_not_fit(ctx, monkeypatch):
    col, _, _, _ = column(ctx, "mixed")
    cf, _, _, _ = column(ctx, "mixed_f32")
    nv = col.n_vectors
    mask = torch.full((16 * nv,), 7, dtype=torch.int64, device=DEV)
    vals = torch.full((64,), 7.0, dtype=torch.float64, device=DEV)
    idx = torch.full((64,), 7, dtype=torch.int64, device=DEV)
    count = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    records = torch.full((nv, 2), 7.0, dtype=torch.float64, device=DEV)
    scratch = ctx.top_k_scratch(col, 64)

    def unreachable(*a, **k):
        raise AssertionError("the library was called")
    for t in ("f64", "f32"):
        monkeypatch.setattr(capi.lib, "alpgpu_top_k_" + t, unreachable)
    ok = dict(col=col, mask=mask, k=64, vals_out=vals, count_out=count, idx_out=idx, records=records, scratch=scratch)

    def rejected(**change):
        with pytest.raises(ValueError):
            ctx.top_k_into(**{**ok, **change})
    wide = torch.full((32 * nv,), 7, dtype=torch.int64, device=DEV)
    for bad in (mask.to(torch.int32), mask.cpu(), mask[:-16], wide, wide[::2], mask.reshape(nv, 16), [1, 2, 3], np.zeros(16 * nv, np.int64)):
        rejected(mask=bad)
    for bad in (-1, 1025, 2**40, 1.5, "3", None, True):
        rejected(k=bad)
        with pytest.raises(ValueError):
            ctx.top_k(col, mask, bad)
        with pytest.raises(ValueError):
            ctx.top_k_scratch(col, bad)
    for bad in (vals.to(torch.float32), vals.cpu(), vals[:63], vals[::2], None, [1.0]):
        rejected(vals_out=bad)
    for bad in (idx.to(torch.int32), idx.cpu(), idx[:63], idx[::2]):
        rejected(idx_out=bad)
    for bad in (count.to(torch.int32), count.cpu(), count[:0], None):
        rejected(count_out=bad)
    unaligned = torch.zeros(2 * nv + 1, dtype=torch.float64, device=DEV)[1:].reshape(nv, 2)
    for bad in (records.to(torch.float32), records.cpu(), records[:-1], records.reshape(-1), records.t(), unaligned):
        rejected(records=bad)
    for bad in (scratch.to(torch.int8), scratch.cpu(), scratch[:-1], torch.zeros(scratch.numel() + 16, dtype=torch.uint8, device=DEV)[8:]):
        rejected(scratch=bad)
    rejected(scratch=ctx.top_k_scratch(col, 63)[:capi.lib.alpgpu_top_k_scratch_bytes(nv, 63)], k=64)  # a scratch made for a smaller k
    rejected(col=cf)  # a float column's values and records are floats
    ctx.synchronize()
    assert bool((mask == 7).all()) and bool((vals == 7.0).all()) and bool((idx == 7).all()) and bool((count == 7).all()) and bool((records == 7.0).all())


# ---- 9. the C++ wrapper ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_cpp_column_top_k_against_decompress_and_a_partial_sort(ctx, tmp_path, dtype):
    """include/alp/batch.hpp: alp::gpu::column<double / float>::top_k of a serialized column against column::decompress and a host std::partial_sort
    with the same comparator (tests/cpp/top_k_test.cpp)"""
    exe = tmp_path / "top_k_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", f"-I{ROOT}/include", "-o", str(exe), f"{ROOT}/tests/cpp/top_k_test.cpp",
                           f"-L{ROOT}/alp_amd", "-lalpgpu", "-ldl", f"-Wl,-rpath,{ROOT}/alp_amd"])
    col, x, _, _ = column(ctx, "adversarial" if dtype == "f64" else "adversarial_f32")  # NaN, +-inf and -0.0 among the values
    ctx.to_blob(col, x.numel()).tofile(str(tmp_path / "col.blob"))
    mask = vectors_cleared(random_mask(col.n_vectors, 67), 3, -1)
    mask[16:32] = 0
    mask.cpu().numpy().tofile(str(tmp_path / "in.mask"))
    p = subprocess.run([str(exe), dtype, str(tmp_path / "col.blob"), str(tmp_path / "in.mask")], capture_output=True, text=True, timeout=600)
    line = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("ok ")]
    assert p.returncode == 0 and len(line) == 1, p.stdout[-3000:] + p.stderr[-2000:]
    assert int(line[0][1]) == col.n_vectors and int(line[0][2]) > 0
