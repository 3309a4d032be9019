"""Round 6: the whole-column entry points captured into a hipGraph and replayed (the library enqueues on the caller's stream and forks / joins its
second stream with events, so a stream capture around a call records all of it).  Every scenario runs in a process of its own: a capture that fails leaves the
process's stream in a state no later test should inherit.  Each prints RESULT <ok> <detail>; the bytes a replay writes must be the bytes the eager call writes."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEAD = r"""
import sys, time
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import numpy as np
import torch
import bench
import datagen
from alp_amd import capi
ctx = capi.Context(0)
side = torch.cuda.Stream()
def same(a, b):
    return bool(torch.equal(a.view(torch.uint8), b.view(torch.uint8)))
""" % (ROOT, os.path.join(ROOT, "tests"))

SCENARIOS = {
    # a hinted column of every packed width by rowgroup, 20 exceptions per vector: the plain store decode (one launch)
    "decode": r"""
col, _, _ = bench.build_decode_column(5300, 0, seed=3, exc_per_vec=20)
ref = ctx.decode(col).clone()
out = torch.zeros_like(ref)
with torch.cuda.stream(side):
    ctx.decode(col, out)          # warm-up on the capture stream
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.decode(col, out)
ok = True
for _ in range(3):
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    ok = ok and same(out, ref)
print("RESULT", ok, "replays of the store decode")
""",
    # the read-ahead forced on: the fork to the context's second stream and the join are part of the capture
    "decode_read_ahead": r"""
n = 40000
col, _, _ = bench.build_decode_column(n, 0, seed=5, bw_of_rowgroup=4, exc_per_vec=20)
ctx.set_option(capi.OPT_DECODE_READ_AHEAD, 0)
ref = ctx.decode(col).clone()
ctx.set_option(capi.OPT_DECODE_READ_AHEAD, 1)
assert ctx.decode_reads_ahead(col)
out = torch.zeros_like(ref)
with torch.cuda.stream(side):
    ctx.decode(col, out)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.decode(col, out)
ok = True
for _ in range(4):
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    ok = ok and same(out, ref)
ctx.decode(col, out)              # and the context still works eagerly afterwards, read-ahead and all
torch.cuda.synchronize()
print("RESULT", ok and same(out, ref), "replays of the store decode with its read-ahead")
""",
    # the fused consumers
    "sum_and_count": r"""
col, _, _ = bench.build_decode_column(5300, 0, seed=4, exc_per_vec=20)
sums_ref = ctx.decode_sum(col).clone()
cnt_ref = ctx.decode_count_range(col, -1.0e3, 1.0e3).clone()
sums, cnt = torch.zeros_like(sums_ref), torch.zeros_like(cnt_ref)
with torch.cuda.stream(side):
    ctx.decode_sum(col, sums); ctx.decode_count_range(col, -1.0e3, 1.0e3, cnt)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.decode_sum(col, sums)
        ctx.decode_count_range(col, -1.0e3, 1.0e3, cnt)
ok = True
for _ in range(3):
    sums.zero_(); cnt.zero_()
    g.replay()
    torch.cuda.synchronize()
    ok = ok and same(sums, sums_ref) and same(cnt, cnt_ref)
print("RESULT", ok, "replays of SUM and COUNT")
""",
    # encode + decode of a small column as ONE graph (the launch-bound case): the rowgroup search on the second stream, the vector encode, the gated recovery
    # kernels and the decode; replayed over new input in the same buffers
    "encode_decode": r"""
n = 700
xs = [torch.from_numpy(np.concatenate([datagen.mixed_column(400, seed=s), datagen.rd_column(200, seed=s + 1), datagen.drifting_column(100, seed=s + 2)])).cuda() for s in (11, 21, 31)]
x = xs[0].clone()
col = capi.DeviceColumn(n, 0)
out = torch.zeros_like(x)
eager = []
for xi in xs:                     # eager: the streams each input must give
    x.copy_(xi)
    ctx.encode(x, col)
    ctx.synchronize()
    eager.append([t.copy() for t in col.to_host()])
with torch.cuda.stream(side):
    ctx.encode(x, col); ctx.decode(col, out)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.encode(x, col)
        ctx.decode(col, out)
ok = True
for xi, want in zip(xs, eager):
    x.copy_(xi)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    ok = ok and same(out, xi)
    got = col.to_host()
    ok = ok and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, want))
t0 = time.perf_counter()
for _ in range(20):
    g.replay()
torch.cuda.synchronize()
t_graph = (time.perf_counter() - t0) / 20
t0 = time.perf_counter()
for _ in range(20):
    ctx.encode(x, col); ctx.decode(col, out)
torch.cuda.synchronize()
t_eager = (time.perf_counter() - t0) / 20
print("RESULT", ok, "encode+decode of %%d vectors: %%.0f us per replay, %%.0f us eager" %% (n, t_graph * 1e6, t_eager * 1e6))
""",
    # columns long enough for the unhinted decode (>= 65 536 vectors, both hints 0: sizes summed and the shape chosen on the stream), double and float, captured with
    # nothing learned before: replays write the eager bytes, the capture leaves the context nothing to plan from, and what it learns eagerly afterwards is the truth
    "unhinted_decode": r"""
ok = True
ref_ctx = capi.Context(0)
for vb in (8, 4):
    col, _, _ = bench.build_decode_column(70000, 0, seed=13, exc_per_vec=20, value_bytes=vb)
    col.c.packed_bytes_hint = col.c.exc_bytes_hint = col.c.alp_rd_rowgroups_hint = 0
    ref = ref_ctx.decode(col).clone()     # (another context: this one learns nothing before the capture; the kernels are loaded)
    torch.cuda.synchronize()
    out = torch.zeros_like(ref)
    with torch.cuda.stream(side):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            ctx.decode(col, out)
    for _ in range(3):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        ok = ok and same(out, ref)
    ok = ok and ctx.decode_plan(col) is None  # nothing to plan from: the capture learned nothing
    for _ in range(2):                        # eager: the first decode learns, the second is planned from what it learned
        out.zero_()
        ctx.decode(col, out)
        torch.cuda.synchronize()
        ok = ok and same(out, ref)
    learned = ctx.decode_plan(col)
    out.zero_()
    g.replay()                                # a replay after them leaves what the context learned alone
    torch.cuda.synchronize()
    ok = ok and same(out, ref) and ctx.decode_plan(col) == learned
    pb, eb, _ = ref_ctx.column_totals(col)
    ok = ok and learned is not None and (learned["packed_bytes"], learned["exc_bytes"]) == (pb, eb)
    dcol = ctx.encode(ref)                    # and an eager encode + decode of the same values
    back = ctx.decode(dcol)
    torch.cuda.synchronize()
    ok = ok and same(back, ref)
    print(vb, ok, learned, pb, eb)
    del g
print("RESULT", ok, "replays of unhinted decodes, then eager ones")
""",
    # an eager unhinted decode (its sizes on their way to the host) and right behind it a capture of encode + decode of the same column: the encode forgets what the
    # context learned about the column inside the capture, without waiting for it; replays over three inputs give the eager streams and the input's bits
    "encode_decode_after_unhinted": r"""
n = 70000
gen = torch.Generator(device="cuda:0")
def make(seed):
    gen.manual_seed(seed)
    x = torch.round(torch.rand(n * 1024, dtype=torch.float64, device="cuda:0", generator=gen) * 1e4, decimals=2)
    x[::97] = torch.rand(x[::97].shape, dtype=torch.float64, device="cuda:0", generator=gen)  # exceptions
    x[n // 2 * 1024:] = torch.rand(n * 1024 - n // 2 * 1024, dtype=torch.float64, device="cuda:0", generator=gen)  # full precision: ALP_RD rowgroups
    return x
def streams(c):
    tot = c.totals.cpu()
    return [c.rowgroups.clone(), c.vectors.clone(), c.packed[: int(tot[0])].clone(), c.exc[: int(tot[1])].clone()]
xs = [make(s) for s in (1, 2, 3)]
x = xs[0].clone()
col = capi.DeviceColumn(n)
out = torch.zeros_like(x)
eager = []
for xi in xs:
    x.copy_(xi)
    ctx.encode(x, col)
    eager.append(streams(col))
x.copy_(xs[0])
with torch.cuda.stream(side):
    ctx.encode(x, col)
    ctx.decode(col, out)                  # unhinted: the sizes travel to the host behind it
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.encode(x, col)
        ctx.decode(col, out)
ok = True
for xi, want in zip(xs, eager):
    x.copy_(xi)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    ok = ok and same(out, xi) and all(torch.equal(a, b) for a, b in zip(streams(col), want))
for _ in range(2):                        # eager afterwards: learns, then decodes from what it learned
    ctx.encode(x, col)
    out.zero_()
    ctx.decode(col, out)
    torch.cuda.synchronize()
    ok = ok and same(out, x)
print("RESULT", ok, "capture of encode + decode behind an eager unhinted decode")
""",
    # encode + decode of a >= 70 000-vector mixed double column and a float column in one graph: several look-back tiles and more than one fused launch each
    "encode_decode_long": r"""
n = 70000
gen = torch.Generator(device="cuda:0")
def make(seed):
    gen.manual_seed(seed)
    x = torch.round(torch.rand(n * 1024, dtype=torch.float64, device="cuda:0", generator=gen) * 1e4, decimals=2)
    x[::89] = torch.rand(x[::89].shape, dtype=torch.float64, device="cuda:0", generator=gen)
    x[2 * n // 5 * 1024: 3 * n // 5 * 1024] = torch.rand(n // 5 * 1024, dtype=torch.float64, device="cuda:0", generator=gen)
    return x, torch.round(x[: n * 1024].float(), decimals=1)
def streams(c):
    tot = c.totals.cpu()
    return [c.rowgroups.clone(), c.vectors.clone(), c.packed[: int(tot[0])].clone(), c.exc[: int(tot[1])].clone()]
inputs = [make(s) for s in (4, 5, 6)]
x, y = inputs[0][0].clone(), inputs[0][1].clone()
cx, cy = capi.DeviceColumn(n), capi.DeviceColumn(n, dtype="f32")
ox, oy = torch.zeros_like(x), torch.zeros_like(y)
eager = []
for xi, yi in inputs:
    x.copy_(xi); y.copy_(yi)
    ctx.encode(x, cx); ctx.encode(y, cy)
    eager.append((streams(cx), streams(cy)))
with torch.cuda.stream(side):
    ctx.encode(x, cx); ctx.decode(cx, ox); ctx.encode(y, cy); ctx.decode(cy, oy)
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        ctx.encode(x, cx); ctx.decode(cx, ox)
        ctx.encode(y, cy); ctx.decode(cy, oy)
ok = True
for (xi, yi), (wx, wy) in zip(inputs, eager):
    x.copy_(xi); y.copy_(yi)
    ox.zero_(); oy.zero_()
    g.replay()
    torch.cuda.synchronize()
    ok = ok and same(ox, xi) and same(oy, yi)
    ok = ok and all(torch.equal(a, b) for a, b in zip(streams(cx), wx)) and all(torch.equal(a, b) for a, b in zip(streams(cy), wy))
print("RESULT", ok, "replays of encode + decode of %%d-vector double and float columns" %% n)
""",
}


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_entry_points_captured_into_a_graph_replay_the_same_bytes(name):
    p = subprocess.run([sys.executable, "-c", HEAD + SCENARIOS[name].replace("%%", "%")], capture_output=True, text=True, timeout=300)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")]
    assert line, (name, p.stdout[-1500:], p.stderr[-3000:])
    print(line[-1])
    assert line[-1].split()[1] == "True", (name, line[-1])
