#!/usr/bin/env python3
"""time_gather.py: random access (alpgpu_gather_*, alpgpu_decode_slice_*) against the store decode (alpgpu_decode_*) of the same column, in one process.

Columns (1 Mi vectors each): bench.py's mixed ALP column (1 % exceptions plus specials), an all-ALP_RD double column (bench.py "rd"), and a float column
(two decimals, 1 % full-precision values).  Timed with device events, each case warmed up, then REPS repetitions: median, min and max in ms.
  gather     k = 2^10 .. 2^26 indices: uniformly random, the same sorted, runs of 64 consecutive indices at random starts
  slice      the whole column from first = 0 (vector-aligned) and from first = 517 (n - 517 values)
  decode     alpgpu_decode_* of the column
Derived: the random-index rate (indices / s at the largest k), the crossover k at which a random gather costs as much as the full decode (log-log
interpolation between the measured k) as a count and as a fraction of the column's values, and slice / decode as fractions of the 8 TB/s HBM peak
over the same algorithmic bytes (descriptors + packed words + exception records read, every value written once).
  python3 tools/time_gather.py [--vectors N] [--reps R] [--out FILE]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from alp_amd import capi  # noqa: E402

PEAK = 8.0e12


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def float_column(nv, dev, seed=3):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.rand(nv * 1024, dtype=torch.float64, device=dev, generator=g) * 2e3 - 1e3
    out = (torch.round(x * 100.0) / 100.0).to(torch.float32)
    m = torch.rand(nv * 1024, device=dev, generator=g) < 0.01
    out[m] = (x[m] * 3.141592653589793).to(torch.float32)
    return out


def run_column(ctx, name, x, reps, lines):
    dev = x.device
    col = ctx.encode(x)
    del x
    pb, eb, _ = ctx.column_totals(col)
    nv = col.n_vectors
    n = nv * 1024
    vb = 8 if col.dtype == "f64" else 4
    tdt = torch.float64 if vb == 8 else torch.float32
    out = torch.empty(n, dtype=tdt, device=dev)
    algo_bytes = 32 * nv + pb + eb + n * vb
    t_dec = timed(lambda: ctx.decode(col, out), reps)
    ref = out.clone()
    lines.append(f"== {name}: {nv} vectors, {pb / (128.0 * nv):.2f} packed bits per value, {eb / nv:.0f} exception bytes per vector")
    lines.append(f"  decode            {t_dec[0]:9.3f} ms  (min {t_dec[1]:.3f}, max {t_dec[2]:.3f})  {algo_bytes / (t_dec[0] * 1e-3) / PEAK:.3f} of 8 TB/s")
    for first in (0, 517):
        m = n - first
        t = timed(lambda: ctx.decode_slice(col, first, m, out), reps)
        ok = torch.equal(out[:m].view(torch.uint8), ref[first:].view(torch.uint8))
        lines.append(f"  slice first={first:<4d}  {t[0]:9.3f} ms  (min {t[1]:.3f}, max {t[2]:.3f})  {algo_bytes / (t[0] * 1e-3) / PEAK:.3f} of 8 TB/s, "
                     f"{t[0] / t_dec[0]:.2f} x decode{'' if ok else '  WRONG BITS'}")
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    random_t = []
    lines.append(f"  {'k':>9s} {'random ms':>10s} {'sorted ms':>10s} {'runs64 ms':>10s} {'random idx/s':>13s}  (median; min-max random)")
    for lk in range(10, 27, 2):
        k = 1 << lk
        idx = torch.randint(0, n, (k,), dtype=torch.int64, device=dev, generator=g)
        srt = torch.sort(idx).values
        starts = torch.randint(0, n - 64, (k // 64,), dtype=torch.int64, device=dev, generator=g)
        runs = (starts[:, None] + torch.arange(64, device=dev)[None, :]).reshape(-1)
        gout = torch.empty(k, dtype=tdt, device=dev)
        res = []
        for ix in (idx, srt, runs):
            res.append(timed(lambda ix=ix: ctx.gather(col, ix, gout), reps))
            assert torch.equal(gout.view(torch.uint8), ref[ix].view(torch.uint8)), f"{name}: gather of {k} differs from the decode"
        random_t.append((k, res[0][0]))
        lines.append(f"  {k:9d} {res[0][0]:10.4f} {res[1][0]:10.4f} {res[2][0]:10.4f} {k / (res[0][0] * 1e-3):13.3e}  ({res[0][1]:.4f}-{res[0][2]:.4f})")
        del idx, srt, starts, runs, gout
    # crossover: first measured k whose random gather is not faster than the decode, interpolated in log-log against the one before
    cross = None
    for (k0, t0), (k1, t1) in zip(random_t, random_t[1:]):
        if t0 < t_dec[0] <= t1:
            cross = float(np.exp(np.log(k0) + (np.log(t_dec[0]) - np.log(t0)) * (np.log(k1) - np.log(k0)) / (np.log(t1) - np.log(t0))))
    kmax, tmax = random_t[-1]
    rate = kmax / (tmax * 1e-3)
    if cross is None:
        lines.append(f"  crossover: beyond the largest k measured ({kmax} = {kmax / n:.4f} of the values; random gather there {tmax / t_dec[0]:.2f} x decode)")
    else:
        lines.append(f"  crossover: a random gather of ~{cross:.3e} indices ({cross / n:.4f} of the values) costs one decode")
    lines.append(f"  random-index rate at k = 2^26: {rate:.3e} indices/s")
    del col, out, ref
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = capi.Context(0)
    lines = [f"time_gather.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, {a.reps} repetitions after 3 warm-ups, device events"]
    for name, make in (("mixed double (bench.py mixed)", lambda: bench.synthetic_input("mixed", a.vectors, dev, seed=1)),
                       ("ALP_RD double (bench.py rd)", lambda: bench.synthetic_input("rd", a.vectors, dev, seed=2)),
                       ("float, two decimals + 1 % exceptions", lambda: float_column(a.vectors, dev))):
        run_column(ctx, name, make(), a.reps, lines)
        print("\n".join(lines[-15:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
