#!/usr/bin/env python3
"""time_select.py: range selection on the compressed column (alpgpu_select_range_*) against what a caller had to do without it, in one process.

Baseline = the API as it was before the selection: ctx.decode(col, out), then (out >= lo) & (out <= hi) into preallocated masks and
torch.nonzero of the mask on the device (and out[idx] when values are wanted).  It needs 8 (4) bytes of scratch per value for the decoded column;
the selection needs alpgpu_select_scratch_bytes (about 12 bytes per VECTOR).
Columns (1 Mi vectors each): bench.py's mixed ALP column (1 % exceptions plus specials), an all-ALP_RD double column (bench.py "rd"), and a float
column (two decimals, 1 % full-precision values) — the columns of time_gather.py.  Selectivities ~0, 1e-4, 1e-2, 0.1, 0.5 and 1 (bounds = quantiles
of a strided sample of the column around its median; "1" is [-inf, +inf], which leaves out the NaNs), indices only and indices + values, and the
count alone (capacity 0) beside alpgpu_decode_count_range_*.
The two arms ALTERNATE, each warmed up, device events around each arm, REPS repetitions: median ms with the arm's min-max spread beside it.
Model printed with each row: the selection's algorithmic bytes = descriptors + packed words + exception records read once by the count pass and
once more by the emit pass for the vectors with a non-zero count, 12 bytes of scratch per vector written and read, 8 (+ 8 or 4) bytes written per
selected value; over the time, as a fraction of the 8 TB/s HBM peak.
  python3 tools/time_select.py [--vectors N] [--reps R] [--out FILE]"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from alp_amd import capi  # noqa: E402

PEAK = 8.0e12
INF = float("inf")


def alternate(arms, reps, warmup=2):
    """arms: [(name, fn)] run in turn, warmup + reps rounds -> {name: (median, min, max)} in ms"""
    ts = {name: [] for name, _ in arms}
    for r in range(warmup + reps):
        for name, fn in arms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                ts[name].append(a.elapsed_time(b))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ts.items()}


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
    sample = x[::251].cpu().numpy()
    s = np.sort(sample[np.isfinite(sample)])
    col = ctx.encode(x)
    del x
    pb, eb, _ = ctx.column_totals(col)
    nv = col.n_vectors
    n = nv * 1024
    vb = 8 if col.dtype == "f64" else 4
    tdt = torch.float64 if vb == 8 else torch.float32
    out = torch.empty(n, dtype=tdt, device=dev)
    m1 = torch.empty(n, dtype=torch.bool, device=dev)
    m2 = torch.empty(n, dtype=torch.bool, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = ctx.select_scratch(col)
    counts = torch.empty(nv, dtype=torch.int32, device=dev)
    compressed = 32 * nv + pb + eb
    lines.append(f"== {name}: {nv} vectors, {pb / (128.0 * nv):.2f} packed bits per value, {eb / nv:.0f} exception bytes per vector, compressed {compressed / 1e9:.3f} GB")
    lines.append(f"  scratch: baseline {n * vb / 1e9:.3f} GB (the decoded column; + 2 x {n / 1e9:.3f} GB of masks), select {scratch.numel() / 1e6:.3f} MB")
    lines.append(f"  {'selectivity':>11s} {'selected':>11s} {'output':>8s} {'select ms':>24s} {'baseline ms':>24s} {'base/sel':>8s} {'model GB':>9s} {'of peak':>8s}")
    bounds = [("~0", float(s[-1]) + 1e6, float(s[-1]) + 2e6)]
    for f in (1e-4, 1e-2, 0.1, 0.5):
        bounds.append((f"{f:g}", float(s[int((0.5 - f / 2) * s.size)]), float(s[min(s.size - 1, int((0.5 + f / 2) * s.size))])))
    bounds.append(("1", -INF, INF))
    for label, lo, hi in bounds:
        ctx.select_range_into(col, lo, hi, None, count, scratch=scratch)
        k = int(count)
        ctx.decode_count_range(col, lo, hi, counts)
        touched = float((counts != 0).sum()) / nv
        idx = torch.empty(max(k, 1), dtype=torch.int64, device=dev)
        vals = torch.empty(max(k, 1), dtype=tdt, device=dev)
        for with_vals in (False, True):
            base = {}

            def baseline():
                ctx.decode(col, out)
                torch.ge(out, lo, out=m1)
                torch.le(out, hi, out=m2)
                m1.logical_and_(m2)
                base["idx"] = torch.nonzero(m1)
                if with_vals:
                    base["vals"] = out[base["idx"].reshape(-1)]

            def select():
                ctx.select_range_into(col, lo, hi, idx[:k], count, vals[:k] if with_vals else None, scratch=scratch)

            t = alternate([("select", select), ("baseline", baseline)], reps)
            ok = int(count) == k and torch.equal(idx[:k], base["idx"].reshape(-1)) and (not with_vals or torch.equal(vals[:k].view(torch.uint8), base["vals"].view(torch.uint8)))
            model = compressed * (1.0 + touched) + 2 * 12 * nv + k * (8 + (vb if with_vals else 0))
            ts, tb = t["select"], t["baseline"]
            lines.append(f"  {label:>11s} {k:11d} {'idx+val' if with_vals else 'idx':>8s} {ts[0]:9.3f} ({ts[1]:6.3f}-{ts[2]:6.3f}) {tb[0]:9.3f} ({tb[1]:6.3f}-{tb[2]:6.3f}) "
                         f"{tb[0] / ts[0]:8.2f} {model / 1e9:9.3f} {model / (ts[0] * 1e-3) / PEAK:8.3f}{'' if ok else '  WRONG RESULT'}")
            base.clear()
        # the count alone (capacity 0) beside the per-vector counts of alpgpu_decode_count_range_*
        t = alternate([("select", lambda: ctx.select_range_into(col, lo, hi, None, count, scratch=scratch)),
                       ("baseline", lambda: ctx.decode_count_range(col, lo, hi, counts))], reps)
        ts, tb = t["select"], t["baseline"]
        model = compressed + 2 * 12 * nv
        lines.append(f"  {label:>11s} {k:11d} {'count':>8s} {ts[0]:9.3f} ({ts[1]:6.3f}-{ts[2]:6.3f}) {tb[0]:9.3f} ({tb[1]:6.3f}-{tb[2]:6.3f}) {tb[0] / ts[0]:8.2f} "
                     f"{model / 1e9:9.3f} {model / (ts[0] * 1e-3) / PEAK:8.3f}  (baseline here: decode_count_range)")
        del idx, vals
        torch.cuda.empty_cache()
    del col, out, m1, m2
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = capi.Context(0)
    sha = hashlib.sha256(open(os.path.join(ROOT, "alp_amd", "libalpgpu.so"), "rb").read()).hexdigest()[:16]
    lines = [f"time_select.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after 2 warm-ups, device events; "
             f"median (min-max) in ms", f"library sha-256 {sha}; command: python3 tools/time_select.py {' '.join(sys.argv[1:])}".rstrip()]
    for name, make in (("mixed double (bench.py mixed)", lambda: bench.synthetic_input("mixed", a.vectors, dev, seed=1)),
                       ("ALP_RD double (bench.py rd)", lambda: bench.synthetic_input("rd", a.vectors, dev, seed=2)),
                       ("float, two decimals + 1 % exceptions", lambda: float_column(a.vectors, dev))):
        run_column(ctx, name, make(), a.reps, lines)
        print("\n".join(lines[-24:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
