#!/usr/bin/env python3
"""time_top_k.py: top-k (alpgpu_top_k_*: ORDER BY x [DESC] LIMIT k over a compressed column under a bitmap) against the route a caller had without
it, in one process.

Columns: bench.py's mixed ALP column, the all-ALP_RD double column (bench.py "rd"), the float column of time_select.py, and the sorted
two-decimal column of time_zone.py (every vector's record above its predecessor's: k kept vectors fill the candidate array).
Per uniformly random bitmap of density in {1, 0.1, 1e-2} and k in {1, 100, 1024}, the largest k:
  new       top_k_into(col, bitmap, k) with NULL records: one decode_minmax_masked pass, the selects, the candidates of at most k vectors, the sort
  records   the same with the records of decode_minmax_masked prepared ahead (outside the timed region)
  today     decode_masked(col, bitmap) into a buffer, torch.topk over it (a NaN-free column is assumed in its favour; indices not produced)
Arms ALTERNATE, each warmed up, device events around each arm: median ms with the arm's min-max spread.  The new calls' values are compared with
today's, bit for bit.
  python3 tools/time_top_k.py [--vectors N] [--reps R] [--out FILE]"""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
from alp_amd import capi  # noqa: E402
from time_mask import fmt  # noqa: E402
from time_select import alternate, float_column  # noqa: E402
from time_take_masked import ibits, random_bitmap  # noqa: E402
from time_zone import sorted_column  # noqa: E402

KS = (1, 100, 1024)
DENSITIES = (1.0, 0.1, 1e-2)


def run_column(ctx, name, col, reps, emit):
    dev = torch.device(f"cuda:{ctx.device}")
    nv = col.n_vectors
    tdt = torch.float64 if col.dtype == "f64" else torch.float32
    pa, ea, _ = ctx.column_totals(col)
    emit(f"== {name}: {nv} vectors, {pa / (128.0 * nv):.2f} packed bits per value, compressed {(32 * nv + pa + ea) / 1e9:.3f} GB, bitmap {128 * nv / 1e6:.1f} MB")
    mask = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    buf = torch.empty(nv * 1024, dtype=tdt, device=dev)
    n_sel = torch.empty(1, dtype=torch.int64, device=dev)
    sel_scratch = ctx.select_scratch(col)
    scratch = ctx.top_k_scratch(col, max(KS))
    records = torch.empty((nv, 2), dtype=tdt, device=dev)
    emit(f"  {'density':>7s} {'k':>5s} {'new ms':>28s} {'records ms':>28s} {'today ms':>28s} {'today/new':>9s} {'today/records':>13s}  new beats today by more than the spreads")
    for i, d in enumerate(DENSITIES):
        random_bitmap(mask, nv, d, False, 70 + i)
        ctx.decode_minmax_masked(col, mask, out=records)
        for k in KS:
            vals = [torch.empty(k, dtype=tdt, device=dev) for _ in range(2)]
            idx = torch.empty(k, dtype=torch.int64, device=dev)
            count = torch.empty(1, dtype=torch.int64, device=dev)
            today_vals = [None]

            def new():
                ctx.top_k_into(col, mask, k, vals[0], count, idx, scratch=scratch)

            def with_records():
                ctx.top_k_into(col, mask, k, vals[1], count, idx, records=records, scratch=scratch)

            def today():
                ctx.decode_masked_into(col, mask, buf, n_sel, scratch=sel_scratch)
                n = int(n_sel.item())  # (the read-back today's route cannot avoid: torch.topk needs the length)
                today_vals[0] = torch.topk(buf[:n], min(k, n)).values

            t = alternate([("new", new), ("records", with_records), ("today", today)], reps, warmup=1)
            n = min(int(count.item()), k)
            note = ""
            if bool(torch.isnan(today_vals[0]).any()):
                note = "  (today's result holds a NaN: not compared)"
            elif not (n == today_vals[0].numel() and torch.equal(ibits(vals[0][:n]), ibits(today_vals[0])) and torch.equal(ibits(vals[1][:n]), ibits(today_vals[0]))):
                # (torch.topk does not order -0.0 and +0.0: a difference there alone is not an error of either route)
                same = n == today_vals[0].numel() and torch.equal(vals[0][:n], today_vals[0]) and torch.equal(vals[1][:n], today_vals[0])
                note = "  (differs from today's only in the signs of zeros)" if same else "  WRONG RESULT"
            tn, tr, tt = t["new"], t["records"], t["today"]
            spread = max(tn[2] - tn[1], tt[2] - tt[1])
            emit(f"  {d:7g} {k:5d} {fmt(tn)} {fmt(tr)} {fmt(tt)} {tt[0] / tn[0]:9.2f} {tt[0] / tr[0]:13.2f}  "
                 f"{'yes' if tt[0] - tn[0] > spread else 'NO'} ({tt[0] - tn[0]:+.3f} ms, spread {spread:.3f} ms){note}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = capi.Context(0)
    sha = hashlib.sha256(open(capi.lib._name, "rb").read()).hexdigest()[:16]
    out = open(a.out, "w") if a.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    emit(f"time_top_k.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after the warm-up, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_top_k.py {' '.join(sys.argv[1:])}".rstrip())
    nv = a.vectors
    kinds = (("mixed double (bench.py mixed)", lambda: bench.synthetic_input("mixed", nv, dev, seed=1)),
             ("ALP_RD double (bench.py rd)", lambda: bench.synthetic_input("rd", nv, dev, seed=1)),
             ("float, two decimals + 1 % exceptions", lambda: float_column(nv, dev, seed=1)),
             ("sorted double, two decimals", lambda: sorted_column(nv, dev)))
    for name, make in kinds:
        x = make()
        col = ctx.encode(x)
        del x
        run_column(ctx, name, col, a.reps, emit)
        del col
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
