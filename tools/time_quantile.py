#!/usr/bin/env python3
"""time_quantile.py: the quantiles (alpgpu_quantile_*: exact order statistics of a compressed column under a bitmap) against the route a caller had
without them, in one process.

Columns: bench.py's mixed ALP column, the all-ALP_RD double column (bench.py "rd"), the float column of time_select.py, the sorted two-decimal column
of time_zone.py, and a constant column: the declared worst case, which never fits the candidate capacity and takes every decode pass.
Per uniformly random bitmap of density in {1, 0.1, 1e-2} and q in {the median, 16 quantiles}:
  new       quantile_into(col, bitmap, q) with NULL zones
  zoned     the same with the records of zone_map prepared ahead (outside the timed region)
  today     decode_masked(col, bitmap) into a buffer, torch.sort, and one read per quantile
Arms ALTERNATE, each warmed up, device events around each arm: median ms with the arm's min-max spread.  For the median, decode_masked +
torch.kthvalue is timed beside them ONCE, unwarmed (torch.sort where kthvalue refuses the size): it takes seconds on columns of this size, so it does
not alternate.  The new calls' lower neighbours are compared with both of today's routes, bit for bit, unless the selection holds a NaN (torch sorts
NaNs last and counts them).  "pass" is the trace's compacting pass of the new arm (8 / 4: never).
  python3 tools/time_quantile.py [--vectors N] [--reps R] [--out FILE]"""
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

QS = ((0.5,), tuple(i / 15 for i in range(16)))
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
    scratch = [ctx.quantile_scratch(col) for _ in range(2)]
    zones = ctx.zone_map(col)
    emit(f"  {'density':>7s} {'q':>3s} {'new ms':>28s} {'zoned ms':>28s} {'today (sort) ms':>28s} {'today/new':>9s} {'today/zoned':>11s} {'pass':>4s} {'kthvalue ms':>11s}  new beats today by more than the spreads")
    for i, d in enumerate(DENSITIES):
        random_bitmap(mask, nv, d, False, 90 + i)
        for q in QS:
            vals = [torch.empty(2 * len(q), dtype=tdt, device=dev) for _ in range(2)]
            ranks = torch.empty(len(q), dtype=torch.int64, device=dev)
            count = torch.empty(1, dtype=torch.int64, device=dev)
            today_vals, has_nan = [None], [False]

            def new():
                ctx.quantile_into(col, mask, q, vals[0], count, ranks, scratch=scratch[0])

            def zoned():
                ctx.quantile_into(col, mask, q, vals[1], count, ranks, zones=zones, scratch=scratch[1])

            def selection():
                ctx.decode_masked_into(col, mask, buf, n_sel, scratch=sel_scratch)
                n = int(n_sel.item())  # (the read-back today's route cannot avoid: the rank needs the length)
                return n, [min(n - 1, int(x * (n - 1))) for x in q]

            def today():
                n, at = selection()
                today_vals[0] = torch.sort(buf[:n]).values[torch.tensor(at, device=dev)]

            kth = "-"
            if len(q) == 1:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                n, at = selection()
                try:
                    kth_val = torch.kthvalue(buf[:n], at[0] + 1).values.reshape(1)
                except RuntimeError:
                    kth_val = None  # (kthvalue refuses the size)
                b.record()
                b.synchronize()
                kth = f"{a.elapsed_time(b):.1f}" if kth_val is not None else "refused"
                has_nan[0] = bool(torch.isnan(buf[:n]).any())

            t = alternate([("new", new), ("zoned", zoned), ("today", today)], reps, warmup=1)
            trace = ctx.quantile_trace(scratch[0])
            lower = [v[0::2] for v in vals]
            note = ""
            n = int(n_sel.item())
            if has_nan[0] or bool(torch.isnan(buf[:n]).any()):
                note = "  (the selection holds a NaN: not compared)"
            else:
                theirs = [today_vals[0]] + ([kth_val] if len(q) == 1 and kth_val is not None else [])
                if not all(torch.equal(ibits(lo), ibits(t_)) for lo in lower for t_ in theirs):
                    # (torch does not order -0.0 and +0.0: a difference there alone is not an error of either route)
                    same = all(torch.equal(lo, t_) for lo in lower for t_ in theirs)
                    note = "  (differs from today's only in the signs of zeros)" if same else "  WRONG RESULT"
            tn, tz, tt = t["new"], t["zoned"], t["today"]
            spread = max(tn[2] - tn[1], tt[2] - tt[1])
            emit(f"  {d:7g} {len(q):3d} {fmt(tn)} {fmt(tz)} {fmt(tt)} {tt[0] / tn[0]:9.2f} {tt[0] / tz[0]:11.2f} {trace['compact_pass']:4d} {kth:>11s}  "
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

    emit(f"time_quantile.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after the warm-up, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_quantile.py {' '.join(sys.argv[1:])}".rstrip())
    nv = a.vectors
    kinds = (("mixed double (bench.py mixed)", lambda: bench.synthetic_input("mixed", nv, dev, seed=1)),
             ("ALP_RD double (bench.py rd)", lambda: bench.synthetic_input("rd", nv, dev, seed=1)),
             ("float, two decimals + 1 % exceptions", lambda: float_column(nv, dev, seed=1)),
             ("sorted double, two decimals", lambda: sorted_column(nv, dev)),
             ("constant double (the declared worst case: every pass decodes)", lambda: torch.full((nv * 1024,), 3.5, dtype=torch.float64, device=dev)))
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
