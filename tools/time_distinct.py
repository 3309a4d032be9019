#!/usr/bin/env python3
"""time_distinct.py: the distinct values (alpgpu_distinct_*: the sorted distinct values of a compressed column and their counts, under a bitmap)
against the route a caller had without them, in one process.

Columns: bench.py's mixed ALP column, the all-ALP_RD double column (bench.py "rd"), the float column of time_select.py and the sorted two-decimal
column of time_zone.py, the last one also with its zone map (prepared ahead, outside the timed region).  Each is REWRITTEN to K distinct values, K in
{16, 4096, 64 Ki, 1 Mi}: K of its own finite values are drawn (evenly from a sorted sample, then made distinct) and every value is replaced by the
nearest drawn value at or below it, so the column keeps the look of its values (decimals stay decimals, a sorted column stays sorted) and NaNs stay.
Per K and bitmap in {NULL, uniformly random of density 1, 0.1, 1e-2}:
  new       distinct_into(col, ...) with capacity = the power of two at or above K, a given scratch, counts wanted
  zoned     (sorted column with its zone map) the same with zones=zone_map(col)
  decode    today's route: decode_masked (NULL bitmap: decode) + torch.unique(sorted=True, return_counts=True): the column materialised and sorted
Arms ALTERNATE, each warmed up, device events around each arm: median ms with the arm's min-max spread.  The new call's values and counts are compared
bit for bit with the decode route's (NaNs dropped, the zeros made +0.0 there), and the trace of one extra call is printed (vectors settled without
the column / from their record / decoded, steps settled by wave agreement, inserts offered to the LDS table, inserts made into the global table).

Time limits are the caller's: run one column per command, each under `timeout 330`.
  python3 tools/time_distinct.py [--vectors N] [--reps R] [--columns mixed,rd,float,sorted+zones] [--distinct 16,4096,...] [--out FILE]"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
from alp_amd import capi  # noqa: E402
from time_mask import fmt  # noqa: E402
from time_select import alternate, float_column  # noqa: E402
from time_take_masked import random_bitmap  # noqa: E402
from time_zone import sorted_column  # noqa: E402

DISTINCT = (16, 4096, 1 << 16, 1 << 20)
BITMAPS = (None, 1.0, 0.1, 1e-2)


def rewritten(x, k):
    """x with every finite value replaced by the nearest of k of the column's own values at or below it (values below the first: the first)"""
    finite = x[torch.isfinite(x)]
    stride = max(1, finite.numel() // (8 * k))
    pool = torch.unique(finite[::stride])
    if pool.numel() > k:
        pool = pool[(torch.arange(k, device=x.device) * pool.numel()) // k]
    idx = (torch.bucketize(x, pool, right=True) - 1).clamp_(min=0)
    return torch.where(torch.isfinite(x), pool[idx], x), pool.numel()


def run_column(ctx, name, make, reps, distinct, with_zones, emit):
    dev = torch.device("cuda:0")
    for k in distinct:
        x, drawn = rewritten(make(), min(k, capi.DISTINCT_MAX - 8))  # (room for the infinities and a zero the column may hold beside the drawn values)
        col = ctx.encode(x)
        del x
        nv = col.n_vectors
        tdt = torch.float64 if col.dtype == "f64" else torch.float32
        pa, ea, _ = ctx.column_totals(col)
        emit(f"== {name} rewritten to {drawn} distinct values: {nv} vectors, {pa / (128.0 * nv):.2f} packed bits per value, compressed {(32 * nv + pa + ea) / 1e9:.3f} GB")
        capacity = 1
        while capacity < drawn + 2:  # (a NaN-free column may still gain a zero or an infinity of its own)
            capacity *= 2
        capacity = min(capacity, capi.DISTINCT_MAX)
        mask = torch.empty(16 * nv, dtype=torch.int64, device=dev)
        buf = torch.empty(nv * 1024, dtype=tdt, device=dev)
        n_sel = torch.empty(1, dtype=torch.int64, device=dev)
        sel_scratch = ctx.select_scratch(col)
        scratch = ctx.distinct_scratch(capacity)
        vals, valsz = torch.empty(capacity, dtype=tdt, device=dev), torch.empty(capacity, dtype=tdt, device=dev)
        cnts, cntsz = torch.empty(capacity, dtype=torch.int64, device=dev), torch.empty(capacity, dtype=torch.int64, device=dev)
        state, statez = torch.empty(4, dtype=torch.int64, device=dev), torch.empty(4, dtype=torch.int64, device=dev)
        zones = ctx.zone_map(col) if with_zones else None
        emit(f"  {'bitmap':>6s} {'D':>8s} {'new ms':>27s} {'zoned ms':>27s} {'decode + unique ms':>27s} {'decode/new':>10s}  new beats decode by more than the spreads; trace")
        for density in BITMAPS:
            if density is not None:
                random_bitmap(mask, nv, density, False, 90)
            m = None if density is None else mask
            route = {}

            def new():
                ctx.distinct_into(col, vals, state, counts_out=cnts, mask=m, scratch=scratch)

            def zoned():
                ctx.distinct_into(col, valsz, statez, counts_out=cntsz, mask=m, zones=zones, scratch=scratch)

            def decode():
                if m is None:
                    ctx.decode(col, out=buf)
                    xs = buf
                else:
                    ctx.decode_masked_into(col, m, buf, n_sel, scratch=sel_scratch)
                    xs = buf[:int(n_sel.item())]  # (the read-back this route cannot avoid)
                xs = xs[~torch.isnan(xs)]
                route["values"], route["counts"] = torch.unique(xs + 0.0, sorted=True, return_counts=True)  # (x + 0.0: -0.0 becomes +0.0)

            arms = [("new", new), ("decode", decode)] + ([("zoned", zoned)] if with_zones else [])
            t = alternate(arms, reps, warmup=1)
            tn, td = t["new"], t["decode"]
            d, _, _, overflow = state.tolist()
            note = ""
            if overflow:
                note += "  OVERFLOW"
            elif d != route["values"].numel() or not torch.equal(vals[:d].view(torch.uint8), route["values"].view(torch.uint8)) or not torch.equal(cnts[:d], route["counts"]):
                note += "  WRONG RESULT (differs from decode + unique)"
            if with_zones and not (torch.equal(state, statez) and torch.equal(vals[:d].view(torch.uint8), valsz[:d].view(torch.uint8)) and torch.equal(cnts[:d], cntsz[:d])):
                note += "  ZONES CHANGED THE RESULT"
            trace = torch.zeros(6, dtype=torch.int64, device=dev)
            ctx.distinct_into(col, vals, state, counts_out=cnts, mask=m, zones=zones, scratch=scratch, trace=trace)
            spread = max(tn[2] - tn[1], td[2] - td[1])
            verdict = f"{'yes' if td[0] - tn[0] > spread else 'NO'} ({td[0] - tn[0]:+.3f} ms, spread {spread:.3f} ms)"
            emit(f"  {'NULL' if density is None else format(density, 'g'):>6s} {d:8d} {fmt(tn)} {fmt(t['zoned']) if with_zones else '-':>27s} {fmt(td)} {td[0] / tn[0]:10.2f}  {verdict}; {trace.tolist()}{note}")
        del col, buf, mask
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--columns", default="mixed,rd,float,sorted+zones")
    ap.add_argument("--distinct", default=",".join(str(k) for k in DISTINCT))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = capi.Context(0)
    sha = hashlib.sha256(open(capi.lib._name, "rb").read()).hexdigest()[:16]
    out = open(a.out, "a") if a.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    emit(f"time_distinct.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after the warm-up, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_distinct.py {' '.join(sys.argv[1:])}".rstrip())
    nv = a.vectors
    kinds = {"mixed": ("mixed double (bench.py mixed)", lambda: bench.synthetic_input("mixed", nv, dev, seed=1), False),
             "rd": ("ALP_RD double (bench.py rd)", lambda: bench.synthetic_input("rd", nv, dev, seed=1), False),
             "float": ("float, two decimals + 1 % exceptions", lambda: float_column(nv, dev, seed=1), False),
             "sorted": ("sorted double, two decimals", lambda: sorted_column(nv, dev), False),
             "sorted+zones": ("sorted double, two decimals, with its zone map", lambda: sorted_column(nv, dev), True)}
    distinct = [int(k) for k in a.distinct.split(",")]
    for key in a.columns.split(","):
        name, make, with_zones = kinds[key]
        run_column(ctx, name, make, a.reps, distinct, with_zones, emit)
    if out:
        out.close()


if __name__ == "__main__":
    main()
