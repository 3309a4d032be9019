#!/usr/bin/env python3
"""time_group.py: grouped aggregation (alpgpu_decode_group_sum_* + alpgpu_group_totals) against the route a caller had without it and against its
floor, in one process.

Value columns (1 Mi vectors each, the columns of time_pair.py): bench.py's mixed ALP column, the all-ALP_RD double column (bench.py "rd") and the
float column of time_select.py.  Keys, each of the value column's type:
  twin      the differently seeded twin of the value column, the groups G touching quantile bands of it that together hold every value
  flag      small integers 0 .. 15, uniformly drawn, the groups the points 0 .. G - 1
Per G in {1, 4, 8, 16} and bitmap density in {1e-2, 0.1, 1}, uniformly random bits and whole vectors:
  group     decode_group_sum(val, key, bitmap, lo, hi) + group_totals: one pass over both columns
  today     per group: copy of the bitmap, select_mask(key, lo_g, hi_g, AND), decode_sum_masked(val), tree_sum: 2 G decodes, parent-commit entry points only
  floor     decode_dot_masked(val, key) + tree_sum under the same bitmap: the same two vectors decoded and the least possible done with them
Arms ALTERNATE, each warmed up, device events around each arm: median ms with the arm's min-max spread.  Every cell's group totals are compared,
bit for bit, with today's route.
  python3 tools/time_group.py [--vectors N] [--reps R] [--out FILE]"""
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
from time_mask import fmt, sorted_sample  # noqa: E402
from time_select import alternate, float_column  # noqa: E402
from time_take_masked import random_bitmap  # noqa: E402

GROUPS = (1, 4, 8, 16)
DENSITIES = (1e-2, 0.1, 1.0)


def run_pair(ctx, name, cv, ck, groups_of, reps, emit):
    dev = torch.device(f"cuda:{ctx.device}")
    nv = cv.n_vectors
    (pa, ea, _), (pb, eb, _) = ctx.column_totals(cv), ctx.column_totals(ck)
    compressed = 64 * nv + pa + ea + pb + eb
    emit(f"== {name}: 2 x {nv} vectors, {pa / (128.0 * nv):.2f} (value) and {pb / (128.0 * nv):.2f} (key) packed bits per value, compressed {compressed / 1e9:.3f} GB together, "
         f"bitmap {128 * nv / 1e6:.1f} MB")
    mask = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    work = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    sums = torch.empty((max(GROUPS), nv), dtype=torch.float64, device=dev)
    counts = torch.empty((max(GROUPS), nv), dtype=torch.int32, device=dev)
    one = torch.empty(nv, dtype=torch.float64, device=dev)
    total1 = torch.empty(1, dtype=torch.float64, device=dev)
    emit(f"  {'bits':>9s} {'density':>7s} {'G':>3s} {'group_sum + totals ms':>28s} {'today: G x (copy, AND, sum) ms':>31s} {'floor: dot_masked ms':>28s} {'today/group':>11s} {'group/floor':>11s}  beats today by more than the spreads")
    for clustered in (False, True):
        for i, d in enumerate(DENSITIES):
            random_bitmap(mask, nv, d, clustered, 60 + i)
            for G in GROUPS:
                lo, hi = groups_of(G)
                totals = torch.empty(G, dtype=torch.float64, device=dev)
                tcounts = torch.empty(G, dtype=torch.int64, device=dev)
                today_totals = torch.empty(G, dtype=torch.float64, device=dev)
                scratch = ctx.group_totals_scratch(nv, G)

                def group():
                    ctx.decode_group_sum(cv, ck, mask, lo, hi, out=sums[:G], counts=counts[:G])
                    ctx.group_totals(sums[:G], counts[:G], scratch=scratch, out=totals, counts_out=tcounts)

                def today():
                    for g in range(G):
                        work.copy_(mask)
                        ctx.select_mask(ck, lo[g], hi[g], op="and", mask=work)
                        ctx.decode_sum_masked(cv, work, out=one)
                        ctx.tree_sum(one, out=today_totals[g:g + 1])

                def floor():
                    ctx.decode_dot_masked(cv, ck, mask, out=one)
                    ctx.tree_sum(one, out=total1)

                t = alternate([("group", group), ("today", today), ("floor", floor)], reps, warmup=1)
                a, b = totals.view(torch.int64), today_totals.view(torch.int64)
                nan = torch.isnan(today_totals)
                ok = torch.equal(torch.isnan(totals), nan) and torch.equal(a[~nan], b[~nan])
                tg, tt, tf = t["group"], t["today"], t["floor"]
                spread = max(tg[2] - tg[1], tt[2] - tt[1])
                emit(f"  {'vectors' if clustered else 'uniform':>9s} {d:7g} {G:3d} {fmt(tg)} {fmt(tt)}    {fmt(tf)} {tt[0] / tg[0]:11.2f} {tg[0] / tf[0]:11.2f}  "
                     f"{'yes' if tt[0] - tg[0] > spread else 'NO'} ({tt[0] - tg[0]:+.3f} ms, spread {spread:.3f} ms){'' if ok else '  WRONG RESULT'}")


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

    emit(f"time_group.py: {ctx.device_info()['name']}, 2 x {a.vectors} vectors per pair, arms alternating, {a.reps} repetitions after the warm-up, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_group.py {' '.join(sys.argv[1:])}".rstrip())
    nv = a.vectors
    kinds = (("mixed double (bench.py mixed)", lambda s: bench.synthetic_input("mixed", nv, dev, seed=s)),
             ("ALP_RD double (bench.py rd)", lambda s: bench.synthetic_input("rd", nv, dev, seed=s)),
             ("float, two decimals + 1 % exceptions", lambda s: float_column(nv, dev, seed=s)))
    for name, make in kinds:
        x = make(1)
        tdt = x.dtype
        cv = ctx.encode(x)
        del x
        twin = make(2)
        sample = sorted_sample(twin)
        ck = ctx.encode(twin)
        del twin

        def bands(G, sample=sample):
            cuts = [float(sample[min(sample.size - 1, int(j * sample.size / G))]) for j in range(1, G)]
            return [-float("inf")] + cuts, cuts + [float("inf")]

        run_pair(ctx, name + ", key: its twin, quantile bands", cv, ck, bands, a.reps, emit)
        del ck
        g = torch.Generator(device=dev)
        g.manual_seed(3)
        flag = torch.randint(0, 16, (nv * 1024,), device=dev, generator=g).to(tdt)
        cf = ctx.encode(flag)
        del flag
        run_pair(ctx, name + ", key: flags 0 .. 15, point groups", cv, cf, lambda G: ([float(j) for j in range(G)],) * 2, a.reps, emit)
        del cv, cf
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
