#!/usr/bin/env python3
"""time_minmax.py: masked and grouped MIN / MAX (alpgpu_decode_minmax_masked_*, alpgpu_decode_group_minmax_* + alpgpu_group_minmax_totals_*) against the
route a caller had without them, in one process.

Value columns (the columns of time_group.py): bench.py's mixed ALP column, the all-ALP_RD double column (bench.py "rd") and the float column of
time_select.py.  The key is a column of small integers 0 .. 15 of the value column's type, uniformly drawn; the groups are the points 0 .. G - 1.
Per bitmap density in {1e-2, 0.1, 1}, uniformly random bits and whole vectors:
  masked    decode_minmax_masked(val, bitmap) + column_minmax: no value reaches HBM
  today     decode_masked(val, bitmap) into a buffer, torch.amin and torch.amax over it (a NaN-free column is assumed in its favour)
and per G in {1, 4, 8, 16}:
  group     decode_group_minmax(val, key, bitmap, lo, hi) + group_minmax_totals: one pass over both columns
  today     per group: copy of the bitmap, select_mask(key, lo_g, hi_g, AND), decode_masked(val), amin, amax: 2 G decodes
Arms ALTERNATE, each warmed up, device events around each arm: median ms with the arm's min-max spread.  Where today's result holds no NaN the
new calls' results are compared with it, bit for bit.
  python3 tools/time_minmax.py [--vectors N] [--reps R] [--out FILE]"""
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

GROUPS = (1, 4, 8, 16)
DENSITIES = (1e-2, 0.1, 1.0)


def verdict(new, old):
    """compared where today's route has a number; torch.amin / amax propagate a NaN the records ignore"""
    if bool(torch.isnan(old).any()):
        return "  (today's result holds a NaN: not compared)"
    return "" if torch.equal(ibits(new.reshape(-1)), ibits(old.reshape(-1))) else "  WRONG RESULT"


def run_pair(ctx, name, cv, ck, reps, emit):
    dev = torch.device(f"cuda:{ctx.device}")
    nv = cv.n_vectors
    tdt = torch.float64 if cv.dtype == "f64" else torch.float32
    (pa, ea, _), (pb, eb, _) = ctx.column_totals(cv), ctx.column_totals(ck)
    emit(f"== {name}: 2 x {nv} vectors, {pa / (128.0 * nv):.2f} (value) and {pb / (128.0 * nv):.2f} (key) packed bits per value, compressed {(64 * nv + pa + ea + pb + eb) / 1e9:.3f} GB together, "
         f"bitmap {128 * nv / 1e6:.1f} MB")
    mask = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    work = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    zones = torch.empty((max(GROUPS), nv, 2), dtype=tdt, device=dev)
    vals = torch.empty(nv * 1024, dtype=tdt, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    scratch = ctx.select_scratch(cv)
    mm, today_mm = torch.empty(2, dtype=tdt, device=dev), torch.empty(2, dtype=tdt, device=dev)

    def today_minmax(bitmap, out):
        ctx.decode_masked_into(cv, bitmap, vals, count, scratch=scratch)
        k = int(count.item())  # (the read-back today's route cannot avoid: the reduction needs the length)
        if k:
            out[0], out[1] = torch.amin(vals[:k]), torch.amax(vals[:k])
        else:
            out[0], out[1] = float("inf"), -float("inf")

    emit(f"  {'bits':>9s} {'density':>7s} {'G':>3s} {'new ms':>28s} {'today ms':>28s} {'today/new':>9s}  beats today by more than the spreads")
    for clustered in (False, True):
        for i, d in enumerate(DENSITIES):
            random_bitmap(mask, nv, d, clustered, 60 + i)

            def masked():
                ctx.decode_minmax_masked(cv, mask, out=zones[0])
                ctx.column_minmax(zones[0], out=mm)

            rows = [("-", alternate([("new", masked), ("today", lambda: today_minmax(mask, today_mm))], reps, warmup=1), verdict(mm, today_mm))]
            for G in GROUPS:
                lo = hi = [float(j) for j in range(G)]
                totals, today_totals = torch.empty((G, 2), dtype=tdt, device=dev), torch.empty((G, 2), dtype=tdt, device=dev)

                def group():
                    ctx.decode_group_minmax(cv, ck, mask, lo, hi, out=zones[:G])
                    ctx.group_minmax_totals(zones[:G], out=totals)

                def today():
                    for g in range(G):
                        work.copy_(mask)
                        ctx.select_mask(ck, lo[g], hi[g], op="and", mask=work)
                        today_minmax(work, today_totals[g])

                rows.append((str(G), alternate([("new", group), ("today", today)], reps, warmup=1), verdict(totals, today_totals)))
            for G, t, note in rows:
                tn, tt = t["new"], t["today"]
                spread = max(tn[2] - tn[1], tt[2] - tt[1])
                emit(f"  {'vectors' if clustered else 'uniform':>9s} {d:7g} {G:>3s} {fmt(tn)} {fmt(tt)} {tt[0] / tn[0]:9.2f}  "
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

    emit(f"time_minmax.py: {ctx.device_info()['name']}, 2 x {a.vectors} vectors per pair, arms alternating, {a.reps} repetitions after the warm-up, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_minmax.py {' '.join(sys.argv[1:])}".rstrip())
    nv = a.vectors
    kinds = (("mixed double (bench.py mixed)", lambda s: bench.synthetic_input("mixed", nv, dev, seed=s)),
             ("ALP_RD double (bench.py rd)", lambda s: bench.synthetic_input("rd", nv, dev, seed=s)),
             ("float, two decimals + 1 % exceptions", lambda s: float_column(nv, dev, seed=s)))
    for name, make in kinds:
        x = make(1)
        tdt = x.dtype
        cv = ctx.encode(x)
        del x
        g = torch.Generator(device=dev)
        g.manual_seed(3)
        flag = torch.randint(0, 16, (nv * 1024,), device=dev, generator=g).to(tdt)
        cf = ctx.encode(flag)
        del flag
        run_pair(ctx, name + ", key: flags 0 .. 15, point groups", cv, cf, reps=a.reps, emit=emit)
        del cv, cf
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
