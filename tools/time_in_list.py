#!/usr/bin/env python3
"""time_in_list.py: set membership (alpgpu_select_in_mask_*) against the routes a caller had without it, in one process.

Columns: bench.py's mixed ALP column, the all-ALP_RD double column (bench.py "rd") and the float column of time_select.py.  A list of R elements is
half values of the column (drawn from a sample of it) and half absent ones, sorted on the device beforehand.  Per R in {2, 16, 256, lds_max,
65536, 1 Mi}:
  in        select_in_mask(col, list) SET
  floor     select_mask(col, lo, hi) SET of the same column: the same decode with no search
  rounds    R rounds of select_mask(col, x, x) OR into a cleared bitmap (R <= 16 only)
  isin      decode(col) to HBM + torch.isin (the bits are not packed: in its favour)
Then, on a sorted column of decimals (time_zone.py), `in` without and with the column's zone map for a clustered list (neighbouring values) and a
spread one; and on the mixed column an AND after a first predicate that leaves 1e-2 of the values (the copy of the prior bitmap is timed alone).
Arms ALTERNATE, each warmed up, device events around each arm: median ms with the arm's min-max spread.  The number of bits `in` sets is compared
with torch.isin's count.
  python3 tools/time_in_list.py [--vectors N] [--reps R] [--out FILE]"""
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
from time_mask import band, fmt, sorted_sample  # noqa: E402
from time_select import alternate, float_column  # noqa: E402
from time_zone import sorted_column  # noqa: E402


def pool_of(x):
    """distinct finite values of a sample of the column, shuffled"""
    u = torch.unique(x[::61])
    u = u[torch.isfinite(u)]
    g = torch.Generator(device=x.device)
    g.manual_seed(9)
    return u[torch.randperm(u.numel(), device=x.device, generator=g)]


def make_list(pool, size, seed, clustered=False):
    """size elements, sorted: half from the pool (clustered: neighbours in value), half absent (full-precision noise)"""
    g = torch.Generator(device=pool.device)
    g.manual_seed(seed)
    n_hit = min(pool.numel(), (size + 1) // 2)
    hits = torch.sort(pool).values[pool.numel() // 3:][:n_hit] if clustered else pool[:n_hit]
    noise = (torch.randn(size - n_hit, dtype=torch.float64, device=pool.device, generator=g) * 777.123456789).to(pool.dtype)
    if clustered:
        noise = hits[0] + noise.abs() % (hits[-1] - hits[0] + 1)
    return torch.sort(torch.cat([hits, noise])).values


def bits_set(ctx, mask, count):
    ctx.mask_to_indices_into(mask, None, count)
    return int(count.item())


def run_column(ctx, name, x, reps, emit):
    dev = x.device
    pool, sample = pool_of(x), sorted_sample(x)
    col = ctx.encode(x)
    del x
    nv = col.n_vectors
    tdt = torch.float64 if col.dtype == "f64" else torch.float32
    pb, eb, _ = ctx.column_totals(col)
    L = ctx.in_list_lds_max(col.dtype)
    emit(f"== {name}: {nv} vectors, {pb / (128.0 * nv):.2f} packed bits per value, compressed {(32 * nv + pb + eb) / 1e9:.3f} GB, bitmap {128 * nv / 1e6:.1f} MB, lds_max {L}")
    mask, other = torch.empty(16 * nv, dtype=torch.int64, device=dev), torch.empty(16 * nv, dtype=torch.int64, device=dev)
    out = torch.empty(nv * 1024, dtype=tdt, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    lo, hi = band(sample, 0.1)
    hits = [0]
    emit(f"  {'R':>8s} {'in ms':>28s} {'floor ms':>28s} {'rounds ms':>28s} {'isin ms':>28s} {'in/floor':>8s} {'rounds/in':>9s} {'isin/in':>8s}")
    for size in (2, 16, 256, L, 65536, 1 << 20):
        lst = make_list(pool, size, size)
        points = [float(v) for v in lst.tolist()] if size <= 16 else []

        def rounds():
            other.zero_()
            for v in points:
                ctx.select_mask(col, v, v, op="or", mask=other)

        def isin():
            ctx.decode(col, out)
            hits[0] = torch.isin(out, lst).sum()

        arms = [("in", lambda: ctx.select_in_mask(col, lst, mask=mask, sorted=True)), ("floor", lambda: ctx.select_mask(col, lo, hi, mask=other))]
        if points:
            arms.append(("rounds", rounds))
        arms.append(("isin", isin))
        t = alternate(arms, reps, warmup=1)
        note = "" if bits_set(ctx, mask, count) == int(hits[0]) else "  WRONG RESULT"
        r = t.get("rounds")
        emit(f"  {size:8d} {fmt(t['in'])} {fmt(t['floor'])} {fmt(r) if r else ' ' * 28} {fmt(t['isin'])} {t['in'][0] / t['floor'][0]:8.2f} "
             f"{(r[0] / t['in'][0]) if r else float('nan'):9.2f} {t['isin'][0] / t['in'][0]:8.2f}{note}")
    return col, sample, L


def run_and(ctx, col, sample, L, pool, reps, emit):
    nv = col.n_vectors
    prior = ctx.select_mask(col, *band(sample, 0.01))
    work = torch.empty_like(prior)
    emit(f"  AND after a first predicate that leaves 1e-2 of the values ({int((prior.reshape(-1, 16) != 0).any(dim=1).sum())} of {nv} vectors open); the copy of the prior bitmap is in both arms")
    emit(f"  {'R':>8s} {'copy + in AND ms':>28s} {'copy + in SET ms':>28s} {'copy ms':>28s}")
    for size in (16, L, 65536):
        lst = make_list(pool, size, size)

        def arm(op):
            work.copy_(prior)
            ctx.select_in_mask(col, lst, op=op, mask=work, sorted=True)

        t = alternate([("and", lambda: arm("and")), ("set", lambda: arm("set")), ("copy", lambda: work.copy_(prior))], reps, warmup=1)
        emit(f"  {size:8d} {fmt(t['and'])} {fmt(t['set'])} {fmt(t['copy'])}")


def run_zones(ctx, nv, dev, reps, emit):
    x = sorted_column(nv, dev)
    pool = pool_of(x)
    col = ctx.encode(x)
    del x
    zones = ctx.zone_map(col)
    L = ctx.in_list_lds_max(col.dtype)
    mask, other = torch.empty(16 * nv, dtype=torch.int64, device=dev), torch.empty(16 * nv, dtype=torch.int64, device=dev)
    emit(f"== sorted decimals (time_zone.py), {nv} vectors: select_in_mask SET without and with the column's zone map")
    emit(f"  {'list':>10s} {'R':>8s} {'negate':>6s} {'plain ms':>28s} {'zoned ms':>28s} {'plain/zoned':>11s}")
    for clustered in (True, False):
        for size in (256, L, 65536):
            lst = make_list(pool, size, size, clustered)
            for negate in (False, True):
                t = alternate([("plain", lambda: ctx.select_in_mask(col, lst, negate=negate, mask=mask, sorted=True)),
                               ("zoned", lambda: ctx.select_in_mask(col, lst, negate=negate, zones=zones, mask=other, sorted=True))], reps, warmup=1)
                note = "" if torch.equal(mask, other) else "  WRONG RESULT"
                emit(f"  {'clustered' if clustered else 'spread':>10s} {size:8d} {str(negate):>6s} {fmt(t['plain'])} {fmt(t['zoned'])} {t['plain'][0] / t['zoned'][0]:11.2f}{note}")


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

    emit(f"time_in_list.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after the warm-up, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_in_list.py {' '.join(sys.argv[1:])}".rstrip())
    nv = a.vectors
    kinds = (("mixed double (bench.py mixed)", lambda: bench.synthetic_input("mixed", nv, dev, seed=1)),
             ("ALP_RD double (bench.py rd)", lambda: bench.synthetic_input("rd", nv, dev, seed=1)),
             ("float, two decimals + 1 % exceptions", lambda: float_column(nv, dev, seed=1)))
    for i, (name, make) in enumerate(kinds):
        x = make()
        pool = pool_of(x)
        col, sample, L = run_column(ctx, name, x, a.reps, emit)
        del x
        if i == 0:
            run_and(ctx, col, sample, L, pool, a.reps, emit)
        del col, pool
        torch.cuda.empty_cache()
    run_zones(ctx, nv, dev, a.reps, emit)
    if out:
        out.close()


if __name__ == "__main__":
    main()
