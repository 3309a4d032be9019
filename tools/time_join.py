#!/usr/bin/env python3
"""time_join.py: the join probe (alpgpu_join_probe_*) against the route a caller had without it, in one process.

Columns: bench.py's mixed ALP column, the all-ALP_RD double column (bench.py "rd"), the float column of time_select.py and the sorted decimals of
time_zone.py (probed with its zone map).  A key list of R distinct elements is half values of the column (drawn from a sample of it) and half absent
ones, sorted on the device beforehand (time_in_list.py: make_list).  Per R in {16, 4096, 64 Ki, 1 Mi} and per bitmap (none; uniformly random bits of
density 1, 0.1 and 1e-2; whole vectors of density 1e-2):
  join      join_probe_into(col, keys) -> pos (no span, no idx, no rows)
  today     decode_masked (no bitmap: decode) of the column into HBM + torch.searchsorted + == + where, over the rows the bitmap selects (their number
            read once beforehand, outside the timing)
  floor     select_in_mask(col, keys) SET (with a bitmap: AND into a copy of it, the copy inside the arm): the same decode and search, 128 bytes per
            vector written instead of 8 per row
Arms ALTERNATE, each warmed up, device events around each arm: median ms with the arm's min-max spread.  join's positions are compared with today's.
Cells where join is slower than today are marked LOSES.
  python3 tools/time_join.py [--vectors N] [--reps R] [--out FILE]"""
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
from time_in_list import make_list, pool_of  # noqa: E402
from time_mask import fmt  # noqa: E402
from time_select import alternate, float_column  # noqa: E402
from time_take_masked import random_bitmap  # noqa: E402
from time_zone import sorted_column  # noqa: E402

BITMAPS = (("none", None, False), ("random 1", 1.0, False), ("random 0.1", 0.1, False), ("random 1e-2", 1e-2, False), ("vectors 1e-2", 1e-2, True))
SIZES = (16, 4096, 1 << 16, 1 << 20)


def distinct_keys(pool, size, seed):
    keys = torch.unique(make_list(pool, size, seed))
    return keys[~torch.isnan(keys)]


def run_column(ctx, name, x, reps, emit, zoned=False):
    dev = x.device
    pool = pool_of(x)
    col = ctx.encode(x)
    del x
    nv = col.n_vectors
    total = nv * 1024
    tdt = torch.float64 if col.dtype == "f64" else torch.float32
    pb, eb, _ = ctx.column_totals(col)
    zones = ctx.zone_map(col) if zoned else None
    emit(f"== {name}: {nv} vectors, {pb / (128.0 * nv):.2f} packed bits per value, compressed {(32 * nv + pb + eb) / 1e9:.3f} GB, lds_max {ctx.in_list_lds_max(col.dtype)}"
         + (", every arm that takes one with the column's zone map" if zoned else ""))
    mask, work = torch.empty(16 * nv, dtype=torch.int64, device=dev), torch.empty(16 * nv, dtype=torch.int64, device=dev)
    pos = torch.empty(total, dtype=torch.int64, device=dev)
    vals = torch.empty(total, dtype=tdt, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = ctx.select_scratch(col)
    emit(f"  {'bitmap':>12s} {'R':>8s} {'rows':>11s} {'join ms':>28s} {'today ms':>28s} {'floor ms':>28s} {'today/join':>10s} {'join/floor':>10s}")
    losses = []
    for bname, density, clustered in BITMAPS:
        m = None
        k = total
        if density is not None:
            random_bitmap(mask, nv, density, clustered, 7)
            m = mask
            ctx.mask_to_indices_into(mask, None, count)
            k = int(count.item())
        for size in SIZES:
            keys = distinct_keys(pool, size, size)
            n_keys = keys.numel()
            res = [None]

            def join():
                ctx.join_probe_into(col, keys, pos, count, mask=m, zones=zones, scratch=scratch)

            def today():
                if m is None:
                    ctx.decode(col, vals)
                else:
                    ctx.decode_masked_into(col, m, vals, count, scratch=scratch)
                v = vals[:k]
                at = torch.searchsorted(keys, v).clamp_(max=n_keys - 1)
                res[0] = torch.where(keys[at] == v, at, -1)

            def floor():
                if m is None:
                    ctx.select_in_mask(col, keys, zones=zones, mask=work, sorted=True)
                else:
                    work.copy_(m)
                    ctx.select_in_mask(col, keys, zones=zones, op="and", mask=work, sorted=True)

            t = alternate([("join", join), ("today", today), ("floor", floor)], reps, warmup=1)
            note = "" if torch.equal(pos[:k], res[0]) else "  WRONG RESULT"
            res[0] = None
            if t["join"][0] > t["today"][0]:
                note += "  LOSES"
                losses.append(f"{bname} / {size}")
            emit(f"  {bname:>12s} {n_keys:8d} {k:11d} {fmt(t['join'])} {fmt(t['today'])} {fmt(t['floor'])} {t['today'][0] / t['join'][0]:10.2f} {t['join'][0] / t['floor'][0]:10.2f}{note}")
    emit("  join LOSES to today's route in: " + (", ".join(losses) if losses else "no cell"))


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

    emit(f"time_join.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after the warm-up, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_join.py {' '.join(sys.argv[1:])}".rstrip())
    nv = a.vectors
    kinds = (("mixed double (bench.py mixed)", lambda: bench.synthetic_input("mixed", nv, dev, seed=1), False),
             ("ALP_RD double (bench.py rd)", lambda: bench.synthetic_input("rd", nv, dev, seed=1), False),
             ("float, two decimals + 1 % exceptions", lambda: float_column(nv, dev, seed=1), False),
             ("sorted decimals (time_zone.py)", lambda: sorted_column(nv, dev), True))
    for name, make, zoned in kinds:
        run_column(ctx, name, make(), a.reps, emit, zoned)
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
