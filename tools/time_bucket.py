#!/usr/bin/env python3
"""time_bucket.py: bucketed aggregation (alpgpu_decode_bucket_sum_* / alpgpu_decode_bucket_minmax_*: SUM, MIN / MAX and COUNT of a value column per bucket
of a key column by sorted edges, under a bitmap) against the route a caller had without it, in one process.

Value columns: bench.py's mixed ALP column, the all-ALP_RD double column (bench.py "rd") and a float column (two decimals, 1 % full precision).  Beside
each a key column of the same type whose values are multiples of 0.25 in [0, B) (ALP vectors without exceptions), once in random order and once
sorted, the sorted one with its zone map (prepared ahead, outside the timed region); the B - 1 edges are 1, 2, ..., B - 1, so bucket b is [b, b + 1);
B in {16, 64, 256, 1024}.  Bitmap in {NULL, uniformly random of density 0.1, 1e-2}.
  sum       bucket_sum_into(val, key, edges, bitmap) into given tensors with a given scratch (the sorted key column: with zones=zone_map(key))
  minmax    bucket_minmax_into, the same arguments
  g-sum     today's route: ceil(B / 16) rounds of decode_group_sum(val, key, bitmap, lo, hi, counts=...) + group_totals with lo = e[b-1] and
            hi = nextafter(e[b], -inf) (-inf and +inf at the ends); under the NULL bitmap it takes a bitmap of all ones
  g-minmax  the same rounds of decode_group_minmax + group_minmax_totals
  hist      histogram(key, edges, bitmap): the counts alone, the floor of both calls
Arms ALTERNATE, each warmed up, device events around each arm: median ms with the arm's min-max spread.  In every cell the new calls' counts are
compared with histogram's and with the rounds' exact counts; per key column SUM(key) by bucket(key), whose every partial sum is exact (multiples of
0.25), is compared with the rounds' bit for bit.  A ratio below 1 (the new call loses) is printed in **bold**.
  python3 tools/time_bucket.py [--vectors N] [--reps R] [--columns mixed,rd,float] [--buckets 16,64,...] [--out FILE]"""
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

BUCKETS = (16, 64, 256, 1024)
BITMAPS = (None, 0.1, 1e-2)


def key_values(nv, B, tdt, dev, in_order):
    g = torch.Generator(device=dev)
    g.manual_seed(40 + B)
    k = torch.randint(0, 4 * B, (nv * 1024,), device=dev, generator=g)
    if in_order:
        k = torch.sort(k).values
    return (k.to(torch.float64) * 0.25).to(tdt)


def ratio(r):
    return f"{r:9.2f}" if r >= 1 else f"{'**%.2f**' % r:>9s}"


def run_column(ctx, name, x, reps, bucket_counts, emit):
    dev = x.device
    val = ctx.encode(x)
    tdt = x.dtype
    ndt = np.float64 if tdt == torch.float64 else np.float32
    del x
    nv = val.n_vectors
    emit(f"== {name}: {nv} vectors")
    mask = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    ones = torch.full((16 * nv,), -1, dtype=torch.int64, device=dev)
    gsums = torch.empty((16, nv), dtype=torch.float64, device=dev)
    gcnts = torch.empty((16, nv), dtype=torch.int32, device=dev)
    grecs = torch.empty((16, nv, 2), dtype=tdt, device=dev)
    gt_scratch = ctx.group_totals_scratch(nv, 16)
    emit(f"  {'B':>4s} {'key column':>12s} {'bitmap':>6s} " + " ".join(f"{n + ' ms':>27s}" for n in ("sum", "minmax", "g-sum", "g-minmax", "hist")) +
         f" {'g-sum/sum':>9s} {'g-mm/mm':>9s} {'hist/sum':>9s} {'hist/mm':>9s}")
    for B in bucket_counts:
        E = B - 1
        edges_np = np.arange(1, B).astype(ndt)
        edges = torch.from_numpy(edges_np).to(dev)
        lo = [-np.inf] + [float(e) for e in edges_np]
        hi = [float(np.nextafter(e, ndt(-np.inf))) for e in edges_np] + [np.inf]
        pad = ((B + 15) // 16) * 16
        for kname, in_order in (("random", False), ("sorted+zones", True)):
            kx = key_values(nv, B, tdt, dev, in_order)
            key = ctx.encode(kx)
            del kx
            zones = ctx.zone_map(key) if in_order else None
            scratch = ctx.bucket_sum_scratch(nv, E)
            sums = torch.empty(B, dtype=torch.float64, device=dev)
            recs = torch.empty((B, 2), dtype=tdt, device=dev)
            cs = torch.empty(B + 1, dtype=torch.int64, device=dev)
            cm = torch.empty(B + 1, dtype=torch.int64, device=dev)
            hist = torch.empty(B + 1, dtype=torch.int64, device=dev)
            tot = torch.empty(pad, dtype=torch.float64, device=dev)
            tcnt = torch.empty(pad, dtype=torch.int64, device=dev)
            trec = torch.empty((pad, 2), dtype=tdt, device=dev)

            def rounds_sum(v, m):
                for r in range(0, B, 16):
                    g = min(16, B - r)
                    ctx.decode_group_sum(v, key, ones if m is None else m, lo[r:r + g], hi[r:r + g], out=gsums[:g], counts=gcnts[:g])
                    ctx.group_totals(gsums[:g], gcnts[:g], scratch=gt_scratch, out=tot[r:r + g], counts_out=tcnt[r:r + g])

            def rounds_minmax(v, m):
                for r in range(0, B, 16):
                    g = min(16, B - r)
                    ctx.decode_group_minmax(v, key, ones if m is None else m, lo[r:r + g], hi[r:r + g], out=grecs[:g])
                    ctx.group_minmax_totals(grecs[:g], out=trec[r:r + g])

            # the self-check of the SUMS: the key column summed by its own buckets; every partial sum is exact whatever the order
            ctx.bucket_sum_into(key, key, edges, sums, counts_out=cs, zones=zones, scratch=scratch)
            rounds_sum(key, None)
            ok = torch.equal(sums.view(torch.int64), tot[:B].view(torch.int64)) and torch.equal(cs[:B], tcnt[:B]) and int(cs[B]) == 0
            emit(f"  {B:4d} {kname:>12s} self-check, SUM(key), COUNT(*) GROUP BY bucket(key) (exact in any order): sums equal the rounds' bit for bit, counts equal: "
                 f"{'yes' if ok else 'NO'} (total {float(sums.sum()):.2f})")
            for density in BITMAPS:
                if density is not None:
                    random_bitmap(mask, nv, density, False, 90)
                m = None if density is None else mask
                arms = [("sum", lambda: ctx.bucket_sum_into(val, key, edges, sums, counts_out=cs, mask=m, zones=zones, scratch=scratch)),
                        ("minmax", lambda: ctx.bucket_minmax_into(val, key, edges, recs, counts_out=cm, mask=m, zones=zones)),
                        ("g-sum", lambda: rounds_sum(val, m)), ("g-minmax", lambda: rounds_minmax(val, m)),
                        ("hist", lambda: ctx.histogram(key, edges, mask=m, out=hist, zones=zones, sorted=True))]
                t = alternate(arms, reps, warmup=1)
                note = ""
                if not (torch.equal(cs, hist) and torch.equal(cm, hist)):
                    note += "  WRONG COUNTS (differ from histogram's)"
                if not torch.equal(cs[:B], tcnt[:B]):
                    note += "  WRONG COUNTS (differ from the rounds')"
                if not torch.equal(recs.view(torch.int64 if tdt == torch.float64 else torch.int32), trec[:B].view(torch.int64 if tdt == torch.float64 else torch.int32)):
                    note += "  RECORDS DIFFER from the rounds'"
                bm = "NULL" if density is None else format(density, "g")
                emit(f"  {B:4d} {kname:>12s} {bm:>6s} " + " ".join(fmt(t[n]) for n in ("sum", "minmax", "g-sum", "g-minmax", "hist")) +
                     f" {ratio(t['g-sum'][0] / t['sum'][0])} {ratio(t['g-minmax'][0] / t['minmax'][0])} {t['hist'][0] / t['sum'][0]:9.2f} {t['hist'][0] / t['minmax'][0]:9.2f}{note}")
            del key, zones
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--columns", default="mixed,rd,float")
    ap.add_argument("--buckets", default=",".join(str(k) for k in BUCKETS))
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

    emit(f"time_bucket.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after the warm-up, device events; median (min-max) in ms")
    args = [w for i, w in enumerate(sys.argv[1:], 1) if w != "--out" and sys.argv[i - 1] != "--out" and not w.startswith("--out=")]  # (where the lines go is no part of the measurement)
    emit(f"library sha-256 {sha}; command: python3 tools/time_bucket.py {' '.join(args)}".rstrip())
    nv = a.vectors
    kinds = {"mixed": ("mixed double (bench.py mixed)", lambda: bench.synthetic_input("mixed", nv, dev, seed=1)),
             "rd": ("ALP_RD double (bench.py rd)", lambda: bench.synthetic_input("rd", nv, dev, seed=1)),
             "float": ("float (two decimals, 1 % full precision)", lambda: float_column(nv, dev))}
    for key in a.columns.split(","):
        name, make = kinds[key]
        run_column(ctx, name, make(), a.reps, [int(k) for k in a.buckets.split(",")], emit)
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
