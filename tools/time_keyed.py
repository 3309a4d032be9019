#!/usr/bin/env python3
"""time_keyed.py: keyed aggregation (alpgpu_decode_keyed_sum_*: SUM and COUNT of a value column per key of a sorted key list, under a bitmap) against
the routes a caller had without it, in one process.

Value columns: bench.py's mixed ALP column and the all-ALP_RD double column (bench.py "rd"); the call is built for double columns only.  Beside each a key
column of the same type with K distinct values (multiples of 0.25: ALP vectors without exceptions), K in {16, 64, 256, 1024}, once in random order
and once sorted, the sorted one with its zone map (prepared ahead, outside the timed region).  Bitmap in {NULL, uniformly random of density 1, 0.1, 1e-2}.
  new       keyed_sum_into(val, key, keys, bitmap) into given tensors with a given scratch (the sorted key column: with zones=zone_map(key))
  group     today's compressed route: ceil(K / 16) rounds of decode_group_sum(val, key, bitmap, [k, k], counts=...) + group_totals; under the NULL
            bitmap it takes a bitmap of all ones
  decode    decode_masked of both columns (NULL bitmap: decode) + torch.searchsorted + index_add_: both columns materialised
  floor     histogram of the key column with the keys as point buckets plus decode_sum_masked of the value column: each column decoded once, no keyed
            sum: what the call cannot beat by much
Arms ALTERNATE, each warmed up, device events around each arm: median ms with the arm's min-max spread.  The new call's counts are compared with the
group route's exact counts.  No arm but `new` uses the new call.

--ab LIB[,LIB...]: variant builds of the library (the same ABI) instead of the other routes: the same keyed_sum_into call from this library and
from each variant, arms alternating; sums and counts are compared with this library's.  A build of keyed_kernels.hip with
-DALPGPU_KEYED_BASELINE_STEP is the step without the lone-lane shortcut.

Time limits are the caller's; run one column per command.  THE DECODE ARM IS SLOW on a column without NaNs: torch's index_add_ of doubles onto K
addresses retries under contention, 2.1-2.2 s for 8 Mi rows at K = 16 under a dense bitmap, which is minutes per repetition at 1 Mi vectors (the
mixed column hides it: every sum there is a NaN, whose bits an add does not change).  --no-decode leaves that arm out; take its figures from a
run with fewer --vectors.
  python3 tools/time_keyed.py [--vectors N] [--reps R] [--columns mixed,rd] [--keys 16,64,...] [--ab LIB,...] [--no-decode] [--out FILE]"""
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
from time_histogram import load_variant  # noqa: E402
from time_mask import fmt  # noqa: E402
from time_select import alternate  # noqa: E402
from time_take_masked import random_bitmap  # noqa: E402

KEYS = (16, 64, 256, 1024)
BITMAPS = (None, 1.0, 0.1, 1e-2)


def key_values(nv, K, tdt, dev, in_order):
    g = torch.Generator(device=dev)
    g.manual_seed(40 + K)
    k = torch.randint(0, K, (nv * 1024,), device=dev, generator=g)
    if in_order:
        k = torch.sort(k).values
    return (k.to(torch.float64) * 0.25).to(tdt)


def run_column(ctxs, names, name, x, reps, key_counts, emit, with_decode=True):
    """ctxs[0]: this library; ctxs[1:]: variants (--ab), which replace the other routes"""
    ctx, ab = ctxs[0], len(ctxs) > 1
    dev = x.device
    vals = [c.encode(x) for c in ctxs]
    val = vals[0]
    tdt = x.dtype
    del x
    nv = val.n_vectors
    emit(f"== {name}: {nv} vectors" + (f"; arms: {', '.join(names)}" if ab else ""))
    mask = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    ones = torch.full((16 * nv,), -1, dtype=torch.int64, device=dev)
    if not ab:
        bufv = torch.empty(nv * 1024, dtype=tdt, device=dev)
        bufk = torch.empty(nv * 1024, dtype=tdt, device=dev)
        n_sel = torch.empty(1, dtype=torch.int64, device=dev)
        sel_scratch = ctx.select_scratch(val)
        gsums = torch.empty((16, nv), dtype=torch.float64, device=dev)
        gcnts = torch.empty((16, nv), dtype=torch.int32, device=dev)
        gt_scratch = ctx.group_totals_scratch(nv, 16)
        vsums = torch.empty(nv, dtype=torch.float64, device=dev)
    head = " ".join(f"{n + ' ms':>27s}" for n in (names if ab else ("new", "group", "decode", "floor")))
    emit(f"  {'K':>4s} {'key column':>12s} {'bitmap':>6s} {head}" + ("  variant / this library" if ab else f" {'group/new':>9s} {'decode/new':>10s} {'new/floor':>9s}  new beats group by more than the spreads"))
    for K in key_counts:
        keys = (torch.arange(K, dtype=torch.float64, device=dev) * 0.25).to(tdt)
        key_list = [float(v) for v in keys.tolist()]
        for kname, in_order in (("random", False), ("sorted+zones", True)):
            kx = key_values(nv, K, tdt, dev, in_order)
            kcols = [c.encode(kx) for c in ctxs]
            del kx
            key = kcols[0]
            zones = [c.zone_map(kc) if in_order else None for c, kc in zip(ctxs, kcols)]
            scratch = [c.keyed_sum_scratch(nv, K) for c in ctxs]
            sums = [torch.empty(K, dtype=torch.float64, device=dev) for _ in ctxs]
            cnts = [torch.empty(K + 1, dtype=torch.int64, device=dev) for _ in ctxs]
            hist = torch.empty(K + 2, dtype=torch.int64, device=dev)
            tot = torch.empty(((K + 15) // 16) * 16, dtype=torch.float64, device=dev)
            tcnt = torch.empty(((K + 15) // 16) * 16, dtype=torch.int64, device=dev)
            dsum = torch.empty(K, dtype=torch.float64, device=dev)
            if not ab:
                # the self-check of the SUMS: the key column summed by itself.  Multiples of 0.25 below 2^8, at most 2^30 of them: every partial sum
                # is exact whatever the order, so the new call's sums must equal the rounds' bit for bit (the value columns' sums have no such yardstick)
                ctx.keyed_sum_into(key, key, keys, sums[0], counts_out=cnts[0], zones=zones[0], scratch=scratch[0])
                for r in range(0, K, 16):
                    part = key_list[r:r + 16]
                    g = len(part)
                    ctx.decode_group_sum(key, key, ones, part, part, out=gsums[:g], counts=gcnts[:g])
                    ctx.group_totals(gsums[:g], gcnts[:g], scratch=gt_scratch, out=tot[r:r + g], counts_out=tcnt[r:r + g])
                ok = torch.equal(sums[0].view(torch.int64), tot[:K].view(torch.int64)) and torch.equal(cnts[0][:K], tcnt[:K]) and int(cnts[0][K]) == 0
                emit(f"  {K:4d} {kname:>12s} self-check, SUM(key), COUNT(*) GROUP BY key (exact in any order): sums equal the rounds' bit for bit, counts equal: {'yes' if ok else 'NO'}"
                     f" (total {float(sums[0].sum()):.2f})")
            for density in BITMAPS:
                if density is not None:
                    random_bitmap(mask, nv, density, False, 90)
                m = None if density is None else mask

                def new(i=0):
                    return lambda: ctxs[i].keyed_sum_into(vals[i], kcols[i], keys, sums[i], counts_out=cnts[i], mask=m, zones=zones[i], scratch=scratch[i])

                def group():
                    for r in range(0, K, 16):
                        part = key_list[r:r + 16]
                        g = len(part)
                        ctx.decode_group_sum(val, key, ones if m is None else m, part, part, out=gsums[:g], counts=gcnts[:g])
                        ctx.group_totals(gsums[:g], gcnts[:g], scratch=gt_scratch, out=tot[r:r + g], counts_out=tcnt[r:r + g])

                def decode():
                    if m is None:
                        ctx.decode(val, out=bufv)
                        ctx.decode(key, out=bufk)
                        xv, xk = bufv, bufk
                    else:
                        ctx.decode_masked_into(val, m, bufv, n_sel, scratch=sel_scratch)
                        ctx.decode_masked_into(key, m, bufk, n_sel, scratch=sel_scratch)
                        n = int(n_sel.item())  # (the read-back this route cannot avoid)
                        xv, xk = bufv[:n], bufk[:n]
                    at = torch.searchsorted(keys, xk).clamp_(max=K - 1)
                    hit = keys[at] == xk
                    dsum.zero_()
                    dsum.index_add_(0, at[hit], xv[hit].to(torch.float64))

                def floor():
                    ctx.histogram(key, keys, mask=m, out=hist, sorted=True)
                    ctx.decode_sum_masked(val, ones if m is None else m, out=vsums)

                bm = "NULL" if density is None else format(density, "g")
                if ab:
                    t = alternate([(names[i], new(i)) for i in range(len(ctxs))], reps, warmup=1)
                    t0 = t[names[0]]
                    notes = []
                    for i in range(1, len(ctxs)):
                        ti = t[names[i]]
                        spread = max(t0[2] - t0[1], ti[2] - ti[1])
                        verdict = "WINS" if t0[0] - ti[0] > spread else ("loses" if ti[0] - t0[0] > spread else "level")
                        nan = torch.isnan(sums[0])  # (a NaN sum has no specified payload: NaNs compare as NaNs, everything else bit for bit)
                        differ = int((torch.isnan(sums[i]) != nan).sum()) + int((sums[i].view(torch.int64)[~nan] != sums[0].view(torch.int64)[~nan]).sum())
                        same = differ == 0 and torch.equal(cnts[i], cnts[0])
                        notes.append(f"{ti[0] / t0[0]:.3f} {verdict} ({ti[0] - t0[0]:+.3f} ms, spread {spread:.3f}), {int(nan.sum())} NaN sums{'' if same else f'  DIFFERENT BITS in {differ} sums'}")
                    emit(f"  {K:4d} {kname:>12s} {bm:>6s} " + " ".join(fmt(t[n]) for n in names) + "  " + "; ".join(notes))
                    continue
                t = alternate([("new", new()), ("group", group), ("floor", floor)] + ([("decode", decode)] if with_decode else []), reps, warmup=1)
                tn, tg, tf = t["new"], t["group"], t["floor"]
                td = t.get("decode", (float("nan"),) * 3)
                note = "" if torch.equal(cnts[0][:K], tcnt[:K]) else "  WRONG RESULT (differs from the group route's counts)"
                spread = max(tn[2] - tn[1], tg[2] - tg[1])
                verdict = f"{'yes' if tg[0] - tn[0] > spread else 'NO'} ({tg[0] - tn[0]:+.3f} ms, spread {spread:.3f} ms)"
                emit(f"  {K:4d} {kname:>12s} {bm:>6s} {fmt(tn)} {fmt(tg)} {fmt(td)} {fmt(tf)} {tg[0] / tn[0]:9.2f} {td[0] / tn[0]:10.2f} {tn[0] / tf[0]:9.2f}  {verdict}{note}")
            del kcols, key, zones
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--columns", default="mixed,rd")
    ap.add_argument("--keys", default=",".join(str(k) for k in KEYS))
    ap.add_argument("--ab", default=None, help="variant builds of the library to time beside this one, comma-separated")
    ap.add_argument("--no-decode", action="store_true", help="leave the decode arm out (its columns print nan)")
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

    emit(f"time_keyed.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after the warm-up, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_keyed.py {' '.join(sys.argv[1:])}".rstrip())
    nv = a.vectors
    kinds = {"mixed": ("mixed double (bench.py mixed)", lambda: bench.synthetic_input("mixed", nv, dev, seed=1)),
             "rd": ("ALP_RD double (bench.py rd)", lambda: bench.synthetic_input("rd", nv, dev, seed=1))}
    ctxs, names = [ctx], ["this"]
    if a.ab:
        paths = a.ab.split(",")
        variants = [load_variant(p, i) for i, p in enumerate(paths)]
        ctxs += [v.Context(0) for v in variants]
        names += [os.path.splitext(os.path.basename(p))[0].replace("libalpgpu_", "") for p in paths]
        for p, v in zip(paths, variants):
            emit(f"variant {p}: library sha-256 {hashlib.sha256(open(v.lib._name, 'rb').read()).hexdigest()[:16]}")
    for key in a.columns.split(","):
        name, make = kinds[key]
        run_column(ctxs, names, name, make(), a.reps, [int(k) for k in a.keys.split(",")], emit, with_decode=not a.no_decode)
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
