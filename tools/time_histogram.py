#!/usr/bin/env python3
"""time_histogram.py: the histograms (alpgpu_histogram_*: bucket counts of a compressed column by sorted edges, under a bitmap) against the routes a
caller had without them, in one process.

Columns: bench.py's mixed ALP column, the all-ALP_RD double column (bench.py "rd"), the float column of time_select.py and the sorted two-decimal
column of time_zone.py, the last one also with its zone map (prepared ahead, outside the timed region).
Per bucket count B in {8, 64, 256, 1024, 4096} (B - 1 edges), bitmap in {NULL, uniformly random of density 1, 0.1, 1e-2} and edge set in {balanced: the
column's own quantiles; one bucket: every edge above the column's largest finite value, the contention worst case}:
  new       histogram(col, edges, bitmap) into a given tensor
  zoned     (sorted column only) the same with zones=zone_map(col)
  group     today's compressed route: ceil(B / 16) rounds of decode_group_sum(col, col, bitmap, lo, hi, counts=...) + group_totals (balanced edges only:
            its work does not depend on the edges); under the NULL bitmap it takes a bitmap of all ones
  decode    decode_masked (NULL bitmap: decode) + torch.bucketize + torch.bincount: the column materialised (balanced edges only)
  floor     select_in_mask with the edges as its list on the same column: the same decode and search with no bins.  It writes a scratch bitmap (op "set",
            every vector decoded: a uniformly random bitmap of these densities leaves no vector without a set bit either)
Arms ALTERNATE, each warmed up, device events around each arm: median ms with the arm's min-max spread.  The new call's buckets are compared with the
group route's exact counts.  No arm but `new` and `zoned` uses the new call, so the others can be timed on a commit without it.

--ab LIB[,LIB...]: variant builds of the library (the same ABI) instead of the other routes: the same histogram call from this library and from each
variant, arms alternating, on the cells a few-bucket route would serve: B = 8 on every column (both edge sets), and every B on the sorted column
with its zone map, where a record admits a few buckets.  Each library encodes the column for itself; counts are compared with this library's; the
variants' trace is printed (vectors settled without the column / from the record / by a few-bucket route / decoded).

Time limits are the caller's: a --columns run of one 1 Mi-vector column takes 60 to 100 s, nearly all of it the group arm at B = 1024 and 4096 (2 to
3 s a repetition); run one column per command, each under `timeout 330`, as profiles/r21_histogram.txt was taken.  An --ab run takes under a minute.
  python3 tools/time_histogram.py [--vectors N] [--reps R] [--columns mixed,rd,float,sorted+zones] [--buckets 8,64,...] [--ab LIB,...] [--out FILE]"""
import argparse
import hashlib
import importlib.util
import math
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

BUCKETS = (8, 64, 256, 1024, 4096)
BITMAPS = (None, 1.0, 0.1, 1e-2)
INF = math.inf


def run_column(ctx, name, x, reps, buckets, with_zones, emit):
    dev = x.device
    sample = x[::251].cpu().numpy()
    s = np.sort(sample[np.isfinite(sample)])
    col = ctx.encode(x)
    del x
    nv = col.n_vectors
    tdt = torch.float64 if col.dtype == "f64" else torch.float32
    ndt = np.float64 if col.dtype == "f64" else np.float32
    pa, ea, _ = ctx.column_totals(col)
    emit(f"== {name}: {nv} vectors, {pa / (128.0 * nv):.2f} packed bits per value, compressed {(32 * nv + pa + ea) / 1e9:.3f} GB, bitmap {128 * nv / 1e6:.1f} MB")
    mask = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    ones = torch.full((16 * nv,), -1, dtype=torch.int64, device=dev)
    scratch_mask = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    buf = torch.empty(nv * 1024, dtype=tdt, device=dev)
    n_sel = torch.empty(1, dtype=torch.int64, device=dev)
    sel_scratch = ctx.select_scratch(col)
    sums = torch.empty((16, nv), dtype=torch.float64, device=dev)
    cnts = torch.empty((16, nv), dtype=torch.int32, device=dev)
    gt_scratch = ctx.group_totals_scratch(nv, 16)
    tot = torch.empty(16, dtype=torch.float64, device=dev)
    zones = ctx.zone_map(col) if with_zones else None
    emit(f"  {'B':>4s} {'bitmap':>6s} {'edges':>10s} {'new ms':>27s} {'zoned ms':>27s} {'group ms':>27s} {'decode ms':>27s} {'floor ms':>27s} {'group/new':>9s} {'decode/new':>10s} {'new/floor':>9s}"
         f"  new beats group by more than the spreads")
    for B in buckets:
        balanced = s[(np.arange(1, B) * s.size) // B].astype(ndt)
        above = (float(s[-1]) + 1.0 + np.arange(B - 1, dtype=np.float64)).astype(ndt)
        for density in BITMAPS:
            if density is not None:
                random_bitmap(mask, nv, density, False, 90)
            m = None if density is None else mask
            t_balanced = None
            for ename, e_np in (("balanced", balanced), ("one bucket", above)):
                edges = torch.from_numpy(np.ascontiguousarray(e_np)).to(dev)
                out = torch.empty(B + 1, dtype=torch.int64, device=dev)
                outz = torch.empty(B + 1, dtype=torch.int64, device=dev)
                group_counts = torch.empty(((B + 15) // 16) * 16, dtype=torch.int64, device=dev)
                lo = [-INF] + [float(v) for v in e_np]
                hi = [float(np.nextafter(v, ndt(-INF))) for v in e_np] + [INF]  # closed ranges made disjoint

                def new():
                    ctx.histogram(col, edges, mask=m, out=out, sorted=True)

                def zoned():
                    ctx.histogram(col, edges, mask=m, zones=zones, out=outz, sorted=True)

                def group():
                    for r in range(0, B, 16):
                        g = min(16, B - r)
                        ctx.decode_group_sum(col, col, ones if m is None else m, lo[r:r + g], hi[r:r + g], out=sums[:g], counts=cnts[:g])
                        ctx.group_totals(sums[:g], cnts[:g], scratch=gt_scratch, out=tot[:g], counts_out=group_counts[r:r + g])

                def decode():
                    if m is None:
                        ctx.decode(col, out=buf)
                        xs = buf
                    else:
                        ctx.decode_masked_into(col, m, buf, n_sel, scratch=sel_scratch)
                        xs = buf[:int(n_sel.item())]  # (the read-back this route cannot avoid)
                    torch.bincount(torch.bucketize(xs, edges, right=True), minlength=B)

                def floor():
                    ctx.select_in_mask(col, edges, mask=scratch_mask, sorted=True)

                arms = [("new", new), ("floor", floor)]
                if with_zones:
                    arms.append(("zoned", zoned))
                if ename == "balanced":
                    arms += [("group", group), ("decode", decode)]
                t = alternate(arms, reps, warmup=1)
                tn, tf = t["new"], t["floor"]
                note = ""
                if with_zones and not torch.equal(out, outz):
                    note += "  ZONES CHANGED THE COUNTS"
                if ename == "balanced":
                    t_balanced = tn
                    if not torch.equal(out[:B], group_counts[:B]):
                        note += "  WRONG RESULT (differs from the group route's counts)"
                    tg, td = t["group"], t["decode"]
                    spread = max(tn[2] - tn[1], tg[2] - tg[1])
                    verdict = f"{'yes' if tg[0] - tn[0] > spread else 'NO'} ({tg[0] - tn[0]:+.3f} ms, spread {spread:.3f} ms)"
                    emit(f"  {B:4d} {'NULL' if density is None else format(density, 'g'):>6s} {ename:>10s} {fmt(tn)} {fmt(t['zoned']) if with_zones else '-':>27s} {fmt(tg)} {fmt(td)} {fmt(tf)} "
                         f"{tg[0] / tn[0]:9.2f} {td[0] / tn[0]:10.2f} {tn[0] / tf[0]:9.2f}  {verdict}{note}")
                else:
                    emit(f"  {B:4d} {'NULL' if density is None else format(density, 'g'):>6s} {ename:>10s} {fmt(tn)} {fmt(t['zoned']) if with_zones else '-':>27s} {'-':>27s} {'-':>27s} {fmt(tf)} "
                         f"{'-':>9s} {'-':>10s} {tn[0] / tf[0]:9.2f}  one bucket / balanced: {tn[0] / t_balanced[0]:.2f}{note}")


def load_variant(path, index):
    """alp_amd/capi.py once more, bound to another build of the library (capi reads ALPGPU_LIB when it is imported)"""
    before = os.environ.get("ALPGPU_LIB")
    os.environ["ALPGPU_LIB"] = os.path.abspath(path)
    try:
        spec = importlib.util.spec_from_file_location(f"capi_variant{index}", os.path.join(ROOT, "alp_amd", "capi.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if before is None:
            del os.environ["ALPGPU_LIB"]
        else:
            os.environ["ALPGPU_LIB"] = before
    return mod


def run_ab(ctxs, names, name, x, reps, buckets, with_zones, emit):
    """ctxs[0]: this library; ctxs[1:]: the variants.  The same call from each, arms alternating."""
    dev = x.device
    sample = x[::251].cpu().numpy()
    s = np.sort(sample[np.isfinite(sample)])
    cols = [c.encode(x) for c in ctxs]
    del x
    nv = cols[0].n_vectors
    ndt = np.float64 if cols[0].dtype == "f64" else np.float32
    emit(f"== {name}: {nv} vectors; arms: {', '.join(names)}")
    mask = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    zones = ctxs[0].zone_map(cols[0]) if with_zones else None
    emit(f"  {'B':>4s} {'bitmap':>6s} {'edges':>10s} " + " ".join(f"{n + ' ms':>27s}" for n in names) + "  variant / this library, and whether the variant wins by more than the spreads; trace of the variant")
    for B in buckets:
        balanced = s[(np.arange(1, B) * s.size) // B].astype(ndt)
        above = (float(s[-1]) + 1.0 + np.arange(B - 1, dtype=np.float64)).astype(ndt)
        for density in BITMAPS:
            if density is not None:
                random_bitmap(mask, nv, density, False, 90)
            m = None if density is None else mask
            for ename, e_np in (("balanced", balanced), ("one bucket", above)):
                edges = torch.from_numpy(np.ascontiguousarray(e_np)).to(dev)
                outs = [torch.empty(B + 1, dtype=torch.int64, device=dev) for _ in ctxs]

                def arm(i):
                    return lambda: ctxs[i].histogram(cols[i], edges, mask=m, zones=zones, out=outs[i], sorted=True)

                t = alternate([(names[i], arm(i)) for i in range(len(ctxs))], reps, warmup=1)
                t0 = t[names[0]]
                notes = []
                for i in range(1, len(ctxs)):
                    ti = t[names[i]]
                    spread = max(t0[2] - t0[1], ti[2] - ti[1])
                    trace = torch.zeros(4, dtype=torch.int64, device=dev)
                    ctxs[i].histogram_into(cols[i], edges, outs[i], mask=m, zones=zones, trace=trace)
                    verdict = "WINS" if t0[0] - ti[0] > spread else ("loses" if ti[0] - t0[0] > spread else "level")
                    wrong = "" if torch.equal(outs[i], outs[0]) else "  WRONG RESULT"
                    notes.append(f"{ti[0] / t0[0]:.3f} {verdict} ({ti[0] - t0[0]:+.3f} ms, spread {spread:.3f}) {trace.tolist()}{wrong}")
                emit(f"  {B:4d} {'NULL' if density is None else format(density, 'g'):>6s} {ename:>10s} " + " ".join(fmt(t[n]) for n in names) + "  " + "; ".join(notes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--columns", default="mixed,rd,float,sorted+zones")  # (sorted+zones times the call without the records too)
    ap.add_argument("--buckets", default=",".join(str(b) for b in BUCKETS))
    ap.add_argument("--ab", default=None, help="variant builds of the library to time beside this one, comma-separated")
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

    emit(f"time_histogram.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after the warm-up, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_histogram.py {' '.join(sys.argv[1:])}".rstrip())
    nv = a.vectors
    kinds = {"mixed": ("mixed double (bench.py mixed)", lambda: bench.synthetic_input("mixed", nv, dev, seed=1), False),
             "rd": ("ALP_RD double (bench.py rd)", lambda: bench.synthetic_input("rd", nv, dev, seed=1), False),
             "float": ("float, two decimals + 1 % exceptions", lambda: float_column(nv, dev, seed=1), False),
             "sorted": ("sorted double, two decimals", lambda: sorted_column(nv, dev), False),
             "sorted+zones": ("sorted double, two decimals, with its zone map", lambda: sorted_column(nv, dev), True)}
    buckets = [int(b) for b in a.buckets.split(",")]
    if a.ab:
        paths = a.ab.split(",")
        variants = [load_variant(p, i) for i, p in enumerate(paths)]
        ctxs = [ctx] + [v.Context(0) for v in variants]
        names = ["this"] + [os.path.splitext(os.path.basename(p))[0].replace("libalpgpu_", "") for p in paths]
        for p, v in zip(paths, variants):
            emit(f"variant {p}: library sha-256 {hashlib.sha256(open(v.lib._name, 'rb').read()).hexdigest()[:16]}")
        for key in a.columns.split(","):
            name, make, with_zones = kinds[key]
            run_ab(ctxs, names, name, make(), a.reps, buckets if with_zones else [b for b in buckets if b <= 8], with_zones, emit)
            torch.cuda.empty_cache()
        if out:
            out.close()
        return
    for key in a.columns.split(","):
        name, make, with_zones = kinds[key]
        run_column(ctx, name, make(), a.reps, buckets, with_zones, emit)
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
