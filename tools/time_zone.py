#!/usr/bin/env python3
"""time_zone.py: zone maps (alpgpu_zone_map_*, alpgpu_zone_map_of_values_*, alpgpu_zones_minmax_*) and the selection that reads them
(alpgpu_select_range_zoned_*) against what the library had before them, in one process.

Build: alpgpu_zone_map_* beside alpgpu_decode_count_range_* of the same column — the consumer it is built like: the same reads, 16 (8) instead of 4
bytes written per vector — on time_select.py's three columns (bench.py's mixed ALP column, an all-ALP_RD double column, a float column);
alpgpu_zone_map_of_values_* of the raw column with its bytes over its time as a fraction of the 8 TB/s HBM peak (bench.py reports the read-only
stream bound of the device it runs on); alpgpu_zones_minmax_* of the records.
Select: the zoned call beside the plain one (alpgpu_select_range_*, same library: the unzoned kernels are instruction for instruction those of the
parent commit) at time_select.py's selectivities, indices only, the whole call and the count pass alone (capacity 0), on (a) a sorted double
column, (b) a clustered one (every rowgroup around a level of its own), (c) the random mixed column, where no zone excludes anything: (c) is the cost
side — 16 bytes more read per vector.  Next to each row: the fraction of vectors the zones exclude / count whole, and the count pass's algorithmic
bytes with and without zones (descriptors + packed words + exception records of the vectors that are decoded, 16 bytes of zone per vector).
The arms ALTERNATE, each warmed up, device events around each arm, REPS repetitions: median ms with the arm's min-max spread beside it.
  python3 tools/time_zone.py [--vectors N] [--reps R] [--out FILE]"""
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
from time_select import alternate, float_column  # noqa: E402

PEAK = 8.0e12
INF = float("inf")


def fmt(t):
    return f"{t[0]:9.3f} ({t[1]:6.3f}-{t[2]:6.3f})"


def decimals(nv, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.round((torch.rand(nv * 1024, dtype=torch.float64, device=dev, generator=g) * 2e5 - 1e5) * 100.0) / 100.0


def sorted_column(nv, dev):
    return torch.sort(decimals(nv, dev, 5)).values


def clustered_column(nv, dev):
    """every rowgroup of 100 vectors around a level of its own, levels in random order"""
    g = torch.Generator(device=dev)
    g.manual_seed(6)
    n_rg = (nv + 99) // 100
    levels = torch.randperm(n_rg, device=dev, generator=g).to(torch.float64) * 50.0
    x = torch.round(torch.rand(nv * 1024, dtype=torch.float64, device=dev, generator=g) * 4000.0) / 100.0
    return torch.round((x + levels.repeat_interleave(100 * 1024)[:nv * 1024]) * 100.0) / 100.0


def build_rows(ctx, name, x, reps, lines):
    dev = x.device
    col = ctx.encode(x)
    pb, eb, _ = ctx.column_totals(col)
    nv = col.n_vectors
    vb = 8 if col.dtype == "f64" else 4
    compressed = 32 * nv + pb + eb
    zones = torch.empty((nv, 2), dtype=x.dtype, device=dev)
    zv = torch.empty((nv, 2), dtype=x.dtype, device=dev)
    counts = torch.empty(nv, dtype=torch.int32, device=dev)
    mm = torch.empty(2, dtype=x.dtype, device=dev)
    t = alternate([("zone_map", lambda: ctx.zone_map(col, zones)), ("count_range", lambda: ctx.decode_count_range(col, -1.0, 1.0, counts)),
                   ("of_values", lambda: ctx.zone_map_of_values(x, zv)), ("minmax", lambda: ctx.column_minmax(zones, mm))], reps)
    ok = torch.equal(zones.view(torch.uint8), zv.view(torch.uint8))
    lines.append(f"== {name}: {nv} vectors, compressed {compressed / 1e9:.3f} GB, raw {nv * 1024 * vb / 1e9:.3f} GB{'' if ok else '  ZONE MAPS DIFFER'}")
    lines.append(f"  zone_map            {fmt(t['zone_map'])} ms   decode_count_range {fmt(t['count_range'])} ms   ratio {t['zone_map'][0] / t['count_range'][0]:.3f}   "
                 f"{compressed / (t['zone_map'][0] * 1e-3) / PEAK:.3f} of peak")
    lines.append(f"  zone_map_of_values  {fmt(t['of_values'])} ms   {nv * 1024 * vb / (t['of_values'][0] * 1e-3) / 1e12:.2f} TB/s read, {nv * 1024 * vb / (t['of_values'][0] * 1e-3) / PEAK:.3f} of peak")
    lines.append(f"  zones_minmax        {fmt(t['minmax'])} ms   ({nv * 2 * vb / 1e6:.1f} MB of records) -> {mm.tolist()}")
    return col, zones, compressed


def select_rows(ctx, name, col, zones, compressed, sample, reps, lines):
    dev = zones.device
    nv = col.n_vectors
    s = np.sort(sample[np.isfinite(sample)])
    count, pcount = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = ctx.select_scratch(col)
    vec = col.to_host()[1]
    plain_alp = torch.from_numpy((vec["scheme"] == capi.SCHEME_ALP) & (vec["exc_cnt"] == 0)).to(dev)
    vbytes = torch.from_numpy(32.0 + 128.0 * vec["bw"] + np.where(vec["scheme"] == capi.SCHEME_ALP_RD, 128.0 * vec["lbw"], 0.0) +
                              vec["exc_cnt"] * np.where(vec["scheme"] == capi.SCHEME_ALP, zones.element_size() + 2.0, 4.0)).to(dev)
    lines.append(f"-- select on {name}: zoned against plain, indices only; count = capacity 0")
    lines.append(f"  {'selectivity':>11s} {'selected':>11s} {'pass':>6s} {'zoned ms':>24s} {'plain ms':>24s} {'plain/zoned':>11s} {'excluded':>9s} {'whole':>7s} {'zoned GB':>9s} {'plain GB':>9s}")
    bounds = [("~0", float(s[-1]) + 1e6, float(s[-1]) + 2e6)]
    for f in (1e-4, 1e-2, 0.1, 0.5):
        bounds.append((f"{f:g}", float(s[int((0.5 - f / 2) * s.size)]), float(s[min(s.size - 1, int((0.5 + f / 2) * s.size))])))
    bounds.append(("1", -INF, INF))
    for label, lo, hi in bounds:
        ctx.select_range_into(col, lo, hi, None, count, scratch=scratch)
        k = int(count)
        out = ~((zones[:, 1] >= lo) & (zones[:, 0] <= hi))
        whole = (zones[:, 0] >= lo) & (zones[:, 1] <= hi) & plain_alp & ~out
        read = float(vbytes[~out & ~whole].sum()) + 32.0 * float(whole.sum())
        idx = torch.empty(max(k, 1), dtype=torch.int64, device=dev)
        pidx = torch.empty(max(k, 1), dtype=torch.int64, device=dev)
        for what in ("count", "all"):
            cap = None if what == "count" else k
            t = alternate([("zoned", lambda: ctx.select_range_into(col, lo, hi, idx[:k] if cap else None, count, scratch=scratch, zones=zones)),
                           ("plain", lambda: ctx.select_range_into(col, lo, hi, pidx[:k] if cap else None, pcount, scratch=scratch))], reps)
            ok = int(count) == int(pcount) == k and (not cap or torch.equal(idx[:k], pidx[:k]))
            lines.append(f"  {label:>11s} {k:11d} {what:>6s} {fmt(t['zoned'])} {fmt(t['plain'])} {t['plain'][0] / t['zoned'][0]:11.2f} {float(out.sum()) / nv:9.4f} {float(whole.sum()) / nv:7.4f} "
                         f"{(read + 2 * zones.element_size() * nv) / 1e9:9.3f} {compressed / 1e9:9.3f}{'' if ok else '  WRONG RESULT'}")
        del idx, pidx
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = capi.Context(0)
    sha = hashlib.sha256(open(os.path.join(ROOT, "alp_amd", "libalpgpu.so"), "rb").read()).hexdigest()[:16]
    lines = [f"time_zone.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after 2 warm-ups, device events; "
             f"median (min-max) in ms", f"library sha-256 {sha}; command: python3 tools/time_zone.py {' '.join(sys.argv[1:])}".rstrip()]
    columns = (("mixed double (bench.py mixed)", lambda: bench.synthetic_input("mixed", a.vectors, dev, seed=1), True),
               ("ALP_RD double (bench.py rd)", lambda: bench.synthetic_input("rd", a.vectors, dev, seed=2), False),
               ("float, two decimals + 1 % exceptions", lambda: float_column(a.vectors, dev), False),
               ("sorted double, two decimals", lambda: sorted_column(a.vectors, dev), True),
               ("clustered double, two decimals", lambda: clustered_column(a.vectors, dev), True))
    for name, make, with_select in columns:
        mark = len(lines)
        x = make()
        sample = x[::251].cpu().numpy()
        col, zones, compressed = build_rows(ctx, name, x, a.reps, lines)
        del x
        torch.cuda.empty_cache()
        if with_select:
            select_rows(ctx, name, col, zones, compressed, sample, a.reps, lines)
        print("\n".join(lines[mark:]), flush=True)
        del col, zones
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
