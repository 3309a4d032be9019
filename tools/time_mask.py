#!/usr/bin/env python3
"""time_mask.py: selection bitmaps (alpgpu_select_mask_*, alpgpu_mask_to_indices, alpgpu_decode_sum_masked_*) against what a caller did without them,
in one process.

Columns (1 Mi vectors each, two of every kind, a and b): bench.py's mixed ALP column, the all-ALP_RD double column (bench.py "rd") and the float
column of time_select.py.  Bounds are quantiles of a strided sample of each column around its median; selectivity 1 is [-inf, +inf].
  conjunction  lo1 <= a <= hi1 AND lo2 <= b <= hi2 as ascending indices, first x second selectivity over {1e-4, 1e-2, 0.1, 0.5, 1}:
                 mask    select_mask(a), select_mask(b, AND), mask_to_indices
                 gather  select_range(a), gather(b, idx), compare and index in torch
                 isin    two select_range calls intersected with torch.isin
               with value-uniform predicates (a as generated) and with a clustered first column (a sorted: whole vectors drop out)
  SET pass     select_mask(SET) beside select_range with capacity 0: the same decode writing 128 bytes per vector instead of 4 (+ the scan)
  AND skip     the AND pass over priors that leave 0 %, 1 %, 10 % and 100 % of the vectors non-zero, beside the SET pass
  masked SUM   decode_sum_masked under a full, a 10 % and a 1e-4 mask (made by select_mask) beside decode_sum (default and, for doubles, the
               persistent kernel: every vector, no mask) and beside select_range(values) + torch.sum
Arms ALTERNATE, each warmed up, device events around each arm: median ms with the arm's min-max spread.  "of peak": the mask route's algorithmic
bytes (compressed vectors read where a vector is decoded, 128 bytes per bitmap read or write of a vector, 12 bytes of scan scratch written and
read, 8 bytes per index) over its time, as a fraction of the 8 TB/s HBM peak.
  python3 tools/time_mask.py [--vectors N] [--reps R] [--out FILE]"""
import argparse
import hashlib
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
from time_select import alternate, float_column  # noqa: E402

PEAK = 8.0e12
INF = float("inf")
GRID = (1e-4, 1e-2, 0.1, 0.5, 1.0)


def fmt(t):
    return f"{t[0]:9.3f} ({t[1]:7.3f}-{t[2]:8.3f})"


def band(sample, f):
    """[lo, hi] around the median of the sorted sample that holds about the fraction f of the values"""
    if f >= 1.0:
        return -INF, INF
    return float(sample[int((0.5 - f / 2) * sample.size)]), float(sample[min(sample.size - 1, int((0.5 + f / 2) * sample.size))])


def sorted_sample(x):
    s = x[::251].cpu().numpy()
    return np.sort(s[np.isfinite(s)])


def nonzero_vectors(mask):
    return int((mask.reshape(-1, 16) != 0).any(dim=1).sum())


class Column:
    def __init__(self, ctx, x):
        self.sample = sorted_sample(x)
        self.col = ctx.encode(x)
        pb, eb, _ = ctx.column_totals(self.col)
        self.compressed = 32 * self.col.n_vectors + pb + eb
        self.bits = pb / (128.0 * self.col.n_vectors)


def conjunction(ctx, a, b, reps, emit, buf):
    nv = a.col.n_vectors
    mask, idx1, idx2, idxn, vals, count, scratch = buf
    emit(f"  {'sel a':>7s} {'sel b':>7s} {'selected':>11s} {'a leaves':>9s} {'mask ms':>28s} {'gather ms':>28s} {'isin ms':>28s} {'gather/mask':>11s} {'isin/mask':>9s} {'of peak':>8s}")
    for f1 in GRID:
        lo1, hi1 = band(a.sample, f1)
        ctx.select_range_into(a.col, lo1, hi1, None, count, scratch=scratch)
        k1 = int(count)
        ctx.select_mask(a.col, lo1, hi1, mask=mask)
        open_a = nonzero_vectors(mask)
        for f2 in GRID:
            lo2, hi2 = band(b.sample, f2)
            ctx.select_range_into(b.col, lo2, hi2, None, count, scratch=scratch)
            k2 = int(count)
            ctx.select_mask(a.col, lo1, hi1, mask=mask)
            ctx.select_mask(b.col, lo2, hi2, op="and", mask=mask)
            open_ab = nonzero_vectors(mask)
            ctx.mask_to_indices_into(mask, None, count, scratch)
            k = int(count)
            res = {}

            def by_mask():
                ctx.select_mask(a.col, lo1, hi1, mask=mask)
                ctx.select_mask(b.col, lo2, hi2, op="and", mask=mask)
                ctx.mask_to_indices_into(mask, idxn[:k] if k else None, count, scratch)

            def by_gather():
                ctx.select_range_into(a.col, lo1, hi1, idx1[:k1] if k1 else None, count, scratch=scratch)
                g = ctx.gather(b.col, idx1[:k1], out=vals[:k1])
                res["gather"] = idx1[:k1][(g >= lo2) & (g <= hi2)]

            def by_isin():
                ctx.select_range_into(a.col, lo1, hi1, idx1[:k1] if k1 else None, count, scratch=scratch)
                ctx.select_range_into(b.col, lo2, hi2, idx2[:k2] if k2 else None, count, scratch=scratch)
                res["isin"] = idx1[:k1][torch.isin(idx1[:k1], idx2[:k2], assume_unique=True)]

            with_isin = k1 + k2 < 2**31  # (torch.isin sorts both lists together and refuses more than INT_MAX elements)
            t = alternate([("mask", by_mask), ("gather", by_gather)] + ([("isin", by_isin)] if with_isin else []), reps, warmup=1)
            ok = torch.equal(idxn[:k], res["gather"]) and (not with_isin or torch.equal(idxn[:k], res["isin"]))
            model = a.compressed + 128 * nv + 128 * nv + (b.compressed / nv + 128) * open_a + (128 + 2 * 12) * nv + 128 * open_ab + 8 * k
            tm = t["mask"]
            isin_ms, isin_ratio = (fmt(t["isin"]), f"{t['isin'][0] / tm[0]:9.2f}") if with_isin else (f"{'(over 2^31 - 1 elements)':>28s}", f"{'-':>9s}")
            emit(f"  {f1:7g} {f2:7g} {k:11d} {open_a / nv:9.4f} {fmt(tm)} {fmt(t['gather'])} {isin_ms} {t['gather'][0] / tm[0]:11.2f} {isin_ratio} "
                 f"{model / (tm[0] * 1e-3) / PEAK:8.3f}{'' if ok else '  WRONG RESULT'}")
            res.clear()


def passes(ctx, a, reps, emit, buf):
    nv = a.col.n_vectors
    mask, idx1, idx2, idxn, vals, count, scratch = buf
    lo, hi = band(a.sample, 0.1)
    t = alternate([("set", lambda: ctx.select_mask(a.col, lo, hi, mask=mask)), ("count", lambda: ctx.select_range_into(a.col, lo, hi, None, count, scratch=scratch))], reps)
    emit(f"  SET pass, selectivity 0.1: select_mask {fmt(t['set'])} ms, select_range with capacity 0 {fmt(t['count'])} ms, ratio {t['set'][0] / t['count'][0]:.3f}; "
         f"SET of peak {(a.compressed + 128 * nv) / (t['set'][0] * 1e-3) / PEAK:.3f}")
    t_set = t["set"][0]
    lo, hi = band(a.sample, 0.5)
    emit(f"  AND pass, selectivity 0.5, over a prior of whole vectors (the bitmap is the pass's fixed point from the second run on):")
    g = torch.Generator(device=mask.device)
    g.manual_seed(11)
    for frac in (0.0, 0.01, 0.1, 1.0):
        keep = torch.rand(nv, device=mask.device, generator=g) < frac if frac < 1.0 else torch.ones(nv, dtype=torch.bool, device=mask.device)
        mask.reshape(nv, 16).copy_(torch.where(keep, -1, 0).to(torch.int64).reshape(nv, 1).expand(nv, 16))
        t = alternate([("and", lambda: ctx.select_mask(a.col, lo, hi, op="and", mask=mask))], reps)
        left = nonzero_vectors(mask)
        model = 128 * nv + (a.compressed / nv + 128) * left
        emit(f"    {100 * frac:5.1f} % of the vectors non-zero ({left:8d}): {fmt(t['and'])} ms, {t['and'][0] / t_set:6.3f} of the SET pass, of peak {model / (t['and'][0] * 1e-3) / PEAK:.3f}")


def masked_sum(ctx, a, reps, emit, buf):
    nv = a.col.n_vectors
    mask, idx1, idx2, idxn, vals, count, scratch = buf
    sums = torch.empty(nv, dtype=torch.float64, device=mask.device)
    counts = torch.empty(nv, dtype=torch.int32, device=mask.device)
    plain = torch.empty(nv, dtype=torch.float64, device=mask.device)
    emit(f"  {'mask':>7s} {'selected':>11s} {'decode_sum_masked ms':>28s} {'decode_sum ms':>28s} {'persistent decode_sum ms':>28s} {'select_range(values)+sum ms':>28s} {'of peak':>8s}")
    for f in (1.0, 0.1, 1e-4):
        lo, hi = band(a.sample, f)
        ctx.select_mask(a.col, lo, hi, mask=mask)
        ctx.mask_to_indices_into(mask, None, count, scratch)
        k = int(count)
        left = nonzero_vectors(mask)
        res = {}

        def by_select():
            ctx.select_range_into(a.col, lo, hi, idx1[:k] if k else None, count, vals[:k] if k else None, scratch=scratch)
            res["sum"] = vals[:k].sum(dtype=torch.float64)

        def persistent():
            ctx.set_option(capi.OPT_CONSUMER_PIPELINED, 1)
            ctx.decode_sum(a.col, plain)
            ctx.set_option(capi.OPT_CONSUMER_PIPELINED, 0)

        arms = [("masked", lambda: ctx.decode_sum_masked(a.col, mask, out=sums, counts=counts)), ("sum", lambda: ctx.decode_sum(a.col, plain)), ("select", by_select)]
        if a.col.dtype == "f64":
            arms.append(("persistent", persistent))
        t = alternate(arms, reps)
        total, want = float(ctx.tree_sum(sums)), float(res["sum"])  # (+-inf among the selected values: both sums are that infinity, or both NaN)
        close = (math.isnan(total) and math.isnan(want)) or total == want or abs(total - want) <= 1e-9 * float(vals[:k].abs().sum(dtype=torch.float64))
        ok = int(counts.sum()) == k and close
        model = 128 * nv + a.compressed / nv * left + 12 * nv
        emit(f"  {f:7g} {k:11d} {fmt(t['masked'])} {fmt(t['sum'])} {fmt(t['persistent']) if 'persistent' in t else '-':>28s} {fmt(t['select'])} "
             f"{model / (t['masked'][0] * 1e-3) / PEAK:8.3f}{'' if ok else '  WRONG RESULT'}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    ctx = capi.Context(0)
    sha = hashlib.sha256(open(os.path.join(ROOT, "alp_amd", "libalpgpu.so"), "rb").read()).hexdigest()[:16]
    out = open(a.out, "w") if a.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    emit(f"time_mask.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after the warm-ups, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_mask.py {' '.join(sys.argv[1:])}".rstrip())
    nv, n = a.vectors, a.vectors * 1024
    kinds = (("mixed double (bench.py mixed)", lambda seed: bench.synthetic_input("mixed", nv, dev, seed=seed), torch.float64),
             ("ALP_RD double (bench.py rd)", lambda seed: bench.synthetic_input("rd", nv, dev, seed=seed), torch.float64),
             ("float, two decimals + 1 % exceptions", lambda seed: float_column(nv, dev, seed=seed), torch.float32))
    for name, make, tdt in kinds:
        buf = (torch.empty(16 * nv, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev),
               torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=tdt, device=dev), torch.zeros(1, dtype=torch.int64, device=dev),
               torch.empty(capi.lib.alpgpu_select_scratch_bytes(nv), dtype=torch.uint8, device=dev))
        xa = make(1)
        a_col = Column(ctx, xa)
        a_sorted = Column(ctx, torch.sort(xa).values)
        del xa
        b_col = Column(ctx, make(2))
        torch.cuda.empty_cache()
        emit(f"== {name}: {nv} vectors; a {a_col.bits:.2f} packed bits per value, compressed {a_col.compressed / 1e9:.3f} GB; a sorted {a_sorted.bits:.2f} bits, {a_sorted.compressed / 1e9:.3f} GB; "
             f"b {b_col.compressed / 1e9:.3f} GB; bitmap {128 * nv / 1e6:.1f} MB")
        emit(" conjunction, value-uniform predicates:")
        conjunction(ctx, a_col, b_col, a.reps, emit, buf)
        emit(" conjunction, clustered first column (a sorted):")
        conjunction(ctx, a_sorted, b_col, a.reps, emit, buf)
        emit(" single passes (column a):")
        passes(ctx, a_col, a.reps, emit, buf)
        emit(" masked SUM (column a):")
        masked_sum(ctx, a_col, a.reps, emit, buf)
        del a_col, a_sorted, b_col, buf
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
