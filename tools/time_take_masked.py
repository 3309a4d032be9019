#!/usr/bin/env python3
"""time_take_masked.py: the masked projection (alpgpu_decode_masked_*) against the two routes a caller had without it, in one process.

Columns (1 Mi vectors each, those of time_mask.py): bench.py's mixed ALP column, the all-ALP_RD double column (bench.py "rd") and the float column of
time_select.py.  Bitmaps of density {1e-4, 1e-2, 0.1, 0.5, 1}: uniformly random bits, and whole vectors (clustered: a vector is all ones or all zeros).
  masked        decode_masked_into: values only (what a projection needs), and with the indices written beside them
  gather        mask_to_indices + gather: the route before this entry point
  decode+index  decode of the whole column + mask_to_indices + torch.index_select
Beside them, per column: the count + scan share of the call (capacity 0), the whole call under an empty bitmap, and the call at density 1 beside
alpgpu_decode_* of the same column (the floor: the same bytes out, plus 128 bytes of bitmap per vector in).
Arms ALTERNATE, each warmed up, device events around each arm: median ms with the arm's min-max spread.
  python3 tools/time_take_masked.py [--vectors N] [--reps R] [--out FILE]"""
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

GRID = (1e-4, 1e-2, 0.1, 0.5, 1.0)


def random_bitmap(mask, nv, density, clustered, seed):
    """fills mask (16 * nv int64 words): clustered, a vector is all ones with probability `density`; else every bit is set with that probability"""
    dev = mask.device
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    if clustered:
        keep = torch.rand(nv, device=dev, generator=g) < density if density < 1.0 else torch.ones(nv, dtype=torch.bool, device=dev)
        mask.reshape(nv, 16).copy_(torch.where(keep, -1, 0).to(torch.int64).reshape(nv, 1).expand(nv, 16))
        return
    w = torch.ones(64, dtype=torch.int64, device=dev) << torch.arange(64, dtype=torch.int64, device=dev)
    step = 1 << 16  # vectors per chunk
    for v0 in range(0, nv, step):
        n = min(step, nv - v0)
        bits = torch.rand(n * 1024, device=dev, generator=g) < density if density < 1.0 else torch.ones(n * 1024, dtype=torch.bool, device=dev)
        mask[16 * v0:16 * (v0 + n)] = (bits.reshape(-1, 64).to(torch.int64) * w).sum(dim=1)


def ibits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def run_column(ctx, name, x, reps, emit):
    dev = x.device
    col = ctx.encode(x)
    del x
    pb, eb, _ = ctx.column_totals(col)
    nv = col.n_vectors
    n = nv * 1024
    tdt = torch.float64 if col.dtype == "f64" else torch.float32
    vb = 8 if col.dtype == "f64" else 4
    mask = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    idx = torch.empty(n, dtype=torch.int64, device=dev)
    idx2 = torch.empty(n, dtype=torch.int64, device=dev)
    vals = torch.empty(n, dtype=tdt, device=dev)
    vals2 = torch.empty(n, dtype=tdt, device=dev)
    full = torch.empty(n, dtype=tdt, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = ctx.select_scratch(col)
    emit(f"== {name}: {nv} vectors, {pb / (128.0 * nv):.2f} packed bits per value, {eb / nv:.0f} exception bytes per vector, compressed {(32 * nv + pb + eb) / 1e9:.3f} GB, "
         f"bitmap {128 * nv / 1e6:.1f} MB")
    emit(f"  {'bits':>9s} {'density':>7s} {'selected':>11s} {'masked ms':>28s} {'masked + indices ms':>28s} {'indices + gather ms':>28s} {'decode + index_select ms':>28s} "
         f"{'gather/masked':>13s} {'decode/masked':>13s} {'Gvalues/s':>9s}")
    for clustered in (False, True):
        for i, d in enumerate(GRID):
            random_bitmap(mask, nv, d, clustered, 50 + i)
            ctx.decode_masked_into(col, mask, None, count, scratch=scratch)
            k = int(count)
            res = {}

            def masked():
                ctx.decode_masked_into(col, mask, vals[:k] if k else None, count, None, scratch)

            def masked_idx():
                ctx.decode_masked_into(col, mask, vals[:k] if k else None, count, idx2[:k] if k else None, scratch)

            def by_gather():
                ctx.mask_to_indices_into(mask, idx[:k] if k else None, count, scratch)
                ctx.gather(col, idx[:k], out=vals2[:k])

            def by_decode():
                ctx.decode(col, full)
                ctx.mask_to_indices_into(mask, idx[:k] if k else None, count, scratch)
                res["v"] = torch.index_select(full, 0, idx[:k])

            t = alternate([("masked", masked), ("masked_idx", masked_idx), ("gather", by_gather), ("decode", by_decode)], reps, warmup=1)
            ok = torch.equal(ibits(vals[:k]), ibits(vals2[:k])) and torch.equal(ibits(vals[:k]), ibits(res["v"])) and torch.equal(idx[:k], idx2[:k])
            res.clear()
            tm = t["masked"][0]
            emit(f"  {'vectors' if clustered else 'uniform':>9s} {d:7g} {k:11d} {fmt(t['masked'])} {fmt(t['masked_idx'])} {fmt(t['gather'])} {fmt(t['decode'])} "
                 f"{t['gather'][0] / tm:13.2f} {t['decode'][0] / tm:13.2f} {k / (tm * 1e-3) / 1e9:9.2f}{'' if ok else '  WRONG RESULT'}")
    # the parts of the call, and its floor
    random_bitmap(mask, nv, 0.1, False, 52)
    ctx.decode_masked_into(col, mask, None, count, scratch=scratch)
    k = int(count)
    t = alternate([("count", lambda: ctx.decode_masked_into(col, mask, None, count, scratch=scratch)),
                   ("call", lambda: ctx.decode_masked_into(col, mask, vals[:k], count, None, scratch))], reps)
    emit(f"  count + scan (capacity 0), uniform 0.1: {fmt(t['count'])} ms of the call's {fmt(t['call'])} ms: {t['count'][0] / t['call'][0]:.3f}")
    mask.zero_()
    t = alternate([("count", lambda: ctx.decode_masked_into(col, mask, None, count, scratch=scratch)),
                   ("call", lambda: ctx.decode_masked_into(col, mask, vals[:n], count, None, scratch))], reps)
    emit(f"  empty bitmap: the call {fmt(t['call'])} ms, its count + scan {fmt(t['count'])} ms, so the emit pass {t['call'][0] - t['count'][0]:.3f} ms")
    mask.fill_(-1)
    t = alternate([("call", lambda: ctx.decode_masked_into(col, mask, vals[:n], count, None, scratch)), ("decode", lambda: ctx.decode(col, full)),
                   ("count", lambda: ctx.decode_masked_into(col, mask, None, count, scratch=scratch))], reps)
    ok = torch.equal(ibits(vals), ibits(full))
    emit(f"  full bitmap: the call {fmt(t['call'])} ms ({(n * vb) / (t['call'][0] * 1e-3) / 1e12:.2f} TB/s of values written), its count + scan {fmt(t['count'])} ms, "
         f"alpgpu_decode_* {fmt(t['decode'])} ms ({(n * vb) / (t['decode'][0] * 1e-3) / 1e12:.2f} TB/s): emit pass / decode {(t['call'][0] - t['count'][0]) / t['decode'][0]:.2f}, "
         f"call / decode {t['call'][0] / t['decode'][0]:.2f}{'' if ok else '  WRONG RESULT'}")


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

    emit(f"time_take_masked.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after the warm-ups, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_take_masked.py {' '.join(sys.argv[1:])}".rstrip())
    nv = a.vectors
    kinds = (("mixed double (bench.py mixed)", lambda: bench.synthetic_input("mixed", nv, dev, seed=1)),
             ("ALP_RD double (bench.py rd)", lambda: bench.synthetic_input("rd", nv, dev, seed=1)),
             ("float, two decimals + 1 % exceptions", lambda: float_column(nv, dev, seed=1)))
    for name, make in kinds:
        run_column(ctx, name, make(), a.reps, emit)
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
