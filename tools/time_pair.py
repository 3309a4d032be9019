#!/usr/bin/env python3
"""time_pair.py: the two-column consumers (alpgpu_compare_mask_*, alpgpu_decode_dot_masked_*) against the routes a caller had without them and
against their floors, in one process.

Column pairs (1 Mi vectors each, the columns of time_mask.py, each paired with a differently seeded twin): bench.py's mixed ALP column, the
all-ALP_RD double column (bench.py "rd") and the float column of time_select.py.
  compare SET     compare_mask(a, b, "lt") beside   decode + compare + pack: decode(a), decode(b), torch.lt and the bits packed 64 to a word, and
                  the floor: select_mask(a, SET) + select_mask(b, SET), which reads the same compressed bytes and writes one more bitmap
  compare AND     over a prior bitmap with 0 %, 1 %, 10 % and 100 % of the vectors open (all ones) and the others all zero
  dot             decode_dot_masked(a, b) under bitmaps of density {1e-4, 1e-2, 0.1, 0.5, 1}, uniformly random bits and whole vectors, beside
                  decode_masked(a) + decode_masked(b) + torch.dot, and the floor: decode_sum_masked(a) + decode_sum_masked(b)
Arms ALTERNATE, each warmed up, device events around each arm: median ms with the arm's min-max spread.
  python3 tools/time_pair.py [--vectors N] [--reps R] [--out FILE]"""
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
from time_take_masked import random_bitmap  # noqa: E402

GRID = (1e-4, 1e-2, 0.1, 0.5, 1.0)
OPEN = (0.0, 0.01, 0.1, 1.0)


def pack_into(bits, out, w):
    """bool tensor of whole vectors -> the bitmap, 64 bits to an int64 word, in chunks (the intermediate is eight times the bitmap)"""
    step = 1 << 26
    for r0 in range(0, bits.numel(), step):
        out[r0 >> 6:(r0 + step) >> 6] = (bits[r0:r0 + step].reshape(-1, 64).to(torch.int64) * w).sum(dim=1)


def run_pair(ctx, name, xa, xb, reps, emit):
    dev = xa.device
    ca, cb = ctx.encode(xa), ctx.encode(xb)
    del xa, xb
    (pa, ea, _), (pb, eb, _) = ctx.column_totals(ca), ctx.column_totals(cb)
    nv = ca.n_vectors
    n = nv * 1024
    tdt = torch.float64 if ca.dtype == "f64" else torch.float32
    compressed = 64 * nv + pa + ea + pb + eb
    emit(f"== {name}: 2 x {nv} vectors, {pa / (128.0 * nv):.2f} and {pb / (128.0 * nv):.2f} packed bits per value, {ea / nv:.0f} and {eb / nv:.0f} exception bytes per vector, "
         f"compressed {compressed / 1e9:.3f} GB together, bitmap {128 * nv / 1e6:.1f} MB")
    mask = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    m2 = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    m3 = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    prior = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    da = torch.empty(n, dtype=tdt, device=dev)
    db = torch.empty(n, dtype=tdt, device=dev)
    w = torch.ones(64, dtype=torch.int64, device=dev) << torch.arange(64, dtype=torch.int64, device=dev)

    # ---- compare_mask SET: the new call, today's route, the floor
    def today():
        ctx.decode(ca, da)
        ctx.decode(cb, db)
        pack_into(da < db, m2, w)

    def floor():
        ctx.select_mask(ca, -1.0, 1.0, mask=m2)
        ctx.select_mask(cb, -1.0, 1.0, mask=m3)

    t = alternate([("pair", lambda: ctx.compare_mask(ca, cb, "lt", mask=mask)), ("floor", floor), ("today", today)], reps, warmup=1)
    today()
    ok = torch.equal(ctx.compare_mask(ca, cb, "lt", mask=mask), m2)
    tp, tf = t["pair"], t["floor"]
    over = tp[0] - tf[0]
    spread = max(tp[2] - tp[1], tf[2] - tf[1])
    emit(f"  compare_mask SET   {fmt(tp)} ms ({compressed / (tp[0] * 1e-3) / 1e12:.2f} TB/s of compressed bytes);  floor select_mask(a) + select_mask(b) {fmt(tf)} ms;  "
         f"decode + decode + torch.lt + pack {fmt(t['today'])} ms: {t['today'][0] / tp[0]:.1f} x;  pair - floor {over:+.3f} ms, the arms' spread {spread:.3f} ms"
         f"{'' if ok else '  WRONG RESULT'}")

    # ---- compare_mask AND over a prior with a share of the vectors open
    emit(f"  {'open':>6s} {'open vectors':>12s} {'compare_mask AND ms':>28s} {'floor: select_mask AND x 2 ms':>30s}")
    for i, f in enumerate(OPEN):
        random_bitmap(prior, nv, f, True, 70 + i)
        open_vectors = int((prior.reshape(nv, 16) != 0).any(dim=1).sum())

        def pair_and():
            mask.copy_(prior)
            ctx.compare_mask(ca, cb, "lt", op="and", mask=mask)

        def floor_and():
            m2.copy_(prior)
            ctx.select_mask(ca, -1e30, 1e30, op="and", mask=m2)  # (keeps every open vector open for the second predicate)
            ctx.select_mask(cb, -1e30, 1e30, op="and", mask=m2)

        def copy_only():
            mask.copy_(prior)

        t = alternate([("pair", pair_and), ("floor", floor_and), ("copy", copy_only)], reps, warmup=1)
        emit(f"  {f:6g} {open_vectors:12d} {fmt(t['pair'])} {fmt(t['floor'])}   (of which the bitmap's copy {t['copy'][0]:.3f} ms)")

    # ---- decode_dot_masked
    sums = torch.empty(nv, dtype=torch.float64, device=dev)
    s2 = torch.empty(nv, dtype=torch.float64, device=dev)
    s3 = torch.empty(nv, dtype=torch.float64, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    scratch = ctx.select_scratch(ca)
    emit(f"  {'bits':>9s} {'density':>7s} {'selected':>11s} {'dot_masked + tree_sum ms':>28s} {'floor: sum_masked x 2 ms':>28s} {'decode_masked x 2 + dot ms':>28s} {'today/dot':>9s} {'dot/floor':>9s}")
    for clustered in (False, True):
        for i, d in enumerate(GRID):
            random_bitmap(mask, nv, d, clustered, 50 + i)
            ctx.decode_masked_into(ca, mask, None, count, scratch=scratch)
            k = int(count)
            res = {}

            def dot():
                ctx.decode_dot_masked(ca, cb, mask, out=sums)
                ctx.tree_sum(sums, out=total)

            def floor_sum():
                ctx.decode_sum_masked(ca, mask, out=s2)
                ctx.decode_sum_masked(cb, mask, out=s3)

            def today_dot():
                ctx.decode_masked_into(ca, mask, da[:k] if k else None, count, None, scratch)
                ctx.decode_masked_into(cb, mask, db[:k] if k else None, count, None, scratch)
                res["v"] = torch.dot(da[:k].to(torch.float64), db[:k].to(torch.float64)) if tdt != torch.float64 else torch.dot(da[:k], db[:k])

            t = alternate([("dot", dot), ("floor", floor_sum), ("today", today_dot)], reps, warmup=1)
            got, want = float(total), float(res["v"])
            ok = got == want or abs(got - want) <= 1e-9 * max(abs(want), float((da[:k].to(torch.float64) * db[:k].to(torch.float64)).abs().sum())) or (got != got and want != want)
            res.clear()
            emit(f"  {'vectors' if clustered else 'uniform':>9s} {d:7g} {k:11d} {fmt(t['dot'])} {fmt(t['floor'])} {fmt(t['today'])} {t['today'][0] / t['dot'][0]:9.2f} "
                 f"{t['dot'][0] / t['floor'][0]:9.2f}{'' if ok else '  WRONG RESULT'}")


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

    emit(f"time_pair.py: {ctx.device_info()['name']}, 2 x {a.vectors} vectors per pair, arms alternating, {a.reps} repetitions after the warm-up, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_pair.py {' '.join(sys.argv[1:])}".rstrip())
    nv = a.vectors
    kinds = (("mixed double (bench.py mixed)", lambda s: bench.synthetic_input("mixed", nv, dev, seed=s)),
             ("ALP_RD double (bench.py rd)", lambda s: bench.synthetic_input("rd", nv, dev, seed=s)),
             ("float, two decimals + 1 % exceptions", lambda s: float_column(nv, dev, seed=s)))
    for name, make in kinds:
        run_pair(ctx, name, make(1), make(2), a.reps, emit)
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
