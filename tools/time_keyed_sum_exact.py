#!/usr/bin/env python3
"""time_keyed_sum_exact.py: the exact keyed SUM for up to 2^20 keys (alpgpu_decode_keyed_exact_sum_*: integers in a fixed-point table in device memory,
rounded once) against the routes a caller had without it, in one process.  tools/time_keyed_minmax_many.py's method and shapes: one device, arms
ALTERNATE, each warmed up, device events around each arm, median ms of the repetitions with the arm's min-max spread.

Value columns: bench.py's mixed ALP column, the all-ALP_RD double column (bench.py "rd") and a float column (tools/time_select.py's).  Beside each a key
column of the same type with K distinct values (multiples of 0.25: ALP vectors without exceptions), K in {1024, 4096, 16 Ki, 64 Ki, 1 Mi}, once in
random order and once sorted, the sorted one with its zone map (prepared ahead, outside the timed region).  Bitmap in {NULL, uniformly random of density
0.1, 1e-2}.
  (a) new       keyed_sum_exact_into(val, key, keys, bitmap) WITHOUT counts, into a table made ahead (the sorted key column: with zones=zone_map(key))
  (b) counts    the same call with counts
  (c) rounds    double columns, today's route: ceil(K / 1024) rounds of keyed_sum_into over consecutive slices of 1024 keys, each with counts.  Left out
                above --rounds-max-keys (each round is a pass over both columns); its cells then say so.  Float columns have no such route.
  (d) decode    decode_masked of both columns (NULL bitmap: decode) + torch.searchsorted + == + index_add_ into float64 + bincount: both columns
                materialised; the only route a float column had.  --no-decode leaves it out (take its figures from a run with fewer --vectors).
  (e) floor     keyed_minmax_many_into without counts on the same pair: the same decode and search with a cheaper update.
The sums of (a) and (b) are compared byte for byte, the counts of (b) and (c) as integers.  The sums of (c) and (d) are floating-point sums in an
order of their own and are NOT expected to be the exact sums' bits; the line reports in how many keys they differ and the largest relative difference.
  python3 tools/time_keyed_sum_exact.py [--vectors N] [--reps R] [--columns mixed,rd,float] [--keys 1024,4096,...] [--rounds-max-keys K] [--no-decode] [--out FILE]"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KEYS = (1024, 4096, 1 << 14, 1 << 16, 1 << 20)
BITMAPS = (None, 0.1, 1e-2)
SLICE = 1024  # KEYED_KEYS_MAX: what one round of today's route takes


def key_values(torch, nv, K, tdt, dev, in_order):
    g = torch.Generator(device=dev)
    g.manual_seed(40 + K)
    k = torch.randint(0, K, (nv * 1024,), device=dev, generator=g)
    if in_order:
        k = torch.sort(k).values
    return (k.to(torch.float64) * 0.25).to(tdt)


def differ(torch, a, b):
    """(keys whose sums differ by their bits, the largest |a - b| / max(|a|, tiny) over the finite ones)"""
    n = int((a.view(torch.int64) != b.view(torch.int64)).sum())
    ok = torch.isfinite(a) & torch.isfinite(b)
    rel = float(((a[ok] - b[ok]).abs() / a[ok].abs().clamp_min(1e-300)).max()) if bool(ok.any()) else 0.0
    return n, rel


def run_column(ctx, name, x, reps, key_counts, emit, with_decode=True, rounds_max_keys=1 << 16):
    import torch
    from time_mask import fmt
    from time_select import alternate
    from time_take_masked import random_bitmap
    dev = x.device
    val = ctx.encode(x)
    tdt = x.dtype
    is_double = tdt == torch.float64
    del x
    nv = val.n_vectors
    emit(f"== {name}: {nv} vectors")
    mask = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    if with_decode:
        bufv = torch.empty(nv * 1024, dtype=tdt, device=dev)
        bufk = torch.empty(nv * 1024, dtype=tdt, device=dev)
        n_sel = torch.empty(1, dtype=torch.int64, device=dev)
        sel_scratch = ctx.select_scratch(val)
    round_scratch = ctx.keyed_sum_scratch(nv, SLICE) if is_double else None
    arms = ("new", "counts", "rounds", "decode", "floor")
    head = " ".join(f"{n + ' ms':>27s}" for n in arms)
    emit(f"  {'K':>7s} {'key column':>12s} {'bitmap':>6s} {head} {'rounds/new':>10s} {'rounds/cnt':>10s} {'decode/cnt':>10s} {'new/floor':>9s}  the new call with counts beats the rounds by more than the spreads")
    nan3 = (float("nan"),) * 3
    for K in key_counts:
        keys = (torch.arange(K, dtype=torch.float64, device=dev) * 0.25).to(tdt)
        n_rounds = (K + SLICE - 1) // SLICE
        with_rounds = is_double and K <= rounds_max_keys
        table = ctx.keyed_sum_exact_table(K)
        for kname, in_order in (("random", False), ("sorted+zones", True)):
            kx = key_values(torch, nv, K, tdt, dev, in_order)
            key = ctx.encode(kx)
            del kx
            zones = ctx.zone_map(key) if in_order else None
            sum_a = torch.empty(K, dtype=torch.float64, device=dev)
            sum_b = torch.empty(K, dtype=torch.float64, device=dev)
            cnt_b = torch.empty(K + 1, dtype=torch.int64, device=dev)
            sum_c = torch.empty(K, dtype=torch.float64, device=dev)
            cnt_c = torch.empty((n_rounds, SLICE + 1), dtype=torch.int64, device=dev)  # a round's counts: its keys' and its own "without a key" word
            sum_d = torch.empty(K, dtype=torch.float64, device=dev)
            rec_e = torch.empty((K, 2), dtype=tdt, device=dev)
            for density in BITMAPS:
                if density is not None:
                    random_bitmap(mask, nv, density, False, 90)
                m = None if density is None else mask

                def new():
                    ctx.keyed_sum_exact_into(val, key, keys, sum_a, mask=m, zones=zones, table=table)

                def counts():
                    ctx.keyed_sum_exact_into(val, key, keys, sum_b, counts_out=cnt_b, mask=m, zones=zones, table=table)

                def rounds():
                    for r in range(n_rounds):
                        k0, k1 = r * SLICE, min(K, (r + 1) * SLICE)
                        ctx.keyed_sum_into(val, key, keys[k0:k1], sum_c[k0:k1], counts_out=cnt_c[r, : k1 - k0 + 1], mask=m, zones=zones, scratch=round_scratch)

                def floor():
                    ctx.keyed_minmax_many_into(val, key, keys, rec_e, mask=m, zones=zones)

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
                    found = keys[at] == xk
                    torch.bincount(at[found], minlength=K)
                    sum_d.zero_()
                    sum_d.index_add_(0, at[found], xv[found].to(torch.float64))

                bm = "NULL" if density is None else format(density, "g")
                t = alternate([("new", new), ("counts", counts)] + ([("rounds", rounds)] if with_rounds else []) + ([("decode", decode)] if with_decode else [])
                              + [("floor", floor)], reps, warmup=1)
                ta, tb, tc, td, te = t["new"], t["counts"], t.get("rounds", nan3), t.get("decode", nan3), t["floor"]
                note = ""
                if sum_a.cpu().numpy().tobytes() != sum_b.cpu().numpy().tobytes():
                    note += "  WRONG RESULT (sums differ with and without counts)"
                if with_rounds:
                    per_key = torch.cat([cnt_c[r, : min(K, (r + 1) * SLICE) - r * SLICE] for r in range(n_rounds)])
                    if not torch.equal(per_key, cnt_b[:K]):
                        note += "  WRONG RESULT (counts differ from the rounds')"
                    note += "  against the rounds %d keys differ, at most %.1e relative" % differ(torch, sum_b, sum_c)
                if with_decode:
                    note += "  against the decode route %d keys differ, at most %.1e relative" % differ(torch, sum_b, sum_d)
                if with_rounds:
                    spread = max(tb[2] - tb[1], tc[2] - tc[1])
                    verdict = f"{'yes' if tc[0] - tb[0] > spread else ('NO, it LOSES' if tb[0] - tc[0] > spread else 'NO, level')} ({tc[0] - tb[0]:+.3f} ms, spread {spread:.3f} ms)"
                else:
                    verdict = "rounds not run: " + (f"{n_rounds} passes over both columns" if is_double else "keyed_sum_into takes double columns only")
                emit(f"  {K:7d} {kname:>12s} {bm:>6s} {fmt(ta)} {fmt(tb)} {fmt(tc)} {fmt(td)} {fmt(te)} {tc[0] / ta[0]:10.2f} {tc[0] / tb[0]:10.2f} {td[0] / tb[0]:10.2f} {ta[0] / te[0]:9.2f}  {verdict}{note}")
            del key, zones
            torch.cuda.empty_cache()
        del table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--columns", default="mixed,rd,float")
    ap.add_argument("--keys", default=",".join(str(k) for k in KEYS))
    ap.add_argument("--rounds-max-keys", type=int, default=1 << 16, help="the rounds arm is left out above this many keys (default 65536: 64 passes)")
    ap.add_argument("--no-decode", action="store_true", help="leave the decode arm out (its columns print nan)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    from alp_amd import capi
    from time_select import float_column
    dev = torch.device("cuda:0")
    ctx = capi.Context(0)
    sha = hashlib.sha256(open(capi.lib._name, "rb").read()).hexdigest()[:16]
    out = open(a.out, "a") if a.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    emit(f"time_keyed_sum_exact.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after the warm-up, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_keyed_sum_exact.py {' '.join(sys.argv[1:])}".rstrip())
    nv = a.vectors
    kinds = {"mixed": ("mixed double (bench.py mixed)", lambda: bench.synthetic_input("mixed", nv, dev, seed=1)),
             "rd": ("ALP_RD double (bench.py rd)", lambda: bench.synthetic_input("rd", nv, dev, seed=1)),
             "float": ("float (two decimals, 1 % full precision)", lambda: float_column(nv, dev))}
    for key in a.columns.split(","):
        name, make = kinds[key]
        run_column(ctx, name, make(), a.reps, [int(k) for k in a.keys.split(",")], emit, with_decode=not a.no_decode, rounds_max_keys=a.rounds_max_keys)
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
