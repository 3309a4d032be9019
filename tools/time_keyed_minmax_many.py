#!/usr/bin/env python3
"""time_keyed_minmax_many.py: keyed MIN / MAX for up to 2^20 keys (alpgpu_decode_keyed_minmax_many_*: the table in device memory) against the routes a
caller had without it, in one process.  tools/time_keyed_minmax.py's method: one device, arms ALTERNATE, each warmed up, device events around each arm,
median ms of the repetitions with the arm's min-max spread, results compared bit for bit between arms.

Value columns: bench.py's mixed ALP column, the all-ALP_RD double column (bench.py "rd") and a float column (tools/time_select.py's).  Beside each a key
column of the same type with K distinct values (multiples of 0.25: ALP vectors without exceptions), K in {1024, 4096, 16 Ki, 64 Ki, 1 Mi}, once in
random order and once sorted, the sorted one with its zone map (prepared ahead, outside the timed region).  Bitmap in {NULL, uniformly random of density
0.1, 1e-2}.
  (a) new       keyed_minmax_many_into(val, key, keys, bitmap) WITHOUT counts (the sorted key column: with zones=zone_map(key))
  (b) counts    the same call with counts
  (c) rounds    today's route: ceil(K / 1024) rounds of keyed_minmax_into over consecutive slices of 1024 keys, each with counts.  Left out above
                --rounds-max-keys (each round is a pass over both columns); its cells then say so.
  (d) decode    decode_masked of both columns (NULL bitmap: decode) + torch.searchsorted + == + scatter_reduce_ amin / amax + bincount: both columns
                materialised.  --no-decode leaves it out (take its figures from a run with fewer --vectors).
  (e) old       at K = 1024 only: keyed_minmax_into alone (the LDS table), which is also what (c) is there.
Records of (a), (b) and (c) and counts of (b) and (c) are compared bit for bit in every cell; (e)'s with (b)'s.  No arm but (a) and (b) uses the new call.
  python3 tools/time_keyed_minmax_many.py [--vectors N] [--reps R] [--columns mixed,rd,float] [--keys 1024,4096,...] [--rounds-max-keys K] [--no-decode] [--out FILE]"""
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


def run_column(ctx, name, x, reps, key_counts, emit, with_decode=True, rounds_max_keys=1 << 16):
    import torch
    from time_mask import fmt
    from time_select import alternate
    from time_take_masked import random_bitmap
    dev = x.device
    val = ctx.encode(x)
    tdt = x.dtype
    del x
    nv = val.n_vectors
    emit(f"== {name}: {nv} vectors")
    mask = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    if with_decode:
        bufv = torch.empty(nv * 1024, dtype=tdt, device=dev)
        bufk = torch.empty(nv * 1024, dtype=tdt, device=dev)
        n_sel = torch.empty(1, dtype=torch.int64, device=dev)
        sel_scratch = ctx.select_scratch(val)
    arms = ("new", "counts", "rounds", "decode", "old")
    head = " ".join(f"{n + ' ms':>27s}" for n in arms)
    emit(f"  {'K':>7s} {'key column':>12s} {'bitmap':>6s} {head} {'rounds/new':>10s} {'rounds/cnt':>10s} {'decode/cnt':>10s} {'cnt/old':>8s}  the new call with counts beats the rounds by more than the spreads")
    nan3 = (float("nan"),) * 3
    for K in key_counts:
        keys = (torch.arange(K, dtype=torch.float64, device=dev) * 0.25).to(tdt)
        n_rounds = (K + SLICE - 1) // SLICE
        with_rounds = K <= rounds_max_keys
        for kname, in_order in (("random", False), ("sorted+zones", True)):
            kx = key_values(torch, nv, K, tdt, dev, in_order)
            key = ctx.encode(kx)
            del kx
            zones = ctx.zone_map(key) if in_order else None
            rec_a = torch.empty((K, 2), dtype=tdt, device=dev)
            rec_b = torch.empty((K, 2), dtype=tdt, device=dev)
            cnt_b = torch.empty(K + 1, dtype=torch.int64, device=dev)
            rec_c = torch.empty((K, 2), dtype=tdt, device=dev)
            cnt_c = torch.empty((n_rounds, SLICE + 1), dtype=torch.int64, device=dev)  # a round's counts: its keys' and its own "without a key" word
            rec_e = torch.empty((min(K, SLICE), 2), dtype=tdt, device=dev)
            cnt_e = torch.empty(min(K, SLICE) + 1, dtype=torch.int64, device=dev)
            dmn = torch.empty(K, dtype=tdt, device=dev)
            dmx = torch.empty(K, dtype=tdt, device=dev)
            for density in BITMAPS:
                if density is not None:
                    random_bitmap(mask, nv, density, False, 90)
                m = None if density is None else mask

                def new():
                    ctx.keyed_minmax_many_into(val, key, keys, rec_a, mask=m, zones=zones)

                def counts():
                    ctx.keyed_minmax_many_into(val, key, keys, rec_b, counts_out=cnt_b, mask=m, zones=zones)

                def rounds():
                    for r in range(n_rounds):
                        k0, k1 = r * SLICE, min(K, (r + 1) * SLICE)
                        ctx.keyed_minmax_into(val, key, keys[k0:k1], rec_c[k0:k1], counts_out=cnt_c[r, : k1 - k0 + 1], mask=m, zones=zones)

                def old():
                    ctx.keyed_minmax_into(val, key, keys, rec_e, counts_out=cnt_e, mask=m, zones=zones)

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
                    hit = found & ~torch.isnan(xv)
                    dmn.fill_(float("inf"))
                    dmx.fill_(float("-inf"))
                    dmn.scatter_reduce_(0, at[hit], xv[hit], "amin")
                    dmx.scatter_reduce_(0, at[hit], xv[hit], "amax")

                bm = "NULL" if density is None else format(density, "g")
                t = alternate([("new", new), ("counts", counts)] + ([("rounds", rounds)] if with_rounds else []) + ([("decode", decode)] if with_decode else [])
                              + ([("old", old)] if K <= SLICE else []), reps, warmup=1)
                ta, tb, tc, td, te = t["new"], t["counts"], t.get("rounds", nan3), t.get("decode", nan3), t.get("old", nan3)
                note = ""
                if rec_a.cpu().numpy().tobytes() != rec_b.cpu().numpy().tobytes():
                    note += "  WRONG RESULT (records differ with and without counts)"
                if with_rounds:
                    if rec_c.cpu().numpy().tobytes() != rec_b.cpu().numpy().tobytes():
                        note += "  WRONG RESULT (records differ from the rounds')"
                    per_key = torch.cat([cnt_c[r, : min(K, (r + 1) * SLICE) - r * SLICE] for r in range(n_rounds)])
                    if not torch.equal(per_key, cnt_b[:K]):
                        note += "  WRONG RESULT (counts differ from the rounds')"
                if K <= SLICE and (rec_e.cpu().numpy().tobytes() != rec_b.cpu().numpy().tobytes() or not torch.equal(cnt_e, cnt_b)):
                    note += "  WRONG RESULT (differs from keyed_minmax_into)"
                if with_rounds:
                    spread = max(tb[2] - tb[1], tc[2] - tc[1])
                    verdict = f"{'yes' if tc[0] - tb[0] > spread else ('NO, it LOSES' if tb[0] - tc[0] > spread else 'NO, level')} ({tc[0] - tb[0]:+.3f} ms, spread {spread:.3f} ms)"
                else:
                    verdict = f"rounds not run: {n_rounds} passes over both columns"
                emit(f"  {K:7d} {kname:>12s} {bm:>6s} {fmt(ta)} {fmt(tb)} {fmt(tc)} {fmt(td)} {fmt(te)} {tc[0] / ta[0]:10.2f} {tc[0] / tb[0]:10.2f} {td[0] / tb[0]:10.2f} {tb[0] / te[0]:8.2f}  {verdict}{note}")
            del key, zones
            torch.cuda.empty_cache()


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

    emit(f"time_keyed_minmax_many.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after the warm-up, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_keyed_minmax_many.py {' '.join(sys.argv[1:])}".rstrip())
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
