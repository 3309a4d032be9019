#!/usr/bin/env python3
"""time_keyed_minmax.py: keyed MIN / MAX (alpgpu_decode_keyed_minmax_*: the record {min, max} and the COUNT of a value column per key of a sorted key
list, under a bitmap) against the routes a caller had without it, in one process.  tools/time_keyed.py's method: one device, arms ALTERNATE, each warmed
up, device events around each arm, median ms of the repetitions with the arm's min-max spread, results compared bit for bit between arms.

Value columns: bench.py's mixed ALP column, the all-ALP_RD double column (bench.py "rd") and a float column (tools/time_select.py's).  Beside each a key
column of the same type with K distinct values (multiples of 0.25: ALP vectors without exceptions), K in {16, 64, 256, 1024}, once in random order and
once sorted, the sorted one with its zone map (prepared ahead, outside the timed region).  Bitmap in {NULL, uniformly random of density 0.1, 1e-2}.
  new       keyed_minmax_into(val, key, keys, bitmap) into given tensors (the sorted key column: with zones=zone_map(key))
  rounds    today's compressed route: ceil(K / 16) rounds of decode_group_minmax(val, key, bitmap, [k, k]) + group_minmax_totals; under the NULL bitmap
            it takes a bitmap of all ones.  Its records are compared with the new call's bit for bit.
  sum       keyed_sum_into on the same pair (double columns only): the same decode and search with another table behind it, a floor for the new call
  decode    decode_masked of both columns (NULL bitmap: decode) + torch.searchsorted + scatter_reduce_ amin / amax: both columns materialised.  Slow
            where many rows meet on few keys; --no-decode leaves it out (take its figures from a run with fewer --vectors).
No arm but `new` uses the new call.

--ab [LIB]: instead of the other routes, the same call from this library and from a build of keyed_minmax_kernels.hip with
-DALPGPU_KEYED_MINMAX_NO_GUARD (every number issues both LDS atomics, no read in front), arms alternating, records and counts compared bit for bit.
Without LIB the variant is build/libalpgpu_kmm_noguard.so, built here if it is missing (--build-variant builds it and exits: no device needed).
  python3 tools/time_keyed_minmax.py [--vectors N] [--reps R] [--columns mixed,rd,float] [--keys 16,64,...] [--ab [LIB]] [--no-decode] [--out FILE]"""
import argparse
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KEYS = (16, 64, 256, 1024)
BITMAPS = (None, 0.1, 1e-2)
VARIANT = os.path.join(ROOT, "build", "libalpgpu_kmm_noguard.so")
VARIANT_FLAG = "-DALPGPU_KEYED_MINMAX_NO_GUARD"


def build_variant(path=VARIANT):
    """the library with keyed_minmax_kernels.hip compiled under VARIANT_FLAG; every other source as build() compiles it (its object is reused if there)"""
    import __graft_entry__ as ge
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj_dir = os.path.join(ROOT, "build", "obj")
    os.makedirs(obj_dir, exist_ok=True)
    flags = [f for f in ge.HIPCC_FLAGS if f != "-shared"]
    objs = []
    for s in ge.HIP_SOURCES:
        src, obj = os.path.join(ge.CSRC, s), os.path.join(obj_dir, s[:-4] + ".o")
        if s == "keyed_minmax_kernels.hip":
            obj = os.path.join(obj_dir, "keyed_minmax_kernels_noguard.o")
            subprocess.check_call([hipcc, *flags, VARIANT_FLAG, "-c", src, "-o", obj])
        elif not os.path.exists(obj):
            subprocess.check_call([hipcc, *flags, "-c", src, "-o", obj])
        objs.append(obj)
    subprocess.check_call([hipcc, *ge.HIPCC_FLAGS, "-o", path, *objs])
    return path


def key_values(torch, nv, K, tdt, dev, in_order):
    g = torch.Generator(device=dev)
    g.manual_seed(40 + K)
    k = torch.randint(0, K, (nv * 1024,), device=dev, generator=g)
    if in_order:
        k = torch.sort(k).values
    return (k.to(torch.float64) * 0.25).to(tdt)


def run_column(ctxs, names, name, x, reps, key_counts, emit, with_decode=True):
    """ctxs[0]: this library; ctxs[1:]: variants (--ab), which replace the other routes"""
    import torch
    from time_mask import fmt
    from time_select import alternate
    from time_take_masked import random_bitmap
    ctx, ab = ctxs[0], len(ctxs) > 1
    dev = x.device
    vals = [c.encode(x) for c in ctxs]
    val = vals[0]
    tdt = x.dtype
    is_double = tdt == torch.float64
    del x
    nv = val.n_vectors
    emit(f"== {name}: {nv} vectors" + (f"; arms: {', '.join(names)}" if ab else ""))
    mask = torch.empty(16 * nv, dtype=torch.int64, device=dev)
    ones = torch.full((16 * nv,), -1, dtype=torch.int64, device=dev)
    if not ab:
        gz = torch.empty((16, nv, 2), dtype=tdt, device=dev)
        if with_decode:
            bufv = torch.empty(nv * 1024, dtype=tdt, device=dev)
            bufk = torch.empty(nv * 1024, dtype=tdt, device=dev)
            n_sel = torch.empty(1, dtype=torch.int64, device=dev)
            sel_scratch = ctx.select_scratch(val)
    arms = names if ab else ("new", "rounds", "sum", "decode")
    head = " ".join(f"{n + ' ms':>27s}" for n in arms)
    emit(f"  {'K':>4s} {'key column':>12s} {'bitmap':>6s} {head}" + ("  variant / this library" if ab else f" {'rounds/new':>10s} {'decode/new':>10s} {'new/sum':>8s}  new beats the rounds by more than the spreads"))
    for K in key_counts:
        keys = (torch.arange(K, dtype=torch.float64, device=dev) * 0.25).to(tdt)
        key_list = [float(v) for v in keys.tolist()]
        for kname, in_order in (("random", False), ("sorted+zones", True)):
            kx = key_values(torch, nv, K, tdt, dev, in_order)
            kcols = [c.encode(kx) for c in ctxs]
            del kx
            key = kcols[0]
            zones = [c.zone_map(kc) if in_order else None for c, kc in zip(ctxs, kcols)]
            recs = [torch.empty((K, 2), dtype=tdt, device=dev) for _ in ctxs]
            cnts = [torch.empty(K + 1, dtype=torch.int64, device=dev) for _ in ctxs]
            tot = torch.empty((((K + 15) // 16) * 16, 2), dtype=tdt, device=dev)
            if is_double and not ab:
                ssum = torch.empty(K, dtype=torch.float64, device=dev)
                scnt = torch.empty(K + 1, dtype=torch.int64, device=dev)
                sscratch = ctx.keyed_sum_scratch(nv, K)
            dmn = torch.empty(K, dtype=tdt, device=dev)
            dmx = torch.empty(K, dtype=tdt, device=dev)
            for density in BITMAPS:
                if density is not None:
                    random_bitmap(mask, nv, density, False, 90)
                m = None if density is None else mask

                def new(i=0):
                    return lambda: ctxs[i].keyed_minmax_into(vals[i], kcols[i], keys, recs[i], counts_out=cnts[i], mask=m, zones=zones[i])

                def rounds():
                    for r in range(0, K, 16):
                        part = key_list[r:r + 16]
                        g = len(part)
                        ctx.decode_group_minmax(val, key, ones if m is None else m, part, part, out=gz[:g])
                        ctx.group_minmax_totals(gz[:g], out=tot[r:r + g])

                def keyed_sum():
                    ctx.keyed_sum_into(val, key, keys, ssum, counts_out=scnt, mask=m, zones=zones[0], scratch=sscratch)

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
                    hit = (keys[at] == xk) & ~torch.isnan(xv)
                    dmn.fill_(float("inf"))
                    dmx.fill_(float("-inf"))
                    dmn.scatter_reduce_(0, at[hit], xv[hit], "amin")
                    dmx.scatter_reduce_(0, at[hit], xv[hit], "amax")

                bm = "NULL" if density is None else format(density, "g")
                if ab:
                    t = alternate([(names[i], new(i)) for i in range(len(ctxs))], reps, warmup=1)
                    t0 = t[names[0]]
                    notes = []
                    for i in range(1, len(ctxs)):
                        ti = t[names[i]]
                        spread = max(t0[2] - t0[1], ti[2] - ti[1])
                        verdict = "WINS" if t0[0] - ti[0] > spread else ("loses" if ti[0] - t0[0] > spread else "level")
                        same = recs[i].cpu().numpy().tobytes() == recs[0].cpu().numpy().tobytes() and torch.equal(cnts[i], cnts[0])
                        notes.append(f"{ti[0] / t0[0]:.3f} {verdict} ({ti[0] - t0[0]:+.3f} ms, spread {spread:.3f}){'' if same else '  DIFFERENT BYTES'}")
                    emit(f"  {K:4d} {kname:>12s} {bm:>6s} " + " ".join(fmt(t[n]) for n in names) + "  " + "; ".join(notes))
                    continue
                t = alternate([("new", new()), ("rounds", rounds)] + ([("sum", keyed_sum)] if is_double else []) + ([("decode", decode)] if with_decode else []), reps, warmup=1)
                nan3 = (float("nan"),) * 3
                tn, tg, ts, td = t["new"], t["rounds"], t.get("sum", nan3), t.get("decode", nan3)
                note = "" if recs[0].cpu().numpy().tobytes() == tot[:K].cpu().numpy().tobytes() else "  WRONG RESULT (records differ from the rounds')"
                if is_double and not torch.equal(cnts[0], scnt):
                    note += "  WRONG RESULT (counts differ from keyed SUM's)"
                spread = max(tn[2] - tn[1], tg[2] - tg[1])
                verdict = f"{'yes' if tg[0] - tn[0] > spread else ('NO, it LOSES' if tn[0] - tg[0] > spread else 'NO, level')} ({tg[0] - tn[0]:+.3f} ms, spread {spread:.3f} ms)"
                emit(f"  {K:4d} {kname:>12s} {bm:>6s} {fmt(tn)} {fmt(tg)} {fmt(ts)} {fmt(td)} {tg[0] / tn[0]:10.2f} {td[0] / tn[0]:10.2f} {tn[0] / ts[0]:8.2f}  {verdict}{note}")
            del kcols, key, zones
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vectors", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--columns", default="mixed,rd,float")
    ap.add_argument("--keys", default=",".join(str(k) for k in KEYS))
    ap.add_argument("--ab", nargs="?", const=VARIANT, default=None, help="time the build without the guard beside this library (default variant: build/libalpgpu_kmm_noguard.so)")
    ap.add_argument("--build-variant", action="store_true", help="build the variant of --ab and exit")
    ap.add_argument("--no-decode", action="store_true", help="leave the decode arm out (its columns print nan)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.build_variant:
        print(build_variant())
        return
    import torch
    import bench
    from alp_amd import capi
    from time_histogram import load_variant
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

    emit(f"time_keyed_minmax.py: {ctx.device_info()['name']}, {a.vectors} vectors per column, arms alternating, {a.reps} repetitions after the warm-up, device events; median (min-max) in ms")
    emit(f"library sha-256 {sha}; command: python3 tools/time_keyed_minmax.py {' '.join(sys.argv[1:])}".rstrip())
    nv = a.vectors
    kinds = {"mixed": ("mixed double (bench.py mixed)", lambda: bench.synthetic_input("mixed", nv, dev, seed=1)),
             "rd": ("ALP_RD double (bench.py rd)", lambda: bench.synthetic_input("rd", nv, dev, seed=1)),
             "float": ("float (two decimals, 1 % full precision)", lambda: float_column(nv, dev))}
    ctxs, names = [ctx], ["guard"]
    if a.ab:
        if a.ab == VARIANT and not os.path.exists(VARIANT):
            build_variant()
        v = load_variant(a.ab, 0)
        ctxs.append(v.Context(0))
        names.append("no guard")
        emit(f"variant {os.path.relpath(a.ab, ROOT)} ({VARIANT_FLAG}): library sha-256 {hashlib.sha256(open(v.lib._name, 'rb').read()).hexdigest()[:16]}")
    for key in a.columns.split(","):
        name, make = kinds[key]
        run_column(ctxs, names, name, make(), a.reps, [int(k) for k in a.keys.split(",")], emit, with_decode=not a.no_decode)
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()
