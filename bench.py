#!/usr/bin/env python3
"""bench.py — headline benchmark of the MI355X ALP path (BASELINE.json): fused ALP decode (falp + patch) GB/s of
decoded doubles per GPU and fraction of the HBM roofline, with encode GB/s and the reference's CPU path next to it.

    python bench.py --gpus 1 --steps 20 --warmup 3 [--full] [--dump-outputs DIR]
    python bench.py --gpus N --steps K --warmup W [--column-gb 100]      (starts its own N local ranks when no launcher did)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W [--column-gb 100]
(--gpus must equal the launcher's WORLD_SIZE; a mismatch, or fewer visible GPUs than ranks, exits non-zero.)

N = 1 (BASELINE.json configs[1]): 1 Mi vectors (1024 doubles each, 8 GiB decoded) of synthetic decimal doubles,
ALP-encoded, bit widths sweeping 1..53 across rowgroups (rowgroup r has bw = 1 + r mod 53), per-vector
base = splitmix64(42, v) mod 2^bw, (f, e) = (min(12, floor((62-bw) log10 2)), f+2), no exceptions; packed words are
uniform random bits (every bit pattern is a valid FFOR stream of uniform digits).  All inputs are resident in HBM
before the timed region.  A "step" = one alpgpu_decode_f64 over the whole column.  A plain run sets up, warms up, times
the steps and prints the headline.  --full adds the extras: the per-bit-width sweep, exceptions, fused consumers, the
encode legs (configs[2], configs[3]), the float path, and the reference's CPU encode and decode timed on the host cores.
--dump-outputs DIR writes a seeded sample of the last timed step's decoded doubles (dump_outputs) at any N.

N > 1, or --column-gb G at any N (BASELINE.json configs[4]): ONE column of G GB (default 100) of doubles, sharded by
whole rowgroups over the ranks (alp_amd/sharding.py; no collective on the data path).  Two legs under the same
barrier + max-over-ranks clock: DECODE of the rank's shard of the configs[1] column (the headline `value`, so that it
is the same metric at every N) and ENCODE (rowgroup init + vector encode) of the rank's shard of the configs[2] mixed
column, generated on the device from global rowgroup-block seeds (the column is the same whatever N is), then
decoded back and compared bit for bit with the input.  At N = 1 the shard is capped to what fits one GPU and
`config.workload` says so.  `scaling` is "strong": the column is fixed, the shards shrink.

One JSON line is printed by rank 0 (see the driver contract in the task description / DESIGN.md).
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import threading
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
from alp_amd import capi  # noqa: E402  (raises if libalpgpu.so is missing: there is no CPU fallback)
from alp_amd.sharding import rowgroup_shard  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured float4 copy)
VEC = 1024
RG = 100


def splitmix64(x: np.ndarray) -> np.ndarray:
    x = (x + np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
    z = x
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def lib_sha16() -> str:
    return hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()[:16]


def build_decode_column(n_vectors: int, device: int, seed: int, bw_of_rowgroup=None, exc_per_vec=0, first_vector: int = 0, value_bytes: int = 8):
    """Synthetic ALP-encoded column in HBM (descriptors on host -> device; packed words generated on device).  exc_per_vec: one count for every
    vector, or an array with one count per vector whose non-zero entries are all the same (the bimodal column).  value_bytes = 4: a float column
    (32-bit words, bit widths 0..32, 6-byte exception entries, (e, f) within the float tables)."""
    v = np.arange(n_vectors, dtype=np.uint64) + np.uint64(first_vector)  # global vector index of this shard's vectors
    rg = (v // np.uint64(100)).astype(np.int64)
    bw = (1 + rg % (53 if value_bytes == 8 else 32)) if bw_of_rowgroup is None else np.broadcast_to(np.asarray(bw_of_rowgroup), rg.shape)
    bw = bw.astype(np.int64)
    if value_bytes == 8:
        f = np.minimum(12, np.floor((62 - bw) * np.log10(2.0))).astype(np.int64)
        f = np.maximum(f, 0)
        e = f + 2
    else:  # float: 10^f * 2^bw stays inside int32, e <= 10 (Constants<float>::MAX_EXPONENT)
        f = np.clip(np.floor((30 - bw) * np.log10(2.0)).astype(np.int64), 0, 8)
        e = np.minimum(f + 2, 10)
    with np.errstate(over="ignore"):
        base = (splitmix64(v + np.uint64(seed) * np.uint64(0x632BE59BD9B4E019)) % (np.uint64(1) << np.minimum(bw, 30 if value_bytes == 4 else 63).astype(np.uint64))).astype(np.int64)
    cnt = np.broadcast_to(np.asarray(exc_per_vec, dtype=np.int64), (n_vectors,))
    c = int(cnt.max()) if n_vectors else 0
    assert ((cnt == 0) | (cnt == c)).all()
    eb1 = value_bytes + 2  # bytes per exception: the value's bits + a 16-bit position
    rec = (eb1 * c + 7) // 8 * 8
    vec = np.zeros(n_vectors, capi.VECTOR_DTYPE)
    vec["bw"], vec["e"], vec["f"], vec["base"] = bw, e, f, base
    vec["scheme"] = capi.SCHEME_ALP
    vec["exc_cnt"] = cnt
    psz = 128 * bw
    vec["packed_off"] = np.concatenate([[0], np.cumsum(psz)[:-1]]).astype(np.uint64)
    n_rec = int((cnt != 0).sum())
    vec["exc_off"] = ((np.cumsum(cnt != 0) - (cnt != 0)) * rec).astype(np.uint64)
    packed_bytes = int(psz.sum())
    rgs = np.zeros((n_vectors + 99) // 100, capi.ROWGROUP_DTYPE)
    rgs["scheme"] = capi.SCHEME_ALP
    rgs["k"] = 1
    col = capi.DeviceColumn(n_vectors, device, packed_capacity=packed_bytes + 1024, exc_capacity=n_rec * rec + 64, dtype="f64" if value_bytes == 8 else "f32")
    dev = col.vectors.device
    col.vectors.copy_(torch.from_numpy(vec.view(np.uint8).reshape(-1)).to(dev))
    col.rowgroups[: rgs.size * 32] = torch.from_numpy(rgs.view(np.uint8).reshape(-1)).to(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1234 + seed)
    chunk = 1 << 28
    for o in range(0, packed_bytes, chunk):
        m = min(chunk, packed_bytes - o)
        col.packed[o:o + m] = torch.randint(0, 256, (m,), dtype=torch.uint8, device=dev, generator=g)
    if c:
        rng = np.random.default_rng(seed)
        one = np.zeros(rec, np.uint8)
        one[: value_bytes * c] = rng.integers(0, 255, value_bytes * c)
        one[value_bytes * c: eb1 * c] = np.sort(rng.choice(1024, c, replace=False)).astype(np.uint16).view(np.uint8)
        col.exc[: n_rec * rec] = torch.from_numpy(one).to(dev).repeat(n_rec)
    col.totals[0] = packed_bytes
    col.totals[1] = n_rec * rec
    col.c.packed_bytes_hint, col.c.exc_bytes_hint = packed_bytes, n_rec * rec  # what alpgpu_column_totals would report
    col.c.alp_rd_rowgroups_hint = 1  # ... "no ALP_RD rowgroup" (informational)
    # algorithmic bytes per launch: read 128*bw + (8 + 2)*exc + 13, write 8192, per vector (float: 6 bytes per exception, 4096 written)
    alg_bytes = int((128 * bw + eb1 * cnt + 13 + 1024 * value_bytes).sum())
    return col, vec, alg_bytes


DUMP_VECTORS = 4096  # decoded vectors written by --dump-outputs: 4096 x 8 KiB = 32 MiB (the budget is 64 MB)
DUMP_SEED = 20240601


def dump_sample_vectors(n_vectors: int, budget: int = DUMP_VECTORS) -> np.ndarray:
    """the vectors --dump-outputs writes: a fixed, seeded, sorted sample of [0, n_vectors) that always holds the first and the last vector"""
    if n_vectors <= budget:
        return np.arange(n_vectors, dtype=np.int64)
    pick = np.random.default_rng(DUMP_SEED).choice(np.arange(1, n_vectors - 1), budget - 2, replace=False)
    return np.sort(np.concatenate([[0, n_vectors - 1], pick])).astype(np.int64)


def dump_outputs(args, out: torch.Tensor, n_vectors: int, name: str = "decoded_f64") -> None:
    """--dump-outputs DIR: what the timed decode returned in its last step (the caller's output buffer), as DIR/<name>.npy — the sampled
    vectors of dump_sample_vectors(), float64, shape (vectors, 1024).  The inputs are seeded, so two builds can be compared value for value."""
    if not args.dump_outputs:
        return
    idx = dump_sample_vectors(n_vectors, max(2, DUMP_VECTORS // max(1, int(os.environ.get("WORLD_SIZE", "1")))))
    torch.cuda.synchronize()
    sample = out.view(-1, VEC)[torch.from_numpy(idx).to(out.device)].cpu().numpy().astype(np.float64, copy=False)
    os.makedirs(args.dump_outputs, exist_ok=True)
    np.save(os.path.join(args.dump_outputs, name + ".npy"), sample)


def time_launches(fn, iters: int, warmup: int):
    """median / mean ms per launch with HIP events on the launch stream (torch's current stream == ctx stream)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ts = np.array([a.elapsed_time(b) for a, b in evs])
    return float(np.median(ts)), float(ts.mean())


# ---- synthetic inputs of the encode legs ------------------------------------------------------
MIX_BLOCK_RG = 640  # rowgroups per generation block of the mixed column: blocks are aligned to GLOBAL rowgroup indices and
#                     seeded by their index, so the column is the same however it is sharded


def mixed_block(block: int, device, seed: int, exc_rate: float = 0.01) -> torch.Tensor:
    """rowgroups [block * MIX_BLOCK_RG, (block + 1) * MIX_BLOCK_RG) of the mixed column: round(x, d) with x ~ U(-1e5, 1e5),
    d cycling 1, 2, 4 by (global) rowgroup; exc_rate (1 %) full-precision values (injected exceptions, SURVEY.md §8(d) mix 3: rates
    0 / 1 % / 10 %); 0.1 % specials (NaN, +-Inf, -0.0)"""
    g = torch.Generator(device=device)
    g.manual_seed(seed * 1_000_003 + block)
    n = MIX_BLOCK_RG * RG * VEC
    x = (torch.rand(n, dtype=torch.float64, device=device, generator=g) - 0.5) * 2e5
    rg = torch.arange(block * MIX_BLOCK_RG, (block + 1) * MIX_BLOCK_RG, device=device)
    sc = torch.tensor([10.0, 100.0, 10000.0], dtype=torch.float64, device=device)[rg % 3].repeat_interleave(RG * VEC)
    out = torch.round(x * sc) / sc
    del sc
    m = torch.rand(n, device=device, generator=g) < exc_rate
    out[m] = x[m] * 3.141592653589793
    del m, x
    sp = torch.rand(n, device=device, generator=g) < 0.001
    specials = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0], dtype=torch.float64, device=device)
    out[sp] = specials[torch.randint(0, 4, (int(sp.sum()),), device=device, generator=g)]
    return out


def mixed_column_shard(first_vector: int, n_vectors: int, device, seed: int, out: torch.Tensor | None = None, exc_rate: float = 0.01) -> torch.Tensor:
    """vectors [first_vector, first_vector + n_vectors) of the (global) mixed column, block by block"""
    if out is None:
        out = torch.empty(n_vectors * VEC, dtype=torch.float64, device=device)
    per = MIX_BLOCK_RG * RG
    v = first_vector
    while v < first_vector + n_vectors:
        b = v // per
        blk = mixed_block(b, device, seed, exc_rate)
        lo = v - b * per
        hi = min(per, first_vector + n_vectors - b * per)
        out[(v - first_vector) * VEC:(v - first_vector + hi - lo) * VEC] = blk[lo * VEC:hi * VEC]
        v += hi - lo
        del blk
    return out


def synthetic_input(kind: str, n_vectors: int, device, seed: int):
    """device-side synthetic double columns for the single-GPU encode legs"""
    if kind == "rd":
        g = torch.Generator(device=device)
        g.manual_seed(seed)
        return torch.rand(n_vectors * VEC, dtype=torch.float64, device=device, generator=g)
    if kind == "uniform2":  # (tools only) two decimals in every rowgroup, 1 % full-precision values: a column whose rowgroups all pick the same (e, f)
        g = torch.Generator(device=device)
        g.manual_seed(seed)
        x = (torch.rand(n_vectors * VEC, dtype=torch.float64, device=device, generator=g) - 0.5) * 2e4
        out = torch.round(x * 100.0) / 100.0
        m = torch.rand(n_vectors * VEC, device=device, generator=g) < 0.01
        out[m] = x[m] * 3.141592653589793
        return out
    return mixed_column_shard(0, n_vectors, device, seed, exc_rate={"mixed": 0.01, "mixed_exc0": 0.0, "mixed_exc10": 0.10}[kind])


# ---- the reference's CPU path on this box's host cores (the only place bench.py touches oracle/) ---------------------------
def _cpu_runner():
    from oracle import pyoracle
    flags = open("/proc/cpuinfo").read() if os.path.exists("/proc/cpuinfo") else ""
    model = next((line.split(":", 1)[1].strip() for line in flags.splitlines() if line.startswith("model name")), "")
    if pyoracle.Reference.available():
        path = pyoracle.REF_AVX512_SO if ("avx512dq" in flags and os.path.exists(pyoracle.REF_AVX512_SO)) else pyoracle.REF_SO
        return pyoracle.Reference(path), "reference", model
    return pyoracle.Oracle(), "port", model


def physical_cores() -> int:
    """distinct (socket, core) pairs of the cores this process may use (SMT siblings counted once)"""
    try:
        allowed = os.sched_getaffinity(0)
        seen, cpu, phys = set(), None, None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k = k.strip()
            if k == "processor":
                cpu, phys = int(v), None
            elif k == "physical id":
                phys = int(v)
            elif k == "core id" and cpu in allowed:
                seen.add((phys, int(v)))
        return max(1, len(seen))
    except Exception:
        return max(1, len(os.sched_getaffinity(0)))


def host_scaling_note(all_cores: float, single: float, threads: int) -> dict:
    """When the box's host CPUs are shared or capped the all-cores figure is a property of the lease, not of the reference: say so, and give
    the per-thread figure times the physical cores next to it, LABELLED as an extrapolation (an upper bound: memory bandwidth does not scale
    with cores for ever — round 2's uncapped boxes measured 0.7-1.2 TB/s decode on these hosts).  "Scales" = all cores deliver at least a quarter
    of (one thread x physical cores): 8 x on 128 cores is not scaling."""
    cores = physical_cores()
    ratio = all_cores / max(single, 1e-9)
    if threads >= 16 and ratio < 0.25 * cores:
        return {"host_note": f"host capped: {threads} threads = {ratio:.1f} x one thread on {cores} physical cores", "extrapolated_all_cores_value": round(single * cores, 1),
                "extrapolated_from": "single thread x physical cores: an upper bound, not a measurement"}
    return {"host_note": f"host threads scale ({ratio:.0f} x one thread on {cores} physical cores)"}


def _run_threads(work, nthreads, prepare=None):
    """one host thread per unit of work, each PINNED to one of the cores this process may use (thread t -> core t mod cores).  prepare(t), if
    given, runs on the pinned thread in front of a barrier and outside the clock: threads use it to make (first-touch) their own buffers, so
    that the pages sit on the NUMA node of the core that streams them — with buffers touched by one thread the all-cores figure of a
    two-socket host is the inter-socket link's (measured: 27 GB/s instead of hundreds)."""
    res = [0.0] * nthreads
    ctxs = [None] * nthreads
    cpus = sorted(os.sched_getaffinity(0))
    gate = threading.Barrier(nthreads + 1)

    def pinned(t):
        if not os.environ.get("ALPGPU_BENCH_NO_PIN"):
            try:
                os.sched_setaffinity(0, {cpus[t % len(cpus)]})  # pid 0 = the calling thread
            except OSError:
                pass
        if prepare is not None:
            ctxs[t] = prepare(t)
        gate.wait()
        res[t] = work(t) if prepare is None else work(t, ctxs[t])
    ths = [threading.Thread(target=pinned, args=(t,)) for t in range(nthreads)]
    for th in ths:
        th.start()
    gate.wait()
    t0 = time.perf_counter()
    for th in ths:
        th.join()
    return time.perf_counter() - t0, res


def cpu_decode_baseline(ctx, col, vec, gpu_out, budget_s: float = 10.0):
    """Times the REFERENCE's CPU decode (falp + patch_exceptions; oracle/_ref, built from /root/reference in the build
    container) on this box's host cores and checks the GPU result against it bit for bit.  Sample: every 8th rowgroup of
    the benchmark column sampled at every 2nd rowgroup (2 and 53 are coprime: every bit width 1..53 is in it) = ~524 k vectors = 4 GiB of
    decoded doubles written and 1.8 GiB of packed words read per pass, against 2 x 256 MiB of L3 on the 2 x EPYC 9575F hosts: DRAM-resident
    (round 2's 1 GiB sample was partly cache-resident).  All-cores: the sample's vectors split over pinned threads, each writing its own
    part of one output buffer.  A second, cache-resident figure (the first 1024 vectors, every thread its own copy of the output) is
    reported next to it."""
    runner, kind, model = _cpu_runner()
    n_rg = (vec.size + RG - 1) // RG
    rgs = np.arange(0, n_rg, 2 if vec.size >= (1 << 19) else 1)
    idx = (rgs[:, None] * RG + np.arange(RG)[None, :]).reshape(-1)
    idx = idx[idx < vec.size]
    n = idx.size
    sv = vec[idx]
    # the sampled vectors' packed words at a fixed stride of 1024 words (what the reference's buffers look like)
    starts, sizes = sv["packed_off"].astype(np.int64), 128 * sv["bw"].astype(np.int64)
    packed = np.zeros((n, 1024), np.int64)
    p8 = packed.view(np.uint8).reshape(n, 8192)
    for r0 in range(0, n, RG):  # one device->host copy per sampled rowgroup (contiguous in the stream)
        r1 = min(n, r0 + RG)
        lo, hi = int(starts[r0]), int(starts[r1 - 1] + sizes[r1 - 1])
        chunk = col.packed[lo:hi].cpu().numpy()
        for v in range(r0, r1):
            o = int(starts[v]) - lo
            p8[v, : sizes[v]] = chunk[o:o + sizes[v]]
    bw, e, f, base = (np.ascontiguousarray(sv[k]) for k in ("bw", "e", "f", "base"))
    cnt = np.zeros(n, np.uint16)
    exc = np.zeros((n, 8), np.float64)
    pos = np.zeros((n, 8), np.uint16)
    threads = max(1, len(os.sched_getaffinity(0)))
    out = np.empty(n * 1024, np.float64)

    def sl(a, lo, hi):
        return a[lo:hi]

    def one_pass(nthreads, reps, local=False):
        bounds = np.linspace(0, n, nthreads + 1).astype(np.int64)

        def prepare(t):  # the thread's own copies of its inputs and its own output: pages on its core's NUMA node
            lo, hi = int(bounds[t]), int(bounds[t + 1])
            return (packed[lo:hi].copy(), np.zeros((hi - lo) * 1024, np.float64)) if hi > lo else None

        def work(t, mine=None):
            lo, hi = int(bounds[t]), int(bounds[t + 1])
            if hi <= lo:
                return 0.0
            pk, o = (mine[0], mine[1]) if mine is not None else (sl(packed, lo, hi), out[lo * 1024:hi * 1024])
            return runner.time_falp_column(pk, 1024, sl(bw, lo, hi), sl(e, lo, hi), sl(f, lo, hi), sl(base, lo, hi), sl(cnt, lo, hi),
                                           sl(exc, lo, hi), sl(pos, lo, hi), 8, hi - lo, o, reps)
        return _run_threads(work, nthreads, prepare if local else None)

    t1, _ = one_pass(1, 1)  # single thread, also page-faults the output and produces the values for the bit check
    got = gpu_out.view(-1, 1024)[torch.from_numpy(idx).to(gpu_out.device)].cpu().numpy()
    exact = bool(np.array_equal(got.view(np.uint64).reshape(-1), out.view(np.uint64)))
    widths = sorted(set(int(b) for b in bw))
    t1b, _ = one_pass(1, 1)
    single = n * 8192 / min(t1, t1b) / 1e9
    wall, _ = one_pass(threads, 1, local=True)
    reps = int(max(3, min(200, budget_s * 0.5 / max(wall, 1e-3))))
    wall, _ = one_pass(threads, reps, local=True)
    all_cores = n * 8192 * reps / wall / 1e9
    # cache-resident variant (what round 1 reported): 1024 vectors, private outputs
    m = min(1024, n)
    outs = [np.empty(m * 1024, np.float64) for _ in range(threads)]

    def cwork(t, reps_):
        return runner.time_falp_column(packed[:m], 1024, bw[:m], e[:m], f[:m], base[:m], cnt[:m], exc[:m], pos[:m], 8, m, outs[t], reps_)
    w1, _ = _run_threads(lambda t: cwork(t, 2), threads)
    creps = int(max(2, min(500, budget_s * 0.25 / max(w1 / 2, 1e-4))))
    wc, _ = _run_threads(lambda t: cwork(t, creps), threads)
    cache_all = threads * m * 8192 * creps / wc / 1e9
    return {
        "value": round(all_cores, 3), "unit": "GB/s decoded doubles", "cores": threads, "kind": kind,
        "sample": f"falp+patch_exceptions, every 2nd rowgroup of the same column: {n} vectors = {n * 8 // 1024} MiB decoded, widths {widths[0]}..{widths[-1]}, DRAM-resident, "
                  f"{reps} passes, {threads} pinned threads ({os.path.basename(runner.path)}; {model})",
        "single_thread_value": round(single, 3), "cache_resident_all_cores_value": round(cache_all, 3),
        "gpu_matches_cpu_bit_exact": exact, "bit_widths_checked": len(widths),
        **host_scaling_note(all_cores, single, threads),
    }


def cpu_encode_baseline(x_gpu: torch.Tensor, ecol, budget_s: float = 10.0):
    """The reference's CPU ENCODE (encoder::init per rowgroup, then encode + analyze_ffor + ffor per vector — the loop of
    publication/source_code/bench_speed/bench_alp_encode.cpp:19-37 and test/test_alp_sample.cpp:137-166) on a 4 GiB slice of the
    same mixed column (round 3's 1 GiB = 4 MiB per thread was cache-resident on the all-cores leg): single thread, and all host
    cores over disjoint whole-rowgroup ranges."""
    runner, kind, model = _cpu_runner()
    if kind != "reference":
        return {"kind": "port", "note": "oracle/_ref is not on this box; the C restatement has no encode timing loop"}
    n = min(524_200, x_gpu.numel() // VEC // RG * RG)  # whole rowgroups, 4 GiB: 16 MiB per thread on 256 threads = 2 GiB per socket against 256 MiB of L3
    col = x_gpu[: n * VEC].cpu().numpy()
    t1, sum_bw = runner.time_encode_column(col, n, 1)
    single = n * 8192 / t1 / 1e9
    # sum of the bit widths the reference chose == the GPU's over the same vectors (a cheap cross-check inside the bench)
    gv = ecol.vectors[: n * 32].cpu().numpy().view(capi.VECTOR_DTYPE)
    gpu_sum = int(gv["bw"].astype(np.int64).sum() + gv["lbw"].astype(np.int64).sum())
    threads = max(1, len(os.sched_getaffinity(0)))
    n_rg = n // RG
    threads = min(threads, n_rg)
    bounds = (np.linspace(0, n_rg, threads + 1).astype(np.int64)) * RG

    def prepare(t):  # the thread's own (NUMA-local) copy of its slice of the input
        lo, hi = int(bounds[t]), int(bounds[t + 1])
        return col[lo * VEC:hi * VEC].copy() if hi > lo else None

    def work(t, mine, reps):
        lo, hi = int(bounds[t]), int(bounds[t + 1])
        return runner.time_encode_column(mine, hi - lo, reps)[0] if hi > lo else 0.0
    wall, _ = _run_threads(lambda t, m: work(t, m, 1), threads, prepare)
    reps = int(max(1, min(100, budget_s * 0.6 / max(wall, 1e-3))))
    wall, _ = _run_threads(lambda t, m: work(t, m, reps), threads, prepare)
    allc = n * 8192 * reps / wall / 1e9
    per_thread_mib = n * 8 // 1024 // max(threads, 1)
    return {"value": round(allc, 3), "unit": "GB/s input doubles", "cores": threads, "kind": kind,
            "single_thread_value": round(single, 3),
            "sample": f"encoder::init + encode + analyze_ffor + ffor, first {n} vectors ({n * 8 // 1024} MiB) of the mixed column; {reps} passes, {threads} pinned threads x {per_thread_mib} MiB",
            "gpu_bit_width_sum_matches_cpu": bool(gpu_sum == sum_bw), **host_scaling_note(allc, single, threads)}


# ---- timed legs -------------------------------------------------------------------------------------------------------
class Clock:
    """W untimed warm-up steps, then exactly K steps bracketed by barrier + device sync on both sides; MAX over ranks."""

    def __init__(self, dist, dev, reduce_on=None):
        self.dist, self.dev = dist, dev
        self.reduce_on = reduce_on if reduce_on is not None else dev  # where the reductions' tensors live (the device, for RCCL)

    def barrier(self):
        torch.cuda.synchronize()
        if self.dist is not None:
            self.dist.barrier()
        torch.cuda.synchronize()

    def run(self, step, steps, warmup):
        for _ in range(warmup):
            step()
        self.barrier()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        t0 = time.perf_counter()
        for a, b in evs:
            a.record()
            step()
            b.record()
        self.barrier()
        elapsed = time.perf_counter() - t0
        kern_ms = float(np.mean([a.elapsed_time(b) for a, b in evs]))  # average step duration (HIP events, launch stream)
        self.local = (elapsed, kern_ms)  # THIS rank's clock, for its record in `ranks`; what is returned is the max over ranks
        if self.dist is not None:
            t = torch.tensor([elapsed, kern_ms], dtype=torch.float64, device=self.reduce_on)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            elapsed, kern_ms = float(t[0]), float(t[1])
        return elapsed, kern_ms

    def total(self, x: int) -> int:
        if self.dist is None:
            return x
        t = torch.tensor([x], dtype=torch.int64, device=self.reduce_on)
        self.dist.all_reduce(t)
        return int(t[0])


def gather_rank_records(dist, record: dict, world: int):
    """every rank's record on rank 0 (all ranks get the list): `ranks` of the N > 1 line — per-GPU rates and device identities of ONE shot,
    since the 8-GPU node is the driver's and its run cannot be repeated.  Objects travel through the process group's own collectives
    (RCCL on the GPU box, gloo in the CPU tests)."""
    if dist is None or world == 1:
        return [record]
    out = [None] * world
    dist.all_gather_object(out, record)
    return sorted(out, key=lambda r: r["rank"])


def device_identity(local_rank: int) -> dict:
    """what tells two GPUs of a node apart in a log: marketing name, PCI bus id, compute units, HBM size"""
    try:
        p = torch.cuda.get_device_properties(local_rank)
        ident = {"device": p.name, "cu_count": int(p.multi_processor_count), "hbm_GiB": round(p.total_memory / 2**30, 1), "local_rank": local_rank}
        for attr in ("pci_bus_id", "pci_device_id", "pci_domain_id"):
            if hasattr(p, attr):
                ident[attr] = int(getattr(p, attr))
        if hasattr(p, "uuid"):
            ident["uuid"] = str(p.uuid)
        return ident
    except Exception as exc:  # (dry run on a box without a GPU)
        return {"device": f"none ({type(exc).__name__})", "local_rank": local_rank}


def encode_alg_bytes(n, pb, eb):
    """read 8192 per vector once, write the packed words, the exception records and 13 B of metadata"""
    return n * 8192 + pb + eb + 13 * n


def traffic_from_profile(result, n):
    """roofline.traffic = HBM bytes per launch from the PMC counters — only from a profile taken with THIS library build"""
    pmc = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    try:
        t = json.load(open(pmc))
        if t.get("vectors") == n and t.get("kernel") == "k_decode_column" and t.get("lib_sha16") == lib_sha16():
            result["roofline"]["traffic"] = t["hbm_bytes_per_launch"]
            result["roofline"]["traffic_source"] = t.get("source")
        else:
            result["roofline"]["traffic_note"] = "profiles/hbm_traffic.json was taken with another build or size of the library: not quoted"
    except Exception:
        pass


def launch_plan(gpus: int, environ, visible_gpus: int):
    """What `python bench.py --gpus N` has to do before it measures anything:
      ("run",)          this process is the (or a) rank: --gpus 1 alone, or a rank of an external launcher whose WORLD_SIZE == N
      ("spawn", N)      --gpus N > 1 and no launcher around it: start N local ranks (one per GPU) and relay rank 0's line
      ("error", text)   the launcher's world size and --gpus disagree, or the box has fewer GPUs than ranks: exit non-zero, loudly
    (The driver launches N > 1 under torch.distributed.run itself; the self-launch is for everybody who types the N = 1 form with
    another N — which used to run the 1-GPU bench and print n_gpus 1.)"""
    if gpus < 1:
        return ("error", f"--gpus must be >= 1, got {gpus}")
    shared = bool(environ.get("ALPGPU_BENCH_TEST_SHARED_GPU")) or bool(environ.get("ALPGPU_BENCH_DRY_RUN"))
    world_env = environ.get("WORLD_SIZE")
    if world_env is None:
        if gpus == 1:
            return ("run",)
        if not shared and visible_gpus < gpus:
            return ("error", f"--gpus {gpus} but only {visible_gpus} GPU(s) are visible on this node: one rank per GPU, no oversubscription")
        return ("spawn", gpus)
    if int(world_env) != gpus:
        return ("error", f"launcher WORLD_SIZE={world_env} but --gpus {gpus}: they must agree (value and n_gpus are whole-job figures)")
    return ("run",)


def ensure_launcher(args):
    plan = launch_plan(args.gpus, os.environ, torch.cuda.device_count() if torch.cuda.is_available() else 0)
    if plan[0] == "run":
        return
    if plan[0] == "error":
        print(f"bench.py: {plan[1]}", file=sys.stderr, flush=True)
        sys.exit(2)
    import socket
    import subprocess
    with socket.socket() as s:  # a free rendezvous port on the loopback
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={plan[1]}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    sys.stdout.flush()
    sys.exit(subprocess.run(cmd, env=env).returncode)  # the ranks inherit stdout: rank 0's JSON line is the last line printed


def dry_run(args):
    """Test knob ALPGPU_BENCH_DRY_RUN (tests/test_bench_cpu.py): the launcher, rendezvous, barrier / max-over-ranks clock and rank 0's
    single line of the N > 1 path on a box WITHOUT a GPU (gloo on the CPU).  Nothing is decoded and the line says so."""
    import torch.distributed as dist
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo")
    total = int(2e9 / 8192) // RG * RG
    first, n = rowgroup_shard(total, rank, world)
    t0 = time.perf_counter()
    if world > 1:
        dist.barrier()
    t = torch.tensor([time.perf_counter() - t0, float(n)], dtype=torch.float64)
    cover = torch.tensor([n], dtype=torch.int64)
    seen = world
    ranks = [{"rank": rank, "first_vector": first, "vectors": n, **device_identity(int(os.environ.get("LOCAL_RANK", "0")))}]
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dist.all_reduce(cover)
        seen = dist.get_world_size()
        ranks = gather_rank_records(dist, ranks[0], world)
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"metric": "dry run: no GPU work", "value": 0.0, "unit": "GB/s", "n_gpus": world, "world_size_seen": seen, "steps": args.steps, "warmup": args.warmup,
                          "data": "none (ALPGPU_BENCH_DRY_RUN)", "config": {"column_vectors": total, "vectors_covered_by_the_shards": int(cover[0])},
                          "ranks": ranks}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10, help="untimed steps first (the first ~10 launches after an idle gap run 3-30 %% slower: tools/launch_trend.py)")
    ap.add_argument("--vectors", type=int, default=1 << 20, help="N = 1 headline: vectors of the configs[1] column (default 1 Mi = 8 GiB decoded)")
    ap.add_argument("--column-gb", type=float, default=None, help="configs[4]: size of the ONE column that is sharded over the ranks (default 100 when N > 1)")
    ap.add_argument("--full", action="store_true", help="N = 1: after the headline, also run the extras (per-bit-width sweeps, tuning, consumers, the encode "
                                                         "legs, real-data-shaped columns, ceilings, the float path) and the reference's CPU baselines")
    ap.add_argument("--no-extras", action="store_true", help="N = 1: skip the extras even with --full (a plain run never runs them)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write a fixed, seeded sample of the timed decode's output of the last step "
                                                                         "as DIR/*.npy (float64, at most 64 MB in all)")
    args = ap.parse_args()
    ensure_launcher(args)

    if os.environ.get("ALPGPU_BENCH_DRY_RUN"):
        return dry_run(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    # Test knob (tests/test_bench_gpu.py): all ranks share GPU 0 and talk over gloo, so that a ONE-GPU box can run the N > 1 code path
    # end to end (rank > 0 shards, the reductions, rank 0's line).  RCCL refuses two ranks on one device; nothing is measured this way.
    shared_gpu = bool(os.environ.get("ALPGPU_BENCH_TEST_SHARED_GPU"))
    if shared_gpu:
        local_rank = 0
    if world > 1 or os.environ.get("ALPGPU_BENCH_FORCE_DIST"):  # (the env var lets a 1-GPU box exercise the N > 1 code path)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if shared_gpu:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=torch.device(f"cuda:{local_rank}"))
    assert torch.cuda.is_available(), "bench.py needs an MI355X; alp_amd has no CPU fallback"
    torch.cuda.set_device(local_rank)
    dev = torch.device(f"cuda:{local_rank}")
    ctx = capi.Context(local_rank)  # launches on torch's current stream of this device
    clock = Clock(dist, dev, reduce_on=torch.device("cpu") if shared_gpu else dev)

    sharded = world > 1 or args.column_gb is not None
    if sharded:
        result = sharded_column_bench(args, ctx, clock, world, rank, local_rank, dev)
    else:
        result = single_gpu_bench(args, ctx, clock, local_rank, dev)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # RCCL writes its version banner through C stdio, which a pipe buffers until exit: flush it first so that the JSON line is the LAST line
        try:
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(fit_the_tail(result), flush=True)


def headline(value, world, args, elapsed, kern_ms, alg_bytes, decoded_bytes_rank, workload, scaling, extra_config):
    achieved = alg_bytes / (kern_ms * 1e-3) / 1e9
    cfg = {"workload": workload}
    cfg.update(extra_config)
    return {
        "metric": "ALP fused decode (falp + patch) throughput, decoded doubles",
        "value": round(value, 2), "unit": "GB/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": scaling,
        "vs_baseline": None, "dtype": "f64", "data": "synthetic", "config": cfg,
        "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": None,
                     "kernel": "k_decode_column", "kernel_ms": round(kern_ms, 4), "algorithmic_bytes_per_launch": alg_bytes},
        "per_gpu_value": round(decoded_bytes_rank * args.steps / elapsed / 1e9, 2),
    }


TAIL_BUDGET = 7700  # characters of stdout the driver keeps (8 KB), with a margin


def fit_the_tail(result: dict) -> str:
    """the JSON line, detail first and graded keys last (ordered_for_the_tail); should a line still outgrow the budget, per-item detail is moved
    out of it, least important first, and the line says which (`moved_out_for_size`; the full record goes to gpurun_out/bench_full.json)"""
    def dump(r):
        return json.dumps(ordered_for_the_tail(r), separators=(",", ":"))
    line = dump(result)
    if len(line) <= TAIL_BUDGET or "extras" not in result:
        return line
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        json.dump(result, open(os.path.join(ROOT, "gpurun_out", "bench_full.json"), "w"))
    except OSError:
        pass
    slim = json.loads(json.dumps(result))
    moved = []
    for path in (("decode_sweep_by_bit_width", "vpw"), ("decode_sweep_by_bit_width_2pct_exceptions", "vpw"), ("decode_tuning",), ("float_decode_sweep_2pct_exceptions", "frac"), ("float_decode_sweep", "frac"), ("decode_sweep_by_bit_width_2pct_exceptions", "frac"),
                 ("decode_sweep_by_bit_width", "frac"), ("decode_sum",), ("decode_bimodal",), ("ceilings",)):
        if len(line) <= TAIL_BUDGET:
            break
        node = slim["extras"]
        for k in path[:-1]:
            node = node.get(k, {})
        if path[-1] in node:
            del node[path[-1]]
            moved.append(".".join(path))
            slim["moved_out_for_size"] = moved
            line = dump(slim)
    return line


def ordered_for_the_tail(result: dict) -> dict:
    """The driver keeps the last 8 KB of stdout.  The N = 1 line is built to fit that whole (tests/test_bench_cpu.py checks the budget on a
    synthetic line); whatever a future key adds, the order puts the detail first and what is graded — every summary, the encode legs, the float
    path, cpu_baseline, roofline and the headline keys — LAST, so a cut tail loses per-width arrays, not floors (missing 4)."""
    first = [k for k in ("extras", "ranks") if k in result]
    last = [k for k in ("summaries", "encode", "scaling_summary", "cpu_baseline", "config", "roofline", "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                        "scaling", "vs_baseline", "dtype", "data", "per_gpu_value") if k in result]
    middle = [k for k in result if k not in first and k not in last]
    return {k: result[k] for k in first + middle + last}


# ---- configs[4]: one column sharded over the ranks -------------------------------------------------------------------------
def sharded_column_bench(args, ctx, clock, world, rank, local_rank, dev):
    gb = args.column_gb if args.column_gb is not None else 100.0
    total_vectors = int(gb * 1e9 / 8192) // RG * RG
    first, n = rowgroup_shard(total_vectors, rank, world)
    note = ""
    free, _ = torch.cuda.mem_get_info(dev)
    fit = int(free * 0.30 / 8192) // RG * RG  # input + output + the compressed column (and generator scratch) must fit
    if n > fit:  # (N = 1 with a 100 GB column, or a small GPU): the largest shard that fits, and say so
        note = f"; rank shards capped from {n} to {fit} vectors to fit {free / 2**30:.0f} GiB of free HBM"
        n = fit
    # ---- decode leg: the rank's shard of the configs[1] column
    col, vec, alg_bytes = build_decode_column(n, local_rank, seed=42, first_vector=first)
    out = torch.empty(n * VEC, dtype=torch.float64, device=dev)
    elapsed, kern_ms = clock.run(lambda: ctx.decode(col, out), args.steps, args.warmup)
    dump_outputs(args, out, n, "decoded_f64" if world == 1 else f"decoded_f64_rank{rank}")
    shape = ctx.decode_vectors_per_wg(col)
    total_decoded = clock.total(n * 8192)
    value = total_decoded * args.steps / elapsed / 1e9
    result = headline(value, world, args, elapsed, kern_ms, alg_bytes, n * 8192,
                      f"BASELINE.json configs[4]: one {total_vectors * 8192 / 1e9:.1f} GB column of doubles sharded by whole rowgroups over {world} GPU(s){note}; "
                      "value = decode of each rank's shard of the configs[1] column (bit widths 1-53 by global rowgroup, no exceptions); "
                      "encode of the rank's shard of the configs[2] mixed column in `encode`", "strong",
                      {"column_vectors": total_vectors, "vectors_per_gpu": n, "decoded_bytes_per_gpu": n * 8192,
                       "decode_launch_shape": f"{shape} vector(s) per 4-wave workgroup (chosen from the column's size hints)",
                       "parallelism": f"{world} whole-rowgroup shards, no collective on the data path"})
    del col
    d_local_elapsed, d_local_ms = clock.local
    # ---- encode leg: the rank's shard of the mixed column, generated on the device; round trip checked at full size
    x = mixed_column_shard(first, n, dev, seed=42)
    ecol = capi.DeviceColumn(n, local_rank, packed_capacity=int(n * 8192 * 0.60) + 4096, exc_capacity=int(n * 8192 * 0.15) + 4096)
    e_steps = max(3, min(args.steps, 10))
    e_elapsed, e_ms = clock.run(lambda: ctx.encode(x, ecol), e_steps, 2)
    e_local_elapsed, e_local_ms = clock.local
    pb, eb, ov = ctx.column_totals(ecol)
    d_elapsed, d_ms = clock.run(lambda: ctx.decode(ecol, out), e_steps, 3)
    rt = bool(torch.equal(out.view(torch.int64), x.view(torch.int64)))
    rt_all = clock.total(1 if rt else 0) == (world if clock.dist is not None else 1)
    total_in = clock.total(n * 8192)
    e_alg = encode_alg_bytes(n, pb, eb)
    result["encode"] = {
        "workload": "rowgroup init + vector encode of the rank's shard of the mixed column (round(x, d), d in {1,2,4} by rowgroup, 1 % full-precision "
                    "values, 0.1 % specials; the reference's search picks (14,12)-like pairs whose int64 product wraps for |v| >= 92233.72: 8-10 % exceptions)",
        "value": round(total_in * e_steps / e_elapsed / 1e9, 2), "unit": "GB/s input doubles (whole job)", "per_gpu_value": round(n * 8192 * e_steps / e_elapsed / 1e9, 2),
        "ms_per_step": round(e_elapsed / e_steps * 1e3, 4), "steps": e_steps,
        "roofline": {"bound": "hbm", "achieved": round(e_alg / e_ms / 1e6, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(e_alg / e_ms / 1e6 / HBM_PEAK_GBPS, 4),
                     "kernels": "k_rowgroup_init (persistent, beside) || k_encode_lean (+ gated recovery launches)", "ms": round(e_ms, 4), "algorithmic_bytes_per_step": e_alg},
        "compressed_bits_per_value": round((pb + eb + 32 * n) * 8 / (n * VEC), 2), "overflow": int(ov),
        "decode_of_the_encoded_shard": {"value": round(total_in * e_steps / d_elapsed / 1e9, 2), "unit": "GB/s decoded doubles (whole job)",
                                        "roofline_frac_algorithmic": round((n * 8192 + pb + eb + 13 * n) / d_ms / 1e6 / HBM_PEAK_GBPS, 4)},
        "roundtrip_bit_exact_all_ranks": bool(rt_all),
    }
    # every rank's own figures and device identity (configs[4]: "per-GPU and aggregate"): one 8-GPU shot returns all of them
    mine = {"rank": rank, **device_identity(local_rank), "first_vector": first, "vectors": n,
            "decode_ms": round(d_local_ms, 4), "decode_GBps": round(n * 8192 * args.steps / d_local_elapsed / 1e9, 2),
            "decode_roofline_frac": round(alg_bytes / d_local_ms / 1e6 / HBM_PEAK_GBPS, 4),
            "encode_ms": round(e_local_ms, 4), "encode_GBps": round(n * 8192 * e_steps / e_local_elapsed / 1e9, 2),
            "encode_roofline_frac": round(e_alg / e_local_ms / 1e6 / HBM_PEAK_GBPS, 4), "roundtrip_bit_exact": rt, "lib_sha16": lib_sha16()}
    result["ranks"] = gather_rank_records(clock.dist, mine, world)
    result["world_size_seen"] = clock.dist.get_world_size() if clock.dist is not None else 1
    result["per_gpu_value"] = round(float(np.mean([r["decode_GBps"] for r in result["ranks"]])), 2)
    result["per_gpu_value_min"] = round(float(np.min([r["decode_GBps"] for r in result["ranks"]])), 2)
    result["per_gpu_note"] = "per_gpu_value = mean of the ranks' own decode rates (their own clocks), _min the slowest; `value` = all shards / the max-over-ranks time"
    # one line that judges a single shot without opening `ranks`: the aggregate against N times the slowest rank's own rate (1.0 = the job runs at the slowest
    # GPU's pace with nothing lost to the barrier), and who that rank was; the same for the encode leg
    slow_d = min(result["ranks"], key=lambda r: r["decode_GBps"])
    slow_e = min(result["ranks"], key=lambda r: r["encode_GBps"])
    result["scaling_summary"] = {"decode_aggregate_over_n_x_slowest": round(result["value"] / max(world * slow_d["decode_GBps"], 1e-9), 4), "decode_slowest_rank": slow_d["rank"],
                                 "decode_per_gpu_min_max": [slow_d["decode_GBps"], max(r["decode_GBps"] for r in result["ranks"])],
                                 "encode_aggregate_over_n_x_slowest": round(result["encode"]["value"] / max(world * slow_e["encode_GBps"], 1e-9), 4), "encode_slowest_rank": slow_e["rank"],
                                 "encode_per_gpu_min_max": [slow_e["encode_GBps"], max(r["encode_GBps"] for r in result["ranks"])], "n_gpus": world,
                                 "distinct_devices": len({(r.get("pci_bus_id"), r.get("uuid"), r.get("local_rank")) for r in result["ranks"]})}
    return result


# ---- N = 1: configs[1] headline + extras -----------------------------------------------------------------------------------
# What the extras' short keys mean (the line has to fit the 8 KB the driver keeps; this is the legend; every `frac` is algorithmic bytes / time / 8 TB/s):
#   decode_sweep_by_bit_width[_2pct_exceptions]: one 1 Mi-vector column per bit width 1..53 (0 / 20 exceptions per vector): frac[i] and vpw[i] (vectors per decode
#       workgroup the launch rule chose) for width i + 1; summary = min / argmin / p10 / mean / max of frac; widths 1..read_ahead_upto ran with the read-ahead
#       kernel beside the decode (ALPGPU_OPT_DECODE_READ_AHEAD, the library's choice), no_read_ahead = the same columns with the option off.
#   decode_tuning: [frac at 1 vector per workgroup, at 2, auto, auto's choice] per case;  decode_bimodal: first half 6 bits + 20 exceptions, second half 44 bits: one / two
#       vectors per workgroup, the rule on the column's averages (`average`), and `auto` = after alpgpu_column_totals, region by region in `runs` launches (ALPGPU_OPT_DECODE_SEGMENTS).
#   decode_sum: per-vector SUM fused into the decode (k_sink_direct) — ms and frac; column_sum / count_range / ring (persistent LDS-ring kernel) / four_wave (staged kernel) fracs.
#   encode_<column>: ms / frac / GBps of alpgpu_encode_f64 (search beside the encode), front_ms (search in front), init_ms + vectors_ms (the two halves alone), bits (compressed
#       bits per value), dec_frac / dec_vpw (decode of that column), rt (GPU round trip bit-exact), unordered_ms / unordered_frac (ALPGPU_OPT_ENCODE_UNORDERED),
#       probe_ms (the kernel's loads + stores alone, same launch shape), probe_search_ms (the same with the persistent search beside it: the measured speed of light of
#       "these bytes + that search"), of_probe_search = probe_search_ms / ms.
#   ceilings: torch copy_ (read + write) and fill_ (write) of 8 GiB, read_only = the probe with no stores (8 GiB read in the encode's launch shape), as fractions of 8 TB/s.
#   float_path: enc_ms / enc_frac (ordered, the default), enc_unordered_* (ALPGPU_OPT_ENCODE_UNORDERED), dec_frac, sum_ms / sum_frac (k_sink_direct_f32), sum4_ms (staged kernel), bits, rt — per column kind, 1 Mi float vectors.
def single_gpu_bench(args, ctx, clock, local_rank, dev):
    n = args.vectors
    col, vec, alg_bytes = build_decode_column(n, local_rank, seed=42)
    out = torch.empty(n * VEC, dtype=torch.float64, device=dev)
    elapsed, kern_ms = clock.run(lambda: ctx.decode(col, out), args.steps, args.warmup)
    shape = ctx.decode_vectors_per_wg(col)
    value = n * 8192 * args.steps / elapsed / 1e9
    achieved = alg_bytes / (kern_ms * 1e-3) / 1e9
    result = headline(value, 1, args, elapsed, kern_ms, alg_bytes, n * 8192,
                      "BASELINE.json configs[1]: falp fused decode, synthetic decimal doubles, 1024-value vectors, bit widths 1-53 by rowgroup, no exceptions",
                      "weak", {"vectors_per_gpu": n, "decoded_bytes_per_gpu": n * 8192, "decode_vectors_per_wg": shape,
                               "parallelism": "1 shard; --gpus N shards ONE 100 GB column over N ranks (configs[4]); this value is that curve's N = 1 point (the rate does not depend on the shard's length)"})
    dump_outputs(args, out, n)
    traffic_from_profile(result, n)
    result["lib_sha16"] = lib_sha16()
    if not args.full or args.no_extras:
        return result

    def frac(bytes_, ms):
        return round(bytes_ / ms / 1e6 / HBM_PEAK_GBPS, 4)

    extras, summaries = {}, {}
    # per-bit-width sweep at the FULL column size (1 Mi vectors): smaller columns leave the packed stream resident in
    # the 256 MiB Infinity Cache across launches and overstate narrow widths by up to 1.8x (profiles/r01_time_one.txt)
    # EVERY width 1..53 (BASELINE.json configs[1] "bit-width sweep 1-53"), without exceptions and with 20 per vector (2 %); the summary prints
    # the minimum, the 10th percentile and the mean, so that the headline (the mean of a column that mixes the widths) cannot hide a floor
    def sweep_of(exc_per_vec):
        fr, vpw, ahead, plain = [], [], 0, []
        for bw in range(1, 54):
            c, _, ab = build_decode_column(n, local_rank, seed=7, bw_of_rowgroup=bw, exc_per_vec=exc_per_vec)
            med, _ = time_launches(lambda: ctx.decode(c, out), 7, 6)
            fr.append(round(ab / med / 1e6 / HBM_PEAK_GBPS, 3))
            vpw.append(ctx.decode_vectors_per_wg(c))
            if ctx.decode_reads_ahead(c):  # the library runs this width with the read-ahead: the same column with the option off, same run
                ahead = bw
                ctx.set_option(capi.OPT_DECODE_READ_AHEAD, 0)
                med, _ = time_launches(lambda: ctx.decode(c, out), 7, 6)
                plain.append(round(ab / med / 1e6 / HBM_PEAK_GBPS, 3))
                ctx.set_option(capi.OPT_DECODE_READ_AHEAD, -1)
            del c
        a = np.array(fr)
        summary = {"min": round(float(a.min()), 4), "argmin_bit_width": int(a.argmin()) + 1, "p10": round(float(np.percentile(a, 10)), 4),
                   "mean": round(float(a.mean()), 4), "max": round(float(a.max()), 4), "widths": 53, "exceptions_per_vector": exc_per_vec,
                   "read_ahead_upto": ahead}
        return {"frac": fr, "vpw": vpw, "no_read_ahead": plain, "summary": summary}
    for key, exc_ in (("decode_sweep_by_bit_width", 0), ("decode_sweep_by_bit_width_2pct_exceptions", 20)):
        extras[key] = sweep_of(exc_)
        summaries[key] = extras[key]["summary"]
    # 2 % exceptions (second run) and the 2-vectors-per-workgroup tuning option, which keeps twice the
    # bytes in flight: better for narrow widths and for vectors with exceptions, worse for wide ones
    tuning = {}
    for label, bw_, exc_ in (("bw16_exc0", 16, 0), ("bw16_exc20", 16, 20), ("bw28_exc10", 28, 10), ("bw8_exc0", 8, 0)):
        c, _, ab = build_decode_column(n, local_rank, seed=8, bw_of_rowgroup=bw_, exc_per_vec=exc_)
        row = []
        for vpw in (1, 2, 0):
            ctx.set_option(capi.OPT_DECODE_VECTORS_PER_WG, vpw)
            med, _ = time_launches(lambda: ctx.decode(c, out), 7, 10)
            row.append(frac(ab, med))
        tuning[label] = row + [ctx.decode_vectors_per_wg(c)]
        del c
    extras["decode_tuning"] = tuning
    # a column whose halves differ: the launch rule sees the AVERAGE width and exception count
    half = n // 2 // RG * RG
    bw_rg = np.where(np.arange(n) < half, 6, 44)
    c, _, ab = build_decode_column(n, local_rank, seed=9, bw_of_rowgroup=bw_rg, exc_per_vec=np.where(np.arange(n) < half, 20, 0))
    bim = {}
    for vpw in (1, 2, 0):
        ctx.set_option(capi.OPT_DECODE_VECTORS_PER_WG, vpw)
        med, _ = time_launches(lambda: ctx.decode(c, out), 7, 10)
        bim["average" if vpw == 0 else f"vpw{vpw}"] = frac(ab, med)  # (a hand-built column: no alpgpu_column_totals yet, the rule sees the two byte hints only)
    bim["average_vpw"] = ctx.decode_vectors_per_wg(c)
    ctx.column_totals(c)  # what a caller does after an encode: the context now knows the column's segments (ALPGPU_OPT_DECODE_SEGMENTS)
    med, _ = time_launches(lambda: ctx.decode(c, out), 7, 10)
    bim["auto"], bim["runs"] = frac(ab, med), ctx.decode_runs(c)
    extras["decode_bimodal"] = bim
    del c
    # decode fused into a SUM consumer: the 8 KiB per vector of decoded doubles never reach HBM
    sums = torch.empty(n, dtype=torch.float64, device=dev)
    med, _ = time_launches(lambda: ctx.decode_sum(col, sums), 7, 10)
    read_bytes = alg_bytes - n * 8192 + n * 8  # packed words + 13 B metadata read, 8 B written per vector
    ds = {"ms": round(med, 3), "frac": frac(read_bytes, med)}
    tot = torch.empty(1, dtype=torch.float64, device=dev)
    cmed, _ = time_launches(lambda: ctx.column_sum(col, tot), 7, 10)
    ds["column_sum"] = frac(read_bytes, cmed)
    cnts = torch.empty(n, dtype=torch.int32, device=dev)
    kmed, _ = time_launches(lambda: ctx.decode_count_range(col, -1.0, 1.0, cnts), 7, 10)
    ds["count_range"] = frac(read_bytes - 4 * n, kmed)
    for label, mode in (("ring", 1), ("four_wave", 3)):  # the persistent LDS-ring kernel and the staged four-wavefront kernel: measured, not the default
        ctx.set_option(capi.OPT_CONSUMER_PIPELINED, mode)
        pmed, _ = time_launches(lambda: ctx.decode_sum(col, sums), 7, 10)
        ds[label] = frac(read_bytes, pmed)
    ctx.set_option(capi.OPT_CONSUMER_PIPELINED, 0)
    for bw_ in (6, 16, 28):  # ... of columns WITH exceptions (20 per vector) next to the same widths without (round 6)
        for exc_ in (0, 20):
            c, _, ab = build_decode_column(n, local_rank, seed=7, bw_of_rowgroup=bw_, exc_per_vec=exc_)
            smed, _ = time_launches(lambda: ctx.decode_sum(c, sums), 7, 6)
            ds[f"bw{bw_}_exc{exc_}"] = [round(smed, 3), frac(ab - n * 8192 + n * 8, smed)]
            del c
    extras["decode_sum"] = ds
    del sums, tot, cnts
    # encode legs (BASELINE.json configs[2], configs[3]): rowgroup init + vector encode, input resident in HBM
    enc_cpu = None
    for kind, label in (("mixed", "encode_alp_mixed"), ("rd", "encode_alp_rd"), ("mixed_exc0", "encode_alp_mixed_exc0"), ("mixed_exc10", "encode_alp_mixed_exc10")):
        x = synthetic_input(kind, n, dev, seed=42)
        ecol = capi.DeviceColumn(n, local_rank)
        med, _ = time_launches(lambda: ctx.encode(x, ecol), 7, 3)  # rowgroup search BESIDE the vector encode (second stream; the default)
        row = {"ms": round(med, 3), "GBps": round(n * 8192 / med / 1e6, 1)}
        if label in ("encode_alp_mixed", "encode_alp_rd"):
            ctx.set_option(capi.OPT_ENCODE_ASYNC_INIT, 0)
            fmed, _ = time_launches(lambda: ctx.encode(x, ecol), 5, 2)  # ... in front of it (round 2's form)
            ctx.set_option(capi.OPT_ENCODE_ASYNC_INIT, 1)
            imed, _ = time_launches(lambda: ctx.rowgroup_init(x, ecol), 5, 1)
            vmed, _ = time_launches(lambda: ctx.encode_vectors(x, ecol), 5, 2)
            row.update(front_ms=round(fmed, 3), init_ms=round(imed, 3), vectors_ms=round(vmed, 3))
            ctx.set_option(capi.OPT_ENCODE_UNORDERED, 1)  # tiles reserve their bytes with one atomic add instead of the ordered look-back
            umed, _ = time_launches(lambda: ctx.encode(x, ecol), 7, 3)
            upb, ueb, _ = ctx.column_totals(ecol)
            ctx.decode(ecol, out)
            row.update(unordered_ms=round(umed, 3), unordered_rt=bool(torch.equal(out[: n * VEC].view(torch.int64), x.view(torch.int64))))
            ctx.set_option(capi.OPT_ENCODE_UNORDERED, 0)
        ctx.encode(x, ecol)
        pb, eb, ov = ctx.column_totals(ecol)
        e_alg = encode_alg_bytes(n, pb, eb)
        dmed, _ = time_launches(lambda: ctx.decode(ecol, out), 7, 10)
        row.update(frac=frac(e_alg, med), bits=round((pb + eb + 32 * n) * 8 / (n * VEC), 2), dec_frac=frac(e_alg, dmed), dec_vpw=ctx.decode_vectors_per_wg(ecol),
                   rt=bool(torch.equal(out[: n * VEC].view(torch.int64), x.view(torch.int64))))
        if "unordered_ms" in row:
            row["unordered_frac"] = frac(e_alg, row["unordered_ms"])
            assert (upb, ueb) == (pb, eb), "the unordered form writes the same number of bytes"
            # the kernel's loads and stores alone (same launch shape, no arithmetic), without and WITH the persistent search beside them: the
            # measured speed of light of this read/write mix next to the nominal peak (alpgpu_debug_traffic_probe[_with_search])
            wb = int(row["bits"] * VEC / 8) // 16 * 16
            pmed, _ = time_launches(lambda: ctx.traffic_probe(x, out, n, wb), 7, 5)
            smed, _ = time_launches(lambda: ctx.traffic_probe_with_search(x, out, n, wb, ecol), 7, 3)
            row.update(probe_ms=round(pmed, 3), probe_search_ms=round(smed, 3), of_probe_search=round(smed / med, 4))
            ctx.encode(x, ecol)  # (the probe's search overwrote the states)
        extras[label] = row
        if kind == "mixed":
            torch.cuda.synchronize()
            enc_cpu = cpu_encode_baseline(x, ecol)
            ro, _ = time_launches(lambda: ctx.traffic_probe(x, out, n, 0), 7, 5)  # read-only: 8 GiB in the encode's launch shape, 8 bytes per vector stored
        del x, ecol
    # ---- columns shaped like real data (round 6, VERDICT round 5 missing 2): rowgroup 0 (100 vectors) of five of the reference's datasets — the inputs of
    # tests/golden/rowgroup_samples.npz, k > 1 states, widths and exception counts that vary from vector to vector — repeated to ~1 Mi vectors on the device
    # (whole rowgroups, so the reference's decisions repeat: compressed size = repeats x the golden rowgroup's, checked), encoded (ordered and unordered) and
    # decoded from the encoder's own output after alpgpu_column_totals.  The reference publishes its numbers per dataset
    # (publication/results/i4i_4xlarge/x86_64_avx512bw_intrinsic_1024_uf1_falp.csv, alp_encode_pde.csv); these are the same shapes at GPU size.
    real = {}
    golden_path = os.path.join(ROOT, "tests", "golden", "rowgroup_samples.npz")
    if os.path.exists(golden_path):
        z = np.load(golden_path)
        reps = max(1, n // RG)
        nr = reps * RG
        for name in sorted({k.split("__")[0] for k in z.files}):
            bits_in = z[name + "__input_bits"][: RG * VEC]
            x = torch.from_numpy(bits_in.view(np.int64)).to(dev).view(torch.float64).repeat(reps)
            ecol = capi.DeviceColumn(nr, local_rank)
            med, _ = time_launches(lambda: ctx.encode(x, ecol), 5, 2)
            ctx.set_option(capi.OPT_ENCODE_UNORDERED, 1)
            umed, _ = time_launches(lambda: ctx.encode(x, ecol), 5, 2)
            ctx.set_option(capi.OPT_ENCODE_UNORDERED, 0)
            ctx.encode(x, ecol)
            pb, eb, ov = ctx.column_totals(ecol)
            rd = z[name + "__scheme"][:RG] == capi.SCHEME_ALP_RD
            want_pb = reps * int((128 * (z[name + "__bw"][:RG].astype(np.int64) + np.where(rd, z[name + "__lbw"][:RG], 0))).sum())
            want_eb = reps * int(((np.where(rd, 4, 10) * z[name + "__exc_cnt"][:RG].astype(np.int64) + 7) // 8 * 8).sum())
            e_alg = encode_alg_bytes(nr, pb, eb)
            dmed, _ = time_launches(lambda: ctx.decode(ecol, out), 7, 6)
            real[name.replace("_tw", "").replace("_f", "")] = {
                "bits": round((pb + eb + 32 * nr) * 8 / (nr * VEC), 2), "golden": bool((pb, eb) == (want_pb, want_eb)), "enc_frac": frac(e_alg, med), "enc_unordered_frac": frac(e_alg, umed),
                "dec_frac": frac(e_alg, dmed), "dec_runs": ctx.decode_runs(ecol), "rt": bool(torch.equal(out[: nr * VEC].view(torch.int64), x.view(torch.int64)))}
            del x, ecol
        extras["real_data"] = real
        summaries["real_data"] = {"columns": len(real), "enc_frac_min": min(r["enc_frac"] for r in real.values()), "dec_frac_min": min(r["dec_frac"] for r in real.values()),
                                  "dec_frac_mean": round(float(np.mean([r["dec_frac"] for r in real.values()])), 4), "all_golden": all(r["golden"] for r in real.values()),
                                  "all_rt": all(r["rt"] for r in real.values())}
    # ---- a column whose sizes the host does not know (round 6; ALPGPU_OPT_DECODE_UNHINTED): hinted / first unhinted decode (the plan made
    # on the device, every candidate launched) / later ones (sizes learned) / the option off (one vector per workgroup, no read-ahead: the old behaviour)
    unh = {}
    for label, bw_, exc_ in (("bw4", 4, 0), ("bw4_exc20", 4, 20), ("benchmark", None, 0)):
        c, _, ab = build_decode_column(n, local_rank, seed=7, bw_of_rowgroup=bw_, exc_per_vec=exc_)
        hmed, _ = time_launches(lambda: ctx.decode(c, out), 7, 6)
        hints = (int(c.c.packed_bytes_hint), int(c.c.exc_bytes_hint))
        c.c.packed_bytes_hint, c.c.exc_bytes_hint = 0, 0
        firsts = []
        for _ in range(5):
            ctx.forget(c)
            firsts.append(time_launches(lambda: ctx.decode(c, out), 1, 0)[0])
        lmed, _ = time_launches(lambda: ctx.decode(c, out), 7, 6)
        ctx.set_option(capi.OPT_DECODE_UNHINTED, 0)
        omed, _ = time_launches(lambda: ctx.decode(c, out), 7, 6)
        ctx.set_option(capi.OPT_DECODE_UNHINTED, 1)
        c.c.packed_bytes_hint, c.c.exc_bytes_hint = hints
        unh[label] = {"hinted": frac(ab, hmed), "first": frac(ab, float(np.median(firsts))), "later": frac(ab, lmed), "off": frac(ab, omed)}
        del c
    extras["decode_unhinted"] = unh
    summaries["decode_unhinted"] = {"later_over_hinted_min": round(min(r["later"] / r["hinted"] for r in unh.values()), 4), "first_over_hinted_min": round(min(r["first"] / r["hinted"] for r in unh.values()), 4)}
    # measured ceilings next to the nominal 8 TB/s: device-to-device copy (1 read + 1 write per byte) and fill of the 8 GiB
    # output buffer (torch's kernels), and the read-only stream above
    src = torch.empty_like(out)
    cmed, _ = time_launches(lambda: out.copy_(src), 7, 10)
    del src
    fmed, _ = time_launches(lambda: out.fill_(1.0), 7, 10)
    extras["ceilings"] = {"copy": round(2 * out.numel() * 8 / cmed / 1e6 / HBM_PEAK_GBPS, 4), "fill": round(out.numel() * 8 / fmed / 1e6 / HBM_PEAK_GBPS, 4),
                          "read_only": round(n * 8192 / ro / 1e6 / HBM_PEAK_GBPS, 4)}
    # single precision: alpgpu_encode_f32 / alpgpu_decode_f32 on 1 Mi float vectors (4 GiB decoded)
    fl = {}
    outf = out.view(torch.float32)[: n * VEC]
    for kind in ("decimal_mixed", "rd"):
        g = torch.Generator(device=dev)
        g.manual_seed(43)
        if kind == "rd":
            xf = torch.rand(n * VEC, dtype=torch.float32, device=dev, generator=g)
        else:  # one- and two-decimal values in +-1000 (cycling per rowgroup), 1 % full-precision values, 0.1 % specials
            xd = (torch.rand(n * VEC, dtype=torch.float64, device=dev, generator=g) - 0.5) * 2e3
            sc = torch.where((torch.arange((n + 99) // 100, device=dev) % 2 == 0), 10.0, 100.0).to(torch.float64).repeat_interleave(100 * VEC)[: n * VEC]
            xf = (torch.round(xd * sc) / sc).to(torch.float32)
            m = torch.rand(n * VEC, device=dev, generator=g) < 0.01
            xf[m] = (xd[m] * 3.141592653589793).to(torch.float32)
            sp = torch.rand(n * VEC, device=dev, generator=g) < 0.001
            specials = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0], dtype=torch.float32, device=dev)
            xf[sp] = specials[torch.randint(0, 4, (int(sp.sum()),), device=dev, generator=g)]
            del xd, sc, m, sp
        fcol = capi.DeviceColumn(n, local_rank, dtype="f32")
        ctx.set_option(capi.OPT_ENCODE_UNORDERED, 1)  # tiles reserve their bytes with one atomic add instead of the ordered look-back
        uemed, _ = time_launches(lambda: ctx.encode(xf, fcol), 3, 1)
        ctx.decode(fcol, outf)
        urt = bool(torch.equal(outf.view(torch.int32), xf.view(torch.int32)))
        ctx.set_option(capi.OPT_ENCODE_UNORDERED, 0)
        emed, _ = time_launches(lambda: ctx.encode(xf, fcol), 3, 1)
        pb, eb, ov = ctx.column_totals(fcol)
        dmed, _ = time_launches(lambda: ctx.decode(fcol, outf), 7, 10)
        rt = bool(torch.equal(outf.view(torch.int32), xf.view(torch.int32)))
        fsums = torch.empty(n, dtype=torch.float64, device=dev)
        smed, _ = time_launches(lambda: ctx.decode_sum(fcol, fsums), 7, 10)  # the default kernel (one wavefront per vector)
        ctx.set_option(capi.OPT_CONSUMER_PIPELINED, 3)
        s4, _ = time_launches(lambda: ctx.decode_sum(fcol, fsums), 7, 5)
        ctx.set_option(capi.OPT_CONSUMER_PIPELINED, 0)
        del fsums
        f_alg = n * (4096 + 13) + pb + eb
        fl[kind] = {"enc_ms": round(emed, 3), "enc_frac": frac(f_alg, emed), "enc_unordered_ms": round(uemed, 3), "enc_unordered_frac": frac(f_alg, uemed), "enc_unordered_rt": urt,
                    "bits": round((pb + eb + 32 * n) * 8 / (n * VEC), 2),
                    "dec_frac": frac(f_alg, dmed), "sum_ms": round(smed, 3), "sum_frac": frac(f_alg - n * 4096 + n * 8, smed), "sum4_ms": round(s4, 3), "rt": rt}
        del xf, fcol
    # float store decode by packed width (round 6): every width 1..32, without and with 20 exceptions per vector
    fsw = {}
    for key, exc_ in (("float_decode_sweep", 0), ("float_decode_sweep_2pct_exceptions", 20)):
        fr, ahead = [], 0
        for bw in range(1, 33):
            c, _, ab = build_decode_column(n, local_rank, seed=7, bw_of_rowgroup=bw, exc_per_vec=exc_, value_bytes=4)
            med, _ = time_launches(lambda: ctx.decode(c, outf), 7, 6)
            fr.append(round(ab / med / 1e6 / HBM_PEAK_GBPS, 3))
            ahead = bw if ctx.decode_reads_ahead(c) else ahead
            del c
        a = np.array(fr)
        fsw[key] = {"frac": fr, "summary": {"min": round(float(a.min()), 4), "argmin_bit_width": int(a.argmin()) + 1, "p10": round(float(np.percentile(a, 10)), 4), "mean": round(float(a.mean()), 4),
                                             "max": round(float(a.max()), 4), "widths": 32, "exceptions_per_vector": exc_, "read_ahead_upto": ahead}}
        extras[key] = fsw[key]
        summaries[key] = fsw[key]["summary"]
    extras["float_path"] = fl
    result["extras"] = extras
    result["summaries"] = summaries
    ctx.decode(col, out)
    torch.cuda.synchronize()
    result["cpu_baseline"] = cpu_decode_baseline(ctx, col, vec, out)
    if enc_cpu is not None:
        result["cpu_baseline"]["encode"] = enc_cpu
    return result


if __name__ == "__main__":
    main()
