#!/usr/bin/env python3
"""probe_graph_memset.py: does a hipMemsetAsync node in a captured graph still write its value at LATER replays?

Captures one graph of alpgpu_memset (a bare hipMemsetAsync on the context's stream) over twelve buffers of 8 bytes to 514 KiB, value 0, and replays it
three times.  Before each replay every buffer is filled with 5; between the first and the second replay the process does other work on the device (an
encode, a decode, a torch.sort).  Prints, per replay and size, the words that are not zero and whether the words behind the buffer kept their 5.

What was observed when alpgpu_histogram_* was written (one MI355X, torch's graph capture; DESIGN.md, "Histograms"): replay 0 all zero; replays 1 and 2
non-zero words for 24, 64, 536, 1024, 32768, 32776, 32784 and 526336 bytes (values like 0x7ffc..., heap addresses, small integers), zero for 8, 16, 544
and 4096; nothing behind a buffer touched.  That is why the histogram call zeroes its counts with a kernel.  The probe says nothing about WHY: the
runtime, torch's capture or the combination.  Exit status 1 if any replay left a non-zero word.
  python3 tools/probe_graph_memset.py"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import datagen  # noqa: E402
from alp_amd import capi  # noqa: E402

SIZES = [8, 16, 24, 64, 536, 544, 1024, 4096, 32768, 32776, 32784, 526336]


def main():
    ctx = capi.Context(0)
    lib = capi.lib
    lib.alpgpu_memset.restype = ctypes.c_int
    lib.alpgpu_memset.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    side = torch.cuda.Stream()
    bufs = [torch.full((s // 8 + 4,), 5, dtype=torch.int64, device="cuda:0") for s in SIZES]

    def calls():
        for s, b in zip(SIZES, bufs):
            assert lib.alpgpu_memset(ctx.h, ctypes.c_void_p(b.data_ptr()), 0, s) == 0

    with torch.cuda.stream(side):
        calls()  # warm-up on the capture stream
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            calls()
    x = torch.from_numpy(datagen.mixed_column(230, seed=81)).cuda()
    bad_total = 0
    for rep in range(3):
        if rep == 1:  # other work between the replays
            col = ctx.encode(x)
            ctx.decode(col)
            torch.sort(torch.rand(1 << 20, device="cuda:0"))
        torch.cuda.synchronize()
        for b in bufs:
            b.fill_(5)
        g.replay()
        torch.cuda.synchronize()
        for s, b in zip(SIZES, bufs):
            w = s // 8
            bad = int((b[:w] != 0).sum())
            bad_total += bad
            first = hex(int(b[:w][b[:w] != 0][0]) & (2**64 - 1)) if bad else "-"
            print(f"replay {rep}: memset of {s:6d} bytes: {bad:5d} of {w:5d} words not zero, first {first}; words behind untouched: {bool((b[w:] == 5).all())}")
    return 1 if bad_total else 0


if __name__ == "__main__":
    sys.exit(main())
