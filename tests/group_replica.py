"""Host replica of the order include/alpgpu.h documents for alpgpu_decode_group_sum_* and alpgpu_group_totals (no GPU, numpy only): shared by
tests/test_group_cpu.py, which pins it on a hand-made case, and tests/test_group_gpu.py, which holds the kernels to it bit for bit."""
import numpy as np


def adjacent_tree(p):
    """[..., 2^k] -> [...]: adjacent pairs, pairs of pairs, ..."""
    while p.shape[-1] > 1:
        p = p[..., 0::2] + p[..., 1::2]
    return p[..., 0]


def host_group_sums(val, key, bits, lo, hi):
    """(sums [G, n] float64, counts [G, n] int64).  Group g: lane L of 64 starts from +0.0 and for m = 0..15 adds value 64 m + L of val (widened to
    double) if its bit is set and lo[g] <= key <= hi[g] there (IEEE comparisons in the key's own type: false with a NaN on either side,
    -0.0 == 0.0), else does nothing; adjacent-lane tree over the 64 partials.  val, key, bits: [n, 1024]; lo, hi: G bounds"""
    x = val.astype(np.float64).reshape(-1, 16, 64)
    k = key.reshape(-1, 16, 64)
    b = bits.reshape(-1, 16, 64)
    n = x.shape[0]
    sums, counts = np.empty((len(lo), n)), np.empty((len(lo), n), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(len(lo)):
            lo_g, hi_g = key.dtype.type(lo[g]), key.dtype.type(hi[g])
            p = np.zeros((n, 64))
            c = np.zeros(n, dtype=np.int64)
            for m in range(16):
                q = b[:, m] & (k[:, m] >= lo_g) & (k[:, m] <= hi_g)
                p = np.where(q, p + x[:, m], p)
                c += q.sum(axis=1)
            sums[g], counts[g] = adjacent_tree(p), c
    return sums, counts


def host_group_totals(sums, counts=None):
    """(totals [G] float64, counts [G] int64 or None): every row by levels of 1024-element blocks padded with +0.0, a block as
    (e0 + e1) + (e2 + e3) per thread of 256, the adjacent tree over a wavefront's 64 threads and (s0 + s1) + (s2 + s3) over the four wavefronts
    — which is the adjacent tree over the 1024; the counts as exact integers"""
    s = np.asarray(sums, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        while True:
            blocks = (s.shape[1] + 1023) // 1024
            pad = np.zeros((s.shape[0], max(blocks, 1) * 1024))
            pad[:, : s.shape[1]] = s
            s = adjacent_tree(pad.reshape(s.shape[0], max(blocks, 1), 1024))
            if blocks <= 1:
                break
    return s[:, 0], None if counts is None else np.asarray(counts).astype(np.int64).sum(axis=1)
