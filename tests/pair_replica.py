"""Host replica of the summation order include/alpgpu.h documents for alpgpu_decode_dot_masked_* (no GPU, numpy only): shared by
tests/test_pair_cpu.py, which pins it on a hand-made case, and tests/test_pair_gpu.py, which holds the kernel to it bit for bit."""
import numpy as np


def pairwise_tree(p):
    """[n, 2^k] -> [n]: adjacent pairs, pairs of pairs, ..."""
    while p.shape[1] > 1:
        p = p[:, 0::2] + p[:, 1::2]
    return p[:, 0]


def host_dots_masked(a, b, bits):
    """lane L of 64 starts from +0.0 and for m = 0..15, if bit 64 m + L is set, forms t = a * b rounded once to double (floats widened first) and
    then acc = acc + t rounded once, else does nothing; adjacent-lane tree over the 64 partials.  numpy multiplies and adds in separate
    operations: nothing here can fuse.  a, b, bits: [n, 1024]"""
    t = np.empty((a.reshape(-1, 1024).shape[0], 16, 64))
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        np.multiply(a.astype(np.float64).reshape(-1, 16, 64), b.astype(np.float64).reshape(-1, 16, 64), out=t)
        sel = bits.reshape(-1, 16, 64)
        p = np.zeros((t.shape[0], 64))
        for m in range(16):
            p = np.where(sel[:, m], p + t[:, m], p)
        return pairwise_tree(p)
