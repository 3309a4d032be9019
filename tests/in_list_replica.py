"""Host replica of set membership (include/alpgpu.h, "set membership": alpgpu_select_in_mask_*): member(x) is a lower bound into the list sorted as
numpy.sort sorts (ascending by <, NaNs last) followed by one ==, which is what the kernel computes; q(r) = first <= r < first + n and
(member(x_r) != negate).  numpy only."""
import numpy as np


def host_member(values, lst):
    """bool array, shaped as values: some element of lst == the value, under C's == (-0.0 == 0.0; a NaN, value or element, never)"""
    values = np.asarray(values)
    s = np.sort(np.asarray(lst, dtype=values.dtype))  # (stable about nothing that matters: -0.0 and +0.0 in either order, NaNs last)
    if s.size == 0:
        return np.zeros(values.shape, dtype=bool)
    at = np.searchsorted(s, values, side="left")  # the first element that is not < the value (numpy orders NaN last here too)
    with np.errstate(invalid="ignore"):
        return (at < s.size) & (s[np.minimum(at, s.size - 1)] == values)


def host_in_mask(values, lst, first=0, n=None, negate=False):
    """q over every value index of the column (values: whole vectors, flat)"""
    values = np.asarray(values).reshape(-1)
    n = values.size - first if n is None else n
    r = np.arange(values.size)
    return (r >= first) & (r < first + n) & (host_member(values, lst) != bool(negate))


def pack_bits(q):
    """bool array of whole vectors -> the bitmap as uint64 words: bit r & 63 of word r >> 6 = q[r]"""
    return np.packbits(np.asarray(q, dtype=bool).reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)
