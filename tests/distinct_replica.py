"""The host replica of the distinct values (include/alpgpu.h, "distinct values": alpgpu_distinct_*), by numpy alone: select, drop the NaNs by their
bits, make every zero +0.0, numpy.unique with counts.  It knows nothing of the library; the tests feed it the store decode (or the oracle's decode)
and compare bytes and integers."""
import numpy as np


def is_nan_bits(x):
    """NaN by the bits, quiet or signalling: exponent all ones and a mantissa that is not zero"""
    x = np.ascontiguousarray(x)
    if x.dtype == np.float64:
        b = x.view(np.uint64)
        return (b & np.uint64(0x7FFFFFFFFFFFFFFF)) > np.uint64(0x7FF0000000000000)
    assert x.dtype == np.float32
    b = x.view(np.uint32)
    return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def host_distinct(x, selected=None):
    """(values, counts, n_nan, n_numbers): the distinct values of the selected x that are no NaNs, ascending (-inf and +inf ordinary, -0.0 and +0.0 one
    value, +0.0), of x's dtype; how often each occurs, uint64; the selected NaNs; the selected values that are no NaNs.  selected: a bool array over
    x, None: all of x."""
    x = np.ascontiguousarray(x)
    sel = np.ones(x.size, bool) if selected is None else np.asarray(selected, bool)
    xs = x.reshape(-1)[sel.reshape(-1)]
    nan = is_nan_bits(xs)
    numbers = xs[~nan].copy()
    numbers[numbers == 0] = 0  # both zeros become +0.0
    values, counts = np.unique(numbers, return_counts=True)
    assert values.dtype == x.dtype and not np.signbit(values[values == 0]).any()
    return values, counts.astype(np.uint64), int(nan.sum()), int(numbers.size)


def unpack_mask(mask_words, n_values):
    """a selection bitmap (uint64 / int64 words, bit r & 63 of word r >> 6 = value index r) as a bool array over the first n_values indices"""
    w = np.ascontiguousarray(mask_words).view(np.uint64)
    bits = (w[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    return bits.reshape(-1)[:n_values].astype(bool)
