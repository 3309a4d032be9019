"""Host replica of top-k (include/alpgpu.h, "top-k": alpgpu_top_k_*): the definition, by numpy on integer views.

okey(x) = bits ^ (sign ? all-ones : sign-bit) is an unsigned monotone bijection on the bits of the values that are no NaNs: -inf < ... < -0.0 < +0.0
< ... < +inf.  The result is the selected values that are no NaNs, sorted by descending okey (largest) or ascending okey (smallest), equal bit
patterns by ascending index, cut to the first k.  Nothing here comes from the code under test."""
import numpy as np


def uint_view(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64 if x.dtype == np.float64 else np.uint32)


def okey(x):
    """the order key of every value of a float64 / float32 array, as an unsigned integer array of the same width"""
    b = uint_view(x)
    width = 8 * b.dtype.itemsize
    sign = b.dtype.type(1) << b.dtype.type(width - 1)
    ones = b.dtype.type(np.iinfo(b.dtype).max)
    return b ^ np.where(b & sign != 0, ones, sign).astype(b.dtype)


def is_nan_bits(x):
    """NaN by the bits, quiet or signalling (what np.isnan says; spelled out because the definition is about bits)"""
    b = uint_view(x)
    width = 8 * b.dtype.itemsize
    mant = 52 if width == 64 else 23
    inf = b.dtype.type(((1 << (width - 1 - mant)) - 1) << mant)
    return (b & b.dtype.type((1 << (width - 1)) - 1)) > inf


def host_top_k(x, bits, k, largest=True):
    """x: the column's decoded values, flat; bits: bool of the same length, the selection.  Returns (values, indices): the first k of the selected
    values that are no NaNs in the order of the definition; values carry the bits of x"""
    x = np.ascontiguousarray(x).reshape(-1)
    idx = np.nonzero(np.asarray(bits, bool).reshape(-1) & ~is_nan_bits(x))[0].astype(np.int64)
    key = okey(x[idx])
    if largest:
        key = ~key
    if 0 < k < idx.size // 4:
        # only to keep long columns quick: an element whose key lies behind the k-th smallest key cannot be among the first k of the order below, so
        # it is dropped before the sort (every element that ties with the k-th key stays)
        near = key <= np.partition(key, k - 1)[k - 1]
        idx, key = idx[near], key[near]
    order = np.lexsort((idx, key))[:k]  # ascending (key, idx): for largest the inverted key, so descending okey
    return x[idx[order]], idx[order]


def unpack_mask(words):
    """a bitmap's int64 / uint64 words on the host -> flat bool, bit r & 63 of word r >> 6 = value index r"""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little").astype(bool)
