"""Host replica of the join probe (include/alpgpu.h, "join probe": alpgpu_join_probe_*): for each value x, lb = the number of keys < x and ub = the
number of keys <= x, by numpy.searchsorted "left" / "right" on the NaN-free prefix of the keys sorted as numpy.sort sorts (a NaN key is never < or
<= anything, so the NaNs at the end add to neither); span = ub - lb, pos = lb (or rows[lb]) where span > 0 and NO_MATCH elsewhere.  A NaN value has
lb = ub = 0 by the definition (no key is < or <= a NaN); numpy orders it behind everything, so it is settled apart.
The rows are those of the bitmap's set bits, ascending.  numpy only; integers compare as integers."""
import numpy as np

NO_MATCH = -1


def host_bounds(values, sorted_keys):
    """(lb, ub) as int64 arrays shaped as values; sorted_keys: sorted as numpy.sort sorts, NaNs (if any) last"""
    values = np.asarray(values)
    keys = np.asarray(sorted_keys, dtype=values.dtype)
    real = keys[: keys.size - int(np.isnan(keys).sum())]  # the NaN-free prefix
    lb = np.searchsorted(real, values, side="left").astype(np.int64)
    ub = np.searchsorted(real, values, side="right").astype(np.int64)
    nan = np.isnan(values)
    lb[nan] = 0
    ub[nan] = 0
    return lb, ub


def host_probe(values, sorted_keys, rows=None):
    """(pos int64, span uint32) for every value"""
    lb, ub = host_bounds(values, sorted_keys)
    span = ub - lb
    hit = span > 0
    payload = lb
    if rows is not None and len(rows) > 0:
        payload = np.asarray(rows, dtype=np.int64)[np.minimum(lb, len(rows) - 1)]  # (read only where hit: lb < the number of keys there)
    pos = np.where(hit, payload, NO_MATCH).astype(np.int64)
    return pos, span.astype(np.uint32)


def unpack_bits(words):
    """the bitmap's uint64 (or int64) words -> bool per value index: bit r & 63 of word r >> 6"""
    w = np.ascontiguousarray(np.asarray(words)).view("<u8").reshape(-1, 1)
    return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little").reshape(-1).astype(bool)


def host_join(values, sorted_keys, mask_words=None, rows=None):
    """(idx, pos, span) of the whole call without a capacity: one row per set bit (mask_words None: every index), ascending"""
    values = np.asarray(values).reshape(-1)
    idx = np.arange(values.size, dtype=np.int64) if mask_words is None else np.nonzero(unpack_bits(mask_words))[0].astype(np.int64)
    pos, span = host_probe(values[idx], sorted_keys, rows)
    return idx, pos, span
