"""Host replica of the records include/alpgpu.h defines for alpgpu_decode_minmax_masked_*, alpgpu_decode_group_minmax_* and
alpgpu_group_minmax_totals_* (no GPU, numpy only): shared by tests/test_minmax_cpu.py, which pins it on a hand-made case, and
tests/test_minmax_gpu.py, which holds the kernels to it bit for bit.  It never compares floats: a record is the minimum / maximum of the
order-preserving integer key of the value bits (b if b >= 0 else b ^ INT_MAX, as tests/test_zone_gpu.py's key) over the selected values that are
not NaN, mapped back to bits, so that -0.0 lies below +0.0, +-inf are ordinary values and the empty record is {+inf, -inf}."""
import numpy as np


def _int(dtype):
    return np.int64 if np.dtype(dtype) == np.float64 else np.int32


def order_key(b):
    """value bits (int64 / int32) -> the key whose ascending order is the values' order; its own inverse"""
    return np.where(b >= 0, b, b ^ np.iinfo(b.dtype).max)


def _reduce(x, take):
    """[..., n] values and a bool array of the same shape -> [..., 2] values {min, max} over the taken entries that are not NaN"""
    it = _int(x.dtype)
    top, bottom = np.iinfo(it).max, np.iinfo(it).min
    k = order_key(np.ascontiguousarray(x).view(it))
    use = take & ~np.isnan(x)
    kmin = np.where(use, k, top).min(axis=-1, initial=top)
    kmax = np.where(use, k, bottom).max(axis=-1, initial=bottom)
    inf = np.array([np.inf, -np.inf], dtype=x.dtype).view(it)
    none = ~use.any(axis=-1)
    out = np.stack([np.where(none, inf[0], order_key(kmin)), np.where(none, inf[1], order_key(kmax))], axis=-1).astype(it)
    return out.view(x.dtype)


def host_minmax_masked(values, bits):
    """(records [n, 2] of the values' type, counts [n] int64): values, bits [n, 1024]; a selected NaN is counted and ignored"""
    values = np.asarray(values).reshape(-1, 1024)
    bits = np.asarray(bits, dtype=bool).reshape(-1, 1024)
    return _reduce(values, bits), bits.sum(axis=1).astype(np.int64)


def host_group_minmax(val, key, bits, lo, hi):
    """(records [G, n, 2], counts [G, n] int64).  Group g selects a value if its bit is set and lo[g] <= key <= hi[g] there (IEEE comparisons in
    the key's own type: false with a NaN on either side, -0.0 == 0.0)"""
    val, key = np.asarray(val).reshape(-1, 1024), np.asarray(key).reshape(-1, 1024)
    bits = np.asarray(bits, dtype=bool).reshape(-1, 1024)
    zones = np.empty((len(lo),) + val.shape[:1] + (2,), dtype=val.dtype)
    counts = np.empty((len(lo), val.shape[0]), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for g in range(len(lo)):
            sel = bits & (key >= key.dtype.type(lo[g])) & (key <= key.dtype.type(hi[g]))
            zones[g], counts[g] = host_minmax_masked(val, sel)
    return zones, counts


def host_minmax_totals(zones):
    """[G, n, 2] records -> [G, 2]: the minimum of the minima and the maximum of the maxima, a NaN in a record ignored; {+inf, -inf} for n == 0"""
    zones = np.asarray(zones)
    every = np.ones(zones.shape[:2], dtype=bool)
    return np.stack([_reduce(zones[:, :, 0], every)[:, 0], _reduce(zones[:, :, 1], every)[:, 1]], axis=-1)
