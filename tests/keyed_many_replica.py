"""Host replica of the records include/alpgpu.h defines for alpgpu_decode_keyed_minmax_many_* (no GPU, numpy only): keyed_minmax_replica.host_keyed_minmax
without the 1024-key bound of keyed_replica.match_keys.  The match is its own searchsorted(side="left"), clamp and C's ==; the records go through
minmax_replica.order_key (the integer order key of the value bits, no float comparison).  tests/test_keyed_minmax_many_cpu.py holds it to
host_keyed_minmax bit for bit up to 1024 keys and pins it on a hand-made case beyond; the GPU suite holds the kernels to it.  It is fed the values that
were encoded, never a result of the call under test."""
import numpy as np

from minmax_replica import _int, order_key

KEYS_MAX = 1 << 20


def match_many(key, keys):
    """(idx, matched) per row: idx = the first position with keys[idx] == key under C's == (keys sorted as numpy.sort sorts, NaNs last; -0.0 == +0.0;
    a NaN on either side never matches), clamped to the list"""
    keys = np.asarray(keys)
    assert keys.dtype == key.dtype and keys.ndim == 1 and 1 <= keys.size <= KEYS_MAX
    at = np.minimum(np.searchsorted(keys, key, side="left"), keys.size - 1)
    with np.errstate(invalid="ignore"):
        matched = keys[at] == key
    return at, matched


def host_keyed_minmax_many(val, key, bits, keys):
    """(records [K, 2] of val's type, counts [K + 1] int64).  val, key: n * 1024 values of one type; bits: n * 1024 bools; keys: K sorted keys,
    1 <= K <= 2^20.  Record i = {min, max} over the selected rows of key i that are no NaNs, {+inf, -inf} without one; counts[i] = the selected
    rows of key i, NaN values included; counts[K] = the selected rows without a key."""
    val, key = np.ascontiguousarray(val).reshape(-1), np.ascontiguousarray(key).reshape(-1)
    keys = np.asarray(keys)
    K = keys.size
    b = np.asarray(bits, bool).reshape(-1)
    it = _int(val.dtype)
    counts = np.zeros(K + 1, np.int64)
    kmin, kmax = np.full(K, np.iinfo(it).max, it), np.full(K, np.iinfo(it).min, it)
    if val.size:
        rows = np.flatnonzero(b)  # the selected rows alone are searched: a sparse bitmap keeps a long column quick
        idx, matched = match_many(key[rows], keys)
        counts[K] = int((~matched).sum())
        rows, idx = rows[matched], idx[matched]
        counts[:K] = np.bincount(idx, minlength=K)
        number = ~np.isnan(val[rows])
        rows, idx = rows[number], idx[number]
        if rows.size:
            k = order_key(val[rows].view(it))
            np.minimum.at(kmin, idx, k)
            np.maximum.at(kmax, idx, k)
    inf = np.array([np.inf, -np.inf], dtype=val.dtype).view(it)
    none = kmin > kmax  # (top, bottom): no number arrived
    out = np.stack([np.where(none, inf[0], order_key(kmin)), np.where(none, inf[1], order_key(kmax))], axis=-1).astype(it)
    return out.view(val.dtype), counts
