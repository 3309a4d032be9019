"""Host replica of the records include/alpgpu.h defines for alpgpu_decode_keyed_minmax_* (no GPU, numpy only): shared by
tests/test_keyed_minmax_cpu.py, which pins it on a hand-made case and holds it to host_group_minmax + host_minmax_totals with point groups, and the GPU
suites, which hold the kernels to it bit for bit.  It is built from keyed_replica.match_keys (the first equal key, C's ==) and what
minmax_replica._reduce reduces (order_key: the integer order key of the value bits, no float comparison; scattered per key here where _reduce goes
along an axis, and tests/test_keyed_minmax_cpu.py holds the two to each other key by key), and is fed the oracle's or the store decode's values,
never a result of the call under test."""
import numpy as np

from keyed_replica import match_keys
from minmax_replica import _int, order_key


def host_keyed_minmax(val, key, bits, keys):
    """(records [K, 2] of val's type, counts [K + 1] int64).  val, key: n * 1024 values of one type; bits: n * 1024 bools; keys: K sorted keys.
    Record i = {min, max} over the selected rows of key i that are no NaNs, {+inf, -inf} without one; counts[i] = the selected rows of key i, NaN
    values included; counts[K] = the selected rows without a key."""
    val, key = np.ascontiguousarray(val).reshape(-1), np.ascontiguousarray(key).reshape(-1)
    keys = np.asarray(keys)
    K = keys.size
    b = np.asarray(bits, bool).reshape(-1)
    it = _int(val.dtype)
    top, bottom = np.iinfo(it).max, np.iinfo(it).min
    counts = np.zeros(K + 1, np.int64)
    kmin, kmax = np.full(K, top, it), np.full(K, bottom, it)
    if val.size:
        idx, matched = match_keys(key, keys)
        counts[K] = int((b & ~matched).sum())
        rows = np.flatnonzero(b & matched)
        counts[:K] = np.bincount(idx[rows], minlength=K)
        rows = rows[~np.isnan(val[rows])]
        if rows.size:
            by_key = np.argsort(idx[rows], kind="stable")
            k, ids = order_key(val[rows].view(it))[by_key], idx[rows][by_key]
            start = np.flatnonzero(np.concatenate([[True], ids[1:] != ids[:-1]]))  # one run of rows per key that has a number
            kmin[ids[start]] = np.minimum.reduceat(k, start)
            kmax[ids[start]] = np.maximum.reduceat(k, start)
    inf = np.array([np.inf, -np.inf], dtype=val.dtype).view(it)
    none = kmin > kmax  # (top, bottom): no number arrived
    out = np.stack([np.where(none, inf[0], order_key(kmin)), np.where(none, inf[1], order_key(kmax))], axis=-1).astype(it)
    return out.view(val.dtype), counts


def same_records(a, b):
    """bit for bit (a record never holds a NaN)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
