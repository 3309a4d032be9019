"""Host replica of the sums include/alpgpu.h defines for alpgpu_decode_keyed_exact_sum_* (no GPU; numpy and Python integers): the match is
keyed_many_replica.match_many, a key's sum is formed as a Python integer, sum of int(x * 2^1074) over its selected rows, and rounded once by int / int
true division, which Python rounds correctly (to nearest, ties to even); OverflowError is +-inf.  A NaN among a key's values, or both infinities, give
a NaN; one infinity gives that infinity; the result passes through + 0.0, so no sum is -0.0.  It is fed the values that were encoded, never a result
of the call under test."""
from fractions import Fraction

import numpy as np

from keyed_many_replica import match_many

SCALE = 1 << 1074
LIMBS = 66
FLAG_NAN, FLAG_POS_INF, FLAG_NEG_INF = 1, 2, 4


def fixed(x):
    """a finite double as the integer x * 2^1074 (exact: every finite double is a multiple of 2^-1074)"""
    n, d = float(x).as_integer_ratio()
    assert SCALE % d == 0
    return n * (SCALE // d)


def round_fixed(N):
    """N * 2^-1074 as the nearest double, ties to even; +-inf beyond DBL_MAX; +0.0 for 0"""
    try:
        return N / SCALE + 0.0  # (int / int: correctly rounded; 0 and every -0.0 become +0.0)
    except OverflowError:
        return float("inf") if N > 0 else float("-inf")


def exact_sum(values):
    """the correctly rounded real sum of a list of doubles under the flags rule"""
    values = np.asarray(values, np.float64)
    nan, pos, neg = bool(np.isnan(values).any()), bool(np.isposinf(values).any()), bool(np.isneginf(values).any())
    if nan or (pos and neg):
        return float("nan")
    if pos or neg:
        return float("inf") if pos else float("-inf")
    return round_fixed(sum(fixed(x) for x in values.tolist()))


def round_limbs(limbs, flags=0):
    """what a table entry rounds to: limbs are 66 Python integers, limb j of weight 2^(32 j - 1074)"""
    assert len(limbs) == LIMBS
    if flags & FLAG_NAN or (flags & FLAG_POS_INF and flags & FLAG_NEG_INF):
        return float("nan")
    if flags & (FLAG_POS_INF | FLAG_NEG_INF):
        return float("inf") if flags & FLAG_POS_INF else float("-inf")
    return round_fixed(sum(int(v) << (32 * j) for j, v in enumerate(limbs)))


def round_fixed_by_fraction(N):
    """round_fixed by another route, for the replica's own test: Fraction -> float is correctly rounded too"""
    try:
        return float(Fraction(N, SCALE)) + 0.0
    except OverflowError:
        return float("inf") if N > 0 else float("-inf")


def host_keyed_sum_exact(val, key, bits, keys):
    """(sums float64[K], counts int64[K + 1]).  val, key: n * 1024 values of one type (float values widen to double exactly); bits: n * 1024 bools;
    keys: K sorted keys, 1 <= K <= 2^20.  counts[i] = the selected rows of key i, counts[K] = the selected rows without a key."""
    val, key = np.ascontiguousarray(val).reshape(-1), np.ascontiguousarray(key).reshape(-1)
    keys = np.asarray(keys)
    K = keys.size
    counts = np.zeros(K + 1, np.int64)
    sums = np.zeros(K, np.float64)
    if val.size:
        rows = np.flatnonzero(np.asarray(bits, bool).reshape(-1))
        idx, matched = match_many(key[rows], keys)
        counts[K] = int((~matched).sum())
        rows, idx = rows[matched], idx[matched]
        counts[:K] = np.bincount(idx, minlength=K)
        x = val[rows].astype(np.float64)
        order = np.argsort(idx, kind="stable")
        idx, x = idx[order], x[order]
        starts = np.flatnonzero(np.concatenate([[True], idx[1:] != idx[:-1]])) if idx.size else np.zeros(0, np.int64)
        ends = np.append(starts[1:], idx.size)
        for s, e in zip(starts.tolist(), ends.tolist()):
            sums[idx[s]] = exact_sum(x[s:e])
    return sums, counts

