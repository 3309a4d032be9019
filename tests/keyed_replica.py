"""Host replica of the order include/alpgpu.h documents for alpgpu_decode_keyed_sum_* (no GPU, numpy only): shared by tests/test_keyed_cpu.py, which
pins it on a hand-made case, and the GPU suites, which hold the kernels to it bit for bit.  It is fed the oracle's or the store decode's values,
never a result of the call under test.

Two forms of the same definition: host_keyed_sum_dense writes the definition out (a [n, 16, 64] array per key, adjacent_tree per step,
np.add.accumulate along the stripe, host_group_totals over the stripes) and is meant for small inputs; host_keyed_sum holds only the selected,
matched rows and is what the GPU suites use.  tests/test_keyed_cpu.py holds the two to each other."""
import numpy as np

from group_replica import adjacent_tree, host_group_totals

KEYS_MAX, STRIPES_MAX = 1024, 4096


def stripe_vectors(n_vectors):
    """L = max(1, ceil(n_vectors / 4096))"""
    return max(1, -(-int(n_vectors) // STRIPES_MAX))


def match_keys(key, keys):
    """(idx, matched) per row: idx = the first position with keys[idx] == key under C's == (keys sorted as numpy.sort sorts, NaNs last; -0.0 == +0.0;
    a NaN on either side never matches)"""
    keys = np.asarray(keys)
    assert keys.dtype == key.dtype and 1 <= keys.size <= KEYS_MAX
    pos = np.searchsorted(keys, key, side="left")
    at = np.minimum(pos, keys.size - 1)
    with np.errstate(invalid="ignore"):
        matched = keys[at] == key
    return at, matched


def host_keyed_sum_dense(val, key, bits, keys):
    """(sums [K] float64, counts [K + 1] int64), the definition written out.  val, key: n * 1024 values; bits: n * 1024 bools; keys: K sorted keys"""
    n = val.size // 1024
    K = len(keys)
    x = val.astype(np.float64).reshape(n, 16, 64)
    b = np.asarray(bits, bool).reshape(n, 16, 64)
    idx, matched = match_keys(key.reshape(n, 16, 64), keys)
    L = stripe_vectors(n)
    S = -(-n // L)
    A = np.zeros((K, max(S, 1)))
    counts = np.zeros(K + 1, np.int64)
    counts[K] = int((b & ~matched).sum())
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(K):
            q = b & matched & (idx == i)
            counts[i] = int(q.sum())
            P = adjacent_tree(np.where(q, x, 0.0))  # [n, 16]: lane l holds the value or +0.0
            for s in range(S):
                steps = P[s * L: min((s + 1) * L, n)].reshape(-1)  # v ascending, m ascending
                A[i, s] = np.add.accumulate(np.concatenate([[0.0], steps]))[-1]  # starts at +0.0, one += per step, in order
    if n == 0:
        return np.zeros(K), counts
    return host_group_totals(A)[0], counts


def host_keyed_sum(val, key, bits, keys):
    """the same result from the selected, matched rows alone.  A lane that does not belong to key i holds +0.0, and x + (+0.0) is x for every x but
    -0.0, which it makes +0.0: so a tree node with one member child is `child + 0.0`, one with two is `left + right`, one with none is +0.0 and
    adds nothing to a stripe's accumulator (which began at +0.0 and is never -0.0)."""
    n = val.size // 1024
    K = len(keys)
    b = np.asarray(bits, bool).reshape(-1)
    idx, matched = match_keys(key.reshape(-1), keys)
    counts = np.zeros(K + 1, np.int64)
    counts[K] = int((b & ~matched).sum())
    if n == 0:
        return np.zeros(K), counts
    rows = np.flatnonzero(b & matched)
    counts[:K] = np.bincount(idx[rows], minlength=K)
    L = stripe_vectors(n)
    S = -(-n // L)
    A = np.zeros((K, S))
    if rows.size:
        x = val.reshape(-1)[rows].astype(np.float64)
        step, lane = rows >> 6, rows & 63
        pair = idx[rows].astype(np.int64) * (n * 16) + step  # (key, step): key-major, steps ascending = v ascending, m ascending
        order = np.lexsort((lane, pair))
        x, pair, node = x[order], pair[order], lane[order]
        with np.errstate(invalid="ignore", over="ignore"):
            for _ in range(6):  # lanes -> pairs -> ... -> the step's root
                node = node >> 1
                same = np.zeros(x.size, bool)
                same[:-1] = (pair[1:] == pair[:-1]) & (node[1:] == node[:-1])  # this entry is a left child whose right sibling is the next entry
                right = np.zeros(x.size, bool)
                right[1:] = same[:-1]
                nxt = np.empty_like(x)
                nxt[:-1] = x[1:]
                nxt[-1:] = 0.0
                x = np.where(same, x + nxt, x + 0.0)[~right]
                pair, node = pair[~right], node[~right]
            # x = P(i, v, m) of every (key, step) with a member, in (key, step) order; the stripe's sequential sum, group by group
            i_of, step_of = pair // (n * 16), pair % (n * 16)
            group = i_of * S + (step_of >> 4) // L
            start = np.flatnonzero(np.concatenate([[True], group[1:] != group[:-1]]))
            rank = np.arange(x.size) - np.repeat(start, np.diff(np.concatenate([start, [x.size]])))
            flat = A.reshape(-1)
            for r in range(int(rank.max()) + 1):
                at = rank == r
                flat[group[at]] = flat[group[at]] + x[at]  # (one entry per group and rank)
    return host_group_totals(A)[0], counts


def same_sums(a, b):
    """bit for bit, NaNs as NaNs (a selected NaN makes its key's sum a NaN of unspecified payload)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))
