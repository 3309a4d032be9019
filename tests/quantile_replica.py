"""Host replica of the quantiles (include/alpgpu.h, "quantiles": alpgpu_select_rank_*, alpgpu_quantile_*): the definition, by numpy on integer views.

S = the selected values that are no NaNs (by the bits), sorted by ascending okey (top-k's order: -inf < ... < -0.0 < +0.0 < ... < +inf); N = |S|.
select_rank: S[min(r, N - 1)], from_top: S[N - 1 - min(r, N - 1)].  quantile: r = min(N - 1, floor(q * (N - 1))) with one double multiplication, the
neighbours S[r] and S[min(r + 1, N - 1)].  Nothing here comes from the code under test."""
import numpy as np

from top_k_replica import is_nan_bits, okey, unpack_mask  # noqa: F401  (unpack_mask: for the tests)


def sorted_selection(x, bits):
    """the selected values of x (flat; bits: bool of the same length) that are no NaNs, in ascending okey order, carrying the bits of x"""
    x = np.ascontiguousarray(x).reshape(-1)
    s = x[np.asarray(bits, bool).reshape(-1) & ~is_nan_bits(x)]
    return s[np.argsort(okey(s), kind="stable")]


def host_select_rank(s, ranks, from_top=False):
    """s: sorted_selection(...).  Returns (values, N); no values for N == 0"""
    n = s.size
    if n == 0:
        return s[:0], 0
    at = np.array([min(int(r), n - 1) for r in ranks], dtype=np.int64)
    if from_top:
        at = n - 1 - at
    return s[at], n


def quantile_ranks(q, n):
    """r_i = min(N - 1, floor(q_i * (N - 1))): one IEEE double multiplication, then floor (n > 0)"""
    pos = np.asarray(q, dtype=np.float64) * np.float64(n - 1)
    return np.minimum(np.floor(pos).astype(np.uint64), np.uint64(n - 1)).astype(np.int64)


def host_quantile(s, q):
    """s: sorted_selection(...).  Returns (pairs [len(q), 2] = the two neighbours, ranks, N); nothing for N == 0"""
    n = s.size
    if n == 0:
        return s[:0].reshape(0, 2), np.zeros(0, np.int64), 0
    r = quantile_ranks(q, n)
    return np.stack([s[r], s[np.minimum(r + 1, n - 1)]], axis=1), r, n
