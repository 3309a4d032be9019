"""The host replica of the histograms (include/alpgpu.h, "histograms": alpgpu_histogram_*), by numpy alone: isnan, searchsorted, bincount.  It knows
nothing of the library; the tests feed it the store decode (or the oracle's decode) and compare integers."""
import numpy as np


def sorted_edges(edges):
    """the edges as the call wants them: ascending, NaNs last (numpy.sort's order)"""
    return np.sort(np.asarray(edges))


def host_histogram(x, edges, selected=None, right=False):
    """counts[len(edges) + 2] as uint64: counts[b] = the selected values that are no NaNs and have b = #{i : edges[i] <= x} (right: < x);
    counts[-1] = the selected NaNs.  edges: sorted, NaNs (inert) last.  selected: a bool array over x, None: all of x."""
    x = np.asarray(x)
    edges = np.asarray(edges, dtype=x.dtype)
    n_edges = edges.size
    sel = np.ones(x.size, bool) if selected is None else np.asarray(selected, bool)
    xs = x[sel]
    nan = np.isnan(xs)
    real = edges[~np.isnan(edges)]  # a NaN edge is never <= anything: behind the last real edge it moves no value
    assert np.all(np.isnan(edges[real.size:])) and np.all(real[:-1] <= real[1:]), "edges must be sorted with their NaNs last"
    b = np.searchsorted(real, xs[~nan], side="left" if right else "right")
    counts = np.zeros(n_edges + 2, np.uint64)
    counts[:n_edges + 1] = np.bincount(b, minlength=n_edges + 1).astype(np.uint64)
    counts[n_edges + 1] = np.uint64(int(nan.sum()))
    return counts


def unpack_mask(mask_words, n_values):
    """a selection bitmap (uint64 / int64 words, bit r & 63 of word r >> 6 = value index r) as a bool array over the first n_values indices"""
    w = np.ascontiguousarray(mask_words).view(np.uint64)
    bits = (w[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    return bits.reshape(-1)[:n_values].astype(bool)
