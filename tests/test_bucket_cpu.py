"""CPU: tests/bucket_replica.py, the host replica of bucketed aggregation, pinned without a GPU: on a hand-made case against the definition written out
(keyed_replica.host_keyed_sum_dense and a loop over the rows), against histogram_replica.host_histogram for the counts, and on `right`, both zeros,
+-inf edges, duplicate and NaN edges and n_edges == 0."""
import math

import numpy as np
import pytest

from bucket_replica import bucket_of, host_bucket_minmax, host_bucket_sum
from histogram_replica import host_histogram
from keyed_replica import same_sums

INF, NAN = math.inf, math.nan


def columns(n, dtype, seed):
    rng = np.random.default_rng(seed)
    val = np.round(rng.normal(0, 100, n * 1024), 2).astype(dtype)
    key = (rng.integers(-40, 41, n * 1024) * 0.25).astype(dtype)
    val[3::97] = NAN
    val[5::101] = -0.0
    key[7::89] = NAN
    key[11::83] = -0.0
    key[13::79] = INF
    key[17::73] = -INF
    bits = rng.random(n * 1024) < 0.7
    return val, key, bits


def loop_bucket(k, edges, right):
    """the definition, one row: C's comparisons, NaN edges inert"""
    if k != k:
        return None
    return sum(1 for e in edges if (e < k if right else e <= k))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("right", [False, True])
def test_buckets_follow_the_definition_on_zeros_infinities_duplicates_and_nan_edges(dtype, right):
    edges = np.array([-INF, -5.0, -0.0, 0.25, 0.25, 0.25, 3.0, INF, NAN, NAN], dtype)
    keys = np.array([-INF, -6.0, -5.0, -0.0, 0.0, 0.125, 0.25, 0.5, 3.0, 1e30, INF, NAN], dtype)
    got = bucket_of(keys, edges, right)
    want = [loop_bucket(float(k), [float(e) for e in edges], right) for k in keys]
    assert [None if b != b else int(b) for b in got] == want
    z = bucket_of(np.array([-0.0, 0.0], dtype), np.array([0.0], dtype), right)
    assert z.tolist() == ([0.0, 0.0] if right else [1.0, 1.0]), "-0.0 == +0.0 on an edge of 0.0"
    assert not np.isin(got, [4, 5]).any(), "duplicate edges give empty buckets"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("right", [False, True])
def test_the_hand_made_case_against_the_definition_written_out(dtype, right):
    val, key, bits = columns(3, dtype, 1)
    edges = np.array([-INF, -7.5, -0.0, 0.25, 0.25, 2.0, 9.75, NAN], dtype)
    B = edges.size + 1
    s, c = host_bucket_sum(val, key, bits, edges, right)
    sd, cd = host_bucket_sum(val, key, bits, edges, right, dense=True)
    assert same_sums(s, sd) and np.array_equal(c, cd) and s.shape == (B,) and c.shape == (B + 1,)
    # counts, and the plain facts about the sums and records, by a loop over the rows
    b = [loop_bucket(float(k), [float(e) for e in edges], right) for k in key]
    rows = [[i for i in range(key.size) if bits[i] and b[i] == j] for j in range(B)]
    assert c[:B].tolist() == [len(r) for r in rows]
    assert int(c[B]) == sum(1 for i in range(key.size) if bits[i] and b[i] is None) > 0
    assert int(c.sum()) == int(bits.sum())
    rec, cm = host_bucket_minmax(val, key, bits, edges, right)
    assert np.array_equal(cm, c) and rec.dtype == val.dtype and rec.shape == (B, 2)
    for j, r in enumerate(rows):
        x = val[r]
        assert np.isnan(s[j]) == bool(np.isnan(x).any())
        if not np.isnan(s[j]):
            assert abs(s[j] - math.fsum(x.astype(np.float64).tolist())) <= 1e-9 * max(1.0, float(np.abs(x.astype(np.float64)).sum()))
        num = x[~np.isnan(x)]
        if num.size == 0:
            assert rec[j].tolist() == [INF, -INF]
        else:
            assert rec[j, 0] == num.min() and rec[j, 1] == num.max()
            if (num == 0).all():  # -0.0 < +0.0
                assert np.signbit(rec[j, 0]) == bool(np.signbit(num).any()) and np.signbit(rec[j, 1]) == bool(np.signbit(num).all())
    assert c[4] == 0, "the bucket between two equal edges is empty"
    assert c[B - 1] == 0 and c[B - 2] > 0, "a NaN edge is inert: nothing lies at or above it"


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("right", [False, True])
def test_counts_are_the_histogram_replicas(dtype, right):
    val, key, bits = columns(5, dtype, 2)
    rng = np.random.default_rng(3)
    for n_edges in (0, 1, 2, 63, 64, 65, 255, 256, 1023):
        edges = np.sort(rng.choice(np.unique(key[~np.isnan(key)]), min(n_edges, 60), replace=False))
        edges = np.sort(np.concatenate([edges, rng.uniform(-12, 12, n_edges - edges.size).astype(dtype)])).astype(dtype)
        assert edges.size == n_edges
        want = host_histogram(key, edges, bits, right).astype(np.int64)
        s, c = host_bucket_sum(val, key, bits, edges, right)
        rec, cm = host_bucket_minmax(val, key, bits, edges, right)
        assert np.array_equal(c, want) and np.array_equal(cm, want), f"{n_edges} edges"


def test_no_edges_is_one_bucket_and_an_empty_column_is_zero():
    val, key, bits = columns(2, np.float64, 4)
    s, c = host_bucket_sum(val, key, bits, np.zeros(0))
    assert s.shape == (1,) and c.tolist() == [int((bits & ~np.isnan(key)).sum()), int((bits & np.isnan(key)).sum())]
    rec, _ = host_bucket_minmax(val, key, bits, np.zeros(0))
    num = val[bits & ~np.isnan(key) & ~np.isnan(val)]
    assert rec.tolist() == [[num.min(), num.max()]]
    none = np.zeros(0)
    s, c = host_bucket_sum(none, none, np.zeros(0, bool), np.array([1.0, 2.0]))
    assert s.tolist() == [0.0] * 3 and not np.signbit(s).any() and c.tolist() == [0] * 4
    rec, c = host_bucket_minmax(none, none, np.zeros(0, bool), np.array([1.0, 2.0]))
    assert rec.tolist() == [[INF, -INF]] * 3 and c.tolist() == [0] * 4
