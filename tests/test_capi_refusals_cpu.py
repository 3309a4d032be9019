"""CPU: what the Python wrappers of the list-taking query families (alp_amd/capi.py) refuse, they refuse with ValueError before the library is
called and before anything is moved to or allocated on a device.  No device: the context is bare, the columns are bare descriptors, and every
launching entry point of the families is replaced by one that fails the test.  One row per wrapper; the rules are the same for all of them
(a list of the column's type, one dimension, the family's length limits, on the host or on this device), so the cases are generated from the row.
The per-family tests of the same name in tests/test_keyed*_cpu.py stay beside this one."""
import numpy as np
import pytest
import torch

from alp_amd import capi

FAMILIES = ("select_in_mask", "histogram", "keyed_sum", "keyed_minmax", "bucket_sum", "bucket_minmax", "join_probe", "distinct", "top_k")
TORCH = {"f64": torch.float64, "f32": torch.float32}
NUMPY = {"f64": np.float64, "f32": np.float32}
OTHER = {"f64": "f32", "f32": "f64"}

# wrapper, what it calls its list, columns it takes, column types it is built for, shortest list, longest list (None: no limit)
ALLOCATING = [
    ("select_in_mask", 1, ("f64", "f32"), 0, None),
    ("histogram", 1, ("f64", "f32"), 0, capi.HISTOGRAM_EDGES_MAX),
    ("keyed_sum", 2, ("f64",), 1, capi.KEYED_KEYS_MAX),
    ("keyed_minmax", 2, ("f64", "f32"), 1, capi.KEYED_KEYS_MAX),
    ("keyed_minmax_many", 2, ("f64", "f32"), 1, capi.KEYED_MANY_KEYS_MAX),
    ("bucket_sum", 2, ("f64", "f32"), 0, capi.BUCKET_EDGES_MAX),
    ("bucket_minmax", 2, ("f64", "f32"), 0, capi.BUCKET_EDGES_MAX),
    ("join_probe", 1, ("f64", "f32"), 0, None),
]
# the raw form, columns it takes, column types, the outputs that follow the list (host tensors of the right type and shape for a list of 3)
RAW = [
    ("histogram_into", 1, ("f64", "f32"), lambda tdt: (torch.zeros(5, dtype=torch.int64),)),
    ("keyed_sum_into", 2, ("f64",), lambda tdt: (torch.zeros(3, dtype=torch.float64),)),
    ("keyed_minmax_into", 2, ("f64", "f32"), lambda tdt: (torch.zeros((3, 2), dtype=tdt),)),
    ("keyed_minmax_many_into", 2, ("f64", "f32"), lambda tdt: (torch.zeros((3, 2), dtype=tdt),)),
    ("bucket_sum_into", 2, ("f64", "f32"), lambda tdt: (torch.zeros(4, dtype=torch.float64),)),
    ("bucket_minmax_into", 2, ("f64", "f32"), lambda tdt: (torch.zeros((4, 2), dtype=tdt),)),
    ("join_probe_into", 1, ("f64", "f32"), lambda tdt: (torch.zeros(8, dtype=torch.int64), torch.zeros(1, dtype=torch.int64))),
]


class Col:  # what the wrappers look at before they reach the library
    def __init__(self, dtype, n_vectors=4):
        self.dtype, self.n_vectors, self.c = dtype, n_vectors, capi.CColumn()


class Elsewhere(torch.Tensor):  # a host tensor that says it lives on cuda:1: nothing dereferences it here
    is_cuda = property(lambda self: True)
    device = property(lambda self: torch.device("cuda", 1))


@pytest.fixture
def ctx(monkeypatch):
    def unreachable(*a, **k):
        raise AssertionError("the library was called")
    names = [n for n in vars(capi.lib) if n.startswith("alpgpu_") and any(f in n for f in FAMILIES) and not n.endswith("_bytes")]
    assert "alpgpu_join_probe_f32" in names and "alpgpu_debug_decode_bucket_minmax_f64" in names and len(names) == 32, names
    for n in names:
        monkeypatch.setattr(capi.lib, n, unreachable)
    c = capi.Context.__new__(capi.Context)
    c.device = 0
    return c


def bad_lists(t, lo, hi):
    """(why, list) for a wrapper over columns of type t that takes lo .. hi elements"""
    tdt, ndt, o = TORCH[t], NUMPY[t], OTHER[t]
    out = [("a numpy array of the other float type", np.array([1.0, 2.0, 3.0], NUMPY[o])),
           ("a tensor of the other float type", torch.zeros(3, dtype=TORCH[o])),
           ("an int64 tensor", torch.zeros(3, dtype=torch.int64)),
           ("an int64 numpy array", np.zeros(3, np.int64)),
           ("a two-dimensional array", np.zeros((2, 2), ndt)),
           ("a two-dimensional tensor", torch.zeros((2, 2), dtype=tdt)),
           ("a list of lists", [[1.0, 2.0], [3.0, 4.0]]),
           ("a tensor on another device", torch.zeros(3, dtype=tdt).as_subclass(Elsewhere))]
    if hi is not None:
        out += [("one more than the limit, numpy", np.zeros(hi + 1, ndt)), ("one more than the limit, tensor", torch.zeros(hi + 1, dtype=tdt))]
    if lo == 1:
        out += [("an empty sequence", []), ("an empty array", np.zeros(0, ndt)), ("an empty tensor", torch.zeros(0, dtype=tdt))]
    return out


@pytest.mark.parametrize("name,n_cols,types,lo,hi", ALLOCATING, ids=[r[0] for r in ALLOCATING])
def test_the_allocating_wrappers_refuse_a_list_that_does_not_fit(ctx, name, n_cols, types, lo, hi):
    fn = getattr(ctx, name)
    for t in types:
        cols = [Col(t) for _ in range(n_cols)]
        for why, bad in bad_lists(t, lo, hi):
            with pytest.raises(ValueError):
                fn(*cols, bad)
                pytest.fail("%s(%s) took %s" % (name, t, why))


@pytest.mark.parametrize("name,n_cols,types,lo,hi", [r for r in ALLOCATING if r[1] == 2], ids=[r[0] for r in ALLOCATING if r[1] == 2])
def test_the_two_column_wrappers_refuse_columns_that_do_not_pair(ctx, name, n_cols, types, lo, hi):
    good = np.array([1.0, 2.0, 3.0])
    for val, key in ((Col("f64"), Col("f32")), (Col("f32"), Col("f64")), (Col("f64", 4), Col("f64", 3))):
        with pytest.raises(ValueError):
            getattr(ctx, name)(val, key, good.astype(NUMPY[val.dtype]))
        with pytest.raises(ValueError):
            getattr(ctx, name)(val, key, good.astype(NUMPY[key.dtype]))


def test_keyed_sum_refuses_float_columns(ctx):
    good = np.array([1.0, 2.0, 3.0], np.float32)
    with pytest.raises(ValueError):
        ctx.keyed_sum(Col("f32"), Col("f32"), good)
    with pytest.raises(ValueError):
        ctx.keyed_sum_into(Col("f32"), Col("f32"), torch.from_numpy(good), torch.zeros(3, dtype=torch.float64))


@pytest.mark.parametrize("t", ("f64", "f32"))
def test_ranges_ops_and_accumulate(ctx, t):
    col, good = Col(t), np.array([1.0, 2.0, 3.0], NUMPY[t])
    for kw in ({"first": -1}, {"n": -1}, {"first": -1024, "n": 2048}):
        with pytest.raises(ValueError):
            ctx.select_in_mask(col, good, **kw)
        with pytest.raises(ValueError):
            ctx.histogram(col, good, **kw)
    with pytest.raises(ValueError):
        ctx.select_in_mask(col, good, first=4 * 1024 + 1)  # n None is what is left of the column: a negative number
    with pytest.raises(ValueError):
        ctx.histogram(col, good, first=4 * 1024 + 1)  # new with the shared range rule: histogram used to allocate its result before it found this
    for kw in ({"op": "and"}, {"op": "or"}, {"op": "xor"}, {"op": "xor", "mask": torch.zeros(64, dtype=torch.int64)}):  # combining wants a mask
        with pytest.raises(ValueError):
            ctx.select_in_mask(col, good, **kw)
    with pytest.raises(ValueError):
        ctx.histogram(col, good, accumulate=True)  # adds to a tensor: there is none


@pytest.mark.parametrize("name,n_cols,types,outs", RAW, ids=[r[0] for r in RAW])
def test_the_raw_forms_take_a_device_tensor_only(ctx, name, n_cols, types, outs):
    fn = getattr(ctx, name)
    for t in types:
        cols = [Col(t) for _ in range(n_cols)]
        good = np.array([1.0, 2.0, 3.0], NUMPY[t])
        for bad in (torch.from_numpy(good), good.tolist(), good, torch.zeros(3, dtype=TORCH[OTHER[t]]), torch.from_numpy(good).as_subclass(Elsewhere)):
            with pytest.raises(ValueError):
                fn(*cols, bad, *outs(TORCH[t]))
    if n_cols == 2:
        for val, key in ((Col("f64"), Col("f32")), (Col("f64", 4), Col("f64", 3))):
            with pytest.raises(ValueError):
                fn(val, key, torch.zeros(3, dtype=torch.float64), *outs(torch.float64))


def test_the_scratch_makers_refuse_sizes_out_of_range(ctx):
    for n, k in ((-1, 4), (10, 0), (10, capi.KEYED_KEYS_MAX + 1)):
        with pytest.raises(ValueError):
            ctx.keyed_sum_scratch(n, k)
    for n, k in ((-1, 4), (10, -1), (10, capi.BUCKET_EDGES_MAX + 1)):
        with pytest.raises(ValueError):
            ctx.bucket_sum_scratch(n, k)
    for cap in (0, -1, capi.DISTINCT_MAX + 1):
        with pytest.raises(ValueError):
            ctx.distinct_scratch(cap)
        with pytest.raises(ValueError):
            ctx.distinct(Col("f64"), capacity=cap)
    for k in (-1, capi.TOP_K_MAX + 1, 1.5, True, "3"):
        with pytest.raises(ValueError):
            ctx.top_k_scratch(Col("f64"), k)
        with pytest.raises(ValueError):
            ctx.top_k(Col("f64"), None, k)
