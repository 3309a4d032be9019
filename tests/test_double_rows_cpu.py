"""CPU: the inputs of tests/test_register_decode_rows_gpu.py are what that suite says they are — the hand-built double vectors of every packed width 0..64 and
every ALP_RD cut 48..63 (double_rows.py).  Only the oracle and the builder are imported: no GPU, no built library.  These properties are what keeps the GPU
comparisons from going vacuous after an edit of the generator."""
import numpy as np
import pytest

import double_rows as dr


@pytest.fixture(scope="module")
def alp():
    return dr.alp_rows()


@pytest.fixture(scope="module")
def rd():
    return dr.rd_rows()


def exception_bits_of(enc):
    return np.concatenate([enc["exc"][v].view(np.uint64)[: int(enc["exc_cnt"][v])] for v in range(enc["bw"].size)])


def test_the_builders_bit_packing_is_the_oracles(oracle):
    rng = np.random.default_rng(2)
    for bw in range(65):
        vals = rng.integers(0, 2**64, 1024, dtype=np.uint64) >> np.uint64(64 - bw) if bw else np.zeros(1024, np.uint64)
        words = dr.pack_u64(vals, bw)
        assert np.array_equal(words.view(np.uint64), oracle.ffor_u64(vals, bw, 0)[: 16 * bw]), bw
        assert np.array_equal(dr.unpack_u64(words, bw), vals), bw
    for bw in (1, 2, 3):
        vals = rng.integers(0, 1 << bw, 1024).astype(np.uint16)
        assert np.array_equal(dr.unpack_u16(dr.pack_u16(vals, bw), bw), vals)
        assert np.array_equal(dr.pack_u16(vals, bw), oracle.ffor_u16(vals, bw)[: 64 * bw])


def test_alp_rows_hold_every_width_factor_and_exception_count(alp, oracle):
    n = alp["bw"].size
    assert n % 100 == 0 and n < 5000 and alp["base"].dtype == np.int64 and alp["packed"].dtype == np.int64 and (alp["scheme"] == 2).all()
    bw, f, e = alp["bw"].astype(int), alp["f"].astype(int), alp["e"].astype(int)
    assert set(bw.tolist()) == set(range(65)) and set(f.tolist()) == set(dr.FACTORS)
    assert (e >= f).all() and (e <= 18).all() and (e - f <= 2).all()
    assert all(((e - f) == d).any() for d in (0, 1, 2))
    assert set(alp["exc_cnt"].tolist()) == set(dr.ALP_EXC_COUNTS) == {0, 1, 5, 63, 64, 65, 128, 129, 1024}
    for w in range(65):  # no width sees only one side of a lane count or of the stage
        at = alp["exc_cnt"][bw == w]
        assert (at == 0).any() and (at >= 129).any() and ((at > 0) & (at <= 128)).any(), w
    # the exception count does not move in step with the base list: every count meets (nearly) every base kind
    for c in dr.ALP_EXC_COUNTS:
        rows = alp["exc_cnt"] == c
        assert len(set(bw[rows].tolist())) >= 50 and set(f[rows].tolist()) == set(dr.FACTORS), c
        assert (alp["base"][rows] == 0).any() and (alp["base"][rows] == -1).any() and (alp["base"][rows] == dr.INT64_MIN + 1).any(), c
    pos = alp["pos"].astype(int)
    for v in range(n):
        c = int(alp["exc_cnt"][v])
        assert (np.diff(pos[v, :c]) > 0).all() and (c == 0 or pos[v, c - 1] < 1024)
    # both extreme digits are in every row outside its exception positions (a bound only bites where base + 0 or base + mask occurs)
    for v in range(0, n, 7):
        if alp["exc_cnt"][v] < 1024 and bw[v] > 0:
            digits = dr.unpack_u64(alp["packed"][v], int(bw[v]))
            keep = np.ones(1024, bool)
            keep[pos[v, : int(alp["exc_cnt"][v])]] = False
            assert (digits[keep] == 0).any() and (digits[keep] == np.uint64((1 << int(bw[v])) - 1)).any(), v
    # exception values: three rows of four finite, the fourth with both NaN kinds, both infinities, -0.0 and a denormal somewhere
    for v in np.nonzero(alp["exc_cnt"] > 0)[0]:
        if v % 4:
            assert np.isfinite(alp["exc"][v, : int(alp["exc_cnt"][v])]).all(), v
    bits = exception_bits_of({k: a[::4] for k, a in alp.items() if a.shape[0] == n})
    is_nan = ((bits >> np.uint64(52)) & np.uint64(0x7FF) == 0x7FF) & (bits & np.uint64(0xFFFFFFFFFFFFF) != 0)
    quiet = bits & np.uint64(1 << 51) != 0
    assert (is_nan & quiet).any() and (is_nan & ~quiet).any()
    for special in (0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000, 0x0000000000000001):
        assert (bits == np.uint64(special)).any(), hex(special)
    assert oracle.decode_column(alp).size == n * 1024  # the oracle takes every row


def test_alp_rows_reach_both_sides_of_the_shortcut_rule_at_every_width(alp):
    bw, f, base = alp["bw"].astype(int), alp["f"].astype(int), [int(b) for b in alp["base"]]
    n = len(base)
    sc = np.array([dr.shortcut_applies(int(bw[v]), int(f[v]), base[v]) for v in range(n)])
    mask = [(1 << int(b)) - 1 for b in bw]  # (Python integers: base + mask may leave int64)
    bnd = [dr.SHORTCUT_BOUND[int(ff)] for ff in f]
    assert len(dr.SHORTCUT_BOUND) == 19 and all(b == min(2**51 - 1, (2**63 - 1) // 10**i) for i, b in enumerate(dr.SHORTCUT_BOUND))
    assert 300 <= int(sc.sum()) <= n - 300
    for ff in dr.FACTORS:
        for b in range(65):
            rows = np.nonzero((f == ff) & (bw == b))[0]
            assert (~sc[rows]).any(), (ff, b)
            if b <= dr.SHORTCUT_MAX_BW and (1 << b) - 1 <= 2 * dr.SHORTCUT_BOUND[ff]:  # the width can qualify: some base fits it between the two bounds
                assert sc[rows].any(), (ff, b)
                # on the bounds themselves the two outcomes differ by that one step
                assert any(sc[v] and base[v] == -bnd[v] for v in rows) and any(not sc[v] and base[v] == -bnd[v] - 1 for v in rows), (ff, b)
                assert any(sc[v] and base[v] + mask[v] == bnd[v] for v in rows) and any(not sc[v] and base[v] + mask[v] == bnd[v] + 1 for v in rows), (ff, b)
            else:
                assert not sc[rows].any(), (ff, b)
    assert not sc[bw > dr.SHORTCUT_MAX_BW].any()
    assert any(base[v] + mask[v] > dr.INT64_MAX for v in range(n)), "a base whose base + mask wraps int64"
    assert any(base[v] == dr.INT64_MIN + 1 for v in range(n)) and any(base[v] == 0 for v in range(n)) and any(base[v] == -1 for v in range(n))
    for c in (129, 1024):  # the branch past the stage on both routes
        assert ((alp["exc_cnt"] == c) & sc).any() and ((alp["exc_cnt"] == c) & ~sc).any(), c


def test_rd_rows_are_cuts_the_reference_can_produce(rd, oracle):
    n = rd["bw"].size
    cuts = dr.rd_cuts()
    assert (rd["scheme"] == 1).all() and n == 100 * len(cuts) and len(cuts) == 45
    assert [(int(rd["bw"][100 * r]), int(rd["lbw"][100 * r])) for r in range(n // 100)] == cuts
    assert set(rd["bw"].tolist()) == set(range(48, 64)) and set(rd["lbw"].tolist()) == {1, 2, 3}
    assert set(rd["exc_cnt"].tolist()) == set(dr.RD_EXC_COUNTS) and {511, 512, 513} <= set(dr.RD_EXC_COUNTS)
    full_dictionaries, finite_rowgroups = 0, 0
    values = oracle.decode_column(rd).reshape(-1, 100 * 1024)
    for r in range(n // 100):
        rows = slice(100 * r, 100 * r + 100)
        rbw, lbw, size = int(rd["bw"][100 * r]), int(rd["lbw"][100 * r]), int(rd["dict_size"][r])
        assert (rd["bw"][rows] == rbw).all() and (rd["lbw"][rows] == lbw).all(), "one cut per rowgroup"
        assert max(1, int(np.ceil(np.log2(size)))) == lbw and len(set(rd["dict"][r, :size].tolist())) == size
        assert int(rd["dict"][r].max()) < 2 ** (64 - rbw)
        used = set()
        for v in (100 * r, 100 * r + 57, 100 * r + 99):
            idx = dr.unpack_u16(rd["packed_left"][v], lbw)
            assert np.array_equal(idx, oracle.unffor_u16(rd["packed_left"][v], lbw)) and int(idx.max()) < size, "left indices stay below the dictionary size"
            used |= set(idx.tolist())
            c = int(rd["exc_cnt"][v])
            assert (np.diff(rd["pos"][v, :c].astype(int)) > 0).all()
            assert c == 0 or int(rd["exc"][v].view(np.uint16)[:c].max()) < 2 ** (64 - rbw)
        if size == 8:
            assert {4, 5, 6, 7} <= used, "the dictionary's upper half is in use"
            full_dictionaries += 1
        finite_rowgroups += bool(np.isfinite(values[r]).all())
    assert full_dictionaries >= 5
    # three rowgroups of four, but for the cuts that leave bit 62 to the right part (63, 1) or too few left patterns without it ((62, 2) and (61, 3))
    assert finite_rowgroups >= 3 * (n // 100) // 4 - 3, finite_rowgroups
    for c in dr.RD_EXC_COUNTS:
        assert len(set(rd["bw"][rd["exc_cnt"] == c].tolist())) == 16, c


def test_the_oracles_decode_of_the_rows_is_a_fixed_function_of_the_seed(alp, rd, oracle):
    for make, first in ((dr.alp_rows, alp), (dr.rd_rows, rd)):
        again = make()
        assert first.keys() == again.keys() and all(first[k].tobytes() == again[k].tobytes() for k in first)
        want = oracle.decode_column(first)
        assert want.tobytes() == oracle.decode_column(again).tobytes()
        # ... and it is falp + patch (the dictionary glue) as ten lines of numpy state them, on a sample of the rows that holds every width / cut
        n = first["bw"].size
        sample = sorted(set(range(0, n, 13)) | {int(np.nonzero(first["bw"] == w)[0][0]) for w in set(first["bw"].tolist())})
        for v in sample:
            got = dr.numpy_decode_vector(first, v)
            assert np.array_equal(got.view(np.uint64), want[1024 * v:1024 * v + 1024].view(np.uint64)), (v, int(first["bw"][v]), int(first["f"][v]), int(first["e"][v]), int(first["base"][v]))


def test_the_moved_builders_give_test_decode_gpu_the_vectors_it_had():
    """tests/test_decode_gpu.py's hand-built vectors come from here now: the shapes and dtypes its three builders spelled out"""
    enc = dr.alp_vectors_with_exception_counts(np.random.default_rng(7006), [0, 1, 129, 1024, 300], 6, "edges")
    assert enc["exc_cnt"].tolist() == [0, 1, 129, 1024, 300] and (enc["bw"] == 6).all() and enc["pos"][1, 0] == 0 and {0, 255, 256, 511, 512, 767, 768, 1023} <= set(enc["pos"][2, :129].tolist())
    front = dr.alp_vectors_with_exception_counts(np.random.default_rng(1), [300, 5], 17, "front")
    assert front["exc_cnt"].tolist() == [256, 5] and int(front["pos"][0, :256].max()) == 255
    e = dr.empty_encoding(37)
    assert {k: (a.shape, a.dtype) for k, a in e.items()} == {
        "scheme": ((37,), np.uint8), "e": ((37,), np.uint8), "f": ((37,), np.uint8), "bw": ((37,), np.uint8), "lbw": ((37,), np.uint8), "base": ((37,), np.int64),
        "exc_cnt": ((37,), np.uint16), "packed": ((37, 1024), np.int64), "packed_left": ((37, 1024), np.uint16), "exc": ((37, 1024), np.float64),
        "pos": ((37, 1024), np.uint16), "dict": ((1, 8), np.uint16), "dict_size": ((1,), np.uint8), "k": ((1,), np.uint8), "combos": ((1, 10), np.int32)}
    assert (e["scheme"] == 2).all() and (e["k"] == 1).all()
