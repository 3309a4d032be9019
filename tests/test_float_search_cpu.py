"""CPU: the float boundary set of the (e,f) search (datagen.search_boundary_values_f32 / search_boundary_mixtures_f32), the inputs of
tests/test_float_search_gpu.py.

  1. the inputs are what they claim: how many values, which candidates the constant vectors make the search choose, both schemes, and what the
     mixtures' rowgroups and vectors look like.  Needs the float oracle only, so it runs everywhere.  The floors are conditions on the inputs, set
     below what the oracle gives for them (1418 values; 65 of the 66 candidates, all but (10,8); 174 ALP_RD; 54 ALP rowgroups, all with k in
     {2, 3}; 19 first candidates; widths 0..32; 1 to 1024 exceptions).
  2. the oracle is the reference on them (skipped when oracle/_ref is absent, like tests/test_oracle_f32.py): encode_value of every value under all
     66 (e,f), decode_value of every resulting integer for f <= 9 (f = 10 reads past FACT_ARR in the reference), every constant-vector column and
     every mixture."""
import numpy as np
import pytest

import datagen
import golden_io

SEEDS = list(range(60))
ALL_EF = [(e, f) for e in range(10, -1, -1) for f in range(e, -1, -1)]  # the search's candidate order


def unique_bits(vals):
    return vals[np.unique(vals.view(np.uint32), return_index=True)[1]]


def describe(v):
    return f"{float(v)!r} (0x{int(np.float32(v).view(np.uint32)):08x})"


def tail_threshold_sample_sets(of32):
    """Sample sets for the two LAST candidates of the float search, (1,0) and (0,0) — the ones k_rowgroup_init<PrecF32> evaluates "on its side": one
    sample per lane, the count by a ballot, the range by a DPP min / max.  With one constant value per set that reduction has nothing to get wrong, so
    here the 32 samples differ, and the set sits on the ALP / ALP_RD threshold (22 bits per value, 704 for 32 samples), where count and range decide
    the scheme: 32 samples that the candidate round-trips (chosen with the oracle's encode_simdized) and practically no other does — integers
    2^30 + 128 j for (0,0), which leave int32 when multiplied by ten; one-decimal values m / 10 with m in [2^23, 1.5 * 2^23) for (1,0), which have
    fraction bits and whose integers times ten or more wrap — spanning 20, 21 or 22 bits, with 0, 1 or 2 of them replaced by 1e30 (an exception,
    48 bits): 21 bits / none and 20 bits / one stay ALP, one bit or one exception more is ALP_RD.  The minimum sits at each of the 32 positions in turn,
    the maximum eleven further on.  -> [(candidate, bits, exceptions, position of the minimum, samples)]"""
    rng = np.random.default_rng(5)
    sets = []
    for e, f in ((0, 0), (1, 0)):
        if e == 0:
            codes = 2**30 + 128 * np.arange(2**15, dtype=np.int64)
        else:
            codes = np.unique(rng.integers(2**23, 2**23 + 2**22, 16 * 1024))
        vals = (codes / 10.0**e).astype(np.float32)
        fits = np.ones(codes.size, bool)
        for o in range(0, codes.size, 1024):
            chunk = np.resize(vals[o:o + 1024], 1024)
            _, _, pos, cnt = of32.encode_simdized(chunk, f, e)
            bad = pos[:cnt].astype(np.int64)
            fits[o + bad[bad < codes.size - o]] = False
        codes, vals = codes[fits], vals[fits]
        for bits in (20, 21, 22):
            top = int(np.searchsorted(codes, codes[0] + 2**bits - 1, side="right")) - 1
            assert int(codes[top] - codes[0]).bit_length() == bits
            for n_exc in (0, 1, 2):
                for p in range(32):
                    s = vals[rng.integers(1, top, 32)]
                    s[p], s[(p + 11) % 32] = vals[0], vals[top]
                    for j in range(n_exc):
                        s[(p + 3 + 7 * j) % 32] = np.float32(1e30)
                    sets.append(((e, f), bits, n_exc, p, s))
    return sets


def column_of_samples(samples):
    """a vector whose first-level samples (every 32nd value) are `samples`"""
    return np.repeat(np.asarray(samples, np.float32), 32)


@pytest.fixture(scope="module")
def of32():
    from oracle.pyoracle import OracleF32
    return OracleF32()


@pytest.fixture(scope="module")
def rf32():
    from oracle.pyoracle import ReferenceF32
    if not ReferenceF32.available():
        pytest.skip("oracle/_ref without float entry points")
    return ReferenceF32()


@pytest.fixture(scope="module")
def values():
    return unique_bits(datagen.search_boundary_values_f32())


@pytest.fixture(scope="module")
def constant_encodings(of32, values):
    """the oracle's encoding of one constant vector per value"""
    return [of32.encode_column(np.full(1024, v, np.float32)) for v in values]


@pytest.fixture(scope="module")
def mixtures(of32):
    cols = [datagen.search_boundary_mixtures_f32(seed) for seed in SEEDS]
    return cols, [of32.encode_column(c) for c in cols]


def test_the_generators_give_what_they_describe():
    vals, tags = datagen.search_boundary_values_f32(tagged=True)
    assert vals.dtype == np.float32 and vals.size == tags.size
    assert np.array_equal(vals.view(np.uint32), datagen.search_boundary_values_f32().view(np.uint32))
    assert (tags[:10] == -1).all() and set(tags[10:].tolist()) == set(range(11))
    bits = set(vals.view(np.uint32).tolist())
    for want in (0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, 1.1754944e-38, np.inf, -np.inf, 3.4028235e38,  # the specials
                 2147483648.0, -2147483904.0, 2147483520.0, 4294967296.0, 12582912.0, 4194304.5, -6291456.5, 9.223372e18):  # the range test's ends, 2^32, the magic number, halves
        assert int(np.float32(want).view(np.uint32)) in bits, want
    assert np.isnan(vals).sum() == 1
    col = datagen.search_boundary_mixtures_f32(3)
    assert col.dtype == np.float32 and col.size == 25 * 1024
    assert np.array_equal(col.view(np.uint32), datagen.search_boundary_mixtures_f32(3).view(np.uint32)) and np.isfinite(col).all()
    pool = set(vals[np.isfinite(vals)].view(np.uint32).tolist())
    off_sample = np.ones(col.size, bool)
    off_sample[::32] = False
    assert (np.abs(col[off_sample]) <= 1000.0).all(), "boundary values sit at sampled positions only"
    placed = [v for v in col[::32].view(np.uint32).tolist() if v in pool]
    assert 25 <= len(placed)


def test_the_inputs_are_what_they_claim(of32, values, constant_encodings, mixtures):
    assert values.size >= 1400
    # constant vectors: which candidate the search chooses first, or ALP_RD
    chosen, n_rd = set(), 0
    for v, enc in zip(values, constant_encodings):
        assert np.array_equal(of32.decode_column(enc).view(np.uint32), np.full(1024, v, np.float32).view(np.uint32)), describe(v)
        if enc["scheme"][0] == 2:
            chosen.add((int(enc["combos"][0][0]), int(enc["combos"][0][1])))
        else:
            n_rd += 1
    assert len(chosen) >= 60 and {(10, 10), (0, 0), (1, 0)} <= chosen, sorted(set(ALL_EF) - chosen)
    assert n_rd >= 100 and n_rd < values.size
    # mixtures
    cols, encs = mixtures
    alp = [enc for enc in encs if enc["scheme"][0] == 2]
    assert len(alp) >= 45
    assert sum(int(enc["k"][0]) > 1 for enc in alp) >= 40
    assert len({(int(enc["combos"][0][0]), int(enc["combos"][0][1])) for enc in alp}) >= 15
    widths = set().union(*[set(enc["bw"].tolist()) for enc in alp])
    assert set(range(33)) <= widths, sorted(set(range(33)) - widths)
    exc = np.concatenate([enc["exc_cnt"] for enc in alp])
    assert exc.max() == 1024 and exc.min() <= 2
    for seed, col, enc in zip(SEEDS, cols, encs):
        assert np.array_equal(of32.decode_column(enc).view(np.uint32), col.view(np.uint32)), f"mixture {seed}"


@pytest.fixture(scope="module")
def tail_sets(of32):
    sets = tail_threshold_sample_sets(of32)
    return sets, [of32.encode_column(column_of_samples(s)) for *_, s in sets]


def test_the_tail_sample_sets_sit_on_the_scheme_threshold(tail_sets):
    """by the reference's rule (32 * bits + 48 * exceptions >= 704 is ALP_RD): 21 bits / none and 20 bits / one exception are ALP under the set's own
    candidate, one bit or one exception more is ALP_RD — for every position of the minimum"""
    sets, encs = tail_sets
    assert len(sets) == 2 * 3 * 3 * 32
    for (cand, bits, n_exc, p, s), enc in zip(sets, encs):
        want_alp = 32 * bits + 48 * n_exc < 704
        what = f"candidate {cand}, {bits} bits, {n_exc} exceptions, minimum at {p}"
        assert (enc["scheme"][0] == 2) == want_alp, what
        if want_alp:
            assert int(enc["k"][0]) == 1 and (int(enc["combos"][0][0]), int(enc["combos"][0][1])) == cand, what


def test_tail_sample_sets_oracle_equals_reference(rf32, tail_sets):
    for (cand, bits, n_exc, p, s), enc in zip(*tail_sets):
        golden_io.assert_same_encoding(enc, rf32.encode_column(column_of_samples(s)), f"candidate {cand}, {bits} bits, {n_exc} exceptions, minimum at {p}", word=np.uint32)


def test_encode_and_decode_value_oracle_equals_reference(of32, rf32, values):
    import ctypes as C
    oe, re_ = of32.fn("encode_value", C.c_int32), rf32.fn("encode_value", C.c_int32)
    od, rd = of32.fn("decode_value", C.c_float), rf32.fn("decode_value", C.c_float)
    for v in values:
        cv = C.c_float(float(v))
        for e, f in ALL_EF:
            a, b = oe(cv, C.c_int(f), C.c_int(e)), re_(cv, C.c_uint8(f), C.c_uint8(e))
            assert a == b, f"encode_value({describe(v)}, e={e}, f={f}): oracle {a}, reference {b}"
            if f <= 9:
                x, y = od(C.c_int32(a), C.c_int(f), C.c_int(e)), rd(C.c_int32(a), C.c_uint8(f), C.c_uint8(e))
                assert np.float32(x).view(np.uint32) == np.float32(y).view(np.uint32), f"decode_value({a}, e={e}, f={f}) of {describe(v)}: oracle {x!r}, reference {y!r}"


def test_constant_vector_columns_oracle_equals_reference(rf32, values, constant_encodings):
    for v, enc in zip(values, constant_encodings):
        golden_io.assert_same_encoding(enc, rf32.encode_column(np.full(1024, v, np.float32)), f"boundary value {describe(v)}", word=np.uint32)


def test_mixtures_oracle_equals_reference(rf32, mixtures):
    for seed, col, enc in zip(SEEDS, *mixtures):
        golden_io.assert_same_encoding(enc, rf32.encode_column(col), f"boundary mixture {seed}", word=np.uint32)
