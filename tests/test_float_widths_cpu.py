"""CPU: the inputs of tests/test_float_widths_gpu.py are what that suite says they are — the float column of every packed width (datagen), the hand-built
float vectors and the arena-straddling column (float_rows.py).  Only the oracle, datagen and the builder are imported: no GPU, no built library.  These
properties are what keeps the GPU comparisons from going vacuous after an edit of a generator."""
import numpy as np
import pytest

import datagen
import float_rows as fr


@pytest.fixture(scope="module")
def of32():
    from oracle.pyoracle import OracleF32
    return OracleF32()


@pytest.mark.parametrize("exceptions", [False, True])
@pytest.mark.parametrize("n_vectors,seed", [(200, 77), (233, 10)])
def test_every_bit_width_column_f32_is_what_it_says(of32, exceptions, n_vectors, seed):
    col = datagen.every_bit_width_column_f32(n_vectors, seed, exceptions)
    assert col.dtype == np.float32 and col.size == n_vectors * 1024
    enc = of32.encode_column(col)
    assert (enc["scheme"] == 2).all(), "every rowgroup must stay ALP"
    assert (enc["k"] == 1).all() and (enc["e"] == 0).all() and (enc["f"] == 0).all()
    assert (enc["combos"][:, :2] == 0).all()
    assert sorted(set(enc["bw"].tolist())) == list(range(33))
    v = np.arange(n_vectors)
    sampled = (v % 100) % 12 == 0
    assert np.array_equal(enc["bw"][~sampled], (v % 33)[~sampled].astype(np.uint8)), "every vector outside the sampled ones has the width it aims at"
    if not exceptions:
        assert int(enc["exc_cnt"].max()) == 0
    else:
        assert int(enc["exc_cnt"][sampled].max()) == 0
        for c in range(3):  # the third that carries exceptions moves with the period of 33: every residue of the vector index gets its turn
            assert (enc["exc_cnt"][v % 3 == c] > 0).any(), c
        assert len(set(enc["bw"][enc["exc_cnt"] > 0].tolist())) >= 30, "(nearly) every width has a vector with exceptions"
        kinds = col[np.isnan(col) | (col == np.float32(0.5)) | (col == np.float32(1e30))]
        assert np.isnan(kinds).any() and (kinds == np.float32(0.5)).any() and np.signbit(col[col == 0]).any()
    assert np.array_equal(of32.decode_column(enc).view(np.uint32), col.view(np.uint32))


def test_alp_rows_reach_both_sides_of_the_shortcut_rule_at_every_width(of32):
    enc = fr.alp_rows()
    n = enc["bw"].size
    assert n % 100 == 0 and enc["base"].dtype == np.int64 and enc["packed"].dtype == np.int32
    bw, f, e, base = enc["bw"].astype(int), enc["f"].astype(int), enc["e"].astype(int), enc["base"]
    assert set(bw.tolist()) == set(range(33)) and set(f.tolist()) == set(range(11))
    assert (e >= f).all() and (e <= 10).all() and (e - f <= 2).all()
    assert all(((e - f) == d).any() for d in (0, 1, 2))
    assert (base >= fr.INT32_MIN).all() and (base <= fr.INT32_MAX).all()
    mask = (1 << bw.astype(np.int64)) - 1
    bnd = np.array(fr.SHORTCUT_BOUND, np.int64)[f]
    sc = np.array([fr.shortcut_applies(int(b), int(ff), int(x)) for b, ff, x in zip(bw, f, base)])
    assert np.array_equal(sc, (bw <= 24) & (base >= -bnd) & (base + mask <= bnd))
    assert 500 <= int(sc.sum()) <= n - 500
    for ff in range(10):
        for b in range(25):
            rows = (f == ff) & (bw == b)
            assert (~sc[rows]).any(), (ff, b)
            if (1 << b) - 1 <= 2 * fr.SHORTCUT_BOUND[ff]:  # some base fits the width between the two bounds
                assert sc[rows].any(), (ff, b)
        at = f == ff
        for what, hit in (("base == -bnd", base == -bnd), ("base == -bnd - 1", base == -bnd - 1), ("base + mask == bnd", base + mask == bnd),
                          ("base + mask == bnd + 1", base + mask == bnd + 1)):
            assert (at & hit).any(), (ff, what)
        # on the bounds themselves the two outcomes differ by that one step, at a width the rule admits
        assert (sc & at & (base == -bnd)).any() and (~sc & at & (base == -bnd - 1) & (bw <= 24)).any(), ff
        assert (sc & at & (base + mask == bnd)).any() and (~sc & at & (base + mask == bnd + 1) & (bw <= 24) & (base >= -bnd)).any(), ff
    assert not sc[f == 10][bw[f == 10] > 0].any()
    # both extreme digits are in every row outside its exception positions (a bound only bites where base + 0 or base + mask occurs)
    for v in range(n):
        if enc["exc_cnt"][v] < 1024 and bw[v] > 0:
            digits = of32.unffor_u32(enc["packed"][v], int(bw[v]), 0)
            keep = np.ones(1024, bool)
            keep[enc["pos"][v, : int(enc["exc_cnt"][v])]] = False
            assert (digits[keep] == 0).any() and (digits[keep] == np.uint32(mask[v])).any(), v
    assert (base + mask > fr.INT32_MAX).any(), "a base whose base + mask wraps int32"
    assert set(enc["exc_cnt"].tolist()) == set(fr.ALP_EXC_COUNTS)
    for c in (257, 1024):
        assert ((enc["exc_cnt"] == c) & sc).any() and ((enc["exc_cnt"] == c) & ~sc).any(), c
        # the sinks' branch past the 256-entry stage says something only where those values are finite and moderate: a NaN or an overflow in the sum,
        # or a value outside every count's bounds, would hide which source they were read from
        moderate = [v for v in np.nonzero(enc["exc_cnt"] == c)[0] if (np.abs(enc["exc"][v, :c].astype(np.float64)) < 1e6).all()]
        assert len(moderate) >= 10, c
        assert all((enc["exc"][v, 256:c] != 0).all() for v in moderate), c
    pos = enc["pos"].astype(int)
    for v in range(n):
        c = int(enc["exc_cnt"][v])
        assert (np.diff(pos[v, :c]) > 0).all() and (c == 0 or pos[v, c - 1] < 1024)
    # exception values: NaNs of both kinds somewhere, and finite values only in at least half of the vectors with exceptions
    bits = np.concatenate([enc["exc"][v].view(np.uint32)[: int(enc["exc_cnt"][v])] for v in range(n)])
    is_nan = ((bits >> 23) & 0xFF == 0xFF) & (bits & 0x7FFFFF != 0)
    assert (is_nan & (bits & 0x400000 != 0)).any() and (is_nan & (bits & 0x400000 == 0)).any()
    with_exc = np.nonzero(enc["exc_cnt"] > 0)[0]
    finite_only = [np.isfinite(enc["exc"][v, : int(enc["exc_cnt"][v])]).all() for v in with_exc]
    assert 2 * sum(finite_only) >= with_exc.size
    out = of32.decode_column(enc)  # the oracle takes every row
    assert out.size == n * 1024


def test_a_width_of_25_passes_the_bounds_only_where_the_shortcut_is_exact_anyway():
    """`bw <= 24` in the rule is implied by its two bounds except at width 25 with base -2^24 or 1 - 2^24 (f <= 2): rows of that kind are here, and
    there every base + digit still lies in [-2^24, 2^24], where (float)(int32) is exact and the shortcut's product is the literal path's — the GPU tests
    cannot tell `<= 24` from `<= 25`, and need not"""
    enc = fr.alp_rows()
    bw, f, base = enc["bw"].astype(int), enc["f"].astype(int), enc["base"]
    bnd = np.array(fr.SHORTCUT_BOUND, np.int64)[f]
    rows = (bw == 25) & (base >= -bnd) & (base + (2**25 - 1) <= bnd)
    assert rows.sum() >= 3 and set(f[rows].tolist()) == {0, 1, 2}
    assert set(base[rows].tolist()) <= {-2**24, 1 - 2**24}
    assert not ((bw > 25) & (base >= -bnd) & (base + ((1 << bw.astype(np.int64)) - 1) <= bnd)).any()


def test_rd_rows_are_cuts_the_reference_can_produce(of32):
    from oracle.pyoracle import Oracle
    o16 = Oracle()
    enc = fr.rd_rows()
    n = enc["bw"].size
    assert (enc["scheme"] == 1).all() and n == 100 * len(fr.rd_cuts())
    assert set(enc["bw"].tolist()) == set(range(16, 32)) and set(enc["lbw"].tolist()) == {1, 2, 3}
    assert set(enc["exc_cnt"].tolist()) == set(fr.RD_EXC_COUNTS)
    for r in range(n // 100):
        rows = slice(100 * r, 100 * r + 100)
        rbw, lbw, size = int(enc["bw"][100 * r]), int(enc["lbw"][100 * r]), int(enc["dict_size"][r])
        assert (enc["bw"][rows] == rbw).all() and (enc["lbw"][rows] == lbw).all(), "one cut per rowgroup"
        assert max(1, int(np.ceil(np.log2(size)))) == lbw and len(set(enc["dict"][r, :size].tolist())) == size
        assert int(enc["dict"][r].max()) < 2 ** (32 - rbw)
        for v in (100 * r, 100 * r + 57):
            assert int(o16.unffor_u16(enc["packed_left"][v], lbw).max()) < size, "left indices stay below the dictionary size"
            c = int(enc["exc_cnt"][v])
            assert (np.diff(enc["pos"][v, :c].astype(int)) > 0).all()
            assert c == 0 or int(enc["exc"][v].view(np.uint16)[:c].max()) < 2 ** (32 - rbw)
    assert of32.decode_column(enc).size == n * 1024


def test_the_builders_bit_packing_is_the_oracles(of32):
    from oracle.pyoracle import Oracle
    o16 = Oracle()
    rng = np.random.default_rng(2)
    for bw in range(33):
        vals = rng.integers(0, 2**bw, 1024, dtype=np.uint64).astype(np.uint32)
        assert np.array_equal(fr.pack_u32(vals, bw).view(np.uint32), of32.ffor_u32(vals, bw)[: 32 * bw]), bw
    for bw in (1, 2, 3):
        vals = rng.integers(0, 1 << bw, 1024).astype(np.uint16)
        assert np.array_equal(fr.pack_u16(vals, bw), o16.ffor_u16(vals, bw)[: 64 * bw])


def test_arena_column_has_a_chunk_on_either_side_of_every_arena(of32):
    enc, where, skewed = fr.arena_column()
    assert (enc["scheme"] == 2).all() and enc["bw"].size % 100 == 0
    pk, rec = fr.record_bytes(enc)
    exc_off = np.concatenate([[0], np.cumsum(rec)])
    seen = set()
    for start, c, arena, kind, over in where:
        assert start % fr.RUN_ALIGN == 0 and start % c == 0, "the run starts a chunk of its shape"
        rows = slice(start, start + c)
        need = fr.chunk_footprint(pk[rows], rec[rows], skew=int(exc_off[start]) & 15)
        if over:
            assert arena < need <= arena + 128, (start, c, arena, kind, need)
        else:
            assert arena - 128 < need <= arena, (start, c, arena, kind, need)
        if kind == "narrow":
            assert (enc["bw"][rows] <= 2).all() and int(rec[rows].sum()) > 2 * int(pk[rows].sum())
        else:
            assert int(enc["exc_cnt"][rows].max()) == 0 and int(enc["bw"][rows].min()) >= 7  # (an arena of 1 KiB per vector: 8 bits is as wide as its chunk gets)
        seen.add((c, arena, kind, over))
    assert seen == {(c, arena, kind, over) for c, arena in fr.STREAM_SHAPES for kind in ("narrow", "wide") for over in (False, True)}
    assert {a for _, a in fr.STREAM_SHAPES} == {8192, 12288, 14336, 16384, 24576, 49152}
    # the run whose records start 8 modulo 16 (the flat copy starts at the 16-byte boundary below: rec_skew = 8), and it still fits its arena
    assert skewed in [s for s, *_ in where] and int(exc_off[skewed]) % 16 == 8 and int(enc["exc_cnt"][skewed]) > 0
    assert of32.decode_column(enc).size == enc["bw"].size * 1024


def test_blocks_for_the_streaming_rule():
    """what the rule's test tiles: exception-free blocks of one width, a block with 20 exceptions per vector, and the mixed block whose average stays inside the
    rule (decode_policy.hpp: more than 1.5 and at most 8.5 packed bits per value, fewer than 16 bytes of exception record per vector)"""
    for bw in range(1, 10):
        b = fr.uniform_block(bw)
        assert (b["bw"] == bw).all() and int(b["exc_cnt"].max()) == 0 and b["bw"].size == 100
        sc = [fr.shortcut_applies(bw, int(f), int(x)) for f, x in zip(b["f"], b["base"])]
        assert any(sc) and not all(sc)
    assert (fr.uniform_block(3, exc_cnt=20)["exc_cnt"] == 20).all()
    m = fr.mixed_width_block()
    assert 1.5 < m["bw"].mean() <= 8.5 and int(m["exc_cnt"].max()) == 0 and m["bw"].size % 100 == 0
    wide = (m["bw"] == 32).astype(int)
    runs = np.nonzero(np.diff(np.concatenate([[0], wide, [0]])) == 1)[0]
    assert runs.size >= 5 and len({int(r) % 12 for r in runs}) >= 5, "runs of twelve 32-bit vectors at several phases of the chunk of twelve"
    for r in runs:
        assert wide[r:r + 12].all()
        # twelve such vectors alone outgrow the default streamed shape's arena (24576 bytes), whatever the chunk's phase
    assert 12 * 32 * 128 > 24576
