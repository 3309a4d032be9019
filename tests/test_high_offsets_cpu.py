"""No GPU: the placements of tests/high_offsets.py are what they claim to be.  For every placement of the small and of the long column, in both value types:
the shifts are aligned, the shifted records neither overlap nor leave the capacities, each seam lies on the byte of the record the table in high_offsets.py
names, and reading the records back through the shifted offsets from a sparse host model of the two streams (windows, not 4 GiB arrays) gives the oracle's
decode of the unshifted column.  The columns here are the ORACLE's encodings of the inputs; tests/test_high_offsets_gpu.py places the GPU encoder's, which
the encode suites pin to the same bytes."""
import functools

import numpy as np
import pytest

import high_offsets as ho
import layout
from alp_amd.capi import SCHEME_ALP, SCHEME_ALP_RD

TWO31, TWO32 = ho.TWO31, ho.TWO32


def oracle_for(dtype):
    from oracle.pyoracle import Oracle, OracleF32
    return Oracle() if dtype == "f64" else OracleF32()


@functools.lru_cache(maxsize=None)
def source(name, dtype):
    x = ho.small_input(dtype) if name == "small" else ho.long_input(dtype)
    W = 8 if dtype == "f64" else 4
    o = oracle_for(dtype)
    enc = o.encode_column(x)
    rg, vec, packed, exc = layout.compact(enc, W)
    src = ho.Source(name, dtype, x, rg, vec, packed, exc, ho.PLACEMENTS if name == "small" else ho.LONG_PLACEMENTS)
    src.decoded = o.decode_column(enc)
    assert np.array_equal(src.decoded.view(src.bits.dtype), src.bits), "the oracle's decode of the unshifted column is the input"
    return src


COLUMNS = ["small-f64", "small-f32", "long-f64", "long-f32"]
CASES = [f"{c}-{p}" for c in COLUMNS for p in (ho.PLACEMENTS if c.startswith("small") else ho.LONG_PLACEMENTS)]


@pytest.fixture(params=COLUMNS)
def src(request):
    return source(*request.param.split("-"))


@pytest.fixture(params=CASES)
def placed(request):
    """(the column, the placement's name), over every placement of every column"""
    column, dtype, name = request.param.split("-")
    return source(column, dtype), name


def test_the_small_column_has_the_vectors_the_placements_need(src):
    """a condition on the inputs: `inside` needs an ALP vector of 8 or more bits and an ALP record of two or more exceptions, `rd_left` an ALP_RD vector and an
    ALP_RD record with exceptions; most vectors of the mixed rowgroups carry several exceptions"""
    if src.name != "small":
        assert src.nv == ho.LONG_VECTORS and (src.vec["scheme"] == SCHEME_ALP).all() and src.vec["exc_cnt"].max() == 0 and src.vec["bw"].max() <= 16
        assert set(src.placements) == set(ho.LONG_PLACEMENTS)
        return
    v = src.vec
    assert set(src.placements) == set(ho.PLACEMENTS) and 400 <= src.nv <= 600
    assert (v["scheme"][:100] == SCHEME_ALP).all() and v["bw"][:100].max() <= 16, "one rowgroup of narrow decimals"
    assert (v["scheme"][100:300] == SCHEME_ALP).all() and (v["exc_cnt"][100:300] >= 2).mean() > 0.9, "two rowgroups whose vectors have several exceptions"
    assert (v["scheme"][300:] == SCHEME_ALP_RD).all() and (v["exc_cnt"][300:] > 0).any(), "two ALP_RD rowgroups"
    pl = src.placements
    m = pl["inside"].p_vector
    assert v["scheme"][m] == SCHEME_ALP and v["bw"][m] >= 8
    m = pl["inside"].e_vector
    assert v["scheme"][m] == SCHEME_ALP and v["exc_cnt"][m] >= 2
    m = pl["rd_left"].p_vector
    assert v["scheme"][m] == SCHEME_ALP_RD and v["lbw"][m] > 0 and v["bw"][m] > 0
    m = pl["rd_left"].e_vector
    assert v["scheme"][m] == SCHEME_ALP_RD and v["exc_cnt"][m] >= 3


def test_alignment_bounds_and_overlap(placed):
    src, name = placed
    pl = src.placements[name]
    assert pl.p_shift % 128 == 0 and pl.e_shift % 8 == 0 and pl.p_shift > 0 and pl.e_shift > 0
    vec = ho.place(src.rg, src.vec, src.packed, src.exc, src.W, pl.p_shift, pl.e_shift)
    for k in ("base", "bw", "e", "f", "lbw", "exc_cnt", "scheme"):
        assert np.array_equal(vec[k], src.vec[k]), "only the two offsets change"
    psz, esz = ho.sizes(vec, src.W)
    for off, sz, align, total in ((vec["packed_off"].astype(np.int64), psz, 128, src.packed.size), (vec["exc_off"].astype(np.int64), esz, 8, src.exc.size)):
        assert (off % align == 0).all()
        assert off.min() >= 0 and int((off + sz).max()) <= ho.CAPACITY, "inside the capacity"
        assert np.array_equal(off[1:], (off + sz)[:-1]), "contiguous, in vector order: no overlap and no gap"
        assert int(off[0]) + total == int((off + sz)[-1])
    # the twin copy of the small column lies above everything the placement touches
    if src.name == "small":
        ts = ho.twin_shift(name)
        assert max(pl.p_shift + src.packed.size, pl.e_shift + src.exc.size) <= ts and ts + max(src.packed.size, src.exc.size) <= ho.CAPACITY
        assert ts % 128 == 0 and ts not in (pl.p_shift, pl.e_shift)
        # under seam_2_31 every offset of the twin fits 32 bits too, under the others the twin lies above 2^32
        assert (TWO31 < ts and ts + max(src.packed.size, src.exc.size) < TWO32) if name == "seam_2_31" else ts > TWO32


def test_each_seam_lies_where_the_table_says(placed):
    src, name = placed
    pl = src.placements[name]
    W = src.W
    vec = ho.place(src.rg, src.vec, src.packed, src.exc, W, pl.p_shift, pl.e_shift)
    psz, esz = ho.sizes(vec, W)
    poff, eoff = vec["packed_off"].astype(np.int64), vec["exc_off"].astype(np.int64)
    bw, lbw, cnt, scheme = (vec[k].astype(np.int64) for k in ("bw", "lbw", "exc_cnt", "scheme"))
    seam = TWO31 if name == "seam_2_31" else TWO32
    assert pl.p_seam == seam and pl.e_seam == seam
    pv, ev = pl.p_vector, pl.e_vector
    has_exc = src.exc.size > 0
    if name in ("seam_2_31", "seam_2_32"):
        # packed: vector pv - 1's record ends on the seam (its last byte is seam - 1), vector pv's first byte is the seam; both have words
        assert pv >= 1 and psz[pv - 1] > 0 and psz[pv] > 0
        assert poff[pv - 1] + psz[pv - 1] == seam and poff[pv] == seam
        assert poff[0] < seam < poff[-1] + psz[-1], "records on both sides"
        if has_exc:  # exceptions: the nearest earlier record with bytes ends on the seam, record ev starts on it
            before = np.nonzero(esz[:ev] > 0)[0]
            assert before.size and esz[ev] > 0 and eoff[ev] == seam and eoff[before[-1]] + esz[before[-1]] == seam
            assert eoff[0] < seam < eoff[-1] + esz[-1]
        else:
            assert (eoff == seam).all()
    elif name == "inside":
        # packed: the seam is byte 128 * (bw // 2) of ALP vector pv's words: word-lane row bw // 2 starts on it, rows below it lie under 2^32
        assert scheme[pv] == SCHEME_ALP and bw[pv] >= 8 and pl.p_byte == 128 * (bw[pv] // 2)
        assert poff[pv] + pl.p_byte == seam and poff[pv] < seam < poff[pv] + psz[pv]
        # exceptions: record ev's values end on the seam (their last byte is seam - 1) and its positions start on it
        assert scheme[ev] == SCHEME_ALP and cnt[ev] >= 2 and pl.e_byte == W * cnt[ev]
        assert eoff[ev] + W * cnt[ev] == seam and eoff[ev] < seam < eoff[ev] + (W + 2) * cnt[ev]
    elif name == "rd_left":
        # packed: ALP_RD vector pv's right parts end on the seam, its left block (128 * lbw bytes) starts on it
        assert scheme[pv] == SCHEME_ALP_RD and lbw[pv] > 0 and pl.p_byte == 128 * bw[pv]
        assert poff[pv] + 128 * bw[pv] == seam and poff[pv] < seam and poff[pv] + psz[pv] == seam + 128 * lbw[pv]
        # exceptions: the seam lies strictly inside the positions [2c, 4c) of ALP_RD record ev
        assert scheme[ev] == SCHEME_ALP_RD and 2 * cnt[ev] < pl.e_byte < 4 * cnt[ev]
        assert eoff[ev] + pl.e_byte == seam
    else:
        assert poff[0] == seam and eoff[0] == seam and pl.p_shift == TWO32 and pl.e_shift == TWO32 and pv == 0 and ev == 0
    if name != "seam_2_31":
        assert poff[-1] + psz[-1] > TWO32, "something lies at or above 2^32"
    else:
        assert poff[-1] + psz[-1] < TWO32 and eoff[-1] + esz[-1] < TWO32, "seam_2_31 stays below 2^32: offsets that fit 32 bits"
    print(f"{src.name} {src.dtype} {name}: p_shift {pl.p_shift:#x} e_shift {pl.e_shift:#x}; packed seam {seam:#x} = byte {pl.p_byte} of vector {pv}'s record, "
          f"exception seam = byte {pl.e_byte} of vector {ev}'s record")


def test_reading_back_through_the_shifted_offsets_gives_the_oracles_decode(placed):
    src, name = placed
    pl = src.placements[name]
    vec = ho.place(src.rg, src.vec, src.packed, src.exc, src.W, pl.p_shift, pl.e_shift)
    packed, exc = ho.sparse_model(src.vec, src.packed, src.exc, pl)
    back = layout.expand(src.rg, vec, packed, exc, src.W)
    got = oracle_for(src.dtype).decode_column(back)
    assert np.array_equal(got.view(src.bits.dtype), src.decoded.view(src.bits.dtype))
    # ... and a 32-bit truncation of the offsets reads something else (zeros of the same model), unless the placement stays below 2^32
    low = vec.copy()
    low["packed_off"] &= np.uint64(0xFFFFFFFF)
    low["exc_off"] &= np.uint64(0xFFFFFFFF)
    if name == "seam_2_31":
        assert np.array_equal(low, vec)
    else:
        wrong = oracle_for(src.dtype).decode_column(layout.expand(src.rg, low, packed, exc, src.W))
        assert not np.array_equal(wrong.view(src.bits.dtype), src.bits), "truncated offsets would decode other bytes: the placement can tell"


def test_the_sparse_model_is_zero_outside_its_windows():
    s = ho.Sparse(1 << 40)
    s.put(TWO32 - 3, np.arange(1, 9, dtype=np.uint8))
    assert s[TWO32 - 5:TWO32 + 7].tolist() == [0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 0, 0]
    assert s[0:4].tolist() == [0, 0, 0, 0] and s[TWO32:TWO32 + 2].tolist() == [4, 5]
    with pytest.raises(AssertionError):
        s.put(TWO32, np.zeros(2, np.uint8))
