"""CPU: the inputs of the ALP_RD search tests (rd_search_inputs.py) and everything the GPU tests of tests/test_rd_search_gpu.py lean on.
(1) Floors, with the oracle alone: the columns reach every cut, dictionary size and left width, D (distinct left parts at the chosen cut) on both
    sides of every bucket count a column can reach, ties split by the dictionary's 8th place, vectors with none and with more than 256
    exceptions; every column is ALP_RD and decodes to its input bits.
(2) Oracle == reference where oracle/_ref is built (skipped otherwise): whole columns, rd_state_from_samples on every sample set at every cut,
    and the committed fixture against what the reference answers now.  The fixture against the oracle runs everywhere.
(3) The device's replay of libstdc++'s containers (alp_amd/csrc/rd_dictionary_order.hpp), compiled for the host, against the containers
    themselves (tests/cpp/rd_order_test.cpp), plain and under the address and undefined-behaviour sanitizers."""
import collections
import functools
import os
import subprocess

import numpy as np
import pytest

import golden_io
import rd_search_golden
import rd_search_inputs as inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = [64, 32]


def _oracle(bits):
    from oracle.pyoracle import Oracle, OracleF32
    return Oracle() if bits == 64 else OracleF32()


def _reference(bits):
    from oracle.pyoracle import Reference, ReferenceF32
    cls = Reference if bits == 64 else ReferenceF32
    if not cls.available():
        pytest.skip("oracle/_ref/libalp_ref.so not built (needs the reference's sources; run oracle/Makefile `ref`)")
    ref = cls()
    if not hasattr(ref.lib, ref.prefix + "rd_state_from_samples"):
        pytest.skip("oracle/_ref was built from an earlier shim, without rd_state_from_samples, and cannot be rebuilt here (oracle/Makefile `ref`)")
    return ref


@functools.lru_cache(maxsize=None)
def survey(bits):
    """per column of (a) to (c): the oracle's state of its (first) rowgroup, D, and a summary of its encoding"""
    orc = _oracle(bits)
    udt = inputs.types(bits)[1]
    out = {}
    for nm, col in inputs.columns(bits).items():
        st = orc.rd_state_from_samples(inputs.samples_of(col))
        enc = orc.encode_column(col)
        out[nm] = dict(cut=bits - st["rbw"], size=st["dict_size"], lbw=st["lbw"], D=st["sorted"].size, dict=set(int(x) for x in st["dict"][:st["dict_size"]]),
                       all_rd=bool((enc["scheme"] == 1).all()), exc_cnt=enc["exc_cnt"].copy(),
                       round_trip=np.array_equal(orc.decode_column(enc).view(udt), col.view(udt)),
                       same_state=(int(enc["bw"][0]), int(enc["lbw"][0]), int(enc["dict_size"][0])) == (st["rbw"], st["lbw"], st["dict_size"])
                       and np.array_equal(enc["dict"][0], st["dict"]))
    return out


@pytest.mark.parametrize("bits", BITS)
def test_columns_reach_every_cut_dictionary_size_and_left_width(bits):
    s = survey(bits).values()
    assert {x["cut"] for x in s} == set(range(1, 17))
    assert {x["size"] for x in s} == set(range(1, 9))
    assert {x["lbw"] for x in s} == {1, 2, 3}
    print(f"f{bits}: {len({(x['cut'], x['size'], x['lbw']) for x in s})} distinct (cut, size, left width) triples, largest D {max(x['D'] for x in s)}")


@pytest.mark.parametrize("bits", BITS)
def test_columns_reach_every_range_of_distinct_left_parts(bits):
    """D on both sides of the first rehash (13 / 14), of the sort's two forms (16 / 17) and of the rehashes at 29 / 30 and 59 / 60"""
    ds = {x["D"] for x in survey(bits).values()}
    for lo, hi in ((9, 13), (14, 16), (17, 29), (30, 59), (60, 124)):
        assert any(lo <= d <= hi for d in ds), (lo, hi, sorted(ds))
    assert {13, 14, 16, 17, 29, 30, 59, 60} <= ds, sorted(ds)
    for nm, x in survey(bits).items():  # (b): cut 16 wins and every singleton is a distinct left part
        if nm.startswith("distinct_k"):
            assert (x["cut"], x["D"]) == (16, 8 + int(nm.split("_")[1][1:])), (nm, x["cut"], x["D"])


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("t,c", inputs.TIES)
def test_tied_left_parts_are_split_by_the_dictionary_boundary(bits, t, c):
    split = 0
    for nv in inputs.TIE_VECTORS:
        x = survey(bits)[f"ties_t{t}_c{c}_v{nv}"]
        tied = set(int(p) for p in inputs.ties_parts(bits, t, c, nv)[1])
        assert x["cut"] == 16
        split += 0 < len(tied & x["dict"]) < len(tied)
    assert split >= 1


@pytest.mark.parametrize("bits", BITS)
def test_every_column_is_alp_rd_and_decodes_to_its_input(bits):
    s = survey(bits)
    assert all(x["all_rd"] for x in s.values()), [nm for nm, x in s.items() if not x["all_rd"]]
    assert all(x["round_trip"] for x in s.values()), [nm for nm, x in s.items() if not x["round_trip"]]
    assert all(x["same_state"] for x in s.values()), "rd_state_from_samples and the column encode disagree about a rowgroup"
    cnt = np.concatenate([x["exc_cnt"] for x in s.values()])
    assert cnt.max() > 256 and cnt.min() == 0
    for part in ("distinct_k", "ties_"):  # the wide exception record and the empty one also occur where the exception index takes all its forms
        c = np.concatenate([x["exc_cnt"] for nm, x in s.items() if nm.startswith(part)])
        assert c.max() > 256 and (part == "ties_" or c.min() == 0)


@pytest.mark.parametrize("bits", BITS)
def test_sample_sets_cover_the_rehashes_and_both_sort_forms(bits):
    """(d): D at cut 16 crosses 127 / 128 and 257 / 258 (the rehashes to 257 and 541 buckets) and reaches 288; sample counts below 32"""
    orc = _oracle(bits)
    ds = {orc.rd_state_from_samples(a, 16)["sorted"].size for a in inputs.synthetic_sample_sets(bits).values()}
    assert {1, 2, 17, 31, 32, 33, 64, 96, 255, 256, 287, 288} <= ds
    assert {a.size for a in inputs.sample_sets(bits).values()} == set(inputs.SAMPLE_SIZES)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_fixture_holds_the_built_sample_sets_and_the_oracle_agrees_with_it(bits):
    """tests/golden/rd_search_samples.npz (the REAL reference's answers, recorded): its samples are the generators' and the oracle gives the
    same cut, widths, dictionary, estimate and sorted list at every cut"""
    udt = inputs.types(bits)[1]
    fix = rd_search_golden.cases(bits)
    sets = inputs.synthetic_sample_sets(bits)
    assert list(fix) == list(sets)
    assert os.path.getsize(rd_search_golden.PATH) < (1 << 20)
    orc = _oracle(bits)
    for nm, (smp, answers) in fix.items():
        assert np.array_equal(smp.view(udt), sets[nm].view(udt)), nm
        for cut, want in enumerate(answers):
            assert rd_search_golden.same_answer(orc.rd_state_from_samples(smp, cut), want), (nm, cut)
        ests = [a["estimate"] for a in answers[1:]]
        assert answers[0]["rbw"] == bits - (1 + int(np.argmin(ests))), "the first strictly smallest estimate wins"


def test_fixture_is_what_the_reference_answers_now():
    got = rd_search_golden.record({64: _reference(64), 32: _reference(32)})
    z = np.load(rd_search_golden.PATH)
    assert sorted(z.files) == sorted(got)
    for k in got:
        assert np.array_equal(z[k], got[k]), k


# ---- oracle == reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", BITS)
def test_columns_oracle_equals_reference(bits):
    orc, ref = _oracle(bits), _reference(bits)
    for nm, col in inputs.columns(bits).items():
        golden_io.assert_same_encoding(orc.encode_column(col), ref.encode_column(col), nm, word=inputs.types(bits)[1])


@pytest.mark.parametrize("bits", BITS)
def test_rd_state_from_samples_oracle_equals_reference(bits):
    orc, ref = _oracle(bits), _reference(bits)
    for nm, smp in inputs.sample_sets(bits).items():
        for cut in range(17):
            assert rd_search_golden.same_answer(orc.rd_state_from_samples(smp, cut), ref.rd_state_from_samples(smp, cut)), (nm, cut)


# ---- the device's replay against the real containers ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _order_rows():
    """one row per (sample set of (d), cut, precision): 'D key count ..' in order of first occurrence"""
    rows = []
    for bits in BITS:
        for smp in inputs.sample_sets(bits).values():
            for cut in range(1, 17):
                kc = inputs.first_occurrence_counts(smp, cut)
                rows.append(" ".join([str(len(kc))] + [f"{k} {c}" for k, c in kc]))
    return rows


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_device_replay_gives_the_order_of_the_real_containers(tmp_path, sanitize):
    """rd_reference_order (one lane of k_rowgroup_init runs it, through unguarded loops) compiled for the host, against std::unordered_map +
    std::sort on every sample set of (d) at every cut: the same order, and under -fsanitize=address,undefined not one report."""
    exe = tmp_path / "rd_order_test"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, f"-I{ROOT}/alp_amd/csrc", "-o", str(exe), f"{ROOT}/tests/cpp/rd_order_test.cpp"])
    rows = _order_rows()
    p = subprocess.run([str(exe)], input="\n".join(rows) + "\n", capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stderr == "", p.stderr[-3000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 2 * len(rows) + 1 and lines[-1].startswith("heap_sorts ")
    sizes = collections.Counter()
    for i, row in enumerate(rows):
        a, b = lines[2 * i].split(), lines[2 * i + 1].split()
        assert a[0] == "replay" and b[0] == "std" and len(a) == 1 + int(row.split()[0])
        assert a[1:] == b[1:], f"row {i} (D = {row.split()[0]}): the replay's order differs from the containers'"
        sizes[len(a) - 1] += 1
    assert max(sizes) == 288 and min(sizes) == 1  # (288 insertions pass every rehash up to 541 buckets)
    assert int(lines[-1].split()[1]) >= 8, "the median-of-three adversary (rd_search_inputs.heap_sort_left_parts) reaches the heap-sort fallback at cut 16, both precisions, four sample counts"
    print(f"{len(rows)} orders identical, D = {min(sizes)}..{max(sizes)}; {lines[-1]}")
