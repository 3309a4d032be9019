"""CPU: the rules that decide whether bytes from outside may reach the decode kernels (alp_amd/csrc/blob_check.hpp: the blob header, one descriptor, the chunk
windows) on every bound of every field, against the same rules in Python integers (tests/blob_replica.py).  tests/cpp/blob_check_test.cpp includes the header
under g++, reads each case of tests/blob_cases.py into a heap buffer of exactly `size` bytes and prints verdict, rule and first bad vector; every line must be the
replica's.  The program is built twice, plainly and with -fsanitize=address,undefined: in the second a read one byte past a case's buffer, or an
arithmetic step the language leaves undefined, ends the run.  Nothing is loaded into Python.

The header rule of the commit before this file did its arithmetic in uint64_t and wrapped; parent_header_rule below is that rule with the wrap written out, and
test_the_wrap_family_passed_the_rule_before names the headers it let through."""
import os
import struct
import subprocess

import pytest

import blob_cases as bc
import blob_replica as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2**64 - 1


@pytest.fixture(scope="module")
def bases(oracle):
    from oracle.pyoracle import OracleF32
    return {"f64": bc.base_f64(oracle), "f32": bc.base_f32(OracleF32())}


@pytest.fixture(scope="module")
def all_cases(bases):
    out = []
    for b in bases.values():
        out += bc.cases(b) + bc.window_cases(b)
    for rows in (bc.rows_f64(), bc.rows_f32()):
        out.append(bc.Case(rows, "hand-built rows", None, lambda p: None, "rows"))
        out.append(bc.Case(rows, "hand-built rows, chunks of 4", None, lambda p: None, "rows", chunk=bc.CHUNK))
    return out


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("blob_check")
    common = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT}/alp_amd/csrc", f"{ROOT}/tests/cpp/blob_check_test.cpp"]
    subprocess.check_call(common + ["-o", str(d / "plain")])
    subprocess.check_call(common + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(d / "sanitized")])
    return d


@pytest.fixture(scope="module")
def results(all_cases, programs):
    """every case built once: the replica's verdict, and the line each build of the program prints for it"""
    procs, outs = {}, {}
    for name in ("plain", "sanitized"):
        outs[name] = open(programs / (name + ".out"), "w+")
        procs[name] = subprocess.Popen([str(programs / name)], stdin=subprocess.PIPE, stdout=outs[name], stderr=open(programs / (name + ".err"), "w"))
    verdicts = []
    for c in all_cases:
        blob, size, _ = c.build()
        verdicts.append(br.check_blob(blob, size, c.vb, c.chunk, c.ranges))
        ranges = [] if c.chunk is None else (c.ranges if c.ranges is not None else [(0, struct.unpack_from("<Q", blob, 24)[0])])
        head = struct.pack("<4Q", size, c.vb, c.chunk or 0, len(ranges)) + b"".join(struct.pack("<2Q", *r) for r in ranges)
        for p in procs.values():
            if p.poll() is None:
                try:
                    p.stdin.write(head)
                    p.stdin.write(blob[:size].tobytes())
                except BrokenPipeError:
                    pass
    lines = {}
    for name, p in procs.items():
        try:
            p.stdin.close()
        except BrokenPipeError:
            pass
        rc = p.wait(timeout=300)
        outs[name].seek(0)
        lines[name] = (rc, outs[name].read().splitlines(), open(programs / (name + ".err")).read()[-3000:])
        outs[name].close()
    return verdicts, lines


def test_base_columns_hold_what_the_cases_need(bases):
    for b in bases.values():
        vec, rg = b.vec, b.rg
        assert b.n == 258 and b.n_values == 258 * 1024 - 7
        assert list(rg["scheme"]) == [bc.ALP, bc.RD, bc.ALP]
        assert (vec["scheme"][:100] == bc.ALP).all() and (vec["scheme"][100:200] == bc.RD).all() and (vec["scheme"][200:] == bc.ALP).all()
        for v in bc.NAMED:  # an ALP and an ALP_RD vector with exceptions at every named index
            assert vec[v]["exc_cnt"] > 0, (b.name, v)
        alp_counts = {int(vec[v]["exc_cnt"]) % 2 for v in bc.NAMED if vec[v]["scheme"] == bc.ALP}
        rd_counts = {int(c) % 2 for c in vec["exc_cnt"][100:200] if c > 0}
        assert alp_counts == {0, 1} and rd_counts == {0, 1}, "odd and even exception counts of both schemes"
        assert (vec["bw"][vec["scheme"] == bc.ALP] > 0).all() and int(vec["bw"].max()) < 8 * b.vb - 1  # records that are not empty, widths with room to grow
        assert 1 <= int(rg["rd_lbw"][1]) <= 3 and int(rg["rd_rbw"][1]) >= 1


def test_build_blob_of_the_base_columns_is_accepted(bases):
    for b in list(bases.values()) + [bc.rows_f64(), bc.rows_f32()]:
        assert br.check_blob(b.blob, b.blob.size, b.vb).ok, b.name
        assert br.check_blob(b.blob, b.blob.size, b.vb, chunk=bc.CHUNK).ok, b.name
        assert br.check_column(b.rg, b.vec, b.exc, b.packed.size, b.exc.size, b.vb).ok, b.name
        assert b.blob.size == 64 + 32 * b.rg.size + 32 * b.vec.size + br.align8(b.packed.size) + b.exc.size
    rows = bc.rows_f64()
    assert set(range(65)) <= set(rows.vec["bw"][rows.vec["scheme"] == bc.ALP].tolist()) and {1, 1024} <= set(rows.vec["exc_cnt"].tolist())
    assert set(range(48, 64)) <= set(rows.vec["bw"][rows.vec["scheme"] == bc.RD].tolist())


def test_every_case_crosses_its_own_rule_and_no_other(all_cases, results):
    """a mutation that is refused for another reason than the one it was written for hides a hole"""
    verdicts, _ = results
    wrong = []
    for c, got in zip(all_cases, verdicts):
        if c.rule == bc.LIE:
            continue
        want = frozenset() if c.rule is None else frozenset({c.rule})
        if got.rules != want or (c.rule not in (None, "header") and got.first_bad != c.bad):
            wrong.append((c.name, c.rule, c.bad, repr(got)))
    assert not wrong, (len(wrong), wrong[:10])
    names = [c.name for c in all_cases]
    assert len(set(names)) == len(names)
    for rule in br.RULES:  # every rule is crossed, and every kind of case has accepted members
        assert any(c.rule == rule for c in all_cases), rule
    for kind in ("header", "descriptor", "position", "unused", "window", "rows"):
        assert any(c.kind == kind and c.rule is None for c in all_cases), kind


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_the_rules_agree_with_the_replica(all_cases, results, build):
    verdicts, lines = results
    rc, got, err = lines[build]
    assert rc == 0, (rc, len(got), all_cases[len(got)].name if len(got) < len(all_cases) else None, err)
    assert len(got) == len(all_cases)
    wrong = [(c.name, line, v.line()) for c, v, line in zip(all_cases, verdicts, got) if line != v.line()]
    assert not wrong, (len(wrong), wrong[:10])


# ---- the header rule as it stood before: uint64_t arithmetic, written out with its wrap ---------------------------------------------------------------
def parent_header_rule(blob, size, value_bytes):
    if size < 64:
        return False
    magic, version, header_bytes, n_values, n, nrg, pb, eb, reserved = br.HEADER.unpack_from(blob, 0)
    if magic != b"ALPGPU1\0" or version != 1 or header_bytes != 64 or (8 if reserved == 0 else reserved) != value_bytes:
        return False
    if nrg != ((n + 99) & M64) // 100 or n_values > (n * 1024) & M64 or (n and (n_values + 1024) & M64 <= (n * 1024) & M64):
        return False
    need = (64 + 32 * (((n + 99) & M64) // 100) + 32 * n + ((pb + 7) & M64 & ~7) + ((eb + 7) & M64 & ~7)) & M64
    return not (pb > 2**56 or eb > 2**56 or size < need)


def test_the_wrap_family_passed_the_rule_before(all_cases):
    """which header cases the rule before this file accepted although the replica refuses them.  The quoted header, at both sizes: 32 * n_rowgroups +
    32 * n_vectors = 2^64, so the blob's size came out as 64 and the descriptor scan then read ~1.8e17 bytes past the buffer.  And n_vectors = 2^64 - 99
    with the base blob's size: n_vectors + 99 wrapped to 0 rowgroups, n_vectors * 1024 wrapped to the n_values given, and 32 * n_vectors wrapped to -3168,
    which made the blob's size come out BELOW the base blob's.  The rest of the family (n_vectors = 2^54, 2^64 - 1, and 2^64 - 99 in 64 bytes) passed one
    wrapped check and happened to be caught by a later one."""
    let_through = []
    for c in all_cases:
        if c.kind != "header" or c.rule != "header":
            continue
        blob, size, _ = c.build()
        assert not br.check_blob(blob, size, c.vb).ok
        if parent_header_rule(blob, size, c.vb):
            let_through.append(c.name.split(":", 1)[1])
    assert sorted(set(let_through)) == ["wrap 32*nrg+32*n=2^64, size 64", "wrap 32*nrg+32*n=2^64, size exact", "wrap n=2^64-99, size exact"]


def test_shard_ranges_are_whole_rowgroups():
    assert br.shard_ranges(258, 2) == [(0, 200), (200, 258)] and br.shard_ranges(258, 3) == [(0, 100), (100, 200), (200, 258)]
    assert br.shard_ranges(258, 4) == [(0, 100), (100, 200), (200, 258), (258, 258)] and br.shard_ranges(0, 2) == [(0, 0), (0, 0)]
