"""CPU: the store decode's launch rule (alp_amd/csrc/decode_policy.hpp) held directly, without a GPU.  The header is plain host-and-device C++: tests/cpp/
decode_policy_test.cpp includes it, is compiled with g++ and prints, per row of inputs, the debug word of alpgpu_debug_decode_plan, the vectors per workgroup, whether
the read-ahead runs, the kind of the stretch (region plans), the unhinted decode's choice and the read-ahead's pace.
(a) The lie matrix of tests/test_decode_planning_gpu.py (decode_lies.py): every lie selects the arm the GPU test then launches, with the read-ahead left to the
    library, off and forced on.
(b) tests/golden/decode_plan_sweep.txt: inputs on and beside every threshold of the rule, every arm, forced shapes and pads, with what the rule answered BEFORE it was
    gathered into decode_policy.hpp (recorded from that commit's functions): the rule reproduces every row exactly."""
import os
import subprocess

import pytest

from decode_lies import LIES_F32, LIES_F64, TILED_VECTORS, lie_hints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEP = os.path.join(ROOT, "tests", "golden", "decode_plan_sweep.txt")
OUT_FIELDS = ("debug_word", "vectors_per_wg", "reads_ahead", "stretch_kind", "unhinted_shape", "unhinted_ahead", "lead_min", "lead_max", "ps_per_vector")


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    exe = tmp_path_factory.mktemp("decode_policy") / "decode_policy_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-I{ROOT}/alp_amd/csrc", "-o", str(exe),
                           f"{ROOT}/tests/cpp/decode_policy_test.cpp"])

    def run(rows):
        """rows of 13 inputs (decode_policy_test.cpp) -> one dict of OUT_FIELDS per row"""
        text = "".join(" ".join(str(int(x)) for x in r) + "\n" for r in rows)
        p = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stderr[-2000:]
        out = [dict(zip(OUT_FIELDS, (int(x) for x in line.split()))) for line in p.stdout.splitlines()]
        assert len(out) == len(rows)
        return out
    return run


def _row(vb, n, hints, ra):
    packed, exc, rd_hint = hints
    return (vb, n, packed, exc, rd_hint, exc // (vb + 2), 100 * (rd_hint - 1), 0, -1, ra, 0, 0, 0)


@pytest.mark.parametrize("n", [TILED_VECTORS, 66000])  # (66 000: what the GPU test's battery of 500 vectors tiles to)
def test_every_lie_selects_its_arm(rule, n):
    cases = [(8, lie, ra) for lie in LIES_F64 for ra in (-1, 0, 1)] + [(4, lie, ra) for lie in LIES_F32 for ra in (-1, 0, 1)]
    got = rule([_row(vb, n, lie_hints(n, *(LIES_F64 if vb == 8 else LIES_F32)[lie][0]), ra) for vb, lie, ra in cases])
    for (vb, lie, ra), g in zip(cases, got):
        word = g["debug_word"]
        if vb == 8:  # the word as capi.Context.decode_plan reads it
            vpw, many, pad = LIES_F64[lie][1]
            assert ((1 if word & 1 else 2), bool(word & 64), word >> 8) == (vpw, many, pad), (lie, ra, g)
            assert g["vectors_per_wg"] == vpw
            assert g["reads_ahead"] == (ra == 1), (lie, ra)  # (too short for the library's own read-ahead)
        else:
            shape = LIES_F32[lie][1]
            assert word & 0xFF == shape and word >> 8 == 0xFF, (lie, ra, g)
            assert g["vectors_per_wg"] == shape
            assert g["reads_ahead"] == (ra == 1 and shape < 16), (lie, ra)


def test_the_rule_reproduces_the_recorded_sweep(rule):
    rows, want = [], []
    for line in open(SWEEP):
        if line.startswith("#") or not line.strip():
            continue
        inputs, outputs = line.split("|")
        rows.append(tuple(int(x) for x in inputs.split()))
        want.append(dict(zip(OUT_FIELDS, (int(x) for x in outputs.split()))))
    assert len(rows) > 2000 and {r[0] for r in rows} == {8, 4}
    got = rule(rows)
    bad = [(r, w, g) for r, w, g in zip(rows, want, got) if w != g]
    assert not bad, (len(bad), bad[:5])
