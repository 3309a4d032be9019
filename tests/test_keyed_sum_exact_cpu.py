"""CPU: the exact keyed SUM (include/alpgpu.h, "exact keyed SUM") is exported and declared; a NULL context is refused with ALPGPU_ERR_INVALID before the
HIP runtime is touched, so this runs without a device; the table-bytes function is monotone and refuses what the calls refuse; the Python wrappers
refuse what the family's refuse before any launch.  alp_amd/csrc/exact_sum.hpp (the split of a double, the limbs, the one rounding) is compiled into a
stand-alone host program under AddressSanitizer and UndefinedBehaviorSanitizer (tests/cpp/exact_sum_host.cpp) and held, bit for bit, to
tests/keyed_exact_replica.py, whose sums are Python integers rounded by int / int.  Everything but the replica's own test needs the feature."""
import ctypes
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import keyed_exact_replica as replica

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alpgpu_decode_keyed_exact_sum_f64", "alpgpu_decode_keyed_exact_sum_f32", "alpgpu_debug_decode_keyed_exact_sum_f64", "alpgpu_debug_decode_keyed_exact_sum_f32",
         "alpgpu_keyed_exact_sum_table_bytes")
NAN, INF = float("nan"), float("inf")
DBL_MAX, TINY, MIN_NORMAL = 1.7976931348623157e308, 5e-324, 2.2250738585072014e-308
U64_MAX = 2**64 - 1


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_library_exports_the_exact_keyed_sum_entry_points():
    from alp_amd import capi
    for n in NAMES:
        assert hasattr(capi.lib, n), n
    assert capi.lib.alpgpu_abi_version() == 3  # the section only adds symbols
    assert capi.KEYED_EXACT_VECTORS_MAX == 1 << 21 and capi.KEYED_MANY_KEYS_MAX == 1 << 20
    for m in ("keyed_sum_exact", "keyed_sum_exact_into", "keyed_sum_exact_table"):
        assert callable(getattr(capi.Context, m))
    assert not hasattr(capi.lib, "alpgpu_decode_keyed_sum_f32"), "the striped keyed SUM stays double only"


def test_the_header_declares_them(tmp_path):
    src = tmp_path / "keyed_sum_exact_decls.c"
    text = ('#include "alpgpu.h"\n_Static_assert(ALPGPU_KEYED_EXACT_VECTORS_MAX == 2097152u, "2^21 vectors are 2^31 rows");\n'
            'uint64_t (*tb)(uint32_t) = alpgpu_keyed_exact_sum_table_bytes;\n')
    for i, (sfx, t) in enumerate((("f64", "double"), ("f32", "float"))):
        text += ('int (*f%d)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_%s*, const %s*, uint32_t, double*, uint64_t*, void*, int)\n'
                 '    = alpgpu_decode_keyed_exact_sum_%s;\n' % (i, sfx, t, sfx))
        text += ('int (*d%d)(alpgpu_ctx*, const alpgpu_column*, const alpgpu_column*, const uint64_t*, const alpgpu_zone_%s*, const %s*, uint32_t, double*, uint64_t*, void*, int,\n'
                 '          const alpgpu_keyed_tuning*, uint64_t*) = alpgpu_debug_decode_keyed_exact_sum_%s;\n' % (i, sfx, t, sfx))
    src.write_text(text)
    p = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", f"-I{ROOT}/include", str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def test_the_three_lists_name_the_new_call_and_the_striped_sum_keeps_its_bound():
    for name in ("README.md", "DESIGN.md", "include/alpgpu.h", "INTEGRATION.md"):
        with open(os.path.join(ROOT, name)) as f:
            text = f.read()
        assert "keyed_sum_exact" in text, name
        if name != "INTEGRATION.md":
            assert "keyed SUM beyond 1024 keys" in text, name


def test_the_table_bytes_are_monotone_and_refuse_what_the_calls_refuse():
    from alp_amd import capi
    f = capi.lib.alpgpu_keyed_exact_sum_table_bytes
    assert f(0) == U64_MAX and f(capi.KEYED_MANY_KEYS_MAX + 1) == U64_MAX and f(2**32 - 1) == U64_MAX
    last = 0
    for k in (1, 2, 3, 63, 64, 1024, 1025, 4097, 65536, capi.KEYED_MANY_KEYS_MAX - 1, capi.KEYED_MANY_KEYS_MAX):
        b = f(k)
        assert b % 16 == 0 and b >= 8 * 67 * k and b > last, k  # 66 limbs and the flags per key
        last = b
    assert f(capi.KEYED_MANY_KEYS_MAX) < 2**30


def test_without_a_context_every_call_is_an_error_and_writes_nothing():
    from alp_amd import capi
    lib = capi.lib
    a = capi.CColumn()
    a.n_vectors = 1
    mask = (ctypes.c_uint64 * 16)(*([7] * 16))
    trace = (ctypes.c_uint64 * 6)(*([7] * 6))
    counts = (ctypes.c_uint64 * 5)(*([7] * 5))
    sums = (ctypes.c_double * 4)(*([7.0] * 4))
    table = (ctypes.c_uint64 * (67 * 4))(*([7] * (67 * 4)))
    tuning = capi.KeyedTuning(1, 0)
    p = lambda t: ctypes.cast(t, ctypes.c_void_p)
    for t, ct in (("f64", ctypes.c_double), ("f32", ctypes.c_float)):
        keys = (ct * 4)(1.0, 2.0, 3.0, 4.0)
        for acc in (0, 1):
            assert getattr(lib, "alpgpu_decode_keyed_exact_sum_" + t)(None, ctypes.byref(a), ctypes.byref(a), p(mask), None, p(keys), 4, p(sums), p(counts), p(table), acc) == -2
            assert b"null context" in lib.alpgpu_last_error()
            assert getattr(lib, "alpgpu_debug_decode_keyed_exact_sum_" + t)(None, ctypes.byref(a), ctypes.byref(a), p(mask), None, p(keys), 4, p(sums), p(counts), p(table), acc,
                                                                             ctypes.byref(tuning), p(trace)) == -2
            assert b"null context" in lib.alpgpu_last_error()
    assert list(sums) == [7.0] * 4 and list(mask) == [7] * 16 and list(counts) == [7] * 5 and list(trace) == [7] * 6 and list(table) == [7] * (67 * 4)


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------------------------------------
class Col:  # what the wrappers look at before they reach the library
    def __init__(self, dtype, n_vectors):
        from alp_amd import capi
        self.dtype, self.n_vectors, self.c = dtype, n_vectors, capi.CColumn()


def bare_context():
    from alp_amd import capi
    ctx = capi.Context.__new__(capi.Context)
    ctx.device, ctx._h, ctx._follow_torch = 0, None, False
    return ctx


def test_python_rejects_arguments_that_do_not_fit_before_any_launch(monkeypatch):
    """no device: the columns are bare descriptors and every check below fails before the library is called"""
    import torch
    from alp_amd import capi

    def unreachable(*a, **k):
        raise AssertionError("the library was called")
    for t in ("f64", "f32"):
        monkeypatch.setattr(capi.lib, "alpgpu_decode_keyed_exact_sum_" + t, unreachable)
        monkeypatch.setattr(capi.lib, "alpgpu_debug_decode_keyed_exact_sum_" + t, unreachable)
    ctx = bare_context()
    a, b, f, g, short = Col("f64", 4), Col("f64", 4), Col("f32", 4), Col("f32", 4), Col("f64", 3)
    good = np.array([1.0, 2.0, 3.0])
    over = capi.KEYED_MANY_KEYS_MAX + 1
    for val, key in ((a, f), (a, short), (f, a)):  # the columns' types and lengths agree
        with pytest.raises(ValueError):
            ctx.keyed_sum_exact(val, key, good)
        with pytest.raises(ValueError):
            ctx.keyed_sum_exact_into(val, key, torch.zeros(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64))
    for bad in (good.astype(np.float32), torch.zeros(3, dtype=torch.float32), torch.zeros(3, dtype=torch.int64), np.zeros((2, 2)), [], np.zeros(0), np.zeros(over),
                torch.zeros(over, dtype=torch.float64)):  # the columns' type, one dimension, 1 .. 2^20 keys
        with pytest.raises(ValueError):
            ctx.keyed_sum_exact(a, b, bad)
    for bad in (good, torch.zeros(3, dtype=torch.float64), np.zeros(0, np.float32), np.zeros(over, np.float32)):  # float columns take float keys
        with pytest.raises(ValueError):
            ctx.keyed_sum_exact(f, g, bad)
    for bad in (good, good.tolist(), torch.from_numpy(good), torch.zeros(3, dtype=torch.float32)):
        with pytest.raises(ValueError):  # the raw form: a DEVICE tensor of the columns' type; host keys are refused
            ctx.keyed_sum_exact_into(a, b, bad, torch.zeros(3, dtype=torch.float64))
    for bad in (0, -1, over):
        with pytest.raises(ValueError):
            ctx.keyed_sum_exact_table(bad)


def test_the_raw_wrapper_passes_its_arguments_through_and_refuses_what_does_not_fit(monkeypatch):
    """no device: host tensors that answer as tensors on cuda:0 reach the (replaced) library with their n_keys and accumulate; the bounds, the
    shapes, the trace's six words and the table's size are checked in front of it"""
    import torch
    from alp_amd import capi

    class OnDevice(torch.Tensor):  # a host tensor that says it lives on cuda:0: nothing dereferences it here
        is_cuda = property(lambda self: True)
        device = property(lambda self: torch.device("cuda", 0))
    seen = []

    def record(h, val, key, mask, zones, keys, n_keys, sums, counts, table, accumulate, *debug):
        seen.append((int(n_keys), counts is not None and counts.value is not None, int(accumulate), len(debug)))
        return 0
    ctx = bare_context()
    dev = lambda t: t.as_subclass(OnDevice)
    for t, tdt in (("f64", torch.float64), ("f32", torch.float32)):
        monkeypatch.setattr(capi.lib, "alpgpu_decode_keyed_exact_sum_" + t, record)
        monkeypatch.setattr(capi.lib, "alpgpu_debug_decode_keyed_exact_sum_" + t, record)
        a, b = Col(t, 4), Col(t, 4)
        for K in (1, 1024, 1025, 4097):
            keys, sums, cnt = dev(torch.zeros(K, dtype=tdt)), dev(torch.zeros(K, dtype=torch.float64)), dev(torch.zeros(K + 1, dtype=torch.int64))
            table = dev(torch.zeros(capi.lib.alpgpu_keyed_exact_sum_table_bytes(K), dtype=torch.uint8))
            del seen[:]
            ctx.keyed_sum_exact_into(a, b, keys, sums, table=table)
            ctx.keyed_sum_exact_into(a, b, keys, sums, counts_out=cnt, table=table, accumulate=True)
            ctx.keyed_sum_exact_into(a, b, keys, sums, counts_out=cnt, table=table, tuning={"grid": 3})
            ctx.keyed_sum_exact_into(a, b, keys, sums, table=table, trace=dev(torch.zeros(6, dtype=torch.int64)))
            assert seen == [(K, False, 0, 0), (K, True, 1, 0), (K, True, 0, 2), (K, False, 0, 2)], (t, K, seen)
            del seen[:]
            with pytest.raises(ValueError):  # accumulate adds to a table
                ctx.keyed_sum_exact_into(a, b, keys, sums, accumulate=True)
            with pytest.raises(ValueError):  # the family's trace of four words is too short here
                ctx.keyed_sum_exact_into(a, b, keys, sums, table=table, trace=dev(torch.zeros(4, dtype=torch.int64)))
            with pytest.raises(ValueError):  # a table one byte short
                ctx.keyed_sum_exact_into(a, b, keys, sums, table=dev(torch.zeros(table.numel() - 1, dtype=torch.uint8)))
            with pytest.raises(ValueError):  # float sums: the sums are doubles for both precisions
                ctx.keyed_sum_exact_into(a, b, keys, dev(torch.zeros(K, dtype=torch.float32)), table=table)
            with pytest.raises(ValueError):  # counts of the wrong length
                ctx.keyed_sum_exact_into(a, b, keys, sums, counts_out=dev(torch.zeros(K, dtype=torch.int64)), table=table)
            with pytest.raises(ValueError):
                ctx.keyed_sum_exact_into(a, b, keys, sums, table=table, tuning={"flush_every": 1})
            assert seen == []
        K = capi.KEYED_MANY_KEYS_MAX + 1
        with pytest.raises(ValueError):
            ctx.keyed_sum_exact_into(a, b, dev(torch.zeros(K, dtype=tdt)), dev(torch.zeros(K, dtype=torch.float64)))
        big, big2 = Col(t, capi.KEYED_EXACT_VECTORS_MAX + 1), Col(t, capi.KEYED_EXACT_VECTORS_MAX + 1)
        with pytest.raises(ValueError):  # more rows than a limb holds
            ctx.keyed_sum_exact_into(big, big2, dev(torch.zeros(4, dtype=tdt)), dev(torch.zeros(4, dtype=torch.float64)))
        assert seen == []
        with pytest.raises(ValueError):  # the striped keyed SUM keeps its bound and its refusal of float columns
            ctx.keyed_sum_into(a, b, dev(torch.zeros(1025 if t == "f64" else 4, dtype=tdt)), dev(torch.zeros(1025 if t == "f64" else 4, dtype=torch.float64)))


# ---- exact_sum.hpp on the host, under the sanitizers --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("exact_sum") / "exact_sum_host"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{ROOT}/alp_amd/csrc", "-o", str(exe),
                           f"{ROOT}/tests/cpp/exact_sum_host.cpp"])
    return str(exe)


def run_host(exe, lines):
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    out = [int(w, 16) for w in p.stdout.split()]
    assert len(out) == len(lines)
    return out


def as_bits(x):
    return 0x7FF8000000000000 if x != x else bits(x)


def check_lists(exe, lists):
    got = run_host(exe, ["v " + " ".join("%016x" % bits(x) for x in xs) for xs in lists])
    bad = [(xs, "%016x" % g, "%016x" % as_bits(replica.exact_sum(xs))) for xs, g in zip(lists, got) if g != as_bits(replica.exact_sum(xs))]
    assert not bad, f"{len(bad)} of {len(lists)} lists differ from the replica: {bad[:3]}"


def test_the_replica_rounds_as_a_second_route_does_and_knows_its_hand_made_cases():
    """the yardstick itself (numpy and Python only): int / int against Fraction -> float, and sums anybody can check by hand"""
    rng = random.Random(3001)
    for _ in range(2000):
        N = rng.getrandbits(rng.randint(1, 2200)) * rng.choice((1, -1))
        a, b = replica.round_fixed(N), replica.round_fixed_by_fraction(N)
        assert bits(a) == bits(b), N
    assert replica.exact_sum([1e300, 1.0, -1e300]) == 1.0
    assert replica.exact_sum([DBL_MAX, DBL_MAX]) == INF and replica.exact_sum([-DBL_MAX, -DBL_MAX]) == -INF
    assert replica.exact_sum([DBL_MAX, DBL_MAX, -DBL_MAX]) == DBL_MAX
    assert bits(replica.exact_sum([-0.0])) == 0 and bits(replica.exact_sum([])) == 0 and bits(replica.exact_sum([1.5, -1.5])) == 0
    assert replica.exact_sum([1.0, INF]) == INF and replica.exact_sum([-INF, 5.0]) == -INF
    assert np.isnan(replica.exact_sum([INF, -INF])) and np.isnan(replica.exact_sum([1.0, NAN])) and np.isnan(replica.exact_sum([INF, NAN]))
    assert replica.exact_sum([TINY] * 3) == 3 * TINY and replica.exact_sum([2.0 ** 53, 1.0]) == 2.0 ** 53 and replica.exact_sum([2.0 ** 53, 1.0, 1.0]) == 2.0 ** 53 + 2
    limbs = [0] * 66
    limbs[33] = 1 << 18  # 2^(32 * 33 + 18 - 1074) = 1.0
    assert replica.round_limbs(limbs) == 1.0 and replica.round_limbs(limbs, replica.FLAG_NAN) != replica.round_limbs(limbs, replica.FLAG_NAN)
    x = np.array([1.5, 2.5, NAN, 4.0, -0.0, 8.0], np.float32)
    k = np.array([1.0, 1.0, 2.0, 3.0, 3.0, 9.0], np.float32)
    s, c = replica.host_keyed_sum_exact(x, k, np.array([1, 1, 1, 0, 1, 1], bool), np.array([1.0, 2.0, 3.0, 3.0], np.float32))
    assert s.dtype == np.float64 and s[0] == 4.0 and np.isnan(s[1]) and bits(s[2]) == 0 and bits(s[3]) == 0 and c.tolist() == [2, 1, 1, 0, 1]


def test_the_prototypes_mix_of_random_lists(host_program):
    """lists of 0 .. 12 values drawn from random bit patterns, both ends of the exponent range, decimals, and cancelling partners"""
    rng = random.Random(3002)
    special = [TINY, -TINY, MIN_NORMAL, -MIN_NORMAL, DBL_MAX, -DBL_MAX, 0.0, -0.0, 1e300, -1e300, 1.0, -1.0, 2.0 ** -1022 - TINY, INF, -INF, NAN]

    def value():
        c = rng.random()
        if c < 0.15:
            return struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
        if c < 0.3:
            return rng.choice(special)
        if c < 0.6:
            return rng.uniform(-1, 1) * 10.0 ** rng.randint(-320, 308)
        return round(rng.uniform(-1000, 1000), 2)
    lists = []
    for _ in range(6000):
        xs = [value() for _ in range(rng.randint(0, 12))]
        if xs and rng.random() < 0.3:
            xs += [-x for x in xs[: rng.randint(1, len(xs))]]
            rng.shuffle(xs)
        lists.append(xs)
    lists += [[1e300, 1.0, -1e300], [DBL_MAX] * 2, [DBL_MAX, DBL_MAX, -DBL_MAX], [-DBL_MAX, -DBL_MAX, DBL_MAX], [-0.0], [-0.0, -0.0], [], [INF], [INF, -INF], [NAN, 1.0], [-INF, -INF, 3.0]]
    check_lists(host_program, lists)


def test_every_rounding_case(host_program):
    """ties to even up and down, just beside a tie, the carry into the exponent, the largest subnormal plus one ulp, the largest double plus half an ulp"""
    ulp = 2.0 ** -52
    half = 2.0 ** -53
    lists = [
        [1.0, half],                          # a tie below an even mantissa: down
        [1.0 + ulp, half],                    # a tie below an odd mantissa: up
        [1.0, half, TINY],                    # just above the tie: up (the sticky bit lies 1021 bits below)
        [1.0 + ulp, half, -TINY],             # just below it: down
        [1.0, -half / 2],                     # 1 - 2^-54: the mantissa of the binade below, a tie there: up to 1.0
        [2.0 - ulp, half],                    # a tie that carries into the exponent
        [2.0 - ulp, half, -TINY],
        [DBL_MAX, 2.0 ** 970],                # half an ulp above the largest double: a tie, up, beyond it
        [DBL_MAX, 2.0 ** 970, -TINY],         # just below that tie: DBL_MAX
        [-DBL_MAX, -2.0 ** 970],
        [MIN_NORMAL - TINY, TINY],            # the largest subnormal plus one ulp: the smallest normal
        [MIN_NORMAL - TINY, TINY, TINY],
        [MIN_NORMAL, -TINY],
        [TINY, TINY], [TINY, -TINY], [-TINY, -TINY, -TINY],
        [2.0 ** 53, 1.0], [2.0 ** 53, 1.0, 1.0], [2.0 ** 53 + 2.0, 1.0], [2.0 ** 53, 1.0, TINY], [-(2.0 ** 53), -1.0, -TINY],
        [2.0 ** 1023, 2.0 ** 1023], [2.0 ** 1023, 2.0 ** 1023, -(2.0 ** 1023)],
    ]
    for e in range(-1074, 1024, 37):          # a tie, and its two neighbours, in binades across the range (where the bits exist)
        one = 2.0 ** e
        if e - 53 >= -1074:
            lists += [[one, 2.0 ** (e - 53)], [one + 2.0 ** (e - 52), 2.0 ** (e - 53)], [one, 2.0 ** (e - 53), TINY], [-one, -(2.0 ** (e - 53))]]
    for sh in range(0, 64):                   # every position of the top bit within a limb and its neighbour
        lists += [[2.0 ** (sh - 30), 2.0 ** (sh - 30 - 53)], [2.0 ** (sh - 30) * (1 + ulp), 2.0 ** (sh - 30 - 53)], [2.0 ** (sh - 30), 2.0 ** (sh - 30 - 53), 2.0 ** (sh - 30 - 110)]]
    check_lists(host_program, lists)


def test_limbs_at_the_headroom_bound_with_carries_passing_through(host_program):
    """table entries as they are: limbs at +-(2^63 - 2^31), what 2^31 rows of 2^32 - 1 leave, in neighbouring positions and opposite signs, so that
    limb + carry passes 2^63 in magnitude; borrows that run through forty digits; random limbs up to that bound"""
    top = 2 ** 63 - 2 ** 31
    rng = random.Random(3003)
    entries = []
    for j in (0, 1, 2, 17, 31, 32, 33, 40, 62):
        for pattern in ((top, top, top), (-top, -top, -top), (top, -top, top), (-top, top, -top), (top, top, -top, -top), (top, -1, -top), (-top, 1, top, top)):
            limbs = [0] * 66
            for i, v in enumerate(pattern):
                limbs[j + i] = v
            entries.append(limbs)
    for _ in range(300):
        limbs = [0] * 66
        j = rng.randint(0, 60)
        for i in range(rng.randint(1, 5)):
            limbs[j + i] = rng.choice((top, -top, rng.randint(-top, top), rng.randint(-(2 ** 33), 2 ** 33), 0, 1, -1))
        entries.append(limbs)
    borrow = [0] * 66  # 2^(32 * 40) - 1 as one high limb and a -1 far below: every digit between is 0xFFFFFFFF
    borrow[40], borrow[0] = 1, -1
    entries.append(borrow)
    entries.append([-v for v in borrow])
    cancel = [0] * 66  # a high limb, a negative neighbour that takes most of it back, and a small rest far below
    cancel[10], cancel[11], cancel[0] = top, -(top >> 32), ((top >> 32) << 32) - top + 1
    entries.append(cancel)
    lines = ["l 0 " + " ".join(str(v) for v in limbs) for limbs in entries]
    lines += ["l %d " % f + " ".join(str(v) for v in entries[0]) for f in range(1, 8)]  # the flags go first
    got = run_host(host_program, lines)
    want = [as_bits(replica.round_limbs(limbs)) for limbs in entries] + [as_bits(replica.round_limbs(entries[0], f)) for f in range(1, 8)]
    bad = [(i, "%016x" % g, "%016x" % w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, f"{len(bad)} of {len(lines)} entries differ from the replica: {bad[:5]}"
    assert len({w for w in want[: len(entries)]}) > 50
