"""CPU: the inputs of tests/test_double_widths_gpu.py are what that suite says they are — double_rows.py's arm_rows (ALP vectors for every per-vector arm of the
store decode and the sinks), interleave (narrow and wide vectors side by side) and the columns the GPU file builds from them.  Only the oracle and the builders are
imported: no GPU, no built library.  The per-vector decisions of decode_kernels.hip and consume_kernels.hip are restated below as constants beside the kernel lines
they restate; `cells` names the arms a set of vectors reaches, REQUIRED_CELLS the ones every column (and, in the GPU file's coverage guard, every family of calls) has
to reach.  These properties are what keeps the GPU comparisons from going vacuous after an edit of a generator."""
import numpy as np
import pytest

import double_rows as dr
from float_rows import SCHEME_ALP, concat_encodings

# ---- the kernels' per-vector decisions ------------------------------------------------------------------------------------------------------------------
# decode_kernels.hip, decode_vector_quarters:  const bool narrow32 = kPerVectorLoops && bw <= 32;   (sinks: if (!kPerVectorLoops && bw <= 32))
UNPACK32_MAX_BW = 32
# decode_kernels.hip, decode_vector_quarters:  if (kPerVectorLoops && cnt == 0) ... else if (kPerVectorLoops && all_staged) ... else ...
#   all_staged = cnt <= LDS::kExcBytes / 8;  kExcStage = 128 (DecodeLds),  DecodeLdsManyExc = DecodeLdsT<kStageBytes, 2 * kExcStage>
STAGES = (128, 256)
# decode_kernels.hip, k_sink_direct:  staged = is_alp && 128u * d.bw <= kSinkStage (3584) && cnt <= kSinkStageMaxExc (48)
SINK_STAGE_MAX_BW, SINK_STAGE_MAX_EXC = 28, 48
# consume_kernels.hip, k_consume_column:  direct = pk_pieces + (exc_loads ? 1 : 0) > kRingPieces (8);  pk_pieces = (8 * bw + 63) >> 6
RING_PIECES = 8
# consume_kernels.hip, k_consume_column:  whole = !direct && rec <= kExcStageBytes (1024);  rec = (10 * cnt + 7) & ~7  (ALP)
RING_RECORD_BYTES = 1024
LITERAL, SHORTCUT64, SHORTCUT32 = 0, 1, 2  # ArithShortcut<0 | 1 | 2>
NO_EXC, ALL_STAGED, PAST_STAGE = 0, 1, 2   # ExcMode<0 | 1 | 2> as the store decode picks them per vector
ARM_EDGES = {SHORTCUT32: (0, 1, 28, 29, 32), SHORTCUT64: (33, 50), LITERAL: dr.ARM_EDGE_WIDTHS}  # the widths at which each arithmetic arm begins and ends
STRIDE_256_CUS = 256 * 2 * 8  # k_consume_column on a 256-CU device: wavefront w reads vectors w, w + 4096, ... (consume_grid: two workgroups of eight wavefronts per CU)


def arith_arms(enc):
    """ArithShortcut of every vector (-1: ALP_RD), from the descriptors"""
    out = np.full(enc["bw"].size, -1)
    for v in np.nonzero(enc["scheme"] == SCHEME_ALP)[0]:
        bw = int(enc["bw"][v])
        out[v] = (SHORTCUT32 if bw <= UNPACK32_MAX_BW else SHORTCUT64) if dr.shortcut_applies(bw, int(enc["f"][v]), int(enc["base"][v])) else LITERAL
    return out


def exc_arms(cnt, stage):
    return np.where(cnt == 0, NO_EXC, np.where(cnt <= stage, ALL_STAGED, PAST_STAGE))


def ring_pieces(enc):
    """1-KiB pieces of k_consume_column's ring that a vector takes: ceil((bw [+ lbw]) / 8) for its words, one for its exception record"""
    alp = enc["scheme"] == SCHEME_ALP
    return (enc["bw"].astype(int) + np.where(alp, 0, enc["lbw"].astype(int)) + 7) // 8 + (enc["exc_cnt"] > 0)


def cells(enc, decoded=None):
    """the arms the ALP vectors of an encoding (those of `decoded`, bool per vector) reach:
      ("store", stage, arithmetic arm, exception arm, bw)   k_decode_column with the 128- and with the 256-entry stage
      ("sink", arithmetic arm, staged in LDS, bw, exc_cnt)   k_sink_direct around its edges 28 | 29 bits and 48 | 49 exceptions
      ("ring", bw, has exceptions, direct)                   k_consume_column: eight pieces, or a ninth and everything from HBM
      ("record", direct, exc_cnt)                            k_consume_column: 102 | 103 exceptions, the record whole in the ring or its positions from HBM"""
    alp = enc["scheme"] == SCHEME_ALP
    if decoded is not None:
        alp = alp & decoded
    at = np.nonzero(alp)[0]
    arith, bw, cnt = arith_arms(enc)[at], enc["bw"][at].astype(int), enc["exc_cnt"][at].astype(int)
    direct = ring_pieces(enc)[at] > RING_PIECES
    out = set()
    for stage in STAGES:
        out |= {("store", stage, int(a), int(x), int(b)) for a, x, b in zip(arith, exc_arms(cnt, stage), bw)}
    staged = (bw <= SINK_STAGE_MAX_BW) & (cnt <= SINK_STAGE_MAX_EXC)
    out |= {("sink", int(a), bool(s), int(b), int(c)) for a, s, b, c in zip(arith, staged, bw, cnt) if b in (28, 29) and c in (48, 49)}
    out |= {("ring", int(b), bool(c > 0), bool(d)) for b, c, d in zip(bw, cnt, direct) if b in (56, 57, 63, 64)}
    out |= {("record", bool(d), int(c)) for c, d in zip(cnt, direct) if c in (102, 103)}
    return out


def required_cells():
    need = {("store", stage, a, x, bw) for stage in STAGES for a, widths in ARM_EDGES.items() for bw in widths for x in (NO_EXC, ALL_STAGED, PAST_STAGE)}
    need |= {("sink", a, bw <= SINK_STAGE_MAX_BW and cnt <= SINK_STAGE_MAX_EXC, bw, cnt) for a in (LITERAL, SHORTCUT32) for bw in (28, 29) for cnt in (48, 49)}
    need |= {("ring", bw, has, (bw + 7) // 8 + has > RING_PIECES) for bw in (56, 57, 63, 64) for has in (False, True)}
    need |= {("record", direct, cnt) for direct in (False, True) for cnt in (102, 103)}
    return need


REQUIRED_CELLS = required_cells()


def column_encodings():
    """the columns tests/test_double_widths_gpu.py reads: {"rows": [alp_rows, arm_rows, rd_rows], "alp_only": [alp_rows, arm_rows], "mixed": interleave(rows)}
    and the order of `mixed` (its vector i is vector order[i] of `rows`)"""
    alp, arm, rd = dr.alp_rows(), dr.arm_rows(), dr.rd_rows()
    rows = concat_encodings([alp, arm, rd])
    mixed, order = dr.interleave(rows)
    return {"rows": rows, "alp_only": concat_encodings([alp, arm]), "mixed": mixed}, order


# ---- the tests ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arm():
    return dr.arm_rows()


@pytest.fixture(scope="module")
def columns():
    return column_encodings()


@pytest.fixture(scope="module")
def decoded_rows(columns, oracle):
    """the oracle's decode of `rows`, [vectors, 1024]"""
    return oracle.decode_column(columns[0]["rows"]).reshape(-1, 1024)


def test_the_restated_rules_are_the_ones_the_issue_names():
    assert ("ring", 57, True, True) in REQUIRED_CELLS and ("ring", 56, True, False) in REQUIRED_CELLS and ("ring", 64, False, False) in REQUIRED_CELLS
    assert ("sink", LITERAL, True, 28, 48) in REQUIRED_CELLS and ("sink", SHORTCUT32, False, 28, 49) in REQUIRED_CELLS and ("sink", SHORTCUT32, False, 29, 48) in REQUIRED_CELLS
    assert (10 * 102 + 7) // 8 * 8 <= RING_RECORD_BYTES < (10 * 103 + 7) // 8 * 8, "102 | 103 exceptions: the record whole in the ring's piece or not"
    assert 128 * SINK_STAGE_MAX_BW == 3584
    assert len([c for c in REQUIRED_CELLS if c[0] == "store"]) == 2 * 3 * (5 + 2 + 10)


def test_arm_rows_are_a_fixed_function_of_the_seed_and_the_oracle_decodes_them(arm, oracle):
    again = dr.arm_rows()
    assert arm.keys() == again.keys() and all(arm[k].tobytes() == again[k].tobytes() for k in arm)
    other = dr.arm_rows(seed=18)
    assert other["packed"].tobytes() != arm["packed"].tobytes()
    n = arm["bw"].size
    assert n % 100 == 0 and 700 <= n <= 1500 and (arm["scheme"] == SCHEME_ALP).all() and arm["base"].dtype == np.int64 and arm["packed"].dtype == np.int64
    want = oracle.decode_column(arm)
    assert want.size == n * 1024 and want.tobytes() == oracle.decode_column(again).tobytes()
    # ... and it is falp + patch as ten lines of numpy state them, on a sample that holds every width (and every row of the edge widths' first count)
    sample = sorted(set(range(0, n, 9)) | {int(np.nonzero(arm["bw"] == w)[0][0]) for w in set(arm["bw"].tolist())})
    assert set(arm["bw"][sample].tolist()) == set(arm["bw"].tolist()) >= set(range(51)) | set(dr.ARM_EDGE_WIDTHS)
    for v in sample:
        got = dr.numpy_decode_vector(arm, v)
        assert np.array_equal(got.view(np.uint64), want[1024 * v:1024 * v + 1024].view(np.uint64)), (v, int(arm["bw"][v]), int(arm["f"][v]), int(arm["e"][v]), int(arm["base"][v]))
    bw, f, e = arm["bw"].astype(int), arm["f"].astype(int), arm["e"].astype(int)
    assert set(f.tolist()) == set(dr.FACTORS) and (e >= f).all() and (e <= 18).all() and (e - f <= 2).all() and all(((e - f) == d).any() for d in (0, 1, 2))
    pos = arm["pos"].astype(int)
    for v in range(n):
        c = int(arm["exc_cnt"][v])
        assert (np.diff(pos[v, :c]) > 0).all() and (c == 0 or pos[v, c - 1] < 1024)
        if v % 4 and c:
            assert np.isfinite(arm["exc"][v, :c]).all(), v
        if c < 1024 - 16 and bw[v] > 0:  # both extreme digits outside the exception positions (a bound only bites where base + 0 or base + mask occurs)
            digits = dr.unpack_u64(arm["packed"][v], int(bw[v]))
            keep = np.ones(1024, bool)
            keep[pos[v, :c]] = False
            assert (digits[keep] == 0).any() and (digits[keep] == np.uint64((1 << int(bw[v])) - 1)).any(), v
    special = np.concatenate([arm["exc"][v].view(np.uint64)[: int(arm["exc_cnt"][v])] for v in range(0, n, 4)])
    is_nan = ((special >> np.uint64(52)) & np.uint64(0x7FF) == 0x7FF) & (special & np.uint64(0xFFFFFFFFFFFFF) != 0)
    assert is_nan.any() and (special == np.uint64(0x7FF0000000000000)).any() and (special == np.uint64(0x8000000000000000)).any()


def test_arm_rows_hold_every_count_on_the_shortcut_route_at_every_width_and_on_the_literal_route_at_the_edges(arm):
    assert dr.ARM_EXC_COUNTS == (0, 1, 48, 49, 102, 103, 128, 129, 255, 256, 257, 1024)
    assert dr.ARM_EDGE_WIDTHS == (28, 29, 32, 33, 50, 51, 56, 57, 63, 64)
    bw, f, cnt = arm["bw"].astype(int), arm["f"].astype(int), arm["exc_cnt"].astype(int)
    base = [int(b) for b in arm["base"]]
    sc = arith_arms(arm) != LITERAL
    assert set(cnt.tolist()) == set(dr.ARM_EXC_COUNTS)
    for w in range(65):
        can = any(w <= dr.SHORTCUT_MAX_BW and (1 << w) - 1 <= 2 * dr.SHORTCUT_BOUND[ff] for ff in dr.FACTORS)
        assert can == (w <= 50) and bool(dr.shortcut_factors(w)) == can
        rows = np.nonzero((bw == w) & sc)[0]
        if not can:
            assert rows.size == 0
            continue
        assert set(cnt[rows].tolist()) == set(dr.ARM_EXC_COUNTS), w
        mask = (1 << w) - 1
        bnd = [dr.SHORTCUT_BOUND[f[v]] for v in rows]
        assert any(base[v] == -b for v, b in zip(rows, bnd)), (w, "a base on the lower bound")
        assert any(base[v] + mask == b for v, b in zip(rows, bnd)), (w, "a base whose base + mask is the upper bound")
        assert any(-b < base[v] and base[v] + mask < b for v, b in zip(rows, bnd)), (w, "a base inside")
        assert set(f[rows].tolist()) == set(dr.shortcut_factors(w)), (w, "every factor that admits the width")
    for w in dr.ARM_EDGE_WIDTHS:
        rows = np.nonzero((bw == w) & ~sc)[0]
        assert set(cnt[rows].tolist()) == set(dr.ARM_EXC_COUNTS), w
        if w <= dr.SHORTCUT_MAX_BW:  # the literal route by the bounds, not by the width: one step outside either bound
            mask = (1 << w) - 1
            assert any(base[v] == -dr.SHORTCUT_BOUND[f[v]] - 1 for v in rows) and any(base[v] + mask == dr.SHORTCUT_BOUND[f[v]] + 1 for v in rows), w
    # the counts do not move in step with the base kind: the pairs on either side of a stage meet bound rows and inside rows
    on_bound = np.array([sc[v] and (base[v] == -dr.SHORTCUT_BOUND[f[v]] or base[v] + (1 << bw[v]) - 1 == dr.SHORTCUT_BOUND[f[v]]) for v in range(bw.size)])
    for c in dr.ARM_EXC_COUNTS:
        assert (on_bound & (cnt == c)).sum() >= 10 and (sc & ~on_bound & (cnt == c)).sum() >= 5, c
    assert REQUIRED_CELLS <= cells(arm), sorted(REQUIRED_CELLS - cells(arm))


def test_what_alp_rows_alone_left_out():
    """the counts the issue gives for dr.alp_rows(): the gaps arm_rows closes are gaps"""
    alp = dr.alp_rows()
    arith, bw, cnt = arith_arms(alp), alp["bw"].astype(int), alp["exc_cnt"].astype(int)
    assert alp["bw"].size == 3500 and int((arith != LITERAL).sum()) == 784  # (by shortcut_applies; 760 of them wider than 0 bits)
    quiet64 = (arith == SHORTCUT64) & (cnt == 0)
    assert int(quiet64.sum()) == 19 and 35 not in set(bw[quiet64].tolist())
    assert not ((arith == SHORTCUT32) & (cnt > 256) & (bw == 32)).any()
    for w in (32, 33, 50):
        assert int(((arith != LITERAL) & (cnt == 0) & (bw == w)).sum()) == 1, w
    assert int(((bw == SINK_STAGE_MAX_BW) & (cnt <= SINK_STAGE_MAX_EXC)).sum()) == 18, "vectors on the staged side of the sink's 28-bit edge"
    assert not set(cnt.tolist()) & {48, 49, 102, 103, 255, 256, 257}
    assert not REQUIRED_CELLS <= cells(alp)


def test_a_width_of_51_passes_the_bounds_only_where_the_shortcut_is_exact_anyway(columns):
    """`bw <= 50` in the store decode's rule is implied by its two bounds except at width 51 with a base in [-bound, bound - (2^51 - 1)] (f <= 3: bases 0, -1 and
    -bound of candidate_bases): rows of that kind are in every column, and there every base + digit still lies in (-2^51, 2^51) with its product inside int64,
    where the shortcut's conversion and product are exact — a build with `bw <= 51` writes the same bits, so the GPU tests cannot tell the two apart, and need
    not (run against such a build, tests/test_double_widths_gpu.py passes).  From 52 bits on no base passes the bounds at all."""
    for name, enc in columns[0].items():
        alp = enc["scheme"] == SCHEME_ALP
        bw, f, base = enc["bw"].astype(int), [int(x) for x in enc["f"]], [int(b) for b in enc["base"]]  # (Python integers: base + mask may leave int64)
        inside = np.array([bool(alp[v]) and -dr.SHORTCUT_BOUND[f[v]] <= base[v] and base[v] + (1 << int(bw[v])) - 1 <= dr.SHORTCUT_BOUND[f[v]] for v in range(bw.size)])
        rows = np.nonzero(inside & (bw == 51))[0]
        assert rows.size >= 3 and {base[v] for v in rows} >= {0, -1}, name
        for v in rows:
            assert f[v] <= 3 and dr.SHORTCUT_BOUND[f[v]] == 2**51 - 1 and -2**51 < base[v] <= 0 and base[v] + 2**51 - 1 < 2**51
            assert (2**51 - 1) * 10 ** f[v] < 2**63
        assert not (inside & (bw > 51)).any(), name
        assert all((1 << w) - 1 > 2 * max(dr.SHORTCUT_BOUND) for w in range(52, 65))


def test_every_column_reaches_every_cell_width_and_cut(columns):
    encs, order = columns
    for name, enc in encs.items():
        n = enc["bw"].size
        assert n % 100 == 0 and n <= 9500, (name, n)
        got = cells(enc)
        assert REQUIRED_CELLS <= got, (name, sorted(REQUIRED_CELLS - got))
        alp = enc["scheme"] == SCHEME_ALP
        assert set(enc["bw"][alp].tolist()) == set(range(65)), name
        if name != "alp_only":
            assert sorted(set(zip(enc["bw"][~alp].tolist(), enc["lbw"][~alp].tolist()))) == sorted(dr.rd_cuts()), name
            assert set(enc["exc_cnt"][~alp].tolist()) == set(dr.RD_EXC_COUNTS), name
        assert set(enc["exc_cnt"][alp].tolist()) == set(dr.ALP_EXC_COUNTS) | set(dr.ARM_EXC_COUNTS), name
    assert encs["alp_only"]["bw"].size + 100 * len(dr.rd_cuts()) == encs["rows"]["bw"].size == encs["mixed"]["bw"].size


def test_the_launch_rule_sees_an_exception_heavy_alp_column_and_a_mostly_alp_rd_one(columns):
    """decode_policy.hpp, policy_shape_f64: many_exc = one && ... && exc_bytes >= kManyExcBytesPerVector (10 * 128) * n_vectors && !mostly_rd, one = !(narrow: bits <= 22 with
    exceptions); mostly_rd = 2 * rd_vectors > n_vectors.  The ALP-only column must get the 256-entry-stage instance, `rows` and `mixed` the ALP_RD shape."""
    encs, _ = columns
    alp = dr.alp_rows()

    def record_bytes_and_bits(enc):
        cnt, is_alp = enc["exc_cnt"].astype(np.int64), enc["scheme"] == SCHEME_ALP
        rec = (np.where(is_alp, 10, 4) * cnt + 7) // 8 * 8
        return float(rec.sum()) / enc["bw"].size, float((enc["bw"].astype(np.int64) + np.where(is_alp, 0, enc["lbw"])).mean())

    rec, bits = record_bytes_and_bits(alp)
    assert 1600 <= rec <= 1680 and 31.0 <= bits <= 32.5, (rec, bits)  # (what the issue counted: 1640 B, 31.8 bits)
    rec, bits = record_bytes_and_bits(encs["alp_only"])
    assert rec >= 1280 and bits > 22, (rec, bits)
    for name in ("rows", "mixed"):
        enc = encs[name]
        assert 2 * int((enc["scheme"] != SCHEME_ALP).sum()) > enc["bw"].size, name


def test_interleave_keeps_every_vector_and_puts_narrow_beside_wide(columns, decoded_rows, oracle):
    encs, order = columns
    rows, mixed = encs["rows"], encs["mixed"]
    n = rows["bw"].size
    assert np.array_equal(np.sort(order), np.arange(n))
    again, order2 = dr.interleave(rows)
    assert np.array_equal(order, order2) and all(mixed[k].tobytes() == again[k].tobytes() for k in mixed)
    assert not np.array_equal(dr.interleave(rows, seed=19)[1], order)
    for k in ("scheme", "bw", "lbw", "e", "f", "base", "exc_cnt"):
        assert np.array_equal(mixed[k], rows[k][order]), k
    # whole rowgroups of one scheme, an ALP_RD rowgroup with the cut and the dictionary it came with
    alp_rg = mixed["scheme"].reshape(-1, 100) == SCHEME_ALP
    assert (alp_rg.all(axis=1) | ~alp_rg.any(axis=1)).all()
    kinds = alp_rg[:, 0]
    assert (kinds[:-1] != kinds[1:]).sum() >= 2 * min(kinds.sum(), (~kinds).sum()) - 1, "ALP_RD rowgroups lie between ALP rowgroups"
    for g in np.nonzero(~kinds)[0]:
        s = int(order[100 * g]) // 100
        assert np.array_equal(order[100 * g:100 * g + 100], 100 * s + np.arange(100)), g
        assert np.array_equal(mixed["dict"][g], rows["dict"][s]) and mixed["dict_size"][g] == rows["dict_size"][s], g
    # the decode of vector i is the decode of the vector it came from
    got = oracle.decode_column(mixed).reshape(-1, 1024)
    assert np.array_equal(got.view(np.uint64), decoded_rows[order].view(np.uint64))
    # neighbours, in vector order (the store decode's workgroups, k_sink_direct's wavefronts) ...
    bw, alp = mixed["bw"].astype(int), mixed["scheme"] == SCHEME_ALP
    narrow, wide = alp & (bw <= 32), alp & (bw > 32)
    assert (narrow[:-1] & wide[1:]).sum() >= 1000 and (wide[:-1] & narrow[1:]).sum() >= 1000 and (wide[:-1] & wide[1:]).sum() >= 200
    assert (narrow[:-1] & ~alp[1:]).any() or (wide[:-1] & ~alp[1:]).any()
    pieces = ring_pieces(mixed)
    assert int(pieces.max()) == RING_PIECES + 1 and ((pieces[:-1] == RING_PIECES) & (pieces[1:] == RING_PIECES + 1)).sum() >= 5, "a 9-piece vector directly after an 8-piece one"
    assert ((pieces[:-1] == RING_PIECES) & (pieces[1:] == RING_PIECES + 1) & alp[:-1] & alp[1:]).any(), "... both of them ALP"
    # ... and as one wavefront of k_consume_column meets them on a 256-CU device, a stride apart: the same classes
    a, b = pieces[:-STRIDE_256_CUS], pieces[STRIDE_256_CUS:]
    assert ((a == RING_PIECES) & (b == RING_PIECES + 1)).any() and ((a == RING_PIECES + 1) & (b <= 4)).any() and ((a <= 4) & (b == RING_PIECES + 1)).any()
    assert ((a <= 2) & (b == RING_PIECES)).any() and ((a == RING_PIECES) & (b <= 2)).any()


def test_at_least_half_of_the_vectors_of_each_column_are_finite(columns, decoded_rows):
    encs, order = columns
    finite = np.isfinite(decoded_rows).all(axis=1)
    n_alp, n_arm = dr.alp_rows()["bw"].size, dr.arm_rows()["bw"].size
    share = lambda m: float(m.sum()) / m.size
    base = share(np.concatenate([finite[:n_alp], finite[n_alp + n_arm:]]))  # [alp_rows, rd_rows], the register-decode suite's column
    assert 0.80 <= base <= 0.84, base
    assert share(finite) >= 0.5 and share(finite[:n_alp + n_arm]) >= 0.5 and share(finite[order]) >= 0.5
    assert share(finite[n_alp:n_alp + n_arm]) >= 0.5, "arm_rows on their own"
