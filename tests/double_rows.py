"""Hand-built double (64-bit) encodings in the checkers' fixed-stride layout (the dict oracle/pyoracle.py's Oracle.encode_column returns): the 64-bit sibling
of float_rows.py.  Every packed width 0..64 under factors across the table, bases on the bounds of the store decode's conversion shortcut and at both ends of
int64, exception records on both sides of every staging limit, and every ALP_RD cut 48..63 with a dictionary of its own; arm_rows adds the ALP vectors that sit on
both sides of every per-vector decision of the store decode and the sinks, interleave an order in which narrow and wide vectors are neighbours.  numpy only: the CPU tests import this
module, so nothing here may need the built library (tests/layout.py and alp_amd.capi do).  The pieces tests/test_decode_gpu.py builds its vectors from
(empty_encoding, SHORTCUT_BOUND, set_random_exceptions, alp_vectors_with_exception_counts) live here too."""
import numpy as np

from float_rows import ROWGROUP, SCHEME_ALP, SCHEME_ALP_RD, VEC, concat_encodings, pack_u16, take_vectors  # noqa: F401  (shared with the float builder)

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
U64 = 2**64 - 1

# the store decode's conversion shortcut (decode_kernels.hip: kAlpByF[f].shortcut_bound) = min(2^51 - 1, floor((2^63 - 1) / 10^f)) for f = 0..18
SHORTCUT_BOUND = (2251799813685247, 2251799813685247, 2251799813685247, 2251799813685247, 922337203685477, 92233720368547, 9223372036854, 922337203685, 92233720368,
                  9223372036, 922337203, 92233720, 9223372, 922337, 92233, 9223, 922, 92, 9)
SHORTCUT_MAX_BW = 50
FACTORS = (0, 2, 6, 11, 14, 18)
ALP_EXC_COUNTS = (0, 1, 5, 63, 64, 65, 128, 129, 1024)  # around a wavefront's 64 lanes and the 128-entry stage of 8-byte exception values
RD_EXC_COUNTS = (0, 1, 5, 511, 512, 513, 1024)          # 2-byte left parts: the same stage holds 512 of them
RD_RIGHT_WIDTHS = tuple(range(48, 64))                  # what the reference's cut limit (16) can produce
RD_LEFT_WIDTHS = (1, 2, 3)                              # max(1, ceil(log2(dictionary size))), dictionary size <= 8
SPECIAL_BITS = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FF4123456789ABC, 0x7FFFFFFFFFFFFFFF,
                         0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000, 0x0000000000000001], np.uint64)
FACT = tuple(10**i for i in range(19))
FRAC = tuple(float("1e-%d" % i) if i else 1.0 for i in range(21))  # the decimal literals of the oracle's table, rounded as a compiler rounds them


def shortcut_applies(bw, f, base):
    """the rule as decode_kernels.hip states it: bw <= 50 && base >= -bound && base <= bound && base + mask <= bound (no wrap under the first three)"""
    bnd = SHORTCUT_BOUND[f]
    return bw <= SHORTCUT_MAX_BW and -bnd <= base <= bnd and base + ((1 << bw) - 1) <= bnd


def empty_encoding(n):
    """n all-zero ALP vectors in the oracle's layout and dtypes"""
    nrg = (n + ROWGROUP - 1) // ROWGROUP
    return dict(
        scheme=np.full(n, SCHEME_ALP, np.uint8), e=np.zeros(n, np.uint8), f=np.zeros(n, np.uint8), bw=np.zeros(n, np.uint8),
        lbw=np.zeros(n, np.uint8), base=np.zeros(n, np.int64), exc_cnt=np.zeros(n, np.uint16),
        packed=np.zeros((n, VEC), np.int64), packed_left=np.zeros((n, VEC), np.uint16),
        exc=np.zeros((n, VEC), np.float64), pos=np.zeros((n, VEC), np.uint16),
        dict=np.zeros((nrg, 8), np.uint16), dict_size=np.zeros(nrg, np.uint8), k=np.ones(nrg, np.uint8),
        combos=np.zeros((nrg, 10), np.int32))


def set_random_exceptions(enc, v, pos, rng):
    """exceptions of vector v at the ascending positions given, their values arbitrary 64-bit patterns (NaN payloads among them)"""
    c = len(pos)
    enc["exc_cnt"][v] = c
    enc["pos"][v, :c] = np.asarray(pos).astype(np.uint16)
    enc["exc"][v, :c] = rng.integers(0, 2**64, c, dtype=np.uint64).view(np.float64)


def alp_vectors_with_exception_counts(rng, counts, bw, placement="random"):
    """hand-built ALP vectors (random packed words) with the given exception counts; placement: random / front (all in the first quarter) /
    edges (quarter boundaries first: 0, 255, 256, 511, 512, 767, 768, 1023)"""
    n = len(counts)
    enc = empty_encoding(n)
    enc["bw"][:] = bw
    enc["base"][:] = rng.integers(-2**40, 2**40, n)
    edges = np.array([0, 255, 256, 511, 512, 767, 768, 1023])
    for v, c in enumerate(counts):
        e = int(rng.integers(0, 19)); f = int(rng.integers(0, e + 1))
        enc["e"][v], enc["f"][v] = e, f
        enc["packed"][v, :16 * bw] = rng.integers(-2**63, 2**63 - 1, 16 * bw, dtype=np.int64)
        if placement == "front":
            pos = np.sort(rng.choice(256, min(c, 256), replace=False))
        elif placement == "edges":
            rest = np.setdiff1d(np.arange(1024), edges)
            pos = np.sort(np.concatenate([edges[:min(c, 8)], rng.choice(rest, max(c - 8, 0), replace=False)]))
        else:
            pos = np.sort(rng.choice(1024, c, replace=False))
        set_random_exceptions(enc, v, pos, rng)
    return enc


# ---- bit packing ------------------------------------------------------------------------------------------------------------------------------------
def pack_u64(values, bw):
    """FastLanes u64 bit packing of 1024 digits below 2^bw (16 lanes x 64 rows: value i -> lane i & 15, row i >> 4; word k of the lane at 16 k + lane) -> the
    16 * bw words"""
    if bw == 0:
        return np.zeros(0, np.int64)
    out = np.zeros(16 * bw + 16, np.uint64)
    v = values.astype(np.uint64).reshape(64, 16)
    for row in range(64):
        at, sh = (row * bw) // 64, (row * bw) % 64
        out[16 * at:16 * at + 16] |= v[row] << np.uint64(sh)  # (uint64 shifts drop what leaves the word)
        if sh + bw > 64:
            out[16 * (at + 1):16 * (at + 1) + 16] |= v[row] >> np.uint64(64 - sh)
    return out[:16 * bw].view(np.int64)


def unpack_u64(words, bw):
    """the inverse: the 1024 digits of a vector's 16 * bw packed words, as uint64"""
    out = np.zeros((64, 16), np.uint64)
    if bw == 0:
        return out.reshape(-1)
    w = np.concatenate([np.ascontiguousarray(words[:16 * bw]).view(np.uint64), np.zeros(16, np.uint64)])
    mask = np.uint64(U64 >> (64 - bw))
    for row in range(64):
        at, sh = (row * bw) // 64, (row * bw) % 64
        d = w[16 * at:16 * at + 16] >> np.uint64(sh)
        if sh + bw > 64:
            d = d | (w[16 * (at + 1):16 * (at + 1) + 16] << np.uint64(64 - sh))
        out[row] = d & mask
    return out.reshape(-1)


def unpack_u16(words, bw):
    """the inverse of float_rows.pack_u16: the 1024 values of 64 * bw packed u16 words"""
    w = np.concatenate([words[:64 * bw].astype(np.uint32), np.zeros(64, np.uint32)])
    out = np.zeros((16, 64), np.uint32)
    for row in range(16):
        at, sh = (row * bw) // 16, (row * bw) % 16
        out[row] = ((w[64 * at:64 * at + 64] | (w[64 * (at + 1):64 * (at + 1) + 64] << 16)) >> sh) & ((1 << bw) - 1)
    return out.reshape(-1)


def random_words(rng, bw, extremes=8):
    """the packed words of 1024 random digits of bw bits; digit 0 and digit 2^bw - 1 (where the shortcut's bounds bite) planted at `extremes` places each,
    more places than a vector's exceptions are likely to cover"""
    digits = rng.integers(0, 2**64, VEC, dtype=np.uint64) >> np.uint64(64 - bw) if bw else np.zeros(VEC, np.uint64)
    at = rng.choice(VEC, 2 * extremes, replace=False)
    digits[at[:extremes]], digits[at[extremes:]] = 0, (1 << bw) - 1
    return pack_u64(digits, bw)


# ---- ALP rows ---------------------------------------------------------------------------------------------------------------------------------------
def candidate_bases(bw, f, rng):
    """the bases of one (width, factor): 0, -1, one whose base + mask passes INT64_MAX (the sum wraps in 64 bits), one beside INT64_MIN, the four on either
    side of the shortcut's two bounds, a random one; those outside int64 dropped, duplicates dropped, order kept"""
    mask, bnd = (1 << bw) - 1, SHORTCUT_BOUND[f]
    bases = [0, -1]
    if mask > 0:
        bases.append(INT64_MAX - mask // 2)
    bases += [INT64_MIN + 1, -bnd, -bnd - 1, bnd - mask, bnd - mask + 1, int(rng.integers(INT64_MIN, INT64_MAX, endpoint=True))]
    seen, out = set(), []
    for b in bases:
        if INT64_MIN <= b <= INT64_MAX and b not in seen:
            seen.add(b)
            out.append(b)
    return out


def exception_bits(rng, cnt, finite):
    """cnt 64-bit patterns: finite ones (half of the rows moderate values, half any finite pattern), or any pattern with NaNs of both kinds, infinities,
    -0.0 and a denormal planted"""
    if finite and rng.random() < 0.5:
        return (rng.standard_normal(cnt) * 1000.0).view(np.uint64)
    bits = rng.integers(0, 2**64, cnt, dtype=np.uint64)
    if finite:
        return np.where((bits >> np.uint64(52)) & np.uint64(0x7FF) == 0x7FF, bits & np.uint64(0xFFEFFFFFFFFFFFFF), bits)  # exponent 2047 -> 2046
    k = min(cnt, SPECIAL_BITS.size)
    if k:
        bits[rng.choice(cnt, k, replace=False)] = rng.permutation(SPECIAL_BITS)[:k]
    return bits


def set_exceptions(enc, v, cnt, bits, rng):
    """cnt exceptions at random ascending positions of vector v; bits: their values (uint64 patterns for ALP, uint16 left parts for ALP_RD)"""
    enc["exc_cnt"][v] = cnt
    enc["pos"][v, :cnt] = np.sort(rng.choice(VEC, cnt, replace=False)).astype(np.uint16)
    if enc["scheme"][v] == SCHEME_ALP:
        enc["exc"][v].view(np.uint64)[:cnt] = bits
    else:
        enc["exc"][v].view(np.uint16)[:cnt] = bits


def alp_rows(seed=15):
    """ALP vectors for every width 0..64 and factor of FACTORS (exponent f..min(18, f + 2), taken in turn) with the bases of candidate_bases, the packed
    words of random digits (any words are a valid FFOR stream; both extreme digits are among them) and exception counts of ALP_EXC_COUNTS in turn, out of step
    with the base list; three rows of four draw their exception values from finite doubles, the fourth from any pattern.  Padded with random rows to whole
    rowgroups."""
    rng = np.random.default_rng(seed)
    rows = [(bw, f, base) for bw in range(65) for f in FACTORS for base in candidate_bases(bw, f, rng)]
    n = (len(rows) + ROWGROUP - 1) // ROWGROUP * ROWGROUP
    while len(rows) < n:
        rows.append((int(rng.integers(0, 65)), FACTORS[int(rng.integers(0, len(FACTORS)))], int(rng.integers(INT64_MIN, INT64_MAX, endpoint=True))))
    enc = empty_encoding(n)
    turn = rng.permutation(n)  # (exception count and exponent in turn, but not in step with the base list's period)
    for v, (bw, f, base) in enumerate(rows):
        enc["bw"][v], enc["f"][v], enc["base"][v] = bw, f, base
        enc["e"][v] = f + int(turn[v]) % (min(18, f + 2) - f + 1)
        enc["packed"][v, :16 * bw] = random_words(rng, bw)
        cnt = ALP_EXC_COUNTS[(int(turn[v]) // 3) % len(ALP_EXC_COUNTS)]
        set_exceptions(enc, v, cnt, exception_bits(rng, cnt, finite=v % 4 != 0), rng)
    for r in range(n // ROWGROUP):
        enc["combos"][r, :2] = enc["e"][r * ROWGROUP], enc["f"][r * ROWGROUP]
    return enc


# ---- ALP rows for the per-vector arms of the store decode and the sinks ---------------------------------------------------------------------------------
ARM_EXC_COUNTS = (0, 1, 48, 49, 102, 103, 128, 129, 255, 256, 257, 1024)  # both sides of: any exception at all, the sink's LDS stage (48), the pipelined consumer's
#                                                                           1-KiB record (102), the store decode's stage of 128 and the 256-entry one, and everything
ARM_EDGE_WIDTHS = (28, 29, 32, 33, 50, 51, 56, 57, 63, 64)               # the sink's stage (28 | 29), the 32-bit unpack (32 | 33), the shortcut (50 | 51), the ring (56 | 57), the ends


def shortcut_factors(bw):
    """the factors of FACTORS under which a vector of this width can take the shortcut: some base fits the width between the two bounds"""
    return [f for f in FACTORS if bw <= SHORTCUT_MAX_BW and (1 << bw) - 1 <= 2 * SHORTCUT_BOUND[f]]


def arm_rows(seed=17):
    """ALP vectors that populate every (arithmetic arm, exception arm) pair of decode_kernels.hip and consume_kernels.hip, built like alp_rows (random words with both
    extreme digits, exception values mostly finite with specials in every fourth row, ascending positions, random rows up to whole rowgroups):
      * every width 0..50 on the SHORTCUT route with every count of ARM_EXC_COUNTS, under the factors that admit the width in turn, the base on the lower bound, on the
        upper bound (base + mask == bound) and inside, in turn and out of step with the counts;
      * every width of ARM_EDGE_WIDTHS on the LITERAL route with every count of ARM_EXC_COUNTS: bases one step outside either bound, one whose base + mask wraps int64,
        one beside INT64_MIN and a random one, each checked to fail the rule."""
    rng = np.random.default_rng(seed)
    rows = []  # (bw, f, base, exception count)
    for bw in range(SHORTCUT_MAX_BW + 1):
        mask, factors = (1 << bw) - 1, shortcut_factors(bw)
        for i, cnt in enumerate(ARM_EXC_COUNTS):
            f = factors[(i + bw) % len(factors)]
            kind = (i + i // 3 + bw) % 3
            if kind == 2 and 2 * SHORTCUT_BOUND[f] - mask < 2:  # no base strictly inside under this factor: the widest bounds have one
                f = 0
            bnd = SHORTCUT_BOUND[f]
            base = (-bnd, bnd - mask, int(rng.integers(-bnd + 1, bnd - mask)) if kind == 2 else 0)[kind]
            assert shortcut_applies(bw, f, base)
            rows.append((bw, f, base, cnt))
    for bw in ARM_EDGE_WIDTHS:
        mask = (1 << bw) - 1
        for i, cnt in enumerate(ARM_EXC_COUNTS):
            f = FACTORS[(i + bw) % len(FACTORS)]
            bnd = SHORTCUT_BOUND[f]
            bases = [b for b in (-bnd - 1, bnd - mask + 1, INT64_MAX - mask // 2, INT64_MIN + 1, int(rng.integers(INT64_MIN, INT64_MAX, endpoint=True)), 0, -1)
                     if INT64_MIN <= b <= INT64_MAX and not shortcut_applies(bw, f, b)]
            rows.append((bw, f, bases[(i + i // 5) % len(bases)], cnt))
    n = (len(rows) + ROWGROUP - 1) // ROWGROUP * ROWGROUP
    while len(rows) < n:
        rows.append((int(rng.integers(0, 65)), FACTORS[int(rng.integers(0, len(FACTORS)))], int(rng.integers(INT64_MIN, INT64_MAX, endpoint=True)),
                     ARM_EXC_COUNTS[int(rng.integers(0, len(ARM_EXC_COUNTS)))]))
    enc = empty_encoding(n)
    for v, (bw, f, base, cnt) in enumerate(rows):
        enc["bw"][v], enc["f"][v], enc["base"][v] = bw, f, base
        enc["e"][v] = f + v % (min(18, f + 2) - f + 1)
        enc["packed"][v, :16 * bw] = random_words(rng, bw)
        set_exceptions(enc, v, cnt, exception_bits(rng, cnt, finite=v % 4 != 0), rng)
    for r in range(n // ROWGROUP):
        enc["combos"][r, :2] = enc["e"][r * ROWGROUP], enc["f"][r * ROWGROUP]
    return enc


def interleave(enc, seed=18):
    """-> (encoding, order): the vectors of an encoding of ALP rowgroups followed by ALP_RD rowgroups in an order in which narrow and wide vectors are neighbours.  The
    ALP vectors are permuted freely (take_vectors): one of at most 32 packed bits, then one wider, every fourth time two wider ones, so that wide follows narrow, narrow
    follows wide and wide follows wide; what is left of either kind closes the ALP part.  The ALP_RD rowgroups move as whole rowgroups with their dictionaries, one behind
    each ALP rowgroup while both last.  Vector i of the result is vector order[i] of `enc`."""
    rng = np.random.default_rng(seed)
    n = enc["scheme"].size
    assert n % ROWGROUP == 0
    n_alp = int((enc["scheme"] == SCHEME_ALP).sum())
    assert n_alp % ROWGROUP == 0 and (enc["scheme"][:n_alp] == SCHEME_ALP).all() and (enc["scheme"][n_alp:] == SCHEME_ALP_RD).all()
    narrow, wide = rng.permutation(np.nonzero(enc["bw"][:n_alp] <= 32)[0]), rng.permutation(np.nonzero(enc["bw"][:n_alp] > 32)[0])
    alp_order, i, j, step = [], 0, 0, 0
    while i < narrow.size or j < wide.size:
        alp_order += narrow[i:i + 1].tolist()
        take = 2 if step % 4 == 3 else 1
        alp_order += wide[j:j + take].tolist()
        i, j, step = i + 1, j + take, step + 1
    alp_order = np.array(alp_order, np.int64)
    assert np.array_equal(np.sort(alp_order), np.arange(n_alp))
    n_alp_rg, n_rd_rg = n_alp // ROWGROUP, (n - n_alp) // ROWGROUP
    order, source = [], []  # source: the rowgroup of `enc` an ALP_RD rowgroup of the result is, -1 for an ALP rowgroup
    for g in range(max(n_alp_rg, n_rd_rg)):
        if g < n_alp_rg:
            order.append(alp_order[g * ROWGROUP:(g + 1) * ROWGROUP])
            source.append(-1)
        if g < n_rd_rg:
            order.append(n_alp + g * ROWGROUP + np.arange(ROWGROUP))
            source.append(n_alp_rg + g)
    order = np.concatenate(order)
    out = take_vectors(enc, order)
    for k in ("dict", "dict_size", "k", "combos"):  # (an ALP rowgroup's as empty_encoding has them: zeros, k = 1)
        out[k] = np.zeros((n // ROWGROUP,) + enc[k].shape[1:], enc[k].dtype)
    out["k"][:] = 1
    for g, s in enumerate(source):
        if s >= 0:
            for k in ("dict", "dict_size", "k", "combos"):
                out[k][g] = enc[k][s]
        else:
            out["combos"][g, :2] = out["e"][g * ROWGROUP], out["f"][g * ROWGROUP]
    return out, order


# ---- ALP_RD rows ------------------------------------------------------------------------------------------------------------------------------------
def rd_cuts():
    """(right width, left width) pairs the reference can arrive at: a dictionary of more than 2^(lbw-1) distinct left parts needs that many patterns in the
    64 - rbw bits above the cut"""
    return [(rbw, lbw) for rbw in RD_RIGHT_WIDTHS for lbw in RD_LEFT_WIDTHS if 2 ** (64 - rbw) >= (2 ** (lbw - 1) + 1 if lbw > 1 else 1)]


def rd_rows(seed=16):
    """ALP_RD vectors: one rowgroup per cut of rd_cuts() with a dictionary of its own (2^(lbw-1) < size <= 2^lbw, distinct entries; entries and exception left
    parts fit the 64 - rbw bits above the cut; every other rowgroup of left width 3 has exactly 8 entries, so that the dictionary's upper half is read), random
    right words, left indices below the dictionary size, exception counts of RD_EXC_COUNTS at random.  RD_EXC_COUNTS has both sides of the store decode's stage
    of 2-byte exception values, decode_kernels.hip:
        constexpr int kExcStage     = 128; // 8-byte exception values staged in LDS per vector (four times as many 2-byte ALP_RD ones); ...
        const bool     all_staged = cnt <= static_cast<int>(LDS::kExcBytes) / (d.scheme == ALPGPU_SCHEME_ALP ? 8 : 2); // wave-uniform
    i.e. 512 left parts.  Three rowgroups of four keep bit 62 (the exponent's top bit) out of their left parts, so that their values are finite."""
    rng = np.random.default_rng(seed)
    cuts = rd_cuts()
    enc = empty_encoding(len(cuts) * ROWGROUP)
    enc["scheme"][:] = SCHEME_ALP_RD
    enc["k"][:] = 0
    eights = 0
    for r, (rbw, lbw) in enumerate(cuts):
        left_max = 2 ** min(16, 64 - rbw)
        size = int(rng.integers(2 ** (lbw - 1) + 1 if lbw > 1 else 1, min(2**lbw, left_max) + 1))
        if lbw == 3 and left_max >= 8:
            eights += 1
            size = 8 if eights % 2 else size
        enc["dict_size"][r] = size
        # (where the cut leaves bit 62 in the right part, or too few left patterns without it, the rowgroup cannot be kept finite)
        keep = 0xFFFF if r % 4 == 0 or rbw > 62 or left_max // 2 < size else 0xFFFF & ~(1 << (62 - rbw))
        entries = rng.permutation(left_max)
        enc["dict"][r, :size] = entries[(entries & keep) == entries][:size].astype(np.uint16)
        for v in range(r * ROWGROUP, (r + 1) * ROWGROUP):
            enc["bw"][v], enc["lbw"][v] = rbw, lbw
            enc["packed"][v, :16 * rbw] = random_words(rng, rbw)
            enc["packed_left"][v, :64 * lbw] = pack_u16(rng.integers(0, size, VEC), lbw)
            cnt = RD_EXC_COUNTS[int(rng.integers(0, len(RD_EXC_COUNTS)))]
            set_exceptions(enc, v, cnt, rng.integers(0, left_max, cnt).astype(np.uint16) & np.uint16(keep), rng)
    return enc


# ---- a ten-line restatement of the decode, for the CPU test --------------------------------------------------------------------------------------------
def numpy_decode_vector(enc, v):
    """falp + patch (ALP) or the dictionary glue (ALP_RD) of vector v in plain numpy: uint64 arithmetic wraps, as the oracle's does"""
    bw, cnt, pos = int(enc["bw"][v]), int(enc["exc_cnt"][v]), enc["pos"][v].astype(np.int64)
    right = unpack_u64(enc["packed"][v], bw)
    if enc["scheme"][v] == SCHEME_ALP:
        with np.errstate(over="ignore"):
            digits = (right + np.uint64(int(enc["base"][v]) & U64)) * np.uint64(FACT[int(enc["f"][v])])
        out = digits.view(np.int64).astype(np.float64) * FRAC[int(enc["e"][v])]
        out[pos[:cnt]] = enc["exc"][v, :cnt]
        return out
    left = enc["dict"][v // ROWGROUP][np.minimum(unpack_u16(enc["packed_left"][v], int(enc["lbw"][v])), 7)].astype(np.uint64)
    left[pos[:cnt]] = enc["exc"][v].view(np.uint16)[:cnt]
    return ((left << np.uint64(bw)) | right).view(np.float64)
