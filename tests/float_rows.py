"""Hand-built float (32-bit) encodings in the checkers' fixed-stride layout (the dict oracle/pyoracle.py's OracleF32.encode_column returns), aimed at what
no generated column reaches: every packed width 0..32 under every factor, bases on the bounds of the decode's conversion shortcut, exception records
of every staging class, ALP_RD cuts 16..31, and chunks of vectors that straddle the streamed decode's arena.  numpy only: the CPU tests import this module,
so nothing here may need the built library (tests/layout.py and alp_amd.capi do)."""
import numpy as np

VEC = 1024
ROWGROUP = 100
SCHEME_ALP_RD, SCHEME_ALP = 1, 2
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1

# the float decode's conversion shortcut (decode_f32_kernels.hip: finish_quad_f32): min(2^24, (2^31 - 1) / 10^f) for f <= 9, 0 for f = 10
SHORTCUT_BOUND = (2**24, 2**24, 2**24, 2147483, 214748, 21474, 2147, 214, 21, 2, 0)
ALP_EXC_COUNTS = (0, 1, 5, 64, 255, 256, 257, 1024)  # around the 256-entry stage of exception values
RD_EXC_COUNTS = (0, 1, 5, 511, 512, 513, 1024)       # 16-bit left parts: the stage holds 512 of them
RD_RIGHT_WIDTHS = tuple(range(16, 32))               # what the reference's cut limit (16) can produce
RD_LEFT_WIDTHS = (1, 2, 3)                           # max(1, ceil(log2(dictionary size))), dictionary size <= 8
SPECIAL_BITS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FA12345, 0x7FFFFFFF, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001], np.uint32)


def shortcut_applies(bw, f, base):
    """the rule as the kernels state it: bw <= 24 && base >= -bnd[f] && base + mask <= bnd[f] (no wrap: the sum is taken in 64 bits)"""
    bnd = SHORTCUT_BOUND[f]
    return bw <= 24 and base >= -bnd and base + ((1 << bw) - 1) <= bnd


def empty_encoding(n):
    """n all-zero vectors in the oracle's layout and dtypes (base is int64 there)"""
    nrg = (n + ROWGROUP - 1) // ROWGROUP
    return dict(
        scheme=np.full(n, SCHEME_ALP, np.uint8), e=np.zeros(n, np.uint8), f=np.zeros(n, np.uint8), bw=np.zeros(n, np.uint8),
        lbw=np.zeros(n, np.uint8), base=np.zeros(n, np.int64), exc_cnt=np.zeros(n, np.uint16),
        packed=np.zeros((n, VEC), np.int32), packed_left=np.zeros((n, VEC), np.uint16),
        exc=np.zeros((n, VEC), np.float32), pos=np.zeros((n, VEC), np.uint16),
        dict=np.zeros((nrg, 8), np.uint16), dict_size=np.zeros(nrg, np.uint8), k=np.ones(nrg, np.uint8),
        combos=np.full((nrg, 10), -1, np.int32))


def concat_encodings(parts):
    """encodings of whole rowgroups (every one but the last a multiple of 100 vectors) one after the other"""
    for p in parts[:-1]:
        assert p["scheme"].size % ROWGROUP == 0
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def take_vectors(enc, order):
    """the encoding's vectors in another order; the rowgroup arrays stay, so only a permutation inside rowgroups of one kind keeps its meaning"""
    out = dict(enc)
    for k in ("scheme", "e", "f", "bw", "lbw", "base", "exc_cnt", "packed", "packed_left", "exc", "pos"):
        out[k] = enc[k][order]
    return out


def candidate_bases(bw, f, rng):
    """the bases the issue names for one (width, factor): 0, -1, 1 - 2^31, one whose base + mask leaves int32, the four on either side of the shortcut's
    two bounds, a random one; those outside int32 dropped, duplicates dropped, order kept"""
    mask, bnd = (1 << bw) - 1, SHORTCUT_BOUND[f]
    bases = [0, -1, 1 - 2**31]
    if mask > 0:
        bases.append(INT32_MAX - mask // 2)  # base + mask > INT32_MAX: the sum wraps in 32 bits
    bases += [-bnd, -bnd - 1, bnd - mask, bnd - mask + 1, int(rng.integers(INT32_MIN, INT32_MAX + 1))]
    seen, out = set(), []
    for b in bases:
        if INT32_MIN <= b <= INT32_MAX and b not in seen:
            seen.add(b)
            out.append(b)
    return out


def exception_bits(rng, cnt, finite):
    """cnt 32-bit patterns: finite ones (half of the rows moderate values, half any finite pattern), or any pattern with NaNs of both kinds,
    infinities, -0.0 and a denormal planted"""
    if finite:
        if rng.random() < 0.5:
            return (rng.standard_normal(cnt) * 1000.0).astype(np.float32).view(np.uint32)
        bits = rng.integers(0, 2**32, cnt, dtype=np.uint64).astype(np.uint32)
        return np.where((bits >> 23) & 0xFF == 0xFF, bits & np.uint32(0xFF7FFFFF), bits)  # exponent 255 -> 254
    bits = rng.integers(0, 2**32, cnt, dtype=np.uint64).astype(np.uint32)
    k = min(cnt, SPECIAL_BITS.size)
    if k:
        bits[rng.choice(cnt, k, replace=False)] = rng.permutation(SPECIAL_BITS)[:k]
    return bits


def set_exceptions(enc, v, cnt, bits, rng):
    """cnt exceptions at random ascending positions of vector v; bits: their values (uint32 patterns for ALP, uint16 left parts for ALP_RD)"""
    enc["exc_cnt"][v] = cnt
    enc["pos"][v, :cnt] = np.sort(rng.choice(VEC, cnt, replace=False)).astype(np.uint16)
    if enc["scheme"][v] == SCHEME_ALP:
        enc["exc"][v].view(np.uint32)[:cnt] = bits
    else:
        enc["exc"][v].view(np.uint16)[:cnt] = bits


def pack_u32(values, bw):
    """FastLanes u32 bit packing of 1024 digits below 2^bw (32 lanes x 32 rows: value i -> lane i & 31, row i >> 5; word k of the lane at 32 k + lane) -> the
    32 * bw words"""
    if bw == 0:
        return np.zeros(0, np.int32)
    out = np.zeros(32 * bw + 32, np.uint64)
    v = values.astype(np.uint64).reshape(32, 32)
    for row in range(32):
        at, sh = (row * bw) // 32, (row * bw) % 32
        out[32 * at:32 * at + 32] |= (v[row] << np.uint64(sh)) & np.uint64(0xFFFFFFFF)
        out[32 * (at + 1):32 * (at + 1) + 32] |= v[row] >> np.uint64(32 - sh)  # (zero unless the digit crosses the word)
    return out[:32 * bw].astype(np.uint32).view(np.int32)


def random_words(rng, bw, extremes=8):
    """the packed words of 1024 random digits of bw bits; digit 0 and digit 2^bw - 1 (where the shortcut's bounds bite) planted at `extremes` places each,
    more places than a vector's exceptions are likely to cover"""
    digits = rng.integers(0, 2**bw, VEC, dtype=np.uint64)
    at = rng.choice(VEC, 2 * extremes, replace=False)
    digits[at[:extremes]], digits[at[extremes:]] = 0, 2**bw - 1
    return pack_u32(digits, bw)


def alp_rows(seed=5):
    """ALP vectors for every width 0..32 and factor 0..10 (exponent f..min(10, f + 2), taken in turn) with the bases of candidate_bases, the packed
    words of random digits (any words are a valid FFOR stream; both extreme digits are among them) and exception counts of ALP_EXC_COUNTS in turn; three rows of four draw their exception values from finite
    floats.  Padded with random rows to whole rowgroups."""
    rng = np.random.default_rng(seed)
    rows = [(bw, f, base) for bw in range(33) for f in range(11) for base in candidate_bases(bw, f, rng)]
    n = (len(rows) + ROWGROUP - 1) // ROWGROUP * ROWGROUP
    while len(rows) < n:
        rows.append((int(rng.integers(0, 33)), int(rng.integers(0, 11)), int(rng.integers(INT32_MIN, INT32_MAX + 1))))
    enc = empty_encoding(n)
    turn = rng.permutation(n)  # (exception count and exponent in turn, but not in step with the base list's period)
    for v, (bw, f, base) in enumerate(rows):
        enc["bw"][v], enc["f"][v], enc["base"][v] = bw, f, base
        enc["e"][v] = f + int(turn[v]) % (min(10, f + 2) - f + 1)
        enc["packed"][v, :32 * bw] = random_words(rng, bw)
        cnt = ALP_EXC_COUNTS[(int(turn[v]) // 3) % len(ALP_EXC_COUNTS)]
        set_exceptions(enc, v, cnt, exception_bits(rng, cnt, finite=v % 4 != 0), rng)
    for r in range(n // ROWGROUP):
        enc["combos"][r, :2] = enc["e"][r * ROWGROUP], enc["f"][r * ROWGROUP]
    return enc


def pack_u16(values, bw):
    """FastLanes u16 bit packing of 1024 values below 2^bw (64 lanes x 16 rows: value i -> lane i & 63, row i >> 6; word k of the lane at 64 k + lane) -> the
    64 * bw words"""
    out = np.zeros(64 * bw, np.uint16)
    v = values.astype(np.uint32).reshape(16, 64)
    for row in range(16):
        at, sh = (row * bw) // 16, (row * bw) % 16
        out[64 * at:64 * at + 64] |= ((v[row] << sh) & 0xFFFF).astype(np.uint16)
        if sh + bw > 16:
            out[64 * (at + 1):64 * (at + 1) + 64] |= (v[row] >> (16 - sh)).astype(np.uint16)
    return out


def rd_cuts():
    """(right width, left width) pairs the reference can arrive at: a dictionary of more than 2^(lbw-1) distinct left parts needs that many patterns in the
    32 - rbw bits above the cut"""
    return [(rbw, lbw) for rbw in RD_RIGHT_WIDTHS for lbw in RD_LEFT_WIDTHS if 2 ** (32 - rbw) >= (2 ** (lbw - 1) + 1 if lbw > 1 else 1)]


def rd_rows(seed=6):
    """ALP_RD vectors: one rowgroup per cut of rd_cuts() with a dictionary of its own (2^(lbw-1) < size <= 2^lbw, distinct entries; entries and exception left
    parts fit the 32 - rbw bits above the cut), random right words, left indices below the dictionary size, exception counts of RD_EXC_COUNTS at random"""
    rng = np.random.default_rng(seed)
    cuts = rd_cuts()
    enc = empty_encoding(len(cuts) * ROWGROUP)
    enc["scheme"][:] = SCHEME_ALP_RD
    enc["k"][:] = 0
    for r, (rbw, lbw) in enumerate(cuts):
        left_max = 2 ** min(16, 32 - rbw)
        size = int(rng.integers(2 ** (lbw - 1) + 1 if lbw > 1 else 1, min(2**lbw, left_max) + 1))
        enc["dict_size"][r] = size
        # three rowgroups of four keep bit 30 (the exponent's top bit) out of their left parts: every value finite, so that sums and zones say something
        keep = 0xFFFF if r % 4 == 0 or rbw > 30 or left_max // 2 < size else 0xFFFF & ~(1 << (30 - rbw))
        entries = rng.permutation(left_max)
        enc["dict"][r, :size] = entries[(entries & keep) == entries][:size].astype(np.uint16)
        for v in range(r * ROWGROUP, (r + 1) * ROWGROUP):
            enc["bw"][v], enc["lbw"][v] = rbw, lbw
            enc["packed"][v, :32 * rbw] = random_words(rng, rbw)
            enc["packed_left"][v, :64 * lbw] = pack_u16(rng.integers(0, size, VEC), lbw)
            cnt = RD_EXC_COUNTS[int(rng.integers(0, len(RD_EXC_COUNTS)))]
            set_exceptions(enc, v, cnt, rng.integers(0, left_max, cnt).astype(np.uint16) & np.uint16(keep), rng)
    return enc


# ---- chunks that straddle the streamed decode's arena ------------------------------------------------------------------------------------------
# (chunk of C vectors, arena bytes) of the streamed shapes (decode_stream_f32_kernels.hip: launch_decode_stream_f32)
STREAM_SHAPES = ((8, 8192), (4, 12288), (12, 12288), (14, 14336), (16, 16384), (12, 24576), (12, 49152))
RUN_ALIGN = 336  # lcm(4, 8, 12, 14, 16): a run that starts here starts a chunk of every shape


def record_bytes(enc):
    """(packed bytes, exception record bytes) of every vector: tests/layout.py's record_sizes for 4-byte values, restated without the library"""
    alp = enc["scheme"] == SCHEME_ALP
    bw, lbw, cnt = enc["bw"].astype(np.int64), enc["lbw"].astype(np.int64), enc["exc_cnt"].astype(np.int64)
    return np.where(alp, 128 * bw, 128 * (bw + lbw)), (np.where(alp, 6 * cnt, 4 * cnt) + 7) // 8 * 8


def chunk_footprint(pk, rec, skew):
    """what a chunk copied flat takes of the arena (stream_issue_chunk: rec_base + rec_total + 16 <= ARENA; the exception span starts at the 16-byte
    boundary below its first byte, `skew` = exc_off & 15 bytes in front of it)"""
    return (int(pk.sum()) + 15) // 16 * 16 + skew + int(rec.sum()) + 16


def _narrow_run(c, target):
    """c vectors of width 2 whose exception records bring the chunk's footprint to exactly `target` (a multiple of 8)"""
    rec_total = target - 16 - 256 * c
    assert rec_total % 8 == 0 and rec_total > 0
    per = rec_total // c // 24 * 24  # 24 bytes = 4 exceptions: a record without pad
    recs = [per] * c
    recs[-1] = rec_total - per * (c - 1)
    cnts = []
    for r in recs:  # the count whose padded record has r bytes: 6 cnt rounded up to 8
        cnt = r // 6
        while (6 * cnt + 7) // 8 * 8 < r:
            cnt += 1
        assert (6 * cnt + 7) // 8 * 8 == r and cnt <= 1024, (r, cnt)
        cnts.append(cnt)
    return [(2, cnt) for cnt in cnts]


def _wide_run(c, arena, over):
    """c exception-free vectors whose words fill the arena up to the last 128 bytes (flat: the copy needs 16 bytes more than the words) or to its end"""
    total = arena // 128 - (0 if over else 1)
    bws = [total // c] * c
    for i in range(total - sum(bws)):
        bws[i] += 1
    assert max(bws) <= 32
    return [(b, 0) for b in bws]


def arena_runs():
    """[(c, arena, kind, over, [(bw, exc_cnt)] * c)]: for every streamed shape a chunk just under and just over its arena, once of narrow vectors with large
    exception records (8 bytes over; 8 bytes under, so that the chunk still fits when its records start 8 modulo 16), once of wide vectors without any (the last 128-byte step under / the first over)"""
    runs = []
    for c, arena in STREAM_SHAPES:
        for over in (False, True):
            runs.append((c, arena, "narrow", over, _narrow_run(c, arena + 8 if over else arena - 8)))
            runs.append((c, arena, "wide", over, _wide_run(c, arena, over)))
    return runs


def arena_column(seed=8):
    """-> (encoding, [(start vector, c, arena, kind, over)], start vector of the run whose first record lies at an exc_off of 8 modulo 16).
    An ALP column (e = f = 0) whose runs of arena_runs() start at multiples of RUN_ALIGN, i.e. at a chunk boundary of every streamed shape; between them
    filler vectors of small widths, every fourth with a few exceptions.  Exception records are multiples of 8 bytes, so a record starts 8 modulo 16 behind an
    odd number of 8-byte units: the filler in front of the last run is given the exception that makes it so."""
    rng = np.random.default_rng(seed)
    runs = arena_runs()
    n = (len(runs) * RUN_ALIGN + 16 + ROWGROUP - 1) // ROWGROUP * ROWGROUP
    enc = empty_encoding(n)
    shape = {}  # vector -> (bw, cnt)
    where = []
    for i, (c, arena, kind, over, vecs) in enumerate(runs):
        for j, bc in enumerate(vecs):
            shape[i * RUN_ALIGN + j] = bc
        where.append((i * RUN_ALIGN, c, arena, kind, over))
    for v in range(n):
        bw, cnt = shape.get(v, (int(rng.integers(0, 6)), int(rng.integers(1, 9)) if v % 4 == 1 else 0))
        enc["bw"][v] = bw
        enc["base"][v] = int(rng.integers(-2**20, 2**20))
        enc["packed"][v, :32 * bw] = random_words(rng, bw)
        set_exceptions(enc, v, cnt, exception_bits(rng, cnt, finite=v % 2 == 0), rng)
    # the skewed run: the last narrow run that fits its arena; one exception more or less in the filler vector in front of it flips the offset's bit 3
    skewed = [s for s, c, arena, kind, over in where if kind == "narrow" and not over][-1]
    _, rec = record_bytes(enc)
    if int(rec[:skewed].sum()) % 16 != 8:
        cnt = int(enc["exc_cnt"][skewed - 1])
        for new in (cnt + 1, cnt + 2, cnt + 3):
            if ((6 * new + 7) // 8 * 8 - int(rec[skewed - 1])) % 16 == 8:
                set_exceptions(enc, skewed - 1, new, exception_bits(rng, new, finite=True), rng)
                break
    return enc, where, skewed


def uniform_block(bw, exc_cnt=0, seed=0, n=ROWGROUP):
    """n ALP vectors of one width with random words, (e, f) cycling over the factors and bases on either side of the shortcut's bounds"""
    rng = np.random.default_rng(1000 * bw + exc_cnt + seed)
    enc = empty_encoding(n)
    for v in range(n):
        f = v % 11
        enc["bw"][v], enc["f"][v], enc["e"][v] = bw, f, min(10, f + v % 3)
        bases = candidate_bases(bw, f, rng)
        enc["base"][v] = bases[(v // 11) % len(bases)]
        enc["packed"][v, :32 * bw] = random_words(rng, bw)
        set_exceptions(enc, v, exc_cnt, exception_bits(rng, exc_cnt, finite=v % 2 == 0), rng)
    return enc


def mixed_width_block(seed=3, n=6 * ROWGROUP):
    """exception-free ALP vectors of mostly 2-4 bits with runs of twelve 32-bit vectors (at varying chunk phases): the average stays inside the streaming
    rule's 1.5 .. 8.5 bits while single chunks do not fit the streamed shape's arena"""
    rng = np.random.default_rng(seed)
    enc = empty_encoding(n)
    bws = rng.integers(2, 5, n)
    for start in range(40, n - 12, 97):  # 97: every phase against the chunk of 12 comes up
        bws[start:start + 12] = 32
    for v in range(n):
        bw, f = int(bws[v]), v % 11
        enc["bw"][v], enc["f"][v], enc["e"][v] = bw, f, min(10, f + v % 3)
        enc["base"][v] = int(rng.integers(-2**24, 2**24)) if v % 2 else candidate_bases(bw, f, rng)[v % 5]
        enc["packed"][v, :32 * bw] = random_words(rng, bw)
    return enc
