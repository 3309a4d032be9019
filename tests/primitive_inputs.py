"""Inputs of the batch-primitive tests (tests/test_primitives_cpu.py, tests/test_primitive_batches_gpu.py) and their expectations: pattern batches whose
vector v holds pattern v % P (P odd, so that the vectors a wavefront meets on consecutive trips of its grid-stride loop differ for any power-of-two grid),
hand-built rowgroup states, exception placements aimed at the ballot ranks, and numpy restatements of the four primitives the oracle only has behind a state
record (rd_encoder::encode / decode, patch_exceptions, analyze_ffor).  numpy and the oracle only: nothing here needs the built library or a GPU."""
import ctypes as C

import numpy as np

import datagen

VEC = 1024
ROWGROUP = 100
SCHEME_ALP_RD, SCHEME_ALP = 1, 2
# alpgpu_rowgroup_state (include/alpgpu.h), the dtype tests/layout.py takes from alp_amd.capi (tests/test_primitives_cpu.py compares the two)
STATE_DTYPE = np.dtype([("scheme", np.uint8), ("k", np.uint8), ("combos", np.uint8, (10,)), ("rd_rbw", np.uint8), ("rd_lbw", np.uint8),
                        ("rd_dict_size", np.uint8), ("pad", np.uint8), ("rd_dict", np.uint16, (8,))], align=False)
EXC_COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 1024)  # around one and two ballots of 64 lanes, and a full vector
SENTINEL_BYTE = 0xA5                                  # what every output holds before a kernel runs


class Prec:
    """what differs between the two precisions: types, the (e,f) table, the ALP_RD cuts, which lane holds which position"""

    def __init__(self, bits):
        self.bits = bits
        self.name = "f64" if bits == 64 else "f32"
        self.fdt, self.idt, self.udt = (np.float64, np.int64, np.uint64) if bits == 64 else (np.float32, np.int32, np.uint32)
        self.max_e = 18 if bits == 64 else 10
        self.ef = [(e, f) for e in range(self.max_e + 1) for f in range(e + 1)]  # 190 / 66 pairs
        self.cuts = tuple(range(48, 64)) if bits == 64 else tuple(range(16, 32))
        self.steps, self.per_lane = (8, 2) if bits == 64 else (4, 4)             # position = steps' stride * m + per_lane * lane + j
        self.imin, self.imax = -2**(bits - 1), 2**(bits - 1) - 1

    def position(self, m, lane, j):
        return 64 * self.per_lane * m + self.per_lane * lane + j

    def step_positions(self, m, j):
        """the 64 positions one (m, j) step of the encoders covers, one per lane"""
        return np.array([self.position(m, lane, j) for lane in range(64)])

    def lane_positions(self, lane):
        """the 16 positions one lane holds"""
        return np.array(sorted(self.position(m, lane, j) for m in range(self.steps) for j in range(self.per_lane)))


F64, F32 = Prec(64), Prec(32)


def second_trip_batch(cu_count):
    """the smallest batch in which some wavefronts take a second trip of ALPGPU_VECTOR_LOOP and a workgroup has one that does not: the grid is capped at
    cu_count * 16 workgroups of 4 wavefronts (prim_grid in primitive_kernels.hip, prim_grid_f32 in primitive_f32_kernels.hip), so 64 * cu_count vectors fill one
    trip; plus one whole workgroup (4) and three wavefronts of the next (3)"""
    return 64 * cu_count + 7


def pattern_of(v, P):
    return v % P


def sentinel(dtype):
    return np.frombuffer(bytes([SENTINEL_BYTE]) * np.dtype(dtype).itemsize, dtype)[0]


# ---- the oracle's functions that take a state record ----------------------------------------------------------------------------------------------
class AlpoState(C.Structure):  # alpo_state, oracle/alp_oracle.h
    _fields_ = [("scheme", C.c_int), ("sampled_values_n", C.c_size_t), ("k_combinations", C.c_int), ("combos", (C.c_int * 2) * 5), ("exp", C.c_uint8),
                ("fac", C.c_uint8), ("right_bit_width", C.c_uint8), ("left_bit_width", C.c_uint8), ("left_parts_dict", C.c_uint16 * 8),
                ("actual_dictionary_size", C.c_uint8), ("rd_sorted_left", C.c_uint16 * 1024), ("rd_sorted_count", C.c_uint16)]


def alpo_state(rec):
    """a rowgroup state record as the oracle's struct; no sorted list, so that a left part outside the dictionary gets dict_size (what both kernels write
    when they are given no order table)"""
    st = AlpoState()
    st.scheme = int(rec["scheme"])
    st.k_combinations = int(rec["k"])
    for i in range(5):
        st.combos[i][0], st.combos[i][1] = int(rec["combos"][2 * i]), int(rec["combos"][2 * i + 1])
    st.right_bit_width, st.left_bit_width = int(rec["rd_rbw"]), int(rec["rd_lbw"])
    st.actual_dictionary_size = int(rec["rd_dict_size"])
    for i in range(8):
        st.left_parts_dict[i] = int(rec["rd_dict"][i])
    return st


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def oracle_find_best_ef(o, prec, rec, vec):
    """encoder::encode's choice of (e, f) for one vector: the state's only candidate, or the second-level sampling's"""
    if int(rec["k"]) <= 1:
        return int(rec["combos"][0]), int(rec["combos"][1])
    st = alpo_state(rec)
    vec = np.ascontiguousarray(vec, prec.fdt)
    fac, exp = np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    o.fn("find_best_ef")(C.byref(st), _p(vec), C.c_int(VEC), _p(fac), _p(exp))
    return int(exp[0]), int(fac[0])


def oracle_rd_encode(o, prec, rec, vec):
    st = alpo_state(rec)
    vec = np.ascontiguousarray(vec, prec.fdt)
    exc, pos, cnt = np.zeros(VEC, np.uint16), np.zeros(VEC, np.uint16), np.zeros(1, np.uint16)
    right, left = np.zeros(VEC, prec.udt), np.zeros(VEC, np.uint16)
    o.fn("rd_encode")(_p(vec), _p(exc), _p(pos), _p(cnt), _p(right), _p(left), C.byref(st))
    return right, left, exc, pos, int(cnt[0])


def oracle_rd_decode(o, prec, rec, right, left, exc, pos, cnt):
    st = alpo_state(rec)
    out = np.zeros(VEC, prec.fdt)
    o.fn("rd_decode")(_p(out), _p(np.ascontiguousarray(right, prec.udt)), _p(np.ascontiguousarray(left, np.uint16)), _p(np.ascontiguousarray(exc, np.uint16)),
                      _p(np.ascontiguousarray(pos, np.uint16)), C.c_uint16(cnt), C.byref(st))
    return out


def oracle_encode_value_f64(o, values, e, f, safe):
    fn = o.fn("encode_value_safe" if safe else "encode_value_unsafe", C.c_int64)
    ce, cf = C.c_int(e), C.c_int(f)
    return np.array([fn(C.c_double(float(v)), cf, ce) for v in values], np.int64)


def oracle_ffor(o, bits, vals, bw, base):
    """Oracle has the 64 / 16 / 8-bit lanes, OracleF32 the 32-bit ones"""
    return getattr(o, f"ffor_u{bits}")(vals, bw, base)


# ---- numpy restatements -----------------------------------------------------------------------------------------------------------------------------
def analyze_ffor_np(enc):
    """encoder::analyze_ffor: base = min, width = bit length of the unsigned difference max - min"""
    mn, mx = int(enc.min()), int(enc.max())
    return (mx - mn).bit_length(), mn


def patch_np(out, exc, pos, cnt):
    """decoder::patch_exceptions on bit patterns: out[pos[j]] = exc[j] for j < cnt, in order"""
    out = out.copy()
    for j in range(int(cnt)):
        out[int(pos[j])] = exc[j]
    return out


def rd_encode_np(prec, bits, rec):
    """rd_encoder::encode on unpacked arrays, without the sampled map: right = bits & mask, left = position in the dictionary or dict_size where absent,
    exceptions (the left parts themselves) in ascending position"""
    rbw, ds = int(rec["rd_rbw"]), int(rec["rd_dict_size"])
    bits = bits.astype(np.uint64)
    right = (bits & np.uint64((1 << rbw) - 1)).astype(prec.udt)
    key = (bits >> np.uint64(rbw)).astype(np.uint16)
    left = np.full(VEC, ds, np.uint16)
    for d in range(ds - 1, -1, -1):  # the first matching entry wins
        left[key == rec["rd_dict"][d]] = d
    pos = np.nonzero(left == ds)[0].astype(np.uint16)
    return right, left, key[pos], pos, pos.size


def rd_decode_np(prec, rec, right, left, exc, pos, cnt):
    """rd_encoder::decode: dictionary entries glued to the right parts (0 for an index past the dictionary's 8 slots), then the exceptions' left parts"""
    rbw = int(rec["rd_rbw"])
    dic = np.concatenate([rec["rd_dict"].astype(np.uint64), np.zeros(1, np.uint64)])
    l = dic[np.minimum(left.astype(np.int64), 8)]
    bits = (l << np.uint64(rbw)) | right.astype(np.uint64)
    p = pos[:cnt].astype(np.int64)
    bits[p] = (exc[:cnt].astype(np.uint64) << np.uint64(rbw)) | right.astype(np.uint64)[p]
    return (bits & np.uint64(2**prec.bits - 1)).astype(prec.udt)


# ---- FFOR pattern batches ---------------------------------------------------------------------------------------------------------------------------
LANE = {64: (np.uint64, 16), 32: (np.uint32, 32), 16: (np.uint16, 64), 8: (np.uint8, 128)}  # lane width -> type, packed words per bit of width
NOOP_WIDTHS = {64: (65, 255), 32: (33, 255), 16: (17, 255), 8: (9, 255)}                     # widths the reference's switch has no case for


def ffor_patterns(o, bits, widths, seed, ef=None):
    """one vector per entry of `widths` (an invalid width gives a vector the kernels must leave alone): values = base + digits below 2^bw, wrapping; their packed
    form from the oracle; for 64 / 32-bit lanes also an (e,f) per vector and the doubles / floats falp gives (the bit patterns)"""
    dt, words = LANE[bits]
    rng = np.random.default_rng(seed)
    P = len(widths)
    raw = rng.integers(0, 2**bits, (P, VEC), dtype=np.uint64).astype(dt)
    base = rng.integers(0, 2**bits, P, dtype=np.uint64).astype(dt)
    vals, packed = np.empty((P, VEC), dt), np.zeros((P, VEC), dt)
    for i, bw in enumerate(widths):
        mask = dt((1 << bw) - 1) if bw < bits else dt(2**bits - 1)
        vals[i] = (raw[i] & mask) + base[i]  # wraps in dt
        if bw <= bits:
            packed[i] = oracle_ffor(o, bits, vals[i], int(bw), int(base[i]))
        else:
            packed[i] = raw[i]
    b = dict(bits=bits, words=words, P=P, bw=np.array(widths, np.uint8), base=base, vals=vals, packed=packed)
    if ef is not None:
        pairs = [ef[(7 * i + 3) % len(ef)] for i in range(P)]
        b["exp"], b["fac"] = np.array([e for e, f in pairs], np.uint8), np.array([f for e, f in pairs], np.uint8)
        udt = np.uint64 if bits == 64 else np.uint32
        b["falp"] = np.stack([o.falp(packed[i], int(bw), int(base[i]), int(b["fac"][i]), int(b["exp"][i])).view(udt) if bw <= bits else np.zeros(VEC, udt)
                              for i, bw in enumerate(widths)])
    return b


def big_ffor_widths(bits):
    """the big batch: every valid width, repeated until the period is odd and at least 33 (65, 33, 51, 45 patterns)"""
    w = list(range(bits + 1))
    while len(w) < 33 or len(w) % 2 == 0:
        w += list(range(bits + 1))
    return w


def noop_mix_widths(bits):
    """valid widths with the two no-op widths between them"""
    lo, hi = NOOP_WIDTHS[bits]
    w = []
    for bw in range(bits + 1):
        w.append(bw)
        if bw % 3 == 0:
            w.append(lo if bw % 2 == 0 else hi)
    return w + [hi, lo]


# ---- every (e,f): integers on the edges of the decoder's arithmetic --------------------------------------------------------------------------------
def edge_integer_rows(prec, seed=2025):
    """one row of 1024 integers per (e,f): 0, +-1, both ends, +-2^53 and its neighbours (+-2^24 for float), +-10^k, the integers whose product with 10^f sits on
    the wrap, and a seeded fill, half of it anywhere, half within twice that wrap point"""
    rng = np.random.default_rng(seed)
    b = prec.bits
    rows = np.empty((len(prec.ef), VEC), prec.idt)
    mant = 53 if b == 64 else 24
    for i, (e, f) in enumerate(prec.ef):
        head = [0, 1, -1, prec.imin, prec.imax]
        for d in (-1, 0, 1):
            head += [2**mant + d, -(2**mant) + d]
            r = (1 << (b - 1)) // 10**f + d
            head += [r, -r]
            r = (1 << b) // 10**f + d
            head += [r, -r]
        head += [s * 10**k for k in range(19 if b == 64 else 10) for s in (1, -1)]
        head = [h & (2**b - 1) for h in head]
        lim = min(2 * ((1 << (b - 1)) // 10**f) + 2, prec.imax)
        near = rng.integers(-lim, lim + 1, 400).astype(np.int64)
        far = rng.integers(prec.imin, prec.imax, VEC - 400 - len(head), dtype=np.int64, endpoint=True)
        rows[i] = np.concatenate([np.array(head, np.uint64), near.view(np.uint64), far.view(np.uint64)]).astype(prec.udt).view(prec.idt)
    return rows


def boundary_vectors(prec):
    """the adversarial vectors, then vectors filled from the search's boundary values (the last one padded with its first value)"""
    adv = datagen.adversarial_vectors() if prec.bits == 64 else datagen.adversarial_vectors_f32()
    vals = datagen.search_boundary_values() if prec.bits == 64 else datagen.search_boundary_values_f32()
    pad = (-vals.size) % VEC
    vals = np.concatenate([vals, np.full(pad, vals[0], vals.dtype)]).reshape(-1, VEC)
    return np.concatenate([np.stack(list(adv.values())).astype(prec.fdt), vals.astype(prec.fdt)])


def unique_boundary_values():
    v = datagen.search_boundary_values()
    return v[np.unique(v.view(np.uint64), return_index=True)[1]]


# ---- analyze_ffor ------------------------------------------------------------------------------------------------------------------------------------
def analyze_cases(prec, seed=11):
    """integers for analyze_ffor: 1024 vectors with the minimum at position p and the maximum at 1023 - p; for every width a range of exactly 2^bw - 1 and one of
    2^(bw-1) (both need bw bits); a constant; both ends of the type.  -> (vectors, [(name, width aimed at or None)])"""
    rng = np.random.default_rng(seed)
    b = prec.bits
    rows, names = [], []

    def vector(mn, mx, pmin, pmax):
        v = rng.integers(mn + 1, mx - 1, VEC, dtype=np.int64, endpoint=True) if mx - mn >= 2 else np.full(VEC, mn, np.int64)
        v[pmax], v[pmin] = mx, mn  # the only minimum and the only maximum wherever the range leaves room between them
        return v.astype(prec.idt)
    for p in range(VEC):
        span = int(rng.integers(2, 2**(1 + p % (b - 2)), endpoint=True))
        mn = int(rng.integers(prec.imin, prec.imax - span, endpoint=True))
        rows.append(vector(mn, mn + span, p, 1023 - p))
        names.append((f"min at {p}, max at {1023 - p}", None))
    for bw in range(1, b + 1):
        for span in (2**bw - 1, 2**(bw - 1)):
            mn = int(rng.integers(prec.imin, prec.imax - span, endpoint=True))
            pmin, pmax = (int(q) for q in rng.choice(VEC, 2, replace=False))
            rows.append(vector(mn, mn + span, pmin, pmax))
            names.append((f"range {span} at width {bw}", bw))
    rows.append(np.full(VEC, int(rng.integers(prec.imin, prec.imax)), prec.idt))
    names.append(("constant", 0))
    v = np.full(VEC, prec.imin, np.int64)
    v[int(rng.integers(0, VEC))] = prec.imax
    rows.append(v.astype(prec.idt))
    names.append(("both ends of the type", b))
    return np.stack(rows), names


# ---- exception placements ---------------------------------------------------------------------------------------------------------------------------
def placements(prec, seed=12, counts=EXC_COUNTS):
    """(name, ascending positions): the counts around one and two ballots at random distinct positions, the vector's two ends, one whole (m, j) step (all 64
    lanes), one lane's 16 values, every second value"""
    rng = np.random.default_rng(seed)
    out = [(f"{c} random", np.sort(rng.choice(VEC, c, replace=False))) for c in counts]
    out.append(("both ends", np.array([0, VEC - 1])))
    out.append(("first step", prec.step_positions(0, 0)))
    out.append(("last step", prec.step_positions(prec.steps - 1, prec.per_lane - 1)))
    out.append(("a middle step", prec.step_positions(prec.steps // 2, 1)))
    out.append(("lane 0", prec.lane_positions(0)))
    out.append(("lane 63", prec.lane_positions(63)))
    out.append(("lane 37", prec.lane_positions(37)))
    out.append(("every second value", np.arange(0, VEC, 2)))
    out.append(("every other second value", np.arange(1, VEC, 2)))
    return [(name, np.asarray(p, np.int64)) for name, p in out]


def patch_cases(prec, seed=13, counts=EXC_COUNTS):
    """hand-built exception lists for patch_*: every placement ascending, the larger ones also descending; slots beyond cnt hold valid positions and other
    values, which a kernel that ran past cnt would apply.  -> dict(out, exc, pos, cnt, want, names), bit patterns throughout"""
    rng = np.random.default_rng(seed)
    lists = []
    for name, p in placements(prec, seed, counts):
        lists.append((name, p))
        if p.size >= 2:
            lists.append((name + ", descending", p[::-1]))
    N = len(lists)
    out = rng.integers(0, 2**prec.bits, (N, VEC), dtype=np.uint64).astype(prec.udt)
    exc = rng.integers(0, 2**prec.bits, (N, VEC), dtype=np.uint64).astype(prec.udt)
    pos = rng.integers(0, VEC, (N, VEC)).astype(np.uint16)
    cnt = np.array([p.size for _, p in lists], np.uint16)
    for i, (_, p) in enumerate(lists):
        pos[i, :p.size] = p
    want = np.stack([patch_np(out[i], exc[i], pos[i], cnt[i]) for i in range(N)])
    return dict(out=out, exc=exc, pos=pos, cnt=cnt, want=want, names=[n for n, _ in lists])


ALP_PLACED_EF = {64: (14, 12), 32: (6, 5)}  # two-decimal doubles / one-decimal floats encode under these; the exceptions below do not


def alp_placed_vectors(prec, seed=14):
    """two-decimal (float: one-decimal) vectors whose exceptions (NaN, infinities, irrational multiples) sit exactly at each placement's positions -> (vectors, placements)"""
    rng = np.random.default_rng(seed)
    pl = placements(prec, seed)
    x = np.round(rng.uniform(0, 100, (len(pl), VEC)), 2 if prec.bits == 64 else 1).astype(prec.fdt)
    for i, (_, p) in enumerate(pl):
        bad = (np.pi * (np.arange(p.size) + 1) / 7.0 + 0.0001234).astype(prec.fdt)
        bad[::5] = np.nan
        bad[1::11] = np.inf
        x[i, p] = bad
    return x, pl


# ---- rowgroup states ------------------------------------------------------------------------------------------------------------------------------------
def alp_state(pairs):
    """an ALP state with the given (e, f) candidates, best first"""
    s = np.zeros(1, STATE_DTYPE)[0]
    s["scheme"], s["k"] = SCHEME_ALP, len(pairs)
    for i, (e, f) in enumerate(pairs):
        s["combos"][2 * i], s["combos"][2 * i + 1] = e, f
    return s


def states_of_encoding(enc):
    """the rowgroup states of an oracle encode_column result (ALP rowgroups only)"""
    nrg = enc["k"].size
    out = np.zeros(nrg, STATE_DTYPE)
    for r in range(nrg):
        assert enc["scheme"][r * ROWGROUP] == SCHEME_ALP
        k = int(enc["k"][r])
        out[r] = alp_state([(int(enc["combos"][r, 2 * i]), int(enc["combos"][r, 2 * i + 1])) for i in range(k)])
    return out


RD_DICT_SIZES = (1, 2, 3, 4, 5, 6, 7, 8, 8, 7, 6, 5, 4, 3, 2, 1)  # per cut, lowest first: the three highest cuts leave 3, 2 and 1 bits to the left part


def rd_states(prec, seed=15):
    """one ALP_RD state per cut, each with a dictionary of its own (distinct random left parts) and a size that leaves at least one left part outside it"""
    rng = np.random.default_rng(seed)
    out = np.zeros(len(prec.cuts), STATE_DTYPE)
    for i, rbw in enumerate(prec.cuts):
        lbits = prec.bits - rbw
        ds = RD_DICT_SIZES[i]
        assert ds < 2**lbits
        out[i]["scheme"], out[i]["rd_rbw"], out[i]["rd_dict_size"] = SCHEME_ALP_RD, rbw, ds
        out[i]["rd_lbw"] = max(1, (ds - 1).bit_length())
        out[i]["rd_dict"][:ds] = rng.choice(2**lbits, ds, replace=False)
    return out


def rd_vector(prec, rec, positions, rng):
    """the bits of one vector under this state: dictionary entries everywhere but at `positions`, which hold left parts outside the dictionary"""
    rbw, ds = int(rec["rd_rbw"]), int(rec["rd_dict_size"])
    lbits = prec.bits - rbw
    left = rec["rd_dict"][rng.integers(0, ds, VEC)].astype(np.uint64)
    outside = np.setdiff1d(np.arange(2**lbits), rec["rd_dict"][:ds])
    left[positions] = outside[rng.integers(0, outside.size, len(positions))]
    right = rng.integers(0, 2**rbw, VEC, dtype=np.uint64)
    return ((left << np.uint64(rbw)) | right).astype(prec.udt)


def rd_batch(prec, states, state_idx, position_lists, seed=16):
    """vectors (bit patterns) for the given state and exception positions each, with the numpy restatement's encoding of them: right, left, exc, pos (unused
    slots hold the sentinel), cnt"""
    rng = np.random.default_rng(seed)
    N = len(position_lists)
    b = dict(bits=np.empty((N, VEC), prec.udt), right=np.empty((N, VEC), prec.udt), left=np.empty((N, VEC), np.uint16),
             exc=np.full((N, VEC), sentinel(np.uint16)), pos=np.full((N, VEC), sentinel(np.uint16)), cnt=np.zeros(N, np.uint16),
             state_idx=np.asarray(state_idx, np.uint32))
    for i, p in enumerate(position_lists):
        rec = states[int(state_idx[i])]
        b["bits"][i] = rd_vector(prec, rec, p, rng)
        r, l, x, q, c = rd_encode_np(prec, b["bits"][i], rec)
        b["right"][i], b["left"][i], b["cnt"][i] = r, l, c
        b["exc"][i, :c], b["pos"][i, :c] = x, q
    return b


# ---- ALP encode patterns for the big batch ---------------------------------------------------------------------------------------------------------------
BIG_EXC_STRIDE = 64
K1_PAIRS = {64: ((14, 9), (14, 8), (14, 7)), 32: ((6, 1), (6, 2), (6, 3))}  # candidates under which every pattern below has few exceptions (the CPU test counts)


def alp_patterns(prec, P=35, seed=17):
    """P vectors of 1..5 (float: 1..3) decimals, drawn as datagen.drifting_column draws its own, with up to 30 (float: 16) exceptions put at random positions, beside
    the few (float: up to 44) that the decimals leave of their own"""
    rng = np.random.default_rng(seed)
    decimals = (1, 3, 5, 2) if prec.bits == 64 else (1, 2, 3, 2)
    hi = 1000 if prec.bits == 64 else 100
    x = np.empty((P, VEC), prec.fdt)
    for p in range(P):
        x[p] = np.round(rng.uniform(0, hi, VEC), decimals[p % 4]).astype(prec.fdt)
        c = int(rng.integers(0, 17 if prec.bits == 32 else 31))
        at = rng.choice(VEC, c, replace=False)
        x[p, at] = rng.choice(np.array([np.nan, np.inf, -np.inf, np.pi * 1e-3, -np.e * 1e-5], prec.fdt), c)
    return x


def drifting_states(o, prec, seed=7):
    """the k > 1 states of the oracle's encoding of a drifting column"""
    col = datagen.drifting_column(200, seed) if prec.bits == 64 else datagen.drifting_column_f32(200, seed)
    enc = o.encode_column(col)
    alp = [r for r in range(enc["k"].size) if enc["scheme"][r * ROWGROUP] == SCHEME_ALP and enc["k"][r] > 1]
    return np.array([alp_state([(int(enc["combos"][r, 2 * i]), int(enc["combos"][r, 2 * i + 1])) for i in range(int(enc["k"][r]))]) for r in alp], STATE_DTYPE)


def alternating_states(o, prec):
    """distinct states, k > 1 at the even places and k = 1 at the odd ones"""
    many = drifting_states(o, prec)
    assert many.size >= 1
    out = np.zeros(6, STATE_DTYPE)
    for i in range(3):
        out[2 * i] = many[i % many.size]
        out[2 * i + 1] = alp_state([K1_PAIRS[prec.bits][i]])
    return out


def simdized_expectations(o, prec, x, exp, fac, exc_stride=VEC):
    """the oracle's encode_simdized of row i of x under (exp[i], fac[i]) -> dict(x, exp, fac, cnt, enc, exc, pos); exc / pos rows are exc_stride long and hold
    the sentinel beyond cnt (bit patterns); a count above exc_stride is kept in cnt (the CPU test refuses such a batch)"""
    N = x.shape[0]
    w = dict(x=np.ascontiguousarray(x).view(prec.udt), exp=np.asarray(exp, np.uint8), fac=np.asarray(fac, np.uint8), cnt=np.zeros(N, np.uint16),
             enc=np.zeros((N, VEC), prec.idt), exc=np.full((N, exc_stride), sentinel(prec.udt)), pos=np.full((N, exc_stride), sentinel(np.uint16)))
    for i in range(N):
        enc, exc, pos, cnt = o.encode_simdized(x[i], int(fac[i]), int(exp[i]))
        w["cnt"][i], w["enc"][i] = cnt, enc
        c = min(cnt, exc_stride)
        w["exc"][i, :c], w["pos"][i, :c] = exc[:c].view(prec.udt), pos[:c]
    return w


def encode_values_expectations(o, prec, x, states, exc_stride):
    """every pattern under every state, row p * len(states) + s: encoder::encode's choice of (e, f), then encode_simdized"""
    P, S = x.shape[0], states.size
    ef = [oracle_find_best_ef(o, prec, states[s], x[p]) for p in range(P) for s in range(S)]
    return simdized_expectations(o, prec, np.repeat(x, S, axis=0), [e for e, f in ef], [f for e, f in ef], exc_stride)


def restride(rows, stride, fill):
    """[N, 1024] rows as [N, stride]: cut, or padded with `fill`"""
    out = np.full((rows.shape[0], stride), fill, rows.dtype)
    w = min(stride, rows.shape[1])
    out[:, :w] = rows[:, :w]
    return out
