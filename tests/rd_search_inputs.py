"""Inputs for the ALP_RD search and encode tests (tests/test_rd_search_cpu.py, tests/test_rd_search_gpu.py): numpy only, seeded, both precisions.

ALP_RD is bitwise, so values are built as bit patterns: B = 64 or 32, a value is (left16 << (B - 16)) | low with the 16-bit left part chosen
and `low` uniformly random; arrays are unsigned integers viewed as floats.  NaN payloads, infinities and denormals occur and are wanted.  Random
low bits leave the (e,f) search nothing that round-trips, so every column takes the ALP_RD scheme on its own.

A rowgroup's first-level samples are the values 0, 32, .., 992 of its vectors 0, 12, .., 96 (sampler.hpp:29-49): rowgroups of 1, 13, 25 and
100 vectors have 32, 64, 96 and 288 samples.

(a) cut_ladder       the top k bits of the left part constant, the other 16 - k drawn from a pool of m values with skewed weights: one
                     100-vector rowgroup per (k, m).  Reaches every cut, every dictionary size and every left width.
(b) many_distinct    cut 16, eight heavy (even) left parts and k singletons on sampled positions: D = 8 + k distinct left parts, on both sides
                     of the 13 / 29 / 59 bucket counts and of the sort's 16; rare left parts off the sample, some of them sampled singletons
                     (listed behind the dictionary), some in no sample.
(c) ties_at_eighth   cut 16, heavy parts and t further parts of c samples each that tie across the dictionary's 8th place.
(d) sample_sets      sample arrays for the entry points that take samples directly: all-distinct, equal counts, ascending / descending /
                     organ-pipe counts, keys that collide modulo a bucket count, and (from 255 samples on) a median-of-three adversary that
                     sends the sort of 63 distinct left parts into its heap-sort fallback.
"""
import functools

import numpy as np

VEC = 1024
SAMPLE_SIZES = (1, 2, 17, 31, 32, 33, 64, 96, 255, 256, 287, 288)
POOL_SIZES = (1, 2, 3, 5, 8, 9, 20, 300)
SINGLETONS = (0, 1, 5, 6, 8, 9, 21, 22, 40, 51, 52, 80, 100, 116)
TIES = ((2, 3), (5, 2), (12, 1), (3, 1))
TIE_VECTORS = (1, 13, 25, 100)
BUCKET_COUNTS = (13, 29, 59, 127, 257)


def types(bits):
    """(float type, unsigned type) of a precision"""
    return (np.float64, np.uint64) if bits == 64 else (np.float32, np.uint32)


def sample_index(n_vectors):
    """flat indices of a rowgroup's first-level samples, in sample order; n_vectors <= 100"""
    v = np.arange(0, n_vectors, 12)
    return (v[:, None] * VEC + 32 * np.arange(32)[None, :]).ravel()


def samples_of(column, rowgroup=0):
    """the first-level samples of one rowgroup of a column"""
    rg = column[rowgroup * 100 * VEC:(rowgroup + 1) * 100 * VEC]
    return np.ascontiguousarray(rg[sample_index(rg.size // VEC)])


def from_left(left16, bits, rng):
    """values whose top 16 bits are left16 and whose other bits are random"""
    fdt, udt = types(bits)
    low = rng.integers(0, 1 << (bits - 16), left16.size, dtype=udt)
    return ((left16.astype(udt) << udt(bits - 16)) | low).view(fdt)


@functools.lru_cache(maxsize=None)
def usable_left_parts(bits):
    """the 16-bit left parts a column may use and still be ALP_RD by its own search: those whose exponent keeps every value away from what an
    (e,f) pair can round-trip (integers from 2^mantissa on, short decimals below).  Zero, denormals, huge values, infinities and NaNs stay."""
    left = np.arange(1 << 16)
    x = ((left >> 7) & 0xFF) - 127 if bits == 32 else ((left >> 4) & 0x7FF) - 1023
    return left[(x < -16) | (x > (36 if bits == 32 else 68))]


def _seed(*parts):
    return np.random.default_rng([int(p) for p in parts])


# ---- (a) -------------------------------------------------------------------------------------------------------------------------------------
def cut_ladder_case(bits, k, m, n_vectors=100):
    rng = _seed(1, bits, k, m)
    free = 16 - k
    m = min(m, 1 << free)
    ok = np.zeros(1 << 16, bool)
    ok[usable_left_parts(bits)] = True
    tops = np.nonzero(ok.reshape(1 << k, 1 << free).sum(axis=1) >= m)[0]  # values of the top k bits under which m usable left parts exist
    top = int(rng.choice(tops)) << free
    pool = rng.choice(np.nonzero(ok[top:top + (1 << free)])[0], m, replace=False)
    w = rng.random(m) ** 3
    left = top | pool[rng.choice(m, n_vectors * VEC, p=w / w.sum())]
    return from_left(left.astype(np.uint16), bits, rng)


def cut_ladder(bits):
    return {f"ladder_k{k}_m{m}": cut_ladder_case(bits, k, m) for k in range(16) for m in POOL_SIZES}


# ---- (b) -------------------------------------------------------------------------------------------------------------------------------------
def many_distinct_case(bits, k, round_robin, n_vectors=100):
    rng = _seed(2, bits, k, int(round_robin))
    # eight heavy parts, even and still eight distinct values without their last bit; every other part is odd
    usable = usable_left_parts(bits)
    heavy = rng.choice(usable[usable % 2 == 0], 8, replace=False).astype(np.uint16)
    others = rng.choice(usable[usable % 2 == 1], k + 40, replace=False).astype(np.uint16)
    singles, unsampled = others[:k], others[k:]
    n = n_vectors * VEC
    w = rng.random(8) + 0.05
    left = heavy[rng.choice(8, n, p=w / w.sum())]
    smp = sample_index(n_vectors)
    slots = rng.permutation(smp.size)
    left[smp[slots[:k]]] = singles
    rest = smp[slots[k:]]
    if round_robin:
        left[rest] = heavy[np.arange(rest.size) % 8]
    else:
        left[rest[:8]] = heavy  # every heavy part is sampled at least once
    # ~3000 rare left parts off the sample: sampled singletons (sorted positions 8, 9, ..) and parts that are in no sample.  Vector 1 keeps
    # none (no exception), vector 2 takes 300 of them (the wide exception record), the others share the rest.
    is_smp = np.zeros(n, bool)
    is_smp[smp] = True
    rare = np.concatenate([singles, unsampled])
    free = np.nonzero(~is_smp)[0]
    free = free[(free // VEC != 1) & (free // VEC != 2)]
    at = np.concatenate([rng.choice(free, min(2700, free.size), replace=False), 2 * VEC + rng.choice(VEC, 300, replace=False)]) if n_vectors > 2 else free[:0]
    left[at] = rare[rng.integers(0, rare.size, at.size)]
    return from_left(left, bits, rng)


def many_distinct(bits):
    return {f"distinct_k{k}_{'rr' if rr else 'rnd'}": many_distinct_case(bits, k, rr) for k in SINGLETONS for rr in (False, True)}


# ---- (c) -------------------------------------------------------------------------------------------------------------------------------------
def ties_parts(bits, t, c, n_vectors):
    """(heavy parts, tied parts, sample counts of the heavy parts) of a ties case.  Seven heavy parts with distinct counts above c where the
    sample has room for them (64 samples and more); a 32-sample rowgroup keeps as many heavy parts, with counts above c, as fit."""
    rng = _seed(3, bits, t, c, n_vectors)
    parts = rng.choice(usable_left_parts(bits), 7 + t, replace=False).astype(np.uint16)
    room = sample_index(n_vectors).size - t * c
    counts = np.arange(c + 1, c + 8)
    if counts.sum() > room:
        counts = np.full(min(7, room // (c + 1)), c + 1)
    counts = counts.copy()
    counts[-1] += room - counts.sum()
    return parts[:counts.size], parts[7:], counts, rng


def ties_case(bits, t, c, n_vectors):
    heavy, tied, counts, rng = ties_parts(bits, t, c, n_vectors)
    n = n_vectors * VEC
    # off the sample the tied parts are as frequent as the heavy ones: every vector's exception count shows which of them the dictionary holds
    allp = np.concatenate([heavy, tied])
    left = allp[rng.integers(0, allp.size, n)]
    smp = sample_index(n_vectors)
    left[smp[rng.permutation(smp.size)]] = np.concatenate([np.repeat(heavy, counts), np.repeat(tied, c)])
    return from_left(left, bits, rng)


def ties_at_eighth(bits):
    return {f"ties_t{t}_c{c}_v{nv}": ties_case(bits, t, c, nv) for t, c in TIES for nv in TIE_VECTORS}


@functools.lru_cache(maxsize=None)
def columns(bits):
    """every column of (a) to (c): {name: array}; treat the arrays as read-only"""
    out = {}
    out.update(cut_ladder(bits))
    out.update(many_distinct(bits))
    out.update(ties_at_eighth(bits))
    for a in out.values():
        a.setflags(write=False)
    return out


def rowgroup_cases(bits):
    """names of the 100-vector (one whole rowgroup) columns, in a fixed order"""
    return [nm for nm, a in columns(bits).items() if a.size == 100 * VEC]


@functools.lru_cache(maxsize=None)
def joined_column(bits):
    """all 100-vector cases as the rowgroups of one column"""
    cols = columns(bits)
    a = np.concatenate([cols[nm] for nm in rowgroup_cases(bits)])
    a.setflags(write=False)
    return a


# ---- (d) -------------------------------------------------------------------------------------------------------------------------------------
def _lay_out(parts, counts, rng):
    """left parts of a sample in which parts[i] occurs counts[i] times and first occurs before parts[i + 1] does; the further occurrences of
    a part lie anywhere behind its first one"""
    pending = list(rng.permutation(np.repeat(np.arange(len(parts)), np.asarray(counts) - 1)))
    seq, seen, total = [], 0, int(np.sum(counts))
    while len(seq) < total:
        usable = next((j for j, p in enumerate(pending) if p < seen), None)
        if seen < len(parts) and (usable is None or rng.random() < 0.5):
            seq.append(seen)
            seen += 1
        else:
            seq.append(pending.pop(usable))
    return np.asarray(parts, np.uint16)[np.array(seq, int)]


def _count_shapes(n):
    """{name: counts in first-occurrence order} that sum to n: ascending, descending and organ-pipe"""
    d = 1
    while (d + 1) * (d + 2) // 2 <= n:
        d += 1
    asc = np.arange(1, d + 1)
    asc[-1] += n - asc.sum()
    pipe = np.concatenate([asc[0::2], asc[1::2][::-1]])
    return {"ascending": asc, "descending": asc[::-1].copy(), "organ_pipe": pipe}


# ---- (d), the sort's heap-sort fallback ------------------------------------------------------------------------------------------------------
def _node_list_order(d):
    """the unordered_map's iteration order for the keys 0..d-1 inserted in this order: every key opens an empty bucket and goes to the front of
    the node list, and each rehash (13, 29, 59, 127, 257, 541 buckets) re-inserts the nodes front to back, which reverses the list"""
    order, buckets = [], 1
    for key in range(d):
        if key + 1 > (buckets if buckets > 1 else 0):
            buckets = next(p for p in (13, 29, 59, 127, 257, 541) if p >= max(key + 2, 2 * buckets, 12))
            order.reverse()
        order.insert(0, key)
    return order


def median_of_three_adversary(d):
    """counts, by position in the array std::sort receives, that drive libstdc++'s introsort of d elements (descending by count) through
    2 * floor(log2 d) bad partitions into its heap-sort fallback, or None if d elements do not get there.  McIlroy's adversary: an element is
    'gas' (count 1: all tied, sorted last) until a comparison between two gas elements forces one to become solid, with a count below every
    earlier solid's; the sort is followed (median of first + 1 / middle / last - 1 to the front, unguarded partition, the right part pending)
    until a range of more than 16 elements is left at depth 0."""
    rank, solid, cand = [None] * d, [0], [0]

    def before(x, y):
        if rank[x] is None and rank[y] is None:
            z = x if x == cand[0] else y
            rank[z], solid[0] = solid[0], solid[0] + 1
        if rank[x] is None:
            cand[0] = x
            return False
        if rank[y] is None:
            cand[0] = y
            return True
        return rank[x] < rank[y]

    s = list(range(d))
    pending = [(0, d, 2 * (d.bit_length() - 1))]
    while pending:
        first, last, depth = pending.pop()
        while last - first > 16:
            if depth == 0:
                return np.array([1 if r is None else 1 + solid[0] - r for r in rank])
            depth -= 1
            a, b, c = first + 1, first + (last - first) // 2, last - 1
            if before(s[a], s[b]):
                m = b if before(s[b], s[c]) else (c if before(s[a], s[c]) else a)
            else:
                m = a if before(s[a], s[c]) else (c if before(s[b], s[c]) else b)
            s[first], s[m] = s[m], s[first]
            lo, hi = first + 1, last
            while True:
                while before(s[lo], s[first]):
                    lo += 1
                hi -= 1
                while before(s[first], s[hi]):
                    hi -= 1
                if not lo < hi:
                    break
                s[lo], s[hi] = s[hi], s[lo]
                lo += 1
            pending.append((lo, last, depth))
            last = lo
    return None


def heap_sort_left_parts(n):
    """left parts of an n-sample set (cut 16: the keys 0..d-1 in order of first occurrence) whose sort falls back to heap sort; None where
    n samples do not suffice (the counts of the solid elements alone take 230 samples)"""
    for d in range(63, 32, -1):
        counts = median_of_three_adversary(d)
        if counts is not None and counts.sum() <= n:
            counts[np.argmax(counts)] += n - counts.sum()  # (the most frequent part stays the most frequent)
            by_key = np.zeros(d, int)
            by_key[_node_list_order(d)] = counts
            return _lay_out(np.arange(d), by_key, _seed(6, n))
    return None


def sample_left_parts(n, rng_tag=0):
    """{family: uint16 left parts of an n-sample set}"""
    out = {}
    rng = _seed(4, n, rng_tag)
    out["all_distinct"] = rng.choice(1 << 16, n, replace=False).astype(np.uint16)
    for c in (2, 4):
        d = -(-n // c)
        parts = rng.choice(1 << 16, d, replace=False)
        out[f"equal_counts_{c}"] = rng.permutation(np.repeat(parts, c)[:n]).astype(np.uint16)
    for nm, counts in _count_shapes(n).items():
        out[f"counts_{nm}"] = _lay_out(rng.choice(1 << 16, counts.size, replace=False), counts, rng)
    for p in BUCKET_COUNTS:
        # half of the keys are multiples of the bucket count (one bucket), the others small keys that each open an empty bucket
        half = min(n // 2, 65535 // p)
        keys = np.concatenate([p * (1 + rng.choice(65535 // p, half, replace=False)), 1 + rng.choice(p - 1, min(n - half, p - 1), replace=False)])
        keys = np.unique(keys)
        fill = np.setdiff1d(rng.choice(1 << 16, 2 * n + 8, replace=False), keys)[:n - keys.size]
        out[f"collide_mod_{p}"] = rng.permutation(np.concatenate([keys, fill])).astype(np.uint16)
    adversary = heap_sort_left_parts(n)
    if adversary is not None:
        out["heap_sort_fallback"] = adversary
    return out


@functools.lru_cache(maxsize=None)
def synthetic_sample_sets(bits):
    """{name: samples} of the built families of (d), every family at every sample count"""
    out = {}
    for n in SAMPLE_SIZES:
        for fam, left in sample_left_parts(n).items():
            assert left.size == n
            a = from_left(left, bits, _seed(5, bits, n, len(out)))
            a.setflags(write=False)
            out[f"{fam}_n{n}"] = a
    return out


@functools.lru_cache(maxsize=None)
def column_sample_sets(bits):
    """{name: samples}: the first-level samples of every column of (a) to (c)"""
    return {f"smp_{nm}": samples_of(a) for nm, a in columns(bits).items()}


def sample_sets(bits):
    out = dict(synthetic_sample_sets(bits))
    out.update(column_sample_sets(bits))
    return out


def first_occurrence_counts(samples, cut):
    """[(left part, count)] of a sample set at a cut, in order of first occurrence: what the dictionary order is decided from"""
    fdt, udt = types(samples.dtype.itemsize * 8)
    left = samples.view(udt) >> udt(samples.dtype.itemsize * 8 - cut)
    parts, first, counts = np.unique(left, return_index=True, return_counts=True)
    order = np.argsort(first)
    return [(int(parts[i]), int(counts[i])) for i in order]
