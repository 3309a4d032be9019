"""The rules a serialized column (blob) and a device column's descriptors must satisfy, in Python integers: the exact reference for alp_amd/csrc/blob_check.hpp
(behind alpgpu_column_from_blob*, alpgpu_decompress_host_* and alpgpu_column_validate).  Written from include/alpgpu.h's description of the records and of
what alpgpu_column_from_blob accepts, not from the C++: Python integers cannot wrap, so sums and products here are simply formed and compared.  numpy and struct only.

A verdict names every rule the lowest offending vector breaks (or "header"), so that a case meant to cross one bound can be shown to cross nothing else:
    header    size, magic / version / header_bytes, value type, n_rowgroups, n_values inside the last vector, the 2^56 caps, the blob's size against `size`
    scheme    a descriptor's scheme is neither ALP nor ALP_RD, or differs from its rowgroup's
    field     a width, e / f or the exception count is out of range (or an ALP_RD width differs from its rowgroup's)
    extent    a record is misaligned or does not lie inside its stream
    window    chunked route only: a chunk's offsets do not ascend, or a non-empty record lies outside its chunk's stream ranges
    position  an exception position is >= 1024 (looked at only where scheme, field and extent hold: only then is it known where the positions are)
`detail` is the first check that fails, in the order the library reports its errors; TEXT maps it to the error text of the public entry points."""
import struct

import numpy as np

SCHEME_ALP_RD, SCHEME_ALP = 1, 2
RULES = ("header", "scheme", "field", "extent", "window", "position")
ORDER = ("scheme", "field", "extent", "window", "position")  # per vector: which broken rule the library reports
HEADER = struct.Struct("<8sIIQQQQQQ")   # magic, version, header_bytes, n_values, n_vectors, n_rowgroups, packed_bytes, exc_bytes, reserved
DESC = struct.Struct("<QQqBBBBHH")      # packed_off, exc_off, base, bw, e, f, lbw, exc_cnt, scheme
STATE = struct.Struct("<BB10sBBBB16s")  # scheme, k, combos, rd_rbw, rd_lbw, rd_dict_size, pad, rd_dict
assert HEADER.size == 64 and DESC.size == 32 and STATE.size == 32
HEADER_FIELDS = {"version": ("<I", 8), "header_bytes": ("<I", 12), "n_values": ("<Q", 16), "n_vectors": ("<Q", 24), "n_rowgroups": ("<Q", 32),
                 "packed_bytes": ("<Q", 40), "exc_bytes": ("<Q", 48), "reserved": ("<Q", 56)}
TEXT = {
    "short": "blob shorter than its header", "identity": "not an ALPGPU v1 blob", "type": "blob holds a column of the other value type",
    "inconsistent": "inconsistent blob header", "truncated": "blob truncated", "scheme": "blob: bad scheme in a descriptor",
    "field": "blob: descriptor field out of range", "extent": "blob: descriptor extent outside its stream",
    "order": "blob: stream offsets do not ascend with the vector index", "record": "blob: a vector's record lies outside its chunk's stream range",
    "position": "blob: exception position out of range"}


class Verdict:
    def __init__(self, rules=(), first_bad=None, detail=None):
        self.rules, self.first_bad, self.detail = frozenset(rules), first_bad, detail
        self.ok = not self.rules

    def __repr__(self):
        return "accept" if self.ok else "refuse(%s at %s: %s)" % ("+".join(sorted(self.rules)), self.first_bad, self.detail)

    def line(self):
        """what tests/cpp/blob_check_test.cpp prints for this verdict"""
        return "accept - -" if self.ok else "refuse %s %s" % (self.detail, "-" if self.first_bad is None else self.first_bad)


def align8(x):
    return (x + 7) // 8 * 8


def build_blob(rg, vec, packed, exc, n_values, value_bytes):
    """the blob of a column given as tests/layout.py: compact returns it: header, rowgroup states, descriptors, the packed stream padded to 8 bytes, the exception stream"""
    rg8, vec8 = np.ascontiguousarray(rg).view(np.uint8).reshape(-1), np.ascontiguousarray(vec).view(np.uint8).reshape(-1)
    assert rg8.size % 32 == 0 and vec8.size % 32 == 0 and value_bytes in (8, 4)
    n = vec8.size // 32
    assert rg8.size // 32 == (n + 99) // 100
    hdr = HEADER.pack(b"ALPGPU1\0", 1, 64, n_values, n, rg8.size // 32, packed.size, exc.size, 0 if value_bytes == 8 else 4)
    parts = [np.frombuffer(hdr, np.uint8), rg8, vec8, packed.view(np.uint8), np.zeros(align8(packed.size) - packed.size, np.uint8), exc.view(np.uint8),
             np.zeros(align8(exc.size) - exc.size, np.uint8)]
    return np.concatenate(parts)


def set_header(blob, **fields):
    for k, v in fields.items():
        fmt, at = HEADER_FIELDS[k]
        struct.pack_into(fmt, blob, at, v)


def check_header(blob, size, value_bytes):
    """-> (detail or None, header fields)"""
    if size < 64:
        return "short", None
    magic, version, header_bytes, n_values, n, nrg, pb, eb, reserved = h = HEADER.unpack_from(blob, 0)
    if magic != b"ALPGPU1\0" or version != 1 or header_bytes != 64:
        return "identity", h
    if {0: 8, 8: 8, 4: 4}.get(reserved) != value_bytes:
        return "type", h
    if nrg != (n + 99) // 100:
        return "inconsistent", h
    if not ((n == 0 and n_values == 0) or (n > 0 and (n - 1) * 1024 < n_values <= n * 1024)):
        return "inconsistent", h
    if pb > 2**56 or eb > 2**56 or 64 + 32 * nrg + 32 * n + align8(pb) + align8(eb) > size:
        return "truncated", h
    return None, h


def vector_rules(d, st, value_bytes, packed_bytes, exc_bytes, exc_stream, exc_at, window=None):
    """the rules one descriptor breaks.  d: DESC fields, st: STATE fields of its rowgroup, exc_stream[exc_at + o]: byte o of the exception stream"""
    packed_off, exc_off, _base, bw, e, f, lbw, cnt, scheme = d
    alp, rd = scheme == SCHEME_ALP, scheme == SCHEME_ALP_RD
    vbits, max_e = 8 * value_bytes, 18 if value_bytes == 8 else 10
    broken = set()
    if not (alp or rd) or st[0] != scheme:
        broken.add("scheme")
    if bw > vbits or cnt > 1024:
        broken.add("field")
    if alp and (e > max_e or f > e):
        broken.add("field")
    if rd and (not 1 <= lbw <= 3 or bw > vbits - 1 or bw != st[3] or lbw != st[4]):
        broken.add("field")
    psz = 128 * (bw + (lbw if rd else 0))   # ALP: bw words per lane; ALP_RD: the right words, then the left ones
    value_size = value_bytes if alp else 2  # an exception's value: the float itself, or a 16-bit left part
    esz = align8((value_size + 2) * cnt)
    if packed_off % 128 or exc_off % 8 or packed_off + psz > packed_bytes or exc_off + esz > exc_bytes:
        broken.add("extent")
    if not broken and window is not None:
        if (psz and not (window[0] <= packed_off and packed_off + psz <= window[1])) or (esz and not (window[2] <= exc_off and exc_off + esz <= window[3])):
            broken.add("window")
    if not broken - {"window"} and cnt:
        at = exc_at + exc_off + value_size * cnt
        pos = np.frombuffer(bytes(exc_stream[at:at + 2 * cnt]), "<u2")
        if int(pos.max()) >= 1024:
            broken.add("position")
    return broken


def _first(broken):
    return next(r for r in ORDER if r in broken)


def check_blob(blob, size, value_bytes, chunk=None, ranges=None):
    """blob: uint8 array of at least `size` bytes of which the library may read the first `size`.  chunk = None: the one-piece route (alpgpu_column_from_blob).
    chunk = c: the chunked host route, chunks of c vectors over each of `ranges` (default: the whole column) in turn"""
    detail, h = check_header(blob, size, value_bytes)
    if detail:
        return Verdict({"header"}, None, detail)
    _, _, _, _, n, nrg, pb, eb, _ = h
    rg_at, vec_at = 64, 64 + 32 * nrg
    exc_at = vec_at + 32 * n + align8(pb)
    desc = lambda v: DESC.unpack_from(blob, vec_at + 32 * v)

    def scan(v0, v1, window):
        for v in range(v0, v1):
            broken = vector_rules(desc(v), STATE.unpack_from(blob, rg_at + 32 * (v // 100)), value_bytes, pb, eb, blob, exc_at, window)
            if broken:
                r = _first(broken)
                return Verdict(broken, v, "record" if r == "window" else r)
        return None

    if chunk is None:
        return scan(0, n, None) or Verdict()
    for v_begin, v_end in (ranges if ranges is not None else [(0, n)]):
        if v_begin >= v_end:
            continue
        ends = lambda v: (desc(v)[0], desc(v)[1]) if v < n else (pb, eb)  # where the bytes of vector v begin: the streams are laid out in vector order
        (P0, E0), (P1, E1) = ends(v_begin), ends(v_end)
        if not (P0 <= P1 <= pb and E0 <= E1 <= eb):
            return Verdict({"window"}, v_begin, "order")
        for v0 in range(v_begin, v_end, chunk):
            v1 = min(v0 + chunk, v_end)
            (p0, e0), (p1, e1) = ends(v0), ends(v1)
            if not (P0 <= p0 <= p1 <= P1 and E0 <= e0 <= e1 <= E1):
                return Verdict({"window"}, v0, "order")
            bad = scan(v0, v1, (p0, p1, e0, e1))
            if bad:
                return bad
    return Verdict()


def check_column(rg, vec, exc, packed_capacity, exc_capacity, value_bytes):
    """a device column's descriptors (alpgpu_column_validate): the per-vector rules against the two capacities; exc: the exception buffer's bytes"""
    rg8, vec8 = np.ascontiguousarray(rg).view(np.uint8).reshape(-1), np.ascontiguousarray(vec).view(np.uint8).reshape(-1)
    exc8 = np.ascontiguousarray(exc).view(np.uint8)
    assert exc8.size >= exc_capacity
    for v in range(vec8.size // 32):
        broken = vector_rules(DESC.unpack_from(vec8, 32 * v), STATE.unpack_from(rg8, 32 * (v // 100)), value_bytes, packed_capacity, exc_capacity, exc8, 0)
        if broken:
            return Verdict(broken, v, _first(broken))
    return Verdict()


def shard_ranges(n, k):
    """whole-rowgroup shards of n vectors over k contexts (include/alpgpu.h: alpgpu_compress_host_multi_*): the first nrg % k shards hold one rowgroup more"""
    nrg = (n + 99) // 100
    out, rg0 = [], 0
    for i in range(k):
        rgs = nrg // k + (1 if i < nrg % k else 0)
        out.append((min(rg0 * 100, n), min((rg0 + rgs) * 100, n)))
        rg0 += rgs
    return out
