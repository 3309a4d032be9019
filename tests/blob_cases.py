"""The cases of tests/test_blob_check_cpu.py and tests/test_blob_validate_gpu.py: blobs and device columns on and one step past every bound the validators
hold (alp_amd/csrc/blob_check.hpp), each a named edit of one base column and each naming the ONE rule it is meant to cross (tests/blob_replica.py's names;
None = accepted).  A case that needs room for a larger record moves the vector's record to bytes appended to the stream (the one-piece route lets records lie
anywhere inside the streams), so that it crosses its own bound and no other.

Base columns, double and float, encoded by the oracle on the host: 258 vectors = an ALP rowgroup, an ALP_RD rowgroup, an ALP rowgroup of 58 vectors;
n_values = 258 * 1024 - 7.  258 is the smallest count with a vector on both sides of a rowgroup edge (99 | 100) and of the guard kernel's workgroup edge
(255 | 256 | 257) and a short last rowgroup.  NAMED are the vectors the descriptor and position edits are applied at, where the scheme fits."""
import numpy as np

import blob_replica as br
import datagen
import layout

N_VECTORS = 258
N_VALUES = N_VECTORS * 1024 - 7
NAMED = (0, 99, 100, 199, 200, 255, 256, 257)
ALP, RD = br.SCHEME_ALP, br.SCHEME_ALP_RD
LIE = "lie"  # the header names the value type the caller asks for, the records are the other type's: whatever the replica finds in them, the library must find too


class Base:
    def __init__(self, name, value_bytes, enc, n_values, values=None):
        self.name, self.vb, self.enc, self.n_values, self.values = name, value_bytes, enc, n_values, values
        self.rg, self.vec, self.packed, self.exc = layout.compact(enc, value_bytes)
        self.n = self.vec.size
        self.blob = br.build_blob(self.rg, self.vec, self.packed, self.exc, n_values, value_bytes)
        self.dtype = "f64" if value_bytes == 8 else "f32"


def base_f64(oracle):
    col = np.concatenate([datagen.mixed_column(100, seed=31), datagen.rd_column(100, seed=32), datagen.mixed_column(58, seed=33)])
    return Base("f64", 8, oracle.encode_column(col), N_VALUES, col)


def base_f32(oracle_f32):
    col = np.concatenate([datagen.mixed_column_f32(100, seed=41), datagen.rd_column_f32(100, seed=42), datagen.mixed_column_f32(58, seed=43)])
    return Base("f32", 4, oracle_f32.encode_column(col), N_VALUES, col)


def rows_f64():
    """the accepted extreme: double_rows.py's [alp_rows, rd_rows], every width, every cut, 1 to 1024 exceptions"""
    import double_rows as dr
    enc = dr.concat_encodings([dr.alp_rows(), dr.rd_rows()])
    return Base("rows_f64", 8, enc, enc["scheme"].size * 1024)


def rows_f32():
    import float_rows as fr
    enc = fr.concat_encodings([fr.alp_rows(), fr.rd_rows()])
    return Base("rows_f32", 4, enc, enc["scheme"].size * 1024)


class Parts:
    """a base column's arrays, free to edit; header fields set in `hdr` overwrite what build_blob derives"""

    def __init__(self, base):
        self.base, self.vb = base, base.vb
        self.rg, self.vec, self.packed, self.exc = base.rg.copy(), base.vec.copy(), base.packed.copy(), base.exc.copy()
        self.hdr, self.size, self.magic = {}, None, None

    def blob(self):
        b = br.build_blob(self.rg, self.vec, self.packed, self.exc, self.base.n_values, self.vb)
        br.set_header(b, **self.hdr)
        if self.magic is not None:
            b[self.magic[0]] = self.magic[1]
        return b

    # ---- sizes as the descriptor has them now
    def psz(self, v):
        d = self.vec[v]
        return 128 * (int(d["bw"]) + (int(d["lbw"]) if d["scheme"] == RD else 0))

    def value_size(self, v):
        return self.vb if self.vec[v]["scheme"] == ALP else 2

    def esz(self, v):
        return br.align8((self.value_size(v) + 2) * int(self.vec[v]["exc_cnt"]))

    # ---- records moved to bytes appended to a stream
    def move_packed(self, v, room=None):
        """vector v's packed record copied behind the stream's end (zero-filled up to `room` bytes); its descriptor points there"""
        off, size = int(self.vec[v]["packed_off"]), self.psz(v)
        assert self.packed.size % 128 == 0
        rec = np.zeros(max(size, room or 0), np.uint8)
        rec[:size] = self.packed[off:off + size]
        self.vec["packed_off"][v] = self.packed.size
        self.packed = np.concatenate([self.packed, rec])

    def move_exc(self, v, record=None):
        """vector v's exception record (or `record`) appended to the exception stream, padded to 8 bytes; its descriptor points there"""
        off, size = int(self.vec[v]["exc_off"]), self.esz(v)
        rec = self.exc[off:off + size] if record is None else record
        assert self.exc.size % 8 == 0
        self.vec["exc_off"][v] = self.exc.size
        self.exc = np.concatenate([self.exc, rec, np.zeros(br.align8(rec.size) - rec.size, np.uint8)])

    def record_of(self, v, cnt):
        """a well-formed exception record of cnt entries for vector v's scheme: the vector's own values repeated, positions 0, 1, 2 ... below 1024"""
        vs, have = self.value_size(v), int(self.vec[v]["exc_cnt"])
        off = int(self.vec[v]["exc_off"])
        vals = np.resize(self.exc[off:off + vs * have], vs * cnt) if have else np.zeros(vs * cnt, np.uint8)
        return np.concatenate([vals, (np.arange(cnt) % 1024).astype("<u2").view(np.uint8)])

    def set_rd_widths(self, r, rbw, lbw):
        """ALP_RD rowgroup r and every vector of it given these widths, each record moved behind the stream's end with room for them"""
        self.rg["rd_rbw"][r], self.rg["rd_lbw"][r] = rbw, lbw
        for v in range(100 * r, min(100 * r + 100, self.vec.size)):
            assert self.vec[v]["scheme"] == RD
            self.move_packed(v, 128 * (rbw + lbw))
            self.vec["bw"][v], self.vec["lbw"][v] = rbw, lbw

    def positions_at(self, v):
        return int(self.vec[v]["exc_off"]) + self.value_size(v) * int(self.vec[v]["exc_cnt"])


class Case:
    """a named edit of a base column; built afresh on demand (a built case is a copy of the whole column)"""

    def __init__(self, base, name, rule, edit, kind, bad=None, same=False, size=None, check_vb=None, chunk=None, ranges=None):
        self.base, self.name, self.rule, self.edit, self.kind, self.bad, self.same = base, base.name + ":" + name, rule, edit, kind, bad, same
        self.fixed_size = size
        self.vb = base.vb if check_vb is None else check_vb
        self.chunk, self.ranges = chunk, ranges
        self.has_column = kind in ("descriptor", "position", "unused")  # alpgpu_column_validate is given the edited arrays

    def build(self):
        """-> (blob, size, parts): the bytes, how many of them the library is told it may read, and the edited arrays"""
        p = Parts(self.base)
        self.edit(p)
        blob = p.blob()
        if self.fixed_size is not None and self.fixed_size > blob.size:  # bytes behind the blob that the caller owns as well
            blob = np.concatenate([blob, np.full(self.fixed_size - blob.size, 0xEE, np.uint8)])
        return blob, blob.size if self.fixed_size is None else self.fixed_size, p


def cases(base):
    """every one-piece case of a 258-vector base column"""
    out = []
    vb, vbits, max_e, n = base.vb, 8 * base.vb, 18 if base.vb == 8 else 10, base.n
    alp_vs = [v for v in NAMED if base.vec[v]["scheme"] == ALP]
    rd_vs = [v for v in NAMED if base.vec[v]["scheme"] == RD]
    exact = base.blob.size

    def add(name, rule, edit, kind, **kw):
        out.append(Case(base, name, rule, edit, kind, **kw))

    def hdr(name, rule, same=False, size=None, **fields):
        add(name, rule, lambda p: p.hdr.update(fields), "header", same=same, size=size)

    # ---- header ----------------------------------------------------------------------------------------------------------------------------------
    add("unedited", None, lambda p: None, "header", same=True)
    for i in range(8):
        add("magic[%d]" % i, "header", lambda p, i=i: setattr(p, "magic", (i, base.blob[i] ^ 0x20)), "header")
    for k, vals in (("version", (0, 2)), ("header_bytes", (0, 63, 65))):
        for x in vals:
            hdr("%s=%d" % (k, x), "header", **{k: x})
    for r in (0, 8, 4, 1, 16, 2**32 + 4):
        for check in (8, 4):
            named = {0: 8, 8: 8, 4: 4}.get(r)
            rule = "header" if named != check else (None if check == vb else LIE)
            add("reserved=%d as %d" % (r, check), rule, lambda p, r=r: p.hdr.update(reserved=r), "header", check_vb=check, same=rule is None)
    nrg = (n + 99) // 100
    hdr("n_rowgroups+1", "header", n_rowgroups=nrg + 1)
    hdr("n_rowgroups-1", "header", n_rowgroups=nrg - 1)
    hdr("n_values=n*1024", None, same=True, n_values=n * 1024)
    hdr("n_values=n*1024+1", "header", n_values=n * 1024 + 1)
    hdr("n_values=(n-1)*1024+1", None, same=True, n_values=(n - 1) * 1024 + 1)
    hdr("n_values=(n-1)*1024", "header", n_values=(n - 1) * 1024)
    hdr("n_values=0", "header", n_values=0)
    hdr("empty column", None, size=64, n_vectors=0, n_rowgroups=0, n_values=0, packed_bytes=0, exc_bytes=0)
    hdr("empty column, n_values=1", "header", size=64, n_vectors=0, n_rowgroups=0, n_values=1, packed_bytes=0, exc_bytes=0)
    for k, have in (("packed_bytes", base.packed.size), ("exc_bytes", base.exc.size)):
        for label, x in (("+8", have + 8), ("2^56", 2**56), ("2^56+8", 2**56 + 8), ("2^63", 2**63), ("2^64-8", 2**64 - 8)):
            hdr("%s=%s" % (k, label), "header", **{k: x})
    for label, size, rule in (("0", 0, "header"), ("63", 63, "header"), ("64", 64, "header"), ("exact-1", exact - 1, "header"), ("exact", exact, None),
                              ("exact+5", exact + 5, None)):
        add("size=" + label, rule, lambda p: None, "header", size=size, same=rule is None)
    # the wrap family: headers whose sums, products or rounded-up quotients leave 64 bits
    quoted = 0x7ebb9079a9d2605
    wraps = (("32*nrg+32*n=2^64", dict(n_vectors=quoted, n_rowgroups=5707532201023995, n_values=12602231099860980736, packed_bytes=0, exc_bytes=0)),
             ("n=2^54", dict(n_vectors=2**54, n_rowgroups=(2**54 + 99) // 100, n_values=0)),
             ("n=2^64-1", dict(n_vectors=2**64 - 1, n_rowgroups=((2**64 - 1 + 99) % 2**64) // 100, n_values=((2**64 - 1) * 1024) % 2**64)),
             ("n=2^64-99", dict(n_vectors=2**64 - 99, n_rowgroups=((2**64 - 99 + 99) % 2**64) // 100, n_values=((2**64 - 99) * 1024) % 2**64)))
    assert (quoted + 99) // 100 == 5707532201023995 and (quoted * 1024) % 2**64 == 12602231099860980736 and 32 * 5707532201023995 + 32 * quoted == 2**64
    for label, fields in wraps:
        hdr("wrap %s, size 64" % label, "header", size=64, **fields)
        hdr("wrap %s, size exact" % label, "header", **fields)

    # ---- descriptors -------------------------------------------------------------------------------------------------------------------------------
    def desc(name, rule, v, edit, same=False, bad=None):
        add("%s @%d" % (name, v), rule, lambda p: edit(p, v), "descriptor", bad=(v if bad is None else bad) if rule else None, same=same)

    def field(k, x):
        return lambda p, v: p.vec[k].__setitem__(v, x)

    for v in alp_vs + rd_vs:
        own = int(base.vec[v]["scheme"])
        for s in (0, 3, 7):
            desc("scheme=%d" % s, "scheme", v, field("scheme", s))
        desc("scheme=own", None, v, field("scheme", own), same=True)
        desc("packed_off+64", "extent", v, lambda p, v: p.vec["packed_off"].__setitem__(v, int(p.vec[v]["packed_off"]) + 64))
        desc("exc_off+4", "extent", v, lambda p, v: p.vec["exc_off"].__setitem__(v, int(p.vec[v]["exc_off"]) + 4))

        def packed_at_end(p, v):  # a copy of the record is the stream's tail: packed_bytes - psz is where it begins
            p.move_packed(v)
        desc("packed_off=packed_bytes-psz", None, v, packed_at_end, same=True)

        def packed_past_end(p, v):
            p.move_packed(v)
            p.vec["packed_off"][v] += 128
        desc("packed_off=packed_bytes-psz+128", "extent", v, packed_past_end)
        desc("packed_off=2^63", "extent", v, field("packed_off", 2**63))
        desc("packed_off=2^64-128", "extent", v, field("packed_off", 2**64 - 128))

        def exc_at_end(p, v):
            p.move_exc(v)
        desc("exc_off=exc_bytes-esz", None, v, exc_at_end, same=True)

        def exc_past_end(p, v):
            p.move_exc(v)
            p.vec["exc_off"][v] += 8
        desc("exc_off=exc_bytes-esz+8", "extent", v, exc_past_end)
        desc("exc_off=2^63", "extent", v, field("exc_off", 2**63))
        desc("exc_off=2^64-8", "extent", v, field("exc_off", 2**64 - 8))

        def no_exceptions_at_end(p, v):
            p.vec["exc_cnt"][v], p.vec["exc_off"][v] = 0, p.exc.size
        desc("exc_off=exc_bytes, exc_cnt=0", None, v, no_exceptions_at_end)

        def one_exception_at_end(p, v):
            p.vec["exc_cnt"][v], p.vec["exc_off"][v] = 1, p.exc.size
        desc("exc_off=exc_bytes, exc_cnt=1", "extent", v, one_exception_at_end)

        def cnt_1024(p, v):
            p.move_exc(v, p.record_of(v, 1024))
            p.vec["exc_cnt"][v] = 1024
        desc("exc_cnt=1024", None, v, cnt_1024)

        def cnt_1025(p, v):
            p.move_exc(v, p.record_of(v, 1025))
            p.vec["exc_cnt"][v] = 1025
        desc("exc_cnt=1025", "field", v, cnt_1025)

    for v in alp_vs:
        def to_rd(p, v):  # the vector made a well-formed ALP_RD vector of a rowgroup that is not one: the rowgroup's unused ALP_RD widths set to match
            r, bw = v // 100, min(int(p.vec[v]["bw"]), vbits - 1)
            p.rg["rd_rbw"][r], p.rg["rd_lbw"][r] = bw, 1
            p.move_packed(v, 128 * (bw + 1))
            p.vec["bw"][v], p.vec["lbw"][v], p.vec["scheme"][v] = bw, 1, RD
        desc("scheme=ALP_RD", "scheme", v, to_rd)

        def bw_to(x):
            def edit(p, v):
                p.move_packed(v, 128 * x)
                p.vec["bw"][v] = x
            return edit
        desc("bw=%d" % vbits, None, v, bw_to(vbits))
        desc("bw=%d" % (vbits + 1), "field", v, bw_to(vbits + 1))

        desc("e=%d" % max_e, None, v, lambda p, v: p.vec["e"].__setitem__(v, max_e))
        desc("e=%d" % (max_e + 1), "field", v, lambda p, v: p.vec["e"].__setitem__(v, max_e + 1))
        desc("f=e", None, v, lambda p, v: p.vec["f"].__setitem__(v, int(p.vec[v]["e"])))
        desc("f=e+1", "field", v, lambda p, v: p.vec["f"].__setitem__(v, int(p.vec[v]["e"]) + 1))
        desc("e=f=0", None, v, lambda p, v: (p.vec["e"].__setitem__(v, 0), p.vec["f"].__setitem__(v, 0)) and None)

        def empty_at_end(bw):
            def edit(p, v):
                p.vec["bw"][v], p.vec["packed_off"][v] = bw, p.packed.size
            return edit
        desc("packed_off=packed_bytes, bw=0", None, v, empty_at_end(0))
        desc("packed_off=packed_bytes, bw=1", "extent", v, empty_at_end(1))

    for v in rd_vs:
        r = v // 100
        desc("scheme=ALP", "scheme", v, field("scheme", ALP))  # (an ALP_RD vector's e = f = 0 and its width are in an ALP vector's range as they are)
        rbw, lbw = int(base.rg["rd_rbw"][r]), int(base.rg["rd_lbw"][r])
        desc("bw=rd_rbw=%d" % (vbits - 1), None, v, lambda p, v: p.set_rd_widths(v // 100, vbits - 1, lbw), bad=100 * r)
        desc("bw=rd_rbw=%d" % vbits, "field", v, lambda p, v: p.set_rd_widths(v // 100, vbits, lbw), bad=100 * r)
        desc("bw=rd_rbw-1", "field", v, field("bw", rbw - 1))
        for x, rule in ((0, "field"), (1, None), (3, None), (4, "field")):
            desc("lbw=rd_lbw=%d" % x, rule, v, lambda p, v, x=x: p.set_rd_widths(v // 100, rbw, x), bad=100 * r)

        def other_lbw(p, v):
            x = lbw % 3 + 1
            p.move_packed(v, 128 * (rbw + x))
            p.vec["lbw"][v] = x
        desc("lbw!=rd_lbw", "field", v, other_lbw)

    for r in range(nrg):
        flip = lambda p, v: p.rg["scheme"].__setitem__(v // 100, ALP + RD - int(p.rg["scheme"][v // 100]))
        desc("rowgroup's scheme flipped", "scheme", 100 * r, flip)

    def two_bad(p, v):
        p.vec["packed_off"][257] += 64
        p.vec["packed_off"][100] += 64
    desc("two bad vectors, 257 and", "extent", 100, two_bad)

    # ---- exception positions ------------------------------------------------------------------------------------------------------------------------
    def with_parity(vs, odd):
        return next(v for v in vs if base.vec[v]["exc_cnt"] > 0 and int(base.vec[v]["exc_cnt"]) % 2 == odd)
    rd_all = [v for v in range(n) if base.vec[v]["scheme"] == RD]
    targets = {with_parity(alp_vs, 1), with_parity(alp_vs, 0), with_parity(rd_vs + rd_all, 1), with_parity(rd_vs + rd_all, 0)}
    targets |= {v for v in alp_vs + rd_vs if base.vec[v]["exc_cnt"] > 0}
    for v in sorted(targets):
        cnt = int(base.vec[v]["exc_cnt"])
        for which, j in (("first", 0), ("last", cnt - 1)):
            for x in (1023, 1024, 0x8000, 0xFFFF):
                def edit(p, v, j=j, x=x):
                    p.exc[p.positions_at(v) + 2 * j:p.positions_at(v) + 2 * j + 2] = np.frombuffer(np.uint16(x).tobytes(), np.uint8)
                add("%s position=%d @%d" % (which, x, v), None if x < 1024 else "position", lambda p, v=v, e=edit: e(p, v), "position", bad=v if x >= 1024 else None)

        def loud_value(p, v):  # every 16-bit half of the first exception VALUE is >= 1024: it is not a position
            at = int(p.vec[v]["exc_off"])
            p.exc[at:at + p.value_size(v)] = 0xFF
        add("exception value of 0xFFFF halves @%d" % v, None, lambda p, v=v: loud_value(p, v), "position")

    # ---- fields the header documents as unused for the vector's scheme: accepted, and the decode does not read them -------------------------------------
    p0 = Parts(base)

    def roomy(vs):  # vectors whose packed record is followed by at least 384 bytes of stream
        return [v for v in vs if base.packed.size - (int(base.vec[v]["packed_off"]) + p0.psz(v)) >= 384]
    for v in roomy(alp_vs):
        add("unused lbw=3 @%d" % v, None, lambda p, v=v: p.vec["lbw"].__setitem__(v, 3), "unused", same=True)
    for v in roomy(rd_vs):
        add("unused e=255 @%d" % v, None, lambda p, v=v: p.vec["e"].__setitem__(v, 255), "unused", same=True)
        add("unused f=255 @%d" % v, None, lambda p, v=v: p.vec["f"].__setitem__(v, 255), "unused", same=True)
        add("unused base=-1 @%d" % v, None, lambda p, v=v: p.vec["base"].__setitem__(v, -1), "unused", same=True)
    return out


CHUNK = 4


def window_cases(base):
    """the chunked route's windows, chunks of CHUNK vectors: over the whole column and over the shards of 2 and 3 contexts"""
    out = []
    n = base.n
    range_sets = {"whole": None, "2 contexts": br.shard_ranges(n, 2), "3 contexts": br.shard_ranges(n, 3)}

    def add(name, rule, edit, bad=None, sets=range_sets):
        for label, ranges in sets.items():
            out.append(Case(base, "window %s, %s" % (name, label), rule, edit, "window", bad=bad, chunk=CHUNK, ranges=ranges))

    add("unedited", None, lambda p: None)
    alp, p0 = base.vec["scheme"] == ALP, Parts(base)

    def one_chunk(c):  # chunk c = vectors 4c .. 4c + 3
        v = next(v for v in range(4 * c + 1, 4 * c + 4) if base.vec[v]["exc_cnt"] > 0 and p0.psz(v) > 0)
        for label, src in (("c-1", 4 * (c - 1)), ("c+1", 4 * (c + 1))):
            add("packed record of %d in chunk %s" % (v, label), "window", lambda p, src=src: p.vec["packed_off"].__setitem__(v, p.vec[src]["packed_off"]), bad=v)
            with_exc = next(u for u in range(src, src + 4) if base.vec[u]["exc_cnt"] > 0)  # (that vector's record, whole: its positions are positions)

            def exc_elsewhere(p, u=with_exc):
                p.vec["exc_cnt"][v], p.vec["exc_off"][v] = p.vec[u]["exc_cnt"], p.vec[u]["exc_off"]
            add("exception record of %d in chunk %s" % (v, label), "window", exc_elsewhere, bad=v)
            if alp[v]:
                def empty_packed(p, src=src):
                    p.vec["bw"][v], p.vec["packed_off"][v] = 0, p.vec[src]["packed_off"]
                add("empty packed record of %d in chunk %s" % (v, label), None, empty_packed)

            def empty_exc(p, src=src):
                p.vec["exc_cnt"][v], p.vec["exc_off"][v] = 0, p.vec[src]["exc_off"]
            add("empty exception record of %d in chunk %s" % (v, label), None, empty_exc)
        # the chunk's first descriptor below the chunk before: chunk c - 1's window would end before it begins
        add("first descriptor of chunk %d below chunk %d (packed)" % (c, c - 1), "window",
            lambda p: p.vec["packed_off"].__setitem__(4 * c, int(p.vec[4 * (c - 1)]["packed_off"]) - 128), bad=4 * (c - 1))
        add("first descriptor of chunk %d below chunk %d (exceptions)" % (c, c - 1), "window",
            lambda p: p.vec["exc_off"].__setitem__(4 * c, int(p.vec[4 * (c - 1)]["exc_off"]) - 8), bad=4 * (c - 1))
    one_chunk(10)  # a chunk of an ALP rowgroup
    one_chunk(30)  # a chunk of the ALP_RD rowgroup
    # the last chunk's window ends at the streams' ends: a record of it moved behind everything else is inside, one of an earlier chunk is not
    last = n - 1
    add("last vector's records at the streams' ends", None, lambda p: (p.move_packed(last), p.move_exc(last)) and None)
    add("vector 41's packed record at the stream's end", "window", lambda p: p.move_packed(41), bad=41)
    add("vector 101's packed record in the shard before", "window",
        lambda p: p.vec["packed_off"].__setitem__(101, p.vec[97]["packed_off"]), bad=101)
    return out
