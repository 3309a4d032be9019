"""A small column placed high in its streams: every decoder follows descriptors as found and alpgpu_column_validate bounds a record by the capacities
alone, so a column of a few hundred vectors can lie around byte 2^31 or 2^32 of a large, otherwise untouched buffer.  `place` shifts every packed_off
and every exc_off by one amount each (the records stay contiguous and in vector order, which the flat arm of the streamed float decode relies on);
`placements` names the shifts that put 2^31 / 2^32 on chosen bytes of chosen records.  Host code only; `HighColumn` (the buffers in HBM) imports torch
when it is made.  tests/test_high_offsets_cpu.py checks, without a GPU, that each placement puts its seam where the table below says."""
from collections import namedtuple

import numpy as np

import datagen
import layout
from alp_amd.capi import SCHEME_ALP, SCHEME_ALP_RD

TWO31, TWO32 = 1 << 31, 1 << 32
CAPACITY = TWO32 + (64 << 20)   # of either stream
TWIN_SHIFT = TWO32 + (48 << 20)  # a second copy of the small column in the same buffers (the second operand of the two-column kernels)
TWIN_SHIFT_31 = TWO31 + (256 << 20)  # ... under seam_2_31, whose offsets all fit 32 bits: the twin's do too


def twin_shift(name):
    """where the twin of the small column lies under the placement `name`, in both streams: above the column, on offsets that differ from the column's"""
    return TWIN_SHIFT_31 if name == "seam_2_31" else TWIN_SHIFT
PLACEMENTS = ("seam_2_31", "seam_2_32", "inside", "rd_left", "all_above")
LONG_PLACEMENTS = ("seam_2_31", "seam_2_32", "all_above")  # (the long column has neither exceptions nor ALP_RD vectors)
LONG_VECTORS = 32768 + 300

# where a placement puts its seam: p_shift / e_shift, the seam's byte address, the vector whose record holds it and the byte of that record it is
Placement = namedtuple("Placement", "name p_shift e_shift p_seam e_seam p_vector p_byte e_vector e_byte")


def small_input(dtype):
    """about 500 vectors: one rowgroup of narrow decimals, two of mixed_column with many exceptions per vector, two of ALP_RD"""
    if dtype == "f64":
        return np.concatenate([datagen.decimal_column(100, 1, lo=0.0, hi=100.0, seed=301), datagen.mixed_column(200, seed=302, exc_rate=0.05), datagen.rd_column(200, seed=303)])
    return np.concatenate([datagen.decimal_column_f32(100, 1, hi=10.0, seed=301), datagen.mixed_column_f32(200, seed=302, exc_rate=0.05, decimals_per_rowgroup=(1, 0)), datagen.rd_column_f32(200, seed=303)])


def long_input(dtype):
    """32768 + 300 narrow vectors, decimals of one digit: as many as the launch shapes that ask for a long column want"""
    if dtype == "f64":
        return datagen.decimal_column(LONG_VECTORS, 1, lo=0.0, hi=100.0, seed=311)
    return datagen.decimal_column_f32(LONG_VECTORS, 1, hi=10.0, seed=311)


def sizes(vec, value_bytes):
    return layout.record_sizes(vec["scheme"], vec["bw"], vec["lbw"], vec["exc_cnt"], value_bytes)


def place(rg, vec, packed, exc, value_bytes, p_shift, e_shift):
    """new descriptors: every packed_off + p_shift (a multiple of 128), every exc_off + e_shift (a multiple of 8)"""
    assert p_shift % 128 == 0 and e_shift % 8 == 0 and p_shift >= 0 and e_shift >= 0
    psz, esz = sizes(vec, value_bytes)
    assert int((vec["packed_off"].astype(np.int64) + psz).max()) <= packed.size and int((vec["exc_off"].astype(np.int64) + esz).max()) <= exc.size
    out = vec.copy()
    out["packed_off"] += np.uint64(p_shift)
    out["exc_off"] += np.uint64(e_shift)
    return out


def _middle(candidates, what):
    assert candidates.size, f"the column has no {what}"
    return int(candidates[candidates.size // 2])


def placements(vec, value_bytes, names=PLACEMENTS):
    """{name: Placement} for descriptors whose records are contiguous from offset 0 (layout.compact's, the ordered encoder's)"""
    W = value_bytes
    psz, esz = sizes(vec, W)
    poff, eoff = vec["packed_off"].astype(np.int64), vec["exc_off"].astype(np.int64)
    alp, rd = vec["scheme"] == SCHEME_ALP, vec["scheme"] == SCHEME_ALP_RD
    bw, cnt = vec["bw"].astype(np.int64), vec["exc_cnt"].astype(np.int64)
    n = vec.size
    # a record boundary inside the column: a vector past the first with words of its own whose predecessor has some too (exception stream: a record of its
    # own and an earlier one; a column without exception records keeps the packed stream's vector and the seam lies on its empty record's offset)
    pv = _middle(np.nonzero((psz[1:] > 0) & (psz[:-1] > 0))[0] + 1, "two adjacent vectors with packed words")
    with_exc = np.nonzero(esz > 0)[0]
    ev = _middle(with_exc[1:], "two exception records") if with_exc.size >= 2 else pv
    out = {}
    for name in names:
        if name in ("seam_2_31", "seam_2_32"):
            seam = TWO31 if name == "seam_2_31" else TWO32
            p = (pv, 0, ev, 0)
        elif name == "inside":
            seam = TWO32
            m = _middle(np.nonzero(alp & (bw >= 8))[0], "ALP vector of 8 or more bits")
            me = _middle(np.nonzero(alp & (cnt >= 2) & ((W * cnt) % 8 == 0))[0], "ALP record of 2 or more exceptions whose positions start 8-aligned")
            p = (m, 128 * (int(bw[m]) // 2), me, W * int(cnt[me]))
        elif name == "rd_left":
            seam = TWO32
            m = _middle(np.nonzero(rd & (vec["lbw"] > 0))[0], "ALP_RD vector")
            # the positions of an ALP_RD record of c exceptions are its bytes [2c, 4c): the first multiple of 8 strictly inside
            k = (2 * cnt) // 8 * 8 + 8
            me = _middle(np.nonzero(rd & (cnt >= 1) & (k < 4 * cnt))[0], "ALP_RD record with a multiple of 8 strictly inside its positions")
            p = (m, 128 * int(bw[m]), me, int(k[me]))
        else:
            assert name == "all_above", name
            seam = TWO32
            p = (0, 0, 0, 0)
        p_vector, p_byte, e_vector, e_byte = p
        out[name] = Placement(name, seam - int(poff[p_vector]) - p_byte, seam - int(eoff[e_vector]) - e_byte, seam, seam, p_vector, p_byte, e_vector, e_byte)
        assert out[name].p_shift % 128 == 0 and out[name].e_shift % 8 == 0 and 0 <= p_vector < n and 0 <= e_vector < n
    return out


class Sparse:
    """a byte stream of `size` bytes that is zero outside its windows: [start, start + len) -> bytes.  Read by slices, as layout.expand reads a numpy stream"""

    def __init__(self, size):
        self.size, self.windows = size, {}

    def put(self, start, data):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert 0 <= start and start + data.size <= self.size
        for s, d in self.windows.items():
            assert start + data.size <= s or s + d.size <= start, "windows do not overlap"
        self.windows[start] = data

    def __getitem__(self, sl):
        a, b = sl.start, sl.stop
        assert sl.step is None and 0 <= a <= b <= self.size, (a, b)
        out = np.zeros(b - a, np.uint8)
        for s, d in self.windows.items():
            lo, hi = max(a, s), min(b, s + d.size)
            if lo < hi:
                out[lo - a:hi - a] = d[lo - s:hi - s]
        return out


def sparse_model(vec, packed, exc, pl):
    """the two streams of the placed column on the host: the small column's bytes at the shifts, zeros elsewhere"""
    p, e = Sparse(CAPACITY), Sparse(CAPACITY)
    p.put(pl.p_shift, packed)
    e.put(pl.e_shift, exc)
    return p, e


class Source:
    """a column as the encoder wrote it from x at offset 0, on the host: the input, the records, the placements"""

    def __init__(self, name, dtype, x, rg, vec, packed, exc, names):
        self.name, self.dtype, self.x = name, dtype, x
        self.W = 8 if dtype == "f64" else 4
        self.rg, self.vec, self.packed, self.exc = rg, vec, np.ascontiguousarray(packed), np.ascontiguousarray(exc)
        self.nv = vec.size
        self.values = x.reshape(self.nv, 1024)
        self.bits = x.view(np.uint64 if self.W == 8 else np.uint32)
        self.placements = placements(vec, self.W, names)
        self.rd_rowgroups = int((rg["scheme"] == SCHEME_ALP_RD).sum())


class HighColumn:
    """one capi.DeviceColumn per value type whose two streams hold 2^32 + 64 MiB each, zero but for the window(s) of the column last put"""

    def __init__(self, ctx, dtype, max_vectors):
        import torch
        from alp_amd import capi
        self.ctx, self.dtype, self.torch = ctx, dtype, torch
        self.col = capi.DeviceColumn(max_vectors, 0, packed_capacity=CAPACITY, exc_capacity=CAPACITY, dtype=dtype, rd_order=False)
        self.twin = capi.DeviceColumn(1, 0, packed_capacity=8, exc_capacity=8, dtype=dtype, rd_order=False)  # its own descriptors, the same streams
        self.windows = []  # (stream tensor, start, bytes) written by the last put
        self.current = None

    def _write(self, stream, start, data):
        t = self.torch
        stream[start:start + data.size] = t.from_numpy(data).to(stream.device)
        self.windows.append((stream, start, data.size))

    def _describe(self, col, src, vec, p_extent, e_extent, repeat=1):
        t = self.torch
        rg = src.rg
        if repeat > 1:  # the whole rowgroups of the column, `repeat` times over: every copy of a vector reads the same records
            whole = src.nv // 100 * 100
            rg, vec = np.tile(rg[:whole // 100], repeat), np.tile(vec[:whole], repeat)
        nv = vec.size
        col.n_vectors, col.n_rowgroups = nv, rg.size
        if col.vectors.numel() < 32 * nv:
            col.vectors = t.zeros(32 * nv, dtype=t.uint8, device=col.vectors.device)
            col.rowgroups = t.zeros(32 * rg.size, dtype=t.uint8, device=col.vectors.device)
        col.rowgroups[:32 * rg.size] = t.from_numpy(rg.view(np.uint8).reshape(-1)).to(col.vectors.device)
        col.vectors[:32 * nv] = t.from_numpy(vec.view(np.uint8).reshape(-1)).to(col.vectors.device)
        col.totals.zero_()
        col.totals[0], col.totals[1] = p_extent, e_extent
        c = col.c
        c.n_vectors, c.n_rowgroups = nv, rg.size
        c.d_rowgroups, c.d_vectors = col.rowgroups.data_ptr(), col.vectors.data_ptr()
        c.d_packed, c.packed_capacity, c.d_exc, c.exc_capacity = self.col.packed.data_ptr(), CAPACITY, self.col.exc.data_ptr(), CAPACITY
        # the hints are the column's own byte counts (per vector, what its records hold), not the extents: the launch plans stay those of a small column
        c.packed_bytes_hint, c.exc_bytes_hint, c.alp_rd_rowgroups_hint = src.packed.size * repeat, src.exc.size * repeat, 1 + src.rd_rowgroups * repeat
        self.ctx.forget(col)

    def put(self, src, name, twin=False, repeat=1):
        """the column `src` under its placement `name`; twin: also a second copy at twin_shift(name) in both streams, described by self.twin; repeat: the descriptors of
        the column's whole rowgroups that many times over (a longer column through the same records: the decoders follow descriptors as found)"""
        key = (src.name, name, twin, repeat)
        if self.current == key:
            return self.col
        self.ctx.synchronize()
        for stream, start, size in self.windows:
            stream[start:start + size].zero_()
        self.windows = []
        pl = src.placements[name]
        assert pl.p_shift + src.packed.size <= CAPACITY and pl.e_shift + src.exc.size <= CAPACITY
        self._write(self.col.packed, pl.p_shift, src.packed)
        self._write(self.col.exc, pl.e_shift, src.exc)
        self._describe(self.col, src, place(src.rg, src.vec, src.packed, src.exc, src.W, pl.p_shift, pl.e_shift), pl.p_shift + src.packed.size, pl.e_shift + src.exc.size, repeat)
        if twin:
            ts = twin_shift(name)
            assert max(pl.p_shift + src.packed.size, pl.e_shift + src.exc.size) <= ts and ts + max(src.packed.size, src.exc.size) <= CAPACITY
            self._write(self.col.packed, ts, src.packed)
            self._write(self.col.exc, ts, src.exc)
            self._describe(self.twin, src, place(src.rg, src.vec, src.packed, src.exc, src.W, ts, ts), ts + src.packed.size, ts + src.exc.size)
        self.ctx.synchronize()
        self.current = key
        return self.col
