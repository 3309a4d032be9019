"""GPU: the library's verdict on every case of tests/blob_cases.py, through each route bytes from outside can take, against the rules in Python integers
(tests/blob_replica.py; tests/test_blob_check_cpu.py holds the same cases on the CPU, under the host sanitizers, and the chunk windows):
  * alpgpu_column_from_blob / _f32 called directly (capi.lib) on a column sized for the base blob, and Context.from_blob: verdict and error text are the
    replica's; a refusal leaves the column's four device buffers as they were (it comes before any copy);
  * alpgpu_decompress_host_f64 / _f32 on the same bytes: these columns are one chunk, whose window begins at vector 0's offsets, so the expectation is the
    replica's with one chunk over the whole column;
  * alpgpu_column_validate on the edited arrays uploaded as a device column whose capacities are the stream lengths: verdict and *first_bad exactly.
Accepted cases that leave the values alone (moved or appended records, the bounds of n_values and size, fields unused for the vector's scheme) decode bit
for bit to the oracle's decode of the base column.  No kernel is handed a column or blob the replica refuses: where the library accepts one, the test has
failed before anything is decoded."""
import ctypes as C

import numpy as np
import pytest
import torch

import blob_cases as bc
import blob_replica as br

pytestmark = pytest.mark.gpu
CANARY = 0xA5
WRAPPER_TEXTS = ("blob shorter than its 64-byte header", "blob header is implausible")  # Context.from_blob's own refusals, both of the header


class Column:
    """a base column, the oracle's decode of it, and a device column sized for it whose buffers hold a canary"""

    def __init__(self, base, want):
        from alp_amd import capi
        self.base, self.want = base, want
        self.bits = want.view(np.uint64 if base.vb == 8 else np.uint32)
        self.col = capi.DeviceColumn(base.n, dtype=base.dtype)
        self.buffers = (self.col.rowgroups, self.col.vectors, self.col.packed, self.col.exc)
        self.paint()

    def paint(self):
        for t in self.buffers:
            t.fill_(CANARY)

    def untouched(self):
        return all(bool((t == CANARY).all()) for t in self.buffers)


@pytest.fixture(scope="module")
def columns(ctx, oracle):
    from oracle.pyoracle import OracleF32
    of = OracleF32()
    f64, f32 = bc.base_f64(oracle), bc.base_f32(of)
    return {"f64": Column(f64, oracle.decode_column(f64.enc)), "f32": Column(f32, of.decode_column(f32.enc))}


@pytest.fixture(scope="module")
def rows(ctx, oracle):
    from oracle.pyoracle import OracleF32
    r64, r32 = bc.rows_f64(), bc.rows_f32()
    return {"f64": Column(r64, oracle.decode_column(r64.enc)), "f32": Column(r32, OracleF32().decode_column(r32.enc))}


def ptr(a):
    return C.c_void_p(a.ctypes.data)


def last_error():
    from alp_amd import capi
    return capi.lib.alpgpu_last_error().decode()


def decoded_bits(ctx, col, n_values):
    out = ctx.decode(col)
    ctx.synchronize()
    return out[:n_values].cpu().numpy().view(np.uint64 if col.dtype == "f64" else np.uint32)


def c_from_blob(ctx, blob, size, vb, col):
    from alp_amd import capi
    nv = C.c_uint64(0)
    fn = capi.lib.alpgpu_column_from_blob if vb == 8 else capi.lib.alpgpu_column_from_blob_f32
    rc = fn(ctx.h, ptr(blob), size, C.byref(col.c), C.byref(nv))
    return rc, last_error() if rc else "", int(nv.value)


def c_decompress_host(ctx, blob, size, vb, out):
    from alp_amd import capi
    nv = C.c_uint64(0)
    fn = capi.lib.alpgpu_decompress_host_f64 if vb == 8 else capi.lib.alpgpu_decompress_host_f32
    rc = fn(ctx.h, ptr(blob), C.c_uint64(size), C.c_void_p(out.data_ptr()), C.c_uint64(out.numel()), C.byref(nv))
    return rc, last_error() if rc else "", int(nv.value)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_build_blob_is_the_library_s_blob(ctx, columns, rows, dtype):
    """tests/blob_replica.py: build_blob writes byte for byte what alpgpu_column_to_blob writes for the same arrays in HBM"""
    from alp_amd import capi
    for b in (columns[dtype].base, rows[dtype].base):
        col = capi.DeviceColumn.from_host(b.rg, b.vec, b.packed, b.exc, dtype=dtype)
        assert np.array_equal(ctx.to_blob(col, b.n_values), b.blob), b.name


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_case_through_from_blob_and_decompress_host(ctx, columns, dtype):
    from alp_amd import capi
    K = columns[dtype]
    base, col = K.base, K.col
    out = torch.empty(base.n * 1024, dtype=torch.float64)  # room for n * 1024 values of either type: one case reads a float blob as doubles
    out = out if dtype == "f64" else out.view(torch.float32)[:base.n * 1024]
    wrong = []
    for c in bc.cases(base):
        blob, size, _ = c.build()
        want = br.check_blob(blob, size, c.vb)
        n_values = br.HEADER.unpack_from(blob, 0)[3] if size >= 64 else 0
        # ---- the C entry point, on a column sized for the base blob
        rc, text, nv = c_from_blob(ctx, blob, size, c.vb, col)
        passed = rc == 0 or (rc == -2 and "column was allocated for a different vector count" in text)  # (the empty column: validated, then not this column's size)
        if passed != want.ok or (not want.ok and (rc != -2 or br.TEXT[want.detail] not in text)):
            wrong.append((c.name, "from_blob", rc, text, repr(want)))
        if rc != 0 and not K.untouched():
            wrong.append((c.name, "from_blob wrote to the column before it refused", rc, text, repr(want)))
        if rc == 0:
            if want.ok and c.same and (nv != n_values or not np.array_equal(decoded_bits(ctx, col, nv), K.bits[:nv])):
                wrong.append((c.name, "from_blob decode", rc, nv, repr(want)))
            K.paint()
        assert want.ok or rc != 0, (c.name, "a refused blob was accepted: nothing of it is decoded")
        # ---- the Python wrapper, where it would call the entry point of the same value type
        if c.vb == (4 if size >= 64 and br.HEADER.unpack_from(blob, 0)[8] == 4 else 8):
            try:
                col2, nv2 = ctx.from_blob(blob[:size])
                assert want.ok, (c.name, "Context.from_blob accepted a refused blob: nothing of it is decoded")
                if c.same and (nv2 != n_values or not np.array_equal(decoded_bits(ctx, col2, nv2), K.bits[:nv2])):
                    wrong.append((c.name, "Context.from_blob decode", 0, nv2, repr(want)))
            except capi.AlpGpuError as e:
                mine = want.rules == {"header"} and any(t in str(e) for t in WRAPPER_TEXTS)
                if want.ok or not (mine or br.TEXT[want.detail] in str(e)):
                    wrong.append((c.name, "Context.from_blob", -2, str(e), repr(want)))
        # ---- the chunked host route: one chunk, whose window is [vector 0's offsets, the streams' ends)
        n = br.HEADER.unpack_from(blob, 0)[4] if size >= 64 else 0
        want_h = br.check_blob(blob, size, c.vb, chunk=max(n, 1))
        rc, text, nv = c_decompress_host(ctx, blob, size, c.vb, out)
        if (rc == 0) != want_h.ok or (not want_h.ok and (rc != -2 or br.TEXT[want_h.detail] not in text)):
            wrong.append((c.name, "decompress_host", rc, text, repr(want_h)))
        elif rc == 0 and c.same and (nv != n_values or not np.array_equal(out[:nv].numpy().view(K.bits.dtype), K.bits[:nv])):
            wrong.append((c.name, "decompress_host decode", rc, nv, repr(want_h)))
        assert want_h.ok or rc != 0, (c.name, "a refused blob was decoded by the host route")
    assert not wrong, (len(wrong), wrong[:8])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_descriptor_and_position_case_through_column_validate(ctx, columns, dtype):
    """the device validator takes the same per-descriptor function (blob_check.hpp): its verdict and its first bad vector are the replica's"""
    from alp_amd import capi
    K = columns[dtype]
    wrong, seen = [], 0
    for c in bc.cases(K.base):
        if not c.has_column:
            continue
        _, _, p = c.build()
        want = br.check_column(p.rg, p.vec, p.exc, p.packed.size, p.exc.size, c.vb)
        assert want.ok == (c.rule is None) and (want.ok or (want.rules == {c.rule} and want.first_bad == c.bad)), (c.name, repr(want))
        col = capi.DeviceColumn.from_host(p.rg, p.vec, p.packed, p.exc, dtype=dtype)
        col.c.packed_capacity, col.c.exc_capacity = p.packed.size, p.exc.size  # the streams' lengths; the buffers stay as allocated
        got = ctx.column_validate(col)
        seen += 1
        if got != want.first_bad:
            wrong.append((c.name, got, repr(want)))
        elif want.ok and c.same:
            nv = K.base.n_values
            if not np.array_equal(decoded_bits(ctx, col, nv), K.bits[:nv]):
                wrong.append((c.name, "decode", repr(want)))
    assert not wrong, (len(wrong), wrong[:8])
    assert seen > 200


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_hand_built_rows_are_accepted_by_every_route_and_decode(ctx, rows, dtype):
    """every width, every cut and 1 to 1024 exceptions: the accepted extreme"""
    from alp_amd import capi
    K = rows[dtype]
    b = K.base
    assert b.n < 10000 and br.check_blob(b.blob, b.blob.size, b.vb).ok and br.check_blob(b.blob, b.blob.size, b.vb, chunk=b.n).ok
    nv = b.n_values
    rc, text, got_nv = c_from_blob(ctx, b.blob, b.blob.size, b.vb, K.col)
    assert (rc, got_nv) == (0, nv), text
    assert np.array_equal(decoded_bits(ctx, K.col, nv), K.bits)
    col2, nv2 = ctx.from_blob(b.blob)
    assert nv2 == nv and np.array_equal(decoded_bits(ctx, col2, nv), K.bits)
    out = torch.empty(nv, dtype=torch.float64 if dtype == "f64" else torch.float32)
    rc, text, got_nv = c_decompress_host(ctx, b.blob, b.blob.size, b.vb, out)
    assert (rc, got_nv) == (0, nv), text
    assert np.array_equal(out.numpy().view(K.bits.dtype), K.bits)
    col3 = capi.DeviceColumn.from_host(b.rg, b.vec, b.packed, b.exc, dtype=dtype)
    col3.c.packed_capacity, col3.c.exc_capacity = b.packed.size, b.exc.size
    assert ctx.column_validate(col3) is None
