"""GPU (-m gpu): CRTHIP_BIND_QUANTIZED - generic attributes as uint16 grid values + a crthip_quant_transform a blob.  Every route that can
put integers into the scratch values, against the oracle-derived expectation (tests/quantized_outputs.py) and against an ordinary FLOAT
decode of the same batch: every non-quantised array must be byte-identical to it.  Tolerance 0.  Output buffers are pre-filled with 0xA5
and every byte no array owns must still be 0xA5 afterwards."""
import ctypes as C

import numpy as np
import pytest
import torch

import corto_amd as ca
import quantized_outputs as qo
import value_ranges as vr

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

FILL = qo.FILL
Q = ca.BIND_QUANTIZED


def make_ctx(single=False):
    c = ca.Context(0)
    if single:
        c.set_single_stream(True)
    c.set_profiling(True)
    return c


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx1():
    c = make_ctx(True)
    yield c
    c.close()


class Piece:
    def __init__(self, blob, name, slot, off, stride, width, dtype, shape, quant):
        self.blob, self.name, self.slot, self.off, self.stride, self.width, self.dtype, self.shape, self.quant = blob, name, slot, off, stride, width, dtype, shape, quant


def bind(b, specs, computed=False, index16=False, normal_format=ca.FMT_FLOAT, records=False):
    """Bind every output of batch b in ONE poisoned device buffer.  specs[i]: (mode, names) - the generic attributes in `names` are bound
    quantised; mode "packed": every array on its own; "strided": quantised arrays on their own at stride 2N + 2 (position: 8); "record": the
    quantised position and uv inside one 16-byte vertex record (position at 0, uv at 8, the rest poison).  Returns (buffer, pieces, records)."""
    pieces, off = [], 0

    def take(n):
        nonlocal off
        off = (off + 255) & ~255
        r = off
        off += n
        return r
    for i, info in enumerate(b.infos):
        mode, names = specs[i]
        nv, nf = info.nvert, info.nface
        rec = take(nv * 16) if mode == "record" else None
        for k, a in enumerate(info.attrs()):
            N = a["components"]
            if a["codec"] == ca.CODEC_NORMAL:
                el = 4 if normal_format == ca.FMT_FLOAT else 2
                pieces.append(Piece(i, a["name"], k, take(nv * 3 * el), 3 * el, 3 * el, np.float32 if el == 4 else np.int16, (nv, 3), False))
            elif a["codec"] == ca.CODEC_COLOR:
                pieces.append(Piece(i, a["name"], k, take(nv * N), N, N, np.uint8, (nv, N), False))
            elif a["name"] in names:
                if mode == "record" and a["name"] in ("position", "uv"):
                    o, st = rec + (0 if a["name"] == "position" else 8), 16
                elif mode == "strided":
                    st = 2 * N + 2
                    o = take((nv - 1) * st + 2 * N if nv else 0)
                else:
                    o, st = take(nv * N * 2), 2 * N
                pieces.append(Piece(i, a["name"], k, o, st, 2 * N, np.uint16, (nv, N), True))
            else:
                pieces.append(Piece(i, a["name"], k, take(nv * N * 4), 4 * N, 4 * N, np.float32, (nv, N), False))
        if computed and nf and not any(a["codec"] == ca.CODEC_NORMAL for a in info.attrs()):
            el = 4 if normal_format == ca.FMT_FLOAT else 2
            pieces.append(Piece(i, "normal", -2, take(nv * 3 * el), 3 * el, 3 * el, np.float32 if el == 4 else np.int16, (nv, 3), False))
        if nf:
            el = 2 if index16 else 4
            pieces.append(Piece(i, "index", -1, take(nf * 3 * el), 3 * el, 3 * el, np.uint16 if index16 else np.uint32, (nf, 3), False))
    buf = torch.full((max(off, 256),), FILL, dtype=torch.uint8, device="cuda:0")
    first = np.cumsum([0] + [info.nattr for info in b.infos])
    recs = torch.full((max(int(first[-1]), 1) * 48,), FILL, dtype=torch.uint8, device="cuda:0") if records else None
    torch.cuda.synchronize()
    base = buf.data_ptr()
    binds = (ca.AttrBinding * max(int(first[-1]), 1))()
    index_ptrs = (C.c_void_p * max(len(b), 1))()
    index_fmt = np.full(max(len(b), 1), ca.FMT_UINT32, dtype=np.uint32)
    fmt_of = {np.float32: ca.FMT_FLOAT, np.int16: ca.FMT_INT16, np.uint8: ca.FMT_UINT8}
    for p in pieces:
        if p.slot >= 0:
            bd = binds[int(first[p.blob]) + p.slot]
            bd.buffer = base + p.off
            bd.format = ca.FMT_UINT16 if p.quant else fmt_of[p.dtype]
            bd.stride = p.stride if p.quant and p.stride != p.width else 0
            bd.reserved = Q if p.quant else 0
            bd.out_components = p.shape[1] if p.dtype == np.uint8 else 0
        elif p.slot == -1:
            index_ptrs[p.blob] = base + p.off
            index_fmt[p.blob] = ca.FMT_UINT16 if index16 else ca.FMT_UINT32
    ca._check(ca.lib().crthip_batch_bind_all(b.handle, binds, index_ptrs, ca._np_ptr(index_fmt)))
    for p in pieces:
        if p.slot == -2:
            b.bind_computed_normals(p.blob, base + p.off, normal_format)
    if records:
        b.bind_quant_transforms(recs.data_ptr())
    b._held = (buf, binds, index_ptrs, index_fmt, recs)
    return buf, pieces, recs


def rows_of(host, p):
    n = p.shape[0]
    if n == 0:
        return np.zeros((0, p.width), np.uint8)
    return np.lib.stride_tricks.as_strided(host[p.off:], shape=(n, p.width), strides=(p.stride, 1))


def reference(ctx, blobs, computed=False, index16=False, normal_format=ca.FMT_FLOAT):
    """the ordinary FLOAT decode of the same batch: per blob name -> array"""
    b = ca.Batch(ctx, blobs)
    b.allocate_outputs(fill=FILL, normal_format=normal_format, index16=index16, computed_normals=computed)
    b.decode()
    st = b.sync()
    assert (st == 0).all(), st
    outs = [b.host_outputs(i) for i in range(len(b))]
    b.close()
    return outs


def check(b, keys, pieces, buf, recs, ref, st, tag=""):
    """every piece against the expectation (quantised) or the FLOAT decode (everything else); statuses; records; poison everywhere else"""
    host = buf.cpu().numpy()
    owned = np.zeros(len(host), bool)
    want_st = np.zeros(len(keys), np.int32)
    first = np.cumsum([0] + [info.nattr for info in b.infos])
    rec_host = recs.cpu().numpy().reshape(-1, 48) if recs is not None else None
    rec_owned = np.zeros(int(first[-1]), bool)
    for p in pieces:
        rows = rows_of(host, p)
        mark = rows_of(owned, p)
        if p.quant:
            e = qo.expected(keys[p.blob], p.name)
            t = b.quant_transform(p.blob, p.name)
            e.check_record(t, (tag, keys[p.blob], p.name))
            if rec_host is not None:
                r = int(first[p.blob]) + p.slot
                assert rec_host[r].tobytes() == bytes(t) == e.record_bytes(), (tag, keys[p.blob], p.name)
                rec_owned[r] = True
            if e.written:
                assert rows.tobytes() == e.out.tobytes(), (tag, keys[p.blob], p.name)
                mark[:] = True
            else:
                want_st[p.blob] = qo.E_FORMAT                # ... and its buffer stays poison (below)
        else:
            assert rows.tobytes() == np.ascontiguousarray(ref[p.blob][p.name]).tobytes(), (tag, keys[p.blob], p.name)
            mark[:] = True
    assert (host[~owned] == FILL).all(), (tag, "a byte outside the arrays was written")
    assert (st == want_st).all(), (tag, st, want_st)
    if rec_host is not None:
        assert (rec_host[:int(first[-1])][~rec_owned] == FILL).all(), (tag, "a record of a non-quantised attribute was touched")
    for i in range(len(keys)):                                # a record nobody bound quantised is refused
        for k, a in enumerate(b.infos[i].attrs()):
            if not any(p.blob == i and p.slot == k and p.quant for p in pieces):
                with pytest.raises(ca.CortoError) as ei:
                    b.quant_transform(i, k)
                assert ei.value.code == qo.E_ARGUMENT


def run(ctx, keys, specs, tag="", ref_ctx=None, **kw):
    """decode the named blobs with `specs` and hold everything against the expectation; returns the kernels that ran and the stats"""
    blobs = [qo.traced(k)[0] for k in keys]
    ref = reference(ref_ctx or ctx, blobs, **kw)
    b = ca.Batch(ctx, blobs)
    buf, pieces, recs = bind(b, specs, records=True, **kw)
    b.decode()
    st = b.sync(raise_on_error=False)
    ran, stats = set(b.kernel_times()), b.stats()
    check(b, keys, pieces, buf, recs, ref, st, tag)
    assert stats.output_bytes == sum(p.shape[0] * p.width for p in pieces), tag
    b.close()
    return ran, stats


def all_generic(keys, mode="packed"):
    return [(mode, set(qo.generic_names(qo.traced(k)[0]))) for k in keys]


# ---- every route that can put integers into the scratch values ----------------------------------------------------------------------

def test_lds16_records(ctx, ctx1):
    keys = ["c4_unit", "icosphere2", "holey_disc20"]
    for c, mode in ((ctx, "packed"), (ctx1, "strided")):
        ran, stats = run(c, keys, all_generic(keys, mode), tag=mode)
        assert "delta_lds16" in ran and "quant_out_blob" in ran and not ({"quant_range", "quant_store", "dequantize"} & ran), sorted(ran)
        assert stats.delta_wide == 0 and stats.delta_redone == 0


def widen_case():
    case = [c for c in vr.handon_cases() if c.id == "widen_N3_window"][0]
    return ca.aligned_blob(case.blob())


def test_lds16_wide_records():
    """values that leave int16 relative to vertex 0: redone in HBM on the first decode, in 32-bit LDS records from then on"""
    qo.BLOBS.setdefault("widen_N3_window", widen_case)
    c, other = make_ctx(), make_ctx()                        # (the FLOAT reference on a context of its own: it would teach `c` the wide layout)
    try:
        for wide in (0, 1):
            ran, stats = run(c, ["widen_N3_window"], [("packed", {"g", "position"})], tag=wide, ref_ctx=other)
            assert stats.delta_wide == wide and stats.delta_redone == 1 - wide and "delta_lds16" in ran and "quant_out_blob" in ran, (wide, sorted(ran))
    finally:
        c.close()
        other.close()


@pytest.mark.parametrize("i32", ["0", "1"])
def test_int16_hand_on(monkeypatch, i32):
    """K-BIT's halfwords at the front of the scratch values, on and off"""
    monkeypatch.setenv("CORTO_VALUES_I32", i32)
    c = make_ctx(True)
    try:
        keys = ["c4_unit", "icosphere2"]
        ran, stats = run(c, keys, all_generic(keys), tag=i32)
        assert (stats.int16_streams > 0) == (i32 == "0") and "quant_out_blob" in ran
    finally:
        c.close()


def test_delta_tiles(ctx, ctx1):
    """a mesh beyond K-DELTA's LDS records, and beyond QOUT_BLOB_MAX: the two-kernel path"""
    assert qo.traced("torus_182")[1]["nvert"] > max(32767, qo.blob_max())
    for c, mode in ((ctx, "packed"), (ctx1, "strided")):
        ran, _ = run(c, ["torus_182"], all_generic(["torus_182"], mode), tag=mode, index16=False)
        assert "delta_tiles" in ran and {"quant_range", "quant_store"} <= ran and "quant_out_blob" not in ran, sorted(ran)


def test_point_cloud_and_single_vertex(ctx):
    keys = ["cloud_40_20", "single_vertex"]
    ran, _ = run(ctx, keys, all_generic(keys))
    assert "cloud_apply" in ran and "quant_out_blob" in ran, sorted(ran)
    e = qo.expected("single_vertex", "g3")
    assert e.nvert == 1 and (e.span == 0).all() and (e.out == 0).all() and (e.base == e.d[0]).all()


# ---- quantised positions feeding normals --------------------------------------------------------------------------------------------

def test_stored_border_normals_fused(ctx, ctx1):
    keys = ["c4_unit", "holey_disc20"]
    for c in (ctx, ctx1):
        for fmt in (ca.FMT_FLOAT, ca.FMT_INT16):
            ran, _ = run(c, keys, [("packed", {"position"})] * 2, normal_format=fmt, index16=True)
            assert "normal_blob" in ran and "normal_faces" not in ran, sorted(ran)


def test_stored_border_normals_beyond_fused(ctx):
    ran, _ = run(ctx, ["torus_105"], [("packed", {"position", "uv"})])
    assert "normal_faces" in ran and "normal_vertex" in ran and "normal_blob" not in ran, sorted(ran)


def test_computed_normals(ctx, ctx1):
    for c in (ctx, ctx1):
        ran, _ = run(c, ["bare_sphere"], [("strided", {"position"})], computed=True, normal_format=ca.FMT_INT16)
        assert "normal_blob_computed" in ran, sorted(ran)


# ---- one batch that mixes ------------------------------------------------------------------------------------------------------------

def test_mixed_batch(ctx, ctx1):
    keys = ["c4_unit", "icosphere2", "holey_disc20", "c4_unit", "cloud_40_20", "icosphere2"]
    specs = [("packed", {"position", "uv"}), ("packed", set()), ("packed", {"position"}), ("record", {"position", "uv"}), ("packed", set()),
             ("strided", {"position", "uv"})]
    for c in (ctx, ctx1):
        ran, _ = run(c, keys, specs, normal_format=ca.FMT_INT16, index16=True)
        assert "quant_out_blob" in ran


# ---- the size class --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step", [-1, 0, 1])
def test_blob_max_on_clouds(ctx, step):
    nv = qo.blob_max() + step
    key = "cloud_exact_%d" % nv
    qo.BLOBS.setdefault(key, lambda: qo.cloud_blob(nv, seed=step + 2))
    assert qo.traced(key)[1]["nvert"] == nv
    ran, _ = run(ctx, [key], [("packed", {"position", "g1", "g2", "g3", "g4"})])
    if step <= 0:
        assert "quant_out_blob" in ran and not ({"quant_range", "quant_store"} & ran), sorted(ran)
    else:
        assert {"quant_range", "quant_store"} <= ran and "quant_out_blob" not in ran, sorted(ran)


# ---- the span edge ---------------------------------------------------------------------------------------------------------------------

def test_span_65535_decodes_and_65536_does_not(ctx, ctx1):
    for key in qo.EDGES:
        qo.assert_edge(key)
    keys = ["edge_65535", "edge_65536", "edge_neg", "c4_unit"]
    for c, mode in ((ctx, "packed"), (ctx1, "strided")):
        blobs = [qo.traced(k)[0] for k in keys]
        ref = reference(c, blobs)
        b = ca.Batch(c, blobs)
        buf, pieces, recs = bind(b, all_generic(keys, mode), records=True)
        b.decode()
        st = b.sync(raise_on_error=False)
        assert list(st) == [0, qo.E_FORMAT, 0, 0], st
        check(b, keys, pieces, buf, recs, ref, st, mode)      # (the refused blob: buffers still poison, index correct, the true span, written == 0)
        for name in ("position", "grid"):
            t = b.quant_transform(1, name)
            assert t.written == 0 and list(t.span[:t.components]) == [65536] * t.components
        b.close()


def test_32_bit_fields(ctx):
    blob, tr = qo.traced("fields32")
    names = {nm for nm in qo.generic_names(blob) if qo.Expected(blob, tr, nm).N <= 4}
    assert any(qo.Expected(blob, tr, nm).written == 0 for nm in names)
    run(ctx, ["fields32", "icosphere2"], [("packed", names), ("packed", {"position"})])


# ---- planning paths --------------------------------------------------------------------------------------------------------------------

def test_decode_with_next_equals_plain(ctx1):
    keys = [["c4_unit"] * 64, ["icosphere2", "torus_182", "cloud_40_20"]]
    specs = [[("packed", {"position", "uv"})] * 64, [("record", {"position", "uv"}), ("packed", {"position", "uv"}), ("packed", {"position"})]]
    objs = [ca.Batch(ctx1, []), ca.Batch(ctx1, [])]
    objs[1].set_parity(1)
    try:
        held = []
        for k in range(2):
            blobs = [qo.traced(x)[0] for x in keys[k]]
            ref = reference(ctx1, blobs, index16=True)
            objs[k].reset(blobs)
            held.append((bind(objs[k], specs[k], records=True, index16=True), ref))
        objs[0].decode_entropy()
        objs[0].decode_with_next(objs[1])
        st0 = objs[0].sync(raise_on_error=False)
        objs[1].decode_with_next(None)
        st1 = objs[1].sync(raise_on_error=False)
        for k, st in ((0, st0), (1, st1)):
            (buf, pieces, recs), ref = held[k]
            check(objs[k], keys[k], pieces, buf, recs, ref, st, ("pair", k))
    finally:
        for o in objs:
            o.close()


def test_resident_batch_equals_host(ctx):
    keys = ["c4_unit", "holey_disc20", "cloud_40_20"]
    blobs = [qo.traced(k)[0] for k in keys]
    ref = reference(ctx, blobs)
    offs, pos = [], 0
    for bl in blobs:
        offs.append(pos)
        pos += (len(bl) + 15) // 16 * 16 + 32
    host = np.zeros(pos + 64, np.uint8)
    for bl, o in zip(blobs, offs):
        host[o:o + len(bl)] = bl
    arena = torch.from_numpy(host).to("cuda:0")
    b = ca.Batch.resident(ctx, arena, offs, [len(bl) for bl in blobs])
    buf, pieces, recs = bind(b, all_generic(keys), records=True)
    b.decode()
    st = b.sync(raise_on_error=False)
    check(b, keys, pieces, buf, recs, ref, st, "resident")
    # a reset drops the device record array: the next decode leaves it alone
    b.reset_resident(arena, offs[:1], [len(blobs[0])])
    recs.fill_(FILL)
    buf, pieces, _ = bind(b, all_generic(keys[:1]))
    b.decode()
    st = b.sync(raise_on_error=False)
    check(b, keys[:1], pieces, buf, None, ref[:1], st, "resident reset")
    assert (recs.cpu().numpy() == FILL).all()
    b.close()


def test_python_mirror(ctx):
    """Batch.allocate_outputs(quantized=...) / host_outputs / quant_transform"""
    blob = qo.traced("icosphere2")[0]
    b = ca.Batch(ctx, [blob])
    b.allocate_outputs(fill=FILL, quantized=("position", "uv"))
    b.decode()
    assert (b.sync() == 0).all()
    out = b.host_outputs(0)
    ref = reference(ctx, [blob])[0]
    for nm in ("position", "uv"):
        e = qo.expected("icosphere2", nm)
        assert out[nm].dtype == np.uint16 and out[nm].tobytes() == e.out.tobytes()
        e.check_record(b.quant_transform(0, nm))
        t = b.quant_transform(0, nm)
        back = (np.array(t.base[:e.N], np.int32) + out[nm].astype(np.int32)).astype(np.float32) * np.float32(t.q)
        assert back.tobytes() == ref[nm].tobytes()
    assert out["normal"].tobytes() == ref["normal"].tobytes() and out["index"].tobytes() == ref["index"].tobytes()
    b.close()


# ---- bind errors -----------------------------------------------------------------------------------------------------------------------

def test_bind_errors(ctx):
    blob5 = ca.aligned_blob(ca.encode(qo.exact_cloud(8)[0], with_normal=False, with_color=False, with_uv=False,
                                      attributes=[("five", np.zeros((8, 5), np.int32), 1.0, 0)]))
    b = ca.Batch(ctx, [qo.traced("c4_unit")[0], blob5])
    buf = torch.full((1 << 16,), FILL, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    names = [a["name"] for a in b.infos[0].attrs()]

    def code(blob, attr, **kw):
        binds = (ca.AttrBinding * b.infos[blob].nattr)()
        bd = binds[attr]
        bd.buffer, bd.format, bd.reserved = base, ca.FMT_UINT16, Q
        for k, v in kw.items():
            setattr(bd, k, v)
        return ca.lib().crthip_batch_bind(b.handle, blob, binds, None, ca.FMT_UINT32)
    pos, nrm, col = names.index("position"), names.index("normal"), names.index("color")
    assert code(0, pos) == 0 and code(0, pos, stride=6) == 0 and code(0, pos, stride=8) == 0 and code(0, pos, out_components=3) == 0
    for fmt in (ca.FMT_FLOAT, ca.FMT_DOUBLE, ca.FMT_INT16, ca.FMT_UINT32, ca.FMT_UINT8, ca.FMT_INT8, 8, 99):
        assert code(0, pos, format=fmt) == qo.E_FORMAT, fmt
    # the one format that is not E_FORMAT: INT32, the stream values' format, keeps the argument error this flag bit had before it meant anything
    # (tests/test_gpu_parity.py pins that call); include/corto_hip.h says so
    assert code(0, pos, format=ca.FMT_INT32) == qo.E_ARGUMENT
    assert code(0, nrm) == qo.E_FORMAT and code(0, nrm, format=ca.FMT_INT16) == qo.E_FORMAT
    assert code(0, col) == qo.E_FORMAT and code(0, col, format=ca.FMT_UINT8) == qo.E_FORMAT
    assert code(0, pos, reserved=Q | ca.BIND_STREAM_VALUES) == qo.E_ARGUMENT
    assert code(0, pos, reserved=Q | 4) == qo.E_ARGUMENT
    five = [a["name"] for a in b.infos[1].attrs()].index("five")
    assert code(1, five) == qo.E_LIMIT
    assert code(0, pos, out_components=2) == qo.E_ARGUMENT and code(0, pos, out_components=4) == qo.E_ARGUMENT
    assert code(0, pos, buffer=base + 1) == qo.E_ARGUMENT
    for stride in (2, 4, 5, 7, 9):
        assert code(0, pos, stride=stride) == qo.E_ARGUMENT, stride
    with pytest.raises(ca.CortoError) as ei:
        b.bind_quant_transforms(base + 8)
    assert ei.value.code == qo.E_ARGUMENT
    b.bind_quant_transforms(None)
    with pytest.raises(ca.CortoError) as ei:                 # nothing decoded yet
        b.quant_transform(0, pos)
    assert ei.value.code == qo.E_ARGUMENT
    b.close()
