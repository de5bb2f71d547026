"""GPU (-m gpu): crthip_batch_bind_computed_normals - normals for blobs that store none, raw bytes against the oracle's decode of a BORDER
twin where upstream defines the value and against the model (tests/computed_normals.py) elsewhere.  Outputs are pre-filled with 0xA5: every
element of a computed normal array must have been written."""
import ctypes as C
import functools

import numpy as np
import pytest

import corto_amd as ca
import computed_normals as cn
import size_classes as sc
from corto_amd import synth
from oracle import oracle as oc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = cn.FILL
KEYS = ["position", "normal", "index"]
E_FORMAT, E_ARGUMENT, E_NEEDS_POSITION = -7, -8, -6
FORMATS = [(ca.FMT_FLOAT, False), (ca.FMT_INT16, True), (ca.FMT_FLOAT, True), (ca.FMT_INT16, False)]      # (normal format, u16 index)


def make_ctx(single):
    c = ca.Context(0)
    if single:
        c.set_single_stream(True)
    c.set_profiling(True)
    return c


@pytest.fixture(scope="module")
def ctxs():
    cs = {False: make_ctx(False), True: make_ctx(True)}
    yield cs
    for c in cs.values():
        c.close()


def decode(ctx, blobs, fmt=ca.FMT_FLOAT, index16=False):
    b = ca.Batch(ctx, blobs)
    b.allocate_outputs(fill=FILL, normal_format=fmt, index16=index16, computed_normals=True)
    b.decode()
    st = b.sync()
    assert (st == 0).all(), st
    return b, set(b.kernel_times())


def check_named(ctx, names, bits=14, tag=""):
    """the named meshes' normal-less blobs in one batch, every format: all outputs against Expected"""
    exps = [cn.expected(n, bits) for n in names]
    for fmt, i16 in FORMATS:
        b, ran = decode(ctx, [e.bare for e in exps], fmt, i16)
        assert "normal_blob_computed" in ran and "normal_blob" not in ran, sorted(ran)
        for i, e in enumerate(exps):
            cn.assert_same(b.host_outputs(i), e.outputs(fmt, i16), KEYS, (tag, names[i], fmt, i16))
        b.close()
    return exps


def test_closed_meshes(ctxs):
    """no boundary vertex, no degenerate one: every vertex is the oracle's decode of the BORDER twin"""
    for e in check_named(ctxs[False], cn.CLOSED, tag="closed"):
        assert e.defined.all()
        assert e.normal(ca.FMT_FLOAT).tobytes() == oc.decode(e.twin)["normal"].tobytes()


def test_open_meshes(ctxs):
    """boundary vertices (where the twin holds corrected normals) equal the model, the interior the oracle too"""
    for e in check_named(ctxs[False], cn.OPEN, tag="open"):
        assert e.bnd.any() and e.defined.any()
        for fmt in (ca.FMT_FLOAT, ca.FMT_INT16):
            assert e.normal(fmt).tobytes() == e.model(fmt)[0].tobytes()      # all vertices equal the model; e.normal took the interior from the oracle


@pytest.mark.parametrize("case", cn.DEGENERATE, ids=[c[0] for c in cn.DEGENERATE])
def test_degenerate_vertices(ctxs, case):
    """3-bit positions: most estimates cancel to zero - (0,0,1) / (0,0,32767) there, the oracle everywhere else"""
    name, bits, nzero, nvert = case
    e, = check_named(ctxs[False], [name], bits, tag="degenerate")
    assert e.degenerate.sum() == nzero and e.nvert == nvert
    assert (e.normal(ca.FMT_FLOAT)[e.degenerate] == (0, 0, 1)).all() and (e.normal(ca.FMT_INT16)[e.degenerate] == (0, 0, 32767)).all()


# ---- size classes, one step either side (tests/size_classes.py's builders) ----

def nface_mesh(nface):
    m = sc.closed_mesh(sc.NFACE_BASE)
    m = synth.non_manifold(m, seed=0, fins=0, dups=nface - m.nface, reversed_dups=0, bowties=0, glue=0)
    assert m.nface == nface
    return m


SIZE_CASES = [      # (id, mesh, the fused kernel takes it)
    ("nface_21845", lambda: nface_mesh(sc.NFACE_MAX), True),
    ("nface_21846", lambda: nface_mesh(sc.NFACE_MAX + 1), False),
    ("torus_105_105", cn.MESHES["torus_105_105"], False),
    ("nvert_32767", lambda: sc.closed_mesh(32767), False),             # K-DELTA's LDS records ...
    ("nvert_32768", lambda: sc.closed_mesh(32768), False),             # ... against k_delta_tiles
    ("torus_182_182", cn.MESHES["torus_182_182"], False),
    ("fn_last", lambda: sc.closed_mesh(sc.FN_LAST), True),             # face normals in LDS (two-stream context) ...
    ("fn_last_plus_1", lambda: sc.closed_mesh(sc.FN_LAST + 1), True),  # ... and in scratch on either context
    ("fused_last", lambda: sc.closed_mesh(sc.FUSED_LAST), True),       # the LDS limit of the fused kernel
    ("fused_last_plus_1", lambda: sc.closed_mesh(sc.FUSED_LAST + 1), False),
    ("delta_last", lambda: sc.closed_mesh(sc.DELTA_LIMITS[2][4]), False),          # the positions' int16 LDS records (N = 3) ...
    ("delta_last_plus_1", lambda: sc.closed_mesh(sc.DELTA_LIMITS[2][4] + 1), False),   # ... and the first mesh beyond them
]


@functools.lru_cache(maxsize=None)
def size_expected(cid):
    mesh = [c for c in SIZE_CASES if c[0] == cid][0][1]()
    return cn.Expected(*cn.twins_of(mesh))


@pytest.mark.parametrize("single", [False, True], ids=["two_stream", "single_stream"])
@pytest.mark.parametrize("case", SIZE_CASES, ids=[c[0] for c in SIZE_CASES])
def test_size_classes(ctxs, case, single):
    cid, _, fused = case
    e = size_expected(cid)
    fmt, i16 = (ca.FMT_INT16, False) if single else (ca.FMT_FLOAT, e.nvert < 65536)
    b, ran = decode(ctxs[single], [e.bare], fmt, i16)
    cn.assert_same(b.host_outputs(0), e.outputs(fmt, i16), KEYS, (cid, single))
    if fused:
        assert "normal_blob_computed" in ran and "normal_faces" not in ran, (cid, sorted(ran))
    else:
        assert "normal_faces" in ran and "normal_vertex" in ran and "normal_blob_computed" not in ran, (cid, sorted(ran))
    assert "normal_blob" not in ran, (cid, sorted(ran))
    b.close()


# ---- layouts ----

def device_bytes(n):
    import torch
    t = torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


def binding(ptr, fmt, stride=0, flags=0):
    bd = ca.AttrBinding()
    bd.buffer = ptr; bd.format = fmt; bd.out_components = 0; bd.stride = stride; bd.reserved = flags
    return bd


def run(b):
    b.decode()
    st = b.sync()
    assert (st == 0).all(), st


def test_interleaved_record_and_double_positions(ctxs):
    """INT16 normals at stride 20 beside float positions in one vertex record (the integer positions then live in scratch): the two
    padding bytes of every record survive; and positions bound as DOUBLE with packed float normals"""
    e = cn.expected("holey_disc_20")
    nv, nf = e.nvert, e.nface
    for single in (False, True):
        b = ca.Batch(ctxs[single], [e.bare])
        assert [a["name"] for a in b.infos[0].attrs()] == ["position"]
        vb, ib = device_bytes(nv * 20), device_bytes(nf * 6)
        b.bind(0, [binding(vb.data_ptr(), ca.FMT_FLOAT, 20)], ib.data_ptr(), ca.FMT_UINT16)
        b.bind_computed_normals(0, vb.data_ptr() + 12, ca.FMT_INT16, 20)
        run(b)
        rec = vb.cpu().numpy().reshape(nv, 20)
        got = {"position": np.ascontiguousarray(rec[:, :12]).view(np.float32), "normal": np.ascontiguousarray(rec[:, 12:18]).view(np.int16),
               "index": ib.cpu().numpy().view(np.uint16).reshape(nf, 3)}
        cn.assert_same(got, e.outputs(ca.FMT_INT16, True), KEYS, ("interleaved", single))
        assert (rec[:, 18:] == FILL).all()
        # DOUBLE positions (upstream's in-place widening: the oracle's bytes), float normals
        pb, nb, ib = device_bytes(nv * 24), device_bytes(nv * 12), device_bytes(nf * 12)
        b.bind(0, [binding(pb.data_ptr(), ca.FMT_DOUBLE)], ib.data_ptr(), ca.FMT_UINT32)
        b.bind_computed_normals(0, nb.data_ptr())
        run(b)
        assert pb.cpu().numpy().tobytes() == oc.decode_attr_format(e.bare, "position", ca.FMT_DOUBLE)[:nv * 24].tobytes()
        got = {"normal": nb.cpu().numpy().view(np.float32).reshape(nv, 3), "index": ib.cpu().numpy().view(np.uint32).reshape(nf, 3)}
        cn.assert_same(got, e.outputs(ca.FMT_FLOAT, False), ["normal", "index"], ("double", single))
        b.close()


# ---- a mixed batch ----

def test_mixed_batch(ctxs):
    """stored DIFF / ESTIMATED / BORDER normals bound as ever, normal-less meshes with and without computed normals, a stored ESTIMATED
    normal left unbound and computed instead, two groups, a non-manifold mesh, a point cloud: every output of every blob"""
    base = synth.torus(24, 12)
    stored = [ca.encode(synth.bumpy_sphere(16, 8), normal_prediction=p) for p in (ca.DIFF, ca.ESTIMATED, ca.BORDER)]
    e_a, e_b, e_plain = cn.expected("icosphere_2"), cn.expected("holey_disc_20"), cn.expected("closed_sphere")
    est_blob = ca.encode(base, normal_prediction=ca.ESTIMATED, with_color=False, with_uv=False)
    e_unbound = cn.Expected(est_blob, cn.twins("torus_24_12")[1])
    two = synth.merge([synth.torus(24, 12), synth.icosphere(2)])
    two.groups = np.array([576, two.nface], dtype=np.uint32)
    e_two = cn.Expected(*cn.twins_of(two))
    e_nm = cn.Expected(*cn.twins_of(synth.non_manifold(base, seed=3)))
    cloud = ca.encode(synth.point_cloud(20, 10), normal_prediction=ca.DIFF)      # (a cloud's ESTIMATED / BORDER normals are never written: src/decoder.cpp:142-143)
    blobs = stored + [e_a.bare, e_b.bare, e_plain.bare, est_blob, e_two.bare, e_nm.bare, cloud]
    I_PLAIN, I_UNBOUND, I_TWO, I_NM, I_CLOUD = 5, 6, 7, 8, 9
    for single in (False, True):
        for fmt, i16 in FORMATS[:2]:
            b = ca.Batch(ctxs[single], blobs)
            outs = b.allocate_outputs(fill=FILL, normal_format=fmt, index16=i16, computed_normals=True)
            assert b.groups(I_TWO) == [576, two.nface]
            assert "normal" in outs[I_PLAIN]
            b.bind_computed_normals(I_PLAIN, None)                          # a normal-less mesh without the binding: its tensor stays as filled
            # the stored ESTIMATED normal of blob I_UNBOUND: unbound, and computed into the tensor that was allocated for it
            binds, first = b._keep[1], sum(info.nattr for info in b.infos[:I_UNBOUND])
            mine = [binds[first + k] for k in range(b.infos[I_UNBOUND].nattr)]
            names = [a["name"] for a in b.infos[I_UNBOUND].attrs()]
            nptr = mine[names.index("normal")].buffer
            loose = [binding(None if n == "normal" else bd.buffer, bd.format, bd.stride) for n, bd in zip(names, mine)]
            b.bind(I_UNBOUND, loose, outs[I_UNBOUND]["index"][0].data_ptr(), ca.FMT_UINT16 if i16 else ca.FMT_UINT32)
            b.bind_computed_normals(I_UNBOUND, nptr, fmt)
            run(b)
            for i in range(3):
                ref = oc.decode(blobs[i], normal_format=fmt, index16=i16)
                cn.assert_same(b.host_outputs(i), ref, [k for k in ref if k not in ("nvert", "nface")], ("stored", i, fmt, single))
            for i, e in ((3, e_a), (4, e_b), (I_UNBOUND, e_unbound), (I_TWO, e_two), (I_NM, e_nm)):
                cn.assert_same(b.host_outputs(i), e.outputs(fmt, i16), KEYS, ("computed", i, fmt, single))
            got = b.host_outputs(I_PLAIN)
            cn.assert_same(got, e_plain.outputs(fmt, i16), ["position", "index"], ("plain", fmt, single))
            assert (got["normal"].view(np.uint8) == FILL).all()
            ref = oc.decode(cloud, normal_format=fmt)
            cn.assert_same(b.host_outputs(I_CLOUD), ref, [k for k in ref if k not in ("nvert", "nface")], ("cloud", fmt, single))
            b.close()


# ---- a pipelined lane ----

def test_pipelined_lane():
    """two batch objects on a single-stream context through crthip_batch_decode_with_next, computed normals in both"""
    seq = [["torus_24_12", "holey_disc_20", "icosphere_2"], ["bumpy_sphere_16_8", "closed_sphere"], ["icosphere_2", "torus_24_12"], ["holey_disc_20"]]
    ctx = make_ctx(True)
    objs = [ca.Batch(ctx, []), ca.Batch(ctx, [])]
    objs[1].set_parity(1)
    try:
        def collect(o, names):
            st = o.sync()
            assert (st == 0).all(), st
            for i, n in enumerate(names):
                cn.assert_same(o.host_outputs(i), cn.expected(n).outputs(ca.FMT_INT16, True), KEYS, ("lane", names, i))
        prev = None
        for k, names in enumerate(seq):
            o = objs[k & 1]
            o.reset([cn.expected(n).bare for n in names])
            o.allocate_outputs(fill=FILL, normal_format=ca.FMT_INT16, index16=True, computed_normals=True)
            if prev is None:
                o.decode_entropy()
            else:
                prev[0].decode_with_next(o)
                collect(*prev)
            prev = (o, names)
        prev[0].decode_with_next(None)
        collect(*prev)
    finally:
        for o in objs:
            o.close()
        ctx.close()


# ---- lifetime and errors ----

def test_lifetime_and_errors(ctxs):
    L = ca.lib()
    e = cn.expected("torus_24_12")
    est_blob = ca.encode(synth.torus(24, 12), normal_prediction=ca.ESTIMATED, with_color=False, with_uv=False)
    cloud = ca.encode(synth.point_cloud(20, 10), normal_prediction=ca.DIFF)
    blobs = [e.bare, cloud, est_blob]
    nbuf = device_bytes(e.nvert * 12 + 16)

    def call(b, i, ptr, fmt=ca.FMT_FLOAT, stride=0):
        return L.crthip_batch_bind_computed_normals(b.handle, i, C.c_void_p(ptr) if ptr else None, fmt, stride)

    def decoded(b, computed):
        """decode; blob 0's own outputs and the others are the oracle's; nbuf holds the computed normals or is untouched"""
        nbuf.fill_(FILL)
        import torch
        torch.cuda.synchronize()
        run(b)
        for i, blob in enumerate(blobs):
            ref = oc.decode(blob)
            cn.assert_same(b.host_outputs(i), ref, [k for k in ref if k not in ("nvert", "nface")], ("untouched", i))
        raw = nbuf.cpu().numpy()
        if computed:
            assert raw[:e.nvert * 12].tobytes() == e.normal(ca.FMT_FLOAT).tobytes()
            assert (raw[e.nvert * 12:] == FILL).all()
        else:
            assert (raw == FILL).all()

    b = ca.Batch(ctxs[False], blobs)
    b.allocate_outputs(fill=FILL)
    p = nbuf.data_ptr()
    # every error of the call, each with the decode that follows untouched
    for args, code in [((3, p), E_ARGUMENT), ((1, p), E_ARGUMENT), ((2, p), E_ARGUMENT), ((0, p, ca.FMT_FLOAT, 10), E_ARGUMENT),
                       ((0, p, ca.FMT_FLOAT, 8), E_ARGUMENT), ((0, p, ca.FMT_INT16, 7), E_ARGUMENT), ((0, p, ca.FMT_INT16, 4), E_ARGUMENT),
                       ((0, p + 2, ca.FMT_FLOAT), E_ARGUMENT), ((0, p + 1, ca.FMT_INT16), E_ARGUMENT),
                       ((0, p, ca.FMT_UINT8), E_FORMAT), ((0, p, ca.FMT_DOUBLE), E_FORMAT), ((0, p, ca.FMT_INT32), E_FORMAT)]:
        assert call(b, *args) == code, (args, code)
        if args[0] < 3:
            assert ("blob %d" % args[0]).encode() in L.crthip_last_error(), L.crthip_last_error()
    decoded(b, False)
    # the position rule of a stored ESTIMATED normal: unbound, or bound as stream values
    pos = b._keep[1][0]
    idx = b.outputs[0]["index"][0].data_ptr()
    b.bind(0, [binding(None, ca.FMT_FLOAT)], idx)
    assert call(b, 0, p) == E_NEEDS_POSITION and b"blob 0" in L.crthip_last_error()
    b.bind(0, [binding(pos.buffer, ca.FMT_INT32, 0, 1)], idx)               # CRTHIP_BIND_STREAM_VALUES
    assert call(b, 0, p) == E_NEEDS_POSITION
    b.rebind()
    decoded(b, False)
    # the binding, and what drops it: NULL, a re-bind of the blob, a reset
    assert call(b, 0, p) == 0
    decoded(b, True)
    decoded(b, True)                                                        # (it stays from decode to decode)
    assert call(b, 0, None) == 0
    decoded(b, False)
    assert call(b, 0, p) == 0
    b.bind(0, [binding(pos.buffer, ca.FMT_FLOAT)], idx)
    decoded(b, False)
    assert call(b, 0, p) == 0
    b.reset(blobs)
    b.allocate_outputs(fill=FILL)
    decoded(b, False)
    assert call(b, 0, p, ca.FMT_FLOAT, 12) == 0                             # (the packed size as a stride is the packed layout)
    decoded(b, True)
    b.close()
