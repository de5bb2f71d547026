"""GPU (-m gpu): crthip_batch_bind_computed_tangents - the kernels against the numpy model of the contract (tests/computed_tangents.py), raw
bytes.  The model's inputs are the oracle's integers and index and the normals the batch itself binds.  Outputs are pre-filled with 0xA5:
every element of a tangent array must have been written, and no byte beside it."""
import ctypes as C
import functools
import tempfile

import numpy as np
import pytest

import corto_amd as ca
import computed_tangents as ct
import size_classes as sc
from corto_amd import synth
from oracle import oracle as oc

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = ct.FILL
Q = ca.BIND_QUANTIZED
SOURCES = ["float", "int16", "computed"]


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


def run(b):
    b.decode()
    st = b.sync()
    assert (st == 0).all(), st
    return st


def device_bytes(n):
    import torch
    t = torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    return t


def binding(ptr, fmt, stride=0, flags=0):
    bd = ca.AttrBinding()
    bd.buffer = ptr; bd.format = fmt; bd.out_components = 0; bd.stride = stride; bd.reserved = flags
    return bd


@functools.lru_cache(maxsize=None)
def source_inputs(name, source):
    """the mesh `name` encoded for a normal source (tests/computed_tangents.py: encode)"""
    return ct.Inputs(ct.encode(ct.MESHES[name](), normals=source)) if source == "computed" else ct.inputs(name)


@functools.lru_cache(maxsize=None)
def bystanders():
    """a point cloud and a mesh without uv: in the batch, and simply without a tangent"""
    return ca.aligned_blob(ca.encode(synth.point_cloud(20, 10), normal_prediction=ca.DIFF)), ca.aligned_blob(ca.encode(synth.icosphere(1), with_uv=False))


def same_outputs(a, b, tag, skip=("tangent",)):
    assert set(a) - set(skip) == set(b) - set(skip), (tag, sorted(a), sorted(b))
    for k in a:
        if k not in skip and k not in ("nvert", "nface"):
            ct.assert_bytes(a[k], b[k], (tag, k))


def expect_tangent(e, out, fmt):
    """the model of blob inputs `e` with the normals the decode left in `out`"""
    return e.model(fmt, normal=np.ascontiguousarray(out["normal"]))[0]


# ---- 1. parity with the model, every other output untouched ----

@pytest.mark.parametrize("single", [False, True], ids=["two_stream", "single_stream"])
@pytest.mark.parametrize("source", SOURCES)
def test_parity_with_the_model(ctxs, source, single):
    es = [source_inputs(n, source) for n in ct.NAMES]
    blobs = [e.blob for e in es] + list(bystanders())
    for fmt, nfmt, i16 in ((ca.FMT_FLOAT, ca.FMT_INT16 if source == "int16" else ca.FMT_FLOAT, False), (ca.FMT_INT16, ca.FMT_FLOAT if source == "float" else ca.FMT_INT16, True)):
        kw = dict(fill=FILL, normal_format=nfmt, index16=i16, computed_normals=source == "computed")
        plain = ca.Batch(ctxs[single], blobs)
        plain.allocate_outputs(**kw)
        st0 = run(plain)
        assert not any(k.startswith("tangent") for k in plain.kernel_times())
        b = ca.Batch(ctxs[single], blobs)
        outs = b.allocate_outputs(computed_tangents=True, tangent_format=fmt, **kw)
        st = run(b)
        ran = set(b.kernel_times())
        assert "tangent_blob" in ran and "tangent_faces" not in ran and "tangent_vertex" not in ran, sorted(ran)
        assert (st == st0).all()
        for i, e in enumerate(es):
            got, ref = b.host_outputs(i), plain.host_outputs(i)
            same_outputs(got, ref, (source, fmt, ct.NAMES[i]))                 # position, uv, normal, index: the deferred dequantisation changes nothing
            if source != "computed":                                            # ... and they are the oracle's
                o = oc.decode(e.blob, normal_format=nfmt, index16=i16)
                same_outputs(got, o, (source, fmt, ct.NAMES[i], "oracle"))
                ct.assert_bytes(got["tangent"], e.model(fmt, nfmt)[0], (source, fmt, nfmt, ct.NAMES[i], "oracle's normals"))
            assert got["tangent"].shape == (e.nvert, 4)
            ct.assert_bytes(got["tangent"], expect_tangent(e, got, fmt), (source, fmt, nfmt, ct.NAMES[i]))
        for i in (len(es), len(es) + 1):
            assert "tangent" not in outs[i]
            same_outputs(b.host_outputs(i), plain.host_outputs(i), (source, fmt, "bystander", i))
        plain.close(); b.close()


# ---- 2. both size classes ----

@functools.lru_cache(maxsize=None)
def blob_max():
    with tempfile.TemporaryDirectory(prefix="tangent_probe") as d:
        p = sc.Probe(d, source="tangent_probe")
        try:
            assert p.const("LDS_AT_MAX") == 24 * p.const("TANGENT_BLOB_MAX")
            return p.const("TANGENT_BLOB_MAX")
        finally:
            p.close()


@functools.lru_cache(maxsize=None)
def sized(nvert):
    e = ct.Inputs(ct.encode(sc.closed_mesh(nvert)))
    assert e.nvert == nvert
    return e


@pytest.mark.parametrize("fmt", [ca.FMT_FLOAT, ca.FMT_INT16], ids=["f32", "i16"])
def test_both_size_classes(ctxs, fmt):
    last = blob_max()
    nfmt, i16 = (ca.FMT_FLOAT, False) if fmt == ca.FMT_INT16 else (ca.FMT_INT16, True)
    for nverts, want, never in (([last], {"tangent_blob"}, {"tangent_faces", "tangent_vertex"}), ([last + 1], {"tangent_faces", "tangent_vertex"}, {"tangent_blob"}),
                                ([last + 1, last, 3 * last + 77], {"tangent_blob", "tangent_faces", "tangent_vertex"}, set())):
        es = [sized(n) for n in nverts]
        b = ca.Batch(ctxs[fmt == ca.FMT_INT16], [e.blob for e in es])
        b.allocate_outputs(fill=FILL, normal_format=nfmt, index16=i16, computed_tangents=True, tangent_format=fmt)
        run(b)
        ran = set(b.kernel_times())
        assert want <= ran and not (never & ran), (nverts, sorted(ran))
        for i, e in enumerate(es):
            got = b.host_outputs(i)
            same_outputs(got, oc.decode(e.blob, normal_format=nfmt, index16=i16), (nverts, i, "oracle"))
            ct.assert_bytes(got["tangent"], e.model(fmt, nfmt)[0], (nverts, i, fmt))
        b.close()


# ---- 3. an interleaved record ----

def test_interleaved_record(ctxs):
    """uint16 position x 3 | pad | int16 normal x 3 | pad | int16 tangent x 4 | uint16 uv x 2: 28 bytes a vertex, and a uint16 index"""
    e = ct.inputs("torus_24_12")
    nv, nf = e.nvert, e.nface
    packed = ca.Batch(ctxs[False], [e.blob])
    packed.allocate_outputs(fill=FILL, normal_format=ca.FMT_INT16, index16=True, quantized=("position", "uv"), computed_tangents=True, tangent_format=ca.FMT_INT16)
    run(packed)
    ref = packed.host_outputs(0)
    ct.assert_bytes(ref["tangent"], e.model(ca.FMT_INT16, ca.FMT_INT16)[0], "packed")
    for single in (False, True):
        b = ca.Batch(ctxs[single], [e.blob])
        names = [a["name"] for a in b.infos[0].attrs()]
        assert sorted(names) == ["normal", "position", "uv"]
        vb, ib = device_bytes(nv * 28), device_bytes(nf * 6)
        at = {"position": (0, ca.FMT_UINT16, Q), "normal": (8, ca.FMT_INT16, 0), "uv": (24, ca.FMT_UINT16, Q)}
        b.bind(0, [binding(vb.data_ptr() + at[n][0], at[n][1], 28, at[n][2]) for n in names], ib.data_ptr(), ca.FMT_UINT16)
        b.bind_computed_tangents(0, vb.data_ptr() + 16, ca.FMT_INT16, 28)
        run(b)
        rec = vb.cpu().numpy().reshape(nv, 28)
        field = lambda o, w, dt: np.ascontiguousarray(rec[:, o:o + w]).view(dt)
        ct.assert_bytes(field(16, 8, np.int16), ref["tangent"], ("record tangent", single))
        ct.assert_bytes(field(0, 6, np.uint16), ref["position"].view(np.uint16), ("record position", single))
        ct.assert_bytes(field(8, 6, np.int16), ref["normal"], ("record normal", single))
        ct.assert_bytes(field(24, 4, np.uint16), ref["uv"].view(np.uint16), ("record uv", single))
        assert (rec[:, 6:8] == FILL).all() and (rec[:, 14:16] == FILL).all()
        ct.assert_bytes(ib.cpu().numpy().view(np.uint16).reshape(nf, 3), ref["index"], ("record index", single))
        b.close()
    packed.close()


# ---- 4. a pipelined lane ----

def test_decode_with_next_equals_plain():
    """two batch objects on parities 0 and 1 of a single-stream context, tangents bound in both: the bytes of two plain decodes"""
    groups = [(["torus_24_12", "icosphere_2", "closed_sphere"], "float"), (["holey_disc_20", "bumpy_sphere_16_8"], "computed")]
    ctx = make_ctx(True)
    objs = [ca.Batch(ctx, []), ca.Batch(ctx, [])]
    objs[1].set_parity(1)
    try:
        refs = []
        for names, source in groups:
            blobs = [source_inputs(n, source).blob for n in names]
            kw = dict(fill=FILL, normal_format=ca.FMT_INT16, index16=True, computed_normals=source == "computed", computed_tangents=True, tangent_format=ca.FMT_INT16)
            p = ca.Batch(ctx, blobs)
            p.allocate_outputs(**kw)
            run(p)
            refs.append([p.host_outputs(i) for i in range(len(blobs))])
            p.close()
        for k, (names, source) in enumerate(groups):
            objs[k].reset([source_inputs(n, source).blob for n in names])
            objs[k].allocate_outputs(fill=FILL, normal_format=ca.FMT_INT16, index16=True, computed_normals=source == "computed", computed_tangents=True,
                                     tangent_format=ca.FMT_INT16)
        objs[0].decode_entropy()
        objs[0].decode_with_next(objs[1])
        st0 = objs[0].sync()
        objs[1].decode_with_next(None)
        st1 = objs[1].sync()
        assert (st0 == 0).all() and (st1 == 0).all()
        for k, (names, source) in enumerate(groups):
            for i, n in enumerate(names):
                got = objs[k].host_outputs(i)
                same_outputs(got, refs[k][i], ("pair", k, n), skip=())
                ct.assert_bytes(got["tangent"], expect_tangent(source_inputs(n, source), got, ca.FMT_INT16), ("pair", k, n))
    finally:
        for o in objs:
            o.close()
        ctx.close()


# ---- 5. errors and lifetime ----

def test_errors_and_lifetime(ctxs):
    L = ca.lib()
    e = ct.inputs("torus_24_12")
    cloud, no_uv = bystanders()
    bare = source_inputs("icosphere_2", "computed").blob                       # no stored normal: no normal source until computed normals are bound
    three = ca.aligned_blob(ca.encode(synth.icosphere(1), with_uv=False, with_color=False, attributes=[("uv", np.zeros((42, 3), np.float32), 1.0, 0)]))
    blobs = [e.blob, cloud, no_uv, bare, three]
    tbuf = device_bytes(e.nvert * 16 + 16)
    p = tbuf.data_ptr()

    def call(b, i, ptr, fmt=ca.FMT_FLOAT, stride=0):
        return L.crthip_batch_bind_computed_tangents(b.handle, i, C.c_void_p(ptr) if ptr else None, fmt, stride)

    def decoded(b, bound):
        """decode; every blob's own outputs are the oracle's; tbuf holds blob 0's tangents or its fill"""
        import torch
        tbuf.fill_(FILL)
        torch.cuda.synchronize()
        run(b)
        for i, blob in enumerate(blobs):
            ref = oc.decode(blob)
            same_outputs(b.host_outputs(i), ref, ("untouched", i))
        raw = tbuf.cpu().numpy()
        if bound:
            assert raw[:e.nvert * 16].tobytes() == e.model(ca.FMT_FLOAT)[0].tobytes()
            assert (raw[e.nvert * 16:] == FILL).all()
        else:
            assert (raw == FILL).all()

    b = ca.Batch(ctxs[False], blobs)
    b.allocate_outputs(fill=FILL)
    A, F, NP = ct.E_ARGUMENT, ct.E_FORMAT, ct.E_NEEDS_POSITION
    for args, code in [((5, p), A), ((1, p), A), ((2, p), A), ((3, p), A), ((4, p), A),
                       ((0, p, ca.FMT_FLOAT, 12), A), ((0, p, ca.FMT_FLOAT, 18), A), ((0, p, ca.FMT_INT16, 6), A), ((0, p, ca.FMT_INT16, 9), A),
                       ((0, p + 2, ca.FMT_FLOAT), A), ((0, p + 1, ca.FMT_INT16), A),
                       ((0, p, ca.FMT_UINT8), F), ((0, p, ca.FMT_DOUBLE), F), ((0, p, ca.FMT_INT32), F), ((0, p, ca.FMT_UINT16), F)]:
        assert call(b, *args) == code, (args, code)
        if args[0] < 5:
            assert ("blob %d" % args[0]).encode() in L.crthip_last_error(), L.crthip_last_error()
    assert L.crthip_batch_bind_computed_tangents(None, 0, C.c_void_p(p), ca.FMT_FLOAT, 0) == A
    decoded(b, False)
    # the position's rule (that of computed normals), the uv's, the normal source
    binds = b._keep[1]
    names = [a["name"] for a in b.infos[0].attrs()]
    mine = [binds[k] for k in range(b.infos[0].nattr)]
    idx = b.outputs[0]["index"][0].data_ptr()

    def rebound(**changes):
        b.bind(0, [changes.get(n, binding(bd.buffer, bd.format, bd.stride)) for n, bd in zip(names, mine)], idx)
    pos, uv = mine[names.index("position")], mine[names.index("uv")]
    rebound(position=binding(None, ca.FMT_FLOAT))
    assert call(b, 0, p) == NP and b"blob 0" in L.crthip_last_error()
    rebound(position=binding(pos.buffer, ca.FMT_INT32, 0, 1))                   # CRTHIP_BIND_STREAM_VALUES
    assert call(b, 0, p) == NP
    rebound(uv=binding(None, ca.FMT_FLOAT))
    assert call(b, 0, p) == A
    rebound(uv=binding(uv.buffer, ca.FMT_INT32, 0, 1))
    assert call(b, 0, p) == A
    rebound(normal=binding(None, ca.FMT_FLOAT))
    assert call(b, 0, p) == A                                                   # no normal source
    b.rebind()
    decoded(b, False)
    # the binding, and what drops it: NULL, a re-bind of the blob, a computed-normals call, a reset
    assert call(b, 0, p) == 0
    decoded(b, True)
    decoded(b, True)                                                            # (it stays from decode to decode)
    assert call(b, 0, None) == 0
    decoded(b, False)
    assert call(b, 0, p) == 0
    rebound()
    decoded(b, False)
    assert call(b, 0, p) == 0
    assert L.crthip_batch_bind_computed_normals(b.handle, 0, None, ca.FMT_FLOAT, 0) == 0
    decoded(b, False)
    assert call(b, 0, p) == 0
    b.reset(blobs)
    b.allocate_outputs(fill=FILL)
    decoded(b, False)
    assert call(b, 0, p, ca.FMT_FLOAT, 16) == 0                                 # (the packed size as a stride is the packed layout)
    decoded(b, True)
    # computed normals as the source: refused before they are bound, taken after
    nbuf = device_bytes(162 * 12)
    assert call(b, 3, p) == A
    b.bind_computed_normals(3, nbuf.data_ptr())
    assert call(b, 3, p) == 0
    assert call(b, 3, None) == 0
    b.close()


# ---- measurement (run with -s): no threshold ----

def test_print_kernel_times():
    """256 blobs of 2 112 vertices (the flagship's unit): tangent_blob beside normal_blob_computed on the same batch, and that kernel on
    the batch without tangents (where it also turns the positions into floats, and no dequantize launch follows)"""
    ctx = make_ctx(True)
    blob = ca.aligned_blob(ct.encode(synth.bumpy_sphere(64, 32), normals="computed"))
    for tangents in (True, False):
        b = ca.Batch(ctx, [blob] * 256)
        b.allocate_outputs(normal_format=ca.FMT_INT16, index16=True, computed_normals=True, computed_tangents=tangents, tangent_format=ca.FMT_INT16)
        rows = {}
        for _ in range(7):
            run(b)
            for k, v in b.kernel_times().items():
                if k in ("tangent_blob", "normal_blob_computed", "dequantize"):
                    rows.setdefault(k, []).append(round(1000.0 * v["ms"], 1))
        print("\nkernel times (us), 7 decodes of 256 x 2112 vertices, tangents %s:" % ("bound" if tangents else "not bound"), rows)
        assert b.infos[0].nvert == 2112 and ("tangent_blob" in rows) == tangents
        b.close()
    ctx.close()
