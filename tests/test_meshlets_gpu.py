"""GPU (-m gpu): crthip_batch_bind_meshlets - the kernels against the sequential model of the contract (tests/meshlets.py), raw bytes.  All three
arrays of every blob live in one device buffer pre-filled with 0xCD, at exactly crthip_meshlet_bound: nothing past the counts may change."""
import ctypes as C
import functools

import numpy as np
import pytest

import corto_amd as ca
import meshlets as ml
from conftest import CLOUD_CASES, MESH_CASES, load_golden
from corto_amd import synth

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = ml.FILL
A = ml.E_ARGUMENT
BLOB, SEGS, PLACE = "meshlet_blob", "meshlet_segments", "meshlet_place"


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


def run(b):
    b.decode()
    st = b.sync()
    assert (st == 0).all(), st
    return st


@functools.lru_cache(maxsize=None)
def model(name, params):
    idx, groups, _ = ml.golden(name)
    exp = ml.build(idx, groups, *params)
    ml.check_properties(idx, groups, params, *exp, tag=(name, params, "model"))
    return exp


class Bound:
    """meshlet bindings of some blobs of a batch, each with parameters of its own: one poisoned device buffer, every array at exactly the bound
    with poisoned gaps between them, a device counts record a blob"""

    def __init__(self, b, params, fill=FILL):
        import torch
        self.b, self.params, self.at, off = b, dict(params), {}, 0
        for i, p in self.params.items():
            bd = ca.meshlet_bound(b.infos[i].nface, b.groups(i), *p)
            o = []
            for n in (bd.meshlets * 16, bd.vertices * 4, bd.triangle_bytes, 16):
                off = (off + 255) & ~255
                o.append((off, n))
                off += n
            self.at[i] = (bd, o)
        self.buf = torch.full((off + 256,), fill, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        self.fill = fill
        self.bind()

    def binding(self, i):
        bd, o = self.at[i]
        base = self.buf.data_ptr()
        return ca.MeshletBinding(base + o[0][0], base + o[1][0], base + o[2][0], base + o[3][0], bd.meshlets, bd.vertices, bd.triangle_bytes, *self.params[i])

    def bind(self):
        for i in self.params:
            self.b.bind_meshlets(i, self.binding(i))

    def read(self):
        """after sync: {blob: (meshlets, vertices, triangles, counts)}; asserts that nothing but [0, counts) of every array and the device records
        changed, and that the device record is the host's"""
        host = self.buf.cpu().numpy()
        untouched = np.ones(len(host), bool)
        res = {}
        for i, (bd, o) in self.at.items():
            c = self.b.meshlet_counts(i)
            arrays = [host[s:s + n] for s, n in o]
            assert tuple(arrays[3].view(np.uint32)) == c.as_tuple(), (i, arrays[3].view(np.uint32), c.as_tuple())
            for (s, n), used in zip(o, (c.meshlets * 16, c.vertices * 4, c.triangle_bytes, 16)):
                assert used <= n, (i, used, n)
                untouched[s:s + used] = False
            res[i] = ca.cut_meshlets(arrays[0], arrays[1], arrays[2], c) + (c,)
        assert (host[untouched] == self.fill).all(), "bytes past the counts were written"
        return res


def index_kw(mode):
    return {"u32": dict(index16=False), "u16": dict(index16=True), "unbound": dict(only={"position"})}[mode]


def golden_batch(ctx, mode, names=MESH_CASES):
    b = ca.Batch(ctx, [ml.golden(n)[2] for n in names])
    b.allocate_outputs(fill=FILL, **index_kw(mode))
    return b


def expect_ran(b, blob, segments):
    ran = set(b.kernel_times())
    assert (BLOB in ran) == blob and (SEGS in ran) == segments and (PLACE in ran) == segments, sorted(k for k in ran if k.startswith("meshlet"))


# ---- 1. the kernels equal the model: the golden meshes, every index form, the parameter table and the window edges ----

EDGES = [(64, t, 0) for t in (63, 64, 65, 128, 129)] + [(64, 124, s) for s in (63, 65)]           # (segment_faces 64 is in the table)


@pytest.mark.parametrize("mode", ["u32", "u16", "unbound"])
def test_kernels_equal_model(ctx, mode):
    b = golden_batch(ctx, mode)
    for k, params in enumerate(ml.PARAMS + EDGES):
        mb = Bound(b, {i: params for i in range(len(MESH_CASES))})
        run(b)
        if mode != "unbound" and k == 0:                                            # (the model's index is the one this decode left)
            for i, n in enumerate(MESH_CASES):
                assert (b.host_outputs(i)["index"].astype(np.uint32) == ml.golden(n)[0]).all(), n
        for i, got in mb.read().items():
            ml.assert_same(got, model(MESH_CASES[i], params), (mode, params, MESH_CASES[i]))
        nsegs = [ca.meshlet_bound(len(ml.golden(n)[0]), ml.golden(n)[1], *params).segments for n in MESH_CASES]
        expect_ran(b, min(nsegs) <= 4, max(nsegs) > 4)
    b.close()


def test_segment_faces_around_a_divisor_of_nface(ctx):
    """nface a multiple of segment_faces, and that segment_faces - 1 and + 1: the last segment full, one face long, one short"""
    b = golden_batch(ctx, "u32")
    for d in (-1, 0, 1):
        params = {}
        for i, n in enumerate(MESH_CASES):
            nf = len(ml.golden(n)[0])
            params[i] = (64, 124, (nf // 2 if nf % 2 == 0 else nf) + d)
        mb = Bound(b, params)
        run(b)
        for i, got in mb.read().items():
            ml.assert_same(got, model(MESH_CASES[i], params[i]), (d, params[i], MESH_CASES[i]))
    b.close()


def test_table_load_confetti(ctx):
    """the golden confetti at (255, 512), and a confetti of one-face components - three new vertices EVERY face, so 85 faces fill a meshlet to
    255 vertices and a window adds 192 claims to them: the most a wave's table ever holds"""
    b = golden_batch(ctx, "u32", ["confetti"])
    for params in ((255, 512, 0), (255, 85, 0), (254, 512, 0)):
        mb = Bound(b, {0: params})
        run(b)
        ml.assert_same(mb.read()[0], model("confetti", params), params)
    b.reset([ca.aligned_blob(ca.encode(synth.confetti(300, seed=5, max_faces=1), with_normal=False, with_color=False, with_uv=False))])
    b.allocate_outputs(fill=FILL)
    assert b.infos[0].nface == 300 and b.infos[0].nvert == 900
    for params in ((255, 512, 0), (254, 512, 0), (255, 84, 128)):
        mb = Bound(b, {0: params})
        run(b)
        idx = b.host_outputs(0)["index"]
        got = mb.read()[0]
        ml.assert_same(got, ml.build(idx, (), *params), params)
        ml.check_properties(idx, (), params, *got[:3], got[3].as_tuple(), tag=params)
        assert got[0][:, 2].max() == min(params[0] // 3, params[1]) * 3
    b.close()


# ---- 2. both partitions on bigger meshes: a C4 unit, two default segments, vertex ids beyond 16 bits ----

@functools.lru_cache(maxsize=None)
def big(name):
    mesh = {"c4_unit": lambda: synth.bumpy_sphere(64, 32), "past_4096": lambda: synth.bumpy_sphere(64, 33), "ids_past_16_bits": lambda: synth.bumpy_sphere(256, 257)}[name]()
    return ca.aligned_blob(ca.encode(mesh, with_normal=False, with_color=False, with_uv=False))


@pytest.mark.parametrize("name,nface,nsegs", [("c4_unit", 4096, 1), ("past_4096", 4224, 2), ("ids_past_16_bits", 131584, 33)])
def test_partitions_on_bigger_meshes(ctx, name, nface, nsegs):
    b = ca.Batch(ctx, [big(name)])
    b.allocate_outputs(fill=FILL)
    assert b.infos[0].nface == nface
    mb = Bound(b, {0: (64, 124, 0)})
    run(b)
    idx = b.host_outputs(0)["index"]
    got = mb.read()[0]
    assert got[3].segments == nsegs
    if name == "ids_past_16_bits":
        assert idx.max() >= 65536 and got[1].max() >= 65536
    exp = ml.build(idx, (), 64, 124, 0)
    ml.assert_same(got, exp, name)
    ml.check_properties(idx, (), (64, 124, 0), *got[:3], got[3].as_tuple(), tag=name)
    expect_ran(b, nsegs <= 4, nsegs > 4)
    b.close()


# ---- 3. a mixed batch: bound and unbound blobs, a cloud, both partitions; every other output as without the binding ----

MIX = ["two_groups", "cloud_diff", "torus", "group_props", "icosphere", "confetti"]
MIX_PARAMS = {0: (64, 124, 0), 3: (32, 40, 100), 5: (8, 4, 16)}                                     # two_groups: 2 segments; group_props: 4 groups cut again; confetti: many


def mix_blobs():
    return [load_golden(n)["crt"] for n in MIX]


def same_outputs(a, b, tag):
    assert set(a) == set(b), (tag, sorted(a), sorted(b))
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (tag, k)


def check_mix(b, mb, plain, tag):
    got = mb.read()
    for i, params in MIX_PARAMS.items():
        ml.assert_same(got[i], model(MIX[i], params), (tag, MIX[i]))
    for i in range(len(MIX)):
        same_outputs(b.host_outputs(i), plain[i], (tag, MIX[i]))
        if i not in MIX_PARAMS:
            with pytest.raises(ca.CortoError):
                b.meshlet_counts(i)


@pytest.fixture(scope="module")
def mix_plain(ctx):
    p = ca.Batch(ctx, mix_blobs())
    p.allocate_outputs(fill=FILL)
    st = run(p)
    assert not any(k.startswith("meshlet") for k in p.kernel_times())
    ref = [p.host_outputs(i) for i in range(len(MIX))]
    p.close()
    return ref, st


def test_mixed_batch(ctx, mix_plain):
    b = ca.Batch(ctx, mix_blobs())
    b.allocate_outputs(fill=FILL)
    mb = Bound(b, MIX_PARAMS)
    st = run(b)
    assert (st == mix_plain[1]).all()
    expect_ran(b, True, True)
    check_mix(b, mb, mix_plain[0], "first")
    # decoded twice in a row: the same bytes over the old ones, and over fresh poison
    run(b)
    check_mix(b, mb, mix_plain[0], "again")
    mb2 = Bound(b, MIX_PARAMS, fill=0x3C)
    run(b)
    check_mix(b, mb2, mix_plain[0], "other buffers")
    # ... re-planned for other blobs, and back
    b.reset([ml.golden("torus")[2], ml.golden("decimated")[2]])
    b.allocate_outputs(fill=FILL)
    with pytest.raises(ca.CortoError):
        b.meshlet_counts(0)
    mo = Bound(b, {1: (64, 124, 64), 0: (16, 16, 0)})
    run(b)
    got = mo.read()
    ml.assert_same(got[1], model("decimated", (64, 124, 64)), "reset decimated")
    ml.assert_same(got[0], model("torus", (16, 16, 0)), "reset torus")
    b.reset(mix_blobs())
    b.allocate_outputs(fill=FILL)
    mb3 = Bound(b, MIX_PARAMS)
    run(b)
    check_mix(b, mb3, mix_plain[0], "back")
    b.close()


def test_allocate_outputs_binds_every_mesh(ctx, mix_plain):
    b = ca.Batch(ctx, mix_blobs())
    b.allocate_outputs(fill=FILL, meshlets=(64, 124, 64))
    run(b)
    for i, n in enumerate(MIX):
        same_outputs(b.host_outputs(i), mix_plain[0][i], n)
        if n in CLOUD_CASES:
            with pytest.raises(ca.CortoError):
                b.meshlet_counts(i)
            continue
        m, v, t = b.meshlets(i)
        ml.assert_same((m, v, t, b.meshlet_counts(i)), model(n, (64, 124, 64)), n)
    b.close()


def test_decode_with_next_parity_1(mix_plain):
    """as `cur` and as `next` of crthip_batch_decode_with_next, the second object on parity 1 of a single-stream context"""
    c = make_ctx(True)
    objs = [ca.Batch(c, []), ca.Batch(c, [])]
    objs[1].set_parity(1)
    try:
        other = ["holey_disc", "c4_unit", "nonmanifold_fins"]
        oparams = {0: (64, 124, 0), 1: (64, 124, 512), 2: (12, 20, 0)}
        objs[0].reset(mix_blobs())
        objs[0].allocate_outputs(fill=FILL)
        m0 = Bound(objs[0], MIX_PARAMS)
        objs[1].reset([ml.golden(n)[2] for n in other])
        objs[1].allocate_outputs(fill=FILL)
        m1 = Bound(objs[1], oparams)
        objs[0].decode_entropy()
        objs[0].decode_with_next(objs[1])
        st0 = objs[0].sync()
        objs[1].decode_with_next(None)
        st1 = objs[1].sync()
        assert (st0 == mix_plain[1]).all() and (st1 == 0).all()
        check_mix(objs[0], m0, mix_plain[0], "cur")
        got = m1.read()
        for i, n in enumerate(other):
            ml.assert_same(got[i], model(n, oparams[i]), ("next", n))
            assert (objs[1].host_outputs(i)["index"] == ml.golden(n)[0]).all()
    finally:
        for o in objs:
            o.close()
        c.close()


# ---- 4. bind-time errors and lifetime ----

def test_errors_and_lifetime(ctx):
    L = ca.lib()
    b = ca.Batch(ctx, [ml.golden("torus")[2], load_golden("cloud_diff")["crt"], ml.golden("two_groups")[2]])
    b.allocate_outputs(fill=FILL)
    mb = Bound(b, {0: (64, 124, 0), 2: (64, 124, 0)})
    good = mb.binding(0)

    def call(i, m):
        return L.crthip_batch_bind_meshlets(b.handle, i, C.byref(m) if m is not None else None)

    def variant(**kw):
        m = ca.MeshletBinding.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    assert L.crthip_batch_bind_meshlets(None, 0, C.byref(good)) == A
    assert call(3, good) == A and b"no such blob" in L.crthip_last_error()
    assert call(1, good) == A and b"point cloud" in L.crthip_last_error() and b"blob 1" in L.crthip_last_error()
    table = [dict(max_vertices=2), dict(max_vertices=256), dict(max_triangles=0), dict(max_triangles=513), dict(segment_faces=65537),
             dict(meshlets=None), dict(vertices=None), dict(triangles=None),
             dict(meshlets=good.meshlets + 8), dict(vertices=good.vertices + 2), dict(triangles=good.triangles + 1), dict(counts=good.counts + 8),
             dict(meshlet_capacity=good.meshlet_capacity - 1), dict(vertex_capacity=good.vertex_capacity - 1), dict(triangle_capacity=good.triangle_capacity - 1)]
    for kw in table:
        assert call(0, variant(**kw)) == A, kw
        assert b"blob 0" in L.crthip_last_error(), (kw, L.crthip_last_error())
    # every blob is held to the bound of its OWN index and group table
    bd2 = ca.meshlet_bound(b.infos[2].nface, b.groups(2), 64, 124, 0)
    assert call(2, variant(meshlet_capacity=bd2.meshlets - 1)) == A and b"blob 2" in L.crthip_last_error()
    for kw in (dict(max_vertices=3), dict(max_vertices=255, max_triangles=512), dict(max_triangles=1, segment_faces=65536), dict(counts=None)):   # the ranges' ends
        m = variant(**kw)
        bd = ca.meshlet_bound(b.infos[0].nface, b.groups(0), m.max_vertices, m.max_triangles, m.segment_faces)
        ok = bd.meshlets <= m.meshlet_capacity and bd.triangle_bytes <= m.triangle_capacity
        assert call(0, m) == (0 if ok else A), kw
    # before any decode, and for a blob that was not bound: no counts
    with pytest.raises(ca.CortoError):
        b.meshlet_counts(0)
    mb.bind()
    run(b)
    assert b.meshlet_counts(0).meshlets > 0 and b.meshlet_counts(2).segments == 2
    # NULL removes it; a later bind of the blob drops it
    assert call(0, None) == 0
    run(b)
    with pytest.raises(ca.CortoError):
        b.meshlet_counts(0)
    assert b.meshlet_counts(2).segments == 2
    b._meshlets = {}
    b.rebind()                                                                      # (crthip_batch_bind_all: every blob bound again)
    run(b)
    assert not any(k.startswith("meshlet") for k in b.kernel_times())
    for i in (0, 2):
        with pytest.raises(ca.CortoError):
            b.meshlet_counts(i)
    b.close()


# ---- measurement (run with -s): no threshold ----

def test_print_kernel_times():
    """256 C4 units (4 096 faces each), seven decodes on a single-stream context: meshlet_blob at (64, 124, default) and at segment_faces 1 024
    (four waves a blob) beside normal_blob_computed on the same batch, and that kernel without meshlets"""
    c = make_ctx(True)
    blob = ca.aligned_blob(ca.encode(synth.bumpy_sphere(64, 32), with_color=False, with_normal=False))
    for params in ((64, 124, 0), (64, 124, 1024), None):
        b = ca.Batch(c, [blob] * 256)
        b.allocate_outputs(normal_format=ca.FMT_INT16, index16=True, computed_normals=True, meshlets=params)
        rows = {}
        for _ in range(7):
            run(b)
            for k, v in b.kernel_times().items():
                if k.startswith("meshlet") or k == "normal_blob_computed":
                    rows.setdefault(k, []).append(round(1000.0 * v["ms"], 1))
        print("\nkernel times (us), 7 decodes of 256 x 4096 faces, meshlets %s:" % (params,), rows)
        if params:
            print("  counts of a blob:", b.meshlet_counts(0).as_tuple())
        assert (BLOB in rows) == (params is not None)
        b.close()
    c.close()
