"""GPU (-m gpu): crthip_batch_bind_meshlet_bounds - the kernel against the sequential model of the record (tests/meshlet_bounds.py), raw bytes.
The meshlet arrays and the records of every blob live in device buffers pre-filled with 0xCD, each array at exactly its bound: nothing past
the counts may change, and every other output of the batch is what a batch without the binding gets."""
import ctypes as C

import numpy as np
import pytest

import computed_tangents as ct
import corto_amd as ca
import meshlet_bounds as mb
import meshlets as ml
from conftest import CLOUD_CASES, MESH_CASES, load_golden
from corto_amd import synth
from oracle import oracle as oc
from test_meshlets_gpu import MIX, MIX_PARAMS, Bound, big, index_kw, make_ctx, mix_blobs, run, same_outputs

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(180)]

FILL = mb.FILL
A, NP = mb.E_ARGUMENT, mb.E_NEEDS_POSITION
KERNEL = "meshlet_bounds"
# (64, 124, 0) and (255, 512, 65536): meshlet_blob in front; (3, 1, 1) and (64, 124, 64): meshlet_segments / meshlet_place for all but the smallest
PARAMS = [(64, 124, 0), (3, 1, 1), (255, 512, 65536), (64, 124, 64)]


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


class BoundB(Bound):
    """Bound (tests/test_meshlets_gpu.py) with a record array for the blobs in `with_bounds` (default: all of params) in a second poisoned
    buffer, each at exactly the bound's meshlets"""

    def __init__(self, b, params, with_bounds=None, fill=FILL, device_counts=True):
        import torch
        self.with_bounds = sorted(params if with_bounds is None else with_bounds)
        self.device_counts = device_counts
        self.bat, off = {}, 0
        for i in self.with_bounds:
            cap = ca.meshlet_bound(b.infos[i].nface, b.groups(i), *params[i]).meshlets
            off = (off + 255) & ~255
            self.bat[i] = (off, cap)
            off += cap * 48
        self.bbuf = torch.full((off + 256,), fill, dtype=torch.uint8, device="cuda:0")
        super().__init__(b, params, fill)

    def binding(self, i):
        m = super().binding(i)
        if not self.device_counts:
            m.counts = None                                                        # (the kernel then reads a copy in the blob's scratch)
        return m

    def bind(self):
        super().bind()
        for i in self.with_bounds:
            o, cap = self.bat[i]
            self.b.bind_meshlet_bounds(i, self.bbuf.data_ptr() + o, cap)

    def read(self):
        if self.device_counts:
            return super().read()
        host = self.buf.cpu().numpy()                                              # (without the device records: their 16 bytes keep the fill)
        res = {}
        for i, (bd, o) in self.at.items():
            c = self.b.meshlet_counts(i)
            arrays = [host[s:s + n] for s, n in o]
            assert (arrays[3] == self.fill).all()
            res[i] = ca.cut_meshlets(arrays[0], arrays[1], arrays[2], c) + (c,)
        return res

    def read_bounds(self):
        """after sync: {blob: records}; asserts that nothing but [0, counts.meshlets) of every record array changed"""
        host = self.bbuf.cpu().numpy()
        untouched = np.ones(len(host), bool)
        res = {}
        for i, (o, cap) in self.bat.items():
            n = self.b.meshlet_counts(i).meshlets
            assert n <= cap
            untouched[o:o + n * 48] = False
            res[i] = host[o:o + n * 48].view(mb.DT).copy()
        assert (host[untouched] == self.fill).all(), "bytes past the counts were written"
        return res

    def untouched(self):
        return bool((self.bbuf.cpu().numpy() == self.fill).all())


def check_golden(bb, names, params, tag):
    """meshlets and bounds of a batch of golden meshes, all at `params`, against the models"""
    meshlets, bounds = bb.read(), bb.read_bounds()
    for i, n in enumerate(names):
        build, exp = mb.golden_build(n, params)
        ml.assert_same(meshlets[i], build, (tag, params, n))
        mb.assert_same(bounds[i], exp, (tag, params, n))


# ---- 1. the kernel equals the model: the golden meshes, every index form, both meshlet paths in front ----

@pytest.mark.parametrize("mode", ["u32", "u16", "unbound"])
def test_kernel_equals_model(ctx, mode):
    blobs = [mb.golden(n)[3] for n in MESH_CASES]
    kw = dict(index_kw(mode))
    kw["only"] = {"position"} | ({"index"} if mode != "unbound" else set())
    plain = ca.Batch(ctx, blobs)
    plain.allocate_outputs(fill=FILL, **kw)
    run(plain)
    ref = [plain.host_outputs(i) for i in range(len(blobs))]
    plain.close()
    b = ca.Batch(ctx, blobs)
    b.allocate_outputs(fill=FILL, **kw)
    for k, params in enumerate(PARAMS):
        bb = BoundB(b, {i: params for i in range(len(blobs))}, device_counts=k != 1)
        run(b)
        assert KERNEL in b.kernel_times()
        check_golden(bb, MESH_CASES, params, mode)
        for i, n in enumerate(MESH_CASES):                                         # the position reached its dequantisation intact
            same_outputs(b.host_outputs(i), ref[i], (mode, params, n))
    b.close()


def packed_position(host, nvert, stride):
    return np.lib.stride_tricks.as_strided(host, shape=(nvert, 12), strides=(stride, 1)).copy().view(np.float32)


@pytest.mark.parametrize("kind", ["strided", "quantized", "computed_normals"])
def test_position_bindings(ctx, kind):
    """the position at a stride and as uint16 grid values (read from scratch), and with computed normals bound beside the bounds (the fused
    normal kernel no longer dequantises the position): the records are the model's, every output what a batch without bounds gets"""
    import torch
    params = (64, 124, 0)
    names = MESH_CASES
    kw = dict(fill=FILL)
    if kind == "quantized":
        kw["quantized"] = ("position",)
        names = [n for n in MESH_CASES if int((mb.golden(n)[0].max(0).astype(np.int64) - mb.golden(n)[0].min(0)).max()) < 65536]   # (a wider span is refused as uint16)
        assert len(names) > len(MESH_CASES) // 2
    blobs = [mb.golden(n)[3] for n in names]
    if kind == "computed_normals":
        kw["computed_normals"] = True
        kw["only"] = {"position", "index", "normal"}
    res = []
    for bounds in (False, True):
        b = ca.Batch(ctx, blobs)
        b.allocate_outputs(**kw)
        sbuf = None
        if kind == "strided":                                                      # every blob's position again, 20 bytes a vertex in a buffer of its own
            offs = np.cumsum([0] + [(info.nvert * 20 + 255) & ~255 for info in b.infos])
            sbuf = torch.full((int(offs[-1]) + 256,), FILL, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            binds, first = b._keep[1], 0
            for i, info in enumerate(b.infos):
                mine = []
                for k, a in enumerate(info.attrs()):
                    bd = ca.AttrBinding()
                    src = binds[first + k]
                    bd.buffer, bd.format, bd.out_components, bd.stride, bd.reserved = src.buffer, src.format, src.out_components, src.stride, src.reserved
                    if a["name"] == "position":
                        bd.buffer, bd.stride = sbuf.data_ptr() + int(offs[i]), 20
                    mine.append(bd)
                b.bind(i, mine, b.outputs[i]["index"][0].data_ptr())
                first += info.nattr
        bb = BoundB(b, {i: params for i in range(len(blobs))}) if bounds else Bound(b, {i: params for i in range(len(blobs))})
        run(b)
        assert (KERNEL in b.kernel_times()) == bounds
        outs = [b.host_outputs(i) for i in range(len(blobs))]
        if kind == "strided":
            host = sbuf.cpu().numpy()
            for i, info in enumerate(b.infos):
                outs[i]["position"] = packed_position(host[int(offs[i]):], info.nvert, 20)
                gaps = np.lib.stride_tricks.as_strided(host[int(offs[i]) + 12:], shape=(info.nvert, 8), strides=(20, 1))
                assert (gaps == FILL).all()
        if kind == "quantized":
            for i in range(len(blobs)):
                outs[i]["position transform"] = np.frombuffer(bytes(b.quant_transform(i, "position")), np.uint8)
        if bounds:
            check_golden(bb, names, params, kind)
        res.append(outs)
        b.close()
    for i, n in enumerate(names):
        same_outputs(res[1][i], res[0][i], (kind, n))
        if kind == "strided":                                                      # ... and the strided floats are the oracle's
            assert res[1][i]["position"].tobytes() == np.ascontiguousarray(oc.decode(blobs[i])["position"], np.float32).tobytes(), n


def test_with_computed_tangents(ctx):
    """tangents read the integer positions too, in front of the bounds: both get them, and k_dequant what they leave"""
    params = (8, 4, 16)
    es = [ct.inputs(n) for n in ct.NAMES]
    res = []
    for bounds in (False, True):
        b = ca.Batch(ctx, [e.blob for e in es])
        b.allocate_outputs(fill=FILL, computed_tangents=True)
        bb = BoundB(b, {i: params for i in range(len(es))}, with_bounds=range(len(es)) if bounds else ())
        run(b)
        ran = set(b.kernel_times())
        assert "tangent_blob" in ran and (KERNEL in ran) == bounds
        res.append([b.host_outputs(i) for i in range(len(es))])
        if bounds:
            meshlets, got = bb.read(), bb.read_bounds()
            for i, e in enumerate(es):
                build = ml.build(e.index, b.groups(i), *params)
                ml.assert_same(meshlets[i], build, ct.NAMES[i])
                exp = mb.model(e.P, *build[:3])
                mb.check_properties(e.P, *build[:3], got[i], tag=ct.NAMES[i])
                mb.assert_same(got[i], exp, ct.NAMES[i])
                assert (got[i]["cone_cutoff"] < 127).mean() > 0.5                 # (four faces a meshlet: most cones cull)
        b.close()
    for i, n in enumerate(ct.NAMES):
        same_outputs(res[1][i], res[0][i], n)


# ---- 2. a bigger mesh of several segments: the grid is sized by a bound several times the count ----

def test_bigger_mesh_with_several_segments(ctx):
    blob, params = big("past_4096"), (64, 124, 512)
    b = ca.Batch(ctx, [blob])
    b.allocate_outputs(fill=FILL)
    bb = BoundB(b, {0: params})
    run(b)
    ran = set(b.kernel_times())
    assert {"meshlet_segments", "meshlet_place", KERNEL} <= ran and "meshlet_blob" not in ran
    meshlets, got = bb.read()[0], bb.read_bounds()[0]
    c = meshlets[3]
    assert c.segments == 9 and bb.bat[0][1] >= 2 * c.meshlets, (c.as_tuple(), bb.bat[0])   # most launched waves return
    idx = b.host_outputs(0)["index"]
    ml.assert_same(meshlets, ml.build(idx, (), *params), "meshlets")
    P = oc.decode(blob, trace=True)["_delta_position"]
    mb.check_properties(P, *meshlets[:3], got, tag="past_4096")
    mb.assert_same(got, mb.model(P, *meshlets[:3]), "past_4096")
    assert b.host_outputs(0)["position"].tobytes() == np.ascontiguousarray(oc.decode(blob)["position"], np.float32).tobytes()
    b.close()


# ---- 3. a mixed batch: blobs with and without the binding, a cloud; every other output as without it ----

WITH_BOUNDS = (0, 5)                                                                 # two_groups (meshlet_blob in front), confetti (segments / place); group_props has meshlets only


def check_mix(b, bb, ref, tag):
    meshlets, bounds = bb.read(), bb.read_bounds()
    assert sorted(bounds) == list(WITH_BOUNDS)
    for i, params in MIX_PARAMS.items():
        build, exp = mb.golden_build(MIX[i], params)
        ml.assert_same(meshlets[i], build, (tag, MIX[i]))
        if i in WITH_BOUNDS:
            mb.assert_same(bounds[i], exp, (tag, MIX[i]))
    for i in range(len(MIX)):
        same_outputs(b.host_outputs(i), ref[i], (tag, MIX[i]))


@pytest.fixture(scope="module")
def mix_ref(ctx):
    """the batch with its meshlet bindings and without bounds: outputs, status, the kernels that ran"""
    p = ca.Batch(ctx, mix_blobs())
    p.allocate_outputs(fill=FILL)
    Bound(p, MIX_PARAMS)
    st = run(p)
    ran = set(p.kernel_times())
    assert KERNEL not in ran and "meshlet_blob" in ran
    ref = [p.host_outputs(i) for i in range(len(MIX))]
    p.close()
    return ref, st, ran


def test_mixed_batch(ctx, mix_ref):
    b = ca.Batch(ctx, mix_blobs())
    b.allocate_outputs(fill=FILL)
    bb = BoundB(b, MIX_PARAMS, with_bounds=WITH_BOUNDS)
    st = run(b)
    assert (st == mix_ref[1]).all()
    assert set(b.kernel_times()) == mix_ref[2] | {KERNEL}                            # one more name, and only with a binding
    check_mix(b, bb, mix_ref[0], "first")
    run(b)                                                                           # decoded twice in a row: the same bytes over the old ones
    check_mix(b, bb, mix_ref[0], "again")
    bb2 = BoundB(b, MIX_PARAMS, with_bounds=WITH_BOUNDS, fill=0x3C, device_counts=False)
    run(b)
    check_mix(b, bb2, mix_ref[0], "other buffers, the counts in scratch")
    # without any bounds binding the batch has the parent's kernel set again
    Bound(b, MIX_PARAMS)
    run(b)
    assert set(b.kernel_times()) == mix_ref[2]
    b.close()


def test_decode_with_next_parity_1(mix_ref):
    """as `cur` and as `next` of crthip_batch_decode_with_next, the second object on parity 1 of a single-stream context"""
    c = make_ctx(True)
    objs = [ca.Batch(c, []), ca.Batch(c, [])]
    objs[1].set_parity(1)
    try:
        other = ["holey_disc", "c4_unit", "nonmanifold_fins"]
        oparams = {0: (64, 124, 0), 1: (64, 124, 512), 2: (12, 20, 0)}
        objs[0].reset(mix_blobs())
        objs[0].allocate_outputs(fill=FILL)
        b0 = BoundB(objs[0], MIX_PARAMS, with_bounds=WITH_BOUNDS)
        objs[1].reset([mb.golden(n)[3] for n in other])
        objs[1].allocate_outputs(fill=FILL)
        b1 = BoundB(objs[1], oparams)
        objs[0].decode_entropy()
        objs[0].decode_with_next(objs[1])
        st0 = objs[0].sync()
        objs[1].decode_with_next(None)
        st1 = objs[1].sync()
        assert (st0 == mix_ref[1]).all() and (st1 == 0).all()
        check_mix(objs[0], b0, mix_ref[0], "cur")
        meshlets, bounds = b1.read(), b1.read_bounds()
        for i, n in enumerate(other):
            build, exp = mb.golden_build(n, oparams[i])
            ml.assert_same(meshlets[i], build, ("next", n))
            mb.assert_same(bounds[i], exp, ("next", n))
            assert objs[1].host_outputs(i)["position"].tobytes() == np.ascontiguousarray(oc.decode(mb.golden(n)[3])["position"], np.float32).tobytes()
    finally:
        for o in objs:
            o.close()
        c.close()


def test_allocate_outputs_binds_every_mesh(ctx):
    params = (64, 124, 64)
    b = ca.Batch(ctx, mix_blobs())
    with pytest.raises(ValueError):
        b.allocate_outputs(fill=FILL, meshlet_bounds=True)
    b.allocate_outputs(fill=FILL, meshlets=params, meshlet_bounds=True)
    run(b)
    assert KERNEL in b.kernel_times()
    for i, n in enumerate(MIX):
        if n in CLOUD_CASES:
            with pytest.raises((KeyError, ca.CortoError)):
                b.meshlet_bounds(i)
            continue
        build, exp = mb.golden_build(n, params)
        ml.assert_same(b.meshlets(i) + (b.meshlet_counts(i),), build, n)
        mb.assert_same(b.meshlet_bounds(i), exp, n)
    b.rebind()                                                                       # (the bindings are applied again, the bounds behind the meshlets)
    run(b)
    assert KERNEL in b.kernel_times()
    mb.assert_same(b.meshlet_bounds(0), mb.golden_build(MIX[0], params)[1], "rebind")
    b.close()


# ---- 4. bind-time errors and lifetime ----

def test_errors_and_lifetime(ctx):
    L = ca.lib()
    params = (64, 124, 0)
    b = ca.Batch(ctx, [mb.golden("torus")[3], load_golden("cloud_diff")["crt"], mb.golden("two_groups")[3]])
    b.allocate_outputs(fill=FILL)
    bb = BoundB(b, {0: params, 2: params}, with_bounds=())
    bb.with_bounds = [0]
    cap = ca.meshlet_bound(b.infos[0].nface, b.groups(0), *params).meshlets
    import torch
    bb.bbuf = torch.full((cap * 48 + 256,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    bb.bat = {0: (0, cap)}
    p = bb.bbuf.data_ptr()
    exp = mb.golden_build("torus", params)[1]

    def call(i, ptr, capacity):
        return L.crthip_batch_bind_meshlet_bounds(b.handle, i, C.c_void_p(ptr) if ptr else None, capacity)

    def decoded(bound):
        bb.bbuf.fill_(FILL)
        torch.cuda.synchronize()
        run(b)
        assert (KERNEL in b.kernel_times()) == bound
        if bound:
            mb.assert_same(bb.read_bounds()[0], exp, "bound")
        else:
            assert bb.untouched()

    assert L.crthip_batch_bind_meshlet_bounds(None, 0, C.c_void_p(p), cap) == A
    assert call(3, p, cap) == A and b"no such blob" in L.crthip_last_error()
    assert call(1, p, cap) == A and b"blob 1" in L.crthip_last_error()                # a point cloud: it can have no meshlet binding
    assert call(0, p, cap - 1) == A and b"blob 0" in L.crthip_last_error() and b"capacity" in L.crthip_last_error()
    assert call(0, p + 8, cap) == A and b"16-byte" in L.crthip_last_error()
    assert call(0, p, cap) == 0 and call(0, p, cap + 5) == 0
    decoded(True)
    decoded(True)                                                                    # (it stays from decode to decode)
    # NULL removes it
    assert call(0, None, 0) == 0
    decoded(False)
    assert b.meshlet_counts(0).meshlets == len(exp)                                  # (the meshlets stay)
    # removing the meshlet binding drops it, and without one it is refused
    assert call(0, p, cap) == 0
    b.bind_meshlets(0, None)
    decoded(False)
    assert call(0, p, cap) == A and b"meshlet binding" in L.crthip_last_error() and b"blob 0" in L.crthip_last_error()
    # a new meshlet binding drops it too: its capacity was checked against the old parameters
    b.bind_meshlets(0, bb.binding(0))
    assert call(0, p, cap) == 0
    b.bind_meshlets(0, bb.binding(0))
    decoded(False)
    # the position's rule, that of computed tangents
    binds, names = b._keep[1], [a["name"] for a in b.infos[0].attrs()]
    mine = [binds[k] for k in range(b.infos[0].nattr)]
    idx = b.outputs[0]["index"][0].data_ptr()

    def rebound(**changes):
        arr = []
        for n, src in zip(names, mine):
            bd = ca.AttrBinding()
            bd.buffer, bd.format, bd.out_components, bd.stride, bd.reserved = changes.get(n, (src.buffer, src.format, src.out_components, src.stride, src.reserved))
            arr.append(bd)
        b.bind(0, arr, idx)
        b.bind_meshlets(0, bb.binding(0))
    pos = mine[names.index("position")]
    rebound(position=(None, ca.FMT_FLOAT, 0, 0, 0))
    assert call(0, p, cap) == NP and b"blob 0" in L.crthip_last_error()
    rebound(position=(pos.buffer, ca.FMT_INT32, 0, 0, 1))                              # CRTHIP_BIND_STREAM_VALUES
    assert call(0, p, cap) == NP
    rebound()
    assert call(0, p, cap) == 0
    decoded(True)
    # a later bind of the blob drops both
    b._meshlets, b._meshlet_bounds = {}, {}
    b.rebind()
    decoded(False)
    assert not any(k.startswith("meshlet") for k in b.kernel_times())
    b.close()


# ---- measurement (run with -s): no threshold ----

def test_print_kernel_times():
    """256 C4 units (4 096 faces each), seven decodes on a single-stream context: meshlet_bounds beside meshlet_blob at (64, 124, default)"""
    c = make_ctx(True)
    blob = ca.aligned_blob(ca.encode(synth.bumpy_sphere(64, 32), with_color=False, with_normal=False))
    for bounds in (True, False):
        b = ca.Batch(c, [blob] * 256)
        b.allocate_outputs(normal_format=ca.FMT_INT16, index16=True, computed_normals=True, meshlets=(64, 124, 0), meshlet_bounds=bounds)
        rows = {}
        for _ in range(7):
            run(b)
            for k, v in b.kernel_times().items():
                if k.startswith("meshlet") or k in ("normal_blob_computed", "dequantize"):
                    rows.setdefault(k, []).append(round(1000.0 * v["ms"], 1))
        print("\nkernel times (us), 7 decodes of 256 x 4096 faces, meshlets (64, 124, 0), bounds %s:" % bounds, rows)
        print("  counts of a blob:", b.meshlet_counts(0).as_tuple(), "bound:", ca.meshlet_bound(b.infos[0].nface, b.groups(0), 64, 124, 0).as_tuple())
        if bounds:
            r = b.meshlet_bounds(0)
            print("  cutoffs below 127 in blob 0: %d of %d" % (int((r["cone_cutoff"] < 127).sum()), len(r)))
        assert (KERNEL in rows) == bounds
        b.close()
    c.close()
