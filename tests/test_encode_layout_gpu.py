"""GPU (-m gpu): crthip_encode_batch_layout - batches encoded straight from render-ready buffers: interleaved vertex records, int16 normals,
a uint16 index, an origin.  Every blob is held against crthip_encode_attrs (ca.encode: pinned to the reference byte for byte) of the same
data converted into packed arrays by this file in numpy float32 - index.astype(uint32), n.astype(float32) / float32(32767), pos - origin:
upstream's own single operations (src/encoder.cpp:114-119, 151-158, 77-81; tests/test_encode_layout_cpu.py has the argument).

The one hostile pointer handed over is an extent that ends four bytes behind its allocation: it is refused by the runtime's pointer
queries on the host, before anything is launched on that mesh.

One context; every input seeded.  Run as one pytest invocation under a time limit of its own."""
import numpy as np
import pytest
import torch

import corto_amd as ca
from corto_amd import synth
from test_encode_layout_cpu import BASES, F32, NVERTS, ORIGIN, STRIDES, n16_of, strided

pytestmark = pytest.mark.gpu

E_ARGUMENT = -8
MODES = ("host", "device", "split")
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ctx():
    c = ca.Context(0)
    yield c
    c.set_encode_topology("host")
    c.close()


def _check_arena(out, offs, lens, expect, total, tag):
    host = out.cpu().numpy() if isinstance(out, torch.Tensor) else out
    want_offs, want_total = ca.arena_layout(lens)
    assert offs.tolist() == want_offs.tolist() and total == want_total, tag
    for i, e in enumerate(expect):
        o, n = int(offs[i]), int(lens[i])
        assert n == len(e), (tag, i)
        assert host[o:o + n].tobytes() == e, (tag, i)
        assert not host[o + n:(o + n + 15) & ~15].any(), (tag, i, "padding")


def dev_view(v):
    """a numpy view made by strided() as a torch view of a device copy of its buffer: same stride, same offset from a 16-byte boundary"""
    buf = v.base if isinstance(v.base, np.ndarray) else np.frombuffer(v.base, dtype=np.uint8)
    while buf.base is not None and isinstance(buf.base, np.ndarray):
        buf = buf.base
    start = (-buf.ctypes.data) % 16
    raw = torch.from_numpy(np.ascontiguousarray(buf[start:])).to(DEV)
    off = v.ctypes.data - (buf.ctypes.data + start)
    dt = {"float32": torch.float32, "int16": torch.int16, "uint16": torch.int16, "uint8": torch.uint8, "float64": torch.float64}[str(v.dtype)]
    es = v.dtype.itemsize
    n = (raw.numel() - off) // es * es
    t = torch.as_strided(raw[off:off + n].view(dt), v.shape, (v.strides[0] // es, 1))
    assert t.data_ptr() % 16 == v.ctypes.data % 16
    return t


def _tiny():
    rng = np.random.default_rng(3)
    pos = rng.standard_normal((5, 3)).astype(F32)
    nrm = pos / np.linalg.norm(pos, axis=1, keepdims=True)
    return synth.Mesh(pos, np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4]], dtype=np.uint32), nrm, rng.integers(0, 256, (5, 4)).astype(np.uint8),
                      rng.random((5, 2)).astype(F32))


def test_round_trip_from_interleaved_buffers(ctx):
    """encode -> decode into interleaved int16 / uint16 buffers -> encode_batch_layout on those buffers as they are -> decode again"""
    meshes = [_tiny(), synth.bumpy_sphere(5, 2, seed=1), synth.bumpy_sphere(9, 6, seed=2), synth.holey_disc(14, seed=3, color_components=4),
              synth.bumpy_sphere(31, 17, seed=4), synth.torus(24, 12, seed=5), synth.bumpy_sphere(40, 30, seed=6), synth.bumpy_sphere(64, 32, seed=7)]
    assert min(m.nvert for m in meshes) == 5 and max(m.nvert for m in meshes) == 2112 and len(meshes) == 8
    blobs = [ca.aligned_blob(ca.encode(m, normal_prediction=i % 3)) for i, m in enumerate(meshes)]
    # the second encode's parameters: every recipe of the position step, every normal prediction
    kws = [dict(normal_prediction=i % 3, **[dict(position_bits=12), dict(position_bits=0, position_q=0.0), dict(position_bits=0, position_q=0.004)][(i // 2) % 3])
           for i in range(8)]
    b = ca.Batch(ctx, blobs)
    b.allocate_interleaved(ca.FMT_INT16, index16=True)
    b.decode(); b.sync()
    views, layouts = zip(*b.interleaved_meshes())
    assert all(l.flags == 3 and l.position_stride == 32 for l in layouts)
    expect, ymeshes = [], []
    for i in range(8):
        h = b.host_outputs(i)
        y = synth.Mesh(h["position"], h["index"].astype(np.uint32), h["normal"].astype(F32) / F32(32767), h["color"], h["uv"])
        ymeshes.append(y)
        expect.append(ca.encode(y, **kws[i]).tobytes())
    ref = ca.Batch(ctx, [ca.aligned_blob(np.frombuffer(e, dtype=np.uint8)) for e in expect])
    ref.allocate_outputs(); ref.decode(); ref.sync()
    for mode in MODES:
        ctx.set_encode_topology(mode)
        out, offs, lens, st = ca.encode_batch_layout(views, ctx, layouts, kw=kws, device_out=True, with_stats=True)
        _check_arena(out, offs, lens, expect, st["total"], ("device out", mode))
        assert st["kernel_times"]["enc_splice"]["launches"] == 1 and st["kernel_times"]["enc_input_check"]["launches"] == 1
        hout, hoffs, hlens, hst = ca.encode_batch_layout(views, ctx, layouts, kw=kws, device_out=False, with_stats=True)
        _check_arena(hout, hoffs, hlens, expect, hst["total"], ("host out", mode))
        assert "enc_splice" not in hst["kernel_times"]
        again = ca.Batch.resident(ctx, out, offs, lens)
        again.allocate_outputs(); again.decode(); again.sync()
        for i in range(8):
            got, want = again.host_outputs(i), ref.host_outputs(i)
            for k in ("position", "normal", "color", "uv", "index"):
                assert got[k].tobytes() == want[k].tobytes(), (mode, i, k)
        again.close()
    ctx.set_encode_topology("host")
    ref.close(); b.close()


def test_alignment_and_strides_on_the_device(ctx):
    """tests/test_encode_layout_cpu.py's sweep as device tensors in one batch: position strides x base offsets x vertex counts (clouds: the box
    of input - o; the box from vertex 0), uint16 index arrays at every 2-byte offset x entry counts (meshes: range check, first edges)"""
    big = synth.bumpy_sphere(70, 40, seed=21)
    views, layouts, kws, expect = [], [], [], []

    def add(y, v, lay, kw):
        views.append(v); layouts.append(lay); kws.append(kw); expect.append(ca.encode(y, **kw).tobytes())
    for nvert in NVERTS:
        for stride in STRIDES:
            for base in BASES:
                p = big.position[:nvert].copy()
                kw = dict(position_bits=0, position_q=0.0) if (stride + base) % 8 else dict(position_bits=9)
                origin = ORIGIN if kw["position_bits"] == 0 else (0.0, 0.0, 0.0)
                add(synth.Mesh((p - np.array(origin, dtype=F32)).astype(F32)), ca.MeshView(dev_view(strided(p, stride, base))),
                    ca.MeshLayout(position_stride=stride, origin=origin), kw)
    nvert = 2049
    pos = big.position[:nvert].copy()
    for k, entries in enumerate((3, 6, 9, 21, 24, 27, 4095, 4098, 8190)):
        idx = (big.index[:entries // 3] % np.uint32(nvert)).astype(np.uint32)
        for off in range(0, 16, 2):
            stride, pbase = ((12, 0), (20, 4), (32, 0), (16, 0))[(k + off // 2) % 4]
            i16 = strided(idx.astype(np.uint16).reshape(1, -1), None, off).reshape(-1, 3)
            add(synth.Mesh(pos, idx), ca.MeshView(dev_view(strided(pos, stride, pbase)), dev_view(i16)),
                ca.MeshLayout(index16=True, position_stride=stride), dict(position_bits=0, position_q=0.0) if off % 4 else dict(position_bits=11))
    assert len(views) == len(NVERTS) * len(STRIDES) * len(BASES) + 72
    for mode in ("host", "device"):
        ctx.set_encode_topology(mode)
        out, offs, lens, st = ca.encode_batch_layout(views, ctx, layouts, kw=kws, device_out=(mode == "device"), with_stats=True)
        _check_arena(out, offs, lens, expect, st["total"], mode)
    ctx.set_encode_topology("host")


def _record_mesh(m, rng):
    """m's data in ONE structured record array (position f32x3 | normal i16x3 + pad | uv f32x2 | colour) and a uint16 index: numpy views"""
    cc = m.color.shape[1]
    rec = np.dtype([("position", F32, 3), ("normal", np.int16, 3), ("pad", np.int16), ("uv", F32, 2), ("color", np.uint8, cc), ("tail", np.uint8, 4 - cc + 4)])
    a = np.zeros(m.nvert, dtype=rec)
    a["position"], a["normal"], a["uv"], a["color"] = m.position, n16_of(m.normal), m.uv, m.color
    v = ca.MeshView(a["position"], m.index.astype(np.uint16), a["normal"], a["color"], a["uv"], groups=m.groups)
    y = synth.Mesh(m.position, m.index, a["normal"].astype(F32) / F32(32767), m.color, m.uv, groups=m.groups)
    return v, y


def test_host_arrays_through_one_record_array(ctx):
    rng = np.random.default_rng(4)
    ms = [synth.bumpy_sphere(12, 7, seed=1, color_components=3), synth.bumpy_sphere(33, 20, seed=2), synth.holey_disc(15, seed=3), synth.torus(20, 9, seed=4)]
    ms[1].groups = [100, ms[1].nface]
    pairs = [_record_mesh(m, rng) for m in ms]
    cloud = synth.point_cloud(17, 9, seed=5)
    pairs.append((ca.MeshView(strided(cloud.position, 28, 4), None, strided(cloud.normal, 12, 8), cloud.color, cloud.uv), cloud))
    kws = [dict(normal_prediction=i % 3, position_bits=0, position_q=[0.0, 0.002][i % 2]) for i in range(len(pairs))]
    attrs = rng.standard_normal((ms[0].nvert, 2))
    kws[0] = dict(kws[0], attributes=[("weight", strided(attrs, 24, 8), 0.01, 0)])
    expect = [ca.encode(y, **dict(k, attributes=[("weight", attrs, 0.01, 0)]) if "attributes" in k else k).tobytes() for (_, y), k in zip(pairs, kws)]
    views = [v for v, _ in pairs]
    assert all(l.position_stride == 36 and l.flags == 3 for l in map(ca.MeshLayout.of, views[:4]))      # read off the views
    for mode in MODES:
        ctx.set_encode_topology(mode)
        for device_out in (False, True):
            out, offs, lens, st = ca.encode_batch_layout(views, ctx, kw=kws, resident=False, device_out=device_out, with_stats=True)
            _check_arena(out, offs, lens, expect, st["total"], (mode, device_out))
    ctx.set_encode_topology("host")


def test_index_limit_65536_vertices_with_a_uint16_index(ctx):
    s = synth.bumpy_sphere(12, 6, seed=7)
    pos = np.zeros((65536, 3), dtype=F32)
    pos[65536 - s.nvert:] = s.position
    idx = s.index + np.uint32(65536 - s.nvert)
    assert idx.max() == 65535
    y = synth.Mesh(pos, idx)
    kw = dict(position_bits=0, position_q=0.001)
    expect = [ca.encode(y, **kw).tobytes()]
    v = ca.MeshView(torch.from_numpy(pos).to(DEV), torch.from_numpy(idx.astype(np.uint16).view(np.int16)).to(DEV))
    for mode in MODES:
        ctx.set_encode_topology(mode)
        out, offs, lens, st = ca.encode_batch_layout([v], ctx, kw=kw, device_out=True, with_stats=True)
        _check_arena(out, offs, lens, expect, st["total"], mode)
    ctx.set_encode_topology("host")


def test_origin_cloud_box_and_mesh_with_explicit_q(ctx):
    origin = (12.5, -3.0, 0.75)
    o = np.array(origin, dtype=F32)
    cloud = synth.point_cloud(40, 30, seed=8)
    cloud.position = (cloud.position + o).astype(F32)
    mesh = synth.bumpy_sphere(30, 20, seed=9)
    mesh.position = (mesh.position + o).astype(F32)
    kws = [dict(position_bits=0, position_q=0.0), dict(position_bits=0, position_q=0.003)]          # the box recipe on input - o; an explicit q
    assert ca.encode_input_model(cloud, 0, layout=ca.MeshLayout(origin=origin), **kws[0])["recipe"] == 3
    expect = [ca.encode(synth.Mesh((m.position - o).astype(F32), m.index, m.normal, m.color, m.uv), **k).tobytes() for m, k in zip((cloud, mesh), kws)]
    views = [ca.mesh_to_device(cloud), ca.mesh_to_device(mesh)]
    layouts = [ca.MeshLayout(origin=origin), ca.MeshLayout(origin=origin)]
    for mode in MODES:
        ctx.set_encode_topology(mode)
        out, offs, lens, st = ca.encode_batch_layout(views, ctx, layouts, kw=kws, device_out=True, with_stats=True)
        _check_arena(out, offs, lens, expect, st["total"], mode)
    ctx.set_encode_topology("host")
    hout, hoffs, hlens = ca.encode_batch_layout([cloud, mesh], ctx, layouts, kw=kws, resident=False)
    _check_arena(hout, hoffs, hlens, expect, int(ca.arena_layout(hlens)[1]), "host arrays")


def _three(bad_value=None):
    ms = [synth.bumpy_sphere(14, 9, seed=11), synth.bumpy_sphere(20, 13, seed=12), synth.holey_disc(13, seed=13)]
    kw = dict(position_bits=0, position_q=0.0)
    expect = [ca.encode(m, **kw).tobytes() for m in ms]
    idx = [m.index.astype(np.uint16) for m in ms]
    if bad_value is not None:
        idx[1][ms[1].nface // 2, 2] = bad_value
    views = [ca.MeshView(torch.from_numpy(m.position).to(DEV), torch.from_numpy(i.view(np.int16)).to(DEV), torch.from_numpy(m.normal).to(DEV),
                         torch.from_numpy(m.color).to(DEV), torch.from_numpy(m.uv).to(DEV)) for m, i in zip(ms, idx)]
    return ms, views, kw, expect


def test_out_of_range_uint16_entry_fails_its_mesh_alone(ctx):
    ms, views, kw, expect = _three()
    for mode in MODES:
        ctx.set_encode_topology(mode)
        clean = ca.encode_batch_layout(views, ctx, kw=kw, device_out=False)
        _check_arena(*clean, expect, int(ca.arena_layout(clean[2])[1]), mode)
        for value in (ms[1].nvert, 0xFFFF):
            _, bad_views, _, _ = _three(value)
            out, offs, lens, status = ca.encode_batch_layout(bad_views, ctx, kw=kw, device_out=False, raise_on_error=False)
            assert status.tolist() == [0, E_ARGUMENT, 0] and lens[1] == 0, (mode, value)
            for i in (0, 2):
                assert out[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes() == expect[i], (mode, value, i)
    ctx.set_encode_topology("host")


def test_strided_extent_outside_its_allocation_is_refused(ctx):
    """The last vertex of a strided position array ends four bytes behind the allocation it lies in (the segment torch's allocator got from
    the runtime, found in its snapshot): CRTHIP_E_ARGUMENT from the pointer queries, nothing launched on that mesh, the neighbour encoded."""
    raw = torch.zeros(12 << 20, dtype=torch.uint8, device=DEV)
    seg = [s for s in torch.cuda.memory_snapshot() if s["address"] <= raw.data_ptr() < s["address"] + s["total_size"]]
    assert len(seg) == 1
    end = seg[0]["address"] + seg[0]["total_size"]                   # the allocation's end, wherever the tensor lies in it
    assert raw.data_ptr() + raw.numel() <= end
    nvert, stride = 8, 16
    extent = (nvert - 1) * stride + 12

    class At:                                                        # (n, 3) float32 at a byte address inside raw
        def __init__(self, address):
            self.address, self.shape, self.device, self.dtype = address, (nvert, 3), raw.device, torch.float32

        def numel(self):
            return nvert * 3

        def data_ptr(self):
            return self.address

        def stride(self, k):
            return stride // 4

        def element_size(self):
            return 4
    good = synth.point_cloud(9, 5, seed=14)
    kw = dict(position_bits=0, position_q=0.01, with_normal=False, with_color=False, with_uv=False)
    neighbour = ca.mesh_to_device(good)
    want = ca.encode(good, **kw).tobytes()
    inside = ca.MeshView(At(end - extent))                           # ends with the allocation: taken
    out, offs, lens, status = ca.encode_batch_layout([inside, neighbour], ctx, kw=kw, device_out=False, raise_on_error=False)
    assert status.tolist() == [0, 0] and lens[0] > 0
    assert out[int(offs[1]):int(offs[1]) + int(lens[1])].tobytes() == want
    outside = ca.MeshView(At(end - extent + 4))
    out, offs, lens, status = ca.encode_batch_layout([outside, neighbour], ctx, kw=kw, device_out=False, raise_on_error=False)
    assert status.tolist() == [E_ARGUMENT, 0] and lens[0] == 0
    assert out[int(offs[1]):int(offs[1]) + int(lens[1])].tobytes() == want
    del raw
