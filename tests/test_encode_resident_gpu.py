"""GPU (-m gpu): crthip_encode_batch_resident - a batch whose meshes live in device memory.  Every blob byte-identical to the host
encoder's (crthip_encode) of the same arrays in host memory and, for the golden cases, to the reference's own bytes; under the three
topology modes; the three recipes of the position step over many workgroups; per-mesh errors; what goes over the link.

What is NOT handed over here, on purpose: pageable host memory, and an extent that leaves its allocation.  Were the pointer check ever
missing, such a test would turn into a device fault on a machine others share.  The extent rule (hipMemGetAddressRange in
encode_batch.cpp: resident_array_ok) is therefore covered by review and not by a GPU test; alignment and pinned host memory, which cannot
fault, are tested.

One context; every input seeded.  Run as one pytest invocation under a time limit of its own."""
import sys

import numpy as np
import pytest
import torch

import corto_amd as ca
from corto_amd import synth
from conftest import GOLDEN, aligned, load_golden
from test_encode_batch_gpu import _corpus

pytestmark = pytest.mark.gpu

E_ARGUMENT = -8
MODES = ("host", "device", "split")


@pytest.fixture(scope="module")
def ctx():
    c = ca.Context(0)
    yield c
    c.set_encode_topology("host")
    c.close()


def _cases():
    sys.path.insert(0, GOLDEN)
    from cases import cases
    return cases()


def _dev(items):
    """(device meshes, keyword dicts with device attributes) of [(mesh, kw), ...]"""
    ms, ks = [], []
    for m, k in items:
        k = dict(k)
        if k.get("attributes") is not None:
            k["attributes"] = ca.attributes_to_device(k["attributes"])
        ms.append(ca.mesh_to_device(m)); ks.append(k)
    return ms, ks


def _resident(ctx, items, **kw):
    ms, ks = _dev(items)
    return ca.encode_batch_resident(ms, ctx, kw=ks, **kw)


def _raw_bytes(items):
    n = 0
    for m, k in items:
        for a, on in (("position", True), ("index", True), ("normal", k.get("with_normal", True)), ("color", k.get("with_color", True)),
                      ("uv", k.get("with_uv", True)), ("radius", True)):
            v = getattr(m, a)
            if on and v is not None:
                n += v.nbytes
        for _, v, _, _ in k.get("attributes") or ():
            n += np.asarray(v).nbytes
    return n


def test_golden_cases_resident(ctx):
    cs = _cases()
    for mode in MODES:
        ctx.set_encode_topology(mode)
        blobs = _resident(ctx, [(m, k) for _, m, k in cs])
        for (name, _, _), b in zip(cs, blobs):
            assert b.tobytes() == load_golden(name)["crt"].tobytes(), (name, mode)
    ctx.set_encode_topology("host")


def _host_encode(m, k):
    if m.nvert == 0:                                               # the host reads position[0] of an empty cloud: give it zeros to read
        backing = np.zeros((4, 3), dtype=np.float32)
        e = synth.Mesh(position=backing[:0])
        e.position = backing[:0]
        for a in ("normal", "color", "uv", "radius"):
            setattr(e, a, getattr(m, a))
        return ca.encode(e, **k)
    return ca.encode(m, **k)


def test_mixed_corpus_in_every_topology_mode(ctx):
    items = _corpus()
    assert len(items) >= 150
    expect = [_host_encode(m, k).tobytes() for m, k in items]
    nmesh = sum(1 for m, _ in items if m.nface)
    for mode in MODES:
        ctx.set_encode_topology(mode)
        blobs, st = _resident(ctx, items, with_stats=True)
        for i, b in enumerate(blobs):
            assert b.tobytes() == expect[i], (mode, i)
        if mode == "device":
            assert st["topology_device"] == nmesh > 0
        if mode == "host":
            assert st["topology_device"] == 0
        assert "enc_input_check" in st["kernel_times"] and "enc_input_reduce" in st["kernel_times"], mode
    ctx.set_encode_topology("host")


def test_generic_attributes_every_format(ctx):
    rng = np.random.default_rng(5)
    items = []
    for s, (dt, ncomp) in enumerate(((np.float32, 1), (np.float64, 3), (np.int32, 16), (np.int16, 5), (np.int8, 2), (np.float32, 16))):
        m = synth.bumpy_sphere(20 + s, 10, seed=40 + s) if s % 2 == 0 else synth.point_cloud(25, 11 + s, seed=40 + s)
        if np.issubdtype(dt, np.floating):
            v = (rng.standard_normal((m.nvert, ncomp)) * 100).astype(dt)
        else:
            info = np.iinfo(dt)
            v = rng.integers(max(info.min, -(1 << 20)), min(info.max, 1 << 20), size=(m.nvert, ncomp)).astype(dt)
        second = (rng.standard_normal((m.nvert, 2)) * 10).astype(np.float64)
        attrs = [("attr_%d" % s, v, 0.25, ca.CORRELATED if s % 3 == 0 else (ca.PARALLEL if s % 3 == 1 else 0)), ("second", second, 0.5, 0)]
        items.append((m, dict(normal_prediction=s % 3, attributes=attrs)))
    for mode in ("host", "device"):
        ctx.set_encode_topology(mode)
        blobs = _resident(ctx, items)
        for (m, k), b in zip(items, blobs):
            assert b.tobytes() == ca.encode(m, **k).tobytes(), mode
    ctx.set_encode_topology("host")


def test_every_step_recipe_over_many_workgroups(ctx):
    mesh = synth.bumpy_sphere(420, 300, seed=3)                   # > 100 K vertices, > 200 K faces
    cloud = synth.point_cloud(400, 300, seed=4)
    assert mesh.nvert >= 100_000 and mesh.nface >= 100_000 and cloud.nvert >= 100_000
    items = []
    for m in (mesh, cloud):
        for k in (dict(position_bits=14), dict(position_bits=0, position_q=0.0), dict(position_bits=0, position_q=0.003)):
            items.append((m, dict(normal_prediction=ca.DIFF, **k)))
    recipes = {ca.encode_input_model(m, 0, **k)["recipe"] for m, k in items}
    assert recipes == {0, 1, 2, 3}
    expect = [ca.encode(m, **k).tobytes() for m, k in items]
    for mode in MODES:                                             # (split: this mesh is beyond LDS, its index comes back for the pool)
        ctx.set_encode_topology(mode)
        blobs, st = _resident(ctx, items, with_stats=True)
        for (m, k), b, e in zip(items, blobs, expect):
            assert b.tobytes() == e, (mode, k)
        print("input pass, %s topology: %s" % (mode, {n: st["kernel_times"][n] for n in ("enc_input_check", "enc_input_reduce")}))
    ctx.set_encode_topology("host")


def test_large_and_tied_clouds(ctx):
    big = synth.point_cloud(1500, 1400, seed=11)
    assert big.nvert >= 2_000_000
    kw = dict(normal_prediction=ca.DIFF, position_bits=20)
    blobs, st = _resident(ctx, [(big, kw)], with_stats=True)
    assert st["clouds_device_sorted"] == 1 and st["clouds_host_sorted"] == 0
    assert blobs[0].tobytes() == ca.encode(big, **kw).tobytes()
    dup = synth.point_cloud(40, 20, seed=12)
    dup.position[1::5] = dup.position[0::5][:len(dup.position[1::5])]
    blobs, st = _resident(ctx, [(dup, dict(normal_prediction=ca.BORDER))], with_stats=True)
    assert st["clouds_host_sorted"] == 1 and blobs[0].tobytes() == ca.encode(dup, normal_prediction=ca.BORDER).tobytes()
    wide = synth.point_cloud(40, 20, seed=13)
    kw = dict(normal_prediction=ca.DIFF, position_bits=0, position_q=1.0)
    wide.position = np.ascontiguousarray((wide.position * np.float32(2 ** 24)).astype(np.float32))
    wide.position[3] = wide.position[2] + np.float32(2 ** 22)
    blobs, st = _resident(ctx, [(wide, kw)], with_stats=True)
    assert st["clouds_host_sorted"] == 1 and blobs[0].tobytes() == ca.encode(wide, **kw).tobytes()


def _carve(items, seed):
    """Every array of the items in ONE device tensor, each at an element-aligned but otherwise odd offset (4 mod 16 for the 4-byte
    types, 8 mod 16 for doubles, 2 mod 4 for int16, odd for bytes).  Returns (buffer, device meshes, keyword dicts)."""
    rng = np.random.default_rng(seed)
    places, pos = [], 0

    def place(a):
        nonlocal pos
        a = np.ascontiguousarray(a)
        es = a.dtype.itemsize
        want = {1: 1, 2: 2, 4: 4, 8: 8}[es] % 16
        pos += 16 * int(rng.integers(1, 4))
        pos = (pos + 15) // 16 * 16 + want
        places.append((pos, a))
        at = pos
        pos += a.nbytes
        return at

    plan = []
    for m, k in items:
        d = {a: (None if getattr(m, a) is None else place(getattr(m, a))) for a in ("position", "index", "normal", "color", "uv", "radius")}
        attrs = [(name, place(v), q, s) for name, v, q, s in (k.get("attributes") or ())]
        plan.append((d, attrs))
    host = np.zeros(pos + 64, dtype=np.uint8)
    for at, a in places:
        host[at:at + a.nbytes] = a.view(np.uint8).reshape(-1)
    buf = torch.from_numpy(host).to("cuda:0")
    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.uint32): torch.int32, np.dtype(np.int32): torch.int32,
           np.dtype(np.int16): torch.int16, np.dtype(np.int8): torch.int8, np.dtype(np.uint8): torch.uint8}

    def view(at, a):
        a = np.ascontiguousarray(a)
        return buf[at:at + a.nbytes].view(tdt[a.dtype]).reshape(a.shape)

    ms, ks = [], []
    for (m, k), (d, attrs) in zip(items, plan):
        ms.append(ca.DeviceMesh(**{a: (None if at is None else view(at, getattr(m, a))) for a, at in d.items()}, groups=m.groups,
                                group_props=getattr(m, "group_props", None)))
        k = dict(k)
        if attrs:
            k["attributes"] = [(name, view(at, v0[1]), q, s) for (name, at, q, s), v0 in zip(attrs, k["attributes"])]
        ks.append(k)
    return buf, ms, ks


def test_one_shared_buffer_at_odd_offsets(ctx):
    rng = np.random.default_rng(9)
    items = [(m, k) for _, m, k in _cases()[:8]] + [(m, k) for _, m, k in _cases()[-2:]]
    big = synth.bumpy_sphere(90, 50, seed=8)
    items.append((big, dict(normal_prediction=ca.ESTIMATED, position_bits=0, position_q=0.0)))
    g = synth.bumpy_sphere(30, 12, seed=2)
    items.append((g, dict(attributes=[("d", rng.standard_normal((g.nvert, 2)), 0.01, 0), ("h", rng.integers(-900, 900, (g.nvert, 3)).astype(np.int16), 1.0, 0),
                                       ("b", rng.integers(-90, 90, (g.nvert, 1)).astype(np.int8), 1.0, 0)])))
    buf, ms, ks = _carve(items, seed=1)
    assert ms[0].position.data_ptr() % 16 == 4
    before = buf.clone()
    for mode in ("host", "device"):
        ctx.set_encode_topology(mode)
        blobs = ca.encode_batch_resident(ms, ctx, kw=ks)
        for (m, k), b in zip(items, blobs):
            assert b.tobytes() == ca.encode(m, **k).tobytes(), mode
        assert torch.equal(buf, before)
    ctx.set_encode_topology("host")


def test_errors_are_codes_and_leave_the_neighbours_alone(ctx):
    a, b, c = synth.bumpy_sphere(16, 8, seed=1), synth.bumpy_sphere(16, 8, seed=2), synth.bumpy_sphere(16, 8, seed=3)
    b.index = b.index.copy(); b.index[5, 1] = b.nvert + 3
    kw = dict(normal_prediction=ca.BORDER)
    for mode in MODES:
        ctx.set_encode_topology(mode)
        blobs, status = _resident(ctx, [(a, kw), (b, kw), (c, kw)], raise_on_error=False)
        assert status.tolist() == [0, E_ARGUMENT, 0], mode
        assert len(blobs[1]) == 0
        assert blobs[0].tobytes() == ca.encode(a, **kw).tobytes() and blobs[2].tobytes() == ca.encode(c, **kw).tobytes()
    ctx.set_encode_topology("host")
    # a pointer off its element alignment
    ms, ks = _dev([(a, kw), (c, kw)])
    raw = torch.zeros(a.position.nbytes + 16, dtype=torch.uint8, device="cuda:0")
    raw[2:2 + a.position.nbytes] = torch.from_numpy(a.position.view(np.uint8).reshape(-1)).to("cuda:0")
    ms[0].position = _Unaligned(raw, 2, a.position.shape)
    blobs, status = ca.encode_batch_resident(ms, ctx, kw=ks, raise_on_error=False)
    assert status.tolist() == [E_ARGUMENT, 0] and blobs[1].tobytes() == ca.encode(c, **kw).tobytes()
    # pinned host memory: host arrays belong to encode_batch
    ms, ks = _dev([(a, kw), (c, kw)])
    ms[1].position = torch.from_numpy(c.position).pin_memory()
    blobs, status = ca.encode_batch_resident(ms, ctx, kw=ks, raise_on_error=False)
    assert status.tolist() == [0, E_ARGUMENT] and blobs[0].tobytes() == ca.encode(a, **kw).tobytes()
    with pytest.raises(ca.CortoError):
        ca.encode_batch_resident(ms, ctx, kw=ks)


class _Unaligned:
    """float32 (n, 3) data at a byte offset of a device byte tensor that torch would refuse to view as float32: shape, device and data_ptr
    are all encode_batch_resident asks of an array"""

    def __init__(self, raw, offset, shape):
        self.raw, self.offset, self.shape = raw, offset, tuple(shape)
        self.device = raw.device

    def numel(self):
        return int(np.prod(self.shape))

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self.raw.data_ptr() + self.offset


def test_traffic_and_kernel_names(ctx):
    items = [(synth.bumpy_sphere(64, 32, seed=s), dict(normal_prediction=s % 3)) for s in range(24)]
    items += [(synth.point_cloud(60, 40, seed=s), dict(normal_prediction=ca.DIFF)) for s in range(4)]
    ctx.set_encode_topology("device")
    hb, hs = ca.encode_batch([m for m, _ in items], ctx, kw=[k for _, k in items], with_stats=True)
    rb, rs = _resident(ctx, items, with_stats=True)
    ctx.set_encode_topology("host")
    assert [b.tobytes() for b in hb] == [b.tobytes() for b in rb]
    raw = _raw_bytes(items)
    print("bytes_to_device: host arrays %d, resident %d, raw attribute and index bytes %d" % (hs["bytes_to_device"], rs["bytes_to_device"], raw))
    assert rs["bytes_to_device"] <= hs["bytes_to_device"] - raw
    assert "enc_input_check" in rs["kernel_times"] and rs["kernel_times"]["enc_input_check"]["launches"] == 1
    assert "enc_input_check" not in hs["kernel_times"] and "enc_input_reduce" not in hs["kernel_times"]


def test_round_trip_through_a_resident_decode(ctx):
    from oracle import oracle as oc
    cs = _cases()
    items = [(m, k) for name, m, k in cs if name in ("nrm_diff", "c4_unit", "two_groups", "torus", "icosphere", "cloud_diff")]
    blobs = _resident(ctx, items)
    offs, total = ca.arena_layout([len(b) for b in blobs])
    host = np.zeros(int(total) + 16, dtype=np.uint8)
    for b, o in zip(blobs, offs):
        host[int(o):int(o) + len(b)] = b
    buf = torch.from_numpy(host).to("cuda:0")
    torch.cuda.synchronize()
    batch = ca.Batch.resident(ctx, buf, offs, [len(b) for b in blobs])
    batch.allocate_outputs(fill=0)
    batch.decode()
    assert (batch.sync() == 0).all()
    for i, ((m, k), b) in enumerate(zip(items, blobs)):
        o = oc.decode(aligned(b), color_components=4 if m.color is None else m.color.shape[1])
        got = batch.host_outputs(i)
        for key in ("position", "normal", "color", "uv", "index"):
            if key in o:
                assert key in got and got[key].tobytes() == o[key].tobytes(), (i, key)
    batch.close()


def test_size_query_then_two_runs(ctx):
    import ctypes as C
    items = [(synth.bumpy_sphere(20, 10, seed=s), {}) for s in range(6)] + [(synth.point_cloud(20, 10, seed=1), {})]
    ms, _ = _dev(items)
    descs = (ca.MeshDesc * len(ms))()
    keep = []
    for i, m in enumerate(ms):
        descs[i], kp = ca._mesh_desc(m, ptr=lambda t: t.data_ptr())
        keep.append(kp)
    n = len(ms)
    L = ca.lib()

    def call(out, cap):
        offs = np.zeros(n + 1, dtype=np.uint64)
        r = L.crthip_encode_batch_resident(ctx.handle, n, descs, None, 0, None if out is None else ca._np_ptr(out), cap, ca._np_ptr(offs),
                                           None, None, None, None, None)
        return int(r), offs

    size, offs0 = call(None, 0)
    assert size > 0 and int(offs0[n]) == size
    runs = []
    for _ in range(2):
        out = np.zeros(size, dtype=np.uint8)
        r, offs = call(out, size)
        assert r == size and offs.tolist() == offs0.tolist()
        runs.append(out.tobytes())
    assert runs[0] == runs[1]
    for i, (m, _) in enumerate(items):
        assert runs[0][int(offs0[i]):int(offs0[i + 1])] == ca.encode(m).tobytes()
