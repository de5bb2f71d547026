"""crthip_mesh_layout without a device: crthip_encode_layout against the packed encoder, the layout variants of the input and topology
models (the kernels' source in the kernels' partition against the host loops, bit for bit), and every refusal.

The yardstick is crthip_encode_attrs (ca.encode), which is pinned to the reference byte for byte, run on arrays this file converts itself
in numpy float32.  Parity with upstream rests on upstream's overloads being exactly these single operations:
    uint16 index   Encoder::addPositions(buffer, const uint16_t *, q, o), src/encoder.cpp:114-119: tmp[i] = _index[i]  ->  index.astype(uint32)
    int16 normals  Encoder::addNormals(const int16_t *, bits, prediction), src/encoder.cpp:151-158: buffer[i*3 + k]/32767.0f
                                                                                              ->  n.astype(float32) / float32(32767)
    origin         Encoder::addPositions(buffer, q, o), src/encoder.cpp:77-81: coords[i] = input[i] - o  ->  pos - origin
                   (a cloud's q == 0 recipe runs on coords, :83-91; a mesh's on the raw buffer, :101-111, before the subtraction)
Strides have no upstream counterpart: a strided array means the packed array of its elements."""
import ctypes as C

import numpy as np
import pytest

import corto_amd as ca
from corto_amd import synth

E_ARGUMENT = -8
F32 = np.float32


def strided(a, stride=None, base=0, fill=0xA5):
    """a (n, k) array's values in a view whose rows lie `stride` bytes apart and whose first byte is `base` bytes past a 16-byte boundary;
    the buffer ends with the last row: nothing behind the checked extent exists"""
    a = np.ascontiguousarray(a)
    n, row = a.shape[0], a.dtype.itemsize * a.shape[1]
    stride = row if stride is None else stride
    need = (n - 1) * stride + row if n else 0
    buf = np.full(need + 32, fill, dtype=np.uint8)
    off = (-buf.ctypes.data) % 16 + base
    v = np.ndarray(shape=a.shape, dtype=a.dtype, buffer=buf, offset=off, strides=(stride, a.dtype.itemsize))
    v[...] = a
    assert v.ctypes.data % 16 == base % 16
    return v


def n16_of(normal):
    return np.clip(np.rint(normal.astype(np.float64) * 32767.0), -32767, 32767).astype(np.int16)


def forms_of(mesh, forms, rng, attributes=None):
    """(views, layout, attribute views, packed yardstick mesh, yardstick attributes, kw overrides) of `mesh` under the named input forms"""
    pos, idx, nrm, col, uv = mesh.position, mesh.index, mesh.normal, mesh.color, mesh.uv
    y = synth.Mesh(pos.copy(), None if idx is None else idx.copy(), None if nrm is None else nrm.copy(), None if col is None else col.copy(),
                   None if uv is None else uv.copy(), groups=mesh.groups)
    origin = (0.0, 0.0, 0.0)
    if "origin" in forms:
        origin = tuple(float(F32(x)) for x in (0.37, -1.25, 0.0625))
        y.position = (pos - np.array(origin, dtype=F32)).astype(F32)          # one float32 subtraction a component
    if "normal16" in forms and nrm is not None:
        nrm = n16_of(nrm)
        y.normal = nrm.astype(F32) / F32(32767)
    if "index16" in forms and idx is not None:
        idx = idx.astype(np.uint16)
        y.index = idx.astype(np.uint32)
    if "stride" in forms:
        pos = strided(pos, 12 + 4 * int(rng.integers(0, 6)), 4 * int(rng.integers(0, 4)))
        if nrm is not None:
            nrm = strided(nrm, 8 if nrm.dtype == np.int16 else 20, 2 if nrm.dtype == np.int16 else 4)
        if col is not None:
            col = strided(col, col.shape[1] + int(rng.integers(0, 5)), int(rng.integers(0, 16)))
        if uv is not None:
            uv = strided(uv, 8 + 4 * int(rng.integers(0, 4)), 8)
        if idx is not None and idx.dtype == np.uint16:
            idx = strided(idx.reshape(1, -1), None, 2 * int(rng.integers(0, 8))).reshape(-1, 3)
    views = ca.MeshView(pos, idx, nrm, col, uv, groups=mesh.groups)
    av = attributes
    if attributes is not None and "stride" in forms:
        av = [(nm, strided(v, v.dtype.itemsize * (v.shape[1] + 2), 0), q, s) for nm, v, q, s in attributes]
    return views, ca.MeshLayout.of(views, av, origin=origin), av, y


def corpus():
    rng = np.random.default_rng(7)
    out = []
    for s, (pred, cc) in enumerate([(ca.DIFF, 3), (ca.ESTIMATED, 4), (ca.BORDER, 4), (ca.BORDER, 3)]):
        m = synth.bumpy_sphere(int(rng.integers(6, 20)), int(rng.integers(4, 14)), seed=50 + s, color_components=cc)
        if s == 1:
            m.groups = [m.nface // 3, m.nface]                               # two groups
        out.append(("mesh%d" % s, m, dict(normal_prediction=pred, position_bits=0, position_q=float(F32(0.003)))))
        c = synth.point_cloud(int(rng.integers(5, 15)), int(rng.integers(4, 12)), seed=60 + s, color_components=cc)
        out.append(("cloud%d" % s, c, dict(normal_prediction=pred, position_bits=0, position_q=0.0)))       # the box recipe
    out.append(("holey", synth.holey_disc(12, seed=3), dict(normal_prediction=ca.ESTIMATED, position_bits=0, position_q=float(F32(0.01)))))
    return out


FORMS = [("index16",), ("normal16",), ("origin",), ("stride",), ("index16", "normal16", "origin", "stride")]


def test_encode_layout_equals_the_packed_encoder():
    rng = np.random.default_rng(11)
    n = 0
    for name, m, kw in corpus():
        attrs = [("weight", rng.standard_normal((m.nvert, 2)), 0.01, 0)]       # one generic double attribute (strided under "stride")
        for forms in FORMS:
            views, lay, av, y = forms_of(m, forms, rng, attrs)
            want = ca.encode(y, attributes=attrs, **kw)
            got = ca.encode_layout(views, lay, attributes=av, **kw)
            assert got.tobytes() == want.tobytes(), (name, forms)
            n += 1
    assert n == 45
    # position_bits > 0 (no origin): the box from vertex 0 through a stride
    m = synth.bumpy_sphere(9, 7, seed=2)
    views, lay, av, y = forms_of(m, ("index16", "normal16", "stride"), rng)
    assert ca.encode_layout(views, lay, position_bits=12).tobytes() == ca.encode(y, position_bits=12).tobytes()


def test_mesh_first_edge_step_is_taken_from_the_raw_positions():
    # src/encoder.cpp:101-111: q comes from the buffer as given, the origin is subtracted afterwards (:80-81)
    m = synth.bumpy_sphere(11, 6, seed=9)
    origin = (100.0, -50.0, 25.0)
    lay = ca.MeshLayout(origin=origin)
    q = ca.encode_input_model(m, 0, position_bits=0, position_q=0.0)["step"]
    assert ca.encode_input_model(m, 0, layout=lay, position_bits=0, position_q=0.0)["step"].view(np.uint32) == q.view(np.uint32)
    y = synth.Mesh((m.position - np.array(origin, dtype=F32)).astype(F32), m.index, m.normal, m.color, m.uv)
    want = ca.encode(y, position_bits=0, position_q=float(q))
    assert ca.encode_layout(m, lay, position_bits=0, position_q=0.0).tobytes() == want.tobytes()


def test_zero_and_null_layouts_are_the_packed_encoder():
    for name, m, kw in corpus()[:4]:
        want = ca.encode(m, **kw).tobytes()
        assert ca.encode_layout(m, ca.MeshLayout(), **kw).tobytes() == want
        d, keep = ca._mesh_desc(m, **kw)
        out = np.zeros(len(want) + 64, dtype=np.uint8)
        n = ca.lib().crthip_encode_layout(C.byref(d), None, None, ca._np_ptr(out), out.size, None, None)
        assert n == len(want) and out[:n].tobytes() == want
        # packed strides spelt out are the packed arrays too
        lay = ca.MeshLayout(position_stride=12, normal_stride=12, color_stride=m.color.shape[1], uv_stride=8)
        assert ca.encode_layout(m, lay, **kw).tobytes() == want


# ---- the input model: the kernels' source in the kernels' partition (which = 1) against the host loops (which = 0) ----

def _bits(r):
    return (r["index_out_of_range"], r["recipe"], r["mn"].view(np.uint32).tolist(), r["mx"].view(np.uint32).tolist(),
            int(np.array([r["sum"]], dtype=np.float64).view(np.uint64)[0]), int(np.array([r["step"]], dtype=np.float32).view(np.uint32)[0]))


def _parity(views, lay, **kw):
    a, b = ca.encode_input_model(views, 0, layout=lay, **kw), ca.encode_input_model(views, 1, layout=lay, **kw)
    assert _bits(a) == _bits(b), (kw, a, b)
    return a


BOX_FIRST, EDGE, BOX_MAX = dict(position_bits=14), dict(position_bits=0, position_q=0.0), dict(position_bits=0, position_q=0.0)
ORIGIN = (0.5, -2.0, 0.125)
NVERTS = (1, 3, 4, 5, 1023, 1024, 1025, 2049)                                   # the run of 4 and the tile of 1024
STRIDES = (12, 16, 20, 32, 48)
BASES = (0, 4, 8, 12)


def _specials(p, rng):
    """NaN, +-0 and +-inf among the positions, the first vertex and the last included now and then"""
    n = p.shape[0]
    for value in (np.nan, np.inf, -np.inf, 0.0, -0.0):
        p[int(rng.integers(0, n)), int(rng.integers(0, 3))] = F32(value)
    return p


def test_input_model_parity_strided_positions():
    rng = np.random.default_rng(5)
    big = synth.bumpy_sphere(70, 40, seed=21).position
    assert big.shape[0] >= max(NVERTS)
    seen = set()
    for nvert in NVERTS:
        for stride in STRIDES:
            for base in BASES:
                for special in (False, True):
                    p = big[:nvert].copy()
                    if special:
                        p = _specials(p, rng)
                    v = ca.MeshView(strided(p, stride, base))
                    packed = synth.Mesh(p)
                    # a cloud's box on input - o, and the box from vertex 0 (no origin)
                    r = _parity(v, ca.MeshLayout(position_stride=stride, origin=ORIGIN), **BOX_MAX)
                    want = ca.encode_input_model(synth.Mesh((p - np.array(ORIGIN, dtype=F32)).astype(F32)), 0, **BOX_MAX)
                    assert _bits(r) == _bits(want), (nvert, stride, base)
                    r = _parity(v, ca.MeshLayout(position_stride=stride), **BOX_FIRST)
                    assert _bits(r) == _bits(ca.encode_input_model(packed, 0, **BOX_FIRST)), (nvert, stride, base)
                    seen.add((nvert, stride, base))
    assert len(seen) == len(NVERTS) * len(STRIDES) * len(BASES)


def _index16_at(idx, byte_offset):
    return strided(idx.astype(np.uint16).reshape(1, -1), None, byte_offset).reshape(-1, 3)


def test_input_model_parity_uint16_index():
    rng = np.random.default_rng(6)
    base = synth.bumpy_sphere(70, 40, seed=22)
    nvert = 2049
    pos = base.position[:nvert].copy()
    for entries in (3, 6, 9, 21, 24, 27, 4095, 4098, 8190):                     # the eight-entry group and the 4096-entry tile
        nface = entries // 3
        idx = (base.index[:nface] % np.uint32(nvert)).astype(np.uint32)
        wide = synth.Mesh(pos, idx)
        for off in range(0, 16, 2):
            for stride, pbase in ((12, 0), (20, 4), (32, 0)):
                v = ca.MeshView(strided(pos, stride, pbase), _index16_at(idx, off))
                lay = ca.MeshLayout(index16=True, position_stride=stride, origin=ORIGIN)
                for kw in (EDGE, BOX_FIRST):
                    if kw is BOX_FIRST:
                        lay = ca.MeshLayout(index16=True, position_stride=stride)
                    r = _parity(v, lay, **kw)
                    assert r["index_out_of_range"] == 0
                    assert _bits(r) == _bits(ca.encode_input_model(wide, 0, **kw)), (entries, off, stride)   # the edge sum: raw positions
            # one entry >= nvert in turn in the head, in a wide group, in the tail, and as a face's first-edge vertex
            head = (16 - off) % 16 // 2
            groups = (entries - min(head, entries)) // 8
            spots = {"first_edge": 1 if entries > 1 else 0, "last": entries - 1}
            if head and head <= entries:
                spots["head"] = head - 1
            if groups:
                spots["group"] = min(head + 8 * (groups // 2) + 5, entries - 1)
            if entries - head - 8 * groups > 0 and entries > head:
                spots["tail"] = head + 8 * groups
            for where, at in spots.items():
                for value in (nvert, 0xFFFF):
                    bad = idx.copy().reshape(-1)
                    bad[at] = value
                    v = ca.MeshView(strided(pos, 16, 0), _index16_at(bad.reshape(-1, 3), off))
                    for kw in (EDGE, BOX_FIRST):
                        r = _parity(v, ca.MeshLayout(index16=True, position_stride=16), **kw)
                        assert r["index_out_of_range"] == 1 and r["sum"] == 0 and r["step"] == 0, (entries, off, where)


def test_input_model_parity_edge_tile_and_special_positions():
    rng = np.random.default_rng(8)
    base = synth.bumpy_sphere(70, 40, seed=23)
    nvert = 1500
    for nface in (1023, 1024, 1025):                                             # the 1024-term edge tile
        idx = (base.index[:nface] % np.uint32(nvert)).astype(np.uint32)
        for special in (False, True):
            p = base.position[:nvert].copy()
            if special:
                p = _specials(p, rng)
                p[idx[0, 0]] = F32(np.nan) if nface == 1024 else p[idx[0, 0]]
            for stride, pbase, off in ((12, 4, 0), (16, 0, 6), (48, 8, 14)):
                v = ca.MeshView(strided(p, stride, pbase), _index16_at(idx, off))
                r = _parity(v, ca.MeshLayout(index16=True, position_stride=stride, origin=ORIGIN), **EDGE)
                assert r["recipe"] == 2
                assert _bits(r) == _bits(ca.encode_input_model(synth.Mesh(p, idx), 0, **EDGE)), (nface, special, stride)


# ---- the topology model: a uint16 index through the device source ----

def _topo_equal(a, b):
    for k in ("faces", "group_end", "quads", "clers", "split_words"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("nvert", "nface", "max_front", "split_bits", "lds"):
        assert a[k] == b[k], k


def test_topology_model_uint16_index_equals_uint32():
    picks = [synth.bumpy_sphere(20, 11, seed=4), synth.non_manifold(synth.bumpy_sphere(16, 9, seed=5), seed=2), synth.confetti(30, seed=3)]
    grouped = synth.bumpy_sphere(14, 8, seed=6)
    grouped.groups = [grouped.nface // 2, grouped.nface]
    picks.append(grouped)
    # nvert = 65536 with entry 65535 in use: the widest index a uint16 array can hold
    s = synth.bumpy_sphere(12, 6, seed=7)
    pos = np.zeros((65536, 3), dtype=F32)
    pos[65536 - s.nvert:] = s.position
    picks.append(synth.Mesh(pos, s.index + np.uint32(65536 - s.nvert)))
    assert picks[-1].index.max() == 65535
    for m in picks:
        assert m.nvert <= 65536
        v = ca.MeshView(m.position, _index16_at(m.index, 6), groups=m.groups)
        lay = ca.MeshLayout(index16=True)
        wide0, wide1 = ca.encode_topology_model(m, 0), ca.encode_topology_model(m, 1)
        for which in (0, 1):
            _topo_equal(ca.encode_topology_model(v, which, layout=lay), wide1 if which else wide0)
        for k in ("faces", "quads", "clers", "split_words"):
            assert wide0[k].tobytes() == wide1[k].tobytes(), k


# ---- refusals: the code comes back and nothing is written ----

def _refused(mesh, lay, attributes=None, model=True, **kw):
    d, keep = ca._mesh_desc(mesh, ptr=ca._view_ptr, **kw)
    lst, keep2 = ca._attr_list(attributes, mesh.nvert, as_views=True)
    out = np.full(1 << 16, 0x5A, dtype=np.uint8)
    nv = np.full(2, 0x77777777, dtype=np.uint32)
    n = ca.lib().crthip_encode_layout(C.byref(d), C.byref(lst) if lst is not None else None, C.byref(lay), ca._np_ptr(out), out.size,
                                      ca._np_ptr(nv), ca._np_ptr(nv[1:]))
    assert (out == 0x5A).all() and (nv == 0x77777777).all()
    if model:                                                                   # the models refuse what the encoder refuses
        r = ca.EncodeInputResult()
        before = bytes(r)
        assert ca.lib().crthip_encode_input_model_layout(C.byref(d), C.byref(lay), 1, C.byref(r)) == n and bytes(r) == before
    return int(n)


def test_refusals():
    m = synth.bumpy_sphere(8, 5, seed=1)
    q = dict(position_bits=0, position_q=0.01)
    assert _refused(m, ca.MeshLayout(flags=4), **q) == E_ARGUMENT
    assert _refused(m, ca.MeshLayout(flags=0x80000001), **q) == E_ARGUMENT
    for bad in (np.nan, np.inf, -np.inf):
        assert _refused(m, ca.MeshLayout(origin=(0.0, bad, 0.0)), **q) == E_ARGUMENT
    assert _refused(m, ca.MeshLayout(origin=(0.0, 1.0, 0.0)), position_bits=14) == E_ARGUMENT       # addPositionsBits has no origin
    assert len(ca.encode_layout(m, ca.MeshLayout(origin=(-0.0, 0.0, 0.0)), position_bits=14)) > 0    # a zero origin is none
    for field, values in (("position_stride", (8, 11, 14, 18)), ("normal_stride", (8, 10, 13)), ("uv_stride", (4, 6, 10)), ("color_stride", (1, 3))):
        for v in values:
            assert _refused(m, ca.MeshLayout(**{field: v}), **q) == E_ARGUMENT, (field, v)
    n16 = ca.MeshView(m.position, m.index, n16_of(m.normal), m.color, m.uv)
    for v in (4, 5, 7):                                                         # int16 normals: a multiple of 2, at least 6
        assert _refused(n16, ca.MeshLayout(normal16=True, normal_stride=v), **q) == E_ARGUMENT
    assert len(ca.encode_layout(n16, ca.MeshLayout(normal16=True, normal_stride=6), **q)) > 0
    # generic attributes: double 8, int16 2, int8 1; at least components * element size
    for values, strides in ((np.zeros((m.nvert, 2)), (8, 12, 20)), (np.zeros((m.nvert, 3), np.int16), (4, 7)), (np.zeros((m.nvert, 3), np.int8), (2,)),
                            (np.zeros((m.nvert, 2), np.int32), (4, 10))):
        for v in strides:
            assert _refused(m, ca.MeshLayout(attr_stride=[v]), attributes=[("a", values, 0.5, 0)], model=False, **q) == E_ARGUMENT, (values.dtype, v)
    # a uint16 index is 2-byte aligned; an entry >= nvert is refused at either width
    raw = np.zeros(m.nface * 6 + 8, dtype=np.uint8)
    odd = np.ndarray(shape=(m.nface, 3), dtype=np.uint16, buffer=raw, offset=(-raw.ctypes.data) % 2 + 1, strides=(6, 2))
    assert _refused(ca.MeshView(m.position, odd), ca.MeshLayout(index16=True), **q) == E_ARGUMENT
    bad = m.index.astype(np.uint16)
    bad[3, 2] = m.nvert
    assert _refused(ca.MeshView(m.position, bad), ca.MeshLayout(index16=True), model=False, **q) == E_ARGUMENT
    assert "out of range" in ca.lib().crthip_last_error().decode()


def test_batch_entry_point_checks_need_no_device():
    L = ca.lib()
    assert L.crthip_abi_version() == 6
    offs = np.full(2, 77, dtype=np.uint64)
    lens = np.full(2, 77, dtype=np.uint32)
    descs = (ca.MeshDesc * 1)()
    call = lambda ctx, n, flags: L.crthip_encode_batch_layout(ctx, n, descs, None, None, 0, flags, None, 0, ca._np_ptr(offs), ca._np_ptr(lens),
                                                              None, None, None, None, None)
    assert call(None, 1, 0) == E_ARGUMENT and "context" in L.crthip_last_error().decode()
    assert call(None, 1, 4) == E_ARGUMENT and "flag" in L.crthip_last_error().decode()
    assert call(C.c_void_p(0x10), 0, 1) == 0 and call(None, 0, 3) == 0           # n == 0: nothing is touched, the context included
    assert offs[0] == 77 and lens[0] == 77
