"""crthip_encode_batch with the CLERS topology pass on the device (Context.set_encode_topology): the same bytes as the host encoder for
every mesh - there is no connectivity the device pass hands back to the host - in device mode and in split mode."""
import ctypes as C

import numpy as np
import pytest

import corto_amd as ca
from corto_amd import synth
from conftest import load_golden
import topology_corpus as tc

pytestmark = pytest.mark.gpu

E_ARGUMENT, E_LIMIT = -8, -11
TOPO_KERNELS = ("enc_topo_compact", "enc_topo_pair", "enc_topo_walk")


@pytest.fixture(scope="module")
def dev():
    c = ca.Context(0)
    c.set_encode_topology("device")
    yield c
    c.close()


@pytest.fixture(scope="module")
def split():
    c = ca.Context(0)
    c.set_encode_topology("split")
    yield c
    c.close()


@pytest.fixture(scope="module")
def host():
    c = ca.Context(0)
    yield c
    c.close()


def _batch(ctx, items, **more):
    return ca.encode_batch([m for _, m, _ in items], ctx, kw=[k for _, _, k in items], with_stats=True, **more)


def test_golden_cases_in_one_batch(dev):
    cs = tc.golden_cases()
    blobs, st = _batch(dev, cs)
    for (name, _, _), b in zip(cs, blobs):
        assert b.tobytes() == load_golden(name)["crt"].tobytes(), name
    assert st["topology_device"] == sum(tc.is_mesh(m) for _, m, _ in cs)


def test_mixed_corpus_matches_single_encodes(dev, host):
    items = tc.mixed_corpus()
    nmesh = sum(tc.is_mesh(m) for _, m, _ in items)
    blobs, st = _batch(dev, items)
    for (name, m, k), b in zip(items, blobs):
        assert b.tobytes() == ca.encode(m, **k).tobytes(), name
    assert st["topology_device"] == nmesh and st["topology_lds"] == nmesh and st["device_topology_ms"] > 0
    for name in TOPO_KERNELS:
        assert name in st["kernel_times"] and st["kernel_times"][name]["launches"] >= 1, name
    # the same batch on a default context: the host pass, the same bytes, none of the new kernels
    hblobs, hst = _batch(host, items)
    assert hst["topology_device"] == 0 and hst["topology_lds"] == 0 and hst["device_topology_ms"] == 0
    for name in TOPO_KERNELS:
        assert name not in hst["kernel_times"], name
    for (name, _, _), a, b in zip(items, blobs, hblobs):
        assert a.tobytes() == b.tobytes(), name


def test_lds_and_global_state_in_one_batch(dev, split):
    """C4 units (4 096 faces: their walk state fits LDS) beside one mesh of 65 536 faces (32-bit links in the global image)"""
    kw = dict(normal_prediction=ca.BORDER)
    items = [("c4_%d" % s, synth.bumpy_sphere(64, 32, seed=s), kw) for s in range(5)]
    items.insert(2, tc.wide_mesh())
    items.append(("cloud", synth.point_cloud(30, 20, seed=2), kw))
    want = [ca.encode(m, **k).tobytes() for _, m, k in items]
    blobs, st = _batch(dev, items)
    assert [b.tobytes() for b in blobs] == want
    assert st["topology_device"] == 6 and st["topology_lds"] == 5
    assert 0 < st["topology_lds"] < st["topology_device"]
    admitted = sum(ca.encode_topology_fits_lds(m) for _, m, _ in items)          # the exported rule
    assert admitted == 5
    for threads in (1, 3):
        blobs, st = _batch(split, items, host_threads=threads)
        assert [b.tobytes() for b in blobs] == want
        assert st["topology_device"] == admitted and st["topology_lds"] == admitted


def test_pairing_rule_cases(dev, split):
    items = tc.pairing_cases()
    want = [ca.encode(m, **k).tobytes() for _, m, k in items]
    for ctx in (dev, split):
        blobs, st = _batch(ctx, items)
        for (name, _, _), b, w in zip(items, blobs, want):
            assert b.tobytes() == w, name
        assert st["topology_device"] == len(items)


def test_per_mesh_errors_leave_the_neighbours_alone(dev):
    kw = dict(normal_prediction=ca.BORDER)
    a, b, c = synth.bumpy_sphere(16, 8, seed=1), synth.bumpy_sphere(16, 8, seed=2), synth.bumpy_sphere(16, 8, seed=3)
    d = synth.bumpy_sphere(16, 8, seed=4)
    d.index = d.index.copy(); d.index[5, 1] = d.nvert + 3
    kws = [kw, dict(kw, color_bits=(6, 9, 6, 5)), kw, kw]
    blobs, status = ca.encode_batch([a, b, c, d], dev, kw=kws, raise_on_error=False)
    assert list(status) == [0, E_ARGUMENT, 0, E_ARGUMENT]
    assert len(blobs[1]) == 0 and len(blobs[3]) == 0
    assert blobs[0].tobytes() == ca.encode(a, **kw).tobytes() and blobs[2].tobytes() == ca.encode(c, **kw).tobytes()


def test_clers_stream_over_the_tunstall_limit(dev):
    """2.2 M separate triangles: 4 CLERS symbols a triangle, 8.8 M > 2^23, known only once the device pass has reported its count"""
    nt = 2_200_000
    pos = np.random.default_rng(3).random((3 * nt, 3), dtype=np.float32)
    big = synth.Mesh(position=pos, index=np.arange(3 * nt, dtype=np.uint32).reshape(-1, 3))
    small = synth.bumpy_sphere(16, 8, seed=4)
    kw = dict(with_normal=False, with_color=False, with_uv=False)
    blobs, status, st = ca.encode_batch([small, big, small], dev, kw=kw, raise_on_error=False, with_stats=True)
    assert status[1] == E_LIMIT and len(blobs[1]) == 0
    assert status[0] == 0 and status[2] == 0
    assert blobs[0].tobytes() == ca.encode(small, **kw).tobytes() and blobs[2].tobytes() == blobs[0].tobytes()
    assert st["topology_device"] == 3 and st["topology_lds"] == 2


def test_round_trip_through_the_batch_decoder(dev):
    from oracle import oracle as oc
    items = [c for c in tc.golden_cases() if c[0] in ("c4_unit", "two_groups", "holey_disc", "nonmanifold_fins", "confetti")]
    items.append(tc.pairing_cases(0)[0])
    blobs = [ca.aligned_blob(b) for b in _batch(dev, items)[0]]
    bt = ca.Batch(dev, blobs)
    bt.allocate_outputs(color_components=4)                         # (rgb and rgba fixtures alike, as the oracle is asked below)
    bt.decode()
    assert (bt.sync() == 0).all()
    for i, (name, m, k) in enumerate(items):
        got, ref = bt.host_outputs(i), oc.decode(ca.aligned_blob(ca.encode(m, **k)), color_components=4)
        for key in ("position", "normal", "color", "uv", "index"):
            assert got[key].tobytes() == ref[key].tobytes(), (name, key)
    bt.close()


def test_size_query_and_repeat_give_the_same_bytes(dev):
    ms = [synth.bumpy_sphere(20, 10, seed=s) for s in range(6)] + [synth.point_cloud(20, 10, seed=1), tc.book(48), tc.random_soup(7)]
    descs = (ca.MeshDesc * len(ms))()
    keep = []
    for i, m in enumerate(ms):
        descs[i], kp = ca._mesh_desc(m)
        keep.append(kp)
    offs0 = np.zeros(len(ms) + 1, dtype=np.uint64)
    total = ca.lib().crthip_encode_batch(dev.handle, len(ms), descs, 0, None, 0, offs0.ctypes.data_as(C.c_void_p), None, None, None, None, None)
    assert total > 0 and offs0[-1] == total
    runs = []
    for _ in range(2):
        out = np.zeros(total, dtype=np.uint8)
        offs = np.zeros(len(ms) + 1, dtype=np.uint64)
        r = ca.lib().crthip_encode_batch(dev.handle, len(ms), descs, 3, out.ctypes.data_as(C.c_void_p), total, offs.ctypes.data_as(C.c_void_p),
                                         None, None, None, None, None)
        assert r == total and (offs == offs0).all()
        runs.append(out)
    assert runs[0].tobytes() == runs[1].tobytes()
    for i, m in enumerate(ms):
        assert runs[0][int(offs0[i]):int(offs0[i + 1])].tobytes() == ca.encode(m).tobytes(), i


def test_unknown_mode_is_refused(host):
    assert ca.lib().crthip_ctx_set_encode_topology(host.handle, 3) == E_ARGUMENT
    assert ca.lib().crthip_ctx_set_encode_topology(host.handle, -1) == E_ARGUMENT
    with pytest.raises(ValueError):
        host.set_encode_topology("gpu")
