"""Generic vertex attributes on the device encoders: crthip_encode_gpu_attrs and crthip_encode_batch_attrs give crthip_encode_attrs's bytes
(FLOAT corpus, the reference-made fixture's INT32 / INT16 / INT8 / DOUBLE inputs, a mixed batch with a refused mesh, the host-sorted cloud
path, a 16-component attribute on a mesh of 65 536+ vertices, a LiDAR-like cloud of a million points through the direct uploads), and
the blobs decode on the batch decoder to what the C oracle decodes and to recipe(x)*q."""
import numpy as np
import pytest

import corto_amd as ca
from corto_amd import synth
from test_encode_generic_cpu import STRATEGIES, corpus, fixture_cases, float_values, recipe

pytestmark = pytest.mark.gpu

E_ARGUMENT, E_FORMAT = -8, -7


@pytest.fixture(scope="module")
def ctx():
    c = ca.Context(0)
    yield c
    c.close()


def float_items():
    """(mesh, keywords) of the FLOAT corpus: every N of the CPU test, every strategy, both entropies"""
    items = []
    k = 0
    for _, m in corpus():
        for N in (1, 3, 5, 16):
            for strategy in STRATEGIES:
                attrs = [("aa_first" if k % 2 else "zz_last", float_values(m.nvert, N, k), 0.03 if k % 3 else 0.5, strategy)]
                items.append((m, dict(entropy=k % 2, attributes=attrs)))
                k += 1
    return items


def fixture_items():
    return [(m, dict(kw, attributes=attrs)) for _, m, kw, attrs, _ in fixture_cases()]


def check_same(ctx, items, single=True):
    host = [ca.encode(m, **kw) for m, kw in items]
    if single:
        for (m, kw), h in zip(items, host):
            assert ca.encode(m, ctx=ctx, **kw).tobytes() == h.tobytes()
    blobs = ca.encode_batch([m for m, _ in items], ctx, kw=[kw for _, kw in items])
    for i, (b, h) in enumerate(zip(blobs, host)):
        assert b.tobytes() == h.tobytes(), i
    return blobs


def test_float_corpus_gpu_and_batch(ctx):
    check_same(ctx, float_items())


def test_fixture_inputs_gpu_and_batch(ctx):
    blobs = check_same(ctx, fixture_items())
    for (_, _, _, _, crt), b in zip(fixture_cases(), blobs):
        assert b.tobytes() == crt.tobytes()


def test_mixed_batch_with_a_refused_mesh(ctx):
    t = synth.torus(16, 8, seed=2)
    c = synth.point_cloud(20, 12, seed=3)
    d = synth.delaunay_disc(300, seed=5, holes=2)
    i16 = np.arange(t.nvert * 2, dtype=np.int16).reshape(-1, 2)
    items = [(t, dict(attributes=[("intensity", i16, 2.0, ca.PARALLEL)])),
             (c, dict()),
             (d, dict(attributes=[("bad", np.ones((d.nvert, 1), np.uint16), 1.0, 0)])),
             (c, dict(attributes=[("gps", np.linspace(-1e6, 1e6, c.nvert).reshape(-1, 1), 0.5, ca.CORRELATED),
                                  ("cls", (np.arange(c.nvert) % 31).astype(np.int8).reshape(-1, 1), 1.0, 0)])),
             (d, dict(attributes=[("normal", np.ones((d.nvert, 2), np.float32), 1.0, 0)])),
             (t, dict(entropy=0))]
    blobs, status = ca.encode_batch([m for m, _ in items], ctx, kw=[kw for _, kw in items], raise_on_error=False)
    assert list(status) == [0, 0, E_FORMAT, 0, E_ARGUMENT, 0]
    for i, (m, kw) in enumerate(items):
        if status[i] == 0:
            assert blobs[i].tobytes() == ca.encode(m, **kw).tobytes(), i
        else:
            assert len(blobs[i]) == 0


def test_cloud_with_duplicate_points_takes_the_host_sort(ctx):
    c = synth.point_cloud(24, 16, seed=9)
    pos = np.concatenate([c.position, c.position[:100]])
    dup = synth.Mesh(pos)
    rng = np.random.default_rng(4)
    attrs = [("w", rng.normal(size=(dup.nvert, 7)).astype(np.float32), 0.01, s) for s in (0,)] + \
            [("t", rng.normal(size=(dup.nvert, 2)) * 1e5, 0.125, ca.PARALLEL | ca.CORRELATED)]
    blobs, st = ca.encode_batch([dup], ctx, kw=[dict(attributes=attrs)], with_stats=True)
    assert st["clouds_host_sorted"] == 1
    assert blobs[0].tobytes() == ca.encode(dup, attributes=attrs).tobytes()


def test_sixteen_components_on_a_large_mesh(ctx):
    m = synth.bumpy_sphere(320, 210, seed=8)
    assert m.nvert >= 65536
    v = float_values(m.nvert, 16, 8)
    for strategy in (ca.PARALLEL, ca.PARALLEL | ca.CORRELATED):
        check_same(ctx, [(m, dict(attributes=[("tangents", v, 0.001, strategy)]))])


def lidar(n=1000003, seed=11):
    rng = np.random.default_rng(seed)
    pos = (rng.random((n, 3), dtype=np.float32) * np.float32(200.0)).astype(np.float32)
    attrs = [("intensity", rng.integers(0, 65535, size=(n, 1)).astype(np.int32).astype(np.int16), 1.0, 0),
             ("classification", rng.integers(0, 20, size=(n, 1)).astype(np.int8), 1.0, 0),
             ("gps_time", (50.0 + np.arange(n) * 5e-5 + rng.random(n) * 1e-6).reshape(-1, 1), 1e-5, ca.CORRELATED)]
    return synth.Mesh(pos), attrs


def test_lidar_cloud_through_the_direct_uploads(ctx):
    m, attrs = lidar()
    kw = dict(position_bits=0, position_q=0.001, attributes=attrs)
    host = ca.encode(m, **kw)
    assert ca.encode_batch([m], ctx, kw=[kw])[0].tobytes() == host.tobytes()
    assert ca.encode(m, ctx=ctx, **kw).tobytes() == host.tobytes()


def test_round_trip_through_the_batch_decoder(ctx):
    """every generic attribute decodes on the device to what the C oracle decodes, and to recipe(x)*q of the input vertex it came from
    (an INT32 attribute "vid" carries the input vertex ids through the encoder's reordering).  recipe(x)*q where every quantised value is
    below 2^28: residuals of 2^30 and more do not come back from upstream's encodeValues (`(1<<ret)>>1` in int, include/corto/cstream.h:133,
    the fields31 fixture) - the fixture's adversarial inputs are there for the encoder's bytes"""
    from oracle import oracle as oc
    items = []
    for m, kw in fixture_items()[::2] + float_items()[::5]:
        vid = np.arange(m.nvert, dtype=np.int32).reshape(-1, 1)
        kw = dict(kw, attributes=list(kw["attributes"]) + [("vid", vid, 1.0, ca.CORRELATED)])
        items.append((m, kw))
    blobs = [ca.aligned_blob(b) for b in ca.encode_batch([m for m, _ in items], ctx, kw=[kw for _, kw in items])]
    b = ca.Batch(ctx, blobs)
    b.allocate_outputs()
    b.decode()
    assert (b.sync() == 0).all()
    covered = set()
    for i, ((m, kw), blob) in enumerate(zip(items, blobs)):
        got = b.host_outputs(i)
        ref = oc.decode(blob)
        ids = got["vid"][:, 0].astype(np.int64)
        assert ids.min() >= 0 and ids.max() < m.nvert
        for name, v, q, s in kw["attributes"]:
            assert got[name].tobytes() == ref[name].tobytes(), (i, name)
            v = np.asarray(v).reshape(m.nvert, -1)
            r = recipe(v, q)
            if np.abs(r.astype(np.int64)).max() >= 1 << 28:
                continue
            want = r[ids].astype(np.float32) * np.float32(q)
            assert np.array_equal(got[name].view(np.uint32), want.view(np.uint32)), (i, name, s)
            covered.add((bool(m.nface), v.dtype.str, v.shape[1] > 4, s))
    b.close()
    assert {d for _, d, _, _ in covered} >= {"<i4", "<i2", "|i1", "<f8", "<f4"}
    assert {(c, w, s) for c, _, w, s in covered} >= {(c, True, s) for c in (False, True) for s in STRATEGIES}
