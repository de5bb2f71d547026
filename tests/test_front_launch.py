"""GPU (-m gpu): k_front - a single-stream context's automata and bit-unpack in one grid (csrc/plan_launch.cpp) - against the two
kernels it replaces ($CORTO_FRONT=0), a two-stream context and the oracle: the same bytes from all four."""
import os

import numpy as np
import pytest

import corto_amd as ca
from conftest import GOLDEN, MESH_CASES, aligned, load_golden
from oracle import oracle as oc

pytestmark = pytest.mark.gpu

KEYS = ("position", "normal", "color", "uv", "radius", "index")


def decode_three_ways(monkeypatch, blobs):
    """the batch on a single-stream context (k_front where the batch allows it), on one with $CORTO_FRONT=0 and on a two-stream one;
    returns the three lists of host outputs and whether the first launched k_front"""
    outs, front = [], None
    for mode in ("front", "split", "two"):
        if mode == "split":
            monkeypatch.setenv("CORTO_FRONT", "0")
        else:
            monkeypatch.delenv("CORTO_FRONT", raising=False)
        c = ca.Context(0)                                    # (the switch is read when a context is made)
        b = None
        try:
            if mode != "two":
                c.set_single_stream(True)
            c.set_profiling(True)
            b = ca.Batch(c, blobs)
            b.allocate_outputs(fill=0)
            b.decode()
            st = b.sync()
            assert (st == 0).all(), (mode, st)
            names = b.kernel_times()
            if mode == "front":
                front = "front" in names
            else:
                assert "front" not in names, (mode, names)
            outs.append([b.host_outputs(i) for i in range(len(blobs))])
        finally:
            if b is not None:
                b.close()
            c.close()
    monkeypatch.delenv("CORTO_FRONT", raising=False)
    return outs, front


def assert_all_same(outs, refs, tag):
    for i, r in enumerate(refs):
        for k in KEYS:
            if k not in r:
                continue
            for way, o in zip(("front", "split", "two"), outs):
                assert k in o[i], (tag, i, way, k)
                assert o[i][k].dtype == r[k].dtype and o[i][k].shape == r[k].shape, (tag, i, way, k)
                assert o[i][k].tobytes() == r[k].tobytes(), (tag, i, way, k)


@pytest.mark.timeout(300)
def test_c4_blobs(monkeypatch):
    z = np.load(os.path.join(GOLDEN, "c4_blobs16.npz"))
    blobs = [aligned(z["crt_%02d" % s]) for s in range(16)]
    outs, front = decode_three_ways(monkeypatch, blobs)
    assert front
    assert_all_same(outs, [oc.decode(b) for b in blobs], "c4")


@pytest.mark.timeout(300)
def test_irregular_and_delaunay_batches(monkeypatch):
    from corto_amd import synth
    meshes = [synth.bumpy_sphere_flipped(64, 32, seed=s) for s in range(12)]
    blobs = [ca.encode(m, position_bits=14, uv_bits=12, normal_bits=10, normal_prediction=ca.BORDER if k % 2 else ca.ESTIMATED) for k, m in enumerate(meshes)]
    outs, front = decode_three_ways(monkeypatch, blobs)
    assert front
    assert_all_same(outs, [oc.decode(b) for b in blobs], "flipped")
    meshes = [synth.delaunay_disc(2310, seed=s, holes=6 + s % 5) for s in range(8)]
    blobs = [ca.encode(m, position_bits=14, uv_bits=12, normal_bits=10, normal_prediction=ca.BORDER) for m in meshes]
    outs, front = decode_three_ways(monkeypatch, blobs)
    assert front
    assert_all_same(outs, [oc.decode(b) for b in blobs], "delaunay")


@pytest.mark.timeout(300)
def test_golden_mesh_fixtures(monkeypatch):
    gs = [load_golden(n) for n in MESH_CASES]
    outs, _ = decode_three_ways(monkeypatch, [g["crt"] for g in gs])
    assert_all_same(outs, gs, "golden")
    for n, g in zip(MESH_CASES, gs):                         # and each alone: most of them a batch that k_front takes
        outs, _ = decode_three_ways(monkeypatch, [g["crt"]])
        assert_all_same(outs, [g], n)


@pytest.mark.timeout(300)
def test_batches_that_mix_in_blobs_k_front_does_not_take(monkeypatch):
    """a big mesh in a batch of C4 blobs (an automaton launched on its own: the batch keeps the two launches), and a finely quantised
    noisy mesh (wide alphabets) beside them"""
    from corto_amd import synth
    z = np.load(os.path.join(GOLDEN, "c4_blobs16.npz"))
    c4 = [aligned(z["crt_%02d" % s]) for s in range(8)]
    big = ca.encode(synth.bumpy_sphere_flipped(200, 100, seed=8, flip=0.1), position_bits=14, uv_bits=12, normal_bits=10, normal_prediction=ca.BORDER)
    wide = ca.encode(synth.bumpy_sphere(64, 32, seed=5, noise=0.2), position_bits=20, uv_bits=16, normal_bits=12, normal_prediction=ca.BORDER)
    for tag, blobs in (("big", c4 + [big]), ("wide", c4 + [wide]), ("both", [big] + c4 + [wide])):
        outs, _ = decode_three_ways(monkeypatch, blobs)
        assert_all_same(outs, [oc.decode(b) for b in blobs], tag)
