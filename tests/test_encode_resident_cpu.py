"""crthip_encode_batch_resident without a device: the entry points' argument checks, and the input pass's source (csrc/enc_input_check.h)
run on the host in the kernels' partition (crthip_encode_input_model, which = 1) against the host encoder's own loops (which = 0), bit
for bit - floats compared as uint32 and the sum as uint64, so NaNs and the sign of a zero count."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import corto_amd as ca
from corto_amd import synth
from conftest import GOLDEN, ROOT

E_ARGUMENT = -8
TILE = 1024                      # EIN_TILE: vertices a workgroup folds into one partial box
EDGE_TILE = 1024                 # EIN_EDGE_TILE


def _cases():
    sys.path.insert(0, GOLDEN)
    from cases import cases
    return cases()


def _bits(r):
    return (r["index_out_of_range"], r["recipe"], r["mn"].view(np.uint32).tolist(), r["mx"].view(np.uint32).tolist(),
            int(np.array([r["sum"]], dtype=np.float64).view(np.uint64)[0]), int(np.array([r["step"]], dtype=np.float32).view(np.uint32)[0]))


def _parity(m, **kw):
    a, b = ca.encode_input_model(m, 0, **kw), ca.encode_input_model(m, 1, **kw)
    assert _bits(a) == _bits(b), (kw, a, b)
    return a


RECIPES = (dict(position_bits=14), dict(position_bits=0, position_q=0.0))   # box from vertex 0; a mesh: mean edge, a cloud: box from +-FLT_MAX


def test_symbols_header_and_abi():
    L = ca.lib()
    assert L.crthip_abi_version() == 6
    header = open(os.path.join(ROOT, "include", "corto_hip.h")).read()
    for name in ("crthip_encode_batch_resident", "crthip_encode_input_model"):
        assert hasattr(L, name), name
        assert name + "(" in header, name


def _call(ctx, n, meshes, offs):
    return ca.lib().crthip_encode_batch_resident(ctx, n, meshes, None, 0, None, 0, offs, None, None, None, None, None)


def test_argument_checks_need_no_device():
    offs = np.full(2, 77, dtype=np.uint64)
    descs = (ca.MeshDesc * 1)()
    assert _call(None, 1, descs, ca._np_ptr(offs)) == E_ARGUMENT
    assert "context" in ca.lib().crthip_last_error().decode()
    # n == 0: nothing to do, and the context is not touched (this one is no context at all)
    bogus = C.c_void_p(0x10)
    assert _call(bogus, 0, None, ca._np_ptr(offs)) == 0
    assert offs[0] == 0
    assert _call(bogus, 0, None, None) == E_ARGUMENT
    assert _call(bogus, 1, descs, None) == E_ARGUMENT


def test_model_parity_golden_cases():
    for name, m, k in _cases():
        for extra in ({},) + RECIPES:
            kw = dict(k); kw.update(extra)
            r = _parity(m, **kw)
            assert r["index_out_of_range"] == 0, name


def test_model_parity_synth_across_tiles():
    rng = np.random.default_rng(2024)
    n = 0
    for s in range(120):
        nu, nv = int(rng.integers(8, 90)), int(rng.integers(5, 60))
        m = synth.bumpy_sphere(nu, nv, seed=1000 + s)
        for kw in RECIPES:
            _parity(m, **kw); n += 1
        c = synth.point_cloud(nu, nv, seed=2000 + s)
        for kw in RECIPES:
            _parity(c, **kw); n += 1
    assert n >= 300
    # vertex counts at the tile size and one either side, over several tiles; face counts around the edge tile
    big = synth.bumpy_sphere(96, 48, seed=5)
    assert big.nvert > 4 * TILE and big.nface > 4 * EDGE_TILE
    for nvert in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 4 * TILE + 3, 3, 4, 5, 1):
        cloud = synth.Mesh(position=big.position[:nvert].copy())
        for kw in RECIPES:
            _parity(cloud, **kw)
        for nface in (EDGE_TILE - 1, EDGE_TILE, EDGE_TILE + 1, 3 * EDGE_TILE + 1, 1):
            idx = (big.index[:nface] % np.uint32(nvert)).astype(np.uint32)
            mesh = synth.Mesh(position=big.position[:nvert].copy(), index=idx)
            for kw in RECIPES:
                _parity(mesh, **kw)


def _edge_inputs():
    base = synth.bumpy_sphere(40, 30, seed=77)
    assert base.nvert > TILE
    out = []

    def variant(name, edit, cloud=False):
        p = base.position.copy()
        edit(p)
        out.append((name, synth.Mesh(position=p, index=None if cloud else base.index.copy())))

    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for cloud in (False, True):
        variant("nan_first", lambda p: p.__setitem__((0, 1), nan), cloud)
        variant("nan_first_all", lambda p: p.__setitem__(0, nan), cloud)
        variant("nan_elsewhere", lambda p: (p.__setitem__((5, 0), nan), p.__setitem__((TILE + 3, 2), nan), p.__setitem__(p.shape[0] - 1, nan)), cloud)
        variant("nan_whole_tile", lambda p: p.__setitem__(slice(TILE, 2 * TILE), nan) if p.shape[0] >= 2 * TILE else p.__setitem__(slice(TILE, None), nan), cloud)
        variant("plus_inf", lambda p: p.__setitem__((7, 0), inf), cloud)
        variant("minus_inf", lambda p: p.__setitem__((9, 2), -inf), cloud)
        variant("both_inf", lambda p: (p.__setitem__((7, 1), inf), p.__setitem__((TILE + 1, 1), -inf)), cloud)
        variant("inf_first", lambda p: p.__setitem__(0, inf), cloud)

        def zeros(first_negative):
            def edit(p):
                p[:] = 0.0
                sel = np.arange(p.shape[0]) % 2 == (0 if first_negative else 1)
                p[sel] = np.float32(-0.0)
            return edit
        variant("zeros_minus_first", zeros(True), cloud)
        variant("zeros_plus_first", zeros(False), cloud)

        def late_zero(p):
            p[:] = 0.0
            p[TILE + 5] = np.float32(-0.0)                        # the other zero only in a later tile: the first one stays
        variant("zero_sign_in_later_tile", late_zero, cloud)
    return out


def test_model_parity_edge_inputs():
    seen = set()
    for name, m in _edge_inputs():
        for kw in RECIPES:
            r = _parity(m, **kw)
            seen.add((name, r["recipe"]))
            if name == "nan_first" and r["recipe"] == 1:
                assert np.isnan(r["mn"][1]) and np.isnan(r["mx"][1]) and not np.isnan(r["mn"][0])
            if name == "nan_elsewhere" and r["recipe"] in (1, 3):
                assert not np.isnan(r["mn"]).any() and not np.isnan(r["mx"]).any()
            if name == "zeros_minus_first" and r["recipe"] == 1:
                assert np.signbit(r["mn"]).all() and np.signbit(r["mx"]).all()
            if name == "zeros_plus_first" and r["recipe"] == 1:
                assert not np.signbit(r["mn"]).any() and not np.signbit(r["mx"]).any()
            if name == "zero_sign_in_later_tile" and r["recipe"] == 1:
                assert not np.signbit(r["mn"]).any() and not np.signbit(r["mx"]).any()
    assert {r for _, r in seen} == {1, 2, 3}


def test_model_index_out_of_range_and_empty():
    m = synth.bumpy_sphere(40, 30, seed=3)
    bad = synth.Mesh(position=m.position.copy(), index=m.index.copy())
    bad.index[EDGE_TILE + 7, 1] = bad.nvert                       # == nvert: the first value out of range, in a face's first edge
    for kw in RECIPES:
        r = _parity(bad, **kw)
        assert r["index_out_of_range"] == 1
        assert r["sum"] == 0 and r["step"] == 0                    # and nothing was gathered through it (the guard page test of a wild read
                                                                   # is the huge index below: a gather would leave the process's memory)
    wild = synth.Mesh(position=m.position.copy(), index=m.index.copy())
    wild.index[3, 0] = 0xFFFFFFF0
    wild.index[m.nface - 1, 2] = 0xFFFFFFFF                       # not on a first edge: only the range pass sees it
    for kw in RECIPES:
        assert _parity(wild, **kw)["index_out_of_range"] == 1
    last = synth.Mesh(position=m.position.copy(), index=m.index.copy())
    last.index[m.nface - 1, 2] = last.nvert
    assert _parity(last, position_bits=14)["index_out_of_range"] == 1
    good = _parity(m, position_bits=0, position_q=0.0)
    assert good["index_out_of_range"] == 0 and good["recipe"] == 2 and good["sum"] > 0
    # nvert == 0: position only has to be non-null and is never read
    backing = np.zeros((4, 3), dtype=np.float32)
    empty = synth.Mesh(position=backing[:0])
    empty.position = backing[:0]
    for kw in RECIPES + (dict(position_bits=0, position_q=0.5),):
        r = _parity(empty, **kw)
        assert r["step"] == np.float32(kw.get("position_q", 0.0)) and r["index_out_of_range"] == 0


def test_model_step_is_the_q_the_encoder_writes():
    cs = _cases()
    picks = [(m, k) for _, m, k in cs[:4]] + [(cs[-1][1], cs[-1][2])]
    big = synth.bumpy_sphere(96, 48, seed=5)
    picks += [(big, dict(normal_prediction=ca.DIFF)), (synth.point_cloud(60, 40, seed=4), dict(normal_prediction=ca.DIFF))]
    for m, k in picks:
        for extra in ({},) + RECIPES + (dict(position_bits=0, position_q=0.25),):
            kw = dict(k); kw.update(extra)
            blob = ca.encode(m, **kw)
            q = [a["q"] for a in ca.probe(ca.aligned_blob(blob)).attrs() if a["name"] == "position"][0]
            step = ca.encode_input_model(m, 0, **kw)["step"]
            assert np.float32(q).view(np.uint32) == np.float32(step).view(np.uint32), kw
