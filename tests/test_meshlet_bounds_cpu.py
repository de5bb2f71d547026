"""crthip_batch_bind_meshlet_bounds without a device: the kernel's source on the host (corto_amd.meshlet_bounds_model: csrc/meshlet_bounds.h in
k_meshlet_bounds.hip's partition, workgroups, waves and lanes shuffled by a seed) against the sequential model of the record
(tests/meshlet_bounds.py), byte for byte; the properties every result has whatever the model says; the declarations and the errors that
need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import corto_amd as ca
import meshlet_bounds as mb
import meshlets as ml
from conftest import MESH_CASES, ROOT, aligned

SEEDS = (0, 1, 7)


def hook_equals_model(P, nvert, build, tag, seeds=SEEDS):
    """build: (meshlets, vertices, triangles, counts) - the hook under every seed against the model, and the properties of both"""
    P = np.asarray(P)[:len(P) if nvert is None else nvert]
    m, v, t, c = build
    exp = mb.model(P, m, v, t)
    mb.check_properties(P, m, v, t, exp, tag=(tag, "model"))
    for seed in seeds:
        got = ca.meshlet_bounds_model(P, None, m, v, t, c, seed=seed)
        mb.assert_same(got, exp, (tag, seed))
    return exp


# ---- 1. hook equals model ----

@pytest.mark.parametrize("params", ml.PARAMS, ids=lambda p: "%d_%d_%d" % p)
def test_hook_equals_model(params):
    for name in MESH_CASES:
        P, idx, groups, _ = mb.golden(name)
        build, exp = mb.golden_build(name, params)
        mb.check_properties(P, *build[:3], exp, tag=(name, params, "model"))
        for seed in SEEDS:
            mb.assert_same(ca.meshlet_bounds_model(P, idx, *build, seed=seed), exp, (name, params, seed))


def test_the_golden_meshes_have_cones_that_cull():
    """the comparison above is not of records that all say "do not cull": a meshlet of four faces of a smooth mesh spans a few degrees, so
    nearly all of them get a cutoff below 127 (a meshlet of 124 faces in decode order is a strip that winds round the surface: few do)"""
    for name in ("torus", "icosphere", "c4_unit"):
        exp = mb.golden_build(name, (8, 4, 16))[1]
        assert (exp["cone_cutoff"] < 127).mean() > 0.9, (name, exp["cone_cutoff"])
        assert (exp["radius"] > 0).all()
        assert (mb.golden_build(name, (64, 124, 0))[1]["cone_cutoff"] < 127).any(), name


@pytest.mark.parametrize("name", sorted(mb.synthetic()))
def test_hand_made_inputs(name):
    P, nvert, idx, params = mb.synthetic()[name]
    n = len(P) if nvert is None else nvert
    build = mb.build_host(idx, params)
    ml.assert_same(build, ml.build(idx, (), *params), name)                      # (the meshlets themselves: the other contract)
    exp = hook_equals_model(P, nvert, build, name)
    m = build[0]
    if name == "one_face":
        assert len(exp) == 1 and exp[0]["cone_cutoff"] == 2 and exp[0]["cone_axis"].tolist() == [0, 0, 127]
    if name == "one_face_each":                                                  # every meshlet is one face: the axis is its normal, m = 1, cutoff 2
        assert len(exp) == len(idx) and (exp["cone_cutoff"] == 2).all()
        p = P.astype(np.int64)
        N = np.cross(p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]]).astype(np.float64)
        N /= np.linalg.norm(N, axis=1)[:, None]
        assert np.abs(exp["cone_axis"] - N * 127).max() <= 0.5 + 1e-3
    if name == "full_meshlet":
        assert m.tolist() == [[0, 0, 255, 512]]
    if name.startswith("wave_edge_"):
        n_ = int(name.rsplit("_", 1)[1])
        assert m.tolist() == [[0, 0, n_, n_]]
    if name == "planar_patch":
        assert (exp["cone_cutoff"] == 2).all() and (exp["cone_axis"] == [0, 0, 127]).all() and (exp["box_min"][:, 2] == 0).all() and (exp["box_max"][:, 2] == 0).all()
    if name == "closed_sphere_one_meshlet":
        assert len(exp) == 1 and exp[0]["cone_cutoff"] == 127
    if name in ("all_degenerate", "two_opposite_faces"):
        assert len(exp) == 1 and exp[0]["cone_cutoff"] == 127 and exp[0]["cone_axis"].tolist() == [0, 0, 0] and exp[0]["radius"] > 0
    if name == "coordinates_at_23_bits":                                         # the shifts kS and kN are not zero
        assert max(abs(mb._s64(x)) for x in mb.face_normal([tuple(int(x) for x in r) for r in P], 0, 1, 2)).bit_length() > 24
    if name == "int32_ends_one_meshlet":
        assert len(exp) == 1 and exp[0]["box_min"].tolist() == [mb.I32_MIN] * 3 and exp[0]["box_max"].tolist() == [mb.I32_MAX] * 3
        assert exp[0]["center"].tolist() == [-1, -1, -1] and exp[0]["radius"] == mb.ceil_sqrt(3 * (2 ** 31) ** 2)
    if name == "absent_ids_all_of_one":
        empty = [k for k in range(len(m)) if (build[1][m[k, 0]:m[k, 0] + m[k, 2]] >= n).all()]
        assert empty and all(exp[k].tobytes() == bytes(43) + b"\x7f" + bytes(4) for k in empty)
    if name == "absent_ids_some":
        assert len(exp) == 1 and (build[1] >= n).any() and exp[0]["radius"] > 0 and exp[0]["cone_cutoff"] < 127
    if name == "one_vertex":
        assert exp[0]["box_min"].tolist() == exp[0]["box_max"].tolist() == exp[0]["center"].tolist() == [5, -6, 7] and exp[0]["radius"] == 0
        assert exp[0]["cone_cutoff"] == 127


def test_no_vertices_at_all():
    """nvert == 0: every id is absent, every record the all-zero one with cutoff 127; the position may be NULL"""
    idx = np.array([[0, 1, 2], [2, 1, 3]], np.uint32)
    build = mb.build_host(idx, (64, 124, 0))
    got = ca.meshlet_bounds_model(np.zeros((0, 3), np.int32), idx, *build)
    assert got.tobytes() == bytes(43) + b"\x7f" + bytes(4)


def test_the_ceiling_square_root_at_its_edges():
    """through the hook: an even and an odd span (the centre is span >> 1 above the minimum), the widest span, and an r2 that is no square"""
    for d, exp in ((6, 3), (7, 4), (2 ** 32 - 1, 2 ** 31)):
        lo = -(d // 2) - 1
        P = np.array([[lo, 0, 0], [lo + d, 0, 0], [lo, 0, 0]], np.int64).astype(np.int32)
        idx = np.array([[0, 1, 2]], np.uint32)
        got = ca.meshlet_bounds_model(P, idx, *mb.build_host(idx, (64, 124, 0)))
        assert got[0]["radius"] == exp and got[0]["radius"] == mb.model(P, *mb.build_host(idx, (64, 124, 0))[:3])[0]["radius"], (d, got)
    # two axes: r2 = 5*5 + 5*5 = 50, the least r with r*r >= 50 is 8
    P = np.array([[0, 0, 0], [10, 10, 0], [0, 10, 0]], np.int32)
    idx = np.array([[0, 1, 2]], np.uint32)
    assert ca.meshlet_bounds_model(P, idx, *mb.build_host(idx, (64, 124, 0)))[0]["radius"] == 8


# ---- 2. nothing past the counts ----

def test_records_at_the_counts_and_nothing_past_them():
    P, idx, groups, _ = mb.golden("group_props")
    for params in ml.PARAMS:
        build, exp = mb.golden_build("group_props", params)
        cap = ml.bound(len(idx), groups, *params)[0]
        for capacity in (build[3][0], cap):                                          # exactly the counts; the bound, as a binding has it
            raw = ca.meshlet_bounds_model(P, idx, *build, seed=9, capacity=capacity, fill=0x5A, raw=True)
            assert len(raw) == capacity * 48 and (raw[build[3][0] * 48:] == 0x5A).all(), (params, capacity)
            mb.assert_same(raw[:build[3][0] * 48].view(mb.DT), exp, (params, capacity))


# ---- 3. declarations and arguments ----

def test_the_calls_are_exported_and_declared():
    L = ca.lib()
    names = ["crthip_batch_bind_meshlet_bounds", "crthip_meshlet_bounds_model"]
    assert all(hasattr(L, n) for n in names)
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "corto_hip.h")).read())
    assert "int crthip_batch_bind_meshlet_bounds(crthip_batch *b, uint32_t i, crthip_meshlet_bounds *bounds, uint32_t capacity);" in hdr
    added = hdr[hdr.index("#define CRTHIP_ABI_VERSION"):]
    added = added[:added.index("*/")]                                                            # the "added within 6" list
    for n in names + ["crthip_meshlet_bounds,"]:
        assert n in added, n
    assert L.crthip_abi_version() == 6 and re.search(r"#define CRTHIP_ABI_VERSION 6\b", hdr)      # additive: the number stays
    assert C.sizeof(ca.MeshletBounds) == 48 and ca.MESHLET_BOUNDS_DTYPE.itemsize == 48
    for f, off in (("box_min", 0), ("box_max", 12), ("center", 24), ("radius", 36), ("cone_axis", 40), ("cone_cutoff", 43), ("reserved", 44)):
        assert getattr(ca.MeshletBounds, f).offset == off == ca.MESHLET_BOUNDS_DTYPE.fields[f][1], f
    for n in ("bind_meshlet_bounds", "meshlet_bounds"):
        assert hasattr(ca.Batch, n)
    assert hasattr(ca, "meshlet_bounds_model")


def test_the_header_is_c99_with_the_new_struct(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "corto_hip.h"\n'
                   "typedef char size_is_48[sizeof(crthip_meshlet_bounds) == 48 ? 1 : -1];\n"
                   "int use(crthip_batch *b, crthip_meshlet_bounds *r) {\n"
                   "  crthip_meshlet_counts c = {0, 0, 0, 0};\n"
                   "  r->cone_cutoff = 127; r->box_min[0] = r->box_max[2]; r->radius = (uint32_t)r->center[1]; r->reserved = (uint32_t)r->cone_axis[2];\n"
                   "  return crthip_batch_bind_meshlet_bounds(b, 0, r, 4) + crthip_meshlet_bounds_model(0, 0, 0, 0, 0, &c, r, 4, 0);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_arguments():
    L = ca.lib()
    rec = (ca.MeshletBounds * 2)()
    assert L.crthip_batch_bind_meshlet_bounds(None, 0, C.byref(rec), 1) == mb.E_ARGUMENT
    assert L.crthip_batch_bind_meshlet_bounds(None, 0, None, 0) == mb.E_ARGUMENT
    assert b"no such blob" in L.crthip_last_error()
    assert L.crthip_meshlet_bounds_model(None, 0, None, None, None, None, None, 0, 0) == mb.E_ARGUMENT


def test_the_hook_refuses_what_is_not_a_finished_build():
    P, idx = mb.grid(2, 2, 10)
    m, v, t, c = mb.build_host(idx, (64, 124, 0))
    assert len(ca.meshlet_bounds_model(P, idx, m, v, t, c)) == 1
    with pytest.raises(ca.CortoError):                                               # capacity below the counts
        ca.meshlet_bounds_model(P, idx, m, v, t, c, capacity=0)
    for col, val in ((0, len(v)), (1, len(t)), (2, 256), (2, len(v) + 1), (3, 513), (3, len(t) // 3 + 1)):
        bad = m.copy()
        bad[0, col] = val
        with pytest.raises(ca.CortoError):
            ca.meshlet_bounds_model(P, idx, bad, v, t, c)
    bad = t.copy()
    bad[4] = m[0, 2]                                                                 # a local id that is not below the vertex count
    with pytest.raises(ca.CortoError):
        ca.meshlet_bounds_model(P, idx, m, v, bad, c)
    with pytest.raises(ValueError):                                                  # counts beyond the arrays
        ca.meshlet_bounds_model(P, idx, m, v, t, (2, len(v), len(t), 1))
    L = ca.lib()
    raw = np.zeros(48 * 2 + 32, np.uint8)
    off = (-raw.ctypes.data) % 16 + 4                                                # a misaligned record array
    cc = ca.MeshletCounts(*c.as_tuple())
    ma = aligned(np.ascontiguousarray(m).view(np.uint8).reshape(-1))
    assert L.crthip_meshlet_bounds_model(P.ctypes.data, len(P), ma.ctypes.data, v.ctypes.data, t.ctypes.data, C.byref(cc),
                                         raw.ctypes.data + off, 1, 0) == mb.E_ARGUMENT
    assert b"16-byte aligned" in L.crthip_last_error()
