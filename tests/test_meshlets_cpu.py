"""crthip_batch_bind_meshlets without a device: the kernels' source on the host (corto_amd.meshlet_model: csrc/meshlet.h in both of
k_meshlet.hip's partitions, segments and lanes shuffled by a seed) against the sequential model of the contract (tests/meshlets.py), byte for byte;
the properties every result has whatever the model says; the bound; the declarations."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import corto_amd as ca
import meshlets as ml
from conftest import MESH_CASES, ROOT

SEEDS = (0, 1, 7)


def both_partitions(index, groups, params, tag, seeds=SEEDS):
    exp = ml.build(index, groups, *params)
    ml.check_properties(index, groups, params, *exp, tag=(tag, "model"))
    for which in (0, 1):
        for seed in seeds:
            got = ca.meshlet_model(index, groups, *params, which=which, seed=seed)
            ml.assert_same(got, exp, (tag, params, which, seed))
            ml.check_properties(index, groups, params, *got[:3], got[3].as_tuple(), tag=(tag, params, which, seed))
    return exp


# ---- 1. hook equals model ----

@pytest.mark.parametrize("params", ml.PARAMS, ids=lambda p: "%d_%d_%d" % p)
def test_hook_equals_model(params):
    for name in MESH_CASES:
        idx, groups, _ = ml.golden(name)
        both_partitions(idx, groups, params, name)


@pytest.mark.parametrize("params", ml.PARAMS, ids=lambda p: "%d_%d_%d" % p)
def test_hook_equals_model_uint16_index(params):
    for name in MESH_CASES:
        idx, groups, _ = ml.golden(name)
        assert idx.max() < 65536
        both_partitions(idx.astype(np.uint16), groups, params, name, seeds=(2,))


@pytest.mark.parametrize("name", ["two_groups", "group_props"])
def test_every_group_end_is_a_meshlet_boundary(name):
    idx, groups, _ = ml.golden(name)
    assert len(groups) >= 2 and groups[-1] == len(idx)
    for params in ml.PARAMS:
        m, v, t, c = ca.meshlet_model(idx, groups, *params, which=1, seed=4)
        first = set(np.concatenate([[0], np.cumsum(m[:, 3])]).tolist())
        assert set(groups) <= first, (params, groups)
        assert c.segments == len(ml.cuts(len(idx), groups, params[2]))
    # ... and the table matters: without it the first group's end falls inside a meshlet
    m = ca.meshlet_model(idx, (), 64, 124, 0)[0]
    assert groups[0] not in set(np.cumsum(m[:, 3]).tolist())


@pytest.mark.parametrize("name", sorted(ml.synthetic()))
def test_inputs_no_decoded_blob_can_produce(name):
    idx, groups = ml.synthetic()[name]
    for params in ml.PARAMS + [(64, 64, 63), (5, 3, 2)]:
        both_partitions(idx, groups, params, name, seeds=(0, 5))


def test_a_face_that_names_a_vertex_twice():
    idx = np.array([[7, 7, 9], [9, 9, 9], [3, 7, 3], [1, 2, 3]], np.uint32)
    m, v, t, c = ca.meshlet_model(idx, (), 64, 124, 0)
    assert m.tolist() == [[0, 0, 5, 4]] and v.tolist() == [7, 9, 3, 1, 2] and t.tolist() == [0, 0, 1, 1, 1, 1, 2, 0, 2, 3, 4, 2]
    assert c.as_tuple() == (1, 5, 12, 1)
    # at three vertices a meshlet the first three faces (7, 9 and 3) still share one; the fourth brings two more and starts the next
    m, v, t, c = ca.meshlet_model(idx, (), 3, 124, 0)
    assert m.tolist() == [[0, 0, 3, 3], [3, 12, 3, 1]] and v.tolist() == [7, 9, 3, 1, 2, 3]
    assert t.tolist() == [0, 0, 1, 1, 1, 1, 2, 0, 2, 0, 0, 0, 0, 1, 2, 0]
    # ... and at two faces a meshlet the triangle limit cuts first
    m, v, t, c = ca.meshlet_model(idx, (), 3, 2, 0)
    assert m.tolist() == [[0, 0, 2, 2], [2, 8, 2, 1], [4, 12, 3, 1]] and v.tolist() == [7, 9, 3, 7, 1, 2, 3]
    assert t.tolist() == [0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 2, 0]


# ---- 2. the bound ----

def test_the_bound():
    for name in MESH_CASES:
        idx, groups, _ = ml.golden(name)
        for params in ml.PARAMS:
            assert ca.meshlet_bound(len(idx), groups, *params).as_tuple() == ml.bound(len(idx), groups, *params), (name, params)
    for idx, groups in ml.synthetic().values():
        for params in ml.PARAMS:
            assert ca.meshlet_bound(len(idx), groups, *params).as_tuple() == ml.bound(len(idx), groups, *params)


def test_the_bound_is_reached_at_3_1_1():
    for name in ("torus", "confetti", "two_groups"):
        idx, groups, _ = ml.golden(name)
        c = ca.meshlet_model(idx, groups, 3, 1, 1)[3]
        bd = ca.meshlet_bound(len(idx), groups, 3, 1, 1)
        assert c.meshlets == bd.meshlets == len(idx) and c.vertices <= bd.vertices and c.segments == len(idx)
    soup = np.arange(3 * 50, dtype=np.uint32).reshape(-1, 3)                     # three new vertices a face: the meshlet and the vertex capacities are met
    c, bd = ca.meshlet_model(soup, (), 3, 1, 1)[3], ca.meshlet_bound(50, (), 3, 1, 1)
    assert c.as_tuple() == (50, 150, 200, 50) and bd.as_tuple() == (50, 150, 300, 50)   # (triangle_bytes: 4 a one-face meshlet against the bound's 3 + 3)
    c, bd = ca.meshlet_model(soup, (), 255, 512, 0)[3], ca.meshlet_bound(50, (), 255, 512, 0)
    assert c.as_tuple() == (1, 150, 152, 1) and bd.as_tuple() == (1, 150, 153, 1)


def test_arrays_at_the_counts_and_nothing_past_them():
    """arrays that end at the capacity, filled with a pattern: bytes past the counts keep it"""
    idx, groups, _ = ml.golden("group_props")
    for params in ml.PARAMS:
        for which in (0, 1):
            m, v, t, c = ca.meshlet_model(idx, groups, *params, which=which, seed=9, raw=True, fill=0x5A)
            assert (m[c.meshlets * 16:] == 0x5A).all() and (v[c.vertices * 4:] == 0x5A).all() and (t[c.triangle_bytes:] == 0x5A).all()
            ml.assert_same(ca.cut_meshlets(m, v, t, c) + (c,), ml.build(idx, groups, *params), (params, which))


# ---- 3. declarations and arguments ----

def test_the_calls_are_exported_and_declared():
    L = ca.lib()
    names = ["crthip_meshlet_bound", "crthip_batch_bind_meshlets", "crthip_batch_meshlet_counts", "crthip_meshlet_model"]
    assert all(hasattr(L, n) for n in names)
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "corto_hip.h")).read())
    assert "typedef struct crthip_meshlet { uint32_t vertex_offset, triangle_offset, vertex_count, triangle_count; } crthip_meshlet;" in hdr
    assert "typedef struct crthip_meshlet_counts { uint32_t meshlets, vertices, triangle_bytes, segments; } crthip_meshlet_counts;" in hdr
    assert ("int crthip_meshlet_bound(uint32_t nface, uint32_t ngroups, const uint32_t *group_end, uint32_t max_vertices, uint32_t max_triangles, "
            "uint32_t segment_faces, crthip_meshlet_counts *out);") in hdr
    assert "int crthip_batch_bind_meshlets(crthip_batch *b, uint32_t i, const crthip_meshlet_binding *m);" in hdr
    assert "int crthip_batch_meshlet_counts(const crthip_batch *b, uint32_t i, crthip_meshlet_counts *out);" in hdr
    added = hdr[hdr.index("#define CRTHIP_ABI_VERSION"):]
    added = added[:added.index("*/")]                                                            # the "added within 6" list
    for n in names + ["crthip_meshlet,", "crthip_meshlet_counts,", "crthip_meshlet_binding,"]:
        assert n in added, n
    assert L.crthip_abi_version() == 6 and re.search(r"#define CRTHIP_ABI_VERSION 6\b", hdr)      # additive: the number stays
    assert C.sizeof(ca.Meshlet) == 16 and C.sizeof(ca.MeshletCounts) == 16 and C.sizeof(ca.MeshletBinding) == 56
    for n in ("MeshletBinding", "MeshletCounts", "meshlet_bound", "meshlet_model"):
        assert hasattr(ca, n)
    for n in ("bind_meshlets", "meshlet_counts", "meshlets"):
        assert hasattr(ca.Batch, n)


def test_the_header_is_c99_with_the_new_structs(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "corto_hip.h"\n'
                   "int use(crthip_batch *b) {\n"
                   "  crthip_meshlet_binding m = {0}; crthip_meshlet_counts c; crthip_meshlet k = {0, 0, 0, 0};\n"
                   "  m.max_vertices = 64; m.max_triangles = 124; (void)k;\n"
                   "  if(crthip_meshlet_bound(10, 0, 0, 64, 124, 0, &c)) return 1;\n"
                   "  m.meshlet_capacity = c.meshlets;\n"
                   "  return crthip_batch_bind_meshlets(b, 0, &m) + crthip_batch_meshlet_counts(b, 0, &c) + (int)sizeof(crthip_meshlet);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_and_out_of_range_arguments():
    L = ca.lib()
    m = ca.MeshletBinding()
    c = ca.MeshletCounts()
    assert L.crthip_batch_bind_meshlets(None, 0, C.byref(m)) == ml.E_ARGUMENT
    assert L.crthip_batch_bind_meshlets(None, 0, None) == ml.E_ARGUMENT
    assert L.crthip_batch_meshlet_counts(None, 0, C.byref(c)) == ml.E_ARGUMENT
    assert L.crthip_meshlet_bound(10, 0, None, 64, 124, 0, None) == ml.E_ARGUMENT
    assert L.crthip_meshlet_bound(10, 2, None, 64, 124, 0, C.byref(c)) == ml.E_ARGUMENT
    for bad in ((2, 124, 0), (256, 124, 0), (64, 0, 0), (64, 513, 0), (64, 124, 65537)):
        assert L.crthip_meshlet_bound(10, 0, None, *bad, C.byref(c)) == ml.E_ARGUMENT, bad
    for good in ((3, 1, 1), (255, 512, 65536), (64, 124, 0)):
        assert L.crthip_meshlet_bound(10, 0, None, *good, C.byref(c)) == 0, good
    assert L.crthip_meshlet_bound(2 ** 32 - 1, 0, None, 64, 124, 0, C.byref(c)) == ml.E_ARGUMENT    # (3*nface words are beyond 32 bits)


def test_the_hook_refuses_what_a_binding_would():
    idx = np.array([[0, 1, 2], [2, 1, 3]], np.uint32)
    bd = ca.meshlet_bound(2, (), 64, 124, 0)
    full = (bd.meshlets, bd.vertices, bd.triangle_bytes)
    for kw in (dict(max_vertices=2), dict(max_vertices=256), dict(max_triangles=0), dict(max_triangles=513), dict(segment_faces=65537), dict(which=2),
               dict(capacity=(full[0] - 1, full[1], full[2])), dict(capacity=(full[0], full[1] - 1, full[2])), dict(capacity=(full[0], full[1], full[2] - 1))):
        with pytest.raises(ca.CortoError):
            ca.meshlet_model(idx, (), **kw)
    assert ca.meshlet_model(idx, (), capacity=full)[3].as_tuple() == (1, 4, 8, 1)
