"""crthip_batch_bind_adjacency without a device: the kernels' source on the host (corto_amd.adjacency_model: csrc/adjacency.h in both of
k_adjacency.hip's partitions, workgroups, threads and so every atomic's order shuffled by a seed) against the sequential model of the contract
(tests/adjacency.py), byte for byte; the properties every result has whatever the model says; the declarations."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import adjacency as adj
import corto_amd as ca
from conftest import MESH_CASES, ROOT
from corto_amd import synth

SEEDS = (0, 1, 7, 12345)
E_LIMIT = -11


def both_partitions(index, nvert, tag, seeds=SEEDS):
    exp = adj.build(index, nvert)
    adj.check_properties(index, nvert, *exp, tag=(tag, "model"))
    for which in (0, 1):
        if which == 0 and not adj.in_blob(nvert, len(index)):
            with pytest.raises(ca.CortoError):                       # (the decode sends such a blob down the other path)
                ca.adjacency_model(index, nvert, which=0)
            continue
        for seed in seeds:
            got = ca.adjacency_model(index, nvert, which=which, seed=seed)
            adj.assert_same(got, exp, (tag, which, seed))
            adj.check_properties(index, nvert, got[0], got[1].as_tuple(), tag=(tag, which, seed))
    return exp


# ---- 1. hook equals model ----

@pytest.mark.parametrize("name", MESH_CASES)
def test_hook_equals_model(name):
    idx, nvert, _ = adj.golden(name)
    both_partitions(idx, nvert, name)


@pytest.mark.parametrize("name", MESH_CASES)
def test_hook_equals_model_uint16_index(name):
    idx, nvert, _ = adj.golden(name)
    assert idx.max() < 65536
    both_partitions(idx.astype(np.uint16), nvert, name)


@pytest.mark.parametrize("name", ["closed_sphere", "torus", "icosphere"])
def test_closed_manifolds(name):
    """(verified from the reference decoder's index of the three fixtures: all of them are closed and oriented)"""
    idx, nvert, _ = adj.golden(name)
    for which in (0, 1):
        twin, c = ca.adjacency_model(idx, nvert, which=which, seed=3)
        assert c.as_tuple() == (3 * len(idx), 0, 0, 0), (name, c.as_tuple())
        assert (twin[twin] == np.arange(len(twin))).all()


def test_a_disc_with_holes_has_a_border():
    idx, nvert, _ = adj.golden("holey_disc")
    c = ca.adjacency_model(idx, nvert, which=1)[1]
    assert c.boundary > 0 and c.duplicate == 0 and c.invalid == 0


def test_confetti_of_lone_faces_is_all_border():
    m = synth.confetti(40, seed=2, max_faces=1)
    idx = np.ascontiguousarray(m.index, np.uint32).reshape(-1, 3)
    assert len(idx) > 0
    for which in (0, 1):
        twin, c = ca.adjacency_model(idx, m.nvert, which=which, seed=5)
        assert (twin == adj.NO_TWIN).all() and c.as_tuple() == (3 * len(idx), 3 * len(idx), 0, 0)
    both_partitions(idx, m.nvert, "confetti_1")


@pytest.mark.parametrize("name", sorted(adj.handmade()))
def test_handmade_indices(name):
    idx, nvert = adj.handmade()[name]
    both_partitions(idx, nvert, name)
    if idx.max() < 65536:
        both_partitions(idx.astype(np.uint16), nvert, name, seeds=(2, 9, 31, 77))


def test_handmade_values():
    h = adj.handmade()
    N = adj.NO_TWIN
    twin, c = ca.adjacency_model(*h["one_face"])
    assert twin.tolist() == [N, N, N] and c.as_tuple() == (3, 3, 0, 0)
    twin, c = ca.adjacency_model(*h["two_faces_consistent"])                      # 1 -> 2 (half-edge 1) against 2 -> 1 (half-edge 3)
    assert twin.tolist() == [N, 3, N, 1, N, N] and c.as_tuple() == (6, 4, 0, 0)
    twin, c = ca.adjacency_model(*h["two_faces_same_direction"])                  # 1 -> 2 is half-edge 1 and half-edge 3
    assert twin.tolist() == [N] * 6 and c.as_tuple() == (6, 6, 1, 0)
    twin, c = ca.adjacency_model(*h["same_face_twice"])
    assert twin.tolist() == [N] * 6 and c.as_tuple() == (6, 6, 3, 0)
    twin, c = ca.adjacency_model(*h["face_and_mirror"])                           # (0 1 2) and (2 1 0): 0->1 / 1->0 = 4, 1->2 / 2->1 = 3, 2->0 / 0->2 = 5
    assert twin.tolist() == [4, 3, 5, 1, 0, 2] and c.as_tuple() == (6, 0, 0, 0)
    idx, nvert = h["degenerate_and_out_of_range"]
    twin, c = ca.adjacency_model(idx, nvert, which=1)
    assert c.invalid == 12 and (twin.reshape(-1, 3)[[1, 3, 5, 6]] == N).all()
    assert twin[1] == 6 and twin[6] == 1                                          # 1 -> 2 of face 0 and 2 -> 1 of face 2, across the invalid face between
    for closed in (True, False):
        idx, nvert = h["fan_300_closed" if closed else "fan_300_open"]
        c = ca.adjacency_model(idx, nvert, which=0, seed=1)[1]
        assert c.as_tuple() == (900, 300 if closed else 302, 0, 0)


def test_the_least_of_several_candidates_wins():
    """three fins on one edge: 0 -> 1 once, 1 -> 0 three times"""
    idx = np.array([[1, 0, 4], [0, 1, 2], [1, 0, 3], [1, 0, 5]], np.uint32)
    for which in (0, 1):
        for seed in SEEDS:
            twin, c = ca.adjacency_model(idx, 6, which=which, seed=seed)
            assert twin[3] == 0 and twin[0] == 3 and twin[6] == 3 and twin[9] == 3 and c.duplicate == 2


def test_random_soups():
    for seed, (nface, nvert) in enumerate([(700, 40), (500, 100000), (300, 9), (2000, 300)]):
        idx = np.random.default_rng(seed).integers(0, nvert + nvert // 8 + 1, (nface, 3)).astype(np.uint32)    # (an eighth of the ids out of range)
        both_partitions(idx, nvert, ("soup", seed), seeds=(0, 4))


def test_the_twin_array_ends_at_its_last_word_and_no_faces_are_fine():
    twin, c = ca.adjacency_model(np.zeros((0, 3), np.uint32), 7)
    assert len(twin) == 0 and c.as_tuple() == (0, 0, 0, 0)
    idx, nvert, _ = adj.golden("group_props")
    raw = np.full(3 * len(idx) + 8, 0x5A5A5A5A, np.uint32)
    for which in (0, 1):
        c = ca.AdjacencyCounts()
        ca._check(ca.lib().crthip_adjacency_model(idx.ctypes.data, 0, len(idx), nvert, raw[4:].ctypes.data, C.byref(c), which, 3))
        assert (raw[:4] == 0x5A5A5A5A).all() and (raw[-4:] == 0x5A5A5A5A).all()
        adj.assert_same((raw[4:-4], c), adj.build(idx, nvert), which)


def test_the_gl_triangles_adjacency_recipe():
    idx, nvert = adj.handmade()["two_faces_consistent"]
    twin, _ = ca.adjacency_model(idx, nvert)
    assert adj.gl_triangles_adjacency(idx, twin).tolist() == [[0, 0, 1, 3, 2, 2], [2, 0, 1, 1, 3, 3]]


# ---- 2. declarations and arguments ----

def test_the_calls_are_exported_and_declared():
    L = ca.lib()
    names = ["crthip_batch_bind_adjacency", "crthip_adjacency_model"]
    assert all(hasattr(L, n) for n in names)
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "corto_hip.h")).read())
    assert "#define CRTHIP_NO_TWIN 0xFFFFFFFFu" in hdr
    assert "typedef struct crthip_adjacency_counts { uint32_t halfedges, boundary, duplicate, invalid; } crthip_adjacency_counts;" in hdr
    assert "int crthip_batch_bind_adjacency(crthip_batch *b, uint32_t i, const crthip_adjacency_binding *a);" in hdr
    added = hdr[hdr.index("#define CRTHIP_ABI_VERSION"):]
    added = added[:added.index("*/")]                                                            # the "added within 6" list
    for n in names + ["CRTHIP_NO_TWIN,", "crthip_adjacency_counts,", "crthip_adjacency_binding,"]:
        assert n in added, n
    assert L.crthip_abi_version() == 6 and re.search(r"#define CRTHIP_ABI_VERSION 6\b", hdr)      # additive: the number stays
    assert C.sizeof(ca.AdjacencyCounts) == 16 and C.sizeof(ca.AdjacencyBinding) == 24 and ca.NO_TWIN == 0xFFFFFFFF
    for n in ("bind_adjacency", "adjacency"):
        assert hasattr(ca.Batch, n)


def test_the_header_is_c99_with_the_new_structs(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "corto_hip.h"\n'
                   "int use(crthip_batch *b, uint32_t *twin) {\n"
                   "  crthip_adjacency_binding a = {0}; crthip_adjacency_counts c = {0, 0, 0, 0};\n"
                   "  a.twin = twin; a.capacity = 30; (void)c;\n"
                   "  return crthip_batch_bind_adjacency(b, 0, &a) + (twin[0] == CRTHIP_NO_TWIN);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_and_out_of_range_arguments():
    L = ca.lib()
    a = ca.AdjacencyBinding()
    assert L.crthip_batch_bind_adjacency(None, 0, C.byref(a)) == adj.E_ARGUMENT
    assert L.crthip_batch_bind_adjacency(None, 0, None) == adj.E_ARGUMENT
    idx = np.array([[0, 1, 2], [2, 1, 3]], np.uint32)
    twin = np.zeros(8, np.uint32)
    c = ca.AdjacencyCounts()
    assert L.crthip_adjacency_model(idx.ctypes.data, 0, 2, 4, twin.ctypes.data, C.byref(c), 2, 0) == adj.E_ARGUMENT        # no such partition
    assert L.crthip_adjacency_model(None, 0, 2, 4, twin.ctypes.data, C.byref(c), 0, 0) == adj.E_ARGUMENT
    assert L.crthip_adjacency_model(idx.ctypes.data, 0, 2, 4, None, C.byref(c), 0, 0) == adj.E_ARGUMENT
    assert L.crthip_adjacency_model(idx.ctypes.data, 0, 2, 4, twin.ctypes.data + 2, C.byref(c), 0, 0) == adj.E_ARGUMENT    # twin is 4-byte aligned
    assert L.crthip_adjacency_model(idx.ctypes.data, 0, 2 ** 31, 4, twin.ctypes.data, C.byref(c), 1, 0) == adj.E_ARGUMENT  # 3*nface words are beyond 32 bits
    assert L.crthip_adjacency_model(idx.ctypes.data, 0, 2, 4, twin.ctypes.data, None, 0, 0) == 0                            # (the record is optional)
    # partition 0 is adjacency_blob's: a blob beyond its LDS is the other partition's
    big, nv = adj.strip(21846, 21848)                                                                                          # 3*nface = 65 538
    assert not adj.in_blob(nv, len(big))
    out = np.zeros(3 * len(big), np.uint32)
    assert L.crthip_adjacency_model(big.ctypes.data, 0, len(big), nv, out.ctypes.data, C.byref(c), 0, 0) == E_LIMIT
    adj.assert_same(ca.adjacency_model(big, nv, which=1, seed=2), adj.build(big, nv), "past 16 bits of half-edges")
