"""crthip_batch_bind_bvh without a device: the kernels' source on the host (corto_amd.bvh_model: csrc/bvh.h in both of k_bvh.hip's partitions,
workgroups, threads and so every atomic and every arrival shuffled by a seed) against the sequential model of the contract (tests/bvh.py), byte
for byte; the properties every result has whatever the model says; the hand-made cases of the contract's edges; the partition limit and the
sort tile's ends.  The bind call's errors need a device batch: tests/test_bvh_gpu.py."""
import functools

import numpy as np
import pytest

import corto_amd as ca
import bvh
import meshlet_edges as me
from conftest import load_golden

SEEDS = (0, 7, 12345)
BLOB_FACES = 4096                                           # bvh_blob's limit as csrc/bvh.h states it
TILE = 2048                                                 # the bigger partition's sort tile
I32_MIN, I32_MAX = -2**31, 2**31 - 1


def both_partitions(pos, idx, tag, seeds=SEEDS):
    """the hook in both partitions equals the model, under every seed.  Returns the model's result"""
    exp = bvh.build(pos, idx)
    bvh.check(pos, idx, exp[0], exp[1], exp[2], exp[3])
    for which in (0, 1):
        if which == 0 and len(idx) > BLOB_FACES:
            with pytest.raises(ca.CortoError):                       # (the decode sends such a blob down the other path)
                ca.bvh_model(pos, idx, which=0)
            continue
        for seed in seeds:
            nodes, parent, order, counts = ca.bvh_model(pos, idx, which=which, seed=seed)
            assert counts.as_tuple() == exp[3], (tag, which, seed, counts.as_tuple(), exp[3])
            assert order.tobytes() == exp[2].tobytes(), (tag, which, seed, "order")
            assert parent.tobytes() == exp[1].tobytes(), (tag, which, seed, "parent")
            if nodes.tobytes() != exp[0].tobytes():
                bad = int(np.flatnonzero(nodes != exp[0])[0])
                raise AssertionError("%s: node %d differs: got %s expected %s" % ((tag, which, seed), bad, nodes[bad], exp[0][bad]))
            bvh.check(pos, idx, nodes, parent, order, counts.as_tuple())
    return exp


def points(mids):
    """a face a mid, all three corners at it (equal corners: an ordinary face): (position, index)"""
    pos = np.array(mids, np.int64).reshape(-1, 3).astype(np.int32)
    v = np.arange(len(pos), dtype=np.uint32)
    return pos, np.stack([v, v, v], axis=1)


# ---- 1. the smallest trees ----

@pytest.mark.parametrize("F", [1, 2, 3])
def test_smallest(F):
    pos, idx = bvh.strip(F, seed=F)
    exp = both_partitions(pos, idx, ("strip", F))
    assert exp[3] == (2 * F - 1, F, 0, (0, 1, 2)[F - 1])
    if F == 1:
        assert exp[0][0]["right"] == bvh.LEAF and exp[0][0]["left"] == 0 and exp[1][0] == bvh.NO_NODE


def test_one_cell_ties_go_by_id():
    """every face has the same box: one key, the order is the face order and the tree is the one over the bits of j"""
    F = 37
    pos = np.array([[5, -3, 9], [6, -3, 9], [5, -2, 9]], np.int32)
    idx = np.tile(np.array([[0, 1, 2]], np.uint32), (F, 1))
    exp = both_partitions(pos, idx, "one_cell")
    assert len(set(exp[4])) == 1 and (exp[2] == np.arange(F)).all()
    # the root splits [0, 36] where bit 5 of j changes: clz64(0 ^ 36) = 58, the largest m with clz64(m) > 58 is 31
    assert exp[0][0]["left"] == 31 and exp[0][0]["right"] == 32
    assert exp[3][3] == 6                                            # 37 leaves by the bits of j: six edges


def test_four_distinct_keys():
    mids = [(0, 0, 0)] * 5 + [(1023, 0, 0)] * 3 + [(0, 1023, 0)] * 4 + [(0, 0, 1023)] * 2
    pos, idx = points(mids)
    rng = np.random.default_rng(1)
    p = rng.permutation(len(idx))
    exp = both_partitions(pos, idx[p], "four_keys")
    assert len(set(exp[4])) == 4


def test_negative_coordinates():
    pos, idx = bvh.lattice(6, step=11)
    pos = pos - np.array([100000, 70000, 30], np.int32)
    assert (pos < 0).all()
    both_partitions(pos, idx, "negative")


@pytest.mark.parametrize("extent,k", [(1023, 0), (1024, 1)])
def test_extent_at_the_shift(extent, k):
    pos, idx = points([(-7, 3, 3), (-7 + extent, 3, 3), (-7 + extent // 2, 3, 3), (-6, 3, 3)])
    exp = both_partitions(pos, idx, ("extent", extent))
    cell = extent >> k                                               # the far face's cell on x: bit i of cell[0] at bit 3i + 2
    assert exp[4][1] == sum(((cell >> i) & 1) << (3 * i + 2) for i in range(10))
    assert exp[4][3] == ((1 >> k) << 2)                              # one step from L: a cell of its own at k = 0, L's cell at k = 1


def test_extent_of_all_32_bits():
    pos = np.array([[I32_MIN, I32_MIN, I32_MIN], [I32_MAX, I32_MAX, I32_MAX], [0, -1, I32_MAX], [I32_MIN, 0, 1]], np.int32)
    idx = np.array([[0, 0, 0], [1, 1, 1], [0, 1, 2], [2, 3, 3], [3, 0, 1], [1, 1, 0]], np.uint32)
    exp = both_partitions(pos, idx, "extent32")
    assert exp[4][0] == 0 and exp[4][1] == (1 << 30) - 1             # k = 22: the two ends are cells 0 and 1023 on every axis
    assert tuple(exp[0][0]["min"]) == (I32_MIN,) * 3 and tuple(exp[0][0]["max"]) == (I32_MAX,) * 3


def test_one_present_among_absent():
    pos, idx = bvh.strip(9, seed=3)
    idx = idx.copy()
    nv = len(pos)
    for f in range(9):
        if f != 4:
            idx[f, f % 3] = nv + f                                   # (an id >= nvert: compared, never an address)
    idx[7] = 0xFFFFFFFF
    exp = both_partitions(pos, idx, "one_present")
    assert exp[3][2] == 8 and exp[2][0] == 4 and exp[4][4] == 0      # the present face comes first; alone, its key is 0
    assert tuple(exp[0][0]["min"]) == tuple(pos[4:7].min(axis=0))    # the root's box is that face's: the empty box is the union's identity


def test_all_absent():
    pos, idx = bvh.strip(6, seed=4)
    exp = both_partitions(pos, idx + np.uint32(len(pos)), "all_absent")
    assert exp[3][2] == 6 and (exp[2] == np.arange(6)).all()
    for n in exp[0]:
        assert tuple(n["min"]) == (I32_MAX,) * 3 and tuple(n["max"]) == (I32_MIN,) * 3


def test_no_vertices_at_all():
    exp = both_partitions(np.zeros((0, 3), np.int32), np.zeros((3, 3), np.uint32), "no_vertices")
    assert exp[3] == (5, 3, 3, 2)


def test_equal_corners():
    pos, idx = bvh.strip(12, seed=5)
    idx = idx.copy()
    idx[3, 1] = idx[3, 0]
    idx[8] = idx[8, 0]
    exp = both_partitions(pos, idx, "equal_corners")
    assert exp[3][2] == 0


def test_uint16_index():
    pos, idx = bvh.lattice(9)
    exp = both_partitions(pos, idx.astype(np.uint16), "u16", seeds=(3,))
    nodes, parent, order, counts = ca.bvh_model(pos, idx, which=0, seed=3)      # (uint32: the same bytes)
    assert nodes.tobytes() == exp[0].tobytes() and order.tobytes() == exp[2].tobytes()
    bad = idx.astype(np.uint16)
    bad[5, 2] = 0xFFFF                                               # (the uint16 id that is >= nvert)
    assert both_partitions(pos, bad, "u16_absent", seeds=(3,))[3][2] == 1


def test_optional_arrays_change_nothing():
    pos, idx = bvh.strip(300, seed=6)
    exp = bvh.build(pos, idx)
    for which in (0, 1):
        nodes, parent, order, counts = ca.bvh_model(pos, idx, which=which, seed=1, with_parent=False, with_order=False)
        assert parent is None and order is None
        assert nodes.tobytes() == exp[0].tobytes() and counts.as_tuple() == exp[3]


# ---- 2. meshes ----

@functools.lru_cache(maxsize=None)
def golden():
    c = me.Case(load_golden("c4_unit")["crt"])
    return c.P, c.index


@pytest.mark.parametrize("name", ["lattice", "disc", "golden"])
def test_meshes(name):
    pos, idx = {"lattice": lambda: bvh.lattice(24), "disc": lambda: bvh.disc(700, seed=2), "golden": golden}[name]()
    exp = both_partitions(pos, idx, name, seeds=(0, 9))
    assert exp[3][2] == 0 and exp[3][3] <= 64


# ---- 3. the partition limit and the sort tile's ends ----

@pytest.mark.parametrize("F", [BLOB_FACES - 1, BLOB_FACES, BLOB_FACES + 1])
def test_partition_limit(F):
    pos, idx = bvh.strip(F, seed=F)
    both_partitions(pos, idx, ("limit", F), seeds=(2,))              # (which 0 refuses 4 097 faces)


@pytest.mark.parametrize("F", [TILE - 1, TILE, TILE + 1])
def test_sort_tile_ends(F):
    pos, idx = bvh.strip(F, seed=F, spread=40)                       # (few cells: long runs of equal keys across the tile's end)
    both_partitions(pos, idx, ("tile", F), seeds=(4,))


def test_hook_arguments():
    pos, idx = bvh.strip(3)
    with pytest.raises(ca.CortoError):
        ca.bvh_model(pos, idx, which=2)
    with pytest.raises(ca.CortoError):
        ca.bvh_model(pos, np.zeros((0, 3), np.uint32))
