"""crthip_batch_bind_weld without a device: the kernels' source on the host (corto_amd.weld_model: csrc/weld.h in both of k_weld.hip's partitions,
workgroups, threads and so every atomic's order shuffled by a seed) against the sequential model of the contract (tests/weld.py), byte for
byte; the properties every result has whatever the model says; that every hand-made case is where it is named; the insert walks; the
declarations.  The bind call's errors need a device batch: tests/test_weld_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import corto_amd as ca
import weld as wd
from conftest import MESH_CASES, ROOT

SEEDS = (0, 1, 7, 12345)
E_LIMIT = -11
# the mean insert walk, in slots: linear probing at a load of at most 1/2 under random hashing expects 2.5 for a miss; the cap allows twice
# that, because a lattice is not random.  A case beyond it: the mix (csrc/weld.h: weld_hash) is the thing to fix, not the cap
MEAN_WALK_CAP = 5.0


def both_partitions(P, index, tag, seeds=SEEDS, with_index=True):
    exp = wd.build(P, index, with_index)
    wd.check_properties(P, index, *exp, tag=(tag, "model"))
    for which in (0, 1):
        if which == 0 and not wd.in_blob(len(P)):
            with pytest.raises(ca.CortoError):                       # (the decode sends such a blob down the other path)
                ca.weld_model(P, index, which=0)
            continue
        for seed in seeds:
            got = ca.weld_model(P, index, which=which, seed=seed, with_index=with_index)
            wd.assert_same(got[:3], exp, (tag, which, seed))
            wd.check_properties(P, index, got[0], got[1], got[2].as_tuple(), tag=(tag, which, seed))
    return exp


# ---- 1. hook equals model ----

@pytest.mark.parametrize("name", MESH_CASES + wd.HANDMADE)
def test_hook_equals_model(name):
    c = wd.case(name)
    both_partitions(c.P, c.index, name)


@pytest.mark.parametrize("name", ["c4_unit", "fields32", "cube24", "seam", "coincident", "grid_8193"])
def test_hook_equals_model_uint16_index_and_no_index(name):
    c = wd.case(name)
    assert c.index.max() < 65536
    both_partitions(c.P, c.index.astype(np.uint16), name, seeds=(2, 9))
    both_partitions(c.P, c.index, name, seeds=(3,), with_index=False)


# ---- 2. every hand-made case is where it is named ----

def test_cube24():
    c = wd.handmade("cube24")
    assert (c.nvert, c.nface) == (24, 12) and wd.multiplicities(c.P) == [3] * 8
    assert wd.model("cube24")[2] == (24, 8, 0, 0)


def test_seam():
    c = wd.handmade("seam")
    n, m = wd.SEAM
    per = (n + 1) * (m + 1)
    assert c.nvert == 2 * per and wd.multiplicities(c.P) == [1] * (2 * per - 2 * (m + 1)) + [2] * (m + 1)
    assert wd.model("seam")[2] == (2 * per, 2 * per - (m + 1), 0, 0)


def test_coincident():
    c = wd.handmade("coincident")
    assert c.nvert > 64 and wd.multiplicities(c.P) == [c.nvert]      # (the encoder keeps such vertices)
    remap, windex, counts = wd.model("coincident")
    assert not remap.any() and not windex.any() and counts == (c.nvert, 1, c.nface, 0)


def test_far_pairs():
    c = wd.handmade("far_pairs")
    per = (wd.FAR[0] + 1) * (wd.FAR[1] + 1)
    assert c.nvert == 2 * per and wd.multiplicities(c.P) == [2] * per
    remap = wd.model("far_pairs")[0].astype(np.int64)
    far = np.arange(c.nvert) - remap
    assert wd.model("far_pairs")[2] == (2 * per, per, 0, 0)
    assert far[far > 0].min() > 256                                    # every pair lies in two workgroups of weld_insert / weld_lookup


@pytest.mark.parametrize("name", sorted(wd.GRIDS))
def test_grids(name):
    c = wd.handmade(name)
    assert c.nvert == wd.GRID_NVERT[name] and wd.slots(c.nvert) == wd.GRID_SLOTS[name]
    assert wd.multiplicities(c.P) == [1] * c.nvert and wd.model(name)[2] == (c.nvert, c.nvert, 0, 0)
    assert (wd.model(name)[0] == np.arange(c.nvert)).all() and (wd.model(name)[1] == c.index.reshape(-1)).all()   # the identity
    assert wd.in_blob(c.nvert) == (name != "grid_8193")
    if name == "grid_512":
        assert 2 * c.nvert == wd.slots(c.nvert)
    if name == "grid_8192":
        assert 4 * wd.slots(c.nvert) == wd.BLOB_LDS_MAX


def test_every_non_grid_case_welds_something():
    for name in wd.NON_GRID:
        c = wd.handmade(name)
        assert wd.model(name)[2][1] < c.nvert, name


def test_the_wide_fixtures_reach_the_sign_bit():
    for name in wd.GOLDEN_WIDE:
        P = wd.golden(name).P.astype(np.int64)
        assert P.min() < -2 ** 28 and P.max() > 2 ** 28, (name, P.min(), P.max())
    P = wd.golden("fields32").P.astype(np.int64)
    assert P.min() < -2 ** 30 and P.max() >= 2 ** 30


def test_slots():
    assert [wd.slots(n) for n in (0, 1, 32, 33, 512, 513, 8192, 8193)] == [64, 64, 64, 128, 1024, 2048, 16384, 32768]


# ---- 3. ids at and beyond nvert, synthetic positions ----

def test_ids_beyond_nvert_pass_through_and_count_as_degenerate():
    c = wd.handmade("seam")
    idx = c.index.copy()
    idx[3, 1] = c.nvert                                               # the first id that is no vertex
    idx[10, 0] = 0xFFFFFFFF
    idx[20] = [c.nvert + 5, c.nvert + 6, c.nvert + 7]
    exp = both_partitions(c.P, idx, "beyond")
    assert exp[2][2] == 3 and exp[1][3 * 3 + 1] == c.nvert and exp[1][30] == 0xFFFFFFFF and exp[1][60:63].tolist() == [c.nvert + 5, c.nvert + 6, c.nvert + 7]
    rng = np.random.default_rng(5)
    for nvert, nface, span in ((40, 700, 1), (300, 500, 2), (9000, 300, 8)):              # 27, 125 and 4 913 rows to draw from
        P = rng.integers(-span, span + 1, (nvert, 3)).astype(np.int32)            # heavy coincidence: few distinct rows
        soup = rng.integers(0, nvert + nvert // 8 + 1, (nface, 3)).astype(np.uint32)   # (an eighth of the ids out of range)
        exp = both_partitions(P, soup, ("soup", nvert), seeds=(0, 4))
        assert exp[2][1] < nvert and exp[2][2] > 0


def test_extreme_coordinates():
    """INT_MIN, INT_MAX, -1 and 0 in every component, each row twice"""
    vals = [-2 ** 31, 2 ** 31 - 1, -1, 0]
    rows = np.array([[x, y, z] for x in vals for y in vals for z in vals], np.int32)
    P = np.concatenate([rows, rows[::-1]])
    idx = np.arange(126, dtype=np.uint32).reshape(-1, 3)
    exp = both_partitions(P, idx, "extreme")
    assert exp[2][1] == 64 and (exp[0][64:] == np.arange(64)[::-1]).all()


def test_the_arrays_end_at_their_last_word_and_empty_inputs_are_fine():
    remap, windex, c, stats = ca.weld_model(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint32))
    assert len(remap) == 0 and len(windex) == 0 and c.as_tuple() == (0, 0, 0, 0) and stats == (0, 0)
    case = wd.golden("group_props")
    exp = wd.model("group_props")
    pos = np.ascontiguousarray(case.P, np.int32)
    for which in (0, 1):
        rr = np.full(case.nvert + 8, 0x5A5A5A5A, np.uint32)
        ri = np.full(3 * case.nface + 8, 0x5A5A5A5A, np.uint32)
        c = ca.WeldCounts()
        ca._check(ca.lib().crthip_weld_model(pos.ctypes.data, case.index.ctypes.data, 0, case.nface, case.nvert, rr[4:].ctypes.data, ri[4:].ctypes.data,
                                             C.byref(c), None, which, 3))
        for raw in (rr, ri):
            assert (raw[:4] == 0x5A5A5A5A).all() and (raw[-4:] == 0x5A5A5A5A).all()
        wd.assert_same((rr[4:-4], ri[4:-4], c), exp, which)


# ---- 4. the insert walks ----

@pytest.mark.parametrize("name", MESH_CASES + wd.LATTICES)
def test_mean_insert_walk(name):
    c = wd.case(name)
    for which in (0, 1):
        if which == 0 and not wd.in_blob(c.nvert):
            continue
        total, longest = ca.weld_model(c.P, c.index, which=which, seed=11)[3]
        assert c.nvert <= total and 1 <= longest <= wd.slots(c.nvert)
        assert total / c.nvert <= MEAN_WALK_CAP, (name, which, total / c.nvert, longest)


# ---- 5. declarations and arguments ----

def test_the_calls_are_exported_and_declared():
    L = ca.lib()
    names = ["crthip_batch_bind_weld", "crthip_weld_model"]
    assert all(hasattr(L, n) for n in names)
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "corto_hip.h")).read())
    assert "#define CRTHIP_WELD_ADJACENCY 1u" in hdr
    assert "typedef struct crthip_weld_counts { uint32_t vertices, unique, degenerate, reserved; } crthip_weld_counts;" in hdr
    assert "int crthip_batch_bind_weld(crthip_batch *b, uint32_t i, const crthip_weld_binding *w);" in hdr
    added = hdr[hdr.index("#define CRTHIP_ABI_VERSION"):]
    added = added[:added.index("*/")]                                                            # the "added within 6" list
    for n in names + ["CRTHIP_WELD_ADJACENCY,", "crthip_weld_counts,", "crthip_weld_binding,"]:
        assert n in added, n
    assert L.crthip_abi_version() == 6 and re.search(r"#define CRTHIP_ABI_VERSION 6\b", hdr)      # additive: the number stays
    assert C.sizeof(ca.WeldCounts) == 16 and C.sizeof(ca.WeldBinding) == 40 and ca.WELD_ADJACENCY == 1
    for n in ("bind_weld", "weld"):
        assert hasattr(ca.Batch, n)


def test_the_header_is_c99_with_the_new_structs(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "corto_hip.h"\n'
                   "int use(crthip_batch *b, uint32_t *remap, uint32_t *index) {\n"
                   "  crthip_weld_binding w = {0}; crthip_weld_counts c = {0, 0, 0, 0};\n"
                   "  w.remap = remap; w.remap_capacity = 10; w.index = index; w.index_capacity = 30; w.flags = CRTHIP_WELD_ADJACENCY; (void)c;\n"
                   "  return crthip_batch_bind_weld(b, 0, &w);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_and_out_of_range_arguments():
    L = ca.lib()
    w = ca.WeldBinding()
    assert L.crthip_batch_bind_weld(None, 0, C.byref(w)) == wd.E_ARGUMENT
    assert L.crthip_batch_bind_weld(None, 0, None) == wd.E_ARGUMENT
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 0]], np.int32)
    idx = np.array([[0, 1, 2], [0, 1, 3]], np.uint32)                                            # (the second face collapses: 3 is 0)
    remap, windex = np.zeros(8, np.uint32), np.zeros(8, np.uint32)
    c = ca.WeldCounts()

    def call(position=P.ctypes.data, index=idx.ctypes.data, nface=2, r=remap.ctypes.data, wi=windex.ctypes.data, counts=C.byref(c), which=0):
        return L.crthip_weld_model(position, index, 0, nface, 4, r, wi, counts, None, which, 0)
    assert call(which=2) == wd.E_ARGUMENT                                                        # no such partition
    assert call(position=None) == wd.E_ARGUMENT and call(index=None) == wd.E_ARGUMENT and call(r=None) == wd.E_ARGUMENT
    assert call(r=remap.ctypes.data + 2) == wd.E_ARGUMENT and call(wi=windex.ctypes.data + 2) == wd.E_ARGUMENT    # 4-byte aligned
    assert call(nface=2 ** 31, which=1) == wd.E_ARGUMENT                                         # 3*nface words are beyond 32 bits
    assert call(counts=None) == 0 and call(wi=None) == 0                                         # (the record and the welded index are optional)
    assert call() == 0 and c.as_tuple() == (4, 3, 1, 0) and remap[:4].tolist() == [0, 1, 2, 0] and windex[:6].tolist() == [0, 1, 2, 0, 1, 0]
    assert call(wi=None) == 0 and c.as_tuple() == (4, 3, 0, 0)                                   # without a welded index no face is looked at
    # partition 0 is weld_blob's: a blob beyond its LDS is the other partition's
    big = wd.handmade("grid_8193")
    pos = np.ascontiguousarray(big.P, np.int32)
    out, outi = np.zeros(big.nvert, np.uint32), np.zeros(3 * big.nface, np.uint32)
    assert L.crthip_weld_model(pos.ctypes.data, big.index.ctypes.data, 0, big.nface, big.nvert, out.ctypes.data, outi.ctypes.data, C.byref(c), None, 0, 0) == E_LIMIT
