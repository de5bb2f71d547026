"""crthip_batch_bind_lod without a device: the kernels' source on the host (corto_amd.lod_model: csrc/lod.h in both of k_lod.hip's partitions,
workgroups, threads and so every atomic's order shuffled by a seed) against the sequential model of the contract (tests/lod.py), byte for byte;
the properties every result has whatever the model says; that every named case is where the table says; the insert walks; the declarations.
The bind call's errors need a device batch: tests/test_lod_gpu.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import corto_amd as ca
import lod as ld
import weld as wd
from conftest import ROOT

SEEDS = (0, 7, 12345)
E_LIMIT = -11
# the mean insert walk, in slots: the bound tests/test_weld_cpu.py holds the weld to (linear probing at a load of at most 1/2 under random
# hashing expects 2.5 for a miss; the cap allows twice that, because a lattice is not random)
MEAN_WALK_CAP = 5.0
FILL32 = ld.FILL * 0x01010101


def both_partitions(P, index, shift, tag, seeds=SEEDS):
    """the hook in both partitions equals the model; the index tail behind 3*faces words keeps the fill.  Returns the model's result"""
    exp = ld.build(P, index, shift)
    ld.check_properties(P, index, shift, *exp, tag=(tag, "model"))
    nvert, nface = len(P), len(np.asarray(index).reshape(-1, 3))
    for which in (0, 1):
        if which == 0 and not ld.in_blob(nvert, nface):
            with pytest.raises(ca.CortoError):                       # (the decode sends such a job down the other path)
                ca.lod_model(P, index, shift, which=0)
            continue
        for seed in seeds:
            remap, lindex, counts, _ = ca.lod_model(P, index, shift, which=which, seed=seed)
            assert remap.shape == (nvert,) and lindex.shape == (3 * nface,)
            written = 3 * counts.faces
            assert (lindex[written:] == FILL32).all(), (tag, which, seed, "the index tail was written")
            ld.assert_same((remap, lindex[:written], counts), exp, (tag, which, seed))
            ld.check_properties(P, index, shift, remap, lindex[:written], counts.as_tuple(), tag=(tag, which, seed))
    return exp


# ---- 1. hook equals model, the properties, the levels ----

@pytest.mark.parametrize("name", ld.NAMED)
def test_hook_equals_model(name):
    c = ld.case(name)
    levels = []
    for shift in ld.SHIFTS[name]:
        exp = both_partitions(c.P, c.index, shift, (name, shift))
        assert exp[2] == ld.model(name, shift)[2]
        levels.append((shift, exp[0], exp[2]))
    ld.check_levels(levels, name)


@pytest.mark.parametrize("name", ["c4_unit", "fields32", "straddle", "grid_17_241"])
def test_hook_equals_model_uint16_index(name):
    c = ld.case(name)
    assert c.index.max() < 65536
    for shift in ld.SHIFTS[name][-2:]:
        both_partitions(c.P, c.index.astype(np.uint16), shift, (name, shift, "u16"), seeds=(2,))


@pytest.mark.parametrize("name", ["c4_unit", "nonmanifold_glued", "grid_90_91", "twice", "fields32"])
def test_shift_0_remap_is_the_welds(name):
    c = ld.case(name)
    expect = wd.build(c.P, c.index)[0]
    for which in (0, 1):
        if which == 0 and not ld.in_blob(c.nvert, c.nface):
            continue
        remap = ca.lod_model(c.P, c.index, 0, which=which, seed=5)[0]
        assert remap.tobytes() == expect.tobytes(), (name, which)
        if wd.in_blob(c.nvert) or which == 1:
            assert remap.tobytes() == ca.weld_model(c.P, c.index, which=which, seed=5)[0].tobytes(), (name, which)


# ---- 2. every named case is where the table says ----

def counts_of(name):
    return [ld.model(name, s)[2] for s in ld.SHIFTS[name]]


def test_c4_unit():
    cs = counts_of("c4_unit")
    assert [c[0] for c in cs] == [2112, 1902, 237, 11] and [c[1] for c in cs] == [4096, 3746, 470, 14]
    c = ld.case("c4_unit")
    assert ld.in_blob(c.nvert, c.nface) and 4 * max(wd.slots(c.nvert), wd.slots(c.nface)) == 32 << 10


def test_goldens_have_a_14_bit_extent_and_negative_coordinates():
    for name in ("c4_unit", "confetti"):
        P = ld.case(name).P.astype(np.int64)
        assert P.min() < 0 and 2 ** 13 <= (P.max(axis=0) - P.min(axis=0)).max() < 2 ** 14, (name, P.min(), P.max())


def test_confetti():
    assert [c[3] for c in counts_of("confetti")] == [0, 28, 70]
    assert counts_of("confetti")[2][1] == 62 and ld.case("confetti").nface == 1315


def test_nonmanifold_glued():
    (c,) = counts_of("nonmanifold_glued")
    assert c[3] == 10 and c[1] == 822 and ld.case("nonmanifold_glued").nface == 832


def test_fields():
    for name, kept, dup in (("fields32", 54, 26), ("fields31", 53, 28)):
        at20, at31 = counts_of(name)
        assert at31[0] == 8 and at31[1] == kept and at31[3] == dup, (name, at31)    # the eight sign octants
        assert at20[0] > 8
        P = ld.case(name).P.astype(np.int64)
        assert P.min() < -2 ** 28 and P.max() > 2 ** 28
    assert ld.case("fields32").nface == 126


def test_grids():
    c = ld.case("grid_64_64")
    assert (c.nvert, c.nface) == (4225, 8192) and ld.in_blob(c.nvert, c.nface) and 4 * wd.slots(c.nface) == ld.BLOB_LDS_MAX
    assert [k[1] for k in counts_of("grid_64_64")] == [8192, 4608, 72]
    c = ld.case("grid_17_241")
    assert c.nface == 8194 and c.nvert <= 8192 and not ld.in_blob(c.nvert, c.nface)       # the first job of partition 1 by faces
    c = ld.case("grid_8192")
    assert c.nvert == 8192 and ld.in_blob(c.nvert, c.nface) and counts_of("grid_8192")[1][1] == 0     # the empty level
    assert counts_of("grid_8192")[0][1] > 0
    c = ld.case("grid_8193")
    assert c.nvert == 8193 and not ld.in_blob(c.nvert, c.nface) and counts_of("grid_8193")[1][1] == 4094
    c = ld.case("grid_90_91")
    assert (c.nvert, c.nface) == (8372, 16380) and not ld.in_blob(c.nvert, c.nface)
    assert [k[1] for k in counts_of("grid_90_91")] == [16380, 9112, 2244]


def test_twice():
    c = ld.case("twice")
    n, m = ld.TWICE
    assert c.nvert == 2 * (n + 1) * (m + 1) == 8580 and c.nface == 4 * n * m and not ld.in_blob(c.nvert, c.nface)
    (k,) = counts_of("twice")
    assert k == ((n + 1) * (m + 1), 2 * n * m, 0, 2 * n * m)                       # as many duplicates as kept faces


@pytest.mark.parametrize("name", sorted(ld.STRIPS))
def test_strips(name):
    c = ld.case(name)
    nface = ld.STRIPS[name]
    assert c.nface == nface
    (k,) = counts_of(name)
    assert k[1:] == ((nface + 1) // 2, nface // 2, 0)                            # every second face is degenerate
    assert ld.model(name, 0)[2][1:] == (nface, 0, 0)                             # ... by clustering alone


def test_straddle():
    c = ld.case("straddle")
    s = 1 << ld.STRADDLE_SHIFT
    remap = ld.model("straddle", ld.STRADDLE_SHIFT)[0]
    P = c.P.astype(np.int64)
    for axis in range(3):
        u = (axis + 1) % 3
        on = lambda x: int(np.flatnonzero((P[:, axis] == x) & (P[:, u] == 0) & (P[:, (axis + 2) % 3] == 0))[0])   # noqa: E731
        assert remap[on(-s)] == remap[on(-1)] != remap[on(0)] == remap[on(s - 1)], axis
    assert ld.model("straddle", ld.STRADDLE_SHIFT)[2][1:] == (6, 6, 3)


# ---- 3. ids at and beyond nvert ----

def test_ids_beyond_nvert_come_out_degenerate_and_are_no_address():
    c = ld.case("straddle")
    idx = c.index.copy()
    idx[1, 1] = c.nvert                                               # the first id that is no vertex
    idx[3, 0] = 0xFFFFFFFF
    idx[4] = [c.nvert + 5, c.nvert + 6, c.nvert + 7]
    base = ld.build(c.P, c.index, 0)[2]
    exp = both_partitions(c.P, idx, 0, "beyond")
    assert exp[2][2] == base[2] + 3 and (exp[1] < c.nvert).all()
    rng = np.random.default_rng(5)
    for nvert, nface, span, shift in ((40, 700, 8, 3), (300, 500, 9, 1), (9000, 300, 100, 2), (500, 9000, 64, 4)):
        P = rng.integers(-span, span + 1, (nvert, 3)).astype(np.int32)
        soup = rng.integers(0, nvert + nvert // 8 + 1, (nface, 3)).astype(np.uint32)   # (an eighth of the ids out of range)
        exp = both_partitions(P, soup, shift, ("soup", nvert), seeds=(0, 4))
        assert exp[2][0] < nvert and exp[2][2] > 0


def test_extreme_coordinates():
    """INT_MIN, INT_MAX, -1 and 0 in every component, each row twice, at shifts 0, 1 and 31"""
    vals = [-2 ** 31, 2 ** 31 - 1, -1, 0]
    rows = np.array([[x, y, z] for x in vals for y in vals for z in vals], np.int32)
    P = np.concatenate([rows, rows[::-1]])
    idx = np.arange(126, dtype=np.uint32).reshape(-1, 3)
    assert both_partitions(P, idx, 0, "extreme0")[2][0] == 64
    assert both_partitions(P, idx, 1, "extreme1")[2][0] == 64       # (-1 >> 1 == -1, 0 >> 1 == 0: still four values a component)
    assert both_partitions(P, idx, 31, "extreme31")[2][0] == 8


def test_the_arrays_end_at_their_last_word_and_empty_inputs_are_fine():
    remap, lindex, c, stats = ca.lod_model(np.zeros((0, 3), np.int32), np.zeros((0, 3), np.uint32), 3)
    assert len(remap) == 0 and len(lindex) == 0 and c.as_tuple() == (0, 0, 0, 0) and stats == (0, 0, 0, 0)
    case = ld.case("confetti")
    shift = 11
    exp = ld.model("confetti", shift)
    pos = np.ascontiguousarray(case.P, np.int32)
    for which in (0, 1):
        rr = np.full(case.nvert + 8, 0x5A5A5A5A, np.uint32)
        ri = np.full(3 * case.nface + 8, 0x5A5A5A5A, np.uint32)
        c = ca.LodCounts()
        ca._check(ca.lib().crthip_lod_model(pos.ctypes.data, case.index.ctypes.data, 0, case.nface, case.nvert, shift, rr[4:].ctypes.data, ri[4:].ctypes.data,
                                            C.byref(c), None, which, 3))
        assert (rr[:4] == 0x5A5A5A5A).all() and (rr[-4:] == 0x5A5A5A5A).all()
        assert (ri[:4] == 0x5A5A5A5A).all() and (ri[4 + 3 * c.faces:] == 0x5A5A5A5A).all()
        ld.assert_same((rr[4:-4], ri[4:4 + 3 * c.faces], c), exp, which)


# ---- 4. the insert walks ----

@pytest.mark.parametrize("name", ld.NAMED)
def test_mean_insert_walks(name):
    c = ld.case(name)
    for shift in ld.SHIFTS[name]:
        exp = ld.model(name, shift)[2]
        inserted = c.nface - exp[2]                                    # the faces that are not degenerate
        for which in (0, 1):
            if which == 0 and not ld.in_blob(c.nvert, c.nface):
                continue
            vtotal, vlongest, ftotal, flongest = ca.lod_model(c.P, c.index, shift, which=which, seed=11)[3]
            assert c.nvert <= vtotal and 1 <= vlongest <= wd.slots(c.nvert)
            assert vtotal / c.nvert <= MEAN_WALK_CAP, (name, shift, which, vtotal / c.nvert, vlongest)
            assert inserted <= ftotal and flongest <= wd.slots(c.nface)
            if inserted:
                assert ftotal / inserted <= MEAN_WALK_CAP, (name, shift, which, ftotal / inserted, flongest)


# ---- 5. declarations and arguments ----

def test_the_calls_are_exported_and_declared():
    L = ca.lib()
    names = ["crthip_batch_bind_lod", "crthip_lod_model"]
    assert all(hasattr(L, n) for n in names)
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "corto_hip.h")).read())
    assert "#define CRTHIP_LOD_MAX_LEVELS 4" in hdr
    assert "typedef struct crthip_lod_counts { uint32_t cells, faces, degenerate, duplicate; } crthip_lod_counts;" in hdr
    assert "int crthip_batch_bind_lod(crthip_batch *b, uint32_t i, const crthip_lod_binding *l);" in hdr
    added = hdr[hdr.index("#define CRTHIP_ABI_VERSION"):]
    added = added[:added.index("*/")]                                                            # the "added within 6" list
    for n in names + ["CRTHIP_LOD_MAX_LEVELS,", "crthip_lod_counts,", "crthip_lod_level,", "crthip_lod_binding,"]:
        assert n in added, n
    assert L.crthip_abi_version() == 6 and re.search(r"#define CRTHIP_ABI_VERSION 6\b", hdr)      # additive: the number stays
    assert C.sizeof(ca.LodCounts) == 16 and C.sizeof(ca.LodLevel) == 40 and C.sizeof(ca.LodBinding) == 176 and ca.LOD_MAX_LEVELS == 4
    for n in ("bind_lod", "lod"):
        assert hasattr(ca.Batch, n)


def test_the_header_is_c99_with_the_new_structs(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "corto_hip.h"\n'
                   "int use(crthip_batch *b, uint32_t *remap, uint32_t *index) {\n"
                   "  crthip_lod_binding l = {0}; crthip_lod_counts c = {0, 0, 0, 0};\n"
                   "  l.levels = 1; l.level[0].remap = remap; l.level[0].remap_capacity = 10; l.level[0].index = index; l.level[0].index_capacity = 30;\n"
                   "  l.level[0].shift = 9; (void)c; (void)sizeof(char[sizeof(crthip_lod_level) == 40 && sizeof l == 176 ? 1 : -1]);\n"
                   "  return crthip_batch_bind_lod(b, 0, &l);\n"
                   "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_and_out_of_range_arguments():
    L = ca.lib()
    b = ca.LodBinding()
    assert L.crthip_batch_bind_lod(None, 0, C.byref(b)) == ld.E_ARGUMENT
    assert L.crthip_batch_bind_lod(None, 0, None) == ld.E_ARGUMENT
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 9, 0], [0, 0, 0], [8, 0, 0]], np.int32)
    idx = np.array([[0, 1, 2], [0, 4, 2], [3, 4, 2]], np.uint32)
    remap, lindex = np.zeros(8, np.uint32), np.full(12, 77, np.uint32)
    c = ca.LodCounts()

    def call(position=P.ctypes.data, index=idx.ctypes.data, nface=3, shift=3, r=remap.ctypes.data, li=lindex.ctypes.data, counts=C.byref(c), which=0):
        return L.crthip_lod_model(position, index, 0, nface, 5, shift, r, li, counts, None, which, 0)
    assert call(which=2) == ld.E_ARGUMENT                                                        # no such partition
    assert call(position=None) == ld.E_ARGUMENT and call(index=None) == ld.E_ARGUMENT
    assert call(r=None) == ld.E_ARGUMENT and call(li=None) == ld.E_ARGUMENT
    assert call(r=remap.ctypes.data + 2) == ld.E_ARGUMENT and call(li=lindex.ctypes.data + 2) == ld.E_ARGUMENT    # 4-byte aligned
    assert call(shift=32) == ld.E_ARGUMENT and call(shift=31) == 0
    assert call(nface=2 ** 31, which=1) == ld.E_ARGUMENT                                         # 3*nface words are beyond 32 bits
    assert call(counts=None) == 0                                                                # (the record is optional)
    for which in (0, 1):
        lindex[:] = 77
        # cells at shift 3: {0, 1, 3} | {2} | {4}; face 0 is degenerate, face 1 is kept, face 2 is its duplicate
        assert call(which=which) == 0 and c.as_tuple() == (3, 1, 1, 1) and remap[:5].tolist() == [0, 0, 2, 0, 4]
        assert lindex.tolist() == [0, 4, 2] + [77] * 9
    # partition 0 is lod_blob's: a job beyond its LDS is the other partition's
    for name in ("grid_8193", "grid_17_241"):
        big = ld.case(name)
        pos = np.ascontiguousarray(big.P, np.int32)
        out, outi = np.zeros(big.nvert, np.uint32), np.zeros(3 * big.nface, np.uint32)
        assert L.crthip_lod_model(pos.ctypes.data, big.index.ctypes.data, 0, big.nface, big.nvert, 1, out.ctypes.data, outi.ctypes.data, C.byref(c), None, 0, 0) == E_LIMIT
