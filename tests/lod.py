"""Clustered levels of detail (crthip_batch_bind_lod): the sequential model of the contract in include/corto_hip.h - a dict from a cell to its
least vertex, a set of keys and a loop, written from the header's words and not from csrc/lod.h -, the properties every result has whatever the
model says, what holds across the levels of one binding, and the named inputs.  Shared by tests/test_lod_cpu.py (the kernels' source on the
host, corto_amd.lod_model) and tests/test_lod_gpu.py (the kernels).  Everything is integers: the comparison is of bytes.

Every hand-made input is a blob of this repository's encoder through meshlet_edges.encode_exact, so its positions are exact integers.  The
encoder renumbers vertices and reorders faces, so nothing here rests on the input's order: the expectation is always the model on what the
oracle decodes (Case.P, Case.index).  The COUNTS of a level do not depend on the numbering (cells are sets of positions, keys are classes of
cell triples), so they are stated as literals."""
import functools

import numpy as np

import meshlet_bounds as mb
import meshlet_edges as me
import weld as wd
from conftest import load_golden

E_ARGUMENT = -8
FILL = 0xCD
BLOB_LDS_MAX = 64 << 10                       # lod_blob's limit as csrc/lod.h states it: the bigger table, 4*T bytes, within 64 KiB


def in_blob(nvert, nface):
    return 4 * max(wd.slots(nvert), wd.slots(nface)) <= BLOB_LDS_MAX


def cells_of(P, shift):
    """a vertex's cell: floor(p / 2^shift) a coordinate (python's >> on an int is the arithmetic shift)"""
    return [tuple(int(x) >> shift for x in r) for r in np.asarray(P).reshape(-1, 3)]


def key_of(a, b, c):
    """the triple rotated so that its least id comes first, the orientation kept"""
    m = min(a, b, c)
    return (a, b, c) if a == m else (b, c, a) if b == m else (c, a, b)


def build(P, index, shift):
    """(remap uint32 (nvert,), index uint32 (3*faces,), (cells, faces, degenerate, duplicate)) of the contract, one level"""
    cells = cells_of(P, shift)
    nvert = len(cells)
    least = {}
    remap = np.zeros(nvert, np.uint32)
    for v, c in enumerate(cells):                                      # (in vertex order: the first one met is the least)
        remap[v] = least.setdefault(c, v)
    ncells = sum(1 for v in range(nvert) if remap[v] == v)
    seen = set()
    kept = []
    degenerate = duplicate = 0
    for face in np.asarray(index).reshape(-1, 3).tolist():
        a, b, c = (int(remap[i]) if i < nvert else int(i) for i in face)
        if a == b or b == c or a == c or max(a, b, c) >= nvert:
            degenerate += 1
            continue
        k = key_of(a, b, c)
        if k in seen:
            duplicate += 1
            continue
        seen.add(k)
        kept += [a, b, c]
    return remap, np.array(kept, np.uint32), (ncells, len(kept) // 3, degenerate, duplicate)


def check_properties(P, index, shift, remap, lindex, counts, tag=""):
    """what holds for every result whatever the model says; lindex: exactly the 3*faces written words"""
    P = np.asarray(P).reshape(-1, 3)
    nvert = len(P)
    flat = np.asarray(index).astype(np.int64).reshape(-1, 3)
    nface = len(flat)
    remap = np.asarray(remap)
    assert remap.dtype == np.uint32 and remap.shape == (nvert,), (tag, remap.dtype, remap.shape)
    r = remap.astype(np.int64)
    v = np.arange(nvert)
    assert (r <= v).all(), tag                                         # remap[v] <= v
    assert (r[r] == r).all(), tag                                      # idempotent
    C = P.astype(np.int64) >> shift                                    # (numpy's >> on int64 is arithmetic too)
    assert (C[r] == C).all(), tag                                      # the representative is in the cell ...
    distinct = len(np.unique(C, axis=0)) if nvert else 0
    assert len(np.unique(r)) == distinct, (tag, len(np.unique(r)), distinct)   # ... and a cell has one: share a remap iff share a cell
    cells, faces, degenerate, duplicate = (int(c) for c in counts)
    assert cells == distinct == int((r == v).sum()), (tag, counts, distinct)
    assert faces + degenerate + duplicate == nface, (tag, counts, nface)
    w = np.asarray(lindex)
    assert w.dtype == np.uint32 and w.shape == (3 * faces,), (tag, w.dtype, w.shape, faces)
    t = w.astype(np.int64).reshape(-1, 3)
    assert (t < nvert).all(), tag                                      # every index word is a vertex
    assert ((t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])).all(), tag
    keys = [key_of(*row) for row in t.tolist()]
    assert len(set(keys)) == len(keys), tag                            # no two kept faces share a key
    # the kept faces are a subsequence of the clustered faces, in order
    ok = flat < nvert
    clustered = np.where(ok, r[np.where(ok, flat, 0)] if nvert else flat, flat)
    k = 0
    rows = clustered.tolist()
    for row in t.tolist():
        while k < nface and rows[k] != row:
            k += 1
        assert k < nface, (tag, "a kept face is no clustered face in order", row)
        k += 1


def check_levels(levels, tag=""):
    """levels: [(shift, remap, counts)] in binding order - what holds from one level to the next"""
    for (s0, r0, c0), (s1, r1, c1) in zip(levels, levels[1:]):
        assert s0 < s1, tag
        r0, r1 = np.asarray(r0).astype(np.int64), np.asarray(r1).astype(np.int64)
        assert (r1 == r1[r0]).all(), (tag, s0, s1)                     # remap_k+1[v] == remap_k+1[remap_k[v]]
        assert int(c1[0]) <= int(c0[0]), (tag, "cells", c0, c1)
        assert int(c1[2]) >= int(c0[2]), (tag, "degenerate", c0, c1)


def assert_same(got, exp, tag):
    """got, exp: (remap, the written index words, counts) - counts a LodCounts or a tuple"""
    gc = got[2].as_tuple() if hasattr(got[2], "as_tuple") else tuple(int(x) for x in got[2])
    assert gc == tuple(exp[2]), (tag, gc, exp[2])
    for what, g, e in (("remap", got[0], exp[0]), ("index", got[1], exp[1])):
        g, e = np.asarray(g), np.asarray(e)
        assert g.dtype == e.dtype and g.shape == e.shape, (tag, what, g.dtype, e.dtype, g.shape, e.shape)
        if g.tobytes() != e.tobytes():
            bad = int(np.flatnonzero(g != e)[0])
            raise AssertionError("%s: %s differs from word %d on: got %s expected %s" % (tag, what, bad, g[bad], e[bad]))


# ------------------------------------------------------------------------------------------------------------------------------------
# the named inputs

STRIP_SHIFT = 4


def _strip(nface):
    """a strip of nface faces in which every second one is degenerate at STRIP_SHIFT: face A_j = (b_j, b_j+1, t_j) has its corners in three
    cells; face B_j = (t_j, b_j+1, t'_j) is a sliver whose t_j and t'_j lie in one cell"""
    P, idx = [], []
    step = 1 << STRIP_SHIFT
    na, nb = (nface + 1) // 2, nface // 2
    for j in range(na + 1):
        P.append([step * j, 0, 0])                                     # b_j: vertex j
    for j in range(na):
        P.append([step * j + 1, step, 0])                              # t_j: vertex na + 1 + 2*j
        P.append([step * j + 2, step, 0])                              # t'_j
    for j in range(na):
        t = na + 1 + 2 * j
        idx.append([j, j + 1, t])
        if j < nb:
            idx.append([t, j + 1, t + 1])
    assert len(idx) == nface
    return np.array(P), np.array(idx, np.uint32)


STRADDLE_SHIFT = 4


def _straddle():
    """vertices at -2^s, -1 and 0 on each axis in turn: -2^s and -1 are one cell, -1 and 0 never"""
    s = 1 << STRADDLE_SHIFT
    P, idx = [], []
    for axis in range(3):
        u = (axis + 1) % 3
        def at(x, y):
            p = [0, 0, 0]
            p[axis], p[u] = x, y
            return p
        n = len(P)
        P += [at(-s, 0), at(-1, 0), at(0, 0), at(s - 1, 0), at(-s, 3 * s), at(0, 3 * s), at(-1, 3 * s)]
        idx += [[n, n + 1, n + 4],          # -2^s and -1 in one cell: degenerate
                [n + 1, n + 2, n + 5],      # -1 and 0 in two cells: kept
                [n + 2, n + 3, n + 5],      # 0 and 2^s - 1 in one cell: degenerate
                [n, n + 2, n + 4],          # kept
                [n + 1, n + 2, n + 6]]      # the face above over again, by -1 for -2^s: its duplicate
    return np.array(P), np.array(idx, np.uint32)


TWICE = (64, 65)


def _twice():
    """the same grid twice, as two components: every face has its duplicate in the other one"""
    Pa, ia = mb.grid(*TWICE, 3)
    return np.concatenate([Pa, Pa]), np.concatenate([ia, ia + len(Pa)])


GRIDS = {"grid_64_64": (64, 64), "grid_17_241": (17, 241), "grid_90_91": (90, 91)}
STRIPS = {"strip_255": 255, "strip_256": 256, "strip_257": 257}

# case -> the shifts of its levels
SHIFTS = {
    "c4_unit": (0, 9, 11, 13), "confetti": (9, 11, 13), "nonmanifold_glued": (0,), "fields32": (20, 31), "fields31": (20, 31),
    "grid_64_64": (1, 2, 5), "grid_17_241": (1, 2, 5), "grid_8192": (1, 2), "grid_8193": (1, 2), "grid_90_91": (0, 2, 3), "twice": (0,),
    "strip_255": (STRIP_SHIFT,), "strip_256": (STRIP_SHIFT,), "strip_257": (STRIP_SHIFT,), "straddle": (STRADDLE_SHIFT,),
}
GOLDEN = ["c4_unit", "confetti", "nonmanifold_glued", "fields32", "fields31"]
HANDMADE = [n for n in SHIFTS if n not in GOLDEN]
NAMED = list(SHIFTS)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in GRIDS:
        return me.Case(me.encode_exact(*mb.grid(*GRIDS[name], 3)))
    if name in STRIPS:
        return me.Case(me.encode_exact(*_strip(STRIPS[name])))
    if name == "twice":
        return me.Case(me.encode_exact(*_twice()))
    if name == "straddle":
        return me.Case(me.encode_exact(*_straddle()))
    if name in wd.GRIDS:
        return wd.handmade(name)
    return me.Case(load_golden(name)["crt"])


@functools.lru_cache(maxsize=None)
def model(name, shift):
    """the model's result on a named case at one shift, computed once and never changed"""
    c = case(name)
    exp = build(c.P, c.index, shift)
    check_properties(c.P, c.index, shift, *exp, tag=(name, shift, "model"))
    return exp
