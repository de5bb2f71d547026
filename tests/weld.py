"""The weld (crthip_batch_bind_weld): the sequential model of the contract in include/corto_hip.h - a dict from a position triple to its least
vertex and a loop, written from the header's words and not from csrc/weld.h -, the properties every result has whatever the model says, and
the named inputs.  Shared by tests/test_weld_cpu.py (the kernels' source on the host, corto_amd.weld_model) and tests/test_weld_gpu.py (the
kernels).  Everything is integers: the comparison is of bytes.

Every hand-made input is a blob of this repository's encoder through meshlet_edges.encode_exact, so its positions are exact integers.  The
encoder renumbers vertices and reorders faces, so nothing here rests on the input's order: the expectation is always the model on what the
oracle decodes (Case.P, Case.index)."""
import functools

import numpy as np

import meshlet_bounds as mb
import meshlet_edges as me
from conftest import MESH_CASES, load_golden

E_ARGUMENT = -8
FILL = 0xCD
BLOB_LDS_MAX = 64 << 10                       # weld_blob's limit as csrc/weld.h states it: a table of 4*T bytes within 64 KiB


def slots(nvert):
    """T: the least power of two >= 2*nvert, at least 64"""
    T = 64
    while T < 2 * nvert:
        T *= 2
    return T


def in_blob(nvert):
    return 4 * slots(nvert) <= BLOB_LDS_MAX


def build(P, index, with_index=True):
    """(remap uint32 (nvert,), welded index uint32 (3*nface,) or None, (vertices, unique, degenerate, 0)) of the contract"""
    rows = [tuple(int(x) for x in r) for r in np.asarray(P).reshape(-1, 3)]
    nvert = len(rows)
    least = {}
    remap = np.zeros(nvert, np.uint32)
    for v, r in enumerate(rows):                                       # (in vertex order: the first one met is the least)
        remap[v] = least.setdefault(r, v)
    unique = sum(1 for v in range(nvert) if remap[v] == v)
    if not with_index:
        return remap, None, (nvert, unique, 0, 0)
    flat = [int(x) for x in np.asarray(index).reshape(-1)]
    welded = np.array([int(remap[i]) if i < nvert else i for i in flat], np.uint32)
    degenerate = 0
    for a, b, c in welded.reshape(-1, 3).tolist():
        degenerate += not (a != b and b != c and a != c and max(a, b, c) < nvert)
    return remap, welded, (nvert, unique, degenerate, 0)


def check_properties(P, index, remap, windex, counts, tag=""):
    """what holds for every result whatever the model says"""
    P = np.asarray(P).reshape(-1, 3)
    nvert = len(P)
    remap = np.asarray(remap)
    assert remap.dtype == np.uint32 and remap.shape == (nvert,), (tag, remap.dtype, remap.shape)
    r = remap.astype(np.int64)
    v = np.arange(nvert)
    assert (r <= v).all(), tag                                         # remap[v] <= v
    assert (r[r] == r).all(), tag                                      # idempotent
    assert (P[r] == P).all(), tag                                      # the representative has the position
    # two vertices share a remap iff they share a position: as many representatives as distinct rows (with the line above, that is the "iff")
    distinct = len(np.unique(P, axis=0)) if nvert else 0
    assert len(np.unique(r)) == distinct, (tag, len(np.unique(r)), distinct)
    vertices, unique, degenerate, reserved = (int(c) for c in counts)
    assert vertices == nvert and reserved == 0 and unique == distinct == int((r == v).sum()), (tag, counts, distinct)
    if windex is None:
        assert degenerate == 0, (tag, counts)
        return
    flat = np.asarray(index).astype(np.int64).reshape(-1)
    w = np.asarray(windex)
    assert w.dtype == np.uint32 and w.shape == flat.shape, (tag, w.dtype, w.shape)
    ok = flat < nvert
    assert (w[~ok] == flat[~ok]).all() and (w[ok] == r[flat[ok]]).all(), tag
    t = w.astype(np.int64).reshape(-1, 3)
    bad = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2]) | (t >= nvert).any(axis=1)
    assert degenerate == int(bad.sum()), (tag, degenerate, int(bad.sum()))


def assert_same(got, exp, tag):
    """got, exp: (remap, windex or None, counts) - counts a WeldCounts or a tuple"""
    gc = got[2].as_tuple() if hasattr(got[2], "as_tuple") else tuple(int(x) for x in got[2])
    assert gc == tuple(exp[2]), (tag, gc, exp[2])
    for what, g, e in (("remap", got[0], exp[0]), ("index", got[1], exp[1])):
        assert (g is None) == (e is None), (tag, what)
        if g is None:
            continue
        g, e = np.asarray(g), np.asarray(e)
        assert g.dtype == e.dtype and g.shape == e.shape, (tag, what, g.dtype, e.dtype, g.shape, e.shape)
        if g.tobytes() != e.tobytes():
            bad = int(np.flatnonzero(g != e)[0])
            raise AssertionError("%s: %s differs from word %d on: got %s expected %s" % (tag, what, bad, g[bad], e[bad]))


def multiplicities(P):
    """how many vertices each distinct position has, sorted"""
    return sorted(np.unique(np.asarray(P).reshape(-1, 3), axis=0, return_counts=True)[1].tolist())


# ------------------------------------------------------------------------------------------------------------------------------------
# the named inputs

@functools.lru_cache(maxsize=None)
def golden(name):
    return me.Case(load_golden(name)["crt"])


def _cube24():
    """a cube whose six faces have four vertices of their own each: 24 vertices on 8 positions, three at each"""
    P, idx = [], []
    for axis in range(3):
        for side in (0, 1):
            u, v = (axis + 1) % 3, (axis + 2) % 3
            quad = []
            for a, b in ((0, 0), (1, 0), (1, 1), (0, 1)):
                p = [0, 0, 0]
                p[axis], p[u], p[v] = 100 * side, 100 * a, 100 * b
                quad.append(p)
            if not side:
                quad.reverse()                                           # outward on both sides
            n = len(P)
            P += quad
            idx += [[n, n + 1, n + 2], [n, n + 2, n + 3]]
    return np.array(P), np.array(idx, np.uint32)


SEAM = (9, 6)                                                            # two 9 x 6-cell grids: 70 vertices each, 7 of them on the seam


def _seam():
    """two grids side by side: the second one's first column lies on the first one's last, with vertices of its own"""
    n, m = SEAM
    Pa, ia = mb.grid(n, m, 10)
    Pb, ib = mb.grid(n, m, 10)
    Pb = Pb + np.array([10 * n, 0, 0])
    return np.concatenate([Pa, Pb]), np.concatenate([ia, ib + len(Pa)])


FAR = (19, 19)                                                           # two grids of 400 vertices on the same 400 positions


def _far_pairs():
    """the same grid twice, as two components: every position has two vertices, one in each"""
    Pa, ia = mb.grid(*FAR, 7)
    return np.concatenate([Pa, Pa]), np.concatenate([ia, ia + len(Pa)])


# grids by their vertex counts: 2*512 is a power of two (T = 1 024) and 513 is one vertex more (T = 2 048); 8 192 is the last blob of weld_blob
# (T = 16 384: 64 KiB) and 8 193 the first of the three kernels (T = 32 768)
GRIDS = {"grid_512": (15, 31), "grid_513": (18, 26), "grid_8192": (1, 4095), "grid_8193": (2, 2730)}
GRID_NVERT = {"grid_512": 512, "grid_513": 513, "grid_8192": 8192, "grid_8193": 8193}
GRID_SLOTS = {"grid_512": 1024, "grid_513": 2048, "grid_8192": 16384, "grid_8193": 32768}

HANDMADE = ["cube24", "seam", "coincident", "far_pairs"] + sorted(GRIDS)
NON_GRID = ["cube24", "seam", "coincident", "far_pairs"]
LATTICES = ["seam", "far_pairs"] + sorted(GRIDS)
GOLDEN_WIDE = ["fields31", "fields32"]                                   # coordinates up to 2^31: the hash sees the sign bit
assert all(n in MESH_CASES for n in GOLDEN_WIDE)


@functools.lru_cache(maxsize=None)
def handmade(name):
    if name == "coincident":
        return me.coincident()
    if name in GRIDS:
        return me.Case(me.encode_exact(*mb.grid(*GRIDS[name], 3)))
    return me.Case(me.encode_exact(*{"cube24": _cube24, "seam": _seam, "far_pairs": _far_pairs}[name]()))


def case(name):
    return handmade(name) if name in HANDMADE else golden(name)


@functools.lru_cache(maxsize=None)
def model(name, with_index=True):
    """the model's result on a named case, computed once and never changed"""
    c = case(name)
    exp = build(c.P, c.index, with_index)
    check_properties(c.P, c.index, *exp, tag=(name, "model"))
    return exp
