"""Levels of detail of a point cloud (crthip_batch_bind_cloud_lod): the sequential model of the contract in include/corto_hip.h - a dict from a
cell to its least vertex, a loop for the kept points and their weights, numpy's min and max for the chunk boxes, written from the header's words
and not from csrc/cloud_lod.h -, the properties every result has whatever the model says, what holds across the levels of one binding, and the
named inputs.  Shared by tests/test_cloud_lod_cpu.py (the kernels' source on the host, corto_amd.cloud_lod_model) and
tests/test_cloud_lod_gpu.py (the kernels).  Everything is integers: the comparison is of bytes.

Every hand-made input is a cloud of this repository's encoder with position_bits=0, position_q=1.0, so its positions are exact integers.  The
encoder reorders the points, so nothing here rests on the input's order: the expectation is always the model on what the oracle decodes
(Case.P).  The COUNTS of a level do not depend on the order (cells are sets of positions), so they are stated as literals."""
import functools

import numpy as np

import corto_amd as ca
import meshlet_edges as me
from conftest import load_golden
from corto_amd import synth

E_ARGUMENT = -8
E_LIMIT = -11
FILL = 0xCD
BLOB_MAX = 8192                                # cloud_lod_blob's limit as csrc/weld.h states it: 4*slots(nvert) bytes within 64 KiB
K_MIN, K_MAX = 32, 65536


def in_blob(nvert):
    return nvert <= BLOB_MAX


def nchunks(n, K):
    return -(-n // K) if K else 0


def cells_of(P, shift):
    """a vertex's cell: floor(p / 2^shift) a coordinate (python's >> on an int is the arithmetic shift)"""
    return [tuple(int(x) >> shift for x in r) for r in np.asarray(P).reshape(-1, 3)]


def build(P, shift, K):
    """(remap uint32 (nvert,), points uint32 (cells,), weight uint32 (cells,), chunks CLOUD_CHUNK_DTYPE (ceil(cells/K),) or None for K == 0,
    (nvert, cells, chunks, 0)) of the contract, one level"""
    P = np.asarray(P, np.int32).reshape(-1, 3)
    nvert = len(P)
    least = {}
    remap = np.zeros(nvert, np.uint32)
    for v, c in enumerate(cells_of(P, shift)):                         # (in vertex order: the first one met is the least)
        remap[v] = least.setdefault(c, v)
    points, weight, at = [], [], {}
    for v in range(nvert):
        if remap[v] == v:
            at[v] = len(points)
            points.append(v)
            weight.append(0)
    for v in range(nvert):
        weight[at[int(remap[v])]] += 1
    points, weight = np.array(points, np.uint32), np.array(weight, np.uint32)
    chunks = None
    if K:
        chunks = np.zeros(nchunks(len(points), K), ca.CLOUD_CHUNK_DTYPE)
        for c in range(len(chunks)):
            sel = P[points[c * K:(c + 1) * K]]
            chunks[c] = (sel.min(0), c * K, sel.max(0), len(sel))
    return remap, points, weight, chunks, (nvert, len(points), nchunks(len(points), K), 0)


def check_properties(P, shift, K, remap, points, weight, chunks, counts, tag=""):
    """what holds for every result whatever the model says; points, weight, chunks: exactly the written words and records"""
    P = np.asarray(P).reshape(-1, 3).astype(np.int64)
    nvert = len(P)
    remap = np.asarray(remap)
    assert remap.dtype == np.uint32 and remap.shape == (nvert,), (tag, remap.dtype, remap.shape)
    r = remap.astype(np.int64)
    v = np.arange(nvert)
    assert (r <= v).all(), tag                                         # remap[v] <= v
    assert (r[r] == r).all(), tag                                      # idempotent
    C = P >> shift                                                     # (numpy's >> on int64 is arithmetic too)
    assert (C[r] == C).all(), tag                                      # the representative is in the cell ...
    distinct = len(np.unique(C, axis=0))
    assert len(np.unique(r)) == distinct, (tag, len(np.unique(r)), distinct)   # ... and a cell has one: share a remap iff share a cell
    n, cells, nch, reserved = (int(c) for c in counts)
    assert n == nvert and cells == distinct and reserved == 0 and nch == nchunks(cells, K), (tag, counts, distinct)
    pts = np.asarray(points)
    assert pts.dtype == np.uint32 and pts.shape == (cells,), (tag, pts.dtype, pts.shape)
    assert (np.diff(pts.astype(np.int64)) > 0).all() and (pts == np.flatnonzero(r == v)).all(), tag   # strictly increasing, {v: remap[v] == v}
    if weight is not None:
        w = np.asarray(weight)
        assert w.dtype == np.uint32 and w.shape == (cells,) and int(w.astype(np.int64).sum()) == nvert, (tag, w.shape)
        assert (w == np.bincount(r, minlength=nvert)[pts]).all(), tag
    if K:
        assert chunks is not None and chunks.shape == (nch,), (tag, nch)
        first = chunks["first"].astype(np.int64)
        count = chunks["count"].astype(np.int64)
        assert (first == np.arange(nch) * K).all() and (count == np.minimum(K, cells - first)).all() and int(count.sum()) == cells, tag   # they tile [0, cells)
        for c in range(nch):                                           # every box is tight: each bound is reached by a point of the chunk
            sel = P[pts[first[c]:first[c] + count[c]]]
            assert (chunks["min"][c] == sel.min(0)).all() and (chunks["max"][c] == sel.max(0)).all(), (tag, c)
            # ... and the box over every original point of the chunk's cells follows from it
            mine = P[np.isin(r, pts[first[c]:first[c] + count[c]])]
            lo, hi = (chunks["min"][c].astype(np.int64) >> shift) << shift, ((chunks["max"][c].astype(np.int64) >> shift) << shift) + (1 << shift) - 1
            assert (mine >= lo).all() and (mine <= hi).all(), (tag, c)
    else:
        assert chunks is None or len(chunks) == 0, tag


def check_levels(levels, tag=""):
    """levels: [(shift, remap, points)] in binding order - what holds from one level to the next"""
    for (s0, r0, p0), (s1, r1, p1) in zip(levels, levels[1:]):
        assert s0 < s1, tag
        r0, r1 = np.asarray(r0).astype(np.int64), np.asarray(r1).astype(np.int64)
        assert (r1 == r1[r0]).all(), (tag, s0, s1)                     # remap_k+1[v] == remap_k+1[remap_k[v]]
        assert set(np.asarray(p1).tolist()) <= set(np.asarray(p0).tolist()), (tag, s0, s1)   # points_k+1 is a subset of points_k


def assert_same(got, exp, tag):
    """got, exp: (remap, points, weight or None, chunks or None, counts) cut to the written words - counts a CloudLodCounts or a tuple.  A None
    in got is an output that was not bound"""
    gc = got[4].as_tuple() if hasattr(got[4], "as_tuple") else tuple(int(x) for x in got[4])
    assert gc == tuple(exp[4]), (tag, gc, exp[4])
    for what, g, e in (("remap", got[0], exp[0]), ("points", got[1], exp[1]), ("weight", got[2], exp[2]), ("chunks", got[3], exp[3])):
        if g is None:
            continue
        g, e = np.asarray(g), np.asarray(e)
        assert g.dtype == e.dtype and g.shape == e.shape, (tag, what, g.dtype, e.dtype, g.shape, e.shape)
        if g.tobytes() != e.tobytes():
            bad = int(np.flatnonzero(g != e)[0])
            raise AssertionError("%s: %s differs from entry %d on: got %s expected %s" % (tag, what, bad, g[bad], e[bad]))


# ------------------------------------------------------------------------------------------------------------------------------------
# the named inputs

STEP = 16                                      # the lattices' spacing: every point in its own cell up to shift 4
STRADDLE_SHIFT = 4


def lattice(n, step=STEP):
    """n distinct points of a cubic lattice around zero"""
    side = 1
    while side ** 3 < n:
        side += 1
    i = np.arange(n)
    return (np.stack([i % side, i // side % side, i // (side * side)], 1) - side // 2) * step


def plane(side, step=STEP):
    """side^2 distinct points of a square lattice"""
    i = np.arange(side * side)
    return np.stack([i % side, i // side, np.zeros_like(i)], 1) * step


def one_cell(n, shift, seed):
    """n points inside the one cell [0, 2^shift)^3, every fifth one on top of the point before it"""
    rng = np.random.default_rng(seed)
    P = rng.integers(0, 1 << shift, (n, 3))
    P[4::5] = P[3::5][:len(P[4::5])]
    return P


def straddle():
    """points at -2^s, -1, 0 and 2^s - 1 on each axis in turn, and at the same places one cell up: -2^s and -1 are one cell, -1 and 0 never"""
    s = 1 << STRADDLE_SHIFT
    P = []
    for axis in range(3):
        for x in (-s, -1, 0, s - 1, -s - 1, s):
            for y in (0, 3 * s):
                p = [0, 0, 0]
                p[axis], p[(axis + 1) % 3] = x, y
                P.append(p)
    return np.unique(np.array(P), axis=0)


def wide(n, seed):
    """the fixture fields32's range: coordinates of both signs around 2^30, multiples of 128 (exact in a float)"""
    return synth.full_width_values(synth.Mesh(np.zeros((n, 3), np.float32)), seed).position.astype(np.int64)


# case -> (the points as they go into the encoder, the shifts of its levels)
HANDMADE = {
    "n1": (lambda: lattice(1), (0, 4)), "n2": (lambda: lattice(2), (0, 4, 5)), "n255": (lambda: lattice(255), (0, 5)),
    "n256": (lambda: lattice(256), (0, 5)), "n257": (lambda: lattice(257), (0, 5, 6, 7)),
    "lattice_8192": (lambda: lattice(8192), (4, 6)), "lattice_8193": (lambda: lattice(8193), (4, 6)),
    "plane_257": (lambda: plane(257), (4, 7)),                       # 66 049 points: 259 blocks, cloud_lod_offsets' second round
    "onecell_300": (lambda: one_cell(300, 10, 1), (0, 10)), "onecell_8193": (lambda: one_cell(8193, 10, 2), (0, 10)),
    "straddle": (straddle, (0, STRADDLE_SHIFT)),
    "wide": (lambda: wide(700, 37), (0, 31)),
    "c31": (lambda: lattice(31), (0,)), "c32": (lambda: lattice(32), (0,)), "c33": (lambda: lattice(33), (0,)), "c64": (lambda: lattice(64), (0,)),
}
GOLDEN = {"cloud_diff": (9, 11), "cloud_border": (9, 11)}
SHIFTS = dict({n: s for n, (_, s) in HANDMADE.items()}, **GOLDEN)
NAMED = list(SHIFTS)
K_SMALL = 32                                   # the chunk size of every case but ...
K_OF = {"plane_257": 1000, "lattice_8193": 100}   # ... these (any integer; fewer records to compare)
# (case, shift) -> cells: literals, computed by the model (they do not depend on the order of the points)
CELLS = {("n1", 0): 1, ("n2", 5): 2, ("n255", 5): 54, ("n256", 5): 55, ("n257", 0): 257, ("n257", 7): 8, ("lattice_8192", 4): 8192, ("lattice_8192", 6): 204,
         ("lattice_8193", 4): 8193, ("lattice_8193", 6): 204, ("plane_257", 4): 66049, ("plane_257", 7): 1089, ("onecell_300", 0): 240,
         ("onecell_300", 10): 1, ("onecell_8193", 0): 6555, ("onecell_8193", 10): 1, ("straddle", 0): 34, ("straddle", 4): 22, ("wide", 0): 700,
         ("wide", 31): 6, ("c31", 0): 31, ("c32", 0): 32, ("c33", 0): 33, ("c64", 0): 64, ("cloud_diff", 9): 3462, ("cloud_diff", 11): 254,
         ("cloud_border", 9): 780, ("cloud_border", 11): 227}


def K_of(name):
    return K_OF.get(name, K_SMALL)


def encode_exact(P):
    """the cloud of integer positions, nothing else stored"""
    P = np.asarray(P, np.int64)
    pos = P.astype(np.float32)
    assert (pos.astype(np.int64) == P).all()
    return ca.encode(synth.Mesh(pos), with_normal=False, with_color=False, with_uv=False, position_bits=0, position_q=1.0)


class Case:
    """a cloud's blob and what the oracle makes of it: integer positions (nvert, 3) int32"""

    def __init__(self, blob):
        self.blob = ca.aligned_blob(blob)
        tr = me.oc.decode(self.blob, trace=True)
        assert tr["nface"] == 0
        self.P = np.ascontiguousarray(tr["_delta_position"], np.int32).reshape(-1, 3)
        self.nvert = len(self.P)


@functools.lru_cache(maxsize=None)
def case(name):
    if name in HANDMADE:
        P = HANDMADE[name][0]()
        c = Case(encode_exact(P))
        assert c.nvert == len(P), name
        return c
    return Case(load_golden(name)["crt"])


@functools.lru_cache(maxsize=None)
def model(name, shift, K=None):
    """the model's result on a named case at one shift (K None: the case's own chunk size; 0: no chunks), computed once and never changed"""
    c = case(name)
    K = K_of(name) if K is None else K
    exp = build(c.P, shift, K)
    check_properties(c.P, shift, K, *exp, tag=(name, shift, K, "model"))
    if (name, shift) in CELLS:
        assert exp[4][1] == CELLS[(name, shift)], (name, shift, exp[4])
    return exp
