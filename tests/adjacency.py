"""Adjacency (crthip_batch_bind_adjacency): the sequential model of the contract in include/corto_hip.h - a dict from a directed edge to its
least half-edge and a loop, written from the header's words and not from csrc/adjacency.h -, the properties every result has whatever the model
says, and the named inputs.  Shared by tests/test_adjacency_cpu.py (the kernels' source on the host, corto_amd.adjacency_model) and
tests/test_adjacency_gpu.py (the kernels).  Everything is integers: the comparison is of bytes."""
import functools

import numpy as np

import corto_amd as ca
from conftest import load_golden

E_ARGUMENT = -8
NO_TWIN = 0xFFFFFFFF
FILL = 0xCD
# adjacency_blob's limit as the header of csrc/adjacency.h states it: ends (nvert + 1 words, rounded up to 16 bytes) and 16-bit entries within
# 64 KiB, and a half-edge within 16 bits
BLOB_LDS_MAX = 64 << 10


def blob_lds(nvert, nface):
    return (((nvert + 1) * 4 + 15) & ~15) + ((nface * 6 + 15) & ~15)


def in_blob(nvert, nface):
    return 3 * nface <= 65536 and blob_lds(nvert, nface) <= BLOB_LDS_MAX


def valid_faces(index, nvert):
    idx = np.asarray(index).astype(np.int64).reshape(-1, 3)
    return (idx[:, 0] != idx[:, 1]) & (idx[:, 1] != idx[:, 2]) & (idx[:, 0] != idx[:, 2]) & (idx < nvert).all(axis=1)


def build(index, nvert):
    """(twin uint32 (3*nface,), (halfedges, boundary, duplicate, invalid)) of the contract"""
    faces = [tuple(int(x) for x in f) for f in np.asarray(index).reshape(-1, 3)]
    ok = [len(set(f)) == 3 and max(f) < nvert for f in faces]
    least, duplicate = {}, 0
    for f, face in enumerate(faces):                                   # (in half-edge order: the first one met is the least)
        for s in range(3):
            if ok[f]:
                e = (face[s], face[(s + 1) % 3])
                duplicate += e in least
                least.setdefault(e, 3 * f + s)
    twin = np.full(3 * len(faces), NO_TWIN, np.uint32)
    boundary = invalid = 0
    for f, face in enumerate(faces):
        for s in range(3):
            if not ok[f]:
                invalid += 1
                continue
            t = least.get((face[(s + 1) % 3], face[s]), NO_TWIN)
            twin[3 * f + s] = t
            boundary += t == NO_TWIN
    return twin, (3 * len(faces), boundary, duplicate, invalid)


def check_properties(index, nvert, twin, counts, tag=""):
    """what holds for every result whatever the model says: twin[h] runs the other way, there is no lower candidate, the counts are
    consistent, duplicate == 0 makes twin an involution"""
    idx = np.asarray(index).astype(np.int64).reshape(-1, 3)
    twin = np.asarray(twin)
    H = 3 * len(idx)
    assert twin.dtype == np.uint32 and twin.shape == (H,), (tag, twin.dtype, twin.shape)
    halfedges, boundary, duplicate, invalid = (int(c) for c in counts)
    org = idx.reshape(-1)
    head = idx[:, [1, 2, 0]].reshape(-1)
    ok = np.repeat(valid_faces(idx, nvert), 3)
    paired = twin != NO_TWIN
    assert halfedges == H and invalid == int((~ok).sum()) and boundary == int((ok & ~paired).sum()), (tag, counts)
    assert not paired[~ok].any(), tag                                  # an invalid half-edge has no twin ...
    t = twin[paired].astype(np.int64)
    assert (t < H).all() and ok[t].all(), tag                          # ... and is nobody's
    assert (org[t] == head[paired]).all() and (head[t] == org[paired]).all(), tag    # the twin runs the other way
    # no lower candidate: among the valid half-edges of one directed edge, sorted by number, the first is the one every twin names
    key = org[ok] * (nvert + 1) + head[ok]
    hs = np.flatnonzero(ok)
    order = np.lexsort((hs, key))
    key, hs = key[order], hs[order]
    firsts = np.concatenate([[True], key[1:] != key[:-1]]) if len(key) else np.zeros(0, bool)
    assert duplicate == int((~firsts).sum()), (tag, duplicate, int((~firsts).sum()))
    least_of = dict(zip(key[firsts].tolist(), hs[firsts].tolist()))
    want = np.array([least_of.get(int(b) * (nvert + 1) + int(a), NO_TWIN) for a, b in zip(org[ok], head[ok])], np.int64)
    assert (twin[ok].astype(np.int64) == want).all(), tag
    if duplicate == 0:
        assert (twin[t] == np.flatnonzero(paired)).all(), tag           # an involution on the paired half-edges


def assert_same(got, exp, tag):
    """got, exp: (twin, counts) - counts an AdjacencyCounts or a tuple"""
    gc = got[1].as_tuple() if hasattr(got[1], "as_tuple") else tuple(int(x) for x in got[1])
    assert gc == tuple(exp[1]), (tag, gc, exp[1])
    g, e = np.asarray(got[0]), np.asarray(exp[0])
    assert g.dtype == e.dtype and g.shape == e.shape, (tag, g.dtype, e.dtype, g.shape, e.shape)
    if g.tobytes() != e.tobytes():
        bad = int(np.flatnonzero(g != e)[0])
        raise AssertionError("%s: twins differ from half-edge %d on: got %s expected %s" % (tag, bad, g[bad], e[bad]))


def gl_triangles_adjacency(index, twin):
    """INTEGRATION.md's recipe: six ids a face for GL_TRIANGLES_ADJACENCY - a corner, then the vertex across the edge that starts there (the
    corner itself where the edge has no twin)"""
    flat = np.asarray(index).astype(np.uint32).reshape(-1)
    t = np.asarray(twin).astype(np.int64)
    opposite = np.where(t == NO_TWIN, flat, flat[np.where(t == NO_TWIN, 0, t // 3 * 3 + (t % 3 + 2) % 3)])
    return np.stack([flat, opposite], 1).reshape(-1, 6)


# ------------------------------------------------------------------------------------------------------------------------------------
# the named inputs: the golden meshes (the reference decoder's index), and what no decoded blob can produce

@functools.lru_cache(maxsize=None)
def golden(name):
    """(index (nface, 3) uint32, nvert, blob)"""
    g = load_golden(name)
    return np.ascontiguousarray(g["index"], np.uint32).reshape(-1, 3), int(ca.probe(g["crt"]).nvert), g["crt"]


def fan(valence, closed):
    """a fan of `valence` faces round vertex 0; closed: the rim's last vertex is its first"""
    rim = np.arange(valence + 1) % valence + 1 if closed else np.arange(valence + 1) + 1
    idx = np.stack([np.zeros(valence, np.int64), rim[:-1], rim[1:]], 1).astype(np.uint32)
    return idx, int(idx.max()) + 1


def strip(nface, nvert):
    """a triangle strip of nface faces with consistent winding over the first nface + 2 of nvert vertices"""
    k = np.arange(nface)
    idx = np.where((k % 2 == 0)[:, None], np.stack([k, k + 1, k + 2], 1), np.stack([k + 1, k, k + 2], 1)).astype(np.uint32)
    assert nface + 2 <= nvert
    return idx, nvert


def handmade():
    """name -> (index, nvert)"""
    A = lambda rows: np.array(rows, np.uint32).reshape(-1, 3)           # noqa: E731
    cases = {
        "one_face": (A([[0, 1, 2]]), 3),
        "two_faces_consistent": (A([[0, 1, 2], [2, 1, 3]]), 4),
        "two_faces_same_direction": (A([[0, 1, 2], [1, 2, 3]]), 4),     # 1 -> 2 twice: both boundary there, one duplicate
        "same_face_twice": (A([[0, 1, 2], [0, 1, 2]]), 3),
        "face_and_mirror": (A([[0, 1, 2], [2, 1, 0]]), 3),
        "degenerate_and_out_of_range": (A([[0, 1, 2], [2, 1, 1], [2, 1, 3], [3, 1, 9], [3, 1, 4], [4, 4, 4], [0xFFFFFFFF, 4, 1], [4, 1, 5]]), 6),
        "fan_300_closed": fan(300, True),
        "fan_300_open": fan(300, False),
    }
    for nvert in (255, 256, 257):
        cases["nvert_%d" % nvert] = strip(nvert - 2, nvert)
    cases["halfedges_255"] = strip(85, 300)
    cases["halfedges_258"] = strip(86, 300)
    return cases
