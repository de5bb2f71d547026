"""Meshlets (crthip_batch_bind_meshlets): the sequential model of the contract in include/corto_hip.h - a dict and a loop, written from the
header's words and not from csrc/meshlet.h -, the bound, the checks every result must pass apart from the model, and the named inputs.  Shared by
tests/test_meshlets_cpu.py (the kernels' source on the host, corto_amd.meshlet_model) and tests/test_meshlets_gpu.py (the kernels).
Everything is integers: the comparison is of bytes."""
import functools

import numpy as np

import corto_amd as ca
from conftest import MESH_CASES, load_golden

E_ARGUMENT = -8
FILL = 0xCD
# (max_vertices, max_triangles, segment_faces): the issue's table
PARAMS = [(64, 124, 0), (64, 124, 64), (8, 4, 16), (3, 1, 1), (255, 512, 65536), (4, 512, 0)]


def cuts(nface, groups, segment_faces):
    """the segments [(s, e)] of an index of nface faces"""
    seg = segment_faces or 4096
    out, s = [], 0
    for e in sorted({nface} | {min(int(g), nface) for g in groups}):
        while s < e:
            out.append((s, min(s + seg, e)))
            s = out[-1][1]
    return out


def build(index, groups=(), max_vertices=64, max_triangles=124, segment_faces=0):
    """(meshlets (n, 4) uint32, vertices uint32, triangles uint8, (meshlets, vertices, triangle_bytes, segments)) of the contract"""
    faces = [tuple(int(x) for x in f) for f in np.asarray(index).reshape(-1, 3)]
    segs = cuts(len(faces), groups, segment_faces)
    meshlets, vertices, triangles = [], [], bytearray()

    def emit(V, tri):
        meshlets.append((len(vertices), len(triangles), len(V), len(tri) // 3))
        vertices.extend(sorted(V, key=V.get))
        triangles.extend(tri + bytes(-len(tri) % 4))
    for s, e in segs:
        V, tri = {}, b""
        for f in faces[s:e]:
            d = [v for k, v in enumerate(f) if v not in V and v not in f[:k]]
            if len(tri) // 3 + 1 > max_triangles or len(V) + len(d) > max_vertices:
                emit(V, tri)
                V, tri = {}, b""
                d = [v for k, v in enumerate(f) if v not in f[:k]]
            for v in d:
                V[v] = len(V)
            tri += bytes(V[v] for v in f)
        if tri:
            emit(V, tri)
    return (np.array(meshlets, np.uint32).reshape(-1, 4), np.array(vertices, np.uint32), np.frombuffer(bytes(triangles), np.uint8),
            (len(meshlets), len(vertices), len(triangles), len(segs)))


def bound(nface, groups, max_vertices, max_triangles, segment_faces):
    """the derived capacity: (meshlets, vertices, triangle_bytes, segments)"""
    tmin = min(max_triangles, -(-(max_vertices - 2) // 3))
    segs = cuts(nface, groups, segment_faces)
    m = sum(-(-(e - s) // tmin) for s, e in segs)
    return (m, 3 * nface, 3 * nface + 3 * m, len(segs))


def check_properties(index, groups, params, meshlets, vertices, triangles, counts, tag=""):
    """what holds for every result whatever the model says: limits, the round trip, the placement rule, zero pads, the bound, group ends"""
    mv, mt, sf = params
    idx = np.asarray(index).astype(np.uint32).reshape(-1, 3)
    m = np.asarray(meshlets).reshape(-1, 4)
    assert (len(m), len(vertices), len(triangles)) == tuple(counts)[:3], (tag, len(m), len(vertices), len(triangles), tuple(counts))
    if len(m):
        assert m[:, 2].max() <= mv and m[:, 3].max() <= mt and m[:, 3].min() >= 1, tag
    padded = (3 * m[:, 3].astype(np.int64) + 3) & ~3
    assert (m[:, 0] == np.concatenate([[0], np.cumsum(m[:, 2])[:-1]])).all() and (m[:, 1] == np.concatenate([[0], np.cumsum(padded)[:-1]])).all(), tag
    assert int(m[:, 2].sum()) == len(vertices) and int(padded.sum()) == len(triangles) and (m[:, 1] % 4 == 0).all(), tag
    first = np.concatenate([[0], np.cumsum(m[:, 3])]).astype(np.int64)                # a meshlet's first face
    assert first[-1] == len(idx), (tag, first[-1], len(idx))
    for k, (vo, to, vc, tc) in enumerate(m.tolist()):
        local = triangles[to:to + 3 * tc]
        assert local.max(initial=0) < vc, (tag, k)
        assert (vertices[vo:vo + vc][local].reshape(-1, 3) == idx[first[k]:first[k] + tc]).all(), (tag, k)
        assert not triangles[to + 3 * tc:to + int(padded[k])].any(), (tag, k)
        assert len(set(vertices[vo:vo + vc].tolist())) == vc, (tag, k)
    bd = bound(len(idx), groups, mv, mt, sf)
    assert all(c <= b for c, b in zip(tuple(counts)[:3], bd)) and tuple(counts)[3] == bd[3], (tag, tuple(counts), bd)
    ends = set(first.tolist())
    for s, e in cuts(len(idx), groups, sf):
        assert s in ends and e in ends, (tag, s, e)


def assert_same(got, exp, tag):
    """got, exp: (meshlets, vertices, triangles, counts) - counts a MeshletCounts or a tuple"""
    gc = got[3].as_tuple() if hasattr(got[3], "as_tuple") else tuple(got[3])
    assert gc == tuple(exp[3]), (tag, gc, exp[3])
    for name, g, e in zip(("meshlets", "vertices", "triangles"), got[:3], exp[:3]):
        g, e = np.asarray(g), np.asarray(e)
        assert g.dtype == e.dtype and g.shape == e.shape, (tag, name, g.dtype, e.dtype, g.shape, e.shape)
        if g.tobytes() != e.tobytes():
            bad = np.argwhere(g.reshape(len(g), -1) != e.reshape(len(e), -1))[0, 0]
            raise AssertionError("%s: %s differ from row %d on: got %s expected %s" % (tag, name, bad, g[bad], e[bad]))


# ------------------------------------------------------------------------------------------------------------------------------------
# the named inputs: the golden meshes (the reference decoder's index and the blob's group table), and what no decoded blob can produce

@functools.lru_cache(maxsize=None)
def golden(name):
    """(index (nface, 3) uint32, group ends, blob)"""
    g = load_golden(name)
    return np.ascontiguousarray(g["index"], np.uint32).reshape(-1, 3), tuple(ca.probe_groups(g["crt"])), g["crt"]


def _rng_index(nface, nvert, seed):
    return np.random.default_rng(seed).integers(0, nvert, (nface, 3)).astype(np.uint32)


def synthetic():
    """name -> (index, groups): inputs only the hook can be given"""
    strip = np.stack([np.arange(300), np.arange(300) + 1, np.arange(300) + 2], 1).astype(np.uint32)
    degenerate = strip.copy()
    degenerate[::3, 1] = degenerate[::3, 0]                             # two equal corners
    degenerate[1::7] = degenerate[1::7, :1]                             # three equal corners
    degenerate[5::11, 2] = degenerate[5::11, 0]
    return {
        "degenerate": (degenerate, ()),
        "ids_past_16_bits": (strip * 7 + 65530, ()),
        "ids_past_31_bits": (strip * 3 + np.uint32(2 ** 31 - 150), ()),
        "ids_at_the_top": (np.uint32(2 ** 32 - 1) - _rng_index(200, 90, 3), ()),
        "groups_beyond_nface": (strip, (100, 5000, 2 ** 32 - 1)),
        "groups_repeated_unsorted": (strip, (200, 50, 50, 0, 200, 300)),
        "no_faces": (np.zeros((0, 3), np.uint32), ()),
        "no_faces_with_groups": (np.zeros((0, 3), np.uint32), (0, 7)),
        "random_dense": (_rng_index(700, 40, 1), (333,)),
        "random_sparse": (_rng_index(500, 100000, 2), ()),
        "all_new": (np.arange(3 * 400, dtype=np.uint32).reshape(-1, 3), ()),
        "one_face": (np.array([[5, 5, 9]], np.uint32), ()),
    }


def host_buffers(counts_or_bound, fill=FILL):
    """three poisoned host arrays at a capacity"""
    c = counts_or_bound
    return np.full(c[0] * 16, fill, np.uint8), np.full(c[1] * 4, fill, np.uint8), np.full(c[2], fill, np.uint8)
