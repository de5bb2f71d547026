"""Shared by the encoder topology tests (test_encode_topology_cpu.py, test_encode_topology_gpu.py): the meshes the device topology pass
is held against the host pass on.  Every builder returns [(name, mesh, encode keywords)]."""
import os
import sys

import numpy as np

import corto_amd as ca
from corto_amd import synth as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_cases():
    """the named fixtures of tests/golden/cases.py, clouds included"""
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    from cases import cases
    return cases()


def mixed_corpus():
    """the three predictions, both entropies, groups, unreferenced vertices, a mesh whose faces are all degenerate, non-manifold meshes, clouds"""
    items = []
    for p in (ca.DIFF, ca.ESTIMATED, ca.BORDER):
        for e in (0, 1):
            kw = dict(normal_prediction=p, entropy=e)
            items.append(("sphere", S.bumpy_sphere(24 + 4 * p, 12, seed=10 * p + e, color_components=3 + e), kw))
            items.append(("delaunay", S.shuffled(S.delaunay_disc(300, seed=p + 3 * e, holes=3), seed=p), kw))
            items.append(("fan", S.cone_fan(40, 2, seed=p + e), dict(kw, position_bits=12)))
            items.append(("decimated", S.decimated(S.icosphere(2, seed=p + e), keep=0.5, seed=p), kw))
            items.append(("confetti", S.confetti(60, seed=p + e), kw))
            items.append(("flipped", S.bumpy_sphere_flipped(16, 8, seed=p + e), kw))
            items.append(("non_manifold", S.non_manifold(S.delaunay_disc(200, seed=5 + p, holes=2), seed=p + e, fins=4, dups=3, reversed_dups=3,
                                                         bowties=2, glue=2), kw))
            items.append(("cloud", S.point_cloud(30, 20, seed=p + e), kw))
            items.append(("torus", S.torus(20, 10, seed=p + e), dict(kw, with_uv=False)))
    for s in range(40):
        m = S.bumpy_sphere(10 + s % 30, 6 + s % 5, seed=100 + s, color_components=3 + s % 2)
        if s % 3 == 0:
            m.radius = (0.5 + np.arange(m.nvert, dtype=np.float32) % 7).reshape(-1, 1)
        if s % 4 == 0:
            m.groups = [m.nface // 3, m.nface]
            m.group_props = [{"material": "m%d" % s}, {}]
        items.append(("grid%d" % s, m, dict(normal_prediction=s % 3, entropy=s % 2, exif={"k": str(s)} if s % 5 == 0 else None)))
    m = S.bumpy_sphere(16, 8, seed=7)                               # unreferenced vertices
    m.position = np.ascontiguousarray(np.vstack([m.position, np.random.default_rng(1).random((20, 3), dtype=np.float32)]))
    for a in ("normal", "uv", "color"):
        v = getattr(m, a)
        setattr(m, a, np.ascontiguousarray(np.vstack([v, np.repeat(v[:1], 20, axis=0)])))
    items.append(("unreferenced", m, dict(normal_prediction=ca.ESTIMATED)))
    d = S.bumpy_sphere(8, 4, seed=8)                                # every face degenerate
    d.index = np.ascontiguousarray(np.repeat(d.index[:, :1], 3, axis=1))
    items.append(("all_degenerate", d, dict(normal_prediction=ca.BORDER)))
    g = S.bumpy_sphere(12, 6, seed=9)                               # groups that end before the last face, one of them empty
    g.groups = [10, 10, g.nface - 7]
    items.append(("short_groups", g, dict(normal_prediction=ca.DIFF)))
    return items


def book(leaves=48, base=0, seed=0):
    """`leaves` faces on one edge (base, base + 1), windings mixed: the edge's bucket holds that many equal keys"""
    rng = np.random.default_rng(seed)
    nv = base + 2 + leaves
    faces = [(0, 1, 2)] if base >= 3 else []
    for i in range(leaves):
        a, b, c = base, base + 1, base + 2 + i
        faces.append((a, b, c) if rng.integers(2) else (b, a, c))
    return S.Mesh(rng.random((nv, 3), dtype=np.float32), np.array(faces, dtype=np.uint32))


def random_soup(seed):
    """3..60 vertices, faces drawn at random with repeats: non-manifold and degenerate configurations are the norm"""
    rng = np.random.default_rng(1000 + seed)
    nv = int(rng.integers(3, 61))
    nf = int(rng.integers(1, 4 * nv + 2))
    pool = rng.integers(0, nv, size=(max(nf // 2, 1), 3))
    idx = np.vstack([pool, pool[rng.integers(0, len(pool), size=nf - len(pool))]]) if nf > len(pool) else pool[:nf]
    flip = rng.random(len(idx)) < 0.3
    idx = np.where(flip[:, None], idx[:, ::-1], idx)
    idx = idx[rng.permutation(len(idx))]
    m = S.Mesh(rng.random((nv, 3), dtype=np.float32), idx.astype(np.uint32))
    if seed % 3 == 0 and len(idx) > 2:
        cut = int(rng.integers(1, len(idx)))
        m.groups = [cut, len(idx)]
    return m


def pairing_cases(nrandom=240):
    kw = dict(with_normal=False, with_color=False, with_uv=False)
    sphere, fan = S.bumpy_sphere(16, 8, seed=3), S.cone_fan(40, 2, seed=4)
    seam = S.merge([sphere, fan])
    seam.groups = [sphere.nface, seam.nface]                        # the fan's apex (valence 40) is the smallest vertex of the second group
    items = [("fan_second_group", seam, dict(normal_prediction=ca.BORDER)),
             ("book48", book(48), kw), ("book64_high_edge", book(64, base=5, seed=1), kw), ("book17", book(17, seed=2), kw)]
    items += [("soup%d" % s, random_soup(s), kw) for s in range(nrandom)]
    return items


def wide_mesh():
    """3*ntri > 65535: 32-bit links, the global state image"""
    return ("bumpy256x128", S.bumpy_sphere(256, 128, seed=5), dict(normal_prediction=ca.ESTIMATED))


def is_mesh(m):
    return m.index is not None and m.nface > 0
