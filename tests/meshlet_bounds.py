"""Meshlet bounds (crthip_batch_bind_meshlet_bounds): the sequential model of the record in include/corto_hip.h - Python ints for the integer
parts, wrapping where the contract says modulo 2^64, np.float32 scalars for the float steps, one operation at a time; written from the
header's words and not from csrc/meshlet_bounds.h -, the properties every result must have whatever the model says, and the named inputs.
Shared by tests/test_meshlet_bounds_cpu.py (the kernel's source on the host, corto_amd.meshlet_bounds_model) and
tests/test_meshlet_bounds_gpu.py (the kernel).  Tolerance 0: the comparison is of bytes."""
import functools
import math

import numpy as np

import corto_amd as ca
import meshlets as ml
from conftest import load_golden
from oracle import oracle as oc

E_NEEDS_POSITION, E_ARGUMENT = -6, -8
FILL = 0xCD
F32 = np.float32
M64 = (1 << 64) - 1
DT = ca.MESHLET_BOUNDS_DTYPE


def _s64(x):
    """a residue modulo 2^64 as the signed value it stands for"""
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def _s32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def _scaled(X):
    """(float32 x 3) sign(x)*(|x| >> k) with k = max(0, bitlength(max |x|) - 24); X: three residues modulo 2^64; |INT64_MIN| is 2^63"""
    mags = [abs(_s64(x)) for x in X]
    k = max(0, max(mags).bit_length() - 24)
    out = []
    for x, mg in zip(X, mags):
        v = mg >> k
        assert v < 1 << 24
        out.append(F32(-v if _s64(x) < 0 else v))
    return out


def _len3(s):
    return np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])


def ceil_sqrt(r2):
    """the smallest r in [0, 2^32 - 1] with r*r >= r2, or 2^32 - 1"""
    r = math.isqrt(r2)
    if r * r < r2:
        r += 1
    return min(r, 2 ** 32 - 1)


def face_normal(p, a, b, c):
    """cross(p[b] - p[a], p[c] - p[a]) as three residues modulo 2^64 (the differences are exact in 64 bits)"""
    e1 = [p[b][i] - p[a][i] for i in range(3)]
    e2 = [p[c][i] - p[a][i] for i in range(3)]
    return [(e1[1] * e2[2] - e1[2] * e2[1]) & M64, (e1[2] * e2[0] - e1[0] * e2[2]) & M64, (e1[0] * e2[1] - e1[1] * e2[0]) & M64]


def cone_faces(p, nvert, V, tri):
    """the meshlet's cone faces: [(a, b, c, N)] with global ids, all present, N != 0"""
    out = []
    for f in range(len(tri) // 3):
        a, b, c = (V[int(tri[3 * f + k])] for k in range(3))
        if a < nvert and b < nvert and c < nvert:
            N = face_normal(p, a, b, c)
            if any(N):
                out.append((a, b, c, N))
    return out


def one(p, nvert, V, tri):
    """the record of one meshlet as a tuple (box_min, box_max, center, radius, axis, cutoff)"""
    present = [v for v in V if v < nvert]
    if not present:
        return ([0] * 3, [0] * 3, [0] * 3, 0, [0] * 3, 127)
    bmin = [min(p[v][c] for v in present) for c in range(3)]
    bmax = [max(p[v][c] for v in present) for c in range(3)]
    span = [(bmax[c] - bmin[c]) & 0xFFFFFFFF for c in range(3)]
    center = [_s32((bmin[c] & 0xFFFFFFFF) + (span[c] >> 1)) for c in range(3)]
    r2 = max(sum((p[v][c] - center[c]) ** 2 for c in range(3)) & M64 for v in present)
    radius = ceil_sqrt(r2)
    axis, cutoff = [0, 0, 0], 127
    faces = cone_faces(p, nvert, V, tri)
    if faces:
        S = [sum(N[c] for *_, N in faces) & M64 for c in range(3)]
        s = _scaled(S)
        with np.errstate(all="ignore"):
            L = _len3(s)
            if L > 0:
                for c in range(3):
                    t = (s[c] / L) * F32(127.0)
                    assert t.dtype == F32
                    axis[c] = int(t + (F32(-0.5) if t < 0 else F32(0.5)))       # int() truncates
                A = [F32(x) for x in axis]
                la = _len3(A)
                m = None
                for *_, N in faces:
                    n = _scaled(N)
                    d = ((A[0] * n[0] + A[1] * n[1]) + A[2] * n[2]) / (la * _len3(n))
                    assert d.dtype == F32 and np.isfinite(d)
                    m = d if m is None or d < m else m
                if m > F32(0.1):
                    w = F32(1.0) - m * m
                    if not w > 0:
                        w = F32(0.0)
                    cutoff = min(127, int(np.sqrt(w) * F32(127.0)) + 2)
    return (bmin, bmax, center, radius, axis, cutoff)


def model(position, meshlets, vertices, triangles, counts=None):
    """the records of a finished meshlet build, a DT array; position (nvert, 3) integers"""
    p = [tuple(int(x) for x in row) for row in np.asarray(position).reshape(-1, 3)]
    m = np.asarray(meshlets).reshape(-1, 4)
    if counts is not None:
        m = m[:tuple(counts)[0]]
    V, T = [int(x) for x in vertices], bytes(np.asarray(triangles, np.uint8))
    out = np.zeros(len(m), DT)
    for k, (vo, to, vc, tc) in enumerate(m.tolist()):
        r = one(p, len(p), V[vo:vo + vc], T[to:to + 3 * tc])
        out[k] = (r[0], r[1], r[2], r[3], r[4], r[5], 0)
    return out


def check_properties(position, meshlets, vertices, triangles, bounds, tag=""):
    """what holds for every result whatever the model says: a tight box, a sphere that holds every vertex with the least integer radius,
    a cone that holds every face normal (float64 on the exact normals), reserved == 0"""
    p = [tuple(int(x) for x in row) for row in np.asarray(position).reshape(-1, 3)]
    nvert = len(p)
    m = np.asarray(meshlets).reshape(-1, 4)
    V, T = [int(x) for x in vertices], bytes(np.asarray(triangles, np.uint8))
    assert len(bounds) == len(m), (tag, len(bounds), len(m))
    for k, (vo, to, vc, tc) in enumerate(m.tolist()):
        b = bounds[k]
        assert int(b["reserved"]) == 0, (tag, k)
        present = [v for v in V[vo:vo + vc] if v < nvert]
        if not present:
            assert bytes(b.tobytes()) == bytes(43) + b"\x7f" + bytes(4), (tag, k)
            continue
        bmin, bmax, center, radius = [int(x) for x in b["box_min"]], [int(x) for x in b["box_max"]], [int(x) for x in b["center"]], int(b["radius"])
        for c in range(3):
            xs = [p[v][c] for v in present]
            assert all(bmin[c] <= x <= bmax[c] for x in xs), (tag, k, "outside the box")
            assert bmin[c] in xs and bmax[c] in xs, (tag, k, "the box is not tight")
        r2 = max(sum((p[v][c] - center[c]) ** 2 for c in range(3)) for v in present)
        # (the centre is the box's midpoint, so no distance is beyond 2^31 a component: r2 < 2^64 and the radius below 2^32, never the clamp)
        assert radius * radius >= r2, (tag, k, "a vertex outside the sphere")
        if radius > 0:
            assert (radius - 1) ** 2 < r2, (tag, k, "the radius is not the least")
        cutoff, axis = int(b["cone_cutoff"]), [int(x) for x in b["cone_axis"]]
        assert 0 <= cutoff <= 127, (tag, k)
        if cutoff < 127:
            la = math.sqrt(sum(x * x for x in axis))
            assert la > 0, (tag, k)
            least = math.sqrt(1.0 - (cutoff / 127.0) ** 2)
            for *_, N in cone_faces(p, nvert, V[vo:vo + vc], T[to:to + 3 * tc]):
                n = [float(_s64(x)) for x in N]
                cos = sum(a * x for a, x in zip(axis, n)) / (la * math.sqrt(sum(x * x for x in n)))
                assert cos >= least, (tag, k, cos, least)


def assert_same(got, exp, tag):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype == DT and got.shape == exp.shape, (tag, got.dtype, got.shape, exp.shape)
    if got.tobytes() != exp.tobytes():
        bad = [k for k in range(len(got)) if got[k].tobytes() != exp[k].tobytes()]
        raise AssertionError("%s: %d of %d records differ, first %d: got %s expected %s" % (tag, len(bad), len(got), bad[0], got[bad[0]], exp[bad[0]]))


# ------------------------------------------------------------------------------------------------------------------------------------
# the named inputs: the golden meshes (the oracle's delta-decoded integer positions and index, the blob's group table), and hand-made ones

@functools.lru_cache(maxsize=None)
def golden(name):
    """(integer positions (nvert, 3) int32, index (nface, 3) uint32, group ends, blob)"""
    g = load_golden(name)
    blob = ca.aligned_blob(g["crt"])
    tr = oc.decode(blob, trace=True)
    return (np.ascontiguousarray(tr["_delta_position"], np.int32).reshape(-1, 3), np.ascontiguousarray(tr["index"], np.uint32).reshape(-1, 3),
            tuple(ca.probe_groups(g["crt"])), blob)


@functools.lru_cache(maxsize=None)
def golden_build(name, params):
    """(meshlets, vertices, triangles, counts tuple) of a golden mesh by the sequential meshlet model, and its bounds by the model here"""
    P, idx, groups, _ = golden(name)
    b = ml.build(idx, groups, *params)
    return b, model(P, *b[:3])


def grid(n, m, scale=1, z=lambda i, j: 0):
    """an (n+1) x (m+1) grid of vertices and its 2*n*m faces"""
    P = np.array([[i * scale, j * scale, z(i, j)] for i in range(n + 1) for j in range(m + 1)], np.int64)
    idx = []
    for i in range(n):
        for j in range(m):
            a = i * (m + 1) + j
            idx += [[a, a + m + 1, a + 1], [a + 1, a + m + 1, a + m + 2]]
    return P.astype(np.int32), np.array(idx, np.uint32)


def sphere(n=8, r=1000):
    """a closed latitude-longitude sphere, outward faces"""
    P = [[0, 0, r]]
    for i in range(1, n):
        for j in range(2 * n):
            t, f = math.pi * i / n, math.pi * j / n
            P.append([round(r * math.sin(t) * math.cos(f)), round(r * math.sin(t) * math.sin(f)), round(r * math.cos(t))])
    P.append([0, 0, -r])
    ring = lambda i, j: 1 + (i - 1) * 2 * n + j % (2 * n)
    idx = []
    for j in range(2 * n):
        idx.append([0, ring(1, j), ring(1, j + 1)])
        idx.append([len(P) - 1, ring(n - 1, j + 1), ring(n - 1, j)])
        for i in range(1, n - 1):
            idx += [[ring(i, j), ring(i + 1, j), ring(i + 1, j + 1)], [ring(i, j), ring(i + 1, j + 1), ring(i, j + 1)]]
    return np.array(P, np.int32), np.array(idx, np.uint32)


def soup(nface, lo, hi, seed):
    """nface faces of three vertices of their own, coordinates uniform in [lo, hi]"""
    P = np.random.default_rng(seed).integers(lo, hi, (3 * nface, 3), endpoint=True).astype(np.int32)
    return P, np.arange(3 * nface, dtype=np.uint32).reshape(-1, 3)


def fan(nvert_rim):
    """a bumpy fan: one centre and a rim; nvert_rim + 1 vertices, nvert_rim - 1 faces"""
    P = [[0, 0, 50]] + [[round(900 * math.cos(0.02 * i)), round(900 * math.sin(0.02 * i)), (i * 37) % 23] for i in range(nvert_rim)]
    return np.array(P, np.int32), np.array([[0, i + 1, i + 2] for i in range(nvert_rim - 1)], np.uint32)


I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def synthetic():
    """name -> (position, nvert or None, index, params): the edges of the issue's table.  nvert: what the hook is told (ids at or beyond
    it are absent); None: len(position)"""
    out = {}
    P, idx = grid(1, 1)
    out["one_face"] = (P, None, idx[:1], (64, 124, 0))
    P, idx = grid(6, 5, 100, lambda i, j: (i * i + 3 * j) % 17)
    out["one_face_each"] = (P, None, idx, (3, 1, 1))
    # 255 vertices, 512 faces in one meshlet: every lane-stride round full plus one short (255 = 3*64 + 63, 512 = 8*64)
    P, idx = fan(254)
    extra = np.random.default_rng(5).integers(0, 255, (512 - len(idx), 3)).astype(np.uint32)
    out["full_meshlet"] = (P, None, np.concatenate([idx, extra]), (255, 512, 65536))
    for n in (63, 64, 65):                                                           # wave edges: n vertices and n faces in one meshlet
        P, idx = fan(n - 1)
        idx = np.concatenate([idx, np.array([[0, 1, n - 1], [1, 2, 3]], np.uint32)])[:n]
        assert len(P) == n and len(idx) == n
        out["wave_edge_%d" % n] = (P, None, idx, (255, 512, 65536))
    P, idx = grid(5, 5, 64)
    out["planar_patch"] = (P, None, idx, (64, 124, 0))
    P, idx = sphere()
    out["closed_sphere_one_meshlet"] = (P, None, idx, (255, 512, 65536))
    P = np.array([[0, 0, 0], [10, 0, 0], [20, 0, 0], [30, 0, 0], [5, 5, 5]], np.int32)
    out["all_degenerate"] = (P, None, np.array([[0, 0, 1], [1, 1, 1], [0, 1, 2], [3, 2, 0], [4, 4, 0]], np.uint32), (64, 124, 0))
    out["two_opposite_faces"] = (np.array([[0, 0, 0], [7, 0, 0], [0, 9, 0]], np.int32), None, np.array([[0, 1, 2], [0, 2, 1]], np.uint32), (64, 124, 0))
    P, idx = soup(40, -(2 ** 23 - 1), 2 ** 23 - 1, 11)
    P[:6] = [[-(2 ** 23 - 1), -(2 ** 23 - 1), 0], [2 ** 23 - 1, -(2 ** 23 - 1), 0], [0, 2 ** 23 - 1, 2 ** 23 - 1]] * 2
    out["coordinates_at_23_bits"] = (P, None, idx, (64, 124, 0))
    P, idx = soup(30, I32_MIN, I32_MAX, 12)
    P[:9] = [[I32_MIN, I32_MIN, I32_MIN], [I32_MAX, I32_MIN, I32_MIN], [I32_MIN, I32_MAX, I32_MAX],
             [I32_MAX, I32_MAX, I32_MAX], [I32_MIN, I32_MIN, I32_MAX], [I32_MAX, I32_MIN, I32_MAX],
             [I32_MIN, 0, 0], [I32_MAX, 0, 0], [0, I32_MAX, I32_MIN]]
    out["coordinates_at_int32_ends"] = (P, None, idx, (6, 2, 0))
    out["int32_ends_one_meshlet"] = (P, None, idx, (255, 512, 0))
    # ids >= nvert: the faces of the second half name vertices the hook is told are not there; at (3, 1, 1) some meshlets have none at all
    P, idx = grid(4, 4, 50, lambda i, j: (7 * i + j * j) % 11)
    idx = idx.copy()
    idx[10:16] += np.uint32(100)
    idx[16:20, 1] = np.uint32(2 ** 32 - 1)
    out["absent_ids_some"] = (P, None, idx, (64, 124, 0))
    out["absent_ids_all_of_one"] = (P, None, idx, (3, 1, 1))
    out["one_vertex"] = (np.array([[5, -6, 7]], np.int32), None, np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.uint32), (64, 124, 0))
    return out


def build_host(index, params, groups=()):
    """a finished meshlet build on the host by the hook: (meshlets, vertices, triangles, counts)"""
    return ca.meshlet_model(index, groups, *params)
