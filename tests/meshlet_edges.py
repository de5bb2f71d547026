"""The edges of the meshlet kernels (crthip_batch_bind_meshlets, crthip_batch_bind_meshlet_bounds) that the device has to meet and that no
golden mesh reaches: empty and cancelling cones, the shift edge of tan_shift_of, the cutoff's clamp, short second to seventh lane-stride rounds,
wide values in big meshlets, partial last workgroups behind one another, a count at its capacity, and 4 | 5 segments - the cases and their
builders, shared by tests/test_meshlet_edges_cpu.py (every case reaches the figures it is named for, and the host hooks equal the models on
it) and tests/test_meshlet_edges_gpu.py (the kernels against the models).

Every input is a blob of this repository's encoder.  Exact integers come from position_bits = 0, position_q = 1 and float32-exact positions;
the encoder renumbers vertices and reorders faces, so nothing here rests on the input's order: the reference is ml.build and mb.model on
what the oracle decodes (Case.P, Case.index) and on the blob's group table, and `figures` measures on the same integers.

What each case was measured to reach on the oracle's integers (tests/test_meshlet_edges_cpu.py asserts the conditions each case is named for;
the other figures are what the builders gave on the day this was written).  |S| and r2 in bits; "clamped": meshlets whose
int(sqrtf(1 - m*m)*127) + 2 is 127 or more with m > 0.1:

  case               params              meshlets  vertices a meshlet    faces a meshlet        cones                                  |S|  r2
  coincident         (64, 124, 0)        3         64, 64, 53            98, 80, 78             3 empty, radius 0, box of no extent    -    0
  collinear          (64, 124, 0)        3         64, 64, 53            98, 80, 78             3 empty, radius > 0                    -    18
  closed_200         (255, 512, 65536)   1         200                   396                    1 cancelling: 396 cone faces, S = 0    0    20
  closed_255         (255, 512, 65536)   1         255                   506                    1 cancelling: 506 cone faces, S = 0    0    20
  flat_{z,x,y}{+,-}  (64, 124, 0)        3 each    64, 64, 63            98, 95, 95             axis +-127 on the plane's, cutoff 2    19   19
  shift_edge         (3, 1, 1)           23        3                     1                      cutoff 2; largest |component| of S     25   28
                                                                                                2^24 - 1, 2^24, 2^24 + 1 in each
                                                                                                component with each sign (18 faces),
                                                                                                and 5 tilted faces (SHIFT_TILTS)
  cutoff_clamp       (4, 2, 2)           4         4                     2                      raw cutoff 126, 126, 127, 128: 2       16   18
                                                                                                clamped, all with m > 0.1
  rounds             (65, 512, 0)        65        34 .. 65              30 .. 100              none empty, 3 clamped                  19   21
                     (128, 512, 0)       29        127, 128              122 .. 212             1 clamped                              20   21
                     (129, 512, 0)       29        97, 129               119 .. 214             1 clamped                              20   21
                     (192, 512, 0)       17        112, 192              147 .. 330                                                    21   21
                     (193, 512, 0)       17        87, 193               100 .. 332                                                    21   21
                     (254, 512, 0)       12        16, 254               12 .. 445                                                     21   21
  full_512           (255, 512, 65536)   1         250                   512                    512 cone faces, S != 0, cutoff 127     17   20
  past_512           (255, 512, 65536)   2         252, 12               512, 4                 the triangle limit cuts at 512         17   21
  wide,              (255, 512, 0)       2         255, 73               480, 116               cutoff 127; S wraps modulo 2^64;       63   62
  wide_no_normals    (64, 124, 0)        8         64 x 7, 36            97, 71, 72 x 4, 85, 55 spans >= 2^31                          63   62
  grid               grid_params(i)      1, 2, 3, 4, 5, 1 meshlets of closed meshes of 34 .. 62 vertices: five partial last workgroups of K-MLB
  segments           (64, 124, sf)       sf = 296, 148, 74, 73: 1, 2, 4 and 5 segments of a closed mesh of 296 faces

rounds: bumpy_sphere(64, 32) x 1000, rounded.  Over ROUND_PARAMS the meshlets' vertex counts fall in every class of VERTEX_CLASSES ([65, 127]
at all but the last triple, {128} at 128, [129, 191] at 129, {192} at 192, [193, 254] at 193 and 254) and their face counts in every class of
FACE_CLASSES ([129, 191] at 128, 129 and 192, [193, 255] at 128 to 193, [257, 319] and [321, 383] from 192 on, [385, 447] at 254 only): every lane-stride round
of K-MLB is the last, short one somewhere, with one lane (65, 129, 193 vertices), with all (128, 192) and with all but one (254).

512 faces in one meshlet: reached.  The encoder keeps a duplicated face on the vertices of its original, so closed_mesh(250) with 16
duplicated faces decodes to 250 vertices and 512 faces: one meshlet at (255, 512, 65536).

wide: the widest the value coder takes is +-1 074 789 632, so r2 stays at 62 bits."""
import functools

import numpy as np

import corto_amd as ca
import meshlet_bounds as mb
import meshlets as ml
import size_classes as sc
import tangent_edges as te
import value_ranges as vr
from corto_amd import synth
from oracle import oracle as oc

F32 = np.float32


class Case:
    """a blob and what the oracle makes of it: integer positions (nvert, 3) int32, index (nface, 3) uint32, group ends; the models' results a
    parameter triple, computed once and never changed"""

    def __init__(self, blob):
        self.blob = ca.aligned_blob(blob)
        tr = oc.decode(self.blob, trace=True)
        self.tr = tr
        self.P = np.ascontiguousarray(tr["_delta_position"], np.int32).reshape(-1, 3)
        self.index = np.ascontiguousarray(tr["index"], np.uint32).reshape(-1, 3)
        self.groups = tuple(ca.probe_groups(self.blob))
        self.nvert, self.nface = len(self.P), len(self.index)
        self._build, self._bounds = {}, {}

    def build(self, params):
        """(meshlets, vertices, triangles, counts) by the sequential model"""
        if params not in self._build:
            self._build[params] = ml.build(self.index, self.groups, *params)
        return self._build[params]

    def bounds(self, params):
        if params not in self._bounds:
            self._bounds[params] = mb.model(self.P, *self.build(params)[:3])
        return self._bounds[params]

    def redone(self):
        """K-DELTA's int16 records cannot hold the positions (tests/value_ranges.py: host_rule)"""
        return bool(vr.host_rule(self.tr["_raw_position"], self.tr["_delta_position"])[0])


def encode_exact(P, index):
    """the blob of integer positions, nothing else stored"""
    P = np.asarray(P, np.int64)
    pos = P.astype(np.float32)
    assert (pos.astype(np.int64) == P).all()
    return ca.encode(synth.Mesh(pos, np.asarray(index, np.uint32)), with_normal=False, with_color=False, with_uv=False, position_bits=0, position_q=1.0)


# ------------------------------------------------------------------------------------------------------------------------------------
# what a case reaches, measured on the oracle's integers

def exact_normal(p, a, b, c):
    """cross(p[b] - p[a], p[c] - p[a]) in unbounded integers"""
    e1 = [p[b][i] - p[a][i] for i in range(3)]
    e2 = [p[c][i] - p[a][i] for i in range(3)]
    return [e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]]


def figures(case, params):
    """a dict a meshlet of the model's build: nv, nt, cone (cone faces), S (the wrapped sum as three signed values, None without cone faces),
    S_exact (the sum in unbounded integers), r2, span (the widest box side), m (the least cosine, None where the contract takes none),
    raw_cutoff (int(sqrtf(1 - m*m)*127) + 2 before the clamp, None where m <= 0.1 or there is no m) and the record"""
    p = [tuple(int(x) for x in row) for row in case.P]
    m, V, T, _ = case.build(params)
    V, T = [int(x) for x in V], bytes(T)
    rec = case.bounds(params)
    out = []
    for k, (vo, to, vc, tc) in enumerate(m.tolist()):
        ids, tri = V[vo:vo + vc], T[to:to + 3 * tc]
        present = [v for v in ids if v < case.nvert]
        faces = mb.cone_faces(p, case.nvert, ids, tri)
        center = [int(x) for x in rec[k]["center"]]
        f = dict(nv=vc, nt=tc, cone=len(faces), S=None, S_exact=None, m=None, raw_cutoff=None, record=rec[k],
                 r2=max((sum((p[v][c] - center[c]) ** 2 for c in range(3)) for v in present), default=0),
                 span=max((int(rec[k]["box_max"][c]) - int(rec[k]["box_min"][c]) for c in range(3)), default=0))
        if faces:
            f["S"] = [mb._s64(sum(N[c] for *_, N in faces)) for c in range(3)]
            f["S_exact"] = [sum(exact_normal(p, a, b, c_)[c] for a, b, c_, _ in faces) for c in range(3)]
            A = [F32(int(x)) for x in rec[k]["cone_axis"]]
            if any(A):
                with np.errstate(all="ignore"):
                    la = mb._len3(A)
                    for *_, N in faces:
                        n = mb._scaled(N)
                        d = ((A[0] * n[0] + A[1] * n[1]) + A[2] * n[2]) / (la * mb._len3(n))
                        f["m"] = d if f["m"] is None or d < f["m"] else f["m"]
                    if f["m"] > F32(0.1):
                        w = F32(1.0) - f["m"] * f["m"]
                        f["raw_cutoff"] = int(np.sqrt(w if w > 0 else F32(0.0)) * F32(127.0)) + 2
                        assert min(127, f["raw_cutoff"]) == int(rec[k]["cone_cutoff"])
        out.append(f)
    return out


def row(case, params):
    """the table's row of a case"""
    fs = figures(case, params)
    S = [max(abs(x) for x in f["S"]) for f in fs if f["S"] is not None]
    return dict(meshlets=len(fs), nv=[f["nv"] for f in fs], nt=[f["nt"] for f in fs], empty=sum(1 for f in fs if not f["cone"]),
                cancelling=sum(1 for f in fs if f["cone"] and not any(f["S"])), clamped=sum(1 for f in fs if f["raw_cutoff"] is not None and f["raw_cutoff"] >= 127),
                widest_S=max(S, default=0).bit_length(), largest_r2=max(f["r2"] for f in fs).bit_length())


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. empty and cancelling cones

P_SMALL = (64, 124, 0)
P_ONE = (255, 512, 65536)


@functools.lru_cache(maxsize=None)
def coincident():
    """every position the same point: boxes of no extent, radius 0, no cone face"""
    m = synth.bumpy_sphere(16, 8)
    return Case(encode_exact(np.full((m.nvert, 3), 12345), m.index))


@functools.lru_cache(maxsize=None)
def collinear():
    """every vertex on the line x = 7 i, y = z = 0: a radius, and still no cone face"""
    m = synth.bumpy_sphere(16, 8)
    P = np.zeros((m.nvert, 3), np.int64)
    P[:, 0] = 7 * np.arange(m.nvert)
    return Case(encode_exact(P, m.index))


CLOSED_SCALE = 1000


@functools.lru_cache(maxsize=None)
def closed_one_meshlet(n):
    """closed_mesh(n) on integers: the exact normals of a closed surface sum to zero"""
    m = sc.closed_mesh(n)
    return Case(encode_exact(np.rint(m.position.astype(np.float64) * CLOSED_SCALE), m.index))


FLAT = [(axis, sign) for axis in "zxy" for sign in (1, -1)]


@functools.lru_cache(maxsize=None)
def flat_grid(axis, sign):
    """a flat 12 x 12 grid of one orientation in the plane `axis` = 0, its normal along +axis (sign 1) or, mirrored, along -axis"""
    P, idx = mb.grid(12, 12, 64)
    if sign < 0:
        idx = idx[:, [0, 2, 1]]
    P = P[:, {"z": [0, 1, 2], "x": [2, 0, 1], "y": [1, 2, 0]}[axis]]                 # (cyclic: the orientation stays)
    return Case(encode_exact(P, idx))


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the shift edge of tan_shift_of and the cutoff's clamp

P_FACE = (3, 1, 1)
SHIFT_LEGS = [(4095, 4097), (4096, 4096), (97 * 257, 673)]                            # |N| = 2^24 - 1, 2^24, 2^24 + 1
SHIFT_MAGNITUDES = [2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1]
assert [a * b for a, b in SHIFT_LEGS] == SHIFT_MAGNITUDES


# An axis-aligned normal gives the same axis under any shift, so five more faces carry a second component y beside the largest one: with
# e1 = (a, 0, 1) and e2 = (c, b, q) in the frame (u, v, axis), N = (-b, c - a q, a b).  (legs, y, the errors of the shift that change the
# record): y was searched on the CPU next to 2^24/254, where 127 y / |N| rounds to 0 or to 1 - a shift one too large drops the low bit of an
# odd y, one too small hands the float conversion a value beyond 2^24
SHIFT_TILTS = [(0, 66053, (1,)), (1, 66053, (-1,)), (1, 66054, (1,)), (2, 66053, (-1,)), (2, 66054, (1,))]


@functools.lru_cache(maxsize=None)
def shift_edge():
    """18 one-face components, each a right triangle whose normal is one of SHIFT_MAGNITUDES along one axis with one sign, and the faces of
    SHIFT_TILTS; at P_FACE a meshlet is a face and S its normal.  nface meshlets: the count equals the bound there"""
    nface = 18 + len(SHIFT_TILTS)
    m = synth.confetti(nface, max_faces=1)
    assert m.nface == nface and m.nvert == 3 * nface
    P = np.zeros((m.nvert, 3), np.int64)
    combos = [(legs, axis, sign) for legs in SHIFT_LEGS for axis in range(3) for sign in (1, -1)]
    for f, ((a, b), axis, sign) in enumerate(combos):
        u, v = (axis + 1) % 3, (axis + 2) % 3                                        # e_u x e_v = e_axis
        o = np.array([100 * f, -37 * f, 11 * f], np.int64)
        c0, c1, c2 = (int(x) for x in m.index[f])
        if sign < 0:
            c1, c2 = c2, c1
        P[c0] = o
        P[c1] = o
        P[c1, u] += a
        P[c2] = o
        P[c2, v] += b
    for t, (legs, y, _) in enumerate(SHIFT_TILTS):
        f, axis, (a, b) = 18 + t, t % 3, SHIFT_LEGS[legs]
        u, v = (axis + 1) % 3, (axis + 2) % 3
        q = -(y // a)
        o = np.array([100 * f, -37 * f, 11 * f], np.int64)
        c0, c1, c2 = (int(x) for x in m.index[f])
        P[c0] = P[c1] = P[c2] = o
        P[c1, u] += a
        P[c1, axis] += 1
        P[c2, u] += y + a * q
        P[c2, v] += b
        P[c2, axis] += q
    return Case(encode_exact(P, m.index))


def bounds_with_shift(case, params, dk):
    """the records by the model with every shift off by dk (never below 0): what a kernel that misses the shift's edge would write"""
    def scaled(X):
        mags = [abs(mb._s64(x)) for x in X]
        k = max(0, max(0, max(mags).bit_length() - 24) + dk)
        return [F32(-(mg >> k) if mb._s64(x) < 0 else (mg >> k)) for x, mg in zip(X, mags)]
    right, mb._scaled = mb._scaled, scaled
    try:
        return mb.model(case.P, *case.build(params)[:3])
    finally:
        mb._scaled = right


P_FOLD = (4, 2, 2)
# (x, z) of the two wings of a fold along y, found by a search on the CPU: the two normals are (z, 0, -x) and (-z, 0, -x) times the edge's
# length, the axis is (0, 0, -127) and the least cosine x / sqrt(x^2 + z^2).  int(sqrtf(1 - m*m)*127) + 2 is 126 for the first two, 127 and
# 128 for the others, all with m > 0.1
FOLDS = [(100, 500), (100, 470), (100, 700), (100, 900)]
FOLD_RAW = [126, 126, 127, 128]


@functools.lru_cache(maxsize=None)
def cutoff_clamp():
    """two-face components folded along their common edge; at P_FOLD a meshlet is a component"""
    P, idx = [], []
    for k, (x, z) in enumerate(FOLDS):
        o = np.array([3000 * k, 50 * k, -20 * k], np.int64)
        n = len(P)
        P += [o, o + [0, 300, 0], o + [x, 0, z], o + [-x, 300, z]]
        idx += [[n, n + 1, n + 2], [n + 1, n, n + 3]]
    return Case(encode_exact(np.array(P), np.array(idx, np.uint32)))


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. lane-stride rounds

ROUND_SCALE = 1000
VERTEX_CLASSES = [(65, 127), (128, 128), (129, 191), (192, 192), (193, 254)]
FACE_CLASSES = [(129, 191), (193, 255), (257, 319), (321, 383), (385, 447)]
# chosen on the CPU from max_vertices 65, 100, 128, 129, 192, 193, 254 at max_triangles 512: 100 adds no class to these
ROUND_PARAMS = [(65, 512, 0), (128, 512, 0), (129, 512, 0), (192, 512, 0), (193, 512, 0), (254, 512, 0)]


@functools.lru_cache(maxsize=None)
def rounds():
    m = synth.bumpy_sphere(64, 32)
    return Case(encode_exact(np.rint(m.position.astype(np.float64) * ROUND_SCALE), m.index))


def classes_hit(case, triples):
    """(vertex classes, face classes) that some meshlet of the model's builds at `triples` falls in: sets of indices"""
    hv, hf = set(), set()
    for params in triples:
        m = case.build(params)[0]
        for nv, nt in m[:, 2:].tolist():
            hv |= {i for i, (lo, hi) in enumerate(VERTEX_CLASSES) if lo <= nv <= hi}
            hf |= {i for i, (lo, hi) in enumerate(FACE_CLASSES) if lo <= nt <= hi}
    return hv, hf


FULL_NVERT = [250, 252]


@functools.lru_cache(maxsize=None)
def full_meshlet(n):
    """closed_mesh(n) with 16 of its faces a second time: 2 n + 12 faces on n vertices - 512 faces in one meshlet for n = 250, and for 252 a
    meshlet that the triangle limit cuts at 512 with the rest behind it.  (The duplicates face the way of their originals: these cones do not
    cancel)"""
    m = synth.non_manifold(sc.closed_mesh(n), fins=0, dups=16, reversed_dups=0, bowties=0, glue=0)
    return Case(encode_exact(np.rint(m.position.astype(np.float64) * CLOSED_SCALE), m.index))


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. wide values in big meshlets

WIDE_PARAMS = [(255, 512, 0), (64, 124, 0)]


@functools.lru_cache(maxsize=None)
def wide(stored_normals=True):
    """te.extreme_ends(300): positions beyond +-2^30 with random signs.  Without stored normals: its decoded integers and index encoded again
    with nothing but the position, for computed normals beside the bounds (a field of 32 bits loses bit 31 in the value coder, so this blob
    decodes to integers of its own, as wide: the conditions are asserted on both)"""
    e = te.extreme_ends(300)
    if stored_normals:
        return Case(e.blob)
    return Case(encode_exact(e.P, e.index))


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. the grid: blobs of 1, 2, 3, 4, 5, 1 meshlets behind one another

GRID_COUNTS = [1, 2, 3, 4, 5, 1]
GRID_NVERT = [34, 41, 48, 55, 62, 40]                                                 # closed meshes, all within 64 vertices


@functools.lru_cache(maxsize=None)
def grid_case(i):
    return Case(ca.encode(sc.closed_mesh(GRID_NVERT[i]), with_color=False, with_uv=False))


def grid_params(i):
    """the triangle limit that cuts blob i's 2 n - 4 faces into GRID_COUNTS[i] meshlets (the vertex limit never bites)"""
    nface = 2 * GRID_NVERT[i] - 4
    return (64, -(-nface // GRID_COUNTS[i]), 0)


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. the builder: 4 | 5 segments

SEGMENT_NVERT = 150


@functools.lru_cache(maxsize=None)
def segment_case():
    return Case(ca.encode(sc.closed_mesh(SEGMENT_NVERT), with_normal=False, with_color=False, with_uv=False))


def segment_params():
    """[(params, segments)]: segment_faces nface, ceil(nface/2), ceil(nface/4) and one less - the first value that gives five"""
    nface = 2 * SEGMENT_NVERT - 4
    q = -(-nface // 4)
    return [((64, 124, nface), 1), ((64, 124, -(-nface // 2)), 2), ((64, 124, q), 4), ((64, 124, q - 1), 5)]


# ------------------------------------------------------------------------------------------------------------------------------------

def all_cases():
    """[(id, case, [params])]: every case of sections 1 to 4 with the triples it is bound at"""
    out = [("coincident", coincident(), [P_SMALL]), ("collinear", collinear(), [P_SMALL]),
           ("closed_200", closed_one_meshlet(200), [P_ONE]), ("closed_255", closed_one_meshlet(255), [P_ONE])]
    out += [("flat_%s%s" % (a, "+" if s > 0 else "-"), flat_grid(a, s), [P_SMALL]) for a, s in FLAT]
    out += [("shift_edge", shift_edge(), [P_FACE]), ("cutoff_clamp", cutoff_clamp(), [P_FOLD]), ("rounds", rounds(), list(ROUND_PARAMS)),
            ("full_512", full_meshlet(250), [P_ONE]), ("past_512", full_meshlet(252), [P_ONE]), ("wide", wide(True), list(WIDE_PARAMS)), ("wide_no_normals", wide(False), list(WIDE_PARAMS))]
    return out
