"""The edges of computed tangents (crthip_batch_bind_computed_tangents) that the device has to meet: values past 32 bits, sums that wrap, shifts
that differ from vertex to vertex and between T and B, the far end of tan_rescale, and the block, round and slot edges of k_tangent_blob,
k_tangent_faces and k_tangent_vertex - the cases and their builders, shared by tests/test_tangent_edges_cpu.py (every case is on the side it is
named for, and the host hook equals the model on it) and tests/test_tangent_edges_gpu.py (the kernels against the model).

Every input goes through the encoder; the reference is the numpy model of tests/computed_tangents.py on the oracle's integers (ct.Inputs).
Exact integers come from position_bits = 0, position_q = 1, uv_bits = 0 (EXACT); an integer uv beyond a float's mantissa goes in as a DOUBLE
generic attribute named "uv"."""
import functools
import tempfile

import numpy as np

import corto_amd as ca
import computed_tangents as ct
import quantized_outputs as qo
import size_classes as sc
from corto_amd import synth

EXACT = dict(position_bits=0, position_q=1.0, uv_bits=0)
DEEP = dict(position_bits=20, uv_bits=16)
FALLBACK_CAP = 4                     # fallback vertices a blob: a test whose answer is mostly (1, 0, 0, 1) proves nothing
TOP = (1 << 31) - 1


@functools.lru_cache(maxsize=None)
def constants():
    """TANGENT_BLOB_MAX, TAN_BLOCK, TAN_THREADS and TAN_ROUND*TAN_THREADS by the library's own headers (tests/cpp/tangent_probe.cpp)"""
    with tempfile.TemporaryDirectory(prefix="tangent_probe") as d:
        p = sc.Probe(d, source="tangent_probe")
        try:
            return {n: p.const(n) for n in ("TANGENT_BLOB_MAX", "TAN_BLOCK", "TAN_THREADS", "TAN_ROUND_FACES")}
        finally:
            p.close()


def blob_max():
    return constants()["TANGENT_BLOB_MAX"]


def one_workgroup(nvert):
    return nvert <= blob_max()


# ------------------------------------------------------------------------------------------------------------------------------------
# what a case reaches, measured on the oracle's integers

class Figures:
    """k a vertex, kT and kB (the shift T alone and B alone ask for: k_tangent_blob rescales T by d = k - kT), the fallback mask, det a face"""

    def __init__(self, e):
        T, B, det = e.sums()
        zero = np.zeros_like(T)
        self.k = ct.shifts(T, B).astype(np.int64)
        self.kT, self.kB = ct.shifts(T, zero).astype(np.int64), ct.shifts(zero, B).astype(np.int64)
        self.d = self.k - self.kT
        self.T_kept = np.abs(ct.scaled(T, self.kT.astype(np.uint64))).max(axis=1) > 0      # what tan_blob_keep_T leaves is not all zero
        self.fallback = e.model(ca.FMT_FLOAT)[1]
        self.det = det
        self.widest = int(np.abs(np.concatenate([T, B], 1)).view(np.uint64).max()).bit_length() if len(T) else 0

    def row(self):
        """the table's row: k, vertices with kT < kB and kT > kB, the largest kB - kT and kT - kB, fallback vertices, the widest |sum| in bits"""
        return dict(k=(int(self.k.min()), int(self.k.max())), kT_lt_kB=int((self.kT < self.kB).sum()), kT_gt_kB=int((self.kT > self.kB).sum()),
                    max_kB_kT=int((self.kB - self.kT).max()), max_kT_kB=int((self.kT - self.kB).max()), fallback=int(self.fallback.sum()),
                    widest=self.widest)


def exact_sums_differ(P, t, index):
    """vertices whose T or B, summed in Python's unbounded integers, is not what int64 holds: the wrap happened"""
    Pl, tl = np.asarray(P).astype(object), np.asarray(t).astype(object)
    idx = np.asarray(index).astype(np.int64)
    a, b, c = idx[:, 0], idx[:, 1], idx[:, 2]
    e1, e2, d1, d2 = Pl[b] - Pl[a], Pl[c] - Pl[a], tl[b] - tl[a], tl[c] - tl[a]
    s1, r1, s2, r2 = d1[:, :1], d1[:, 1:], d2[:, :1], d2[:, 1:]
    det = (s1 * r2 - s2 * r1)[:, 0]
    sg = np.array([(x > 0) - (x < 0) for x in det], dtype=object)[:, None]
    Tf, Bf = sg * (e1 * r2 - e2 * r1), sg * (e2 * s1 - e1 * s2)
    T, B = np.zeros((len(Pl), 3), object), np.zeros((len(Pl), 3), object)
    for k in range(3):
        np.add.at(T, idx[:, k], Tf)
        np.add.at(B, idx[:, k], Bf)
    got = ct.accumulate(P, t, index)
    exact = np.concatenate([T, B], 1)
    held = np.concatenate([got[0], got[1]], 1).astype(object)
    return int((exact != held).any(axis=1).sum())


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. value edges

def _ends(n, rng):
    """uvs at or next to +-(2^31 - 1): differences of 33 bits"""
    st = np.where(rng.random((n, 2)) < 0.5, -1, 1).astype(np.int64)
    t = st * (TOP - rng.integers(0, 4096, (n, 2)))
    t[::17] = st[::17] * TOP
    return t


def _uv_blob(mesh, P, t):
    pos = P.astype(np.float32)
    assert (pos.astype(np.int64) == P).all()
    return ct.Inputs(ca.encode(synth.Mesh(pos, mesh.index, mesh.normal, mesh.color, None), with_color=False, with_uv=False, normal_prediction=ca.BORDER,
                               position_bits=0, position_q=1.0, attributes=[("uv", t.astype(np.float64), 1.0, 0)]))


@functools.lru_cache(maxsize=None)
def extreme_ends(nvert, seed=11):
    """closed_mesh(nvert) with every uv at or next to +-(2^31 - 1) (a DOUBLE generic "uv": exact) and every position beyond +-2^30 with a random
    sign, the largest a float32 input and the reference's value coder take: a field of 32 bits loses bit 31 there (corto_amd.synth.
    full_width_values), so what decodes is spread over all of int32, both ends included - the blob is what the oracle makes of it"""
    m = sc.closed_mesh(nvert)
    rng = np.random.default_rng(seed)
    sp = np.where(rng.random((m.nvert, 3)) < 0.5, -1, 1).astype(np.int64)
    return _uv_blob(m, sp * ((1 << 30) + 128 * rng.integers(0, 1 << 13, (m.nvert, 3))), _ends(m.nvert, rng))


RESCALE_CENTRES = 3


@functools.lru_cache(maxsize=None)
def extreme_rescale(nvert, seed=5):
    """the far end of tan_rescale: uvs as extreme_ends, positions of 26 bits (multiples of 4: exact as float32, and no field of 31 or 32 bits, so they
    decode as given), and RESCALE_CENTRES vertices, far apart, on whose ring of faces the positions are g*v + a few units with v a handful: the
    g*v part cancels in T, which stays below 2^24 (kT = 0) and not zero, while B = g * sum |det| passes 2^56: d = k - kT >= 32.  T shifts to
    nothing there, so these vertices are fallbacks by the contract - which is why there are three of them and no more"""
    m = sc.closed_mesh(nvert)
    n = m.nvert
    rng = np.random.default_rng(seed)
    sp = np.where(rng.random((n, 3)) < 0.5, -1, 1).astype(np.int64)
    P = sp * ((1 << 25) + 4 * rng.integers(0, 1 << 22, (n, 3)))
    t = _ends(n, rng)
    idx = m.index.astype(np.int64)
    g = np.array([1 << 21, -(1 << 20), 3 << 19], np.int64)
    for c in [n // 7, n // 2 + 3, (6 * n) // 7][:RESCALE_CENTRES]:
        ring = np.unique(idx[(idx == c).any(axis=1)])
        v = rng.permutation(len(ring)) - len(ring) // 2
        P[ring] = v[:, None] * g[None, :] + rng.integers(-9, 10, (len(ring), 3))
        t[ring, 1] = TOP - 16 + v                                               # (next to an end like its neighbours': only differences count)
    return _uv_blob(m, P, t)


@functools.lru_cache(maxsize=None)
def full_width(nvert):
    return ct.Inputs(ct.encode(synth.full_width_values(sc.closed_mesh(nvert), seed=37), **EXACT))


@functools.lru_cache(maxsize=None)
def deep(nvert):
    return ct.Inputs(ct.encode(sc.closed_mesh(nvert), **DEEP))


# (id, builder, nvert): each in both size classes
VALUE_CASES = [("full_width_2304", full_width, 2304), ("full_width_2305", full_width, 2305), ("full_width_3073", full_width, 3073),
               ("deep_2304", deep, 2304), ("deep_2305", deep, 2305), ("extreme_ends_2304", extreme_ends, 2304), ("extreme_ends_2305", extreme_ends, 2305),
               ("extreme_rescale_2304", extreme_rescale, 2304), ("extreme_rescale_2305", extreme_rescale, 2305)]
VALUE_IDS = [c[0] for c in VALUE_CASES]


def value_case(cid):
    _, make, nvert = VALUE_CASES[VALUE_IDS.index(cid)]
    return make(nvert)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. an affine sheet through a blob: the answer is known without the model

A = np.array([[3, 1], [1, 4], [-2, 2]], dtype=np.int64)          # columns (3, 1, -2) and (1, 4, 2), as tests/test_computed_tangents_cpu.py
SHEETS = [8, 49]                                                 # 64 vertices (one workgroup) and 2 401 (batch-wide)
SHEET_BOUND = 1e-6                                               # a few float32 roundings of a unit vector, 2^-24 each


@functools.lru_cache(maxsize=None)
def sheet(n, negate_u=False):
    """an n x n grid: positions (uv @ A.T) << 20, uvs << 14 (u negated on request), the stored normal the plane's"""
    g = np.arange(n)
    u, v = [x.reshape(-1) for x in np.meshgrid(g, g, indexing="ij")]
    uv = np.stack([u, v], 1).astype(np.int64)
    P = (uv @ A.T) << 20
    if negate_u:
        uv = uv * [-1, 1]
    at = lambda i, j: i * n + j
    faces = [f for i in range(n - 1) for j in range(n - 1) for f in ((at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1)))]
    nrm = np.cross(A[:, 0], A[:, 1]).astype(np.float64)
    nrm = np.tile(nrm / np.linalg.norm(nrm), (n * n, 1)).astype(np.float32)
    pos, tex = P.astype(np.float32), (uv << 14).astype(np.float32)
    assert (pos.astype(np.int64) == P).all() and (tex.astype(np.int64) == uv << 14).all()
    return ct.Inputs(ct.encode(synth.Mesh(pos, np.array(faces, np.uint32), nrm, None, tex), **EXACT))


def sheet_answer(normal, negate_u=False):
    """A[:, 0] made orthogonal to the decoded normal and normalised, in float64, and w: (xyz, w)"""
    nd = np.asarray(normal, np.float64)
    a0 = A[:, 0].astype(np.float64)
    x = a0 - nd * (nd @ a0) / (nd @ nd)
    x /= np.linalg.norm(x)
    return (-x, -1.0) if negate_u else (x, 1.0)


def sheet_deviation(tangent, normals, negate_u=False):
    """the largest |component - answer| over the vertices of FLOAT tangents, each against its own decoded normal; asserts w"""
    worst = 0.0
    for nrm in np.unique(np.asarray(normals), axis=0):
        x, w = sheet_answer(nrm, negate_u)
        rows = (np.asarray(normals) == nrm).all(axis=1)
        assert (tangent[rows, 3] == w).all()
        worst = max(worst, float(np.abs(tangent[rows, :3].astype(np.float64) - x).max()))
    return worst


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. block, round and slot edges: (id, mesh, encode keywords, nvert, nface)

def tetrahedron():
    """the smallest closed mesh: four vertices, four faces"""
    pos = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32) * 0.5
    idx = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.uint32)
    nrm = (pos / np.linalg.norm(pos, axis=1, keepdims=True)).astype(np.float32)
    uv = np.array([[0.1, 0.1], [0.9, 0.2], [0.3, 0.8], [0.7, 0.6]], np.float32)
    return synth.Mesh(pos, idx, nrm, None, uv)


def _closed(nvert):
    return lambda: sc.closed_mesh(nvert)


def _open(nvert, holes):
    return lambda: sc.open_mesh(nvert, holes)


# k_tangent_faces: nface around 6 x TAN_BLOCK (the last block full, one face short of full, a single face);
# k_tangent_vertex: nvert around 3 x TAN_BLOCK; one of them on the deep grid
WIDE_EDGES = [("faces_6143", _open(3074, 1), {}, 3074, 6143), ("faces_6144", _closed(3074), {}, 3074, 6144), ("faces_6145", _open(3075, 1), {}, 3075, 6145),
              ("vertices_3071", _closed(3071), {}, 3071, 6138), ("vertices_3072", _closed(3072), {}, 3072, 6140), ("vertices_3073", _closed(3073), {}, 3073, 6142),
              ("vertices_3073_deep", _closed(3073), DEEP, 3073, 6142)]
# k_tangent_blob: nface around one and two face rounds (TAN_ROUND*TAN_THREADS faces), nvert around a lane's first slot, the smallest mesh
BLOB_EDGES = [("round_1023", _open(514, 1), {}, 514, 1023), ("round_1024", _closed(514), {}, 514, 1024), ("round_1025", _open(515, 1), {}, 515, 1025),
              ("round_2047", _open(1026, 1), {}, 1026, 2047), ("round_2048", _closed(1026), {}, 1026, 2048), ("round_2049", _open(1027, 1), {}, 1027, 2049),
              ("slots_255", _closed(255), {}, 255, 506), ("slots_256", _closed(256), {}, 256, 508), ("slots_257", _closed(257), {}, 257, 510),
              ("tetrahedron", tetrahedron, {}, 4, 4)]
EDGE_CASES = WIDE_EDGES + BLOB_EDGES
EDGE_IDS = [c[0] for c in EDGE_CASES]


@functools.lru_cache(maxsize=None)
def edge_case(cid):
    _, make, kw, nvert, nface = EDGE_CASES[EDGE_IDS.index(cid)]
    e = ct.Inputs(ct.encode(make(), **kw))
    assert (e.nvert, e.nface) == (nvert, nface), (cid, e.nvert, e.nface)
    return e


@functools.lru_cache(maxsize=None)
def bystanders():
    """a point cloud and a mesh without uv: in the batch, and simply without a tangent"""
    return ca.aligned_blob(ca.encode(synth.point_cloud(20, 10), normal_prediction=ca.DIFF)), ca.aligned_blob(ca.encode(synth.icosphere(1), with_uv=False))


def one_batch():
    """every batch-wide edge case in one batch (fblock0, vblock0 and the tan_acc offsets are non-zero for all but the first), two one-workgroup
    blobs and the two bystanders between them: [(id or None, blob)]"""
    cloud, no_uv = bystanders()
    ids = [c[0] for c in WIDE_EDGES]
    order = ids[:2] + ["round_1025", None] + ids[2:5] + [None, "slots_257"] + ids[5:]
    extra = iter([cloud, no_uv])
    return [(cid, edge_case(cid).blob if cid else next(extra)) for cid in order]


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. the batch-wide path beside what it shares scratch or buffers with

@functools.lru_cache(maxsize=None)
def sized(nvert, normals="float"):
    e = ct.Inputs(ct.encode(sc.closed_mesh(nvert), normals=normals))
    assert e.nvert == nvert
    return e


def unfused_nvert():
    return sc.FUSED_LAST + 1


def record_nvert():
    """a blob above TANGENT_BLOB_MAX and above the quantised outputs' one-workgroup limit"""
    return max(blob_max(), qo.blob_max()) + 1


BIG = [(32768, True), (65535, True), (65537, False)]                 # (nvert, uint16 index)
COMPANIONS = [1500, 2400, 3000]                                      # stored normals: beside the blobs above in a batch


def companions():
    """[(inputs, stored normals)] of every other blob the batches of section 4 hold"""
    return [(sized(n), True) for n in COMPANIONS + [record_nvert()]] + [(sized(n, "computed"), False) for n in (1500, 2400, unfused_nvert())]
