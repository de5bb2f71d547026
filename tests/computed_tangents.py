"""Computed tangents (crthip_batch_bind_computed_tangents): the numpy model of the value in include/corto_hip.h, the blobs and the inputs -
shared by tests/test_computed_tangents_cpu.py (the kernels' source on the host, corto_amd.tangent_model, against the model) and
tests/test_computed_tangents_gpu.py (the kernels against the model).

Inputs are the oracle's: `_delta_position` / `_delta_uv` of its trace are the delta-decoded integers, `normal` its decoded normals in the
format the batch binds them in.  The per-face terms are summed in int64 (numpy wraps modulo 2^64 as the contract says), the per-vertex
finish is explicit float32 steps.  Tolerance 0 everywhere: the kernels must give the model's bytes."""
import functools

import numpy as np

import corto_amd as ca
from corto_amd import synth
from oracle import oracle as oc

FILL = 0xA5
E_NEEDS_POSITION, E_FORMAT, E_ARGUMENT = -6, -7, -8
F32 = np.float32


def face_terms(P, t, index):
    """(Tf, Bf, det) a face: int64, wrapping"""
    P, t, idx = np.asarray(P).astype(np.int64), np.asarray(t).astype(np.int64), np.asarray(index).astype(np.int64).reshape(-1, 3)
    a, b, c = idx[:, 0], idx[:, 1], idx[:, 2]
    with np.errstate(over="ignore"):
        e1, e2 = P[b] - P[a], P[c] - P[a]
        d1, d2 = t[b] - t[a], t[c] - t[a]
        s1, r1, s2, r2 = d1[:, :1], d1[:, 1:], d2[:, :1], d2[:, 1:]
        det = s1 * r2 - s2 * r1
        sg = (det > 0).astype(np.int64) - (det < 0).astype(np.int64)
        Tf = sg * (e1 * r2 - e2 * r1)
        Bf = sg * (e2 * s1 - e1 * s2)
    return Tf, Bf, det[:, 0]


def accumulate(P, t, index, order=None):
    """T[v], B[v]: the face terms added to a, b and c (a face that names a vertex twice adds twice), faces in `order`"""
    idx = np.asarray(index).astype(np.int64).reshape(-1, 3)
    Tf, Bf, det = face_terms(P, t, idx)
    if order is not None:
        idx, Tf, Bf = idx[order], Tf[order], Bf[order]
    T, B = np.zeros((len(P), 3), np.int64), np.zeros((len(P), 3), np.int64)
    for k in range(3):
        np.add.at(T, idx[:, k], Tf)
        np.add.at(B, idx[:, k], Bf)
    return T, B, det


def shifts(T, B):
    """k a vertex: max(0, bitlength(max |x| over the six components) - 24); |INT64_MIN| is 2^63"""
    m = np.abs(np.concatenate([T, B], 1)).view(np.uint64).max(axis=1) if len(T) else np.zeros(0, np.uint64)
    return np.array([max(0, int(x).bit_length() - 24) for x in m], dtype=np.uint64)


def scaled(X, k):
    """sign(x)*(|x| >> k) as float32 (exact: below 2^24)"""
    mag = (np.abs(X).view(np.uint64) >> k[:, None]).astype(np.int64)
    v = np.where(X < 0, -mag, mag)
    assert (np.abs(v) < 1 << 24).all()
    return v.astype(F32)


def f2s(x):
    """float -> int16 by the rule of the INT16 normals: truncation; out of int32's range or NaN gives INT32_MIN, whose low half is 0"""
    with np.errstate(invalid="ignore"):
        ok = (x > F32(-2147483904.0)) & (x < F32(2147483648.0))
        i = np.where(ok, np.trunc(np.where(ok, x, 0)), -2.0 ** 31).astype(np.int64)
    return (i & 0xFFFF).astype(np.uint16).view(np.int16)


def finish(T, B, normal, fmt):
    """the per-vertex value from the sums and the normals as bound (float32, or int16 converted without rescaling): ((nvert, 4), fallback mask, k)"""
    k = shifts(T, B)
    Tf, Bf = scaled(T, k), scaled(B, k)
    n = np.asarray(normal)
    assert n.dtype in (np.float32, np.int16)
    n = n.astype(F32)
    nx, ny, nz = n[:, 0], n[:, 1], n[:, 2]
    with np.errstate(all="ignore"):
        nn = (nx * nx + ny * ny) + nz * nz
        nt = (nx * Tf[:, 0] + ny * Tf[:, 1]) + nz * Tf[:, 2]
        u = Tf * nn[:, None] - n * nt[:, None]
        ux, uy, uz = u[:, 0], u[:, 1], u[:, 2]
        ln = np.sqrt((ux * ux + uy * uy) + uz * uz)
        cx, cy, cz = ny * uz - nz * uy, nz * ux - nx * uz, nx * uy - ny * ux
        h = (cx * Bf[:, 0] + cy * Bf[:, 1]) + cz * Bf[:, 2]
        for a in (nn, nt, u, ln, cx, h):
            assert a.dtype == F32
        minus = h < 0
        ok = np.isfinite(ln) & (ln > 0)
        if fmt == ca.FMT_FLOAT:
            out = np.empty((len(T), 4), F32)
            out[:, :3] = u / ln[:, None]
            out[:, 3] = np.where(minus, F32(-1), F32(1))
            out[~ok] = (1, 0, 0, 1)
        else:
            l = F32(32767.0) / ln
            out = np.empty((len(T), 4), np.int16)
            out[:, :3] = f2s(u * l[:, None])
            out[:, 3] = np.where(minus, -32767, 32767)
            out[~ok] = (32767, 0, 0, 32767)
    return out, ~ok, k


def model(P, t, index, normal, fmt, order=None):
    T, B, _ = accumulate(P, t, index, order)
    return finish(T, B, normal, fmt)[0]


def strided(records, stride, fill=FILL, offset=0):
    """(nvert, 4) records laid out every `stride` bytes from byte `offset` of a buffer otherwise full of `fill`: the bytes a strided store must leave"""
    r = np.ascontiguousarray(records)
    w = r.shape[1] * r.itemsize
    buf = np.full(offset + ((len(r) - 1) * stride + w if len(r) else 0), fill, np.uint8)
    if len(r):
        np.lib.stride_tricks.as_strided(buf[offset:], shape=(len(r), w), strides=(stride, 1))[:] = r.view(np.uint8).reshape(len(r), w)
    return buf


# ------------------------------------------------------------------------------------------------------------------------------------
# the meshes of the contract's table: (fallback vertices, faces with det < 0, faces with det == 0) at 14-bit positions and 12-bit uvs

MESHES = {
    "torus_24_12": lambda: synth.torus(24, 12),
    "icosphere_2": lambda: synth.icosphere(2),
    "closed_sphere": lambda: synth.closed_sphere(),
    "holey_disc_20": lambda: synth.holey_disc(20),
    "bumpy_sphere_16_8": lambda: synth.bumpy_sphere(16, 8),
}
TABLE = {"torus_24_12": (0, 68, 0), "icosphere_2": (0, 174, 0), "closed_sphere": (2, 20, 48), "holey_disc_20": (2, 0, 0), "bumpy_sphere_16_8": (0, 16, 0)}
NAMES = list(MESHES)


def table_counts(name):
    """the table's row measured: the synth mesh itself, quantised with the steps its blob carries (the encoder drops holey_disc's two
    unreferenced vertices and renumbers the rest, so the oracle's arrays have 439): (nvert, fallback vertices, det < 0, det == 0)"""
    m = MESHES[name]()
    q = {a["name"]: F32(a["q"]) for a in oc.parse_header(inputs(name).blob)["attrs"]}
    P = np.rint(m.position.astype(np.float64) / q["position"]).astype(np.int64)
    t = np.rint(m.uv.astype(np.float64) / q["uv"]).astype(np.int64)
    T, B, det = accumulate(P, t, m.index)
    fb = finish(T, B, np.ascontiguousarray(m.normal, F32), ca.FMT_FLOAT)[1]
    return m.nvert, int(fb.sum()), int((det < 0).sum()), int((det == 0).sum())


def encode(mesh, normals="float", **kw):
    """normals: "float" / "int16" - stored BORDER normals (bound in that format); "computed" - none stored (crthip_batch_bind_computed_normals)"""
    return ca.encode(mesh, with_color=False, with_normal=normals != "computed", normal_prediction=ca.BORDER, **kw)


class Inputs:
    """what the tangents of `blob` are made of, by the oracle: the integers, the index, the normals in both formats"""

    def __init__(self, blob):
        self.blob = ca.aligned_blob(blob)
        tr = oc.decode(self.blob, trace=True)
        self.tr = tr
        self.nvert, self.nface = tr["nvert"], tr["nface"]
        self.P, self.t, self.index = tr["_delta_position"], tr["_delta_uv"], tr["index"]
        self._normal = {ca.FMT_FLOAT: tr["normal"]} if "normal" in tr else {}
        self._model = {}

    def normal(self, nfmt):
        if nfmt not in self._normal:
            self._normal[nfmt] = oc.decode(self.blob, normal_format=nfmt)["normal"]
        return self._normal[nfmt]

    def sums(self):
        if "sums" not in self._model:
            self._model["sums"] = accumulate(self.P, self.t, self.index)
        return self._model["sums"]

    def model(self, fmt, nfmt=ca.FMT_FLOAT, normal=None):
        """(tangents, fallback mask, k); `normal`: normals from elsewhere (computed ones), never cached"""
        T, B, _ = self.sums()
        if normal is not None:
            return finish(T, B, normal, fmt)
        if (fmt, nfmt) not in self._model:
            self._model[(fmt, nfmt)] = finish(T, B, self.normal(nfmt), fmt)
        return self._model[(fmt, nfmt)]


@functools.lru_cache(maxsize=None)
def inputs(name):
    return Inputs(encode(MESHES[name]()))


def assert_bytes(got, exp, tag):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (tag, got.dtype, exp.dtype, got.shape, exp.shape)
    if got.tobytes() != exp.tobytes():
        g, e = got.reshape(len(got), -1), exp.reshape(len(exp), -1)
        bad = np.unique(np.argwhere(g.view(np.uint8) != e.view(np.uint8))[:, 0])
        raise AssertionError("%s: %d mismatching rows, first %d got %s expected %s" % (tag, len(bad), bad[0], g[bad[0]], e[bad[0]]))
