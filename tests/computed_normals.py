"""Computed normals (crthip_batch_bind_computed_normals): the model of the value, the blobs and what each must decode to - shared by
tests/test_computed_normals_cpu.py (the model against the oracle) and tests/test_computed_normals_gpu.py (the kernels against both).

A mesh encoded without normals and the same mesh encoded with BORDER normals (its "twin") decode to the same positions and index, and
upstream's decoder leaves est/|est| at every vertex of the twin that is off the boundary: there the oracle's decode of the twin is the
expected value.  On the boundary, and where the estimate is zero (upstream: 0/0, or nothing written), the model below is."""
import functools

import numpy as np

import corto_amd as ca
from corto_amd import synth
from oracle import oracle as oc

FILL = 0xA5


def estimate(P, index):
    """estimateNormals (src/normal_attribute.cpp:40-59) in float32: per-face cross products of the INTEGER positions as floats
    (include/corto/point.h:113-115: every product and difference rounded on its own, no FMA), added per vertex face after face - three
    += a face, in face order, so that a face naming a vertex twice adds twice."""
    Pf = np.asarray(P).astype(np.float32)
    idx = np.asarray(index).astype(np.int64)
    p0 = Pf[idx[:, 0]]
    u, v = Pf[idx[:, 1]] - p0, Pf[idx[:, 2]] - p0
    n = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
    assert n.dtype == np.float32
    est = [[np.float32(0), np.float32(0), np.float32(0)] for _ in range(len(Pf))]
    for f in range(len(idx)):
        nx, ny, nz = n[f]
        for w in idx[f]:
            e = est[w]
            e[0] += nx; e[1] += ny; e[2] += nz
    return np.array(est, dtype=np.float32).reshape(len(Pf), 3)


def lengths(est):
    s = est[:, 0] * est[:, 0] + est[:, 1] * est[:, 1]
    s = s + est[:, 2] * est[:, 2]
    return np.sqrt(s)


def model(P, index, fmt):
    """the computed normal of every vertex: est/len, or (int16_t)(est*(32767.0f/len)); a zero estimate gives (0,0,1) / (0,0,32767)"""
    est = estimate(P, index)
    ln = lengths(est)
    assert ln.dtype == np.float32
    zero = ln < np.float32(0.00001)
    with np.errstate(divide="ignore", invalid="ignore"):
        if fmt == ca.FMT_FLOAT:
            out = est / ln[:, None]
            out[zero] = (0.0, 0.0, 1.0)
        else:
            l = np.float32(32767.0) / ln
            v = est * l[:, None]
            v[zero] = 0
            out = np.trunc(v).astype(np.int32).astype(np.int16)          # cvttss2si, then the int16_t conversion
            out[zero] = (0, 0, 32767)
    return out, zero


def boundary(index, nvert):
    """markBoundary (src/normal_attribute.cpp:24-37): the XOR of every vertex's neighbours over its faces; non-zero = boundary"""
    idx = np.asarray(index).astype(np.uint32)
    b = np.zeros(nvert, dtype=np.uint32)
    a, bb, c = idx[:, 0], idx[:, 1], idx[:, 2]
    np.bitwise_xor.at(b, a, bb ^ c)
    np.bitwise_xor.at(b, bb, c ^ a)
    np.bitwise_xor.at(b, c, a ^ bb)
    return b != 0


# ------------------------------------------------------------------------------------------------------------------------------------
# the meshes

MESHES = {
    "torus_24_12": lambda: synth.torus(24, 12),
    "icosphere_2": lambda: synth.icosphere(2),
    "closed_sphere": lambda: synth.closed_sphere(),
    "holey_disc_20": lambda: synth.holey_disc(20),
    "bumpy_sphere_16_8": lambda: synth.bumpy_sphere(16, 8),
    "torus_105_105": lambda: synth.torus(105, 105),
    "torus_182_182": lambda: synth.torus(182, 182),
    "torus_48_24": lambda: synth.torus(48, 24),
    "icosphere_3": lambda: synth.icosphere(3),
}
LOOPED = ["torus_24_12", "icosphere_2", "closed_sphere", "holey_disc_20", "bumpy_sphere_16_8"]        # small enough for the model's loop on the CPU
CLOSED = ["torus_24_12", "icosphere_2", "closed_sphere"]
OPEN = ["holey_disc_20", "bumpy_sphere_16_8"]
DEGENERATE = [("torus_48_24", 3, 735, 1152), ("icosphere_3", 3, 200, 642)]       # (mesh, position_bits, vertices with a zero estimate, nvert)


def twins_of(mesh, **kw):
    """(the blob without normals, its BORDER twin)"""
    bare = ca.encode(mesh, with_normal=False, with_color=False, with_uv=False, **kw)
    twin = ca.encode(mesh, with_normal=True, normal_prediction=ca.BORDER, with_color=False, with_uv=False, **kw)
    return bare, twin


@functools.lru_cache(maxsize=None)
def twins(name, position_bits=14):
    return twins_of(MESHES[name](), position_bits=position_bits)


class Expected:
    """what a blob without normals must decode to with computed normals: position / index as the oracle decodes the blob itself; the
    normal: the oracle's decode of the twin where upstream defines it (off the boundary, a non-zero estimate), the model's elsewhere"""

    def __init__(self, bare, twin):
        self.bare, self.twin = bare, twin
        tr = oc.decode(bare, trace=True)
        self.nvert, self.nface = tr["nvert"], tr["nface"]
        self.P = tr["_delta_position"]                                   # the integer positions, delta-decoded
        self.index = tr["index"]
        self.position = tr["position"]
        self.bnd = boundary(self.index, self.nvert)
        ref = oc.decode(twin, normal_format=ca.FMT_FLOAT)
        self.degenerate = np.isnan(ref["normal"]).any(axis=1) & ~self.bnd   # upstream's 0/0 (a boundary vertex takes a correction instead)
        self.defined = ~self.bnd & ~self.degenerate
        self._model = {}

    def model(self, fmt):
        if fmt not in self._model:
            self._model[fmt] = model(self.P, self.index, fmt)
        return self._model[fmt]

    def normal(self, fmt):
        ref = oc.decode(self.twin, normal_format=fmt)["normal"]
        exp = ref.copy()
        exp[self.degenerate] = (0, 0, 1) if fmt == ca.FMT_FLOAT else (0, 0, 32767)
        if self.bnd.any():
            exp[self.bnd] = self.model(fmt)[0][self.bnd]
        return exp

    def outputs(self, fmt=ca.FMT_FLOAT, index16=False):
        return {"position": self.position, "normal": self.normal(fmt), "index": self.index.astype(np.uint16) if index16 else self.index}


@functools.lru_cache(maxsize=None)
def expected(name, position_bits=14):
    return Expected(*twins(name, position_bits))


def assert_same(got, exp, keys, tag):
    for k in keys:
        a, e = np.asarray(got[k]), np.asarray(exp[k])
        assert a.dtype == e.dtype and a.shape == e.shape, (tag, k, a.dtype, e.dtype, a.shape, e.shape)
        if a.tobytes() != e.tobytes():
            av, ev = a.reshape(len(a), -1), e.reshape(len(e), -1)
            bad = np.unique(np.argwhere(av.view(np.uint8) != ev.view(np.uint8))[:, 0])
            raise AssertionError("%s %s: %d mismatching rows, first %d got %s expected %s" % (tag, k, len(bad), bad[0], av[bad[0]], ev[bad[0]]))
