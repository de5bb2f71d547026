"""CPU: computed tangents (crthip_batch_bind_computed_tangents) - the kernels' source on the host (corto_amd.tangent_model: csrc/tangent.h in
k_tangent.hip's partitions) against the numpy model of the contract (tests/computed_tangents.py), byte for byte; an affine sheet whose
answer is known without the model; the edges of the value; the contract's table; the declaration.  No kernel runs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import corto_amd as ca
import computed_tangents as ct
from conftest import ROOT
from corto_amd import synth

FMTS = [(ca.FMT_FLOAT, "f32"), (ca.FMT_INT16, "i16")]
STRIDE = {ca.FMT_FLOAT: 32, ca.FMT_INT16: 12}


def hook_equals_model(P, t, index, normal, tag, whichs=(0, 1), seeds=(1, 2, 3)):
    """every partition, seed, output format and layout of the hook against the model; returns the FLOAT tangents"""
    res = None
    for fmt, _ in FMTS:
        exp = ct.model(P, t, index, normal, fmt)
        if fmt == ca.FMT_FLOAT:
            assert not np.isnan(exp).any(), tag
            res = exp
        for which in whichs:
            for seed in seeds:
                got = ca.tangent_model(P, t, index, normal, fmt=fmt, which=which, seed=seed)
                ct.assert_bytes(got, exp, (tag, fmt, which, seed, "packed"))
                st = STRIDE[fmt]
                want = ct.strided(exp, st, offset=st - 4)                       # records inside a filled buffer: nothing between them may change
                buf = np.full(len(want), ct.FILL, np.uint8)
                ca.tangent_model(P, t, index, normal, fmt=fmt, stride=st, which=which, seed=seed, out=buf, offset=st - 4)
                assert buf.tobytes() == want.tobytes(), (tag, fmt, which, seed, "strided")
    return res


# ---- 1. hook equals model, byte for byte ----

@pytest.mark.parametrize("nfmt", [f for f, _ in FMTS], ids=["normal_" + n for _, n in FMTS])
@pytest.mark.parametrize("name", ct.NAMES)
def test_hook_equals_model(name, nfmt):
    e = ct.inputs(name)
    hook_equals_model(e.P, e.t, e.index, e.normal(nfmt), (name, nfmt))
    if nfmt == ca.FMT_FLOAT:                                                    # a uint16 index reads the same faces
        got = ca.tangent_model(e.P, e.t, e.index.astype(np.uint16), e.normal(nfmt), which=1, seed=5)
        ct.assert_bytes(got, e.model(ca.FMT_FLOAT, nfmt)[0], (name, "u16 index"))


def test_face_order_does_not_matter():
    """permuting the faces leaves T and B unchanged (integer sums), hence every byte"""
    e = ct.inputs("torus_24_12")
    T, B, _ = e.sums()
    order = np.random.RandomState(7).permutation(e.nface)
    T2, B2, _ = ct.accumulate(e.P, e.t, e.index, order)
    assert (T == T2).all() and (B == B2).all()
    got = ca.tangent_model(e.P, e.t, e.index[order], e.normal(ca.FMT_FLOAT), which=1, seed=9)
    ct.assert_bytes(got, e.model(ca.FMT_FLOAT)[0], "permuted faces")


# ---- 2. independent of the model: an affine sheet ----

A = np.array([[3, 1], [1, 4], [-2, 2]], dtype=np.int64)          # columns (3, 1, -2) and (1, 4, 2): their dot product is 3, not orthogonal


def sheet(negate_u=False):
    g = np.arange(8)
    u, v = [x.reshape(-1) for x in np.meshgrid(g, g, indexing="ij")]
    uv = np.stack([u, v], 1).astype(np.int64)
    P = uv @ A.T
    if negate_u:
        uv = uv * [-1, 1]
    at = lambda i, j: i * 8 + j
    faces = [f for i in range(7) for j in range(7) for f in ((at(i, j), at(i + 1, j), at(i + 1, j + 1)), (at(i, j), at(i + 1, j + 1), at(i, j + 1)))]
    n = np.cross(A[:, 0], A[:, 1]).astype(np.float64)
    return P.astype(np.int32), uv.astype(np.int32), np.array(faces, np.uint32), n


@pytest.mark.parametrize("normal_kind", ["unit_f32", "integer_i16"])
def test_affine_sheet(normal_kind):
    P, uv, idx, n = sheet()
    nrm = np.tile(n / np.linalg.norm(n), (64, 1)).astype(np.float32) if normal_kind == "unit_f32" else np.tile(n, (64, 1)).astype(np.int16)
    nd = nrm[0].astype(np.float64)
    a0, a1 = A[:, 0].astype(np.float64), A[:, 1].astype(np.float64)
    x = a0 - nd * (nd @ a0) / (nd @ nd)                                         # A[:,0] made orthogonal to n ...
    x /= np.linalg.norm(x)                                                      # ... and normalised
    w = np.sign(np.cross(nd, a0) @ a1)
    assert w == 1.0
    for which in (0, 1):
        got = ca.tangent_model(P, uv, idx, nrm, which=which, seed=3)
        assert np.abs(got[:, :3].astype(np.float64) - x).max() <= 1e-6, np.abs(got[:, :3] - x).max()      # a few float32 roundings of a unit vector, 2^-24 each
        assert (got[:, 3] == w).all()
        P2, uv2, idx2, _ = sheet(negate_u=True)
        neg = ca.tangent_model(P2, uv2, idx2, nrm, which=which, seed=3)
        assert (neg[:, 3] == -w).all()
        assert (neg[:, :3] == -got[:, :3]).all()                                # exactly: k == 0 here, and the sums mirror
        gi = ca.tangent_model(P, uv, idx, nrm, fmt=ca.FMT_INT16, which=which, seed=3)
        assert np.abs(gi[:, :3] - x * 32767).max() <= 1.0 and (gi[:, 3] == 32767).all()


# ---- 3. edges of the value ----

UP = np.array([[0, 0, 1]], np.float32)


def test_one_triangle():
    P = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0]], np.int32)
    t = np.array([[0, 0], [5, 0], [0, 5]], np.int32)
    got = hook_equals_model(P, t, np.array([[0, 1, 2]], np.uint32), np.repeat(UP, 3, 0), "triangle")
    assert (got == (1, 0, 0, 1)).all()                                          # u runs along x, v along y, n = z: right-handed
    t[:, 0] = -t[:, 0]
    got = hook_equals_model(P, t, np.array([[0, 1, 2]], np.uint32), np.repeat(UP, 3, 0), "mirrored triangle")
    assert (got == (-1, 0, 0, -1)).all()


def test_a_face_that_names_a_vertex_twice():
    """its uv differences make det 0: it adds nothing, with the hook as with the model"""
    P = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [7, 7, 1]], np.int32)
    t = np.array([[0, 0], [5, 0], [0, 5], [4, 4]], np.int32)
    n = np.repeat(UP, 4, 0)
    base = hook_equals_model(P, t, np.array([[0, 1, 2], [1, 3, 2]], np.uint32), n, "base")
    for f in ([0, 0, 1], [2, 1, 2], [3, 1, 1]):
        got = hook_equals_model(P, t, np.array([[0, 1, 2], f, [1, 3, 2]], np.uint32), n, ("twice", f))
        assert got.tobytes() == base.tobytes()


def test_fallbacks():
    P = np.array([[0, 0, 0], [10, 0, 0], [0, 10, 0], [3, 3, 3]], np.int32)
    t = np.array([[0, 0], [5, 0], [0, 5], [1, 1]], np.int32)
    idx = np.array([[0, 1, 2]], np.uint32)
    n = np.repeat(UP, 4, 0)
    fb, fbi = np.array([1, 0, 0, 1], np.float32), np.array([32767, 0, 0, 32767], np.int16)
    got = hook_equals_model(P, t, idx, n, "unreferenced")                       # vertex 3: no face names it
    assert (got[3] == fb).all() and (got[:3] == (1, 0, 0, 1)).all()
    got = hook_equals_model(P, np.full_like(t, 9), idx, n, "uvs equal")          # no uv area anywhere
    assert (got == fb).all()
    assert (ca.tangent_model(P, np.full_like(t, 9), idx, n, fmt=ca.FMT_INT16) == fbi).all()
    nn = n.copy(); nn[1] = np.nan                                               # a NaN normal
    got = hook_equals_model(P, t, idx, nn, "nan normal")
    assert (got[1] == fb).all() and not np.isnan(got).any()
    par = n.copy(); par[:] = (1, 0, 0)                                          # the tangent parallel to the normal
    got = hook_equals_model(P, t, idx, par, "parallel")
    assert (got == fb).all()
    got = hook_equals_model(P, t, np.zeros((0, 3), np.uint32), n, "no faces")
    assert (got == fb).all()


def exact_sums_differ(P, t, index):
    """vertices whose T, summed in Python's unbounded integers, is not what int64 holds: the wrap happened"""
    Pl, tl = np.asarray(P).astype(object), np.asarray(t).astype(object)
    T = [[0, 0, 0] for _ in range(len(Pl))]
    for a, b, c in np.asarray(index).astype(np.int64):
        r1, r2 = tl[b][1] - tl[a][1], tl[c][1] - tl[a][1]
        det = (tl[b][0] - tl[a][0]) * r2 - (tl[c][0] - tl[a][0]) * r1
        sg = (det > 0) - (det < 0)
        for v in (a, b, c):
            for i in range(3):
                T[v][i] += sg * ((Pl[b][i] - Pl[a][i]) * r2 - (Pl[c][i] - Pl[a][i]) * r1)
    got = ct.accumulate(P, t, index)[0]
    return sum(any(T[v][i] != int(got[v][i]) for i in range(3)) for v in range(len(Pl)))


def test_full_width_values():
    """integers near +-2^30 through the encoder (k > 0), and the same mesh with every integer at +-(2^31 - 1), where sums leave 64 bits:
    the wrap is part of the value, and the hook's is the model's"""
    m = synth.full_width_values(synth.bumpy_sphere(9, 7, seed=37), seed=37)
    e = ct.Inputs(ct.encode(m, normals="float", position_bits=0, position_q=1.0, uv_bits=0))
    assert np.abs(e.P).max() >= 2 ** 30 and np.abs(e.t).max() >= 2 ** 29
    assert ct.shifts(*e.sums()[:2]).max() > 30
    for nfmt in (ca.FMT_FLOAT, ca.FMT_INT16):
        hook_equals_model(e.P, e.t, e.index, e.normal(nfmt), ("full width", nfmt), seeds=(1,))
    top = 2 ** 31 - 1
    P, t = np.where(e.P < 0, -top, top).astype(np.int32), np.where(e.t < 0, -top, top).astype(np.int32)
    P[::3, 0] //= 3; t[::5, 1] //= 7; t[1::4, 0] //= 5                          # (not every face degenerate)
    assert exact_sums_differ(P, t, e.index) > 0
    hook_equals_model(P, t, e.index, e.normal(ca.FMT_FLOAT), "wrapping", seeds=(1,))


def test_deeper_grids_need_a_shift():
    """positions of 20 bits and uvs of 16: the sums pass 24 bits by seven bits and more (11 on this torus), at every vertex"""
    e = ct.Inputs(ct.encode(synth.torus(24, 12), position_bits=20, uv_bits=16))
    k = ct.shifts(*e.sums()[:2])
    assert k.max() >= 7 and k.min() > 0
    hook_equals_model(e.P, e.t, e.index, e.normal(ca.FMT_FLOAT), "20/16 bits", seeds=(1,))


# ---- 4. the contract's table ----

def test_fallback_and_face_counts():
    nvert = {"torus_24_12": 288, "icosphere_2": 162, "closed_sphere": 266, "holey_disc_20": 441, "bumpy_sphere_16_8": 144}
    negative, both_signs = 0, 0
    for name in ct.NAMES:
        nv, fb, neg, zero = ct.table_counts(name)
        assert nv == nvert[name] and (fb, neg, zero) == ct.TABLE[name], (name, nv, fb, neg, zero)
        negative += neg > 0
        # through the encoder and the oracle: the same faces; the disc's two unreferenced vertices (its only fallbacks) are not stored
        e = ct.inputs(name)
        out, efb, _ = e.model(ca.FMT_FLOAT)
        det = e.sums()[2]
        assert (int((det < 0).sum()), int((det == 0).sum())) == ct.TABLE[name][1:], name
        assert int(efb.sum()) == (0 if name == "holey_disc_20" else fb) and e.nvert == nv - (2 if name == "holey_disc_20" else 0), name
        both_signs += (out[:, 3] < 0).any() and (out[:, 3] > 0).any()
    assert negative >= 4 and both_signs >= 4


# ---- 5. declaration and arguments ----

def test_the_calls_are_exported_and_declared():
    L = ca.lib()
    assert hasattr(L, "crthip_batch_bind_computed_tangents") and hasattr(L, "crthip_tangent_model")
    hdr = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "corto_hip.h")).read())
    assert "int crthip_batch_bind_computed_tangents(crthip_batch *b, uint32_t i, void *buffer, uint32_t format, uint32_t stride);" in hdr
    assert ("int crthip_tangent_model(const int32_t *position, const int32_t *uv, const void *index, uint32_t index_u16, uint32_t nvert, uint32_t nface, "
            "const void *normal, uint32_t normal_format, uint32_t normal_stride, void *out, uint32_t format, uint32_t stride, int which, uint32_t seed);") in hdr
    assert L.crthip_abi_version() == 6 and re.search(r"#define CRTHIP_ABI_VERSION 6\b", hdr)      # additive: the number stays


def test_a_null_batch_is_an_argument_error():
    L = ca.lib()
    buf = np.zeros(16, dtype=np.float32)
    assert L.crthip_batch_bind_computed_tangents(None, 0, buf.ctypes.data_as(C.c_void_p), ca.FMT_FLOAT, 0) == ct.E_ARGUMENT
    assert L.crthip_batch_bind_computed_tangents(None, 0, None, ca.FMT_FLOAT, 0) == ct.E_ARGUMENT


def test_the_hook_refuses_what_a_binding_would():
    P, t, idx = np.zeros((3, 3), np.int32), np.zeros((3, 2), np.int32), np.array([[0, 1, 2]], np.uint32)
    n = np.repeat(UP, 3, 0)
    for kw in (dict(stride=12), dict(stride=18), dict(fmt=ca.FMT_INT16, stride=6), dict(fmt=ca.FMT_INT16, stride=9), dict(which=2), dict(fmt=ca.FMT_UINT16)):
        with pytest.raises(Exception):
            ca.tangent_model(P, t, idx, n, out=np.zeros(256, np.uint8), **kw)
