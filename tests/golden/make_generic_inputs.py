#!/usr/bin/env python3
"""Fixture for generic attributes with non-FLOAT inputs (Encoder::addAttribute(name, buffer, format, N, q, strategy) with INT32, INT16, INT8 and
DOUBLE buffers, include/corto/encoder.h:70, src/encoder.cpp:187-197; GenericAttr<int>::quantize, include/corto/vertex_attribute.h:79-104),
made FROM THE UNMODIFIED REFERENCE.  Run in the build container only, after oracle/Makefile has built oracle/_ref/libcorto_ref.so:

    python tests/golden/make_generic_inputs.py

oracle/refcodec.encode passes one FLOAT attribute only, so this script compiles a small driver of its own (below) against the
reference's public headers and oracle/_ref/libcorto_ref.so, which exports crt::Encoder.  Data only goes into the repository:
per mesh the inputs, per case the steps, strategy and the .crt bytes the reference Encoder wrote (generic_inputs.npz).
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from corto_amd import synth            # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("REF", "/root/reference")          # as oracle/Makefile
REFLIB = os.path.join(ROOT, "oracle", "_ref", "libcorto_ref.so")

DRIVER = r"""
#include <stdint.h>
#include <string.h>
#include "corto.h"
using namespace crt;
extern "C" int64_t gen_encode(uint32_t nvert, uint32_t nface, const float *pos, const uint32_t *index, int pos_bits,
                              const float *normal, const uint8_t *color, const float *uv, float uv_q, int entropy,
                              int nattr, const char *const *names, const void *const *bufs, const int *formats, const int *comps,
                              const float *qs, const uint32_t *strategies, uint8_t *out, int64_t cap) {
	try {
		Encoder enc(nvert, nface, (Stream::Entropy)entropy);
		if(nface) enc.addPositionsBits(pos, (uint32_t *)index, pos_bits); else enc.addPositionsBits(pos, pos_bits);
		if(normal) enc.addNormals(normal, 10, NormalAttr::BORDER);
		if(color) enc.addColors(color, 6, 7, 6, 5);
		if(uv) enc.addUvs(uv, uv_q);
		for(int k = 0; k < nattr; k++)
			enc.addAttribute(names[k], (const char *)bufs[k], (VertexAttribute::Format)formats[k], comps[k], qs[k], strategies[k]);
		enc.encode();
		const int64_t size = enc.stream.size();
		if(out && cap >= size) memcpy(out, enc.stream.data(), size);
		return size;
	} catch(const char *) {
		return -1;
	}
}
"""

FMT = {np.dtype(np.int32): 1, np.dtype(np.int16): 3, np.dtype(np.int8): 5, np.dtype(np.float32): 6, np.dtype(np.float64): 7}


def build_driver(tmp):
    src = os.path.join(tmp, "gen_driver.cpp")
    so = os.path.join(tmp, "gen_driver.so")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-fPIC", "-ffp-contract=off", "-w", "-shared", "-I" + os.path.join(REF, "include", "corto"),
                           "-o", so, src, REFLIB, "-Wl,-rpath," + os.path.dirname(REFLIB)])
    L = C.CDLL(so)
    L.gen_encode.restype = C.c_int64
    return L


def encode(L, mesh, attrs, entropy, with_normal, with_color, with_uv):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)     # noqa: E731
    n = len(attrs)
    vals = [np.ascontiguousarray(v) for (_, v, _, _) in attrs]
    names = (C.c_char_p * max(n, 1))(*[a[0].encode() for a in attrs])
    bufs = (C.c_void_p * max(n, 1))(*[v.ctypes.data for v in vals])
    fmts = np.array([FMT[v.dtype] for v in vals] or [0], dtype=np.int32)
    comps = np.array([v.shape[1] for v in vals] or [0], dtype=np.int32)
    qs = np.array([a[2] for a in attrs] or [0], dtype=np.float32)
    sts = np.array([a[3] for a in attrs] or [0], dtype=np.uint32)
    uv_q = float(np.float32(2.0) ** np.float32(-12))
    args = (C.c_uint32(mesh.nvert), C.c_uint32(mesh.nface), ptr(mesh.position), ptr(mesh.index), 14,
            ptr(mesh.normal) if with_normal else None, ptr(mesh.color) if with_color else None, ptr(mesh.uv) if with_uv else None,
            C.c_float(uv_q), entropy, n, names, bufs, ptr(fmts), ptr(comps), ptr(qs), ptr(sts))
    size = L.gen_encode(*args, None, C.c_int64(0))
    assert size > 0, size
    out = np.zeros(size, dtype=np.uint8)
    assert L.gen_encode(*args, ptr(out), C.c_int64(size)) == size
    return out


def adversarial(nvert, rng):
    """int32 beyond +-2^24 and negatives (the int -> float rounding, truncation toward zero); doubles at q multiples +-1 ulp and, in a second
    array, also beyond the int range, +-inf and NaN.  Those quantise to INT_MIN, and a residual of INT_MIN in a stream without CORRELATED
    makes upstream's encodeValues write a 64-bit field (ilog2(abs(INT_MIN)) + 1, include/corto/cstream.h:128-133; BitStream::write then reads
    bmask past its end): undefined, and no decoder reads it back.  So the second array goes into the CORRELATED cases only (encodeArray's
    needed() is defined for every int)."""
    i32 = rng.integers(-(1 << 31), (1 << 31) - 1, size=(nvert, 2), dtype=np.int64).astype(np.int32)
    i32[: nvert // 2, 1] = rng.integers(-(1 << 25), 1 << 25, size=nvert // 2)
    i32[:8, 0] = [(1 << 24) + 1, (1 << 24) + 3, -(1 << 24) - 1, 2147483647, -2147483648, -7, 7, -1]
    q = 0.1
    k = rng.integers(-5000, 5000, size=(nvert, 3)).astype(np.float64)
    d = k * np.float64(np.float32(q))
    d[:, 1] = np.nextafter(d[:, 1], np.inf)
    d[:, 2] = np.nextafter(d[:, 2], -np.inf)
    tame = d.copy()
    tame[:6, 0] = [214748364.7, -214748364.8, 214748364.79, -0.0, 5e-324, -5e-324]
    special = [np.inf, -np.inf, np.nan, 3e9, -3e9, 214748364.7, -214748364.8, -214748364.9, 214748364.79, 1e300, -0.0, 5e-324]
    d[: len(special), 0] = special
    return i32, tame, d, q


def main():
    rng = np.random.default_rng(20261016)
    d = {}
    names = []
    with tempfile.TemporaryDirectory() as tmp:
        L = build_driver(tmp)
        mesh = synth.torus(24, 12, seed=5)
        cloud = synth.point_cloud(24, 16, seed=6)
        case_id = 0
        for kind, m in (("mesh", mesh), ("cloud", cloud)):
            nv = m.nvert
            i32, tame, special, dq = adversarial(nv, rng)
            inputs = [("a_int8", rng.integers(-128, 128, size=(nv, 1)).astype(np.int8)),
                      ("intensity", rng.integers(-32768, 32768, size=(nv, 3)).astype(np.int16)),
                      ("label32", i32),
                      ("time", tame),
                      ("time_x", special),
                      ("wide", rng.normal(size=(nv, 5)).astype(np.float64) * 1000.0),
                      ("zz_class", rng.integers(-3, 20, size=(nv, 7)).astype(np.int8))]
            for nm, v in inputs:
                d["%s.in.%s" % (kind, nm)] = v
            for strategy in range(4):
                for entropy in (0, 1):
                    qs = [1.0, 3.0, 1.0 if strategy % 2 else 7.0, dq, dq, 0.25, 2.0 if strategy else 1.0]
                    attrs = [(nm, v, q, strategy) for (nm, v), q in zip(inputs, qs) if nm != "time_x" or strategy & 2]
                    full = (strategy + entropy) % 2 == 0                 # every other case next to normals, colours and uvs
                    blob = encode(L, m, attrs, entropy, full, full, full)
                    name = "c%02d" % case_id
                    d[name + ".crt"] = blob
                    d[name + ".kind"] = np.array([kind == "mesh", entropy, int(full)], dtype=np.int32)
                    d[name + ".names"] = np.frombuffer(",".join(a[0] for a in attrs).encode(), dtype=np.uint8)
                    d[name + ".q"] = np.array([a[2] for a in attrs], dtype=np.float32)
                    d[name + ".strategy"] = np.array([strategy] * len(attrs), dtype=np.uint32)
                    names.append(name)
                    print("%s %-5s strategy %d entropy %d full %d: %6d B" % (name, kind, strategy, entropy, full, len(blob)))
                    case_id += 1
        d["mesh.position"], d["mesh.index"] = mesh.position, mesh.index
        d["mesh.normal"], d["mesh.color"], d["mesh.uv"] = mesh.normal, mesh.color, mesh.uv
        d["cloud.position"] = cloud.position
        d["cloud.normal"], d["cloud.color"], d["cloud.uv"] = cloud.normal, cloud.color, cloud.uv
    d["cases"] = np.frombuffer(",".join(names).encode(), dtype=np.uint8)
    np.savez_compressed(os.path.join(OUT, "generic_inputs.npz"), **d)


if __name__ == "__main__":
    main()
