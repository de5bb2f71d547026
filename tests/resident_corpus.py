"""Blobs for the resident-walk tests (test_resident_walk_cpu.py, test_resident_batch_gpu.py): every golden blob, blobs whose header uses
what the walk must restate exactly (duplicate exif keys and attribute names, a name cut at an embedded NUL), and blobs too big for a walk
record (kilobytes of exif, hundreds of log streams)."""
import glob
import os
import struct

import numpy as np

import corto_amd as ca
from corto_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def golden_blobs():
    """[(name, uint8 blob)] of every .crt in tests/golden, file by file"""
    out = []
    for f in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        z = np.load(f)
        stem = os.path.basename(f)[:-4]
        for k in z.files:
            if k == "crt" or k.startswith("crt_") or k.endswith(".crt"):
                out.append((stem if k == "crt" else stem + ":" + k, np.ascontiguousarray(z[k], dtype=np.uint8)))
    return out


def _str(b):
    return struct.pack("<H", len(b)) + b


def parse_header(blob):
    """(exif [(key bytes, value bytes)], attrs [(name bytes, codec, q bytes, N, format, strategy)], version, entropy, nvert, nface, body)"""
    b = bytes(blob)
    pos = 4
    version, entropy = struct.unpack_from("<IB", b, pos); pos += 5

    def s():
        nonlocal pos
        n, = struct.unpack_from("<H", b, pos); pos += 2
        v = b[pos:pos + n]; pos += n
        return v
    nexif, = struct.unpack_from("<I", b, pos); pos += 4
    exif = [(s(), s()) for _ in range(nexif)]
    nattr, = struct.unpack_from("<I", b, pos); pos += 4
    attrs = []
    for _ in range(nattr):
        name = s()
        codec, = struct.unpack_from("<I", b, pos)
        q = b[pos + 4:pos + 8]
        N, fmt, strat = b[pos + 8], b[pos + 9], b[pos + 10]
        pos += 11
        attrs.append((name, codec, q, N, fmt, strat))
    nvert, nface = struct.unpack_from("<II", b, pos); pos += 8
    return exif, attrs, version, entropy, nvert, nface, b[pos:]


def build(exif, attrs, version, entropy, nvert, nface, body):
    h = struct.pack("<IIB", 0x787A6300, version, entropy) + struct.pack("<I", len(exif))
    h += b"".join(_str(k) + _str(v) for k, v in exif)
    h += struct.pack("<I", len(attrs))
    h += b"".join(_str(n) + struct.pack("<I", c) + q + bytes([N, f, st]) for n, c, q, N, f, st in attrs)
    return h + struct.pack("<II", nvert, nface) + body


def crafted(blob):
    """the same mesh behind a header that the walk has to read like std::map does: an exif key given twice (the last value wins, cut
    at a NUL), a decoy entry of the first attribute in front of the real one (the real one wins), a name with an embedded NUL and
    junk behind it; the header keeps its length modulo 4 so that the body's bit blocks stay aligned"""
    exif, attrs, version, entropy, nvert, nface, body = parse_header(blob)
    old = len(bytes(blob)) - len(body)
    n0, c0, q0, N0, f0, s0 = attrs[0]
    decoy = (n0 + b"\0", 1 if c0 != 1 else 2, struct.pack("<f", 0.5), 7, 0, 0)
    named = [(n + b"\0junk\0", c, q, N, f, st) if k == len(attrs) - 1 else (n, c, q, N, f, st) for k, (n, c, q, N, f, st) in enumerate(attrs)]
    ex = list(exif) + [(b"dup\0", b"first\0"), (b"alpha\0", b"1\0"), (b"dup\0", b"second\0tail\0")]
    for pad in range(4):
        h = build(ex + [(b"pad\0", b"x" * pad + b"\0")], [decoy] + named, version, entropy, nvert, nface, b"")
        if (len(h) - old) % 4 == 0:
            return np.frombuffer(build(ex + [(b"pad\0", b"x" * pad + b"\0")], [decoy] + named, version, entropy, nvert, nface, body),
                                 dtype=np.uint8).copy()
    raise AssertionError("no padding keeps the body aligned")


def big_exif_blob():
    """a small mesh with 3 KB of exif: its header does not fit a walk record"""
    m = synth.bumpy_sphere(16, 8, seed=5)
    return ca.encode(m, exif={"note": "n" * 3000, "author": "walk"}).copy()


def many_streams_blob(nattr=8):
    """a mesh with `nattr` generic attributes of 16 parallel components: one log stream each, 128 in all, more than a record holds"""
    rng = np.random.default_rng(11)
    m = synth.bumpy_sphere(12, 6, seed=6)
    attrs = [("g%02d" % k, rng.integers(-50, 50, size=(m.nvert, 16)).astype(np.float32), 1.0, ca.PARALLEL) for k in range(nattr)]
    return ca.encode(m, with_normal=False, with_color=False, with_uv=False, attributes=attrs).copy()


def corpus():
    """[(name, blob)]: the golden blobs, a crafted header of three of them, and the two blobs too big for a record"""
    g = golden_blobs()
    by = dict(g)
    out = list(g)
    for name in ("c4_unit", "group_props", "entropy_none"):
        out.append(("crafted:" + name, crafted(by[name])))
    out.append(("big_exif", big_exif_blob()))
    out.append(("many_streams", many_streams_blob()))
    return out


def write_corpus(path, blobs):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(blobs)))
        for b in blobs:
            b = np.ascontiguousarray(b, dtype=np.uint8)
            f.write(struct.pack("<I", len(b)))
            f.write(b.tobytes())
