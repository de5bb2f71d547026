"""The encoders' tile and size-class limits and the inputs that sit on either side of each: shared by tests/test_encode_size_classes_cpu.py
(every case is on the side it is named for, every host model equals the host encoder and the reference), tests/test_encode_size_classes_gpu.py
(every case through every entry point that reaches its kernel, on the path it is meant to take) and tests/golden/make_enc_boundaries.py
(the reference's bytes for every case).

The predicates come from tests/cpp/enc_size_probe.cpp, which includes the library's headers: nothing here restates a formula.  A row is
(id, builder, kwargs, side): `builder(**kwargs)` makes the input, `side` is what the probe answered for it on the day the table was written - the
CPU module asks again for the input's real counts, so a changed limit names the rows that crossed.  Inputs are rebuilt from seeds, never stored.

Out of scope: the corner sort's 32-bit pass needs 16.7 M estimated-normal vertices in one chunk and is left unreached (the 24-bit pass is the
65 536-vertex rows); the Tunstall coder's 2^23 stream limit is pinned by test_per_mesh_errors_leave_the_neighbours_alone."""
import hashlib
import os

import numpy as np

import corto_amd as ca
from corto_amd import synth
import size_classes as sc

ROOT = sc.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "enc_boundaries.npz")
INLINE_MAX = 2048            # reference bytes up to this size are stored as they are, longer ones as length + sha256


class Probe(sc.Probe):
    """tests/cpp/enc_size_probe.cpp"""

    def __init__(self, workdir):
        super().__init__(workdir, source="enc_size_probe")

    def num(self, *q):
        return int(self.ask(*q)[0])

    def fits(self, nvert, nface):
        return self.ask("fits", nvert, nface)[0] == "1"

    def parse(self, size):
        r = self.ask("parse", size)
        return r[0] == "1", r[1] == "1"

    def trie(self, nsym, lengths):
        """(level_bound, level_bound*nsym^2, the device builds the trie) of a dictionary's 256 word lengths"""
        r = self.ask("trie", nsym, *[int(x) for x in lengths])
        return int(r[0]), int(r[1]), r[2] == "1"


# ------------------------------------------------------------------------------------------------------------------------------------
# builders: each returns (mesh, encode keywords)

LEAN = dict(with_color=False, with_uv=False)


def closed(nvert, pred, seed=0, **kw):
    return sc.closed_mesh(nvert, seed=seed), dict(LEAN, normal_prediction=pred, **kw)


def holed(nvert, holes, pred, seed=0, **kw):
    return sc.open_mesh(nvert, holes, seed=seed), dict(LEAN, normal_prediction=pred, **kw)


def boundary_vertices(mesh):
    """vertices with an edge that one face alone uses - the XOR of a vertex's neighbours over its faces is non-zero exactly there
    (src/normal_attribute.cpp: markBoundary)"""
    idx = mesh.index.astype(np.int64)
    x = np.zeros(mesh.nvert, dtype=np.int64)
    for k in range(3):
        np.bitwise_xor.at(x, idx[:, k], idx[:, (k + 1) % 3])
        np.bitwise_xor.at(x, idx[:, k], idx[:, (k + 2) % 3])
    return int(np.count_nonzero(x))


def bordered(nvert, nboundary, seed=0):
    """closed_mesh(nvert) with faces removed until exactly `nboundary` vertices lie on a boundary: faces that share no vertex with a hole add
    three, a face beside a one-face hole (sharing an edge, its third vertex untouched) adds one.  Holes spread over the whole encode order."""
    m = sc.closed_mesh(nvert, seed=seed)
    idx = m.index.astype(np.int64)
    nf = len(idx)
    touched = np.zeros(m.nvert, bool)
    drop = np.zeros(nf, bool)
    want_holes, widen = nboundary // 3, nboundary % 3
    step = max(1, nf // (want_holes + 1))
    holes = []
    f = (3 + seed) % nf
    tries = 0
    while len(holes) < want_holes and tries < 4 * nf:
        if not drop[f] and not touched[idx[f]].any():
            drop[f] = True; touched[idx[f]] = True; holes.append(f)
            f = (f + step) % nf
        else:
            f = (f + 1) % nf
        tries += 1
    assert len(holes) == want_holes, (nvert, nboundary)
    # widen the last `widen` holes: a face that shares an edge with the hole and whose third vertex no hole touches
    edge_faces = {}
    for fi, (a, b, c) in enumerate(idx):
        for e in ((a, b), (b, c), (c, a)):
            edge_faces.setdefault((min(e), max(e)), []).append(fi)
    done = 0
    for h in reversed(holes):
        if done == widen:
            break
        a, b, c = idx[h]
        for e in ((a, b), (b, c), (c, a)):
            other = [g for g in edge_faces[(min(e), max(e))] if g != h and not drop[g]]
            if other:
                third = [v for v in idx[other[0]] if v not in e][0]
                if not touched[third]:
                    drop[other[0]] = True; touched[third] = True; done += 1
                    break
    assert done == widen, (nvert, nboundary, done)
    out = synth.Mesh(m.position, m.index[~drop], m.normal, m.color, m.uv)
    assert boundary_vertices(out) == nboundary, (boundary_vertices(out), nboundary)
    return out, dict(LEAN, normal_prediction=ca.BORDER)


def padded(nvert_base, nvert, pred, seed=0):
    """closed_mesh(nvert_base) with unreferenced vertices up to `nvert`"""
    m = sc.closed_mesh(nvert_base, seed=seed)
    extra = nvert - m.nvert
    rng = np.random.default_rng(seed + 5)
    pos = np.ascontiguousarray(np.vstack([m.position, rng.random((extra, 3), dtype=np.float32)]))
    nrm = np.ascontiguousarray(np.vstack([m.normal, np.repeat(m.normal[:1], extra, axis=0)]))
    return synth.Mesh(pos, m.index, nrm, None, None), dict(normal_prediction=pred)


def coloured(nvert, seed=0):
    """positions and a 4-byte colour alone"""
    m = sc.closed_mesh(nvert, seed=seed, color_components=4)
    return m, dict(with_normal=False, with_uv=False)


def cloud(n, seed=0):
    """the first n points of a sampled sphere, positions on a 20-bit grid: no two quantised points are equal, the device sort is kept"""
    nu = max(4, int(np.ceil(np.sqrt(2.0 * (n + 8)))))
    m = synth.point_cloud(nu, nu // 2 + 2, seed=seed)
    assert m.nvert >= n, (m.nvert, n)
    f = lambda a: None if a is None else np.ascontiguousarray(a[:n])
    return synth.Mesh(f(m.position), None, f(m.normal), f(m.color), f(m.uv)), dict(normal_prediction=ca.DIFF, position_bits=20)


def empty_cloud(seed=0):
    """no vertex at all.  (The host encoder reads position[0] of a cloud before it looks at the count: the empty array is the front of zeros)"""
    m, kw = cloud(4, seed=seed)
    f = lambda a: None if a is None else a[:0].copy()
    backing = np.zeros((4, 3), dtype=np.float32)
    e = synth.Mesh(backing[:0], None, f(m.normal), f(m.color), f(m.uv))
    e.position = backing[:0]
    return e, dict(normal_prediction=ca.DIFF)


def faceless(nvert, seed=0):
    """vertices and an index array of no faces"""
    m, kw = cloud(nvert, seed=seed)
    return synth.Mesh(m.position, np.zeros((0, 3), dtype=np.uint32), m.normal, m.color, m.uv), dict(kw, normal_prediction=ca.ESTIMATED)


def degenerate(seed=0):
    """every face names one vertex three times"""
    d = synth.bumpy_sphere(8, 4, seed=seed)
    d.index = np.ascontiguousarray(np.repeat(d.index[:, :1], 3, axis=1))
    return d, dict(normal_prediction=ca.BORDER)


def build(row):
    return row[1](**row[2])


# ------------------------------------------------------------------------------------------------------------------------------------
# mesh rows.  side: what the probe said of the row's counts when the table was written

D, E, B = ca.DIFF, ca.ESTIMATED, ca.BORDER
_P = {D: "diff", E: "est", B: "border"}

# 256-thread job blocks (k_enc_quantize_batch, k_enc_corners, k_enc_est_normal, k_enc_input_check) and DENC_BLOCK (k_enc_delta):
# side = (job blocks of nvert, k_enc_delta workgroups of nvert)
BLOCK_SIDES = {255: (1, 1), 256: (1, 1), 257: (2, 1), 1023: (4, 1), 1024: (4, 1), 1025: (5, 2)}
BLOCK_CASES = [("blocks_%d_%s" % (nv, _P[p]), closed if p != B else holed, dict(nvert=nv, pred=p, seed=nv % 7, **({} if p != B else {"holes": 3})), BLOCK_SIDES[nv])
               for nv in sorted(BLOCK_SIDES) for p in (D, E, B)]

# BORDER's compaction (k_enc_delta): the running count `w` of boundary vertices passes 256 and 512 inside the scan.  side = the count
BORDER_CASES = [("border_w_%d" % nb, bordered, dict(nvert=2400, nboundary=nb, seed=nb % 5), nb) for nb in (255, 256, 257, 511, 512, 513)]

# the corner sort's tiles: batches of ESTIMATED meshes by their corner total.  side = workgroups of one radix pass
CORNER_BATCHES = [
    ("corners_4095", [(closed, dict(nvert=343, pred=E, seed=1)), (holed, dict(nvert=344, holes=1, pred=E, seed=2))], 1),
    ("corners_4098", [(closed, dict(nvert=343, pred=E, seed=1)), (closed, dict(nvert=344, pred=E, seed=2))], 2),
    ("corners_8190", [(closed, dict(nvert=457, pred=E, seed=s)) for s in (1, 2, 3)], 2),
    ("corners_8193", [(closed, dict(nvert=457, pred=E, seed=1)), (closed, dict(nvert=457, pred=E, seed=2)), (holed, dict(nvert=458, holes=1, pred=E, seed=3))], 3),
]

# the corner sort's pass count: batches by their total of estimated-normal vertices.  side = key bits
VBASE_BATCHES = [("vbase_%d" % (100 + last), [(closed, dict(nvert=100, pred=E, seed=1)), (closed, dict(nvert=last, pred=E, seed=2))], bits)
                 for last, bits in ((155, 8), (156, 16), (157, 16))] + \
                [("vbase_%d" % (60000 + last), [(closed, dict(nvert=30000, pred=E, seed=1)), (closed, dict(nvert=30000, pred=B if last == 5536 else E, seed=2)),
                                               (closed, dict(nvert=last, pred=E, seed=3))], bits)
                 for last, bits in ((5535, 16), (5536, 24), (5537, 24))]

# jobs of no items at the front, in the middle and at the end of one batch, among ordinary neighbours
ZERO_BATCH = [("zero_cloud_first", empty_cloud, dict(seed=1)), ("n1", closed, dict(nvert=300, pred=E, seed=1)), ("n2", cloud, dict(n=257, seed=2)),
              ("zero_faces_middle", faceless, dict(nvert=40, seed=3)), ("n3", holed, dict(nvert=257, holes=3, pred=B, seed=4)),
              ("n4", closed, dict(nvert=256, pred=D, seed=5)), ("all_degenerate_last", degenerate, dict(seed=6))]

# enc_topo_fits_lds.  side = the walk state is in LDS.  FITS_LAST: the largest closed mesh that fits.  The face bound (3*nface <= 65535)
# is shadowed: 21 845 faces need 742 KB of state, so both of its rows are outside, by the LDS bound.  The vertex bound (nvert <= 65534)
# binds for a small mesh beside many unreferenced vertices.
FITS_LAST = 2283
FITS_CASES = [("fits_last", closed, dict(nvert=FITS_LAST, pred=E, seed=1), True), ("fits_next", closed, dict(nvert=FITS_LAST + 1, pred=E, seed=1), False),
              ("fits_faces_65535", holed, dict(nvert=10925, holes=1, pred=E, seed=2), False), ("fits_faces_65538", closed, dict(nvert=10925, pred=E, seed=2), False),
              ("fits_nvert_65534", padded, dict(nvert_base=100, nvert=65534, pred=E, seed=3), True),
              ("fits_nvert_65535", padded, dict(nvert_base=100, nvert=65535, pred=E, seed=3), False)]

# build_image's DIRECT_BYTES: an input array below it is staged, one at it goes up from the caller's array.  side = (array, bytes, direct)
DIRECT_CASES = [("direct_position_87381", closed, dict(nvert=87381, pred=D, seed=1, with_normal=False), ("position", 87381 * 12, False)),
                ("direct_position_87382", closed, dict(nvert=87382, pred=D, seed=1, with_normal=False), ("position", 87382 * 12, True)),
                ("direct_color_262143", coloured, dict(nvert=262143, seed=2), ("color", 262143 * 4, False)),
                ("direct_color_262144", coloured, dict(nvert=262144, seed=2), ("color", 262144 * 4, True)),
                ("direct_index_87381", holed, dict(nvert=43693, holes=1, pred=D, seed=3, with_normal=False), ("index", 87381 * 12, False)),
                ("direct_index_87382", closed, dict(nvert=43693, pred=D, seed=3, with_normal=False), ("index", 87382 * 12, True))]

# the clouds' Morton sort (uint64 keys).  side = workgroups of one radix pass
CLOUD_SIDES = {1: 1, 2: 1, 3: 1, 4095: 1, 4096: 1, 4097: 2, 8191: 2, 8192: 2, 8193: 3}
CLOUD_CASES = [("cloud_%d" % n, cloud, dict(n=n, seed=n % 11), CLOUD_SIDES[n]) for n in sorted(CLOUD_SIDES)]


# rows the reference itself cannot encode - it faults on an item with no vertex or with no face left after the degenerate ones are dropped -
# so the host encoder alone says what their bytes are
NO_REFERENCE = ("zero.zero_cloud_first", "zero.all_degenerate_last")


def mesh_rows():
    """every mesh and cloud row, each once: [(id, builder, kwargs)]"""
    rows = [r[:3] for r in BLOCK_CASES + BORDER_CASES + FITS_CASES + DIRECT_CASES + CLOUD_CASES]
    for bid, items, _ in CORNER_BATCHES + VBASE_BATCHES:
        rows += [("%s.%d" % (bid, k), b, kw) for k, (b, kw) in enumerate(items)]
    rows += [("zero.%s" % n, b, kw) for n, b, kw in ZERO_BATCH]
    return rows


# ------------------------------------------------------------------------------------------------------------------------------------
# Tunstall streams.  side = (one window, staged once, k_enc_hist workgroups)

TUN_SIDES = {63: (True, True, 1), 64: (True, True, 1), 65: (False, True, 1), 127: (False, True, 1), 128: (False, True, 1), 129: (False, True, 1),
             4671: (False, True, 1), 4672: (False, True, 1), 4673: (False, False, 1), 8191: (False, False, 1), 8192: (False, False, 1), 8193: (False, False, 1),
             262143: (False, False, 1), 262144: (False, False, 1), 262145: (False, False, 2),
             524287: (False, False, 2), 524288: (False, False, 2), 524289: (False, False, 3)}
TUN_KINDS = ("six", "two", "tail1", "tail2", "tail3")


def tun_stream(n, kind, seed=0):
    """six: six uneven symbols; two: two symbols, one at 0.4 % (dictionary words of up to 255 symbols); tailK: one symbol with a single other
    one K positions before the end"""
    rng = np.random.default_rng(1000 + seed)
    if kind == "six":
        return rng.choice(np.arange(6, dtype=np.uint8) * 9, n, p=[0.55, 0.2, 0.12, 0.08, 0.03, 0.02])
    if kind == "two":
        s = np.where(rng.random(n) < 0.004, 3, 200).astype(np.uint8)
        s[n // 2] = 3                                                # (both symbols occur in the short streams too)
        return s
    s = np.full(n, 17, dtype=np.uint8)
    s[n - int(kind[4:])] = 4
    return s


TUN_CASES = [("tun_%d_%s" % (n, k), tun_stream, dict(n=n, kind=k, seed=n % 13), TUN_SIDES[n]) for n in sorted(TUN_SIDES) for k in TUN_KINDS]


def flat_stream(nsym, reps=40, seed=0):
    """nsym symbols with equal counts: every dictionary word is one or two symbols long, so level_bound is 1 and the trie's bound nsym^2"""
    return np.random.default_rng(seed).permutation(np.repeat(np.arange(nsym, dtype=np.uint8), reps))


# ENC_TRIE_LDS_MAX = 24 576 entries: 156^2 = 24 336 is the last alphabet whose trie the device builds (and parses from LDS), 157^2 = 24 649
# the first left to the host routine (and walked in global memory).  side = the device builds it
TRIE_CASES = [("trie_156", flat_stream, dict(nsym=156, seed=1), True), ("trie_157", flat_stream, dict(nsym=157, seed=1), False)]


def stream_lengths(s):
    """(nsym, the 256 word lengths of the dictionary) of a byte stream: its probabilities as the coder takes them (count*255/size, likeliest
    first: src/tunstall.cpp getProbabilities) through the oracle's dictionary builder.  Equal probabilities may come in another order than
    the coder's: the lengths are the same"""
    from oracle import oracle as oc
    sym, cnt = np.unique(s, return_counts=True)
    pr = sorted(((int(c) * 255 // len(s)) & 255, int(v)) for v, c in zip(sym, cnt))[::-1]
    return len(sym), oc.tunstall_tables(np.array([[v, q] for q, v in pr], dtype=np.uint8))[1]


def block_tables(block):
    """(nsym, probabilities) of a Tunstall block's header"""
    nsym = int(block[0])
    return nsym, np.asarray(block[1:1 + 2 * nsym]).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------------------------------------------
# value arrays for crthip_encode_values.  A row's builder returns (kind, array).  side = 256-item tiles of k_enc_pack

def values(kind, count, N, scale, seed=0):
    rng = np.random.default_rng(2000 + seed)
    a = np.rint(rng.normal(0, scale, (count, N)))
    return (kind, a.clip(-128, 127).astype(np.int8)) if kind == ca.ENC_VALUES_I8 else (kind, a.astype(np.int32))


def full_tiles(count, seed=0):
    """ARRAY, N = 16: one element of width 1 (16 bits: carry_bits = 16 from the first tile on), then every component in [2^30, 2^31) -
    width 32, 512 bits an element: with the carry, the fullest tile k_enc_pack can see"""
    rng = np.random.default_rng(3000 + seed)
    a = rng.integers(2 ** 30, 2 ** 31, (count, 16), dtype=np.int64).astype(np.int32)
    a[0] = -1
    return ca.ENC_ARRAY, a


def word_edge(extra_bit, count=400, seed=0):
    """ARRAY, N = 1, every element 8 bits wide: the first tile ends on a word (256*8 bits: carry_bits = 0); extra_bit: its first element is
    9 bits wide and the tile ends one bit past the word"""
    rng = np.random.default_rng(4000 + seed)
    a = rng.integers(64, 128, (count, 1)).astype(np.int32)
    if extra_bit:
        a[0] = 200
    return ca.ENC_ARRAY, a


_K = {ca.ENC_ARRAY: "array", ca.ENC_VALUES_I32: "i32", ca.ENC_VALUES_I8: "i8"}
VALUE_CASES = [("values_%s_%d" % (_K[k], c), values, dict(kind=k, count=c, N=N, scale=s, seed=c % 9), -(-c * (1 if k == ca.ENC_ARRAY else N) // 256))
               for k, N, s in ((ca.ENC_ARRAY, 3, 40), (ca.ENC_VALUES_I32, 3, 900), (ca.ENC_VALUES_I8, 4, 6)) for c in (255, 256, 257, 511, 512, 513)]
# VALUES log arrays lie component after component: component c's Tunstall source starts c*count bytes in, 0..3 bytes off a dword
VALUE_CASES += [("values_i8_261_heads", values, dict(kind=ca.ENC_VALUES_I8, count=261, N=4, scale=6, seed=3), 5),
                ("values_i8_262145_heads", values, dict(kind=ca.ENC_VALUES_I8, count=262145, N=4, scale=2, seed=4), 4097),
                ("values_full_tiles", full_tiles, dict(count=518, seed=1), 3),
                ("values_word_edge_0", word_edge, dict(extra_bit=False), 2), ("values_word_edge_1", word_edge, dict(extra_bit=True), 2)]


# ------------------------------------------------------------------------------------------------------------------------------------
# the fixture: the reference's bytes of every row (tests/golden/make_enc_boundaries.py)

def pack_reference(data: bytes):
    """what the fixture stores for a row: its bytes when short, else length + sha256"""
    if len(data) <= INLINE_MAX:
        return np.frombuffer(data, dtype=np.uint8).copy()
    return np.frombuffer(len(data).to_bytes(8, "little") + hashlib.sha256(data).digest(), dtype=np.uint8).copy()


_fixture = {}


def reference_matches(cid, data: bytes):
    """`data` is what the reference wrote for row `cid`"""
    if not _fixture:
        z = np.load(FIXTURE)
        _fixture.update({k: z[k] for k in z.files})
    kind, stored = ("b", _fixture["b:" + cid]) if "b:" + cid in _fixture else ("d", _fixture["d:" + cid])
    if kind == "b":
        return stored.tobytes() == data
    return int.from_bytes(stored[:8].tobytes(), "little") == len(data) and stored[8:].tobytes() == hashlib.sha256(data).digest()
