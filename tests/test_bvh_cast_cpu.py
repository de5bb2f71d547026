"""crthip_bvh_cast without a device: the kernel's source on the host (corto_amd.bvh_cast_model: csrc/bvh_cast.h, one workgroup of 64 segments
after another) against the sequential model of the contract (tests/bvh_cast.py: a brute force over all faces in Python integers), byte for
byte, on trees from corto_amd.bvh_model in both partitions; the watertight shots; the contract's edges; corrupt trees, which go to the hook
ONLY; the call's errors as far as they can be reached without a device (the others: tests/test_bvh_cast_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import corto_amd as ca
import bvh
import bvh_cast as bc

BLOB_FACES = 4096                                           # bvh_blob's limit as csrc/bvh.h states it
R = 1 << 19


def trees(pos, idx):
    """the nodes of both partitions (one where the blob is beyond bvh_blob's limit), which the BVH's own tests hold equal"""
    out = []
    for which in (0, 1):
        if which == 0 and len(idx) > BLOB_FACES:
            continue
        out.append(ca.bvh_model(pos, idx, which=which, seed=which * 7)[0])
    return out


def agree(pos, idx, segs, flags=(0, bc.ANY, bc.FRONT, bc.ANY | bc.FRONT), tag="", **kw):
    """the hook on every tree equals the model under every flag combination; returns the nearest run's records"""
    base, u16 = bc.quantize(pos)
    first = None
    for fl in flags:
        want = bc.cast(u16, idx, segs, base=base, flags=fl)
        for t, nodes in enumerate(trees(pos, idx)):
            got = ca.bvh_cast_model(nodes, u16, idx, segs, base=base, flags=fl, **kw)
            if got.tobytes() != want.tobytes():
                bad = int(np.flatnonzero(got != want)[0])
                raise AssertionError("%s flags %d tree %d: segment %d %s: got %s expected %s" % (tag, fl, t, bad, segs[bad], got[bad], want[bad]))
        if fl == 0:
            first = want
        if fl == bc.ANY and first is not None:                          # any-hit against the status of the nearest run
            assert (want["status"] == first["status"]).all() and (want["face"] == bc.NO_FACE).all()
    return first


# ---- 1. the smallest trees, the generators, both index widths ----

@pytest.mark.parametrize("F", [1, 2, 3])
def test_smallest(F):
    pos, idx = bvh.strip(F, seed=F)
    segs = np.concatenate([bc.random_segments(pos, 200, seed=F, margin=100), bc.vertex_shots(pos, range(len(pos)))])
    rec = agree(pos, idx, segs, tag="strip %d" % F)
    assert (rec["status"] == bc.HIT).any() and (rec["status"] == bc.MISS).any()
    if F == 1:
        assert ca.bvh_model(pos, idx)[0][0]["right"] == bvh.LEAF        # the root is a leaf


@pytest.mark.parametrize("gen", ["lattice", "strip", "disc", "lattice_u16"])
def test_generators(gen):
    if gen == "lattice":
        pos, idx = bvh.lattice(9, extra=3)
    elif gen == "lattice_u16":
        pos, idx = bvh.lattice(7, m=5)
        idx = idx.astype(np.uint16)
    elif gen == "strip":
        pos, idx = bvh.strip(300, seed=3, spread=900)
    else:
        pos, idx = bvh.disc(400, seed=1)
    segs = np.concatenate([bc.random_segments(pos, 260, seed=5), bc.camera_grid(pos, 12, 11)])
    rec = agree(pos, idx, segs, tag=gen)
    assert (rec["status"] == bc.HIT).sum() > 20


def test_big_partition_only():
    """a blob beyond bvh_blob's limit: 4 232 faces, the tree of the tiled sort"""
    pos, idx = bvh.lattice(46)
    assert len(idx) > BLOB_FACES
    segs = np.concatenate([bc.camera_grid(pos, 9, 9), bc.random_segments(pos, 60, seed=2)])
    agree(pos, idx, segs, flags=(0, bc.ANY | bc.FRONT), tag="lattice 46")


# ---- 2. watertightness ----

def test_watertight_vertices_and_edges():
    """every shot through a vertex or an edge midpoint of a gap-free patch hits, from both sides, and a vertex shot reports the least face
    id among the faces around the vertex"""
    pos, idx = bvh.lattice(8, step=6)
    vs = bc.vertex_shots(pos, range(len(pos)))
    es = bc.edge_midpoint_shots(pos, idx, range(len(idx)))
    rec = agree(pos, idx, np.concatenate([vs, es]), tag="watertight")
    assert (rec["status"] == bc.HIT).all()
    assert set(rec["side"][:len(vs)].tolist()) == {0, 1}
    for k, r in enumerate(rec[:len(vs)]):
        v = k // 2
        around = np.flatnonzero((idx == v).any(axis=1))
        assert r["face"] == around.min() and 2 * int(r["num"]) == int(r["den"]), (v, r, around)
    # front faces only: the shot from one side hits, the one from the other side misses
    front = agree(pos, idx, vs, flags=(bc.FRONT,), tag="front")
    base, u16 = bc.quantize(pos)
    front = bc.cast(u16, idx, vs, base=base, flags=bc.FRONT)
    assert (front["status"].reshape(-1, 2).sum(axis=1) == 1).all() and (front["side"][front["status"] == bc.HIT] == 1).all()


def test_closed_surface():
    """a closed octahedron: shots from its centre through every vertex and every edge midpoint hit, and so do those coming back"""
    pos = np.array([[40, 0, 0], [-40, 0, 0], [0, 40, 0], [0, -40, 0], [0, 0, 40], [0, 0, -40]], np.int32) + 100
    idx = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.uint32)
    c = np.array([100, 100, 100])
    targets = [pos[v] for v in range(6)] + [(pos[a] + pos[b]) // 2 for f in idx for a, b in ((f[0], f[1]), (f[1], f[2]), (f[2], f[0]))]
    p = [c] * len(targets) + [c + 3 * (np.array(t) - c) for t in targets]
    q = [c + 3 * (np.array(t) - c) for t in targets] + [c] * len(targets)
    rec = agree(pos, idx, bc.segments(p, q), tag="octahedron")
    assert (rec["status"] == bc.HIT).all()
    assert (rec["side"][:len(targets)] == 0).all() and (rec["side"][len(targets):] == 1).all()   # from inside: along the normal


# ---- 3. the contract's edges ----

TRI = (np.array([[0, 0, 0], [20, 0, 0], [0, 20, 0]], np.int32), np.array([[0, 1, 2]], np.uint32))


def test_endpoints_on_the_face_and_one_step_short():
    pos, idx = TRI
    segs = bc.segments([(5, 5, 0), (5, 5, 9), (5, 5, 9), (5, 5, -9), (0, 0, 0), (5, 5, 1)],
                       [(5, 5, 9), (5, 5, 0), (5, 5, 1), (5, 5, -1), (0, 0, 7), (5, 5, -1)])
    rec = agree(pos, idx, segs, tag="endpoints")
    assert rec["status"].tolist() == [bc.HIT, bc.HIT, bc.MISS, bc.MISS, bc.HIT, bc.HIT]
    assert rec["num"][0] == 0 and rec["den"][0] > 0                      # t = 0
    assert rec["num"][1] == rec["den"][1] > 0                            # t = 1
    assert rec["num"][4] == 0                                            # a start on a vertex


def test_coplanar_and_degenerate_and_absent():
    pos = np.array([[0, 0, 0], [20, 0, 0], [0, 20, 0], [10, 10, 0], [40, 40, 5]], np.int32)
    # face 0 ordinary; 1 two equal corners; 2 collinear; 3 absent (an id >= nvert); 4 absent by 0xFFFF..
    idx = np.array([[0, 1, 2], [0, 0, 1], [1, 3, 2], [0, 1, 5], [0, 1, 0xFFFFFFF0]], np.uint32)
    segs = bc.segments([(-5, 5, 0), (1, 1, 0), (10, 10, 5), (10, 0, 5), (15, 5, 5)], [(30, 5, 0), (3, 3, 0), (10, 10, -5), (10, 0, -5), (15, 5, -5)])
    rec = agree(pos, idx, segs, tag="coplanar")
    assert rec["status"].tolist() == [bc.MISS, bc.MISS, bc.HIT, bc.HIT, bc.HIT] and (rec["face"][2:] == 0).all()
    # all faces absent or degenerate: nothing is ever hit
    rec = agree(pos, idx[1:], segs, tag="nothing")
    assert (rec["status"] == bc.MISS).all()
    # nvert below the array's length makes faces absent without touching the buffer's tail
    base, u16 = bc.quantize(pos)
    for nodes in trees(pos[:2], idx[:1]):
        got = ca.bvh_cast_model(nodes, u16, idx[:1], segs, base=base, nvert=2)
        assert got.tobytes() == bc.cast(u16, idx[:1], segs, base=base, nvert=2).tobytes() and (got["status"] == bc.MISS).all()


def test_coincident_faces_lower_id_wins():
    pos = np.array([[0, 0, 0], [20, 0, 0], [0, 20, 0], [0, 0, 0], [20, 0, 0], [0, 20, 0], [0, 0, 3], [20, 0, 3], [0, 20, 3]], np.int32)
    for perm in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        idx = np.array([[6, 7, 8], [3, 5, 4], [0, 1, 2]], np.uint32)[perm]
        rec = agree(pos, idx, bc.segments([(5, 5, -9), (5, 5, 9)], [(5, 5, 9), (5, 5, -9)]), tag="coincident")
        lower = min(k for k in range(3) if idx[k][0] in (0, 3))
        assert rec["face"][0] == lower and rec["status"][0] == bc.HIT
        assert rec["face"][1] == int(np.flatnonzero(idx[:, 0] == 6)[0])   # from above the lone upper face is nearer


def test_range_limits():
    pos, idx = TRI
    base, u16 = bc.quantize(pos + 7)
    b = np.asarray(base)
    ends = [-R, -R + 1, R - 1, R, R + 1, -R - 1]
    p, q = [], []
    for e in ends:
        for c in range(3):
            E = b.copy(); E[c] += e
            p.append(E); q.append(b + 1)
            p.append(b + 1); q.append(E)
    p += [b - R, b + R - 1, (2**31 - 1,) * 3, (-2**31,) * 3]
    q += [b + R - 1, b - R, b, b]
    segs = bc.segments(p, q)
    for base_ in (base, base + 1000):                                    # (the range follows the base, not the world)
        want = bc.cast(u16, idx, segs, base=base_)
        for nodes in trees(pos + 7 + (np.asarray(base_) - b), idx):
            got = ca.bvh_cast_model(nodes, u16, idx, segs, base=base_)
            assert got.tobytes() == want.tobytes()
    want = bc.cast(u16, idx, segs, base=base)
    n = len(ends) * 6
    inr = np.repeat([abs(e) <= R and e != R for e in ends], 6)
    assert ((want["status"][:n] != bc.RANGE) == inr).all()
    assert want["status"][n:].tolist() == [bc.HIT, bc.HIT, bc.RANGE, bc.RANGE]
    assert all(tuple(r)[1:] == (bc.NO_FACE, 0, 0, 0, 0) for r in want[want["status"] == bc.RANGE])


def test_widest_products_do_not_overflow():
    """vertices at 0 and 65 535 with segments between the range's corners: the largest of |n|, |D|, |K|, |U|, |V|, |W| any case reaches is
    measured on Python integers and must stay below 2^63.  It comes to 2^56.2: the contract's bounds are for independent vectors, but the
    corners of one face all lie in the 2^16 cube, so from an endpoint 2^19.8 away B and C are within 2^-3 rad of each other and
    |B x C| is near 2^36.6, times |d| below 2^20.8 - the true ceiling is near 2^57.4, and a case must pass 2^55 to count as near it"""
    c = [0, 65535]
    pos = np.array([(x, y, z) for x in c for y in c for z in c], np.int32) + 12345
    idx = np.array([[0, 3, 5], [6, 5, 3], [0, 7, 1], [7, 0, 6], [1, 2, 4], [7, 4, 2], [0, 5, 6], [3, 6, 5]], np.uint32)
    base, u16 = bc.quantize(pos)
    b = np.asarray(base)
    corners = [b + np.array([x, y, z]) for x in (-R, R - 1) for y in (-R, R - 1) for z in (-R, R - 1)]
    near = [b + np.array(v) for v in ((-R, 0, 65535), (R - 1, 65535, 0), (0, -R, R - 1), (65535, R - 1, -R))]
    pts = corners + near
    segs = bc.segments([p for p in pts for q in pts if p is not q], [q for p in pts for q in pts if p is not q])
    widest = [0]
    want = bc.cast(u16, idx, segs, base=base, widest=widest)
    assert 2**55 < widest[0] < 2**63, widest[0].bit_length()
    for fl in (0, bc.FRONT):
        want = bc.cast(u16, idx, segs, base=base, flags=fl)
        for nodes in trees(pos, idx):
            assert ca.bvh_cast_model(nodes, u16, idx, segs, base=base, flags=fl).tobytes() == want.tobytes()
    assert (want["status"] == bc.HIT).any()


def test_transform_record_and_written_zero():
    pos, idx = bvh.lattice(4)
    base, u16 = bc.quantize(pos)
    segs = bc.camera_grid(pos, 5, 5)
    t = ca.QuantTransform()
    t.base[0], t.base[1], t.base[2], t.components, t.written, t.q = int(base[0]), int(base[1]), int(base[2]), 3, 1, 0.5
    want = bc.cast(u16, idx, segs, base=base)
    for nodes in trees(pos, idx):
        # the record's base is the frame: the set's own base[] is not read
        assert ca.bvh_cast_model(nodes, u16, idx, segs, base=(999, -999, 5), transform=t).tobytes() == want.tobytes()
        t0 = ca.QuantTransform.from_buffer_copy(bytes(t)); t0.written = 0
        got = ca.bvh_cast_model(nodes, u16, idx, segs, base=base, transform=t0)
        assert got.tobytes() == bc.cast(u16, idx, segs, base=base, written=False).tobytes() and (got["status"] == bc.RANGE).all()


def test_stride_8():
    pos, idx = bvh.lattice(5)
    base, u16 = bc.quantize(pos)
    rec = np.full((len(u16), 8), 0xEE, np.uint8)
    rec[:, :6] = u16.view(np.uint8).reshape(-1, 6)
    segs = np.concatenate([bc.camera_grid(pos, 6, 6), bc.random_segments(pos, 50, seed=8)])
    want = bc.cast(u16, idx, segs, base=base)
    for nodes in trees(pos, idx):
        assert ca.bvh_cast_model(nodes, rec, idx, segs, base=base).tobytes() == want.tobytes()
        assert ca.bvh_cast_model(nodes, u16, idx, segs, base=base, raw_set=lambda cs: setattr(cs, "pos_stride", 6)).tobytes() == want.tobytes()


def test_segment_counts_at_the_workgroup_edges():
    pos, idx = bvh.lattice(5)
    base, u16 = bc.quantize(pos)
    nodes = trees(pos, idx)[0]
    all_ = bc.random_segments(pos, 257, seed=4)
    want = bc.cast(u16, idx, all_, base=base)
    for n in (0, 1, 63, 64, 65, 257):
        got = ca.bvh_cast_model(nodes, u16, idx, all_[:n], base=base)
        assert len(got) == n and got.tobytes() == want[:n].tobytes()


def clustered(levels, per=3, seed=0):
    """faces in clusters that halve in size and distance level after level: long common Morton prefixes, the tallest trees these inputs give"""
    rng = np.random.default_rng(seed)
    pos, at = [], 0
    for k in range(levels):
        size = max(1, (1 << 15) >> k)
        for _ in range(per):
            o = at + rng.integers(0, size, 3)
            pos += [o, o + (1, 0, 0), o + (0, 1, 1)]
        at += size
    pos = np.array(pos, np.int32)
    return pos, np.arange(len(pos), dtype=np.uint32).reshape(-1, 3)


def test_tallest_tree():
    """the tallest tree the generators give: `clustered` reaches height 20 at 48 faces (a lattice of 128 faces: 9; the contract allows 64,
    30 from the Morton bits and the rest from runs of equal keys).  The hook's stack of 65 entries is never the limit on a valid tree"""
    pos, idx = clustered(16)
    height = ca.bvh_model(pos, idx)[3].height
    assert height >= 15, height
    segs = np.concatenate([bc.random_segments(pos, 150, seed=9, margin=3), bc.vertex_shots(pos, range(0, len(pos), 3), reach=4)])
    rec = agree(pos, idx, segs, tag="clustered")
    assert (rec["status"] == bc.HIT).any()


def test_statistics_count_fewer_nodes_than_faces():
    pos, idx = bvh.lattice(20)
    base, u16 = bc.quantize(pos)
    segs = bc.camera_grid(pos, 10, 10)
    _, (nodes_taken, faces_tested) = ca.bvh_cast_model(trees(pos, idx)[0], u16, idx, segs, base=base, with_stats=True)
    assert 0 < faces_tested < len(segs) * len(idx) // 20 and nodes_taken >= len(segs)


# ---- 4. corrupt trees: the hook ONLY, never a device ----

def node(lo, left, hi, right):
    return (lo, left, hi, right)


BIG = ((-100000,) * 3, (100000,) * 3)


def corrupt(kind, F):
    nn = 2 * F - 1
    nodes = np.zeros(nn, bvh.NODE)
    for k in range(nn):                                                  # every node a leaf of face 0 with a box around everything
        nodes[k] = node(BIG[0], 0, BIG[1], bvh.LEAF)
    if kind == "cycle":
        nodes[0] = node(BIG[0], 1, BIG[1], 2)
        nodes[1] = node(BIG[0], 0, BIG[1], 2)                            # back to the root
    elif kind == "self":
        nodes[0] = node(BIG[0], 0, BIG[1], 0)
    elif kind == "child":
        nodes[0] = node(BIG[0], 1, BIG[1], nn)                           # the first id outside
    elif kind == "child_far":
        nodes[0] = node(BIG[0], 0xFFFFFFFE, BIG[1], 1)
    elif kind == "leaf":
        nodes[0] = node(BIG[0], 1, BIG[1], 2)
        nodes[1] = node(BIG[0], F, BIG[1], bvh.LEAF)                     # a face id outside
    elif kind == "chain":                                                # 70 internal nodes down the left side: a stack of 66
        for k in range(70):
            nodes[k] = node(BIG[0], k + 1, BIG[1], 100 + k)
    elif kind == "garbage":
        rng = np.random.default_rng(F)
        nodes = np.frombuffer(rng.integers(0, 256, nn * 32, dtype=np.uint8).tobytes(), bvh.NODE).copy()
        nodes[0] = node((-2**31,) * 3, int(nodes[0]["left"]), (2**31 - 1,) * 3, int(nodes[0]["right"]) | 1)
    return nodes


@pytest.mark.parametrize("kind,F", [("cycle", 2), ("cycle", 300), ("self", 2), ("self", 40), ("child", 2), ("child_far", 5), ("leaf", 2), ("chain", 100)])
def test_corrupt_tree_ends_with_tree_status(kind, F):
    pos = np.array([[0, 0, 500], [9, 0, 500], [0, 9, 500]], np.int32)          # the face lies off every segment: no early hit
    idx = np.zeros((F, 3), np.uint32); idx[:] = (0, 1, 2)
    base, u16 = bc.quantize(pos)
    segs = bc.segments([(1, 1, 10), (3, 3, 400)], [(1, 1, -10), (3, 3, 300)])
    for fl in (0, bc.ANY):
        got = ca.bvh_cast_model(corrupt(kind, F), u16, idx, segs, base=base, flags=fl)
        assert all(tuple(r) == (bc.TREE, bc.NO_FACE, 0, 0, 0, 0) for r in got), (kind, got)


@pytest.mark.parametrize("F", [1, 2, 33, 500])
def test_garbage_nodes_end_in_bounded_time(F):
    pos, idx = bvh.strip(F, seed=F, spread=300)
    base, u16 = bc.quantize(pos)
    segs = bc.random_segments(pos, 64, seed=F)
    _, (taken, _) = ca.bvh_cast_model(corrupt("garbage", F), u16, idx, segs, base=base, with_stats=True)
    assert taken <= len(segs) * (2 * F - 1)


# ---- 5. the call's errors, in order ----

def refused(raw_set, word):
    pos, idx = TRI
    base, u16 = bc.quantize(pos)
    with pytest.raises(ca.CortoError) as e:
        ca.bvh_cast_model(trees(pos, idx)[0], u16, idx, bc.segments([(1, 1, 5)], [(1, 1, -5)]), base=base, raw_set=raw_set)
    assert e.value.code == -8 and word in str(e.value), str(e.value)


def test_set_errors_in_order():
    def put(**kw):
        def f(cs):
            for k, v in kw.items():
                setattr(cs, k, (getattr(cs, k) or 0) + v if k in ("nodes", "position", "index", "segments") and v else v)
        return f
    for field, off in (("nodes", 8), ("position", 1), ("index", 2), ("segments", 8)):
        refused(put(**{field: off}), field)
        refused(put(**{field: None}), field)
    refused(lambda cs: setattr(cs, "transform", 0x1008), "transform")
    refused(put(nface=0), "nface")
    refused(put(nface=2**31), "nface")
    refused(put(index_format=ca.FMT_INT32), "index_format")
    refused(put(index_format=ca.FMT_FLOAT), "index_format")
    for s in (2, 5, 7, 9):
        refused(put(pos_stride=s), "pos_stride")
    refused(put(flags=4), "flags")
    refused(put(flags=0x80000001), "flags")
    refused(put(reserved=1), "reserved")
    # the order: the first of several wins
    refused(put(nodes=8, nface=0, reserved=1), "nodes")
    refused(put(segments=None, nface=0), "segments")
    refused(put(nface=0, index_format=9, pos_stride=7, flags=8, reserved=1), "nface")
    refused(put(index_format=9, pos_stride=7, flags=8, reserved=1), "index_format")
    refused(put(pos_stride=7, flags=8, reserved=1), "pos_stride")
    refused(put(flags=8, reserved=1), "flags")
    # a uint16 index is held to 2 bytes, a uint32 one to 4
    pos, idx = TRI
    base, u16 = bc.quantize(pos)
    nodes = trees(pos, idx)[0]
    seg = bc.segments([(1, 1, 5)], [(1, 1, -5)])
    with pytest.raises(ca.CortoError):
        ca.bvh_cast_model(nodes, u16, idx.astype(np.uint16), seg, base=base, raw_set=lambda cs: setattr(cs, "index", cs.index + 1))
    # no segments: the arrays are not looked at, the scalar fields are
    assert len(ca.bvh_cast_model(nodes, u16, idx, seg[:0], base=base, raw_set=lambda cs: setattr(cs, "nodes", 8))) == 0
    with pytest.raises(ca.CortoError):
        ca.bvh_cast_model(nodes, u16, idx, seg[:0], base=base, raw_set=lambda cs: setattr(cs, "flags", 4))


def test_null_arguments_without_a_device():
    L = ca.lib()
    assert L.crthip_bvh_cast(None, 0, None) == -8 and b"ctx" in L.crthip_last_error()
    assert L.crthip_bvh_cast(None, 1, None) == -8 and b"ctx" in L.crthip_last_error()
    assert L.crthip_bvh_cast_model(None, None) == -8
    cs = ca.CastSet()
    cs.nface, cs.nseg, cs.nodes, cs.position, cs.index, cs.segments = 1, 1, 0x1000, 0x1000, 0x1000, 0x1000
    assert L.crthip_bvh_cast_model(C.byref(cs), None) == -8 and b"hits" in L.crthip_last_error()


def test_helpers():
    s = ca.make_segments([(1, 2, 3)], [(4, 5, 6)])
    assert s.dtype == ca.SEGMENT_DTYPE and s.itemsize == 32 and ca.CAST_HIT_DTYPE.itemsize == 32 and C.sizeof(ca.CastSet) == 88
    assert tuple(s["p"][0]) == (1, 2, 3) and tuple(s["q"][0]) == (4, 5, 6)
    w = ca.world_segments([(0.5, -0.5, 1.24)], [(1.5, 2.5, -1.26)], 0.5)
    assert tuple(w["p"][0]) == (1, -1, 2) and tuple(w["q"][0]) == (3, 5, -3)      # (1.24 / 0.5 = 2.48 -> 2, -1.26 / 0.5 = -2.52 -> -3)
    assert bc.SEGMENT == ca.SEGMENT_DTYPE and bc.HITREC == ca.CAST_HIT_DTYPE


def test_fast_model_equals_the_model():
    """tests/bvh_cast.py's numpy brute force, which the GPU tests use on blobs of thousands of faces, against the one in Python integers"""
    cases = [bvh.lattice(6), bvh.strip(40, seed=2, spread=500), (TRI[0], TRI[1])]
    c = [0, 65535]
    cases.append((np.array([(x, y, z) for x in c for y in c for z in c], np.int32), np.array([[0, 3, 5], [6, 5, 3], [0, 7, 1], [1, 2, 99]], np.uint32)))
    for k, (pos, idx) in enumerate(cases):
        base, u16 = bc.quantize(pos)
        b = np.asarray(base)
        segs = np.concatenate([bc.random_segments(pos, 80, seed=k), bc.vertex_shots(pos, range(min(len(pos), 20))), bc.edge_midpoint_shots(pos, idx, [0]),
                               bc.segments([b - R, b + R - 1, b + R], [b + R - 1, b - R, b])])
        for fl in (0, bc.ANY, bc.FRONT, bc.ANY | bc.FRONT):
            assert bc.cast_fast(u16, idx, segs, base=base, flags=fl).tobytes() == bc.cast(u16, idx, segs, base=base, flags=fl).tobytes(), (k, fl)
        assert bc.cast_fast(u16, idx, segs, base=base, written=False).tobytes() == bc.cast(u16, idx, segs, base=base, written=False).tobytes()
