"""crthip_bvh_query without a device: the kernel's source on the host (corto_amd.bvh_query_model: csrc/bvh_query.h, one workgroup of 64 boxes
after another) against the sequential model of the contract (tests/bvh_query.py: every face, no tree, the default rule by clipping in
rationals), byte for byte, on trees from corto_amd.bvh_model in both partitions; the touching boxes; the contract's edges; corrupt trees,
which go to the hook ONLY; the call's errors as far as they can be reached without a device (the others: tests/test_bvh_query_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import corto_amd as ca
import bvh
import bvh_query as bq

BLOB_FACES = 4096                                           # bvh_blob's limit as csrc/bvh.h states it
R = 1 << 19
FILL = 0xCD
POISON = 0xCDCDCDCD


def trees(pos, idx):
    """the nodes of both partitions (one where the blob is beyond bvh_blob's limit), which the BVH's own tests hold equal"""
    out = []
    for which in (0, 1):
        if which == 0 and len(idx) > BLOB_FACES:
            continue
        out.append(ca.bvh_model(pos, idx, which=which, seed=which * 7)[0])
    return out


def mixed(pos, idx, n=60, seed=0, touching=12):
    """every generator of tests/bvh_query.py on one mesh: the touching pairs, centroid boxes, random boxes with every seventh out of range,
    the whole mesh's box, empty boxes"""
    rng = np.random.default_rng(seed)
    vs = rng.choice(len(pos), min(len(pos), touching), replace=False)
    present = np.flatnonzero((np.asarray(idx).astype(np.int64) < len(pos)).all(axis=1))   # (the generators read a face's corners)
    fs = rng.choice(present, min(len(present), touching), replace=False)
    return np.concatenate([bq.vertex_touches(pos, vs), bq.edge_midpoint_touches(pos, idx, fs[:4]), bq.plane_touches(pos, idx, fs), bq.side_touches(pos),
                           bq.face_box_touches(pos, idx, fs[:4]), bq.centroid_boxes(pos, idx, fs), bq.out_of_range(bq.random_boxes(pos, n, seed=seed)),
                           bq.whole_box(pos), bq.empty_boxes(pos)])


def agree(pos, idx, bx, flags=bq.FLAGS, capacity=3, tag="", fast=False, u16=None, base=None, **kw):
    """the hook on every tree equals the model under every flag combination - records and lists, the words beyond `written` still poisoned;
    returns {flags: (records, lists)}"""
    if base is None:
        base, u16 = bq.quantize(pos)
    order = bq.order_of(pos, idx)
    model = bq.query_fast if fast else bq.query
    out = {}
    for fl in flags:
        want, lists = model(u16, idx, bx, order, base=base, flags=fl, capacity=capacity)
        faces = bq.expected_faces(want, lists, capacity, FILL)
        for t, nodes in enumerate(trees(pos, idx)):
            got, words = ca.bvh_query_model(nodes, u16, idx, bx, base=base, flags=fl, capacity=capacity, fill=FILL, **kw)
            if got.tobytes() != want.tobytes():
                bad = int(np.flatnonzero(got != want)[0])
                raise AssertionError("%s flags %d tree %d: box %d %s: got %s expected %s" % (tag, fl, t, bad, bx[bad], got[bad], want[bad]))
            if words.tobytes() != faces.tobytes():
                bad = int(np.flatnonzero((words != faces).any(axis=1))[0])
                raise AssertionError("%s flags %d tree %d: box %d %s: list %s expected %s" % (tag, fl, t, bad, bx[bad], words[bad], faces[bad]))
        out[fl] = (want, lists)
    for a, b in ((0, bq.COUNT), (bq.BOXES, bq.BOXES | bq.COUNT), (bq.INSIDE, bq.INSIDE | bq.COUNT)):    # a count pass counts what a list pass counts
        if a in out and b in out:
            assert (out[a][0]["count"] == out[b][0]["count"]).all() and (out[b][0]["written"] == 0).all() and (out[b][0]["status"] != bq.CLIPPED).all()
    if 0 in out and bq.BOXES in out and bq.INSIDE in out:                    # INSIDE implies a match, a match implies BOXES
        for li, ld, lb in zip(out[bq.INSIDE][1], out[0][1], out[bq.BOXES][1]):
            assert set(li) <= set(ld) <= set(lb)
    return out


# ---- 1. the named meshes, both partitions, every flag combination ----

@pytest.mark.parametrize("name", ["strip1", "lattice1", "lattice12"])
def test_small_meshes_against_the_rational_model(name):
    pos, idx = {"strip1": lambda: bvh.strip(1, seed=1), "lattice1": lambda: bvh.lattice(1), "lattice12": lambda: bvh.lattice(12, step=6)}[name]()
    bx = mixed(pos, idx, n=25 if name == "lattice12" else 120, seed=3, touching=10)
    out = agree(pos, idx, bx, tag=name)
    rec = out[0][0]
    assert (rec["status"] == bq.RANGE).sum() >= 3 and (rec["count"] >= 1).sum() >= 10      # (conditions on the inputs, not on the hook)
    if name == "lattice12":
        assert (rec["status"] == bq.CLIPPED).any() and (rec["count"] >= 1).sum() * 4 >= len(bx)
    if name == "strip1":
        assert ca.bvh_model(pos, idx)[0][0]["right"] == bvh.LEAF        # the root is a leaf


@pytest.mark.parametrize("name", ["f4096", "f4097", "disc"])
def test_big_meshes_against_the_fast_model(name):
    pos, idx = {"f4096": lambda: bvh.lattice(32, m=64), "f4097": lambda: bvh.lattice(32, m=64, extra=1), "disc": lambda: bvh.disc(400, seed=1)}[name]()
    assert name != "f4096" or len(idx) == BLOB_FACES
    assert name != "f4097" or len(idx) == BLOB_FACES + 1
    bx = mixed(pos, idx, n=70, seed=5)
    out = agree(pos, idx, bx, tag=name, fast=True, capacity=5)
    rec = out[0][0]
    assert (rec["status"] == bq.CLIPPED).any() and (rec["status"] == bq.RANGE).any() and (rec["count"] >= 1).sum() * 4 >= len(bx)


def test_fast_model_equals_the_model_and_the_contract_axes():
    """tests/bvh_query.py's numpy form and the contract's separating axes in Python integers against the clipping in rationals"""
    cases = [bvh.lattice(3), bvh.strip(25, seed=2, spread=40), bvh.strip(12, seed=4, spread=2000)]
    c = [0, 65535]
    cases.append((np.array([(x, y, z) for x in c for y in c for z in c], np.int32), np.array([[0, 3, 5], [6, 5, 3], [0, 7, 1], [1, 2, 99], [4, 4, 2], [1, 1, 1]], np.uint32)))
    for k, (pos, idx) in enumerate(cases):
        base, u16 = bq.quantize(pos)
        order = bq.order_of(pos, idx)
        assert (order == bvh.build(pos, idx)[2]).all()
        bx = mixed(pos, idx, n=50, seed=k, touching=8)
        for fl in bq.FLAGS:
            a = bq.query(u16, idx, bx, order, base=base, flags=fl, capacity=2)
            b = bq.query_fast(u16, idx, bx, order, base=base, flags=fl, capacity=2)
            s = bq.query(u16, idx, bx, order, base=base, flags=fl, capacity=2, rule=bq.sat_match)
            assert a[0].tobytes() == b[0].tobytes() == s[0].tobytes() and a[1] == b[1] == s[1], (k, fl)
        a = bq.query(u16, idx, bx, order, base=base, written=False)
        assert a[0].tobytes() == bq.query_fast(u16, idx, bx, order, base=base, written=False)[0].tobytes() and (a[0]["status"] == bq.RANGE).all()


# ---- 2. touching ----

def test_touching_boxes_match_and_their_twins_one_unit_away_do_not():
    pos, idx = bvh.lattice(8, step=6)
    vt = bq.vertex_touches(pos, range(len(pos)))
    pt = bq.plane_touches(pos, idx, range(len(idx)))
    st = bq.side_touches(pos)
    assert len(pt) >= 20
    out = agree(pos, idx, np.concatenate([vt, pt, st]), flags=(0,), capacity=8, tag="touching")
    rec, lists = out[0]
    v, p, s = rec[:len(vt)], rec[len(vt):len(vt) + len(pt)], rec[len(vt) + len(pt):]
    assert (v["count"][0::2] >= 1).all() and (v["count"][1::2] == 0).all()
    for k in range(len(pos)):                                            # the point box at a vertex matches exactly the faces around it
        assert sorted(lists[2 * k]) == np.flatnonzero((idx == k).any(axis=1)).tolist()
    assert (p["count"][0::2] >= 1).all() and (s["count"] == [16, 0]).all()   # (the 9 vertices of greatest x: both faces of the 8 quads beside them)
    # the twin of a plane touch misses the face that the box touched
    faces_touched = 0
    for k in range(0, len(pt), 2):
        touched = set(lists[len(vt) + k]) - set(lists[len(vt) + k + 1])
        faces_touched += bool(touched)
    assert faces_touched == len(pt) // 2
    # INSIDE: a face's own corner box holds it, and no longer one unit along x
    ft = bq.face_box_touches(pos, idx, range(len(idx)))
    rec, lists = agree(pos, idx, ft, flags=(bq.INSIDE,), capacity=4, tag="face boxes")[bq.INSIDE]
    assert all(k in lists[2 * k] for k in range(len(idx))) and (rec["count"][1::2] == 0).all()


def test_edge_midpoints_match_both_faces_of_an_edge():
    pos, idx = bvh.lattice(5, step=6)
    et = bq.edge_midpoint_touches(pos, idx, range(len(idx)))
    rec, lists = agree(pos, idx, et, flags=(0, bq.BOXES), capacity=6, tag="edges")[0]
    for f in range(len(idx)):
        for k in range(3):
            a, b = int(idx[f][k]), int(idx[f][(k + 1) % 3])
            around = set(np.flatnonzero((idx == a).any(axis=1) & (idx == b).any(axis=1)).tolist())
            assert around <= set(lists[2 * (3 * f + k)]), (f, k)


# ---- 3. the contract's edges ----

TRI = (np.array([[0, 0, 0], [20, 0, 0], [0, 20, 0]], np.int32), np.array([[0, 1, 2]], np.uint32))


def test_degenerate_and_absent_faces():
    pos = np.array([[0, 0, 0], [20, 0, 0], [0, 20, 0], [10, 10, 0], [40, 40, 5]], np.int32)
    # face 0 ordinary; 1 two equal corners (a segment); 2 collinear (a segment); 3 all equal (a point); 4 absent (an id >= nvert); 5 absent by 0xFFFF..
    idx = np.array([[0, 1, 2], [0, 0, 1], [1, 3, 2], [4, 4, 4], [0, 1, 5], [0, 1, 0xFFFFFFF0]], np.uint32)
    bx = np.concatenate([bq.boxes([(5, -3, -1), (9, 9, 0), (40, 40, 5), (41, 40, 5), (11, 11, -2), (12, 12, 0), (30, 30, 0)],
                                  [(6, 0, 1), (11, 11, 0), (40, 40, 5), (45, 45, 9), (14, 14, 2), (15, 15, 3), (45, 45, 9)]),
                         bq.whole_box(pos), bq.random_boxes(pos, 60, seed=1, margin=4, size=12)])
    out = agree(pos, idx, bx, capacity=4, tag="degenerate")
    lists = out[0][1]
    assert set(lists[0]) == {0, 1} and set(lists[1]) == {0, 2} and lists[2] == [3] and lists[3] == [] and lists[4] == [] and lists[5] == [] and lists[6] == [3]
    assert sorted(lists[7]) == [0, 1, 2, 3]
    # all faces absent: the tree is all empty boxes, nothing is ever found
    out = agree(pos, idx[4:], bx, tag="nothing")
    assert all((out[fl][0]["count"] == 0).all() for fl in bq.FLAGS)
    # nvert below the array's length makes faces absent without touching the buffer's tail
    base, u16 = bq.quantize(pos)
    for nodes in trees(pos[:4], idx[:3]):
        got, _ = ca.bvh_query_model(nodes, u16, idx[:3], bx, base=base, nvert=4, capacity=4)
        assert got.tobytes() == bq.query(u16, idx[:3], bx, bq.order_of(pos[:4], idx[:3]), base=base, nvert=4, capacity=4)[0].tobytes()
    for nodes in trees(pos[:2], idx[:1]):
        got, _ = ca.bvh_query_model(nodes, u16, idx[:1], bx, base=base, nvert=2)
        assert (got["count"] == 0).all()


def test_whole_mesh_box_lists_the_order_without_the_absent_faces():
    pos, idx = bvh.lattice(6, extra=2)
    idx = idx.copy()
    idx[5, 1] = len(pos) + 3; idx[40, 0] = 0xFFFFFFFF
    order = bvh.build(pos, idx)[2]
    present = [int(f) for f in order if f not in (5, 40)]
    F = len(idx)
    for fl in (0, bq.BOXES, bq.INSIDE):
        rec, lists = agree(pos, idx, bq.whole_box(pos), flags=(fl,), capacity=F, tag="whole")[fl]
        assert lists[0] == present and tuple(rec[0]) == (bq.OK, F - 2, F - 2, 0)


def test_capacities_around_the_count_and_null_faces():
    pos, idx = bvh.lattice(7, step=6)
    base, u16 = bq.quantize(pos)
    order = bq.order_of(pos, idx)
    bx = np.concatenate([bq.centroid_boxes(pos, idx, [30], half=9), mixed(pos, idx, n=30, seed=2, touching=6)])
    count = int(bq.query_fast(u16, idx, bx[:1], order, base=base)[0]["count"][0])
    assert count >= 4
    for fl in (0, bq.BOXES):
        for cap, status, written in ((0, bq.CLIPPED, 0), (count - 1, bq.CLIPPED, count - 1), (count, bq.OK, count), (count + 1, bq.OK, count)):
            rec, _ = agree(pos, idx, bx, flags=(fl, fl | bq.COUNT), capacity=cap, tag="capacity %d" % cap, fast=True)[fl]
            if fl == 0:
                assert tuple(rec[0]) == (status, count, written, 0)
    nodes = trees(pos, idx)[0]
    want = bq.query(u16, idx, bx, order, base=base, flags=bq.COUNT)[0]
    for cap in (0, 5):                                                    # faces NULL: legal under COUNT at any capacity, and at capacity 0 without
        got, words = ca.bvh_query_model(nodes, u16, idx, bx, base=base, flags=bq.COUNT, capacity=cap, null_faces=True)
        assert got.tobytes() == want.tobytes() and (words == POISON).all()
    got, _ = ca.bvh_query_model(nodes, u16, idx, bx, base=base, flags=0, capacity=0, null_faces=True)
    assert got.tobytes() == bq.query(u16, idx, bx, order, base=base, capacity=0)[0].tobytes() and (got["status"] == bq.CLIPPED).any()


@pytest.mark.parametrize("shift", ["zero", "negative", "off_minimum"])
def test_bases(shift):
    pos, idx = bvh.lattice(5)
    if shift == "zero":
        pos = (pos - pos.min(axis=0)).astype(np.int32)
    base, u16 = bq.quantize(pos)
    assert (base == 0).all() if shift == "zero" else (base < 0).all()
    if shift == "off_minimum":                                           # the frame is base + u16, whatever the base is
        base, u16 = base - (100, 7, 60000), u16 + np.array([100, 7, 60000], np.uint16)
    agree(pos, idx, mixed(pos, idx, n=40, seed=6, touching=5), flags=(0, bq.INSIDE), tag=shift, base=base, u16=u16)


def test_range_limits():
    pos, idx = TRI
    base, u16 = bq.quantize(pos + 7)
    b = np.asarray(base)
    ends = [-R, -R + 1, R - 1, R, R + 1, -R - 1]
    lo, hi = [], []
    for e in ends:
        for c in range(3):
            E = b.copy(); E[c] += e
            lo.append(np.minimum(E, b + 1)); hi.append(np.maximum(E, b + 1))
    lo += [b - R, b - R, (-2**31,) * 3, b, b + R]
    hi += [b + R - 1, b + R, b, (2**31 - 1,) * 3, b - R]                 # (the last: empty AND out of range - the range comes first)
    bx = bq.boxes(lo, hi)
    order = bq.order_of(pos + 7, idx)
    for base_ in (base, base + 1000):                                    # (the range follows the base, not the world)
        want = bq.query(u16, idx, bx, order, base=base_, capacity=1)[0]
        for nodes in trees(pos + 7 + (np.asarray(base_) - b), idx):
            got, _ = ca.bvh_query_model(nodes, u16, idx, bx, base=base_, capacity=1)
            assert got.tobytes() == want.tobytes()
    want = bq.query(u16, idx, bx, order, base=base, capacity=1)[0]
    n = len(ends) * 3
    inr = np.repeat([abs(e) <= R and e != R for e in ends], 3)
    assert ((want["status"][:n] != bq.RANGE) == inr).all()
    assert want["status"][n:].tolist() == [bq.OK, bq.RANGE, bq.RANGE, bq.RANGE, bq.RANGE] and want["count"][n] == 1
    assert all(tuple(r) == (bq.RANGE, 0, 0, 0) for r in want[want["status"] == bq.RANGE])


def test_empty_boxes_walk_nothing():
    pos, idx = bvh.lattice(4)
    base, u16 = bq.quantize(pos)
    bx = bq.empty_boxes(pos, 6)
    got, words, (taken, tested) = ca.bvh_query_model(trees(pos, idx)[0], u16, idx, bx, base=base, capacity=2, with_stats=True)
    assert all(tuple(r) == (bq.OK, 0, 0, 0) for r in got) and (words == POISON).all() and taken == 0 and tested == 0


def test_widest_intermediate_stays_in_64_bits():
    """vertices at 0 and 65 535 against boxes between the range's corners: the largest magnitude any intermediate of the contract's separating
    axes reaches, measured on Python integers, must stay below 2^63.  It comes to 58 544 939 745 673 200 = 2^55.70, in the plane test's
    sum h|n|: |n[c]| reaches 2^35 (edges of 2^17, doubled) and h 2^20, three terms - under the contract's 2^59, which is for independent
    factors.  A case must pass 2^55 to count as near the ceiling"""
    c = [0, 65535]
    pos = np.array([(x, y, z) for x in c for y in c for z in c], np.int32) + 12345
    idx = np.array([[0, 3, 5], [6, 5, 3], [0, 7, 1], [7, 0, 6], [1, 2, 4], [7, 4, 2], [0, 5, 6], [3, 6, 5]], np.uint32)
    base, u16 = bq.quantize(pos)
    b = np.asarray(base)
    corners = [b + np.array([x, y, z]) for x in (-R, R - 1) for y in (-R, R - 1) for z in (-R, R - 1)]
    near = [b + np.array(v) for v in ((-R, 0, 65535), (R - 1, 65535, 0), (0, -R, R - 1), (65535, R - 1, -R), (0, 0, 0), (65535, 65535, 65535), (30000, 30000, 30000))]
    pts = corners + near
    bx = bq.boxes([np.minimum(p, q) for p in pts for q in pts], [np.maximum(p, q) for p in pts for q in pts])
    order = bq.order_of(pos, idx)
    widest = [0]
    want = bq.query(u16, idx, bx, order, base=base, capacity=8, rule=lambda t, lo, hi: bq.sat_match(t, lo, hi, widest))
    print("widest intermediate: %d = 2^%.2f" % (widest[0], np.log2(float(widest[0]))))
    assert 2**55 < widest[0] < 2**63, widest[0].bit_length()
    clipped = bq.query(u16, idx, bx[::7], order, base=base, capacity=8)
    assert clipped[0].tobytes() == want[0][::7].tobytes() and clipped[1] == want[1][::7]
    for nodes in trees(pos, idx):
        got, words = ca.bvh_query_model(nodes, u16, idx, bx, base=base, capacity=8)
        assert got.tobytes() == want[0].tobytes() and words.tobytes() == bq.expected_faces(*want, 8).tobytes()
    assert (want[0]["count"] == 8).any() and (want[0]["count"] == 0).any()


def test_transform_record_and_written_zero():
    pos, idx = bvh.lattice(4)
    base, u16 = bq.quantize(pos)
    order = bq.order_of(pos, idx)
    bx = mixed(pos, idx, n=20, seed=1, touching=4)
    t = ca.QuantTransform()
    t.base[0], t.base[1], t.base[2], t.components, t.written, t.q = int(base[0]), int(base[1]), int(base[2]), 3, 1, 0.5
    want, lists = bq.query_fast(u16, idx, bx, order, base=base, capacity=3)
    for nodes in trees(pos, idx):
        # the record's base is the frame: the set's own base[] is not read
        got, words = ca.bvh_query_model(nodes, u16, idx, bx, base=(999, -999, 5), transform=t, capacity=3)
        assert got.tobytes() == want.tobytes() and words.tobytes() == bq.expected_faces(want, lists, 3).tobytes()
        t0 = ca.QuantTransform.from_buffer_copy(bytes(t)); t0.written = 0
        got, words = ca.bvh_query_model(nodes, u16, idx, bx, base=base, transform=t0, capacity=3)
        assert got.tobytes() == bq.query(u16, idx, bx, order, base=base, written=False)[0].tobytes()
        assert all(tuple(r) == (bq.RANGE, 0, 0, 0) for r in got) and (words == POISON).all()


def test_stride_8_and_u16_index():
    pos, idx = bvh.lattice(5)
    base, u16 = bq.quantize(pos)
    rec = np.full((len(u16), 8), 0xEE, np.uint8)
    rec[:, :6] = u16.view(np.uint8).reshape(-1, 6)
    bx = mixed(pos, idx, n=40, seed=8, touching=5)
    order = bq.order_of(pos, idx)
    for fl in (0, bq.INSIDE):
        want, lists = bq.query_fast(u16, idx, bx, order, base=base, flags=fl, capacity=4)
        faces = bq.expected_faces(want, lists, 4)
        for nodes in trees(pos, idx):
            for p, i, kw in ((rec, idx, {}), (u16, idx, dict(raw_set=lambda cs: setattr(cs, "pos_stride", 6))), (u16, idx.astype(np.uint16), {}), (rec, idx.astype(np.uint16), {})):
                got, words = ca.bvh_query_model(nodes, p, i, bx, base=base, flags=fl, capacity=4, **kw)
                assert got.tobytes() == want.tobytes() and words.tobytes() == faces.tobytes()
    # a uint16 index whose 0xFFFF is an absent corner
    idx16 = idx.astype(np.uint16); idx16[3, 2] = 0xFFFF
    want, lists = bq.query_fast(u16, idx16, bx, bq.order_of(pos, idx16), base=base, capacity=4)
    got, words = ca.bvh_query_model(ca.bvh_model(pos, idx16.astype(np.uint32))[0], u16, idx16, bx, base=base, capacity=4)
    assert got.tobytes() == want.tobytes() and words.tobytes() == bq.expected_faces(want, lists, 4).tobytes() and not any(3 in l for l in lists)


def test_box_counts_at_the_workgroup_edges():
    pos, idx = bvh.lattice(5)
    base, u16 = bq.quantize(pos)
    nodes = trees(pos, idx)[0]
    all_ = bq.out_of_range(bq.random_boxes(pos, 257, seed=4))
    want, lists = bq.query_fast(u16, idx, all_, bq.order_of(pos, idx), base=base, capacity=2)
    for n in (0, 1, 63, 64, 65, 257):
        got, words = ca.bvh_query_model(nodes, u16, idx, all_[:n], base=base, capacity=2)
        assert len(got) == n and got.tobytes() == want[:n].tobytes() and words.tobytes() == bq.expected_faces(want[:n], lists[:n], 2).tobytes()


def test_statistics_count_fewer_faces_than_a_brute_force():
    pos, idx = bvh.lattice(20)
    base, u16 = bq.quantize(pos)
    bx = bq.centroid_boxes(pos, idx, range(0, len(idx), 8))
    _, _, (taken, tested) = ca.bvh_query_model(trees(pos, idx)[0], u16, idx, bx, base=base, with_stats=True)
    assert 0 < tested < len(bx) * len(idx) // 20 and taken >= len(bx)


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
        nodes[1] = node(BIG[0], 0, BIG[1], 2)                            # back to the root: more than 2F - 1 nodes taken
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
    """each of the four bounds - a child id, a leaf's face, the stack, the nodes taken - hit by a hand-made tree: {TREE, 0, 0, 0}, whatever the
    faces would have matched, and nothing outside the slices (bvh_query_model holds the guards)"""
    pos = np.array([[0, 0, 500], [9, 0, 500], [0, 9, 500]], np.int32)
    idx = np.zeros((F, 3), np.uint32); idx[:] = (0, 1, 2)
    base, u16 = bq.quantize(pos)
    bx = bq.boxes([(1, 1, 490), (-50, -50, 0)], [(3, 3, 510), (-40, -40, 10)])        # one around the face, one off it
    for fl in bq.FLAGS:
        got, words = ca.bvh_query_model(corrupt(kind, F), u16, idx, bx, base=base, flags=fl, capacity=3)
        assert all(tuple(r) == (bq.TREE, 0, 0, 0) for r in got), (kind, got)
        assert ((words == POISON) | (words < F)).all()


@pytest.mark.parametrize("F", [1, 2, 33, 500])
def test_garbage_nodes_end_in_bounded_time(F):
    pos, idx = bvh.strip(F, seed=F, spread=300)
    base, u16 = bq.quantize(pos)
    bx = np.concatenate([bq.whole_box(pos), bq.random_boxes(pos, 63, seed=F, size=300)])
    for fl in (0, bq.COUNT, bq.BOXES):
        got, words, (taken, _) = ca.bvh_query_model(corrupt("garbage", F), u16, idx, bx, base=base, flags=fl, capacity=4, with_stats=True)
        assert taken <= len(bx) * (2 * F - 1)
        assert (got["status"] <= bq.TREE).all() and (got["reserved"] == 0).all() and (got["written"] <= 4).all() and (got["count"] <= 2 * F - 1).all()
        assert all(tuple(r)[1:] == (0, 0, 0) for r in got[got["status"] >= bq.RANGE])
        assert ((words == POISON) | (words < F)).all()


# ---- 5. the call's errors, in order ----

def refused(raw_set, word, flags=0, capacity=2, **kw):
    pos, idx = TRI
    base, u16 = bq.quantize(pos)
    with pytest.raises(ca.CortoError) as e:
        ca.bvh_query_model(trees(pos, idx)[0], u16, idx, bq.boxes([(1, 1, -5)], [(2, 2, 5)]), base=base, raw_set=raw_set, flags=flags, capacity=capacity, **kw)
    assert e.value.code == -8 and word in str(e.value), str(e.value)


def test_set_errors_in_order():
    def put(**kw):
        def f(cs):
            for k, v in kw.items():
                if k == "reserved":
                    cs.reserved[v] = 1
                else:
                    setattr(cs, k, (getattr(cs, k) or 0) + v if k in ("nodes", "position", "index", "boxes") and v else v)
        return f
    for field, off in (("nodes", 8), ("position", 1), ("index", 2), ("boxes", 8)):
        refused(put(**{field: off}), field)
        refused(put(**{field: None}), field)
    refused(lambda cs: setattr(cs, "transform", 0x1008), "transform")
    refused(lambda cs: None, "faces", null_faces=True)                   # no COUNT, a capacity, no list
    refused(put(nface=0), "nface")
    refused(put(nface=2**31), "nface")
    refused(put(index_format=ca.FMT_INT32), "index_format")
    refused(put(index_format=ca.FMT_FLOAT), "index_format")
    for s in (2, 5, 7, 9):
        refused(put(pos_stride=s), "pos_stride")
    refused(put(flags=8), "flags")
    refused(put(flags=0x80000001), "flags")
    for fl in (bq.BOXES | bq.INSIDE, bq.BOXES | bq.INSIDE | bq.COUNT):
        refused(put(flags=fl), "CRTHIP_QUERY_BOXES")
    refused(put(reserved=0), "reserved")
    refused(put(reserved=1), "reserved")
    # the order: the first of several wins
    refused(put(nodes=8, nface=0, reserved=1), "nodes")
    refused(put(boxes=None, nface=0), "boxes")
    refused(put(nface=0), "faces", null_faces=True)
    refused(put(nface=0, index_format=9, pos_stride=7, flags=8, reserved=1), "nface")
    refused(put(index_format=9, pos_stride=7, flags=8, reserved=1), "index_format")
    refused(put(pos_stride=7, flags=8, reserved=1), "pos_stride")
    refused(put(flags=8 | bq.BOXES | bq.INSIDE, reserved=1), "unknown flags")
    refused(put(flags=bq.BOXES | bq.INSIDE, reserved=1), "CRTHIP_QUERY_BOXES")
    # a uint16 index is held to 2 bytes, a uint32 one to 4
    pos, idx = TRI
    base, u16 = bq.quantize(pos)
    nodes = trees(pos, idx)[0]
    bx = bq.boxes([(1, 1, -5)], [(2, 2, 5)])
    with pytest.raises(ca.CortoError):
        ca.bvh_query_model(nodes, u16, idx.astype(np.uint16), bx, base=base, raw_set=lambda cs: setattr(cs, "index", cs.index + 1))
    # no boxes: the arrays are not looked at, the scalar fields are
    assert len(ca.bvh_query_model(nodes, u16, idx, bx[:0], base=base, raw_set=lambda cs: setattr(cs, "nodes", 8))[0]) == 0
    with pytest.raises(ca.CortoError):
        ca.bvh_query_model(nodes, u16, idx, bx[:0], base=base, raw_set=lambda cs: setattr(cs, "flags", 8))


def test_null_arguments_without_a_device():
    L = ca.lib()
    assert L.crthip_bvh_query(None, 0, None) == -8 and b"ctx" in L.crthip_last_error()
    assert L.crthip_bvh_query(None, 1, None) == -8 and b"ctx" in L.crthip_last_error()
    assert L.crthip_bvh_query_model(None, None, None) == -8
    qs = ca.QuerySet()
    qs.nface, qs.nbox, qs.nodes, qs.position, qs.index, qs.boxes = 1, 1, 0x1000, 0x1000, 0x1000, 0x1000
    assert L.crthip_bvh_query_model(C.byref(qs), None, None) == -8 and b"results" in L.crthip_last_error()


def test_helpers():
    b = ca.make_boxes([(1, 2, 3)], [(4, 5, 6)])
    assert b.dtype == ca.BOX_DTYPE and b.itemsize == 32 and ca.QUERY_RESULT_DTYPE.itemsize == 16 and C.sizeof(ca.QuerySet) == 104
    assert tuple(b["min"][0]) == (1, 2, 3) and tuple(b["max"][0]) == (4, 5, 6)
    w = ca.world_boxes([(0.5, -0.6, 1.24)], [(1.5, 2.6, -1.26)], 0.5)    # outward: floor for min, ceil for max
    assert tuple(w["min"][0]) == (1, -2, 2) and tuple(w["max"][0]) == (3, 6, -2)
    assert bq.BOX == ca.BOX_DTYPE and bq.RESULT == ca.QUERY_RESULT_DTYPE and ca.BVH_NODE_DTYPE.itemsize == 32
    assert (ca.QUERY_COUNT, ca.QUERY_BOXES, ca.QUERY_INSIDE) == (bq.COUNT, bq.BOXES, bq.INSIDE)
    assert (ca.QUERY_OK, ca.QUERY_CLIPPED, ca.QUERY_RANGE, ca.QUERY_TREE) == (bq.OK, bq.CLIPPED, bq.RANGE, bq.TREE)
    # the bytes of a node are a valid box: a node's own box finds the faces under it
    pos, idx = bvh.lattice(3)
    base, u16 = bq.quantize(pos)
    nodes = ca.bvh_model(pos, idx)[0]
    rec, _ = ca.bvh_query_model(nodes, u16, idx, np.frombuffer(nodes.tobytes(), ca.BOX_DTYPE), base=base, flags=bq.COUNT)
    assert rec["count"][0] == len(idx) and (rec["count"] >= 1).all() and (rec["status"] == bq.OK).all()
