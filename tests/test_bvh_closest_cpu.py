"""crthip_bvh_closest without a device: the kernel's source on the host (corto_amd.bvh_closest_model: csrc/bvh_closest.h, one workgroup of 64
points after another) against the sequential model of the contract (tests/bvh_closest.py: every face, no tree, distances in rationals), byte
for byte, on trees from corto_amd.bvh_model in both partitions and in both child orders; the contract's edges - ties, the inclusive radius,
degenerate and absent faces, the range, products beyond 128 bits -; corrupt trees, which go to the hook ONLY; the call's errors as far as
they can be reached without a device (the others: tests/test_bvh_closest_gpu.py)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import corto_amd as ca
import bvh
import bvh_closest as bc

BLOB_FACES = 4096                                           # bvh_blob's limit as csrc/bvh.h states it
R = 1 << 19
FILL = 0xCD


def trees(pos, idx):
    """the nodes of both partitions (one where the blob is beyond bvh_blob's limit), which the BVH's own tests hold equal"""
    out = []
    for which in (0, 1):
        if which == 0 and len(idx) > BLOB_FACES:
            continue
        out.append(ca.bvh_model(pos, idx, which=which, seed=which * 7)[0])
    return out


def agree(pos, idx, pts, flags=bc.FLAGS, tag="", fast=False, u16=None, base=None, orders=(0, 1), **kw):
    """the hook on every tree and in both child orders equals the model under every flag combination; returns {flags: records}"""
    if base is None:
        base, u16 = bc.quantize(pos)
    cands = None if fast else bc.candidates(u16, idx, pts, base=base)
    out = {}
    for fl in flags:
        want = bc.closest_fast(u16, idx, pts, base=base, flags=fl) if fast else bc.closest(u16, idx, pts, base=base, flags=fl, cands=cands)
        for t, nodes in enumerate(trees(pos, idx)):
            for order in orders:
                got = ca.bvh_closest_model(nodes, u16, idx, pts, base=base, flags=fl, fill=FILL, order=order, **kw)
                if got.tobytes() != want.tobytes():
                    bad = int(np.flatnonzero(got != want)[0])
                    raise AssertionError("%s flags %d tree %d order %d: point %d %s: got %s expected %s" % (tag, fl, t, order, bad, pts[bad], got[bad], want[bad]))
        out[fl] = want
    if bc.WITHIN in out and bc.WITHIN | bc.ANY in out:                    # ANY says HIT exactly where WITHIN finds a face
        assert ((out[bc.WITHIN]["status"] == bc.HIT) == (out[bc.WITHIN | bc.ANY]["status"] == bc.HIT)).all()
    return out


def conditions(pos, idx, pts, out, features=range(7)):
    """what the inputs must show on the MODEL's answer, before any hook's answer counts"""
    plain, within, anyhit = out[0], out[bc.WITHIN], out[bc.WITHIN | bc.ANY]
    hit = plain["status"] == bc.HIT
    assert set(features) <= set(plain["feature"][hit].tolist()), np.bincount(plain["feature"][hit], minlength=7)
    assert (plain["status"] == bc.RANGE).any()
    assert (within["status"] == bc.HIT).any() and (within["status"] == bc.MISS).any()
    assert (anyhit["status"] == bc.HIT).any() and (anyhit["status"] == bc.MISS).any()
    assert all(tuple(r)[1:] == (bc.NO_FACE, 0, 0, 0, 0, 0, 0) for r in anyhit) and all(tuple(r)[1:] == (bc.NO_FACE, 0, 0, 0, 0, 0, 0) for r in plain[~hit])
    # a point with two or more faces at the minimum, the least id reported
    base, u16 = bc.quantize(pos)
    ties = 0
    for k in np.flatnonzero(hit)[:40]:
        num, den = bc.fractions_of(plain[k:k + 1])[0]
        c = bc.candidates(u16, idx, pts[k:k + 1], base=base, rule=bc.face_rule)[0]
        same = [f for f, n, d, _ in c if n * den == num * d]
        assert min(same) == plain["face"][k]
        ties += len(same) >= 2
    assert ties >= 1
    # the radius is inclusive: beside()'s three copies - at exactly r, at r - 1, at 0
    k = int(np.flatnonzero((pts["radius"][:-2] == 17) & (pts["radius"][1:-1] == 16) & (pts["radius"][2:] == 0))[0])
    assert bc.fractions_of(plain[k:k + 1])[0] == (17 * 17, 1) and plain["feature"][k] < 3
    assert within["status"][k] == bc.HIT and within[k].tobytes() == plain[k].tobytes() and within["status"][k + 1] == bc.MISS and within["status"][k + 2] == bc.MISS
    assert plain[k].tobytes() == plain[k + 1].tobytes() == plain[k + 2].tobytes()       # (without WITHIN the radius is a user word)


# ---- 1. the named meshes, both partitions, both orders, every flag combination ----

@pytest.mark.parametrize("name", ["strip1", "lattice1", "lattice12"])
def test_small_meshes_against_the_rational_model(name):
    pos, idx = {"strip1": lambda: bvh.strip(1, seed=1), "lattice1": lambda: bvh.lattice(1), "lattice12": lambda: bvh.lattice(12, step=6)}[name]()
    pts = bc.mixed(pos, idx, n=12 if name == "lattice12" else 120, seed=3, some=6 if name == "lattice12" else 10)
    out = agree(pos, idx, pts, tag=name)
    if name != "strip1":                                                 # (one face: no ties)
        conditions(pos, idx, pts, out)
    else:
        assert ca.bvh_model(pos, idx)[0][0]["right"] == bvh.LEAF and set(range(7)) <= set(out[0]["feature"].tolist())


@pytest.mark.parametrize("name", ["f4096", "f4097"])
def test_big_meshes_against_the_fast_model(name):
    pos, idx = {"f4096": lambda: bvh.lattice(32, m=64), "f4097": lambda: bvh.lattice(32, m=64, extra=1)}[name]()
    assert len(idx) == BLOB_FACES + (name == "f4097")
    pts = bc.mixed(pos, idx, n=60, seed=5)
    out = agree(pos, idx, pts, tag=name, fast=True)
    conditions(pos, idx, pts, out, features=(0, 3, 6))


def test_fast_model_and_the_candidate_rule_equal_the_rational_model():
    cases = [bvh.lattice(3), bvh.strip(25, seed=2, spread=40), bvh.strip(12, seed=4, spread=2000)]
    c = [0, 65535]
    cases.append((np.array([(x, y, z) for x in c for y in c for z in c], np.int32), np.array([[0, 3, 5], [6, 5, 3], [0, 7, 1], [1, 2, 99], [4, 4, 2], [1, 1, 1]], np.uint32)))
    for k, (pos, idx) in enumerate(cases):
        base, u16 = bc.quantize(pos)
        pts = bc.mixed(pos, idx, n=40, seed=k, some=8)
        slow, rule = bc.candidates(u16, idx, pts, base=base), bc.candidates(u16, idx, pts, base=base, rule=bc.face_rule)
        assert slow == rule, k                                           # every face of every point: num, den and feature
        for fl in bc.FLAGS:
            a = bc.closest(u16, idx, pts, base=base, flags=fl, cands=slow)
            assert a.tobytes() == bc.closest_fast(u16, idx, pts, base=base, flags=fl).tobytes(), (k, fl)
            assert a.tobytes() == bc.closest_fast(u16, idx, pts, base=base, flags=fl, rule=bc.face_rule).tobytes(), (k, fl)
        a = bc.closest(u16, idx, pts, base=base, written=False)
        assert a.tobytes() == bc.closest_fast(u16, idx, pts, base=base, written=False).tobytes() and (a["status"] == bc.RANGE).all()


# ---- 2. the contract's edges ----

TRI = (np.array([[0, 0, 0], [20, 0, 0], [0, 20, 0]], np.int32), np.array([[0, 1, 2]], np.uint32))


def test_every_feature_of_one_triangle():
    pos, idx = TRI
    p = [(-3, -4, 0), (25, -1, 2), (-1, 26, -2), (7, -5, 0), (15, 15, 3), (-6, 9, 1), (5, 5, 9), (5, 5, 0), (10, 10, 0), (10, 0, 0), (0, 0, 0)]
    out = agree(pos, idx, bc.points(p, 5), tag="features")
    assert out[0]["feature"].tolist() == [0, 1, 2, 3, 4, 5, 6, 6, 4, 3, 0]
    assert bc.fractions_of(out[0][:7]) == [(25, 1), (30, 1), (41, 1), (25 * 400, 400), (59 * 800, 800), (37 * 400, 400), (81 * 160000, 160000)]
    assert out[bc.WITHIN]["status"].tolist() == [1, 0, 0, 1, 0, 0, 0, 1, 1, 1, 1]              # 25 <= 5^2 <= 25; the others are farther


def test_degenerate_and_absent_faces():
    pos = np.array([[0, 0, 0], [20, 0, 0], [0, 20, 0], [10, 10, 0], [40, 40, 5]], np.int32)
    # face 0 ordinary; 1 two equal corners (a segment); 2 collinear (a segment); 3 all equal (a point); 4 absent (an id >= nvert); 5 absent by 0xFFFF..
    idx = np.array([[0, 1, 2], [0, 0, 1], [1, 3, 2], [4, 4, 4], [0, 1, 5], [0, 1, 0xFFFFFFF0]], np.uint32)
    pts = np.concatenate([bc.points([(10, -4, 0), (12, 12, 0), (13, 13, 0), (40, 40, 9), (41, 40, 5), (10, 0, 0), (30, 30, 1)], 4), bc.random_points(pos, 80, seed=1, margin=6, radius=8)])
    out = agree(pos, idx, pts, tag="degenerate")
    rec = out[0]
    # (faces 1 and 2 lie on face 0's border: at equal distance the least id, face 0, with ITS feature)
    assert rec["face"][:7].tolist() == [0, 0, 0, 3, 3, 0, 3] and rec["feature"][:7].tolist() == [3, 4, 4, 0, 0, 3, 0]
    assert bc.fractions_of(rec[2:3]) == [(18 * 800, 800)]
    # the degenerate faces alone: segments and a point
    out = agree(pos, idx[1:4], pts, tag="segments")
    assert (out[0]["status"] == bc.HIT).all() and (out[0]["feature"] <= 5).all() and {0, 1, 2} == set(out[0]["face"].tolist())
    # all faces absent: the tree is all empty boxes, every point gets the MISS record
    out = agree(pos, idx[4:], pts, tag="nothing")
    assert all(all(tuple(r) == bc.record(bc.MISS) for r in out[fl]) for fl in bc.FLAGS)
    # nvert below the array's length makes faces absent without touching the buffer's tail
    base, u16 = bc.quantize(pos)
    for nodes in trees(pos[:4], idx[:3]):
        got = ca.bvh_closest_model(nodes, u16, idx[:3], pts, base=base, nvert=4)
        assert got.tobytes() == bc.closest(u16, idx[:3], pts, base=base, nvert=4).tobytes()
    for nodes in trees(pos[:2], idx[:1]):
        got = ca.bvh_closest_model(nodes, u16, idx[:1], pts, base=base, nvert=2)
        assert (got["status"] == bc.MISS).all()


def test_absent_faces_among_a_mesh():
    pos, idx = bvh.lattice(6, extra=2)
    idx = idx.copy()
    idx[5, 1] = len(pos) + 3; idx[40, 0] = 0xFFFFFFFF; idx[41] = idx[41][[0, 0, 1]]
    pts = np.concatenate([bc.off_centroids(pos, bvh.lattice(6, extra=2)[1], [5, 40, 41, 7], heights=(0, 2)), bc.random_points(pos, 40, seed=2)])
    out = agree(pos, idx, pts, tag="absent")
    assert not ({5, 40} & set(out[0]["face"].tolist())) and (out[0]["status"] == bc.HIT).all()


def test_products_beyond_128_bits():
    """corners at 0 and 65 535 on every axis against points at the range's corners: the model's comparisons must form a product of at least
    2^128 - where a 128-bit comparison would be wrong - and stay below the contract's 2^178"""
    c = [0, 65535]
    pos = np.array([(x, y, z) for x in c for y in c for z in c], np.int32) + 12345
    idx = np.array([[0, 3, 5], [6, 5, 3], [0, 7, 1], [7, 0, 6], [1, 2, 4], [7, 4, 2], [0, 5, 6], [3, 6, 5]], np.uint32)
    base, u16 = bc.quantize(pos)
    b = np.asarray(base)
    near = [b + np.array(v) for v in ((-R, 0, 65535), (R - 1, 65535, 0), (0, -R, R - 1), (65535, R - 1, -R), (0, 0, 0), (65535, 65535, 65535), (30000, 30000, 30000),
                                      (-R, 20000, 40000), (70000, 70000, -R), (40000, R - 1, 20000), (R - 1, R - 1, 30000))]
    pts = np.concatenate([bc.range_corners(base), bc.points(near, 1 << 20), bc.points(near, 300000), bc.off_centroids(pos, idx, range(len(idx)), heights=(5, -300), radius=100)])
    widest = [0]
    want = bc.closest(u16, idx, pts, base=base, rule=bc.face_rule, widest=widest)
    print("widest product: 2^%.2f" % np.log2(float(widest[0])))
    assert 2**128 <= widest[0] < 2**178, widest[0].bit_length()
    assert (want["num_hi"] > 0).any() and (want["den_hi"] > 0).any() and 6 in want["feature"]
    out = agree(pos, idx, pts, tag="wide")
    assert out[0].tobytes() == want.tobytes()
    assert (out[bc.WITHIN]["status"] == bc.MISS).any() and (out[bc.WITHIN]["status"] == bc.HIT).any()


def test_radius_limits():
    pos, idx = TRI
    base, u16 = bc.quantize(pos)
    far = np.asarray(base) + (R - 1, R - 1, R - 1)                       # |A|^2 of the nearest corner, far beyond 2^32
    d2 = min(int(((far - p) ** 2).sum()) for p in pos.astype(np.int64))
    r = int(np.sqrt(float(d2)))
    while r * r < d2:
        r += 1
    pts = bc.points([far] * 6 + [(3, 3, 0)] * 3, [r, r - 1, 1 << 21, (1 << 21) + 1, 0xFFFFFFFF, 0, 0, 1, 0xFFFFFFFF])
    out = agree(pos, idx, pts, tag="radius")
    assert out[bc.WITHIN]["status"].tolist() == [1, 0, 1, 1, 1, 0, 1, 1, 1]
    assert len(set(out[0][:6].tobytes()[k * 48:(k + 1) * 48] for k in range(6))) == 1


@pytest.mark.parametrize("shift", ["zero", "negative", "off_minimum"])
def test_bases(shift):
    pos, idx = bvh.lattice(5)
    if shift == "zero":
        pos = (pos - pos.min(axis=0)).astype(np.int32)
    base, u16 = bc.quantize(pos)
    assert (base == 0).all() if shift == "zero" else (base < 0).all()
    if shift == "off_minimum":                                           # the frame is base + u16, whatever the base is
        base, u16 = base - (100, 7, 60000), u16 + np.array([100, 7, 60000], np.uint16)
    agree(pos, idx, bc.mixed(pos, idx, n=30, seed=6, some=5), flags=(0, bc.WITHIN), tag=shift, base=base, u16=u16, fast=True)


def test_range_limits():
    pos, idx = TRI
    base, u16 = bc.quantize(pos + 7)
    b = np.asarray(base)
    ends = [-R, -R + 1, R - 1, R, R + 1, -R - 1]
    p = []
    for e in ends:
        for c in range(3):
            E = b.copy(); E[c] += e
            p.append(E)
    p += [b - R, b + R - 1, b + R, (-2**31,) * 3, (2**31 - 1,) * 3]
    pts = bc.points(p, 1 << 21)
    for base_ in (base, base + 1000):                                    # (the range follows the base, not the world)
        want = bc.closest(u16, idx, pts, base=base_)
        for nodes in trees(pos + 7 + (np.asarray(base_) - b), idx):
            assert ca.bvh_closest_model(nodes, u16, idx, pts, base=base_).tobytes() == want.tobytes()
    want = bc.closest(u16, idx, pts, base=base)
    n = len(ends) * 3
    inr = np.repeat([abs(e) <= R and e != R for e in ends], 3)
    assert ((want["status"][:n] != bc.RANGE) == inr).all()
    assert want["status"][n:].tolist() == [bc.HIT, bc.HIT, bc.RANGE, bc.RANGE, bc.RANGE]
    assert all(tuple(r) == bc.record(bc.RANGE) for r in want[want["status"] == bc.RANGE])


def test_transform_record_and_written_zero():
    pos, idx = bvh.lattice(4)
    base, u16 = bc.quantize(pos)
    pts = bc.mixed(pos, idx, n=20, seed=1, some=4)
    t = ca.QuantTransform()
    t.base[0], t.base[1], t.base[2], t.components, t.written, t.q = int(base[0]), int(base[1]), int(base[2]), 3, 1, 0.5
    want = bc.closest_fast(u16, idx, pts, base=base)
    for nodes in trees(pos, idx):
        # the record's base is the frame: the set's own base[] is not read
        assert ca.bvh_closest_model(nodes, u16, idx, pts, base=(999, -999, 5), transform=t).tobytes() == want.tobytes()
        t0 = ca.QuantTransform.from_buffer_copy(bytes(t)); t0.written = 0
        got = ca.bvh_closest_model(nodes, u16, idx, pts, base=base, transform=t0)
        assert got.tobytes() == bc.closest(u16, idx, pts, base=base, written=False).tobytes() and all(tuple(r) == bc.record(bc.RANGE) for r in got)


def test_stride_8_and_u16_index():
    pos, idx = bvh.lattice(5)
    base, u16 = bc.quantize(pos)
    rec = np.full((len(u16), 8), 0xEE, np.uint8)
    rec[:, :6] = u16.view(np.uint8).reshape(-1, 6)
    pts = bc.mixed(pos, idx, n=30, seed=8, some=5)
    for fl in (0, bc.WITHIN):
        want = bc.closest_fast(u16, idx, pts, base=base, flags=fl)
        for nodes in trees(pos, idx):
            for p, i, kw in ((rec, idx, {}), (u16, idx, dict(raw_set=lambda cs: setattr(cs, "pos_stride", 6))), (u16, idx.astype(np.uint16), {}), (rec, idx.astype(np.uint16), {})):
                assert ca.bvh_closest_model(nodes, p, i, pts, base=base, flags=fl, **kw).tobytes() == want.tobytes()
    # a uint16 index whose 0xFFFF is an absent corner
    idx16 = idx.astype(np.uint16); idx16[3, 2] = 0xFFFF
    want = bc.closest_fast(u16, idx16, pts, base=base)
    got = ca.bvh_closest_model(ca.bvh_model(pos, idx16.astype(np.uint32))[0], u16, idx16, pts, base=base)
    assert got.tobytes() == want.tobytes() and 3 not in got["face"]


def test_point_counts_at_the_workgroup_edges():
    pos, idx = bvh.lattice(5)
    base, u16 = bc.quantize(pos)
    nodes = trees(pos, idx)[0]
    all_ = bc.out_of_range(bc.random_points(pos, 257, seed=4), base)
    want = bc.closest_fast(u16, idx, all_, base=base, flags=bc.WITHIN)
    for n in (0, 1, 63, 64, 65, 257):
        got = ca.bvh_closest_model(nodes, u16, idx, all_[:n], base=base, flags=bc.WITHIN)
        assert len(got) == n and got.tobytes() == want[:n].tobytes()


def test_pruned_walks_take_fewer_nodes_than_an_exhaustive_one():
    """the counts themselves go to profiles/bvh_closest.md; here only: both orders prune, on the same bytes"""
    pos, idx = bvh.lattice(20)
    base, u16 = bc.quantize(pos)
    pts = bc.off_centroids(pos, idx, range(0, len(idx), 8), heights=(2,))
    nodes = trees(pos, idx)[0]
    got = {}
    for order in (0, 1):
        got[order], (taken, tested) = ca.bvh_closest_model(nodes, u16, idx, pts, base=base, with_stats=True, order=order)
        print("order %d: %.1f nodes and %.1f faces a point of %d nodes and %d faces" % (order, taken / len(pts), tested / len(pts), 2 * len(idx) - 1, len(idx)))
        assert len(pts) <= taken < len(pts) * (2 * len(idx) - 1) and 0 < tested < len(pts) * len(idx)
    assert got[0].tobytes() == got[1].tobytes()
    with pytest.raises(ca.CortoError):
        ca.bvh_closest_model(nodes, u16, idx, pts, base=base, order=2)


# ---- 3. corrupt trees: the hook ONLY, never a device ----

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
    elif kind == "chain":                                                # 70 internal nodes down the left side, the right ones internal too: a stack of 66
        for k in range(70):
            nodes[k] = node(BIG[0], k + 1, BIG[1], 100 + k)
    elif kind == "garbage":
        rng = np.random.default_rng(F)
        nodes = np.frombuffer(rng.integers(0, 256, nn * 32, dtype=np.uint8).tobytes(), bvh.NODE).copy()
        nodes[0] = node((-2**31,) * 3, int(nodes[0]["left"]), (2**31 - 1,) * 3, int(nodes[0]["right"]) | 1)
    return nodes


@pytest.mark.parametrize("kind,F", [("cycle", 2), ("cycle", 300), ("self", 2), ("self", 40), ("child", 2), ("child_far", 5), ("leaf", 2), ("chain", 100)])
def test_corrupt_tree_ends_with_tree_status(kind, F):
    """each of the four bounds - a child id, a leaf's face, the stack, the nodes taken - hit by a hand-made tree whose boxes hold everything, so
    that nothing is pruned away before the bound: the TREE record, whatever the faces would have answered (without WITHIN: under it a best
    may rightly skip the corrupt part), and nothing outside the records (bvh_closest_model holds the guards)"""
    pos = np.array([[0, 0, 500], [9, 0, 500], [0, 9, 500]], np.int32)
    idx = np.zeros((F, 3), np.uint32); idx[:] = (0, 1, 2)
    base, u16 = bc.quantize(pos)
    pts = bc.points([(2, 2, 495), (-50, -50, 0)], 1 << 21)
    for order in (0, 1):
        got = ca.bvh_closest_model(corrupt(kind, F), u16, idx, pts, base=base, order=order)
        assert all(tuple(r) == bc.record(bc.TREE) for r in got), (kind, order, got)
        for fl in (bc.WITHIN, bc.WITHIN | bc.ANY):
            got = ca.bvh_closest_model(corrupt(kind, F), u16, idx, pts, base=base, flags=fl, order=order)
            assert all(tuple(r) in (bc.record(bc.TREE), bc.record(bc.HIT)) or (r["status"] == bc.HIT and r["face"] == 0) for r in got), (kind, order, got)


@pytest.mark.parametrize("F", [1, 2, 33, 500])
def test_garbage_nodes_end_in_bounded_time(F):
    pos, idx = bvh.strip(F, seed=F, spread=300)
    base, u16 = bc.quantize(pos)
    pts = bc.random_points(pos, 64, seed=F, margin=300, radius=1 << 22)
    for fl in bc.FLAGS:
        for order in (0, 1):
            got, (taken, _) = ca.bvh_closest_model(corrupt("garbage", F), u16, idx, pts, base=base, flags=fl, with_stats=True, order=order)
            assert taken <= len(pts) * (2 * F - 1)
            assert (got["status"] <= bc.TREE).all() and (got["reserved"] == 0).all() and (got["feature"] <= 6).all()
            named = (got["status"] == bc.HIT) & (got["face"] != bc.NO_FACE)
            assert (got["face"][named] < F).all() and (got["den_lo"][named] | got["den_hi"][named]).all()
            assert all(tuple(r)[1:] == (bc.NO_FACE, 0, 0, 0, 0, 0, 0) for r in got[~named])
            assert not (fl & bc.ANY) or not named.any()


# ---- 4. the call's errors, in order ----

def refused(raw_set, word, flags=0, **kw):
    pos, idx = TRI
    base, u16 = bc.quantize(pos)
    with pytest.raises(ca.CortoError) as e:
        ca.bvh_closest_model(trees(pos, idx)[0], u16, idx, bc.points([(1, 1, -5)]), base=base, raw_set=raw_set, flags=flags, **kw)
    assert e.value.code == -8 and word in str(e.value), str(e.value)


def test_set_errors_in_order():
    def put(**kw):
        def f(cs):
            for k, v in kw.items():
                setattr(cs, k, (getattr(cs, k) or 0) + v if k in ("nodes", "position", "index", "points") and v else v)
        return f
    for field, off in (("nodes", 8), ("position", 1), ("index", 2), ("points", 8)):
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
    refused(put(flags=bc.ANY), "CRTHIP_CLOSEST_ANY")
    refused(put(reserved=1), "reserved")
    # the order: the first of several wins
    refused(put(nodes=8, nface=0, reserved=1), "nodes")
    refused(put(points=None, nface=0), "points")
    refused(put(nface=0, index_format=9, pos_stride=7, flags=4, reserved=1), "nface")
    refused(put(index_format=9, pos_stride=7, flags=4, reserved=1), "index_format")
    refused(put(pos_stride=7, flags=4, reserved=1), "pos_stride")
    refused(put(flags=4 | bc.ANY, reserved=1), "unknown flags")
    refused(put(flags=bc.ANY, reserved=1), "CRTHIP_CLOSEST_ANY")
    # a uint16 index is held to 2 bytes, a uint32 one to 4
    pos, idx = TRI
    base, u16 = bc.quantize(pos)
    nodes = trees(pos, idx)[0]
    pts = bc.points([(1, 1, -5)])
    with pytest.raises(ca.CortoError):
        ca.bvh_closest_model(nodes, u16, idx.astype(np.uint16), pts, base=base, raw_set=lambda cs: setattr(cs, "index", cs.index + 1))
    # no points: the arrays are not looked at, the scalar fields are
    assert len(ca.bvh_closest_model(nodes, u16, idx, pts[:0], base=base, raw_set=lambda cs: setattr(cs, "nodes", 8))) == 0
    for fl in (4, bc.ANY):
        with pytest.raises(ca.CortoError):
            ca.bvh_closest_model(nodes, u16, idx, pts[:0], base=base, raw_set=lambda cs: setattr(cs, "flags", fl))


def test_null_arguments_without_a_device():
    L = ca.lib()
    assert L.crthip_bvh_closest(None, 0, None) == -8 and b"ctx" in L.crthip_last_error()
    assert L.crthip_bvh_closest(None, 1, None) == -8 and b"ctx" in L.crthip_last_error()
    assert L.crthip_bvh_closest_model(None, None) == -8
    cs = ca.ClosestSet()
    cs.nface, cs.npoint, cs.nodes, cs.position, cs.index, cs.points = 1, 1, 0x1000, 0x1000, 0x1000, 0x1000
    assert L.crthip_bvh_closest_model(C.byref(cs), None) == -8 and b"hits" in L.crthip_last_error()


def test_helpers():
    p = ca.make_points([(1, 2, 3), (4, 5, 6)], [7, 8])
    assert p.dtype == ca.CLOSEST_POINT_DTYPE and p.itemsize == 16 and ca.CLOSEST_HIT_DTYPE.itemsize == 48 and C.sizeof(ca.ClosestSet) == C.sizeof(ca.CastSet) == 88
    assert [f[0] for f in ca.ClosestSet._fields_] == [{"segments": "points", "nseg": "npoint"}.get(f[0], f[0]) for f in ca.CastSet._fields_]
    assert tuple(p["p"][1]) == (4, 5, 6) and p["radius"].tolist() == [7, 8]
    w = ca.world_points([(0.74, -0.76, 1.25)], 0.5, radius=[1.01])      # the nearest grid point, halves to even; the radius rounded up
    assert tuple(w["p"][0]) == (1, -2, 2) and w["radius"][0] == 3 and ca.world_points([(0, 0, 0)], 0.5)["radius"][0] == 0
    assert bc.POINT == ca.CLOSEST_POINT_DTYPE and bc.HITREC == ca.CLOSEST_HIT_DTYPE
    assert (ca.CLOSEST_WITHIN, ca.CLOSEST_ANY) == (bc.WITHIN, bc.ANY)
    assert (ca.CLOSEST_MISS, ca.CLOSEST_HIT, ca.CLOSEST_RANGE, ca.CLOSEST_TREE) == (bc.MISS, bc.HIT, bc.RANGE, bc.TREE)
    # the float is sqrt(num/den), NaN where there is no distance
    rec = np.zeros(4, ca.CLOSEST_HIT_DTYPE)
    rec[0] = bc.record(bc.HIT, 3, 6, 81 * 160000, 160000); rec[1] = bc.record(bc.MISS); rec[2] = bc.record(bc.HIT, 1, 4, 2 << 100, 1 << 67); rec[3] = bc.record(bc.HIT, 0, 0, 0, 1)
    d = ca.closest_distance(rec)
    assert d[0] == 9.0 and np.isnan(d[1]) and d[2] == float(Fraction(2 << 100, 1 << 67)) ** 0.5 and d[3] == 0.0
    assert ca.closest_fractions(rec) == bc.fractions_of(rec)
