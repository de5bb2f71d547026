"""A sequential model of crthip_bvh_query, written from the contract in include/corto_hip.h alone: a brute force over ALL faces in Python's
arbitrary-precision integers and rationals - no tree, nothing of csrc/bvh_query.h.  The default rule is decided by CLIPPING the triangle by
the box's six half-spaces in fractions.Fraction, so it shares no method with the kernel's separating axes; the contract's separating axes
in Python integers stand beside it (sat_match), held equal to the clipping and used to measure the widest intermediate; ranks come from the
BVH model's (key, f) order.  With it a numpy int64 fast form for big inputs, held equal to the slow one, and the box generators the tests
share.  No test here: tests/test_bvh_query_cpu.py and tests/test_bvh_query_gpu.py use it."""
from fractions import Fraction

import numpy as np

import bvh

COUNT, BOXES, INSIDE = 1, 2, 4
OK, CLIPPED, RANGE, TREE = 0, 1, 2, 3
FLAGS = (0, COUNT, BOXES, INSIDE, COUNT | BOXES, COUNT | INSIDE)          # every legal combination
R = 1 << 19
BOX = np.dtype([("min", np.int32, 3), ("user0", np.uint32), ("max", np.int32, 3), ("user1", np.uint32)])
RESULT = np.dtype([("status", np.uint32), ("count", np.uint32), ("written", np.uint32), ("reserved", np.uint32)])


# ---- the rules on one face -------------------------------------------------------------------------------------------------------------------

def clip(poly, c, bound, sign):
    """the convex polygon `poly` (a list of points, Fractions) cut by the closed half-space sign*(x[c] - bound) <= 0"""
    out = []
    for k in range(len(poly)):
        cur, nxt = poly[k], poly[(k + 1) % len(poly)]
        dc, dn = sign * (cur[c] - bound), sign * (nxt[c] - bound)
        if dc <= 0:
            out.append(cur)
        if (dc < 0 < dn) or (dn < 0 < dc):
            t = dc / (dc - dn)
            out.append(tuple(cur[i] + (nxt[i] - cur[i]) * t for i in range(3)))
    return out


def clip_match(tri, lo, hi):
    """the closed triangle (three integer points; equal or collinear ones allowed) shares a point with the closed box [lo, hi]"""
    poly = [tuple(Fraction(int(x)) for x in p) for p in tri]
    for c in range(3):
        for bound, sign in ((int(lo[c]), -1), (int(hi[c]), 1)):
            poly = clip(poly, c, bound, sign)
            if not poly:
                return False
    return True


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def sat_match(tri, lo, hi, widest=None):
    """the contract's separating axes as it words them - doubled coordinates, all three projections an axis - in Python integers; widest: a
    one-element list that keeps the largest magnitude any intermediate reached"""
    c2 = tuple(int(lo[c]) + int(hi[c]) for c in range(3))
    h = tuple(int(hi[c]) - int(lo[c]) for c in range(3))
    V = [tuple(2 * int(p[c]) - c2[c] for c in range(3)) for p in tri]
    seen = [abs(x) for v in V for x in v]
    e = [sub(V[1], V[0]), sub(V[2], V[1]), sub(V[0], V[2])]
    seen += [abs(x) for v in e for x in v]
    n = cross(e[0], e[1])
    d, r = dot(n, V[0]), sum(h[c] * abs(n[c]) for c in range(3))
    seen += [abs(x) for x in n] + [abs(d), r] + [abs(n[c] * V[0][c]) for c in range(3)]
    verdict = True
    if any(min(v[c] for v in V) > h[c] or max(v[c] for v in V) < -h[c] for c in range(3)):
        verdict = False
    if abs(d) > r:
        verdict = False
    for k in range(3):
        u = tuple(1 if c == k else 0 for c in range(3))
        for i in range(3):
            a = cross(u, e[i])
            p = [dot(a, v) for v in V]
            ra = sum(h[c] * abs(a[c]) for c in range(3))
            seen += [abs(x) for x in p] + [ra] + [abs(a[c] * v[c]) for v in V for c in range(3)]
            if min(p) > ra or max(p) < -ra:
                verdict = False
    if widest is not None:
        widest[0] = max(widest[0], max(seen))
    return verdict


def face_match(tri, lo, hi, flags, rule=clip_match):
    if flags & BOXES:
        return all(min(p[c] for p in tri) <= hi[c] and max(p[c] for p in tri) >= lo[c] for c in range(3))
    if flags & INSIDE:
        return all(lo[c] <= p[c] <= hi[c] for p in tri for c in range(3))
    return rule(tri, lo, hi)


# ---- the whole call on one set ---------------------------------------------------------------------------------------------------------------

def order_of(position, index):
    """the faces in BVH rank order: (key, f) ascending, bvh.build's `order` without building the tree (tests/test_bvh_query_cpu.py holds
    the two equal)"""
    present, bmin, bmax = bvh.face_boxes(position, index)
    keys = bvh.face_keys(present, bmin, bmax)
    return np.array(sorted(range(len(keys)), key=lambda f: (keys[f], f)), np.uint32)


def records(counts_and_status, flags, capacity):
    """RESULT records from (status, count) pairs under the contract's written / CLIPPED rule"""
    out = np.zeros(len(counts_and_status), RESULT)
    for i, (status, count) in enumerate(counts_and_status):
        if status != OK:
            out[i] = (status, 0, 0, 0)
            continue
        written = 0 if flags & COUNT else min(count, capacity)
        out[i] = (CLIPPED if written < count and not flags & COUNT else OK, count, written, 0)
    return out


def query(position_u16, index, boxes, order, base=(0, 0, 0), flags=0, capacity=0, written=True, nvert=None, rule=clip_match):
    """(RESULT records, a list a box of ALL its matching faces in rank order - not cut at the capacity) of `boxes` (BOX) against every face:
    position_u16 (nvert, 3) the buffer's halfwords, so that p[v] = base + position_u16[v]; order: the faces by rank"""
    pos = [tuple(int(x) + int(base[c]) for c, x in enumerate(row)) for row in np.asarray(position_u16).reshape(-1, 3)]
    nv = len(pos) if nvert is None else nvert
    faces = [tuple(int(x) for x in f) for f in np.asarray(index).reshape(-1, 3)]
    heads, lists = [], []
    for b in boxes:
        lo, hi = tuple(int(x) for x in b["min"]), tuple(int(x) for x in b["max"])
        if not written or not all(-R <= E[c] - int(base[c]) < R for E in (lo, hi) for c in range(3)):
            heads.append((RANGE, 0)); lists.append([])
            continue
        found = []
        if all(lo[c] <= hi[c] for c in range(3)):
            for f in order:
                ia, ib, ic = faces[int(f)]
                if ia >= nv or ib >= nv or ic >= nv:
                    continue
                if face_match((pos[ia], pos[ib], pos[ic]), lo, hi, flags, rule):
                    found.append(int(f))
        heads.append((OK, len(found))); lists.append(found)
    return records(heads, flags, capacity), lists


def query_fast(position_u16, index, boxes, order, base=(0, 0, 0), flags=0, capacity=0, written=True, nvert=None):
    """query()'s answer for big inputs: still every face and no tree, in numpy int64 over all faces of a box at once - exact, because in range
    every quantity stays far below 2^63.  tests/test_bvh_query_cpu.py holds it equal to query()"""
    base = np.asarray([int(b) for b in base], np.int64)
    pos = np.asarray(position_u16).reshape(-1, 3).astype(np.int64) + base
    nv = len(pos) if nvert is None else nvert
    idx = np.asarray(index).reshape(-1, 3).astype(np.int64)
    order = np.asarray(order, np.int64)
    present = (idx < nv).all(axis=1)
    safe = np.where(present[:, None], idx, 0)
    P = [pos[safe[:, k]] * 2 if len(pos) else np.zeros((len(idx), 3), np.int64) for k in range(3)]   # doubled corners
    heads, lists = [], []
    for b in boxes:
        lo, hi = b["min"].astype(np.int64), b["max"].astype(np.int64)
        if not written or not ((lo - base >= -R) & (lo - base < R) & (hi - base >= -R) & (hi - base < R)).all():
            heads.append((RANGE, 0)); lists.append([])
            continue
        if (lo > hi).any():
            heads.append((OK, 0)); lists.append([])
            continue
        c2, h = lo + hi, hi - lo
        V = [p - c2 for p in P]
        mn, mx = np.minimum(np.minimum(V[0], V[1]), V[2]), np.maximum(np.maximum(V[0], V[1]), V[2])
        m = present & (mn <= h).all(axis=1) & (mx >= -h).all(axis=1)
        if flags & INSIDE:
            m &= (mn >= -h).all(axis=1) & (mx <= h).all(axis=1)
        elif not flags & BOXES:
            e = [V[1] - V[0], V[2] - V[1], V[0] - V[2]]
            n = np.cross(e[0], e[1])
            m &= np.abs((n * V[0]).sum(axis=1)) <= (np.abs(n) * h).sum(axis=1)
            for k in range(3):
                i, j = (k + 1) % 3, (k + 2) % 3                          # u_k x e = -e[j] on axis i, +e[i] on axis j
                for ed in e:
                    p = [ed[:, i] * v[:, j] - ed[:, j] * v[:, i] for v in V]
                    r = h[i] * np.abs(ed[:, j]) + h[j] * np.abs(ed[:, i])
                    m &= ~((np.minimum(np.minimum(p[0], p[1]), p[2]) > r) | (np.maximum(np.maximum(p[0], p[1]), p[2]) < -r))
        found = [int(f) for f in order[m[order]]]
        heads.append((OK, len(found))); lists.append(found)
    return records(heads, flags, capacity), lists


def expected_faces(results, lists, capacity, fill=0xCD):
    """the `faces` array a call leaves in a buffer of `fill` bytes: a box's first `written` matches, the rest of its slice untouched"""
    out = np.full((len(results), capacity), fill * 0x01010101, np.uint32)
    for i, r in enumerate(results):
        w = int(r["written"])
        out[i, :w] = lists[i][:w]
    return out


def boxes(lo, hi):
    lo = np.asarray(lo, np.int64).reshape(-1, 3)
    hi = np.asarray(hi, np.int64).reshape(-1, 3)
    b = np.zeros(len(lo), BOX)
    b["min"], b["max"] = lo, hi
    b["user0"] = np.arange(len(lo), dtype=np.uint32) * 2654435761 & 0xFFFFFFFF   # (never read: any bits)
    b["user1"] = ~b["user0"]
    return b


def moved(bx, step):
    """the same boxes moved by `step` (3,) or (n, 3)"""
    out = bx.copy()
    out["min"] = bx["min"].astype(np.int64) + step
    out["max"] = bx["max"].astype(np.int64) + step
    return out


def pairs(a, b):
    """a[0], b[0], a[1], b[1], ...: every box followed by its twin"""
    out = np.zeros(2 * len(a), BOX)
    out[0::2], out[1::2] = a, b
    return out


# ---- box generators (all in absolute grid units) ---------------------------------------------------------------------------------------------
# The touching generators give PAIRS: a box that meets the mesh in its boundary only, then the same box moved one unit away.

def vertex_touches(position, ids):
    """the point box AT vertex v, then the same box one unit up the z axis"""
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    a = boxes(pos[list(ids)], pos[list(ids)])
    return pairs(a, moved(a, (0, 0, 1)))


def edge_midpoint_touches(position, index, faces):
    """around the midpoint of every edge of the named faces: [floor(m), ceil(m)] a component - the midpoint itself where it is an integer
    point - then the same box one unit up the z axis"""
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    lo, hi = [], []
    for f in faces:
        c = [int(x) for x in np.asarray(index).reshape(-1, 3)[f]]
        for k in range(3):
            s = pos[c[k]] + pos[c[(k + 1) % 3]]
            lo.append(s // 2); hi.append(-((-s) // 2))
    a = boxes(lo, hi)
    return pairs(a, moved(a, (0, 0, 1)))


def plane_touches(position, index, faces, reach=2, limit=4096):
    """for every named face that has an integer point strictly inside it: the box with one CORNER at that point that reaches `reach` units
    to the side the face's normal points to, so that it meets the face's plane in that corner only (along an in-plane segment where a normal
    component is 0); then the same box one unit further along the normal's signs"""
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    lo, hi, step = [], [], []
    for f in faces:
        a, b, c = (tuple(int(x) for x in pos[int(v)]) for v in np.asarray(index).reshape(-1, 3)[f])
        n = cross(sub(b, a), sub(c, a))
        if n == (0, 0, 0):
            continue
        mn, mx = [min(a[k], b[k], c[k]) for k in range(3)], [max(a[k], b[k], c[k]) for k in range(3)]
        if (mx[0] - mn[0] + 1) * (mx[1] - mn[1] + 1) * (mx[2] - mn[2] + 1) > limit:
            continue
        inside = None
        for x in range(mn[0], mx[0] + 1):
            for y in range(mn[1], mx[1] + 1):
                for z in range(mn[2], mx[2] + 1):
                    p = (x, y, z)
                    if dot(n, sub(p, a)) != 0:
                        continue
                    w = [dot(n, cross(sub(q1, q0), sub(p, q0))) for q0, q1 in ((a, b), (b, c), (c, a))]
                    if all(t > 0 for t in w):
                        inside = p
                        break
                if inside:
                    break
            if inside:
                break
        if inside is None:
            continue
        s = [1 if n[k] > 0 else -1 if n[k] < 0 else 1 for k in range(3)]
        lo.append([min(inside[k], inside[k] + s[k] * reach) for k in range(3)])
        hi.append([max(inside[k], inside[k] + s[k] * reach) for k in range(3)])
        step.append([s[k] if n[k] else 0 for k in range(3)])
    a = boxes(lo, hi) if lo else np.zeros(0, BOX)
    return pairs(a, moved(a, np.array(step, np.int64).reshape(-1, 3)))


def side_touches(position):
    """a slab against the +x side of the mesh's box - it meets the vertices of greatest x in its face x = max only - then one unit away"""
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    a = boxes([(hi[0], lo[1], lo[2])], [(hi[0] + 3, hi[1], hi[2])])
    return pairs(a, moved(a, (1, 0, 0)))


def face_box_touches(position, index, faces):
    """the exact corner box of the named faces - under INSIDE the face lies in it with every corner on its boundary - then one unit up x,
    which leaves the corner of least x outside"""
    _, bmin, bmax = bvh.face_boxes(position, index)
    a = boxes(bmin[list(faces)], bmax[list(faces)])
    return pairs(a, moved(a, (1, 0, 0)))


def centroid_boxes(position, index, faces, half=3):
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    c = pos[np.asarray(index).reshape(-1, 3)[list(faces)].astype(np.int64)].sum(axis=1) // 3
    return boxes(c - half, c + half)


def random_boxes(position, n, seed=0, margin=20, size=40, base=None):
    """n boxes of random place and size (up to `size` a side) in the positions' box grown by `margin`, clipped to the range of `base`
    (default: the minimum)"""
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    lo, hi = pos.min(axis=0) - margin, pos.max(axis=0) + margin
    b = pos.min(axis=0) if base is None else np.asarray(base, np.int64)
    lo, hi = np.maximum(lo, b - R), np.minimum(hi, b + R - 1)
    a = rng.integers(lo, hi + 1, (n, 3))
    return boxes(a, np.minimum(a + rng.integers(0, size + 1, (n, 3)), hi))


def whole_box(position):
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    return boxes([pos.min(axis=0)], [pos.max(axis=0)])


def empty_boxes(position, n=3):
    """in range, min > max on one axis (a different one each)"""
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    a = boxes([lo] * n, [hi] * n)
    for k in range(n):
        a["min"][k, k % 3] = a["max"][k, k % 3] + 1 + k
    return a


def out_of_range(bx, every=7, phase=3):
    """every `every`-th box pushed out of the range: its max x 2^20 further"""
    out = bx.copy()
    far = np.arange(len(out)) % every == phase
    out["max"][far, 0] += 1 << 20
    return out


def quantize(position):
    """integer positions (nvert, 3) -> (base (3,), uint16 (nvert, 3)) as CRTHIP_BIND_QUANTIZED stores them: base the minimum a component"""
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    base = pos.min(axis=0) if len(pos) else np.zeros(3, np.int64)
    rel = pos - base
    assert rel.max(initial=0) <= 65535
    return base, rel.astype(np.uint16)
