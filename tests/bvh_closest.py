"""A sequential model of crthip_bvh_closest, written from the contract in include/corto_hip.h alone: a brute force over ALL faces in Python's
integers and fractions.Fraction - no tree, no pruning, nothing of csrc/bvh_closest.h.  The distance to a face comes by a method the kernel
does not use (the clamped projection on each edge segment, then the barycentric coordinates of the plane's foot, in Fractions), the feature
from the membership of that rational closest point in the closed features; the contract's candidate rule in Python integers stands beside
it (tests/test_bvh_closest_cpu.py holds the two equal), and a numpy form for large meshes that runs the exact arithmetic only on the faces
a float64 pass cannot tell from the nearest.  With them the point generators the tests share.  No test here."""
from fractions import Fraction

import numpy as np

WITHIN, ANY = 1, 2
MISS, HIT, RANGE, TREE = 0, 1, 2, 3
NO_FACE = 0xFFFFFFFF
FLAGS = (0, WITHIN, WITHIN | ANY)                                          # every legal combination
R = 1 << 19
RMAX = 1 << 21                                                             # radii beyond it are no limit
POINT = np.dtype([("p", np.int32, 3), ("radius", np.uint32)])
HITREC = np.dtype([("status", np.uint32), ("face", np.uint32), ("feature", np.uint32), ("reserved", np.uint32), ("num_lo", np.uint64), ("num_hi", np.uint64),
                   ("den_lo", np.uint64), ("den_hi", np.uint64)])
M64 = (1 << 64) - 1


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


# ---- one face ----------------------------------------------------------------------------------------------------------------------------------

def closest_point(P, tri):
    """the point of the closed triangle `tri` (three integer points; equal or collinear ones allowed) nearest to P, and its squared distance,
    in Fractions: the least over the three edge segments with the projection clamped to [0, 1], and the plane's foot where its barycentric
    coordinates are all >= 0"""
    p = tuple(Fraction(int(x)) for x in P)
    V = [tuple(Fraction(int(x)) for x in v) for v in tri]
    best = None
    for i in range(3):
        a, b = V[i], V[(i + 1) % 3]
        ab = sub(b, a)
        l = dot(ab, ab)
        t = Fraction(0) if l == 0 else max(Fraction(0), min(Fraction(1), dot(sub(p, a), ab) / l))
        q = tuple(a[k] + t * ab[k] for k in range(3))
        d = dot(sub(q, p), sub(q, p))
        if best is None or d < best[0]:
            best = (d, q)
    a, b, c = V
    u, v = sub(b, a), sub(c, a)
    n = cross(u, v)
    nn = dot(n, n)
    if nn > 0:
        w = sub(p, a)
        g, h = dot(cross(u, w), n) / nn, dot(cross(w, v), n) / nn            # the weights of c and b
        if g >= 0 and h >= 0 and g + h <= 1:
            q = tuple(a[k] + h * u[k] + g * v[k] for k in range(3))
            d = dot(sub(q, p), sub(q, p))
            if d < best[0]:
                best = (d, q)
    return best


def feature_of(q, tri):
    """the least code whose closed feature holds the rational point q of the triangle: 0, 1, 2 the corners, 3, 4, 5 the edges ab, bc, ca, 6"""
    V = [tuple(Fraction(int(x)) for x in v) for v in tri]
    for k in range(3):
        if q == V[k]:
            return k
    for i in range(3):
        a, b = V[i], V[(i + 1) % 3]
        ab, aq = sub(b, a), sub(q, a)
        if ab != (0, 0, 0) and cross(aq, ab) == (0, 0, 0) and 0 <= dot(aq, ab) <= dot(ab, ab):   # (an edge of equal ends is that corner, met above)
            return 3 + i
    return 6


def formula(P, tri, feature):
    """{num, den} of a feature as the contract's table words it, Python integers, not reduced"""
    A = [sub(tuple(int(x) for x in v), tuple(int(x) for x in P)) for v in tri]
    e = [sub(A[(i + 1) % 3], A[i]) for i in range(3)]
    if feature < 3:
        return dot(A[feature], A[feature]), 1
    if feature < 6:
        c = cross(A[feature - 3], e[feature - 3])
        return dot(c, c), dot(e[feature - 3], e[feature - 3])
    n = cross(e[0], e[1])
    return dot(n, A[0]) ** 2, dot(n, n)


def face_slow(P, tri, widest=None):
    """(num, den, feature) of one present face by the rational method"""
    d, q = closest_point(P, tri)
    feature = feature_of(q, tri)
    num, den = formula(P, tri, feature)
    assert den > 0 and Fraction(num, den) == d
    return num, den, feature


def face_rule(P, tri, widest=None):
    """(num, den, feature) by the contract's candidate rule: the seven candidates in the order 0 to 6, one taken only if STRICTLY less than the
    best so far.  widest: a one-element list that keeps the largest product any comparison of two distances formed"""
    def less(n1, d1, n2, d2):
        a, b = n1 * d2, n2 * d1
        if widest is not None:
            widest[0] = max(widest[0], a, b)
        return a < b
    A = [sub(tuple(int(x) for x in v), tuple(int(x) for x in P)) for v in tri]
    e = [sub(A[(i + 1) % 3], A[i]) for i in range(3)]
    best = (dot(A[0], A[0]), 1, 0)
    for k in (1, 2):
        if less(dot(A[k], A[k]), 1, best[0], best[1]):
            best = (dot(A[k], A[k]), 1, k)
    for i in range(3):
        ee, s = dot(e[i], e[i]), -dot(A[i], e[i])
        if ee > 0 and 0 <= s <= ee:
            c = cross(A[i], e[i])
            if less(dot(c, c), ee, best[0], best[1]):
                best = (dot(c, c), ee, 3 + i)
    n = cross(e[0], e[1])
    nn = dot(n, n)
    if nn > 0 and all(dot(cross(A[i], e[i]), n) >= 0 for i in range(3)):
        k = dot(n, A[0])
        if less(k * k, nn, best[0], best[1]):
            best = (k * k, nn, 6)
    return best


# ---- a set -------------------------------------------------------------------------------------------------------------------------------------

def record(status, face=NO_FACE, feature=0, num=0, den=0):
    return (status, face, feature, 0, num & M64, num >> 64, den & M64, den >> 64)


def fractions_of(rec):
    """[(num, den)] of HITREC records as Python integers"""
    return [(int(r["num_lo"]) | int(r["num_hi"]) << 64, int(r["den_lo"]) | int(r["den_hi"]) << 64) for r in rec]


def in_range(p, base):
    return all(-R <= int(p[c]) - int(base[c]) < R for c in range(3))


def answer(cands, radius, flags):
    """the record of one in-range point from its present faces' [(f, num, den, feature)] (all of them, or at least every one at the least
    distance)"""
    if not cands:
        return record(MISS)
    f, num, den, feature = min(cands, key=lambda c: (Fraction(c[1], c[2]), c[0]))
    if flags & WITHIN:
        r = min(int(radius), RMAX)
        if num > r * r * den:
            return record(MISS)
        if flags & ANY:
            return record(HIT)
    return record(HIT, f, feature, num, den)


def candidates(u16, index, points, base=(0, 0, 0), nvert=None, written=True, rule=face_slow, widest=None):
    """for every point None (out of range, or written == 0) or [(f, num, den, feature)] over ALL present faces: what every flag combination's
    answer is made of.  u16: (nvert, 3) positions relative to base; index (nface, 3); points: POINT, absolute grid units; written: the
    transform record's word"""
    u16 = np.asarray(u16).astype(np.int64).reshape(-1, 3)
    idx = np.asarray(index).astype(np.int64).reshape(-1, 3)
    nvert = len(u16) if nvert is None else nvert
    present = [f for f in range(len(idx)) if (idx[f] < nvert).all()]
    tris = {f: [tuple(int(x) for x in u16[v]) for v in idx[f]] for f in present}
    out = []
    for pt in points:
        if not written or not in_range(pt["p"], base):
            out.append(None)
            continue
        P = tuple(int(pt["p"][c]) - int(base[c]) for c in range(3))
        out.append([(f,) + rule(P, tris[f], widest) for f in present])
    return out


def closest(u16, index, points, base=(0, 0, 0), flags=0, nvert=None, written=True, rule=face_slow, widest=None, cands=None):
    """the records (HITREC) of a set under `flags`; cands: candidates() of the same set, where several flag combinations share them"""
    if cands is None:
        cands = candidates(u16, index, points, base, nvert, written, rule, widest)
    out = np.zeros(len(points), HITREC)
    for k, pt in enumerate(points):
        out[k] = record(RANGE) if cands[k] is None else answer(cands[k], pt["radius"], flags)
    return out


def float_distances(P, T):
    """float64 squared distances from the points P (n, 3) to the triangles T (F, 3, 3): (n, F), closest_point's method in numpy"""
    P = np.asarray(P, np.float64)[:, None, :]
    T = np.asarray(T, np.float64)
    best = np.full((P.shape[0], len(T)), np.inf)
    for i in range(3):
        a, b = T[None, :, i, :], T[None, :, (i + 1) % 3, :]
        ab = b - a
        l = (ab * ab).sum(-1)
        t = np.clip(((P - a) * ab).sum(-1) / np.where(l > 0, l, 1.0), 0.0, 1.0)
        q = a + t[..., None] * ab
        best = np.minimum(best, ((q - P) ** 2).sum(-1))
    a = T[None, :, 0, :]
    u, v = T[None, :, 1, :] - a, T[None, :, 2, :] - a
    n = np.cross(u, v)
    nn = (n * n).sum(-1)
    w = P - a
    ok = nn > 0
    safe = np.where(ok, nn, 1.0)
    g, h = (np.cross(u, w) * n).sum(-1) / safe, (np.cross(w, v) * n).sum(-1) / safe
    slack = 1e-9                                                              # (a foot on the border is an edge's candidate as well)
    inside = ok & (g >= -slack) & (h >= -slack) & (g + h <= 1 + slack)
    return np.where(inside, np.minimum(best, (n * w).sum(-1) ** 2 / safe), best)


def candidates_fast(u16, index, points, base=(0, 0, 0), nvert=None, written=True, rule=face_slow):
    """candidates() for meshes of thousands of faces: a float64 pass over all faces, then the exact rule on every face whose float distance
    is within a relative 1e-6 (and 1e-3 grid units squared) of the point's least - the float pass errs by far less, so the exact minimum
    and every tie are among them, and answer() needs no more"""
    u16 = np.asarray(u16).astype(np.int64).reshape(-1, 3)
    idx = np.asarray(index).astype(np.int64).reshape(-1, 3)
    nvert = len(u16) if nvert is None else nvert
    present = np.flatnonzero((idx < nvert).all(axis=1))
    b = np.asarray([int(x) for x in base], np.int64)
    rel = np.asarray(points["p"], np.int64).reshape(-1, 3) - b
    out = [[] if written and in_range(p["p"], base) else None for p in points]
    if not len(present):
        return out
    T = u16[idx[present]]
    todo = [k for k in range(len(points)) if out[k] is not None]
    for lo in range(0, len(todo), 64):
        ks = todo[lo:lo + 64]
        D = float_distances(rel[ks], T)
        for row, k in zip(D, ks):
            near = np.flatnonzero(row <= row.min() * (1 + 1e-6) + 1e-3)
            P = tuple(int(x) for x in rel[k])
            out[k] = [(int(present[j]),) + rule(P, [tuple(int(x) for x in c) for c in T[j]]) for j in near]
    return out


def closest_fast(u16, index, points, base=(0, 0, 0), flags=0, nvert=None, written=True, rule=face_slow, cands=None):
    """closest() on candidates_fast()"""
    return closest(u16, index, points, base, flags, cands=candidates_fast(u16, index, points, base, nvert, written, rule) if cands is None else cands)


def quantize(position):
    """integer positions (nvert, 3) -> (base (3,), uint16 (nvert, 3)) as CRTHIP_BIND_QUANTIZED stores them: base the minimum a component"""
    pos = np.asarray(position, np.int64).reshape(-1, 3)
    base = pos.min(axis=0) if len(pos) else np.zeros(3, np.int64)
    rel = pos - base
    assert rel.max(initial=0) <= 65535
    return base, rel.astype(np.uint16)


# ---- point generators (all in absolute grid units) ---------------------------------------------------------------------------------------------

def points(p, radius=0):
    p = np.asarray(p, np.int64).reshape(-1, 3)
    out = np.zeros(len(p), POINT)
    out["p"], out["radius"] = p, radius
    return out


def present_faces(position, index):
    return np.flatnonzero((np.asarray(index).astype(np.int64) < len(position)).all(axis=1))


def on_vertices(position, vs, radius=0):
    """the vertices themselves: distance 0 to every face around one, so the least id among them wins"""
    return points(np.asarray(position, np.int64)[list(vs)], radius)


def edge_midpoints(position, index, fs, radius=1):
    """the midpoint of every edge of the faces fs, rounded down a component: on the edge where the corners' sums are even, beside it else"""
    pos = np.asarray(position, np.int64)
    return points([(pos[int(index[f][k])] + pos[int(index[f][(k + 1) % 3])]) // 2 for f in fs for k in range(3)], radius)


def off_centroids(position, index, fs, heights=(0, 3, -40), radius=50):
    """for each face of fs its centroid, rounded down, moved along the face's normal by each of `heights` grid units (rounded): above the
    interior of the face where the face is not a sliver"""
    pos = np.asarray(position, np.int64)
    out = []
    for f in fs:
        a, b, c = (pos[int(v)] for v in index[f])
        n = np.cross(b - a, c - a).astype(np.float64)
        l = np.linalg.norm(n)
        for h in heights:
            out.append((a + b + c) // 3 + (np.rint(n / l * h).astype(np.int64) if l > 0 else 0))
    return points(out, radius)


def beside(position, index, r):
    """the point r grid units beyond the mesh's +x side, level with its vertex of greatest x (the first such among the present faces'
    corners): every other point of the mesh has a lower x, or the same x and another y or z, so the nearest is that vertex at exactly r - a
    corner, num/den == r^2 - and
    three copies: radius r (within, inclusive), r - 1 (not), and 0"""
    pos = np.asarray(position, np.int64)
    used = np.unique(np.asarray(index).astype(np.int64)[present_faces(position, index)])
    v = used[np.argmax(pos[used][:, 0])]
    return points([pos[v] + (r, 0, 0)] * 3, [r, r - 1, 0])


def range_corners(base, radius=RMAX):
    b = np.asarray([int(x) for x in base], np.int64)
    return points([b + (x, y, z) for x in (-R, R - 1) for y in (-R, R - 1) for z in (-R, R - 1)], radius)


def random_points(position, n, seed=0, margin=40, radius=30):
    """n points in the mesh's box grown by `margin`, radii 0 .. radius"""
    pos = np.asarray(position, np.int64)
    rng = np.random.default_rng(seed)
    out = points(rng.integers(pos.min(axis=0) - margin, pos.max(axis=0) + margin + 1, (n, 3)))
    out["radius"] = rng.integers(0, radius + 1, n)
    return out


def out_of_range(pts, base, every=7):
    """a copy with every `every`-th point moved just beyond the range on one axis"""
    out = pts.copy()
    for j, k in enumerate(range(every - 1, len(out), every)):
        c = j % 3
        out["p"][k][c] = int(base[c]) + (R if j % 2 else -R - 1)
    return out


def probes(position, index, f):
    """fourteen points about face f, on either side of its plane: off the centroid, beyond each corner and beyond each edge's midpoint, away
    from the centroid - by a tenth of the face's shortest edge, three grid units at the least (none for a face without a normal)"""
    pos = np.asarray(position, np.float64)
    V = [pos[int(v)] for v in index[f]]
    n = np.cross(V[1] - V[0], V[2] - V[0])
    if not n.any():
        return points([])
    n /= np.linalg.norm(n)
    g = (V[0] + V[1] + V[2]) / 3
    step = max(3.0, 0.1 * min(np.linalg.norm(V[(k + 1) % 3] - V[k]) for k in range(3)))
    out = []
    for s in (step, -step):
        out.append(g + s * n)
        for k in range(3):
            m = (V[k] + V[(k + 1) % 3]) / 2
            out.append(V[k] + (V[k] - g) / np.linalg.norm(V[k] - g) * step + s * n)
            out.append(m + (m - g) / np.linalg.norm(m - g) * step + s * n)
    return points(np.rint(out).astype(np.int64), int(2 * step))


def feature_cover(position, index, seed=0):
    """seven points whose answers - the MODEL's, on this mesh with the base at the minimum - carry the feature codes 0 to 6 in that order:
    probes() of one face after another until every code has been seen.  Which code a point gets depends on the nearest face's corner order
    and, at a tie, on the least id (over a shared edge both faces are equally near), so the points are chosen by the answer they are to
    have, and the faces with an edge of their own - no other face has it - come first, those whose edge ab it is before the others"""
    base, u16 = quantize(position)
    rng = np.random.default_rng(seed)
    fs = rng.permutation(present_faces(position, index))
    idx = np.asarray(index).astype(np.int64)[fs]
    key = np.stack([np.minimum(idx, np.roll(idx, -1, axis=1)), np.maximum(idx, np.roll(idx, -1, axis=1))], axis=2)      # (n, edge, 2)
    _, inverse, counts = np.unique(key.reshape(-1, 2), axis=0, return_inverse=True, return_counts=True)
    own = (counts[inverse.reshape(-1)] == 1).reshape(-1, 3)
    found = {}
    for f in fs[np.argsort(-(2 * own[:, 0] + own.any(axis=1)), kind="stable")]:
        pts = probes(position, index, f)
        rec = closest_fast(u16, index, pts, base=base) if len(pts) else []
        for p, r in zip(pts, rec):
            if r["status"] == HIT:
                found.setdefault(int(r["feature"]), p)
        if len(found) == 7:
            break
    assert len(found) == 7, sorted(found)
    return np.array([found[k] for k in range(7)], POINT)


def mixed(position, index, n=40, seed=0, some=10):
    """every generator on one mesh"""
    pos = np.asarray(position, np.int64)
    base = pos.min(axis=0)
    rng = np.random.default_rng(seed)
    fs = present_faces(position, index)
    used = np.unique(np.asarray(index).astype(np.int64)[fs])
    vs = rng.choice(used, min(len(used), some), replace=False)
    fs = rng.choice(fs, min(len(fs), some), replace=False)
    return np.concatenate([on_vertices(pos, vs), edge_midpoints(pos, index, fs[:4]), off_centroids(pos, index, fs), beside(pos, index, 17),
                           range_corners(base), out_of_range(random_points(pos, n, seed=seed), base)])
